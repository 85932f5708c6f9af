"""NIfTI-1 reading and writing with the standard library and numpy (the monai driver's LoadImaged, dataset/CT_pancreas_monai.py:40).

Scope: single-file `.nii` / `.nii.gz`, either byte order, 3-D volumes of uint8, int8, int16, uint16, int32, float32 or float64.
Refused with a `NiftiError`: NIfTI-2, `.hdr` / `.img` pairs, 4-D data, RGB and complex datatypes.  The affine follows nibabel's
`get_best_affine`: the sform if sform_code != 0, else the qform if qform_code != 0, else the base affine diag(-px, py, pz) centred on
the volume.  Voxels come back as stored (x fastest), as a numpy array [Z][Y][X] in native byte order, so an upload needs no
transpose; `scl_slope` / `scl_inter` are returned beside them, not applied (nibabel's rule: a slope of 0 or a non-finite slope means
no scaling).  nibabel is not a dependency, so parity with it is unpinned: the field layout and the affine rules are restated from
the NIfTI-1 standard and nibabel's documented behaviour.
"""
import gzip
import struct

import numpy as np

HEADER_BYTES = 348
_DTYPES = {2: np.uint8, 256: np.int8, 4: np.int16, 512: np.uint16, 8: np.int32, 16: np.float32, 64: np.float64}
_REFUSED = {32: 'complex64', 128: 'RGB24', 1792: 'complex128', 2048: 'complex256', 2304: 'RGBA32', 1: 'binary'}
# header fields copied from `like` by save(): (offset, struct format)
_COPIED = [(39, 'B'), (56, '3f'), (68, 'h'), (74, 'h'), (120, 'h'), (122, 'B'), (123, 'B'), (124, '2f'), (132, '2f'),
           (148, '80s'), (228, '24s'), (328, '16s')]


class NiftiError(ValueError):
    pass


class NiftiImage:
    """data: numpy [Z][Y][X] as stored; shape: (X, Y, Z); affine: 4x4 float64 voxel (x, y, z) -> world; pixdim: 8 floats
    (pixdim[0] = qfac); slope / inter: the intensity map nibabel applies; header: the 348 header bytes; endian: '<' or '>'."""

    def __init__(self, data, affine, pixdim, slope, inter, header, endian, qform_code, sform_code):
        self.data, self.affine, self.pixdim = data, affine, pixdim
        self.slope, self.inter = slope, inter
        self.header, self.endian = header, endian
        self.qform_code, self.sform_code = qform_code, sform_code

    @property
    def shape(self):
        return tuple(int(n) for n in self.data.shape[::-1])

    def scaled(self):
        """the voxels as nibabel's get_fdata gives them: float64 data * slope + inter ([Z][Y][X])"""
        return self.data.astype(np.float64) * self.slope + self.inter


def _read_bytes(path):
    p = str(path)
    low = p.lower()
    if low.endswith(('.hdr', '.img', '.hdr.gz', '.img.gz')):
        raise NiftiError(f'{p}: .hdr / .img pairs are not supported (single-file .nii / .nii.gz only)')
    if not low.endswith(('.nii', '.nii.gz')):
        raise NiftiError(f'{p}: not a .nii / .nii.gz file')
    opener = gzip.open if low.endswith('.gz') else open
    with opener(p, 'rb') as f:
        return f.read()


def quaternion_matrix(b, c, d):
    """rotation of the NIfTI quaternion (a, b, c, d), a = sqrt(1 - b^2 - c^2 - d^2) clamped at 0 (nibabel quat2mat)"""
    a = np.sqrt(max(1.0 - (b * b + c * c + d * d), 0.0))
    n = a * a + b * b + c * c + d * d
    if n < np.finfo(np.float64).eps:
        return np.eye(3)
    s = 2.0 / n
    X, Y, Z = b * s, c * s, d * s
    wX, wY, wZ = a * X, a * Y, a * Z
    xX, xY, xZ = b * X, b * Y, b * Z
    yY, yZ, zZ = c * Y, c * Z, d * Z
    return np.array([[1.0 - (yY + zZ), xY - wZ, xZ + wY],
                     [xY + wZ, 1.0 - (xX + zZ), yZ - wX],
                     [xZ - wY, yZ + wX, 1.0 - (xX + yY)]])


def base_affine(shape, pixdim):
    """nibabel's shape_zoom_affine(shape, zooms, x_flip=True): diag(-px, py, pz) centred on the volume"""
    z = np.array([-float(pixdim[1]), float(pixdim[2]), float(pixdim[3])])
    aff = np.eye(4)
    aff[:3, :3] = np.diag(z)
    aff[:3, 3] = -(np.asarray(shape, dtype=np.float64) - 1) / 2.0 * z
    return aff


def parse_header(hdr):
    """(fields dict, endian) of a NIfTI-1 header; raises NiftiError on NIfTI-2, a bad magic, 4-D data or a refused datatype"""
    if len(hdr) < HEADER_BYTES:
        raise NiftiError('truncated NIfTI header')
    le, be = struct.unpack('<i', hdr[:4])[0], struct.unpack('>i', hdr[:4])[0]
    if 540 in (le, be):
        raise NiftiError('NIfTI-2 files are not supported (NIfTI-1 only)')
    if le == HEADER_BYTES:
        e = '<'
    elif be == HEADER_BYTES:
        e = '>'
    else:
        raise NiftiError(f'not a NIfTI-1 header (sizeof_hdr {le})')
    magic = hdr[344:348]
    if magic == b'ni1\x00':
        raise NiftiError('.hdr / .img pairs are not supported (single-file .nii / .nii.gz only)')
    if magic != b'n+1\x00':
        raise NiftiError(f'bad NIfTI-1 magic {magic!r}')
    u = lambda off, fmt: struct.unpack_from(e + fmt, hdr, off)           # noqa: E731
    dim = u(40, '8h')
    ndim = dim[0]
    if ndim < 3 or ndim > 7:
        raise NiftiError(f'only 3-D volumes are supported (dim[0] = {ndim})')
    if any(n != 1 for n in dim[4:ndim + 1]):
        raise NiftiError(f'only 3-D volumes are supported (dim = {dim[1:ndim + 1]})')
    if min(dim[1:4]) < 1:
        raise NiftiError(f'bad dimensions {dim[1:4]}')
    datatype = u(70, 'h')[0]
    if datatype in _REFUSED:
        raise NiftiError(f'datatype {datatype} ({_REFUSED[datatype]}) is not supported')
    if datatype not in _DTYPES:
        raise NiftiError(f'datatype {datatype} is not supported')
    f = dict(dim=dim[1:4], datatype=datatype, pixdim=np.array(u(76, '8f'), dtype=np.float64), vox_offset=u(108, 'f')[0],
             scl_slope=u(112, 'f')[0], scl_inter=u(116, 'f')[0], qform_code=u(252, 'h')[0], sform_code=u(254, 'h')[0],
             quatern=u(256, '3f'), qoffset=u(268, '3f'), srow=np.array(u(280, '12f'), dtype=np.float64).reshape(3, 4))
    return f, e


def header_affine(f):
    """nibabel get_best_affine: sform, else qform, else the base affine"""
    if f['sform_code'] != 0:
        aff = np.eye(4)
        aff[:3] = f['srow']
        return aff
    if f['qform_code'] != 0:
        b, c, d = (float(np.float32(v)) for v in f['quatern'])
        vox = f['pixdim'][1:4].copy()
        if np.any(vox < 0):
            raise NiftiError('pixdim[1:4] must be positive')
        vox[2] *= -1.0 if f['pixdim'][0] < 0 else 1.0
        aff = np.eye(4)
        aff[:3, :3] = quaternion_matrix(b, c, d) @ np.diag(vox)
        aff[:3, 3] = [float(v) for v in f['qoffset']]
        return aff
    return base_affine(f['dim'], f['pixdim'])


def load(path):
    """read a .nii / .nii.gz file -> NiftiImage"""
    raw = _read_bytes(path)
    f, e = parse_header(raw)
    X, Y, Z = f['dim']
    dt = np.dtype(_DTYPES[f['datatype']]).newbyteorder(e)
    off = int(f['vox_offset'])
    if off < HEADER_BYTES:
        off = 352
    n = X * Y * Z
    if len(raw) < off + n * dt.itemsize:
        raise NiftiError(f'{path}: file holds fewer voxels than its header declares')
    data = np.frombuffer(raw, dtype=dt, count=n, offset=off).reshape(Z, Y, X).astype(dt.newbyteorder('='))
    slope, inter = float(f['scl_slope']), float(f['scl_inter'])
    if slope == 0.0 or not np.isfinite(slope):
        slope, inter = 1.0, 0.0
    if not np.isfinite(inter):
        inter = 0.0
    return NiftiImage(data, header_affine(f), f['pixdim'], slope, inter, raw[:HEADER_BYTES], e, f['qform_code'], f['sform_code'])


def _quaternion(R):
    """(b, c, d) of a proper rotation with a >= 0 (Shepperd's method)"""
    t = np.trace(R)
    if t > 0:
        s = 2.0 * np.sqrt(t + 1.0)
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = np.array([(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s])
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = np.array([(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s])
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = np.array([(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s])
    if q[0] < 0:
        q = -q
    return q[1:] / np.linalg.norm(q)


def save(path, array_zyx, affine, like=None):
    """write a uint8 (uint8 / bool input) or float32 (anything else) volume [Z][Y][X] as little-endian NIfTI-1 (.nii or .nii.gz)
    with the sform and the qform set from `affine` (nibabel's set_qform: zooms = column norms, qfac from the determinant, the
    nearest rotation by SVD).  `like` (a NiftiImage) lends its descriptive header fields and its qform / sform codes."""
    a = np.asarray(array_zyx)
    if a.ndim != 3:
        raise NiftiError(f'save writes 3-D volumes [Z][Y][X], got shape {a.shape}')
    if a.dtype in (np.uint8, np.bool_):
        a, code, bits = a.astype('<u1'), 2, 8
    else:
        a, code, bits = a.astype('<f4'), 16, 32
    aff = np.asarray(affine, dtype=np.float64)
    Z, Y, X = a.shape
    hdr = bytearray(352)
    if like is not None:
        for off, fmt in _COPIED:
            struct.pack_into('<' + fmt, hdr, off, *struct.unpack_from(like.endian + fmt, like.header, off))
    rzs = aff[:3, :3]
    zooms = np.sqrt((rzs * rzs).sum(0))
    zooms[zooms == 0] = 1.0
    R = rzs / zooms
    qfac = 1.0
    if np.linalg.det(R) < 0:
        qfac = -1.0
        R[:, 2] *= -1
    P, _, Qt = np.linalg.svd(R)
    b, c, d = _quaternion(P @ Qt)
    qcode = like.qform_code if like is not None and like.qform_code else 2
    scode = like.sform_code if like is not None and like.sform_code else 2
    struct.pack_into('<i', hdr, 0, HEADER_BYTES)
    struct.pack_into('<8h', hdr, 40, 3, X, Y, Z, 1, 1, 1, 1)
    struct.pack_into('<2h', hdr, 70, code, bits)
    struct.pack_into('<8f', hdr, 76, qfac, *zooms, 1.0, 1.0, 1.0, 1.0)
    struct.pack_into('<3f', hdr, 108, 352.0, 1.0, 0.0)
    struct.pack_into('<2h', hdr, 252, qcode, scode)
    struct.pack_into('<6f', hdr, 256, b, c, d, *aff[:3, 3])
    struct.pack_into('<12f', hdr, 280, *aff[:3].ravel())
    hdr[344:348] = b'n+1\x00'
    blob = bytes(hdr) + a.tobytes()
    p = str(path)
    if p.lower().endswith('.gz'):
        with gzip.open(p, 'wb') as f:
            f.write(blob)
    elif p.lower().endswith('.nii'):
        with open(p, 'wb') as f:
            f.write(blob)
    else:
        raise NiftiError(f'{p}: save writes .nii or .nii.gz')
