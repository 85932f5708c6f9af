"""The monai driver's data side on the host (dataset/CT_pancreas_monai.py): NIfTI-1 parsing and writing (lintransunet_amd/nifti.py),
the Spacingd + Orientationd geometry (lintransunet_amd/geometry.py), the draw order of the patch augmentations and the C-ABI
refusals of the two new entry points.  Headers are built byte by byte here with struct.pack at the NIfTI-1 offsets, not with the
project's writer."""
import gzip
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data, geometry, nifti  # noqa: E402

_CODES = {np.dtype(np.uint8): 2, np.dtype(np.int16): 4, np.dtype(np.int32): 8, np.dtype(np.float32): 16,
          np.dtype(np.float64): 64, np.dtype(np.int8): 256, np.dtype(np.uint16): 512}


def nii_bytes(data_zyx, pixdim=(1.0, 1.0, 1.0), qfac=1.0, qform_code=0, sform_code=0, quatern=(0.0, 0.0, 0.0),
              qoffset=(0.0, 0.0, 0.0), srow=None, slope=1.0, inter=0.0, endian='<', dim=None, sizeof_hdr=348, datatype=None,
              magic=b'n+1\x00'):
    """a single-file NIfTI-1 image: 348-byte header at the standard offsets, 4 extension bytes, voxels x fastest"""
    a = np.asarray(data_zyx)
    Z, Y, X = a.shape
    h = bytearray(352)
    struct.pack_into(endian + 'i', h, 0, sizeof_hdr)
    struct.pack_into(endian + '8h', h, 40, *(dim or (3, X, Y, Z, 1, 1, 1, 1)))
    code = datatype if datatype is not None else _CODES[a.dtype]
    struct.pack_into(endian + '2h', h, 70, code, a.dtype.itemsize * 8)
    struct.pack_into(endian + '8f', h, 76, qfac, *pixdim, 0.0, 0.0, 0.0, 0.0)
    struct.pack_into(endian + '3f', h, 108, 352.0, slope, inter)
    struct.pack_into(endian + '2h', h, 252, qform_code, sform_code)
    struct.pack_into(endian + '3f', h, 256, *quatern)
    struct.pack_into(endian + '3f', h, 268, *qoffset)
    sr = np.zeros((3, 4)) if srow is None else np.asarray(srow, dtype=np.float64)
    struct.pack_into(endian + '12f', h, 280, *sr.ravel())
    h[344:348] = magic
    return bytes(h) + a.astype(a.dtype.newbyteorder(endian)).tobytes()


def write_nii(path, data_zyx, **kw):
    blob = nii_bytes(data_zyx, **kw)
    opener = gzip.open if str(path).endswith('.gz') else open
    with opener(str(path), 'wb') as f:
        f.write(blob)
    return str(path)


def _vol(shape_zyx=(5, 4, 3), dtype=np.int16, seed=0):
    return np.random.RandomState(seed).randint(-100, 100, size=shape_zyx).astype(dtype)


def test_sform_wins(tmp_path):
    srow = [[-0.7, 0.1, 0.0, 12.5], [0.0, 0.8, 0.05, -3.0], [0.0, 0.0, 2.5, 40.0]]
    v = _vol()
    img = nifti.load(write_nii(tmp_path / 'a.nii', v, pixdim=(0.7, 0.8, 2.5), qform_code=1, sform_code=2, quatern=(0, 0, 1),
                               srow=srow))
    np.testing.assert_allclose(img.affine[:3], np.float32(srow), rtol=0, atol=0)
    assert img.shape == (3, 4, 5) and img.data.shape == (5, 4, 3)
    np.testing.assert_array_equal(img.data, v)


def test_qform_quaternion_001_and_qfac(tmp_path):
    v = _vol()
    img = nifti.load(write_nii(tmp_path / 'q.nii', v, pixdim=(0.7, 0.8, 2.5), qform_code=1, quatern=(0, 0, 1),
                               qoffset=(10, -20, 30)))
    want = np.diag([-0.7, -0.8, 2.5, 1.0])
    want[:3, 3] = (10, -20, 30)
    np.testing.assert_allclose(img.affine, want, atol=1e-6)
    img = nifti.load(write_nii(tmp_path / 'f.nii', v, pixdim=(0.7, 0.8, 2.5), qfac=-1.0, qform_code=1, quatern=(0, 0, 1),
                               qoffset=(10, -20, 30)))
    want[2, 2] = -2.5
    np.testing.assert_allclose(img.affine, want, atol=1e-6)


def test_qform_general_rotation(tmp_path):
    ang = np.deg2rad(5.0)                        # about x: quaternion (cos a/2, sin a/2, 0, 0)
    img = nifti.load(write_nii(tmp_path / 'r.nii', _vol(), pixdim=(1.0, 2.0, 3.0), qform_code=1,
                               quatern=(np.sin(ang / 2), 0, 0)))
    R = np.array([[1, 0, 0], [0, np.cos(ang), -np.sin(ang)], [0, np.sin(ang), np.cos(ang)]])
    np.testing.assert_allclose(img.affine[:3, :3], R @ np.diag([1.0, 2.0, 3.0]), atol=1e-6)


def test_neither_form_gives_base_affine(tmp_path):
    img = nifti.load(write_nii(tmp_path / 'n.nii', _vol(), pixdim=(0.7, 0.8, 2.5)))
    want = np.diag([-0.7, 0.8, 2.5, 1.0])
    want[:3, 3] = [0.7 * (3 - 1) / 2, -0.8 * (4 - 1) / 2, -2.5 * (5 - 1) / 2]
    np.testing.assert_allclose(img.affine, want, atol=1e-6)


@pytest.mark.parametrize('dtype', [np.uint8, np.int8, np.int16, np.uint16, np.int32, np.float32, np.float64])
def test_big_endian_and_dtypes(tmp_path, dtype):
    v = (np.arange(60).reshape(5, 4, 3) * 3 - (0 if np.dtype(dtype).kind == 'u' else 50)).astype(dtype)
    img = nifti.load(write_nii(tmp_path / 'b.nii', v, endian='>', sform_code=1, srow=[[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3]]))
    assert img.endian == '>' and img.data.dtype == np.dtype(dtype) and img.data.dtype.isnative
    np.testing.assert_array_equal(img.data, v)
    np.testing.assert_allclose(img.affine[:3, 3], [1, 2, 3])


def test_gzip_and_slope_intercept(tmp_path):
    v = _vol()
    img = nifti.load(write_nii(tmp_path / 'g.nii.gz', v, slope=2.0, inter=-1024.0))
    np.testing.assert_array_equal(img.data, v)
    assert (img.slope, img.inter) == (2.0, -1024.0)
    np.testing.assert_allclose(img.scaled(), v * 2.0 - 1024.0)
    img = nifti.load(write_nii(tmp_path / 'z.nii', v, slope=0.0, inter=5.0))         # slope 0: no scaling (nibabel)
    assert (img.slope, img.inter) == (1.0, 0.0)


def test_refusals(tmp_path):
    v = _vol()
    with pytest.raises(nifti.NiftiError, match='NIfTI-2'):
        nifti.load(write_nii(tmp_path / 'n2.nii', v, sizeof_hdr=540))
    with pytest.raises(nifti.NiftiError, match='3-D'):
        nifti.load(write_nii(tmp_path / 'd4.nii', np.zeros((2, 5, 4, 3), np.int16).reshape(10, 4, 3), dim=(4, 3, 4, 5, 2, 1, 1, 1)))
    with pytest.raises(nifti.NiftiError, match='RGB'):
        nifti.load(write_nii(tmp_path / 'rgb.nii', v, datatype=128))
    with pytest.raises(nifti.NiftiError, match='complex'):
        nifti.load(write_nii(tmp_path / 'c.nii', v, datatype=32))
    with pytest.raises(nifti.NiftiError, match='hdr'):
        nifti.load(write_nii(tmp_path / 'pair.hdr', v, magic=b'ni1\x00'))
    with pytest.raises(nifti.NiftiError, match='hdr'):
        nifti.load(write_nii(tmp_path / 'pair.nii', v, magic=b'ni1\x00'))
    # a trailing size-1 dimension is still a 3-D volume
    assert nifti.load(write_nii(tmp_path / 'd41.nii', v, dim=(4, 3, 4, 5, 1, 1, 1, 1))).shape == (3, 4, 5)


@pytest.mark.parametrize('ext', ['.nii', '.nii.gz'])
@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_writer_round_trip(tmp_path, ext, dtype):
    v = (np.random.RandomState(3).rand(7, 6, 5) * 200).astype(dtype)
    c, s = np.cos(np.deg2rad(5.0)), np.sin(np.deg2rad(5.0))
    aff = np.array([[-0.75 * c, 0.75 * s, 0, 100.5], [0.75 * s, 0.75 * c, 0, -20.25], [0, 0, -2.5, 8.0], [0, 0, 0, 1]])
    aff = aff.astype(np.float32).astype(np.float64)                                  # the header holds float32
    src = nifti.load(write_nii(tmp_path / ('src' + ext), v, pixdim=(0.75, 0.75, 2.5), sform_code=1, qform_code=1, srow=aff[:3]))
    p = tmp_path / ('out' + ext)
    nifti.save(p, v, aff, like=src)
    got = nifti.load(p)
    assert got.data.dtype == np.dtype(dtype)
    np.testing.assert_array_equal(got.data, v)
    np.testing.assert_array_equal(got.affine, aff)
    assert (got.qform_code, got.sform_code) == (1, 1)
    # the qform written beside the sform describes the same grid
    raw = open(p, 'rb').read() if ext == '.nii' else gzip.open(p, 'rb').read()
    f, _ = nifti.parse_header(raw)
    f['sform_code'] = 0
    np.testing.assert_allclose(nifti.header_affine(f), aff, atol=1e-5)


def test_worked_example_geometry():
    aff = np.diag([-0.8, -0.8, 2.5, 1.0])
    aff[:3, 3] = (200, 150, -300)
    M, shape, out = geometry.spacing_plan((512, 512, 100), aff, (0.5, 0.5, 2.0), 'RAS')
    assert shape == (819, 819, 125)
    np.testing.assert_allclose(M, [[-0.625, 0, 0, 511.25], [0, -0.625, 0, 511.25], [0, 0, 0.8, 0]], atol=1e-12)
    want = np.diag([0.5, 0.5, 2.0, 1.0])
    want[:3, 3] = (-209, -259, -300)
    np.testing.assert_allclose(out, want, atol=1e-9)
    # the plan is consistent: output voxel -> world through the output affine = through the pull matrix and the input affine
    p = np.array([[0, 0, 0, 1], [818, 818, 124, 1], [17, 400, 3, 1]], dtype=np.float64).T
    m4 = np.vstack([M, [0, 0, 0, 1]])
    np.testing.assert_allclose(out @ p, aff @ m4 @ p, atol=1e-9)


def test_shape_rounds_half_to_even():
    # ptp + 1 = 2.5, 4.5, 3.5 -> 2, 4, 4 (round half up would give 3, 5, 4)
    shape, _ = geometry.compute_shape_offset((4, 8, 6), np.eye(4), np.diag([2.0, 2.0, 2.0, 1.0]))
    assert tuple(shape) == (2, 4, 4)
    assert geometry.spacing_plan((4, 8, 6), np.eye(4), (2.0, 2.0, 2.0))[1] == (2, 4, 4)


def test_orientation_helpers():
    assert geometry.axcodes2ornt('RAS').tolist() == [[0, 1], [1, 1], [2, 1]]
    assert geometry.axcodes2ornt('LPI').tolist() == [[0, -1], [1, -1], [2, -1]]
    aff = np.array([[0, 0, -2.0, 0], [0.5, 0, 0, 0], [0, 0.5, 0, 0], [0, 0, 0, 1]])     # slices first
    assert geometry.io_orientation(aff).tolist() == [[1, 1], [2, 1], [0, -1]]
    M, shape, out = geometry.spacing_plan((10, 12, 7), aff, (1.0, 1.0, 1.0))
    # RAS axis 0 is the file's z (world x, 6 x 2.0 mm -> 13), 1 the file's x (9 x 0.5 -> 5.5 -> 6), 2 the file's y (11 x 0.5 -> 6.5 -> 6)
    assert shape == (13, 6, 6)
    assert np.all(np.diag(out)[:3] > 0)
    with pytest.raises(ValueError):
        geometry.axcodes2ornt('RAQ')


def test_pair_check():
    geometry.check_pair((4, 5, 6), np.eye(4), (4, 5, 6), np.eye(4) + 5e-4)
    with pytest.raises(ValueError, match='shapes'):
        geometry.check_pair((4, 5, 6), np.eye(4), (4, 5, 7), np.eye(4))
    with pytest.raises(ValueError, match='affines'):
        geometry.check_pair((4, 5, 6), np.eye(4), (4, 5, 6), np.eye(4) * 1.01)


def test_intensity_map_is_scale_intensity_range():
    a_min, a_max, b_min, b_max = data.MONAI_CT_WINDOW
    alpha, beta, lo, hi = data.intensity_map(data.MONAI_CT_WINDOW, slope=1.5, inter=-20.0)
    v = np.array([-1000.0, -60.0, 0.0, 77.99, 100.0, 143.0, 3000.0])
    x = v * 1.5 - 20.0
    want = np.clip((x - a_min) / (a_max - a_min) * (b_max - b_min) + b_min, b_min, b_max)
    np.testing.assert_allclose(np.clip(alpha * v + beta, lo, hi), want, atol=1e-12)
    np.testing.assert_allclose(want[2], (0.0 * 1.5 - 20.0 - 77.99) / 75.4, atol=1e-12)
    assert data.intensity_map(None, 2.0, 3.0) == (2.0, 3.0, -np.inf, np.inf)


def test_label_u8_refuses_out_of_range():
    assert data.label_u8(np.array([0, 1, 2], np.int16)).dtype == np.uint8
    with pytest.raises(ValueError):
        data.label_u8(np.array([0, 256], np.int16))
    with pytest.raises(ValueError):
        data.label_u8(np.array([0.5], np.float32))


class _Recorder(np.random.RandomState):
    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def rand(self, *a):
        self.calls.append('rand')
        return super().rand(*a)

    def randint(self, *a, **k):
        self.calls.append(('randint', a[0]))
        return super().randint(*a, **k)


def test_draw_order():
    lab = np.zeros((20, 20, 10), np.uint8)
    lab[5:12, 6:14, 2:8] = 1
    rs = _Recorder(7)
    got = [data.draw_monai_sample(lab, (8, 8, 4), rs) for _ in range(4)]
    n_fg, n_bg = int(lab.sum()), int(lab.size - lab.sum())
    calls = rs.calls
    assert len(calls) == 4 * 5
    for s in range(4):
        c = calls[5 * s:5 * s + 5]
        # crop centre (pos / neg draw, index draw), flip, rot90 k = randint(3) + 1, then the rot90 probability
        assert c[0] == 'rand' and c[1][0] == 'randint' and c[1][1] in (n_fg, n_bg)
        assert c[2] == 'rand' and c[3] == ('randint', 3) and c[4] == 'rand'
    # the same values from a plain RandomState replayed by hand
    ref = np.random.RandomState(7)
    for center, flip, k in got:
        cen = data.crop_centers(lab, (8, 8, 4), 1, rand_state=ref)[0]
        f = ref.rand() < 0.5
        kk = ref.randint(3) + 1
        r = ref.rand() < 0.5
        assert (center, flip, k) == (cen, f, kk if r else 0)


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_orient_desc_matches_numpy(flip, k):
    shapes = [(5, 5)] if k % 2 else [(5, 5), (4, 7)]
    for h, w in shapes:
        crop = np.arange(h * w).reshape(h, w)
        want = np.rot90(np.flip(crop, 0) if flip else crop, k, (0, 1))
        fh, fw, sw = data.orient_desc(flip, k)
        got = np.empty_like(want)
        for x in range(want.shape[0]):
            for y in range(want.shape[1]):
                u, v = (y, x) if sw else (x, y)
                got[x, y] = crop[h - 1 - u if fh else u, w - 1 - v if fw else v]
        np.testing.assert_array_equal(got, want)


def test_monai_schedule():
    from lintransunet_amd import optim

    class _Opt:
        param_groups = [{'lr': 1e-4}]
    s = optim.monai_schedule(_Opt())
    assert (s.factor, s.patience, s.threshold, s.cooldown, s.min_lrs) == (0.6, 4, 1e-2, 1, [1e-7])


def test_cabi_refusals_without_launch():
    """bad dtype, NULL matrix, unpaired pointers, swap_hw with h != w and a crop outside the volume are refused before launching"""
    import ctypes
    from lintransunet_amd import _lib
    lib = _lib.load()
    fake = 1 << 20                                                                # never dereferenced: every call below is refused
    rs = [fake, 0, fake, 8, 8, 8, 1, 8, 64, fake, fake, 8, 8, 8, 64, 8, 1, fake, 0, 1.0, 0.0, -1.0, 1.0, None]
    assert lib.ltu_resample_grid(*rs[:1], 7, *rs[2:]) == -1                      # LTU_E_DTYPE
    assert lib.ltu_resample_grid(*rs[:17], None, *rs[18:]) == -4                  # NULL matrix: LTU_E_ARG
    assert lib.ltu_resample_grid(*rs[:9], None, *rs[10:]) == -4                   # image source without an image output
    assert lib.ltu_resample_grid(None, 0, None, *rs[3:9], None, None, *rs[11:]) == -4
    assert lib.ltu_resample_grid(*rs[:18], 3, *rs[19:]) == -4                     # lane axis
    assert lib.ltu_resample_grid(*rs[:11], 0, *rs[12:]) == -2                     # empty output: LTU_E_SHAPE
    desc = (ctypes.c_int * 12)(0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0)
    co = [fake, fake, fake, fake, ctypes.addressof(desc), 2, 16, 16, 8, 8, 4, 4, None]
    assert lib.ltu_crop_orient(*co) == -2                                         # swap_hw with h 8 != w 4
    desc[5] = 0
    desc[6] = 9                                                                   # second patch starts at h0 = 9: 9 + 8 > 16
    assert lib.ltu_crop_orient(*co) == -2
    assert lib.ltu_crop_orient(*co[:4], None, *co[5:]) == -4
    assert lib.ltu_crop_orient(*co[:5], _lib.CROP_ORIENT_MAX + 1, *co[6:]) == -4
    desc[6] = 0
    assert lib.ltu_crop_orient(fake, fake, fake + 4, fake, *co[4:]) == -3        # d % 4 == 0: the f32 output must be 16-byte aligned
