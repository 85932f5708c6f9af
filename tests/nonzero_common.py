"""Case builders and the numpy / scipy oracle of the nonzero crop (csrc/nonzero.hip, the hole filling of csrc/components.hip;
data.nonzero_mask, data.normalize_masked, infer.fill_holes, SpacedScan / MultiScan(crop=, intensity='zscore_nonzero')).
numpy + scipy only: shared by tests/test_nonzero.py (CPU) and tests/test_gpu_nonzero.py."""
import struct

import numpy as np
from scipy import ndimage

TILE = (8, 16, 32)                                   # the labeller's tile (CC_TH, CC_TW, CC_TD of csrc/components.hip)
SHAPES = [(5, 4, 3), (37, 29, 23), (33, 17, 40), (96, 96, 40)]      # tiny; ragged against the tiles; every axis crosses a tile face; many workgroups


def structure(connectivity):
    return ndimage.generate_binary_structure(3, connectivity)


def fill(mask, connectivity=1):
    """scipy's answer: bool, the shape of mask"""
    return ndimage.binary_fill_holes(np.asarray(mask) != 0, structure(connectivity))


def _linked(shape, step):
    """a one-voxel cavity inside a solid block that reaches the outside only through diagonal steps along `step` (two axes: across
    edges; three: across corners).  Per axis the cavity sits one voxel past the first tile face where the axis is long enough, so the
    chain crosses the tile there.  The block is h >= t - 2, everything before it is background."""
    t = [TILE[a] if shape[a] >= TILE[a] + 4 else 3 for a in range(3)]
    m = np.zeros(shape, bool)
    m[t[0] - 2:] = True
    p = np.array([t[0] + 1, t[1] + 1, t[2] + 1])
    for k in range(4):
        m[tuple(p - k * np.array(step))] = False
    return m


def hole_cases(shape):
    """name -> bool mask [H, W, D]; the structured cases need room and are left out of the tiny shape"""
    rs = np.random.RandomState(sum(shape))
    H, W, D = shape
    cases = {'random50': rs.rand(*shape) < 0.5, 'random85': rs.rand(*shape) < 0.85, 'empty': np.zeros(shape, bool),
             'full': np.ones(shape, bool)}
    if min(shape) < 12:
        return cases
    shell = np.zeros(shape, bool)
    shell[1:-1, 1:-1, 1:-1] = True
    shell[4:-4, 4:-4, 4:-4] = False                  # the cavity: several tiles wide
    cases['shell'] = shell
    channel = shell.copy()
    channel[:4, W // 2, D // 2] = False              # one voxel wide, from the face h = 0 into the cavity
    cases['shell_channel'] = channel
    nested = shell.copy()
    nested[6:-6, 6:-6, 6:-6] = True                  # a mask inside the cavity ...
    nested[H // 2, W // 2, D // 2] = False           # ... with a hole of its own
    cases['nested'] = nested
    cases['edge_link'] = _linked(shape, (1, 1, 0))   # filled at connectivity 1, open at 2 and 3
    cases['corner_link'] = _linked(shape, (1, 1, 1))  # filled at 1 and 2, open at 3
    ends = np.ones(shape, bool)                      # the last voxel of each of the six faces (four distinct corners) and the first
    for c in ((0, W - 1, D - 1), (H - 1, W - 1, D - 1), (H - 1, 0, D - 1), (H - 1, W - 1, 0), (0, 0, 0)):
        inward = np.array([1 if v == 0 else -1 for v in c])
        for k in range(3):                           # the corner voxel and two more down the diagonal: open only at connectivity 3
            ends[tuple(np.array(c) + k * inward)] = False
    cases['face_ends'] = ends
    return cases


def scaled_nonzero(vol, slope=1.0, inter=0.0):
    """fmaf(v, slope, inter) != 0 of float32 operands, taken in float64: the product of two float32 is exact there, and the sum
    is zero only when it is exactly zero (the cases stay clear of results that underflow float32).  A NaN is nonzero."""
    v = np.asarray(vol).astype(np.float64)
    return (v * np.float64(np.float32(slope)) + np.float64(np.float32(inter))) != 0


def union_nonzero(vols, scalings=None):
    scalings = [(1.0, 0.0)] * len(vols) if scalings is None else scalings
    m = np.zeros(np.asarray(vols[0]).shape, bool)
    for v, (slope, inter) in zip(vols, scalings):
        m |= scaled_nonzero(v, slope, inter)
    return m


def box_of(mask):
    """((lo, hi exclusive) per axis, count) of a non-empty mask"""
    idx = np.nonzero(mask)
    return tuple((int(i.min()), int(i.max()) + 1) for i in idx), int(np.count_nonzero(mask))


def box_slices(box):
    return tuple(slice(lo, hi) for lo, hi in box)


def oracle(vols, scalings=None):
    """crop, then fill, then the masked z-score in float64: {'mask', 'box', 'count', 'means', 'stds', 'z'}; z[c] is the box of
    channel c, (v * slope + inter - mean) / max(std, 1e-8) inside the mask, 0 outside"""
    scalings = [(1.0, 0.0)] * len(vols) if scalings is None else scalings
    mask = fill(union_nonzero(vols, scalings), 1)
    box, count = box_of(mask)
    sl = box_slices(box)
    means, stds, z = [], [], []
    for v, (slope, inter) in zip(vols, scalings):
        y = np.asarray(v).astype(np.float64) * slope + inter
        mean, std = float(y[mask].mean()), float(y[mask].std())
        means.append(mean)
        stds.append(std)
        z.append(np.where(mask, (y - mean) / max(std, 1e-8), 0.0)[sl])
    return {'mask': mask, 'box': box, 'count': count, 'means': means, 'stds': stds, 'z': z}


def head_phantom(shape, seed=5, kinds=('i2', 'f4')):
    """a skull-stripped head as stored, [Z][Y][X]: an off-centre ellipsoid of tissue in exact zeros (about 85 % of the voxels), a
    zero-valued cavity inside it (every channel: a hole of the mask), and in every channel a sprinkle of exact zeros of its own (the
    union over the channels matters).  kinds: 'i2' an int16 channel around 600 +- 150, 'f4' a float32 one around 1.5 +- 0.4, 'u1' a
    uint8 one around 120 +- 30.  Returns (volumes, label u8 with classes 1 and 2 inside the head)."""
    rs = np.random.RandomState(seed)
    Z, Y, X = shape
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    c = np.array([0.55 * Z, 0.45 * Y, 0.6 * X])
    r = np.array([0.3 * Z, 0.33 * Y, 0.27 * X])
    d2 = ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2
    head, cavity = d2 <= 1.0, d2 <= 0.05
    vols = []
    for kind in kinds:
        if kind == 'i2':
            v = np.clip(np.rint(rs.normal(600.0, 150.0, shape)), 1, 4000).astype(np.int16)
        elif kind == 'u1':
            v = np.clip(np.rint(rs.normal(120.0, 30.0, shape)), 1, 255).astype(np.uint8)
        else:
            v = np.maximum(rs.normal(1.5, 0.4, shape), 0.01).astype(np.float32)
        v[~head | cavity] = 0
        v[head & (rs.rand(*shape) < 0.02)] = 0
        vols.append(v)
    lab = np.zeros(shape, np.uint8)
    lab[head & (d2 <= 0.5) & ~cavity] = 1
    lab[head & (d2 <= 0.2) & ~cavity] = 2
    return vols, lab


def save_i16(nifti, path, vol_zyx, affine, inter=0.0):
    """nifti.save writes float32: its header is kept, the datatype, the intercept and the voxels are replaced by int16 ones"""
    nifti.save(path, vol_zyx.astype(np.float32), affine)
    with open(path, 'rb') as f:
        hdr = bytearray(f.read()[:352])
    struct.pack_into('<2h', hdr, 70, 4, 16)
    struct.pack_into('<2f', hdr, 112, 1.0, inter)
    with open(path, 'wb') as f:
        f.write(bytes(hdr) + vol_zyx.astype('<i2').tobytes())
