"""Shared by tests/test_spline.py (no GPU) and tests/test_gpu_spline.py: the float64 oracle of the cubic B-spline path
(ltu_spline_prefilter + ltu_resample_spline), a float32 run of the same oracle that sets the tolerances, the seeded inputs and the
case table.

Everything is indexed logically: a source v[s0, s1, s2] of shape S and an output of shape O, whatever the memory layouts are.  The
oracle's coefficients are scipy.ndimage.spline_filter1d(order=3, mode='mirror') along every axis of order 3 and length > 1; its
value at c = M (p, 1), clamped to [0, S - 1], is the explicit tap sum sum_ijk w0[i] w1[j] w2[k] coef[...] with mirrored tap
indices, then the clamp to [lo, hi].  For orders (3, 3, 3) that is scipy.ndimage.map_coordinates(order=3, mode='mirror') at the
clamped coordinates (test_spline.py holds it to 4e-15).

Tolerances.  fp32 against float64 cannot be exact, so the bound is measured on the oracle, never on the kernel: the same oracle run
in float32 (scipy's filter with float32 output per axis, the tap weights and the running sum in float32) on the inputs of the
tests below, the largest absolute deviation from the float64 result taken over all of them (measure_tolerances() below; test_spline.py
checks that the constants still are what it returns), and the GPU gets 4 times that: its order of operations and its fused multiply-adds differ from scipy's.
A wrong tap, weight or boundary is an error of 1e-2 or more on these inputs."""
import functools

import numpy as np
from scipy import ndimage

from lintransunet_amd import geometry

# measure_tolerances() with scipy 1.15.3, rounded down: 2.64e-6 on coefficients up to 34.9, 2.07e-6 on values up to 4.1
COEF_F32_DEV = 2.6e-6        # float32 prefilter against float64 over PREFILTER_SHAPES x PREFILTER_ORDERS x the three stored dtypes
VALUE_F32_DEV = 2.0e-6       # float32 prefilter + tap sum against float64 over GATHER_CASES x GATHER_ORDERS
COEF_TOL = 4 * COEF_F32_DEV
VALUE_TOL = 4 * VALUE_F32_DEV

WINDOW = (-96.0, 215.0, (-96.0 - 77.99) / 75.4, (215.0 - 77.99) / 75.4)      # the driver's CT window: clips, roughly unit variance
PREFILTER_SHAPES = ((67, 5, 3), (5, 130, 3), (3, 5, 130), (2, 3, 70), (1, 66, 1), (1, 1, 1))
PREFILTER_ORDERS = ((3, 3, 3), (3, 3, 0))
GATHER_ORDERS = ((3, 3, 3), (3, 3, 0), (1, 3, 3))
MAP_COORDINATES_SHAPES = ((67, 5, 3), (2, 130, 1), (3, 2, 70), (1, 1, 1))


def taps_of(order):
    return 4 if order == 3 else order + 1


def coefficients(v, orders, dtype=np.float64):
    """B-spline coefficients of v [S0, S1, S2]: scipy's filter along every axis of order 3 and length > 1, output in dtype"""
    c = np.asarray(v, dtype=dtype)
    for a in range(3):
        if orders[a] == 3 and c.shape[a] > 1:
            c = ndimage.spline_filter1d(c, order=3, axis=a, mode='mirror', output=dtype)
    return c


def mirror(i, n):
    """whole-sample mirror of integer indices: i mod 2 (n - 1), folded; 0 when n = 1"""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m > n - 1, p - m, m)


def coords(M, O):
    """c = M (p, 1) for every output voxel, before the clamp: float64 [3, O0, O1, O2]"""
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in O], indexing='ij')
    p = np.stack(list(grids) + [np.ones(O)], 0).reshape(4, -1)
    return (np.asarray(M, dtype=np.float64) @ p).reshape(3, *O)


def clamped(c, S):
    return [np.clip(c[a], 0.0, S[a] - 1.0) for a in range(3)]


def axis_taps(u, n, order, dtype=np.float64):
    """[(index, weight)] of one source axis at the clamped coordinate u (float64); the weights are formed in dtype from t in dtype"""
    if order == 0:
        return [(np.floor(u + 0.5).astype(np.int64), np.ones(u.shape, dtype=dtype))]
    f = np.floor(u)
    i = f.astype(np.int64)
    t = (u - f).astype(dtype)
    one = dtype(1)
    if order == 1:
        return [(mirror(i, n), one - t), (mirror(i + 1, n), t)]
    w = ((one - t) ** 3 / dtype(6), (dtype(3) * t ** 3 - dtype(6) * t ** 2 + dtype(4)) / dtype(6),
         (dtype(-3) * t ** 3 + dtype(3) * t ** 2 + dtype(3) * t + one) / dtype(6), t ** 3 / dtype(6))
    return [(mirror(i - 1 + j, n), w[j]) for j in range(4)]


def gather(coef, M, O, orders, lo=-np.inf, hi=np.inf, dtype=np.float64):
    """the tap sum of coef [S0, S1, S2] at M (p, 1) for every p of O, clamped to [lo, hi]; sum and weights in dtype"""
    coef = np.asarray(coef, dtype=dtype)
    S = coef.shape
    u = clamped(coords(M, O), S)
    taps = [axis_taps(u[a], S[a], orders[a], dtype) for a in range(3)]
    acc = np.zeros(O, dtype=dtype)
    for i2, w2 in taps[2]:
        for i1, w1 in taps[1]:
            for i0, w0 in taps[0]:
                acc = acc + (w0 * w1 * w2) * coef[i0, i1, i2]
    return np.clip(acc, dtype(lo), dtype(hi))


def resample64(v, M, O, orders, lo=-np.inf, hi=np.inf):
    """the float64 oracle: mapped voxels v [S0, S1, S2] -> values on O"""
    return gather(coefficients(v, orders), M, O, orders, lo, hi)


def resample32(v, M, O, orders, lo=-np.inf, hi=np.inf):
    """the same oracle in float32 (scipy's filter with float32 output per axis, float32 weights and sum): the yardstick of VALUE_TOL"""
    return gather(coefficients(np.asarray(v, dtype=np.float32), orders, np.float32), M, O, orders, lo, hi, np.float32)


def mapped(raw, imap):
    alpha, beta, lo, hi = imap
    return np.clip(np.asarray(raw, dtype=np.float64) * alpha + beta, lo, hi)


def outside_share(M, O, S):
    """share of output voxels whose coordinate is clamped on some axis"""
    c = coords(M, O)
    out = np.zeros(O, dtype=bool)
    for a in range(3):
        out |= (c[a] < 0) | (c[a] > S[a] - 1)
    return float(out.mean())


@functools.lru_cache(maxsize=None)
def raw_scan(S, kind, seed=0):
    """a seeded stored scan, logical [S0, S1, S2]: white noise around the window so that about a tenth of the voxels clip, as
    uint8 (with slope 1.5 / intercept -200, see stored_map), int16 or float32.  Callers must not write to it."""
    rs = np.random.RandomState(1000 * seed + 7 * sum(S) + len(kind))
    hu = 60.0 + 110.0 * rs.standard_normal(S)
    if kind == 'u8':
        return np.clip(np.round((hu + 200.0) / 1.5), 0, 255).astype(np.uint8)
    if kind == 'i16':
        return np.round(hu).astype(np.int16)
    return hu.astype(np.float32)


def stored_map(kind):
    """(alpha, beta, lo, hi) of the driver's window for a stored scan of `kind`"""
    from lintransunet_amd import data
    slope, inter = (1.5, -200.0) if kind == 'u8' else (1.0, 0.0)
    return data.intensity_map(WINDOW, slope, inter)


@functools.lru_cache(maxsize=None)
def unit_volume(S, seed=0):
    """unit-variance float32 white noise, logical [S0, S1, S2]; callers must not write to it"""
    return np.random.RandomState(77 + seed).standard_normal(S).astype(np.float32)


def affine(pix, origin=(0.0, 0.0, 0.0), perm=(0, 1, 2), signs=(-1, -1, 1)):
    """file axis i -> world axis perm[i] with sign signs[i] and spacing pix[i]"""
    a = np.eye(4)
    a[:3, :3] = 0
    for i in range(3):
        a[perm[i], i] = signs[i] * pix[i]
    a[:3, 3] = origin
    return a


def _rot(axis, deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def _oblique_matrix():
    """output (70, 45, 33) -> source (37, 41, 29): output axis 2 along source axis 0, axes 0 and 1 along source axes 1 and 2, scaled,
    then 9 degrees about source axis 2 and 6 about source axis 0; the offset leaves a fifth of the output outside the source"""
    base = np.zeros((3, 3))
    base[0, 2], base[1, 0], base[2, 1] = 1.17, 0.61, 0.66
    m = np.zeros((3, 4))
    m[:, :3] = _rot(0, 6.0) @ _rot(2, 9.0) @ base
    m[:, 3] = (2.0, -2.5, -3.5)
    return m


@functools.lru_cache(maxsize=None)
def gather_cases():
    """name -> dict(S source shape, O output shape (default layout: the last axis fastest), M 3x4 pull matrix, lanes: the lane axes
    to run (None = geometry.lane_axis's choice on the coefficients' layout), transposed: per lane, whether the tile goes through LDS).
    'plan' (the pancreas scans' geometry: file x -> output H) takes the LDS path, 'slices_first' (file x -> output D) the direct one."""
    plan_aff = affine((0.7, 0.7, 2.5), (20.0, 15.0, -30.0))
    M, ras, _ = geometry.spacing_plan((50, 36, 9), plan_aff, (0.5, 0.5, 2.0))
    plan = dict(S=(50, 36, 9), O=tuple(ras), M=M, lanes=(None,), transposed=(True,))
    first_aff = affine((2.5, 0.7, 0.7), (5.0, -3.0, 7.0), perm=(2, 0, 1), signs=(1, -1, 1))
    M, ras, _ = geometry.spacing_plan((9, 50, 36), first_aff, (2.0, 0.5, 0.5))
    first = dict(S=(9, 50, 36), O=tuple(ras), M=M, lanes=(None,), transposed=(False,))
    oblique = dict(S=(37, 41, 29), O=(70, 45, 33), M=_oblique_matrix(), lanes=(0, 1, 2), transposed=(True, True, False))
    return {'oblique': oblique, 'plan': plan, 'slices_first': first}


GATHER_CASES = ('oblique', 'plan', 'slices_first')


@functools.lru_cache(maxsize=None)
def gather_reference(case, orders):
    """(float32 source [S0, S1, S2], float64 oracle values [O0, O1, O2]); computed once per process, callers must not write to them"""
    cfg = gather_cases()[case]
    v = unit_volume(cfg['S'])
    return v, resample64(v, cfg['M'], cfg['O'], orders)


def measure_tolerances():
    """(COEF_F32_DEV, largest |coefficient|, VALUE_F32_DEV, largest |value|) as measured here, on the CPU, by the float32 oracle"""
    cdev = cmax = vdev = vmax = 0.0
    for S in PREFILTER_SHAPES:
        for orders in PREFILTER_ORDERS:
            for kind in ('u8', 'i16', 'f32'):
                v = mapped(raw_scan(S, kind), stored_map(kind))
                want = coefficients(v, orders)
                got = coefficients(v.astype(np.float32), orders, np.float32)
                cdev, cmax = max(cdev, float(np.abs(got - want).max())), max(cmax, float(np.abs(want).max()))
    for case in GATHER_CASES:
        cfg = gather_cases()[case]
        for orders in GATHER_ORDERS:
            v, want = gather_reference(case, orders)
            got = resample32(v, cfg['M'], cfg['O'], orders)
            vdev, vmax = max(vdev, float(np.abs(got - want).max())), max(vmax, float(np.abs(want).max()))
    return cdev, cmax, vdev, vmax
