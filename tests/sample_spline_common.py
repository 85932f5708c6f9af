"""Shared by tests/test_sample_spline.py (no GPU) and tests/test_gpu_sample_spline.py: the float64 oracle of the cubic patch gather
(ltu_sample_spline behind data.sample_affine(order=3 / (3, 3, 1))), a float32 run of the same oracle and a coordinate perturbation
that together set the tolerances, the seeded inputs and the patch table.

The oracle.  Coordinates in float64, c = M (p + u(p), 1) with u = data.elastic_displacement (0 without a lattice).  Where every
component of c lies in [0, S - 1], ends included, the value is the explicit tap sum over scipy.ndimage.spline_filter1d(order=3,
mode='mirror') coefficients (tests/spline_common.py: taps f-1 .. f+2 per order-3 axis, f and f+1 with (1-t, t) along D at order 1,
tap indices whole-sample mirrored), then the clamp to [lo, hi]; everywhere else it is `fill`, unclamped.  For orders (3, 3, 3)
without clamp that is scipy.ndimage.map_coordinates(order=3, mode='constant', cval=fill) (test_sample_spline.py holds it to 1e-12).
A patch that is not cubic (an integer matrix, no lattice) reads the source voxel at its integer coordinate, or fill: no clamp.

Tolerances.  Measured on the oracle, never on the kernel (measure_tolerances(); test_sample_spline.py checks that the constants
still are what it returns), as the sum of two parts, each the largest over ORDERS x SIZES x the patches of CALLS['mixed']:
  arithmetic   4 x the largest deviation of the same oracle run in float32 (scipy's filter with float32 output per axis, weights and
               running sum in float32) at the same float64 coordinates; 4 because the GPU's order of operations and its fused
               multiply-adds differ from scipy's (the factor tests/spline_common.py uses);
  coordinates  the largest change of the float64 oracle when every coordinate component moves by +-COORD_BOUND (all 8 sign
               patterns): the kernel forms coordinates with an fp32 bracket that include/ltu_hip.h states to be within ~2e-5 voxel
               of fp64.  On unit-variance white noise the spline's slope reaches 3 per voxel and axis, so this part dominates.
  With a lattice the bound is wider: M[:, :3] u joins the fp32 bracket, "at most 64 |M| more on a bracket of at most 256 |M|"
  (csrc/augment.hip), so the bracket's share grows by (256 + 64) / 256, and u itself is an fp32 sum: three contractions of 4 terms
  with weights of about 6 roundings each, about 20 ulp of the largest |u| here (0.4 lattice cells of (24 - 1) / 3 voxels = 3.1,
  ulp 2.4e-7): 5e-6 voxel, times the largest absolute row sum of M[:, :3] over the patches (measure_tolerances() returns it).
Voxels whose oracle coordinate is within EDGE_BAND = 1e-3 of 0 or of S - 1 on some axis are left out of every comparison (the fp32
coordinate may fall on the other side of the hard edge there); edge_band() marks them.
A wrong tap, weight or boundary is an error of 1e-2 or more on white noise."""
import functools
import itertools

import numpy as np

from lintransunet_amd import data
from tests.spline_common import axis_taps, coefficients, unit_volume

SCAN = (29, 23, 11)
SPACING = (0.5, 0.5, 2.0)
SIZES = {'vec': (24, 24, 12), 'scalar': (20, 20, 7)}          # d % 4 == 0 takes the vector store
ORDERS = ((3, 3, 3), (3, 3, 1))
FILL = -7.5
CLAMP = (-1.5, 1.5)
GRID = (6, 6, 4)
EDGE_BAND = 1e-3
COORD_BOUND = 2e-5                                             # include/ltu_hip.h, sample_affine: "within ~2e-5 voxel of fp64"
U_F32_ERR = 5e-6                                               # the fp32 displacement, see above
# name -> (start, flip, k, angles, zoom).  'inplane' begins half a slice below the scan: its D coordinates are -0.5 .. 10.5, none of
# them on the edge 0 or 10 (an integer start would put a twelfth of the patch there)
PATCHES = {
    'oblique': ((3, -4, 2), True, 1, (0.1, -0.07, 0.3), 1.2),
    'inplane': ((4, 2, -0.5), False, 0, (0.0, 0.0, 0.5), 1.0),
    'integer': ((2, -3, 1), True, 1, (0.0, 0.0, 0.0), 1.0),
    'zoom': ((1, 0, 0), False, 0, (0.0, 0.0, 0.0), 1.3),
}
# 'mixed' is the issue's call (an oblique matrix: the general kernel), 'zdec' has z-decoupled matrices only (the other kernel)
CALLS = {'mixed': ('oblique', 'inplane', 'integer', 'zoom'), 'zdec': ('inplane', 'integer', 'zoom')}
DEFORMED = ('oblique', 'zoom')                                 # the two matrices of the deformation test

# measure_tolerances() with scipy 1.15.3, rounded down to two digits: 1.27e-6, 2.12e-4 and 3.03e-4 on values up to 3.9 before the clamp
VALUE_F32_DEV = 1.2e-6       # float32 oracle against float64, largest over the cases
COORD_DEV = 2.1e-4           # float64 oracle at coordinates moved by +-COORD_BOUND
COORD_DEV_DEFORMED = 3.0e-4  # the same at +-deformed_bound(row sum), on DEFORMED with lattices()
TOL = 4 * VALUE_F32_DEV + COORD_DEV
TOL_DEFORMED = 4 * VALUE_F32_DEV + COORD_DEV_DEFORMED


def scan_image():
    """unit-variance float32 white noise [H, W, D]; callers must not write to it"""
    return unit_volume(SCAN)


@functools.lru_cache(maxsize=None)
def scan_label():
    """a label with three values: two nested ellipsoids"""
    g = np.meshgrid(*[np.arange(n) for n in SCAN], indexing='ij')
    r = ((g[0] - 14) / 11.0) ** 2 + ((g[1] - 11) / 9.0) ** 2 + ((g[2] - 5) / 4.0) ** 2
    return (r <= 1).astype(np.uint8) + (r <= 0.3).astype(np.uint8)


def patch_mats(names, size):
    return np.stack([data.patch_matrix(PATCHES[n][0], size, *PATCHES[n][1:], SPACING) for n in names])


def is_cubic(M, phi=None):
    """sample_affine's rule: a patch is cubic unless its 12 matrix entries are integers and its lattice is absent or all zero"""
    M = np.asarray(M, dtype=np.float64)
    return bool((M != np.round(M)).any() or (phi is not None and np.any(np.asarray(phi) != 0)))


def lattices(size, n):
    """[n, 3, *GRID] float32: RandomState(11).uniform(-1, 1) times 0.4 lattice cells per axis, as tests/test_gpu_elastic.py draws"""
    rs = np.random.RandomState(11)
    cell = np.array([(size[a] - 1) / (GRID[a] - 3) for a in range(3)]).reshape(1, 3, 1, 1, 1)
    return (rs.uniform(-1, 1, (n, 3, *GRID)) * 0.4 * cell).astype(np.float32)


def coords(M, size, phi=None):
    """c = M (p + u(p), 1) in float64: [3, h, w, d]"""
    p = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in size], indexing='ij'), 0)
    if phi is not None:
        p = p + data.elastic_displacement(phi, size)
    M = np.asarray(M, dtype=np.float64)
    return np.einsum('sa,axyz->sxyz', M[:, :3], p) + M[:, 3].reshape(3, 1, 1, 1)


def inside(c, S=SCAN):
    top = (np.array(S, dtype=np.float64) - 1).reshape(3, 1, 1, 1)
    return ((c >= 0) & (c <= top)).all(0)


def edge_band(c, S=SCAN, width=EDGE_BAND):
    """voxels with a coordinate component within `width` of 0 or of S - 1"""
    top = (np.array(S, dtype=np.float64) - 1).reshape(3, 1, 1, 1)
    return ((np.abs(c) <= width) | (np.abs(c - top) <= width)).any(0)


def tap_sum(coef, c, orders, fill=FILL, clamp=None, dtype=np.float64):
    """the cubic gather of coef [H, W, D] at coordinates c [3, ...]: tap sum (weights and running sum in dtype) and clamp where c is
    inside, fill elsewhere"""
    coef = np.asarray(coef, dtype=dtype)
    S = coef.shape
    ins = inside(c, S)
    u = [np.clip(c[a], 0.0, S[a] - 1.0) for a in range(3)]
    taps = [axis_taps(u[a], S[a], orders[a], dtype) for a in range(3)]
    acc = np.zeros(c.shape[1:], dtype=dtype)
    for i0, w0 in taps[0]:
        for i1, w1 in taps[1]:
            for i2, w2 in taps[2]:
                acc = acc + (w0 * w1 * w2) * coef[i0, i1, i2]
    if clamp is not None:
        acc = np.clip(acc, dtype(clamp[0]), dtype(clamp[1]))
    return np.where(ins, acc, dtype(fill))


def source_voxels(v, c, fill=FILL):
    """a patch that is not cubic: the source voxel at its integer coordinate, fill outside"""
    i = np.round(c).astype(np.int64)
    assert np.array_equal(i, c), 'only integer coordinates stay trilinear'
    ins = inside(c, v.shape)
    i = [np.clip(i[a], 0, v.shape[a] - 1) for a in range(3)]
    return np.where(ins, np.asarray(v, dtype=np.float64)[i[0], i[1], i[2]], fill)


def oracle(v, M, size, orders, phi=None, fill=FILL, clamp=CLAMP, dtype=np.float64, shift=None):
    """(values [h, w, d], float64 coordinates) of one patch as data.sample_affine(order=orders) defines it; shift [3] moves every
    coordinate (the perturbation of measure_tolerances)"""
    c = coords(M, size, phi)
    if not is_cubic(M, phi):
        return source_voxels(v, c, fill), c
    cs = c if shift is None else c + np.asarray(shift, dtype=np.float64).reshape(3, 1, 1, 1)
    return tap_sum(coefficients(np.asarray(v, dtype=dtype), orders, dtype), cs, orders, fill, clamp, dtype), c


@functools.lru_cache(maxsize=None)
def reference(call, size_name, orders, deformed=False, clamp=CLAMP):
    """[(values float64 [h, w, d], coordinates, comparable mask)] per patch of CALLS[call] (of DEFORMED with lattices() when deformed);
    computed once per process, callers must not write to it"""
    size = SIZES[size_name]
    names = DEFORMED if deformed else CALLS[call]
    mats = patch_mats(names, size)
    phi = lattices(size, len(names)) if deformed else [None] * len(names)
    out = []
    for M, f in zip(mats, phi):
        val, c = oracle(scan_image(), M, size, orders, f, clamp=clamp)
        out.append((val, c, ~edge_band(c) if is_cubic(M, f) else np.ones(size, dtype=bool)))
    return out


def deformed_bound(M):
    """the coordinate bound of a deformed patch (module docstring): the bracket's share grown by the displacement's part of it, plus
    the fp32 error of u through the largest absolute row sum of M[:, :3]"""
    return COORD_BOUND * (256 + 64) / 256 + U_F32_ERR * float(np.abs(np.asarray(M)[:, :3]).sum(1).max())


def _coord_dev(v, M, size, orders, phi, bound):
    base, c = oracle(v, M, size, orders, phi)
    keep = ~edge_band(c)
    dev = 0.0
    for signs in itertools.product((-1.0, 1.0), repeat=3):
        moved, _ = oracle(v, M, size, orders, phi, shift=[s * bound for s in signs])
        dev = max(dev, float(np.abs(moved - base)[keep].max()))
    return dev


def measure_tolerances():
    """(VALUE_F32_DEV, COORD_DEV, COORD_DEV_DEFORMED, largest |value|, largest row sum of |M[:, :3]|) as measured here, on the CPU"""
    v = scan_image()
    fdev = cdev = ddev = vmax = row = 0.0
    for orders in ORDERS:
        for size in SIZES.values():
            names = CALLS['mixed']
            mats = patch_mats(names, size)
            phis = dict(zip(DEFORMED, lattices(size, len(DEFORMED))))
            for name, M in zip(names, mats):
                if not is_cubic(M):
                    continue
                row = max(row, float(np.abs(M[:, :3]).sum(1).max()))
                for phi in ([None, phis[name]] if name in phis else [None]):
                    want, c = oracle(v, M, size, orders, phi)
                    got, _ = oracle(v, M, size, orders, phi, dtype=np.float32)
                    fdev = max(fdev, float(np.abs(got - want).max()))
                    vmax = max(vmax, float(np.abs(want[inside(c)]).max()))
                    if phi is None:
                        cdev = max(cdev, _coord_dev(v, M, size, orders, None, COORD_BOUND))
                    else:
                        ddev = max(ddev, _coord_dev(v, M, size, orders, phi, deformed_bound(M)))
    return fdev, cdev, ddev, vmax, row
