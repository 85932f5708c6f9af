"""Shared by tests/test_label_vote.py (no GPU) and tests/test_gpu_label_vote.py: the float64 oracle of the label vote
(ltu_resample_vote behind data.resample(label_order=1), ltu_sample_vote behind data.sample_affine(label_order=1)), written from the
rule in include/ltu_hip.h, the tie bands, and the seeded inputs.

The rule.  An output voxel has a source coordinate c.  Its 8 trilinear taps are floor(c) + (0 | 1) per axis with the weights
(1 - t | t), t = c - floor(c).  Tap r has the weight w_r (the product over the axes) and the label l_r, the u8 voxel at the tap.  The
score of a value v is the sum of w_r over the taps with l_r == v; the output is the SMALLEST v of maximal score.  Two outside rules:
  'clamp'  the scan resampler: c is clamped to [0, S - 1] first and the upper tap at the last index is that index again, so there
           is no outside;
  'zero'   the augmentation gathers: a tap outside the scan holds label 0 (the nearest path's "0 outside", the image's fill).
That is the arg-max over the classes of the linearly interpolated indicator maps ("one-hot, order 1"), nnU-Net's label resampling.

Bands.  The kernels form c and t in fp32 brackets, so where the two best scores are close the device may pick the other one.  A score
is a sum of products of t and 1 - t: its derivative along an axis is a signed sum of products of the other two axes' weights, at most
1 in magnitude, so a score moves by at most the coordinate's change per axis, summed over 3 axes, and the margin (top score minus
second score) by twice that.
  affine, resampler  include/ltu_hip.h states the affine gather's fp32 bracket to be within ~2e-5 voxel of fp64 (the resampler's
           coordinate is fp64 and only t is rounded to fp32: far inside that): 2 * 3 * 2e-5 = 1.2e-4, and BAND = 2e-4 leaves 8e-5
           for the fp32 rounding of the weights and of the score sums (8 weights of 2 roundings and 7 adds of values <= 1: about
           23 * 6e-8 = 1.4e-6 per score).
  elastic  the deformation's M[:, :3] u joins the bracket, "at most 64 |M| more on a bracket of at most 256 |M|" (csrc/augment.hip):
           the bracket's share grows to 2e-5 * (256 + 64) / 256 = 2.5e-5, and u itself is an fp32 sum of three contractions of 4
           terms, about 20 ulp of the largest |u| here (3.1 voxels, ulp 2.4e-7): 5e-6 voxel, times the largest absolute row sum of
           M[:, :3] (the derivation tests/sample_spline_common.py::deformed_bound makes for the cubic gather).  band_elastic(M) =
           6 * (2.5e-5 + 5e-6 * rowsum) + 8e-5, the same rounding allowance: 2.9e-4 at a row sum of 2.
Voxels whose float64 margin is below the band are skipped.  Conditions, not measurements: a case may skip at most MAX_SKIP of its
voxels and must differ from the nearest label in at least MIN_DIFF of them (a kernel that falls back to nearest fails)."""
import functools
import itertools

import numpy as np

BAND = 2e-4
ROUNDING = BAND - 2 * 3 * 2e-5
MAX_SKIP = 0.005
MIN_DIFF = 0.005


def band_elastic(M):
    row = float(np.abs(np.asarray(M, dtype=np.float64).reshape(3, 4)[:, :3]).sum(1).max())
    return 6 * (2e-5 * (256 + 64) / 256 + 5e-6 * row) + ROUNDING


def grid_coords(M, shape):
    """c = M (p, 1) in float64 for every voxel p of `shape`: [3, *shape]"""
    M = np.asarray(M, dtype=np.float64).reshape(3, 4)
    p = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij'), 0)
    return np.einsum('sa,axyz->sxyz', M[:, :3], p) + M[:, 3].reshape(3, 1, 1, 1)


def vote(label, c, outside):
    """(voted labels u8, margin float64, nearest labels u8) of the u8 volume `label` at coordinates c [3, ...] in ITS axes, under
    the outside rule 'clamp' or 'zero'.  margin: top score minus second score over all values (an absent value scores 0).  nearest:
    the voxel at the round-half-even coordinate (of the clamped coordinate under 'clamp'; 0 outside under 'zero')."""
    assert outside in ('clamp', 'zero')
    label = np.asarray(label)
    assert label.dtype == np.uint8 and label.ndim == 3
    S = label.shape
    c = np.asarray(c, dtype=np.float64)
    if outside == 'clamp':
        c = np.stack([np.clip(c[a], 0.0, S[a] - 1.0) for a in range(3)])
    f = np.floor(c)
    t = c - f
    i0 = f.astype(np.int64)
    values = np.union1d(np.unique(label), [0]).astype(np.int64)
    scores = np.zeros((len(values),) + c.shape[1:], dtype=np.float64)
    for bits in itertools.product((0, 1), repeat=3):
        w = np.ones(c.shape[1:], dtype=np.float64)
        idx, ins = [], np.ones(c.shape[1:], dtype=bool)
        for a in range(3):
            w = w * (t[a] if bits[a] else 1.0 - t[a])
            i = i0[a] + bits[a]
            if outside == 'clamp':
                i = np.minimum(i, S[a] - 1)
            ins &= (i >= 0) & (i < S[a])
            idx.append(np.clip(i, 0, S[a] - 1))
        l = np.where(ins, label[idx[0], idx[1], idx[2]], 0).astype(np.int64)
        for n, v in enumerate(values):
            scores[n] += np.where(l == v, w, 0.0)
    order = np.sort(scores, axis=0)
    margin = order[-1] - order[-2] if len(values) > 1 else np.full(c.shape[1:], np.inf)
    voted = values[np.argmax(scores, axis=0)].astype(np.uint8)            # the first maximum: the smallest value
    r = np.rint(c).astype(np.int64)
    ins = np.ones(c.shape[1:], dtype=bool)
    for a in range(3):
        ins &= (r[a] >= 0) & (r[a] < S[a])
    rc = [np.clip(r[a], 0, S[a] - 1) for a in range(3)]
    nearest = np.where(ins, label[rc[0], rc[1], rc[2]], 0).astype(np.uint8)
    return voted, margin, nearest


# ---- the ball: a ball of radius 5.3 voxels rasterised on 16^3, brought to 37^3 (factor 2.37) ---------------------------------------
BALL_COARSE, BALL_FINE, BALL_FACTOR = (16, 16, 16), (37, 37, 37), 2.37
BALL_CENTRE, BALL_RADIUS = (7.3, 7.9, 7.6), 5.3


def ball_matrix():
    """fine voxel -> coarse voxel, voxel centres aligned as a resampling does: c = (p + 1/2) / factor - 1/2"""
    M = np.zeros((3, 4))
    M[:, :3] = np.eye(3) / BALL_FACTOR
    M[:, 3] = 0.5 / BALL_FACTOR - 0.5
    return M


def _ball(c):
    d2 = sum((c[a] - BALL_CENTRE[a]) ** 2 for a in range(3))
    return (d2 <= BALL_RADIUS ** 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def ball():
    """(coarse ball u8 [16]^3, the ball rasterised directly on the fine grid u8 [37]^3, the fine grid's coarse coordinates);
    callers must not write to them"""
    coarse = _ball(np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in BALL_COARSE], indexing='ij'), 0))
    c = grid_coords(ball_matrix(), BALL_FINE)
    return coarse, _ball(c), c


# ---- the blob label: smoothed noise thresholded into 4 values -----------------------------------------------------------------------
BLOB_SCAN = (24, 20, 12)


@functools.lru_cache(maxsize=None)
def blob_label(shape=BLOB_SCAN, seed=0, values=(0, 1, 2, 3)):
    """u8 [shape]: white noise of RandomState(seed), box-smoothed three times along every axis (reflecting ends), cut at its
    quantiles into len(values) equally filled `values` (4 by default); callers must not write to it"""
    v = np.random.RandomState(seed).standard_normal(shape)
    for _ in range(3):
        for a in range(3):
            p = np.pad(v, [(1, 1) if b == a else (0, 0) for b in range(3)], mode='symmetric')
            sl = [slice(None)] * 3
            acc = np.zeros_like(v)
            for o in range(3):
                sl[a] = slice(o, o + shape[a])
                acc += p[tuple(sl)]
            v = acc / 3.0
    q = np.quantile(v, np.arange(1, len(values)) / len(values))
    return np.asarray(values, dtype=np.uint8)[np.digitize(v, q)]


# ---- the gather cases: patches of the blob label through data.patch_matrix ----------------------------------------------------------
SIZES = {'vec': (20, 18, 8), 'scalar': (17, 15, 5)}            # d % 4 == 0 takes 4 voxels per lane and the vector store
# name -> (start, flip, k, angles about H, W, D, zoom).  'rotd' and 'zoom' are z-decoupled matrices; 'zoom' (0.45: the patch covers
# 2.2 x its extent of the scan, from a fractional start) reaches past the scan on every side, so taps outside count for label 0
PATCHES = {
    'rotd': ((2, 1, 2), False, 0, (0.0, 0.0, 0.4), 1.2),
    'oblique': ((3, 2, 1), True, 0, (0.25, -0.2, 0.6), 0.8),
    'zoom': ((1.3, 0.4, 0.8), False, 0, (0.0, 0.0, 0.0), 0.45),
}
CALLS = {'zdec': ('rotd', 'zoom'), 'general': ('rotd', 'oblique', 'zoom')}      # the kernel variant is chosen from the whole call
LATTICES = {'vec': ((4, 4, 4), (4, 4, 6)), 'scalar': ((4, 4, 4),)}            # (4, 4, 6) at d = 8: a run of 4 voxels spans three cells
ELASTIC_CELLS = 0.15                                                           # amplitude in lattice cells (0.4 is where folding begins)


def patch_mats(names, size):
    from lintransunet_amd import data
    return np.stack([data.patch_matrix(PATCHES[n][0], size, *PATCHES[n][1:]) for n in names])


def lattices(size, grid, n):
    """[n, 3, *grid] float32: RandomState(5).uniform(-1, 1) times ELASTIC_CELLS lattice cells per patch axis"""
    cell = np.array([(size[a] - 1) / (grid[a] - 3) for a in range(3)]).reshape(1, 3, 1, 1, 1)
    return (np.random.RandomState(5).uniform(-1, 1, (n, 3, *grid)) * ELASTIC_CELLS * cell).astype(np.float32)


def patch_coords(M, size, phi=None):
    """c = M (p + u(p), 1) in float64, u = data.elastic_displacement: [3, h, w, d]"""
    from lintransunet_amd import data
    p = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in size], indexing='ij'), 0)
    if phi is not None:
        p = p + data.elastic_displacement(phi, size)
    M = np.asarray(M, dtype=np.float64).reshape(3, 4)
    return np.einsum('sa,axyz->sxyz', M[:, :3], p) + M[:, 3].reshape(3, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def gather_reference(call, size_name, grid=None):
    """[(name, voted, comparable mask, nearest)] per patch of CALLS[call], deformed by lattices(size, grid, n) when grid is given;
    comparable: the float64 margin is at least the band.  Computed once per process, callers must not write to it."""
    size, names = SIZES[size_name], CALLS[call]
    mats = patch_mats(names, size)
    phi = lattices(size, grid, len(names)) if grid is not None else [None] * len(names)
    out = []
    for name, M, f in zip(names, mats, phi):
        voted, margin, nearest = vote(blob_label(), patch_coords(M, size, f), 'zero')
        out.append((name, voted, margin >= (band_elastic(M) if grid is not None else BAND), nearest))
    return out


def check_case(got, voted, keep, nearest, what):
    """the comparison every device case makes: inside both caps, equal to the oracle outside the band; prints the figures first"""
    got = np.asarray(got)
    skip, diff = 1.0 - keep.mean(), (voted != nearest).mean()
    wrong = int((got != voted)[keep].sum())
    print(f'{what}: {wrong} of {int(keep.sum())} compared voxels differ from the oracle; skipped {skip:.5f}, oracle differs from nearest in {diff:.4f},'
          f' device differs from nearest in {(got != nearest).mean():.4f}')
    assert skip <= MAX_SKIP, (what, skip)
    assert diff >= MIN_DIFF, (what, diff)
    assert wrong == 0, (what, wrong)


# ---- the resampler cases --------------------------------------------------------------------------------------------------------------
RS_SOURCE = (23, 19, 11)                                       # (S0, S1, S2), S0 fastest in the default layout [S2][S1][S0]
RS_OUTPUTS = ((70, 67, 3), (5, 70, 9))                         # cross the 64-wide tile on each axis between them
ANY_VALUES = (0, 3, 200, 255)


def resample_matrix(S, O):
    """output voxel -> source voxel: the grids' extents matched with voxel centres aligned (c = (p + 1/2) S / O - 1/2), plus a
    little shear, so that no axis is separable and the corners leave the source (the clamp acts)"""
    M = np.zeros((3, 4))
    for a in range(3):
        M[a, a] = S[a] / O[a]
        M[a, 3] = 0.5 * S[a] / O[a] - 0.5
    M[0, 1], M[1, 2], M[2, 0] = 0.03, -0.05, 0.01
    return M


@functools.lru_cache(maxsize=None)
def source_label(values):
    """u8 indexed [s0, s1, s2]: the blob label on RS_SOURCE with the given values.  The default device layout is its transpose
    [S2][S1][S0]; the layout data.to_native passes is this array itself with strides (S1 S2, S2, 1)."""
    return blob_label(RS_SOURCE, 3, tuple(values))


@functools.lru_cache(maxsize=None)
def resample_reference(values, O):
    """(voted, comparable mask, nearest) [O0, O1, O2] of source_label(values) through resample_matrix"""
    voted, margin, nearest = vote(source_label(values), grid_coords(resample_matrix(RS_SOURCE, O), O), 'clamp')
    return voted, margin >= BAND, nearest
