"""Shared by tests/test_native_probs.py (no GPU) and tests/test_gpu_native_probs.py: the float64 numpy oracle of
ltu_resample_argmax (trilinear resampling of [C, ...] probabilities at c = M (p, 1) with clamped coordinates, the arg-max with the
first index winning, the top-two margin), a float32 emulation of the kernel's tap sum, the seeded inputs and the case table.

Everything is indexed logically: a source P[c, s0, s1, s2] of shape S, an output of shape O, whatever the memory layouts are.  Every
case stores its source as a contiguous [C, S0, S1, S2] array (the RAS layout: the last axis fastest) and its output with the first
axis fastest (a file's [Z][Y][X] array), so a returned tensor is compared after .permute(2, 1, 0)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from lintransunet_amd import geometry

MARGIN = 4e-6          # labels are compared where the float64 top-two margin is at least this: twice the 2e-6 bound on a value
VALUE_TOL = 2e-6       # fp32 tap sum against float64: ~11 roundings of 6e-8 on terms <= 1 give 7e-7, times 3
NEAR_TIE_CAP = 1e-3    # share of output voxels the label comparison may leave out (a condition on the inputs)


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


def _general_matrix():
    """output (70, 66, 9) -> source (23, 70, 67): output axis 2 runs along source axis 0 at 2.4 source voxels per step, axes 0 and 1
    along source axes 1 and 2 at 0.92 and 0.95, then 7 degrees about source axis 2 and 7 about source axis 0; the offset leaves 11.7 %
    of the output outside the source: below source axes 0, 1 and 2 (3.2 %, 4.2 %, 0.2 %) and above axes 0 and 2 (4.0 %, 0.7 %)"""
    base = np.zeros((3, 3))
    base[0, 2], base[1, 0], base[2, 1] = 2.4, 0.92, 0.95
    m = np.zeros((3, 4))
    m[:, :3] = _rot(0, 7.0) @ _rot(2, 7.0) @ base
    m[:, 3] = (5.5, 0.5, -1.0)
    return m


def _plan_case(shape, aff, pixdim):
    M, ras, _ = geometry.spacing_plan(shape, aff, pixdim)
    return dict(S=tuple(ras), O=tuple(shape), M=geometry.invert(M), lanes=(None,))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(S source shape, O output shape, M 3x4 pull matrix (output voxel -> source voxel), lanes: the lane axes to run
    (None = geometry.lane_axis's choice))"""
    msd = _plan_case((70, 66, 9), affine((0.8, 0.8, 2.5), (20.0, 15.0, -30.0)), (0.5, 0.5, 2.0))
    assert msd['S'] == (111, 105, 11), msd['S']
    first = _plan_case((9, 70, 66), affine((2.5, 0.8, 0.8), (5.0, -3.0, 7.0), perm=(2, 0, 1), signs=(1, -1, 1)), (2.0, 0.5, 0.5))
    assert first['S'] == (111, 105, 11), first['S']
    general = dict(S=(23, 70, 67), O=(70, 66, 9), M=_general_matrix(), lanes=(0, 1, 2))
    return {'msd': msd, 'slices_first': first, 'general': general}


CASE_NAMES = ('msd', 'slices_first', 'general')
INPUTS = ((2, 'random'), (3, 'random'), (8, 'random'), (3, 'smooth'))      # (C, kind)


def src_strides(S):
    return (S[1] * S[2], S[2], 1)


def out_strides(O):
    return (1, O[0], O[0] * O[1])


def coords(M, O):
    """c = M (p, 1) for every output voxel, before the clamp: float64 [3, O0, O1, O2]"""
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in O], indexing='ij')
    p = np.stack(list(grids) + [np.ones(O)], 0).reshape(4, -1)
    return (np.asarray(M, dtype=np.float64) @ p).reshape(3, *O)


def _taps(c, S):
    cc = [np.clip(c[s], 0.0, S[s] - 1.0) for s in range(3)]
    i0 = [np.floor(v).astype(np.int64) for v in cc]
    i1 = [i + (i < S[s] - 1) for s, i in enumerate(i0)]
    t = [v - np.floor(v) for v in cc]
    return i0, i1, t


def sample64(P, M, O):
    """float64 trilinear resampling of P [C, S0, S1, S2] -> [C, O0, O1, O2]: border padding, taps floor(c) and the next voxel"""
    P = np.asarray(P, dtype=np.float64)
    S = P.shape[1:]
    i0, i1, t = _taps(coords(M, O), S)
    out = np.zeros((P.shape[0],) + tuple(O))
    for k in range(8):
        b = (k & 1, (k >> 1) & 1, k >> 2)
        w = np.ones(O)
        for s in range(3):
            w = w * (t[s] if b[s] else 1.0 - t[s])
        out += w * P[:, (i1 if b[0] else i0)[0], (i1 if b[1] else i0)[1], (i1 if b[2] else i0)[2]]
    return out


def sample32(P, M, O):
    """the kernel's arithmetic in numpy: float64 coordinates, float32 weights t = (float)(c - floor(c)), the products and the running
    sum in float32, taps in the order k = 0 .. 7 (the fused multiply-add of the device is one rounding of the exact w v + acc; here
    the exact float64 product is added in float64 and rounded once more to float32)"""
    P = np.asarray(P, dtype=np.float32)
    S = P.shape[1:]
    i0, i1, t = _taps(coords(M, O), S)
    t = [v.astype(np.float32) for v in t]
    one = np.float32(1.0)
    acc = np.zeros((P.shape[0],) + tuple(O), dtype=np.float32)
    for k in range(8):
        b = (k & 1, (k >> 1) & 1, k >> 2)
        w = ((t[0] if b[0] else one - t[0]) * (t[1] if b[1] else one - t[1])) * (t[2] if b[2] else one - t[2])
        v = P[:, (i1 if b[0] else i0)[0], (i1 if b[1] else i0)[1], (i1 if b[2] else i0)[2]]
        acc = (w.astype(np.float64) * v.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def argmax_first(v):
    """the first maximal index along axis 0 (numpy's and torch's rule)"""
    return np.argmax(v, axis=0).astype(np.uint8)


def margin(v):
    """top value minus runner-up along axis 0"""
    s = np.sort(v, axis=0)
    return s[-1] - s[-2]


def outside_share(M, O, S):
    """share of output voxels whose coordinate is clamped on some axis"""
    c = coords(M, O)
    out = np.zeros(O, dtype=bool)
    for s in range(3):
        out |= (c[s] < 0) | (c[s] > S[s] - 1)
    return float(out.mean())


@functools.lru_cache(maxsize=None)
def make_probs(C, S, kind, seed=0):
    """softmax(2 randn) per voxel from a seeded generator, float32 [C, S0, S1, S2]; 'smooth': the logits box-filtered three times and
    rescaled to +-6 (segmentation-like)"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * C + (1 if kind == 'smooth' else 0))
    z = torch.randn((C,) + tuple(S), generator=g, dtype=torch.float64)
    if kind == 'smooth':
        for _ in range(3):
            z = F.avg_pool3d(z[None], 3, stride=1, padding=1, count_include_pad=False)[0]
        z = z * (6.0 / z.abs().max())
    else:
        z = 2.0 * z
    return torch.softmax(z, 0).to(torch.float32).contiguous()


@functools.lru_cache(maxsize=None)
def reference(case, C, kind):
    """(probabilities f32 tensor [C, S...], float64 resampled [C, O...], float64 arg-max u8 [O...], top-two margin [O...]); computed
    once per process and shared: callers must not write to them"""
    cfg = cases()[case]
    P = make_probs(C, cfg['S'], kind)
    want = sample64(P.numpy(), cfg['M'], cfg['O'])
    return P, want, argmax_first(want), margin(want)
