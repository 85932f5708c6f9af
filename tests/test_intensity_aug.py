"""Host side of the contrast, gamma and low-resolution augmentations (lintransunet_amd/data.py: lowres_tables, the new
Augmentation draws, Augmentation.nnunet), the oracles of tests/intensity_aug_common.py against torch's own interpolation, and the
C-ABI refusals of csrc/intensity_aug.hip, which are decided before any launch (the library loads without a GPU)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data  # noqa: E402
from tests import intensity_aug_common as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_ALIGN, E_ARG = -2, -3, -4
SIZES = [(8, 8, 8), (16, 12, 7), (33, 20, 9), (48, 40, 24), (17, 31, 5)]
SCALES = [0.5, 0.75, 1.0] + [float(s) for s in np.random.RandomState(11).uniform(0.5, 1.0, 12)]
NAMES = ['ltu_patch_stats_parts_elems', 'ltu_patch_stats', 'ltu_intensity_apply', 'ltu_intensity_rescale', 'ltu_lowres_gather']


def _low_sizes(size, scale, axes=(0, 1, 2)):
    return tuple(max(int(round(S * scale)), 1) if a in axes else S for a, S in enumerate(size))


@pytest.mark.parametrize('size', SIZES)
def test_lowres_oracle_equals_torch_nearest_exact_then_trilinear(size):
    x = torch.from_numpy(np.random.RandomState(sum(size)).standard_normal(size))[None, None]
    worst = 0.0
    for scale in SCALES:
        for axes in ((0, 1, 2), (0, 1)):
            low = F.interpolate(x, size=_low_sizes(size, scale, axes), mode='nearest-exact')
            ref = F.interpolate(low, size=size, mode='trilinear', align_corners=False)[0, 0].numpy()
            got = C.lowres(x[0, 0].numpy(), scale, axes)
            assert got.dtype == np.float64
            worst = max(worst, float(np.abs(got - ref).max()))
    print(f'{size}: worst deviation from F.interpolate over {2 * len(SCALES)} cases {worst:.2e}')
    assert worst <= 1e-12, worst


def test_integer_nearest_exact_rule_matches_torch_indices():
    for S in range(4, 200):
        src = torch.arange(S, dtype=torch.float64)[None, None]
        for Sl in range(S // 2, S + 1):
            ref = F.interpolate(src, size=Sl, mode='nearest-exact')[0, 0].numpy().astype(np.int64)
            j = np.arange(Sl)
            assert np.array_equal(np.minimum(((2 * j + 1) * S) // (2 * Sl), S - 1), ref), (S, Sl)


@pytest.mark.parametrize('size', SIZES)
def test_lowres_tables_equal_the_oracle(size):
    for scale in SCALES:
        for axes in ((0, 1, 2), (0, 1), (2,), ()):
            idx, lam = data.lowres_tables(size, scale, axes)
            ridx, rlam = C.lowres_tables(size, scale, axes)
            assert idx.dtype == np.int32 and lam.dtype == np.float32 and idx.shape == (2, sum(size)) and lam.shape == (sum(size),)
            assert np.array_equal(idx, ridx) and np.array_equal(lam, rlam), (scale, axes)
            # an axis left out of `axes`, and every axis at scale 1, is the identity
            off = 0
            for a, S in enumerate(size):
                if a not in axes or scale == 1.0:
                    assert np.array_equal(idx[0, off:off + S], np.arange(S)) and not lam[off:off + S].any()
                off += S
    for bad in (0.0, -0.5, 1.0001, float('nan')):
        with pytest.raises(ValueError):
            data.lowres_tables(size, bad)
    with pytest.raises(ValueError):
        data.lowres_tables(size, 0.5, axes=(0, 3))


# Augmentation().draw(np.random.RandomState(20261020)) and the generator's next randint(1 << 30), recorded from the commit before the
# new draws existed
PARENT_DRAW = {'rotate': True, 'angles': [0.0, 0.0, 0.09361421783396118], 'zoom': False, 'zoom_factor': 1.2666566629734561,
               'noise': False, 'noise_std': 0.007931501538114684, 'seed': 1145605502925619303, 'blur': False,
               'sigma': 0.5362567819832945, 'bright': False, 'mul': 0.8358094491061117, 'contrast': False, 'gamma': 1.1353469919882566}
PARENT_NEXT = 865151372
# the same for Augmentation(elastic_prob=0.5, elastic_grid=(4, 4, 4)) from RandomState(7), phi as its sum
PARENT_ELASTIC = {'rotate': True, 'angles': [0.0, 0.0, 1.404073122013643], 'zoom': False, 'zoom_factor': 1.0769471092873035,
                  'noise': False, 'noise_std': 0.007205113335976155, 'seed': 2475912637482972040, 'blur': False,
                  'sigma': 0.8396149980604702, 'bright': False, 'mul': 0.9404705665742692, 'contrast': True, 'gamma': 0.9305164794463948,
                  'elastic': False, 'elastic_mm': 0.853541414319662, 'phi': -1.8039697328495272}
PARENT_ELASTIC_NEXT = 631060919


def test_default_draws_are_the_parent_commits():
    rs = np.random.RandomState(20261020)
    p = data.Augmentation().draw(rs)
    assert p == PARENT_DRAW and list(p) == list(PARENT_DRAW)
    assert rs.randint(1 << 30) == PARENT_NEXT
    rs = np.random.RandomState(7)
    p = data.Augmentation(elastic_prob=0.5, elastic_grid=(4, 4, 4)).draw(rs)
    p['phi'] = float(p['phi'].sum())
    assert p == PARENT_ELASTIC and list(p) == list(PARENT_ELASTIC)
    assert rs.randint(1 << 30) == PARENT_ELASTIC_NEXT
    # retain_stats and lowres_axes make no draw
    rs = np.random.RandomState(20261020)
    assert data.Augmentation(retain_stats=True, lowres_axes=(0, 1)).draw(rs) == PARENT_DRAW and rs.randint(1 << 30) == PARENT_NEXT


def test_new_draws_follow_the_old_ones_in_order():
    new = ['scale_contrast', 'contrast_factor', 'lowres', 'lowres_scale', 'invgamma', 'invgamma_g']
    rs, rd = np.random.RandomState(20261020), np.random.RandomState(20261020)
    aug = data.Augmentation(contrast_prob=0.5, lowres_prob=0.5, invgamma_prob=0.5)
    p = aug.draw(rs)
    assert list(p) == list(PARENT_DRAW) + new
    assert {k: p[k] for k in PARENT_DRAW} == PARENT_DRAW
    data.Augmentation().draw(rd)
    assert (rd.rand() < 0.5) == p['scale_contrast'] and rd.uniform(0.75, 1.25) == p['contrast_factor']
    assert (rd.rand() < 0.5) == p['lowres'] and rd.uniform(0.5, 1.0) == p['lowres_scale']
    assert (rd.rand() < 0.5) == p['invgamma'] and rd.uniform(0.7, 1.5) == p['invgamma_g']
    assert rs.randint(1 << 30) == rd.randint(1 << 30)
    # behind the elastic draws, and a group is drawn only when its probability is > 0
    rs = np.random.RandomState(7)
    p = data.Augmentation(elastic_prob=0.5, elastic_grid=(4, 4, 4), lowres_prob=1.0).draw(rs)
    assert list(p) == list(PARENT_ELASTIC) + ['lowres', 'lowres_scale'] and bool(p['lowres'])
    assert p['gamma'] == PARENT_ELASTIC['gamma'] and float(p['phi'].sum()) == PARENT_ELASTIC['phi']
    # fire or not, the values drawn are the same
    pa = data.Augmentation(contrast_prob=1e-9, lowres_prob=1e-9, invgamma_prob=1e-9).draw(np.random.RandomState(3))
    pb = data.Augmentation(contrast_prob=1.0, lowres_prob=1.0, invgamma_prob=1.0).draw(np.random.RandomState(3))
    assert not any(pa[k] for k in new[::2]) and all(pb[k] for k in new[::2])
    assert [pa[k] for k in new[1::2]] == [pb[k] for k in new[1::2]]


def test_nnunet_defaults():
    a = data.Augmentation.nnunet()
    assert (a.rot_prob, a.zoom_prob, a.zoom_range) == (0.2, 0.2, (0.7, 1.4))
    assert (a.noise_prob, a.blur_prob, a.brightness_prob) == (0.1, 0.2, 0.15)
    assert (a.contrast_prob, a.contrast) == (0.15, (0.75, 1.25))
    assert (a.lowres_prob, a.lowres_scale, a.lowres_axes) == (0.25, (0.5, 1.0), (0, 1, 2))
    assert (a.invgamma_prob, a.invgamma) == (0.1, (0.7, 1.5))
    assert (a.gamma_prob, a.gamma) == (0.3, (0.7, 1.5))
    assert a.retain_stats is True and a.order == (3, 3, 3)
    b = data.Augmentation.nnunet(order=1, lowres_prob=0.0)
    assert b.order == (1, 1, 1) and b.lowres_prob == 0.0 and b.retain_stats is True
    d = data.Augmentation()
    assert (d.contrast_prob, d.lowres_prob, d.invgamma_prob, d.retain_stats) == (0.0, 0.0, 0.0, False)
    with pytest.raises(ValueError):
        data.Augmentation(lowres_scale=(0.5, 1.5))
    with pytest.raises(ValueError):
        data.Augmentation(lowres_axes=(0, 4))


def test_new_names_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    declared = set(re.findall(r'^(?:int|long long)\s+(ltu_\w+)\s*\(', header, flags=re.M))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in ('contrast', 'gamma_transform', 'lowres_tables', 'simulate_lowres', 'patch_stats'):
        assert callable(getattr(data, name))
    assert lib.ltu_patch_stats_parts_elems.restype is ctypes.c_longlong
    # the scratch of the statistics: one record of 4 doubles per workgroup, a count that depends on `per` alone and is capped
    q = lib.ltu_patch_stats_parts_elems
    assert q(1, 1) == 4 and q(3, 17 * 31 * 5) == 3 * 4 and q(3, 48 * 40 * 24) == 3 * 4 * 12
    assert q(2, 128 ** 3) == 2 * 4 * 256 and q(2, 1 << 30) == 2 * 4 * 256
    assert q(0, 64) == 0 and q(1, 0) == 0 and q(1, 1 << 31) == 0 and q(65536, 64) == 0


def _ptr(a):
    return a.ctypes.data


def test_stats_and_apply_refusals_before_any_launch():
    lib = _lib.load()
    X, Y, PARTS, ST, ST2 = 4096, 8192, 16384, 32768, 65536
    n, per = 3, 17 * 31 * 5
    need = lib.ltu_patch_stats_parts_elems(n, per)
    f = lib.ltu_patch_stats
    assert f(0, n, per, PARTS, need, ST, None) == E_ARG
    assert f(X, n, per, 0, need, ST, None) == E_ARG
    assert f(X, n, per, PARTS, need, 0, None) == E_ARG
    assert f(X, -1, per, PARTS, need, ST, None) == E_ARG
    assert f(X, n, per, PARTS, need - 1, ST, None) == E_ARG                # a short parts buffer
    assert f(X, n, 0, PARTS, need, ST, None) == E_SHAPE
    assert f(X, n, 1 << 31, PARTS, 1 << 20, ST, None) == E_SHAPE
    assert f(X, 65536, per, PARTS, 1 << 30, ST, None) == E_SHAPE
    assert f(X + 4, n, per, PARTS, need, ST, None) == E_ALIGN
    assert f(X, n, per, PARTS + 4, need, ST, None) == E_ALIGN
    assert f(X, n, per, PARTS, need, ST + 4, None) == E_ALIGN
    assert f(X, 0, per, PARTS, 0, ST, None) == 0                           # nothing to do

    g = lib.ltu_intensity_apply
    ops = np.array([_lib.IAUG_CONTRAST, _lib.IAUG_NONE, _lib.IAUG_GAMMA_INV], np.int32)
    par = np.array([1.2, 0.0, 0.7], np.float32)

    def call(x=X, out=Y, o=ops, p=par, st=ST, cnt=n, per_=per, parts=PARTS, cap=need, ost=ST2):
        return g(x, out, _ptr(o) if o is not None else 0, _ptr(p) if p is not None else 0, st, cnt, per_, parts, cap, ost, None)
    for kw in (dict(x=0), dict(out=0), dict(o=None), dict(p=None), dict(st=0), dict(cnt=-1), dict(cnt=_lib.INTENSITY_AUG_MAX_N + 1),
               dict(parts=0), dict(cap=need - 1)):
        assert call(**kw) == E_ARG, kw
    for bad_op in (-1, 4):
        o = ops.copy()
        o[2] = bad_op
        assert call(o=o) == E_ARG
    for bad in (np.nan, np.inf):
        p = par.copy()
        p[0] = bad
        assert call(p=p) == E_ARG
    assert call(per_=0) == E_SHAPE and call(per_=1 << 31, cap=1 << 20) == E_SHAPE
    for kw in (dict(x=X + 4), dict(out=Y + 8), dict(st=ST + 4), dict(parts=PARTS + 4), dict(ost=ST2 + 4)):
        assert call(**kw) == E_ALIGN, kw
    assert call(cnt=0) == 0

    h = lib.ltu_intensity_rescale
    on = np.array([1, 0, 1], np.uint8)
    assert h(0, _ptr(on), ST, ST2, n, per, None) == E_ARG
    assert h(Y, 0, ST, ST2, n, per, None) == E_ARG
    assert h(Y, _ptr(on), 0, ST2, n, per, None) == E_ARG
    assert h(Y, _ptr(on), ST, 0, n, per, None) == E_ARG
    assert h(Y, _ptr(on), ST, ST2, -1, per, None) == E_ARG
    assert h(Y, _ptr(on), ST, ST2, _lib.INTENSITY_AUG_MAX_N + 1, per, None) == E_ARG
    assert h(Y, _ptr(on), ST, ST2, n, 0, None) == E_SHAPE
    assert h(Y + 4, _ptr(on), ST, ST2, n, per, None) == E_ALIGN
    assert h(Y, _ptr(on), ST + 4, ST2, n, per, None) == E_ALIGN
    assert h(Y, _ptr(on), ST, ST2, 0, per, None) == 0
    assert h(Y, _ptr(np.zeros(3, np.uint8)), ST, ST2, n, per, None) == 0   # no volume asks: nothing is launched


def test_lowres_gather_refusals_before_any_launch():
    f = _lib.load().ltu_lowres_gather
    X, Y, T = 4096, 8192, 16384
    H, W, D = 17, 31, 5
    assert f(0, Y, T, 2, H, W, D, None) == E_ARG
    assert f(X, 0, T, 2, H, W, D, None) == E_ARG
    assert f(X, Y, 0, 2, H, W, D, None) == E_ARG
    assert f(X, X, T, 2, H, W, D, None) == E_ARG                           # out of place only
    assert f(X, Y, T, -1, H, W, D, None) == E_ARG
    for shape in ((0, W, D), (H, 0, D), (H, W, 0), (_lib.LOWRES_MAX_EXTENT + 1, W, D), (H, W, _lib.LOWRES_MAX_EXTENT + 1)):
        assert f(X, Y, T, 2, *shape, None) == E_SHAPE, shape
    assert f(X, Y, T, 65536, H, W, D, None) == E_SHAPE
    assert f(X + 2, Y, T, 2, H, W, D, None) == E_ALIGN
    assert f(X, Y, T + 2, 2, H, W, D, None) == E_ALIGN
    assert f(X, Y + 2, T, 2, H, W, D, None) == E_ALIGN
    assert f(X, Y, T, 0, H, W, D, None) == 0


def test_float32_evaluation_stays_near_the_float64_oracle():
    """the two evaluations of tests/intensity_aug_common.py the GPU tolerances are measured from agree to float32 rounding"""
    vols = C.volumes((16, 12, 7))
    for x in vols:
        span = max(float(np.abs(x).max()), 1.0)
        for f in (0.75, 1.25):
            assert C.tolerance(C.contrast(x, f), C.contrast(x, f, np.float32))[1] <= 1e-5 * span
        for g in (0.7, 1.5):
            for inv in (False, True):
                for keep in (False, True):
                    assert C.tolerance(C.gamma(x, g, inv, keep), C.gamma(x, g, inv, keep, np.float32))[1] <= 1e-4 * span
        assert C.tolerance(C.lowres(x, 0.73), C.lowres(x, 0.73, dtype=np.float32))[1] <= 1e-5 * span
        assert np.array_equal(C.lowres(x, 1.0, dtype=np.float32), x) and np.array_equal(C.lowres(x, 0.5, axes=(), dtype=np.float32), x)
    assert np.array_equal(C.gamma(vols[2], 1.5, True, True, np.float32), vols[2])
    # retain_stats restores mean and standard deviation
    y = C.gamma(vols[0], 1.5, True, True)
    assert abs(y.mean() - vols[0].astype(np.float64).mean()) <= 1e-12 and abs(y.std() - vols[0].astype(np.float64).std()) <= 1e-12
