"""Gaussian-weighted and mirrored sliding-window inference (csrc/blend.hip, infer.sliding_window_inference(mode=, sigma_scale=,
mirror_axes=)): the importance tables against a float64 restatement of monai 0.7.0's compute_importance_map, the item order,
the refusals, and on the GPU the blend against a float64 numpy restatement of the contract, flip equivariance, determinism across
calls and window batch sizes, exact integer sums of unit tables on one-hot windows, and the real model's softmax output."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import infer as O  # noqa: E402

DEV = 'cuda'


# ---------------------------------------------------------------------------------------------- float64 restatement
def _gauss_axis(r, s):
    """monai's gaussian_1d(sigma, truncated=4.0, approx='erf') placed on a delta at r // 2 (the GaussianFilter of a one-hot
    centre), normalised to a maximum of 1"""
    sigma = r * s
    tail = int(max(sigma * 4.0, 0.5) + 0.5)
    x = np.arange(-tail, tail + 1, dtype=np.float64)
    t = 1.0 / (sigma * math.sqrt(2.0))
    ker = np.array([max(0.0, 0.5 * (math.erf(t * (v + 0.5)) - math.erf(t * (v - 0.5)))) for v in x])
    g = np.zeros(r)
    c = r // 2
    for i in range(r):
        if abs(i - c) <= tail:
            g[i] = ker[i - c + tail]
    return g / g.max()


def _ref_map(roi, mode, sigma_scale):
    """the 3-D importance map, float64: ones, or the separable Gaussian clamped to its smallest non-zero value"""
    if mode == 'constant':
        return np.ones(roi)
    sig = sigma_scale if isinstance(sigma_scale, tuple) else (sigma_scale,) * 3
    m = np.einsum('i,j,k->ijk', *[_gauss_axis(r, s) for r, s in zip(roi, sig)])
    return np.maximum(m, m[m > 0].min())


def _ref_blend(x, roi, sw, predict, overlap, mode='constant', sigma_scale=0.125, mirror_axes=()):
    """float64 restatement of the contract: x numpy [B, 1, H, W, D]; predict(window float64 [1, h, w, d], item) -> [C, h, w, d].
    Items in order (sample-major windows, mirror variants adjacent), window voxel u read from start + (r - 1 - u) on a flipped
    axis, the prediction flipped back and added with the weight of its position: out = sum w p / sum w, cropped."""
    B = x.shape[0]
    img0 = x.shape[2:]
    roi = tuple(int(r) for r in roi)
    pads = O.padding(img0, roi)
    xp = np.pad(x, [(0, 0), (0, 0)] + [tuple(p) for p in pads])
    img = xp.shape[2:]
    starts = O.patch_starts(img, roi, O.scan_interval(img, roi, overlap))
    wmap = _ref_map(roi, mode, sigma_scale)
    masks = [[a for j, a in enumerate(mirror_axes) if (m >> j) & 1] for m in range(1 << len(mirror_axes))]
    votes = wsum = None
    k = 0
    for idx in range(B * len(starts)):
        b, st = idx // len(starts), starts[idx % len(starts)]
        sl = tuple(slice(s, s + r) for s, r in zip(st, roi))
        for flips in masks:
            win = xp[b][(slice(None),) + sl]
            if flips:
                win = np.flip(win, [1 + a for a in flips])
            p = np.asarray(predict(np.ascontiguousarray(win), k), dtype=np.float64)
            if flips:
                p = np.flip(p, [1 + a for a in flips])
            if votes is None:
                votes = np.zeros((B, p.shape[0]) + img)
                wsum = np.zeros((B,) + img)
            votes[b][(slice(None),) + sl] += wmap * p
            wsum[b][sl] += wmap
            k += 1
    out = votes / wsum[:, None]
    return out[(slice(None), slice(None)) + tuple(slice(lo, lo + n) for (lo, _), n in zip(pads, img0))]


def _soft_logits(w, ramp):
    """three logits of a window [n, 1, h, w, d] (torch or numpy, any float dtype) that depend on the window-local position"""
    v = w[:, 0]
    return v, 0.5 * v + ramp, -0.7 * v + 0.3 * ramp * ramp


def _ramp(roi, lib):
    h, w, d = roi
    a = lib.arange(h) / h
    b = lib.arange(w) / w
    c = lib.arange(d) / d
    return 2.0 * a[:, None, None] - 1.5 * b[None, :, None] + c[None, None, :]


def _softmax3(l0, l1, l2, lib):
    m = lib.maximum(lib.maximum(l0, l1), l2)
    e0, e1, e2 = lib.exp(l0 - m), lib.exp(l1 - m), lib.exp(l2 - m)
    s = e0 + e1 + e2
    return e0 / s, e1 / s, e2 / s


def _soft_predictor(win):
    """a soft stand-in model on the GPU: element-wise ops only, so a window's output does not depend on its batch; it depends on
    the window-local position, so a missing flip-back changes the blend"""
    ramp = _ramp(tuple(win.shape[2:]), torch).to(win.device, torch.float32)
    p = _softmax3(*_soft_logits(win, ramp), torch)
    return torch.stack(p, 1)


def _soft_predictor_np(win, _k):
    ramp = _ramp(win.shape[1:], np).astype(np.float64)
    return np.stack(_softmax3(*_soft_logits(win[None], ramp), np), 1)[0]


def _pointwise_predictor(win):
    """flip-equivariant: depends on the voxel value only"""
    v = win[:, 0]
    return torch.stack(_softmax3(v, 2.0 * v - 0.5, -v, torch), 1)


# ---------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('roi', [(512, 512, 32), (16, 16, 8), (7, 5, 3)])
@pytest.mark.parametrize('sigma_scale', [0.125, (0.125, 0.125, 0.25)])
def test_importance_tables_match_float64(roi, sigma_scale):
    from lintransunet_amd import infer as P
    g0, g1, g2, wmin = P.importance_tables(roi, 'gaussian', sigma_scale)
    sig = sigma_scale if isinstance(sigma_scale, tuple) else (sigma_scale,) * 3
    for g, r, s in zip((g0, g1, g2), roi, sig):
        ref = _gauss_axis(r, s)
        assert g.shape == (r,)
        assert g[r // 2] == 1.0 and g.max() == 1.0
        np.testing.assert_allclose(g, ref, rtol=1e-7, atol=0)
    ref_min = np.prod([_gauss_axis(r, s)[_gauss_axis(r, s) > 0].min() for r, s in zip(roi, sig)])
    assert abs(wmin - ref_min) <= 1e-7 * ref_min
    if np.prod(roi) <= 16 * 16 * 8:                 # the 3-D map itself: its smallest non-zero value is the clamp
        m = np.einsum('i,j,k->ijk', _gauss_axis(roi[0], sig[0]), _gauss_axis(roi[1], sig[1]), _gauss_axis(roi[2], sig[2]))
        assert abs(m[m > 0].min() - wmin) <= 1e-7 * wmin
        w = np.maximum(np.einsum('i,j,k->ijk', g0, g1, g2), wmin)
        np.testing.assert_allclose(w, _ref_map(roi, 'gaussian', sigma_scale), rtol=1e-7, atol=0)


def test_importance_tables_truncated_tails_and_constant():
    """a small sigma: entries beyond the tail are exactly 0 and the map is clamped to wmin there"""
    from lintransunet_amd import infer as P
    roi = (16, 16, 8)
    g0, g1, g2, wmin = P.importance_tables(roi, 'gaussian', 0.05)          # sigma 0.8 / 0.8 / 0.4: tails 3, 3, 2
    assert (g0 == 0).sum() == 16 - 7 and (g2 == 0).sum() == 8 - 5
    for g, r in zip((g0, g1, g2), roi):
        np.testing.assert_allclose(g, _gauss_axis(r, 0.05), rtol=1e-7, atol=0)
    assert wmin > 0 and abs(wmin - g0[g0 > 0].min() * g1[g1 > 0].min() * g2[g2 > 0].min()) <= 1e-7 * wmin
    w = np.maximum(np.einsum('i,j,k->ijk', g0, g1, g2), wmin)
    assert w.min() == wmin and (w == wmin).sum() > 16 * 16 * 8 // 2
    np.testing.assert_allclose(w, _ref_map(roi, 'gaussian', 0.05), rtol=1e-7, atol=0)
    c = P.importance_tables((7, 5, 3), 'constant', 0)
    assert all(np.array_equal(t, np.ones(r)) for t, r in zip(c[:3], (7, 5, 3))) and c[3] == 1.0


def test_item_order_and_batches():
    from lintransunet_amd import infer as P
    assert P.mirror_masks(()) == [0]
    assert P.mirror_masks((0,)) == [0, 1]
    assert P.mirror_masks((0, 1)) == [0, 1, 2, 3]
    assert P.mirror_masks((2, 0)) == [0, 4, 1, 5]
    assert P.mirror_masks((0, 1, 2)) == list(range(8))
    starts = [(0, 0, 0), (0, 4, 0), (3, 4, 2)]
    axes = (1, 2)
    items = P.window_items(2, starts, axes)
    want = []
    for idx in range(2 * len(starts)):
        for m in range(4):
            mask = (2 if m & 1 else 0) | (4 if m & 2 else 0)
            want.append((idx // len(starts), *starts[idx % len(starts)], mask))
    assert items == want
    assert P.window_items(1, starts) == [(0, *s, 0) for s in starts]
    batches = P.item_batches(items, 5)
    assert [len(b) for b in batches] == [5, 5, 5, 5, 4]
    assert [it for b in batches for it in b] == items


def test_python_refusals():
    """bad mode / sigma_scale / mirror_axes raise ValueError before anything runs (CPU input and a predictor that must not be
    called: the options are checked first)"""
    from lintransunet_amd import infer as P

    def never(_):
        raise AssertionError('predictor called')

    x = torch.zeros(1, 1, 8, 8, 8)
    bad = [dict(mode='linear'), dict(mode=None), dict(mode='gaussian', sigma_scale=0), dict(mode='gaussian', sigma_scale=-0.1),
           dict(mode='gaussian', sigma_scale=(0.1, 0.0, 0.1)), dict(mode='gaussian', sigma_scale=float('nan')),
           dict(sigma_scale=(0.1, 0.2)), dict(sigma_scale='wide'), dict(mirror_axes=(3,)), dict(mirror_axes=(-1,)),
           dict(mirror_axes=(0, 0)), dict(mirror_axes=(True,)), dict(mirror_axes=0), dict(mirror_axes='01'),
           dict(mirror_axes=(0.0,))]
    for kw in bad:
        with pytest.raises(ValueError):
            P.sliding_window_inference(x, (4, 4, 4), 2, never, overlap=0.5, **kw)
        with pytest.raises(ValueError):
            P.infer_volume(torch.nn.Identity(), x, depth_size=4, roi_xy=4, **kw)
    with pytest.raises(ValueError):
        P.importance_tables((4, 4, 4), 'gaussian', 0)
    with pytest.raises(ValueError):
        P.importance_tables((4, 0, 4), 'gaussian', 0.1)
    # constant mode ignores sigma_scale (the reference's call passes sigma_scale=0)
    P._blend_options('constant', 0, ())


def test_probs_refused_in_training_mode():
    from lintransunet_amd.model import get_model_dict
    model = get_model_dict('MaskTransUnet')([8, 8, 8, 16, 32], [20, 12, 9, 10, 6], [False, True, True, True, True], 1, 2)
    assert model.training
    with pytest.raises(ValueError):
        model(torch.zeros(1, 1, 32, 32, 32), probs=True)


def test_cabi_refusals_without_launch():
    """NULL pointers, n > LTU_BLEND_ITEMS_MAX, a mask above 7, C outside 1..8, a window larger than the padded image, a start
    outside it and a sample index out of range are refused before any HIP call"""
    from lintransunet_amd import _lib
    lib = _lib.load()
    fake = 1 << 20                                                                # never dereferenced: every call below is refused
    n = 3
    desc = (ctypes.c_int * (5 * (_lib.BLEND_ITEMS_MAX + 1)))()
    for k, row in enumerate([(0, 0, 0, 0, 0), (1, 4, 0, 2, 5), (0, 8, 8, 4, 7)]):
        for j, v in enumerate(row):
            desc[5 * k + j] = v
    d = ctypes.addressof(desc)
    # blend: seg, votes, wsum, g0, g1, g2, wmin, desc, n, B, C, Hp, Wp, Dp, h, w, d, s
    bl = [fake, fake, fake, fake, fake, fake, 1.0, d, n, 2, 3, 24, 24, 12, 16, 16, 8, None]
    gm = [fake, fake, d, n, 2, 20, 20, 10, 24, 24, 12, 16, 16, 8, None]            # vol, win, desc, n, B, H, W, D, Hp, Wp, Dp, h, w, d
    for i in (0, 1, 2, 3, 4, 5, 7):
        assert lib.ltu_window_blend(*bl[:i], None, *bl[i + 1:]) == -4, i           # NULL pointer: LTU_E_ARG
    for i in (0, 1, 2):
        assert lib.ltu_window_gather_mirror(*gm[:i], None, *gm[i + 1:]) == -4, i
    assert lib.ltu_window_blend(*bl[:8], _lib.BLEND_ITEMS_MAX + 1, *bl[9:]) == -4          # n > 32
    assert lib.ltu_window_gather_mirror(*gm[:3], _lib.BLEND_ITEMS_MAX + 1, *gm[4:]) == -4
    assert lib.ltu_window_blend(*bl[:8], -1, *bl[9:]) == -4
    for C in (0, 9):
        assert lib.ltu_window_blend(*bl[:10], C, *bl[11:]) == -2                  # C outside 1..8: LTU_E_SHAPE
    assert lib.ltu_window_blend(*bl[:14], 25, *bl[15:]) == -2                     # window larger than the padded image
    assert lib.ltu_window_gather_mirror(*gm[:13], 13, None) == -2
    assert lib.ltu_window_gather_mirror(*gm[:5], 25, *gm[6:]) == -2               # image larger than the padded one
    desc[14] = 8                                                                  # mask 8
    assert lib.ltu_window_blend(*bl) == -4 and lib.ltu_window_gather_mirror(*gm) == -4
    desc[14] = 7
    desc[11] = 9                                                                  # item 2 starts at h0 = 9: 9 + 16 > 24
    assert lib.ltu_window_blend(*bl) == -2 and lib.ltu_window_gather_mirror(*gm) == -2
    desc[11] = -1
    assert lib.ltu_window_blend(*bl) == -2 and lib.ltu_window_gather_mirror(*gm) == -2
    desc[11] = 8
    desc[5] = 2                                                                   # item 1: sample 2 of B = 2
    assert lib.ltu_window_blend(*bl) == -2 and lib.ltu_window_gather_mirror(*gm) == -2
    desc[5] = 1
    assert lib.ltu_window_blend(*bl[:8], 0, *bl[9:]) == 0                         # nothing to do: no launch


# ---------------------------------------------------------------------------------------------- GPU
CASES = [((2, 1, 37, 21, 12), (16, 16, 8), 4, 0.6),          # B = 2
         ((1, 1, 10, 40, 6), (16, 16, 8), 3, 0.6),           # smaller than the window along H and D: zero padding
         ((1, 1, 33, 29, 9), (32, 16, 8), 3, 0.25)]          # ragged


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('mode', ['gaussian', 'constant'])
@pytest.mark.parametrize('axes', [(), (0,), (0, 1, 2)])
def test_blend_matches_float64(case, mode, axes):
    from lintransunet_amd import infer as P
    shape, roi, sw, overlap = case
    g = torch.Generator().manual_seed(11)
    x = torch.randn(shape, generator=g)
    got = P.sliding_window_inference(x.to(DEV), roi, sw, _soft_predictor, overlap=overlap, mode=mode, mirror_axes=axes)
    ref = _ref_blend(x.double().numpy(), roi, sw, _soft_predictor_np, overlap, mode, 0.125, axes)
    assert got.shape == ref.shape
    err = np.abs(got.cpu().double().numpy() - ref).max()
    assert err <= 1e-5, err


@pytest.mark.gpu
def test_blend_reference_size_matches_float64():
    """the reference's geometry: a 512x512x40 scan, 512x512x32 windows, sw_batch_size 4, overlap 0.6; Gaussian + mirror (0, 1)"""
    from lintransunet_amd import infer as P
    g = torch.Generator().manual_seed(12)
    x = torch.randn((1, 1, 512, 512, 40), generator=g)
    roi = (512, 512, 32)
    got = P.sliding_window_inference(x.to(DEV), roi, 4, _soft_predictor, overlap=0.6, mode='gaussian', mirror_axes=(0, 1))
    ref = _ref_blend(x.double().numpy(), roi, 4, _soft_predictor_np, 0.6, 'gaussian', 0.125, (0, 1))
    err = np.abs(got.cpu().double().numpy() - ref).max()
    assert err <= 1e-5, err


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['gaussian', 'constant'])
@pytest.mark.parametrize('shape,overlap,tol', [((2, 1, 32, 32, 16), 0.0, 1e-6), ((2, 1, 37, 21, 12), 0.6, 1e-5)])
def test_flip_equivariant_predictor(mode, shape, overlap, tol):
    """a point-wise predictor commutes with flips: mirroring changes nothing but fp32 rounding.  Tiling windows (one window per
    voxel, 8 summands with the mirrors) hold 1e-6; at overlap 0.6 a voxel sums up to 24 Gaussian-weighted terms, 192 with the
    mirrors, and an fp32 emulation of the contract on the CPU gives the same 3.5e-6 difference as the kernel"""
    from lintransunet_amd import infer as P
    g = torch.Generator().manual_seed(13)
    x = torch.randn(shape, generator=g).to(DEV)
    a = P.sliding_window_inference(x, (16, 16, 8), 4, _pointwise_predictor, overlap=overlap, mode=mode)
    b = P.sliding_window_inference(x, (16, 16, 8), 4, _pointwise_predictor, overlap=overlap, mode=mode, mirror_axes=(0, 1, 2))
    assert (a - b).abs().max().item() <= tol


@pytest.mark.gpu
@pytest.mark.parametrize('mode,axes', [('gaussian', (0, 2)), ('constant', ())], ids=['gaussian_mirror', 'constant'])
def test_deterministic_across_calls_and_batch_sizes(mode, axes):
    """fixed per-voxel item order: bit-identical between calls and for every sw_batch_size (40 > 32 items splits a predictor
    batch into two launches), for the plain average of a soft predictor as for the Gaussian / mirrored blend"""
    from lintransunet_amd import infer as P
    g = torch.Generator().manual_seed(14)
    x = torch.randn((2, 1, 37, 21, 12), generator=g).to(DEV)
    kw = dict(overlap=0.6, mode=mode, mirror_axes=axes)
    first = P.sliding_window_inference(x, (16, 16, 8), 4, _soft_predictor, **kw)
    assert torch.equal(P.sliding_window_inference(x, (16, 16, 8), 4, _soft_predictor, **kw), first)
    for sw in (1, 3, 8, 40):
        assert torch.equal(P.sliding_window_inference(x, (16, 16, 8), sw, _soft_predictor, **kw), first), sw


@pytest.mark.gpu
def test_unit_tables_are_integer_sums_on_one_hot():
    """ltu_window_blend with tables of ones and wmin = 1 on one-hot windows (a repeated window, partial overlaps, both samples of
    B = 2) = the integer accumulation of the same items on the host, exactly"""
    from lintransunet_amd import _lib
    from lintransunet_amd.ops import _p, _s
    g = torch.Generator().manual_seed(15)
    B, C, img, roi = 2, 3, (24, 20, 12), (16, 16, 8)
    items = [(0, 0, 0, 0), (0, 8, 4, 4), (1, 2, 2, 2), (0, 0, 0, 0), (0, 4, 4, 0), (1, 8, 4, 4)]
    n = len(items)
    cls = torch.randint(0, C, (n,) + roi, generator=g)
    onehot = torch.nn.functional.one_hot(cls, C)                                         # [n, h, w, d, C]
    seg = onehot.to(torch.float32).to(DEV).contiguous()
    ref_v = np.zeros((B, C) + img, dtype=np.int64)
    ref_c = np.zeros((B,) + img, dtype=np.int64)
    for (b, h0, w0, d0), oh in zip(items, onehot.numpy()):
        sl = (slice(h0, h0 + roi[0]), slice(w0, w0 + roi[1]), slice(d0, d0 + roi[2]))
        ref_v[b][(slice(None),) + sl] += np.moveaxis(oh, -1, 0)
        ref_c[b][sl] += 1
    votes = torch.zeros((B, C) + img, device=DEV)
    wsum = torch.zeros((B,) + img, device=DEV)
    ones = torch.ones(sum(roi), device=DEV)
    desc = np.array([it + (0,) for it in items], dtype=np.int32)
    _lib.call('ltu_window_blend', _p(seg), _p(votes), _p(wsum), _p(ones), _p(ones[roi[0]:]), _p(ones[roi[0] + roi[1]:]), 1.0,
              desc.ctypes.data, n, B, C, *img, *roi, _s())
    assert torch.equal(votes.cpu(), torch.from_numpy(ref_v).to(torch.float32))
    assert torch.equal(wsum.cpu(), torch.from_numpy(ref_c).to(torch.float32))


def _onehot8_predictor(w):
    """8 classes from thresholds of the window intensities, one-hot, channels-last memory"""
    cls = sum((w[:, 0] > t).long() for t in (-1.2, -0.7, -0.3, 0.0, 0.3, 0.7, 1.2))
    return torch.nn.functional.one_hot(cls, 8).to(torch.float32).permute(0, 4, 1, 2, 3)


@pytest.mark.gpu
def test_constant_mode_channel_limit():
    """the blend kernels stop at 8 output channels: 8 one-hot channels equal the oracle exactly, a 9th is refused as an LtuError
    that names the limit, not as the library's LTU_E_SHAPE"""
    from lintransunet_amd import _lib, infer as P
    g = torch.Generator().manual_seed(18)
    x = torch.randn((1, 1, 10, 9, 7), generator=g)
    roi = (6, 6, 4)
    ref = O.sliding_window_inference(x, roi, 3, _onehot8_predictor, overlap=0.5)
    got = P.sliding_window_inference(x.to(DEV), roi, 3, _onehot8_predictor, overlap=0.5)
    assert got.shape == ref.shape == (1, 8, 10, 9, 7) and torch.equal(got.cpu(), ref)
    with pytest.raises(_lib.LtuError, match='1 .. 8') as err:
        P.sliding_window_inference(x.to(DEV), roi, 3, lambda w: torch.cat((_onehot8_predictor(w), w), 1), overlap=0.5)
    assert 'LTU_E_SHAPE' not in str(err.value)


def _model():
    from lintransunet_amd.model import get_model_dict
    torch.manual_seed(3)
    return get_model_dict('MaskTransUnet')([8, 8, 8, 16, 32], [20, 12, 9, 10, 6], [False, True, True, True, True], 1, 2).to(DEV)


@pytest.mark.gpu
def test_model_probs_and_graph():
    from lintransunet_amd import infer as P
    model = _model().eval()
    g = torch.Generator().manual_seed(16)
    x = torch.randn((2, 1, 32, 32, 32), generator=g).to(DEV)
    with torch.no_grad():
        p = model(x, probs=True)
        oh = model(x)
    assert p.shape == oh.shape == (2, 2, 32, 32, 32) and p.dtype == torch.float32
    assert p.permute(0, 2, 3, 4, 1).is_contiguous()                               # channels-last: blended without a copy
    assert (p.sum(1) - 1).abs().max().item() <= 1e-6
    want = torch.nn.functional.one_hot(p.argmax(1), 2).permute(0, 4, 1, 2, 3).to(torch.float32)
    assert torch.equal(oh, want)
    pred = P.GraphedPredictor(model, 2, (32, 32, 32), x.device, probs=True)
    assert torch.equal(pred(x), p)


@pytest.mark.gpu
def test_model_gaussian_mirror_matches_float64_and_infer_volume():
    """the real model through a GraphedPredictor(probs=True): the blend equals float64 blending of the per-item outputs it was
    given (recorded by a thin wrapper), and infer_volume returns the same tensor bit for bit"""
    from lintransunet_amd import infer as P
    model = _model().eval()
    g = torch.Generator().manual_seed(17)
    x = torch.randn((1, 1, 48, 32, 40), generator=g)
    roi, sw = (32, 32, 32), 2
    graphed = P.GraphedPredictor(model, sw, roi, DEV, probs=True)
    outs = []

    def recorder(win):
        y = graphed(win)
        outs.extend(y.double().cpu().numpy())
        return y

    got = P.sliding_window_inference(x.to(DEV), roi, sw, recorder, overlap=0.6, mode='gaussian', mirror_axes=(0, 1))
    ref = _ref_blend(x.double().numpy(), roi, sw, lambda _w, k: outs[k], 0.6, 'gaussian', 0.125, (0, 1))
    err = np.abs(got.cpu().double().numpy() - ref).max()
    assert err <= 1e-5, err
    assert (got.sum(1) - 1).abs().max().item() <= 1e-5
    vol = P.infer_volume(model, x.to(DEV), depth_size=32, roi_xy=32, sw_batch_size=sw, overlap=0.6, mode='gaussian', probs=True,
                         mirror_axes=(0, 1), graph=True)
    assert torch.equal(vol, got)
