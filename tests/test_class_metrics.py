"""Multi-class evaluation metrics of infer.class_metrics / infer.evaluate_multiclass / losses.get_multi_criterions
(csrc/class_metrics.hip): the eight criteria of inference_multi_classes.py:153 and its label map.  A float64 numpy restatement of
loss/multi_criterions.py is pinned to the reference by tests/golden/multi_metrics.npz (make_golden_multi_metrics.py runs the
reference's own modules); the GPU path is checked against the golden values and against the restatement."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = 'cuda'
NAMES = ('DiceClassLoss0', 'DiceClassLoss', 'DiceClassLoss2', 'Recall', 'Precision', 'Recall2', 'Precision2', 'LocalizationLoss')
ENTRY_POINTS = ('ltu_class_metrics_ws_elems', 'ltu_class_metrics_pass', 'ltu_class_metrics_finalize')
CASES = ('onehot', 'soft', 'absent2_both', 'absent2_pred', 'empty_fg', 'c4')


# ---------------------------------------------------------------------------------------------- CPU restatement
def restate(pred, masks, threshold=None):
    """float64 restatement of loss/multi_criterions.py on pred [B, C, H, W, D] and class ids masks [B, 1, H, W, D]:
    per sample Dice / Recall / Precision [B, C], the foreground Dice [B] and the multi-class LocalizationLoss [B]"""
    p = np.asarray(pred, dtype=np.float64)
    if threshold is not None:
        p = (p >= threshold).astype(np.float64)
    m = np.asarray(masks)[:, 0].astype(np.int64)
    B, C = p.shape[:2]
    t = np.stack([m == c for c in range(C)], 1).astype(np.float64)
    ax = (2, 3, 4)
    sp, st, spt = p.sum(ax), t.sum(ax), (p * t).sum(ax)
    out = {'Dice': (2 * spt + 1e-9) / (sp + st + 1e-9), 'Recall': (spt + 1e-5) / (st + 1e-5), 'Precision': (spt + 1e-5) / (sp + 1e-5)}
    fp, ft = 1 - p[:, 0], (m != 0).astype(np.float64)
    out['ForegroundDice'] = (2 * (fp * ft).sum((1, 2, 3)) + 1e-9) / (fp.sum((1, 2, 3)) + ft.sum((1, 2, 3)) + 1e-9)
    # LocalizationLoss: the three "axes" of the reference all reduce to the H profile; no factor 8
    prof_p = 1 / (1 + np.exp(-(fp.sum((2, 3)) - 10)))
    prof_t = 1 / (1 + np.exp(-(ft.sum((2, 3)) - 10)))
    cp = np.cumsum(prof_p, -1) / (prof_p.sum(-1, keepdims=True) + 1e-6)
    ct = np.cumsum(prof_t, -1) / (prof_t.sum(-1, keepdims=True) + 1e-6)
    out['LocalizationLoss'] = np.abs(cp - ct).mean(-1)
    return out


def driver_values(r):
    """the eight values of the driver from the per-sample restatement"""
    return np.array([1 - r['ForegroundDice'].mean(), 1 - r['Dice'][:, 1].mean(), 1 - r['Dice'][:, 2].mean(),
                     r['Recall'][:, 1].mean(), r['Precision'][:, 1].mean(), r['Recall'][:, 2].mean(), r['Precision'][:, 2].mean(),
                     r['LocalizationLoss'].mean()])


def _golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'multi_metrics.npz'))


def _close(got, ref, rtol, atol=1e-12):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= rtol * np.abs(ref) + atol), (got, ref, np.abs(got - ref))


# ---------------------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize('tag', CASES)
def test_restatement_matches_reference_golden(tag):
    g = _golden()
    assert tuple(g['names']) == NAMES
    _close(driver_values(restate(g[f'{tag}_pred'], g[f'{tag}_masks'])), g[f'{tag}_values'], 1e-6)


def test_golden_covers_the_issue_cases():
    g = _golden()
    assert g['soft_pred'].shape[3] * g['soft_pred'].shape[4] % 4 != 0             # a ragged W * D
    assert len(np.unique(g['soft_pred'])) > 2
    assert g['c4_pred'].shape[1] == 4
    for tag in ('absent2_both',):
        assert not (g[f'{tag}_masks'] == 2).any() and not g[f'{tag}_pred'][:, 2].any()
    assert not g['absent2_pred_pred'][:, 2].any() and (g['absent2_pred_masks'] == 2).any()
    assert not g['empty_fg_masks'][0].any() and not g['empty_fg_pred'][:, 1:].any()


def test_get_multi_criterions_maps_the_driver_names():
    from lintransunet_amd import infer, losses
    assert infer.MULTI_METRIC_NAMES == NAMES
    crit = losses.get_multi_criterions(list(NAMES) + ['CrossEntroLoss', 'RecallLoss', 'PrecisionLoss'])
    assert list(crit) == list(NAMES) + ['CrossEntroLoss', 'RecallLoss', 'PrecisionLoss']
    assert all(isinstance(m, torch.nn.Module) for m in crit.values())
    for name in ('CrossEntroLoss', 'DiceClassLoss0', 'DiceClassLoss', 'DiceClassLoss2'):       # the differentiable modules
        assert isinstance(crit[name], losses.Loss_Dict[name])
    for name in ('Recall', 'Precision', 'Recall2', 'Precision2', 'LocalizationLoss'):
        assert isinstance(crit[name], losses._MultiEvalMetric)
    # the multi-class LocalizationLoss is not the binary one of loss/criterions.py
    assert not isinstance(crit['LocalizationLoss'], losses.LocalizationLoss)
    with pytest.raises(KeyError, match='IOULoss'):
        losses.get_multi_criterions(['DiceClassLoss', 'IOULoss'])


def test_entry_points_declared_and_contract_errors():
    from lintransunet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and f' {name}(' in header and hasattr(lib, name), name
    n = lib.ltu_class_metrics_ws_elems(1, 3, 512, 512, 200)
    assert n >= 1 * 12 * 512 and n % (12 * 512) == 0                           # [B][3C + 3][H][chunks] doubles
    assert lib.ltu_class_metrics_ws_elems(1, 9, 4, 4, 4) == 0                    # refused shape
    fake = 1 << 20
    need = lib.ltu_class_metrics_ws_elems(2, 3, 8, 8, 8)
    args = (fake, fake, None, fake, need, 2, 3, 8, 8, 8, 0.5, None)
    assert lib.ltu_class_metrics_pass(*args[:4], need - 1, *args[5:]) == -4     # short scratch: LTU_E_ARG, nothing launched
    assert lib.ltu_class_metrics_pass(*args[:3], None, *args[4:]) == -4
    assert lib.ltu_class_metrics_pass(*args[:10], float('nan'), None) == -4
    assert lib.ltu_class_metrics_pass(*args[:6], 9, *args[7:]) == -2             # C outside 2 .. 8
    assert lib.ltu_class_metrics_pass(*args[:6], 1, *args[7:]) == -2
    assert lib.ltu_class_metrics_finalize(fake, need - 1, fake, 2, 3, 8, 8, 8, None) == -4


def test_rejects_cpu_and_bad_arguments():
    from lintransunet_amd import _lib, infer as P
    with pytest.raises(_lib.LtuError):
        P.class_metrics(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4, dtype=torch.int64))
    with pytest.raises(_lib.LtuError):
        P.evaluate_multiclass(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------- GPU tests
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(got, ref, rtol, classes=None):
    for name in ('Dice', 'Recall', 'Precision'):
        r = ref[name] if classes is None else ref[name][:, list(classes)]
        _close(got[name].cpu().numpy(), r, rtol, 1e-7)
    _close(got['ForegroundDice'].cpu().numpy(), ref['ForegroundDice'], rtol, 1e-7)
    _close(got['LocalizationLoss'].cpu().numpy(), ref['LocalizationLoss'], rtol, 1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', CASES)
def test_evaluate_multiclass_matches_reference_golden(tag):
    from lintransunet_amd import infer as P
    g = _golden()
    got = P.evaluate_multiclass(_dev(g[f'{tag}_pred']), _dev(g[f'{tag}_masks']))
    assert tuple(got) == NAMES
    vals = np.array([got[n].item() for n in NAMES])
    _close(vals, g[f'{tag}_values'], 1e-5 if tag == 'soft' else 1e-6, 1e-7)


def _random_case(seed, B, C, shape, ties=False):
    rng = np.random.default_rng(seed)
    if ties:
        pred = rng.integers(0, 3, (B, C) + shape).astype(np.float32) / 2                 # values 0, 0.5, 1: many ties
    else:
        logits = rng.normal(0, 2, (B, C) + shape)
        pred = (np.exp(logits) / np.exp(logits).sum(1, keepdims=True)).astype(np.float32)
    masks = rng.integers(0, C, (B, 1) + shape).astype(np.uint8)
    masks[:, :, : shape[0] // 3] = 0                                                     # rows without foreground
    return pred, masks


@pytest.mark.gpu
@pytest.mark.parametrize('C', [2, 3, 4])
@pytest.mark.parametrize('threshold', [None, 0.5])
@pytest.mark.parametrize('shape', [(24, 21, 13), (24, 20, 13)])                          # W * D ragged / a multiple of 4
def test_class_metrics_matches_restatement(C, threshold, shape):
    from lintransunet_amd import infer as P
    pred, masks = _random_case(7 * C + len(shape), 2, C, shape)
    got = P.class_metrics(_dev(pred), _dev(masks), threshold=threshold)
    assert got['Dice'].shape == (2, C) and got['ForegroundDice'].shape == (2,)
    _check(got, restate(pred, masks, threshold), 1e-6 if threshold is not None else 1e-5)
    sub = P.class_metrics(_dev(pred), _dev(masks), class_indices=(C - 1, 0), threshold=threshold)
    for name in ('Dice', 'Recall', 'Precision'):
        assert torch.equal(sub[name], got[name][:, [C - 1, 0]])


@pytest.mark.gpu
@pytest.mark.parametrize('tag', CASES)
def test_class_metrics_empty_classes(tag):
    """every golden case (absent classes on one or both sides, empty foreground) against the restatement, per sample and class"""
    from lintransunet_amd import infer as P
    g = _golden()
    pred, masks = g[f'{tag}_pred'], g[f'{tag}_masks']
    _check(P.class_metrics(_dev(pred), _dev(masks)), restate(pred, masks), 1e-5 if tag == 'soft' else 1e-6)
    _check(P.class_metrics(_dev(pred), _dev(masks), threshold=0.5), restate(pred, masks, 0.5), 1e-6)


def _scan(D, seed):
    """a 512 x 512 x D scan: organ (1) and lesion (2) ellipsoids, a one-hot prediction that misses part of them"""
    shape = (512, 512, D)
    hh, ww, dd = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in shape], indexing='ij', sparse=True)

    def ell(c, r):
        return ((hh - c[0]) / r[0]) ** 2 + ((ww - c[1]) / r[1]) ** 2 + ((dd - c[2]) / r[2]) ** 2 <= 1

    lab = np.zeros(shape, np.uint8)
    lab[ell((300, 250, D / 2), (60, 40, D / 4))] = 1
    lab[ell((320, 262, D / 2 + 2), (15, 12, D / 8))] = 2
    plab = np.zeros(shape, np.uint8)
    plab[ell((305, 248, D / 2 + 1), (58, 42, D / 4 - 1))] = 1
    plab[ell((316, 262, D / 2 + 2), (16, 10, D / 8))] = 2
    plab[ell((200, 100, D / 3), (8, 6, 3))] = 1
    rng = np.random.default_rng(seed)
    noise = rng.random(shape) < 0.002
    plab[noise] = rng.integers(0, 3, int(noise.sum()))
    return plab, lab


def _onehot_dev(plab, C=3):
    t = torch.from_numpy(plab).to(DEV).long()
    return torch.nn.functional.one_hot(t, C).permute(3, 0, 1, 2)[None].to(torch.float32).contiguous()


def _restate_onehot(plab, lab, C=3):
    """the restatement for a one-hot prediction, without materialising it in float64"""
    p = np.stack([plab == c for c in range(C)])[None]
    return restate(p, lab[None, None])


def _ulps(got, ref, n):
    r32 = np.asarray(ref, np.float64).astype(np.float32)
    assert np.all(np.abs(np.asarray(got, np.float32) - r32) <= n * np.spacing(np.abs(r32))), (got, ref)


@pytest.mark.gpu
def test_whole_scan_512x512x48_bit_identical_and_label_map():
    from lintransunet_amd import infer as P
    plab, lab = _scan(48, 1)
    pred, masks = _onehot_dev(plab), torch.from_numpy(lab[None, None]).to(DEV)
    got = P.class_metrics(pred, masks, return_label_map=True)
    again = P.class_metrics(pred, masks, return_label_map=True)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    assert torch.equal(got['label_map'], torch.argmax(pred, 1).to(torch.uint8))
    _check(got, _restate_onehot(plab, lab), 1e-6)
    ev = P.evaluate_multiclass(pred, masks)
    ev2 = P.evaluate_multiclass(pred, masks)
    assert all(torch.equal(ev[n], ev2[n]) for n in NAMES)
    _close(np.array([ev[n].item() for n in NAMES]), driver_values(_restate_onehot(plab, lab)), 1e-6, 1e-7)


@pytest.mark.gpu
def test_whole_scan_class0_beyond_2_pow_24():
    """512 x 512 x 80: class 0 covers more than 2^24 voxels, so any fp32 total would be inexact; the integer-valued sums here
    are exact, so every ratio equals the float64 restatement rounded to f32 (a last-ulp margin for the fused fp64 steps)"""
    from lintransunet_amd import infer as P
    plab, lab = _scan(80, 2)
    assert (lab == 0).sum() > 2 ** 24 and (plab == 0).sum() > 2 ** 24
    got = P.class_metrics(_onehot_dev(plab), torch.from_numpy(lab[None, None]).to(DEV))
    ref = _restate_onehot(plab, lab)
    for name in ('Dice', 'Recall', 'Precision', 'ForegroundDice'):
        _ulps(got[name].cpu().numpy(), ref[name], 1)
    _close(got['LocalizationLoss'].cpu().numpy(), ref['LocalizationLoss'], 1e-6, 1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(24, 21, 13), (16, 32, 8)])
@pytest.mark.parametrize('C', [2, 3, 5, 8])
def test_label_map_equals_torch_argmax_with_ties(shape, C):
    from lintransunet_amd import infer as P
    pred, masks = _random_case(C, 2, C, shape, ties=True)
    pred[0, :, 0, 0, :] = 0.5                                                            # a row where every class ties
    got = P.class_metrics(_dev(pred), _dev(masks), return_label_map=True)
    ref = torch.argmax(torch.from_numpy(pred), 1).to(torch.uint8)
    assert got['label_map'].dtype == torch.uint8 and torch.equal(got['label_map'].cpu(), ref)
    ev = P.evaluate_multiclass(_dev(pred), _dev(masks), return_label_map=True) if C >= 3 else None
    if ev is not None:
        assert torch.equal(ev['label_map'].cpu(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize('C', [3, 4])
def test_integer_and_onehot_masks_agree(C):
    from lintransunet_amd import infer as P
    pred, masks = _random_case(40 + C, 2, C, (20, 18, 11))
    m = torch.from_numpy(masks).long()
    onehot = torch.nn.functional.one_hot(m[:, 0], C).permute(0, 4, 1, 2, 3).contiguous()
    for thr in (None, 0.5):
        a = P.class_metrics(_dev(pred), m.to(DEV), threshold=thr)
        b = P.class_metrics(_dev(pred), onehot.to(DEV), threshold=thr)
        c = P.class_metrics(_dev(pred), _dev(masks), threshold=thr)
        for k in a:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


@pytest.mark.gpu
def test_short_scratch_is_refused_without_launch():
    from lintransunet_amd import _lib
    from lintransunet_amd.ops import _p, _s
    B, C, H, W, D = 2, 3, 8, 8, 8
    pred = torch.rand((B, C, H, W, D), device=DEV)
    tgt = torch.zeros((B, H, W, D), device=DEV, dtype=torch.uint8)
    lmap = torch.full((B, H, W, D), 7, device=DEV, dtype=torch.uint8)
    out = torch.full((B + 1, 3 * C + 2), -7.0, device=DEV)
    ws = _lib.load().ltu_class_metrics_ws_elems(B, C, H, W, D)
    scratch = torch.full((ws,), 3.0, device=DEV, dtype=torch.float64)
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
        _lib.call('ltu_class_metrics_pass', _p(pred), _p(tgt), _p(lmap), _p(scratch), ws - 1, B, C, H, W, D, 0.5, _s())
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
        _lib.call('ltu_class_metrics_finalize', _p(scratch), ws - 1, _p(out), B, C, H, W, D, _s())
    torch.cuda.synchronize()
    assert torch.all(lmap == 7) and torch.all(out == -7.0) and torch.all(scratch == 3.0)


@pytest.mark.gpu
def test_looped_get_multi_criterions_equals_evaluate_multiclass():
    """the driver's loop `[l(predict2, label).item() for l in criterions.values()]` over get_multi_criterions, with label the
    one-hot of masks as the driver builds it"""
    from lintransunet_amd import infer as P, losses
    g = _golden()
    for tag in ('onehot', 'soft'):
        pred, masks = _dev(g[f'{tag}_pred']), _dev(g[f'{tag}_masks'])
        label = torch.nn.functional.one_hot(masks[:, 0].long(), 3).permute(0, 4, 1, 2, 3).contiguous()
        crit = losses.get_multi_criterions(list(NAMES))
        looped = [crit[n](pred, label).item() for n in NAMES]
        ev = P.evaluate_multiclass(pred, masks)
        for n, v in zip(NAMES, looped):
            if n.startswith('DiceClassLoss'):          # the differentiable level-loss kernel: fp32 sums in another order
                assert abs(v - ev[n].item()) <= 1e-5 * max(abs(v), 1e-3), (tag, n, v, ev[n].item())
            else:
                assert v == ev[n].item(), (tag, n)
        _close(np.array(looped), g[f'{tag}_values'], 1e-5, 1e-7)


@pytest.mark.gpu
def test_chain_model_infer_volume_largest_component_metrics():
    """dim_output = 3 model with seeded parameters -> infer_volume -> keep_largest_component -> evaluate_multiclass, against the
    restatement applied to the GPU's own predict2"""
    from lintransunet_amd import infer as P
    from lintransunet_amd.model import get_model_dict
    from oracle import net as O_net, seedgen
    cfg = O_net.NetConfig(num_layers=[8, 8, 8, 16, 32], roi_size_list=[20, 12, 9, 10, 6], dim_output=3)
    model = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, 1, 3)
    model.load_state_dict(seedgen.seeded_params(O_net.param_shapes(cfg), 41), strict=True)
    model = model.to(DEV)
    x = seedgen.seeded_volume((1, 1, 48, 40, 36), 42).to(DEV)
    g = torch.Generator().manual_seed(43)
    masks = torch.nn.functional.avg_pool3d(torch.randn((1, 1, 48, 40, 36), generator=g), 5, stride=1, padding=2) * 4
    masks = ((masks > 0.2).long() + (masks > 0.9).long()).to(torch.uint8)
    predict = P.infer_volume(model, x, depth_size=32, roi_xy=32, sw_batch_size=2, overlap=0.6)
    predict2 = P.keep_largest_component(predict)
    got = P.evaluate_multiclass(predict2, masks.to(DEV), return_label_map=True)
    p2 = predict2.cpu().numpy()
    _close(np.array([got[n].item() for n in NAMES]), driver_values(restate(p2, masks.numpy())), 1e-6, 1e-7)
    assert torch.equal(got['label_map'].cpu(), torch.argmax(predict2.cpu(), 1).to(torch.uint8))
