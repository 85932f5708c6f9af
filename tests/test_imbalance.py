"""The imbalance stage of the level loss, host side: the restatement of tests/imbalance_common.py that the GPU tests compare against
(its analytic gradients against torch.autograd on a float64 CPU restatement, its two named special cases), the new names of
losses.LevelCriterion with the ranges of losses.Imbalance, and the C-ABI surface of csrc/loss_imbalance.hip."""
import os
import re

import numpy as np
import pytest
import torch

from tests.imbalance_common import CLAMP32, imbalance_ref, late_probs, sums_ref, tolerance
from tests.topk_common import make_labels, make_probs, voxel_losses_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ltu_loss_imb_ws_floats', 'ltu_loss_imb_fwd', 'ltu_loss_imb_bwd')


# ---------------------------------------------------------------------------------------------- the oracle
def _torch_total(p, label, classes, weights, alpha, beta, gamma, eps, batch, w_focal, gf, fa):
    """the formulas once more, in torch float64, written for autograd (one-hot products, no analytic derivative anywhere)"""
    B, C = p.shape[0], p.shape[-1]
    pf = p.reshape(B, -1, C)
    t = (label.reshape(B, -1, 1) == torch.arange(C).reshape(1, 1, C)).double()
    I, FP, FN = (pf * t).sum(1), (pf * (1 - t)).sum(1), (t * (1 - pf)).sum(1)
    total = pf.new_zeros(())
    for c, w in zip(classes, weights):
        i, fp, fn = (I[:, c], FP[:, c], FN[:, c]) if not batch else (I[:, c].sum(), FP[:, c].sum(), FN[:, c].sum())
        r = (alpha * fp + beta * fn) / (i + alpha * fp + beta * fn + eps)
        total = total + w * (r if gamma == 1 else r ** (1.0 / gamma)).mean()
    a = torch.ones(C, dtype=torch.float64) if fa is None else torch.tensor(fa, dtype=torch.float64)
    nl = -torch.log(torch.clamp(pf, min=float(CLAMP32)))
    focus = 1.0 if gf == 0 else (1 - pf) ** gf
    return total + w_focal * (t * a * focus * nl).sum() / (B * pf.shape[1])


CONFIGS = [dict(alpha=0.3, beta=0.7, gamma=1.0, batch=False, gf=0.0, fa=None),
           dict(alpha=0.5, beta=0.5, gamma=4.0 / 3.0, batch=True, gf=2.0, fa=(0.5, 2.0, 1.0, 0.0, 3.0)),
           dict(alpha=0.3, beta=0.7, gamma=4.0 / 3.0, batch=False, gf=1.0, fa=None),
           dict(alpha=1.0, beta=0.0, gamma=3.0, batch=True, gf=2.5, fa=None)]


@pytest.mark.parametrize('late', [False, True])
@pytest.mark.parametrize('cfg', CONFIGS)
def test_oracle_gradients_against_autograd(cfg, late):
    B, spatial, C = 2, (6, 5, 4), 5
    if late:
        p, lab = late_probs(B, spatial, C, 3)
    else:
        p, lab = make_probs(B, spatial, C, 1), make_labels(B, spatial, C, 2)
    lab = lab.copy()
    lab.reshape(-1)[[5, 77]] = 200                                   # labels without a channel
    classes, weights = (1, 0, 4), (1.0, 0.5, 2.0)
    r = imbalance_ref(p, lab, classes, weights, w_focal=0.8, **cfg)
    pt = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    total = _torch_total(pt, torch.from_numpy(lab.astype(np.int64)), classes, weights, cfg['alpha'], cfg['beta'], cfg['gamma'],
                         cfg['eps'] if 'eps' in cfg else 1e-5, cfg['batch'], 0.8, cfg['gf'], cfg['fa'])
    total.backward()
    assert abs(total.item() - r['total']) <= 1e-12 * abs(r['total'])
    g = pt.grad.numpy()
    # torch's clamp passes no gradient below the clamp and (1 - p)^gf has a finite derivative at p = 1 for gf >= 1: the same rules
    assert np.isfinite(g).all() and np.abs(g - r['grad']).max() <= 1e-11 * np.abs(g).max()


def test_tversky_half_half_is_soft_dice():
    B, spatial, C = 3, (7, 5, 4), 4
    p, lab = make_probs(B, spatial, C, 7), make_labels(B, spatial, C, 8)
    pf, t = p.reshape(B, -1, C).astype(np.float64), (lab.reshape(B, -1, 1) == np.arange(C))
    for batch in (False, True):
        r = imbalance_ref(p, lab, range(C), [1.0] * C, alpha=0.5, beta=0.5, gamma=1.0, eps=0.5e-5, batch=batch, grad=False)
        I, P, T = (pf * t).sum(1), pf.sum(1), t.sum(1)
        if batch:
            I, P, T = I.sum(0), P.sum(0), T.sum(0)
        dice = (2 * I + 1e-5) / (P + T + 1e-5)                       # nnU-Net's soft Dice
        want = 1 - dice if batch else (1 - dice).mean(0)
        assert np.abs(r['values'] - want).max() <= 1e-13


def test_focal_gamma_zero_is_mean_cross_entropy():
    B, spatial, C = 2, (9, 7, 5), 3
    p, lab = late_probs(B, spatial, C, 11)
    lab = lab.copy()
    lab.reshape(-1)[[3, 100, 200]] = 77
    l, _, _ = voxel_losses_ref(p, lab)                               # -log max(p[label], 1e-6), 0 where label >= C
    r = imbalance_ref(p, lab, w_focal=1.0, gf=0.0)
    assert abs(r['focal'] - l.mean()) <= 1e-14 and r['total'] == r['focal']
    g = r['grad'].reshape(-1, C)
    assert not g[lab.reshape(-1) == 77].any()


def test_sums_are_non_negative_on_the_late_input():
    p, lab = late_probs(2, (12, 10, 8), 3, 21)
    for dtype in (np.float64, np.float32):
        assert all((x >= 0).all() for x in sums_ref(p, lab, 2.0, dtype=dtype))
    pf = p.reshape(2, -1, 3)
    t = lab.reshape(2, -1, 1) == np.arange(3)
    # what the direct sums avoid: in float32, T - I on this input is off by more than the whole of FN for some class
    I32, T32 = (pf * t).sum(1, dtype=np.float32), t.sum(1, dtype=np.float32)
    FN = sums_ref(p, lab)[2]
    print('FN direct', FN.ravel(), 'T - I in float32', (T32 - I32).ravel())
    tol = tolerance(imbalance_ref(p, lab, (1, 2), (1, 1), gamma=4 / 3), imbalance_ref(p, lab, (1, 2), (1, 1), gamma=4 / 3, dtype=np.float32))
    assert tol['value'][1] < 1e-5 and tol['grad'][1] < 1e-5


# ---------------------------------------------------------------------------------------------- names
def test_level_criterion_accepts_the_names():
    from lintransunet_amd import losses as L
    crit = L.LevelCriterion({'CrossEntroLoss': 10, 'TverskyLoss': 1, 'TverskyLoss2': 1, 'TverskyLoss0c': 0.5, 'FocalCELoss': 1})
    assert crit.tversky == ['TverskyLoss', 'TverskyLoss2', 'TverskyLoss0c'] and crit.focalce and crit.base_names == ['CrossEntroLoss']
    assert [L.LevelCriterion.TVERSKY[n] for n in crit.tversky] == [1, 2, 0]
    assert L.LevelCriterion.TVERSKY == {L.tversky_name(c): c for c in range(8)}
    assert not L.LevelCriterion({'FocalCELoss': 1}).base_names and not L.LevelCriterion({'CrossEntroLoss': 1}).focalce
    rec = L.Imbalance(alpha=0.5, beta=0.5, tversky_gamma=4 / 3, batch=True, focal_gamma=0.0, focal_alpha=[1, 2, 3])
    assert L.LevelCriterion({'TverskyLoss7': 1}, imbalance=rec).imbalance is rec and rec.focal_alpha == (1.0, 2.0, 3.0)
    d = L.Imbalance()
    assert (d.alpha, d.beta, d.tversky_gamma, d.batch, d.eps, d.focal_gamma, d.focal_alpha) == (0.3, 0.7, 1.0, False, 1e-5, 2.0, None)
    for unknown in ('HausdorffLoss', 'TopKLoss', 'DiceClassLoss8', 'BoundaryLoss8', 'TverskyLoss8', 'TverskyLoss1', 'FocalCELoss2'):
        with pytest.raises(KeyError):
            L.LevelCriterion({'CrossEntroLoss': 1, unknown: 1})
    with pytest.raises(ValueError):
        L.LevelCriterion({'TverskyLoss': 1}, imbalance={'alpha': 0.5})


@pytest.mark.parametrize('bad', [dict(alpha=-0.1), dict(beta=-1.0), dict(alpha=0.0, beta=0.0), dict(alpha=float('nan')),
                                 dict(tversky_gamma=0.9), dict(tversky_gamma=4.0), dict(tversky_gamma=float('inf')), dict(eps=0.0),
                                 dict(eps=-1e-5), dict(focal_gamma=0.5), dict(focal_gamma=-1.0), dict(focal_gamma=5.5),
                                 dict(focal_gamma=float('nan')), dict(focal_alpha=(1.0, -1.0)), dict(focal_alpha=(1.0, float('inf'))),
                                 dict(focal_alpha=(1.0,))])
def test_imbalance_ranges_are_refused(bad):
    from lintransunet_amd import losses as L
    with pytest.raises(ValueError):
        L.Imbalance(**bad)


def test_imbalance_ranges_accepted():
    from lintransunet_amd import losses as L
    for ok in (dict(alpha=0.0, beta=1.0), dict(alpha=1.0, beta=0.0), dict(tversky_gamma=1.0), dict(tversky_gamma=3.0), dict(focal_gamma=0.0),
               dict(focal_gamma=1.0), dict(focal_gamma=5.0), dict(focal_alpha=(0.0, 1.0))):
        L.Imbalance(**ok)


def test_class_checks_need_no_device():
    from lintransunet_amd import losses as L
    p, lab = torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError):
        L.LevelCriterion({'TverskyLoss3': 1})(p, lab)               # 3 classes: no class 3
    with pytest.raises(ValueError):
        L.LevelCriterion({'FocalCELoss': 1}, imbalance=L.Imbalance(focal_alpha=(1, 1)))(p, lab)
    with pytest.raises(ValueError):
        L.LevelCriterion({'FocalCELoss': 1, 'FocalLoss': 1})(torch.zeros(1, 5, 4, 4, 4), lab)      # beside the wider family: 4 classes


def test_registries():
    from lintransunet_amd import losses as L
    ms = L.get_criterions(['TverskyLoss', 'FocalCELoss'])
    assert isinstance(ms['TverskyLoss'], L.TverskyLoss) and isinstance(ms['FocalCELoss'], L.FocalCELoss)
    assert ms['TverskyLoss'].impl.tversky == ['TverskyLoss'] and ms['FocalCELoss'].impl.imbalance.focal_gamma == 2.0
    m = L.TverskyLoss(class_index=0, alpha=0.5, beta=0.5, gamma=4 / 3, batch=True)
    assert m.impl.tversky == ['TverskyLoss0c'] and m.impl.imbalance.batch and m.impl.imbalance.tversky_gamma == 4 / 3
    assert L.FocalCELoss(gamma=0.0, alpha=(1, 2)).impl.imbalance.focal_alpha == (1.0, 2.0)
    for name in ('TverskyLoss', 'FocalCELoss'):                      # the multi-class evaluation registry is not widened
        with pytest.raises(KeyError):
            L.get_multi_criterions([name])


def test_train_takes_the_record():
    import inspect
    from lintransunet_amd import train
    specs = train.level_specs(5, ('FocalCELoss', 'TverskyLoss', 'TverskyLoss2'), criterion_weight=[1.0, 0.5, 0.5])
    assert len(specs) == 5 and all(s == {'FocalCELoss': 1.0, 'TverskyLoss': 0.5, 'TverskyLoss2': 0.5} for s in specs)
    assert not train.has_topk(specs) and not train.has_boundary(specs)
    for fn in (train.deep_supervision_loss, train.train_step, train.GraphedStep.__init__):
        assert inspect.signature(fn).parameters['imbalance'].default is None


# ---------------------------------------------------------------------------------------------- C-ABI surface
def test_cabi_surface():
    from lintransunet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    protos = dict(re.findall(r'^(?:int|long long)\s+(ltu_\w+)\s*\(([^;]*)\);', header, flags=re.M | re.S))
    lib = _lib.load()
    for name in NEW:
        assert name in protos and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len([a for a in protos[name].split(',') if a.strip()]) == len(_lib.SIGNATURES[name]), name
    assert lib.ltu_loss_imb_ws_floats.restype is _lib.L
    # (1 + blocks) * B * C * 4 floats; 0 for what the calls refuse: C outside 2 .. 8, B * C * 4 > 256
    assert lib.ltu_loss_imb_ws_floats(2, 960, 3) == 5 * 2 * 3 * 4 and lib.ltu_loss_imb_ws_floats(8, 64 * 64 * 96, 8) == (1 + 128) * 256
    assert lib.ltu_loss_imb_ws_floats(2, 960, 1) == 0 and lib.ltu_loss_imb_ws_floats(2, 960, 9) == 0
    assert lib.ltu_loss_imb_ws_floats(9, 960, 8) == 0 and lib.ltu_loss_imb_ws_floats(0, 960, 3) == 0
    src = open(os.path.join(ROOT, 'lintransunet_amd', 'csrc', 'loss_imbalance.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert 'hipDeviceSynchronize' not in code and 'hipStreamSynchronize' not in code and 'hipMemcpy' not in code
    assert not re.search(r'atomic\w*\s*\(', code)                    # partials folded in a fixed order
    for helper in ('ls_walk_block', 'ls_store_partial', 'ls_fold', 'ls_walk_grid', 'loss_rows', 'loss_v4', 'loss_bwd_grid', 'LTU_DISPATCH_C'):
        assert helper in code, helper
    assert 'loss_imbalance.hip' in open(os.path.join(ROOT, 'lintransunet_amd', 'csrc', 'Makefile')).read()
