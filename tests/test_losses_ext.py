"""The wider training-loss family (csrc/loss_ext.hip, ops.level_loss_ext, losses.LevelCriterion): a float64 torch restatement
of every new loss is pinned to the reference's own values and gradients by tests/golden/losses_ext.npz
(make_golden_losses_ext.py); the registry, the refusals and the C-ABI contract are checked here without a GPU.  The GPU
path is checked against both in test_gpu_losses_ext.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_NAMES = ('DiceLoss', 'IOULoss', 'SSLoss', 'FocalLoss', 'MSELoss', 'ContainLoss', 'ContainLoss2', 'BalanceDiceLoss2',
             'CrossEntroLoss0', 'ClassifyLoss')
ENTRY_POINTS = ('ltu_loss_ext_ws_floats', 'ltu_loss_ext_fwd', 'ltu_loss_ext_bwd')
EPS = 1e-5


# ---------------------------------------------------------------------------------------------- float64 restatement
def restate(name, p, lab, gamma=2.0, sigma=0.05, alpha=None, eps=EPS):
    """float64 restatement of the issue's table: p [B, C, ...] probabilities (any float dtype, autograd-able), lab [B, 1, ...]
    class ids.  Returns the loss as a 0-dim tensor."""
    B, C = p.shape[:2]
    p = p.reshape(B, C, -1).double()
    lab = lab.reshape(B, -1).long().to(p.device)
    S = p.shape[-1]
    t = torch.stack([lab == c for c in range(C)], 1).double()
    P, T, I = p.sum(-1), t.sum(-1), (p * t).sum(-1)
    if name == 'DiceLoss':
        return 1 - ((2 * I + eps) / (P + T + eps)).mean()
    if name == 'IOULoss':
        return 1 - ((I + eps) / (P + T - I)).mean()
    if name == 'SSLoss':
        Q, R = (p * p).sum(-1), (t * p * p).sum(-1)
        return (sigma * (R - 2 * I + T) / (T + eps) + (1 - sigma) * (Q - R) / (S - T + eps)).mean()
    if name == 'FocalLoss':
        lp = torch.where(t > 0, torch.log(torch.where(t > 0, p, torch.ones_like(p))), torch.zeros_like(p))
        return -(t * (1 - p) ** gamma * lp).sum() / (B * S * C)
    if name == 'MSELoss':
        return ((p - t) ** 2).mean()
    if name in ('ContainLoss', 'ContainLoss2'):
        a = alpha if alpha is not None else (0.4 if name == 'ContainLoss' else 0.3)
        return 1 - ((I[:, 1] + eps) / ((1 - a) * (T[:, 1] + eps) + a * (P[:, 1] + eps))).mean()
    if name == 'BalanceDiceLoss2':
        wc = 1 / (T[:, 1:] + eps) ** 2
        return 1 - ((2 * (I[:, 1:] * wc).sum(1) + eps) / (((P[:, 1:] + T[:, 1:]) * wc).sum(1) + eps)).mean()
    if name == 'CrossEntroLoss0':
        p0, t0 = p[:, 0], t[:, 0]
        wa = (S - (p0.sum(-1, keepdim=True) + eps)) / S
        wb = (p0.sum(-1, keepdim=True) - eps) / S
        la = torch.log(torch.clamp(p0, min=1e-6))
        lb = torch.log(torch.clamp(1 - p0, min=1e-6))
        return -(wa * t0 * (1 - p0) * la + wb * (1 - t0) * p0 * lb).sum() / (2 * B * S)
    if name == 'ClassifyLoss':
        m = 1 - t[:, 0]
        y = (torch.arange(C, dtype=p.dtype, device=p.device)[None, :, None] * p).sum(1)
        return (m * (y - lab.double()) ** 2).sum() / (m.sum() + eps)
    if name == 'Recall':
        return ((I[:, 1] + eps) / (T[:, 1] + eps)).mean()
    if name == 'Precision':
        return ((I[:, 1] + eps) / (P[:, 1] + eps)).mean()
    raise KeyError(name)


def golden_cases(G):
    """(case, key, name, params) of every loss in the fixture"""
    out = []
    for k in G.files:
        case, _, rest = k.partition('_')
        if case not in ('c2', 'c2m', 'c3m') or rest in ('p', 'lab') or rest.endswith(('_dp', '_param')):
            continue
        name, _, suffix = rest.partition('_')
        params = {}
        if suffix:
            v = float(G[f'{k}_param'])
            params = {'FocalLoss': {'gamma': v}, 'SSLoss': {'sigma': v}, 'ContainLoss': {'alpha': v}}[name]
        out.append((case, k, name, params))
    return out


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'losses_ext.npz'))


def test_fixture_covers_every_new_name(G):
    names = {name for _, _, name, _ in golden_cases(G)}
    assert names == set(NEW_NAMES) | {'Recall', 'Precision'}
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'losses_ext.npz')) < 1 << 19
    assert int(G['distribution_loss_fails']) == 1           # the reference's own DistributionLoss fails on this input


def test_restatement_matches_reference(G):
    for case, key, name, params in golden_cases(G):
        p = torch.from_numpy(G[f'{case}_p']).double().requires_grad_(True)
        v = restate(name, p, torch.from_numpy(G[f'{case}_lab']), **params)
        ref = float(G[key])
        # MSEcLoss casts to fp32 inside the reference; where the reference adds eps to an integer count (one-hot or label sums:
        # SSLoss, ContainLoss, Recall, ...) torch does that sum in fp32, which moves the value by a few 1e-8
        tol = 1e-6 if name == 'MSELoss' else 1e-7
        assert abs(v.item() - ref) <= tol * max(1.0, abs(ref)), (key, v.item(), ref)
        if f'{key}_dp' in G.files:
            v.backward()
            gref = torch.from_numpy(G[f'{key}_dp']).double()
            err = ((p.grad - gref).norm() / gref.norm()).item()
            assert err < 1e-6, (key, err)                       # the fixture stores the gradient in fp32


def test_get_criterions_serves_the_new_names():
    from lintransunet_amd import losses as L
    crit = L.get_criterions(list(NEW_NAMES) + ['Recall', 'Precision'])
    want = {'DiceLoss': L.DiceLoss, 'IOULoss': L.IOULoss, 'SSLoss': L.SSLoss, 'FocalLoss': L.FocalLoss, 'MSELoss': L.MSEcLoss,
            'ContainLoss': L.ContainLoss, 'ContainLoss2': L.ContainLoss2, 'BalanceDiceLoss2': L.BalanceDiceLoss2,
            'CrossEntroLoss0': L.CrossEntroLoss0, 'ClassifyLoss': L.ClassifyLoss, 'Recall': L.Recall, 'Precision': L.Precision}
    for name, cls in want.items():
        assert type(crit[name]) is cls, name
    assert isinstance(crit['Recall'], L._EvalMetric) and not crit['Recall'].COMPLEMENT
    assert isinstance(crit['Precision'], L._EvalMetric) and not crit['Precision'].COMPLEMENT
    # the reference defaults, and non-default arguments carried to the kernel's parameters
    assert crit['FocalLoss'].impl.params == {'gamma': 2}
    assert crit['SSLoss'].impl.params == {'sigma': 0.05, 'eps': 1e-5}
    assert L.FocalLoss(gamma=3).impl.params == {'gamma': 3}
    assert L.DiceLoss(eps=1e-3).impl.params == {'eps': 1e-3}
    assert L.ContainLoss.ALPHA == 0.4 and L.ContainLoss2.ALPHA == 0.3
    for name in NEW_NAMES:
        assert crit[name].impl.extended, name
    # a spec of the original names only keeps the original kernel
    assert not L.LevelCriterion({'CrossEntroLoss': 1.0, 'DiceClassLoss': 1.0}).extended
    assert L.LevelCriterion({'CrossEntroLoss': 1.0, 'FocalLoss': 0.5}).extended
    with pytest.raises(ValueError):
        L.ContainLoss(class_index=0)
    with pytest.raises(ValueError):
        L.MSEcLoss(reduction='none')


def test_refusals_unchanged():
    from lintransunet_amd import losses as L
    with pytest.raises(KeyError, match='shape error'):
        L.get_criterions(['DistributionLoss'])
    with pytest.raises(KeyError, match='shape error'):
        L.LevelCriterion({'DistributionLoss': 1.0})
    with pytest.raises(KeyError, match='no HIP kernel'):
        L.LevelCriterion({'RegionCrossEntroLoss': 1.0})
    # the multi-class registry is not widened
    with pytest.raises(KeyError, match='IOULoss'):
        L.get_multi_criterions(['DiceClassLoss', 'IOULoss'])
    for name in NEW_NAMES:
        assert name not in L.Multi_Loss_Dict


def test_level_specs_pass_the_new_names():
    from lintransunet_amd import train
    specs = train.level_specs(criterion_list=('FocalLoss', 'IOULoss'))
    assert specs[-1] == {'FocalLoss': 1.0, 'IOULoss': 1.0}
    specs = train.level_specs(criterion_list=('CrossEntroLoss0', 'BalanceDiceLoss2', 'ClassifyLoss'), criterion_weight=[1, 0.5, 0.2])
    assert all(s == {'CrossEntroLoss0': 1, 'BalanceDiceLoss2': 0.5, 'ClassifyLoss': 0.2} for s in specs)


def test_entry_points_declared_and_contract_errors():
    from lintransunet_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and f' {name}(' in header and hasattr(lib, name), name
    for i, term in enumerate(ops.LOSS_EXT_TERMS):
        if not term.startswith('DICE') or term == 'DICE0' or term == 'DICE':      # DICE0 + c: the per-class Dice
            assert f'LTU_LOSS_EXT_{term} = {i}' in header, term
    nt = len(ops.LOSS_EXT_TERMS)
    for i, par in enumerate(ops.LOSS_EXT_PARAMS):
        assert f'LTU_LOSS_EXT_{par.upper()} = {nt + i}' in header, par
    assert f'LTU_LOSS_EXT_NCFG = {nt + len(ops.LOSS_EXT_PARAMS)}' in header
    fake = 1 << 20
    B, S, C = 2, 4096, 3
    need = lib.ltu_loss_ext_ws_floats(B, S, C)
    assert need >= 2 * B * (7 * C + 3)
    cfg = ops.loss_ext_cfg({'FOCAL': 1.0, 'IOU': 0.5})
    fwd = lambda c=C, ws=need, cf=cfg, b=B: lib.ltu_loss_ext_fwd(fake, fake, fake, ws, fake, fake, b, S, c, cf, None, None)
    bwd = lambda c=C, cf=cfg, b=B: lib.ltu_loss_ext_bwd(fake, fake, fake, cf, fake, fake, b, S, c, None)
    assert fwd(c=1) == -2 and fwd(c=5) == -2                                    # LTU_E_SHAPE, nothing launched
    assert bwd(c=1) == -2 and bwd(c=5) == -2
    assert fwd(c=4, b=9, ws=1 << 30) == -2                                      # beyond the finalize's 256 partial rows
    assert fwd(ws=need - 1) == -4                                               # short scratch: LTU_E_ARG
    assert lib.ltu_loss_ext_fwd(fake, fake, None, need, fake, fake, B, S, C, cfg, None, None) == -4
    for k, v in ((ops.LOSS_EXT_TERMS.index('FOCAL'), float('nan')), (nt, float('nan')), (nt + 1, float('inf'))):
        bad = ops.loss_ext_cfg({'FOCAL': 1.0})
        bad[k] = v
        assert fwd(cf=bad) == -4 and bwd(cf=bad) == -4                         # NaN / inf weights or parameters
    assert fwd(cf=None) == -4 and bwd(cf=None) == -4
    absent = ops.loss_ext_cfg({'DICE2': 1.0, 'FOCAL': 1.0})                     # Dice of class 2 at C = 2
    assert fwd(c=2, cf=absent) == -4 and bwd(c=2, cf=absent) == -4
    with pytest.raises(KeyError):
        ops.loss_ext_cfg({'DIST': 1.0})


def test_refuses_dice_of_an_absent_class():
    from lintransunet_amd import losses as L
    crit = L.LevelCriterion({'DiceClassLoss2': 1.0, 'FocalLoss': 1.0})
    with pytest.raises(ValueError, match='DiceClassLoss2'):
        crit(torch.full((1, 2, 4, 4, 4), 0.5), torch.zeros(1, 1, 4, 4, 4, dtype=torch.int64))


def test_rejects_cpu_tensors():
    from lintransunet_amd import _lib, ops
    with pytest.raises(_lib.LtuError):
        ops.level_loss_ext(torch.zeros(1, 8, 2), torch.zeros(1, 8, dtype=torch.uint8), {'FOCAL': 1.0})
