"""The wider training-loss family on the GPU (csrc/loss_ext.hip through ops.level_loss_ext and losses.LevelCriterion): every new
name against the reference's own values and gradients (tests/golden/losses_ext.npz), against the float64 restatement of
test_losses_ext.py over batch sizes, class counts and S % 4, mixed specs against the single losses and against ops.level_loss,
the run-time scale, reproducibility, and a training step (eager and captured) with the new names on the binary and the
multi-class path."""
import os

import numpy as np
import pytest
import torch

from oracle import net as O_net          # noqa: E402
from oracle import seedgen               # noqa: E402
from oracle import step as O_step        # noqa: E402
from tests.test_losses_ext import NEW_NAMES, golden_cases, restate

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SMALL = dict(num_layers=[8, 8, 8, 16, 32], roi_size_list=[20, 12, 9, 10, 6])
PARAM_KW = {'FocalLoss': 'gamma', 'SSLoss': 'sigma'}


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def probs(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(shape, generator=g, dtype=torch.float64) * 1.5, 1).to(dtype)


def labels(B, C, sp, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, C, (B, 1) + sp, generator=g).to(torch.uint8)


def run_module(mod, p, target, **kw):
    """module value and gradient with respect to p [B, C, ...] (fed channels-last as the model produces it)"""
    pd = p.permute(0, *range(2, p.dim()), 1).contiguous().to(DEV).requires_grad_(True)
    v = mod(pd.permute(0, p.dim() - 1, *range(1, p.dim() - 1)), target.to(DEV), **kw)
    v.backward()
    return v.item(), pd.grad.permute(0, p.dim() - 1, *range(1, p.dim() - 1)).detach().cpu()


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'losses_ext.npz'))


def test_every_new_name_matches_reference(G):
    from lintransunet_amd import losses as L
    for case, key, name, params in golden_cases(G):
        p = torch.from_numpy(G[f'{case}_p'])
        lab = torch.from_numpy(G[f'{case}_lab'])
        C = p.shape[1]
        target = lab if case == 'c2' else torch.nn.functional.one_hot(lab[:, 0].long(), C).permute(0, 4, 1, 2, 3).float()
        ref = float(G[key])
        if name in ('Recall', 'Precision'):
            v = L.get_criterions([name])[name](p.to(DEV), target.to(DEV))
            assert abs(v.item() - ref) <= 1e-5 * max(1.0, abs(ref)), key
            continue
        if name == 'ContainLoss' and params:
            mod, kw = L.ContainLoss(), params
        elif params:
            mod, kw = L.Loss_Dict[name](**{PARAM_KW[name]: next(iter(params.values()))}), {}
        else:
            mod, kw = L.get_criterions([name])[name], {}
        v, g = run_module(mod, p, target, **kw)
        assert abs(v - ref) <= 1e-5 * max(1.0, abs(ref)), (key, v, ref)
        assert rel_err(g, torch.from_numpy(G[f'{key}_dp'])) < 1e-4, key


@pytest.mark.parametrize('B', [1, 2, 4])
@pytest.mark.parametrize('C', [2, 3, 4])
@pytest.mark.parametrize('sp', [(12, 10, 8), (9, 7, 5)])
def test_against_restatement(B, C, sp):
    from lintransunet_amd import losses as L
    p = probs((B, C) + sp, 100 * B + C)
    lab = labels(B, C, sp, 7 + B + C)
    for name in NEW_NAMES:
        pr = p.double().requires_grad_(True)
        ref = restate(name, pr, lab)
        ref.backward()
        v, g = run_module(L.get_criterions([name])[name], p, lab)
        assert abs(v - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), (name, v, ref.item())
        assert rel_err(g, pr.grad) < 1e-4, name


def test_level0_shape():
    """2 x 128^3 (the finest level of the benchmarked patch): the vectorised passes over many blocks and the full fold"""
    from lintransunet_amd import losses as L
    sp = (128, 128, 128)
    for C, names in ((2, ('FocalLoss', 'IOULoss', 'SSLoss', 'ContainLoss', 'DiceLoss')),
                     (3, ('CrossEntroLoss0', 'BalanceDiceLoss2', 'ClassifyLoss', 'MSELoss'))):
        p = probs((2, C) + sp, 11 + C)
        lab = labels(2, C, sp, 12 + C)
        for name in names:
            pr = p.double().requires_grad_(True)
            ref = restate(name, pr, lab)
            ref.backward()
            v, g = run_module(L.get_criterions([name])[name], p, lab)
            assert abs(v - ref.item()) <= 1e-4 * max(1.0, abs(ref.item())), (name, v, ref.item())
            assert rel_err(g, pr.grad) < 1e-4, name


def test_eps_zero_against_restatement():
    """a non-default eps of 0 reaches the kernel; the terms switched off (whose values are 0/0 there) must not leak into the loss"""
    from lintransunet_amd import losses as L
    sp = (12, 10, 8)
    p = probs((2, 3) + sp, 71)
    lab = labels(2, 3, sp, 72)
    for name in ('DiceLoss', 'IOULoss', 'SSLoss', 'BalanceDiceLoss2', 'CrossEntroLoss0', 'ClassifyLoss', 'ContainLoss'):
        pr = p.double().requires_grad_(True)
        ref = restate(name, pr, lab, eps=0.0)
        ref.backward()
        v, g = run_module(L.Loss_Dict[name](eps=0.0), p, lab)
        assert np.isfinite(v) and torch.isfinite(g).all(), name
        assert abs(v - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), (name, v, ref.item())
        assert rel_err(g, pr.grad) < 1e-4, name


def test_switched_off_term_with_infinite_value():
    """class 2 absent from sample 0 on both sides (P = T = 0): the IoU of that (b, c) is eps / 0 = inf.  A spec without IOULoss
    must still give the finite loss and gradient of its own terms"""
    from lintransunet_amd import losses as L
    sp = (12, 10, 8)
    p = probs((2, 3) + sp, 81)
    p[0, :2] = probs((1, 2) + sp, 82)[0]
    p[0, 2] = 0.0
    lab = labels(2, 3, sp, 83)
    lab[0] = lab[0] % 2
    for name in ('DiceLoss', 'FocalLoss', 'SSLoss', 'MSELoss', 'CrossEntroLoss0'):
        pr = p.double().requires_grad_(True)
        ref = restate(name, pr, lab)
        ref.backward()
        v, g = run_module(L.get_criterions([name])[name], p, lab)
        assert np.isfinite(v) and torch.isfinite(g).all(), name
        assert abs(v - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), (name, v, ref.item())
        assert rel_err(g, pr.grad) < 1e-4, name
    pd = _cl(p).requires_grad_(True)
    tot, named = L.LevelCriterion({'DiceLoss': 1.0, 'CrossEntroLoss': 0.5})(pd.permute(0, 4, 1, 2, 3), lab.to(DEV))
    tot.backward()
    assert torch.isfinite(tot) and torch.isfinite(pd.grad).all() and set(named) == {'DiceLoss', 'CrossEntroLoss'}


def test_focal_gradient_at_p_one():
    """gamma < 1: a labelled voxel with p == 1 exactly has the limit 0 as its focal gradient (the reference's autograd: NaN)"""
    from lintransunet_amd import losses as L
    sp = (12, 10, 8)
    p = probs((2, 2) + sp, 91)
    lab = labels(2, 2, sp, 92)
    sure = torch.zeros((2,) + sp, dtype=torch.bool)
    sure[:, ::3] = True
    onehot = torch.nn.functional.one_hot(lab[:, 0].long(), 2).permute(0, 4, 1, 2, 3).float()
    p = torch.where(sure[:, None], onehot, p)
    pr = p.double().requires_grad_(True)
    ref = restate('FocalLoss', pr, lab, gamma=0.5)
    ref.backward()
    v, g = run_module(L.FocalLoss(gamma=0.5), p, lab)
    assert torch.isfinite(g).all()
    assert abs(v - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    assert (g.permute(0, 2, 3, 4, 1)[sure] == 0).all()
    keep = ~sure[:, None].expand_as(g)
    assert rel_err(g[keep], pr.grad[keep]) < 1e-4


def _cl(p):
    return p.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def test_mixed_specs_and_old_terms():
    from lintransunet_amd import losses as L, ops
    sp = (16, 12, 10)
    for C in (2, 3):
        p = probs((2, C) + sp, 31 + C)
        lab = labels(2, C, sp, 41 + C)
        spec = {'CrossEntroLoss': 1.0, 'DiceClassLoss': 0.7, 'FocalLoss': 0.5, 'IOULoss': 2.0, 'BalanceDiceLoss2': 0.3,
                'CrossEntroLoss0': 1.5, 'ClassifyLoss': 0.2, 'DiceClassLoss0': 0.4, 'BalanceDiceLoss': 0.6, 'ContainLoss': 0.25}
        pd = _cl(p).requires_grad_(True)
        tot, named = L.LevelCriterion(spec, scale=0.8)(pd.permute(0, 4, 1, 2, 3), lab.to(DEV))
        tot.backward()
        want, gwant = 0.0, torch.zeros_like(pd)
        for name, w in spec.items():
            ps = _cl(p).requires_grad_(True)
            v = L.Loss_Dict[name]()(ps.permute(0, 4, 1, 2, 3), lab.to(DEV))
            v.backward()
            want += 0.8 * w * v.item()
            gwant += 0.8 * w * ps.grad
            assert abs(named[name].item() - w * v.item()) <= 1e-5 * max(1.0, abs(w * v.item())), name
        assert abs(tot.item() - want) <= 1e-5 * max(1.0, abs(want)), (C, tot.item(), want)
        assert rel_err(pd.grad, gwant) < 1e-5
        # the original terms carried by the new family agree with ops.level_loss
        wce, wbal, wd = 1.0, 0.6, [0.1, 0.7, 0.3 if C > 2 else 0.0, 0.0, 0.4]      # no Dice of an absent class
        lab_u8 = L._labels(lab.to(DEV), C)
        pa = _cl(p).requires_grad_(True)
        ta, va = ops.level_loss(pa, lab_u8, wce, wbal, wd)
        ta.backward()
        pb = _cl(p).requires_grad_(True)
        tb, vb = ops.level_loss_ext(pb, lab_u8, {'CE': wce, 'BAL': wbal, 'DICE0': wd[0], 'DICE1': wd[1], 'DICE2': wd[2], 'FG': wd[4]})
        tb.backward()
        assert abs(ta.item() - tb.item()) <= 1e-6 * max(1.0, abs(ta.item()))
        for i in (1, 2, 3, 4, 7) + ((5,) if C > 2 else ()):
            assert abs(va[i].item() - vb[i].item()) <= 1e-6, i
        assert rel_err(pb.grad, pa.grad) < 1e-6
        # a spec of the original names only is still the original kernel, bit for bit
        old = {'CrossEntroLoss': 1.0, 'DiceClassLoss': 1.0}
        pc = _cl(p).requires_grad_(True)
        tc, _ = L.LevelCriterion(old, scale=0.5)(pc.permute(0, 4, 1, 2, 3), lab.to(DEV))
        tc.backward()
        pe = _cl(p).requires_grad_(True)
        te, _ = ops.level_loss(pe, lab_u8, 0.5, 0.0, [0.0, 0.5, 0.0, 0.0, 0.0])
        te.backward()
        assert torch.equal(tc, te) and torch.equal(pc.grad, pe.grad)


def test_scale_dev_and_reproducibility():
    from lintransunet_amd import losses as L
    sp = (20, 16, 12)
    p = probs((2, 3) + sp, 51)
    lab = labels(2, 3, sp, 52)
    spec = {'FocalLoss': 1.0, 'SSLoss': 0.5, 'ClassifyLoss': 0.3, 'CrossEntroLoss0': 1.0, 'CrossEntroLoss': 1.0}

    def run(**kw):
        pd = _cl(p).requires_grad_(True)
        t, named = L.LevelCriterion(spec, **kw)(pd.permute(0, 4, 1, 2, 3), lab.to(DEV))
        t.backward()
        return t.detach().clone(), pd.grad.clone(), {k: v.clone() for k, v in named.items()}

    t1, g1, n1 = run(scale=0.4)
    t2, g2, _ = run(scale_dev=torch.tensor([0.4], device=DEV))
    assert abs(t1.item() - t2.item()) <= 1e-6 * abs(t1.item()) and rel_err(g2, g1) < 1e-6
    t3, g3, n3 = run(scale=0.4)
    assert torch.equal(t1, t3) and torch.equal(g1, g3)                 # no atomics: bit-identical
    assert all(torch.equal(n1[k], n3[k]) for k in n1)


def _build(cfg, seed):
    from lintransunet_amd.model import get_model_dict
    m = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, cfg.dim_input, cfg.dim_output, dropout=0.0)
    m.load_state_dict(seedgen.seeded_params(O_net.param_shapes(cfg), seed), strict=True)
    return m.to(DEV).train()


def _grads_agree(a, b):
    """two runs of the same small fp32 step (test_gpu_model.grads_agree: InstanceNorm statistics use fp32 atomics)"""
    return (a - b).double().norm().item() <= 5e-3 * max(b.double().norm().item(), 1e-6)


@pytest.mark.parametrize('case', ['binary', 'multi'])
def test_train_step_and_graphed_step(case):
    from lintransunet_amd import train
    from lintransunet_amd.losses import LevelCriterion
    if case == 'binary':
        cfg = O_net.NetConfig(**SMALL)
        specs = train.level_specs(5, criterion_list=('FocalLoss', 'IOULoss'))
        label = seedgen.seeded_label((2, 1, 32, 32, 32), 602).to(DEV)
    else:
        cfg = O_net.NetConfig(dim_output=3, **SMALL)
        specs = train.level_specs(5, ('CrossEntroLoss0', 'BalanceDiceLoss2', 'ClassifyLoss'), criterion_weight=[10, 1, 2])
        label = seedgen.seeded_label((2, 1, 32, 32, 32), 602, n_classes=3).to(DEV)
    x = seedgen.seeded_volume((2, 1, 32, 32, 32), 601).to(DEV)
    w = O_step.dynamic_weights(0)
    m = _build(cfg, 600)
    totals, named = train.train_step(m, x, label, w, specs=specs)
    torch.cuda.synchronize()
    eager = [t.item() for t in totals]
    assert all(np.isfinite(eager))
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    assert grads and all(torch.isfinite(g).all() for g in grads.values())
    assert set(named[0]) == set(specs[-1])
    # the level totals are LevelCriterion on the model's outputs
    predict, masks = m(x)
    pyr = train.label_pyramid(label, 5)
    for lvl in range(5):
        pred = predict if lvl == 0 else masks[-lvl]
        want, _ = LevelCriterion(specs[-lvl - 1], scale=w[lvl])(pred.detach(), pyr[lvl].reshape(pred.shape[0], 1, *pred.shape[2:]))
        assert abs(want.item() - eager[lvl]) <= 1e-4 * max(1.0, abs(eager[lvl])), (lvl, want.item(), eager[lvl])
    # the captured step replays the same losses and gradients
    m2 = _build(cfg, 600)
    red = train.GradReducer(m2, bucket_mb=0.5, unused=train.UNUSED_PARAMETERS)
    g = train.GraphedStep(m2, x, label, w, red, specs=specs)
    for _ in range(2):
        tg, _ = g(x, label)
    torch.cuda.synchronize()
    got = [t.item() for t in tg]
    for a, b in zip(got, eager):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (got, eager)
    pm = dict(m2.named_parameters())
    for k, r in grads.items():
        assert torch.isfinite(pm[k].grad).all(), k
        if k.endswith('.bias') and any(t in k for t in ('.conv1.', '.conv2.', 'input_block', 'down_embed', 'up_embed', 'W_x.0', 'W_g.0',
                                                          'self_attn.linears.1.')):
            assert (pm[k].grad - r).abs().max().item() <= 1e-5, k          # analytically zero: rounding residue only
            continue
        assert _grads_agree(pm[k].grad, r), k
