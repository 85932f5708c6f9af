"""Soft morphology, soft skeleton, label skeletons and the soft-clDice stage on the GPU (csrc/softmorph.hip) against the oracles of
tests/cldice_common.py: the published composition on tie-free noise (on which no tie rule can change a gradient,
tests/test_cldice.py), the rule oracle on plateaus; the stage inside the loss chain, the scratch contract, graph capture and a
training step (eager and captured).

Allowance: 4 x the deviation of the same oracle evaluated in float32 from its float64 evaluation, on the test's own input, with a
floor of 4 fp32 ulps of the value (of the field's largest magnitude for gradients and skeletons).  The kernels have no tile: every
launch is a flat walk of 256-thread workgroups, so 37 x 22 x 70 gives 223 workgroups with a ragged last one."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import net as O_net          # noqa: E402
from oracle import seedgen               # noqa: E402
from oracle import step as O_step        # noqa: E402
from tests.cldice_common import (SHAPES, blob_labels, field_allowance, field_error, noise, noise_probs, plateau_case, pub_cldice,
                                 pub_label_skeletons, pub_op, rule_cldice, value_allowance)
from tests.test_gpu_structure import _compare as compare_gradients
from tests.topk_common import make_labels, make_probs

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ITERS = (1, 3, 6)
SMALL = dict(num_layers=[8, 8, 8, 16, 32], roi_size_list=[20, 12, 9, 10, 6])      # of tests/test_gpu_boundary.py


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------- 1. the operators
@pytest.mark.parametrize('B,spatial', SHAPES)
@pytest.mark.parametrize('name,iters', [('erode', None), ('dilate', None)] + [('skeleton', i) for i in ITERS])
def test_operators_against_the_published_composition(name, iters, B, spatial):
    from lintransunet_amd import ops
    x = noise((B,) + spatial, 31)
    g = np.random.default_rng(32).standard_normal(x.shape).astype(np.float32)
    y64, dx64 = pub_op(name, x, g, iters)
    y32, dx32 = pub_op(name, x, g, iters, torch.float32)
    xt = _t(x).requires_grad_(True)
    y = {'erode': ops.soft_erode, 'dilate': ops.soft_dilate}[name](xt) if iters is None else ops.soft_skeleton(xt, iters)
    y.backward(_t(g))
    ey, eg = field_error(y.detach().cpu().numpy(), y64), field_error(xt.grad.cpu().numpy(), dx64)
    ay, ag = field_allowance(y64, y32), field_allowance(dx64, dx32)
    print(f'{name} {iters} B={B} {spatial}: forward {ey:.2e} (allowed {ay:.2e}), gradient {eg:.2e} (allowed {ag:.2e})')
    assert ey <= ay and eg <= ag
    if iters is None:
        assert np.array_equal(y.detach().cpu().numpy(), y64.astype(np.float32))      # a copy of one input voxel
    # a second call: bit for bit
    x2 = _t(x).requires_grad_(True)
    y2 = {'erode': ops.soft_erode, 'dilate': ops.soft_dilate}[name](x2) if iters is None else ops.soft_skeleton(x2, iters)
    y2.backward(_t(g))
    assert torch.equal(y2, y) and torch.equal(x2.grad, xt.grad)


@pytest.mark.parametrize('B,spatial', SHAPES)
@pytest.mark.parametrize('iters', ITERS)
def test_label_skeletons_byte_for_byte(iters, B, spatial):
    from lintransunet_amd import ops
    lab = blob_labels(B, spatial, 3, 41)
    lab[0][lab[0] == 2] = 4                      # class 2 absent from sample 0's label, class 3 from all of it
    classes = (1, 0, 3, 2, 4)
    got = ops.label_skeletons(_t(lab), classes, iters)
    want = pub_label_skeletons(lab, classes, iters)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want.astype(np.uint8))
    assert want[:, 2].sum() == 0
    full = np.full((B,) + spatial, 5, np.uint8)   # a class that fills the patch
    got = ops.label_skeletons(_t(full), (5, 1), iters)
    assert np.array_equal(got.cpu().numpy(), pub_label_skeletons(full, (5, 1), iters).astype(np.uint8))
    assert torch.equal(ops.label_skeletons(_t(full), (5, 1), iters), got)


# ---------------------------------------------------------------------------------------------- 2. the stage
def _stage(p, lab, classes, weights, iters, **kw):
    from lintransunet_amd import ops
    pt = _t(p).requires_grad_(True)
    total, _, values = ops.level_loss_cldice(pt, _t(lab), classes, weights, iters, **kw)
    total.backward()
    return total.item(), values.cpu().numpy().astype(np.float64), pt.grad.cpu().numpy()


def _compare(tag, got, ref64, ref32):
    (total, values, dp), (t64, v64, d64), (t32, v32, d32) = got, ref64, ref32
    ev = [abs(total - t64)] + list(np.abs(values - v64))
    av = [value_allowance(t64, t32)] + [value_allowance(a, b) for a, b in zip(v64, v32)]
    eg, ag = field_error(dp, d64), field_allowance(d64, d32)
    print(f'{tag}: total {total:.8f} oracle {t64:.8f}; value errors {["%.2e" % e for e in ev]} allowed {["%.2e" % a for a in av]}; '
          f'gradient {eg:.2e} allowed {ag:.2e}')
    assert all(e <= a for e, a in zip(ev, av)) and eg <= ag


@pytest.mark.parametrize('B,spatial', SHAPES)
@pytest.mark.parametrize('iters', ITERS)
@pytest.mark.parametrize('classes', [(1, 2), (2, 1)])
def test_stage_against_the_published_composition(classes, iters, B, spatial):
    """Measured on the MI355X over the 24 cases (totals 0.80 - 1.42, values 0.57 - 0.95): value and total errors <= 9.0e-8 (smallest
    allowance 2.4e-7), gradient <= 1.7e-7 of its maximum (smallest allowance 4.8e-7).  The operators' test above: skeleton <= 9.9e-8
    of its maximum, its gradient <= 2.3e-7, erode / dilate forward exact, gradient <= 1.7e-7.  Plateaus: value 4.6e-9, gradient
    3.7e-8."""
    p, lab = noise_probs(B, spatial, 3, 51), blob_labels(B, spatial, 3, 52)
    weights = (1.0, 0.5)
    got = _stage(p, lab, classes, weights, iters)
    _compare(f'{classes} iters {iters} B={B} {spatial}', got, pub_cldice(p, lab, classes, weights, iters)[:3],
             pub_cldice(p, lab, classes, weights, iters, torch.float32)[:3])
    assert not got[2][..., 0].any()               # nothing goes to a channel no term names


def test_absent_class_gives_tsens_one():
    p = noise_probs(1, (9, 7, 5), 3, 53)
    lab = np.zeros((1, 9, 7, 5), np.uint8)
    _compare('class absent from the label', _stage(p, lab, (1,), (1.0,), 3), pub_cldice(p, lab, (1,), (1.0,), 3)[:3],
             pub_cldice(p, lab, (1,), (1.0,), 3, torch.float32)[:3])


@pytest.mark.parametrize('iters', ITERS)
def test_plateaus_against_the_rule(iters):
    p, lab = plateau_case()
    classes, weights = (1, 2), (1.0, 0.5)
    *ref64, m64 = rule_cldice(p, lab, classes, weights, iters)
    *ref32, m32 = rule_cldice(p, lab, classes, weights, iters, np.float32)
    # a condition on the input, not a tolerance: no relu mask depends on the precision, at any voxel and iteration
    assert all(np.array_equal(a, b) for a, b in zip(m64, m32))
    _compare(f'plateaus iters {iters}', _stage(p, lab, classes, weights, iters), ref64, ref32)


# ---------------------------------------------------------------------------------------------- 3. the chain
FAMILIES = {'orig': 4, 'wide': 5, 'ext': 3}
CLD = ((1, 2), (0.6, 0.4), 3)


@functools.lru_cache(maxsize=None)
def _chain_inputs(B, spatial, C):
    from lintransunet_amd import ops
    p = torch.from_numpy(make_probs(B, spatial, C, 7 * B + C)).to(DEV)
    lab = torch.from_numpy(make_labels(B, spatial, C, 9 * B + C)).to(DEV)
    return p, lab, ops.signed_distance_maps(lab, (1, 2), (1.0, 1.0, 2.0))


def _chain_stage(family, name, phi):
    from lintransunet_amd import ops
    if name == 'cldice':
        return (None, *CLD)
    if name == 'boundary':
        return (phi, (1, 2), (0.05, 0.02), None)
    if name == 'topk':
        return (0.7, 0.2, None)
    if name == 'imbalance':
        return (((1, 2), (0.6, 0.4), {'gamma': 4.0 / 3.0}), (0.5, 2.0, None))
    if family == 'ext':
        return ('ltu_loss_ext', ops.loss_ext_cfg({'CE': 1.0, 'FOCAL': 1.0, 'DICE': 0.5}))
    wd = (0.0, 1.0, 1.0, 0.5, 0.5) if family == 'orig' else (0.0, 1.0, 1.0, 0.0, 1.0, 0.5)
    return ('ltu_loss' if family == 'orig' else 'ltu_loss_wide', (10.0, 0.5, wd))


def _chain_run(family, stages, B, spatial):
    from lintransunet_amd import ops
    p, lab, phi = _chain_inputs(B, spatial, FAMILIES[family])
    pg = p.clone().requires_grad_(True)
    total, *reports = ops.level_loss_chain(pg, lab, **{s: _chain_stage(family, s, phi) for s in stages})
    total.backward()
    return total.detach(), pg.grad, reports


@functools.lru_cache(maxsize=None)
def _chain_alone(family, stage, B, spatial):
    return _chain_run(family, (stage,), B, spatial)


ALL = ('base', 'boundary', 'topk', 'imbalance', 'cldice')


@pytest.mark.parametrize('B,spatial', SHAPES[:2])
@pytest.mark.parametrize('family,stages', [(f, s) for f in FAMILIES for s in (('base', 'cldice'), ALL)])
def test_chain_is_the_sum_of_its_stages(family, stages, B, spatial):
    total, grad, reports = _chain_run(family, stages, B, spatial)
    alone = [_chain_alone(family, s, B, spatial) for s in stages]
    assert len(reports) == len(ALL)
    for k, name in enumerate(ALL):
        if name not in stages:
            assert reports[k] is None
        else:
            assert not reports[k].requires_grad and torch.equal(reports[k], alone[stages.index(name)][2][k]), name
    want = sum(t.item() for t, _, _ in alone)
    assert abs(want) >= 0.5 * sum(abs(t.item()) for t, _, _ in alone)
    gsum = sum(g.double() for _, g, _ in alone)
    eg = (grad.double() - gsum).abs().max().item() / gsum.abs().max().item()
    print(f'{family} {"+".join(stages)} B={B} {spatial}: total {total.item():.8f} separate {want:.8f}, gradient max |diff| / max {eg:.2e}')
    assert abs(total.item() - want) <= 1e-6 * abs(want)
    assert eg <= 1e-6
    total2, grad2, reports2 = _chain_run(family, stages, B, spatial)
    assert torch.equal(total2, total) and torch.equal(grad2, grad)
    assert all(a is None if b is None else torch.equal(a, b) for a, b in zip(reports2, reports))


# ---------------------------------------------------------------------------------------------- 4. the scratch contract
def test_short_scratch_is_refused_before_any_launch():
    from lintransunet_amd import _lib, ops
    B, (H, W, D), C, K, iters = 1, (9, 7, 5), 3, 2, 3
    p, lab = _t(noise_probs(B, (H, W, D), C, 61)), _t(blob_labels(B, (H, W, D), C, 62))
    skel = ops.label_skeletons(lab, (1, 2), iters)
    lib = _lib.load()
    need = lib.ltu_loss_cldice_scratch_elems(B, H, W, D, K, iters)
    assert need > 0 and lib.ltu_loss_cldice_scratch_elems(B, H, W, D, K, 11) == 0
    scratch = torch.full((need,), 7.0, device=DEV)
    values, dp = torch.full((K + 1,), -5.0, device=DEV), torch.full_like(p, -5.0)
    cls, w = (ctypes.c_int * K)(1, 2), (ctypes.c_float * K)(1.0, 0.5)
    one = torch.ones(1, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
        _lib.call('ltu_loss_cldice_fwd', p.data_ptr(), lab.data_ptr(), skel.data_ptr(), cls, w, K, iters, scratch.data_ptr(), need - 1,
                  values.data_ptr(), 0, 0, B, H, W, D, C, s)
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
        _lib.call('ltu_loss_cldice_bwd', p.data_ptr(), lab.data_ptr(), cls, K, iters, scratch.data_ptr(), need - 1, one.data_ptr(),
                  dp.data_ptr(), 0, B, H, W, D, C, s)
    x = p[..., 1].contiguous()
    y = torch.full_like(x, -5.0)
    sneed = lib.ltu_soft_skeleton_scratch_elems(B, H, W, D, iters)
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
        _lib.call('ltu_soft_skeleton_fwd', x.data_ptr(), y.data_ptr(), scratch.data_ptr(), sneed - 1, B, H, W, D, iters, s)
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
        _lib.call('ltu_soft_skeleton_bwd', x.data_ptr(), x.data_ptr(), y.data_ptr(), scratch.data_ptr(), sneed - 1, B, H, W, D, iters, s)
    torch.cuda.synchronize()
    assert (scratch == 7.0).all() and (values == -5.0).all() and (dp == -5.0).all() and (y == -5.0).all()      # nothing was launched


# ---------------------------------------------------------------------------------------------- 5. capture
def test_capture_replays_the_eager_bytes():
    from lintransunet_amd import losses as L, ops
    spec = {'CrossEntroLoss': 1.0, 'ClDiceLoss': 1.0, 'ClDiceLoss2': 0.5}
    B, spatial, C = 2, (12, 10, 8), 3
    inputs = [(_t(make_probs(B, spatial, C, 70 + i)).permute(0, 4, 1, 2, 3).contiguous(),
               _t(blob_labels(B, spatial, C, 80 + i)).unsqueeze(1)) for i in range(2)]
    crit = L.LevelCriterion(spec, cldice_iters=3)

    def run(p, lab):
        total, named = crit(p, lab)
        total.backward()
        return total, named, ops.label_skeletons(lab[:, 0], (1, 2), 3)

    ps, labs = inputs[0][0].clone().requires_grad_(True), inputs[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(ps, labs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ps.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        total_s, named_s, skel_s = run(ps, labs)
    seen = []
    for p, lab in (inputs[1], inputs[0]):
        with torch.no_grad():
            ps.copy_(p)
        labs.copy_(lab)
        graph.replay()
        torch.cuda.synchronize()
        pe = p.clone().requires_grad_(True)
        total_e, named_e, skel_e = run(pe, lab)
        torch.cuda.synchronize()
        assert torch.equal(total_s, total_e) and torch.equal(ps.grad, pe.grad) and torch.equal(skel_s, skel_e)
        assert all(torch.equal(named_s[k], named_e[k]) for k in spec)
        seen.append(total_s.item())
    assert seen[0] != seen[1]


# ---------------------------------------------------------------------------------------------- 6. the training step
def _build(act_dtype):
    from lintransunet_amd import train
    from lintransunet_amd.model import get_model_dict
    cfg = O_net.NetConfig(dim_output=3, **SMALL)
    m = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, cfg.dim_input, cfg.dim_output, dropout=0.0,
                                        act_dtype=act_dtype)
    m.load_state_dict(seedgen.seeded_params(O_net.param_shapes(cfg), 900), strict=True)
    m = m.to(DEV).train()
    return m, train.GradReducer(m, bucket_mb=32.0, unused=train.UNUSED_PARAMETERS)


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


# fp32 steps: two identical eager steps of a spec WITHOUT the name already differ in every gradient (none of this stage's kernels
# launched; observed rel-L2 1e-7 .. 2e-7 on weights), i.e. the fp32 weight-gradient sums are taken in an order that varies from run to
# run.  A weight-gradient element is an fp32 sum of up to n = 2 * 32^3 * 27 = 1.8e6 products; two orders of such a sum agree to about
# 2^-24 sqrt(n) = 8e-5 of the sum of the magnitudes, which bounds the rel-L2 of the whole tensor.  A bias gradient in front of an
# InstanceNorm is analytically zero (tests/test_gpu_structure.py, ANALYTIC_ZERO) and what is computed is the residue of that sum, so
# every bias is held against the norm of its module's weight gradient.
TOL_F32 = 1e-4


def _rel(g, r, ref, k):
    partner = ref.get(k[:-len('bias')] + 'weight') if k.endswith('.bias') else None
    floor = partner.norm().item() if partner is not None else 0.0
    return (g.double() - r.double()).norm().item() / max(r.norm().item(), floor, 1e-30)


def _close_gradients(got, ref, tag):
    """every parameter gradient to rel-L2 <= TOL_F32 of its own norm (a bias: of its module's weight gradient, if larger)"""
    assert set(got) == set(ref)
    errs = {k: _rel(got[k], r, ref, k) for k, r in ref.items()}
    worst = max(errs, key=errs.get)
    print(f'[{tag}] worst rel-L2 {errs[worst]:.2e} ({worst}), {sum(e == 0.0 for e in errs.values())} / {len(errs)} bit-equal')
    bad = {k: e for k, e in errs.items() if not e <= TOL_F32}
    assert not bad, (tag, bad)


@pytest.mark.parametrize('act_dtype', [torch.float32, torch.bfloat16])
def test_train_step_and_graphed_step(act_dtype, monkeypatch):
    """Level totals (the forward) are compared bit for bit in both dtypes.  Gradients: in bf16 the way tests/test_gpu_structure.py
    compares two runs (bit-equal here), in fp32 to TOL_F32 (above); in both the change the name causes must exceed 10 x TOL_F32."""
    from lintransunet_amd import train
    check = compare_gradients if act_dtype == torch.bfloat16 else _close_gradients
    x = seedgen.seeded_volume((2, 1, 32, 32, 32), 901).to(DEV)
    label = seedgen.seeded_label((2, 1, 32, 32, 32), 902, n_classes=3).to(DEV)
    w = O_step.dynamic_weights(0)
    plain = train.level_specs(5, ('CrossEntroLoss', 'DiceClassLoss'))
    specs = list(plain)
    specs[-1] = dict(plain[-1], ClDiceLoss=0.5)              # the finest level's spec (deep_supervision_loss reads specs[-lvl - 1])
    m, red = _build(act_dtype)
    level_scale = torch.tensor(w, device=DEV, dtype=torch.float32)

    def eager(sp, **kw):
        for _ in range(2):
            red.zero_grad()
            totals, named = train.train_step(m, x, label, w, specs=sp, reducer=red, level_scale=level_scale, **kw)
        torch.cuda.synchronize()
        return [t.item() for t in totals], named, _grads(m)

    tot_e, named, g_eager = eager(specs, cldice_iters=2)
    assert all(torch.isfinite(g).all() for g in g_eager.values()) and all(np.isfinite(tot_e))
    assert 'ClDiceLoss' in named[0] and all('ClDiceLoss' not in n for n in named[1:])
    assert 0.0 < named[0]['ClDiceLoss'].item() < 0.5
    # a spec without the name: the bits it gives do not depend on the unused argument, and the name does change level 0 alone
    tot_p, _, g_plain = eager(plain)
    tot_q, _, g_q = eager(plain, cldice_iters=7)
    assert tot_p == tot_q
    check(g_q, g_plain, 'spec without the name, cldice_iters passed and unused')
    moved = max(_rel(g_eager[k], g_plain[k], g_plain, k) for k in g_plain)
    print(f'largest rel-L2 change of a gradient with the name: {moved:.2e}')
    assert moved >= 10 * TOL_F32                                                  # the name reaches the parameters, above the noise
    assert tot_p[0] != tot_e[0] and tot_p[1:] == tot_e[1:]
    # the captured step without the weight-gradient queue: the same kernels on one stream, bit for bit
    monkeypatch.setenv('LTU_WQ', '0')
    step = train.GraphedStep(m, x, label, w, red, specs=specs, cldice_iters=2)
    assert step.wq_stream is None and step.cldice_iters == 2
    tot_g, _ = step(x, label)
    torch.cuda.synchronize()
    assert [t.item() for t in tot_g] == tot_e
    check(_grads(m), g_eager, 'captured against eager')
