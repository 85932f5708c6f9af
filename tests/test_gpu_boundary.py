"""Boundary loss on the GPU: the signed distance maps of csrc/distmap.hip against scipy, the loss kernels of
csrc/loss_boundary.hip against float64, losses.LevelCriterion with a boundary name on each of the three loss families, the whole
thing under graph capture, and a training step (eager and captured) with the term at all five levels.  The float64 restatement
and the label volumes are tests/boundary_common.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import losses as O_loss      # noqa: E402
from oracle import net as O_net          # noqa: E402
from oracle import seedgen               # noqa: E402
from oracle import step as O_step        # noqa: E402
from tests.boundary_common import boundary_grad_ref, boundary_values_ref, make_labels, phi_ref_batch
from tests.manyclass_common import onehot

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SMALL = dict(num_layers=[8, 8, 8, 16, 32], roi_size_list=[20, 12, 9, 10, 6])
CLASSES = (1, 2, 3)
# odd extents; an axis longer than a wave and than 128; the 512 limit; lines with no source (class 3, and most lines of the others)
SHAPES = [(37, 20, 9), (130, 5, 3), (512, 3, 2), (9, 6, 67)]
SPACINGS = [(1.0, 1.0, 1.0), (0.7, 0.7, 2.5)]


@functools.lru_cache(maxsize=None)
def _case(shape, spacing):
    lab = make_labels(shape)
    # the kernel takes the spacing as fp32: the reference measures with the same numbers
    sp32 = tuple(float(np.float32(s)) for s in spacing)
    ref = phi_ref_batch(lab, CLASSES, sp32)
    ref.setflags(write=False)
    return lab, ref


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


# ---------------------------------------------------------------------------------------------- 1. maps against scipy
@pytest.mark.parametrize('spacing', SPACINGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_maps_against_scipy(shape, spacing):
    from lintransunet_amd import ops
    lab, ref = _case(shape, spacing)
    assert lab[0, -1, -1, -1] == 1 and not (lab[0] == 3).any() and (lab[1] == 3).all()
    d = torch.from_numpy(lab).to(DEV)
    phi = ops.signed_distance_maps(d, CLASSES, spacing)
    again = ops.signed_distance_maps(d, CLASSES, spacing)
    torch.cuda.synchronize()
    assert phi.shape == (2, 3) + shape and phi.dtype == torch.float32
    assert torch.equal(phi, again)                                 # bit-identical
    got = phi.cpu().numpy()
    assert np.isfinite(got).all()
    assert not got[0, 2].any() and not got[1].any()               # class 3 absent / filling: exactly 0, as are classes 1, 2 of sample 1
    if spacing == (1.0, 1.0, 1.0):
        ref32 = ref.astype(np.float32)
        ulps = np.abs(got.astype(np.float64) - ref32.astype(np.float64)) / np.spacing(np.abs(ref32)).astype(np.float64)
        print(f'{shape} unit spacing: worst error {ulps.max():.2f} ulp')
        assert ulps.max() <= 1.0, np.unravel_index(ulps.argmax(), ulps.shape)
    else:
        err = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
        print(f'{shape} spacing {spacing}: worst relative error {err.max():.3e}')
        assert err.max() <= 1e-6, np.unravel_index(err.argmax(), err.shape)


def test_maps_of_random_labels_three_samples():
    """every voxel its own region, B = 3, K = 8 (class 7 absent), class order shuffled: the volume index of every pass"""
    from lintransunet_amd import ops
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 7, (3, 11, 70, 13)).astype(np.uint8)
    lab[1, 2:9, 10:50, 3:11] = 4
    classes = (4, 0, 7, 2, 1, 6, 3, 5)
    ref = phi_ref_batch(lab, classes, (0.5, 0.5, 2.0))
    got = ops.signed_distance_maps(torch.from_numpy(lab).to(DEV), classes, (0.5, 0.5, 2.0)).cpu().numpy()
    assert not got[:, 2].any()
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    assert err.max() <= 1e-6, np.unravel_index(err.argmax(), err.shape)


# ---------------------------------------------------------------------------------------------- 2. loss kernels against float64
def _probs(B, C, sp, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn((B,) + sp + (C,), generator=g, dtype=torch.float64) * 1.5, -1).float()      # channels-last


def _blocky_labels(B, C, sp, seed):
    """labels 0 .. C-1 in blocks of about a quarter of each axis: real interiors and boundaries for every class"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, C, (B, 4, 4, 3))
    idx = [np.minimum(np.arange(n) * k // n, k - 1) for n, k in zip(sp, (4, 4, 3))]
    return np.ascontiguousarray(coarse[:, idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]].astype(np.uint8))


def _ptr(t):
    return 0 if t is None else t.data_ptr()


@pytest.mark.parametrize('C,classes', [(3, (1,)), (3, (1, 2)), (5, (0, 4))])
def test_loss_kernels_against_float64(C, classes):
    from lintransunet_amd import _lib, ops
    B, sp = 2, (37, 20, 9)
    S, K = 37 * 20 * 9, len(classes)
    p = _probs(B, C, sp, 10 + C + K)
    lab = _blocky_labels(B, C, sp, 20 + C)
    phi64 = phi_ref_batch(lab, classes, (0.7, 0.7, 2.5))
    phi = torch.from_numpy(phi64).float()
    w = [0.3, 1.7][:K]
    vref = boundary_values_ref(p.numpy(), phi.numpy(), classes)
    mean_abs = [np.abs(p.numpy().astype(np.float64)[..., c] * phi.numpy().astype(np.float64)[:, k]).mean() for k, c in enumerate(classes)]
    pd, phid, labd = p.to(DEV).requires_grad_(True), phi.to(DEV), torch.from_numpy(lab).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    cls, wv = (ctypes.c_int * K)(*classes), (ctypes.c_float * K)(*w)

    def fwd(base_total=None, scale_dev=None, term_scale_dev=None):
        n = _lib.load().ltu_loss_boundary_sums_floats(B, S, K)
        sums = torch.full(((n + 1) // 2,), float('nan'), device=DEV, dtype=torch.float64)      # no initialisation needed
        values = torch.empty(K + 1, device=DEV)
        _lib.call('ltu_loss_boundary_fwd', pd.data_ptr(), phid.data_ptr(), cls, wv, K, sums.data_ptr(), 2 * sums.numel(), values.data_ptr(),
                  _ptr(base_total), _ptr(scale_dev), _ptr(term_scale_dev), B, S, C, stream)
        return values.cpu().double().numpy()

    v = fwd()
    for k in range(K):
        print(f'C={C} class {classes[k]}: value {v[1 + k]:.8e} ref {vref[k]:.8e} |diff| {abs(v[1 + k] - vref[k]):.2e} bound {1e-5 * mean_abs[k]:.2e}')
        assert abs(v[1 + k] - vref[k]) <= 1e-5 * mean_abs[k]
    tot = float(np.dot(w, vref))
    tol = 1e-5 * float(np.dot(np.abs(w), mean_abs))
    assert abs(v[0] - tot) <= tol
    assert np.array_equal(fwd(), v)                                # bit-reproducible
    # the two run-time scales and the base total, each as defined
    t = lambda x: torch.tensor([x], device=DEV, dtype=torch.float32)
    assert abs(fwd(scale_dev=t(0.25))[0] - 0.25 * tot) <= tol
    assert abs(fwd(term_scale_dev=t(3.0))[0] - 3.0 * tot) <= 3 * tol
    assert abs(fwd(scale_dev=t(0.5), term_scale_dev=t(-2.0))[0] + tot) <= tol
    assert abs(fwd(base_total=t(7.5), term_scale_dev=t(0.5))[0] - (7.5 + 0.5 * tot)) <= tol + 7.5 * 2.0 ** -23
    assert fwd(base_total=t(7.5), term_scale_dev=t(0.0))[0] == 7.5
    assert np.array_equal(fwd(scale_dev=t(0.25))[1:], v[1:])       # the report stays unweighted
    # backward, alone: the term in its channels, exact zeros in the others
    gval = 0.75
    gref = boundary_grad_ref(tuple(p.shape), phi.numpy(), classes, w, g=gval)
    gs = t(gval)

    def bwd(dp, accumulate, scale_dev=None, term_scale_dev=None):
        _lib.call('ltu_loss_boundary_bwd', phid.data_ptr(), cls, wv, K, _ptr(scale_dev), _ptr(term_scale_dev), gs.data_ptr(), dp.data_ptr(),
                  accumulate, B, S, C, stream)
        return dp.cpu().double().numpy()

    dp = bwd(torch.full_like(pd, float('nan')), 0)
    others = [c for c in range(C) if c not in classes]
    assert not dp[..., others].any()
    assert (np.abs(dp - gref) <= 1e-6 * np.abs(gref)).all()        # every element
    dp = bwd(torch.empty_like(pd), 0, scale_dev=t(0.5), term_scale_dev=t(4.0))
    assert (np.abs(dp - 2.0 * gref) <= 1e-6 * np.abs(2.0 * gref)).all()
    # backward into a gradient that is already there
    g = torch.Generator().manual_seed(99)
    dp0 = torch.randn(p.shape, generator=g) * float(np.abs(gref).max())
    dp = bwd(dp0.to(DEV), 1)
    want = dp0.double().numpy() + gref
    assert np.abs(dp - want).max() <= 1e-6 * np.abs(want).max()
    assert np.array_equal(dp[..., others], dp0.double().numpy()[..., others])
    # through autograd: the single-term function with no base
    tot_t, base_values, values = ops.level_loss_boundary(pd, labd, phid, classes, w)
    (tot_t * gval).backward()
    assert base_values is None and abs(tot_t.item() - tot) <= tol and not values.requires_grad
    assert np.abs(pd.grad.cpu().double().numpy() - gref).max() <= 1e-6 * np.abs(gref).max()


# ---------------------------------------------------------------------------------------------- 3. LevelCriterion, three families
def _cl(p):
    return p.to(DEV).requires_grad_(True)


@pytest.mark.parametrize('C,spec,name', [(3, {'CrossEntroLoss': 1.0, 'DiceClassLoss': 1.0, 'BoundaryLoss': 0.01}, 'BoundaryLoss'),
                                        (5, {'CrossEntroLoss': 1.0, 'DiceClassLoss': 1.0, 'BoundaryLoss4': 0.01}, 'BoundaryLoss4'),
                                        (3, {'FocalLoss': 1.0, 'BoundaryLoss2': 0.01}, 'BoundaryLoss2')])
def test_level_criterion_adds_the_term(C, spec, name):
    from lintransunet_amd import losses as L
    B, sp, spacing = 2, (37, 20, 9), (0.7, 0.7, 2.5)
    cls = L.LevelCriterion.BOUNDARY[name]
    p = _probs(B, C, sp, 40 + C)
    lab = _blocky_labels(B, C, sp, 50 + C)
    target = torch.from_numpy(lab).unsqueeze(1).to(DEV)
    phi64 = phi_ref_batch(lab, (cls,), tuple(float(np.float32(s)) for s in spacing))
    vref = boundary_values_ref(p.numpy(), phi64, (cls,))[0]
    gref = boundary_grad_ref(tuple(p.shape), phi64, (cls,), (0.01,))
    plain = {k: v for k, v in spec.items() if k != name}
    pa = _cl(p)
    ta, named_a = L.LevelCriterion(plain)(pa.permute(0, 4, 1, 2, 3), target)       # today's kernels
    ta.backward()
    pb = _cl(p)
    tb, named_b = L.LevelCriterion(spec, spacing=spacing)(pb.permute(0, 4, 1, 2, 3), target)
    tb.backward()
    want = ta.item() + 0.01 * vref
    assert abs(tb.item() - want) <= 1e-5 * max(1.0, abs(want)), (tb.item(), want)
    assert rel_err(pb.grad, pa.grad.double().cpu() + torch.from_numpy(gref)) < 1e-4
    assert list(named_b) == list(spec) and abs(named_b[name].item() - 0.01 * vref) <= 1e-5 * max(1.0, abs(vref))
    assert all(torch.equal(named_b[k], named_a[k]) for k in plain)
    # maps handed in are the maps it would have built
    pc = _cl(p)
    tc, _ = L.LevelCriterion(spec)(pc.permute(0, 4, 1, 2, 3), target, phi=torch.from_numpy(phi64).float().to(DEV))
    assert abs(tc.item() - want) <= 1e-5 * max(1.0, abs(want))
    # the single-term module
    pm = _cl(p)
    v = L.BoundaryLoss(class_index=cls, spacing=spacing)(pm.permute(0, 4, 1, 2, 3), target)
    v.backward()
    assert abs(v.item() - vref) <= 1e-5 * max(1.0, abs(vref))
    assert rel_err(pm.grad, torch.from_numpy(gref) * 100.0) < 1e-5


def test_spec_without_boundary_names_is_the_old_path():
    from lintransunet_amd import losses as L, ops
    B, C, sp = 2, 3, (16, 12, 10)
    p = _probs(B, C, sp, 61)
    lab = torch.from_numpy(_blocky_labels(B, C, sp, 62)).to(DEV)
    pa = _cl(p)
    ta, _ = L.LevelCriterion({'CrossEntroLoss': 1.0, 'DiceClassLoss': 1.0}, scale=0.5, spacing=(3.0, 3.0, 3.0),
                             term_scale_dev=torch.tensor([5.0], device=DEV))(pa.permute(0, 4, 1, 2, 3), lab.unsqueeze(1))
    ta.backward()
    pb = _cl(p)
    tb, _ = ops.level_loss(pb, lab, 0.5, 0.0, [0.0, 0.5, 0.0, 0.0, 0.0])
    tb.backward()
    assert torch.equal(ta, tb) and torch.equal(pa.grad, pb.grad)


# ---------------------------------------------------------------------------------------------- 4. capture
def test_capture_replays_new_inputs_and_scale():
    from lintransunet_amd import losses as L, ops
    B, C, sp, spacing = 2, 3, (20, 12, 9), (0.5, 0.5, 2.0)
    spec = {'CrossEntroLoss': 1.0, 'DiceClassLoss': 1.0, 'BoundaryLoss': 0.01, 'BoundaryLoss2': 0.02}
    inputs = [(_probs(B, C, sp, 70 + i).to(DEV), torch.from_numpy(_blocky_labels(B, C, sp, 80 + i)).to(DEV)) for i in range(2)]
    term = torch.ones(1, device=DEV)
    crit = L.LevelCriterion(spec, spacing=spacing, term_scale_dev=term)

    def run(p, lab):
        phi = ops.signed_distance_maps(lab, crit.boundary_classes, spacing)
        total, named = crit(p.permute(0, 4, 1, 2, 3), lab.unsqueeze(1), phi=phi)
        total.backward()
        return total, named, phi

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
        total_s, named_s, phi_s = run(ps, labs)
    for (p, lab), a in ((inputs[1], 0.3), (inputs[0], 1.0), (inputs[1], 0.0)):
        with torch.no_grad():
            ps.copy_(p)
        labs.copy_(lab)
        term.fill_(a)
        graph.replay()
        torch.cuda.synchronize()
        pe = p.clone().requires_grad_(True)
        total_e, named_e, phi_e = run(pe, lab)
        torch.cuda.synchronize()
        assert torch.equal(phi_s, phi_e) and torch.equal(total_s, total_e) and torch.equal(ps.grad, pe.grad)
        assert all(torch.equal(named_s[k], named_e[k]) for k in spec)
    assert phi_s.abs().max().item() > 1.0


# ---------------------------------------------------------------------------------------------- 5. the training step
NAMES = ('CrossEntroLoss', 'DiceClassLoss', 'DiceClassLoss2', 'BoundaryLoss', 'BoundaryLoss2')
WEIGHTS = [10.0, 1.0, 1.0, 0.01, 0.01]
STEP_SPACING = (0.5, 0.5, 2.0)


def _build():
    from lintransunet_amd import train
    from lintransunet_amd.model import get_model_dict
    cfg = O_net.NetConfig(dim_output=3, **SMALL)
    m = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, cfg.dim_input, cfg.dim_output, dropout=0.0,
                                        act_dtype=torch.bfloat16)
    m.load_state_dict(seedgen.seeded_params(O_net.param_shapes(cfg), 900), strict=True)
    m = m.to(DEV).train()
    return m, train.GradReducer(m, bucket_mb=32.0, unused=train.UNUSED_PARAMETERS)


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def test_train_step_and_graphed_step(monkeypatch):
    from lintransunet_amd import train
    x = seedgen.seeded_volume((1, 1, 32, 32, 32), 901).to(DEV)
    label = seedgen.seeded_label((1, 1, 32, 32, 32), 902, n_classes=3).to(DEV)
    w = O_step.dynamic_weights(0)
    specs = train.level_specs(5, NAMES, criterion_weight=WEIGHTS)
    plain = train.level_specs(5, NAMES[:3], criterion_weight=WEIGHTS[:3])
    m, red = _build()
    # the eager step reads the level weights from the device, as the captured step does
    level_scale = torch.tensor(w, device=DEV, dtype=torch.float32)
    one = torch.ones(1, device=DEV)

    def eager(sp, **kw):
        for _ in range(2):
            red.zero_grad()
            totals, named = train.train_step(m, x, label, w, specs=sp, reducer=red, level_scale=level_scale, spacing=STEP_SPACING, **kw)
        torch.cuda.synchronize()
        return [t.item() for t in totals], named, _grads(m)

    tot_e, named, g_eager = eager(specs, boundary_scale=one)
    assert g_eager and all(torch.isfinite(g).all() for g in g_eager.values())
    assert list(named[0]) == list(NAMES)
    # every level total against float64, on the model's own predictions and the pyramid's labels
    with torch.no_grad():
        predict, masks = m(x)
    pyr = train.label_pyramid(label, 5)
    for lvl in range(5):
        pred = (predict if lvl == 0 else masks[-lvl]).double().cpu()
        lab = pyr[lvl].cpu()
        sp = tuple(s * 32.0 / n for s, n in zip(STEP_SPACING, lab.shape[1:]))
        t = onehot(lab.unsqueeze(1), 3).double()
        base = 10.0 * O_loss._multi_ce(pred, t) + O_loss.dice_class_onehot(pred, t, 1) + O_loss.dice_class_onehot(pred, t, 2)
        phi = phi_ref_batch(lab.numpy(), (1, 2), sp)
        v = boundary_values_ref(pred.permute(0, 2, 3, 4, 1).numpy(), phi, (1, 2))
        want = w[lvl] * (float(base) + 0.01 * (v[0] + v[1]))
        print(f'level {lvl} {tuple(lab.shape[1:])} spacing {sp}: total {tot_e[lvl]:.6f} float64 {want:.6f} boundary values {v}')
        assert abs(tot_e[lvl] - want) <= 1e-4 * abs(want), (lvl, tot_e[lvl], want)
        assert abs(named[lvl]['BoundaryLoss2'].item() - 0.01 * v[1]) <= 1e-4 * max(abs(v[1]), 1e-3)
    # the captured step without the weight-gradient queue: the same kernels on one stream, bit for bit
    monkeypatch.setenv('LTU_WQ', '0')
    step = train.GraphedStep(m, x, label, w, red, specs=specs, spacing=STEP_SPACING)
    assert step.wq_stream is None and step.boundary_scale is not None
    tot_g, _ = step(x, label)
    torch.cuda.synchronize()
    assert [t.item() for t in tot_g] == tot_e
    g_graph = _grads(m)
    differ = [k for k in g_eager if not torch.equal(g_graph[k], g_eager[k])]
    assert not differ, differ
    # alpha = 0: the gradients of the spec without the boundary names
    step.set_boundary_scale(0.0)
    tot_0, _ = step(x, label)
    torch.cuda.synchronize()
    g_zero = _grads(m)
    tot_p, _, g_plain = eager(plain)
    assert [t.item() for t in tot_0] == tot_p
    differ = [k for k in g_plain if not torch.equal(g_zero[k], g_plain[k])]
    assert not differ, differ
    assert any(not torch.equal(g_zero[k], g_graph[k]) for k in g_plain)      # and the term did pull on the weights before
