"""Top-k cross-entropy on the GPU: the kernels of csrc/loss_topk.hip against the float64 restatement of tests/topk_common.py
(random inputs, exact ties, the clamp, labels without a channel, the device-resident fraction, the argument contract),
losses.LevelCriterion with the name on every loss family, the whole thing under graph capture, and a training step (eager and
captured) with the term at all five levels."""
import functools

import numpy as np
import pytest
import torch

from oracle import net as O_net          # noqa: E402
from oracle import seedgen               # noqa: E402
from oracle import step as O_step        # noqa: E402
from tests.topk_common import count_ref, make_labels, make_probs, set_label_prob, tied_probs, topk_ref, voxel_losses_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda'
E_SHAPE, E_ARG = -2, -4
SMALL = dict(num_layers=[8, 8, 8, 16, 32], roi_size_list=[20, 12, 9, 10, 6])      # of tests/test_gpu_boundary.py
# less than one workgroup, S odd (scalar kernels); N % 4 == 0 (four-voxel kernels); 8 classes; several workgroups per sample,
# S not a multiple of 256
CASES = [(2, (7, 5, 3), 2), (3, (37, 20, 9), 3), (1, (130, 5, 3), 8), (2, (64, 64, 33), 3)]
FRACS = ['1/N', 0.1, 0.5, 1.0]


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _t(x):
    return torch.tensor([x], device=DEV, dtype=torch.float32)


class Kernels:
    """ltu_loss_topk_fwd / _bwd on one (p, label) through the raw C-ABI; the scratch is filled with garbage first"""

    def __init__(self, p, lab):
        from lintransunet_amd import _lib
        self.lib = _lib
        self.p = torch.from_numpy(np.array(p)).to(DEV)
        self.lab = torch.from_numpy(np.array(lab)).to(DEV)
        self.B, self.C = p.shape[0], p.shape[-1]
        self.S = int(np.prod(p.shape[1:-1]))
        self.need = _lib.load().ltu_loss_topk_scratch_elems(self.B, self.S)
        assert self.need >= self.B * self.S
        self.scratch = torch.full((self.need,), 0x7fc12345, device=DEV, dtype=torch.int32)      # no initialisation needed
        self.stream = torch.cuda.current_stream().cuda_stream

    def fwd(self, frac=0.1, frac_dev=None, w=1.0, base_total=None, scale_dev=None):
        values = torch.full((3,), float('nan'), device=DEV)
        self.lib.call('ltu_loss_topk_fwd', self.p.data_ptr(), self.lab.data_ptr(), self.scratch.data_ptr(), self.need, values.data_ptr(),
                      _ptr(base_total), w, frac, _ptr(frac_dev), _ptr(scale_dev), self.B, self.S, self.C, self.stream)
        return values.cpu().numpy()

    def bwd(self, dp=None, accumulate=0, w=1.0, g=1.0, scale_dev=None):
        dp = torch.full_like(self.p, float('nan')) if dp is None else dp
        self.lib.call('ltu_loss_topk_bwd', self.p.data_ptr(), self.lab.data_ptr(), self.scratch.data_ptr(), self.need, w, _ptr(scale_dev),
                      _t(g).data_ptr(), dp.data_ptr(), accumulate, self.B, self.S, self.C, self.stream)
        return dp.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(B, spatial, C):
    p, lab = make_probs(B, spatial, C, 11 * B + C), make_labels(B, spatial, C, 13 * B + C)
    p.setflags(write=False)
    lab.setflags(write=False)
    return p, lab


@functools.lru_cache(maxsize=None)
def _ref(B, spatial, C, k):
    p, lab = _case(B, spatial, C)
    r = topk_ref(p, lab, k)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


# ---------------------------------------------------------------------------------------------- 1. kernels against float64
@pytest.mark.parametrize('frac', FRACS)
@pytest.mark.parametrize('B,spatial,C', CASES)
def test_kernels_against_float64(B, spatial, C, frac):
    from lintransunet_amd import ops
    p, lab = _case(B, spatial, C)
    N = B * int(np.prod(spatial))
    frac = 1.0 / N if frac == '1/N' else frac
    k = ops.topk_count(frac, N)
    assert k == count_ref(frac, N) and (frac != FRACS[1] or N != 270336 or k == 27033)
    r = _ref(B, spatial, C, k)
    kern = Kernels(p, lab)
    v = kern.fwd(frac)
    dp = kern.bwd()
    ev, et = abs(v[1] - r['value']) / r['value'], abs(v[2] - r['tau']) / r['tau']
    print(f'B={B} {spatial} C={C} frac={frac:.3g} k={k}: value {v[1]:.8e} ref {r["value"]:.8e} rel {ev:.2e}; tau {v[2]:.8e} ref '
          f'{r["tau"]:.8e} rel {et:.2e}')
    assert ev <= 1e-5 and et <= 1e-5 and v[0] == v[1]
    # the gradient, on every voxel but those a last-bit difference of logf may move across the threshold
    near = np.abs(r['l'] - r['tau']) <= 1e-5 * r['tau']
    assert near.sum() <= 8, near.sum()
    keep = ~near.reshape(p.shape[:-1])
    gmax = np.abs(r['grad']).max()
    eg = np.abs(dp.astype(np.float64) - r['grad'])[keep].max() / gmax
    print(f'   gradient: max |diff| / max {eg:.2e}, {near.sum()} voxels at the threshold left out, {int((dp != 0).sum())} non-zero')
    assert np.isfinite(dp).all() and eg <= 1e-5
    if k == 1:
        assert v[1] == v[2]                                        # one voxel: the maximum
    # a second call: bit for bit
    assert np.array_equal(kern.fwd(frac), v) and np.array_equal(kern.bwd(), dp)
    # weight, run-time scale, base total and the incoming gradient, each as defined; the report stays unweighted
    v2 = kern.fwd(frac, w=0.5, base_total=_t(7.5), scale_dev=_t(3.0))
    assert np.array_equal(v2[1:], v[1:]) and abs(v2[0] - (7.5 + 1.5 * r['value'])) <= 1e-5 * (7.5 + 1.5 * r['value'])
    dp0 = torch.from_numpy(np.random.default_rng(5).standard_normal(p.shape).astype(np.float32) * np.float32(gmax)).to(DEV)
    dp2 = kern.bwd(dp0.clone(), accumulate=1, w=0.5, g=-2.0, scale_dev=_t(3.0))
    want = dp0.cpu().numpy().astype(np.float64) - 3.0 * r['grad']
    assert (np.abs(dp2 - want)[keep]).max() <= 1e-5 * np.abs(want).max()
    untouched = r['grad'] == 0
    untouched[~keep] = False
    assert np.array_equal(dp2[untouched], dp0.cpu().numpy()[untouched])


# ---------------------------------------------------------------------------------------------- 2. exact ties
def test_exact_ties():
    from lintransunet_amd import ops
    B, spatial, C = 2, (9, 6, 11), 3
    p, lab, grp = tied_probs(B, spatial, C, 5)
    N = grp.size
    n3, n2 = int((grp == 3).sum()), int((grp == 2).sum())
    k = n3 + n2 // 2                                               # strictly inside the p = 1/4 group
    frac = (k + 0.5) / N
    assert ops.topk_count(frac, N) == k and 0 < n2 // 2 < n2
    kern = Kernels(p, lab)
    v = kern.fwd(frac)
    tau = np.float32(-np.log(0.25))
    assert v[2] == tau, (v[2], tau)
    r = topk_ref(p, lab, k)
    assert abs(v[1] - r['value']) <= 1e-6 * r['value']
    dp = kern.bwd()
    g = dp.sum(-1)                                                 # one channel per voxel is non-zero
    assert (np.count_nonzero(dp, axis=-1) <= 1).all()
    assert (g[grp == 3] == -8.0 * np.float32(1.0 / k)).all()                              # weight 1 / k, dl/dp = -8
    assert (g[grp == 2] == -4.0 * np.float32((k - n3) / (n2 * k))).all()                  # the tie: exactly (k - n_gt) / (n_eq k)
    assert not g[grp < 2].any()
    # the whole batch: p == 1.0 gives l = -0.0, which must sort last, not first
    v = kern.fwd(1.0)
    l, _, _ = voxel_losses_ref(p, lab)
    assert v[2] == 0.0 and abs(v[1] - l.mean()) <= 1e-6 * l.mean(), v
    dp = kern.bwd().sum(-1)
    assert (dp[grp == 0] == -np.float32(1.0 / N)).all() and (dp[grp == 3] == -8.0 * np.float32(1.0 / N)).all()


# ---------------------------------------------------------------------------------------------- 3. clamp
def test_clamp():
    B, spatial, C = 2, (20, 12, 9), 3
    p, lab = make_probs(B, spatial, C, 31), make_labels(B, spatial, C, 32)
    low = np.random.default_rng(33).random(lab.shape) < 0.3
    p = np.where(low[..., None], set_label_prob(p, lab, np.full(lab.shape, 1e-7, np.float32)), p)
    kern = Kernels(p, lab)
    v = kern.fwd(0.1)
    want = np.float32(-np.log(np.float64(np.float32(1e-6))))
    print(f'clamp: value {v[1]!r} tau {v[2]!r} fp32(-log 1e-6) {want!r}')
    # logf is within 2 ulp: the clamped loss is one fp32 number, and value and tau are that number
    assert v[1] == v[2] and abs(np.float64(v[2]) - np.float64(want)) <= 2 * np.spacing(want)
    dp = kern.bwd()
    assert np.isfinite(dp).all() and not dp.any()
    r = topk_ref(p, lab, count_ref(0.1, lab.size))
    assert r['n_gt'] == 0 and r['n_eq'] == low.sum() and not r['grad'].any()


# ---------------------------------------------------------------------------------------------- 4. labels >= C
@pytest.mark.parametrize('frac', [0.1, 1.0])
def test_labels_without_a_channel(frac):
    B, spatial, C = 2, (20, 12, 9), 3
    p, lab = make_probs(B, spatial, C, 41), make_labels(B, spatial, C, 42)
    lab = lab.copy()
    odd = np.random.default_rng(43).choice(lab.size, 9, replace=False)
    lab.reshape(-1)[odd] = 200
    N = lab.size
    r = topk_ref(p, lab, count_ref(frac, N))
    kern = Kernels(p, lab)
    v = kern.fwd(frac)
    assert abs(v[1] - r['value']) <= 1e-5 * r['value'] and abs(v[2] - r['tau']) <= 1e-5 * r['tau']
    if frac == 1.0:
        assert v[2] == 0.0 and r['n_eq'] == 9                      # they are the minimum, and they count in N
    dp = kern.bwd()
    assert not dp.reshape(N, C)[odd].any()
    near = (np.abs(r['l'] - r['tau']) <= 1e-5 * r['tau']).reshape(lab.shape)
    assert near.sum() <= 8 + 9
    assert np.abs(dp - r['grad'])[~near].max() <= 1e-5 * np.abs(r['grad']).max()


# ---------------------------------------------------------------------------------------------- 5. device fraction
def test_device_fraction():
    B, spatial, C = 3, (37, 20, 9), 3
    p, lab = _case(B, spatial, C)
    N = lab.size
    kern = Kernels(p, lab)
    fd = _t(0.5)
    for f in (0.5, 0.1):
        fd.fill_(f)
        v_dev, dp_dev = kern.fwd(0.77, frac_dev=fd), kern.bwd()    # the host argument is ignored beside a device one
        v_host, dp_host = kern.fwd(f), kern.bwd()
        assert np.array_equal(v_dev, v_host) and np.array_equal(dp_dev, dp_host)
    assert v_host[1] > kern.fwd(0.5)[1]                            # fewer, harder voxels: a larger mean
    lo, hi = kern.fwd(1.0 / N * 1.000001), kern.fwd(1.0)
    for bad, want in ((0.0, lo), (-1.0, lo), (2.0, hi), (float('nan'), hi), (float('inf'), hi)):
        fd.fill_(bad)
        assert np.array_equal(kern.fwd(0.5, frac_dev=fd), want), bad


# ---------------------------------------------------------------------------------------------- 6. argument errors
def test_argument_errors():
    from lintransunet_amd import _lib
    lib = _lib.load()
    B, S = 2, 105
    need = lib.ltu_loss_topk_scratch_elems(B, S)
    p, lab = torch.zeros(B * S * 9, device=DEV), torch.zeros(B * S, device=DEV, dtype=torch.uint8)
    scratch, values, one = torch.zeros(need, device=DEV, dtype=torch.int32), torch.zeros(3, device=DEV), torch.ones(1, device=DEV)
    dp = torch.zeros_like(p)
    st = torch.cuda.current_stream().cuda_stream

    def fwd(C=3, n=need, frac=0.1, w=1.0, frac_dev=0, pp=p.data_ptr(), Bv=B, Sv=S):
        return lib.ltu_loss_topk_fwd(pp, lab.data_ptr(), scratch.data_ptr(), n, values.data_ptr(), 0, w, frac, frac_dev, 0, Bv, Sv, C, st)

    def bwd(C=3, n=need, w=1.0, g=one.data_ptr()):
        return lib.ltu_loss_topk_bwd(p.data_ptr(), lab.data_ptr(), scratch.data_ptr(), n, w, 0, g, dp.data_ptr(), 0, B, S, C, st)

    assert fwd() == 0 and bwd() == 0
    assert fwd(C=1) == E_SHAPE and fwd(C=9) == E_SHAPE and bwd(C=1) == E_SHAPE and bwd(C=9) == E_SHAPE
    assert fwd(Bv=0) == E_SHAPE and fwd(Sv=0) == E_SHAPE and fwd(Bv=2, Sv=2 ** 30) == E_SHAPE
    assert fwd(n=need - 1) == E_ARG and bwd(n=need - 1) == E_ARG
    assert fwd(frac=0.0) == E_ARG and fwd(frac=1.5) == E_ARG and fwd(frac=float('nan')) == E_ARG
    assert fwd(frac=0.0, frac_dev=one.data_ptr()) == 0             # a device fraction replaces the host one
    assert fwd(w=float('inf')) == E_ARG and fwd(w=float('nan')) == E_ARG and bwd(w=float('inf')) == E_ARG
    assert fwd(pp=0) == E_ARG and bwd(g=0) == E_ARG
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 7. LevelCriterion
W_TOPK = 0.7
SPECS = {'orig': (3, {'CrossEntroLoss': 10, 'DiceClassLoss': 1}), 'wide': (5, {'CrossEntroLoss': 10, 'DiceClassLoss': 1}),
         'ext': (3, {'FocalLoss': 1.0}), 'boundary': (3, {'BoundaryLoss': 0.05}), 'alone': (3, {})}


def _predict(C, seed):
    """[2, C, 12, 10, 8] probabilities and u8 labels [2, 1, 12, 10, 8]"""
    p = torch.from_numpy(make_probs(2, (12, 10, 8), C, seed)).permute(0, 4, 1, 2, 3).contiguous()
    lab = torch.from_numpy(make_labels(2, (12, 10, 8), C, seed + 1)).unsqueeze(1)
    return p.to(DEV), lab.to(DEV)


@pytest.mark.parametrize('family', list(SPECS))
def test_level_criterion_adds_the_term(family):
    from lintransunet_amd import losses as L
    C, plain = SPECS[family]
    spec = dict(plain, TopKCELoss=W_TOPK)
    p, lab = _predict(C, 50 + C)
    frac = 0.2
    pa = p.clone().requires_grad_(True)
    if plain:
        ta, named_a = L.LevelCriterion(plain)(pa, lab)
        ta.backward()
        ga, ta = pa.grad, ta.item()
    else:
        ga, ta, named_a = torch.zeros_like(p), 0.0, {}
    pt = p.clone().requires_grad_(True)
    tt, named_t = L.LevelCriterion({'TopKCELoss': W_TOPK}, topk_fraction=frac)(pt, lab)
    tt.backward()
    pb = p.clone().requires_grad_(True)
    tb, named_b = L.LevelCriterion(spec, topk_fraction=frac)(pb, lab)
    tb.backward()
    torch.cuda.synchronize()
    # the term itself against float64
    r = topk_ref(p.permute(0, 2, 3, 4, 1).cpu().numpy(), lab[:, 0].cpu().numpy(), count_ref(frac, lab.numel()))
    assert abs(named_t['TopKCELoss'].item() - W_TOPK * r['value']) <= 1e-5 * W_TOPK * r['value']
    assert abs(tt.item() - W_TOPK * r['value']) <= 1e-5 * W_TOPK * r['value']
    # total and gradient: the two separate ones, joined by one fp32 add
    want = ta + named_b['TopKCELoss'].item()                     # the report is w * value
    print(f'{family}: total {tb.item():.8f} separate {ta:.8f} + {tt.item():.8f}')
    assert abs(tb.item() - want) <= 1e-6 * abs(want) and abs(tb.item() - (ta + tt.item())) <= 1e-6 * abs(want)
    gsum = ga.double() + pt.grad.double()
    assert (pb.grad.double() - gsum).abs().max().item() <= 1e-6 * gsum.abs().max().item()
    assert list(named_b) == list(spec)
    assert torch.equal(named_b['TopKCELoss'], named_t['TopKCELoss']) and all(torch.equal(named_b[n], named_a[n]) for n in plain)


def test_single_term_module_and_ops():
    from lintransunet_amd import losses as L, ops
    p, lab = _predict(3, 60)
    r = topk_ref(p.permute(0, 2, 3, 4, 1).cpu().numpy(), lab[:, 0].cpu().numpy(), count_ref(0.1, lab.numel()))
    pm = p.clone().requires_grad_(True)
    v = L.get_criterions(['TopKCELoss'])['TopKCELoss'](pm, lab)
    v.backward()
    assert abs(v.item() - r['value']) <= 1e-5 * r['value']
    pc = p.permute(0, 2, 3, 4, 1).contiguous().requires_grad_(True)
    total, base_values, values = ops.level_loss_topk(pc, lab[:, 0].contiguous(), 1.0)
    total.backward()
    assert base_values is None and not values.requires_grad and values.shape == (2,)
    assert total.item() == v.item() == values[0].item() and abs(values[1].item() - r['tau']) <= 1e-5 * r['tau']
    assert torch.equal(pc.grad.permute(0, 4, 1, 2, 3), pm.grad)
    with pytest.raises(ValueError):
        ops.level_loss_topk(pc, lab[:, 0].contiguous(), 1.0, frac=0.0)


def test_spec_without_the_name_is_the_old_path():
    from lintransunet_amd import losses as L, ops
    p, lab = _predict(3, 62)
    pa = p.clone().requires_grad_(True)
    ta, _ = L.LevelCriterion({'CrossEntroLoss': 1.0, 'DiceClassLoss': 1.0}, scale=0.5, topk_fraction=0.3,
                             topk_fraction_dev=_t(0.4))(pa, lab)
    ta.backward()
    pb = p.permute(0, 2, 3, 4, 1).contiguous().requires_grad_(True)
    tb, _ = ops.level_loss(pb, lab[:, 0].contiguous(), 0.5, 0.0, [0.0, 0.5, 0.0, 0.0, 0.0])
    tb.backward()
    assert torch.equal(ta, tb) and torch.equal(pa.grad, pb.grad.permute(0, 4, 1, 2, 3))


# ---------------------------------------------------------------------------------------------- 8. capture
def test_capture_replays_new_inputs_and_fraction():
    from lintransunet_amd import losses as L
    spec = {'CrossEntroLoss': 1.0, 'DiceClassLoss': 1.0, 'BoundaryLoss': 0.05, 'TopKCELoss': 1.0}
    inputs = [_predict(3, 70 + 2 * i) for i in range(2)]
    fd = _t(0.5)
    crit = L.LevelCriterion(spec, topk_fraction_dev=fd)

    def run(p, lab):
        total, named = crit(p, lab)
        total.backward()
        return total, named

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
        total_s, named_s = run(ps, labs)
    seen = []
    for (p, lab), f in ((inputs[1], 0.5), (inputs[1], 0.1), (inputs[0], 0.1)):
        with torch.no_grad():
            ps.copy_(p)
        labs.copy_(lab)
        fd.fill_(f)
        graph.replay()
        torch.cuda.synchronize()
        pe = p.clone().requires_grad_(True)
        total_e, named_e = run(pe, lab)
        torch.cuda.synchronize()
        assert torch.equal(total_s, total_e) and torch.equal(ps.grad, pe.grad)
        assert all(torch.equal(named_s[k], named_e[k]) for k in spec)
        seen.append(named_s['TopKCELoss'].item())
    assert seen[1] > seen[0]                                       # the fraction did change what the replay computes


# ---------------------------------------------------------------------------------------------- 9. the training step
NAMES = ('CrossEntroLoss', 'DiceClassLoss', 'DiceClassLoss2', 'TopKCELoss')
WEIGHTS = [10.0, 1.0, 1.0, 1.0]


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
    x = seedgen.seeded_volume((2, 1, 32, 32, 32), 901).to(DEV)
    label = seedgen.seeded_label((2, 1, 32, 32, 32), 902, n_classes=3).to(DEV)
    w = O_step.dynamic_weights(0)
    specs = train.level_specs(5, NAMES, criterion_weight=WEIGHTS)
    plain = train.level_specs(5, NAMES[:3], criterion_weight=WEIGHTS[:3])
    m, red = _build()
    level_scale = torch.tensor(w, device=DEV, dtype=torch.float32)

    def eager(sp, **kw):
        for _ in range(2):
            red.zero_grad()
            totals, named = train.train_step(m, x, label, w, specs=sp, reducer=red, level_scale=level_scale, **kw)
        torch.cuda.synchronize()
        return [t.item() for t in totals], named, _grads(m)

    tot_e, named, g_eager = eager(specs, topk_fraction=0.1)
    tot_p, _, _ = eager(plain)
    assert g_eager and all(torch.isfinite(g).all() for g in g_eager.values()) and all(np.isfinite(tot_e))
    assert list(named[0]) == list(NAMES)
    assert all(a > b for a, b in zip(tot_e, tot_p)) and sum(tot_e) > sum(tot_p)
    # the captured step without the weight-gradient queue: the same kernels on one stream, bit for bit
    monkeypatch.setenv('LTU_WQ', '0')
    step = train.GraphedStep(m, x, label, w, red, specs=specs, topk_fraction=0.1)
    assert step.wq_stream is None and step.topk_fraction is not None
    tot_g, _ = step(x, label)
    torch.cuda.synchronize()
    assert [t.item() for t in tot_g] == tot_e
    g_graph = _grads(m)
    differ = [k for k in g_eager if not torch.equal(g_graph[k], g_eager[k])]
    assert not differ, differ
    # the whole batch: the plain mean cross-entropy of each level's prediction
    step.set_topk_fraction(1.0)
    _, named_1 = step(x, label)
    torch.cuda.synchronize()
    with torch.no_grad():
        predict, masks = m(x)
    pyr = train.label_pyramid(label, 5)
    for lvl in range(5):
        pred = (predict if lvl == 0 else masks[-lvl]).float().permute(0, 2, 3, 4, 1).cpu().numpy()
        l, _, _ = voxel_losses_ref(pred, pyr[lvl].cpu().numpy())
        got = named_1[lvl]['TopKCELoss'].item()
        print(f'level {lvl}: TopKCELoss at fraction 1 {got:.6f}, mean cross-entropy {l.mean():.6f}, at 0.1 {named[lvl]["TopKCELoss"].item():.6f}')
        assert abs(got - l.mean()) <= 1e-4 * l.mean()
        assert named[lvl]['TopKCELoss'].item() > got
    with pytest.raises(ValueError):
        step.set_topk_fraction(0.0)
    with pytest.raises(ValueError):
        train.GraphedStep(m, x, label, w, red, specs=plain).set_topk_fraction(0.5)
