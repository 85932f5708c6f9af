"""The guarded AdamW step on the GPU (csrc/optim.hip behind optim.FusedAdamW's max_grad_norm / skip_nonfinite / ema_decay).  The
oracle is torch on the CPU: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, a step not taken for a skipped one, and an EMA
computed from the reference's weights after each step.  Gates: parameters and EMA rtol 2e-5 / atol 2e-7 (the gate of
test_optim.py::test_fused_adamw_matches_torch: same arithmetic, as many steps of drift); the norm 1e-5 relative (fewer than 100
fp32 additions per chain ahead of the fp64 fold: 100 * 2^-24 = 6e-6 on the sum, 3e-6 on its root)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL, NORM_RTOL = 2e-5, 2e-7, 1e-5


def _small_pair():
    """the two-layer model of test_fused_adamw_matches_torch: the CPU reference first, the GPU model a copy of it"""
    ref = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5))
    model = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5))
    model.load_state_dict(ref.state_dict())
    return model.cuda(), ref


def _backward(model, ref, x):
    model(x.cuda()).square().mean().backward()
    ref(x).square().mean().backward()


def _assert_params_close(model, ref, what):
    for (k, a), (_, b) in zip(model.state_dict().items(), ref.state_dict().items()):
        assert torch.allclose(a.cpu().to(b.dtype), b, rtol=RTOL, atol=ATOL), (what, k, (a.cpu() - b).abs().max().item())


def _ema_by_name(opt, model):
    sd = opt.ema_state_dict(model)
    return {k: sd[k].cpu() for k, _ in model.named_parameters()}


def _snapshot(opt):
    return [t.clone() for group in (opt.flat_p, opt.m, opt.v, opt.ema) for t in group]


def _same(a, b):
    # bit-exact, NaN-free buffers
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# bucket_mb 0.001 is the setting of test_fused_adamw_matches_torch: ONE bucket of 822 elements for this model (a bucket closes when
# it reaches the cap of 262 floats, and the 703-element weight comes last); 4e-6 caps a bucket at one float, so every parameter is
# a bucket of its own: 5, 95, 19 and 703 elements, all odd, all with a tail
BUCKET_MB = [0.001, 4e-6]


@pytest.mark.parametrize('bucket_mb', BUCKET_MB)
def test_clipping_matches_torch(bucket_mb):
    from lintransunet_amd import train, optim
    torch.manual_seed(0)
    model, ref = _small_pair()
    reducer = train.GradReducer(model, bucket_mb=bucket_mb)
    assert [f.numel() for f in reducer.flat] == ([822] if bucket_mb == 0.001 else [5, 95, 19, 703])
    opt = optim.FusedAdamW(reducer, lr=1e-2, max_grad_norm=0.25)
    topt = torch.optim.AdamW(ref.parameters(), lr=1e-2)
    norms = []
    for it in range(9):
        x = torch.randn(11, 37)
        opt.zero_grad(); topt.zero_grad()
        _backward(model, ref, x)
        norm = torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.25).item()
        opt.step(); topt.step()
        norms.append(norm)
        got = opt.grad_norm.item()
        print(f'step {it}: cpu norm {norm:.6f} gpu norm {got:.6f} rel {abs(got - norm) / norm:.2e}')
        assert abs(got - norm) <= NORM_RTOL * norm, (it, got, norm)
        _assert_params_close(model, ref, it)
    # judged by the reference's own norms the threshold is crossed both ways: clipping is neither idle nor always on
    assert sum(n > 0.25 for n in norms) >= 2 and sum(n < 0.25 for n in norms) >= 2, norms
    assert opt.counters() == (9, 0)


class _TwoLinears(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.big = torch.nn.Linear(2048, 2100)
        self.tiny = torch.nn.Linear(3, 1)


def test_bucket_larger_than_one_grid_sweep_with_ema():
    """buckets of 1, 3, 2 100 and 4 300 800 elements: the last is more than the 4096 x 256 x 4 elements one sweep of the capped grid
    covers, the first two are less than one workgroup (and the tail path only).  Step 0 is clipped (norm about 2.07), step 1 is not
    (about 0.41).
    The reference is the same pair of torch calls on the CPU, clip_grad_norm_ + AdamW.step, on a FLOAT64 copy of the model: over
    4.3 M elements torch's fp32 norm is itself off by 9.3e-5 and 1.05e-4 (steps 0 and 1, against float64 of the same gradients;
    the kernel's norm is within 5e-8 of float64), ten times the 1e-5 gate, and its clipping coefficient carries that error into
    the moments.  Gates as everywhere in this file.
    Both sides are fed the SAME gradient bits (drawn in fp32 on the CPU, copied into the buckets): among 4.3 M elements some
    gradients are within a few eps of zero, where lr * m / (sqrt(v) + eps) turns the last bits of a gradient computed by two
    different matrix products into differences far above the gate; with equal inputs the gate measures the update's arithmetic."""
    from lintransunet_amd import train, optim, _lib
    from lintransunet_amd.ops import _p, _s
    torch.manual_seed(3)
    ref = _TwoLinears()
    model = _TwoLinears()
    model.load_state_dict(ref.state_dict())
    model, ref = model.cuda(), ref.double()
    reducer = train.GradReducer(model, bucket_mb=4e-6)          # a cap of one float: every parameter is its own bucket
    assert sorted(f.numel() for f in reducer.flat) == [1, 3, 2100, 2048 * 2100]
    assert 2048 * 2100 // 4 > 4096 * 256
    opt = optim.FusedAdamW(reducer, lr=1e-2, max_grad_norm=1.0, ema_decay=0.9)
    topt = torch.optim.AdamW(ref.parameters(), lr=1e-2)
    ema = {k: v.detach().clone() for k, v in ref.named_parameters()}
    gpu_params = dict(model.named_parameters())
    for it, scale in enumerate((1e-3, 2e-4)):
        for k, p in ref.named_parameters():
            g = scale * torch.randn(p.shape)
            p.grad = g.double()
            gpu_params[k].grad.copy_(g)
        norm = torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0).item()
        assert (norm > 1.0) == (it == 0)
        opt.step(); topt.step()
        got = opt.grad_norm.item()
        print(f'step {it}: cpu norm {norm:.8f} gpu norm {got:.8f} rel {abs(got - norm) / norm:.2e}')
        assert abs(got - norm) <= NORM_RTOL * norm, (it, got, norm)
        _assert_params_close(model, ref, it)
        mine = _ema_by_name(opt, model)
        for k, p in ref.named_parameters():
            ema[k] = 0.9 * ema[k] + 0.1 * p.detach()
            assert torch.allclose(mine[k].double(), ema[k], rtol=RTOL, atol=ATOL), (it, k, (mine[k] - ema[k]).abs().max().item())
    # two identical calls of the sum of squares + fold on the big bucket: the same bits
    g = max(reducer.flat, key=lambda f: f.numel())
    parts = _lib.load().ltu_grad_sumsq_parts(g.numel())
    assert parts == 4096
    bits = []
    for _ in range(2):
        scratch = torch.zeros(parts, device='cuda')
        state = torch.zeros(12, device='cuda')
        _lib.call('ltu_grad_sumsq', _p(g), g.numel(), 1.0, _p(scratch), scratch.numel(), _s())
        _lib.call('ltu_adamw_guard', _p(scratch), parts, _p(state), 1.0, 0.0, 1, 0.9, 0.999, _s())
        bits.append(state.view(torch.int32).tolist())
    assert bits[0] == bits[1], bits
    want = g.double().square().sum().sqrt().item()
    assert abs(torch.tensor(bits[0][0], dtype=torch.int32).view(torch.float32).item() - want) <= NORM_RTOL * want


@pytest.mark.parametrize('bucket_mb', BUCKET_MB)
def test_nonfinite_steps_are_skipped(bucket_mb):
    from lintransunet_amd import train, optim
    torch.manual_seed(0)
    model, ref = _small_pair()
    reducer = train.GradReducer(model, bucket_mb=bucket_mb)
    opt = optim.FusedAdamW(reducer, lr=1e-2, skip_nonfinite=True, ema_decay=0.9)
    topt = torch.optim.AdamW(ref.parameters(), lr=1e-2)

    def good_step(it):
        x = torch.randn(11, 37)
        opt.zero_grad(); topt.zero_grad()
        _backward(model, ref, x)
        opt.step(); topt.step()
        _assert_params_close(model, ref, it)

    for it in range(3):
        good_step(it)
    flat = reducer.flat
    assert flat[-1].numel() & 3                              # the last element of the last bucket is on the tail path
    mid = flat[len(flat) // 2]
    poisons = [(flat[0], 0, float('nan')), (flat[-1], flat[-1].numel() - 1, float('inf')), (mid, mid.numel() // 2, float('-inf'))]
    for k, (bucket, idx, value) in enumerate(poisons):
        opt.zero_grad(); topt.zero_grad()
        _backward(model, ref, torch.randn(11, 37))
        bucket[idx] = value
        before = _snapshot(opt)
        opt.step()                                           # the reference skips by not stepping
        assert _same(_snapshot(opt), before), k
        assert opt.counters() == (3, k + 1)
        assert not torch.isfinite(opt.grad_norm).item()
    for it in range(3, 5):                                   # bias correction with t = 4, 5 (not 7, 8), or the gate fails
        good_step(it)
    sd = opt.state_dict()
    assert sd['step'] == 5 and sd['skipped'] == 3 and len(sd['ema']) == len(flat)
    # a fresh optimizer on a copy of the model, restored from the state dict, takes the next step bit-identically
    model2 = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5)).cuda()
    model2.load_state_dict(model.state_dict())
    reducer2 = train.GradReducer(model2, bucket_mb=bucket_mb)
    opt2 = optim.FusedAdamW(reducer2, lr=1e-2, skip_nonfinite=True, ema_decay=0.9)
    opt2.load_state_dict(sd)
    assert opt2.counters() == (5, 3)
    opt.zero_grad()
    model(torch.randn(11, 37).cuda()).square().mean().backward()
    for a, b in zip(reducer.flat, reducer2.flat):
        b.copy_(a)
    opt.step(); opt2.step()
    assert _same(_snapshot(opt), _snapshot(opt2))
    assert opt.counters() == opt2.counters() == (6, 3)


def test_captured_step_equals_eager_step():
    from lintransunet_amd import train, optim
    torch.manual_seed(0)
    model_a, _ = _small_pair()
    model_b = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5)).cuda()
    model_b.load_state_dict(model_a.state_dict())
    kw = dict(lr=1e-2, max_grad_norm=0.25, skip_nonfinite=True, ema_decay=0.9)
    red_a, red_b = train.GradReducer(model_a, bucket_mb=4e-6), train.GradReducer(model_b, bucket_mb=4e-6)      # four buckets
    opt_a, opt_b = optim.FusedAdamW(red_a, **kw), optim.FusedAdamW(red_b, **kw)

    def feed(it, poisoned):
        gen = torch.Generator().manual_seed(100 + it)
        for fa, fb in zip(red_a.flat, red_b.flat):
            g = 0.05 * torch.randn(fa.numel(), generator=gen)
            fa.copy_(g); fb.copy_(g)
        if poisoned:
            red_a.flat[1][1] = float('nan'); red_b.flat[1][1] = float('nan')

    # warm-up of the stream capture on a side stream, as torch asks for; the eager twin takes the same (applied) step
    feed(99, False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt_b.step()
    torch.cuda.current_stream().wait_stream(side)
    opt_a.step()
    assert _same(_snapshot(opt_a), _snapshot(opt_b))
    graph = torch.cuda.CUDAGraph()
    feed(98, False)
    with torch.cuda.graph(graph):
        opt_b.step()                                         # captured, not executed
    graph.replay()
    opt_a.step()
    assert _same(_snapshot(opt_a), _snapshot(opt_b)) and opt_a.counters() == opt_b.counters() == (2, 0)
    for it in range(4):
        feed(it, poisoned=it in (1, 3))                      # the second and the fourth gradient carry a NaN
        opt_a.step()
        graph.replay()
        assert _same(_snapshot(opt_a), _snapshot(opt_b)), it
        assert opt_a.counters() == opt_b.counters() == (2 + (it + 2) // 2, (it + 1) // 2), it
    assert opt_a.counters() == (4, 2)


def test_ema_evaluation_through_the_model():
    from lintransunet_amd import train, optim
    from lintransunet_amd.model import get_model_dict
    from oracle import seedgen, step as O_step
    torch.manual_seed(1)
    make = lambda: get_model_dict('MaskTransUnet')([8, 8, 8, 16, 32], [20, 12, 9, 10, 6], [False, True, True, True, True], 1, 2,
                                                   dropout=0.0)
    model = make().cuda().train()
    unused0 = {k: v.detach().clone() for k, v in model.named_parameters() if k in train.UNUSED_PARAMETERS}
    assert len(unused0) == 14
    reducer = train.GradReducer(model, unused=train.UNUSED_PARAMETERS)
    opt = optim.FusedAdamW(reducer, lr=2e-3, weight_decay=0.0, max_grad_norm=1.0, ema_decay=0.5)
    x = seedgen.seeded_volume((2, 1, 32, 32, 32), 11).cuda()
    lab = seedgen.seeded_label((2, 1, 32, 32, 32), 12).cuda()
    step = train.GraphedStep(model, x, lab, O_step.dynamic_weights(0), reducer)
    for _ in range(4):
        step(x, lab)
        opt.step()
    assert opt.counters() == (4, 0)
    esd = opt.ema_state_dict(model)
    assert len(esd) == 614 and list(esd) == list(model.state_dict())
    for k, v in unused0.items():
        assert torch.equal(esd[k], v), k
    changed = sum(not torch.equal(esd[k], v) for k, v in model.state_dict().items())
    assert changed >= 100, changed                           # the average lags behind the weights
    model2 = make().cuda().eval()
    model2.load_state_dict(esd, strict=True)
    model.eval()
    with torch.no_grad():
        want = model2(x, probs=True).clone()
        plain = model(x, probs=True).clone()
        before = [t.clone() for t in opt.flat_p]
        ptrs = [t.data_ptr() for t in opt.flat_p]
        with opt.ema_weights():
            inside = model(x, probs=True).clone()
        assert torch.equal(inside, want)
        assert not torch.equal(inside, plain)
        assert _same(opt.flat_p, before) and ptrs == [t.data_ptr() for t in opt.flat_p]
        assert torch.equal(model(x, probs=True), plain)
    model.train()
    w0 = model.decode.final_block.weight.detach().clone()
    step(x, lab)                                             # the capture is still valid: no storage moved
    opt.step()
    assert opt.counters() == (5, 0)
    assert (model.decode.final_block.weight.detach() - w0).abs().max().item() > 0


def test_argument_errors_write_nothing():
    from lintransunet_amd import _lib
    from lintransunet_amd.ops import _p, _s
    lib = _lib.load()
    sizes = [1, 3, 4, 1023, 2 ** 22 + 3]
    parts = [lib.ltu_grad_sumsq_parts(n) for n in sizes]
    assert all(p > 0 for p in parts) and parts == sorted(parts), parts
    n = 5003                                                       # a tail of three
    need = lib.ltu_grad_sumsq_parts(n)
    assert need >= 2
    buf = torch.ones(n + 4, device='cuda')
    scratch = torch.full((need + 4,), -7.0, device='cuda')
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):          # a scratch one float short
        _lib.call('ltu_grad_sumsq', _p(buf), n, 1.0, _p(scratch), need - 1, _s())
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):          # gradient pointer 4 bytes off a 16-byte boundary
        _lib.call('ltu_grad_sumsq', _p(buf) + 4, n, 1.0, _p(scratch), need, _s())
    assert torch.equal(scratch, torch.full_like(scratch, -7.0))
    state = torch.zeros(12, device='cuda')
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):          # NaN max_norm
        _lib.call('ltu_adamw_guard', _p(scratch), need, _p(state), 1.0, float('nan'), 1, 0.9, 0.999, _s())
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):          # misaligned state
        _lib.call('ltu_adamw_guard', _p(scratch), need, _p(state) + 4, 1.0, 0.0, 1, 0.9, 0.999, _s())
    assert torch.equal(state, torch.zeros_like(state))
    _lib.call('ltu_grad_sumsq', _p(buf), n, 1.0, _p(scratch), need, _s())
    _lib.call('ltu_adamw_guard', _p(scratch), need, _p(state), 1.0, 0.0, 1, 0.9, 0.999, _s())
    assert abs(state[0].item() - n ** 0.5) <= NORM_RTOL * n ** 0.5
    assert torch.equal(scratch[need:], torch.full((4,), -7.0, device='cuda'))
    p, m, v, e = (torch.full((n + 4,), c, device='cuda') for c in (1.0, 2.0, 3.0, 4.0))
    args = lambda pp, ee, d: (pp, _p(buf), _p(m), _p(v), ee, n, 1e-2, 0.9, 0.999, 1e-8, 1e-2, d, _p(state), _s())
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):          # ema_decay = 1 with an EMA buffer
        _lib.call('ltu_adamw_guarded', *args(_p(p), _p(e), 1.0))
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):          # misaligned parameter pointer
        _lib.call('ltu_adamw_guarded', *args(_p(p) + 4, _p(e), 0.9))
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):          # misaligned EMA pointer
        _lib.call('ltu_adamw_guarded', *args(_p(p), _p(e) + 8, 0.9))
    for t, c in ((p, 1.0), (m, 2.0), (v, 3.0), (e, 4.0)):
        assert torch.equal(t, torch.full_like(t, c))
    _lib.call('ltu_adamw_guarded', *args(_p(p), _p(e), 0.9))       # the same call, valid: writes n elements and no more
    for t, c in ((p, 1.0), (m, 2.0), (v, 3.0), (e, 4.0)):
        assert not (t[:n] == c).any().item() and torch.equal(t[n:], torch.full((4,), c, device='cuda'))
