"""optim.FusedSGD and ltu_sgd / ltu_sgd_guarded on the GPU (csrc/optim.hip).  The oracle is torch on the CPU: torch.optim.SGD, with
torch.nn.utils.clip_grad_norm_ where clipping is on, a step not taken for a skipped one, and an EMA computed from the reference's
weights after each step.  Fixtures and gates are those of test_gpu_optim_guard.py: the 37-19-5 two-layer model in one 822-element
bucket or in buckets of 5, 95, 19 and 703 elements; parameters, momentum buffers (by their effect on the parameters) and EMA
rtol 2e-5 / atol 2e-7, the norm 1e-5 relative.  For scale: torch's own fp32 SGD drifts from its float64 run by 1.2e-6 relative /
3.5e-8 absolute over 9 such steps at the nnU-Net settings."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL, NORM_RTOL = 2e-5, 2e-7, 1e-5
BUCKET_MB = [0.001, 4e-6]
NNUNET = dict(momentum=0.99, nesterov=True, weight_decay=3e-5)


def _two_layer():
    return torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5))


def _small_pair():
    """the CPU reference first, the GPU model a copy of it"""
    ref, model = _two_layer(), _two_layer()
    model.load_state_dict(ref.state_dict())
    return model.cuda(), ref


def _backward(model, ref, x):
    model(x.cuda()).square().mean().backward()
    ref(x).square().mean().backward()


def _assert_params_close(model, ref, what):
    for (k, a), (_, b) in zip(model.state_dict().items(), ref.state_dict().items()):
        assert torch.allclose(a.cpu().to(b.dtype), b, rtol=RTOL, atol=ATOL), (what, k, (a.cpu() - b).abs().max().item())


def _snapshot(opt):
    return [t.clone() for group in (opt.flat_p, opt.buf, opt.ema) for t in group]


def _same(a, b):
    # bit-exact, NaN-free buffers
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _ema_by_name(opt, model):
    sd = opt.ema_state_dict(model)
    return {k: sd[k].cpu() for k, _ in model.named_parameters()}


# ---------------------------------------------------------------------------------------------- 1. against torch.optim.SGD

@pytest.mark.parametrize('bucket_mb', BUCKET_MB)
@pytest.mark.parametrize('kw', [dict(), dict(momentum=0.9, dampening=0.1, weight_decay=1e-2), NNUNET], ids=['lr_only', 'dampened', 'nnunet'])
def test_matches_torch_over_nine_steps(kw, bucket_mb):
    from lintransunet_amd import train, optim
    torch.manual_seed(0)
    model, ref = _small_pair()
    reducer = train.GradReducer(model, bucket_mb=bucket_mb)
    assert [f.numel() for f in reducer.flat] == ([822] if bucket_mb == 0.001 else [5, 95, 19, 703])
    opt = optim.FusedSGD(reducer, lr=1e-2, **kw)
    topt = torch.optim.SGD(ref.parameters(), lr=1e-2, **kw)
    if not kw:
        assert opt.buf == [] and 'buf' in opt.state_dict() and opt.state_dict()['buf'] == []          # no momentum storage
    else:
        assert [b.numel() for b in opt.buf] == [f.numel() for f in reducer.flat]
    for it in range(9):
        x = torch.randn(11, 37)
        opt.zero_grad(); topt.zero_grad()
        _backward(model, ref, x)
        opt.step(); topt.step()
        _assert_params_close(model, ref, it)
    assert opt.counters() == (9, 0)
    norm = torch.cat([p.grad.reshape(-1) for p in ref.parameters()]).double().norm().item()
    assert abs(opt.grad_norm.item() - norm) <= NORM_RTOL * norm          # the guard launches run without clip or skip, too


@pytest.mark.parametrize('kw', [dict(), dict(ema_decay=0.9, **NNUNET)], ids=['lr_only', 'nnunet_ema'])
def test_best_checkpoint_takes_the_optimizer_unchanged(kw, tmp_path):
    from lintransunet_amd import train, optim
    torch.manual_seed(0)
    model, _ = _small_pair()
    reducer = train.GradReducer(model, bucket_mb=4e-6)
    opt = optim.FusedSGD(reducer, lr=1e-2, **kw)
    model(torch.randn(11, 37).cuda()).square().mean().backward()
    opt.step()
    assert optim.BestCheckpoint(str(tmp_path), rank=0).update(model, 1.0, 1.0, optimizer=opt)
    side = torch.load(tmp_path / 'temp_model.extra.pt')['optimizer']
    assert (side['step'], side['skipped']) == (1, 0) and side['param_groups'] == opt.param_groups
    assert len(side['buf']) == len(opt.buf) and all(torch.equal(a, b.cpu()) for a, b in zip(side['buf'], opt.buf))
    assert ('ema' in side) == bool(kw)
    assert list(torch.load(tmp_path / 'temp_model.pt')) == list(model.state_dict())


# ---------------------------------------------------------------------------------------------- 2. clipping

@pytest.mark.parametrize('bucket_mb', BUCKET_MB)
def test_clipping_matches_torch(bucket_mb):
    """the reference's norms on this seed lie between 0.44 and 0.62, six above and three below 0.505"""
    from lintransunet_amd import train, optim
    torch.manual_seed(0)
    model, ref = _small_pair()
    reducer = train.GradReducer(model, bucket_mb=bucket_mb)
    opt = optim.FusedSGD(reducer, lr=1e-2, momentum=0.9, max_grad_norm=0.505)
    topt = torch.optim.SGD(ref.parameters(), lr=1e-2, momentum=0.9)
    norms = []
    for it in range(9):
        x = torch.randn(11, 37)
        opt.zero_grad(); topt.zero_grad()
        _backward(model, ref, x)
        norm = torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.505).item()
        opt.step(); topt.step()
        norms.append(norm)
        got = opt.grad_norm.item()
        print(f'step {it}: cpu norm {norm:.6f} gpu norm {got:.6f} rel {abs(got - norm) / norm:.2e}')
        assert abs(got - norm) <= NORM_RTOL * norm, (it, got, norm)
        _assert_params_close(model, ref, it)
    # judged by the reference's own norms the threshold is crossed both ways: clipping is neither idle nor always on
    assert sum(n > 0.505 for n in norms) >= 2 and sum(n < 0.505 for n in norms) >= 2, norms
    assert opt.counters() == (9, 0)


# ---------------------------------------------------------------------------------------------- 3. skipping

@pytest.mark.parametrize('bucket_mb', BUCKET_MB)
def test_nonfinite_steps_are_skipped(bucket_mb):
    """the FIRST step is skipped, with dampening 0.1: the step after it must be torch's first step (buf = g, not 0.9 g), or the
    gate fails from there on"""
    from lintransunet_amd import train, optim
    torch.manual_seed(0)
    model, ref = _small_pair()
    reducer = train.GradReducer(model, bucket_mb=bucket_mb)
    kw = dict(lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=1e-2)
    opt = optim.FusedSGD(reducer, skip_nonfinite=True, ema_decay=0.9, **kw)
    topt = torch.optim.SGD(ref.parameters(), **kw)
    ema = {k: v.detach().clone() for k, v in ref.named_parameters()}
    flat = reducer.flat
    assert flat[-1].numel() & 3                              # the last element of the last bucket is on the tail path
    mid = flat[len(flat) // 2]
    applied = skipped = 0

    def good_step():
        nonlocal applied
        x = torch.randn(11, 37)
        opt.zero_grad(); topt.zero_grad()
        _backward(model, ref, x)
        opt.step(); topt.step()
        applied += 1
        _assert_params_close(model, ref, applied)
        mine = _ema_by_name(opt, model)
        for k, p in ref.named_parameters():
            ema[k] = 0.9 * ema[k] + 0.1 * p.detach()
            assert torch.allclose(mine[k], ema[k], rtol=RTOL, atol=ATOL), (applied, k)
        assert opt.counters() == (applied, skipped)

    def poisoned_step(bucket, idx, value):
        nonlocal skipped
        opt.zero_grad(); topt.zero_grad()
        _backward(model, ref, torch.randn(11, 37))
        bucket[idx] = value
        before = _snapshot(opt)
        opt.step()                                           # the reference skips by not stepping
        skipped += 1
        assert _same(_snapshot(opt), before), (bucket.numel(), idx, value)
        assert opt.counters() == (applied, skipped)
        assert not torch.isfinite(opt.grad_norm).item()

    poisoned_step(flat[0], 0, float('nan'))                  # before anything was applied
    assert all(not b.any().item() for b in opt.buf)
    for _ in range(3):
        good_step()
    poisoned_step(flat[0], 0, float('nan'))
    poisoned_step(flat[-1], flat[-1].numel() - 1, float('inf'))
    poisoned_step(mid, mid.numel() // 2, float('-inf'))
    for _ in range(2):
        good_step()
    sd = opt.state_dict()
    assert sd['step'] == 5 and sd['skipped'] == 4 and len(sd['ema']) == len(sd['buf']) == len(flat)
    # a fresh optimizer on a copy of the model, restored from the state dict, takes the next step bit-identically
    model2 = _two_layer().cuda()
    model2.load_state_dict(model.state_dict())
    reducer2 = train.GradReducer(model2, bucket_mb=bucket_mb)
    opt2 = optim.FusedSGD(reducer2, skip_nonfinite=True, ema_decay=0.9, **dict(kw, lr=3e-3))
    opt2.load_state_dict(sd)                                 # brings the learning rate along, to the device too
    assert opt2.counters() == (5, 4) and opt2.param_groups == opt.param_groups
    opt.zero_grad()
    model(torch.randn(11, 37).cuda()).square().mean().backward()
    for a, b in zip(reducer.flat, reducer2.flat):
        b.copy_(a)
    opt.step(); opt2.step()
    assert _same(_snapshot(opt), _snapshot(opt2))
    assert opt.counters() == opt2.counters() == (6, 4)


# ---------------------------------------------------------------------------------------------- 4. more than one grid sweep

class _TwoLinears(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.big = torch.nn.Linear(2048, 2100)
        self.tiny = torch.nn.Linear(3, 1)


def test_bucket_larger_than_one_grid_sweep_with_ema():
    """buckets of 1, 3, 2 100 and 4 300 800 elements: the last is more than the 4096 x 256 x 4 elements one sweep of the capped grid
    covers, the first two are less than one workgroup (and the tail path only).  Nesterov + clip + EMA, step 0 clipped (norm
    about 2.07), step 1 not (about 0.41).  The reference is clip_grad_norm_ + SGD.step on a FLOAT64 copy of the model (over 4.3 M
    elements torch's fp32 norm is itself off by 1e-4, ten times the gate), and both sides are fed the SAME gradient bits, drawn
    in fp32 on the CPU and copied into the buckets, as test_gpu_optim_guard.py explains for AdamW: the gate then measures the
    update's arithmetic and not two matrix products' last bits."""
    from lintransunet_amd import train, optim
    torch.manual_seed(3)
    ref = _TwoLinears()
    model = _TwoLinears()
    model.load_state_dict(ref.state_dict())
    model, ref = model.cuda(), ref.double()
    reducer = train.GradReducer(model, bucket_mb=4e-6)          # a cap of one float: every parameter is its own bucket
    assert sorted(f.numel() for f in reducer.flat) == [1, 3, 2100, 2048 * 2100]
    assert 2048 * 2100 // 4 > 4096 * 256
    opt = optim.FusedSGD(reducer, lr=1e-2, max_grad_norm=1.0, ema_decay=0.9, **NNUNET)
    topt = torch.optim.SGD(ref.parameters(), lr=1e-2, **NNUNET)
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
    assert opt.counters() == (2, 0)


# ---------------------------------------------------------------------------------------------- 5. one arithmetic, every instantiation

def _guard_state(coef, applied, skip=0):
    state = torch.zeros(12, device='cuda')
    state[1] = coef
    state[4:5].view(torch.int32)[0] = skip
    state[6:10].view(torch.int64)[0] = applied
    return state


@pytest.mark.parametrize('first', [1, 0])
@pytest.mark.parametrize('mom,damp,nest', [(0.0, 0.0, 0), (0.9, 0.1, 0), (0.99, 0.0, 1)])
def test_every_instantiation_gives_the_same_bits(mom, damp, nest, first):
    """ltu_sgd against ltu_sgd_guarded (state: coef = grad_scale, applied = 1 iff first_step, the same lr on the device) without
    and with an EMA buffer: bit-equal p and buf; two identical calls: the same bits; and the float64 formula within the gates"""
    from lintransunet_amd import _lib
    from lintransunet_amd.ops import _p, _s
    n, lr, wd, scale, d = 4 * 256 * 3 + 3, 0.0123, 1e-2, 0.37, 0.9          # three workgroups and a tail of three
    gen = torch.Generator().manual_seed(7)
    p0, g, b0, e0 = (torch.randn(n, generator=gen).cuda() for _ in range(4))
    lr_dev = torch.full((1,), lr, device='cuda')
    state = _guard_state(scale, 1 if first else 5)

    def run(which):
        p, b, e = p0.clone(), b0.clone(), e0.clone()
        pb = _p(b) if mom else 0
        if which == 'plain':
            _lib.call('ltu_sgd', _p(p), _p(g), pb, n, lr, mom, damp, wd, nest, first, scale, _s())
        else:
            _lib.call('ltu_sgd_guarded', _p(p), _p(g), pb, _p(e) if which == 'ema' else 0, n, _p(lr_dev), mom, damp, wd, nest, d,
                      _p(state), _s())
        return p, b, e

    plain, guarded, with_ema, again = run('plain'), run('guarded'), run('ema'), run('ema')
    for other in (guarded, with_ema):
        assert torch.equal(plain[0], other[0]) and torch.equal(plain[1], other[1])
    assert all(torch.equal(a, b) for a, b in zip(with_ema, again))
    assert torch.equal(plain[2], e0) and torch.equal(guarded[2], e0)
    if not mom:
        assert torch.equal(plain[1], b0)                     # no load, no store
    # the formula in float64, on the fp32 inputs (lr as the device holds it)
    P, G, B = p0.double().cpu(), g.double().cpu() * float(torch.tensor(scale, dtype=torch.float32)), b0.double().cpu()
    G = G + float(torch.tensor(wd, dtype=torch.float32)) * P
    if mom:
        m32, omd = float(torch.tensor(mom, dtype=torch.float32)), float(1 - torch.tensor(damp, dtype=torch.float32))
        B = G if first else m32 * B + omd * G
        G = G + m32 * B if nest else B
        assert torch.allclose(with_ema[1].double().cpu(), B, rtol=RTOL, atol=ATOL)
    P = P - lr_dev.item() * G
    assert torch.allclose(with_ema[0].double().cpu(), P, rtol=RTOL, atol=ATOL)
    assert torch.allclose(with_ema[2].double().cpu(), 0.9 * e0.double().cpu() + 0.1 * P, rtol=RTOL, atol=ATOL)
    # skip = 1: nothing is written
    skip = _guard_state(scale, 3, skip=1)
    p, b, e = p0.clone(), b0.clone(), e0.clone()
    _lib.call('ltu_sgd_guarded', _p(p), _p(g), _p(b) if mom else 0, _p(e), n, _p(lr_dev), mom, damp, wd, nest, d, _p(skip), _s())
    assert torch.equal(p, p0) and torch.equal(b, b0) and torch.equal(e, e0)


# ---------------------------------------------------------------------------------------------- 6. capture under a moving lr

def test_captured_step_follows_a_moving_learning_rate():
    """twin optimizers, one eager and one captured ONCE, under PolyLR(total_iters=6) stepping between the steps: bit-equal after
    every step (two of them skipped), equal to torch's SGD run with the same lr sequence within the gates, and different from a run
    with the learning rate held: the replays read the device scalar"""
    from lintransunet_amd import train, optim
    torch.manual_seed(0)
    model_a, ref = _small_pair()
    model_b, model_c = _two_layer().cuda(), _two_layer().cuda()
    model_b.load_state_dict(model_a.state_dict()); model_c.load_state_dict(model_a.state_dict())
    kw = dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=3e-5, max_grad_norm=0.25, skip_nonfinite=True, ema_decay=0.9)
    reds = [train.GradReducer(m, bucket_mb=4e-6) for m in (model_a, model_b, model_c)]          # four buckets each
    opt_a, opt_b, opt_c = (optim.FusedSGD(r, **kw) for r in reds)
    topt = torch.optim.SGD(ref.parameters(), lr=1e-2, momentum=0.9, nesterov=True, weight_decay=3e-5)
    name_of = {id(p): k for k, p in model_b.named_parameters()}
    ref_params = dict(ref.named_parameters())

    def feed(it, poisoned):
        gen = torch.Generator().manual_seed(100 + it)
        for bucket, flats in zip(reds[1].buckets, zip(*(r.flat for r in reds))):
            g = 0.05 * torch.randn(flats[0].numel(), generator=gen)
            for f in flats:
                f.copy_(g)
            off = 0
            for p in bucket:                                 # the same bits as the reference's gradients
                ref_params[name_of[id(p)]].grad = g[off:off + p.numel()].view(p.shape).clone()
                off += p.numel()
        if poisoned:
            for r in reds:
                r.flat[1][1] = float('nan')

    def reference_step(lr):
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.25)
        topt.param_groups[0]['lr'] = lr
        topt.step()

    # warm-up of the stream capture on a side stream, as torch asks for; everyone takes the same (applied) step
    feed(99, False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt_b.step()
    torch.cuda.current_stream().wait_stream(side)
    opt_a.step(); opt_c.step(); reference_step(1e-2)
    assert _same(_snapshot(opt_a), _snapshot(opt_b))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_b.step()                                         # captured, not executed
    assert opt_b.counters() == (1, 0)
    sched_a, sched_b = optim.PolyLR(opt_a, total_iters=6), optim.PolyLR(opt_b, total_iters=6)
    lrs = []
    for it in range(6):
        poisoned = it in (1, 4)
        feed(it, poisoned)
        lrs.append(opt_b.param_groups[0]['lr'])
        opt_a.step(); opt_c.step()
        graph.replay()
        if not poisoned:
            reference_step(lrs[-1])
        assert _same(_snapshot(opt_a), _snapshot(opt_b)), it
        applied = 1 + sum(k not in (1, 4) for k in range(it + 1))
        assert opt_a.counters() == opt_b.counters() == (applied, it + 1 - (applied - 1)), it
        _assert_params_close(model_b, ref, it)
        assert torch.equal(opt_b._lr_dev.cpu(), torch.tensor([lrs[-1]], dtype=torch.float32))
        sched_a.step(); sched_b.step()
    assert lrs == [1e-2 * (1 - t / 6) ** 0.9 for t in range(6)] and opt_b.param_groups[0]['lr'] == 0.0
    assert opt_b.counters() == (5, 2) and opt_c.counters() == (5, 2)
    # with the learning rate held, every bucket ends up elsewhere: outside the gates
    assert opt_c.param_groups[0]['lr'] == 1e-2
    for pb, pc in zip(opt_b.flat_p, opt_c.flat_p):
        assert not torch.allclose(pb, pc, rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------- 7. argument errors

def test_argument_errors_write_nothing():
    from lintransunet_amd import _lib
    from lintransunet_amd.ops import _p, _s
    n = 5003                                                       # a tail of three
    p, g, b, e = (torch.full((n + 4,), c, device='cuda') for c in (1.0, 0.5, 3.0, 4.0))
    lr_dev = torch.full((4,), 1e-2, device='cuda')
    state = _guard_state(1.0, 2)
    state0 = state.clone()

    def guarded(pp=None, gg=None, bb=None, ee=None, nn=n, lr=None, mom=0.9, damp=0.0, wd=1e-2, nest=0, d=0.9, st=None):
        pick = lambda v, default: default if v is None else v
        return ('ltu_sgd_guarded', pick(pp, _p(p)), pick(gg, _p(g)), pick(bb, _p(b)), pick(ee, _p(e)), nn, pick(lr, _p(lr_dev)), mom,
                damp, wd, nest, d, pick(st, _p(state)), _s())

    def plain(pp=None, gg=None, bb=None, nn=n, lr=1e-2, mom=0.9, damp=0.0, wd=1e-2, nest=0, first=0, scale=1.0):
        pick = lambda v, default: default if v is None else v
        return ('ltu_sgd', pick(pp, _p(p)), pick(gg, _p(g)), pick(bb, _p(b)), nn, lr, mom, damp, wd, nest, first, scale, _s())

    nan = float('nan')
    bad = [guarded(d=1.0), guarded(d=-0.1), guarded(d=nan),           # ema_decay outside [0, 1) with an EMA buffer
           guarded(pp=_p(p) + 4), guarded(gg=_p(g) + 8), guarded(bb=_p(b) + 4), guarded(ee=_p(e) + 8),          # misaligned buffers
           guarded(st=_p(state) + 4), guarded(st=0),                  # misaligned / null state
           guarded(lr=0), guarded(lr=_p(lr_dev) + 2),                 # null / misaligned learning-rate pointer
           guarded(pp=0), guarded(gg=0), guarded(bb=0),               # null buffers (momentum without its buffer)
           guarded(mom=0.0),                                          # a momentum buffer without momentum
           guarded(nest=1, mom=0.0, bb=0), guarded(nest=1, damp=0.1),          # torch's Nesterov rule
           guarded(mom=nan), guarded(mom=-0.5), guarded(damp=nan), guarded(wd=nan), guarded(wd=-1e-2),
           plain(lr=nan), plain(lr=-1e-2), plain(scale=nan), plain(mom=nan), plain(damp=nan), plain(wd=nan),
           plain(nest=1, mom=0.0, bb=0), plain(nest=1, damp=0.1), plain(gg=_p(g) + 4), plain(pp=_p(p) + 12), plain(bb=0), plain(mom=0.0)]
    for call in bad:
        with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
            _lib.call(*call)
    _lib.call(*guarded(nn=0)); _lib.call(*plain(nn=0)); _lib.call(*guarded(nn=-3))          # nothing to do: LTU_OK
    for t, c in ((p, 1.0), (g, 0.5), (b, 3.0), (e, 4.0)):
        assert torch.equal(t, torch.full_like(t, c))
    assert torch.equal(state, state0) and torch.equal(lr_dev, torch.full_like(lr_dev, 1e-2))
    _lib.call(*guarded())                                          # the same call, valid: writes n elements and no more
    for t, c in ((p, 1.0), (b, 3.0), (e, 4.0)):
        assert not (t[:n] == c).any().item() and torch.equal(t[n:], torch.full((4,), c, device='cuda'))
    _lib.call(*plain())
    for t, c in ((p, 1.0), (b, 3.0)):
        assert torch.equal(t[n:], torch.full((4,), c, device='cuda'))
    assert torch.equal(g, torch.full_like(g, 0.5)) and torch.equal(state, state0)
    assert torch.equal(e[n:], torch.full((4,), 4.0, device='cuda'))


# ---------------------------------------------------------------------------------------------- 8. through the model

def test_nnunet_recipe_through_the_model():
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
    opt = optim.nnunet_sgd(reducer, ema_decay=0.5)
    sched = optim.nnunet_schedule(opt)
    assert opt.param_groups[0] == dict(lr=1e-2, momentum=0.99, dampening=0.0, weight_decay=3e-5, nesterov=True)
    x = seedgen.seeded_volume((2, 1, 32, 32, 32), 11).cuda()
    lab = seedgen.seeded_label((2, 1, 32, 32, 32), 12).cuda()
    step = train.GraphedStep(model, x, lab, O_step.dynamic_weights(0), reducer)
    for _ in range(4):
        step(x, lab)
        opt.step()
        sched.step()
    assert opt.counters() == (4, 0)
    assert opt._lr_dev.item() == torch.tensor(1e-2 * (1 - 4 / 1000) ** 0.9, dtype=torch.float32).item()
    esd = opt.ema_state_dict(model)
    assert len(esd) == 614 and list(esd) == list(model.state_dict())
    for k, v in unused0.items():
        assert torch.equal(esd[k], v), k
    assert all(torch.isfinite(v).all().item() for v in esd.values())
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
