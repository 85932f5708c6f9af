"""Region-based training on the GPU (csrc/region.hip, the sigmoid heads of csrc/pointwise.hip, ltu_roi_plan_union) against the float64
restatement of tests/region_common.py: heads, bit-masks and their pyramid, the ROI foreground, the loss stage, labels and counts, and
the model with its step.

Tolerance: each compared quantity is evaluated once more in float32 numpy on the test's own input; the kernels may deviate from the
float64 oracle by 4 x what that evaluation deviates, and at least by 4 ulps of the value (region_common.allowed_scalar number by number;
allowed_field for a gradient tensor, compared as one quantity: largest absolute deviation over the largest |value|).  A bf16 `dz` gets
one bf16 rounding of the float64 value on top.  Every test prints what it measured beside what it allowed."""
import functools

import numpy as np
import pytest
import torch

from oracle import net as O_net          # noqa: E402
from oracle import seedgen               # noqa: E402
from oracle import step as O_step        # noqa: E402
from tests import region_common as RC
from tests.test_gpu_conv_paths import launched

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32, BF16 = 0, 1
SMALL = dict(num_layers=[8, 8, 8, 16, 32], roi_size_list=[20, 12, 9, 10, 6])      # of tests/test_gpu_model.py
NON_NESTED = ((1, 2), (2, 3), (4,))
ODD = (9, 7, 5)                 # S = 315, S % 4 != 0: the scalar kernels, 2 workgroups a sample
ONE = (8, 8, 4)                 # S = 256, S % 4 == 0: the four-voxel kernels inside one workgroup's walk
MANY = (12, 10, 8)              # S = 960: 4 workgroups a sample, the last one ragged
LONG = (64, 64, 160)            # S = 655360 at B = 2: 1280 voxels a workgroup, a two-in-flight trip and a remainder trip (R <= 4)


def _lib():
    from lintransunet_amd import _lib as lib
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _t(x):
    return torch.tensor([x], device=DEV, dtype=torch.float32)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # a copy: the cached cases are read-only


def _worst(err, allowed):
    """largest err / allowed (0 / 0 counts as 0) and the entry it belongs to"""
    err, allowed = np.asarray(err, np.float64).ravel(), np.asarray(allowed, np.float64).ravel()
    ratio = np.where(err > 0, err / np.where(allowed > 0, allowed, 1e-300), 0.0)
    k = int(ratio.argmax())
    return float(ratio[k]), float(err[k]), float(allowed[k])


def _held(got, v64, v32, what, extra=None):
    """number by number: |got - v64| <= max(4 |v32 - v64|, 4 ulps) (+ extra); prints the worst entry"""
    allowed = RC.allowed_scalar(v64, v32) + (0.0 if extra is None else extra)
    err = np.abs(np.asarray(got, np.float64) - np.asarray(v64, np.float64))
    ratio, e, a = _worst(err, allowed)
    print(f'{what}: worst error {e:.3e} allowed {a:.3e} ({ratio:.2f} of the allowance)')
    assert np.isfinite(np.asarray(got, np.float64)).all() and ratio <= 1.0, (what, e, a)
    return ratio


# ---------------------------------------------------------------------------------------------- 1. heads
def _logits(M, CP, seed):
    rng = np.random.default_rng(seed)
    z = (4.0 * rng.standard_normal((M, CP))).astype(np.float32)
    z[0, :], z[1, :], z[2, :] = 100.0, -100.0, 0.0
    z[3, ::2], z[3, 1::2] = 100.0, -100.0
    z[5:25] *= 4.0                                                   # |z| up to ~60: exp(-z) from 1e-26 to 1e26
    return z


def _torch_dtype(dt):
    return torch.float32 if dt == F32 else torch.bfloat16


def _head_cps(R, dt):
    first = (R + 3) // 4 * 4 if dt == F32 else (R + 7) // 8 * 8
    return sorted({first, 16, 32})


def _offset_copy(t):
    """the same values one element further into a fresh buffer: rows that start off every vector boundary"""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


def _head_fwd(z, R):
    M, CP = z.shape
    p = torch.full((M, R), float('nan'), device=DEV)
    _lib().call('ltu_head_sigmoid_fwd', z.data_ptr(), p.data_ptr(), M, R, CP, F32 if z.dtype == torch.float32 else BF16, _stream())
    return p


def _head_bwd(dp, p, dz):
    M, CP = dz.shape
    _lib().call('ltu_head_sigmoid_bwd', dp.data_ptr(), p.data_ptr(), dz.data_ptr(), M, p.shape[1], CP,
                F32 if dz.dtype == torch.float32 else BF16, _stream())
    return dz


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('R', [1, 3, 5, 8])
def test_head_sigmoid(R, dt):
    M, tdt = 1000, _torch_dtype(dt)
    rng = np.random.default_rng(100 + R)
    dp_h = rng.standard_normal((M, R)).astype(np.float32)
    dp = _dev(dp_h)
    ref_p = None
    for CP in _head_cps(R, dt) + [2 * R + 1]:                        # .. and one odd width: rows off every boundary
        zh = _logits(M, CP, 7)                                       # the first R columns are the same numbers at every width
        zh[:, :R] = _logits(M, 32, 7)[:, :R]
        z = _dev(zh).to(tdt)
        z64 = z.float().cpu().numpy().astype(np.float64)[:, :R]
        p = _head_fwd(z, R)
        ph = p.cpu().numpy()
        assert (ph >= 0).all() and (ph <= 1).all()
        assert (ph[0] == 1).all() and (ph[1] == 0).all() and (ph[2] == 0.5).all()
        _held(ph, RC.sigmoid_ref(z64), RC.sigmoid_ref(z64.astype(np.float32), np.float32), f'head p R={R} CP={CP} dtype={dt}')
        if ref_p is None:
            ref_p = p
        assert torch.equal(p, ref_p), CP                             # vector and scalar launches of the same rows: the same bits
        assert torch.equal(_head_fwd(_offset_copy(z), R), ref_p), CP   # a misaligned base pointer: the scalar launch
        named = dt == BF16 and CP == 16                              # one case records what the two launches were
        run = launched if named else (lambda fn: (fn(), None))
        dz, k_dz = run(lambda: _head_bwd(dp, p, torch.full((M, CP), float('nan'), device=DEV, dtype=tdt)))
        dz_off, k_off = run(lambda: _head_bwd(dp, p, _offset_copy(torch.full((M, CP), float('nan'), device=DEV, dtype=tdt))))
        assert torch.equal(dz, dz_off), CP
        if named:                                                    # .. so that comparison is one between two kernels
            assert f'head_bwd_bf16x8_kernel<Sigmoid, {R}>' in k_dz, k_dz
            assert f'head_bwd_kernel<Sigmoid, bf16_t, {R}, false>' in k_off, k_off
        dzh = dz.float().cpu().numpy()
        assert not dzh[:, R:].any() and not np.signbit(dzh[:, R:]).any()      # padded columns: exactly 0
        d64 = RC.sigmoid_grad_ref(dp_h, ph)
        d32 = RC.sigmoid_grad_ref(dp_h, ph, np.float32)
        extra = None if dt == F32 else RC.bf16_half_ulp(np.abs(d64) + RC.allowed_scalar(d64, d32))
        _held(dzh[:, :R], d64, d32, f'head dz R={R} CP={CP} dtype={dt}', extra)


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('R', [1, 3, 5, 8])
def test_final_sigmoid(R, dt):
    B, h, w, D = 2, 3, 5, 7
    tdt = _torch_dtype(dt)
    rng = np.random.default_rng(200 + R)
    dp_h = rng.standard_normal((B, 2 * h, 2 * w, D, R)).astype(np.float32)
    first = 4 * R if dt == F32 else (4 * R + 7) // 8 * 8
    ref_p = None
    for CP in sorted({first, first + 8, 40}):
        zh = _logits(B * h * w * D, CP, 9)
        zh[:, :4 * R] = _logits(B * h * w * D, 40, 9)[:, :4 * R]
        z = _dev(zh.reshape(B, h, w, D, CP)).to(tdt)
        z64 = z.float().cpu().numpy().astype(np.float64)
        p = torch.full((B, 2 * h, 2 * w, D, R), float('nan'), device=DEV)
        _lib().call('ltu_final_sigmoid_fwd', z.data_ptr(), p.data_ptr(), B, h, w, D, R, CP, dt, _stream())
        ph = p.cpu().numpy()
        assert (ph >= 0).all() and (ph <= 1).all()
        _held(ph, RC.unembed_ref(RC.sigmoid_ref(z64), R), RC.unembed_ref(RC.sigmoid_ref(z64.astype(np.float32), np.float32), R),
              f'final p R={R} CP={CP} dtype={dt}')
        if ref_p is None:
            ref_p = p
        assert torch.equal(p, ref_p), CP
        dz = torch.full((B, h, w, D, CP), float('nan'), device=DEV, dtype=tdt)
        _lib().call('ltu_final_sigmoid_bwd', _dev(dp_h).data_ptr(), p.data_ptr(), dz.data_ptr(), B, h, w, D, R, CP, dt, _stream())
        dzh = dz.float().cpu().numpy()
        assert not dzh[..., 4 * R:].any()
        d64 = RC.embed_ref(RC.sigmoid_grad_ref(dp_h, ph), CP)
        d32 = RC.embed_ref(RC.sigmoid_grad_ref(dp_h, ph, np.float32), CP)
        extra = None if dt == F32 else RC.bf16_half_ulp(np.abs(d64) + RC.allowed_scalar(d64, d32))
        _held(dzh, d64, d32, f'final dz R={R} CP={CP} dtype={dt}', extra)


def test_heads_through_autograd():
    from lintransunet_amd import ops
    rng = np.random.default_rng(5)
    z = _dev(rng.standard_normal((4, 6, 5, 16)).astype(np.float32)).requires_grad_(True)
    g = _dev(rng.standard_normal((4, 6, 5, 3)).astype(np.float32))
    p = ops.head_sigmoid(z, 3)
    (dz,) = torch.autograd.grad(p, z, g)
    want = _head_bwd(g.reshape(-1, 3), p.detach().reshape(-1, 3), torch.empty((120, 16), device=DEV))
    assert p.shape == (4, 6, 5, 3) and torch.equal(dz.reshape(-1, 16), want)
    zf = _dev(rng.standard_normal((2, 3, 5, 7, 12)).astype(np.float32)).requires_grad_(True)
    pf = ops.final_sigmoid(zf, 3)
    (dzf,) = torch.autograd.grad(pf, zf, torch.ones_like(pf))
    ph = pf.detach().cpu().numpy()
    assert pf.shape == (2, 6, 10, 7, 3)
    _held(dzf.cpu().numpy(), RC.embed_ref(RC.sigmoid_grad_ref(np.ones_like(ph), ph), 12),
          RC.embed_ref(RC.sigmoid_grad_ref(np.ones_like(ph), ph, np.float32), 12), 'final dz through autograd')


# ---------------------------------------------------------------------------------------------- 2. bits and pyramid
@pytest.mark.parametrize('spatial,n_levels,shapes', [((8, 12, 6), 3, [(8, 12, 6), (4, 6, 6), (2, 3, 6)]),
                                                     ((8, 16, 12), 4, [(8, 16, 12), (4, 8, 12), (2, 4, 12), (1, 2, 6)])])
def test_bits_and_pyramid(spatial, n_levels, shapes):
    """2 x (8, 12, 6) as far as it pools - W = 12 halves to 6 and 3, and a third (2, 2, kd) window does not fit an odd extent, which
    ltu_bits_orpool refuses as ltu_label_maxpool does - and 2 x (8, 16, 12) through three poolings: the pyramid's (kd 1, 1, 2, the
    order of train.label_pyramid) and, pooling by pooling, kd alternating 1, 2, 1"""
    from lintransunet_amd import _lib as lib, losses as L, ops, train
    rng = np.random.default_rng(21)
    label = rng.integers(0, 5, (2, *spatial)).astype(np.uint8)
    label.reshape(-1)[rng.choice(label.size, 12, replace=False)] = 200      # stray values: in no region
    rec = L.Regions(NON_NESTED)
    want = RC.pyramid_ref(label, NON_NESTED, n_levels)
    got = train.region_pyramid(_dev(label).unsqueeze(1), rec, n_levels)
    assert len(got) == n_levels and [tuple(g.shape) for g in got] == [(2, *sh) for sh in shapes]
    for lvl, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.uint8 and np.array_equal(g.cpu().numpy(), w), lvl
    assert not want[0][label == 200].any() and (want[0] == 3).any()
    if shapes[-1][1] % 2:
        with pytest.raises(lib.LtuError):
            ops.bits_orpool(got[-1], 1)
    else:
        cur, ref = got[0], want[0]
        for kd in (1, 2, 1):
            cur, ref = ops.bits_orpool(cur, kd), RC.orpool_ref(ref, kd)
            assert np.array_equal(cur.cpu().numpy(), ref), kd
        assert tuple(cur.shape) == (2, 1, 2, 6)
    for kd in (1, 2):
        assert np.array_equal(ops.bits_orpool(got[0], kd).cpu().numpy(), RC.orpool_ref(want[0], kd))
    # what label_maxpool on the raw label would have given for these regions is something else
    assert not np.array_equal(RC.bits_ref(ops.label_maxpool(_dev(label), 1).cpu().numpy(), NON_NESTED), want[1])


# ---------------------------------------------------------------------------------------------- 3. ROI foreground
def test_roi_plan_union_against_the_two_channel_plan():
    from lintransunet_amd import ops
    rng = np.random.default_rng(31)
    B, H, W, D, R, roi = 3, 24, 20, 6, 3, 10
    p = (rng.integers(0, 32, (B, H, W, D, R)) / 64.0).astype(np.float32)       # below 0.5 everywhere ..
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    for b, (ch, cw, r) in enumerate(((9, 8, 0), (15, 11, 2))):      # .. but for a blob in one region; sample 2 stays empty
        blob = ((hh - ch) ** 2 + (ww - cw) ** 2 <= 16)[:, :, None]
        p[b, ..., r] = np.where(blob, (rng.integers(32, 65, (H, W, D)) / 64.0), p[b, ..., r]).astype(np.float32)
    assert (p.max(-1) == 0.5).any() and not (p[2].max(-1) >= 0.5).any()
    m = p.max(-1)
    p2 = np.stack([1.0 - m, m], -1).astype(np.float32)
    assert np.array_equal(1.0 - p2[..., 0].astype(np.float64), m.astype(np.float64))      # exact on the 1/64 grid
    a = ops.RoiPlan(_dev(p), roi, 0.5, union=True)
    b = ops.RoiPlan(_dev(p2), roi, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(a.box, b.box)
    # ibuf and fbuf, every entry the plan kernel writes: the taps src0 / wt, the adjoint lists' lengths cnt and their first cnt
    # entries lidx / lw (the lists are sized for the worst case and the rest of them is never written or read)
    from tests.stream_common import plan_offsets
    offs = plan_offsets(B, H, W, a.eval_h, a.eval_w)
    assert offs['n_int'] == a.ibuf.numel() == b.ibuf.numel() and offs['n_float'] == a.fbuf.numel() == b.fbuf.numel()
    ia, ib, fa, fb = a.ibuf.cpu(), b.ibuf.cpu(), a.fbuf.cpu(), b.fbuf.cpu()
    for name in ('fh', 'fw', 'bh', 'bw'):
        o = offs[name]
        ND, NS, Lmax = o['ND'], o['NS'], o['L']
        assert torch.equal(ia[o['src0']:o['lidx']], ib[o['src0']:o['lidx']]), name              # src0 and cnt
        assert torch.equal(fa[o['wt']:o['lw']].view(torch.int32), fb[o['wt']:o['lw']].view(torch.int32)), name
        cnt = ia[o['cnt']:o['cnt'] + B * NS].reshape(B, NS, 1)
        live = torch.arange(Lmax).reshape(1, 1, Lmax) < cnt
        la, lb = (t[o['lidx']:o['lidx'] + B * NS * Lmax].reshape(B, NS, Lmax) for t in (ia, ib))
        wa, wb = (t[o['lw']:o['lw'] + B * NS * Lmax].reshape(B, NS, Lmax).view(torch.int32) for t in (fa, fb))
        assert live.any() and torch.equal(la[live], lb[live]) and torch.equal(wa[live], wb[live]), name
    assert not torch.equal(a.box[0], a.box[2])                       # the blob moved the box off the empty-foreground one


# ---------------------------------------------------------------------------------------------- 4. the stage
class Stage:
    """ltu_loss_region_fwd / _bwd on one (p, bits) through the raw C-ABI; the scratch is filled with garbage first"""

    def __init__(self, p, bits):
        self.lib = _lib()
        self.p, self.bits = _dev(p), _dev(bits)
        self.B, self.R = p.shape[0], p.shape[-1]
        self.S = int(np.prod(p.shape[1:-1]))
        self.need = self.lib.load().ltu_loss_region_ws_floats(self.B, self.S, self.R)
        assert self.need > 0
        self.sums = torch.full((self.need,), float('nan'), device=DEV)
        self.coef = torch.full((self.B, self.R, 3), float('nan'), device=DEV)

    def fwd(self, w_bce=1.0, w_dice=1.0, batch=True, eps=1e-5, base_total=None, scale_dev=None):
        values = torch.full((self.R + 4,), float('nan'), device=DEV)
        self.lib.call('ltu_loss_region_fwd', self.p.data_ptr(), self.bits.data_ptr(), self.sums.data_ptr(), self.need, values.data_ptr(),
                      self.coef.data_ptr(), _ptr(base_total), w_bce, w_dice, int(batch), eps, _ptr(scale_dev), self.B, self.S, self.R, _stream())
        return values.cpu().numpy()

    def bwd(self, dp=None, accumulate=0, g=1.0):
        dp = torch.full_like(self.p, float('nan')) if dp is None else dp
        self.lib.call('ltu_loss_region_bwd', self.p.data_ptr(), self.bits.data_ptr(), self.coef.data_ptr(), self.coef.numel(), _t(g).data_ptr(),
                      dp.data_ptr(), accumulate, self.B, self.S, self.R, _stream())
        return dp.cpu().numpy()

    def kernel_sums(self):
        s = self.sums[:self.B * self.R * 4].cpu().numpy().reshape(self.B, self.R, 4)
        return s[..., 0], s[..., 1], s[..., 2], s[..., 3]


@functools.lru_cache(maxsize=None)
def _case(B, spatial, R, late):
    members = NON_NESTED if R == 3 else None
    p, label, bits, members = RC.make_region_case(B, spatial, R, 17 * B + R, members)
    if late:
        p = RC.late_region_probs(bits, R, 23 * B + R)
    for a in (p, bits):
        a.setflags(write=False)
    return p, bits


def _check_stage(st, p, bits, cfg, what):
    """forward + backward of one setting against the oracle; -> (values, dp)"""
    r64, r32 = RC.region_ref(p, bits, **cfg), RC.region_ref(p, bits, dtype=np.float32, **cfg)
    v = st.fwd(**cfg)
    assert v[0] == v[-1]                                             # the second copy of the total
    _held(v[:-1], RC.report(r64), RC.report(r32), f'{what}: report')
    ks = st.kernel_sums()
    assert all((x >= 0).all() for x in ks)                           # I, FP, FN, E: no difference of two sums anywhere
    for name, got, s64, s32 in zip('I FP FN E'.split(), ks, r64['sums'], r32['sums']):
        _held(got, s64, s32, f'{what}: {name}')
    dp = st.bwd()
    allowed, err = RC.allowed_field(r64['grad'], r32['grad']), RC.field_error(dp, r64['grad'])
    print(f'{what}: dp error {err:.3e} allowed {allowed:.3e}')
    assert np.isfinite(dp).all() and err <= allowed, (what, err, allowed)
    return v, dp


@pytest.mark.parametrize('late', [False, True])
@pytest.mark.parametrize('batch', [False, True])
@pytest.mark.parametrize('spatial', [ODD, ONE, MANY])
@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('R', [1, 3, 8])
def test_stage_against_float64(R, B, spatial, batch, late):
    p, bits = _case(B, spatial, R, late)
    if late:
        assert ((p == 0) | (p == 1)).mean() > 0.9
    st = Stage(p, bits)
    cfg = dict(w_bce=0.75, w_dice=1.25, batch=batch, eps=1e-5)
    v, dp = _check_stage(st, p, bits, cfg, f'R={R} B={B} {spatial} batch={batch} late={late}')
    assert np.array_equal(st.fwd(**cfg), v) and np.array_equal(st.bwd(), dp)      # a second call: bit for bit


def test_stage_long_rows():
    p, bits = _case(2, LONG, 3, False)
    _check_stage(Stage(p, bits), p, bits, dict(w_bce=1.0, w_dice=1.0, batch=True, eps=1e-5), f'R=3 B=2 {LONG}')


def test_stage_written_scale_and_before():
    p, bits = _case(2, MANY, 3, False)
    st = Stage(p, bits)
    cfg = dict(w_bce=0.75, w_dice=1.25, batch=True, eps=1e-5)
    v = st.fwd(**cfg)
    dp = st.bwd()
    # written = 1 adds into what dp holds: one fp32 add of the written value
    rng = np.random.default_rng(3)
    held = rng.standard_normal(p.shape).astype(np.float32)
    acc = st.bwd(dp=_dev(held), accumulate=1)
    assert np.array_equal(acc, held + dp)
    # the upstream gradient and scale_dev scale the gradient; scale_dev the value; `before` is added to the total
    r64 = RC.region_ref(p, bits, **cfg)
    assert RC.field_error(st.bwd(g=-2.5), -2.5 * r64['grad']) <= RC.allowed_field(r64['grad'], RC.region_ref(p, bits, dtype=np.float32, **cfg)['grad'])
    vs = st.fwd(scale_dev=_t(0.5), base_total=_t(3.0), **cfg)
    assert abs(vs[0] - (3.0 + 0.5 * r64['total'])) <= 4 * np.spacing(np.float32(3.0 + 0.5 * r64['total'])) and vs[0] == vs[-1]
    assert np.array_equal(vs[1:-1], v[1:-1])                          # the terms are reported unweighted
    assert RC.field_error(st.bwd(), 0.5 * r64['grad']) <= RC.allowed_field(r64['grad'], RC.region_ref(p, bits, dtype=np.float32, **cfg)['grad'])
    # the odd shape takes the scalar kernels: the same there
    po, bo = _case(1, ODD, 3, False)
    so = Stage(po, bo)
    so.fwd(**cfg)
    d0 = so.bwd()
    ho = rng.standard_normal(po.shape).astype(np.float32)
    assert np.array_equal(so.bwd(dp=_dev(ho), accumulate=1), ho + d0)


def test_stage_through_the_chain_and_capture():
    from lintransunet_amd import losses as L, ops
    rec = L.Regions(NON_NESTED, batch=False)
    inputs = [_case(2, MANY, 3, late) for late in (False, True)]
    p0, b0 = inputs[0]
    # the chain returns the stage's report as its last entry, and the criterion names its terms
    pg = _dev(p0).requires_grad_(True)
    out = ops.level_loss_chain(pg, _dev(b0), region=(1.0, 1.0, False, 1e-5))
    assert len(out) == 7 and all(o is None for o in out[1:6]) and torch.equal(out[0], out[6][0]) and not out[6].requires_grad
    st = Stage(p0, b0)
    v = st.fwd(batch=False)
    assert np.array_equal(out[6].cpu().numpy(), v[:-1])
    out[0].backward()
    assert np.array_equal(pg.grad.cpu().numpy(), st.bwd())
    crit = L.LevelCriterion({'RegionBCELoss': 2.0, 'RegionDiceLoss': 0.5}, regions=rec)
    label = np.zeros(b0.shape, np.uint8)                             # a label with these bit-masks: 0, 1, 2, 3, 4 <-> 0, 1, 3, 2, 4
    for lab, bit in ((1, 1), (2, 3), (3, 2), (4, 4)):
        label[b0 == bit] = lab
    assert np.array_equal(RC.bits_ref(label, NON_NESTED), b0)
    total, named = crit(_dev(p0).permute(0, 4, 1, 2, 3), _dev(label).unsqueeze(1))
    r = RC.region_ref(p0, b0, 2.0, 0.5, False, 1e-5)
    assert abs(named['RegionBCELoss'].item() - 2.0 * r['bce']) <= 1e-5 * r['bce'] and abs(named['RegionDiceLoss'].item() - 0.5 * r['dice']) <= 1e-5
    assert abs(total.item() - r['total']) <= 1e-5 * r['total']
    with pytest.raises(ValueError):
        ops.level_loss_chain(pg, _dev(b0), base=('ltu_loss', (1.0, 0.0, (0.0,) * 5)), region=(1.0, 1.0, False, 1e-5))

    # captured: the replay equals the eager bytes, on an input other than the captured one
    def run(p, bits):
        total, values = ops.level_loss_region(p, bits, 0.75, 1.25, batch=True)
        total.backward()
        return total, values

    ps, bs = _dev(p0).requires_grad_(True), _dev(b0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(ps, bs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ps.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        total_s, values_s = run(ps, bs)
    for p, bits in (inputs[1], inputs[0]):
        with torch.no_grad():
            ps.copy_(_dev(p))
        bs.copy_(_dev(bits))
        graph.replay()
        torch.cuda.synchronize()
        pe = _dev(p).requires_grad_(True)
        total_e, values_e = run(pe, _dev(bits))
        torch.cuda.synchronize()
        assert torch.equal(total_s, total_e) and torch.equal(values_s, values_e) and torch.equal(ps.grad, pe.grad)


@pytest.mark.parametrize('spatial', [ODD, MANY])
def test_one_region_against_the_imbalance_stage(spatial):
    """D_0 is the Tversky term at alpha = beta = 0.5 and BCE the focal term at gamma 0 on (1 - p, p): the existing stage as a yardstick"""
    from lintransunet_amd import ops
    rng = np.random.default_rng(41)
    B = 2
    p = (rng.integers(1, 4096, (B, *spatial, 1)) / 4096.0).astype(np.float32)      # 1 - p is exact on this grid
    bits = rng.integers(0, 2, (B, *spatial)).astype(np.uint8)
    cfg = dict(w_bce=1.0, w_dice=1.0, batch=True, eps=1e-5)
    r64, r32 = RC.region_ref(p, bits, **cfg), RC.region_ref(p, bits, dtype=np.float32, **cfg)
    pg = _dev(p).requires_grad_(True)
    total, values = ops.level_loss_region(pg, _dev(bits), batch=True)
    total.backward()
    p2 = torch.cat([1.0 - _dev(p), _dev(p)], -1).requires_grad_(True)
    t2, _, v2 = ops.level_loss_imbalance(p2, _dev(bits), tversky=((1,), (1.0,), dict(alpha=0.5, beta=0.5, gamma=1.0, eps=1e-5, batch=True)),
                                         focal=(1.0, 0.0, None))
    t2.backward()
    allowed = RC.allowed_scalar(r64['total'], r32['total'])
    print(f'total: region {total.item():.9g} imbalance {t2.item():.9g} float64 {r64["total"]:.9g} allowed {allowed:.3e}')
    assert abs(total.item() - t2.item()) <= allowed and abs(total.item() - r64['total']) <= allowed
    assert abs(values[3].item() - v2[0].item()) <= RC.allowed_scalar(r64['D'][0], r32['D'][0])
    assert abs(values[1].item() - v2[1].item()) <= RC.allowed_scalar(r64['bce'], r32['bce'])
    g2 = (p2.grad[..., 1] - p2.grad[..., 0]).cpu().numpy()
    ga = RC.allowed_field(r64['grad'], r32['grad'])
    err = RC.field_error(pg.grad[..., 0].cpu().numpy(), np.asarray(g2, np.float64))
    print(f'dp: region against imbalance {err:.3e} allowed {ga:.3e}')
    assert err <= ga and RC.field_error(pg.grad.cpu().numpy(), r64['grad']) <= ga


# ---------------------------------------------------------------------------------------------- 5. labels and counts
@pytest.mark.parametrize('R,order', [(2, (7, 200)), (3, (1, 2, 3)), (8, (8, 7, 6, 5, 4, 3, 2, 1))])
def test_region_labels_both_layouts(R, order):
    from lintransunet_amd import infer, losses as L
    rng = np.random.default_rng(50 + R)
    rec = L.Regions(tuple((r + 1,) for r in range(R)), class_order=order)
    planes = (rng.integers(0, 9, (2, R, 5, 7, 3)) / 8.0).astype(np.float32)
    assert (planes == 0.5).any()
    want = RC.labels_ref(planes, order, 0.5)
    pl = _dev(planes)
    cl = pl.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)     # channels-last memory behind the [B,R,...] view
    assert not cl.is_contiguous() or R == 1
    for t in (pl, cl):
        got = infer.region_labels(t, rec)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(infer.region_labels(pl[1], rec).cpu().numpy(), want[1])      # one volume of planes, as to_native_probs returns
    assert np.array_equal(infer.region_labels(pl, rec, threshold=0.25).cpu().numpy(), RC.labels_ref(planes, order, 0.25))
    # counts, from a label map and from probabilities in both layouts
    members = tuple(tuple(range(r + 1, R + 1)) for r in range(R))
    rec2 = L.Regions(members)
    truth = rng.integers(0, R + 1, (2, 1, 5, 7, 3)).astype(np.uint8)
    pred = rng.integers(0, R + 1, (2, 1, 5, 7, 3)).astype(np.uint8)
    tb = RC.bits_ref(truth[:, 0], members)
    for predict, pb in ((_dev(pred), RC.bits_ref(pred[:, 0], members)), (pl, RC.prob_bits_ref(planes)), (cl, RC.prob_bits_ref(planes))):
        m = infer.region_metrics(predict, _dev(truth), rec2)
        TP, FP, FN, dice = RC.counts_ref(pb, tb, R)
        for key, w in (('TP', TP), ('FP', FP), ('FN', FN)):
            assert m[key].dtype == torch.int64 and m[key].shape == (2, R) and np.array_equal(m[key].cpu().numpy(), w), key
        assert m['Dice'].shape == (2, R) and np.array_equal(m['Dice'].cpu().numpy(), dice.astype(np.float32))


def test_region_metrics_empty_regions():
    from lintransunet_amd import infer, losses as L
    rec = L.Regions(((1,), (2,), (3,)))
    truth = np.zeros((1, 1, 4, 4, 4), np.uint8)
    pred = np.zeros((1, 1, 4, 4, 4), np.uint8)
    truth[0, 0, :2], pred[0, 0, 1:3] = 1, 1                           # region 0: half overlap
    pred[0, 0, 3] = 3                                                # region 2: predicted, absent from the truth; region 1: empty on both sides
    m = infer.region_metrics(_dev(pred), _dev(truth), rec)
    assert m['Dice'].cpu().tolist() == [[0.5, 1.0, 0.0]]
    assert m['TP'].cpu().tolist() == [[16, 0, 0]] and m['FP'].cpu().tolist() == [[16, 0, 16]] and m['FN'].cpu().tolist() == [[16, 0, 0]]


# ---------------------------------------------------------------------------------------------- 6. the model
EQ_SEED = 101        # chosen so that no mask voxel of the softmax model lies within 1e-5 of 0.5 (asserted below)


def _build(cfg, params, dtype=torch.float32, regions=None):
    from lintransunet_amd.model import MaskTransUnet
    model = MaskTransUnet(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, cfg.dim_input, cfg.dim_output, dropout=0.0, act_dtype=dtype,
                          regions=regions)
    model.load_state_dict(params, strict=True)
    return model.to(DEV).train()


def _is_head(key):
    return 'mask_conv_list' in key or 'final_block' in key


def test_one_region_model_equals_the_two_class_model():
    from lintransunet_amd import losses as L, train
    from tests.test_gpu_model import grads_agree, rel_err
    cfg2 = O_net.NetConfig(**SMALL)
    cfg1 = O_net.NetConfig(dim_output=1, **SMALL)
    assert any(cfg2.is_roi_list)
    soft = seedgen.seeded_params(O_net.param_shapes(cfg2), EQ_SEED)
    reg = {}
    for k, v in soft.items():
        v = v.clone()
        if 'mask_conv_list' in k:
            reg[k] = v[1:2].clone()                                  # class 1's rows are the region's ..
            v[0:1] = 0                                               # .. and class 0's logit is exactly 0: softmax(0, z)[1] = sigmoid(z)
        elif 'final_block' in k:
            reg[k] = v[4:8].clone()
            v[0:4] = 0
        else:
            reg[k] = v
        soft[k] = v
    rec = L.Regions(((1,),))
    m2, m1 = _build(cfg2, soft), _build(cfg1, reg, regions=rec)
    assert {k: tuple(v.shape) for k, v in m1.state_dict().items()} == {k: tuple(v) for k, v in O_net.param_shapes(cfg1).items()}
    x = seedgen.seeded_volume((2, 1, 32, 32, 32), EQ_SEED + 1).to(DEV)
    label = seedgen.seeded_label((2, 1, 32, 32, 32), EQ_SEED + 2).to(DEV)
    w = O_step.dynamic_weights(0)
    out2, masks2 = m2(x)
    gap = min((m[:, 1] - 0.5).abs().min().item() for m in masks2)
    print(f'closest mask voxel of the softmax model to 0.5: {gap:.3e}')
    assert gap > 1e-5
    out1, masks1 = m1(x)
    assert out1.shape == (2, 1, 32, 32, 32)
    assert len(m1.last_boxes) == len(m2.last_boxes) > 0
    for i, (a, b) in enumerate(zip(m1.last_boxes, m2.last_boxes)):
        assert torch.equal(a, b), f'box{i}'
    assert rel_err(out1[:, 0], out2[:, 1].detach().cpu().numpy()) <= 1e-3
    for i, (a, b) in enumerate(zip(masks1, masks2)):
        assert rel_err(a[:, 0], b[:, 1].detach().cpu().numpy()) <= 1e-3, f'mask{i}'
    t1, _ = train.deep_supervision_loss(out1, masks1, label, w, train.level_specs(5, ('RegionBCELoss', 'RegionDiceLoss'), [1, 1]), regions=rec)
    t2, _ = train.deep_supervision_loss(out2, masks2, label, w, train.level_specs(5, ('FocalCELoss', 'TverskyLoss'), [1, 1]),
                                        imbalance=L.Imbalance(0.5, 0.5, 1.0, batch=True, eps=1e-5, focal_gamma=0))
    for lvl, (a, b) in enumerate(zip(t1, t2)):
        assert abs(a.item() - b.item()) <= 1e-4 * max(1.0, abs(b.item())), (lvl, a.item(), b.item())
    torch.autograd.backward(t1, [torch.ones_like(t) for t in t1])
    torch.autograd.backward(t2, [torch.ones_like(t) for t in t2])
    torch.cuda.synchronize()
    p1, p2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    checked = 0
    for k, p in p2.items():
        if p.grad is None:
            assert p1[k].grad is None, k
            continue
        g2 = p.grad[1:2] if 'mask_conv_list' in k else p.grad[4:8] if 'final_block' in k else p.grad
        assert grads_agree(p1[k].grad, g2, k), k
        checked += 1
    assert checked > 100


def _brats_model(dtype=torch.float32, seed=300, full=False):
    from lintransunet_amd import losses as L
    cfg = O_net.NetConfig(dim_output=3, **({} if full else SMALL))
    return _build(cfg, seedgen.seeded_params(O_net.param_shapes(cfg), seed), dtype, regions=L.Regions.brats()), cfg


def test_region_model_state_dict_is_the_class_models():
    cfg = O_net.NetConfig(dim_output=3, **SMALL)
    params = seedgen.seeded_params(O_net.param_shapes(cfg), 300)
    region, _ = _brats_model()
    plain = _build(cfg, params)
    a, b = region.state_dict(), plain.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
    assert region.regions.members == ((1, 2, 3), (2, 3), (3,)) and plain.regions is None


def test_region_model_steps():
    from lintransunet_amd import data, train
    from tests.test_gpu_model import grads_agree
    x, label = data.synthetic_patches(2, (32, 32, 32), 7, DEV, n_classes=4)
    assert set(label.unique().tolist()) == {0, 1, 2, 3}
    w = O_step.dynamic_weights(0)

    def run(dtype=torch.float32, **cfgkw):
        torch.manual_seed(99)
        m, _ = _brats_model(dtype, **cfgkw)
        totals, named = train.train_step(m, x, label, w)
        torch.cuda.synchronize()
        return m, [t.item() for t in totals], named, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    # twice from the same state: the same bits - in the setting tests/test_gpu_model.py::test_step_is_reproducible holds the class
    # model to (bf16 storage, the reference's channels: the fp32 InstanceNorm sums are atomics and move the last bits) - and the
    # bf16-storage run finishes with finite losses and gradients
    _, lb, _, gb = run(torch.bfloat16, full=True)
    assert all(np.isfinite(lb)) and all(torch.isfinite(g).all() for g in gb.values())
    _, lb1, _, gb1 = run(torch.bfloat16, full=True)
    assert lb1 == lb and all(torch.equal(gb1[k], gb[k]) for k in gb)
    m, l0, named, g0 = run()
    assert all(np.isfinite(l0)) and all(set(n) == {'RegionBCELoss', 'RegionDiceLoss'} for n in named)
    with pytest.raises(ValueError):
        train.train_step(m, x, label, w, specs=train.level_specs(5))      # class names on a region model: before any launch
    # captured
    torch.manual_seed(99)
    mg, _ = _brats_model()
    red = train.GradReducer(mg, bucket_mb=0.5, unused=train.UNUSED_PARAMETERS)
    step = train.GraphedStep(mg, x, label, w, red)
    for _ in range(2):
        totals, _ = step(x, label)
    torch.cuda.synchronize()
    pm = dict(mg.named_parameters())
    for k, g in g0.items():
        assert grads_agree(pm[k].grad, g, k), k
    assert np.allclose([t.item() for t in totals], l0, rtol=1e-4, atol=1e-6)
    # eval: the indicator of the probabilities
    m.eval()
    with torch.no_grad():
        pr = m(x, probs=True)
        ind = m(x)
    assert pr.shape == ind.shape == (2, 3, 32, 32, 32) and pr.dtype == ind.dtype == torch.float32
    assert 0.0 <= pr.min().item() and pr.max().item() <= 1.0 and torch.equal(ind, (pr > 0.5).float())


def test_infer_volume_and_region_labels():
    from lintransunet_amd import infer
    m, _ = _brats_model()
    x = seedgen.seeded_volume((1, 1, 32, 32, 48), 61).to(DEV)        # two windows of depth 32
    p = infer.infer_volume(m, x, depth_size=32, roi_xy=32, sw_batch_size=2, overlap=0.5, probs=True)
    assert p.shape == (1, 3, 32, 32, 48) and m.training
    got = infer.region_labels(p, m.regions)
    want = RC.labels_ref(p.cpu().numpy(), m.regions.class_order, 0.5)
    assert got.shape == (1, 32, 32, 48) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(infer.region_labels(p.contiguous(), m.regions).cpu().numpy(), want)
    print('labels painted:', np.bincount(want.ravel(), minlength=4).tolist())
