"""Parameter-side kernels on views packed inside flat buckets, on the GPU (the table, helpers and references: bucket_common.py).

1. Weight-gradient destinations at every residue: each case of bucket_common.CASES packs its destinations (weight, then its bias /
   gamma / beta directly behind it) into one guarded buffer and runs the production path with `p._ltu_grad` set to the packed
   views (the entry points the sibling tables drive through the C-ABI are driven the same way, with the packed pointers), at
   residues 0, 1, 2, 3 with the same operands and the same old values.  Per residue: the named kernels ran, both guard bands are
   bit-identical; residues 1..3 are bit-equal to residue 0 (rule 'bits') or, for the fp32-atomics cases (rule 'sum'), within the
   float64 bound like residue 0; `view - old` at residue 0 agrees with float64: weight-like gradients max|err| / max|ref| <= 1e-4,
   biases / gamma / beta / the gate's psi bias |err| <= 1e-5 of their summed magnitudes (plus the siblings' named slack where a
   sum runs over values the kernel rounded to bf16 without storing them).
2. Readers of re-homed master weights: ltu_weight_prep / ltu_weight_prep_chunks for every record kind, ltu_cast_f32,
   ltu_transpose_f32 and ltu_pack_conv_weight with the SOURCE at residues 0..3: bit-equal to the numpy restatement.
3. Optimizer tails: ltu_adamw, ltu_grad_sumsq, ltu_adamw_guarded on guarded buffers whose length is no multiple of 4.
4. The real model (benchmark channels, 3 classes, bf16, 2 x 64 x 64 x 32): gradients with no reducer, with the reducer in
   registration order, after rebucket(), and with the weights re-homed by FusedAdamW.

LTU_BUCKET_VIEWS_REPORT=<file> appends one JSON line per GPU case: kernels launched, residues, worst error / bound, the census.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import bucket_common as BC
from tests import stream_common as R
from tests import test_gpu_conv_paths as CP
from tests import test_gpu_stream_paths as SP
from tests import test_gpu_token_paths as TP
from tests.test_gpu_conv_paths import knobs, launched
from tests.test_gpu_token_paths import _call, _ptr, _stream

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _report(line):
    path = os.environ.get('LTU_BUCKET_VIEWS_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(line) + '\n')


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available()
    from lintransunet_amd import ops  # noqa: F401
    return True


# ---------------------------------------------------------------------------------------------- part 1: runners

class Ref:
    """expected `view - old` of one destination: kind 'w' (weight-like: WGRAD_TOL of the max), 's' (a sum: SUM_REL of the summed
    magnitudes `mag`, + `extra`), 'same' (must keep its old bits)"""

    def __init__(self, kind, ref=None, mag=None, extra=None):
        self.kind, self.ref, self.mag, self.extra = kind, ref, mag, extra


def _param(t):
    return t.float().to(DEV).contiguous().requires_grad_(True)


def _home(params, pack):
    """what train.GradReducer._assign does to a parameter, with the packed views (no hook: nothing counts arrivals here)"""
    assert len(params) == len(pack.views)
    for p, v in zip(params, pack.views):
        assert p.numel() == v.numel()
        p._ltu_grad = v.view_as(p)


def _seed(case):
    return sum(map(ord, case.sib.name if case.sib is not None else case.name))


def _cp_case(case):
    return CP.Case('bucket_' + case.name, case.op, case.shape, {})


def run_conv(case, pack):
    from lintransunet_amd import ops
    r, s = CP.reference(_cp_case(case)), case.shape
    vox = (0, 2, 3, 4)
    with ops.use(ops.Context()):
        if case.op == 'conv3d':
            cop = s['cop']
            x0 = CP._cl(r['x0'])
            x1 = CP._cl(r['x1']) if r['x1'] is not None else None
            p = [_param(r['w']), _param(r['b'])]
            _home(p, pack)
            y = ops.conv3d(x0, p[0], p[1], stride=s['stride'], x1=x1, cop=cop)
            go = CP._cl(r['go'])
            if cop:
                pad = torch.zeros(y.shape, device=DEV, dtype=torch.bfloat16)
                pad[..., :s['Co']] = go
                go = pad
            _, seen = launched(lambda: (y.backward(go), ops.flush_deferred()))
            refs = [Ref('w', r['dw'][0]), Ref('s', r['db'][0], r['go'].abs().sum(vox))]
        elif case.op == 'pair':
            n1, Cb = s['n1'], s['Cb']
            x = CP._cl(r['x'])
            p = [_param(r[k]) for k in ('wa', 'ba', 'wb', 'bb')]
            _home(p, pack)
            prep = ops.conv_pair_prep(*(t.detach() for t in p), n1, torch.bfloat16)
            y0, y1 = ops.conv3d_pair(x, *p, prep)
            g1 = torch.zeros(y1.shape, device=DEV, dtype=torch.bfloat16)
            g1[..., :Cb] = CP._cl(r['gb'])
            ga = CP._cl(r['ga'])
            _, seen = launched(lambda: (torch.autograd.backward([y0, y1], [ga, g1]), ops.flush_deferred()))
            refs = [Ref('w', r['dw'][0]), Ref('s', r['db'][0], r['ga'].abs().sum(vox)),
                    Ref('w', r['dw'][1]), Ref('s', r['db'][1], r['gb'].abs().sum(vox))]
        else:
            x = CP._cl(r['x'])
            p = [_param(r['w']), _param(r['b'])]
            _home(p, pack)
            prep = ops.upconv_prep(p[0].detach(), torch.bfloat16)
            y = ops.upconv3d(x, p[0], p[1], prep)
            go = CP._cl(r['go'])
            _, seen = launched(lambda: (y.backward(go), ops.flush_deferred()))
            refs = [Ref('w', r['dw'][0]), Ref('s', r['db'][0], r['go'].abs().sum(vox))]
    assert all(t.grad is None for t in p), 'a fused parameter got an autograd gradient'
    return seen, refs


class _Named:
    def __init__(self, name):
        self.name = name


def run_linear(case, pack):
    from lintransunet_amd import ops
    s = case.shape
    M, K, N, nw = s['M'], s['K'], s['N'], s['nw']
    g, W, b = TP._linear_operands(_Named(case.sib.name if case.sib is not None else case.name), nw, N, K)
    x, go = TP._bf(torch.randn(M, K, generator=g)), TP._bf(torch.randn(M, N, generator=g))
    wp, bp = [_param(w) for w in W], [_param(v) for v in b]
    _home([t for pair in zip(wp, bp) for t in pair], pack)
    with ops.use(ops.Context()):
        y = ops.linear(TP._dev(x), wp, bp)
        gg = TP._dev(go)
        _, seen = launched(lambda: (y.backward(gg), ops.flush_deferred()))
    assert all(t.grad is None for t in wp + bp)
    return seen, [x_ for dw, db, mag in BC.linear_wgrad_ref(go, x, nw) for x_ in (Ref('w', dw), Ref('s', db, mag))]


def fat_kernels():
    """what the fat-tile case must launch: the fat kernel where it is compiled in, else the grouped ring and its fold"""
    from lintransunet_amd import _lib
    return [BC.FAT] if _lib.experiments() else [TP.WG, TP.FOLD]


def run_wgrad(case, pack):
    """TP.run_wgrad with the destinations of the layer's four projections packed back to back"""
    from lintransunet_amd import _lib, ops
    s = case.shape
    M, d = s['M'], s['d']
    g = TP._gen(_seed(case))
    jobs, refs, views = [], [], iter(pack.views)
    for N, K, nw in TP._wgrad_jobs(d):
        go, x = TP._bf(torch.randn(M, N, generator=g)), TP._bf(torch.randn(M, K, generator=g))
        dws, dbs = [], []
        for i in range(nw):
            dws.append(next(views).view(N // nw, K))
            dbs.append(next(views))
        jobs.append((TP._dev(go), TP._dev(x), dws, dbs, M, N, K))
        refs += [x_ for dw, db, mag in BC.linear_wgrad_ref(go, x, nw) for x_ in (Ref('w', dw), Ref('s', db, mag))]
    keep = []
    if s['mode'] == 'group':
        _, seen = launched(lambda: ops.Context()._wgrad_group_launch(jobs, keep))
    else:
        arr = (_lib.ReduceJob * len(jobs))()

        def run():
            for j, (go, x, dws, dbs, M_, N, K) in zip(arr, jobs):
                ws = torch.empty(_lib.load().ltu_wgrad_ws_floats(M_, N, K), device=DEV, dtype=torch.float32)
                keep.append(ws)
                _call('ltu_linear_wgrad', _ptr(go), N, _ptr(x), K, ops._ptr_array(dws), ops._ptr_array(dbs), len(dws), M_, N, K, _ptr(ws),
                      ws.numel(), ctypes.addressof(j), ops.BF16, _stream())
                assert j.part, 'the ring declined the deferred weight gradient'
            _call('ltu_reduce_batch', ctypes.addressof(arr), len(jobs), _stream())
        _, seen = launched(run)
    return seen, refs


def run_ln(case, pack):
    from lintransunet_amd import ops
    s = case.shape
    M, d, p = s['M'], s['d'], s['p']
    g = TP._gen(_seed(case))
    x, r = TP._bf(torch.randn(M, d, generator=g)), TP._bf(torch.randn(M, d, generator=g))
    x = TP._bf(x + 2.0 * (torch.arange(M) < M // 5).double()[:, None])
    gamma, beta = TP._f32(1 + 0.2 * torch.randn(d, generator=g)), TP._f32(0.1 * torch.randn(d, generator=g))
    gy = [TP._bf(torch.randn(M, d, generator=g)) for _ in range(2 if s['dy2'] else 1)]
    gp, bp = _param(gamma), _param(beta)
    _home([gp, bp], pack)
    seed = 2000 + _seed(case)
    with ops.use(ops.Context()):
        y = ops.res_layernorm(TP._dev(x), TP._dev(r), gp, bp, TP.LN_EPS, p, seed, fork=s['dy2'])
        ys = y if s['dy2'] else (y,)
        z, stat = (t.double().cpu() for t in ys[0].grad_fn.saved_tensors)
        gg = [TP._dev(t) for t in gy]
        _, seen = launched(lambda: (torch.autograd.backward(list(ys), gg), ops.flush_deferred()))
    assert gp.grad is None and bp.grad is None
    dg, db, mg, mb = BC.ln_param_ref(sum(gy), z, stat[:, :1], stat[:, 1:])
    return seen, [Ref('s', dg, mg), Ref('s', db, mb)]


TAIL_ORDER = ('wo', 'bo', 'w1', 'b1', 'w2', 'b2', 'g1', 'be1', 'g2', 'be2')


def run_tail(case, pack):
    """ops.layer_tail forward and backward with all ten parameters of the layer's post-attention half homed in the packed buffer.
    The references are per stage, from the bf16 tensors the chain kernels stored: the forward's saved tensors, and the data
    gradients of a second, stand-alone ltu_layer_tail_bwd call on them (the kernel is deterministic: the same values the autograd
    call fed to the weight-gradient kernels)"""
    from lintransunet_amd import ops
    from lintransunet_amd.model import _WeightStore
    s = case.shape
    B, N, d, p = s['B'], s['N'], s['d'], s['p']
    M = B * N
    seed0 = _seed(case)
    P = TP._tail_params(d, seed0, False)
    g = TP._gen(seed0 + 1)
    x = TP._bf(torch.randn(M, d, generator=g))
    x = TP._bf(x + 1.5 * (torch.arange(M) < M // 7).double()[:, None])
    a_in = TP._bf(torch.randn(M, d, generator=g))
    qkv_in = TP._bf(torch.randn(M, 3 * d, generator=g) * 1.5)
    dy = TP._bf(torch.randn(M, d, generator=g))
    dy2 = TP._bf(torch.randn(M, d, generator=g)) if s['dy2'] else None
    seeds = (11 + seed0, 22, 33)
    par = {k: _param(P[k]) for k in TAIL_ORDER}
    _home([par[k] for k in TAIL_ORDER], pack)
    st = _WeightStore(torch.device(DEV, torch.cuda.current_device()), torch.bfloat16)
    for k in ('wo', 'w1', 'w2'):
        st.add_linear(k, [par[k]], frag=True)
    st.finalize()
    st.refresh()
    po, p1, p2 = (st.lin[k] for k in ('wo', 'w1', 'w2'))
    assert po.fragT is not None and p1.fragT is not None and p2.fragT is not None
    gys = [TP._dev(dy)] + ([TP._dev(dy2)] if dy2 is not None else [])
    with ops.use(ops.Context()):
        a = TP._dev(qkv_in) if s['attn'] else TP._dev(a_in)
        out = ops.layer_tail(a, TP._dev(x), tuple(par[k] for k in TAIL_ORDER), (po, p1, p2), TP.LN_EPS, p, seeds, s['dy2'],
                             attn=(B, N) if s['attn'] else None)
        ys = out if s['dy2'] else (out,)
        a_s, z1, stat1, t1, u, h, z2, stat2 = ys[0].grad_fn.saved_tensors[:8]
        _, seen = launched(lambda: (torch.autograd.backward(list(ys), gys), ops.flush_deferred()))
    assert all(par[k].grad is None for k in TAIL_ORDER)
    # the data gradients the weight-gradient kernels read, once more
    dr2, dr1, dz1, da = (torch.empty_like(a_s) for _ in range(4))
    du = torch.empty_like(u)
    nblk = ops._lib.load().ltu_layer_tail_blocks(M)
    lnws = torch.empty((2, nblk, 2 * d), device=DEV, dtype=torch.float32)
    _call('ltu_layer_tail_bwd', _ptr(gys[0]), _ptr(gys[1] if len(gys) > 1 else None), _ptr(z2), _ptr(z1), _ptr(u), _ptr(stat2), _ptr(stat1),
          _ptr(par['g2']), _ptr(par['g1']), _ptr(p2.fragT), _ptr(p1.fragT), _ptr(po.fragT), _ptr(dr2), _ptr(du), _ptr(dr1), _ptr(dz1), _ptr(da),
          _ptr(lnws[0]), _ptr(lnws[1]), lnws[0].numel(), M, d, float(p), seeds[0], seeds[1], seeds[2], 0, 1, ops.BF16, _stream())
    torch.cuda.synchronize()
    G = lambda t: t.double().cpu()                                   # noqa: E731
    DR2, DU, DR1 = G(dr2), G(du), G(dr1)
    (dwo, dbo, mo), = BC.linear_wgrad_ref(DR1, G(a_s), 1)
    (dw1, db1, m1), = BC.linear_wgrad_ref(DU, G(t1), 1)
    (dw2, db2, m2), = BC.linear_wgrad_ref(DR2, G(h), 1)
    gy = dy + (dy2 if dy2 is not None else 0)
    Z2, S2, Z1, S1 = G(z2), G(stat2), G(z1), G(stat1)
    dg2, dbe2, mg2, mb2 = BC.ln_param_ref(gy, Z2, S2[:, :1], S2[:, 1:])
    # LayerNorm 1 sums dt1 + dz2, both rounded to bf16 in LDS and not stored (tlayer.hip; TP.run_tail restates them with their slack:
    # one bf16 ulp where the fp32 value may round the other way), carried into the column sums
    zn2 = (Z2 - S2[:, :1]) * S2[:, 1:]
    dz2 = TP._ln_bwd(gy, zn2, S2[:, 1:], P['g2'])
    gg2 = gy * P['g2']
    dz2mag = S2[:, 1:] * (gg2.abs() + gg2.mean(1, keepdim=True).abs() + zn2.abs() * (gg2 * zn2).mean(1, keepdim=True).abs())
    dz2b, dz2sl = TP.rounded(dz2, dz2mag)
    dt1, dtmag = TP._proj_ref(DU, P['w1'].T, torch.zeros(1, dtype=torch.float64))
    dtb, dtsl = TP.rounded(dt1, dtmag)
    gsum, sl = dtb + dz2b, dtsl + dz2sl
    zn1 = (Z1 - S1[:, :1]) * S1[:, 1:]
    dg1, dbe1, mg1, mb1 = BC.ln_param_ref(gsum, Z1, S1[:, :1], S1[:, 1:])
    refs = [Ref('w', dwo), Ref('s', dbo, mo), Ref('w', dw1), Ref('s', db1, m1), Ref('w', dw2), Ref('s', db2, m2),
            Ref('s', dg1, mg1, (sl * zn1.abs()).sum(0)), Ref('s', dbe1, mb1, sl.sum(0)), Ref('s', dg2, mg2), Ref('s', dbe2, mb2)]
    return seen, refs


def run_dw(case, pack):
    """SP.run_dw's calls with the weight and bias gradients packed (C * 27 floats, then C)"""
    from lintransunet_amd import _lib, ops
    s = case.shape
    B, H, W, D, C, p = s['B'], s['H'], s['W'], s['D'], s['C'], s['p']
    n = B * H * W * D * C
    g = TP._gen(_seed(case))
    x = TP._bf(torch.randn(B, H, W, D, C, generator=g))
    w, b = TP._f32(0.3 * torch.randn(C, 1, 3, 3, 3, generator=g)), TP._f32(torch.randn(C, generator=g))
    gs = [TP._bf(torch.randn(B, H, W, D, C, generator=g)) for _ in range(s['ports'])]
    seed = 3000 + _seed(case)
    xg, wg, bg = TP._dev(x), TP._dev(w, torch.float32), TP._dev(b, torch.float32)
    y, dx = TP._nan((n,)), TP._nan((n,))
    _call('ltu_dwconv_fwd', _ptr(xg), _ptr(wg), _ptr(bg), _ptr(y), B, H, W, D, C, float(p), seed, 0, ops.BF16, _stream())
    torch.cuda.synchronize()
    Y = y.double().cpu().reshape(B, H, W, D, C)
    keep = float(np.float32(1) / (np.float32(1) - np.float32(p)))
    mask = torch.where((Y == 0).all(1).all(1).all(1), 0.0, keep).double()
    gsum = gs[0] if len(gs) == 1 else (gs[0].float() + gs[1].float()).bfloat16().double()
    gg = [TP._dev(t) for t in gs] + [None]
    dwt, db = pack.views
    nws = _lib.load().ltu_dwconv_bwd_ws_floats(B, H, W, D, C, ops.BF16)
    ws = torch.empty(nws, device=DEV, dtype=torch.float32) if s['ws'] else None
    _, seen = launched(lambda: _call('ltu_dwconv_bwd', _ptr(gg[0]), _ptr(gg[1]), _ptr(xg), _ptr(wg), _ptr(dx), _ptr(dwt), _ptr(db), _ptr(ws),
                                     nws if s['ws'] else 0, B, H, W, D, C, float(p), seed, 0, ops.BF16, _stream()))
    _, dw_ref, db_ref = R.dw_bwd(gsum, x, w, mask)
    mag = (gsum.abs() * mask[:, None, None, None, :]).sum((0, 1, 2, 3))
    return seen, [Ref('w', dw_ref), Ref('s', db_ref, mag)]


def run_gate(case, pack):
    """SP.run_gate's calls with psi's weight gradient (C floats), its one-float bias gradient and a neighbour view packed"""
    from lintransunet_amd import _lib, ops
    s = case.shape
    B, S, C = s['B'], s['S'], s['C']
    M, n = B * S, B * S * C
    u1, u2, skip, dout, pw, pb = SP.gate_operands(case.sib)
    u1g, u2g, skg = TP._dev(u1), TP._dev(u2), TP._dev(skip)
    pwg, pbg = TP._dev(pw, torch.float32), TP._dev(pb, torch.float32)
    nws = _lib.load().ltu_norm_ws_floats()
    ws = torch.empty(nws, device=DEV, dtype=torch.float32)
    st1, st2 = SP._zeros((B, C, 3)), SP._zeros((B, C, 3))
    _call('ltu_instnorm_stats', _ptr(u1g), _ptr(st1), _ptr(ws), nws, B, S, C, ops.BF16, _stream())
    _call('ltu_instnorm_stats', _ptr(u2g), _ptr(st2), _ptr(ws), nws, B, S, C, ops.BF16, _stream())
    a, out = TP._nan((M,), torch.float32), TP._nan((n,))
    _call('ltu_gate_fwd', _ptr(u1g), _ptr(u2g), _ptr(st1), _ptr(st2), _ptr(pwg), _ptr(pbg), _ptr(skg), _ptr(a), _ptr(out), B, S, C, ops.BF16,
          _stream())
    dskip, du1, du2 = (TP._nan((n,)) for _ in range(3))
    ds = TP._nan((M,), torch.float32)
    bs1, bs2 = SP._zeros((B, C, 2)), SP._zeros((B, C, 2))
    dpw, dpb, _neighbour = pack.views
    gg = TP._dev(dout)
    wsb = ws if s['ws'] else None
    _, seen = launched(lambda: _call('ltu_gate_bwd', _ptr(gg), _ptr(u1g), _ptr(u2g), _ptr(st1), _ptr(st2), _ptr(pwg), _ptr(skg), _ptr(a),
                                     _ptr(dskip), _ptr(ds), _ptr(dpw), _ptr(dpb), _ptr(bs1), _ptr(bs2), _ptr(wsb), nws if s['ws'] else 0,
                                     _ptr(du1), _ptr(du2), B, S, C, ops.BF16, _stream()))
    torch.cuda.synchronize()
    G1, G2 = st1.double().cpu(), st2.double().cpu()
    m1, r1 = R.in_stat2(G1[..., 0], G1[..., 1], G1[..., 2], S)
    m2, r2 = R.in_stat2(G2[..., 0], G2[..., 1], G2[..., 2], S)
    h1, h2 = R.in_hat(u1, m1, r1), R.in_hat(u2, m2, r2)
    DS = ds.double().cpu().reshape(B, S)                              # the sums are formed from the kernel's own ds (SP.run_gate)
    dpw_ref, dpb_ref, _, _ = R.gate_sums(DS, h1, h2, pw)
    return seen, [Ref('w', dpw_ref), Ref('s', dpb_ref.reshape(1), DS.abs().sum().reshape(1)), Ref('same')]


RUNNERS = {'conv3d': run_conv, 'pair': run_conv, 'upconv': run_conv, 'linear': run_linear, 'wgrad': run_wgrad, 'ln': run_ln,
           'tail': run_tail, 'dw': run_dw, 'gate': run_gate}


def check_dest(label, got, old, ref):
    """worst error / bound of one destination's `view - old` (got, old: fp32 cpu), and a failure text or None"""
    if ref.kind == 'same':
        ok = BC.bit_equal(got, old)
        return (0.0 if ok else math.inf), (None if ok else f'{label}: a view no kernel owns was written')
    if not torch.isfinite(got).all():
        return math.inf, f'{label}: non-finite values'
    delta = got.double() - old.double()
    want = ref.ref.reshape(-1)
    if ref.kind == 'w':
        err = (delta - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
        return err / BC.WGRAD_TOL, (f'{label}: max|err| / max|ref| = {err:.3g} > {BC.WGRAD_TOL}' if err > BC.WGRAD_TOL else None)
    bound = BC.SUM_REL * ref.mag.reshape(-1) + (ref.extra.reshape(-1) if ref.extra is not None else 0)
    ratio = (delta - want).abs() / bound.clamp_min(1e-30)
    worst = ratio.max().item()
    i = int(ratio.argmax())
    return worst, (f'{label}: element {i}: got {delta[i].item():.8g}, ref {want[i].item():.8g}, {worst:.2f} x the bound' if worst > 1 else None)


def run_case(case):
    """every residue of one case; returns the report line (fails: every assertion that did not hold)"""
    labels = [lab for lab, _ in BC.dest_sizes(case)]
    sizes = [n for _, n in BC.dest_sizes(case)]
    old = BC.olds(case)
    want = fat_kernels() if case.name == 'wgroup_fat' else None
    line = {'case': case.name, 'entry': case.entry, 'rule': case.rule, 'knobs': case.knobs, 'residues': {}, 'ratio': {}, 'fails': []}
    fails, first = line['fails'], None
    with knobs(case.knobs):
        for res in BC.RESIDUES:
            pack = BC.Packed(sizes, res, old)
            seen, refs = RUNNERS[case.op](case, pack)
            torch.cuda.synchronize()
            names = want or case.names(res)
            miss = [k for k in names if k not in seen] + [f'{k} ran (must not)' for k in seen if any(k.startswith(a) for a in case.absent)]
            guards = pack.guard_fails()
            views = [v.detach().cpu().clone() for v in pack.views]
            changed = not BC.bit_equal(pack.body.cpu(), torch.cat(old))
            line['residues'][res] = {'starts': pack.starts(), 'kernels': sorted(seen), 'missing': miss, 'guards': guards}
            fails += [f'residue {res}: expected kernels did not run: {miss}; launched {sorted(seen)}'] if miss else []
            fails += [f'residue {res}: {g}' for g in guards]
            if not changed:
                fails.append(f'residue {res}: no destination changed')
            if res == 0:
                first = views
            elif case.rule == 'bits':
                diff = [lab for lab, a, b in zip(labels, views, first) if not BC.bit_equal(a, b)]
                line['residues'][res]['bit_equal'] = not diff
                if diff:
                    fails.append(f'residue {res}: differs in bits from residue 0: {diff}')
            if res == 0 or case.rule == 'sum':
                for lab, v, o, ref in zip(labels, views, old, refs):
                    worst, msg = check_dest(lab, v, o, ref)
                    line['ratio'][lab] = max(line['ratio'].get(lab, 0.0), worst)
                    if msg:
                        fails.append(f'residue {res}: {msg}')
    return line


@pytest.mark.parametrize('case', BC.CASES, ids=[c.name for c in BC.CASES])
def test_packed_destinations(gpu, case):
    line = run_case(case)
    _report({'part': 1, **line})
    worst = max(line['ratio'].items(), key=lambda kv: kv[1]) if line['ratio'] else None
    print(f'[bucket views {case.name}] rule {case.rule}, worst error / bound {worst}')
    assert not line['fails'], f'{case.name}:\n  ' + '\n  '.join(line['fails'])


# ---------------------------------------------------------------------------------------------- part 2: readers of master weights

def _sources():
    """the fp32 masters the weight-prep records read, seeded; values of every magnitude a weight takes, none of them bf16-exact"""
    g = np.random.default_rng(77)
    mk = lambda *shape: (g.standard_normal(shape) * np.exp(g.uniform(-6, 2, shape))).astype(np.float32)      # noqa: E731
    return {'w128': mk(128, 128), 'w96x40': mk(96, 40), 'w96x64': mk(96, 64), 'conv5x12': mk(5, 12, 27), 'bias3': mk(3),
            'up32x64': mk(32, 64, 27), 'pa': mk(8, 16, 27), 'pb': mk(3, 16, 27), 'ba': mk(8), 'bb': mk(3)}


PAIR_N1 = 16


def _wprep_plan(f32):
    """(records, destinations): records (src name, dst name, dst element offset, kind, R, C, p0, p1, pad); destinations name ->
    (elements, always fp32).  Every kind the store emits for the output dtype: in fp32 mode it emits neither the bf16 copies
    (kind 0) nor the fragment orders (8, 9).  Shapes: the dense kinds at 128 x 128 (four chunks, the 16-byte path) and 96 x 40
    (n % 8 == 0 and R % 8 == 0: the 16-byte path with C % 4 == 0 ... and a transpose with p1 % 8 != 0: refused); the fragment
    orders at 128 x 128 and 96 x 64 (model._WeightStore.add_linear emits them for multiples of 32 only, and their index map reads
    past a source that is none); conv packs with Co 5 -> 8, Ci 12 -> 16; a padded bias 3 -> 8; sub-pixel operands at 32 x 64; a conv
    pair through ops.pair_records"""
    recs, dst = [], {}

    def add(src, name, n, kind, R, C, p0=0, p1=0, pad=0, always32=False):
        dst[name] = (n, always32)
        recs.append((src, name, 0, kind, R, C, p0, p1, pad))
    for src, R_, C_ in (('w128', 128, 128), ('w96x40', 96, 40)):
        if not f32:
            add(src, f'{src}.cast', R_ * C_, 0, R_, C_)
        add(src, f'{src}.t', C_ * R_, 1, R_, C_, R_, 0)
    add('w96x40', 'w96x40.t_off', 40 * 200, 1, 96, 40, 200, 4)
    add('w96x40', 'w96x40.t_ld', 40 * 104, 1, 96, 40, 104, 8)
    if not f32:
        for src, R_, C_ in (('w128', 128, 128), ('w96x64', 96, 64)):
            add(src, f'{src}.frag', R_ * C_, 8, R_, C_)
            add(src, f'{src}.fragT', R_ * C_, 9, R_, C_)
    add('conv5x12', 'conv.wf', 8 * 27 * 16, 2, 5, 12, 8, 16)
    add('conv5x12', 'conv.wd', 16 * 27 * 8, 3, 5, 12, 8, 16)
    add('bias3', 'conv.bias', 8, 4, 1, 3, always32=True)
    add('up32x64', 'up.wf', 64 * 32 * 64, 5, 32, 64, 32, 64)
    add('up32x64', 'up.wd', 64 * 32 * 64, 6, 32, 64, 32, 64)
    n0, n1, Ci = 8, PAIR_N1, 16
    dst['pair.wf'], dst['pair.wd'], dst['pair.bias'] = ((n0 + n1) * 27 * Ci, False), (Ci * 27 * (n0 + n1), False), (n0 + n1, True)
    return recs, dst


def _pair_records(srcs, dsts, esz):
    """ops.pair_records on the packed sources, as (src name, dst name, dst element offset, kind, ...) records"""
    from lintransunet_amd import ops
    wa, ba, wb, bb = (srcs[k].views[0] for k in ('pa', 'ba', 'pb', 'bb'))
    rows = ops.pair_records(wa.view(8, 16, 3, 3, 3), ba, wb.view(3, 16, 3, 3, 3), bb, PAIR_N1, dsts['pair.wf'], dsts['pair.wd'], dsts['pair.bias'])
    by_src = {srcs[k].views[0].data_ptr(): k for k in ('pa', 'ba', 'pb', 'bb')}
    out = []
    for src, dptr, kind, R_, C_, p0, p1, pad in rows:
        name = next(k for k in ('pair.wf', 'pair.wd', 'pair.bias') if dsts[k].data_ptr() <= dptr < dsts[k].data_ptr() + dsts[k].numel() * dsts[k].element_size())
        off = (dptr - dsts[name].data_ptr()) // (4 if name == 'pair.bias' else esz)
        out.append((by_src[src], name, off, kind, R_, C_, p0, p1, pad))
    return out


WPREP_MODES = {'table': ({}, 'weight_prep_kernel<{T}>'), 'chunks': ({}, 'weight_prep_chunk_kernel<{T}, 1>'),
               'chunks_nc4': ({'LTU_WPREP_NC4_MIN': 1}, 'weight_prep_chunk_kernel<{T}, 4>'),
               'chunks_narrow': ({'LTU_WPREP_BLOCKS': 3}, 'weight_prep_chunk_kernel<{T}, 1>')}


@pytest.mark.parametrize('f32', [False, True], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('mode', list(WPREP_MODES))
def test_weight_prep_reads_packed_masters(gpu, mode, f32):
    """every record kind with its SOURCE at residues 0..3 of a guarded buffer, into NaN-filled destinations: what the record owns is
    bit-equal to the numpy restatement (rounded to bf16 nearest-even), nothing else is written, the sources and their guards keep
    their bits"""
    from lintransunet_amd import ops
    src_np = _sources()
    plan, dst_plan = _wprep_plan(f32)
    odt, esz = (torch.float32, 4) if f32 else (torch.bfloat16, 2)
    kn, kernel = WPREP_MODES[mode]
    kernel = kernel.format(T='float' if f32 else 'bf16_t')
    report = {'part': 2, 'case': f'weight_prep/{mode}/{"fp32" if f32 else "bf16"}', 'residues': {}}
    for res in BC.RESIDUES:
        srcs = {k: BC.Packed([v.size], res, [torch.from_numpy(v)]) for k, v in src_np.items()}
        dsts = {k: torch.full((n,), float('nan'), device=DEV, dtype=torch.float32 if a32 else odt) for k, (n, a32) in dst_plan.items()}
        recs = plan + _pair_records(srcs, dsts, esz)
        rows = np.zeros(len(recs), dtype=ops.WPREP_DTYPE)
        for i, (s, dname, off, kind, R_, C_, p0, p1, pad) in enumerate(recs):
            rows[i] = (srcs[s].views[0].data_ptr(), dsts[dname].data_ptr() + off * dsts[dname].element_size(), kind, R_, C_, p0, p1, pad)
        table = torch.from_numpy(rows.view(np.uint8).copy()).to(DEV)
        chunks = torch.tensor(BC.chunk_list([r[3:] for r in recs]), dtype=torch.int32).reshape(-1, 2).to(DEV)
        assert chunks.shape[0] > len(recs)

        def run():
            if mode == 'table':
                _call('ltu_weight_prep', table.data_ptr(), len(recs), ops.F32 if f32 else ops.BF16, _stream())
            else:
                _call('ltu_weight_prep_chunks', table.data_ptr(), chunks.data_ptr(), chunks.shape[0], ops.F32 if f32 else ops.BF16, _stream())
        with knobs(kn):
            _, seen = launched(run)
        torch.cuda.synchronize()
        assert kernel in seen, (kernel, sorted(seen))
        for k, pk in srcs.items():
            assert not pk.guard_fails() and BC.bit_equal(pk.body.cpu(), torch.from_numpy(src_np[k]).reshape(-1)), f'residue {res}: source {k} changed'
        kinds = set()
        for dname, (n, a32) in dst_plan.items():
            val, wr = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=bool)
            for s, dn, off, kind, R_, C_, p0, p1, pad in recs:
                if dn == dname:
                    v, w = BC.wprep_ref(kind, src_np[s], R_, C_, p0, p1, pad, n - off)
                    assert not (wr[off:] & w).any(), 'two records own one element'
                    val[off:][w] = v[w]
                    wr[off:] |= w
                    kinds.add(kind)
            got = dsts[dname].cpu()
            assert not torch.isnan(got.float())[torch.from_numpy(wr)].any(), f'residue {res}: {dname}: NaN left inside the logical extent'
            assert torch.isnan(got.float())[torch.from_numpy(~wr)].all(), f'residue {res}: {dname}: written outside the record\'s elements'
            if a32 or f32:
                same = got.numpy().view(np.uint32)[wr] == val.view(np.uint32)[wr]
            else:
                same = got.view(torch.int16).numpy().view(np.uint16)[wr] == BC.bf16_bits(val)[wr]
            assert same.all(), f'residue {res}: {dname}: {int((~same).sum())} of {int(wr.sum())} elements differ from the restatement'
        assert kinds == ({1, 2, 3, 4, 5, 6, 7} if f32 else set(range(10)))
        report['residues'][res] = {'kernels': sorted(seen), 'records': len(recs), 'chunks': int(chunks.shape[0])}
    _report(report)


@pytest.mark.parametrize('f32', [False, True], ids=['bf16', 'fp32'])
def test_stand_alone_weight_operands_read_packed_masters(gpu, f32):
    """ltu_cast_f32, ltu_transpose_f32, ltu_pack_conv_weight (the operand preparation of ops without a weight store) with the source
    at residues 0..3: equal to numpy, hence bit-equal across residues"""
    from lintransunet_amd import ops
    src_np = _sources()
    odt, code = (torch.float32, ops.F32) if f32 else (torch.bfloat16, ops.BF16)

    def same(got, val):
        if f32:
            return bool((got.cpu().numpy().view(np.uint32).reshape(-1) == val.view(np.uint32).reshape(-1)).all())
        return bool((got.cpu().view(torch.int16).numpy().view(np.uint16).reshape(-1) == BC.bf16_bits(val).reshape(-1)).all())
    for res in BC.RESIDUES:
        srcs = {k: BC.Packed([v.size], res, [torch.from_numpy(v)]) for k, v in src_np.items()}
        w = src_np['w96x40']
        cast = torch.full((w.size,), float('nan'), device=DEV, dtype=odt)
        _call('ltu_cast_f32', _ptr(srcs['w96x40'].views[0]), _ptr(cast), w.size, code, _stream())
        assert same(cast, w), f'residue {res}: ltu_cast_f32'
        ldo, off = 200, 4                                             # two blocks side by side would give ldo = 192; 200 leaves columns unwritten
        tr = torch.full((40, ldo), float('nan'), device=DEV, dtype=odt)
        _call('ltu_transpose_f32', _ptr(srcs['w96x40'].views[0]), _ptr(tr), 96, 40, ldo, off, code, _stream())
        assert same(tr[:, off:off + 96].contiguous(), np.ascontiguousarray(w.T)), f'residue {res}: ltu_transpose_f32'
        assert torch.isnan(tr[:, :off].float()).all() and torch.isnan(tr[:, off + 96:].float()).all()
        c = src_np['conv5x12']
        wf = torch.full((8 * 27 * 16,), float('nan'), device=DEV, dtype=odt)
        wd = torch.full((16 * 27 * 8,), float('nan'), device=DEV, dtype=odt)
        _call('ltu_pack_conv_weight', _ptr(srcs['conv5x12'].views[0]), _ptr(wf), _ptr(wd), 5, 12, 8, 16, code, _stream())
        assert same(wf, BC.wprep_ref(2, c, 5, 12, 8, 16, 0, wf.numel())[0]), f'residue {res}: ltu_pack_conv_weight wf'
        assert same(wd, BC.wprep_ref(3, c, 5, 12, 8, 16, 0, wd.numel())[0]), f'residue {res}: ltu_pack_conv_weight wd'
        torch.cuda.synchronize()
        for k in ('w96x40', 'conv5x12'):
            assert not srcs[k].guard_fails() and BC.bit_equal(srcs[k].body.cpu(), torch.from_numpy(src_np[k]).reshape(-1))
    _report({'part': 2, 'case': f'stand_alone_operands/{"fp32" if f32 else "bf16"}', 'residues': list(BC.RESIDUES)})


# ---------------------------------------------------------------------------------------------- part 3: optimizer tails

OPT_SIZES = [1, 3, 1021, 4 * 256 * 8 + 2]
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)


def _opt_arrays(n, seed):
    g = torch.Generator().manual_seed(seed)
    p, gr, m = (torch.randn(n, generator=g) for _ in range(3))
    return p, 0.1 * gr, 0.05 * m, 1e-3 * torch.rand(n, generator=g), torch.randn(n, generator=g)


def _close(what, got, ref):
    """test_optim.py's tolerance against the float64 step"""
    assert torch.allclose(got.double().cpu(), ref, rtol=2e-5, atol=2e-7), f'{what}: max |err| {(got.double().cpu() - ref).abs().max().item():.3g}'


@pytest.mark.parametrize('n', OPT_SIZES)
def test_adamw_tail_and_guards(gpu, n):
    """ltu_adamw on buffers of n floats (n % 4 in {1, 2, 3}: the scalar tail) inside guard bands: float64 AdamW, guards intact"""
    p, g, m, v, _ = _opt_arrays(n, 500 + n)
    pk = [BC.Packed([n], 0, [t]) for t in (p, g, m, v)]
    step, gscale = 3, 0.5
    h = HYPER
    _call('ltu_adamw', *(_ptr(k.views[0]) for k in pk), n, h['lr'], h['b1'], h['b2'], h['eps'], h['wd'], step, gscale, _stream())
    torch.cuda.synchronize()
    for what, k in zip('pgmv', pk):
        assert not k.guard_fails(), (what, k.guard_fails())
    assert BC.bit_equal(pk[1].body.cpu(), g)
    p2, m2, v2, _ = BC.adamw_ref(p.double(), g.double(), m.double(), v.double(), h['lr'], h['b1'], h['b2'], h['eps'], h['wd'], step, gscale)
    for what, k, ref in (('p', pk[0], p2), ('m', pk[2], m2), ('v', pk[3], v2)):
        _close(what, k.body, ref)
    assert not BC.bit_equal(pk[0].body.cpu()[-1:], p[-1:]), 'the last element was not updated'
    _report({'part': 3, 'case': f'ltu_adamw/{n}', 'guards': 'intact'})


@pytest.mark.parametrize('ema', [False, True], ids=['no_ema', 'ema'])
@pytest.mark.parametrize('n', OPT_SIZES)
def test_guarded_adamw_tail_and_guards(gpu, n, ema):
    """ltu_grad_sumsq -> ltu_adamw_guard -> ltu_adamw_guarded on guarded buffers: the partial sums give the float64 sum of squares
    within 1e-6 relative, the clipped step is the float64 step, no guard float changes"""
    from lintransunet_amd import _lib
    lib = _lib.load()
    p, g, m, v, e = _opt_arrays(n, 600 + n)
    arrays = [p, g, m, v] + ([e] if ema else [])
    pk = [BC.Packed([n], 0, [t]) for t in arrays]
    parts = int(lib.ltu_grad_sumsq_parts(n))
    scratch = BC.Packed([parts], 0, [torch.zeros(parts)])
    state = torch.zeros(12, device=DEV, dtype=torch.float32)
    gscale, decay, h = 0.5, 0.9, HYPER
    ss = ((g.double() * gscale) ** 2).sum().item()
    max_norm = 0.5 * math.sqrt(ss)                                    # clips: the coefficient is 0.5 gscale
    _call('ltu_grad_sumsq', _ptr(pk[1].views[0]), n, gscale, _ptr(scratch.views[0]), parts, _stream())
    _call('ltu_adamw_guard', _ptr(scratch.views[0]), parts, _ptr(state), gscale, max_norm, 1, h['b1'], h['b2'], _stream())
    _call('ltu_adamw_guarded', _ptr(pk[0].views[0]), _ptr(pk[1].views[0]), _ptr(pk[2].views[0]), _ptr(pk[3].views[0]),
          _ptr(pk[4].views[0]) if ema else 0, n, h['lr'], h['b1'], h['b2'], h['eps'], h['wd'], decay if ema else 0.0, _ptr(state), _stream())
    torch.cuda.synchronize()
    for k in pk + [scratch]:
        assert not k.guard_fails(), k.guard_fails()
    assert BC.bit_equal(pk[1].body.cpu(), g)
    got_ss = scratch.body.double().sum().item()
    assert abs(got_ss - ss) <= 1e-6 * ss, (got_ss, ss)
    coef = gscale * min(1.0, max_norm / (math.sqrt(ss) + 1e-6))
    p2, m2, v2, e2 = BC.adamw_ref(p.double(), g.double(), m.double(), v.double(), h['lr'], h['b1'], h['b2'], h['eps'], h['wd'], 1, coef,
                                  e.double() if ema else None, decay)
    for what, k, ref in (('p', pk[0], p2), ('m', pk[2], m2), ('v', pk[3], v2)) + ((('ema', pk[4], e2),) if ema else ()):
        _close(what, k.body, ref)
    _report({'part': 3, 'case': f'ltu_adamw_guarded/{n}/{"ema" if ema else "no_ema"}', 'sumsq_rel_err': abs(got_ss - ss) / ss, 'guards': 'intact'})


# ---------------------------------------------------------------------------------------------- part 4: the real model

CLASSES = 3
# Gradients that no-reducer and reducer steps form with DIFFERENT kernels, whatever the addresses (a documented change of summation
# order, not of alignment): a parameter whose gradient is not a fused bucket view takes, in ops._Linear.backward / ops._LayerTail
# (_wgrad_now_or_group), one ltu_linear_wgrad per projection instead of the layer's grouped launch (wgrad_group_push: "only
# gradients that live in a reducer's flat buffer take part"), and in ops._LayerTail / ops._ResLayerNorm it folds the gamma / beta
# partials at once (ltu_reduce_batch on one job, reduce_parts) instead of deferring them to the batched fold.  Against the
# no-reducer step these are held to test_gpu_structure's tolerances; between the three reducer layouts they must be bit-equal too.
FUSION_DEPENDENT = ('.self_attn.linears.', '.linear1.', '.linear2.', '.layer_norm1.', '.layer_norm2.')
# psi's gradients are reached through atomicAdd, one per sample (gate_fold_kernel, see bucket_common.CASES): with B = 2 either order of
# the two additions may win in any variant, so a difference there is held to the same tolerances in every comparison
ATOMIC_ORDER = ('.psi.0.',)


def _model_and_inputs():
    from lintransunet_amd import train
    from lintransunet_amd.model import get_model_dict
    from oracle import net as O_net, seedgen, step as O_step
    cfg = O_net.NetConfig(dim_output=CLASSES)
    assert cfg.num_layers == [16, 32, 64, 128, 256] and cfg.roi_size_list == [100, 65, 40, 25, 10]
    m = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, 1, CLASSES, dropout=0.0, act_dtype=torch.bfloat16)
    m.load_state_dict(seedgen.seeded_params(O_net.param_shapes(cfg), 4242), strict=True)
    m = m.to(DEV).train()
    x = seedgen.seeded_volume((2, 1, 64, 64, 32), 31).to(DEV)
    lab = seedgen.seeded_label((2, 1, 64, 64, 32), 32, n_classes=CLASSES).to(DEV)
    specs = train.level_specs(5, ('CrossEntroLoss', 'DiceClassLoss', 'DiceClassLoss2'), criterion_weight=[10, 1, 2])
    return m, x, lab, O_step.dynamic_weights(0), specs


def _grads(m):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _compare(got, ref, tag, exact):
    """bit-equality of every gradient; the ATOMIC_ORDER ones and, unless `exact`, the FUSION_DEPENDENT ones may instead lie within
    test_gpu_structure's TOL / TOL_BIAS (rel-L2, a bias floored at 1e-4 of its module's weight-gradient norm, the analytically zero
    ones at that norm)"""
    from tests.test_gpu_structure import ANALYTIC_ZERO, TOL, TOL_BIAS
    assert set(got) == set(ref)
    nbit, bad, worst = 0, [], (0.0, None)
    for k, r in ref.items():
        g = got[k]
        if r is None or g is None:
            assert r is None and g is None, f'{tag}: {k} has a gradient in one variant only'
            continue
        if BC.bit_equal(g, r):
            nbit += 1
            continue
        partner = ref.get(k[:-len('bias')] + 'weight') if k.endswith('.bias') else None
        floor = (1.0 if k.endswith(ANALYTIC_ZERO) else 1e-4) * partner.norm().item() if partner is not None else 0.0
        err = (g - r).norm().item() / max(r.norm().item(), floor, 1e-30)
        if err > worst[0]:
            worst = (err, k)
        if not any(s in k for s in ATOMIC_ORDER + (() if exact else FUSION_DEPENDENT)):
            bad.append(f'{k}: differs in bits (rel-L2 {err:.3e})')
        elif not err <= (TOL_BIAS if k.endswith('.bias') else TOL):
            bad.append(f'{k}: rel-L2 {err:.3e} (|g| {r.norm().item():.3e}, floor {floor:.3e})')
    print(f'[{tag}] {nbit} gradients bit-equal, worst rel-L2 {worst[0]:.2e} ({worst[1]})')
    assert not bad, tag + ':\n  ' + '\n  '.join(bad)
    return nbit, worst


def test_model_gradients_do_not_depend_on_the_bucket_layout(gpu):
    """one eager train_step on the same seeded weights and inputs with (i) no reducer, (ii) the reducer in registration order,
    (iii) after rebucket(), (iv) with the weights re-homed by FusedAdamW: equal level losses; (iii) and (iv) bit-equal to (ii) in
    every gradient; (ii) bit-equal to (i) outside FUSION_DEPENDENT (named there), those within test_gpu_structure's tolerances.
    Observed: 600 / 600 bit-equal between the reducer layouts, 417 / 600 against (i) (worst rel-L2 9e-6, a q-projection bias); in the
    gradient-ready order the 16 views of the decoder's conv pairs (conv1 + mask head, behind the one-float psi biases) sit at
    residue 1 and every other family at residue 0: for those, part 1 is the only test off 16-byte alignment"""
    from lintransunet_amd import optim, train
    w = None

    def step(m, x, lab, w, specs, red=None):
        if red is not None:
            red.zero_grad()
        tot, _ = train.train_step(m, x, lab, w, specs=specs, reducer=red)
        torch.cuda.synchronize()
        return [t.item() for t in tot]
    # (i)
    m, x, lab, w, specs = _model_and_inputs()
    loss = {'none': step(m, x, lab, w, specs)}
    grads = {'none': _grads(m)}
    unused = set(train.UNUSED_PARAMETERS)
    assert all((g is None) == (k in unused) for k, g in grads['none'].items())
    del m
    # (ii) .. (iv) on one model: the layouts follow one another as in training
    m, x, lab, w, specs = _model_and_inputs()
    red = train.GradReducer(m, bucket_mb=32.0, unused=train.UNUSED_PARAMETERS)
    rows = {'registration': BC.census(m, red)}
    loss['registration'] = step(m, x, lab, w, specs, red)
    grads['registration'] = _grads(m)
    red.rebucket()
    rows['ready'] = BC.census(m, red)
    loss['ready'] = step(m, x, lab, w, specs, red)
    grads['ready'] = _grads(m)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = optim.FusedAdamW(red)
    assert opt.generation == red.generation
    for k, p in m.named_parameters():
        assert BC.bit_equal(p.detach(), before[k]), f'{k}: re-homing changed the weight'
    weight_rows = []
    for plist, flat in zip(red.buckets, opt.flat_p):
        off = 0
        for p in plist:
            assert p.data.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() and p.data.storage_offset() == off
            weight_rows.append(off % 4)
            off += p.numel()
        assert off == flat.numel()
    assert weight_rows == [r for _, _, r, _ in rows['ready']], 'the masters sit at the offsets of their gradients'
    loss['rehomed'] = step(m, x, lab, w, specs, red)
    grads['rehomed'] = _grads(m)
    assert rows['ready'] == BC.census(m, red)
    # nothing outside a bucket: the views tile every bucket (BC.census) and the unused parameters got nothing
    for k, p in m.named_parameters():
        assert (p.grad is None) == (k in unused), k
    for f in red.flat:
        assert f.data_ptr() % 16 == 0 and torch.isfinite(f).all()
    assert loss['registration'] == loss['none'] and loss['ready'] == loss['none'] and loss['rehomed'] == loss['none'], loss
    out = {}
    out['registration vs none'] = _compare(grads['registration'], grads['none'], 'registration order vs no reducer', exact=False)
    out['ready vs registration'] = _compare(grads['ready'], grads['registration'], 'after rebucket vs registration order', exact=True)
    out['rehomed vs registration'] = _compare(grads['rehomed'], grads['registration'], 're-homed weights vs registration order', exact=True)
    _compare(grads['ready'], grads['none'], 'after rebucket vs no reducer', exact=False)
    _compare(grads['rehomed'], grads['none'], 're-homed weights vs no reducer', exact=False)
    # the census: 600 bucketed parameters, 24 views off 16-byte alignment in registration order at 3 classes
    reg = rows['registration']
    assert len(reg) == 600 and sum(1 for r in reg if r[2]) == 24, (len(reg), sum(1 for r in reg if r[2]))
    ready = BC.census_by_family(rows['ready'])
    assert any(r for fam in ready.values() for r in fam if r), 'the gradient-ready order left every view 16-byte aligned'
    none_off = sorted(f for f in BC.ENTRY_POINTS if not any(r for r in ready.get(f, {}) if r))
    print(f'[census, gradient-ready order] {ready}; families with every view aligned (part 1 covers them): {none_off}')
    _report({'part': 4, 'case': 'model', 'loss': loss['none'],
             'compare': {k: {'bit_equal': v[0], 'worst_rel_l2': v[1][0], 'worst': v[1][1]} for k, v in out.items()},
             'census_registration': BC.census_by_family(reg),
             'census_ready': {f: {str(r): n for r, n in d.items()} for f, d in ready.items()},
             'ready_families_all_aligned': none_off,
             'ready_misaligned': [(n, r) for n, _, r, _ in rows['ready'] if r]})
