"""The imbalance stage of the level loss on the GPU (csrc/loss_imbalance.hip: Tversky, focal Tversky, focal cross-entropy) against
the float64 restatement of tests/imbalance_common.py: every parameter on the shapes that reach each code path, classes that are
absent, labels without a channel, the late-training input, the argument contract, the stage inside the loss chain, graph capture,
and a training step (eager and captured) with the names at all five levels.

Tolerance: the project's rule.  Each comparison computes, on the CPU and on its own input, how far a float32 evaluation of the same
formulas is from the float64 one (imbalance_common.tolerance) and allows the kernels 4 x that.  Values: setting by setting,
relative, over the numbers the forward produces (the four sums of every (sample, class), the Tversky values, the focal value, the
total); the kernels' report is held to it number by number, their sums to a bound of their own (SUMS_BOUND).  Gradients: the largest absolute deviation over the largest
|gradient|, the float32 deviation taken as the largest over the settings a test runs on its input.  Setting by setting the rule
cannot be met for the gradients: on single settings the float32 evaluation lands as close as 9.3e-9 of the largest gradient to the
float64 one, a sixth of half an ulp of fp32, while any fp32 kernel is a rounding or two away (kernel 0.97 - 1.4e-7 against 4 x
1.9 - 2.9e-8 on such settings).  The measured figures are in DESIGN.md."""
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import net as O_net          # noqa: E402
from oracle import seedgen               # noqa: E402
from oracle import step as O_step        # noqa: E402
from tests.imbalance_common import grad_error, imbalance_ref, late_probs, onehot_probs, sums_error, tolerance, value_error
from tests.topk_common import make_labels, make_probs

pytestmark = pytest.mark.gpu

DEV = 'cuda'
E_SHAPE, E_ARG = -2, -4
SMALL = dict(num_layers=[8, 8, 8, 16, 32], roi_size_list=[20, 12, 9, 10, 6])      # of tests/test_gpu_boundary.py
S4 = (2, (12, 10, 8))           # S % 4 == 0: the four-voxel kernels, 4 blocks per sample, the last one ragged
ODD = (1, (9, 7, 5))            # S odd: the scalar kernels, 2 blocks
WIDE = (3, (8, 8, 6))           # at C = 8: one trip in flight
BIG = (8, (64, 64, 96))         # 3072 voxels a block: a two-in-flight trip and a remainder trip; B C 4 = 256 at C = 8
TVERSKY = list(itertools.product([(0.3, 0.7), (0.5, 0.5)], [1.0, 4.0 / 3.0], [False, True]))
# The kernels' four sums per (sample, class), read back from the scratch, against the float64 ones.  They are sums of non-negative
# fp32 terms, so their relative error is at most (additions on the longest path) x 2^-24: on the shapes here at most 12 in a thread
# (three trips of four voxels), 6 in the wave, 4 across the waves and 20 in the fold of up to 128 partials, 42 in all; 64 is allowed.
# The float32 rule is not applied to them: numpy sums pairwise and lands within 3e-8 on some inputs, which no other order of fp32
# additions is bound to match (1.4e-7 was measured)
SUMS_BOUND = 64 * 2.0 ** -24
# focal gamma: 0, 1 and 2 are formed by products, every other value through exp2 / log2: 1.5 (an exponent below 1 in the derivative)
# and 2.5
FOCAL = list(itertools.product([0.0, 1.0, 1.5, 2.0, 2.5], [False, True]))


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _t(x):
    return torch.tensor([x], device=DEV, dtype=torch.float32)


def _floats(v):
    import ctypes
    return (ctypes.c_float * len(v))(*[float(x) for x in v])


def _ints(v):
    import ctypes
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _fa(C):
    return tuple(0.25 + 0.5 * ((3 * c) % C) for c in range(C))


class Kernels:
    """ltu_loss_imb_fwd / _bwd on one (p, label) through the raw C-ABI; the scratch is filled with garbage first"""

    def __init__(self, p, lab):
        from lintransunet_amd import _lib
        self.lib = _lib
        self.p = torch.from_numpy(np.array(p)).to(DEV)
        self.lab = torch.from_numpy(np.array(lab)).to(DEV)
        self.B, self.C = p.shape[0], p.shape[-1]
        self.S = int(np.prod(p.shape[1:-1]))
        self.need = _lib.load().ltu_loss_imb_ws_floats(self.B, self.S, self.C)
        assert self.need > 0
        self.sums = torch.full((self.need,), float('nan'), device=DEV)      # no initialisation needed
        self.coef = torch.full((self.B, self.C, 3), float('nan'), device=DEV)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.gf = 0.0

    def fwd(self, classes=(), weights=(), alpha=0.3, beta=0.7, gamma=1.0, eps=1e-5, batch=False, w_focal=0.0, gf=0.0, fa=None,
            base_total=None, scale_dev=None):
        K = len(classes)
        values = torch.full((K + 3,), float('nan'), device=DEV)
        self.gf = gf
        self.lib.call('ltu_loss_imb_fwd', self.p.data_ptr(), self.lab.data_ptr(), self.sums.data_ptr(), self.need, values.data_ptr(),
                      self.coef.data_ptr(), _ptr(base_total), _ints(classes), _floats(weights), K,
                      _floats([alpha, beta, gamma, eps, 1.0 if batch else 0.0]), w_focal, gf, None if fa is None else _floats(fa),
                      _ptr(scale_dev), self.B, self.S, self.C, self.stream)
        return values.cpu().numpy()

    def bwd(self, dp=None, accumulate=0, g=1.0):
        dp = torch.full_like(self.p, float('nan')) if dp is None else dp
        self.lib.call('ltu_loss_imb_bwd', self.p.data_ptr(), self.lab.data_ptr(), self.coef.data_ptr(), self.coef.numel(), self.gf,
                      _t(g).data_ptr(), dp.data_ptr(), accumulate, self.B, self.S, self.C, self.stream)
        return dp.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(B, spatial, C):
    p, lab = make_probs(B, spatial, C, 17 * B + C), make_labels(B, spatial, C, 19 * B + C)
    p.setflags(write=False)
    lab.setflags(write=False)
    return p, lab


def _allowed(p, lab, cfgs):
    """-> (oracles, allowed value deviation of each setting, allowed gradient deviation) for the settings `cfgs` a test runs on
    (p, lab): 4 x the deviation of the float32 evaluation - of each setting for the values, the largest over the settings for the
    gradients (see the module's docstring)"""
    r64 = [imbalance_ref(p, lab, **cfg) for cfg in cfgs]
    tols = [tolerance(r, imbalance_ref(p, lab, dtype=np.float32, **cfg)) for r, cfg in zip(r64, cfgs)]
    dv, dg = [t['value'][1] for t in tols], [t['grad'][1] for t in tols]
    print(f'float32 evaluation over {len(cfgs)} settings: values {min(dv):.2e} .. {max(dv):.2e}, gradients {min(dg):.2e} .. {max(dg):.2e}')
    return r64, [4.0 * d for d in dv], 4.0 * max(dg)


def _kernel_sums(kern, cfg):
    """(I, FP, FN, F) [B, C] as the finalize kernel left them at the head of the scratch; F there is without the class weight"""
    s = kern.sums[:kern.B * kern.C * 4].cpu().numpy().astype(np.float64).reshape(kern.B, kern.C, 4)
    fa = np.ones(kern.C) if cfg.get('fa') is None else np.asarray(cfg['fa'], np.float64)
    return s[..., 0], s[..., 1], s[..., 2], s[..., 3] * fa


def _check(kern, p, lab, cfgs, what):
    """forward + backward of every setting against the oracle at the project's tolerance; -> [(values, dp)]"""
    r64, tol_v, tol_g = _allowed(p, lab, cfgs)
    out, worst_v, worst_s, worst_g = [], 0.0, 0.0, 0.0
    for cfg, r, tv in zip(cfgs, r64, tol_v):
        v = kern.fwd(**cfg)
        er, es = value_error(v[1:-1].tolist() + [v[0]], r), sums_error(_kernel_sums(kern, cfg), r)
        dp = kern.bwd()
        eg = grad_error(dp, r)
        worst_v, worst_s, worst_g = max(worst_v, er / tv if tv else float(er > 0)), max(worst_s, es), max(worst_g, eg)
        assert np.isfinite(v).all() and np.isfinite(dp).all()
        assert v[0] == v[-1]                                         # the second copy of the total
        assert er <= tv and eg <= tol_g, (what, cfg, f'report {er:.3e} allowed {tv:.3e}', eg, tol_g)
        assert es <= SUMS_BOUND, (what, cfg, es)
        out.append((v, dp))
    print(f'{what}: kernel values at most {worst_v:.2f} of the allowed; sums {worst_s:.2e}; gradients {worst_g:.2e} allowed {tol_g:.2e}')
    return out


def _cfg(tv, fo, C, classes=None):
    (alpha, beta), gamma, batch = tv
    gf, with_fa = fo
    classes = tuple(range(C)) if classes is None else classes
    return dict(classes=classes, weights=tuple(1.0 - 0.125 * k for k in range(len(classes))), alpha=alpha, beta=beta, gamma=gamma,
                batch=batch, w_focal=0.75, gf=gf, fa=_fa(C) if with_fa else None)


# ---------------------------------------------------------------------------------------------- 1. kernels against float64
@pytest.mark.parametrize('shape,C', [(S4, 2), (S4, 5), (S4, 8), (ODD, 2), (ODD, 5), (ODD, 8), (WIDE, 8)])
def test_kernels_against_float64(shape, C):
    """every Tversky setting with every focal setting, all classes as terms (up to 8, one weight each)"""
    B, spatial = shape
    p, lab = _case(B, spatial, C)
    kern = Kernels(p, lab)
    cfgs = [_cfg(tv, fo, C) for tv, fo in itertools.product(TVERSKY, FOCAL)]
    v, dp = _check(kern, p, lab, cfgs, f'B={B} {spatial} C={C}')[0]
    assert np.array_equal(kern.fwd(**cfgs[0]), v) and np.array_equal(kern.bwd(), dp)      # a second call, after all the others: bit for bit


@pytest.mark.parametrize('C', [2, 8])
def test_kernels_against_float64_many_blocks(C):
    B, spatial = BIG
    p, lab = _case(B, spatial, C)
    kern = Kernels(p, lab)
    classes = (1, 0) if C == 2 else (1, 7, 4)
    cfgs = [_cfg(((0.3, 0.7), 4.0 / 3.0, False), (2.0, True), C, classes), _cfg(((0.5, 0.5), 1.0, True), (0.0, False), C, classes)]
    _check(kern, p, lab, cfgs, f'B={B} {spatial} C={C}')


# ---------------------------------------------------------------------------------------------- 2. absent classes, labels >= C
@pytest.mark.parametrize('batch', [False, True])
def test_absent_classes_and_labels_without_a_channel(batch):
    (B, spatial), C = S4, 5
    p, lab = _case(B, spatial, C)
    lab = lab.copy()
    lab[0][lab[0] == 3] = 1                                          # class 3: absent from sample 0
    lab[lab == 4] = 2                                                # class 4: absent from the whole batch
    odd = np.random.default_rng(5).choice(lab.size, 9, replace=False)
    lab.reshape(-1)[odd] = 200                                       # no channel: t = 0 everywhere
    kern = Kernels(p, lab)
    cfg = _cfg(((0.3, 0.7), 4.0 / 3.0, batch), (2.0, True), C, (1, 3, 4))
    v, dp = _check(kern, p, lab, [cfg], f'absent classes, batch={batch}')[0]
    # an absent class is all false positives: 1 - TI = alpha FP / (alpha FP + eps), just below 1
    assert 0.999 < v[3] < 1.0
    r = imbalance_ref(p, lab, **cfg)
    assert not r['grad'].reshape(-1, C)[odd][:, [0, 2]].any() and not dp.reshape(-1, C)[odd][:, [0, 2]].any()      # classes without a term


# ---------------------------------------------------------------------------------------------- 3. late in training
def test_late_input():
    (B, spatial), C = S4, 3
    p, lab = late_probs(B, spatial, C, 31)
    pl = np.take_along_axis(p, lab[..., None].astype(np.int64), -1)[..., 0]
    assert (pl >= 0.999).mean() > 0.95 and 0.4 < (pl == 1.0).mean() < 0.55
    kern = Kernels(p, lab)
    settings = ((((0.3, 0.7), 4.0 / 3.0, False), (2.0, True)), (((0.5, 0.5), 1.0, True), (0.0, False)), (((0.3, 0.7), 4.0 / 3.0, True), (1.0, False)),
                (((0.3, 0.7), 4.0 / 3.0, False), (1.5, True)), (((0.5, 0.5), 1.0, True), (2.5, False)), (((0.3, 0.7), 1.0, False), (2.5, True)))
    _check(kern, p, lab, [_cfg(tv, fo, C) for tv, fo in settings], 'late')
    sums = kern.sums[:B * C * 4].cpu().numpy()
    assert (sums >= 0).all()                                         # I, FP, FN, F: no difference of two sums anywhere


def test_exactly_zero_term_has_zero_gradient():
    (B, spatial), C = S4, 3
    lab = _case(B, spatial, C)[1]
    p = onehot_probs(lab, C)
    kern = Kernels(p, lab)
    for batch in (False, True):
        v = kern.fwd(classes=(0, 1, 2), weights=(1.0, 1.0, 1.0), gamma=4.0 / 3.0, batch=batch)
        dp = kern.bwd()
        assert not v.any() and not dp.any(), (v, np.abs(dp).max())   # 1 - TI == 0: value 0, and the chosen subgradient 0
    # gamma = 1 has a finite derivative there, and the focal term's is 0 at p = 1 for gamma_f >= 1
    # (q = 1 - p is exactly 0 on every voxel: the exp2 / log2 form of 1.5 and 2.5 meets log2(0))
    for v, dp in _check(kern, p, lab, [_cfg(((0.3, 0.7), 1.0, False), (gf, fa), C) for gf in (2.0, 1.5, 2.5) for fa in (False, True)],
                        'one-hot, gamma 1'):
        assert not v.any() and dp.any()


# ---------------------------------------------------------------------------------------------- 4. focal at gamma 0 = top-k at 1.0
def test_focal_gamma_zero_against_topk_at_fraction_one():
    from lintransunet_amd import ops
    (B, spatial), C = S4, 5
    p, lab = _case(B, spatial, C)
    r64 = imbalance_ref(p, lab, w_focal=1.0, gf=0.0)
    tol = tolerance(r64, imbalance_ref(p, lab, w_focal=1.0, gf=0.0, dtype=np.float32))
    pt, labt = torch.from_numpy(np.array(p)).to(DEV), torch.from_numpy(np.array(lab)).to(DEV)
    pa = pt.clone().requires_grad_(True)
    ta, base_values, va = ops.level_loss_imbalance(pa, labt, focal=(1.0, 0.0, None))
    ta.backward()
    pb = pt.clone().requires_grad_(True)
    tb, _, vb = ops.level_loss_topk(pb, labt, 1.0, frac=1.0)
    tb.backward()
    torch.cuda.synchronize()
    assert base_values is None and va.shape == (1,) and not va.requires_grad and va[0].item() == ta.item()
    ref = float(r64['focal'])
    ea, eb, ed = abs(ta.item() - ref) / ref, abs(tb.item() - ref) / ref, abs(ta.item() - tb.item()) / ref
    ga, gb = pa.grad.cpu().numpy(), pb.grad.cpu().numpy()
    gmax = np.abs(r64['grad']).max()
    print(f'value: focal {ea:.2e} top-k {eb:.2e} apart {ed:.2e} float32 {tol["value"][1]:.2e} allowed {tol["value"][0]:.2e}; gradient: '
          f'focal {grad_error(ga, r64):.2e} top-k {grad_error(gb, r64):.2e} apart {np.abs(ga - gb).max() / gmax:.2e} allowed {tol["grad"][0]:.2e}')
    assert ea <= tol['value'][0] and ed <= tol['value'][0]
    assert grad_error(ga, r64) <= tol['grad'][0] and np.abs(ga.astype(np.float64) - gb).max() / gmax <= tol['grad'][0]


# ---------------------------------------------------------------------------------------------- 5. accumulate, scale_dev
def test_accumulate_and_run_time_scale():
    C = 5
    for (Bv, sp) in (S4, ODD):                                       # four-voxel and scalar backward
        p, lab = _case(Bv, sp, C)
        kern = Kernels(p, lab)
        for gf in (2.0, 2.5, 1.5):
            cfg = _cfg(((0.3, 0.7), 4.0 / 3.0, False), (gf, True), C, (1, 2, 4))
            v, dp = _check(kern, p, lab, [cfg], f'accumulate {sp} focal gamma {gf}')[0]      # the write path against the oracle
            assert np.array_equal(kern.bwd(torch.zeros_like(kern.p), accumulate=1), dp)
            # onto something: one fp32 add a channel
            dp0 = torch.from_numpy(np.random.default_rng(9).standard_normal(p.shape).astype(np.float32) * np.abs(dp).max()).to(DEV)
            assert np.array_equal(kern.bwd(dp0.clone(), accumulate=1), dp0.cpu().numpy() + dp)
            assert np.array_equal(kern.bwd(g=-2.0), -2.0 * dp)
            # base total and run-time scale, as defined; the report stays unweighted.  0.25 is a power of two: host weights x 0.25
            # are the same fp32 numbers as scale_dev[0] x weight on the device, so the bits agree
            vs = kern.fwd(base_total=_t(7.5), scale_dev=_t(0.25), **cfg)
            dps = kern.bwd()
            quarter = dict(cfg, weights=tuple(0.25 * w for w in cfg['weights']), w_focal=0.25 * cfg['w_focal'])
            vq = kern.fwd(base_total=_t(7.5), **quarter)
            assert np.array_equal(vs, vq) and np.array_equal(dps, kern.bwd()) and np.array_equal(vs[1:-1], v[1:-1])
            assert abs(vs[0] - (7.5 + 0.25 * v[0])) <= 1e-6 * vs[0] and np.array_equal(dps, 0.25 * dp)


# ---------------------------------------------------------------------------------------------- 6. argument errors
def test_argument_errors_launch_nothing():
    from lintransunet_amd import _lib
    lib = _lib.load()
    B, S, C = 2, 105, 3
    need = lib.ltu_loss_imb_ws_floats(B, S, C)
    SENT = 1234.5
    p, lab = torch.full((B * S * 9,), 0.25, device=DEV), torch.zeros(B * S, device=DEV, dtype=torch.uint8)
    sums, coef = torch.full((need,), SENT, device=DEV), torch.full((B * 9 * 3,), SENT, device=DEV)
    values, dp, one = torch.full((11,), SENT, device=DEV), torch.full_like(p, SENT), torch.ones(1, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    good = dict(alpha=0.3, beta=0.7, gamma=4.0 / 3.0, eps=1e-5, batch=0.0)

    def fwd(Cv=C, Bv=B, n=need, pp=None, classes=(1, 2), w=(1.0, 1.0), w_focal=1.0, gf=2.0, fa=None, cls_ptr=True, **par):
        pr = dict(good, **par)
        return lib.ltu_loss_imb_fwd(p.data_ptr() if pp is None else pp, lab.data_ptr(), sums.data_ptr(), n, values.data_ptr(), coef.data_ptr(), 0,
                                    _ints(classes) if cls_ptr else None, _floats(w), len(classes),
                                    _floats([pr[k] for k in ('alpha', 'beta', 'gamma', 'eps', 'batch')]), w_focal, gf,
                                    None if fa is None else _floats(fa), 0, Bv, S, Cv, st)

    def bwd(Cv=C, Bv=B, n=B * C * 3, gf=2.0, g=None, dpp=None):
        return lib.ltu_loss_imb_bwd(p.data_ptr(), lab.data_ptr(), coef.data_ptr(), n, gf, one.data_ptr() if g is None else g,
                                    dp.data_ptr() if dpp is None else dpp, 0, Bv, S, Cv, st)

    inf, nan = float('inf'), float('nan')
    shape = [fwd(Cv=1), fwd(Cv=9), fwd(Bv=9, Cv=8), fwd(Bv=0), bwd(Cv=1), bwd(Cv=9), bwd(Bv=9, Cv=8)]
    arg = [fwd(n=need - 1), fwd(pp=0), fwd(cls_ptr=False), fwd(classes=(1, 3)), fwd(classes=(-1,), w=(1.0,)), fwd(gf=0.5), fwd(gf=5.5), fwd(gf=nan),
           fwd(gamma=4.0), fwd(gamma=0.5), fwd(gamma=nan), fwd(alpha=-0.1), fwd(alpha=0.0, beta=0.0), fwd(beta=inf), fwd(eps=0.0), fwd(eps=nan),
           fwd(batch=2.0), fwd(w=(1.0, inf)), fwd(w_focal=nan), fwd(fa=(1.0, -1.0, 1.0)), fwd(fa=(1.0, nan, 1.0)),
           fwd(classes=tuple(range(3)) * 3, w=(1.0,) * 9),
           bwd(n=B * C * 3 - 1), bwd(gf=0.5), bwd(g=0), bwd(dpp=0)]
    torch.cuda.synchronize()
    assert shape == [E_SHAPE] * len(shape), shape
    assert arg == [E_ARG] * len(arg), arg
    for t in (sums, coef, values, dp):                               # nothing was launched
        assert (t == SENT).all()
    assert fwd() == 0 and bwd() == 0 and fwd(classes=(), w=(), cls_ptr=False) == 0
    torch.cuda.synchronize()
    assert (dp[:B * S * C] != SENT).all() and (dp[B * S * C:] == SENT).all()
    # the Python entry makes the same checks before the first launch
    from lintransunet_amd import ops
    pc, lc = torch.full((2, 4, 4, 4, 3), 1 / 3, device=DEV), torch.zeros((2, 4, 4, 4), device=DEV, dtype=torch.uint8)
    for kw in (dict(tversky=((3,), (1.0,), None)), dict(tversky=((1,), (1.0,), {'gamma': 4.0})), dict(focal=(1.0, 0.5, None)),
               dict(focal=(1.0, 2.0, (1.0, 1.0))), dict(tversky=((1, 2), (1.0,), None)), dict()):
        with pytest.raises(ValueError):
            ops.level_loss_imbalance(pc, lc, **kw)


# ---------------------------------------------------------------------------------------------- 7. the chain
W_T, W_T2, W_F = 0.7, 0.4, 0.6
REC = dict(alpha=0.3, beta=0.7, tversky_gamma=4.0 / 3.0, batch=True, focal_gamma=2.0)
NEW = {'TverskyLoss': W_T, 'TverskyLoss2': W_T2, 'FocalCELoss': W_F}
SPECS = {'orig': (3, {'CrossEntroLoss': 10, 'DiceClassLoss': 1}), 'wide': (5, {'CrossEntroLoss': 10, 'DiceClassLoss': 1}),
         'ext': (3, {'FocalLoss': 1.0}), 'all': (3, {'CrossEntroLoss': 10, 'DiceClassLoss': 1, 'BoundaryLoss': 0.05, 'TopKCELoss': 1.0}),
         'alone': (3, {})}


def _predict(C, seed):
    """[2, C, 12, 10, 8] probabilities and u8 labels [2, 1, 12, 10, 8]"""
    p = torch.from_numpy(make_probs(2, (12, 10, 8), C, seed)).permute(0, 4, 1, 2, 3).contiguous()
    lab = torch.from_numpy(make_labels(2, (12, 10, 8), C, seed + 1)).unsqueeze(1)
    return p.to(DEV), lab.to(DEV)


def _run(crit, p, lab):
    pp = p.clone().requires_grad_(True)
    total, named = crit(pp, lab)
    total.backward()
    torch.cuda.synchronize()
    return total.detach().clone(), {k: v.clone() for k, v in named.items()}, pp.grad


@pytest.mark.parametrize('family', list(SPECS))
def test_chain_is_the_sum_of_its_stages(family):
    from lintransunet_amd import losses as L
    C, plain = SPECS[family]
    rec = L.Imbalance(**REC)
    p, lab = _predict(C, 50 + C)
    if plain:
        ta, named_a, ga = _run(L.LevelCriterion(plain), p, lab)
    else:
        ta, named_a, ga = torch.zeros((), device=DEV), {}, torch.zeros_like(p)
    ti, named_i, gi = _run(L.LevelCriterion(NEW, imbalance=rec), p, lab)
    spec = dict(plain, **NEW)
    crit = L.LevelCriterion(spec, imbalance=rec)
    tb, named_b, gb = _run(crit, p, lab)
    # total and gradient: the separate ones, joined by one fp32 add
    want = ta.double() + ti.double()
    print(f'{family}: total {tb.item():.8f} separate {ta.item():.8f} + {ti.item():.8f}')
    assert abs(tb.double() - want).item() <= 1e-6 * abs(want).item()
    gsum = ga.double() + gi.double()
    assert (gb.double() - gsum).abs().max().item() <= 1e-6 * gsum.abs().max().item()
    # reports: bit for bit those of the stages alone, in the order of the spec
    assert list(named_b) == list(spec)
    assert all(torch.equal(named_b[n], named_a[n]) for n in plain) and all(torch.equal(named_b[n], named_i[n]) for n in NEW)
    # a second call: bit for bit
    tb2, named_b2, gb2 = _run(crit, p, lab)
    assert torch.equal(tb2, tb) and torch.equal(gb2, gb) and all(torch.equal(named_b2[n], named_b[n]) for n in spec)


def test_spec_without_the_names_is_untouched_by_the_record():
    from lintransunet_amd import losses as L
    spec = {'CrossEntroLoss': 10, 'DiceClassLoss': 1, 'TopKCELoss': 1}
    p, lab = _predict(3, 62)
    ta, named_a, ga = _run(L.LevelCriterion(spec), p, lab)
    tb, named_b, gb = _run(L.LevelCriterion(spec, imbalance=L.Imbalance(alpha=0.5, beta=0.5, tversky_gamma=2.0, batch=True, focal_gamma=0.0)), p, lab)
    assert torch.equal(ta, tb) and torch.equal(ga, gb) and all(torch.equal(named_a[n], named_b[n]) for n in spec)


def test_single_term_modules():
    from lintransunet_amd import losses as L
    p, lab = _predict(5, 64)
    pn, ln = np.ascontiguousarray(p.permute(0, 2, 3, 4, 1).cpu().numpy()), np.ascontiguousarray(lab[:, 0].cpu().numpy())
    modules = ((L.get_criterions(['TverskyLoss'])['TverskyLoss'], dict(classes=(1,), weights=(1.0,))),
               (L.TverskyLoss(class_index=4, alpha=0.5, beta=0.5, gamma=4.0 / 3.0, batch=True),
                dict(classes=(4,), weights=(1.0,), alpha=0.5, beta=0.5, gamma=4.0 / 3.0, batch=True)),
               (L.get_criterions(['FocalCELoss'])['FocalCELoss'], dict(w_focal=1.0, gf=2.0)),
               (L.FocalCELoss(gamma=0.0, alpha=_fa(5)), dict(w_focal=1.0, gf=0.0, fa=_fa(5))))
    # the kernels on these settings against the oracle; a module then gives the bits of the raw call
    kern = Kernels(pn, ln)
    raw = _check(kern, pn, ln, [cfg for _, cfg in modules], 'single-term modules')
    for (module, _), (v, dp) in zip(modules, raw):
        pm = p.clone().requires_grad_(True)
        total = module(pm, lab)
        total.backward()
        assert total.item() == v[0] and np.array_equal(pm.grad.permute(0, 2, 3, 4, 1).cpu().numpy(), dp)


# ---------------------------------------------------------------------------------------------- 8. capture
def test_capture_replays_the_eager_bytes():
    from lintransunet_amd import losses as L
    spec = dict({'CrossEntroLoss': 1.0, 'DiceClassLoss': 1.0}, **NEW)
    inputs = [_predict(3, 70 + 2 * i) for i in range(2)]
    crit = L.LevelCriterion(spec, imbalance=L.Imbalance(**REC))

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
    for p, lab in (inputs[1], inputs[0]):
        with torch.no_grad():
            ps.copy_(p)
        labs.copy_(lab)
        graph.replay()
        torch.cuda.synchronize()
        pe = p.clone().requires_grad_(True)
        total_e, named_e = run(pe, lab)
        torch.cuda.synchronize()
        assert torch.equal(total_s, total_e) and torch.equal(ps.grad, pe.grad)
        assert all(torch.equal(named_s[k], named_e[k]) for k in spec)
        seen.append(total_s.item())
    assert seen[0] != seen[1]                                        # the replay did follow its input


# ---------------------------------------------------------------------------------------------- 9. the training step
NAMES = ('FocalCELoss', 'TverskyLoss', 'TverskyLoss2')
WEIGHTS = [1.0, 0.5, 0.5]


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
    from lintransunet_amd import losses as L, train
    x = seedgen.seeded_volume((2, 1, 32, 32, 32), 901).to(DEV)
    label = seedgen.seeded_label((2, 1, 32, 32, 32), 902, n_classes=3).to(DEV)
    w = O_step.dynamic_weights(0)
    specs = train.level_specs(5, NAMES, criterion_weight=WEIGHTS)
    rec = L.Imbalance(alpha=0.3, beta=0.7, tversky_gamma=4.0 / 3.0, batch=True, focal_gamma=2.0, focal_alpha=(0.5, 1.0, 2.0))
    m, red = _build()
    level_scale = torch.tensor(w, device=DEV, dtype=torch.float32)
    for _ in range(2):
        red.zero_grad()
        totals, named = train.train_step(m, x, label, w, specs=specs, reducer=red, level_scale=level_scale, imbalance=rec)
    torch.cuda.synchronize()
    tot_e, g_eager = [t.item() for t in totals], _grads(m)
    assert g_eager and all(torch.isfinite(g).all() for g in g_eager.values()) and all(np.isfinite(tot_e))
    assert all(list(n) == list(NAMES) for n in named) and len(named) == 5
    # the level totals are those of deep_supervision_loss called directly on the model's outputs
    with torch.no_grad():
        predict, masks = m(x)
    direct, named_d = train.deep_supervision_loss(predict, masks, label, w, specs, level_scale=level_scale, imbalance=rec)
    torch.cuda.synchronize()
    print('level totals', tot_e, 'direct', [t.item() for t in direct])
    assert [t.item() for t in direct] == tot_e
    assert all(torch.equal(named_d[lvl][n], named[lvl][n]) for lvl in range(5) for n in NAMES)
    # other parameters give another loss: the record does reach the kernels
    other, _ = train.deep_supervision_loss(predict, masks, label, w, specs, level_scale=level_scale)
    assert all(a.item() != b for a, b in zip(other, tot_e))
    # the captured step without the weight-gradient queue: the same kernels on one stream, bit for bit
    monkeypatch.setenv('LTU_WQ', '0')
    step = train.GraphedStep(m, x, label, w, red, specs=specs, imbalance=rec)
    assert step.wq_stream is None and step.topk_fraction is None and step.boundary_scale is None and step.imbalance is rec
    tot_g, _ = step(x, label)
    torch.cuda.synchronize()
    assert [t.item() for t in tot_g] == tot_e
    g_graph = _grads(m)
    assert all(torch.isfinite(g).all() for g in g_graph.values())
    differ = [k for k in g_eager if not torch.equal(g_graph[k], g_eager[k])]
    assert not differ, differ
