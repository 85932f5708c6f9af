"""Restatement of the imbalance stage of the level loss (csrc/loss_imbalance.hip: Tversky, focal Tversky and focal cross-entropy)
straight from its formulas, values and analytic gradients, in a number format of choice: float64 is the oracle, float32 the
evaluation whose own deviation from the oracle sets the tolerance.  numpy only: shared by tests/test_imbalance.py (CPU) and
tests/test_gpu_imbalance.py.

With t_c = [label == c] (0 in every class where label >= C), per (sample b, class c):
    I = sum p t    FP = sum p (1 - t)    FN = sum t (1 - p)    F = sum t a_c (1 - p)^gf (-log max(p, 1e-6))
    Tversky term of class c:  r = 1 - TI = (alpha FP + beta FN) / (I + alpha FP + beta FN + eps),  v = r^(1 / gamma)
        per sample: value = mean_b v[b];  batch: I, FP, FN summed over b first, value = v
    focal cross-entropy:      value = (1 / (B S)) sum_{b, c} F[b, c]          (not evaluated, 0, where its weight is 0)
    total = sum_k w_k value_k + w_focal value_focal
Where r is exactly 0 and gamma > 1 the gradient of that term is 0 (the kernels' chosen subgradient); the focal gradient is that of
the clamped expression (no (1 - p)^gf / p part at p <= 1e-6)."""
import numpy as np

from tests.topk_common import make_labels, make_probs, set_label_prob

CLAMP32 = np.float32(1e-6)        # the kernels clamp at the fp32 constant


def sums_ref(p, label, gf=0.0, fa=None, dtype=np.float64):
    """p [B, ..., C], label [B, ...] -> (I, FP, FN, F) [B, C] each, every operation and every sum in `dtype`"""
    dt = np.dtype(dtype).type
    B, C = p.shape[0], p.shape[-1]
    pf = np.asarray(p).reshape(B, -1, C).astype(dtype)
    lab = np.asarray(label).reshape(B, -1).astype(np.int64)
    fa = np.ones(C, dtype) if fa is None else np.asarray(fa, dtype)
    one = dt(1)
    out = np.zeros((4, B, C), dtype)
    for b in range(B):
        for c in range(C):
            t = lab[b] == c
            pc = pf[b, :, c]
            pt = pc[t]
            q = one - pt
            out[0, b, c] = pt.sum(dtype=dtype)
            out[1, b, c] = pc[~t].sum(dtype=dtype)
            out[2, b, c] = q.sum(dtype=dtype)
            nl = -np.log(np.maximum(pt, dt(CLAMP32)))
            pw = np.ones_like(q) if gf == 0 else np.power(q, dt(gf))
            out[3, b, c] = (fa[c] * pw * nl).sum(dtype=dtype)
    return out[0], out[1], out[2], out[3]


def _tversky(I, FP, FN, alpha, beta, gamma, eps, dt):
    """v = r^(1 / gamma) and its derivative as the voxel coefficients (a, bc): dv/dp = a + t bc"""
    num = dt(alpha) * FP + dt(beta) * FN
    ie = I + dt(eps)
    den = ie + num
    r = num / den
    if gamma == 1:
        v, dv = r, np.ones_like(r)
    else:
        ig = dt(1) / dt(gamma)
        pos = r > 0
        v = np.where(pos, np.power(np.where(pos, r, dt(1)), ig), dt(0))
        dv = np.where(pos, ig * v / np.where(pos, r, dt(1)), dt(0))
    d2 = den * den
    return v, dv * (dt(alpha) * ie) / d2, -dv * (num + (dt(alpha) + dt(beta)) * ie) / d2


def imbalance_ref(p, label, classes=(), weights=(), alpha=0.3, beta=0.7, gamma=1.0, eps=1e-5, batch=False, w_focal=0.0, gf=0.0, fa=None,
                  dtype=np.float64, grad=True):
    """-> dict(values [K] Tversky values, focal, total, grad [shape of p] or None, sums): everything in `dtype`"""
    dt = np.dtype(dtype).type
    B, C = p.shape[0], p.shape[-1]
    S = int(np.prod(p.shape[1:-1]))
    I, FP, FN, F = sums_ref(p, label, gf, fa, dtype)
    if w_focal == 0:
        F = np.zeros_like(F)                 # a stage without a focal weight does not evaluate the term: its value reads 0
    A = np.zeros((B, C), dtype)
    Bc = np.zeros((B, C), dtype)
    values = []
    for c, w in zip(classes, weights):
        if batch:
            v, a, bc = _tversky(I[:, c].sum(dtype=dtype), FP[:, c].sum(dtype=dtype), FN[:, c].sum(dtype=dtype), alpha, beta, gamma, eps, dt)
            values.append(v)
            A[:, c] += dt(w) * a
            Bc[:, c] += dt(w) * bc
        else:
            v, a, bc = _tversky(I[:, c], FP[:, c], FN[:, c], alpha, beta, gamma, eps, dt)
            values.append(v.sum(dtype=dtype) / dt(B))
            A[:, c] += dt(w) / dt(B) * a
            Bc[:, c] += dt(w) / dt(B) * bc
    n = dt(B) * dt(S)
    focal = F.sum(dtype=dtype) / n
    total = dt(0)
    for w, v in zip(weights, values):
        total = total + dt(w) * v
    total = total + dt(w_focal) * focal
    g = None
    if grad:
        fav = np.ones(C, dtype) if fa is None else np.asarray(fa, dtype)
        pf = np.asarray(p).reshape(B, S, C).astype(dtype)
        lab = np.asarray(label).reshape(B, S).astype(np.int64)
        g = np.empty((B, S, C), dtype)
        g[:] = A[:, None, :]
        valid = lab < C
        li = np.minimum(lab, C - 1)
        pl = np.take_along_axis(pf, li[..., None], -1)[..., 0]
        q = dt(1) - pl
        inv = np.where(pl > dt(CLAMP32), dt(1) / np.where(pl > 0, pl, dt(1)), dt(0))
        if gf == 0:
            fp = inv                                                             # f = log max(p, 1e-6)
        else:
            L = np.log(np.maximum(pl, dt(CLAMP32)))
            fp = np.power(q, dt(gf - 1)) * (-dt(gf) * L + q * inv)               # f = (1 - p)^gf log max(p, 1e-6)
        G = -dt(w_focal) * fav / n                                               # [C]
        add = np.take_along_axis(Bc, li, -1) + G[li] * fp
        upd = np.take_along_axis(g, li[..., None], -1)[..., 0] + np.where(valid, add, dt(0))
        np.put_along_axis(g, li[..., None], upd[..., None], -1)
        g = g.reshape(p.shape)
    return dict(values=np.array(values, dtype), focal=focal, total=total, grad=g, sums=(I, FP, FN, F))


def _rel(a, b):
    """largest |b - a| / |a| over the entries with a != 0 (absolute where a == 0)"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float((np.abs(b - a) / np.where(a != 0, np.abs(a), 1.0)).max()) if a.size else 0.0


def tolerance(r64, r32):
    """The project's rule on the test's own input: a kernel may deviate from the float64 oracle by 4 x what the float32 evaluation of
    the same formulas deviates.  -> dict(value=(allowed, measured), grad=(allowed, measured)).  `value` is relative: the largest
    deviation over the numbers the forward produces - the sums I, FP, FN, F of every (sample, class), the Tversky values, the focal
    value and the total - each against its own float64 figure; the kernels' report is held to it number by number (value_error).  `grad` is the largest absolute deviation over the voxels divided by the largest |gradient|."""
    dev = max(_rel(_report(r64), _report(r32)), sums_error(r32['sums'], r64))
    out = {'value': (4.0 * dev, dev)}
    if r64['grad'] is not None and r32['grad'] is not None:
        gmax = float(np.abs(r64['grad']).max())
        gdev = float(np.abs(r32['grad'].astype(np.float64) - r64['grad']).max()) / (gmax if gmax > 0 else 1.0)
        out['grad'] = (4.0 * gdev, gdev)
    return out


def sums_error(got, r64):
    """`got` = (I, FP, FN, F) [B, C] each against the oracle's, in the measure of tolerance()['value']"""
    return max(_rel(a, b) for a, b in zip(r64['sums'], got))


def _report(r):
    return [*r['values'], r['focal'], r['total']]


def value_error(got, r64):
    """`got` = [Tversky values .., focal, total] against the oracle, in the measure of tolerance()['value']"""
    ref = _report(r64)
    assert len(got) == len(ref)
    return _rel(ref, got)


def grad_error(got, r64):
    gmax = float(np.abs(r64['grad']).max())
    return float(np.abs(np.asarray(got, np.float64) - r64['grad']).max()) / (gmax if gmax > 0 else 1.0)


# ---------------------------------------------------------------------------------------------- inputs
def late_probs(B, spatial, C, seed, confident=0.97):
    """Late in training: `confident` of the voxels have p[label] >= 0.999, half of those exactly 1.0 with exact zeros in the other
    channels; the rest are make_probs.  -> (p fp32 [B, *spatial, C], label u8)"""
    rng = np.random.default_rng(seed)
    p = make_probs(B, spatial, C, seed + 1)
    lab = make_labels(B, spatial, C, seed + 2)
    u = rng.random(lab.shape)
    conf = u < confident
    exact = u < confident / 2
    near = (0.999 + 0.001 * rng.random(lab.shape)).astype(np.float32)
    near = np.minimum(near, np.nextafter(np.float32(1), np.float32(0)))
    sharp = set_label_prob(p, lab, np.where(exact, np.float32(1), near))
    return np.where(conf[..., None], sharp, p).astype(np.float32), lab


def onehot_probs(label, C):
    """p = the one-hot of the label (fp32): every Tversky term has 1 - TI exactly 0"""
    return (np.asarray(label)[..., None] == np.arange(C)).astype(np.float32)
