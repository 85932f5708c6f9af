"""Restatement of region-based training (csrc/region.hip, the sigmoid heads of csrc/pointwise.hip) straight from its rules, in a
number format of choice: float64 is the oracle, float32 the evaluation whose own deviation from the oracle sets the tolerance.
numpy only: shared by tests/test_regions.py (CPU) and tests/test_gpu_regions.py.

Region r is the set of u8 labels members[r]; bits = lut[label], lut[v] = sum_r [v in members[r]] << r; t_r = (bits >> r) & 1.
Pyramid: bitwise OR over (2, 2, kd) windows.  Heads: p = 1 / (1 + exp(-z)), dz = dp p (1 - p) from the stored p.  Per (sample b,
region r):
    I = sum p t    FP = sum p (1 - t)    FN = sum t (1 - p)    E = sum -[t log max(p, 1e-6) + (1 - t) log max(1 - p, 1e-6)]
    BCE = sum_{b, r} E / (B S R)
    D_r = (FP + FN) / (2 I + FP + FN + 2 eps)    batch: I, FP, FN summed over b first;  else the mean over b of the sample's ratio
    Dice = (1 / R) sum_r D_r            total = w_bce BCE + w_dice Dice
The gradient of E is that of the clamped expression: no t / p part at p <= 1e-6, no (1 - t) / (1 - p) part at 1 - p <= 1e-6.
Labels: start at 0; for r = 0 .. R-1 in order write class_order[r] where p_r > threshold.  Counts: TP, FP, FN per (sample, region)
between two bit-mask volumes, Dice = 2 TP / (2 TP + FP + FN), 1 where both sides are empty.

Tolerance (the rule of the issue this file came with): a quantity may deviate from the float64 oracle by 4 x what a float32 evaluation
of the same formula on the same input deviates, and at least by 4 ulps of the value.  The float32 evaluation forms every sum over
voxels in sequence (numpy's cumulative sum): numpy's plain sum adds pairwise, an order no kernel is bound to follow and one that
lands far closer to float64 than a float32 accumulator does; the sequential sum is the plain float32 reading of a sum."""
import numpy as np

CLAMP32 = np.float32(1e-6)        # the kernels clamp at the fp32 constant
ULP32 = 2.0 ** -23                # spacing of fp32 relative to a value in [1, 2)


# ---------------------------------------------------------------------------------------------- table, bits, pyramid
def lut_ref(members):
    lut = np.zeros(256, np.uint8)
    for r, region in enumerate(members):
        for v in region:
            lut[v] |= np.uint8(1 << r)
    return lut


def bits_ref(label, members):
    return lut_ref(members)[np.asarray(label, np.uint8)]


def orpool_ref(bits, kd):
    """u8 [B, H, W, D] -> bitwise OR over (2, 2, kd) windows"""
    B, H, W, D = bits.shape
    x = np.asarray(bits, np.uint8).reshape(B, H // 2, 2, W // 2, 2, D // kd, kd)
    return np.bitwise_or.reduce(np.bitwise_or.reduce(np.bitwise_or.reduce(x, axis=6), axis=4), axis=2)


def maxpool_ref(label, kd):
    B, H, W, D = label.shape
    return np.asarray(label).reshape(B, H // 2, 2, W // 2, 2, D // kd, kd).max(axis=(2, 4, 6))


def pyramid_kds(n_levels):
    """the depth factor of each pooling of train.label_pyramid: level 0 -> 1 with kd 1, then 2, 1, 2 .."""
    return [1] + [2 if lvl % 2 == 0 else 1 for lvl in range(1, n_levels - 1)]


def pyramid_ref(label, members, n_levels):
    """label u8 [B, H, W, D] -> the bit-masks of levels 0 .. n_levels - 1"""
    out = [bits_ref(label, members)]
    for kd in pyramid_kds(n_levels):
        out.append(orpool_ref(out[-1], kd))
    return out


# ---------------------------------------------------------------------------------------------- heads
def sigmoid_ref(z, dtype=np.float64):
    z = np.asarray(z).astype(dtype)
    with np.errstate(over='ignore'):
        return (np.dtype(dtype).type(1) / (np.dtype(dtype).type(1) + np.exp(-z))).astype(dtype)


def sigmoid_grad_ref(dp, p, dtype=np.float64):
    """dz = dp p (1 - p) from the stored (fp32) p"""
    dp, p = np.asarray(dp).astype(dtype), np.asarray(p).astype(dtype)
    return dp * p * (np.dtype(dtype).type(1) - p)


def unembed_ref(z, R):
    """the final head's window un-embedding: z [B, h, w, D, >= 4R] -> [B, 2h, 2w, D, R], channel 4r + 2 kh + kw of coarse voxel
    (h, w) is region r of fine voxel (2h + kh, 2w + kw)"""
    B, h, w, D = z.shape[:4]
    v = np.asarray(z)[..., :4 * R].reshape(B, h, w, D, R, 2, 2)          # [.., r, kh, kw]
    return v.transpose(0, 1, 5, 2, 6, 3, 4).reshape(B, 2 * h, 2 * w, D, R)


def embed_ref(g, CP):
    """the adjoint: g [B, 2h, 2w, D, R] -> [B, h, w, D, CP] with zeros in the padded columns"""
    B, H, W, D, R = g.shape
    v = np.asarray(g).reshape(B, H // 2, 2, W // 2, 2, D, R).transpose(0, 1, 3, 5, 6, 2, 4).reshape(B, H // 2, W // 2, D, 4 * R)
    out = np.zeros((B, H // 2, W // 2, D, CP), v.dtype)
    out[..., :4 * R] = v
    return out


# ---------------------------------------------------------------------------------------------- the loss stage
def _sum(x, dtype):
    """a sum over voxels in `dtype`: float64 as numpy forms it, float32 in sequence (see the module's docstring)"""
    x = np.asarray(x, dtype).ravel()
    if x.size == 0:
        return np.dtype(dtype).type(0)
    return x.sum(dtype=dtype) if np.dtype(dtype) == np.float64 else np.cumsum(x, dtype=dtype)[-1]


def sums_ref(p, bits, dtype=np.float64):
    """p [B, ..., R], bits u8 [B, ...] -> (I, FP, FN, E) [B, R] each, every operation and every sum in `dtype`"""
    dt = np.dtype(dtype).type
    B, R = p.shape[0], p.shape[-1]
    pf = np.asarray(p).reshape(B, -1, R).astype(dtype)
    bt = np.asarray(bits).reshape(B, -1).astype(np.int64)
    out = np.zeros((4, B, R), dtype)
    for b in range(B):
        for r in range(R):
            t = ((bt[b] >> r) & 1).astype(bool)
            pr = pf[b, :, r]
            q = dt(1) - pr
            out[0, b, r] = _sum(pr[t], dtype)
            out[1, b, r] = _sum(pr[~t], dtype)
            out[2, b, r] = _sum(q[t], dtype)
            out[3, b, r] = _sum(-np.log(np.maximum(np.where(t, pr, q), dt(CLAMP32))), dtype)
    return out[0], out[1], out[2], out[3]


def _dice(I, FP, FN, eps, dt):
    """D and its derivative as the voxel coefficients (a, bc): dD/dp = a + t bc"""
    num = FP + FN
    ie = dt(2) * I + dt(2) * dt(eps)
    den = ie + num
    return num / den, ie / (den * den), -dt(2) / den


def region_ref(p, bits, w_bce=1.0, w_dice=1.0, batch=True, eps=1e-5, dtype=np.float64, grad=True):
    """-> dict(bce, dice, D [R], total, grad [shape of p] or None, sums): everything in `dtype`"""
    dt = np.dtype(dtype).type
    B, R = p.shape[0], p.shape[-1]
    S = int(np.prod(p.shape[1:-1]))
    I, FP, FN, E = sums_ref(p, bits, dtype)
    n = dt(B) * dt(S) * dt(R)
    bce = E.sum(dtype=dtype) / n
    A, Bc = np.zeros((B, R), dtype), np.zeros((B, R), dtype)
    if batch:
        D, a, bc = _dice(I.sum(0, dtype=dtype), FP.sum(0, dtype=dtype), FN.sum(0, dtype=dtype), eps, dt)
        A[:], Bc[:] = dt(w_dice) / dt(R) * a, dt(w_dice) / dt(R) * bc
    else:
        v, a, bc = _dice(I, FP, FN, eps, dt)
        D = v.sum(0, dtype=dtype) / dt(B)
        A[:], Bc[:] = dt(w_dice) / (dt(R) * dt(B)) * a, dt(w_dice) / (dt(R) * dt(B)) * bc
    dice = D.sum(dtype=dtype) / dt(R)
    total = dt(w_bce) * bce + dt(w_dice) * dice
    g = None
    if grad:
        pf = np.asarray(p).reshape(B, S, R).astype(dtype)
        t = ((np.asarray(bits).reshape(B, S, 1).astype(np.int64) >> np.arange(R)) & 1).astype(bool)
        q = dt(1) - pf
        with np.errstate(divide='ignore'):
            e = np.where(t, np.where(pf > dt(CLAMP32), -dt(1) / np.where(pf > 0, pf, dt(1)), dt(0)),
                         np.where(q > dt(CLAMP32), dt(1) / np.where(q > 0, q, dt(1)), dt(0)))
        g = (A[:, None, :] + np.where(t, Bc[:, None, :], dt(0)) + dt(w_bce) / n * e).astype(dtype).reshape(p.shape)
    return dict(bce=bce, dice=dice, D=np.asarray(D, dtype), total=total, grad=g, sums=(I, FP, FN, E))


def report(r):
    """the stage's report [total, BCE, Dice, D_0 .. D_{R-1}] of an oracle result"""
    return np.array([r['total'], r['bce'], r['dice'], *r['D']], np.float64)


# ---------------------------------------------------------------------------------------------- tolerance
def allowed_scalar(v64, v32):
    """per number: max(4 |v32 - v64|, 4 ulps of the value)"""
    v64, v32 = np.asarray(v64, np.float64), np.asarray(v32, np.float64)
    return np.maximum(4.0 * np.abs(v32 - v64), 4.0 * np.spacing(np.abs(v64).astype(np.float32)).astype(np.float64))


def allowed_field(v64, v32):
    """a tensor compared as one quantity (a gradient): the largest absolute deviation over the largest |value|;
    -> max(4 x the float32 evaluation's, 4 ulps)"""
    return max(4.0 * field_error(v32, v64), 4.0 * ULP32)


def field_error(got, v64):
    v64 = np.asarray(v64, np.float64)
    m = float(np.abs(v64).max())
    return float(np.abs(np.asarray(got, np.float64) - v64).max()) / (m if m > 0 else 1.0)


def bf16_half_ulp(v):
    """half the spacing of bf16 (8 significant bits) at |v|: one rounding to bf16"""
    v = np.abs(np.asarray(v, np.float64))
    with np.errstate(divide='ignore'):
        e = np.floor(np.log2(np.where(v > 0, v, 1.0)))
    return np.where(v > 0, 2.0 ** (e - 8), 0.0)


def to_bf16(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


# ---------------------------------------------------------------------------------------------- labels and counts
def labels_ref(p, class_order, threshold=0.5):
    """p [B, R, ...] -> u8 [B, ...] by nnU-Net's rule, vectorised"""
    p = np.asarray(p)
    out = np.zeros((p.shape[0], *p.shape[2:]), np.uint8)
    for r, c in enumerate(class_order):
        out[p[:, r] > threshold] = c
    return out


def counts_ref(pred_bits, true_bits, R):
    """-> (TP, FP, FN) int64 [B, R], Dice float64 [B, R] (1 where both sides are empty)"""
    B = pred_bits.shape[0]
    a, t = np.asarray(pred_bits).reshape(B, -1).astype(np.int64), np.asarray(true_bits).reshape(B, -1).astype(np.int64)
    sh = np.arange(R).reshape(1, 1, R)
    ab, tb = ((a[..., None] >> sh) & 1).astype(bool), ((t[..., None] >> sh) & 1).astype(bool)
    TP, FP, FN = (ab & tb).sum(1), (ab & ~tb).sum(1), (~ab & tb).sum(1)
    den = 2 * TP + FP + FN
    return TP, FP, FN, np.where(den > 0, 2 * TP / np.where(den > 0, den, 1), 1.0)


def prob_bits_ref(p, threshold=0.5):
    """p [B, R, ...] -> u8 [B, ...], bit r = [p_r > threshold]"""
    p = np.asarray(p)
    out = np.zeros((p.shape[0], *p.shape[2:]), np.uint8)
    for r in range(p.shape[1]):
        out |= ((p[:, r] > threshold).astype(np.uint8) << r).astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------- inputs
def make_region_case(B, spatial, R, seed, members=None):
    """-> (p fp32 [B, *spatial, R] in (0, 1), label u8, bits u8, members): random probabilities and labels 0 .. R with a few stray
    values (200); default members: region r = labels {r + 1 .. R} (nested, as BraTS's)"""
    rng = np.random.default_rng(seed)
    members = members or tuple(tuple(range(r + 1, R + 1)) for r in range(R))
    p = rng.random((B, *spatial, R)).astype(np.float32)
    label = rng.integers(0, R + 1, (B, *spatial)).astype(np.uint8)
    label.reshape(-1)[rng.choice(label.size, min(5, label.size), replace=False)] = 200
    return p, label, bits_ref(label, members), members


def late_region_probs(bits, R, seed, confident=0.97, wrong=0.01):
    """Late in training: `confident` of the entries sit at exactly 0.0 or 1.0 on the correct side, `wrong` of them at exactly 0.0 or 1.0
    on the wrong side (confidently wrong), the rest random.  -> p fp32 [*bits.shape, R]"""
    rng = np.random.default_rng(seed)
    t = ((np.asarray(bits)[..., None].astype(np.int64) >> np.arange(R)) & 1).astype(np.float32)
    u = rng.random(t.shape)
    p = rng.random(t.shape).astype(np.float32)
    p = np.where(u < confident, t, p)
    p = np.where(u > 1.0 - wrong, 1.0 - t, p)
    return p.astype(np.float32)
