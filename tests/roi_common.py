"""CPU helpers of tests/test_roi_sweep.py and tests/test_gpu_roi_sweep.py: a seeded family of probability maps that reaches every
branch of the ROI box finder and of the warp index maps (csrc/roi.hip: roi_hist_kernel, roi_plan_kernel), the scalar float32
replay of the two maps in the reference's operation order, and the taps F.grid_sample derives from a coordinate.  No GPU, no
library.

A case is one sample: a target mask of some kind, turned into class probabilities whose channel 0 puts `1 - p0` (float32) on,
beside or far from the threshold.  The kernels' contract is foreground = (1 - prob[..., 0] in float32) >= thr with NaN background;
`reference_mask` is that expression evaluated by torch.  Cases come in batches of 8 of one geometry, class count and threshold:
one ops.RoiPlan call each."""
import numpy as np
import torch

F32 = np.float32

# (H, W, D, roi_size)
GEOMETRIES = (
    (40, 36, 4, 20),     # the geometry of tests/golden/roi.npz
    (33, 47, 3, 16),     # eval_h = 19 and eval_w = 11 are odd: the back plans' source length 2 ceil(eval / 2) differs from eval
    (16, 16, 8, 40),     # image smaller than the ROI grid: min_len > full, both rules always fire
    (64, 24, 5, 12),     # H much larger than W
    (23, 61, 2, 9),      # eval_w - w_roi = 1
    (96, 80, 2, 25),     # larger image
    (61, 53, 7, 20),     # 22 631 voxels: 5 histogram blocks of 4 527 voxels, no multiple of a row of 371
    (20, 11, 3, 20),     # min_len <= full < 2 min_len on both axes: a padded extent exceeds full - min_len where the original did not
)
KINDS = (
    'box', 'box', 'box', 'small', 'big', 'pin_h0', 'pin_h1', 'pin_w0',
    'pin_w1', 'tiny_h0', 'tiny_h1', 'tiny_w0', 'tiny_w1', 'box_out', 'box_out', 'box_out',
    'out', 'out', 'out', 'empty', 'full', 'body_out', 'body_out', 'exact1000',
)
PKINDS = ('hard', 'edge', 'ulp', 'random', 'nan')
BATCH = 8
N_BATCH = len(KINDS) // BATCH            # batch j of a geometry holds the kinds j, j + 3, j + 6, ...: every batch mixes kinds
CLASSES = (2, 3, 8)
THR_DEFAULT = 0.5
THR_OTHER = (0, 2, 0.3)                  # (geometry, batch, thr): the one batch at a non-default threshold
SEED = 20261020


def roi_sizes(roi_size):
    """oracle.roi.roi_geometry restated (Unet_3Dblock.py:695-715), so that this module needs no import of the oracle"""
    eval_h = int(1.2 * roi_size)
    eval_w = int(eval_h * 0.6)
    return dict(h_roi=roi_size, w_roi=int(roi_size * 0.6), eval_h=eval_h, eval_w=eval_w, min_h=eval_h // 2, min_w=eval_w // 2)


# ---------------------------------------------------------------------------------------------- masks

def _span(rs, full, lo, hi):
    """a random extent [a, a + n) inside [0, full) with lo <= n <= hi"""
    lo = max(1, min(lo, full))
    n = int(rs.randint(lo, max(lo, min(hi, full)) + 1))
    return int(rs.randint(0, full - n + 1)), n


def _outliers(rs, m, avoid=None):
    """1-3 single voxels, outside the box `avoid` = (a, h, b, w) on both axes where the image leaves room"""
    H, W, D = m.shape
    for _ in range(int(rs.randint(1, 4))):
        for _ in range(64):
            r, c = int(rs.randint(0, H)), int(rs.randint(0, W))
            if avoid is None or (not avoid[0] - 1 <= r <= avoid[0] + avoid[1] and not avoid[2] - 1 <= c <= avoid[2] + avoid[3]):
                break
        m[r, c, int(rs.randint(0, D))] = True


def make_mask(rs, kind, H, W, D, geo):
    """target foreground, bool [H, W, D]"""
    m = np.zeros((H, W, D), bool)
    mh, mw = geo['min_h'], geo['min_w']

    def fill(a, h, b, w):
        m[a:a + h, b:b + w, :] = rs.rand(h, w, D) < (1.0 if rs.rand() < 0.5 else 0.5)

    if kind == 'box':                                      # anything from a few rows to most of the image
        (a, h), (b, w) = _span(rs, H, 2, H), _span(rs, W, 2, W)
        fill(a, h, b, w)
    elif kind == 'small':                                  # shorter than min_len: the pad rule
        (a, h), (b, w) = _span(rs, H, 1, max(1, mh - 1)), _span(rs, W, 1, max(1, mw - 1))
        m[a:a + h, b:b + w, :] = True
    elif kind == 'big':                                    # longer than full - min_len: the shrink rule
        (a, h), (b, w) = _span(rs, H, H - mh + 2, H), _span(rs, W, W - mw + 2, W)
        m[a:a + h, b:b + w, :] = True
    elif kind.startswith('pin_') or kind.startswith('tiny_'):
        tiny = kind.startswith('tiny_')
        (a, h) = _span(rs, H, 1, max(1, mh // 2)) if tiny else _span(rs, H, 2, H - 1)
        (b, w) = _span(rs, W, 1, max(1, mw // 2)) if tiny else _span(rs, W, 2, W - 1)
        if kind.endswith('h0'): a = 0
        if kind.endswith('h1'): a = H - h
        if kind.endswith('w0'): b = 0
        if kind.endswith('w1'): b = W - w
        if tiny:
            m[a:a + h, b:b + w, :] = True
        else:
            fill(a, h, b, w)
    elif kind == 'box_out' or (kind == 'body_out' and body_extent(H, W, D, geo) is None) or (kind == 'exact1000' and (H - 2) * (W - 2) * D < 998):
        (a, h), (b, w) = _span(rs, H, 2, max(2, H // 2)), _span(rs, W, 2, max(2, W // 2))
        fill(a, h, b, w)
        _outliers(rs, m, (a, h, b, w))
    elif kind == 'out':
        _outliers(rs, m)
    elif kind == 'empty':
        pass
    elif kind == 'full':
        m[:] = True
    elif kind == 'body_out':
        # more than 3000 voxels in a dense body that neither rule touches (min_len <= extent <= full - min_len), and 1-2 single
        # voxels beyond it on every side: below 0.1 % of the total, so lo and hi both land on the body, inside the outliers' span
        h, w = body_extent(H, W, D, geo)
        a, b = int(rs.randint(2, H - h - 1)), int(rs.randint(2, W - w - 1))
        m[a:a + h, b:b + w, :] = True
        for _ in range(int(rs.randint(1, 3))):
            m[int(rs.randint(0, a - 1)), int(rs.randint(0, b - 1)), int(rs.randint(0, D))] = True
            m[int(rs.randint(a + h + 1, H)), int(rs.randint(b + w + 1, W)), int(rs.randint(0, D))] = True
    elif kind == 'exact1000':
        # exactly 1000 voxels: one in the first and one in the last occupied row and column, 998 strictly between.  The cumulative
        # ratio of the first row is then fdiv(1, 1000) = 0.001f itself (>= must hold) and that of the row before the last is
        # fdiv(999, 1000) = 0.999f itself (> must not hold)
        for _ in range(256):
            r0, nr = _span(rs, H, max(3, mh + 1), max(3, H - mh + 1))
            c0, nc = _span(rs, W, max(3, mw + 1), max(3, W - mw + 1))
            if (nr - 2) * (nc - 2) * D >= 998:
                break
        else:
            r0, nr, c0, nc = 0, H, 0, W
        inner = np.zeros((nr - 2) * (nc - 2) * D, bool)
        inner[rs.permutation(inner.size)[:998]] = True
        m[r0 + 1:r0 + nr - 1, c0 + 1:c0 + nc - 1, :] = inner.reshape(nr - 2, nc - 2, D)
        m[r0, c0, int(rs.randint(0, D))] = True
        m[r0 + nr - 1, c0 + nc - 1, int(rs.randint(0, D))] = True
        assert m.sum() == 1000
    else:
        raise ValueError(kind)
    return m


def body_extent(H, W, D, geo):
    """(rows, columns) of the body of a 'body_out' mask, or None where the image cannot hold more than 3000 voxels that way"""
    h, w = min(H - geo['min_h'], H - 4), min(W - geo['min_w'], W - 4)
    if h < geo['min_h'] + 1 or w < geo['min_w'] + 1 or h * w * D <= 3000:
        return None
    return h, w


# ---------------------------------------------------------------------------------------------- probabilities

def fg_of_p0(p0, thr):
    """the kernels' contract on channel 0 (float32 array): (1 - p0 in float32) >= thr, NaN is background"""
    with np.errstate(invalid='ignore'):
        return (F32(1) - p0.astype(F32)) >= F32(thr)


def threshold_neighbours(thr):
    """p0 values (float32) whose float32 `1 - p0` is exactly thr, the smallest reachable value above it and the largest reachable
    value below it.  Above 0.5 that is one ulp away; just below 0.5 the spacing of p0 (in [0.5, 1)) is twice that of 1 - p0, so
    the nearest value some p0 reaches is one ulp of p0 away"""
    t = F32(thr)
    q = F32(F32(1) - t)
    cands = [q]
    for _ in range(6):
        cands = [np.nextafter(cands[0], F32(-1))] + cands + [np.nextafter(cands[-1], F32(2))]
    cands = np.array(cands, F32)
    fg = F32(1) - cands
    at = cands[fg == t]
    above = cands[fg > t]
    below = cands[fg < t]
    assert len(at) and len(above) and len(below), thr
    return at[0], above[np.argmin(F32(1) - above)], below[np.argmax(F32(1) - below)]


def make_prob(rs, mask, C, thr, pkind):
    """class probabilities float32 [H, W, D, C] whose channel 0 realises `mask` under the contract (except the 'nan' kind's
    few NaN voxels, which are background whatever the mask says)"""
    at, above, below = threshold_neighbours(thr)
    t = float(F32(thr))
    u = rs.rand(*mask.shape)
    if pkind == 'hard':
        p0 = np.where(mask, 0.0, 1.0)
    elif pkind == 'edge':                                  # foreground exactly on the threshold, background just below it
        p0 = np.where(mask, at, below)
    elif pkind == 'ulp':                                   # just above / just below
        p0 = np.where(mask, above, below)
    else:                                                  # anywhere on the right side, a third of the voxels on or beside the threshold
        far = np.where(mask, (1 - t) * u, (1 - t) + t * u)
        near = np.where(mask, np.where(u < 0.5, at, above), below)
        p0 = np.where(rs.rand(*mask.shape) < 1 / 3, near, far)
        p0 = np.where(mask & ~fg_of_p0(p0.astype(F32), thr), at, p0)          # roundings of `far` that crossed the threshold
        p0 = np.where(~mask & fg_of_p0(p0.astype(F32), thr), below, p0)
    p0 = p0.astype(F32)
    if pkind == 'nan':
        p0[rs.rand(*mask.shape) < 0.02] = np.nan
    rest = rs.rand(*mask.shape, C - 1) + 1e-3
    rest = rest / rest.sum(-1, keepdims=True) * (1 - np.nan_to_num(p0.astype(np.float64), nan=0.5))[..., None]
    return np.concatenate((p0[..., None], rest.astype(F32)), -1)


def reference_mask(prob, thr):
    """the contract, evaluated by torch on the CPU: bool [B, 1, H, W, D] from prob [B, H, W, D, C] (float32)"""
    fg = torch.ones((), dtype=torch.float32) - prob[..., 0]
    assert fg.dtype == torch.float32
    return (fg >= torch.tensor(thr, dtype=torch.float32))[:, None]


# ---------------------------------------------------------------------------------------------- the family

def case_seed(g, k):
    return SEED + 1000 * g + k


def make_case(g, k, C, thr, geometry=None, kind=None, pkind=None):
    """(target mask bool [H, W, D], prob float32 [H, W, D, C]) of case k of geometry g"""
    H, W, D, roi_size = geometry or GEOMETRIES[g]
    kind = kind or KINDS[k]
    pkind = pkind or ('edge' if kind == 'exact1000' else PKINDS[(g + k) % len(PKINDS)])
    rs = np.random.RandomState(case_seed(g, k))
    mask = make_mask(rs, kind, H, W, D, roi_sizes(roi_size))
    return mask, make_prob(rs, mask, C, thr, pkind)


def batches():
    """[(g, j, case indices k, C, thr)]: every geometry in N_BATCH batches of BATCH cases"""
    out = []
    for g in range(len(GEOMETRIES)):
        for j in range(N_BATCH):
            thr = THR_OTHER[2] if (g, j) == THR_OTHER[:2] else THR_DEFAULT
            out.append((g, j, tuple(range(j, len(KINDS), N_BATCH)), CLASSES[(g + j) % len(CLASSES)], thr))
    return out


def make_batch(g, ks, C, thr):
    """prob float32 tensor [B, H, W, D, C] of the cases ks of geometry g"""
    return torch.from_numpy(np.stack([make_case(g, k, C, thr)[1] for k in ks]))


# ---------------------------------------------------------------------------------------------- float32 replay of the maps

def _f(x):
    return np.asarray(x, dtype=F32)


def replay_fwd(x0, x1, span, roi, eval_roi):
    """csrc/roi.hip map_fwd for idx = 0 .. eval_roi - 1: Unet_3Dblock.py:51-64, one float32 rounding per operation"""
    idx = np.arange(eval_roi, dtype=F32)
    x0, x1, span_f = _f(x0), _f(x1), _f(span)
    k2 = (x1 - x0) / _f(roi - 1)
    k1 = ((span_f - x1) + x0) / _f(eval_roi - roi)
    pos = idx * k2 + x0 * (_f(1) - k2 / k1)
    r = k1 / k2
    pos = np.where(pos <= x0, pos * r + x0 * (_f(1) - r), pos)
    pos = np.where(pos >= x1, pos * r + x1 * (_f(1) - r), pos)
    out = pos * _f(2) / span_f - _f(1)
    assert out.dtype == F32
    return out


def replay_back(x0, x1, span, roi, eval_roi, single_division=False):
    """csrc/roi.hip map_back for idx = 0 .. span: Unet_3Dblock.py:66-82.  Lines 69-70 divide a Python int by a tensor, which torch
    evaluates as tensor.reciprocal() * int: the two slopes are a reciprocal and a product (two roundings), every other quotient
    one division.  single_division=True is the variant that rounds the slopes once (not the reference's)"""
    idx = np.arange(span + 1, dtype=F32)
    x0, x1, span_f, ev = _f(x0), _f(x1), _f(span), _f(eval_roi)
    if single_division:
        k2 = _f(roi) / (x1 - x0)
        k1 = _f(eval_roi - roi) / ((span_f - x1) + x0)
    else:
        k2 = _f(roi) * (_f(1) / (x1 - x0))
        k1 = _f(eval_roi - roi) * (_f(1) / ((span_f - x1) + x0))
    p0 = x0 * k1
    p1 = ev - (span_f - x1) * k1
    pos = idx * k2 + p0 * (_f(1) - k2 / k1)
    r = k1 / k2
    pos = np.where(pos <= p0, pos * r + p0 * (_f(1) - r), pos)
    pos = np.where(pos >= p1, pos * r + p1 * (_f(1) - r), pos)
    out = pos * _f(2) / ev - _f(1)
    assert out.dtype == F32
    return out


# ---------------------------------------------------------------------------------------------- grid_sample taps

def taps_f32(g, size):
    """what F.grid_sample (bilinear, zeros padding, align_corners=True) makes of the normalised float32 coordinates g along an axis
    of `size` samples, in float32: (src0 int64, w0, w1 float32).  ix = ((g + 1) / 2) (size - 1), taps floor(ix) and floor(ix) + 1 with
    weights (fl + 1) - ix and ix - fl; a tap outside the source carries weight 0"""
    g = _f(g)
    ix = ((g + _f(1)) / _f(2)) * _f(size - 1)
    fl = np.floor(ix)
    w0 = (fl + _f(1)) - ix
    w1 = ix - fl
    inside0 = (fl >= 0) & (fl <= size - 1)
    inside1 = (fl + 1 >= 0) & (fl + 1 <= size - 1)
    w0 = np.where(inside0, w0, _f(0))
    w1 = np.where(inside1, w1, _f(0))
    assert w0.dtype == F32 and w1.dtype == F32
    return np.where(inside0 | inside1, fl, 0).astype(np.int64), w0, w1


def dense_f64(g, size):
    """the same taps from the same float32 coordinates, every operation in float64: [len(g)][size]"""
    g = np.asarray(g, dtype=F32).astype(np.float64)
    ix = ((g + 1) / 2) * (size - 1)
    fl = np.floor(ix)
    A = np.zeros((len(g), size))
    for i in range(len(g)):
        for tap, w in ((int(fl[i]), fl[i] + 1 - ix[i]), (int(fl[i]) + 1, ix[i] - fl[i])):
            if 0 <= tap <= size - 1:
                A[i, tap] += w
    return A


def tap_bound(size):
    """|A_kernel - A_float64| per entry: ix = ((g + 1) / 2) (size - 1) carries three float32 roundings of values up to `size`, and the
    weights one more: 4 * 2^-24 * size"""
    return 4 * 2.0 ** -24 * size


def widen(A):
    """0 / 1 support of A widened by one source index either way: where a float32 tap may put weight"""
    S = (np.asarray(A) != 0).astype(np.float64)
    W = S.copy()
    W[..., 1:] += S[..., :-1]
    W[..., :-1] += S[..., 1:]
    return (W > 0).astype(np.float64)
