"""float64 restatement of the top-k cross-entropy (nnU-Net's TopKLoss with the symmetric tie rule of csrc/loss_topk.hip) and the
inputs its tests run on.  numpy only: shared by tests/test_topk.py (CPU) and tests/test_gpu_topk.py."""
import math

import numpy as np

CLAMP = float(np.float32(1e-6))        # the kernels clamp at the fp32 constant


def count_ref(frac, N):
    """k = min(max(floor(frac N), 1), N) with frac taken as fp32 and the product formed in double"""
    f = float(np.float32(frac))
    if not math.isfinite(f):
        return int(N)
    return int(min(max(math.floor(f * N), 1), N))


def voxel_losses_ref(p, label):
    """p [..., C] channels-last probabilities, label [...] -> (l float64 [N], p_label float64 [N], valid [N]): l = -log(max(p[label],
    1e-6)), 0 where label >= C"""
    p = np.asarray(p, np.float64)
    C = p.shape[-1]
    lab = np.asarray(label).reshape(-1).astype(np.int64)
    flat = p.reshape(-1, C)
    valid = lab < C
    pl = np.where(valid, flat[np.arange(lab.size), np.minimum(lab, C - 1)], 1.0)
    l = np.where(valid, -np.log(np.maximum(pl, CLAMP)), 0.0)
    return l + 0.0, pl, valid                                      # + 0.0: -0.0 -> 0.0


def topk_ref(p, label, k):
    """-> dict(value, tau, k, n_gt, n_eq, grad [shape of p], l [N]): value = (sum_{l > tau} l + (k - n_gt) tau) / k with tau the
    k-th largest l over the whole batch; grad = weight * (-1 / p) in channel label where p >= 1e-6, weight = 1 / k above tau,
    (k - n_gt) / (n_eq k) on it, 0 below it; no gradient where label >= C"""
    p = np.asarray(p, np.float64)
    C = p.shape[-1]
    l, pl, valid = voxel_losses_ref(p, label)
    N = l.size
    assert 1 <= k <= N
    tau = np.partition(l, N - k)[N - k]
    gt, eq = l > tau, l == tau
    n_gt, n_eq = int(gt.sum()), int(eq.sum())
    assert n_gt < k <= n_gt + n_eq
    value = (l[gt].sum() + (k - n_gt) * tau) / k
    weight = np.where(gt, 1.0 / k, np.where(eq, (k - n_gt) / (n_eq * k), 0.0))
    dl = np.where(valid & (pl >= CLAMP), -1.0 / np.where(pl > 0, pl, 1.0), 0.0)
    grad = np.zeros((N, C), np.float64)
    lab = np.asarray(label).reshape(-1).astype(np.int64)
    idx = np.nonzero(valid)[0]
    grad[idx, lab[idx]] = (weight * dl)[idx]
    return dict(value=float(value), tau=float(tau), k=int(k), n_gt=n_gt, n_eq=n_eq, grad=grad.reshape(p.shape), l=l)


# ---------------------------------------------------------------------------------------------- inputs
def make_probs(B, spatial, C, seed):
    """softmax(1.5 randn) made in float64, cast to fp32: [B, *spatial, C] channels-last"""
    rng = np.random.default_rng(seed)
    z = 1.5 * rng.standard_normal((B,) + tuple(spatial) + (C,))
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def make_labels(B, spatial, C, seed):
    """uniform labels 0 .. C-1, u8 [B, *spatial]"""
    return np.random.default_rng(seed).integers(0, C, (B,) + tuple(spatial)).astype(np.uint8)


def set_label_prob(p, label, values):
    """p with p[label] replaced by `values` [B, *spatial] and the rest of each voxel sharing 1 - value equally (fp32)"""
    p = np.array(p, np.float32)
    C = p.shape[-1]
    v = np.asarray(values, np.float32)
    out = np.repeat(((1.0 - v.astype(np.float64)) / (C - 1))[..., None], C, -1).astype(np.float32)
    np.put_along_axis(out, np.asarray(label).astype(np.int64)[..., None], v[..., None], -1)
    return out


def tied_probs(B, spatial, C, seed):
    """labels and probabilities whose p[label] is drawn from {1, 1/2, 1/4, 1/8}: l ties exactly in four groups.
    -> (p fp32, label u8, group index [B, *spatial] with 0: p = 1 ... 3: p = 1/8)"""
    rng = np.random.default_rng(seed)
    lab = make_labels(B, spatial, C, seed + 1)
    grp = rng.integers(0, 4, lab.shape)
    p = set_label_prob(np.zeros(lab.shape + (C,), np.float32), lab, np.float32(0.5) ** grp.astype(np.float32))
    return p, lab, grp
