"""float64 restatement of the boundary loss (Kervadec et al., "Boundary loss for highly unbalanced segmentation") and the label
volumes its tests run on.  numpy + scipy only: shared by tests/test_boundary.py (CPU) and tests/test_gpu_boundary.py."""
import numpy as np
from scipy.ndimage import distance_transform_edt


def phi_ref(label, cls, spacing=(1.0, 1.0, 1.0)):
    """signed distance map of G = {label == cls} of one volume [H,W,D]: dist(x, G) outside G, -(dist(x, not G) - 1) inside (the 1
    is not scaled by the spacing: Kervadec's one_hot2dist), 0 everywhere when G is empty or fills the volume"""
    g = np.asarray(label) == cls
    if not g.any() or g.all():
        return np.zeros(g.shape, np.float64)
    sp = tuple(float(s) for s in spacing)
    return distance_transform_edt(~g, sampling=sp) * ~g - (distance_transform_edt(g, sampling=sp) - 1.0) * g


def phi_ref_batch(label, classes, spacing=(1.0, 1.0, 1.0)):
    """label [B,H,W,D] -> float64 [B,K,H,W,D]"""
    label = np.asarray(label)
    return np.stack([np.stack([phi_ref(label[b], c, spacing) for c in classes]) for b in range(label.shape[0])])


def boundary_values_ref(p, phi, classes):
    """p [B,*spatial,C] channels-last probabilities, phi [B,K,*spatial] -> value_k = mean over (b, s) of p[..., c_k] phi_k"""
    p = np.asarray(p, np.float64)
    phi = np.asarray(phi, np.float64)
    return np.array([(p[..., c] * phi[:, k]).mean() for k, c in enumerate(classes)])


def boundary_grad_ref(p_shape, phi, classes, weights, g=1.0):
    """dTotal/dp, channels-last: g w_k phi_k / (B S) in channel c_k, 0 elsewhere"""
    phi = np.asarray(phi, np.float64)
    dp = np.zeros(p_shape, np.float64)
    n = float(np.prod(p_shape[:-1]))
    for k, c in enumerate(classes):
        dp[..., c] += g * weights[k] * phi[:, k] / n
    return dp


def make_labels(shape, B=2, seed=0):
    """u8 [B,H,W,D] with classes 0 .. 3: boxes of classes 1 and 2, isolated single voxels (one at the last index of every axis), a
    3-D checkerboard region of classes 1 / 2 (every voxel an envelope apex), class 3 absent in sample 0 and filling sample 1"""
    H, W, D = shape
    rng = np.random.default_rng(seed)
    lab = np.zeros((B, H, W, D), np.uint8)
    for b in range(B):
        v = lab[b]
        if b == 1:
            v[...] = 3                          # class 3 fills the sample: every other class is absent there
            continue
        v[H // 8:H // 8 + max(1, H // 4), 0:max(1, W // 2), 0:max(1, D // 2)] = 1
        v[H // 2:H // 2 + max(1, H // 5), W // 3:, D // 3:] = 2
        h0, h1 = (3 * H) // 4, min(H, (3 * H) // 4 + 6)
        hh, ww, dd = np.meshgrid(np.arange(h0, h1), np.arange(W), np.arange(D), indexing='ij')
        v[h0:h1] = np.where((hh + ww + dd) % 2 == 0, 1, 2).astype(np.uint8)
        for _ in range(6):
            v[rng.integers(H), rng.integers(W), rng.integers(D)] = rng.integers(1, 3)
        v[H - 1, W - 1, D - 1] = 1
        v[0, W - 1, 0] = 2
    return lab
