"""Oracles of the soft morphology, the soft skeleton and soft-clDice (csrc/softmorph.hip), and the inputs their tests run on.
Shared by tests/test_cldice.py (CPU) and tests/test_gpu_cldice.py.

Two oracles, both run in float64 (and in float32 to size the allowance of a comparison):
  * `pub_*`: the published composition in torch (Shit et al.'s soft_erode / soft_dilate / soft_open / soft_skel over max_pool3d, with
    autograd), and the loss assembled from it with one term per named class;
  * `rule_*`: the stated rule in numpy - explicit taps in the stated order, the first that attains the extremum, and an explicit
    backward that gives the whole gradient of an output voxel to that tap.
On a tie-free input the two agree; on plateaus only the rule oracle says what the kernels do."""
import numpy as np
import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------------------------------- the published composition (torch)


def pub_erode(x):
    """x [N,1,H,W,D]"""
    p1 = -F.max_pool3d(-x, (3, 1, 1), (1, 1, 1), (1, 0, 0))
    p2 = -F.max_pool3d(-x, (1, 3, 1), (1, 1, 1), (0, 1, 0))
    p3 = -F.max_pool3d(-x, (1, 1, 3), (1, 1, 1), (0, 0, 1))
    return torch.min(torch.min(p1, p2), p3)


def pub_dilate(x):
    return F.max_pool3d(x, (3, 3, 3), (1, 1, 1), (1, 1, 1))


def pub_open(x):
    return pub_dilate(pub_erode(x))


def pub_skeleton(x, iters):
    img1 = pub_open(x)
    skel = F.relu(x - img1)
    for _ in range(iters):
        x = pub_erode(x)
        img1 = pub_open(x)
        delta = F.relu(x - img1)
        skel = skel + F.relu(delta - skel * delta)
    return skel


PUB_OPS = {'erode': lambda x, iters: pub_erode(x), 'dilate': lambda x, iters: pub_dilate(x), 'skeleton': pub_skeleton}


def pub_op(name, x, g, iters=None, dtype=torch.float64):
    """x, g numpy [N,H,W,D] -> (y, dx) of operator `name` under the upstream gradient g, as numpy float64"""
    xt = torch.from_numpy(np.asarray(x)).to(dtype).unsqueeze(1).requires_grad_(True)
    y = PUB_OPS[name](xt, iters)
    y.backward(torch.from_numpy(np.asarray(g)).to(dtype).unsqueeze(1))
    return y.detach()[:, 0].double().numpy(), xt.grad[:, 0].double().numpy()


def pub_label_skeletons(label, classes, iters):
    """label u8 [B,H,W,D] -> float64 [B,K,H,W,D], the published skeleton of the maps [label == c]"""
    lab = torch.from_numpy(np.asarray(label))
    return np.stack([pub_skeleton((lab == c).double().unsqueeze(1), iters)[:, 0].numpy() for c in classes], 1)


def pub_cldice(p, label, classes, weights, iters, dtype=torch.float64):
    """p [B,H,W,D,C], label [B,H,W,D] -> (total, values [K], dp) of sum_k w_k (1 - 2 Tprec Tsens / (Tprec + Tsens)), smooth 1, sums
    over the batch, one term per named class; numpy float64"""
    pt = torch.from_numpy(np.asarray(p)).to(dtype).requires_grad_(True)
    lab = torch.from_numpy(np.asarray(label))
    total, values = 0.0, []
    for c, w in zip(classes, weights):
        P = pt[..., c].unsqueeze(1)
        G = (lab == c).to(dtype).unsqueeze(1)
        SP, SG = pub_skeleton(P, iters), pub_skeleton(G, iters)
        tprec = ((SP * G).sum() + 1.0) / (SP.sum() + 1.0)
        tsens = ((SG * P).sum() + 1.0) / (SG.sum() + 1.0)
        v = 1.0 - 2.0 * (tprec * tsens) / (tprec + tsens)
        values.append(v.item())
        total = total + w * v
    total.backward()
    return total.item(), np.array(values), pt.grad.double().numpy()


# ---------------------------------------------------------------------------------------------- the stated rule (numpy)
ERODE_TAPS = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
DILATE_TAPS = [(0, 0, 0)] + [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


def _shifted(x, off, fill):
    """y[v] = x[v + off] inside the volume, `fill` outside; x [N,H,W,D]"""
    y = np.full_like(x, fill)
    src, dst = [slice(None)], [slice(None)]
    for o, n in zip(off, x.shape[1:]):
        if abs(o) >= n:
            return y
        src.append(slice(max(o, 0), n + min(o, 0)))
        dst.append(slice(max(-o, 0), n + min(-o, 0)))
    y[tuple(dst)] = x[tuple(src)]
    return y


def rule_morph(x, dilate):
    """-> (y, tap): the extremum over the taps in the stated order, tap = index into the tap list of the first that attains it"""
    taps, sign = (DILATE_TAPS, 1.0) if dilate else (ERODE_TAPS, -1.0)
    best = x.copy()
    tap = np.zeros(x.shape, np.int64)
    for t, off in enumerate(taps[1:], 1):
        v = _shifted(x, off, -np.inf * sign)
        better = v > best if dilate else v < best          # strictly: an earlier tap keeps a tie
        best = np.where(better, v, best)
        tap = np.where(better, t, tap)
    return best, tap


def rule_morph_bwd(g, tap, dilate):
    """the whole gradient of an output voxel to its tap"""
    taps = DILATE_TAPS if dilate else ERODE_TAPS
    dx = np.zeros_like(g)
    idx = np.indices(g.shape)
    for t, off in enumerate(taps):
        m = tap == t
        tgt = [idx[0][m]] + [idx[a + 1][m] + off[a] for a in range(3)]
        np.add.at(dx, tuple(tgt), g[m])
    return dx


def rule_skeleton(x, g, iters, dtype=np.float64):
    """x, g [N,H,W,D] -> (s, dx, masks): the skeleton, its gradient under the upstream g, and the relu masks [I_j > D_j] and
    [delta_j - s_{j-1} delta_j > 0] of every iteration (the latter from j = 1)"""
    x = np.asarray(x, dtype)
    I, tapE, tapD, delta, r, m, sk = [x], [], [], [], [], [None], []
    for j in range(iters + 1):
        nxt, te = rule_morph(I[j], False)
        D, td = rule_morph(nxt, True)
        diff = I[j] - D
        I.append(nxt); tapE.append(te); tapD.append(td)
        r.append(diff > 0)
        delta.append(np.where(diff > 0, diff, 0).astype(dtype))
        if j == 0:
            sk.append(delta[0])
        else:
            u = delta[j] - sk[j - 1] * delta[j]
            m.append(u > 0)
            sk.append(sk[j - 1] + np.where(u > 0, u, 0).astype(dtype))
    gs = np.asarray(g, dtype)
    e = [None] * (iters + 1)
    for j in range(iters, 0, -1):
        e[j] = np.where(m[j] & r[j], gs - gs * sk[j - 1], 0).astype(dtype)
        gs = np.where(m[j], gs - gs * delta[j], gs).astype(dtype)
    e[0] = np.where(r[0], gs, 0).astype(dtype)
    G = rule_morph_bwd(-e[iters], tapD[iters], True)             # gradient of I_{iters+1}
    for k in range(iters, -1, -1):
        G = e[k] + rule_morph_bwd(G, tapE[k], False)
        if k > 0:
            G = G + rule_morph_bwd(-e[k - 1], tapD[k - 1], True)
    return sk[iters], G.astype(dtype), r + m[1:]


def rule_cldice(p, label, classes, weights, iters, dtype=np.float64):
    """as pub_cldice, from the rule oracle -> (total, values [K], dp, masks)"""
    p = np.asarray(p, dtype)
    label = np.asarray(label)
    dp = np.zeros(p.shape, dtype)
    total, values, masks = dtype(0), [], []
    for c, w in zip(classes, weights):
        P = p[..., c]
        G = (label == c).astype(dtype)
        SG = rule_skeleton(G, np.zeros_like(G), iters, dtype)[0]
        SP = rule_skeleton(P, np.zeros_like(P), iters, dtype)[0]
        A, Bs, Cc, Dd = (SP * G).sum(dtype=dtype), SP.sum(dtype=dtype), (SG * P).sum(dtype=dtype), SG.sum(dtype=dtype)
        tp, ts = (A + 1) / (Bs + 1), (Cc + 1) / (Dd + 1)
        v = 1 - 2 * tp * ts / (tp + ts)
        dtp, dts = -2 * ts * ts / (tp + ts) ** 2, -2 * tp * tp / (tp + ts) ** 2
        seed = (w * dtp / (Bs + 1)) * G + (-w * dtp * tp / (Bs + 1))
        _, dP, mk = rule_skeleton(P, seed.astype(dtype), iters, dtype)
        dp[..., c] = dP + (w * dts / (Dd + 1)) * SG
        values.append(float(v)); masks += mk
        total = total + dtype(w) * v
    return float(total), np.array(values), dp.astype(np.float64), masks


# ---------------------------------------------------------------------------------------------- allowances
ULP32 = 2.0 ** -23


def value_allowance(v64, v32):
    """4 x the deviation of the float32 oracle from the float64 one, at least 4 fp32 ulps of the value"""
    return max(4.0 * abs(v32 - v64), 4.0 * ULP32 * abs(v64))


def field_error(got, want):
    """largest |difference| over the largest |want|"""
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def field_allowance(f64, f32):
    """as value_allowance for a field (gradient, skeleton), relative to its largest magnitude: at least 4 ulps of that"""
    return max(4.0 * field_error(f32, f64), 4.0 * ULP32)


# ---------------------------------------------------------------------------------------------- inputs
SHAPES = [(2, (12, 10, 8)), (1, (9, 7, 5)), (1, (37, 22, 70)), (1, (1, 5, 3))]


def noise(shape, seed):
    """fp32 values spread over (0.02, 0.98), all different: a tie-free input.  (Independent uniform draws collide in fp32 at the
    larger shapes, so the values are a shuffled jittered grid.)"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = (0.02 + 0.96 * (rng.permutation(n) + rng.uniform(0.25, 0.75, n)) / n).astype(np.float32)
    assert np.unique(x).size == n
    return x.reshape(shape)


def noise_probs(B, spatial, C, seed):
    """p fp32 [B, *spatial, C]: every channel tie-free noise (the stage reads channels one by one; rows need not sum to 1)"""
    return np.stack([noise((B,) + tuple(spatial), seed + 17 * c) for c in range(C)], -1)


def blob_labels(B, spatial, C, seed):
    """u8 [B, *spatial]: class c > 0 is a union of a few boxes and a thin line each, class 0 the rest"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((B,) + tuple(spatial), np.uint8)
    for b in range(B):
        for c in range(1, C):
            for _ in range(3):
                lo = [int(rng.integers(0, n)) for n in spatial]
                ext = [int(rng.integers(1, max(2, n // 2 + 1))) for n in spatial]
                lab[b][tuple(slice(l, l + e) for l, e in zip(lo, ext))] = c
            h, w = (int(rng.integers(0, n)) for n in spatial[:2])
            lab[b, h, w, :] = c
    return lab


def plateau_case(seed=0):
    """p fp32 [1,14,12,16,3], label u8: channel 1 holds exact 0.0 / 1.0 regions - a tube one, two and three voxels thick, a slab,
    an isolated voxel - with a soft rim (values in (0, 1), multiples of 1/8) on part of them; channel 2 a 0 / 1 box; channel 0
    the rest.  The label follows channel 1 > 0.5 shifted by one voxel, so that prediction and label overlap in part."""
    H, W, D = 14, 12, 16
    a = np.zeros((H, W, D), np.float32)
    a[2, 2, 1:15] = 1.0                       # tube, one voxel thick
    a[5:7, 2:4, 1:15] = 1.0                   # two thick
    a[9:12, 1:4, 2:14] = 1.0                  # three thick
    a[1:13, 7, 3:13] = 1.0                    # slab
    a[3, 10, 8] = 1.0                         # isolated voxel
    a[4, 2:4, 1:9] = 0.5                      # soft rim on part of the two-thick tube
    a[8, 1:4, 2:9] = 0.25
    a[1:7, 8, 3:13] = 0.625                   # and on part of the slab
    b = np.zeros((H, W, D), np.float32)
    b[6:10, 9:11, 4:9] = 1.0
    p = np.stack([np.clip(1.0 - a - b, 0.0, 1.0), a, b], -1)[None].astype(np.float32)
    lab = np.zeros((1, H, W, D), np.uint8)
    lab[0][np.roll(a, 1, 2) > 0.5] = 1
    lab[0][(b > 0.5) & (lab[0] == 0)] = 2
    return p, lab
