"""Oracles of the intensity augmentations (lintransunet_amd/data.py: contrast, gamma_transform, simulate_lowres, patch_stats), written
from the formulas alone.  Every oracle takes one (patch, channel) volume x [H][W][D] and a dtype: np.float64 is the specification,
np.float32 is the same formula evaluated in float32 the way a float32 implementation may (the statistics of float32 values taken
in float64 and rounded, t^g formed as exp2(g * log2 t) in float32, one rounding per product and per sum).  The GPU tests allow
4 x the largest deviation of the float32 evaluation from the float64 one on their own inputs (`tolerance`): the kernels may fuse
and order their float32 operations differently, the margin the spline and sampler tests use."""
import numpy as np

EPS = 1e-7


def stats(x):
    """{min, max, sum, sum of squares} of a float32 volume, the sums in float64"""
    v = np.asarray(x, dtype=np.float64).ravel()
    return np.array([v.min(), v.max(), v.sum(), (v * v).sum()])


def contrast(x, f, dtype=np.float64):
    x = np.asarray(x)
    m = dtype(np.asarray(x, dtype=np.float64).mean())
    v = x.astype(dtype)
    return np.clip((v - m) * dtype(f) + m, v.min(), v.max())


def gamma(x, g, invert=False, retain_stats=True, dtype=np.float64):
    x = np.asarray(x)
    u = (-x if invert else x).astype(dtype)
    lo = u.min()
    r = u.max() - lo
    if r == 0:                                       # a constant volume comes back unchanged
        return x.astype(dtype)
    t = (u - lo) / max(r, dtype(EPS))
    if dtype is np.float32:
        with np.errstate(divide='ignore'):
            pw = np.exp2(np.float32(g) * np.log2(t))          # t = 0: log2 = -inf, exp2 = 0
        assert pw.dtype == np.float32
    else:
        pw = t ** g
    v = pw * r + lo
    if retain_stats:
        u64, v64 = u.astype(np.float64), v.astype(np.float64)
        a = u64.std() / max(v64.std(), EPS)
        v = (v - dtype(v64.mean())) * dtype(a) + dtype(u64.mean())
    assert v.dtype == dtype
    return -v if invert else v


def lowres_axis(S, scale, on=True):
    """one axis of extent S: (S', i0, i1, lam) - the high-resolution indices of the lower and the upper tap and the float64 weight of
    the upper one, per output index"""
    Sl = max(int(round(S * scale)), 1) if on else S
    i0, i1, lam = [], [], []
    for o in range(S):
        src = max((o + 0.5) * Sl / S - 0.5, 0.0)
        j0 = min(int(np.floor(src)), Sl - 1)
        j1 = min(j0 + 1, Sl - 1)
        lam.append(0.0 if j0 == j1 else src - j0)
        i0.append(min(((2 * j0 + 1) * S) // (2 * Sl), S - 1))
        i1.append(min(((2 * j1 + 1) * S) // (2 * Sl), S - 1))
    return Sl, np.array(i0), np.array(i1), np.array(lam, dtype=np.float64)


def lowres_tables(size, scale, axes=(0, 1, 2)):
    """what data.lowres_tables returns: (int32 [2][H + W + D], float32 [H + W + D])"""
    ax = [lowres_axis(S, scale, a in axes) for a, S in enumerate(size)]
    idx = np.stack([np.concatenate([a[1] for a in ax]), np.concatenate([a[2] for a in ax])]).astype(np.int32)
    return idx, np.concatenate([a[3] for a in ax]).astype(np.float32)


def lowres(x, scale, axes=(0, 1, 2), dtype=np.float64):
    """trilinear_up(nearest_exact_down(x)) as the 8-tap sum with weights (1 - lam | lam) per axis; float32: the weights from the
    float32 lam, w = (wx wy) wz, the taps added in the order x, y, z (z fastest), a tap of weight 0 left out"""
    x = np.asarray(x)
    v = x.astype(dtype)
    tabs = [lowres_axis(S, scale, a in axes) for a, S in enumerate(x.shape)]
    lam = [t[3].astype(np.float32).astype(dtype) if dtype is np.float32 else t[3] for t in tabs]
    one = dtype(1.0)
    out = None
    for bx in (0, 1):
        for by in (0, 1):
            for bz in (0, 1):
                ix, iy, iz = tabs[0][1 + bx], tabs[1][1 + by], tabs[2][1 + bz]
                wx = lam[0] if bx else one - lam[0]
                wy = lam[1] if by else one - lam[1]
                wz = lam[2] if bz else one - lam[2]
                w = (wx[:, None, None] * wy[None, :, None]) * wz[None, None, :]
                tap = v[np.ix_(ix, iy, iz)]
                if out is None:
                    out = w * tap
                else:
                    out = np.where(w != 0, out + w * tap, out)
    assert out.dtype == dtype
    return out


def chain(x, p, retain_stats, axes=(0, 1, 2), dtype=np.float64):
    """data._augmented's intensity stages on one volume under one Augmentation.draw dict p: contrast, low resolution, inverted gamma,
    gamma.  In float32 every stage hands a float32 volume to the next, as the device does"""
    v = np.asarray(x, dtype=np.float32)
    cast = (lambda a: a.astype(np.float32)) if dtype is np.float32 else (lambda a: a)
    if dtype is not np.float32:
        v = v.astype(np.float64)
    if p.get('scale_contrast'):
        v = cast(contrast(v, p['contrast_factor'], dtype))
    if p.get('lowres'):
        v = cast(lowres(v, p['lowres_scale'], axes, dtype))
    if p.get('invgamma'):
        v = cast(gamma(v, p['invgamma_g'], True, retain_stats, dtype))
    if p.get('contrast'):
        v = cast(gamma(v, p['gamma'], False, retain_stats, dtype))
    return v


def tolerance(ref64, ref32):
    """(allowed deviation from the float64 oracle, the measured deviation of the float32 evaluation): 4 x the maximum over every voxel"""
    dev = float(np.abs(np.asarray(ref32, dtype=np.float64) - np.asarray(ref64, dtype=np.float64)).max())
    return 4.0 * dev, dev


def volumes(size, seed=0):
    """the GPU tests' inputs [3][H][W][D] float32: unit-variance noise (one voxel -0.0, which only a bit-exact copy keeps), a shifted
    all-negative volume, a constant volume"""
    rs = np.random.RandomState(seed)
    a = rs.standard_normal(size)
    a[0, 0, 1] = -0.0
    b = -50.0 + 3.0 * rs.standard_normal(size)
    b = np.minimum(b, -1.0)
    c = np.full(size, 0.3)
    return np.stack([a, b, c]).astype(np.float32)
