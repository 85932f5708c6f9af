"""CPU helpers of tests/test_gpu_stream_paths.py: the launchers' geometry formulas restated in Python, and float64 restatements,
stage by stage, of the operations the norm / gate / stencil / resampling kernels compute.  No GPU, no library."""
import math

import torch
import torch.nn.functional as F

IN_EPS = 1e-5
LRELU_SLOPE = 0.01
RISK = 2.0 ** -14             # an fp32 pre-activation this close to zero (relative to the magnitudes it sums) may take either branch


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- launcher geometry (csrc/*.hip)

def stats_rows(S, B, chunks=1024):
    """norm.hip stats_rows: (rows per chunk, chunks per sample) of instnorm_stats / instnorm_bwd_stats"""
    want = max(1, chunks // max(B, 1))
    rows = max(cdiv(S, want), 64)
    return rows, cdiv(S, rows)


def in_small_plan(S, C, kb=256, no_small=False):
    """norm.hip in_small_plan (bf16): (threads, NIT) of the one-launch kernels, or None"""
    if C % 8 or S > 4096 or S < 1 or S * C * 2 > kb * 1024 or no_small:
        return None
    nthr = 256 if S <= 1024 else 1024
    n = cdiv(S, nthr)
    return nthr, (1 if n <= 1 else 2 if n <= 2 else 4)


def per_sample_grid(nvec, B, total=4096):
    """norm.hip per_sample_grid: workgroups (of 256 vectors) per sample of the apply kernels"""
    cap = max(total // max(B, 1), 1)
    return max(1, min(cdiv(nvec, 256), cap))


def reduce_parts_nb(nparts):
    """norm.hip launch_reduce_parts: the template argument"""
    return 4 if nparts <= 128 else 8 if nparts <= 256 else 16 if nparts <= 512 else 32


def in_fixedc(C):
    """norm.hip ltu_instnorm_apply / _bwd: the loop stride of 256 four-vectors is a multiple of the channel count"""
    return 1024 % C == 0


def in_stats_accepts(C):
    """norm.hip ltu_instnorm_stats / _fwd / _bwd shape rule"""
    return C % 4 == 0 and C <= 1024 and 256 % (C // 4) == 0


def gate_rows(S, B, C):
    """pointwise.hip ltu_gate_bwd: (rows per block, row blocks per sample = parts folded, rows of the last block)"""
    nrg = 256 // (C // 4)
    cap = min((1 << 20) // (C * 5), 2048)
    want = max(1, cap // max(B, 1))
    rows = max(cdiv(S, want), nrg)
    rows = cdiv(rows, nrg) * nrg
    n = cdiv(S, rows)
    return rows, n, S - (n - 1) * rows


def sgrid(n, per_block=256):
    """pointwise.hip sgrid"""
    return max(1, min(cdiv(n, per_block), 8192))


def dw_geometry(B, H, W, D, C, blocks=512):
    """pointwise.hip launch_dwconv_halo (bf16: 64 channels per chunk): (chunks, bricks per workgroup, workgroups, bricks of the last)"""
    nchunk = cdiv(C, 64)
    bricks = B * cdiv(H, 4) * cdiv(W, 4) * cdiv(D, 8)
    nblk = min(max(blocks // nchunk, 1), bricks)
    bpb = cdiv(bricks, nblk)
    nblk = cdiv(bricks, bpb)
    return nchunk, bpb, nblk, bricks - (nblk - 1) * bpb


def tri_route(L_fine, L_coarse, inner, pair=True, rows=True):
    """roi.hip launch_tri_adj1d (bf16: 8 elements per vector): which kernel a 1-D adjoint pass takes"""
    nv = inner // 8
    if pair and L_fine != L_coarse and nv <= 64 and inner < (1 << 20) and rows:
        return 'tri_adj1d_pair_rows_kernel'
    if pair and L_fine != L_coarse:
        return 'tri_adj1d_pair_kernel'
    return 'tri_adj1d_kernel'


def tri_passes(B, H, W, D, C, sd, ports, pair=True):
    """roi.hip ltu_trilinear_adjoint: [(axis, kernel<bf16_t, HAS2>)] in launch order: depth (sd == 2), width, height"""
    out, two = [], ports > 1
    if sd == 2:
        out.append(('d', tri_route(2 * D, D, C, pair), two))
        two = False
    out.append(('w', tri_route(2 * W, W, D * C, pair), two))
    out.append(('h', tri_route(2 * H, H, W * D * C, pair), False))
    return [(ax, f'{k}<bf16_t, {str(has2).lower()}>') for ax, k, has2 in out]


TRI_TAB = 256


def pw_small_plan(M, N, K, no_pw=False):
    """pw_small.hip launch_pw_small_bf16 behind gemm.hip ltu_linear_fwd (lda == K, ldy == N, one weight block):
    (KS, NT, workgroups, 32-row tiles) or None when the launcher declines"""
    if no_pw or N % 8 or N > 64 or M < 65536 or K not in (16, 32, 64, 128):
        return None
    ntile = cdiv(M, 32)
    return K // 16, 2 if N > 32 else 1, max(1, min(cdiv(ntile, 16), 4096)), ntile


def whalo_splits(B, H, W, D, C, N, blocks=None):
    """conv_halo.hip launch_conv_wgrad_halo_bf16 (first generation): splits of the brick range"""
    cc = 32 if C % 32 == 0 else 16
    blocks = blocks or (768 if cc == 16 else 512)
    bricks = B * cdiv(H, 4) * cdiv(W, 4) * cdiv(D, 8)
    ns = min(max(blocks // (cdiv(C, cc) * cdiv(N, 32)), 1), bricks)
    return cdiv(bricks, cdiv(bricks, ns))


def wgrad_reduce_sg(N, K, nsplit):
    """gemm_bf16.hip launch_wgrad_reduce: the template argument"""
    quads = N * (K // 4)
    return 64 if quads < 256 * 16 and nsplit >= 128 else 16 if quads < 256 * 64 and nsplit >= 32 else 4


# ---------------------------------------------------------------------------------------------- bf16 emulation

def bf(t):
    return t.bfloat16().double()


def rounded(x, mag):
    """bf16 rounding of an fp32 value the kernel does not store, on its float64 value x: (rounded value, slack).  slack is one bf16
    ulp where x lies within RISK * mag of a rounding midpoint (the kernel's fp32 value may round the other way)"""
    xb = x.float().bfloat16().double()
    ulp = torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-30))) - 7)
    near = (ulp / 2 - (x - xb).abs()) <= RISK * mag
    return xb, torch.where(near, ulp, torch.zeros_like(ulp))


# ---------------------------------------------------------------------------------------------- InstanceNorm, per stage
# layout [B][S][C]; statistics [B][C]

def in_sums(x):
    """what instnorm_stats publishes: shift = first voxel, s1 = sum(x - shift), s2 = sum((x - shift)^2); and the magnitude of s1"""
    shift = x[:, 0, :]
    d = x - shift[:, None, :]
    return shift, d.sum(1), (d * d).sum(1), d.abs().sum(1)


def in_stat2(shift, s1, s2, S):
    """norm.hip in_stat / pointwise.hip in_stat2 in float64: (mean, rstd)"""
    m1 = s1 / S
    var = (s2 / S - m1 * m1).clamp_min(0.0)
    return shift + m1, 1.0 / torch.sqrt(var + IN_EPS)


def in_hat(x, mean, rstd):
    return (x - mean[:, None, :]) * rstd[:, None, :]


def in_apply(h, act, mask, res):
    a = torch.where(h > 0, h, h * LRELU_SLOPE) if act else h
    y = a * mask
    return y + res if res is not None else y


def in_bwd_g(g, h, act, mask):
    """g' = dy * mask * act'(xhat) (the kernels test h <= 0)"""
    gg = g * mask
    return torch.where(h <= 0, gg * LRELU_SLOPE, gg) if act else gg


def in_bwd_sums(gg, h):
    """bsums [B][C][2] = {sum g', sum g' xhat} and their magnitudes"""
    return torch.stack((gg.sum(1), (gg * h).sum(1)), -1), torch.stack((gg.abs().sum(1), (gg * h).abs().sum(1)), -1)


def in_bwd_apply(gg, h, rstd, bsums, S):
    return rstd[:, None, :] * (gg - bsums[:, None, :, 0] / S - h * bsums[:, None, :, 1] / S)


def in_risk(x, mean, rstd, exact0=None):
    """elements whose xhat lies within RISK of zero relative to the magnitudes |x| + |mean| it is the difference of: the kernel's fp32
    value may fall on the other side of the LeakyReLU switch.  exact0 [B][C]: channels with s1 == s2 == 0 (constant), where the
    kernels' x - mean is exactly 0 like the reference's"""
    r = (x - mean[:, None, :]).abs() <= RISK * (x.abs() + mean.abs()[:, None, :])
    if exact0 is not None:
        r = r & ~exact0[:, None, :]
    return r


# ---------------------------------------------------------------------------------------------- attention gate, per stage
# u1, u2, skip [B][S][C]; statistics [B][C]; a, ds [B][S]

def gate_fwd(h1, h2, pw, pb, skip):
    """(r = relu(h1 + h2), sdot, a = sigmoid(sdot))"""
    r = (h1 + h2).clamp_min(0.0)
    sdot = (r * pw).sum(-1) + pb
    return r, sdot, torch.sigmoid(sdot)


def gate_bwd_reduce(g, skip, a):
    """stage 1, per voxel: dskip = g a and ds = (sum_c g skip) a (1 - a)"""
    da = (g * skip).sum(-1)
    ds = da * a * (1 - a)
    return g * a[..., None], ds


def gate_dr(ds, h1, h2, pw):
    return torch.where(h1 + h2 > 0, ds[..., None] * pw, torch.zeros((), dtype=torch.float64))


def gate_sums(ds, h1, h2, pw):
    """from a given ds: dpsi_w [C], dpsi_b, bs1 / bs2 [B][C][2]"""
    r = (h1 + h2).clamp_min(0.0)
    dr = gate_dr(ds, h1, h2, pw)
    dpw = (ds[..., None] * r).sum((0, 1))
    bs1 = torch.stack((dr.sum(1), (dr * h1).sum(1)), -1)
    bs2 = torch.stack((dr.sum(1), (dr * h2).sum(1)), -1)
    return dpw, ds.sum(), bs1, bs2


def gate_bwd_apply(dr, h, rstd, bs, S):
    return rstd[:, None, :] * (dr - bs[:, None, :, 0] / S - h * bs[:, None, :, 1] / S)


def gate_risk(u1, m1, r1, u2, m2, r2):
    """pre-activations h1 + h2 within RISK of zero relative to the magnitudes summed into them"""
    t = in_hat(u1, m1, r1) + in_hat(u2, m2, r2)
    mag = (u1.abs() + m1.abs()[:, None, :]) * r1[:, None, :] + (u2.abs() + m2.abs()[:, None, :]) * r2[:, None, :]
    return t.abs() <= RISK * mag


# ---------------------------------------------------------------------------------------------- positional depthwise conv
# x [B][H][W][D][C]; w [C][1][3][3][3] in the reference's (kd, kh, kw) order; mask [B][C] in {0, 1 / (1 - p)}

def _shift(t, dh, dw, dd):
    """s[b, h, w, d] = t[b, h + dh, w + dw, d + dd], zero outside"""
    B, H, W, D, C = t.shape
    p = F.pad(t, (0, 0, 1, 1, 1, 1, 1, 1))
    return p[:, 1 + dh:1 + dh + H, 1 + dw:1 + dw + W, 1 + dd:1 + dd + D]


def dw_fwd(x, w, b, mask):
    """y = mask (x + sum_t w[c][kd][kh][kw] x[v + (kh - 1, kw - 1, kd - 1)] + b)"""
    acc = x + b
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                acc = acc + w[:, 0, kd, kh, kw] * _shift(x, kh - 1, kw - 1, kd - 1)
    return acc * mask[:, None, None, None, :]


def dw_bwd(g, x, w, mask):
    """(dx, dw, db) of dw_fwd for the output gradient g"""
    gm = g * mask[:, None, None, None, :]
    dx = gm.clone()
    dw = torch.zeros_like(w)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                dx = dx + w[:, 0, kd, kh, kw] * _shift(gm, 1 - kh, 1 - kw, 1 - kd)
                dw[:, 0, kd, kh, kw] = (gm * _shift(x, kh - 1, kw - 1, kd - 1)).sum((0, 1, 2, 3))
    return dx, dw, gm.sum((0, 1, 2, 3))


# ---------------------------------------------------------------------------------------------- trilinear x2, align_corners=True

def tri_matrix(L_in, L_out):
    """[L_out][L_in] of 1-D linear interpolation, align_corners=True (the identity when the lengths agree)"""
    A = torch.zeros(L_out, L_in, dtype=torch.float64)
    for o in range(L_out):
        src = float(o) if L_in == L_out else o * (L_in - 1) / (L_out - 1) if L_out > 1 else 0.0
        a = min(int(math.floor(src)), L_in - 1)
        lam = src - a
        A[o, a] += 1 - lam
        A[o, min(a + 1, L_in - 1)] += lam
    return A


def tri_support(A):
    """0 / 1 support of A widened by one input index either way: where an fp32 tap may put weight"""
    S = (A != 0).double()
    S = S + F.pad(S, (1, 0))[:, :-1] + F.pad(S, (0, 1))[:, 1:]
    return (S > 0).double()


def tri_fwd(x, Ah, Aw, Ad):
    """x [B][H][W][D][C] -> [B][Ho][Wo][Do][C]"""
    return torch.einsum('ph,qw,rd,bhwdc->bpqrc', Ah, Aw, Ad, x)


def tri_adj_axis(g, A, axis):
    """one 1-D adjoint pass: contracts the fine axis (1 = h, 2 = w, 3 = d) of g with A [fine][coarse]"""
    return torch.movedim(torch.tensordot(g, A, dims=([axis], [0])), -1, axis)


# ---------------------------------------------------------------------------------------------- ROI plans

def plan_offsets(B, H, W, eval_h, eval_w):
    """roi.hip carve_all: {plan: dict(ND, NS, L, src0, cnt, lidx (int offsets), wt, lw (float offsets))} for fh, fw, bh, bw"""
    up_h, up_w = 2 * ((eval_h + 1) // 2), 2 * ((eval_w + 1) // 2)
    io = fo = 0
    out = {}
    for name, ND, NS in (('fh', eval_h, H), ('fw', eval_w, W), ('bh', H, up_h), ('bw', W, up_w)):
        L = 2 * ND
        p = dict(ND=ND, NS=NS, L=L, src0=io, cnt=io + B * ND, lidx=io + B * ND + B * NS, wt=fo, lw=fo + B * ND * 2)
        io += B * ND + B * NS + B * NS * L
        fo += B * ND * 2 + B * NS * L
        out[name] = p
    out['n_int'], out['n_float'] = io, fo
    return out


def plan_matrices(ibuf, fbuf, p, B):
    """dense per-sample gather matrices A [B][ND][NS] from src0 / wt (taps clamped into range, as plan_gather reads them) and the
    transposed matrices T [B][NS][ND] from the adjoint lists cnt / lidx / lw"""
    ND, NS, L = p['ND'], p['NS'], p['L']
    src0 = ibuf[p['src0']:p['src0'] + B * ND].reshape(B, ND)
    wt = fbuf[p['wt']:p['wt'] + B * ND * 2].reshape(B, ND, 2).double()
    cnt = ibuf[p['cnt']:p['cnt'] + B * NS].reshape(B, NS)
    lidx = ibuf[p['lidx']:p['lidx'] + B * NS * L].reshape(B, NS, L)
    lw = fbuf[p['lw']:p['lw'] + B * NS * L].reshape(B, NS, L).double()
    A = torch.zeros(B, ND, NS, dtype=torch.float64)
    T = torch.zeros(B, NS, ND, dtype=torch.float64)
    for b in range(B):
        for i in range(ND):
            s0 = int(src0[b, i])
            A[b, i, min(max(s0, 0), NS - 1)] += wt[b, i, 0]
            A[b, i, min(max(s0 + 1, 0), NS - 1)] += wt[b, i, 1]
        for x in range(NS):
            for k in range(int(cnt[b, x])):
                T[b, x, int(lidx[b, x, k])] += lw[b, x, k]
    return A, T


def plan_apply(x, Ah, Aw):
    """x [B][NSh][NSw][D][C] -> [B][NDh][NDw][D][C]: A_h (x) A_w per sample"""
    return torch.einsum('bix,bjy,bxydc->bijdc', Ah, Aw, x)
