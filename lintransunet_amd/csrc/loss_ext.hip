// The wider deep-supervision loss family of one decoder level for gfx950: every training loss of loss/criterions.py and
// loss/multi_criterions.py that a `--criterion_list` can name, forward + analytic backward.
//
// Reference: loss/criterions.py 8-32 (DiceLoss), 466-530 (ContainLoss, ContainLoss2), 563-585 (IOULoss), 588-615 (SSLoss),
// 618-644 (FocalLoss), 738-751 (MSEcLoss); loss/multi_criterions.py 517-541 (BalanceDiceLoss2), 617-637 (ClassifyLoss),
// 640-663 (CrossEntroLoss0); and the five terms of loss.hip (CE, balanced Dice, per-class Dice, foreground-union Dice), so a spec
// that mixes old and new names still reads the probabilities once in the forward and once in the backward.
//
// With p = p[b,s,c], t = [label[b,s] == c] every term is a function of per-(sample, class) sums over the S voxels
//     P = sum p   T = sum t   I = sum p t   E = sum t (1-p) log max(p, 1e-6)   Q = sum p^2   R = sum t p^2
//     F = sum t (1-p)^gamma log p
// and three per-sample sums: E0b = sum (1-t_0) p_0 log max(1-p_0, 1e-6) (CrossEntroLoss0), M = sum m and
// K = sum m (y - label)^2 with m = 1 - t_0, y = sum_c c p_c (ClassifyLoss).  The backward is one streaming pass
//     dL/dp[s,c] = alpha + a p + t (beta + b p) + t (psi f'(p) + phi h'(p)) + [c = 0] (1-t) omega g'(p) + kappa_c m (y - label)
//     f(p) = (1-p) log max(p, 1e-6),  h(p) = (1-p)^gamma log p,  g(p) = p log max(1-p, 1e-6)
// with the eight per-(b, c) coefficients written by the finalize kernel.  Sums and derivative terms the spec does not use are
// switched off by a wave-uniform flag word.
#include "loss_stream.h"

#define LX_MAXC 4
#define LX_NS 7               // per-(b, c) sums: P T I E Q R F
#define LX_NX 3               // per-b sums behind them: E0b M K
#define LX_NK 8               // coefficients per (b, c): alpha a beta b psi phi omega kappa
#define LX_FIN 256            // finalize block: B * (7 C + 3) partial rows fold in one pass

enum { FL_E = 1, FL_Q = 2, FL_F = 4, FL_F2 = 8, FL_E0B = 16, FL_CLS = 32 };

static __host__ __device__ inline int lx_row(int C) { return LX_NS * C + LX_NX; }

struct LossExtCfg {
  float v[LTU_LOSS_EXT_NCFG];
};

// y = sum_c c p_c, a chain of fused multiply-adds from class 1 up
template <int C>
__device__ __forceinline__ float lx_mean_class(const float* f) {
  float y = 0.f;
#pragma unroll
  for (int c = 1; c < C; ++c) y = fmaf((float)c, f[c], y);
  return y;
}

// One voxel into the running sums a[c * LX_NS + k] (per class) and a[LX_NS * C + k] (per sample).  pl = probability of the labelled
// class (1 when the label is outside 0 .. C-1: E and F then add nothing); the logs of E and F are taken once per voxel and routed to
// the labelled class by selects.  Where a product meets a sum the rounding is written out, not left to -ffp-contract=fast (see the
// finalize kernel of loss.hip): p^2 is rounded on its own and added to Q and R (the bits the results of the four-voxel kernels have
// always carried), the class-index mean y is a chain of fused multiply-adds.  The other products meet their sum behind a select and
// cannot be fused.
template <int C>
__device__ __forceinline__ void lx_add(int lab, const float* f, float (&a)[LX_NS * C + LX_NX], unsigned fl, float gam) {
  float pl = 1.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float* acc = a + c * LX_NS;
    const float pc = f[c];
    const bool t = lab == c;
    acc[0] += pc;
    acc[1] += t ? 1.f : 0.f;
    acc[2] += t ? pc : 0.f;
    if (fl & FL_Q) {
      const float q = ls_rounded(pc * pc);
      acc[4] += q;
      acc[5] += t ? q : 0.f;
    }
    pl = t ? pc : pl;
  }
  if (fl & FL_E) {
    const float e = (1.f - pl) * logf(fmaxf(pl, 1e-6f));
#pragma unroll
    for (int c = 0; c < C; ++c) a[c * LX_NS + 3] += lab == c ? e : 0.f;
  }
  if (fl & FL_F) {
    // voxels with t = 0 add exactly 0 (the reference's 0 * log 0 there is NaN when p == 0)
    const float om = 1.f - pl;
    const float h = ((fl & FL_F2) ? om * om : powf(om, gam)) * logf(pl);
#pragma unroll
    for (int c = 0; c < C; ++c) a[c * LX_NS + 6] += lab == c ? h : 0.f;
  }
  float* ex = a + LX_NS * C;
  if (fl & FL_E0B) {
    const float p0 = f[0];
    ex[0] += lab == 0 ? 0.f : p0 * logf(fmaxf(1.f - p0, 1e-6f));
  }
  if (fl & FL_CLS) {
    const float d = lx_mean_class<C>(f) - (float)lab;
    ex[1] += lab != 0 ? 1.f : 0.f;
    ex[2] += lab != 0 ? d * d : 0.f;
  }
}

// p f32 [B][S][C], label u8 [B][S]; sums [1 + block][B][7 C + 3].  V4 (S % 4 == 0): four voxels per thread and trip, two trips in
// flight (loss_stream.h)
template <int C, bool V4>
__global__ void __launch_bounds__(256) lx_sums_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label, float* __restrict__ sums,
                                                      long long S, int rows_per_block, unsigned fl, float gam) {
  float a[LX_NS * C + LX_NX];
#pragma unroll
  for (int k = 0; k < LX_NS * C + LX_NX; ++k) a[k] = 0.f;
  ls_walk_block<C, V4, true>(p, label, S, rows_per_block, [&](int lab, const float* f) { lx_add<C>(lab, f, a, fl, gam); });
  ls_store_partial<LX_NS * C + LX_NX>(a, sums);
}

// One block of LX_FIN threads.  (1) The per-block partials fold in a fixed order (as in loss.hip: no fp32 atomics, the loss and its
// gradient are reproducible bit for bit).  (2) Thread b < B forms the per-sample pieces (balanced-Dice numerators, CE weights).
// (3) Thread (b, c) < B C writes its eight coefficients and its share of every term value.  (4) Thread k < LTU_LOSS_EXT_NTERM sums
// the shares of term k in (b, c) order; thread 0 then forms the total.  values: [0] total, [1 + k] term k, [1 + NTERM] total again.
__global__ void __launch_bounds__(LX_FIN) lx_finalize_kernel(const float* __restrict__ sums, int nblk, float* __restrict__ values,
                                                             float* __restrict__ coef, int B, long long S, int C, LossExtCfg cfg,
                                                             const float* __restrict__ scale_dev) {
  __shared__ float sm[LX_FIN];
  __shared__ float per_b[LX_FIN / (2 * LX_NS + LX_NX) + 1][8];        // B <= 15 (C = 2)
  __shared__ float share[LX_FIN / (LX_NS + 1)][LTU_LOSS_EXT_NTERM];
  __shared__ float val[LTU_LOSS_EXT_NTERM];
  const int W = lx_row(C);
  const int nout = B * W;                                  // <= LX_FIN
  ls_fold(sums, nblk, nout, sm);
  const float sc = scale_dev != nullptr ? scale_dev[0] : 1.f;
  float w[LTU_LOSS_EXT_NTERM];
#pragma unroll
  for (int k = 0; k < LTU_LOSS_EXT_NTERM; ++k) w[k] = cfg.v[k] * sc;
  const float sig = cfg.v[LTU_LOSS_EXT_SIGMA], eps = cfg.v[LTU_LOSS_EXT_EPS];
  const float Sf = (float)S, Bf = (float)B, Z = (float)B * Sf * (float)C, Z2 = 2.f * (float)B * Sf, nbc = (float)B * (float)C;
  // (2) per sample: [0] sum_c T, [1] Nb, [2] Db (balanced Dice over all classes), [3] Nb2, [4] Db2 (classes 1 ..), [5] w_a, [6] w_b
  if ((int)threadIdx.x < B) {
    const float* sb = sm + threadIdx.x * W;
    float Ttot = 0.f, num = 0.f, den = 0.f, num2 = 0.f, den2 = 0.f;
    for (int c = 0; c < C; ++c) Ttot += sb[c * LX_NS + 1];
    for (int c = 0; c < C; ++c) {
      const float P = sb[c * LX_NS], T = sb[c * LX_NS + 1], I = sb[c * LX_NS + 2];
      const float t = T + 1e-5f, wc = 1.f / (t * t);
      num += I * wc;
      den += (P + T) * wc;
      if (c > 0) {
        const float t2 = T + eps, wc2 = 1.f / (t2 * t2);
        num2 += I * wc2;
        den2 += (P + T) * wc2;
      }
    }
    float* q = per_b[threadIdx.x];
    const float P0 = sb[0];
    q[0] = Ttot;
    q[1] = 2.f * num + 1e-5f; q[2] = den + 1e-5f;
    q[3] = 2.f * num2 + eps; q[4] = den2 + eps;
    q[5] = (Sf - (P0 + eps)) / Sf; q[6] = (P0 - eps) / Sf;
  }
  __syncthreads();
  // (3) per (b, c)
  if ((int)threadIdx.x < B * C) {
    const int b = threadIdx.x / C, c = threadIdx.x % C;
    const float* sb = sm + b * W;
    const float* s = sb + c * LX_NS;
    const float P = s[0], T = s[1], I = s[2], E = s[3], Q = s[4], R = s[5], F = s[6];
    const float* q = per_b[b];
    float* sh = share[threadIdx.x];
    for (int k = 0; k < LTU_LOSS_EXT_NTERM; ++k) sh[k] = 0.f;
    float al = 0.f, la = 0.f, be = 0.f, lb = 0.f, psi = 0.f, phi = 0.f, om = 0.f, ka = 0.f;
    // a term with weight 0 adds nothing to the coefficients (its value may be inf / NaN on this data, e.g. IoU of an empty class,
    // and 0 * inf would poison the gradient of the terms that are on); its reported value is still formed
    auto on = [&](int k) { return cfg.v[k] != 0.f; };
    // CrossEntroLoss (criterions.py:696-735): w = (sum T - (P + 1e-5)) / sum T
    {
      const float Ttot = q[0], wce = (Ttot - (P + 1e-5f)) / Ttot;
      sh[LTU_LOSS_EXT_CE] = -wce * E;
      if (on(LTU_LOSS_EXT_CE)) {
        al += w[LTU_LOSS_EXT_CE] * E / (Z * Ttot);
        psi += -w[LTU_LOSS_EXT_CE] * wce / Z;
      }
    }
    // BalanceDiceLoss over all classes (eps 1e-5), BalanceDiceLoss2 over classes 1 .. C-1 (eps cfg)
    {
      const float t = T + 1e-5f, wc = 1.f / (t * t), Nb = q[1], Db = q[2];
      if (c == 0) sh[LTU_LOSS_EXT_BAL] = Nb / Db;
      if (on(LTU_LOSS_EXT_BAL)) {
        al += w[LTU_LOSS_EXT_BAL] * Nb * wc / (Bf * Db * Db);
        be += -w[LTU_LOSS_EXT_BAL] * 2.f * wc / (Bf * Db);
      }
      if (c > 0) {
        const float t2 = T + eps, wc2 = 1.f / (t2 * t2), N2 = q[3], D2 = q[4];
        if (c == 1) sh[LTU_LOSS_EXT_BAL2] = N2 / D2;
        if (on(LTU_LOSS_EXT_BAL2)) {
          al += w[LTU_LOSS_EXT_BAL2] * N2 * wc2 / (Bf * D2 * D2);
          be += -w[LTU_LOSS_EXT_BAL2] * 2.f * wc2 / (Bf * D2);
        }
      }
    }
    // DiceClassLoss of class c (eps 1e-9)
    {
      const float N = 2.f * I + 1e-9f, D = P + T + 1e-9f, wd = w[LTU_LOSS_EXT_DICE0 + c];
      sh[LTU_LOSS_EXT_DICE0 + c] = N / D;
      if (on(LTU_LOSS_EXT_DICE0 + c)) {
        al += wd * N / (Bf * D * D);
        be += -wd * 2.f / (Bf * D);
      }
    }
    // DiceLoss: 1 - mean_{b,c} (2I + eps) / (P + T + eps)
    {
      const float N = 2.f * I + eps, D = P + T + eps, wd = w[LTU_LOSS_EXT_DICE];
      sh[LTU_LOSS_EXT_DICE] = N / D;
      if (on(LTU_LOSS_EXT_DICE)) {
        al += wd * N / (nbc * D * D);
        be += -wd * 2.f / (nbc * D);
      }
    }
    // IOULoss: 1 - mean (I + eps) / (P + T - I)
    {
      const float N = I + eps, U = P + T - I, wi = w[LTU_LOSS_EXT_IOU];
      sh[LTU_LOSS_EXT_IOU] = N / U;
      if (on(LTU_LOSS_EXT_IOU)) {
        al += wi * N / (nbc * U * U);
        be += -wi * (1.f / U + N / (U * U)) / nbc;
      }
    }
    // SSLoss: mean sigma (R - 2I + T) / (T + eps) + (1 - sigma) (Q - R) / (S - T + eps)
    {
      const float e1 = T + eps, e2 = Sf - T + eps, ws = w[LTU_LOSS_EXT_SS];
      sh[LTU_LOSS_EXT_SS] = sig * (R - 2.f * I + T) / e1 + (1.f - sig) * (Q - R) / e2;
      if (on(LTU_LOSS_EXT_SS)) {
        la += ws * 2.f * (1.f - sig) / (nbc * e2);
        be += -ws * 2.f * sig / (nbc * e1);
        lb += ws * (2.f * sig / (nbc * e1) - 2.f * (1.f - sig) / (nbc * e2));
      }
    }
    // FocalLoss: -(1/Z) F;  MSELoss: (1/Z) (Q - 2I + T)
    sh[LTU_LOSS_EXT_FOCAL] = F;
    if (on(LTU_LOSS_EXT_FOCAL)) phi += -w[LTU_LOSS_EXT_FOCAL] / Z;
    sh[LTU_LOSS_EXT_MSE] = Q - 2.f * I + T;
    if (on(LTU_LOSS_EXT_MSE)) {
      la += 2.f * w[LTU_LOSS_EXT_MSE] / Z;
      be += -2.f * w[LTU_LOSS_EXT_MSE] / Z;
    }
    if (c == 0) {
      // DiceClassLoss0: Dice of the foreground union, P' = S - P, T' = S - T, I' = S - P - T + I (eps 1e-9)
      const float Nf = 2.f * (Sf - P - T + I) + 1e-9f, Df = (Sf - P) + (Sf - T) + 1e-9f, wf = w[LTU_LOSS_EXT_FG];
      sh[LTU_LOSS_EXT_FG] = Nf / Df;
      if (on(LTU_LOSS_EXT_FG)) {
        al += wf * (2.f / Df - Nf / (Df * Df)) / Bf;
        be += -wf * 2.f / (Bf * Df);
      }
      // CrossEntroLoss0: L = -(1/(2BS)) sum_b [w_a E + w_b E0b],  w_a = (S - P - eps) / S,  w_b = (P - eps) / S
      const float E0b = sb[LX_NS * C], wa = q[5], wb = q[6], w0 = w[LTU_LOSS_EXT_CE0];
      sh[LTU_LOSS_EXT_CE0] = wa * E + wb * E0b;
      if (on(LTU_LOSS_EXT_CE0)) {
        al += w0 * (E - E0b) / (Z2 * Sf);
        psi += -w0 * wa / Z2;
        om += -w0 * wb / Z2;
      }
    }
    if (c == 1) {
      // ContainLoss / ContainLoss2 (class 1): 1 - mean_b (I + eps) / ((1 - alpha)(T + eps) + alpha (P + eps))
      const float al1[2] = {cfg.v[LTU_LOSS_EXT_ALPHA], cfg.v[LTU_LOSS_EXT_ALPHA2]};
      for (int j = 0; j < 2; ++j) {
        const float a = al1[j], N = I + eps, Dn = (1.f - a) * (T + eps) + a * (P + eps), wc = w[LTU_LOSS_EXT_CONTAIN + j];
        sh[LTU_LOSS_EXT_CONTAIN + j] = N / Dn;
        if (on(LTU_LOSS_EXT_CONTAIN + j)) {
          al += wc * a * N / (Bf * Dn * Dn);
          be += -wc / (Bf * Dn);
        }
      }
    }
    // ClassifyLoss, pooled over the batch: L = sum K / (sum M + eps);  dL/dp_c = 2 c m (y - label) / (sum M + eps)
    {
      float Mt = 0.f, Kt = 0.f;
      for (int bb = 0; bb < B; ++bb) {
        Mt += sm[bb * W + LX_NS * C + 1];
        Kt += sm[bb * W + LX_NS * C + 2];
      }
      if (threadIdx.x == 0) sh[LTU_LOSS_EXT_CLASSIFY] = Kt / (Mt + eps);
      if (on(LTU_LOSS_EXT_CLASSIFY)) ka = w[LTU_LOSS_EXT_CLASSIFY] * 2.f * (float)c / (Mt + eps);
    }
    float* o = coef + (long long)threadIdx.x * LX_NK;
    *reinterpret_cast<float4*>(o) = make_float4(al, la, be, lb);
    *reinterpret_cast<float4*>(o + 4) = make_float4(psi, phi, om, ka);
  }
  __syncthreads();
  // (4) term values: shares summed in (b, c) order
  if ((int)threadIdx.x < LTU_LOSS_EXT_NTERM) {
    const int k = threadIdx.x;
    float t = 0.f;
    for (int i = 0; i < B * C; ++i) t += share[i][k];
    float v;
    switch (k) {
      case LTU_LOSS_EXT_CE: v = t / Z; break;
      case LTU_LOSS_EXT_DICE: case LTU_LOSS_EXT_IOU: v = 1.f - t / nbc; break;
      case LTU_LOSS_EXT_SS: v = t / nbc; break;
      case LTU_LOSS_EXT_FOCAL: v = -t / Z; break;
      case LTU_LOSS_EXT_MSE: v = t / Z; break;
      case LTU_LOSS_EXT_CE0: v = -t / Z2; break;
      case LTU_LOSS_EXT_CLASSIFY: v = t; break;
      default: v = 1.f - t / Bf; break;           // BAL, DICE0..3, FG, CONTAIN, CONTAIN2, BAL2: means over the batch
    }
    val[k] = v;
    values[1 + k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.f;
    for (int k = 0; k < LTU_LOSS_EXT_NTERM; ++k)
      if (cfg.v[k] != 0.f) total += w[k] * val[k];                 // terms switched off are not folded in (0 * NaN)
    values[0] = total;
    values[1 + LTU_LOSS_EXT_NTERM] = total;     // the autograd wrapper exposes this copy as the differentiable scalar
  }
}

// f'(p) of f = (1-p) log max(p, 1e-6) (the clamp passes no gradient below 1e-6) and h'(p) of h = (1-p)^gamma log p
__device__ __forceinline__ float lx_dce(float p) { return -logf(fmaxf(p, 1e-6f)) + (p > 1e-6f ? (1.f - p) / p : 0.f); }
// At p == 1 exactly (log p == 0) the first term of h' is its limit 0, also for gamma < 1 where (1-p)^(gamma-1) is inf there.
__device__ __forceinline__ float lx_dfocal(float p, unsigned fl, float gam) {
  const float om = 1.f - p, lp = logf(p);
  if (fl & FL_F2) return fmaf(-2.f * om, lp, om * om / p);
  return (lp != 0.f ? -gam * powf(om, gam - 1.f) * lp : 0.f) + powf(om, gam) / p;
}

// gradient of one voxel: f[C] probabilities, k[C][8] coefficients (scaled by gs on the way out).  Every product that meets a sum
// does so in a fused multiply-add, written out: the four-voxel and the one-voxel kernel then do the same arithmetic for a voxel
// (left to the compiler they did not)
template <int C>
__device__ __forceinline__ void lx_grad(int lab, const float* f, const float (&k)[C][LX_NK], float* o, unsigned fl, float gam, float gs) {
  float pl = 1.f;
#pragma unroll
  for (int c = 0; c < C; ++c) pl = lab == c ? f[c] : pl;
  const float dce = (fl & FL_E) ? lx_dce(pl) : 0.f;
  const float dfo = (fl & FL_F) ? lx_dfocal(pl, fl, gam) : 0.f;
  const float md = (fl & FL_CLS) && lab != 0 ? lx_mean_class<C>(f) - (float)lab : 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float pc = f[c];
    const bool t = lab == c;
    float g = fmaf(k[c][1], pc, k[c][0]);
    if (t) g += fmaf(k[c][5], dfo, fmaf(k[c][4], dce, fmaf(k[c][3], pc, k[c][2])));
    if (c == 0 && (fl & FL_E0B) && !t) {
      // g'(p) of g = p log max(1-p, 1e-6)
      const float q = 1.f - pc;
      g = fmaf(k[0][6], logf(fmaxf(q, 1e-6f)) - (q > 1e-6f ? pc / q : 0.f), g);
    }
    g = fmaf(k[c][7], md, g);
    o[c] = gs * g;
  }
}

template <int C>
__device__ __forceinline__ void lx_load_coef(const float* __restrict__ coef, int b, float (&k)[C][LX_NK]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float4 u = *reinterpret_cast<const float4*>(coef + ((long long)b * C + c) * LX_NK);
    const float4 v = *reinterpret_cast<const float4*>(coef + ((long long)b * C + c) * LX_NK + 4);
    k[c][0] = u.x; k[c][1] = u.y; k[c][2] = u.z; k[c][3] = u.w;
    k[c][4] = v.x; k[c][5] = v.y; k[c][6] = v.z; k[c][7] = v.w;
  }
}

// V4 (S % 4 == 0): four voxels per thread, 16-byte loads and stores (loss_stream.h)
template <int C, bool V4>
__global__ void __launch_bounds__(256) lx_bwd_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label, const float* __restrict__ coef,
                                                     const float* __restrict__ gscale, float* __restrict__ dp, long long S, unsigned fl, float gam) {
  const float gs = gscale[0];
  float k[C][LX_NK];
  lx_load_coef<C>(coef, blockIdx.y, k);
  ls_walk_grid<C, V4>(p, label, dp, S, [&](int lab, const float* f, float* o) { lx_grad<C>(lab, f, k, o, fl, gam, gs); });
}

// 0 = usable; LTU_E_SHAPE / LTU_E_ARG otherwise.  Flags: the sums and derivative terms the nonzero weights need.
static int lx_check(int B, long long S, int C, const float* cfg, unsigned* fl) {
  if (C < 2 || C > LX_MAXC || B < 1 || S < 1 || (long long)B * lx_row(C) > LX_FIN) return LTU_E_SHAPE;
  if (cfg == nullptr) return LTU_E_ARG;
  for (int k = 0; k < LTU_LOSS_EXT_NCFG; ++k)
    if (!std::isfinite(cfg[k])) return LTU_E_ARG;
  for (int k = C; k < LX_MAXC; ++k)
    if (cfg[LTU_LOSS_EXT_DICE0 + k] != 0.f) return LTU_E_ARG;      // Dice of a class the prediction does not have
  unsigned f = 0;
  if (cfg[LTU_LOSS_EXT_CE] != 0.f || cfg[LTU_LOSS_EXT_CE0] != 0.f) f |= FL_E;
  if (cfg[LTU_LOSS_EXT_SS] != 0.f || cfg[LTU_LOSS_EXT_MSE] != 0.f) f |= FL_Q;
  if (cfg[LTU_LOSS_EXT_FOCAL] != 0.f) f |= FL_F | (cfg[LTU_LOSS_EXT_GAMMA] == 2.f ? FL_F2 : 0u);
  if (cfg[LTU_LOSS_EXT_CE0] != 0.f) f |= FL_E0B;
  if (cfg[LTU_LOSS_EXT_CLASSIFY] != 0.f) f |= FL_CLS;
  *fl = f;
  return LTU_OK;
}

extern "C" long long ltu_loss_ext_ws_floats(int B, long long S, int C) {
  return (1 + cdiv(S, loss_rows(B, S))) * (long long)B * lx_row(C);
}

extern "C" int ltu_loss_ext_fwd(const float* p, const uint8_t* label, float* sums, long long sums_floats, float* values, float* coef, int B,
                                long long S, int C, const float* cfg, const float* scale_dev, ltu_stream_t s) {
  unsigned fl = 0;
  const int rc = lx_check(B, S, C, cfg, &fl);
  if (rc != LTU_OK) return rc;
  const long long rows = loss_rows(B, S);
  const int nblk = (int)cdiv(S, rows);
  if (sums == nullptr || (1 + (long long)nblk) * B * lx_row(C) > sums_floats) return LTU_E_ARG;
  LossExtCfg c;
  for (int k = 0; k < LTU_LOSS_EXT_NCFG; ++k) c.v[k] = cfg[k];
  const float gam = c.v[LTU_LOSS_EXT_GAMMA];
  const bool v4 = loss_v4(S, C);
  const dim3 grid(nblk, B);
  hipStream_t st = (hipStream_t)s;
  LTU_DISPATCH_C(C, {
    if constexpr (CT >= 2 && CT <= LX_MAXC) {          // lx_check: no other class count gets here, none is instantiated
      if (v4) hipLaunchKernelGGL((lx_sums_kernel<CT, true>), grid, dim3(256), 0, st, p, label, sums, S, (int)rows, fl, gam);
      else hipLaunchKernelGGL((lx_sums_kernel<CT, false>), grid, dim3(256), 0, st, p, label, sums, S, (int)rows, fl, gam);
    }
  });
  hipLaunchKernelGGL(lx_finalize_kernel, dim3(1), dim3(LX_FIN), 0, st, sums, nblk, values, coef, B, S, C, c, scale_dev);
  return ltu_check_launch();
}

extern "C" int ltu_loss_ext_bwd(const float* p, const uint8_t* label, const float* coef, const float* cfg, const float* gscale, float* dp,
                                int B, long long S, int C, ltu_stream_t s) {
  unsigned fl = 0;
  const int rc = lx_check(B, S, C, cfg, &fl);
  if (rc != LTU_OK) return rc;
  const float gam = cfg[LTU_LOSS_EXT_GAMMA];
  hipStream_t st = (hipStream_t)s;
  const bool v4 = loss_v4(S, C);
  const dim3 grid = loss_bwd_grid(B, S, v4);
  LTU_DISPATCH_C(C, {
    if constexpr (CT >= 2 && CT <= LX_MAXC) {
      if (v4) hipLaunchKernelGGL((lx_bwd_kernel<CT, true>), grid, dim3(256), 0, st, p, label, coef, gscale, dp, S, fl, gam);
      else hipLaunchKernelGGL((lx_bwd_kernel<CT, false>), grid, dim3(256), 0, st, p, label, coef, gscale, dp, S, fl, gam);
    }
  });
  return ltu_check_launch();
}
