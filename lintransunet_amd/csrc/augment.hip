// Augmentation of the NIfTI pipeline's patches on the device (no reference counterpart: the monai driver crops, flips and rot90s
// only).  Three kernels: ltu_sample_affine cuts rotated / zoomed / flipped patches straight from the scan in one gather (and adds
// Gaussian noise in the store), ltu_sample_elastic is that gather with a B-spline free-form deformation folded in, ltu_gauss_blur3
// blurs a batch of patches in one launch (three 1-D passes inside a workgroup).  ltu_sample_channels is either gather for a scan of
// up to four channels on one grid: the same kernels, instantiated per channel count.  ltu_sample_spline is ltu_sample_channels with
// a cubic B-spline image interpolation (64 or 32 taps on prefiltered coefficients) for the patches that ask for it: the same kernels
// again, instantiated per tap count along D, with the cubic taps as a workgroup-uniform branch.  ltu_sample_vote is the label half of
// either gather with the label taken by class vote over the 8 trilinear taps (nnU-Net's "one-hot, order 1") instead of nearest: the
// same kernels once more, a compile-time choice instantiated for the label-only, one-channel case alone.
//
// ---- the noise generator (restated in numpy by lintransunet_amd/data.py::noise_reference) ------------------------------------
// Stateless like the dropout masks: the normal deviate of voxel i (the linear index (x * w + y) * d + z inside its patch, < 2^32)
// of a patch with the 64-bit seed (lo = low 32 bits, hi = high 32 bits) is, with fmix32 of common.h and uint32 arithmetic,
//   ka = fmix32(lo ^ 0x243F6A88) + fmix32(hi ^ 0x85A308D3) * 0x9E3779B1
//   kb = fmix32(hi ^ 0x13198A2E) + fmix32(lo ^ 0x03707344) * 0x9E3779B1
//   j  = i >> 1                                       (one Box-Muller pair per two voxels)
//   w1 = fmix32(j ^ ka),  w2 = fmix32((j + 0x9E3779B9) ^ kb)
//   u1 = ((w1 >> 9) + 0.5) * 2^-23,  u2 = ((w2 >> 9) + 0.5) * 2^-23        (exact in fp32, in (0, 1))
//   r  = sqrt(-2 ln u1),  z[2j] = r cos(2 pi u2),  z[2j + 1] = r sin(2 pi u2)
// in fp32 with logf / sqrtf / sincospif.  |z| <= sqrt(48 ln 2) = 5.77.
#include "common.h"
#include "resample_coords.h"

struct NoiseKey { uint32_t ka, kb; };
__device__ __forceinline__ NoiseKey noise_key(unsigned long long seed) {
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  NoiseKey k;
  k.ka = fmix32(lo ^ 0x243F6A88u) + fmix32(hi ^ 0x85A308D3u) * 0x9E3779B1u;
  k.kb = fmix32(hi ^ 0x13198A2Eu) + fmix32(lo ^ 0x03707344u) * 0x9E3779B1u;
  return k;
}
// the two deviates of pair j
__device__ __forceinline__ void noise_pair(const NoiseKey& k, uint32_t j, float* z0, float* z1) {
  const uint32_t w1 = fmix32(j ^ k.ka), w2 = fmix32((j + 0x9E3779B9u) ^ k.kb);
  const float u1 = ((float)(w1 >> 9) + 0.5f) * 1.1920928955078125e-7f, u2 = ((float)(w2 >> 9) + 0.5f) * 1.1920928955078125e-7f;
  const float r = sqrtf(-2.f * logf(u1));
  float sn, cs;
  sincospif(2.f * u2, &sn, &cs);
  *z0 = r * cs;
  *z1 = r * sn;
}

// ---- ltu_sample_affine ---------------------------------------------------------------------------------------------------------
// A workgroup takes TX consecutive x (patch H index), TY consecutive y and ZL * VEC consecutive z of one patch: ZL lanes along z,
// then TY along y, then TX along x, powers of two chosen on the host from d and w so that ZL * TY * TX = 256 (a shallow, narrow
// patch folds several x into a block instead of leaving lanes idle).  A row's origin o = M (x, y0, z0, 1) is fp64 and is split per
// axis into an integer base and a fraction in [0, 1); inside the row tile the coordinate is base + (fr + m1 * yl + m2 * zl) with the
// bracket in fp32: at most 256 steps of a tile keep it within ~2e-5 of the fp64 coordinate, floors, weights and tap indices are
// fp32 / int32, and a matrix with integer entries gives exact integers: the weights are then 1 and 0 and the sum of w * v returns
// the source voxel's value (its bits, except that a source -0.0 comes out as +0.0: 0.f + -0.f, and adding the 0 * v terms).  The bracket is clamped to [-2 - base, S + 1 - base] before the conversion (base itself
// is clamped to +-2^22, beyond every scan the entry point accepts), so the conversion is defined for every finite matrix.
//
// NCH > 1 (ltu_sample_channels): the scan holds NCH channels [NCH][H][W][D] on one grid.  Everything above is formed once per output
// voxel; each channel then runs its own 8 taps (the same expressions in the same order as NCH == 1, so channel c has the bits of a
// single-channel call on img[c]) with its own fill, sigma and seed.  A launch carries 32 patches of one channel or 8 of up to four
// (the arguments stay below 4 KiB); the entry points split a call into such launches.
template <int NCH>
struct SampleArgs {
  static constexpr int MAXN = NCH == 1 ? LTU_SAMPLE_AFFINE_MAX : 8;
  double mat[MAXN][12];
  unsigned long long seed[MAXN][NCH];
  float sigma[MAXN][NCH];
  float fill[NCH];
};
// ltu_sample_spline (ND = taps along D: 4 at order 3, 2 at order 1) carries the coefficient volume, each channel's clamp and which
// patches of the launch are cubic on top; the kernels of the three older entry points (ND == 0) keep SampleArgs as their argument
template <int NCH>
struct CubicArgs : SampleArgs<NCH> {
  const float* coef;
  float lo[NCH], hi[NCH];
  unsigned char cubic[SampleArgs<NCH>::MAXN];
};
template <int NCH, int ND>
using SaArgs = std::conditional_t<ND == 0, SampleArgs<NCH>, CubicArgs<NCH>>;
template <int NCH>
__device__ __forceinline__ bool sa_cubic(const SampleArgs<NCH>&, int) { return false; }
template <int NCH>
__device__ __forceinline__ bool sa_cubic(const CubicArgs<NCH>& c, int k) { return c.cubic[k] != 0; }

struct SaAxis { int base; float fr, lo, hi; };
__device__ __forceinline__ SaAxis sa_axis(double o, int S) {
  const double b = fmin(fmax(floor(o), -4194304.0), 4194304.0);
  SaAxis a;
  a.base = (int)b;
  a.fr = (float)fmin(fmax(o - b, -3.0e7), 3.0e7);       // [0, 1) unless base was clamped: then far out on the right side
  a.lo = (float)(-2.0 - b);
  a.hi = (float)((double)S + 1.0 - b);                  // exact in fp32: |.| <= 2^23 + 2
  return a;
}
// in-tile coordinate -> (index of the lower tap, weight of the upper tap)
__device__ __forceinline__ void sa_split(const SaAxis& a, float l, int* i0, float* t) {
  l = fminf(fmaxf(l, a.lo), a.hi);
  const float f = floorf(l);
  *t = l - f;
  *i0 = a.base + (int)f;
}
// round half to even of base + l
__device__ __forceinline__ int sa_round(int i0, float t) { return i0 + ((t > 0.5f || (t == 0.5f && (i0 & 1))) ? 1 : 0); }
// the label of one voxel: nearest, 0 outside the scan
template <typename IDX>
__device__ __forceinline__ uint8_t sa_label(const uint8_t* __restrict__ lab, const int (&i0)[3], const float (&t)[3], int H, int W,
                                            int D) {
  const int xr = sa_round(i0[0], t[0]), yr = sa_round(i0[1], t[1]), zr = sa_round(i0[2], t[2]);
  const bool in = (unsigned)xr < (unsigned)H && (unsigned)yr < (unsigned)W && (unsigned)zr < (unsigned)D;
  uint8_t lv = 0;
  if (in) lv = lab[((IDX)xr * W + yr) * D + zr];
  return lv;
}

// An interpolated value must have the same bits in every instantiation (VEC, NCH, IDX): -ffp-contract=fast would fuse a product
// into a following sum or not, depending on what else shares the operands (with several channels the compiler packs two channels'
// products into one instruction and leaves them unfused).  So the tap sums are explicit fmaf chains, and a product that is to be
// rounded before it is added goes through sa_rounded: an empty statement the compiler cannot look through, no instruction.
__device__ __forceinline__ float sa_rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// the label of one voxel by class vote (ltu_sample_vote): the 8 taps of sa_taps in its order r = 0 .. 7 with its weight expression,
// a tap outside the scan holding label 0 (sa_label's "0 outside", the image's fill), then label_vote8 (resample_coords.h).  Every
// tap is loaded, at its index clamped into the scan, and replaced by 0 when it was outside: 8 loads in flight together instead of
// 8 branches with a load each.
template <typename IDX>
__device__ __forceinline__ uint8_t sa_vote(const uint8_t* __restrict__ lab, const int (&i0)[3], const float (&t)[3], int H, int W,
                                           int D) {
  int l[8];
  float wt[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int bx = r >> 2, by = (r >> 1) & 1, bz = r & 1;
    const int xi = i0[0] + bx, yi = i0[1] + by, zi = i0[2] + bz;
    const bool in = (unsigned)xi < (unsigned)H && (unsigned)yi < (unsigned)W && (unsigned)zi < (unsigned)D;
    wt[r] = sa_rounded((bx ? t[0] : 1.f - t[0]) * (by ? t[1] : 1.f - t[1]) * (bz ? t[2] : 1.f - t[2]));
    const int xc = min(max(xi, 0), H - 1), yc = min(max(yi, 0), W - 1), zc = min(max(zi, 0), D - 1);
    const int v = lab[((IDX)xc * W + yc) * D + zc];
    l[r] = in ? v : 0;
  }
  return label_vote8(l, wt);
}

// the 8 trilinear taps of one voxel (lower corner i0, upper weights t): bounds test, weight and offset once, then every channel's
// own sum in tap order into vi[ch][j].  fill is a copy in registers: read from the kernel's argument struct at the tap, "fill or
// voxel" becomes one load through a pointer into either address space, a flat load (1.4x the time of the oblique gather).
template <int NCH, typename IDX, int VEC>
__device__ __forceinline__ void sa_taps(const float* __restrict__ img, long long HWD, const float (&fill)[NCH], const int (&i0)[3],
                                        const float (&t)[3], int H, int W, int D, int j, float (&vi)[NCH][VEC]) {
  float acc[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) acc[ch] = 0.f;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int bx = r >> 2, by = (r >> 1) & 1, bz = r & 1;
    const int xi = i0[0] + bx, yi = i0[1] + by, zi = i0[2] + bz;
    const bool in = (unsigned)xi < (unsigned)H && (unsigned)yi < (unsigned)W && (unsigned)zi < (unsigned)D;
    const float wt = (bx ? t[0] : 1.f - t[0]) * (by ? t[1] : 1.f - t[1]) * (bz ? t[2] : 1.f - t[2]);
    float v[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) v[ch] = fill[ch];
    if (in) {                                      // one branch per tap, the channels' loads together behind it
      const float* p = img + (((IDX)xi * W + yi) * D + zi);          // the offset exists only for a tap inside the scan
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) v[ch] = p[ch * HWD];
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) acc[ch] = fmaf(wt, v[ch], acc[ch]);
  }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) vi[ch][j] = acc[ch];
}

// ---- the cubic taps of ltu_sample_spline ----------------------------------------------------------------------------------------
// One voxel of a cubic patch, from the same (i0, t) the trilinear taps take: scipy.ndimage.map_coordinates(order=3, mode='constant')
// on mirror-prefiltered coefficients.  The voxel is inside when every coordinate component lies in [0, S - 1], ends included
// (i0 >= 0 and i0 + t <= S - 1); it is then clamp(sum of w * coef[taps], lo, hi) with the taps f-1 .. f+2 per cubic axis (2 taps f, f+1
// along D at ND == 2), whole-sample mirrored, and fill - unclamped - otherwise: there is no blending across the edge.  Inside test,
// 4 + 4 + ND offsets and weights once per voxel; each channel then runs its own sum in the fixed order of sp_tap_sum (spline.hip):
// the ND taps along D, adjacent floats away from the ends, as the inner fused multiply-add chain, then (wx wy) * row added by one
// fused multiply-add, W inside H.  The 4 ND taps of one H index and channel are loaded before the first is used, so that they are
// in flight together; the channels take their turn inside the H tap, so 4 ND loaded values and offsets are live at a time whatever
// NCH is (128 registers at NCH = 1, 131 at NCH = 4, against 250 with the channel loop outermost).

// the tap sum of one voxel per channel, in its fixed order; ADJ: the taps along D are oz[0] .. oz[0] + ND - 1
template <int NCH, int ND, bool ADJ>
__device__ __forceinline__ void sc_sum(const float* __restrict__ coef, long long HWD, const int (&ox)[4], const int (&oy)[4],
                                       const int (&oz)[ND], const float (&wx)[4], const float (&wy)[4], const float (&wz)[ND],
                                       float (&acc)[NCH]) {
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) acc[ch] = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const float* __restrict__ p = coef + ch * HWD;
      float v[4][ND];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float* __restrict__ q = p + (unsigned)(ox[a] + oy[b] + oz[0]);                // unsigned: a 32-bit offset on a uniform base
#pragma unroll
        for (int e = 0; e < ND; ++e) v[b][e] = ADJ ? q[e] : p[(unsigned)(ox[a] + oy[b] + oz[e])];
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        float row = wz[0] * v[b][0];
#pragma unroll
        for (int e = 1; e < ND; ++e) row = fmaf(wz[e], v[b][e], row);
        acc[ch] = fmaf(wx[a] * wy[b], row, acc[ch]);
      }
      // without it the scheduler hoists every channel's loads of every H tap to the top: 250 registers at NCH >= 2
      if (NCH > 1) __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int NCH, int ND, int VEC>
__device__ __forceinline__ void sc_taps(const float* __restrict__ coef, long long HWD, const float (&fill)[NCH], const float (&lo)[NCH],
                                        const float (&hi)[NCH], const int (&i0)[3], const float (&t)[3], int H, int W, int D, int j,
                                        float (&vi)[NCH][VEC]) {
  const int S[3] = {H, W, D};
  bool in = true;
#pragma unroll
  for (int s = 0; s < 3; ++s) in = in && i0[s] >= 0 && (i0[s] < S[s] - 1 || (i0[s] == S[s] - 1 && t[s] == 0.f));
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) vi[ch][j] = fill[ch];
  if (!in) return;
  int ox[4], oy[4], oz[ND];
  float wx[4], wy[4], wz[ND];
  sp_cubic_weights(t[0], wx);
  sp_cubic_weights(t[1], wy);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    ox[a] = sp_mirror(i0[0] - 1 + a, H) * (W * D);         // H W D < 2^31 (checked on the host)
    oy[a] = sp_mirror(i0[1] - 1 + a, W) * D;
  }
  if (ND == 4) {
    sp_cubic_weights(t[2], wz);
#pragma unroll
    for (int a = 0; a < ND; ++a) oz[a] = sp_mirror(i0[2] - 1 + a, D);
  } else {
    wz[0] = 1.f - t[2];
    wz[1] = t[2];
    oz[0] = i0[2];
    oz[1] = sp_mirror(i0[2] + 1, D);                       // i0 + 1 == D only with t == 0: a valid address, weight 0
  }
  // away from the ends of D no tap along it is mirrored: the ND taps are adjacent floats, and the same sum with the offsets 0 ..
  // ND - 1 as constants fetches a row with one load instead of ND (ltu_resample_spline's step from 1.76 to 0.89 ms)
  bool adjacent = true;
#pragma unroll
  for (int e = 1; e < ND; ++e) adjacent = adjacent && oz[e] == oz[0] + e;
  float acc[NCH];
  if (adjacent) sc_sum<NCH, ND, true>(coef, HWD, ox, oy, oz, wx, wy, wz, acc);
  else sc_sum<NCH, ND, false>(coef, HWD, ox, oy, oz, wx, wy, wz, acc);
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) vi[ch][j] = fminf(fmaxf(acc[ch], lo[ch]), hi[ch]);
}

// the store of a lane's VEC voxels at (x, y, z) of patch k: noise per channel, then whole vectors
template <int VEC, int NCH>
__device__ __forceinline__ void sa_store(float* __restrict__ oimg, uint8_t* __restrict__ olab, bool has_img, bool has_lab,
                                         float (&vi)[NCH][VEC], const uint8_t (&vl)[VEC], const unsigned long long (&seed)[NCH],
                                         const float (&sigma)[NCH], int k, int x, int y, int z, int h, int w, int d) {
  const uint32_t vox = ((uint32_t)x * (uint32_t)w + (uint32_t)y) * (uint32_t)d + (uint32_t)z;       // < 2^32 (checked on the host)
  const long long hwd = (long long)h * w * d;
  if (has_img) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const long long dst = ((long long)k * NCH + ch) * hwd + vox;
      const float sg = sigma[ch];
      if (sg > 0.f) {
        const NoiseKey key = noise_key(seed[ch]);
        if (VEC == 4) {                     // vox % 4 == 0: two whole pairs
          float n[4];
          noise_pair(key, vox >> 1, &n[0], &n[1]);
          noise_pair(key, (vox >> 1) + 1, &n[2], &n[3]);
#pragma unroll
          for (int j = 0; j < VEC; ++j) vi[ch][j] = fmaf(sg, n[j], vi[ch][j]);
        } else {
          float n0, n1;
          noise_pair(key, vox >> 1, &n0, &n1);
          vi[ch][0] = fmaf(sg, (vox & 1) ? n1 : n0, vi[ch][0]);
        }
      }
      if (VEC == 4) *reinterpret_cast<float4*>(oimg + dst) = make_float4(vi[ch][0], vi[ch][1], vi[ch][2], vi[ch][3]);
      else oimg[dst] = vi[ch][0];
    }
  }
  if (has_lab) {
    const long long dst = (long long)k * hwd + vox;
    if (VEC == 4)
      *reinterpret_cast<uint32_t*>(olab + dst) = (uint32_t)vl[0] | ((uint32_t)vl[1] << 8) | ((uint32_t)vl[2] << 16) | ((uint32_t)vl[3] << 24);
    else olab[dst] = vl[0];
  }
}

// ZDEC: every matrix of the launch has the form [[a, b, 0, .], [c, e, 0, .], [0, 0, g, .]] (rotation about D only): the in-plane
// taps, weights and the label's in-plane voxel are computed once per lane, the VEC depth voxels are 1-D lerps on the four rows.
// ND != 0 (ltu_sample_spline): a patch with c.cubic[k] takes the cubic taps at the general kernel's coordinates (with a z-decoupled
// matrix they are the z-decoupled kernel's: fmaf(0, ., fr) == fr); every other patch runs the code below as it stands, so it has
// the bits of the ND == 0 kernel the same call would have chosen.  A workgroup belongs to one patch: the branch is uniform.
// VOTE (ltu_sample_vote; img == nullptr, NCH == 1, ND == 0): the label by class vote over the 8 trilinear taps.  The z-decoupled
// path forms tap (r, e)'s weight as wxy[r] * (e ? tz : 1 - tz), which is sa_vote's product (x y) z, in sa_vote's tap order 2 r + e:
// the same bytes as the general kernel on the same matrices.
template <bool ZDEC, int VEC, int NCH, typename IDX, int ND = 0, bool VOTE = false>
__global__ void __launch_bounds__(256) sample_affine_kernel(const float* __restrict__ img, const uint8_t* __restrict__ lab,
                                                            float* __restrict__ oimg, uint8_t* __restrict__ olab, SaArgs<NCH, ND> c,
                                                            int H, int W, int D, int h, int w, int d, int zl_log2, int ty_log2) {
  static_assert(!VOTE || (NCH == 1 && ND == 0), "the vote is instantiated for the label-only call alone");
  const int k = blockIdx.z;
  const int zl = 1 << zl_log2, ty = 1 << ty_log2;
  const int x = (int)(blockIdx.y << (8 - zl_log2 - ty_log2)) + (int)(threadIdx.x >> (zl_log2 + ty_log2));
  const int ztiles = (d + zl * VEC - 1) / (zl * VEC);
  const int tile_y = blockIdx.x / ztiles, tile_z = blockIdx.x - tile_y * ztiles;
  const int y0 = tile_y * ty, z0 = tile_z * zl * VEC;
  const int yl = (threadIdx.x >> zl_log2) & (ty - 1), zq = (threadIdx.x & (zl - 1)) * VEC;
  const int y = y0 + yl, z = z0 + zq;
  if (x >= h || y >= w || z >= d) return;
  const double* m = c.mat[k];
  SaAxis ax[3];
  float my[3], mz[3];
  const int S[3] = {H, W, D};
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    ax[s] = sa_axis(fma(m[4 * s], (double)x, fma(m[4 * s + 1], (double)y0, fma(m[4 * s + 2], (double)z0, m[4 * s + 3]))), S[s]);
    my[s] = (float)m[4 * s + 1];
    mz[s] = (float)m[4 * s + 2];
  }
  const long long HWD = (long long)H * W * D;          // channel ch of the scan begins at img + ch * HWD
  float fill[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) fill[ch] = c.fill[ch];
  float vi[NCH][VEC];
  uint8_t vl[VEC];
  if (ND != 0 && sa_cubic(c, k)) {
    if constexpr (ND != 0) {
      float lo[NCH], hi[NCH];
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        lo[ch] = c.lo[ch];
        hi[ch] = c.hi[ch];
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        int i0[3];
        float t[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) sa_split(ax[s], fmaf(my[s], (float)yl, fmaf(mz[s], (float)(zq + j), ax[s].fr)), &i0[s], &t[s]);
        if (img != nullptr) sc_taps<NCH, ND>(c.coef, HWD, fill, lo, hi, i0, t, H, W, D, j, vi);
        if (lab != nullptr) vl[j] = sa_label<IDX>(lab, i0, t, H, W, D);
      }
    }
  } else if (ZDEC) {
    int i0[2];
    float t[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) sa_split(ax[s], fmaf(my[s], (float)yl, ax[s].fr), &i0[s], &t[s]);
    IDX row[4];                        // offset of the row's first voxel; 0 for a row outside the scan (never loaded through)
    bool in[4];
    float wxy[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int xi = i0[0] + (r >> 1), yi = i0[1] + (r & 1);
      in[r] = (unsigned)xi < (unsigned)H && (unsigned)yi < (unsigned)W;
      row[r] = in[r] ? ((IDX)xi * W + yi) * D : (IDX)0;
      wxy[r] = ((r >> 1) ? t[0] : 1.f - t[0]) * ((r & 1) ? t[1] : 1.f - t[1]);
    }
    const int xr = sa_round(i0[0], t[0]), yr = sa_round(i0[1], t[1]);
    const bool lin = (unsigned)xr < (unsigned)H && (unsigned)yr < (unsigned)W;
    const IDX lrow = lin ? ((IDX)xr * W + yr) * D : (IDX)0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      int iz;
      float tz;
      sa_split(ax[2], fmaf(mz[2], (float)(zq + j), ax[2].fr), &iz, &tz);
      if (img != nullptr) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const float* ic = img + ch * HWD;
          float p[2];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int zi = iz + e;
            const bool zin = (unsigned)zi < (unsigned)D;
            float acc = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = fmaf(wxy[r], (in[r] && zin) ? ic[row[r] + zi] : fill[ch], acc);
            p[e] = acc;
          }
          vi[ch][j] = sa_rounded(sa_rounded(1.f - tz) * p[0]) + sa_rounded(tz * p[1]);
        }
      }
      if constexpr (VOTE) {
        int l[8];
        float wt[8];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int zi = iz + e;
            wt[2 * r + e] = sa_rounded(wxy[r] * (e ? tz : 1.f - tz));
            const int v = lab[row[r] + min(max(zi, 0), D - 1)];            // row[r] is 0 for a row outside: a valid address
            l[2 * r + e] = (in[r] && (unsigned)zi < (unsigned)D) ? v : 0;
          }
        vl[j] = label_vote8(l, wt);
      } else if (lab != nullptr) {
        const int zr = sa_round(iz, tz);
        vl[j] = (lin && (unsigned)zr < (unsigned)D) ? lab[lrow + zr] : (uint8_t)0;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      int i0[3];
      float t[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) sa_split(ax[s], fmaf(my[s], (float)yl, fmaf(mz[s], (float)(zq + j), ax[s].fr)), &i0[s], &t[s]);
      if (img != nullptr) sa_taps<NCH, IDX>(img, HWD, fill, i0, t, H, W, D, j, vi);
      if constexpr (VOTE) vl[j] = sa_vote<IDX>(lab, i0, t, H, W, D);
      else if (lab != nullptr) vl[j] = sa_label<IDX>(lab, i0, t, H, W, D);
    }
  }
  sa_store<VEC, NCH>(oimg, olab, img != nullptr, lab != nullptr, vi, vl, c.seed[k], c.sigma[k], k, x, y, z, h, w, d);
}

template <bool ZDEC, int VEC, int NCH, typename IDX, int ND, bool VOTE>
static void sample_affine_launch(const float* img, const uint8_t* lab, float* oi, uint8_t* ol, const SaArgs<NCH, ND>& c, int n, int H,
                                 int W, int D, int h, int w, int d, hipStream_t st) {
  const int per_lane = (d + VEC - 1) / VEC;
  int zl_log2 = 0;
  while ((1 << zl_log2) < per_lane && zl_log2 < (VEC == 4 ? 4 : 6)) ++zl_log2;
  int ty_log2 = 0;
  while ((1 << ty_log2) < w && zl_log2 + ty_log2 < 8) ++ty_log2;
  const int zl = 1 << zl_log2, ty = 1 << ty_log2, tx = 256 >> (zl_log2 + ty_log2);
  const unsigned tiles = cdiv(w, ty) * cdiv(d, zl * VEC);
  hipLaunchKernelGGL((sample_affine_kernel<ZDEC, VEC, NCH, IDX, ND, VOTE>), dim3(tiles, cdiv(h, tx), n), dim3(256), 0, st, img, lab, oi, ol,
                     c, H, W, D, h, w, d, zl_log2, ty_log2);
}

// ---- ltu_sample_elastic --------------------------------------------------------------------------------------------------------
// ltu_sample_affine's gather with a cubic B-spline free-form deformation folded in ahead of the pull matrix (restated in numpy by
// lintransunet_amd/data.py::elastic_displacement).  A patch of size (h, w, d) carries a control lattice phi[3][gh][gw][gd] of
// displacements in PATCH voxels along the patch axes H, W, D, 4 <= g_a <= LTU_ELASTIC_MAX_GRID.  For the patch voxel p = (x, y, z)
// and, per axis a with patch coordinate t and patch extent n_a,
//   s = t * (g_a - 3) / (n_a - 1)        (s = 0 when n_a == 1)
//   i = min(floor(s), g_a - 4),  f = s - i
//   B(f) = ((1-f)^3, 3f^3 - 6f^2 + 4, -3f^3 + 3f^2 + 3f + 1, f^3) / 6
//   u_c(p) = sum_{l,m,n in 0..3} B_l(fx) B_m(fy) B_n(fz) * phi[c][ix+l][iy+m][iz+n]
//   source coordinate = M * (p + u(p), 1)
// the uniform cubic B-spline FFD: C2-smooth, exactly 0 for a zero lattice (the B are >= 0 and every product is +0), applied in patch
// space so that the crop, flip, rot90, rotation and zoom of M keep their meaning.  Image, label, fill and noise as in sample_affine.
//
// The tile of a workgroup is sample_affine's (ZL lanes of VEC voxels along z, TY along y, TX along x) with TX capped at SE_TX_MAX.
// The spline is contracted axis by axis, each stage where its inputs are shared widest:
//   x  once per workgroup: the lattice is loaded from memory once and enters LDS already contracted with the B(fx) of each of the
//      tile's TX rows, A[xl][c][gw][gd] (at most 8 * 3 * 64 floats = 6 KiB; a 512 x 512 x 32 patch has TX = 1: 768 B);
//   y  once per lane: the 4 rows iy .. iy+3 of A into the NC lattice columns c0 .. c0+NC-1 along z that the lane's run of VEC voxels
//      touches (c0 = iz of its first voxel): 4 * NC LDS reads and FMAs per component, the lanes of a wave reading few distinct
//      addresses (iy and c0 change every (n - 1) / (g - 3) voxels);
//   z  per voxel: 4 FMAs per component on the columns at off = iz - c0, picked by compile-time-indexed selects (no register array is
//      indexed at run time).  A run that crosses a lattice cell boundary has off > 0 in its later voxels; the far-end clamp
//      i = min(floor(s), g - 4) gives f = 1 there.
// NC: 4 for VEC == 1; for VEC == 4, 5 when the run spans at most two cells (3 (gd - 3) <= 0.99 (d - 1), the host decides) and 8
// otherwise (off <= gd - 4 <= 4).  Columns at or beyond gd are read at gd - 1 and never selected.
// Each component of u is clamped to +-LTU_ELASTIC_MAX_DISP with fmaxf / fminf (NaN -> -LTU_ELASTIC_MAX_DISP), so every lattice
// content gives a defined coordinate, and M[:, :3] u joins sample_affine's fp32 bracket: at most 64 |M| more on a bracket of at
// most 256 |M|, its error stays well inside the label's 1e-4 tie band.  With a zero lattice the bracket is sample_affine's plus
// +-0: the same bits.  There is no z-decoupled variant: a deformed row's in-plane taps change with z.
#define SE_TX_MAX 8
#define SE_PLANE (LTU_ELASTIC_MAX_GRID * LTU_ELASTIC_MAX_GRID)

// Every sum of the spline and of the displaced coordinate is an explicit fmaf chain (sa_rounded's comment: the patch must not
// depend on the instantiation, and the channel kernels share all of this with the single-channel one).
// patch coordinate t >= 0 at lattice scale -> (index of the first of the 4 control points, their weights)
__device__ __forceinline__ void se_basis(float t, float scale, int g, int* i, float (&b)[4]) {
  const float s = sa_rounded(t * scale);
  const int ii = min(max((int)floorf(s), 0), g - 4);
  const float f = s - (float)ii, f2 = f * f, f3 = f2 * f, om = 1.f - f;
  const float sixth = 1.f / 6.f;
  b[0] = om * om * om * sixth;
  b[1] = fmaf(3.f, f3, fmaf(-6.f, f2, 4.f)) * sixth;
  b[2] = fmaf(-3.f, f3, fmaf(3.f, f2, fmaf(3.f, f, 1.f))) * sixth;
  b[3] = f3 * sixth;
  *i = ii;
}
// w[0] p[0] + w[1] p[stride] + w[2] p[2 stride] + w[3] p[3 stride], summed in this order
__device__ __forceinline__ float se_dot4(const float (&w)[4], const float* p, int stride) {
  return fmaf(w[3], p[3 * stride], fmaf(w[2], p[2 * stride], fmaf(w[1], p[stride], w[0] * p[0])));
}

template <int VEC, int NC, int NCH, typename IDX, int ND = 0, bool VOTE = false>
__global__ void __launch_bounds__(256) sample_elastic_kernel(const float* __restrict__ img, const uint8_t* __restrict__ lab,
                                                             float* __restrict__ oimg, uint8_t* __restrict__ olab, SaArgs<NCH, ND> c,
                                                             const float* __restrict__ phi, int gh, int gw, int gd, float sx, float sy,
                                                             float sz, int H, int W, int D, int h, int w, int d, int zl_log2,
                                                             int ty_log2, int tx_log2) {
  static_assert(NC >= 4 && NC <= LTU_ELASTIC_MAX_GRID && (VEC == 4 || NC == 4), "NC columns cover a run of VEC voxels");
  static_assert(!VOTE || (NCH == 1 && ND == 0), "the vote is instantiated for the label-only call alone");
  __shared__ float A[SE_TX_MAX * 3 * SE_PLANE];
  const int k = blockIdx.z;
  const int zl = 1 << zl_log2, ty = 1 << ty_log2, tx = 1 << tx_log2;
  const int x0 = (int)(blockIdx.y << tx_log2);
  const int plane = gw * gd;
  const float* pk = phi + (long long)k * 3 * gh * plane;
  for (int e = threadIdx.x; e < tx * 3 * plane; e += 256) {          // e = (xl * 3 + component) * plane + (j * gd + q)
    const int xl = e / (3 * plane), r = e - xl * 3 * plane, cc = r / plane, jq = r - cc * plane;
    float v = 0.f;
    if (x0 + xl < h) {
      int ix;
      float bx[4];
      se_basis((float)(x0 + xl), sx, gh, &ix, bx);
      const float* p = pk + (cc * gh + ix) * plane + jq;             // rows ix .. ix + 3 <= gh - 1
      v = se_dot4(bx, p, plane);
    }
    A[e] = v;
  }
  __syncthreads();
  const int xl = (int)(threadIdx.x >> (zl_log2 + ty_log2));
  const int x = x0 + xl;
  const int ztiles = (d + zl * VEC - 1) / (zl * VEC);
  const int tile_y = blockIdx.x / ztiles, tile_z = blockIdx.x - tile_y * ztiles;
  const int y0 = tile_y * ty, z0 = tile_z * zl * VEC;
  const int yl = (threadIdx.x >> zl_log2) & (ty - 1), zq = (threadIdx.x & (zl - 1)) * VEC;
  const int y = y0 + yl, z = z0 + zq;
  if (xl >= tx || x >= h || y >= w || z >= d) return;
  const double* m = c.mat[k];
  SaAxis ax[3];
  float mx[3], my[3], mz[3];
  const int S[3] = {H, W, D};
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    ax[s] = sa_axis(fma(m[4 * s], (double)x, fma(m[4 * s + 1], (double)y0, fma(m[4 * s + 2], (double)z0, m[4 * s + 3]))), S[s]);
    mx[s] = (float)m[4 * s];
    my[s] = (float)m[4 * s + 1];
    mz[s] = (float)m[4 * s + 2];
  }
  int iy, c0;
  float by[4], bz[4];
  se_basis((float)y, sy, gw, &iy, by);
  se_basis((float)z, sz, gd, &c0, bz);
  float col[3][NC];
  {
    const float* a = A + xl * 3 * plane + iy * gd;                   // rows iy .. iy + 3 <= gw - 1
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const int qi = min(c0 + q, gd - 1);
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        const float* p = a + cc * plane + qi;
        col[cc][q] = se_dot4(by, p, gd);
      }
    }
  }
  const long long HWD = (long long)H * W * D;
  float fill[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) fill[ch] = c.fill[ch];
  float vi[NCH][VEC];
  uint8_t vl[VEC];
  const bool cubic = ND != 0 && sa_cubic(c, k);        // uniform in the workgroup; the deformed coordinate is shared, the taps differ
  [[maybe_unused]] float lo[NCH], hi[NCH];
  if constexpr (ND != 0) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      lo[ch] = c.lo[ch];
      hi[ch] = c.hi[ch];
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    int off = 0;
    if (j > 0) {
      int iz;
      se_basis((float)(z + j), sz, gd, &iz, bz);
      off = min(max(iz - c0, 0), NC - 4);
    }
    float u[3];
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      float acc = 0.f;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        float v = col[cc][n];
#pragma unroll
        for (int o = 1; o <= NC - 4; ++o) v = off == o ? col[cc][n + o] : v;
        acc = fmaf(bz[n], v, acc);
      }
      u[cc] = fminf(fmaxf(acc, -(float)LTU_ELASTIC_MAX_DISP), (float)LTU_ELASTIC_MAX_DISP);
    }
    int i0[3];
    float t[3];
#pragma unroll
    for (int s = 0; s < 3; ++s)
      sa_split(ax[s], fmaf(my[s], (float)yl, fmaf(mz[s], (float)(zq + j), ax[s].fr)) +
                          sa_rounded(fmaf(mz[s], u[2], fmaf(my[s], u[1], mx[s] * u[0]))),
               &i0[s], &t[s]);
    if (img != nullptr) {
      if (cubic) {
        if constexpr (ND != 0) sc_taps<NCH, ND>(c.coef, HWD, fill, lo, hi, i0, t, H, W, D, j, vi);
      } else {
        sa_taps<NCH, IDX>(img, HWD, fill, i0, t, H, W, D, j, vi);
      }
    }
    if constexpr (VOTE) vl[j] = sa_vote<IDX>(lab, i0, t, H, W, D);
    else if (lab != nullptr) vl[j] = sa_label<IDX>(lab, i0, t, H, W, D);
  }
  sa_store<VEC, NCH>(oimg, olab, img != nullptr, lab != nullptr, vi, vl, c.seed[k], c.sigma[k], k, x, y, z, h, w, d);
}

template <int VEC, int NC, int NCH, typename IDX, int ND, bool VOTE>
static void sample_elastic_launch(const float* img, const uint8_t* lab, float* oi, uint8_t* ol, const SaArgs<NCH, ND>& c,
                                  const float* phi, int gh, int gw, int gd, int n, int H, int W, int D, int h, int w, int d,
                                  hipStream_t st) {
  const int per_lane = (d + VEC - 1) / VEC;
  int zl_log2 = 0;
  while ((1 << zl_log2) < per_lane && zl_log2 < (VEC == 4 ? 4 : 6)) ++zl_log2;
  int ty_log2 = 0;
  while ((1 << ty_log2) < w && zl_log2 + ty_log2 < 8) ++ty_log2;
  int tx_log2 = 8 - zl_log2 - ty_log2;                 // a tile narrower than 256 / SE_TX_MAX lanes leaves the rest of them idle
  if ((1 << tx_log2) > SE_TX_MAX) tx_log2 = 3;
  static_assert(SE_TX_MAX == 8, "tx_log2 is capped at 3");
  const int zl = 1 << zl_log2, ty = 1 << ty_log2, tx = 1 << tx_log2;
  const unsigned tiles = cdiv(w, ty) * cdiv(d, zl * VEC);
  const float sx = h > 1 ? (float)((double)(gh - 3) / (double)(h - 1)) : 0.f;
  const float sy = w > 1 ? (float)((double)(gw - 3) / (double)(w - 1)) : 0.f;
  const float sz = d > 1 ? (float)((double)(gd - 3) / (double)(d - 1)) : 0.f;
  hipLaunchKernelGGL((sample_elastic_kernel<VEC, NC, NCH, IDX, ND, VOTE>), dim3(tiles, cdiv(h, tx), n), dim3(256), 0, st, img, lab, oi, ol,
                     c, phi, gh, gw, gd, sx, sy, sz, H, W, D, h, w, d, zl_log2, ty_log2, tx_log2);
}

// ---- the three entry points ------------------------------------------------------------------------------------------------------
// One call of any of them: the scan's K channels, per-patch matrices, per-patch-and-channel sigmas and seeds, per-channel fills, and
// the lattice when the call deforms.
struct SampleCall {
  const float* img;
  const uint8_t* lab;
  float* oi;
  uint8_t* ol;
  const double* mats;
  const float* phi;                    // NULL: the affine kernels
  int gh, gw, gd;
  const float* sigma;                  // [n][K] or NULL
  const unsigned long long* seeds;     // [n][K] or NULL
  const float* fill;                   // [K]
  int n, K, H, W, D, h, w, d;
  // ltu_sample_spline only (nd = the taps along D, 0 for the other entry points)
  int nd;
  const float* coef;
  const float* lo;                     // [K]
  const float* hi;                     // [K]
  const unsigned char* cubic;          // [n]
};

// everything the entry points refuse, in sample_affine's order; LTU_OK with *run = false: nothing to do
static int sample_check(const SampleCall& q, bool elastic, bool* run) {
  *run = false;
  if (q.mats == nullptr || (elastic && q.phi == nullptr) || (q.img == nullptr) != (q.oi == nullptr) ||
      (q.lab == nullptr) != (q.ol == nullptr) || (q.img == nullptr && q.lab == nullptr) || q.n < 0 || q.n > LTU_SAMPLE_AFFINE_MAX ||
      (q.sigma != nullptr && q.seeds == nullptr) || q.fill == nullptr)
    return LTU_E_ARG;
  if (q.K < 1 || q.K > LTU_MAX_INPUT_CHANNELS) return LTU_E_SHAPE;
  for (int ch = 0; ch < q.K; ++ch)
    if (!(q.fill[ch] - q.fill[ch] == 0.f)) return LTU_E_ARG;
  if (elastic && (q.gh < 4 || q.gw < 4 || q.gd < 4 || q.gh > LTU_ELASTIC_MAX_GRID || q.gw > LTU_ELASTIC_MAX_GRID ||
                  q.gd > LTU_ELASTIC_MAX_GRID))
    return LTU_E_SHAPE;
  if (q.n == 0) return LTU_OK;
  const int smax = 1 << 22;
  if (q.H < 1 || q.W < 1 || q.D < 1 || q.H > smax || q.W > smax || q.D > smax || q.h < 1 || q.w < 1 || q.d < 1 || q.h > 65535 ||
      (long long)q.h * q.w * q.d >= (1LL << 32) || (long long)cdiv(q.w, 4) * cdiv(q.d, 4) >= (1LL << 31))
    return LTU_E_SHAPE;
  for (int k = 0; k < q.n; ++k) {
    for (int j = 0; j < 12; ++j) {
      const double v = q.mats[12 * k + j];
      if (!(v - v == 0.0)) return LTU_E_ARG;             // NaN or infinite
    }
    for (int ch = 0; ch < q.K && q.sigma != nullptr; ++ch) {
      const float sg = q.sigma[k * q.K + ch];
      if (!(sg >= 0.f) || !(sg - sg == 0.f)) return LTU_E_ARG;
    }
  }
  // the cubic taps index the coefficients with 32 bits (ltu_spline_prefilter builds no larger volume either)
  if (q.nd != 0 && (long long)q.H * q.W * q.D >= (1LL << 31)) return LTU_E_SHAPE;
  if ((elastic && ((uintptr_t)q.phi & 3) != 0) || (q.d % 4 == 0 && (((uintptr_t)q.oi & 15) != 0 || ((uintptr_t)q.ol & 3) != 0)))
    return LTU_E_ALIGN;
  *run = true;
  return LTU_OK;
}

// a checked call as launches of at most SampleArgs<NCH>::MAXN patches; the kernel variant is chosen from the whole call, so that a
// patch has the same bits wherever the call is split.  ND != 0 (ltu_sample_spline) chooses as ND == 0 does, so that its trilinear
// patches run the expressions ltu_sample_channels would run on them; its scans are below 2^31 voxels: 32-bit indices only.
template <int NCH, int ND, bool VOTE = false>
static void sample_go(const SampleCall& q, hipStream_t st) {
  bool zdec = true;
  for (int k = 0; k < q.n; ++k) {
    const double* m = q.mats + 12 * k;
    zdec = zdec && m[2] == 0.0 && m[6] == 0.0 && m[8] == 0.0 && m[9] == 0.0;
  }
  const int vec = (q.d % 4 == 0) ? 4 : 1;
  const bool small = (long long)q.H * q.W * q.D < (1LL << 31);
  const bool two_cells = 3.0 * (q.gd - 3) <= 0.99 * (q.d - 1);       // a run of 4 voxels along z spans at most two lattice cells
  const long long hwd = (long long)q.h * q.w * q.d;
  SaArgs<NCH, ND> c;
  for (int ch = 0; ch < NCH; ++ch) c.fill[ch] = q.fill[ch];
  if constexpr (ND != 0) {
    c.coef = q.coef;
    for (int ch = 0; ch < NCH; ++ch) {
      c.lo[ch] = q.lo[ch];
      c.hi[ch] = q.hi[ch];
    }
  }
  for (int k0 = 0; k0 < q.n; k0 += SampleArgs<NCH>::MAXN) {
    const int n = q.n - k0 < SampleArgs<NCH>::MAXN ? q.n - k0 : SampleArgs<NCH>::MAXN;
    for (int k = 0; k < n; ++k) {
      for (int j = 0; j < 12; ++j) c.mat[k][j] = q.mats[12 * (k0 + k) + j];
      for (int ch = 0; ch < NCH; ++ch) {
        c.sigma[k][ch] = (q.img != nullptr && q.sigma != nullptr) ? q.sigma[(k0 + k) * NCH + ch] : 0.f;
        c.seed[k][ch] = q.seeds != nullptr ? q.seeds[(k0 + k) * NCH + ch] : 0ull;
      }
      if constexpr (ND != 0) c.cubic[k] = q.cubic[k0 + k];
    }
    float* oi = q.oi != nullptr ? q.oi + k0 * NCH * hwd : nullptr;
    uint8_t* ol = q.ol != nullptr ? q.ol + k0 * hwd : nullptr;
#define SA_GO(Z, V)                                                                                                          \
  do {                                                                                                                       \
    if (small) sample_affine_launch<Z, V, NCH, int, ND, VOTE>(q.img, q.lab, oi, ol, c, n, q.H, q.W, q.D, q.h, q.w, q.d, st); \
    else if constexpr (ND == 0)                                                                                              \
      sample_affine_launch<Z, V, NCH, long long, ND, VOTE>(q.img, q.lab, oi, ol, c, n, q.H, q.W, q.D, q.h, q.w, q.d, st);    \
  } while (0)
#define SE_GO(V, NCOL)                                                                                                               \
  do {                                                                                                                               \
    const float* pk = q.phi + (long long)k0 * 3 * q.gh * q.gw * q.gd;                                                                \
    if (small)                                                                                                                       \
      sample_elastic_launch<V, NCOL, NCH, int, ND, VOTE>(q.img, q.lab, oi, ol, c, pk, q.gh, q.gw, q.gd, n, q.H, q.W, q.D, q.h, q.w,  \
                                                         q.d, st);                                                                   \
    else if constexpr (ND == 0)                                                                                                      \
      sample_elastic_launch<V, NCOL, NCH, long long, ND, VOTE>(q.img, q.lab, oi, ol, c, pk, q.gh, q.gw, q.gd, n, q.H, q.W, q.D, q.h, \
                                                               q.w, q.d, st);                                                        \
  } while (0)
    if (q.phi != nullptr) {
      if (vec == 1) SE_GO(1, 4);
      else if (two_cells) SE_GO(4, 5);
      else SE_GO(4, LTU_ELASTIC_MAX_GRID);
    } else if (zdec && vec == 4) SA_GO(true, 4);
    else if (zdec) SA_GO(true, 1);
    else if (vec == 4) SA_GO(false, 4);
    else SA_GO(false, 1);
#undef SA_GO
#undef SE_GO
  }
}

template <int ND>
static void sample_go_channels(const SampleCall& q, hipStream_t st) {
  switch (q.K) {
    case 1: sample_go<1, ND>(q, st); break;
    case 2: sample_go<2, ND>(q, st); break;
    case 3: sample_go<3, ND>(q, st); break;
    default: sample_go<4, ND>(q, st); break;
  }
}

static int sample_run(const SampleCall& q, bool elastic, ltu_stream_t s, bool vote = false) {
  bool run;
  const int rc = sample_check(q, elastic, &run);
  if (rc != LTU_OK || !run) return rc;
  if (vote) {                          // label only, one "channel": the patch-count splitting of a K == 1 call
    sample_go<1, 0, true>(q, (hipStream_t)s);
    return ltu_check_launch();
  }
  static_assert(LTU_MAX_INPUT_CHANNELS == 4, "one instantiation per channel count");
  switch (q.nd) {
    case 0: sample_go_channels<0>(q, (hipStream_t)s); break;
    case 2: sample_go_channels<2>(q, (hipStream_t)s); break;
    default: sample_go_channels<4>(q, (hipStream_t)s); break;
  }
  return ltu_check_launch();
}

extern "C" int ltu_sample_affine(const float* img, const uint8_t* lab, float* out_img, uint8_t* out_lab, const double* mats,
                                 const float* noise_sigma, const unsigned long long* seeds, int n, int H, int W, int D, int h, int w,
                                 int d, float fill, ltu_stream_t s) {
  const SampleCall q = {img, lab, out_img, out_lab, mats, nullptr, 0, 0, 0, noise_sigma, seeds, &fill, n, 1, H, W, D, h, w, d};
  return sample_run(q, false, s);
}

extern "C" int ltu_sample_elastic(const float* img, const uint8_t* lab, float* out_img, uint8_t* out_lab, const double* mats,
                                  const float* phi, int gh, int gw, int gd, const float* noise_sigma, const unsigned long long* seeds,
                                  int n, int H, int W, int D, int h, int w, int d, float fill, ltu_stream_t s) {
  const SampleCall q = {img, lab, out_img, out_lab, mats, phi, gh, gw, gd, noise_sigma, seeds, &fill, n, 1, H, W, D, h, w, d};
  return sample_run(q, true, s);
}

extern "C" int ltu_sample_channels(const float* img, const uint8_t* lab, float* out_img, uint8_t* out_lab, const double* mats,
                                   const float* phi, int gh, int gw, int gd, const float* noise_sigma,
                                   const unsigned long long* seeds, const float* fill, int n, int K, int H, int W, int D, int h, int w,
                                   int d, ltu_stream_t s) {
  const SampleCall q = {img, lab, out_img, out_lab, mats, phi, gh, gw, gd, noise_sigma, seeds, fill, n, K, H, W, D, h, w, d};
  return sample_run(q, phi != nullptr, s);
}

extern "C" int ltu_sample_spline(const float* img, const float* coef, const uint8_t* lab, float* out_img, uint8_t* out_lab,
                                 const double* mats, const float* phi, int gh, int gw, int gd, const float* noise_sigma,
                                 const unsigned long long* seeds, const float* fill, const float* lo, const float* hi,
                                 const unsigned char* cubic, int n, int K, int H, int W, int D, int h, int w, int d, int order_d,
                                 ltu_stream_t s) {
  if (coef == nullptr || cubic == nullptr || lo == nullptr || hi == nullptr || (order_d != 1 && order_d != 3)) return LTU_E_ARG;
  if (K < 1 || K > LTU_MAX_INPUT_CHANNELS) return LTU_E_SHAPE;
  for (int ch = 0; ch < K; ++ch)
    if (!(lo[ch] <= hi[ch])) return LTU_E_ARG;             // a NaN bound too
  const SampleCall q = {img, lab, out_img, out_lab, mats, phi, gh, gw, gd, noise_sigma, seeds, fill, n, K, H, W, D, h, w, d,
                        order_d == 3 ? 4 : 2, coef, lo, hi, cubic};
  return sample_run(q, phi != nullptr, s);
}

// the label half of ltu_sample_channels by class vote: the same matrices, lattice, checks and launches, no image, no noise
extern "C" int ltu_sample_vote(const uint8_t* lab, uint8_t* out_lab, const double* mats, const float* phi, int gh, int gw, int gd, int n,
                               int H, int W, int D, int h, int w, int d, ltu_stream_t s) {
  if (lab == nullptr || out_lab == nullptr) return LTU_E_ARG;
  const float fill = 0.f;
  const SampleCall q = {nullptr, lab, nullptr, out_lab, mats, phi, gh, gw, gd, nullptr, nullptr, &fill, n, 1, H, W, D, h, w, d};
  return sample_run(q, phi != nullptr, s, true);
}

// ---- ltu_gauss_blur3 -----------------------------------------------------------------------------------------------------------
// One workgroup blurs a TH x TW x 32 tile of one patch.  Pass D reads the input rows of the tile and of its (rh, rw) halo in H and W
// from memory - 4 outputs per lane from 4 + 2 rd consecutive voxels, reflected at the patch's ends - and writes LDS buffer B
// [TH + 2 rh][TW + 2 rw][32]; pass W reads B and writes C [TH + 2 rh][TW][32]; pass H reads C and stores mul * value.  The halos are
// the call's largest radius per axis (the host knows them), so a call that blurs in plane only carries no halo it does not need.
// LDS rows are 32 floats with the lanes along D in every pass: the 32 lanes of a half wave fall on 32 different banks in the W and
// the H pass as they stand, no padding needed.  Every voxel of the tile is read from memory once per pass-D row it appears in (the
// halo rows of neighbouring tiles overlap), written once, and nothing intermediate leaves the CU.
#define GB_TD 32
#define GB_TH 16
#define GB_TAPS (LTU_BLUR_MAX_RADIUS + 1)
static_assert(GB_TD == 32, "the blur's index arithmetic (rows of 8 quads / 32 lanes) is written for 32");
struct BlurArgs {
  float wt[LTU_BLUR_MAX_N][3][GB_TAPS];       // wt[k][axis][t], t = 0 .. radius; 0 beyond
  int rad[LTU_BLUR_MAX_N][3];
  float mul[LTU_BLUR_MAX_N];
};

// scipy's 'reflect' (d c b a | a b c d | d c b a) for any i
__device__ __forceinline__ int reflect_idx(int i, int n) {
  int mth = i % (2 * n);
  if (mth < 0) mth += 2 * n;
  return mth < n ? mth : 2 * n - 1 - mth;
}

// 4 outputs from the window v[0 .. 4 + 2 R): out[i] = w[0] v[R + i] + sum_t w[t] (v[R + i - t] + v[R + i + t])
template <int RMAX>
__device__ __forceinline__ void blur4(const float (&v)[4 + 2 * RMAX], const float* __restrict__ wt, int r, float (&o)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float acc = wt[0] * v[RMAX + i];
#pragma unroll
    for (int t = 1; t <= RMAX; ++t)
      if (t <= r) acc = fmaf(wt[t], v[RMAX + i - t] + v[RMAX + i + t], acc);
    o[i] = r == 0 ? v[RMAX + i] : acc;
  }
}

template <int RMAX>
__global__ void __launch_bounds__(512) gauss_blur3_kernel(const float* __restrict__ x, float* __restrict__ out, BlurArgs c, int H, int W,
                                                          int D, int TW, int rh, int rw) {
  extern __shared__ float gb_lds[];
  const int k = blockIdx.y;
  const int tilesD = (D + GB_TD - 1) / GB_TD, tilesW = (W + TW - 1) / TW;
  int b = blockIdx.x;
  const int td = b % tilesD; b /= tilesD;
  const int tw = b % tilesW;
  const int th = b / tilesW;
  const int h0 = th * GB_TH, w0 = tw * TW, d0 = td * GB_TD;
  const int BH = GB_TH + 2 * rh, BW = TW + 2 * rw;
  float* B = gb_lds;                              // [BH][BW][32]
  float* C = gb_lds + BH * BW * GB_TD;            // [BH][TW][32]
  const long long per = (long long)H * W * D;
  const float* xk = x + k * per;
  float* ok = out + k * per;
  const int rhk = c.rad[k][0], rwk = c.rad[k][1], rdk = c.rad[k][2];
  const float* wh = c.wt[k][0];
  const float* ww = c.wt[k][1];
  const float* wd = c.wt[k][2];

  // pass D: memory -> B
  for (int it = threadIdx.x; it < BH * BW * (GB_TD / 4); it += blockDim.x) {
    const int q = it & 7, rowi = it >> 3;
    const int wwi = rowi % BW, hhi = rowi / BW;
    const int dq = d0 + 4 * q;
    if (dq >= D) continue;
    const int gh = reflect_idx(h0 - rh + hhi, H), gw = reflect_idx(w0 - rw + wwi, W);
    const float* row = xk + ((long long)gh * W + gw) * D;
    float v[4 + 2 * RMAX];
    const bool interior = dq - rdk >= 0 && dq + 3 + rdk < D;
#pragma unroll
    for (int j = 0; j < 4 + 2 * RMAX; ++j) {
      const int off = j - RMAX;                   // window position relative to dq
      v[j] = 0.f;
      if (off >= -rdk && off < 4 + rdk) v[j] = row[interior ? dq + off : reflect_idx(dq + off, D)];
    }
    float o[4];
    blur4<RMAX>(v, wd, rdk, o);
    *reinterpret_cast<float4*>(B + (hhi * BW + wwi) * GB_TD + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
  }
  __syncthreads();
  // pass W: B -> C, 4 consecutive w per lane, lanes along d
  for (int it = threadIdx.x; it < BH * (TW / 4) * GB_TD; it += blockDim.x) {
    const int dl = it & 31, r2 = it >> 5;
    const int wq = r2 % (TW / 4), hhi = r2 / (TW / 4);
    const float* brow = B + (hhi * BW + rw + 4 * wq) * GB_TD + dl;       // window position 0 of this lane
    float v[4 + 2 * RMAX];
#pragma unroll
    for (int j = 0; j < 4 + 2 * RMAX; ++j) {
      const int off = j - RMAX;
      v[j] = 0.f;
      if (off >= -rwk && off < 4 + rwk) v[j] = brow[off * GB_TD];
    }
    float o[4];
    blur4<RMAX>(v, ww, rwk, o);
#pragma unroll
    for (int i = 0; i < 4; ++i) C[(hhi * TW + 4 * wq + i) * GB_TD + dl] = o[i];
  }
  __syncthreads();
  // pass H: C -> memory, 4 consecutive h per lane, lanes along d
  const float mul = c.mul[k];
  for (int it = threadIdx.x; it < (GB_TH / 4) * TW * GB_TD; it += blockDim.x) {
    const int dl = it & 31, r2 = it >> 5;
    const int wl = r2 % TW, hq = r2 / TW;
    const int gw = w0 + wl, gd = d0 + dl;
    if (gw >= W || gd >= D || h0 + 4 * hq >= H) continue;
    const float* crow = C + ((rh + 4 * hq) * TW + wl) * GB_TD + dl;
    float v[4 + 2 * RMAX];
#pragma unroll
    for (int j = 0; j < 4 + 2 * RMAX; ++j) {
      const int off = j - RMAX;
      v[j] = 0.f;
      if (off >= -rhk && off < 4 + rhk) v[j] = crow[off * TW * GB_TD];
    }
    float o[4];
    blur4<RMAX>(v, wh, rhk, o);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gh = h0 + 4 * hq + i;
      if (gh < H) ok[((long long)gh * W + gw) * D + gd] = mul == 1.f ? o[i] : o[i] * mul;
    }
  }
}

extern "C" int ltu_gauss_blur3(const float* x, float* out, const float* weights, const int* radii, const float* mul, int n, int H,
                               int W, int D, ltu_stream_t s) {
  if (x == nullptr || out == nullptr || x == out || weights == nullptr || radii == nullptr || n < 0 || n > LTU_BLUR_MAX_N)
    return LTU_E_ARG;
  if (n == 0) return LTU_OK;
  if (H < 1 || W < 1 || D < 1 || H > (1 << 22) || W > (1 << 22) || D > (1 << 22)) return LTU_E_SHAPE;
  BlurArgs c;
  int rmax[3] = {0, 0, 0};
  const int ext[3] = {H, W, D};
  for (int k = 0; k < n; ++k) {
    for (int a = 0; a < 3; ++a) {
      const int r = radii[3 * k + a];
      if (r < 0) return LTU_E_ARG;
      if (r > LTU_BLUR_MAX_RADIUS || (r > 0 && r >= ext[a])) return LTU_E_SHAPE;
      c.rad[k][a] = r;
      if (r > rmax[a]) rmax[a] = r;
      for (int t = 0; t < GB_TAPS; ++t) {
        const float wv = t <= r ? weights[(3 * k + a) * GB_TAPS + t] : 0.f;
        if (!(wv - wv == 0.f)) return LTU_E_ARG;
        c.wt[k][a][t] = wv;
      }
    }
    const float m = mul != nullptr ? mul[k] : 1.f;
    if (!(m - m == 0.f)) return LTU_E_ARG;
    c.mul[k] = m;
  }
  // the widest tile whose two buffers fit the CU's 160 KiB
  const int rh = rmax[0], rw = rmax[1];
  int TW = 16;
  auto lds_bytes = [&](int tw) { return ((GB_TH + 2 * rh) * (tw + 2 * rw) + (GB_TH + 2 * rh) * tw) * GB_TD * (int)sizeof(float); };
  if (lds_bytes(TW) > 160 * 1024) TW = 8;
  const int smem = lds_bytes(TW);
  const long long tiles = (long long)cdiv(H, GB_TH) * cdiv(W, TW) * cdiv(D, GB_TD);
  if (tiles >= (1LL << 31)) return LTU_E_SHAPE;
  const bool wide = rmax[0] > 4 || rmax[1] > 4 || rmax[2] > 4;
  static LtuDevOnce attr_once;
  if (attr_once.first()) {
    ltu_dyn_lds(&gauss_blur3_kernel<4>, 160 * 1024);
    ltu_dyn_lds(&gauss_blur3_kernel<8>, 160 * 1024);
  }
  if (wide)
    hipLaunchKernelGGL(gauss_blur3_kernel<8>, dim3((unsigned)tiles, n), dim3(512), smem, (hipStream_t)s, x, out, c, H, W, D, TW, rh, rw);
  else
    hipLaunchKernelGGL(gauss_blur3_kernel<4>, dim3((unsigned)tiles, n), dim3(512), smem, (hipStream_t)s, x, out, c, H, W, D, TW, rh, rw);
  return ltu_check_launch();
}
