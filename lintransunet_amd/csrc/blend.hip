// Weighted and mirrored sliding-window blending: monai 0.7.0 sliding_window_inference(mode="gaussian") with its importance map
// given as three per-axis tables, plus mirror test-time augmentation (each window predicted again flipped along chosen axes, the
// prediction flipped back before it is blended).  Items are (sample, window start in the padded image, flip mask); the
// descriptors of one launch travel as a by-value kernel argument, so a launch needs no host-to-device copy.
//
// No atomics: every padded voxel covered by a launch is owned by one thread - the thread of the FIRST item that covers it - which
// loads votes / wsum once, adds the terms of every covering item in item order and stores once.  Each voxel therefore sees its
// updates in one fixed order, whatever the batching: the result is bit-identical between calls and for every window batch size.
#include "common.h"

struct BlendItems {
  int b[LTU_BLEND_ITEMS_MAX], h0[LTU_BLEND_ITEMS_MAX], w0[LTU_BLEND_ITEMS_MAX], d0[LTU_BLEND_ITEMS_MAX], mask[LTU_BLEND_ITEMS_MAX];
};

// desc: HOST int32 [n][5] = (b, h0, w0, d0, mask).  Whole windows inside the padded image, b < B, mask 0..7.
static int blend_items(BlendItems& it, const int* desc, int n, int B, int Hp, int Wp, int Dp, int h, int w, int d) {
  for (int k = 0; k < n; ++k) {
    const int* de = desc + 5 * k;
    if (de[4] < 0 || de[4] > 7) return LTU_E_ARG;
    if (de[0] < 0 || de[0] >= B || de[1] < 0 || de[2] < 0 || de[3] < 0 || de[1] > Hp - h || de[2] > Wp - w || de[3] > Dp - d)
      return LTU_E_SHAPE;
    it.b[k] = de[0]; it.h0[k] = de[1]; it.w0[k] = de[2]; it.d0[k] = de[3]; it.mask[k] = de[4];
  }
  return LTU_OK;
}

static int blend_shape(int n, int B, int Hp, int Wp, int Dp, int h, int w, int d) {
  if (n < 0 || n > LTU_BLEND_ITEMS_MAX) return LTU_E_ARG;
  if (B < 1 || h < 1 || w < 1 || d < 1 || h > Hp || w > Wp || d > Dp) return LTU_E_SHAPE;
  if ((long long)h * w * d >= (1LL << 31)) return LTU_E_SHAPE;
  return LTU_OK;
}

// one grid row (blockIdx.y) per item, so the item's descriptor is wave-uniform
static dim3 blend_grid(int n, long long per) {
  long long bx = (per + 255) / 256;
  if (bx > 2048) bx = 2048;
  return dim3((unsigned)bx, (unsigned)n);
}

// win [n][h][w][d] <- vol [B][H][W][D]: window voxel u of item k reads padded coordinate start + u, or start + r - 1 - u on an
// axis its mask flips (bit a = axis a); the padded image puts vol at offset pad_lo = (Hp - H) / 2 per axis, zeros elsewhere.
__global__ void __launch_bounds__(256) window_gather_mirror_kernel(const float* __restrict__ vol, float* __restrict__ win,
                                                                   BlendItems it, int H, int W, int D, int h, int w, int d, int ph,
                                                                   int pw, int pd) {
  const int k = blockIdx.y;
  const int b = it.b[k], m = it.mask[k];
  const int sh = it.h0[k] - ph, sw = it.w0[k] - pw, sd = it.d0[k] - pd;
  const int per = h * w * d;
  float* out = win + (long long)k * per;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < per; i += gridDim.x * 256) {
    int r = i;
    const int z = r % d; r /= d;
    const int y = r % w, x = r / w;
    const int xh = sh + ((m & 1) ? h - 1 - x : x), yw = sw + ((m & 2) ? w - 1 - y : y), zd = sd + ((m & 4) ? d - 1 - z : z);
    float v = 0.f;
    if ((unsigned)xh < (unsigned)H && (unsigned)yw < (unsigned)W && (unsigned)zd < (unsigned)D)
      v = vol[(((long long)b * H + xh) * W + yw) * D + zd];
    out[i] = v;
  }
}

// votes [B][C][Hp][Wp][Dp] += w * seg, wsum [B][Hp][Wp][Dp] += w, seg channels-last [n][h][w][d][C].  Thread (k, v) handles the
// padded voxel p = start_k + v (v in volume orientation: lanes walk D on the accumulators) iff no item j < k of the same sample
// covers p; it then applies every covering item j >= k in order: v_j = p - start_j, the prediction is read at the flipped
// position u_j (u = r - 1 - v on the axes item j flips) and weighted by max(g0[v0] g1[v1] g2[v2], wmin).
template <int C>
__global__ void __launch_bounds__(256) window_blend_kernel(const float* __restrict__ seg, float* __restrict__ votes,
                                                           float* __restrict__ wsum, const float* __restrict__ g0,
                                                           const float* __restrict__ g1, const float* __restrict__ g2, float wmin,
                                                           BlendItems it, int n, int Hp, int Wp, int Dp, int h, int w, int d) {
  const int k = blockIdx.y;
  const int b = it.b[k], hk = it.h0[k], wk = it.w0[k], dk = it.d0[k];
  const int per = h * w * d;
  const long long vol = (long long)Hp * Wp * Dp;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < per; i += gridDim.x * 256) {
    int r = i;
    const int z = r % d; r /= d;
    const int y = r % w, x = r / w;
    const int ph = hk + x, pw = wk + y, pd = dk + z;
    bool own = true;
    for (int j = 0; j < k; ++j)
      if (it.b[j] == b && (unsigned)(ph - it.h0[j]) < (unsigned)h && (unsigned)(pw - it.w0[j]) < (unsigned)w &&
          (unsigned)(pd - it.d0[j]) < (unsigned)d) {
        own = false;
        break;
      }
    if (!own) continue;
    const long long pos = ((long long)ph * Wp + pw) * Dp + pd;
    float* vp = votes + (long long)b * C * vol + pos;
    float* wp = wsum + (long long)b * vol + pos;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = vp[c * vol];
    float ws = *wp;
    for (int j = k; j < n; ++j) {
      if (it.b[j] != b) continue;
      const int v0 = ph - it.h0[j], v1 = pw - it.w0[j], v2 = pd - it.d0[j];
      if ((unsigned)v0 >= (unsigned)h || (unsigned)v1 >= (unsigned)w || (unsigned)v2 >= (unsigned)d) continue;
      const int m = it.mask[j];
      const int u0 = (m & 1) ? h - 1 - v0 : v0, u1 = (m & 2) ? w - 1 - v1 : v1, u2 = (m & 4) ? d - 1 - v2 : v2;
      const float* sp = seg + ((((long long)j * h + u0) * w + u1) * d + u2) * C;
      const float wt = fmaxf(g0[v0] * g1[v1] * g2[v2], wmin);
      ws += wt;
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = fmaf(wt, sp[c], acc[c]);          // fused for every C: a channel's sum does not depend on C
    }
#pragma unroll
    for (int c = 0; c < C; ++c) vp[c * vol] = acc[c];
    *wp = ws;
  }
}

extern "C" int ltu_window_gather_mirror(const float* vol, float* win, const int* desc, int n, int B, int H, int W, int D, int Hp,
                                        int Wp, int Dp, int h, int w, int d, ltu_stream_t s) {
  if (vol == nullptr || win == nullptr || desc == nullptr) return LTU_E_ARG;
  int rc = blend_shape(n, B, Hp, Wp, Dp, h, w, d);
  if (rc != LTU_OK) return rc;
  if (H < 1 || W < 1 || D < 1 || H > Hp || W > Wp || D > Dp) return LTU_E_SHAPE;
  BlendItems it;
  if ((rc = blend_items(it, desc, n, B, Hp, Wp, Dp, h, w, d)) != LTU_OK) return rc;
  if (n == 0) return LTU_OK;
  const long long per = (long long)h * w * d;
  hipLaunchKernelGGL(window_gather_mirror_kernel, blend_grid(n, per), dim3(256), 0, (hipStream_t)s, vol, win, it, H, W, D, h, w, d,
                     (Hp - H) / 2, (Wp - W) / 2, (Dp - D) / 2);
  return ltu_check_launch();
}

extern "C" int ltu_window_blend(const float* seg, float* votes, float* wsum, const float* g0, const float* g1, const float* g2,
                                float wmin, const int* desc, int n, int B, int C, int Hp, int Wp, int Dp, int h, int w, int d,
                                ltu_stream_t s) {
  if (seg == nullptr || votes == nullptr || wsum == nullptr || g0 == nullptr || g1 == nullptr || g2 == nullptr || desc == nullptr)
    return LTU_E_ARG;
  int rc = blend_shape(n, B, Hp, Wp, Dp, h, w, d);
  if (rc != LTU_OK) return rc;
  if (C < 1 || C > 8) return LTU_E_SHAPE;
  BlendItems it;
  if ((rc = blend_items(it, desc, n, B, Hp, Wp, Dp, h, w, d)) != LTU_OK) return rc;
  if (n == 0) return LTU_OK;
  const dim3 grid = blend_grid(n, (long long)h * w * d);
  hipStream_t st = (hipStream_t)s;
#define LTU_BLEND_CASE(CC)                                                                                                          \
  case CC:                                                                                                                          \
    hipLaunchKernelGGL(window_blend_kernel<CC>, grid, dim3(256), 0, st, seg, votes, wsum, g0, g1, g2, wmin, it, n, Hp, Wp, Dp, h, w, \
                       d);                                                                                                          \
    break;
  switch (C) {
    LTU_BLEND_CASE(1) LTU_BLEND_CASE(2) LTU_BLEND_CASE(3) LTU_BLEND_CASE(4)
    LTU_BLEND_CASE(5) LTU_BLEND_CASE(6) LTU_BLEND_CASE(7) LTU_BLEND_CASE(8)
  }
#undef LTU_BLEND_CASE
  return ltu_check_launch();
}
