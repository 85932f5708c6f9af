// Data side of the monai training driver (dataset/CT_pancreas_monai.py:37-58, 91-105): LoadImaged -> ScaleIntensityRanged ->
// Spacingd(bilinear / nearest) -> Orientationd('RAS'), then RandCropByPosNegLabeld -> RandFlipd -> RandRotate90d, as two
// streaming kernels.  The host folds Spacingd and Orientationd into one float64 pull matrix (output voxel -> source voxel,
// lintransunet_amd/geometry.py); a raw scan is uploaded once as stored (x fastest) and resampled straight into the RAS [H][W][D]
// volume the rest of the project reads.
#include "common.h"
#include "resample_coords.h"

// ---- resampling: out[p] = sample(src, M (p, 1)) ------------------------------------------------------------------------------
// Tile = 64 outputs along the lane axis P (the output axis whose step moves the source address least: lanes of a wave then read
// neighbouring source voxels along x) x 64 rows along Q x one index of R.  When P is not the output's fastest axis (the forward
// direction: source x maps to output H, output D is fastest) the tile goes through LDS and is stored with the lanes along Q, so both
// the gathers and the stores are coalesced.
#define RS_T 64
struct ResampleArgs {
  const void* src_img;
  const uint8_t* src_lab;
  float* out_img;
  uint8_t* out_lab;
  const double* mat;                 // [3][4]: row s = source axis s
  long long ss[3], os[3];            // element strides of source / output axes
  int S[3], O[3];
  int P, Q, R;                       // output axes: lane axis, row axis, grid axis
  int transpose;                     // store phase with lanes along Q
  float alpha, beta, lo, hi;         // image map per tap: clamp(alpha * v + beta, lo, hi)
};

template <typename T>
__device__ __forceinline__ float tap(const T* __restrict__ p) { return (float)*p; }

// IDX: int when every source offset fits in 31 bits (the tap addressing is then 32-bit; the kernel is VALU-bound)
// The tap code is shared by resample_grid_kernel and resample_argmax_kernel, so that a channel resampled by either has the same bits:
// clamp_coords (border padding), tap_setup (per source axis the offsets of the two taps and the fp32 weight of the upper one) and
// tap_sum (the 8 taps in the order k = 0 .. 7, each mapped first).  clamp_coords lives in resample_coords.h, shared with spline.hip.
template <typename IDX>
__device__ __forceinline__ void tap_setup(const int* S, const long long* ss, const double* c, IDX* o0, IDX* o1, float* t) {
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const double f = floor(c[s]);
    const int i0 = (int)f;
    const int i1 = i0 + (i0 < S[s] - 1 ? 1 : 0);
    t[s] = (float)(c[s] - f);
    o0[s] = (IDX)i0 * (IDX)ss[s];
    o1[s] = (IDX)i1 * (IDX)ss[s];
  }
}

template <typename T, typename IDX>
__device__ __forceinline__ float tap_sum(const T* __restrict__ src, const IDX* o0, const IDX* o1, const float* t, float alpha,
                                         float beta, float lo, float hi) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int bx = k & 1, by = (k >> 1) & 1, bz = k >> 2;
    const float w = (bx ? t[0] : 1.f - t[0]) * (by ? t[1] : 1.f - t[1]) * (bz ? t[2] : 1.f - t[2]);
    const float v = tap(src + (bx ? o1[0] : o0[0]) + (by ? o1[1] : o0[1]) + (bz ? o1[2] : o0[2]));
    // the product is rounded before it is added, as resample_grid_kernel has always been compiled; pinned, because -ffp-contract=fast
    // otherwise leaves the choice to the compiler, which fuses in some instantiations of resample_argmax_kernel and not in others
    float p = w * fminf(fmaxf(fmaf(alpha, v, beta), lo), hi);
    asm("" : "+v"(p));
    acc += p;
  }
  return acc;
}

template <typename T, typename IDX>
__device__ __forceinline__ void resample_one(const ResampleArgs& a, const T* __restrict__ src, double c0, double c1, double c2,
                                             float* vimg, uint8_t* vlab) {
  double c[3];
  clamp_coords(a.S, c0, c1, c2, c);
  if (src != nullptr) {
    IDX o0[3], o1[3];
    float t[3];
    tap_setup<IDX>(a.S, a.ss, c, o0, o1, t);
    *vimg = tap_sum<T, IDX>(src, o0, o1, t, a.alpha, a.beta, a.lo, a.hi);
  }
  if (a.src_lab != nullptr) {
    // grid_sample nearest: round half to even of the clamped coordinate
    const IDX off = (IDX)rint(c[0]) * (IDX)a.ss[0] + (IDX)rint(c[1]) * (IDX)a.ss[1] + (IDX)rint(c[2]) * (IDX)a.ss[2];
    *vlab = a.src_lab[off];
  }
}

template <typename T, typename IDX>
__global__ void __launch_bounds__(256) resample_grid_kernel(ResampleArgs a) {
  __shared__ float simg[RS_T][RS_T + 1];
  __shared__ uint8_t slab[RS_T][RS_T + 4];
  const int tilesP = (a.O[a.P] + RS_T - 1) / RS_T, tilesQ = (a.O[a.Q] + RS_T - 1) / RS_T;
  long long b = blockIdx.x;
  const int tp = (int)(b % tilesP); b /= tilesP;
  const int tq = (int)(b % tilesQ);
  const int r = (int)(b / tilesQ);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const T* src = (const T*)a.src_img;
  const int pP = tp * RS_T + lane;
  const double m[3][4] = {{a.mat[0], a.mat[1], a.mat[2], a.mat[3]}, {a.mat[4], a.mat[5], a.mat[6], a.mat[7]},
                          {a.mat[8], a.mat[9], a.mat[10], a.mat[11]}};
  double base[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) base[s] = fma(m[s][a.R], (double)r, m[s][3]) + m[s][a.P] * (double)pP;
  const long long obase = (long long)r * a.os[a.R];
  for (int row = wv; row < RS_T; row += 4) {
    const int pQ = tq * RS_T + row;
    float vi = 0.f;
    uint8_t vl = 0;
    const bool in = pP < a.O[a.P] && pQ < a.O[a.Q];
    if (in)
      resample_one<T, IDX>(a, src, fma(m[0][a.Q], (double)pQ, base[0]), fma(m[1][a.Q], (double)pQ, base[1]),
                      fma(m[2][a.Q], (double)pQ, base[2]), &vi, &vl);
    if (a.transpose) {
      simg[row][lane] = vi;
      slab[row][lane] = vl;
    } else if (in) {
      const long long o = obase + (long long)pP * a.os[a.P] + (long long)pQ * a.os[a.Q];
      if (a.out_img != nullptr) a.out_img[o] = vi;
      if (a.out_lab != nullptr) a.out_lab[o] = vl;
    }
  }
  if (!a.transpose) return;
  __syncthreads();
  const int qQ = tq * RS_T + lane;
  if (qQ >= a.O[a.Q]) return;
  for (int col = wv; col < RS_T; col += 4) {
    const int qP = tp * RS_T + col;
    if (qP >= a.O[a.P]) break;
    const long long o = obase + (long long)qP * a.os[a.P] + (long long)qQ * a.os[a.Q];
    if (a.out_img != nullptr) a.out_img[o] = simg[lane][col];
    if (a.out_lab != nullptr) a.out_lab[o] = slab[lane][col];
  }
}

extern "C" int ltu_resample_grid(const void* src_img, int src_dtype, const uint8_t* src_lab, int S0, int S1, int S2, long long ss0,
                                 long long ss1, long long ss2, float* out_img, uint8_t* out_lab, int O0, int O1, int O2,
                                 long long os0, long long os1, long long os2, const double* mat, int lane_axis, float alpha,
                                 float beta, float lo, float hi, ltu_stream_t s) {
  if (mat == nullptr || (src_img == nullptr) != (out_img == nullptr) || (src_lab == nullptr) != (out_lab == nullptr) ||
      (src_img == nullptr && src_lab == nullptr) || lane_axis < 0 || lane_axis > 2)
    return LTU_E_ARG;
  if (src_img != nullptr && src_dtype != LTU_F32 && src_dtype != LTU_U8 && src_dtype != LTU_I16) return LTU_E_DTYPE;
  if (S0 < 1 || S1 < 1 || S2 < 1 || O0 < 1 || O1 < 1 || O2 < 1 || ss0 < 1 || ss1 < 1 || ss2 < 1 || os0 < 1 || os1 < 1 || os2 < 1)
    return LTU_E_SHAPE;
  ResampleArgs a;
  a.src_img = src_img; a.src_lab = src_lab; a.out_img = out_img; a.out_lab = out_lab; a.mat = mat;
  a.ss[0] = ss0; a.ss[1] = ss1; a.ss[2] = ss2;
  a.os[0] = os0; a.os[1] = os1; a.os[2] = os2;
  a.S[0] = S0; a.S[1] = S1; a.S[2] = S2;
  a.O[0] = O0; a.O[1] = O1; a.O[2] = O2;
  a.alpha = alpha; a.beta = beta; a.lo = lo; a.hi = hi;
  // Q = the other axis with the smaller output stride; the tile is transposed through LDS when Q is faster than P
  a.P = lane_axis;
  const int u = (lane_axis + 1) % 3, v = (lane_axis + 2) % 3;
  a.Q = a.os[u] <= a.os[v] ? u : v;
  a.R = 3 - a.P - a.Q;
  a.transpose = a.os[a.Q] < a.os[a.P] ? 1 : 0;
  const long long blocks = (long long)cdiv(a.O[a.P], RS_T) * cdiv(a.O[a.Q], RS_T) * a.O[a.R];
  if (blocks >= (1LL << 31)) return LTU_E_SHAPE;
  const dim3 grid((unsigned)blocks), block(256);
  const bool small = (long long)(S0 - 1) * ss0 + (long long)(S1 - 1) * ss1 + (long long)(S2 - 1) * ss2 < (1LL << 31);
  const int type = (src_img == nullptr || src_dtype == LTU_U8) ? 0 : (src_dtype == LTU_I16 ? 1 : 2);
  if (small) {
    if (type == 0) hipLaunchKernelGGL((resample_grid_kernel<uint8_t, int>), grid, block, 0, (hipStream_t)s, a);
    else if (type == 1) hipLaunchKernelGGL((resample_grid_kernel<int16_t, int>), grid, block, 0, (hipStream_t)s, a);
    else hipLaunchKernelGGL((resample_grid_kernel<float, int>), grid, block, 0, (hipStream_t)s, a);
  } else {
    if (type == 0) hipLaunchKernelGGL((resample_grid_kernel<uint8_t, long long>), grid, block, 0, (hipStream_t)s, a);
    else if (type == 1) hipLaunchKernelGGL((resample_grid_kernel<int16_t, long long>), grid, block, 0, (hipStream_t)s, a);
    else hipLaunchKernelGGL((resample_grid_kernel<float, long long>), grid, block, 0, (hipStream_t)s, a);
  }
  return ltu_check_launch();
}

// ---- label by class vote: lab[p] = argmax_v sum of the trilinear weights of the taps that hold v ---------------------------------
// nnU-Net's label resampling ("one-hot, order 1") without the one-hot volume: clamp_coords, tap_setup and tap_sum's weight
// expression and tap order k = 0 .. 7, then label_vote8 (resample_coords.h).  The score of a class has the bits of tap_sum on its
// float32 indicator map with the identity map (each w * 1 rounded, then added; an added 0 changes nothing), so the label is
// ltu_resample_argmax's on the one-hot channels, for any u8 values and without a class count.  Same tile as resample_grid_kernel,
// with the u8 tile alone in LDS when it is transposed.
template <typename IDX>
__device__ __forceinline__ uint8_t vote_one(const ResampleArgs& a, double c0, double c1, double c2) {
  double c[3];
  clamp_coords(a.S, c0, c1, c2, c);
  IDX o0[3], o1[3];
  float t[3];
  tap_setup<IDX>(a.S, a.ss, c, o0, o1, t);
  int l[8];
  float w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int bx = k & 1, by = (k >> 1) & 1, bz = k >> 2;
    w[k] = (bx ? t[0] : 1.f - t[0]) * (by ? t[1] : 1.f - t[1]) * (bz ? t[2] : 1.f - t[2]);
    asm("" : "+v"(w[k]));            // rounded before it is added, as tap_sum's product is
    l[k] = a.src_lab[(bx ? o1[0] : o0[0]) + (by ? o1[1] : o0[1]) + (bz ? o1[2] : o0[2])];
  }
  return label_vote8(l, w);
}

template <typename IDX>
__global__ void __launch_bounds__(256) resample_vote_kernel(ResampleArgs a) {
  __shared__ uint8_t slab[RS_T][RS_T + 4];
  const int tilesP = (a.O[a.P] + RS_T - 1) / RS_T, tilesQ = (a.O[a.Q] + RS_T - 1) / RS_T;
  long long b = blockIdx.x;
  const int tp = (int)(b % tilesP); b /= tilesP;
  const int tq = (int)(b % tilesQ);
  const int r = (int)(b / tilesQ);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int pP = tp * RS_T + lane;
  const double m[3][4] = {{a.mat[0], a.mat[1], a.mat[2], a.mat[3]}, {a.mat[4], a.mat[5], a.mat[6], a.mat[7]},
                          {a.mat[8], a.mat[9], a.mat[10], a.mat[11]}};
  double base[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) base[s] = fma(m[s][a.R], (double)r, m[s][3]) + m[s][a.P] * (double)pP;
  const long long obase = (long long)r * a.os[a.R];
  for (int row = wv; row < RS_T; row += 4) {
    const int pQ = tq * RS_T + row;
    uint8_t vl = 0;
    const bool in = pP < a.O[a.P] && pQ < a.O[a.Q];
    if (in)
      vl = vote_one<IDX>(a, fma(m[0][a.Q], (double)pQ, base[0]), fma(m[1][a.Q], (double)pQ, base[1]),
                         fma(m[2][a.Q], (double)pQ, base[2]));
    if (a.transpose) slab[row][lane] = vl;
    else if (in) a.out_lab[obase + (long long)pP * a.os[a.P] + (long long)pQ * a.os[a.Q]] = vl;
  }
  if (!a.transpose) return;
  __syncthreads();
  const int qQ = tq * RS_T + lane;
  if (qQ >= a.O[a.Q]) return;
  const int cols = min(RS_T, a.O[a.P] - tp * RS_T);
  for (int col = wv; col < cols; col += 4)
    a.out_lab[obase + (long long)(tp * RS_T + col) * a.os[a.P] + (long long)qQ * a.os[a.Q]] = slab[lane][col];
}

extern "C" int ltu_resample_vote(const uint8_t* src_lab, int S0, int S1, int S2, long long ss0, long long ss1, long long ss2,
                                 uint8_t* out_lab, int O0, int O1, int O2, long long os0, long long os1, long long os2,
                                 const double* mat, int lane_axis, ltu_stream_t s) {
  if (mat == nullptr || src_lab == nullptr || out_lab == nullptr || lane_axis < 0 || lane_axis > 2) return LTU_E_ARG;
  if (S0 < 1 || S1 < 1 || S2 < 1 || O0 < 1 || O1 < 1 || O2 < 1 || ss0 < 1 || ss1 < 1 || ss2 < 1 || os0 < 1 || os1 < 1 || os2 < 1)
    return LTU_E_SHAPE;
  ResampleArgs a;
  a.src_img = nullptr; a.src_lab = src_lab; a.out_img = nullptr; a.out_lab = out_lab; a.mat = mat;
  a.ss[0] = ss0; a.ss[1] = ss1; a.ss[2] = ss2;
  a.os[0] = os0; a.os[1] = os1; a.os[2] = os2;
  a.S[0] = S0; a.S[1] = S1; a.S[2] = S2;
  a.O[0] = O0; a.O[1] = O1; a.O[2] = O2;
  a.alpha = 1.f; a.beta = 0.f; a.lo = -INFINITY; a.hi = INFINITY;
  a.P = lane_axis;
  const int u = (lane_axis + 1) % 3, v = (lane_axis + 2) % 3;
  a.Q = a.os[u] <= a.os[v] ? u : v;
  a.R = 3 - a.P - a.Q;
  a.transpose = a.os[a.Q] < a.os[a.P] ? 1 : 0;
  const long long blocks = (long long)cdiv(a.O[a.P], RS_T) * cdiv(a.O[a.Q], RS_T) * a.O[a.R];
  if (blocks >= (1LL << 31)) return LTU_E_SHAPE;
  const dim3 grid((unsigned)blocks), block(256);
  const bool small = (long long)(S0 - 1) * ss0 + (long long)(S1 - 1) * ss1 + (long long)(S2 - 1) * ss2 < (1LL << 31);
  if (small) hipLaunchKernelGGL((resample_vote_kernel<int>), grid, block, 0, (hipStream_t)s, a);
  else hipLaunchKernelGGL((resample_vote_kernel<long long>), grid, block, 0, (hipStream_t)s, a);
  return ltu_check_launch();
}

// ---- arg-max of resampled probabilities: lab[p] = argmax_c sample(probs[c], M (p, 1)) ------------------------------------------
// The way back of a prediction (data.to_native_probs): C planar f32 channels on the RAS grid are pulled onto the file's grid and the
// arg-max is taken there.  The coordinate, the tap offsets and the weights do not depend on the channel: they are formed once per
// output voxel, then C x 8 taps are gathered.  Same tile as above; the u8 labels (and the f32 probabilities of the classes of `mask`,
// K = popcount planes of stride ocs) go through LDS when P is not the output's fastest axis: one u8 tile and ONE f32 tile, refilled
// per selected class from the registers that hold a thread's 16 rows x C values (PROBS instantiation only).
struct ArgmaxArgs {
  const float* probs;
  uint8_t* out_lab;
  float* out_prob;
  const double* mat;                 // [3][4]: row s = source axis s
  long long cs, ocs;                 // element strides of a source channel / an output probability plane
  long long ss[3], os[3];
  int S[3], O[3];
  int P, Q, R;
  int transpose;
  unsigned mask;                     // bit c: class c's resampled probability is stored too
};

// one output voxel: v[c] = channel c resampled (bit for bit resample_grid_kernel<float> with the identity map), *vl = the first
// maximal c (strict >: torch.argmax, class_metrics.hip's label map)
template <int C, typename IDX>
__device__ __forceinline__ void argmax_one(const ArgmaxArgs& a, double c0, double c1, double c2, float* v, uint8_t* vl) {
  double c[3];
  clamp_coords(a.S, c0, c1, c2, c);
  IDX o0[3], o1[3];
  float t[3];
  tap_setup<IDX>(a.S, a.ss, c, o0, o1, t);
#pragma unroll
  for (int k = 0; k < C; ++k)        // the channel base is a 64-bit pointer offset: IDX covers one channel only
    v[k] = tap_sum<float, IDX>(a.probs + (long long)k * a.cs, o0, o1, t, 1.f, 0.f, -INFINITY, INFINITY);
  float best = v[0];
  int lab = 0;
#pragma unroll
  for (int k = 1; k < C; ++k)
    if (v[k] > best) {
      best = v[k];
      lab = k;
    }
  *vl = (uint8_t)lab;
}

template <int C, typename IDX, bool PROBS>
__device__ __forceinline__ void resample_argmax_tile(const ArgmaxArgs& a) {
  constexpr int ROWS = RS_T / 4;     // rows of the tile per thread
  __shared__ uint8_t slab[RS_T][RS_T + 4];
  __shared__ float simg[PROBS ? RS_T : 1][RS_T + 1];
  const int tilesP = (a.O[a.P] + RS_T - 1) / RS_T, tilesQ = (a.O[a.Q] + RS_T - 1) / RS_T;
  long long b = blockIdx.x;
  const int tp = (int)(b % tilesP); b /= tilesP;
  const int tq = (int)(b % tilesQ);
  const int r = (int)(b / tilesQ);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int pP = tp * RS_T + lane;
  const double m[3][4] = {{a.mat[0], a.mat[1], a.mat[2], a.mat[3]}, {a.mat[4], a.mat[5], a.mat[6], a.mat[7]},
                          {a.mat[8], a.mat[9], a.mat[10], a.mat[11]}};
  double base[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) base[s] = fma(m[s][a.R], (double)r, m[s][3]) + m[s][a.P] * (double)pP;
  const long long obase = (long long)r * a.os[a.R];
  float keep[PROBS ? ROWS : 1][C];
  auto do_row = [&](int it) {
    const int row = wv + 4 * it;
    const int pQ = tq * RS_T + row;
    float v[C];
#pragma unroll
    for (int k = 0; k < C; ++k) v[k] = 0.f;
    uint8_t vl = 0;
    const bool in = pP < a.O[a.P] && pQ < a.O[a.Q];
    if (in)
      argmax_one<C, IDX>(a, fma(m[0][a.Q], (double)pQ, base[0]), fma(m[1][a.Q], (double)pQ, base[1]),
                         fma(m[2][a.Q], (double)pQ, base[2]), v, &vl);
    if (a.transpose) {
      slab[row][lane] = vl;
      if constexpr (PROBS) {
#pragma unroll
        for (int k = 0; k < C; ++k) keep[PROBS ? it : 0][k] = v[k];
      }
    } else if (in) {
      const long long o = obase + (long long)pP * a.os[a.P] + (long long)pQ * a.os[a.Q];
      a.out_lab[o] = vl;
      if constexpr (PROBS) {
        long long plane = 0;
#pragma unroll
        for (int k = 0; k < C; ++k)
          if ((a.mask >> k) & 1u) {
            a.out_prob[plane + o] = v[k];
            plane += a.ocs;
          }
      }
    }
  };
  if (PROBS) {                       // keep[][] stays in registers only with constant indices
#pragma unroll
    for (int it = 0; it < ROWS; ++it) do_row(it);
  } else {
    for (int it = 0; it < ROWS; ++it) do_row(it);
  }
  if (!a.transpose) return;
  __syncthreads();
  const int qQ = tq * RS_T + lane;
  const int cols = min(RS_T, a.O[a.P] - tp * RS_T);
  if (qQ < a.O[a.Q])
    for (int col = wv; col < cols; col += 4)
      a.out_lab[obase + (long long)(tp * RS_T + col) * a.os[a.P] + (long long)qQ * a.os[a.Q]] = slab[lane][col];
  if (!PROBS) return;
  long long plane = 0;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    if (!((a.mask >> k) & 1u)) continue;         // uniform over the grid: every thread of the block meets the same barriers
#pragma unroll
    for (int it = 0; it < ROWS; ++it) simg[PROBS ? wv + 4 * it : 0][lane] = keep[PROBS ? it : 0][k];
    __syncthreads();
    if (qQ < a.O[a.Q])
      for (int col = wv; col < cols; col += 4)
        a.out_prob[plane + obase + (long long)(tp * RS_T + col) * a.os[a.P] + (long long)qQ * a.os[a.Q]] =
            simg[PROBS ? lane : 0][col];
    __syncthreads();                             // the tile is refilled for the next class
    plane += a.ocs;
  }
}

template <int C, typename IDX, bool PROBS>
__global__ void __launch_bounds__(256) resample_argmax_kernel(ArgmaxArgs a) {
  resample_argmax_tile<C, IDX, PROBS>(a);
}

// The label-only kernel from C = 6 up, held at 4 waves per SIMD: left to its default the compiler keeps it under 72 registers and
// waits after every one or two of the 8 C gathers of a voxel (C = 8: 1.45 ms for 819x819x125 -> 512x512x100); with the registers of 4
// waves it issues 16 before the first wait (0.96 ms).  The other instantiations are slower or spill under the same hint.
template <int C, typename IDX>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) resample_argmax_wide_kernel(ArgmaxArgs a) {
  resample_argmax_tile<C, IDX, false>(a);
}

template <int C>
static void launch_argmax(const ArgmaxArgs& a, bool small, dim3 grid, hipStream_t s) {
  const dim3 block(256);
  if (a.mask != 0) {
    if (small) hipLaunchKernelGGL((resample_argmax_kernel<C, int, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((resample_argmax_kernel<C, long long, true>), grid, block, 0, s, a);
  } else if constexpr (C >= 6) {
    if (small) hipLaunchKernelGGL((resample_argmax_wide_kernel<C, int>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((resample_argmax_wide_kernel<C, long long>), grid, block, 0, s, a);
  } else {
    if (small) hipLaunchKernelGGL((resample_argmax_kernel<C, int, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((resample_argmax_kernel<C, long long, false>), grid, block, 0, s, a);
  }
}

extern "C" int ltu_resample_argmax(const float* probs, int C, long long cs, int S0, int S1, int S2, long long ss0, long long ss1,
                                   long long ss2, uint8_t* out_lab, float* out_prob, int class_mask, long long ocs, int O0, int O1,
                                   int O2, long long os0, long long os1, long long os2, const double* mat, int lane_axis,
                                   ltu_stream_t s) {
  if (probs == nullptr || mat == nullptr || out_lab == nullptr || lane_axis < 0 || lane_axis > 2) return LTU_E_ARG;
  if (C < 2 || C > 8) return LTU_E_SHAPE;
  if (class_mask < 0 || (class_mask >> C) != 0 || (class_mask != 0 && out_prob == nullptr)) return LTU_E_ARG;
  if (S0 < 1 || S1 < 1 || S2 < 1 || O0 < 1 || O1 < 1 || O2 < 1 || ss0 < 1 || ss1 < 1 || ss2 < 1 || os0 < 1 || os1 < 1 || os2 < 1 ||
      cs < 1 || (class_mask != 0 && ocs < 1))
    return LTU_E_SHAPE;
  ArgmaxArgs a;
  a.probs = probs; a.out_lab = out_lab; a.out_prob = out_prob; a.mat = mat; a.cs = cs; a.ocs = ocs; a.mask = (unsigned)class_mask;
  a.ss[0] = ss0; a.ss[1] = ss1; a.ss[2] = ss2;
  a.os[0] = os0; a.os[1] = os1; a.os[2] = os2;
  a.S[0] = S0; a.S[1] = S1; a.S[2] = S2;
  a.O[0] = O0; a.O[1] = O1; a.O[2] = O2;
  a.P = lane_axis;
  const int u = (lane_axis + 1) % 3, v = (lane_axis + 2) % 3;
  a.Q = a.os[u] <= a.os[v] ? u : v;
  a.R = 3 - a.P - a.Q;
  a.transpose = a.os[a.Q] < a.os[a.P] ? 1 : 0;
  const long long blocks = (long long)cdiv(a.O[a.P], RS_T) * cdiv(a.O[a.Q], RS_T) * a.O[a.R];
  if (blocks >= (1LL << 31)) return LTU_E_SHAPE;
  const dim3 grid((unsigned)blocks);
  const bool small = (long long)(S0 - 1) * ss0 + (long long)(S1 - 1) * ss1 + (long long)(S2 - 1) * ss2 < (1LL << 31);
  switch (C) {
    case 2: launch_argmax<2>(a, small, grid, (hipStream_t)s); break;
    case 3: launch_argmax<3>(a, small, grid, (hipStream_t)s); break;
    case 4: launch_argmax<4>(a, small, grid, (hipStream_t)s); break;
    case 5: launch_argmax<5>(a, small, grid, (hipStream_t)s); break;
    case 6: launch_argmax<6>(a, small, grid, (hipStream_t)s); break;
    case 7: launch_argmax<7>(a, small, grid, (hipStream_t)s); break;
    default: launch_argmax<8>(a, small, grid, (hipStream_t)s); break;
  }
  return ltu_check_launch();
}

// ---- patches: crop + RandFlipd(spatial_axis 0) + RandRotate90d(spatial_axes (0, 1)) ------------------------------------------
// out[k][x][y][z] = vol[h0 + a][w0 + b][d0 + z],  (u, v) = swap ? (y, x) : (x, y),  a = flip_h ? h-1-u : u,  b = flip_w ? w-1-v : v.
// D stays fastest on both sides: a straight gather, VEC consecutive z per thread (one 16-byte f32 / 4-byte u8 store).
struct CropOrientArgs {
  int desc[LTU_CROP_ORIENT_MAX][6];
};

template <int VEC>
__global__ void __launch_bounds__(256) crop_orient_kernel(const float* __restrict__ img, const uint8_t* __restrict__ lab,
                                                          float* __restrict__ oimg, uint8_t* __restrict__ olab, CropOrientArgs c,
                                                          int n, int H, int W, int D, int h, int w, int d) {
  const int dv = d / VEC;
  const long long per = (long long)h * w * dv, total = per * n;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i / per);
    long long rr = i - (long long)k * per;
    const int z = (int)(rr % dv) * VEC; rr /= dv;
    const int y = (int)(rr % w), x = (int)(rr / w);
    const int* de = c.desc[k];
    const int u = de[5] ? y : x, v = de[5] ? x : y;
    const int aa = de[3] ? h - 1 - u : u, bb = de[4] ? w - 1 - v : v;
    const long long src = ((long long)(de[0] + aa) * W + (de[1] + bb)) * D + de[2] + z;
    const long long dst = (((long long)k * h + x) * w + y) * d + z;
    if (VEC == 4) {
      if (img != nullptr)
        *reinterpret_cast<float4*>(oimg + dst) = make_float4(img[src], img[src + 1], img[src + 2], img[src + 3]);
      if (lab != nullptr)
        *reinterpret_cast<uint32_t*>(olab + dst) =
            (uint32_t)lab[src] | ((uint32_t)lab[src + 1] << 8) | ((uint32_t)lab[src + 2] << 16) | ((uint32_t)lab[src + 3] << 24);
    } else {
      if (img != nullptr) oimg[dst] = img[src];
      if (lab != nullptr) olab[dst] = lab[src];
    }
  }
}

extern "C" int ltu_crop_orient(const float* img, const uint8_t* lab, float* out_img, uint8_t* out_lab, const int* desc, int n, int H,
                               int W, int D, int h, int w, int d, ltu_stream_t s) {
  if (desc == nullptr || (img == nullptr) != (out_img == nullptr) || (lab == nullptr) != (out_lab == nullptr) ||
      (img == nullptr && lab == nullptr) || n < 0 || n > LTU_CROP_ORIENT_MAX)
    return LTU_E_ARG;
  if (n == 0) return LTU_OK;
  if (h < 1 || w < 1 || d < 1 || h > H || w > W || d > D) return LTU_E_SHAPE;
  CropOrientArgs c;
  for (int k = 0; k < n; ++k) {
    const int* de = desc + 6 * k;
    if (de[0] < 0 || de[1] < 0 || de[2] < 0 || de[0] + h > H || de[1] + w > W || de[2] + d > D) return LTU_E_SHAPE;
    if (de[5] && h != w) return LTU_E_SHAPE;
    for (int j = 0; j < 6; ++j) c.desc[k][j] = j < 3 ? de[j] : (de[j] != 0);
  }
  const int vec = (d % 4 == 0) ? 4 : 1;
  if (vec == 4 && (((uintptr_t)out_img & 15) != 0 || ((uintptr_t)out_lab & 3) != 0)) return LTU_E_ALIGN;
  const long long total = (long long)n * h * w * (d / vec);
  long long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  if (vec == 4)
    hipLaunchKernelGGL(crop_orient_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, img, lab, out_img, out_lab, c, n,
                       H, W, D, h, w, d);
  else
    hipLaunchKernelGGL(crop_orient_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, img, lab, out_img, out_lab, c, n,
                       H, W, D, h, w, d);
  return ltu_check_launch();
}
