// Cubic B-spline resampling of a scan (nnU-Net's image interpolation; the reference driver's Spacingd is trilinear, resample.hip):
// ltu_spline_prefilter turns the stored voxels into B-spline coefficients, ltu_resample_spline gathers them through the same float64
// pull matrix, coordinates and tiles as ltu_resample_grid.  Per SOURCE axis the order is 3 (cubic), 1 (linear) or 0 (nearest), so
// that the coarse axis of an anisotropic scan can be taken on its own.
#include "common.h"
#include "resample_coords.h"

// ---- prefilter -------------------------------------------------------------------------------------------------------------------
// scipy.ndimage.spline_filter1d(order 3, mode 'mirror') per filtered axis, in fp32: samples times the gain 6, then
//   c+[0] = sum_k z^k s[mirror(k)],  c+[i] = s[i] + z c+[i-1],  c[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]),  c[i] = z (c[i+1] - c+[i]).
// The start sum is the exact periodic-mirror sum (period 2 n - 2) for n <= SP_HORIZON and is cut after SP_HORIZON terms above that:
// |z|^24 = 1.9e-14, six orders below the fp32 resolution of the sum (6e-8).
// Passes (bytes per voxel, S = the source's element size):
//   axis 0, order 3: spline_x_kernel, 16 rows x 64 columns per LDS tile, one wave per 16 rows.  Forward sweep: read S (mapped as it is
//                    loaded), write 4 (c+); backward sweep: read 4, write 4.                                   S + 12 bytes
//   axis 0, other:   spline_map_kernel, read S, write 4.                                                      S + 4 bytes
//   axis 1 / 2, order 3: spline_line_kernel in place, lanes along axis 0, every thread walks its line: forward read 4 write 4,
//                    backward read 4 write 4.                                                                  16 bytes each
#define SP_T 64
#define SP_ROWS 16
#define SP_HORIZON 24
#define SP_CHUNK 16
static constexpr double SP_ZD = -0.26794919243112270647;          // sqrt(3) - 2
static constexpr float SP_Z = (float)SP_ZD;
static constexpr float SP_GAIN = 6.f;                             // (1 - z) (1 - 1 / z)
static constexpr float SP_LAST = (float)(SP_ZD / (SP_ZD * SP_ZD - 1.0));

template <typename T>
__device__ __forceinline__ float sp_load(const T* __restrict__ p, float alpha, float beta, float lo, float hi) {
  return fminf(fmaxf(fmaf(alpha, (float)*p, beta), lo), hi);
}

// c+[0] of a line of n >= 2 samples; s(k) = sample k times the gain.  Fixed order: Horner from the far end (n > SP_HORIZON), or
// scipy's closed form of the periodic sum, c0 = (s0 + z^(n-1) s[n-1] + sum_{i=1}^{n-2} z^i (s[i] + z^(n-1) s[n-1-i])) / (1 - z^(2n-2)).
template <typename F>
__device__ __forceinline__ float sp_causal_init(int n, F s) {
  if (n > SP_HORIZON) {
    float sum = s(SP_HORIZON - 1);
    for (int k = SP_HORIZON - 2; k >= 0; --k) sum = fmaf(SP_Z, sum, s(k));
    return sum;
  }
  float zn = SP_Z;
  for (int i = 2; i < n; ++i) zn *= SP_Z;
  float c0 = fmaf(zn, s(n - 1), s(0));
  float zi = SP_Z;
  for (int i = 1; i < n - 1; ++i) {
    c0 = fmaf(zi, fmaf(zn, s(n - 1 - i), s(i)), c0);
    zi *= SP_Z;
  }
  return c0 / fmaf(-zn, zn, 1.f);
}

struct PrefilterArgs {
  const void* src;
  float* coef;
  long long ss[3];
  int S[3];
  float alpha, beta, lo, hi;
};

// axis 0 is not filtered: coef = map(src), dense
template <typename T>
__global__ void __launch_bounds__(256) spline_map_kernel(PrefilterArgs a) {
  const T* src = (const T*)a.src;
  const long long total = (long long)a.S[0] * a.S[1] * a.S[2];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % a.S[0]);
    const long long r = i / a.S[0];
    const int y = (int)(r % a.S[1]), z = (int)(r / a.S[1]);
    a.coef[i] = sp_load(src + x * a.ss[0] + y * a.ss[1] + z * a.ss[2], a.alpha, a.beta, a.lo, a.hi);
  }
}

// axis 0 filtered.  One wave owns SP_ROWS rows (a row = one line along axis 0) and walks them tile by tile: a tile of SP_ROWS x 64 is
// loaded with the lanes along the line (coalesced), walked in LDS with one lane per row (row stride 65 words: conflict-free both ways),
// and stored with the lanes along the line again.  16 rows, not 64: the walk is a sliver of the time, the loads' latency is most of
// it, and a 512 x 512 x 100 scan then gives 3200 waves to hide it instead of 800.  The recursion state (c+[i-1], c+[i-2] forward, c[i+1] backward) stays in the lane's registers from tile
// to tile.  The forward sweep leaves c+ in coef, the backward sweep reads it back and leaves c.
template <typename T>
__global__ void __launch_bounds__(SP_T) spline_x_kernel(PrefilterArgs a) {
  __shared__ float tile[SP_ROWS][SP_T + 1];
  const T* src = (const T*)a.src;
  const int lane = threadIdx.x;
  const int n = a.S[0];
  const long long rows = (long long)a.S[1] * a.S[2];
  const long long r0 = (long long)blockIdx.x * SP_ROWS;
  const int nrows = (int)(rows - r0 < SP_ROWS ? rows - r0 : SP_ROWS);
  const int tiles = (n + SP_T - 1) / SP_T;
  const bool walker = lane < nrows;
  float p1 = 0.f, p2 = 0.f;
  for (int t = 0; t < tiles; ++t) {
    const int col = t * SP_T + lane;
    const int ncol = n - t * SP_T < SP_T ? n - t * SP_T : SP_T;
    if (col < n) {
      int y = (int)(r0 % a.S[1]), z = (int)(r0 / a.S[1]);
      for (int i = 0; i < nrows; ++i) {
        tile[i][lane] = SP_GAIN * sp_load(src + col * a.ss[0] + y * a.ss[1] + z * a.ss[2], a.alpha, a.beta, a.lo, a.hi);
        if (++y == a.S[1]) {
          y = 0;
          ++z;
        }
      }
    }
    __syncthreads();
    if (walker) {
      int k = 0;
      if (t == 0) {                    // the start sum reads the first min(n, SP_HORIZON) <= 64 samples: all in tile 0
        p1 = sp_causal_init(n, [&](int j) { return tile[lane][j]; });
        tile[lane][0] = p1;
        k = 1;
      }
      for (; k < ncol; ++k) {
        p2 = p1;
        p1 = fmaf(SP_Z, p1, tile[lane][k]);
        tile[lane][k] = p1;
      }
    }
    __syncthreads();
    if (col < n)
      for (int i = 0; i < nrows; ++i) a.coef[(r0 + i) * n + col] = tile[i][lane];
    __syncthreads();
  }
  float nx = 0.f;
  for (int t = tiles - 1; t >= 0; --t) {
    const int col = t * SP_T + lane;
    const int ncol = n - t * SP_T < SP_T ? n - t * SP_T : SP_T;
    if (col < n)
      for (int i = 0; i < nrows; ++i) tile[i][lane] = a.coef[(r0 + i) * n + col];
    __syncthreads();
    if (walker) {
      int k = ncol - 1;
      if (t == tiles - 1) {
        nx = SP_LAST * fmaf(SP_Z, p2, p1);
        tile[lane][k] = nx;
        --k;
      }
      for (; k >= 0; --k) {
        nx = SP_Z * (nx - tile[lane][k]);
        tile[lane][k] = nx;
      }
    }
    __syncthreads();
    if (col < n)
      for (int i = 0; i < nrows; ++i) a.coef[(r0 + i) * n + col] = tile[i][lane];
    __syncthreads();
  }
}

// axis 1 or 2 filtered, in place.  Line l = (x, o): base x + o * ostride, n samples `stride` apart; consecutive threads take
// consecutive x, so every load and store of a wave is one run of 64 floats (broken only where a row of axis 0 ends).  SP_CHUNK
// samples are loaded before the recursion runs over them, so that the loads of a chunk are in flight together.
__global__ void __launch_bounds__(SP_T) spline_line_kernel(float* __restrict__ coef, int S0, long long lines, long long ostride,
                                                           int n, long long stride) {
  const long long l = (long long)blockIdx.x * SP_T + threadIdx.x;
  if (l >= lines) return;
  float* p = coef + (l % S0) + (l / S0) * ostride;
  float p1 = sp_causal_init(n, [&](int j) { return SP_GAIN * p[j * stride]; });
  float p2 = 0.f;
  p[0] = p1;
  for (int k0 = 1; k0 < n; k0 += SP_CHUNK) {
    float v[SP_CHUNK];
#pragma unroll
    for (int j = 0; j < SP_CHUNK; ++j) v[j] = k0 + j < n ? p[(k0 + j) * stride] : 0.f;
#pragma unroll
    for (int j = 0; j < SP_CHUNK; ++j)
      if (k0 + j < n) {
        p2 = p1;
        p1 = fmaf(SP_Z, p1, SP_GAIN * v[j]);
        p[(k0 + j) * stride] = p1;
      }
  }
  float nx = SP_LAST * fmaf(SP_Z, p2, p1);
  p[(n - 1) * stride] = nx;
  for (int k0 = n - 2; k0 >= 0; k0 -= SP_CHUNK) {
    float v[SP_CHUNK];
#pragma unroll
    for (int j = 0; j < SP_CHUNK; ++j) v[j] = k0 - j >= 0 ? p[(k0 - j) * stride] : 0.f;
#pragma unroll
    for (int j = 0; j < SP_CHUNK; ++j)
      if (k0 - j >= 0) {
        nx = SP_Z * (nx - v[j]);
        p[(k0 - j) * stride] = nx;
      }
  }
}

static bool sp_order_ok(int o) { return o == 0 || o == 1 || o == 3; }

extern "C" int ltu_spline_prefilter(const void* src, int src_dtype, int S0, int S1, int S2, long long ss0, long long ss1,
                                    long long ss2, float* coef, int order0, int order1, int order2, float alpha, float beta, float lo,
                                    float hi, ltu_stream_t s) {
  if (src == nullptr || coef == nullptr || !sp_order_ok(order0) || !sp_order_ok(order1) || !sp_order_ok(order2) || alpha != alpha ||
      beta != beta || lo != lo || hi != hi)
    return LTU_E_ARG;
  if (src_dtype != LTU_F32 && src_dtype != LTU_U8 && src_dtype != LTU_I16) return LTU_E_DTYPE;
  if (S0 < 1 || S1 < 1 || S2 < 1 || ss0 < 1 || ss1 < 1 || ss2 < 1) return LTU_E_SHAPE;
  const long long total = (long long)S0 * S1 * S2;
  if (total >= (1LL << 31)) return LTU_E_SHAPE;
  PrefilterArgs a;
  a.src = src; a.coef = coef;
  a.ss[0] = ss0; a.ss[1] = ss1; a.ss[2] = ss2;
  a.S[0] = S0; a.S[1] = S1; a.S[2] = S2;
  a.alpha = alpha; a.beta = beta; a.lo = lo; a.hi = hi;
  hipStream_t st = (hipStream_t)s;
  if (order0 == 3 && S0 > 1) {
    const dim3 grid(cdiv((long long)S1 * S2, SP_ROWS)), block(SP_T);
    if (src_dtype == LTU_U8) hipLaunchKernelGGL(spline_x_kernel<uint8_t>, grid, block, 0, st, a);
    else if (src_dtype == LTU_I16) hipLaunchKernelGGL(spline_x_kernel<int16_t>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(spline_x_kernel<float>, grid, block, 0, st, a);
  } else {
    long long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    const dim3 grid((unsigned)blocks), block(256);
    if (src_dtype == LTU_U8) hipLaunchKernelGGL(spline_map_kernel<uint8_t>, grid, block, 0, st, a);
    else if (src_dtype == LTU_I16) hipLaunchKernelGGL(spline_map_kernel<int16_t>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(spline_map_kernel<float>, grid, block, 0, st, a);
  }
  if (order1 == 3 && S1 > 1) {
    const long long lines = (long long)S0 * S2;
    hipLaunchKernelGGL(spline_line_kernel, dim3(cdiv(lines, SP_T)), dim3(SP_T), 0, st, coef, S0, lines, (long long)S0 * S1, S1,
                       (long long)S0);
  }
  if (order2 == 3 && S2 > 1) {
    const long long lines = (long long)S0 * S1;
    hipLaunchKernelGGL(spline_line_kernel, dim3(cdiv(lines, SP_T)), dim3(SP_T), 0, st, coef, S0, lines, (long long)S0, S2,
                       (long long)S0 * S1);
  }
  return ltu_check_launch();
}

// ---- gather ----------------------------------------------------------------------------------------------------------------------
// Tile, lane axis and the LDS transpose as resample_grid_kernel (resample.hip).  N0, N1, N2 = taps per source axis: 4 (order 3), 2
// (order 1), 1 (order 0).  A voxel keeps N0 + N1 + N2 offsets and weights, not N0 N1 N2 of either; the N0 taps along axis 0 (adjacent
// floats) form the inner fused multiply-add chain.
struct SplineArgs {
  const float* coef;
  float* out;
  const double* mat;                 // [3][4]: row s = source axis s
  long long os[3];
  int S[3], O[3];
  int P, Q, R;
  int transpose;
  float lo, hi;
};

// sp_mirror and sp_cubic_weights: resample_coords.h
template <int N>
__device__ __forceinline__ void sp_axis_taps(int n, int stride, double c, int* off, float* w) {
  if (N == 1) {
    off[0] = (int)floor(c + 0.5) * stride;         // c <= n - 1: the tap is inside
    w[0] = 1.f;
    return;
  }
  const double f = floor(c);
  const int i = (int)f;
  const float t = (float)(c - f);
  if (N == 2) {
    off[0] = i * stride;
    off[1] = sp_mirror(i + 1, n) * stride;         // i + 1 = n only with t = 0
    w[0] = 1.f - t;
    w[1] = t;
    return;
  }
  sp_cubic_weights(t, w);
#pragma unroll
  for (int j = 0; j < 4; ++j) off[j] = sp_mirror(i - 1 + j, n) * stride;
}

// the tap sum in its fixed order; o0 are the axis-0 offsets relative to coef
template <int N0, int N1, int N2>
__device__ __forceinline__ float sp_tap_sum(const float* __restrict__ coef, const int* o0, const int* o1, const int* o2,
                                            const float* w0, const float* w1, const float* w2) {
  // the N1 N0 taps of one index along axis 2 are loaded before the first is used, so that they are in flight together (left to
  // itself the compiler waits for every row before it asks for the next)
  float acc = 0.f;
#pragma unroll
  for (int k2 = 0; k2 < N2; ++k2) {
    float v[N1][N0];
#pragma unroll
    for (int k1 = 0; k1 < N1; ++k1) {
      const float* __restrict__ p = coef + (o2[k2] + o1[k1]);
#pragma unroll
      for (int k0 = 0; k0 < N0; ++k0) v[k1][k0] = p[o0[k0]];
    }
#pragma unroll
    for (int k1 = 0; k1 < N1; ++k1) {
      float row = w0[0] * v[k1][0];
#pragma unroll
      for (int k0 = 1; k0 < N0; ++k0) row = fmaf(w0[k0], v[k1][k0], row);
      acc = fmaf(w2[k2] * w1[k1], row, acc);
    }
  }
  return acc;
}

template <int N0, int N1, int N2>
__device__ __forceinline__ float spline_one(const SplineArgs& a, double c0, double c1, double c2) {
  double c[3];
  clamp_coords(a.S, c0, c1, c2, c);
  int o0[N0], o1[N1], o2[N2];
  float w0[N0], w1[N1], w2[N2];
  sp_axis_taps<N0>(a.S[0], 1, c[0], o0, w0);
  sp_axis_taps<N1>(a.S[1], a.S[0], c[1], o1, w1);
  sp_axis_taps<N2>(a.S[2], a.S[0] * a.S[1], c[2], o2, w2);
  float acc;
  // away from the ends of axis 0 no tap is mirrored and the four are adjacent floats: the same sum with the offsets 0 .. 3 as
  // constants, which the loads then carry as immediates instead of four 64-bit address additions per row
  bool inner = false;
  if constexpr (N0 == 4) inner = o0[1] == o0[0] + 1 && o0[2] == o0[0] + 2 && o0[3] == o0[0] + 3;
  if (inner) {
    const int adjacent[4] = {0, 1, 2, 3};
    acc = sp_tap_sum<N0, N1, N2>(a.coef + o0[0], adjacent, o1, o2, w0, w1, w2);
  } else {
    acc = sp_tap_sum<N0, N1, N2>(a.coef, o0, o1, o2, w0, w1, w2);
  }
  return fminf(fmaxf(acc, a.lo), a.hi);
}

template <int N0, int N1, int N2>
__global__ void __launch_bounds__(256) resample_spline_kernel(SplineArgs a) {
  __shared__ float simg[SP_T][SP_T + 1];
  const int tilesP = (a.O[a.P] + SP_T - 1) / SP_T, tilesQ = (a.O[a.Q] + SP_T - 1) / SP_T;
  long long b = blockIdx.x;
  const int tp = (int)(b % tilesP); b /= tilesP;
  const int tq = (int)(b % tilesQ);
  const int r = (int)(b / tilesQ);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int pP = tp * SP_T + lane;
  const double m[3][4] = {{a.mat[0], a.mat[1], a.mat[2], a.mat[3]}, {a.mat[4], a.mat[5], a.mat[6], a.mat[7]},
                          {a.mat[8], a.mat[9], a.mat[10], a.mat[11]}};
  double base[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) base[s] = fma(m[s][a.R], (double)r, m[s][3]) + m[s][a.P] * (double)pP;
  const long long obase = (long long)r * a.os[a.R];
  for (int row = wv; row < SP_T; row += 4) {
    const int pQ = tq * SP_T + row;
    float v = 0.f;
    const bool in = pP < a.O[a.P] && pQ < a.O[a.Q];
    if (in)
      v = spline_one<N0, N1, N2>(a, fma(m[0][a.Q], (double)pQ, base[0]), fma(m[1][a.Q], (double)pQ, base[1]),
                                 fma(m[2][a.Q], (double)pQ, base[2]));
    if (a.transpose) simg[row][lane] = v;
    else if (in) a.out[obase + (long long)pP * a.os[a.P] + (long long)pQ * a.os[a.Q]] = v;
  }
  if (!a.transpose) return;
  __syncthreads();
  const int qQ = tq * SP_T + lane;
  if (qQ >= a.O[a.Q]) return;
  for (int col = wv; col < SP_T; col += 4) {
    const int qP = tp * SP_T + col;
    if (qP >= a.O[a.P]) break;
    a.out[obase + (long long)qP * a.os[a.P] + (long long)qQ * a.os[a.Q]] = simg[lane][col];
  }
}

static int sp_taps(int order) { return order == 3 ? 4 : order + 1; }

extern "C" int ltu_resample_spline(const float* coef, int S0, int S1, int S2, int order0, int order1, int order2, float* out, int O0,
                                   int O1, int O2, long long os0, long long os1, long long os2, const double* mat, int lane_axis,
                                   float lo, float hi, ltu_stream_t s) {
  if (coef == nullptr || out == nullptr || mat == nullptr || lane_axis < 0 || lane_axis > 2 || lo != lo || hi != hi ||
      !sp_order_ok(order0) || !sp_order_ok(order1) || !sp_order_ok(order2))
    return LTU_E_ARG;
  // built: order 3 on every axis, or on two axes with 0 or 1 on the third (7 of the 27 triples)
  if ((order0 == 3) + (order1 == 3) + (order2 == 3) < 2) return LTU_E_ARG;
  if (S0 < 1 || S1 < 1 || S2 < 1 || O0 < 1 || O1 < 1 || O2 < 1 || os0 < 1 || os1 < 1 || os2 < 1) return LTU_E_SHAPE;
  if ((long long)S0 * S1 * S2 >= (1LL << 31)) return LTU_E_SHAPE;
  SplineArgs a;
  a.coef = coef; a.out = out; a.mat = mat; a.lo = lo; a.hi = hi;
  a.os[0] = os0; a.os[1] = os1; a.os[2] = os2;
  a.S[0] = S0; a.S[1] = S1; a.S[2] = S2;
  a.O[0] = O0; a.O[1] = O1; a.O[2] = O2;
  // Q = the other axis with the smaller output stride; the tile is transposed through LDS when Q is faster than P
  a.P = lane_axis;
  const int u = (lane_axis + 1) % 3, v = (lane_axis + 2) % 3;
  a.Q = a.os[u] <= a.os[v] ? u : v;
  a.R = 3 - a.P - a.Q;
  a.transpose = a.os[a.Q] < a.os[a.P] ? 1 : 0;
  const long long blocks = (long long)cdiv(a.O[a.P], SP_T) * cdiv(a.O[a.Q], SP_T) * a.O[a.R];
  if (blocks >= (1LL << 31)) return LTU_E_SHAPE;
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t st = (hipStream_t)s;
  switch (sp_taps(order0) * 100 + sp_taps(order1) * 10 + sp_taps(order2)) {
    case 444: hipLaunchKernelGGL((resample_spline_kernel<4, 4, 4>), grid, block, 0, st, a); break;
    case 144: hipLaunchKernelGGL((resample_spline_kernel<1, 4, 4>), grid, block, 0, st, a); break;
    case 244: hipLaunchKernelGGL((resample_spline_kernel<2, 4, 4>), grid, block, 0, st, a); break;
    case 414: hipLaunchKernelGGL((resample_spline_kernel<4, 1, 4>), grid, block, 0, st, a); break;
    case 424: hipLaunchKernelGGL((resample_spline_kernel<4, 2, 4>), grid, block, 0, st, a); break;
    case 441: hipLaunchKernelGGL((resample_spline_kernel<4, 4, 1>), grid, block, 0, st, a); break;
    case 442: hipLaunchKernelGGL((resample_spline_kernel<4, 4, 2>), grid, block, 0, st, a); break;
    default: return LTU_E_ARG;
  }
  return ltu_check_launch();
}
