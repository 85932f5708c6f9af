// Signed Euclidean distance maps of label patches for the boundary loss (Kervadec et al., "Boundary loss for highly unbalanced
// segmentation"), all B x K volumes of a batch in one call.
//
// Definition (the same words are in include/ltu_hip.h and ops.signed_distance_maps): G = {label == c} inside the patch, spacing
// (s_H, s_W, s_D); phi(x) = dist(x, G) outside G, -(dist(x, not G) - 1) inside G (the 1 is not scaled by the spacing), and
// phi = 0 everywhere when G is empty or fills the patch.  Distances are Euclidean, to voxel centres, inside the patch only.
//
// One buffer carries both polarities.  After any number of separable passes the squared distance to G is 0 exactly at the voxels
// of G, and the squared distance to not-G is 0 exactly outside G, so phi itself holds, in place, +d2(x, G) outside and
// -d2(x, not G) inside; the sign bit is the membership and the label is read once, by the first pass.
//   H pass: one lane per (volume, w, d) column, lanes along d (contiguous loads and stores).  Forward sweep from the label into
//           a u16 code per voxel (membership bit + distance in voxels to the nearest voxel of the other set so far) kept in LDS,
//           backward sweep from LDS to phi.  Every lane also raises its volume's "has inside" / "has outside" flag (a plain
//           store of 1: all writers agree).
//   W pass: one lane per (volume, h, d) line, lanes along d.  Lower envelope of parabolas (Felzenszwalb-Huttenlocher) for each
//           polarity in turn; the apex stack lives in LDS laid out [entry][lane].  Volumes without a boundary are skipped.
//   D pass: the lines are contiguous, so a workgroup copies its lines into LDS with consecutive lanes on consecutive addresses,
//           runs one lane per line on the LDS copy (odd pitch: no bank conflict), and writes phi = sqrt / -(sqrt - 1) / 0 back
//           the way it came.
// The envelope's comparisons and the squared distances are formed in double and stored as fp32 between passes, as the evaluation
// EDT (surface.hip) does: with unit spacing every squared distance is an integer below 2^24 and exact.  No atomics, no host read;
// two calls give bit-identical maps.
#include "common.h"

#include <math.h>

#define DM_MAX_AXIS 512
#define DM_MAX_K 8
#define DM_LDS_BYTES 65536         // per workgroup: two workgroups share a CU's 160 KiB
#define DM_INF __builtin_inff()
#define DM_FAR 0x7FFF              // u16 code of "no voxel of the other set so far"

struct DmClasses {
  int id[DM_MAX_K];
};

__device__ __forceinline__ bool dm_neg(float v) { return (__float_as_uint(v) >> 31) != 0u; }

// ------------------------------------------------------------------------------------------------ H pass
// grid (column blocks, B K); code [H][lanes] u16 in LDS; flags [B K][2] = (has inside, has outside), zeroed before the launch
__global__ void __launch_bounds__(256) dm_h_kernel(const uint8_t* __restrict__ label, float* __restrict__ phi, int* __restrict__ flags,
                                                   DmClasses cls, int K, int H, long long WD, int lanes, float sh) {
  extern __shared__ unsigned char dm_lds[];
  uint16_t* code = reinterpret_cast<uint16_t*>(dm_lds) + threadIdx.x;
  const int vol = blockIdx.y, b = vol / K;
  const uint8_t cid = (uint8_t)cls.id[vol % K];
  const long long c = (long long)blockIdx.x * lanes + threadIdx.x;
  if ((int)threadIdx.x >= lanes || c >= WD) return;
  const uint8_t* lab = label + (long long)b * H * WD + c;
  float* o = phi + (long long)vol * H * WD + c;
  const double s2 = (double)sh * sh;
  int last_in = -1, last_out = -1;
  for (int x = 0; x < H; ++x) {                // distance to the nearest voxel of the other set at or before x
    const bool m = lab[(long long)x * WD] == cid;
    if (m) last_in = x; else last_out = x;
    const int other = m ? last_out : last_in;
    code[(long long)x * lanes] = (uint16_t)((other >= 0 ? x - other : DM_FAR) | (m ? 0x8000 : 0));
  }
  int next_in = -1, next_out = -1;
  for (int x = H - 1; x >= 0; --x) {           // the nearer of the two sides, squared, scaled and signed
    const int cd = code[(long long)x * lanes];
    const bool m = (cd & 0x8000) != 0;
    if (m) next_in = x; else next_out = x;
    const int other = m ? next_out : next_in;
    int dv = cd & 0x7FFF;
    if (other >= 0 && other - x < dv) dv = other - x;
    const float v = dv < DM_FAR ? (float)(s2 * (double)dv * (double)dv) : DM_INF;
    o[(long long)x * WD] = m ? -v : v;
  }
  if (last_in >= 0) flags[2 * vol] = 1;
  if (last_out >= 0) flags[2 * vol + 1] = 1;
}

// ------------------------------------------------------------------------------------------------ envelope of one line
// One polarity of one line of n signed values: with f(i) = |line(i)| where the sign of line(i) is `neg`, 0 elsewhere,
// line(q) <- (neg ? - : +) min_i (s2 (q - i)^2 + f(i)) at every q whose sign is `neg`; the other entries stay.  The apexes vs[] and
// their values fs[] of the envelope sit in LDS at [j * lanes].  What this writes keeps the sign it found, so the other polarity can
// run on the same line afterwards.
// The parabolas with apexes (p, gp) and (q, gq), p < q, meet at z = N / (2 s2 (q - p)) with N = (gq + s2 q^2) - (gp + s2 p^2).  No z
// is ever formed: two of them are compared by cross-multiplying (the denominators are positive and share 2 s2), one with an
// abscissa x by N < 2 s2 (q - p) x.  With unit spacing every product is an integer far below 2^53: the decisions are exact.
template <class LD, class ST>
__device__ __forceinline__ void dm_envelope(LD ld, ST st, int n, double s2, bool neg, float* fs, uint16_t* vs, int lanes) {
  auto height = [&](int v, double f) { return f + s2 * (double)v * (double)v; };
  int k = -1, vt = 0, vb = 0;                   // top of the stack; apexes of the top (vt) and of the one below it (vb)
  double ht = 0.0, hb = 0.0;                    // their heights f + s2 v^2
  for (int i = 0; i < n; ++i) {
    const float x = ld(i);
    const float f = dm_neg(x) == neg ? fabsf(x) : 0.f;
    if (!(f < DM_INF)) continue;
    const double hi = height(i, (double)f);
    // the top parabola is nowhere lowest when the new one meets it at or left of where it met the one below: pop it
    while (k >= 1 && !((hi - ht) * (double)(vt - vb) > (ht - hb) * (double)(i - vt))) {
      --k;
      vt = vb; ht = hb;
      if (k >= 1) { vb = vs[(k - 1) * lanes]; hb = height(vb, (double)fs[(k - 1) * lanes]); }
    }
    ++k;
    vs[k * lanes] = (uint16_t)i;
    fs[k * lanes] = f;
    vb = vt; hb = ht;
    vt = i; ht = hi;
  }
  if (k < 0) return;                            // no source: every entry of this polarity is already inf
  int j = 0, vj = vs[0];
  double fj = fs[0];
  double nn = 0.0, dn = 0.0;                    // the next parabola takes over right of nn / dn
  auto next = [&]() {
    const int v1 = vs[(j + 1) * lanes];
    nn = height(v1, (double)fs[(j + 1) * lanes]) - height(vj, fj);
    dn = 2.0 * s2 * (double)(v1 - vj);
  };
  if (k > 0) next();
  for (int q = 0; q < n; ++q) {
    while (j < k && nn < dn * (double)q) {
      ++j;
      vj = vs[j * lanes];
      fj = fs[j * lanes];
      if (j < k) next();
    }
    if (dm_neg(ld(q)) != neg) continue;
    const double dq = (double)(q - vj);
    const float r = (float)(s2 * dq * dq + fj);
    st(q, neg ? -r : r);
  }
}

// both polarities of one line; a polarity without a voxel of its sign on the line has nothing to write and is skipped
template <class LD, class ST>
__device__ __forceinline__ void dm_line(LD ld, ST st, int n, double s2, float* fs, uint16_t* vs, int lanes) {
  bool any_pos = false, any_neg = false;
  for (int i = 0; i < n; ++i) {
    const bool m = dm_neg(ld(i));
    any_neg |= m;
    any_pos |= !m;
  }
  if (any_pos) dm_envelope(ld, st, n, s2, false, fs, vs, lanes);
  if (any_neg) dm_envelope(ld, st, n, s2, true, fs, vs, lanes);
}

// ------------------------------------------------------------------------------------------------ W pass
// line L = (vol H + h) D + d; stack f32 [W][lanes] then u16 [W][lanes] in LDS
__global__ void __launch_bounds__(256) dm_w_kernel(float* __restrict__ phi, const int* __restrict__ flags, int H, int W, int D,
                                                   long long nlines, int lanes, float sw) {
  extern __shared__ unsigned char dm_lds[];
  float* fs = reinterpret_cast<float*>(dm_lds) + threadIdx.x;
  uint16_t* vs = reinterpret_cast<uint16_t*>(dm_lds + (size_t)4 * W * lanes) + threadIdx.x;
  const long long L = (long long)blockIdx.x * lanes + threadIdx.x;
  if ((int)threadIdx.x >= lanes || L >= nlines) return;
  const long long vh = L / D;
  const int vol = (int)(vh / H);
  if (!(flags[2 * vol] && flags[2 * vol + 1])) return;       // no boundary in this volume: the D pass writes its zeros
  float* line = phi + vh * W * D + (L - vh * D);
  const double s2 = (double)sw * sw;
  auto ld = [&](int i) { return line[(long long)i * D]; };
  auto st = [&](int i, float v) { line[(long long)i * D] = v; };
  dm_line(ld, st, W, s2, fs, vs, lanes);
}

// ------------------------------------------------------------------------------------------------ D pass + the map itself
// workgroup = `lanes` consecutive lines (vol, h, w) = one contiguous run of phi.  LDS: copy f32 [lanes][pitch] (pitch odd), stack
// f32 [D][lanes], u16 [D][lanes]
__global__ void __launch_bounds__(256) dm_d_kernel(float* __restrict__ phi, const int* __restrict__ flags, long long HW, int D,
                                                   long long nlines, int lanes, int pitch, float sd) {
  extern __shared__ unsigned char dm_lds[];
  float* copy = reinterpret_cast<float*>(dm_lds);
  float* fs = copy + (size_t)lanes * pitch;
  uint16_t* vs = reinterpret_cast<uint16_t*>(fs + (size_t)D * lanes);
  const long long L0 = (long long)blockIdx.x * lanes;
  const int nl = (int)(nlines - L0 < lanes ? nlines - L0 : lanes);
  float* run = phi + L0 * D;
  const int total = nl * D;
  for (int e = threadIdx.x; e < total; e += blockDim.x) copy[(e / D) * pitch + e % D] = run[e];
  __syncthreads();
  if ((int)threadIdx.x < nl) {
    const int vol = (int)((L0 + threadIdx.x) / HW);
    if (flags[2 * vol] && flags[2 * vol + 1]) {
      float* line = copy + (size_t)threadIdx.x * pitch;
      const double s2 = (double)sd * sd;
      auto ld = [&](int i) { return line[i]; };
      auto st = [&](int i, float v) { line[i] = v; };
      dm_line(ld, st, D, s2, fs + threadIdx.x, vs + threadIdx.x, lanes);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    const int l = e / D;
    const int vol = (int)((L0 + l) / HW);
    const float v = copy[l * pitch + e % D];
    float out = 0.f;                            // empty or full class: no boundary in sight
    if (flags[2 * vol] && flags[2 * vol + 1] && fabsf(v) < DM_INF)
      out = dm_neg(v) ? (float)(1.0 - sqrt((double)-v)) : sqrtf(v);      // inside: the subtraction in double keeps the last bit
    run[e] = out;
  }
}

// ------------------------------------------------------------------------------------------------ host
// lanes (= lines) of a workgroup whose lines need `per_lane` bytes of LDS each
static int dm_lanes(long long per_lane) {
  const long long l = DM_LDS_BYTES / per_lane;
  return l >= 256 ? 256 : l >= 64 ? (int)(l / 64 * 64) : (int)l;
}
static int dm_threads(int lanes) { return lanes < 64 ? 64 : lanes; }

extern "C" long long ltu_distmap_scratch_elems(int B, int K, int H, int W, int D) {
  if (B <= 0 || K <= 0 || H <= 0 || W <= 0 || D <= 0) return 0;
  return 2LL * B * K;
}

extern "C" int ltu_distmap_signed(const uint8_t* label, const int* classes, int K, float* phi, void* scratch, long long scratch_elems,
                                  int B, int H, int W, int D, float sh, float sw, float sd, ltu_stream_t s) {
  if (B <= 0 || K < 1 || K > DM_MAX_K || H <= 0 || W <= 0 || D <= 0) return LTU_E_SHAPE;
  if (H > DM_MAX_AXIS || W > DM_MAX_AXIS || D > DM_MAX_AXIS || (long long)B * K > 65535) return LTU_E_SHAPE;
  if (classes == nullptr) return LTU_E_ARG;
  DmClasses cls;
  for (int k = 0; k < DM_MAX_K; ++k) cls.id[k] = -1;
  for (int k = 0; k < K; ++k) {
    if (classes[k] < 0 || classes[k] > 255) return LTU_E_ARG;
    for (int j = 0; j < k; ++j)
      if (classes[j] == classes[k]) return LTU_E_ARG;
    cls.id[k] = classes[k];
  }
  if (!(sh > 0.f) || !(sw > 0.f) || !(sd > 0.f) || !(sh < DM_INF) || !(sw < DM_INF) || !(sd < DM_INF)) return LTU_E_ARG;
  if (label == nullptr || phi == nullptr || scratch == nullptr || scratch_elems < ltu_distmap_scratch_elems(B, K, H, W, D))
    return LTU_E_ARG;
  const int V = B * K;
  const long long WD = (long long)W * D, HW = (long long)H * W;
  const int lh = dm_lanes(2LL * H), lw = dm_lanes(6LL * W);
  const int pitch = D | 1, ld = dm_lanes(4LL * pitch + 6LL * D);
  const long long lines_w = (long long)V * H * D, lines_d = (long long)V * HW;
  const long long blocks_w = (lines_w + lw - 1) / lw, blocks_d = (lines_d + ld - 1) / ld;
  if (blocks_w > 0x7FFFFFFFLL || blocks_d > 0x7FFFFFFFLL) return LTU_E_SHAPE;
  int* flags = (int*)scratch;
  hipStream_t st = (hipStream_t)s;
  hipError_t e = hipMemsetAsync(flags, 0, sizeof(int) * 2 * (size_t)V, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(dm_h_kernel, dim3(cdiv(WD, lh), V), dim3(dm_threads(lh)), (size_t)2 * H * lh, st, label, phi, flags, cls, K, H, WD,
                     lh, sh);
  hipLaunchKernelGGL(dm_w_kernel, dim3((unsigned)blocks_w), dim3(dm_threads(lw)), (size_t)6 * W * lw, st, phi, flags, H, W, D, lines_w,
                     lw, sw);
  hipLaunchKernelGGL(dm_d_kernel, dim3((unsigned)blocks_d), dim3(dm_threads(ld)), (size_t)ld * (4 * pitch + 6 * D), st, phi, flags, HW,
                     D, lines_d, ld, pitch, sd);
  return ltu_check_launch();
}
