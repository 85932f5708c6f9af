// Guarded AdamW step on the flat gradient buckets: global gradient norm (clipping), non-finite skip and weight EMA.
//   per bucket   ltu_grad_sumsq     sum of (g * grad_scale)^2, one fp32 partial per workgroup into the caller's scratch row
//   once         ltu_adamw_guard    folds the partials of ALL buckets in fp64 -> guard state (norm, coef, skip, counters, bias corrections)
//   per bucket   ltu_adamw_guarded  adamw_kernel's arithmetic (misc.hip) with coef / bc1 / bc2 / skip read from the guard state, + EMA
//   per bucket   ltu_sgd_guarded    the SGD family behind the same two guard launches (below, with its plain form ltu_sgd)
// Nothing is read back and nothing is atomic: the partial count is a function of n alone and every fold runs in a fixed order, so
// two calls on the same buckets give the same bits, and every rank of a data-parallel run takes the same decision from its own
// copy of the reduced buckets.
#include <math.h>

#include "common.h"

// the guard state record of include/ltu_hip.h (12 32-bit words, 16-byte aligned, zero-filled once by the caller)
struct GuardState {
  float norm, coef, bc1, bc2;
  int skip, reserved0;
  long long applied, skipped;
  long long reserved1;
};
static_assert(sizeof(GuardState) == LTU_GUARD_STATE_BYTES, "guard state layout");

// the launch width of both per-bucket kernels: a function of n only, capped as ltu_adamw caps it
static inline long long optim_blocks(long long n) {
  long long blocks = ((n >> 2) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  return blocks;
}

__global__ void __launch_bounds__(256) grad_sumsq_kernel(const float* __restrict__ g, long long n, float gscale, float* __restrict__ part) {
  __shared__ float s_wave[4];
  const long long nv = n >> 2;
  float acc = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) {
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gg = f4at(gv, k) * gscale;
      acc += gg * gg;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {        // tail
    const float gg = g[(nv << 2) + threadIdx.x] * gscale;
    acc += gg * gg;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// b^t by squaring, in double (t >= 1)
__device__ __forceinline__ double pow_int(double b, long long t) {
  double r = 1.0;
  for (; t > 0; t >>= 1, b *= b)
    if (t & 1) r *= b;
  return r;
}

// one workgroup: thread t folds partials [t * chunk, (t + 1) * chunk) in index order, thread 0 folds the 256 chunk sums in index order
__global__ void __launch_bounds__(256) adamw_guard_kernel(const float* __restrict__ part, long long parts, GuardState* __restrict__ state,
                                                          float gscale, float max_norm, int skip_nonfinite, float b1, float b2) {
  __shared__ double s_sum[256];
  const long long chunk = (parts + 255) / 256, i0 = threadIdx.x * chunk;
  const long long i1 = i0 + chunk < parts ? i0 + chunk : parts;
  double acc = 0.0;
  for (long long i = i0; i < i1; ++i) acc += (double)part[i];
  s_sum[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  for (int t = 0; t < 256; ++t) sum += s_sum[t];
  const float norm = (float)sqrt(sum);                   // NaN / inf partials (an overflowed square included) stay NaN / inf
  const bool finite = fabsf(norm) <= 3.402823466e38f;    // false for NaN
  const int skip = skip_nonfinite && !finite;
  float coef = gscale;
  if (max_norm > 0.f) coef *= fminf(1.f, max_norm / (norm + 1e-6f));      // torch.nn.utils.clip_grad_norm_'s coefficient
  state->norm = norm;
  state->skip = skip;
  if (skip) {
    state->coef = 0.f;
    state->skipped += 1;
    return;
  }
  const long long t = state->applied + 1;
  state->applied = t;
  state->coef = coef;
  state->bc1 = (float)(1.0 - pow_int((double)b1, t));
  state->bc2 = (float)(1.0 - pow_int((double)b2, t));
}

template <bool EMA>
__global__ void __launch_bounds__(256) adamw_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, float* __restrict__ ema, long long n, float lr, float b1,
                                                            float b2, float eps, float wd, float d, const GuardState* __restrict__ state) {
  if (state->skip) return;                               // uniform: the whole launch leaves every buffer untouched
  const float gscale = state->coef, bc1 = state->bc1, bc2 = state->bc2;
  const long long nv = n >> 2;
  const float step_size = lr / bc1, inv_sqrt_bc2 = rsqrtf(bc2), decay = 1.f - lr * wd;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i], mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 ev;
    if (EMA) ev = reinterpret_cast<float4*>(ema)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gg = f4at(gv, k) * gscale;
      const float mm = b1 * f4at(mv, k) + (1.f - b1) * gg;
      const float v2 = b2 * f4at(vv, k) + (1.f - b2) * gg * gg;
      f4at(mv, k) = mm; f4at(vv, k) = v2;
      f4at(pv, k) = f4at(pv, k) * decay - step_size * mm / (sqrtf(v2) * inv_sqrt_bc2 + eps);
      if (EMA) f4at(ev, k) = d * f4at(ev, k) + (1.f - d) * f4at(pv, k);
    }
    reinterpret_cast<float4*>(p)[i] = pv; reinterpret_cast<float4*>(m)[i] = mv; reinterpret_cast<float4*>(v)[i] = vv;
    if (EMA) reinterpret_cast<float4*>(ema)[i] = ev;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {        // tail
    const long long i = (nv << 2) + threadIdx.x;
    const float gg = g[i] * gscale;
    const float mm = b1 * m[i] + (1.f - b1) * gg;
    const float v2 = b2 * v[i] + (1.f - b2) * gg * gg;
    m[i] = mm; v[i] = v2;
    const float pn = p[i] * decay - step_size * mm / (sqrtf(v2) * inv_sqrt_bc2 + eps);
    p[i] = pn;
    if (EMA) ema[i] = d * ema[i] + (1.f - d) * pn;
  }
}

extern "C" long long ltu_grad_sumsq_parts(long long n) { return n <= 0 ? 0 : optim_blocks(n); }

extern "C" int ltu_grad_sumsq(const float* g, long long n, float grad_scale, float* scratch, long long scratch_floats, ltu_stream_t s) {
  if (n <= 0) return LTU_OK;
  if (g == nullptr || scratch == nullptr || ((uintptr_t)g & 15) || ((uintptr_t)scratch & 3)) return LTU_E_ARG;
  const long long blocks = optim_blocks(n);
  if (scratch_floats < blocks) return LTU_E_ARG;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, g, n, grad_scale, scratch);
  return ltu_check_launch();
}

extern "C" int ltu_adamw_guard(const float* scratch, long long parts, void* state, float grad_scale, float max_norm, int skip_nonfinite,
                               float beta1, float beta2, ltu_stream_t s) {
  if (parts < 0 || (parts > 0 && scratch == nullptr) || ((uintptr_t)scratch & 3)) return LTU_E_ARG;
  if (state == nullptr || ((uintptr_t)state & 15) || max_norm != max_norm) return LTU_E_ARG;
  hipLaunchKernelGGL(adamw_guard_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, scratch, parts, (GuardState*)state, grad_scale, max_norm,
                     skip_nonfinite, beta1, beta2);
  return ltu_check_launch();
}

extern "C" int ltu_adamw_guarded(float* p, const float* g, float* m, float* v, float* ema, long long n, float lr, float beta1, float beta2,
                                 float eps, float weight_decay, float ema_decay, const void* state, ltu_stream_t s) {
  if (state == nullptr || ((uintptr_t)state & 15)) return LTU_E_ARG;
  if (ema != nullptr && !(ema_decay >= 0.f && ema_decay < 1.f)) return LTU_E_ARG;
  if (n <= 0) return LTU_OK;
  if (p == nullptr || g == nullptr || m == nullptr || v == nullptr) return LTU_E_ARG;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) return LTU_E_ARG;
  const dim3 grid((unsigned)optim_blocks(n)), block(256);
  if (ema != nullptr)
    hipLaunchKernelGGL(adamw_guarded_kernel<true>, grid, block, 0, (hipStream_t)s, p, g, m, v, ema, n, lr, beta1, beta2, eps, weight_decay,
                       ema_decay, (const GuardState*)state);
  else
    hipLaunchKernelGGL(adamw_guarded_kernel<false>, grid, block, 0, (hipStream_t)s, p, g, m, v, ema, n, lr, beta1, beta2, eps, weight_decay,
                       0.f, (const GuardState*)state);
  return ltu_check_launch();
}

// ------------------------------------------------------------------------------------------------ SGD (momentum, Nesterov)
// torch.optim.SGD's arithmetic per element on the same flat buckets, with the same guard (ltu_grad_sumsq + ltu_adamw_guard with
// betas of 0: the norm, the decision and the counters are the optimizer-independent part of the state):
//   g' = g * coef;  wd != 0: g' += wd * p;  momentum: buf = g' on the first applied step, else momentum * buf + (1 - dampening) * g';
//   g' = g' + momentum * buf (Nesterov) or buf;  p -= lr * g';  ema = d * ema + (1 - d) * p
// ROUNDING: every multiply-add below is an explicit fmaf and every other product is rounded on its own (a product that is an
// operand of fmaf cannot be contracted any further), so -ffp-contract=fast has nothing left to decide and all instantiations
// (plain / guarded, EMA or not, vector body / tail) give the same parameter and buffer bits:
//   g' = g * coef;  g' = fmaf(wd, p, g');  buf = fmaf(momentum, buf, (1 - dampening) * g');  g' = fmaf(momentum, buf, g');
//   p = fmaf(-lr, g', p);  ema = fmaf(d, ema, (1 - d) * p)
// GUARDED reads coef / skip / applied from the guard state and the learning rate from device memory (one uniform load per
// thread), so a captured launch follows a schedule without being captured again; the plain form takes them from the host.
// MOM = false passes no buffer and makes no load or store of one.
template <bool MOM, bool NEST>
__device__ __forceinline__ float sgd_elem(float p, float g, float& b, float coef, float wd, float mom, float omd, float lr, bool first) {
  float gg = g * coef;
  if (wd != 0.f) gg = fmaf(wd, p, gg);
  if (MOM) {
    b = first ? gg : fmaf(mom, b, omd * gg);
    gg = NEST ? fmaf(mom, b, gg) : b;
  }
  return fmaf(-lr, gg, p);
}

template <bool GUARDED, bool MOM, bool NEST, bool EMA>
__global__ void __launch_bounds__(256) sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  float* __restrict__ ema, long long n, float lr_host, const float* __restrict__ lr_dev,
                                                  float mom, float omd, float wd, float d, float coef_host, int first_host,
                                                  const GuardState* __restrict__ state) {
  if (GUARDED && state->skip) return;                    // uniform: the whole launch leaves every buffer untouched
  const float coef = GUARDED ? state->coef : coef_host, lr = GUARDED ? *lr_dev : lr_host;
  const bool first = GUARDED ? state->applied == 1 : first_host != 0;
  const float omd_e = 1.f - d;
  const long long nv = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 bv, ev;
    if (MOM) bv = reinterpret_cast<float4*>(buf)[i];
    if (EMA) ev = reinterpret_cast<float4*>(ema)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float b = MOM ? f4at(bv, k) : 0.f;
      const float pn = sgd_elem<MOM, NEST>(f4at(pv, k), f4at(gv, k), b, coef, wd, mom, omd, lr, first);
      f4at(pv, k) = pn;
      if (MOM) f4at(bv, k) = b;
      if (EMA) f4at(ev, k) = fmaf(d, f4at(ev, k), omd_e * pn);
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    if (MOM) reinterpret_cast<float4*>(buf)[i] = bv;
    if (EMA) reinterpret_cast<float4*>(ema)[i] = ev;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {        // tail
    const long long i = (nv << 2) + threadIdx.x;
    float b = MOM ? buf[i] : 0.f;
    const float pn = sgd_elem<MOM, NEST>(p[i], g[i], b, coef, wd, mom, omd, lr, first);
    p[i] = pn;
    if (MOM) buf[i] = b;
    if (EMA) ema[i] = fmaf(d, ema[i], omd_e * pn);
  }
}

// the checks both entry points share; LTU_OK with *launch = false for n <= 0
static int sgd_check(const float* p, const float* g, const float* buf, const float* ema, long long n, float momentum, float dampening,
                     float weight_decay, int nesterov, bool* launch) {
  *launch = false;
  if (!(momentum >= 0.f) || dampening != dampening || !(weight_decay >= 0.f)) return LTU_E_ARG;      // NaN included
  if (nesterov && (momentum <= 0.f || dampening != 0.f)) return LTU_E_ARG;                           // torch's rule
  if (n <= 0) return LTU_OK;
  if (p == nullptr || g == nullptr || (buf == nullptr) != (momentum == 0.f)) return LTU_E_ARG;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf | (uintptr_t)ema) & 15) return LTU_E_ARG;
  *launch = true;
  return LTU_OK;
}

template <bool GUARDED, bool EMA, typename... Args>
static void sgd_launch(bool mom, bool nest, long long n, hipStream_t s, Args... args) {
  const dim3 grid((unsigned)optim_blocks(n)), block(256);
  if (!mom)
    hipLaunchKernelGGL((sgd_kernel<GUARDED, false, false, EMA>), grid, block, 0, s, args...);
  else if (!nest)
    hipLaunchKernelGGL((sgd_kernel<GUARDED, true, false, EMA>), grid, block, 0, s, args...);
  else
    hipLaunchKernelGGL((sgd_kernel<GUARDED, true, true, EMA>), grid, block, 0, s, args...);
}

extern "C" int ltu_sgd(float* p, const float* g, float* buf, long long n, float lr, float momentum, float dampening, float weight_decay,
                       int nesterov, int first_step, float grad_scale, ltu_stream_t s) {
  if (!(lr >= 0.f) || grad_scale != grad_scale) return LTU_E_ARG;
  bool launch;
  const int rc = sgd_check(p, g, buf, nullptr, n, momentum, dampening, weight_decay, nesterov, &launch);
  if (!launch) return rc;
  sgd_launch<false, false>(momentum != 0.f, nesterov != 0, n, (hipStream_t)s, p, g, buf, (float*)nullptr, n, lr, (const float*)nullptr, momentum,
                           1.f - dampening, weight_decay, 0.f, grad_scale, first_step, (const GuardState*)nullptr);
  return ltu_check_launch();
}

extern "C" int ltu_sgd_guarded(float* p, const float* g, float* buf, float* ema, long long n, const float* lr_dev, float momentum,
                               float dampening, float weight_decay, int nesterov, float ema_decay, const void* state, ltu_stream_t s) {
  if (state == nullptr || ((uintptr_t)state & 15) || lr_dev == nullptr || ((uintptr_t)lr_dev & 3)) return LTU_E_ARG;
  if (ema != nullptr && !(ema_decay >= 0.f && ema_decay < 1.f)) return LTU_E_ARG;
  bool launch;
  const int rc = sgd_check(p, g, buf, ema, n, momentum, dampening, weight_decay, nesterov, &launch);
  if (!launch) return rc;
  const bool mom = momentum != 0.f, nest = nesterov != 0;
  if (ema != nullptr)
    sgd_launch<true, true>(mom, nest, n, (hipStream_t)s, p, g, buf, ema, n, 0.f, lr_dev, momentum, 1.f - dampening, weight_decay, ema_decay,
                           0.f, 0, (const GuardState*)state);
  else
    sgd_launch<true, false>(mom, nest, n, (hipStream_t)s, p, g, buf, ema, n, 0.f, lr_dev, momentum, 1.f - dampening, weight_decay, 0.f, 0.f,
                            0, (const GuardState*)state);
  return ltu_check_launch();
}
