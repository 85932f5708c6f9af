// Source coordinates of the pull resamplers (resample.hip: trilinear and arg-max; spline.hip: cubic B-spline), shared so that every
// kernel that pulls through the same float64 matrix lands on the same clamped coordinate.
#pragma once
#include <hip/hip_runtime.h>

// border padding: the coordinate is clamped to [0, S - 1] per source axis (grid_sample padding_mode 'border', in voxel units)
__device__ __forceinline__ void clamp_coords(const int* S, double c0, double c1, double c2, double* c) {
  c[0] = fmin(fmax(c0, 0.0), (double)(S[0] - 1));
  c[1] = fmin(fmax(c1, 0.0), (double)(S[1] - 1));
  c[2] = fmin(fmax(c2, 0.0), (double)(S[2] - 1));
}

// ---- the label vote ("one-hot, order 1"), shared by resample.hip's ltu_resample_vote and augment.hip's ltu_sample_vote ---------------
// The 8 trilinear taps of a voxel hold at most 8 distinct labels, so interpolating every class's indicator map and taking the arg-max
// needs no one-hot volume: the score of a value v is s_v = sum of w[q] over the taps with l[q] == v, added in tap order q = 0 .. 7
// with plain fp32 adds, and the smallest v of maximal score wins (torch.argmax's first maximum, ltu_resample_argmax's rule).  The
// score of tap r's label is formed as sum_q (l[q] == l[r] ? w[q] : 0): the weights are >= +0, so an added 0 changes no bit.  64
// selects and adds in registers, no LDS.  The caller makes every w[q] opaque first (the product that forms it must be rounded before
// it is added: -ffp-contract=fast would otherwise fuse it into the sum where the select folds away, q == r).  8 equal taps need no
// scores (theirs is the only one): where that holds in every lane of a wave - the inside of a structure, the background - the wave
// skips the vote.
__device__ __forceinline__ uint8_t label_vote8(const int (&l)[8], const float (&w)[8]) {
  bool same = true;
#pragma unroll
  for (int q = 1; q < 8; ++q) same = same && l[q] == l[0];
  if (same) return (uint8_t)l[0];
  float best = -1.f;                 // below every score: tap 0 always takes it
  int lab = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) s += l[q] == l[r] ? w[q] : 0.f;
    const bool take = s > best || (s == best && l[r] < lab);
    best = take ? s : best;
    lab = take ? l[r] : lab;
  }
  return (uint8_t)lab;
}

// ---- cubic B-spline taps, shared by spline.hip's resampler and augment.hip's patch gather ----------------------------------------
// whole-sample mirror of a tap index in -1 .. n + 1 (all that occurs once the coordinate lies in [0, n - 1])
__device__ __forceinline__ int sp_mirror(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i = i < 0 ? -i : i;
  i = i >= p ? i - p : i;
  return i > n - 1 ? p - i : i;
}

// the weights of the taps f-1 .. f+2 at the fraction t: ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6
__device__ __forceinline__ void sp_cubic_weights(float t, float* w) {
  const float u = 1.f - t, t2 = t * t;
  w[0] = u * u * u * (1.f / 6.f);
  w[1] = fmaf(t2, fmaf(0.5f, t, -1.f), 2.f / 3.f);
  w[2] = fmaf(t, fmaf(t, fmaf(-0.5f, t, 0.5f), 0.5f), 1.f / 6.f);
  w[3] = t2 * t * (1.f / 6.f);
}
