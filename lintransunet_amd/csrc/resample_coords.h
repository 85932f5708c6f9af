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
