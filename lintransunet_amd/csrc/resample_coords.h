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
