// Host launchers of the 5 .. 8-class head kernels (manyclass.hip).  ltu_head_softmax_* / ltu_final_softmax_* (pointwise.hip)
// hand C > 4 over to these; C <= 4 never reaches them.
#pragma once
#include "common.h"

#define LTU_WIDE_MAXC 8

int ltu_head_softmax_wide_fwd(const void* z, float* p, long long M, int C, int CP, int dtype, ltu_stream_t s);
int ltu_head_softmax_wide_bwd(const float* dp, const float* p, void* dz, long long M, int C, int CP, int dtype, ltu_stream_t s);
int ltu_final_softmax_wide_fwd(const void* z, float* p, int B, int h, int w, int D, int C, int CP, int dtype, ltu_stream_t s);
int ltu_final_softmax_wide_bwd(const float* dp, const float* p, void* dz, int B, int h, int w, int D, int C, int CP, int dtype,
                               ltu_stream_t s);
