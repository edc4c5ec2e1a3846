// The device plan of the multicolour sweeps (spmv_mcgs.hip), shared with the
// ILU(0) factorisation (spmv_ilu0.hip), which writes the values and dinv of a
// plan it owns.
#pragma once

#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "spmv_hip.h"

// The off-diagonal values of a part live in ONE of two forms, by the plan's
// value_bits: 64 -- val / long_val (val32 / long_val32 are NULL); 32 -- val32 /
// long_val32, the fp64 values rounded to nearest-even (val / long_val are NULL).
struct McgsPartDev {
  int32_t* slice_pos0 = nullptr;
  int64_t* slice_ptr = nullptr;
  int32_t* len = nullptr;
  int32_t* col = nullptr;
  double* val = nullptr;
  float* val32 = nullptr;
  int32_t* long_pos = nullptr;
  int64_t* long_ptr = nullptr;
  int32_t* long_col = nullptr;
  double* long_val = nullptr;
  float* long_val32 = nullptr;
  std::vector<int32_t> color_slice, color_long; // host: num_colors + 1 each
};

struct spmv_hip_mcgs_plan {
  spmv_hip_ctx* ctx = nullptr;
  int32_t n = 0;
  int32_t num_colors = 0;
  int32_t* perm = nullptr;
  double* dinv = nullptr;
  std::vector<int32_t> color_start; // host
  McgsPartDev before, after;
  int value_bits = 64;
  int64_t bytes = 0;
};

// An fp64 plan of either builder becomes an fp32 plan (spmv_mcgs.hip): per
// value array a float array is allocated, a kernel rounds into it and the fp64
// array is freed, one array after the other; plan->bytes follows.  Waits for
// the stream.  *out_of_range: the values fp32_range.h's rule refuses (the
// caller decides what they mean).  On a failure the plan is the caller's to
// destroy, in whichever state it is: every array is in one form or the other.
int mcgs_plan_narrow(spmv_hip_mcgs_plan* plan, hipStream_t stream,
                     int64_t* out_of_range);
