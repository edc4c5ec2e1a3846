// The device plan of the multicolour sweeps (spmv_mcgs.hip), shared with the
// ILU(0) factorisation (spmv_ilu0.hip), which writes the values and dinv of a
// plan it owns.
#pragma once

#include <cstdint>
#include <vector>

#include "spmv_hip.h"

struct McgsPartDev {
  int32_t* slice_pos0 = nullptr;
  int64_t* slice_ptr = nullptr;
  int32_t* len = nullptr;
  int32_t* col = nullptr;
  double* val = nullptr;
  int32_t* long_pos = nullptr;
  int64_t* long_ptr = nullptr;
  int32_t* long_col = nullptr;
  double* long_val = nullptr;
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
  int64_t bytes = 0;
};
