// The device plan of the multicolour ILU(0) (spmv_ilu0.hip), shared with the
// builder that makes one from the CSR arrays on the device
// (spmv_mcgs_build.hip: spmv_hip_ilu0_plan_build).
#pragma once

#include <cstdint>

#include "mcgs_plan.h"

struct Ilu0PartDev {
  int64_t* ptr = nullptr;  // n + 1, by position
  int32_t* cpos = nullptr; // position of the column
  int32_t* src = nullptr;  // index into the matrix's values
  int64_t* slot = nullptr; // >= 0: sliced val; < 0: long_val[~slot]
  double* w = nullptr;     // the working values = the factor, part-CSR order
  int64_t count = 0;
};

struct spmv_hip_ilu0_plan {
  spmv_hip_ctx* ctx = nullptr;
  spmv_hip_mcgs_plan* inner = nullptr;
  int32_t n = 0;
  int64_t num_values = 0;
  Ilu0PartDev before, after;
  double* wd = nullptr;       // n: d~ by position
  double* wdinv = nullptr;    // n: 1.0 / d~ by position
  // {pivots not finite or zero, pivots negative, values out of fp32's range
  // (an inner plan that keeps floats)}, 16 bytes
  unsigned* counts = nullptr;
  int64_t bytes = 0;          // without the inner plan's
};
