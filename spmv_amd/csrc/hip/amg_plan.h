// One coarsening step of spmv::AmgPreconditioner on the device: what
// spmv_amg.hip (which builds and owns it) and spmv_amg_block.hip (which reads
// agg and the member lists) share.  spmv_hip_amg_plan_create checked every
// index in it against the sizes it records.
#pragma once

#include <cstdint>

struct spmv_hip_ctx;

struct spmv_hip_amg_plan {
  spmv_hip_ctx* ctx = nullptr;
  int32_t fine_rows = 0, coarse_rows = 0, num_diagonal = 0;
  int64_t num_values = 0, coarse_nnz = 0, src_count = 0, xrow_count = 0;
  int32_t* agg = nullptr;        // fine_rows
  int32_t* member_ptr = nullptr; // coarse_rows + 1
  int32_t* member = nullptr;     // fine_rows
  int64_t* src_ptr = nullptr;    // coarse_nnz + 1
  int32_t* src = nullptr;        // src_count
  int64_t* xrow_ptr = nullptr;   // fine_rows + 1 (symmetric storage only)
  int32_t* xrow_src = nullptr;   // xrow_count
  int64_t bytes = 0;
};
