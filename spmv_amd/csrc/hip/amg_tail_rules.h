// The host side of the fused AMG tail (spmv_amg.hip: amg_tail_kernel;
// host/amg.cpp: AmgPreconditioner::set_tail_rows), plain C++ with no device
// call so that it can be built and run alone under the sanitizers
// (tools/amg_tail_check.cpp):
//   amg_tail_first_level    which suffix of the hierarchy is the tail
//   amg_tail_fill_table     the descriptor builder of spmv_hip_amg_tail_create:
//                           every rule of a level that needs no device memory,
//                           and the table entry the kernel reads
//   amg_tail_csr_is_sound   every index the kernel's products will use (on the
//                           copies tail_create reads back)
//   amg_tail_lanes_is_sound the row order of a level
#pragma once

#include <cstdint>

#include "spmv_hip.h"

// threads of the one workgroup; the kernel's row loops step by it in int32
constexpr int kAmgTailBlock = 1024;
constexpr int32_t kAmgTailMaxRows = INT32_MAX - kAmgTailBlock;

// One level of the tail as the kernel reads it (the device table of
// spmv_hip_amg_tail): coarse_rows / agg / member_ptr / member describe the step
// to the next entry (0 / NULL on the last one); a, b are the level's Chebyshev
// coefficients, the smoother's below the last entry and the coarsest level's
// on it (entries past the degree are 0.0 and never read).
struct AmgTailDev {
  int32_t rows, lanes, coarse_rows, pad;
  const int32_t* rowptr;
  const int32_t* colind;
  const double* values;
  const double* dinv;
  double* r;
  double* w;
  double* dd;
  double* z;
  const int32_t* agg;
  const int32_t* member_ptr;
  const int32_t* member;
  double a[SPMV_HIP_AMG_TAIL_MAX_DEGREE], b[SPMV_HIP_AMG_TAIL_MAX_DEGREE];
};

// What the builder needs of a level's coarsening step (spmv_hip_amg_plan is
// opaque here): present = the level names one that belongs to the context.
struct AmgTailStep {
  bool present;
  int32_t fine_rows, coarse_rows;
  const int32_t* agg;
  const int32_t* member_ptr;
  const int32_t* member;
};

// The tail is the longest suffix t .. nl-1 of the levels with t >= 1 in which
// every level has rows[l] <= max_rows; -> t, or nl when there is none (max_rows
// <= 0, one level, or a last level that is too large).  Level 0 is never in it.
inline int amg_tail_first_level(const int64_t* rows, int nl, int64_t max_rows)
{
  if (!rows || nl < 2 || max_rows <= 0)
    return nl < 0 ? 0 : nl;
  int t = nl;
  while (t > 1 && rows[t - 1] <= max_rows)
    --t;
  return t;
}

// rowptr monotone from 0 to nnz, every column in [0, ncols)
inline bool amg_tail_csr_is_sound(int64_t rows, int64_t ncols, int64_t nnz,
                                  const int32_t* rowptr, const int32_t* colind)
{
  if (rows < 1 || ncols < 1 || nnz < 0 || !rowptr || (nnz > 0 && !colind))
    return false;
  if (rowptr[0] != 0 || rowptr[rows] != nnz)
    return false;
  for (int64_t i = 0; i < rows; ++i)
    if (rowptr[i + 1] < rowptr[i] || rowptr[i + 1] > nnz)
      return false;
  for (int64_t e = 0; e < nnz; ++e)
    if (colind[e] < 0 || colind[e] >= ncols)
      return false;
  return true;
}

// 0 = one lane per row, left to right; else the lanes of the sub-wavefront
// order: a power of two in 4 .. 64
inline bool amg_tail_lanes_is_sound(int lanes)
{
  return lanes == 0
         || (lanes >= 4 && lanes <= 64 && (lanes & (lanes - 1)) == 0);
}

inline bool amg_tail_is_aligned(const void* p, uintptr_t bytes)
{
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}

// The descriptor builder.  Checks the sizes and degrees of `in` and, per level,
// everything that can be checked without reading device memory -- rows in 1 ..
// kAmgTailMaxRows, an entry count that fits int32, every array present, index
// arrays 4-byte and double arrays 8-byte aligned, the lane count, a step on
// every level but the last whose fine_rows / coarse_rows are this level's and
// the next level's rows -- and fills out[0 .. num_levels) with the entries the
// kernel reads; of a and b exactly `degree` entries are read (smooth_degree
// below the last level, coarse_degree on it).  steps: one per level.  false:
// a rule does not hold; out is then not to be used.
inline bool amg_tail_fill_table(const spmv_hip_amg_tail_host& in,
                                const AmgTailStep* steps, AmgTailDev* out)
{
  const int nlev = in.num_levels;
  if (nlev < 1 || nlev > SPMV_HIP_AMG_TAIL_MAX_LEVELS || !in.levels || !steps
      || !out)
    return false;
  if (in.smooth_degree < 1 || in.smooth_degree > SPMV_HIP_AMG_TAIL_MAX_DEGREE
      || in.coarse_degree < 1
      || in.coarse_degree > SPMV_HIP_AMG_TAIL_MAX_DEGREE)
    return false;
  for (int l = 0; l < nlev; ++l) {
    const spmv_hip_amg_tail_level& h = in.levels[l];
    const AmgTailStep& st = steps[l];
    const bool last = l == nlev - 1;
    const int degree = last ? in.coarse_degree : in.smooth_degree;
    if (h.rows < 1 || h.rows > kAmgTailMaxRows || h.nnz < 0
        || h.nnz > INT32_MAX)
      return false;
    if (!h.rowptr || (h.nnz > 0 && (!h.colind || !h.values)) || !h.dinv || !h.r
        || !h.w || !h.dd || !h.z || !h.a || !h.b)
      return false;
    if (!amg_tail_is_aligned(h.rowptr, 4) || !amg_tail_is_aligned(h.colind, 4))
      return false;
    for (const void* v : {(const void*)h.values, (const void*)h.dinv,
                          (const void*)h.r, (const void*)h.w,
                          (const void*)h.dd, (const void*)h.z})
      if (!amg_tail_is_aligned(v, 8))
        return false;
    if (!amg_tail_lanes_is_sound(h.lanes_per_row))
      return false;
    if (last) {
      if (h.step != nullptr || st.present)
        return false;
    } else {
      if (h.step == nullptr || !st.present || st.fine_rows != h.rows
          || st.coarse_rows < 1 || st.coarse_rows != in.levels[l + 1].rows
          || !st.agg || !st.member_ptr || !st.member)
        return false;
    }
    AmgTailDev& d = out[l];
    d = AmgTailDev();
    d.rows = h.rows;
    d.lanes = h.lanes_per_row;
    d.rowptr = h.rowptr;
    d.colind = h.colind;
    d.values = h.values;
    d.dinv = h.dinv;
    d.r = h.r;
    d.w = h.w;
    d.dd = h.dd;
    d.z = h.z;
    if (!last) {
      d.coarse_rows = st.coarse_rows;
      d.agg = st.agg;
      d.member_ptr = st.member_ptr;
      d.member = st.member;
    }
    for (int j = 0; j < degree; ++j) {
      d.a[j] = h.a[j];
      d.b[j] = h.b[j];
    }
  }
  return true;
}

// One level's coefficients rewritten in a table entry (tail_set_coefficients)
inline void amg_tail_set_entry_coefficients(AmgTailDev& d, int degree,
                                            const double* a, const double* b)
{
  for (int j = 0; j < degree; ++j) {
    d.a[j] = a[j];
    d.b[j] = b[j];
  }
}
