// The transposed product of a general block (Matrix::transpmult,
// spmv/Matrix.h:78-81; the reference declares it and throws, Matrix.cpp:145-148),
// gfx950.  For a column range [c0, c1) of the block:
//   out[j - c0] = fl(alpha * s_j + beta * out[j - c0])
// s_j starts at +0.0 and adds v * in[i] left to right over the entries (i, j, v)
// of column j in ascending (i, position in row i) order -- the row-order CSR sum
// of the transpose that a STABLE sort of the entries by column makes.  The map
// of that sort (t_ptr / t_row / t_pos) is built on the device by the helper the
// symmetric kernels share (spmv_tmap_build, spmv_sym.hip).  Three forms
// (plan_get "t_form"):
//   1 copy      the values permuted into column order (t_val) and an INNER
//               general plan on (t_ptr, t_row, t_val), created and baked like a
//               forward block: every forward form (lattice, LX / XW, diagonal,
//               sliced jagged, gather) runs A^T, all of them bit-identical to
//               the row-order CSR sum
//   2 in place  csr_tmap_kernel: one lane per output column over the map and
//               the caller's values (8 B per entry + 4 B per column of map, no
//               copy of the values)
//   3 self      a square block over [0, n) whose transpose is the block itself,
//               bit for bit: the forward plan runs it; only t_pos is kept (the
//               check runs again in plan_values_changed) and a block that is no
//               longer its own transpose takes the in-place kernel over
//               (rowptr, colind, t_pos) -- the transpose's pattern is the block's
#include "csr_plan.h"

#include <chrono>
#include <cstring>
#include <new>

struct SpmvTranspose {
  int32_t c0 = 0, c1 = 0;       // the column range
  const int32_t* rowptr0 = nullptr; // the arrays the map was built from
  const int32_t* colind0 = nullptr;
  const void* values0 = nullptr;    // ... and the values the copy was made from
  int elem = 0;                     // their size (4 or 8)
  int32_t* t_ptr = nullptr;         // c1 - c0 + 1 (null in the self form: rowptr)
  int32_t* t_row = nullptr;         // per entry, column order (self form: colind)
  int32_t* t_pos = nullptr;         // per entry: its position in `values`
  void* t_val = nullptr;            // copy form: values[t_pos[e]]
  spmv_hip_csr_plan* inner = nullptr; // copy form: the plan of the transpose
  int form = 2;
  int pattern_self = 0;  // t_ptr == rowptr and t_row == colind
  int in_place = 0;      // plan_set "t_in_place"
  int plan_us = 0;
};

namespace
{

// ---------------------------------------------------------------------------
// In-place kernel: csr_symt_kernel's second phase for a general block.  A
// workgroup owns 256 consecutive output columns; the entries of those columns
// are consecutive in the map, so t_row / t_pos stream coalesced, tile by tile:
// every lane gathers values[t_pos[e]] and in[t_row[e]] for one entry and parks
// the product in LDS, then each column's lane adds its products left to right.
// No atomics, every out written once by its own lane.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void csr_tmap_kernel(
    int32_t num_out, const int32_t* __restrict__ t_ptr,
    const int32_t* __restrict__ t_row, const int32_t* __restrict__ t_pos,
    const T* __restrict__ values, T alpha, const T* __restrict__ in, T beta,
    T* __restrict__ out, int num_col_blocks)
{
  constexpr int TILE = 4 * kBlock;
  __shared__ T s_prod[TILE];
  __shared__ int32_t s_ptr[kRows + 1];
  const int t = threadIdx.x;
  for (int cb = blockIdx.x; cb < num_col_blocks; cb += gridDim.x) {
    const int32_t j0 = cb * kRows;
    const int nc = min(kRows, num_out - j0);
    __syncthreads(); // previous column block done with s_ptr / s_prod
    if (t <= nc)
      s_ptr[t] = t_ptr[j0 + t];
    if (t == 0 && nc == kRows)
      s_ptr[kRows] = t_ptr[j0 + kRows];
    __syncthreads();
    const int32_t a = s_ptr[0], b = s_ptr[nc];
    int32_t lo = 0, hi = 0;
    if (t < nc) {
      lo = s_ptr[t];
      hi = s_ptr[t + 1];
    }
    T acc = T(0);
    for (int64_t base = a; base < b; base += TILE) {
      if (base != a)
        __syncthreads(); // column owners finished reading the previous tile
#pragma unroll
      for (int c = 0; c < TILE / kBlock; ++c) {
        const int64_t e = base + c * kBlock + t;
        T p = T(0);
        if (e < b)
          p = values[t_pos[e]] * in[t_row[e]];
        s_prod[c * kBlock + t] = p;
      }
      __syncthreads();
      const int32_t elo = (int32_t)(max((int64_t)lo, base) - base);
      const int32_t ehi = (int32_t)(min((int64_t)hi, base + TILE) - base);
      for (int32_t e = elo; e < ehi; ++e)
        acc += s_prod[e];
    }
    if (t < nc) {
      const T c = alpha * acc;
      T y = c;
      if (beta != T(0))
        y = c + beta * out[j0 + t];
      out[j0 + t] = y;
    }
  }
}

// a block without entries: every column is empty (alpha * 0.0)
template <typename T>
__global__ __launch_bounds__(kBlock) void tmap_empty_kernel(int64_t n, T alpha,
                                                            T beta,
                                                            T* __restrict__ out)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const T c = alpha * T(0);
    out[i] = beta != T(0) ? c + beta * out[i] : c;
  }
}

// the copy form's values: t_val[e] = values[t_pos[e]]
template <typename T>
__global__ __launch_bounds__(kBlock) void tmap_permute_kernel(
    int64_t nnz, const int32_t* __restrict__ t_pos, const T* __restrict__ values,
    T* __restrict__ t_val)
{
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz;
       e += (int64_t)gridDim.x * blockDim.x)
    t_val[e] = values[t_pos[e]];
}

// is the transpose the block itself?  `differs` = 1 where the pattern (PAT)
// or a value's bits differ.  (Every lane that finds a difference stores the
// same 1: no read-modify-write.)
template <typename U, bool PAT>
__global__ __launch_bounds__(kBlock) void tmap_self_check_kernel(
    int32_t n, int64_t nnz, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ colind, const U* __restrict__ values,
    const int32_t* __restrict__ t_ptr, const int32_t* __restrict__ t_row,
    const int32_t* __restrict__ t_pos, int32_t* __restrict__ differs)
{
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  bool d = false;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz;
       e += stride) {
    if constexpr (PAT)
      d |= t_row[e] != colind[e];
    d |= values[t_pos[e]] != values[e];
  }
  if constexpr (PAT)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n;
         i += stride)
      d |= t_ptr[i] != rowptr[i];
  if (d)
    *differs = 1;
}

// 1 = the transpose equals the block (values compared by their bits)
int self_check(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* pl,
               const SpmvTranspose* tr, bool pattern, int* is_self,
               hipStream_t st)
{
  *is_self = 0;
  int32_t* flag = nullptr;
  SPMV_CHECK_HIP(hipMalloc(&flag, sizeof(int32_t)));
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(int32_t), st);
  int32_t differs = 1;
  if (e == hipSuccess) {
    const int64_t work = pl->nnz > pl->num_rows ? pl->nnz : (int64_t)pl->num_rows + 1;
    const int grid = spmv_grid_for(ctx, work, kBlock);
#define SPMV_SELF(U, P)                                                        \
  hipLaunchKernelGGL((tmap_self_check_kernel<U, P>), dim3(grid), dim3(kBlock), \
                     0, st, pl->num_rows, pl->nnz, tr->rowptr0, tr->colind0,   \
                     static_cast<const U*>(tr->values0), tr->t_ptr,            \
                     tr->t_row, tr->t_pos, flag)
    if (tr->elem == 8) {
      if (pattern)
        SPMV_SELF(uint64_t, true);
      else
        SPMV_SELF(uint64_t, false);
    } else {
      if (pattern)
        SPMV_SELF(uint32_t, true);
      else
        SPMV_SELF(uint32_t, false);
    }
#undef SPMV_SELF
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync(&differs, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess)
    e = hipStreamSynchronize(st);
  (void)hipFree(flag);
  SPMV_CHECK_HIP(e);
  *is_self = differs == 0;
  return SPMV_HIP_OK;
}

int permute_values(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* pl,
                   SpmvTranspose* tr, hipStream_t st)
{
  const int grid = spmv_grid_for(ctx, pl->nnz, kBlock);
  if (tr->elem == 8)
    hipLaunchKernelGGL((tmap_permute_kernel<double>), dim3(grid), dim3(kBlock), 0,
                       st, pl->nnz, tr->t_pos,
                       static_cast<const double*>(tr->values0),
                       static_cast<double*>(tr->t_val));
  else
    hipLaunchKernelGGL((tmap_permute_kernel<float>), dim3(grid), dim3(kBlock), 0,
                       st, pl->nnz, tr->t_pos,
                       static_cast<const float*>(tr->values0),
                       static_cast<float*>(tr->t_val));
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

void drop_copy(SpmvTranspose* tr)
{
  if (tr->inner)
    spmv_hip_csr_plan_destroy(tr->inner);
  tr->inner = nullptr;
  (void)hipFree(tr->t_val);
  tr->t_val = nullptr;
}

// the copy form: t_val and the inner plan, created and baked like a forward
// block (CSRSpMV::init + bake_values).  Out of memory: nothing kept, the
// caller runs the in-place kernel.
int build_copy(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* pl, SpmvTranspose* tr,
               hipStream_t st)
{
  const int32_t m = tr->c1 - tr->c0;
  hipError_t e = hipMalloc(&tr->t_val, (size_t)tr->elem * (size_t)pl->nnz);
  if (e != hipSuccess) {
    tr->t_val = nullptr;
    return static_cast<int>(e);
  }
  int rc = permute_values(ctx, pl, tr, st);
  if (rc == SPMV_HIP_OK)
    rc = static_cast<int>(hipStreamSynchronize(st));
  // ROWBLOCK, never AUTO: the row-list kernel would give empty columns +0.0
  // (it zero-fills) and the vector kernel sums a row out of order
  if (rc == SPMV_HIP_OK)
    rc = spmv_hip_csr_plan_create(ctx, m, pl->num_rows, pl->nnz, tr->t_ptr,
                                  tr->t_row, 0, SPMV_HIP_ALGO_ROWBLOCK, &tr->inner);
  if (rc == SPMV_HIP_OK) {
    rc = tr->elem == 8
             ? spmv_hip_csr_plan_bake_values_f64(
                   ctx, tr->inner, static_cast<const double*>(tr->t_val), nullptr, st)
             : spmv_hip_csr_plan_bake_values_f32(
                   ctx, tr->inner, static_cast<const float*>(tr->t_val), nullptr, st);
    if (rc == SPMV_HIP_ENOTSUP) // no value-baking form: the CSR-order kernels
      rc = SPMV_HIP_OK;
  }
  if (rc != SPMV_HIP_OK)
    drop_copy(tr);
  return rc;
}

bool out_of_memory(int rc)
{
  return rc == SPMV_HIP_ENOMEM || rc == static_cast<int>(hipErrorOutOfMemory);
}

template <typename T>
int run_transpose(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* plan,
                  int32_t num_rows, int32_t num_cols, int64_t nnz,
                  const int32_t* rowptr, const int32_t* colind, const T* values,
                  T alpha, const T* in, T beta, T* out, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(plan && plan->ctx == ctx && !plan->symmetric && plan->tr);
  SPMV_REQUIRE(num_rows == plan->num_rows && num_cols == plan->num_cols
               && nnz == plan->nnz);
  const SpmvTranspose* tr = plan->tr;
  // the map holds the content of the arrays it was built from
  SPMV_REQUIRE(rowptr == tr->rowptr0 && colind == tr->colind0);
  const int32_t m = tr->c1 - tr->c0;
  if (m == 0)
    return SPMV_HIP_OK;
  SPMV_REQUIRE(out && (nnz == 0 || (in && values)));
  hipStream_t st = spmv_stream(ctx, stream);
  if (nnz == 0) {
    const int grid = spmv_grid_for(ctx, m, kBlock);
    hipLaunchKernelGGL((tmap_empty_kernel<T>), dim3(grid), dim3(kBlock), 0, st,
                       (int64_t)m, alpha, beta, out);
    SPMV_CHECK_LAUNCH();
    return SPMV_HIP_OK;
  }
  const bool baked = values == tr->values0 && tr->elem == (int)sizeof(T);
  if (baked && !tr->in_place && tr->form == 3) { // the block is its own transpose
    if constexpr (sizeof(T) == 8)
      return spmv_hip_csr_spmv_f64(ctx, plan, num_rows, num_cols, nnz, rowptr,
                                   colind, values, nullptr, alpha, in, beta, out,
                                   nullptr, stream);
    else
      return spmv_hip_csr_spmv_f32(ctx, plan, num_rows, num_cols, nnz, rowptr,
                                   colind, values, nullptr, alpha, in, beta, out,
                                   stream);
  }
  if (baked && !tr->in_place && tr->form == 1 && tr->inner) {
    if constexpr (sizeof(T) == 8)
      return spmv_hip_csr_spmv_f64(ctx, tr->inner, m, num_rows, nnz, tr->t_ptr,
                                   tr->t_row, static_cast<const double*>(tr->t_val),
                                   nullptr, alpha, in, beta, out, nullptr, stream);
    else
      return spmv_hip_csr_spmv_f32(ctx, tr->inner, m, num_rows, nnz, tr->t_ptr,
                                   tr->t_row, static_cast<const float*>(tr->t_val),
                                   nullptr, alpha, in, beta, out, stream);
  }
  // in place: reads the caller's values (given up with plan_release_matrix)
  SPMV_REQUIRE(!(plan->released & 2) && tr->t_pos);
  const int32_t* t_ptr = tr->t_ptr ? tr->t_ptr : rowptr;
  const int32_t* t_row = tr->t_row ? tr->t_row : colind;
  const int ncb = (m + kRows - 1) / kRows;
  int grid = ctx->num_cus * kBlocksPerCU;
  if (grid > ncb)
    grid = ncb;
  hipLaunchKernelGGL((csr_tmap_kernel<T>), dim3(grid), dim3(kBlock), 0, st, m,
                     t_ptr, t_row, tr->t_pos, values, alpha, in, beta, out, ncb);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // namespace

// --- plan API hooks (spmv_csr_plan.hip) ---------------------------------------
void spmv_tr_free(spmv_hip_csr_plan* pl)
{
  SpmvTranspose* tr = pl->tr;
  if (!tr)
    return;
  (void)hipSetDevice(pl->ctx->device);
  drop_copy(tr);
  (void)hipFree(tr->t_ptr);
  (void)hipFree(tr->t_row);
  (void)hipFree(tr->t_pos);
  delete tr;
  pl->tr = nullptr;
}

// plan_values_changed: the copy refreshed, the self-transpose check again
// (nothing is allocated: a block that is no longer its own transpose takes the
// in-place kernel, whose map it has)
int spmv_tr_values_changed(spmv_hip_ctx* ctx, spmv_hip_csr_plan* pl, hipStream_t st)
{
  SpmvTranspose* tr = pl->tr;
  if (!tr || pl->nnz == 0 || tr->c1 == tr->c0)
    return SPMV_HIP_OK;
  if (tr->pattern_self) {
    int is_self = 0;
    const int rs = self_check(ctx, pl, tr, false, &is_self, st);
    if (rs != SPMV_HIP_OK)
      return rs;
    if (is_self && tr->form != 3 && pl->algo == SPMV_HIP_ALGO_ROWBLOCK) {
      drop_copy(tr); // (not needed any more)
      tr->form = 3;
    } else if (!is_self && tr->form == 3) {
      tr->form = 2;
    }
  }
  if (tr->form == 1 && tr->inner) {
    int rc = permute_values(ctx, pl, tr, st);
    if (rc == SPMV_HIP_OK)
      rc = spmv_hip_csr_plan_values_changed(ctx, tr->inner, st);
    return rc;
  }
  return SPMV_HIP_OK;
}

// plan_get keys of the transpose (EINVAL: not one of them)
int spmv_tr_get(const spmv_hip_csr_plan* pl, const char* key, int* value)
{
  const SpmvTranspose* tr = pl->tr;
  if (!strncmp(key, "t.", 2)) { // the inner plan's decisions
    if (!tr || !tr->inner) {
      *value = 0;
      return SPMV_HIP_OK;
    }
    return spmv_hip_csr_plan_get(tr->inner, key + 2, value);
  }
  if (!strcmp(key, "t_form")) {
    *value = !tr ? 0 : tr->in_place ? 2 : tr->form;
  } else if (!strcmp(key, "t_plan_us")) {
    *value = tr ? tr->plan_us : 0;
  } else if (!strcmp(key, "t_kib")) {
    int64_t b = 0;
    if (tr) {
      if (tr->t_ptr)
        b += 4 * ((int64_t)(tr->c1 - tr->c0) + 1);
      if (tr->t_row)
        b += 4 * pl->nnz;
      if (tr->t_pos)
        b += 4 * pl->nnz;
      if (tr->t_val)
        b += (int64_t)tr->elem * pl->nnz;
      int inner_kib = 0;
      if (tr->inner)
        (void)spmv_hip_csr_plan_get(tr->inner, "plan_kib", &inner_kib);
      b += (int64_t)inner_kib * 1024;
    }
    *value = (int)((b + 1023) / 1024);
  } else {
    return SPMV_HIP_EINVAL;
  }
  return SPMV_HIP_OK;
}

int spmv_tr_set(spmv_hip_csr_plan* pl, const char* key, int value)
{
  SpmvTranspose* tr = pl->tr;
  if (!strncmp(key, "t.", 2)) { // a knob of the inner plan
    SPMV_REQUIRE(tr && tr->inner);
    return spmv_hip_csr_plan_set(tr->inner, key + 2, value);
  }
  if (!strcmp(key, "t_in_place")) {
    SPMV_REQUIRE(tr && (value == 0 || value == 1));
    SPMV_REQUIRE(value == 0 || !(pl->released & 2)); // (it reads the values)
    tr->in_place = value;
    return SPMV_HIP_OK;
  }
  return SPMV_HIP_EINVAL;
}

extern "C" {

int spmv_hip_csr_plan_build_transpose(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan,
                                      const int32_t* rowptr, const int32_t* colind,
                                      const void* values, int value_bytes,
                                      int32_t col_begin, int32_t col_end,
                                      void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(plan && plan->ctx == ctx && !plan->symmetric);
  SPMV_REQUIRE(!plan->released); // (colind / values were given up)
  SPMV_REQUIRE(value_bytes == 4 || value_bytes == 8);
  SPMV_REQUIRE(col_begin >= 0 && col_begin <= col_end && col_end <= plan->num_cols);
  SPMV_REQUIRE(plan->nnz == 0 || (rowptr && colind && values));
  SPMV_REQUIRE(!plan->structure_baked()
               || (rowptr == plan->rowptr0 && colind == plan->colind0));
  hipStream_t st = spmv_stream(ctx, stream);
  SPMV_CHECK_HIP(hipStreamSynchronize(st)); // (the caller's kernels: not plan time)
  const auto t_begin = std::chrono::steady_clock::now();
  spmv_tr_free(plan);
  SpmvTranspose* tr = new (std::nothrow) SpmvTranspose;
  if (!tr)
    return SPMV_HIP_ENOMEM;
  tr->c0 = col_begin;
  tr->c1 = col_end;
  tr->rowptr0 = rowptr;
  tr->colind0 = colind;
  tr->values0 = values;
  tr->elem = value_bytes;
  plan->tr = tr;
  int rc = SPMV_HIP_OK;
  if (plan->nnz > 0) {
    int refused = 0;
    rc = spmv_tmap_build(ctx, plan->num_rows, plan->nnz, rowptr, colind, col_begin,
                         col_end, false, &tr->t_ptr, &tr->t_pos, &tr->t_row,
                         &refused, st);
    if (rc == SPMV_HIP_OK && refused)
      rc = SPMV_HIP_EINVAL; // an entry outside [col_begin, col_end)
    // the self form needs the forward plan's row-block kernels: they sum in
    // CSR order (the vector kernel does not, the row-list kernel zero-fills)
    const bool square = plan->num_rows == plan->num_cols && col_begin == 0
                        && col_end == plan->num_cols;
    if (rc == SPMV_HIP_OK && square) {
      int same = 0;
      rc = self_check(ctx, plan, tr, true, &same, st);
      if (rc == SPMV_HIP_OK && same) {
        tr->pattern_self = 1;
        if (plan->algo == SPMV_HIP_ALGO_ROWBLOCK)
          tr->form = 3;
      }
    }
    if (rc == SPMV_HIP_OK && tr->form != 3 && !ctx->csr_in_place) {
      const int rb = build_copy(ctx, plan, tr, st);
      if (rb == SPMV_HIP_OK)
        tr->form = 1;
      else if (!out_of_memory(rb))
        rc = rb;
      // (no memory for the copy: the in-place kernel)
    }
    if (rc == SPMV_HIP_OK && tr->pattern_self && tr->form != 1) {
      // the transpose's pattern is the block's: rowptr / colind serve as the
      // map, only the positions stay
      (void)hipFree(tr->t_ptr);
      (void)hipFree(tr->t_row);
      tr->t_ptr = tr->t_row = nullptr;
    }
  }
  if (rc != SPMV_HIP_OK) {
    spmv_tr_free(plan);
    return rc;
  }
  tr->plan_us = (int)std::chrono::duration_cast<std::chrono::microseconds>(
                    std::chrono::steady_clock::now() - t_begin)
                    .count();
  return SPMV_HIP_OK;
}

int spmv_hip_csr_spmvt_f64(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* plan,
                           int32_t num_rows, int32_t num_cols,
                           int64_t num_non_zeros, const int32_t* rowptr,
                           const int32_t* colind, const double* values,
                           double alpha, const double* in, double beta,
                           double* out, void* stream)
{
  return run_transpose<double>(ctx, plan, num_rows, num_cols, num_non_zeros,
                               rowptr, colind, values, alpha, in, beta, out,
                               stream);
}

int spmv_hip_csr_spmvt_f32(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* plan,
                           int32_t num_rows, int32_t num_cols,
                           int64_t num_non_zeros, const int32_t* rowptr,
                           const int32_t* colind, const float* values,
                           float alpha, const float* in, float beta, float* out,
                           void* stream)
{
  return run_transpose<float>(ctx, plan, num_rows, num_cols, num_non_zeros,
                              rowptr, colind, values, alpha, in, beta, out,
                              stream);
}

} // extern "C"
