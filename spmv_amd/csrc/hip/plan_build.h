// What the device-side setup builders (spmv_mcgs_build.hip: the colouring and
// the sweep / ILU(0) plans; spmv_amg_build.hip: the aggregates and the Galerkin
// plan) share: the priority hash of the rounds, the check of a block's CSR
// arrays where they lie, temporaries on the books (Temp / CubTemp / TempBytes),
// scans, the transposed map kept for a call, and the plans' own arrays.
// Everything is internal to the including translation unit.
#pragma once

#include "common.h"

#include <hipcub/hipcub.hpp>

#include "csr_plan.h"
#include "plan_scratch.h"

namespace
{

constexpr int kNatural = 1; // SPMV_HIP_MCGS_NATURAL
constexpr int kBatch = 8;   // rounds per read of the counters

// poisson.hip's splitmix64 finaliser
__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t row_hash(int32_t i)
{
  return mix64((uint64_t)((int64_t)i + 1) * 0x9E3779B97F4A7C15ull);
}

// Everything a later kernel indexes with, checked where it lies.  bit 0: rowptr
// (starts at 0, monotone, ends at nnz), bit 1: a column outside [0, num_cols),
// bit 2: a colour outside [0, num_colors).  A row whose bounds are wrong is
// not walked.
__global__ __launch_bounds__(kBlock) void mcgs_check_kernel(
    int32_t n, int32_t num_cols, int64_t nnz, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ colind, const int32_t* __restrict__ colour,
    int32_t num_colors, int32_t* __restrict__ flags)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int bad = 0;
    const int64_t r0 = rowptr[i], r1 = rowptr[i + 1];
    if (r0 < 0 || r1 < r0 || r1 > nnz || (i == 0 && r0 != 0)
        || (i == n - 1 && r1 != nnz)) {
      bad |= 1;
    } else {
      for (int64_t e = r0; e < r1; ++e) {
        const int32_t c = colind[e];
        if (c < 0 || c >= num_cols)
          bad |= 2;
      }
    }
    if (colour && (colour[i] < 0 || colour[i] >= num_colors))
      bad |= 4;
    if (bad)
      atomicOr(flags, bad);
  }
}

__global__ __launch_bounds__(kBlock) void mcgs_iota_kernel(int32_t n,
                                                           int32_t* __restrict__ out)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (int32_t)i;
}

// what the builder's temporaries hold, now and at most
struct TempBytes {
  int64_t now = 0, peak = 0;
  void add(int64_t b)
  {
    now += b;
    peak = now > peak ? now : peak;
  }
};

template <typename T>
struct Temp {
  PlanScratch<T> mem;
  int64_t bytes = 0;
  TempBytes* book = nullptr;
  hipError_t alloc(size_t count, TempBytes* b)
  {
    drop();
    const hipError_t e = mem.alloc(count ? count : 1);
    if (e == hipSuccess) {
      book = b;
      bytes = (int64_t)(sizeof(T) * (count ? count : 1));
      book->add(bytes);
    }
    return e;
  }
  void drop()
  {
    mem.reset();
    if (book)
      book->add(-bytes);
    bytes = 0;
  }
  T* get() const { return mem.get(); }
};

// plan_cub with the call's scratch on the books while it lives
struct CubTemp {
  PlanScratch<void> mem;
  int64_t bytes = 0;
  TempBytes* book = nullptr;
  ~CubTemp()
  {
    if (book)
      book->add(-bytes);
  }
  template <typename Call>
  hipError_t run(TempBytes* b, Call&& call)
  {
    size_t need = 0;
    hipError_t e = call(static_cast<void*>(nullptr), need);
    if (e == hipSuccess)
      e = mem.alloc(need ? need : 16);
    if (e == hipSuccess) {
      book = b;
      bytes = (int64_t)(need ? need : 16);
      book->add(bytes);
      e = call(mem.get(), need);
    }
    return e;
  }
};

#define MB_HIP(expr)                                                           \
  do {                                                                         \
    const hipError_t _e = (expr);                                              \
    if (_e != hipSuccess)                                                      \
      return plan_fail(_e);                                                    \
  } while (0)

int bits_for(int64_t count) // the smallest b >= 1 with 2^b >= count
{
  int b = 1;
  while (b < 62 && ((int64_t)1 << b) < count)
    ++b;
  return b;
}

// in-place exclusive sum over count + 1 int64 (the last addend is zeroed: the
// last element becomes the total)
hipError_t scan_in_place(int64_t* a, int64_t count, hipStream_t st)
{
  hipError_t e = hipMemsetAsync(a + count, 0, sizeof(int64_t), st);
  PlanScratch<void> tmp;
  if (e == hipSuccess)
    e = plan_cub(tmp, [&](void* t, size_t& tb) {
      return hipcub::DeviceScan::ExclusiveSum(t, tb, a, a, (int)(count + 1), st);
    });
  if (e == hipSuccess)
    e = hipStreamSynchronize(st); // tmp goes away with this frame
  return e;
}

// The transposed map of the pattern over all columns, kept for the call.
struct TMap {
  int32_t *ptr = nullptr, *pos = nullptr, *row = nullptr;
  ~TMap()
  {
    plan_drop(ptr);
    plan_drop(pos);
    plan_drop(row);
  }
};

// an array of the plan: `count` elements, none for 0, as the host builders'
// upload() -- plan_bytes of the two builders agree
template <typename T>
hipError_t plan_array(T** field, size_t count, int64_t* bytes)
{
  *field = nullptr;
  if (count == 0)
    return hipSuccess;
  const hipError_t e = spmv_plan_malloc(field, count * sizeof(T));
  if (e == hipSuccess)
    *bytes += (int64_t)(count * sizeof(T));
  else
    *field = nullptr;
  return e;
}

// rowptr of an empty block that owns no arrays
hipError_t zero_rowptr(Temp<int32_t>& mem, int32_t n, TempBytes* book,
                       hipStream_t st, const int32_t** rowptr)
{
  hipError_t e = mem.alloc((size_t)n + 1, book);
  if (e == hipSuccess)
    e = hipMemsetAsync(mem.get(), 0, sizeof(int32_t) * ((size_t)n + 1), st);
  *rowptr = mem.get();
  return e;
}

// flags of mcgs_check_kernel, fetched
int check_input(spmv_hip_ctx* ctx, int32_t n, int32_t num_cols, int64_t nnz,
                const int32_t* rowptr, const int32_t* colind,
                const int32_t* colour, int32_t num_colors, TempBytes* book,
                hipStream_t st, int32_t* flags_out)
{
  Temp<int32_t> flags;
  MB_HIP(flags.alloc(1, book));
  MB_HIP(hipMemsetAsync(flags.get(), 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(mcgs_check_kernel, dim3(spmv_grid_for(ctx, n, kBlock)),
                     dim3(kBlock), 0, st, n, num_cols, nnz, rowptr, colind, colour,
                     num_colors, flags.get());
  MB_HIP(hipGetLastError());
  MB_HIP(plan_fetch(flags_out, flags.get(), 1, st));
  return SPMV_HIP_OK;
}

int build_tmap(spmv_hip_ctx* ctx, int32_t n, int32_t num_cols, int64_t nnz,
               const int32_t* rowptr, const int32_t* colind, TempBytes* book,
               hipStream_t st, TMap* t)
{
  if (nnz == 0)
    return SPMV_HIP_OK;
  int refused = 0;
  const int rc = spmv_tmap_build(ctx, n, nnz, rowptr, colind, 0, num_cols, false,
                                 &t->ptr, &t->pos, &t->row, &refused, st);
  if (rc != SPMV_HIP_OK)
    return plan_fail((hipError_t)rc);
  if (refused) // (the columns were checked: not reached)
    return SPMV_HIP_EINVAL;
  // the map and, while it was built, as much again of spmv_tmap_build's own
  book->add((int64_t)sizeof(int32_t) * (6 * nnz + num_cols + 1));
  book->add(-(int64_t)sizeof(int32_t) * 3 * nnz);
  return SPMV_HIP_OK;
}

bool args_ok(int32_t n, int32_t num_cols, int64_t nnz, const int32_t* rowptr,
             const int32_t* colind)
{
  return n >= 0 && n < INT32_MAX - 1 && num_cols >= n && nnz >= 0
         && nnz <= INT32_MAX
         && (nnz == 0 || (rowptr && colind));
}

} // namespace
