// The streaming core of the solver vector kernels (gfx950): what blas1.hip,
// blas1_pcg.hip, blas1_bicgstab.hip, blas1_cheb.hip and blas1_block.hip share.
// Include it after common.h.  Everything is local to the including file
// (anonymous namespace, macros): no symbol leaves a translation unit.
//
// Streaming shape (measured with tools/membench on MI355X, 1-4 GiB vectors):
// a persistent grid walks UNITS of kU x 4 KiB, every lane keeps kU 16-byte
// loads per stream in flight, and vectors that cannot stay in the 256 MiB
// Infinity Cache anyway are read and written non-temporally.  Against plain
// 16-byte grid-stride loops this gave 4.6-4.9 -> 5.8-5.9 TB/s for the
// two-read-one-write shape (r -= alpha Ap), 4.7-5.0 -> 5.6-5.7 TB/s for the
// three-read-two-write shape (x, p update) and 6.3 -> 7.1 TB/s for dots.
// A vector of n doubles is walked as n / 2 16-byte elements; the odd last
// double, if any, is left to one thread (odd_tail).
#pragma once

#include "common.h"

namespace
{

typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int kU = 4;                           // 16-B loads in flight per stream
constexpr int64_t kUnit = (int64_t)kU * kBlock; // double2 elements per step

template <bool NT>
__device__ __forceinline__ f64x2 vload(const double* p, int64_t i2)
{
  const f64x2* q = reinterpret_cast<const f64x2*>(p) + i2;
  return NT ? __builtin_nontemporal_load(q) : *q;
}
template <bool NT>
__device__ __forceinline__ void vstore(double* p, int64_t i2, f64x2 v)
{
  f64x2* q = reinterpret_cast<f64x2*>(p) + i2;
  if (NT)
    __builtin_nontemporal_store(v, q);
  else
    *q = v;
}
template <bool NT>
__device__ __forceinline__ double sload(const double* p)
{
  return NT ? __builtin_nontemporal_load(p) : *p;
}
template <bool NT>
__device__ __forceinline__ void sstore(double* p, double v)
{
  if (NT)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// for (unit of this workgroup) { load phase ; compute + store phase }
#define SPMV_FOR_UNITS(n2)                                                     \
  for (int64_t base = (int64_t)blockIdx.x * kUnit; base < (n2);               \
       base += (int64_t)gridDim.x * kUnit)
#define SPMV_FOR_LANE_ELEMS(i, n2)                                             \
  _Pragma("unroll") for (int u = 0; u < kU; ++u)                               \
    if (const int64_t i = base + u * kBlock + threadIdx.x; i < (n2))

// this thread handles the odd last element of a vector of n doubles
__device__ __forceinline__ bool odd_tail(int64_t n)
{
  return (n & 1) && blockIdx.x == 0 && threadIdx.x == 0;
}

// sum over the double2 elements [0, n2) of x . y : this thread's share
template <bool NT>
__device__ __forceinline__ double stream_dot(int64_t n2, const double* x,
                                             const double* y)
{
  double acc = 0.0;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 a[kU], b[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      a[u] = vload<NT>(x, i);
      b[u] = vload<NT>(y, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      acc += a[u].x * b[u].x;
      acc += a[u].y * b[u].y;
    }
  }
  return acc;
}

// x += alpha p over the double2 elements [0, n2)
template <bool NT>
__device__ __forceinline__ void stream_axpy(int64_t n2, double alpha,
                                            const double* p, double* x)
{
  SPMV_FOR_UNITS(n2)
  {
    f64x2 pv[kU], xv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      pv[u] = vload<NT>(p, i);
      xv[u] = vload<NT>(x, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      xv[u].x += alpha * pv[u].x;
      xv[u].y += alpha * pv[u].y;
      vstore<NT>(x, i, xv[u]);
    }
  }
}

__device__ __forceinline__ void clear_partials_tail(double* partials, int len)
{
  for (int i = gridDim.x + blockIdx.x * blockDim.x + threadIdx.x; i < len;
       i += gridDim.x * blockDim.x)
    partials[i] = 0.0;
}

// The one way a partial array becomes a scalar: the single-workgroup reducers
// and the consumer-side prologues both go through here, so they agree bit for
// bit.  Valid in thread 0; ends behind a barrier only for thread 0's reads of
// s_red -- callers that reuse s_red synchronise first.
__device__ __forceinline__ double sum_partials(
    const double* __restrict__ partials, const double* __restrict__ partials2,
    int len, double* s_red)
{
  double acc = 0.0;
  for (int i = threadIdx.x; i < len; i += kBlock)
    acc += partials[i];
  if (partials2) // the remote block's share of p.Ap
    for (int i = threadIdx.x; i < len; i += kBlock)
      acc += partials2[i];
  return spmv_block_sum(acc, s_red);
}

// ... and its value in every thread of the workgroup.  Self-contained: on
// return s_red and s_bcast are free, the caller needs no barrier of its own.
__device__ __forceinline__ double consume_partials(
    const double* __restrict__ partials, const double* __restrict__ partials2,
    int len, double* s_red, double* s_bcast)
{
  const double s = sum_partials(partials, partials2, len, s_red);
  if (threadIdx.x == 0)
    *s_bcast = s;
  __syncthreads();
  const double v = *s_bcast;
  __syncthreads(); // s_red and s_bcast may be written again
  return v;
}

// the workgroup's shares of two dot products into their slots (one share:
// spmv_dot_epilogue of common.h)
__device__ __forceinline__ void store_pair_partials(
    double acc_a, double acc_b, double* __restrict__ partials_a,
    double* __restrict__ partials_b, int len, double* s_red)
{
  const double s_a = spmv_block_sum(acc_a, s_red);
  __syncthreads(); // s_red is reused
  const double s_b = spmv_block_sum(acc_b, s_red);
  if (threadIdx.x == 0) {
    partials_a[blockIdx.x] = s_a;
    partials_b[blockIdx.x] = s_b;
  }
  clear_partials_tail(partials_a, len);
  clear_partials_tail(partials_b, len);
}

// ---- host side ----------------------------------------------------------------
// the 16-byte accesses above need 16-byte aligned vectors (null passes: the
// entry points check separately which vectors a length requires)
template <typename... P>
bool aligned16(const P*... p)
{
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 15u) == 0;
}

// grid of a streaming kernel over a vector of n doubles ...
int stream_grid(const spmv_hip_ctx* ctx, int64_t n)
{
  return spmv_grid_for(ctx, n / 2, (int)kUnit);
}
// ... where every workgroup leaves a partial: never more than the array holds
int stream_grid_capped(const spmv_hip_ctx* ctx, int64_t n)
{
  const int grid = stream_grid(ctx, n);
  return grid > ctx->dot_blocks ? ctx->dot_blocks : grid;
}

} // namespace

// Vectors of at least ctx->blas1_nt_min_elems doubles stream past the caches
// (non-temporal loads and stores); shorter ones stay cached between kernels.
#define SPMV_LAUNCH_NT(ctx, n, kernel, grid, st, ...)                          \
  do {                                                                         \
    if ((int64_t)(n) >= (ctx)->blas1_nt_min_elems)                             \
      hipLaunchKernelGGL(kernel<true>, dim3(grid), dim3(kBlock), 0, st,        \
                         __VA_ARGS__);                                         \
    else                                                                       \
      hipLaunchKernelGGL(kernel<false>, dim3(grid), dim3(kBlock), 0, st,       \
                         __VA_ARGS__);                                         \
  } while (0)

// every kernel of iteration k: the workspace is this context's, k in range
#define SPMV_REQUIRE_WS_K(ctx, ws, k, kmin)                                    \
  SPMV_REQUIRE((ws) && (ws)->ctx == (ctx) && (k) >= (kmin) && (k) <= (ws)->kmax)
