// What the vector kernels of the two block solvers share (blas1_block.hip:
// cg_block; blas1_pcg_block.hip: pcg_block): blocks of nrhs INTERLEAVED
// vectors, element (i, c) at V[i * nrhs + c]; partials [len][nrhs], added in
// index order per column.  Include it after common.h.  Everything is local to
// the including file (anonymous namespace, macros).
#pragma once

#include "common.h"
#include "blas1_stream.h"
#include "pcgb_ws.h"

namespace
{

__device__ __forceinline__ void clear_partials_tail(double* partials, int len,
                                                    int nrhs)
{
  for (int i = gridDim.x * nrhs + blockIdx.x * blockDim.x + threadIdx.x;
       i < len * nrhs; i += gridDim.x * blockDim.x)
    partials[i] = 0.0;
}

// ---- K = 2, 4, 8 ------------------------------------------------------------
// The workgroup's sums of its lanes' two accumulators, per column: lanes of
// equal tid % (K/2) hold the same column pair and are combined with shuffles
// at offsets 32 ... K/2, the waves through LDS in wave order.
template <int K>
__device__ __forceinline__ void block_sum_pairs(double a0, double a1,
                                                double (*s_red)[K], double* out)
{
#pragma unroll
  for (int off = 32; off >= K / 2; off >>= 1) {
    a0 += __shfl_down(a0, off, 64);
    a1 += __shfl_down(a1, off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < K / 2) {
    s_red[wave][2 * lane] = a0;
    s_red[wave][2 * lane + 1] = a1;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double r = 0.0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w)
      r += s_red[w][threadIdx.x];
    out[threadIdx.x] = r;
  }
}

// ---- nrhs at run time (1..8): one thread per row -----------------------------
// one block sum per column, columns in order (nrhs is uniform)
__device__ __forceinline__ void rows_epilogue(const double (&acc)[SPMV_CGB_MAX],
                                              int nrhs, double* s_red,
                                              double* partials, int len)
{
#pragma unroll
  for (int c = 0; c < SPMV_CGB_MAX; ++c) {
    if (c < nrhs) {
      const double s = spmv_block_sum(acc[c], s_red);
      if (threadIdx.x == 0)
        partials[(int64_t)blockIdx.x * nrhs + c] = s;
      __syncthreads(); // s_red is reused
    }
  }
  clear_partials_tail(partials, len, nrhs);
}

#define SPMV_FOR_ROWS(row, M)                                                  \
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;           \
       row < (M); row += (int64_t)gridDim.x * blockDim.x)
#define SPMV_FOR_COLS(c, nrhs)                                                 \
  _Pragma("unroll") for (int c = 0; c < SPMV_CGB_MAX; ++c) if (c < (nrhs))

__device__ __forceinline__ int done_mask(const CgbState* st, int nrhs)
{
  int m = 0;
  for (int c = 0; c < nrhs; ++c)
    m |= st->done[c] ? (1 << c) : 0;
  return m;
}

// ---- reducers (one workgroup) -------------------------------------------------
// the sum of column c of the partials, added as reduce_partials_kernel does
__device__ __forceinline__ double reduce_column(const double* partials, int len,
                                                int nrhs, int c, double* s_red)
{
  double acc = 0.0;
  for (int i = threadIdx.x; i < len; i += kBlock)
    acc += partials[(int64_t)i * nrhs + c];
  const double s = spmv_block_sum(acc, s_red);
  __syncthreads(); // s_red is reused by the next column
  return s;        // valid in thread 0
}

// ---- host side ----------------------------------------------------------------
bool native_width(int nrhs) { return nrhs == 2 || nrhs == 4 || nrhs == 8; }

bool nrhs_ok(int nrhs) { return nrhs >= 1 && nrhs <= SPMV_CGB_MAX; }

// grid of the row kernels (the streaming kernels: stream_grid_capped)
int rows_grid(const spmv_hip_ctx* ctx, int64_t M)
{
  const int g = spmv_grid_for(ctx, M, kBlock);
  return g < ctx->dot_blocks ? g : ctx->dot_blocks;
}

} // namespace

// Blocks of at least ctx->blas1_nt_min_elems doubles (M * nrhs) stream past the
// caches, like the vectors of blas1.hip.
#define SPMV_CGB_LAUNCH_NT(nt, kernel, grid, st, ...)                          \
  do {                                                                         \
    if (nt)                                                                    \
      hipLaunchKernelGGL((kernel<true>), dim3(grid), dim3(kBlock), 0, st,      \
                         __VA_ARGS__);                                         \
    else                                                                       \
      hipLaunchKernelGGL((kernel<false>), dim3(grid), dim3(kBlock), 0, st,     \
                         __VA_ARGS__);                                         \
  } while (0)
#define SPMV_CGB_LAUNCH_K(K, nt, kernel, grid, st, ...)                        \
  do {                                                                         \
    if (nt)                                                                    \
      hipLaunchKernelGGL((kernel<K, true>), dim3(grid), dim3(kBlock), 0, st,   \
                         __VA_ARGS__);                                         \
    else                                                                       \
      hipLaunchKernelGGL((kernel<K, false>), dim3(grid), dim3(kBlock), 0, st,  \
                         __VA_ARGS__);                                         \
  } while (0)
// nrhs = 2, 4, 8: the streaming kernel of that width
#define SPMV_CGB_LAUNCH_WIDTH(nrhs, nt, kernel, grid, st, ...)                 \
  do {                                                                         \
    if ((nrhs) == 2)                                                           \
      SPMV_CGB_LAUNCH_K(2, nt, kernel, grid, st, __VA_ARGS__);                 \
    else if ((nrhs) == 4)                                                      \
      SPMV_CGB_LAUNCH_K(4, nt, kernel, grid, st, __VA_ARGS__);                 \
    else                                                                       \
      SPMV_CGB_LAUNCH_K(8, nt, kernel, grid, st, __VA_ARGS__);                 \
  } while (0)
