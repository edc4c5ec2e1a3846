// Multi-vector SpMV (Matrix::mult_block): Y = alpha A X + beta Y for a block of
// k vectors, for gfx950 (MI355X).
//
// LAYOUT.  A block of k vectors is interleaved (row-major): element (i, c)
// lives at X[i * k + c].  One gathered column of the matrix then fetches the k
// values of that x row from one place -- 8 k useful bytes of the 128-byte line
// instead of 8 -- and the matrix stream (12 B per entry + 4 B per row) is read
// once for all k vectors.
//
// BITS.  Column c of Y has the bits of the single-vector product on column c
// of X: per row the products are added left to right starting from +0.0, mul
// and add rounded separately (-ffp-contract=off), alpha * sum, then
// + beta * y only when beta != 0 (csr_kernels.cpp:41-51).
//
// NATIVE kernel (general blocks, fp64 vectors, K = 2, 4, 8; values fp64 or
// fp32): csr_rowblock_kernel's scheme with K products per entry.
//   * A workgroup of 256 threads owns RB = 512 / K consecutive rows.  Their
//     span of the CSR arrays is streamed in tiles: every lane loads two
//     consecutive entries (16 B of fp64 values, 8 B of column indices,
//     coalesced, optionally non-temporal), then the K values of both x rows
//     with K / 2 16-byte loads each, and parks the 2 K products in LDS.
//   * LDS holds one plane per column PAIR: s_prod[p][e] is the 16-byte pair
//     (columns 2p, 2p + 1) of entry e.  A lane's two entries are 32 contiguous
//     bytes of a plane (ds_write_b128, lanes 32 B apart: 2-way on the 32-bank
//     write path, below the store's own transfer time); an entry-major layout
//     [e][K] would put the lanes 16 K bytes apart -- 4- and 8-way conflicts.
//   * Thread t owns row t % RB and column pair t / RB: K / 2 threads per row,
//     each with two independent sums, so all 256 threads add whatever K is.
//     A wave reads ONE plane with consecutive rows in consecutive lanes
//     (ds_read_b128; rows of 7 entries are 112 B apart: conflict-free over the
//     64 banks), strictly left to right.
//   * Tile = 1024 entries for K = 2, 512 for K = 4 and 8: 16, 16 and 32 KiB of
//     products, i.e. 8, 8 and 4 workgroups per CU out of 160 KiB (32, 32, 16
//     waves).  The single-vector kernel's 8 KiB tile would be 32 / 64 KiB here.
//   * y: one 16-byte store per thread, the K / 2 threads of a row side by side.
//
// FALLBACK (symmetric storage, any other k, released CSR arrays, the fp32
// library type, plan key "mv_native" = 0): X is de-interleaved into plan-owned
// scratch, the plan's single-vector launch runs once per column in whatever
// form the plan chose, and Y is interleaved back (de-interleaved first when
// beta != 0).  Total and bit-exact for every storage and plan form.
#include "csr_plan.h"

#include <cstring>

#include "plan_scratch.h"

namespace
{

constexpr int kMvTr = 128; // rows per transpose tile
constexpr int kMvTc = 16;  // columns per transpose tile

// n x k interleaved -> k columns of stride ld, through an LDS tile: the loads
// walk whole rows (contiguous when k <= kMvTc), the stores one column each
template <typename T>
__global__ __launch_bounds__(kBlock) void mv_deinterleave_kernel(
    int64_t n, int k, const T* __restrict__ in, T* __restrict__ cols, int64_t ld)
{
  __shared__ T s_tile[kMvTc][kMvTr + 1];
  const int64_t ntr = (n + kMvTr - 1) / kMvTr;
  const int ntc = (k + kMvTc - 1) / kMvTc;
  for (int64_t tile = blockIdx.x; tile < ntr * ntc; tile += gridDim.x) {
    const int64_t i0 = (tile / ntc) * kMvTr;
    const int c0 = (int)(tile % ntc) * kMvTc;
    const int nr = (int)min((int64_t)kMvTr, n - i0);
    const int nc = min(kMvTc, k - c0);
    __syncthreads();
    for (int idx = threadIdx.x; idx < nr * nc; idx += kBlock) {
      const int r = idx / nc, c = idx % nc;
      s_tile[c][r] = in[(i0 + r) * k + c0 + c];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nr * nc; idx += kBlock) {
      const int c = idx / nr, r = idx % nr;
      cols[(int64_t)(c0 + c) * ld + i0 + r] = s_tile[c][r];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void mv_interleave_kernel(
    int64_t n, int k, const T* __restrict__ cols, int64_t ld, T* __restrict__ out)
{
  __shared__ T s_tile[kMvTc][kMvTr + 1];
  const int64_t ntr = (n + kMvTr - 1) / kMvTr;
  const int ntc = (k + kMvTc - 1) / kMvTc;
  for (int64_t tile = blockIdx.x; tile < ntr * ntc; tile += gridDim.x) {
    const int64_t i0 = (tile / ntc) * kMvTr;
    const int c0 = (int)(tile % ntc) * kMvTc;
    const int nr = (int)min((int64_t)kMvTr, n - i0);
    const int nc = min(kMvTc, k - c0);
    __syncthreads();
    for (int idx = threadIdx.x; idx < nr * nc; idx += kBlock) {
      const int c = idx / nr, r = idx % nr;
      s_tile[c][r] = cols[(int64_t)(c0 + c) * ld + i0 + r];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nr * nc; idx += kBlock) {
      const int r = idx / nc, c = idx % nc;
      out[(i0 + r) * k + c0 + c] = s_tile[c][r];
    }
  }
}

// ghost pack of a block: out[g * k + c] = in[indices[g] * k + c]
template <typename T>
__global__ __launch_bounds__(kBlock) void mv_gather_block_kernel(
    int64_t total, int k, const int32_t* __restrict__ indices,
    const T* __restrict__ in, T* __restrict__ out)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = i / k;
    const int c = (int)(i - g * k);
    out[i] = in[(int64_t)indices[g] * k + c];
  }
}

template <typename TV>
struct MvVal;
template <>
struct MvVal<double> {
  using pair_t = f64x2;
};
template <>
struct MvVal<float> {
  typedef float pair_t __attribute__((ext_vector_type(2)));
};

// ---------------------------------------------------------------------------
// the native kernel (see the head of the file)
//   TV  = type of `values` (double, or float: the mixed-precision product)
//   K   = vectors in the block (2, 4, 8)
//   NT  = non-temporal loads for the read-once matrix stream
//   wide: values / colind allow the two-entry loads (uniform)
// ---------------------------------------------------------------------------
template <typename TV, int K, bool NT>
__global__ __launch_bounds__(kBlock) void csr_mv_rowblock_kernel(
    int32_t num_rows, int64_t nnz, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ colind, const TV* __restrict__ values,
    double alpha, const double* __restrict__ in, double beta,
    double* __restrict__ out, int wide, RowBlockOrder ord)
{
  constexpr int V = 2;               // entries per lane and load
  constexpr int CH = K == 2 ? 2 : 1; // loads per lane and tile
  constexpr int TILE = kBlock * CH * V;
  constexpr int NP = K / 2;          // column pairs = threads per row
  constexpr int RB = kBlock / NP;    // rows per workgroup
  static_assert(K == 2 || K == 4 || K == 8, "K");
  using val_t = typename MvVal<TV>::pair_t;

  __shared__ __attribute__((aligned(16))) f64x2 s_prod[NP * TILE];
  __shared__ int32_t s_rowptr[RB + 1];

  const int t = threadIdx.x;
  const int row = t % RB; // (a wave holds one column pair: RB >= 64)
  const int pr = t / RB;
  const f64x2* sp = s_prod + pr * TILE;

  const int num_slots = order_slots(ord);
  for (int it = blockIdx.x; it < num_slots; it += gridDim.x) {
    const int rb = order_row_block(ord, it);
    if (rb < 0)
      continue; // uniform per workgroup
    const int32_t r0 = rb * RB;
    const int nr = min(RB, num_rows - r0);

    __syncthreads(); // previous iteration done with s_rowptr / s_prod
    if (t <= nr)
      s_rowptr[t] = rowptr[r0 + t];
    if (RB == kBlock && t == 0 && nr == RB)
      s_rowptr[RB] = rowptr[r0 + RB];
    __syncthreads();

    const int32_t a = s_rowptr[0];
    const int32_t b = s_rowptr[nr];
    int32_t lo = 0, hi = 0;
    if (row < nr) {
      lo = s_rowptr[row];
      hi = s_rowptr[row + 1];
    }
    f64x2 sum = {0.0, 0.0};

    // tiles start V-aligned so the wide loads are naturally aligned
    const int64_t base0 = a & ~(V - 1);
    // last V-aligned slot of the span: lanes past it re-read that slot
    const int64_t jclamp = (int64_t)(b - 1) & ~(int64_t)(V - 1);
    for (int64_t base = base0; base < b; base += TILE) {
      if (base != base0)
        __syncthreads(); // row owners finished reading the previous tile
      if (wide && jclamp + V <= nnz) {
        // all matrix loads, then all gathers, then the products
        val_t v[CH];
        i32x2 ci[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int64_t j0 = base + (int64_t)(c * kBlock + t) * V;
          const int64_t jl = j0 < jclamp ? j0 : jclamp;
          v[c] = stream_load<NT>(reinterpret_cast<const val_t*>(values + jl));
          ci[c] = stream_load<NT>(reinterpret_cast<const i32x2*>(colind + jl));
        }
        f64x2 xg[CH][V][NP];
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const f64x2* xr
                = reinterpret_cast<const f64x2*>(in + (int64_t)ci[c][e] * K);
#pragma unroll
            for (int p = 0; p < NP; ++p)
              xg[c][e][p] = xr[p];
          }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int64_t j0 = base + (int64_t)(c * kBlock + t) * V;
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const bool live = j0 + e < b;
            const double ve = (double)v[c][e];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
              f64x2 pv;
              pv[0] = live ? ve * xg[c][e][p][0] : 0.0;
              pv[1] = live ? ve * xg[c][e][p][1] : 0.0;
              s_prod[p * TILE + (c * kBlock + t) * V + e] = pv;
            }
          }
        }
      } else { // unaligned arrays, or the last row block: element-wise
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int64_t j0 = base + (int64_t)(c * kBlock + t) * V;
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const int64_t j = j0 + e;
            const bool live = j < b;
            double ve = 0.0;
            const f64x2* xr = reinterpret_cast<const f64x2*>(in);
            if (live) {
              ve = (double)values[j];
              xr = reinterpret_cast<const f64x2*>(in + (int64_t)colind[j] * K);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
              f64x2 pv = {0.0, 0.0};
              if (live) {
                const f64x2 x = xr[p];
                pv[0] = ve * x[0];
                pv[1] = ve * x[1];
              }
              s_prod[p * TILE + (c * kBlock + t) * V + e] = pv;
            }
          }
        }
      }
      // entries in [base, a) belong to earlier rows: no row of this block
      // reads their products
      __syncthreads();
      const int32_t jlo = max((int64_t)lo, base) - base;
      const int32_t jhi = min((int64_t)hi, base + TILE) - base;
      int32_t j = jlo;
      // four LDS reads in flight, adds strictly left to right per column
      for (; j + 4 <= jhi; j += 4) {
        const f64x2 p0 = sp[j], p1 = sp[j + 1], p2 = sp[j + 2], p3 = sp[j + 3];
        sum += p0;
        sum += p1;
        sum += p2;
        sum += p3;
      }
      for (; j < jhi; ++j)
        sum += sp[j];
    }

    if (row < nr) {
      f64x2* yp = reinterpret_cast<f64x2*>(out + (int64_t)(r0 + row) * K + 2 * pr);
      f64x2 c;
      c[0] = alpha * sum[0];
      c[1] = alpha * sum[1];
      f64x2 y = c;
      if (beta != 0.0) {
        const f64x2 yo = *yp;
        y[0] = c[0] + beta * yo[0];
        y[1] = c[1] + beta * yo[1];
      }
      *yp = y;
    }
  }
}

template <typename TV, int K>
int launch_native_k(const spmv_hip_csr_plan* pl, hipStream_t st,
                    const int32_t* rowptr, const int32_t* colind,
                    const TV* values, double alpha, const double* in,
                    double beta, double* out)
{
  constexpr int RB = kBlock / (K / 2);
  const int nrb = (pl->num_rows + RB - 1) / RB;
  // LDS: 16 KiB of products (K = 2, 4) or 32 KiB (K = 8) per workgroup
  int grid = pl->ctx->num_cus * (K == 8 ? 4 : kBlocksPerCU);
  if (grid > nrb)
    grid = nrb;
  if (grid < 1)
    grid = 1;
  if (grid >= 8) // slots with equal it % 8 stay on one XCD (XCD groups)
    grid -= grid % 8;
  const RowBlockOrder ord = pl->row_block_order(nrb);
  // two entries per load: 2 * sizeof(TV) bytes of values, 8 of column indices
  const int wide = (reinterpret_cast<uintptr_t>(values) % (2 * sizeof(TV)) == 0
                    && reinterpret_cast<uintptr_t>(colind) % 8 == 0)
                       ? 1
                       : 0;
  if (pl->nontemporal)
    hipLaunchKernelGGL((csr_mv_rowblock_kernel<TV, K, true>), dim3(grid),
                       dim3(kBlock), 0, st, pl->num_rows, pl->nnz, rowptr, colind,
                       values, alpha, in, beta, out, wide, ord);
  else
    hipLaunchKernelGGL((csr_mv_rowblock_kernel<TV, K, false>), dim3(grid),
                       dim3(kBlock), 0, st, pl->num_rows, pl->nnz, rowptr, colind,
                       values, alpha, in, beta, out, wide, ord);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

template <typename TV>
int launch_native(const spmv_hip_csr_plan* pl, hipStream_t st,
                  const int32_t* rowptr, const int32_t* colind, const TV* values,
                  double alpha, const double* in, double beta, double* out, int k)
{
  if (k == 2)
    return launch_native_k<TV, 2>(pl, st, rowptr, colind, values, alpha, in, beta,
                                  out);
  if (k == 4)
    return launch_native_k<TV, 4>(pl, st, rowptr, colind, values, alpha, in, beta,
                                  out);
  return launch_native_k<TV, 8>(pl, st, rowptr, colind, values, alpha, in, beta,
                                out);
}

template <typename T>
int launch_deinterleave(spmv_hip_ctx* ctx, int64_t n, int k, const T* in, T* cols,
                        int64_t ld, hipStream_t st)
{
  const int64_t tiles = ((n + kMvTr - 1) / kMvTr) * ((k + kMvTc - 1) / kMvTc);
  const int grid = spmv_grid_for(ctx, tiles, 1);
  hipLaunchKernelGGL((mv_deinterleave_kernel<T>), dim3(grid), dim3(kBlock), 0, st,
                     n, k, in, cols, ld);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

template <typename T>
int launch_interleave(spmv_hip_ctx* ctx, int64_t n, int k, const T* cols,
                      int64_t ld, T* out, hipStream_t st)
{
  const int64_t tiles = ((n + kMvTr - 1) / kMvTr) * ((k + kMvTc - 1) / kMvTc);
  const int grid = spmv_grid_for(ctx, tiles, 1);
  hipLaunchKernelGGL((mv_interleave_kernel<T>), dim3(grid), dim3(kBlock), 0, st, n,
                     k, cols, ld, out);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

// column stride of the scratch: whole units of 4 elements (32 bytes of fp64, 16
// of fp32), so that every column
// starts as aligned as the scratch itself (some plan forms need 16 bytes)
inline int64_t mv_stride(int64_t n) { return (n + 3) & ~(int64_t)3; }

// the plan's scratch, at least `bytes` long (grown on demand)
int mv_scratch(spmv_hip_csr_plan* pl, size_t bytes, hipStream_t st)
{
  if (pl->mv_scratch && pl->mv_bytes >= bytes)
    return SPMV_HIP_OK;
  if (pl->mv_scratch) {
    // an earlier launch, on this stream or another, may still read it
    // (this stream's launches; hipFree itself waits for the rest of the device)
    SPMV_CHECK_HIP(hipStreamSynchronize(st));
    plan_drop(pl->mv_scratch);
    pl->mv_bytes = 0;
  }
  void* p = nullptr;
  const hipError_t e = spmv_plan_malloc(&p, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return static_cast<int>(e);
  }
  pl->mv_scratch = p;
  pl->mv_bytes = bytes;
  return SPMV_HIP_OK;
}

template <typename T>
bool ranges_overlap(const T* in, int64_t n_in, const T* out, int64_t n_out)
{
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(in);
  const uintptr_t a1 = a0 + sizeof(T) * (uintptr_t)n_in;
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(out);
  const uintptr_t b1 = b0 + sizeof(T) * (uintptr_t)n_out;
  return a0 < b1 && b0 < a1;
}

// one single-vector launch of the plan, by value / vector type
int run_single(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* pl, int32_t nr,
               int32_t nc, int64_t nnz, const int32_t* rowptr,
               const int32_t* colind, const double* values, const double* diagonal,
               double alpha, const double* in, double beta, double* out,
               hipStream_t st)
{
  return spmv_hip_csr_spmv_f64(ctx, pl, nr, nc, nnz, rowptr, colind, values,
                               diagonal, alpha, in, beta, out, nullptr, st);
}
int run_single(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* pl, int32_t nr,
               int32_t nc, int64_t nnz, const int32_t* rowptr,
               const int32_t* colind, const float* values, const float* diagonal,
               float alpha, const float* in, float beta, float* out,
               hipStream_t st)
{
  return spmv_hip_csr_spmv_f32(ctx, pl, nr, nc, nnz, rowptr, colind, values,
                               diagonal, alpha, in, beta, out, st);
}
int run_single(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* pl, int32_t nr,
               int32_t nc, int64_t nnz, const int32_t* rowptr,
               const int32_t* colind, const float* values, const double*,
               double alpha, const double* in, double beta, double* out,
               hipStream_t st)
{
  return spmv_hip_csr_spmv_f32f64(ctx, pl, nr, nc, nnz, rowptr, colind, values,
                                  alpha, in, beta, out, nullptr, st);
}

// TV: values, T: vectors and arithmetic
template <typename TV, typename T>
int run_block(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan, int32_t num_rows,
              int32_t num_cols, int64_t nnz, const int32_t* rowptr,
              const int32_t* colind, const TV* values, const T* diagonal, T alpha,
              const T* in, T beta, T* out, int k, void* stream)
{
  constexpr bool mixed = sizeof(TV) != sizeof(T);
  SPMV_REQUIRE(k >= 1);
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(plan && plan->ctx == ctx);
  SPMV_REQUIRE(!mixed || (!plan->symmetric && !plan->released));
  SPMV_REQUIRE(num_rows == plan->num_rows && num_cols == plan->num_cols
               && nnz == plan->nnz);
  SPMV_REQUIRE(!plan->structure_baked()
               || (rowptr == plan->rowptr0 && colind == plan->colind0));
  if (num_rows == 0)
    return SPMV_HIP_OK;
  SPMV_REQUIRE(in && out);
  SPMV_REQUIRE(nnz == 0 || (rowptr && colind && values));
  SPMV_REQUIRE(!ranges_overlap(in, (int64_t)num_cols * k, out, (int64_t)num_rows * k));
  hipStream_t st = spmv_stream(ctx, stream);
  if (k == 1) { // the existing product, as it is: one column, no scratch
    const int rc = run_single(ctx, plan, num_rows, num_cols, nnz, rowptr, colind,
                              values, diagonal, alpha, in, beta, out, st);
    if (rc == SPMV_HIP_OK)
      plan->mv_form = 2;
    return rc;
  }
  if (nnz == 0 && !plan->symmetric) { // out = alpha*0 + beta*out, all k columns
    const int64_t n = (int64_t)num_rows * k;
    const int grid = spmv_grid_for(ctx, n, kBlock);
    hipLaunchKernelGGL((empty_rows_kernel<T>), dim3(grid), dim3(kBlock), 0, st, n,
                       alpha * T(0), beta, out);
    SPMV_CHECK_LAUNCH();
    plan->mv_form = 2;
    return SPMV_HIP_OK;
  }
  if constexpr (sizeof(T) == 8) {
    if (plan->mv_native && !plan->symmetric && !plan->released
        && (k == 2 || k == 4 || k == 8) && aligned16(in) && aligned16(out)) {
      const int rc = launch_native<TV>(plan, st, rowptr, colind, values, alpha, in,
                                       beta, out, k);
      if (rc == SPMV_HIP_OK)
        plan->mv_form = 1;
      return rc;
    }
  }
  // per-column fallback through the plan's own single-vector launch; what that
  // launch would refuse is refused here, before the scratch and the transposes
  // (the columns of the scratch are 16-byte aligned)
  SPMV_REQUIRE(!plan->released
               || spmv_released_launch_ok(plan, values, nullptr, diagonal,
                                          (int)sizeof(T)));
  const int64_t ldx = mv_stride(num_cols), ldy = mv_stride(num_rows);
  const int rs = mv_scratch(plan, sizeof(T) * (size_t)(ldx + ldy) * (size_t)k, st);
  if (rs != SPMV_HIP_OK)
    return rs;
  T* xs = static_cast<T*>(plan->mv_scratch);
  T* ys = xs + ldx * k;
  int rc = launch_deinterleave<T>(ctx, num_cols, k, in, xs, ldx, st);
  if (rc == SPMV_HIP_OK && beta != T(0))
    rc = launch_deinterleave<T>(ctx, num_rows, k, out, ys, ldy, st);
  for (int c = 0; c < k && rc == SPMV_HIP_OK; ++c)
    rc = run_single(ctx, plan, num_rows, num_cols, nnz, rowptr, colind, values,
                    diagonal, alpha, xs + ldx * c, beta, ys + ldy * c, st);
  if (rc == SPMV_HIP_OK)
    rc = launch_interleave<T>(ctx, num_rows, k, ys, ldy, out, st);
  if (rc == SPMV_HIP_OK)
    plan->mv_form = 2;
  return rc;
}

template <typename T>
int transpose_entry(spmv_hip_ctx* ctx, bool to_interleaved, int64_t n, int k,
                    const T* in, int64_t ld, T* out, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(n >= 0 && k >= 1 && ld >= n);
  if (n == 0)
    return SPMV_HIP_OK;
  SPMV_REQUIRE(in && out);
  const int64_t n_cols = ld * (k - 1) + n, n_il = n * k;
  SPMV_REQUIRE(!ranges_overlap(in, to_interleaved ? n_cols : n_il, out,
                               to_interleaved ? n_il : n_cols));
  hipStream_t st = spmv_stream(ctx, stream);
  if (to_interleaved)
    return launch_interleave<T>(ctx, n, k, in, ld, out, st);
  return launch_deinterleave<T>(ctx, n, k, in, out, ld, st);
}

template <typename T>
int gather_block_entry(spmv_hip_ctx* ctx, int num_indices, const int32_t* indices,
                       int k, const T* in, T* out, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(num_indices >= 0 && k >= 1);
  if (num_indices == 0)
    return SPMV_HIP_OK;
  SPMV_REQUIRE(indices && in && out);
  const int64_t total = (int64_t)num_indices * k;
  const int grid = spmv_grid_for(ctx, total, kBlock);
  hipLaunchKernelGGL((mv_gather_block_kernel<T>), dim3(grid), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), total, k, indices, in, out);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // namespace

// --- plan API hooks (spmv_csr_plan.hip) ---------------------------------------
void spmv_mv_free(spmv_hip_csr_plan* pl)
{
  if (!pl->mv_scratch)
    return;
  (void)hipSetDevice(pl->ctx->device);
  plan_drop(pl->mv_scratch);
  pl->mv_bytes = 0;
}

extern "C" {

int spmv_hip_csr_spmm_f64(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan,
                          int32_t num_rows, int32_t num_cols,
                          int64_t num_non_zeros, const int32_t* rowptr,
                          const int32_t* colind, const double* values,
                          const double* diagonal, double alpha, const double* in,
                          double beta, double* out, int k, void* stream)
{
  return run_block<double, double>(ctx, plan, num_rows, num_cols, num_non_zeros,
                                   rowptr, colind, values, diagonal, alpha, in,
                                   beta, out, k, stream);
}

int spmv_hip_csr_spmm_f32f64(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan,
                             int32_t num_rows, int32_t num_cols,
                             int64_t num_non_zeros, const int32_t* rowptr,
                             const int32_t* colind, const float* values,
                             const double* diagonal, double alpha,
                             const double* in, double beta, double* out, int k,
                             void* stream)
{
  SPMV_REQUIRE(diagonal == nullptr); // (general blocks only)
  return run_block<float, double>(ctx, plan, num_rows, num_cols, num_non_zeros,
                                  rowptr, colind, values, diagonal, alpha, in,
                                  beta, out, k, stream);
}

int spmv_hip_csr_spmm_f32(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan,
                          int32_t num_rows, int32_t num_cols,
                          int64_t num_non_zeros, const int32_t* rowptr,
                          const int32_t* colind, const float* values,
                          const float* diagonal, float alpha, const float* in,
                          float beta, float* out, int k, void* stream)
{
  return run_block<float, float>(ctx, plan, num_rows, num_cols, num_non_zeros,
                                 rowptr, colind, values, diagonal, alpha, in, beta,
                                 out, k, stream);
}

int spmv_hip_interleave_f64(spmv_hip_ctx* ctx, int64_t n, int k,
                            const double* columns, int64_t ld, double* out,
                            void* stream)
{
  return transpose_entry<double>(ctx, true, n, k, columns, ld, out, stream);
}

int spmv_hip_interleave_f32(spmv_hip_ctx* ctx, int64_t n, int k,
                            const float* columns, int64_t ld, float* out,
                            void* stream)
{
  return transpose_entry<float>(ctx, true, n, k, columns, ld, out, stream);
}

int spmv_hip_deinterleave_f64(spmv_hip_ctx* ctx, int64_t n, int k, const double* in,
                              int64_t ld, double* columns, void* stream)
{
  return transpose_entry<double>(ctx, false, n, k, in, ld, columns, stream);
}

int spmv_hip_deinterleave_f32(spmv_hip_ctx* ctx, int64_t n, int k, const float* in,
                              int64_t ld, float* columns, void* stream)
{
  return transpose_entry<float>(ctx, false, n, k, in, ld, columns, stream);
}

int spmv_hip_gather_block_f64(spmv_hip_ctx* ctx, int num_indices,
                              const int32_t* indices, int k, const double* in,
                              double* out, void* stream)
{
  return gather_block_entry<double>(ctx, num_indices, indices, k, in, out, stream);
}

int spmv_hip_gather_block_f32(spmv_hip_ctx* ctx, int num_indices,
                              const int32_t* indices, int k, const float* in,
                              float* out, void* stream)
{
  return gather_block_entry<float>(ctx, num_indices, indices, k, in, out, stream);
}

} // extern "C"
