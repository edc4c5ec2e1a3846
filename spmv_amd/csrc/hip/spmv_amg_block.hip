// The AMG V-cycle for blocks of nrhs INTERLEAVED vectors (gfx950): the vector
// kernels of spmv::amg_apply_block.  Element (i, c) of a block lives at
// V[i * nrhs + c], the layout of Matrix::mult_block; d-inverse, the aggregates
// and the member lists are shared by all columns.  Column c of every result
// has the bits of the single-vector kernel (blas1_cheb.hip, spmv_amg.hip) on
// column c: the element arithmetic is amg_elem.h's, and no sum crosses a column.
//
//   cheb_apply0_block   d = b0 * (dinv*r) ; z = d
//   cheb_step_block     d = a*d + b*(dinv*(r - w)) ; z = z + d   (no dot: the
//                       cycle never runs inside a solver's state)
//   amg_post0_block     d = b0 * (dinv*(r - w)) ; z = z + d
//   amg_prolong_block   z(i, c) = z(i, c) + scale * e(agg[i], c)     (streams z)
//   amg_restrict_block  rc(I, c) = (t_0 + t_1) + ..., t_m = r(i_m, c) - w(i_m, c)
//                       over the members of I ascending
//
// Two forms of each, as in blas1_block.hip:
//   K = 2, 4, 8 (all block pointers 16-byte aligned): the block is walked as
//     n * K / 2 16-byte elements on blas1_stream.h's units; element e is the
//     column pair (2p, 2p + 1), p = e % (K/2), of row e / (K/2).  The K/2 lanes
//     of a row sit side by side and read the row's dinv / agg word in the same
//     load instruction: one fetch per row.  Prolong gathers the K contiguous
//     doubles of the coarse row with those K/2 lanes' 16-byte loads.  Restrict
//     runs one lane per (aggregate, column pair).  No odd tail: n * K is even.
//   nrhs at run time (1, 3, 5, 6, 7, or a pointer that is only 8-byte aligned):
//     one thread per row (per aggregate), scalar accesses, the columns in order.
//
// No kernel waits on another workgroup; no atomics.  Built with
// -ffp-contract=off: every product, sum and difference is a rounding of its own.
#include "common.h"
#include "blas1_stream.h"
#include "amg_elem.h"
#include "amg_plan.h"

namespace
{

constexpr int kMaxNrhs = SPMV_HIP_CGB_MAX_NRHS;

// log2(K / 2)
template <int K>
struct PairShift {
  static_assert(K == 2 || K == 4 || K == 8, "compiled widths");
  static constexpr int value = K == 2 ? 0 : K == 4 ? 1 : 2;
};

#define SPMV_FOR_ROWS(row, M)                                                  \
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;           \
       row < (M); row += (int64_t)gridDim.x * blockDim.x)

// ---- step 0 from z = 0 -------------------------------------------------------
// LAST: the iteration has one step, d is not written
template <int K, bool NT, bool LAST>
__global__ __launch_bounds__(kBlock) void cheb_apply0_block_kernel(
    int64_t n2, double b0, const double* __restrict__ r,
    const double* __restrict__ dinv, double* __restrict__ d,
    double* __restrict__ z)
{
  constexpr int SH = PairShift<K>::value;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 rv[kU];
    double dv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      rv[u] = vload<NT>(r, i);
      dv[u] = dinv[i >> SH];
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      f64x2 t;
      t.x = cheb_first<true>(b0, dv[u], rv[u].x);
      t.y = cheb_first<true>(b0, dv[u], rv[u].y);
      if constexpr (!LAST)
        vstore<NT>(d, i, t);
      vstore<NT>(z, i, t);
    }
  }
}

template <bool NT, bool LAST>
__global__ __launch_bounds__(kBlock) void cheb_apply0_rows_kernel(
    int64_t n, int nrhs, double b0, const double* __restrict__ r,
    const double* __restrict__ dinv, double* __restrict__ d,
    double* __restrict__ z)
{
  SPMV_FOR_ROWS(row, n)
  {
    const double dv = dinv[row];
    for (int c = 0; c < nrhs; ++c) {
      const int64_t i = row * nrhs + c;
      const double t = cheb_first<true>(b0, dv, sload<NT>(r + i));
      if constexpr (!LAST)
        sstore<NT>(d + i, t);
      sstore<NT>(z + i, t);
    }
  }
}

// ---- step j >= 1 ---------------------------------------------------------------
// LAST: d is not written
template <int K, bool NT, bool LAST>
__global__ __launch_bounds__(kBlock) void cheb_step_block_kernel(
    int64_t n2, double a, double b, const double* __restrict__ w,
    const double* __restrict__ r, const double* __restrict__ dinv,
    double* __restrict__ d, double* __restrict__ z)
{
  constexpr int SH = PairShift<K>::value;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 wv[kU], rv[kU], ev[kU], zv[kU];
    double dv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      wv[u] = vload<NT>(w, i);
      rv[u] = vload<NT>(r, i);
      dv[u] = dinv[i >> SH];
      ev[u] = vload<NT>(d, i);
      zv[u] = vload<NT>(z, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      const double tx = cheb_corr<true>(b, dv[u], rv[u].x, wv[u].x);
      const double ty = cheb_corr<true>(b, dv[u], rv[u].y, wv[u].y);
      ev[u].x = cheb_next(a, ev[u].x, tx);
      ev[u].y = cheb_next(a, ev[u].y, ty);
      if constexpr (!LAST)
        vstore<NT>(d, i, ev[u]);
      zv[u].x = zv[u].x + ev[u].x;
      zv[u].y = zv[u].y + ev[u].y;
      vstore<NT>(z, i, zv[u]);
    }
  }
}

template <bool NT, bool LAST>
__global__ __launch_bounds__(kBlock) void cheb_step_rows_kernel(
    int64_t n, int nrhs, double a, double b, const double* __restrict__ w,
    const double* __restrict__ r, const double* __restrict__ dinv,
    double* __restrict__ d, double* __restrict__ z)
{
  SPMV_FOR_ROWS(row, n)
  {
    const double dv = dinv[row];
    for (int c = 0; c < nrhs; ++c) {
      const int64_t i = row * nrhs + c;
      const double t
          = cheb_corr<true>(b, dv, sload<NT>(r + i), sload<NT>(w + i));
      const double e = cheb_next(a, sload<NT>(d + i), t);
      if constexpr (!LAST)
        sstore<NT>(d + i, e);
      sstore<NT>(z + i, sload<NT>(z + i) + e);
    }
  }
}

// ---- step 0 of the post-smoother -------------------------------------------------
template <int K, bool NT, bool LAST>
__global__ __launch_bounds__(kBlock) void amg_post0_block_kernel(
    int64_t n2, double b0, const double* __restrict__ w,
    const double* __restrict__ r, const double* __restrict__ dinv,
    double* __restrict__ d, double* __restrict__ z)
{
  constexpr int SH = PairShift<K>::value;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 wv[kU], rv[kU], zv[kU];
    double dv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      wv[u] = vload<NT>(w, i);
      rv[u] = vload<NT>(r, i);
      dv[u] = dinv[i >> SH];
      zv[u] = vload<NT>(z, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      f64x2 t;
      t.x = cheb_corr<true>(b0, dv[u], rv[u].x, wv[u].x);
      t.y = cheb_corr<true>(b0, dv[u], rv[u].y, wv[u].y);
      if constexpr (!LAST)
        vstore<NT>(d, i, t);
      zv[u].x = zv[u].x + t.x;
      zv[u].y = zv[u].y + t.y;
      vstore<NT>(z, i, zv[u]);
    }
  }
}

template <bool NT, bool LAST>
__global__ __launch_bounds__(kBlock) void amg_post0_rows_kernel(
    int64_t n, int nrhs, double b0, const double* __restrict__ w,
    const double* __restrict__ r, const double* __restrict__ dinv,
    double* __restrict__ d, double* __restrict__ z)
{
  SPMV_FOR_ROWS(row, n)
  {
    const double dv = dinv[row];
    for (int c = 0; c < nrhs; ++c) {
      const int64_t i = row * nrhs + c;
      const double t
          = cheb_corr<true>(b0, dv, sload<NT>(r + i), sload<NT>(w + i));
      if constexpr (!LAST)
        sstore<NT>(d + i, t);
      sstore<NT>(z + i, sload<NT>(z + i) + t);
    }
  }
}

// ---- prolong: z streams, the coarse row is gathered ------------------------------
template <int K, bool NT>
__global__ __launch_bounds__(kBlock) void amg_prolong_block_kernel(
    int64_t n2, double scale, const int32_t* __restrict__ agg,
    const double* __restrict__ e, double* __restrict__ z)
{
  constexpr int SH = PairShift<K>::value;
  constexpr int H = K / 2;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 zv[kU], ev[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      zv[u] = vload<NT>(z, i);
      ev[u] = vload<false>(e, (int64_t)agg[i >> SH] * H + (i & (H - 1)));
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      zv[u].x = amg_prolong_elem(zv[u].x, scale, ev[u].x);
      zv[u].y = amg_prolong_elem(zv[u].y, scale, ev[u].y);
      vstore<NT>(z, i, zv[u]);
    }
  }
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void amg_prolong_rows_kernel(
    int64_t n, int nrhs, double scale, const int32_t* __restrict__ agg,
    const double* __restrict__ e, double* __restrict__ z)
{
  SPMV_FOR_ROWS(row, n)
  {
    const double* ec = e + (int64_t)agg[row] * nrhs;
    for (int c = 0; c < nrhs; ++c) {
      const int64_t i = row * nrhs + c;
      sstore<NT>(z + i, amg_prolong_elem(sload<NT>(z + i), scale, ec[c]));
    }
  }
}

// ---- restrict: one lane per (aggregate, column pair) ------------------------------
// The order of a column's sum is the member list's, whatever the launch shape.
template <int K>
__global__ __launch_bounds__(kBlock) void amg_restrict_block_kernel(
    int64_t items, const int32_t* __restrict__ member_ptr,
    const int32_t* __restrict__ member, const double* __restrict__ r,
    const double* __restrict__ w, double* __restrict__ rc)
{
  constexpr int SH = PairShift<K>::value;
  constexpr int H = K / 2;
  SPMV_FOR_ROWS(it, items)
  {
    const int64_t I = it >> SH;
    const int p = (int)(it & (H - 1));
    const int32_t m0 = member_ptr[I], m1 = member_ptr[I + 1];
    f64x2 acc = {0.0, 0.0}; // (an aggregate has a member)
    for (int32_t m = m0; m < m1; ++m) {
      const int64_t i2 = (int64_t)member[m] * H + p;
      const f64x2 rv = vload<false>(r, i2), wv = vload<false>(w, i2);
      const double tx = amg_restrict_term(rv.x, wv.x);
      const double ty = amg_restrict_term(rv.y, wv.y);
      acc.x = m == m0 ? tx : amg_restrict_add(acc.x, tx);
      acc.y = m == m0 ? ty : amg_restrict_add(acc.y, ty);
    }
    vstore<false>(rc, it, acc);
  }
}

// one lane per aggregate, nrhs sums
__global__ __launch_bounds__(kBlock) void amg_restrict_rows_kernel(
    int64_t coarse_rows, int nrhs, const int32_t* __restrict__ member_ptr,
    const int32_t* __restrict__ member, const double* __restrict__ r,
    const double* __restrict__ w, double* __restrict__ rc)
{
  SPMV_FOR_ROWS(I, coarse_rows)
  {
    const int32_t m0 = member_ptr[I], m1 = member_ptr[I + 1];
    double acc[kMaxNrhs];
#pragma unroll
    for (int c = 0; c < kMaxNrhs; ++c)
      acc[c] = 0.0;
    for (int32_t m = m0; m < m1; ++m) {
      const int64_t base = (int64_t)member[m] * nrhs;
#pragma unroll
      for (int c = 0; c < kMaxNrhs; ++c)
        if (c < nrhs) {
          const double t = amg_restrict_term(r[base + c], w[base + c]);
          acc[c] = m == m0 ? t : amg_restrict_add(acc[c], t);
        }
    }
#pragma unroll
    for (int c = 0; c < kMaxNrhs; ++c)
      if (c < nrhs)
        rc[I * nrhs + c] = acc[c];
  }
}

// ---- host side ---------------------------------------------------------------------
bool width_ok(int nrhs) { return nrhs >= 1 && nrhs <= kMaxNrhs; }
bool compiled_width(int nrhs) { return nrhs == 2 || nrhs == 4 || nrhs == 8; }
int rows_grid(const spmv_hip_ctx* ctx, int64_t rows)
{
  return spmv_grid_for(ctx, rows, kBlock);
}

} // namespace

// kernel<K, NT, LAST> for K = nrhs in {2, 4, 8}
#define AMGB_LAUNCH_K(kernel, K, nt, last, grid, st, ...)                      \
  do {                                                                         \
    const dim3 _g(grid), _b(kBlock);                                           \
    switch (((nt) ? 2 : 0) | ((last) ? 1 : 0)) {                               \
    case 0: hipLaunchKernelGGL((kernel<K, false, false>), _g, _b, 0, st, __VA_ARGS__); break; \
    case 1: hipLaunchKernelGGL((kernel<K, false, true>), _g, _b, 0, st, __VA_ARGS__); break;  \
    case 2: hipLaunchKernelGGL((kernel<K, true, false>), _g, _b, 0, st, __VA_ARGS__); break;  \
    default: hipLaunchKernelGGL((kernel<K, true, true>), _g, _b, 0, st, __VA_ARGS__); break;  \
    }                                                                          \
  } while (0)
#define AMGB_LAUNCH_WIDTH(kernel, nrhs, nt, last, grid, st, ...)               \
  do {                                                                         \
    if ((nrhs) == 2)                                                           \
      AMGB_LAUNCH_K(kernel, 2, nt, last, grid, st, __VA_ARGS__);               \
    else if ((nrhs) == 4)                                                      \
      AMGB_LAUNCH_K(kernel, 4, nt, last, grid, st, __VA_ARGS__);               \
    else                                                                       \
      AMGB_LAUNCH_K(kernel, 8, nt, last, grid, st, __VA_ARGS__);               \
  } while (0)
// kernel<NT, LAST>, nrhs at run time
#define AMGB_LAUNCH_ROWS(kernel, nt, last, grid, st, ...)                      \
  do {                                                                         \
    const dim3 _g(grid), _b(kBlock);                                           \
    switch (((nt) ? 2 : 0) | ((last) ? 1 : 0)) {                               \
    case 0: hipLaunchKernelGGL((kernel<false, false>), _g, _b, 0, st, __VA_ARGS__); break; \
    case 1: hipLaunchKernelGGL((kernel<false, true>), _g, _b, 0, st, __VA_ARGS__); break;  \
    case 2: hipLaunchKernelGGL((kernel<true, false>), _g, _b, 0, st, __VA_ARGS__); break;  \
    default: hipLaunchKernelGGL((kernel<true, true>), _g, _b, 0, st, __VA_ARGS__); break;  \
    }                                                                          \
  } while (0)

extern "C" {

int spmv_hip_cheb_apply0_block_f64(spmv_hip_ctx* ctx, int64_t n, int nrhs,
                                   double b0, const double* r, const double* dinv,
                                   double* d, double* z, void* stream)
{
  SPMV_REQUIRE(ctx && n >= 0 && width_ok(nrhs));
  SPMV_REQUIRE(n == 0 || (r && dinv && z));
  SPMV_SET_DEVICE(ctx);
  if (n == 0)
    return SPMV_HIP_OK;
  const int64_t elems = n * nrhs;
  const bool nt = elems >= ctx->blas1_nt_min_elems, last = d == nullptr;
  hipStream_t st = spmv_stream(ctx, stream);
  if (compiled_width(nrhs) && aligned16(r, d, z))
    AMGB_LAUNCH_WIDTH(cheb_apply0_block_kernel, nrhs, nt, last,
                      stream_grid(ctx, elems), st, elems / 2, b0, r, dinv, d, z);
  else
    AMGB_LAUNCH_ROWS(cheb_apply0_rows_kernel, nt, last, rows_grid(ctx, n), st, n,
                     nrhs, b0, r, dinv, d, z);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cheb_step_block_f64(spmv_hip_ctx* ctx, int64_t n, int nrhs, double a,
                                 double b, int last, const double* w,
                                 const double* r, const double* dinv, double* d,
                                 double* z, void* stream)
{
  SPMV_REQUIRE(ctx && n >= 0 && width_ok(nrhs));
  SPMV_REQUIRE(n == 0 || (w && r && dinv && d && z));
  SPMV_SET_DEVICE(ctx);
  if (n == 0)
    return SPMV_HIP_OK;
  const int64_t elems = n * nrhs;
  const bool nt = elems >= ctx->blas1_nt_min_elems;
  hipStream_t st = spmv_stream(ctx, stream);
  if (compiled_width(nrhs) && aligned16(w, r, d, z))
    AMGB_LAUNCH_WIDTH(cheb_step_block_kernel, nrhs, nt, last != 0,
                      stream_grid(ctx, elems), st, elems / 2, a, b, w, r, dinv, d,
                      z);
  else
    AMGB_LAUNCH_ROWS(cheb_step_rows_kernel, nt, last != 0, rows_grid(ctx, n), st,
                     n, nrhs, a, b, w, r, dinv, d, z);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_amg_post0_block_f64(spmv_hip_ctx* ctx, int64_t n, int nrhs, double b0,
                                 const double* w, const double* r,
                                 const double* dinv, double* d, double* z,
                                 void* stream)
{
  SPMV_REQUIRE(ctx && n >= 0 && width_ok(nrhs));
  SPMV_REQUIRE(n == 0 || (w && r && dinv && z));
  SPMV_SET_DEVICE(ctx);
  if (n == 0)
    return SPMV_HIP_OK;
  const int64_t elems = n * nrhs;
  const bool nt = elems >= ctx->blas1_nt_min_elems, last = d == nullptr;
  hipStream_t st = spmv_stream(ctx, stream);
  if (compiled_width(nrhs) && aligned16(w, r, d, z))
    AMGB_LAUNCH_WIDTH(amg_post0_block_kernel, nrhs, nt, last,
                      stream_grid(ctx, elems), st, elems / 2, b0, w, r, dinv, d,
                      z);
  else
    AMGB_LAUNCH_ROWS(amg_post0_rows_kernel, nt, last, rows_grid(ctx, n), st, n,
                     nrhs, b0, w, r, dinv, d, z);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_amg_restrict_block_f64(spmv_hip_ctx* ctx,
                                    const spmv_hip_amg_plan* plan, int nrhs,
                                    const double* r, const double* w, double* rc,
                                    void* stream)
{
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx && plan->coarse_rows > 0);
  SPMV_REQUIRE(width_ok(nrhs) && r && w && rc);
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  const int64_t nc = plan->coarse_rows;
  const dim3 blk(kBlock);
  if (compiled_width(nrhs) && aligned16(r, w, rc)) {
    const int64_t items = nc * (nrhs / 2);
    const dim3 g(rows_grid(ctx, items));
    if (nrhs == 2)
      hipLaunchKernelGGL(amg_restrict_block_kernel<2>, g, blk, 0, st, items,
                         plan->member_ptr, plan->member, r, w, rc);
    else if (nrhs == 4)
      hipLaunchKernelGGL(amg_restrict_block_kernel<4>, g, blk, 0, st, items,
                         plan->member_ptr, plan->member, r, w, rc);
    else
      hipLaunchKernelGGL(amg_restrict_block_kernel<8>, g, blk, 0, st, items,
                         plan->member_ptr, plan->member, r, w, rc);
  } else {
    hipLaunchKernelGGL(amg_restrict_rows_kernel, dim3(rows_grid(ctx, nc)), blk, 0,
                       st, nc, nrhs, plan->member_ptr, plan->member, r, w, rc);
  }
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_amg_prolong_block_f64(spmv_hip_ctx* ctx,
                                   const spmv_hip_amg_plan* plan, int nrhs,
                                   double scale, const double* e, double* z,
                                   void* stream)
{
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx && plan->coarse_rows > 0);
  SPMV_REQUIRE(width_ok(nrhs) && e && z);
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  const int64_t n = plan->fine_rows, elems = n * nrhs;
  const bool nt = elems >= ctx->blas1_nt_min_elems;
  const dim3 blk(kBlock);
  if (compiled_width(nrhs) && aligned16(e, z)) {
    const dim3 g(stream_grid(ctx, elems));
#define AMGB_PROLONG(K)                                                        \
  do {                                                                         \
    if (nt)                                                                    \
      hipLaunchKernelGGL((amg_prolong_block_kernel<K, true>), g, blk, 0, st,   \
                         elems / 2, scale, plan->agg, e, z);                   \
    else                                                                       \
      hipLaunchKernelGGL((amg_prolong_block_kernel<K, false>), g, blk, 0, st,  \
                         elems / 2, scale, plan->agg, e, z);                   \
  } while (0)
    if (nrhs == 2)
      AMGB_PROLONG(2);
    else if (nrhs == 4)
      AMGB_PROLONG(4);
    else
      AMGB_PROLONG(8);
#undef AMGB_PROLONG
  } else {
    const dim3 g(rows_grid(ctx, n));
    if (nt)
      hipLaunchKernelGGL(amg_prolong_rows_kernel<true>, g, blk, 0, st, n, nrhs,
                         scale, plan->agg, e, z);
    else
      hipLaunchKernelGGL(amg_prolong_rows_kernel<false>, g, blk, 0, st, n, nrhs,
                         scale, plan->agg, e, z);
  }
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
