// BLAS-1 kernels of spmv::cg_block (gfx950): the reducer-kernel CG sequence of
// blas1.hip for a block of nrhs INTERLEAVED vectors -- element (i, c) at
// V[i * nrhs + c], the layout of Matrix::mult_block.  nrhs independent
// recurrences (spmv/cg.cpp:21-98 once per column) run in lockstep:
//
//   init       R = P = B ; X = 0 ; partials of r.r                (cg.cpp:39-47)
//   dot        partials of p.Ap                                   (cg.cpp:63)
//   reduce_pAp partials -> pAp[k][c] ; raises done[c], all_done   (cg.cpp:64,80)
//   update_r   r -= alpha_c Ap ; partials of r.r                  (cg.cpp:66-73)
//   reduce_rr  partials -> rr[k][c]                               (cg.cpp:74)
//   update_xp  x += alpha_c p ; stop test ; p = beta_c p + r      (cg.cpp:69-85)
//
// Every column has its own alpha, beta and stopping test.  A column that has
// stopped is frozen: no kernel changes its x, r or p and its scalars are not
// extended.  Partials are [len][nrhs]; the reducers add them in index order
// per column, so the bits of column c depend on A, on column c of B, on nrhs
// and on c -- not on what the other columns hold or on when they stop.
//
// nrhs = 2, 4, 8 (template K): the streaming shape of blas1_stream.h -- a
// persistent grid walks units of kU x kBlock 16-byte elements.  The unit
// stride is a multiple of K, so a lane sees the same column pair
// (2 (tid % (K/2)), +1) in every step and keeps two accumulators and two
// alphas / betas in registers.
//   Interleaved stores: a 16-byte element holds two columns.  When one of
//   them has stopped, the lane STORES BACK THE VALUE IT LOADED for that column
//   in this very kernel (nobody else writes the element); when both have
//   stopped, the lane neither loads nor stores.
// Other nrhs in 1..8: one kernel family with nrhs at run time, one thread per
// row and scalar accesses; a stopped column is left out of loads and stores.
// init always runs in that form (one pass per solve; B needs no alignment).
//
// Built with -ffp-contract=off like blas1.hip: every element sees the
// multiplies and adds of the single-vector kernels.  The block sums, the
// one-thread-per-row frame and the launch macros are blas1_block.h's, shared
// with blas1_pcg_block.hip.
#include "common.h"
#include "blas1_block.h"
#include "solver_ws.h"

#include <climits>
#include <cmath>

struct spmv_hip_cgb_ws {
  spmv_hip_ctx* ctx = nullptr;
  int kmax = 0;
  int nrhs = 0;
  SolverArrays own;
  double* rr = nullptr;       // [kmax + 1][nrhs]
  double* pAp = nullptr;      // [kmax + 1][nrhs]
  double* partials = nullptr; // [ctx->dot_blocks][nrhs]
  CgbState* st = nullptr;
};

namespace
{

// what iteration k does to one column (cg.cpp:66,76-80)
struct ColStep {
  double alpha = 0.0, beta = 0.0;
  int mode = 0; // 0: stopped, frozen; 1: meets the tolerance now (x only); 2: goes on
};

__device__ __forceinline__ ColStep col_step(const CgbState* st,
                                            const double* rr, const double* pAp,
                                            int k, int nrhs, int c)
{
  ColStep s;
  if (st->done[c])
    return s;
  const double rnorm0 = sqrt(rr[c]);
  const double rnorm_old = sqrt(rr[(k - 1) * nrhs + c]);
  const double rnorm_new = sqrt(rr[k * nrhs + c]);                  // :76
  s.alpha = (rnorm_old * rnorm_old) / pAp[k * nrhs + c];            // :66
  s.beta = (rnorm_new * rnorm_new) / (rnorm_old * rnorm_old);       // :77
  s.mode = (rnorm_new / rnorm0 < st->rtol) ? 1 : 2;                 // :80
  return s;
}

// -alpha of iteration k for one column that has not stopped (cg.cpp:66)
__device__ __forceinline__ double col_nalpha(const double* rr, const double* pAp,
                                             int k, int nrhs, int c)
{
  const double rnorm_old = sqrt(rr[(k - 1) * nrhs + c]);
  const double alpha = (rnorm_old * rnorm_old) / pAp[k * nrhs + c];
  return -alpha;
}

template <int K, bool NT>
__global__ __launch_bounds__(kBlock) void cgb_dot_kernel(
    int64_t n2, const CgbState* __restrict__ st, const double* __restrict__ x,
    const double* __restrict__ y, double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64][K];
  if (st->all_done)
    return;
  const int c0 = 2 * (threadIdx.x % (K / 2));
  const bool on0 = !st->done[c0], on1 = !st->done[c0 + 1];
  double acc0 = 0.0, acc1 = 0.0;
  if (on0 || on1) {
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
        if (on0)
          acc0 += a[u].x * b[u].x;
        if (on1)
          acc1 += a[u].y * b[u].y;
      }
    }
  }
  block_sum_pairs<K>(acc0, acc1, s_red, partials + (int64_t)blockIdx.x * K);
  clear_partials_tail(partials, len, K);
}

// r += (-alpha_c) Ap (cg.cpp:66,70) ; partials of r.r (:73)
template <int K, bool NT>
__global__ __launch_bounds__(kBlock) void cgb_update_r_kernel(
    int64_t n2, int k, const double* __restrict__ rr,
    const double* __restrict__ pAp, const CgbState* __restrict__ st,
    const double* __restrict__ Ap, double* __restrict__ r,
    double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64][K];
  if (st->all_done)
    return;
  const int c0 = 2 * (threadIdx.x % (K / 2));
  const bool on0 = !st->done[c0], on1 = !st->done[c0 + 1];
  const double na0 = on0 ? col_nalpha(rr, pAp, k, K, c0) : 0.0;
  const double na1 = on1 ? col_nalpha(rr, pAp, k, K, c0 + 1) : 0.0;
  double acc0 = 0.0, acc1 = 0.0;
  if (on0 || on1) {
    SPMV_FOR_UNITS(n2)
    {
      f64x2 av[kU], rv[kU];
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        av[u] = vload<NT>(Ap, i);
        rv[u] = vload<NT>(r, i);
      }
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        if (on0) {
          rv[u].x += na0 * av[u].x;
          acc0 += rv[u].x * rv[u].x;
        }
        if (on1) {
          rv[u].y += na1 * av[u].y;
          acc1 += rv[u].y * rv[u].y;
        }
        vstore<NT>(r, i, rv[u]); // a stopped column: the value just loaded
      }
    }
  }
  block_sum_pairs<K>(acc0, acc1, s_red, partials + (int64_t)blockIdx.x * K);
  clear_partials_tail(partials, len, K);
}

// x += alpha_c p (cg.cpp:69) ; stop test (:80) ; p = beta_c p + r (:84-85)
template <int K, bool NT>
__global__ __launch_bounds__(kBlock) void cgb_update_xp_kernel(
    int64_t n2, int k, const double* __restrict__ rr,
    const double* __restrict__ pAp, const CgbState* __restrict__ st,
    const double* __restrict__ r, double* __restrict__ x,
    double* __restrict__ p)
{
  if (st->all_done)
    return;
  const int c0 = 2 * (threadIdx.x % (K / 2));
  const ColStep s0 = col_step(st, rr, pAp, k, K, c0);
  const ColStep s1 = col_step(st, rr, pAp, k, K, c0 + 1);
  if (s0.mode == 0 && s1.mode == 0)
    return;
  // a column that meets the tolerance now takes its x update and keeps its p
  const bool any_p = s0.mode == 2 || s1.mode == 2;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 pv[kU], xv[kU], rv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      pv[u] = vload<NT>(p, i);
      xv[u] = vload<NT>(x, i);
      if (any_p)
        rv[u] = vload<NT>(r, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      if (s0.mode)
        xv[u].x += s0.alpha * pv[u].x;
      if (s1.mode)
        xv[u].y += s1.alpha * pv[u].y;
      vstore<NT>(x, i, xv[u]); // a stopped column: the value just loaded
      if (any_p) {
        if (s0.mode == 2) {
          pv[u].x = s0.beta * pv[u].x;
          pv[u].x += rv[u].x;
        }
        if (s1.mode == 2) {
          pv[u].y = s1.beta * pv[u].y;
          pv[u].y += rv[u].y;
        }
        vstore<NT>(p, i, pv[u]); // likewise for a column whose p stays
      }
    }
  }
}

// ---- nrhs at run time (1..8): one thread per row -----------------------------
// CG start (cg.cpp:39-50) in one pass over B: R = P = B, X = 0 (defined here,
// as cg_init_kernel does) and the partials of r.r per column
template <bool NT>
__global__ __launch_bounds__(kBlock) void cgb_init_kernel(
    int64_t M, int nrhs, const double* __restrict__ b, double* __restrict__ r,
    double* __restrict__ p, double* __restrict__ x,
    double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64];
  double acc[SPMV_CGB_MAX] = {};
  SPMV_FOR_ROWS(row, M)
  {
    SPMV_FOR_COLS(c, nrhs)
    {
      const int64_t i = row * nrhs + c;
      const double v = b[i];
      sstore<NT>(r + i, v);
      sstore<NT>(p + i, v);
      sstore<NT>(x + i, 0.0);
      acc[c] += v * v;
    }
  }
  rows_epilogue(acc, nrhs, s_red, partials, len);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void cgb_dot_rows_kernel(
    int64_t M, int nrhs, const CgbState* __restrict__ st,
    const double* __restrict__ x, const double* __restrict__ y,
    double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (st->all_done)
    return;
  const int dm = done_mask(st, nrhs);
  double acc[SPMV_CGB_MAX] = {};
  SPMV_FOR_ROWS(row, M)
  {
    SPMV_FOR_COLS(c, nrhs)
    {
      if (!((dm >> c) & 1)) {
        const int64_t i = row * nrhs + c;
        acc[c] += sload<NT>(x + i) * sload<NT>(y + i);
      }
    }
  }
  rows_epilogue(acc, nrhs, s_red, partials, len);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void cgb_update_r_rows_kernel(
    int64_t M, int nrhs, int k, const double* __restrict__ rr,
    const double* __restrict__ pAp, const CgbState* __restrict__ st,
    const double* __restrict__ Ap, double* __restrict__ r,
    double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (st->all_done)
    return;
  const int dm = done_mask(st, nrhs);
  double na[SPMV_CGB_MAX] = {};
  SPMV_FOR_COLS(c, nrhs)
  {
    if (!((dm >> c) & 1))
      na[c] = col_nalpha(rr, pAp, k, nrhs, c);
  }
  double acc[SPMV_CGB_MAX] = {};
  SPMV_FOR_ROWS(row, M)
  {
    SPMV_FOR_COLS(c, nrhs)
    {
      if (!((dm >> c) & 1)) { // a stopped column is neither read nor written
        const int64_t i = row * nrhs + c;
        double rv = sload<NT>(r + i);
        rv += na[c] * sload<NT>(Ap + i);
        sstore<NT>(r + i, rv);
        acc[c] += rv * rv;
      }
    }
  }
  rows_epilogue(acc, nrhs, s_red, partials, len);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void cgb_update_xp_rows_kernel(
    int64_t M, int nrhs, int k, const double* __restrict__ rr,
    const double* __restrict__ pAp, const CgbState* __restrict__ st,
    const double* __restrict__ r, double* __restrict__ x,
    double* __restrict__ p)
{
  if (st->all_done)
    return;
  ColStep s[SPMV_CGB_MAX];
  SPMV_FOR_COLS(c, nrhs) { s[c] = col_step(st, rr, pAp, k, nrhs, c); }
  SPMV_FOR_ROWS(row, M)
  {
    SPMV_FOR_COLS(c, nrhs)
    {
      if (s[c].mode) { // a stopped column is neither read nor written
        const int64_t i = row * nrhs + c;
        double pv = sload<NT>(p + i);
        double xv = sload<NT>(x + i);
        xv += s[c].alpha * pv;
        sstore<NT>(x + i, xv);
        if (s[c].mode == 2) {
          pv = s[c].beta * pv;
          pv += sload<NT>(r + i);
          sstore<NT>(p + i, pv);
        }
      }
    }
  }
}

// ---- reducers (one workgroup) -------------------------------------------------
// Reduces the p.Ap partials of iteration k.  Being the first single-workgroup
// kernel after update_xp of iteration k-1, it also raises done[c] for every
// column whose rr[k-1] met the tolerance (cg.cpp:80-81), and at k = 1 for a
// column with r_0 . r_0 == 0 (stopped at k = 0 with x = 0); all_done once
// every column has stopped.  The pAp slot of a stopped column keeps the zero
// of the reset, on every rank, so the all-reduce that follows leaves it zero.
__global__ __launch_bounds__(kBlock) void cgb_reduce_pAp_kernel(
    const double* __restrict__ partials, int len, int k, int nrhs,
    const double* __restrict__ rr, double* __restrict__ pAp,
    CgbState* __restrict__ st)
{
  __shared__ double s_red[kBlock / 64];
  if (st->all_done)
    return;
  const int dm = done_mask(st, nrhs); // read by every thread before any write
  __syncthreads();
  int stopped = 0;
  for (int c = 0; c < nrhs; ++c) { // every branch is uniform in the workgroup
    bool d = (dm >> c) & 1;
    if (!d) {
      const double rr0 = rr[c];
      if (k == 1)
        d = rr0 == 0.0;
      else
        d = sqrt(rr[(k - 1) * nrhs + c]) / sqrt(rr0) < st->rtol;
      if (d && threadIdx.x == 0) {
        st->kstop[c] = k - 1;
        st->done[c] = 1;
      }
    }
    if (d) {
      ++stopped;
      continue;
    }
    const double s = reduce_column(partials, len, nrhs, c, s_red);
    if (threadIdx.x == 0)
      pAp[k * nrhs + c] = s;
  }
  if (stopped == nrhs && threadIdx.x == 0)
    st->all_done = 1;
}

__global__ __launch_bounds__(kBlock) void cgb_reduce_rr_kernel(
    const double* __restrict__ partials, int len, int k, int nrhs,
    double* __restrict__ rr, const CgbState* __restrict__ st)
{
  __shared__ double s_red[kBlock / 64];
  if (st->all_done)
    return;
  const int dm = done_mask(st, nrhs);
  for (int c = 0; c < nrhs; ++c) {
    if ((dm >> c) & 1)
      continue; // its history ends at kstop[c]
    const double s = reduce_column(partials, len, nrhs, c, s_red);
    if (threadIdx.x == 0)
      rr[k * nrhs + c] = s;
  }
}

__global__ void cgb_reset_kernel(CgbState* st, double rtol, double* rr,
                                 double* pAp, int count)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    st->rtol = rtol;
    st->all_done = 0;
  }
  if (i < SPMV_CGB_MAX) {
    st->done[i] = 0;
    st->kstop[i] = -1;
  }
  if (i < count) {
    rr[i] = 0.0;
    pAp[i] = 0.0;
  }
}

} // namespace

extern "C" {

int spmv_hip_cgb_ws_create(spmv_hip_ctx* ctx, int kmax, int nrhs,
                           spmv_hip_cgb_ws** out)
{
  SPMV_REQUIRE(ctx && out && nrhs_ok(nrhs));
  SPMV_REQUIRE(kmax >= 0 && kmax < INT_MAX / (2 * SPMV_CGB_MAX));
  return solver_ws_create(ctx, kmax, out, [&](spmv_hip_cgb_ws& w) {
    w.nrhs = nrhs;
    const size_t hist = (size_t)(kmax + 1) * nrhs;
    w.own.alloc(w.rr, hist);
    w.own.alloc(w.pAp, hist);
    w.own.alloc(w.partials, (size_t)ctx->dot_blocks * nrhs);
    w.own.alloc(w.st, 1);
  });
}

int spmv_hip_cgb_ws_destroy(spmv_hip_cgb_ws* ws)
{
  return solver_ws_destroy(ws);
}

int spmv_hip_cgb_ws_reset(spmv_hip_cgb_ws* ws, double rtol, void* stream)
{
  SPMV_REQUIRE(ws);
  SPMV_SET_DEVICE(ws->ctx);
  const int count = (ws->kmax + 1) * ws->nrhs;
  hipLaunchKernelGGL(cgb_reset_kernel, ws_reset_grid(count), dim3(kBlock), 0,
                     spmv_stream(ws->ctx, stream), ws->st, rtol, ws->rr,
                     ws->pAp, count);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cgb_ws_capacity(const spmv_hip_cgb_ws* ws, int* kmax, int* nrhs)
{
  SPMV_REQUIRE(ws && kmax && nrhs);
  *kmax = ws->kmax;
  *nrhs = ws->nrhs;
  return SPMV_HIP_OK;
}

int spmv_hip_cgb_ws_rr(spmv_hip_cgb_ws* ws, int k, double** slot)
{
  SPMV_REQUIRE(ws && slot && k >= 0 && k <= ws->kmax);
  *slot = ws->rr + (size_t)k * ws->nrhs;
  return SPMV_HIP_OK;
}

int spmv_hip_cgb_ws_pAp(spmv_hip_cgb_ws* ws, int k, double** slot)
{
  SPMV_REQUIRE(ws && slot && k >= 0 && k <= ws->kmax);
  *slot = ws->pAp + (size_t)k * ws->nrhs;
  return SPMV_HIP_OK;
}

int spmv_hip_cgb_ws_partials(spmv_hip_cgb_ws* ws, double** partials)
{
  SPMV_REQUIRE(ws && partials);
  *partials = ws->partials;
  return SPMV_HIP_OK;
}

int spmv_hip_cgb_ws_done_flag(spmv_hip_cgb_ws* ws, const int32_t** all_done)
{
  SPMV_REQUIRE(ws && all_done);
  *all_done = &ws->st->all_done;
  return SPMV_HIP_OK;
}

int spmv_hip_cgb_ws_read_async(spmv_hip_cgb_ws* ws, int32_t* host_state,
                               size_t host_state_len, double* host_rr,
                               size_t host_rr_len, void* stream)
{
  SPMV_REQUIRE(ws);
  // a short state buffer gets nothing at all either
  SPMV_REQUIRE(!host_state || host_state_len >= SPMV_HIP_CGB_STATE_WORDS);
  return ws_read_async(ws->ctx, stream, host_state, &ws->st->all_done,
                       SPMV_HIP_CGB_STATE_WORDS, host_rr, host_rr_len, ws->rr,
                       ((size_t)ws->kmax + 1) * (size_t)ws->nrhs);
}

int spmv_hip_cgb_init_f64(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int64_t M,
                          const double* B, double* R, double* P, double* X,
                          void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && M >= 0);
  SPMV_REQUIRE(M == 0 || (B && R && P && X));
  SPMV_SET_DEVICE(ctx);
  const int nrhs = ws->nrhs;
  const bool nt = M * nrhs >= ctx->blas1_nt_min_elems;
  SPMV_CGB_LAUNCH_NT(nt, cgb_init_kernel, rows_grid(ctx, M),
                     spmv_stream(ctx, stream), M, nrhs, B, R, P, X,
                     ws->partials, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cgb_dot_f64(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int64_t M,
                         const double* P, const double* AP, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && M >= 0);
  SPMV_REQUIRE(M == 0 || (P && AP));
  const int nrhs = ws->nrhs;
  SPMV_REQUIRE(!native_width(nrhs) || aligned16(P, AP));
  SPMV_SET_DEVICE(ctx);
  const bool nt = M * nrhs >= ctx->blas1_nt_min_elems;
  hipStream_t st = spmv_stream(ctx, stream);
  if (native_width(nrhs)) {
    const int64_t n2 = M * nrhs / 2;
    SPMV_CGB_LAUNCH_WIDTH(nrhs, nt, cgb_dot_kernel,
                          stream_grid_capped(ctx, M * nrhs), st, n2, ws->st, P,
                          AP, ws->partials, ctx->dot_blocks);
  } else {
    SPMV_CGB_LAUNCH_NT(nt, cgb_dot_rows_kernel, rows_grid(ctx, M), st, M, nrhs,
                       ws->st, P, AP, ws->partials, ctx->dot_blocks);
  }
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cgb_reduce_pAp(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int k,
                            void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && k >= 1 && k <= ws->kmax);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(cgb_reduce_pAp_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->partials, ctx->dot_blocks, k,
                     ws->nrhs, ws->rr, ws->pAp, ws->st);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cgb_reduce_rr(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int k,
                           void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && k >= 0 && k <= ws->kmax);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(cgb_reduce_rr_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->partials, ctx->dot_blocks, k,
                     ws->nrhs, ws->rr, ws->st);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cgb_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int k,
                              int64_t M, const double* AP, double* R,
                              void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && k >= 1 && k <= ws->kmax && M >= 0);
  SPMV_REQUIRE(M == 0 || (AP && R));
  const int nrhs = ws->nrhs;
  SPMV_REQUIRE(!native_width(nrhs) || aligned16(AP, R));
  SPMV_SET_DEVICE(ctx);
  const bool nt = M * nrhs >= ctx->blas1_nt_min_elems;
  hipStream_t st = spmv_stream(ctx, stream);
  if (native_width(nrhs)) {
    const int64_t n2 = M * nrhs / 2;
    SPMV_CGB_LAUNCH_WIDTH(nrhs, nt, cgb_update_r_kernel,
                          stream_grid_capped(ctx, M * nrhs), st, n2, k, ws->rr,
                          ws->pAp, ws->st, AP, R, ws->partials, ctx->dot_blocks);
  } else {
    SPMV_CGB_LAUNCH_NT(nt, cgb_update_r_rows_kernel, rows_grid(ctx, M), st, M,
                       nrhs, k, ws->rr, ws->pAp, ws->st, AP, R, ws->partials,
                       ctx->dot_blocks);
  }
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cgb_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int k,
                               int64_t M, const double* R, double* X, double* P,
                               void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && k >= 1 && k <= ws->kmax && M >= 0);
  SPMV_REQUIRE(M == 0 || (R && X && P));
  const int nrhs = ws->nrhs;
  SPMV_REQUIRE(!native_width(nrhs) || aligned16(R, X, P));
  SPMV_SET_DEVICE(ctx);
  const bool nt = M * nrhs >= ctx->blas1_nt_min_elems;
  hipStream_t st = spmv_stream(ctx, stream);
  if (native_width(nrhs)) {
    const int64_t n2 = M * nrhs / 2;
    SPMV_CGB_LAUNCH_WIDTH(nrhs, nt, cgb_update_xp_kernel,
                          stream_grid_capped(ctx, M * nrhs), st, n2, k, ws->rr,
                          ws->pAp, ws->st, R, X, P);
  } else {
    SPMV_CGB_LAUNCH_NT(nt, cgb_update_xp_rows_kernel, rows_grid(ctx, M), st, M,
                       nrhs, k, ws->rr, ws->pAp, ws->st, R, X, P);
  }
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
