// BLAS-1 kernels of spmv::pcg_block (gfx950): pcg_sgs's recurrence with a
// stored Z = M^-1 R for a block of nrhs INTERLEAVED vectors -- element (i, c)
// at V[i * nrhs + c], the layout of Matrix::mult_block -- nrhs independent
// recurrences in lockstep, the way blas1_block.hip runs cg():
//
//   init         R = B ; X = 0 ; partials of r.r
//   dot          partials of p.Ap ; with Z = M^-1 R stored: partials of r.z
//   dot (dinv)   Z = dinv * R (row i's dinv[i] for all its columns) ; partials
//                of r.z, in one pass
//   reduce_pAp   partials -> pAp[k][c] ; raises done[c], all_done
//   update_r     r -= alpha_c Ap ; partials of r.r ; alpha_c = rz[k-1][c] / pAp[k][c]
//   reduce_rz_rr partials -> {rz[k][0:nrhs], rr[k][0:nrhs]}, contiguous: one
//                all-reduce of 2 nrhs doubles
//   update_xp    x += alpha_c p ; stop test ; p = beta_c p + z
//                beta_c = rz[k][c] / rz[k-1][c] ; stop: sqrt(rr[k][c]) / sqrt(rr[0][c]) < rtol
//
// The column rules are cg_block's: every column has its own alpha, beta and
// stopping test; a column that has stopped is frozen (no kernel changes its x,
// r or p, its scalars are not extended); a column with r_0 . r_0 == 0 stops at
// k = 0 with x = 0.  Z of a stopped column may still be written (the sweeps and
// the dinv form do): nothing reads it.  Partials are [len][nrhs], added in index
// order per column, so the bits of column c depend on A, M, column c of B, nrhs
// and c only.
//
// nrhs = 2, 4, 8 (template K): the streaming shape of blas1_stream.h with
// cg_block's store-back rule -- a 16-byte element holds two columns; when one
// of them has stopped the lane stores back the value it loaded for it, when
// both have stopped it neither loads nor stores.  Other nrhs in 1..8: one
// thread per row, scalar accesses, a stopped column left out.  init always
// runs in that form (B needs no alignment).
//
// Built with -ffp-contract=off: every element sees the multiplies and adds of
// the single-vector kernels of pcg_sgs (blas1_cheb.hip).
#include "common.h"
#include "blas1_block.h"

#include <climits>
#include <cmath>

namespace
{

// the scalars of column c: zr is [k][2][nrhs]
__device__ __forceinline__ double rz_at(const double* zr, int k, int nrhs, int c)
{
  return zr[(2 * k) * nrhs + c];
}
__device__ __forceinline__ double rr_at(const double* zr, int k, int nrhs, int c)
{
  return zr[(2 * k + 1) * nrhs + c];
}

// what iteration k does to one column
struct ColStep {
  double alpha = 0.0, beta = 0.0;
  int mode = 0; // 0: stopped, frozen; 1: meets the tolerance now (x only); 2: goes on
};

__device__ __forceinline__ ColStep col_step(const CgbState* st,
                                            const double* zr, const double* pAp,
                                            int k, int nrhs, int c)
{
  ColStep s;
  if (st->done[c])
    return s;
  const double rz_old = rz_at(zr, k - 1, nrhs, c);
  s.alpha = rz_old / pAp[k * nrhs + c];
  s.beta = rz_at(zr, k, nrhs, c) / rz_old;
  s.mode = (sqrt(rr_at(zr, k, nrhs, c)) / sqrt(rr_at(zr, 0, nrhs, c)) < st->rtol)
               ? 1
               : 2;
  return s;
}

// -alpha of iteration k for one column that has not stopped
__device__ __forceinline__ double col_nalpha(const double* zr, const double* pAp,
                                             int k, int nrhs, int c)
{
  return -(rz_at(zr, k - 1, nrhs, c) / pAp[k * nrhs + c]);
}

// ---- K = 2, 4, 8 ------------------------------------------------------------
// partials of x . y per column.  DINV: y = dinv * x is formed and stored first
// (x = R, y = Z): 16-byte element i holds the columns c0, c0 + 1 of row i / (K/2)
template <int K, bool NT, bool DINV>
__global__ __launch_bounds__(kBlock) void pcgb_dot_kernel(
    int64_t n2, const CgbState* __restrict__ st, const double* __restrict__ dinv,
    const double* __restrict__ x, double* __restrict__ y,
    double* __restrict__ partials, int len)
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
      double d[kU];
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        a[u] = vload<NT>(x, i);
        if constexpr (DINV)
          d[u] = dinv[i / (K / 2)];
        else
          b[u] = vload<NT>(y, i);
      }
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        if constexpr (DINV) {
          b[u].x = d[u] * a[u].x;
          b[u].y = d[u] * a[u].y;
          vstore<NT>(y, i, b[u]); // (a stopped column's z is not read)
        }
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

// r += (-alpha_c) Ap ; partials of r.r
template <int K, bool NT>
__global__ __launch_bounds__(kBlock) void pcgb_update_r_kernel(
    int64_t n2, int k, const double* __restrict__ zr,
    const double* __restrict__ pAp, const CgbState* __restrict__ st,
    const double* __restrict__ Ap, double* __restrict__ r,
    double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64][K];
  if (st->all_done)
    return;
  const int c0 = 2 * (threadIdx.x % (K / 2));
  const bool on0 = !st->done[c0], on1 = !st->done[c0 + 1];
  const double na0 = on0 ? col_nalpha(zr, pAp, k, K, c0) : 0.0;
  const double na1 = on1 ? col_nalpha(zr, pAp, k, K, c0 + 1) : 0.0;
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

// x += alpha_c p ; stop test ; p = beta_c p + z
template <int K, bool NT>
__global__ __launch_bounds__(kBlock) void pcgb_update_xp_kernel(
    int64_t n2, int k, const double* __restrict__ zr,
    const double* __restrict__ pAp, const CgbState* __restrict__ st,
    const double* __restrict__ z, double* __restrict__ x,
    double* __restrict__ p)
{
  if (st->all_done)
    return;
  const int c0 = 2 * (threadIdx.x % (K / 2));
  const ColStep s0 = col_step(st, zr, pAp, k, K, c0);
  const ColStep s1 = col_step(st, zr, pAp, k, K, c0 + 1);
  if (s0.mode == 0 && s1.mode == 0)
    return;
  // a column that meets the tolerance now takes its x update and keeps its p
  const bool any_p = s0.mode == 2 || s1.mode == 2;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 pv[kU], xv[kU], zv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      pv[u] = vload<NT>(p, i);
      xv[u] = vload<NT>(x, i);
      if (any_p)
        zv[u] = vload<NT>(z, i);
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
          pv[u].x += zv[u].x;
        }
        if (s1.mode == 2) {
          pv[u].y = s1.beta * pv[u].y;
          pv[u].y += zv[u].y;
        }
        vstore<NT>(p, i, pv[u]); // likewise for a column whose p stays
      }
    }
  }
}

// ---- nrhs at run time (1..8): one thread per row -----------------------------
// start in one pass over B: R = B, X = 0 and the partials of r.r per column
template <bool NT>
__global__ __launch_bounds__(kBlock) void pcgb_init_kernel(
    int64_t M, int nrhs, const double* __restrict__ b, double* __restrict__ r,
    double* __restrict__ x, double* __restrict__ partials, int len)
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
      sstore<NT>(x + i, 0.0);
      acc[c] += v * v;
    }
  }
  rows_epilogue(acc, nrhs, s_red, partials, len);
}

template <bool NT, bool DINV>
__global__ __launch_bounds__(kBlock) void pcgb_dot_rows_kernel(
    int64_t M, int nrhs, const CgbState* __restrict__ st,
    const double* __restrict__ dinv, const double* __restrict__ x,
    double* __restrict__ y, double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (st->all_done)
    return;
  const int dm = done_mask(st, nrhs);
  double acc[SPMV_CGB_MAX] = {};
  SPMV_FOR_ROWS(row, M)
  {
    double d = 0.0;
    if constexpr (DINV)
      d = dinv[row];
    SPMV_FOR_COLS(c, nrhs)
    {
      if (!((dm >> c) & 1)) {
        const int64_t i = row * nrhs + c;
        const double xv = sload<NT>(x + i);
        double yv;
        if constexpr (DINV) {
          yv = d * xv;
          sstore<NT>(y + i, yv);
        } else {
          yv = sload<NT>(y + i);
        }
        acc[c] += xv * yv;
      }
    }
  }
  rows_epilogue(acc, nrhs, s_red, partials, len);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void pcgb_update_r_rows_kernel(
    int64_t M, int nrhs, int k, const double* __restrict__ zr,
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
      na[c] = col_nalpha(zr, pAp, k, nrhs, c);
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
__global__ __launch_bounds__(kBlock) void pcgb_update_xp_rows_kernel(
    int64_t M, int nrhs, int k, const double* __restrict__ zr,
    const double* __restrict__ pAp, const CgbState* __restrict__ st,
    const double* __restrict__ z, double* __restrict__ x,
    double* __restrict__ p)
{
  if (st->all_done)
    return;
  ColStep s[SPMV_CGB_MAX];
  SPMV_FOR_COLS(c, nrhs) { s[c] = col_step(st, zr, pAp, k, nrhs, c); }
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
          pv += sload<NT>(z + i);
          sstore<NT>(p + i, pv);
        }
      }
    }
  }
}

// ---- reducers (one workgroup) -------------------------------------------------
// Reduces the p.Ap partials of iteration k.  Being the first single-workgroup
// kernel after update_xp of iteration k-1, it also raises done[c] for every
// column whose rr[k-1] met the tolerance, and at k = 1 for a column with
// r_0 . r_0 == 0 (stopped at k = 0 with x = 0); all_done once every column has
// stopped.  The slots of a stopped column keep the zero of the reset, on every
// rank, so the all-reduces that follow leave them zero.
__global__ __launch_bounds__(kBlock) void pcgb_reduce_pAp_kernel(
    const double* __restrict__ partials, int len, int k, int nrhs,
    const double* __restrict__ zr, double* __restrict__ pAp,
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
      const double rr0 = rr_at(zr, 0, nrhs, c);
      if (k == 1)
        d = rr0 == 0.0;
      else
        d = sqrt(rr_at(zr, k - 1, nrhs, c)) / sqrt(rr0) < st->rtol;
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

// partials of r.z and r.r -> rz[k][c], rr[k][c]
__global__ __launch_bounds__(kBlock) void pcgb_reduce_rz_rr_kernel(
    const double* __restrict__ partials_rz,
    const double* __restrict__ partials_rr, int len, int k, int nrhs,
    double* __restrict__ zr, const CgbState* __restrict__ st)
{
  __shared__ double s_red[kBlock / 64];
  if (st->all_done)
    return;
  const int dm = done_mask(st, nrhs);
  for (int c = 0; c < nrhs; ++c) {
    if ((dm >> c) & 1)
      continue; // its history ends at kstop[c]
    const double rz = reduce_column(partials_rz, len, nrhs, c, s_red);
    const double rr = reduce_column(partials_rr, len, nrhs, c, s_red);
    if (threadIdx.x == 0) {
      zr[(2 * k) * nrhs + c] = rz;
      zr[(2 * k + 1) * nrhs + c] = rr;
    }
  }
}

__global__ void pcgb_reset_kernel(CgbState* st, double rtol, double* zr,
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
    zr[2 * i] = 0.0;
    zr[2 * i + 1] = 0.0;
    pAp[i] = 0.0;
  }
}

} // namespace

#define SPMV_PCGB_REQUIRE_WS_K(ctx, ws, k, kmin)                               \
  SPMV_REQUIRE((ctx) && (ws) && (ws)->ctx == (ctx) && (k) >= (kmin)            \
               && (k) <= (ws)->kmax)

extern "C" {

int spmv_hip_pcgb_ws_create(spmv_hip_ctx* ctx, int kmax, int nrhs,
                            spmv_hip_pcgb_ws** out)
{
  SPMV_REQUIRE(out);
  *out = nullptr;
  SPMV_REQUIRE(ctx && nrhs_ok(nrhs));
  SPMV_REQUIRE(kmax >= 0 && kmax < INT_MAX / (4 * SPMV_CGB_MAX));
  return solver_ws_create(ctx, kmax, out, [&](spmv_hip_pcgb_ws& w) {
    w.nrhs = nrhs;
    const size_t hist = (size_t)(kmax + 1) * nrhs;
    const size_t part = (size_t)ctx->dot_blocks * nrhs;
    w.own.alloc(w.zr, 2 * hist);
    w.own.alloc(w.pAp, hist);
    w.own.alloc(w.partials, part);
    w.own.alloc(w.partials_rr, part);
    w.own.alloc(w.st, 1);
  });
}

int spmv_hip_pcgb_ws_destroy(spmv_hip_pcgb_ws* ws)
{
  return solver_ws_destroy(ws);
}

int spmv_hip_pcgb_ws_reset(spmv_hip_pcgb_ws* ws, double rtol, void* stream)
{
  SPMV_REQUIRE(ws);
  SPMV_SET_DEVICE(ws->ctx);
  const int count = (ws->kmax + 1) * ws->nrhs;
  hipLaunchKernelGGL(pcgb_reset_kernel, ws_reset_grid(count), dim3(kBlock), 0,
                     spmv_stream(ws->ctx, stream), ws->st, rtol, ws->zr,
                     ws->pAp, count);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcgb_ws_capacity(const spmv_hip_pcgb_ws* ws, int* kmax, int* nrhs)
{
  SPMV_REQUIRE(ws && kmax && nrhs);
  *kmax = ws->kmax;
  *nrhs = ws->nrhs;
  return SPMV_HIP_OK;
}

int spmv_hip_pcgb_ws_rz_rr(spmv_hip_pcgb_ws* ws, int k, double** slot)
{
  SPMV_REQUIRE(ws && slot && k >= 0 && k <= ws->kmax);
  *slot = ws->zr + 2 * (size_t)k * ws->nrhs;
  return SPMV_HIP_OK;
}

int spmv_hip_pcgb_ws_pAp(spmv_hip_pcgb_ws* ws, int k, double** slot)
{
  SPMV_REQUIRE(ws && slot && k >= 0 && k <= ws->kmax);
  *slot = ws->pAp + (size_t)k * ws->nrhs;
  return SPMV_HIP_OK;
}

int spmv_hip_pcgb_ws_read_async(spmv_hip_pcgb_ws* ws, int32_t* host_state,
                                size_t host_state_len, double* host_rz_rr,
                                size_t host_rz_rr_len, void* stream)
{
  SPMV_REQUIRE(ws);
  // a short state buffer gets nothing at all either
  SPMV_REQUIRE(!host_state || host_state_len >= SPMV_HIP_CGB_STATE_WORDS);
  return ws_read_async(ws->ctx, stream, host_state, &ws->st->all_done,
                       SPMV_HIP_CGB_STATE_WORDS, host_rz_rr, host_rz_rr_len,
                       ws->zr, 2 * ((size_t)ws->kmax + 1) * (size_t)ws->nrhs);
}

int spmv_hip_pcgb_init_f64(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int64_t M,
                           const double* B, double* R, double* X, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && M >= 0);
  SPMV_REQUIRE(M == 0 || (B && R && X));
  SPMV_SET_DEVICE(ctx);
  const int nrhs = ws->nrhs;
  const bool nt = M * nrhs >= ctx->blas1_nt_min_elems;
  SPMV_CGB_LAUNCH_NT(nt, pcgb_init_kernel, rows_grid(ctx, M),
                     spmv_stream(ctx, stream), M, nrhs, B, R, X,
                     ws->partials_rr, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

// the two dot products share one launcher: Y is read, or written first (dinv)
static int pcgb_dot(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int64_t M,
                    const double* dinv, const double* X, double* Y, void* stream)
{
  const int nrhs = ws->nrhs;
  SPMV_REQUIRE(!native_width(nrhs) || aligned16(X, Y));
  SPMV_SET_DEVICE(ctx);
  const bool nt = M * nrhs >= ctx->blas1_nt_min_elems;
  hipStream_t st = spmv_stream(ctx, stream);
  const int len = ctx->dot_blocks;
  if (native_width(nrhs)) {
    const int64_t n2 = M * nrhs / 2;
    const int grid = stream_grid_capped(ctx, M * nrhs);
#define SPMV_PCGB_DOT(K, NT, DINV)                                             \
  hipLaunchKernelGGL((pcgb_dot_kernel<K, NT, DINV>), dim3(grid), dim3(kBlock), \
                     0, st, n2, ws->st, dinv, X, Y, ws->partials, len)
#define SPMV_PCGB_DOT_K(K)                                                     \
  do {                                                                         \
    if (nt && dinv)                                                            \
      SPMV_PCGB_DOT(K, true, true);                                            \
    else if (nt)                                                               \
      SPMV_PCGB_DOT(K, true, false);                                           \
    else if (dinv)                                                             \
      SPMV_PCGB_DOT(K, false, true);                                           \
    else                                                                       \
      SPMV_PCGB_DOT(K, false, false);                                          \
  } while (0)
    if (nrhs == 2)
      SPMV_PCGB_DOT_K(2);
    else if (nrhs == 4)
      SPMV_PCGB_DOT_K(4);
    else
      SPMV_PCGB_DOT_K(8);
#undef SPMV_PCGB_DOT_K
#undef SPMV_PCGB_DOT
  } else {
    const int grid = rows_grid(ctx, M);
#define SPMV_PCGB_DOT_ROWS(NT, DINV)                                           \
  hipLaunchKernelGGL((pcgb_dot_rows_kernel<NT, DINV>), dim3(grid),             \
                     dim3(kBlock), 0, st, M, nrhs, ws->st, dinv, X, Y,         \
                     ws->partials, len)
    if (nt && dinv)
      SPMV_PCGB_DOT_ROWS(true, true);
    else if (nt)
      SPMV_PCGB_DOT_ROWS(true, false);
    else if (dinv)
      SPMV_PCGB_DOT_ROWS(false, true);
    else
      SPMV_PCGB_DOT_ROWS(false, false);
#undef SPMV_PCGB_DOT_ROWS
  }
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcgb_dot_pAp_f64(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int64_t M,
                              const double* P, const double* AP, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && M >= 0);
  SPMV_REQUIRE(M == 0 || (P && AP));
  // (the kernel without dinv only reads its second vector)
  return pcgb_dot(ctx, ws, M, nullptr, P, const_cast<double*>(AP), stream);
}

int spmv_hip_pcgb_dot_rz_f64(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int64_t M,
                             const double* dinv, const double* R, double* Z,
                             void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && M >= 0);
  SPMV_REQUIRE(M == 0 || (R && Z));
  return pcgb_dot(ctx, ws, M, dinv, R, Z, stream);
}

int spmv_hip_pcgb_reduce_pAp(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int k,
                             void* stream)
{
  SPMV_PCGB_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(pcgb_reduce_pAp_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->partials, ctx->dot_blocks, k,
                     ws->nrhs, ws->zr, ws->pAp, ws->st);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcgb_reduce_rz_rr(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int k,
                               void* stream)
{
  SPMV_PCGB_REQUIRE_WS_K(ctx, ws, k, 0);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(pcgb_reduce_rz_rr_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->partials, ws->partials_rr,
                     ctx->dot_blocks, k, ws->nrhs, ws->zr, ws->st);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcgb_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int k,
                               int64_t M, const double* AP, double* R,
                               void* stream)
{
  SPMV_PCGB_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(M >= 0 && (M == 0 || (AP && R)));
  const int nrhs = ws->nrhs;
  SPMV_REQUIRE(!native_width(nrhs) || aligned16(AP, R));
  SPMV_SET_DEVICE(ctx);
  const bool nt = M * nrhs >= ctx->blas1_nt_min_elems;
  hipStream_t st = spmv_stream(ctx, stream);
  if (native_width(nrhs)) {
    const int64_t n2 = M * nrhs / 2;
    SPMV_CGB_LAUNCH_WIDTH(nrhs, nt, pcgb_update_r_kernel,
                          stream_grid_capped(ctx, M * nrhs), st, n2, k, ws->zr,
                          ws->pAp, ws->st, AP, R, ws->partials_rr,
                          ctx->dot_blocks);
  } else {
    SPMV_CGB_LAUNCH_NT(nt, pcgb_update_r_rows_kernel, rows_grid(ctx, M), st, M,
                       nrhs, k, ws->zr, ws->pAp, ws->st, AP, R, ws->partials_rr,
                       ctx->dot_blocks);
  }
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcgb_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int k,
                                int64_t M, const double* Z, double* X,
                                double* P, void* stream)
{
  SPMV_PCGB_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(M >= 0 && (M == 0 || (Z && X && P)));
  const int nrhs = ws->nrhs;
  SPMV_REQUIRE(!native_width(nrhs) || aligned16(Z, X, P));
  SPMV_SET_DEVICE(ctx);
  const bool nt = M * nrhs >= ctx->blas1_nt_min_elems;
  hipStream_t st = spmv_stream(ctx, stream);
  if (native_width(nrhs)) {
    const int64_t n2 = M * nrhs / 2;
    SPMV_CGB_LAUNCH_WIDTH(nrhs, nt, pcgb_update_xp_kernel,
                          stream_grid_capped(ctx, M * nrhs), st, n2, k, ws->zr,
                          ws->pAp, ws->st, Z, X, P);
  } else {
    SPMV_CGB_LAUNCH_NT(nt, pcgb_update_xp_rows_kernel, rows_grid(ctx, M), st, M,
                       nrhs, k, ws->zr, ws->pAp, ws->st, Z, X, P);
  }
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
