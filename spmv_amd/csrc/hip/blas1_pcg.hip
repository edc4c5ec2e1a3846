// BLAS-1 kernels of spmv::pcg (gfx950): CG with a diagonal preconditioner,
// given as the vector dinv of its inverse, in the launch structure of the
// unpreconditioned loop of blas1.hip.  With z = dinv * r (elementwise):
//
//   init       r = b ; x = 0 ; p = dinv*b ; partials of r.z and r.r
//   reduce_pAp partials (+ the remote block's) -> pAp[k] ; raises `done`
//   update_r   r -= alpha Ap ; partials of r.z and r.r
//              alpha = rz[k-1] / pAp[k]
//   reduce_rz_rr  partials -> {rz[k], rr[k]}, one pair (one all-reduce of 2)
//   update_xp  x += alpha p ; stop test ; p = beta p + dinv*r
//              beta = rz[k] / rz[k-1] ; stop: sqrt(rr[k]) / sqrt(rr[0]) < rtol
//   update_r_cs / update_xp_cs   the same two with the reducers folded into
//              their prologues (one rank), as in blas1.hip
//
// z is never stored: update_r and update_xp both form dinv*r in registers, so
// dinv is read twice per iteration where a stored z would be written once and
// read once -- the same bytes, one work vector less.  10 vector passes per
// iteration beside the SpMV (update_r: Ap, r, dinv in, r out; update_xp: r,
// dinv, x, p in, x, p out) against 8 of the unpreconditioned loop.
//
// The stopping test is the unpreconditioned one of cg(); a system with
// r_0 . r_0 == 0 is declared stopped at k = 0 (the rule of cg_block).  x takes
// the update of the iteration that meets the tolerance, p does not; after
// `done` every kernel here returns at once.
//
// Built with -ffp-contract=off: dinv*r, beta*p and their sum are three
// roundings, r*(dinv*r) two.  Streaming shape: see blas1_stream.h (persistent
// grid, units of kU 16-byte loads per lane and stream, non-temporal from
// blas1_nt_min_elems doubles on).
//
// Also here, as setup work of the Jacobi preconditioner: the diagonal of a CSR
// block (one thread per row) and the checked inverse of a diagonal.
#include "common.h"
#include "blas1_stream.h"
#include "pcg_ws.h"

#include <cmath>

namespace
{

// What the first kernel of iteration k finds about iteration k - 1: the solve
// stops there when rr[k-1] met the tolerance (k >= 2), or at k = 0 when
// r_0 . r_0 == 0.  Uniform across the grid: every thread reads the same words.
__device__ __forceinline__ bool stopped_before(const double* __restrict__ zr,
                                               int k, double rtol)
{
  const double rr0 = zr[1];
  if (k == 1)
    return rr0 == 0.0;
  return sqrt(zr[2 * (k - 1) + 1]) / sqrt(rr0) < rtol;
}

// r += nalpha * Ap ; this thread's shares of r.(dinv*r) and r.r
template <bool NT>
__device__ __forceinline__ void stream_update_r(int64_t n2, double nalpha,
                                                const double* Ap,
                                                const double* dinv, double* r,
                                                double& acc_rz, double& acc_rr)
{
  SPMV_FOR_UNITS(n2)
  {
    f64x2 av[kU], rv[kU], dv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      av[u] = vload<NT>(Ap, i);
      rv[u] = vload<NT>(r, i);
      dv[u] = vload<NT>(dinv, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      rv[u].x += nalpha * av[u].x;
      rv[u].y += nalpha * av[u].y;
      vstore<NT>(r, i, rv[u]);
      const double zx = dv[u].x * rv[u].x, zy = dv[u].y * rv[u].y;
      acc_rz += rv[u].x * zx;
      acc_rz += rv[u].y * zy;
      acc_rr += rv[u].x * rv[u].x;
      acc_rr += rv[u].y * rv[u].y;
    }
  }
}

// x += alpha p ; p = beta p + dinv*r
template <bool NT>
__device__ __forceinline__ void stream_update_xp(int64_t n2, double alpha,
                                                 double beta, const double* r,
                                                 const double* dinv, double* x,
                                                 double* p)
{
  SPMV_FOR_UNITS(n2)
  {
    f64x2 pv[kU], xv[kU], rv[kU], dv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      pv[u] = vload<NT>(p, i);
      xv[u] = vload<NT>(x, i);
      rv[u] = vload<NT>(r, i);
      dv[u] = vload<NT>(dinv, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      xv[u].x += alpha * pv[u].x;
      xv[u].y += alpha * pv[u].y;
      vstore<NT>(x, i, xv[u]);
      const double zx = dv[u].x * rv[u].x, zy = dv[u].y * rv[u].y;
      pv[u].x = beta * pv[u].x;
      pv[u].y = beta * pv[u].y;
      pv[u].x += zx;
      pv[u].y += zy;
      vstore<NT>(p, i, pv[u]);
    }
  }
}

// the odd last element of the three updates (workgroup 0, thread 0)
__device__ __forceinline__ void tail_update_r(int64_t i, double nalpha,
                                              const double* Ap,
                                              const double* dinv, double* r,
                                              double& acc_rz, double& acc_rr)
{
  const double rv = r[i] + nalpha * Ap[i];
  r[i] = rv;
  const double z = dinv[i] * rv;
  acc_rz += rv * z;
  acc_rr += rv * rv;
}

// body of update_r / update_r_cs behind their prologues
template <bool NT>
__device__ __forceinline__ void update_r_body(
    int64_t n, double alpha, const double* __restrict__ Ap,
    const double* __restrict__ dinv, double* __restrict__ r,
    double* __restrict__ partials_rz, double* __restrict__ partials_rr, int len,
    double* s_red)
{
  const double nalpha = -alpha;
  double acc_rz = 0.0, acc_rr = 0.0;
  stream_update_r<NT>(n >> 1, nalpha, Ap, dinv, r, acc_rz, acc_rr);
  if (odd_tail(n))
    tail_update_r(n - 1, nalpha, Ap, dinv, r, acc_rz, acc_rr);
  store_pair_partials(acc_rz, acc_rr, partials_rz, partials_rr, len, s_red);
}

// body of update_xp / update_xp_cs: rz_new, rr_new are iteration k's scalars
template <bool NT>
__device__ __forceinline__ void update_xp_body(
    int64_t n, double rr0, double rz_old, double rz_new, double rr_new,
    double pap, double rtol, const double* __restrict__ r,
    const double* __restrict__ dinv, double* __restrict__ x,
    double* __restrict__ p)
{
  const double alpha = rz_old / pap;
  const double beta = rz_new / rz_old;
  const bool converged = sqrt(rr_new) / sqrt(rr0) < rtol;
  const bool tail = odd_tail(n);
  const int64_t i = n - 1;
  if (converged) { // x takes this iteration's update, p stays
    stream_axpy<NT>(n >> 1, alpha, p, x);
    if (tail)
      x[i] += alpha * p[i];
    return;
  }
  stream_update_xp<NT>(n >> 1, alpha, beta, r, dinv, x, p);
  if (tail) {
    x[i] += alpha * p[i];
    const double z = dinv[i] * r[i];
    p[i] = beta * p[i] + z;
  }
}

// Start in one pass over b: r = b, x0 = 0, p = dinv*b, partials of r.z and r.r
// (b and dinv need no alignment here).
template <bool NT>
__global__ __launch_bounds__(kBlock) void pcg_init_kernel(
    int64_t n, const double* __restrict__ b, const double* __restrict__ dinv,
    double* __restrict__ r, double* __restrict__ p, double* __restrict__ x,
    double* __restrict__ partials_rz, double* __restrict__ partials_rr, int len)
{
  __shared__ double s_red[kBlock / 64];
  double acc_rz = 0.0, acc_rr = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = b[i];
    const double z = dinv[i] * v;
    if constexpr (NT) {
      __builtin_nontemporal_store(v, &r[i]);
      __builtin_nontemporal_store(z, &p[i]);
      __builtin_nontemporal_store(0.0, &x[i]);
    } else {
      r[i] = v;
      p[i] = z;
      x[i] = 0.0;
    }
    acc_rz += v * z;
    acc_rr += v * v;
  }
  store_pair_partials(acc_rz, acc_rr, partials_rz, partials_rr, len, s_red);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void pcg_update_r_kernel(
    int64_t n, int k, const double* __restrict__ zr,
    const double* __restrict__ pAp, const PcgScalars* __restrict__ sc,
    const double* __restrict__ Ap, const double* __restrict__ dinv,
    double* __restrict__ r, double* __restrict__ partials_rz,
    double* __restrict__ partials_rr, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double alpha = zr[2 * (k - 1)] / pAp[k];
  update_r_body<NT>(n, alpha, Ap, dinv, r, partials_rz, partials_rr, len, s_red);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void pcg_update_xp_kernel(
    int64_t n, int k, const double* __restrict__ zr,
    const double* __restrict__ pAp, const PcgScalars* __restrict__ sc,
    const double* __restrict__ r, const double* __restrict__ dinv,
    double* __restrict__ x, double* __restrict__ p)
{
  if (sc->done)
    return;
  update_xp_body<NT>(n, zr[1], zr[2 * (k - 1)], zr[2 * k], zr[2 * k + 1],
                     pAp[k], sc->rtol, r, dinv, x, p);
}

// Reduces the p.Ap partials of iteration k.  The first single-workgroup kernel
// after the p update of iteration k - 1, so it also raises `done` (see
// stopped_before): every later pcg_* kernel then returns at once.
__global__ __launch_bounds__(kBlock) void pcg_reduce_pAp_kernel(
    const double* __restrict__ partials, const double* __restrict__ partials2,
    int len, int k, const double* __restrict__ zr, double* __restrict__ pAp,
    PcgScalars* __restrict__ sc)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  if (stopped_before(zr, k, sc->rtol)) { // uniform across the workgroup
    if (threadIdx.x == 0) {
      sc->kstop = k - 1;
      sc->done = 1;
    }
    return;
  }
  const double s = sum_partials(partials, partials2, len, s_red);
  if (threadIdx.x == 0)
    pAp[k] = s;
}

// partials of r.z and r.r -> the pair {rz[k], rr[k]}
__global__ __launch_bounds__(kBlock) void pcg_reduce_rz_rr_kernel(
    const double* __restrict__ partials_rz,
    const double* __restrict__ partials_rr, int len, double* __restrict__ pair,
    const PcgScalars* __restrict__ sc)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double rz = sum_partials(partials_rz, nullptr, len, s_red);
  __syncthreads(); // s_red is reused
  const double rr = sum_partials(partials_rr, nullptr, len, s_red);
  if (threadIdx.x == 0) {
    pair[0] = rz;
    pair[1] = rr;
  }
}

// ---- consumer-side reductions (one rank), as in blas1.hip -------------------
// pcg_reduce_pAp_kernel + pcg_update_r_kernel in one launch
template <bool NT>
__global__ __launch_bounds__(kBlock) void pcg_update_r_cs_kernel(
    int64_t n, int k, const double* __restrict__ zr, double* __restrict__ pAp,
    PcgScalars* __restrict__ sc, const double* __restrict__ pap_partials,
    const double* __restrict__ pap_partials2, int len,
    const double* __restrict__ Ap, const double* __restrict__ dinv,
    double* __restrict__ r, double* __restrict__ partials_rz,
    double* __restrict__ partials_rr)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  if (stopped_before(zr, k, sc->rtol)) { // uniform across the grid
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      sc->kstop = k - 1;
      sc->done = 1;
    }
    return;
  }
  const double pap
      = consume_partials(pap_partials, pap_partials2, len, s_red, &s_bcast);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    pAp[k] = pap;
  const double alpha = zr[2 * (k - 1)] / pap;
  update_r_body<NT>(n, alpha, Ap, dinv, r, partials_rz, partials_rr, len, s_red);
}

// pcg_reduce_rz_rr_kernel + pcg_update_xp_kernel in one launch
template <bool NT>
__global__ __launch_bounds__(kBlock) void pcg_update_xp_cs_kernel(
    int64_t n, int k, double* __restrict__ zr, const double* __restrict__ pAp,
    const PcgScalars* __restrict__ sc, const double* __restrict__ partials_rz,
    const double* __restrict__ partials_rr, int len,
    const double* __restrict__ r, const double* __restrict__ dinv,
    double* __restrict__ x, double* __restrict__ p)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  const double rz_new
      = consume_partials(partials_rz, nullptr, len, s_red, &s_bcast);
  const double rr_new
      = consume_partials(partials_rr, nullptr, len, s_red, &s_bcast);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    zr[2 * k] = rz_new;
    zr[2 * k + 1] = rr_new;
  }
  update_xp_body<NT>(n, zr[1], zr[2 * (k - 1)], rz_new, rr_new, pAp[k],
                     sc->rtol, r, dinv, x, p);
}

__global__ void pcg_reset_kernel(PcgScalars* sc, double rtol, double* zr,
                                 double* pAp, int kmax)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    sc->rtol = rtol;
    sc->done = 0;
    sc->kstop = -1;
  }
  if (i <= kmax) {
    zr[2 * i] = 0.0;
    zr[2 * i + 1] = 0.0;
    pAp[i] = 0.0;
  }
}

// ---- setup of the Jacobi preconditioner --------------------------------------
// d[i] = sum of the entries of row i whose column is i, in storage order; 0
// when the row has none.  One thread per row.
template <typename T>
__global__ __launch_bounds__(kBlock) void csr_diagonal_kernel(
    int32_t num_rows, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ colind, const T* __restrict__ values,
    T* __restrict__ d)
{
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < num_rows;
       i += gridDim.x * blockDim.x) {
    T acc = 0;
    for (int32_t j = rowptr[i]; j < rowptr[i + 1]; ++j)
      if (colind[j] == i)
        acc += values[j];
    d[i] = acc;
  }
}

// dinv = 1 / d (d and dinv may be the same vector); counts the entries that
// are not finite or not > 0 (one vector atomic per wave that found any)
__global__ __launch_bounds__(kBlock) void jacobi_invert_kernel(
    int64_t n, const double* d, double* dinv, int32_t* bad_count)
{
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = d[i];
    dinv[i] = 1.0 / v;
    if (!(v > 0.0) || !isfinite(v))
      ++bad;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    bad += __shfl_down(bad, off, 64);
  if ((threadIdx.x & 63) == 0 && bad != 0)
    atomicAdd(bad_count, bad);
}

} // namespace

extern "C" {

// ---- workspace ----------------------------------------------------------------
int spmv_hip_pcg_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_pcg_ws** out)
{
  SPMV_REQUIRE(ctx && out && kmax >= 0);
  return solver_ws_create(ctx, kmax, out, [&](spmv_hip_pcg_ws& w) {
    const size_t hist = (size_t)kmax + 1, part = (size_t)ctx->dot_blocks;
    w.own.alloc(w.zr, 2 * hist);
    w.own.alloc(w.pAp, hist);
    w.own.alloc(w.partials, part);
    w.own.alloc(w.partials_rz, part);
    w.own.alloc(w.partials_rr, part);
    w.own.alloc(w.sc, 1);
  });
}

int spmv_hip_pcg_ws_destroy(spmv_hip_pcg_ws* ws)
{
  return solver_ws_destroy(ws);
}

int spmv_hip_pcg_ws_reset(spmv_hip_pcg_ws* ws, double rtol, void* stream)
{
  SPMV_REQUIRE(ws);
  SPMV_SET_DEVICE(ws->ctx);
  const int n = ws->kmax + 1;
  hipLaunchKernelGGL(pcg_reset_kernel, ws_reset_grid(n), dim3(kBlock), 0,
                     spmv_stream(ws->ctx, stream), ws->sc, rtol, ws->zr,
                     ws->pAp, ws->kmax);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_ws_capacity(const spmv_hip_pcg_ws* ws, int* kmax)
{
  return solver_ws_capacity(ws, kmax);
}

int spmv_hip_pcg_ws_rz_rr(spmv_hip_pcg_ws* ws, int k, double** pair)
{
  SPMV_REQUIRE(ws && pair && k >= 0 && k <= ws->kmax);
  *pair = ws->zr + 2 * (size_t)k;
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_ws_pAp(spmv_hip_pcg_ws* ws, int k, double** slot)
{
  SPMV_REQUIRE(ws && slot && k >= 0 && k <= ws->kmax);
  *slot = ws->pAp + k;
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_ws_partials(spmv_hip_pcg_ws* ws, double** partials)
{
  SPMV_REQUIRE(ws && partials);
  *partials = ws->partials;
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_ws_done_flag(spmv_hip_pcg_ws* ws, const int32_t** done)
{
  SPMV_REQUIRE(ws && done);
  *done = &ws->sc->done;
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_ws_read_async(spmv_hip_pcg_ws* ws, int32_t* host_done_kstop,
                               double* host_rz_rr, size_t host_rz_rr_len,
                               void* stream)
{
  SPMV_REQUIRE(ws);
  return ws_read_async(ws->ctx, stream, host_done_kstop, &ws->sc->done, 2,
                       host_rz_rr, host_rz_rr_len, ws->zr,
                       2 * ((size_t)ws->kmax + 1));
}

// ---- kernels ------------------------------------------------------------------
int spmv_hip_pcg_init_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int64_t n,
                          const double* b, const double* dinv, double* r,
                          double* p, double* x, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE(n == 0 || (b && dinv && r && p && x));
  SPMV_SET_DEVICE(ctx);
  int grid = spmv_grid_for(ctx, n, kBlock);
  if (grid > ctx->dot_blocks)
    grid = ctx->dot_blocks;
  SPMV_LAUNCH_NT(ctx, n, pcg_init_kernel, grid, spmv_stream(ctx, stream), n, b,
                 dinv, r, p, x, ws->partials_rz, ws->partials_rr,
                 ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_reduce_pAp(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                            void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(pcg_reduce_pAp_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->partials,
                     (const double*)nullptr, ctx->dot_blocks, k, ws->zr,
                     ws->pAp, ws->sc);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_reduce_pAp2(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                             const double* partials2, void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(partials2);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(pcg_reduce_pAp_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->partials, partials2,
                     ctx->dot_blocks, k, ws->zr, ws->pAp, ws->sc);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_reduce_rz_rr(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                              void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 0);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(pcg_reduce_rz_rr_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->partials_rz,
                     ws->partials_rr, ctx->dot_blocks, ws->zr + 2 * (size_t)k,
                     ws->sc);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                              int64_t n, const double* Ap, const double* dinv,
                              double* r, void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (Ap && dinv && r)));
  SPMV_REQUIRE(aligned16(Ap, dinv, r));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, pcg_update_r_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, k, ws->zr, ws->pAp, ws->sc, Ap,
                 dinv, r, ws->partials_rz, ws->partials_rr, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                               int64_t n, const double* r, const double* dinv,
                               double* x, double* p, void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (r && dinv && x && p)));
  SPMV_REQUIRE(aligned16(r, dinv, x, p));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, pcg_update_xp_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, k, ws->zr, ws->pAp, ws->sc, r,
                 dinv, x, p);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_update_r_cs_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                                 int64_t n, const double* Ap,
                                 const double* dinv, double* r,
                                 const double* pap_partials2, void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (Ap && dinv && r)));
  SPMV_REQUIRE(aligned16(Ap, dinv, r));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, pcg_update_r_cs_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, k, ws->zr, ws->pAp, ws->sc,
                 ws->partials, pap_partials2, ctx->dot_blocks, Ap, dinv, r,
                 ws->partials_rz, ws->partials_rr);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_pcg_update_xp_cs_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                                  int64_t n, const double* r,
                                  const double* dinv, double* x, double* p,
                                  void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (r && dinv && x && p)));
  SPMV_REQUIRE(aligned16(r, dinv, x, p));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, pcg_update_xp_cs_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, k, ws->zr, ws->pAp, ws->sc,
                 ws->partials_rz, ws->partials_rr, ctx->dot_blocks, r, dinv, x,
                 p);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

// ---- Jacobi setup ---------------------------------------------------------------
int spmv_hip_csr_diagonal_f64(spmv_hip_ctx* ctx, int32_t num_rows,
                              const int32_t* rowptr, const int32_t* colind,
                              const double* values, double* d, void* stream)
{
  SPMV_REQUIRE(ctx && num_rows >= 0);
  if (num_rows == 0)
    return SPMV_HIP_OK;
  SPMV_REQUIRE(rowptr && colind && values && d);
  SPMV_SET_DEVICE(ctx);
  const int grid = spmv_grid_for(ctx, num_rows, kBlock);
  hipLaunchKernelGGL((csr_diagonal_kernel<double>), dim3(grid), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), num_rows, rowptr, colind, values,
                     d);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_csr_diagonal_f32(spmv_hip_ctx* ctx, int32_t num_rows,
                              const int32_t* rowptr, const int32_t* colind,
                              const float* values, float* d, void* stream)
{
  SPMV_REQUIRE(ctx && num_rows >= 0);
  if (num_rows == 0)
    return SPMV_HIP_OK;
  SPMV_REQUIRE(rowptr && colind && values && d);
  SPMV_SET_DEVICE(ctx);
  const int grid = spmv_grid_for(ctx, num_rows, kBlock);
  hipLaunchKernelGGL((csr_diagonal_kernel<float>), dim3(grid), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), num_rows, rowptr, colind, values,
                     d);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_jacobi_invert_f64(spmv_hip_ctx* ctx, int64_t n, const double* d,
                               double* dinv, int32_t* bad_count, void* stream)
{
  SPMV_REQUIRE(ctx && n >= 0 && bad_count && (n == 0 || (d && dinv)));
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  SPMV_CHECK_HIP(hipMemsetAsync(bad_count, 0, sizeof(int32_t), st));
  if (n == 0)
    return SPMV_HIP_OK;
  const int grid = spmv_grid_for(ctx, n, kBlock);
  hipLaunchKernelGGL(jacobi_invert_kernel, dim3(grid), dim3(kBlock), 0, st, n,
                     d, dinv, bad_count);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
