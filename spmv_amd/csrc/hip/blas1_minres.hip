// BLAS-1 kernels of spmv::minres (gfx950): preconditioned MINRES for a
// symmetric, possibly indefinite matrix and a symmetric positive definite
// preconditioner, in the launch structure of blas1_gmres.hip.  The recurrence
// is spelled out in host/cg.h; one iteration, `.` the global dot product:
//
//   (SpMV)        Av = A v, with the partials of alfa = v.Av (fused, or the
//                 dot-partials kernel of blas1.hip)
//   update_r      alfa from its partials (one rank: every workgroup adds them
//                 itself, in the reducer's order) or from the reducer's slot;
//                 t = (Av - (beta/oldb) r1) - (alfa/beta) r2 over r1's buffer
//                 (first step: t = Av - (alfa/beta) r2); with a diagonal
//                 preconditioner or none also y = dinv * t and the partials of
//                 t.y (none: of t.t, y is not written)
//   reduce        partials -> the slot of alfa or of ry, one workgroup
//   step          ONE WAVE: every scalar of the recurrence, hist[k], k, status,
//                 done, and the five coefficients update_xwv reads
//   update_xwv    w = ((v - oldeps w1) - delta w2) * (1/gamma) over w1's
//                 buffer; x = x + phi w; v = y * (1/beta)
//
// and once per solve: init (y = dinv * r2, partials of r2.y), reduce, start
// (beta1, hist[0], the state of k = 0), update_xwv with k = 0 (v alone).
//
// Accumulation order of a dot product: stream_dot's (a thread adds its 2 * kU
// products per trip, .x then .y, element order; the odd tail element last,
// thread 0 of workgroup 0; spmv_block_sum; sum_partials), so the depth of
// blas1_cases.depth applies.
//
// Stop protocol.  `done` is raised by step or start.  After it init, reduce,
// update_r, start and step return at once.  update_xwv of iteration k runs
// when, and only when, the state says that step k completed (sc->k == k): the
// step that raised `done` with a new iterate (tolerance, kmax, beta == 0) still
// gets its x, exactly once, the steps that stop WITHOUT one (ry < 0, gamma ==
// 0) leave k alone, and every later launch finds k behind its own.  After
// `done` the next v is not formed.
//
// Built with -ffp-contract=off: every product, sum, difference, quotient and
// square root is a rounding of its own.  Streaming shape: blas1_stream.h.
#include "common.h"
#include "blas1_stream.h"
#include "minres_ws.h"

#include <cmath>
#include <cstddef>

namespace
{

__device__ __forceinline__ void raise_done(MinresScalars* sc, int kstop,
                                           int status)
{
  sc->kstop = kstop;
  sc->status = status;
  sc->done = 1;
}

// y = dinv * r2 ; partials of r2.y (dinv == nullptr: of r2.r2, y not written)
template <bool NT>
__global__ __launch_bounds__(kBlock) void minres_init_kernel(
    int64_t n, const MinresScalars* sc, const double* __restrict__ r2,
    const double* __restrict__ dinv, double* __restrict__ y,
    double* __restrict__ p_ry, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 rv[kU], dv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      rv[u] = vload<NT>(r2, i);
      if (dinv)
        dv[u] = vload<NT>(dinv, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      f64x2 yv = rv[u];
      if (dinv) {
        yv.x = dv[u].x * rv[u].x;
        yv.y = dv[u].y * rv[u].y;
        vstore<NT>(y, i, yv);
      }
      acc += rv[u].x * yv.x;
      acc += rv[u].y * yv.y;
    }
  }
  if (odd_tail(n)) {
    const double t = r2[n - 1];
    double yt = t;
    if (dinv) {
      yt = dinv[n - 1] * t;
      y[n - 1] = yt;
    }
    acc += t * yt;
  }
  const double s = spmv_block_sum(acc, s_red);
  if (threadIdx.x == 0)
    p_ry[blockIdx.x] = s;
  clear_partials_tail(p_ry, len);
}

// one workgroup: partials (+ partials2, the remote block's share of v.Av) ->
// the slot
__global__ __launch_bounds__(kBlock) void minres_reduce_kernel(
    const MinresScalars* sc, const double* __restrict__ partials,
    const double* __restrict__ partials2, int len, double* __restrict__ dst)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double s = sum_partials(partials, partials2, len, s_red);
  if (threadIdx.x == 0)
    *dst = s;
}

// r1 is read and written at the same index by the same thread: no __restrict__
template <bool NT>
__global__ __launch_bounds__(kBlock) void minres_update_r_kernel(
    int64_t n, MinresScalars* sc, const double* __restrict__ Av, double* r1,
    const double* __restrict__ r2, const double* __restrict__ dinv,
    double* __restrict__ y, const double* __restrict__ p_alfa,
    const double* __restrict__ p_alfa2, int len, int reduced,
    double* __restrict__ p_ry)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  double alfa;
  if (reduced) {
    alfa = sc->alfa;
  } else {
    // (nobody reads the slot in this launch: step does)
    alfa = consume_partials(p_alfa, p_alfa2, len, s_red, &s_bcast);
    if (blockIdx.x == 0 && threadIdx.x == 0)
      sc->alfa = alfa;
  }
  const bool first = sc->k == 0;
  const double bob = sc->bob;
  const double q = alfa / sc->beta;
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 av[kU], r1v[kU], r2v[kU], dv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      av[u] = vload<NT>(Av, i);
      if (!first)
        r1v[u] = vload<NT>(r1, i);
      r2v[u] = vload<NT>(r2, i);
      if (dinv)
        dv[u] = vload<NT>(dinv, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      f64x2 t = av[u];
      if (!first) {
        t.x = t.x - bob * r1v[u].x;
        t.y = t.y - bob * r1v[u].y;
      }
      t.x = t.x - q * r2v[u].x;
      t.y = t.y - q * r2v[u].y;
      vstore<NT>(r1, i, t);
      f64x2 yv = t;
      if (dinv) {
        yv.x = dv[u].x * t.x;
        yv.y = dv[u].y * t.y;
        vstore<NT>(y, i, yv);
      }
      acc += t.x * yv.x;
      acc += t.y * yv.y;
    }
  }
  if (odd_tail(n)) {
    double t = Av[n - 1];
    if (!first)
      t = t - bob * r1[n - 1];
    t = t - q * r2[n - 1];
    r1[n - 1] = t;
    double yt = t;
    if (dinv) {
      yt = dinv[n - 1] * t;
      y[n - 1] = yt;
    }
    acc += t * yt;
  }
  if (!p_ry) // the preconditioner's application and its own dot follow
    return;
  const double s = spmv_block_sum(acc, s_red);
  if (threadIdx.x == 0)
    p_ry[blockIdx.x] = s;
  clear_partials_tail(p_ry, len);
}

// one wave: beta1, hist[0] and the state in front of the first step
__global__ __launch_bounds__(64) void minres_start_kernel(
    MinresScalars* sc, double* __restrict__ hist)
{
  if (threadIdx.x != 0 || sc->done)
    return;
  const double ry = sc->ry;
  if (ry < 0.0) { // M is not positive definite
    raise_done(sc, 0, 2);
    return;
  }
  const double beta1 = sqrt(ry);
  hist[0] = beta1;
  if (beta1 == 0.0) { // x = 0 is the answer
    raise_done(sc, 0, 0);
    return;
  }
  sc->oldb = 0.0;
  sc->beta = beta1;
  sc->dbar = 0.0;
  sc->epsln = 0.0;
  sc->phibar = beta1;
  sc->cs = -1.0;
  sc->sn = 0.0;
  sc->inv_beta = 1.0 / beta1;
}

// one wave: the scalar part of an iteration.  Every comparison is written so
// that a NaN goes on: a solve on non-finite data ends at kmax.
__global__ __launch_bounds__(64) void minres_step_kernel(
    MinresScalars* sc, double* __restrict__ hist)
{
  if (threadIdx.x != 0 || sc->done)
    return;
  const int k = sc->k;
  if (k >= sc->kmax) { // (no room in the history: the host never asks)
    raise_done(sc, k, 0);
    return;
  }
  const double alfa = sc->alfa;
  const double ry = sc->ry;
  if (ry < 0.0) {
    raise_done(sc, k, 2);
    return;
  }
  const double oldb = sc->beta;
  const double beta = sqrt(ry);
  const double cs0 = sc->cs, sn0 = sc->sn, dbar0 = sc->dbar;
  const double oldeps = sc->epsln;
  const double delta = cs0 * dbar0 + sn0 * alfa;
  const double gbar = sn0 * dbar0 - cs0 * alfa;
  const double epsln = sn0 * beta;
  const double dbar = -cs0 * beta;
  const double gamma = sqrt(gbar * gbar + beta * beta);
  if (gamma == 0.0) { // a singular direction
    raise_done(sc, k, 3);
    return;
  }
  const double cs = gbar / gamma;
  const double sn = beta / gamma;
  const double phi = cs * sc->phibar;
  const double phibar = sn * sc->phibar;
  sc->oldb = oldb;
  sc->beta = beta;
  sc->epsln = epsln;
  sc->dbar = dbar;
  sc->cs = cs;
  sc->sn = sn;
  sc->phibar = phibar;
  sc->oldeps = oldeps;
  sc->delta = delta;
  sc->inv_gamma = 1.0 / gamma;
  sc->phi = phi;
  sc->k = k + 1;
  const double res = fabs(phibar);
  hist[k + 1] = res;
  if (beta == 0.0) { // the Lanczos process ended: x is exact
    raise_done(sc, k + 1, 1);
    return;
  }
  if (res / hist[0] < sc->rtol || k + 1 == sc->kmax) {
    raise_done(sc, k + 1, 0);
    return;
  }
  sc->inv_beta = 1.0 / beta;
  sc->bob = beta / oldb;
}

// k == 0: v = y * inv_beta alone (after start).  w1 is read and written at the
// same index by the same thread.
template <bool NT>
__global__ __launch_bounds__(kBlock) void minres_update_xwv_kernel(
    int64_t n, const MinresScalars* sc, int k, double* __restrict__ v,
    double* w1, const double* __restrict__ w2, double* __restrict__ x,
    const double* __restrict__ y)
{
  if (sc->k != k)
    return;
  const bool go_on = sc->done == 0;
  const bool update = k != 0;
  if (!update && !go_on)
    return;
  const double oldeps = sc->oldeps, delta = sc->delta;
  const double inv_gamma = sc->inv_gamma, phi = sc->phi;
  const double inv_beta = sc->inv_beta;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 vv[kU], av[kU], bv[kU], xv[kU], yv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      if (update) {
        vv[u] = vload<NT>(v, i);
        av[u] = vload<NT>(w1, i);
        bv[u] = vload<NT>(w2, i);
        xv[u] = vload<NT>(x, i);
      }
      if (go_on)
        yv[u] = vload<NT>(y, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      if (update) {
        f64x2 w;
        w.x = ((vv[u].x - oldeps * av[u].x) - delta * bv[u].x) * inv_gamma;
        w.y = ((vv[u].y - oldeps * av[u].y) - delta * bv[u].y) * inv_gamma;
        vstore<NT>(w1, i, w);
        xv[u].x = xv[u].x + phi * w.x;
        xv[u].y = xv[u].y + phi * w.y;
        vstore<NT>(x, i, xv[u]);
      }
      if (go_on) {
        yv[u].x = yv[u].x * inv_beta;
        yv[u].y = yv[u].y * inv_beta;
        vstore<NT>(v, i, yv[u]);
      }
    }
  }
  if (odd_tail(n)) {
    const int64_t e = n - 1;
    if (update) {
      const double w = ((v[e] - oldeps * w1[e]) - delta * w2[e]) * inv_gamma;
      w1[e] = w;
      x[e] = x[e] + phi * w;
    }
    if (go_on)
      v[e] = y[e] * inv_beta;
  }
}

__global__ void minres_reset_kernel(MinresScalars* sc, double rtol, int kmax,
                                    double* hist, int hist_len)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    double* d = reinterpret_cast<double*>(sc);
    for (int j = 0; j < kMinresDoubles; ++j)
      d[j] = 0.0;
    sc->rtol = rtol;
    sc->done = 0;
    sc->kstop = -1;
    sc->status = 0;
    sc->k = 0;
    sc->kmax = kmax;
  }
  if (i < hist_len)
    hist[i] = 0.0;
}

static_assert(offsetof(MinresScalars, done) == kMinresDoubles * sizeof(double),
              "the doubles of MinresScalars come first");

} // namespace

extern "C" {

// ---- workspace ----------------------------------------------------------------
int spmv_hip_minres_ws_create(spmv_hip_ctx* ctx, int kmax,
                              spmv_hip_minres_ws** out)
{
  SPMV_REQUIRE(ctx && out && kmax >= 0);
  return solver_ws_create(ctx, kmax, out, [&](spmv_hip_minres_ws& w) {
    w.own.alloc(w.hist, (size_t)kmax + 1);
    w.own.alloc(w.p_alfa, ctx->dot_blocks);
    w.own.alloc(w.p_ry, ctx->dot_blocks);
    w.own.alloc(w.sc, 1);
  });
}

int spmv_hip_minres_ws_destroy(spmv_hip_minres_ws* ws)
{
  return solver_ws_destroy(ws);
}

int spmv_hip_minres_ws_reset(spmv_hip_minres_ws* ws, double rtol, int kmax,
                             void* stream)
{
  SPMV_REQUIRE(ws && kmax >= 0 && kmax <= ws->kmax);
  SPMV_SET_DEVICE(ws->ctx);
  const int n = ws->kmax + 1;
  hipLaunchKernelGGL(minres_reset_kernel, ws_reset_grid(n), dim3(kBlock), 0,
                     spmv_stream(ws->ctx, stream), ws->sc, rtol, kmax, ws->hist,
                     n);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_minres_ws_capacity(const spmv_hip_minres_ws* ws, int* kmax)
{
  return solver_ws_capacity(ws, kmax);
}

int spmv_hip_minres_ws_array(spmv_hip_minres_ws* ws, int which, double** p,
                             int64_t* count)
{
  SPMV_REQUIRE(ws && p);
  double* q = nullptr;
  int64_t n = 0;
  switch (which) {
  case SPMV_HIP_MINRES_ALFA: q = &ws->sc->alfa, n = 1; break;
  case SPMV_HIP_MINRES_RY: q = &ws->sc->ry, n = 1; break;
  case SPMV_HIP_MINRES_HIST: q = ws->hist, n = (int64_t)ws->kmax + 1; break;
  case SPMV_HIP_MINRES_PART_ALFA: q = ws->p_alfa, n = ws->ctx->dot_blocks; break;
  case SPMV_HIP_MINRES_PART_RY: q = ws->p_ry, n = ws->ctx->dot_blocks; break;
  case SPMV_HIP_MINRES_SCALARS:
    q = reinterpret_cast<double*>(ws->sc), n = kMinresDoubles;
    break;
  default: return SPMV_HIP_EINVAL;
  }
  *p = q;
  if (count)
    *count = n;
  return SPMV_HIP_OK;
}

int spmv_hip_minres_ws_read_async(spmv_hip_minres_ws* ws,
                                  int32_t* host_done_kstop_status,
                                  double* host_hist, size_t host_hist_len,
                                  void* stream)
{
  SPMV_REQUIRE(ws);
  return ws_read_async(ws->ctx, stream, host_done_kstop_status, &ws->sc->done,
                       3, host_hist, host_hist_len, ws->hist,
                       (size_t)ws->kmax + 1);
}

int spmv_hip_minres_ws_set_state(spmv_hip_minres_ws* ws, int k, int done,
                                 void* stream)
{
  SPMV_REQUIRE(ws && k >= 0 && k <= ws->kmax);
  const int32_t words[4] = {done ? 1 : 0, done ? k : -1, 0, k};
  return ws_put_words(ws->ctx, stream, &ws->sc->done, words, 4);
}

int spmv_hip_minres_ws_get_state(spmv_hip_minres_ws* ws, int32_t* host_words5,
                                 void* stream)
{
  SPMV_REQUIRE(ws && host_words5);
  return ws_get_words(ws->ctx, stream, host_words5, &ws->sc->done, 5);
}

// ---- kernels ------------------------------------------------------------------
int spmv_hip_minres_init_f64(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws,
                             int64_t n, const double* r2, const double* dinv,
                             double* y, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE((n == 0 || (r2 && (!dinv || y))) && aligned16(r2, dinv, y));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, minres_init_kernel, stream_grid_capped(ctx, n),
                 spmv_stream(ctx, stream), n, ws->sc, r2, dinv, y, ws->p_ry,
                 ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_minres_reduce(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws, int which,
                           const double* partials2, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_REQUIRE(which == SPMV_HIP_MINRES_ALFA
               || (which == SPMV_HIP_MINRES_RY && !partials2));
  SPMV_SET_DEVICE(ctx);
  const bool alfa = which == SPMV_HIP_MINRES_ALFA;
  hipLaunchKernelGGL(minres_reduce_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc,
                     alfa ? ws->p_alfa : ws->p_ry, partials2, ctx->dot_blocks,
                     alfa ? &ws->sc->alfa : &ws->sc->ry);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_minres_start(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws,
                          void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(minres_start_kernel, dim3(1), dim3(64), 0,
                     spmv_stream(ctx, stream), ws->sc, ws->hist);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_minres_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws,
                                 int64_t n, const double* Av, double* r1,
                                 const double* r2, const double* dinv, double* y,
                                 int reduced, const double* partials2,
                                 int want_dot, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE((n == 0 || (Av && r1 && r2 && (!dinv || y)))
               && aligned16(Av, r1, r2, dinv, y));
  SPMV_REQUIRE(n == 0 || (r1 != r2 && r1 != Av));
  SPMV_SET_DEVICE(ctx);
  const int grid = want_dot ? stream_grid_capped(ctx, n) : stream_grid(ctx, n);
  SPMV_LAUNCH_NT(ctx, n, minres_update_r_kernel, grid, spmv_stream(ctx, stream),
                 n, ws->sc, Av, r1, r2, dinv, y, ws->p_alfa, partials2,
                 ctx->dot_blocks, reduced ? 1 : 0,
                 want_dot ? ws->p_ry : (double*)nullptr);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_minres_step(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws,
                         void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(minres_step_kernel, dim3(1), dim3(64), 0,
                     spmv_stream(ctx, stream), ws->sc, ws->hist);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_minres_update_xwv_f64(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws,
                                   int k, int64_t n, double* v, double* w1,
                                   const double* w2, double* x, const double* y,
                                   void* stream)
{
  SPMV_REQUIRE_WS_K(ctx, ws, k, 0);
  SPMV_REQUIRE(ctx && n >= 0);
  SPMV_REQUIRE((n == 0 || (v && y && (k == 0 || (w1 && w2 && x))))
               && aligned16(v, w1, w2, x, y));
  SPMV_REQUIRE(n == 0 || k == 0 || w1 != w2);
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, minres_update_xwv_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, ws->sc, k, v, w1, w2, x, y);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
