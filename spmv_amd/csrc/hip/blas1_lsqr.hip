// BLAS-1 kernels of spmv::lsqr (gfx950): LSQR (Paige and Saunders) for
// rectangular and square nonsymmetric matrices on Matrix::mult and
// Matrix::transpmult, in the launch structure of blas1_minres.hip.  The
// recurrence is spelled out in host/cg.h.  Both vectors of the Golub-Kahan
// process are kept UN-NORMALISED: ut with its scale ib = 1 / beta, vt with ia =
// 1 / alpha; A and A^T are linear, so the scales ride into the kernel that
// consumes the product.  One iteration, `.` the global dot product:
//
//   (mult)        Av = A vt
//   update_u      ut = Av * ia - alpha * (ut * ib) in place; partials of ut.ut
//   (transpmult)  Atu = A^T ut, the reverse halo update
//   update_v      beta = sqrt(ut.ut) from the partials (one rank: every
//                 workgroup adds them itself, in the reducer's order) or from
//                 the reducer's slot; ib = 1 / beta; vn = Atu * ib - beta * (vt
//                 * ia) over vt; partials of vn.vn (beta == 0: vt stays, the
//                 partials are zero)
//   reduce        partials -> the slot of uu or of vv, one workgroup (several
//                 ranks only)
//   step          one workgroup adds the partials of vn.vn in the reducer's
//                 order (or reads the slot); its thread 0 then holds every
//                 scalar of the recurrence: both rotations, the two histories,
//                 k, status, done, and the coefficients update_xw reads
//   update_xw     x = x + t1 * w; not stopped: w = vt * ia - t2 * w
//
// and once per solve: the dot-partials kernel of blas1.hip on ut = b,
// transpmult, update_v with first != 0 (vt = Atu * ib), start (hist_r[0],
// hist_ar[0], the state of k = 0), update_xw with k = 0 (w = vt * ia alone).
//
// Accumulation order of a dot product: stream_dot's (a thread adds its 2 * kU
// products per trip, .x then .y, element order; the odd tail element last,
// thread 0 of workgroup 0; spmv_block_sum; sum_partials), so the depth of
// blas1_cases.depth applies.
//
// Alignment.  Vectors whose addresses are all multiples of 16 are walked with
// 16-byte accesses; any other set of 8-byte aligned vectors with two 8-byte
// accesses per element, the same elements in the same threads, so the bits do
// not depend on the alignment.
//
// Stop protocol.  `done` is raised by step or start.  After it update_u,
// update_v, reduce, start and step return at once.  update_xw of iteration k
// runs when, and only when, the state says that step k completed (sc->k == k):
// the step that raised `done` still gets its x, exactly once, and every later
// launch finds k behind its own.  After `done` the next w is not formed.
//
// Built with -ffp-contract=off: every product, sum, difference, quotient and
// square root is a rounding of its own.  Streaming shape: blas1_stream.h.
#include "common.h"
#include "blas1_stream.h"
#include "lsqr_ws.h"

#include <cmath>
#include <cstddef>

namespace
{

__device__ __forceinline__ void raise_done(LsqrScalars* sc, int kstop,
                                           int status)
{
  sc->kstop = kstop;
  sc->status = status;
  sc->done = 1;
}

// element i2 of a vector: one 16-byte access (AL) or two of 8 bytes
template <bool NT, bool AL>
__device__ __forceinline__ f64x2 ld(const double* p, int64_t i2)
{
  if (AL)
    return vload<NT>(p, i2);
  f64x2 v;
  v.x = sload<NT>(p + 2 * i2);
  v.y = sload<NT>(p + 2 * i2 + 1);
  return v;
}
template <bool NT, bool AL>
__device__ __forceinline__ void st(double* p, int64_t i2, f64x2 v)
{
  if (AL) {
    vstore<NT>(p, i2, v);
  } else {
    sstore<NT>(p + 2 * i2, v.x);
    sstore<NT>(p + 2 * i2 + 1, v.y);
  }
}

// ut is read and written at the same index by the same thread: no __restrict__
template <bool NT, bool AL>
__global__ __launch_bounds__(kBlock) void lsqr_update_u_kernel(
    int64_t n, const LsqrScalars* sc, const double* __restrict__ Av, double* ut,
    double* __restrict__ p_uu, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double ia = sc->ia, ib = sc->ib, alpha = sc->alpha;
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 av[kU], uv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      av[u] = ld<NT, AL>(Av, i);
      uv[u] = ld<NT, AL>(ut, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      f64x2 t;
      t.x = av[u].x * ia - alpha * (uv[u].x * ib);
      t.y = av[u].y * ia - alpha * (uv[u].y * ib);
      st<NT, AL>(ut, i, t);
      acc += t.x * t.x;
      acc += t.y * t.y;
    }
  }
  if (odd_tail(n)) {
    const double t = Av[n - 1] * ia - alpha * (ut[n - 1] * ib);
    ut[n - 1] = t;
    acc += t * t;
  }
  const double s = spmv_block_sum(acc, s_red);
  if (threadIdx.x == 0)
    p_uu[blockIdx.x] = s;
  clear_partials_tail(p_uu, len);
}

// vt is read and written at the same index by the same thread
template <bool NT, bool AL>
__global__ __launch_bounds__(kBlock) void lsqr_update_v_kernel(
    int64_t n, LsqrScalars* sc, const double* __restrict__ Atu, double* vt,
    const double* __restrict__ p_uu, int len, int first, int reduced,
    double* __restrict__ p_vv)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  double uu;
  if (reduced) {
    uu = sc->uu;
  } else {
    // (nobody reads the slot in this launch: start and step do)
    uu = consume_partials(p_uu, nullptr, len, s_red, &s_bcast);
    if (blockIdx.x == 0 && threadIdx.x == 0)
      sc->uu = uu;
  }
  const double beta = sqrt(uu);
  double acc = 0.0;
  if (beta != 0.0) { // (a NaN goes on)
    const double ib = 1.0 / beta;
    const double ia = sc->ia;
    const int64_t n2 = n >> 1;
    SPMV_FOR_UNITS(n2)
    {
      f64x2 av[kU], vv[kU];
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        av[u] = ld<NT, AL>(Atu, i);
        if (!first)
          vv[u] = ld<NT, AL>(vt, i);
      }
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        f64x2 t;
        t.x = av[u].x * ib;
        t.y = av[u].y * ib;
        if (!first) {
          t.x = t.x - beta * (vv[u].x * ia);
          t.y = t.y - beta * (vv[u].y * ia);
        }
        st<NT, AL>(vt, i, t);
        acc += t.x * t.x;
        acc += t.y * t.y;
      }
    }
    if (odd_tail(n)) {
      double t = Atu[n - 1] * ib;
      if (!first)
        t = t - beta * (vt[n - 1] * ia);
      vt[n - 1] = t;
      acc += t * t;
    }
  }
  const double s = spmv_block_sum(acc, s_red);
  if (threadIdx.x == 0)
    p_vv[blockIdx.x] = s;
  clear_partials_tail(p_vv, len);
}

// one workgroup: partials -> the slot
__global__ __launch_bounds__(kBlock) void lsqr_reduce_kernel(
    const LsqrScalars* sc, const double* __restrict__ partials, int len,
    double* __restrict__ dst)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double s = sum_partials(partials, nullptr, len, s_red);
  if (threadIdx.x == 0)
    *dst = s;
}

// vv where start and step take it from: the slot, or the partials added in the
// reducer's order by this workgroup and left in the slot.  Valid in thread 0.
__device__ __forceinline__ double take_vv(LsqrScalars* sc,
                                          const double* __restrict__ p_vv,
                                          int len, int reduced, double* s_red)
{
  if (reduced)
    return sc->vv;
  const double s = sum_partials(p_vv, nullptr, len, s_red);
  if (threadIdx.x == 0)
    sc->vv = s;
  return s;
}

// one workgroup, thread 0: hist_r[0], hist_ar[0] and the state in front of the
// first step
__global__ __launch_bounds__(kBlock) void lsqr_start_kernel(
    LsqrScalars* sc, const double* __restrict__ p_vv, int len, int reduced,
    double* __restrict__ hist_r, double* __restrict__ hist_ar)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done) // (uniform: thread 0 raises it behind the sum's barrier)
    return;
  const double vv = take_vv(sc, p_vv, len, reduced, s_red);
  if (threadIdx.x != 0)
    return;
  const double beta = sqrt(sc->uu);
  hist_r[0] = beta;
  if (beta == 0.0) { // x = 0 is the answer
    raise_done(sc, 0, 0);
    return;
  }
  const double alpha = sqrt(vv);
  hist_ar[0] = alpha * beta;
  if (alpha == 0.0) { // A^T b = 0: x = 0 is the least-squares solution
    raise_done(sc, 0, 2);
    return;
  }
  sc->alpha = alpha;
  sc->beta = beta;
  sc->ia = 1.0 / alpha;
  sc->ib = 1.0 / beta;
  sc->phibar = beta;
  sc->rhobar = alpha;
  sc->anorm2 = 0.0;
  sc->psi2 = 0.0;
}

// one workgroup, thread 0: the scalar part of an iteration.  Every comparison
// is written so that a NaN goes on: a solve on non-finite data ends at kmax.
__global__ __launch_bounds__(kBlock) void lsqr_step_kernel(
    LsqrScalars* sc, const double* __restrict__ p_vv, int len, int reduced,
    double* __restrict__ hist_r, double* __restrict__ hist_ar)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double vv = take_vv(sc, p_vv, len, reduced, s_red);
  if (threadIdx.x != 0)
    return;
  const int k = sc->k;
  if (k >= sc->kmax) { // (no room in the histories: the host never asks)
    raise_done(sc, k, 0);
    return;
  }
  const double alpha = sc->alpha, damp = sc->damp;
  const double beta = sqrt(sc->uu);
  const double alpha_n = beta != 0.0 ? sqrt(vv) : 0.0;
  const double anorm2
      = sc->anorm2 + alpha * alpha + beta * beta + damp * damp;
  const double rhobar0 = sc->rhobar;
  const double rhobar1 = sqrt(rhobar0 * rhobar0 + damp * damp);
  const double cs1 = rhobar0 / rhobar1;
  const double sn1 = damp / rhobar1;
  const double psi = sn1 * sc->phibar;
  const double phibar1 = cs1 * sc->phibar;
  const double psi2 = sc->psi2 + psi * psi;
  const double rho = sqrt(rhobar1 * rhobar1 + beta * beta);
  const double cs = rhobar1 / rho;
  const double sn = beta / rho;
  const double theta = sn * alpha_n;
  const double rhobar = -cs * alpha_n;
  const double phi = cs * phibar1;
  const double phibar = sn * phibar1;
  sc->beta = beta;
  sc->anorm2 = anorm2;
  sc->psi2 = psi2;
  sc->rhobar = rhobar;
  sc->phibar = phibar;
  sc->t1 = phi / rho;
  sc->k = k + 1;
  const double res = sqrt(phibar * phibar + psi2);
  const double ares = fabs(phibar * alpha_n * cs);
  hist_r[k + 1] = res;
  hist_ar[k + 1] = ares;
  if (beta == 0.0 || alpha_n == 0.0) { // the bidiagonalisation ended
    raise_done(sc, k + 1, 2);
    return;
  }
  if (res / hist_r[0] < sc->rtol) {
    raise_done(sc, k + 1, 0);
    return;
  }
  if (ares / (sqrt(anorm2) * res) < sc->ltol) {
    raise_done(sc, k + 1, 1);
    return;
  }
  if (k + 1 == sc->kmax) {
    raise_done(sc, k + 1, 0);
    return;
  }
  sc->alpha = alpha_n;
  sc->ia = 1.0 / alpha_n;
  sc->ib = 1.0 / beta;
  sc->t2 = theta / rho;
}

// k == 0: w = vt * ia alone (after start).  x and w are read and written at the
// same index by the same thread.
template <bool NT, bool AL>
__global__ __launch_bounds__(kBlock) void lsqr_update_xw_kernel(
    int64_t n, const LsqrScalars* sc, int k, const double* __restrict__ vt,
    double* w, double* x)
{
  if (sc->k != k)
    return;
  const bool go_on = sc->done == 0;
  const bool update = k != 0;
  if (!update && !go_on)
    return;
  const double t1 = sc->t1, t2 = sc->t2, ia = sc->ia;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 vv[kU], wv[kU], xv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      if (update) {
        wv[u] = ld<NT, AL>(w, i);
        xv[u] = ld<NT, AL>(x, i);
      }
      if (go_on)
        vv[u] = ld<NT, AL>(vt, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      if (update) {
        xv[u].x = xv[u].x + t1 * wv[u].x;
        xv[u].y = xv[u].y + t1 * wv[u].y;
        st<NT, AL>(x, i, xv[u]);
      }
      if (go_on) {
        f64x2 t;
        t.x = vv[u].x * ia;
        t.y = vv[u].y * ia;
        if (update) {
          t.x = t.x - t2 * wv[u].x;
          t.y = t.y - t2 * wv[u].y;
        }
        st<NT, AL>(w, i, t);
      }
    }
  }
  if (odd_tail(n)) {
    const int64_t e = n - 1;
    const double w0 = update ? w[e] : 0.0;
    if (update)
      x[e] = x[e] + t1 * w0;
    if (go_on) {
      double t = vt[e] * ia;
      if (update)
        t = t - t2 * w0;
      w[e] = t;
    }
  }
}

__global__ void lsqr_reset_kernel(LsqrScalars* sc, double rtol, double ltol,
                                  double damp, int kmax, double* hist,
                                  int hist_len)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    double* d = reinterpret_cast<double*>(sc);
    for (int j = 0; j < kLsqrDoubles; ++j)
      d[j] = 0.0;
    sc->rtol = rtol;
    sc->ltol = ltol;
    sc->damp = damp;
    sc->done = 0;
    sc->kstop = -1;
    sc->status = 0;
    sc->k = 0;
    sc->kmax = kmax;
  }
  if (i < hist_len)
    hist[i] = 0.0;
}

static_assert(offsetof(LsqrScalars, done) == kLsqrDoubles * sizeof(double),
              "the doubles of LsqrScalars come first");

// 8-byte alignment is what a double* promises; checked all the same
template <typename... P>
bool aligned8(const P*... p)
{
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 7u) == 0;
}

} // namespace

// cached or non-temporal (the family's threshold), 16-byte accesses or pairs
#define SPMV_LAUNCH_NT_AL(ctx, n, al, kernel, grid, st, ...)                   \
  do {                                                                         \
    const bool nt_ = (int64_t)(n) >= (ctx)->blas1_nt_min_elems;                \
    if (nt_ && (al))                                                           \
      hipLaunchKernelGGL((kernel<true, true>), dim3(grid), dim3(kBlock), 0,    \
                         st, __VA_ARGS__);                                     \
    else if (nt_)                                                              \
      hipLaunchKernelGGL((kernel<true, false>), dim3(grid), dim3(kBlock), 0,   \
                         st, __VA_ARGS__);                                     \
    else if (al)                                                               \
      hipLaunchKernelGGL((kernel<false, true>), dim3(grid), dim3(kBlock), 0,   \
                         st, __VA_ARGS__);                                     \
    else                                                                       \
      hipLaunchKernelGGL((kernel<false, false>), dim3(grid), dim3(kBlock), 0,  \
                         st, __VA_ARGS__);                                     \
  } while (0)

extern "C" {

// ---- workspace ----------------------------------------------------------------
int spmv_hip_lsqr_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_lsqr_ws** out)
{
  SPMV_REQUIRE(ctx && out && kmax >= 0);
  return solver_ws_create(ctx, kmax, out, [&](spmv_hip_lsqr_ws& w) {
    w.own.alloc(w.hist, 2 * ((size_t)kmax + 1));
    w.own.alloc(w.p_uu, ctx->dot_blocks);
    w.own.alloc(w.p_vv, ctx->dot_blocks);
    w.own.alloc(w.sc, 1);
  });
}

int spmv_hip_lsqr_ws_destroy(spmv_hip_lsqr_ws* ws)
{
  return solver_ws_destroy(ws);
}

int spmv_hip_lsqr_ws_reset(spmv_hip_lsqr_ws* ws, double rtol, double ltol,
                           double damp, int kmax, void* stream)
{
  SPMV_REQUIRE(ws && kmax >= 0 && kmax <= ws->kmax);
  SPMV_SET_DEVICE(ws->ctx);
  const int n = 2 * (ws->kmax + 1);
  hipLaunchKernelGGL(lsqr_reset_kernel, ws_reset_grid(n), dim3(kBlock), 0,
                     spmv_stream(ws->ctx, stream), ws->sc, rtol, ltol, damp,
                     kmax, ws->hist, n);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lsqr_ws_capacity(const spmv_hip_lsqr_ws* ws, int* kmax)
{
  return solver_ws_capacity(ws, kmax);
}

int spmv_hip_lsqr_ws_array(spmv_hip_lsqr_ws* ws, int which, double** p,
                           int64_t* count)
{
  SPMV_REQUIRE(ws && p);
  double* q = nullptr;
  int64_t n = 0;
  switch (which) {
  case SPMV_HIP_LSQR_UU: q = &ws->sc->uu, n = 1; break;
  case SPMV_HIP_LSQR_VV: q = &ws->sc->vv, n = 1; break;
  case SPMV_HIP_LSQR_HIST_R: q = ws->hist, n = (int64_t)ws->kmax + 1; break;
  case SPMV_HIP_LSQR_HIST_AR:
    q = ws->hist + ws->kmax + 1, n = (int64_t)ws->kmax + 1;
    break;
  case SPMV_HIP_LSQR_PART_UU: q = ws->p_uu, n = ws->ctx->dot_blocks; break;
  case SPMV_HIP_LSQR_PART_VV: q = ws->p_vv, n = ws->ctx->dot_blocks; break;
  case SPMV_HIP_LSQR_SCALARS:
    q = reinterpret_cast<double*>(ws->sc), n = kLsqrDoubles;
    break;
  default: return SPMV_HIP_EINVAL;
  }
  *p = q;
  if (count)
    *count = n;
  return SPMV_HIP_OK;
}

int spmv_hip_lsqr_ws_read_async(spmv_hip_lsqr_ws* ws,
                                int32_t* host_done_kstop_status,
                                double* host_hist, size_t host_hist_len,
                                void* stream)
{
  SPMV_REQUIRE(ws);
  return ws_read_async(ws->ctx, stream, host_done_kstop_status, &ws->sc->done,
                       3, host_hist, host_hist_len, ws->hist,
                       2 * ((size_t)ws->kmax + 1));
}

int spmv_hip_lsqr_ws_set_state(spmv_hip_lsqr_ws* ws, int k, int done,
                               void* stream)
{
  SPMV_REQUIRE(ws && k >= 0 && k <= ws->kmax);
  const int32_t words[4] = {done ? 1 : 0, done ? k : -1, 0, k};
  return ws_put_words(ws->ctx, stream, &ws->sc->done, words, 4);
}

int spmv_hip_lsqr_ws_get_state(spmv_hip_lsqr_ws* ws, int32_t* host_words5,
                               void* stream)
{
  SPMV_REQUIRE(ws && host_words5);
  return ws_get_words(ws->ctx, stream, host_words5, &ws->sc->done, 5);
}

// ---- kernels ------------------------------------------------------------------
int spmv_hip_lsqr_update_u_f64(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws,
                               int64_t n, const double* Av, double* ut,
                               void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE((n == 0 || (Av && ut && Av != ut)) && aligned8(Av, ut));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_AL(ctx, n, aligned16(Av, ut), lsqr_update_u_kernel,
                    stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n,
                    ws->sc, Av, ut, ws->p_uu, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lsqr_update_v_f64(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws,
                               int64_t n, const double* Atu, double* vt,
                               int first, int reduced, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE((n == 0 || (Atu && vt && Atu != vt)) && aligned8(Atu, vt));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_AL(ctx, n, aligned16(Atu, vt), lsqr_update_v_kernel,
                    stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n,
                    ws->sc, Atu, vt, ws->p_uu, ctx->dot_blocks, first ? 1 : 0,
                    reduced ? 1 : 0, ws->p_vv);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lsqr_reduce(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws, int which,
                         void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_REQUIRE(which == SPMV_HIP_LSQR_UU || which == SPMV_HIP_LSQR_VV);
  SPMV_SET_DEVICE(ctx);
  const bool uu = which == SPMV_HIP_LSQR_UU;
  hipLaunchKernelGGL(lsqr_reduce_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, uu ? ws->p_uu : ws->p_vv,
                     ctx->dot_blocks, uu ? &ws->sc->uu : &ws->sc->vv);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lsqr_start(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws, int reduced,
                        void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(lsqr_start_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, ws->p_vv, ctx->dot_blocks,
                     reduced ? 1 : 0, ws->hist, ws->hist + ws->kmax + 1);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lsqr_step(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws, int reduced,
                       void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(lsqr_step_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, ws->p_vv, ctx->dot_blocks,
                     reduced ? 1 : 0, ws->hist, ws->hist + ws->kmax + 1);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lsqr_update_xw_f64(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws, int k,
                                int64_t n, const double* vt, double* w,
                                double* x, void* stream)
{
  SPMV_REQUIRE_WS_K(ctx, ws, k, 0);
  SPMV_REQUIRE(ctx && n >= 0);
  SPMV_REQUIRE((n == 0 || (vt && w && (k == 0 || x))) && aligned8(vt, w, x));
  SPMV_REQUIRE(n == 0 || (w != vt && w != x && x != vt));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_AL(ctx, n, aligned16(vt, w, x), lsqr_update_xw_kernel,
                    stream_grid(ctx, n), spmv_stream(ctx, stream), n, ws->sc, k,
                    vt, w, x);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
