// Ghost pack kernel and the CG loop's fused BLAS-1 kernels (gfx950).
//
// gather: DeviceExecutor::gather_ghosts_run (spmv/device_executor.h:123-126,
//         spmv/reference_executor.cpp:150-164).
// CG:     spmv::cg (spmv/cg.cpp:21-98).  Seven BLAS calls + two host
//         reductions per iteration become two streaming kernels
//           K2: x += alpha p ; r -= alpha Ap ; partial r.r      (cg.cpp:66-73)
//           K3: converged? ; p = beta p + r                     (cg.cpp:77-85)
//         plus single-workgroup reducers.  alpha, beta and the stopping test
//         are evaluated on the device from the scalar history rr[], pAp[];
//         precedent for device-resident scalars: cuda/cg.cuda.cu:14-38,73-84.
//         On one rank the x update is deferred by one iteration
//         (cg_update_p2_cs_kernel / cg_update_x2p_cs_kernel, see there): x is
//         read and written every second iteration, 9 vector passes per pair
//         on the x/p side instead of 10, same bits.  The price is a second p
//         vector in the workspace (8 N bytes: 1.07 GB at 512^3).
//
// Built with -ffp-contract=off: axpy/scal round like unfused BLAS-1.
// Streaming shape: see blas1_stream.h.
#include "common.h"
#include "blas1_stream.h"
#include "solver_ws.h"

#include <cmath>

namespace
{

// r += nalpha * Ap (cg.cpp:70), returns this thread's share of r.r (:73)
template <bool NT>
__device__ __forceinline__ double stream_update_r(int64_t n2, double nalpha,
                                                  const double* Ap, double* r)
{
  double acc = 0.0;
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
      rv[u].x += nalpha * av[u].x;
      rv[u].y += nalpha * av[u].y;
      vstore<NT>(r, i, rv[u]);
      acc += rv[u].x * rv[u].x;
      acc += rv[u].y * rv[u].y;
    }
  }
  return acc;
}

// x += alpha p (cg.cpp:69) ; r += nalpha Ap (:70) ; share of r.r (:73)
template <bool NT>
__device__ __forceinline__ double stream_update_xr(int64_t n2, double alpha,
                                                   double nalpha, const double* p,
                                                   const double* Ap, double* x,
                                                   double* r)
{
  double acc = 0.0;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 pv[kU], av[kU], xv[kU], rv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      pv[u] = vload<NT>(p, i);
      av[u] = vload<NT>(Ap, i);
      xv[u] = vload<NT>(x, i);
      rv[u] = vload<NT>(r, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      xv[u].x += alpha * pv[u].x;
      xv[u].y += alpha * pv[u].y;
      rv[u].x += nalpha * av[u].x;
      rv[u].y += nalpha * av[u].y;
      vstore<NT>(x, i, xv[u]);
      vstore<NT>(r, i, rv[u]);
      acc += rv[u].x * rv[u].x;
      acc += rv[u].y * rv[u].y;
    }
  }
  return acc;
}

// x += alpha p (cg.cpp:69) over all n doubles: what an iteration that meets
// the tolerance does to x while p stays (:80-81)
template <bool NT>
__device__ __forceinline__ void axpy_all(int64_t n, double alpha,
                                         const double* p, double* x)
{
  stream_axpy<NT>(n >> 1, alpha, p, x);
  if (odd_tail(n))
    x[n - 1] += alpha * p[n - 1];
}

// p_out = beta p_in + r (cg.cpp:84-85): in place (p_out == p_in), or into the
// OTHER p buffer while p_in stays
template <bool NT>
__device__ __forceinline__ void stream_update_p2(int64_t n2, double beta,
                                                 const double* r,
                                                 const double* p_in,
                                                 double* p_out)
{
  SPMV_FOR_UNITS(n2)
  {
    f64x2 pv[kU], rv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      pv[u] = vload<NT>(p_in, i);
      rv[u] = vload<NT>(r, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      pv[u].x = beta * pv[u].x;
      pv[u].y = beta * pv[u].y;
      pv[u].x += rv[u].x;
      pv[u].y += rv[u].y;
      vstore<NT>(p_out, i, pv[u]);
    }
  }
}

// x += alpha p (cg.cpp:69) ; p = beta p + r (:84-85)
template <bool NT>
__device__ __forceinline__ void stream_update_xp(int64_t n2, double alpha,
                                                 double beta, const double* r,
                                                 double* x, double* p)
{
  SPMV_FOR_UNITS(n2)
  {
    f64x2 pv[kU], xv[kU], rv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      pv[u] = vload<NT>(p, i);
      xv[u] = vload<NT>(x, i);
      rv[u] = vload<NT>(r, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      xv[u].x += alpha * pv[u].x;
      xv[u].y += alpha * pv[u].y;
      vstore<NT>(x, i, xv[u]);
      pv[u].x = beta * pv[u].x;
      pv[u].y = beta * pv[u].y;
      pv[u].x += rv[u].x;
      pv[u].y += rv[u].y;
      vstore<NT>(p, i, pv[u]);
    }
  }
}

// x += alpha0 p0 ; x += alpha1 p1 (cg.cpp:69 of two consecutive iterations,
// in their order) ; with UPDATE_P also p0 = beta p1 + r (:84-85), in place
// over the older direction: the lane that writes an element has read it
template <bool NT, bool UPDATE_P>
__device__ __forceinline__ void stream_update_x2p(int64_t n2, double alpha0,
                                                  double alpha1, double beta,
                                                  const double* r, double* x,
                                                  double* p0, const double* p1)
{
  SPMV_FOR_UNITS(n2)
  {
    f64x2 qv[kU], pv[kU], xv[kU], rv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      qv[u] = vload<NT>(p0, i);
      pv[u] = vload<NT>(p1, i);
      xv[u] = vload<NT>(x, i);
      if constexpr (UPDATE_P)
        rv[u] = vload<NT>(r, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      xv[u].x += alpha0 * qv[u].x;
      xv[u].y += alpha0 * qv[u].y;
      xv[u].x += alpha1 * pv[u].x;
      xv[u].y += alpha1 * pv[u].y;
      vstore<NT>(x, i, xv[u]);
      if constexpr (UPDATE_P) {
        pv[u].x = beta * pv[u].x;
        pv[u].y = beta * pv[u].y;
        pv[u].x += rv[u].x;
        pv[u].y += rv[u].y;
        vstore<NT>(p0, i, pv[u]);
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void gather_kernel(
    int n, const int32_t* __restrict__ indices, const T* __restrict__ in,
    T* __restrict__ out)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x)
    out[i] = in[indices[i]];
}

// reverse halo accumulate (spmv/L2GMap.cpp:921-922,947-948) for ONE neighbour's
// segment: indices are distinct inside a segment, so no atomics are needed
template <typename T>
__global__ __launch_bounds__(kBlock) void scatter_add_kernel(
    int n, const int32_t* __restrict__ indices, const T* __restrict__ in,
    T* __restrict__ out)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x)
    out[indices[i]] += in[i];
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void dot_partial_kernel(
    int64_t n, const double* __restrict__ x, const double* __restrict__ y,
    DotOut dot)
{
  __shared__ double s_red[kBlock / 64];
  double acc = stream_dot<NT>(n >> 1, x, y);
  if (odd_tail(n))
    acc += x[n - 1] * y[n - 1];
  spmv_dot_epilogue(dot, acc, s_red);
}

// Sum `len` partials in a fixed order with one workgroup.
__global__ __launch_bounds__(kBlock) void reduce_partials_kernel(
    const double* __restrict__ partials, int len, double* __restrict__ result,
    const int32_t* __restrict__ done)
{
  __shared__ double s_red[kBlock / 64];
  if (done && *done)
    return;
  const double s = sum_partials(partials, nullptr, len, s_red);
  if (threadIdx.x == 0)
    *result = s;
}

// ---- CG -----------------------------------------------------------------
struct CgScalars {
  double rtol;
  int32_t done;
  int32_t kstop;
};

// What the first kernel of iteration k finds about iteration k - 1: the solve
// stops there when rr[k-1] met the tolerance (cg.cpp:80-81; k >= 2).  Uniform
// across the grid: every thread reads the same words.
__device__ __forceinline__ bool stopped_before(const double* __restrict__ rr,
                                               int k,
                                               const CgScalars* __restrict__ sc)
{
  if (k >= 2) {
    const double rnorm0 = sqrt(rr[0]);
    const double rnorm_prev = sqrt(rr[k - 1]);
    if (rnorm_prev / rnorm0 < sc->rtol)
      return true;
  }
  return false;
}

// alpha, beta and the stopping test of iteration k from its scalars
struct CgStep {
  double alpha, beta;
  bool converged;
};
__device__ __forceinline__ CgStep cg_step(double rr0, double rr_old,
                                          double rr_new, double pap, double rtol)
{
  const double rnorm0 = sqrt(rr0);
  const double rnorm_old = sqrt(rr_old);
  const double rnorm_new = sqrt(rr_new);                           // cg.cpp:76
  CgStep s;
  s.alpha = (rnorm_old * rnorm_old) / pap;                         // :66
  s.beta = (rnorm_new * rnorm_new) / (rnorm_old * rnorm_old);      // :77
  s.converged = rnorm_new / rnorm0 < rtol;                         // :80
  return s;
}

// alpha of iteration k (cg.cpp:50,76 ; :66)
__device__ __forceinline__ double cg_alpha(double rr_old, double pap)
{
  const double rnorm_old = sqrt(rr_old);
  return (rnorm_old * rnorm_old) / pap;
}

// x += alpha p ; r += (-alpha) Ap ; partial r.r
template <bool NT>
__global__ __launch_bounds__(kBlock) void cg_update_xr_kernel(
    int64_t n, const double* __restrict__ rr_prev,
    const double* __restrict__ pAp, const CgScalars* __restrict__ sc,
    const double* __restrict__ p, const double* __restrict__ Ap,
    double* __restrict__ x, double* __restrict__ r,
    double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double alpha = cg_alpha(*rr_prev, *pAp);
  const double nalpha = -alpha;
  double acc = stream_update_xr<NT>(n >> 1, alpha, nalpha, p, Ap, x, r);
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    x[i] += alpha * p[i];
    double rv = r[i] + nalpha * Ap[i];
    r[i] = rv;
    acc += rv * rv;
  }
  spmv_dot_epilogue(DotOut{partials, len}, acc, s_red);
}

// stopping test on rr[k], then p = beta p + r
template <bool NT>
__global__ __launch_bounds__(kBlock) void cg_update_p_kernel(
    int64_t n, int k, const double* __restrict__ rr0,
    const double* __restrict__ rr_prev, const double* __restrict__ rr_new,
    CgScalars* __restrict__ sc, const double* __restrict__ r,
    double* __restrict__ p)
{
  if (sc->done)
    return;
  const double rnorm0 = sqrt(*rr0);
  const double rnorm_old = sqrt(*rr_prev);
  const double rnorm_new = sqrt(*rr_new);                           // cg.cpp:76
  const double beta = (rnorm_new * rnorm_new) / (rnorm_old * rnorm_old); // :77
  if (rnorm_new / rnorm0 < sc->rtol)                                // :80
    return; // p is left untouched (:81); cg_reduce_pAp_kernel raises `done`
  stream_update_p2<NT>(n >> 1, beta, r, p, p);
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    p[i] = beta * p[i] + r[i];
  }
}

// ---- the same two updates, regrouped so that p is read once ---------------
// K2': r += (-alpha) Ap ; partial r.r                  (cg.cpp:66,70,73)
// K3': x += alpha p ; stop test ; p = beta p + r        (cg.cpp:69,77-85)
// Element-wise arithmetic and its order per element are unchanged; only the
// kernel an update lives in differs (8 instead of 9 vector passes).  x is
// still updated in the iteration that converges and p is not (cg.cpp:80-81).

// body of update_r / update_r_cs behind their prologues
template <bool NT>
__device__ __forceinline__ void update_r_body(int64_t n, double nalpha,
                                              const double* __restrict__ Ap,
                                              double* __restrict__ r,
                                              double* __restrict__ partials,
                                              int len, double* s_red)
{
  double acc = stream_update_r<NT>(n >> 1, nalpha, Ap, r);
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    double rv = r[i] + nalpha * Ap[i];
    r[i] = rv;
    acc += rv * rv;
  }
  spmv_dot_epilogue(DotOut{partials, len}, acc, s_red);
}

// body of update_xp / update_xp_cs: rr_new is iteration k's
template <bool NT>
__device__ __forceinline__ void update_xp_body(
    int64_t n, double rr0, double rr_old, double rr_new, double pap,
    double rtol, const double* __restrict__ r, double* __restrict__ x,
    double* __restrict__ p)
{
  const CgStep s = cg_step(rr0, rr_old, rr_new, pap, rtol);
  if (s.converged) { // x takes this iteration's update, p stays (:80-81)
    axpy_all<NT>(n, s.alpha, p, x);
    return;
  }
  stream_update_xp<NT>(n >> 1, s.alpha, s.beta, r, x, p);
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    x[i] += s.alpha * p[i];
    p[i] = s.beta * p[i] + r[i];
  }
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void cg_update_r_kernel(
    int64_t n, const double* __restrict__ rr_prev,
    const double* __restrict__ pAp, const CgScalars* __restrict__ sc,
    const double* __restrict__ Ap, double* __restrict__ r,
    double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  update_r_body<NT>(n, -cg_alpha(*rr_prev, *pAp), Ap, r, partials, len, s_red);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void cg_update_xp_kernel(
    int64_t n, int k, const double* __restrict__ rr0,
    const double* __restrict__ rr_prev, const double* __restrict__ rr_new,
    const double* __restrict__ pAp, CgScalars* __restrict__ sc,
    const double* __restrict__ r, double* __restrict__ x,
    double* __restrict__ p)
{
  if (sc->done)
    return;
  update_xp_body<NT>(n, *rr0, *rr_prev, *rr_new, *pAp, sc->rtol, r, x, p);
}

// Reduces the p.Ap partials of iteration k.  It is the first single-workgroup
// kernel after the p-update of iteration k-1, so it also raises `done` when
// rr[k-1] met the tolerance (see stopped_before): every later cg_* kernel then
// returns at once and x, r, p keep their iteration-(k-1) values.  In-order
// stream execution makes the flag visible to the following launches.
__global__ __launch_bounds__(kBlock) void cg_reduce_pAp_kernel(
    const double* __restrict__ partials, const double* __restrict__ partials2,
    int len, int k,
    const double* __restrict__ rr, double* __restrict__ pAp,
    CgScalars* __restrict__ sc)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  if (stopped_before(rr, k, sc)) { // uniform across the workgroup
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

// ---- consumer-side reductions (one rank) -----------------------------------
// Instead of a single-workgroup reducer launch between producer and consumer,
// EVERY workgroup of the consuming kernel adds the <= 2048 partials itself, in
// the reducers' order (consume_partials: same loop, same tree => the same
// bits), and workgroup 0 records the value in the history.  16 KB of
// L2-resident reads per workgroup against two kernel launches per iteration:
// what a small problem spends most of its iteration on.  Needs the scalar on
// this rank only, so it is used when the communicator has one rank.

// cg_reduce_pAp_kernel + cg_update_r_kernel in one launch
template <bool NT>
__global__ __launch_bounds__(kBlock) void cg_update_r_cs_kernel(
    int64_t n, int k, const double* __restrict__ rr, double* __restrict__ pAp,
    CgScalars* __restrict__ sc, const double* __restrict__ pap_partials,
    const double* __restrict__ pap_partials2, int len,
    const double* __restrict__ Ap, double* __restrict__ r,
    double* __restrict__ rr_partials)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  if (stopped_before(rr, k, sc)) { // uniform across the grid
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
  update_r_body<NT>(n, -cg_alpha(rr[k - 1], pap), Ap, r, rr_partials, len,
                    s_red);
}

// reduce_partials_kernel (r.r) + cg_update_xp_kernel in one launch
template <bool NT>
__global__ __launch_bounds__(kBlock) void cg_update_xp_cs_kernel(
    int64_t n, int k, double* __restrict__ rr, const double* __restrict__ pAp,
    CgScalars* __restrict__ sc, const double* __restrict__ rr_partials, int len,
    const double* __restrict__ r, double* __restrict__ x, double* __restrict__ p)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  const double rr_new
      = consume_partials(rr_partials, nullptr, len, s_red, &s_bcast);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    rr[k] = rr_new;
  update_xp_body<NT>(n, rr[0], rr[k - 1], rr_new, pAp[k], sc->rtol, r, x, p);
}

// ---- the x update deferred by one iteration (one rank, CgOptions::defer_x) --
// Nothing inside an iteration reads x, so cg_update_xp_cs_kernel's pass over
// it is spent twice per pair of iterations for one accumulation each.  With p
// kept in two buffers that swap, a pair becomes
//   P   (iteration k):   rr[k]; stop test; p_out = beta p_in + r     3 passes
//   X2P (iteration k+1): rr[k+1]; x += a_k p_prev; x += a_k+1 p_cur;
//                        stop test; p_prev = beta p_cur + r          6 passes
// instead of 2 x 5.  Every multiply and add of an element is the one of
// cg_update_xp_cs_kernel, in its order, and a_k is recomputed from the history
// with the same expression: x, p, r and the scalars keep their bits.
// An iteration that meets the tolerance applies whatever x update is pending
// and leaves p alone, as before (:80-81); a loop that ends on a P step is
// closed by cg_flush_x_kernel.

// P step: reduce_partials_kernel (r.r) + stop test + p update, x deferred
template <bool NT>
__global__ __launch_bounds__(kBlock) void cg_update_p2_cs_kernel(
    int64_t n, int k, double* __restrict__ rr, const double* __restrict__ pAp,
    CgScalars* __restrict__ sc, const double* __restrict__ rr_partials, int len,
    const double* __restrict__ r, double* __restrict__ x,
    const double* __restrict__ p_in, double* __restrict__ p_out)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  const double rr_new
      = consume_partials(rr_partials, nullptr, len, s_red, &s_bcast);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    rr[k] = rr_new;
  const CgStep s = cg_step(rr[0], rr[k - 1], rr_new, pAp[k], sc->rtol);
  if (s.converged) { // x takes this iteration's update now, p stays (:80-81)
    axpy_all<NT>(n, s.alpha, p_in, x);
    return;
  }
  stream_update_p2<NT>(n >> 1, s.beta, r, p_in, p_out);
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    p_out[i] = s.beta * p_in[i] + r[i];
  }
}

// X2P step (k >= 2): the x updates of iterations k-1 and k, then the p update
template <bool NT>
__global__ __launch_bounds__(kBlock) void cg_update_x2p_cs_kernel(
    int64_t n, int k, double* __restrict__ rr, const double* __restrict__ pAp,
    CgScalars* __restrict__ sc, const double* __restrict__ rr_partials, int len,
    const double* __restrict__ r, double* __restrict__ x,
    double* __restrict__ p_prev, const double* __restrict__ p_cur)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  const double rr_new
      = consume_partials(rr_partials, nullptr, len, s_red, &s_bcast);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    rr[k] = rr_new;
  const double alpha_prev = cg_alpha(rr[k - 2], pAp[k - 1]); // :66, k-1
  const CgStep s = cg_step(rr[0], rr[k - 1], rr_new, pAp[k], sc->rtol);
  const bool tail = odd_tail(n);
  const int64_t i = n - 1;
  if (s.converged) { // x takes both updates, p stays (:80-81)
    stream_update_x2p<NT, false>(n >> 1, alpha_prev, s.alpha, s.beta, r, x,
                                 p_prev, p_cur);
    if (tail) {
      x[i] += alpha_prev * p_prev[i];
      x[i] += s.alpha * p_cur[i];
    }
    return;
  }
  stream_update_x2p<NT, true>(n >> 1, alpha_prev, s.alpha, s.beta, r, x, p_prev,
                              p_cur);
  if (tail) {
    x[i] += alpha_prev * p_prev[i];
    x[i] += s.alpha * p_cur[i];
    p_prev[i] = s.beta * p_cur[i] + r[i];
  }
}

// After a loop whose last iteration k was a P step: x += a_k p_k, unless the
// solve has stopped (`done`) or iteration k itself met the tolerance -- then
// the P step's converged branch has applied it, and `done` is only raised by
// the next iteration's r kernel, which never ran.
template <bool NT>
__global__ __launch_bounds__(kBlock) void cg_flush_x_kernel(
    int64_t n, int k, const double* __restrict__ rr,
    const double* __restrict__ pAp, const CgScalars* __restrict__ sc,
    const double* __restrict__ p, double* __restrict__ x)
{
  if (sc->done)
    return;
  const double rnorm0 = sqrt(rr[0]);
  const double rnorm_old = sqrt(rr[k - 1]);
  const double rnorm_new = sqrt(rr[k]);
  if (rnorm_new / rnorm0 < sc->rtol) // :80, as cg_update_p2_cs_kernel
    return;
  const double alpha = (rnorm_old * rnorm_old) / pAp[k]; // :66
  axpy_all<NT>(n, alpha, p, x);
}

// CG start (cg.cpp:39-50) in one pass over b: r = p = b, x0 = 0 (defined here
// instead of relying on fresh pages) and the partials of r.r.
template <bool NT>
__global__ __launch_bounds__(kBlock) void cg_init_kernel(
    int64_t n, const double* __restrict__ b, double* __restrict__ r,
    double* __restrict__ p, double* __restrict__ x,
    double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = b[i];
    sstore<NT>(&r[i], v);
    sstore<NT>(&p[i], v);
    sstore<NT>(&x[i], 0.0);
    acc += v * v;
  }
  spmv_dot_epilogue(DotOut{partials, len}, acc, s_red);
}

// ---- mixed-precision CG support -----------------------------
// out = (float) in
__global__ __launch_bounds__(kBlock) void convert_f64_f32_kernel(
    int64_t n, const double* __restrict__ in, float* __restrict__ out)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (float)in[i];
}

// y += a x
__global__ __launch_bounds__(kBlock) void axpy_kernel(
    int64_t n, double a, const double* __restrict__ x, double* __restrict__ y)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    y[i] += a * x[i];
}

// residual replacement: r = b - Ax (Ax given), partials of r.r.  Inside the
// CG loop it is a no-op once `done` is raised, like every other cg_* kernel;
// the closing check after the loop passes sc = nullptr.
__global__ __launch_bounds__(kBlock) void cg_residual_kernel(
    int64_t n, const CgScalars* __restrict__ sc, const double* __restrict__ b,
    const double* __restrict__ Ax, double* __restrict__ r,
    double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc && sc->done)
    return;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double rv = b[i] - Ax[i];
    r[i] = rv;
    acc += rv * rv;
  }
  spmv_dot_epilogue(DotOut{partials, len}, acc, s_red);
}

__global__ void cg_reset_kernel(CgScalars* sc, double rtol, double* rr,
                                double* pAp, int kmax)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    sc->rtol = rtol;
    sc->done = 0;
    sc->kstop = -1;
  }
  if (i <= kmax) {
    rr[i] = 0.0;
    pAp[i] = 0.0;
  }
}

__global__ __launch_bounds__(kBlock) void fill_gaussian_kernel(
    int64_t N, int64_t i_begin, int64_t count, double* __restrict__ x)
{
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count;
       k += (int64_t)gridDim.x * blockDim.x) {
    const double z = (double)(k + i_begin) / (double)N; // demos/spmv.cpp:65
    const double u = 5 * (z - 0.5);
    x[k] = exp(-10 * (u * u)); // pow(u, 2.0) == u*u exactly
  }
}

__global__ __launch_bounds__(kBlock) void fill_const_kernel(
    int64_t count, double value, double* __restrict__ x)
{
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count;
       k += (int64_t)gridDim.x * blockDim.x)
    x[k] = value;
}

// the four index kernels' entry points: gather / scatter_add, f64 / f32
template <typename T>
int launch_indexed(void (*kernel)(int, const int32_t*, const T*, T*),
                   spmv_hip_ctx* ctx, int num_indices, const int32_t* indices,
                   const T* in, T* out, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(num_indices >= 0);
  if (num_indices == 0)
    return SPMV_HIP_OK;
  SPMV_REQUIRE(indices && in && out);
  const int grid = spmv_grid_for(ctx, num_indices, kBlock);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), num_indices, indices, in, out);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // namespace

struct spmv_hip_cg_ws {
  spmv_hip_ctx* ctx = nullptr;
  int kmax = 0;
  SolverArrays own;
  double* rr = nullptr;       // kmax + 1
  double* pAp = nullptr;      // kmax + 1
  double* partials = nullptr; // ctx->dot_blocks
  double* partials_rr = nullptr; // ctx->dot_blocks (consumer-side reductions)
  CgScalars* sc = nullptr;
};

extern "C" {

int spmv_hip_gather_f64(spmv_hip_ctx* ctx, int num_indices,
                        const int32_t* indices, const double* in, double* out,
                        void* stream)
{
  return launch_indexed(gather_kernel<double>, ctx, num_indices, indices, in,
                        out, stream);
}

int spmv_hip_scatter_add_f64(spmv_hip_ctx* ctx, int num_indices,
                             const int32_t* indices, const double* in,
                             double* out, void* stream)
{
  return launch_indexed(scatter_add_kernel<double>, ctx, num_indices, indices,
                        in, out, stream);
}

int spmv_hip_scatter_add_f32(spmv_hip_ctx* ctx, int num_indices,
                             const int32_t* indices, const float* in,
                             float* out, void* stream)
{
  return launch_indexed(scatter_add_kernel<float>, ctx, num_indices, indices,
                        in, out, stream);
}

int spmv_hip_gather_f32(spmv_hip_ctx* ctx, int num_indices,
                        const int32_t* indices, const float* in, float* out,
                        void* stream)
{
  return launch_indexed(gather_kernel<float>, ctx, num_indices, indices, in,
                        out, stream);
}

int spmv_hip_dot_partials_len(const spmv_hip_ctx* ctx, int* len)
{
  SPMV_REQUIRE(ctx && len);
  *len = ctx->dot_blocks;
  return SPMV_HIP_OK;
}

int spmv_hip_dot_partial_f64(spmv_hip_ctx* ctx, int64_t n, const double* x,
                             const double* y, double* partials, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(n >= 0 && partials && (n == 0 || (x && y)));
  SPMV_REQUIRE(aligned16(x, y));
  DotOut dot;
  dot.partials = partials;
  dot.len = ctx->dot_blocks;
  SPMV_LAUNCH_NT(ctx, n, dot_partial_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, x, y, dot);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_init_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int64_t n,
                         const double* b, double* r, double* p, double* x,
                         void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(ws && ws->ctx == ctx && n >= 0 && (n == 0 || (b && r && p && x)));
  int grid = spmv_grid_for(ctx, n, kBlock);
  if (grid > ctx->dot_blocks)
    grid = ctx->dot_blocks;
  SPMV_LAUNCH_NT(ctx, n, cg_init_kernel, grid, spmv_stream(ctx, stream), n, b,
                 r, p, x, ws->partials, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_convert_f64_f32(spmv_hip_ctx* ctx, int64_t n, const double* in,
                             float* out, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (in && out)));
  if (n == 0)
    return SPMV_HIP_OK;
  const int grid = spmv_grid_for(ctx, n, kBlock);
  hipLaunchKernelGGL(convert_f64_f32_kernel, dim3(grid), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), n, in, out);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_axpy_f64(spmv_hip_ctx* ctx, int64_t n, double a, const double* x,
                      double* y, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (x && y)));
  if (n == 0)
    return SPMV_HIP_OK;
  const int grid = spmv_grid_for(ctx, n, kBlock);
  hipLaunchKernelGGL(axpy_kernel, dim3(grid), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), n, a, x, y);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_residual_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws,
                             int respect_done, int64_t n, const double* b,
                             const double* Ax, double* r, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(ws && ws->ctx == ctx && n >= 0 && (n == 0 || (b && Ax && r)));
  int grid = spmv_grid_for(ctx, n, kBlock);
  if (grid > ctx->dot_blocks)
    grid = ctx->dot_blocks;
  hipLaunchKernelGGL(cg_residual_kernel, dim3(grid), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), n,
                     respect_done ? ws->sc : (const CgScalars*)nullptr, b, Ax, r,
                     ws->partials, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_reduce_partials_f64(spmv_hip_ctx* ctx, const double* partials,
                                 double* result, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(partials && result);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), partials, ctx->dot_blocks,
                     result, (const int32_t*)nullptr);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

// ---- CG workspace -------------------------------------------------------------
int spmv_hip_cg_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_cg_ws** out)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(out && kmax >= 0);
  return solver_ws_create(ctx, kmax, out, [&](spmv_hip_cg_ws& w) {
    w.own.alloc(w.rr, (size_t)kmax + 1);
    w.own.alloc(w.pAp, (size_t)kmax + 1);
    w.own.alloc(w.partials, ctx->dot_blocks);
    w.own.alloc(w.partials_rr, ctx->dot_blocks);
    w.own.alloc(w.sc, 1);
  });
}

int spmv_hip_cg_ws_destroy(spmv_hip_cg_ws* ws)
{
  return solver_ws_destroy(ws);
}

int spmv_hip_cg_ws_reset(spmv_hip_cg_ws* ws, double rtol, void* stream)
{
  SPMV_REQUIRE(ws);
  SPMV_SET_DEVICE(ws->ctx);
  const int n = ws->kmax + 1;
  hipLaunchKernelGGL(cg_reset_kernel, ws_reset_grid(n), dim3(kBlock), 0,
                     spmv_stream(ws->ctx, stream), ws->sc, rtol, ws->rr,
                     ws->pAp, ws->kmax);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_ws_rr(spmv_hip_cg_ws* ws, int k, double** slot)
{
  SPMV_REQUIRE(ws && slot && k >= 0 && k <= ws->kmax);
  *slot = ws->rr + k;
  return SPMV_HIP_OK;
}

int spmv_hip_cg_ws_pAp(spmv_hip_cg_ws* ws, int k, double** slot)
{
  SPMV_REQUIRE(ws && slot && k >= 0 && k <= ws->kmax);
  *slot = ws->pAp + k;
  return SPMV_HIP_OK;
}

int spmv_hip_cg_ws_partials(spmv_hip_cg_ws* ws, double** partials)
{
  SPMV_REQUIRE(ws && partials);
  *partials = ws->partials;
  return SPMV_HIP_OK;
}

int spmv_hip_cg_ws_done_flag(spmv_hip_cg_ws* ws, const int32_t** done)
{
  SPMV_REQUIRE(ws && done);
  *done = &ws->sc->done;
  return SPMV_HIP_OK;
}

int spmv_hip_cg_ws_capacity(const spmv_hip_cg_ws* ws, int* kmax)
{
  return solver_ws_capacity(ws, kmax);
}

int spmv_hip_cg_ws_read_async(spmv_hip_cg_ws* ws, int32_t* host_done_kstop,
                              double* host_rr, size_t host_rr_len, void* stream)
{
  SPMV_REQUIRE(ws);
  return ws_read_async(ws->ctx, stream, host_done_kstop, &ws->sc->done, 2,
                       host_rr, host_rr_len, ws->rr, (size_t)ws->kmax + 1);
}

int spmv_hip_cg_dot_rr_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int64_t n,
                           const double* r, void* stream)
{
  SPMV_REQUIRE(ws && ws->ctx == ctx);
  return spmv_hip_dot_partial_f64(ctx, n, r, r, ws->partials, stream);
}

int spmv_hip_cg_reduce_rr(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                          void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 0);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->partials, ctx->dot_blocks,
                     ws->rr + k, &ws->sc->done);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_reduce_pAp(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                           void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  hipLaunchKernelGGL(cg_reduce_pAp_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->partials,
                     (const double*)nullptr, ctx->dot_blocks, k, ws->rr,
                     ws->pAp, ws->sc);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_reduce_pAp2(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                            const double* partials2, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(partials2);
  hipLaunchKernelGGL(cg_reduce_pAp_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->partials, partials2,
                     ctx->dot_blocks, k, ws->rr, ws->pAp, ws->sc);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_update_xr_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                              int64_t n, const double* p, const double* Ap,
                              double* x, double* r, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (p && Ap && x && r)));
  SPMV_REQUIRE(aligned16(p, Ap, x, r));
  SPMV_LAUNCH_NT(ctx, n, cg_update_xr_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, ws->rr + (k - 1), ws->pAp + k,
                 ws->sc, p, Ap, x, r, ws->partials, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_update_p_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                             int64_t n, const double* r, double* p,
                             void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (r && p)));
  SPMV_REQUIRE(aligned16(r, p));
  SPMV_LAUNCH_NT(ctx, n, cg_update_p_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, k, ws->rr, ws->rr + (k - 1),
                 ws->rr + k, ws->sc, r, p);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                             int64_t n, const double* Ap, double* r,
                             void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (Ap && r)));
  SPMV_REQUIRE(aligned16(Ap, r));
  SPMV_LAUNCH_NT(ctx, n, cg_update_r_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, ws->rr + (k - 1), ws->pAp + k,
                 ws->sc, Ap, r, ws->partials, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                              int64_t n, const double* r, double* x, double* p,
                              void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (r && x && p)));
  SPMV_REQUIRE(aligned16(r, x, p));
  SPMV_LAUNCH_NT(ctx, n, cg_update_xp_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, k, ws->rr, ws->rr + (k - 1),
                 ws->rr + k, ws->pAp + k, ws->sc, r, x, p);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_update_r_cs_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                                int64_t n, const double* Ap, double* r,
                                const double* pap_partials2, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (Ap && r)));
  SPMV_REQUIRE(aligned16(Ap, r));
  SPMV_LAUNCH_NT(ctx, n, cg_update_r_cs_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, k, ws->rr, ws->pAp, ws->sc,
                 ws->partials, pap_partials2, ctx->dot_blocks, Ap, r,
                 ws->partials_rr);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_update_xp_cs_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                                 int64_t n, const double* r, double* x,
                                 double* p, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (r && x && p)));
  SPMV_REQUIRE(aligned16(r, x, p));
  SPMV_LAUNCH_NT(ctx, n, cg_update_xp_cs_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, k, ws->rr, ws->pAp, ws->sc,
                 ws->partials_rr, ctx->dot_blocks, r, x, p);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_update_p2_cs_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                                 int64_t n, const double* r, double* x,
                                 const double* p_in, double* p_out,
                                 void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (r && x && p_in && p_out && p_in !=
               p_out)));
  SPMV_REQUIRE(aligned16(r, x, p_in, p_out));
  SPMV_LAUNCH_NT(ctx, n, cg_update_p2_cs_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, k, ws->rr, ws->pAp, ws->sc,
                 ws->partials_rr, ctx->dot_blocks, r, x, p_in, p_out);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_update_x2p_cs_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                                  int64_t n, const double* r, double* x,
                                  double* p_prev, const double* p_cur,
                                  void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 2);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (r && x && p_prev && p_cur && p_prev !=
               p_cur)));
  SPMV_REQUIRE(aligned16(r, x, p_prev, p_cur));
  SPMV_LAUNCH_NT(ctx, n, cg_update_x2p_cs_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, k, ws->rr, ws->pAp, ws->sc,
                 ws->partials_rr, ctx->dot_blocks, r, x, p_prev, p_cur);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cg_flush_x_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                            int64_t n, const double* p, double* x,
                            void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (p && x)));
  SPMV_REQUIRE(aligned16(p, x));
  SPMV_LAUNCH_NT(ctx, n, cg_flush_x_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, k, ws->rr, ws->pAp, ws->sc, p, x);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_fill_gaussian_f64(spmv_hip_ctx* ctx, int64_t N, int64_t i_begin,
                               int64_t count, double* x, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(N > 0 && i_begin >= 0 && count >= 0);
  if (count == 0)
    return SPMV_HIP_OK;
  SPMV_REQUIRE(x);
  const int grid = spmv_grid_for(ctx, count, kBlock);
  hipLaunchKernelGGL(fill_gaussian_kernel, dim3(grid), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), N, i_begin, count, x);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_fill_const_f64(spmv_hip_ctx* ctx, int64_t count, double value,
                            double* x, void* stream)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_REQUIRE(count >= 0);
  if (count == 0)
    return SPMV_HIP_OK;
  SPMV_REQUIRE(x);
  const int grid = spmv_grid_for(ctx, count, kBlock);
  hipLaunchKernelGGL(fill_const_kernel, dim3(grid), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), count, value, x);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
