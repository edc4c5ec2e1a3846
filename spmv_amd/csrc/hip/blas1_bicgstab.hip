// BLAS-1 kernels of spmv::bicgstab (gfx950): BiCGStab for nonsymmetric systems
// with an optional diagonal right preconditioner, given as the vector dinv of
// its inverse, in the launch structure of blas1.hip / blas1_pcg.hip.  From
// x0 = 0, with `.` the global dot product and ph = dinv*p, sh = dinv*s
// (elementwise; p and s themselves without dinv):
//
//   init          r = rhat = p = b ; ph = dinv*b ; x = 0 ; partials of b.b
//                 (rho[0] = rr[0])
//   dot_rv        partials of rhat.v                      (v = A ph)
//   reduce_rv     partials -> rv[k]
//   update_s      breakdown 1 when rv[k] == 0 (raises `done`, nothing written)
//                 alpha = rho[k-1] / rv[k] ; s = r - alpha v ; sh = dinv*s
//   dot_ts_tt     partials of t.s and t.t                 (t = A sh)
//   reduce_ts_tt  partials -> {ts[k], tt[k]}, one pair (one all-reduce of 2)
//   update_xr     omega = tt == 0 ? 0 : ts / tt ; x += alpha ph ; x += omega sh
//                 r = s - omega t ; partials of r.r and rhat.r
//   reduce_rr_rho partials -> {rr[k], rho[k]}, one pair
//   update_p      stop: sqrt(rr[k]) / sqrt(rr[0]) < rtol ; breakdown 2 when
//                 omega == 0 or rho[k] == 0 (both raise `done`, p stays)
//                 beta = (rho[k] / rho[k-1]) * (alpha / omega)
//                 p = r + beta (p - omega v) ; ph = dinv*p
//   update_s_cs / update_xr_cs / update_p_cs   the same three with the reducers
//                 folded into their prologues (one rank), as in blas1.hip
//
// Vector passes per iteration beside the two SpMVs, with dinv: 23 (dot_rv 2,
// update_s 5, dot_ts_tt 2, update_xr 8, update_p 6); without: 18 (2, 3, 2, 7,
// 4) -- `PRE` is a template flag, not a vector of ones: no multiply, no dinv
// stream, and ph / sh are p / s.
//
// `done` is raised by the kernel that takes the decision (update_s, update_p):
// every workgroup reads the same scalars and decides alike, workgroup 0 writes
// the flag, and a workgroup that starts late enough to see it returns like the
// others -- on those paths nothing else is written.  After `done` every kernel
// here returns at once.  A system with rr[0] == 0 stops at k = 0 with x = 0.
//
// Built with -ffp-contract=off: every product and sum above is a rounding of
// its own.  Streaming shape: see blas1_stream.h (persistent grid, units of
// kU 16-byte loads per lane and stream, non-temporal from blas1_nt_min_elems
// doubles on).
#include "common.h"
#include "blas1_stream.h"
#include "solver_ws.h"

#include <cmath>

struct BicgScalars {
  double rtol;
  int32_t done;
  int32_t kstop;
  int32_t status; // 0 converged (or running), 1 / 2 the breakdowns
  int32_t pad;
};

struct spmv_hip_bicg_ws {
  spmv_hip_ctx* ctx = nullptr;
  int kmax = 0;
  SolverArrays own;
  double* rv = nullptr;   // kmax + 1: rhat.v
  double* tstt = nullptr; // [kmax + 1][2]: {ts[k], tt[k]}
  double* rrho = nullptr; // [kmax + 1][2]: {rr[k], rho[k]}
  // one array per dot product, ctx->dot_blocks each: a consumer-side kernel
  // reads one pair while it fills the next
  double* p_rv = nullptr;
  double* p_ts = nullptr;
  double* p_tt = nullptr;
  double* p_rr = nullptr;
  double* p_rho = nullptr;
  BicgScalars* sc = nullptr;
};

namespace
{

// the scalars of an iteration, formed alike wherever they are needed
__device__ __forceinline__ double omega_of(double ts, double tt)
{
  return tt == 0.0 ? 0.0 : ts / tt;
}

// the solve ends: kstop iterations completed (uniform across the grid, see
// the head of this file; only workgroup 0 writes)
__device__ __forceinline__ void raise_done(BicgScalars* sc, int kstop,
                                           int status)
{
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    sc->kstop = kstop;
    sc->status = status;
    sc->done = 1;
  }
}

// ---- bodies behind the prologues --------------------------------------------
// update_s / update_s_cs: rvk = rv[k]
template <bool NT, bool PRE>
__device__ __forceinline__ void update_s_body(int64_t n, int k, double rvk,
                                              const double* rrho,
                                              BicgScalars* sc, const double* r,
                                              const double* v,
                                              const double* dinv, double* s,
                                              double* sh)
{
  const double rr0 = rrho[0];
  if (rr0 == 0.0) { // b == 0 (k == 1): x = 0 is the answer
    raise_done(sc, 0, 0);
    return;
  }
  if (rvk == 0.0) { // breakdown 1: no alpha
    raise_done(sc, k - 1, 1);
    return;
  }
  const double alpha = rrho[2 * (k - 1) + 1] / rvk;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 rv[kU], vv[kU], dv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      rv[u] = vload<NT>(r, i);
      vv[u] = vload<NT>(v, i);
      if constexpr (PRE)
        dv[u] = vload<NT>(dinv, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      f64x2 sv;
      sv.x = rv[u].x - alpha * vv[u].x;
      sv.y = rv[u].y - alpha * vv[u].y;
      vstore<NT>(s, i, sv);
      if constexpr (PRE) {
        f64x2 hv;
        hv.x = dv[u].x * sv.x;
        hv.y = dv[u].y * sv.y;
        vstore<NT>(sh, i, hv);
      }
    }
  }
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    const double sv = r[i] - alpha * v[i];
    s[i] = sv;
    if constexpr (PRE)
      sh[i] = dinv[i] * sv;
  }
}

// update_xr / update_xr_cs: ts, tt are iteration k's; without PRE ph is p and
// sh is not read (it is s)
template <bool NT, bool PRE>
__device__ __forceinline__ void update_xr_body(
    int64_t n, double alpha, double ts, double tt, const double* ph,
    const double* sh, const double* s, const double* t, const double* rhat,
    double* x, double* r, double* partials_rr, double* partials_rho, int len,
    double* s_red)
{
  const double omega = omega_of(ts, tt);
  double acc_rr = 0.0, acc_rho = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 xv[kU], pv[kU], hv[kU], sv[kU], tv[kU], qv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      xv[u] = vload<NT>(x, i);
      pv[u] = vload<NT>(ph, i);
      sv[u] = vload<NT>(s, i);
      if constexpr (PRE)
        hv[u] = vload<NT>(sh, i);
      tv[u] = vload<NT>(t, i);
      qv[u] = vload<NT>(rhat, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      if constexpr (!PRE)
        hv[u] = sv[u];
      xv[u].x += alpha * pv[u].x;
      xv[u].y += alpha * pv[u].y;
      xv[u].x += omega * hv[u].x;
      xv[u].y += omega * hv[u].y;
      vstore<NT>(x, i, xv[u]);
      f64x2 rv;
      rv.x = sv[u].x - omega * tv[u].x;
      rv.y = sv[u].y - omega * tv[u].y;
      vstore<NT>(r, i, rv);
      acc_rr += rv.x * rv.x;
      acc_rr += rv.y * rv.y;
      acc_rho += qv[u].x * rv.x;
      acc_rho += qv[u].y * rv.y;
    }
  }
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    const double sv = s[i];
    const double hv = PRE ? sh[i] : sv;
    double xv = x[i];
    xv += alpha * ph[i];
    xv += omega * hv;
    x[i] = xv;
    const double rv = sv - omega * t[i];
    r[i] = rv;
    acc_rr += rv * rv;
    acc_rho += rhat[i] * rv;
  }
  store_pair_partials(acc_rr, acc_rho, partials_rr, partials_rho, len, s_red);
}

// update_p / update_p_cs: rr_k, rho_k are iteration k's
template <bool NT, bool PRE>
__device__ __forceinline__ void update_p_body(
    int64_t n, int k, double rr_k, double rho_k, const double* rrho,
    const double* rvh, const double* tstt, BicgScalars* sc, const double* r,
    const double* v, const double* dinv, double* p, double* ph)
{
  if (sqrt(rr_k) / sqrt(rrho[0]) < sc->rtol) { // x and r updated, p not
    raise_done(sc, k, 0);
    return;
  }
  const double rho_prev = rrho[2 * (k - 1) + 1];
  const double alpha = rho_prev / rvh[k];
  const double omega = omega_of(tstt[2 * k], tstt[2 * k + 1]);
  if (omega == 0.0 || rho_k == 0.0) { // breakdown 2: no beta
    raise_done(sc, k, 2);
    return;
  }
  const double beta = (rho_k / rho_prev) * (alpha / omega);
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 rv[kU], pv[kU], vv[kU], dv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      rv[u] = vload<NT>(r, i);
      pv[u] = vload<NT>(p, i);
      vv[u] = vload<NT>(v, i);
      if constexpr (PRE)
        dv[u] = vload<NT>(dinv, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      f64x2 w;
      w.x = pv[u].x - omega * vv[u].x;
      w.y = pv[u].y - omega * vv[u].y;
      w.x = rv[u].x + beta * w.x;
      w.y = rv[u].y + beta * w.y;
      vstore<NT>(p, i, w);
      if constexpr (PRE) {
        f64x2 hv;
        hv.x = dv[u].x * w.x;
        hv.y = dv[u].y * w.y;
        vstore<NT>(ph, i, hv);
      }
    }
  }
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    double w = p[i] - omega * v[i];
    w = r[i] + beta * w;
    p[i] = w;
    if constexpr (PRE)
      ph[i] = dinv[i] * w;
  }
}

// ---- kernels ------------------------------------------------------------------
// Start in one pass over b (b and dinv need no alignment here): r = rhat = p =
// b, ph = dinv*b, x0 = 0; rho[0] = rr[0] = b.b, so both partial arrays of the
// pair take the same sums.
template <bool NT, bool PRE>
__global__ __launch_bounds__(kBlock) void bicg_init_kernel(
    int64_t n, const double* __restrict__ b, const double* __restrict__ dinv,
    double* __restrict__ r, double* __restrict__ rhat, double* __restrict__ p,
    double* __restrict__ ph, double* __restrict__ x,
    double* __restrict__ partials_rr, double* __restrict__ partials_rho, int len)
{
  __shared__ double s_red[kBlock / 64];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = b[i];
    if constexpr (NT) {
      __builtin_nontemporal_store(v, &r[i]);
      __builtin_nontemporal_store(v, &rhat[i]);
      __builtin_nontemporal_store(v, &p[i]);
      __builtin_nontemporal_store(0.0, &x[i]);
    } else {
      r[i] = v;
      rhat[i] = v;
      p[i] = v;
      x[i] = 0.0;
    }
    if constexpr (PRE) {
      const double z = dinv[i] * v;
      if constexpr (NT)
        __builtin_nontemporal_store(z, &ph[i]);
      else
        ph[i] = z;
    }
    acc += v * v;
  }
  store_pair_partials(acc, acc, partials_rr, partials_rho, len, s_red);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void bicg_dot_rv_kernel(
    int64_t n, const BicgScalars* sc, const double* __restrict__ rhat,
    const double* __restrict__ v, double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 a[kU], c[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      a[u] = vload<NT>(rhat, i);
      c[u] = vload<NT>(v, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      acc += a[u].x * c[u].x;
      acc += a[u].y * c[u].y;
    }
  }
  if (odd_tail(n))
    acc += rhat[n - 1] * v[n - 1];
  const double s = spmv_block_sum(acc, s_red);
  if (threadIdx.x == 0)
    partials[blockIdx.x] = s;
  clear_partials_tail(partials, len);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void bicg_dot_ts_tt_kernel(
    int64_t n, const BicgScalars* sc, const double* __restrict__ t,
    const double* __restrict__ s, double* __restrict__ partials_ts,
    double* __restrict__ partials_tt, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  double acc_ts = 0.0, acc_tt = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 a[kU], c[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      a[u] = vload<NT>(t, i);
      c[u] = vload<NT>(s, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      acc_ts += a[u].x * c[u].x;
      acc_ts += a[u].y * c[u].y;
      acc_tt += a[u].x * a[u].x;
      acc_tt += a[u].y * a[u].y;
    }
  }
  if (odd_tail(n)) {
    const double tv = t[n - 1];
    acc_ts += tv * s[n - 1];
    acc_tt += tv * tv;
  }
  store_pair_partials(acc_ts, acc_tt, partials_ts, partials_tt, len, s_red);
}

// single-workgroup reducers: one partial array -> a slot, two -> a pair
__global__ __launch_bounds__(kBlock) void bicg_reduce1_kernel(
    const double* __restrict__ partials, int len, double* __restrict__ slot,
    const BicgScalars* sc)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double s = sum_partials(partials, nullptr, len, s_red);
  if (threadIdx.x == 0)
    slot[0] = s;
}

__global__ __launch_bounds__(kBlock) void bicg_reduce2_kernel(
    const double* __restrict__ partials_a,
    const double* __restrict__ partials_b, int len, double* __restrict__ pair,
    const BicgScalars* sc)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double a = sum_partials(partials_a, nullptr, len, s_red);
  __syncthreads(); // s_red is reused
  const double b = sum_partials(partials_b, nullptr, len, s_red);
  if (threadIdx.x == 0) {
    pair[0] = a;
    pair[1] = b;
  }
}

// The history arrays carry no __restrict__: a consumer-side kernel stores
// slot k from workgroup 0 while the others read slots of k - 1 and 0.
template <bool NT, bool PRE>
__global__ __launch_bounds__(kBlock) void bicg_update_s_kernel(
    int64_t n, int k, const double* rrho, const double* rvh, BicgScalars* sc,
    const double* __restrict__ r, const double* __restrict__ v,
    const double* __restrict__ dinv, double* __restrict__ s,
    double* __restrict__ sh)
{
  if (sc->done)
    return;
  update_s_body<NT, PRE>(n, k, rvh[k], rrho, sc, r, v, dinv, s, sh);
}

template <bool NT, bool PRE>
__global__ __launch_bounds__(kBlock) void bicg_update_xr_kernel(
    int64_t n, int k, const double* rrho, const double* rvh, const double* tstt,
    const BicgScalars* sc, const double* __restrict__ ph,
    const double* __restrict__ sh, const double* __restrict__ s,
    const double* __restrict__ t, const double* __restrict__ rhat,
    double* __restrict__ x, double* __restrict__ r,
    double* __restrict__ partials_rr, double* __restrict__ partials_rho, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double alpha = rrho[2 * (k - 1) + 1] / rvh[k];
  update_xr_body<NT, PRE>(n, alpha, tstt[2 * k], tstt[2 * k + 1], ph, sh, s, t,
                          rhat, x, r, partials_rr, partials_rho, len, s_red);
}

template <bool NT, bool PRE>
__global__ __launch_bounds__(kBlock) void bicg_update_p_kernel(
    int64_t n, int k, const double* rrho, const double* rvh, const double* tstt,
    BicgScalars* sc, const double* __restrict__ r, const double* __restrict__ v,
    const double* __restrict__ dinv, double* __restrict__ p,
    double* __restrict__ ph)
{
  if (sc->done)
    return;
  update_p_body<NT, PRE>(n, k, rrho[2 * k], rrho[2 * k + 1], rrho, rvh, tstt, sc,
                         r, v, dinv, p, ph);
}

// ---- consumer-side reductions (one rank), as in blas1.hip -------------------
// bicg_reduce1_kernel(rv) + bicg_update_s_kernel in one launch
template <bool NT, bool PRE>
__global__ __launch_bounds__(kBlock) void bicg_update_s_cs_kernel(
    int64_t n, int k, const double* rrho, double* rvh, BicgScalars* sc,
    const double* partials_rv, int len, const double* __restrict__ r,
    const double* __restrict__ v, const double* __restrict__ dinv,
    double* __restrict__ s, double* __restrict__ sh)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  const double rvk
      = consume_partials(partials_rv, nullptr, len, s_red, &s_bcast);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    rvh[k] = rvk;
  update_s_body<NT, PRE>(n, k, rvk, rrho, sc, r, v, dinv, s, sh);
}

// bicg_reduce2_kernel(ts, tt) + bicg_update_xr_kernel in one launch
template <bool NT, bool PRE>
__global__ __launch_bounds__(kBlock) void bicg_update_xr_cs_kernel(
    int64_t n, int k, const double* rrho, const double* rvh, double* tstt,
    const BicgScalars* sc, const double* partials_ts, const double* partials_tt,
    int len, const double* __restrict__ ph, const double* __restrict__ sh,
    const double* __restrict__ s, const double* __restrict__ t,
    const double* __restrict__ rhat, double* __restrict__ x,
    double* __restrict__ r, double* __restrict__ partials_rr,
    double* __restrict__ partials_rho)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  const double ts
      = consume_partials(partials_ts, nullptr, len, s_red, &s_bcast);
  const double tt
      = consume_partials(partials_tt, nullptr, len, s_red, &s_bcast);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    tstt[2 * k] = ts;
    tstt[2 * k + 1] = tt;
  }
  const double alpha = rrho[2 * (k - 1) + 1] / rvh[k];
  update_xr_body<NT, PRE>(n, alpha, ts, tt, ph, sh, s, t, rhat, x, r,
                          partials_rr, partials_rho, len, s_red);
}

// bicg_reduce2_kernel(rr, rho) + bicg_update_p_kernel in one launch
template <bool NT, bool PRE>
__global__ __launch_bounds__(kBlock) void bicg_update_p_cs_kernel(
    int64_t n, int k, double* rrho, const double* rvh, const double* tstt,
    BicgScalars* sc, const double* partials_rr, const double* partials_rho,
    int len, const double* __restrict__ r, const double* __restrict__ v,
    const double* __restrict__ dinv, double* __restrict__ p,
    double* __restrict__ ph)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  const double rr_k
      = consume_partials(partials_rr, nullptr, len, s_red, &s_bcast);
  const double rho_k
      = consume_partials(partials_rho, nullptr, len, s_red, &s_bcast);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rrho[2 * k] = rr_k;
    rrho[2 * k + 1] = rho_k;
  }
  update_p_body<NT, PRE>(n, k, rr_k, rho_k, rrho, rvh, tstt, sc, r, v, dinv, p,
                         ph);
}

__global__ void bicg_reset_kernel(BicgScalars* sc, double rtol, double* rv,
                                  double* tstt, double* rrho, int kmax)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    sc->rtol = rtol;
    sc->done = 0;
    sc->kstop = -1;
    sc->status = 0;
    sc->pad = 0;
  }
  if (i <= kmax) {
    rv[i] = 0.0;
    tstt[2 * i] = 0.0;
    tstt[2 * i + 1] = 0.0;
    rrho[2 * i] = 0.0;
    rrho[2 * i + 1] = 0.0;
  }
}

} // namespace

// NT by the vector length (see blas1_stream.h), PRE by the caller's dinv
#define SPMV_LAUNCH_NT_PRE(ctx, n, pre, kernel, grid, st, ...)                 \
  do {                                                                         \
    const bool _nt = (int64_t)(n) >= (ctx)->blas1_nt_min_elems;                \
    if (_nt && (pre))                                                          \
      hipLaunchKernelGGL((kernel<true, true>), dim3(grid), dim3(kBlock), 0,    \
                         st, __VA_ARGS__);                                     \
    else if (_nt)                                                              \
      hipLaunchKernelGGL((kernel<true, false>), dim3(grid), dim3(kBlock), 0,   \
                         st, __VA_ARGS__);                                     \
    else if (pre)                                                              \
      hipLaunchKernelGGL((kernel<false, true>), dim3(grid), dim3(kBlock), 0,   \
                         st, __VA_ARGS__);                                     \
    else                                                                       \
      hipLaunchKernelGGL((kernel<false, false>), dim3(grid), dim3(kBlock), 0,  \
                         st, __VA_ARGS__);                                     \
  } while (0)

extern "C" {

// ---- workspace ----------------------------------------------------------------
int spmv_hip_bicg_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_bicg_ws** out)
{
  SPMV_REQUIRE(ctx && out && kmax >= 0);
  return solver_ws_create(ctx, kmax, out, [&](spmv_hip_bicg_ws& w) {
    const size_t hist = (size_t)kmax + 1;
    w.own.alloc(w.rv, hist);
    w.own.alloc(w.tstt, 2 * hist);
    w.own.alloc(w.rrho, 2 * hist);
    for (double** p : {&w.p_rv, &w.p_ts, &w.p_tt, &w.p_rr, &w.p_rho})
      w.own.alloc(*p, ctx->dot_blocks);
    w.own.alloc(w.sc, 1);
  });
}

int spmv_hip_bicg_ws_destroy(spmv_hip_bicg_ws* ws)
{
  return solver_ws_destroy(ws);
}

int spmv_hip_bicg_ws_reset(spmv_hip_bicg_ws* ws, double rtol, void* stream)
{
  SPMV_REQUIRE(ws);
  SPMV_SET_DEVICE(ws->ctx);
  const int n = ws->kmax + 1;
  hipLaunchKernelGGL(bicg_reset_kernel, ws_reset_grid(n), dim3(kBlock), 0,
                     spmv_stream(ws->ctx, stream), ws->sc, rtol, ws->rv,
                     ws->tstt, ws->rrho, ws->kmax);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_ws_capacity(const spmv_hip_bicg_ws* ws, int* kmax)
{
  return solver_ws_capacity(ws, kmax);
}

int spmv_hip_bicg_ws_rv(spmv_hip_bicg_ws* ws, int k, double** slot)
{
  SPMV_REQUIRE(ws && slot && k >= 0 && k <= ws->kmax);
  *slot = ws->rv + k;
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_ws_ts_tt(spmv_hip_bicg_ws* ws, int k, double** pair)
{
  SPMV_REQUIRE(ws && pair && k >= 0 && k <= ws->kmax);
  *pair = ws->tstt + 2 * (size_t)k;
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_ws_rr_rho(spmv_hip_bicg_ws* ws, int k, double** pair)
{
  SPMV_REQUIRE(ws && pair && k >= 0 && k <= ws->kmax);
  *pair = ws->rrho + 2 * (size_t)k;
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_ws_done_flag(spmv_hip_bicg_ws* ws, const int32_t** done)
{
  SPMV_REQUIRE(ws && done);
  *done = &ws->sc->done;
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_ws_read_async(spmv_hip_bicg_ws* ws,
                                int32_t* host_done_kstop_status,
                                double* host_rr_rho, size_t host_rr_rho_len,
                                void* stream)
{
  SPMV_REQUIRE(ws);
  return ws_read_async(ws->ctx, stream, host_done_kstop_status, &ws->sc->done,
                       3, host_rr_rho, host_rr_rho_len, ws->rrho,
                       2 * ((size_t)ws->kmax + 1));
}

// ---- kernels ------------------------------------------------------------------
int spmv_hip_bicg_init_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int64_t n,
                           const double* b, const double* dinv, double* r,
                           double* rhat, double* p, double* ph, double* x,
                           void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE(n == 0 || (b && r && rhat && p && x));
  SPMV_REQUIRE(n == 0 || !dinv || ph);
  SPMV_SET_DEVICE(ctx);
  int grid = spmv_grid_for(ctx, n, kBlock);
  if (grid > ctx->dot_blocks)
    grid = ctx->dot_blocks;
  SPMV_LAUNCH_NT_PRE(ctx, n, dinv != nullptr, bicg_init_kernel, grid,
                     spmv_stream(ctx, stream), n, b, dinv, r, rhat, p, ph, x,
                     ws->p_rr, ws->p_rho, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_dot_rv_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                             int64_t n, const double* rhat, const double* v,
                             void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (rhat && v)));
  SPMV_REQUIRE(aligned16(rhat, v));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, bicg_dot_rv_kernel, stream_grid_capped(ctx, n),
                 spmv_stream(ctx, stream), n, ws->sc, rhat, v, ws->p_rv,
                 ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_dot_ts_tt_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                                int64_t n, const double* t, const double* s,
                                void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (t && s)));
  SPMV_REQUIRE(aligned16(t, s));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, bicg_dot_ts_tt_kernel, stream_grid_capped(ctx, n),
                 spmv_stream(ctx, stream), n, ws->sc, t, s, ws->p_ts, ws->p_tt,
                 ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_reduce_rv(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                            void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(bicg_reduce1_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->p_rv, ctx->dot_blocks,
                     ws->rv + k, ws->sc);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_reduce_ts_tt(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                               void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(bicg_reduce2_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->p_ts, ws->p_tt,
                     ctx->dot_blocks, ws->tstt + 2 * (size_t)k, ws->sc);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_reduce_rr_rho(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                                void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 0);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(bicg_reduce2_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->p_rr, ws->p_rho,
                     ctx->dot_blocks, ws->rrho + 2 * (size_t)k, ws->sc);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

// dinv == NULL selects the unpreconditioned instantiation: sh (update_s),
// sh (update_xr) and ph (update_p) are then neither read nor written
#define SPMV_BICG_CHECK_S(n, r, v, dinv, s, sh)                                \
  SPMV_REQUIRE((n) >= 0 && ((n) == 0 || ((r) && (v) && (s))));                 \
  SPMV_REQUIRE((n) == 0 || !(dinv) || (sh));                                   \
  SPMV_REQUIRE(aligned16(r, v, dinv, s) && (!(dinv) || aligned16(sh)))

int spmv_hip_bicg_update_s_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                               int64_t n, const double* r, const double* v,
                               const double* dinv, double* s, double* sh,
                               void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_BICG_CHECK_S(n, r, v, dinv, s, sh);
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_PRE(ctx, n, dinv != nullptr, bicg_update_s_kernel,
                     stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n, k,
                     ws->rrho, ws->rv, ws->sc, r, v, dinv, s, sh);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_update_s_cs_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws,
                                  int k, int64_t n, const double* r,
                                  const double* v, const double* dinv,
                                  double* s, double* sh, void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_BICG_CHECK_S(n, r, v, dinv, s, sh);
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_PRE(ctx, n, dinv != nullptr, bicg_update_s_cs_kernel,
                     stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n, k,
                     ws->rrho, ws->rv, ws->sc, ws->p_rv, ctx->dot_blocks, r, v,
                     dinv, s, sh);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

// sh == NULL selects the unpreconditioned instantiation (ph is then p)
#define SPMV_BICG_CHECK_XR(n, ph, sh, s, t, rhat, x, r)                        \
  SPMV_REQUIRE((n) >= 0                                                        \
               && ((n) == 0 || ((ph) && (s) && (t) && (rhat) && (x) && (r)))); \
  SPMV_REQUIRE(aligned16(ph, sh, s, t, rhat, x, r))

int spmv_hip_bicg_update_xr_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                                int64_t n, const double* ph, const double* sh,
                                const double* s, const double* t,
                                const double* rhat, double* x, double* r,
                                void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_BICG_CHECK_XR(n, ph, sh, s, t, rhat, x, r);
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_PRE(ctx, n, sh != nullptr, bicg_update_xr_kernel,
                     stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n, k,
                     ws->rrho, ws->rv, ws->tstt, ws->sc, ph, sh, s, t, rhat, x,
                     r, ws->p_rr, ws->p_rho, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_update_xr_cs_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws,
                                   int k, int64_t n, const double* ph,
                                   const double* sh, const double* s,
                                   const double* t, const double* rhat,
                                   double* x, double* r, void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_BICG_CHECK_XR(n, ph, sh, s, t, rhat, x, r);
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_PRE(ctx, n, sh != nullptr, bicg_update_xr_cs_kernel,
                     stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n, k,
                     ws->rrho, ws->rv, ws->tstt, ws->sc, ws->p_ts, ws->p_tt,
                     ctx->dot_blocks, ph, sh, s, t, rhat, x, r, ws->p_rr,
                     ws->p_rho);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

// dinv == NULL selects the unpreconditioned instantiation (ph is not written)
#define SPMV_BICG_CHECK_P(n, r, v, dinv, p, ph)                                \
  SPMV_REQUIRE((n) >= 0 && ((n) == 0 || ((r) && (v) && (p))));                 \
  SPMV_REQUIRE((n) == 0 || !(dinv) || (ph));                                   \
  SPMV_REQUIRE(aligned16(r, v, dinv, p) && (!(dinv) || aligned16(ph)))

int spmv_hip_bicg_update_p_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                               int64_t n, const double* r, const double* v,
                               const double* dinv, double* p, double* ph,
                               void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_BICG_CHECK_P(n, r, v, dinv, p, ph);
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_PRE(ctx, n, dinv != nullptr, bicg_update_p_kernel,
                     stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n, k,
                     ws->rrho, ws->rv, ws->tstt, ws->sc, r, v, dinv, p, ph);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_bicg_update_p_cs_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws,
                                  int k, int64_t n, const double* r,
                                  const double* v, const double* dinv,
                                  double* p, double* ph, void* stream)
{
  SPMV_REQUIRE(ctx);
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_BICG_CHECK_P(n, r, v, dinv, p, ph);
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_PRE(ctx, n, dinv != nullptr, bicg_update_p_cs_kernel,
                     stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n, k,
                     ws->rrho, ws->rv, ws->tstt, ws->sc, ws->p_rr, ws->p_rho,
                     ctx->dot_blocks, r, v, dinv, p, ph);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
