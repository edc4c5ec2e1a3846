// BLAS-1 kernels of the Chebyshev polynomial preconditioner (gfx950):
// spmv::chebyshev_apply and spmv::pcg_chebyshev.
//
// z = q(dinv*A) dinv r is the `degree`-step Chebyshev iteration for A z = r
// from z = 0, with the coefficients a_j, b_j of chebyshev_coefficients (host):
//
//   step 0       d = b_0 * (dinv*r) ;                      z = d
//   step j >= 1  w = A z (Matrix::mult, between the kernels)
//                d = a_j*d + b_j*(dinv*(r - w)) ;          z = z + d
//
// Everything here is elementwise; the coefficients are kernel arguments.  dinv
// is a template flag (PRE): without it no multiply and no dinv stream.  The
// LAST step does not write d.
//
//   apply0     step 0                              (chebyshev_apply)
//   step       step j >= 1: w, r, dinv, d, z in; d, z out -- 7 passes, 6
//              without dinv, one less when LAST.  Inside pcg_chebyshev (a
//              workspace is given) it returns at once after `done`, and the
//              LAST step also leaves the partials of r.z: it reads r anyway
//   init       r = b ; x = 0 ; partials of r.r ; step 0
//   update_r   r -= alpha Ap ; partials of r.r ; step 0
//              alpha = rz[k-1] / pAp[k]
//              (degree 1: step 0 is LAST, so init / update_r leave the
//              partials of r.z too and one kernel is the whole preconditioner)
//   update_xp  x += alpha p ; stop test ; p = beta p + z
//              beta = rz[k] / rz[k-1] ; stop: sqrt(rr[k]) / sqrt(rr[0]) < rtol
//   scale      out = dinv * (in / s): setup work of lambda_max_estimate
//
// and, for spmv::pcg_sgs, whose preconditioner is not elementwise
// (spmv_mcgs.hip) and which shares update_xp:
//   sgs_init      r = b ; x = 0 ; partials of r.r
//   sgs_update_r  r -= alpha Ap ; partials of r.r
//   sgs_dot_rz    partials of r.z after the sweeps
//
// pcg_chebyshev runs on the device state of spmv::pcg (pcg_ws.h) and on its
// reducers (blas1_pcg.hip: pcg_reduce_pAp, _pAp2, pcg_reduce_rz_rr), whose
// scalar layout fits as it is: the partials of r.r come from update_r, those of
// r.z from the LAST step, and pcg_reduce_rz_rr after the LAST step installs
// the pair {rz[k], rr[k]}.  Every dot product is finished by a reducer kernel.
//
// Built with -ffp-contract=off: every product and sum is a rounding of its
// own.  Streaming shape: see blas1_stream.h (persistent grid, units of kU
// 16-byte loads per lane and stream, non-temporal from blas1_nt_min_elems
// doubles on, a scalar tail for an odd n).
#include "common.h"
#include "blas1_stream.h"
#include "pcg_ws.h"
#include "amg_elem.h"

#include <cmath>

namespace
{

// the workgroup's share of one dot product into its slot (as the producers of
// blas1_pcg.hip leave theirs: pcg_reduce_rz_rr adds `len` entries)
__device__ __forceinline__ void store_partials(double acc,
                                               double* __restrict__ partials,
                                               int len, double* s_red)
{
  const double s = spmv_block_sum(acc, s_red);
  if (threadIdx.x == 0)
    partials[blockIdx.x] = s;
  clear_partials_tail(partials, len);
  __syncthreads(); // s_red may be written again
}

// (scaled<PRE>, cheb_first, cheb_corr, cheb_next: amg_elem.h)

// ---- step 0 on a stored r: d = b0 * (dinv*r) ; z = d --------------------------
template <bool NT, bool PRE, bool LAST>
__global__ __launch_bounds__(kBlock) void cheb_apply0_kernel(
    int64_t n, double b0, const double* __restrict__ r,
    const double* __restrict__ dinv, double* __restrict__ d,
    double* __restrict__ z)
{
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 rv[kU], dv[kU] = {};
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      rv[u] = vload<NT>(r, i);
      if constexpr (PRE)
        dv[u] = vload<NT>(dinv, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      f64x2 t;
      t.x = cheb_first<PRE>(b0, dv[u].x, rv[u].x);
      t.y = cheb_first<PRE>(b0, dv[u].y, rv[u].y);
      if constexpr (!LAST)
        vstore<NT>(d, i, t);
      vstore<NT>(z, i, t);
    }
  }
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    const double t = cheb_first<PRE>(b0, PRE ? dinv[i] : 0.0, r[i]);
    if constexpr (!LAST)
      d[i] = t;
    z[i] = t;
  }
}

// ---- step j >= 1: d = a*d + b*(dinv*(r - w)) ; z += d --------------------------
// DOT: this thread's share of r.z (the LAST step inside pcg_chebyshev)
template <bool NT, bool PRE, bool LAST, bool DOT>
__global__ __launch_bounds__(kBlock) void cheb_step_kernel(
    int64_t n, double a, double b, const PcgScalars* __restrict__ sc,
    const double* __restrict__ w, const double* __restrict__ r,
    const double* __restrict__ dinv, double* __restrict__ d,
    double* __restrict__ z, double* __restrict__ partials_rz, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc && sc->done)
    return;
  double acc_rz = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 wv[kU], rv[kU], dv[kU] = {}, ev[kU], zv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      wv[u] = vload<NT>(w, i);
      rv[u] = vload<NT>(r, i);
      if constexpr (PRE)
        dv[u] = vload<NT>(dinv, i);
      ev[u] = vload<NT>(d, i);
      zv[u] = vload<NT>(z, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      const double tx = cheb_corr<PRE>(b, dv[u].x, rv[u].x, wv[u].x);
      const double ty = cheb_corr<PRE>(b, dv[u].y, rv[u].y, wv[u].y);
      ev[u].x = cheb_next(a, ev[u].x, tx);
      ev[u].y = cheb_next(a, ev[u].y, ty);
      if constexpr (!LAST)
        vstore<NT>(d, i, ev[u]);
      zv[u].x += ev[u].x;
      zv[u].y += ev[u].y;
      vstore<NT>(z, i, zv[u]);
      if constexpr (DOT) {
        acc_rz += rv[u].x * zv[u].x;
        acc_rz += rv[u].y * zv[u].y;
      }
    }
  }
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    const double t = cheb_corr<PRE>(b, PRE ? dinv[i] : 0.0, r[i], w[i]);
    const double e = cheb_next(a, d[i], t);
    if constexpr (!LAST)
      d[i] = e;
    const double zi = z[i] + e;
    z[i] = zi;
    if constexpr (DOT)
      acc_rz += r[i] * zi;
  }
  if constexpr (DOT)
    store_partials(acc_rz, partials_rz, len, s_red);
}

// ---- start: r = b ; x = 0 ; partials of r.r ; step 0 ---------------------------
// (b and dinv need no alignment here; LAST = degree 1: partials of r.z too)
template <bool NT, bool PRE, bool LAST>
__global__ __launch_bounds__(kBlock) void cheb_init_kernel(
    int64_t n, double b0, const double* __restrict__ bvec,
    const double* __restrict__ dinv, double* __restrict__ r,
    double* __restrict__ x, double* __restrict__ d, double* __restrict__ z,
    double* __restrict__ partials_rz, double* __restrict__ partials_rr, int len)
{
  __shared__ double s_red[kBlock / 64];
  double acc_rz = 0.0, acc_rr = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = bvec[i];
    const double t = b0 * scaled<PRE>(PRE ? dinv[i] : 0.0, v);
    if constexpr (NT) {
      __builtin_nontemporal_store(v, &r[i]);
      __builtin_nontemporal_store(0.0, &x[i]);
      if constexpr (!LAST)
        __builtin_nontemporal_store(t, &d[i]);
      __builtin_nontemporal_store(t, &z[i]);
    } else {
      r[i] = v;
      x[i] = 0.0;
      if constexpr (!LAST)
        d[i] = t;
      z[i] = t;
    }
    acc_rr += v * v;
    if constexpr (LAST)
      acc_rz += v * t;
  }
  store_partials(acc_rr, partials_rr, len, s_red);
  if constexpr (LAST)
    store_partials(acc_rz, partials_rz, len, s_red);
}

// ---- r -= alpha Ap ; partials of r.r ; step 0 ------------------------------------
template <bool NT, bool PRE, bool LAST>
__global__ __launch_bounds__(kBlock) void cheb_update_r_kernel(
    int64_t n, int k, double b0, const double* __restrict__ zr,
    const double* __restrict__ pAp, const PcgScalars* __restrict__ sc,
    const double* __restrict__ Ap, const double* __restrict__ dinv,
    double* __restrict__ r, double* __restrict__ d, double* __restrict__ z,
    double* __restrict__ partials_rz, double* __restrict__ partials_rr, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double nalpha = -(zr[2 * (k - 1)] / pAp[k]);
  double acc_rz = 0.0, acc_rr = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 av[kU], rv[kU], dv[kU] = {};
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      av[u] = vload<NT>(Ap, i);
      rv[u] = vload<NT>(r, i);
      if constexpr (PRE)
        dv[u] = vload<NT>(dinv, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      rv[u].x += nalpha * av[u].x;
      rv[u].y += nalpha * av[u].y;
      vstore<NT>(r, i, rv[u]);
      f64x2 t;
      t.x = b0 * scaled<PRE>(dv[u].x, rv[u].x);
      t.y = b0 * scaled<PRE>(dv[u].y, rv[u].y);
      if constexpr (!LAST)
        vstore<NT>(d, i, t);
      vstore<NT>(z, i, t);
      acc_rr += rv[u].x * rv[u].x;
      acc_rr += rv[u].y * rv[u].y;
      if constexpr (LAST) {
        acc_rz += rv[u].x * t.x;
        acc_rz += rv[u].y * t.y;
      }
    }
  }
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    const double rv = r[i] + nalpha * Ap[i];
    r[i] = rv;
    const double t = b0 * scaled<PRE>(PRE ? dinv[i] : 0.0, rv);
    if constexpr (!LAST)
      d[i] = t;
    z[i] = t;
    acc_rr += rv * rv;
    if constexpr (LAST)
      acc_rz += rv * t;
  }
  store_partials(acc_rr, partials_rr, len, s_red);
  if constexpr (LAST)
    store_partials(acc_rz, partials_rz, len, s_red);
}

// ---- x += alpha p ; stop test ; p = beta p + z -------------------------------------
template <bool NT>
__global__ __launch_bounds__(kBlock) void cheb_update_xp_kernel(
    int64_t n, int k, const double* __restrict__ zr,
    const double* __restrict__ pAp, const PcgScalars* __restrict__ sc,
    const double* __restrict__ z, double* __restrict__ x,
    double* __restrict__ p)
{
  if (sc->done)
    return;
  const double rz_old = zr[2 * (k - 1)];
  const double alpha = rz_old / pAp[k];
  const double beta = zr[2 * k] / rz_old;
  const bool converged = sqrt(zr[2 * k + 1]) / sqrt(zr[1]) < sc->rtol;
  const bool tail = odd_tail(n);
  const int64_t n2 = n >> 1;
  if (converged) { // x takes this iteration's update, p stays
    SPMV_FOR_UNITS(n2)
    {
      f64x2 pv[kU], xv[kU];
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        pv[u] = vload<NT>(p, i);
        xv[u] = vload<NT>(x, i);
      }
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        xv[u].x += alpha * pv[u].x;
        xv[u].y += alpha * pv[u].y;
        vstore<NT>(x, i, xv[u]);
      }
    }
    if (tail)
      x[n - 1] += alpha * p[n - 1];
    return;
  }
  SPMV_FOR_UNITS(n2)
  {
    f64x2 pv[kU], xv[kU], zv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      pv[u] = vload<NT>(p, i);
      xv[u] = vload<NT>(x, i);
      zv[u] = vload<NT>(z, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      xv[u].x += alpha * pv[u].x;
      xv[u].y += alpha * pv[u].y;
      vstore<NT>(x, i, xv[u]);
      pv[u].x = beta * pv[u].x;
      pv[u].y = beta * pv[u].y;
      pv[u].x += zv[u].x;
      pv[u].y += zv[u].y;
      vstore<NT>(p, i, pv[u]);
    }
  }
  if (tail) {
    const int64_t i = n - 1;
    x[i] += alpha * p[i];
    p[i] = beta * p[i] + z[i];
  }
}

// ---- setup (lambda_max_estimate): out = dinv * (in / s), or in / s ----------------
// (no alignment assumed)
template <bool PRE>
__global__ __launch_bounds__(kBlock) void cheb_scale_kernel(
    int64_t n, double s, const double* __restrict__ dinv,
    const double* __restrict__ in, double* __restrict__ out)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = scaled<PRE>(PRE ? dinv[i] : 0.0, in[i] / s);
}

// ---- pcg_sgs: the recurrence of pcg_chebyshev around a preconditioner that is
// ---- not elementwise (spmv_mcgs.hip), so step 0 leaves the kernels above ------
// r = b ; x = 0 ; partials of r.r  (b needs no alignment)
template <bool NT>
__global__ __launch_bounds__(kBlock) void sgs_init_kernel(
    int64_t n, const double* __restrict__ bvec, double* __restrict__ r,
    double* __restrict__ x, double* __restrict__ partials_rr, int len)
{
  __shared__ double s_red[kBlock / 64];
  double acc_rr = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = bvec[i];
    if constexpr (NT) {
      __builtin_nontemporal_store(v, &r[i]);
      __builtin_nontemporal_store(0.0, &x[i]);
    } else {
      r[i] = v;
      x[i] = 0.0;
    }
    acc_rr += v * v;
  }
  store_partials(acc_rr, partials_rr, len, s_red);
}

// r -= alpha Ap ; partials of r.r
template <bool NT>
__global__ __launch_bounds__(kBlock) void sgs_update_r_kernel(
    int64_t n, int k, const double* __restrict__ zr,
    const double* __restrict__ pAp, const PcgScalars* __restrict__ sc,
    const double* __restrict__ Ap, double* __restrict__ r,
    double* __restrict__ partials_rr, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double nalpha = -(zr[2 * (k - 1)] / pAp[k]);
  double acc_rr = 0.0;
  const int64_t n2 = n >> 1;
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
      acc_rr += rv[u].x * rv[u].x;
      acc_rr += rv[u].y * rv[u].y;
    }
  }
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    const double rv = r[i] + nalpha * Ap[i];
    r[i] = rv;
    acc_rr += rv * rv;
  }
  store_partials(acc_rr, partials_rr, len, s_red);
}

// partials of r.z, z = M(r) as the sweeps left it
template <bool NT>
__global__ __launch_bounds__(kBlock) void sgs_dot_rz_kernel(
    int64_t n, const PcgScalars* __restrict__ sc, const double* __restrict__ r,
    const double* __restrict__ z, double* __restrict__ partials_rz, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  double acc_rz = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 rv[kU], zv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      rv[u] = vload<NT>(r, i);
      zv[u] = vload<NT>(z, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      acc_rz += rv[u].x * zv[u].x;
      acc_rz += rv[u].y * zv[u].y;
    }
  }
  if (odd_tail(n))
    acc_rz += r[n - 1] * z[n - 1];
  store_partials(acc_rz, partials_rz, len, s_red);
}

} // namespace

// kernel<NT, PRE, LAST>: NT by the vector's length (see blas1_stream.h), PRE
// by dinv
#define SPMV_CHEB_LAUNCH3(ctx, n, pre, last, kernel, grid, st, ...)            \
  do {                                                                         \
    const bool _nt = (int64_t)(n) >= (ctx)->blas1_nt_min_elems;                \
    const int _v = (_nt ? 4 : 0) | ((pre) ? 2 : 0) | ((last) ? 1 : 0);         \
    const dim3 _g(grid), _b(kBlock);                                           \
    switch (_v) {                                                              \
    case 0: hipLaunchKernelGGL((kernel<false, false, false>), _g, _b, 0, st, __VA_ARGS__); break; \
    case 1: hipLaunchKernelGGL((kernel<false, false, true>), _g, _b, 0, st, __VA_ARGS__); break;  \
    case 2: hipLaunchKernelGGL((kernel<false, true, false>), _g, _b, 0, st, __VA_ARGS__); break;  \
    case 3: hipLaunchKernelGGL((kernel<false, true, true>), _g, _b, 0, st, __VA_ARGS__); break;   \
    case 4: hipLaunchKernelGGL((kernel<true, false, false>), _g, _b, 0, st, __VA_ARGS__); break;  \
    case 5: hipLaunchKernelGGL((kernel<true, false, true>), _g, _b, 0, st, __VA_ARGS__); break;   \
    case 6: hipLaunchKernelGGL((kernel<true, true, false>), _g, _b, 0, st, __VA_ARGS__); break;   \
    default: hipLaunchKernelGGL((kernel<true, true, true>), _g, _b, 0, st, __VA_ARGS__); break;   \
    }                                                                          \
  } while (0)

namespace
{
// cheb_step_kernel<NT, PRE, LAST, DOT> with DOT = LAST inside a solve
template <bool NT, bool PRE>
void launch_step(bool last, bool dot, int grid, hipStream_t st, int64_t n,
                 double a, double b, const PcgScalars* sc, const double* w,
                 const double* r, const double* dinv, double* d, double* z,
                 double* partials_rz, int len)
{
  const dim3 g(grid), blk(kBlock);
  if (!last)
    hipLaunchKernelGGL((cheb_step_kernel<NT, PRE, false, false>), g, blk, 0, st,
                       n, a, b, sc, w, r, dinv, d, z, partials_rz, len);
  else if (!dot)
    hipLaunchKernelGGL((cheb_step_kernel<NT, PRE, true, false>), g, blk, 0, st,
                       n, a, b, sc, w, r, dinv, d, z, partials_rz, len);
  else
    hipLaunchKernelGGL((cheb_step_kernel<NT, PRE, true, true>), g, blk, 0, st, n,
                       a, b, sc, w, r, dinv, d, z, partials_rz, len);
}
} // namespace

extern "C" {

int spmv_hip_cheb_apply0_f64(spmv_hip_ctx* ctx, int64_t n, double b0,
                             const double* r, const double* dinv, double* d,
                             double* z, void* stream)
{
  SPMV_REQUIRE(ctx && n >= 0 && (n == 0 || (r && z)));
  SPMV_REQUIRE(aligned16(r, dinv, d, z));
  SPMV_SET_DEVICE(ctx);
  const int grid = stream_grid(ctx, n);
  SPMV_CHEB_LAUNCH3(ctx, n, dinv != nullptr, d == nullptr, cheb_apply0_kernel,
                    grid, spmv_stream(ctx, stream), n, b0, r, dinv, d, z);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cheb_step_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int64_t n,
                           double a, double b, int last, const double* w,
                           const double* r, const double* dinv, double* d,
                           double* z, void* stream)
{
  SPMV_REQUIRE(ctx && (!ws || ws->ctx == ctx));
  SPMV_REQUIRE(n >= 0 && (n == 0 || (w && r && d && z)));
  SPMV_REQUIRE(aligned16(w, r, dinv, d, z));
  SPMV_SET_DEVICE(ctx);
  const int grid = stream_grid_capped(ctx, n);
  hipStream_t st = spmv_stream(ctx, stream);
  const PcgScalars* sc = ws ? ws->sc : nullptr;
  double* prz = ws ? ws->partials_rz : nullptr;
  const bool nt = n >= ctx->blas1_nt_min_elems, dot = ws && last;
  if (nt && dinv)
    launch_step<true, true>(last, dot, grid, st, n, a, b, sc, w, r, dinv, d, z,
                            prz, ctx->dot_blocks);
  else if (nt)
    launch_step<true, false>(last, dot, grid, st, n, a, b, sc, w, r, dinv, d, z,
                             prz, ctx->dot_blocks);
  else if (dinv)
    launch_step<false, true>(last, dot, grid, st, n, a, b, sc, w, r, dinv, d, z,
                             prz, ctx->dot_blocks);
  else
    launch_step<false, false>(last, dot, grid, st, n, a, b, sc, w, r, dinv, d,
                              z, prz, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cheb_init_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int64_t n,
                           double b0, const double* b, const double* dinv,
                           double* r, double* x, double* d, double* z,
                           void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE(n == 0 || (b && r && x && z));
  SPMV_SET_DEVICE(ctx);
  int grid = spmv_grid_for(ctx, n, kBlock);
  if (grid > ctx->dot_blocks)
    grid = ctx->dot_blocks;
  SPMV_CHEB_LAUNCH3(ctx, n, dinv != nullptr, d == nullptr, cheb_init_kernel,
                    grid, spmv_stream(ctx, stream), n, b0, b, dinv, r, x, d, z,
                    ws->partials_rz, ws->partials_rr, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cheb_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                               int64_t n, double b0, const double* Ap,
                               const double* dinv, double* r, double* d,
                               double* z, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && k >= 1 && k <= ws->kmax);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (Ap && r && z)));
  SPMV_REQUIRE(aligned16(Ap, dinv, r, d, z));
  SPMV_SET_DEVICE(ctx);
  const int grid = stream_grid_capped(ctx, n);
  SPMV_CHEB_LAUNCH3(ctx, n, dinv != nullptr, d == nullptr, cheb_update_r_kernel,
                    grid, spmv_stream(ctx, stream), n, k, b0, ws->zr, ws->pAp,
                    ws->sc, Ap, dinv, r, d, z, ws->partials_rz, ws->partials_rr,
                    ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cheb_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                                int64_t n, const double* z, double* x, double* p,
                                void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && k >= 1 && k <= ws->kmax);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (z && x && p)));
  SPMV_REQUIRE(aligned16(z, x, p));
  SPMV_SET_DEVICE(ctx);
  const int grid = stream_grid(ctx, n);
  hipStream_t st = spmv_stream(ctx, stream);
  SPMV_LAUNCH_NT(ctx, n, cheb_update_xp_kernel, grid, st, n, k, ws->zr, ws->pAp,
                 ws->sc, z, x, p);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cheb_scale_f64(spmv_hip_ctx* ctx, int64_t n, double s,
                            const double* dinv, const double* in, double* out,
                            void* stream)
{
  SPMV_REQUIRE(ctx && n >= 0 && (n == 0 || (in && out)));
  SPMV_SET_DEVICE(ctx);
  const int grid = spmv_grid_for(ctx, n, kBlock);
  hipStream_t st = spmv_stream(ctx, stream);
  if (dinv)
    hipLaunchKernelGGL(cheb_scale_kernel<true>, dim3(grid), dim3(kBlock), 0, st,
                       n, s, dinv, in, out);
  else
    hipLaunchKernelGGL(cheb_scale_kernel<false>, dim3(grid), dim3(kBlock), 0,
                       st, n, s, dinv, in, out);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_sgs_init_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int64_t n,
                          const double* b, double* r, double* x, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE(n == 0 || (b && r && x));
  SPMV_SET_DEVICE(ctx);
  int grid = spmv_grid_for(ctx, n, kBlock);
  if (grid > ctx->dot_blocks)
    grid = ctx->dot_blocks;
  hipStream_t st = spmv_stream(ctx, stream);
  SPMV_LAUNCH_NT(ctx, n, sgs_init_kernel, grid, st, n, b, r, x, ws->partials_rr,
                 ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_sgs_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                              int64_t n, const double* Ap, double* r,
                              void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && k >= 1 && k <= ws->kmax);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (Ap && r)));
  SPMV_REQUIRE(aligned16(Ap, r));
  SPMV_SET_DEVICE(ctx);
  const int grid = stream_grid_capped(ctx, n);
  hipStream_t st = spmv_stream(ctx, stream);
  SPMV_LAUNCH_NT(ctx, n, sgs_update_r_kernel, grid, st, n, k, ws->zr, ws->pAp,
                 ws->sc, Ap, r, ws->partials_rr, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_sgs_dot_rz_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int64_t n,
                            const double* r, const double* z, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (r && z)));
  SPMV_REQUIRE(aligned16(r, z));
  SPMV_SET_DEVICE(ctx);
  const int grid = stream_grid_capped(ctx, n);
  hipStream_t st = spmv_stream(ctx, stream);
  SPMV_LAUNCH_NT(ctx, n, sgs_dot_rz_kernel, grid, st, n, ws->sc, r, z,
                 ws->partials_rz, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
