// BLAS-1 kernels of spmv::idrs (gfx950): IDR(s), the biortho variant of van
// Gijzen and Sonneveld (2011), 1 <= s <= 8, on SIGN shadow vectors, in the
// launch structure of blas1_cgshift.hip.  The recurrence is spelled out in
// host/cg.h.
//
// Shadow vectors.  p_j(i) = +1.0 where bit j of one 64-bit hash of the GLOBAL
// row index is clear, -1.0 where it is set (sign_bits below).  P is never
// stored and never streamed: p_j . w adds w_i or -w_i, so the multi-dot P^T w
// reads w once and has no product, and a partition of the rows changes only the
// summation order.
//
// Inner step q of a cycle, `.` the global dot product (M is the s x s lower
// triangular scalar matrix, B^-1 the right preconditioner):
//
//   prep(q)      a thread's tile of r in registers: v = r - c_q g_q - ...;
//                FUSED (B^-1 none or dinv): u = om*(dinv*v) + c_q u_q + ... goes
//                straight into the padded vector the SpMV reads, v is never
//                stored; STORE_V writes v for sgs / ILU(0) / amg / Chebyshev and
//                FROM_VH forms u from vh = B^-1 v in place afterwards
//   (mult)       g = A u
//   sign_dot     s partial rows of P^T g, laid out [j][workgroup]
//   [reduce]     several ranks only: rows -> the slots `red`, then one all-reduce
//   biortho(q)   one workgroup adds the rows in the reducer's order; thread 0:
//                a_0..a_{q-1}, column q of M, be; a zero or non-finite pivot
//                raises `done` with status 1
//   update(q)    g_q = g - a_0 g_0 - ..; u_q = u - a_0 u_0 - ..; r = r - be*g_q;
//                x = x + be*u_q; partials of r.r: 2q + 8 vector passes
//   step(q)      one workgroup adds the partials of r.r; thread 0: k, the
//                history, the stop test, f_i -= be*M[i][q], and the coefficients
//                c of the step that follows
//
// and after q = s - 1: prep(PLAIN) or B^-1 (vh), mult (t = A vh), omega_dot
// (partials of t.r and t.t in one pass), omega (om, status 2), omega_update (r,
// x, the partials of r.r and the s sign sums of the new r in the same pass),
// step(s).  Once per solve: sign_dot of b with the extra row b.b, step(-1).
//
// Layout.  g_i = G + i * ld and u_i = U + i * ld are contiguous vectors.
//
// Alignment.  Vectors whose addresses are all multiples of 16 (even ld) are
// walked with 16-byte accesses; any other set of 8-byte aligned vectors with two
// 8-byte accesses per element, the same elements in the same threads, so the
// bits do not depend on the alignment.
//
// Stop protocol.  `done` is raised by step, biortho or omega, each BEHIND the
// last kernel that moved x for the k it records; every kernel enqueued after it
// returns at once, so x is exactly the iterate of the returned k.
//
// Built with -ffp-contract=off: every product, sum, difference, quotient and
// square root is a rounding of its own.  Streaming shape: blas1_stream.h.
#include "common.h"
#include "blas1_stream.h"
#include "idrs_ws.h"

#include <cmath>
#include <cstddef>

namespace
{

enum { kFused = 0, kStoreV = 1, kFromVh = 2, kPlain = 3 };

__device__ __forceinline__ void raise_done(IdrsScalars* sc, int status)
{
  sc->kstop = sc->k;
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

// The signs of global row gi: bit j set -> p_j(gi) = -1.  h0 = seed * GOLD +
// GOLD (uint64 wraparound), formed once on the host.
__device__ __forceinline__ uint32_t sign_bits(uint64_t gi, uint64_t h0)
{
  uint64_t z = gi + h0;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return static_cast<uint32_t>(z) & 0xffu;
}

// h_j += p_j(row) * w for j < s (fully unrolled: h stays in registers)
__device__ __forceinline__ void sign_add(double (&h)[kIdrsMaxS], int s,
                                         uint32_t bits, double w)
{
#pragma unroll
  for (int j = 0; j < kIdrsMaxS; ++j)
    if (j < s)
      h[j] += ((bits >> j) & 1u) ? -w : w;
}

// the workgroup's shares of the s sign sums into rows 0 .. s-1
__device__ __forceinline__ void store_sign_partials(
    const double (&h)[kIdrsMaxS], int s, double* __restrict__ part, int len,
    double* s_red)
{
#pragma unroll
  for (int j = 0; j < kIdrsMaxS; ++j) {
    if (j < s) { // uniform
      const double v = spmv_block_sum(h[j], s_red);
      double* const row = part + (size_t)j * len;
      if (threadIdx.x == 0)
        row[blockIdx.x] = v;
      clear_partials_tail(row, len);
      __syncthreads(); // s_red is reused
    }
  }
}

__device__ __forceinline__ void store_row_partial(double acc, double* row,
                                                  int len, double* s_red)
{
  const double v = spmv_block_sum(acc, s_red);
  if (threadIdx.x == 0)
    row[blockIdx.x] = v;
  clear_partials_tail(row, len);
}

// rows 0 .. s-1 of P^T w; with_ww: w.w in row kIdrsRowRr
template <bool NT, bool AL>
__global__ __launch_bounds__(kBlock) void idrs_sign_dot_kernel(
    int64_t n, const IdrsScalars* __restrict__ sc, int s, uint64_t h0,
    int64_t row0, const double* __restrict__ w, int with_ww,
    double* __restrict__ part, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  double h[kIdrsMaxS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double ww = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 wv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2) { wv[u] = ld<NT, AL>(w, i); }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      const uint64_t gi = (uint64_t)row0 + 2 * (uint64_t)i;
      sign_add(h, s, sign_bits(gi, h0), wv[u].x);
      sign_add(h, s, sign_bits(gi + 1, h0), wv[u].y);
      if (with_ww) { // uniform
        ww += wv[u].x * wv[u].x;
        ww += wv[u].y * wv[u].y;
      }
    }
  }
  if (odd_tail(n)) {
    const double t = w[n - 1];
    sign_add(h, s, sign_bits((uint64_t)row0 + (uint64_t)(n - 1), h0), t);
    if (with_ww)
      ww += t * t;
  }
  store_sign_partials(h, s, part, len, s_red);
  if (with_ww)
    store_row_partial(ww, part + (size_t)kIdrsRowRr * len, len, s_red);
}

// src and out are the same vector in mode kFromVh: no __restrict__ on them
template <bool NT, bool AL>
__global__ __launch_bounds__(kBlock) void idrs_prep_kernel(
    int64_t n, const IdrsScalars* __restrict__ sc, int s, int q, int mode,
    const double* src, const double* __restrict__ G,
    const double* __restrict__ U, int64_t ldg,
    const double* __restrict__ dinv, double* out)
{
  if (sc->done)
    return;
  const double om = sc->om;
  const bool sub_g = mode == kFused || mode == kStoreV;
  const bool scale = dinv && (mode == kFused || mode == kPlain);
  const bool add_u = mode == kFused || mode == kFromVh;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 v[kU];
    SPMV_FOR_LANE_ELEMS(i, n2) { v[u] = ld<NT, AL>(src, i); }
    if (sub_g) {
      for (int j = q; j < s; ++j) {
        const double c = sc->c[j];
        const double* const gj = G + j * ldg;
        f64x2 gv[kU];
        SPMV_FOR_LANE_ELEMS(i, n2) { gv[u] = ld<NT, AL>(gj, i); }
        SPMV_FOR_LANE_ELEMS(i, n2)
        {
          v[u].x = v[u].x - c * gv[u].x;
          v[u].y = v[u].y - c * gv[u].y;
        }
      }
    }
    if (scale) {
      f64x2 dv[kU];
      SPMV_FOR_LANE_ELEMS(i, n2) { dv[u] = ld<NT, AL>(dinv, i); }
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        v[u].x = dv[u].x * v[u].x;
        v[u].y = dv[u].y * v[u].y;
      }
    }
    if (add_u) {
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        v[u].x = om * v[u].x;
        v[u].y = om * v[u].y;
      }
      for (int j = q; j < s; ++j) {
        const double c = sc->c[j];
        const double* const uj = U + j * ldg;
        f64x2 uv[kU];
        SPMV_FOR_LANE_ELEMS(i, n2) { uv[u] = ld<NT, AL>(uj, i); }
        SPMV_FOR_LANE_ELEMS(i, n2)
        {
          v[u].x = v[u].x + c * uv[u].x;
          v[u].y = v[u].y + c * uv[u].y;
        }
      }
    }
    SPMV_FOR_LANE_ELEMS(i, n2) { st<NT, AL>(out, i, v[u]); }
  }
  if (odd_tail(n)) {
    const int64_t e = n - 1;
    double v = src[e];
    if (sub_g)
      for (int j = q; j < s; ++j)
        v = v - sc->c[j] * G[j * ldg + e];
    if (scale)
      v = dinv[e] * v;
    if (add_u) {
      v = om * v;
      for (int j = q; j < s; ++j)
        v = v + sc->c[j] * U[j * ldg + e];
    }
    out[e] = v;
  }
}

// Columns 0 .. q-1 of G and U are read, column q is written; r and x are read
// and written at the same index by the same thread.
template <bool NT, bool AL>
__global__ __launch_bounds__(kBlock) void idrs_update_kernel(
    int64_t n, const IdrsScalars* __restrict__ sc, int q,
    const double* __restrict__ g, const double* __restrict__ uin, double* G,
    double* U, int64_t ldg, double* r, double* x, double* __restrict__ p_rr,
    int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double be = sc->be;
  double* const gq = G + q * ldg;
  double* const uq = U + q * ldg;
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 gv[kU], uv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      gv[u] = ld<NT, AL>(g, i);
      uv[u] = ld<NT, AL>(uin, i);
    }
    for (int j = 0; j < q; ++j) {
      const double a = sc->a[j];
      const double* const gj = G + j * ldg;
      const double* const uj = U + j * ldg;
      f64x2 gc[kU], uc[kU];
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        gc[u] = ld<NT, AL>(gj, i);
        uc[u] = ld<NT, AL>(uj, i);
      }
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        gv[u].x = gv[u].x - a * gc[u].x;
        gv[u].y = gv[u].y - a * gc[u].y;
        uv[u].x = uv[u].x - a * uc[u].x;
        uv[u].y = uv[u].y - a * uc[u].y;
      }
    }
    f64x2 rv[kU], xv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      rv[u] = ld<NT, AL>(r, i);
      xv[u] = ld<NT, AL>(x, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      st<NT, AL>(gq, i, gv[u]);
      st<NT, AL>(uq, i, uv[u]);
      rv[u].x = rv[u].x - be * gv[u].x;
      rv[u].y = rv[u].y - be * gv[u].y;
      xv[u].x = xv[u].x + be * uv[u].x;
      xv[u].y = xv[u].y + be * uv[u].y;
      st<NT, AL>(r, i, rv[u]);
      st<NT, AL>(x, i, xv[u]);
      acc += rv[u].x * rv[u].x;
      acc += rv[u].y * rv[u].y;
    }
  }
  if (odd_tail(n)) {
    const int64_t e = n - 1;
    double gv = g[e], uv = uin[e];
    for (int j = 0; j < q; ++j) {
      const double a = sc->a[j];
      gv = gv - a * G[j * ldg + e];
      uv = uv - a * U[j * ldg + e];
    }
    gq[e] = gv;
    uq[e] = uv;
    const double t = r[e] - be * gv;
    r[e] = t;
    x[e] = x[e] + be * uv;
    acc += t * t;
  }
  store_row_partial(acc, p_rr, len, s_red);
}

// partials of t.r and t.t in one pass
template <bool NT, bool AL>
__global__ __launch_bounds__(kBlock) void idrs_omega_dot_kernel(
    int64_t n, const IdrsScalars* __restrict__ sc, const double* __restrict__ t,
    const double* __restrict__ r, double* __restrict__ p_tr,
    double* __restrict__ p_tt, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  double tr = 0.0, tt = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 tv[kU], rv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      tv[u] = ld<NT, AL>(t, i);
      rv[u] = ld<NT, AL>(r, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      tr += tv[u].x * rv[u].x;
      tr += tv[u].y * rv[u].y;
      tt += tv[u].x * tv[u].x;
      tt += tv[u].y * tv[u].y;
    }
  }
  if (odd_tail(n)) {
    tr += t[n - 1] * r[n - 1];
    tt += t[n - 1] * t[n - 1];
  }
  store_pair_partials(tr, tt, p_tr, p_tt, len, s_red);
}

// r = r - om*t; x = x + om*vh; the partials of r.r and of P^T r, same pass
template <bool NT, bool AL>
__global__ __launch_bounds__(kBlock) void idrs_omega_update_kernel(
    int64_t n, const IdrsScalars* __restrict__ sc, int s, uint64_t h0,
    int64_t row0, const double* __restrict__ t, const double* __restrict__ vh,
    double* r, double* x, double* __restrict__ part, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double om = sc->om;
  double h[kIdrsMaxS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 tv[kU], vv[kU], rv[kU], xv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      tv[u] = ld<NT, AL>(t, i);
      vv[u] = ld<NT, AL>(vh, i);
      rv[u] = ld<NT, AL>(r, i);
      xv[u] = ld<NT, AL>(x, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      rv[u].x = rv[u].x - om * tv[u].x;
      rv[u].y = rv[u].y - om * tv[u].y;
      xv[u].x = xv[u].x + om * vv[u].x;
      xv[u].y = xv[u].y + om * vv[u].y;
      st<NT, AL>(r, i, rv[u]);
      st<NT, AL>(x, i, xv[u]);
      const uint64_t gi = (uint64_t)row0 + 2 * (uint64_t)i;
      sign_add(h, s, sign_bits(gi, h0), rv[u].x);
      sign_add(h, s, sign_bits(gi + 1, h0), rv[u].y);
      acc += rv[u].x * rv[u].x;
      acc += rv[u].y * rv[u].y;
    }
  }
  if (odd_tail(n)) {
    const int64_t e = n - 1;
    const double rn = r[e] - om * t[e];
    r[e] = rn;
    x[e] = x[e] + om * vh[e];
    sign_add(h, s, sign_bits((uint64_t)row0 + (uint64_t)e, h0), rn);
    acc += rn * rn;
  }
  store_sign_partials(h, s, part, len, s_red);
  store_row_partial(acc, part + (size_t)kIdrsRowRr * len, len, s_red);
}

// ---- the single-workgroup scalar kernels ----------------------------------------

// rows 0 .. s-1 -> s_h[0 .. s-1], in the reducer's order (valid in thread 0)
__device__ __forceinline__ void sum_sign_rows(const double* __restrict__ part,
                                              int len, int s, double* s_red,
                                              double* s_h)
{
  for (int j = 0; j < s; ++j) {
    const double v = sum_partials(part + (size_t)j * len, nullptr, len, s_red);
    if (threadIdx.x == 0)
      s_h[j] = v;
    __syncthreads(); // s_red is reused
  }
}

// c_q .. c_{s-1} by forward substitution on M[q:, q:] (thread 0)
__device__ __forceinline__ void idrs_coef(IdrsScalars* sc, int s, int q)
{
  for (int i = q; i < s; ++i) {
    double t = sc->f[i];
    for (int j = q; j < i; ++j)
      t = t - sc->M[i * kIdrsMaxS + j] * sc->c[j];
    sc->c[i] = t / sc->M[i * kIdrsMaxS + i];
  }
}

// k += 1, the history, the stop test (thread 0); a NaN goes on
__device__ __forceinline__ bool idrs_goes_on(IdrsScalars* sc,
                                             double* __restrict__ hist)
{
  if (sc->k >= sc->kmax) { // (no room in the history: the host never asks)
    raise_done(sc, 0);
    return false;
  }
  const int k = sc->k + 1;
  sc->k = k;
  const double h = sqrt(sc->rr);
  hist[k] = h;
  if (h / sc->hist0 < sc->rtol || k == sc->kmax) {
    raise_done(sc, 0);
    return false;
  }
  return true;
}

// q = -1: start; 0 <= q < s: the end of inner step q; q = s: of the om step
__global__ __launch_bounds__(kBlock) void idrs_step_kernel(
    IdrsScalars* sc, int s, int q, int reduced,
    const double* __restrict__ part, int len, double* __restrict__ hist)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_h[kIdrsMaxS];
  if (sc->done) // (uniform: thread 0 raises it behind the sums' barriers)
    return;
  const bool full = q < 0 || q == s;
  double rr = 0.0;
  if (!reduced) {
    if (full)
      sum_sign_rows(part, len, s, s_red, s_h);
    rr = sum_partials(part + (size_t)kIdrsRowRr * len, nullptr, len, s_red);
  }
  if (threadIdx.x != 0)
    return;
  if (reduced)
    rr = sc->red[s];
  sc->rr = rr;
  if (full)
    for (int j = 0; j < s; ++j)
      sc->f[j] = reduced ? sc->red[j] : s_h[j];
  if (q < 0) {
    const double h0 = sqrt(rr);
    sc->hist0 = h0;
    hist[0] = h0;
    if (rr == 0.0 || sc->kmax == 0) { // x = 0 is the answer / no step is asked
      raise_done(sc, 0);
      return;
    }
    idrs_coef(sc, s, 0);
    return;
  }
  if (!idrs_goes_on(sc, hist))
    return;
  if (q == s) {
    idrs_coef(sc, s, 0);
    return;
  }
  const double be = sc->be;
  for (int i = q + 1; i < s; ++i)
    sc->f[i] = sc->f[i] - be * sc->M[i * kIdrsMaxS + q];
  if (q + 1 < s)
    idrs_coef(sc, s, q + 1);
}

// h = P^T g of the un-orthogonalised g: every a_i and the new column of M by
// scalar arithmetic, because p_i . g_j = M[i][j] is already known
__global__ __launch_bounds__(kBlock) void idrs_biortho_kernel(
    IdrsScalars* sc, int s, int q, int reduced,
    const double* __restrict__ part, int len)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_h[kIdrsMaxS];
  if (sc->done)
    return;
  if (!reduced)
    sum_sign_rows(part, len, s, s_red, s_h);
  if (threadIdx.x != 0)
    return;
  if (reduced)
    for (int j = 0; j < s; ++j)
      s_h[j] = sc->red[j];
  for (int i = 0; i < q; ++i) {
    double t = s_h[i];
    for (int j = 0; j < i; ++j)
      t = t - sc->a[j] * sc->M[i * kIdrsMaxS + j];
    sc->a[i] = t / sc->M[i * kIdrsMaxS + i];
  }
  for (int i = q; i < s; ++i) {
    double t = s_h[i];
    for (int j = 0; j < q; ++j)
      t = t - sc->a[j] * sc->M[i * kIdrsMaxS + j];
    sc->M[i * kIdrsMaxS + q] = t;
  }
  const double piv = sc->M[q * kIdrsMaxS + q];
  if (piv == 0.0 || !isfinite(piv)) {
    raise_done(sc, 1);
    return;
  }
  sc->be = sc->f[q] / piv;
}

__global__ __launch_bounds__(kBlock) void idrs_omega_kernel(
    IdrsScalars* sc, int reduced, const double* __restrict__ part, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  double tr = 0.0, tt = 0.0;
  if (!reduced) {
    tr = sum_partials(part + (size_t)kIdrsRowTr * len, nullptr, len, s_red);
    __syncthreads(); // s_red is reused
    tt = sum_partials(part + (size_t)kIdrsRowTt * len, nullptr, len, s_red);
  }
  if (threadIdx.x != 0)
    return;
  if (reduced) {
    tr = sc->red[kIdrsRowTr];
    tt = sc->red[kIdrsRowTt];
  }
  if (!(tt > 0.0)) { // (a NaN too)
    raise_done(sc, 2);
    return;
  }
  double om = tr / tt;
  const double rho = tr / (sqrt(tt) * sqrt(sc->rr));
  const double kappa = sc->kappa;
  if (fabs(rho) < kappa)
    om = om * kappa / fabs(rho);
  if (om == 0.0 || !isfinite(om)) {
    raise_done(sc, 2);
    return;
  }
  sc->om = om;
}

// workgroup b: row list.row[b] of the partials -> red[list.dst[b]]
struct IdrsRedList {
  int row[kIdrsMaxS + 1];
  int dst[kIdrsMaxS + 1];
};

__global__ __launch_bounds__(kBlock) void idrs_reduce_kernel(
    IdrsScalars* sc, IdrsRedList list, const double* __restrict__ part, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double v = sum_partials(part + (size_t)list.row[blockIdx.x] * len,
                                nullptr, len, s_red);
  if (threadIdx.x == 0)
    sc->red[list.dst[blockIdx.x]] = v;
}

__global__ void idrs_reset_kernel(IdrsScalars* sc, double rtol, double kappa,
                                  int kmax, int s, double* hist, int hist_len)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    double* d = reinterpret_cast<double*>(sc);
    for (int j = 0; j < kIdrsDoubles; ++j)
      d[j] = 0.0;
    int32_t* w = &sc->done;
    for (int j = 0; j < kIdrsWords; ++j)
      w[j] = 0;
    sc->rtol = rtol;
    sc->kappa = kappa;
    sc->om = 1.0;
    for (int j = 0; j < kIdrsMaxS; ++j)
      sc->M[j * kIdrsMaxS + j] = 1.0;
    sc->kstop = -1;
    sc->kmax = kmax;
    sc->s = s;
  }
  if (i < hist_len)
    hist[i] = 0.0;
}

static_assert(kIdrsDoubles == SPMV_HIP_IDRS_DOUBLES
                  && kIdrsWords == SPMV_HIP_IDRS_WORDS
                  && kIdrsRows == SPMV_HIP_IDRS_ROWS
                  && kIdrsMaxS == SPMV_HIP_IDRS_MAX_S,
              "idrs_ws.h and spmv_hip.h agree");
static_assert(offsetof(IdrsScalars, done) == kIdrsDoubles * sizeof(double),
              "the doubles of IdrsScalars come first");
static_assert(sizeof(IdrsScalars)
                  == kIdrsDoubles * sizeof(double) + kIdrsWords * sizeof(int32_t),
              "the words of IdrsScalars follow without a gap");

// 8-byte alignment is what a double* promises; checked all the same
template <typename... P>
bool aligned8(const P*... p)
{
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 7u) == 0;
}

uint64_t hash_base(uint64_t seed)
{
  const uint64_t gold = 0x9E3779B97F4A7C15ull;
  return seed * gold + gold;
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

// every kernel entry: the workspace is this context's and has been reset
#define SPMV_REQUIRE_IDRS(ctx, ws)                                             \
  SPMV_REQUIRE((ctx) && (ws) && (ws)->ctx == (ctx) && (ws)->s >= 1)

extern "C" {

// ---- workspace ----------------------------------------------------------------
int spmv_hip_idrs_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_idrs_ws** out)
{
  SPMV_REQUIRE(ctx && out && kmax >= 0);
  return solver_ws_create(ctx, kmax, out, [&](spmv_hip_idrs_ws& w) {
    w.own.alloc(w.hist, (size_t)kmax + 1);
    w.own.alloc(w.part, kIdrsRows * (size_t)ctx->dot_blocks);
    w.own.alloc(w.sc, 1);
  });
}

int spmv_hip_idrs_ws_destroy(spmv_hip_idrs_ws* ws)
{
  return solver_ws_destroy(ws);
}

int spmv_hip_idrs_ws_reset(spmv_hip_idrs_ws* ws, double rtol, double kappa,
                           int kmax, int s, uint64_t seed, void* stream)
{
  SPMV_REQUIRE(ws && kmax >= 0 && kmax <= ws->kmax);
  SPMV_REQUIRE(s >= 1 && s <= kIdrsMaxS);
  SPMV_SET_DEVICE(ws->ctx);
  ws->s = s;
  ws->seed = seed;
  const int n = ws->kmax + 1;
  hipLaunchKernelGGL(idrs_reset_kernel, ws_reset_grid(n), dim3(kBlock), 0,
                     spmv_stream(ws->ctx, stream), ws->sc, rtol, kappa, kmax, s,
                     ws->hist, n);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_idrs_ws_capacity(const spmv_hip_idrs_ws* ws, int* kmax)
{
  return solver_ws_capacity(ws, kmax);
}

int spmv_hip_idrs_ws_array(spmv_hip_idrs_ws* ws, int which, double** p,
                           int64_t* count)
{
  SPMV_REQUIRE(ws && p);
  double* q = nullptr;
  int64_t n = 0;
  switch (which) {
  case SPMV_HIP_IDRS_RED: q = ws->sc->red, n = kIdrsRows; break;
  case SPMV_HIP_IDRS_HIST: q = ws->hist, n = (int64_t)ws->kmax + 1; break;
  case SPMV_HIP_IDRS_PART:
    q = ws->part, n = (int64_t)kIdrsRows * ws->ctx->dot_blocks;
    break;
  case SPMV_HIP_IDRS_SCALARS:
    q = reinterpret_cast<double*>(ws->sc), n = kIdrsDoubles;
    break;
  default: return SPMV_HIP_EINVAL;
  }
  *p = q;
  if (count)
    *count = n;
  return SPMV_HIP_OK;
}

int spmv_hip_idrs_ws_read_async(spmv_hip_idrs_ws* ws, int32_t* host_state,
                                double* host_hist, size_t host_hist_len,
                                void* stream)
{
  SPMV_REQUIRE(ws);
  return ws_read_async(ws->ctx, stream, host_state, &ws->sc->done,
                       SPMV_HIP_IDRS_STATE_WORDS, host_hist, host_hist_len,
                       ws->hist, (size_t)ws->kmax + 1);
}

int spmv_hip_idrs_ws_set_words(spmv_hip_idrs_ws* ws, const int32_t* host_words,
                               void* stream)
{
  SPMV_REQUIRE(ws && host_words);
  // the words the kernels turn into addresses are checked here
  const int32_t k = host_words[3], kmax = host_words[4], s = host_words[5];
  SPMV_REQUIRE(k >= 0 && kmax >= k && kmax <= ws->kmax && s == ws->s);
  return ws_put_words(ws->ctx, stream, &ws->sc->done, host_words, kIdrsWords);
}

int spmv_hip_idrs_ws_get_words(spmv_hip_idrs_ws* ws, int32_t* host_words,
                               void* stream)
{
  SPMV_REQUIRE(ws && host_words);
  return ws_get_words(ws->ctx, stream, host_words, &ws->sc->done, kIdrsWords);
}

// ---- kernels ------------------------------------------------------------------
int spmv_hip_idrs_sign_dot_f64(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws,
                               int64_t n, int64_t row0, const double* w,
                               int with_ww, void* stream)
{
  SPMV_REQUIRE_IDRS(ctx, ws);
  SPMV_REQUIRE(n >= 0 && row0 >= 0 && (n == 0 || w) && aligned8(w));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_AL(ctx, n, aligned16(w), idrs_sign_dot_kernel,
                    stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n,
                    ws->sc, ws->s, hash_base(ws->seed), row0, w,
                    with_ww ? 1 : 0, ws->part, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_idrs_prep_f64(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int q,
                           int mode, int64_t n, const double* src,
                           const double* G, const double* U, int64_t ld,
                           const double* dinv, double* out, void* stream)
{
  SPMV_REQUIRE_IDRS(ctx, ws);
  SPMV_REQUIRE(mode >= kFused && mode <= kPlain && n >= 0 && ld >= n);
  SPMV_REQUIRE(mode == kPlain ? q == ws->s : (q >= 0 && q < ws->s));
  SPMV_REQUIRE((n == 0 || (src && out && (mode == kPlain || (G && U))))
               && aligned8(src, G, U, dinv, out));
  // in place only where the mode says so
  SPMV_REQUIRE(n == 0 || (mode == kFromVh) == (src == out));
  SPMV_REQUIRE(n == 0 || !dinv || (dinv != out && dinv != src));
  SPMV_SET_DEVICE(ctx);
  const bool al = aligned16(src, G, U, dinv, out) && (ld & 1) == 0;
  SPMV_LAUNCH_NT_AL(ctx, n, al, idrs_prep_kernel, stream_grid(ctx, n),
                    spmv_stream(ctx, stream), n, ws->sc, ws->s, q, mode, src, G,
                    U, ld, dinv, out);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_idrs_update_f64(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int q,
                             int64_t n, const double* g, const double* u,
                             double* G, double* U, int64_t ld, double* r,
                             double* x, void* stream)
{
  SPMV_REQUIRE_IDRS(ctx, ws);
  SPMV_REQUIRE(q >= 0 && q < ws->s && n >= 0 && ld >= n);
  SPMV_REQUIRE((n == 0 || (g && u && G && U && r && x))
               && aligned8(g, u, G, U, r, x));
  SPMV_REQUIRE(n == 0 || (g != u && g != r && g != x && u != r && u != x
                          && r != x && G != U));
  SPMV_SET_DEVICE(ctx);
  const bool al = aligned16(g, u, G, U, r, x) && (ld & 1) == 0;
  SPMV_LAUNCH_NT_AL(ctx, n, al, idrs_update_kernel, stream_grid_capped(ctx, n),
                    spmv_stream(ctx, stream), n, ws->sc, q, g, u, G, U, ld, r, x,
                    ws->part + (size_t)kIdrsRowRr * ctx->dot_blocks,
                    ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_idrs_omega_dot_f64(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws,
                                int64_t n, const double* t, const double* r,
                                void* stream)
{
  SPMV_REQUIRE_IDRS(ctx, ws);
  SPMV_REQUIRE(n >= 0 && (n == 0 || (t && r)) && aligned8(t, r));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_AL(ctx, n, aligned16(t, r), idrs_omega_dot_kernel,
                    stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n,
                    ws->sc, t, r,
                    ws->part + (size_t)kIdrsRowTr * ctx->dot_blocks,
                    ws->part + (size_t)kIdrsRowTt * ctx->dot_blocks,
                    ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_idrs_omega_update_f64(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws,
                                   int64_t n, int64_t row0, const double* t,
                                   const double* vh, double* r, double* x,
                                   void* stream)
{
  SPMV_REQUIRE_IDRS(ctx, ws);
  SPMV_REQUIRE(n >= 0 && row0 >= 0 && (n == 0 || (t && vh && r && x))
               && aligned8(t, vh, r, x));
  SPMV_REQUIRE(n == 0 || (t != r && t != x && vh != r && vh != x && r != x));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_AL(ctx, n, aligned16(t, vh, r, x), idrs_omega_update_kernel,
                    stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n,
                    ws->sc, ws->s, hash_base(ws->seed), row0, t, vh, r, x,
                    ws->part, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_idrs_reduce(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int which,
                         void* stream)
{
  SPMV_REQUIRE_IDRS(ctx, ws);
  IdrsRedList list = {};
  int count = 0;
  const int s = ws->s;
  if (which == SPMV_HIP_IDRS_REDUCE_H || which == SPMV_HIP_IDRS_REDUCE_HRR)
    for (int j = 0; j < s; ++j, ++count)
      list.row[count] = list.dst[count] = j;
  if (which == SPMV_HIP_IDRS_REDUCE_RR || which == SPMV_HIP_IDRS_REDUCE_HRR) {
    list.row[count] = kIdrsRowRr;
    list.dst[count++] = s;
  }
  if (which == SPMV_HIP_IDRS_REDUCE_OM) {
    list.row[0] = list.dst[0] = kIdrsRowTr;
    list.row[1] = list.dst[1] = kIdrsRowTt;
    count = 2;
  }
  SPMV_REQUIRE(count > 0);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(idrs_reduce_kernel, dim3(count), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, list, ws->part,
                     ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_idrs_step(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int q,
                       int reduced, void* stream)
{
  SPMV_REQUIRE_IDRS(ctx, ws);
  SPMV_REQUIRE(q >= -1 && q <= ws->s);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(idrs_step_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, ws->s, q,
                     reduced ? 1 : 0, ws->part, ctx->dot_blocks, ws->hist);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_idrs_start(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int reduced,
                        void* stream)
{
  return spmv_hip_idrs_step(ctx, ws, -1, reduced, stream);
}

int spmv_hip_idrs_biortho(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int q,
                          int reduced, void* stream)
{
  SPMV_REQUIRE_IDRS(ctx, ws);
  SPMV_REQUIRE(q >= 0 && q < ws->s);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(idrs_biortho_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, ws->s, q,
                     reduced ? 1 : 0, ws->part, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_idrs_omega(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int reduced,
                        void* stream)
{
  SPMV_REQUIRE_IDRS(ctx, ws);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(idrs_omega_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, reduced ? 1 : 0,
                     ws->part, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
