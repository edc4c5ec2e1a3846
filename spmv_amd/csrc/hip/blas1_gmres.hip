// BLAS-1 kernels of spmv::gmres (gfx950): restarted GMRES with right
// preconditioning and twice-iterated classical Gram-Schmidt (CGS2), in the
// launch structure of blas1_bicgstab.hip.  One inner step at basis size j + 1
// (V = v_0 .. v_j, w = A M^-1 v_j), `.` the global dot product:
//
//   multi_dot     partials of v_i . w, i = 0..j, ONE launch: a workgroup keeps
//                 its tile of w in registers and streams the basis past it in
//                 groups of kGmresGroup vectors (w is re-read between groups)
//   reduce        the j + 1 partial rows -> h[0..j] (first pass) or c[0..j]
//                 (second pass), one workgroup per row
//   multi_axpy    w = w - h_0 v_0 - ... - h_j v_j in that order, w's tile in
//                 registers, every v_i read once; the second pass takes c,
//                 adds h_i = h_i + c_i (one thread) and leaves partials of w.w
//   givens        hn = sqrt(w.w); column (h_0..h_j, hn) through the rotations
//                 0..j-1, the new rotation, R_jj, g, k, hist[k], the stop test
//                 and the status; inv = 1.0 / hn
//   scale         v_{j+1} = w * inv (v_0 = r * inv after `start`)
//
// and per cycle:
//
//   residual      r = b - Ax (r = b in the first cycle) ; partials of r.r
//   start         beta = sqrt(r.r) ; first cycle: hist[0] = beta ; r.r == 0
//                 stops ; g = (beta, 0, ..) ; inv = 1.0 / beta
//   solve_y       back substitution on the jn columns kept
//   combine       u = y_0 v_0 ; u = u + y_i v_i, i = 1..jn-1
//   add           x = x + z   (z = M^-1 u, or u itself)
//
// Partials of the multi-dot are laid out [i][workgroup], ctx->dot_blocks per
// row.  Accumulation order of one v_i . w: a thread adds its 2 * kU products
// per trip (.x then .y, element order), over its trips; the odd tail element
// last (thread 0 of workgroup 0); spmv_block_sum; sum_partials -- the order of
// stream_dot and its reducer, so the depth of blas1_cases.depth applies.
//
// Stop protocol.  `done` is raised by givens (tolerance, k == kmax, lucky
// breakdown, R_jj == 0) or start (r.r == 0).  After it multi_dot, reduce,
// multi_axpy, givens, scale and start return at once.  The cycle-end kernels
// (solve_y, combine, add) look at `finished` instead: the cycle that stopped
// still gets its update, exactly once -- the residual kernel that FOLLOWS a
// cycle end raises `finished` when it finds `done` (start raises both), and
// the host enqueues at most one cycle end that is not followed by a residual.
// After `finished` nothing here writes x, the history or k.
//
// Built with -ffp-contract=off: every product, sum, difference, quotient and
// square root above is a rounding of its own.  Streaming shape: blas1_stream.h.
#include "common.h"
#include "blas1_stream.h"
#include "solver_ws.h"

#include <cmath>

constexpr int kGmresMaxRestart = SPMV_HIP_GMRES_MAX_RESTART; // 64
constexpr int kGmresGroup = SPMV_HIP_GMRES_GROUP;            // 8 accumulators
constexpr int kGmresHalf = 4; // vectors whose loads are in flight together

struct GmresScalars {
  double rtol;
  double inv; // 1.0 / beta (start) or 1.0 / hn (givens): what scale multiplies by
  double ww;  // w.w or r.r: the reducer's slot (the all-reduce works on it)
  // read_async copies the next four
  int32_t done;
  int32_t kstop;
  int32_t status; // 0 converged / kmax / running, 1 lucky breakdown, 2 R_jj == 0
  int32_t k;      // inner steps completed
  int32_t jn;     // columns kept in the current cycle
  int32_t finished;
  int32_t kmax;
  int32_t restart;
};

struct spmv_hip_gmres_ws {
  spmv_hip_ctx* ctx = nullptr;
  int kmax = 0;             // capacity of hist
  SolverArrays own;
  double* small = nullptr;  // one allocation: the arrays below up to hist
  double* h = nullptr;      // kGmresMaxRestart: first-pass / summed coefficients
  double* c = nullptr;      // kGmresMaxRestart: second-pass coefficients
  double* cs = nullptr;     // rotations
  double* sn = nullptr;
  double* g = nullptr;      // kGmresMaxRestart + 1
  double* y = nullptr;      // kGmresMaxRestart
  double* R = nullptr;      // column l at R + l * kGmresMaxRestart
  double* hist = nullptr;   // kmax + 1
  double* part = nullptr;   // [kGmresMaxRestart][dot_blocks]
  double* p_ww = nullptr;   // dot_blocks
  GmresScalars* sc = nullptr;
};

namespace
{

__device__ __forceinline__ void raise_done(GmresScalars* sc, int kstop,
                                           int status)
{
  sc->kstop = kstop;
  sc->status = status;
  sc->done = 1;
}

// ---- one group of CNT basis vectors against a tile -------------------------
// acc[g] += v_{g} . w over this workgroup's units (V points at the group)
template <bool NT, int CNT>
__device__ __forceinline__ void dot_group(int64_t n2, const double* V,
                                          int64_t stride, const double* w,
                                          double* acc)
{
  SPMV_FOR_UNITS(n2)
  {
    f64x2 wv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2) { wv[u] = vload<NT>(w, i); }
#pragma unroll
    for (int h0 = 0; h0 < CNT; h0 += kGmresHalf) {
      f64x2 vv[kGmresHalf][kU];
#pragma unroll
      for (int g = 0; g < kGmresHalf; ++g)
        if (h0 + g < CNT) {
          SPMV_FOR_LANE_ELEMS(i, n2)
          {
            vv[g][u] = vload<NT>(V + (int64_t)(h0 + g) * stride, i);
          }
        }
#pragma unroll
      for (int g = 0; g < kGmresHalf; ++g)
        if (h0 + g < CNT) {
          SPMV_FOR_LANE_ELEMS(i, n2)
          {
            acc[h0 + g] += vv[g][u].x * wv[u].x;
            acc[h0 + g] += vv[g][u].y * wv[u].y;
          }
        }
    }
  }
}

// t = t - coef_g * v_g (SUB) or t = t + coef_g * v_g, g = 0..CNT-1 in order,
// on the tile t of the unit at `base`
template <bool NT, int CNT, bool SUB>
__device__ __forceinline__ void axpy_group(int64_t n2, int64_t base,
                                           const double* V, int64_t stride,
                                           const double* coef, f64x2* t)
{
#pragma unroll
  for (int h0 = 0; h0 < CNT; h0 += kGmresHalf) {
    f64x2 vv[kGmresHalf][kU];
#pragma unroll
    for (int g = 0; g < kGmresHalf; ++g)
      if (h0 + g < CNT) {
        SPMV_FOR_LANE_ELEMS(i, n2)
        {
          vv[g][u] = vload<NT>(V + (int64_t)(h0 + g) * stride, i);
        }
      }
#pragma unroll
    for (int g = 0; g < kGmresHalf; ++g)
      if (h0 + g < CNT) {
        const double a = coef[h0 + g];
        SPMV_FOR_LANE_ELEMS(i, n2)
        {
          if constexpr (SUB) {
            t[u].x = t[u].x - a * vv[g][u].x;
            t[u].y = t[u].y - a * vv[g][u].y;
          } else {
            t[u].x = t[u].x + a * vv[g][u].x;
            t[u].y = t[u].y + a * vv[g][u].y;
          }
        }
      }
  }
}

// the groups of vectors [first, nvec) against the tile t, in order
template <bool NT, bool SUB>
__device__ __forceinline__ void axpy_groups(int64_t n2, int64_t base,
                                            const double* V, int64_t stride,
                                            const double* coef, int first,
                                            int nvec, f64x2* t)
{
  for (int g0 = first; g0 < nvec; g0 += kGmresGroup) {
    const double* Vg = V + (int64_t)g0 * stride;
    const double* cg = coef + g0;
    switch (nvec - g0 < kGmresGroup ? nvec - g0 : kGmresGroup) {
    case 1: axpy_group<NT, 1, SUB>(n2, base, Vg, stride, cg, t); break;
    case 2: axpy_group<NT, 2, SUB>(n2, base, Vg, stride, cg, t); break;
    case 3: axpy_group<NT, 3, SUB>(n2, base, Vg, stride, cg, t); break;
    case 4: axpy_group<NT, 4, SUB>(n2, base, Vg, stride, cg, t); break;
    case 5: axpy_group<NT, 5, SUB>(n2, base, Vg, stride, cg, t); break;
    case 6: axpy_group<NT, 6, SUB>(n2, base, Vg, stride, cg, t); break;
    case 7: axpy_group<NT, 7, SUB>(n2, base, Vg, stride, cg, t); break;
    default: axpy_group<NT, 8, SUB>(n2, base, Vg, stride, cg, t); break;
    }
  }
}
static_assert(kGmresGroup == 8, "the switches spell the group sizes 1..8");

// ---- kernels ------------------------------------------------------------------
template <bool NT>
__global__ __launch_bounds__(kBlock) void gmres_multi_dot_kernel(
    int64_t n, const GmresScalars* sc, const double* __restrict__ V,
    int64_t stride, int nvec, const double* __restrict__ w,
    double* __restrict__ partials, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const int64_t n2 = n >> 1;
  for (int g0 = 0; g0 < nvec; g0 += kGmresGroup) {
    const int cnt = nvec - g0 < kGmresGroup ? nvec - g0 : kGmresGroup;
    const double* Vg = V + (int64_t)g0 * stride;
    double acc[kGmresGroup];
#pragma unroll
    for (int g = 0; g < kGmresGroup; ++g)
      acc[g] = 0.0;
    switch (cnt) {
    case 1: dot_group<NT, 1>(n2, Vg, stride, w, acc); break;
    case 2: dot_group<NT, 2>(n2, Vg, stride, w, acc); break;
    case 3: dot_group<NT, 3>(n2, Vg, stride, w, acc); break;
    case 4: dot_group<NT, 4>(n2, Vg, stride, w, acc); break;
    case 5: dot_group<NT, 5>(n2, Vg, stride, w, acc); break;
    case 6: dot_group<NT, 6>(n2, Vg, stride, w, acc); break;
    case 7: dot_group<NT, 7>(n2, Vg, stride, w, acc); break;
    default: dot_group<NT, 8>(n2, Vg, stride, w, acc); break;
    }
    if (odd_tail(n)) {
      const double wl = w[n - 1];
#pragma unroll
      for (int g = 0; g < kGmresGroup; ++g)
        if (g < cnt)
          acc[g] += Vg[(int64_t)g * stride + n - 1] * wl;
    }
#pragma unroll
    for (int g = 0; g < kGmresGroup; ++g)
      if (g < cnt) { // cnt is uniform: every thread takes the same barriers
        double* row = partials + (int64_t)(g0 + g) * len;
        const double s = spmv_block_sum(acc[g], s_red);
        if (threadIdx.x == 0)
          row[blockIdx.x] = s;
        clear_partials_tail(row, len);
        __syncthreads(); // s_red is reused
      }
  }
}

// one workgroup per row of partials
__global__ __launch_bounds__(kBlock) void gmres_reduce_kernel(
    const GmresScalars* sc, const double* __restrict__ partials, int len,
    double* __restrict__ dst)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double s = sum_partials(partials + (int64_t)blockIdx.x * len, nullptr,
                                len, s_red);
  if (threadIdx.x == 0)
    dst[blockIdx.x] = s;
}

// SECOND: coef = c, hacc = h takes h_i + c_i, partials of w.w
template <bool NT, bool SECOND>
__device__ __forceinline__ void multi_axpy_body(
    int64_t n, const double* __restrict__ V, int64_t stride, int nvec,
    const double* __restrict__ coef, double* __restrict__ hacc,
    double* __restrict__ w, double* __restrict__ partials_ww, int len,
    double* s_red)
{
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 wv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2) { wv[u] = vload<NT>(w, i); }
    axpy_groups<NT, true>(n2, base, V, stride, coef, 0, nvec, wv);
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      vstore<NT>(w, i, wv[u]);
      if constexpr (SECOND) {
        acc += wv[u].x * wv[u].x;
        acc += wv[u].y * wv[u].y;
      }
    }
  }
  if (odd_tail(n)) {
    double t = w[n - 1];
    for (int i = 0; i < nvec; ++i)
      t = t - coef[i] * V[(int64_t)i * stride + n - 1];
    w[n - 1] = t;
    if constexpr (SECOND)
      acc += t * t;
  }
  if constexpr (SECOND) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      for (int i = 0; i < nvec; ++i)
        hacc[i] = hacc[i] + coef[i];
    const double s = spmv_block_sum(acc, s_red);
    if (threadIdx.x == 0)
      partials_ww[blockIdx.x] = s;
    clear_partials_tail(partials_ww, len);
  }
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void gmres_multi_axpy1_kernel(
    int64_t n, const GmresScalars* sc, const double* __restrict__ V,
    int64_t stride, int nvec, const double* __restrict__ h,
    double* __restrict__ w)
{
  if (sc->done)
    return;
  multi_axpy_body<NT, false>(n, V, stride, nvec, h, nullptr, w, nullptr, 0,
                             nullptr);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void gmres_multi_axpy2_kernel(
    int64_t n, const GmresScalars* sc, const double* __restrict__ V,
    int64_t stride, int nvec, const double* __restrict__ c,
    double* __restrict__ h, double* __restrict__ w,
    double* __restrict__ partials_ww, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  multi_axpy_body<NT, true>(n, V, stride, nvec, c, h, w, partials_ww, len,
                            s_red);
}

// dst = src * inv (in place when dst == src: no __restrict__)
template <bool NT>
__global__ __launch_bounds__(kBlock) void gmres_scale_kernel(
    int64_t n, const GmresScalars* sc, const double* src, double* dst)
{
  if (sc->done)
    return;
  const double inv = sc->inv;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 a[kU];
    SPMV_FOR_LANE_ELEMS(i, n2) { a[u] = vload<NT>(src, i); }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      a[u].x = a[u].x * inv;
      a[u].y = a[u].y * inv;
      vstore<NT>(dst, i, a[u]);
    }
  }
  if (odd_tail(n))
    dst[n - 1] = src[n - 1] * inv;
}

// r = b - Ax (Ax == nullptr: r = b) ; partials of r.r.  Raises `finished` when
// the solve has stopped: the cycle end before this launch was the last.
template <bool NT>
__global__ __launch_bounds__(kBlock) void gmres_residual_kernel(
    int64_t n, GmresScalars* sc, const double* __restrict__ b,
    const double* __restrict__ Ax, double* __restrict__ r,
    double* __restrict__ partials_ww, int len)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      sc->finished = 1;
    return;
  }
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 bv[kU], av[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      bv[u] = vload<NT>(b, i);
      if (Ax)
        av[u] = vload<NT>(Ax, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      if (Ax) {
        bv[u].x = bv[u].x - av[u].x;
        bv[u].y = bv[u].y - av[u].y;
      }
      vstore<NT>(r, i, bv[u]);
      acc += bv[u].x * bv[u].x;
      acc += bv[u].y * bv[u].y;
    }
  }
  if (odd_tail(n)) {
    const double t = Ax ? b[n - 1] - Ax[n - 1] : b[n - 1];
    r[n - 1] = t;
    acc += t * t;
  }
  const double s = spmv_block_sum(acc, s_red);
  if (threadIdx.x == 0)
    partials_ww[blockIdx.x] = s;
  clear_partials_tail(partials_ww, len);
}

// the value of w.w / r.r: the workgroup's own sum of the partials, or the slot
// the reducer filled and the host all-reduced (several ranks)
__device__ __forceinline__ double finish_ww(const GmresScalars* sc,
                                            const double* partials_ww, int len,
                                            int reduced, double* s_red)
{
  if (reduced)
    return sc->ww;
  return sum_partials(partials_ww, nullptr, len, s_red);
}

// single workgroup: the start of a cycle
__global__ __launch_bounds__(kBlock) void gmres_start_kernel(
    GmresScalars* sc, const double* __restrict__ partials_ww, int len,
    int reduced, int first, double* __restrict__ g, double* __restrict__ hist)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double rr = finish_ww(sc, partials_ww, len, reduced, s_red);
  if (threadIdx.x != 0)
    return;
  const double beta = sqrt(rr);
  if (first)
    hist[0] = beta;
  sc->jn = 0;
  if (rr == 0.0) { // x is the answer (first cycle: x = 0)
    raise_done(sc, sc->k, 0);
    sc->finished = 1;
    return;
  }
  g[0] = beta;
  for (int i = 1; i <= kGmresMaxRestart; ++i)
    g[i] = 0.0;
  sc->inv = 1.0 / beta;
}

// single workgroup: inner step j after the second multi_axpy
__global__ __launch_bounds__(kBlock) void gmres_givens_kernel(
    GmresScalars* sc, int j, const double* __restrict__ partials_ww, int len,
    int reduced, const double* __restrict__ h, double* __restrict__ cs,
    double* __restrict__ sn, double* __restrict__ g, double* __restrict__ R,
    double* __restrict__ hist)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double ww = finish_ww(sc, partials_ww, len, reduced, s_red);
  if (threadIdx.x != 0)
    return;
  const double hn = sqrt(ww);
  double* col = R + (int64_t)j * kGmresMaxRestart; // column j of R, in place
  for (int i = 0; i <= j; ++i)
    col[i] = h[i];
  // rotations 0..j-1 act on (col_i, col_{i+1}); col_{j+1} = hn enters only the
  // new one
  for (int i = 0; i < j; ++i) {
    const double t = cs[i] * col[i] + sn[i] * col[i + 1];
    col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1];
    col[i] = t;
  }
  const double a = col[j], b = hn;
  double c, s;
  if (b == 0.0) {
    c = 1.0;
    s = 0.0;
  } else if (fabs(b) > fabs(a)) {
    const double tau = a / b;
    s = 1.0 / sqrt(1.0 + tau * tau);
    c = s * tau;
  } else {
    const double tau = b / a;
    c = 1.0 / sqrt(1.0 + tau * tau);
    s = c * tau;
  }
  const double rjj = c * a + s * b;
  if (rjj == 0.0) { // the column is discarded: j columns stay
    sc->jn = j;
    raise_done(sc, sc->k, 2);
    return;
  }
  col[j] = rjj;
  cs[j] = c;
  sn[j] = s;
  g[j + 1] = -s * g[j];
  g[j] = c * g[j];
  const int k = sc->k + 1;
  sc->k = k;
  sc->jn = j + 1;
  const double res = fabs(g[j + 1]);
  hist[k] = res;
  if (hn == 0.0) { // lucky breakdown
    raise_done(sc, k, 1);
    return;
  }
  if (res / hist[0] < sc->rtol || k == sc->kmax) {
    raise_done(sc, k, 0);
    return;
  }
  sc->inv = 1.0 / hn;
}

// single workgroup: y from the jn columns kept
__global__ __launch_bounds__(kBlock) void gmres_solve_y_kernel(
    const GmresScalars* sc, const double* __restrict__ R,
    const double* __restrict__ g, double* __restrict__ y)
{
  if (sc->finished || threadIdx.x != 0)
    return;
  const int jn = sc->jn;
  for (int i = jn - 1; i >= 0; --i) {
    double s = g[i];
    for (int l = i + 1; l < jn; ++l)
      s = s - R[(int64_t)l * kGmresMaxRestart + i] * y[l];
    y[i] = s / R[(int64_t)i * kGmresMaxRestart + i];
  }
}

// u = y_0 v_0 ; u = u + y_i v_i, i = 1..jn-1
template <bool NT>
__global__ __launch_bounds__(kBlock) void gmres_combine_kernel(
    int64_t n, const GmresScalars* sc, const double* __restrict__ V,
    int64_t stride, const double* __restrict__ y, double* __restrict__ u_out)
{
  if (sc->finished)
    return;
  const int jn = sc->jn;
  if (jn == 0)
    return;
  const double y0 = y[0];
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 t[kU];
    SPMV_FOR_LANE_ELEMS(i, n2) { t[u] = vload<NT>(V, i); }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      t[u].x = y0 * t[u].x;
      t[u].y = y0 * t[u].y;
    }
    axpy_groups<NT, false>(n2, base, V, stride, y, 1, jn, t);
    SPMV_FOR_LANE_ELEMS(i, n2) { vstore<NT>(u_out, i, t[u]); }
  }
  if (odd_tail(n)) {
    double t = y0 * V[n - 1];
    for (int i = 1; i < jn; ++i)
      t = t + y[i] * V[(int64_t)i * stride + n - 1];
    u_out[n - 1] = t;
  }
}

// x = x + z
template <bool NT>
__global__ __launch_bounds__(kBlock) void gmres_add_kernel(
    int64_t n, const GmresScalars* sc, const double* __restrict__ z,
    double* __restrict__ x)
{
  if (sc->finished || sc->jn == 0)
    return;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 zv[kU], xv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      zv[u] = vload<NT>(z, i);
      xv[u] = vload<NT>(x, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      xv[u].x = xv[u].x + zv[u].x;
      xv[u].y = xv[u].y + zv[u].y;
      vstore<NT>(x, i, xv[u]);
    }
  }
  if (odd_tail(n))
    x[n - 1] = x[n - 1] + z[n - 1];
}

// z = dinv * v: the diagonal right preconditioner
template <bool NT>
__global__ __launch_bounds__(kBlock) void gmres_diag_kernel(
    int64_t n, const double* __restrict__ dinv, const double* __restrict__ v,
    double* __restrict__ z)
{
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 dv[kU], vv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      dv[u] = vload<NT>(dinv, i);
      vv[u] = vload<NT>(v, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      vv[u].x = dv[u].x * vv[u].x;
      vv[u].y = dv[u].y * vv[u].y;
      vstore<NT>(z, i, vv[u]);
    }
  }
  if (odd_tail(n))
    z[n - 1] = dinv[n - 1] * v[n - 1];
}

__global__ void gmres_reset_kernel(GmresScalars* sc, double rtol, int kmax,
                                   int restart, double* small, int small_len)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    sc->rtol = rtol;
    sc->inv = 0.0;
    sc->ww = 0.0;
    sc->done = 0;
    sc->kstop = -1;
    sc->status = 0;
    sc->k = 0;
    sc->jn = 0;
    sc->finished = 0;
    sc->kmax = kmax;
    sc->restart = restart;
  }
  if (i < small_len)
    small[i] = 0.0;
}

// doubles of the small arrays in front of hist
constexpr size_t kGmresSmall = (size_t)6 * kGmresMaxRestart + 1
                               + (size_t)kGmresMaxRestart * kGmresMaxRestart;

} // namespace

extern "C" {

// ---- workspace ----------------------------------------------------------------
int spmv_hip_gmres_ws_create(spmv_hip_ctx* ctx, int kmax,
                             spmv_hip_gmres_ws** out)
{
  SPMV_REQUIRE(ctx && out && kmax >= 0);
  const size_t m = kGmresMaxRestart;
  return solver_ws_create(ctx, kmax, out, [&](spmv_hip_gmres_ws& w) {
    w.own.alloc(w.small, kGmresSmall + (size_t)kmax + 1);
    w.own.alloc(w.part, m * (size_t)ctx->dot_blocks);
    w.own.alloc(w.p_ww, ctx->dot_blocks);
    if (w.own.alloc(w.sc, 1) != 0)
      return;
    w.h = w.small;
    w.c = w.h + m;
    w.cs = w.c + m;
    w.sn = w.cs + m;
    w.y = w.sn + m;
    w.g = w.y + m; // m + 1
    w.R = w.g + m + 1;
    w.hist = w.R + m * m;
  });
}

int spmv_hip_gmres_ws_destroy(spmv_hip_gmres_ws* ws)
{
  return solver_ws_destroy(ws);
}

int spmv_hip_gmres_ws_reset(spmv_hip_gmres_ws* ws, double rtol, int kmax,
                            int restart, void* stream)
{
  SPMV_REQUIRE(ws && kmax >= 0 && kmax <= ws->kmax);
  SPMV_REQUIRE(restart >= 1 && restart <= kGmresMaxRestart);
  SPMV_SET_DEVICE(ws->ctx);
  const int n = (int)(kGmresSmall + (size_t)ws->kmax + 1);
  hipLaunchKernelGGL(gmres_reset_kernel, ws_reset_grid(n), dim3(kBlock), 0,
                     spmv_stream(ws->ctx, stream), ws->sc, rtol, kmax, restart,
                     ws->small, n);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_ws_capacity(const spmv_hip_gmres_ws* ws, int* kmax)
{
  return solver_ws_capacity(ws, kmax);
}

int spmv_hip_gmres_ws_done_flag(spmv_hip_gmres_ws* ws, const int32_t** done)
{
  SPMV_REQUIRE(ws && done);
  *done = &ws->sc->done;
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_ws_array(spmv_hip_gmres_ws* ws, int which, double** p,
                            int64_t* count)
{
  SPMV_REQUIRE(ws && p);
  const int64_t m = kGmresMaxRestart;
  double* q = nullptr;
  int64_t n = 0;
  switch (which) {
  case SPMV_HIP_GMRES_H: q = ws->h, n = m; break;
  case SPMV_HIP_GMRES_C: q = ws->c, n = m; break;
  case SPMV_HIP_GMRES_WW: q = &ws->sc->ww, n = 1; break;
  case SPMV_HIP_GMRES_CS: q = ws->cs, n = m; break;
  case SPMV_HIP_GMRES_SN: q = ws->sn, n = m; break;
  case SPMV_HIP_GMRES_G: q = ws->g, n = m + 1; break;
  case SPMV_HIP_GMRES_Y: q = ws->y, n = m; break;
  case SPMV_HIP_GMRES_R: q = ws->R, n = m * m; break;
  case SPMV_HIP_GMRES_HIST: q = ws->hist, n = (int64_t)ws->kmax + 1; break;
  case SPMV_HIP_GMRES_INV: q = &ws->sc->inv, n = 1; break;
  case SPMV_HIP_GMRES_PART: q = ws->part, n = m * ws->ctx->dot_blocks; break;
  case SPMV_HIP_GMRES_PART_WW: q = ws->p_ww, n = ws->ctx->dot_blocks; break;
  default: return SPMV_HIP_EINVAL;
  }
  *p = q;
  if (count)
    *count = n;
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_ws_read_async(spmv_hip_gmres_ws* ws,
                                 int32_t* host_done_kstop_status_k,
                                 double* host_hist, size_t host_hist_len,
                                 void* stream)
{
  SPMV_REQUIRE(ws);
  return ws_read_async(ws->ctx, stream, host_done_kstop_status_k,
                       &ws->sc->done, 4, host_hist, host_hist_len, ws->hist,
                       (size_t)ws->kmax + 1);
}

int spmv_hip_gmres_ws_set_state(spmv_hip_gmres_ws* ws, int k, int jn, int done,
                                int finished, void* stream)
{
  SPMV_REQUIRE(ws && k >= 0 && k <= ws->kmax && jn >= 0
               && jn <= kGmresMaxRestart);
  const int32_t words[6] = {done ? 1 : 0, done ? k : -1, 0, k, jn,
                            finished ? 1 : 0};
  return ws_put_words(ws->ctx, stream, &ws->sc->done, words, 6);
}

int spmv_hip_gmres_ws_get_state(spmv_hip_gmres_ws* ws, int32_t* host_words6,
                                void* stream)
{
  SPMV_REQUIRE(ws && host_words6);
  return ws_get_words(ws->ctx, stream, host_words6, &ws->sc->done, 6);
}

// ---- kernels ------------------------------------------------------------------
// the basis: nvec vectors of n doubles at V, V + stride, ...
#define SPMV_GMRES_CHECK_BASIS(ctx, ws, n, V, stride, nvec)                    \
  SPMV_REQUIRE((ctx) && (ws) && (ws)->ctx == (ctx) && (n) >= 0);               \
  SPMV_REQUIRE((nvec) >= 1 && (nvec) <= kGmresMaxRestart);                     \
  SPMV_REQUIRE((n) == 0 || ((V) && (stride) >= (n)));                          \
  SPMV_REQUIRE(((stride) & 1) == 0 && aligned16(V))

int spmv_hip_gmres_multi_dot_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws,
                                 int64_t n, const double* V, int64_t stride,
                                 int nvec, const double* w, void* stream)
{
  SPMV_GMRES_CHECK_BASIS(ctx, ws, n, V, stride, nvec);
  SPMV_REQUIRE((n == 0 || w) && aligned16(w));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, gmres_multi_dot_kernel, stream_grid_capped(ctx, n),
                 spmv_stream(ctx, stream), n, ws->sc, V, stride, nvec, w,
                 ws->part, ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_reduce(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws, int which,
                          int nvec, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_REQUIRE(which == SPMV_HIP_GMRES_H || which == SPMV_HIP_GMRES_C
               || which == SPMV_HIP_GMRES_WW);
  SPMV_REQUIRE(nvec >= 1 && nvec <= kGmresMaxRestart);
  SPMV_REQUIRE(which != SPMV_HIP_GMRES_WW || nvec == 1);
  SPMV_SET_DEVICE(ctx);
  const double* src = which == SPMV_HIP_GMRES_WW ? ws->p_ww : ws->part;
  double* dst = which == SPMV_HIP_GMRES_H   ? ws->h
                : which == SPMV_HIP_GMRES_C ? ws->c
                                            : &ws->sc->ww;
  hipLaunchKernelGGL(gmres_reduce_kernel, dim3(nvec), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, src, ctx->dot_blocks,
                     dst);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_multi_axpy_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws,
                                  int second, int64_t n, const double* V,
                                  int64_t stride, int nvec, double* w,
                                  void* stream)
{
  SPMV_GMRES_CHECK_BASIS(ctx, ws, n, V, stride, nvec);
  SPMV_REQUIRE((n == 0 || w) && aligned16(w));
  SPMV_SET_DEVICE(ctx);
  const int grid = stream_grid_capped(ctx, n);
  hipStream_t st = spmv_stream(ctx, stream);
  if (second)
    SPMV_LAUNCH_NT(ctx, n, gmres_multi_axpy2_kernel, grid, st, n, ws->sc, V,
                   stride, nvec, ws->c, ws->h, w, ws->p_ww, ctx->dot_blocks);
  else
    SPMV_LAUNCH_NT(ctx, n, gmres_multi_axpy1_kernel, grid, st, n, ws->sc, V,
                   stride, nvec, ws->h, w);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_givens(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws, int j,
                          int reduced, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_REQUIRE(j >= 0 && j < kGmresMaxRestart);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(gmres_givens_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, j, ws->p_ww,
                     ctx->dot_blocks, reduced ? 1 : 0, ws->h, ws->cs, ws->sn,
                     ws->g, ws->R, ws->hist);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_start(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws, int first,
                         int reduced, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(gmres_start_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, ws->p_ww,
                     ctx->dot_blocks, reduced ? 1 : 0, first ? 1 : 0, ws->g,
                     ws->hist);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_scale_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws, int64_t n,
                             const double* src, double* dst, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE((n == 0 || (src && dst)) && aligned16(src, dst));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, gmres_scale_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, ws->sc, src, dst);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_solve_y(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws,
                           void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(gmres_solve_y_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, ws->R, ws->g, ws->y);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_combine_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws,
                               int64_t n, const double* V, int64_t stride,
                               double* u, void* stream)
{
  SPMV_GMRES_CHECK_BASIS(ctx, ws, n, V, stride, 1);
  SPMV_REQUIRE((n == 0 || u) && aligned16(u));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, gmres_combine_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, ws->sc, V, stride, ws->y, u);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_add_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws, int64_t n,
                           const double* z, double* x, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE((n == 0 || (z && x)) && aligned16(z, x));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, gmres_add_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, ws->sc, z, x);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_residual_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws,
                                int64_t n, const double* b, const double* Ax,
                                double* r, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE((n == 0 || (b && r)) && aligned16(b, Ax, r));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, gmres_residual_kernel, stream_grid_capped(ctx, n),
                 spmv_stream(ctx, stream), n, ws->sc, b, Ax, r, ws->p_ww,
                 ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_gmres_diag_f64(spmv_hip_ctx* ctx, int64_t n, const double* dinv,
                            const double* v, double* z, void* stream)
{
  SPMV_REQUIRE(ctx && n >= 0);
  SPMV_REQUIRE((n == 0 || (dinv && v && z)) && aligned16(dinv, v, z));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT(ctx, n, gmres_diag_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, dinv, v, z);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
