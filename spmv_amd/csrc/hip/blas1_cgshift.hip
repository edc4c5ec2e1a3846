// BLAS-1 kernels of spmv::cg_shifted (gfx950): multi-shift CG (Frommer;
// Jegerlehner 1996) for (A + sigma_s I) x_s = b, s < ns <= 8, on the Krylov
// space of the seed A, in the launch structure of blas1_lsqr.hip.  The
// recurrence is spelled out in host/cg.h.  One iteration, `.` the global dot
// product:
//
//   (mult_dot)  q = A p with the partials of p.q
//   update_r    p.q from the partials (one rank: every workgroup adds them
//               itself, in the reducer's order) or from the reducer's slot;
//               a = rr / pq; r = r - a * q; partials of r.r.  Not (pq > 0):
//               nothing is written, step ends the solve
//   reduce      partials -> the slot of pq or of rrn, one workgroup (several
//               ranks only)
//   step        one workgroup adds the partials of r.r in the reducer's order
//               (or reads the slot); its thread 0 then does the scalar
//               arithmetic of every ACTIVE shift, the stop tests, the
//               histories, and leaves two compacted lists: `upd`, the shifts
//               update_xp moves, and `act`, the shifts the next step moves
//   update_xp   one pass: a thread's tile of r and of the seed's p in
//               registers; for every shift of `upd`: x_s += cx_s * p_s and,
//               unless s stopped in this step, p_s = zeta_s * r + cp_s * p_s;
//               then the seed's p = r + bn * p.  A shift that is not in `upd`
//               is neither read nor written.
//
// and once per solve: the dot-partials kernel of blas1.hip on r = b, start.
//
// Layout.  x_s = X + s * ldx and p_s = PS + s * ldp are CONTIGUOUS vectors: a
// stopped shift costs nothing, where an interleaved block (blas1_block.hip)
// would carry its column through every cache line.
//
// Alignment.  Vectors whose addresses are all multiples of 16 (even ldx, ldp)
// are walked with 16-byte accesses; any other set of 8-byte aligned vectors
// with two 8-byte accesses per element, the same elements in the same threads,
// so the bits do not depend on the alignment.
//
// Stop protocol.  `done` is raised by step or start.  After it update_r,
// reduce, start and step return at once.  update_xp of iteration k runs when,
// and only when, the state says that step k completed (sc->k == k): the step
// that raised `done` still gets its x updates, exactly once, and every later
// launch finds k behind its own.  After `done` no p is formed.
//
// Built with -ffp-contract=off: every product, sum, difference, quotient and
// square root is a rounding of its own.  Streaming shape: blas1_stream.h.
#include "common.h"
#include "blas1_stream.h"
#include "cgs_ws.h"

#include <cmath>
#include <cstddef>

namespace
{

__device__ __forceinline__ void raise_done(CgsScalars* sc, int kstop, int status)
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

// r is read and written at the same index by the same thread: no __restrict__
template <bool NT, bool AL>
__global__ __launch_bounds__(kBlock) void cgs_update_r_kernel(
    int64_t n, CgsScalars* sc, const double* __restrict__ q, double* r,
    const double* __restrict__ p_pq, const double* __restrict__ p_pq2, int len,
    int reduced, double* __restrict__ p_rrn)
{
  __shared__ double s_red[kBlock / 64];
  __shared__ double s_bcast;
  if (sc->done)
    return;
  double pq;
  if (reduced) {
    pq = sc->pq;
  } else {
    // (nobody reads the slot in this launch: step does)
    pq = consume_partials(p_pq, p_pq2, len, s_red, &s_bcast);
    if (blockIdx.x == 0 && threadIdx.x == 0)
      sc->pq = pq;
  }
  if (!(pq > 0.0)) // (a NaN too) uniform across the grid; step raises `done`
    return;
  const double a = sc->rr / pq;
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 qv[kU], rv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      qv[u] = ld<NT, AL>(q, i);
      rv[u] = ld<NT, AL>(r, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      f64x2 t;
      t.x = rv[u].x - a * qv[u].x;
      t.y = rv[u].y - a * qv[u].y;
      st<NT, AL>(r, i, t);
      acc += t.x * t.x;
      acc += t.y * t.y;
    }
  }
  if (odd_tail(n)) {
    const double t = r[n - 1] - a * q[n - 1];
    r[n - 1] = t;
    acc += t * t;
  }
  const double s = spmv_block_sum(acc, s_red);
  if (threadIdx.x == 0)
    p_rrn[blockIdx.x] = s;
  clear_partials_tail(p_rrn, len);
}

// one workgroup: partials (+ the remote block's share of p.q) -> the slot
__global__ __launch_bounds__(kBlock) void cgs_reduce_kernel(
    const CgsScalars* sc, const double* __restrict__ partials,
    const double* __restrict__ partials2, int len, double* __restrict__ dst)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double s = sum_partials(partials, partials2, len, s_red);
  if (threadIdx.x == 0)
    *dst = s;
}

// one workgroup, thread 0: rr = r0.r0, hist_s[0] of every shift
__global__ __launch_bounds__(kBlock) void cgs_start_kernel(
    CgsScalars* sc, const double* __restrict__ p_rrn, int len, int reduced,
    double* __restrict__ hist, int stride)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done) // (uniform: thread 0 raises it behind the sum's barrier)
    return;
  double rr = 0.0;
  if (!reduced)
    rr = sum_partials(p_rrn, nullptr, len, s_red);
  if (threadIdx.x != 0)
    return;
  if (reduced)
    rr = sc->rrn;
  else
    sc->rrn = rr;
  sc->rr = rr;
  const double h0 = sqrt(rr);
  sc->hist0 = h0;
  for (int s = 0; s < sc->ns; ++s)
    hist[(size_t)s * stride] = h0;
  if (rr == 0.0) // x_s = 0 is the answer of every shift
    raise_done(sc, 0, 0);
}

// one workgroup, thread 0: the scalar part of an iteration.  The rtol
// comparison is written so that a NaN goes on.
__global__ __launch_bounds__(kBlock) void cgs_step_kernel(
    CgsScalars* sc, const double* __restrict__ p_rrn, int len, int reduced,
    double* __restrict__ hist, int stride)
{
  __shared__ double s_red[kBlock / 64];
  if (sc->done)
    return;
  const double pq = sc->pq;
  const bool broke = !(pq > 0.0); // uniform
  double rrn = 0.0;
  if (!broke && !reduced)
    rrn = sum_partials(p_rrn, nullptr, len, s_red);
  if (threadIdx.x != 0)
    return;
  const int k = sc->k;
  if (broke) { // the seed is not positive definite: X stays the last iterate
    raise_done(sc, k, 1);
    return;
  }
  if (k >= sc->kmax) { // (no room in the histories: the host never asks)
    raise_done(sc, k, 0);
    return;
  }
  if (reduced)
    rrn = sc->rrn;
  else
    sc->rrn = rrn;
  const double rr = sc->rr, a_old = sc->a_old, b_old = sc->b_old;
  const double rtol = sc->rtol, hist0 = sc->hist0;
  const double a = rr / pq;
  const double bn = rrn / rr;
  const double rnorm = sqrt(rrn);
  const double ab = a * b_old;
  const int n_act = sc->n_act;
  int na = 0;
  for (int j = 0; j < n_act; ++j) {
    const int s = sc->act[j];
    const double rho = sc->rho[s];
    const double rn
        = a_old / (ab * (1.0 - rho) + a_old * (1.0 + sc->sigma[s] * a));
    const double z = sc->zeta[s] * rn;
    sc->cx[s] = a * rn;
    sc->zeta[s] = z;
    sc->rho[s] = rn;
    const double h = fabs(z) * rnorm;
    hist[(size_t)s * stride + k + 1] = h;
    sc->its[s] = k + 1;
    if (h / hist0 < rtol) { // s stops: x_s moves, p_s stays
      sc->upd[j] = s;
    } else {
      sc->cp[s] = bn * (rn * rn);
      sc->upd[j] = s | 8;
      sc->act[na++] = s; // (na <= j: what is overwritten has been read)
    }
  }
  sc->n_upd = n_act;
  sc->n_act = na;
  sc->bn = bn;
  sc->a_old = a;
  sc->b_old = bn;
  sc->rr = rrn;
  sc->k = k + 1;
  if (na == 0 || rrn == 0.0 || k + 1 == sc->kmax)
    raise_done(sc, k + 1, 0);
}

// The hot kernel.  x_s and p_s are read and written at the same index by the
// same thread; p likewise.
template <bool NT, bool AL>
__global__ __launch_bounds__(kBlock) void cgs_update_xp_kernel(
    int64_t n, const CgsScalars* __restrict__ sc, int k,
    const double* __restrict__ r, double* p, double* X, int64_t ldx, double* PS,
    int64_t ldp)
{
  if (sc->k != k)
    return;
  const bool go_on = sc->done == 0;
  const int n_upd = sc->n_upd;
  const double bn = sc->bn;
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 rv[kU], pv[kU];
    if (go_on) {
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        rv[u] = ld<NT, AL>(r, i);
        pv[u] = ld<NT, AL>(p, i);
      }
    }
    for (int j = 0; j < n_upd; ++j) {
      const int w = sc->upd[j];
      const int s = w & 7;
      const bool with_p = go_on && (w & 8) != 0;
      double* const xs = X + s * ldx;
      double* const ps = PS + s * ldp;
      const double cx = sc->cx[s], z = sc->zeta[s], cp = sc->cp[s];
      f64x2 xv[kU], sv[kU];
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        xv[u] = ld<NT, AL>(xs, i);
        sv[u] = ld<NT, AL>(ps, i);
      }
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        xv[u].x = xv[u].x + cx * sv[u].x;
        xv[u].y = xv[u].y + cx * sv[u].y;
        st<NT, AL>(xs, i, xv[u]);
        if (with_p) {
          f64x2 t;
          t.x = z * rv[u].x + cp * sv[u].x;
          t.y = z * rv[u].y + cp * sv[u].y;
          st<NT, AL>(ps, i, t);
        }
      }
    }
    if (go_on) {
      SPMV_FOR_LANE_ELEMS(i, n2)
      {
        f64x2 t;
        t.x = rv[u].x + bn * pv[u].x;
        t.y = rv[u].y + bn * pv[u].y;
        st<NT, AL>(p, i, t);
      }
    }
  }
  if (odd_tail(n)) {
    const int64_t e = n - 1;
    const double re = go_on ? r[e] : 0.0;
    for (int j = 0; j < n_upd; ++j) {
      const int w = sc->upd[j];
      const int s = w & 7;
      double* const xs = X + s * ldx;
      double* const ps = PS + s * ldp;
      const double p0 = ps[e];
      xs[e] = xs[e] + sc->cx[s] * p0;
      if (go_on && (w & 8) != 0)
        ps[e] = sc->zeta[s] * re + sc->cp[s] * p0;
    }
    if (go_on)
      p[e] = re + bn * p[e];
  }
}

struct CgsShifts {
  double v[kCgsMaxNs];
};

__global__ void cgs_reset_kernel(CgsScalars* sc, double rtol, int kmax, int ns,
                                 CgsShifts shifts, double* hist, int hist_len)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    double* d = reinterpret_cast<double*>(sc);
    for (int j = 0; j < kCgsDoubles; ++j)
      d[j] = 0.0;
    int32_t* w = &sc->done;
    for (int j = 0; j < kCgsWords; ++j)
      w[j] = 0;
    sc->rtol = rtol;
    sc->a_old = 1.0;
    for (int s = 0; s < ns; ++s) {
      sc->sigma[s] = shifts.v[s];
      sc->zeta[s] = 1.0;
      sc->rho[s] = 1.0;
      sc->act[s] = s;
    }
    sc->kstop = -1;
    sc->kmax = kmax;
    sc->ns = ns;
    sc->n_act = ns;
  }
  if (i < hist_len)
    hist[i] = 0.0;
}

static_assert(offsetof(CgsScalars, done) == kCgsDoubles * sizeof(double),
              "the doubles of CgsScalars come first");
static_assert(sizeof(CgsScalars)
                  == kCgsDoubles * sizeof(double) + kCgsWords * sizeof(int32_t),
              "the words of CgsScalars follow without a gap");

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
int spmv_hip_cgs_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_cgs_ws** out)
{
  SPMV_REQUIRE(ctx && out && kmax >= 0);
  return solver_ws_create(ctx, kmax, out, [&](spmv_hip_cgs_ws& w) {
    w.own.alloc(w.hist, kCgsMaxNs * ((size_t)kmax + 1));
    w.own.alloc(w.p_pq, ctx->dot_blocks);
    w.own.alloc(w.p_rrn, ctx->dot_blocks);
    w.own.alloc(w.sc, 1);
  });
}

int spmv_hip_cgs_ws_destroy(spmv_hip_cgs_ws* ws)
{
  return solver_ws_destroy(ws);
}

int spmv_hip_cgs_ws_reset(spmv_hip_cgs_ws* ws, double rtol, int kmax, int ns,
                          const double* host_shifts, void* stream)
{
  SPMV_REQUIRE(ws && kmax >= 0 && kmax <= ws->kmax);
  SPMV_REQUIRE(ns >= 1 && ns <= kCgsMaxNs && host_shifts);
  SPMV_SET_DEVICE(ws->ctx);
  CgsShifts sh;
  for (int s = 0; s < kCgsMaxNs; ++s)
    sh.v[s] = s < ns ? host_shifts[s] : 0.0;
  ws->ns = ns;
  const int n = kCgsMaxNs * (ws->kmax + 1);
  hipLaunchKernelGGL(cgs_reset_kernel, ws_reset_grid(n), dim3(kBlock), 0,
                     spmv_stream(ws->ctx, stream), ws->sc, rtol, kmax, ns, sh,
                     ws->hist, n);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cgs_ws_capacity(const spmv_hip_cgs_ws* ws, int* kmax)
{
  return solver_ws_capacity(ws, kmax);
}

int spmv_hip_cgs_ws_array(spmv_hip_cgs_ws* ws, int which, double** p,
                          int64_t* count)
{
  SPMV_REQUIRE(ws && p);
  double* q = nullptr;
  int64_t n = 0;
  switch (which) {
  case SPMV_HIP_CGS_PQ: q = &ws->sc->pq, n = 1; break;
  case SPMV_HIP_CGS_RRN: q = &ws->sc->rrn, n = 1; break;
  case SPMV_HIP_CGS_HIST:
    q = ws->hist, n = (int64_t)kCgsMaxNs * ((int64_t)ws->kmax + 1);
    break;
  case SPMV_HIP_CGS_PART_PQ: q = ws->p_pq, n = ws->ctx->dot_blocks; break;
  case SPMV_HIP_CGS_PART_RRN: q = ws->p_rrn, n = ws->ctx->dot_blocks; break;
  case SPMV_HIP_CGS_SCALARS:
    q = reinterpret_cast<double*>(ws->sc), n = kCgsDoubles;
    break;
  default: return SPMV_HIP_EINVAL;
  }
  *p = q;
  if (count)
    *count = n;
  return SPMV_HIP_OK;
}

int spmv_hip_cgs_ws_read_async(spmv_hip_cgs_ws* ws, int32_t* host_state,
                               double* host_hist, size_t host_hist_len,
                               void* stream)
{
  SPMV_REQUIRE(ws);
  return ws_read_async(ws->ctx, stream, host_state, &ws->sc->done,
                       SPMV_HIP_CGS_STATE_WORDS, host_hist, host_hist_len,
                       ws->hist, kCgsMaxNs * ((size_t)ws->kmax + 1));
}

int spmv_hip_cgs_ws_set_words(spmv_hip_cgs_ws* ws, const int32_t* host_words,
                              void* stream)
{
  SPMV_REQUIRE(ws && host_words);
  // the words update_xp turns into addresses are checked here
  const int32_t* w = host_words;
  const int32_t k = w[3 + kCgsMaxNs], kmax = w[4 + kCgsMaxNs];
  const int32_t ns = w[5 + kCgsMaxNs], n_act = w[6 + kCgsMaxNs];
  const int32_t n_upd = w[7 + kCgsMaxNs];
  SPMV_REQUIRE(k >= 0 && kmax >= k && kmax <= ws->kmax && ns == ws->ns);
  SPMV_REQUIRE(n_act >= 0 && n_act <= ns && n_upd >= 0 && n_upd <= ns);
  for (int j = 0; j < n_act; ++j)
    SPMV_REQUIRE(w[8 + kCgsMaxNs + j] >= 0 && w[8 + kCgsMaxNs + j] < ns);
  for (int j = 0; j < n_upd; ++j)
    SPMV_REQUIRE(w[8 + 2 * kCgsMaxNs + j] >= 0
                 && (w[8 + 2 * kCgsMaxNs + j] & 7) < ns
                 && w[8 + 2 * kCgsMaxNs + j] < 16);
  return ws_put_words(ws->ctx, stream, &ws->sc->done, host_words, kCgsWords);
}

int spmv_hip_cgs_ws_get_words(spmv_hip_cgs_ws* ws, int32_t* host_words,
                              void* stream)
{
  SPMV_REQUIRE(ws && host_words);
  return ws_get_words(ws->ctx, stream, host_words, &ws->sc->done, kCgsWords);
}

// ---- kernels ------------------------------------------------------------------
int spmv_hip_cgs_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_cgs_ws* ws, int64_t n,
                              const double* q, double* r,
                              const double* pq_partials2, int reduced,
                              void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx && n >= 0);
  SPMV_REQUIRE((n == 0 || (q && r && q != r)) && aligned8(q, r));
  SPMV_SET_DEVICE(ctx);
  SPMV_LAUNCH_NT_AL(ctx, n, aligned16(q, r), cgs_update_r_kernel,
                    stream_grid_capped(ctx, n), spmv_stream(ctx, stream), n,
                    ws->sc, q, r, ws->p_pq, pq_partials2, ctx->dot_blocks,
                    reduced ? 1 : 0, ws->p_rrn);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cgs_reduce(spmv_hip_ctx* ctx, spmv_hip_cgs_ws* ws, int which,
                        const double* partials2, void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_REQUIRE(which == SPMV_HIP_CGS_PQ
               || (which == SPMV_HIP_CGS_RRN && !partials2));
  SPMV_SET_DEVICE(ctx);
  const bool pq = which == SPMV_HIP_CGS_PQ;
  hipLaunchKernelGGL(cgs_reduce_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, pq ? ws->p_pq : ws->p_rrn,
                     partials2, ctx->dot_blocks,
                     pq ? &ws->sc->pq : &ws->sc->rrn);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cgs_start(spmv_hip_ctx* ctx, spmv_hip_cgs_ws* ws, int reduced,
                       void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(cgs_start_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, ws->p_rrn,
                     ctx->dot_blocks, reduced ? 1 : 0, ws->hist, ws->kmax + 1);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cgs_step(spmv_hip_ctx* ctx, spmv_hip_cgs_ws* ws, int reduced,
                      void* stream)
{
  SPMV_REQUIRE(ctx && ws && ws->ctx == ctx);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(cgs_step_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->sc, ws->p_rrn,
                     ctx->dot_blocks, reduced ? 1 : 0, ws->hist, ws->kmax + 1);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_cgs_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_cgs_ws* ws, int k,
                               int64_t n, const double* r, double* p, double* X,
                               int64_t ldx, double* PS, int64_t ldp,
                               void* stream)
{
  SPMV_REQUIRE_WS_K(ctx, ws, k, 1);
  SPMV_REQUIRE(ctx && n >= 0 && ws->ns >= 1);
  SPMV_REQUIRE((n == 0 || (r && p && X && PS)) && aligned8(r, p, X, PS));
  // the columns the kernel addresses: ws->ns of them, ldx and ldp apart
  SPMV_REQUIRE(ldx >= n && ldp >= n);
  SPMV_REQUIRE(n == 0 || (r != p && r != X && r != PS && p != X && p != PS
                          && X != PS));
  SPMV_SET_DEVICE(ctx);
  const bool al = aligned16(r, p, X, PS)
                  && (ws->ns == 1 || ((ldx | ldp) & 1) == 0);
  SPMV_LAUNCH_NT_AL(ctx, n, al, cgs_update_xp_kernel, stream_grid(ctx, n),
                    spmv_stream(ctx, stream), n, ws->sc, k, r, p, X, ldx, PS,
                    ldp);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
