// spmv::idrs for HipExecutor: see cg.h.
#include "cg.h"

#include "solver_common.h"

namespace spmv
{
using namespace detail;

// ---------------------------------------------------------------------------
// idrs: see cg.h.  On the compute stream, M rows, ld = M rounded up to even:
//     prologue: rules, workspace, ws_reset ; r = b ; x = G = U = 0 ; ghost tail
//     sign_dot(r, with b.b) ; [reduce(HRR) ; all-reduce of s + 1] ; start
//     until kmax steps are enqueued or the lagging poll sees `done`:
//       q = 0..s-1:
//         FUSED (none / dinv): prep(q) writes u straight into the padded vector
//         stored B^-1: prep(STORE_V) ; u = B^-1 v ; prep(FROM_VH), in place
//         halo start of u ; t = A u ; sign_dot(t) ; [reduce(H) ; all-reduce of s]
//         biortho(q) ; update(q) ; [reduce(RR) ; all-reduce of 1] ; step(q)
//       om step: prep(PLAIN) or u = B^-1 r ; halo start ; t = A u ; omega_dot
//         [reduce(OM) ; all-reduce of 2] ; omega ; omega_update
//         [reduce(HRR) ; all-reduce of s + 1] ; step(s)
//     epilogue: history, sync, times
// ---------------------------------------------------------------------------
IdrsWorkspace::IdrsWorkspace(HipExecutor& exec)
    : SolverWorkspace(exec), cheb(exec)
{
}

IdrsWorkspace::~IdrsWorkspace() { release(); }

void IdrsWorkspace::release()
{
  release_common();
  drop_scalars(ws, kmax_cap, spmv_hip_idrs_ws_destroy);
  free_vectors({&r, &t, &u, &G, &U, &v, &dinv});
  m_cap = n_cap = gu_cap = v_cap = dinv_cap = -1;
  ld = 0;
}

void IdrsWorkspace::ensure(int64_t M, int64_t N_padded, int s, int kmax,
                           bool need_v, bool need_dinv)
{
  open(SPMV_HIP_IDRS_STATE_WORDS);
  regrow_scalars(
      ws, kmax_cap, kmax, kmax > kmax_cap, spmv_hip_idrs_ws_destroy,
      [&](auto out) {
        return spmv_hip_idrs_ws_create(_exec.context(), kmax, out);
      },
      "spmv_hip_idrs_ws_create");
  regrow(m_cap, M, {&r, &t});
  regrow(n_cap, N_padded, {&u});
  // every solve lays its columns out afresh: the stride is this call's
  ld = (M + 1) / 2 * 2;
  regrow(gu_cap, s * ld, {&G, &U});
  if (need_v)
    regrow(v_cap, M, {&v});
  if (need_dinv)
    regrow(dinv_cap, M, {&dinv});
}

void idrs_check_arguments(const GmresPreconditioner* M, int s, int kmax,
                          double kappa, int64_t rows, const double* b,
                          const double* x)
{
  const GmresPreconditioner none;
  const GmresPreconditioner& p = M ? *M : none;
  idrs_check_rules(s, kmax, kappa, p.dinv != nullptr, p.cheb_degree, p.lmin,
                   p.lmax, p.sgs != nullptr, p.amg != nullptr,
                   p.amg ? p.amg->rows() : p.sgs ? p.sgs->rows() : 0, rows, b, x,
                   p.dinv);
}

int idrs(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
         const double* b, double* x, const GmresPreconditioner* precond, int s,
         int kmax, double rtol, std::vector<double>* rnorm_history,
         const IdrsOptions* options, CgStats* stats, IdrsWorkspace* workspace,
         int* status)
{
  // plain argument rules first: nothing below has touched a device yet
  const IdrsOptions opt = options ? *options : IdrsOptions();
  idrs_check_arguments(precond, s, kmax, opt.kappa, A.row_map()->local_size(),
                       b, x);
  const Dims dims = check_problem("idrs", A, kmax);
  const int64_t M = dims.M, N_padded = dims.N_padded;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  const int64_t row0 = A.row_map()->global_offset();
  const GmresPreconditioner pre = precond ? *precond : GmresPreconditioner();
  spmv_hip_ctx* ctx = exec.context();

  IdrsWorkspace own(exec);
  IdrsWorkspace& w = workspace ? *workspace : own;
  const bool cheb = pre.cheb_degree >= 1;
  const bool stored = cheb || pre.sgs || pre.amg;
  const double* const fused_dinv = stored ? nullptr : pre.dinv;
  const bool copy_dinv = cheb && pre.dinv && !is_aligned16(pre.dinv);
  w.ensure(M, N_padded, s, kmax, stored, copy_dinv);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  SolveStream guard(exec, w.stream); // every launch below goes to w.stream

  throw_on_error(spmv_hip_idrs_ws_reset(w.ws, rtol, opt.kappa, kmax, s, opt.seed,
                                        nullptr),
                 "spmv_hip_idrs_ws_reset");
  const double* cheb_dinv = pre.dinv;
  if (copy_dinv) { // chebyshev_apply loads 16 bytes at a time
    exec.copy<double>(w.dinv, pre.dinv, M);
    cheb_dinv = w.dinv;
  }
  // x is the iterate itself: the kernels take any 8-byte alignment with the
  // same bits.  G and U start as zeros: step q reads columns q..s-1 of the
  // previous cycle.
  exec.copy<double>(w.r, b, M);
  exec.memset<double>(x, 0, M);
  exec.memset<double>(w.G, 0, s * w.ld);
  exec.memset<double>(w.U, 0, s * w.ld);
  // the ghost tail is defined here instead of relying on fresh pages
  exec.memset<double>(w.u, 0, N_padded);
  for (int i = 0; i < SPMV_HIP_IDRS_STATE_WORDS; ++i)
    w.flags[i] = 0;
  w.flags[1] = -1;

  auto read = ws_reader(w.ws, w.flags, spmv_hip_idrs_ws_read_async,
                        "spmv_hip_idrs_ws_read_async");
  double* red = nullptr;
  throw_on_error(spmv_hip_idrs_ws_array(w.ws, SPMV_HIP_IDRS_RED, &red, nullptr),
                 "spmv_hip_idrs_ws_array");
  const bool several = comm.size() > 1;
  // partial rows -> their slots, summed over the ranks
  auto finish = [&](int which, int first, int count) {
    if (!several)
      return; // the consumer adds the partials itself
    throw_on_error(spmv_hip_idrs_reduce(ctx, w.ws, which, nullptr),
                   "spmv_hip_idrs_reduce");
    comm.reduce_sum(red + first, count, w.stream);
  };
  auto prep = [&](int q, int mode, const double* src, double* out) {
    throw_on_error(spmv_hip_idrs_prep_f64(ctx, w.ws, q, mode, M, src, w.G, w.U,
                                          w.ld, fused_dinv, out, nullptr),
                   "spmv_hip_idrs_prep_f64");
  };
  // w.u (padded) = B^-1 src for a stored preconditioner
  auto apply_stored = [&](const double* src) {
    apply_stored_preconditioner(exec, A, pre, cheb_dinv, &w.cheb, src, w.u);
  };
  std::vector<void*>& timing_ev = w.timing_ev;
  int steps = 0; // products enqueued
  // t = A u, timed
  auto product = [&]() {
    col_l2g->update(w.u); // starts on the side stream
    if (opt.time_spmv)
      exec.record_event(timing_ev[2 * (size_t)(steps - 1)], w.stream);
    A.mult(w.u, w.t);
    if (opt.time_spmv)
      exec.record_event(timing_ev[2 * (size_t)(steps - 1) + 1], w.stream);
  };

  throw_on_error(spmv_hip_idrs_sign_dot_f64(ctx, w.ws, M, row0, w.r, 1, nullptr),
                 "spmv_hip_idrs_sign_dot_f64");
  finish(SPMV_HIP_IDRS_REDUCE_HRR, 0, s + 1);
  throw_on_error(spmv_hip_idrs_start(ctx, w.ws, several, nullptr),
                 "spmv_hip_idrs_start");

  LaggingPoll poll(exec, w, opt.poll_every, kmax);
  while (steps < kmax && !poll.stopped) {
    for (int q = 0; q < s && steps < kmax && !poll.stopped; ++q) {
      ++steps;
      if (!stored) {
        prep(q, SPMV_HIP_IDRS_FUSED, w.r, w.u);
      } else {
        prep(q, SPMV_HIP_IDRS_STORE_V, w.r, w.v);
        apply_stored(w.v);
        prep(q, SPMV_HIP_IDRS_FROM_VH, w.u, w.u);
      }
      product();
      throw_on_error(spmv_hip_idrs_sign_dot_f64(ctx, w.ws, M, row0, w.t, 0,
                                                nullptr),
                     "spmv_hip_idrs_sign_dot_f64");
      finish(SPMV_HIP_IDRS_REDUCE_H, 0, s);
      throw_on_error(spmv_hip_idrs_biortho(ctx, w.ws, q, several, nullptr),
                     "spmv_hip_idrs_biortho");
      throw_on_error(spmv_hip_idrs_update_f64(ctx, w.ws, q, M, w.t, w.u, w.G,
                                              w.U, w.ld, w.r, x, nullptr),
                     "spmv_hip_idrs_update_f64");
      finish(SPMV_HIP_IDRS_REDUCE_RR, s, 1);
      throw_on_error(spmv_hip_idrs_step(ctx, w.ws, q, several, nullptr),
                     "spmv_hip_idrs_step");
      poll.step(steps, read);
    }
    if (steps >= kmax || poll.stopped)
      break;
    ++steps;
    if (!stored)
      prep(s, SPMV_HIP_IDRS_PLAIN, w.r, w.u);
    else
      apply_stored(w.r);
    product();
    throw_on_error(spmv_hip_idrs_omega_dot_f64(ctx, w.ws, M, w.t, w.r, nullptr),
                   "spmv_hip_idrs_omega_dot_f64");
    finish(SPMV_HIP_IDRS_REDUCE_OM, 9, 2);
    throw_on_error(spmv_hip_idrs_omega(ctx, w.ws, several, nullptr),
                   "spmv_hip_idrs_omega");
    throw_on_error(spmv_hip_idrs_omega_update_f64(ctx, w.ws, M, row0, w.t, w.u,
                                                  w.r, x, nullptr),
                   "spmv_hip_idrs_omega_update_f64");
    finish(SPMV_HIP_IDRS_REDUCE_HRR, 0, s + 1);
    throw_on_error(spmv_hip_idrs_step(ctx, w.ws, s, several, nullptr),
                   "spmv_hip_idrs_step");
    poll.step(steps, read);
  }

  // final state: {done, kstop, status, k} and the history
  const std::vector<double> hist
      = read_history(spmv_hip_idrs_ws_capacity, w.ws, kmax, 1, read);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    if (opt.time_spmv)
      sum_spmv_times(ctx, timing_ev, 2 * (size_t)steps, *stats);
  }

  // every way out of the loop raises `done` on the device
  const int k_final = w.flags[0] != 0 ? w.flags[1] : w.flags[3];
  if (status)
    *status = w.flags[2];
  if (rnorm_history)
    rnorm_history->assign(hist.begin(), hist.begin() + k_final + 1);
  return k_final;
}

} // namespace spmv
