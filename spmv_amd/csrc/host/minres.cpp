// spmv::minres for HipExecutor: see cg.h.
#include "cg.h"

#include <utility>

#include "solver_common.h"

namespace spmv
{
using namespace detail;

// ---------------------------------------------------------------------------
// minres: see cg.h.  On the compute stream, Y = w.y with a preconditioner, the
// current r2 without one:
//     prologue: rules, workspace, aligned copies, ghost tail of v, ws_reset
//     r2 = b ; x = w2 = 0 ; [init: y = dinv*r2, partials of r2.y | M^-1 ; dot]
//     reduce(RY) ; all-reduce of 1 ; start ; update_xwv(0): v = y / beta1
//     k = 1..kmax, until the lagging poll sees `done`:
//       halo start of v ; Av = A v (+ fused v.Av share, else dot_partial)
//       several ranks: reduce(ALFA) ; all-reduce of 1
//       update_r (t over r1's buffer; the buffers swap) ; [M^-1 ; dot]
//       reduce(RY) ; all-reduce of 1 ; step ; update_xwv(k) (w over w1's
//       buffer; the buffers swap)
//     epilogue: history, copy back of an unaligned x, sync, times
// t is written over r1 and w over w1, so TWO buffers each rotate by pointer:
// the third vector of either recurrence never exists.
// ---------------------------------------------------------------------------
MinresWorkspace::~MinresWorkspace() { release(); }

void MinresWorkspace::release()
{
  release_common();
  drop_scalars(ws, kmax_cap, spmv_hip_minres_ws_destroy);
  free_vectors({&Av, &ra, &rb, &wa, &wb, &v, &y, &x, &dinv, &dot2});
  m_cap = n_cap = y_cap = x_cap = dinv_cap = -1;
}

void MinresWorkspace::ensure(int64_t M, int64_t N_padded, int kmax, int len,
                             bool need_y, bool need_x, bool need_dinv)
{
  open(4);
  if (!dot2)
    dot2 = _exec.alloc<double>(len);
  regrow_scalars(
      ws, kmax_cap, kmax, kmax > kmax_cap, spmv_hip_minres_ws_destroy,
      [&](auto out) {
        return spmv_hip_minres_ws_create(_exec.context(), kmax, out);
      },
      "spmv_hip_minres_ws_create");
  regrow(m_cap, M, {&Av, &ra, &rb, &wa, &wb});
  regrow(n_cap, N_padded, {&v});
  if (need_y)
    regrow(y_cap, M, {&y});
  if (need_x)
    regrow(x_cap, M, {&x});
  if (need_dinv)
    regrow(dinv_cap, M, {&dinv});
}

int minres(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
           const double* b, double* x, const MinresPreconditioner* precond,
           int kmax, double rtol, std::vector<double>* rnorm_history,
           const CgOptions* options, CgStats* stats, MinresWorkspace* workspace,
           int* status)
{
  // plain argument rules first: nothing below has touched a device yet
  const MinresPreconditioner pre
      = precond ? *precond : MinresPreconditioner();
  const int64_t rows = A.row_map()->local_size();
  minres_check_rules(kmax, pre.dinv != nullptr, pre.sgs != nullptr,
                     pre.amg != nullptr, pre.sgs ? pre.sgs->rows() : 0,
                     pre.sgs ? pre.sgs->negative_pivots() : 0,
                     pre.amg ? pre.amg->rows() : 0, rows, b, x, pre.dinv);
  const Dims dims = check_problem("minres", A, kmax);
  const int64_t M = dims.M, N_padded = dims.N_padded;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  const CgOptions opt = options ? *options : CgOptions();
  spmv_hip_ctx* ctx = exec.context();
  const int len = dot_partials_len(ctx);

  MinresWorkspace own(exec);
  MinresWorkspace& w = workspace ? *workspace : own;
  const bool applied = pre.sgs || pre.amg; // M^-1 is a call of its own
  const bool x_aligned = is_aligned16(x);
  const bool dinv_aligned = is_aligned16(pre.dinv);
  w.ensure(M, N_padded, kmax, len, pre.dinv || applied, !x_aligned,
           pre.dinv && !dinv_aligned);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  SolveStream guard(exec, w.stream); // every launch below goes to w.stream

  throw_on_error(spmv_hip_minres_ws_reset(w.ws, rtol, kmax, nullptr),
                 "spmv_hip_minres_ws_reset");
  auto slot = [&](int which) {
    return ws_array(w.ws, spmv_hip_minres_ws_array, which,
                    "spmv_hip_minres_ws_array");
  };
  double* const slot_alfa = slot(SPMV_HIP_MINRES_ALFA);
  double* const slot_ry = slot(SPMV_HIP_MINRES_RY);
  double* const part_alfa = slot(SPMV_HIP_MINRES_PART_ALFA);
  double* const part_ry = slot(SPMV_HIP_MINRES_PART_RY);
  const bool several = comm.size() > 1;

  const double* di = pre.dinv;
  if (pre.dinv && !dinv_aligned) { // the streaming kernels load 16 bytes at a time
    exec.copy<double>(w.dinv, pre.dinv, M);
    di = w.dinv;
  }
  double* const xi = x_aligned ? x : w.x;
  // r1 / r2 and w1 / w2: the buffers swap after every update
  double *r1 = w.ra, *r2 = w.rb, *w1 = w.wa, *w2 = w.wb;
  exec.copy<double>(r2, b, M);
  exec.memset<double>(xi, 0, M);
  exec.memset<double>(w1, 0, M);
  exec.memset<double>(w2, 0, M);
  // the ghost tail is defined here instead of relying on fresh pages
  if (N_padded > M)
    exec.memset<double>(w.v + M, 0, N_padded - M);
  exec.memset<double>(w.dot2, 0, len);
  w.flags[0] = 0;
  w.flags[1] = -1;
  w.flags[2] = 0;

  auto read = ws_reader(w.ws, w.flags, spmv_hip_minres_ws_read_async,
                        "spmv_hip_minres_ws_read_async");
  // y = M^-1 r2 where that is a call of its own, and the partials of r2.y
  auto apply_and_dot = [&]() {
    if (pre.sgs)
      sgs_apply(exec, *pre.sgs, r2, w.y);
    else
      amg_apply(exec, *pre.amg, r2, w.y);
    throw_on_error(spmv_hip_dot_partial_f64(ctx, M, r2, w.y, part_ry, nullptr),
                   "spmv_hip_dot_partial_f64");
  };
  // PART_RY -> the slot step / start read
  auto finish_ry = [&]() {
    throw_on_error(spmv_hip_minres_reduce(ctx, w.ws, SPMV_HIP_MINRES_RY, nullptr,
                                          nullptr),
                   "spmv_hip_minres_reduce");
    if (several)
      comm.reduce_sum(slot_ry, 1, w.stream);
  };
  // what update_xwv reads as y
  auto y_now = [&]() -> const double* { return pre.dinv || applied ? w.y : r2; };

  if (applied)
    apply_and_dot();
  else
    throw_on_error(spmv_hip_minres_init_f64(ctx, w.ws, M, r2, di, w.y, nullptr),
                   "spmv_hip_minres_init_f64");
  finish_ry();
  throw_on_error(spmv_hip_minres_start(ctx, w.ws, nullptr),
                 "spmv_hip_minres_start");
  throw_on_error(spmv_hip_minres_update_xwv_f64(ctx, w.ws, 0, M, w.v, w1, w2, xi,
                                                y_now(), nullptr),
                 "spmv_hip_minres_update_xwv_f64");

  std::vector<void*>& timing_ev = w.timing_ev;
  LaggingPoll poll(exec, w, opt.poll_every, kmax);
  int k = 0;
  while (k < kmax && !poll.stopped) {
    ++k;
    col_l2g->update(w.v); // starts on the side stream
    void* ev1 = nullptr;
    if (opt.time_spmv) {
      ev1 = timing_ev[2 * (size_t)(k - 1) + 1];
      exec.record_event(timing_ev[2 * (size_t)(k - 1)], w.stream);
    }
    const bool fused = A.mult_dot(w.v, w.Av, part_alfa, w.dot2, ev1);
    if (!fused)
      throw_on_error(spmv_hip_dot_partial_f64(ctx, M, w.v, w.Av, part_alfa,
                                              nullptr),
                     "spmv_hip_dot_partial_f64");
    const double* part2 = fused ? w.dot2 : nullptr;
    if (several) {
      throw_on_error(spmv_hip_minres_reduce(ctx, w.ws, SPMV_HIP_MINRES_ALFA,
                                            part2, nullptr),
                     "spmv_hip_minres_reduce");
      comm.reduce_sum(slot_alfa, 1, w.stream);
    }
    throw_on_error(spmv_hip_minres_update_r_f64(ctx, w.ws, M, w.Av, r1, r2, di,
                                                w.y, several, part2, !applied,
                                                nullptr),
                   "spmv_hip_minres_update_r_f64");
    std::swap(r1, r2); // t is the new r2
    if (applied)
      apply_and_dot();
    finish_ry();
    throw_on_error(spmv_hip_minres_step(ctx, w.ws, nullptr),
                   "spmv_hip_minres_step");
    throw_on_error(spmv_hip_minres_update_xwv_f64(ctx, w.ws, k, M, w.v, w1, w2,
                                                  xi, y_now(), nullptr),
                   "spmv_hip_minres_update_xwv_f64");
    std::swap(w1, w2); // w is the new w2
    poll.step(k, read);
  }

  // final state: {done, kstop, status} and the history
  const std::vector<double> hist
      = read_history(spmv_hip_minres_ws_capacity, w.ws, kmax, 1, read);
  if (xi != x)
    exec.copy<double>(x, xi, M);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    if (opt.time_spmv)
      sum_spmv_times(ctx, timing_ev, 2 * (size_t)k, *stats);
  }

  // every way out of the loop raises `done` on the device; it is not raised
  // only when no step ran (kmax == 0) and b is neither zero nor refused
  const int k_final = w.flags[0] != 0 ? w.flags[1] : 0;
  if (status)
    *status = w.flags[2];
  if (rnorm_history)
    rnorm_history->assign(hist.begin(), hist.begin() + k_final + 1);
  return k_final;
}

} // namespace spmv
