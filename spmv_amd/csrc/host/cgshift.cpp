// spmv::cg_shifted for HipExecutor: see cg.h.
#include "cg.h"

#include "solver_common.h"

namespace spmv
{
using namespace detail;

// ---------------------------------------------------------------------------
// cg_shifted: see cg.h.  On the compute stream, M rows, ns shifts:
//     prologue: rules, workspace, aligned copy of X, ghost tail of p, ws_reset
//     r = p = p_s = b ; X = 0 ; partials of r.r ; [reduce(RRN) ; all-reduce]
//     start
//     k = 1..kmax, until the lagging poll sees `done`:
//       halo start of p ; q = A p with the partials of p.q
//       [reduce(PQ) ; all-reduce] ; update_r ; [reduce(RRN) ; all-reduce]
//       step ; update_xp(k)
//     epilogue: histories, copy back of an unaligned X, sync, times
// ---------------------------------------------------------------------------
CgShiftedWorkspace::~CgShiftedWorkspace() { release(); }

void CgShiftedWorkspace::release()
{
  release_common();
  drop_scalars(ws, kmax_cap, spmv_hip_cgs_ws_destroy);
  free_vectors({&r, &q, &p, &ps, &x, &dot2});
  m_cap = n_cap = ps_cap = x_cap = -1;
  ld = 0;
}

void CgShiftedWorkspace::ensure(int64_t M, int64_t N_padded, int ns, int kmax,
                                int len, bool need_x)
{
  open(SPMV_HIP_CGS_STATE_WORDS);
  if (!dot2)
    dot2 = _exec.alloc<double>(len);
  regrow_scalars(
      ws, kmax_cap, kmax, kmax > kmax_cap, spmv_hip_cgs_ws_destroy,
      [&](auto out) {
        return spmv_hip_cgs_ws_create(_exec.context(), kmax, out);
      },
      "spmv_hip_cgs_ws_create");
  regrow(m_cap, M, {&r, &q});
  regrow(n_cap, N_padded, {&p});
  // every solve lays its columns out afresh: the stride is this call's
  ld = (M + 1) / 2 * 2;
  regrow(ps_cap, ns * ld, {&ps});
  if (need_x)
    regrow(x_cap, ns * ld, {&x});
}

int cg_shifted(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
               const double* b, double* X, int64_t ldx, const double* shifts,
               int ns, int kmax, double rtol, std::vector<int>* iterations,
               std::vector<double>* rnorm_history, int* status,
               const CgOptions* options, CgStats* stats,
               CgShiftedWorkspace* workspace)
{
  // plain argument rules first: nothing below has touched a device yet
  cgs_check_rules(ns, kmax, A.row_map()->local_size(), ldx, shifts, b, X);
  const Dims dims = check_problem("cg_shifted", A, kmax);
  const int64_t M = dims.M, N_padded = dims.N_padded;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  const CgOptions opt = options ? *options : CgOptions();
  spmv_hip_ctx* ctx = exec.context();
  const int len = dot_partials_len(ctx);

  CgShiftedWorkspace own(exec);
  CgShiftedWorkspace& w = workspace ? *workspace : own;
  const bool x_aligned = is_aligned16(X) && (ns == 1 || (ldx & 1) == 0);
  w.ensure(M, N_padded, ns, kmax, len, !x_aligned);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  SolveStream guard(exec, w.stream); // every launch below goes to w.stream

  throw_on_error(spmv_hip_cgs_ws_reset(w.ws, rtol, kmax, ns, shifts, nullptr),
                 "spmv_hip_cgs_ws_reset");
  auto slot = [&](int which) {
    return ws_array(w.ws, spmv_hip_cgs_ws_array, which,
                    "spmv_hip_cgs_ws_array");
  };
  double* const slot_pq = slot(SPMV_HIP_CGS_PQ);
  double* const slot_rrn = slot(SPMV_HIP_CGS_RRN);
  double* const part_pq = slot(SPMV_HIP_CGS_PART_PQ);
  double* const part_rrn = slot(SPMV_HIP_CGS_PART_RRN);
  const bool several = comm.size() > 1;

  double* const Xi = x_aligned ? X : w.x;
  const int64_t ldi = x_aligned ? ldx : w.ld;
  exec.copy<double>(w.r, b, M);
  exec.copy<double>(w.p, b, M);
  for (int s = 0; s < ns; ++s) {
    exec.copy<double>(w.ps + s * w.ld, b, M);
    exec.memset<double>(Xi + s * ldi, 0, M);
  }
  // the ghost tail is defined here instead of relying on fresh pages
  if (N_padded > M)
    exec.memset<double>(w.p + M, 0, N_padded - M);
  exec.memset<double>(w.dot2, 0, len);
  for (int i = 0; i < SPMV_HIP_CGS_STATE_WORDS; ++i)
    w.flags[i] = 0;
  w.flags[1] = -1;

  auto read = ws_reader(w.ws, w.flags, spmv_hip_cgs_ws_read_async,
                        "spmv_hip_cgs_ws_read_async");
  // a partial array -> its slot, summed over the ranks
  auto finish = [&](int which, const double* part2, double* at) {
    if (!several)
      return; // the consumer adds the partials itself
    throw_on_error(spmv_hip_cgs_reduce(ctx, w.ws, which, part2, nullptr),
                   "spmv_hip_cgs_reduce");
    comm.reduce_sum(at, 1, w.stream);
  };

  throw_on_error(spmv_hip_dot_partial_f64(ctx, M, w.r, w.r, part_rrn, nullptr),
                 "spmv_hip_dot_partial_f64");
  finish(SPMV_HIP_CGS_RRN, nullptr, slot_rrn);
  throw_on_error(spmv_hip_cgs_start(ctx, w.ws, several, nullptr),
                 "spmv_hip_cgs_start");

  std::vector<void*>& timing_ev = w.timing_ev;
  LaggingPoll poll(exec, w, opt.poll_every, kmax);
  int k = 0;
  while (k < kmax && !poll.stopped) {
    ++k;
    col_l2g->update(w.p); // starts on the side stream
    void* ev1 = nullptr;
    if (opt.time_spmv) {
      ev1 = timing_ev[2 * (size_t)(k - 1) + 1];
      exec.record_event(timing_ev[2 * (size_t)(k - 1)], w.stream);
    }
    const bool fused = A.mult_dot(w.p, w.q, part_pq, w.dot2, ev1);
    if (!fused)
      throw_on_error(spmv_hip_dot_partial_f64(ctx, M, w.p, w.q, part_pq,
                                              nullptr),
                     "spmv_hip_dot_partial_f64");
    const double* part2 = fused ? w.dot2 : nullptr;
    finish(SPMV_HIP_CGS_PQ, part2, slot_pq);
    throw_on_error(spmv_hip_cgs_update_r_f64(ctx, w.ws, M, w.q, w.r, part2,
                                             several, nullptr),
                   "spmv_hip_cgs_update_r_f64");
    finish(SPMV_HIP_CGS_RRN, nullptr, slot_rrn);
    throw_on_error(spmv_hip_cgs_step(ctx, w.ws, several, nullptr),
                   "spmv_hip_cgs_step");
    throw_on_error(spmv_hip_cgs_update_xp_f64(ctx, w.ws, k, M, w.r, w.p, Xi, ldi,
                                              w.ps, w.ld, nullptr),
                   "spmv_hip_cgs_update_xp_f64");
    poll.step(k, read);
  }

  // final state: {done, kstop, status, its[8]} and the histories, hist_s at
  // s * (the WORKSPACE's capacity + 1): the stride read_history sized them by
  const std::vector<double> hist = read_history(
      spmv_hip_cgs_ws_capacity, w.ws, kmax, SPMV_HIP_CGS_MAX_NS, read);
  const size_t stride = hist.size() / SPMV_HIP_CGS_MAX_NS;
  if (Xi != X)
    for (int s = 0; s < ns; ++s)
      exec.copy<double>(X + s * ldx, Xi + s * ldi, M);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    if (opt.time_spmv)
      sum_spmv_times(ctx, timing_ev, 2 * (size_t)k, *stats);
  }

  // every way out of the loop raises `done` on the device; it is not raised
  // only when no step ran (kmax == 0) and b is not zero
  if (status)
    *status = w.flags[2];
  if (iterations)
    iterations->assign(ns, 0);
  if (rnorm_history)
    rnorm_history->assign((size_t)ns * ((size_t)kmax + 1), -1.0);
  int k_max = 0;
  for (int s = 0; s < ns; ++s) {
    const int ks = w.flags[3 + s];
    k_max = std::max(k_max, ks);
    if (iterations)
      (*iterations)[s] = ks;
    if (rnorm_history)
      std::copy(hist.begin() + s * stride, hist.begin() + s * stride + ks + 1,
                rnorm_history->begin() + (size_t)s * ((size_t)kmax + 1));
  }
  return k_max;
}

} // namespace spmv
