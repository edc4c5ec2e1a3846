// spmv::bicgstab for HipExecutor: see cg.h.
#include "cg.h"

#include "solver_common.h"

namespace spmv
{
using namespace detail;

// ---------------------------------------------------------------------------
// bicgstab: see cg.h.  Per iteration (compute stream), PH / SH being ph / sh
// with a dinv and p / s without:
//     halo start of PH on the map's side stream ; v = A PH (Matrix::mult)
//     one rank, consumer_reductions:            otherwise:
//       dot_rv                                    dot_rv
//       update_s_cs   (rv[k]; s, sh)              reduce_rv ; all-reduce of 1
//                                                 update_s
//     halo start of SH ; t = A SH
//       dot_ts_tt                                 dot_ts_tt
//       update_xr_cs  ({ts,tt}[k]; x; r;          reduce_ts_tt ; all-reduce of 2
//                      r.r, rhat.r)               update_xr
//       update_p_cs   ({rr,rho}[k]; stop; p, ph)  reduce_rr_rho ; all-reduce of 2
//                                                 update_p
// 2 SpMV + 5 (or 8) launches; beside the SpMVs 23 vector passes with a dinv
// (dot_rv 2, update_s 5, dot_ts_tt 2, update_xr 8, update_p 6) and 18 without
// (2, 3, 2, 7, 4), where cg() without defer_x streams 8.
// ---------------------------------------------------------------------------
BicgstabWorkspace::~BicgstabWorkspace() { release(); }

void BicgstabWorkspace::release()
{
  release_common();
  drop_scalars(ws, kmax_cap, spmv_hip_bicg_ws_destroy);
  free_vectors({&r, &rhat, &v, &t, &p, &s, &ph, &sh, &x, &dinv});
  m_cap = n_cap = h_cap = x_cap = dinv_cap = -1;
}

void BicgstabWorkspace::ensure(int64_t M, int64_t N_padded, int kmax,
                               bool need_x, bool need_dinv, bool need_h)
{
  open(4);
  regrow_scalars(
      ws, kmax_cap, kmax, kmax > kmax_cap, spmv_hip_bicg_ws_destroy,
      [&](auto out) {
        return spmv_hip_bicg_ws_create(_exec.context(), kmax, out);
      },
      "spmv_hip_bicg_ws_create");
  regrow(m_cap, M, {&r, &rhat, &v, &t});
  regrow(n_cap, N_padded, {&p, &s});
  if (need_h)
    regrow(h_cap, N_padded, {&ph, &sh});
  if (need_x)
    regrow(x_cap, M, {&x});
  if (need_dinv)
    regrow(dinv_cap, M, {&dinv});
}
int bicgstab(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
             const double* b, double* x, const double* dinv, int kmax,
             double rtol, std::vector<double>* rnorm_history,
             const CgOptions* options, CgStats* stats,
             BicgstabWorkspace* workspace, int* status)
{
  const Dims dims = check_problem("bicgstab", A, kmax);
  const int64_t M = dims.M, N_padded = dims.N_padded;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  const CgOptions opt = options ? *options : CgOptions();
  spmv_hip_ctx* ctx = exec.context();
  // x is the iterate from the first kernel on: it cannot share b or dinv
  if (ranges_overlap(x, b, M))
    throw std::runtime_error("bicgstab: x overlaps b (x is updated in place)");
  if (dinv && ranges_overlap(x, dinv, M))
    throw std::runtime_error("bicgstab: x overlaps dinv (x is updated in place)");

  BicgstabWorkspace own(exec);
  BicgstabWorkspace& w = workspace ? *workspace : own;
  const bool pre = dinv != nullptr;
  const bool x_aligned = is_aligned16(x);
  const bool dinv_aligned = is_aligned16(dinv);
  w.ensure(M, N_padded, kmax, !x_aligned, !dinv_aligned, pre);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  SolveStream guard(exec, w.stream); // every launch below goes to w.stream

  throw_on_error(spmv_hip_bicg_ws_reset(w.ws, rtol, nullptr),
                 "spmv_hip_bicg_ws_reset");

  double* const xi = x_aligned ? x : w.x;
  const double* di = dinv;
  if (pre && !dinv_aligned) { // the streaming kernels load 16 bytes at a time
    exec.copy<double>(w.dinv, dinv, M);
    di = w.dinv;
  }
  // what the two SpMVs read (padded); without a dinv p and s themselves
  double* const PH = pre ? w.ph : w.p;
  double* const SH = pre ? w.sh : w.s;
  // their ghost tails are defined here instead of relying on fresh pages
  if (N_padded > M) {
    exec.memset<double>(PH + M, 0, N_padded - M);
    exec.memset<double>(SH + M, 0, N_padded - M);
  }
  // r = rhat = p = b, ph = dinv*b, x0 = 0, partials of b.b: one pass
  throw_on_error(spmv_hip_bicg_init_f64(ctx, w.ws, M, b, di, w.r, w.rhat, w.p,
                                        pre ? w.ph : nullptr, xi, nullptr),
                 "spmv_hip_bicg_init_f64");
  w.flags[0] = 0;
  w.flags[1] = -1;
  w.flags[2] = 0;

  // the state words alone (h == nullptr), or with the history of pairs
  auto read = ws_reader(w.ws, w.flags, spmv_hip_bicg_ws_read_async,
                        "spmv_hip_bicg_ws_read_async");

  // {rr0, rho0}: one all-reduce of 2 doubles
  throw_on_error(spmv_hip_bicg_reduce_rr_rho(ctx, w.ws, 0, nullptr),
                 "spmv_hip_bicg_reduce_rr_rho");
  comm.reduce_sum(ws_slot(w.ws, spmv_hip_bicg_ws_rr_rho, 0,
                          "spmv_hip_bicg_ws_rr_rho"),
                  2, w.stream);

  const bool consume = opt.consumer_reductions && comm.size() == 1;
  std::vector<void*>& timing_ev = w.timing_ev;
  // y = A q between two events when the SpMVs are timed
  auto mult = [&](double* q, double* y, size_t ev) {
    col_l2g->update(q); // starts on the side stream
    if (opt.time_spmv)
      exec.record_event(timing_ev[ev], w.stream);
    A.mult(q, y);
    if (opt.time_spmv)
      exec.record_event(timing_ev[ev + 1], w.stream);
  };
  LaggingPoll poll(exec, w, opt.poll_every, kmax);
  int k = 0;
  while (k < kmax && !poll.stopped) {
    ++k;
    mult(PH, w.v, 4 * (size_t)(k - 1));
    throw_on_error(spmv_hip_bicg_dot_rv_f64(ctx, w.ws, k, M, w.rhat, w.v,
                                            nullptr),
                   "spmv_hip_bicg_dot_rv_f64");
    if (consume) {
      // one rank: the update kernels add the partials themselves
      throw_on_error(spmv_hip_bicg_update_s_cs_f64(ctx, w.ws, k, M, w.r, w.v,
                                                   di, w.s,
                                                   pre ? w.sh : nullptr,
                                                   nullptr),
                     "spmv_hip_bicg_update_s_cs_f64");
    } else {
      throw_on_error(spmv_hip_bicg_reduce_rv(ctx, w.ws, k, nullptr),
                     "spmv_hip_bicg_reduce_rv");
      comm.reduce_sum(ws_slot(w.ws, spmv_hip_bicg_ws_rv, k,
                              "spmv_hip_bicg_ws_rv"),
                      1, w.stream);
      throw_on_error(spmv_hip_bicg_update_s_f64(ctx, w.ws, k, M, w.r, w.v, di,
                                                w.s, pre ? w.sh : nullptr,
                                                nullptr),
                     "spmv_hip_bicg_update_s_f64");
    }
    mult(SH, w.t, 4 * (size_t)(k - 1) + 2);
    throw_on_error(spmv_hip_bicg_dot_ts_tt_f64(ctx, w.ws, k, M, w.t, w.s,
                                               nullptr),
                   "spmv_hip_bicg_dot_ts_tt_f64");
    if (consume) {
      throw_on_error(spmv_hip_bicg_update_xr_cs_f64(ctx, w.ws, k, M, PH,
                                                    pre ? w.sh : nullptr, w.s,
                                                    w.t, w.rhat, xi, w.r,
                                                    nullptr),
                     "spmv_hip_bicg_update_xr_cs_f64");
      throw_on_error(spmv_hip_bicg_update_p_cs_f64(ctx, w.ws, k, M, w.r, w.v,
                                                   di, w.p,
                                                   pre ? w.ph : nullptr,
                                                   nullptr),
                     "spmv_hip_bicg_update_p_cs_f64");
    } else {
      throw_on_error(spmv_hip_bicg_reduce_ts_tt(ctx, w.ws, k, nullptr),
                     "spmv_hip_bicg_reduce_ts_tt");
      comm.reduce_sum(ws_slot(w.ws, spmv_hip_bicg_ws_ts_tt, k,
                              "spmv_hip_bicg_ws_ts_tt"),
                      2, w.stream); // ts[k] and tt[k] at once
      throw_on_error(spmv_hip_bicg_update_xr_f64(ctx, w.ws, k, M, PH,
                                                 pre ? w.sh : nullptr, w.s, w.t,
                                                 w.rhat, xi, w.r, nullptr),
                     "spmv_hip_bicg_update_xr_f64");
      throw_on_error(spmv_hip_bicg_reduce_rr_rho(ctx, w.ws, k, nullptr),
                     "spmv_hip_bicg_reduce_rr_rho");
      comm.reduce_sum(ws_slot(w.ws, spmv_hip_bicg_ws_rr_rho, k,
                              "spmv_hip_bicg_ws_rr_rho"),
                      2, w.stream); // rr[k] and rho[k] at once
      throw_on_error(spmv_hip_bicg_update_p_f64(ctx, w.ws, k, M, w.r, w.v, di,
                                                w.p, pre ? w.ph : nullptr,
                                                nullptr),
                     "spmv_hip_bicg_update_p_f64");
    }

    poll.step(k, read);
  }

  // final state: {done, kstop, status} and the history of pairs {rr[k], rho[k]}
  const std::vector<double> rrho
      = read_history(spmv_hip_bicg_ws_capacity, w.ws, kmax, 2, read);
  if (xi != x)
    exec.copy<double>(x, xi, M);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    if (opt.time_spmv)
      sum_spmv_times(ctx, timing_ev, 4 * (size_t)k, *stats);
  }

  // The kernel that takes a decision raises `done` itself, so the flag is
  // exact when the loop ends: not raised means k iterations ran to the end.
  int k_final = k, st = 0;
  if (w.flags[0] != 0) {
    k_final = w.flags[1];
    st = w.flags[2];
  } else if (rrho[0] == 0.0) {
    k_final = 0; // (kmax == 0: no kernel ran to say so)
  }
  if (status)
    *status = st;
  write_history(rnorm_history, k_final,
                [&](int j) { return rrho[2 * (size_t)j]; });
  return k_final;
}

} // namespace spmv
