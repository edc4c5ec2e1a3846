// spmv::lsqr for HipExecutor: see cg.h.
#include "cg.h"

#include "solver_common.h"

namespace spmv
{
using namespace detail;

// ---------------------------------------------------------------------------
// lsqr: see cg.h.  On the compute stream, m rows and n owned columns:
//     prologue: rules, workspace, aligned copy of x, ghost tail of vt, ws_reset
//     ut = b ; x = 0 ; partials of ut.ut ; [reduce(UU) ; all-reduce of 1]
//     Atu = A^T ut ; reverse halo ; update_v(first) ; [reduce(VV) ; all-reduce]
//     start ; update_xw(0): w = vt * ia
//     k = 1..kmax, until the lagging poll sees `done`:
//       halo start of vt ; Av = A vt ; update_u ; [reduce(UU) ; all-reduce]
//       Atu = A^T ut ; reverse halo ; update_v ; [reduce(VV) ; all-reduce]
//       step ; update_xw(k)
//     epilogue: histories, copy back of an unaligned x, sync, times
// ---------------------------------------------------------------------------
LsqrWorkspace::~LsqrWorkspace() { release(); }

void LsqrWorkspace::release()
{
  release_common();
  drop_scalars(ws, kmax_cap, spmv_hip_lsqr_ws_destroy);
  free_vectors({&ut, &Av, &vt, &Atu, &w, &x});
  m_cap = n_cap = w_cap = x_cap = -1;
}

void LsqrWorkspace::ensure(int64_t M, int64_t N, int64_t N_padded, int kmax,
                           bool need_x)
{
  open(4);
  regrow_scalars(
      ws, kmax_cap, kmax, kmax > kmax_cap, spmv_hip_lsqr_ws_destroy,
      [&](auto out) {
        return spmv_hip_lsqr_ws_create(_exec.context(), kmax, out);
      },
      "spmv_hip_lsqr_ws_create");
  regrow(m_cap, M, {&ut, &Av});
  regrow(n_cap, N_padded, {&vt, &Atu});
  regrow(w_cap, N, {&w});
  if (need_x)
    regrow(x_cap, N, {&x});
}

int lsqr(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
         const double* b, double* x, int kmax, double rtol, double ltol,
         double damp, std::vector<double>* hist_r, std::vector<double>* hist_ar,
         int* status, const CgOptions* options, CgStats* stats,
         LsqrWorkspace* workspace)
{
  // plain argument rules first: nothing below has touched a device yet
  lsqr_check_rules(kmax, ltol, damp, A.row_map()->local_size(),
                   A.col_map()->local_size(), b, x);
  const Dims dims = check_problem("lsqr", A, kmax);
  const int64_t M = dims.M, N_padded = dims.N_padded;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  const int64_t N = col_l2g->local_size();
  const CgOptions opt = options ? *options : CgOptions();
  spmv_hip_ctx* ctx = exec.context();

  LsqrWorkspace own(exec);
  LsqrWorkspace& w = workspace ? *workspace : own;
  const bool x_aligned = is_aligned16(x);
  w.ensure(M, N, N_padded, kmax, !x_aligned);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  SolveStream guard(exec, w.stream); // every launch below goes to w.stream

  throw_on_error(spmv_hip_lsqr_ws_reset(w.ws, rtol, ltol, damp, kmax, nullptr),
                 "spmv_hip_lsqr_ws_reset");
  auto slot = [&](int which) {
    return ws_array(w.ws, spmv_hip_lsqr_ws_array, which,
                    "spmv_hip_lsqr_ws_array");
  };
  double* const slot_uu = slot(SPMV_HIP_LSQR_UU);
  double* const slot_vv = slot(SPMV_HIP_LSQR_VV);
  double* const part_uu = slot(SPMV_HIP_LSQR_PART_UU);
  const bool several = comm.size() > 1;

  double* const xi = x_aligned ? x : w.x;
  exec.copy<double>(w.ut, b, M);
  exec.memset<double>(xi, 0, N);
  // the ghost tail is defined here instead of relying on fresh pages
  if (N_padded > N)
    exec.memset<double>(w.vt + N, 0, N_padded - N);
  w.flags[0] = 0;
  w.flags[1] = -1;
  w.flags[2] = 0;

  auto read = ws_reader(w.ws, w.flags, spmv_hip_lsqr_ws_read_async,
                        "spmv_hip_lsqr_ws_read_async");
  // a partial array -> its slot, summed over the ranks
  auto finish = [&](int which, double* at) {
    if (!several)
      return; // the consumer adds the partials itself
    throw_on_error(spmv_hip_lsqr_reduce(ctx, w.ws, which, nullptr),
                   "spmv_hip_lsqr_reduce");
    comm.reduce_sum(at, 1, w.stream);
  };
  std::vector<void*>& timing_ev = w.timing_ev;
  // Atu = A^T ut over the owned columns, between two events when timed
  auto transposed = [&](bool timed, size_t ev) {
    if (timed)
      exec.record_event(timing_ev[ev], w.stream);
    A.transpmult(w.ut, w.Atu);
    if (timed)
      exec.record_event(timing_ev[ev + 1], w.stream);
    if (several)
      col_l2g->reverse_update(w.Atu);
  };

  throw_on_error(spmv_hip_dot_partial_f64(ctx, M, w.ut, w.ut, part_uu, nullptr),
                 "spmv_hip_dot_partial_f64");
  finish(SPMV_HIP_LSQR_UU, slot_uu);
  transposed(false, 0);
  throw_on_error(spmv_hip_lsqr_update_v_f64(ctx, w.ws, N, w.Atu, w.vt, 1,
                                            several, nullptr),
                 "spmv_hip_lsqr_update_v_f64");
  finish(SPMV_HIP_LSQR_VV, slot_vv);
  throw_on_error(spmv_hip_lsqr_start(ctx, w.ws, several, nullptr),
                 "spmv_hip_lsqr_start");
  throw_on_error(spmv_hip_lsqr_update_xw_f64(ctx, w.ws, 0, N, w.vt, w.w, xi,
                                             nullptr),
                 "spmv_hip_lsqr_update_xw_f64");

  LaggingPoll poll(exec, w, opt.poll_every, kmax);
  int k = 0;
  while (k < kmax && !poll.stopped) {
    ++k;
    const size_t ev = 4 * (size_t)(k - 1);
    col_l2g->update(w.vt); // starts on the side stream
    if (opt.time_spmv)
      exec.record_event(timing_ev[ev], w.stream);
    A.mult(w.vt, w.Av);
    if (opt.time_spmv)
      exec.record_event(timing_ev[ev + 1], w.stream);
    throw_on_error(spmv_hip_lsqr_update_u_f64(ctx, w.ws, M, w.Av, w.ut, nullptr),
                   "spmv_hip_lsqr_update_u_f64");
    finish(SPMV_HIP_LSQR_UU, slot_uu);
    transposed(opt.time_spmv, ev + 2);
    throw_on_error(spmv_hip_lsqr_update_v_f64(ctx, w.ws, N, w.Atu, w.vt, 0,
                                              several, nullptr),
                   "spmv_hip_lsqr_update_v_f64");
    finish(SPMV_HIP_LSQR_VV, slot_vv);
    throw_on_error(spmv_hip_lsqr_step(ctx, w.ws, several, nullptr),
                   "spmv_hip_lsqr_step");
    throw_on_error(spmv_hip_lsqr_update_xw_f64(ctx, w.ws, k, N, w.vt, w.w, xi,
                                               nullptr),
                   "spmv_hip_lsqr_update_xw_f64");
    poll.step(k, read);
  }

  // final state: {done, kstop, status} and both histories, hist_ar behind the
  // WORKSPACE's capacity of hist_r: half of what read_history sized
  const std::vector<double> hist
      = read_history(spmv_hip_lsqr_ws_capacity, w.ws, kmax, 2, read);
  const size_t half = hist.size() / 2;
  if (xi != x)
    exec.copy<double>(x, xi, N);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    if (opt.time_spmv)
      sum_spmv_times(ctx, timing_ev, 4 * (size_t)k, *stats);
  }

  // every way out of the loop raises `done` on the device; it is not raised
  // only when no step ran (kmax == 0) and neither b nor A^T b is zero
  const int k_final = w.flags[0] != 0 ? w.flags[1] : 0;
  if (status)
    *status = w.flags[2];
  if (hist_r)
    hist_r->assign(hist.begin(), hist.begin() + k_final + 1);
  if (hist_ar)
    hist_ar->assign(hist.begin() + half, hist.begin() + half + k_final + 1);
  return k_final;
}

} // namespace spmv
