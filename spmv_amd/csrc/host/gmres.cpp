// spmv::gmres for HipExecutor: see cg.h.
#include "cg.h"

#include "solver_common.h"

namespace spmv
{
using namespace detail;

// ---------------------------------------------------------------------------
// gmres: see cg.h.  The basis is ONE allocation of restart + 1 vectors at the
// stride N_padded (rounded up to even): every v_j carries its own ghost tail,
// so without a preconditioner Matrix::mult reads v_j where it lies -- no copy
// pass; with one, M^-1 v_j lands in the padded work vector z.  w IS the slot
// of v_{j+1}: the SpMV writes it, the two Gram-Schmidt passes update it in
// place and the scale kernel normalises it in place.
//
// Inner step at basis size j + 1 (compute stream), Z = z or v_j:
//     [z = M^-1 v_j] ; halo start of Z ; w = A Z
//     multi_dot ; reduce(H) ; all-reduce of j + 1
//     multi_axpy (first)
//     multi_dot ; reduce(C) ; all-reduce of j + 1
//     multi_axpy (second: h += c ; partials of w.w)
//     one rank: givens adds the partials itself; otherwise reduce(WW) ;
//               all-reduce of 1 ; givens
//     scale (not after the last step of a cycle: v_restart is never read)
// 1 SpMV + 8 launches on one rank (+ 1 reducer with several); beside the SpMV
// and M^-1, 4 (j + 1) + 2 ceil((j + 1) / 8) + 4 + 2 vector passes: each
// multi_dot reads j + 1 vectors and w once per group of 8, each multi_axpy
// reads j + 1 and reads and writes w, the scale reads and writes w.  Single
// dots and axpys would stream 2 (j + 1) + 3 (j + 1) per Gram-Schmidt pass.
// Cycle end: solve_y ; combine (jn reads, 1 write) ; [z = M^-1 u] ; add (3).
// Cycle start: [halo of x ; A x] ; residual (3 passes, first cycle 2) ;
// [reduce(WW) ; all-reduce] ; start ; scale (2).
// ---------------------------------------------------------------------------
GmresWorkspace::GmresWorkspace(HipExecutor& exec)
    : SolverWorkspace(exec), cheb(exec)
{
}

GmresWorkspace::~GmresWorkspace() { release(); }

void GmresWorkspace::release()
{
  release_common();
  drop_scalars(ws, kmax_cap, spmv_hip_gmres_ws_destroy);
  free_vectors({&r, &ax, &u, &z, &x, &V, &b, &dinv});
  m_cap = n_cap = v_cap = b_cap = dinv_cap = -1;
}

void GmresWorkspace::ensure(int64_t M, int64_t N_padded, int64_t basis_elems,
                            int kmax, bool need_b, bool need_dinv)
{
  open(4);
  regrow_scalars(
      ws, kmax_cap, kmax, kmax > kmax_cap, spmv_hip_gmres_ws_destroy,
      [&](auto out) {
        return spmv_hip_gmres_ws_create(_exec.context(), kmax, out);
      },
      "spmv_hip_gmres_ws_create");
  regrow(m_cap, M, {&r, &ax, &u});
  regrow(n_cap, N_padded, {&z, &x});
  regrow(v_cap, basis_elems, {&V});
  if (need_b)
    regrow(b_cap, M, {&b});
  if (need_dinv)
    regrow(dinv_cap, M, {&dinv});
}

void gmres_check_arguments(const GmresPreconditioner* M, int restart, int kmax,
                           int64_t rows)
{
  const GmresPreconditioner none;
  const GmresPreconditioner& p = M ? *M : none;
  if (p.amg && p.sgs)
    throw std::runtime_error(
        "spmv::gmres - Error: one preconditioner at a time (amg excludes sgs, "
        "dinv and the Chebyshev degree)");
  // (amg obeys the rules of sgs)
  gmres_check_rules(restart, kmax, p.dinv != nullptr, p.cheb_degree, p.lmin,
                    p.lmax, p.sgs || p.amg,
                    p.amg ? p.amg->rows() : p.sgs ? p.sgs->rows() : 0, rows);
}

int gmres(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
          const double* b, double* x, const GmresPreconditioner* precond,
          int restart, int kmax, double rtol,
          std::vector<double>* rnorm_history, const CgOptions* options,
          CgStats* stats, GmresWorkspace* workspace, int* status)
{
  // plain argument rules first: nothing below has touched a device yet
  gmres_check_arguments(precond, restart, kmax, A.row_map()->local_size());
  const Dims dims = check_problem("gmres", A, kmax);
  const int64_t M = dims.M, N_padded = dims.N_padded;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  const CgOptions opt = options ? *options : CgOptions();
  const GmresPreconditioner pre = precond ? *precond : GmresPreconditioner();
  const double* dinv = pre.dinv;
  if (ranges_overlap(x, b, M))
    throw std::runtime_error("gmres: x overlaps b");
  if (dinv && ranges_overlap(x, dinv, M))
    throw std::runtime_error("gmres: x overlaps dinv");
  spmv_hip_ctx* ctx = exec.context();

  GmresWorkspace own(exec);
  GmresWorkspace& w = workspace ? *workspace : own;
  const bool cheb = pre.cheb_degree >= 1;
  const bool diag = dinv && !cheb;
  const bool any_pre = cheb || diag || pre.sgs || pre.amg;
  const bool b_aligned = is_aligned16(b);
  const bool dinv_aligned = is_aligned16(dinv);
  const int64_t stride = gmres_basis_stride(N_padded);
  w.ensure(M, N_padded, gmres_basis_elems(N_padded, restart), kmax, !b_aligned,
           dinv && !dinv_aligned);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  SolveStream guard(exec, w.stream); // every launch below goes to w.stream

  throw_on_error(spmv_hip_gmres_ws_reset(w.ws, rtol, kmax, restart, nullptr),
                 "spmv_hip_gmres_ws_reset");
  const double* bi = b;
  if (!b_aligned) { // the streaming kernels load 16 bytes at a time
    exec.copy<double>(w.b, b, M);
    bi = w.b;
  }
  const double* di = dinv;
  if (dinv && !dinv_aligned) {
    exec.copy<double>(w.dinv, dinv, M);
    di = w.dinv;
  }
  // The iterate lives in the padded w.x (r = b - A x reads it through
  // Matrix::mult); the caller's x takes one copy at the end.  Ghost tails are
  // defined here instead of relying on fresh pages.
  exec.memset<double>(w.x, 0, N_padded);
  // u is what the preconditioner reads at a cycle end; combine leaves it alone
  // when no column was kept, so it is defined from the start
  exec.memset<double>(w.u, 0, M);
  if (N_padded > M) {
    exec.memset<double>(w.z + M, 0, N_padded - M);
    for (int j = 0; j <= restart; ++j)
      exec.memset<double>(w.V + j * stride + M, 0, N_padded - M);
  }
  w.flags[0] = 0;
  w.flags[1] = -1;
  w.flags[2] = 0;
  w.flags[3] = 0;

  auto read = ws_reader(w.ws, w.flags, spmv_hip_gmres_ws_read_async,
                        "spmv_hip_gmres_ws_read_async");
  auto slot = [&](int which) {
    return ws_array(w.ws, spmv_hip_gmres_ws_array, which,
                    "spmv_hip_gmres_ws_array");
  };
  const bool several = comm.size() > 1;
  double* const slot_h = slot(SPMV_HIP_GMRES_H);
  double* const slot_c = slot(SPMV_HIP_GMRES_C);
  double* const slot_ww = slot(SPMV_HIP_GMRES_WW);

  // dst (padded) = M^-1 src; returns what holds the result (src itself
  // without a preconditioner)
  auto apply_pre = [&](double* src) -> double* {
    if (!any_pre)
      return src;
    if (!apply_stored_preconditioner(exec, A, pre, di, &w.cheb, src, w.z))
      throw_on_error(spmv_hip_gmres_diag_f64(ctx, M, di, src, w.z, nullptr),
                     "spmv_hip_gmres_diag_f64");
    return w.z;
  };
  // PART_WW -> the value start / givens take: with several ranks through the
  // reducer's slot and one all-reduce
  auto finish_ww = [&]() {
    if (!several)
      return;
    throw_on_error(spmv_hip_gmres_reduce(ctx, w.ws, SPMV_HIP_GMRES_WW, 1,
                                         nullptr),
                   "spmv_hip_gmres_reduce");
    comm.reduce_sum(slot_ww, 1, w.stream);
  };
  auto begin_cycle = [&](bool first) {
    if (!first) {
      col_l2g->update(w.x);
      A.mult(w.x, w.ax);
    }
    throw_on_error(spmv_hip_gmres_residual_f64(ctx, w.ws, M, bi,
                                               first ? nullptr : w.ax, w.r,
                                               nullptr),
                   "spmv_hip_gmres_residual_f64");
    finish_ww();
    throw_on_error(spmv_hip_gmres_start(ctx, w.ws, first, several, nullptr),
                   "spmv_hip_gmres_start");
  };
  // one Gram-Schmidt pass of w against v_0 .. v_j
  auto orthogonalise = [&](int j, double* wv, bool second) {
    throw_on_error(spmv_hip_gmres_multi_dot_f64(ctx, w.ws, M, w.V, stride,
                                                j + 1, wv, nullptr),
                   "spmv_hip_gmres_multi_dot_f64");
    throw_on_error(spmv_hip_gmres_reduce(ctx, w.ws,
                                         second ? SPMV_HIP_GMRES_C
                                                : SPMV_HIP_GMRES_H,
                                         j + 1, nullptr),
                   "spmv_hip_gmres_reduce");
    if (several)
      comm.reduce_sum(second ? slot_c : slot_h, j + 1, w.stream);
    throw_on_error(spmv_hip_gmres_multi_axpy_f64(ctx, w.ws, second, M, w.V,
                                                 stride, j + 1, wv, nullptr),
                   "spmv_hip_gmres_multi_axpy_f64");
  };
  auto end_cycle = [&]() {
    throw_on_error(spmv_hip_gmres_solve_y(ctx, w.ws, nullptr),
                   "spmv_hip_gmres_solve_y");
    throw_on_error(spmv_hip_gmres_combine_f64(ctx, w.ws, M, w.V, stride, w.u,
                                              nullptr),
                   "spmv_hip_gmres_combine_f64");
    const double* zu = apply_pre(w.u);
    throw_on_error(spmv_hip_gmres_add_f64(ctx, w.ws, M, zu, w.x, nullptr),
                   "spmv_hip_gmres_add_f64");
  };

  std::vector<void*>& timing_ev = w.timing_ev;
  LaggingPoll poll(exec, w, opt.poll_every, kmax);
  begin_cycle(true); // hist[0], also for kmax == 0
  int steps = 0;     // inner steps enqueued
  bool first = true;
  while (steps < kmax && !poll.stopped) {
    if (!first)
      begin_cycle(false);
    first = false;
    throw_on_error(spmv_hip_gmres_scale_f64(ctx, w.ws, M, w.r, w.V, nullptr),
                   "spmv_hip_gmres_scale_f64");
    for (int j = 0; j < restart && steps < kmax && !poll.stopped; ++j) {
      ++steps;
      double* const vj = w.V + j * stride;
      double* const wv = vj + stride; // the slot of v_{j+1}
      double* const Z = apply_pre(vj);
      col_l2g->update(Z); // starts on the side stream
      if (opt.time_spmv)
        exec.record_event(timing_ev[2 * (size_t)(steps - 1)], w.stream);
      A.mult(Z, wv);
      if (opt.time_spmv)
        exec.record_event(timing_ev[2 * (size_t)(steps - 1) + 1], w.stream);
      orthogonalise(j, wv, false);
      orthogonalise(j, wv, true);
      finish_ww();
      throw_on_error(spmv_hip_gmres_givens(ctx, w.ws, j, several, nullptr),
                     "spmv_hip_gmres_givens");
      if (j + 1 < restart)
        throw_on_error(spmv_hip_gmres_scale_f64(ctx, w.ws, M, wv, wv, nullptr),
                       "spmv_hip_gmres_scale_f64");
      poll.step(steps, read);
    }
    end_cycle(); // once per cycle, whether it ran to its end or the poll ended it
  }

  // final state: {done, kstop, status, k} and the history
  const std::vector<double> hist
      = read_history(spmv_hip_gmres_ws_capacity, w.ws, kmax, 1, read);
  exec.copy<double>(x, w.x, M);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    if (opt.time_spmv)
      sum_spmv_times(ctx, timing_ev, 2 * (size_t)steps, *stats);
  }

  // every way out of the inner loop raises `done` on the device; it is not
  // raised only when no step ran (kmax == 0)
  const int k_final = w.flags[0] != 0 ? w.flags[1] : w.flags[3];
  if (status)
    *status = w.flags[2];
  if (rnorm_history)
    rnorm_history->assign(hist.begin(), hist.begin() + k_final + 1);
  return k_final;
}

} // namespace spmv
