// spmv::lobpcg for HipExecutor: see cg.h.
#include "cg.h"

#include "solver_common.h"

namespace spmv
{
using namespace detail;

// ---------------------------------------------------------------------------
// lobpcg: see cg.h.  On the compute stream, k = nev, "Gram" = the Gram kernel, its
// reducer and, with several ranks, the all-reduce of 2 m m doubles:
//     prologue: rules, workspace, aligned copy of X, ghost tail of W, P = AP = 0
//       Gram(X, X) ; rr(orth) ; update(X alone)         X = X R^-1
//       W = X ; halo ; AX = A W
//       Gram(X, AX) ; rr ; update(X, AX)                 the first Ritz pairs
//       residual (+ W) ; norms                           it = 0
//     it = 1..kmax, until the lagging poll sees `done`:
//       [W = M^-1 R] ; halo of W ; AW = A W
//       Gram(six blocks) ; rr ; update ; residual (+ W) ; norms
//     epilogue: W = X ; halo ; AW = A W ; residual(final) ; norms(final) ; the
//       history, copy back of an unaligned X, sync, times
// With B (the pencil): Gram is gram_gen over [S | AS | BS], update is
// update_gen over the three triples, BX stands in X's place in the residual:
//     prologue: ... BP = 0
//       W = X ; halo ; BX = B W
//       Gram(X, BX) ; rr(orth) ; update(X, BX)           X = X R^-1, BX likewise
//       W = X ; halo ; AX = A W
//       Gram(X, AX, BX) ; rr ; update(X, AX, BX)
//       residual (+ W) ; norms
//     it: ... halo of W ; AW = A W ; BW = B W ; Gram(nine blocks) ; rr ; update ;
//       residual (+ W) ; norms
//     epilogue: W = X ; halo ; AW = A W ; BW = B W ; residual(final) ; ...
// ---------------------------------------------------------------------------
LobpcgWorkspace::~LobpcgWorkspace() { release(); }

void LobpcgWorkspace::release()
{
  release_common();
  drop_scalars(ws, kmax_cap, spmv_hip_lobpcg_ws_destroy);
  free_vectors({&r, &p, &ax, &aw, &ap, &x, &w, &bx, &bw, &bp});
  nev_cap = 0;
  m_cap = n_cap = x_cap = b_cap = -1;
}

void LobpcgWorkspace::ensure(int64_t m_elems, int64_t n_elems, int kmax, int nev,
                             bool need_x, bool with_b)
{
  open(SPMV_HIP_LOBPCG_STATE_WORDS);
  regrow_scalars(
      ws, kmax_cap, kmax, kmax > kmax_cap || nev != nev_cap,
      spmv_hip_lobpcg_ws_destroy,
      [&](auto out) {
        nev_cap = 0; // while they are gone
        return spmv_hip_lobpcg_ws_create(_exec.context(), kmax, nev, out);
      },
      "spmv_hip_lobpcg_ws_create");
  nev_cap = nev;
  regrow(m_cap, m_elems, {&r, &p, &ax, &aw, &ap});
  if (need_x)
    regrow(x_cap, m_elems, {&x});
  regrow(n_cap, n_elems, {&w});
  if (with_b)
    regrow(b_cap, m_elems, {&bx, &bw, &bp});
}

int lobpcg(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
           double* X, int nev, const BlockPreconditioner& M, int kmax,
           double rtol, double atol, std::vector<double>* eigenvalues,
           std::vector<double>* resnorm_history, int* status,
           const LobpcgOptions* options, LobpcgStats* stats,
           LobpcgWorkspace* workspace, const Matrix<double>* B)
{
  // plain argument rules first: nothing below has touched a device yet
  const int64_t rows = A.row_map()->local_size();
  lobpcg_check_rules(nev, kmax, rtol, atol, M.dinv != nullptr, M.sgs != nullptr,
                     M.amg != nullptr, M.sgs ? M.sgs->rows() : 0,
                     M.sgs ? M.sgs->negative_pivots() : 0,
                     M.amg ? M.amg->rows(0) : 0, rows);
  const bool gen = B != nullptr;
  if (gen) {
    const std::vector<std::int64_t>& ga = A.col_map()->ghosts();
    const std::vector<std::int64_t>& gb = B->col_map()->ghosts();
    lobpcg_check_pencil(rows, B->row_map()->local_size(), ga.data(),
                        (int64_t)ga.size(), gb.data(), (int64_t)gb.size());
  }
  const Dims dims = check_problem("lobpcg", A, kmax);
  if (gen)
    check_problem("lobpcg", *B, kmax); // (no ghost rows in B either)
  const int64_t M_rows = dims.M;
  const int64_t m_elems = M_rows * nev, n_elems = dims.N_padded * nev;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  const LobpcgOptions opt = options ? *options : LobpcgOptions();
  spmv_hip_ctx* ctx = exec.context();
  const bool several = comm.size() > 1;
  const bool applied = M.sgs || M.amg; // M^-1 is a call of its own

  LobpcgWorkspace own(exec);
  LobpcgWorkspace& w = workspace ? *workspace : own;
  const bool x_aligned = is_aligned16(X);
  w.ensure(m_elems, n_elems, kmax, nev, !x_aligned, gen);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  SolveStream guard(exec, w.stream); // every launch below goes to w.stream

  throw_on_error(spmv_hip_lobpcg_ws_reset(w.ws, rtol, atol, kmax, opt.largest,
                                          nullptr),
                 "spmv_hip_lobpcg_ws_reset");
  double* const slot_gram
      = ws_array(w.ws, spmv_hip_lobpcg_ws_array, SPMV_HIP_LOBPCG_GRAM,
                 "spmv_hip_lobpcg_ws_array");
  double* const slot_rn
      = ws_array(w.ws, spmv_hip_lobpcg_ws_array, SPMV_HIP_LOBPCG_RN,
                 "spmv_hip_lobpcg_ws_array");

  double* const Xi = x_aligned ? X : w.x;
  if (!x_aligned)
    exec.copy<double>(w.x, X, m_elems);
  // the ghost tail of W is defined here instead of relying on fresh pages; P
  // and AP are summed by the first Gram pass before anything wrote them
  if (n_elems > m_elems)
    exec.memset<double>(w.w + m_elems, 0, n_elems - m_elems);
  exec.memset<double>(w.p, 0, m_elems);
  exec.memset<double>(w.ap, 0, m_elems);
  if (gen)
    exec.memset<double>(w.bp, 0, m_elems);
  for (int i = 0; i < SPMV_HIP_LOBPCG_STATE_WORDS; ++i)
    w.flags[i] = 0;

  // Gram sums of `blocks` blocks, then the one-workgroup step on them
  auto gram_rr = [&](int blocks, const double* ax, int mode, int advance) {
    if (gen)
      throw_on_error(spmv_hip_lobpcg_gram_gen_f64(ctx, w.ws, M_rows, blocks, Xi,
                                                  w.w, w.p, ax, w.aw, w.ap, w.bx,
                                                  w.bw, w.bp, nullptr),
                     "spmv_hip_lobpcg_gram_gen_f64");
    else
      throw_on_error(spmv_hip_lobpcg_gram_f64(ctx, w.ws, M_rows, blocks, Xi, w.w,
                                              w.p, ax, w.aw, w.ap, nullptr),
                     "spmv_hip_lobpcg_gram_f64");
    // (one thread per entry: the rr kernel's one wave would walk the partials
    // of 18 entries per lane one after the other)
    throw_on_error(spmv_hip_lobpcg_gram_reduce(ctx, w.ws, M_rows, blocks,
                                               nullptr),
                   "spmv_hip_lobpcg_gram_reduce");
    if (several) {
      const size_t m = (size_t)blocks * nev;
      comm.reduce_sum(slot_gram, 2 * m * m, w.stream);
    }
    throw_on_error(spmv_hip_lobpcg_rr(ctx, w.ws, M_rows, blocks, mode, 1,
                                      advance, nullptr),
                   "spmv_hip_lobpcg_rr");
  };
  // R = AX - X diag(theta) (+ W where that is no call of its own), the norms;
  // bx (the pencil): R = AX - BX diag(theta)
  auto residual_norms = [&](const double* ax, const double* bx, int final) {
    throw_on_error(spmv_hip_lobpcg_residual_f64(
                       ctx, w.ws, M_rows, bx ? bx : Xi, ax, M.dinv, w.r,
                       final || applied ? nullptr : w.w, final, nullptr),
                   "spmv_hip_lobpcg_residual_f64");
    if (several) {
      throw_on_error(spmv_hip_lobpcg_norms(ctx, w.ws, 1, final, nullptr),
                     "spmv_hip_lobpcg_norms");
      comm.reduce_sum(slot_rn + (final ? nev : 0), nev, w.stream);
      if (!final)
        throw_on_error(spmv_hip_lobpcg_norms(ctx, w.ws, 2, 0, nullptr),
                       "spmv_hip_lobpcg_norms");
    } else {
      throw_on_error(spmv_hip_lobpcg_norms(ctx, w.ws, 0, final, nullptr),
                     "spmv_hip_lobpcg_norms");
    }
  };
  // out = A X through the padded block W (not guarded by the state: what it
  // leaves after `done` is not used)
  // out_b (the pencil): B X as well, from the same exchange.  The exchange
  // runs on A's column map; with an overlapping model only A's product waits
  // for it (B's own map has nothing in flight), so B's product alone is put
  // behind it here
  auto mult_x = [&](double* out_a, double* out_b) {
    exec.copy<double>(w.w, Xi, m_elems);
    col_l2g->update_block(w.w, nev);
    if (out_a)
      A.mult_block(w.w, out_a, nev, nullptr);
    else
      col_l2g->update_finalise_block(w.w, nev);
    if (out_b)
      B->mult_block(w.w, out_b, nev, nullptr);
  };
  // the one-block update of the prologue; ax: AX as well
  auto update_x = [&](double* ax) {
    if (gen)
      throw_on_error(spmv_hip_lobpcg_update_gen_f64(
                         ctx, w.ws, M_rows, 1, Xi, nullptr, nullptr, ax, nullptr,
                         nullptr, w.bx, nullptr, nullptr, nullptr),
                     "spmv_hip_lobpcg_update_gen_f64");
    else
      throw_on_error(spmv_hip_lobpcg_update_f64(ctx, w.ws, M_rows, 1, Xi,
                                                nullptr, nullptr, ax, nullptr,
                                                nullptr, nullptr),
                     "spmv_hip_lobpcg_update_f64");
  };

  if (gen)
    mult_x(nullptr, w.bx);
  gram_rr(1, gen ? w.bx : Xi, 1, 0); // (mode 1 reads Gb alone)
  update_x(nullptr);
  mult_x(w.ax, nullptr);
  gram_rr(1, w.ax, 0, 0);
  update_x(w.ax);
  residual_norms(w.ax, gen ? w.bx : nullptr, 0);

  auto read = [&](double* h, size_t n) {
    throw_on_error(spmv_hip_lobpcg_ws_read_async(w.ws, w.flags, h, n, nullptr,
                                                 nullptr),
                   "spmv_hip_lobpcg_ws_read_async");
  };

  std::vector<void*>& timing_ev = w.timing_ev;
  LaggingPoll poll(exec, w, opt.poll_every, kmax);
  int k = 0;
  while (k < kmax && !poll.stopped) {
    ++k;
    if (M.sgs)
      sgs_apply_block(exec, *M.sgs, w.r, w.w, nev);
    else if (M.amg) // (on the object's own scratch)
      amg_apply_block(exec, *M.amg, w.r, w.w, nev);
    col_l2g->update_block(w.w, nev); // starts on the side stream
    void* ev1 = nullptr;
    if (opt.time_spmv) {
      ev1 = timing_ev[2 * (size_t)(k - 1) + 1];
      exec.record_event(timing_ev[2 * (size_t)(k - 1)], w.stream);
    }
    A.mult_block(w.w, w.aw, nev, ev1);
    if (gen) // (behind A's product, which waited for the halo of W)
      B->mult_block(w.w, w.bw, nev, nullptr);
    gram_rr(3, w.ax, 0, 1);
    if (gen)
      throw_on_error(spmv_hip_lobpcg_update_gen_f64(
                         ctx, w.ws, M_rows, 3, Xi, w.w, w.p, w.ax, w.aw, w.ap,
                         w.bx, w.bw, w.bp, nullptr),
                     "spmv_hip_lobpcg_update_gen_f64");
    else
      throw_on_error(spmv_hip_lobpcg_update_f64(ctx, w.ws, M_rows, 3, Xi, w.w,
                                                w.p, w.ax, w.aw, w.ap, nullptr),
                     "spmv_hip_lobpcg_update_f64");
    residual_norms(w.ax, gen ? w.bx : nullptr, 0);
    poll.step(k, read);
  }

  // the true residuals: AX (and BX) from X itself
  mult_x(w.aw, gen ? w.bw : nullptr);
  residual_norms(w.aw, gen ? w.bw : nullptr, 1);

  int cap = 0, cap_nev = 0;
  throw_on_error(spmv_hip_lobpcg_ws_capacity(w.ws, &cap, &cap_nev),
                 "spmv_hip_lobpcg_ws_capacity");
  std::vector<double> hist(((size_t)std::max(kmax, cap) + 1) * nev, -1.0);
  std::vector<double> scal(3 * (size_t)nev, 0.0);
  throw_on_error(spmv_hip_lobpcg_ws_read_async(w.ws, w.flags, hist.data(),
                                               hist.size(), scal.data(), nullptr),
                 "spmv_hip_lobpcg_ws_read_async");
  if (Xi != X)
    exec.copy<double>(X, Xi, m_elems);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = LobpcgStats();
    if (opt.time_spmv)
      sum_spmv_times(ctx, timing_ev, 2 * (size_t)k, *stats);
    stats->true_resnorm.resize(nev);
    for (int c = 0; c < nev; ++c)
      stats->true_resnorm[c] = std::sqrt(scal[2 * (size_t)nev + c]);
    stats->restarts = w.flags[6];
  }

  // every way out of the loop raises `done` on the device (norms does at
  // it == kmax)
  const int k_final = w.flags[0] != 0 ? w.flags[1] : 0;
  if (status)
    *status = w.flags[2];
  if (eigenvalues)
    eigenvalues->assign(scal.begin(), scal.begin() + nev);
  if (resnorm_history) {
    resnorm_history->assign((size_t)nev * ((size_t)kmax + 1), -1.0);
    for (int c = 0; c < nev; ++c)
      for (int j = 0; j <= k_final; ++j)
        (*resnorm_history)[(size_t)c * ((size_t)kmax + 1) + j]
            = hist[(size_t)j * nev + c];
  }
  return k_final;
}

} // namespace spmv
