// spmv::cg for HipExecutor: see cg.h.  Algebra and update order follow
// spmv/cg.cpp:21-98; the launch structure is MI355X-specific:
//
//   per iteration (compute stream)            reference line
//     halo start on the map's side stream      cg.cpp:59
//     SpMV local block  (+ fused p.Ap share)   cg.cpp:60,63
//     [wait halo event] SpMV remote block      Matrix.cpp:498-511
//     reduce partials -> pAp[k]; all-reduce    cg.cpp:64-65
//     r -= a Ap; partials of r.r               cg.cpp:66,70,73
//     reduce partials -> rr[k];  all-reduce    cg.cpp:74-76
//     x += a p; stop test; p = beta p + r      cg.cpp:69,77-85
//
// The partial sums of a dot product are added in a fixed order either by the
// consuming update kernel itself (one rank) or by a single-workgroup reducer
// kernel.  3 (or 5) kernel launches per iteration (+ the small remote-block
// kernel and two one-double RCCL all-reduces with more than one rank); the
// reference's CUDA path needs 7 cuBLAS calls, 5 scalar kernels and 3 host
// synchronisations for the same step (cuda/cg.cuda.cu:101-151).
#include "cg.h"

#include "solver_common.h"

namespace spmv
{
using namespace detail;

// ---------------------------------------------------------------------------
void SolverWorkspace::open(int flag_words)
{
  if (stream)
    return;
  stream = _exec.create_stream();
  poll_event = _exec.create_event();
  void* mem = nullptr;
  throw_on_error(spmv_hip_host_alloc(_exec.context(),
                                     flag_words * sizeof(int32_t), &mem),
                 "spmv_hip_host_alloc");
  flags = static_cast<int32_t*>(mem);
}

void SolverWorkspace::regrow(int64_t& cap, int64_t want,
                             std::initializer_list<double**> vecs)
{
  if (want <= cap)
    return;
  for (double** q : vecs) {
    _exec.free(*q);
    *q = nullptr;
  }
  cap = -1;
  for (double** q : vecs)
    *q = _exec.alloc<double>(want);
  cap = want;
}

void SolverWorkspace::reserve_events(size_t n)
{
  while (timing_ev.size() < n)
    timing_ev.push_back(_exec.create_event(true));
}

void SolverWorkspace::release_common()
{
  try {
    if (stream)
      _exec.synchronize_stream(stream);
    _exec.destroy_event(poll_event);
    for (void* e : timing_ev)
      _exec.destroy_event(e);
    if (stream)
      _exec.destroy_stream(stream);
    spmv_hip_host_free(_exec.context(), flags);
  } catch (...) {
  }
  timing_ev.clear();
  flags = nullptr;
  stream = poll_event = nullptr;
}

void SolverWorkspace::free_vectors(std::initializer_list<double**> vecs)
{
  try {
    for (double** q : vecs)
      _exec.free(*q);
  } catch (...) {
  }
  for (double** q : vecs)
    *q = nullptr;
}
// ---------------------------------------------------------------------------
CgWorkspace::~CgWorkspace() { release(); }

void CgWorkspace::release()
{
  release_common();
  drop_scalars(ws, kmax_cap, spmv_hip_cg_ws_destroy);
  free_vectors({&r, &Ap, &x, &p, &p2, &dot2});
  m_cap = n_cap = -1;
}

void CgWorkspace::ensure(int64_t M, int64_t N_padded, int kmax, int len)
{
  open(2);
  if (!dot2)
    dot2 = _exec.alloc<double>(len);
  regrow_scalars(
      ws, kmax_cap, kmax, kmax > kmax_cap, spmv_hip_cg_ws_destroy,
      [&](auto out) {
        return spmv_hip_cg_ws_create(_exec.context(), kmax, out);
      },
      "spmv_hip_cg_ws_create");
  regrow(m_cap, M, {&r, &Ap}); // cg.cpp:39-40
  if (N_padded > n_cap) { // ensure_p2() brings it back at the new size
    _exec.free(p2);
    p2 = nullptr;
  }
  regrow(n_cap, N_padded, {&x, &p}); // cg.cpp:41-42
}

void CgWorkspace::ensure_p2()
{
  if (!p2 && n_cap > 0)
    p2 = _exec.alloc<double>(n_cap);
}

int cg(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
       const double* b, double* x, int kmax, double rtol,
       std::vector<double>* rnorm_history, const CgOptions* options,
       CgStats* stats, CgWorkspace* workspace)
{
  const Dims dims = check_problem("cg", A, kmax);
  const int64_t M = dims.M, N_padded = dims.N_padded;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  const CgOptions opt = options ? *options : CgOptions();
  spmv_hip_ctx* ctx = exec.context();
  const int len = dot_partials_len(ctx);
  // x is the iterate from the first kernel on (cg.h): it cannot share b
  if (ranges_overlap(x, b, M))
    throw std::runtime_error("cg: x overlaps b (x is updated in place)");

  CgWorkspace own(exec);
  CgWorkspace& w = workspace ? *workspace : own;
  w.ensure(M, N_padded, kmax, len);

  SolveStream guard(exec, w.stream); // every launch below goes to w.stream

  throw_on_error(spmv_hip_cg_ws_reset(w.ws, rtol, nullptr),
                 "spmv_hip_cg_ws_reset");
  double* partials = nullptr;
  throw_on_error(spmv_hip_cg_ws_partials(w.ws, &partials),
                 "spmv_hip_cg_ws_partials");

  // The iterate lives in the caller's x (no copy at the end, cg.cpp:89) unless
  // the mixed mode needs its halo (then in the padded work vector).
  const bool mixed = opt.mixed && A.enable_mixed();
  const bool x_aligned = is_aligned16(x);
  double* const xi = (mixed || !x_aligned) ? w.x : x;
  // CgOptions::defer_x: p_k lives in buffer (k - 1) & 1, every solve starts
  // on buffer 0 with no x update pending
  const bool defer = opt.defer_x && opt.consumer_reductions && comm.size() == 1
                     && !mixed && x_aligned;
  if (defer)
    w.ensure_p2();
  double* const pbuf[2] = {w.p, defer ? w.p2 : w.p};
  // r = p = b, x0 = 0, partials of r.r: one pass (cg.cpp:41-47; x0 and the
  // ghost tails are defined here instead of relying on fresh pages)
  if (N_padded > M) {
    exec.memset<double>(w.p + M, 0, N_padded - M);
    if (defer)
      exec.memset<double>(w.p2 + M, 0, N_padded - M);
    if (mixed)
      exec.memset<double>(w.x + M, 0, N_padded - M);
  }
  exec.memset<double>(w.dot2, 0, len);
  throw_on_error(spmv_hip_cg_init_f64(ctx, w.ws, M, b, w.r, w.p, xi, nullptr),
                 "spmv_hip_cg_init_f64");
  w.flags[0] = 0;
  w.flags[1] = -1;

  // the state words alone (h == nullptr), or with the squared-residual history
  auto read = ws_reader(w.ws, w.flags, spmv_hip_cg_ws_read_async,
                        "spmv_hip_cg_ws_read_async");

  // rnorm0 (cg.cpp:47-50)
  throw_on_error(spmv_hip_cg_reduce_rr(ctx, w.ws, 0, nullptr),
                 "spmv_hip_cg_reduce_rr");
  comm.reduce_sum(ws_slot(w.ws, spmv_hip_cg_ws_rr, 0, "spmv_hip_cg_ws_rr"), 1,
                  w.stream);

  const bool consume = opt.consumer_reductions && comm.size() == 1;
  // whatever happens below, leave the matrix in fp64 mode
  struct MixedGuard {
    const Matrix<double>& A;
    ~MixedGuard() { A.use_mixed(false); }
  } mixed_guard{A};
  // Timing events live in the workspace: a solve that reuses one (the
  // benchmark, after its warm-up) creates nothing inside its timed region.
  std::vector<void*>& timing_ev = w.timing_ev;
  if (opt.time_spmv)
    w.reserve_timing(kmax);
  LaggingPoll poll(exec, w, opt.poll_every, kmax);
  int k = 0;
  while (k < kmax && !poll.stopped) { // cg.cpp:55
    ++k;
    double* const pk = pbuf[(k - 1) & 1];
    col_l2g->update(pk); // cg.cpp:59 (starts on the side stream)
    void* ev1 = nullptr;
    if (opt.time_spmv) {
      ev1 = timing_ev[2 * (size_t)(k - 1) + 1];
      exec.record_event(timing_ev[2 * (size_t)(k - 1)], w.stream);
    }
    // cg.cpp:60,63: Ap = A p with the p.Ap partials produced by the SpMV
    // kernels themselves (local block's share + remote block's share)
    const bool replace
        = mixed && opt.replace_every > 0 && k % opt.replace_every == 0;
    A.use_mixed(mixed);
    if (replace) {
      // residual replacement: the usual iteration in the reference's grouping
      // (x first), then r := b - A x with the fp64 values instead of the
      // recurrence, rr[k] from it, p from both
      const bool fused = A.mult_dot(w.p, w.Ap, partials, w.dot2, ev1);
      if (fused) {
        throw_on_error(spmv_hip_cg_reduce_pAp2(ctx, w.ws, k, w.dot2, nullptr),
                       "spmv_hip_cg_reduce_pAp2");
      } else {
        throw_on_error(spmv_hip_dot_partial_f64(ctx, M, w.p, w.Ap, partials,
                                                nullptr),
                       "spmv_hip_dot_partial_f64");
        throw_on_error(spmv_hip_cg_reduce_pAp(ctx, w.ws, k, nullptr),
                       "spmv_hip_cg_reduce_pAp");
      }
      comm.reduce_sum(ws_slot(w.ws, spmv_hip_cg_ws_pAp, k,
                              "spmv_hip_cg_ws_pAp"),
                      1, w.stream);
      throw_on_error(spmv_hip_cg_update_xr_f64(ctx, w.ws, k, M, w.p, w.Ap, xi,
                                               w.r, nullptr),
                     "spmv_hip_cg_update_xr_f64");
      A.use_mixed(false);
      col_l2g->update(xi);
      A.mult(xi, w.Ap);
      throw_on_error(spmv_hip_cg_residual_f64(ctx, w.ws, 1, M, b, w.Ap, w.r,
                                              nullptr),
                     "spmv_hip_cg_residual_f64");
      throw_on_error(spmv_hip_cg_reduce_rr(ctx, w.ws, k, nullptr),
                     "spmv_hip_cg_reduce_rr");
      comm.reduce_sum(ws_slot(w.ws, spmv_hip_cg_ws_rr, k, "spmv_hip_cg_ws_rr"),
                      1, w.stream);
      throw_on_error(spmv_hip_cg_update_p_f64(ctx, w.ws, k, M, w.r, w.p,
                                              nullptr),
                     "spmv_hip_cg_update_p_f64");
    } else if (consume) {
      // one rank: the update kernels add the partials themselves
      const bool fused = A.mult_dot(pk, w.Ap, partials, w.dot2, ev1);
      if (!fused)
        throw_on_error(spmv_hip_dot_partial_f64(ctx, M, pk, w.Ap, partials,
                                                nullptr),
                       "spmv_hip_dot_partial_f64");
      throw_on_error(spmv_hip_cg_update_r_cs_f64(ctx, w.ws, k, M, w.Ap, w.r,
                                                 fused ? w.dot2 : nullptr,
                                                 nullptr),
                     "spmv_hip_cg_update_r_cs_f64");
      if (!defer)
        throw_on_error(spmv_hip_cg_update_xp_cs_f64(ctx, w.ws, k, M, w.r, xi,
                                                    w.p, nullptr),
                       "spmv_hip_cg_update_xp_cs_f64");
      else if (k & 1) // P step: p_(k+1) into the other buffer, x += a_k p_k waits
        throw_on_error(spmv_hip_cg_update_p2_cs_f64(ctx, w.ws, k, M, w.r, xi,
                                                    pbuf[0], pbuf[1], nullptr),
                       "spmv_hip_cg_update_p2_cs_f64");
      else // X2P step: both x updates, p_(k+1) over p_(k-1) in buffer 0
        throw_on_error(spmv_hip_cg_update_x2p_cs_f64(ctx, w.ws, k, M, w.r, xi,
                                                     pbuf[0], pbuf[1], nullptr),
                       "spmv_hip_cg_update_x2p_cs_f64");
    } else {
      const bool fused = A.mult_dot(w.p, w.Ap, partials, w.dot2, ev1);
      if (fused) {
        throw_on_error(spmv_hip_cg_reduce_pAp2(ctx, w.ws, k, w.dot2, nullptr),
                       "spmv_hip_cg_reduce_pAp2");
      } else {
        throw_on_error(spmv_hip_dot_partial_f64(ctx, M, w.p, w.Ap, partials,
                                                nullptr),
                       "spmv_hip_dot_partial_f64");
        throw_on_error(spmv_hip_cg_reduce_pAp(ctx, w.ws, k, nullptr),
                       "spmv_hip_cg_reduce_pAp");
      }
      comm.reduce_sum(ws_slot(w.ws, spmv_hip_cg_ws_pAp, k,
                              "spmv_hip_cg_ws_pAp"),
                      1, w.stream); // cg.cpp:65
      // r -= alpha Ap with the r.r partials (cg.cpp:66,70,73); the x update
      // of :69 rides with the p update below so p is read once per iteration
      throw_on_error(spmv_hip_cg_update_r_f64(ctx, w.ws, k, M, w.Ap, w.r,
                                              nullptr),
                     "spmv_hip_cg_update_r_f64");
      throw_on_error(spmv_hip_cg_reduce_rr(ctx, w.ws, k, nullptr),
                     "spmv_hip_cg_reduce_rr");
    }
    if (!consume && !replace) {
      comm.reduce_sum(ws_slot(w.ws, spmv_hip_cg_ws_rr, k, "spmv_hip_cg_ws_rr"),
                      1, w.stream); // cg.cpp:75
      // x += alpha p ; stop test ; p = beta p + r   (cg.cpp:69,77-85)
      throw_on_error(spmv_hip_cg_update_xp_f64(ctx, w.ws, k, M, w.r, xi, w.p,
                                               nullptr),
                     "spmv_hip_cg_update_xp_f64");
    }

    poll.step(k, read);
  }

  // The loop ended on a P step: its x update is still pending (the kernel
  // does nothing if the solve has stopped or iteration k met the tolerance).
  if (defer && (k & 1))
    throw_on_error(spmv_hip_cg_flush_x_f64(ctx, w.ws, k, M, pbuf[0], xi,
                                           nullptr),
                   "spmv_hip_cg_flush_x_f64");

  // final state: {done, kstop} and the squared-residual history
  const std::vector<double> rr
      = read_history(spmv_hip_cg_ws_capacity, w.ws, kmax, 1, read);
  double true_rr = -1.0;
  if (mixed) {
    // the true residual of what the mixed loop produced, with the fp64 values
    A.use_mixed(false);
    col_l2g->update(xi);
    A.mult(xi, w.Ap);
    throw_on_error(spmv_hip_cg_residual_f64(ctx, w.ws, 0, M, b, w.Ap, w.r,
                                            nullptr),
                   "spmv_hip_cg_residual_f64");
    throw_on_error(spmv_hip_reduce_partials_f64(ctx, partials, w.dot2, nullptr),
                   "spmv_hip_reduce_partials_f64");
    comm.reduce_sum(w.dot2, 1, w.stream);
    throw_on_error(spmv_hip_copy_d2h_async(ctx, &true_rr, w.dot2,
                                           sizeof(double), nullptr),
                   "spmv_hip_copy_d2h_async");
  }
  if (xi != x)
    exec.copy<double>(x, xi, M); // cg.cpp:89
  exec.synchronize_stream(w.stream);

  if (stats) {
    stats->spmv_launches = 0;
    stats->spmv_ms_total = 0.0;
    if (opt.time_spmv)
      sum_spmv_times(ctx, timing_ev, 2 * (size_t)k, *stats);
  }

  // `done` is raised by the p.Ap reducer of the NEXT iteration; when the loop
  // ends first, the history decides.  Either way the value returned is the
  // reference's k.  (No rule for r_0 . r_0 == 0: that runs to kmax on NaNs.)
  auto rr_at = [&](int j) { return rr[j]; };
  const int k_final
      = w.flags[0] != 0 ? w.flags[1] : first_k_below(rr_at, k, rtol);
  write_history(rnorm_history, k_final, rr_at);
  if (mixed) {
    const double rnorm0 = std::sqrt(rr[0]);
    const double true_rel = rnorm0 > 0 ? std::sqrt(true_rr) / rnorm0 : 0.0;
    int extra = 0;
    double final_rel = true_rel;
    if (true_rel >= rtol && rtol > 0 && k_final < kmax) {
      // The fp32 values took the iteration as far as they could: solve the
      // correction equation A d = b - A x with the fp64 values (w.r still
      // holds that residual) and add it.  A fresh workspace: this one's
      // vectors are the operands.
      A.use_mixed(false);
      double* d = exec.alloc<double>(M);
      double* rhs = exec.alloc<double>(M);
      exec.copy<double>(rhs, w.r, M);
      exec.synchronize_stream(w.stream);
      exec.set_stream(guard.prev);
      std::vector<double> h2;
      CgOptions o2 = opt;
      o2.mixed = false;
      o2.time_spmv = false;
      try {
        extra = cg(comm, exec, A, rhs, d, kmax - k_final, rtol / true_rel, &h2,
                   &o2, nullptr, nullptr);
        throw_on_error(spmv_hip_axpy_f64(ctx, M, 1.0, d, x, nullptr),
                       "spmv_hip_axpy_f64");
        exec.synchronize();
      } catch (...) {
        exec.free(d);
        exec.free(rhs);
        throw;
      }
      exec.free(d);
      exec.free(rhs);
      if (!h2.empty() && rnorm0 > 0)
        final_rel = h2.back() / rnorm0;
      if (rnorm_history)
        for (size_t j = 1; j < h2.size(); ++j)
          rnorm_history->push_back(h2[j]);
    }
    if (stats) {
      // iterations enqueued past the converged one were no-ops on the device
      stats->replacements
          = opt.replace_every > 0 ? k_final / opt.replace_every : 0;
      stats->true_rel_residual = true_rel;
      stats->continuation_iterations = extra;
      stats->final_true_rel_residual = final_rel;
    }
    return k_final + extra;
  }
  return k_final;
}

// ---------------------------------------------------------------------------
// cg_block: see cg.h.  Per iteration (compute stream), on any number of ranks:
//     halo of the block P on the map's side stream
//     mult_block: local block [wait halo event] remote block
//     block dot partials of p.Ap ; reducer -> pAp[k][0:nrhs] ; all-reduce
//     r -= alpha_c Ap with the r.r partials ; reducer -> rr[k][0:nrhs] ; all-reduce
//     x += alpha_c p ; stop test ; p = beta_c p + r
// The two all-reduces carry nrhs doubles each (Comm::reduce_sum: the peer
// windows up to SPMV_HIP_REDUCE_MAX_COUNT doubles, the transport's all-reduce
// beyond; every rank takes the same branch, nrhs being collective).
// ---------------------------------------------------------------------------
CgBlockWorkspace::~CgBlockWorkspace() { release(); }

void CgBlockWorkspace::release()
{
  release_common();
  drop_scalars(ws, kmax_cap, spmv_hip_cgb_ws_destroy);
  free_vectors({&r, &Ap, &x, &p});
  nrhs_cap = 0;
  m_cap = n_cap = x_cap = -1;
}

void CgBlockWorkspace::ensure(int64_t m_elems, int64_t n_elems, int kmax,
                              int nrhs, bool need_x)
{
  open(SPMV_HIP_CGB_STATE_WORDS);
  regrow_scalars(
      ws, kmax_cap, kmax, kmax > kmax_cap || nrhs != nrhs_cap,
      spmv_hip_cgb_ws_destroy,
      [&](auto out) {
        nrhs_cap = 0; // while they are gone
        return spmv_hip_cgb_ws_create(_exec.context(), kmax, nrhs, out);
      },
      "spmv_hip_cgb_ws_create");
  nrhs_cap = nrhs;
  regrow(m_cap, m_elems, {&r, &Ap});
  if (need_x)
    regrow(x_cap, m_elems, {&x});
  regrow(n_cap, n_elems, {&p});
}
int cg_block(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
             const double* B, double* X, int nrhs, int kmax, double rtol,
             std::vector<int>* iterations, std::vector<double>* rnorm_history,
             const CgOptions* options, CgStats* stats,
             CgBlockWorkspace* workspace)
{
  const Dims dims = check_problem("cg_block", A, kmax);
  if (nrhs < 1 || nrhs > SPMV_HIP_CGB_MAX_NRHS)
    throw std::runtime_error("spmv::cg_block - Error: nrhs must be in 1..8");
  const int64_t M = dims.M;
  const int64_t m_elems = M * nrhs, n_elems = dims.N_padded * nrhs;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  const CgOptions opt = options ? *options : CgOptions();
  spmv_hip_ctx* ctx = exec.context();
  // X is the iterate from the first kernel on (cg.h): it cannot share B
  if (ranges_overlap(X, B, m_elems))
    throw std::runtime_error("cg_block: X overlaps B (X is updated in place)");

  CgBlockWorkspace own(exec);
  CgBlockWorkspace& w = workspace ? *workspace : own;
  const bool x_aligned = is_aligned16(X);
  w.ensure(m_elems, n_elems, kmax, nrhs, !x_aligned);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  SolveStream guard(exec, w.stream); // every launch below goes to w.stream

  throw_on_error(spmv_hip_cgb_ws_reset(w.ws, rtol, nullptr),
                 "spmv_hip_cgb_ws_reset");
  double* const Xi = x_aligned ? X : w.x;
  // R = P = B, X0 = 0, partials of r.r: one pass (cg.cpp:41-47); the ghost
  // tail of P is defined here instead of relying on fresh pages
  if (n_elems > m_elems)
    exec.memset<double>(w.p + m_elems, 0, n_elems - m_elems);
  throw_on_error(spmv_hip_cgb_init_f64(ctx, w.ws, M, B, w.r, w.p, Xi, nullptr),
                 "spmv_hip_cgb_init_f64");
  for (int i = 0; i < SPMV_HIP_CGB_STATE_WORDS; ++i)
    w.flags[i] = i > SPMV_HIP_CGB_MAX_NRHS ? -1 : 0;

  // the state words alone (h == nullptr), or with the squared-residual history
  auto read = [&](double* h, size_t n) {
    throw_on_error(spmv_hip_cgb_ws_read_async(w.ws, w.flags,
                                              SPMV_HIP_CGB_STATE_WORDS, h, n,
                                              nullptr),
                   "spmv_hip_cgb_ws_read_async");
  };

  // rnorm0 of every column (cg.cpp:47-50)
  throw_on_error(spmv_hip_cgb_reduce_rr(ctx, w.ws, 0, nullptr),
                 "spmv_hip_cgb_reduce_rr");
  comm.reduce_sum(ws_slot(w.ws, spmv_hip_cgb_ws_rr, 0, "spmv_hip_cgb_ws_rr"),
                  nrhs, w.stream);

  std::vector<void*>& timing_ev = w.timing_ev;
  LaggingPoll poll(exec, w, opt.poll_every, kmax); // looks at all_done
  int k = 0;
  while (k < kmax && !poll.stopped) { // cg.cpp:55
    ++k;
    col_l2g->update_block(w.p, nrhs); // cg.cpp:59 (starts on the side stream)
    void* ev1 = nullptr;
    if (opt.time_spmv) {
      ev1 = timing_ev[2 * (size_t)(k - 1) + 1];
      exec.record_event(timing_ev[2 * (size_t)(k - 1)], w.stream);
    }
    // cg.cpp:60: not guarded by the state -- what it leaves in the columns
    // that have stopped is not used
    A.mult_block(w.p, w.Ap, nrhs, ev1);
    throw_on_error(spmv_hip_cgb_dot_f64(ctx, w.ws, M, w.p, w.Ap, nullptr),
                   "spmv_hip_cgb_dot_f64"); // cg.cpp:63
    throw_on_error(spmv_hip_cgb_reduce_pAp(ctx, w.ws, k, nullptr),
                   "spmv_hip_cgb_reduce_pAp");
    comm.reduce_sum(ws_slot(w.ws, spmv_hip_cgb_ws_pAp, k,
                            "spmv_hip_cgb_ws_pAp"),
                    nrhs, w.stream); // cg.cpp:65
    throw_on_error(spmv_hip_cgb_update_r_f64(ctx, w.ws, k, M, w.Ap, w.r,
                                             nullptr),
                   "spmv_hip_cgb_update_r_f64"); // cg.cpp:66,70,73
    throw_on_error(spmv_hip_cgb_reduce_rr(ctx, w.ws, k, nullptr),
                   "spmv_hip_cgb_reduce_rr");
    comm.reduce_sum(ws_slot(w.ws, spmv_hip_cgb_ws_rr, k, "spmv_hip_cgb_ws_rr"),
                    nrhs, w.stream); // cg.cpp:75
    throw_on_error(spmv_hip_cgb_update_xp_f64(ctx, w.ws, k, M, w.r, Xi, w.p,
                                              nullptr),
                   "spmv_hip_cgb_update_xp_f64"); // cg.cpp:69,77-85

    poll.step(k, read);
  }

  // final state and the squared-residual history, nrhs doubles per iteration
  const std::vector<double> rr = read_history(
      +[](const spmv_hip_cgb_ws* s, int* cap) {
        int cap_nrhs = 0;
        return spmv_hip_cgb_ws_capacity(s, cap, &cap_nrhs);
      },
      w.ws, kmax, (size_t)nrhs, read);
  if (Xi != X)
    exec.copy<double>(X, Xi, m_elems);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    if (opt.time_spmv)
      sum_spmv_times(ctx, timing_ev, 2 * (size_t)k, *stats);
  }

  if (iterations)
    iterations->assign(nrhs, 0);
  if (rnorm_history)
    rnorm_history->assign((size_t)nrhs * ((size_t)kmax + 1), -1.0);
  int k_max = 0;
  for (int c = 0; c < nrhs; ++c) {
    auto rr_at = [&](int j) { return rr[(size_t)j * nrhs + c]; };
    int kc;
    if (w.flags[1 + c] != 0)
      kc = w.flags[1 + SPMV_HIP_CGB_MAX_NRHS + c];
    else if (rr_at(0) == 0.0)
      kc = 0; // (kmax == 0: no reducer ran to say so)
    else // done[c] is raised by the p.Ap reducer of the NEXT iteration
      kc = first_k_below(rr_at, k, rtol);
    k_max = std::max(k_max, kc);
    if (iterations)
      (*iterations)[c] = kc;
    if (rnorm_history)
      for (int j = 0; j <= kc; ++j)
        (*rnorm_history)[(size_t)c * ((size_t)kmax + 1) + j]
            = std::sqrt(rr_at(j));
  }
  return k_max;
}

} // namespace spmv
