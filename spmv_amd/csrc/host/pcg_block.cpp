// spmv::sgs_apply_block and spmv::pcg_block for HipExecutor: see cg.h.
#include "cg.h"

#include "solver_common.h"

namespace spmv
{
using namespace detail;

void sgs_apply_block(HipExecutor& exec, const SgsPreconditioner& M,
                     const double* R, double* Z, int nrhs)
{
  if (nrhs < 1 || nrhs > SPMV_HIP_CGB_MAX_NRHS)
    throw std::runtime_error(
        "spmv::sgs_apply_block - Error: nrhs must be in 1..8");
  const int64_t elems = (int64_t)M.rows() * nrhs;
  if (ranges_overlap(Z, R, elems))
    throw std::runtime_error("sgs_apply_block: Z overlaps R");
  if (elems > 0 && (!R || !Z))
    throw std::runtime_error("sgs_apply_block: NULL vector");
  throw_on_error(spmv_hip_mcgs_apply_block_f64(exec.context(), M.plan(), nullptr,
                                               R, Z, nrhs, nullptr),
                 "spmv_hip_mcgs_apply_block_f64");
}

// ---------------------------------------------------------------------------
// pcg_block: see cg.h.  Per iteration (compute stream), on any number of ranks:
//     halo of the block P on the map's side stream
//     mult_block: local block [wait halo event] remote block
//     block dot partials of p.Ap ; reducer -> pAp[k][0:nrhs] ; all-reduce of nrhs
//     r -= alpha_c Ap with the r.r partials
//     Z = M^-1 R: the 2C - 1 block sweeps or the block V-cycle and the r.z
//       partials, or (dinv) both in one kernel
//     reducer -> {rz[k], rr[k]}[0:nrhs] ; all-reduce of 2 nrhs
//     x += alpha_c p ; stop test ; p = beta_c p + z
// ---------------------------------------------------------------------------
PcgBlockWorkspace::~PcgBlockWorkspace() { release(); }

void PcgBlockWorkspace::release()
{
  release_common();
  drop_scalars(ws, kmax_cap, spmv_hip_pcgb_ws_destroy);
  single.reset();
  free_vectors({&r, &Ap, &z, &x, &p});
  nrhs_cap = 0;
  m_cap = n_cap = x_cap = -1;
}

void PcgBlockWorkspace::ensure(int64_t m_elems, int64_t n_elems, int kmax,
                               int nrhs, bool need_x)
{
  open(SPMV_HIP_CGB_STATE_WORDS);
  regrow_scalars(
      ws, kmax_cap, kmax, kmax > kmax_cap || nrhs != nrhs_cap,
      spmv_hip_pcgb_ws_destroy,
      [&](auto out) {
        nrhs_cap = 0; // while they are gone
        return spmv_hip_pcgb_ws_create(_exec.context(), kmax, nrhs, out);
      },
      "spmv_hip_pcgb_ws_create");
  nrhs_cap = nrhs;
  regrow(m_cap, m_elems, {&r, &Ap, &z});
  if (need_x)
    regrow(x_cap, m_elems, {&x});
  regrow(n_cap, n_elems, {&p});
}

int pcg_block(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
              const double* B, double* X, int nrhs, const BlockPreconditioner& M,
              int kmax, double rtol, std::vector<int>* iterations,
              std::vector<double>* rnorm_history, const CgOptions* options,
              CgStats* stats, PcgBlockWorkspace* workspace)
{
  // (rows() and negative_pivots() are host fields of the object)
  const int64_t rows = A.row_map()->local_size();
  pcg_block_check_rules(nrhs, kmax, M.dinv != nullptr, M.sgs != nullptr,
                        M.amg != nullptr, M.sgs ? M.sgs->rows() : 0,
                        M.sgs ? M.sgs->negative_pivots() : 0,
                        M.amg ? M.amg->rows(0) : 0, rows, B, X, M.dinv);
  if (M.amg && nrhs == 1) { // a block of one column: pcg_amg itself
    PcgBlockWorkspace own1(exec);
    PcgBlockWorkspace& w1 = workspace ? *workspace : own1;
    if (!w1.single)
      w1.single = std::make_unique<SgsWorkspace>(exec);
    std::vector<double> hist;
    const int k = pcg_amg(comm, exec, A, *M.amg, B, X, kmax, rtol, &hist,
                          options, stats, w1.single.get());
    if (iterations)
      iterations->assign(1, k);
    if (rnorm_history) {
      rnorm_history->assign((size_t)kmax + 1, -1.0);
      std::copy(hist.begin(), hist.end(), rnorm_history->begin());
    }
    return k;
  }
  const Dims dims = check_problem("pcg_block", A, kmax);
  const int64_t M_rows = dims.M;
  const int64_t m_elems = M_rows * nrhs, n_elems = dims.N_padded * nrhs;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  const CgOptions opt = options ? *options : CgOptions();
  spmv_hip_ctx* ctx = exec.context();
  const spmv_hip_mcgs_plan* plan = M.sgs ? M.sgs->plan() : nullptr;

  PcgBlockWorkspace own(exec);
  PcgBlockWorkspace& w = workspace ? *workspace : own;
  const bool x_aligned = is_aligned16(X);
  w.ensure(m_elems, n_elems, kmax, nrhs, !x_aligned);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  SolveStream guard(exec, w.stream); // every launch below goes to w.stream

  throw_on_error(spmv_hip_pcgb_ws_reset(w.ws, rtol, nullptr),
                 "spmv_hip_pcgb_ws_reset");
  double* const Xi = x_aligned ? X : w.x;
  // the ghost tail of P is defined here instead of relying on fresh pages
  if (n_elems > m_elems)
    exec.memset<double>(w.p + m_elems, 0, n_elems - m_elems);

  // Z = M^-1 R and the partials of r.z
  auto precondition = [&] {
    if (plan)
      throw_on_error(spmv_hip_mcgs_apply_block_f64(ctx, plan, w.ws, w.r, w.z,
                                                   nrhs, nullptr),
                     "spmv_hip_mcgs_apply_block_f64");
    else if (M.amg) // (on the object's own scratch, stopped columns included)
      amg_apply_block(exec, *M.amg, w.r, w.z, nrhs);
    throw_on_error(spmv_hip_pcgb_dot_rz_f64(ctx, w.ws, M_rows, M.dinv, w.r, w.z,
                                            nullptr),
                   "spmv_hip_pcgb_dot_rz_f64");
  };
  // {rz[k], rr[k]} of every column: one all-reduce of 2 nrhs doubles
  auto reduce_rz_rr = [&](int k) {
    throw_on_error(spmv_hip_pcgb_reduce_rz_rr(ctx, w.ws, k, nullptr),
                   "spmv_hip_pcgb_reduce_rz_rr");
    comm.reduce_sum(ws_slot(w.ws, spmv_hip_pcgb_ws_rz_rr, k,
                            "spmv_hip_pcgb_ws_rz_rr"),
                    2 * (size_t)nrhs, w.stream);
  };

  // R = B, X0 = 0, partials of r.r: one pass; then Z0 = M^-1 R0 and P1 = Z0
  throw_on_error(spmv_hip_pcgb_init_f64(ctx, w.ws, M_rows, B, w.r, Xi, nullptr),
                 "spmv_hip_pcgb_init_f64");
  precondition();
  exec.copy<double>(w.p, w.z, m_elems);
  for (int i = 0; i < SPMV_HIP_CGB_STATE_WORDS; ++i)
    w.flags[i] = i > SPMV_HIP_CGB_MAX_NRHS ? -1 : 0;

  // the state words alone (h == nullptr), or with the history of {rz, rr}
  auto read = [&](double* h, size_t n) {
    throw_on_error(spmv_hip_pcgb_ws_read_async(w.ws, w.flags,
                                               SPMV_HIP_CGB_STATE_WORDS, h, n,
                                               nullptr),
                   "spmv_hip_pcgb_ws_read_async");
  };

  reduce_rz_rr(0);

  std::vector<void*>& timing_ev = w.timing_ev;
  LaggingPoll poll(exec, w, opt.poll_every, kmax); // looks at all_done
  int k = 0;
  while (k < kmax && !poll.stopped) {
    ++k;
    col_l2g->update_block(w.p, nrhs); // starts on the side stream
    void* ev1 = nullptr;
    if (opt.time_spmv) {
      ev1 = timing_ev[2 * (size_t)(k - 1) + 1];
      exec.record_event(timing_ev[2 * (size_t)(k - 1)], w.stream);
    }
    // not guarded by the state: what it leaves in the columns that have
    // stopped is not used
    A.mult_block(w.p, w.Ap, nrhs, ev1);
    throw_on_error(spmv_hip_pcgb_dot_pAp_f64(ctx, w.ws, M_rows, w.p, w.Ap,
                                             nullptr),
                   "spmv_hip_pcgb_dot_pAp_f64");
    throw_on_error(spmv_hip_pcgb_reduce_pAp(ctx, w.ws, k, nullptr),
                   "spmv_hip_pcgb_reduce_pAp");
    comm.reduce_sum(ws_slot(w.ws, spmv_hip_pcgb_ws_pAp, k,
                            "spmv_hip_pcgb_ws_pAp"),
                    nrhs, w.stream);
    throw_on_error(spmv_hip_pcgb_update_r_f64(ctx, w.ws, k, M_rows, w.Ap, w.r,
                                              nullptr),
                   "spmv_hip_pcgb_update_r_f64");
    precondition();
    reduce_rz_rr(k);
    throw_on_error(spmv_hip_pcgb_update_xp_f64(ctx, w.ws, k, M_rows, w.z, Xi,
                                               w.p, nullptr),
                   "spmv_hip_pcgb_update_xp_f64");

    poll.step(k, read);
  }

  // final state and the history, 2 nrhs doubles per iteration
  const std::vector<double> zr = read_history(
      +[](const spmv_hip_pcgb_ws* s, int* cap) {
        int cap_nrhs = 0;
        return spmv_hip_pcgb_ws_capacity(s, cap, &cap_nrhs);
      },
      w.ws, kmax, 2 * (size_t)nrhs, read);
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
    auto rr_at = [&](int j) { return zr[(2 * (size_t)j + 1) * nrhs + c]; };
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
