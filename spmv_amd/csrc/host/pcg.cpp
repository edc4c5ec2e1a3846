// spmv::pcg, the Chebyshev polynomial preconditioner and the multicolour
// symmetric Gauss-Seidel preconditioner for HipExecutor: see cg.h.
#include "cg.h"

#include <algorithm>
#include <chrono>
#include <initializer_list>
#include <limits>
#include <string>
#include <type_traits>
#include <utility>

#include "sgs_build.h"
#include "solver_common.h"

namespace spmv
{
using namespace detail;

// ---------------------------------------------------------------------------
// pcg, pcg_chebyshev and pcg_sgs (see cg.h) are one frame, pcg_solve(), on one
// set of device scalars (spmv_hip_pcg_ws) and reducers.  On the compute stream:
//     prologue: checks, workspace, aligned copies, ghost tails, ws_reset
//     [init]    r = b, x = 0, z0 = M(r0), p1 = z0, partials of r.z and r.r
//     reduce_rz_rr(0) ; all-reduce of 2
//     k = 1..kmax, until the lagging poll sees `done`:
//       [body]  spmv_and_pAp: halo start of p on the map's side stream ;
//                 Ap = A p (+ fused p.Ap share, else dot_partial) ;
//                 reduce_pAp(2) ; all-reduce of 1
//               [update r, z = M(r), partials of r.z and r.r]
//               reduce_rz_rr(k) ; all-reduce of 2
//               [update x ; stop test ; update p]
//     epilogue: history, copy back of an unaligned x, sync, times, k_final
// A solver plugs in what stands in brackets:
//   pcg            init; one rank with consumer_reductions: spmv_and_pAp
//                  without its reducer, update_r_cs (pAp[k]; r; r.z, r.r),
//                  update_xp_cs ({rz,rr}[k]; x; p): 3 launches; otherwise
//                  update_r and update_xp in the two slots: 5 launches.
//                  z = dinv*r is not stored.  Beside the SpMV 10 vector passes
//                  (update_r: Ap, r, dinv in, r out; update_xp: r, dinv, x, p
//                  in, x, p out) where cg() without defer_x streams 8.
//   pcg_chebyshev  cheb_init / cheb_update_r (r ; partials of r.r ; step 0 of
//                  M: d, z), then degree - 1 times: halo start of z ; w = A z ;
//                  cheb_step (the last one: partials of r.z, no d); all
//                  `degree` SpMVs of an iteration are timed.  degree SpMVs +
//                  degree + 1 streaming launches + 2 reducers; beside the SpMVs
//                  7 (degree - 1) + 11 vector passes with a dinv for degree >=
//                  2 (update_r: Ap, r, dinv in, r, d, z out; a step: w, r,
//                  dinv, d, z in, d, z out, the last one without d out;
//                  update_xp: z, x, p in, x, p out), 10 for degree 1.
//   pcg_sgs        sgs_init / sgs_update_r (r ; partials of r.r), then the 2C -
//                  1 sweeps of z = M^-1 r (local: no halo) and sgs_dot_rz
//                  (partials of r.z).
// The last two keep z and share cheb_update_xp (x ; stop test ; p).
// ---------------------------------------------------------------------------
void PcgFamilyWorkspace::ensure_common(int64_t M, int kmax, int len,
                                       bool need_x,
                                       std::initializer_list<double**> m_vecs)
{
  open(2);
  if (!dot2)
    dot2 = _exec.alloc<double>(len);
  // the device scalars of the family for up to kmax iterations
  regrow_scalars(
      ws, kmax_cap, kmax, kmax > kmax_cap, spmv_hip_pcg_ws_destroy,
      [&](auto out) {
        return spmv_hip_pcg_ws_create(_exec.context(), kmax, out);
      },
      "spmv_hip_pcg_ws_create");
  regrow(m_cap, M, m_vecs);
  if (need_x)
    regrow(x_cap, M, {&x});
}

void PcgFamilyWorkspace::release_family(
    std::initializer_list<double**> own_vecs)
{
  release_common();
  drop_scalars(ws, kmax_cap, spmv_hip_pcg_ws_destroy);
  free_vectors({&r, &Ap, &x, &p, &dot2});
  free_vectors(own_vecs);
  m_cap = n_cap = x_cap = -1;
}

PcgWorkspace::~PcgWorkspace() { release(); }

void PcgWorkspace::release()
{
  release_family({&dinv});
  dinv_cap = -1;
}

void PcgWorkspace::ensure(int64_t M, int64_t N_padded, int kmax, int len,
                          bool need_x, bool need_dinv)
{
  ensure_common(M, kmax, len, need_x, {&r, &Ap});
  if (need_dinv)
    regrow(dinv_cap, M, {&dinv});
  regrow(n_cap, N_padded, {&p});
}

ChebyshevWorkspace::~ChebyshevWorkspace() { release(); }

void ChebyshevWorkspace::release()
{
  release_family({&d, &w, &z, &dinv});
  dinv_cap = -1;
}

void ChebyshevWorkspace::ensure(int64_t M, int64_t N_padded, int kmax, int len,
                                bool need_x, bool need_dinv)
{
  ensure_common(M, kmax, len, need_x, {&r, &Ap, &d, &w});
  if (need_dinv)
    regrow(dinv_cap, M, {&dinv});
  regrow(n_cap, N_padded, {&p, &z});
}

SgsWorkspace::~SgsWorkspace() { release(); }

void SgsWorkspace::release() { release_family({&z}); }

void SgsWorkspace::ensure(int64_t M, int64_t N_padded, int kmax, int len,
                          bool need_x)
{
  ensure_common(M, kmax, len, need_x, {&r, &Ap, &z});
  regrow(n_cap, N_padded, {&p});
}

namespace
{
// What a solve of the family holds between its prologue and its epilogue, and
// the two steps that every loop body is made of.  W: the solver's workspace.
template <class W>
struct PcgSolve {
  const Comm& comm;
  HipExecutor& exec;
  const Matrix<double>& A;
  const L2GMap& col_l2g;
  spmv_hip_ctx* const ctx;
  const CgOptions& opt;
  W& w;
  const int64_t M;
  double* const xi;       // the iterate: the caller's x, or w.x
  const double* const di; // the caller's dinv, w.dinv, or null
  double* const partials;
  size_t ev_next = 0; // two events per timed SpMV

  // Ap = A p with the p.Ap partials produced by the SpMV kernels themselves
  // (local block's share + remote block's share, the latter in w.dot2) where
  // they can: returns whether they did.  reduce: pAp[k] is finished by its
  // reducer and the all-reduce of 1 (a consumer kernel adds the partials
  // itself).
  bool spmv_and_pAp(int k, bool reduce)
  {
    col_l2g.update(w.p); // starts on the side stream
    void* ev1 = nullptr;
    if (opt.time_spmv) {
      ev1 = w.timing_ev[ev_next + 1];
      exec.record_event(w.timing_ev[ev_next], w.stream);
      ev_next += 2;
    }
    const bool fused = A.mult_dot(w.p, w.Ap, partials, w.dot2, ev1);
    if (!fused)
      throw_on_error(spmv_hip_dot_partial_f64(ctx, M, w.p, w.Ap, partials,
                                              nullptr),
                     "spmv_hip_dot_partial_f64");
    if (reduce) {
      if (fused)
        throw_on_error(spmv_hip_pcg_reduce_pAp2(ctx, w.ws, k, w.dot2, nullptr),
                       "spmv_hip_pcg_reduce_pAp2");
      else
        throw_on_error(spmv_hip_pcg_reduce_pAp(ctx, w.ws, k, nullptr),
                       "spmv_hip_pcg_reduce_pAp");
      comm.reduce_sum(ws_slot(w.ws, spmv_hip_pcg_ws_pAp, k,
                              "spmv_hip_pcg_ws_pAp"),
                      1, w.stream);
    }
    return fused;
  }

  // {rz[k], rr[k]} from their partials: one all-reduce of 2 doubles
  void reduce_rz_rr(int k)
  {
    throw_on_error(spmv_hip_pcg_reduce_rz_rr(ctx, w.ws, k, nullptr),
                   "spmv_hip_pcg_reduce_rz_rr");
    comm.reduce_sum(ws_slot(w.ws, spmv_hip_pcg_ws_rz_rr, k,
                            "spmv_hip_pcg_ws_rz_rr"),
                    2, w.stream);
  }
};

// The frame described at the top for spmv::<who>.  dinv may be null where the
// solver allows it (pcg_sgs has none); more_tails: the padded vectors beside p
// whose ghost tail is zeroed; init(s) and body(s, k) are the solver's slots,
// inlined here.  Returns k_final.
template <class W, class Init, class Body>
int pcg_solve(const char* who, const Comm& comm, HipExecutor& exec,
              const Matrix<double>& A, const Dims& dims, const double* b,
              double* x, const double* dinv, int kmax, double rtol,
              std::vector<double>* rnorm_history, const CgOptions& opt,
              CgStats* stats, W* workspace, int spmvs_per_iteration,
              std::initializer_list<double* W::*> more_tails, Init&& init,
              Body&& body)
{
  constexpr bool has_dinv = !std::is_same<W, SgsWorkspace>::value;
  const int64_t M = dims.M, N_padded = dims.N_padded;
  spmv_hip_ctx* ctx = exec.context();
  const int len = dot_partials_len(ctx);
  // x is the iterate from the first kernel on: it cannot share b or dinv
  if (ranges_overlap(x, b, M))
    throw std::runtime_error(std::string(who)
                             + ": x overlaps b (x is updated in place)");
  if (dinv && ranges_overlap(x, dinv, M))
    throw std::runtime_error(std::string(who)
                             + ": x overlaps dinv (x is updated in place)");

  W own(exec);
  W& w = workspace ? *workspace : own;
  const bool x_aligned = is_aligned16(x);
  const bool dinv_aligned = is_aligned16(dinv);
  if constexpr (has_dinv)
    w.ensure(M, N_padded, kmax, len, !x_aligned, !dinv_aligned);
  else
    w.ensure(M, N_padded, kmax, len, !x_aligned);
  if (opt.time_spmv)
    w.reserve_timing(kmax * spmvs_per_iteration);

  SolveStream guard(exec, w.stream); // every launch below goes to w.stream

  throw_on_error(spmv_hip_pcg_ws_reset(w.ws, rtol, nullptr),
                 "spmv_hip_pcg_ws_reset");
  double* partials = nullptr;
  throw_on_error(spmv_hip_pcg_ws_partials(w.ws, &partials),
                 "spmv_hip_pcg_ws_partials");

  const double* di = dinv;
  if constexpr (has_dinv) {
    if (dinv && !dinv_aligned) { // the streaming kernels load 16 bytes at a time
      exec.copy<double>(w.dinv, dinv, M);
      di = w.dinv;
    }
  }
  // the ghost tails are defined here instead of relying on fresh pages
  if (N_padded > M) {
    exec.memset<double>(w.p + M, 0, N_padded - M);
    for (double* W::*v : more_tails)
      exec.memset<double>(w.*v + M, 0, N_padded - M);
  }
  exec.memset<double>(w.dot2, 0, len);

  PcgSolve<W> s{comm, exec, A, *dims.col_l2g, ctx, opt, w, M,
                x_aligned ? x : w.x, di, partials};
  init(s);
  w.flags[0] = 0;
  w.flags[1] = -1;

  // the state words alone (h == nullptr), or with the history of pairs
  auto read = ws_reader(w.ws, w.flags, spmv_hip_pcg_ws_read_async,
                        "spmv_hip_pcg_ws_read_async");

  s.reduce_rz_rr(0);
  LaggingPoll poll(exec, w, opt.poll_every, kmax);
  int k = 0;
  while (k < kmax && !poll.stopped) {
    ++k;
    body(s, k);
    poll.step(k, read);
  }

  // final state: {done, kstop} and the history of pairs {rz[k], rr[k]}
  const std::vector<double> zr
      = read_history(spmv_hip_pcg_ws_capacity, w.ws, kmax, 2, read);
  if (s.xi != x)
    exec.copy<double>(x, s.xi, M);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    if (opt.time_spmv)
      sum_spmv_times(ctx, w.timing_ev, s.ev_next, *stats);
  }

  auto rr_at = [&](int j) { return zr[2 * (size_t)j + 1]; };
  int k_final;
  if (w.flags[0] != 0)
    k_final = w.flags[1];
  else if (rr_at(0) == 0.0)
    k_final = 0; // (kmax == 0: no kernel ran to say so)
  else // `done` is raised by the first launch of the NEXT iteration
    k_final = first_k_below(rr_at, k, rtol);
  write_history(rnorm_history, k_final, rr_at);
  return k_final;
}

// An iteration of the two solvers that keep z: update_r() updates r and
// leaves z = M(r) with the partials of r.z and r.r
template <class W, class UpdateR>
void stored_z_iteration(PcgSolve<W>& s, int k, UpdateR&& update_r)
{
  s.spmv_and_pAp(k, true);
  update_r();
  s.reduce_rz_rr(k); // rz[k] and rr[k] at once
  throw_on_error(spmv_hip_cheb_update_xp_f64(s.ctx, s.w.ws, k, s.M, s.w.z, s.xi,
                                             s.w.p, nullptr),
                 "spmv_hip_cheb_update_xp_f64");
}
} // namespace

void jacobi_inverse(HipExecutor& exec, const double* d, double* dinv, int64_t n)
{
  if (n < 0)
    throw std::runtime_error("spmv::jacobi_inverse - Error: n < 0");
  int32_t* count = exec.alloc<int32_t>(1);
  int32_t bad = 0;
  try {
    throw_on_error(spmv_hip_jacobi_invert_f64(exec.context(), n, d, dinv, count,
                                              nullptr),
                   "spmv_hip_jacobi_invert_f64");
    exec.copy_to<int32_t>(&bad, exec.get_host(), count, 1); // waits
  } catch (...) {
    exec.free(count);
    throw;
  }
  exec.free(count);
  if (bad != 0)
    throw std::runtime_error(
        "spmv::jacobi_inverse - Error: the diagonal is not positive ("
        + std::to_string(bad) + " of " + std::to_string(n)
        + " entries are not finite or not > 0)");
}

int pcg(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
        const double* b, double* x, const double* dinv, int kmax, double rtol,
        std::vector<double>* rnorm_history, const CgOptions* options,
        CgStats* stats, PcgWorkspace* workspace)
{
  const Dims dims = check_problem("pcg", A, kmax);
  const CgOptions opt = options ? *options : CgOptions();
  // one rank: the update kernels add the partials themselves
  const bool consume = opt.consumer_reductions && comm.size() == 1;
  using Solve = PcgSolve<PcgWorkspace>;
  return pcg_solve(
      "pcg", comm, exec, A, dims, b, x, dinv, kmax, rtol, rnorm_history, opt,
      stats, workspace, 1, {},
      // r = b, x0 = 0, p = dinv*b, partials of r.z and r.r: one pass
      [&](Solve& s) {
        throw_on_error(spmv_hip_pcg_init_f64(s.ctx, s.w.ws, s.M, b, s.di, s.w.r,
                                             s.w.p, s.xi, nullptr),
                       "spmv_hip_pcg_init_f64");
      },
      [&](Solve& s, int k) {
        PcgWorkspace& w = s.w;
        const bool fused = s.spmv_and_pAp(k, !consume);
        if (consume) {
          throw_on_error(spmv_hip_pcg_update_r_cs_f64(
                             s.ctx, w.ws, k, s.M, w.Ap, s.di, w.r,
                             fused ? w.dot2 : nullptr, nullptr),
                         "spmv_hip_pcg_update_r_cs_f64");
          throw_on_error(spmv_hip_pcg_update_xp_cs_f64(s.ctx, w.ws, k, s.M, w.r,
                                                       s.di, s.xi, w.p, nullptr),
                         "spmv_hip_pcg_update_xp_cs_f64");
        } else {
          throw_on_error(spmv_hip_pcg_update_r_f64(s.ctx, w.ws, k, s.M, w.Ap,
                                                   s.di, w.r, nullptr),
                         "spmv_hip_pcg_update_r_f64");
          s.reduce_rz_rr(k); // rz[k] and rr[k] at once
          throw_on_error(spmv_hip_pcg_update_xp_f64(s.ctx, w.ws, k, s.M, w.r,
                                                    s.di, s.xi, w.p, nullptr),
                         "spmv_hip_pcg_update_xp_f64");
        }
      });
}

// (chebyshev_coefficients: solver_args.cpp)
void chebyshev_apply(HipExecutor& exec, const Matrix<double>& A,
                     const double* r, double* z, const double* dinv, int degree,
                     double lmin, double lmax, ChebyshevWorkspace* workspace)
{
  double ca[kChebyshevMaxDegree], cb[kChebyshevMaxDegree];
  chebyshev_coefficients(degree, lmin, lmax, ca, cb);
  const Dims dims = check_problem("chebyshev_apply", A, 0);
  const int64_t M = dims.M, N_padded = dims.N_padded;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  if (ranges_overlap(z, r, M))
    throw std::runtime_error("chebyshev_apply: z overlaps r");
  if (dinv && ranges_overlap(z, dinv, M))
    throw std::runtime_error("chebyshev_apply: z overlaps dinv");
  spmv_hip_ctx* ctx = exec.context();
  const int len = dot_partials_len(ctx);

  ChebyshevWorkspace own(exec);
  ChebyshevWorkspace& w = workspace ? *workspace : own;
  const bool dinv_aligned = is_aligned16(dinv);
  w.ensure(M, N_padded, 0, len, false, !dinv_aligned);

  // everything on the executor's current stream, nothing waits
  const double* ri = r;
  if (!is_aligned16(r)) { // the streaming kernels load 16 bytes at a time
    exec.copy<double>(w.r, r, M);
    ri = w.r;
  }
  const double* di = dinv;
  if (dinv && !dinv_aligned) {
    exec.copy<double>(w.dinv, dinv, M);
    di = w.dinv;
  }
  if (N_padded > M)
    exec.memset<double>(w.z + M, 0, N_padded - M);
  throw_on_error(spmv_hip_cheb_apply0_f64(ctx, M, cb[0], ri, di,
                                          degree > 1 ? w.d : nullptr, w.z,
                                          nullptr),
                 "spmv_hip_cheb_apply0_f64");
  for (int j = 1; j < degree; ++j) {
    col_l2g->update(w.z);
    A.mult(w.z, w.w);
    throw_on_error(spmv_hip_cheb_step_f64(ctx, nullptr, M, ca[j], cb[j],
                                          j == degree - 1, w.w, ri, di, w.d, w.z,
                                          nullptr),
                   "spmv_hip_cheb_step_f64");
  }
  exec.copy<double>(z, w.z, M);
  if (!workspace) // its vectors go away with it
    exec.synchronize_stream(exec.get_stream());
}

int pcg_chebyshev(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
                  const double* b, double* x, const double* dinv, int degree,
                  double lmin, double lmax, int kmax, double rtol,
                  std::vector<double>* rnorm_history, const CgOptions* options,
                  CgStats* stats, ChebyshevWorkspace* workspace)
{
  double ca[kChebyshevMaxDegree], cb[kChebyshevMaxDegree];
  chebyshev_coefficients(degree, lmin, lmax, ca, cb);
  const Dims dims = check_problem("pcg_chebyshev", A, kmax);
  const CgOptions opt = options ? *options : CgOptions();
  using Solve = PcgSolve<ChebyshevWorkspace>;
  // steps 1 .. degree - 1 of z = M(r); the last one leaves the r.z partials
  auto cheb_steps = [&](Solve& s, bool timed) {
    ChebyshevWorkspace& w = s.w;
    for (int j = 1; j < degree; ++j) {
      s.col_l2g.update(w.z); // starts on the side stream
      if (timed)
        exec.record_event(w.timing_ev[s.ev_next], w.stream);
      A.mult(w.z, w.w);
      if (timed) {
        exec.record_event(w.timing_ev[s.ev_next + 1], w.stream);
        s.ev_next += 2;
      }
      throw_on_error(spmv_hip_cheb_step_f64(s.ctx, w.ws, s.M, ca[j], cb[j],
                                            j == degree - 1, w.w, w.r, s.di, w.d,
                                            w.z, nullptr),
                     "spmv_hip_cheb_step_f64");
    }
  };
  // degree 1: no d
  auto dvec = [&](Solve& s) { return degree > 1 ? s.w.d : nullptr; };
  return pcg_solve(
      "pcg_chebyshev", comm, exec, A, dims, b, x, dinv, kmax, rtol,
      rnorm_history, opt, stats, workspace, degree, {&ChebyshevWorkspace::z},
      // r = b, x0 = 0, partials of r.r, step 0 of M: one pass; then the rest
      // of z0 = M(r0) and p1 = z0
      [&](Solve& s) {
        throw_on_error(spmv_hip_cheb_init_f64(s.ctx, s.w.ws, s.M, cb[0], b, s.di,
                                              s.w.r, s.xi, dvec(s), s.w.z,
                                              nullptr),
                       "spmv_hip_cheb_init_f64");
        cheb_steps(s, false);
        exec.copy<double>(s.w.p, s.w.z, s.M);
      },
      [&](Solve& s, int k) {
        stored_z_iteration(s, k, [&] {
          throw_on_error(spmv_hip_cheb_update_r_f64(s.ctx, s.w.ws, k, s.M, cb[0],
                                                    s.w.Ap, s.di, s.w.r, dvec(s),
                                                    s.w.z, nullptr),
                         "spmv_hip_cheb_update_r_f64");
          cheb_steps(s, opt.time_spmv);
        });
      });
}

namespace
{
// the entry checks of both setup paths -> the local block
const CSRMatrix<double>* sgs_local_block(const Matrix<double>& A)
{
  std::shared_ptr<L2GMap> row_map = A.row_map();
  std::shared_ptr<const L2GMap> col_map = A.col_map();
  if (row_map->num_ghosts() > 0
      || row_map->local_size() != col_map->local_size()
      || row_map->global_offset() != col_map->global_offset())
    throw std::runtime_error(
        "spmv::SgsPreconditioner - Error: rows and owned columns are not the "
        "same index range on this rank");
  const auto* blk = dynamic_cast<const CSRMatrix<double>*>(A.local_block());
  if (!blk)
    throw std::runtime_error(
        "spmv::SgsPreconditioner - Error: the matrix has no local block");
  if (blk->csr_released())
    throw std::runtime_error(
        "spmv::SgsPreconditioner - Error: the CSR arrays of this matrix were "
        "released (release_csr); build the preconditioner before releasing "
        "them");
  return blk;
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now() - t0)
      .count();
}

[[noreturn]] void throw_fp32_range(int64_t bad)
{
  throw std::runtime_error(
      "spmv::SgsPreconditioner - Error: fp32 range: " + std::to_string(bad)
      + " off-diagonal value(s) round to Inf, zero or an fp32 subnormal "
        "(values = fp32)");
}

[[noreturn]] void throw_bad_diagonal(int64_t bad, int64_t n)
{
  // jacobi_inverse's rule and message
  throw std::runtime_error(
      "spmv::SgsPreconditioner - Error: the diagonal is not positive ("
      + std::to_string(bad) + " of " + std::to_string(n)
      + " entries are not finite or not > 0)");
}
} // namespace

SgsPreconditioner::SgsPreconditioner(HipExecutor& exec, const Matrix<double>& A)
    : _exec(exec)
{
  build_on_host(A, SgsValues::fp64);
}

SgsPreconditioner::SgsPreconditioner(HipExecutor& exec, const Matrix<double>& A,
                                     const SgsOptions& options)
    : _exec(exec)
{
  if (options.setup == SgsSetup::host) {
    if (options.colors || options.order != SgsOrder::hashed)
      throw std::invalid_argument(
          "spmv::SgsPreconditioner - Error: setup = host colours by itself: it "
          "takes neither colors nor an order");
    build_on_host(A, options.values);
    return;
  }
  try {
    build_on_device(A, options);
  } catch (...) { // (the destructor does not run)
    spmv_hip_mcgs_plan_destroy(_plan);
    throw;
  }
}

void SgsPreconditioner::build_on_device(const Matrix<double>& A,
                                        const SgsOptions& options)
{
  const auto t0 = std::chrono::steady_clock::now();
  const CSRMatrix<double>* blk = sgs_local_block(A);
  const int64_t n = A.row_map()->local_size();
  const int64_t nnz = blk->non_zeros();
  const bool symmetric = A.symmetric();
  if (n >= std::numeric_limits<int32_t>::max() || blk->cols() < n)
    throw std::runtime_error(
        "spmv::SgsPreconditioner - Error: rows and owned columns are not the "
        "same index range on this rank");
  spmv_hip_ctx* ctx = _exec.context();
  // an empty block owns no arrays
  const int32_t* rowptr = nnz > 0 ? blk->rowptr() : nullptr;
  const int32_t* colind = nnz > 0 ? blk->colind() : nullptr;
  const double* values = nnz > 0 ? blk->values() : nullptr;

  struct DeviceInts { // the colours, for the time of the setup
    HipExecutor& exec;
    int32_t* p = nullptr;
    ~DeviceInts()
    {
      if (p)
        exec.free(p);
    }
  } d_colors{_exec};
  if (n > 0)
    d_colors.p = _exec.alloc<int32_t>((size_t)n);
  int num_colors = 0;
  if (options.colors) {
    int32_t lo = 0, hi = -1;
    for (int64_t i = 0; i < n; ++i) {
      lo = std::min(lo, options.colors[i]);
      hi = std::max(hi, options.colors[i]);
    }
    if (lo < 0)
      throw std::runtime_error(
          "spmv::SgsPreconditioner - Error: a colour is negative");
    num_colors = hi + 1;
    if (n > 0)
      _exec.copy_from<int32_t>(d_colors.p, _exec.get_host(), options.colors,
                               (size_t)n);
  } else {
    throw_on_error(
        spmv_hip_mcgs_color(ctx, (int32_t)n, blk->cols(), nnz, rowptr, colind,
                            symmetric ? 1 : 0,
                            options.order == SgsOrder::natural
                                ? SPMV_HIP_MCGS_NATURAL
                                : SPMV_HIP_MCGS_HASHED,
                            d_colors.p, &num_colors, &_rounds, nullptr),
        "spmv_hip_mcgs_color");
  }
  _color_ms = ms_since(t0);

  int64_t info[SPMV_HIP_MCGS_INFO_WORDS] = {};
  int64_t out_of_range = 0;
  const int rc
      = options.values == SgsValues::fp64
            ? spmv_hip_mcgs_plan_build(
                ctx, (int32_t)n, blk->cols(), nnz, rowptr, colind, values,
                symmetric ? blk->diagonal() : nullptr, symmetric ? 1 : 0,
                d_colors.p, num_colors, kSgsLongThreshold, &_plan, info, nullptr)
            : spmv_hip_mcgs_plan_build_ex(
                ctx, (int32_t)n, blk->cols(), nnz, rowptr, colind, values,
                symmetric ? blk->diagonal() : nullptr, symmetric ? 1 : 0,
                d_colors.p, num_colors, kSgsLongThreshold, 32, &_plan, info,
                &out_of_range, nullptr);
  // (a diagonal that is not positive is the older rule: it speaks first)
  if (rc == SPMV_HIP_ERANGE && out_of_range != 0) {
    if (info[0] != 0)
      throw_bad_diagonal(info[0], n);
    throw_fp32_range(out_of_range);
  }
  if (rc == SPMV_HIP_EINVAL && info[1] == SPMV_HIP_MCGS_IMPROPER)
    throw std::runtime_error(
        "spmv::sgs_build - Error: the colouring is not proper (row "
        + std::to_string(info[3]) + ")");
  if (rc == SPMV_HIP_EINVAL && info[1] == SPMV_HIP_MCGS_UNWORN_COLOR)
    throw std::runtime_error(
        "spmv::SgsPreconditioner - Error: a colour below the largest is not "
        "worn by any row");
  if (rc == SPMV_HIP_EINVAL && info[1] == SPMV_HIP_MCGS_BAD_COLOR)
    throw std::runtime_error(
        "spmv::SgsPreconditioner - Error: a colour is out of range");
  throw_on_error(rc, "spmv_hip_mcgs_plan_build");
  if (info[0] != 0)
    throw_bad_diagonal(info[0], n);
  _num_colors = num_colors;
  _rows = (int)n;
  _value_bits = options.values == SgsValues::fp32 ? 32 : 64;
  _temp_bytes = info[2];
  _setup_ms = ms_since(t0);
  _build_ms = _setup_ms - _color_ms;
}

void SgsPreconditioner::build_on_host(const Matrix<double>& A, SgsValues width)
{
  const auto t0 = std::chrono::steady_clock::now();
  HipExecutor& exec = _exec;
  const CSRMatrix<double>* blk = sgs_local_block(A);
  std::shared_ptr<L2GMap> row_map = A.row_map();
  const int64_t n = row_map->local_size();
  const int64_t nnz = blk->non_zeros();
  const bool symmetric = A.symmetric();

  // the block, read back (the copies wait for the device)
  const DeviceExecutor& host = exec.get_host();
  std::vector<int32_t> rowptr((size_t)n + 1, 0), colind((size_t)nnz);
  std::vector<double> values((size_t)nnz), diagonal;
  if (nnz > 0) { // (an empty block owns no arrays)
    exec.copy_to<int32_t>(rowptr.data(), host, blk->rowptr(), (size_t)n + 1);
    exec.copy_to<int32_t>(colind.data(), host, blk->colind(), (size_t)nnz);
    exec.copy_to<double>(values.data(), host, blk->values(), (size_t)nnz);
  }
  if (symmetric && n > 0) {
    diagonal.resize((size_t)n);
    exec.copy_to<double>(diagonal.data(), host, blk->diagonal(), (size_t)n);
  }

  SgsHostPlan hp = sgs_build(rowptr.data(), colind.data(), values.data(),
                             symmetric ? diagonal.data() : nullptr, n, n,
                             symmetric);
  std::vector<int32_t>().swap(colind);
  std::vector<double>().swap(values);

  // jacobi_inverse's rule and message
  int64_t bad = 0;
  std::vector<double> dinv((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const double v = hp.d[(size_t)i];
    dinv[(size_t)i] = 1.0 / v;
    if (!(v > 0.0) || !std::isfinite(v))
      ++bad;
  }
  if (bad != 0)
    throw_bad_diagonal(bad, n);

  auto part_of = [](const SgsSlicedPart& s) {
    return spmv_hip_mcgs_part{s.color_slice.data(), s.slice_pos0.data(),
                              s.slice_ptr.data(),   s.len.data(),
                              s.col.data(),         s.val.data(),
                              s.color_long.data(),  s.long_pos.data(),
                              s.long_ptr.data(),    s.long_col.data(),
                              s.long_val.data()};
  };
  const SgsSlicedPart before = sgs_slice(hp, hp.before);
  hp.before = SgsCsrPart();
  const SgsSlicedPart after = sgs_slice(hp, hp.after);
  hp.after = SgsCsrPart();
  spmv_hip_mcgs_host in{};
  in.num_rows = hp.n;
  in.num_colors = hp.num_colors;
  in.perm = hp.perm.data();
  in.color_start = hp.color_start.data();
  in.dinv = dinv.data();
  in.before = part_of(before);
  in.after = part_of(after);
  if (width == SgsValues::fp64) {
    throw_on_error(spmv_hip_mcgs_plan_create(exec.context(), &in, &_plan),
                   "spmv_hip_mcgs_plan_create");
  } else {
    int64_t out_of_range = 0;
    const int rc = spmv_hip_mcgs_plan_create_ex(exec.context(), &in, 32, &_plan,
                                                &out_of_range);
    if (rc == SPMV_HIP_ERANGE && out_of_range != 0)
      throw_fp32_range(out_of_range);
    throw_on_error(rc, "spmv_hip_mcgs_plan_create_ex");
    _value_bits = 32;
  }
  _num_colors = hp.num_colors;
  _colors = std::move(hp.colors);
  _rows = hp.n;
  _setup_ms = ms_since(t0);
}

SgsPreconditioner::~SgsPreconditioner()
{
  try {
    if (_plan) // a sweep may still be in flight
      _exec.synchronize();
  } catch (...) {
  }
  if (_owns_plan)
    spmv_hip_mcgs_plan_destroy(_plan);
}

void SgsPreconditioner::adopt(spmv_hip_mcgs_plan* plan, int num_colors,
                              std::vector<int32_t> colors)
{
  _plan = plan;
  _num_colors = num_colors;
  _colors = std::move(colors);
  _rows = (int)_colors.size();
}

void SgsPreconditioner::adopt(spmv_hip_mcgs_plan* plan, int num_colors, int rows)
{
  _plan = plan;
  _num_colors = num_colors;
  _colors.clear();
  _rows = rows;
}

void SgsPreconditioner::set_setup_record(int rounds, double color_ms,
                                         double build_ms, int64_t temp_bytes)
{
  _rounds = rounds;
  _color_ms = color_ms;
  _build_ms = build_ms;
  _setup_ms = color_ms + build_ms;
  _temp_bytes = temp_bytes;
}

void SgsPreconditioner::colors(int32_t* out) const
{
  if (!out && _rows > 0)
    throw std::runtime_error("spmv::SgsPreconditioner::colors - Error: NULL output");
  if (_colors.empty() && _rows > 0) {
    // device setup: the colour of a row is the colour of its position
    std::vector<int32_t> perm((size_t)_rows), start((size_t)_num_colors + 1);
    throw_on_error(spmv_hip_mcgs_plan_export(_plan, perm.data(), start.data(),
                                             nullptr, nullptr, nullptr),
                   "spmv_hip_mcgs_plan_export");
    _colors.resize((size_t)_rows);
    for (int c = 0; c < _num_colors; ++c)
      for (int32_t pos = start[(size_t)c]; pos < start[(size_t)c + 1]; ++pos)
        _colors[(size_t)perm[(size_t)pos]] = c;
  }
  std::copy(_colors.begin(), _colors.end(), out);
}

int64_t SgsPreconditioner::plan_bytes() const
{
  int64_t bytes = 0;
  throw_on_error(spmv_hip_mcgs_plan_bytes(plan(), &bytes),
                 "spmv_hip_mcgs_plan_bytes");
  return bytes;
}

void sgs_apply(HipExecutor& exec, const SgsPreconditioner& M, const double* r,
               double* z)
{
  if (ranges_overlap(z, r, M.rows()))
    throw std::runtime_error("sgs_apply: z overlaps r");
  if (M.rows() > 0 && (!r || !z))
    throw std::runtime_error("sgs_apply: NULL vector");
  throw_on_error(spmv_hip_mcgs_apply_f64(exec.context(), M.plan(), nullptr, r, z,
                                         nullptr),
                 "spmv_hip_mcgs_apply_f64");
}

int pcg_sgs(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
            const SgsPreconditioner& Mpre, const double* b, double* x, int kmax,
            double rtol, std::vector<double>* rnorm_history,
            const CgOptions* options, CgStats* stats, SgsWorkspace* workspace)
{
  const Dims dims = check_problem("pcg_sgs", A, kmax);
  const CgOptions opt = options ? *options : CgOptions();
  if (Mpre.rows() != dims.M)
    throw std::runtime_error(
        "spmv::pcg_sgs - Error: the preconditioner was built for "
        + std::to_string(Mpre.rows()) + " rows, the matrix has "
        + std::to_string(dims.M));
  if (Mpre.negative_pivots() > 0)
    throw std::runtime_error(
        "spmv::pcg_sgs - Error: the preconditioner has "
        + std::to_string(Mpre.negative_pivots())
        + " negative pivot(s): it is not positive definite");
  using Solve = PcgSolve<SgsWorkspace>;
  // z = M^-1 r and the partials of r.z
  auto precondition = [&](Solve& s) {
    throw_on_error(spmv_hip_mcgs_apply_f64(s.ctx, Mpre.plan(), s.w.ws, s.w.r,
                                           s.w.z, nullptr),
                   "spmv_hip_mcgs_apply_f64");
    throw_on_error(spmv_hip_sgs_dot_rz_f64(s.ctx, s.w.ws, s.M, s.w.r, s.w.z,
                                           nullptr),
                   "spmv_hip_sgs_dot_rz_f64");
  };
  return pcg_solve(
      "pcg_sgs", comm, exec, A, dims, b, x, nullptr, kmax, rtol, rnorm_history,
      opt, stats, workspace, 1, {},
      // r = b, x0 = 0, partials of r.r: one pass; then z0 = M^-1 r0 and p1 = z0
      [&](Solve& s) {
        throw_on_error(spmv_hip_sgs_init_f64(s.ctx, s.w.ws, s.M, b, s.w.r, s.xi,
                                             nullptr),
                       "spmv_hip_sgs_init_f64");
        precondition(s);
        exec.copy<double>(s.w.p, s.w.z, s.M);
      },
      [&](Solve& s, int k) {
        stored_z_iteration(s, k, [&] {
          throw_on_error(spmv_hip_sgs_update_r_f64(s.ctx, s.w.ws, k, s.M, s.w.Ap,
                                                   s.w.r, nullptr),
                         "spmv_hip_sgs_update_r_f64");
          precondition(s);
        });
      });
}

int pcg_amg(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
            const AmgPreconditioner& Mpre, const double* b, double* x, int kmax,
            double rtol, std::vector<double>* rnorm_history,
            const CgOptions* options, CgStats* stats, AmgPcgWorkspace* workspace)
{
  const Dims dims = check_problem("pcg_amg", A, kmax);
  const CgOptions opt = options ? *options : CgOptions();
  if (Mpre.rows() != dims.M)
    throw std::runtime_error(
        "spmv::pcg_amg - Error: the preconditioner was built for "
        + std::to_string(Mpre.rows()) + " rows, the matrix has "
        + std::to_string(dims.M));
  using Solve = PcgSolve<SgsWorkspace>;
  // z = M^-1 r (the cycle runs on the object's own scratch, also after `done`)
  // and the partials of r.z
  auto precondition = [&](Solve& s) {
    amg_apply(exec, Mpre, s.w.r, s.w.z);
    throw_on_error(spmv_hip_sgs_dot_rz_f64(s.ctx, s.w.ws, s.M, s.w.r, s.w.z,
                                           nullptr),
                   "spmv_hip_sgs_dot_rz_f64");
  };
  return pcg_solve(
      "pcg_amg", comm, exec, A, dims, b, x, nullptr, kmax, rtol, rnorm_history,
      opt, stats, workspace, 1, {},
      [&](Solve& s) {
        throw_on_error(spmv_hip_sgs_init_f64(s.ctx, s.w.ws, s.M, b, s.w.r, s.xi,
                                             nullptr),
                       "spmv_hip_sgs_init_f64");
        precondition(s);
        exec.copy<double>(s.w.p, s.w.z, s.M);
      },
      [&](Solve& s, int k) {
        stored_z_iteration(s, k, [&] {
          throw_on_error(spmv_hip_sgs_update_r_f64(s.ctx, s.w.ws, k, s.M, s.w.Ap,
                                                   s.w.r, nullptr),
                         "spmv_hip_sgs_update_r_f64");
          precondition(s);
        });
      });
}

double lambda_max_estimate(const Comm& comm, HipExecutor& exec,
                           const Matrix<double>& A, const double* dinv,
                           const double* v0, int steps)
{
  if (steps < 1)
    throw std::runtime_error("spmv::lambda_max_estimate - Error: steps < 1");
  const Dims dims = check_problem("lambda_max_estimate", A, 0);
  const int64_t M = dims.M, N_padded = dims.N_padded;
  const std::shared_ptr<const L2GMap>& col_l2g = dims.col_l2g;
  spmv_hip_ctx* ctx = exec.context();
  const int len = dot_partials_len(ctx);

  // q, u: local; v: padded (the SpMV reads it); 3 scalars; one partial array
  // (everything is allocated before the first reduction)
  struct Buffers {
    HipExecutor& exec;
    double *q = nullptr, *u = nullptr, *v = nullptr, *s = nullptr,
           *partials = nullptr;
    ~Buffers()
    {
      try {
        exec.synchronize_stream(exec.get_stream());
        for (double* ptr : {q, u, v, s, partials})
          exec.free(ptr);
      } catch (...) {
      }
    }
  } m{exec};
  m.q = exec.alloc<double>(M);
  m.u = exec.alloc<double>(M);
  m.v = exec.alloc<double>(N_padded);
  m.s = exec.alloc<double>(3);
  m.partials = exec.alloc<double>(len);
  if (N_padded > M)
    exec.memset<double>(m.v + M, 0, N_padded - M);

  void* st = exec.get_stream();
  // s[i] = the global dot product of the i-th pair; ONE host wait for all
  auto dots = [&](std::initializer_list<std::pair<const double*, const double*>>
                      pairs,
                  double* out) {
    int i = 0;
    for (const auto& pr : pairs) {
      throw_on_error(spmv_hip_dot_partial_f64(ctx, M, pr.first, pr.second,
                                              m.partials, nullptr),
                     "spmv_hip_dot_partial_f64");
      throw_on_error(spmv_hip_reduce_partials_f64(ctx, m.partials, m.s + i,
                                                  nullptr),
                     "spmv_hip_reduce_partials_f64");
      ++i;
    }
    comm.reduce_sum(m.s, pairs.size(), st);
    exec.copy_to<double>(out, exec.get_host(), m.s, pairs.size()); // waits
  };
  auto scale = [&](double s, const double* dv, const double* in, double* out) {
    throw_on_error(spmv_hip_cheb_scale_f64(ctx, M, s, dv, in, out, nullptr),
                   "spmv_hip_cheb_scale_f64");
  };

  double h[3] = {0.0, 0.0, 0.0};
  dots({{v0, v0}}, h);
  if (!(h[0] > 0.0) || !std::isfinite(h[0]))
    throw std::runtime_error(
        "spmv::lambda_max_estimate - Error: v0 . v0 is not a positive number");
  scale(std::sqrt(h[0]), nullptr, v0, m.q); // q = v0 / ||v0||
  double lambda = 0.0;
  for (int it = 0; it < steps; ++it) {
    scale(1.0, dinv, m.q, m.v); // v = dinv*q
    col_l2g->update(m.v);
    A.mult(m.v, m.u); // u = A v
    dots({{m.v, m.u}, {m.v, m.q}, {m.u, m.u}}, h);
    lambda = h[0] / h[1];
    if (!(h[2] > 0.0) || !std::isfinite(h[2]))
      throw std::runtime_error(
          "spmv::lambda_max_estimate - Error: the iteration broke down "
          "(||A v|| is not a positive number)");
    scale(std::sqrt(h[2]), nullptr, m.u, m.q); // q = u / ||u||
  }
  return lambda;
}

} // namespace spmv
