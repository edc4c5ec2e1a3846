// Conjugate Gradient on the MI355X backend, mirroring the reference's
// per-executor overload set of spmv::cg (spmv/cg.h, spmv/cuda/cg_cuda.h:30-32).
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <initializer_list>
#include <memory>
#include <vector>

#include "comm.h"
#include "executor.h"
#include "matrix.h"
#include "solver_args.h"

struct spmv_hip_cg_ws;
struct spmv_hip_cgb_ws;
struct spmv_hip_pcg_ws;
struct spmv_hip_pcgb_ws;
struct spmv_hip_bicg_ws;
struct spmv_hip_gmres_ws;
struct spmv_hip_minres_ws;
struct spmv_hip_lsqr_ws;
struct spmv_hip_lobpcg_ws;
struct spmv_hip_cgs_ws;
struct spmv_hip_idrs_ws;
struct spmv_hip_mcgs_plan;
struct spmv_hip_ilu0_plan;
struct spmv_hip_amg_tail;
struct spmv_hip_amg_plan;

namespace spmv
{

// What the workspaces of all solvers share: the solve's stream, the event and
// the pinned words of the host's lagging look at the device's state, the
// timing events, and how the work vectors of one capacity are regrown.
class SolverWorkspace
{
public:
  SolverWorkspace(const SolverWorkspace&) = delete;
  SolverWorkspace& operator=(const SolverWorkspace&) = delete;

  HipExecutor& _exec;
  int32_t* flags = nullptr; // pinned: the device's state words, [0] = done
  void* stream = nullptr;   // compute stream of the solve
  void* poll_event = nullptr;
  std::vector<void*> timing_ev; // CgOptions::time_spmv: 2 events per SpMV

  // events for CgOptions::time_spmv of a solve with up to `spmvs` timed SpMVs
  // (one per iteration; pcg_chebyshev: iterations * degree), created ahead of
  // it (a benchmark keeps them out of its timed region)
  void reserve_timing(int spmvs)
  {
    reserve_events(2 * (size_t)std::max(spmvs, 0));
  }

protected:
  explicit SolverWorkspace(HipExecutor& exec) : _exec(exec) {}
  ~SolverWorkspace() = default;
  // first use: creates the stream and the poll event, allocates the pinned words
  void open(int flag_words);
  // want > cap: frees the vectors of one capacity, then allocates them at the
  // new one; the capacity is -1 and the pointers are null while they are gone
  void regrow(int64_t& cap, int64_t want, std::initializer_list<double**> vecs);
  // timing_ev grows to n events
  void reserve_events(size_t n);
  // waits for the stream, then destroys the events and the stream and frees
  // the pinned words; what a release() calls first
  void release_common();
  // frees and nulls every vector (errors are swallowed: a release() never throws)
  void free_vectors(std::initializer_list<double**> vecs);
};

// Work vectors + device scalars of one solve (cg.cpp:39-42 allocates and
// frees them on every call).  Passing the same CgWorkspace to repeated cg()
// calls keeps the allocations; it regrows itself when a call needs more.
class CgWorkspace : public SolverWorkspace
{
public:
  explicit CgWorkspace(HipExecutor& exec) : SolverWorkspace(exec) {}
  ~CgWorkspace();

  // ---- internal to cg() ----
  void ensure(int64_t M, int64_t N_padded, int kmax, int partials_len);
  // the second p buffer of CgOptions::defer_x, allocated by the first solve
  // that takes that path (after ensure())
  void ensure_p2();
  void release();

  spmv_hip_cg_ws* ws = nullptr;
  int kmax_cap = -1;
  int64_t m_cap = -1, n_cap = -1;
  double *r = nullptr, *Ap = nullptr, *x = nullptr, *p = nullptr;
  double* p2 = nullptr;     // CgOptions::defer_x: the second p buffer (n_cap)
  double* dot2 = nullptr;   // partials of the remote block's p.Ap share
  // flags: {done, kstop}; timing_ev: 2 events per iteration
};

struct CgOptions {
  int poll_every = 16;    // host looks at the device's `done` flag this often
  bool time_spmv = false; // bracket every local-block SpMV with HIP events
  // One rank only (no all-reduce between producer and consumer): the update
  // kernels add the dot-product partials themselves, in the reducers' order,
  // so an iteration is 3 launches and the scalars keep their bits.  With more
  // than one rank (or when switched off) every dot product is finished by a
  // single-workgroup reducer kernel (5 launches per iteration).
  bool consumer_reductions = true;
  // With consumer_reductions on one rank (fp64, every vector 16-byte aligned):
  // nothing inside an iteration reads x, so its update is deferred by one
  // iteration and two of them are applied in one pass, in their order and
  // with their roundings (same bits).  p alternates between two buffers; the
  // x/p side of a pair of iterations takes 9 vector passes instead of 10, for
  // one more work vector (8 bytes per row).  Elsewhere it has no effect.
  bool defer_x = true;
  // Mixed precision: the SpMV of every iteration streams an
  // fp32 copy of the matrix values (half the matrix bytes; x, p, r and all
  // arithmetic stay fp64).  Every `replace_every` iterations the recurrence
  // residual is replaced by the true one, r = b - A x, computed with the fp64
  // values (residual replacement keeps the single Krylov sequence); when the
  // loop ends the true residual is checked once more and, if it misses rtol,
  // the correction equation A d = r is solved with the fp64 values and added
  // (CgStats reports both).  General storage only; ignored for symmetric.
  bool mixed = false;
  int replace_every = 50;
};

struct CgStats {
  int spmv_launches = 0;    // local-block SpMV kernels timed
  double spmv_ms_total = 0; // sum of their durations (HIP events, same stream)
  // CgOptions::mixed
  int replacements = 0;             // residual replacements inside the loop
  double true_rel_residual = -1.0;  // ||b - A x|| / ||r_0|| with fp64 values,
                                    // at the end of the mixed loop
  int continuation_iterations = 0;  // fp64 iterations of the correction solve
  double final_true_rel_residual = -1.0; // ... after it (= the above if none)
};

// Unpreconditioned CG from x0 = 0 (spmv/cg.cpp:21-98).  `b` and `x` are
// DEVICE pointers of A.row_map()->local_size() doubles (cuda/cg.cuda.cu:70).
// Stops when k == kmax or ||r_k|| / ||r_0|| < rtol; returns k.
//
// All scalars (alpha, beta, the residual history) stay on the device; the
// host enqueues iterations without waiting and only looks at a pinned flag
// every `poll_every` iterations to stop enqueuing once the device has
// declared convergence.  Kernels issued after convergence are no-ops, so x
// is exactly the iterate of the returned k.
//
// `x` IS the iterate (cg.cpp keeps a padded work vector and copies it out at
// the end, :89): it is zeroed at the start of the solve and updated in place
// from iteration 1 on, so
//   * `x` must not overlap `b` (std::runtime_error; the reference would
//     tolerate x == b because it writes x only once, after the loop), and
//   * if the solve throws, `x` holds whatever iterate had been reached --
//     unlike the reference it is not left untouched.
// (An `x` that is not 16-byte aligned, and every mixed-precision solve, go
// through the workspace's own vector and one copy at the end instead.)
//
// If rnorm_history != nullptr it receives ||r_0||, ..., ||r_k||.
int cg(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
       const double* b, double* x, int kmax, double rtol,
       std::vector<double>* rnorm_history = nullptr,
       const CgOptions* options = nullptr, CgStats* stats = nullptr,
       CgWorkspace* workspace = nullptr);

// Work vectors + device scalars of cg_block(), kept across calls like
// CgWorkspace; it regrows itself when a call needs more rows, more iterations
// or another nrhs.
class CgBlockWorkspace : public SolverWorkspace
{
public:
  explicit CgBlockWorkspace(HipExecutor& exec) : SolverWorkspace(exec) {}
  ~CgBlockWorkspace();

  // ---- internal to cg_block() ----
  // m_elems = rows * nrhs, n_elems = (local + ghosts) * nrhs; need_x: the
  // caller's X is not 16-byte aligned, the iterate lives in `x`
  void ensure(int64_t m_elems, int64_t n_elems, int kmax, int nrhs,
              bool need_x);
  void release();

  spmv_hip_cgb_ws* ws = nullptr;
  int kmax_cap = -1, nrhs_cap = 0;
  int64_t m_cap = -1, n_cap = -1, x_cap = -1;
  double *r = nullptr, *Ap = nullptr; // m_cap
  double* x = nullptr; // x_cap: the iterate when the caller's X is unaligned
  double* p = nullptr; // n_cap: padded, the ghost tail is zeroed by every solve
  // flags: {all_done, done[], kstop[]} (spmv_hip.h); timing_ev: 2 events per
  // iteration
};

// CG for several right-hand sides: solves A X = B for `nrhs` columns with
// nrhs INDEPENDENT unpreconditioned CG recurrences from X0 = 0 (cg.cpp:21-98
// once per column) that run in lockstep -- one halo exchange of the block, one
// Matrix::mult_block and one all-reduce of nrhs doubles per reduction.  This
// is not block-Krylov CG: no information passes between columns, and the bits
// of column c (x, residual history, iteration count) depend on A, on column c
// of B, on nrhs and on c only.
//
// Layout of Matrix::mult_block: element (i, c) at B[i * nrhs + c] and
// X[i * nrhs + c]; both DEVICE pointers of A.row_map()->local_size() * nrhs
// doubles.  1 <= nrhs <= 8 (std::runtime_error otherwise).  As with cg(), X is
// the iterate and must not overlap B (std::runtime_error); an X that is not
// 16-byte aligned goes through the workspace's copy and one copy at the end.
//
// Every column has its own alpha, beta and stopping test ||r_k|| / ||r_0|| <
// rtol.  The iteration in which a column meets the tolerance updates its x
// and r and leaves its p (cg.cpp:80-81); from then on the column is frozen.
// The solve ends when every column has stopped or at k == kmax; the value
// returned is the largest per-column iteration count.
//
// Unlike cg(), which runs a system with r_0 . r_0 == 0 to kmax on NaNs, a
// column with r_0 . r_0 == 0 is declared stopped at k = 0 with x = 0: a
// caller may pad a block with zero columns.
//
// iterations    (optional) nrhs entries: the k of every column.
// rnorm_history (optional) nrhs * (kmax + 1) entries: ||r_j|| of column c at
//               [c * (kmax + 1) + j] for j <= iterations[c], -1.0 beyond.
// options       poll_every and time_spmv apply (time_spmv brackets the
//               local-block mult_block launch); consumer_reductions, defer_x
//               and mixed are IGNORED: every dot product is finished by a
//               reducer kernel, x is updated in every iteration, in fp64.
int cg_block(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
             const double* B, double* X, int nrhs, int kmax, double rtol,
             std::vector<int>* iterations = nullptr,
             std::vector<double>* rnorm_history = nullptr,
             const CgOptions* options = nullptr, CgStats* stats = nullptr,
             CgBlockWorkspace* workspace = nullptr);

// What the workspaces of pcg(), pcg_chebyshev() and pcg_sgs() share: the device
// scalars (spmv_hip_pcg_ws) and the vectors every one of them has.  A derived
// class adds its own vectors and their capacities.
class PcgFamilyWorkspace : public SolverWorkspace
{
public:
  spmv_hip_pcg_ws* ws = nullptr;
  int kmax_cap = -1;
  int64_t m_cap = -1, n_cap = -1, x_cap = -1;
  double *r = nullptr, *Ap = nullptr; // m_cap
  double* x = nullptr;    // x_cap: the iterate when the caller's x is unaligned
  double* p = nullptr;    // n_cap: padded, the ghost tail is zeroed by every solve
  double* dot2 = nullptr; // partials of the remote block's p.Ap share
  // flags: {done, kstop}; timing_ev: 2 events per timed SpMV

protected:
  explicit PcgFamilyWorkspace(HipExecutor& exec) : SolverWorkspace(exec) {}
  ~PcgFamilyWorkspace() = default;
  // The head of every ensure(): the stream and flags, dot2, the scalars for
  // kmax iterations, the vectors of M doubles (`m_vecs`: r, Ap and the class's
  // own) and, if need_x, x.  The class's ensure() goes on with its dinv copy
  // and the padded vectors (n_cap); the order of the allocations is kept.
  void ensure_common(int64_t M, int kmax, int partials_len, bool need_x,
                     std::initializer_list<double**> m_vecs);
  // everything above, then the class's own vectors
  void release_family(std::initializer_list<double**> own_vecs);
};

// Work vectors + device scalars of pcg(), kept across calls like CgWorkspace;
// it regrows itself when a call needs more rows or more iterations.
class PcgWorkspace : public PcgFamilyWorkspace
{
public:
  explicit PcgWorkspace(HipExecutor& exec) : PcgFamilyWorkspace(exec) {}
  ~PcgWorkspace();

  // ---- internal to pcg() ----
  // need_x / need_dinv: the caller's x / dinv is not 16-byte aligned and lives
  // in the workspace's copy during the solve
  void ensure(int64_t M, int64_t N_padded, int kmax, int partials_len,
              bool need_x, bool need_dinv);
  void release();

  int64_t dinv_cap = -1;
  double* dinv = nullptr; // dinv_cap: the copy of an unaligned dinv
};

// dinv[i] = 1.0 / d[i] (spmv_hip_jacobi_invert_f64); `d` and `dinv` DEVICE
// pointers of n doubles (they may be the same vector).  Reads the device's
// count of entries that are not finite or not > 0 ONCE -- the only host wait of
// the preconditioner's setup, outside any solve -- and throws
// std::runtime_error("... diagonal is not positive ...") when it is nonzero
// (dinv then holds the quotients all the same).
void jacobi_inverse(HipExecutor& exec, const double* d, double* dinv, int64_t n);

// CG with a diagonal preconditioner from x0 = 0.  `dinv` is any positive
// DEVICE vector of A.row_map()->local_size() doubles, the inverse of the
// preconditioner's diagonal: Jacobi's comes from Matrix::diagonal and
// jacobi_inverse, the solver does not care.  With `.` the global dot product:
//
//   r0 = b; p1 = dinv*r0 (elementwise); rz0 = r0.(dinv*r0); rr0 = r0.r0
//   for k = 1..kmax:
//     Ap    = A p_k                  (halo update of p first, as in cg())
//     alpha = rz[k-1] / (p_k . Ap)
//     x    += alpha * p_k
//     r    -= alpha * Ap
//     rz[k] = r.(dinv*r); rr[k] = r.r
//     if sqrt(rr[k]) / sqrt(rr[0]) < rtol: stop (x and r updated, p not)
//     beta  = rz[k] / rz[k-1]
//     p_(k+1) = beta * p_k + dinv*r
//
// Products and sums are separate roundings.  z = dinv*r is never stored: the
// two update kernels recompute it, dinv is read twice per iteration.  The
// stopping test is cg()'s, on the unpreconditioned 2-norm, so the histories of
// the two solvers compare; rnorm_history receives ||r_0||, ..., ||r_k||.  A
// system with r_0 . r_0 == 0 stops at k = 0 with x = 0 (the rule of cg_block,
// not cg()'s run to kmax on NaNs).  Returns k.
//
// As in cg(): scalars stay on the device, reductions are two-stage and
// deterministic, convergence is decided on the device and the host only looks
// at a pinned flag every `poll_every` iterations; `x` IS the iterate and must
// not overlap `b` or `dinv` (std::runtime_error, "overlaps"); an `x` (or a
// `dinv`) that is not 16-byte aligned goes through the workspace's copy, x
// with one copy at the end; kmax < 0 throws; the executor's stream is
// restored on every exit path.
//
// options: poll_every, time_spmv and consumer_reductions apply (one rank with
//          consumer_reductions: 3 launches per iteration, else 5); defer_x and
//          mixed are IGNORED: x is updated in every iteration, in fp64.
int pcg(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
        const double* b, double* x, const double* dinv, int kmax, double rtol,
        std::vector<double>* rnorm_history = nullptr,
        const CgOptions* options = nullptr, CgStats* stats = nullptr,
        PcgWorkspace* workspace = nullptr);

// ---- Chebyshev polynomial preconditioner ------------------------------------
// The coefficients of the `degree`-step Chebyshev iteration on the interval
// [lmin, lmax] (host, plain C++, fp64, in exactly this order; the factors 2 and
// 0.5 are exact):
//
//   theta = 0.5*(lmax+lmin); delta = 0.5*(lmax-lmin); sigma = theta/delta
//   rho_0 = 1/sigma;  a_0 = 0;  b_0 = 1/theta
//   j = 1..degree-1:  rho_j = 1/(2*sigma - rho_{j-1});  a_j = rho_j*rho_{j-1}
//                     b_j = 2*rho_j/delta
//
// a[] and b[] take `degree` entries each.  1 <= degree <= 16 ("degree"); lmin
// and lmax finite with 0 < lmin < lmax ("bounds"): std::runtime_error otherwise.
// (kChebyshevMaxDegree = 16: solver_args.h, whose declaration this repeats)
void chebyshev_coefficients(int degree, double lmin, double lmax, double* a,
                            double* b);

// Work vectors + device scalars of pcg_chebyshev() and chebyshev_apply(), kept
// across calls like PcgWorkspace; it regrows itself when a call needs more rows
// or more iterations.  The device scalars and their reducers are pcg()'s.
class ChebyshevWorkspace : public PcgFamilyWorkspace
{
public:
  explicit ChebyshevWorkspace(HipExecutor& exec) : PcgFamilyWorkspace(exec) {}
  ~ChebyshevWorkspace();

  // ---- internal to pcg_chebyshev() / chebyshev_apply() ----
  // need_x / need_dinv: the caller's x / dinv is not 16-byte aligned and lives
  // in the workspace's copy (chebyshev_apply: an unaligned r goes through `r`,
  // z always through the padded `z`)
  void ensure(int64_t M, int64_t N_padded, int kmax, int partials_len,
              bool need_x, bool need_dinv);
  void release();

  int64_t dinv_cap = -1;
  double *d = nullptr, *w = nullptr; // m_cap
  // n_cap: padded like p, what the SpMVs of M read; its ghost tail is zeroed by
  // every call
  double* z = nullptr;
  double* dinv = nullptr; // dinv_cap: the copy of an unaligned dinv
};

// z = q(dinv*A) dinv r: the preconditioner as an operation of its own (it also
// serves as a smoother), the `degree`-step Chebyshev iteration for A z = r from
// z = 0 with the coefficients above:
//
//   j = 0:   d = b_0 * (dinv*r);                    z = d
//   j >= 1:  w = A z  (halo update of z, then Matrix::mult)
//            d = a_j*d + b_j*(dinv*(r - w));        z = z + d
//
// Elementwise; every product and sum is a rounding of its own, so the result
// is the same bits as the restatement on Matrix::mult.  `r`, `z`: DEVICE
// vectors of A.row_map()->local_size() doubles, any alignment, not overlapping
// ("overlaps"); `dinv` as in pcg(), or nullptr (no multiply, no dinv stream).
// Step j >= 1 is one streaming kernel (w, r, dinv, d, z in; d, z out; the last
// step does not write d).  Only Matrix::mult is used: every plan form, both
// storages and every halo model serve.  Runs on the executor's current stream;
// nothing is read back from the device, and with a workspace the host does not
// wait (without one the call waits before its own work vectors go away).
void chebyshev_apply(HipExecutor& exec, const Matrix<double>& A,
                     const double* r, double* z, const double* dinv, int degree,
                     double lmin, double lmax,
                     ChebyshevWorkspace* workspace = nullptr);

// CG with the Chebyshev polynomial preconditioner M(r) = chebyshev_apply(r)
// from x0 = 0: pcg()'s recurrence with a STORED z = M(r).
//
//   r0 = b; z0 = M(r0); p1 = z0; rz[0] = r0.z0; rr[0] = r0.r0
//   for k = 1..kmax:
//     Ap    = A p_k (fused p.Ap where the SpMV can); alpha = rz[k-1] / (p_k.Ap)
//     r    -= alpha * Ap; rr[k] = r.r; z = M(r); rz[k] = r.z
//     x    += alpha * p_k
//     if sqrt(rr[k]) / sqrt(rr[0]) < rtol: stop (x and r updated, p not)
//     beta  = rz[k] / rz[k-1]; p_(k+1) = beta * p_k + z
//
// The kernel that updates r also leaves the partials of r.r and runs step 0 of
// M; the last step of M leaves the partials of r.z (degree 1: one kernel does
// both); one kernel updates x, applies the stop test and updates p.  An
// iteration is `degree` SpMVs + degree + 1 streaming launches + 2 reducer
// launches; beside the SpMVs 7*(degree - 1) + 11 vector passes with a dinv
// (degree 1: 10, no d is written), one per step less without.  With several
// ranks: one all-reduce of 1 double (p.Ap) and ONE of 2 doubles ({rz[k],
// rr[k]}, installed together after the last step).
//
// dinv: as in pcg(), or nullptr.  degree, lmin, lmax: see
// chebyshev_coefficients; they are checked before anything touches a device.
// The bounds are those of the spectrum of dinv*A.  Advised: lmax = 1.1 *
// lambda_max_estimate(20 steps), lmin = lmax / 30.  Degree 1 is Jacobi-PCG up
// to the factor b_0.
//
// As in pcg(): the stopping test is cg()'s; rnorm_history receives ||r_0||,
// ..., ||r_k||; a system with r_0 . r_0 == 0 stops at k = 0 with x = 0; scalars
// stay on the device, the stop is decided on the device and every kernel after
// `done` returns at once, so x is exactly the iterate of the returned k; the
// host only polls a pinned flag every `poll_every` iterations; `x` IS the
// iterate and must not overlap `b` or `dinv` (std::runtime_error, "overlaps");
// an `x` (or a `dinv`) that is not 16-byte aligned goes through the
// workspace's copy; kmax < 0 throws ("kmax"); the executor's stream is
// restored on every exit path.
//
// options: poll_every and time_spmv apply (time_spmv brackets ALL `degree`
//          Matrix::mult calls of an iteration, each between two events:
//          CgStats::spmv_launches is `degree` per iteration, the local-block
//          kernel for A p as in pcg()); consumer_reductions,
//          defer_x and mixed are IGNORED: every dot product is finished by a
//          reducer kernel, as in cg_block, x is updated in every iteration, in
//          fp64.
int pcg_chebyshev(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
                  const double* b, double* x, const double* dinv, int degree,
                  double lmin, double lmax, int kmax, double rtol,
                  std::vector<double>* rnorm_history = nullptr,
                  const CgOptions* options = nullptr, CgStats* stats = nullptr,
                  ChebyshevWorkspace* workspace = nullptr);

// An estimate of the largest eigenvalue of dinv*A (A itself with dinv ==
// nullptr): `steps` steps of the power iteration with the generalised Rayleigh
// quotient.  Setup code; the host waits once per step.
//
//   q = v0 / ||v0||
//   repeat `steps` times:  v = dinv*q;  u = A v;  lambda = (v.u) / (v.q)
//                          q = u / ||u||
//
// Returns the last lambda (the same on every rank).  `v0`: a DEVICE vector of
// A.row_map()->local_size() doubles (the right-hand side will do), not
// modified.  The dot products go through the deterministic partial sums of
// cg() and the communicator's all-reduce.  steps < 1 ("steps") or v0.v0 == 0
// ("v0") throws std::runtime_error.  The estimate approaches the eigenvalue
// from below (0.96 to 0.975 of it after 20 steps on the Poisson test matrices),
// hence the advised lmax = 1.1 * estimate(20 steps), lmin = lmax / 30.
double lambda_max_estimate(const Comm& comm, HipExecutor& exec,
                           const Matrix<double>& A, const double* dinv,
                           const double* v0, int steps);

// ---- Multicolour symmetric Gauss-Seidel preconditioner ------------------------
// M = (D + L) D^-1 (D + U) on the LOCAL DIAGONAL BLOCK of A -- the rows of this
// rank and the columns < local_size; ghost columns and the remote block are
// ignored, so on several ranks the preconditioner is block-Jacobi over the ranks
// with SGS inside each, and an application needs no halo exchange -- with the
// rows in colour-major order:
//
//   colouring  greedy in natural row order over the pattern of B + B^T, B the
//              block without its diagonal (symmetric storage: the stored
//              strictly lower block): colour(i) = the smallest colour not worn
//              by an already coloured neighbour.  Deterministic; the 7-point
//              Poisson matrix gets two colours, the parity of x + y + z.
//   rows       colour-major, natural order within a colour
//   before(i)  the off-diagonal entries of row i whose column's colour is
//              smaller than colour(i); after(i): larger.  Each ascending by
//              column, duplicates of a column in storage order.  Symmetric
//              storage: a row's entries are its stored lower entries and the
//              entries of its column in the stored block (a stable transpose).
//   d_i        what Matrix::diagonal defines; dinv_i = 1.0 / d_i
//
//   forward,  colours 0 .. C-1:  s = 0.0; for e in before(i): s = s + a_e * z[col_e]
//                                z_i = (r_i - s) * dinv_i
//   backward, colours C-2 .. 0:  t = 0.0; for e in after(i):  t = t + a_e * z[col_e]
//                                z_i = z_i - dinv_i * t
//
// Every product and sum is a rounding of its own.  Inside a colour the rows are
// independent: one launch per colour and direction (2C - 1 per application),
// ordered by the stream alone.
//
// The constructor is the setup and the one place that waits on the device: it
// reads the block back, colours and reorders it on the host
// (host/sgs_build.h) and uploads the plan's own copy (slices of 64 rows stored
// column-major, one lane per row; rows with more than 64 entries in a part take
// a wavefront each).  A may release_csr() AFTERWARDS; on a matrix that has
// released its CSR arrays the constructor throws, for both storages (the lower
// block's arrays are gone).  Rows and owned columns must be the same index
// range on the rank, as for Matrix::diagonal (std::runtime_error).  A diagonal
// entry that is not finite or not > 0 throws with jacobi_inverse's message
// ("... diagonal is not positive ...").
//
// SgsOptions chooses where that setup runs.  setup = host (the default, and the
// two-argument constructor) is the path above.  setup = device reads nothing of
// the matrix back: the block is coloured where it lies (spmv_hip_mcgs_color:
// greedy first-fit in a priority order, Jones-Plassmann rounds) and the plan is
// built from the device arrays (spmv_hip_mcgs_plan_build: every array equal to
// what the host builder makes from the same colours); only counters and the
// tables of num_colors + 1 entries cross to the host.  order = hashed (the
// default) colours in a pseudo-random order -- a handful of rounds, but more
// colours than the host's greedy (7-point Poisson: 6 against 2, so 11 launches
// per application against 3, and another iteration count); order = natural is
// the host's colouring entry for entry, in as many rounds as the longest
// ascending path of the pattern (about 3 n for Poisson n^3): slow on long
// dependency chains.  colors (host, rows entries, 0-based, every colour up to
// the largest worn, proper on B + B^T) replaces the colouring; it is checked
// on the device ("the colouring is not proper", "colour").  The entry checks
// and messages are the same on both paths.  setup = host with colors, or with
// an order other than the default, throws std::invalid_argument: the host
// builder colours by itself.
//
// values = fp32 (with every setup, order and colors) keeps the off-diagonal
// values of the sweep plan -- the a_e above, both parts, long rows included --
// as float, each the fp64 value rounded to nearest-even: a sweep streams 8
// bytes per stored entry, not 12, and plan_bytes() drops by 4 bytes per stored
// entry (padding included).  dinv, r, z, the sums and every operation stay
// fp64: s = s + (double)a32_e * z[col_e], so sgs_apply has the bits of the fp64
// sweeps on the widened values, and M is still a fixed SPD operator -- equal
// values round to equal floats -- that pcg_sgs, pcg_block, gmres, minres, idrs
// and lobpcg take under the same rules; the Krylov method converges to fp64
// accuracy on A all the same.  A matrix whose values are exact in fp32
// (Poisson: 6 and -1) gives the bits of the fp64 object.  A finite non-zero
// value whose rounding is +-Inf, zero or an fp32 subnormal is refused
// (std::runtime_error, "fp32 range"): the plan must not depend on a denormal
// mode.  The values are counted on the device while they are rounded; the
// constructor waits once more for the count.  values = fp64 (the default) is
// the object as it ever was, on the code path it ever took.
enum class SgsSetup { host, device };
enum class SgsOrder { hashed, natural };
enum class SgsValues { fp64, fp32 };
struct SgsOptions {
  SgsSetup setup = SgsSetup::host;
  SgsOrder order = SgsOrder::hashed;
  const int32_t* colors = nullptr;
  SgsValues values = SgsValues::fp64;
};

class SgsPreconditioner
{
public:
  SgsPreconditioner(HipExecutor& exec, const Matrix<double>& A);
  SgsPreconditioner(HipExecutor& exec, const Matrix<double>& A,
                    const SgsOptions& options);
  virtual ~SgsPreconditioner();
  SgsPreconditioner(const SgsPreconditioner&) = delete;
  SgsPreconditioner& operator=(const SgsPreconditioner&) = delete;

  int rows() const { return _rows; }
  int num_colors() const { return _num_colors; }
  // host copy, rows() entries (setup = device: fetched from the plan on the
  // first call)
  void colors(int32_t* out) const;
  // rounds of the device colouring (0: host setup, or colours of the caller's)
  int rounds() const { return _rounds; }
  // wall time of the constructor; of which colouring and plan (device setup)
  double setup_ms() const { return _setup_ms; }
  double color_ms() const { return _color_ms; }
  double build_ms() const { return _build_ms; }
  // peak device memory of the device setup's temporaries (0: host setup)
  int64_t setup_temp_bytes() const { return _temp_bytes; }
  virtual int64_t plan_bytes() const; // device memory of the plan
  // 64 or 32: the width of the sweep plan's off-diagonal values
  int value_bits() const { return _value_bits; }
  // the plan the sweeps run on (a derived class may refuse: check_usable)
  spmv_hip_mcgs_plan* plan() const
  {
    check_usable();
    return _plan;
  }
  // pivots of the factor that are negative: 0 here, Ilu0Preconditioner counts
  virtual int64_t negative_pivots() const { return 0; }

protected:
  // An object whose plan the derived class builds, owns and adopts (adopt());
  // this class then neither creates nor destroys one.
  explicit SgsPreconditioner(HipExecutor& exec) : _exec(exec), _owns_plan(false) {}
  void adopt(spmv_hip_mcgs_plan* plan, int num_colors,
             std::vector<int32_t> colors);
  // ... of a plan built on the device: colors() fetches them when asked
  void adopt(spmv_hip_mcgs_plan* plan, int num_colors, int rows);
  // what rounds(), color_ms(), build_ms() (setup_ms() their sum) and
  // setup_temp_bytes() answer for a derived class's device setup
  void set_setup_record(int rounds, double color_ms, double build_ms,
                        int64_t temp_bytes);
  // called by plan(): throws when the plan must not be used now
  virtual void check_usable() const {}

  HipExecutor& _exec;
  spmv_hip_mcgs_plan* _plan = nullptr;
  bool _owns_plan = true;
  int _num_colors = 0;
  int _rows = 0;
  int _value_bits = 64;
  mutable std::vector<int32_t> _colors; // (device setup: empty until asked for)

private:
  void build_on_host(const Matrix<double>& A, SgsValues width);
  void build_on_device(const Matrix<double>& A, const SgsOptions& options);
  int _rounds = 0;
  double _setup_ms = 0, _color_ms = 0, _build_ms = 0;
  int64_t _temp_bytes = 0;
};

// ---- Multicolour ILU(0), factored on the device ---------------------------------
// M = (D~ + L~) D~^-1 (D~ + U~) on the local diagonal block (as above: block-
// Jacobi over the ranks, no halo exchange), the incomplete LU factorisation
// without fill in the colour-major ordering; for a symmetric matrix the same
// factor is IC(0) in the form L D L^T.  Colouring, positions and d_i are
// SgsPreconditioner's; pos(j) is the position of row j.
//
//   before(i)  the off-diagonal entries of row i whose column's colour is
//              smaller than colour(i); after(i): larger.  Each ascending by
//              pos(column) -- NOT by column: the elimination needs position
//              order, and the sweeps of this plan add in it.  A column that
//              occurs twice in one row of the block is refused
//              (std::runtime_error, "duplicate").
//   factor     rows in position order (rows of one colour never read each other):
//                w = copy of row i (before, diagonal, after)
//                for k in before(i), ascending pos(k):
//                  m = w[k] * dinv~[k]
//                  for (j, u) in after~(k), in its order:
//                    if j == i or j is in the pattern of row i:
//                      w[j] = w[j] - m * u
//                l~(i, .) = w on before(i); u~(i, .) = w on after(i)
//                d~_i = w[i]; dinv~_i = 1.0 / d~_i
//              Every product, difference and quotient is one rounding; fill
//              outside the pattern is dropped.
//   apply      sgs_apply's two sweeps with l~, u~ and dinv~: sgs_apply, pcg_sgs
//              and GmresPreconditioner::sgs take the object as it is.
//
// The constructor reads the block's PATTERN back and does the symbolic work on
// the host (host/ilu0_build.h); the numbers never leave the device: a gather
// from the matrix's values, one launch per colour 1 .. C-1 (a wavefront per
// row), a scatter into the sweep plan (spmv_ilu0.hip).  refactor(A) repeats
// only that, for a matrix with the SAME pattern and storage whose values have
// changed (time stepping, Newton; Matrix::plan_values_changed does the same for
// the SpMV plans' copies): no read-back, no host pass.  The one wait of
// a factorisation is the read of two counts:
//   pivots d~ that are not finite or zero: the call throws ("pivot"); after a
//     failed refactor the object is not usable (plan() throws "pivot") until a
//     later refactor succeeds;
//   pivots that are finite and negative: negative_pivots().  pcg_sgs refuses
//     such a preconditioner ("pivot"): it is not positive definite; gmres takes
//     it.
// The constructor and refactor throw on a matrix that has released its CSR
// arrays ("released"); release_csr() afterwards is fine until the next
// refactor.  refactor checks rows, storage and the number of stored entries;
// that the pattern is the same is the caller's promise.
//
// SgsOptions (above) chooses where the symbolic half runs.  setup = host (the
// default, and the two-argument constructor) is the path above; with colors or
// an order it throws std::invalid_argument.  setup = device reads nothing of
// the matrix back: spmv_hip_mcgs_color colours the block (hashed or natural) or
// the caller's colors are taken, and spmv_hip_ilu0_plan_build makes every array
// of the plan from the CSR arrays where they lie, equal to what the host makes
// from the same colours (order = natural: the host-built object, bit for bit
// in factor(), sgs_apply, pcg_sgs and gmres).  A duplicate column, an improper
// colouring and the block rules are refused with the host path's words
// ("duplicate", "not proper", "same index range", "released"); a diagonal that
// is not positive is left to the factorisation's pivot counts on both paths.
// colors() and pattern() fetch the colours from the plan on their first call.
// rounds(), color_ms(), build_ms() and setup_temp_bytes() describe the device
// setup; symbolic_ms() is the wall time of colouring and build together.
//
// values = fp32: the factorisation stays fp64 -- the working copy, factor(),
// pattern() and the pivot counts do not change --; l~ and u~ are rounded to
// float as they are scattered into the sweep plan, dinv~ stays fp64, and
// refactor rounds again.  The factor of a symmetric matrix stays symmetric
// (equal values round to equal floats).  A factor entry out of fp32's range
// throws "fp32 range" from the constructor and from refactor, counted at the
// wait of the pivot counts; after such a refactor the object is not usable
// (plan() throws "fp32 range") until a later refactor succeeds.
class Ilu0Preconditioner : public SgsPreconditioner
{
public:
  Ilu0Preconditioner(HipExecutor& exec, const Matrix<double>& A);
  Ilu0Preconditioner(HipExecutor& exec, const Matrix<double>& A,
                     const SgsOptions& options);
  ~Ilu0Preconditioner() override;
  // the device plan, for copies of its part arrays (spmv_hip_ilu0_plan_export)
  const spmv_hip_ilu0_plan* ilu_plan() const { return _ilu; }

  void refactor(const Matrix<double>& A);
  int64_t negative_pivots() const override { return _negative; }
  // the sweep plan, the working copy of the factor, the maps, the diagonal
  int64_t plan_bytes() const override;

  // host copies (they wait for the device).  The parts are CSR over positions
  // (row perm[pos], colour-major, natural order within a colour); a NULL
  // output is skipped.
  int64_t before_entries() const { return _nbefore; }
  int64_t after_entries() const { return _nafter; }
  // ptr: rows() + 1 entries; col: the entries' columns (rows' numbers)
  void pattern(int64_t* before_ptr, int32_t* before_col, int64_t* after_ptr,
               int32_t* after_col) const;
  // l~ and u~ in the order of pattern(), d~ by POSITION
  void factor(double* l, double* u, double* d) const;

  // wall time of the constructor's two halves, for measurements
  double symbolic_ms() const { return _symbolic_ms; }
  double numeric_ms() const { return _numeric_ms; }

protected:
  // throws ("pivot") while the last factorisation left no usable factor
  void check_usable() const override;

private:
  void construct(const Matrix<double>& A, const SgsOptions& options);
  void symbolic_on_host(const CSRMatrix<double>* blk, int64_t n,
                        SgsValues values);
  void symbolic_on_device(const CSRMatrix<double>* blk, int64_t n,
                          const SgsOptions& options,
                          std::chrono::steady_clock::time_point t0);
  void numeric(const Matrix<double>& A);
  bool _usable = true;
  bool _out_of_range = false; // why not: the last factor left fp32's range

  spmv_hip_ilu0_plan* _ilu = nullptr;
  double* _diag = nullptr; // general storage: Matrix::diagonal's output
  int64_t _nbefore = 0, _nafter = 0, _num_values = 0, _negative = 0;
  bool _symmetric = false;
  double _symbolic_ms = 0, _numeric_ms = 0;
};


// z = M^-1 r.  `r`, `z`: DEVICE vectors of rows() doubles, any alignment, not
// overlapping ("overlaps").  Runs on the executor's current stream; the host
// does not wait.
void sgs_apply(HipExecutor& exec, const SgsPreconditioner& M, const double* r,
               double* z);
inline void ilu0_apply(HipExecutor& exec, const Ilu0Preconditioner& M,
                       const double* r, double* z)
{
  sgs_apply(exec, M, r, z);
}

// Work vectors + device scalars of pcg_sgs(), kept across calls like
// ChebyshevWorkspace; the device scalars and their reducers are pcg()'s.
class SgsWorkspace : public PcgFamilyWorkspace
{
public:
  explicit SgsWorkspace(HipExecutor& exec) : PcgFamilyWorkspace(exec) {}
  ~SgsWorkspace();

  // ---- internal to pcg_sgs() ----
  void ensure(int64_t M, int64_t N_padded, int kmax, int partials_len,
              bool need_x);
  void release();

  double* z = nullptr; // m_cap
};

// CG with the preconditioner M from x0 = 0: pcg_chebyshev()'s recurrence with
// the stored z = sgs_apply(r).
//
//   r0 = b; z0 = M^-1 r0; p1 = z0; rz[0] = r0.z0; rr[0] = r0.r0
//   for k = 1..kmax:
//     Ap    = A p_k (fused p.Ap where the SpMV can); alpha = rz[k-1] / (p_k.Ap)
//     r    -= alpha * Ap; rr[k] = r.r; z = M^-1 r; rz[k] = r.z
//     x    += alpha * p_k
//     if sqrt(rr[k]) / sqrt(rr[0]) < rtol: stop (x and r updated, p not)
//     beta  = rz[k] / rz[k-1]; p_(k+1) = beta * p_k + z
//
// An iteration is one SpMV, the 2C - 1 sweeps, 3 streaming launches (r and the
// partials of r.r; the partials of r.z; x, the stop test and p) and 2 reducer
// launches; beside the SpMV and the sweeps 3 + 2 + 5 = 10 vector passes.  With
// several ranks: one all-reduce of 1 double (p.Ap) and ONE of 2 doubles
// ({rz[k], rr[k]}).  M must have been built from A (or from a matrix with A's
// rows on this rank): M.rows() != A's rows throws.  M may be an
// Ilu0Preconditioner (IC(0) in the form L D L^T for a symmetric A): the same
// sweeps on its factor; one with negative_pivots() > 0 is not positive definite
// and is refused (std::runtime_error, "pivot").
//
// As in pcg_chebyshev(): the stopping test is cg()'s; rnorm_history receives
// ||r_0||, ..., ||r_k||; a system with r_0 . r_0 == 0 stops at k = 0 with x = 0;
// scalars stay on the device, the stop is decided on the device and every
// kernel after `done` returns at once, so x is exactly the iterate of the
// returned k; the host only polls a pinned flag every `poll_every` iterations;
// `x` IS the iterate and must not overlap `b` (std::runtime_error,
// "overlaps"); an `x` that is not 16-byte aligned goes through the workspace's
// copy; kmax < 0 throws ("kmax"); the executor's stream is restored on every
// exit path.
//
// options: poll_every and time_spmv apply (time_spmv brackets the ONE
//          Matrix::mult of an iteration: CgStats::spmv_launches is 1 per
//          iteration); consumer_reductions, defer_x and mixed are IGNORED, as in
//          pcg_chebyshev.
int pcg_sgs(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
            const SgsPreconditioner& M, const double* b, double* x, int kmax,
            double rtol, std::vector<double>* rnorm_history = nullptr,
            const CgOptions* options = nullptr, CgStats* stats = nullptr,
            SgsWorkspace* workspace = nullptr);

// ---- Preconditioned CG for several right-hand sides -----------------------------
// Z = M^-1 R for nrhs INTERLEAVED vectors, the layout of Matrix::mult_block:
// element (i, c) at R[i * nrhs + c] and Z[i * nrhs + c], DEVICE blocks of
// M.rows() * nrhs doubles, 1 <= nrhs <= 8 ("nrhs"), any alignment, not
// overlapping ("overlaps").  M is an SgsPreconditioner or an
// Ilu0Preconditioner as it is: the sweeps read the plan sgs_apply reads, once
// for all columns.  Column c of Z has the bits of sgs_apply on column c.  Runs
// on the executor's current stream; the host does not wait.
void sgs_apply_block(HipExecutor& exec, const SgsPreconditioner& M,
                     const double* R, double* Z, int nrhs);

class AmgPreconditioner;

// The preconditioner of pcg_block(): exactly one of the three is set.
struct BlockPreconditioner {
  // a positive DEVICE vector of rows doubles (any alignment), shared by all
  // columns: z(i, c) = dinv[i] * r(i, c)
  const double* dinv = nullptr;
  // Z = sgs_apply_block(*sgs, R): an SgsPreconditioner or an Ilu0Preconditioner
  const SgsPreconditioner* sgs = nullptr;
  // Z = amg_apply_block(*amg, R): one V-cycle per column (see below)
  const AmgPreconditioner* amg = nullptr;
};

// Work vectors + device scalars of pcg_block(), kept across calls like
// CgBlockWorkspace; it regrows itself when a call needs more rows, more
// iterations or another nrhs.
class PcgBlockWorkspace : public SolverWorkspace
{
public:
  explicit PcgBlockWorkspace(HipExecutor& exec) : SolverWorkspace(exec) {}
  ~PcgBlockWorkspace();

  // ---- internal to pcg_block() ----
  void ensure(int64_t m_elems, int64_t n_elems, int kmax, int nrhs,
              bool need_x);
  void release();

  spmv_hip_pcgb_ws* ws = nullptr;
  int kmax_cap = -1, nrhs_cap = 0;
  int64_t m_cap = -1, n_cap = -1, x_cap = -1;
  double *r = nullptr, *Ap = nullptr, *z = nullptr; // m_cap
  double* x = nullptr; // x_cap: the iterate when the caller's X is unaligned
  double* p = nullptr; // n_cap: padded, the ghost tail is zeroed by every solve
  // flags: {all_done, done[], kstop[]} (spmv_hip.h); timing_ev: 2 events per
  // iteration
  // nrhs == 1 with an AmgPreconditioner: the solve IS pcg_amg, on this
  // workspace of its own (made on first use, released with the rest)
  std::unique_ptr<SgsWorkspace> single;
};

// Preconditioned CG for several right-hand sides: pcg_sgs()'s recurrence with
// a stored Z = M^-1 R, once per column of A X = B and in lockstep the way
// cg_block() runs cg() -- one halo exchange of the block P, one
// Matrix::mult_block, one application of M to the block and two all-reduces
// (nrhs doubles: p.Ap; 2 nrhs doubles: {rz, rr}) per iteration.
//
//   R = B; Z = M^-1 R; P = Z; rz[0][c] = r_c.z_c; rr[0][c] = r_c.r_c
//   for k = 1..kmax, per column c that has not stopped:
//     AP = A P;  alpha_c = rz[k-1][c] / (p_c.Ap_c)
//     r_c -= alpha_c Ap_c;  rr[k][c] = r_c.r_c;  Z = M^-1 R;  rz[k][c] = r_c.z_c
//     x_c += alpha_c p_c
//     if sqrt(rr[k][c]) / sqrt(rr[0][c]) < rtol: column c stops (p_c not updated)
//     beta_c = rz[k][c] / rz[k-1][c];  p_c = beta_c p_c + z_c
//
// Layout, nrhs (1..8), X as the iterate, the 16-byte rule for X, iterations,
// rnorm_history (nrhs * (kmax + 1) entries, -1.0 beyond a column's k) and the
// value returned are cg_block()'s, and so are its column rules: own alpha,
// beta, stop and count per column; a stopped column's x, r and p are frozen; a
// column with r_0 . r_0 == 0 stops at k = 0 with x = 0; the bits of column c
// depend on A, M, column c of B, nrhs and c, not on the other columns or on
// when they stop.  With several ranks M is block-Jacobi over the ranks, as for
// pcg_sgs().
//
// With M.dinv, Z = dinv * R is formed by the kernel that leaves the r.z
// partials; with M.sgs the 2C - 1 block sweeps run instead (they may go on
// writing a stopped column's Z: nothing reads it); with M.amg one
// amg_apply_block into Z, then the same r.z launch (the cycle runs on the
// object's own scratch and goes on for a stopped column: nothing reads it).
// Per iteration beside the mult_block: 3 streaming launches and 2 reducers (+
// the sweeps or the cycle).  With several ranks the cycle is block-Jacobi over
// the ranks, no halo exchange, as for pcg_amg().  A block of ONE column with
// M.amg is pcg_amg() itself (as amg_apply_block with nrhs == 1 is amg_apply):
// after the argument rules the call is handed to it, on a workspace kept inside
// the PcgBlockWorkspace, so k, the history and x have pcg_amg's bits; the
// history is laid out as for any block (kmax + 1 entries, -1.0 beyond k).
//
// The arguments are checked before anything touches a device
// (pcg_block_check_rules of solver_args.h; std::runtime_error): "nrhs", "kmax",
// "preconditioner" (not exactly one of dinv, sgs and amg), "rows" (sgs->rows()
// or amg->rows(0)), "pivot" (an Ilu0Preconditioner with negative_pivots() > 0),
// "overlaps" (X with B or dinv).  An AmgPreconditioner whose last refresh
// failed throws as amg_apply does.  The executor's stream is restored on every
// exit path.
// options: poll_every and time_spmv apply (one timed mult_block per
// iteration); consumer_reductions, defer_x and mixed are IGNORED, as in
// cg_block().
int pcg_block(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
              const double* B, double* X, int nrhs, const BlockPreconditioner& M,
              int kmax, double rtol, std::vector<int>* iterations = nullptr,
              std::vector<double>* rnorm_history = nullptr,
              const CgOptions* options = nullptr, CgStats* stats = nullptr,
              PcgBlockWorkspace* workspace = nullptr);

// ---- Aggregation multigrid preconditioner ---------------------------------------
// Every rule is checked before anything touches a device; std::runtime_error
// names the field (amg_check_options of solver_args.h).
struct AmgOptions {
  double theta = 0.25;          // strength threshold, in [0, 1]
  int max_levels = 10;          // 1..16
  int64_t min_coarse_rows = 200; // >= 1: a level with more rows is coarsened
  int smooth_degree = 2;        // 1..kChebyshevMaxDegree, pre and post
  int coarse_degree = 8;        // 1..kChebyshevMaxDegree, the coarsest level
  double eig_ratio = 4.0;       // > 1: lmin = lmax / eig_ratio
  double coarse_scale = 1.0;    // 1 <= coarse_scale < 2
  // Where the symbolic setup runs (see "Setup" below).  An order with setup =
  // host throws std::invalid_argument, as SgsOptions does.
  SgsSetup setup = SgsSetup::host;
  SgsOrder order = SgsOrder::hashed; // device only
};
constexpr int kAmgMaxLevels = 16;

// M^-1 = one V-cycle of plain (unsmoothed) aggregation multigrid on the LOCAL
// DIAGONAL BLOCK of A: SgsPreconditioner's scope -- the rows of this rank and
// the columns < local_size, ghost columns and the remote block ignored,
// block-Jacobi over the ranks, no halo exchange; rows and owned columns the
// same index range (std::runtime_error otherwise); fp64; both storages.
//
// Hierarchy.  The expanded row of a level: general storage, the row's stored
// entries with a column < local_size in storage order; symmetric storage (level
// 0 only, coarse levels are general), the stored lower entries, the diagonal
// entry, then the mirror images of the stored entries of its column ascending by
// row.  Per level l:
//   A_l      level 0: A's own local block, NOT copied (A must outlive this
//            object or be replaced by refresh()); its products are the block's
//            mult on a vector whose ghost tail is zero
//   d_i      Matrix::diagonal's definition; dinv_i = 1.0 / d_i; a d_i that is
//            not finite and > 0 throws ("diagonal is not positive")
//   g_i      (|a_e0| + |a_e1| + ...) * dinv_i over the expanded row in its order
//   lmax_l   max_i g_i, the row-sum bound of dinv*A: a true upper bound, so the
//            smoother converges and M is positive definite without a power
//            iteration; lmin_l = lmax_l / eig_ratio.  A g_i that is NaN takes no
//            part in the maximum (a NaN never replaces a number).  An lmax_l
//            that is not finite and > 0 -- a subnormal d_i has dinv_i = Inf,
//            a row of huge entries overflows its sum -- throws ("the row-sum
//            bound is not finite")
//   aggregates, P^T A_l P: host/amg_build.h; the coarse values are summed on
//            the device from per-entry source lists, left to right
// A level is coarsened while rows_l > min_coarse_rows and levels < max_levels;
// an aggregation that merges nothing is discarded (a diagonal matrix has one
// level).  Context options apply to the coarse blocks as to any block; a
// context that releases CSR arrays ("release_csr") is refused ("released").
//
// Cycle, z = M^-1 r, with a_j, b_j = chebyshev_coefficients(degree, lmin_l,
// lmax_l) and s = smooth_degree:
//   coarsest level:  z = the coarse_degree-step Chebyshev iteration from z = 0
//   otherwise:  pre   z = the s-step Chebyshev iteration from z = 0
//               w = A_l z; rc[I] = (t_0 + t_1) + ... over the members of I
//                 ascending, t_m = r[i_m] - w[i_m]
//               e = cycle(l + 1, rc);  z[i] = z[i] + coarse_scale * e[agg(i)]
//               post  j = 0:      w = A_l z; d = b_0*(dinv*(r - w));         z = z + d
//                     j = 1..s-1: w = A_l z; d = a_j*d + b_j*(dinv*(r - w)); z = z + d
// Every product, sum, difference and quotient is a rounding of its own.  With a
// symmetric A the operator is symmetric, and positive definite for 1 <=
// coarse_scale < 2.
//
// The constructor is the setup and, with refresh(), the one place that waits
// on the device.  It throws on a matrix that has released its CSR arrays
// ("released").  refresh(A): new values on the same pattern and storage (rows,
// storage and the number of stored entries are checked; the pattern is the
// caller's promise): aggregates, patterns and source lists are kept, the
// Galerkin sums, d, dinv and the bounds are recomputed on the device, no host
// pass; the only waits are the reads of the counts and bounds.  After a failed
// refresh the object is unusable until a later one succeeds.
//
// The level work vectors belong to the object: an application is NOT
// reentrant -- one amg_apply / pcg_amg / gmres at a time per object.
//
// Setup.  setup = host (the default): the constructor reads every level's
// matrix back and runs host/amg_build.h single-threaded.  setup = device: the
// aggregates (spmv_hip_amg_aggregate) and every list of a step
// (spmv_hip_amg_plan_build) are made on the device from the arrays where they
// lie; nothing of any level's matrix crosses to the host, only counts (n_agg,
// the coarse entries, rounds) and the words of the diagonal check and the
// bound.  The three passes are amg_build.h's with "i ascending" read as "i in
// descending priority": order = natural, prio(i) = rows - i, gives the host's
// hierarchy entry for entry, bit for bit, but needs as many rounds as the
// longest dependency chain (slow on a lattice in row order); order = hashed
// (the default of the device setup), mcgs_color's hash, decides a lattice in a
// few dozen rounds and gives OTHER aggregates.
// refresh(), the cycle, the tail and the solvers take the object unchanged;
// no host copy of agg is kept, aggregates() fetches it on its first call.
//
// The tail.  The levels below the finest are small, and an application spends
// most of its time launching their kernels.  set_tail_rows(max_rows) names the
// longest suffix t .. levels()-1, t >= 1, in which every level has rows(l) <=
// max_rows (amg_tail_first_level); apply() then runs levels 0 .. t-1 as before,
// the restrict from level t-1 included, everything that touches the levels >= t
// in ONE launch of one workgroup (spmv_hip_amg_tail_run_f64), and goes on with
// the prolong into level t-1: (levels()-1-t)(4s+3) + 2c-1 launches become one.
// The bits do not change: the same element arithmetic, and every level's product
// in the order of its plan, as the plan reports it when set_tail_rows builds
// the tail (a coarse block's plan does not change afterwards).  Level 0 is
// never part of it; a hierarchy of one level has none.  0 (the default) = no
// tail, the launches of the plain cycle.  A negative value throws ("tail_rows",
// amg_check_tail_rows of solver_args.h) before anything touches a device.  It
// may be called between applications, not while one is in flight; it waits for
// the device.  refresh() keeps the setting and rewrites the tail's coefficients
// before it returns.  Advice (one MI355X): 8192 -- levels
// of about 3 000 rows gain (Poisson 64^3: an application 0.90 -> 0.41 ms), a
// level of 21 000 to 32 000 rows in one workgroup loses several-fold.
class AmgPreconditioner
{
public:
  AmgPreconditioner(HipExecutor& exec, const Matrix<double>& A,
                    const AmgOptions& options = AmgOptions());
  ~AmgPreconditioner();
  AmgPreconditioner(const AmgPreconditioner&) = delete;
  AmgPreconditioner& operator=(const AmgPreconditioner&) = delete;

  void refresh(const Matrix<double>& A);

  int rows() const { return rows(0); }
  int levels() const;
  int rows(int level) const;
  int64_t non_zeros(int level) const; // stored entries of the level's block
  double lmax(int level) const;
  // the aggregate of every row of `level` (rows(level) entries; the last level
  // has none: throws)
  void aggregates(int level, int32_t* out) const;
  // a host copy of the operator of level >= 1 (it waits); NULL outputs skipped
  void level_matrix(int level, int32_t* rowptr, int32_t* colind,
                    double* values) const;
  int64_t plan_bytes() const; // device memory beyond A: levels, lists, vectors
  double symbolic_ms() const { return _symbolic_ms; }
  double numeric_ms() const { return _numeric_ms; }
  // The device setup's record; setup = host: 0.  rounds: of pass 1 (pass = 0),
  // of pass 3 (pass = 1) or of both (pass < 0) of the step from `level`; 0 for
  // the last level.  aggregate_ms + build_ms is the part of symbolic_ms spent in
  // the two device builders; setup_temp_bytes the peak of their temporaries.
  int rounds(int level, int pass = -1) const;
  double aggregate_ms() const { return _aggregate_ms; }
  double build_ms() const { return _build_ms; }
  int64_t setup_temp_bytes() const { return _setup_temp_bytes; }
  // the device plan of the step from `level` (or of the expanded rows of
  // symmetric storage), for spmv_hip_amg_plan_sizes / _export; may be NULL
  const spmv_hip_amg_plan* step_plan(int level) const;
  const AmgOptions& options() const { return _opt; }

  void set_tail_rows(int64_t max_rows);
  int tail_levels() const; // 0: no tail
  // lanes per row of the product of `level` inside the tail (0 = one lane per
  // row, left to right), as its plan reported them; -1: not a level of the tail.
  // For tests: it lets a case assert WHICH order ran, nothing else needs it.
  int tail_lanes(int level) const;

  // z = M^-1 r (amg_apply)
  void apply(const double* r, double* z) const;
  // Z = M^-1 R for nrhs interleaved vectors (amg_apply_block)
  void apply_block(const double* R, double* Z, int nrhs) const;
  // frees the block scratch of apply_block (it waits for the device); the next
  // block application allocates it again.  A no-op when there is none.
  void release_block_scratch();

private:
  struct Level;
  void ensure_block_scratch(int nrhs) const;
  void free_block_scratch() const;
  void numeric(const Matrix<double>& A, bool build);
  struct Clock;
  void levels_on_host(Clock& clock);
  void levels_on_device(Clock& clock);
  void add_coarse_level(Level& L, int32_t nc, int64_t nnz_c, int32_t* c_rowptr,
                        int32_t* c_colind);
  int32_t step_on_device(Level& L, bool sym, bool coarsen, int32_t** c_rowptr,
                         int32_t** c_colind, int64_t* c_nnz);
  void level_numbers(Level& L);
  void check_usable() const;
  void release();
  void drop_tail();
  void build_tail();

  HipExecutor& _exec;
  AmgOptions _opt;
  std::vector<std::unique_ptr<Level>> _levels;
  uint64_t* _stat = nullptr;
  spmv_hip_amg_tail* _tail = nullptr;
  int _tail_first = 0;
  int64_t _tail_rows = 0;
  std::vector<int> _tail_lanes;
  bool _symmetric = false, _usable = false;
  int64_t _num_values = 0;
  double _symbolic_ms = 0, _numeric_ms = 0, _aggregate_ms = 0, _build_ms = 0;
  int64_t _setup_temp_bytes = 0;
  // apply_block: the width the levels' block vectors hold (0: none), the width
  // of the last application (the ghost tail of level 0's z is zeroed for it),
  // and the columns of level 0's per-column product (see amg_apply_block)
  mutable int _block_cap = 0, _block_last = 0;
  mutable double* _block_cols = nullptr;
  mutable int64_t _block_cols_elems = 0;
};

// z = M^-1 r.  `r`, `z`: DEVICE vectors of rows() doubles, any alignment, not
// overlapping ("overlaps").  Runs on the executor's current stream; the host
// does not wait.  Not reentrant (see above).
void amg_apply(HipExecutor& exec, const AmgPreconditioner& M, const double* r,
               double* z);

// Z = M^-1 R for nrhs INTERLEAVED vectors, the layout of Matrix::mult_block:
// element (i, c) at R[i * nrhs + c] and Z[i * nrhs + c], DEVICE blocks of
// M.rows(0) * nrhs doubles, 1 <= nrhs <= 8 ("nrhs"), any alignment, Z not
// overlapping R ("overlaps").  Runs on the executor's current stream; the host
// does not wait; R is unchanged.  Not reentrant per object, like amg_apply; an
// object whose last refresh failed throws as amg_apply does.
//
// Column c of Z has the bits of amg_apply on column c of R -- for every nrhs,
// every alignment, both storages and every AmgOptions, whatever the other
// columns hold (NaN and Inf included): column c depends on M, column c of R,
// nrhs and c alone.  nrhs == 1 IS amg_apply.
//
// The cycle is amg_apply's with every vector a block: the block kernels of
// hip/spmv_amg_block.hip (the element arithmetic of hip/amg_elem.h, shared
// with the single-vector kernels; dinv, the aggregates and the member lists
// read once for all columns) and one CSRMatrix::mult_block per product, which
// streams the level's matrix once for all columns.  mult_block's columns have
// mult's bits for every plan form but one: a level whose plan reports algo ==
// SPMV_HIP_ALGO_VECTOR adds a row in the sub-wavefront kernel's pairwise order,
// the native multi-vector kernel left to right.  Such a level takes the plan's
// own single-vector launch per column instead: the object's coarse blocks get
// the plan key "mv_native" = 0 at the first block application (mult_block then
// de-interleaves by itself; mult is not affected); level 0 is the CALLER'S
// matrix, no key of its plan is ever changed: its block is de-interleaved here
// (spmv_hip_deinterleave_f64), multiplied column by column and interleaved back.
//
// The fused tail (set_tail_rows) is a single-vector kernel and is NOT used by
// the block path: the block cycle runs those levels with the block kernels,
// launch by launch.  The tail has the bits of the separate launches, so the
// criterion above holds with a tail set, and tail_levels() does not change.  A
// block tail kernel does not exist.
//
// Scratch.  Per level r, w, dd of rows * nrhs and z of cols * nrhs doubles
// (ghost tail zero); d and dinv are shared with amg_apply.  Allocated by the
// first block application, regrown (it waits for the device) for a larger
// nrhs, reused for a smaller one, freed with the object or by
// release_block_scratch(); counted in plan_bytes() while it exists.  An R that
// is not 16-byte aligned is copied into level 0's block r first.
void amg_apply_block(HipExecutor& exec, const AmgPreconditioner& M,
                     const double* R, double* Z, int nrhs);

// pcg_amg's workspace: the vectors and device scalars of pcg_sgs
using AmgPcgWorkspace = SgsWorkspace;

// CG with M = one AMG V-cycle from x0 = 0: pcg_sgs()'s recurrence and frame
// with z = amg_apply(r).  pcg_sgs's contract holds word for word: the stop
// test, the zero right-hand side, an unaligned x, "overlaps", "kmax", the
// stream restored on every exit, and which options apply (poll_every,
// time_spmv: ONE timed Matrix::mult per iteration).  After `done` the cycle may
// still run on its own scratch; x, the history and k do not change.
// M.rows() != A's rows throws.
int pcg_amg(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
            const AmgPreconditioner& M, const double* b, double* x, int kmax,
            double rtol, std::vector<double>* rnorm_history = nullptr,
            const CgOptions* options = nullptr, CgStats* stats = nullptr,
            AmgPcgWorkspace* workspace = nullptr);

// Work vectors + device scalars of bicgstab(), kept across calls like
// PcgWorkspace; it regrows itself when a call needs more rows or more
// iterations.
class BicgstabWorkspace : public SolverWorkspace
{
public:
  explicit BicgstabWorkspace(HipExecutor& exec) : SolverWorkspace(exec) {}
  ~BicgstabWorkspace();

  // ---- internal to bicgstab() ----
  // need_x / need_dinv: the caller's x / dinv is not 16-byte aligned and lives
  // in the workspace's copy during the solve; need_h: a dinv was given, ph and
  // sh are vectors of their own
  void ensure(int64_t M, int64_t N_padded, int kmax, bool need_x, bool need_dinv,
              bool need_h);
  void reserve_timing(int iterations)
  {
    reserve_events(4 * (size_t)std::max(iterations, 0));
  }
  void release();

  spmv_hip_bicg_ws* ws = nullptr;
  int kmax_cap = -1;
  int64_t m_cap = -1, n_cap = -1, h_cap = -1, x_cap = -1, dinv_cap = -1;
  double *r = nullptr, *rhat = nullptr, *v = nullptr, *t = nullptr; // m_cap
  // n_cap: padded -- without a dinv p and s are what the SpMVs read; the
  // ghost tails are zeroed by every solve that reads them
  double *p = nullptr, *s = nullptr;
  double *ph = nullptr, *sh = nullptr; // h_cap: padded, dinv*p and dinv*s
  double* x = nullptr;      // x_cap: the iterate when the caller's x is unaligned
  double* dinv = nullptr;   // dinv_cap: the copy of an unaligned dinv
  // flags: {done, kstop, status}; timing_ev: 4 events per iteration
};

// BiCGStab from x0 = 0 for a matrix that need not be symmetric, with an
// optional diagonal RIGHT preconditioner.  `dinv` is nullptr or any finite
// nonzero DEVICE vector of A.row_map()->local_size() doubles, the inverse of
// the preconditioner's diagonal (Jacobi's: Matrix::diagonal + jacobi_inverse).
// Only Matrix::mult is used: every plan form, both storages and every halo
// model serve.  With `.` the global dot product:
//
//   r0 = b; rhat = b; p1 = b; rho[0] = rr[0] = b.b
//   for k = 1..kmax:
//     ph = dinv*p_k (p_k itself if dinv == nullptr); v = A ph; rv = rhat.v
//     rv == 0: breakdown 1 -- stop, k-1 iterations completed, x untouched by
//              this iteration
//     alpha = rho[k-1] / rv; s = r - alpha*v; sh = dinv*s (or s)
//     t = A sh; ts = t.s; tt = t.t; omega = (tt == 0) ? 0 : ts / tt
//     x += alpha*ph; x += omega*sh        (two roundings each, in this order)
//     r = s - omega*t; rr[k] = r.r; rho[k] = rhat.r
//     if sqrt(rr[k]) / sqrt(rr[0]) < rtol: stop (x and r updated, p not)
//     omega == 0 or rho[k] == 0: breakdown 2 -- stop after this iteration
//              (x, r and rr[k] are valid)
//     beta = (rho[k]/rho[k-1]) * (alpha/omega); p_(k+1) = r + beta*(p_k - omega*v)
//
// Products and sums are separate roundings.  There is no half-step exit on s,
// so an iteration has three reductions: rv, the pair {ts, tt}, the pair
// {rr, rho}; with several ranks each pair is ONE all-reduce of 2 doubles.  The
// stopping test is cg()'s; rnorm_history receives ||r_0||, ..., ||r_k||.  A
// system with r_0 . r_0 == 0 stops at k = 0 with x = 0 (the rule of pcg).
// Returns k, the number of iterations completed.  `status` (optional) receives
// 0 (the tolerance was met, or kmax was reached), 1 or 2 (the breakdowns
// above).  After a breakdown x is the last finite iterate: the quotient that
// cannot be formed never is, so no NaN of its making reaches x, r or the
// history.
//
// As in pcg(): scalars stay on the device, reductions are two-stage and
// deterministic, the decision to stop is taken on the device and the host only
// looks at a pinned flag every `poll_every` iterations; `x` IS the iterate and
// must not overlap `b` or `dinv` (std::runtime_error, "overlaps"); an `x` (or a
// `dinv`) that is not 16-byte aligned goes through the workspace's copy, x
// with one copy at the end; kmax < 0 throws; the executor's stream is
// restored on every exit path.  The halo update of ph / sh precedes each mult.
//
// options: poll_every, time_spmv (BOTH Matrix::mult calls of an iteration are
//          bracketed: CgStats::spmv_launches is 2 per iteration) and
//          consumer_reductions apply (one rank with consumer_reductions: 2 SpMV
//          + 5 launches per iteration, else 2 SpMV + 8 and 3 all-reduces);
//          defer_x and mixed are IGNORED: x is updated in every iteration, in
//          fp64.
int bicgstab(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
             const double* b, double* x, const double* dinv, int kmax,
             double rtol, std::vector<double>* rnorm_history = nullptr,
             const CgOptions* options = nullptr, CgStats* stats = nullptr,
             BicgstabWorkspace* workspace = nullptr, int* status = nullptr);

// ---- Restarted GMRES ----------------------------------------------------------
// (kGmresMaxRestart = 64: solver_args.h)

// The right preconditioner of gmres(): any FIXED linear operator.  All
// defaults: none.
struct GmresPreconditioner {
  // the inverse diagonal of bicgstab()'s dinv (z = dinv*v), or Chebyshev's dinv
  const double* dinv = nullptr;
  // >= 1: z = chebyshev_apply(v, dinv (may be nullptr), cheb_degree, lmin, lmax)
  int cheb_degree = 0;
  double lmin = 0, lmax = 0;
  // z = sgs_apply(*sgs, v); excludes the two above ("preconditioner")
  const SgsPreconditioner* sgs = nullptr;
  // z = amg_apply(*amg, v); excludes the three above ("preconditioner")
  const AmgPreconditioner* amg = nullptr;
};

// Work vectors + device scalars of gmres(), kept across calls like
// BicgstabWorkspace; it regrows itself when a call needs more rows, a longer
// restart or more iterations.  Owns the ChebyshevWorkspace of a Chebyshev
// preconditioner.
class GmresWorkspace : public SolverWorkspace
{
public:
  explicit GmresWorkspace(HipExecutor& exec);
  ~GmresWorkspace();

  // ---- internal to gmres() ----
  // basis_elems = stride * (restart + 1); need_b / need_dinv: the caller's b /
  // dinv is not 16-byte aligned and lives in the workspace's copy
  void ensure(int64_t M, int64_t N_padded, int64_t basis_elems, int kmax,
              bool need_b, bool need_dinv);
  void release();

  spmv_hip_gmres_ws* ws = nullptr;
  ChebyshevWorkspace cheb;
  int kmax_cap = -1;
  int64_t m_cap = -1, n_cap = -1, v_cap = -1, b_cap = -1, dinv_cap = -1;
  double *r = nullptr, *ax = nullptr, *u = nullptr; // m_cap
  // n_cap: padded -- z = M^-1 v_j is what the SpMV reads with a
  // preconditioner, x is the iterate (r = b - A x reads it through
  // Matrix::mult); the ghost tails are zeroed by every solve
  double *z = nullptr, *x = nullptr;
  double* V = nullptr;    // v_cap: the basis, restart + 1 padded vectors
  double* b = nullptr;    // b_cap: the copy of an unaligned b
  double* dinv = nullptr; // dinv_cap: the copy of an unaligned dinv
  // flags: {done, kstop, status, k}; timing_ev: 2 events per inner step
};

// the argument rules of gmres() that need no device (std::runtime_error):
// kmax < 0 ("kmax"), restart outside 1..kGmresMaxRestart ("restart"), sgs
// together with dinv or a Chebyshev degree, amg together with any of them
// ("preconditioner"),
// chebyshev_coefficients' rules ("degree", "bounds"), sgs->rows() != rows
// (gmres_check_rules of solver_args.h on the fields of M)
void gmres_check_arguments(const GmresPreconditioner* M, int restart, int kmax,
                           int64_t rows);

// Restarted GMRES(m) from x0 = 0 with a RIGHT preconditioner and twice-iterated
// classical Gram-Schmidt (CGS2), for a matrix that need not be symmetric.  It
// has no breakdown except the lucky one, and M^-1 is any fixed linear operator:
// none, dinv* (elementwise), chebyshev_apply, sgs_apply or amg_apply.  Only Matrix::mult
// is used: every plan form, both storages and every halo model serve.  With
// `.` the global dot product, m = restart, every product, sum, difference,
// quotient and square root one rounding of its own:
//
//   x = 0; r = b; rr0 = b.b; hist[0] = sqrt(rr0); k = 0; status = 0
//   rr0 == 0: return 0                       (the rule of pcg / bicgstab)
//   cycle:
//     beta = sqrt(r.r) (first cycle: hist[0]); v_0 = r * (1.0 / beta);
//     g = (beta, 0, ..)
//     for j = 0 .. m-1:
//       w  = A (M^-1 v_j)                    halo update first
//       h_i = v_i . w, i = 0..j              ONE multi-dot, one all-reduce of j+1
//       for i = 0..j in order:  w = w - h_i * v_i
//       c_i = v_i . w, i = 0..j              second pass, one all-reduce of j+1
//       for i = 0..j in order:  w = w - c_i * v_i ;  h_i = h_i + c_i
//       hn = sqrt(w.w)                       all-reduce of 1
//       column = (h_0..h_j, hn); rotations 0..j-1 in order:
//         t = c_i*col_i + s_i*col_{i+1}; col_{i+1} = -s_i*col_i + c_i*col_{i+1};
//         col_i = t
//       new rotation from a = col_j, b = col_{j+1}:
//         b == 0:     c = 1, s = 0
//         |b| > |a|:  tau = a/b; s = 1/sqrt(1 + tau*tau); c = s*tau
//         else:       tau = b/a; c = 1/sqrt(1 + tau*tau); s = c*tau
//       R_jj = c*a + s*b
//       R_jj == 0: status = 2; the column is discarded; leave with j columns
//       g_{j+1} = -s*g_j; g_j = c*g_j; k += 1; hist[k] = |g_{j+1}|
//       hn == 0: status = 1 (lucky breakdown); leave the loop
//       hist[k] / hist[0] < rtol or k == kmax: leave the loop
//       v_{j+1} = w * (1.0 / hn)
//     with the jn columns kept, i = jn-1 .. 0:
//       s = g_i; for l = i+1 .. jn-1 in order: s = s - R_il * y_l; y_i = s / R_ii
//     jn > 0: u = y_0 * v_0; for i = 1..jn-1: u = u + y_i * v_i; x = x + M^-1 u
//     if the loop was left early: return k
//     r = b - A x  (the true residual; its norm is NOT written to the history)
//     r.r == 0: return k
//
// rnorm_history receives hist[0..k]: for a right preconditioner hist[k] is the
// residual norm of x in exact arithmetic, so the histories compare with
// bicgstab()'s; the stopping test is cg()'s.  Returns k, the inner steps
// completed; `status` (optional) receives 0, 1 or 2 as above.
//
// As in bicgstab(): scalars (the Hessenberg columns, the rotations, g, the
// history, k) stay on the device, reductions are two-stage and deterministic,
// the decision to stop is taken on the device and the host only looks at a
// pinned flag every `poll_every` inner steps.  After the stop the Arnoldi
// kernels return at once, the cycle that stopped still gets its update of x
// exactly once, and nothing afterwards changes x, the history or k (the
// preconditioner and the SpMV may still run on scratch).  The iterate lives in
// the workspace's padded vector (r = b - A x reads it through Matrix::mult)
// and `x` takes ONE copy at the end, so an `x` of any alignment serves; a `b`
// or `dinv` that is not 16-byte aligned goes through the workspace's copy.
// `x` must not overlap `b` or `dinv` (std::runtime_error, "overlaps"); the
// argument rules are those of gmres_check_arguments, checked before anything
// touches a device; the executor's stream is restored on every exit path.
//
// options: poll_every and time_spmv apply (time_spmv brackets the Matrix::mult
//          of every Arnoldi step: CgStats::spmv_launches is 1 per inner step
//          enqueued; the SpMVs of r = b - A x and of a Chebyshev
//          preconditioner are not timed); consumer_reductions, defer_x and
//          mixed are IGNORED.
int gmres(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
          const double* b, double* x, const GmresPreconditioner* M, int restart,
          int kmax, double rtol, std::vector<double>* rnorm_history = nullptr,
          const CgOptions* options = nullptr, CgStats* stats = nullptr,
          GmresWorkspace* workspace = nullptr, int* status = nullptr);

// ---- Preconditioned MINRES ----------------------------------------------------

// The preconditioner of minres(): symmetric positive definite.  All defaults:
// none.  At most one may be set ("preconditioner").
struct MinresPreconditioner {
  // a POSITIVE device vector, z = dinv*r (Jacobi: 1 / |diag|)
  const double* dinv = nullptr;
  // z = sgs_apply(*sgs, r): SGS, or ILU(0) / IC(0) with negative_pivots() == 0
  // ("pivot")
  const SgsPreconditioner* sgs = nullptr;
  // z = amg_apply(*amg, r)
  const AmgPreconditioner* amg = nullptr;
};

// Work vectors + device scalars of minres(), kept across calls like
// GmresWorkspace; it regrows itself when a call needs more rows or more
// iterations.
class MinresWorkspace : public SolverWorkspace
{
public:
  explicit MinresWorkspace(HipExecutor& exec) : SolverWorkspace(exec) {}
  ~MinresWorkspace();

  // ---- internal to minres() ----
  // need_y: a preconditioner is set; need_x / need_dinv: the caller's x / dinv
  // is not 16-byte aligned and lives in the workspace's copy
  void ensure(int64_t M, int64_t N_padded, int kmax, int partials_len,
              bool need_y, bool need_x, bool need_dinv);
  void release();

  spmv_hip_minres_ws* ws = nullptr;
  int kmax_cap = -1;
  int64_t m_cap = -1, n_cap = -1, y_cap = -1, x_cap = -1, dinv_cap = -1;
  // m_cap: Av; r1 and r2 rotate over ra, rb (t is written over r1); w1 and w2
  // rotate over wa, wb (w is written over w1)
  double *Av = nullptr, *ra = nullptr, *rb = nullptr, *wa = nullptr,
         *wb = nullptr;
  double* v = nullptr;    // n_cap: padded, what the SpMV reads
  double* y = nullptr;    // y_cap: M^-1 r2 (without a preconditioner y IS r2)
  double* x = nullptr;    // x_cap: the iterate of an unaligned x
  double* dinv = nullptr; // dinv_cap: the copy of an unaligned dinv
  double* dot2 = nullptr; // partials of the remote block's v.Av share
  // flags: {done, kstop, status}; timing_ev: 2 events per iteration
};

// Preconditioned MINRES from x0 = 0 for a SYMMETRIC matrix that need not be
// definite (a shifted operator A - sigma I, a saddle-point system), in either
// storage, and a symmetric positive definite preconditioner M: none, dinv*
// (elementwise), sgs_apply or amg_apply.  One SpMV, one application of M^-1 and
// a fixed number of vector passes per iteration; the residual in the M^-1-norm
// never grows.  Only Matrix::mult (mult_dot) is used: every plan form and halo
// model serves.  With `.` the global dot product, every product, sum,
// difference, quotient and square root one rounding of its own:
//
//   x = 0; r1 = r2 = b; y = M^-1 r2; ry = r2.y
//   ry < 0: status 2, return 0.     beta1 = sqrt(ry); hist[0] = beta1
//   beta1 == 0: return 0 with x = 0            (the rule of pcg / gmres)
//   oldb = 0; beta = beta1; dbar = 0; epsln = 0; phibar = beta1; cs = -1;
//   sn = 0; w = w2 = 0; k = 0
//   v = y * (1.0 / beta)
//   while k < kmax:
//     Av   = A v                     halo update of v first; alfa = v.Av
//     t    = (Av - (beta/oldb)*r1) - (alfa/beta)*r2
//                                    (k == 0: t = Av - (alfa/beta)*r2)
//     r1 = r2; r2 = t; y = M^-1 r2; ry = r2.y
//     ry < 0: status 2; stop (x is the iterate of k)
//     oldb = beta; beta = sqrt(ry)
//     oldeps = epsln; delta = cs*dbar + sn*alfa; gbar = sn*dbar - cs*alfa
//     epsln = sn*beta; dbar = -cs*beta
//     gamma = sqrt(gbar*gbar + beta*beta)
//     gamma == 0: status 3; stop (singular direction; x is the iterate of k)
//     cs = gbar/gamma; sn = beta/gamma; phi = cs*phibar; phibar = sn*phibar
//     w1 = w2; w2 = w; w = ((v - oldeps*w1) - delta*w2) * (1.0/gamma)
//     x = x + phi*w
//     k += 1; hist[k] = |phibar|
//     beta == 0: status 1 (the Lanczos process ended: x is exact); stop
//     hist[k] / hist[0] < rtol: stop
//     v = y * (1.0 / beta)
//
// alfa is taken as v.(A v), BEFORE r1 is subtracted: equal in exact arithmetic
// (v is M-orthogonal to the previous Lanczos vector), it lets the SpMV's fused
// dot serve and makes the whole update of t one kernel.
//
// rnorm_history receives hist[0..k]: the residual in the M^-1-norm, sqrt(r .
// M^-1 r).  Without a preconditioner that is the 2-norm and the histories
// compare with cg()'s; with one they do NOT compare with pcg()'s, which are
// 2-norms.  Returns k; `status` (optional) receives 0 (converged, or kmax
// reached), 1, 2 or 3 as above.  A non-finite scalar takes the "go on" branch of
// every comparison, so such a solve ends at kmax, as in gmres().
//
// Scaling.  (2^s A, 2^t b) repeats the solve of (A, b) bit for bit (x times
// 2^(t-s); the history times 2^t without a preconditioner, times 2^(t - s/2)
// for an even s with an M^-1 that scales by 2^-s) only while gbar*gbar +
// beta*beta stays a normal number: roughly |s| < 510 without a preconditioner,
// any s with one, since alfa, gbar and (from k = 1) beta then do not scale.
// Outside that range the sum overflows (gamma = Inf: a non-finite history that
// runs to kmax, or, where beta == 0, status 1 with hist[k] = 0 and an x that
// never moved) or underflows to 0 (gamma == 0: status 3 on a regular system).
// A right-hand side whose r.M^-1 r underflows to 0 (b = 1e-200) stops at the
// start with beta1 == 0, k = 0 and x = 0 although b != 0.
//
// Launches of one iteration on one rank, beside the SpMV (with its fused
// v.Av; symmetric storage: plus one dot kernel): update_r (adds the partials of
// alfa itself; t over r1's buffer, y = dinv*t, partials of r2.y), the reducer,
// step (one wave: all the scalars above, the history, the stop), update_xwv (w
// over w1's buffer, x, the next v): 4 launches and 14 vector passes with dinv
// (update_r: Av, r1, r2, dinv in, r2, y out; update_xwv: v, w1, w2, x, y in, w,
// x, v out), 12 without a preconditioner (y is r2 itself).  With sgs or amg the
// application and the dot-partials kernel follow update_r.  With several ranks:
// one reducer more and two all-reduces of 1 double (alfa, ry).
//
// As in gmres(): the scalars stay on the device, reductions are two-stage and
// deterministic, the decision to stop is taken on the device and the host only
// looks at a pinned flag every `poll_every` iterations.  After the stop every
// kernel returns at once, so x is exactly the iterate of the returned k (the
// SpMV and the preconditioner may still run on scratch).  `x` IS the iterate,
// as in pcg(): zeroed at the start, updated in place, and after a throw it
// holds whatever had been reached; an `x` or `dinv` that is not 16-byte
// aligned goes through the workspace's copy (b is copied anyway: it is the
// first r2).  The argument rules are minres_check_rules' (solver_args.h:
// "kmax", "preconditioner", "rows", "pivot", "overlaps"), checked before
// anything touches a device; the executor's stream is restored on every exit
// path.
//
// options: poll_every and time_spmv apply (one timed Matrix::mult per
//          iteration); consumer_reductions, defer_x and mixed are IGNORED.
int minres(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
           const double* b, double* x, const MinresPreconditioner* M, int kmax,
           double rtol, std::vector<double>* rnorm_history = nullptr,
           const CgOptions* options = nullptr, CgStats* stats = nullptr,
           MinresWorkspace* workspace = nullptr, int* status = nullptr);

// ---- LSQR -----------------------------------------------------------------------

// Work vectors + device scalars of lsqr(), kept across calls like
// MinresWorkspace; it regrows itself when a call needs more rows, more columns
// or more iterations.
class LsqrWorkspace : public SolverWorkspace
{
public:
  explicit LsqrWorkspace(HipExecutor& exec) : SolverWorkspace(exec) {}
  ~LsqrWorkspace();

  // ---- internal to lsqr() ----
  // need_x: the caller's x is not 16-byte aligned and lives in the workspace's
  // copy
  void ensure(int64_t M, int64_t N, int64_t N_padded, int kmax, bool need_x);
  // two products per iteration
  void reserve_timing(int iterations)
  {
    reserve_events(4 * (size_t)std::max(iterations, 0));
  }
  void release();

  spmv_hip_lsqr_ws* ws = nullptr;
  int kmax_cap = -1;
  int64_t m_cap = -1, n_cap = -1, w_cap = -1, x_cap = -1;
  double *ut = nullptr, *Av = nullptr;  // m_cap: the row space
  double *vt = nullptr, *Atu = nullptr; // n_cap: padded, what mult reads and
                                        // transpmult writes
  double* w = nullptr;                  // w_cap: the owned columns
  double* x = nullptr;                  // x_cap: the iterate of an unaligned x
  // flags: {done, kstop, status}; timing_ev: 4 events per iteration
};

// LSQR (Paige and Saunders, 1982) from x0 = 0 for ANY matrix, rectangular or
// square, in either storage: min ||A x - b|| of an over-determined system, the
// damped fit min ||A x - b||^2 + damp^2 ||x||^2, the minimum-norm solution of
// an under-determined system, and a breakdown-free solver for the square
// nonsymmetric systems on which bicgstab() gives up.  Only Matrix::mult,
// Matrix::transpmult, col_map()->update and reverse_update are used: every plan
// form and halo model serves.  b: A.row_map()->local_size() doubles; x:
// A.col_map()->local_size() doubles.  With `.` the global dot product, A^T u
// the transposed product followed by the reverse halo update, taken over the
// owned columns, every product, sum, difference, quotient and square root one
// rounding of its own:
//
//   x = 0; ut = b; beta = sqrt(ut.ut); hist_r[0] = beta
//   beta == 0: return 0 with x = 0
//   ib = 1/beta; vt = (A^T ut)*ib; alpha = sqrt(vt.vt); hist_ar[0] = alpha*beta
//   alpha == 0: status 2, return 0
//   ia = 1/alpha; w = vt*ia; phibar = beta; rhobar = alpha; anorm2 = 0;
//   psi2 = 0; k = 0
//   while k < kmax:
//     ut = (A vt)*ia - alpha*(ut*ib)          halo update of vt first
//     beta = sqrt(ut.ut)
//     anorm2 = ((anorm2 + alpha*alpha) + beta*beta) + damp*damp
//     beta != 0: ib = 1/beta; vn = (A^T ut)*ib - beta*(vt*ia);
//                alpha_n = sqrt(vn.vn)        (else alpha_n = 0)
//     rhobar1 = sqrt(rhobar*rhobar + damp*damp); cs1 = rhobar/rhobar1;
//     sn1 = damp/rhobar1
//     psi = sn1*phibar; phibar = cs1*phibar; psi2 = psi2 + psi*psi
//     rho = sqrt(rhobar1*rhobar1 + beta*beta); cs = rhobar1/rho; sn = beta/rho
//     theta = sn*alpha_n; rhobar = -cs*alpha_n; phi = cs*phibar;
//     phibar = sn*phibar
//     x = x + (phi/rho)*w;  k += 1
//     hist_r[k] = sqrt(phibar*phibar + psi2)
//     hist_ar[k] = |(phibar*alpha_n)*cs|
//     beta == 0 or alpha_n == 0: status 2; stop (the bidiagonalisation ended:
//                                x is the solution in exact arithmetic)
//     hist_r[k] / hist_r[0] < rtol: stop
//     hist_ar[k] / (sqrt(anorm2)*hist_r[k]) < ltol: status 1; stop
//     vt = vn; alpha = alpha_n; ia = 1/alpha; w = vt*ia - (theta/rho)*w
//
// ut and vt are the UN-NORMALISED vectors of the Golub-Kahan process: their
// scales ib and ia ride into the kernel that consumes the next product (A and
// A^T are linear), which saves two read-and-write passes per iteration.  vt is
// the padded column-space vector mult reads; its ghost tail is zeroed by every
// solve and refreshed by the halo update before each mult.
//
// hist_r receives hist_r[0..k]: the estimate of ||b - A x|| (damp > 0: of
// sqrt(||b - A x||^2 + damp^2 ||x||^2)); hist_ar receives hist_ar[0..k]: the
// estimate of ||A^T (b - A x) - damp^2 x||.  Returns k; `status` (optional)
// receives 0 (kmax reached, or the rtol test), 1 (the least-squares test) or 2.
// A non-finite scalar takes the "go on" branch of every comparison, so such a
// solve ends at kmax with status 0, as in minres(); the workspace is usable
// afterwards.  In the kernels' order: start tests beta == 0 (status 0), writes
// hist_ar[0], then tests alpha == 0 (status 2); step writes every scalar, k and
// both histories, then tests the breakdown, rtol, ltol and k == kmax in that
// order, so an exit that coincides with kmax keeps its status.
//
// Non-finite and extreme data.  A NaN in b or A: kmax, status 0, x all NaN.  An
// Inf in b: the same with hist_r[0] = Inf.  A b whose b.b overflows (1e200):
// beta = Inf, ib = 0, vt = 0 and alpha == 0: k = 0, status 2, hist_r (Inf),
// hist_ar (NaN), x = 0.  A b whose b.b underflows to 0 (1e-200) stops at the
// start with k = 0, status 0 and x = 0 although b != 0.  A damp whose square
// overflows (1e200) makes rhobar1 and rho infinite: phibar = 0 passes the rtol
// test while phi is a NaN, so the solve returns k = 1, status 0, hist_r[1] = 0
// and an x of NaN -- a wrong answer that looks converged.  A damp whose square
// underflows (1e-200) is the solve of damp = 0, bit for bit.
//
// Scaling.  (2^s A, 2^t b, 2^s damp) repeats the solve of (A, b, damp) bit for
// bit (x times 2^(t-s), hist_r times 2^t, hist_ar times 2^(s+t), the same k
// and status); so do (A, -b) and (-A, b) with -x.  vt is un-normalised, of size
// 2^s |A^T b| / |b|, so the relation holds only while vt.vt stays a normal
// number, roughly |s| < 510.  Above, vt.vt overflows: alpha = Inf, ia = 0 and
// the solve runs to kmax on NaN with status 0.  Below, it underflows to 0:
// alpha == 0, k = 0 and status 2 on a regular system.
//
// Launches of one iteration on one rank, beside mult and transpmult: update_u
// (3 passes of m), update_v (adds the partials of ut.ut itself, in the
// reducer's order; 3 passes of n), step (one workgroup adds the partials of
// vn.vn in the reducer's order, its thread 0 does all the scalar arithmetic),
// update_xw (5 passes of n): 4 launches, 11 vector passes.  With several ranks:
// two reducer launches more and two all-reduces of 1 double (ut.ut, vn.vn).
//
// As in minres(): the scalars stay on the device, the decision to stop is
// taken there and the host only looks at a pinned flag every `poll_every`
// iterations.  update_xw runs exactly when step k completed, so x is the
// iterate of the returned k whatever poll_every is, and w is not written on the
// step that stops.  `x` IS the iterate: zeroed at the start, updated in place;
// an x that is not 16-byte aligned goes through the workspace's copy (b is
// copied anyway: it is the first ut).  The argument rules are
// lsqr_check_rules' (solver_args.h: "kmax", "ltol", "damp", "overlaps"),
// checked before anything touches a device; the executor's stream is restored
// on every exit path.
//
// options: poll_every and time_spmv apply (both products are bracketed:
//          spmv_launches is 2 per iteration); the other CgOptions are IGNORED.
int lsqr(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
         const double* b, double* x, int kmax, double rtol, double ltol,
         double damp, std::vector<double>* hist_r = nullptr,
         std::vector<double>* hist_ar = nullptr, int* status = nullptr,
         const CgOptions* options = nullptr, CgStats* stats = nullptr,
         LsqrWorkspace* workspace = nullptr);

// ---- LOBPCG ---------------------------------------------------------------------
struct LobpcgOptions {
  int poll_every = 16;    // host looks at the device's `done` flag this often
  bool time_spmv = false; // bracket the one mult_block of every iteration
  // the Rayleigh-Ritz step keeps the nev LARGEST Ritz values (eigenvalues come
  // back descending): a converged lambda_max with a residual bound, where
  // lambda_max_estimate() gives an estimate
  bool largest = false;
};

// CgStats plus what the epilogue measured
struct LobpcgStats : CgStats {
  // ||A x_c - theta_c x_c|| (with B: ||A x_c - theta_c B x_c||) with AX = A X
  // (and BX = B X) computed explicitly after the loop (the loop's AX and BX are
  // updated implicitly and drift), nev entries
  std::vector<double> true_resnorm;
  int restarts = 0; // Rayleigh-Ritz steps repeated without P
};

// Work blocks + device scalars of lobpcg(), kept across calls like
// PcgBlockWorkspace; it regrows itself when a call needs more rows, more
// iterations or another nev.  Every block is rewritten by the next prologue.
class LobpcgWorkspace : public SolverWorkspace
{
public:
  explicit LobpcgWorkspace(HipExecutor& exec) : SolverWorkspace(exec) {}
  ~LobpcgWorkspace();

  // ---- internal to lobpcg() ----
  // with_b: the blocks of a solve with B as well (they stay for later solves)
  void ensure(int64_t m_elems, int64_t n_elems, int kmax, int nev, bool need_x,
              bool with_b = false);
  void release();

  // (flags: {done, kstop, status, it, active, has_p, restarts, basis})
  spmv_hip_lobpcg_ws* ws = nullptr;
  int kmax_cap = -1, nev_cap = 0;
  int64_t m_cap = -1, n_cap = -1, x_cap = -1, b_cap = -1;
  double *r = nullptr, *p = nullptr, *ax = nullptr, *aw = nullptr,
         *ap = nullptr;  // m_cap
  double *bx = nullptr, *bw = nullptr, *bp = nullptr; // b_cap: solves with B
  double* x = nullptr;   // x_cap: the iterate when the caller's X is unaligned
  double* w = nullptr;   // n_cap: padded, the ghost tail is zeroed by every solve
};

// LOBPCG (Knyazev, 2001): the nev smallest (options->largest: largest)
// eigenpairs of a SYMMETRIC A in either storage, fp64, rows and owned columns
// the same index range, 1 <= nev <= 8.  X is a device block of local_size * nev
// doubles in the mult_block layout: the initial guess on entry (never all
// zero), the Ritz vectors, orthonormal to rounding, on exit.  Every product,
// sum, difference, quotient and square root is one rounding; k = nev:
//
//   prologue: G = X^T X; X = X R^-1 (R = chol(G)); AX = A X; Rayleigh-Ritz on
//             (X^T AX, X^T X), k x k: X, AX, theta
//   it = 0:   R = AX - X diag(theta); rn_c = ||r_c||; hist[c][0] = rn_c
//             column c has met its test when rn_c < max(rtol |theta_c|, atol)
//             (a NaN says "go on"); it is then inactive for good
//   while some column is active and it < kmax:
//     W  = M^-1 R     (dinv * R in the residual kernel, sgs_apply_block,
//                      amg_apply_block, or W = R)
//     AW = A W        (update_block of the padded W, then mult_block)
//     S  = [X, W_act, P_act], AS likewise: soft locking, X keeps all columns;
//          P is absent in the first iteration and after a restart
//     Gb = S^T S, Ga = S^T AS: one pass over the six blocks, masked columns
//          summed as well and ignored by the next step
//     Rayleigh-Ritz on (Ga, Gb), m = k + 2 n_act <= 24 -> theta, C (m x k)
//     X' = S C; AX' = AS C; P' = [W_act, P_act] C_wp; AP' likewise: one pass,
//          in place; P and AP of an inactive column are left alone
//     R = AX - X diag(theta); rn; hist; the mask; it += 1
//   epilogue: AX = A X explicitly, R and ||r_c|| from it -> stats->true_resnorm
//
// The Rayleigh-Ritz step (one workgroup, blas1_lobpcg.hip states every rule):
// Gram sums finished in a fixed order (the workgroups' partials of an entry
// added left to right in index order -- NOT sum_partials' tree, which the dot
// products of the other solvers use), compacted by the active mask, scaled by
// 1 / sqrt(diag Gb), Gb = R^T R by Cholesky, R^-T Ga R^-1, cyclic Jacobi with a
// fixed pair order, nev Ritz values selected ascending (largest: descending),
// ties by index, C = R^-1 Z with the scaling undone.  A Cholesky pivot that
// fails piv > 0 (a NaN fails it), or a Ritz value that is not finite, repeats
// the step with S = [X, W_act] (a restart); if that fails too the solve ends
// with status 1 and X the last iterate.  Non-finite data end that way as well,
// and so does a rank-deficient initial X whenever its factorisation meets a
// pivot that is not positive (status 1 at k = 0).  In rounded arithmetic the
// pivot of a dependent column is a difference of nearly equal numbers and may
// come out a tiny positive one: no threshold other than > 0 decides, so such a
// block is not guaranteed to be refused; it then runs on a basis of rounding
// noise and usually collapses at a later step.
//
// Edges (tests/lobpcg_edges.py, found on the restatement, held on the device):
//  - Rows.  With local rows = nev the prologue's pairs are exact to rounding and
//    the solve returns at k = 0, status 0.  With fewer than 3 nev rows [X, W, P]
//    cannot have full rank: the pivots are rounding noise and the solve usually
//    ends with status 1 within a few iterations, unless it converges first.
//    Such a run may also reach kmax with status 0 and Ritz values far outside
//    the spectrum (diag(1..8), nev 3: theta = -2.5e59): check true_resnorm.
//  - The test rn_c < max(rtol |theta_c|, atol) is strict.  An exactly converged
//    pair with theta_c = 0 (rn_c = 0) does not meet it at atol = 0: the column
//    stays active, W = 0, and the step collapses (status 1); pass atol > 0.
//  - Scales.  2^s A gives the same X and theta, history times 2^s for
//    -335 <= s <= 339 without a preconditioner (W = R carries 2^s, W^T A W
//    2^3s) and for -490 <= s <= 510 with dinv 2^-s; columns of X0 times 2^t
//    give the same result for -512 <= t <= 507 (x0.x0 = 2^(2t) 443 on the
//    Poisson matrix of 11^3 rows).  Beyond: status 1 at k = 0 where a Gram sum
//    overflows; where products underflow, first other bits, further out a
//    status 1 some iterations later.
//  - A NaN or Inf in dinv meets the first step's Gram sums: status 1 at k = 0,
//    and X is the prologue's orthonormalised and rotated block, not the X0
//    passed in.  A NaN or Inf in X0 returns X0 itself (the first factorisation
//    fails); an Inf in A returns the orthonormalised X0; an entry of A whose
//    products overflow (1e200) ends at k = 0 with the prologue's rotated block,
//    finite theta and true_resnorm = Inf.
//  - Several ranks take every branch from their own copy of the all-reduced
//    Gram sums and norms: Comm::reduce_sum must leave the same bits on every
//    rank (it does on the peer windows and on the transports of this
//    repository), else one rank restarts or stops alone and the
//    others wait in the next all-reduce.
//
// Returns the number of iterations.  eigenvalues (optional): nev Ritz values.
// resnorm_history (optional): nev * (kmax + 1) entries, column c at
// [c * (kmax + 1) + it], -1.0 beyond the iteration at which the column met its
// test.  status (optional): 0 every column met its test or kmax was reached,
// 1 the basis collapsed.  The scalars stay on the device, the decision to stop
// is taken there and the host only looks at a pinned flag every poll_every
// iterations; after `done` every kernel returns at once, so X is exactly the
// iterate of the returned k.  An X that is not 16-byte aligned goes through the
// workspace's copy.
//
// M: at most one member set; none: W = R.  The arguments are checked before
// anything touches a device (lobpcg_check_rules of solver_args.h;
// std::runtime_error): "nev", "kmax", "tol" (rtol, atol finite, >= 0, not both
// 0), "preconditioner", "rows", "pivot".  Several ranks: one all-reduce of the
// Gram sums (2 m m doubles) and one of nev doubles per iteration, the halo
// exchange of W before mult_block, preconditioners block-Jacobi over the ranks.
// Launches of one iteration on one rank beside mult_block and M: gram,
// gram_reduce, rr, update, residual, norms; 6 + 10 + 3 (+1 with W) block passes.
//
// B != nullptr: the GENERALISED problem A x = lambda B x, A symmetric, B
// SYMMETRIC POSITIVE DEFINITE, both fp64, each in either storage (the storages
// may differ).  The nev smallest (largest) eigenpairs of the pencil; on exit X
// is B-orthonormal to rounding (X^T B X = I) and the eigenvalues are the Ritz
// values of the pencil.  M approximates A^-1 as before.  One rounding per
// operation; k = nev:
//
//   prologue: BX = B X (through the padded W, like AX); Gb = X^T BX;
//             R = chol(Gb); X = X R^-1, BX = BX R^-1 (one update, the same
//             coefficients: BX is updated implicitly); AX = A X; Rayleigh-Ritz
//             on (X^T AX, X^T BX); X, AX, BX <- . C
//   it = 0:   R = AX - BX diag(theta); rn_c = ||r_c||; the test is the one
//             above, rn_c < max(rtol |theta_c|, atol)
//   while some column is active and it < kmax:
//     W  = M^-1 R
//     one update_block of the padded W, then AW = A W and BW = B W
//     S  = [X, W_act, P_act], AS and BS likewise
//     Gb = S^T BS, Ga = S^T AS: one pass over the nine blocks; the upper
//          triangle entry (i, j), i <= j, is sum_rows s_i * (Bs)_j, in the
//          summation order of the pass over six blocks
//     Rayleigh-Ritz on (Ga, Gb): the step above, unchanged (gram_reduce, the
//          all-reduce of 2 m m doubles, rr)
//     X' = S C, P' = [W_act, P_act] C_wp, likewise AX', AP' and BX', BP': in
//          place, each of the nine blocks read once and each of the six
//          outputs written once (one launch, a thread owns a row of ONE triple)
//     R = AX - BX diag(theta); rn; hist; the mask; it += 1
//   epilogue: AX = A X and BX = B X explicitly, R and ||r_c|| from them ->
//             stats->true_resnorm = ||A x_c - theta_c B x_c||
//
// Restarts, the collapse, soft locking, the state words and `done` are exactly
// those above: they hang off the Rayleigh-Ritz step.  A B that is not positive
// definite shows up as a Cholesky pivot of Gb that fails piv > 0, and the solve
// ends with status 1 like a rank-deficient block; NO OTHER TEST of definiteness
// (or of symmetry) is made, and an indefinite B whose Gb happens to factor is
// not refused.  With B the identity the solve has the bits of the solve
// without B: BX then goes through the arithmetic of X.
//
// The rule "pencil" (lobpcg_check_pencil of solver_args.h, checked with the
// other rules before anything touches a device): B has A's local row count and
// B's column map exactly A's ghost list, the same global indices in the same
// order -- what two operators assembled on one mesh have.  One halo exchange of
// the padded W (A's column map) then serves both products: B's product runs
// behind A's, which waits for the exchange; where B's product comes alone (the
// prologue's BX = B X) lobpcg() makes the stream wait for A's exchange itself
// (update_finalise_block), since B's own column map has nothing in flight.
// Launches of one
// iteration on one rank beside the two mult_block and M: gram_gen,
// gram_reduce, rr, update_gen, residual, norms (six, as above); 9 + 15 + 3
// (+1 with W) block passes.  Several ranks: the same two all-reduces, of the
// same sizes.  options->time_spmv brackets A's product alone.  The workspace
// grows bx, bw, bp at the first solve with B and may alternate between solves
// with and without B.
int lobpcg(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
           double* X, int nev, const BlockPreconditioner& M, int kmax,
           double rtol, double atol, std::vector<double>* eigenvalues = nullptr,
           std::vector<double>* resnorm_history = nullptr, int* status = nullptr,
           const LobpcgOptions* options = nullptr, LobpcgStats* stats = nullptr,
           LobpcgWorkspace* workspace = nullptr,
           const Matrix<double>* B = nullptr);

// ---- multi-shift CG -------------------------------------------------------------

// Work vectors + device scalars of cg_shifted(), kept across calls like
// LsqrWorkspace; it regrows itself when a call needs more rows, more
// iterations or more shifts.
class CgShiftedWorkspace : public SolverWorkspace
{
public:
  explicit CgShiftedWorkspace(HipExecutor& exec) : SolverWorkspace(exec) {}
  ~CgShiftedWorkspace();

  // ---- internal to cg_shifted() ----
  // need_x: a column of the caller's X is not 16-byte aligned and the iterate
  // lives in the workspace's copy
  void ensure(int64_t M, int64_t N_padded, int ns, int kmax, int len,
              bool need_x);
  void release();

  spmv_hip_cgs_ws* ws = nullptr;
  int kmax_cap = -1;
  int64_t m_cap = -1, n_cap = -1, ps_cap = -1, x_cap = -1;
  int64_t ld = 0;           // stride of ps and x: M rounded up to an even number
  double *r = nullptr, *q = nullptr; // m_cap
  double* p = nullptr;      // n_cap: the padded seed direction mult_dot reads
  double* ps = nullptr;     // ps_cap = ns * ld: the directions p_s
  double* x = nullptr;      // x_cap = ns * ld: the iterate of an unaligned X
  double* dot2 = nullptr;   // len: the remote block's share of p.q
  // flags: {done, kstop, status, its[8]}; timing_ev: 2 events per iteration
};

// Multi-shift CG (Frommer; Jegerlehner 1996): solves (A + sigma_s I) x_s = b for
// ns shifts with ONE product per iteration.  The Krylov space of A + sigma I is
// that of A and the residuals are collinear, r_s = zeta_s r, so every shifted
// system rides on the seed recurrence of A for three scalars and two vector
// updates per iteration, and its stopping test is free: ||r_s|| = |zeta_s| ||r||.
// A: symmetric positive definite, in either storage; only Matrix::mult_dot and
// col_map()->update are used: every plan form and halo model serves.  1 <= ns
// <= 8; every sigma_s finite and >= 0, in any order, duplicates allowed; the
// seed is always A.  b: A.row_map()->local_size() doubles; solution s is the
// CONTIGUOUS vector X + s * ldx, ldx >= rows (not the interleaved layout of
// mult_block: most of a solve runs with few shifts active, and a stopped column
// of an interleaved block still travels in every cache line; here it is neither
// read nor written, and each x_s is handed on as an ordinary vector).  With `.`
// the global dot product, every product, sum, difference, quotient and square
// root one rounding of its own, the parentheses as written (the RATIO form: it
// carries rho_s = zeta_s^(k+1) / zeta_s^k, not the product of two zetas, so a
// zeta that underflows does no harm):
//
//   r = b; p = b; rr = r.r; hist_s[0] = sqrt(rr) for every s
//   for every s: x_s = 0; p_s = b; zeta_s = 1; rho_s = 1
//   a_old = 1; b_old = 0; k = 0
//   rr == 0: every shift stopped at k = 0, status 0
//   while k < kmax and some shift is active:
//     q = A p; pq = p.q                       halo update of p first
//     not (pq > 0): status 1; stop            (a NaN fails it; X stays the last
//                                             iterate)
//     a = rr / pq
//     for every active s:
//       rhon_s = a_old / ((a*b_old)*(1 - rho_s) + a_old*(1 + sigma_s*a))
//     r = r - a*q; rrn = r.r; bn = rrn / rr; k += 1
//     for every active s:
//       x_s = x_s + (a*rhon_s)*p_s
//       zeta_s = zeta_s*rhon_s; rho_s = rhon_s
//       hist_s[k] = |zeta_s| * sqrt(rrn); iterations_s = k
//       hist_s[k] / hist_s[0] < rtol: s stops (x_s updated, p_s left alone)
//       else p_s = zeta_s*r + (bn*(rhon_s*rhon_s))*p_s
//     p = r + bn*p; rr = rrn; a_old = a; b_old = bn
//     rrn == 0: every active shift stops, status 0
//
// A stopped shift is frozen for good.  A non-finite scalar takes the "go on"
// branch of the rtol comparison, as in minres() and lsqr().  Returns the largest
// iterations_s; `iterations` (optional) receives the ns counts, `rnorm_history`
// (optional) ns * (kmax + 1) doubles in cg_block's layout, hist_s[j] at
// s * (kmax + 1) + j, -1.0 beyond iterations_s; `status` (optional) 0 or 1.
// In the kernels' order: start writes hist_s[0], then tests rr == 0; step tests
// not (pq > 0) first, then forms a, bn and every rhon_s (whose divisor has no
// zero test of its own), writes hist_s[k], tests rtol per shift, and last "no
// shift left, rrn == 0 or k == kmax".  No step runs beyond kmax, so a pq <= 0
// that step kmax + 1 would have met is not found: status 0.
//
// Non-finite and extreme data.  A NaN or Inf in b, or a NaN in A, makes the
// first pq a NaN: k = 0, status 1, X = 0.  A b whose b.b overflows (1e200): rr =
// pq = Inf, a is a NaN, the second pq is a NaN: k = 1, status 1, X all NaN.  A b
// whose b.b underflows to 0 (1e-200): k = 0, status 0, X = 0 although b != 0.  A
// huge finite shift (1e300) beside others: rhon_s = 1 / (sigma_s a) and zeta_s
// are tiny, x_s = b / sigma_s after one step, the shift stops there and the
// other columns have the bits they have without it.
//
// Scaling.  (2^s A, 2^t b, 2^s sigma) repeats the solve of (A, b, sigma) bit
// for bit, every x_s times 2^(t-s) and every history times 2^t, with the same
// counts; (A, -b) gives -X; (-A, b) is status 1 at k = 0.  No square of an
// entry of A is formed, so s alone has no floor (s = +-540 repeats the exact
// solves); the relation ends where rr = 2^(2t) r.r or pq = 2^(2t+s) p.Ap leaves
// the normal range, e.g. (s, t) = (-400, -300).
//
// Launches of one iteration on one rank, beside mult_dot: update_r (adds the
// partials of p.q itself, in the reducer's order; 3 passes), step (one
// workgroup adds the partials of r.r in the reducer's order, its thread 0 does
// the scalar arithmetic of every active shift and leaves the compacted lists),
// update_xp (reads r once; 4 passes per shift it moves, 2 for one that stops in
// this step, 2 for the seed's p): 3 launches (4 where mult_dot cannot fuse its
// dot), 4 n_act + 6 vector passes.  With several ranks: two reducer launches
// more and two all-reduces of 1 double (pq, rrn), whatever ns is.
//
// As in lsqr(): the scalars stay on the device, the decision to stop is taken
// there and the host only looks at a pinned flag every `poll_every` iterations.
// update_xp runs exactly when step k completed, so X is the iterate of the
// returned counts whatever poll_every is.  `X` IS the iterate: zeroed at the
// start, updated in place; columns that are not 16-byte aligned (an odd ldx
// with ns > 1, or X 8 bytes off) go through the workspace's copy and one copy
// back at the end.  The argument rules are cgs_check_rules' (solver_args.h:
// "ns", "kmax", "ldx", "shifts", "overlaps"), checked before anything touches a
// device; the executor's stream is restored on every exit path; the workspace
// is usable after every exit.
//
// options: poll_every and time_spmv apply (spmv_launches is 1 per iteration);
//          the other CgOptions are IGNORED.
int cg_shifted(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
               const double* b, double* X, int64_t ldx, const double* shifts,
               int ns, int kmax, double rtol,
               std::vector<int>* iterations = nullptr,
               std::vector<double>* rnorm_history = nullptr,
               int* status = nullptr, const CgOptions* options = nullptr,
               CgStats* stats = nullptr,
               CgShiftedWorkspace* workspace = nullptr);

// ---- IDR(s) ---------------------------------------------------------------------

struct IdrsOptions {
  int poll_every = 16;    // host looks at the device's `done` flag this often
  bool time_spmv = false; // bracket every Matrix::mult of the recurrence
  uint64_t seed = 0;      // of the shadow signs
  double kappa = 0.7;     // the om step is lengthened where |rho| < kappa
};

// Work vectors + device scalars of idrs(), kept across calls like
// GmresWorkspace; it regrows itself when a call needs more rows, a larger s or
// more iterations, and is usable after every exit.  Owns the ChebyshevWorkspace
// of a Chebyshev preconditioner.
class IdrsWorkspace : public SolverWorkspace
{
public:
  explicit IdrsWorkspace(HipExecutor& exec);
  ~IdrsWorkspace();

  // ---- internal to idrs() ----
  // need_v: a stored preconditioner (sgs / ILU(0) / amg / Chebyshev) reads v;
  // need_dinv: Chebyshev's dinv is not 16-byte aligned
  void ensure(int64_t M, int64_t N_padded, int s, int kmax, bool need_v,
              bool need_dinv);
  void release();

  spmv_hip_idrs_ws* ws = nullptr;
  ChebyshevWorkspace cheb;
  int kmax_cap = -1;
  int64_t m_cap = -1, n_cap = -1, gu_cap = -1, v_cap = -1, dinv_cap = -1;
  int64_t ld = 0;          // stride of G and U: M rounded up to an even number
  double *r = nullptr, *t = nullptr; // m_cap (t: g, then A vh)
  double* u = nullptr;     // n_cap: the padded u / vh the SpMV reads
  double *G = nullptr, *U = nullptr; // gu_cap = s * ld each
  double* v = nullptr;     // v_cap: what a stored preconditioner reads
  double* dinv = nullptr;  // dinv_cap: the copy of an unaligned dinv
  // flags: {done, kstop, status, k}; timing_ev: 2 events per product
};

// the argument rules of idrs() that need no device (idrs_check_rules of
// solver_args.h on the fields of M and the options)
void idrs_check_arguments(const GmresPreconditioner* M, int s, int kmax,
                          double kappa, int64_t rows, const double* b,
                          const double* x);

// IDR(s) (Sonneveld and van Gijzen; the biortho variant of 2011) from x0 = 0
// with a RIGHT preconditioner B^-1 (GmresPreconditioner: none, dinv*,
// chebyshev_apply, sgs_apply / ILU(0) or amg_apply), for a matrix that need not
// be symmetric: short recurrences, ONE product per step, 2 s + 4 vectors
// whatever the iteration count.  IDR(1) is mathematically BiCGStab; s = 4 or 8
// is markedly more robust on convection-dominated systems.  Only Matrix::mult
// and col_map()->update are used: every plan form, both storages and every halo
// model serve.  1 <= s <= 8.
//
// Shadow space.  P has s columns of random SIGNS: with gi the global index of a
// row, in uint64 arithmetic with wraparound,
//     z = gi + seed*0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15
//     z = (z ^ z>>30) * 0xBF58476D1CE4E5B9
//     z = (z ^ z>>27) * 0x94D049BB133111EB
//     z ^= z>>31
//     p_j(i) = +1.0 if bit j of z is clear, else -1.0
// P is never stored and never streamed; p_j . w adds w_i or -w_i; the signs
// depend on the global row alone, so a partition changes only the summation
// order.
//
// With `.` the deterministic two-stage dot product, M the s x s lower
// triangular scalar matrix, every product, sum, difference, quotient and square
// root one rounding of its own:
//
//   x = 0; r = b; G = U = 0 (n x s); M = I; om = 1; k = 0; status = 0
//   f = P^T r; rr = r.r; hist[0] = sqrt(rr);   rr == 0: return 0
//   cycle:
//     for q = 0..s-1:
//       c_i, i = q..s-1 in order: t = f_i; for j = q..i-1: t = t - M[i][j]*c_j;
//                                 c_i = t / M[i][i]
//       v  = r - c_q g_q - ... - c_{s-1} g_{s-1}            (in that order)
//       u  = om*(B^-1 v) + c_q u_q + ... + c_{s-1} u_{s-1}  (in that order)
//       g  = A u                                            (halo update first)
//       h  = P^T g                      (ONE launch, s sums; one all-reduce of s)
//       a_i, i = 0..q-1 in order: t = h_i; for j < i: t = t - a_j*M[i][j];
//                                 a_i = t / M[i][i]
//       g_q = g - a_0 g_0 - ...;  u_q = u - a_0 u_0 - ...
//       M[i][q], i = q..s-1: t = h_i; for j < q: t = t - a_j*M[i][j]; M[i][q] = t
//       M[q][q] is zero or not finite: status = 1, stop (nothing of this step
//                                      is written to x, r, G, U)
//       be = f_q / M[q][q]; r = r - be*g_q; x = x + be*u_q; rr = r.r; k += 1;
//       hist[k] = sqrt(rr)
//       hist[k]/hist[0] < rtol or k == kmax: stop
//       f_i = f_i - be*M[i][q], i = q+1..s-1
//     vh = B^-1 r; t = A vh; tr = t.r; tt = t.t
//     not (tt > 0): status = 2, stop
//     om = tr/tt; rho = tr/(sqrt(tt)*sqrt(rr));
//     |rho| < kappa: om = om*kappa/|rho|
//     om is zero or not finite: status = 2, stop
//     r = r - om*t; x = x + om*vh; rr = r.r; f = P^T r; k += 1;
//     hist[k] = sqrt(rr); the same stop test
//
// The biorthogonalisation is the one-synchronisation form: one multi-dot of the
// un-orthogonalised g yields every a_i and the new column of M by scalar
// arithmetic on the device, because p_i . g_j = M[i][j] is already known.  A
// non-finite scalar takes the "go on" branch of the rtol test, but that test is
// not the first one a NaN meets.  In the kernels' order: step(start) writes
// hist[0] and tests rr == 0 (false on a NaN); biortho of inner step 0 then
// tests "M[0][0] is zero or not finite", which a NaN or Inf in b, A or dinv
// makes true through h = P^T (A u): such a solve ends at k = 0 with status 1
// and x = 0, before any rtol test is reached.  Only a solve whose pivots and om
// stay finite while rr overflows (hist[k] / hist[0] = Inf / Inf) goes on.
// omega tests not (tt > 0) first; where tt > 0 and t.r == 0 (a skew-symmetric
// A) om = 0 and rho = 0, the kappa rule makes om = 0 * kappa / 0 a NaN, and it
// is "not finite" that ends the solve.  A stop at kmax wins over a breakdown
// that only the next step would find.
//
// Non-finite and extreme data.  A NaN or Inf in b, a NaN in A, a NaN or Inf in
// dinv: k = 0, status 1, x = 0 (hist[0] is NaN, Inf or finite).  A b whose b.b
// overflows (1e200): the s inner steps run on finite sums with hist = Inf, the
// om step finds tt = Inf and om = 0: k = s, status 2, x finite.  A b whose b.b
// underflows to 0 (1e-200): k = 0, status 0, x = 0 although b != 0.
//
// Scaling.  (2^s A, 2^t b), with a B^-1 that scales by 2^-s (dinv 2^-s;
// Chebyshev with the same bounds; SGS, ILU(0), AMG built from the scaled
// matrix), repeats the solve of (A, b) bit for bit, x times 2^(t-s) and the
// history times 2^t, at odd s + t too; so do (A, -b) and, with dinv left
// alone, (-A, b), with -x.  With such a B^-1 no s has a floor.  Without one tt
// = t.t carries 2^(2(s+t)): beyond |s + t| of about 510 it overflows (om = 0:
// status 2 at the first om step on a regular system) or underflows to 0 (not
// (tt > 0): the same exit); a solve that ends inside its first cycle never
// forms tt and has no floor.
// Returns k, the
// products completed; x is exactly the iterate of that k; rnorm_history
// receives hist[0..k] (the recurrence's residual norms); `status` (optional)
// 0 at rtol or kmax, 1 on a zero pivot of M, 2 on a zero or non-finite om.
//
// Launches of an inner step on one rank, beside the product: prep, sign_dot,
// biortho, update, step -- 5 launches and 2 s + 11 vector passes with no
// preconditioner (dinv: one more; a stored preconditioner: prep twice and its
// own kernels).  An om step: prep, omega_dot, omega, omega_update, step -- 5
// launches, 10 passes.  With several ranks a reducer launch and an all-reduce
// follow each multi-dot: s and 1 doubles per inner step, 2 and s + 1 per om
// step.  The scalars, M, f, the history and k never leave the device inside the
// loop; the host polls a pinned flag every `poll_every` steps, and kernels
// enqueued after `done` return at once.  `x` IS the iterate (zeroed at the
// start, updated in place, at any 8-byte alignment).  x must not overlap b or
// dinv ("overlaps"); the argument rules are idrs_check_rules' (solver_args.h:
// "s", "kmax", "kappa", "preconditioner", "rows", "overlaps"), checked before
// anything touches a device; the executor's stream is restored on every exit
// path.
//
// options: poll_every, time_spmv (one timed Matrix::mult per step: spmv_launches
//          is the number of steps enqueued), seed and kappa.
int idrs(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
         const double* b, double* x, const GmresPreconditioner* M, int s,
         int kmax, double rtol, std::vector<double>* rnorm_history = nullptr,
         const IdrsOptions* options = nullptr, CgStats* stats = nullptr,
         IdrsWorkspace* workspace = nullptr, int* status = nullptr);

} // namespace spmv
