// The frame every solver of cg.h stands in (internal to cg.cpp, pcg.cpp and
// bicgstab.cpp): argument checks, the switch to the solve's stream, the host's
// lagging look at the device's `done` flag, and the read-back at the end.
// Plain inline functions and small structs: nothing here allocates or makes an
// indirect call inside an iteration loop.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "cg.h"
#include "spmv_hip.h"

namespace spmv
{
namespace detail
{

// the streaming kernels load 16 bytes at a time
inline bool is_aligned16(const void* q)
{
  return (reinterpret_cast<uintptr_t>(q) & 15u) == 0;
}

// u[0:M] and v[0:M] share a byte
inline bool ranges_overlap(const double* u, const double* v, int64_t M)
{
  const uintptr_t ub = reinterpret_cast<uintptr_t>(u);
  const uintptr_t vb = reinterpret_cast<uintptr_t>(v);
  const uintptr_t bytes = (uintptr_t)M * sizeof(double);
  return M > 0 && ub < vb + bytes && vb < ub + bytes;
}

struct Dims {
  int64_t M;        // rows of this rank
  int64_t N_padded; // local columns + ghosts: what an SpMV reads
  std::shared_ptr<const L2GMap> col_l2g;
};

// cg.cpp:32-33 and the kmax rule of cg.h, for spmv::<who>
inline Dims check_problem(const char* who, const Matrix<double>& A, int kmax)
{
  std::shared_ptr<const L2GMap> col_l2g = A.col_map();
  std::shared_ptr<const L2GMap> row_l2g = A.row_map();
  if (row_l2g->num_ghosts() > 0)
    throw std::runtime_error(std::string("spmv::") + who
                             + " - Error: A.row_map() has ghost entries");
  if (kmax < 0)
    throw std::runtime_error(std::string("spmv::") + who + " - Error: kmax < 0");
  return {row_l2g->local_size(),
          col_l2g->local_size() + col_l2g->num_ghosts(), col_l2g};
}

inline int dot_partials_len(spmv_hip_ctx* ctx)
{
  int len = 0;
  throw_on_error(spmv_hip_dot_partials_len(ctx, &len),
                 "spmv_hip_dot_partials_len");
  return len;
}

// Orders the solve's stream after whatever the caller enqueued on the
// executor's current one (b may still be in flight) and makes it the stream of
// every launch; restores the executor's stream when the solve leaves, also on
// exceptions.
struct SolveStream {
  HipExecutor& exec;
  void* const prev;
  SolveStream(HipExecutor& e, void* solve_stream) : exec(e), prev(e.get_stream())
  {
    void* ev = exec.create_event();
    exec.record_event(ev, prev);
    exec.stream_wait_event(solve_stream, ev);
    exec.destroy_event(ev);
    exec.set_stream(solve_stream);
  }
  ~SolveStream()
  {
    try {
      exec.set_stream(prev);
    } catch (...) {
    }
  }
  SolveStream(const SolveStream&) = delete;
  SolveStream& operator=(const SolveStream&) = delete;
};

// z (padded) = M^-1 src for the right preconditioners of gmres() and idrs() that
// run kernels of their own: Chebyshev (cheb_dinv: null or 16-byte aligned), sgs
// / ILU(0), amg.  False, and nothing done, where `pre` names none of them (no
// preconditioner, or dinv alone, which each solver applies in its own kernels).
inline bool apply_stored_preconditioner(HipExecutor& exec,
                                        const Matrix<double>& A,
                                        const GmresPreconditioner& pre,
                                        const double* cheb_dinv,
                                        ChebyshevWorkspace* cheb_ws,
                                        const double* src, double* z)
{
  if (pre.cheb_degree >= 1)
    chebyshev_apply(exec, A, src, z, cheb_dinv, pre.cheb_degree, pre.lmin,
                    pre.lmax, cheb_ws);
  else if (pre.sgs)
    sgs_apply(exec, *pre.sgs, src, z);
  else if (pre.amg)
    amg_apply(exec, *pre.amg, src, z);
  else
    return false;
  return true;
}

// The device address of one scalar slot of a solver's workspace (for the
// all-reduce): `get` is its spmv_hip_*_ws_<name> getter.
template <class Ws>
double* ws_slot(Ws* ws, int (*get)(Ws*, int, double**), int k, const char* what)
{
  double* q = nullptr;
  throw_on_error(get(ws, k, &q), what);
  return q;
}

// ... and of one array of its state: `get` is its spmv_hip_*_ws_array.
template <class Ws>
double* ws_array(Ws* ws, int (*get)(Ws*, int, double**, int64_t*), int which,
                 const char* what)
{
  double* q = nullptr;
  throw_on_error(get(ws, which, &q, nullptr), what);
  return q;
}

// The `read` of LaggingPoll::step and read_history from a solver's
// spmv_hip_*_ws_read_async: the state words into `flags`, and the history into
// h[0:n] unless h is null.
template <class Ws>
auto ws_reader(Ws* ws, int32_t* flags,
               int (*read_async)(Ws*, int32_t*, double*, size_t, void*),
               const char* what)
{
  return [=](double* h, size_t n) {
    throw_on_error(read_async(ws, flags, h, n, nullptr), what);
  };
}

// The lifetime of a workspace's device scalars, `ws` with its capacity
// `kmax_cap`.  regrow_scalars: when `stale` (kmax > kmax_cap, or a block width
// that changed) they are destroyed and `create(&ws)` makes them anew for kmax
// iterations -- an earlier solve on the workspace has been synchronised, so
// nothing still reads the old ones.  While they are gone ws is null and
// kmax_cap -1, also when create throws.  drop_scalars: what a release() does.
template <class Ws>
void drop_scalars(Ws*& ws, int& kmax_cap, int (*destroy)(Ws*))
{
  destroy(ws);
  ws = nullptr;
  kmax_cap = -1;
}

template <class Ws, class Create>
void regrow_scalars(Ws*& ws, int& kmax_cap, int kmax, bool stale,
                    int (*destroy)(Ws*), Create&& create, const char* what)
{
  if (!stale)
    return;
  drop_scalars(ws, kmax_cap, destroy);
  throw_on_error(create(&ws), what);
  kmax_cap = kmax;
}

// Lagging look at the flag: every `poll_every` iterations wait for the copy
// issued `poll_every` iterations ago (bounds the host's run-ahead, never drains
// the queue), then issue the next one.  `read(nullptr, 0)` is the solver's
// spmv_hip_*_ws_read_async of the state words alone, into w.flags.
struct LaggingPoll {
  HipExecutor& exec;
  const SolverWorkspace& w;
  const int poll_every, kmax;
  bool poll_pending = false;
  bool stopped = false;
  LaggingPoll(HipExecutor& e, const SolverWorkspace& ws, int every, int kmax_)
      : exec(e), w(ws), poll_every(every < 1 ? 1 : every), kmax(kmax_)
  {
  }
  template <class Read>
  void step(int k, Read&& read)
  {
    if (k % poll_every == 0 && k < kmax) {
      if (poll_pending) {
        exec.synchronize_event(w.poll_event);
        stopped = w.flags[0] != 0;
      }
      if (!stopped) {
        read(nullptr, 0);
        exec.record_event(w.poll_event, w.stream);
        poll_pending = true;
      }
    }
  }
};

// Final state: the state words and the history of `width` doubles per
// iteration.  The device history has the WORKSPACE's capacity, which an earlier
// solve with a larger kmax may have set: the copy is that long, and the C ABI
// refuses a shorter destination.
template <class Ws, class Read>
std::vector<double> read_history(int (*capacity)(const Ws*, int*), const Ws* ws,
                                 int kmax, size_t width, Read&& read)
{
  int cap = 0;
  throw_on_error(capacity(ws, &cap), "spmv_hip ws_capacity");
  std::vector<double> hist(((size_t)std::max(kmax, cap) + 1) * width, 0.0);
  read(hist.data(), hist.size());
  return hist;
}

// CgOptions::time_spmv: adds the durations of the first n_events / 2 event
// pairs to `stats` (after the solve's stream has been synchronised)
inline void sum_spmv_times(spmv_hip_ctx* ctx, const std::vector<void*>& ev,
                           size_t n_events, CgStats& stats)
{
  for (size_t i = 0; i + 1 < n_events; i += 2) {
    float ms = 0.f;
    throw_on_error(spmv_hip_event_elapsed_ms(ctx, ev[i], ev[i + 1], &ms),
                   "spmv_hip_event_elapsed_ms");
    stats.spmv_ms_total += ms;
    ++stats.spmv_launches;
  }
}

// `done` is raised on the device by the NEXT iteration; when the loop ends
// first, the same test (cg.cpp:80) is applied to the history on the host:
// the first j in 1..k with ||r_j|| / ||r_0|| < rtol, or k.  rr_at(j) = r_j.r_j.
template <class RrAt>
int first_k_below(RrAt&& rr_at, int k, double rtol)
{
  const double rnorm0 = std::sqrt(rr_at(0));
  for (int j = 1; j <= k; ++j)
    if (std::sqrt(rr_at(j)) / rnorm0 < rtol)
      return j;
  return k;
}

// rnorm_history (optional) = ||r_0||, ..., ||r_k_final||
template <class RrAt>
void write_history(std::vector<double>* rnorm_history, int k_final,
                   RrAt&& rr_at)
{
  if (!rnorm_history)
    return;
  rnorm_history->resize(k_final + 1);
  for (int j = 0; j <= k_final; ++j)
    (*rnorm_history)[j] = std::sqrt(rr_at(j));
}

} // namespace detail
} // namespace spmv
