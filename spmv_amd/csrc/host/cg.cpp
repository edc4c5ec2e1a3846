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

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <utility>

#include "spmv_hip.h"

namespace spmv
{

// ---------------------------------------------------------------------------
CgWorkspace::~CgWorkspace() { release(); }

void CgWorkspace::release()
{
  try {
    if (stream)
      _exec.synchronize_stream(stream);
    _exec.destroy_event(poll_event);
    for (void* e : timing_ev)
      _exec.destroy_event(e);
    if (stream)
      _exec.destroy_stream(stream);
    spmv_hip_cg_ws_destroy(ws);
    _exec.free(r);
    _exec.free(Ap);
    _exec.free(x);
    _exec.free(p);
    _exec.free(p2);
    _exec.free(dot2);
    spmv_hip_host_free(_exec.context(), flags);
  } catch (...) {
  }
  timing_ev.clear();
  ws = nullptr;
  r = Ap = x = p = p2 = dot2 = nullptr;
  flags = nullptr;
  stream = poll_event = nullptr;
  kmax_cap = -1;
  m_cap = n_cap = -1;
}

void CgWorkspace::ensure(int64_t M, int64_t N_padded, int kmax, int len)
{
  spmv_hip_ctx* ctx = _exec.context();
  if (!stream) {
    stream = _exec.create_stream();
    poll_event = _exec.create_event();
    void* mem = nullptr;
    throw_on_error(spmv_hip_host_alloc(ctx, 2 * sizeof(int32_t), &mem),
                   "spmv_hip_host_alloc");
    flags = static_cast<int32_t*>(mem);
    dot2 = _exec.alloc<double>(len);
  }
  if (kmax > kmax_cap) {
    spmv_hip_cg_ws_destroy(ws);
    ws = nullptr;
    throw_on_error(spmv_hip_cg_ws_create(ctx, kmax, &ws),
                   "spmv_hip_cg_ws_create");
    kmax_cap = kmax;
  }
  if (M > m_cap) {
    _exec.free(r);
    _exec.free(Ap);
    r = _exec.alloc<double>(M); // cg.cpp:39-40
    Ap = _exec.alloc<double>(M);
    m_cap = M;
  }
  if (N_padded > n_cap) {
    _exec.free(x);
    _exec.free(p);
    _exec.free(p2);
    p2 = nullptr; // ensure_p2() brings it back at the new size
    x = _exec.alloc<double>(N_padded); // cg.cpp:41-42
    p = _exec.alloc<double>(N_padded);
    n_cap = N_padded;
  }
}

void CgWorkspace::ensure_p2()
{
  if (!p2 && n_cap > 0)
    p2 = _exec.alloc<double>(n_cap);
}

void CgWorkspace::reserve_timing(int iterations)
{
  while (timing_ev.size() < 2 * (size_t)(iterations < 0 ? 0 : iterations))
    timing_ev.push_back(_exec.create_event(true));
}

namespace
{
// restores the executor's stream when cg() leaves, also on exceptions
struct StreamGuard {
  HipExecutor& exec;
  void* prev;
  ~StreamGuard()
  {
    try {
      exec.set_stream(prev);
    } catch (...) {
    }
  }
};

} // namespace

int cg(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
       const double* b, double* x, int kmax, double rtol,
       std::vector<double>* rnorm_history, const CgOptions* options,
       CgStats* stats, CgWorkspace* workspace)
{
  std::shared_ptr<const L2GMap> col_l2g = A.col_map();
  std::shared_ptr<const L2GMap> row_l2g = A.row_map();
  if (row_l2g->num_ghosts() > 0) // cg.cpp:32-33
    throw std::runtime_error("spmv::cg - Error: A.row_map() has ghost entries");
  if (kmax < 0)
    throw std::runtime_error("spmv::cg - Error: kmax < 0");
  const CgOptions opt = options ? *options : CgOptions();
  const int poll_every = opt.poll_every < 1 ? 1 : opt.poll_every;

  const int64_t M = row_l2g->local_size();
  const int64_t N_padded = col_l2g->local_size() + col_l2g->num_ghosts();
  spmv_hip_ctx* ctx = exec.context();
  int len = 0;
  throw_on_error(spmv_hip_dot_partials_len(ctx, &len),
                 "spmv_hip_dot_partials_len");

  { // x is the iterate from the first kernel on (cg.h): it cannot share b
    const uintptr_t xb = reinterpret_cast<uintptr_t>(x),
                    bb = reinterpret_cast<uintptr_t>(b);
    const uintptr_t bytes = (uintptr_t)M * sizeof(double);
    if (M > 0 && xb < bb + bytes && bb < xb + bytes)
      throw std::runtime_error("cg: x overlaps b (x is updated in place)");
  }
  CgWorkspace own(exec);
  CgWorkspace& w = workspace ? *workspace : own;
  w.ensure(M, N_padded, kmax, len);

  StreamGuard guard{exec, exec.get_stream()};
  { // order after whatever the caller enqueued (b may still be in flight)
    void* ev = exec.create_event();
    exec.record_event(ev, guard.prev);
    exec.stream_wait_event(w.stream, ev);
    exec.destroy_event(ev);
  }
  exec.set_stream(w.stream); // every launch below goes to this stream

  throw_on_error(spmv_hip_cg_ws_reset(w.ws, rtol, nullptr),
                 "spmv_hip_cg_ws_reset");
  double* partials = nullptr;
  throw_on_error(spmv_hip_cg_ws_partials(w.ws, &partials),
                 "spmv_hip_cg_ws_partials");

  // The iterate lives in the caller's x (no copy at the end, cg.cpp:89) unless
  // the mixed mode needs its halo (then in the padded work vector).
  const bool mixed = opt.mixed && A.enable_mixed();
  const bool x_aligned = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
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

  auto slot = [&](bool rr, int k) {
    double* s = nullptr;
    throw_on_error(rr ? spmv_hip_cg_ws_rr(w.ws, k, &s)
                      : spmv_hip_cg_ws_pAp(w.ws, k, &s),
                   "spmv_hip_cg_ws slot");
    return s;
  };

  // rnorm0 (cg.cpp:47-50)
  throw_on_error(spmv_hip_cg_reduce_rr(ctx, w.ws, 0, nullptr),
                 "spmv_hip_cg_reduce_rr");
  comm.reduce_sum(slot(true, 0), 1, w.stream);

  const bool consume = opt.consumer_reductions && comm.size() == 1;
  // whatever happens below, leave the matrix in fp64 mode
  struct MixedGuard {
    const Matrix<double>& A;
    ~MixedGuard() { A.use_mixed(false); }
  } mixed_guard{A};
  int replacements = 0;
  // Timing events live in the workspace: a solve that reuses one (the
  // benchmark, after its warm-up) creates nothing inside its timed region.
  std::vector<void*>& timing_ev = w.timing_ev;
  if (opt.time_spmv)
    w.reserve_timing(kmax);
  int k = 0;
  bool stopped = false;
  bool poll_pending = false;
  while (k < kmax && !stopped) { // cg.cpp:55
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
      comm.reduce_sum(slot(false, k), 1, w.stream);
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
      comm.reduce_sum(slot(true, k), 1, w.stream);
      throw_on_error(spmv_hip_cg_update_p_f64(ctx, w.ws, k, M, w.r, w.p,
                                              nullptr),
                     "spmv_hip_cg_update_p_f64");
      ++replacements;
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
      comm.reduce_sum(slot(false, k), 1, w.stream); // cg.cpp:65
      // r -= alpha Ap with the r.r partials (cg.cpp:66,70,73); the x update
      // of :69 rides with the p update below so p is read once per iteration
      throw_on_error(spmv_hip_cg_update_r_f64(ctx, w.ws, k, M, w.Ap, w.r,
                                              nullptr),
                     "spmv_hip_cg_update_r_f64");
      throw_on_error(spmv_hip_cg_reduce_rr(ctx, w.ws, k, nullptr),
                     "spmv_hip_cg_reduce_rr");
    }
    if (!consume && !replace) {
      comm.reduce_sum(slot(true, k), 1, w.stream); // cg.cpp:75
      // x += alpha p ; stop test ; p = beta p + r   (cg.cpp:69,77-85)
      throw_on_error(spmv_hip_cg_update_xp_f64(ctx, w.ws, k, M, w.r, xi, w.p,
                                               nullptr),
                     "spmv_hip_cg_update_xp_f64");
    }

    if (k % poll_every == 0 && k < kmax) {
      // Lagging look at the flag: wait for the copy issued `poll_every`
      // iterations ago (bounds the host's run-ahead, never drains the queue),
      // then issue the next one.
      if (poll_pending) {
        exec.synchronize_event(w.poll_event);
        stopped = w.flags[0] != 0;
      }
      if (!stopped) {
        throw_on_error(spmv_hip_cg_ws_read_async(w.ws, w.flags, nullptr, 0,
                                                 nullptr),
                       "spmv_hip_cg_ws_read_async");
        exec.record_event(w.poll_event, w.stream);
        poll_pending = true;
      }
    }
  }

  // The loop ended on a P step: its x update is still pending (the kernel
  // does nothing if the solve has stopped or iteration k met the tolerance).
  if (defer && (k & 1))
    throw_on_error(spmv_hip_cg_flush_x_f64(ctx, w.ws, k, M, pbuf[0], xi,
                                           nullptr),
                   "spmv_hip_cg_flush_x_f64");

  // final state: {done, kstop} and the squared-residual history
  // (the device history has the WORKSPACE's capacity, which an earlier solve
  // with a larger kmax may have set: the copy is that long, and the C ABI
  // refuses a shorter destination)
  int cap = 0;
  throw_on_error(spmv_hip_cg_ws_capacity(w.ws, &cap), "spmv_hip_cg_ws_capacity");
  std::vector<double> rr((size_t)std::max(kmax, cap) + 1, 0.0);
  throw_on_error(spmv_hip_cg_ws_read_async(w.ws, w.flags, rr.data(), rr.size(),
                                           nullptr),
                 "spmv_hip_cg_ws_read_async");
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
    for (size_t i = 0; opt.time_spmv && i + 1 < 2 * (size_t)k; i += 2) {
      float ms = 0.f;
      throw_on_error(spmv_hip_event_elapsed_ms(ctx, timing_ev[i],
                                               timing_ev[i + 1], &ms),
                     "spmv_hip_event_elapsed_ms");
      stats->spmv_ms_total += ms;
      ++stats->spmv_launches;
    }
  }

  int k_final = k;
  if (w.flags[0] != 0) {
    k_final = w.flags[1];
  } else {
    // `done` is raised by the p.Ap reducer of the NEXT iteration; when the
    // loop ends first, apply the same test (cg.cpp:80) to the history on the
    // host.  Either way the value returned is the reference's k.
    const double rnorm0 = std::sqrt(rr[0]);
    for (int j = 1; j <= k; ++j)
      if (std::sqrt(rr[j]) / rnorm0 < rtol) {
        k_final = j;
        break;
      }
  }
  if (rnorm_history) {
    rnorm_history->resize(k_final + 1);
    for (int j = 0; j <= k_final; ++j)
      (*rnorm_history)[j] = std::sqrt(rr[j]);
  }
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
      (void)replacements;
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
  try {
    if (stream)
      _exec.synchronize_stream(stream);
    _exec.destroy_event(poll_event);
    for (void* e : timing_ev)
      _exec.destroy_event(e);
    if (stream)
      _exec.destroy_stream(stream);
    spmv_hip_cgb_ws_destroy(ws);
    _exec.free(r);
    _exec.free(Ap);
    _exec.free(x);
    _exec.free(p);
    spmv_hip_host_free(_exec.context(), state);
  } catch (...) {
  }
  timing_ev.clear();
  ws = nullptr;
  r = Ap = x = p = nullptr;
  state = nullptr;
  stream = poll_event = nullptr;
  kmax_cap = -1;
  nrhs_cap = 0;
  m_cap = n_cap = x_cap = -1;
}

void CgBlockWorkspace::ensure(int64_t m_elems, int64_t n_elems, int kmax,
                              int nrhs, bool need_x)
{
  spmv_hip_ctx* ctx = _exec.context();
  if (!stream) {
    stream = _exec.create_stream();
    poll_event = _exec.create_event();
    void* mem = nullptr;
    throw_on_error(spmv_hip_host_alloc(
                       ctx, SPMV_HIP_CGB_STATE_WORDS * sizeof(int32_t), &mem),
                   "spmv_hip_host_alloc");
    state = static_cast<int32_t*>(mem);
  }
  if (kmax > kmax_cap || nrhs != nrhs_cap) {
    // (an earlier solve on this workspace has been synchronised: nothing
    // still reads the old scalars)
    spmv_hip_cgb_ws_destroy(ws);
    ws = nullptr;
    kmax_cap = -1;
    nrhs_cap = 0;
    throw_on_error(spmv_hip_cgb_ws_create(ctx, kmax, nrhs, &ws),
                   "spmv_hip_cgb_ws_create");
    kmax_cap = kmax;
    nrhs_cap = nrhs;
  }
  if (m_elems > m_cap) {
    _exec.free(r);
    _exec.free(Ap);
    r = Ap = nullptr;
    m_cap = -1;
    r = _exec.alloc<double>(m_elems);
    Ap = _exec.alloc<double>(m_elems);
    m_cap = m_elems;
  }
  if (need_x && m_elems > x_cap) {
    _exec.free(x);
    x = nullptr;
    x_cap = -1;
    x = _exec.alloc<double>(m_elems);
    x_cap = m_elems;
  }
  if (n_elems > n_cap) {
    _exec.free(p);
    p = nullptr;
    n_cap = -1;
    p = _exec.alloc<double>(n_elems);
    n_cap = n_elems;
  }
}

void CgBlockWorkspace::reserve_timing(int iterations)
{
  while (timing_ev.size() < 2 * (size_t)(iterations < 0 ? 0 : iterations))
    timing_ev.push_back(_exec.create_event(true));
}

int cg_block(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
             const double* B, double* X, int nrhs, int kmax, double rtol,
             std::vector<int>* iterations, std::vector<double>* rnorm_history,
             const CgOptions* options, CgStats* stats,
             CgBlockWorkspace* workspace)
{
  std::shared_ptr<const L2GMap> col_l2g = A.col_map();
  std::shared_ptr<const L2GMap> row_l2g = A.row_map();
  if (row_l2g->num_ghosts() > 0) // cg.cpp:32-33
    throw std::runtime_error(
        "spmv::cg_block - Error: A.row_map() has ghost entries");
  if (kmax < 0)
    throw std::runtime_error("spmv::cg_block - Error: kmax < 0");
  if (nrhs < 1 || nrhs > SPMV_HIP_CGB_MAX_NRHS)
    throw std::runtime_error("spmv::cg_block - Error: nrhs must be in 1..8");
  const CgOptions opt = options ? *options : CgOptions();
  const int poll_every = opt.poll_every < 1 ? 1 : opt.poll_every;

  const int64_t M = row_l2g->local_size();
  const int64_t N_padded = col_l2g->local_size() + col_l2g->num_ghosts();
  const int64_t m_elems = M * nrhs, n_elems = N_padded * nrhs;
  spmv_hip_ctx* ctx = exec.context();

  { // X is the iterate from the first kernel on (cg.h): it cannot share B
    const uintptr_t xb = reinterpret_cast<uintptr_t>(X),
                    bb = reinterpret_cast<uintptr_t>(B);
    const uintptr_t bytes = (uintptr_t)m_elems * sizeof(double);
    if (M > 0 && xb < bb + bytes && bb < xb + bytes)
      throw std::runtime_error("cg_block: X overlaps B (X is updated in place)");
  }
  CgBlockWorkspace own(exec);
  CgBlockWorkspace& w = workspace ? *workspace : own;
  const bool x_aligned = (reinterpret_cast<uintptr_t>(X) & 15u) == 0;
  w.ensure(m_elems, n_elems, kmax, nrhs, !x_aligned);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  StreamGuard guard{exec, exec.get_stream()};
  { // order after whatever the caller enqueued (B may still be in flight)
    void* ev = exec.create_event();
    exec.record_event(ev, guard.prev);
    exec.stream_wait_event(w.stream, ev);
    exec.destroy_event(ev);
  }
  exec.set_stream(w.stream); // every launch below goes to this stream

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
    w.state[i] = i > SPMV_HIP_CGB_MAX_NRHS ? -1 : 0;

  auto slot = [&](bool rr, int k) {
    double* s = nullptr;
    throw_on_error(rr ? spmv_hip_cgb_ws_rr(w.ws, k, &s)
                      : spmv_hip_cgb_ws_pAp(w.ws, k, &s),
                   "spmv_hip_cgb_ws slot");
    return s;
  };

  // rnorm0 of every column (cg.cpp:47-50)
  throw_on_error(spmv_hip_cgb_reduce_rr(ctx, w.ws, 0, nullptr),
                 "spmv_hip_cgb_reduce_rr");
  comm.reduce_sum(slot(true, 0), nrhs, w.stream);

  std::vector<void*>& timing_ev = w.timing_ev;
  int k = 0;
  bool stopped = false;
  bool poll_pending = false;
  while (k < kmax && !stopped) { // cg.cpp:55
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
    comm.reduce_sum(slot(false, k), nrhs, w.stream); // cg.cpp:65
    throw_on_error(spmv_hip_cgb_update_r_f64(ctx, w.ws, k, M, w.Ap, w.r,
                                             nullptr),
                   "spmv_hip_cgb_update_r_f64"); // cg.cpp:66,70,73
    throw_on_error(spmv_hip_cgb_reduce_rr(ctx, w.ws, k, nullptr),
                   "spmv_hip_cgb_reduce_rr");
    comm.reduce_sum(slot(true, k), nrhs, w.stream); // cg.cpp:75
    throw_on_error(spmv_hip_cgb_update_xp_f64(ctx, w.ws, k, M, w.r, Xi, w.p,
                                              nullptr),
                   "spmv_hip_cgb_update_xp_f64"); // cg.cpp:69,77-85

    if (k % poll_every == 0 && k < kmax) {
      // lagging look at all_done, as cg() looks at its flag
      if (poll_pending) {
        exec.synchronize_event(w.poll_event);
        stopped = w.state[0] != 0;
      }
      if (!stopped) {
        throw_on_error(spmv_hip_cgb_ws_read_async(w.ws, w.state,
                                                  SPMV_HIP_CGB_STATE_WORDS,
                                                  nullptr, 0, nullptr),
                       "spmv_hip_cgb_ws_read_async");
        exec.record_event(w.poll_event, w.stream);
        poll_pending = true;
      }
    }
  }

  // final state and the squared-residual history (the device history has the
  // WORKSPACE's capacity; the C ABI refuses a shorter destination)
  int cap = 0, cap_nrhs = 0;
  throw_on_error(spmv_hip_cgb_ws_capacity(w.ws, &cap, &cap_nrhs),
                 "spmv_hip_cgb_ws_capacity");
  std::vector<double> rr(((size_t)std::max(kmax, cap) + 1) * (size_t)nrhs, 0.0);
  throw_on_error(spmv_hip_cgb_ws_read_async(w.ws, w.state,
                                            SPMV_HIP_CGB_STATE_WORDS, rr.data(),
                                            rr.size(), nullptr),
                 "spmv_hip_cgb_ws_read_async");
  if (Xi != X)
    exec.copy<double>(X, Xi, m_elems);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    for (size_t i = 0; opt.time_spmv && i + 1 < 2 * (size_t)k; i += 2) {
      float ms = 0.f;
      throw_on_error(spmv_hip_event_elapsed_ms(ctx, timing_ev[i],
                                               timing_ev[i + 1], &ms),
                     "spmv_hip_event_elapsed_ms");
      stats->spmv_ms_total += ms;
      ++stats->spmv_launches;
    }
  }

  if (iterations)
    iterations->assign(nrhs, 0);
  if (rnorm_history)
    rnorm_history->assign((size_t)nrhs * ((size_t)kmax + 1), -1.0);
  int k_max = 0;
  for (int c = 0; c < nrhs; ++c) {
    auto rr_at = [&](int j) { return rr[(size_t)j * nrhs + c]; };
    int kc = k;
    if (w.state[1 + c] != 0) {
      kc = w.state[1 + SPMV_HIP_CGB_MAX_NRHS + c];
    } else if (rr_at(0) == 0.0) {
      kc = 0; // (kmax == 0: no reducer ran to say so)
    } else {
      // done[c] is raised by the p.Ap reducer of the NEXT iteration; when the
      // loop ends first, apply the same test (cg.cpp:80) here, as cg() does
      const double rnorm0 = std::sqrt(rr_at(0));
      for (int j = 1; j <= k; ++j)
        if (std::sqrt(rr_at(j)) / rnorm0 < rtol) {
          kc = j;
          break;
        }
    }
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

// ---------------------------------------------------------------------------
// pcg: see cg.h.  Per iteration (compute stream):
//     halo start on the map's side stream
//     SpMV local block (+ fused p.Ap share) [wait halo event] remote block
//     one rank, consumer_reductions:            otherwise:
//       update_r_cs   (pAp[k]; r; r.z, r.r)       reduce_pAp(2) ; all-reduce of 1
//       update_xp_cs  ({rz,rr}[k]; x; p)          update_r
//                                                 reduce_rz_rr ; all-reduce of 2
//                                                 update_xp
// 3 (or 5) launches; beside the SpMV 10 vector passes (update_r: Ap, r, dinv
// in, r out; update_xp: r, dinv, x, p in, x, p out) where cg() without
// defer_x streams 8.
// ---------------------------------------------------------------------------
PcgWorkspace::~PcgWorkspace() { release(); }

void PcgWorkspace::release()
{
  try {
    if (stream)
      _exec.synchronize_stream(stream);
    _exec.destroy_event(poll_event);
    for (void* e : timing_ev)
      _exec.destroy_event(e);
    if (stream)
      _exec.destroy_stream(stream);
    spmv_hip_pcg_ws_destroy(ws);
    _exec.free(r);
    _exec.free(Ap);
    _exec.free(x);
    _exec.free(dinv);
    _exec.free(p);
    _exec.free(dot2);
    spmv_hip_host_free(_exec.context(), flags);
  } catch (...) {
  }
  timing_ev.clear();
  ws = nullptr;
  r = Ap = x = dinv = p = dot2 = nullptr;
  flags = nullptr;
  stream = poll_event = nullptr;
  kmax_cap = -1;
  m_cap = n_cap = x_cap = dinv_cap = -1;
}

void PcgWorkspace::ensure(int64_t M, int64_t N_padded, int kmax, int len,
                          bool need_x, bool need_dinv)
{
  spmv_hip_ctx* ctx = _exec.context();
  if (!stream) {
    stream = _exec.create_stream();
    poll_event = _exec.create_event();
    void* mem = nullptr;
    throw_on_error(spmv_hip_host_alloc(ctx, 2 * sizeof(int32_t), &mem),
                   "spmv_hip_host_alloc");
    flags = static_cast<int32_t*>(mem);
    dot2 = _exec.alloc<double>(len);
  }
  if (kmax > kmax_cap) {
    // (an earlier solve on this workspace has been synchronised: nothing
    // still reads the old scalars)
    spmv_hip_pcg_ws_destroy(ws);
    ws = nullptr;
    kmax_cap = -1;
    throw_on_error(spmv_hip_pcg_ws_create(ctx, kmax, &ws),
                   "spmv_hip_pcg_ws_create");
    kmax_cap = kmax;
  }
  if (M > m_cap) {
    _exec.free(r);
    _exec.free(Ap);
    r = Ap = nullptr;
    m_cap = -1;
    r = _exec.alloc<double>(M);
    Ap = _exec.alloc<double>(M);
    m_cap = M;
  }
  if (need_x && M > x_cap) {
    _exec.free(x);
    x = nullptr;
    x_cap = -1;
    x = _exec.alloc<double>(M);
    x_cap = M;
  }
  if (need_dinv && M > dinv_cap) {
    _exec.free(dinv);
    dinv = nullptr;
    dinv_cap = -1;
    dinv = _exec.alloc<double>(M);
    dinv_cap = M;
  }
  if (N_padded > n_cap) {
    _exec.free(p);
    p = nullptr;
    n_cap = -1;
    p = _exec.alloc<double>(N_padded);
    n_cap = N_padded;
  }
}

void PcgWorkspace::reserve_timing(int iterations)
{
  while (timing_ev.size() < 2 * (size_t)(iterations < 0 ? 0 : iterations))
    timing_ev.push_back(_exec.create_event(true));
}

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
  std::shared_ptr<const L2GMap> col_l2g = A.col_map();
  std::shared_ptr<const L2GMap> row_l2g = A.row_map();
  if (row_l2g->num_ghosts() > 0)
    throw std::runtime_error("spmv::pcg - Error: A.row_map() has ghost entries");
  if (kmax < 0)
    throw std::runtime_error("spmv::pcg - Error: kmax < 0");
  const CgOptions opt = options ? *options : CgOptions();
  const int poll_every = opt.poll_every < 1 ? 1 : opt.poll_every;

  const int64_t M = row_l2g->local_size();
  const int64_t N_padded = col_l2g->local_size() + col_l2g->num_ghosts();
  spmv_hip_ctx* ctx = exec.context();
  int len = 0;
  throw_on_error(spmv_hip_dot_partials_len(ctx, &len),
                 "spmv_hip_dot_partials_len");

  { // x is the iterate from the first kernel on: it cannot share b or dinv
    const uintptr_t xb = reinterpret_cast<uintptr_t>(x);
    const uintptr_t bytes = (uintptr_t)M * sizeof(double);
    auto overlaps = [&](const double* v) {
      const uintptr_t vb = reinterpret_cast<uintptr_t>(v);
      return M > 0 && xb < vb + bytes && vb < xb + bytes;
    };
    if (overlaps(b))
      throw std::runtime_error("pcg: x overlaps b (x is updated in place)");
    if (overlaps(dinv))
      throw std::runtime_error("pcg: x overlaps dinv (x is updated in place)");
  }
  PcgWorkspace own(exec);
  PcgWorkspace& w = workspace ? *workspace : own;
  const bool x_aligned = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
  const bool dinv_aligned = (reinterpret_cast<uintptr_t>(dinv) & 15u) == 0;
  w.ensure(M, N_padded, kmax, len, !x_aligned, !dinv_aligned);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  StreamGuard guard{exec, exec.get_stream()};
  { // order after whatever the caller enqueued (b, dinv may still be in flight)
    void* ev = exec.create_event();
    exec.record_event(ev, guard.prev);
    exec.stream_wait_event(w.stream, ev);
    exec.destroy_event(ev);
  }
  exec.set_stream(w.stream); // every launch below goes to this stream

  throw_on_error(spmv_hip_pcg_ws_reset(w.ws, rtol, nullptr),
                 "spmv_hip_pcg_ws_reset");
  double* partials = nullptr;
  throw_on_error(spmv_hip_pcg_ws_partials(w.ws, &partials),
                 "spmv_hip_pcg_ws_partials");

  double* const xi = x_aligned ? x : w.x;
  const double* di = dinv;
  if (!dinv_aligned) { // the streaming kernels load 16 bytes at a time
    exec.copy<double>(w.dinv, dinv, M);
    di = w.dinv;
  }
  // the ghost tail of p is defined here instead of relying on fresh pages
  if (N_padded > M)
    exec.memset<double>(w.p + M, 0, N_padded - M);
  exec.memset<double>(w.dot2, 0, len);
  // r = b, x0 = 0, p = dinv*b, partials of r.z and r.r: one pass
  throw_on_error(spmv_hip_pcg_init_f64(ctx, w.ws, M, b, di, w.r, w.p, xi,
                                       nullptr),
                 "spmv_hip_pcg_init_f64");
  w.flags[0] = 0;
  w.flags[1] = -1;

  auto pair_slot = [&](int k) {
    double* s = nullptr;
    throw_on_error(spmv_hip_pcg_ws_rz_rr(w.ws, k, &s), "spmv_hip_pcg_ws_rz_rr");
    return s;
  };
  auto pAp_slot = [&](int k) {
    double* s = nullptr;
    throw_on_error(spmv_hip_pcg_ws_pAp(w.ws, k, &s), "spmv_hip_pcg_ws_pAp");
    return s;
  };

  // {rz0, rr0}: one all-reduce of 2 doubles
  throw_on_error(spmv_hip_pcg_reduce_rz_rr(ctx, w.ws, 0, nullptr),
                 "spmv_hip_pcg_reduce_rz_rr");
  comm.reduce_sum(pair_slot(0), 2, w.stream);

  const bool consume = opt.consumer_reductions && comm.size() == 1;
  std::vector<void*>& timing_ev = w.timing_ev;
  int k = 0;
  bool stopped = false;
  bool poll_pending = false;
  while (k < kmax && !stopped) {
    ++k;
    col_l2g->update(w.p); // starts on the side stream
    void* ev1 = nullptr;
    if (opt.time_spmv) {
      ev1 = timing_ev[2 * (size_t)(k - 1) + 1];
      exec.record_event(timing_ev[2 * (size_t)(k - 1)], w.stream);
    }
    // Ap = A p with the p.Ap partials produced by the SpMV kernels themselves
    // (local block's share + remote block's share) where they can
    const bool fused = A.mult_dot(w.p, w.Ap, partials, w.dot2, ev1);
    if (!fused)
      throw_on_error(spmv_hip_dot_partial_f64(ctx, M, w.p, w.Ap, partials,
                                              nullptr),
                     "spmv_hip_dot_partial_f64");
    if (consume) {
      // one rank: the update kernels add the partials themselves
      throw_on_error(spmv_hip_pcg_update_r_cs_f64(ctx, w.ws, k, M, w.Ap, di,
                                                  w.r, fused ? w.dot2 : nullptr,
                                                  nullptr),
                     "spmv_hip_pcg_update_r_cs_f64");
      throw_on_error(spmv_hip_pcg_update_xp_cs_f64(ctx, w.ws, k, M, w.r, di, xi,
                                                   w.p, nullptr),
                     "spmv_hip_pcg_update_xp_cs_f64");
    } else {
      if (fused)
        throw_on_error(spmv_hip_pcg_reduce_pAp2(ctx, w.ws, k, w.dot2, nullptr),
                       "spmv_hip_pcg_reduce_pAp2");
      else
        throw_on_error(spmv_hip_pcg_reduce_pAp(ctx, w.ws, k, nullptr),
                       "spmv_hip_pcg_reduce_pAp");
      comm.reduce_sum(pAp_slot(k), 1, w.stream);
      throw_on_error(spmv_hip_pcg_update_r_f64(ctx, w.ws, k, M, w.Ap, di, w.r,
                                               nullptr),
                     "spmv_hip_pcg_update_r_f64");
      throw_on_error(spmv_hip_pcg_reduce_rz_rr(ctx, w.ws, k, nullptr),
                     "spmv_hip_pcg_reduce_rz_rr");
      comm.reduce_sum(pair_slot(k), 2, w.stream); // rz[k] and rr[k] at once
      throw_on_error(spmv_hip_pcg_update_xp_f64(ctx, w.ws, k, M, w.r, di, xi,
                                                w.p, nullptr),
                     "spmv_hip_pcg_update_xp_f64");
    }

    if (k % poll_every == 0 && k < kmax) {
      // lagging look at the flag, as in cg()
      if (poll_pending) {
        exec.synchronize_event(w.poll_event);
        stopped = w.flags[0] != 0;
      }
      if (!stopped) {
        throw_on_error(spmv_hip_pcg_ws_read_async(w.ws, w.flags, nullptr, 0,
                                                  nullptr),
                       "spmv_hip_pcg_ws_read_async");
        exec.record_event(w.poll_event, w.stream);
        poll_pending = true;
      }
    }
  }

  // final state: {done, kstop} and the history of pairs (it has the
  // WORKSPACE's capacity; the C ABI refuses a shorter destination)
  int cap = 0;
  throw_on_error(spmv_hip_pcg_ws_capacity(w.ws, &cap),
                 "spmv_hip_pcg_ws_capacity");
  std::vector<double> zr(2 * ((size_t)std::max(kmax, cap) + 1), 0.0);
  throw_on_error(spmv_hip_pcg_ws_read_async(w.ws, w.flags, zr.data(), zr.size(),
                                            nullptr),
                 "spmv_hip_pcg_ws_read_async");
  if (xi != x)
    exec.copy<double>(x, xi, M);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    for (size_t i = 0; opt.time_spmv && i + 1 < 2 * (size_t)k; i += 2) {
      float ms = 0.f;
      throw_on_error(spmv_hip_event_elapsed_ms(ctx, timing_ev[i],
                                               timing_ev[i + 1], &ms),
                     "spmv_hip_event_elapsed_ms");
      stats->spmv_ms_total += ms;
      ++stats->spmv_launches;
    }
  }

  auto rr_at = [&](int j) { return zr[2 * (size_t)j + 1]; };
  int k_final = k;
  if (w.flags[0] != 0) {
    k_final = w.flags[1];
  } else if (rr_at(0) == 0.0) {
    k_final = 0; // (kmax == 0: no kernel ran to say so)
  } else {
    // `done` is raised by the first kernel of the NEXT iteration; when the
    // loop ends first, apply the same test to the history here, as cg() does
    const double rnorm0 = std::sqrt(rr_at(0));
    for (int j = 1; j <= k; ++j)
      if (std::sqrt(rr_at(j)) / rnorm0 < rtol) {
        k_final = j;
        break;
      }
  }
  if (rnorm_history) {
    rnorm_history->resize(k_final + 1);
    for (int j = 0; j <= k_final; ++j)
      (*rnorm_history)[j] = std::sqrt(rr_at(j));
  }
  return k_final;
}

// ---------------------------------------------------------------------------
// Chebyshev polynomial preconditioner: see cg.h.  pcg_chebyshev per iteration
// (compute stream), on the scalars and reducers of pcg():
//     halo start of p ; Ap = A p (+ fused p.Ap share)
//     reduce_pAp ; all-reduce of 1
//     cheb_update_r   (r ; partials of r.r ; step 0 of M: d, z)
//     degree - 1 times:  halo start of z ; w = A z ; cheb_step
//                        (the last one: partials of r.z, no d)
//     reduce_rz_rr ; all-reduce of 2
//     cheb_update_xp  (x ; stop test ; p)
// degree SpMVs + degree + 1 streaming launches + 2 reducers; beside the SpMVs
// 7 (degree - 1) + 11 vector passes with a dinv for degree >= 2 (update_r: Ap,
// r, dinv in, r, d, z out; a step: w, r, dinv, d, z in, d, z out, the last one
// without d out; update_xp: z, x, p in, x, p out), 10 for degree 1.
// ---------------------------------------------------------------------------
void chebyshev_coefficients(int degree, double lmin, double lmax, double* a,
                            double* b)
{
  if (degree < 1 || degree > kChebyshevMaxDegree)
    throw std::runtime_error(
        "spmv::chebyshev_coefficients - Error: degree must be 1.."
        + std::to_string(kChebyshevMaxDegree));
  if (!std::isfinite(lmin) || !std::isfinite(lmax) || !(lmin > 0.0)
      || !(lmin < lmax))
    throw std::runtime_error("spmv::chebyshev_coefficients - Error: bounds must "
                             "be finite with 0 < lmin < lmax");
  if (!a || !b)
    throw std::runtime_error("spmv::chebyshev_coefficients - Error: NULL output");
  // (volatile: every operation below is one fp64 rounding, whatever the
  // compiler's contraction setting)
  volatile double theta = 0.5 * (lmax + lmin);
  volatile double delta = 0.5 * (lmax - lmin);
  volatile double sigma = theta / delta;
  volatile double rho = 1.0 / sigma;
  a[0] = 0.0;
  b[0] = 1.0 / theta;
  for (int j = 1; j < degree; ++j) {
    volatile double two_sigma = 2.0 * sigma;
    volatile double den = two_sigma - rho;
    volatile double rho_new = 1.0 / den;
    volatile double aj = rho_new * rho;
    volatile double two_rho = 2.0 * rho_new;
    a[j] = aj;
    b[j] = two_rho / delta;
    rho = rho_new;
  }
}

ChebyshevWorkspace::~ChebyshevWorkspace() { release(); }

void ChebyshevWorkspace::release()
{
  try {
    if (stream)
      _exec.synchronize_stream(stream);
    _exec.destroy_event(poll_event);
    for (void* e : timing_ev)
      _exec.destroy_event(e);
    if (stream)
      _exec.destroy_stream(stream);
    spmv_hip_pcg_ws_destroy(ws);
    _exec.free(r);
    _exec.free(Ap);
    _exec.free(d);
    _exec.free(w);
    _exec.free(p);
    _exec.free(z);
    _exec.free(x);
    _exec.free(dinv);
    _exec.free(dot2);
    spmv_hip_host_free(_exec.context(), flags);
  } catch (...) {
  }
  timing_ev.clear();
  ws = nullptr;
  r = Ap = d = w = p = z = x = dinv = dot2 = nullptr;
  flags = nullptr;
  stream = poll_event = nullptr;
  kmax_cap = -1;
  m_cap = n_cap = x_cap = dinv_cap = -1;
}

void ChebyshevWorkspace::ensure(int64_t M, int64_t N_padded, int kmax, int len,
                                bool need_x, bool need_dinv)
{
  spmv_hip_ctx* ctx = _exec.context();
  if (!stream) {
    stream = _exec.create_stream();
    poll_event = _exec.create_event();
    void* mem = nullptr;
    throw_on_error(spmv_hip_host_alloc(ctx, 2 * sizeof(int32_t), &mem),
                   "spmv_hip_host_alloc");
    flags = static_cast<int32_t*>(mem);
    dot2 = _exec.alloc<double>(len);
  }
  if (kmax > kmax_cap) {
    // (an earlier solve on this workspace has been synchronised: nothing
    // still reads the old scalars)
    spmv_hip_pcg_ws_destroy(ws);
    ws = nullptr;
    kmax_cap = -1;
    throw_on_error(spmv_hip_pcg_ws_create(ctx, kmax, &ws),
                   "spmv_hip_pcg_ws_create");
    kmax_cap = kmax;
  }
  if (M > m_cap) {
    for (double** v : {&r, &Ap, &d, &w}) {
      _exec.free(*v);
      *v = nullptr;
    }
    m_cap = -1;
    for (double** v : {&r, &Ap, &d, &w})
      *v = _exec.alloc<double>(M);
    m_cap = M;
  }
  if (need_x && M > x_cap) {
    _exec.free(x);
    x = nullptr;
    x_cap = -1;
    x = _exec.alloc<double>(M);
    x_cap = M;
  }
  if (need_dinv && M > dinv_cap) {
    _exec.free(dinv);
    dinv = nullptr;
    dinv_cap = -1;
    dinv = _exec.alloc<double>(M);
    dinv_cap = M;
  }
  if (N_padded > n_cap) {
    for (double** v : {&p, &z}) {
      _exec.free(*v);
      *v = nullptr;
    }
    n_cap = -1;
    for (double** v : {&p, &z})
      *v = _exec.alloc<double>(N_padded);
    n_cap = N_padded;
  }
}

void ChebyshevWorkspace::reserve_timing(int spmvs)
{
  while (timing_ev.size() < 2 * (size_t)(spmvs < 0 ? 0 : spmvs))
    timing_ev.push_back(_exec.create_event(true));
}

namespace
{
bool is_aligned16(const void* q)
{
  return (reinterpret_cast<uintptr_t>(q) & 15u) == 0;
}

bool ranges_overlap(const double* u, const double* v, int64_t M)
{
  const uintptr_t ub = reinterpret_cast<uintptr_t>(u);
  const uintptr_t vb = reinterpret_cast<uintptr_t>(v);
  const uintptr_t bytes = (uintptr_t)M * sizeof(double);
  return M > 0 && ub < vb + bytes && vb < ub + bytes;
}
} // namespace

void chebyshev_apply(HipExecutor& exec, const Matrix<double>& A,
                     const double* r, double* z, const double* dinv, int degree,
                     double lmin, double lmax, ChebyshevWorkspace* workspace)
{
  double ca[kChebyshevMaxDegree], cb[kChebyshevMaxDegree];
  chebyshev_coefficients(degree, lmin, lmax, ca, cb);
  std::shared_ptr<const L2GMap> col_l2g = A.col_map();
  std::shared_ptr<const L2GMap> row_l2g = A.row_map();
  if (row_l2g->num_ghosts() > 0)
    throw std::runtime_error(
        "spmv::chebyshev_apply - Error: A.row_map() has ghost entries");
  const int64_t M = row_l2g->local_size();
  const int64_t N_padded = col_l2g->local_size() + col_l2g->num_ghosts();
  if (ranges_overlap(z, r, M))
    throw std::runtime_error("chebyshev_apply: z overlaps r");
  if (dinv && ranges_overlap(z, dinv, M))
    throw std::runtime_error("chebyshev_apply: z overlaps dinv");
  spmv_hip_ctx* ctx = exec.context();
  int len = 0;
  throw_on_error(spmv_hip_dot_partials_len(ctx, &len),
                 "spmv_hip_dot_partials_len");

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
  std::shared_ptr<const L2GMap> col_l2g = A.col_map();
  std::shared_ptr<const L2GMap> row_l2g = A.row_map();
  if (row_l2g->num_ghosts() > 0)
    throw std::runtime_error(
        "spmv::pcg_chebyshev - Error: A.row_map() has ghost entries");
  if (kmax < 0)
    throw std::runtime_error("spmv::pcg_chebyshev - Error: kmax < 0");
  const CgOptions opt = options ? *options : CgOptions();
  const int poll_every = opt.poll_every < 1 ? 1 : opt.poll_every;

  const int64_t M = row_l2g->local_size();
  const int64_t N_padded = col_l2g->local_size() + col_l2g->num_ghosts();
  spmv_hip_ctx* ctx = exec.context();
  int len = 0;
  throw_on_error(spmv_hip_dot_partials_len(ctx, &len),
                 "spmv_hip_dot_partials_len");

  // x is the iterate from the first kernel on: it cannot share b or dinv
  if (ranges_overlap(x, b, M))
    throw std::runtime_error(
        "pcg_chebyshev: x overlaps b (x is updated in place)");
  if (dinv && ranges_overlap(x, dinv, M))
    throw std::runtime_error(
        "pcg_chebyshev: x overlaps dinv (x is updated in place)");

  ChebyshevWorkspace own(exec);
  ChebyshevWorkspace& w = workspace ? *workspace : own;
  const bool x_aligned = is_aligned16(x);
  const bool dinv_aligned = is_aligned16(dinv);
  w.ensure(M, N_padded, kmax, len, !x_aligned, !dinv_aligned);
  if (opt.time_spmv)
    w.reserve_timing(kmax * degree);

  StreamGuard guard{exec, exec.get_stream()};
  { // order after whatever the caller enqueued (b, dinv may still be in flight)
    void* ev = exec.create_event();
    exec.record_event(ev, guard.prev);
    exec.stream_wait_event(w.stream, ev);
    exec.destroy_event(ev);
  }
  exec.set_stream(w.stream); // every launch below goes to this stream

  throw_on_error(spmv_hip_pcg_ws_reset(w.ws, rtol, nullptr),
                 "spmv_hip_pcg_ws_reset");
  double* partials = nullptr;
  throw_on_error(spmv_hip_pcg_ws_partials(w.ws, &partials),
                 "spmv_hip_pcg_ws_partials");

  double* const xi = x_aligned ? x : w.x;
  const double* di = dinv;
  if (dinv && !dinv_aligned) { // the streaming kernels load 16 bytes at a time
    exec.copy<double>(w.dinv, dinv, M);
    di = w.dinv;
  }
  // the ghost tails of p and z are defined here instead of relying on fresh
  // pages
  if (N_padded > M) {
    exec.memset<double>(w.p + M, 0, N_padded - M);
    exec.memset<double>(w.z + M, 0, N_padded - M);
  }
  exec.memset<double>(w.dot2, 0, len);
  double* const dvec = degree > 1 ? w.d : nullptr; // degree 1: no d

  std::vector<void*>& timing_ev = w.timing_ev;
  size_t ev_next = 0; // two events per timed SpMV
  // steps 1 .. degree - 1 of z = M(r); the last one leaves the r.z partials
  auto cheb_steps = [&](bool timed) {
    for (int j = 1; j < degree; ++j) {
      col_l2g->update(w.z); // starts on the side stream
      if (timed)
        exec.record_event(timing_ev[ev_next], w.stream);
      A.mult(w.z, w.w);
      if (timed) {
        exec.record_event(timing_ev[ev_next + 1], w.stream);
        ev_next += 2;
      }
      throw_on_error(spmv_hip_cheb_step_f64(ctx, w.ws, M, ca[j], cb[j],
                                            j == degree - 1, w.w, w.r, di, w.d,
                                            w.z, nullptr),
                     "spmv_hip_cheb_step_f64");
    }
  };

  // r = b, x0 = 0, partials of r.r, step 0 of M: one pass; then the rest of
  // z0 = M(r0) and p1 = z0
  throw_on_error(spmv_hip_cheb_init_f64(ctx, w.ws, M, cb[0], b, di, w.r, xi,
                                        dvec, w.z, nullptr),
                 "spmv_hip_cheb_init_f64");
  cheb_steps(false);
  exec.copy<double>(w.p, w.z, M);
  w.flags[0] = 0;
  w.flags[1] = -1;

  auto pair_slot = [&](int k) {
    double* s = nullptr;
    throw_on_error(spmv_hip_pcg_ws_rz_rr(w.ws, k, &s), "spmv_hip_pcg_ws_rz_rr");
    return s;
  };
  auto pAp_slot = [&](int k) {
    double* s = nullptr;
    throw_on_error(spmv_hip_pcg_ws_pAp(w.ws, k, &s), "spmv_hip_pcg_ws_pAp");
    return s;
  };

  // {rz0, rr0}: one all-reduce of 2 doubles
  throw_on_error(spmv_hip_pcg_reduce_rz_rr(ctx, w.ws, 0, nullptr),
                 "spmv_hip_pcg_reduce_rz_rr");
  comm.reduce_sum(pair_slot(0), 2, w.stream);

  int k = 0;
  bool stopped = false;
  bool poll_pending = false;
  while (k < kmax && !stopped) {
    ++k;
    col_l2g->update(w.p); // starts on the side stream
    void* ev1 = nullptr;
    if (opt.time_spmv) {
      ev1 = timing_ev[ev_next + 1];
      exec.record_event(timing_ev[ev_next], w.stream);
      ev_next += 2;
    }
    // Ap = A p with the p.Ap partials produced by the SpMV kernels themselves
    // (local block's share + remote block's share) where they can
    const bool fused = A.mult_dot(w.p, w.Ap, partials, w.dot2, ev1);
    if (!fused) {
      throw_on_error(spmv_hip_dot_partial_f64(ctx, M, w.p, w.Ap, partials,
                                              nullptr),
                     "spmv_hip_dot_partial_f64");
      throw_on_error(spmv_hip_pcg_reduce_pAp(ctx, w.ws, k, nullptr),
                     "spmv_hip_pcg_reduce_pAp");
    } else {
      throw_on_error(spmv_hip_pcg_reduce_pAp2(ctx, w.ws, k, w.dot2, nullptr),
                     "spmv_hip_pcg_reduce_pAp2");
    }
    comm.reduce_sum(pAp_slot(k), 1, w.stream);
    throw_on_error(spmv_hip_cheb_update_r_f64(ctx, w.ws, k, M, cb[0], w.Ap, di,
                                              w.r, dvec, w.z, nullptr),
                   "spmv_hip_cheb_update_r_f64");
    cheb_steps(opt.time_spmv);
    throw_on_error(spmv_hip_pcg_reduce_rz_rr(ctx, w.ws, k, nullptr),
                   "spmv_hip_pcg_reduce_rz_rr");
    comm.reduce_sum(pair_slot(k), 2, w.stream); // rz[k] and rr[k] at once
    throw_on_error(spmv_hip_cheb_update_xp_f64(ctx, w.ws, k, M, w.z, xi, w.p,
                                               nullptr),
                   "spmv_hip_cheb_update_xp_f64");

    if (k % poll_every == 0 && k < kmax) {
      // lagging look at the flag, as in cg()
      if (poll_pending) {
        exec.synchronize_event(w.poll_event);
        stopped = w.flags[0] != 0;
      }
      if (!stopped) {
        throw_on_error(spmv_hip_pcg_ws_read_async(w.ws, w.flags, nullptr, 0,
                                                  nullptr),
                       "spmv_hip_pcg_ws_read_async");
        exec.record_event(w.poll_event, w.stream);
        poll_pending = true;
      }
    }
  }

  // final state: {done, kstop} and the history of pairs (it has the
  // WORKSPACE's capacity; the C ABI refuses a shorter destination)
  int cap = 0;
  throw_on_error(spmv_hip_pcg_ws_capacity(w.ws, &cap),
                 "spmv_hip_pcg_ws_capacity");
  std::vector<double> zr(2 * ((size_t)std::max(kmax, cap) + 1), 0.0);
  throw_on_error(spmv_hip_pcg_ws_read_async(w.ws, w.flags, zr.data(), zr.size(),
                                            nullptr),
                 "spmv_hip_pcg_ws_read_async");
  if (xi != x)
    exec.copy<double>(x, xi, M);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    for (size_t i = 0; opt.time_spmv && i + 1 < ev_next; i += 2) {
      float ms = 0.f;
      throw_on_error(spmv_hip_event_elapsed_ms(ctx, timing_ev[i],
                                               timing_ev[i + 1], &ms),
                     "spmv_hip_event_elapsed_ms");
      stats->spmv_ms_total += ms;
      ++stats->spmv_launches;
    }
  }

  auto rr_at = [&](int j) { return zr[2 * (size_t)j + 1]; };
  int k_final = k;
  if (w.flags[0] != 0) {
    k_final = w.flags[1];
  } else if (rr_at(0) == 0.0) {
    k_final = 0; // (kmax == 0: no kernel ran to say so)
  } else {
    // `done` is raised by the first reducer of the NEXT iteration; when the
    // loop ends first, apply the same test to the history here, as pcg() does
    const double rnorm0 = std::sqrt(rr_at(0));
    for (int j = 1; j <= k; ++j)
      if (std::sqrt(rr_at(j)) / rnorm0 < rtol) {
        k_final = j;
        break;
      }
  }
  if (rnorm_history) {
    rnorm_history->resize(k_final + 1);
    for (int j = 0; j <= k_final; ++j)
      (*rnorm_history)[j] = std::sqrt(rr_at(j));
  }
  return k_final;
}

double lambda_max_estimate(const Comm& comm, HipExecutor& exec,
                           const Matrix<double>& A, const double* dinv,
                           const double* v0, int steps)
{
  if (steps < 1)
    throw std::runtime_error("spmv::lambda_max_estimate - Error: steps < 1");
  std::shared_ptr<const L2GMap> col_l2g = A.col_map();
  std::shared_ptr<const L2GMap> row_l2g = A.row_map();
  if (row_l2g->num_ghosts() > 0)
    throw std::runtime_error(
        "spmv::lambda_max_estimate - Error: A.row_map() has ghost entries");
  const int64_t M = row_l2g->local_size();
  const int64_t N_padded = col_l2g->local_size() + col_l2g->num_ghosts();
  spmv_hip_ctx* ctx = exec.context();
  int len = 0;
  throw_on_error(spmv_hip_dot_partials_len(ctx, &len),
                 "spmv_hip_dot_partials_len");

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
  try {
    if (stream)
      _exec.synchronize_stream(stream);
    _exec.destroy_event(poll_event);
    for (void* e : timing_ev)
      _exec.destroy_event(e);
    if (stream)
      _exec.destroy_stream(stream);
    spmv_hip_bicg_ws_destroy(ws);
    for (double* q : {r, rhat, v, t, p, s, ph, sh, x, dinv})
      _exec.free(q);
    spmv_hip_host_free(_exec.context(), flags);
  } catch (...) {
  }
  timing_ev.clear();
  ws = nullptr;
  r = rhat = v = t = p = s = ph = sh = x = dinv = nullptr;
  flags = nullptr;
  stream = poll_event = nullptr;
  kmax_cap = -1;
  m_cap = n_cap = h_cap = x_cap = dinv_cap = -1;
}

void BicgstabWorkspace::ensure(int64_t M, int64_t N_padded, int kmax,
                               bool need_x, bool need_dinv, bool need_h)
{
  spmv_hip_ctx* ctx = _exec.context();
  if (!stream) {
    stream = _exec.create_stream();
    poll_event = _exec.create_event();
    void* mem = nullptr;
    throw_on_error(spmv_hip_host_alloc(ctx, 4 * sizeof(int32_t), &mem),
                   "spmv_hip_host_alloc");
    flags = static_cast<int32_t*>(mem);
  }
  if (kmax > kmax_cap) {
    // (an earlier solve on this workspace has been synchronised: nothing
    // still reads the old scalars)
    spmv_hip_bicg_ws_destroy(ws);
    ws = nullptr;
    kmax_cap = -1;
    throw_on_error(spmv_hip_bicg_ws_create(ctx, kmax, &ws),
                   "spmv_hip_bicg_ws_create");
    kmax_cap = kmax;
  }
  // frees the vectors of one capacity, then allocates them at the new one;
  // the capacity is -1 while they are gone
  auto regrow = [&](int64_t& cap, int64_t want,
                    std::initializer_list<double**> vecs) {
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
  };
  regrow(m_cap, M, {&r, &rhat, &v, &t});
  regrow(n_cap, N_padded, {&p, &s});
  if (need_h)
    regrow(h_cap, N_padded, {&ph, &sh});
  if (need_x)
    regrow(x_cap, M, {&x});
  if (need_dinv)
    regrow(dinv_cap, M, {&dinv});
}

void BicgstabWorkspace::reserve_timing(int iterations)
{
  while (timing_ev.size() < 4 * (size_t)(iterations < 0 ? 0 : iterations))
    timing_ev.push_back(_exec.create_event(true));
}

int bicgstab(const Comm& comm, HipExecutor& exec, const Matrix<double>& A,
             const double* b, double* x, const double* dinv, int kmax,
             double rtol, std::vector<double>* rnorm_history,
             const CgOptions* options, CgStats* stats,
             BicgstabWorkspace* workspace, int* status)
{
  std::shared_ptr<const L2GMap> col_l2g = A.col_map();
  std::shared_ptr<const L2GMap> row_l2g = A.row_map();
  if (row_l2g->num_ghosts() > 0)
    throw std::runtime_error(
        "spmv::bicgstab - Error: A.row_map() has ghost entries");
  if (kmax < 0)
    throw std::runtime_error("spmv::bicgstab - Error: kmax < 0");
  const CgOptions opt = options ? *options : CgOptions();
  const int poll_every = opt.poll_every < 1 ? 1 : opt.poll_every;

  const int64_t M = row_l2g->local_size();
  const int64_t N_padded = col_l2g->local_size() + col_l2g->num_ghosts();
  spmv_hip_ctx* ctx = exec.context();

  { // x is the iterate from the first kernel on: it cannot share b or dinv
    const uintptr_t xb = reinterpret_cast<uintptr_t>(x);
    const uintptr_t bytes = (uintptr_t)M * sizeof(double);
    auto overlaps = [&](const double* q) {
      const uintptr_t qb = reinterpret_cast<uintptr_t>(q);
      return M > 0 && xb < qb + bytes && qb < xb + bytes;
    };
    if (overlaps(b))
      throw std::runtime_error("bicgstab: x overlaps b (x is updated in place)");
    if (dinv && overlaps(dinv))
      throw std::runtime_error(
          "bicgstab: x overlaps dinv (x is updated in place)");
  }
  BicgstabWorkspace own(exec);
  BicgstabWorkspace& w = workspace ? *workspace : own;
  const bool pre = dinv != nullptr;
  const bool x_aligned = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
  const bool dinv_aligned = (reinterpret_cast<uintptr_t>(dinv) & 15u) == 0;
  w.ensure(M, N_padded, kmax, !x_aligned, !dinv_aligned, pre);
  if (opt.time_spmv)
    w.reserve_timing(kmax);

  StreamGuard guard{exec, exec.get_stream()};
  { // order after whatever the caller enqueued (b, dinv may still be in flight)
    void* ev = exec.create_event();
    exec.record_event(ev, guard.prev);
    exec.stream_wait_event(w.stream, ev);
    exec.destroy_event(ev);
  }
  exec.set_stream(w.stream); // every launch below goes to this stream

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

  auto slot = [&](int (*get)(spmv_hip_bicg_ws*, int, double**), int k,
                  const char* what) {
    double* q = nullptr;
    throw_on_error(get(w.ws, k, &q), what);
    return q;
  };

  // {rr0, rho0}: one all-reduce of 2 doubles
  throw_on_error(spmv_hip_bicg_reduce_rr_rho(ctx, w.ws, 0, nullptr),
                 "spmv_hip_bicg_reduce_rr_rho");
  comm.reduce_sum(slot(spmv_hip_bicg_ws_rr_rho, 0, "spmv_hip_bicg_ws_rr_rho"),
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
  int k = 0;
  bool stopped = false;
  bool poll_pending = false;
  while (k < kmax && !stopped) {
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
      comm.reduce_sum(slot(spmv_hip_bicg_ws_rv, k, "spmv_hip_bicg_ws_rv"), 1,
                      w.stream);
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
      comm.reduce_sum(slot(spmv_hip_bicg_ws_ts_tt, k, "spmv_hip_bicg_ws_ts_tt"),
                      2, w.stream); // ts[k] and tt[k] at once
      throw_on_error(spmv_hip_bicg_update_xr_f64(ctx, w.ws, k, M, PH,
                                                 pre ? w.sh : nullptr, w.s, w.t,
                                                 w.rhat, xi, w.r, nullptr),
                     "spmv_hip_bicg_update_xr_f64");
      throw_on_error(spmv_hip_bicg_reduce_rr_rho(ctx, w.ws, k, nullptr),
                     "spmv_hip_bicg_reduce_rr_rho");
      comm.reduce_sum(slot(spmv_hip_bicg_ws_rr_rho, k,
                           "spmv_hip_bicg_ws_rr_rho"),
                      2, w.stream); // rr[k] and rho[k] at once
      throw_on_error(spmv_hip_bicg_update_p_f64(ctx, w.ws, k, M, w.r, w.v, di,
                                                w.p, pre ? w.ph : nullptr,
                                                nullptr),
                     "spmv_hip_bicg_update_p_f64");
    }

    if (k % poll_every == 0 && k < kmax) {
      // lagging look at the flag, as in cg()
      if (poll_pending) {
        exec.synchronize_event(w.poll_event);
        stopped = w.flags[0] != 0;
      }
      if (!stopped) {
        throw_on_error(spmv_hip_bicg_ws_read_async(w.ws, w.flags, nullptr, 0,
                                                   nullptr),
                       "spmv_hip_bicg_ws_read_async");
        exec.record_event(w.poll_event, w.stream);
        poll_pending = true;
      }
    }
  }

  // final state: {done, kstop, status} and the history of pairs (it has the
  // WORKSPACE's capacity; the C ABI refuses a shorter destination)
  int cap = 0;
  throw_on_error(spmv_hip_bicg_ws_capacity(w.ws, &cap),
                 "spmv_hip_bicg_ws_capacity");
  std::vector<double> rrho(2 * ((size_t)std::max(kmax, cap) + 1), 0.0);
  throw_on_error(spmv_hip_bicg_ws_read_async(w.ws, w.flags, rrho.data(),
                                             rrho.size(), nullptr),
                 "spmv_hip_bicg_ws_read_async");
  if (xi != x)
    exec.copy<double>(x, xi, M);
  exec.synchronize_stream(w.stream);

  if (stats) {
    *stats = CgStats();
    for (size_t i = 0; opt.time_spmv && i + 1 < 4 * (size_t)k; i += 2) {
      float ms = 0.f;
      throw_on_error(spmv_hip_event_elapsed_ms(ctx, timing_ev[i],
                                               timing_ev[i + 1], &ms),
                     "spmv_hip_event_elapsed_ms");
      stats->spmv_ms_total += ms;
      ++stats->spmv_launches;
    }
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
  if (rnorm_history) {
    rnorm_history->resize(k_final + 1);
    for (int j = 0; j <= k_final; ++j)
      (*rnorm_history)[j] = std::sqrt(rrho[2 * (size_t)j]);
  }
  return k_final;
}

} // namespace spmv
