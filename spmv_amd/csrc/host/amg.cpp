// spmv::AmgPreconditioner and amg_apply for HipExecutor: see cg.h.  The
// aggregates, patterns and source lists are amg_build.h's, on the host, or
// (AmgOptions::setup = device) spmv_amg_build.hip's, on the device; the
// numbers are spmv_amg.hip's, on the device, on the executor's current stream:
//     per coarsening step  galerkin (the coarse values) ; the coarse block's
//                          plan ; a read-back of the values for the next step
//     per level            diag (d, dinv, the bound) ; read of the counts
// refresh() repeats the galerkin sums and the diag kernels only.
// The tail (set_tail_rows): a descriptor table of the levels t .. last, built
// by spmv_hip_amg_tail_create from the level objects as they are; apply() puts
// one launch in the place of everything that touches those levels.
#include "cg.h"

#include <chrono>
#include <cstring>
#include <string>
#include <utility>

#include "../hip/amg_tail_rules.h"
#include "amg_build.h"
#include "solver_common.h"

namespace spmv
{
using namespace detail;

struct AmgPreconditioner::Level {
  const CSRMatrix<double>* op = nullptr; // level 0: A's local block
  std::unique_ptr<CSRMatrix<double>> own; // levels >= 1
  int32_t rows = 0, cols = 0;
  int64_t nnz = 0;
  // the step to the next level (has_step) and / or the expanded rows of
  // symmetric storage
  spmv_hip_amg_plan* plan = nullptr;
  bool has_step = false;
  std::vector<int32_t> agg; // setup = device: fetched by aggregates()
  int rounds[2] = {0, 0};   // setup = device: of pass 1 and pass 3
  // d, dinv, r, w, dd: rows; z: cols, ghost tail zero
  double *d = nullptr, *dinv = nullptr, *z = nullptr, *r = nullptr,
         *w = nullptr, *dd = nullptr;
  // apply_block: r, w, dd of rows * _block_cap, z of cols * _block_cap doubles
  double *rb = nullptr, *wb = nullptr, *ddb = nullptr, *zb = nullptr;
  double lmax = 0, lmin = 0;
  double sa[kChebyshevMaxDegree], sb[kChebyshevMaxDegree]; // smoother
  double ca[kChebyshevMaxDegree], cb[kChebyshevMaxDegree]; // coarsest level
};

struct AmgPreconditioner::Clock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double lap()
  {
    const auto t1 = std::chrono::steady_clock::now();
    const double ms
        = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
  }
};

namespace
{

const CSRMatrix<double>* amg_block_of(const Matrix<double>& A, const char* who)
{
  std::shared_ptr<L2GMap> row_map = A.row_map();
  std::shared_ptr<const L2GMap> col_map = A.col_map();
  if (row_map->num_ghosts() > 0
      || row_map->local_size() != col_map->local_size()
      || row_map->global_offset() != col_map->global_offset())
    throw std::runtime_error(
        std::string("spmv::AmgPreconditioner") + who
        + " - Error: rows and owned columns are not the same index range on "
          "this rank");
  const auto* blk = dynamic_cast<const CSRMatrix<double>*>(A.local_block());
  if (!blk)
    throw std::runtime_error(std::string("spmv::AmgPreconditioner") + who
                             + " - Error: the matrix has no local block");
  if (blk->csr_released())
    throw std::runtime_error(
        std::string("spmv::AmgPreconditioner") + who
        + " - Error: the CSR arrays of this matrix were released "
          "(release_csr); the hierarchy reads its values");
  return blk;
}

} // namespace

AmgPreconditioner::AmgPreconditioner(HipExecutor& exec, const Matrix<double>& A,
                                     const AmgOptions& options)
    : _exec(exec), _opt(options)
{
  amg_check_options(_opt.theta, _opt.max_levels, _opt.min_coarse_rows,
                    _opt.smooth_degree, _opt.coarse_degree, _opt.eig_ratio,
                    _opt.coarse_scale);
  if (_opt.setup == SgsSetup::host && _opt.order != SgsOrder::hashed)
    throw std::invalid_argument(
        "spmv::AmgPreconditioner - Error: setup = host aggregates in row order: "
        "it takes no order");
  amg_block_of(A, "");
  _symmetric = A.symmetric();
  try {
    numeric(A, true);
  } catch (...) {
    release();
    throw;
  }
}

AmgPreconditioner::~AmgPreconditioner() { release(); }

void AmgPreconditioner::release()
{
  try {
    _exec.synchronize(); // a cycle may still be in flight
  } catch (...) {
  }
  spmv_hip_amg_tail_destroy(_tail); // (it refers to the levels' arrays)
  _tail = nullptr;
  free_block_scratch();
  for (auto& lp : _levels) {
    if (!lp)
      continue;
    spmv_hip_amg_plan_destroy(lp->plan);
    lp->plan = nullptr;
    for (double** v : {&lp->d, &lp->dinv, &lp->z, &lp->r, &lp->w, &lp->dd}) {
      try {
        if (*v)
          _exec.free(*v);
      } catch (...) {
      }
      *v = nullptr;
    }
  }
  _levels.clear();
  try {
    if (_stat)
      _exec.free(_stat);
  } catch (...) {
  }
  _stat = nullptr;
}

void AmgPreconditioner::check_usable() const
{
  if (!_usable)
    throw std::runtime_error(
        "spmv::AmgPreconditioner - Error: the last refresh failed (the "
        "diagonal is not positive, or the row-sum bound is not finite); "
        "refresh before using it");
}

// d, dinv, the bound and the Chebyshev coefficients of one level
void AmgPreconditioner::level_numbers(Level& L)
{
  if (L.rows == 0)
    return;
  if (L.nnz == 0 && !_symmetric) // an empty block owns no arrays
    throw std::runtime_error(
        "spmv::AmgPreconditioner - Error: the diagonal is not positive ("
        + std::to_string(L.rows) + " of " + std::to_string(L.rows)
        + " entries are not finite or not > 0)");
  const CSRMatrix<double>& B = *L.op;
  throw_on_error(spmv_hip_amg_diag_f64(_exec.context(), L.plan, L.rows, L.rows,
                                       B.rowptr(), B.colind(), B.values(),
                                       B.diagonal(), L.d, L.dinv, _stat,
                                       nullptr),
                 "spmv_hip_amg_diag_f64");
  uint64_t words[SPMV_HIP_AMG_STAT_WORDS];
  _exec.copy_to<uint64_t>(words, _exec.get_host(), _stat,
                          SPMV_HIP_AMG_STAT_WORDS); // waits
  if (words[0] != 0)
    throw std::runtime_error(
        "spmv::AmgPreconditioner - Error: the diagonal is not positive ("
        + std::to_string(words[0]) + " of " + std::to_string(L.rows)
        + " entries are not finite or not > 0)");
  double lmax = 0.0;
  for (int k = 1; k < SPMV_HIP_AMG_STAT_WORDS; ++k) {
    double g;
    std::memcpy(&g, &words[k], sizeof g);
    if (g > lmax)
      lmax = g;
  }
  // d > 0 does not bound g: a subnormal d has dinv = Inf, and a row of huge
  // entries overflows its sum.  (Rows whose g is NaN took no part: a level
  // of such rows alone has the bound 0.0.)
  if (!(lmax - lmax == 0.0) || !(lmax > 0.0))
    throw std::runtime_error(
        "spmv::AmgPreconditioner - Error: the row-sum bound is not finite (max "
        "of |row| / d = "
        + std::to_string(lmax) + " on a level of " + std::to_string(L.rows)
        + " rows: a diagonal entry too small to invert, or entries whose sum "
          "overflows)");
  L.lmax = lmax;
  L.lmin = lmax / _opt.eig_ratio;
  chebyshev_coefficients(_opt.smooth_degree, L.lmin, L.lmax, L.sa, L.sb);
  chebyshev_coefficients(_opt.coarse_degree, L.lmin, L.lmax, L.ca, L.cb);
}

// One step of the device setup: the aggregates of L and the plan of its step
// (symmetric storage: the xrow lists, step or no step), from L's arrays where
// they lie.  -> the rows of the coarse level, 0: no step; then *c_rowptr /
// *c_colind are the coarse pattern on the device, the caller's to free or to
// hand on.
int32_t AmgPreconditioner::step_on_device(Level& L, bool sym, bool coarsen,
                                       int32_t** c_rowptr, int32_t** c_colind,
                                       int64_t* c_nnz)
{
  spmv_hip_ctx* ctx = _exec.context();
  const CSRMatrix<double>& B = *L.op;
  const bool has = L.nnz > 0; // (an empty block owns no arrays)
  const int32_t* rowptr = has ? B.rowptr() : nullptr;
  const int32_t* colind = has ? B.colind() : nullptr;
  int64_t info[SPMV_HIP_AMG_INFO_WORDS];
  int32_t* agg = nullptr;
  int32_t nc = 0;
  *c_rowptr = *c_colind = nullptr;
  *c_nnz = 0;
  Clock clock;
  try {
    if (coarsen) {
      agg = _exec.alloc<int32_t>((size_t)L.rows);
      throw_on_error(
          spmv_hip_amg_aggregate(ctx, L.rows, L.cols, L.nnz, rowptr, colind,
                                 has ? B.values() : nullptr,
                                 sym ? B.diagonal() : nullptr, sym ? 1 : 0,
                                 _opt.theta,
                                 _opt.order == SgsOrder::natural
                                     ? SPMV_HIP_MCGS_NATURAL
                                     : SPMV_HIP_MCGS_HASHED,
                                 agg, &nc, L.rounds, info, nullptr),
          "spmv_hip_amg_aggregate");
      _setup_temp_bytes = std::max(_setup_temp_bytes, info[1]);
      if (nc == L.rows) // nothing merged: discard it
        nc = 0;
      if (nc == 0)
        L.rounds[0] = L.rounds[1] = 0;
    }
    _aggregate_ms += clock.lap();
    if (nc > 0)
      *c_rowptr = _exec.alloc<int32_t>((size_t)nc + 1);
    throw_on_error(spmv_hip_amg_plan_build(ctx, L.rows, L.cols, L.nnz, rowptr,
                                           colind, sym ? 1 : 0,
                                           nc > 0 ? agg : nullptr, nc, *c_rowptr,
                                           c_colind, c_nnz, &L.plan, info,
                                           nullptr),
                   "spmv_hip_amg_plan_build");
    _setup_temp_bytes = std::max(_setup_temp_bytes, info[1]);
  } catch (...) {
    if (agg)
      _exec.free(agg);
    if (*c_rowptr)
      _exec.free(*c_rowptr);
    *c_rowptr = nullptr;
    throw;
  }
  if (agg)
    _exec.free(agg);
  _build_ms += clock.lap();
  return nc;
}

// The coarse level of L's step: the pattern arrays (device, filled; this
// function owns them from the call on) are adopted by a new block whose values
// the device sums from L's plan.
void AmgPreconditioner::add_coarse_level(Level& L, int32_t nc, int64_t nnz_c,
                                         int32_t* c_rowptr, int32_t* c_colind)
{
  // coarse blocks live on this executor; the object does not own it
  std::shared_ptr<DeviceExecutor> shared(std::shared_ptr<void>(), &_exec);
  double* c_values = nullptr;
  std::unique_ptr<Level> next;
  try {
    c_values = _exec.alloc<double>((size_t)nnz_c);
    next = std::make_unique<Level>();
    throw_on_error(spmv_hip_amg_galerkin_f64(_exec.context(), L.plan,
                                             L.op->values(), L.op->diagonal(),
                                             c_values, nullptr),
                   "spmv_hip_amg_galerkin_f64");
  } catch (...) {
    for (void* p : {(void*)c_rowptr, (void*)c_colind, (void*)c_values})
      if (p)
        _exec.free(p);
    throw;
  }
  // (the block owns the arrays from here on; its plan sees the values)
  next->own.reset(new CSRMatrix<double>(CSRMatrix<double>::AdoptDevice(), shared,
                                        nc, nc, nnz_c, c_rowptr, c_colind,
                                        c_values, nullptr, false));
  if (next->own->csr_released())
    throw std::runtime_error(
        "spmv::AmgPreconditioner - Error: the context released the CSR "
        "arrays of a coarse level (release_csr); the hierarchy needs them");
  next->op = next->own.get();
  next->rows = next->cols = nc;
  next->nnz = nnz_c;
  _levels.push_back(std::move(next));
}

// setup = host: every level is read back and coarsened by amg_build.h
void AmgPreconditioner::levels_on_host(Clock& clock)
{
  spmv_hip_ctx* ctx = _exec.context();
  const DeviceExecutor& host = _exec.get_host();
  const CSRMatrix<double>* blk = _levels[0]->op;
  const int64_t n0 = _levels[0]->rows;
  // level 0, read back (the copies wait for the device)
  std::vector<int32_t> rowptr((size_t)n0 + 1, 0), colind((size_t)_num_values);
  std::vector<double> values((size_t)_num_values), diagonal;
  if (_num_values > 0) { // (an empty block owns no arrays)
    _exec.copy_to<int32_t>(rowptr.data(), host, blk->rowptr(), (size_t)n0 + 1);
    _exec.copy_to<int32_t>(colind.data(), host, blk->colind(),
                           (size_t)_num_values);
    _exec.copy_to<double>(values.data(), host, blk->values(),
                          (size_t)_num_values);
  }
  if (_symmetric && n0 > 0) {
    diagonal.resize((size_t)n0);
    _exec.copy_to<double>(diagonal.data(), host, blk->diagonal(), (size_t)n0);
  }
  for (;;) {
    Level& L = *_levels.back();
    const bool sym = _symmetric && _levels.size() == 1;
    const bool coarsen = L.rows > _opt.min_coarse_rows
                         && (int)_levels.size() < _opt.max_levels;
    if (!coarsen && !sym)
      break;
    const AmgExpanded x
        = amg_expand(rowptr.data(), colind.data(), L.rows, L.rows, sym);
    AmgStep step;
    if (coarsen) {
      step = amg_aggregate(x, values.data(), diagonal.data(), _opt.theta);
      if (step.n_agg == L.rows) // nothing merged: discard it
        step = AmgStep();
      else
        amg_galerkin_pattern(x, &step);
    }
    const int32_t nc = step.n_agg;
    const int64_t nnz_c = (int64_t)step.colind.size();
    spmv_hip_amg_host in{};
    in.fine_rows = L.rows;
    in.coarse_rows = nc;
    in.num_values = L.nnz;
    in.num_diagonal = sym ? L.rows : 0;
    in.coarse_nnz = nnz_c;
    if (nc > 0) {
      in.agg = step.agg.data();
      in.member_ptr = step.member_ptr.data();
      in.member = step.member.data();
      in.src_ptr = step.src_ptr.data();
      in.src = step.src.data();
    }
    if (sym) {
      in.xrow_ptr = x.ptr.data();
      in.xrow_src = x.src.data();
    }
    throw_on_error(spmv_hip_amg_plan_create(ctx, &in, &L.plan),
                   "spmv_hip_amg_plan_create");
    if (nc == 0)
      break;
    L.has_step = true;
    L.agg = std::move(step.agg);
    _symbolic_ms += clock.lap();

    // the coarse block: pattern uploaded, values summed on the device
    int32_t *c_rowptr = nullptr, *c_colind = nullptr;
    try {
      c_rowptr = _exec.alloc<int32_t>((size_t)nc + 1);
      c_colind = _exec.alloc<int32_t>((size_t)nnz_c);
      _exec.copy_from<int32_t>(c_rowptr, host, step.rowptr.data(), (size_t)nc + 1);
      _exec.copy_from<int32_t>(c_colind, host, step.colind.data(), (size_t)nnz_c);
    } catch (...) {
      for (int32_t* p : {c_rowptr, c_colind})
        if (p)
          _exec.free(p);
      throw;
    }
    add_coarse_level(L, nc, nnz_c, c_rowptr, c_colind);
    // the next step aggregates on the host
    rowptr = std::move(step.rowptr);
    colind = std::move(step.colind);
    values.resize((size_t)nnz_c);
    _exec.copy_to<double>(values.data(), host, _levels.back()->own->values(),
                          (size_t)nnz_c);
    diagonal.clear();
    _numeric_ms += clock.lap();
  }
}

// setup = device: nothing of any level's matrix is read back
void AmgPreconditioner::levels_on_device(Clock& clock)
{
  for (;;) {
    Level& L = *_levels.back();
    const bool sym = _symmetric && _levels.size() == 1;
    const bool coarsen = L.rows > _opt.min_coarse_rows
                         && (int)_levels.size() < _opt.max_levels;
    if (!coarsen && !sym)
      break;
    int32_t *c_rowptr = nullptr, *c_colind = nullptr;
    int64_t nnz_c = 0;
    const int32_t nc
        = step_on_device(L, sym, coarsen, &c_rowptr, &c_colind, &nnz_c);
    if (nc == 0)
      break;
    L.has_step = true;
    _symbolic_ms += clock.lap();
    add_coarse_level(L, nc, nnz_c, c_rowptr, c_colind);
    _numeric_ms += clock.lap();
  }
}

void AmgPreconditioner::numeric(const Matrix<double>& A, bool build)
{
  const auto* blk = static_cast<const CSRMatrix<double>*>(A.local_block());
  spmv_hip_ctx* ctx = _exec.context();
  _usable = false;
  Clock clock;
  if (build) {
    _symbolic_ms = _numeric_ms = _aggregate_ms = _build_ms = 0;
    _setup_temp_bytes = 0;
    _stat = _exec.alloc<uint64_t>(SPMV_HIP_AMG_STAT_WORDS);
    _num_values = blk->non_zeros();
    auto first = std::make_unique<Level>();
    first->op = blk;
    first->rows = (int32_t)A.row_map()->local_size();
    first->cols = blk->cols();
    first->nnz = _num_values;
    _levels.push_back(std::move(first));
    if (_opt.setup == SgsSetup::device)
      levels_on_device(clock);
    else
      levels_on_host(clock);
    for (auto& lp : _levels) {
      Level& L = *lp;
      if (L.rows == 0)
        continue;
      const size_t n = (size_t)L.rows;
      for (double** v : {&L.d, &L.dinv, &L.r, &L.w, &L.dd})
        *v = _exec.alloc<double>(n);
      L.z = _exec.alloc<double>((size_t)L.cols);
      _exec.memset<double>(L.z, 0, (size_t)L.cols);
    }
    _symbolic_ms += clock.lap();
  } else {
    Level& L0 = *_levels[0];
    L0.op = blk;
    for (size_t l = 0; l + 1 < _levels.size(); ++l) {
      Level& L = *_levels[l];
      Level& C = *_levels[l + 1];
      throw_on_error(
          spmv_hip_amg_galerkin_f64(ctx, L.plan, L.op->values(),
                                    L.op->diagonal(),
                                    const_cast<double*>(C.own->values()),
                                    nullptr),
          "spmv_hip_amg_galerkin_f64");
      C.own->values_changed();
    }
  }
  for (auto& lp : _levels)
    level_numbers(*lp);
  // the tail's table holds coefficients of its own (the reads above waited:
  // nothing is in flight)
  for (int l = _tail ? _tail_first : levels(); l < levels(); ++l) {
    const Level& L = *_levels[(size_t)l];
    const bool last = l == levels() - 1;
    throw_on_error(spmv_hip_amg_tail_set_coefficients(
                       _tail, l - _tail_first, last ? L.ca : L.sa,
                       last ? L.cb : L.sb),
                   "spmv_hip_amg_tail_set_coefficients");
  }
  _numeric_ms += clock.lap();
  _usable = true;
}

void AmgPreconditioner::drop_tail()
{
  if (!_tail)
    return;
  _exec.synchronize(); // an application may still be in flight
  spmv_hip_amg_tail_destroy(_tail);
  _tail = nullptr;
  _tail_first = 0;
  _tail_lanes.clear();
}

void AmgPreconditioner::build_tail()
{
  drop_tail();
  const int nl = levels();
  std::vector<int64_t> rows((size_t)nl);
  for (int l = 0; l < nl; ++l)
    rows[(size_t)l] = _levels[(size_t)l]->rows;
  const int t = amg_tail_first_level(rows.data(), nl, _tail_rows);
  if (t >= nl)
    return;
  _exec.synchronize(); // tail_create reads the levels' index arrays back
  std::vector<spmv_hip_amg_tail_level> desc((size_t)(nl - t));
  std::vector<int> lanes((size_t)(nl - t));
  for (int l = t; l < nl; ++l) {
    const Level& L = *_levels[(size_t)l];
    const CSRMatrix<double>& B = *L.own;
    const bool last = l == nl - 1;
    // the order of the level's product is the plan's to say
    const int vec = B.query("algo") == SPMV_HIP_ALGO_VECTOR
                        ? B.query("lanes_per_row")
                        : 0;
    spmv_hip_amg_tail_level& d = desc[(size_t)(l - t)];
    d = spmv_hip_amg_tail_level();
    d.rows = L.rows;
    d.lanes_per_row = lanes[(size_t)(l - t)] = vec;
    d.nnz = L.nnz;
    d.rowptr = B.rowptr();
    d.colind = B.colind();
    d.values = B.values();
    d.dinv = L.dinv;
    d.r = L.r;
    d.w = L.w;
    d.dd = L.dd;
    d.z = L.z;
    d.step = last ? nullptr : L.plan;
    d.a = last ? L.ca : L.sa;
    d.b = last ? L.cb : L.sb;
  }
  spmv_hip_amg_tail_host in{};
  in.num_levels = nl - t;
  in.smooth_degree = _opt.smooth_degree;
  in.coarse_degree = _opt.coarse_degree;
  in.coarse_scale = _opt.coarse_scale;
  in.levels = desc.data();
  throw_on_error(spmv_hip_amg_tail_create(_exec.context(), &in, &_tail),
                 "spmv_hip_amg_tail_create");
  _tail_first = t;
  _tail_lanes = std::move(lanes);
}

void AmgPreconditioner::set_tail_rows(int64_t max_rows)
{
  amg_check_tail_rows(max_rows);
  _tail_rows = max_rows;
  try {
    build_tail();
  } catch (...) {
    _tail_rows = 0; // no tail exists: the setting says so
    throw;
  }
}

int AmgPreconditioner::tail_levels() const
{
  return _tail ? levels() - _tail_first : 0;
}

int AmgPreconditioner::tail_lanes(int level) const
{
  if (level < 0 || level >= levels())
    throw std::runtime_error(
        "spmv::AmgPreconditioner::tail_lanes - Error: no such level");
  if (!_tail || level < _tail_first)
    return -1;
  return _tail_lanes[(size_t)(level - _tail_first)];
}

void AmgPreconditioner::refresh(const Matrix<double>& A)
{
  const CSRMatrix<double>* blk = amg_block_of(A, "::refresh");
  if (A.row_map()->local_size() != rows(0) || A.symmetric() != _symmetric
      || blk->non_zeros() != _num_values || blk->cols() != _levels[0]->cols)
    throw std::runtime_error(
        "spmv::AmgPreconditioner::refresh - Error: not the pattern this object "
        "was built for (rows, storage or number of stored entries differ)");
  _numeric_ms = 0;
  numeric(A, false);
}

int AmgPreconditioner::levels() const { return (int)_levels.size(); }

namespace
{
void check_level(int level, int levels, const char* who)
{
  if (level < 0 || level >= levels)
    throw std::runtime_error(std::string("spmv::AmgPreconditioner::") + who
                             + " - Error: no such level");
}
} // namespace

int AmgPreconditioner::rows(int level) const
{
  check_level(level, levels(), "rows");
  return _levels[(size_t)level]->rows;
}

int64_t AmgPreconditioner::non_zeros(int level) const
{
  check_level(level, levels(), "non_zeros");
  return _levels[(size_t)level]->nnz;
}

double AmgPreconditioner::lmax(int level) const
{
  check_level(level, levels(), "lmax");
  check_usable();
  return _levels[(size_t)level]->lmax;
}

int AmgPreconditioner::rounds(int level, int pass) const
{
  check_level(level, levels(), "rounds");
  const Level& L = *_levels[(size_t)level];
  if (pass > 1)
    throw std::runtime_error(
        "spmv::AmgPreconditioner::rounds - Error: no such pass");
  return pass < 0 ? L.rounds[0] + L.rounds[1] : L.rounds[pass];
}

const spmv_hip_amg_plan* AmgPreconditioner::step_plan(int level) const
{
  check_level(level, levels(), "step_plan");
  return _levels[(size_t)level]->plan;
}

void AmgPreconditioner::aggregates(int level, int32_t* out) const
{
  check_level(level, levels() - 1, "aggregates");
  Level& L = *_levels[(size_t)level];
  if (L.agg.empty() && L.rows > 0) { // setup = device keeps no host copy
    L.agg.resize((size_t)L.rows);
    spmv_hip_amg_export ex{};
    ex.agg = L.agg.data();
    throw_on_error(spmv_hip_amg_plan_export(L.plan, &ex),
                   "spmv_hip_amg_plan_export");
  }
  const std::vector<int32_t>& agg = L.agg;
  if (!out && !agg.empty())
    throw std::runtime_error(
        "spmv::AmgPreconditioner::aggregates - Error: NULL output");
  std::copy(agg.begin(), agg.end(), out);
}

void AmgPreconditioner::level_matrix(int level, int32_t* rowptr, int32_t* colind,
                                     double* values) const
{
  check_level(level, levels(), "level_matrix");
  if (level < 1)
    throw std::runtime_error(
        "spmv::AmgPreconditioner::level_matrix - Error: level 0 is the "
        "matrix's own block");
  const Level& L = *_levels[(size_t)level];
  const DeviceExecutor& host = _exec.get_host();
  if (rowptr)
    _exec.copy_to<int32_t>(rowptr, host, L.own->rowptr(), (size_t)L.rows + 1);
  if (colind)
    _exec.copy_to<int32_t>(colind, host, L.own->colind(), (size_t)L.nnz);
  if (values)
    _exec.copy_to<double>(values, host, L.own->values(), (size_t)L.nnz);
}

int64_t AmgPreconditioner::plan_bytes() const
{
  int64_t total = SPMV_HIP_AMG_STAT_WORDS * 8;
  if (_tail) {
    int64_t bytes = 0;
    throw_on_error(spmv_hip_amg_tail_bytes(_tail, &bytes),
                   "spmv_hip_amg_tail_bytes");
    total += bytes;
  }
  for (const auto& lp : _levels) {
    const Level& L = *lp;
    int64_t bytes = 0;
    if (L.plan)
      throw_on_error(spmv_hip_amg_plan_bytes(L.plan, &bytes),
                     "spmv_hip_amg_plan_bytes");
    total += bytes;
    if (L.own)
      total += (int64_t)L.own->format_size()
               + (int64_t)L.own->query("plan_kib") * 1024;
    if (L.rows > 0)
      total += ((int64_t)L.rows * 5 + L.cols) * 8;
    // the block scratch, once it exists: the vectors, and the columns a coarse
    // block's plan keeps for its per-column product (the plan's own: they stay
    // with it after release_block_scratch)
    if (L.rows > 0 && _block_cap > 0)
      total += ((int64_t)L.rows * 3 + L.cols) * 8 * _block_cap;
    if (L.own)
      total += (int64_t)L.own->query("mv_kib") * 1024;
  }
  total += _block_cols_elems * 8;
  return total;
}

void AmgPreconditioner::apply(const double* r, double* z) const
{
  check_usable();
  const Level& L0 = *_levels[0];
  const int64_t n0 = L0.rows;
  if (ranges_overlap(z, r, n0))
    throw std::runtime_error("amg_apply: z overlaps r");
  if (n0 == 0)
    return;
  if (!r || !z)
    throw std::runtime_error("amg_apply: NULL vector");
  spmv_hip_ctx* ctx = _exec.context();
  const int nl = levels(), s = _opt.smooth_degree;

  // everything on the executor's current stream, nothing waits
  const double* r0 = r;
  if (!is_aligned16(r)) { // the streaming kernels load 16 bytes at a time
    _exec.copy<double>(L0.r, r, (size_t)n0);
    r0 = L0.r;
  }
  auto rhs = [&](int l) { return l == 0 ? r0 : _levels[(size_t)l]->r; };
  auto product = [&](const Level& L) { L.op->mult(1.0, L.z, 0.0, L.w); };
  // the `degree`-step Chebyshev iteration from z = 0
  auto chebyshev = [&](const Level& L, const double* rl, int degree,
                       const double* a, const double* b) {
    throw_on_error(spmv_hip_cheb_apply0_f64(ctx, L.rows, b[0], rl, L.dinv,
                                            degree > 1 ? L.dd : nullptr, L.z,
                                            nullptr),
                   "spmv_hip_cheb_apply0_f64");
    for (int j = 1; j < degree; ++j) {
      product(L);
      throw_on_error(spmv_hip_cheb_step_f64(ctx, nullptr, L.rows, a[j], b[j],
                                            j == degree - 1, L.w, rl, L.dinv,
                                            L.dd, L.z, nullptr),
                     "spmv_hip_cheb_step_f64");
    }
  };
  // the first level of the tail (nl: none): everything from its smoother down
  // to the coarsest level and back up to its post-smoother is one launch
  const int t = _tail ? _tail_first : nl;
  for (int l = 0; l < nl; ++l) {
    const Level& L = *_levels[(size_t)l];
    if (l == t) {
      throw_on_error(spmv_hip_amg_tail_run_f64(ctx, _tail, nullptr),
                     "spmv_hip_amg_tail_run_f64");
      break;
    }
    if (l == nl - 1) {
      chebyshev(L, rhs(l), _opt.coarse_degree, L.ca, L.cb);
      break;
    }
    chebyshev(L, rhs(l), s, L.sa, L.sb);
    product(L);
    throw_on_error(spmv_hip_amg_restrict_f64(ctx, L.plan, rhs(l), L.w,
                                             _levels[(size_t)l + 1]->r, nullptr),
                   "spmv_hip_amg_restrict_f64");
  }
  for (int l = std::min(nl - 2, t - 1); l >= 0; --l) {
    const Level& L = *_levels[(size_t)l];
    throw_on_error(spmv_hip_amg_prolong_f64(ctx, L.plan, _opt.coarse_scale,
                                            _levels[(size_t)l + 1]->z, L.z,
                                            nullptr),
                   "spmv_hip_amg_prolong_f64");
    product(L);
    throw_on_error(spmv_hip_amg_post0_f64(ctx, L.rows, L.sb[0], L.w, rhs(l),
                                          L.dinv, s > 1 ? L.dd : nullptr, L.z,
                                          nullptr),
                   "spmv_hip_amg_post0_f64");
    for (int j = 1; j < s; ++j) {
      product(L);
      throw_on_error(spmv_hip_cheb_step_f64(ctx, nullptr, L.rows, L.sa[j],
                                            L.sb[j], j == s - 1, L.w, rhs(l),
                                            L.dinv, L.dd, L.z, nullptr),
                     "spmv_hip_cheb_step_f64");
    }
  }
  _exec.copy<double>(z, L0.z, (size_t)n0);
}

void amg_apply(HipExecutor&, const AmgPreconditioner& M, const double* r,
               double* z)
{
  M.apply(r, z);
}

// ---- the block cycle --------------------------------------------------------------
namespace
{
// column stride of level 0's per-column product: whole units of 4 doubles, so
// that every column starts 16-byte aligned
int64_t block_col_stride(int64_t n) { return (n + 3) & ~(int64_t)3; }
} // namespace

void AmgPreconditioner::free_block_scratch() const
{
  for (auto& lp : _levels) {
    if (!lp)
      continue;
    for (double** v : {&lp->rb, &lp->wb, &lp->ddb, &lp->zb}) {
      try {
        if (*v)
          _exec.free(*v);
      } catch (...) {
      }
      *v = nullptr;
    }
  }
  try {
    if (_block_cols)
      _exec.free(_block_cols);
  } catch (...) {
  }
  _block_cols = nullptr;
  _block_cols_elems = 0;
  _block_cap = _block_last = 0;
}

void AmgPreconditioner::release_block_scratch()
{
  if (_block_cap == 0 && !_block_cols)
    return;
  _exec.synchronize(); // a cycle may still be in flight
  free_block_scratch();
}

void AmgPreconditioner::ensure_block_scratch(int nrhs) const
{
  if (nrhs <= _block_cap)
    return;
  if (_block_cap > 0 || _block_cols) {
    _exec.synchronize(); // an application of the narrower width may be in flight
    free_block_scratch();
  }
  try {
    for (auto& lp : _levels) {
      Level& L = *lp;
      if (L.rows == 0)
        continue;
      const size_t n = (size_t)L.rows * (size_t)nrhs;
      for (double** v : {&L.rb, &L.wb, &L.ddb})
        *v = _exec.alloc<double>(n);
      L.zb = _exec.alloc<double>((size_t)L.cols * (size_t)nrhs);
      // A coarse block whose single-vector product adds in the sub-wavefront
      // order: its mult_block takes that launch per column from now on
      if (L.own && L.own->query("algo") == SPMV_HIP_ALGO_VECTOR)
        L.own->tune("mv_native", 0);
    }
  } catch (...) {
    free_block_scratch();
    throw;
  }
  _block_cap = nrhs;
  _block_last = 0;
}

void AmgPreconditioner::apply_block(const double* R, double* Z, int nrhs) const
{
  const int64_t n0 = _levels.empty() ? 0 : _levels[0]->rows;
  amg_apply_block_check_rules(nrhs, n0, R, Z);
  if (nrhs == 1) {
    apply(R, Z);
    return;
  }
  check_usable();
  if (n0 == 0)
    return;
  if (!R || !Z)
    throw std::runtime_error("amg_apply_block: NULL vector");
  ensure_block_scratch(nrhs);
  spmv_hip_ctx* ctx = _exec.context();
  const Level& L0 = *_levels[0];
  const int nl = levels(), s = _opt.smooth_degree;
  const size_t m0 = (size_t)n0 * (size_t)nrhs;

  // everything on the executor's current stream, nothing waits
  if (nrhs != _block_last) { // the ghost tail of z sits where this width puts it
    if (L0.cols > L0.rows)
      _exec.memset<double>(L0.zb + m0, 0,
                           (size_t)(L0.cols - L0.rows) * (size_t)nrhs);
    _block_last = nrhs;
  }
  const double* r0 = R;
  if (!is_aligned16(R)) { // the streaming kernels load 16 bytes at a time
    _exec.copy<double>(L0.rb, R, m0);
    r0 = L0.rb;
  }
  auto rhs = [&](int l) { return l == 0 ? r0 : _levels[(size_t)l]->rb; };
  // w = A z.  mult_block's columns have mult's bits except where the native
  // multi-vector kernel would replace the sub-wavefront kernel (nrhs 2, 4, 8):
  // the coarse blocks were told not to take it (ensure_block_scratch); level 0
  // is the caller's matrix and is multiplied column by column here.
  auto product = [&](const Level& L) {
    const bool native = nrhs == 2 || nrhs == 4 || nrhs == 8;
    if (L.own || !native || L.op->symmetric() || L.nnz == 0
        || L.op->query("algo") != SPMV_HIP_ALGO_VECTOR) {
      L.op->mult_block(1.0, L.zb, 0.0, L.wb, nrhs);
      return;
    }
    const int64_t ldx = block_col_stride(L.cols), ldy = block_col_stride(L.rows);
    const int64_t need = (ldx + ldy) * nrhs;
    if (need > _block_cols_elems) {
      if (_block_cols) {
        _exec.synchronize();
        _exec.free(_block_cols);
        _block_cols = nullptr;
        _block_cols_elems = 0;
      }
      _block_cols = _exec.alloc<double>((size_t)need);
      _block_cols_elems = need;
    }
    double* xs = _block_cols;
    double* ys = xs + ldx * nrhs;
    throw_on_error(spmv_hip_deinterleave_f64(ctx, L.cols, nrhs, L.zb, ldx, xs,
                                             nullptr),
                   "spmv_hip_deinterleave_f64");
    for (int c = 0; c < nrhs; ++c)
      L.op->mult(1.0, xs + ldx * c, 0.0, ys + ldy * c);
    throw_on_error(spmv_hip_interleave_f64(ctx, L.rows, nrhs, ys, ldy, L.wb,
                                           nullptr),
                   "spmv_hip_interleave_f64");
  };
  auto chebyshev = [&](const Level& L, const double* rl, int degree,
                       const double* a, const double* b) {
    throw_on_error(spmv_hip_cheb_apply0_block_f64(ctx, L.rows, nrhs, b[0], rl,
                                                  L.dinv,
                                                  degree > 1 ? L.ddb : nullptr,
                                                  L.zb, nullptr),
                   "spmv_hip_cheb_apply0_block_f64");
    for (int j = 1; j < degree; ++j) {
      product(L);
      throw_on_error(spmv_hip_cheb_step_block_f64(ctx, L.rows, nrhs, a[j], b[j],
                                                  j == degree - 1, L.wb, rl,
                                                  L.dinv, L.ddb, L.zb, nullptr),
                     "spmv_hip_cheb_step_block_f64");
    }
  };
  // (the fused tail is a single-vector kernel: every level runs launch by
  // launch, with the same bits)
  for (int l = 0; l < nl; ++l) {
    const Level& L = *_levels[(size_t)l];
    if (l == nl - 1) {
      chebyshev(L, rhs(l), _opt.coarse_degree, L.ca, L.cb);
      break;
    }
    chebyshev(L, rhs(l), s, L.sa, L.sb);
    product(L);
    throw_on_error(spmv_hip_amg_restrict_block_f64(ctx, L.plan, nrhs, rhs(l),
                                                   L.wb,
                                                   _levels[(size_t)l + 1]->rb,
                                                   nullptr),
                   "spmv_hip_amg_restrict_block_f64");
  }
  for (int l = nl - 2; l >= 0; --l) {
    const Level& L = *_levels[(size_t)l];
    throw_on_error(spmv_hip_amg_prolong_block_f64(ctx, L.plan, nrhs,
                                                  _opt.coarse_scale,
                                                  _levels[(size_t)l + 1]->zb,
                                                  L.zb, nullptr),
                   "spmv_hip_amg_prolong_block_f64");
    product(L);
    throw_on_error(spmv_hip_amg_post0_block_f64(ctx, L.rows, nrhs, L.sb[0], L.wb,
                                                rhs(l), L.dinv,
                                                s > 1 ? L.ddb : nullptr, L.zb,
                                                nullptr),
                   "spmv_hip_amg_post0_block_f64");
    for (int j = 1; j < s; ++j) {
      product(L);
      throw_on_error(spmv_hip_cheb_step_block_f64(ctx, L.rows, nrhs, L.sa[j],
                                                  L.sb[j], j == s - 1, L.wb,
                                                  rhs(l), L.dinv, L.ddb, L.zb,
                                                  nullptr),
                     "spmv_hip_cheb_step_block_f64");
    }
  }
  _exec.copy<double>(Z, L0.zb, m0);
}

void amg_apply_block(HipExecutor&, const AmgPreconditioner& M, const double* R,
                     double* Z, int nrhs)
{
  M.apply_block(R, Z, nrhs);
}

} // namespace spmv
