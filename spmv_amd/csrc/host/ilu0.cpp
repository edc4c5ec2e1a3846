// spmv::Ilu0Preconditioner for HipExecutor: see cg.h.  The symbolic half is
// ilu0_build.h's, on the host, or (SgsOptions::setup = device) the colouring and
// spmv_hip_ilu0_plan_build of spmv_mcgs_build.hip, on the device; the numeric
// half is spmv_ilu0.hip's, on the device, on the executor's current stream:
//     Matrix::diagonal (general storage; symmetric storage has the array)
//     gather ; C - 1 factor launches ; finish ; scatter
//     read of the two pivot counts (the one wait)
#include "cg.h"

#include <algorithm>
#include <chrono>
#include <limits>
#include <string>
#include <utility>

#include "ilu0_build.h"
#include "solver_common.h"

namespace spmv
{
using namespace detail;

namespace
{

const CSRMatrix<double>* block_of(const Matrix<double>& A, const char* who)
{
  std::shared_ptr<L2GMap> row_map = A.row_map();
  std::shared_ptr<const L2GMap> col_map = A.col_map();
  if (row_map->num_ghosts() > 0
      || row_map->local_size() != col_map->local_size()
      || row_map->global_offset() != col_map->global_offset())
    throw std::runtime_error(
        std::string("spmv::Ilu0Preconditioner") + who
        + " - Error: rows and owned columns are not the same index range on "
          "this rank");
  const auto* blk = dynamic_cast<const CSRMatrix<double>*>(A.local_block());
  if (!blk)
    throw std::runtime_error(std::string("spmv::Ilu0Preconditioner") + who
                             + " - Error: the matrix has no local block");
  if (blk->csr_released())
    throw std::runtime_error(
        std::string("spmv::Ilu0Preconditioner") + who
        + " - Error: the CSR arrays of this matrix were released "
          "(release_csr); the factorisation reads its values");
  return blk;
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now() - t0)
      .count();
}

} // namespace

Ilu0Preconditioner::Ilu0Preconditioner(HipExecutor& exec, const Matrix<double>& A)
    : SgsPreconditioner(exec)
{
  construct(A, SgsOptions());
}

Ilu0Preconditioner::Ilu0Preconditioner(HipExecutor& exec, const Matrix<double>& A,
                                       const SgsOptions& options)
    : SgsPreconditioner(exec)
{
  if (options.setup == SgsSetup::host
      && (options.colors || options.order != SgsOrder::hashed))
    throw std::invalid_argument(
        "spmv::Ilu0Preconditioner - Error: setup = host colours by itself: it "
        "takes neither colors nor an order");
  construct(A, options);
}

void Ilu0Preconditioner::construct(const Matrix<double>& A,
                                   const SgsOptions& options)
{
  const CSRMatrix<double>* blk = block_of(A, "");
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t n = A.row_map()->local_size();
  _symmetric = A.symmetric();
  _num_values = blk->non_zeros();
  try { // (the destructor does not run)
    if (options.setup == SgsSetup::host)
      symbolic_on_host(blk, n, options.values);
    else
      symbolic_on_device(blk, n, options, t0);
  } catch (...) {
    spmv_hip_ilu0_plan_destroy(_ilu);
    throw;
  }
  _symbolic_ms = ms_since(t0);

  const auto t1 = std::chrono::steady_clock::now();
  try {
    if (!_symmetric && n > 0)
      _diag = _exec.alloc<double>((size_t)n);
    numeric(A);
  } catch (...) {
    if (_diag)
      _exec.free(_diag);
    spmv_hip_ilu0_plan_destroy(_ilu);
    throw;
  }
  _numeric_ms = ms_since(t1);
}

void Ilu0Preconditioner::symbolic_on_host(const CSRMatrix<double>* blk, int64_t n,
                                          SgsValues values)
{
  HipExecutor& exec = _exec;
  const int64_t nnz = blk->non_zeros();
  // the pattern, read back (the copies wait for the device); no values
  const DeviceExecutor& host = exec.get_host();
  std::vector<int32_t> rowptr((size_t)n + 1, 0), colind((size_t)nnz);
  if (nnz > 0) { // (an empty block owns no arrays)
    exec.copy_to<int32_t>(rowptr.data(), host, blk->rowptr(), (size_t)n + 1);
    exec.copy_to<int32_t>(colind.data(), host, blk->colind(), (size_t)nnz);
  }
  Ilu0Symbolic sym = ilu0_symbolic(rowptr.data(), colind.data(), n, n, _symmetric);
  std::vector<int32_t>().swap(colind);
  _nbefore = (int64_t)sym.before.cpos.size();
  _nafter = (int64_t)sym.after.cpos.size();

  auto sliced_of = [](const SgsSlicedPart& s) {
    return spmv_hip_mcgs_part{s.color_slice.data(), s.slice_pos0.data(),
                              s.slice_ptr.data(),   s.len.data(),
                              s.col.data(),         s.val.data(),
                              s.color_long.data(),  s.long_pos.data(),
                              s.long_ptr.data(),    s.long_col.data(),
                              s.long_val.data()};
  };
  auto part_of = [](const Ilu0Part& p) {
    return spmv_hip_ilu0_part{p.ptr.data(), p.cpos.data(), p.src.data(),
                              p.slot.data()};
  };
  const std::vector<double> no_dinv((size_t)n, 0.0); // the factorisation's to write
  spmv_hip_ilu0_host in{};
  in.mcgs.num_rows = sym.n;
  in.mcgs.num_colors = sym.num_colors;
  in.mcgs.perm = sym.perm.data();
  in.mcgs.color_start = sym.color_start.data();
  in.mcgs.dinv = no_dinv.data();
  in.mcgs.before = sliced_of(sym.sliced_before);
  in.mcgs.after = sliced_of(sym.sliced_after);
  in.num_values = nnz;
  in.before = part_of(sym.before);
  in.after = part_of(sym.after);
  if (values == SgsValues::fp64) {
    throw_on_error(spmv_hip_ilu0_plan_create(exec.context(), &in, &_ilu),
                   "spmv_hip_ilu0_plan_create");
  } else {
    throw_on_error(spmv_hip_ilu0_plan_create_ex(exec.context(), &in, 32, &_ilu),
                   "spmv_hip_ilu0_plan_create_ex");
    _value_bits = 32;
  }
  spmv_hip_mcgs_plan* inner = nullptr;
  spmv_hip_ilu0_mcgs_plan(_ilu, &inner);
  adopt(inner, sym.num_colors, std::move(sym.colors));
}

// Nothing of the matrix crosses to the host: the colouring of
// SgsPreconditioner's device setup (or the caller's colours), then
// spmv_hip_ilu0_plan_build on the arrays where they lie.
void Ilu0Preconditioner::symbolic_on_device(
    const CSRMatrix<double>* blk, int64_t n, const SgsOptions& options,
    std::chrono::steady_clock::time_point t0)
{
  const int64_t nnz = blk->non_zeros();
  if (n >= std::numeric_limits<int32_t>::max() || blk->cols() < n)
    throw std::runtime_error(
        "spmv::Ilu0Preconditioner - Error: rows and owned columns are not the "
        "same index range on this rank");
  spmv_hip_ctx* ctx = _exec.context();
  // an empty block owns no arrays
  const int32_t* rowptr = nnz > 0 ? blk->rowptr() : nullptr;
  const int32_t* colind = nnz > 0 ? blk->colind() : nullptr;

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
  int num_colors = 0, rounds = 0;
  if (options.colors) {
    int32_t lo = 0, hi = -1;
    for (int64_t i = 0; i < n; ++i) {
      lo = std::min(lo, options.colors[i]);
      hi = std::max(hi, options.colors[i]);
    }
    if (lo < 0)
      throw std::runtime_error(
          "spmv::Ilu0Preconditioner - Error: a colour is negative");
    num_colors = hi + 1;
    if (n > 0)
      _exec.copy_from<int32_t>(d_colors.p, _exec.get_host(), options.colors,
                               (size_t)n);
  } else {
    throw_on_error(
        spmv_hip_mcgs_color(ctx, (int32_t)n, blk->cols(), nnz, rowptr, colind,
                            _symmetric ? 1 : 0,
                            options.order == SgsOrder::natural
                                ? SPMV_HIP_MCGS_NATURAL
                                : SPMV_HIP_MCGS_HASHED,
                            d_colors.p, &num_colors, &rounds, nullptr),
        "spmv_hip_mcgs_color");
  }
  const double color_ms = ms_since(t0);

  int64_t info[SPMV_HIP_MCGS_INFO_WORDS] = {};
  const int rc
      = options.values == SgsValues::fp64
            ? spmv_hip_ilu0_plan_build(ctx, (int32_t)n, blk->cols(), nnz, rowptr,
                                       colind, _symmetric ? 1 : 0, d_colors.p,
                                       num_colors, kSgsLongThreshold, &_ilu,
                                       info, nullptr)
            : spmv_hip_ilu0_plan_build_ex(ctx, (int32_t)n, blk->cols(), nnz,
                                          rowptr, colind, _symmetric ? 1 : 0,
                                          d_colors.p, num_colors,
                                          kSgsLongThreshold, 32, &_ilu, info,
                                          nullptr);
  if (options.values == SgsValues::fp32)
    _value_bits = 32;
  if (rc == SPMV_HIP_EINVAL && info[1] == SPMV_HIP_ILU0_DUPLICATE)
    throw std::runtime_error(
        "spmv::ilu0_symbolic - Error: duplicate column in row "
        + std::to_string(info[3]) + " of the local diagonal block");
  if (rc == SPMV_HIP_EINVAL && info[1] == SPMV_HIP_MCGS_IMPROPER)
    throw std::runtime_error(
        "spmv::ilu0_symbolic - Error: the colouring is not proper (row "
        + std::to_string(info[3]) + ")");
  if (rc == SPMV_HIP_EINVAL && info[1] == SPMV_HIP_MCGS_UNWORN_COLOR)
    throw std::runtime_error(
        "spmv::Ilu0Preconditioner - Error: a colour below the largest is not "
        "worn by any row");
  if (rc == SPMV_HIP_EINVAL && info[1] == SPMV_HIP_MCGS_BAD_COLOR)
    throw std::runtime_error(
        "spmv::Ilu0Preconditioner - Error: a colour is out of range");
  throw_on_error(rc, "spmv_hip_ilu0_plan_build");
  int64_t sizes[SPMV_HIP_ILU0_SIZES_WORDS] = {};
  throw_on_error(spmv_hip_ilu0_plan_sizes(_ilu, sizes), "spmv_hip_ilu0_plan_sizes");
  _nbefore = sizes[1];
  _nafter = sizes[2];
  spmv_hip_mcgs_plan* inner = nullptr;
  spmv_hip_ilu0_mcgs_plan(_ilu, &inner);
  // (the colours stay on the device until colors() or pattern() asks)
  adopt(inner, num_colors, (int)n);
  set_setup_record(rounds, color_ms, ms_since(t0) - color_ms, info[2]);
}

Ilu0Preconditioner::~Ilu0Preconditioner()
{
  try {
    if (_ilu) // a sweep may still be in flight
      _exec.synchronize();
  } catch (...) {
  }
  _plan = nullptr; // the inner plan goes with its owner
  spmv_hip_ilu0_plan_destroy(_ilu);
  try {
    if (_diag)
      _exec.free(_diag);
  } catch (...) {
  }
}

void Ilu0Preconditioner::check_usable() const
{
  if (!_usable && _out_of_range)
    throw std::runtime_error(
        "spmv::Ilu0Preconditioner - Error: fp32 range: the last factorisation "
        "left entries that round to Inf, zero or an fp32 subnormal; refactor "
        "before using it");
  if (!_usable)
    throw std::runtime_error(
        "spmv::Ilu0Preconditioner - Error: the last factorisation met a pivot "
        "that is zero or not finite; refactor before using it");
}

void Ilu0Preconditioner::numeric(const Matrix<double>& A)
{
  const auto* blk = static_cast<const CSRMatrix<double>*>(A.local_block());
  const double* diagonal = blk->diagonal();
  if (!_symmetric && rows() > 0) {
    A.diagonal(_diag);
    diagonal = _diag;
  }
  _usable = false;
  _out_of_range = false;
  _negative = 0;
  spmv_hip_ctx* ctx = _exec.context();
  throw_on_error(spmv_hip_ilu0_factor(ctx, _ilu, blk->values(), diagonal, nullptr),
                 "spmv_hip_ilu0_factor");
  int64_t bad = 0, negative = 0, out_of_range = 0;
  if (_value_bits == 64)
    throw_on_error(spmv_hip_ilu0_pivots(ctx, _ilu, &bad, &negative, nullptr),
                   "spmv_hip_ilu0_pivots");
  else // the same wait, one more count
    throw_on_error(spmv_hip_ilu0_counts(ctx, _ilu, &bad, &negative, &out_of_range,
                                        nullptr),
                   "spmv_hip_ilu0_counts");
  if (bad != 0)
    throw std::runtime_error(
        "spmv::Ilu0Preconditioner - Error: " + std::to_string(bad) + " of "
        + std::to_string(rows()) + " pivot(s) are zero or not finite");
  if (out_of_range != 0) {
    _out_of_range = true;
    throw std::runtime_error(
        "spmv::Ilu0Preconditioner - Error: fp32 range: "
        + std::to_string(out_of_range)
        + " factor entries round to Inf, zero or an fp32 subnormal (values = "
          "fp32)");
  }
  _negative = negative;
  _usable = true;
}

void Ilu0Preconditioner::refactor(const Matrix<double>& A)
{
  const CSRMatrix<double>* blk = block_of(A, "::refactor");
  if (A.row_map()->local_size() != rows() || A.symmetric() != _symmetric
      || blk->non_zeros() != _num_values)
    throw std::runtime_error(
        "spmv::Ilu0Preconditioner::refactor - Error: not the pattern this "
        "object was built for (rows, storage or number of stored entries "
        "differ)");
  numeric(A);
}

int64_t Ilu0Preconditioner::plan_bytes() const
{
  int64_t bytes = 0;
  throw_on_error(spmv_hip_ilu0_plan_bytes(_ilu, &bytes),
                 "spmv_hip_ilu0_plan_bytes");
  return bytes + (_diag ? (int64_t)rows() * 8 : 0);
}

void Ilu0Preconditioner::pattern(int64_t* before_ptr, int32_t* before_col,
                                 int64_t* after_ptr, int32_t* after_col) const
{
  throw_on_error(spmv_hip_ilu0_get_pattern(_exec.context(), _ilu, before_ptr,
                                           before_col, after_ptr, after_col),
                 "spmv_hip_ilu0_get_pattern");
  // positions -> rows: perm, the stable counting sort of the colours (device
  // setup: fetched from the plan on the first call)
  const int32_t n = rows();
  std::vector<int32_t> next((size_t)_num_colors + 1, 0), perm((size_t)n);
  std::vector<int32_t> colour((size_t)n);
  colors(colour.data());
  for (int32_t i = 0; i < n; ++i)
    ++next[(size_t)colour[i] + 1];
  for (int c = 0; c < _num_colors; ++c)
    next[(size_t)c + 1] += next[c];
  for (int32_t i = 0; i < n; ++i)
    perm[(size_t)next[colour[i]]++] = i;
  if (before_col)
    for (int64_t e = 0; e < _nbefore; ++e)
      before_col[e] = perm[(size_t)before_col[e]];
  if (after_col)
    for (int64_t e = 0; e < _nafter; ++e)
      after_col[e] = perm[(size_t)after_col[e]];
}

void Ilu0Preconditioner::factor(double* l, double* u, double* d) const
{
  throw_on_error(
      spmv_hip_ilu0_get_factor(_exec.context(), _ilu, l, u, d, nullptr),
      "spmv_hip_ilu0_get_factor");
}

} // namespace spmv
