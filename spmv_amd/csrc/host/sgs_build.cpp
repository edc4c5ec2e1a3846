// Colouring and colour-major copy of the local diagonal block: see sgs_build.h.
#include "sgs_build.h"

#include <algorithm>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>

namespace spmv
{

namespace
{

void check_input(const int32_t* rowptr, const int32_t* colind, int64_t nrows,
                 int64_t ncols_local)
{
  if (nrows < 0 || nrows != ncols_local
      || nrows > std::numeric_limits<int32_t>::max())
    throw std::runtime_error(
        "spmv::sgs_build - Error: rows and owned columns are not the same "
        "index range");
  if (nrows > 0 && !rowptr)
    throw std::runtime_error("spmv::sgs_build - Error: NULL rowptr");
  if (nrows > 0 && rowptr[nrows] > rowptr[0] && !colind)
    throw std::runtime_error("spmv::sgs_build - Error: NULL colind");
  for (int64_t i = 0; i < nrows; ++i)
    if (rowptr[i + 1] < rowptr[i] || rowptr[i] < 0)
      throw std::runtime_error("spmv::sgs_build - Error: rowptr is not monotone");
  for (int64_t e = nrows ? rowptr[0] : 0; e < (nrows ? rowptr[nrows] : 0); ++e)
    if (colind[e] < 0)
      throw std::runtime_error("spmv::sgs_build - Error: negative column");
}

// an off-diagonal entry of the local diagonal block, as stored
inline bool off_diagonal(int32_t i, int32_t c, int64_t ncols_local,
                         bool symmetric)
{
  return c < ncols_local && c != i && (!symmetric || c < i);
}

// Stable transpose of the stored entries (i, c) that `keep` selects: row c of
// the result lists the rows i in ascending order, duplicates in storage order.
// `values` may be NULL (pattern only).
struct Transposed {
  std::vector<int64_t> ptr;
  std::vector<int32_t> row;
  std::vector<double> val;
};

template <class Keep>
Transposed transpose(const int32_t* rowptr, const int32_t* colind,
                     const double* values, int32_t n, Keep&& keep)
{
  Transposed t;
  t.ptr.assign((size_t)n + 1, 0);
  for (int32_t i = 0; i < n; ++i)
    for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e)
      if (keep(i, colind[e]))
        ++t.ptr[(size_t)colind[e] + 1];
  for (int32_t c = 0; c < n; ++c)
    t.ptr[(size_t)c + 1] += t.ptr[c];
  t.row.resize((size_t)t.ptr[n]);
  if (values)
    t.val.resize((size_t)t.ptr[n]);
  std::vector<int64_t> next(t.ptr.begin(), t.ptr.end() - 1);
  for (int32_t i = 0; i < n; ++i)
    for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e)
      if (keep(i, colind[e])) {
        const int64_t at = next[colind[e]]++;
        t.row[(size_t)at] = i;
        if (values)
          t.val[(size_t)at] = values[e];
      }
  return t;
}

} // namespace

std::vector<int32_t> sgs_color(const int32_t* rowptr, const int32_t* colind,
                               int64_t nrows, int64_t ncols_local,
                               bool symmetric, int* num_colors)
{
  check_input(rowptr, colind, nrows, ncols_local);
  const int32_t n = (int32_t)nrows;
  // The neighbours j < i of row i in B + B^T: the entries (i, j), j < i, of the
  // row itself and the rows j < i that hold an entry (j, i) -- the transposed
  // pattern of the entries above the diagonal.  Symmetric input has none.
  Transposed upper;
  if (!symmetric)
    upper = transpose(rowptr, colind, nullptr, n, [&](int32_t i, int32_t c) {
      return c < ncols_local && c > i;
    });
  std::vector<int32_t> colour((size_t)n, -1);
  std::vector<int32_t> worn(1, -1); // worn[c] == i: a neighbour of i wears c
  int ncol = 0;
  for (int32_t i = 0; i < n; ++i) {
    for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e)
      if (colind[e] < i)
        worn[(size_t)colour[colind[e]]] = i;
    if (!symmetric)
      for (int64_t e = upper.ptr[i]; e < upper.ptr[(size_t)i + 1]; ++e)
        worn[(size_t)colour[upper.row[(size_t)e]]] = i;
    int32_t c = 0;
    while (c < ncol && worn[(size_t)c] == i)
      ++c;
    colour[i] = c;
    if (c == ncol) {
      ++ncol;
      worn.push_back(-1); // worn.size() == ncol + 1
    }
  }
  if (num_colors)
    *num_colors = ncol;
  return colour;
}

SgsHostPlan sgs_build(const int32_t* rowptr, const int32_t* colind,
                      const double* values, const double* diagonal,
                      int64_t nrows, int64_t ncols_local, bool symmetric)
{
  SgsHostPlan plan;
  int ncol = 0;
  plan.colors = sgs_color(rowptr, colind, nrows, ncols_local, symmetric, &ncol);
  const int32_t n = plan.n = (int32_t)nrows;
  plan.num_colors = ncol;
  if (n > 0 && rowptr[n] > rowptr[0] && !values)
    throw std::runtime_error("spmv::sgs_build - Error: NULL values");

  // colour-major, natural order within a colour: a stable counting sort
  plan.color_start.assign((size_t)ncol + 1, 0);
  for (int32_t i = 0; i < n; ++i)
    ++plan.color_start[(size_t)plan.colors[i] + 1];
  for (int c = 0; c < ncol; ++c)
    plan.color_start[(size_t)c + 1] += plan.color_start[c];
  plan.perm.resize((size_t)n);
  {
    std::vector<int32_t> next(plan.color_start.begin(),
                              plan.color_start.end() - 1);
    for (int32_t i = 0; i < n; ++i)
      plan.perm[(size_t)next[plan.colors[i]]++] = i;
  }

  // the diagonal: Matrix::diagonal's rule
  plan.d.assign((size_t)n, 0.0);
  for (int32_t i = 0; i < n; ++i) {
    if (diagonal) {
      plan.d[i] = diagonal[i];
      continue;
    }
    double acc = 0;
    for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e)
      if (colind[e] == i)
        acc += values[e];
    plan.d[i] = acc;
  }

  // symmetric storage: the entries of column i of the stored block
  Transposed mirror;
  if (symmetric)
    mirror = transpose(rowptr, colind, values, n, [&](int32_t i, int32_t c) {
      return off_diagonal(i, c, ncols_local, true);
    });

  plan.before.ptr.assign((size_t)n + 1, 0);
  plan.after.ptr.assign((size_t)n + 1, 0);
  std::vector<std::pair<int32_t, double>> row;
  for (int32_t pos = 0; pos < n; ++pos) {
    const int32_t i = plan.perm[pos];
    row.clear();
    for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e)
      if (off_diagonal(i, colind[e], ncols_local, symmetric))
        row.emplace_back(colind[e], values[e]);
    if (symmetric)
      for (int64_t e = mirror.ptr[i]; e < mirror.ptr[(size_t)i + 1]; ++e)
        row.emplace_back(mirror.row[(size_t)e], mirror.val[(size_t)e]);
    auto by_col = [](const std::pair<int32_t, double>& a,
                     const std::pair<int32_t, double>& b) {
      return a.first < b.first;
    };
    if (!std::is_sorted(row.begin(), row.end(), by_col))
      std::stable_sort(row.begin(), row.end(), by_col);
    const int32_t ci = plan.colors[i];
    for (const auto& cv : row) {
      const int32_t cc = plan.colors[cv.first];
      if (cc == ci)
        throw std::runtime_error(
            "spmv::sgs_build - Error: the colouring is not proper (row "
            + std::to_string(i) + ", column " + std::to_string(cv.first) + ")");
      SgsCsrPart& part = cc < ci ? plan.before : plan.after;
      part.col.push_back(cv.first);
      part.val.push_back(cv.second);
    }
    plan.before.ptr[(size_t)pos + 1] = (int64_t)plan.before.col.size();
    plan.after.ptr[(size_t)pos + 1] = (int64_t)plan.after.col.size();
  }
  return plan;
}

SgsSlicedPart sgs_slice(const SgsHostPlan& plan, const SgsCsrPart& part,
                        int long_threshold)
{
  const int32_t n = plan.n;
  const int ncol = plan.num_colors;
  if ((int64_t)part.ptr.size() != (int64_t)n + 1)
    throw std::runtime_error("spmv::sgs_slice - Error: the part is not of this plan");
  SgsSlicedPart s;
  s.len.assign((size_t)n, 0);
  s.color_slice.assign((size_t)ncol + 1, 0);
  s.color_long.assign((size_t)ncol + 1, 0);
  s.slice_ptr.push_back(0);
  s.long_ptr.push_back(0);
  for (int c = 0; c < ncol; ++c) {
    const int32_t c0 = plan.color_start[c], c1 = plan.color_start[(size_t)c + 1];
    for (int32_t p0 = c0; p0 < c1; p0 += 64) {
      const int32_t p1 = std::min<int32_t>(p0 + 64, c1);
      int64_t width = 0;
      for (int32_t pos = p0; pos < p1; ++pos) {
        const int64_t m = part.ptr[(size_t)pos + 1] - part.ptr[pos];
        if (m > long_threshold) {
          s.len[pos] = -1;
          s.long_pos.push_back(pos);
          s.long_col.insert(s.long_col.end(), part.col.begin() + part.ptr[pos],
                            part.col.begin() + part.ptr[(size_t)pos + 1]);
          s.long_val.insert(s.long_val.end(), part.val.begin() + part.ptr[pos],
                            part.val.begin() + part.ptr[(size_t)pos + 1]);
          s.long_ptr.push_back((int64_t)s.long_col.size());
        } else {
          s.len[pos] = (int32_t)m;
          width = std::max(width, m);
        }
      }
      const size_t base = s.col.size();
      s.col.resize(base + (size_t)width * 64, 0);
      s.val.resize(base + (size_t)width * 64, 0.0);
      for (int32_t pos = p0; pos < p1; ++pos)
        for (int32_t k = 0; k < s.len[pos]; ++k) {
          const size_t at = base + (size_t)k * 64 + (size_t)(pos - p0);
          s.col[at] = part.col[(size_t)part.ptr[pos] + k];
          s.val[at] = part.val[(size_t)part.ptr[pos] + k];
        }
      s.slice_pos0.push_back(p0);
      s.slice_ptr.push_back((int64_t)s.col.size());
    }
    s.color_slice[(size_t)c + 1] = (int32_t)s.slice_pos0.size();
    s.color_long[(size_t)c + 1] = (int32_t)s.long_pos.size();
  }
  return s;
}

} // namespace spmv
