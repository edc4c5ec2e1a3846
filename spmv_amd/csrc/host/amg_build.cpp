// Host half of spmv::AmgPreconditioner: see amg_build.h.
#include "amg_build.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>

namespace spmv
{

AmgExpanded amg_expand(const int32_t* rowptr, const int32_t* colind,
                       int64_t nrows, int64_t ncols_local, bool symmetric)
{
  if (nrows < 0 || nrows != ncols_local)
    throw std::runtime_error(
        "spmv::amg_expand - Error: rows and owned columns are not the same "
        "index range");
  if (nrows > std::numeric_limits<int32_t>::max())
    throw std::runtime_error("spmv::amg_expand - Error: too many rows");
  AmgExpanded x;
  const int32_t n = (int32_t)nrows;
  x.n = n;
  x.symmetric = symmetric;
  x.ptr.assign((size_t)n + 1, 0);
  if (n == 0)
    return x;
  if (!rowptr)
    throw std::runtime_error("spmv::amg_expand - Error: NULL row pointer");
  const int64_t nnz = rowptr[n];
  if (rowptr[0] != 0 || nnz < 0 || (nnz > 0 && !colind))
    throw std::runtime_error("spmv::amg_expand - Error: bad row pointer");
  for (int32_t i = 0; i < n; ++i)
    if (rowptr[i + 1] < rowptr[i])
      throw std::runtime_error("spmv::amg_expand - Error: bad row pointer");
  x.num_values = nnz;
  // an entry of the level: general c < n, symmetric c < i
  auto kept = [&](int32_t i, int32_t c) {
    return c >= 0 && (symmetric ? c < i : c < n);
  };
  // lengths (symmetric: lower + 1 + mirrored)
  std::vector<int64_t>& ptr = x.ptr;
  for (int32_t i = 0; i < n; ++i) {
    if (symmetric)
      ++ptr[(size_t)i + 1];
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int32_t c = colind[e];
      if (!kept(i, c))
        continue;
      ++ptr[(size_t)i + 1];
      if (symmetric)
        ++ptr[(size_t)c + 1];
    }
  }
  for (int32_t i = 0; i < n; ++i)
    ptr[(size_t)i + 1] += ptr[i];
  x.col.resize((size_t)ptr[n]);
  x.src.resize((size_t)ptr[n]);
  std::vector<int64_t> next(ptr.begin(), ptr.end() - 1);
  // rows ascending: row i's own entries and its diagonal are placed when i is
  // visited, before any mirror image (those come from rows k > i, ascending)
  for (int32_t i = 0; i < n; ++i) {
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int32_t c = colind[e];
      if (!kept(i, c))
        continue;
      x.col[(size_t)next[i]] = c;
      x.src[(size_t)next[i]++] = (int32_t)e;
    }
    if (symmetric) {
      x.col[(size_t)next[i]] = i;
      x.src[(size_t)next[i]++] = ~i;
    }
  }
  if (symmetric)
    for (int32_t k = 0; k < n; ++k)
      for (int64_t e = rowptr[k]; e < rowptr[k + 1]; ++e) {
        const int32_t c = colind[e];
        if (!kept(k, c))
          continue;
        x.col[(size_t)next[c]] = k;
        x.src[(size_t)next[c]++] = (int32_t)e;
      }
  return x;
}

AmgStep amg_aggregate(const AmgExpanded& x, const double* values,
                      const double* diagonal, double theta)
{
  const int32_t n = x.n;
  AmgStep s;
  s.n = n;
  s.agg.assign((size_t)n, -1);
  auto value = [&](int64_t e) {
    const int32_t q = x.src[(size_t)e];
    return q >= 0 ? values[q] : diagonal[~q];
  };
  // strong(i), CSR
  std::vector<int64_t> sptr((size_t)n + 1, 0);
  std::vector<int32_t> scol;
  std::vector<int32_t> seen((size_t)n, -1);
  for (int32_t i = 0; i < n; ++i) {
    double m = 0.0;
    for (int64_t e = x.ptr[i]; e < x.ptr[(size_t)i + 1]; ++e)
      if (x.col[(size_t)e] != i) {
        const double a = std::fabs(value(e));
        if (a > m)
          m = a;
      }
    const double bar = theta * m;
    for (int64_t e = x.ptr[i]; e < x.ptr[(size_t)i + 1]; ++e) {
      const int32_t j = x.col[(size_t)e];
      if (j == i)
        continue;
      const double a = value(e);
      if (a != 0.0 && std::fabs(a) >= bar && seen[(size_t)j] != i) {
        seen[(size_t)j] = i;
        scol.push_back(j);
      }
    }
    sptr[(size_t)i + 1] = (int64_t)scol.size();
  }
  std::vector<int32_t>& agg = s.agg;
  int32_t n_agg = 0;
  // pass 1
  for (int32_t i = 0; i < n; ++i) {
    if (agg[(size_t)i] >= 0)
      continue;
    bool all_free = true;
    for (int64_t e = sptr[i]; e < sptr[(size_t)i + 1] && all_free; ++e)
      all_free = agg[(size_t)scol[(size_t)e]] < 0;
    if (!all_free)
      continue;
    agg[(size_t)i] = n_agg;
    for (int64_t e = sptr[i]; e < sptr[(size_t)i + 1]; ++e)
      agg[(size_t)scol[(size_t)e]] = n_agg;
    ++n_agg;
  }
  // pass 2
  {
    const std::vector<int32_t> snapshot(agg);
    for (int32_t i = 0; i < n; ++i) {
      if (snapshot[(size_t)i] >= 0)
        continue;
      for (int64_t e = sptr[i]; e < sptr[(size_t)i + 1]; ++e) {
        const int32_t a = snapshot[(size_t)scol[(size_t)e]];
        if (a >= 0) {
          agg[(size_t)i] = a;
          break;
        }
      }
    }
  }
  // pass 3
  for (int32_t i = 0; i < n; ++i) {
    if (agg[(size_t)i] >= 0)
      continue;
    agg[(size_t)i] = n_agg;
    for (int64_t e = sptr[i]; e < sptr[(size_t)i + 1]; ++e) {
      int32_t& a = agg[(size_t)scol[(size_t)e]];
      if (a < 0)
        a = n_agg;
    }
    ++n_agg;
  }
  s.n_agg = n_agg;
  // members, ascending by row (a counting sort in row order)
  s.member_ptr.assign((size_t)n_agg + 1, 0);
  for (int32_t i = 0; i < n; ++i)
    ++s.member_ptr[(size_t)agg[(size_t)i] + 1];
  for (int32_t a = 0; a < n_agg; ++a)
    s.member_ptr[(size_t)a + 1] += s.member_ptr[a];
  s.member.resize((size_t)n);
  std::vector<int32_t> next(s.member_ptr.begin(), s.member_ptr.end() - 1);
  for (int32_t i = 0; i < n; ++i)
    s.member[(size_t)next[(size_t)agg[(size_t)i]]++] = i;
  return s;
}

void amg_galerkin_pattern(const AmgExpanded& x, AmgStep* step)
{
  AmgStep& s = *step;
  const int32_t n_agg = s.n_agg;
  s.rowptr.assign((size_t)n_agg + 1, 0);
  s.colind.clear();
  s.src_ptr.assign(1, 0);
  s.src.clear();
  s.src.reserve(x.src.size());
  // per coarse row: the distinct J, sorted; then the lists by counting
  std::vector<int32_t> slot((size_t)n_agg, -1); // J -> index in this row
  std::vector<int32_t> cols;
  std::vector<int64_t> count, fill;
  for (int32_t I = 0; I < n_agg; ++I) {
    cols.clear();
    const int32_t m0 = s.member_ptr[I], m1 = s.member_ptr[(size_t)I + 1];
    for (int32_t m = m0; m < m1; ++m) {
      const int32_t i = s.member[(size_t)m];
      for (int64_t e = x.ptr[i]; e < x.ptr[(size_t)i + 1]; ++e) {
        const int32_t J = s.agg[(size_t)x.col[(size_t)e]];
        if (slot[(size_t)J] < 0) {
          slot[(size_t)J] = 0;
          cols.push_back(J);
        }
      }
    }
    std::sort(cols.begin(), cols.end());
    for (size_t k = 0; k < cols.size(); ++k)
      slot[(size_t)cols[k]] = (int32_t)k;
    count.assign(cols.size() + 1, 0);
    for (int32_t m = m0; m < m1; ++m) {
      const int32_t i = s.member[(size_t)m];
      for (int64_t e = x.ptr[i]; e < x.ptr[(size_t)i + 1]; ++e)
        ++count[(size_t)slot[(size_t)s.agg[(size_t)x.col[(size_t)e]]] + 1];
    }
    const int64_t base = (int64_t)s.src.size();
    for (size_t k = 0; k < cols.size(); ++k)
      count[k + 1] += count[k];
    s.src.resize((size_t)(base + count[cols.size()]));
    fill.assign(count.begin(), count.end() - 1);
    for (int32_t m = m0; m < m1; ++m) {
      const int32_t i = s.member[(size_t)m];
      for (int64_t e = x.ptr[i]; e < x.ptr[(size_t)i + 1]; ++e) {
        const int32_t k = slot[(size_t)s.agg[(size_t)x.col[(size_t)e]]];
        s.src[(size_t)(base + fill[(size_t)k]++)] = x.src[(size_t)e];
      }
    }
    if ((int64_t)s.colind.size() + (int64_t)cols.size()
        > std::numeric_limits<int32_t>::max())
      throw std::runtime_error(
          "spmv::amg_galerkin_pattern - Error: too many coarse entries");
    for (size_t k = 0; k < cols.size(); ++k) {
      s.colind.push_back(cols[k]);
      s.src_ptr.push_back(base + count[k + 1]);
      slot[(size_t)cols[k]] = -1;
    }
    s.rowptr[(size_t)I + 1] = (int32_t)s.colind.size();
  }
}

} // namespace spmv
