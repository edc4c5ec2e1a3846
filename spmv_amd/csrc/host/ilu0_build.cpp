// Symbolic setup of the multicolour ILU(0): see ilu0_build.h.
#include "ilu0_build.h"

#include <algorithm>
#include <stdexcept>
#include <string>
#include <utility>

namespace spmv
{

namespace
{

// where the entries of `part` lie in `s` = sgs_slice(part): sgs_build.h's rule
void fill_slots(const Ilu0Symbolic& sym, const SgsSlicedPart& s, Ilu0Part& part)
{
  part.slot.assign(part.cpos.size(), 0);
  for (int c = 0; c < sym.num_colors; ++c) {
    const int32_t c1 = sym.color_start[(size_t)c + 1];
    for (int32_t sl = s.color_slice[c]; sl < s.color_slice[(size_t)c + 1]; ++sl) {
      const int32_t p0 = s.slice_pos0[sl];
      const int32_t p1 = std::min<int32_t>(p0 + 64, c1);
      for (int32_t pos = p0; pos < p1; ++pos)
        for (int32_t k = 0; k < s.len[pos]; ++k) // (a long row: len = -1)
          part.slot[(size_t)part.ptr[pos] + k]
              = s.slice_ptr[sl] + (int64_t)k * 64 + (pos - p0);
    }
  }
  for (size_t l = 0; l < s.long_pos.size(); ++l) {
    const int32_t pos = s.long_pos[l];
    const int64_t m = part.ptr[(size_t)pos + 1] - part.ptr[pos];
    for (int64_t k = 0; k < m; ++k)
      part.slot[(size_t)(part.ptr[pos] + k)] = ~(s.long_ptr[l] + k);
  }
}

} // namespace

Ilu0Symbolic ilu0_symbolic(const int32_t* rowptr, const int32_t* colind,
                           int64_t nrows, int64_t ncols_local, bool symmetric,
                           int long_threshold)
{
  Ilu0Symbolic sym;
  int ncol = 0;
  if (nrows != ncols_local) // pos and colors are indexed by columns < ncols_local
    throw std::runtime_error(
        "spmv::ilu0_symbolic - Error: rows and owned columns are not the same "
        "index range");
  // (checks the rest of the input: monotone rowptr, no negative column)
  sym.colors = sgs_color(rowptr, colind, nrows, ncols_local, symmetric, &ncol);
  const int32_t n = sym.n = (int32_t)nrows;
  sym.num_colors = ncol;

  // colour-major, natural order within a colour: sgs_build's counting sort
  sym.color_start.assign((size_t)ncol + 1, 0);
  for (int32_t i = 0; i < n; ++i)
    ++sym.color_start[(size_t)sym.colors[i] + 1];
  for (int c = 0; c < ncol; ++c)
    sym.color_start[(size_t)c + 1] += sym.color_start[c];
  sym.perm.resize((size_t)n);
  sym.pos.resize((size_t)n);
  {
    std::vector<int32_t> next(sym.color_start.begin(), sym.color_start.end() - 1);
    for (int32_t i = 0; i < n; ++i) {
      const int32_t p = next[sym.colors[i]]++;
      sym.perm[(size_t)p] = i;
      sym.pos[(size_t)i] = p;
    }
  }

  auto stored = [&](int32_t i, int32_t c) { // an off-diagonal entry, as stored
    return c < ncols_local && c != i && (!symmetric || c < i);
  };

  // symmetric storage: the stored entries of column i, with their indices
  std::vector<int64_t> mptr;
  std::vector<int32_t> mrow, msrc;
  if (symmetric) {
    mptr.assign((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; ++i)
      for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e)
        if (stored(i, colind[e]))
          ++mptr[(size_t)colind[e] + 1];
    for (int32_t c = 0; c < n; ++c)
      mptr[(size_t)c + 1] += mptr[c];
    mrow.resize((size_t)mptr[n]);
    msrc.resize((size_t)mptr[n]);
    std::vector<int64_t> next(mptr.begin(), mptr.end() - 1);
    for (int32_t i = 0; i < n; ++i)
      for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e)
        if (stored(i, colind[e])) {
          const int64_t at = next[colind[e]]++;
          mrow[(size_t)at] = i;
          msrc[(size_t)at] = e;
        }
  }

  // the parts by column (what sgs_slice lays out), in position order
  SgsCsrPart cols_before, cols_after;
  cols_before.ptr.assign((size_t)n + 1, 0);
  cols_after.ptr.assign((size_t)n + 1, 0);
  sym.before.ptr.assign((size_t)n + 1, 0);
  sym.after.ptr.assign((size_t)n + 1, 0);
  struct Entry {
    int32_t cpos, col, src;
  };
  std::vector<Entry> row;
  for (int32_t p = 0; p < n; ++p) {
    const int32_t i = sym.perm[p];
    row.clear();
    for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e)
      if (stored(i, colind[e]))
        row.push_back({sym.pos[colind[e]], colind[e], e});
    if (symmetric)
      for (int64_t e = mptr[i]; e < mptr[(size_t)i + 1]; ++e)
        row.push_back({sym.pos[mrow[(size_t)e]], mrow[(size_t)e], msrc[(size_t)e]});
    std::sort(row.begin(), row.end(),
              [](const Entry& a, const Entry& b) { return a.cpos < b.cpos; });
    const int32_t ci = sym.colors[i];
    for (size_t k = 0; k < row.size(); ++k) {
      if (k > 0 && row[k].cpos == row[k - 1].cpos)
        throw std::runtime_error(
            "spmv::ilu0_symbolic - Error: duplicate column " + std::to_string(row[k].col)
            + " in row " + std::to_string(i) + " of the local diagonal block");
      const int32_t cc = sym.colors[row[k].col];
      if (cc == ci)
        throw std::runtime_error(
            "spmv::ilu0_symbolic - Error: the colouring is not proper (row "
            + std::to_string(i) + ", column " + std::to_string(row[k].col) + ")");
      Ilu0Part& part = cc < ci ? sym.before : sym.after;
      part.cpos.push_back(row[k].cpos);
      part.src.push_back(row[k].src);
      (cc < ci ? cols_before : cols_after).col.push_back(row[k].col);
    }
    sym.before.ptr[(size_t)p + 1] = (int64_t)sym.before.cpos.size();
    sym.after.ptr[(size_t)p + 1] = (int64_t)sym.after.cpos.size();
  }
  cols_before.ptr = sym.before.ptr;
  cols_after.ptr = sym.after.ptr;
  cols_before.val.assign(cols_before.col.size(), 0.0);
  cols_after.val.assign(cols_after.col.size(), 0.0);

  // sgs_slice reads n, num_colors and color_start of the plan
  SgsHostPlan shape;
  shape.n = n;
  shape.num_colors = ncol;
  shape.color_start = sym.color_start;
  sym.sliced_before = sgs_slice(shape, cols_before, long_threshold);
  cols_before = SgsCsrPart();
  sym.sliced_after = sgs_slice(shape, cols_after, long_threshold);
  cols_after = SgsCsrPart();
  fill_slots(sym, sym.sliced_before, sym.before);
  fill_slots(sym, sym.sliced_after, sym.after);
  return sym;
}

} // namespace spmv
