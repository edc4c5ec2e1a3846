// Stand-alone check of the host half of the multicolour ILU(0) preconditioner
// (spmv_amd/csrc/host/ilu0_build.{h,cpp} on sgs_build.{h,cpp}): the symbolic
// setup on the CPU, meant to be built with the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ispmv_amd/csrc/host tools/ilu0_build_check.cpp
//       spmv_amd/csrc/host/ilu0_build.cpp spmv_amd/csrc/host/sgs_build.cpp
//       -o ilu0_build_check && ./ilu0_build_check
//
// Matrices: 7-point Poisson on 5^3 and 11^3, a nonsymmetric band of 257 rows
// (offsets 1, 37), the arrow matrix of 130 rows (a hub row of 129 entries: the
// long list), a ragged symmetric matrix of 1 001 rows with a hub row of about
// 300 entries, a diagonal matrix, n = 1, n = 0; the symmetric ones also in the
// symmetric input form.  Checked: perm / pos are inverse colour-major
// permutations; the two parts hold every off-diagonal entry of the block once,
// ascending by position, with the source index of its value; every slot is used
// once and holds the entry's column in the sliced layout; a duplicate column is
// refused.  Then the factorisation is run on the host THROUGH the slot map, the
// numbers living in the sliced value arrays as the sweeps read them, and
// compared bit for bit with the plain restatement of cg.h's definition (maps of
// position -> value, row after row), read back with the kernel's indexing.
// Exit status 0 and "ilu0_build_check: OK" when everything holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ilu0_build.h"

using namespace spmv;

namespace
{

int failures = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (++failures <= 20) {                                                  \
        std::printf("FAILED %s:%d: ", __FILE__, __LINE__);                     \
        std::printf(__VA_ARGS__);                                              \
        std::printf("\n");                                                     \
      }                                                                        \
    }                                                                          \
  } while (0)

struct Csr {
  std::vector<int32_t> rowptr = {0}, colind;
  std::vector<double> values;
  int32_t n() const { return (int32_t)rowptr.size() - 1; }
};

Csr from_map(int32_t n, const std::vector<std::map<int32_t, double>>& rows)
{
  Csr m;
  for (int32_t i = 0; i < n; ++i) {
    for (const auto& cv : rows[i]) {
      m.colind.push_back(cv.first);
      m.values.push_back(cv.second);
    }
    m.rowptr.push_back((int32_t)m.colind.size());
  }
  return m;
}

Csr poisson(int32_t n)
{
  const int32_t N = n * n * n;
  std::vector<std::map<int32_t, double>> rows(N);
  for (int32_t i = 0; i < N; ++i) {
    const int32_t c[3] = {i % n, (i / n) % n, i / (n * n)};
    rows[i][i] = 6.0 + 0.01 * (i % 7);
    int32_t stride = 1;
    for (int d = 0; d < 3; ++d, stride *= n) {
      if (c[d] > 0)
        rows[i][i - stride] = -1.0 - 0.001 * ((i + (i - stride)) % 5);
      if (c[d] < n - 1)
        rows[i][i + stride] = -1.0 - 0.001 * ((i + (i + stride)) % 5);
    }
  }
  return from_map(N, rows);
}

Csr banded(int32_t n)
{
  std::vector<std::map<int32_t, double>> rows(n);
  for (int32_t i = 0; i < n; ++i) {
    rows[i][i] = 6.0 + 0.3 * std::sin((double)i);
    for (int32_t d : {1, 37})
      if (i + d < n) {
        rows[i][i + d] = -(0.3 + 0.25 * std::sin((double)(3 * i + 2 * d)));
        rows[i + d][i] = -(0.5 + 0.4 * std::cos((double)(2 * i + d)));
      }
  }
  return from_map(n, rows);
}

Csr arrow(int32_t n)
{
  std::vector<std::map<int32_t, double>> rows(n);
  double sum = 0;
  for (int32_t i = 0; i + 1 < n; ++i) {
    rows[i][i] = 2.0 + 0.5 * std::sin(3.0 * i);
    rows[i][n - 1] = -(0.5 + 0.4 * std::sin((double)i));
    rows[n - 1][i] = -(0.3 + 0.25 * std::cos(2.0 * i));
    sum += std::fabs(rows[n - 1][i]);
  }
  rows[n - 1][n - 1] = sum + 3.0;
  return from_map(n, rows);
}

Csr ragged(int32_t n, unsigned seed)
{
  std::mt19937 rng(seed);
  std::vector<std::map<int32_t, double>> rows(n);
  auto couple = [&](int32_t a, int32_t b) {
    if (a == b || a == 7 || b == 7)
      return;
    const double v = -0.1 - 0.9 * (double)(rng() % 1000) / 1000.0;
    rows[a][b] = v;
    rows[b][a] = v;
  };
  for (int32_t i = 0; i < n; ++i)
    for (unsigned k = rng() % 12; k > 0; --k)
      couple(i, (int32_t)(rng() % (unsigned)n));
  for (int32_t i = n - 12; i < n; ++i)
    for (int32_t j = i + 1; j < n; ++j)
      couple(i, j);
  for (int k = 0; k < 300; ++k)
    couple(100, (int32_t)(rng() % (unsigned)n));
  for (int32_t i = 0; i < n; ++i) {
    double off = 0;
    for (const auto& cv : rows[i])
      off += std::fabs(cv.second);
    rows[i][i] = off + 1.0 + (double)(rng() % 100) / 100.0;
  }
  return from_map(n, rows);
}

Csr lower_of(const Csr& m)
{
  Csr l;
  for (int32_t i = 0; i < m.n(); ++i) {
    for (int32_t e = m.rowptr[i]; e < m.rowptr[i + 1]; ++e)
      if (m.colind[e] <= i) {
        l.colind.push_back(m.colind[e]);
        l.values.push_back(m.values[e]);
      }
    l.rowptr.push_back((int32_t)l.colind.size());
  }
  return l;
}

// the value of a part's entry (pos, k) read with the kernel's indexing
// (spmv_mcgs.hip): a slice of 64 positions column-major, or the long list
double& sliced_at(const Ilu0Symbolic& y, SgsSlicedPart& s, int32_t pos, int64_t k,
                  int32_t* col)
{
  if (s.len[pos] < 0) {
    for (size_t l = 0; l < s.long_pos.size(); ++l)
      if (s.long_pos[l] == pos) {
        *col = s.long_col[(size_t)(s.long_ptr[l] + k)];
        return s.long_val[(size_t)(s.long_ptr[l] + k)];
      }
    throw std::runtime_error("a long row is not in the long list");
  }
  const int c = y.colors[y.perm[pos]];
  const int32_t sl = s.color_slice[c] + (pos - y.color_start[c]) / 64;
  const int64_t at = s.slice_ptr[sl] + 64 * k + (pos - s.slice_pos0[sl]);
  *col = s.col[(size_t)at];
  return s.val[(size_t)at];
}

void check(const char* name, const Csr& m, bool symmetric, int want_colors = -1)
{
  const int32_t n = m.n();
  Ilu0Symbolic y = ilu0_symbolic(m.rowptr.data(), m.colind.data(), n, n, symmetric);
  CHECK(y.n == n, "%s: n", name);
  if (want_colors >= 0)
    CHECK(y.num_colors == want_colors, "%s: %d colours", name, y.num_colors);
  // permutations
  CHECK((int32_t)y.perm.size() == n && (int32_t)y.pos.size() == n, "%s: sizes", name);
  for (int32_t p = 0; p < n; ++p) {
    CHECK(y.pos[y.perm[p]] == p, "%s: pos(perm(%d))", name, p);
    if (p > 0)
      CHECK(y.colors[y.perm[p - 1]] < y.colors[y.perm[p]]
                || (y.colors[y.perm[p - 1]] == y.colors[y.perm[p]]
                    && y.perm[p - 1] < y.perm[p]),
            "%s: order at position %d", name, p);
  }
  // the entries of the block, by (row, column) -> source index
  std::map<std::pair<int32_t, int32_t>, int32_t> want;
  for (int32_t i = 0; i < n; ++i)
    for (int32_t e = m.rowptr[i]; e < m.rowptr[i + 1]; ++e) {
      const int32_t c = m.colind[e];
      if (c >= n || c == i || (symmetric && c > i))
        continue;
      want[{i, c}] = e;
      if (symmetric)
        want[{c, i}] = e;
    }
  size_t seen = 0;
  Ilu0Part* parts[2] = {&y.before, &y.after};
  SgsSlicedPart* sliced[2] = {&y.sliced_before, &y.sliced_after};
  for (int h = 0; h < 2; ++h) {
    const Ilu0Part& p = *parts[h];
    std::set<int64_t> slots;
    CHECK((int32_t)p.ptr.size() == n + 1 && p.ptr[0] == 0, "%s: ptr", name);
    for (int32_t pos = 0; pos < n; ++pos) {
      const int32_t i = y.perm[pos];
      for (int64_t e = p.ptr[pos]; e < p.ptr[(size_t)pos + 1]; ++e) {
        const int32_t q = p.cpos[(size_t)e], j = y.perm[q];
        ++seen;
        CHECK(e == p.ptr[pos] || p.cpos[(size_t)e - 1] < q, "%s: order in row %d",
              name, i);
        CHECK(h == 0 ? y.colors[j] < y.colors[i] : y.colors[j] > y.colors[i],
              "%s: part of (%d, %d)", name, i, j);
        const auto it = want.find({i, j});
        CHECK(it != want.end() && it->second == p.src[(size_t)e],
              "%s: source of (%d, %d)", name, i, j);
        CHECK(slots.insert(p.slot[(size_t)e]).second, "%s: slot twice", name);
        int32_t col = -1;
        double& v = sliced_at(y, *sliced[h], pos, e - p.ptr[pos], &col);
        CHECK(col == j, "%s: column at (%d, %d)", name, i, j);
        const int64_t s = p.slot[(size_t)e];
        double* by_slot = s >= 0 ? &sliced[h]->val[(size_t)s]
                                 : &sliced[h]->long_val[(size_t)~s];
        CHECK(by_slot == &v, "%s: slot of (%d, %d)", name, i, j);
      }
    }
  }
  CHECK(seen == want.size(), "%s: %zu entries, %zu wanted", name, seen, want.size());

  // the diagonal: Matrix::diagonal's rule
  std::vector<double> diag((size_t)n, 0.0);
  for (int32_t i = 0; i < n; ++i)
    for (int32_t e = m.rowptr[i]; e < m.rowptr[i + 1]; ++e)
      if (m.colind[e] == i)
        diag[i] += m.values[e];

  // (a) the plain restatement: maps of position -> value
  std::vector<std::map<int32_t, double>> low((size_t)n), up((size_t)n);
  std::vector<double> d((size_t)n), dinv((size_t)n);
  for (int h = 0; h < 2; ++h)
    for (int32_t pos = 0; pos < n; ++pos)
      for (int64_t e = parts[h]->ptr[pos]; e < parts[h]->ptr[(size_t)pos + 1]; ++e)
        (h == 0 ? low : up)[pos][parts[h]->cpos[(size_t)e]]
            = m.values[(size_t)parts[h]->src[(size_t)e]];
  for (int32_t pos = 0; pos < n; ++pos) {
    double wd = diag[y.perm[pos]];
    for (auto& kv : low[pos]) { // ascending pos(k); kv.second is final here
      const double mult = kv.second * dinv[kv.first];
      for (const auto& ju : up[kv.first]) {
        double* w = nullptr;
        if (ju.first == pos)
          w = &wd;
        else if (low[pos].count(ju.first))
          w = &low[pos][ju.first];
        else if (up[pos].count(ju.first))
          w = &up[pos][ju.first];
        if (w) {
          const double prod = mult * ju.second;
          *w = *w - prod;
        }
      }
    }
    d[pos] = wd;
    dinv[pos] = 1.0 / wd;
  }

  // (b) through the slot map, the numbers in the sliced arrays
  auto at = [&](int h, int64_t e) -> double& {
    const int64_t s = parts[h]->slot[(size_t)e];
    return s >= 0 ? sliced[h]->val[(size_t)s] : sliced[h]->long_val[(size_t)~s];
  };
  for (int h = 0; h < 2; ++h)
    for (size_t e = 0; e < parts[h]->cpos.size(); ++e)
      at(h, (int64_t)e) = m.values[(size_t)parts[h]->src[e]];
  std::vector<double> d2((size_t)n), dinv2((size_t)n);
  for (int32_t pos = 0; pos < n; ++pos) {
    double wd = diag[y.perm[pos]];
    const Ilu0Part &b = y.before, &a = y.after;
    for (int64_t e = b.ptr[pos]; e < b.ptr[(size_t)pos + 1]; ++e) {
      const int32_t k = b.cpos[(size_t)e];
      const double mult = at(0, e) * dinv2[k];
      for (int64_t f = a.ptr[k]; f < a.ptr[(size_t)k + 1]; ++f) {
        const int32_t j = a.cpos[(size_t)f];
        const double prod = mult * at(1, f);
        if (j == pos) {
          wd = wd - prod;
          continue;
        }
        for (int h = 0; h < 2; ++h) { // the kernel's binary search, as a scan
          const Ilu0Part& p = *parts[h];
          for (int64_t g = p.ptr[pos]; g < p.ptr[(size_t)pos + 1]; ++g)
            if (p.cpos[(size_t)g] == j)
              at(h, g) = at(h, g) - prod;
        }
      }
    }
    d2[pos] = wd;
    dinv2[pos] = 1.0 / wd;
  }
  for (int32_t pos = 0; pos < n; ++pos) {
    CHECK(std::memcmp(&d[pos], &d2[pos], 8) == 0, "%s: pivot at %d", name, pos);
    for (int h = 0; h < 2; ++h)
      for (int64_t e = parts[h]->ptr[pos]; e < parts[h]->ptr[(size_t)pos + 1]; ++e) {
        int32_t col = -1;
        const double got = sliced_at(y, *sliced[h], pos, e - parts[h]->ptr[pos], &col);
        const double w = (h == 0 ? low : up)[pos][parts[h]->cpos[(size_t)e]];
        CHECK(std::memcmp(&got, &w, 8) == 0, "%s: factor entry at (%d, %d)", name,
              pos, (int)(e - parts[h]->ptr[pos]));
      }
  }
  bool changed = false;
  for (int32_t pos = 0; pos < n; ++pos)
    changed = changed || d[pos] != diag[y.perm[pos]];
  CHECK(changed == (y.num_colors > 1), "%s: pivots changed: %d", name, (int)changed);
}

} // namespace

int main()
{
  for (int32_t n : {5, 11}) {
    const Csr m = poisson(n);
    const std::string name = "poisson" + std::to_string(n);
    check(name.c_str(), m, false, 2);
    check((name + " lower").c_str(), lower_of(m), true, 2);
    check((name + " full, symmetric form").c_str(), m, true, 2);
  }
  check("banded257", banded(257), false);
  check("arrow130", arrow(130), false, 2);
  const Csr rag = ragged(1001, 7);
  check("ragged1001", rag, false);
  check("ragged1001 lower", lower_of(rag), true);

  std::vector<std::map<int32_t, double>> rows(70);
  for (int32_t i = 0; i < 70; ++i)
    rows[i][i] = 2.0 + i;
  check("diagonal70", from_map(70, rows), false, 1);
  check("diagonal70", from_map(70, rows), true, 1);
  rows.assign(1, {{0, 3.0}});
  check("n1", from_map(1, rows), false, 1);
  check("empty", Csr(), false, 0);

  // a column twice in a row is refused
  Csr dup;
  dup.rowptr = {0, 3, 5, 7};
  dup.colind = {0, 2, 2, 1, 0, 2, 0};
  dup.values.assign(7, 1.0);
  bool threw = false;
  try {
    ilu0_symbolic(dup.rowptr.data(), dup.colind.data(), 3, 3, false);
  } catch (const std::exception& e) {
    threw = std::strstr(e.what(), "duplicate") != nullptr;
  }
  CHECK(threw, "a duplicate column was accepted");

  if (failures) {
    std::printf("ilu0_build_check: %d FAILED\n", failures);
    return 1;
  }
  std::printf("ilu0_build_check: OK\n");
  return 0;
}
