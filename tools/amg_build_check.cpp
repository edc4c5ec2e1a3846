// Stand-alone check of the host half of the aggregation multigrid
// preconditioner (spmv_amd/csrc/host/amg_build.{h,cpp}): expanded rows,
// aggregates, coarse pattern and source lists on the CPU, meant to be built with
// the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ispmv_amd/csrc/host tools/amg_build_check.cpp
//       spmv_amd/csrc/host/amg_build.cpp -o amg_build_check && ./amg_build_check
//
// Matrices: 7-point Poisson on 5^3 and 11^3, a nonsymmetric band of 257 rows
// (offsets 1, 37), the arrow matrix of 130 rows (one aggregate of 130 members),
// a ragged symmetric matrix of 1 001 rows with a hub row of about 300 entries, a
// matrix with ghost columns, with an explicit zero and with a duplicate column,
// a diagonal matrix (nothing merges), n = 1, n = 0; theta 0, 0.25 and 1; the
// symmetric ones also in the symmetric input form, which must give the same
// aggregates and the same coarse pattern.  Checked: every row wears one
// aggregate, numbered in order of creation; the member lists are the rows of
// their aggregate, ascending; the coarse rows ascend by column without
// duplicates; the source lists partition the expanded entries, each entry under
// the pair of aggregates of its row and column, ordered by row and then by the
// expanded row's order; P^T A P summed through the lists equals the dense triple
// product to 8 ulps of the contributions' absolute sum.
// Exit status 0 and "amg_build_check: OK" when everything holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include "amg_build.h"

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

Csr from_rows(const std::vector<std::vector<std::pair<int32_t, double>>>& rows)
{
  Csr m;
  for (const auto& row : rows) {
    for (const auto& cv : row) {
      m.colind.push_back(cv.first);
      m.values.push_back(cv.second);
    }
    m.rowptr.push_back((int32_t)m.colind.size());
  }
  return m;
}

Csr from_map(int32_t n, const std::vector<std::map<int32_t, double>>& rows)
{
  std::vector<std::vector<std::pair<int32_t, double>>> r((size_t)n);
  for (int32_t i = 0; i < n; ++i)
    r[(size_t)i].assign(rows[(size_t)i].begin(), rows[(size_t)i].end());
  return from_rows(r);
}

Csr poisson(int32_t n)
{
  const int32_t N = n * n * n;
  std::vector<std::map<int32_t, double>> rows((size_t)N);
  for (int32_t i = 0; i < N; ++i) {
    const int32_t c[3] = {i % n, (i / n) % n, i / (n * n)};
    rows[(size_t)i][i] = 6.0;
    int32_t stride = 1;
    for (int d = 0; d < 3; ++d, stride *= n) {
      if (c[d] > 0)
        rows[(size_t)i][i - stride] = -1.0;
      if (c[d] < n - 1)
        rows[(size_t)i][i + stride] = -1.0;
    }
  }
  return from_map(N, rows);
}

Csr banded(int32_t n)
{
  std::vector<std::map<int32_t, double>> rows((size_t)n);
  for (int32_t i = 0; i < n; ++i) {
    rows[(size_t)i][i] = 6.0 + 0.3 * std::sin((double)i);
    for (int32_t d : {1, 37}) {
      if (i + d < n)
        rows[(size_t)i][i + d] = -(0.3 + 0.25 * std::sin((double)(3 * i + 2 * d)));
      if (i - d >= 0)
        rows[(size_t)i][i - d] = -(0.5 + 0.4 * std::cos((double)(2 * i - d)));
    }
  }
  return from_map(n, rows);
}

Csr arrow(int32_t n)
{
  std::vector<std::map<int32_t, double>> rows((size_t)n);
  for (int32_t i = 0; i < n; ++i) {
    rows[(size_t)i][i] = i == n - 1 ? 2.0 * n : 4.0;
    if (i < n - 1) {
      rows[(size_t)i][n - 1] = -1.0;
      rows[(size_t)n - 1][i] = -1.0;
    }
  }
  return from_map(n, rows);
}

Csr ragged(int32_t n, unsigned seed)
{
  std::mt19937 rng(seed);
  std::vector<std::map<int32_t, double>> rows((size_t)n);
  auto couple = [&](int32_t a, int32_t b) {
    if (a == b || a == 7 || b == 7)
      return;
    const double v = -(0.1 + (double)(rng() % 900) / 1000.0);
    rows[(size_t)a][b] = v;
    rows[(size_t)b][a] = v;
  };
  for (int32_t i = 0; i < n; ++i)
    for (unsigned k = rng() % 12; k > 0; --k)
      couple(i, (int32_t)(rng() % (unsigned)n));
  for (int k = 0; k < 300; ++k)
    couple(100, (int32_t)(rng() % (unsigned)n));
  for (int32_t i = 0; i < n; ++i) {
    double off = 0;
    for (const auto& cv : rows[(size_t)i])
      off += std::fabs(cv.second);
    rows[(size_t)i][i] = off + 1.0;
  }
  return from_map(n, rows);
}

Csr diagonal_matrix(int32_t n)
{
  std::vector<std::map<int32_t, double>> rows((size_t)n);
  for (int32_t i = 0; i < n; ++i)
    rows[(size_t)i][i] = 2.0 + (double)(i % 3);
  return from_map(n, rows);
}

// the symmetric input form: strictly lower block and the diagonal array
void lower_of(const Csr& a, Csr* low, std::vector<double>* diag)
{
  const int32_t n = a.n();
  diag->assign((size_t)n, 0.0);
  *low = Csr();
  for (int32_t i = 0; i < n; ++i) {
    for (int32_t e = a.rowptr[(size_t)i]; e < a.rowptr[(size_t)i + 1]; ++e) {
      const int32_t c = a.colind[(size_t)e];
      if (c < i) {
        low->colind.push_back(c);
        low->values.push_back(a.values[(size_t)e]);
      } else if (c == i) {
        (*diag)[(size_t)i] += a.values[(size_t)e];
      }
    }
    low->rowptr.push_back((int32_t)low->colind.size());
  }
}

double value_of(int32_t q, const Csr& a, const std::vector<double>& diag)
{
  return q >= 0 ? a.values[(size_t)q] : diag[(size_t)~q];
}

// everything the header promises about one step; returns it
AmgStep check_step(const char* what, const Csr& a, int32_t n, bool symmetric,
                   const std::vector<double>& diag, double theta)
{
  const AmgExpanded x
      = amg_expand(a.rowptr.data(), a.colind.data(), n, n, symmetric);
  CHECK(x.n == n && (int32_t)x.ptr.size() == n + 1, "%s: expanded size", what);
  // expanded rows: every kept stored entry once as itself; symmetric: once
  // more mirrored, behind the diagonal, ascending by row
  for (int32_t i = 0; i < n; ++i) {
    bool diag_seen = false;
    int32_t last_mirror = -1;
    for (int64_t e = x.ptr[(size_t)i]; e < x.ptr[(size_t)i + 1]; ++e) {
      const int32_t c = x.col[(size_t)e], q = x.src[(size_t)e];
      CHECK(c >= 0 && c < n, "%s: column", what);
      if (!symmetric) {
        CHECK(q >= a.rowptr[(size_t)i] && q < a.rowptr[(size_t)i + 1]
                  && a.colind[(size_t)q] == c,
              "%s: source of row %d", what, i);
        CHECK(e == x.ptr[(size_t)i] || q > x.src[(size_t)e - 1],
              "%s: storage order", what);
      } else if (q < 0) {
        CHECK(~q == i && c == i && !diag_seen, "%s: diagonal", what);
        diag_seen = true;
      } else if (!diag_seen) {
        CHECK(c < i && a.colind[(size_t)q] == c, "%s: lower entry", what);
      } else {
        CHECK(c > i && a.colind[(size_t)q] == i && c >= last_mirror
                  && q >= a.rowptr[(size_t)c] && q < a.rowptr[(size_t)c + 1],
              "%s: mirror image", what);
        last_mirror = c;
      }
    }
    CHECK(!symmetric || diag_seen, "%s: row %d has no diagonal", what, i);
  }
  AmgStep s = amg_coarsen(x, a.values.data(), diag.data(), theta);
  CHECK(s.n == n && (int32_t)s.agg.size() == n, "%s: agg size", what);
  // numbered in order of creation is not order of row, but every number occurs
  std::vector<int32_t> count((size_t)s.n_agg, 0);
  for (int32_t i = 0; i < n; ++i) {
    CHECK(s.agg[(size_t)i] >= 0 && s.agg[(size_t)i] < s.n_agg, "%s: agg range",
          what);
    if (s.agg[(size_t)i] >= 0 && s.agg[(size_t)i] < s.n_agg)
      ++count[(size_t)s.agg[(size_t)i]];
  }
  CHECK((int32_t)s.member_ptr.size() == s.n_agg + 1 && s.member_ptr[0] == 0,
        "%s: member_ptr", what);
  for (int32_t I = 0; I < s.n_agg; ++I) {
    const int32_t m0 = s.member_ptr[(size_t)I], m1 = s.member_ptr[(size_t)I + 1];
    CHECK(m1 - m0 == count[(size_t)I] && m1 > m0, "%s: members of %d", what, I);
    for (int32_t m = m0; m < m1; ++m) {
      CHECK(s.agg[(size_t)s.member[(size_t)m]] == I, "%s: member", what);
      CHECK(m == m0 || s.member[(size_t)m] > s.member[(size_t)m - 1],
            "%s: members ascending", what);
    }
  }
  // pattern and lists against a map built the slow way
  std::map<std::pair<int32_t, int32_t>, std::vector<int32_t>> want;
  for (int32_t i = 0; i < n; ++i)
    for (int64_t e = x.ptr[(size_t)i]; e < x.ptr[(size_t)i + 1]; ++e)
      want[{s.agg[(size_t)i], s.agg[(size_t)x.col[(size_t)e]]}].push_back(
          x.src[(size_t)e]);
  CHECK(want.size() == s.colind.size()
            && s.src_ptr.size() == s.colind.size() + 1
            && s.src.size() == x.src.size(),
        "%s: coarse sizes", what);
  size_t E = 0;
  for (const auto& kv : want) {
    if (E >= s.colind.size())
      break;
    const int32_t I = kv.first.first, J = kv.first.second;
    CHECK(s.rowptr[(size_t)I] <= (int32_t)E && (int32_t)E < s.rowptr[(size_t)I + 1]
              && s.colind[E] == J,
          "%s: coarse entry %zu", what, E);
    const int64_t e0 = s.src_ptr[E], e1 = s.src_ptr[E + 1];
    CHECK(e1 - e0 == (int64_t)kv.second.size(), "%s: list length", what);
    if (e1 - e0 == (int64_t)kv.second.size())
      for (int64_t e = e0; e < e1; ++e)
        CHECK(s.src[(size_t)e] == kv.second[(size_t)(e - e0)], "%s: list order",
              what);
    ++E;
  }
  // the triple product through the lists against the dense one
  if (n <= 400 && s.n_agg > 0) {
    std::vector<double> dense((size_t)s.n_agg * s.n_agg, 0.0),
        scale((size_t)s.n_agg * s.n_agg, 0.0);
    for (int32_t i = 0; i < n; ++i)
      for (int64_t e = x.ptr[(size_t)i]; e < x.ptr[(size_t)i + 1]; ++e) {
        const size_t at = (size_t)s.agg[(size_t)i] * s.n_agg
                          + s.agg[(size_t)x.col[(size_t)e]];
        const double v = value_of(x.src[(size_t)e], a, diag);
        dense[at] += v;
        scale[at] += std::fabs(v);
      }
    for (int32_t I = 0; I < s.n_agg; ++I)
      for (int32_t k = s.rowptr[(size_t)I]; k < s.rowptr[(size_t)I + 1]; ++k) {
        double acc = value_of(s.src[(size_t)s.src_ptr[(size_t)k]], a, diag);
        for (int64_t e = s.src_ptr[(size_t)k] + 1; e < s.src_ptr[(size_t)k + 1]; ++e)
          acc = acc + value_of(s.src[(size_t)e], a, diag);
        const size_t at = (size_t)I * s.n_agg + s.colind[(size_t)k];
        CHECK(std::fabs(acc - dense[at]) <= 8 * 0x1p-53 * scale[at],
              "%s: P^T A P at (%d, %d)", what, I, s.colind[(size_t)k]);
      }
  }
  return s;
}

void check_matrix(const char* what, const Csr& a, bool also_symmetric)
{
  const int32_t n = a.n();
  const std::vector<double> none;
  for (double theta : {0.0, 0.25, 1.0}) {
    const AmgStep g = check_step(what, a, n, false, none, theta);
    if (!also_symmetric)
      continue;
    Csr low;
    std::vector<double> diag;
    lower_of(a, &low, &diag);
    const AmgStep s = check_step(what, low, n, true, diag, theta);
    CHECK(s.n_agg == g.n_agg && s.agg == g.agg && s.member == g.member
              && s.rowptr == g.rowptr && s.colind == g.colind
              && s.src_ptr == g.src_ptr,
          "%s: the two storages differ (theta %g)", what, theta);
  }
}

} // namespace

int main()
{
  check_matrix("poisson5", poisson(5), true);
  check_matrix("poisson11", poisson(11), true);
  check_matrix("banded257", banded(257), false);
  check_matrix("arrow130", arrow(130), true);
  check_matrix("ragged1001", ragged(1001, 7), true);
  check_matrix("diag40", diagonal_matrix(40), true);
  check_matrix("diag1", diagonal_matrix(1), true);
  {
    const std::vector<double> none;
    const Csr p5 = poisson(5);
    const AmgStep s = check_step("poisson5", p5, p5.n(), false, none, 0.25);
    CHECK(s.n_agg < p5.n() && s.n_agg > 0, "poisson5 does not coarsen");
    const Csr d = diagonal_matrix(40);
    CHECK(check_step("diag40", d, 40, false, none, 0.25).n_agg == 40,
          "a diagonal matrix merges rows");
    const Csr ar = arrow(130);
    CHECK(check_step("arrow130", ar, 130, false, none, 0.25).n_agg == 1,
          "the arrow matrix is one aggregate");
    // n = 0
    const int32_t zero = 0;
    const AmgExpanded x0 = amg_expand(&zero, nullptr, 0, 0, false);
    const AmgStep s0 = amg_coarsen(x0, nullptr, nullptr, 0.25);
    CHECK(s0.n_agg == 0 && s0.colind.empty(), "n = 0");
    // ghost columns are dropped: the first 40 rows of poisson 4^3
    const Csr p4 = poisson(4);
    Csr head;
    head.rowptr.assign(p4.rowptr.begin(), p4.rowptr.begin() + 41);
    head.colind.assign(p4.colind.begin(), p4.colind.begin() + head.rowptr[40]);
    head.values.assign(p4.values.begin(), p4.values.begin() + head.rowptr[40]);
    check_step("ghosts", head, 40, false, none, 0.25);
    // an explicit zero is no strong neighbour but stays in the pattern; a
    // duplicate column is summed into one coarse entry and kept once as a
    // neighbour
    const Csr odd = from_rows({{{0, 4.0}, {1, 0.0}, {2, -1.0}, {2, -0.5}},
                               {{0, 0.0}, {1, 4.0}},
                               {{0, -1.0}, {2, 4.0}, {0, -0.5}}});
    const AmgStep so = check_step("odd", odd, 3, false, none, 0.0);
    CHECK(so.n_agg == 2 && so.agg[0] == so.agg[2] && so.agg[1] != so.agg[0],
          "explicit zero / duplicate column");
    CHECK(so.colind.size() == 4, "a zero entry left the pattern");
    // rows and owned columns must be the same range
    bool thrown = false;
    try {
      (void)amg_expand(p4.rowptr.data(), p4.colind.data(), 64, 63, false);
    } catch (const std::runtime_error&) {
      thrown = true;
    }
    CHECK(thrown, "ncols_local != nrows accepted");
  }
  if (failures) {
    std::printf("amg_build_check: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("amg_build_check: OK\n");
  return 0;
}
