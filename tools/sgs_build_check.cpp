// Stand-alone check of the host half of the multicolour symmetric Gauss-Seidel
// preconditioner (spmv_amd/csrc/host/sgs_build.{h,cpp}): the colouring, the
// colour-major copy and the sliced layout, on the CPU, meant to be built with
// the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ispmv_amd/csrc/host tools/sgs_build_check.cpp
//       spmv_amd/csrc/host/sgs_build.cpp -o sgs_build_check && ./sgs_build_check
//
// Matrices: the shapes of tests/test_gpu_pcg.py (7-point Poisson on 11^3 and
// 24^3, the band of 4 097 rows with offsets 1, 37, 600), a ragged matrix of
// 3 001 rows with two rows of about 500 entries, a diagonal matrix, n = 1, a
// one-way pattern, n = 0; each in the general and the symmetric input form.
// Checked: the colouring is proper over B + B^T and wears every colour; Poisson
// gets the parity of x + y + z; perm is a colour-major permutation, ascending
// within a colour; the two parts hold every off-diagonal entry once, ascending
// by column; and the sweeps read from the SLICED layout with the kernel's
// indexing (spmv_mcgs.hip) give the bits of the sweeps over the CSR parts.
// Exit status 0 and "sgs_build_check: OK" when everything holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "sgs_build.h"

using namespace spmv;

namespace
{

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
  for (int32_t z = 0; z < n; ++z)
    for (int32_t y = 0; y < n; ++y)
      for (int32_t x = 0; x < n; ++x) {
        const int32_t i = x + n * (y + n * z);
        rows[i][i] = 6.0;
        if (x > 0) rows[i][i - 1] = -1.0;
        if (x < n - 1) rows[i][i + 1] = -1.0;
        if (y > 0) rows[i][i - n] = -1.0;
        if (y < n - 1) rows[i][i + n] = -1.0;
        if (z > 0) rows[i][i - n * n] = -1.0;
        if (z < n - 1) rows[i][i + n * n] = -1.0;
      }
  return from_map(N, rows);
}

Csr banded(int32_t n)
{
  std::vector<std::map<int32_t, double>> rows(n);
  for (int32_t i = 0; i < n; ++i)
    rows[i][i] = 6.0 + 0.3 * std::sin((double)i);
  for (int32_t d : {1, 37, 600})
    for (int32_t i = 0; i + d < n; ++i) {
      const double v = -(0.5 + 0.4 * std::cos((double)(2 * i + d)));
      rows[i][i + d] = v;
      rows[i + d][i] = v;
    }
  return from_map(n, rows);
}

Csr ragged(int32_t n, unsigned seed)
{
  std::mt19937_64 rng(seed);
  std::vector<std::map<int32_t, double>> rows(n);
  auto couple = [&](int32_t i, int32_t j) {
    if (i == j || i == 7 || j == 7)
      return;
    const double v = -0.1 - 0.9 * (double)(rng() % 1000) / 1000.0;
    rows[i][j] = v;
    rows[j][i] = v;
  };
  for (int32_t i = 0; i < n; ++i)
    for (int k = (int)(rng() % 21); k > 0; --k)
      couple(i, (int32_t)(rng() % n));
  for (int32_t hub : {100, n - 501})
    for (int k = 0; k < 500; ++k)
      couple(hub, (int32_t)(rng() % n));
  for (int32_t i = n - 24; i < n; ++i)
    for (int32_t j = i + 1; j < n; ++j)
      couple(i, j);
  for (int32_t i = 0; i < n; ++i) {
    double off = 0;
    for (const auto& cv : rows[i])
      off += std::fabs(cv.second);
    rows[i][i] = off + 1.5;
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

int failures = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    if (!(cond)) {                                                             \
      ++failures;                                                              \
      std::printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond);           \
      std::printf(__VA_ARGS__);                                                \
      std::printf("\n");                                                       \
    }                                                                          \
  } while (0)

// the sweeps over the CSR parts: cg.h as written
std::vector<double> apply_csr(const SgsHostPlan& p, const std::vector<double>& r)
{
  std::vector<double> z((size_t)p.n, std::nan(""));
  for (int c = 0; c < p.num_colors; ++c)
    for (int32_t pos = p.color_start[c]; pos < p.color_start[c + 1]; ++pos) {
      const int32_t i = p.perm[pos];
      double s = 0.0;
      for (int64_t e = p.before.ptr[pos]; e < p.before.ptr[pos + 1]; ++e)
        s = s + p.before.val[e] * z[p.before.col[e]];
      z[i] = (r[i] - s) * (1.0 / p.d[i]);
    }
  for (int c = p.num_colors - 2; c >= 0; --c)
    for (int32_t pos = p.color_start[c]; pos < p.color_start[c + 1]; ++pos) {
      const int32_t i = p.perm[pos];
      double t = 0.0;
      for (int64_t e = p.after.ptr[pos]; e < p.after.ptr[pos + 1]; ++e)
        t = t + p.after.val[e] * z[p.after.col[e]];
      z[i] = z[i] - (1.0 / p.d[i]) * t;
    }
  return z;
}

// one colour from the sliced layout, indexed as mcgs_sweep_kernel does
void sweep_sliced(const SgsHostPlan& p, const SgsSlicedPart& s, int c,
                  bool forward, const std::vector<double>& r,
                  std::vector<double>& z, const char* name)
{
  const int32_t pos_end = p.color_start[c + 1];
  std::vector<std::pair<int32_t, double>> out; // rows of a colour are independent
  for (int32_t sl = s.color_slice[c]; sl < s.color_slice[c + 1]; ++sl)
    for (int lane = 0; lane < 64; ++lane) {
      const int32_t pos = s.slice_pos0[sl] + lane;
      if (pos >= pos_end)
        continue;
      const int32_t m = s.len[pos];
      if (m < 0)
        continue;
      const int64_t base = s.slice_ptr[sl] + lane;
      double acc = 0.0;
      for (int32_t k = 0; k < m; ++k) {
        const int64_t e = base + (int64_t)k * 64;
        CHECK(e < s.slice_ptr[sl + 1], "%s: entry past its slice", name);
        acc = acc + s.val[e] * z[s.col[e]];
      }
      out.emplace_back(p.perm[pos], acc);
    }
  for (int32_t l = s.color_long[c]; l < s.color_long[c + 1]; ++l) {
    const int32_t pos = s.long_pos[l];
    CHECK(s.len[pos] == -1, "%s: long row not marked", name);
    double acc = 0.0;
    for (int64_t e = s.long_ptr[l]; e < s.long_ptr[l + 1]; ++e)
      acc = acc + s.long_val[e] * z[s.long_col[e]];
    out.emplace_back(p.perm[pos], acc);
  }
  CHECK((int32_t)out.size() == pos_end - p.color_start[c],
        "%s: colour %d: %zu rows served", name, c, out.size());
  for (const auto& ia : out) {
    const int32_t i = ia.first;
    const double dinv = 1.0 / p.d[i];
    z[i] = forward ? (r[i] - ia.second) * dinv : z[i] - dinv * ia.second;
  }
}

void check(const char* name, const Csr& m, bool symmetric, int want_colors = -1)
{
  const int32_t n = m.n();
  int nc = 0;
  const std::vector<int32_t> colour = sgs_color(
      m.rowptr.data(), m.colind.data(), n, n, symmetric, &nc);
  // the entries of B, and B + B^T
  std::vector<std::set<int32_t>> nb(n);
  int64_t off = 0;
  for (int32_t i = 0; i < n; ++i)
    for (int32_t e = m.rowptr[i]; e < m.rowptr[i + 1]; ++e) {
      const int32_t c = m.colind[e];
      if (c < n && c != i && (!symmetric || c < i)) {
        nb[i].insert(c);
        nb[c].insert(i);
        ++off;
      }
    }
  std::vector<int> worn(nc, 0);
  for (int32_t i = 0; i < n; ++i) {
    CHECK(colour[i] >= 0 && colour[i] < nc, "%s: colour of %d", name, i);
    ++worn[colour[i]];
    std::set<int32_t> before;
    for (int32_t j : nb[i]) {
      CHECK(colour[j] != colour[i], "%s: %d and %d share a colour", name, i, j);
      if (j < i)
        before.insert(colour[j]);
    }
    int32_t c = 0;
    while (before.count(c))
      ++c;
    CHECK(colour[i] == c, "%s: row %d is not greedy", name, i);
  }
  for (int c = 0; c < nc; ++c)
    CHECK(worn[c] > 0, "%s: colour %d is not worn", name, c);
  if (want_colors >= 0)
    CHECK(nc == want_colors, "%s: %d colours", name, nc);

  const SgsHostPlan p = sgs_build(m.rowptr.data(), m.colind.data(),
                                  m.values.data(), nullptr, n, n, symmetric);
  CHECK(p.colors == colour && p.num_colors == nc, "%s: build's colours", name);
  std::vector<int> seen(n, 0);
  for (int32_t pos = 0; pos < n; ++pos) {
    ++seen[p.perm[pos]];
    if (pos > 0)
      CHECK(colour[p.perm[pos - 1]] < colour[p.perm[pos]]
                || (colour[p.perm[pos - 1]] == colour[p.perm[pos]]
                    && p.perm[pos - 1] < p.perm[pos]),
            "%s: perm at %d", name, pos);
  }
  for (int32_t i = 0; i < n; ++i)
    CHECK(seen[i] == 1, "%s: row %d in perm %d times", name, i, seen[i]);
  const int64_t both = (int64_t)p.before.col.size() + (int64_t)p.after.col.size();
  CHECK(both == (symmetric ? 2 * off : off), "%s: %lld entries in the parts", name,
        (long long)both);
  for (const SgsCsrPart* part : {&p.before, &p.after})
    for (int32_t pos = 0; pos < n; ++pos)
      for (int64_t e = part->ptr[pos]; e < part->ptr[pos + 1]; ++e) {
        const int32_t i = p.perm[pos], c = part->col[e];
        CHECK(nb[i].count(c) == 1, "%s: (%d, %d) is no entry", name, i, c);
        CHECK((part == &p.before) == (colour[c] < colour[i]), "%s: part of (%d, %d)",
              name, i, c);
        if (e > part->ptr[pos])
          CHECK(part->col[e - 1] <= c, "%s: row %d not sorted", name, i);
      }

  // the sliced layout gives the bits of the CSR parts
  const SgsSlicedPart sb = sgs_slice(p, p.before), sa = sgs_slice(p, p.after);
  std::vector<double> r(n);
  std::mt19937_64 rng(n + 1);
  for (double& v : r)
    v = (double)(rng() % 2000001) / 1000000.0 - 1.0;
  const std::vector<double> want = apply_csr(p, r);
  std::vector<double> z((size_t)n, std::nan(""));
  for (int c = 0; c < nc; ++c)
    sweep_sliced(p, sb, c, true, r, z, name);
  for (int c = nc - 2; c >= 0; --c)
    sweep_sliced(p, sa, c, false, r, z, name);
  CHECK(n == 0 || std::memcmp(z.data(), want.data(), (size_t)n * 8) == 0,
        "%s: the sliced sweeps differ", name);
  for (int32_t i = 0; i < n; ++i)
    CHECK(std::isfinite(z[i]), "%s: z[%d]", name, i);
  std::printf("%-28s %s  rows %6d  colours %3d  long rows %zu + %zu  padding %.2f\n",
              name, symmetric ? "symmetric" : "general  ", n, nc,
              sb.long_pos.size(), sa.long_pos.size(),
              both ? (double)(sb.col.size() + sa.col.size() + sb.long_col.size()
                              + sa.long_col.size())
                         / (double)both
                   : 1.0);
}

} // namespace

int main()
{
  for (int32_t n : {11, 24}) {
    const Csr m = poisson(n);
    const std::string name = "poisson" + std::to_string(n);
    check(name.c_str(), m, false, 2);
    check((name + " lower").c_str(), lower_of(m), true, 2);
    check((name + " full, symmetric form").c_str(), m, true, 2);
    int nc = 0;
    const std::vector<int32_t> c = sgs_color(m.rowptr.data(), m.colind.data(),
                                             m.n(), m.n(), false, &nc);
    for (int32_t i = 0; i < m.n(); ++i)
      CHECK(c[i] == (i % n + (i / n) % n + i / (n * n)) % 2, "parity at %d", i);
  }
  const Csr band = banded(4097);
  check("banded4097", band, false);
  check("banded4097 lower", lower_of(band), true);
  const Csr rag = ragged(3001, 7);
  check("ragged3001", rag, false);
  check("ragged3001 lower", lower_of(rag), true);

  std::vector<std::map<int32_t, double>> rows(70);
  for (int32_t i = 0; i < 70; ++i)
    rows[i][i] = 2.0 + i;
  check("diagonal70", from_map(70, rows), false, 1);
  check("diagonal70", from_map(70, rows), true, 1);
  rows.assign(1, {{0, 3.0}});
  check("n1", from_map(1, rows), false, 1);
  check("n1", from_map(1, rows), true, 1);
  // (0, 2), (1, 3) and (4, 0) are present, their mirror images are not
  rows.assign(5, {});
  for (int32_t i = 0; i < 5; ++i)
    rows[i][i] = 4.0;
  rows[0][2] = -1.0;
  rows[1][3] = -0.5;
  rows[4][0] = -1.0;
  check("one-way pattern", from_map(5, rows), false, 2);
  check("empty", Csr(), false, 0);

  // sizes that do not match are refused
  bool threw = false;
  try {
    sgs_color(band.rowptr.data(), band.colind.data(), band.n(), band.n() - 1,
              false);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "nrows != ncols_local was accepted");

  if (failures) {
    std::printf("sgs_build_check: %d FAILED\n", failures);
    return 1;
  }
  std::printf("sgs_build_check: OK\n");
  return 0;
}
