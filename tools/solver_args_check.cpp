// Stand-alone check of the solvers' plain-C++ argument rules and sizes
// (spmv_amd/csrc/host/solver_args.{h,cpp}) on the CPU, meant to be built with
// the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ispmv_amd/csrc/host tools/solver_args_check.cpp
//       spmv_amd/csrc/host/solver_args.cpp -o solver_args_check
//       && ./solver_args_check
//
// Checked: every rule of gmres_check_rules raises its word and the accepted
// range raises nothing; the order of the rules (kmax, restart, preconditioner,
// Chebyshev, rows); gmres_basis_stride is even, >= N_padded and < N_padded + 2;
// gmres_basis_elems is stride * (restart + 1) and refuses a product that does
// not fit; chebyshev_coefficients fills exactly `degree` entries (the arrays
// here are exactly that long, so a write past them is the sanitizer's to find)
// with the recurrence of cg.h, and refuses its bad arguments;
// lobpcg_check_pencil accepts equal row counts and ghost lists and names
// "pencil" for every difference, reading exactly the announced lengths.
// Exit status 0 and "solver_args_check: OK" when everything holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "solver_args.h"

using namespace spmv;

namespace
{
int failures = 0;

void expect(bool ok, const char* what)
{
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++failures;
  }
}

// the word of the exception f raises, "" when it raises nothing
template <class F>
std::string raised(F&& f)
{
  try {
    f();
  } catch (const std::runtime_error& e) {
    return e.what();
  }
  return "";
}

bool has(const std::string& s, const char* word)
{
  return s.find(word) != std::string::npos;
}

void rules()
{
  auto r = [](int restart, int kmax, bool dinv, int deg, double lo, double hi,
              bool sgs, int64_t srows, int64_t rows) {
    return raised([&] {
      gmres_check_rules(restart, kmax, dinv, deg, lo, hi, sgs, srows, rows);
    });
  };
  for (int m : {1, 2, 30, 64})
    for (int kmax : {0, 1, 400})
      expect(r(m, kmax, false, 0, 0, 0, false, 0, 10).empty(), "accepted range");
  expect(r(5, 10, true, 0, 0, 0, false, 0, 10).empty(), "dinv alone");
  expect(r(5, 10, true, 4, 0.1, 3.0, false, 0, 10).empty(), "chebyshev + dinv");
  expect(r(5, 10, false, 16, 0.1, 3.0, false, 0, 10).empty(), "degree 16");
  expect(r(5, 10, false, 0, 0, 0, true, 10, 10).empty(), "sgs alone");
  expect(has(r(5, -1, false, 0, 0, 0, false, 0, 10), "kmax"), "kmax < 0");
  for (int m : {0, -1, 65, std::numeric_limits<int>::max(),
                std::numeric_limits<int>::min()})
    expect(has(r(m, 10, false, 0, 0, 0, false, 0, 10), "restart"), "restart");
  expect(has(r(5, 10, true, 0, 0, 0, true, 10, 10), "preconditioner"),
         "sgs + dinv");
  expect(has(r(5, 10, false, 4, 0.1, 3.0, true, 10, 10), "preconditioner"),
         "sgs + chebyshev");
  for (int deg : {17, -1, std::numeric_limits<int>::min()})
    expect(has(r(5, 10, false, deg, 0.1, 3.0, false, 0, 10), "degree"), "degree");
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double bad[][2] = {{0.0, 1.0}, {-1.0, 1.0}, {2.0, 1.0}, {1.0, 1.0},
                           {1.0, inf}, {nan, 1.0}, {1.0, nan}, {-inf, 1.0}};
  for (const auto& b : bad)
    expect(has(r(5, 10, false, 4, b[0], b[1], false, 0, 10), "bounds"), "bounds");
  expect(has(r(5, 10, false, 0, 0, 0, true, 9, 10), "rows"), "rows");
  // order: kmax before restart before preconditioner before Chebyshev before rows
  expect(has(r(0, -1, true, 17, 0, 0, true, 9, 10), "kmax"), "order 1");
  expect(has(r(0, 1, true, 17, 0, 0, true, 9, 10), "restart"), "order 2");
  expect(has(r(5, 1, true, 17, 0, 0, true, 9, 10), "one preconditioner"),
         "order 3");
  expect(has(r(5, 1, false, 17, 0, 0, false, 9, 10), "degree"), "order 4");
}

void sizes()
{
  const int64_t big = std::numeric_limits<int64_t>::max();
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)1331,
                    (int64_t)13824, ((int64_t)1 << 40) + 1, big - 1, big - 2}) {
    const int64_t s = gmres_basis_stride(n);
    expect(s % 2 == 0 && s >= n && s < n + 2, "stride");
  }
  expect(has(raised([&] { gmres_basis_stride(big); }), "overflows"), "stride max");
  expect(has(raised([&] { gmres_basis_stride(-1); }), "overflows"), "stride < 0");
  for (int m : {1, 5, 64})
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)4097, (int64_t)134217728})
      expect(gmres_basis_elems(n, m) == gmres_basis_stride(n) * (m + 1), "elems");
  // 2^60 doubles at 65 vectors: the byte count does not fit
  expect(has(raised([&] { gmres_basis_elems((int64_t)1 << 60, 64); }),
             "overflows"),
         "elems overflow");
  expect(has(raised([&] { gmres_basis_elems(big - 1, 1); }), "overflows"),
         "elems overflow at the top");
  expect(has(raised([&] { gmres_basis_elems(8, -1); }), "overflows"),
         "restart < 0");
  // the largest product that fits
  const int64_t most = big / (int64_t)sizeof(double) / 65;
  const int64_t n_ok = most - (most & 1);
  expect(gmres_basis_elems(n_ok, 64) == n_ok * 65, "largest basis");
}

void chebyshev()
{
  for (int degree = 1; degree <= kChebyshevMaxDegree; ++degree) {
    // exactly `degree` long, on the heap: an overrun is reported
    std::vector<double> a(degree, -7.0), b(degree, -7.0);
    chebyshev_coefficients(degree, 0.1, 3.3, a.data(), b.data());
    const double theta = 0.5 * (3.3 + 0.1), delta = 0.5 * (3.3 - 0.1);
    const double sigma = theta / delta;
    double rho = 1.0 / sigma;
    expect(a[0] == 0.0 && b[0] == 1.0 / theta, "step 0");
    for (int j = 1; j < degree; ++j) {
      const double rho_new = 1.0 / (2.0 * sigma - rho);
      expect(a[j] == rho_new * rho && b[j] == 2.0 * rho_new / delta, "step j");
      rho = rho_new;
    }
  }
  double a[1], b[1];
  expect(has(raised([&] { chebyshev_coefficients(0, 0.1, 1, a, b); }), "degree"),
         "degree 0");
  expect(has(raised([&] { chebyshev_coefficients(17, 0.1, 1, a, b); }), "degree"),
         "degree 17");
  expect(has(raised([&] { chebyshev_coefficients(1, 1, 0.5, a, b); }), "bounds"),
         "bounds");
  expect(has(raised([&] { chebyshev_coefficients(1, 0.1, 1, nullptr, b); }),
             "NULL"),
         "NULL a");
  expect(has(raised([&] { chebyshev_coefficients(1, 0.1, 1, a, nullptr); }),
             "NULL"),
         "NULL b");
}
// lobpcg_check_pencil: the ghost lists are exactly as long as announced, on the
// heap (reading past them is the sanitizer's to find); lists of length 0 are NULL
void pencil()
{
  auto r = [](int64_t ra, int64_t rb, const std::vector<int64_t>& a,
              const std::vector<int64_t>& b) {
    return raised([&] {
      lobpcg_check_pencil(ra, rb, a.empty() ? nullptr : a.data(),
                          (int64_t)a.size(), b.empty() ? nullptr : b.data(),
                          (int64_t)b.size());
    });
  };
  expect(r(5, 5, {}, {}).empty(), "pencil: no ghosts");
  expect(r(0, 0, {}, {}).empty(), "pencil: no rows");
  expect(r(5, 5, {7, 9, 12}, {7, 9, 12}).empty(), "pencil: the same ghosts");
  expect(has(r(5, 4, {}, {}), "pencil"), "pencil: rows");
  expect(has(r(5, 5, {7, 9, 12}, {7, 9}), "pencil"), "pencil: a missing ghost");
  expect(has(r(5, 5, {7, 9}, {7, 9, 12}), "pencil"), "pencil: one too many");
  expect(has(r(5, 5, {}, {3}), "pencil"), "pencil: ghosts against none");
  expect(has(r(5, 5, {7, 9, 12}, {7, 12, 9}), "pencil"), "pencil: permuted");
  expect(has(r(5, 5, {7, 9, 12}, {7, 9, 13}), "pencil"), "pencil: another ghost");
  // the rows come first
  expect(has(r(5, 4, {7}, {8, 9}), "local rows"), "pencil: order");
}
} // namespace

int main()
{
  rules();
  sizes();
  chebyshev();
  pencil();
  if (failures) {
    std::printf("solver_args_check: %d FAILED\n", failures);
    return 1;
  }
  std::printf("solver_args_check: OK\n");
  return 0;
}
