// see solver_args.h
#include "solver_args.h"

#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>

namespace spmv
{

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

void gmres_check_rules(int restart, int kmax, bool has_dinv, int cheb_degree,
                       double lmin, double lmax, bool has_sgs, int64_t sgs_rows,
                       int64_t rows)
{
  if (kmax < 0)
    throw std::runtime_error("spmv::gmres - Error: kmax < 0");
  if (restart < 1 || restart > kGmresMaxRestart)
    throw std::runtime_error("spmv::gmres - Error: restart must be 1.."
                             + std::to_string(kGmresMaxRestart));
  if (has_sgs && (has_dinv || cheb_degree != 0))
    throw std::runtime_error(
        "spmv::gmres - Error: one preconditioner at a time (sgs excludes dinv "
        "and the Chebyshev degree)");
  if (cheb_degree != 0) {
    double ca[kChebyshevMaxDegree], cb[kChebyshevMaxDegree];
    chebyshev_coefficients(cheb_degree, lmin, lmax, ca, cb);
  }
  if (has_sgs && sgs_rows != rows)
    throw std::runtime_error("spmv::gmres - Error: the preconditioner has "
                             + std::to_string(sgs_rows) + " rows, A has "
                             + std::to_string(rows));
}

namespace
{
// u[0:n) and v[0:m) doubles share a byte
bool doubles_overlap(const double* u, int64_t n, const double* v, int64_t m)
{
  const std::uintptr_t ub = reinterpret_cast<std::uintptr_t>(u);
  const std::uintptr_t vb = reinterpret_cast<std::uintptr_t>(v);
  return n > 0 && m > 0 && ub < vb + (std::uintptr_t)m * sizeof(double)
         && vb < ub + (std::uintptr_t)n * sizeof(double);
}
} // namespace

void pcg_block_check_rules(int nrhs, int kmax, bool has_dinv, bool has_sgs,
                           int64_t sgs_rows, int64_t sgs_negative_pivots,
                           int64_t rows, const double* B, const double* X,
                           const double* dinv)
{
  pcg_block_check_rules(nrhs, kmax, has_dinv, has_sgs, false, sgs_rows,
                        sgs_negative_pivots, 0, rows, B, X, dinv);
}

void amg_apply_block_check_rules(int nrhs, int64_t rows, const double* R,
                                 const double* Z)
{
  if (nrhs < 1 || nrhs > 8)
    throw std::runtime_error(
        "spmv::amg_apply_block - Error: nrhs must be in 1..8");
  if (doubles_overlap(Z, rows * nrhs, R, rows * nrhs))
    throw std::runtime_error("amg_apply_block: Z overlaps R");
}

void pcg_block_check_rules(int nrhs, int kmax, bool has_dinv, bool has_sgs,
                           bool has_amg, int64_t sgs_rows,
                           int64_t sgs_negative_pivots, int64_t amg_rows,
                           int64_t rows, const double* B, const double* X,
                           const double* dinv)
{
  if (nrhs < 1 || nrhs > 8)
    throw std::runtime_error("spmv::pcg_block - Error: nrhs must be in 1..8");
  if (kmax < 0)
    throw std::runtime_error("spmv::pcg_block - Error: kmax < 0");
  if ((int)has_dinv + (int)has_sgs + (int)has_amg != 1)
    throw std::runtime_error(
        has_amg ? "spmv::pcg_block - Error: exactly one preconditioner (dinv, "
                  "sgs or amg)"
                : "spmv::pcg_block - Error: exactly one preconditioner (dinv or "
                  "sgs)");
  if ((has_sgs && sgs_rows != rows) || (has_amg && amg_rows != rows))
    throw std::runtime_error(
        "spmv::pcg_block - Error: the preconditioner was built for "
        + std::to_string(has_sgs ? sgs_rows : amg_rows)
        + " rows, the matrix has " + std::to_string(rows));
  if (has_sgs && sgs_negative_pivots > 0)
    throw std::runtime_error(
        "spmv::pcg_block - Error: the preconditioner has "
        + std::to_string(sgs_negative_pivots)
        + " negative pivot(s): it is not positive definite");
  const int64_t elems = rows * nrhs;
  if (doubles_overlap(X, elems, B, elems))
    throw std::runtime_error(
        "pcg_block: X overlaps B (X is updated in place)");
  if (has_dinv && doubles_overlap(X, elems, dinv, rows))
    throw std::runtime_error(
        "pcg_block: X overlaps dinv (X is updated in place)");
}

void minres_check_rules(int kmax, bool has_dinv, bool has_sgs, bool has_amg,
                        int64_t sgs_rows, int64_t sgs_negative_pivots,
                        int64_t amg_rows, int64_t rows, const double* b,
                        const double* x, const double* dinv)
{
  if (kmax < 0)
    throw std::runtime_error("spmv::minres - Error: kmax < 0");
  if ((int)has_dinv + (int)has_sgs + (int)has_amg > 1)
    throw std::runtime_error(
        "spmv::minres - Error: one preconditioner at a time (dinv, sgs or amg)");
  if ((has_sgs && sgs_rows != rows) || (has_amg && amg_rows != rows))
    throw std::runtime_error(
        "spmv::minres - Error: the preconditioner was built for "
        + std::to_string(has_sgs ? sgs_rows : amg_rows)
        + " rows, the matrix has " + std::to_string(rows));
  if (has_sgs && sgs_negative_pivots > 0)
    throw std::runtime_error(
        "spmv::minres - Error: the preconditioner has "
        + std::to_string(sgs_negative_pivots)
        + " negative pivot(s): it is not positive definite");
  if (doubles_overlap(x, rows, b, rows))
    throw std::runtime_error("minres: x overlaps b (x is updated in place)");
  if (has_dinv && doubles_overlap(x, rows, dinv, rows))
    throw std::runtime_error("minres: x overlaps dinv (x is updated in place)");
}

void lsqr_check_rules(int kmax, double ltol, double damp, int64_t rows,
                      int64_t cols, const double* b, const double* x)
{
  if (kmax < 0)
    throw std::runtime_error("spmv::lsqr - Error: kmax < 0");
  if (!(ltol >= 0.0) || !std::isfinite(ltol))
    throw std::runtime_error(
        "spmv::lsqr - Error: ltol must be finite and not negative");
  if (!(damp >= 0.0) || !std::isfinite(damp))
    throw std::runtime_error(
        "spmv::lsqr - Error: damp must be finite and not negative");
  if (doubles_overlap(x, cols, b, rows))
    throw std::runtime_error("lsqr: x overlaps b (x is updated in place)");
}

void lobpcg_check_rules(int nev, int kmax, double rtol, double atol,
                        bool has_dinv, bool has_sgs, bool has_amg,
                        int64_t sgs_rows, int64_t sgs_negative_pivots,
                        int64_t amg_rows, int64_t rows)
{
  if (nev < 1 || nev > 8)
    throw std::runtime_error("spmv::lobpcg - Error: nev must be in 1..8");
  if (kmax < 0)
    throw std::runtime_error("spmv::lobpcg - Error: kmax < 0");
  if (!(rtol >= 0.0) || !std::isfinite(rtol) || !(atol >= 0.0)
      || !std::isfinite(atol) || (rtol == 0.0 && atol == 0.0))
    throw std::runtime_error(
        "spmv::lobpcg - Error: tol: rtol and atol must be finite, not negative "
        "and not both 0");
  if ((int)has_dinv + (int)has_sgs + (int)has_amg > 1)
    throw std::runtime_error(
        "spmv::lobpcg - Error: one preconditioner at a time (dinv, sgs or amg)");
  if ((has_sgs && sgs_rows != rows) || (has_amg && amg_rows != rows))
    throw std::runtime_error(
        "spmv::lobpcg - Error: the preconditioner was built for "
        + std::to_string(has_sgs ? sgs_rows : amg_rows)
        + " rows, the matrix has " + std::to_string(rows));
  if (has_sgs && sgs_negative_pivots > 0)
    throw std::runtime_error(
        "spmv::lobpcg - Error: the preconditioner has "
        + std::to_string(sgs_negative_pivots)
        + " negative pivot(s): it is not positive definite");
}

void lobpcg_check_pencil(int64_t rows_a, int64_t rows_b, const int64_t* ghosts_a,
                         int64_t num_ghosts_a, const int64_t* ghosts_b,
                         int64_t num_ghosts_b)
{
  if (rows_a != rows_b)
    throw std::runtime_error("spmv::lobpcg - Error: pencil: B has "
                             + std::to_string(rows_b) + " local rows, A has "
                             + std::to_string(rows_a));
  if (num_ghosts_a != num_ghosts_b)
    throw std::runtime_error("spmv::lobpcg - Error: pencil: B has "
                             + std::to_string(num_ghosts_b) + " ghosts, A has "
                             + std::to_string(num_ghosts_a));
  for (int64_t i = 0; i < num_ghosts_a; ++i)
    if (ghosts_a[i] != ghosts_b[i])
      throw std::runtime_error(
          "spmv::lobpcg - Error: pencil: ghost " + std::to_string(i) + " of B is "
          + std::to_string(ghosts_b[i]) + ", of A "
          + std::to_string(ghosts_a[i])
          + " (B must have A's ghosts in A's order)");
}

void cgs_check_rules(int ns, int kmax, int64_t rows, int64_t ldx,
                     const double* shifts, const double* b, const double* X)
{
  if (ns < 1 || ns > 8)
    throw std::runtime_error("spmv::cg_shifted - Error: ns must be in 1..8");
  if (kmax < 0)
    throw std::runtime_error("spmv::cg_shifted - Error: kmax < 0");
  if (ldx < rows)
    throw std::runtime_error("spmv::cg_shifted - Error: ldx < the local rows");
  if (!shifts)
    throw std::runtime_error("spmv::cg_shifted - Error: shifts is NULL");
  for (int s = 0; s < ns; ++s)
    if (!(shifts[s] >= 0.0) || !std::isfinite(shifts[s]))
      throw std::runtime_error("spmv::cg_shifted - Error: shifts must be "
                               "finite and not negative");
  if (doubles_overlap(X, (int64_t)(ns - 1) * ldx + rows, b, rows))
    throw std::runtime_error("cg_shifted: X overlaps b (X is updated in place)");
}

void idrs_check_rules(int s, int kmax, double kappa, bool has_dinv,
                      int cheb_degree, double lmin, double lmax, bool has_sgs,
                      bool has_amg, int64_t pre_rows, int64_t rows,
                      const double* b, const double* x, const double* dinv)
{
  if (s < 1 || s > 8)
    throw std::runtime_error("spmv::idrs - Error: s must be in 1..8");
  if (kmax < 0)
    throw std::runtime_error("spmv::idrs - Error: kmax < 0");
  if (!std::isfinite(kappa) || !(kappa >= 0.0) || !(kappa < 1.0))
    throw std::runtime_error(
        "spmv::idrs - Error: kappa must be finite with 0 <= kappa < 1");
  if (has_amg && has_sgs)
    throw std::runtime_error(
        "spmv::idrs - Error: one preconditioner at a time (amg excludes sgs, "
        "dinv and the Chebyshev degree)");
  if ((has_sgs || has_amg) && (has_dinv || cheb_degree != 0))
    throw std::runtime_error(
        "spmv::idrs - Error: one preconditioner at a time (sgs and amg exclude "
        "dinv and the Chebyshev degree)");
  if (cheb_degree != 0) {
    double ca[kChebyshevMaxDegree], cb[kChebyshevMaxDegree];
    chebyshev_coefficients(cheb_degree, lmin, lmax, ca, cb);
  }
  if ((has_sgs || has_amg) && pre_rows != rows)
    throw std::runtime_error("spmv::idrs - Error: the preconditioner has "
                             + std::to_string(pre_rows) + " rows, A has "
                             + std::to_string(rows));
  if (doubles_overlap(x, rows, b, rows))
    throw std::runtime_error("idrs: x overlaps b (x is updated in place)");
  if (has_dinv && doubles_overlap(x, rows, dinv, rows))
    throw std::runtime_error("idrs: x overlaps dinv");
}

void amg_check_tail_rows(int64_t max_rows)
{
  if (max_rows < 0)
    throw std::runtime_error(
        "spmv::AmgPreconditioner::set_tail_rows - Error: tail_rows must be at "
        "least 0 (0 = no tail)");
}

void amg_check_options(double theta, int max_levels, int64_t min_coarse_rows,
                       int smooth_degree, int coarse_degree, double eig_ratio,
                       double coarse_scale)
{
  auto refuse = [](const char* what) {
    throw std::runtime_error(std::string("spmv::AmgOptions - Error: ") + what);
  };
  if (!(theta >= 0.0 && theta <= 1.0))
    refuse("theta must be in [0, 1]");
  if (max_levels < 1 || max_levels > 16)
    refuse("max_levels must be 1..16");
  if (min_coarse_rows < 1)
    refuse("min_coarse_rows must be at least 1");
  if (smooth_degree < 1 || smooth_degree > kChebyshevMaxDegree)
    refuse("smooth_degree must be 1..16");
  if (coarse_degree < 1 || coarse_degree > kChebyshevMaxDegree)
    refuse("coarse_degree must be 1..16");
  if (!(eig_ratio > 1.0) || !std::isfinite(eig_ratio))
    refuse("eig_ratio must be a finite number > 1");
  if (!(coarse_scale >= 1.0 && coarse_scale < 2.0))
    refuse("coarse_scale must satisfy 1 <= coarse_scale < 2");
}

int64_t gmres_basis_stride(int64_t N_padded)
{
  if (N_padded < 0 || N_padded == std::numeric_limits<int64_t>::max())
    throw std::runtime_error("spmv::gmres - Error: the basis stride overflows");
  return N_padded + (N_padded & 1);
}

int64_t gmres_basis_elems(int64_t N_padded, int restart)
{
  const int64_t stride = gmres_basis_stride(N_padded);
  const int64_t count = (int64_t)restart + 1;
  if (restart < 0
      || (stride != 0
          && count > std::numeric_limits<int64_t>::max() / (int64_t)sizeof(double)
                         / stride))
    throw std::runtime_error("spmv::gmres - Error: the basis overflows");
  return stride * count;
}

} // namespace spmv
