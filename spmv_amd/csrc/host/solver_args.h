// The solvers' argument rules and sizes that are plain C++ (no device, no other
// header of the mirror: tools/solver_args_check.cpp compiles solver_args.cpp
// alone, under the sanitizers).  Declared for users in cg.h.
#pragma once

#include <cstdint>

namespace spmv
{

constexpr int kChebyshevMaxDegree = 16;
constexpr int kGmresMaxRestart = 64;

// see cg.h
void chebyshev_coefficients(int degree, double lmin, double lmax, double* a,
                            double* b);

// The argument rules of gmres() (std::runtime_error): kmax < 0 ("kmax"),
// restart outside 1..kGmresMaxRestart ("restart"), an SGS preconditioner
// together with a dinv or a Chebyshev degree ("preconditioner"),
// chebyshev_coefficients' rules when cheb_degree != 0 ("degree", "bounds"),
// an SGS preconditioner of sgs_rows != rows rows ("rows").
void gmres_check_rules(int restart, int kmax, bool has_dinv, int cheb_degree,
                       double lmin, double lmax, bool has_sgs, int64_t sgs_rows,
                       int64_t rows);

// The argument rules of pcg_block() (std::runtime_error), in this order: nrhs
// outside 1..8 ("nrhs"), kmax < 0 ("kmax"), both or neither of dinv and sgs
// ("preconditioner"), an SGS / ILU(0) preconditioner of sgs_rows != rows rows
// ("rows") or with negative pivots ("pivot"), X sharing a byte with B (rows *
// nrhs doubles each) or with dinv (rows doubles) ("overlaps").  The pointers are
// compared, never dereferenced.
void pcg_block_check_rules(int nrhs, int kmax, bool has_dinv, bool has_sgs,
                           int64_t sgs_rows, int64_t sgs_negative_pivots,
                           int64_t rows, const double* B, const double* X,
                           const double* dinv);

// ... with the third preconditioner, an AmgPreconditioner of amg_rows rows:
// "preconditioner" unless exactly one of dinv, sgs and amg is set, "rows" also
// for amg_rows != rows; the other rules and their order as above.
void pcg_block_check_rules(int nrhs, int kmax, bool has_dinv, bool has_sgs,
                           bool has_amg, int64_t sgs_rows,
                           int64_t sgs_negative_pivots, int64_t amg_rows,
                           int64_t rows, const double* B, const double* X,
                           const double* dinv);
// The argument rules of amg_apply_block() (std::runtime_error): nrhs outside
// 1..8 ("nrhs"), Z sharing a byte with R, rows * nrhs doubles each
// ("overlaps").  The pointers are compared, never dereferenced.
void amg_apply_block_check_rules(int nrhs, int64_t rows, const double* R,
                                 const double* Z);

// The rules of AmgOptions (cg.h); std::runtime_error names the field: theta in
// [0, 1], max_levels 1..16, min_coarse_rows >= 1, smooth_degree and
// coarse_degree 1..kChebyshevMaxDegree, eig_ratio > 1, 1 <= coarse_scale < 2.
void amg_check_options(double theta, int max_levels, int64_t min_coarse_rows,
                       int smooth_degree, int coarse_degree, double eig_ratio,
                       double coarse_scale);
// The rule of AmgPreconditioner::set_tail_rows: max_rows >= 0; a negative value
// throws std::runtime_error naming "tail_rows".
void amg_check_tail_rows(int64_t max_rows);

// The argument rules of minres() (std::runtime_error), in this order: kmax < 0
// ("kmax"), more than one of dinv, sgs and amg ("preconditioner"), an SGS /
// ILU(0) or AMG preconditioner built for other than `rows` rows ("rows"), an
// ILU(0) preconditioner with negative pivots ("pivot": it is not positive
// definite), x sharing a byte with b or dinv, rows doubles each ("overlaps").
// The pointers are compared, never dereferenced.
void minres_check_rules(int kmax, bool has_dinv, bool has_sgs, bool has_amg,
                        int64_t sgs_rows, int64_t sgs_negative_pivots,
                        int64_t amg_rows, int64_t rows, const double* b,
                        const double* x, const double* dinv);

// The argument rules of lobpcg() (std::runtime_error), in this order: "nev" not
// in 1..8, "kmax" < 0, "tol" (rtol and atol finite, >= 0, not both 0), more
// than one "preconditioner", its "rows", a negative "pivot".
void lobpcg_check_rules(int nev, int kmax, double rtol, double atol,
                        bool has_dinv, bool has_sgs, bool has_amg,
                        int64_t sgs_rows, int64_t sgs_negative_pivots,
                        int64_t amg_rows, int64_t rows);
// The rule "pencil" of lobpcg() with B (std::runtime_error): B has A's local
// row count, and B's column map has exactly A's ghost list, the same global
// indices in the same order (two operators assembled on one mesh), so that one
// halo exchange of the padded W serves both products.  The lists are read,
// nothing else; a list of length 0 may be NULL.
void lobpcg_check_pencil(int64_t rows_a, int64_t rows_b, const int64_t* ghosts_a,
                         int64_t num_ghosts_a, const int64_t* ghosts_b,
                         int64_t num_ghosts_b);

// The argument rules of lsqr() (std::runtime_error), in this order: kmax < 0
// ("kmax"), ltol negative or not finite ("ltol"), damp negative or not finite
// ("damp"), x (cols doubles) sharing a byte with b (rows doubles) ("overlaps").
// The pointers are compared, never dereferenced.
void lsqr_check_rules(int kmax, double ltol, double damp, int64_t rows,
                      int64_t cols, const double* b, const double* x);

// The argument rules of cg_shifted() (std::runtime_error), in this order: ns
// outside 1..8 ("ns"), kmax < 0 ("kmax"), ldx < rows ("ldx"), a shift that is
// negative or not finite, or shifts == NULL ("shifts"), X ((ns - 1) * ldx + rows
// doubles) sharing a byte with b (rows doubles) ("overlaps").  shifts is a HOST
// array and is read; b and X are compared, never dereferenced.
void cgs_check_rules(int ns, int kmax, int64_t rows, int64_t ldx,
                     const double* shifts, const double* b, const double* X);

// The argument rules of idrs() (std::runtime_error), in this order: s outside
// 1..8 ("s"), kmax < 0 ("kmax"), kappa not finite or outside [0, 1) ("kappa"),
// gmres_check_rules' rules on the preconditioner ("preconditioner", "degree",
// "bounds", "rows"; amg obeys the rules of sgs), x sharing a byte with b or dinv,
// rows doubles each ("overlaps").  The pointers are compared, never
// dereferenced.
void idrs_check_rules(int s, int kmax, double kappa, bool has_dinv,
                      int cheb_degree, double lmin, double lmax, bool has_sgs,
                      bool has_amg, int64_t pre_rows, int64_t rows,
                      const double* b, const double* x, const double* dinv);

// stride of the basis vectors: N_padded rounded up to an even number, so that
// every v_j is 16-byte aligned
int64_t gmres_basis_stride(int64_t N_padded);
// doubles of the basis: restart + 1 vectors at that stride; throws
// ("overflows") when the product does not fit int64_t
int64_t gmres_basis_elems(int64_t N_padded, int restart);

} // namespace spmv
