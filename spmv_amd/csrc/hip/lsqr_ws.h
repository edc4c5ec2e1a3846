// Device state of spmv::lsqr (blas1_lsqr.hip).
#pragma once

#include "solver_ws.h"

// The doubles first, in the order of SPMV_HIP_LSQR_SCALARS (spmv_hip.h).
struct LsqrScalars {
  double rtol, ltol, damp;
  double uu; // ut.ut: the reducer's slot, or what update_v summed itself
  double vv; // vn.vn: the reducer's slot, or what start / step summed itself
  // the recurrence's state between two steps
  double alpha, beta, phibar, rhobar, anorm2, psi2;
  // what the vector kernels multiply by
  double ia; // 1.0 / alpha: the scale of vt (update_u, update_v, update_xw)
  double ib; // 1.0 / beta: the scale of ut (update_u)
  double t1; // phi / rho: the step of x along w
  double t2; // theta / rho: update_xw, on w
  // read_async copies the first three
  int32_t done;
  int32_t kstop;
  int32_t status; // 0 converged / kmax / running, 1 the least-squares test,
                  // 2 the bidiagonalisation ended
  int32_t k;      // steps completed
  int32_t kmax;
};
constexpr int kLsqrDoubles = 15;

struct spmv_hip_lsqr_ws {
  spmv_hip_ctx* ctx = nullptr;
  int kmax = 0;            // capacity of either history
  SolverArrays own;
  double* hist = nullptr;  // 2 * (kmax + 1): hist_r, then hist_ar
  double* p_uu = nullptr;  // ctx->dot_blocks: partials of ut.ut
  double* p_vv = nullptr;  // ctx->dot_blocks: partials of vn.vn
  LsqrScalars* sc = nullptr;
};
