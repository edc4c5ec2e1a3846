// Device state of spmv::minres (blas1_minres.hip).
#pragma once

#include "solver_ws.h"

// The doubles first, in the order of SPMV_HIP_MINRES_SCALARS (spmv_hip.h).
struct MinresScalars {
  double rtol;
  double alfa; // v.Av: the reducer's slot, or what update_r summed itself
  double ry;   // r2.y: the reducer's slot (the all-reduce works on it)
  // the recurrence's state between two steps
  double beta, oldb, dbar, epsln, phibar, cs, sn;
  // what the vector kernels multiply by
  double bob;       // beta / oldb: update_r, on r1
  double oldeps;    // update_xwv, on w1
  double delta;     // ... on w2
  double inv_gamma; // 1.0 / gamma
  double phi;       // the step of x along w
  double inv_beta;  // 1.0 / beta: v = y * inv_beta
  // read_async copies the first three
  int32_t done;
  int32_t kstop;
  int32_t status; // 0 converged / kmax / running, 1 beta == 0, 2 ry < 0,
                  // 3 gamma == 0
  int32_t k;      // steps completed
  int32_t kmax;
};
constexpr int kMinresDoubles = 16;

struct spmv_hip_minres_ws {
  spmv_hip_ctx* ctx = nullptr;
  int kmax = 0;            // capacity of hist
  SolverArrays own;
  double* hist = nullptr;  // kmax + 1
  double* p_alfa = nullptr; // ctx->dot_blocks: partials of v.Av
  double* p_ry = nullptr;   // ctx->dot_blocks: partials of r2.y
  MinresScalars* sc = nullptr;
};
