// Device state of spmv::pcg, shared by the translation units whose kernels
// work on it (blas1_pcg.hip: the solver and the reducers; blas1_cheb.hip:
// pcg_chebyshev, which runs on the same scalars and reducers).
#pragma once

#include "solver_ws.h"

struct PcgScalars {
  double rtol;
  int32_t done;
  int32_t kstop;
};

struct spmv_hip_pcg_ws {
  spmv_hip_ctx* ctx = nullptr;
  int kmax = 0;
  SolverArrays own;
  double* zr = nullptr;          // [kmax + 1][2]: {rz[k], rr[k]}
  double* pAp = nullptr;         // kmax + 1
  double* partials = nullptr;    // p.Ap, ctx->dot_blocks
  double* partials_rz = nullptr; // r.z,  ctx->dot_blocks
  double* partials_rr = nullptr; // r.r,  ctx->dot_blocks
  PcgScalars* sc = nullptr;
};
