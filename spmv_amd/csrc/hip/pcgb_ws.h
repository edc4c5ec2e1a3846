// Device state of the block solvers, shared by the translation units whose
// kernels work on it: CgbState is the per-column stop state of spmv::cg_block
// (blas1_block.hip) and of spmv::pcg_block (blas1_pcg_block.hip); the block
// sweeps of spmv_mcgs.hip look at its all_done.
#pragma once

#include "solver_ws.h"

#define SPMV_CGB_MAX SPMV_HIP_CGB_MAX_NRHS

struct CgbState {
  double rtol;
  // {all_done, done[8], kstop[8]}: what spmv_hip_cgb_ws_read_async and
  // spmv_hip_pcgb_ws_read_async copy
  int32_t all_done;
  int32_t done[SPMV_CGB_MAX];
  int32_t kstop[SPMV_CGB_MAX];
};
static_assert(SPMV_HIP_CGB_STATE_WORDS == 1 + 2 * SPMV_CGB_MAX, "state words");

struct spmv_hip_pcgb_ws {
  spmv_hip_ctx* ctx = nullptr;
  int kmax = 0;
  int nrhs = 0;
  SolverArrays own;
  double* zr = nullptr;  // [kmax + 1][2][nrhs]: rz[k][0:nrhs], then rr[k][0:nrhs]
  double* pAp = nullptr; // [kmax + 1][nrhs]
  double* partials = nullptr;    // p.Ap, then r.z: [ctx->dot_blocks][nrhs]
  double* partials_rr = nullptr; // r.r:            [ctx->dot_blocks][nrhs]
  CgbState* st = nullptr;
};
