// Device state of spmv::lobpcg (blas1_lobpcg.hip).
#pragma once

#include "solver_ws.h"

struct LobpcgState {
  double rtol, atol;
  // read_async copies SPMV_HIP_LOBPCG_STATE_WORDS words from `done` on
  int32_t done;
  int32_t kstop;    // the iterate X holds once `done` is raised
  int32_t status;   // 0 converged / kmax / running, 1 the basis collapsed
  int32_t it;       // iterations completed
  int32_t active;   // bit c: column c has not met its test yet
  int32_t has_p;    // P and AP hold a direction (not in the first iteration)
  int32_t restarts; // Rayleigh-Ritz steps repeated without P
  int32_t basis;    // bit j: basis column j of [X, W, P] was used by the last step
  // set by reset
  int32_t largest, kmax;
};

struct spmv_hip_lobpcg_ws {
  spmv_hip_ctx* ctx = nullptr;
  int kmax = 0; // capacity of hist
  int nev = 0;
  int gram_cap = 0;        // workgroups of the Gram kernel at most
  SolverArrays own;
  double* hist = nullptr;  // [kmax + 1][nev]: ||r_c|| per iteration, -1.0 where
                           // the column had met its test before
  double* theta = nullptr; // [nev]
  double* coef = nullptr;  // [3 nev][nev]: row j = basis column j of [X, W, P]
  double* gram = nullptr;  // [2][m][m], m = blocks * nev: Gb, then Ga; the
                           // upper triangles, the rest zero (the all-reduce's)
  double* gpart = nullptr; // [gram_cap][2][m][m]: the Gram kernel's partials
  double* rn = nullptr;    // [2][nev]: ||r_c||^2 of the iteration, then of the
                           // epilogue (the all-reduces work on them)
  double* rpart = nullptr; // [ctx->dot_blocks][nev]: partials of ||r_c||^2
  LobpcgState* st = nullptr;
};
