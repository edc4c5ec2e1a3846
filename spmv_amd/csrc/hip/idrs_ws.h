// Device state of spmv::idrs (blas1_idrs.hip).
#pragma once

#include "solver_ws.h"

constexpr int kIdrsMaxS = 8; // SPMV_HIP_IDRS_MAX_S
// rows of the partial array and slots of `red`
constexpr int kIdrsRowRr = 8;  // r.r (w.w of sign_dot)
constexpr int kIdrsRowTr = 9;  // t.r
constexpr int kIdrsRowTt = 10; // t.t
constexpr int kIdrsRows = 11;

// The doubles first, in the order of SPMV_HIP_IDRS_SCALARS (spmv_hip.h); the
// words behind them in the order of spmv_hip_idrs_ws_get_words.
struct IdrsScalars {
  double rtol;
  double kappa;
  double om;
  double rr;    // r.r of the iterate
  double hist0; // sqrt(b.b)
  double be;    // f_q / M[q][q]: the step of update
  double f[kIdrsMaxS];
  double c[kIdrsMaxS]; // c_q .. c_{s-1} of the step that follows
  double a[kIdrsMaxS]; // a_0 .. a_{q-1} of biortho
  // the reducers' slots (several ranks): sign sums at 0 .. s-1, r.r at [s],
  // t.r and t.t at [9] and [10]
  double red[kIdrsRows];
  double M[kIdrsMaxS * kIdrsMaxS]; // M[i][j] at i * 8 + j, lower triangular
  // read_async copies the first 4 words
  int32_t done;
  int32_t kstop;
  int32_t status; // 0 rtol / kmax / running, 1 zero pivot of M, 2 bad om
  int32_t k;      // steps completed
  int32_t kmax;
  int32_t s;
};
constexpr int kIdrsDoubles = 6 + 3 * kIdrsMaxS + kIdrsRows + kIdrsMaxS * kIdrsMaxS;
constexpr int kIdrsWords = 6;

struct spmv_hip_idrs_ws {
  spmv_hip_ctx* ctx = nullptr;
  int kmax = 0;           // capacity of the history
  int s = 0;              // of the last reset
  uint64_t seed = 0;      // of the last reset
  SolverArrays own;
  double* hist = nullptr; // kmax + 1
  double* part = nullptr; // kIdrsRows * ctx->dot_blocks: row j at j * dot_blocks
  IdrsScalars* sc = nullptr;
};
