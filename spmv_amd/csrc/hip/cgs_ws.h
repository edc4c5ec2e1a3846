// Device state of spmv::cg_shifted (blas1_cgshift.hip).
#pragma once

#include "solver_ws.h"

constexpr int kCgsMaxNs = 8; // SPMV_HIP_CGS_MAX_NS

// The doubles first, in the order of SPMV_HIP_CGS_SCALARS (spmv_hip.h); the
// words behind them in the order of spmv_hip_cgs_ws_get_words.
struct CgsScalars {
  double rtol;
  double pq;    // p.q: the reducer's slot, or what update_r summed itself
  double rrn;   // r.r after update_r: the slot, or what step summed itself
  double rr;    // r.r in front of the step
  double a_old; // the seed's previous step length (1 in front of the first)
  double b_old; // the seed's previous beta (0 in front of the first)
  double bn;    // this step's beta: update_xp forms the seed's p = r + bn * p
  double hist0; // sqrt(r0.r0), hist_s[0] of every shift
  double sigma[kCgsMaxNs];
  double zeta[kCgsMaxNs]; // r_s = zeta_s * r; update_xp's coefficient of r
  double rho[kCgsMaxNs];  // zeta_s^k / zeta_s^(k-1)
  double cx[kCgsMaxNs];   // a * rho_n: the step of x_s along p_s
  double cp[kCgsMaxNs];   // bn * (rho_n * rho_n): update_xp, on p_s
  // read_async copies the first 3 + kCgsMaxNs words
  int32_t done;
  int32_t kstop;
  int32_t status; // 0 converged / kmax / running, 1 p.q was not positive
  int32_t its[kCgsMaxNs]; // iterations_s
  int32_t k;              // steps completed
  int32_t kmax;
  int32_t ns;
  int32_t n_act; // shifts the next step moves: act[0..n_act), ascending
  int32_t n_upd; // shifts the last step moved: upd[0..n_upd)
  int32_t act[kCgsMaxNs];
  int32_t upd[kCgsMaxNs]; // s | 8 where p_s moves too (s did not stop)
};
constexpr int kCgsDoubles = 8 + 5 * kCgsMaxNs;
constexpr int kCgsWords = 3 + kCgsMaxNs + 5 + 2 * kCgsMaxNs;

struct spmv_hip_cgs_ws {
  spmv_hip_ctx* ctx = nullptr;
  int kmax = 0;            // capacity of every history
  int ns = 0;              // of the last reset
  SolverArrays own;
  double* hist = nullptr;  // kCgsMaxNs * (kmax + 1): hist_s at s * (kmax + 1)
  double* p_pq = nullptr;  // ctx->dot_blocks: partials of p.q
  double* p_rrn = nullptr; // ctx->dot_blocks: partials of r.r
  CgsScalars* sc = nullptr;
};
