// Kernels of spmv::lobpcg (gfx950): the block eigensolver of cg.h on blocks of
// nev INTERLEAVED vectors -- element (i, c) at V[i * nev + c], the layout of
// Matrix::mult_block.  The basis of one step is S = [X, W, P] (3 nev columns,
// column j of block b is basis column b * nev + j), AS = [AX, AW, AP].
//
//   gram      one pass over the six blocks: per-workgroup partials of the upper
//             triangles of Gb = S^T S and Ga = S^T AS
//   gram_reduce  the partials of every entry in index order -> one slot (one
//             thread per entry)
//   rr        ONE workgroup of one wave: reads the slot (or finishes the Gram sums
//             itself, in the same order), compacts them by
//             the active mask, scales, factors Gb, forms R^-T Ga R^-1, runs the
//             cyclic Jacobi iteration, selects nev Ritz values and leaves theta,
//             the coefficients C = R^-1 Z and the basis mask
//   update    X' = S C, AX' = AS C, P' = [W, P] C_wp, AP' = [AW, AP] C_wp in one
//             pass, in place (a thread owns a row).  With one block and no AX it
//             is the prologue's X R^-1 (lobpcg_orth)
//   residual  R = AX - X diag(theta), optionally W = dinv * R or W = R, and the
//             partials of ||r_c||^2
//   norms     partials -> ||r_c||, the history, the convergence mask, `done`
//
// The pencil A x = lambda B x (lobpcg() with B) adds BS = [BX, BW, BP]:
//   gram_gen    the gram kernel with the rows staged as [S | AS | BS]:
//               Gb = S^T BS (entry (i, j), i <= j: the sum of s_i * (Bs)_j), Ga
//               as before, the partials in the same layout and order, so
//               gram_reduce and rr read them unchanged and BS = S gives gram's bits
//   update_gen  the update on three triples, a thread owns a row of one triple
//   residual    with BX in X's place: R = AX - BX diag(theta)
//
// The `done` protocol is minres's: once it is raised every kernel returns at
// once, so X is exactly the iterate of the returned k.
//
// Summation order of ONE Gram entry (i, j), restated in tests/lobpcg_cases.py
// (gram_partials, gram_sum): the rows are walked in chunks of kGramRows = 64,
// workgroup b of g takes the chunks b, b + g, b + 2g, ...  Inside a chunk, row
// r (0..63) belongs to row group r % G, G = 256 / (2 T), T the number of 4 x 4
// tiles in the upper triangle of the (padded) m x m matrix.  A row group adds
// its products s_i(row) * as_j(row) one by one, rows ascending, chunks in the
// workgroup's order, from 0.0; the workgroup adds its G row groups in order
// from 0.0; the rr kernel (or gram_reduce) adds the workgroups in index order
// from 0.0.  Masked columns are summed like the others: no shape here depends
// on data.
//
// A thread of the Gram kernel holds one 4 x 4 tile of one of the two matrices:
// the 6 nev values of a row are staged once in LDS and every tile reads its 8
// of them from there, so each block is read from memory once per call (at
// nev = 8: 2688 B of LDS reads per 384 B row).  MFMA is not used: its
// accumulation order is not the one above.
//
// Built with -ffp-contract=off: every product, sum, difference, quotient and
// square root is one rounding.
#include "common.h"
#include "blas1_block.h"
#include "lobpcg_ws.h"

#include <climits>
#include <cmath>

namespace
{

constexpr int kMaxM = 3 * SPMV_CGB_MAX; // 24: columns of [X, W, P]
constexpr int kGramRows = 64;           // rows of one staged chunk
constexpr int kRrThreads = 64;          // the rr kernel is one wave
constexpr int kSweeps = 30;             // Jacobi sweeps at most
constexpr int kLd = kMaxM + 1;          // leading dimension of the LDS matrices

// ---- rows of a block ---------------------------------------------------------
// KK values of row `row`; VEC: nev is even and the block 16-byte aligned
template <int KK, bool NT, bool VEC>
__device__ __forceinline__ void load_row(const double* __restrict__ v,
                                         int64_t row, int k, double (&out)[KK])
{
  if constexpr (VEC) {
#pragma unroll
    for (int j2 = 0; j2 < KK / 2; ++j2)
      if (2 * j2 < k) {
        const f64x2 q = vload<NT>(v, (row * k) / 2 + j2);
        out[2 * j2] = q.x;
        out[2 * j2 + 1] = q.y;
      }
  } else {
#pragma unroll
    for (int j = 0; j < KK; ++j)
      if (j < k)
        out[j] = sload<NT>(v + row * k + j);
  }
}

template <int KK, bool NT, bool VEC>
__device__ __forceinline__ void store_row(double* __restrict__ v, int64_t row,
                                          int k, const double (&in)[KK])
{
  if constexpr (VEC) {
#pragma unroll
    for (int j2 = 0; j2 < KK / 2; ++j2)
      if (2 * j2 < k) {
        f64x2 q;
        q.x = in[2 * j2];
        q.y = in[2 * j2 + 1];
        vstore<NT>(v, (row * k) / 2 + j2, q);
      }
  } else {
#pragma unroll
    for (int j = 0; j < KK; ++j)
      if (j < k)
        sstore<NT>(v + row * k + j, in[j]);
  }
}

// ---- gram ----------------------------------------------------------------------
// the chunk's rows of one block into the staged rows, at column `off`
template <bool NT, bool VEC>
__device__ __forceinline__ void stage_block(const double* __restrict__ src,
                                            int64_t r0, int nr, int k,
                                            double* s_buf, int stride, int off)
{
  if constexpr (VEC) {
    const int n2 = nr * k / 2;
    for (int e2 = threadIdx.x; e2 < n2; e2 += kBlock) {
      const f64x2 q = vload<NT>(src, r0 * k / 2 + e2);
      const int e = 2 * e2;
      double* d = s_buf + (e / k) * stride + off + e % k;
      d[0] = q.x;
      d[1] = q.y;
    }
  } else {
    const int n = nr * k;
    for (int e = threadIdx.x; e < n; e += kBlock)
      s_buf[(e / k) * stride + off + e % k] = sload<NT>(src + r0 * k + e);
  }
}

// GEN: the pencil form.  The rows are staged as [S | AS | BS] and the Gb tiles
// take their right-hand operand from BS; the tiles, the row groups and the
// partials are the same, so BS = S gives the bits of the form without B.
template <bool NT, bool VEC, bool GEN>
__global__ __launch_bounds__(kBlock) void lobpcg_gram_kernel(
    int64_t M, int k, int nb, const LobpcgState* __restrict__ st,
    const double* __restrict__ S0, const double* __restrict__ S1,
    const double* __restrict__ S2, const double* __restrict__ A0,
    const double* __restrict__ A1, const double* __restrict__ A2,
    const double* __restrict__ B0, const double* __restrict__ B1,
    const double* __restrict__ B2, double* __restrict__ partials)
{
  // the staged rows (kGramRows x 2 mp <= 3072; GEN: x 3 mp <= 4608), then the
  // row groups' tiles (<= kBlock * 16)
  __shared__ double s_buf[GEN ? kGramRows * 3 * kMaxM : kBlock * 16];
  if (st->done)
    return;
  const int m = nb * k, mt = (m + 3) / 4, mp = 4 * mt;
  const int stride = (GEN ? 3 : 2) * mp;
  const int nt = mt * (mt + 1) / 2, jobs = 2 * nt, G = kBlock / jobs;
  const int t = threadIdx.x;
  const int job = t % jobs, g = t / jobs; // g == G: a thread without a tile
  const int which = job / nt;
  int ti = 0, tj = job % nt;
  while (tj >= mt - ti) {
    tj -= mt - ti;
    ++ti;
  }
  tj += ti;
  const int a_off = 4 * ti;
  const int b_off = (which ? mp : GEN ? 2 * mp : 0) + 4 * tj;

  // the padding columns stay zero: no load writes them
  for (int i = t; i < kGramRows * stride; i += kBlock)
    s_buf[i] = 0.0;
  __syncthreads();

  double acc[4][4] = {};
  for (int64_t r0 = (int64_t)blockIdx.x * kGramRows; r0 < M;
       r0 += (int64_t)gridDim.x * kGramRows) {
    const int nr = M - r0 < kGramRows ? (int)(M - r0) : kGramRows;
    stage_block<NT, VEC>(S0, r0, nr, k, s_buf, stride, 0);
    stage_block<NT, VEC>(A0, r0, nr, k, s_buf, stride, mp);
    if (nb > 1) {
      stage_block<NT, VEC>(S1, r0, nr, k, s_buf, stride, k);
      stage_block<NT, VEC>(A1, r0, nr, k, s_buf, stride, mp + k);
    }
    if (nb > 2) {
      stage_block<NT, VEC>(S2, r0, nr, k, s_buf, stride, 2 * k);
      stage_block<NT, VEC>(A2, r0, nr, k, s_buf, stride, mp + 2 * k);
    }
    if constexpr (GEN) {
      stage_block<NT, VEC>(B0, r0, nr, k, s_buf, stride, 2 * mp);
      if (nb > 1)
        stage_block<NT, VEC>(B1, r0, nr, k, s_buf, stride, 2 * mp + k);
      if (nb > 2)
        stage_block<NT, VEC>(B2, r0, nr, k, s_buf, stride, 2 * mp + 2 * k);
    }
    __syncthreads();
    if (g < G) {
      for (int r = g; r < nr; r += G) {
        const double* row = s_buf + r * stride;
        double a[4], b[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          a[x] = row[a_off + x];
          b[x] = row[b_off + x];
        }
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y)
            acc[x][y] += a[x] * b[y];
      }
    }
    __syncthreads(); // the next chunk overwrites the rows
  }

  if (g < G) {
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y)
        s_buf[(g * jobs + job) * 16 + 4 * x + y] = acc[x][y];
  }
  __syncthreads();
  const int mm = m * m;
  double* out = partials + (int64_t)blockIdx.x * 2 * mm;
  for (int e = t; e < 2 * mm; e += kBlock) {
    const int w = e / mm, i = (e % mm) / m, j = e % m;
    double s = 0.0;
    if (i <= j) {
      const int bi = i / 4, bj = j / 4;
      const int tile = w * nt + bi * mt - bi * (bi - 1) / 2 + (bj - bi);
      for (int q = 0; q < G; ++q)
        s += s_buf[(q * jobs + tile) * 16 + 4 * (i % 4) + j % 4];
    }
    out[e] = s;
  }
}

// entry e of the Gram sums: the workgroups' partials in index order
__device__ __forceinline__ double gram_entry(const double* __restrict__ partials,
                                             int nparts, int mm2, int e)
{
  double s = 0.0;
#pragma unroll 8 // (the loads are independent, the adds stay in order)
  for (int b = 0; b < nparts; ++b)
    s += partials[(int64_t)b * mm2 + e];
  return s;
}

// partials -> the slot the rr kernel reads (and, with several ranks, the
// all-reduce works on): one thread per entry, so the chains of a step run side
// by side instead of 18 deep in the one wave of the rr kernel
__global__ __launch_bounds__(kRrThreads) void lobpcg_gram_reduce_kernel(
    const LobpcgState* __restrict__ st, int m, const double* __restrict__ partials,
    int nparts, double* __restrict__ slot)
{
  if (st->done)
    return;
  const int mm = m * m;
  const int e = blockIdx.x * kRrThreads + threadIdx.x;
  if (e < 2 * mm) {
    const int i = (e % mm) / m, j = e % m;
    slot[e] = i <= j ? gram_entry(partials, nparts, 2 * mm, e) : 0.0;
  }
}

// ---- rr --------------------------------------------------------------------------
// mode 0: the Rayleigh-Ritz step; mode 1: C = D R^-1 alone (the prologue's
// orthonormalisation: no Jacobi, no theta).  nparts > 0: src holds partials;
// nparts == 0: src is the reduced slot.  advance: a step that succeeds
// completes an iteration.
//
// Jacobi rules: pairs (p, q), p < q, row by row.  A pair whose entry is 0 is
// skipped.  A pair whose entry g changes neither |b_pp| + |g| nor |b_qq| + |g|
// is set to 0 and not rotated.  Otherwise tau = (b_qq - b_pp) / (2 g),
// t = sign(tau) / (|tau| + sqrt(1 + tau tau)) (sign(0) = 1),
// c = 1 / sqrt(1 + t t), s = t c.  The iteration stops after the first sweep
// that rotates nothing, or after kSweeps sweeps.
__global__ __launch_bounds__(kRrThreads) void lobpcg_rr_kernel(
    LobpcgState* __restrict__ st, int k, int nb, int mode, int advance,
    const double* __restrict__ src, int nparts, double* __restrict__ coef,
    double* __restrict__ theta)
{
  __shared__ double s_raw[2 * kMaxM * kMaxM];
  __shared__ double s_b[kMaxM][kLd], s_a[kMaxM][kLd], s_z[kMaxM][kLd];
  __shared__ double s_v[kMaxM][SPMV_CGB_MAX + 1];
  __shared__ double s_d[kMaxM], s_rd[kMaxM], s_th[kMaxM];
  __shared__ int s_idx[kMaxM], s_sel[SPMV_CGB_MAX], s_m, s_mask;
  if (st->done)
    return;
  const int t = threadIdx.x;
  const int mf = nb * k, mm = mf * mf;
  for (int e = t; e < 2 * mm; e += kRrThreads) {
    const int i = (e % mm) / mf, j = e % mf;
    double v = 0.0;
    if (i <= j)
      v = nparts ? gram_entry(src, nparts, 2 * mm, e) : src[e];
    s_raw[e] = v;
  }
  const int active = st->active, has_p = st->has_p, largest = st->largest;
  __syncthreads();

  bool fail = false;
  int attempt = 0, m = 0;
  for (; attempt < 2; ++attempt) {
    const bool use_p = nb == 3 && has_p && attempt == 0;
    if (attempt == 1 && !(nb == 3 && has_p))
      break; // there is no P to drop
    fail = false;
    if (t == 0) {
      int n = 0, mask = 0;
      for (int c = 0; c < k; ++c)
        s_idx[n++] = c;
      if (nb >= 2)
        for (int c = 0; c < k; ++c)
          if ((active >> c) & 1)
            s_idx[n++] = k + c;
      if (use_p)
        for (int c = 0; c < k; ++c)
          if ((active >> c) & 1)
            s_idx[n++] = 2 * k + c;
      for (int a = 0; a < n; ++a)
        mask |= 1 << s_idx[a];
      s_m = n;
      s_mask = mask;
    }
    __syncthreads();
    m = s_m;
    if (t < m)
      s_d[t] = 1.0 / sqrt(s_raw[s_idx[t] * mf + s_idx[t]]);
    __syncthreads();
    for (int e = t; e < m * m; e += kRrThreads) {
      const int a = e / m, b = e % m;
      const int lo = a < b ? a : b, hi = a < b ? b : a;
      const int at = s_idx[lo] * mf + s_idx[hi];
      s_b[a][b] = (s_raw[at] * s_d[lo]) * s_d[hi];
      s_a[a][b] = (s_raw[mm + at] * s_d[lo]) * s_d[hi];
      s_z[a][b] = a == b ? 1.0 : 0.0;
    }
    __syncthreads();

    // Gb = R^T R, R over the upper triangle, its diagonal in s_rd
    for (int j = 0; j < m; ++j) {
      double piv = s_b[j][j];
      for (int p = 0; p < j; ++p)
        piv -= s_b[p][j] * s_b[p][j];
      if (!(piv > 0.0)) { // the same in every thread; a NaN fails too
        fail = true;
        break;
      }
      const double rjj = sqrt(piv);
      if (t == j)
        s_rd[j] = rjj;
      if (t > j && t < m) {
        double v = s_b[j][t];
        for (int p = 0; p < j; ++p)
          v -= s_b[p][j] * s_b[p][t];
        s_b[j][t] = v / rjj;
      }
      __syncthreads();
    }

    if (!fail && mode == 0) {
      // Y = R^-T Ga (thread = column), then B = Y R^-1 (thread = row), in place
      if (t < m)
        for (int i = 0; i < m; ++i) {
          double v = s_a[i][t];
          for (int p = 0; p < i; ++p)
            v -= s_b[p][i] * s_a[p][t];
          s_a[i][t] = v / s_rd[i];
        }
      __syncthreads();
      if (t < m)
        for (int j = 0; j < m; ++j) {
          double v = s_a[t][j];
          for (int p = 0; p < j; ++p)
            v -= s_a[t][p] * s_b[p][j];
          s_a[t][j] = v / s_rd[j];
        }
      __syncthreads();
      for (int e = t; e < m * m; e += kRrThreads) {
        const int a = e / m, b = e % m;
        if (a < b)
          s_a[b][a] = s_a[a][b];
      }
      __syncthreads();

      for (int sweep = 0; sweep < kSweeps; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < m - 1; ++p)
          for (int q = p + 1; q < m; ++q) {
            const double apq = s_a[p][q], app = s_a[p][p], aqq = s_a[q][q];
            if (apq == 0.0)
              continue; // (the same in every thread)
            const double g = fabs(apq);
            const bool small = fabs(app) + g == fabs(app)
                               && fabs(aqq) + g == fabs(aqq);
            double tt = 0.0, c = 1.0, s = 0.0;
            if (!small) {
              const double tau = (aqq - app) / (2.0 * apq);
              tt = 1.0 / (fabs(tau) + sqrt(1.0 + tau * tau));
              if (tau < 0.0)
                tt = -tt;
              c = 1.0 / sqrt(1.0 + tt * tt);
              s = tt * c;
            }
            const int zr = t - 32;
            double brp = 0.0, brq = 0.0, zp = 0.0, zq = 0.0;
            if (t < m) {
              brp = s_a[t][p];
              brq = s_a[t][q];
            }
            if (zr >= 0 && zr < m) {
              zp = s_z[zr][p];
              zq = s_z[zr][q];
            }
            __syncthreads(); // every read of this pair before any write
            if (small) {
              if (t == 0) {
                s_a[p][q] = 0.0;
                s_a[q][p] = 0.0;
              }
            } else {
              rotated = true;
              if (t == p) {
                s_a[p][p] = app - tt * apq;
                s_a[p][q] = 0.0;
              } else if (t == q) {
                s_a[q][q] = aqq + tt * apq;
                s_a[q][p] = 0.0;
              } else if (t < m) {
                const double np = c * brp - s * brq;
                const double nq = s * brp + c * brq;
                s_a[t][p] = np;
                s_a[p][t] = np;
                s_a[t][q] = nq;
                s_a[q][t] = nq;
              }
              if (zr >= 0 && zr < m) {
                s_z[zr][p] = c * zp - s * zq;
                s_z[zr][q] = s * zp + c * zq;
              }
            }
            __syncthreads();
          }
        if (!rotated)
          break;
      }

      // nev Ritz values, ascending (descending: largest), ties by index
      for (int a = 0; a < m; ++a) {
        const double th = s_a[a][a];
        if (!(th - th == 0.0))
          fail = true; // a Ritz value that is not finite: breakdown as well
      }
      if (t < m) {
        const double th = s_a[t][t];
        int rank = 0;
        for (int b = 0; b < m; ++b) {
          const double tb = s_a[b][b];
          const bool before = largest ? tb > th : tb < th;
          if (before || (tb == th && b < t))
            ++rank;
        }
        s_th[t] = th;
        if (rank < k && !fail)
          s_sel[rank] = t;
      }
    } else if (!fail) {
      if (t < k)
        s_sel[t] = t;
    }
    __syncthreads();
    if (!fail)
      break;
  }

  if (fail) { // with P and without: the basis has collapsed
    if (t == 0) {
      st->status = 1;
      st->kstop = st->it;
      st->done = 1;
    }
    return;
  }
  // C = D R^-1 Z(:, sel): back substitution, thread = column
  if (t < k) {
    const int zc = s_sel[t];
    for (int i = m - 1; i >= 0; --i) {
      double v = s_z[i][zc];
      for (int p = i + 1; p < m; ++p)
        v -= s_b[i][p] * s_v[p][t];
      s_v[i][t] = v / s_rd[i];
    }
  }
  __syncthreads();
  for (int e = t; e < mf * k; e += kRrThreads) {
    const int j = e / k, c = e % k;
    double v = 0.0;
    for (int a = 0; a < m; ++a)
      if (s_idx[a] == j)
        v = s_v[a][c] * s_d[a];
    coef[e] = v;
  }
  if (mode == 0 && t < k)
    theta[t] = s_th[s_sel[t]];
  if (t == 0) {
    st->basis = s_mask;
    if (attempt == 1)
      st->restarts += 1;
    if (mode == 0 && nb == 3)
      st->has_p = 1;
    if (advance)
      st->it += 1;
  }
}

// ---- update ------------------------------------------------------------------------
// one half of the update on one row: xo = [s0, s1, s2] C over the basis columns
// in use, po = [s1, s2] C_wp for the active columns (a column that has met its
// test keeps the P it has)
template <int KK>
__device__ __forceinline__ void combine_row(const double (&s)[3][KK], int k,
                                            int nb, int basis, int active,
                                            const double* s_c, double (&xo)[KK],
                                            double (&po)[KK])
{
#pragma unroll
  for (int c = 0; c < KK; ++c) {
    if (c < k) {
      double ax = 0.0, ap = 0.0;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        if (b < nb) {
#pragma unroll
          for (int j = 0; j < KK; ++j) {
            if (j < k && ((basis >> (b * k + j)) & 1)) {
              const double cf = s_c[(b * k + j) * k + c];
              ax += s[b][j] * cf;
              if (b > 0)
                ap += s[b][j] * cf;
            }
          }
        }
      }
      xo[c] = ax;
      po[c] = ((active >> c) & 1) ? ap : s[2][c];
    }
  }
}

// K = 1, 2, 4, 8: that width; K = 0: nev at run time
template <int K, bool NT, bool VEC>
__global__ __launch_bounds__(kBlock) void lobpcg_update_kernel(
    int64_t M, int nev, int nb, const LobpcgState* __restrict__ st,
    const double* __restrict__ coef, double* __restrict__ X,
    const double* __restrict__ W, double* __restrict__ P,
    double* __restrict__ AX, const double* __restrict__ AW,
    double* __restrict__ AP)
{
  constexpr int KK = K ? K : SPMV_CGB_MAX;
  __shared__ double s_c[kMaxM * SPMV_CGB_MAX];
  if (st->done)
    return;
  const int k = K ? K : nev;
  for (int e = threadIdx.x; e < nb * k * k; e += kBlock)
    s_c[e] = coef[e];
  const int basis = st->basis, active = st->active;
  __syncthreads();
  SPMV_FOR_ROWS(row, M)
  {
    double s[3][KK] = {}, xo[KK], po[KK];
    load_row<KK, NT, VEC>(X, row, k, s[0]);
    if (nb == 3) {
      load_row<KK, NT, VEC>(W, row, k, s[1]);
      load_row<KK, NT, VEC>(P, row, k, s[2]);
    }
    combine_row<KK>(s, k, nb, basis, active, s_c, xo, po);
    store_row<KK, NT, VEC>(X, row, k, xo);
    if (nb == 3)
      store_row<KK, NT, VEC>(P, row, k, po);
    if (AX) {
      load_row<KK, NT, VEC>(AX, row, k, s[0]);
      if (nb == 3) {
        load_row<KK, NT, VEC>(AW, row, k, s[1]);
        load_row<KK, NT, VEC>(AP, row, k, s[2]);
      }
      combine_row<KK>(s, k, nb, basis, active, s_c, xo, po);
      store_row<KK, NT, VEC>(AX, row, k, xo);
      if (nb == 3)
        store_row<KK, NT, VEC>(AP, row, k, po);
    }
  }
}

// The pencil form: the triples [X, W, P], [AX, AW, AP], [BX, BW, BP] are
// independent given C, so blockIdx.y picks one and a thread holds 3 nev values
// of a row, not 6 nev (or 9 nev).  combine_row is the arithmetic of the kernel
// above.  A triple whose first block is NULL is skipped.
struct LobpcgTriples {
  double* x[3];
  const double* w[3];
  double* p[3];
};

template <int K, bool NT, bool VEC>
__global__ __launch_bounds__(kBlock) void lobpcg_update_triple_kernel(
    int64_t M, int nev, int nb, const LobpcgState* __restrict__ st,
    const double* __restrict__ coef, LobpcgTriples tr)
{
  constexpr int KK = K ? K : SPMV_CGB_MAX;
  __shared__ double s_c[kMaxM * SPMV_CGB_MAX];
  double* __restrict__ X = tr.x[blockIdx.y];
  const double* __restrict__ W = tr.w[blockIdx.y];
  double* __restrict__ P = tr.p[blockIdx.y];
  if (st->done || !X)
    return;
  const int k = K ? K : nev;
  for (int e = threadIdx.x; e < nb * k * k; e += kBlock)
    s_c[e] = coef[e];
  const int basis = st->basis, active = st->active;
  __syncthreads();
  SPMV_FOR_ROWS(row, M)
  {
    double s[3][KK] = {}, xo[KK], po[KK];
    load_row<KK, NT, VEC>(X, row, k, s[0]);
    if (nb == 3) {
      load_row<KK, NT, VEC>(W, row, k, s[1]);
      load_row<KK, NT, VEC>(P, row, k, s[2]);
    }
    combine_row<KK>(s, k, nb, basis, active, s_c, xo, po);
    store_row<KK, NT, VEC>(X, row, k, xo);
    if (nb == 3)
      store_row<KK, NT, VEC>(P, row, k, po);
  }
}

// ---- residual ------------------------------------------------------------------------
// R = AX - X diag(theta) (the pencil: BX stands in X's place); W (optional) =
// dinv * R, or R; partials of ||r_c||^2.
// final: the epilogue's call, which runs although `done` is raised
template <int K, bool NT, bool VEC>
__global__ __launch_bounds__(kBlock) void lobpcg_residual_kernel(
    int64_t M, int nev, const LobpcgState* __restrict__ st, int final,
    const double* __restrict__ theta, const double* __restrict__ X,
    const double* __restrict__ AX, const double* __restrict__ dinv,
    double* __restrict__ R, double* __restrict__ W,
    double* __restrict__ partials, int len)
{
  constexpr int KK = K ? K : SPMV_CGB_MAX;
  __shared__ double s_red[kBlock / 64];
  if (!final && st->done)
    return;
  const int k = K ? K : nev;
  double th[KK];
#pragma unroll
  for (int c = 0; c < KK; ++c)
    th[c] = c < k ? theta[c] : 0.0;
  double acc[SPMV_CGB_MAX] = {};
  SPMV_FOR_ROWS(row, M)
  {
    double x[KK], ax[KK], r[KK], w[KK];
    load_row<KK, NT, VEC>(X, row, k, x);
    load_row<KK, NT, VEC>(AX, row, k, ax);
    const double d = dinv ? dinv[row] : 1.0;
#pragma unroll
    for (int c = 0; c < KK; ++c) {
      if (c < k) {
        r[c] = ax[c] - x[c] * th[c];
        acc[c] += r[c] * r[c];
        w[c] = dinv ? d * r[c] : r[c];
      }
    }
    store_row<KK, NT, VEC>(R, row, k, r);
    if (W)
      store_row<KK, NT, VEC>(W, row, k, w);
  }
  rows_epilogue(acc, k, s_red, partials, len);
}

// ---- norms ---------------------------------------------------------------------------
// phase 0: partials -> ||r_c||^2 and the decision; 1: the sums alone (several
// ranks: the all-reduce follows); 2: the decision from the reduced sums.
// final: sums into the epilogue's slot, no decision, `done` ignored.
// The decision (thread 0): rn_c = sqrt(sum); an active column's history gets
// rn_c; it has met its test when rn_c < max(rtol |theta_c|, atol) (a NaN says
// "go on") and is then inactive for good; `done` once no column is active or
// it == kmax.
__global__ __launch_bounds__(kBlock) void lobpcg_norms_kernel(
    LobpcgState* __restrict__ st, int k, int phase, int final,
    const double* __restrict__ partials, int len, double* __restrict__ rn,
    const double* __restrict__ theta, double* __restrict__ hist)
{
  __shared__ double s_red[kBlock / 64];
  if (!final && st->done)
    return;
  double* slot = final ? rn + k : rn;
  if (phase != 2) {
    for (int c = 0; c < k; ++c) {
      const double s = reduce_column(partials, len, k, c, s_red);
      if (threadIdx.x == 0)
        slot[c] = s;
    }
  }
  if (final || phase == 1 || threadIdx.x != 0)
    return;
  const int it = st->it;
  int active = st->active;
  for (int c = 0; c < k; ++c) {
    if (!((active >> c) & 1))
      continue;
    const double r = sqrt(slot[c]);
    hist[(int64_t)it * k + c] = r;
    const double a = st->rtol * fabs(theta[c]);
    const double tol = a > st->atol ? a : st->atol;
    if (r < tol)
      active &= ~(1 << c);
  }
  st->active = active;
  if (active == 0 || it >= st->kmax) {
    st->kstop = it;
    st->done = 1;
  }
}

__global__ void lobpcg_reset_kernel(LobpcgState* st, double rtol, double atol,
                                    int kmax, int largest, int nev, double* hist,
                                    int count, double* theta, double* rn)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    st->rtol = rtol;
    st->atol = atol;
    st->done = 0;
    st->kstop = 0;
    st->status = 0;
    st->it = 0;
    st->active = (1 << nev) - 1;
    st->has_p = 0;
    st->restarts = 0;
    st->basis = 0;
    st->largest = largest;
    st->kmax = kmax;
  }
  if (i < nev) {
    theta[i] = 0.0;
    rn[i] = 0.0;
    rn[nev + i] = 0.0;
  }
  if (i < count)
    hist[i] = -1.0;
}

__global__ void lobpcg_set_state_kernel(LobpcgState* st, int active, int has_p,
                                        int it, int done)
{
  st->active = active;
  st->has_p = has_p;
  st->it = it;
  st->done = done;
}

int gram_grid(const spmv_hip_lobpcg_ws* ws, int64_t M)
{
  const int64_t chunks = (M + kGramRows - 1) / kGramRows;
  if (chunks < 1)
    return 1;
  return chunks < ws->gram_cap ? (int)chunks : ws->gram_cap;
}

bool blocks_ok(int nb) { return nb == 1 || nb == 3; }

} // namespace

#define SPMV_LOBPCG_REQUIRE(ctx, ws)                                           \
  SPMV_REQUIRE((ctx) && (ws) && (ws)->ctx == (ctx))

// K = 1, 2, 4, 8 natively, other widths at run time; 16-byte accesses for an
// even nev when every block is aligned; non-temporal from blas1_nt_min_elems on
#define SPMV_LOBPCG_LAUNCH_3(kernel, K, nt, vec, grid, st, ...)                \
  do {                                                                         \
    if ((nt) && (vec))                                                         \
      hipLaunchKernelGGL((kernel<K, true, true>), dim3(grid), dim3(kBlock), 0, \
                         st, __VA_ARGS__);                                     \
    else if (nt)                                                               \
      hipLaunchKernelGGL((kernel<K, true, false>), dim3(grid), dim3(kBlock),   \
                         0, st, __VA_ARGS__);                                  \
    else if (vec)                                                              \
      hipLaunchKernelGGL((kernel<K, false, true>), dim3(grid), dim3(kBlock),   \
                         0, st, __VA_ARGS__);                                  \
    else                                                                       \
      hipLaunchKernelGGL((kernel<K, false, false>), dim3(grid), dim3(kBlock),  \
                         0, st, __VA_ARGS__);                                  \
  } while (0)
#define SPMV_LOBPCG_LAUNCH_ROWS(kernel, nev, nt, vec, grid, st, ...)           \
  do {                                                                         \
    if ((nev) == 1)                                                            \
      SPMV_LOBPCG_LAUNCH_3(kernel, 1, nt, false, grid, st, __VA_ARGS__);       \
    else if ((nev) == 2)                                                       \
      SPMV_LOBPCG_LAUNCH_3(kernel, 2, nt, vec, grid, st, __VA_ARGS__);         \
    else if ((nev) == 4)                                                       \
      SPMV_LOBPCG_LAUNCH_3(kernel, 4, nt, vec, grid, st, __VA_ARGS__);         \
    else if ((nev) == 8)                                                       \
      SPMV_LOBPCG_LAUNCH_3(kernel, 8, nt, vec, grid, st, __VA_ARGS__);         \
    else                                                                       \
      SPMV_LOBPCG_LAUNCH_3(kernel, 0, nt, false, grid, st, __VA_ARGS__);       \
  } while (0)

extern "C" {

int spmv_hip_lobpcg_ws_create(spmv_hip_ctx* ctx, int kmax, int nev,
                              spmv_hip_lobpcg_ws** out)
{
  SPMV_REQUIRE(out);
  *out = nullptr;
  SPMV_REQUIRE(ctx && nrhs_ok(nev));
  SPMV_REQUIRE(kmax >= 0 && kmax < INT_MAX / (4 * SPMV_CGB_MAX));
  return solver_ws_create(ctx, kmax, out, [&](spmv_hip_lobpcg_ws& w) {
    w.nev = nev;
    const int two_per_cu = 2 * ctx->num_cus;
    w.gram_cap = two_per_cu < ctx->dot_blocks ? two_per_cu : ctx->dot_blocks;
    if (w.gram_cap < 1)
      w.gram_cap = 1;
    const size_t mm2 = 2 * (size_t)(3 * nev) * (3 * nev);
    w.own.alloc(w.hist, ((size_t)kmax + 1) * nev);
    w.own.alloc(w.theta, nev);
    w.own.alloc(w.coef, (size_t)3 * nev * nev);
    w.own.alloc(w.gram, mm2);
    w.own.alloc(w.gpart, mm2 * w.gram_cap);
    w.own.alloc(w.rn, (size_t)2 * nev);
    w.own.alloc(w.rpart, (size_t)ctx->dot_blocks * nev);
    w.own.alloc(w.st, 1);
  });
}

int spmv_hip_lobpcg_ws_destroy(spmv_hip_lobpcg_ws* ws)
{
  return solver_ws_destroy(ws);
}

int spmv_hip_lobpcg_ws_reset(spmv_hip_lobpcg_ws* ws, double rtol, double atol,
                             int kmax, int largest, void* stream)
{
  SPMV_REQUIRE(ws && kmax >= 0 && kmax <= ws->kmax);
  SPMV_SET_DEVICE(ws->ctx);
  const int count = (ws->kmax + 1) * ws->nev;
  hipLaunchKernelGGL(lobpcg_reset_kernel, ws_reset_grid(count), dim3(kBlock), 0,
                     spmv_stream(ws->ctx, stream), ws->st, rtol, atol, kmax,
                     largest ? 1 : 0, ws->nev, ws->hist, count, ws->theta,
                     ws->rn);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_ws_capacity(const spmv_hip_lobpcg_ws* ws, int* kmax,
                                int* nev)
{
  SPMV_REQUIRE(ws && kmax && nev);
  *kmax = ws->kmax;
  *nev = ws->nev;
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_ws_array(spmv_hip_lobpcg_ws* ws, int which, double** p,
                             int64_t* len)
{
  SPMV_REQUIRE(ws && p);
  const int nev = ws->nev;
  const int64_t mm2 = 2 * (int64_t)(3 * nev) * (3 * nev);
  int64_t n = 0;
  switch (which) {
  case SPMV_HIP_LOBPCG_HIST:
    *p = ws->hist;
    n = ((int64_t)ws->kmax + 1) * nev;
    break;
  case SPMV_HIP_LOBPCG_THETA:
    *p = ws->theta;
    n = nev;
    break;
  case SPMV_HIP_LOBPCG_COEF:
    *p = ws->coef;
    n = 3 * nev * nev;
    break;
  case SPMV_HIP_LOBPCG_GRAM:
    *p = ws->gram;
    n = mm2;
    break;
  case SPMV_HIP_LOBPCG_GPART:
    *p = ws->gpart;
    n = mm2 * ws->gram_cap;
    break;
  case SPMV_HIP_LOBPCG_RN:
    *p = ws->rn;
    n = 2 * nev;
    break;
  case SPMV_HIP_LOBPCG_RPART:
    *p = ws->rpart;
    n = (int64_t)ws->ctx->dot_blocks * nev;
    break;
  default:
    return SPMV_HIP_EINVAL;
  }
  if (len)
    *len = n;
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_ws_read_async(spmv_hip_lobpcg_ws* ws, int32_t* host_state,
                                  double* host_hist, size_t host_hist_len,
                                  double* host_scalars, void* stream)
{
  SPMV_REQUIRE(ws);
  const int rc = ws_read_async(ws->ctx, stream, host_state, &ws->st->done,
                               SPMV_HIP_LOBPCG_STATE_WORDS, host_hist,
                               host_hist_len, ws->hist,
                               ((size_t)ws->kmax + 1) * (size_t)ws->nev);
  if (rc != SPMV_HIP_OK)
    return rc;
  hipStream_t st = spmv_stream(ws->ctx, stream);
  if (host_scalars) { // theta[nev], then rn[2][nev]
    SPMV_CHECK_HIP(hipMemcpyAsync(host_scalars, ws->theta,
                                  sizeof(double) * ws->nev,
                                  hipMemcpyDeviceToHost, st));
    SPMV_CHECK_HIP(hipMemcpyAsync(host_scalars + ws->nev, ws->rn,
                                  sizeof(double) * 2 * ws->nev,
                                  hipMemcpyDeviceToHost, st));
  }
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_ws_set_state(spmv_hip_lobpcg_ws* ws, int active, int has_p,
                                 int it, int done, void* stream)
{
  SPMV_REQUIRE(ws && it >= 0 && it <= ws->kmax);
  SPMV_REQUIRE(active >= 0 && active < (1 << ws->nev));
  SPMV_SET_DEVICE(ws->ctx);
  hipLaunchKernelGGL(lobpcg_set_state_kernel, dim3(1), dim3(1), 0,
                     spmv_stream(ws->ctx, stream), ws->st, active,
                     has_p ? 1 : 0, it, done ? 1 : 0);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_gram_grid(const spmv_hip_lobpcg_ws* ws, int64_t M, int* grid)
{
  SPMV_REQUIRE(ws && grid && M >= 0);
  *grid = gram_grid(ws, M);
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_gram_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                             int64_t M, int blocks, const double* X,
                             const double* W, const double* P, const double* AX,
                             const double* AW, const double* AP, void* stream)
{
  SPMV_LOBPCG_REQUIRE(ctx, ws);
  SPMV_REQUIRE(M >= 0 && blocks_ok(blocks));
  SPMV_REQUIRE(M == 0 || (X && AX));
  SPMV_REQUIRE(M == 0 || blocks == 1 || (W && P && AW && AP));
  SPMV_SET_DEVICE(ctx);
  const int nev = ws->nev;
  const bool nt = M * nev >= ctx->blas1_nt_min_elems;
  const bool vec = nev % 2 == 0
                   && (blocks == 1 ? aligned16(X, AX)
                                   : aligned16(X, W, P, AX, AW, AP));
  hipStream_t st = spmv_stream(ctx, stream);
  const int grid = gram_grid(ws, M);
  const double* const none = nullptr;
#define SPMV_LOBPCG_GRAM(NT, VEC)                                              \
  hipLaunchKernelGGL((lobpcg_gram_kernel<NT, VEC, false>), dim3(grid),         \
                     dim3(kBlock), 0, st, M, nev, blocks, ws->st, X, W, P, AX, \
                     AW, AP, none, none, none, ws->gpart)
  if (nt && vec)
    SPMV_LOBPCG_GRAM(true, true);
  else if (nt)
    SPMV_LOBPCG_GRAM(true, false);
  else if (vec)
    SPMV_LOBPCG_GRAM(false, true);
  else
    SPMV_LOBPCG_GRAM(false, false);
#undef SPMV_LOBPCG_GRAM
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_gram_gen_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                                 int64_t M, int blocks, const double* X,
                                 const double* W, const double* P,
                                 const double* AX, const double* AW,
                                 const double* AP, const double* BX,
                                 const double* BW, const double* BP,
                                 void* stream)
{
  SPMV_LOBPCG_REQUIRE(ctx, ws);
  SPMV_REQUIRE(M >= 0 && blocks_ok(blocks));
  SPMV_REQUIRE(M == 0 || (X && AX && BX));
  SPMV_REQUIRE(M == 0 || blocks == 1 || (W && P && AW && AP && BW && BP));
  SPMV_SET_DEVICE(ctx);
  const int nev = ws->nev;
  const bool nt = M * nev >= ctx->blas1_nt_min_elems;
  const bool vec
      = nev % 2 == 0
        && (blocks == 1 ? aligned16(X, AX, BX)
                        : aligned16(X, W, P, AX, AW, AP, BX, BW, BP));
  hipStream_t st = spmv_stream(ctx, stream);
  const int grid = gram_grid(ws, M);
#define SPMV_LOBPCG_GRAM(NT, VEC)                                              \
  hipLaunchKernelGGL((lobpcg_gram_kernel<NT, VEC, true>), dim3(grid),          \
                     dim3(kBlock), 0, st, M, nev, blocks, ws->st, X, W, P, AX, \
                     AW, AP, BX, BW, BP, ws->gpart)
  if (nt && vec)
    SPMV_LOBPCG_GRAM(true, true);
  else if (nt)
    SPMV_LOBPCG_GRAM(true, false);
  else if (vec)
    SPMV_LOBPCG_GRAM(false, true);
  else
    SPMV_LOBPCG_GRAM(false, false);
#undef SPMV_LOBPCG_GRAM
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_gram_reduce(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                                int64_t M, int blocks, void* stream)
{
  SPMV_LOBPCG_REQUIRE(ctx, ws);
  SPMV_REQUIRE(M >= 0 && blocks_ok(blocks));
  SPMV_SET_DEVICE(ctx);
  const int m = blocks * ws->nev;
  hipLaunchKernelGGL(lobpcg_gram_reduce_kernel,
                     dim3((2 * m * m + kRrThreads - 1) / kRrThreads),
                     dim3(kRrThreads), 0, spmv_stream(ctx, stream), ws->st, m,
                     ws->gpart, gram_grid(ws, M), ws->gram);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_rr(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws, int64_t M,
                       int blocks, int mode, int reduced, int advance,
                       void* stream)
{
  SPMV_LOBPCG_REQUIRE(ctx, ws);
  SPMV_REQUIRE(M >= 0 && blocks_ok(blocks) && (mode == 0 || mode == 1));
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(lobpcg_rr_kernel, dim3(1), dim3(kRrThreads), 0,
                     spmv_stream(ctx, stream), ws->st, ws->nev, blocks, mode,
                     advance ? 1 : 0, reduced ? ws->gram : ws->gpart,
                     reduced ? 0 : gram_grid(ws, M), ws->coef, ws->theta);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_update_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                               int64_t M, int blocks, double* X, const double* W,
                               double* P, double* AX, const double* AW,
                               double* AP, void* stream)
{
  SPMV_LOBPCG_REQUIRE(ctx, ws);
  SPMV_REQUIRE(M >= 0 && blocks_ok(blocks));
  SPMV_REQUIRE(M == 0 || X);
  SPMV_REQUIRE(M == 0 || blocks == 1 || (W && P));
  SPMV_REQUIRE(M == 0 || blocks == 1 || !AX || (AW && AP));
  SPMV_SET_DEVICE(ctx);
  const int nev = ws->nev;
  const bool nt = M * nev >= ctx->blas1_nt_min_elems;
  bool vec = nev % 2 == 0 && aligned16(X, AX);
  if (blocks == 3)
    vec = vec && aligned16(W, P, AW, AP);
  hipStream_t st = spmv_stream(ctx, stream);
  SPMV_LOBPCG_LAUNCH_ROWS(lobpcg_update_kernel, nev, nt, vec, rows_grid(ctx, M),
                          st, M, nev, blocks, ws->st, ws->coef, X, W, P, AX, AW,
                          AP);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_residual_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                                 int64_t M, const double* X, const double* AX,
                                 const double* dinv, double* R, double* W,
                                 int final, void* stream)
{
  SPMV_LOBPCG_REQUIRE(ctx, ws);
  SPMV_REQUIRE(M >= 0 && (M == 0 || (X && AX && R)));
  SPMV_SET_DEVICE(ctx);
  const int nev = ws->nev;
  const bool nt = M * nev >= ctx->blas1_nt_min_elems;
  const bool vec = nev % 2 == 0 && aligned16(X, AX, R, W);
  hipStream_t st = spmv_stream(ctx, stream);
  SPMV_LOBPCG_LAUNCH_ROWS(lobpcg_residual_kernel, nev, nt, vec,
                          rows_grid(ctx, M), st, M, nev, ws->st, final ? 1 : 0,
                          ws->theta, X, AX, dinv, R, W, ws->rpart,
                          ctx->dot_blocks);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_lobpcg_update_gen_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                                   int64_t M, int blocks, double* X,
                                   const double* W, double* P, double* AX,
                                   const double* AW, double* AP, double* BX,
                                   const double* BW, double* BP, void* stream)
{
  SPMV_LOBPCG_REQUIRE(ctx, ws);
  SPMV_REQUIRE(M >= 0 && blocks_ok(blocks));
  SPMV_REQUIRE(M == 0 || (X && BX));
  SPMV_REQUIRE(M == 0 || blocks == 1 || (W && P && BW && BP));
  SPMV_REQUIRE(M == 0 || blocks == 1 || !AX || (AW && AP));
  SPMV_SET_DEVICE(ctx);
  const int nev = ws->nev;
  const bool nt = M * nev >= ctx->blas1_nt_min_elems;
  bool vec = nev % 2 == 0 && aligned16(X, AX, BX);
  if (blocks == 3)
    vec = vec && aligned16(W, P, AW, AP, BW, BP);
  hipStream_t st = spmv_stream(ctx, stream);
  const LobpcgTriples tr = {{X, AX, BX}, {W, AW, BW}, {P, AP, BP}};
  // y: the triple
  SPMV_LOBPCG_LAUNCH_ROWS(lobpcg_update_triple_kernel, nev, nt, vec,
                          dim3(rows_grid(ctx, M), 3), st, M, nev, blocks,
                          ws->st, ws->coef, tr);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

// (the residual kernel itself: BX stands where X stands without B)
int spmv_hip_lobpcg_residual_gen_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                                     int64_t M, const double* AX,
                                     const double* BX, const double* dinv,
                                     double* R, double* W, int final,
                                     void* stream)
{
  return spmv_hip_lobpcg_residual_f64(ctx, ws, M, BX, AX, dinv, R, W, final,
                                      stream);
}

int spmv_hip_lobpcg_norms(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws, int phase,
                          int final, void* stream)
{
  SPMV_LOBPCG_REQUIRE(ctx, ws);
  SPMV_REQUIRE(phase >= 0 && phase <= 2);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(lobpcg_norms_kernel, dim3(1), dim3(kBlock), 0,
                     spmv_stream(ctx, stream), ws->st, ws->nev, phase,
                     final ? 1 : 0, ws->rpart, ctx->dot_blocks, ws->rn,
                     ws->theta, ws->hist);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
