// Aggregation multigrid on the device (gfx950): the kernels of
// spmv::AmgPreconditioner beside the SpMVs and the Chebyshev steps it borrows.
//
// The host (host/amg_build.h) delivers one coarsening step: the aggregate of
// every fine row, the member rows of every aggregate (ascending), and for every
// entry of the coarse operator P^T A P the list of the fine entries it sums, as
// indices into the fine level's value array (>= 0) or its diagonal array (~src,
// symmetric storage).  On one stream and in its order alone:
//
//   amg_galerkin   coarse_values[E] = v_0 + v_1 + ... left to right over the list
//                  of E: one lane per coarse entry, so the bits do not depend on
//                  the launch shape
//   amg_diag       per row: d = the sum of the entries on the diagonal (storage
//                  order, from 0.0; symmetric storage: the diagonal array),
//                  dinv = 1.0 / d, g = (|a_0| + |a_1| + ...) * dinv over the
//                  expanded row; the workgroup's maximum of g into its word of
//                  `stat`, the number of d that are not finite or not > 0 into
//                  word 0 (an integer atomic per wavefront).  A maximum has no
//                  order: the host takes it over the words.
//   amg_restrict   rc[I] = (t_0 + t_1) + ..., t_m = r[i_m] - w[i_m] over the
//                  members of I ascending: one lane per aggregate
//   amg_prolong    z[i] = z[i] + scale * e[agg[i]]                     (streams z)
//   amg_post0      d = b0 * (dinv * (r - w)) ; z = z + d     (streams, step 0 of
//                  the post-smoother; steps >= 1 are cheb_step of blas1_cheb.hip)
//   amg_tail       the levels t .. last of one application in ONE launch of one
//                  workgroup of 1024 threads: the smoother, the products, the
//                  restricts, the coarsest level and the way back up, level
//                  after level from a descriptor table on the device.  The
//                  element arithmetic is amg_elem.h's, shared with the kernels
//                  above and blas1_cheb.hip; a level's product runs in the
//                  order of its plan (one lane per row left to right, or the
//                  sub-wavefront kernel's lanes and pairwise adds), so the bits
//                  are those of the separate launches.
//
// No kernel waits on another workgroup; no floating-point atomics.  Built with
// -ffp-contract=off: every product, sum, difference and quotient is a rounding
// of its own.  plan_create checks every index a kernel will use.
#include "common.h"
#include "blas1_stream.h"
#include "amg_elem.h"
#include "amg_tail_rules.h"

#include <new>
#include <vector>

#include "plan_scratch.h"
#include "amg_plan.h" // struct spmv_hip_amg_plan

namespace
{

constexpr int kStatBlocks = SPMV_HIP_AMG_STAT_WORDS - 1;

__device__ __forceinline__ double amg_value(int32_t q,
                                            const double* __restrict__ values,
                                            const double* __restrict__ diagonal)
{
  return q >= 0 ? values[q] : diagonal[~q];
}

__global__ __launch_bounds__(kBlock) void amg_galerkin_kernel(
    int64_t coarse_nnz, const int64_t* __restrict__ src_ptr,
    const int32_t* __restrict__ src, const double* __restrict__ values,
    const double* __restrict__ diagonal, double* __restrict__ coarse_values)
{
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t E = (int64_t)blockIdx.x * kBlock + threadIdx.x; E < coarse_nnz;
       E += stride) {
    const int64_t e0 = src_ptr[E], e1 = src_ptr[E + 1];
    double acc = 0.0; // (an empty list cannot occur: the pattern has a source)
    if (e0 < e1)
      acc = amg_value(src[e0], values, diagonal);
    for (int64_t e = e0 + 1; e < e1; ++e)
      acc = acc + amg_value(src[e], values, diagonal);
    coarse_values[E] = acc;
  }
}

// the tail of amg_diag's two forms: dinv, g, the counts
__device__ __forceinline__ void amg_diag_finish(bool active, int64_t i, double d,
                                                double asum, double* dvec,
                                                double* dinv, double* gmax,
                                                bool* bad)
{
  if (!active)
    return;
  const double di = 1.0 / d;
  dvec[i] = d;
  dinv[i] = di;
  const double g = asum * di;
  if (g > *gmax)
    *gmax = g;
  *bad = !(d - d == 0.0) || !(d > 0.0);
}

// SYM: the expanded rows come as source lists (xrow); else rowptr / colind,
// entries with a column >= ncols_local dropped
template <bool SYM>
__global__ __launch_bounds__(kBlock) void amg_diag_kernel(
    int32_t n, int32_t ncols_local, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ colind, const int64_t* __restrict__ xrow_ptr,
    const int32_t* __restrict__ xrow_src, const double* __restrict__ values,
    const double* __restrict__ diagonal, double* __restrict__ dvec,
    double* __restrict__ dinv, unsigned long long* stat)
{
  __shared__ double s_max[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  // (every lane of a wavefront makes the same number of rounds)
  const int64_t rounds = ((int64_t)n + stride - 1) / stride;
  double gmax = 0.0;
  for (int64_t rd = 0; rd < rounds; ++rd) {
    const int64_t i = rd * stride + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool active = i < n;
    double d = 0.0, asum = 0.0;
    bool first = true, bad = false;
    if (active) {
      if constexpr (SYM) {
        d = diagonal[i];
        for (int64_t e = xrow_ptr[i]; e < xrow_ptr[i + 1]; ++e) {
          const double a = fabs(amg_value(xrow_src[e], values, diagonal));
          asum = first ? a : asum + a;
          first = false;
        }
      } else {
        for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
          const int32_t c = colind[e];
          if (c >= ncols_local)
            continue;
          const double v = values[e];
          if (c == i)
            d = d + v;
          const double a = fabs(v);
          asum = first ? a : asum + a;
          first = false;
        }
      }
    }
    amg_diag_finish(active, i, d, asum, dvec, dinv, &gmax, &bad);
    const unsigned nbad = (unsigned)__popcll(__ballot(bad));
    if (lane == 0 && nbad)
      atomicAdd(stat, (unsigned long long)nbad);
  }
  // the workgroup's maximum: g >= 0, and a NaN never replaces a number
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(gmax, off, 64);
    if (o > gmax)
      gmax = o;
  }
  if (lane == 0)
    s_max[wave] = gmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = s_max[0];
    for (int k = 1; k < kBlock / 64; ++k)
      if (s_max[k] > m)
        m = s_max[k];
    stat[1 + blockIdx.x] = (unsigned long long)__double_as_longlong(m);
  }
}

__global__ __launch_bounds__(kBlock) void amg_restrict_kernel(
    int32_t coarse_rows, const int32_t* __restrict__ member_ptr,
    const int32_t* __restrict__ member, const double* __restrict__ r,
    const double* __restrict__ w, double* __restrict__ rc)
{
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t I = (int64_t)blockIdx.x * kBlock + threadIdx.x; I < coarse_rows;
       I += stride) {
    rc[I] = amg_restrict_sum(member_ptr[I], member_ptr[I + 1], member, r, w);
  }
}

// z streams; agg is read once, e is gathered (it is the smaller vector)
template <bool NT>
__global__ __launch_bounds__(kBlock) void amg_prolong_kernel(
    int64_t n, double scale, const int32_t* __restrict__ agg,
    const double* __restrict__ e, double* __restrict__ z)
{
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 zv[kU], ev[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      zv[u] = vload<NT>(z, i);
      ev[u].x = e[agg[2 * i]];
      ev[u].y = e[agg[2 * i + 1]];
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      zv[u].x = amg_prolong_elem(zv[u].x, scale, ev[u].x);
      zv[u].y = amg_prolong_elem(zv[u].y, scale, ev[u].y);
      vstore<NT>(z, i, zv[u]);
    }
  }
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    z[i] = amg_prolong_elem(z[i], scale, e[agg[i]]);
  }
}

// LAST: the post-smoother has one step, d is not written
template <bool NT, bool LAST>
__global__ __launch_bounds__(kBlock) void amg_post0_kernel(
    int64_t n, double b0, const double* __restrict__ w,
    const double* __restrict__ r, const double* __restrict__ dinv,
    double* __restrict__ d, double* __restrict__ z)
{
  const int64_t n2 = n >> 1;
  SPMV_FOR_UNITS(n2)
  {
    f64x2 wv[kU], rv[kU], dv[kU], zv[kU];
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      wv[u] = vload<NT>(w, i);
      rv[u] = vload<NT>(r, i);
      dv[u] = vload<NT>(dinv, i);
      zv[u] = vload<NT>(z, i);
    }
    SPMV_FOR_LANE_ELEMS(i, n2)
    {
      f64x2 t;
      t.x = cheb_corr<true>(b0, dv[u].x, rv[u].x, wv[u].x);
      t.y = cheb_corr<true>(b0, dv[u].y, rv[u].y, wv[u].y);
      if constexpr (!LAST)
        vstore<NT>(d, i, t);
      zv[u].x = zv[u].x + t.x;
      zv[u].y = zv[u].y + t.y;
      vstore<NT>(z, i, zv[u]);
    }
  }
  if (odd_tail(n)) {
    const int64_t i = n - 1;
    const double t = cheb_corr<true>(b0, dinv[i], r[i], w[i]);
    if constexpr (!LAST)
      d[i] = t;
    z[i] = z[i] + t;
  }
}

template <typename T>
int amg_upload(const T* host, size_t count, T** dev, int64_t* bytes)
{
  *dev = nullptr;
  if (count == 0)
    return SPMV_HIP_OK;
  SPMV_REQUIRE(host != nullptr);
  const hipError_t e = spmv_plan_malloc(dev, count * sizeof(T));
  if (e != hipSuccess)
    return plan_fail(e);
  *bytes += (int64_t)(count * sizeof(T));
  SPMV_CHECK_HIP(hipMemcpy(*dev, host, count * sizeof(T), hipMemcpyHostToDevice));
  return SPMV_HIP_OK;
}

bool src_is_sound(const spmv_hip_amg_host& in, int32_t q)
{
  return q >= 0 ? (int64_t)q < in.num_values : ~q < in.num_diagonal;
}

// Everything a kernel will index with is checked here, once, on the host.
bool amg_is_sound(const spmv_hip_amg_host& in)
{
  const int32_t n = in.fine_rows, nc = in.coarse_rows;
  if (n < 0 || nc < 0 || nc > n || in.num_values < 0 || in.num_diagonal < 0
      || in.coarse_nnz < 0)
    return false;
  if (in.num_diagonal != 0 && in.num_diagonal != n)
    return false;
  if (nc == 0) {
    if (in.coarse_nnz != 0)
      return false;
  } else {
    if (!in.agg || !in.member_ptr || !in.member || !in.src_ptr)
      return false;
    for (int32_t i = 0; i < n; ++i)
      if (in.agg[i] < 0 || in.agg[i] >= nc)
        return false;
    // the member lists: a partition of the rows, each ascending, each the
    // rows of its aggregate
    if (in.member_ptr[0] != 0 || in.member_ptr[nc] != n)
      return false;
    for (int32_t I = 0; I < nc; ++I) {
      const int32_t m0 = in.member_ptr[I], m1 = in.member_ptr[I + 1];
      if (m1 <= m0 || m0 < 0 || m1 > n)
        return false;
      for (int32_t m = m0; m < m1; ++m) {
        const int32_t i = in.member[m];
        if (i < 0 || i >= n || in.agg[i] != I)
          return false;
        if (m > m0 && i <= in.member[m - 1])
          return false;
      }
    }
    if (in.src_ptr[0] != 0)
      return false;
    for (int64_t E = 0; E < in.coarse_nnz; ++E)
      if (in.src_ptr[E + 1] <= in.src_ptr[E])
        return false;
    const int64_t count = in.src_ptr[in.coarse_nnz];
    if (count > 0 && !in.src)
      return false;
    for (int64_t e = 0; e < count; ++e)
      if (!src_is_sound(in, in.src[e]))
        return false;
  }
  if (in.xrow_ptr) {
    if (in.xrow_ptr[0] != 0)
      return false;
    for (int32_t i = 0; i < n; ++i)
      if (in.xrow_ptr[i + 1] < in.xrow_ptr[i])
        return false;
    const int64_t count = n > 0 ? in.xrow_ptr[n] : 0;
    if (count > 0 && !in.xrow_src)
      return false;
    for (int64_t e = 0; e < count; ++e)
      if (!src_is_sound(in, in.xrow_src[e]))
        return false;
  }
  return true;
}

// ---- the fused tail ---------------------------------------------------------------
// (AmgTailDev, the table entry the kernel reads, and its builder:
// amg_tail_rules.h)
constexpr int kTailBlock = kAmgTailBlock;

// w = A z in the order the level's plan runs; ends with the barrier
__device__ __forceinline__ void tail_product(const AmgTailDev* L)
{
  const int32_t n = L->rows;
  const int lanes = L->lanes;
  const int32_t* rowptr = L->rowptr;
  const int32_t* colind = L->colind;
  const double* values = L->values;
  const double* z = L->z;
  double* w = L->w;
  if (lanes == 0) { // one lane per row, left to right from 0.0
    for (int32_t i = threadIdx.x; i < n; i += kTailBlock) {
      double sum = 0.0;
      const int32_t hi = rowptr[i + 1];
      for (int32_t e = rowptr[i]; e < hi; ++e)
        sum += values[e] * z[colind[e]];
      w[i] = sum;
    }
  } else { // csr_vector_kernel's order (spmv_csr.hip)
    const int sub = threadIdx.x & (lanes - 1);
    const int32_t grp = threadIdx.x / lanes, rpb = kTailBlock / lanes;
    // (the same number of rounds for every thread: the shuffles are inside)
    const int32_t rounds = (n + rpb - 1) / rpb;
    for (int32_t rd = 0; rd < rounds; ++rd) {
      const int32_t i = rd * rpb + grp;
      double sum = 0.0;
      if (i < n) {
        const int32_t hi = rowptr[i + 1];
        for (int32_t e = rowptr[i] + sub; e < hi; e += lanes)
          sum += values[e] * z[colind[e]];
      }
      for (int off = lanes >> 1; off > 0; off >>= 1)
        sum += __shfl_down(sum, off, lanes);
      if (i < n && sub == 0)
        w[i] = sum;
    }
  }
  __syncthreads();
}

// the `degree`-step Chebyshev iteration for A z = r from z = 0
__device__ __forceinline__ void tail_chebyshev(const AmgTailDev* L, int degree)
{
  const int32_t n = L->rows;
  const double* r = L->r;
  const double* dinv = L->dinv;
  double* dd = L->dd;
  double* z = L->z;
  const double b0 = L->b[0];
  for (int32_t i = threadIdx.x; i < n; i += kTailBlock) {
    const double t = cheb_first<true>(b0, dinv[i], r[i]);
    if (degree > 1)
      dd[i] = t;
    z[i] = t;
  }
  __syncthreads();
  for (int j = 1; j < degree; ++j) {
    tail_product(L);
    const double a = L->a[j], b = L->b[j];
    const double* w = L->w;
    for (int32_t i = threadIdx.x; i < n; i += kTailBlock) {
      const double t = cheb_corr<true>(b, dinv[i], r[i], w[i]);
      const double e = cheb_next(a, dd[i], t);
      if (j < degree - 1)
        dd[i] = e;
      z[i] = z[i] + e;
    }
    __syncthreads();
  }
}

// Levels tab[0 .. nlev): down, the coarsest level, up.  ONE workgroup; the
// phases are separated by __syncthreads() alone, and every loop around a barrier
// or a shuffle has the same trip count in every thread.  In: tab[0].r.  Out:
// tab[0].z.
__global__ __launch_bounds__(kTailBlock) void amg_tail_kernel(
    const AmgTailDev* __restrict__ tab, int nlev, int s, int c, double scale)
{
  for (int l = 0; l < nlev; ++l) {
    const AmgTailDev* L = tab + l;
    if (l == nlev - 1) {
      tail_chebyshev(L, c);
      break;
    }
    tail_chebyshev(L, s);
    tail_product(L);
    const int32_t nc = L->coarse_rows;
    const int32_t* member_ptr = L->member_ptr;
    double* rc = tab[l + 1].r;
    for (int32_t I = threadIdx.x; I < nc; I += kTailBlock)
      rc[I] = amg_restrict_sum(member_ptr[I], member_ptr[I + 1], L->member, L->r,
                               L->w);
    __syncthreads();
  }
  for (int l = nlev - 2; l >= 0; --l) {
    const AmgTailDev* L = tab + l;
    const int32_t n = L->rows;
    const int32_t* agg = L->agg;
    const double* e = tab[l + 1].z;
    const double* r = L->r;
    const double* dinv = L->dinv;
    double* dd = L->dd;
    double* z = L->z;
    for (int32_t i = threadIdx.x; i < n; i += kTailBlock)
      z[i] = amg_prolong_elem(z[i], scale, e[agg[i]]);
    __syncthreads();
    for (int j = 0; j < s; ++j) {
      tail_product(L);
      const double a = L->a[j], b = L->b[j];
      const double* w = L->w;
      for (int32_t i = threadIdx.x; i < n; i += kTailBlock) {
        const double t = cheb_corr<true>(b, dinv[i], r[i], w[i]);
        const double d = j == 0 ? t : cheb_next(a, dd[i], t);
        if (j < s - 1)
          dd[i] = d;
        z[i] = z[i] + d;
      }
      __syncthreads();
    }
  }
}

} // namespace

struct spmv_hip_amg_tail {
  spmv_hip_ctx* ctx = nullptr;
  int nlev = 0, s = 0, c = 0;
  double scale = 1.0;
  std::vector<AmgTailDev> host; // the table as uploaded
  AmgTailDev* dev = nullptr;
  int64_t bytes = 0;
};

extern "C" {

int spmv_hip_amg_tail_create(spmv_hip_ctx* ctx, const spmv_hip_amg_tail_host* in,
                             spmv_hip_amg_tail** tail)
{
  SPMV_REQUIRE(ctx && in && tail);
  *tail = nullptr;
  const int nlev = in->num_levels;
  SPMV_REQUIRE(nlev >= 1 && nlev <= SPMV_HIP_AMG_TAIL_MAX_LEVELS && in->levels);
  SPMV_SET_DEVICE(ctx);
  spmv_hip_amg_tail* t = new (std::nothrow) spmv_hip_amg_tail();
  if (!t)
    return SPMV_HIP_ENOMEM;
  t->ctx = ctx;
  t->nlev = nlev;
  t->s = in->smooth_degree;
  t->c = in->coarse_degree;
  t->scale = in->coarse_scale;
  // Everything the kernel will index with is checked here, once: sizes,
  // vectors and steps by the device-free builder (amg_tail_fill_table; a
  // step's lists were checked by spmv_hip_amg_plan_create against the sizes it
  // records), then the CSR arrays, read back from the device.
  int rc = SPMV_HIP_OK;
  std::vector<int32_t> rowptr, colind;
  try {
    t->host.resize((size_t)nlev);
    std::vector<AmgTailStep> steps((size_t)nlev);
    for (int l = 0; l < nlev; ++l) {
      const spmv_hip_amg_plan* p = in->levels[l].step;
      AmgTailStep& st = steps[(size_t)l];
      st = AmgTailStep();
      if (p && p->ctx == ctx) {
        st.present = true;
        st.fine_rows = p->fine_rows;
        st.coarse_rows = p->coarse_rows;
        st.agg = p->agg;
        st.member_ptr = p->member_ptr;
        st.member = p->member;
      }
    }
    if (!amg_tail_fill_table(*in, steps.data(), t->host.data()))
      rc = SPMV_HIP_EINVAL;
    for (int l = 0; l < nlev && rc == SPMV_HIP_OK; ++l) {
      const spmv_hip_amg_tail_level& h = in->levels[l];
      rowptr.resize((size_t)h.rows + 1);
      colind.resize((size_t)h.nnz);
      hipError_t e = hipMemcpy(rowptr.data(), h.rowptr, rowptr.size() * 4,
                               hipMemcpyDeviceToHost);
      if (e == hipSuccess && h.nnz > 0)
        e = hipMemcpy(colind.data(), h.colind, colind.size() * 4,
                      hipMemcpyDeviceToHost);
      if (e != hipSuccess)
        rc = plan_fail(e);
      else if (!amg_tail_csr_is_sound(h.rows, h.rows, h.nnz, rowptr.data(),
                                      colind.data()))
        rc = SPMV_HIP_EINVAL;
    }
  } catch (const std::bad_alloc&) {
    rc = SPMV_HIP_ENOMEM;
  }
  if (rc == SPMV_HIP_OK) {
    const size_t bytes = (size_t)nlev * sizeof(AmgTailDev);
    hipError_t e = spmv_plan_malloc(&t->dev, bytes);
    if (e == hipSuccess) {
      t->bytes = (int64_t)bytes;
      e = hipMemcpy(t->dev, t->host.data(), bytes, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess)
      rc = plan_fail(e);
  }
  if (rc != SPMV_HIP_OK) {
    spmv_hip_amg_tail_destroy(t);
    return rc;
  }
  *tail = t;
  return SPMV_HIP_OK;
}

int spmv_hip_amg_tail_destroy(spmv_hip_amg_tail* tail)
{
  if (!tail)
    return SPMV_HIP_OK;
  (void)hipSetDevice(tail->ctx->device);
  plan_drop(tail->dev);
  delete tail;
  return SPMV_HIP_OK;
}

int spmv_hip_amg_tail_bytes(const spmv_hip_amg_tail* tail, int64_t* bytes)
{
  SPMV_REQUIRE(tail && bytes);
  *bytes = tail->bytes;
  return SPMV_HIP_OK;
}

int spmv_hip_amg_tail_set_coefficients(spmv_hip_amg_tail* tail, int level,
                                       const double* a, const double* b)
{
  SPMV_REQUIRE(tail && a && b && level >= 0 && level < tail->nlev);
  SPMV_SET_DEVICE(tail->ctx);
  const int degree = level == tail->nlev - 1 ? tail->c : tail->s;
  AmgTailDev& d = tail->host[(size_t)level];
  amg_tail_set_entry_coefficients(d, degree, a, b);
  // (a blocking copy: the table is complete when this returns)
  SPMV_CHECK_HIP(hipMemcpy(tail->dev + level, &d, sizeof d, hipMemcpyHostToDevice));
  return SPMV_HIP_OK;
}

int spmv_hip_amg_tail_run_f64(spmv_hip_ctx* ctx, const spmv_hip_amg_tail* tail,
                              void* stream)
{
  SPMV_REQUIRE(ctx && tail && tail->ctx == ctx && tail->dev);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(amg_tail_kernel, dim3(1), dim3(kTailBlock), 0,
                     spmv_stream(ctx, stream), tail->dev, tail->nlev, tail->s,
                     tail->c, tail->scale);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_amg_plan_create(spmv_hip_ctx* ctx, const spmv_hip_amg_host* in,
                             spmv_hip_amg_plan** plan)
{
  SPMV_REQUIRE(ctx && in && plan);
  *plan = nullptr;
  SPMV_REQUIRE(amg_is_sound(*in));
  spmv_hip_amg_plan* p = new (std::nothrow) spmv_hip_amg_plan();
  if (!p)
    return SPMV_HIP_ENOMEM;
  SPMV_SET_DEVICE(ctx);
  p->ctx = ctx;
  p->fine_rows = in->fine_rows;
  p->coarse_rows = in->coarse_rows;
  p->num_values = in->num_values;
  p->num_diagonal = in->num_diagonal;
  p->coarse_nnz = in->coarse_nnz;
  const size_t n = (size_t)in->fine_rows, nc = (size_t)in->coarse_rows;
  const bool step = nc > 0;
  p->src_count = step ? in->src_ptr[in->coarse_nnz] : 0;
  p->xrow_count = in->xrow_ptr && n > 0 ? in->xrow_ptr[n] : 0;
  int rc;
  if ((rc = amg_upload(in->agg, step ? n : 0, &p->agg, &p->bytes)) != SPMV_HIP_OK
      || (rc = amg_upload(in->member_ptr, step ? nc + 1 : 0, &p->member_ptr,
                          &p->bytes)) != SPMV_HIP_OK
      || (rc = amg_upload(in->member, step ? n : 0, &p->member, &p->bytes))
             != SPMV_HIP_OK
      || (rc = amg_upload(in->src_ptr, step ? (size_t)in->coarse_nnz + 1 : 0,
                          &p->src_ptr, &p->bytes)) != SPMV_HIP_OK
      || (rc = amg_upload(in->src, (size_t)p->src_count, &p->src, &p->bytes))
             != SPMV_HIP_OK
      || (rc = amg_upload(in->xrow_ptr, in->xrow_ptr ? n + 1 : 0, &p->xrow_ptr,
                          &p->bytes)) != SPMV_HIP_OK
      || (rc = amg_upload(in->xrow_src, (size_t)p->xrow_count, &p->xrow_src,
                          &p->bytes)) != SPMV_HIP_OK) {
    spmv_hip_amg_plan_destroy(p);
    return rc;
  }
  *plan = p;
  return SPMV_HIP_OK;
}

int spmv_hip_amg_plan_destroy(spmv_hip_amg_plan* plan)
{
  if (!plan)
    return SPMV_HIP_OK;
  (void)hipSetDevice(plan->ctx->device);
  plan_drop(plan->agg);
  plan_drop(plan->member_ptr);
  plan_drop(plan->member);
  plan_drop(plan->src_ptr);
  plan_drop(plan->src);
  plan_drop(plan->xrow_ptr);
  plan_drop(plan->xrow_src);
  delete plan;
  return SPMV_HIP_OK;
}

int spmv_hip_amg_plan_bytes(const spmv_hip_amg_plan* plan, int64_t* bytes)
{
  SPMV_REQUIRE(plan && bytes);
  *bytes = plan->bytes;
  return SPMV_HIP_OK;
}

int spmv_hip_amg_galerkin_f64(spmv_hip_ctx* ctx, const spmv_hip_amg_plan* plan,
                              const double* values, const double* diagonal,
                              double* coarse_values, void* stream)
{
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx);
  SPMV_REQUIRE(plan->num_values == 0 || values);
  SPMV_REQUIRE(plan->num_diagonal == 0 || diagonal);
  SPMV_REQUIRE(plan->coarse_nnz == 0 || coarse_values);
  SPMV_SET_DEVICE(ctx);
  if (plan->coarse_nnz == 0)
    return SPMV_HIP_OK;
  hipLaunchKernelGGL(amg_galerkin_kernel,
                     dim3(spmv_grid_for(ctx, plan->coarse_nnz, kBlock)),
                     dim3(kBlock), 0, spmv_stream(ctx, stream), plan->coarse_nnz,
                     plan->src_ptr, plan->src, values, diagonal, coarse_values);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_amg_diag_f64(spmv_hip_ctx* ctx, const spmv_hip_amg_plan* plan,
                          int32_t n, int32_t ncols_local, const int32_t* rowptr,
                          const int32_t* colind, const double* values,
                          const double* diagonal, double* d, double* dinv,
                          uint64_t* stat, void* stream)
{
  SPMV_REQUIRE(ctx && n >= 0 && stat && (n == 0 || (d && dinv)));
  const bool sym = plan && plan->xrow_ptr;
  if (sym)
    SPMV_REQUIRE(plan->ctx == ctx && plan->fine_rows == n && diagonal
                 && plan->num_diagonal == n
                 && (plan->num_values == 0 || values));
  else
    SPMV_REQUIRE(n == 0 || (rowptr && colind && values));
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  SPMV_CHECK_HIP(hipMemsetAsync(stat, 0, SPMV_HIP_AMG_STAT_WORDS * 8, st));
  if (n == 0)
    return SPMV_HIP_OK;
  int grid = spmv_grid_for(ctx, n, kBlock);
  if (grid > kStatBlocks)
    grid = kStatBlocks;
  unsigned long long* words = reinterpret_cast<unsigned long long*>(stat);
  if (sym)
    hipLaunchKernelGGL((amg_diag_kernel<true>), dim3(grid), dim3(kBlock), 0, st, n,
                       n, nullptr, nullptr, plan->xrow_ptr, plan->xrow_src, values,
                       diagonal, d, dinv, words);
  else
    hipLaunchKernelGGL((amg_diag_kernel<false>), dim3(grid), dim3(kBlock), 0, st,
                       n, ncols_local, rowptr, colind, nullptr, nullptr, values,
                       nullptr, d, dinv, words);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_amg_restrict_f64(spmv_hip_ctx* ctx, const spmv_hip_amg_plan* plan,
                              const double* r, const double* w, double* rc,
                              void* stream)
{
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx && plan->coarse_rows > 0);
  SPMV_REQUIRE(r && w && rc);
  SPMV_SET_DEVICE(ctx);
  hipLaunchKernelGGL(amg_restrict_kernel,
                     dim3(spmv_grid_for(ctx, plan->coarse_rows, kBlock)),
                     dim3(kBlock), 0, spmv_stream(ctx, stream), plan->coarse_rows,
                     plan->member_ptr, plan->member, r, w, rc);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_amg_prolong_f64(spmv_hip_ctx* ctx, const spmv_hip_amg_plan* plan,
                             double scale, const double* e, double* z,
                             void* stream)
{
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx && plan->coarse_rows > 0);
  SPMV_REQUIRE(e && z && aligned16(z));
  SPMV_SET_DEVICE(ctx);
  const int64_t n = plan->fine_rows;
  SPMV_LAUNCH_NT(ctx, n, amg_prolong_kernel, stream_grid(ctx, n),
                 spmv_stream(ctx, stream), n, scale, plan->agg, e, z);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_amg_post0_f64(spmv_hip_ctx* ctx, int64_t n, double b0,
                           const double* w, const double* r, const double* dinv,
                           double* d, double* z, void* stream)
{
  SPMV_REQUIRE(ctx && n >= 0 && (n == 0 || (w && r && dinv && z)));
  SPMV_REQUIRE(aligned16(w, r, dinv, d, z));
  SPMV_SET_DEVICE(ctx);
  const int grid = stream_grid(ctx, n);
  hipStream_t st = spmv_stream(ctx, stream);
  const bool nt = n >= ctx->blas1_nt_min_elems;
  const dim3 g(grid), blk(kBlock);
  if (nt && d)
    hipLaunchKernelGGL((amg_post0_kernel<true, false>), g, blk, 0, st, n, b0, w, r,
                       dinv, d, z);
  else if (nt)
    hipLaunchKernelGGL((amg_post0_kernel<true, true>), g, blk, 0, st, n, b0, w, r,
                       dinv, d, z);
  else if (d)
    hipLaunchKernelGGL((amg_post0_kernel<false, false>), g, blk, 0, st, n, b0, w,
                       r, dinv, d, z);
  else
    hipLaunchKernelGGL((amg_post0_kernel<false, true>), g, blk, 0, st, n, b0, w, r,
                       dinv, d, z);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"
