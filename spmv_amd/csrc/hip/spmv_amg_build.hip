// The symbolic setup of spmv::AmgPreconditioner on the device (gfx950): the
// aggregates of a level and the plan of its coarsening step, both from the CSR
// arrays where they lie.  No entry of the matrix, pattern or value, travels to
// the host: only counters (rounds, n_agg, the number of coarse entries).
//
// EXPANDED ROW (host/amg_build.h's amg_expand, walked on the fly, XRows::each).
// General storage: the stored entries with a column < n in storage order.
// Symmetric storage: the stored entries with a column < i, the diagonal entry
// (source ~i), then the mirror images of the stored entries of column i,
// ascending by row, through the transposed map (spmv_tmap_build: a stable sort
// by column).
//
// AGGREGATES (spmv_hip_amg_aggregate).  Strength is amg_build.cpp's, evaluated
// per entry: m_i the running maximum of |a_e| over the entries with a column
// != i, from 0.0 (a NaN never replaces a number), bar = theta * m_i, an entry
// is strong iff a_e != 0.0 and |a_e| >= bar.  bar is computed once per row (8
// bytes a row); no strong list is stored.  The
// three passes of amg_build.h with "i ascending" read as "i in descending
// priority": natural, prio(i) = n - i (amg_aggregate entry for entry), and
// hashed, prio(i) = mix64((i + 1) * G mod 2^64) unsigned (mcgs_color's).
//   pass 1  N[i] = {i} + strong(i).  i is a root iff no root k of higher
//           priority has a vertex in common with N[i]; every vertex of a root's
//           N is its member.  A round, two launches:
//             bid   an undecided row that sees a marked vertex in its N becomes
//                   a non-root; otherwise it bids its priority (atomicMax) on
//                   every vertex of its N
//             take  an undecided row that holds the maximum on all of its N
//                   becomes a root and marks N with its number
//   pass 2  one launch on the marks of pass 1: an unmarked row joins the root
//           of the first strong entry, in expanded order, whose column is marked
//   pass 3  among the rows still free: i is a root iff no root k of higher
//           priority has i in strong(k); a free non-root joins the root of
//           highest priority that points to it.  A round, two launches:
//             push  an undecided row bids on the free rows it points to; a row
//                   that became a root in the last round claims them (atomicMax
//                   into an array of its own, never reset)
//             take  an undecided row with a claim above its priority becomes a
//                   member; one with no bid above its priority a root
//           and at the end every root takes the members whose claim is its own.
//   numbering   the roots of pass 1 ascending by row, then those of pass 3
// The bids are memset before every round.  The order between launches is the
// stream's and nothing else: no kernel waits on another workgroup, nothing
// spins; a launch reads nothing that the same launch writes, except the bids
// and claims, which are integer maxima of priorities no two rows share.  So
// the aggregates AND the number of rounds depend on the matrix and the order
// alone.  The undecided row of highest priority decides in every round: n + 1
// rounds of a pass suffice and more are SPMV_HIP_ERANGE, not a hang.  The host
// reads the "rows left" counters of kBatch rounds at a time.
//
// PLAN (spmv_hip_amg_plan_build).  From an aggregate per row, every array of
// spmv_hip_amg_plan as amg_galerkin_pattern + spmv_hip_amg_plan_create make it:
//   1 check, on the device, before anything is indexed: rowptr, columns, agg
//   2 member: the rows stably sorted by agg (radix sort); member_ptr from the
//     sorted aggregates; every aggregate has a member
//   3 the lengths of the expanded rows, their scan (symmetric storage: the
//     plan's xrow_ptr)
//   4 every expanded entry, in expanded order, as the key (agg(i), agg(j)) of
//     2 * bits_for(n_agg) bits with its source as payload (symmetric storage:
//     the payloads are the plan's xrow_src); ONE stable radix sort: the sources
//     of a coarse entry by member row, then in expanded order
//   5 the heads of the runs of equal keys, scanned: src_ptr, the coarse colind
//     and, from the rows of the heads, the coarse rowptr
// Temporaries are PlanScratch arrays on the books, gone at return; a failure
// frees everything.
#include "common.h"

#include <hipcub/hipcub.hpp>

#include <new>

#include "amg_plan.h"
#include "csr_plan.h"
#include "plan_build.h"
#include "plan_scratch.h"

namespace
{

using bid_t = unsigned long long;

// the rows of a level, expanded on the fly
struct XRows {
  int32_t n;
  const int32_t* rowptr;
  const int32_t* colind;
  const int32_t *t_ptr, *t_pos, *t_row; // symmetric storage with entries
  int symmetric;

  // f(column, source) for every entry of row i in expanded order, until f
  // returns false
  template <typename F>
  __device__ __forceinline__ void each(int32_t i, F&& f) const
  {
    for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int32_t c = colind[e];
      if (symmetric ? c >= i : c >= n)
        continue;
      if (!f(c, e))
        return;
    }
    if (!symmetric)
      return;
    if (!f(i, ~i))
      return;
    if (t_ptr)
      for (int32_t k = t_ptr[i]; k < t_ptr[i + 1]; ++k) {
        const int32_t j = t_row[k];
        if (j <= i)
          continue;
        if (!f(j, t_pos[k]))
          return;
      }
  }
};

__device__ __forceinline__ bid_t prio_of(int32_t i, int32_t n, int order)
{
  return order == kNatural ? (bid_t)(n - i) : (bid_t)row_hash(i);
}

// theta * m_i.  (An entry with a column != i has a source >= 0: it is a value.)
__device__ __forceinline__ double bar_of(const XRows& x,
                                         const double* __restrict__ values,
                                         int32_t i, double theta)
{
  double m = 0.0;
  x.each(i, [&](int32_t c, int32_t s) {
    if (c != i) {
      const double a = fabs(values[s]);
      if (a > m)
        m = a;
    }
    return true;
  });
  return theta * m;
}

__device__ __forceinline__ bool is_strong(double a, double bar)
{
  return a != 0.0 && fabs(a) >= bar;
}

// one add per wavefront of the rows a round leaves undecided
__device__ __forceinline__ void add_left(int32_t my_left, int32_t* left)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    my_left += __shfl_down(my_left, off, 64);
  if ((threadIdx.x & 63) == 0 && my_left)
    atomicAdd(left, my_left);
}

// state of a row in pass 1
constexpr int32_t kOpen = 0, kRoot = 1, kNonRoot = 2;
// ... and in pass 3
constexpr int32_t kTaken = 0, kFree = 1, kNewRoot = 2, kRoot3 = 3, kMember = 4;

// theta * m_i of every row, once: the rounds read it instead of walking the row
__global__ __launch_bounds__(kBlock) void amg_bar_kernel(
    XRows x, const double* __restrict__ values, double theta,
    double* __restrict__ bars)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < x.n;
       i += (int64_t)gridDim.x * blockDim.x)
    bars[i] = bar_of(x, values, (int32_t)i, theta);
}

// pass 1, bid.  own[v] >= 0: v is marked by the root own[v].
__global__ __launch_bounds__(kBlock) void amg_p1_bid_kernel(
    XRows x, const double* __restrict__ values,
    const double* __restrict__ bars, int order,
    int32_t* __restrict__ st, const int32_t* __restrict__ own, bid_t* bid)
{
  for (int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < x.n;
       i64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)i64;
    if (st[i] != kOpen)
      continue;
    const double bar = bars[i];
    bool marked = own[i] >= 0;
    if (!marked)
      x.each(i, [&](int32_t c, int32_t s) {
        if (c != i && is_strong(values[s], bar) && own[c] >= 0)
          marked = true;
        return !marked;
      });
    if (marked) {
      st[i] = kNonRoot;
      continue;
    }
    const bid_t p = prio_of(i, x.n, order);
    atomicMax(bid + i, p);
    x.each(i, [&](int32_t c, int32_t s) {
      if (c != i && is_strong(values[s], bar))
        atomicMax(bid + c, p);
      return true;
    });
  }
}

// pass 1, take.  (No row reads own here; two roots of one launch share no
// vertex: both would hold its maximum.)
__global__ __launch_bounds__(kBlock) void amg_p1_take_kernel(
    XRows x, const double* __restrict__ values,
    const double* __restrict__ bars, int order,
    int32_t* __restrict__ st, int32_t* __restrict__ own,
    const bid_t* __restrict__ bid, int32_t* __restrict__ left)
{
  int32_t my_left = 0;
  for (int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < x.n;
       i64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)i64;
    if (st[i] != kOpen)
      continue;
    const bid_t p = prio_of(i, x.n, order);
    bool all = bid[i] == p;
    double bar = 0.0;
    if (all) {
      bar = bars[i];
      x.each(i, [&](int32_t c, int32_t s) {
        if (c != i && is_strong(values[s], bar) && bid[c] != p)
          all = false;
        return all;
      });
    }
    if (!all) {
      ++my_left;
      continue;
    }
    st[i] = kRoot;
    own[i] = i;
    x.each(i, [&](int32_t c, int32_t s) {
      if (c != i && is_strong(values[s], bar))
        own[c] = i;
      return true;
    });
  }
  add_left(my_left, left);
}

// pass 2: own2[i] = the root an unmarked row joins (-1: none, or marked); st =
// the state pass 3 starts from
__global__ __launch_bounds__(kBlock) void amg_p2_kernel(
    XRows x, const double* __restrict__ values,
    const double* __restrict__ bars,
    const int32_t* __restrict__ own, int32_t* __restrict__ own2,
    int32_t* __restrict__ st)
{
  for (int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < x.n;
       i64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)i64;
    int32_t o = -1;
    if (own[i] < 0) {
      const double bar = bars[i];
      x.each(i, [&](int32_t c, int32_t s) {
        if (c != i && is_strong(values[s], bar) && own[c] >= 0)
          o = own[c];
        return o < 0;
      });
    }
    own2[i] = o;
    st[i] = own[i] < 0 && o < 0 ? kFree : kTaken;
  }
}

// pass 3, push.  (st of another row is only compared with kTaken, which no
// launch of this pass writes or removes.)
__global__ __launch_bounds__(kBlock) void amg_p3_push_kernel(
    XRows x, const double* __restrict__ values,
    const double* __restrict__ bars, int order,
    int32_t* st, bid_t* bid, bid_t* claim)
{
  for (int64_t k64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k64 < x.n;
       k64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t k = (int32_t)k64;
    const int32_t s = st[k];
    if (s != kFree && s != kNewRoot)
      continue;
    const double bar = bars[k];
    const bid_t p = prio_of(k, x.n, order);
    bid_t* to = s == kFree ? bid : claim;
    x.each(k, [&](int32_t c, int32_t q) {
      if (c != k && is_strong(values[q], bar)
          && __hip_atomic_load(st + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                 != kTaken)
        atomicMax(to + c, p);
      return true;
    });
    if (s == kNewRoot)
      __hip_atomic_store(st + k, kRoot3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// pass 3, take
__global__ __launch_bounds__(kBlock) void amg_p3_take_kernel(
    int32_t n, int order, int32_t* __restrict__ st, const bid_t* __restrict__ bid,
    const bid_t* __restrict__ claim, int32_t* __restrict__ left)
{
  int32_t my_left = 0;
  for (int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < n;
       i64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)i64;
    if (st[i] != kFree)
      continue;
    const bid_t p = prio_of(i, n, order);
    if (claim[i] > p)
      st[i] = kMember;
    else if (bid[i] < p)
      st[i] = kNewRoot;
    else
      ++my_left;
  }
  add_left(my_left, left);
}

// pass 3, the end: every claim has been pushed; a root takes itself and the
// members whose highest claim is its own
__global__ __launch_bounds__(kBlock) void amg_p3_owner_kernel(
    XRows x, const double* __restrict__ values,
    const double* __restrict__ bars, int order,
    const int32_t* __restrict__ st, const bid_t* __restrict__ claim,
    int32_t* __restrict__ own2)
{
  for (int64_t k64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k64 < x.n;
       k64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t k = (int32_t)k64;
    if (st[k] != kRoot3)
      continue;
    const double bar = bars[k];
    const bid_t p = prio_of(k, x.n, order);
    own2[k] = k;
    x.each(k, [&](int32_t c, int32_t q) {
      if (c != k && is_strong(values[q], bar) && st[c] == kMember && claim[c] == p)
        own2[c] = k;
      return true;
    });
  }
}

// the addends of the two numberings
__global__ __launch_bounds__(kBlock) void amg_root_flags_kernel(
    int32_t n, const int32_t* __restrict__ own, const int32_t* __restrict__ st,
    int64_t* __restrict__ num1, int64_t* __restrict__ num3)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    num1[i] = own[i] == i ? 1 : 0;
    num3[i] = st[i] == kRoot3 ? 1 : 0;
  }
}

// agg from the roots' numbers (num1[n]: the roots of pass 1)
__global__ __launch_bounds__(kBlock) void amg_number_kernel(
    int32_t n, const int32_t* __restrict__ own, const int32_t* __restrict__ own2,
    const int32_t* __restrict__ st, const int64_t* __restrict__ num1,
    const int64_t* __restrict__ num3, int32_t* __restrict__ agg)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t o = own[i];
    int64_t a;
    if (o >= 0)
      a = num1[o];
    else if (st[i] == kTaken)
      a = num1[own2[i]];
    else
      a = num1[n] + num3[own2[i]];
    agg[i] = (int32_t)a;
  }
}

// ---- the plan's kernels ------------------------------------------------------
// member_ptr[I] = the first position whose aggregate is >= I, from the sorted
// aggregates (all in [0, n_agg)); position n closes the table
__global__ __launch_bounds__(kBlock) void amg_member_ptr_kernel(
    int32_t n, int32_t n_agg, const int32_t* __restrict__ sorted,
    int32_t* __restrict__ member_ptr)
{
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= n;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t prev = p == 0 ? -1 : sorted[p - 1];
    const int32_t cur = p == n ? n_agg : sorted[p];
    for (int32_t c = prev + 1; c <= cur; ++c)
      member_ptr[c] = (int32_t)p;
  }
}

__global__ __launch_bounds__(kBlock) void amg_empty_kernel(
    int32_t n_agg, const int32_t* __restrict__ member_ptr,
    int32_t* __restrict__ flag)
{
  for (int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < n_agg;
       a += (int64_t)gridDim.x * blockDim.x)
    if (member_ptr[a + 1] <= member_ptr[a])
      atomicOr(flag, 1);
}

__global__ __launch_bounds__(kBlock) void amg_xlen_kernel(XRows x,
                                                          int64_t* __restrict__ len)
{
  for (int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < x.n;
       i64 += (int64_t)gridDim.x * blockDim.x) {
    int64_t m = 0;
    x.each((int32_t)i64, [&](int32_t, int32_t) {
      ++m;
      return true;
    });
    len[i64] = m;
  }
}

// Per row: the sources of its expanded entries at xptr[i] on, and (keys != NULL)
// their keys (agg(i), agg(j))
__global__ __launch_bounds__(kBlock) void amg_expand_kernel(
    XRows x, const int64_t* __restrict__ xptr, const int32_t* __restrict__ agg,
    int bits, uint64_t* __restrict__ keys, int32_t* __restrict__ src)
{
  for (int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < x.n;
       i64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)i64;
    int64_t q = xptr[i];
    const uint64_t hi = keys ? (uint64_t)agg[i] << bits : 0;
    x.each(i, [&](int32_t c, int32_t s) {
      if (keys)
        keys[q] = hi | (uint64_t)agg[c];
      src[q++] = s;
      return true;
    });
  }
}

__global__ __launch_bounds__(kBlock) void amg_heads_kernel(
    int64_t count, const uint64_t* __restrict__ keys, int64_t* __restrict__ head)
{
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < count;
       q += (int64_t)gridDim.x * blockDim.x)
    head[q] = q == 0 || keys[q] != keys[q - 1] ? 1 : 0;
}

// index[q]: the heads in front of q.  A head is the first source of its coarse
// entry.
__global__ __launch_bounds__(kBlock) void amg_entries_kernel(
    int64_t count, const uint64_t* __restrict__ keys,
    const int64_t* __restrict__ index, int bits, int64_t coarse_nnz,
    int64_t* __restrict__ src_ptr, int32_t* __restrict__ colind,
    int32_t* __restrict__ crow)
{
  const uint64_t low = ((uint64_t)1 << bits) - 1;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < count;
       q += (int64_t)gridDim.x * blockDim.x) {
    if (q == 0)
      src_ptr[coarse_nnz] = count;
    if (q != 0 && keys[q] == keys[q - 1])
      continue;
    const int64_t e = index[q];
    src_ptr[e] = q;
    colind[e] = (int32_t)(keys[q] & low);
    crow[e] = (int32_t)(keys[q] >> bits);
  }
}

// rowptr[I] = the first coarse entry whose row is >= I
__global__ __launch_bounds__(kBlock) void amg_rowptr_kernel(
    int64_t coarse_nnz, int32_t n_agg, const int32_t* __restrict__ crow,
    int32_t* __restrict__ rowptr)
{
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= coarse_nnz;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t prev = e == 0 ? -1 : crow[e - 1];
    const int32_t cur = e == coarse_nnz ? n_agg : crow[e];
    for (int32_t c = prev + 1; c <= cur; ++c)
      rowptr[c] = (int32_t)e;
  }
}

// ---- host side ---------------------------------------------------------------
struct AmgPlanDeleter {
  spmv_hip_amg_plan* p = nullptr;
  ~AmgPlanDeleter() { spmv_hip_amg_plan_destroy(p); }
  spmv_hip_amg_plan* release()
  {
    spmv_hip_amg_plan* q = p;
    p = nullptr;
    return q;
  }
};

// Rounds until one leaves no row undecided: kBatch rounds a read.  round(left)
// enqueues one round whose counter is `left`.
template <typename Round>
int run_rounds(int32_t n, int32_t* counters, hipStream_t st, Round&& round,
               int* rounds)
{
  int32_t host[kBatch];
  int done_rounds = 0;
  bool done = false;
  while (!done) {
    // n + 1 rounds decide any matrix: more is a fault of this code
    if ((int64_t)done_rounds >= (int64_t)n + 1)
      return SPMV_HIP_ERANGE;
    MB_HIP(hipMemsetAsync(counters, 0, sizeof(int32_t) * kBatch, st));
    for (int b = 0; b < kBatch; ++b)
      MB_HIP(round(counters + b));
    MB_HIP(plan_fetch(host, counters, kBatch, st));
    for (int b = 0; b < kBatch && !done; ++b) {
      ++done_rounds;
      done = host[b] == 0;
    }
  }
  *rounds = done_rounds;
  return SPMV_HIP_OK;
}

int reason_of(int32_t flags)
{
  return (flags & 1)   ? SPMV_HIP_AMG_BAD_ROWPTR
         : (flags & 2) ? SPMV_HIP_AMG_BAD_COLUMN
                       : SPMV_HIP_AMG_BAD_AGG;
}

void clear_info(int64_t* info)
{
  for (int k = 0; k < SPMV_HIP_AMG_INFO_WORDS; ++k)
    info[k] = 0;
}

} // namespace

extern "C" {

int spmv_hip_amg_aggregate(spmv_hip_ctx* ctx, int32_t num_rows, int32_t num_cols,
                           int64_t nnz, const int32_t* rowptr,
                           const int32_t* colind, const double* values,
                           const double* diagonal, int symmetric, double theta,
                           int order, int32_t* agg, int32_t* n_agg, int* rounds,
                           int64_t* info, void* stream)
{
  SPMV_REQUIRE(ctx && n_agg && rounds && info);
  *n_agg = 0;
  rounds[0] = rounds[1] = 0;
  clear_info(info);
  SPMV_REQUIRE(args_ok(num_rows, num_cols, nnz, rowptr, colind));
  SPMV_REQUIRE(nnz == 0 || values);
  SPMV_REQUIRE(order == 0 || order == kNatural);
  SPMV_REQUIRE(theta >= 0.0 && theta <= 1.0);
  SPMV_REQUIRE(num_rows == 0 || agg);
  (void)diagonal; // (the diagonal entry is no neighbour: it is never read)
  if (num_rows == 0)
    return SPMV_HIP_OK;
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  const int32_t n = num_rows;
  const int sym = symmetric ? 1 : 0;
  TempBytes book;
  Temp<int32_t> zeros;
  if (!rowptr)
    MB_HIP(zero_rowptr(zeros, n, &book, st, &rowptr));
  int32_t flags = 0;
  int rc = check_input(ctx, n, num_cols, nnz, rowptr, colind, nullptr, 0, &book,
                       st, &flags);
  if (rc != SPMV_HIP_OK)
    return rc;
  if (flags) {
    info[0] = reason_of(flags);
    return SPMV_HIP_EINVAL;
  }
  TMap t;
  if (sym && (rc = build_tmap(ctx, n, num_cols, nnz, rowptr, colind, &book, st, &t))
                 != SPMV_HIP_OK)
    return rc;
  const XRows x{n, rowptr, colind, t.ptr, t.pos, t.row, sym};

  Temp<int32_t> state, own, own2, counters;
  Temp<bid_t> bid, claim;
  Temp<double> bars;
  MB_HIP(bars.alloc((size_t)n, &book));
  MB_HIP(state.alloc((size_t)n, &book));
  MB_HIP(own.alloc((size_t)n, &book));
  MB_HIP(own2.alloc((size_t)n, &book));
  MB_HIP(counters.alloc(kBatch, &book));
  MB_HIP(bid.alloc((size_t)n, &book));
  MB_HIP(claim.alloc((size_t)n, &book));
  MB_HIP(hipMemsetAsync(state.get(), 0, sizeof(int32_t) * (size_t)n, st));
  MB_HIP(hipMemsetAsync(own.get(), 0xff, sizeof(int32_t) * (size_t)n, st));
  MB_HIP(hipMemsetAsync(claim.get(), 0, sizeof(bid_t) * (size_t)n, st));
  const dim3 grid(spmv_grid_for(ctx, n, kBlock)), block(kBlock);
  hipLaunchKernelGGL(amg_bar_kernel, grid, block, 0, st, x, values, theta,
                     bars.get());
  MB_HIP(hipGetLastError());

  // pass 1
  rc = run_rounds(
      n, counters.get(), st,
      [&](int32_t* left) {
        hipError_t e = hipMemsetAsync(bid.get(), 0, sizeof(bid_t) * (size_t)n, st);
        if (e != hipSuccess)
          return e;
        hipLaunchKernelGGL(amg_p1_bid_kernel, grid, block, 0, st, x, values,
                           bars.get(), order, state.get(), own.get(), bid.get());
        hipLaunchKernelGGL(amg_p1_take_kernel, grid, block, 0, st, x, values,
                           bars.get(), order, state.get(), own.get(), bid.get(), left);
        return hipGetLastError();
      },
      &rounds[0]);
  if (rc != SPMV_HIP_OK)
    return rc;

  // pass 2
  hipLaunchKernelGGL(amg_p2_kernel, grid, block, 0, st, x, values, bars.get(), own.get(),
                     own2.get(), state.get());
  MB_HIP(hipGetLastError());

  // pass 3
  rc = run_rounds(
      n, counters.get(), st,
      [&](int32_t* left) {
        hipError_t e = hipMemsetAsync(bid.get(), 0, sizeof(bid_t) * (size_t)n, st);
        if (e != hipSuccess)
          return e;
        hipLaunchKernelGGL(amg_p3_push_kernel, grid, block, 0, st, x, values,
                           bars.get(), order, state.get(), bid.get(), claim.get());
        hipLaunchKernelGGL(amg_p3_take_kernel, grid, block, 0, st, n, order,
                           state.get(), bid.get(), claim.get(), left);
        return hipGetLastError();
      },
      &rounds[1]);
  if (rc != SPMV_HIP_OK)
    return rc;
  // (the roots of the last round have not claimed yet)
  hipLaunchKernelGGL(amg_p3_push_kernel, grid, block, 0, st, x, values, bars.get(),
                     order, state.get(), bid.get(), claim.get());
  hipLaunchKernelGGL(amg_p3_owner_kernel, grid, block, 0, st, x, values, bars.get(),
                     order, state.get(), claim.get(), own2.get());
  MB_HIP(hipGetLastError());

  // the numbering
  Temp<int64_t> num1, num3;
  MB_HIP(num1.alloc((size_t)n + 1, &book));
  MB_HIP(num3.alloc((size_t)n + 1, &book));
  hipLaunchKernelGGL(amg_root_flags_kernel, grid, block, 0, st, n, own.get(),
                     state.get(), num1.get(), num3.get());
  MB_HIP(hipGetLastError());
  MB_HIP(scan_in_place(num1.get(), n, st));
  MB_HIP(scan_in_place(num3.get(), n, st));
  hipLaunchKernelGGL(amg_number_kernel, grid, block, 0, st, n, own.get(),
                     own2.get(), state.get(), num1.get(), num3.get(), agg);
  MB_HIP(hipGetLastError());
  int64_t roots[2] = {0, 0};
  MB_HIP(plan_fetch(&roots[0], num1.get() + n, 1, st));
  MB_HIP(plan_fetch(&roots[1], num3.get() + n, 1, st));
  *n_agg = (int32_t)(roots[0] + roots[1]);
  info[1] = book.peak;
  return SPMV_HIP_OK;
}

int spmv_hip_amg_plan_build(spmv_hip_ctx* ctx, int32_t num_rows, int32_t num_cols,
                            int64_t nnz, const int32_t* rowptr,
                            const int32_t* colind, int symmetric,
                            const int32_t* agg, int32_t n_agg,
                            int32_t* coarse_rowptr, int32_t** coarse_colind,
                            int64_t* coarse_nnz, spmv_hip_amg_plan** plan,
                            int64_t* info, void* stream)
{
  SPMV_REQUIRE(ctx && plan && info && coarse_colind && coarse_nnz);
  *plan = nullptr;
  *coarse_colind = nullptr;
  *coarse_nnz = 0;
  clear_info(info);
  SPMV_REQUIRE(args_ok(num_rows, num_cols, nnz, rowptr, colind));
  SPMV_REQUIRE(n_agg >= 0 && n_agg <= num_rows);
  SPMV_REQUIRE(n_agg == 0 || (agg && coarse_rowptr));
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  const int32_t n = num_rows;
  const int sym = symmetric ? 1 : 0;
  const bool step = n_agg > 0;
  TempBytes book;
  AmgPlanDeleter guard;
  guard.p = new (std::nothrow) spmv_hip_amg_plan();
  if (!guard.p)
    return SPMV_HIP_ENOMEM;
  spmv_hip_amg_plan* p = guard.p;
  p->ctx = ctx;
  p->fine_rows = n;
  p->coarse_rows = n_agg;
  p->num_values = nnz;
  p->num_diagonal = sym ? n : 0;
  if (n == 0) {
    *plan = guard.release();
    return SPMV_HIP_OK;
  }

  // 1 the checks
  Temp<int32_t> zeros;
  if (!rowptr)
    MB_HIP(zero_rowptr(zeros, n, &book, st, &rowptr));
  int32_t flags = 0;
  int rc = check_input(ctx, n, num_cols, nnz, rowptr, colind, step ? agg : nullptr,
                       n_agg, &book, st, &flags);
  if (rc != SPMV_HIP_OK)
    return rc;
  if (flags) {
    info[0] = reason_of(flags);
    return SPMV_HIP_EINVAL;
  }
  const dim3 grid(spmv_grid_for(ctx, n, kBlock)), block(kBlock);

  // 2 the member lists
  if (step) {
    MB_HIP(plan_array(&p->agg, (size_t)n, &p->bytes));
    MB_HIP(plan_array(&p->member_ptr, (size_t)n_agg + 1, &p->bytes));
    MB_HIP(plan_array(&p->member, (size_t)n, &p->bytes));
    MB_HIP(hipMemcpyAsync(p->agg, agg, sizeof(int32_t) * (size_t)n,
                          hipMemcpyDeviceToDevice, st));
    Temp<int32_t> iota, sorted, empty;
    MB_HIP(iota.alloc((size_t)n, &book));
    MB_HIP(sorted.alloc((size_t)n, &book));
    MB_HIP(empty.alloc(1, &book));
    MB_HIP(hipMemsetAsync(empty.get(), 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(mcgs_iota_kernel, grid, block, 0, st, n, iota.get());
    MB_HIP(hipGetLastError());
    CubTemp tmp;
    MB_HIP(tmp.run(&book, [&](void* tm, size_t& tb) {
      return hipcub::DeviceRadixSort::SortPairs(tm, tb, agg, sorted.get(),
                                                iota.get(), p->member, (int)n, 0,
                                                bits_for(n_agg), st);
    }));
    hipLaunchKernelGGL(amg_member_ptr_kernel,
                       dim3(spmv_grid_for(ctx, (int64_t)n + 1, kBlock)), block, 0,
                       st, n, n_agg, sorted.get(), p->member_ptr);
    hipLaunchKernelGGL(amg_empty_kernel, dim3(spmv_grid_for(ctx, n_agg, kBlock)),
                       block, 0, st, n_agg, p->member_ptr, empty.get());
    MB_HIP(hipGetLastError());
    int32_t has_empty = 0;
    MB_HIP(plan_fetch(&has_empty, empty.get(), 1, st));
    if (has_empty) {
      info[0] = SPMV_HIP_AMG_EMPTY_AGG;
      return SPMV_HIP_EINVAL;
    }
  }

  // 3 the expanded rows' lengths
  TMap t;
  if (sym && (rc = build_tmap(ctx, n, num_cols, nnz, rowptr, colind, &book, st, &t))
                 != SPMV_HIP_OK)
    return rc;
  const XRows x{n, rowptr, colind, t.ptr, t.pos, t.row, sym};
  Temp<int64_t> xptr_tmp;
  int64_t* xptr;
  if (sym) {
    MB_HIP(plan_array(&p->xrow_ptr, (size_t)n + 1, &p->bytes));
    xptr = p->xrow_ptr;
  } else {
    MB_HIP(xptr_tmp.alloc((size_t)n + 1, &book));
    xptr = xptr_tmp.get();
  }
  hipLaunchKernelGGL(amg_xlen_kernel, grid, block, 0, st, x, xptr);
  MB_HIP(hipGetLastError());
  MB_HIP(scan_in_place(xptr, n, st));
  int64_t count = 0;
  MB_HIP(plan_fetch(&count, xptr + n, 1, st));
  if (count >= INT32_MAX) // (the scans take count + 1 elements as an int)
    return SPMV_HIP_ERANGE;
  info[2] = count;

  // 4 the entries: sources and keys, one stable sort
  const int bits = bits_for(n_agg);
  Temp<int32_t> src_tmp;
  Temp<uint64_t> keys, keys_sorted;
  int32_t* src_in;
  if (sym) {
    MB_HIP(plan_array(&p->xrow_src, (size_t)count, &p->bytes));
    p->xrow_count = count;
    src_in = p->xrow_src;
  } else {
    MB_HIP(src_tmp.alloc((size_t)count, &book));
    src_in = src_tmp.get();
  }
  if (step) {
    MB_HIP(keys.alloc((size_t)count, &book));
    MB_HIP(keys_sorted.alloc((size_t)count, &book));
    MB_HIP(plan_array(&p->src, (size_t)count, &p->bytes));
    p->src_count = count;
  }
  if (count > 0) {
    hipLaunchKernelGGL(amg_expand_kernel, grid, block, 0, st, x, xptr, agg, bits,
                       step ? keys.get() : nullptr, src_in);
    MB_HIP(hipGetLastError());
  }
  PlanScratch<int32_t> c_colind; // the caller's once the build has succeeded
  if (step) {
    // 5 the heads
    Temp<int64_t> index;
    MB_HIP(index.alloc((size_t)count + 1, &book));
    if (count > 0) {
      CubTemp tmp;
      MB_HIP(tmp.run(&book, [&](void* tm, size_t& tb) {
        return hipcub::DeviceRadixSort::SortPairs(
            tm, tb, keys.get(), keys_sorted.get(), src_in, p->src, (int)count, 0,
            2 * bits, st);
      }));
      hipLaunchKernelGGL(amg_heads_kernel, dim3(spmv_grid_for(ctx, count, kBlock)),
                         block, 0, st, count, keys_sorted.get(), index.get());
      MB_HIP(hipGetLastError());
      MB_HIP(hipStreamSynchronize(st)); // the sort's scratch goes with this scope
    }
    MB_HIP(scan_in_place(index.get(), count, st));
    int64_t nnz_c = 0;
    MB_HIP(plan_fetch(&nnz_c, index.get() + count, 1, st));
    p->coarse_nnz = nnz_c;
    MB_HIP(plan_array(&p->src_ptr, (size_t)nnz_c + 1, &p->bytes));
    Temp<int32_t> crow;
    MB_HIP(crow.alloc((size_t)nnz_c, &book));
    if (nnz_c > 0)
      MB_HIP(c_colind.alloc((size_t)nnz_c));
    if (count > 0) {
      hipLaunchKernelGGL(amg_entries_kernel,
                         dim3(spmv_grid_for(ctx, count, kBlock)), block, 0, st,
                         count, keys_sorted.get(), index.get(), bits, nnz_c,
                         p->src_ptr, c_colind.get(), crow.get());
    } else {
      MB_HIP(hipMemsetAsync(p->src_ptr, 0, sizeof(int64_t), st));
    }
    hipLaunchKernelGGL(amg_rowptr_kernel,
                       dim3(spmv_grid_for(ctx, nnz_c + 1, kBlock)), block, 0, st,
                       nnz_c, n_agg, crow.get(), coarse_rowptr);
    MB_HIP(hipGetLastError());
    MB_HIP(hipStreamSynchronize(st)); // the temporaries go with this scope
  }
  MB_HIP(hipStreamSynchronize(st));
  info[1] = book.peak;
  *coarse_nnz = p->coarse_nnz;
  c_colind.give(*coarse_colind);
  if (*coarse_colind) // the caller's from here on: off the builders' books
    --spmv_plan_live_allocs;
  *plan = guard.release();
  return SPMV_HIP_OK;
}

int spmv_hip_amg_plan_sizes(const spmv_hip_amg_plan* plan, int64_t* sizes)
{
  SPMV_REQUIRE(plan && sizes);
  sizes[0] = plan->fine_rows;
  sizes[1] = plan->coarse_rows;
  sizes[2] = plan->num_values;
  sizes[3] = plan->num_diagonal;
  sizes[4] = plan->coarse_nnz;
  sizes[5] = plan->src_count;
  sizes[6] = plan->xrow_ptr ? 1 : 0;
  sizes[7] = plan->xrow_count;
  sizes[8] = plan->bytes;
  return SPMV_HIP_OK;
}

int spmv_hip_amg_plan_export(const spmv_hip_amg_plan* plan,
                             const spmv_hip_amg_export* out)
{
  SPMV_REQUIRE(plan && out);
  SPMV_SET_DEVICE(plan->ctx);
  MB_HIP(hipStreamSynchronize(plan->ctx->stream));
  auto fetch = [&](auto* host, const auto* dev, int64_t count) {
    if (!host || !dev || count == 0)
      return hipSuccess;
    return hipMemcpy(host, dev, sizeof(*host) * (size_t)count,
                     hipMemcpyDeviceToHost);
  };
  const int64_t n = plan->fine_rows, nc = plan->coarse_rows;
  MB_HIP(fetch(out->agg, plan->agg, n));
  MB_HIP(fetch(out->member_ptr, plan->member_ptr, nc + 1));
  MB_HIP(fetch(out->member, plan->member, n));
  MB_HIP(fetch(out->src_ptr, plan->src_ptr, plan->coarse_nnz + 1));
  MB_HIP(fetch(out->src, plan->src, plan->src_count));
  MB_HIP(fetch(out->xrow_ptr, plan->xrow_ptr, n + 1));
  MB_HIP(fetch(out->xrow_src, plan->xrow_src, plan->xrow_count));
  return SPMV_HIP_OK;
}

} // extern "C"
