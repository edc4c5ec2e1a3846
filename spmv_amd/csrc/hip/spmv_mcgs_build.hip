// The setup of the multicolour sweeps on the device (gfx950): a parallel
// colouring of the local diagonal block and a builder of the sliced plan
// spmv_mcgs.hip reads, both from the CSR arrays where they lie.  No entry of
// the matrix, pattern or value, travels to the host: only counters and the
// num_colors + 1-sized tables the plan keeps there.
//
// COLOURING (spmv_hip_mcgs_color).  Greedy first-fit in a priority order:
//   colour(i) = the smallest colour not worn by a neighbour j of i with
//               prio(j) > prio(i)
// over the pattern of B + B^T, B the local diagonal block without its diagonal
// by host/sgs_build.cpp's rule off_diagonal(): c < num_rows, c != i, symmetric
// storage c < i.  Two orders: natural, prio(i) = -i (host/sgs_build.h's
// sgs_color, entry for entry), and hashed, prio(i) = mix64((i + 1) * G mod 2^64)
// compared unsigned (G odd, mix64 a bijection: no two rows tie).
//
// It is computed in Jones-Plassmann rounds, one launch per round, one lane per
// row: an uncoloured row whose neighbours of higher priority are all coloured
// takes its colour.  The result depends neither on scheduling nor on how many
// rows a round colours:
//   - a row only ever reads the colours of neighbours of HIGHER priority;
//   - a colour is final once written (-1 -> c, never again);
//   - a neighbour of lower priority cannot be coloured before the row is, so
//     nothing the row reads changes after the row has decided;
//   - a stale read of "uncoloured" only delays the row to a later round.
// The order between rounds is the stream's order and nothing else: no kernel
// here waits on another workgroup, nothing spins.  The host reads the "rows
// left" counters of a batch of rounds and stops when one is zero; the row of
// highest priority among the uncoloured is always ready, so num_rows rounds
// suffice and more are an error, not a hang.  The first-fit search looks at 64
// colours at a time and rescans the neighbours for the next window: any number
// of colours.  The neighbours of a row are its own entries and the rows of the
// transposed map of the pattern (spmv_tmap_build over all num_cols columns;
// columns >= num_rows are ghosts and ignored).
//
// PLAN (spmv_hip_mcgs_plan_build).  From a colour per row, every array of the
// plan as host/sgs_build.cpp's sgs_build + sgs_slice and spmv_hip_mcgs_plan_
// create produce it:
//   1 check, on the device, before anything is indexed: rowptr, columns, colours
//   2 perm: rows stably sorted by colour (radix sort); color_start from the
//     sorted colours; every colour worn
//   3 per row: the entries of each part counted, the colouring proved proper,
//     d by Matrix::diagonal's rule and dinv = 1.0 / d
//   4 every off-diagonal local entry as a key (position, part, column) with the
//     index of its value as payload -- a row's stored entries, then (symmetric
//     storage) the stable transpose of its column --, ONE stable radix sort:
//     ascending by column inside a part, duplicates in storage order
//   5 scans of the lengths; the sorted entries scattered into the slices and
//     the long lists.  Padding is memset: column 0, value +0.0.
// Temporaries are PlanScratch arrays, gone at return; a failure frees all.
//
// ILU(0) PLAN (spmv_hip_ilu0_plan_build).  The same five steps make the plan
// spmv_ilu0.hip factors on, every array as host/ilu0_build.cpp's ilu0_symbolic
// and spmv_hip_ilu0_plan_create produce it.  What differs (kIlu / `ilu`):
//   - no value is read; values, padding and dinv are +0.0 (memset), the
//     factorisation's to write; a diagonal is not looked at
//   4 the key's low field is the POSITION of the column: a part ascends by it
//     (the elimination's order), and the layout holds the column perm[field]
//   4b adjacent equal keys are two entries of one row with one column -- in
//     symmetric storage a stored entry and a mirror image, or two of either:
//     refused (SPMV_HIP_ILU0_DUPLICATE), a factor entry has ONE source
//   5 the scatter also writes the parts' CSR over positions: cpos, src (the
//     index of the stored entry, for its mirror image too) and slot, the place
//     it has just written (index into val, ~index into long_val); ptr is the
//     scan of the parts' counts
#include "common.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <new>
#include <vector>

#include "csr_plan.h"
#include "ilu0_plan.h"
#include "mcgs_plan.h"
#include "plan_build.h"
#include "plan_scratch.h"

namespace
{

// prio(j) > prio(i); hi = row_hash(i)
__device__ __forceinline__ bool higher(int32_t j, int32_t i, uint64_t hi, int order)
{
  return order == kNatural ? j < i : row_hash(j) > hi;
}

// sgs_build.cpp's off_diagonal()
__device__ __forceinline__ bool off_diagonal(int32_t i, int32_t c, int32_t n,
                                             int symmetric)
{
  return c < n && c != i && (!symmetric || c < i);
}

// ... and the same rule for the entry (j, i) of the transposed map of column i
__device__ __forceinline__ bool off_diagonal_t(int32_t i, int32_t j, int symmetric)
{
  return j != i && (!symmetric || j > i);
}

// One round.  left: the rows still uncoloured after it (one add per
// wavefront); max_colour: the largest colour given so far.
__global__ __launch_bounds__(kBlock) void mcgs_color_round_kernel(
    int32_t n, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ colind, const int32_t* __restrict__ t_ptr,
    const int32_t* __restrict__ t_row, int symmetric, int order, int32_t* colour,
    int32_t* __restrict__ left, int32_t* __restrict__ max_colour)
{
  int32_t my_left = 0, my_max = -1;
  for (int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < n;
       i64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)i64;
    if (colour[i] >= 0) // written by this lane alone, in an earlier launch
      continue;
    const uint64_t hi = row_hash(i);
    const int32_t r0 = rowptr[i], r1 = rowptr[i + 1];
    const int32_t t0 = t_ptr ? t_ptr[i] : 0, t1 = t_ptr ? t_ptr[i + 1] : 0;
    bool ready = true;
    int32_t mine = -1;
    for (int32_t base = 0; ready && mine < 0; base += 64) {
      uint64_t worn = 0; // colours base .. base + 63 of the neighbours above
      for (int32_t e = r0; e < r1 && ready; ++e) {
        const int32_t j = colind[e];
        if (!off_diagonal(i, j, n, symmetric) || !higher(j, i, hi, order))
          continue;
        const int32_t cj = __hip_atomic_load(colour + j, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        if (cj < 0)
          ready = false;
        else if (cj >= base && cj - base < 64)
          worn |= 1ull << (cj - base);
      }
      for (int32_t k = t0; k < t1 && ready; ++k) {
        const int32_t j = t_row[k];
        if (!off_diagonal_t(i, j, symmetric) || !higher(j, i, hi, order))
          continue;
        const int32_t cj = __hip_atomic_load(colour + j, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        if (cj < 0)
          ready = false;
        else if (cj >= base && cj - base < 64)
          worn |= 1ull << (cj - base);
      }
      if (ready && worn != ~0ull)
        mine = base + __ffsll((unsigned long long)~worn) - 1;
    }
    if (mine >= 0) {
      __hip_atomic_store(colour + i, mine, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      my_max = mine > my_max ? mine : my_max;
    } else {
      ++my_left;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    my_left += __shfl_down(my_left, off, 64);
    const int32_t o = __shfl_down(my_max, off, 64);
    my_max = o > my_max ? o : my_max;
  }
  if ((threadIdx.x & 63) == 0) {
    if (my_left)
      atomicAdd(left, my_left);
    if (my_max >= 0)
      atomicMax(max_colour, my_max);
  }
}

// color_start[c] = the first position whose colour is >= c, from the sorted
// colours (all in [0, C)): position p writes the colours between its
// predecessor's and its own; p == n closes the table.
__global__ __launch_bounds__(kBlock) void mcgs_color_start_kernel(
    int32_t n, int32_t num_colors, const int32_t* __restrict__ sorted,
    const int32_t* __restrict__ perm, int32_t* __restrict__ color_start,
    int32_t* __restrict__ pos_of)
{
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= n;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t prev = p == 0 ? -1 : sorted[p - 1];
    const int32_t cur = p == n ? num_colors : sorted[p];
    for (int32_t c = prev + 1; c <= cur; ++c)
      color_start[c] = (int32_t)p;
    if (p < n)
      pos_of[perm[p]] = (int32_t)p;
  }
}

// Per row: the entries of the two parts counted (by position), the colouring
// proved proper on B + B^T (symmetric storage: the row's stored entries and its
// column's; general storage: every stored entry is seen from its own row), the
// diagonal by Matrix::diagonal's rule and its inverse.  kIlu: no value is read
// and dinv stays the placeholder the caller has set.
template <bool kIlu>
__global__ __launch_bounds__(kBlock) void mcgs_count_kernel(
    int32_t n, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ colind, const double* __restrict__ values,
    const double* __restrict__ diagonal, const int32_t* __restrict__ t_ptr,
    const int32_t* __restrict__ t_row, int symmetric,
    const int32_t* __restrict__ colour, const int32_t* __restrict__ pos_of,
    int32_t* __restrict__ cnt_before, int32_t* __restrict__ cnt_after,
    int64_t* __restrict__ total, double* __restrict__ dinv,
    int32_t* __restrict__ improper_row, unsigned long long* __restrict__ bad_diag)
{
  for (int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < n;
       i64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)i64;
    const int32_t ci = colour[i];
    int32_t nb = 0, na = 0;
    bool improper = false;
    double d = 0.0;
    for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int32_t c = colind[e];
      if (!kIlu && c == i && !diagonal)
        d = d + values[e];
      if (!off_diagonal(i, c, n, symmetric))
        continue;
      const int32_t cc = colour[c];
      improper |= cc == ci;
      nb += cc < ci;
      na += cc > ci;
    }
    if (symmetric && t_ptr)
      for (int32_t k = t_ptr[i]; k < t_ptr[i + 1]; ++k) {
        const int32_t j = t_row[k];
        if (!off_diagonal_t(i, j, 1))
          continue;
        const int32_t cc = colour[j];
        improper |= cc == ci;
        nb += cc < ci;
        na += cc > ci;
      }
    if (!kIlu) {
      if (diagonal)
        d = diagonal[i];
      dinv[i] = 1.0 / d;
      if (!(d > 0.0) || !isfinite(d))
        atomicAdd(bad_diag, 1ull);
    }
    if (improper)
      atomicMin(improper_row, i);
    const int32_t pos = pos_of[i];
    cnt_before[pos] = nb;
    cnt_after[pos] = na;
    total[pos] = (int64_t)nb + na;
  }
}

// Per position and part: len (-1: a long row) and the two addends of the long
// lists' scans (rows, entries).
__global__ __launch_bounds__(kBlock) void mcgs_len_kernel(
    int32_t n, int32_t threshold, const int32_t* __restrict__ cnt,
    int32_t* __restrict__ len, int64_t* __restrict__ long_rows,
    int64_t* __restrict__ long_entries)
{
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t m = cnt[p];
    const bool is_long = m > threshold;
    len[p] = is_long ? -1 : m;
    long_rows[p] = is_long ? 1 : 0;
    long_entries[p] = is_long ? m : 0;
  }
}

// Per slice: 64 * its width, the addend of slice_ptr's scan.  pos_end[s]: the
// end of the slice's colour.
__global__ __launch_bounds__(kBlock) void mcgs_width_kernel(
    int32_t num_slices, const int32_t* __restrict__ slice_pos0,
    const int32_t* __restrict__ slice_end, const int32_t* __restrict__ len,
    int64_t* __restrict__ span)
{
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < num_slices;
       s += (int64_t)gridDim.x * blockDim.x) {
    int32_t w = 0;
    for (int32_t p = slice_pos0[s]; p < slice_end[s]; ++p)
      w = len[p] > w ? len[p] : w;
    span[s] = (int64_t)w * 64;
  }
}

// the long list's rows: position and first entry (long_ptr's last: `total`)
__global__ __launch_bounds__(kBlock) void mcgs_long_rows_kernel(
    int32_t n, const int32_t* __restrict__ len,
    const int64_t* __restrict__ long_index, const int64_t* __restrict__ long_first,
    int64_t num_long, int64_t total, int32_t* __restrict__ long_pos,
    int64_t* __restrict__ long_ptr)
{
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * blockDim.x) {
    if (p == 0)
      long_ptr[num_long] = total;
    if (len[p] >= 0)
      continue;
    const int64_t l = long_index[p];
    long_pos[l] = (int32_t)p;
    long_ptr[l] = long_first[p];
  }
}

// color_long[c] = the long rows in front of colour c, for both parts
__global__ void mcgs_color_long_kernel(int32_t num_colors,
                                       const int32_t* __restrict__ color_start,
                                       const int64_t* __restrict__ index_before,
                                       const int64_t* __restrict__ index_after,
                                       int32_t* __restrict__ out)
{
  for (int32_t c = blockIdx.x * blockDim.x + threadIdx.x; c <= num_colors;
       c += gridDim.x * blockDim.x) {
    out[c] = (int32_t)index_before[color_start[c]];
    out[num_colors + 1 + c] = (int32_t)index_after[color_start[c]];
  }
}

// Key of an entry: position, part (0 before, 1 after), column -- for the ILU(0)
// plan the POSITION of the column --; `bits` each for position and column.
__device__ __forceinline__ uint64_t entry_key(int32_t pos, int part, int32_t col,
                                              int bits)
{
  return ((uint64_t)pos << (bits + 1)) | ((uint64_t)part << bits) | (uint64_t)col;
}

// Per row: its entries as keys, in the order "stored entries, then the
// column's", at first[position]; the payload is the index of the value (of the
// stored lower entry, for a mirror image).
template <bool kIlu>
__global__ __launch_bounds__(kBlock) void mcgs_expand_kernel(
    int32_t n, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ colind, const int32_t* __restrict__ t_ptr,
    const int32_t* __restrict__ t_pos, const int32_t* __restrict__ t_row,
    int symmetric, const int32_t* __restrict__ colour,
    const int32_t* __restrict__ pos_of, const int64_t* __restrict__ first,
    int bits, uint64_t* __restrict__ keys, int32_t* __restrict__ src)
{
  for (int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < n;
       i64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)i64;
    const int32_t ci = colour[i], pos = pos_of[i];
    int64_t q = first[pos];
    for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int32_t c = colind[e];
      if (!off_diagonal(i, c, n, symmetric))
        continue;
      keys[q] = entry_key(pos, colour[c] > ci, kIlu ? pos_of[c] : c, bits);
      src[q++] = e;
    }
    if (symmetric && t_ptr)
      for (int32_t k = t_ptr[i]; k < t_ptr[i + 1]; ++k) {
        const int32_t j = t_row[k];
        if (!off_diagonal_t(i, j, 1))
          continue;
        keys[q] = entry_key(pos, colour[j] > ci, kIlu ? pos_of[j] : j, bits);
        src[q++] = t_pos[k];
      }
  }
}

struct PartOut {
  const int32_t* cnt;        // by position
  const int64_t* long_index; // by position: the row's slot in the long list
  const int64_t* slice_ptr;
  const int64_t* long_ptr;
  int32_t* col;
  double* val;
  int32_t* long_col;
  double* long_val;
};

// The ILU(0) plan's own arrays of a part (host/ilu0_build.h's Ilu0Part), CSR
// over positions.
struct IluOut {
  const int64_t* ptr;
  int32_t* cpos;
  int32_t* src;
  int64_t* slot;
};

// Per sorted entry: into its slice (entry k of lane l at slice_ptr[s] + 64 k +
// l) or its long row.  kIlu: the key's low field is the column's position; the
// layout receives the column perm[position] and NO value (the placeholders are
// memset, the factorisation writes them), and the entry's position, source and
// slot (fill_slots' rule: the index into val, or ~index into long_val) go to
// the part's CSR arrays.
template <bool kIlu>
__global__ __launch_bounds__(kBlock) void mcgs_scatter_kernel(
    int64_t num_entries, const uint64_t* __restrict__ keys,
    const int32_t* __restrict__ src, const double* __restrict__ values, int bits,
    int32_t threshold, const int64_t* __restrict__ first,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ colour,
    const int32_t* __restrict__ color_start,
    const int32_t* __restrict__ color_slice, PartOut before, PartOut after,
    IluOut ilu_before, IluOut ilu_after)
{
  const uint64_t low = ((uint64_t)1 << bits) - 1;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < num_entries;
       q += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t key = keys[q];
    const int32_t pos = (int32_t)(key >> (bits + 1));
    const int part = (int)((key >> bits) & 1);
    const int32_t field = (int32_t)(key & low);
    const int32_t col = kIlu ? perm[field] : field;
    const PartOut& out = part ? after : before;
    // the part's k-th entry of the row
    const int64_t k = q - first[pos] - (part ? before.cnt[pos] : 0);
    int64_t slot;
    if (out.cnt[pos] > threshold) {
      const int64_t at = out.long_ptr[out.long_index[pos]] + k;
      out.long_col[at] = col;
      if (!kIlu)
        out.long_val[at] = values[src[q]];
      slot = ~at;
    } else {
      const int32_t c = colour[perm[pos]];
      const int32_t in_colour = pos - color_start[c];
      const int64_t s = color_slice[c] + (in_colour >> 6);
      const int64_t at = out.slice_ptr[s] + 64 * k + (in_colour & 63);
      out.col[at] = col;
      if (!kIlu)
        out.val[at] = values[src[q]];
      slot = at;
    }
    if (kIlu) {
      const IluOut& o = part ? ilu_after : ilu_before;
      const int64_t e = o.ptr[pos] + k;
      o.cpos[e] = field;
      o.src[e] = src[q];
      o.slot[e] = slot;
    }
  }
}

// ILU(0): a factor entry has ONE source.  Two entries of a row with the same
// column are adjacent equal keys after the sort; the smallest such row.
__global__ __launch_bounds__(kBlock) void ilu0_duplicate_kernel(
    int64_t num_entries, const uint64_t* __restrict__ keys, int bits,
    const int32_t* __restrict__ perm, int32_t* __restrict__ duplicate_row)
{
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
       q < num_entries; q += (int64_t)gridDim.x * blockDim.x)
    if (keys[q] == keys[q - 1])
      atomicMin(duplicate_row, perm[(int32_t)(keys[q] >> (bits + 1))]);
}

// ILU(0): the addends of a part's ptr (int64, by position)
__global__ __launch_bounds__(kBlock) void ilu0_widen_kernel(
    int32_t n, const int32_t* __restrict__ cnt, int64_t* __restrict__ out)
{
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * blockDim.x)
    out[p] = cnt[p];
}

// ---- host side ---------------------------------------------------------------
struct PlanDeleter {
  spmv_hip_mcgs_plan* p = nullptr;
  ~PlanDeleter() { spmv_hip_mcgs_plan_destroy(p); }
  spmv_hip_mcgs_plan* release()
  {
    spmv_hip_mcgs_plan* q = p;
    p = nullptr;
    return q;
  }
};

} // namespace

extern "C" {

int spmv_hip_mcgs_color(spmv_hip_ctx* ctx, int32_t num_rows, int32_t num_cols,
                        int64_t nnz, const int32_t* rowptr, const int32_t* colind,
                        int symmetric, int order, int32_t* colors,
                        int* num_colors, int* rounds, void* stream)
{
  SPMV_REQUIRE(ctx && num_colors && rounds);
  SPMV_REQUIRE(args_ok(num_rows, num_cols, nnz, rowptr, colind));
  SPMV_REQUIRE(order == 0 || order == kNatural);
  SPMV_REQUIRE(num_rows == 0 || colors);
  *num_colors = 0;
  *rounds = 0;
  if (num_rows == 0)
    return SPMV_HIP_OK;
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  const int32_t n = num_rows;
  TempBytes book;
  Temp<int32_t> zeros;
  if (!rowptr)
    MB_HIP(zero_rowptr(zeros, n, &book, st, &rowptr));
  int32_t flags = 0;
  int rc = check_input(ctx, n, num_cols, nnz, rowptr, colind, nullptr, 0, &book,
                       st, &flags);
  if (rc != SPMV_HIP_OK)
    return rc;
  SPMV_REQUIRE(flags == 0);
  TMap t;
  if ((rc = build_tmap(ctx, n, num_cols, nnz, rowptr, colind, &book, st, &t))
      != SPMV_HIP_OK)
    return rc;
  Temp<int32_t> counters; // kBatch "rows left" and the largest colour
  MB_HIP(counters.alloc(kBatch + 1, &book));
  MB_HIP(hipMemsetAsync(colors, 0xff, sizeof(int32_t) * (size_t)n, st));
  MB_HIP(hipMemsetAsync(counters.get() + kBatch, 0xff, sizeof(int32_t), st));
  const int grid = spmv_grid_for(ctx, n, kBlock);
  int32_t host[kBatch + 1];
  int done_rounds = 0;
  bool done = false;
  while (!done) {
    // num_rows rounds colour any matrix: more is a fault of this code
    if ((int64_t)done_rounds >= (int64_t)n + 1)
      return SPMV_HIP_ERANGE;
    MB_HIP(hipMemsetAsync(counters.get(), 0, sizeof(int32_t) * kBatch, st));
    for (int b = 0; b < kBatch; ++b)
      hipLaunchKernelGGL(mcgs_color_round_kernel, dim3(grid), dim3(kBlock), 0, st,
                         n, rowptr, colind, t.ptr, t.row, symmetric ? 1 : 0, order,
                         colors, counters.get() + b, counters.get() + kBatch);
    MB_HIP(hipGetLastError());
    MB_HIP(plan_fetch(host, counters.get(), kBatch + 1, st));
    for (int b = 0; b < kBatch && !done; ++b) {
      ++done_rounds;
      done = host[b] == 0;
    }
  }
  *rounds = done_rounds;
  *num_colors = host[kBatch] + 1;
  return SPMV_HIP_OK;
}

} // extern "C"

namespace
{

// The builder of both plans, after the callers' argument checks, into `p` (the
// caller's to destroy on failure).  ilu == nullptr: the sweep plan of
// spmv_hip_mcgs_plan_build.  Otherwise the inner plan of an ILU(0) plan and
// the part arrays of `ilu` (ptr, cpos, src, slot; count): the entries ascend by
// the column's POSITION, a duplicate is refused, no value is read (values and
// diagonal are NULL) and every value, padding and dinv is +0.0.
int build_plan(spmv_hip_ctx* ctx, int32_t n, int32_t num_cols, int64_t nnz,
               const int32_t* rowptr, const int32_t* colind,
               const double* values, const double* diagonal, int sym,
               const int32_t* colors, int32_t C, int long_threshold,
               spmv_hip_mcgs_plan* p, spmv_hip_ilu0_plan* ilu, int64_t* info,
               hipStream_t st)
{
  TempBytes book;
  p->ctx = ctx;
  p->n = n;
  p->num_colors = C;
  p->color_start.assign((size_t)C + 1, 0);
  for (McgsPartDev* d : {&p->before, &p->after}) {
    d->color_slice.assign((size_t)C + 1, 0);
    d->color_long.assign((size_t)C + 1, 0);
  }

  // 1 the checks
  Temp<int32_t> zeros;
  if (n > 0 && !rowptr)
    MB_HIP(zero_rowptr(zeros, n, &book, st, &rowptr));
  if (n > 0) {
    int32_t flags = 0;
    const int rc = check_input(ctx, n, num_cols, nnz, rowptr, colind, colors, C,
                               &book, st, &flags);
    if (rc != SPMV_HIP_OK)
      return rc;
    if (flags) {
      info[1] = (flags & 1)   ? SPMV_HIP_MCGS_BAD_ROWPTR
                : (flags & 2) ? SPMV_HIP_MCGS_BAD_COLUMN
                              : SPMV_HIP_MCGS_BAD_COLOR;
      return SPMV_HIP_EINVAL;
    }
  }

  // 2 perm and color_start
  Temp<int32_t> pos_of, d_cstart;
  MB_HIP(plan_array(&p->perm, (size_t)n, &p->bytes));
  MB_HIP(plan_array(&p->dinv, (size_t)n, &p->bytes));
  const int grid_n = spmv_grid_for(ctx, n, kBlock);
  if (n > 0) {
    Temp<int32_t> iota, sorted;
    MB_HIP(iota.alloc((size_t)n, &book));
    MB_HIP(sorted.alloc((size_t)n, &book));
    MB_HIP(pos_of.alloc((size_t)n, &book));
    MB_HIP(d_cstart.alloc((size_t)C + 1, &book));
    hipLaunchKernelGGL(mcgs_iota_kernel, dim3(grid_n), dim3(kBlock), 0, st, n,
                       iota.get());
    MB_HIP(hipGetLastError());
    CubTemp tmp;
    MB_HIP(tmp.run(&book, [&](void* t, size_t& tb) {
      return hipcub::DeviceRadixSort::SortPairs(t, tb, colors, sorted.get(),
                                                iota.get(), p->perm, (int)n, 0,
                                                bits_for(C), st);
    }));
    hipLaunchKernelGGL(mcgs_color_start_kernel,
                       dim3(spmv_grid_for(ctx, (int64_t)n + 1, kBlock)),
                       dim3(kBlock), 0, st, n, C, sorted.get(), p->perm,
                       d_cstart.get(), pos_of.get());
    MB_HIP(hipGetLastError());
    MB_HIP(plan_fetch(p->color_start.data(), d_cstart.get(), (size_t)C + 1, st));
    for (int c = 0; c < C; ++c) // every colour is worn
      if (p->color_start[(size_t)c + 1] <= p->color_start[c]) {
        info[1] = SPMV_HIP_MCGS_UNWORN_COLOR;
        return SPMV_HIP_EINVAL;
      }
  }

  // the slices: the same for both parts
  std::vector<int32_t> slice_pos0, slice_end;
  std::vector<int32_t>& cslice = p->before.color_slice;
  for (int c = 0; c < C; ++c) {
    const int32_t c0 = p->color_start[c], c1 = p->color_start[(size_t)c + 1];
    for (int32_t p0 = c0; p0 < c1; p0 += 64) {
      slice_pos0.push_back(p0);
      slice_end.push_back(p0 + 64 < c1 ? p0 + 64 : c1);
    }
    cslice[(size_t)c + 1] = (int32_t)slice_pos0.size();
  }
  p->after.color_slice = cslice;
  const size_t ns = slice_pos0.size();
  McgsPartDev* parts[2] = {&p->before, &p->after};
  for (McgsPartDev* d : parts) {
    MB_HIP(plan_array(&d->slice_pos0, ns, &p->bytes));
    MB_HIP(plan_array(&d->slice_ptr, ns + 1, &p->bytes));
    MB_HIP(plan_array(&d->len, (size_t)n, &p->bytes));
    if (ns)
      MB_HIP(hipMemcpyAsync(d->slice_pos0, slice_pos0.data(), sizeof(int32_t) * ns,
                            hipMemcpyHostToDevice, st));
  }
  if (n == 0) { // the two tables of one zero each, as the host builder's
    for (McgsPartDev* d : parts) {
      MB_HIP(plan_array(&d->long_ptr, 1, &p->bytes));
      MB_HIP(hipMemsetAsync(d->slice_ptr, 0, sizeof(int64_t), st));
      MB_HIP(hipMemsetAsync(d->long_ptr, 0, sizeof(int64_t), st));
    }
    MB_HIP(hipStreamSynchronize(st));
    info[2] = book.peak;
    return SPMV_HIP_OK;
  }
  if (ilu) // the placeholder: the factorisation writes dinv
    MB_HIP(hipMemsetAsync(p->dinv, 0, sizeof(double) * (size_t)n, st));
  Temp<int32_t> d_slice_end, d_cslice;
  MB_HIP(d_slice_end.alloc(ns, &book));
  MB_HIP(d_cslice.alloc((size_t)C + 1, &book));
  MB_HIP(hipMemcpyAsync(d_slice_end.get(), slice_end.data(), sizeof(int32_t) * ns,
                        hipMemcpyHostToDevice, st));
  MB_HIP(hipMemcpyAsync(d_cslice.get(), cslice.data(), sizeof(int32_t) * (C + 1),
                        hipMemcpyHostToDevice, st));
  MB_HIP(hipStreamSynchronize(st)); // (the host vectors are pageable)

  // 3 the lengths, the proof of the colouring, the diagonal
  TMap t;
  if (sym) {
    const int rc = build_tmap(ctx, n, num_cols, nnz, rowptr, colind, &book, st, &t);
    if (rc != SPMV_HIP_OK)
      return rc;
  }
  Temp<int32_t> cnt[2], improper;
  Temp<int64_t> first, long_index[2], long_first[2];
  Temp<unsigned long long> bad_diag;
  MB_HIP(first.alloc((size_t)n + 1, &book));
  MB_HIP(improper.alloc(1, &book));
  MB_HIP(bad_diag.alloc(1, &book));
  for (int h = 0; h < 2; ++h) {
    MB_HIP(cnt[h].alloc((size_t)n, &book));
    MB_HIP(long_index[h].alloc((size_t)n + 1, &book));
    MB_HIP(long_first[h].alloc((size_t)n + 1, &book));
  }
  const int32_t no_row = INT32_MAX; // (n < INT32_MAX: args_ok)
  MB_HIP(hipMemcpy(improper.get(), &no_row, sizeof(int32_t), hipMemcpyHostToDevice));
  MB_HIP(hipMemsetAsync(bad_diag.get(), 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(ilu ? mcgs_count_kernel<true> : mcgs_count_kernel<false>,
                     dim3(grid_n), dim3(kBlock), 0, st, n, rowptr, colind, values,
                     diagonal, t.ptr, t.row, sym, colors, pos_of.get(),
                     cnt[0].get(), cnt[1].get(), first.get(), p->dinv,
                     improper.get(), bad_diag.get());
  MB_HIP(hipGetLastError());
  int32_t improper_row = 0;
  unsigned long long bad = 0;
  MB_HIP(plan_fetch(&improper_row, improper.get(), 1, st));
  MB_HIP(plan_fetch(&bad, bad_diag.get(), 1, st));
  if (improper_row < n) {
    info[1] = SPMV_HIP_MCGS_IMPROPER;
    info[3] = improper_row;
    return SPMV_HIP_EINVAL;
  }
  info[0] = (int64_t)bad;

  // 5a the scans
  const int grid_s = spmv_grid_for(ctx, (int64_t)ns, kBlock);
  for (int h = 0; h < 2; ++h) {
    McgsPartDev* d = parts[h];
    hipLaunchKernelGGL(mcgs_len_kernel, dim3(grid_n), dim3(kBlock), 0, st, n,
                       (int32_t)long_threshold, cnt[h].get(), d->len,
                       long_index[h].get(), long_first[h].get());
    hipLaunchKernelGGL(mcgs_width_kernel, dim3(grid_s), dim3(kBlock), 0, st,
                       (int32_t)ns, d->slice_pos0, d_slice_end.get(), d->len,
                       d->slice_ptr);
    MB_HIP(hipGetLastError());
    MB_HIP(scan_in_place(long_index[h].get(), n, st));
    MB_HIP(scan_in_place(long_first[h].get(), n, st));
    MB_HIP(scan_in_place(d->slice_ptr, (int64_t)ns, st));
  }
  MB_HIP(scan_in_place(first.get(), n, st));
  int64_t num_entries = 0, num_long[2], long_entries[2], sliced[2];
  MB_HIP(plan_fetch(&num_entries, first.get() + n, 1, st));
  for (int h = 0; h < 2; ++h) {
    MB_HIP(plan_fetch(&num_long[h], long_index[h].get() + n, 1, st));
    MB_HIP(plan_fetch(&long_entries[h], long_first[h].get() + n, 1, st));
    MB_HIP(plan_fetch(&sliced[h], parts[h]->slice_ptr + ns, 1, st));
  }
  if (num_entries >= INT32_MAX) // (the scans take count + 1 elements as an int)
    return SPMV_HIP_ERANGE;

  // ILU(0): the parts' own CSR over positions
  Ilu0PartDev* ilu_parts[2] = {ilu ? &ilu->before : nullptr,
                               ilu ? &ilu->after : nullptr};
  if (ilu)
    for (int h = 0; h < 2; ++h) {
      Ilu0PartDev* d = ilu_parts[h];
      MB_HIP(plan_array(&d->ptr, (size_t)n + 1, &ilu->bytes));
      hipLaunchKernelGGL(ilu0_widen_kernel, dim3(grid_n), dim3(kBlock), 0, st, n,
                         cnt[h].get(), d->ptr);
      MB_HIP(hipGetLastError());
      MB_HIP(scan_in_place(d->ptr, n, st));
      MB_HIP(plan_fetch(&d->count, d->ptr + n, 1, st));
      MB_HIP(plan_array(&d->cpos, (size_t)d->count, &ilu->bytes));
      MB_HIP(plan_array(&d->src, (size_t)d->count, &ilu->bytes));
      MB_HIP(plan_array(&d->slot, (size_t)d->count, &ilu->bytes));
    }

  // the long lists' tables
  Temp<int32_t> d_clong;
  MB_HIP(d_clong.alloc(2 * ((size_t)C + 1), &book));
  for (int h = 0; h < 2; ++h) {
    McgsPartDev* d = parts[h];
    MB_HIP(plan_array(&d->col, (size_t)sliced[h], &p->bytes));
    MB_HIP(plan_array(&d->val, (size_t)sliced[h], &p->bytes));
    MB_HIP(plan_array(&d->long_pos, (size_t)num_long[h], &p->bytes));
    MB_HIP(plan_array(&d->long_ptr, (size_t)num_long[h] + 1, &p->bytes));
    MB_HIP(plan_array(&d->long_col, (size_t)long_entries[h], &p->bytes));
    MB_HIP(plan_array(&d->long_val, (size_t)long_entries[h], &p->bytes));
    if (sliced[h]) { // the padding: column 0, value +0.0
      MB_HIP(hipMemsetAsync(d->col, 0, sizeof(int32_t) * (size_t)sliced[h], st));
      MB_HIP(hipMemsetAsync(d->val, 0, sizeof(double) * (size_t)sliced[h], st));
    }
    if (ilu && long_entries[h])
      MB_HIP(hipMemsetAsync(d->long_val, 0,
                            sizeof(double) * (size_t)long_entries[h], st));
    hipLaunchKernelGGL(mcgs_long_rows_kernel, dim3(grid_n), dim3(kBlock), 0, st,
                       n, d->len, long_index[h].get(), long_first[h].get(),
                       num_long[h], long_entries[h], d->long_pos, d->long_ptr);
    MB_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(mcgs_color_long_kernel, dim3(1), dim3(kBlock), 0, st, C,
                     d_cstart.get(), long_index[0].get(), long_index[1].get(),
                     d_clong.get());
  MB_HIP(hipGetLastError());
  MB_HIP(plan_fetch(p->before.color_long.data(), d_clong.get(), (size_t)C + 1, st));
  MB_HIP(plan_fetch(p->after.color_long.data(), d_clong.get() + C + 1,
                    (size_t)C + 1, st));

  // 4 and 5b the entries: keys, one stable sort, the scatter
  if (num_entries > 0) {
    const int bits = bits_for(n);
    Temp<uint64_t> keys, keys_sorted;
    Temp<int32_t> src, src_sorted;
    MB_HIP(keys.alloc((size_t)num_entries, &book));
    MB_HIP(keys_sorted.alloc((size_t)num_entries, &book));
    MB_HIP(src.alloc((size_t)num_entries, &book));
    MB_HIP(src_sorted.alloc((size_t)num_entries, &book));
    hipLaunchKernelGGL(ilu ? mcgs_expand_kernel<true> : mcgs_expand_kernel<false>,
                       dim3(grid_n), dim3(kBlock), 0, st, n, rowptr, colind, t.ptr,
                       t.pos, t.row, sym, colors, pos_of.get(), first.get(), bits,
                       keys.get(), src.get());
    MB_HIP(hipGetLastError());
    CubTemp tmp;
    MB_HIP(tmp.run(&book, [&](void* tm, size_t& tb) {
      return hipcub::DeviceRadixSort::SortPairs(
          tm, tb, keys.get(), keys_sorted.get(), src.get(), src_sorted.get(),
          (int)num_entries, 0, 2 * bits + 1, st);
    }));
    const int grid_e = spmv_grid_for(ctx, num_entries, kBlock);
    if (ilu) { // (`improper` has done its work and holds INT32_MAX)
      hipLaunchKernelGGL(ilu0_duplicate_kernel, dim3(grid_e), dim3(kBlock), 0, st,
                         num_entries, keys_sorted.get(), bits, p->perm,
                         improper.get());
      MB_HIP(hipGetLastError());
      int32_t duplicate_row = 0;
      MB_HIP(plan_fetch(&duplicate_row, improper.get(), 1, st));
      if (duplicate_row < n) {
        info[1] = SPMV_HIP_ILU0_DUPLICATE;
        info[3] = duplicate_row;
        return SPMV_HIP_EINVAL;
      }
    }
    PartOut out[2];
    IluOut iout[2] = {};
    for (int h = 0; h < 2; ++h) {
      out[h] = PartOut{cnt[h].get(),       long_index[h].get(), parts[h]->slice_ptr,
                       parts[h]->long_ptr, parts[h]->col,       parts[h]->val,
                       parts[h]->long_col, parts[h]->long_val};
      if (ilu)
        iout[h] = IluOut{ilu_parts[h]->ptr, ilu_parts[h]->cpos, ilu_parts[h]->src,
                         ilu_parts[h]->slot};
    }
    hipLaunchKernelGGL(ilu ? mcgs_scatter_kernel<true> : mcgs_scatter_kernel<false>,
                       dim3(grid_e), dim3(kBlock), 0, st, num_entries,
                       keys_sorted.get(), src_sorted.get(), values, bits,
                       (int32_t)long_threshold, first.get(), p->perm, colors,
                       d_cstart.get(), d_cslice.get(), out[0], out[1], iout[0],
                       iout[1]);
    MB_HIP(hipGetLastError());
    MB_HIP(hipStreamSynchronize(st)); // the temporaries go with this scope
  }
  MB_HIP(hipStreamSynchronize(st));
  info[2] = book.peak;
  return SPMV_HIP_OK;
}

struct Ilu0PlanDeleter {
  spmv_hip_ilu0_plan* p = nullptr;
  ~Ilu0PlanDeleter() { spmv_hip_ilu0_plan_destroy(p); }
  spmv_hip_ilu0_plan* release()
  {
    spmv_hip_ilu0_plan* q = p;
    p = nullptr;
    return q;
  }
};

} // namespace

extern "C" {

int spmv_hip_mcgs_plan_build(spmv_hip_ctx* ctx, int32_t num_rows,
                             int32_t num_cols, int64_t nnz, const int32_t* rowptr,
                             const int32_t* colind, const double* values,
                             const double* diagonal, int symmetric,
                             const int32_t* colors, int32_t num_colors,
                             int long_threshold, spmv_hip_mcgs_plan** plan,
                             int64_t* info, void* stream)
{
  SPMV_REQUIRE(ctx && plan && info);
  *plan = nullptr;
  for (int k = 0; k < SPMV_HIP_MCGS_INFO_WORDS; ++k)
    info[k] = 0;
  SPMV_REQUIRE(args_ok(num_rows, num_cols, nnz, rowptr, colind));
  SPMV_REQUIRE(nnz == 0 || values);
  SPMV_REQUIRE(long_threshold >= 0 && num_colors >= 0);
  SPMV_REQUIRE((num_rows == 0) == (num_colors == 0));
  SPMV_REQUIRE(num_rows == 0 || colors);
  SPMV_REQUIRE(!symmetric || num_rows == 0 || diagonal);
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  const int sym = symmetric ? 1 : 0;
  if (!sym)
    diagonal = nullptr;
  PlanDeleter guard;
  guard.p = new (std::nothrow) spmv_hip_mcgs_plan();
  if (!guard.p)
    return SPMV_HIP_ENOMEM;
  const int rc = build_plan(ctx, num_rows, num_cols, nnz, rowptr, colind, values,
                            diagonal, sym, colors, num_colors, long_threshold,
                            guard.p, nullptr, info, st);
  if (rc == SPMV_HIP_OK)
    *plan = guard.release();
  return rc;
}

int spmv_hip_mcgs_plan_build_ex(spmv_hip_ctx* ctx, int32_t num_rows,
                                int32_t num_cols, int64_t nnz,
                                const int32_t* rowptr, const int32_t* colind,
                                const double* values, const double* diagonal,
                                int symmetric, const int32_t* colors,
                                int32_t num_colors, int long_threshold,
                                int value_bits, spmv_hip_mcgs_plan** plan,
                                int64_t* info, int64_t* out_of_range,
                                void* stream)
{
  SPMV_REQUIRE(plan != nullptr);
  *plan = nullptr;
  SPMV_REQUIRE(out_of_range && (value_bits == 64 || value_bits == 32));
  *out_of_range = 0;
  PlanDeleter guard;
  int rc = spmv_hip_mcgs_plan_build(ctx, num_rows, num_cols, nnz, rowptr, colind,
                                    values, diagonal, symmetric, colors,
                                    num_colors, long_threshold, &guard.p, info,
                                    stream);
  if (rc == SPMV_HIP_OK && value_bits == 32) {
    rc = mcgs_plan_narrow(guard.p, spmv_stream(ctx, stream), out_of_range);
    if (rc == SPMV_HIP_OK && *out_of_range != 0)
      rc = SPMV_HIP_ERANGE;
  }
  if (rc == SPMV_HIP_OK)
    *plan = guard.release();
  return rc;
}

int spmv_hip_ilu0_plan_build_ex(spmv_hip_ctx* ctx, int32_t num_rows,
                                int32_t num_cols, int64_t nnz,
                                const int32_t* rowptr, const int32_t* colind,
                                int symmetric, const int32_t* colors,
                                int32_t num_colors, int long_threshold,
                                int value_bits, spmv_hip_ilu0_plan** plan,
                                int64_t* info, void* stream)
{
  SPMV_REQUIRE(plan != nullptr);
  *plan = nullptr;
  SPMV_REQUIRE(value_bits == 64 || value_bits == 32);
  Ilu0PlanDeleter guard;
  int rc = spmv_hip_ilu0_plan_build(ctx, num_rows, num_cols, nnz, rowptr, colind,
                                    symmetric, colors, num_colors, long_threshold,
                                    &guard.p, info, stream);
  if (rc == SPMV_HIP_OK && value_bits == 32) {
    // the placeholders (+0.0) in the form the factorisation will write
    int64_t none = 0;
    rc = mcgs_plan_narrow(guard.p->inner, spmv_stream(ctx, stream), &none);
  }
  if (rc == SPMV_HIP_OK)
    *plan = guard.release();
  return rc;
}

int spmv_hip_ilu0_plan_build(spmv_hip_ctx* ctx, int32_t num_rows,
                             int32_t num_cols, int64_t nnz, const int32_t* rowptr,
                             const int32_t* colind, int symmetric,
                             const int32_t* colors, int32_t num_colors,
                             int long_threshold, spmv_hip_ilu0_plan** plan,
                             int64_t* info, void* stream)
{
  SPMV_REQUIRE(ctx && plan && info);
  *plan = nullptr;
  for (int k = 0; k < SPMV_HIP_MCGS_INFO_WORDS; ++k)
    info[k] = 0;
  SPMV_REQUIRE(args_ok(num_rows, num_cols, nnz, rowptr, colind));
  SPMV_REQUIRE(long_threshold >= 0 && num_colors >= 0);
  SPMV_REQUIRE((num_rows == 0) == (num_colors == 0));
  SPMV_REQUIRE(num_rows == 0 || colors);
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  Ilu0PlanDeleter guard; // (destroys the inner plan with its owner)
  guard.p = new (std::nothrow) spmv_hip_ilu0_plan();
  if (!guard.p)
    return SPMV_HIP_ENOMEM;
  spmv_hip_ilu0_plan* p = guard.p;
  p->ctx = ctx;
  p->n = num_rows;
  p->num_values = nnz;
  p->inner = new (std::nothrow) spmv_hip_mcgs_plan();
  if (!p->inner)
    return SPMV_HIP_ENOMEM;
  p->inner->ctx = ctx;
  const int rc = build_plan(ctx, num_rows, num_cols, nnz, rowptr, colind, nullptr,
                            nullptr, symmetric ? 1 : 0, colors, num_colors,
                            long_threshold, p->inner, p, info, st);
  if (rc != SPMV_HIP_OK)
    return rc;
  // the working arrays, as ilu0_plan_create reserves them
  const size_t n = (size_t)num_rows;
  MB_HIP(plan_array(&p->before.w, (size_t)p->before.count, &p->bytes));
  MB_HIP(plan_array(&p->after.w, (size_t)p->after.count, &p->bytes));
  MB_HIP(plan_array(&p->wd, n, &p->bytes));
  MB_HIP(plan_array(&p->wdinv, n, &p->bytes));
  MB_HIP(plan_array(&p->counts, (size_t)4, &p->bytes));
  *plan = guard.release();
  return SPMV_HIP_OK;
}

int spmv_hip_mcgs_plan_sizes(const spmv_hip_mcgs_plan* plan, int64_t* sizes)
{
  SPMV_REQUIRE(plan && sizes);
  SPMV_SET_DEVICE(plan->ctx);
  hipStream_t st = plan->ctx->stream;
  const int C = plan->num_colors;
  sizes[0] = plan->n;
  sizes[1] = C;
  sizes[2] = plan->before.color_slice[(size_t)C];
  const McgsPartDev* parts[2] = {&plan->before, &plan->after};
  for (int h = 0; h < 2; ++h) {
    const McgsPartDev* d = parts[h];
    const int64_t ns = d->color_slice[(size_t)C], nl = d->color_long[(size_t)C];
    int64_t entries = 0, long_entries = 0;
    MB_HIP(plan_fetch(&entries, d->slice_ptr + ns, 1, st));
    MB_HIP(plan_fetch(&long_entries, d->long_ptr + nl, 1, st));
    sizes[3 + 3 * h] = entries;
    sizes[4 + 3 * h] = nl;
    sizes[5 + 3 * h] = long_entries;
  }
  sizes[9] = plan->bytes;
  return SPMV_HIP_OK;
}

int spmv_hip_mcgs_plan_export(const spmv_hip_mcgs_plan* plan, int32_t* perm,
                              int32_t* color_start, double* dinv,
                              const spmv_hip_mcgs_export* before,
                              const spmv_hip_mcgs_export* after)
{
  SPMV_REQUIRE(plan != nullptr);
  int64_t sizes[SPMV_HIP_MCGS_SIZES_WORDS];
  const int rc = spmv_hip_mcgs_plan_sizes(plan, sizes);
  if (rc != SPMV_HIP_OK)
    return rc;
  hipStream_t st = plan->ctx->stream;
  MB_HIP(hipStreamSynchronize(st));
  auto fetch = [&](auto* host, const auto* dev, int64_t count) {
    if (!host || count == 0)
      return hipSuccess;
    return hipMemcpy(host, dev, sizeof(*host) * (size_t)count,
                     hipMemcpyDeviceToHost);
  };
  // the values of a part, widened where the plan keeps floats
  std::vector<float> narrow;
  auto fetch_values = [&](double* host, const double* dev, const float* dev32,
                          int64_t count) {
    if (plan->value_bits == 64 || !host || count == 0)
      return fetch(host, dev, count);
    try {
      narrow.resize((size_t)count);
    } catch (...) {
      return hipErrorOutOfMemory;
    }
    const hipError_t e = fetch(narrow.data(), dev32, count);
    if (e == hipSuccess)
      std::copy(narrow.begin(), narrow.end(), host);
    return e;
  };
  const int64_t n = plan->n, C = plan->num_colors, ns = sizes[2];
  MB_HIP(fetch(perm, plan->perm, n));
  MB_HIP(fetch(dinv, plan->dinv, n));
  if (color_start)
    std::copy(plan->color_start.begin(), plan->color_start.end(), color_start);
  const McgsPartDev* parts[2] = {&plan->before, &plan->after};
  const spmv_hip_mcgs_export* outs[2] = {before, after};
  for (int h = 0; h < 2; ++h) {
    const spmv_hip_mcgs_export* o = outs[h];
    if (!o)
      continue;
    const McgsPartDev* d = parts[h];
    const int64_t entries = sizes[3 + 3 * h], nl = sizes[4 + 3 * h],
                  long_entries = sizes[5 + 3 * h];
    if (o->color_slice)
      std::copy(d->color_slice.begin(), d->color_slice.end(), o->color_slice);
    if (o->color_long)
      std::copy(d->color_long.begin(), d->color_long.end(), o->color_long);
    (void)C;
    MB_HIP(fetch(o->slice_pos0, d->slice_pos0, ns));
    MB_HIP(fetch(o->slice_ptr, d->slice_ptr, ns + 1));
    MB_HIP(fetch(o->len, d->len, n));
    MB_HIP(fetch(o->col, d->col, entries));
    MB_HIP(fetch_values(o->val, d->val, d->val32, entries));
    MB_HIP(fetch(o->long_pos, d->long_pos, nl));
    MB_HIP(fetch(o->long_ptr, d->long_ptr, nl + 1));
    MB_HIP(fetch(o->long_col, d->long_col, long_entries));
    MB_HIP(fetch_values(o->long_val, d->long_val, d->long_val32,
                        long_entries));
  }
  return SPMV_HIP_OK;
}

} // extern "C"
