// Multicolour ILU(0) factored on the device (gfx950): the numeric half of
// spmv::Ilu0Preconditioner.  M = (D~ + L~) D~^-1 (D~ + U~) on the local diagonal
// block in the colour-major ordering; its application is spmv_mcgs.hip's two
// sweeps on a plan whose values and dinv THIS file writes.
//
// The host (host/ilu0_build.h, through ilu0_plan_create) or the device builder
// (spmv_mcgs_build.hip: ilu0_plan_build) delivers, per part (before / after) and
// by POSITION: the row pointer, the position of every entry's column (ascending
// in a row), the index of its value in the matrix's value array and its slot in
// the sliced layout.  A factorisation is, on one stream and in its order alone:
//
//   ilu0_gather   the working values of both parts from the matrix's values
//   ilu0_diag     the working diagonal d (by position) and 1.0 / d
//   ilu0_factor   one launch per colour 1 .. C-1, one wavefront per row:
//                   for k in before(i), ascending pos(k):
//                     m = w[k] * dinv~[k]
//                     for (j, u) in after~(k): if j == i or j in row i:
//                       w[j] = w[j] - m * u
//                   d~_i = w[i]; dinv~_i = 1.0 / d~_i
//   ilu0_finish   dinv~ by row into the sweep plan; the pivot counts
//   ilu0_scatter  l~ and u~ into the sliced values of the sweep plan
//
// Order and paths of ilu0_factor.  The loop over k is wave-uniform; the lanes
// stride over after~(k), the finished row of an EARLIER launch.  before(i), the
// diagonal and after(i) form one list ascending by position (smaller colours,
// the row itself, larger colours), so a lane finds its j by one binary search
// in that list; the distinct j of one k are distinct entries and lanes never
// collide.  The list's values are written by some lanes in step k and read by
// all in a later step:
//   * a row whose list has at most kSlab entries keeps values and positions in
//     a slab of LDS of its wavefront (LDS operations of one wavefront execute in
//     order) and writes the values back at the end;
//   * a longer row (a hub row) works in the global arrays themselves, through
//     the CU's L1 that all lanes of the wavefront share.
// Both paths put a wavefront-scope release / acquire fence pair between two
// steps: it costs no instruction and keeps the compiler from moving a step's
// loads above the previous step's stores.  What the hub-row path RESTS ON is
// the hardware's order, not the fence: the vector memory operations of one
// wavefront go to the CU's one L1 in issue order, a store updates or drops the
// line it hits, so a later load of the same wavefront -- any lane -- sees an
// earlier store.  This is the rule by which LLVM's AMDGPU memory model (AMDGPU
// backend user guide, "Memory Model", gfx90a / gfx942 and their successors)
// emits no wait and no cache action for wavefront-scope synchronisation, and
// no more for workgroup scope while the workgroup's waves share an L1.  A port
// to a part where that does not hold (an L1 per SIMD, a split workgroup) must
// make the pair workgroup-scope fences, which wait for the stores.  Every entry receives its
// subtractions in ascending pos(k) whichever lane performs them, so the bits do
// not depend on the distribution of the work.  No kernel waits on another
// workgroup; no floating-point atomics; the pivot counts are integer atomics,
// one per wavefront.
//
// Built with -ffp-contract=off: every product, difference and quotient is a
// rounding of its own.
#include "common.h"

#include <new>
#include <vector>

#include "fp32_range.h"
#include "ilu0_plan.h"
#include "plan_scratch.h"

namespace
{

constexpr int kWaves = kBlock / 64;
constexpr int kSlab = 256;
constexpr int64_t kMaxGridX = (int64_t)1 << 20; // blocks of a factor launch in x

__global__ __launch_bounds__(kBlock) void ilu0_gather_kernel(
    int64_t count, const int32_t* __restrict__ src,
    const double* __restrict__ values, double* __restrict__ w)
{
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < count;
       e += stride)
    w[e] = values[src[e]];
}

__global__ __launch_bounds__(kBlock) void ilu0_diag_kernel(
    int32_t n, const int32_t* __restrict__ perm,
    const double* __restrict__ diagonal, double* __restrict__ wd,
    double* __restrict__ wdinv)
{
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n;
       p += stride) {
    const double d = diagonal[perm[p]];
    wd[p] = d;
    wdinv[p] = 1.0 / d;
  }
}

// between two steps of a row: what the lanes wrote is what the lanes read
__device__ __forceinline__ void wave_step()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the row's list in a slab of LDS
struct LdsRow {
  double* w;
  int32_t* c;
  __device__ __forceinline__ double get(int i) const { return w[i]; }
  __device__ __forceinline__ void set(int i, double v) const { w[i] = v; }
  __device__ __forceinline__ int32_t cpos(int i) const { return c[i]; }
};

// the row's list where it lies in global memory: before, diagonal, after
struct GlobalRow {
  double* bw;
  double* d;
  double* aw;
  const int32_t* bc;
  const int32_t* ac;
  int nb;
  int32_t pos;
  __device__ __forceinline__ double* at(int i) const
  {
    return i < nb ? bw + i : i == nb ? d : aw + (i - nb - 1);
  }
  __device__ __forceinline__ double get(int i) const { return *at(i); }
  __device__ __forceinline__ void set(int i, double v) const { *at(i) = v; }
  __device__ __forceinline__ int32_t cpos(int i) const
  {
    return i < nb ? bc[i] : i == nb ? pos : ac[i - nb - 1];
  }
};

// a_w is read at the rows of earlier launches only; the row of this wavefront
// (GlobalRow) writes its own entries of the same array
template <class Row>
__device__ __forceinline__ void factor_row(const Row& row, int nb, int tot,
                                           int lane, const int64_t* a_ptr,
                                           const int32_t* a_cpos,
                                           const double* a_w,
                                           const double* wdinv)
{
  for (int kk = 0; kk < nb; ++kk) {
    const int32_t kpos = row.cpos(kk);
    const double m = row.get(kk) * wdinv[kpos];
    const int64_t e1 = a_ptr[kpos + 1];
    for (int64_t e = a_ptr[kpos] + lane; e < e1; e += 64) {
      const int32_t jpos = a_cpos[e];
      int lo = kk + 1, hi = tot; // after~(k) lies behind k
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row.cpos(mid) < jpos)
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo < tot && row.cpos(lo) == jpos)
        row.set(lo, row.get(lo) - m * a_w[e]);
    }
    wave_step();
  }
}

// Rows pos0 .. pos1 - 1 (one colour), one wavefront each.
__global__ __launch_bounds__(kBlock) void ilu0_factor_kernel(
    int32_t pos0, int32_t pos1, const int64_t* __restrict__ b_ptr,
    const int32_t* __restrict__ b_cpos, double* b_w,
    const int64_t* __restrict__ a_ptr, const int32_t* __restrict__ a_cpos,
    double* a_w, double* wd, double* wdinv)
{
  __shared__ double s_w[kWaves][kSlab];
  __shared__ int32_t s_c[kWaves][kSlab];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // (a colour of 2^24 rows and more does not fit one grid dimension: see the launch)
  const int64_t block = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t p64 = (int64_t)pos0 + block * kWaves + wave;
  if (p64 >= pos1)
    return;
  const int32_t pos = (int32_t)p64;
  const int64_t b0 = b_ptr[pos], a0 = a_ptr[pos];
  const int64_t nb64 = b_ptr[pos + 1] - b0, na64 = a_ptr[pos + 1] - a0;
  const int nb = (int)nb64;
  const int64_t tot64 = nb64 + 1 + na64;
  const GlobalRow g{b_w + b0, wd + pos, a_w + a0, b_cpos + b0, a_cpos + a0, nb, pos};
  if (tot64 <= kSlab) {
    const int tot = (int)tot64;
    const LdsRow l{s_w[wave], s_c[wave]};
    for (int i = lane; i < tot; i += 64) {
      l.w[i] = g.get(i);
      l.c[i] = g.cpos(i);
    }
    wave_step();
    factor_row(l, nb, tot, lane, a_ptr, a_cpos, a_w, wdinv);
    for (int i = lane; i < tot; i += 64)
      g.set(i, l.w[i]);
    if (lane == 0)
      wdinv[pos] = 1.0 / l.w[nb];
  } else {
    // (a list beyond 2^31 entries cannot occur: positions are int32 and distinct)
    factor_row(g, nb, (int)tot64, lane, a_ptr, a_cpos, a_w, wdinv);
    if (lane == 0)
      wdinv[pos] = 1.0 / *g.d;
  }
}

__global__ __launch_bounds__(kBlock) void ilu0_finish_kernel(
    int32_t n, const int32_t* __restrict__ perm, const double* __restrict__ wd,
    const double* __restrict__ wdinv, double* __restrict__ dinv,
    unsigned* counts)
{
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  // (every lane of a wavefront makes the same number of rounds)
  const int64_t rounds = ((int64_t)n + stride - 1) / stride;
  for (int64_t r = 0; r < rounds; ++r) {
    const int64_t p = r * stride + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool bad = false, neg = false;
    if (p < n) {
      const double d = wd[p];
      dinv[perm[p]] = wdinv[p];
      const bool finite = d - d == 0.0;
      bad = !finite || d == 0.0;
      neg = finite && d < 0.0;
    }
    const unsigned nbad = (unsigned)__popcll(__ballot(bad));
    const unsigned nneg = (unsigned)__popcll(__ballot(neg));
    if (lane == 0) {
      if (nbad)
        atomicAdd(counts, nbad);
      if (nneg)
        atomicAdd(counts + 1, nneg);
    }
  }
}

__global__ __launch_bounds__(kBlock) void ilu0_scatter_kernel(
    int64_t count, const int64_t* __restrict__ slot,
    const double* __restrict__ w, double* __restrict__ val,
    double* __restrict__ long_val)
{
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < count;
       e += stride) {
    const int64_t s = slot[e];
    if (s >= 0)
      val[s] = w[e];
    else
      long_val[~s] = w[e];
  }
}

// ... into a sweep plan that keeps floats: every value rounded to nearest-even
// as it is written; counts[2] += the values out of fp32's range (fp32_range.h),
// one add per wavefront that met any
__global__ __launch_bounds__(kBlock) void ilu0_scatter_narrow_kernel(
    int64_t count, const int64_t* __restrict__ slot,
    const double* __restrict__ w, float* __restrict__ val,
    float* __restrict__ long_val, unsigned* counts)
{
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  // (every lane of a wavefront makes the same number of rounds)
  const int64_t rounds = (count + stride - 1) / stride;
  for (int64_t k = 0; k < rounds; ++k) {
    const int64_t e = k * stride + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool mine = false;
    if (e < count) {
      const double v = w[e];
      const int64_t s = slot[e];
      if (s >= 0)
        val[s] = (float)v;
      else
        long_val[~s] = (float)v;
      mine = spmv_fp32_out_of_range(v);
    }
    const unsigned nbad = (unsigned)__popcll(__ballot(mine));
    if ((threadIdx.x & 63) == 0 && nbad)
      atomicAdd(counts + 2, nbad);
  }
}

template <typename T>
int upload(const T* host, size_t count, T** dev, int64_t* bytes)
{
  *dev = nullptr;
  if (count == 0)
    return SPMV_HIP_OK;
  SPMV_REQUIRE(host != nullptr);
  SPMV_CHECK_HIP(spmv_plan_malloc(dev, count * sizeof(T)));
  *bytes += (int64_t)(count * sizeof(T));
  SPMV_CHECK_HIP(hipMemcpy(*dev, host, count * sizeof(T), hipMemcpyHostToDevice));
  return SPMV_HIP_OK;
}

template <typename T>
int reserve(size_t count, T** dev, int64_t* bytes)
{
  *dev = nullptr;
  if (count == 0)
    return SPMV_HIP_OK;
  SPMV_CHECK_HIP(spmv_plan_malloc(dev, count * sizeof(T)));
  *bytes += (int64_t)(count * sizeof(T));
  return SPMV_HIP_OK;
}

// Everything a kernel will index with is checked here, once, on the host.
bool part_is_sound(const spmv_hip_ilu0_host& in, const spmv_hip_ilu0_part& p,
                   const spmv_hip_mcgs_part& sliced, bool is_before)
{
  const spmv_hip_mcgs_host& m = in.mcgs;
  const int32_t n = m.num_rows, C = m.num_colors;
  if (n == 0)
    return true;
  if (!p.ptr || p.ptr[0] != 0)
    return false;
  for (int32_t pos = 0; pos < n; ++pos)
    if (p.ptr[pos + 1] < p.ptr[pos])
      return false;
  const int64_t count = p.ptr[n];
  if (count > 0 && (!p.cpos || !p.src || !p.slot))
    return false;
  const int64_t nval = sliced.slice_ptr[sliced.color_slice[C]];
  const int64_t nlong = sliced.long_ptr[sliced.color_long[C]];
  for (int c = 0; c < C; ++c) {
    const int32_t c0 = m.color_start[c], c1 = m.color_start[c + 1];
    for (int32_t pos = c0; pos < c1; ++pos)
      for (int64_t e = p.ptr[pos]; e < p.ptr[pos + 1]; ++e) {
        const int32_t q = p.cpos[e];
        // the column wears a smaller / larger colour; ascending in the row
        if (is_before ? (q < 0 || q >= c0) : (q < c1 || q >= n))
          return false;
        if (e > p.ptr[pos] && q <= p.cpos[e - 1])
          return false;
        if (p.src[e] < 0 || p.src[e] >= in.num_values)
          return false;
        const int64_t s = p.slot[e];
        if (s >= 0 ? s >= nval : ~s >= nlong)
          return false;
      }
  }
  return true;
}

int upload_part(int32_t n, const spmv_hip_ilu0_part& p, Ilu0PartDev* d,
                int64_t* bytes)
{
  d->count = n > 0 ? p.ptr[n] : 0;
  const size_t cnt = (size_t)d->count;
  int rc;
  if ((rc = upload(p.ptr, n > 0 ? (size_t)n + 1 : 0, &d->ptr, bytes)) != SPMV_HIP_OK
      || (rc = upload(p.cpos, cnt, &d->cpos, bytes)) != SPMV_HIP_OK
      || (rc = upload(p.src, cnt, &d->src, bytes)) != SPMV_HIP_OK
      || (rc = upload(p.slot, cnt, &d->slot, bytes)) != SPMV_HIP_OK
      || (rc = reserve(cnt, &d->w, bytes)) != SPMV_HIP_OK)
    return rc;
  return SPMV_HIP_OK;
}

void free_part(Ilu0PartDev* d)
{
  plan_drop(d->ptr);
  plan_drop(d->cpos);
  plan_drop(d->src);
  plan_drop(d->slot);
  plan_drop(d->w);
}

} // namespace

extern "C" {

int spmv_hip_ilu0_plan_create(spmv_hip_ctx* ctx, const spmv_hip_ilu0_host* in,
                              spmv_hip_ilu0_plan** plan)
{
  SPMV_REQUIRE(ctx && in && plan);
  *plan = nullptr;
  SPMV_REQUIRE(in->num_values >= 0);
  // the sweep plan first: it checks the colours, perm and the sliced layout
  spmv_hip_mcgs_plan* inner = nullptr;
  const int rc0 = spmv_hip_mcgs_plan_create(ctx, &in->mcgs, &inner);
  if (rc0 != SPMV_HIP_OK)
    return rc0;
  spmv_hip_ilu0_plan* p = new (std::nothrow) spmv_hip_ilu0_plan();
  if (!p) {
    spmv_hip_mcgs_plan_destroy(inner);
    return SPMV_HIP_EINVAL;
  }
  p->ctx = ctx;
  p->inner = inner;
  p->n = in->mcgs.num_rows;
  p->num_values = in->num_values;
  const size_t n = (size_t)p->n;
  int rc = SPMV_HIP_OK;
  if (!part_is_sound(*in, in->before, in->mcgs.before, true)
      || !part_is_sound(*in, in->after, in->mcgs.after, false))
    rc = SPMV_HIP_EINVAL;
  if (rc != SPMV_HIP_OK
      || (rc = upload_part(p->n, in->before, &p->before, &p->bytes)) != SPMV_HIP_OK
      || (rc = upload_part(p->n, in->after, &p->after, &p->bytes)) != SPMV_HIP_OK
      || (rc = reserve(n, &p->wd, &p->bytes)) != SPMV_HIP_OK
      || (rc = reserve(n, &p->wdinv, &p->bytes)) != SPMV_HIP_OK
      || (rc = reserve((size_t)4, &p->counts, &p->bytes)) != SPMV_HIP_OK) {
    spmv_hip_ilu0_plan_destroy(p);
    return rc;
  }
  *plan = p;
  return SPMV_HIP_OK;
}

int spmv_hip_ilu0_plan_create_ex(spmv_hip_ctx* ctx, const spmv_hip_ilu0_host* in,
                                 int value_bits, spmv_hip_ilu0_plan** plan)
{
  SPMV_REQUIRE(plan != nullptr);
  *plan = nullptr;
  SPMV_REQUIRE(value_bits == 64 || value_bits == 32);
  spmv_hip_ilu0_plan* p = nullptr;
  int rc = spmv_hip_ilu0_plan_create(ctx, in, &p);
  if (rc == SPMV_HIP_OK && value_bits == 32) {
    // the placeholders in the form the factorisation will write
    int64_t none = 0;
    rc = mcgs_plan_narrow(p->inner, ctx->stream, &none);
    if (rc != SPMV_HIP_OK) {
      spmv_hip_ilu0_plan_destroy(p);
      return rc;
    }
  }
  *plan = p;
  return rc;
}

int spmv_hip_ilu0_plan_destroy(spmv_hip_ilu0_plan* plan)
{
  if (!plan)
    return SPMV_HIP_OK;
  (void)hipSetDevice(plan->ctx->device);
  free_part(&plan->before);
  free_part(&plan->after);
  plan_drop(plan->wd);
  plan_drop(plan->wdinv);
  plan_drop(plan->counts);
  spmv_hip_mcgs_plan_destroy(plan->inner);
  delete plan;
  return SPMV_HIP_OK;
}

int spmv_hip_ilu0_plan_bytes(const spmv_hip_ilu0_plan* plan, int64_t* bytes)
{
  SPMV_REQUIRE(plan && bytes);
  *bytes = plan->bytes + plan->inner->bytes;
  return SPMV_HIP_OK;
}

int spmv_hip_ilu0_plan_sizes(const spmv_hip_ilu0_plan* plan, int64_t* sizes)
{
  SPMV_REQUIRE(plan && sizes);
  sizes[0] = plan->n;
  sizes[1] = plan->before.count;
  sizes[2] = plan->after.count;
  sizes[3] = plan->bytes;
  return SPMV_HIP_OK;
}

int spmv_hip_ilu0_plan_export(const spmv_hip_ilu0_plan* plan,
                              const spmv_hip_ilu0_export* before,
                              const spmv_hip_ilu0_export* after)
{
  SPMV_REQUIRE(plan != nullptr);
  SPMV_SET_DEVICE(plan->ctx);
  SPMV_CHECK_HIP(hipStreamSynchronize(plan->ctx->stream));
  auto fetch = [](void* dst, const void* src, size_t bytes) {
    return dst && bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)
                        : hipSuccess;
  };
  const size_t n1 = plan->n > 0 ? (size_t)plan->n + 1 : 0;
  const Ilu0PartDev* parts[2] = {&plan->before, &plan->after};
  const spmv_hip_ilu0_export* outs[2] = {before, after};
  for (int h = 0; h < 2; ++h) {
    const spmv_hip_ilu0_export* o = outs[h];
    if (!o)
      continue;
    const size_t cnt = (size_t)parts[h]->count;
    SPMV_CHECK_HIP(fetch(o->ptr, parts[h]->ptr, n1 * 8));
    SPMV_CHECK_HIP(fetch(o->cpos, parts[h]->cpos, cnt * 4));
    SPMV_CHECK_HIP(fetch(o->src, parts[h]->src, cnt * 4));
    SPMV_CHECK_HIP(fetch(o->slot, parts[h]->slot, cnt * 8));
  }
  return SPMV_HIP_OK;
}

int spmv_hip_ilu0_mcgs_plan(const spmv_hip_ilu0_plan* plan,
                            spmv_hip_mcgs_plan** inner)
{
  SPMV_REQUIRE(plan && inner);
  *inner = plan->inner;
  return SPMV_HIP_OK;
}

int spmv_hip_ilu0_factor(spmv_hip_ctx* ctx, spmv_hip_ilu0_plan* plan,
                         const double* values, const double* diagonal,
                         void* stream)
{
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx);
  const int32_t n = plan->n;
  SPMV_REQUIRE(n == 0 || diagonal);
  SPMV_REQUIRE(plan->before.count + plan->after.count == 0 || values);
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  SPMV_CHECK_HIP(hipMemsetAsync(plan->counts, 0, 16, st));
  if (n == 0)
    return SPMV_HIP_OK;
  spmv_hip_mcgs_plan* in = plan->inner;
  Ilu0PartDev& b = plan->before;
  Ilu0PartDev& a = plan->after;
  for (Ilu0PartDev* part : {&b, &a})
    if (part->count > 0)
      hipLaunchKernelGGL(ilu0_gather_kernel,
                         dim3(spmv_grid_for(ctx, part->count, kBlock)),
                         dim3(kBlock), 0, st, part->count, part->src, values,
                         part->w);
  const int rows_grid = spmv_grid_for(ctx, n, kBlock);
  hipLaunchKernelGGL(ilu0_diag_kernel, dim3(rows_grid), dim3(kBlock), 0, st, n,
                     in->perm, diagonal, plan->wd, plan->wdinv);
  for (int c = 1; c < in->num_colors; ++c) {
    const int32_t p0 = in->color_start[c], p1 = in->color_start[c + 1];
    if (p1 <= p0) // (mcgs_plan_create refuses a colour nobody wears)
      continue;
    // one wavefront per row: grid.x * kBlock must stay below 2^32, which a
    // colour of the 512^3 Poisson matrix (2^26 rows) exceeds; the blocks beyond
    // kMaxGridX go to grid.y (at most 2^31 / kWaves / kMaxGridX = 512 of them)
    const int64_t blocks = ((int64_t)p1 - p0 + kWaves - 1) / kWaves;
    const int64_t gx = blocks < kMaxGridX ? blocks : kMaxGridX;
    const int64_t gy = (blocks + gx - 1) / gx;
    hipLaunchKernelGGL(ilu0_factor_kernel, dim3((unsigned)gx, (unsigned)gy),
                       dim3(kBlock), 0, st, p0,
                       p1, b.ptr, b.cpos, b.w, a.ptr, a.cpos, a.w, plan->wd,
                       plan->wdinv);
  }
  hipLaunchKernelGGL(ilu0_finish_kernel, dim3(rows_grid), dim3(kBlock), 0, st, n,
                     in->perm, plan->wd, plan->wdinv, in->dinv, plan->counts);
  McgsPartDev* sweep[2] = {&in->before, &in->after};
  Ilu0PartDev* part[2] = {&b, &a};
  for (int h = 0; h < 2; ++h) {
    if (part[h]->count == 0)
      continue;
    const dim3 grid(spmv_grid_for(ctx, part[h]->count, kBlock));
    if (in->value_bits == 32)
      hipLaunchKernelGGL(ilu0_scatter_narrow_kernel, grid, dim3(kBlock), 0, st,
                         part[h]->count, part[h]->slot, part[h]->w,
                         sweep[h]->val32, sweep[h]->long_val32, plan->counts);
    else
      hipLaunchKernelGGL(ilu0_scatter_kernel, grid, dim3(kBlock), 0, st,
                         part[h]->count, part[h]->slot, part[h]->w, sweep[h]->val,
                         sweep[h]->long_val);
  }
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_ilu0_pivots(spmv_hip_ctx* ctx, const spmv_hip_ilu0_plan* plan,
                         int64_t* not_usable, int64_t* negative, void* stream)
{
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx && not_usable && negative);
  SPMV_SET_DEVICE(ctx);
  unsigned host[2] = {0, 0};
  SPMV_CHECK_HIP(plan_fetch(host, plan->counts, 2, spmv_stream(ctx, stream)));
  *not_usable = host[0];
  *negative = host[1];
  return SPMV_HIP_OK;
}

int spmv_hip_ilu0_counts(spmv_hip_ctx* ctx, const spmv_hip_ilu0_plan* plan,
                         int64_t* not_usable, int64_t* negative,
                         int64_t* out_of_range, void* stream)
{
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx && not_usable && negative
               && out_of_range);
  SPMV_SET_DEVICE(ctx);
  unsigned host[3] = {0, 0, 0};
  SPMV_CHECK_HIP(plan_fetch(host, plan->counts, 3, spmv_stream(ctx, stream)));
  *not_usable = host[0];
  *negative = host[1];
  *out_of_range = host[2];
  return SPMV_HIP_OK;
}

int spmv_hip_ilu0_get_pattern(spmv_hip_ctx* ctx, const spmv_hip_ilu0_plan* plan,
                              int64_t* before_ptr, int32_t* before_cpos,
                              int64_t* after_ptr, int32_t* after_cpos)
{
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx);
  SPMV_SET_DEVICE(ctx);
  const size_t n1 = plan->n > 0 ? (size_t)plan->n + 1 : 0;
  auto fetch = [](void* dst, const void* src, size_t bytes) {
    return dst && bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)
                        : hipSuccess;
  };
  SPMV_CHECK_HIP(fetch(before_ptr, plan->before.ptr, n1 * 8));
  SPMV_CHECK_HIP(fetch(after_ptr, plan->after.ptr, n1 * 8));
  SPMV_CHECK_HIP(fetch(before_cpos, plan->before.cpos, (size_t)plan->before.count * 4));
  SPMV_CHECK_HIP(fetch(after_cpos, plan->after.cpos, (size_t)plan->after.count * 4));
  return SPMV_HIP_OK;
}

int spmv_hip_ilu0_get_factor(spmv_hip_ctx* ctx, const spmv_hip_ilu0_plan* plan,
                             double* l, double* u, double* d, void* stream)
{
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx);
  SPMV_SET_DEVICE(ctx);
  SPMV_CHECK_HIP(hipStreamSynchronize(spmv_stream(ctx, stream)));
  auto fetch = [](void* dst, const void* src, size_t bytes) {
    return dst && bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)
                        : hipSuccess;
  };
  SPMV_CHECK_HIP(fetch(l, plan->before.w, (size_t)plan->before.count * 8));
  SPMV_CHECK_HIP(fetch(u, plan->after.w, (size_t)plan->after.count * 8));
  SPMV_CHECK_HIP(fetch(d, plan->wd, (size_t)plan->n * 8));
  return SPMV_HIP_OK;
}

} // extern "C"
