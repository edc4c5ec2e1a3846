// Multicolour symmetric Gauss-Seidel sweeps (gfx950): the application of
// spmv::SgsPreconditioner, z = M^-1 r with M = (D + L) D^-1 (D + U) in the
// colour-major ordering of the rows of the local diagonal block.
//
//   forward,  colours 0 .. C-1:   s = 0; for e in before(i): s = s + a_e * z[col_e]
//                                 z_i = (r_i - s) * dinv_i
//   backward, colours C-2 .. 0:   t = 0; for e in after(i):  t = t + a_e * z[col_e]
//                                 z_i = z_i - dinv_i * t
//
// before(i) / after(i): the off-diagonal entries of row i whose column wears a
// smaller / larger colour, ascending by column.  One launch per colour and
// direction, 2C - 1 in all; the order between colours is the stream's order and
// nothing else -- no kernel here waits on another workgroup.  Inside a launch
// no row reads what another row of the launch writes: a row of colour c reads
// z only at columns of other colours.
//
// Layout (host/sgs_build.h, SgsSlicedPart): the rows of a colour in slices of
// 64 consecutive positions, a slice column-major, one lane per row, so a
// wavefront's loads of values and columns are contiguous.  A row with more than
// 64 entries in a part takes a wavefront of its own from the long list: 64
// entries are loaded and multiplied at a time, then added in their order, one
// lane's product after the other, so the sum has the bits of the sequential
// loop above.  The long rows of a colour are served by extra wavefronts of the
// same launch.
//
// The block form (mcgs_sweep_block_kernel, spmv_hip_mcgs_apply_block_f64) runs
// the same sweeps on nrhs INTERLEAVED vectors, element (i, c) at V[i * nrhs +
// c], on the same plan: a lane loads val[e] and col[e] once per entry, gathers
// the nrhs contiguous doubles of z at that column and keeps nrhs sums, each
// added in the entries' order -- column c has the bits of the single-vector
// sweep on column c.  Inside a launch a row of colour c writes only its own
// nrhs elements of Z and reads Z only at rows of other colours, so the in-place
// update has no hazard here either.  nrhs = 2, 4, 8 are compiled widths with
// 16-byte gathers and stores where R and Z are 16-byte aligned (a row of the
// block is then 16-byte aligned too) and the scalar form of the same kernel
// where they are not; one instantiation with nrhs at run time serves 1, 3, 5,
// 6 and 7.
//
// fp32 values (SgsOptions::values = fp32, value_bits 32).  A plan may keep val
// and long_val of both parts as float, each the fp64 value rounded to
// nearest-even: a sweep then streams 8 bytes per stored entry, not 12.  Both
// kernels are templates on the stored type and compute acc = acc + (double)v32
// * z[col] -- the widening is exact, so the result has the bits of the fp64
// sweep on the widened values; dinv, r, z and the sums stay fp64.  A value load
// of a slice column is 256 contiguous bytes of a wavefront, one load per k.
// The plan is narrowed after either builder has made the fp64 plan
// (mcgs_plan_narrow: per array allocate, round, free), the values out of
// fp32's range (fp32_range.h) counted in the same kernel.  The fp64 arrays are
// not kept:
//   plan_bytes(fp32) = plan_bytes(fp64) - 4 * (E_before + E_after
//                                              + L_before + L_after)
// E: the sliced entries of a part, padding included (slice_ptr's last), L: its
// long entries (long_ptr's last).
//
// Built with -ffp-contract=off: every product and sum is a rounding of its own.
#include "common.h"
#include "pcg_ws.h"
#include "pcgb_ws.h"

#include <vector>

#include "fp32_range.h"
#include "mcgs_plan.h"
#include "plan_scratch.h"

namespace
{

constexpr int kWaves = kBlock / 64;

// One colour, one direction.  Wavefront w of the launch: slice first_slice + w
// while w < num_slices, then long row first_long + (w - num_slices).
// V: the stored value type, double or float (value_bits 64 / 32); a float is
// widened before its product, exactly: the sum has the bits of the fp64 sweep
// on the widened values.
template <typename V, bool FORWARD>
__global__ __launch_bounds__(kBlock) void mcgs_sweep_kernel(
    int32_t first_slice, int32_t num_slices, int32_t pos_end,
    int32_t first_long, int32_t num_long,
    const int32_t* __restrict__ slice_pos0,
    const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ len,
    const int32_t* __restrict__ col, const V* __restrict__ val,
    const int32_t* __restrict__ long_pos, const int64_t* __restrict__ long_ptr,
    const int32_t* __restrict__ long_col, const V* __restrict__ long_val,
    const int32_t* __restrict__ perm, const double* __restrict__ dinv,
    const double* __restrict__ r, double* z, const PcgScalars* __restrict__ sc)
{
  if (sc && sc->done)
    return;
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (w < num_slices) {
    const int64_t s = first_slice + w;
    const int32_t pos = slice_pos0[s] + lane;
    if (pos >= pos_end)
      return;
    const int32_t m = len[pos];
    if (m < 0) // a long row: another wavefront's
      return;
    const int64_t base = slice_ptr[s] + lane;
    double acc = 0.0;
#pragma unroll 4
    for (int32_t k = 0; k < m; ++k) {
      const int64_t e = base + (int64_t)k * 64;
      acc = acc + (double)val[e] * z[col[e]];
    }
    const int32_t i = perm[pos];
    if constexpr (FORWARD)
      z[i] = (r[i] - acc) * dinv[i];
    else
      z[i] = z[i] - dinv[i] * acc;
    return;
  }
  const int64_t l = w - num_slices;
  if (l >= num_long)
    return;
  const int32_t pos = long_pos[first_long + l];
  const int64_t e0 = long_ptr[first_long + l], e1 = long_ptr[first_long + l + 1];
  double acc = 0.0;
  for (int64_t e = e0; e < e1; e += 64) {
    const int64_t mine = e + lane;
    const double prod
        = mine < e1 ? (double)long_val[mine] * z[long_col[mine]] : 0.0;
    const int cnt = e1 - e < 64 ? (int)(e1 - e) : 64;
    for (int j = 0; j < cnt; ++j) // in the entries' order, every lane the same
      acc = acc + __shfl(prod, j, 64);
  }
  if (lane == 0) {
    const int32_t i = perm[pos];
    if constexpr (FORWARD)
      z[i] = (r[i] - acc) * dinv[i];
    else
      z[i] = z[i] - dinv[i] * acc;
  }
}

// ---- the block form -----------------------------------------------------------
typedef double f64x2 __attribute__((ext_vector_type(2)));

// the KM slots of row i of a block: VEC 16 bytes at a time (KM == nrhs, even),
// else one double at a time, slots c >= nrhs left at zero
template <bool VEC, int KM>
__device__ __forceinline__ void block_load(const double* v, int64_t i, int nrhs,
                                           double (&out)[KM])
{
  const double* q = v + i * nrhs;
#pragma unroll
  for (int c = 0; c < KM; c += VEC ? 2 : 1) {
    if constexpr (VEC) {
      const f64x2 t = *reinterpret_cast<const f64x2*>(q + c);
      out[c] = t.x;
      out[c + 1] = t.y;
    } else {
      out[c] = c < nrhs ? q[c] : 0.0;
    }
  }
}

template <bool VEC, int KM>
__device__ __forceinline__ void block_store(double* v, int64_t i, int nrhs,
                                            const double (&in)[KM])
{
  double* q = v + i * nrhs;
#pragma unroll
  for (int c = 0; c < KM; c += VEC ? 2 : 1) {
    if constexpr (VEC) {
      f64x2 t;
      t.x = in[c];
      t.y = in[c + 1];
      *reinterpret_cast<f64x2*>(q + c) = t;
    } else {
      if (c < nrhs)
        q[c] = in[c];
    }
  }
}

// z(i, :) from the sums of row i, as mcgs_sweep_kernel does for one vector
template <bool VEC, bool FORWARD, int KM>
__device__ __forceinline__ void block_finish(int64_t i, int nrhs, double d,
                                             const double (&acc)[KM],
                                             const double* r, double* z)
{
  double out[KM];
  block_load<VEC, KM>(FORWARD ? r : z, i, nrhs, out);
#pragma unroll
  for (int c = 0; c < KM; ++c) {
    if constexpr (FORWARD)
      out[c] = (out[c] - acc[c]) * d;
    else
      out[c] = out[c] - d * acc[c];
  }
  block_store<VEC, KM>(z, i, nrhs, out);
}

// One colour, one direction, nrhs interleaved vectors; the wavefronts are
// mcgs_sweep_kernel's.  K = 2, 4, 8: the width at compile time (VEC: 16-byte
// accesses); K = 0: nrhs at run time, 1..8.  Every index of an accumulator is
// a constant after unrolling: they stay in registers.
template <typename V, int K, bool VEC, bool FORWARD>
__global__ __launch_bounds__(kBlock) void mcgs_sweep_block_kernel(
    int32_t first_slice, int32_t num_slices, int32_t pos_end,
    int32_t first_long, int32_t num_long,
    const int32_t* __restrict__ slice_pos0,
    const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ len,
    const int32_t* __restrict__ col, const V* __restrict__ val,
    const int32_t* __restrict__ long_pos, const int64_t* __restrict__ long_ptr,
    const int32_t* __restrict__ long_col, const V* __restrict__ long_val,
    const int32_t* __restrict__ perm, const double* __restrict__ dinv,
    int nrhs_rt, const double* __restrict__ r, double* z,
    const CgbState* __restrict__ st)
{
  constexpr int KM = K ? K : SPMV_CGB_MAX;
  static_assert(!VEC || K != 0, "16-byte accesses need a compiled width");
  const int nrhs = K ? K : nrhs_rt;
  if (st && st->all_done)
    return;
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (w < num_slices) {
    const int64_t s = first_slice + w;
    const int32_t pos = slice_pos0[s] + lane;
    if (pos >= pos_end)
      return;
    const int32_t m = len[pos];
    if (m < 0) // a long row: another wavefront's
      return;
    const int64_t base = slice_ptr[s] + lane;
    double acc[KM] = {};
#pragma unroll 2
    for (int32_t k = 0; k < m; ++k) {
      const int64_t e = base + (int64_t)k * 64;
      const double a = (double)val[e];
      double zv[KM];
      block_load<VEC, KM>(z, col[e], nrhs, zv);
#pragma unroll
      for (int c = 0; c < KM; ++c)
        acc[c] = acc[c] + a * zv[c];
    }
    const int32_t i = perm[pos];
    block_finish<VEC, FORWARD, KM>(i, nrhs, dinv[i], acc, r, z);
    return;
  }
  const int64_t l = w - num_slices;
  if (l >= num_long)
    return;
  const int32_t pos = long_pos[first_long + l];
  const int64_t e0 = long_ptr[first_long + l], e1 = long_ptr[first_long + l + 1];
  double acc[KM] = {};
  for (int64_t e = e0; e < e1; e += 64) {
    const int64_t mine = e + lane;
    double prod[KM] = {};
    if (mine < e1) {
      const double a = (double)long_val[mine];
      double zv[KM];
      block_load<VEC, KM>(z, long_col[mine], nrhs, zv);
#pragma unroll
      for (int c = 0; c < KM; ++c)
        prod[c] = a * zv[c];
    }
    const int cnt = e1 - e < 64 ? (int)(e1 - e) : 64;
    for (int j = 0; j < cnt; ++j) { // in the entries' order, every lane the same
#pragma unroll
      for (int c = 0; c < KM; ++c)
        if (c < nrhs)
          acc[c] = acc[c] + __shfl(prod[c], j, 64);
    }
  }
  if (lane == 0) {
    const int32_t i = perm[pos];
    block_finish<VEC, FORWARD, KM>(i, nrhs, dinv[i], acc, r, z);
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

// Everything a kernel will index with is checked here, once, on the host.
bool part_is_sound(const spmv_hip_mcgs_host& in, const spmv_hip_mcgs_part& p)
{
  const int32_t n = in.num_rows, C = in.num_colors;
  if (!p.color_slice || !p.color_long || !p.slice_ptr || !p.long_ptr)
    return false;
  if (p.color_slice[0] != 0 || p.color_long[0] != 0 || p.slice_ptr[0] != 0
      || p.long_ptr[0] != 0)
    return false;
  for (int c = 0; c < C; ++c)
    if (p.color_slice[c + 1] < p.color_slice[c]
        || p.color_long[c + 1] < p.color_long[c])
      return false;
  const int32_t ns = p.color_slice[C], nl = p.color_long[C];
  if ((ns > 0 && !p.slice_pos0) || (n > 0 && !p.len) || (nl > 0 && !p.long_pos))
    return false;
  for (int c = 0; c < C; ++c) {
    const int32_t c0 = in.color_start[c], c1 = in.color_start[c + 1];
    // the slices of a colour tile its positions
    if ((int64_t)p.color_slice[c + 1] - p.color_slice[c]
        != ((int64_t)c1 - c0 + 63) / 64)
      return false;
    for (int32_t s = p.color_slice[c]; s < p.color_slice[c + 1]; ++s) {
      if (p.slice_pos0[s] != c0 + 64 * (s - p.color_slice[c]))
        return false;
      const int64_t span = p.slice_ptr[s + 1] - p.slice_ptr[s];
      if (span < 0 || span % 64 != 0)
        return false;
      const int32_t p1 = p.slice_pos0[s] + 64 < c1 ? p.slice_pos0[s] + 64 : c1;
      for (int32_t pos = p.slice_pos0[s]; pos < p1; ++pos)
        if (p.len[pos] > span / 64)
          return false;
    }
    for (int32_t l = p.color_long[c]; l < p.color_long[c + 1]; ++l)
      if (p.long_pos[l] < c0 || p.long_pos[l] >= c1 || p.len[p.long_pos[l]] >= 0
          || p.long_ptr[l + 1] < p.long_ptr[l])
        return false;
  }
  const int64_t ne = p.slice_ptr[ns], nle = p.long_ptr[nl];
  if ((ne > 0 && (!p.col || !p.val)) || (nle > 0 && (!p.long_col || !p.long_val)))
    return false;
  for (int64_t e = 0; e < ne; ++e)
    if (p.col[e] < 0 || p.col[e] >= n)
      return false;
  for (int64_t e = 0; e < nle; ++e)
    if (p.long_col[e] < 0 || p.long_col[e] >= n)
      return false;
  return true;
}

int upload_part(const spmv_hip_mcgs_host& in, const spmv_hip_mcgs_part& p,
                McgsPartDev* d, int64_t* bytes)
{
  const int32_t C = in.num_colors;
  const size_t ns = (size_t)p.color_slice[C], nl = (size_t)p.color_long[C];
  d->color_slice.assign(p.color_slice, p.color_slice + C + 1);
  d->color_long.assign(p.color_long, p.color_long + C + 1);
  int rc;
  if ((rc = upload(p.slice_pos0, ns, &d->slice_pos0, bytes)) != SPMV_HIP_OK
      || (rc = upload(p.slice_ptr, ns + 1, &d->slice_ptr, bytes)) != SPMV_HIP_OK
      || (rc = upload(p.len, (size_t)in.num_rows, &d->len, bytes)) != SPMV_HIP_OK
      || (rc = upload(p.col, (size_t)p.slice_ptr[ns], &d->col, bytes))
             != SPMV_HIP_OK
      || (rc = upload(p.val, (size_t)p.slice_ptr[ns], &d->val, bytes))
             != SPMV_HIP_OK
      || (rc = upload(p.long_pos, nl, &d->long_pos, bytes)) != SPMV_HIP_OK
      || (rc = upload(p.long_ptr, nl + 1, &d->long_ptr, bytes)) != SPMV_HIP_OK
      || (rc = upload(p.long_col, (size_t)p.long_ptr[nl], &d->long_col, bytes))
             != SPMV_HIP_OK
      || (rc = upload(p.long_val, (size_t)p.long_ptr[nl], &d->long_val, bytes))
             != SPMV_HIP_OK)
    return rc;
  return SPMV_HIP_OK;
}

void free_part(McgsPartDev* d)
{
  for (void* q : {(void*)d->slice_pos0, (void*)d->slice_ptr, (void*)d->len,
                  (void*)d->col, (void*)d->val, (void*)d->val32,
                  (void*)d->long_pos, (void*)d->long_ptr, (void*)d->long_col,
                  (void*)d->long_val, (void*)d->long_val32})
    if (q)
      (void)spmv_plan_free(q);
}

// the value arrays of a part in the form V
template <typename V>
struct PartValues;
template <>
struct PartValues<double> {
  static const double* val(const McgsPartDev& p) { return p.val; }
  static const double* long_val(const McgsPartDev& p) { return p.long_val; }
};
template <>
struct PartValues<float> {
  static const float* val(const McgsPartDev& p) { return p.val32; }
  static const float* long_val(const McgsPartDev& p) { return p.long_val32; }
};

// out[e] = in[e] rounded to nearest-even; *bad += the values out of fp32's
// range (fp32_range.h), one add per wavefront that met any
__global__ __launch_bounds__(kBlock) void mcgs_narrow_kernel(
    int64_t count, const double* __restrict__ in, float* __restrict__ out,
    unsigned long long* __restrict__ bad)
{
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  // (every lane of a wavefront makes the same number of rounds)
  const int64_t rounds = (count + stride - 1) / stride;
  for (int64_t k = 0; k < rounds; ++k) {
    const int64_t e = k * stride + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool mine = false;
    if (e < count) {
      const double v = in[e];
      out[e] = (float)v;
      mine = spmv_fp32_out_of_range(v);
    }
    const unsigned long long nbad
        = (unsigned long long)__popcll(__ballot(mine));
    if ((threadIdx.x & 63) == 0 && nbad)
      atomicAdd(bad, nbad);
  }
}

template <typename V, bool FORWARD>
void launch_colour(const spmv_hip_mcgs_plan* plan, const McgsPartDev& p, int c,
                   const double* r, double* z, const PcgScalars* sc,
                   hipStream_t st)
{
  const int32_t ns = p.color_slice[c + 1] - p.color_slice[c];
  const int32_t nl = p.color_long[c + 1] - p.color_long[c];
  const int64_t waves = (int64_t)ns + nl;
  if (waves == 0)
    return;
  const unsigned grid = (unsigned)((waves + kWaves - 1) / kWaves);
  hipLaunchKernelGGL((mcgs_sweep_kernel<V, FORWARD>), dim3(grid), dim3(kBlock), 0,
                     st, p.color_slice[c], ns, plan->color_start[c + 1],
                     p.color_long[c], nl, p.slice_pos0, p.slice_ptr, p.len,
                     p.col, PartValues<V>::val(p), p.long_pos, p.long_ptr,
                     p.long_col, PartValues<V>::long_val(p), plan->perm,
                     plan->dinv, r, z, sc);
}

// the 2C - 1 launches of one application
template <typename V>
void apply_single(const spmv_hip_mcgs_plan* plan, const double* r, double* z,
                  const PcgScalars* sc, hipStream_t st)
{
  const int C = plan->num_colors;
  for (int c = 0; c < C; ++c)
    launch_colour<V, true>(plan, plan->before, c, r, z, sc, st);
  for (int c = C - 2; c >= 0; --c)
    launch_colour<V, false>(plan, plan->after, c, r, z, sc, st);
}

template <typename V, int K, bool VEC, bool FORWARD>
void launch_colour_block(const spmv_hip_mcgs_plan* plan, const McgsPartDev& p,
                         int c, int nrhs, const double* r, double* z,
                         const CgbState* state, hipStream_t st)
{
  const int32_t ns = p.color_slice[c + 1] - p.color_slice[c];
  const int32_t nl = p.color_long[c + 1] - p.color_long[c];
  const int64_t waves = (int64_t)ns + nl;
  if (waves == 0)
    return;
  const unsigned grid = (unsigned)((waves + kWaves - 1) / kWaves);
  hipLaunchKernelGGL((mcgs_sweep_block_kernel<V, K, VEC, FORWARD>), dim3(grid),
                     dim3(kBlock), 0, st, p.color_slice[c], ns,
                     plan->color_start[c + 1], p.color_long[c], nl, p.slice_pos0,
                     p.slice_ptr, p.len, p.col, PartValues<V>::val(p),
                     p.long_pos, p.long_ptr, p.long_col,
                     PartValues<V>::long_val(p), plan->perm, plan->dinv, nrhs, r,
                     z, state);
}

// the 2C - 1 launches of one width
template <typename V, int K, bool VEC>
void apply_block(const spmv_hip_mcgs_plan* plan, int nrhs, const double* r,
                 double* z, const CgbState* state, hipStream_t st)
{
  const int C = plan->num_colors;
  for (int c = 0; c < C; ++c)
    launch_colour_block<V, K, VEC, true>(plan, plan->before, c, nrhs, r, z, state,
                                         st);
  for (int c = C - 2; c >= 0; --c)
    launch_colour_block<V, K, VEC, false>(plan, plan->after, c, nrhs, r, z, state,
                                          st);
}

// the width and the alignment choose the instantiation, as for every plan
template <typename V>
void apply_block_any(const spmv_hip_mcgs_plan* plan, int nrhs, bool vec,
                     const double* R, double* Z, const CgbState* state,
                     hipStream_t st)
{
  if (nrhs == 2 && vec)
    apply_block<V, 2, true>(plan, nrhs, R, Z, state, st);
  else if (nrhs == 2)
    apply_block<V, 2, false>(plan, nrhs, R, Z, state, st);
  else if (nrhs == 4 && vec)
    apply_block<V, 4, true>(plan, nrhs, R, Z, state, st);
  else if (nrhs == 4)
    apply_block<V, 4, false>(plan, nrhs, R, Z, state, st);
  else if (nrhs == 8 && vec)
    apply_block<V, 8, true>(plan, nrhs, R, Z, state, st);
  else if (nrhs == 8)
    apply_block<V, 8, false>(plan, nrhs, R, Z, state, st);
  else
    apply_block<V, 0, false>(plan, nrhs, R, Z, state, st);
}

// one value array of a plan from fp64 to fp32 (mcgs_plan_narrow)
int narrow_array(spmv_hip_ctx* ctx, int64_t count, double** wide, float** narrow,
                 unsigned long long* bad, int64_t* bytes, hipStream_t st)
{
  if (count == 0 || !*wide)
    return SPMV_HIP_OK;
  SPMV_CHECK_HIP(spmv_plan_malloc(narrow, (size_t)count * sizeof(float)));
  *bytes += count * (int64_t)sizeof(float);
  hipLaunchKernelGGL(mcgs_narrow_kernel, dim3(spmv_grid_for(ctx, count, kBlock)),
                     dim3(kBlock), 0, st, count, *wide, *narrow, bad);
  SPMV_CHECK_HIP(hipGetLastError());
  SPMV_CHECK_HIP(hipStreamSynchronize(st));
  SPMV_CHECK_HIP(spmv_plan_free(*wide));
  *wide = nullptr;
  *bytes -= count * (int64_t)sizeof(double);
  return SPMV_HIP_OK;
}

} // namespace

extern "C" {

int spmv_hip_mcgs_plan_create(spmv_hip_ctx* ctx, const spmv_hip_mcgs_host* in,
                              spmv_hip_mcgs_plan** plan)
{
  SPMV_REQUIRE(ctx && in && plan);
  *plan = nullptr;
  const int32_t n = in->num_rows, C = in->num_colors;
  SPMV_REQUIRE(n >= 0 && C >= 0 && (n == 0) == (C == 0));
  SPMV_REQUIRE(in->color_start && (n == 0 || (in->perm && in->dinv)));
  SPMV_REQUIRE(in->color_start[0] == 0 && in->color_start[C] == n);
  for (int c = 0; c < C; ++c) // every colour is worn
    SPMV_REQUIRE(in->color_start[c + 1] > in->color_start[c]);
  for (int32_t pos = 0; pos < n; ++pos)
    SPMV_REQUIRE(in->perm[pos] >= 0 && in->perm[pos] < n);
  SPMV_REQUIRE(part_is_sound(*in, in->before) && part_is_sound(*in, in->after));
  SPMV_SET_DEVICE(ctx);
  spmv_hip_mcgs_plan* p = new (std::nothrow) spmv_hip_mcgs_plan();
  if (!p)
    return SPMV_HIP_EINVAL;
  p->ctx = ctx;
  p->n = n;
  p->num_colors = C;
  p->color_start.assign(in->color_start, in->color_start + C + 1);
  int rc;
  if ((rc = upload(in->perm, (size_t)n, &p->perm, &p->bytes)) != SPMV_HIP_OK
      || (rc = upload(in->dinv, (size_t)n, &p->dinv, &p->bytes)) != SPMV_HIP_OK
      || (rc = upload_part(*in, in->before, &p->before, &p->bytes)) != SPMV_HIP_OK
      || (rc = upload_part(*in, in->after, &p->after, &p->bytes))
             != SPMV_HIP_OK) {
    spmv_hip_mcgs_plan_destroy(p);
    return rc;
  }
  *plan = p;
  return SPMV_HIP_OK;
}

int spmv_hip_mcgs_plan_create_ex(spmv_hip_ctx* ctx, const spmv_hip_mcgs_host* in,
                                 int value_bits, spmv_hip_mcgs_plan** plan,
                                 int64_t* out_of_range)
{
  SPMV_REQUIRE(plan != nullptr);
  *plan = nullptr;
  SPMV_REQUIRE(out_of_range && (value_bits == 64 || value_bits == 32));
  *out_of_range = 0;
  spmv_hip_mcgs_plan* p = nullptr;
  int rc = spmv_hip_mcgs_plan_create(ctx, in, &p);
  if (rc != SPMV_HIP_OK || value_bits == 64) {
    *plan = p;
    return rc;
  }
  rc = mcgs_plan_narrow(p, ctx->stream, out_of_range);
  if (rc == SPMV_HIP_OK && *out_of_range != 0)
    rc = SPMV_HIP_ERANGE;
  if (rc != SPMV_HIP_OK) {
    spmv_hip_mcgs_plan_destroy(p);
    return rc;
  }
  *plan = p;
  return SPMV_HIP_OK;
}

int spmv_hip_mcgs_plan_destroy(spmv_hip_mcgs_plan* plan)
{
  if (!plan)
    return SPMV_HIP_OK;
  (void)hipSetDevice(plan->ctx->device);
  free_part(&plan->before);
  free_part(&plan->after);
  plan_drop(plan->perm);
  plan_drop(plan->dinv);
  delete plan;
  return SPMV_HIP_OK;
}

int spmv_hip_mcgs_plan_bytes(const spmv_hip_mcgs_plan* plan, int64_t* bytes)
{
  SPMV_REQUIRE(plan && bytes);
  *bytes = plan->bytes;
  return SPMV_HIP_OK;
}

int spmv_hip_mcgs_plan_value_bits(const spmv_hip_mcgs_plan* plan, int* bits)
{
  SPMV_REQUIRE(plan && bits);
  *bits = plan->value_bits;
  return SPMV_HIP_OK;
}

int spmv_hip_mcgs_apply_f64(spmv_hip_ctx* ctx, const spmv_hip_mcgs_plan* plan,
                            spmv_hip_pcg_ws* ws, const double* r, double* z,
                            void* stream)
{
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx && (!ws || ws->ctx == ctx));
  SPMV_REQUIRE(plan->n == 0 || (r && z));
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  const PcgScalars* sc = ws ? ws->sc : nullptr;
  if (plan->value_bits == 32)
    apply_single<float>(plan, r, z, sc, st);
  else
    apply_single<double>(plan, r, z, sc, st);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

int spmv_hip_mcgs_apply_block_f64(spmv_hip_ctx* ctx,
                                  const spmv_hip_mcgs_plan* plan,
                                  spmv_hip_pcgb_ws* ws, const double* R,
                                  double* Z, int nrhs, void* stream)
{
  SPMV_REQUIRE(nrhs >= 1 && nrhs <= SPMV_CGB_MAX);
  SPMV_REQUIRE(ctx && plan && plan->ctx == ctx);
  SPMV_REQUIRE(!ws || (ws->ctx == ctx && ws->nrhs == nrhs));
  SPMV_REQUIRE(plan->n == 0 || (R && Z));
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  const CgbState* state = ws ? ws->st : nullptr;
  const bool vec
      = ((reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(Z)) & 15u)
        == 0;
  if (plan->value_bits == 32)
    apply_block_any<float>(plan, nrhs, vec, R, Z, state, st);
  else
    apply_block_any<double>(plan, nrhs, vec, R, Z, state, st);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

} // extern "C"

int mcgs_plan_narrow(spmv_hip_mcgs_plan* plan, hipStream_t st,
                     int64_t* out_of_range)
{
  SPMV_REQUIRE(plan && out_of_range && plan->value_bits == 64);
  SPMV_SET_DEVICE(plan->ctx);
  *out_of_range = 0;
  plan->value_bits = 32;
  if (plan->n == 0)
    return SPMV_HIP_OK;
  PlanScratch<unsigned long long> bad;
  SPMV_CHECK_HIP(bad.alloc(1));
  SPMV_CHECK_HIP(hipMemsetAsync(bad.get(), 0, sizeof(unsigned long long), st));
  const int C = plan->num_colors;
  for (McgsPartDev* d : {&plan->before, &plan->after}) {
    const size_t ns = (size_t)d->color_slice[(size_t)C];
    const size_t nl = (size_t)d->color_long[(size_t)C];
    int64_t entries = 0, long_entries = 0;
    SPMV_CHECK_HIP(plan_fetch(&entries, d->slice_ptr + ns, 1, st));
    SPMV_CHECK_HIP(plan_fetch(&long_entries, d->long_ptr + nl, 1, st));
    int rc = narrow_array(plan->ctx, entries, &d->val, &d->val32, bad.get(),
                          &plan->bytes, st);
    if (rc == SPMV_HIP_OK)
      rc = narrow_array(plan->ctx, long_entries, &d->long_val, &d->long_val32,
                        bad.get(), &plan->bytes, st);
    if (rc != SPMV_HIP_OK)
      return rc;
  }
  unsigned long long host = 0;
  SPMV_CHECK_HIP(plan_fetch(&host, bad.get(), 1, st));
  *out_of_range = (int64_t)host;
  return SPMV_HIP_OK;
}
