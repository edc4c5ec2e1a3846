// Device memory of the plan-building translation units.  They allocate ONLY
// through this header: spmv_plan_malloc / spmv_plan_free are hipMalloc /
// hipFree with the call's wall time added to a per-thread counter, and
// PlanScratch is the owner (dev_scratch.h) over them.
// spmv_hip_csr_plan_create / _bake_values_* / _values_changed read the counter
// around their work and file the difference under the plan ("plan_mem_us"):
// plan_us then splits into analysis (kernels, copies, host logic) and memory
// (allocation of the plan's own arrays, release of the scratch).  Why: one
// bench record of round 5 showed 2.3 s and 2.8 s for the two multi-GB baking
// forms where every other run shows 12-18 ms (profiles/
// r05_bench_n1_default_detail.json) -- with this split a recurrence says
// whether the device driver's allocator stalled or the analysis did.
#pragma once

#include <chrono>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "dev_scratch.h"
#include "spmv_hip.h"

extern thread_local int64_t spmv_plan_mem_ns; // spmv_csr_plan.hip
// arrays this thread has allocated through spmv_plan_malloc and not yet freed
// through spmv_plan_free (spmv_hip_plan_live_allocations): the builders'
// tests read it around a refused call to see that nothing was left behind
extern thread_local int64_t spmv_plan_live_allocs; // spmv_csr_plan.hip

template <typename P>
static inline hipError_t spmv_plan_malloc(P** p, size_t bytes)
{
  const auto t0 = std::chrono::steady_clock::now();
  const hipError_t e = hipMalloc(p, bytes);
  spmv_plan_mem_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(
                          std::chrono::steady_clock::now() - t0)
                          .count();
  if (e == hipSuccess && bytes > 0)
    ++spmv_plan_live_allocs;
  return e;
}
static inline hipError_t spmv_plan_free(void* p)
{
  const auto t0 = std::chrono::steady_clock::now();
  const hipError_t e = hipFree(p);
  if (p)
    --spmv_plan_live_allocs;
  spmv_plan_mem_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(
                          std::chrono::steady_clock::now() - t0)
                          .count();
  return e;
}

struct PlanAlloc {
  static hipError_t malloc(void** p, size_t bytes) { return spmv_plan_malloc(p, bytes); }
  static hipError_t free(void* p) { return spmv_plan_free(p); }
};
template <typename T>
using PlanScratch = DevScratch<T, PlanAlloc>;

template <typename T>
static inline void plan_drop(T*& field)
{
  plan_drop<PlanAlloc>(field);
}

// A hipcub device-wide call, both phases: call(nullptr, bytes) asks for the
// size, `tmp` gets that many bytes (16 for none), call(tmp, bytes) runs.  The
// caller's lambda holds the hipcub call itself, so its iterator and functor
// types -- which decide the kernels instantiated -- are the caller's.  `tmp`
// is the caller's because the call is asynchronous: it must outlive the work.
template <typename Call>
static inline hipError_t plan_cub(PlanScratch<void>& tmp, Call&& call)
{
  size_t bytes = 0;
  hipError_t e = call(static_cast<void*>(nullptr), bytes);
  if (e == hipSuccess)
    e = tmp.alloc(bytes ? bytes : 16);
  if (e == hipSuccess)
    e = call(tmp.get(), bytes);
  return e;
}

// `count` elements back to the host, and wait for them
template <typename T>
static inline hipError_t plan_fetch(T* host, const T* dev, size_t count,
                                    hipStream_t stream)
{
  const hipError_t e
      = hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, stream);
  return e == hipSuccess ? hipStreamSynchronize(stream) : e;
}

// the failure tail of the builders that report "no memory" as such: the
// sticky error is cleared, every other code passes through
static inline int plan_fail(hipError_t e)
{
  (void)hipGetLastError();
  return e == hipErrorOutOfMemory ? SPMV_HIP_ENOMEM : static_cast<int>(e);
}
