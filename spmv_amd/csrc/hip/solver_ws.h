// The HIP side of ws_core.h: the eleven solver workspaces (blas1*.hip) allocate
// ONLY through this header.  It binds the owner to hipMalloc / hipFree, puts
// hipSetDevice around create and destroy, and holds the copies every workspace
// makes between the host and its state words -- the int32 words of its scalars
// struct from `done` (cg_block, pcg_block: `all_done`) on -- and its history.
// What stays in each solver's file: its struct with the embedded `own`, its
// arrays and their lengths, its reset kernel, its `which` table and its
// argument checks.
#pragma once

#include "common.h"
#include "ws_core.h"

static_assert(kWsOk == SPMV_HIP_OK && kWsNoMem == SPMV_HIP_ENOMEM,
              "ws_core.h and spmv_hip.h agree");

struct SolverAlloc {
  static hipError_t malloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void* p) { return hipFree(p); }
};
using SolverArrays = WsArrays<SolverAlloc>;

// ws_create on the context's device; the caller has checked its arguments
template <typename Ws, typename Fill>
static inline int solver_ws_create(spmv_hip_ctx* ctx, int kmax, Ws** out,
                                   Fill&& fill)
{
  SPMV_SET_DEVICE(ctx);
  return ws_create(ctx, kmax, out, fill);
}

template <typename Ws>
static inline int solver_ws_destroy(Ws* ws)
{
  if (ws)
    (void)hipSetDevice(ws->ctx->device);
  return ws_destroy(ws);
}

template <typename Ws>
static inline int solver_ws_capacity(const Ws* ws, int* kmax)
{
  SPMV_REQUIRE(ws && kmax);
  *kmax = ws->kmax;
  return SPMV_HIP_OK;
}

// workgroups of a reset kernel that gives `count` history slots a thread each
static inline dim3 ws_reset_grid(int count)
{
  return dim3((count + kBlock - 1) / kBlock);
}

// n_words state words and the history of hist_count doubles to the host, async
// on the stream.  Either destination may be null (then it is skipped, host_len
// ignored).
static inline int ws_read_async(spmv_hip_ctx* ctx, void* stream,
                                int32_t* host_words, const int32_t* dev_words,
                                size_t n_words, double* host_hist,
                                size_t host_len, const double* dev_hist,
                                size_t hist_count)
{
  // checked before anything is enqueued: a short buffer gets nothing at all
  SPMV_REQUIRE(!host_hist || host_len >= hist_count);
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  if (host_words)
    SPMV_CHECK_HIP(hipMemcpyAsync(host_words, dev_words,
                                  n_words * sizeof(int32_t),
                                  hipMemcpyDeviceToHost, st));
  if (host_hist)
    SPMV_CHECK_HIP(hipMemcpyAsync(host_hist, dev_hist,
                                  sizeof(double) * hist_count,
                                  hipMemcpyDeviceToHost, st));
  return SPMV_HIP_OK;
}

// the test hooks: installs n words and waits (the source is a local or a
// pageable buffer of the caller's) / reads n words, async on the stream
static inline int ws_put_words(spmv_hip_ctx* ctx, void* stream,
                               int32_t* dev_words, const int32_t* host_words,
                               size_t n)
{
  SPMV_SET_DEVICE(ctx);
  hipStream_t st = spmv_stream(ctx, stream);
  SPMV_CHECK_HIP(hipMemcpyAsync(dev_words, host_words, n * sizeof(int32_t),
                                hipMemcpyHostToDevice, st));
  SPMV_CHECK_HIP(hipStreamSynchronize(st));
  return SPMV_HIP_OK;
}

static inline int ws_get_words(spmv_hip_ctx* ctx, void* stream,
                               int32_t* host_words, const int32_t* dev_words,
                               size_t n)
{
  SPMV_SET_DEVICE(ctx);
  SPMV_CHECK_HIP(hipMemcpyAsync(host_words, dev_words, n * sizeof(int32_t),
                                hipMemcpyDeviceToHost,
                                spmv_stream(ctx, stream)));
  return SPMV_HIP_OK;
}
