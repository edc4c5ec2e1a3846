// Ownership of a solver workspace's device arrays, and the parts of create and
// destroy every workspace shares.  A workspace struct embeds one WsArrays as
// `own`; each alloc() allocates into a typed field of the struct and remembers
// the field, release() frees and nulls what was remembered.  The allocator is a
// template argument -- a type with two static functions, malloc(void**, size_t
// bytes) and free(void*), whose status converts to an int that is 0 on success
// (the owner keeps it as an int) -- so that this header knows nothing of HIP
// and tools/ws_core_check.cpp can run the unwinding after a failed allocation
// on the CPU under the sanitizers (no device lets a test provoke one).
// solver_ws.h binds it to hipMalloc / hipFree.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>

constexpr int kWsOk = 0;     // SPMV_HIP_OK
constexpr int kWsNoMem = -2; // SPMV_HIP_ENOMEM (solver_ws.h asserts both)
// arrays of one workspace at most (bicgstab has nine)
constexpr int kWsMaxArrays = 12;

template <typename Alloc>
class WsArrays
{
public:
  WsArrays() = default;
  WsArrays(const WsArrays&) = delete;
  WsArrays& operator=(const WsArrays&) = delete;

  // `count` elements into `field`, which must be null and outlive release().
  // After the first failure every further call does nothing and returns that
  // first status.
  template <typename T>
  int alloc(T*& field, std::size_t count)
  {
    if (status_ != 0)
      return status_;
    if (n_ == kWsMaxArrays)
      std::abort(); // a workspace with more arrays: raise kWsMaxArrays
    void* p = nullptr;
    status_ = static_cast<int>(Alloc::malloc(&p, sizeof(T) * count));
    if (status_ != 0)
      return status_;
    field = static_cast<T*>(p);
    fields_[n_++] = &field;
    return status_;
  }
  int status() const { return status_; }

  // frees and nulls every remembered field; the owner can be filled again
  void release()
  {
    while (n_ > 0) {
      void* const slot = fields_[--n_]; // the address of a T* field
      void* p = nullptr;
      std::memcpy(&p, slot, sizeof(p));
      (void)Alloc::free(p);
      p = nullptr;
      std::memcpy(slot, &p, sizeof(p));
    }
    status_ = 0;
  }

private:
  void* fields_[kWsMaxArrays] = {};
  int n_ = 0;
  int status_ = 0;
};

// new Ws with ctx and kmax set, then fill(*ws) -- the solver's own fields and
// its ws.own.alloc calls.  A failed allocation unwinds: everything allocated so
// far is freed, the struct deleted, *out left alone, and the allocator's status
// returned as it is.
template <typename Ws, typename Ctx, typename Fill>
int ws_create(Ctx* ctx, int kmax, Ws** out, Fill&& fill)
{
  Ws* ws = new (std::nothrow) Ws;
  if (!ws)
    return kWsNoMem;
  ws->ctx = ctx;
  ws->kmax = kmax;
  fill(*ws);
  const int status = ws->own.status();
  if (status != 0) {
    ws->own.release();
    delete ws;
    return status;
  }
  *out = ws;
  return kWsOk;
}

template <typename Ws>
int ws_destroy(Ws* ws)
{
  if (!ws)
    return kWsOk;
  ws->own.release();
  delete ws;
  return kWsOk;
}
