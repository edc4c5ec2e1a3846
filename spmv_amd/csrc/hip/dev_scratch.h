// Ownership of device arrays while a plan is built.  A DevScratch owns ONE
// array and frees it when it goes out of scope, is reset, or allocates again;
// an array that ends up in the plan is handed to the plan's field with give().
// The allocator is a template argument -- a type with two static functions,
// malloc(void**, size_t bytes) and free(void*) -- so that this header knows
// nothing of HIP and tools/plan_scratch_check.cpp can run every path of it on
// the CPU under the sanitizers, allocation failures included (which cannot be
// provoked on a device).  plan_scratch.h binds it to the timed hipMalloc.
#pragma once

#include <cstddef>
#include <utility>

template <typename T>
struct DevElemSize {
  static constexpr std::size_t value = sizeof(T);
};
template <>
struct DevElemSize<void> { // an untyped array is counted in bytes
  static constexpr std::size_t value = 1;
};

template <typename T, typename Alloc>
class DevScratch
{
public:
  DevScratch() = default;
  DevScratch(const DevScratch&) = delete;
  DevScratch& operator=(const DevScratch&) = delete;
  DevScratch(DevScratch&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DevScratch& operator=(DevScratch&& o) noexcept
  {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
    }
    return *this;
  }
  ~DevScratch() { reset(); }

  // `count` elements (T = void: bytes); what was held is freed first.  Returns
  // the allocator's status; after a failure the owner is empty.
  auto alloc(std::size_t count)
  {
    reset();
    void* p = nullptr;
    const auto status = Alloc::malloc(&p, DevElemSize<T>::value * count);
    p_ = static_cast<T*>(p);
    return status;
  }
  T* get() const { return p_; }
  void reset()
  {
    if (p_)
      (void)Alloc::free(p_);
    p_ = nullptr;
  }
  // the array becomes the plan's: what the field held is freed first
  void give(T*& field)
  {
    if (field)
      (void)Alloc::free(field);
    field = std::exchange(p_, nullptr);
  }

private:
  T* p_ = nullptr;
};

// free a plan's field and null it (the *_free functions)
template <typename Alloc, typename T>
inline void plan_drop(T*& field)
{
  if (field)
    (void)Alloc::free(field);
  field = nullptr;
}
