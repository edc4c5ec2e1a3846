// Stand-alone check of the plan builders' ownership of device arrays
// (spmv_amd/csrc/hip/dev_scratch.h) on the CPU, meant to be built with the
// sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ispmv_amd/csrc/hip tools/plan_scratch_check.cpp -o plan_scratch_check
//       && ./plan_scratch_check
//
// The allocator counts over std::malloc and can be told to fail its k-th
// allocation -- the paths no test can take on a device.  Checked: an owner
// frees exactly once at scope end; a second alloc frees the first array, reset
// frees and nulls; a moved-from owner frees nothing; give frees the field's old
// array, hands the new one over and leaves the owner empty; plan_drop frees and
// nulls and does nothing on null; and a builder modelled on
// spmv_sj_build_long_list (seven owners, one of them reused, one array the
// plan's on success) leaves nothing allocated whichever allocation fails, and
// only the plan's array when none does -- both with the array handed over by
// give (as spmv_tmap_build does) and with it allocated straight into the field
// and left to the caller's plan_drop on failure (as the long list itself
// does).  A double free, a leak or a use after free is the sanitizers' to
// report.
// Exit status 0 and "plan_scratch_check: OK" when everything holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "dev_scratch.h"

namespace
{
int failures = 0;

void expect(bool ok, const char* what)
{
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++failures;
  }
}

struct Counting {
  static int live, mallocs, frees, fail_at; // fail_at: the k-th malloc fails (0: none)
  static int malloc(void** p, std::size_t bytes)
  {
    ++mallocs;
    if (mallocs == fail_at) {
      *p = nullptr;
      return 2; // (the value of hipErrorOutOfMemory; any non-zero would do)
    }
    *p = std::malloc(bytes ? bytes : 1);
    ++live;
    return 0;
  }
  static int free(void* p)
  {
    if (p) {
      ++frees;
      --live;
    }
    std::free(p);
    return 0;
  }
  static void restart(int fail = 0)
  {
    live = mallocs = frees = 0;
    fail_at = fail;
  }
};
int Counting::live = 0, Counting::mallocs = 0, Counting::frees = 0, Counting::fail_at = 0;

template <typename T>
using Scratch = DevScratch<T, Counting>;

void owner()
{
  Counting::restart();
  {
    Scratch<int32_t> a;
    expect(a.get() == nullptr, "an owner starts empty");
    expect(a.alloc(5) == 0 && a.get() != nullptr, "alloc");
    a.get()[4] = 7; // (5 elements: the sanitizer watches the sixth)
    expect(Counting::live == 1 && Counting::frees == 0, "held");
  }
  expect(Counting::live == 0 && Counting::frees == 1, "freed exactly once at scope end");

  Counting::restart();
  {
    Scratch<void> a; // (an untyped array is counted in bytes)
    expect(a.alloc(16) == 0, "alloc void");
    void* first = a.get();
    expect(a.alloc(32) == 0 && Counting::frees == 1 && Counting::live == 1,
           "a second alloc frees the first array");
    (void)first;
    a.reset();
    expect(a.get() == nullptr && Counting::frees == 2 && Counting::live == 0,
           "reset frees and nulls");
    a.reset();
    expect(Counting::frees == 2, "reset of an empty owner frees nothing");
  }
  expect(Counting::frees == 2 && Counting::mallocs == 2, "nothing more at scope end");

  Counting::restart(1);
  {
    Scratch<double> a;
    expect(a.alloc(3) != 0 && a.get() == nullptr, "a failed alloc leaves the owner empty");
  }
  expect(Counting::live == 0 && Counting::frees == 0, "and frees nothing");
}

void moves()
{
  Counting::restart();
  {
    Scratch<int64_t> a;
    expect(a.alloc(2) == 0, "alloc");
    int64_t* p = a.get();
    Scratch<int64_t> b(std::move(a));
    expect(a.get() == nullptr && b.get() == p, "move construction");
    Scratch<int64_t> c;
    expect(c.alloc(1) == 0, "alloc");
    c = std::move(b); // (frees what c held)
    expect(b.get() == nullptr && c.get() == p && Counting::frees == 1, "move assignment");
  }
  expect(Counting::live == 0 && Counting::frees == 2, "a moved-from owner frees nothing");
}

void give_and_drop()
{
  Counting::restart();
  int32_t* field = nullptr;
  {
    Scratch<int32_t> a;
    expect(a.alloc(4) == 0, "alloc");
    int32_t* p = a.get();
    a.give(field);
    expect(field == p && a.get() == nullptr && Counting::frees == 0,
           "give hands the array over and leaves the owner empty");
  }
  expect(Counting::live == 1, "the field's array outlives the owner");
  {
    Scratch<int32_t> a;
    expect(a.alloc(8) == 0, "alloc");
    int32_t* p = a.get();
    a.give(field);
    expect(field == p && Counting::frees == 1 && Counting::live == 1,
           "give frees the field's old array");
  }
  plan_drop<Counting>(field);
  expect(field == nullptr && Counting::frees == 2 && Counting::live == 0,
         "plan_drop frees and nulls");
  plan_drop<Counting>(field);
  expect(field == nullptr && Counting::frees == 2, "plan_drop of null does nothing");
}

// spmv_sj_build_long_list in outline: a counter and a temporary, the temporary
// released and used again, four more arrays in an inner block, the list itself
// the plan's when everything succeeded: handed over by give, or (into_field)
// allocated straight into the field and left there for the caller on failure
int build_like_long_list(int32_t*& field, bool into_field)
{
  Scratch<int32_t> count;
  Scratch<void> tmp;
  Scratch<int32_t> rows;
  auto rows_at = [&]() { return into_field ? field : rows.get(); };
  int e = count.alloc(1);
  if (e == 0)
    e = tmp.alloc(64);
  tmp.reset();
  if (e == 0) {
    e = into_field ? Counting::malloc(reinterpret_cast<void**>(&field),
                                      10 * sizeof(int32_t))
                   : rows.alloc(10);
    if (e == 0)
      e = tmp.alloc(128); // (reused)
    Scratch<uint64_t> key, key2;
    Scratch<int32_t> rows2;
    Scratch<void> tmp2;
    if (e == 0)
      e = key.alloc(10);
    if (e == 0)
      e = key2.alloc(10);
    if (e == 0)
      e = rows2.alloc(10);
    if (e == 0)
      e = tmp2.alloc(256);
    if (e == 0) {
      key.get()[9] = key2.get()[9] = 1;
      rows_at()[9] = rows2.get()[9] = 1;
      count.get()[0] = 10;
    }
  }
  if (e != 0)
    return e;
  if (!into_field)
    rows.give(field);
  return 0;
}

void failure_sweep(bool into_field)
{
  Counting::restart();
  int32_t* field = nullptr;
  expect(build_like_long_list(field, into_field) == 0, "the builder succeeds");
  const int total = Counting::mallocs;
  expect(total == 8, "eight allocations (seven owners, one reused)");
  expect(Counting::live == 1 && field != nullptr, "only the plan's array is left");
  plan_drop<Counting>(field);
  expect(Counting::live == 0, "and the plan frees it");
  for (int k = 1; k <= total; ++k) {
    Counting::restart(k);
    expect(build_like_long_list(field, into_field) != 0, "the builder reports the failure");
    // (allocated into the field: the caller's free function drops it, as
    // spmv_sjds_free does; handed over by give: it never got there)
    expect(into_field || field == nullptr, "the field stays null");
    plan_drop<Counting>(field);
    expect(field == nullptr && Counting::live == 0,
           "nothing is left allocated after a failure");
    expect(Counting::frees == k - 1, "every array allocated before it is freed once");
  }
}
} // namespace

int main()
{
  owner();
  moves();
  give_and_drop();
  failure_sweep(false);
  failure_sweep(true);
  if (failures) {
    std::printf("plan_scratch_check: %d FAILED\n", failures);
    return 1;
  }
  std::printf("plan_scratch_check: OK\n");
  return 0;
}
