// Stand-alone check of the solver workspaces' ownership core
// (spmv_amd/csrc/hip/ws_core.h) on the CPU, meant to be built with the
// sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ispmv_amd/csrc/hip tools/ws_core_check.cpp -o ws_core_check
//       && ./ws_core_check
//
// The allocator counts over std::malloc and can be told to fail its i-th
// allocation -- the unwinding of create that no test can reach on a device.
// The workspace is a dummy with nine arrays, as many as the largest real one
// (bicgstab), of three element types.  Checked: for every i from 1 to 10 create
// returns the allocator's status when the i-th allocation fails (i <= 9), leaves
// *out alone and nothing allocated, and frees each of the i - 1 arrays exactly
// once; with no failure it returns 0 and every field is set and usable; destroy
// frees all nine once; destroy(null) is 0; create, destroy, create again leaves
// the counts balanced; an owner whose alloc failed refuses further allocs with
// the first status, and release() nulls every field it had filled.  A double
// free, a leak or a use after free is the sanitizers' to report.
// Exit status 0 and "ws_core_check: OK" when everything holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <set>

#include "ws_core.h"

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
  static int mallocs, frees, fail_at; // fail_at: the i-th malloc fails (0: none)
  static std::set<void*> live;
  static bool bad_free; // a pointer freed that was not live (twice, or never ours)
  static int malloc(void** p, std::size_t bytes)
  {
    ++mallocs;
    if (mallocs == fail_at) {
      *p = nullptr;
      return 2; // (the value of hipErrorOutOfMemory; any non-zero would do)
    }
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    return 0;
  }
  static int free(void* p)
  {
    ++frees;
    if (live.erase(p) != 1)
      bad_free = true;
    else
      std::free(p);
    return 0;
  }
  static void restart(int fail = 0)
  {
    mallocs = frees = 0;
    fail_at = fail;
    bad_free = false;
  }
};
int Counting::mallocs = 0, Counting::frees = 0, Counting::fail_at = 0;
std::set<void*> Counting::live;
bool Counting::bad_free = false;

struct Ctx {
  int blocks = 7;
};
struct Scalars {
  double rtol;
  int32_t done, kstop;
};
constexpr int kFields = 9;

struct Ws {
  Ctx* ctx = nullptr;
  int kmax = 0;
  int width = 0; // a field of the solver's own, set by fill
  WsArrays<Counting> own;
  double* a = nullptr;
  double* b = nullptr;
  double* c = nullptr;
  double* p0 = nullptr;
  double* p1 = nullptr;
  double* p2 = nullptr;
  int32_t* idx = nullptr;
  double* p3 = nullptr;
  Scalars* sc = nullptr;
};

int create(Ctx* ctx, int kmax, Ws** out)
{
  return ws_create(ctx, kmax, out, [&](Ws& w) {
    w.width = 3;
    const std::size_t hist = (std::size_t)kmax + 1;
    w.own.alloc(w.a, hist);
    w.own.alloc(w.b, 2 * hist);
    w.own.alloc(w.c, 2 * hist);
    for (double** p : {&w.p0, &w.p1, &w.p2})
      w.own.alloc(*p, ctx->blocks);
    w.own.alloc(w.idx, 5);
    w.own.alloc(w.p3, ctx->blocks);
    w.own.alloc(w.sc, 1);
  });
}

void use(Ws* ws) // (the sanitizer watches the element past each end)
{
  ws->a[ws->kmax] = 1.0;
  ws->b[2 * ws->kmax + 1] = ws->c[2 * ws->kmax + 1] = 2.0;
  ws->p0[6] = ws->p1[6] = ws->p2[6] = ws->p3[6] = 3.0;
  ws->idx[4] = 4;
  ws->sc->kstop = -1;
}

void failure_sweep()
{
  Ctx ctx;
  for (int i = 1; i <= kFields + 1; ++i) {
    Counting::restart(i);
    Ws* const untouched = reinterpret_cast<Ws*>(&ctx);
    Ws* ws = untouched;
    const int rc = create(&ctx, 5, &ws);
    if (i <= kFields) {
      expect(rc == 2, "create returns the allocator's status unchanged");
      expect(ws == untouched, "a failed create leaves *out alone");
      expect(Counting::mallocs == i, "no allocation is tried after the failure");
      expect(Counting::frees == i - 1, "every array allocated before it is freed once");
      expect(Counting::live.empty(), "nothing is left allocated after a failure");
    } else {
      expect(rc == kWsOk && ws != untouched, "create succeeds");
      expect(ws->ctx == &ctx && ws->kmax == 5 && ws->width == 3,
             "ctx, kmax and the solver's own field are set");
      expect(Counting::mallocs == kFields && Counting::frees == 0
                 && (int)Counting::live.size() == kFields,
             "nine arrays, none freed");
      use(ws);
      expect(ws_destroy(ws) == kWsOk, "destroy");
      expect(Counting::frees == kFields && Counting::live.empty(),
             "destroy frees every array once");
    }
    expect(!Counting::bad_free, "no array is freed twice");
  }
}

void null_and_again()
{
  Counting::restart();
  expect(ws_destroy(static_cast<Ws*>(nullptr)) == kWsOk, "destroy(null) is OK");
  expect(Counting::frees == 0, "and frees nothing");
  Ctx ctx;
  Ws* ws = nullptr;
  expect(create(&ctx, 0, &ws) == kWsOk && ws, "create");
  use(ws);
  expect(ws_destroy(ws) == kWsOk, "destroy");
  ws = nullptr;
  expect(create(&ctx, 8, &ws) == kWsOk && ws && ws->kmax == 8, "create again");
  use(ws);
  expect(ws_destroy(ws) == kWsOk, "destroy again");
  expect(Counting::mallocs == 2 * kFields && Counting::frees == 2 * kFields
             && Counting::live.empty() && !Counting::bad_free,
         "create, destroy, create, destroy: the counts balance");
}

void owner_alone()
{
  Counting::restart(3);
  WsArrays<Counting> own;
  double *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;
  expect(own.alloc(a, 4) == 0 && a, "first alloc");
  expect(own.alloc(b, 4) == 0 && b, "second alloc");
  expect(own.alloc(c, 4) == 2 && !c, "the failing alloc leaves its field null");
  expect(own.alloc(d, 4) == 2 && !d && Counting::mallocs == 3,
         "a further alloc is a no-op that returns the first status");
  expect(own.status() == 2, "the owner keeps the first status");
  own.release();
  expect(!a && !b && !c && !d, "release nulls every remembered field");
  expect(Counting::frees == 2 && Counting::live.empty() && !Counting::bad_free,
         "and frees each once");
  own.release();
  expect(Counting::frees == 2, "a second release frees nothing");
  expect(own.status() == 0 && own.alloc(a, 1) == 0 && a, "a released owner fills again");
  own.release();
  expect(Counting::live.empty() && !Counting::bad_free, "and lets go again");
}
} // namespace

int main()
{
  failure_sweep();
  null_and_again();
  owner_alone();
  if (failures) {
    std::printf("ws_core_check: %d FAILED\n", failures);
    return 1;
  }
  std::printf("ws_core_check: OK\n");
  return 0;
}
