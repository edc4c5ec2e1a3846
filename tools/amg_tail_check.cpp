// Stand-alone check of the host side of the fused AMG tail
// (spmv_amd/csrc/hip/amg_tail_rules.h): which levels form the tail, the
// descriptor builder that spmv_hip_amg_tail_create calls (amg_tail_fill_table:
// per-level validation and the table entries the kernel reads), the index
// checks on a level's CSR arrays and the row-order rule.  No device: the
// "device" pointers of a level are heap blocks here, which the builder never
// dereferences.  Every array is a heap block of exactly its length -- the
// coefficient arrays a and b of exactly `degree` entries -- so a read past an
// end is caught when this is built with the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude
//       -Ispmv_amd/csrc/hip tools/amg_tail_check.cpp -o amg_tail_check
// Prints OK and returns 0, or names the first rule that does not hold.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <vector>

#include "amg_tail_rules.h"

namespace
{

int failures = 0;

void expect(bool ok, const char* what)
{
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n", what);
    ++failures;
  }
}

int first(std::vector<int64_t> rows, int64_t max_rows)
{
  return amg_tail_first_level(rows.data(), (int)rows.size(), max_rows);
}

bool sound(int64_t rows, int64_t ncols, int64_t nnz, std::vector<int32_t> rowptr,
           std::vector<int32_t> colind)
{
  return amg_tail_csr_is_sound(rows, ncols, nnz, rowptr.data(),
                               colind.empty() ? nullptr : colind.data());
}

void selection()
{
  expect(first({13824, 1685, 150}, 0) == 3, "0 = no tail");
  expect(first({13824, 1685, 150}, 149) == 3, "a coarsest level too large");
  expect(first({13824, 1685, 150}, 150) == 2, "the coarsest level alone");
  expect(first({13824, 1685, 150}, 1684) == 2, "one row short of level 1");
  expect(first({13824, 1685, 150}, 1685) == 1, "two levels");
  expect(first({13824, 1685, 150}, 1000000000) == 1, "level 0 is never in it");
  expect(first({200}, 1000000000) == 1, "one level has no tail");
  expect(first({}, 5) == 0, "no level at all");
  expect(first({3001, 77}, 77) == 1, "two levels, the coarse one");
  // a suffix: a small level above a large one is not part of it
  expect(first({900, 50, 400, 60}, 100) == 3, "the suffix stops at a large level");
  expect(first({900, 50, 400, 60}, 400) == 1, "all levels >= 1");
  expect(first({900, 50, 400, 60}, -7) == 4, "a negative bound selects nothing");
  expect(amg_tail_first_level(nullptr, 3, 10) == 3, "NULL sizes");
}

void csr_checks()
{
  const std::vector<int32_t> rp = {0, 2, 2, 5}, ci = {0, 2, 1, 0, 2};
  expect(sound(3, 3, 5, rp, ci), "a sound block");
  expect(sound(1, 1, 0, {0, 0}, {}), "an empty row alone");
  expect(!sound(0, 3, 0, {0}, {}), "no rows");
  expect(!sound(3, 3, 5, {1, 2, 2, 5}, ci), "rowptr does not start at 0");
  expect(!sound(3, 3, 5, {0, 3, 2, 5}, ci), "rowptr decreases");
  expect(!sound(3, 3, 5, {0, 2, 7, 5}, ci), "rowptr beyond the entries");
  expect(!sound(3, 3, 4, rp, ci), "rowptr's end is not the entry count");
  expect(!sound(3, 3, 5, rp, {0, 2, 1, 0, 3}), "a column beyond the block");
  expect(!sound(3, 3, 5, rp, {0, 2, -1, 0, 2}), "a negative column");
  expect(!sound(3, 3, 5, rp, {}), "entries without a column array");
  expect(!amg_tail_csr_is_sound(3, 3, 5, nullptr, ci.data()), "NULL rowptr");
  expect(!sound(3, 3, -1, rp, ci), "a negative entry count");
  // a long row: every entry is looked at, none beyond
  std::vector<int32_t> lrp = {0, 2500}, lci(2500, 0);
  expect(sound(1, 1, 2500, lrp, lci), "one long row");
  lci.back() = 1;
  expect(!sound(1, 1, 2500, lrp, lci), "its last column out of range");
}

void lanes()
{
  for (int l : {0, 4, 8, 16, 32, 64})
    expect(amg_tail_lanes_is_sound(l), "a lane count of the vector kernel");
  for (int l : {-1, 1, 2, 3, 6, 65, 128})
    expect(!amg_tail_lanes_is_sound(l), "a lane count it never has");
}

// A tail of the given level sizes with everything the builder looks at, each
// array a heap block of its exact length.
struct Fixture {
  int s, c;
  std::vector<int32_t> rows;
  std::vector<std::unique_ptr<int32_t[]>> ints;
  std::vector<std::unique_ptr<double[]>> doubles;
  std::vector<spmv_hip_amg_tail_level> levels;
  std::vector<AmgTailStep> steps;
  std::vector<AmgTailDev> table;
  spmv_hip_amg_tail_host in{};
  // a stand-in for the opaque step handle: only compared with NULL
  const spmv_hip_amg_plan* handle
      = reinterpret_cast<const spmv_hip_amg_plan*>(&in);

  int32_t* ivec(size_t n)
  {
    ints.emplace_back(new int32_t[n ? n : 1]());
    return ints.back().get();
  }
  double* dvec(size_t n, double fill)
  {
    doubles.emplace_back(new double[n ? n : 1]);
    for (size_t i = 0; i < (n ? n : 1); ++i)
      doubles.back()[i] = fill;
    return doubles.back().get();
  }

  Fixture(std::vector<int32_t> sizes, int s_, int c_) : s(s_), c(c_), rows(sizes)
  {
    const int nlev = (int)rows.size();
    levels.resize((size_t)nlev);
    steps.resize((size_t)nlev);
    table.resize((size_t)nlev);
    for (int l = 0; l < nlev; ++l) {
      const size_t n = (size_t)rows[(size_t)l];
      const bool last = l == nlev - 1;
      const int degree = last ? c : s;
      spmv_hip_amg_tail_level& h = levels[(size_t)l];
      h = spmv_hip_amg_tail_level();
      h.rows = rows[(size_t)l];
      h.lanes_per_row = l % 2 ? 8 : 0;
      h.nnz = (int64_t)(2 * n);
      h.rowptr = ivec(n + 1);
      h.colind = ivec(2 * n);
      h.values = dvec(2 * n, 1.0);
      h.dinv = dvec(n, 1.0);
      h.r = dvec(n, 0.0);
      h.w = dvec(n, 0.0);
      h.dd = dvec(n, 0.0);
      h.z = dvec(n, 0.0);
      h.a = dvec((size_t)degree, 10.0 + l); // exactly `degree` entries
      h.b = dvec((size_t)degree, 20.0 + l);
      AmgTailStep& st = steps[(size_t)l];
      st = AmgTailStep();
      if (!last) {
        h.step = handle;
        st.present = true;
        st.fine_rows = h.rows;
        st.coarse_rows = rows[(size_t)l + 1];
        st.agg = ivec(n);
        st.member_ptr = ivec((size_t)st.coarse_rows + 1);
        st.member = ivec(n);
      }
    }
    in.num_levels = nlev;
    in.smooth_degree = s;
    in.coarse_degree = c;
    in.coarse_scale = 1.0;
    in.levels = levels.data();
  }

  bool fill() { return amg_tail_fill_table(in, steps.data(), table.data()); }
};

void builder_fills_the_table(int s, int c)
{
  Fixture f({2049, 300, 7}, s, c);
  expect(f.fill(), "a sound tail of three levels");
  for (int l = 0; l < 3; ++l) {
    const spmv_hip_amg_tail_level& h = f.levels[(size_t)l];
    const AmgTailDev& d = f.table[(size_t)l];
    const bool last = l == 2;
    const int degree = last ? c : s;
    expect(d.rows == h.rows && d.lanes == h.lanes_per_row, "rows and lanes");
    expect(d.rowptr == h.rowptr && d.colind == h.colind && d.values == h.values
               && d.dinv == h.dinv && d.r == h.r && d.w == h.w && d.dd == h.dd
               && d.z == h.z,
           "the level's arrays");
    if (last)
      expect(d.coarse_rows == 0 && !d.agg && !d.member_ptr && !d.member,
             "the last entry has no step");
    else
      expect(d.coarse_rows == f.rows[(size_t)l + 1]
                 && d.agg == f.steps[(size_t)l].agg
                 && d.member_ptr == f.steps[(size_t)l].member_ptr
                 && d.member == f.steps[(size_t)l].member,
             "the step's lists");
    for (int j = 0; j < SPMV_HIP_AMG_TAIL_MAX_DEGREE; ++j) {
      expect(d.a[j] == (j < degree ? 10.0 + l : 0.0), "a: degree entries, then 0");
      expect(d.b[j] == (j < degree ? 20.0 + l : 0.0), "b: degree entries, then 0");
    }
  }
  // new coefficients of exactly `degree` entries into one entry
  std::unique_ptr<double[]> a(new double[(size_t)s]), b(new double[(size_t)s]);
  for (int j = 0; j < s; ++j) {
    a[(size_t)j] = 1.5;
    b[(size_t)j] = 2.5;
  }
  amg_tail_set_entry_coefficients(f.table[0], s, a.get(), b.get());
  expect(f.table[0].a[s - 1] == 1.5 && f.table[0].b[0] == 2.5,
         "rewritten coefficients");
  if (s < SPMV_HIP_AMG_TAIL_MAX_DEGREE)
    expect(f.table[0].a[s] == 0.0, "nothing past the degree");
}

void refused(const char* what, const std::function<void(Fixture&)>& corrupt,
             std::vector<int32_t> sizes = {300, 40})
{
  Fixture f(sizes, 2, 3);
  expect(f.fill(), "the fixture itself is sound");
  corrupt(f);
  expect(!f.fill(), what);
}

void builder_refusals()
{
  Fixture one({5}, 1, 1);
  expect(one.fill(), "a tail of the coarsest level alone");
  Fixture sixteen(std::vector<int32_t>(16, 3), 16, 16);
  expect(sixteen.fill(), "sixteen levels, degree 16");

  refused("no levels", [](Fixture& f) { f.in.num_levels = 0; });
  refused("seventeen levels", [](Fixture& f) { f.in.num_levels = 17; });
  refused("NULL level array", [](Fixture& f) { f.in.levels = nullptr; });
  refused("smooth_degree 0", [](Fixture& f) { f.in.smooth_degree = 0; });
  refused("smooth_degree 17", [](Fixture& f) { f.in.smooth_degree = 17; });
  refused("coarse_degree 0", [](Fixture& f) { f.in.coarse_degree = 0; });
  refused("coarse_degree 17", [](Fixture& f) { f.in.coarse_degree = 17; });
  refused("no rows", [](Fixture& f) { f.levels[1].rows = 0; });
  refused("rows the kernel's int32 loops would pass",
          [](Fixture& f) { f.levels[0].rows = kAmgTailMaxRows + 1; });
  refused("a negative entry count", [](Fixture& f) { f.levels[0].nnz = -1; });
  refused("an entry count beyond int32",
          [](Fixture& f) { f.levels[0].nnz = (int64_t)INT32_MAX + 1; });
  refused("NULL rowptr", [](Fixture& f) { f.levels[0].rowptr = nullptr; });
  refused("NULL colind", [](Fixture& f) { f.levels[1].colind = nullptr; });
  refused("NULL values", [](Fixture& f) { f.levels[0].values = nullptr; });
  refused("NULL dinv", [](Fixture& f) { f.levels[1].dinv = nullptr; });
  refused("NULL r", [](Fixture& f) { f.levels[0].r = nullptr; });
  refused("NULL w", [](Fixture& f) { f.levels[0].w = nullptr; });
  refused("NULL dd", [](Fixture& f) { f.levels[1].dd = nullptr; });
  refused("NULL z", [](Fixture& f) { f.levels[1].z = nullptr; });
  refused("NULL a", [](Fixture& f) { f.levels[0].a = nullptr; });
  refused("NULL b", [](Fixture& f) { f.levels[1].b = nullptr; });
  auto off = [](auto* p, int bytes) {
    return reinterpret_cast<decltype(p)>(
        reinterpret_cast<uintptr_t>(p) + (uintptr_t)bytes);
  };
  refused("unaligned z", [&](Fixture& f) { f.levels[0].z = off(f.levels[0].z, 4); });
  refused("unaligned r", [&](Fixture& f) { f.levels[1].r = off(f.levels[1].r, 4); });
  refused("unaligned w", [&](Fixture& f) { f.levels[0].w = off(f.levels[0].w, 1); });
  refused("unaligned dd",
          [&](Fixture& f) { f.levels[0].dd = off(f.levels[0].dd, 2); });
  refused("unaligned dinv",
          [&](Fixture& f) { f.levels[0].dinv = off(f.levels[0].dinv, 4); });
  refused("unaligned values",
          [&](Fixture& f) { f.levels[1].values = off(f.levels[1].values, 4); });
  refused("unaligned rowptr",
          [&](Fixture& f) { f.levels[0].rowptr = off(f.levels[0].rowptr, 2); });
  refused("unaligned colind",
          [&](Fixture& f) { f.levels[0].colind = off(f.levels[0].colind, 1); });
  refused("an empty level needs no colind or values, but a full one does",
          [](Fixture& f) { f.levels[0].colind = nullptr; });
  refused("a lane count the kernel never has",
          [](Fixture& f) { f.levels[0].lanes_per_row = 3; });
  refused("no step between two levels",
          [](Fixture& f) { f.levels[0].step = nullptr; });
  refused("a step of another context (not present)",
          [](Fixture& f) { f.steps[0].present = false; });
  refused("a step whose fine rows are not the level's",
          [](Fixture& f) { f.steps[0].fine_rows = 299; });
  refused("a step whose coarse rows are not the next level's",
          [](Fixture& f) { f.steps[0].coarse_rows = 41; });
  refused("the next level's rows are not the step's",
          [](Fixture& f) { f.levels[1].rows = 39; });
  refused("a step without its lists", [](Fixture& f) { f.steps[0].agg = nullptr; });
  refused("a last level that has a step",
          [](Fixture& f) { f.levels[1].step = f.handle; });
  refused("a last level whose step is present",
          [](Fixture& f) { f.steps[1].present = true; });
  refused("a middle level without a step",
          [](Fixture& f) { f.levels[1].step = nullptr; }, {2049, 300, 7});
  // an empty level: no colind, no values
  Fixture empty({4, 2}, 1, 1);
  empty.levels[1].nnz = 0;
  empty.levels[1].colind = nullptr;
  empty.levels[1].values = nullptr;
  expect(empty.fill(), "a level without entries needs no colind or values");
}

} // namespace

int main()
{
  selection();
  csr_checks();
  lanes();
  builder_fills_the_table(1, 1);
  builder_fills_the_table(2, 8);
  builder_fills_the_table(16, 16);
  builder_fills_the_table(1, 16);
  builder_fills_the_table(16, 1);
  builder_refusals();
  if (failures) {
    std::fprintf(stderr, "%d rule(s) failed\n", failures);
    return 1;
  }
  std::puts("OK");
  return 0;
}
