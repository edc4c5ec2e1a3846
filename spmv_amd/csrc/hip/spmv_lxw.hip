// LX form of the general CSR SpMV, LDS-DMA kernel (gfx950 / MI355X).
//
// Stands behind the same CSRSpMV<T>::init/run hook as the other general
// kernels (spmv/csr_kernels.h:26-78); arithmetic and summation order are those
// of spmv/csr_kernels.cpp:41-51: a row is summed left to right, mul and add
// rounded separately => bit-identical to the oracle.
//
// The LX form (spmv_csr_forms.hip) rewrites every entry's column as a 16-bit offset
// into a per-row-block set of staged x WINDOWS.  The register-staged kernel
// (csr_rowblock_lx_kernel) alternates phases -- fetch windows, wait, stream a
// tile of values + offsets, wait, multiply, park products in LDS, barrier, add
// -- and needs eight workgroups per CU to cover them; PMC passes at 512^3
// showed it at the fabric's byte ceiling (15.5 GB read + 1.07 GB written per
// launch = 6.9 TB/s for 12.1 GB requested): every x element crossed the
// fabric 3.5 times, because the three uses of a window (as a block's own
// columns, and as the far window of the blocks a plane below and above) are
// 4.9 MB of matrix stream per XCD apart -- more than its L2 holds.
//
// This kernel takes the lattice kernel's skeleton (spmv_lat.hip):
//   * lane = row.  A persistent workgroup walks its row blocks with
//     EVERYTHING one block ahead: values (8 B), offsets (2 B) and the x
//     windows of block k+1 arrive by LDS-DMA (global_load_lds_dwordx4: no
//     VGPRs, no LDS store instructions) into the second set of LDS slots while
//     block k is summed; the row pointer pair, y (beta != 0) and the row's own
//     x (fused dot) travel in a second register set.  ONE barrier per block.
//   * the row owner walks its entries in LDS: value, offset, x[offset] --
//     products are never parked.
//   * the y of a block is stored one step LATE, right behind the next
//     step's wait (which covers stores too): issued at the end of its own
//     step the store's whole round trip would be exposed in every step.
//   * a row block the plan could not stage (too many windows, too wide)
//     gathers x from global memory through `colind`, its values still by DMA;
//     one with more entries than a slot holds reads everything from global
//     memory.  The decision is per row block.
//
// LDS per workgroup (dynamic, sized by the plan): 2 x (values slot + offsets
// slot + x buffer); 60 KiB for the 7-point matrix => 2 workgroups per CU.
// (A coded block's codes use a quarter of its offsets slot, see below.)
//
// Measured at 512^3 (7-point matrix, lattice analysis off; one process, the
// kernels alternating): 2.24-2.51 ms against 2.39-2.48 ms for the
// register-staged kernel in the plane-walk order (2.46-2.60 in the plain
// order, round 2's 0.67), i.e. the same within the spread between processes --
// 1.5 % slower at 384^3 and 512^3, equal at 216^3, 6 % faster at 256^3, 14 %
// at 128^3 -- while moving 12.0 GB instead of 13.7 GB (plain order: 15.5 GB)
// across the fabric per launch (profiles/r03_pmc_lx*).  What a step is made
// of (parts switched off one at a time, same process, 2.47 ms whole): without
// the y store 1.96 ms -- before the store moved behind the next wait; 2.24
// with it there --, without the values 1.54, without the offsets 2.15,
// without the x windows 2.40, without the row sums 2.57 (no gain: the
// arithmetic is free), nothing but the skeleton's own loads and barrier 0.85;
// one workgroup per CU instead of two 2.99.  Three things had to go before it
// reached the old kernel at all, each a wait the compiler adds for a register
// that a load may still be writing: the piece list read with v_readlane in
// the middle of the DMA issue (now extracted right after the wait), the
// order-table entry sharing a register with its computed alternative
// (template parameter TAB), and the block record fetched by SCALAR loads,
// whose counter the LDS reads share (now one vector load a step ahead).
// Dropped after measuring: copying the two window pieces a block shares with
// its predecessor in the plane walk inside LDS instead of fetching them again
// (plan-time inheritance table; 11.93 against 12.04 GB of fabric reads -- the
// L2 already served them -- and 1-7 % slower); the values two row blocks ahead
// instead of one (three value slots, 75 KiB per workgroup, still two per CU:
// 2.51 against 2.54 ms at 512^3, 3 % slower at 128^3 and 384^3 -- the bytes a
// workgroup has in flight are not what bounds the kernel either).
//
// 4-bit codes (template parameter C4, plan key "lx4"): three quarters of the
// offsets stream say nothing new -- an offset is the row's lane t plus a
// distance d that depends only on the entry's diagonal and window, and a
// 7-point row block has at most seven of them.  The plan (lx4_encode_kernel,
// spmv_csr_forms.hip) gives every staged block with at most 16 distinct d a
// dictionary (8 more words of its record: it arrives with the same vector
// load a step ahead) and one nibble per entry in a SECOND index array, 0.5 B
// per entry; such a block's issue() sends its codes into the offsets slot
// instead of its 16-bit offsets, any other block does what it did (the
// 16-bit array stays: the register-staged kernel and lx4 = 0 read it).  The
// row sum reads a row's eight nibbles as two aligned dwords and a funnel
// shift and turns each into t + dict[code]; values, x reads and the order of
// the adds are untouched.  Slots, LDS size, grid and row-block order do not
// depend on it, so the fused dot's partials keep their bits.
// Measured at 512^3 (profiles/lx4_ab.json; one process, the variants
// alternating, fused dot on, median of 7 x 10 launches): codes off 2.317 ms,
// dictionary as an LDS table per slot 2.175 ms (-6.1 %), as eight uniform
// registers and a select tree (7 selects, a shift pair per entry) 2.375 ms
// -- SLOWER than the offsets: here the arithmetic is no longer free.  The
// table is the default ("lx4_lut" 2 selects the tree).  Inside CG
// (rocprofv3 kernel trace of the benchmark) 2.421 -> 2.244 ms; fabric reads
// (FETCH_SIZE, calibrated on a streaming dot in the same run) 12.56 ->
// 10.49 GB per launch, more than the 1.41 GB the stream lost: fewer x pieces
// are evicted from the L2 between their uses.  The step: 252.5 -> 263.2 it/s,
// five alternating runs each, ranges apart.  The plan pass: 4.6 ms beside
// lx_build_kernel's 14.2 ms, +0.49 GB of plan memory.  Not tried: sizing the
// offsets slot for codes only (a third workgroup per CU would change the
// grid and with it the partials); byte row lengths instead of the row pointer.
//
// Ring variant (csr_lxw_ring_kernel; plan key / context option "lx_ring"):
// with codes and narrowed values a step streams 4.5 B per entry, and the
// two-slot kernel ran 1.96 ms at 512^3 where the bytes would allow 1.5-1.85:
// 512 workgroups x 14 KB per step / 1.93 us per step = the 3.7 TB/s it
// reached -- ONE memory round trip per step, everything exactly one block
// ahead.  The ring keeps TWO blocks in flight per workgroup in three LDS slots
// sized for what a narrowed, coded block streams (8 KiB of values, 1-4 KiB of
// codes, the x pieces, 512 B of row descriptors; 61.6 KiB for the 7-point
// matrix, still two workgroups per CU): block k is summed from slot k mod 3, block k + 1 is in flight, block
// k + 2 is issued in step k into the slot block k - 1 left.  Grid, row-block
// order, lane-to-row map and the row sum are csr_lxw_kernel's, so y and the
// fused dot's partials keep their bits.  It runs only for a plan whose EVERY
// row block is staged, coded and fits (lx_ring_fits, counted by
// lx4_encode_kernel), TV = float under T = double, LDS table, not XW; anything
// else launches csr_lxw_kernel unchanged.
//   What a step issues, per wave, in this order (all of it inline assembly:
// the compiler counts none of it, so it adds no vmcnt wait of its own, and
// its full wait before s_barrier finds nothing pending):
//     1 store   y of block k - 1 (late; under exec, skipped by a wave without
//               rows)
//     1 load    y of block k + 1 (the head of `out` when beta == 0) -- of a
//               clamped row, never skipped
//     1 load    record of block k + 3 (record 0 when there is none)
//     1 load    order-table entry of block k + 4 (TAB only; clamped)
//     N DMA     block k + 2: VR = 2 value pieces, 1 code piece -- in wave 2 the
//               block's ROW DESCRIPTORS instead --, PWR x pieces; N = VR + 1 +
//               PWR, always all of them: a piece beyond the block's data (or
//               of a slot without a row block) reads the head of its array
//               into the dump area by lane 0 alone; address, LDS target and
//               lane count are chosen by selects
//   then the row sum (LDS only), then `s_waitcnt vmcnt(N)`: the counter retires
// in order, so with at most the N youngest instructions in flight -- block
// k + 2's DMA -- everything older has landed: block k + 1's DMA (issued a step
// earlier), the loads, the store.  What is issued BEFORE the DMA may be
// skipped without harm (it is older than what is waited for).  Every DMA
// instruction stands behind a lane mask (64 lanes, 32 for the descriptors, 1
// for a surplus piece) and the s_cbranch_execz the compiler puts there; lane
// 0 always takes part, so the branch is never taken and the count is exact.
// The loaded registers are operands of the wait, so no use moves above it.
// Prologue and drain wait with vmcnt(0); a workgroup with fewer than three
// blocks issues the missing ones into the dump area and needs no other path.
//   Row descriptors (plan array lx_rowdesc, csr_plan.h; lx_rowdesc_kernel):
// one 16-bit word per row, bits 0..10 the row's first entry relative to the
// block's span start `a`, bits 11..15 its length (at most 31; a block with a
// longer row is not counted in lx_ring_blocks and the plan keeps
// csr_lxw_kernel).  A block's 512 B arrive with its DMA -- a fitting block's
// codes fill at most two pieces, so wave 2's code piece was surplus in every
// block -- into 512 B per slot, and the row sum takes lo and hi from one
// ds_read_u16 plus `a`.  Before, every lane loaded rowptr[r] and rowptr[r + 1]
// into registers the step waited for: 0.54 GB per launch at 512^3, now 0.27.
// A surplus piece used to be a whole 1-KiB piece read from the head of its
// array into a 1-KiB dump area; issued by lane 0 alone it moves 16 B, the dump
// area is 64 B, and the three descriptor slots fit where it was: 63,040 B of
// dynamic LDS for the 7-point matrix (62,464 before), two workgroups per CU.
//   PWR: 4 x pieces per wave cover every plan (16 pieces); a plan that stages
// at most 12 (the 7-point matrix: 11) runs the instantiation with 3 -- one
// DMA instruction less per wave and step, vmcnt(6).  Plan key "lx_ring_pwr" 4
// asks for the other one.
//   Disassembly of the instantiation <DOT = 1, NT = 0, TAB = 1, VR = 2,
// PWR = 4> (hipcc -O3 for gfx950): every step passes ONE vector-memory
// wait, `s_waitcnt vmcnt(7)` (a second one, vmcnt(0), sits inside the branch of
// a block whose own x is not staged, behind that load), followed by `s_waitcnt
// lgkmcnt(0)`, `s_barrier`; between two of them 1 global_store_dwordx2 (behind
// s_cbranch_execz), 1 global_load_dwordx2 (y), 2 global_load_dword (record,
// table), 7 global_load_lds_dwordx4; none of the three destination registers
// is read or written before the wait; one ds_read_u16 per row.  70 VGPRs, no
// spills, no scratch, 128 B of static LDS.
//   Measured at 512^3, one MI355X, one session against the parent (three
// slots, row pointers by register loads, PWR = 4; profiles/lxdesc_ab.json):
// SpMV with the fused dot, plan_set alternating in one process, two-slot
// 1.957-1.962, ring PWR = 4 1.614-1.616, PWR = 3 1.543-1.548 ms (-4.3 %,
// ranges apart; the parent's ring measured 1.654-1.656 in its own session).
// With PWR = 4 the headline did not move: parent 324.98-327.46, new
// 325.29-326.62 it/s, ranges overlapping -- the descriptors alone are no gain
// that can be told from noise.  With PWR = 3: parent 324.19-324.66, new
// 332.09-333.11 it/s, five alternating runs each, ranges apart (+2.5 %);
// x_sample and residual_history array_equal.  Kernel trace of the benchmark
// 1.638 -> 1.591 ms per launch; fabric reads (FETCH_SIZE, calibrated on the
// streaming dot of the same run) 7.12 -> 6.21 GB per launch -- 0.27 GB of row
// pointers, the rest surplus pieces that missed and x pieces they evicted
// (profiles/lxdesc_kernel_stats_*.csv, lxdesc_pmc_fetch_*.csv).  The ring's
// history: profiles/lxring_ab.json (two-slot 1.962 -> ring 1.655 ms; headline
// 292.95-294.65 -> 326.7-331.4 it/s).  At 128^3 (11 steps per workgroup) the
// ring LOSES, 0.0296 against 0.0270 ms -- three waits in a row in the prologue
// --, so by default it runs from 128 steps per workgroup on (lxw_ring_ok,
// which says why not from 216^3's 77 on); asked for by name it runs at any
// size, which is how the tests reach the prologue, the drain and the wrap
// with small matrices (plan key "lxw_grid_cap" gives a small matrix's
// workgroups many row blocks).
// Not tried: a fourth slot; two x pieces per wave for plans that stage at
// most eight.
//
// 4-bit value codes (template parameter VC of the ring kernel; plan key /
// context option "lx_vcode", plan arrays lx_vcode and lx_vdict): with codes
// and descriptors the fp32 values were half of what a step streams, and for
// the 7-point matrix they carry two numbers.  The plan (lxvc_encode_kernel,
// spmv_csr_forms.hip; every values bake) gives a row block whose stored
// values have at most 16 distinct BIT PATTERNS a 16-entry fp64 dictionary
// (128 B, ascending as unsigned integers, unused entries 0) and one nibble
// per entry in an array laid out exactly like the column codes; the
// instantiation runs when EVERY block has them (plan_get "lx_vcode_all") and
// the ring's other conditions hold -- the fp32 copy is not among them any
// more: a dictionary entry has the value's own bits, so values that are not
// exact in fp32 qualify too.  It takes precedence over the fp32 copy, which
// stays.
//   What a step issues now, per wave: the store and the two or three loads as
// before, then N = VR + 1 + PWR DMA instructions with VR = 1: ONE value piece
// -- the block's value codes in waves 0 and 1 (the address of the wave's
// column-code piece in the other array; a fitting block's codes fill at most
// two pieces), the block's DICTIONARY by lanes 0..7 in wave 2, a surplus piece
// by lane 0 in wave 3 --, the code piece or the descriptors, PWR x pieces;
// `s_waitcnt vmcnt(N)` as before, N = 5 for the 7-point matrix.  Per slot LDS
// holds a codes slot's bytes of value codes (1 KiB for the 7-point matrix)
// and 128 B of dictionary where 8 KiB of values were; the launch still asks
// for the fp32 ring's LDS, so that the workgroups per CU, the grid, the
// row-block order and the lane-to-row map stay what they are and y and the
// fused dot's partials keep their bits.  In the row sum v[k] is one
// ds_read_b64 of the slot's dictionary at the nibble taken from the value
// codes exactly as the column nibble is taken from the column codes (two
// dwords and a funnel shift per eight entries; sixteen doubles span 32
// banks); no fp32 -> fp64 conversion remains; multiplications, additions and
// their order are untouched.
//   Disassembly of <DOT = 1, NT = 0, TAB = 1, VR = 1, PWR = 3, VC = 1> (hipcc
// -O3 for gfx950): every step passes ONE vector-memory wait, `s_waitcnt
// vmcnt(5)` (the vmcnt(0) inside the branch of a block whose own x is not
// staged as before), then `s_waitcnt lgkmcnt(0)`, `s_barrier`; between two of
// them 1 global_store_dwordx2, 1 global_load_dwordx2, 2 global_load_dword, 5
// global_load_lds_dwordx4 (15 in the kernel: two blocks in the prologue).  70
// VGPRs, no spills, no scratch, 128 B of static LDS.
//   Measured at 512^3, one MI355X, one session against the parent (the fp32
// ring, PWR = 3; profiles/lxvcode_ab.json): the headline, five alternating
// runs each, parent 331.95-338.89, new 344.95-355.53 it/s, ranges apart
// (+3.9 % between the nearest ends, +4.5 % between the medians); the new
// sources with "lx_vcode" defaulting to 0 331.65 (the parent library's sixth
// run of the session gave 331.63); x_sample and residual_history
// array_equal.  What a launch streams: 0.47 GB of value codes + 0.07 GB of
// dictionaries where 3.75 GB of fp32 values were -- 1.07 B per entry of matrix
// stream instead of 4.5.  Kernel trace of the benchmark: 1.589 -> 1.460 ms
// per launch (-8.1 %; the byte saving does not convert one for one, the
// step stays bound by latency).  The plan pass: 7.5 ms beside
// lx4_encode_kernel's 4.7 ms; plan memory +0.47 GB of codes, +67 MB of
// dictionaries.  Not measured here: the fabric bytes (FETCH_SIZE), the
// one-process alternation at 216^3 / 384^3 (the 128-steps gate stands as it
// was).
//
// XW variant (round 5): the same kernel on the CALLER's CSR arrays as they are.
// The 16-bit offsets are a plan-owned copy of the index stream (2 B per entry
// of plan memory, 10 B per entry streamed); the plain row-block kernel streams
// the caller's arrays untouched but gathers x entry by entry -- at 512^3 x
// crossed the fabric 3.5 times (15.6 GB read for 12.9 GB of matrix + x;
// profiles/r04_pmc_csr_rowblock_spmv_*), and walking the row blocks plane by
// plane does not help it: one step of an XCD's workgroups streams 6.8 MB
// through its 4 MB L2 (2.89 against 2.91 ms, profiles/r05_rowblock_walk.log).
// XW = true streams `colind` (32 bit) by LDS-DMA where the LX form streams its
// offsets, stages the same x windows, and turns a column into its staged
// position with the block's window list (at most eight windows: a select
// chain on uniform registers; more windows: the block gathers).  Plan memory:
// 144 B per row block.
#include "csr_plan.h"
#include "lat_dma.h"

#include <new>
#include <type_traits>

namespace
{

struct LxwBlock {
  int rb;        // row block, -1 = none
  int nwin;      // >= 0 staged, -1 direct
  int32_t a;     // span start in `values`
  int32_t cnt;   // entries
  int np;        // staged pieces
  int own;       // staged position of the block's first row's OWN column
                 // (x[rb * kRows] -- the fused dot's x), -1 = not staged
  int coded;     // its offsets also exist as 4-bit codes + a dictionary
};

// A block's record travels as ONE vector load (lane l holds word l) issued a
// whole step before it is needed and is taken apart with v_readlane right
// after the step's wait.  Not scalar loads: those share their counter with
// the LDS reads, so the first LDS read of the row sums would wait for a
// record coming from HBM -- 1-2 us per step.
template <int REC>
__device__ __forceinline__ int32_t lxw_fetch(int rb,
                                             const int32_t* __restrict__ rec)
{
  int32_t w = 0;
  if (rb >= 0) {
    const int l = (int)(threadIdx.x & 63);
    w = rec[(int64_t)rb * REC + (l < REC ? l : REC - 1)];
  }
  return w;
}

__device__ __forceinline__ LxwBlock lxw_decode(int rb, int32_t w)
{
  LxwBlock b{-1, -1, 0, 0, 0, -1, 0};
  if (rb >= 0) {
    b.rb = rb;
    b.nwin = __builtin_amdgcn_readlane(w, 0);
    b.a = __builtin_amdgcn_readlane(w, 1);
    b.cnt = __builtin_amdgcn_readlane(w, 2);
    const int32_t w3 = __builtin_amdgcn_readlane(w, 3);
    b.np = w3 & kLxwNpMask;
    b.own = ((w3 >> kLxwOwnShift) & kLxwOwnMask) - 1;
    b.coded = (w3 >> kLxwCodedBit) & 1;
  }
  return b;
}

template <typename T>
struct LxwRegs {
  int32_t lo, hi; // the row's span
  T y0;
};

// (The fused dot's x_i is NOT among them: the block's own columns sit in one
// of its staged windows wherever the rows have a diagonal neighbourhood -- the
// plan records where, LxwBlock::own -- and are read from LDS in the block's own
// step.  As a second global load a step ahead it cost the kernel 15 % at 512^3:
// 2.53 against 2.19 ms, profiles/r05_rocprof_bench_n512_kernel_stats.csv.)
template <typename T>
__device__ __forceinline__ LxwRegs<T> lxw_loads(const LxwBlock& blk, int t,
                                                int32_t num_rows,
                                                const int32_t* __restrict__ rowptr,
                                                const T* __restrict__ in, T beta,
                                                const T* __restrict__ out)
{
  LxwRegs<T> g;
  g.lo = g.hi = 0;
  g.y0 = T(0);
  if (blk.rb >= 0) {
    const int32_t r = blk.rb * kRows + t;
    if (r < num_rows) {
      g.lo = rowptr[r];
      g.hi = rowptr[r + 1];
      if (beta != T(0))
        g.y0 = out[r];
    }
  }
  return g;
}

// TV = type of `values`, T = type of x, y and the arithmetic.  TV = float
// under T = double is the plan's narrowed copy of values that are exact in
// fp32 (lx_val32, padded to whole 16-byte chunks): widened in the row sum.
//   vcap   entries per values slot (slot bytes a multiple of 1 KiB)
//   lcap   entries per offsets slot
//   xcap   elements per x buffer (pieces * kLxwPiece)
//   TAB    the row-block order comes from a table (plane walk).  A template
//          parameter because the two sources of a slot's row block must not
//          share a register: a table entry is a LOADED value, and the compiler
//          waits for every load in flight -- the DMA pieces included -- before
//          it lets the computed alternative overwrite that register.
//   XW     the index stream is the caller's `colind` (lidx unused), the
//          record is the XW one (kXwRec ints: windows behind the pieces)
//   C4     != 0: a row block whose record says so streams its 4-bit codes
//          (`code`, 0.5 B per entry) into the offsets slot instead of the
//          16-bit offsets; an entry of row lane t with code c is staged at
//          t + dict[c], the dictionary being 8 words of the record.  The
//          look-up: 1 = a 32-byte LDS table per slot, written by the lanes
//          that hold those words; 2 = the words as uniform registers (taken
//          with v_readlane right after the wait, like the piece list) and a
//          select tree.  The branch is uniform per row block; 0 compiles to
//          the kernel without any of it.
template <typename TV, typename T, bool DOT, bool NT, bool TAB, bool XW, int C4>
__global__ __launch_bounds__(kBlock) void csr_lxw_kernel(
    int32_t num_rows, int32_t num_cols, int64_t nnz,
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
    const TV* __restrict__ values, const uint16_t* __restrict__ lidx,
    const uint8_t* __restrict__ code, const int32_t* __restrict__ rec, T alpha, const T* __restrict__ in, T beta,
    T* __restrict__ out, DotOut dot, RowBlockOrder ord, int vcap, int lcap,
    int xcap)
{
  using IDX = typename std::conditional<XW, int32_t, uint16_t>::type;
  constexpr int REC = XW ? kXwRec : kLxwRec;
  constexpr int IA = 16 / (int)sizeof(IDX) - 1; // index chunk alignment mask
  constexpr int V = 16 / (int)sizeof(TV); // values per 16-byte chunk
  constexpr int E = 16 / (int)sizeof(T);  // x elements per 16-byte chunk
  // lanes of one DMA instruction that cover a piece of kLxwPiece elements
  constexpr int PL = kLxwPiece / E;       // 64 (fp64), 32 (fp32)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  TV* const s_val = reinterpret_cast<TV*>(smem);
  IDX* const s_lidx
      = reinterpret_cast<IDX*>(smem + 2 * (size_t)vcap * sizeof(TV));
  T* const s_x = reinterpret_cast<T*>(smem + 2 * (size_t)vcap * sizeof(TV)
                                      + 2 * (size_t)lcap * sizeof(IDX));
  __shared__ double s_red[kBlock / 64];
  // C4 == 1: the dictionaries of the two slots, two 16-bit entries per word
  __shared__ int32_t s_dict[C4 == 1 ? 2 * kLxwDictSize / 2 : 1];
  static_assert(!(XW && C4), "the XW records carry no dictionary");

  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lane = t & 63;
  const int stride = gridDim.x;
  const int num_slots = order_slots(ord);
  double dot_acc = 0.0;
  // last aligned chunk of x that lies inside the vector
  const int32_t col_last = (num_cols - E) & ~(E - 1);

  // does the block's data sit in its LDS slots?
  auto fits = [&](const LxwBlock& b) {
    return b.cnt + (b.a & (V - 1)) <= vcap && b.cnt + (b.a & IA) <= lcap;
  };
  // does the block stream its 4-bit codes?  (they and the dword behind a
  // row's last one lie inside the offsets slot: always, by the slot's size --
  // at least 1 KiB and 2 B per entry --, checked all the same)
  auto coded = [&](const LxwBlock& b) {
    if constexpr (C4 != 0)
      return b.coded != 0
             && (b.cnt + (b.a & 31) + 7) / 8 * 4 + 8
                    <= lcap * (int)sizeof(IDX);
    else
      return false;
  };
  const int64_t code_len = lx_code_bytes(nnz);
  // entries of `values` a 16-byte chunk may touch: the caller's array ends
  // with its last entry, the plan's narrowed copy (TV = float under T =
  // double) is padded to whole chunks
  const int64_t val_len = std::is_same<TV, T>::value ? nnz : lx32_len(nnz);
  // A wave's share of a block's piece list: pieces wave, wave + 4, ... as
  // UNIFORM values, extracted from the per-lane list right after a wait -- a
  // v_readlane of a loaded register in the middle of the DMA issue would make
  // the compiler wait for everything in flight, the DMA pieces included.
  constexpr int PW = kLxwMaxPieces / (kBlock / 64); // pieces per wave
  struct Pieces {
    int32_t col[PW]; // first column of piece wave + 4 k
  };
  auto pieces_of = [&](int32_t w) { // w: the record, one word per lane
    Pieces pc;
#pragma unroll
    for (int k = 0; k < PW; ++k)
      pc.col[k] = __builtin_amdgcn_readlane(
          w, kLxwPieces0 + wave + (kBlock / 64) * k);
    return pc;
  };
  // DMA of one block's streams and windows into slot `sl`
  auto issue = [&](const LxwBlock& b, const Pieces& pc, int32_t w, int sl) {
    if (b.rb < 0 || b.cnt <= 0 || !fits(b))
      return;
    if constexpr (C4 == 1) {
      // the slot's dictionary: the lanes of wave 0 that hold its words (the
      // record has landed; the slot's readers left it before the barrier)
      if (coded(b) && t >= kLxwDict0 && t < kLxwDict0 + kLxwDictSize / 2)
        s_dict[sl * (kLxwDictSize / 2) + t - kLxwDict0] = w;
    }
    const int64_t a = b.a, e = (int64_t)b.a + b.cnt;
    lat_issue_dma<TV, NT>(values, val_len, a & ~(int64_t)(V - 1), e,
                          s_val + (size_t)sl * vcap, t);
    if (b.nwin < 0)
      return;
    if constexpr (XW)
      lat_issue_dma<int32_t, NT>(colind, nnz, a & ~(int64_t)IA, e,
                                 s_lidx + (size_t)sl * lcap, t);
    else if (coded(b))
      lat_issue_dma<uint8_t, NT>(
          code, code_len, (a >> 1) & ~(int64_t)15, (e + 1) >> 1,
          reinterpret_cast<uint8_t*>(s_lidx + (size_t)sl * lcap), t);
    else
      lat_issue_dma<uint16_t, NT>(lidx, nnz + 8, a & ~(int64_t)IA, e,
                                  s_lidx + (size_t)sl * lcap, t);
    const unsigned lds0 = (unsigned)(uintptr_t)(
        (__attribute__((address_space(3))) void*)(s_x + (size_t)sl * xcap));
#pragma unroll
    for (int k = 0; k < PW; ++k) {
      const int p = wave + (kBlock / 64) * k;
      if (p >= b.np)
        continue; // uniform
      if (lane < PL) {
        int32_t c = pc.col[k] + lane * E;
        c = c < col_last ? c : col_last; // padding past the end of x
        glds16<false>(in + c,
                      lds0 + (unsigned)(p * kLxwPiece * (int)sizeof(T)));
      }
    }
  };

  // slot -> row block (raw: before the bounds check of order_slot_decode)
  auto slot_raw = [&](int i) { return order_slot_raw_t<TAB>(ord, i, num_slots); };
  int it = blockIdx.x;
  LxwBlock cur;
  int nxt_rb;
  int32_t nxt_w; // the next block's record, in flight
  int32_t cur_w0;
  {
    const int rb0 = order_slot_decode(ord, slot_raw(it));
    nxt_rb = order_slot_decode(ord, slot_raw(it + stride));
    const int32_t w0 = lxw_fetch<REC>(rb0, rec);
    nxt_w = lxw_fetch<REC>(nxt_rb, rec);
    cur = lxw_decode(rb0, w0);
    cur_w0 = w0;
    issue(cur, pieces_of(w0), w0, 0);
  }
  int nn_raw = slot_raw(it + 2 * stride);
  LxwRegs<T> gA = lxw_loads<T>(cur, t, num_rows, rowptr, in, beta, out);
  LxwRegs<T> gB;
  int slot = 0;
  // The y of a block is STORED A STEP LATER, right after the next step's wait:
  // the wait at the top of a step covers everything the wave has in flight,
  // stores included, and a store issued at the end of a step would be waited
  // for at once -- its whole round trip exposed, every step (measured: 0.5 ms
  // of 2.47 at 512^3).
  T y_late = T(0);
  int32_t r_late = -1;

  // XW: the current block's windows as uniform values (taken from its record
  // right after a wait, like the piece list)
  struct Windows {
    int32_t f[kXwMaxWin]; // f[k]: first column of window k (f[0] unused)
    int32_t d[kXwMaxWin];
  };
  auto windows_of = [&](int32_t w) {
    Windows ws;
#pragma unroll
    for (int k = 0; k < kXwMaxWin; ++k) {
      ws.f[k] = 0;
      ws.d[k] = 0;
      if constexpr (XW) {
        if (k > 0)
          ws.f[k] = __builtin_amdgcn_readlane(w, kXwFirst0 + k - 1);
        ws.d[k] = __builtin_amdgcn_readlane(w, kXwDelta0 + k);
      }
    }
    return ws;
  };
  Windows cur_ws = windows_of(cur_w0);
  // C4 == 2: the current block's dictionary as uniform values
  struct Dict {
    int32_t w[kLxwDictSize / 2];
  };
  auto dict_of = [&](int32_t w) {
    Dict dc;
#pragma unroll
    for (int k = 0; k < kLxwDictSize / 2; ++k) {
      dc.w[k] = 0;
      if constexpr (C4 == 2)
        dc.w[k] = __builtin_amdgcn_readlane(w, kLxwDict0 + k);
    }
    return dc;
  };
  Dict cur_dc = dict_of(cur_w0);

  auto step = [&](const LxwRegs<T>& g, LxwRegs<T>& gn) {
    // everything this wave has in flight has landed; after the barrier that
    // holds for all waves, and all of them have left the previous block (the
    // builtin, not inline assembly: see spmv_lat.hip)
    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0)
    __syncthreads();
    if (r_late >= 0)
      out[r_late] = y_late;
    r_late = -1;
    const LxwBlock nxt = lxw_decode(nxt_rb, nxt_w);
    const Windows nxt_ws = windows_of(nxt_w);
    const Dict nxt_dc = dict_of(nxt_w);
    issue(nxt, pieces_of(nxt_w), nxt_w, slot ^ 1);
    gn = lxw_loads<T>(nxt, t, num_rows, rowptr, in, beta, out);
    // the block after the next one: its table entry has landed with the wait
    // above; its record is needed a step from now
    const int nn_rb = order_slot_decode(ord, nn_raw);
    const int32_t nn_w = lxw_fetch<REC>(nn_rb, rec);
    const int nnn_raw = slot_raw(it + 3 * stride);

    const int32_t r = cur.rb * kRows + t;
    if (cur.rb >= 0 && r < num_rows) {
      T sum = 0;
      T x_own = T(0);
      bool own_staged = false;
      int32_t j = g.lo;
      const int32_t hi = g.hi;
      if (cur.cnt > 0 && fits(cur)) {
        // index by the entry's position in `values`
        const TV* sv = s_val + (size_t)slot * vcap + (cur.a & (V - 1)) - cur.a;
        if (cur.nwin >= 0) {
          const IDX* sl = s_lidx + (size_t)slot * lcap + (cur.a & IA) - cur.a;
          const T* sx = s_x + (size_t)slot * xcap;
          if constexpr (DOT) {
            if (cur.own >= 0) { // uniform
              x_own = sx[cur.own + t];
              own_staged = true;
            }
          }
          if (coded(cur)) { // uniform
            // The same walk on the codes: a row's eight nibbles are two
            // aligned dwords and a funnel shift; a nibble past the row's end
            // is another row's (its position may lie outside the buffer): it
            // reads position 0 and is not added.
            const uint32_t* sc = reinterpret_cast<const uint32_t*>(
                s_lidx + (size_t)slot * lcap);
            const int32_t n0 = cur.a & ~31; // the entry of the slot's nibble 0
            for (; j < hi; j += 8) {
              const unsigned n = (unsigned)(j - n0);
              const uint32_t c_lo = sc[n >> 3], c_hi = sc[(n >> 3) + 1];
              const uint32_t bits
                  = __builtin_amdgcn_alignbit(c_hi, c_lo, (n & 7) * 4);
              unsigned l[8];
              T v[8], xv[8];
#pragma unroll
              for (int k = 0; k < 8; ++k) {
                const int32_t jj = j + k < hi ? j + k : hi - 1;
                v[k] = (T)sv[jj];
              }
#pragma unroll
              for (int k = 0; k < 8; ++k) {
                const unsigned c = (bits >> (4 * k)) & 15u;
                int32_t d;
                if constexpr (C4 == 1) {
                  d = reinterpret_cast<const int16_t*>(
                      s_dict + slot * (kLxwDictSize / 2))[c];
                } else {
                  const int32_t p0 = c & 2 ? cur_dc.w[1] : cur_dc.w[0];
                  const int32_t p1 = c & 2 ? cur_dc.w[3] : cur_dc.w[2];
                  const int32_t p2 = c & 2 ? cur_dc.w[5] : cur_dc.w[4];
                  const int32_t p3 = c & 2 ? cur_dc.w[7] : cur_dc.w[6];
                  const int32_t q0 = c & 4 ? p1 : p0;
                  const int32_t q1 = c & 4 ? p3 : p2;
                  const int32_t pr = c & 8 ? q1 : q0;
                  // low half (even code) or high half, sign-extended
                  d = (int32_t)((uint32_t)pr << (16 - 16 * (int)(c & 1))) >> 16;
                }
                l[k] = j + k < hi ? (unsigned)(t + d) : 0u;
              }
#pragma unroll
              for (int k = 0; k < 8; ++k)
                xv[k] = sx[l[k]];
#pragma unroll
              for (int k = 0; k < 8; ++k)
                if (j + k < hi)
                  sum += v[k] * xv[k];
            }
          }
          // eight entries' LDS reads in flight (offsets, then values and x:
          // two round trips per eight entries), adds strictly left to right;
          // entries past the row's end read a valid slot and are not added
          for (; j < hi; j += 8) {
            unsigned l[8];
            T v[8], xv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const int32_t jj = j + k < hi ? j + k : hi - 1;
              l[k] = sl[jj];
              v[k] = (T)sv[jj];
            }
            if constexpr (XW) {
              // column -> staged position: + the delta of the last window
              // that starts at or below it (windows ascend)
#pragma unroll
              for (int k = 0; k < 8; ++k) {
                const int32_t c = (int32_t)l[k];
                int32_t d = cur_ws.d[0];
#pragma unroll
                for (int q = 1; q < kXwMaxWin; ++q)
                  d = c >= cur_ws.f[q] ? cur_ws.d[q] : d;
                l[k] = (unsigned)(c + d);
              }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
              xv[k] = sx[l[k]];
#pragma unroll
            for (int k = 0; k < 8; ++k)
              if (j + k < hi)
                sum += v[k] * xv[k];
          }
        } else { // direct: the global gather
          for (; j < hi; ++j)
            sum += (T)sv[j] * in[colind[j]];
        }
      } else { // more entries than a slot holds: the reference loop
        for (; j < hi; ++j)
          sum += (T)values[j] * in[colind[j]];
      }
      const T c = alpha * sum;
      T y = c;
      if (beta != T(0))
        y = c + beta * g.y0;
      y_late = y;
      r_late = r;
      if constexpr (DOT) {
        if (!own_staged) // a block without a staged window over its own rows
          x_own = in[r];
        dot_acc += (double)x_own * (double)c;
      }
    }
    slot ^= 1;
    cur = nxt;
    cur_ws = nxt_ws;
    cur_dc = nxt_dc;
    nxt_rb = nn_rb;
    nxt_w = nn_w;
    nn_raw = nnn_raw;
    it += stride;
  };
  // two steps per trip: the register sets swap roles without copies
  while (it < num_slots) {
    step(gA, gB);
    if (it >= num_slots)
      break;
    step(gB, gA);
  }
  if (r_late >= 0)
    out[r_late] = y_late;
  if constexpr (DOT)
    spmv_dot_epilogue(dot, dot_acc, s_red);
}

// ---------------------------------------------------------------------------
// Ring variant: three LDS slots, two row blocks in flight (see the header).
// Every global access of the loop is inline assembly, so that the compiler
// counts none of them and adds no vmcnt wait of its own (it would wait for
// "its" loads and, the counter retiring in order, for the DMA pieces issued
// behind them); the one wait of a step is written here, with the loaded
// registers as operands so that no use can move above it.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int32_t ring_ld32(const int32_t* p)
{
  int32_t v;
  asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ double ring_ld64(const double* p)
{
  double v;
  asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ void ring_st64(double* p, double v)
{
  asm volatile("global_store_dwordx2 %0, %1, off" : : "v"(p), "v"(v) : "memory");
}
// waits until at most N of this wave's vector memory instructions are in
// flight; the registers are the loads in flight (see the kernel): five in the
// prologue, three in a step
template <int N>
__device__ __forceinline__ void ring_wait(int32_t& a, int32_t& b, double& c,
                                          int32_t& d, int32_t& e)
{
  asm volatile("s_waitcnt vmcnt(%5)"
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e)
               : "n"(N)
               : "memory");
}
template <int N>
__device__ __forceinline__ void ring_wait(double& c, int32_t& d, int32_t& e)
{
  asm volatile("s_waitcnt vmcnt(%3)"
               : "+v"(c), "+v"(d), "+v"(e)
               : "n"(N)
               : "memory");
}

//   VR    value pieces (1 KiB each) a wave issues per step: a values slot is
//         VR * 4 KiB
//   PWR   x pieces a wave issues per step
//   ccap  bytes per codes slot (whole KiB, at most 4: one piece per wave)
//   xcap  elements per x buffer (at most 4 * PWR pieces)
// A wave issues VR + 1 + PWR DMA instructions per row block, whatever the
// block needs: a piece beyond its data (and every piece of a slot without a
// row block) reads the head of its array and lands in the dump area behind
// the slots.  The "+ 1" is a code piece in waves 0, 1 and 3 and the
// block's row descriptors (`desc`, csr_plan.h) in wave kRingDescWave: a
// fitting block's codes fill at most two pieces, so that wave's code piece
// was surplus in every block.
constexpr int kRingDescWave = 2;
// A surplus piece is issued by lane 0 alone (the other lanes sit it out: the
// instruction still issues and is still counted), so the dump area holds one
// lane's 16 bytes, not a piece.
constexpr int kRingDumpBytes = 64;
static_assert(lx_ring_code_bytes(kLxwRingVcap - 3) <= kRingDescWave * 1024,
              "a fitting block's codes reach the descriptor wave's piece");
//   VC    the values arrive as 4-bit codes and a per-block fp64 dictionary
//         (`vcode`, `vdict`; csr_plan.h) instead of fp32 numbers, VR = 1: a
//         value-codes slot is a codes slot's size (`ccap`: the two streams of
//         a block have the same layout and share their DMA addresses), the
//         block's 128-B dictionary rides in wave kRingDescWave's value piece
//         by eight lanes (a fitting block's value codes fill at most two
//         pieces, like its column codes), and wave 3's value piece is surplus
//         in every block.  `values` is not read.
template <bool DOT, bool NT, bool TAB, int VR, int PWR, bool VC>
__global__ __launch_bounds__(kBlock) void csr_lxw_ring_kernel(
    int32_t num_rows, int32_t num_cols, int64_t nnz,
    const float* __restrict__ values, const uint8_t* __restrict__ vcode,
    const double* __restrict__ vdict, const uint8_t* __restrict__ code,
    const uint16_t* __restrict__ desc, const int32_t* __restrict__ rec,
    double alpha, const double* __restrict__ in, double beta,
    double* __restrict__ out, DotOut dot, RowBlockOrder ord, int ccap, int xcap)
{
  using T = double;
  static_assert(!VC || VR == 1, "value codes: one value piece per wave");
  constexpr int NW = kBlock / 64;
  constexpr int VCAP = VR * NW * 256; // floats per values slot (!VC)
  constexpr int DMA = VR + 1 + PWR;   // DMA instructions per wave and block
  constexpr int DB = kLxVcDictSize * (int)sizeof(double); // dictionary bytes
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // the values' slots: fp32 numbers, or (VC) three slots of value codes and
  // behind them the three dictionaries
  const unsigned val_bytes
      = VC ? 3u * ((unsigned)ccap + DB) : 3u * VCAP * (unsigned)sizeof(float);
  float* const s_val = reinterpret_cast<float*>(smem);
  const unsigned char* const s_vcode = smem;
  const double* const s_vdict
      = reinterpret_cast<const double*>(smem + 3 * (size_t)ccap);
  unsigned char* const s_code = smem + val_bytes;
  T* const s_x = reinterpret_cast<T*>(s_code + 3 * (size_t)ccap);
  // row descriptors: 512 B per slot (half a DMA piece: lanes 0..31)
  const uint16_t* const s_desc = reinterpret_cast<const uint16_t*>(
      reinterpret_cast<unsigned char*>(s_x) + 3 * (size_t)xcap * sizeof(T));
  __shared__ double s_red[NW];
  __shared__ int32_t s_dict[3 * kLxwDictSize / 2];
  const unsigned lds_val = (unsigned)(uintptr_t)(
      (__attribute__((address_space(3))) void*)s_val);
  const unsigned lds_vdict = lds_val + 3u * (unsigned)ccap; // (VC)
  const unsigned lds_code = lds_val + val_bytes;
  const unsigned lds_x = lds_code + 3u * (unsigned)ccap;
  const unsigned lds_desc = lds_x + 3u * (unsigned)xcap * (unsigned)sizeof(T);
  const unsigned lds_dump = lds_desc + 3u * (unsigned)(kRows * 2);

  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lane = t & 63;
  const int stride = gridDim.x;
  const int num_slots = order_slots(ord);
  double dot_acc = 0.0;
  const int32_t col_last = (num_cols - 2) & ~1;
  const int64_t code_len = lx_code_bytes(nnz);
  const int64_t val_len = lx32_len(nnz);
  // where a surplus piece reads: the head of the array, inside it
  const int64_t vdump = lane * 4 < val_len - 4 ? lane * 4 : val_len - 4;
  const int64_t cdump = lane * 16 < code_len - 16 ? lane * 16 : code_len - 16;
  const int32_t xdump = lane * 2 < col_last ? lane * 2 : col_last;

  // DMA of block b into slot sl: exactly DMA instructions, none under a branch
  auto issue = [&](const LxwBlock& b, int32_t w, int sl) {
    const bool live = b.rb >= 0;
    const int64_t a = b.a, e = (int64_t)b.a + b.cnt;
    if constexpr (!VC) {
      const int64_t base = a & ~(int64_t)3;
      const int64_t jclamp = (e - 1) & ~(int64_t)3;
      const int pieces = live ? (int)(((e - base) * 4 + 1023) >> 10) : 0;
#pragma unroll
      for (int r = 0; r < VR; ++r) {
        const int q = wave + NW * r;
        const bool real = q < pieces; // uniform
        int64_t j = base + (int64_t)(q * 64 + lane) * 4;
        j = j < jclamp ? j : jclamp;
        j = real ? j : vdump;
        // (a surplus piece: lane 0 alone -- issued, counted, 16 B written)
        if (lane < (real ? 64 : 1))
          glds16<NT>(values + j,
                     real ? lds_val + (unsigned)(sl * VCAP * 4 + q * 1024)
                          : lds_dump);
      }
    }
    {
      const int64_t base = (a >> 1) & ~(int64_t)15, end = (e + 1) >> 1;
      const int64_t jclamp = (end - 1) & ~(int64_t)15;
      const int pieces = live ? (int)((end - base + 1023) >> 10) : 0;
      const bool real = wave < pieces; // uniform
      int64_t j = base + (int64_t)(wave * 64 + lane) * 16;
      j = j < jclamp ? j : jclamp;
      j = real ? j : cdump;
      const bool dsc = wave == kRingDescWave; // uniform
      if constexpr (VC) {
        // the value codes: the column codes' piece of the other array; wave
        // kRingDescWave: the block's dictionary instead (no block: that of
        // row block 0), by its lanes 0..7
        const uint8_t* const vsrc
            = dsc ? reinterpret_cast<const uint8_t*>(
                        vdict + (int64_t)(live ? b.rb : 0) * kLxVcDictSize)
                        + (lane & 7) * 16
                  : vcode + j;
        if (lane < (dsc ? DB / 16 : real ? 64 : 1))
          glds16<NT>(vsrc, dsc ? lds_vdict + (unsigned)(sl * DB)
                               : real ? lds_val + (unsigned)(sl * ccap + wave * 1024)
                                      : lds_dump);
      }
      // wave kRingDescWave: the block's 512 B of row descriptors instead (no
      // block: those of row block 0), by its lanes 0..31 -- the others sit the
      // instruction out, so it writes half a piece; never all lanes of a
      // wave, so the instruction is always issued and always counted
      const uint8_t* const src
          = dsc ? reinterpret_cast<const uint8_t*>(desc)
                      + (int64_t)(live ? b.rb : 0) * (kRows * 2) + (lane & 31) * 16
                : code + j;
      if (lane < (dsc ? 32 : real ? 64 : 1))
        glds16<NT>(src, dsc ? lds_desc + (unsigned)(sl * (kRows * 2))
                            : real ? lds_code + (unsigned)(sl * ccap + wave * 1024)
                                   : lds_dump);
    }
    const int np = live ? b.np : 0;
#pragma unroll
    for (int k = 0; k < PWR; ++k) {
      const int p = wave + NW * k;
      const bool real = p < np; // uniform
      // (the piece list of the record, taken after its wait)
      const int32_t col = __builtin_amdgcn_readlane(w, kLxwPieces0 + p);
      int32_t c = col + lane * 2;
      c = c < col_last ? c : col_last; // padding past the end of x
      c = real ? c : xdump;
      if (lane < (real ? 64 : 1))
        glds16<false>(in + c,
                      real ? lds_x + (unsigned)((sl * xcap + p * kLxwPiece) * 8)
                           : lds_dump);
    }
  };
  // the slot's dictionary: the lanes of wave 0 that hold its words
  auto put_dict = [&](const LxwBlock& b, int32_t w, int sl) {
    if (b.rb >= 0 && t >= kLxwDict0 && t < kLxwDict0 + kLxwDictSize / 2)
      s_dict[sl * (kLxwDictSize / 2) + t - kLxwDict0] = w;
  };
  // slot -> row block: the table entry as a load in flight (clamped; decode
  // checks the slot), or computed
  auto raw_of = [&](int i) {
    if constexpr (TAB)
      return ring_ld32(ord.table + (i < num_slots ? i : num_slots - 1));
    else
      return order_slot_raw_t<false>(ord, i, num_slots);
  };
  auto rb_of = [&](int i, int raw) {
    return i < num_slots ? order_slot_decode(ord, raw) : -1;
  };
  // a block's record, one word per lane (no block: record 0, ignored)
  auto fetch = [&](int rb) {
    return ring_ld32(rec + (int64_t)(rb < 0 ? 0 : rb) * kLxwRec
                     + (lane < kLxwRec ? lane : kLxwRec - 1));
  };
  // a block's y: always one load, of a row that exists; beta == 0 reads the
  // head of y instead of streaming it
  auto loads = [&](int rb, double& y0) {
    int32_t r = (rb < 0 ? 0 : rb) * kRows + t;
    r = r < num_rows ? r : num_rows - 1;
    y0 = ring_ld64(out + (beta != 0.0 ? r : (t < num_rows ? t : num_rows - 1)));
  };

  int it = blockIdx.x;
  // prologue: blocks k and k + 1 issued, the record of k + 2 and the table
  // entry of k + 3 landed -- each stage behind a vmcnt(0)
  int32_t raw0 = raw_of(it), raw1 = raw_of(it + stride);
  int32_t raw2 = raw_of(it + 2 * stride), raw3 = raw_of(it + 3 * stride);
  double dz = 0.0;
  ring_wait<0>(raw0, raw1, dz, raw2, raw3);
  const int rb0 = rb_of(it, raw0), rb1 = rb_of(it + stride, raw1);
  int rb2 = rb_of(it + 2 * stride, raw2);
  int32_t w0 = fetch(rb0), w1 = fetch(rb1), w2 = fetch(rb2);
  int32_t iz = 0;
  ring_wait<0>(w0, w1, dz, w2, iz);
  LxwBlock cur = lxw_decode(rb0, w0);
  LxwBlock nxt = lxw_decode(rb1, w1);
  put_dict(cur, w0, 0);
  put_dict(nxt, w1, 1);
  issue(cur, w0, 0);
  issue(nxt, w1, 1);
  double y0;
  loads(cur.rb, y0);
  ring_wait<0>(y0, iz, iz);
  __syncthreads();
  int s0 = 0, s2 = 2; // slots of block k and of block k + 2
  T y_late = T(0);
  int32_t r_late = -1;

  // Step k.  In flight on entry: nothing but the DMA of block k + 1 (DMA
  // instructions).  Issued here, in this order: the late y store of block
  // k - 1; the y of block k + 1 (1), the record of block
  // k + 3 (1), the table entry of block k + 4 (TAB: 1); the DMA of block k + 2
  // (DMA).  The wait at the end leaves the youngest DMA instructions in
  // flight -- block k + 2's --: the counter retires in order, so everything
  // issued before them has landed, block k + 1 included.  What precedes the
  // DMA may be skipped (the store: a wave without rows) without harm, since
  // it is older than what is waited for; the DMA itself is never skipped.
  while (it < num_slots) {
    if (r_late >= 0)
      ring_st64(out + r_late, y_late);
    r_late = -1;
    double ny0;
    loads(nxt.rb, ny0);
    const int rb3 = rb_of(it + 3 * stride, raw3);
    int32_t w3 = fetch(rb3);
    int32_t raw4 = raw_of(it + 4 * stride);
    const LxwBlock blk2 = lxw_decode(rb2, w2);
    put_dict(blk2, w2, s2); // (block k - 1's readers left before the barrier)
    issue(blk2, w2, s2);

    const int32_t r = cur.rb * kRows + t;
    if (cur.rb >= 0 && r < num_rows) {
      T sum = 0;
      T x_own = T(0);
      // the row's span: its descriptor (landed with the block's DMA) + cur.a
      const int32_t dsc = s_desc[s0 * kRows + t];
      int32_t j = cur.a + (dsc & kLxwDescStartMask);
      const int32_t hi = j + (dsc >> kLxwDescStartBits);
      // index by the entry's position in `values`
      const float* sv = s_val + (size_t)s0 * VCAP + (cur.a & 3) - cur.a;
      // (VC) the slot's value codes, laid out like its column codes, and its
      // dictionary
      const uint32_t* svc
          = reinterpret_cast<const uint32_t*>(s_vcode + (size_t)s0 * ccap);
      const T* sd = s_vdict + s0 * kLxVcDictSize;
      const T* sx = s_x + (size_t)s0 * xcap;
      if constexpr (DOT) {
        if (cur.own >= 0) // uniform
          x_own = sx[cur.own + t];
      }
      // the walk of csr_lxw_kernel on the codes, operation for operation
      const uint32_t* sc
          = reinterpret_cast<const uint32_t*>(s_code + (size_t)s0 * ccap);
      const int32_t n0 = cur.a & ~31; // the entry of the slot's nibble 0
      for (; j < hi; j += 8) {
        const unsigned n = (unsigned)(j - n0);
        const uint32_t c_lo = sc[n >> 3], c_hi = sc[(n >> 3) + 1];
        const uint32_t bits = __builtin_amdgcn_alignbit(c_hi, c_lo, (n & 7) * 4);
        unsigned l[8];
        T v[8], xv[8];
        if constexpr (VC) {
          // a value is its nibble's dictionary entry (a nibble past the row's
          // end is another row's: any of the 16 entries, not added)
          const uint32_t v_lo = svc[n >> 3], v_hi = svc[(n >> 3) + 1];
          const uint32_t vbits
              = __builtin_amdgcn_alignbit(v_hi, v_lo, (n & 7) * 4);
#pragma unroll
          for (int k = 0; k < 8; ++k)
            v[k] = sd[(vbits >> (4 * k)) & 15u];
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int32_t jj = j + k < hi ? j + k : hi - 1;
            v[k] = (T)sv[jj];
          }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const unsigned c = (bits >> (4 * k)) & 15u;
          const int32_t d = reinterpret_cast<const int16_t*>(
              s_dict + s0 * (kLxwDictSize / 2))[c];
          l[k] = j + k < hi ? (unsigned)(t + d) : 0u;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
          xv[k] = sx[l[k]];
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (j + k < hi)
            sum += v[k] * xv[k];
      }
      const T c = alpha * sum;
      T y = c;
      if (beta != T(0))
        y = c + beta * y0;
      y_late = y;
      r_late = r;
      if constexpr (DOT) {
        if (cur.own < 0) { // no staged window over the block's own rows
          // (waited for at once, inside the branch: a load the compiler
          // counted would put its vmcnt(0) behind the join, in every step)
          x_own = ring_ld64(in + r);
          asm volatile("s_waitcnt vmcnt(0)" : "+v"(x_own) : : "memory");
        }
        dot_acc += (double)x_own * (double)c;
      }
    }
    ring_wait<DMA>(ny0, w3, raw4);
    __syncthreads();
    cur = nxt;
    nxt = blk2;
    y0 = ny0;
    rb2 = rb3;
    w2 = w3;
    raw3 = raw4;
    s2 = s0;
    s0 = s0 == 2 ? 0 : s0 + 1;
    it += stride;
  }
  // the DMA of the blocks that do not exist (dump area) is still in flight
  ring_wait<0>(y0, w2, raw3);
  if (r_late >= 0)
    ring_st64(out + r_late, y_late);
  if constexpr (DOT)
    spmv_dot_epilogue(dot, dot_acc, s_red);
}

struct LxwGeom {
  int vcap, lcap, xcap;
  size_t lds;
  int per_cu;
};

// idx_bytes: 2 (the LX form's offsets) or 4 (XW: the caller's column indices)
LxwGeom lxw_geom(const spmv_hip_csr_plan* pl, int elem_bytes, int idx_bytes)
{
  LxwGeom g;
  const bool xw = idx_bytes == 4;
  const int V = 16 / elem_bytes;
  const int max_cnt = xw ? pl->xw_max_cnt : pl->lxw_max_cnt;
  // slot for the largest staged block plus the slack of the 16-byte alignment
  // of its first chunk, in whole 1-KiB DMA pieces; at most 32 KiB
  int64_t vb = ((int64_t)(max_cnt + V) * elem_bytes + 1023) & ~1023ll;
  vb = vb < 1024 ? 1024 : (vb > 32768 ? 32768 : vb);
  g.vcap = (int)(vb / elem_bytes);
  int64_t lb = ((int64_t)(g.vcap + 8) * idx_bytes + 1023) & ~1023ll;
  g.lcap = (int)(lb / idx_bytes);
  int np = xw ? pl->xw_max_pieces : pl->lxw_max_pieces;
  np = np < 1 ? 1 : np;
  g.xcap = np * kLxwPiece;
  g.lds = 2 * (size_t)vb + 2 * (size_t)lb + 2 * (size_t)g.xcap * elem_bytes;
  int per = (int)((160 * 1024 - 1024) / (g.lds + 64));
  per = per < 1 ? 1 : (per > kBlocksPerCU ? kBlocksPerCU : per);
  if (pl->lxw_blocks_per_cu > 0 && pl->lxw_blocks_per_cu < per)
    per = pl->lxw_blocks_per_cu;
  g.per_cu = per;
  return g;
}

int lxw_grid(const spmv_hip_csr_plan* pl, int elem_bytes, int idx_bytes)
{
  const LxwGeom g = lxw_geom(pl, elem_bytes, idx_bytes);
  const int nrb = (pl->num_rows + kRows - 1) / kRows;
  int grid = pl->ctx->num_cus * g.per_cu;
  if (grid > pl->ctx->dot_blocks)
    grid = pl->ctx->dot_blocks;
  if (grid > nrb)
    grid = nrb;
  if (pl->lxw_grid_cap > 0 && grid > pl->lxw_grid_cap)
    grid = pl->lxw_grid_cap; // (tests: many steps per workgroup, small matrix)
  if (grid < 1)
    grid = 1;
  if (grid >= 8)
    grid -= grid % 8;
  return grid;
}

// The ring kernel's slots for this plan: a values slot is fixed (VR pieces
// per wave), the codes slot holds the largest block's codes, the x buffer the
// most pieces a block stages; the dump area follows.
struct LxwRingGeom {
  int ccap, xcap;
  size_t lds;
  int per_cu; // workgroups per CU that its LDS allows
};

LxwRingGeom lxw_ring_geom(const spmv_hip_csr_plan* pl)
{
  LxwRingGeom g;
  const int max_cnt = pl->lxw_max_cnt < 1 ? 1 : pl->lxw_max_cnt;
  g.ccap = (lx_ring_code_bytes(max_cnt) + 1023) & ~1023;
  int np = pl->lxw_max_pieces;
  np = np < 1 ? 1 : np;
  g.xcap = np * kLxwPiece;
  g.lds = 3 * ((size_t)kLxwRingVcap * sizeof(float) + (size_t)g.ccap
               + (size_t)g.xcap * sizeof(double) + kRows * 2) // (descriptors)
          + kRingDumpBytes;
  // (static LDS: the reduction buffer and three dictionaries, 128 B)
  g.per_cu = (int)((160 * 1024 - 1024) / (g.lds + 256));
  return g;
}

// Per plan, never per block: value codes for every row block or narrowed
// values (the launch prefers the codes), codes with the LDS table, every
// row block staged, coded and fitting, and three slots in the LDS that keeps
// the workgroups per CU where lxw_geom puts them.
// every row block has value codes and they are switched on
bool lxw_vcode_on(const spmv_hip_csr_plan* pl)
{
  const int nrb = (pl->num_rows + kRows - 1) / kRows;
  return pl->lx_vc && pl->lx_vcode && pl->lx_vdict && pl->lx_vc_values0
         && pl->lx_vcode_blocks == nrb;
}

bool lxw_ring_ok(const spmv_hip_csr_plan* pl, bool forced)
{
  const int nrb = (pl->num_rows + kRows - 1) / kRows;
  // (the values: as codes and dictionaries, or narrowed)
  if (!(forced || pl->lx_ring) || pl->symmetric || !pl->lx || !pl->lxw
      || !pl->lxw_rec || !pl->lx4 || !pl->lx_code || pl->lx4_lut != 1
      || !((pl->lx_v32 && pl->lx_val32) || lxw_vcode_on(pl)) || !pl->lx_rowdesc)
    return false;
  if (nrb < 1 || pl->lx_staged != nrb || pl->lx4_blocks != nrb
      || pl->lx_ring_blocks != nrb || !lx_ring_fits(pl->lxw_max_cnt)
      || pl->lxw_max_pieces > kLxwMaxPieces)
    return false;
  if (lxw_ring_geom(pl).per_cu < lxw_geom(pl, 8, 2).per_cu)
    return false;
  // Gate on the row blocks a workgroup walks: the ring's prologue (three
  // waits in a row) is paid once per launch and the gain once per step.
  // Measured (fused dot, one process, plan_set alternating): 11 steps (128^3)
  // 0.0296 against 0.0270 ms; 77 steps (216^3) 0.127 against 0.157 ms; 432
  // (384^3) 0.670 against 0.823; 1024 (512^3) 1.655 against 1.962.  The
  // default starts at 128 steps, above 216^3 although the ring gains there:
  // the benchmark's 216^3 record prices the launch in CSR bytes against the
  // HBM peak and the suite bounds that fraction below 1, which 0.127 ms
  // exceeds (1.06) with x and part of the matrix in the Infinity Cache.
  // Asked for by name (plan_set "lx_ring" 1, context option 2) it runs
  // regardless.
  constexpr int kMinSteps = 128;
  const int grid = lxw_grid(pl, 8, 2);
  return forced || pl->lx_ring >= 2 || (nrb + grid - 1) / grid >= kMinSteps;
}

// VC: the value-coded instantiation (`values` unused).  It asks for the LDS of
// the fp32 one although its slots are smaller (1 KiB of value codes and a
// 128-B dictionary where 8 KiB of values were): the workgroups per CU, and
// with them how the grid spreads over the CUs, stay what they are.
template <bool DOT, int PWR, bool VC>
int lxw_ring_launch_p(const spmv_hip_csr_plan* pl, hipStream_t st,
                      const float* values, double alpha, const double* in,
                      double beta, double* out, DotOut dot)
{
  constexpr int VR = VC ? 1 : kLxwRingValRounds;
  const LxwRingGeom g = lxw_ring_geom(pl);
  const int nrb = (pl->num_rows + kRows - 1) / kRows;
  // grid and row-block order: those of csr_lxw_kernel, so that y and the fused
  // dot's partials keep their bits
  const int grid = lxw_grid(pl, 8, 2);
  RowBlockOrder ord = pl->row_block_order(nrb);
  ord.xcd_group = pl->lat_xcd_group;
  if (pl->zwalk && pl->zw_table && pl->zw_grid == grid) {
    ord.table = pl->zw_table;
    ord.num_slots = pl->zw_slots;
  }
  auto kern
      = ord.table
            ? (pl->nontemporal ? csr_lxw_ring_kernel<DOT, true, true, VR, PWR, VC>
                               : csr_lxw_ring_kernel<DOT, false, true, VR, PWR, VC>)
            : (pl->nontemporal ? csr_lxw_ring_kernel<DOT, true, false, VR, PWR, VC>
                               : csr_lxw_ring_kernel<DOT, false, false, VR, PWR, VC>);
  if (g.lds > 48 * 1024) // beyond the default dynamic-LDS limit
    SPMV_CHECK_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), g.lds, st, pl->num_rows,
                     pl->num_cols, pl->nnz, values, pl->lx_vcode, pl->lx_vdict,
                     pl->lx_code, pl->lx_rowdesc, pl->lxw_rec, alpha, in, beta, out,
                     dot, ord, g.ccap, g.xcap);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

// x pieces per wave: kLxwMaxPieces / 4 covers every plan; one fewer where the
// plan stages at most twelve pieces (the 7-point matrix: 11), unless the plan
// key "lx_ring_pwr" asks for all four -- one DMA instruction less per wave
// and step, `s_waitcnt vmcnt(6)` (value codes: vmcnt(5))
template <bool DOT, bool VC>
int lxw_ring_launch(const spmv_hip_csr_plan* pl, hipStream_t st,
                    const float* values, double alpha, const double* in,
                    double beta, double* out, DotOut dot)
{
  constexpr int NW = kBlock / 64, PWR = kLxwMaxPieces / NW;
  if (pl->lx_ring_pwr != PWR && pl->lxw_max_pieces <= (PWR - 1) * NW)
    return lxw_ring_launch_p<DOT, PWR - 1, VC>(pl, st, values, alpha, in, beta,
                                               out, dot);
  return lxw_ring_launch_p<DOT, PWR, VC>(pl, st, values, alpha, in, beta, out,
                                         dot);
}

template <typename TV, typename T, bool DOT, bool XW, int C4>
int lxw_launch_c(const spmv_hip_csr_plan* pl, hipStream_t st,
                 const int32_t* rowptr, const int32_t* colind, const TV* values,
                 T alpha, const T* in, T beta, T* out, DotOut dot)
{
  // (the geometry does not depend on C4: the codes take a quarter of the
  // offsets slot, and the grid, the row-block order and with them the fused
  // dot's partials stay what they are without the codes)
  // (nor on TV: narrowed values run in the slots of T -- the same bytes per
  // values slot, so the offsets slot and the x buffer start where they do for
  // TV = T, and a slot holds sizeof(T) / sizeof(TV) times the entries: a block
  // that fits the fp64 slot fits, and `a & 3` entries of alignment slack with)
  const LxwGeom g = lxw_geom(pl, (int)sizeof(T), XW ? 4 : 2);
  const int vcap = g.vcap * (int)(sizeof(T) / sizeof(TV));
  const int nrb = (pl->num_rows + kRows - 1) / kRows;
  const int grid = lxw_grid(pl, (int)sizeof(T), XW ? 4 : 2);
  RowBlockOrder ord = pl->row_block_order(nrb);
  ord.xcd_group = pl->lat_xcd_group;
  if (pl->zwalk && pl->zw_table && pl->zw_grid == grid) {
    ord.table = pl->zw_table;
    ord.num_slots = pl->zw_slots;
  }
  auto kern
      = ord.table
            ? (pl->nontemporal ? csr_lxw_kernel<TV, T, DOT, true, true, XW, C4>
                               : csr_lxw_kernel<TV, T, DOT, false, true, XW, C4>)
            : (pl->nontemporal ? csr_lxw_kernel<TV, T, DOT, true, false, XW, C4>
                               : csr_lxw_kernel<TV, T, DOT, false, false, XW, C4>);
  if (g.lds > 48 * 1024) // beyond the default dynamic-LDS limit
    SPMV_CHECK_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), g.lds, st, pl->num_rows,
                     pl->num_cols, pl->nnz, rowptr, colind, values,
                     XW ? nullptr : pl->lx_lidx, C4 ? pl->lx_code : nullptr,
                     XW ? pl->xw_rec : pl->lxw_rec, alpha, in, beta, out, dot,
                     ord, vcap, g.lcap, g.xcap);
  SPMV_CHECK_LAUNCH();
  return SPMV_HIP_OK;
}

template <typename TV, typename T, bool DOT, bool XW>
int lxw_launch(const spmv_hip_csr_plan* pl, hipStream_t st,
               const int32_t* rowptr, const int32_t* colind, const TV* values,
               T alpha, const T* in, T beta, T* out, DotOut dot)
{
  if constexpr (!XW && std::is_same<TV, float>::value
                && std::is_same<T, double>::value) {
    if (lxw_ring_ok(pl, false))
      return lxw_ring_launch<DOT, false>(pl, st, values, alpha, in, beta, out,
                                         dot);
  }
  if constexpr (!XW) {
    if (pl->lx4 && pl->lx_code)
      return pl->lx4_lut == 2
                 ? lxw_launch_c<TV, T, DOT, XW, 2>(pl, st, rowptr, colind, values,
                                                   alpha, in, beta, out, dot)
                 : lxw_launch_c<TV, T, DOT, XW, 1>(pl, st, rowptr, colind, values,
                                                   alpha, in, beta, out, dot);
  }
  return lxw_launch_c<TV, T, DOT, XW, 0>(pl, st, rowptr, colind, values, alpha,
                                         in, beta, out, dot);
}

} // namespace

int spmv_lxw_grid(const spmv_hip_csr_plan* pl, int elem_bytes)
{
  return lxw_grid(pl, elem_bytes, 2);
}

bool spmv_lxw_ring_ok(const spmv_hip_csr_plan* pl, bool forced)
{
  return lxw_ring_ok(pl, forced);
}

bool spmv_lxw_vcode_ok(const spmv_hip_csr_plan* pl)
{
  return lxw_vcode_on(pl) && lxw_ring_ok(pl, false);
}

int spmv_lxw_run_vcode(const spmv_hip_csr_plan* pl, hipStream_t st, double alpha,
                       const double* in, double beta, double* out, DotOut dot)
{
  if (dot.partials)
    return lxw_ring_launch<true, true>(pl, st, nullptr, alpha, in, beta, out, dot);
  return lxw_ring_launch<false, true>(pl, st, nullptr, alpha, in, beta, out, dot);
}

int spmv_xw_grid(const spmv_hip_csr_plan* pl, int elem_bytes)
{
  return lxw_grid(pl, elem_bytes, 4);
}

int spmv_lxw_run_f64(const spmv_hip_csr_plan* pl, hipStream_t st,
                     const int32_t* rowptr, const int32_t* colind,
                     const double* values, double alpha, const double* in,
                     double beta, double* out, DotOut dot)
{
  if (dot.partials)
    return lxw_launch<double, double, true, false>(pl, st, rowptr, colind, values,
                                                   alpha, in, beta, out, dot);
  return lxw_launch<double, double, false, false>(pl, st, rowptr, colind, values,
                                                  alpha, in, beta, out, dot);
}

// `values`: the plan's narrowed copy (lx_val32) of the fp64 values
int spmv_lxw_run_f32f64(const spmv_hip_csr_plan* pl, hipStream_t st,
                        const int32_t* rowptr, const int32_t* colind,
                        const float* values, double alpha, const double* in,
                        double beta, double* out, DotOut dot)
{
  if (dot.partials)
    return lxw_launch<float, double, true, false>(pl, st, rowptr, colind, values,
                                                  alpha, in, beta, out, dot);
  return lxw_launch<float, double, false, false>(pl, st, rowptr, colind, values,
                                                 alpha, in, beta, out, dot);
}

int spmv_lxw_run_f32(const spmv_hip_csr_plan* pl, hipStream_t st,
                     const int32_t* rowptr, const int32_t* colind,
                     const float* values, float alpha, const float* in,
                     float beta, float* out)
{
  return lxw_launch<float, float, false, false>(pl, st, rowptr, colind, values,
                                                alpha, in, beta, out, DotOut());
}

int spmv_xw_run_f64(const spmv_hip_csr_plan* pl, hipStream_t st,
                    const int32_t* rowptr, const int32_t* colind,
                    const double* values, double alpha, const double* in,
                    double beta, double* out, DotOut dot)
{
  if (dot.partials)
    return lxw_launch<double, double, true, true>(pl, st, rowptr, colind, values,
                                                  alpha, in, beta, out, dot);
  return lxw_launch<double, double, false, true>(pl, st, rowptr, colind, values,
                                                 alpha, in, beta, out, dot);
}

int spmv_xw_run_f32(const spmv_hip_csr_plan* pl, hipStream_t st,
                    const int32_t* rowptr, const int32_t* colind,
                    const float* values, float alpha, const float* in,
                    float beta, float* out)
{
  return lxw_launch<float, float, false, true>(pl, st, rowptr, colind, values,
                                               alpha, in, beta, out, DotOut());
}
