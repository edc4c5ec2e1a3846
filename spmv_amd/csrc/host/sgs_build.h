// Host half of the multicolour symmetric Gauss-Seidel preconditioner
// (spmv::SgsPreconditioner, cg.h): the colouring, the colour-major copy of the
// local diagonal block and its sliced device layout.  Plain C++17, no device,
// no other header of the mirror: tools/sgs_build_check.cpp compiles this file
// pair alone under the sanitizers.
//
// Input form (both entry points): the rows of this rank as CSR with local
// column numbers.  An entry (i, c) belongs to the local diagonal block when
// c < ncols_local; c == i is the diagonal; symmetric input: only c < i is an
// off-diagonal entry (entries above the diagonal are dropped, as create_matrix
// does) and the block stands for B + B^T.  nrows != ncols_local throws.
#pragma once

#include <cstdint>
#include <vector>

namespace spmv
{

// One of the two parts of every row, CSR over POSITIONS (colour-major rows):
// row perm[pos] owns the entries ptr[pos] .. ptr[pos + 1], ascending by column,
// duplicates of one column in storage order; columns in the caller's numbering.
struct SgsCsrPart {
  std::vector<int64_t> ptr = {0};
  std::vector<int32_t> col;
  std::vector<double> val;
};

struct SgsHostPlan {
  int32_t n = 0;
  int32_t num_colors = 0;
  std::vector<int32_t> colors;      // n: colour of row i
  std::vector<int32_t> perm;        // n: perm[pos] = row, colour-major
  std::vector<int32_t> color_start; // num_colors + 1 positions
  std::vector<double> d;            // n: the diagonal (Matrix::diagonal's rule)
  SgsCsrPart before, after;         // column's colour < / > the row's colour
};

// A part as the kernels of spmv_mcgs.hip read it.  The rows of a colour are
// cut into slices of 64 consecutive positions (the last slice of a colour may
// be short; no slice spans two colours).  Slice s stores its entries
// column-major: entry k of lane l at slice_ptr[s] + 64 * k + l, k below the
// slice's width = the longest row in it; lanes with fewer entries are padded
// (column 0, value 0) and never read past len[pos].  A row with more than
// `long_threshold` entries in this part keeps len[pos] = -1 and goes to the
// long list instead: entries contiguous, one wavefront per row.
struct SgsSlicedPart {
  std::vector<int32_t> color_slice; // num_colors + 1: first slice of a colour
  std::vector<int32_t> slice_pos0;  // first position of a slice
  std::vector<int64_t> slice_ptr;   // slices + 1
  std::vector<int32_t> len;         // n, by position; -1: long row
  std::vector<int32_t> col;
  std::vector<double> val;
  std::vector<int32_t> color_long;  // num_colors + 1: first long row of a colour
  std::vector<int32_t> long_pos;    // position of a long row
  std::vector<int64_t> long_ptr;    // long rows + 1
  std::vector<int32_t> long_col;
  std::vector<double> long_val;
};

constexpr int kSgsLongThreshold = 64;

// Greedy colouring in natural row order over the pattern of B + B^T, B the
// local diagonal block without its diagonal: colour(i) = the smallest colour
// not worn by a neighbour j < i.  Deterministic.  Returns the colours;
// *num_colors (optional) = their number (0 for an empty matrix).
std::vector<int32_t> sgs_color(const int32_t* rowptr, const int32_t* colind,
                               int64_t nrows, int64_t ncols_local,
                               bool symmetric, int* num_colors = nullptr);

// The colouring plus the colour-major copy.  `diagonal` (optional, nrows
// entries) replaces the sum of the entries (i, i) in storage order -- symmetric
// storage keeps its diagonal in an array of its own.
SgsHostPlan sgs_build(const int32_t* rowptr, const int32_t* colind,
                      const double* values, const double* diagonal,
                      int64_t nrows, int64_t ncols_local, bool symmetric);

SgsSlicedPart sgs_slice(const SgsHostPlan& plan, const SgsCsrPart& part,
                        int long_threshold = kSgsLongThreshold);

} // namespace spmv
