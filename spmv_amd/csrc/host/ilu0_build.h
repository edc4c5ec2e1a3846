// Host half of the multicolour ILU(0) preconditioner (spmv::Ilu0Preconditioner,
// cg.h): the symbolic setup.  The colouring and the colour-major positions are
// sgs_color's and sgs_build's; the parts are ordered by POSITION of the column
// (the elimination needs that order), every entry knows where its value comes
// from in the matrix's value array and where it goes in the sliced layout of
// sgs_slice.  No values are read: the numbers are the device's business.
// Plain C++17, no device, no other header of the mirror but sgs_build.h:
// tools/ilu0_build_check.cpp compiles the two file pairs alone under the
// sanitizers.
//
// Input form: that of sgs_build.h.  A column that occurs twice among the
// off-diagonal entries of one row of the block (symmetric storage: among the
// stored lower entries of the row and the entries of its column) throws
// std::runtime_error ("duplicate"): a factor entry has ONE source.
#pragma once

#include <cstdint>
#include <vector>

#include "sgs_build.h"

namespace spmv
{

// One of the two parts of every row, CSR over positions: position `pos` (row
// perm[pos]) owns the entries ptr[pos] .. ptr[pos + 1], ascending by cpos.
struct Ilu0Part {
  std::vector<int64_t> ptr = {0};
  std::vector<int32_t> cpos; // the column's position
  std::vector<int32_t> src;  // index of the value in the matrix's value array
                             // (symmetric storage: of the stored lower entry,
                             // for the entry and for its mirror image)
  std::vector<int64_t> slot; // >= 0: index into SgsSlicedPart::val;
                             // < 0: index ~slot into SgsSlicedPart::long_val
};

struct Ilu0Symbolic {
  int32_t n = 0;
  int32_t num_colors = 0;
  std::vector<int32_t> colors;      // n: colour of row i
  std::vector<int32_t> perm;        // n: perm[pos] = row, colour-major
  std::vector<int32_t> pos;         // n: pos[row], the inverse of perm
  std::vector<int32_t> color_start; // num_colors + 1 positions
  Ilu0Part before, after;           // column's colour < / > the row's colour
  // the layout spmv_mcgs.hip sweeps over: columns (rows' numbers) in the parts'
  // order, every value 0.0
  SgsSlicedPart sliced_before, sliced_after;
};

Ilu0Symbolic ilu0_symbolic(const int32_t* rowptr, const int32_t* colind,
                           int64_t nrows, int64_t ncols_local, bool symmetric,
                           int long_threshold = kSgsLongThreshold);

} // namespace spmv
