// Host half of the aggregation multigrid preconditioner
// (spmv::AmgPreconditioner, cg.h): the expanded rows of a level, its
// aggregates, and the pattern and source lists of the Galerkin operator
// P^T A P, P the piecewise-constant prolongation.  Plain C++17, no device, no
// other header of the mirror: tools/amg_build_check.cpp compiles this file
// pair alone under the sanitizers.  Everything is deterministic.
//
// Input form: the rows of a level as CSR with local column numbers.  An entry
// (i, c) belongs to the level when c < ncols_local (ghost columns are dropped).
// Symmetric input: only c < i is an entry (the stored strictly lower block;
// anything else is dropped, as create_matrix does), the diagonal lives in an
// array of its own and the level stands for L + D + L^T.  nrows != ncols_local
// throws.
#pragma once

#include <cstdint>
#include <vector>

namespace spmv
{

// The expanded rows.  General: a row's entries in storage order.  Symmetric:
// the row's stored lower entries in storage order, the diagonal entry, then
// the mirror images of the stored entries of its column, ascending by their row
// (a stable transpose).  src >= 0: the entry is values[src]; src < 0: it is
// diagonal[~src].
struct AmgExpanded {
  int32_t n = 0;
  int64_t num_values = 0; // length of the value array the sources index
  bool symmetric = false;
  std::vector<int64_t> ptr = {0}; // n + 1
  std::vector<int32_t> col;
  std::vector<int32_t> src;
};

AmgExpanded amg_expand(const int32_t* rowptr, const int32_t* colind,
                       int64_t nrows, int64_t ncols_local, bool symmetric);

// One coarsening step.
//   m_i        the largest |a_e| over the entries of row i with column != i
//   strong(i)  in row order, the columns j != i of the entries with a_e != 0 and
//              |a_e| >= theta * m_i; a column is kept once, at its first
//              occurrence
//   pass 1     i ascending: if i and every j of strong(i) are unaggregated they
//              form the next aggregate (no strong neighbour: a singleton)
//   pass 2     i ascending, on a snapshot of the aggregates after pass 1: an
//              unaggregated i joins the aggregate of the first j of strong(i)
//              that has one in the snapshot
//   pass 3     i ascending: a row still unaggregated forms the next aggregate
//              with its still unaggregated strong neighbours
// Aggregates are numbered in order of creation, members ascending by row.
// The coarse entry (I, J) exists iff some expanded entry (i, j) has agg(i) = I,
// agg(j) = J; rows ascending by column.  Its sources, in the order the device
// adds them: the member rows of I ascending, inside a row the expanded order.
struct AmgStep {
  int32_t n = 0;     // rows of the fine level
  int32_t n_agg = 0; // rows of the coarse level
  std::vector<int32_t> agg;              // n
  std::vector<int32_t> member_ptr = {0}; // n_agg + 1
  std::vector<int32_t> member;           // n
  std::vector<int32_t> rowptr = {0};     // n_agg + 1: the coarse pattern
  std::vector<int32_t> colind;
  std::vector<int64_t> src_ptr = {0}; // coarse entries + 1
  std::vector<int32_t> src;           // AmgExpanded's encoding
};

// only the aggregates (agg, member_ptr, member, n, n_agg)
AmgStep amg_aggregate(const AmgExpanded& x, const double* values,
                      const double* diagonal, double theta);
// ... and the coarse pattern with its source lists
void amg_galerkin_pattern(const AmgExpanded& x, AmgStep* step);

inline AmgStep amg_coarsen(const AmgExpanded& x, const double* values,
                           const double* diagonal, double theta)
{
  AmgStep s = amg_aggregate(x, values, diagonal, theta);
  amg_galerkin_pattern(x, &s);
  return s;
}

} // namespace spmv
