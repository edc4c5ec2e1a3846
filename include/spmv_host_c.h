/*
 * include/spmv_host_c.h -- C facade over the C++17 host mirror
 * (spmv_amd/csrc/host: spmv::HipExecutor, L2GMap, Matrix<double>, cg).
 *
 * The C++ classes are what a LIBSPMV user programs against; this facade only
 * exists so that non-C++ harnesses (this repo's pytest suite and bench.py,
 * via ctypes) can drive exactly those classes.  One function per C++ call,
 * named after it; the parity tests therefore read like the reference's
 * tests/test_spmv.cpp: create executor -> create_matrix -> alloc x,y ->
 * col_map()->update(x) -> mult(x, y).
 *
 * Every function returns 0 on success and -1 after catching a C++ exception;
 * spmvh_last_error() then returns its what().  Device pointers are plain
 * void* / double*.
 */
#ifndef SPMV_HOST_C_H
#define SPMV_HOST_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spmvh_exec spmvh_exec;     /* shared_ptr<spmv::HipExecutor>     */
typedef struct spmvh_comm spmvh_comm;     /* shared_ptr<const spmv::Comm>      */
typedef struct spmvh_matrix spmvh_matrix; /* spmv::Matrix<double>*             */

const char* spmvh_last_error(void);

/* spmv::CommunicationModel, same values as spmv/mpi_utils.h:43-52 */
enum {
  SPMVH_P2P_BLOCKING = 0,
  SPMVH_P2P_NONBLOCKING = 1,
  SPMVH_COLLECTIVE_BLOCKING = 2,
  SPMVH_COLLECTIVE_NONBLOCKING = 3,
  SPMVH_ONESIDED_PUT_ACTIVE = 4,
  SPMVH_ONESIDED_PUT_PASSIVE = 5,
  SPMVH_SHMEM = 6,
  SPMVH_SHMEM_NODUP = 7
};

/* ---- executor: HipExecutor::create(device_id, HostExecutor::create()) ---- */
int spmvh_exec_create(int device_id, spmvh_exec** exec);
int spmvh_exec_destroy(spmvh_exec* exec);
int spmvh_exec_alloc(spmvh_exec* exec, size_t num_bytes, void** ptr);
int spmvh_exec_free(spmvh_exec* exec, void* ptr);
int spmvh_exec_memset(spmvh_exec* exec, void* ptr, int value, size_t num_bytes);
int spmvh_exec_copy(spmvh_exec* exec, void* dst, const void* src,
                    size_t num_bytes); /* device -> device */
int spmvh_exec_copy_from_host(spmvh_exec* exec, void* dst, const void* host_src,
                              size_t num_bytes);
int spmvh_exec_copy_to_host(spmvh_exec* exec, void* host_dst, const void* src,
                            size_t num_bytes);
int spmvh_exec_synchronize(spmvh_exec* exec);
int spmvh_exec_num_cus(spmvh_exec* exec, int* num_cus);
int spmvh_exec_device_type(spmvh_exec* exec, int* type); /* 1 cpu, 2 gpu */
/* the spmv_hip_ctx* behind the executor (for harness-side timing events) */
int spmvh_exec_context(spmvh_exec* exec, void** ctx);
/* HostExecutor has no compute path: creating a CSRMatrix on it must throw.
 * Returns 0 if it did (message in spmvh_last_error), 1 if it did not. */
int spmvh_host_executor_rejects_compute(void);

/* ---- communicators ---------------------------------------------------------- */
int spmvh_comm_self(spmvh_comm** comm);
int spmvh_rccl_unique_id(void* id_bytes /* 128 bytes */);
int spmvh_comm_rccl(spmvh_exec* exec, int nranks, int rank, const void* id_bytes,
                    spmvh_comm** comm);
/* transport supplied by the caller; allgather is mandatory (host memory,
 * recv = nranks * bytes_per_rank), must return 0 */
typedef int (*spmvh_allgather_fn)(void* user, const void* send, void* recv,
                                  size_t bytes_per_rank);
/* optional device transport (may be NULL: device calls then fail).  Semantics
 * of spmv::Comm::neighbor_exchange / allreduce_sum: DEVICE pointers, offsets
 * in elements, everything ordered on `stream`. */
typedef int (*spmvh_exchange_fn)(void* user, size_t elem_bytes,
                                 int num_neighbours, const int* neighbours,
                                 const void* send_buf,
                                 const int32_t* send_counts,
                                 const int32_t* send_offsets, void* recv_base,
                                 const int32_t* recv_counts,
                                 const int32_t* recv_offsets, void* stream);
typedef int (*spmvh_allreduce_fn)(void* user, double* device_inout,
                                  size_t count, void* stream);
int spmvh_comm_callback(int rank, int nranks, spmvh_allgather_fn allgather,
                        spmvh_exchange_fn exchange, spmvh_allreduce_fn allreduce,
                        void* user, spmvh_comm** comm);
/* RcclComm::info(): out = {nranks, rank (both as RCCL reports them), RCCL
 * version code, 1 if the reductions have a communicator of their own} */
int spmvh_comm_rccl_info(spmvh_comm* comm, int out[4], char* lib_path,
                         int lib_path_len);
int spmvh_comm_destroy(spmvh_comm* comm);
/* the deterministic peer reduction of the CG scalars (Comm::enable_peer_reduce:
 * collective; *ok = 0: some rank cannot reach some window, the transport's
 * all-reduce stays) and one reduction through it (Comm::reduce_sum) */
int spmvh_comm_enable_peer_reduce(spmvh_comm* comm, spmvh_exec* exec, int* ok);
/* Comm::ranks_share_a_process (collective on its first call): do two ranks of
 * the communicator live in ONE process (ranks as threads)?  Decided by a
 * per-process token (pid + a 64-bit nonce), not the pid alone */
int spmvh_comm_ranks_share_a_process(spmvh_comm* comm, int* shared);
int spmvh_comm_reduce_sum(spmvh_comm* comm, double* device_inout, int count,
                          void* stream);

/* ---- matrix: Matrix<double>::create_matrix / create_poisson3d --------------- */
/* rowptr has nrows_local + num_row_ghosts + 1 entries: the extra rows hold
 * contributions to the global rows `row_ghosts` owned by other ranks and are
 * shipped to them (Matrix.cpp:188-292). */
int spmvh_matrix_create(spmvh_comm* comm, spmvh_exec* exec,
                        const int32_t* rowptr, const int32_t* colind,
                        const double* values, int64_t nrows_local,
                        int64_t ncols_local, const int64_t* row_ghosts,
                        int64_t num_row_ghosts, const int64_t* col_ghosts,
                        int64_t num_col_ghosts, int symmetric, int cm,
                        spmvh_matrix** A);
int spmvh_matrix_create_poisson3d(spmvh_comm* comm, spmvh_exec* exec, int32_t n,
                                  int symmetric, int cm, spmvh_matrix** A);
/* seeded unstructured test matrix generated on the device (one rank, general
 * storage; spmv_hip_unstructured_fill_f64) */
int spmvh_matrix_create_unstructured(spmvh_comm* comm, spmvh_exec* exec,
                                     int64_t nrows, int per_row, int64_t band,
                                     int far_permille, uint64_t seed,
                                     spmvh_matrix** A);
/* seeded FEM-like test matrix generated on the device (one rank, general
 * storage; spmv_hip_fem_count / spmv_hip_fem_fill_f64) */
struct spmv_hip_fem_params; /* include/spmv_hip.h */
int spmvh_matrix_create_fem_like(spmvh_comm* comm, spmvh_exec* exec,
                                 const struct spmv_hip_fem_params* params,
                                 spmvh_matrix** A);
/* ... its strictly lower part + diagonal in symmetric storage
 * (spmv_hip_csr_lower_split_*) */
int spmvh_matrix_create_fem_like_sym(spmvh_comm* comm, spmvh_exec* exec,
                                     const struct spmv_hip_fem_params* params,
                                     spmvh_matrix** A);
/* The Poisson matrix on a 3-D block partition (the reference
 * partitions by row slabs only, read_petsc.cpp:20-37): px * py * pz boxes,
 * rank = ix + px (iy + py iz), rank-major global numbering (a box's points are
 * consecutive, x fastest), so each rank still owns one contiguous row range.
 * px * py * pz must equal the communicator's size. */
int spmvh_matrix_create_poisson3d_boxes(spmvh_comm* comm, spmvh_exec* exec,
                                        int32_t n, int px, int py, int pz,
                                        int symmetric, int cm, spmvh_matrix** A);
/* Its host half (no device, no communicator): rank `rank`'s rows in
 * spmvh_matrix_create's input form.  sizes = {rows, non-zeros, ghosts, global
 * row offset, box extents x y z}; the arrays are filled when non-NULL (call
 * once with NULLs for the sizes). */
int spmvh_poisson3d_box_rows(int32_t n, int px, int py, int pz, int rank,
                             int64_t sizes[7], int32_t* rowptr, int32_t* colind,
                             double* values, int64_t* col_ghosts);
int spmvh_matrix_destroy(spmvh_matrix* A);
int spmvh_matrix_rows(spmvh_matrix* A, int* rows);
int spmvh_matrix_cols(spmvh_matrix* A, int* cols);
int spmvh_matrix_non_zeros(spmvh_matrix* A, int64_t* nnz);
int spmvh_matrix_format_size(spmvh_matrix* A, size_t* bytes);
int spmvh_matrix_symmetric(spmvh_matrix* A, int* symmetric);
/* local / remote block sizes: out[0..5] = rows, cols, nnz of local then remote
 * (remote all zero when the matrix has a single block) */
int spmvh_matrix_blocks(spmvh_matrix* A, int64_t out[6]);
/* DEVICE pointers of the local block's value array (non-zeros of the local
 * block doubles, in its CSR order; symmetric storage: the strictly lower
 * entries) and of its diagonal array (symmetric storage; NULL otherwise), for a
 * caller who rewrites the coefficients in place on a fixed pattern.  Such a
 * caller then calls spmvh_matrix_plan_values_changed (Matrix::
 * plan_values_changed: every copy the SpMV plans keep is refreshed; without it
 * mult may return the OLD matrix's product) and, for an Ilu0Preconditioner,
 * spmvh_ilu0_refactor.  Both: error after release_csr ("released"). */
int spmvh_matrix_local_values(spmvh_matrix* A, double** values,
                              double** diagonal);
int spmvh_matrix_plan_values_changed(spmvh_matrix* A);
/* spmv_hip_csr_plan_get / _set on the local (remote = 0) or remote block's
 * plan: which form it took, what it cost, launch-shape knobs */
int spmvh_matrix_plan_get(spmvh_matrix* A, int remote, const char* key,
                          int* value);
/* Matrix::enable_mixed / use_mixed: fp32 copies of the blocks'
 * values (ok = 0: symmetric storage, nothing done); mult / mult_dot then stream
 * those while `on`. */
int spmvh_matrix_enable_mixed(spmvh_matrix* A, int* ok);
int spmvh_matrix_use_mixed(spmvh_matrix* A, int on);
/* CSRMatrix::release_csr on both blocks: the device copies of colind / values
 * of a block whose plan holds the matrix in its own format are freed
 * (spmv_hip_csr_plan_owns_matrix); *bytes_freed = what came back (0: nothing) */
int spmvh_matrix_release_csr(spmvh_matrix* A, int64_t* bytes_freed);
int spmvh_matrix_plan_set(spmvh_matrix* A, int remote, const char* key,
                          int value);
/* A.col_map()->update(x) ; A.mult(x, y) ; A.col_map()->update_finalise(x) */
int spmvh_matrix_update(spmvh_matrix* A, double* x);
int spmvh_matrix_update_finalise(spmvh_matrix* A, double* x);
int spmvh_matrix_mult(spmvh_matrix* A, double* x, double* y);
/* Matrix::transpmult: y = A^T b, b in row space (rows() entries), y in column
 * space (local_size + num_ghosts entries: this rank's part, then the ghost
 * columns' contributions that spmvh_l2g_map_reverse_update / the matrix's
 * col_map()->reverse_update adds to their owners).  enable_transpose builds
 * the transposed maps now (before release_csr). */
int spmvh_matrix_transpmult(spmvh_matrix* A, double* b, double* y);
int spmvh_matrix_enable_transpose(spmvh_matrix* A);
/* Matrix::mult_block: Y = A X for a block of k >= 1 INTERLEAVED vectors --
 * element (i, c) at X[i * k + c]; X holds (local_size + num_ghosts) * k
 * entries, Y rows() * k.  Column c of Y has the bits of spmvh_matrix_mult on
 * column c of X.  update_block / update_finalise_block are
 * col_map()->update_block(X, k) / update_finalise_block(X, k): the halo of
 * all k vectors in one exchange. */
int spmvh_matrix_mult_block(spmvh_matrix* A, double* X, double* Y, int k);
int spmvh_matrix_update_block(spmvh_matrix* A, double* X, int k);
int spmvh_matrix_update_finalise_block(spmvh_matrix* A, double* X, int k);

/* ---- fp32 instantiation: Matrix<float> (device_executor.h:88-99 carries float
 * visitors).  Same calls, float data. */
typedef struct spmvh_matrix_f32 spmvh_matrix_f32;
int spmvh_matrix_f32_create(spmvh_comm* comm, spmvh_exec* exec,
                            const int32_t* rowptr, const int32_t* colind,
                            const float* values, int64_t nrows_local,
                            int64_t ncols_local, const int64_t* row_ghosts,
                            int64_t num_row_ghosts, const int64_t* col_ghosts,
                            int64_t num_col_ghosts, int symmetric, int cm,
                            spmvh_matrix_f32** A);
int spmvh_matrix_f32_destroy(spmvh_matrix_f32* A);
int spmvh_matrix_f32_info(spmvh_matrix_f32* A, int* rows, int64_t* nnz,
                          int32_t* local_size, int32_t* num_ghosts);
int spmvh_matrix_f32_update(spmvh_matrix_f32* A, float* x);
int spmvh_matrix_f32_mult(spmvh_matrix_f32* A, float* x, float* y);
int spmvh_matrix_f32_transpmult(spmvh_matrix_f32* A, float* b, float* y);
int spmvh_matrix_f32_mult_block(spmvh_matrix_f32* A, float* X, float* Y, int k);
int spmvh_matrix_f32_update_block(spmvh_matrix_f32* A, float* X, int k);
int spmvh_matrix_f32_update_finalise_block(spmvh_matrix_f32* A, float* X, int k);

/* Host half of create_matrix only (Matrix<double>::split_rows): no device.
 * sizes[0..7] = local rows, cols, nnz, remote rows, cols, nnz, number of
 * (renumbered) ghost columns, nnz_full. */
typedef struct spmvh_split spmvh_split;
int spmvh_split_create(const int32_t* rowptr, const int32_t* colind,
                       const double* values, int64_t nrows_local,
                       int64_t ncols_local, int64_t global_row_offset,
                       int64_t global_col_offset, const int64_t* col_ghosts,
                       int64_t num_col_ghosts, int symmetric, int cm,
                       spmvh_split** split, int64_t sizes[8]);
/* which: 0 local, 1 remote.  Arrays sized from `sizes`; diagonal/ghosts may
 * be NULL. */
/* collective variant with ghost-row elimination (split_rows_distributed) */
int spmvh_split_create_dist(spmvh_comm* comm, const int32_t* rowptr,
                            const int32_t* colind, const double* values,
                            int64_t nrows_local, int64_t ncols_local,
                            const int64_t* row_ghosts, int64_t num_row_ghosts,
                            const int64_t* col_ghosts, int64_t num_col_ghosts,
                            int symmetric, int cm, spmvh_split** split,
                            int64_t sizes[8]);
int spmvh_split_get(spmvh_split* split, int which, int32_t* rowptr,
                    int32_t* colind, double* values);
int spmvh_split_extra(spmvh_split* split, double* diagonal, int64_t* ghosts);
int spmvh_split_destroy(spmvh_split* split);

/* ---- column map (L2GMap) inspection ------------------------------------------ */
int spmvh_l2g_sizes(spmvh_matrix* A, int32_t* local_size, int32_t* num_ghosts,
                    int64_t* global_size, int64_t* global_offset,
                    int* overlapping, int* num_neighbours, int* num_indices,
                    int* packs);
/* 1 = the halo of A.col_map() moves by peer stores into the neighbours'
 * windows (onesided_put_* models on several ranks; include/spmv_hip.h) */
int spmvh_l2g_onesided(spmvh_matrix* A, int* onesided);
int spmvh_l2g_ghosts(spmvh_matrix* A, int64_t* ghosts);
/* plan arrays: neighbours[nn], send_count[nn], recv_count[nn],
 * send_offset[nn+1], recv_offset[nn+1], indexbuf[num_indices] */
int spmvh_l2g_plan(spmvh_matrix* A, int32_t* neighbours, int32_t* send_count,
                   int32_t* recv_count, int32_t* send_offset,
                   int32_t* recv_offset, int32_t* indexbuf);
int spmvh_l2g_global_to_local(spmvh_matrix* A, int64_t global, int32_t* local);

/* Stand-alone L2GMap (no matrix), for plan tests:
 * L2GMap(comm, local_size, ghosts, exec-or-host, cm).  use_host_exec != 0
 * builds it on a HostExecutor (plan only; update() would throw). */
typedef struct spmvh_l2g spmvh_l2g;
int spmvh_l2g_create(spmvh_comm* comm, spmvh_exec* exec, int use_host_exec,
                     int64_t local_size, const int64_t* ghosts,
                     int64_t num_ghosts, int cm, spmvh_l2g** map);
int spmvh_l2g_destroy(spmvh_l2g* map);
int spmvh_l2g_map_sizes(spmvh_l2g* map, int* num_neighbours, int* num_indices,
                        int* packs);
int spmvh_l2g_map_plan(spmvh_l2g* map, int32_t* neighbours, int32_t* send_count,
                       int32_t* recv_count, int32_t* send_offset,
                       int32_t* recv_offset, int32_t* indexbuf);
int spmvh_l2g_map_update(spmvh_l2g* map, double* x);
/* L2GMap::update_block / update_finalise_block on a block of k interleaved
 * fp64 vectors ((local_size + num_ghosts) * k entries) */
int spmvh_l2gmap_update_block(spmvh_l2g* map, double* X, int k);
int spmvh_l2gmap_update_finalise_block(spmvh_l2g* map, double* X, int k);
/* L2GMap::reverse_update(vec) (L2GMap.h:103): ghost tail -> owners, added */
int spmvh_l2g_map_reverse_update(spmvh_l2g* map, double* x);
int spmvh_l2g_map_reverse_update_f32(spmvh_l2g* map, float* x);

/* ---- cg: spmv::cg(comm, exec, A, b, x, kmax, rtol) ---------------------------- */
/* rnorm_history (host, kmax+1 doubles) may be NULL; *num_its = returned k */
int spmvh_cg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
             const double* b, double* x, int kmax, double rtol, int* num_its,
             double* rnorm_history);

/* ---- PETSc binary ingest (spmv/read_petsc.{h,cpp}) ------------------------------
 * read_petsc_binary_matrix / read_petsc_binary_vector of the mirror.  The
 * vector comes back as a device pointer the caller frees with
 * spmvh_exec_free. */
int spmvh_read_petsc_matrix(spmvh_comm* comm, spmvh_exec* exec,
                            const char* filename, int symmetric, int cm,
                            spmvh_matrix** A);
int spmvh_read_petsc_vector(spmvh_comm* comm, spmvh_exec* exec,
                            const char* filename, double** device_vec,
                            int64_t* nrows_local);
/* host-only parse of rank `rank` of `size` (no device): sizes[0..6] = global
 * rows, cols, nnz, row_begin, row_end, local nnz, number of ghost columns */
typedef struct spmvh_petsc_rows spmvh_petsc_rows;
int spmvh_petsc_rows_read(const char* filename, int rank, int size,
                          spmvh_petsc_rows** rows, int64_t sizes[7]);
int spmvh_petsc_rows_get(spmvh_petsc_rows* rows, int32_t* rowptr,
                         int32_t* colind, double* values, int64_t* col_ghosts);
int spmvh_petsc_rows_destroy(spmvh_petsc_rows* rows);

/* Same solve with the optional arguments of the C++ overload: a reusable
 * spmv::CgWorkspace (may be NULL) and per-iteration HIP-event timing of the
 * local-block SpMV kernel (time_spmv bit 0 -> *spmv_ms_total, *spmv_launches;
 * bit 2 switches CgOptions::consumer_reductions off, bit 3 CgOptions::defer_x;
 * bits 8-15 set CgOptions::poll_every). */
typedef struct spmvh_cg_workspace spmvh_cg_workspace;
/* cg with CgOptions::mixed (fp32 copy of the matrix values in the SpMV,
 * residual replacement every `replace_every` iterations, fp64 correction
 * solve if the true residual misses rtol).  out_stats = {spmv_ms_total,
 * spmv_launches, replacements, true ||b-Ax||/||r0|| after the mixed loop,
 * fp64 iterations of the correction solve, true relative residual at the
 * end}.  rnorm_history holds up to history_capacity entries. */
int spmvh_cg_mixed(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                   const double* b, double* x, int kmax, double rtol,
                   int replace_every, int* num_its, double* rnorm_history,
                   int history_capacity, spmvh_cg_workspace* ws, int time_spmv,
                   double out_stats[6]);
int spmvh_cg_workspace_create(spmvh_exec* exec, spmvh_cg_workspace** ws);
int spmvh_cg_workspace_destroy(spmvh_cg_workspace* ws);
/* create the timing events of a time_spmv solve of up to `iterations` steps
 * ahead of it (keeps them out of a benchmark's timed region) */
int spmvh_cg_workspace_reserve_timing(spmvh_cg_workspace* ws, int iterations);
int spmvh_cg_ex(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                const double* b, double* x, int kmax, double rtol, int* num_its,
                double* rnorm_history, spmvh_cg_workspace* ws, int time_spmv,
                double* spmv_ms_total, int* spmv_launches);

/* spmv::cg_block: A X = B for nrhs right-hand sides, nrhs independent CG
 * recurrences in lockstep on INTERLEAVED blocks (element (i, c) at
 * B[i * nrhs + c], X[i * nrhs + c]; device pointers of rows * nrhs doubles,
 * 1 <= nrhs <= 8, X must not overlap B).  iterations: nrhs entries;
 * rnorm_history (may be NULL): nrhs * (kmax + 1) entries, ||r_j|| of column c
 * at [c * (kmax + 1) + j] for j <= iterations[c], -1.0 beyond.  *max_its = the
 * largest entry of iterations.  ws: a reusable spmv::CgBlockWorkspace (may be
 * NULL).  flags: bit 0 -> CgOptions::time_spmv (*spmv_ms_total, *spmv_launches,
 * both may be NULL), bits 8-15 CgOptions::poll_every (0 = default). */
typedef struct spmvh_cg_block_workspace spmvh_cg_block_workspace;
int spmvh_cg_block_workspace_create(spmvh_exec* exec,
                                    spmvh_cg_block_workspace** ws);
int spmvh_cg_block_workspace_destroy(spmvh_cg_block_workspace* ws);
int spmvh_cg_block(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                   const double* B, double* X, int nrhs, int kmax, double rtol,
                   int* max_its, int* iterations, double* rnorm_history,
                   spmvh_cg_block_workspace* ws, int flags,
                   double* spmv_ms_total, int* spmv_launches);

/* Jacobi-preconditioned CG.
 * spmvh_matrix_diagonal: Matrix::diagonal -- d (device, rows entries) = the
 * diagonal of this rank's rows; general storage after release_csr is an error
 * (take the diagonal first), symmetric storage keeps its diagonal.
 * spmvh_jacobi_inverse: spmv::jacobi_inverse -- dinv = 1 / d on the device (n
 * doubles each; they may coincide); an entry that is not finite or not > 0 is
 * an error whose text says "diagonal is not positive".  One host wait.
 * spmvh_pcg: spmv::pcg -- CG from x0 = 0 with the diagonal preconditioner
 * whose inverse is dinv (device, rows doubles, positive; where it came from
 * does not matter).  x must not overlap b or dinv.  rnorm_history (may be
 * NULL): kmax + 1 entries, ||r_0|| .. ||r_k|| of the unpreconditioned residual.
 * ws: a reusable spmv::PcgWorkspace (may be NULL).  flags: bit 0 ->
 * CgOptions::time_spmv (*spmv_ms_total, *spmv_launches, both may be NULL),
 * bit 2 switches CgOptions::consumer_reductions off, bits 8-15
 * CgOptions::poll_every (0 = default). */
typedef struct spmvh_pcg_workspace spmvh_pcg_workspace;
int spmvh_matrix_diagonal(spmvh_matrix* A, double* d);
int spmvh_jacobi_inverse(spmvh_exec* exec, const double* d, double* dinv,
                         int64_t n);
int spmvh_pcg_workspace_create(spmvh_exec* exec, spmvh_pcg_workspace** ws);
int spmvh_pcg_workspace_destroy(spmvh_pcg_workspace* ws);
int spmvh_pcg_workspace_reserve_timing(spmvh_pcg_workspace* ws, int iterations);
int spmvh_pcg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
              const double* b, double* x, const double* dinv, int kmax,
              double rtol, int* num_its, double* rnorm_history,
              spmvh_pcg_workspace* ws, int flags, double* spmv_ms_total,
              int* spmv_launches);

/* ---- Chebyshev polynomial preconditioner (host/cg.h; not in the reference) ---
 * spmvh_chebyshev_coefficients: spmv::chebyshev_coefficients -- a[], b[] (host,
 * `degree` doubles each) of the Chebyshev iteration on [lmin, lmax]; an error
 * whose text says "degree" (outside 1..16) or "bounds" (not finite, or not
 * 0 < lmin < lmax).  Touches no device.
 * spmvh_chebyshev_apply: spmv::chebyshev_apply -- z = q(dinv*A) dinv r (device,
 * rows doubles each, any alignment, not overlapping); dinv may be NULL; ws may
 * be NULL (then the call waits for its own work vectors).
 * spmvh_pcg_chebyshev: spmv::pcg_chebyshev -- CG from x0 = 0 with that
 * preconditioner; arguments as spmvh_pcg plus degree, lmin, lmax; dinv may be
 * NULL.  flags: bit 0 CgOptions::time_spmv (`degree` intervals per iteration),
 * bits 8-15 CgOptions::poll_every (0 = default); consumer_reductions does not
 * apply.  spmvh_chebyshev_workspace_reserve_timing counts SpMVs (iterations *
 * degree).
 * spmvh_lambda_max_estimate: spmv::lambda_max_estimate -- `steps` power
 * iterations on dinv*A from v0 (device, rows doubles, unchanged); dinv may be
 * NULL; an error whose text says "steps" (< 1) or "v0" (v0.v0 == 0). */
typedef struct spmvh_chebyshev_workspace spmvh_chebyshev_workspace;
int spmvh_chebyshev_coefficients(int degree, double lmin, double lmax, double* a,
                                 double* b);
int spmvh_chebyshev_workspace_create(spmvh_exec* exec,
                                     spmvh_chebyshev_workspace** ws);
int spmvh_chebyshev_workspace_destroy(spmvh_chebyshev_workspace* ws);
int spmvh_chebyshev_workspace_reserve_timing(spmvh_chebyshev_workspace* ws,
                                             int spmvs);
int spmvh_chebyshev_apply(spmvh_exec* exec, spmvh_matrix* A, const double* r,
                          double* z, const double* dinv, int degree, double lmin,
                          double lmax, spmvh_chebyshev_workspace* ws);
int spmvh_pcg_chebyshev(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                        const double* b, double* x, const double* dinv,
                        int degree, double lmin, double lmax, int kmax,
                        double rtol, int* num_its, double* rnorm_history,
                        spmvh_chebyshev_workspace* ws, int flags,
                        double* spmv_ms_total, int* spmv_launches);
int spmvh_lambda_max_estimate(spmvh_comm* comm, spmvh_exec* exec,
                              spmvh_matrix* A, const double* dinv,
                              const double* v0, int steps, double* lambda);

/* ---- Multicolour symmetric Gauss-Seidel (host/cg.h; not in the reference) -----
 * Two entries that touch NO device (host/sgs_build.h).  Input: the rows of a
 * rank as CSR with local column numbers; entries with column >= ncols_local
 * are ghosts and ignored, column == row is the diagonal; symmetric != 0: only
 * column < row counts as an off-diagonal entry and the block stands for
 * B + B^T.  nrows != ncols_local is an error.
 * spmvh_sgs_color: the greedy colouring over B + B^T -> colors_out (nrows
 * entries), *ncolors_out.
 * spmvh_sgs_build_create: the colouring and the colour-major copy; sizes[3] =
 * {colours, entries of `before`, entries of `after`}.  spmvh_sgs_build_get
 * copies out (every pointer may be NULL): colors (nrows), perm (nrows),
 * color_start (colours + 1), d (nrows, the diagonal), and the two parts as CSR
 * over POSITIONS: ptr (nrows + 1, int64), col, val.
 *
 * spmvh_sgs_create: spmv::SgsPreconditioner(exec, A) -- the setup; errors whose
 * text says "diagonal is not positive", "released" or "same index range".
 * spmvh_sgs_create_ex: SgsPreconditioner(exec, A, SgsOptions) -- setup 0 host,
 * 1 device (colouring and plan built on the device: nothing of the matrix is
 * read back); order -1 not given, 0 hashed, 1 natural (as many rounds as the
 * longest ascending path: slow on long dependency chains); colors NULL or rows
 * entries (host) that replace the colouring.  setup 0 with an order or colors
 * is an error; further errors say "not proper", "colour".
 * spmvh_sgs_create_ex2: the same with SgsOptions::values -- values 0 fp64 (in
 * every respect spmvh_sgs_create_ex), 1 fp32: the sweep plan keeps its
 * off-diagonal values as float, rounded to nearest-even, with every setup,
 * order and colors; anything else is an error ("values"), checked with the
 * other rules of the options before a handle is looked at.  A value out of
 * fp32's range is an error that says "fp32 range".
 * spmvh_sgs_value_bits: 64 or 32.
 * spmvh_fp32_range_count: the rule of that range as a plain host function --
 * how many of the n doubles (host) are finite, non-zero and round to +-Inf,
 * zero or an fp32 subnormal; the kernels that round count by the same rule.
 * spmvh_sgs_setup_info: rounds of the device colouring (0 otherwise) and the
 * wall time of the constructor; _setup_detail: the device setup's colouring
 * and build times and the peak bytes of its temporaries (each may be NULL).
 * spmvh_sgs_export_sizes: sizes[10] = {rows, colours, slices, before: sliced
 * entries, long rows, long entries, after: the same three, device bytes};
 * spmvh_sgs_export: the plan's arrays to host buffers of those sizes; before /
 * after: 11 pointers each in the order of spmv_hip_mcgs_export (color_slice,
 * slice_pos0, slice_ptr, len, col, val, color_long, long_pos, long_ptr,
 * long_col, long_val); every pointer may be NULL.
 * spmvh_sgs_info: rows, colours, device bytes of the plan (each may be NULL).
 * spmvh_sgs_colors: the colours, rows entries (host).
 * spmvh_sgs_apply: spmv::sgs_apply -- z = M^-1 r (device, rows doubles each, any
 * alignment, not overlapping: "overlaps"), on the executor's current stream.
 * spmvh_pcg_sgs: spmv::pcg_sgs; arguments as spmvh_pcg with M in place of
 * dinv.  flags: bit 0 CgOptions::time_spmv (one interval per iteration), bits
 * 8-15 CgOptions::poll_every (0 = default). */
typedef struct spmvh_sgs_build spmvh_sgs_build;
typedef struct spmvh_sgs spmvh_sgs;
typedef struct spmvh_sgs_workspace spmvh_sgs_workspace;
int spmvh_sgs_color(const int32_t* rowptr, const int32_t* colind, int64_t nrows,
                    int64_t ncols_local, int symmetric, int32_t* colors_out,
                    int* ncolors_out);
int spmvh_sgs_build_create(const int32_t* rowptr, const int32_t* colind,
                           const double* values, int64_t nrows,
                           int64_t ncols_local, int symmetric,
                           spmvh_sgs_build** build, int64_t* sizes);
int spmvh_sgs_build_get(spmvh_sgs_build* build, int32_t* colors, int32_t* perm,
                        int32_t* color_start, double* d, int64_t* before_ptr,
                        int32_t* before_col, double* before_val,
                        int64_t* after_ptr, int32_t* after_col,
                        double* after_val);
int spmvh_sgs_build_destroy(spmvh_sgs_build* build);
int spmvh_sgs_create(spmvh_exec* exec, spmvh_matrix* A, spmvh_sgs** M);
int spmvh_sgs_create_ex(spmvh_exec* exec, spmvh_matrix* A, int setup, int order,
                        const int32_t* colors, spmvh_sgs** M);
int spmvh_sgs_create_ex2(spmvh_exec* exec, spmvh_matrix* A, int setup, int order,
                         const int32_t* colors, int values, spmvh_sgs** M);
int spmvh_sgs_value_bits(spmvh_sgs* M, int* bits);
int spmvh_fp32_range_count(const double* values, int64_t n, int64_t* count);
int spmvh_sgs_setup_info(spmvh_sgs* M, int* rounds, double* setup_ms);
int spmvh_sgs_setup_detail(spmvh_sgs* M, double* color_ms, double* build_ms,
                           int64_t* temp_bytes);
int spmvh_sgs_export_sizes(spmvh_sgs* M, int64_t* sizes);
int spmvh_sgs_export(spmvh_sgs* M, int32_t* perm, int32_t* color_start,
                     double* dinv, void* const* before, void* const* after);
int spmvh_sgs_destroy(spmvh_sgs* M);
int spmvh_sgs_info(spmvh_sgs* M, int* rows, int* num_colors,
                   int64_t* plan_bytes);
int spmvh_sgs_colors(spmvh_sgs* M, int32_t* colors);
int spmvh_sgs_apply(spmvh_exec* exec, spmvh_sgs* M, const double* r, double* z);
int spmvh_sgs_workspace_create(spmvh_exec* exec, spmvh_sgs_workspace** ws);
int spmvh_sgs_workspace_destroy(spmvh_sgs_workspace* ws);
int spmvh_sgs_workspace_reserve_timing(spmvh_sgs_workspace* ws, int iterations);
int spmvh_pcg_sgs(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                  spmvh_sgs* M, const double* b, double* x, int kmax,
                  double rtol, int* num_its, double* rnorm_history,
                  spmvh_sgs_workspace* ws, int flags, double* spmv_ms_total,
                  int* spmv_launches);

/* ---- Preconditioned CG for several right-hand sides (spmv::pcg_block) -----------
 * Blocks are INTERLEAVED as for spmvh_cg_block: element (i, c) at V[i * nrhs +
 * c], 1 <= nrhs <= 8.
 * spmvh_sgs_apply_block: spmv::sgs_apply_block -- Z = M^-1 R for nrhs vectors
 * (device, rows * nrhs doubles each, any alignment, not overlapping:
 * "overlaps"; "nrhs"), on the executor's current stream; M from spmvh_sgs_create
 * or spmvh_ilu0_create.  Column c has the bits of spmvh_sgs_apply on column c.
 * spmvh_pcg_block: spmv::pcg_block; arguments as spmvh_cg_block plus the
 * preconditioner: exactly one of dinv (device, rows doubles, shared by all
 * columns) and M is not NULL.  Errors name "nrhs", "kmax", "preconditioner",
 * "rows", "pivot" or "overlaps".  ws: a reusable spmv::PcgBlockWorkspace (may
 * be NULL).  flags as for spmvh_cg_block.
 * spmvh_pcg_block_check_arguments: those rules alone (no device; the pointers
 * are compared, never read). */
typedef struct spmvh_pcg_block_workspace spmvh_pcg_block_workspace;
int spmvh_sgs_apply_block(spmvh_exec* exec, spmvh_sgs* M, const double* R,
                          double* Z, int nrhs);
int spmvh_pcg_block_workspace_create(spmvh_exec* exec,
                                     spmvh_pcg_block_workspace** ws);
int spmvh_pcg_block_workspace_destroy(spmvh_pcg_block_workspace* ws);
int spmvh_pcg_block_check_arguments(int nrhs, int kmax, int has_dinv,
                                    int has_sgs, int64_t sgs_rows,
                                    int64_t sgs_negative_pivots, int64_t rows,
                                    const double* B, const double* X,
                                    const double* dinv);
int spmvh_pcg_block(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                    const double* B, double* X, int nrhs, const double* dinv,
                    spmvh_sgs* M, int kmax, double rtol, int* max_its,
                    int* iterations, double* rnorm_history,
                    spmvh_pcg_block_workspace* ws, int flags,
                    double* spmv_ms_total, int* spmv_launches);

/* ---- Multicolour ILU(0) (spmv::Ilu0Preconditioner, host/cg.h) ----------------
 * spmvh_ilu0_symbolic_*: host/ilu0_build.h, no device.  Input as
 * spmvh_sgs_color; sizes[7] = {colours, entries of `before`, of `after`, sliced
 * and long entries of `before`, sliced and long entries of `after`}.  _get: each
 * output may be NULL; colors / perm / pos nrows entries, color_start colours + 1;
 * per part ptr (nrows + 1, by position), cpos, src, slot, and the columns of the
 * sliced layout (sliced_col, long_col).  A column twice in a row: "duplicate".
 * spmvh_ilu0_create: spmv::Ilu0Preconditioner(exec, A); the handle is an
 * spmvh_sgs and serves wherever one does (spmvh_sgs_info / _colors / _apply /
 * _destroy, spmvh_pcg_sgs, spmvh_gmres).  The calls below need a handle made
 * here ("not an Ilu0Preconditioner" otherwise).
 * spmvh_ilu0_refactor: refactor(A) -- device only; errors "pivot", "released".
 * spmvh_ilu0_info: info[6] = {entries of before, of after, negative pivots,
 * plan bytes, the constructor's symbolic and numeric wall time in microseconds}.
 * spmvh_ilu0_pattern / _factor: the host copies of cg.h (outputs may be NULL).
 * spmvh_ilu0_create_ex2: spmvh_ilu0_create_ex with `values` as
 * spmvh_sgs_create_ex2 takes it; fp32 rounds l~ and u~ as they are scattered
 * into the sweep plan (the factorisation, spmvh_ilu0_factor and the pivot
 * counts stay fp64), the constructor and spmvh_ilu0_refactor say "fp32 range".
 * spmvh_ilu0_create_ex: Ilu0Preconditioner(exec, A, SgsOptions) -- the
 * arguments and their rules are spmvh_sgs_create_ex's; setup 1 colours the
 * block and builds the plan on the device (spmv_hip_ilu0_plan_build), nothing
 * of the matrix is read back; errors say "duplicate", "not proper", "colour",
 * "pivot".  spmvh_sgs_setup_info / _setup_detail / _export_sizes / _export
 * answer for the handle.
 * spmvh_ilu0_export_sizes: sizes[4] = {rows, entries of before, of after, device
 * bytes without the sweep plan's}; spmvh_ilu0_export: the part arrays of the
 * device plan, of either setup; before / after: 4 pointers each (ptr rows + 1
 * int64, cpos int32, src int32, slot int64), every pointer may be NULL. */
typedef struct spmvh_ilu0_symbolic spmvh_ilu0_symbolic;
int spmvh_ilu0_symbolic_create(const int32_t* rowptr, const int32_t* colind,
                               int64_t nrows, int64_t ncols_local, int symmetric,
                               spmvh_ilu0_symbolic** sym, int64_t* sizes);
int spmvh_ilu0_symbolic_get(spmvh_ilu0_symbolic* sym, int32_t* colors,
                            int32_t* perm, int32_t* pos, int32_t* color_start,
                            int64_t* before_ptr, int32_t* before_cpos,
                            int32_t* before_src, int64_t* before_slot,
                            int32_t* before_sliced_col, int32_t* before_long_col,
                            int64_t* after_ptr, int32_t* after_cpos,
                            int32_t* after_src, int64_t* after_slot,
                            int32_t* after_sliced_col, int32_t* after_long_col);
int spmvh_ilu0_symbolic_destroy(spmvh_ilu0_symbolic* sym);
int spmvh_ilu0_create(spmvh_exec* exec, spmvh_matrix* A, spmvh_sgs** M);
int spmvh_ilu0_refactor(spmvh_sgs* M, spmvh_matrix* A);
int spmvh_ilu0_info(spmvh_sgs* M, int64_t* info);
int spmvh_ilu0_pattern(spmvh_sgs* M, int64_t* before_ptr, int32_t* before_col,
                       int64_t* after_ptr, int32_t* after_col);
int spmvh_ilu0_factor(spmvh_sgs* M, double* l, double* u, double* d);
int spmvh_ilu0_create_ex(spmvh_exec* exec, spmvh_matrix* A, int setup, int order,
                         const int32_t* colors, spmvh_sgs** M);
int spmvh_ilu0_create_ex2(spmvh_exec* exec, spmvh_matrix* A, int setup,
                          int order, const int32_t* colors, int values,
                          spmvh_sgs** M);
int spmvh_ilu0_export_sizes(spmvh_sgs* M, int64_t* sizes);
int spmvh_ilu0_export(spmvh_sgs* M, void* const* before, void* const* after);

/* ---- BiCGStab (spmv::bicgstab, host/cg.h; not in the reference) -------------
 * spmvh_bicgstab: BiCGStab from x0 = 0 for a matrix that need not be
 * symmetric.  dinv: NULL, or the inverse diagonal of a right preconditioner
 * (device, rows doubles, finite and nonzero).  x must not overlap b or dinv.
 * *num_its = the iterations completed; *status (may be NULL) = 0 (tolerance
 * met or kmax reached), 1 (rhat.v == 0: the iteration wrote nothing) or 2
 * (omega == 0 or rho == 0: x, r and the last residual norm are valid).
 * rnorm_history (may be NULL): kmax + 1 entries, ||r_0|| .. ||r_k||.
 * ws: a reusable spmv::BicgstabWorkspace (may be NULL).  flags: bit 0 ->
 * CgOptions::time_spmv (*spmv_ms_total, *spmv_launches, both may be NULL; two
 * SpMVs per iteration), bit 2 switches CgOptions::consumer_reductions off,
 * bits 8-15 CgOptions::poll_every (0 = default). */
typedef struct spmvh_bicgstab_workspace spmvh_bicgstab_workspace;
int spmvh_bicgstab_workspace_create(spmvh_exec* exec,
                                    spmvh_bicgstab_workspace** ws);
int spmvh_bicgstab_workspace_destroy(spmvh_bicgstab_workspace* ws);
int spmvh_bicgstab_workspace_reserve_timing(spmvh_bicgstab_workspace* ws,
                                            int iterations);
int spmvh_bicgstab(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                   const double* b, double* x, const double* dinv, int kmax,
                   double rtol, int* num_its, int* status,
                   double* rnorm_history, spmvh_bicgstab_workspace* ws,
                   int flags, double* spmv_ms_total, int* spmv_launches);

/* ---- Restarted GMRES (spmv::gmres, host/cg.h; not in the reference) ---------
 * spmvh_gmres: GMRES(restart) from x0 = 0 with a right preconditioner for a
 * matrix that need not be symmetric.  The preconditioner: none (dinv NULL,
 * cheb_degree 0, sgs NULL), the diagonal dinv, chebyshev_apply (cheb_degree >=
 * 1, dinv or NULL, lmin, lmax) or sgs_apply (sgs; excludes the others).  1 <=
 * restart <= 64.  x must not overlap b or dinv.  *num_its = the inner steps
 * completed; *status (may be NULL) = 0 (tolerance met or kmax reached), 1 (the
 * lucky breakdown: x solves the system) or 2 (a zero pivot: x is the update of
 * the columns before it).  rnorm_history (may be NULL): kmax + 1 entries.
 * ws: a reusable spmv::GmresWorkspace (may be NULL).  flags: bit 0 ->
 * CgOptions::time_spmv (*spmv_ms_total, *spmv_launches, both may be NULL; one
 * SpMV per inner step), bits 8-15 CgOptions::poll_every (0 = default).
 * spmvh_gmres_check_arguments: the argument rules alone (no device). */
typedef struct spmvh_gmres_workspace spmvh_gmres_workspace;
int spmvh_gmres_workspace_create(spmvh_exec* exec, spmvh_gmres_workspace** ws);
int spmvh_gmres_workspace_destroy(spmvh_gmres_workspace* ws);
int spmvh_gmres_workspace_reserve_timing(spmvh_gmres_workspace* ws,
                                         int iterations);
int spmvh_gmres_check_arguments(int restart, int kmax, int cheb_degree,
                                double lmin, double lmax);
int spmvh_gmres(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                const double* b, double* x, const double* dinv,
                int cheb_degree, double lmin, double lmax, spmvh_sgs* sgs,
                int restart, int kmax, double rtol, int* num_its, int* status,
                double* rnorm_history, spmvh_gmres_workspace* ws, int flags,
                double* spmv_ms_total, int* spmv_launches);

/* ---- Aggregation multigrid (spmv::AmgPreconditioner, host/cg.h) -----------------
 * spmvh_amg_check_options: the rules of spmv::AmgOptions, no device.
 * spmvh_amg_symbolic_*: one coarsening step of host/amg_build.h on HOST
 * arrays, no device.  Symmetric input: the stored strictly lower block and a
 * diagonal array.  sizes[4] = {aggregates, coarse entries, sources, expanded
 * entries}; _get copies out what is not NULL: agg (nrows), member_ptr
 * (aggregates + 1), member (nrows), the coarse pattern rowptr (aggregates + 1)
 * and colind, src_ptr (coarse entries + 1), src, and the expanded rows xrow_ptr
 * (nrows + 1), xrow_col, xrow_src.  A source >= 0 indexes values, < 0 is
 * diagonal[~src].
 * spmvh_amg_create: options = NULL (defaults) or 7 doubles {theta, max_levels,
 * min_coarse_rows, smooth_degree, coarse_degree, eig_ratio, coarse_scale}.
 * It and spmvh_amg_refresh fail with "diagonal is not positive" or, where a
 * level's bound max_i |row i| / d_i is not finite and > 0, "the row-sum bound
 * is not finite"; after a failed refresh every use fails until one succeeds.
 * spmvh_amg_info: info[4] = {levels, plan_bytes, symbolic us, numeric us}.
 * spmvh_amg_level_info: sizes[2] = {rows, stored entries}, *lmax the bound.
 * spmvh_amg_level_matrix: host copies of a level >= 1 (NULL outputs skipped).
 * spmvh_amg_apply: z = M^-1 r, device vectors, the host does not wait.
 * spmvh_amg_set_tail_rows: AmgPreconditioner::set_tail_rows (0 = no tail; a
 * negative value fails with "tail_rows" before anything else is looked at);
 * spmvh_amg_check_tail_rows: that rule alone, no device.
 * spmvh_amg_tail_levels: the number of levels the fused launch runs, 0 = none.
 * spmvh_amg_tail_lanes (an addition for the tests alone, so that a case can
 * assert which row order ran): lanes per row of `level`'s product inside the
 * tail as its plan reported them (0 = one lane per row), -1 = not a level of
 * the tail.  It reads spmv_hip_csr_plan_get's keys "algo" and "lanes_per_row",
 * the latter a getter added for this purpose.
 * spmvh_amg_apply_block: spmv::amg_apply_block -- Z = M^-1 R for nrhs
 * INTERLEAVED vectors (element (i, c) at V[i * nrhs + c], device, rows * nrhs
 * doubles each, any alignment, not overlapping: "overlaps"; 1 <= nrhs <= 8:
 * "nrhs"), on the executor's current stream; column c has the bits of
 * spmvh_amg_apply on column c.  spmvh_amg_apply_block_check_arguments: those
 * two rules alone, no device, the pointers are compared, never read.
 * spmvh_amg_release_block_scratch: frees the block scratch (it waits); the
 * next block application allocates it again.
 * spmvh_pcg_block_amg: spmv::pcg_block with BlockPreconditioner::amg = M; the
 * arguments of spmvh_pcg_block with M in place of dinv / the SGS handle.
 * spmvh_pcg_block_amg_check_arguments: the rules of pcg_block with the third
 * preconditioner (exactly one of the three: "preconditioner"; "rows" also for
 * amg_rows), no device.
 * spmvh_pcg_amg: the arguments of spmvh_pcg_sgs.  spmvh_gmres_amg: the
 * arguments of spmvh_gmres and the AMG handle (excludes the others). */
typedef struct spmvh_amg spmvh_amg;
typedef struct spmvh_amg_symbolic spmvh_amg_symbolic;
int spmvh_amg_check_options(double theta, int max_levels,
                            int64_t min_coarse_rows, int smooth_degree,
                            int coarse_degree, double eig_ratio,
                            double coarse_scale);
int spmvh_amg_symbolic_create(const int32_t* rowptr, const int32_t* colind,
                              const double* values, const double* diagonal,
                              int64_t nrows, int64_t ncols_local, int symmetric,
                              double theta, spmvh_amg_symbolic** sym,
                              int64_t* sizes);
int spmvh_amg_symbolic_get(spmvh_amg_symbolic* sym, int32_t* agg,
                           int32_t* member_ptr, int32_t* member,
                           int32_t* rowptr, int32_t* colind, int64_t* src_ptr,
                           int32_t* src, int64_t* xrow_ptr, int32_t* xrow_col,
                           int32_t* xrow_src);
int spmvh_amg_symbolic_destroy(spmvh_amg_symbolic* sym);
int spmvh_amg_create(spmvh_exec* exec, spmvh_matrix* A, const double* options,
                     spmvh_amg** M);
/* spmvh_amg_create_ex: spmvh_amg_create with AmgOptions::setup (0 host, 1
 * device) and ::order (-1 none given, 0 hashed, 1 natural; device only: setup =
 * 0 with an order >= 0 fails).  spmvh_amg_setup_info: info[4] = {aggregate us, build us, the
 * peak of the device setup's temporaries in bytes, setup}; zeros for setup =
 * host.  spmvh_amg_level_rounds: rounds[2] = the rounds of pass 1 and pass 3
 * of the step from `level` (0: host, or no step).  spmvh_amg_step_sizes /
 * _export: spmv_hip_amg_plan_sizes / _export of the level's plan (sizes all 0
 * and _export an error where the level has none); host arrays, NULL skipped. */
int spmvh_amg_create_ex(spmvh_exec* exec, spmvh_matrix* A, const double* options,
                        int setup, int order, spmvh_amg** M);
int spmvh_amg_setup_info(spmvh_amg* M, int64_t* info);
int spmvh_amg_level_rounds(spmvh_amg* M, int level, int* rounds);
int spmvh_amg_step_sizes(spmvh_amg* M, int level, int64_t* sizes);
int spmvh_amg_step_export(spmvh_amg* M, int level, int32_t* agg,
                          int32_t* member_ptr, int32_t* member, int64_t* src_ptr,
                          int32_t* src, int64_t* xrow_ptr, int32_t* xrow_src);
int spmvh_amg_destroy(spmvh_amg* M);
int spmvh_amg_refresh(spmvh_amg* M, spmvh_matrix* A);
int spmvh_amg_info(spmvh_amg* M, int64_t* info);
int spmvh_amg_level_info(spmvh_amg* M, int level, int64_t* sizes, double* lmax);
int spmvh_amg_aggregates(spmvh_amg* M, int level, int32_t* agg);
int spmvh_amg_level_matrix(spmvh_amg* M, int level, int32_t* rowptr,
                           int32_t* colind, double* values);
int spmvh_amg_apply(spmvh_exec* exec, spmvh_amg* M, const double* r, double* z);
int spmvh_amg_apply_block(spmvh_exec* exec, spmvh_amg* M, const double* R,
                          double* Z, int nrhs);
int spmvh_amg_apply_block_check_arguments(int nrhs, int64_t rows,
                                          const double* R, const double* Z);
int spmvh_amg_release_block_scratch(spmvh_amg* M);
int spmvh_pcg_block_amg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                        const double* B, double* X, int nrhs, spmvh_amg* M,
                        int kmax, double rtol, int* max_its, int* iterations,
                        double* rnorm_history, spmvh_pcg_block_workspace* ws,
                        int flags, double* spmv_ms_total, int* spmv_launches);
int spmvh_pcg_block_amg_check_arguments(int nrhs, int kmax, int has_dinv,
                                        int has_sgs, int has_amg,
                                        int64_t sgs_rows,
                                        int64_t sgs_negative_pivots,
                                        int64_t amg_rows, int64_t rows,
                                        const double* B, const double* X,
                                        const double* dinv);
int spmvh_amg_check_tail_rows(int64_t max_rows);
int spmvh_amg_set_tail_rows(spmvh_amg* M, int64_t max_rows);
int spmvh_amg_tail_levels(spmvh_amg* M, int* tail_levels);
int spmvh_amg_tail_lanes(spmvh_amg* M, int level, int* lanes);
int spmvh_pcg_amg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                  spmvh_amg* M, const double* b, double* x, int kmax,
                  double rtol, int* num_its, double* rnorm_history,
                  spmvh_sgs_workspace* ws, int flags, double* spmv_ms_total,
                  int* spmv_launches);
int spmvh_gmres_amg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                    const double* b, double* x, const double* dinv,
                    int cheb_degree, double lmin, double lmax, spmvh_sgs* sgs,
                    int restart, int kmax, double rtol, int* num_its,
                    int* status, double* rnorm_history,
                    spmvh_gmres_workspace* ws, int flags, double* spmv_ms_total,
                    int* spmv_launches, spmvh_amg* amg);

/* ---- Preconditioned MINRES (spmv::minres, host/cg.h; not in the reference) ---
 * spmvh_minres: MINRES from x0 = 0 for a symmetric matrix that need not be
 * definite.  At most one of dinv (a positive device vector), sgs (SGS, or
 * ILU(0) without negative pivots) and amg may be given; all NULL: no
 * preconditioner.  rnorm_history (may be NULL): kmax + 1 doubles, receives
 * hist[0..*num_its], the residual in the M^-1-norm.  *status (may be NULL): 0
 * converged or kmax reached, 1 the Lanczos process ended (x is exact), 2 the
 * preconditioner is not positive definite (r.M^-1 r < 0), 3 a singular
 * direction.  ws: a reusable spmv::MinresWorkspace (may be NULL).  flags: bit 0
 * -> CgOptions::time_spmv, bits 8-15 -> poll_every (0 = default).
 * spmvh_minres_check_rules: minres_check_rules of solver_args.h alone (no
 * device; the pointers are compared, never dereferenced). */
typedef struct spmvh_minres_workspace spmvh_minres_workspace;
int spmvh_minres_workspace_create(spmvh_exec* exec, spmvh_minres_workspace** ws);
int spmvh_minres_workspace_destroy(spmvh_minres_workspace* ws);
int spmvh_minres_workspace_reserve_timing(spmvh_minres_workspace* ws,
                                          int iterations);
int spmvh_minres_check_rules(int kmax, int has_dinv, int has_sgs, int has_amg,
                             int64_t sgs_rows, int64_t sgs_negative_pivots,
                             int64_t amg_rows, int64_t rows, const double* b,
                             const double* x, const double* dinv);
int spmvh_minres(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                 const double* b, double* x, const double* dinv,
                 spmvh_sgs* sgs, spmvh_amg* amg, int kmax, double rtol,
                 int* num_its, int* status, double* rnorm_history,
                 spmvh_minres_workspace* ws, int flags, double* spmv_ms_total,
                 int* spmv_launches);

/* ---- LSQR (spmv::lsqr, host/cg.h; not in the reference) -----------------------
 * spmvh_lsqr: LSQR from x0 = 0 for any matrix, rectangular or square: min ||A x
 * - b||, with damp > 0 min ||A x - b||^2 + damp^2 ||x||^2.  b: the matrix's
 * local rows, x: its owned columns (device pointers of any alignment).  hist_r
 * and hist_ar (each may be NULL): kmax + 1 doubles, receive [0..*num_its] of
 * the estimates of ||b - A x|| and of ||A^T (b - A x) - damp^2 x||.  *status
 * (may be NULL): 0 kmax reached or hist_r[k] / hist_r[0] < rtol, 1 the
 * least-squares test hist_ar[k] / (||A|| hist_r[k]) < ltol, 2 the
 * bidiagonalisation ended (x is exact).  ws: a reusable spmv::LsqrWorkspace (may
 * be NULL).  flags: bit 0 -> CgOptions::time_spmv (both products are counted: 2
 * launches per iteration), bits 8-15 -> poll_every (0 = default).
 * spmvh_lsqr_check_rules: lsqr_check_rules of solver_args.h alone (no device;
 * the pointers are compared, never dereferenced). */
typedef struct spmvh_lsqr_workspace spmvh_lsqr_workspace;
int spmvh_lsqr_workspace_create(spmvh_exec* exec, spmvh_lsqr_workspace** ws);
int spmvh_lsqr_workspace_destroy(spmvh_lsqr_workspace* ws);
int spmvh_lsqr_workspace_reserve_timing(spmvh_lsqr_workspace* ws, int iterations);
int spmvh_lsqr_check_rules(int kmax, double ltol, double damp, int64_t rows,
                           int64_t cols, const double* b, const double* x);
int spmvh_lsqr(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
               const double* b, double* x, int kmax, double rtol, double ltol,
               double damp, int* num_its, int* status, double* hist_r,
               double* hist_ar, spmvh_lsqr_workspace* ws, int flags,
               double* spmv_ms_total, int* spmv_launches);

/* ---- LOBPCG (spmv::lobpcg, host/cg.h; not in the reference) -------------------
 * spmvh_lobpcg: the nev smallest (flags bit 1: largest) eigenpairs of a symmetric
 * matrix.  X: device block of rows * nev doubles in the mult_block layout, the
 * initial guess on entry, the Ritz vectors on exit.  At most one of dinv, sgs and
 * amg (each may be NULL).  eigenvalues, true_resnorm: nev doubles;
 * resnorm_history: nev * (kmax + 1) doubles, -1.0 beyond a column's last (each
 * may be NULL).  *status (may be NULL): 0, or 1 the basis collapsed.  ws: a
 * reusable spmv::LobpcgWorkspace (may be NULL).  flags: bit 0 -> time_spmv, bit 1
 * -> largest, bits 8-15 -> poll_every (0 = default).
 * spmvh_lobpcg_check_rules: lobpcg_check_rules of solver_args.h alone (no
 * device). */
typedef struct spmvh_lobpcg_workspace spmvh_lobpcg_workspace;
int spmvh_lobpcg_workspace_create(spmvh_exec* exec, spmvh_lobpcg_workspace** ws);
int spmvh_lobpcg_workspace_destroy(spmvh_lobpcg_workspace* ws);
int spmvh_lobpcg_workspace_reserve_timing(spmvh_lobpcg_workspace* ws,
                                          int iterations);
int spmvh_lobpcg_check_rules(int nev, int kmax, double rtol, double atol,
                             int has_dinv, int has_sgs, int has_amg,
                             int64_t sgs_rows, int64_t sgs_negative_pivots,
                             int64_t amg_rows, int64_t rows);
int spmvh_lobpcg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A, double* X,
                 int nev, const double* dinv, spmvh_sgs* sgs, spmvh_amg* amg,
                 int kmax, double rtol, double atol, int* num_its, int* status,
                 double* eigenvalues, double* resnorm_history,
                 double* true_resnorm, int* restarts, spmvh_lobpcg_workspace* ws,
                 int flags, double* spmv_ms_total, int* spmv_launches);
/* spmvh_lobpcg_gen: the pencil A x = lambda B x, B symmetric positive definite
 * with A's rows and A's ghosts (rule "pencil"; B == NULL: spmvh_lobpcg).  X is
 * B-orthonormal on exit, true_resnorm is ||A x_c - theta_c B x_c||, a B that is
 * not positive definite ends with *status 1.  Everything else as spmvh_lobpcg.
 * spmvh_lobpcg_check_pencil: lobpcg_check_pencil of solver_args.h alone (no
 * device): the local row counts and the ghost lists (global indices) of A and
 * B. */
int spmvh_lobpcg_check_pencil(int64_t rows_a, int64_t rows_b,
                              const int64_t* ghosts_a, int64_t num_ghosts_a,
                              const int64_t* ghosts_b, int64_t num_ghosts_b);
int spmvh_lobpcg_gen(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                     spmvh_matrix* B, double* X, int nev, const double* dinv,
                     spmvh_sgs* sgs, spmvh_amg* amg, int kmax, double rtol,
                     double atol, int* num_its, int* status, double* eigenvalues,
                     double* resnorm_history, double* true_resnorm,
                     int* restarts, spmvh_lobpcg_workspace* ws, int flags,
                     double* spmv_ms_total, int* spmv_launches);

/* ---- multi-shift CG (spmv::cg_shifted, host/cg.h; not in the reference) ---------
 * spmvh_cg_shifted: (A + shifts[s] I) x_s = b for s < ns (1..8) from x_s = 0 with
 * one product per iteration; A symmetric positive definite, every shift finite
 * and >= 0 (a HOST array of ns doubles).  b: the matrix's local rows; solution s
 * is the contiguous device vector X + s * ldx, ldx >= rows (any alignment).
 * iterations (may be NULL): ns ints; rnorm_history (may be NULL): ns * (kmax + 1)
 * doubles, hist_s[j] at s * (kmax + 1) + j, -1.0 beyond iterations[s]; *num_its:
 * the largest count.  *status (may be NULL): 0 every shift met rtol or kmax was
 * reached, 1 p.(A p) was not positive (A is not positive definite, or the data
 * are not finite): X is the last iterate.  ws: a reusable
 * spmv::CgShiftedWorkspace (may be NULL).  flags: bit 0 -> CgOptions::time_spmv,
 * bits 8-15 -> poll_every (0 = default).
 * spmvh_cgs_check_rules: cgs_check_rules of solver_args.h alone (no device;
 * shifts is read on the host, b and X are compared, never dereferenced). */
typedef struct spmvh_cgs_workspace spmvh_cgs_workspace;
int spmvh_cgs_workspace_create(spmvh_exec* exec, spmvh_cgs_workspace** ws);
int spmvh_cgs_workspace_destroy(spmvh_cgs_workspace* ws);
int spmvh_cgs_workspace_reserve_timing(spmvh_cgs_workspace* ws, int iterations);
int spmvh_cgs_check_rules(int ns, int kmax, int64_t rows, int64_t ldx,
                          const double* shifts, const double* b, const double* X);
int spmvh_cg_shifted(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                     const double* b, double* X, int64_t ldx,
                     const double* shifts, int ns, int kmax, double rtol,
                     int* num_its, int* iterations, double* rnorm_history,
                     int* status, spmvh_cgs_workspace* ws, int flags,
                     double* spmv_ms_total, int* spmv_launches);

/* ---- IDR(s) (spmv::idrs, host/cg.h; not in the reference) -------------------------
 * spmvh_idrs: IDR(s), 1 <= s <= 8, from x = 0 on sign shadow vectors, with the
 * right preconditioner of spmvh_gmres_amg (dinv, the Chebyshev degree and
 * bounds, sgs / ILU(0), amg; at most one), for a matrix that need not be
 * symmetric: one product per step.  b, x: the matrix's local rows (x at any
 * 8-byte alignment, updated in place).  kappa: 0.7 is the usual choice; seed:
 * of the shadow signs.  rnorm_history (may be NULL): kmax + 1 doubles, hist[0..
 * *num_its] written.  *status (may be NULL): 0 rtol or kmax was reached, 1 a
 * zero or non-finite pivot of M, 2 a zero or non-finite om.  ws: a reusable
 * spmv::IdrsWorkspace (may be NULL).  flags: bit 0 -> time_spmv, bits 8-15 ->
 * poll_every (0 = default).
 * spmvh_idrs_check_rules: idrs_check_rules of solver_args.h alone (no device;
 * the pointers are compared, never dereferenced). */
typedef struct spmvh_idrs_workspace spmvh_idrs_workspace;
int spmvh_idrs_workspace_create(spmvh_exec* exec, spmvh_idrs_workspace** ws);
int spmvh_idrs_workspace_destroy(spmvh_idrs_workspace* ws);
int spmvh_idrs_workspace_reserve_timing(spmvh_idrs_workspace* ws, int iterations);
int spmvh_idrs_check_rules(int s, int kmax, double kappa, int has_dinv,
                           int cheb_degree, double lmin, double lmax,
                           int has_sgs, int has_amg, int64_t pre_rows,
                           int64_t rows, const double* b, const double* x,
                           const double* dinv);
int spmvh_idrs(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
               const double* b, double* x, const double* dinv, int cheb_degree,
               double lmin, double lmax, spmvh_sgs* sgs, spmvh_amg* amg, int s,
               int kmax, double rtol, double kappa, uint64_t seed, int* num_its,
               int* status, double* rnorm_history, spmvh_idrs_workspace* ws,
               int flags, double* spmv_ms_total, int* spmv_launches);

#ifdef __cplusplus
}
#endif
#endif /* SPMV_HOST_C_H */
