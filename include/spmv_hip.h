/*
 * include/spmv_hip.h -- C ABI of libspmv_hip.so, the MI355X (gfx950) backend
 * for the LIBSPMV hot path: fp64/fp32 CSR and symmetric-CSR SpMV, the ghost
 * pack kernel, the CG loop's fused BLAS-1 kernels, device memory/stream
 * plumbing and the RCCL halo / all-reduce transport.
 *
 * This is the drop-in boundary.  Each entry point names the reference
 * interface (file:line relative to the LIBSPMV tree) it stands behind; a
 * `spmv::HipExecutor` (spmv_amd/csrc/host/hip_executor.h) binds exactly these
 * symbols, and INTEGRATION.md shows the same binding inside the reference.
 *
 * Conventions
 *   - Every function returns int: 0 = success, >0 = hipError_t,
 *     >=10000 = 10000 + ncclResult_t, <0 = SPMV_HIP_E*.  Nothing throws,
 *     nothing calls exit().  spmv_hip_error_string() decodes a code.
 *   - All `const T*` / `T*` data arguments are DEVICE pointers unless the
 *     parameter name starts with `host_`.
 *   - `stream` is a hipStream_t passed as void* (NULL = the context's current
 *     stream, see spmv_hip_set_stream).  Nothing synchronises the host unless
 *     its name says so.
 *   - One context per GPU; a context is used by one host thread at a time
 *     (same rule as the reference's executors).
 */
#ifndef SPMV_HIP_H
#define SPMV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPMV_HIP_ABI_VERSION 5

enum {
  SPMV_HIP_OK = 0,
  SPMV_HIP_EINVAL = -1,   /* bad argument (null handle, negative size, ...) */
  SPMV_HIP_ENOMEM = -2,   /* host allocation failed                         */
  SPMV_HIP_ENOTSUP = -3,  /* feature not available in this build           */
  SPMV_HIP_ERANGE = -4,   /* size exceeds a 32-bit index the format fixes  */
  SPMV_HIP_EPEER = -5     /* one-sided halo: a neighbour did not answer in
                             time (an earlier exchange of this window failed) */
};

typedef struct spmv_hip_ctx spmv_hip_ctx;           /* one GPU             */
typedef struct spmv_hip_csr_plan spmv_hip_csr_plan; /* CSRSpMV::_aux_data  */
typedef struct spmv_hip_cg_ws spmv_hip_cg_ws;       /* cg() work vectors   */
typedef struct spmv_hip_cgb_ws spmv_hip_cgb_ws;     /* cg_block() scalars  */
typedef struct spmv_hip_pcg_ws spmv_hip_pcg_ws;     /* pcg() scalars       */
typedef struct spmv_hip_pcgb_ws spmv_hip_pcgb_ws;   /* pcg_block() scalars */
typedef struct spmv_hip_lobpcg_ws spmv_hip_lobpcg_ws; /* lobpcg() scalars */
typedef struct spmv_hip_bicg_ws spmv_hip_bicg_ws;   /* bicgstab() scalars  */
typedef struct spmv_hip_gmres_ws spmv_hip_gmres_ws; /* gmres() scalars     */
typedef struct spmv_hip_comm spmv_hip_comm;         /* RCCL communicator   */

int spmv_hip_abi_version(void);
const char* spmv_hip_error_string(int code);

/* ---- context / device queries ------------------------------------------
 * HipExecutor ctor/dtor, get_num_devices, get_num_cus, synchronize
 * (device_executor.h:82-85; cuda/cuda_executor.cpp:13-47). */
int spmv_hip_device_count(int* count);
int spmv_hip_ctx_create(int device_id, spmv_hip_ctx** ctx);
int spmv_hip_ctx_destroy(spmv_hip_ctx* ctx);
int spmv_hip_ctx_device(const spmv_hip_ctx* ctx, int* device_id);
int spmv_hip_num_cus(const spmv_hip_ctx* ctx, int* num_cus);
int spmv_hip_synchronize(spmv_hip_ctx* ctx); /* whole device */
/* tuning options of a context; EINVAL for an unknown key.
 *   "blas1_nt_min_elems": the CG vector kernels stream vectors of at least
 *   this many elements past the caches (non-temporal loads and stores);
 *   shorter vectors stay cached between kernels.  Default 2^24.
 *   "lat_min_nnz", "lx_min_nnz", "lx_max_x_bytes": from how many entries (up to
 *   how large an x) plans build the lattice / LX forms.
 *   "bake_general": 0 = plan_bake_values on a general plan always returns
 *   SPMV_HIP_ENOTSUP (the CSR-order kernels on the caller's values).
 *   "const_diagonals": 1 (default) = plan_bake_values looks whether every
 *   diagonal of a lattice matrix is constant, bit for bit (constant-coefficient
 *   stencils: the Poisson operators); then the plan keeps ONE number per
 *   diagonal and the per-row presence mask instead of a copy of the values, and
 *   the kernel multiplies by that number -- same products, same sums, same
 *   order, same bits.  0 = always keep (and stream) the values.
 *   "const_tile": lattice lines per lane of that kernel on 3-D lattices (1, 2
 *   or 4; default 4).
 *   "wdia_half": 0 = the wide diagonal form (a baked copy of a general matrix
 *   with <= 32 diagonals) keeps every diagonal even when it finds the matrix
 *   symmetric bit for bit; default 1 = then only the diagonals <= 0.
 *   "poisson_skew_ppm": the device generator below writes a NON-symmetric
 *   variant (lower neighbours -1 - s, upper -1 + s, s = value * 1e-6).
 *   "poisson_stencil": 7 (default) or 27 -- the generator writes the 27-point
 *   operator (all neighbours with |dx|,|dy|,|dz| <= 1; diagonal 26,
 *   off-diagonal -1); its row slabs must be whole planes.
 *   "csr_in_place": 1 = plans make NO copy of the index or value stream of a
 *   matrix without lattice structure -- neither the LX form's 16-bit offsets
 *   (2 B per entry) nor the sliced jagged arrays (10 B per entry): the caller's
 *   CSR arrays are streamed as they are, x windows staged in LDS where the
 *   columns of a row block form <= 8 windows (the XW kernel, 144 B of plan
 *   memory per 256 rows), gathered otherwise.  Default 0.
 *   "xw_min_nnz", "xw_min_x_bytes": from how many entries / how large an x on
 *   such a plan stages the windows; "xw_probe": 1 (default) = its first four
 *   launches -- each a complete product with the same bits -- time the XW
 *   kernel against the gather kernel and the plan keeps the faster one
 *   (csr_plan_get "xw_pick"); 0 = XW wherever its records exist. */
int spmv_hip_ctx_set_option(spmv_hip_ctx* ctx, const char* key, int64_t value);
/* ... and read back (release_csr, put_timeout_ms, the *_min_nnz thresholds,
 * xw_min_x_bytes); SPMV_HIP_EINVAL for a key without a getter */
int spmv_hip_ctx_get_option(const spmv_hip_ctx* ctx, const char* key, int64_t* value);
/*   "lx_min_nnz": csr_plan_create builds the LX form of a general matrix
 *   (LDS-staged x windows + 16-bit column offsets, 2 B per entry of extra
 *   device memory) from this many entries on.  Default 2^20; a huge value
 *   switches the form off.
 *   "lx_max_x_bytes": ... and only for matrices whose input vector
 *   (num_cols * 8 bytes) is at most this large.  Default 128 MiB (the form
 *   pays while x stays in the Infinity Cache).
 *   "lx_codes" (0 / 1, default 1): ... with a second index array of 4-bit
 *   codes (0.5 B per entry) for the row blocks whose offsets are the row's
 *   lane plus one of at most 16 distances; the LDS-DMA kernel streams it in
 *   place of the 16-bit offsets (plan keys "lx4", "lx4_blocks", "lx4_all"). */

/* ---- streams / events ---------------------------------------------------
 * CudaExecutor::set/reset/get_cuda_stream (cuda/cuda_executor.h:72-76). */
int spmv_hip_stream_create(spmv_hip_ctx* ctx, void** stream);
/* high_priority != 0: the stream's kernels are dispatched ahead of other
 * ready work -- used for the halo stream so the small RCCL send/recv kernel is
 * placed before the CU-filling local SpMV that becomes ready at the same time */
int spmv_hip_stream_create_priority(spmv_hip_ctx* ctx, int high_priority,
                                    void** stream);
int spmv_hip_stream_destroy(spmv_hip_ctx* ctx, void* stream);
int spmv_hip_stream_synchronize(spmv_hip_ctx* ctx, void* stream);
int spmv_hip_set_stream(spmv_hip_ctx* ctx, void* stream); /* NULL = reset */
int spmv_hip_get_stream(const spmv_hip_ctx* ctx, void** stream);
int spmv_hip_event_create(spmv_hip_ctx* ctx, int timing, void** event);
int spmv_hip_event_destroy(spmv_hip_ctx* ctx, void* event);
int spmv_hip_event_record(spmv_hip_ctx* ctx, void* event, void* stream);
int spmv_hip_event_synchronize(spmv_hip_ctx* ctx, void* event);
int spmv_hip_stream_wait_event(spmv_hip_ctx* ctx, void* stream, void* event);
int spmv_hip_event_elapsed_ms(spmv_hip_ctx* ctx, void* start, void* stop,
                              float* ms);

/* ---- memory ---------------------------------------------------------------
 * DeviceExecutor::_alloc/_free/_memset/_copy/_copy_async/_copy_from/_copy_to
 * (device_executor.h:129-139). */
int spmv_hip_alloc(spmv_hip_ctx* ctx, size_t num_bytes, void** ptr);
int spmv_hip_free(spmv_hip_ctx* ctx, void* ptr);
int spmv_hip_host_alloc(spmv_hip_ctx* ctx, size_t num_bytes, void** host_ptr);
int spmv_hip_host_free(spmv_hip_ctx* ctx, void* host_ptr);
int spmv_hip_memset_async(spmv_hip_ctx* ctx, void* ptr, int value,
                          size_t num_bytes, void* stream);
int spmv_hip_copy_d2d_async(spmv_hip_ctx* ctx, void* dst, const void* src,
                            size_t num_bytes, void* stream);
int spmv_hip_copy_h2d_async(spmv_hip_ctx* ctx, void* dst,
                            const void* host_src, size_t num_bytes,
                            void* stream);
int spmv_hip_copy_d2h_async(spmv_hip_ctx* ctx, void* host_dst, const void* src,
                            size_t num_bytes, void* stream);
/* peer copy between two contexts (cuda/cuda_executor.cpp:82-94) */
int spmv_hip_copy_peer_async(spmv_hip_ctx* dst_ctx, void* dst,
                             spmv_hip_ctx* src_ctx, const void* src,
                             size_t num_bytes, void* stream);

/* ---- CSR SpMV -------------------------------------------------------------
 * CSRSpMV<T>::init / run / finalize (csr_kernels.h:26-78); reference
 * arithmetic csr_kernels.cpp:20-52.
 *
 * plan_create inspects the (device-resident) row pointer once and picks the
 * kernel and launch shape; it stores no copy of the matrix (plan_bake_values_*
 * below is the one, explicit exception).  `symmetric`
 * selects the strictly-lower + diagonal kernel.  rowptr/colind may be NULL
 * when num_non_zeros == 0 (csr_matrix.cpp:34).
 *
 * Plan creation also analyses the index arrays and, where the matrix allows,
 * bakes a compressed form of their CONTENT into the plan (all of them produce
 * the same bits as the plain kernels):
 *   lattice form   every block of 256 rows has its columns at row + one of
 *                  <= 8 constant offsets: no index stream at all, values by
 *                  LDS-DMA one row block ahead
 *   LX form        few contiguous column windows per row block: x staged in
 *                  LDS, 16-bit column offsets
 *   row list       mostly-empty blocks (SPMV_HIP_ALGO_ROWLIST)
 *   symmetric      the symmetric lattice form (<= 3 constant lower offsets) or
 *                  the transposed map (entries sorted by column): atomic-free
 * CONTRACT: a plan with such a form must be launched with the very rowptr /
 * colind pointers it was created with -- the kernels no longer read colind,
 * so other arrays of the same shape would silently compute with the old
 * structure; spmv returns SPMV_HIP_EINVAL instead.  `values`, `in`, `out` are
 * free to change from call to call.
 *
 * run computes out = alpha * A * in + beta * out.
 *   - beta == 0: out is write-only and never read.
 *   - general kernel, SPMV_HIP_ALGO_ROWBLOCK: each row is summed left to
 *     right in fp64 without FMA contraction, i.e. bit-identical to
 *     csr_kernels.cpp:41-51.
 *   - symmetric kernel (strictly lower block): the reference's sequential
 *     order (csr_kernels.cpp:26-40) seen from the row -- finalise
 *     fl(alpha*sum + beta*out), then add fl(fl(alpha*v)*in[r]) for the
 *     entries (r, i) of the row's column in ascending r -- with no atomics:
 *     bit-identical to the reference.  plan_set "sym_det" / "slat" = 0 (or a
 *     block that is not strictly lower) selects the older atomic kernels: out
 *     is scaled by beta, every term accumulated with hardware fp64 atomics,
 *     order of additions not deterministic.
 *   - `dot_partials` (optional, may be NULL; not for a diagonal-only
 *     symmetric block): fuses
 *     the CG dot product.  The kernel writes spmv_hip_dot_partials_len()
 *     doubles whose sum is sum_i in[i] * (alpha * (A in)_i), this block's own
 *     share (beta*out is not included, so the shares of a local and a remote
 *     block add up to in . (A in)); reduce with spmv_hip_reduce_partials_f64.
 *     The atomic symmetric kernels use the mirror identity: row i contributes
 *     in_i * alpha * (2 (d_i in_i + (L in)_i) - d_i in_i).
 */
enum {
  SPMV_HIP_ALGO_AUTO = 0,
  SPMV_HIP_ALGO_ROWBLOCK = 1, /* row blocks streamed through LDS, exact order */
  SPMV_HIP_ALGO_VECTOR = 2,   /* sub-wavefront per row, shuffle reduction     */
  SPMV_HIP_ALGO_SCALAR = 3,   /* one lane per row (short rows, reference)     */
  SPMV_HIP_ALGO_ROWLIST = 4   /* mostly-empty block: walk the compacted list of
                                 non-empty rows (built by plan_create), exact
                                 order; general kernel only                    */
};

int spmv_hip_csr_plan_create(spmv_hip_ctx* ctx, int32_t num_rows,
                             int32_t num_cols, int64_t num_non_zeros,
                             const int32_t* rowptr, const int32_t* colind,
                             int symmetric, int algo,
                             spmv_hip_csr_plan** plan);
int spmv_hip_csr_plan_destroy(spmv_hip_csr_plan* plan);
/* Bookkeeping for tests: the number of device arrays the CALLING THREAD has
 * allocated inside the plan builders (csr, mcgs, ilu0, amg plans and their
 * temporaries) and not yet freed there.  A builder that refuses its input
 * leaves it where it was.  An array a builder hands to the caller (the coarse
 * colind of spmv_hip_amg_plan_build) leaves the count with the hand-over. */
int spmv_hip_plan_live_allocations(int64_t* count);
/* Optional: let the plan keep its OWN copy of the matrix values in the layout
 * its kernel streams best -- one array per lower offset plus the diagonal
 * ("symmetric diagonal form", a DIA fast path).  This is what
 * CSRSpMV::init does with the matrix it is given (csr_kernels.h:26-78; the
 * cuSPARSE descriptor of cuda/csr_kernels.cu binds the values there too).
 *   symmetric plan   in the symmetric lattice form (<= 3 constant lower
 *                    offsets); pass values and diagonal
 *   general plan     (diagonal = NULL) in the lattice form, square, with <= 3
 *                    distinct |col - row| > 0.  If the device check finds the
 *                    matrix SYMMETRIC entry for entry and bit for bit, the
 *                    plan keeps the lower half and the diagonal only (49
 *                    instead of 73 B per row of a 7-point matrix); if not,
 *                    ALL values by offset (the "full" form: the bytes of the
 *                    CSR values, no index stream, no row pointer).  Either
 *                    way the kernel sums each row in the general kernel's own
 *                    order: same bits as csr_kernels.cpp:41-51.
 *                    A general matrix on MORE diagonals (<= 32: 27-point
 *                    stencils) takes the "wide diagonal form": values by
 *                    offset + a 32-bit presence mask per row; only the
 *                    diagonals <= 0 when the matrix is symmetric bit for bit.
 *   constant diagonals  (either storage; ctx option "const_diagonals") when
 *                    every diagonal is constant, bit for bit, the plan keeps
 *                    no values at all: one number per diagonal + the mask.
 * plan_create and plan_bake_values wait for `stream` before they start (the
 * plan's clock counts the plan's work) and return after the plan's own kernels
 * have completed.
 * Anything else: SPMV_HIP_ENOTSUP, nothing changes.  Costs (offsets + 1) * 8 B
 * per row of device memory (constant diagonals: 1 or 4 B per row).  A launch that passes these very `values` (and
 * `diagonal`) pointers takes the diagonal-form kernel; a launch with other
 * pointers takes the CSR-order kernels as before.  CONTRACT: whoever rewrites
 * the baked arrays in place calls spmv_hip_csr_plan_values_changed (or bakes
 * again, or drops the copy: values = NULL).  A general plan that took neither
 * the lattice nor the LX form (ragged rows, more than 16 entries per row) keeps
 * its copy in the SLICED JAGGED order instead (spmv_sjds.hip): 64-row slices
 * as jagged diagonals + 16-bit column codes into an LDS-staged copy of x.
 * NARROWED VALUES (fp64 only; ctx option "lx_narrow_values", default 1): a
 * general plan in the LX form with its LDS-DMA records, whose values no form
 * above took, is still SPMV_HIP_ENOTSUP -- its kernel keeps CSR order -- but
 * when EVERY value is a normal binary32 number or +-0 held exactly (integers,
 * dyadic rationals, single-precision data) the plan keeps an fp32 copy (4 B per
 * entry) and launches with these `values` stream it in place of the 8-byte
 * values, widening in the row sum: the same products and adds in the same
 * order, y and the fused dot bit for bit.  One value that is not exact and the
 * plan streams the caller's fp64 array as before.  plan_get "lx_v32" says
 * which; plan_set "lx_v32" 0 / 1 switches while a copy exists.  The contract
 * above holds: rewritten values need plan_values_changed or a new bake. */
int spmv_hip_csr_plan_bake_values_f64(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan,
                                      const double* values,
                                      const double* diagonal, void* stream);
int spmv_hip_csr_plan_bake_values_f32(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan,
                                      const float* values, const float* diagonal,
                                      void* stream);
/* The caller has REWRITTEN the baked `values` (and `diagonal`) arrays in place
 * -- a time step with new coefficients on the same sparsity, the common use of
 * a raw C ABI; the reference's CSRMatrix is immutable (csr_matrix.cpp:22-59)
 * and needs no such call.  Refreshes every copy the plan keeps, from the
 * pointers it was baked with, in `stream` order (the call returns after the
 * refresh has completed):
 *   sliced jagged form   the copy is rewritten in place, nothing is allocated;
 *   diagonal forms       the checks run again on the new values (constant
 *                        diagonals? still symmetric?) and the copy is rebuilt
 *                        in the form they allow; a matrix the forms no longer
 *                        hold falls back to the CSR-order kernels (no other
 *                        form is built inside this call: bake again for the
 *                        sliced jagged form);
 *   fp32 copies of the mixed SpMV likewise.
 * A plan without a baked copy: nothing to do.  SPMV_HIP_OK in all these cases
 * -- launches with the same pointers then return the NEW matrix's product.
 * Without this call they return the OLD one (the copy is the plan's own; the
 * sliced jagged form, which reads its long rows from the caller's arrays, a
 * mixture of the two): the contract of plan_bake_values.  plan_get "values_changed_us" = what the last
 * call cost. */
int spmv_hip_csr_plan_values_changed(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan,
                                     void* stream);
/* PLAN MEMORY (ABI 4).  A plan that took one of the value-baking forms holds a
 * complete copy of the matrix in its own format; the caller's `colind` and
 * `values` are then read by nothing but a fallback.  (The reference's CSRMatrix
 * owns exactly one copy of the matrix, spmv/csr_matrix.cpp:34-70; with a plan
 * on top the device would hold two.)
 *   plan_owns_matrix     *mask = the arrays the plan no longer needs to read:
 *                        bit 0 (1) = colind, bit 1 (2) = values.  Non-zero for a
 *                        general plan in a diagonal form (values by offset,
 *                        or no values at all where every diagonal is constant)
 *                        or in the sliced jagged form WITHOUT long rows (those
 *                        are streamed from the caller's arrays), and for
 *                        symmetric storage in the merged sliced jagged form
 *                        without long rows (its kernel reads the merged copy,
 *                        `rowptr` and `diagonal`); 0 otherwise (CSR-order
 *                        kernels, LX, XW, lattice kernels, the other symmetric
 *                        forms, an fp32 twin baked for the mixed SpMV).
 *                        `rowptr` is never given up (4 B per row).
 *   plan_release_matrix  the caller frees the arrays of `mask` (a subset of
 *                        what plan_owns_matrix reports, else SPMV_HIP_EINVAL).
 *                        From then on the plan COMPARES the `colind` / `values`
 *                        pointers of a launch with the ones it was built from
 *                        and never reads them, and refuses with SPMV_HIP_EINVAL
 *                        whatever would: plan_values_changed, plan_bake_values_*
 *                        (a drop included), plan_set of a key that selects
 *                        another kernel, a launch the baked form does not take
 *                        (other pointers, an x that is not 16-byte aligned).
 *                        A symmetric plan also drops what only those refused
 *                        paths read (transposed map, value positions: 16 B per
 *                        stored entry).  Irreversible for the plan's lifetime. */
int spmv_hip_csr_plan_owns_matrix(const spmv_hip_csr_plan* plan, int* mask);
int spmv_hip_csr_plan_release_matrix(spmv_hip_csr_plan* plan, int mask);
/* ... and the fp32 copy for spmv_hip_csr_spmv_f32f64 (mixed precision) on a
 * general fp64 plan whose values are baked: `values32` is the caller's fp32
 * copy of the CSR values (the same device check runs on its bits).  Launches
 * of spmv_f32f64 with this pointer then stream 17 instead of 33 B of matrix
 * data per row of a 7-point matrix.  values32 = NULL drops the copy. */
int spmv_hip_csr_plan_bake_values_f32f64(spmv_hip_ctx* ctx,
                                         spmv_hip_csr_plan* plan,
                                         const float* values32, void* stream);
int spmv_hip_csr_plan_algo(const spmv_hip_csr_plan* plan, int* algo);
/* The plane-walk order table the lattice kernels take (host arithmetic only, no
 * device: for inspection and tests).  Slot (round * L + step) * grid + w holds
 * the row block workgroup w computes at that step, -1 = none; planes are
 * `plane_rows` rows apart; segments = runs along the plane axis (0 = choose).
 * Call with table = NULL for the size. */
int spmv_hip_zwalk_table(int32_t num_rows, int64_t plane_rows, int grid,
                         int segments, int32_t* table, int64_t capacity,
                         int64_t* num_slots, int* segments_out);
/* Knobs (key/value; EINVAL for an unknown key or a value out of range):
 *   "algo" "lanes_per_row" "chunks" "nontemporal" "xcd_group" "blocks_per_cu"
 *   "nt_store"                           the plain general kernels
 *   "lx" "lx_chunks"                     LX form on/off (built plans only)
 *   "lat" "lat_blocks_per_cu" "lat_xcd_group" "lat_chain"   lattice form
 *                  (lat_chain: x handed from plane to plane in registers)
 *   "slat" "slat_blocks_per_cu"          symmetric lattice form
 *   "sdia" "sdia_chain" "sdia_nt"        symmetric diagonal form (baked plans):
 *                  on/off, plane chain on/off, non-temporal streams (bit mask)
 *   "sdia_tile" "sdia_tile_segments" "sdia_tile_blocks_per_cu"   constant
 *                  diagonals on a 3-D lattice: lattice lines per lane (1, 2,
 *                  4), its own plane-walk table, workgroups per CU
 *   "lxw" "lxw_blocks_per_cu"            LX form: the LDS-DMA kernel on/off
 *   "lx4" "lx4_lut"                      ... streaming 4-bit codes in place of
 *                  the 16-bit offsets for the row blocks that have them (1 needs
 *                  the codes: context option "lx_codes", default 1, at plan
 *                  creation; same launch grid, same bits); lx4_lut: the
 *                  dictionary look-up, 1 = LDS table, 2 = select tree
 *   "lx_ring"                            ... in the ring variant of that kernel
 *                  (three LDS slots, two row blocks in flight per workgroup):
 *                  get = 1 when a launch would take it -- narrowed values
 *                  ("lx_v32"), codes with the LDS table, EVERY row block
 *                  staged, coded and fitting (get "lx_ring_blocks"), and,
 *                  unless asked for by name, at least 128 row blocks per
 *                  workgroup; set 1 asks for it by name and is refused on an
 *                  ineligible plan, set 0 keeps the two-slot kernel.  Same
 *                  grid, same bits.  Context option "lx_ring" (default 1; 0 =
 *                  never, 2 = wherever eligible) is read at plan creation.
 *                  The ring kernel reads a row's span from the plan's row
 *                  descriptors (get "lx_rowdesc" = 1 when the plan has them;
 *                  2 B per row, built with the DMA records): a row block
 *                  with a row of more than 31 entries is not eligible.
 *   "lx_vcode"                           ... streaming 4-bit VALUE codes and a
 *                  16-entry fp64 dictionary per row block in place of the
 *                  values (fp64 plans; built by plan_bake_values_f64 on a
 *                  ring-eligible plan when EVERY row block's stored values
 *                  have at most 16 distinct bit patterns; they need not be
 *                  exact in fp32 and take precedence over "lx_v32").  get = 1
 *                  when the plan has them and they are switched on; set 0
 *                  gives the launch without them, set 1 switches them back
 *                  on.  get "lx_vcode_blocks": row blocks that qualified at
 *                  the last bake, "lx_vcode_all": 1 when all did (the arrays
 *                  exist only then: 0.5 B per entry + 128 B per row block).
 *                  Context option "lx_vcode" (default 1) is read at plan
 *                  creation (the switch) and at every bake (the arrays).
 *                  Same grid, same bits.
 *   "lx_ring_pwr"                        x pieces a wave of the ring kernel
 *                  issues per step: 0 = 3 where the plan stages at most 12
 *                  pieces, else 4 (get: the figure in use); 4 = always 4
 *   "lxw_grid_cap"                       at most that many workgroups in the
 *                  DMA kernels' grid (0 = no cap): lets a small matrix give a
 *                  workgroup many row blocks
 *   "xw" "xw_probe"                      the same kernel on the caller's CSR
 *                  arrays (plans with XW records): on/off -- 1 asks for it by
 *                  name and ends the probe --; xw_probe 1 = let the next four
 *                  launches choose between it and the gather kernel again
 *   "wdia" "wdia_xcd_group" "wdia_blocks_per_cu" "wdia_zwalk"
 *   "wdia_zwalk_segments"                wide diagonal form (baked plans)
 *   "wdia_box" "wdia_box_segments" "wdia_box_blocks_per_cu"   constant
 *                  27-point box stencils: lattice lines per lane (0 = the
 *                  general kernel, 2, 4), its plane-walk table, workgroups/CU
 *   "zwalk" "zwalk_segments"             plane-walk row-block order of the
 *                  three lattice kernels (every workgroup walks a 256-row
 *                  column of the lattice from plane to plane): use the table;
 *                  (re)build it with that many runs along the plane axis (0 =
 *                  choose), whatever the size of the matrix
 *   "sym_det"                            transposed-map kernel (0: atomics)
 *   "sym_window" "sym_rows"              the atomic symmetric kernels */
int spmv_hip_csr_plan_set(spmv_hip_csr_plan* plan, const char* key, int value);
/* What the plan decided and what it cost: "algo", "lanes_per_row" (of
 * SPMV_HIP_ALGO_VECTOR; the fused AMG tail asks for it); "lat", "lx", "slat", "sdia",
 * "sym_det" (1 = that form is in use), "lat_blocks", "lx_blocks", "lx_staged";
 * "lattice_d1", "lattice_d2" (row distance of the next grid line / plane when
 * the matrix is a 3-D lattice, else 0), "zwalk", "zwalk_segments",
 * "zwalk_grid", "lat_chain", "sdia_chain", "sdia_nt", "sdia_offsets" (lower
 * offsets of the baked copy), "sdia_general" (baked from a general matrix: 1 = symmetric, half stored; 2 =
 * full form), "sdia_mixed" (fp32 copy), "sdia_const" (constant diagonals: no
 * values kept), "sdia_tile" (lines per lane in use), "sdia_tile_walk"; "lxw",
 * "lxw_grid" (its fp64 launch grid), "lx4" (4-bit codes in use), "lx4_blocks"
 * (row blocks that have codes), "lx4_all" (every staged block has), "lx4_lut";
 * "xw", "xw_staged" (row blocks with staged windows), "xw_pick" (1 = the XW
 * kernel runs, 0 = the plan's probe found the gather kernel faster, -1 = the
 * probe's four launches are not all complete), "xw_probe_xw_us",
 * "xw_probe_gather_us" (what it measured);
 * "wdia", "wdia_offsets", "wdia_half", "wdia_const", "wdia_box", "wdia_mixed", "wdia_d2",
 * "wdia_zwalk", "wdia_zwalk_segments";
 * "blocks_per_cu", "nontemporal"; "plan_us" (wall time of plan creation, its
 * analysis kernels included), "plan_mem_us" (the part of it -- and of later
 * bakes -- spent inside hipMalloc / hipFree) and "plan_kib" (device memory the
 * plan owns). */
int spmv_hip_csr_plan_get(const spmv_hip_csr_plan* plan, const char* key,
                          int* value);

/* out = alpha * A * in + beta * out  (CSRSpMV<T>::run, csr_kernels.cpp:20-52),
 * every row summed left to right, mul and add rounded separately: the bits of
 * the reference loops, special values included (tests/test_gpu_special_values.py
 * holds every plan form to this):
 *   - only stored entries take part: an absent entry of a form stored by
 *     offset, a padded slot, a lane past the row's end and a load clamped into
 *     range contribute nothing -- not 0 * x, which is NaN under an Inf or NaN x;
 *   - NaN and Inf propagate as in the loop: a stored 0.0 under an Inf x gives
 *     NaN, a NaN in x reaches every row (and the fused dot) that reads it.
 *     NaNs are one class: sign and payload of a generated NaN are not defined;
 *   - the sign of a zero follows the loop (the sum starts at +0.0, symmetric
 *     storage: at diagonal[i] * in[i]), with the beta == 0 note below;
 *   - the left-to-right order holds through overflow: a partial sum that
 *     reaches +-Inf stays there, whatever another order would give;
 *   - subnormals: fp64 and fp32 products and sums are not flushed (gradual
 *     underflow, as the reference on x86-64); the mixed f32f64 kernels widen
 *     fp32-subnormal values exactly.
 * The order-tolerant kernels -- SPMV_HIP_ALGO_VECTOR and the atomic symmetric
 * kernels (plan_get "sym_det" == 0 without the lattice form) -- sum in another
 * order: they promise the rounding bound on rows that are finite in the loop
 * and a non-finite result on the others, not the bits, the kind of non-finite
 * value or the sign of a zero.
 * TWO defined differences to the reference loops:
 *   beta == 0 means `out` is WRITE-ONLY -- the kernels store alpha*sum and never
 *   read out[i] (the reference computes alpha*sum + 0*out[i] on a
 *   buffer cg.cpp:40 never initialises, so a NaN/Inf there would poison it).
 *   Consequence for the sign of zero: where alpha*sum is -0.0 the reference's
 *   "+ 0*out[i]" turns it into +0.0 (for out[i] >= +0) while this library
 *   returns -0.0.  The two compare equal (np.array_equal, ==); only the sign
 *   bit differs, and only for rows whose sum is an exact negative zero.
 *   SPMV_HIP_ALGO_ROWLIST at beta == 1 (the remote block of a partitioned matrix,
 *   once per CG iteration) walks the listed rows only: a row WITHOUT entries
 *   keeps out[i], where the loop computes alpha*0 + out[i].  The two differ only
 *   where out[i] is an exact -0.0 (the loop gives +0.0 for alpha*0 == +0.0) and
 *   for a non-finite alpha (the loop gives NaN); they compare equal otherwise.
 *   plan_set "rowlist_exact" 1 makes the launch go over all rows at beta == 1
 *   too and removes the difference.  Every other beta, every other kernel and a
 *   block without any entry (num_non_zeros == 0, spmv and spmm) follow the loop:
 *   a row without entries gets alpha*0 + beta*out[i], alpha*0 at beta == 0.
 * dot_partials (may be NULL; general fp64 and symmetric fp64): the launch also
 * leaves spmv_hip_dot_partials_len() partial sums of in . (alpha * A * in),
 * the block's share of p.Ap in CG (cg.cpp:63). */
int spmv_hip_csr_spmv_f64(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* plan,
                          int32_t num_rows, int32_t num_cols,
                          int64_t num_non_zeros, const int32_t* rowptr,
                          const int32_t* colind, const double* values,
                          const double* diagonal, double alpha,
                          const double* in, double beta, double* out,
                          double* dot_partials, void* stream);
/* Mixed precision (device_executor.h:88-99 carries the float
 * visitors): `values` in fp32 -- half the matrix bytes -- x, y and every
 * product and sum in fp64.  General (non-symmetric) blocks; the same plan
 * serves both value types.  With fp32-representable values (the Poisson
 * matrix) the result equals spmv_hip_csr_spmv_f64 bit for bit. */
int spmv_hip_csr_spmv_f32f64(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* plan,
                             int32_t num_rows, int32_t num_cols,
                             int64_t num_non_zeros, const int32_t* rowptr,
                             const int32_t* colind, const float* values,
                             double alpha, const double* in, double beta,
                             double* out, double* dot_partials, void* stream);
int spmv_hip_csr_spmv_f32(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* plan,
                          int32_t num_rows, int32_t num_cols,
                          int64_t num_non_zeros, const int32_t* rowptr,
                          const int32_t* colind, const float* values,
                          const float* diagonal, float alpha, const float* in,
                          float beta, float* out, void* stream);

/* ---- transposed product (Matrix::transpmult, spmv/Matrix.h:78-81) ----------
 * For a GENERAL plan and a column range [col_begin, col_end) of its block:
 *   out[j - col_begin] = alpha * s_j + beta * out[j - col_begin]
 * where s_j starts at +0.0 and adds v * in[i] left to right over the stored
 * entries (i, j, v) of column j in ascending i, then ascending position in row
 * i (duplicates keep their CSR order): the row-order CSR sum of the transpose
 * built by a STABLE sort of the entries by column, mul and add rounded
 * separately.  `in` holds num_rows entries, `out` col_end - col_begin; as in
 * the forward product beta == 0 makes `out` write-only (an empty column gives
 * alpha * 0.0, -0.0 for alpha < 0).
 *   plan_build_transpose  builds the transposed map on the device (t_ptr:
 *                         col_end - col_begin + 1 ints, t_row / t_pos: one int
 *                         per entry) and the form of the product; `values` are
 *                         the caller's values, value_bytes = 8 (fp64) or 4
 *                         (fp32).  SPMV_HIP_EINVAL when an entry's column lies
 *                         outside [col_begin, col_end), for a symmetric plan and
 *                         after plan_release_matrix.  A second call replaces
 *                         the first.
 *   plan_get "t_form"     0 none;  1 COPY: the values permuted into column
 *                         order and an inner general plan on the transpose's
 *                         CSR -- every forward form runs A^T (keys "t.<key>"
 *                         read the inner plan, e.g. "t.sdia_const");  2 IN
 *                         PLACE: one lane per output column over (t_ptr, t_row,
 *                         t_pos) and the caller's values, no value copy (the
 *                         map itself is 8 B per entry + 4 B per column) -- ctx
 *                         option "csr_in_place", a launch with a `values`
 *                         pointer other than the one the build saw, or no
 *                         memory for the copy;  3 SELF: a square block over
 *                         [0, n) that is its own transpose bit for bit (with
 *                         row-block kernels) runs the forward plan, no copy,
 *                         only t_pos kept.  "t_plan_us" (the build's wall
 *                         time), "t_kib" (device memory of the map, the copy
 *                         and the inner plan).
 *   plan_set "t_in_place" 1 forces the in-place kernel (A/B tests), 0 undoes
 *                         it; "t.<key>" sets a knob of the inner plan.
 * spmv_hip_csr_plan_values_changed refreshes the copy and runs the
 * self-transpose check again (a block that is no longer its own transpose
 * takes the in-place kernel: nothing is allocated); plan_destroy frees
 * everything.  The bits do not depend on the form. */
int spmv_hip_csr_plan_build_transpose(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan,
                                      const int32_t* rowptr, const int32_t* colind,
                                      const void* values, int value_bytes,
                                      int32_t col_begin, int32_t col_end,
                                      void* stream);
int spmv_hip_csr_spmvt_f64(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* plan,
                           int32_t num_rows, int32_t num_cols,
                           int64_t num_non_zeros, const int32_t* rowptr,
                           const int32_t* colind, const double* values,
                           double alpha, const double* in, double beta,
                           double* out, void* stream);
int spmv_hip_csr_spmvt_f32(spmv_hip_ctx* ctx, const spmv_hip_csr_plan* plan,
                           int32_t num_rows, int32_t num_cols,
                           int64_t num_non_zeros, const int32_t* rowptr,
                           const int32_t* colind, const float* values,
                           float alpha, const float* in, float beta, float* out,
                           void* stream);

/* ---- multi-vector product (Matrix::mult_block) -------------------------------
 * Y = alpha A X + beta Y for a block of k >= 1 vectors.  LAYOUT: a block is
 * INTERLEAVED (row-major) -- element (i, c), 0 <= c < k, lives at X[i * k + c];
 * `in` holds num_cols * k elements, `out` num_rows * k, both device pointers.
 * For every column c, Y[:, c] has THE SAME BITS as the single-vector product
 * spmv_hip_csr_spmv_* on X[:, c] for the same storage (rows summed left to
 * right, mul and add rounded separately; beta == 0: `out` is write-only).
 * k == 1 is the existing product.
 *   plan_get "mv_form"   the last launch: 0 none yet;  1 NATIVE: one pass over
 *                        the caller's CSR arrays for all k vectors (general
 *                        plans, fp64 vectors, fp64 or fp32 values, k = 2, 4, 8,
 *                        `in` and `out` 16-byte aligned);  2 PER COLUMN: X is
 *                        de-interleaved into plan-owned scratch, the plan's
 *                        single-vector launch runs once per column in whatever
 *                        form the plan took, Y is interleaved back -- symmetric
 *                        storage, any other k, a plan after
 *                        plan_release_matrix, the fp32 library type.  k == 1
 *                        reports 2 as well: one column, the single-vector
 *                        launch on `in` / `out` themselves, no scratch.
 *   plan_get "mv_kib"    the scratch held: (num_cols + num_rows) * k elements,
 *                        each column rounded up to 4 elements; allocated on
 *                        first use, grown on demand, never shrunk, freed with
 *                        the plan (512^3 rows, k = 8: about 17 GB).  When
 *                        it cannot be allocated the call returns the HIP error
 *                        code and launches nothing.
 *   plan_set "mv_native" 0 forces the per-column form (A/B tests), 1 (the
 *                        default) undoes it.
 * The calls record the form in the plan, so the plan is not const here, and
 * two of them on one plan must not run concurrently.  SPMV_HIP_EINVAL, before
 * anything is launched: NULL handles, k < 1, shapes other than the plan's, `in`
 * and `out` overlapping.  `diagonal` as in spmv_hip_csr_spmv_* (NULL for the
 * mixed product, which takes general plans only). */
int spmv_hip_csr_spmm_f64(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan,
                          int32_t num_rows, int32_t num_cols,
                          int64_t num_non_zeros, const int32_t* rowptr,
                          const int32_t* colind, const double* values,
                          const double* diagonal, double alpha, const double* in,
                          double beta, double* out, int k, void* stream);
int spmv_hip_csr_spmm_f32f64(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan,
                             int32_t num_rows, int32_t num_cols,
                             int64_t num_non_zeros, const int32_t* rowptr,
                             const int32_t* colind, const float* values,
                             const double* diagonal, double alpha,
                             const double* in, double beta, double* out, int k,
                             void* stream);
int spmv_hip_csr_spmm_f32(spmv_hip_ctx* ctx, spmv_hip_csr_plan* plan,
                          int32_t num_rows, int32_t num_cols,
                          int64_t num_non_zeros, const int32_t* rowptr,
                          const int32_t* colind, const float* values,
                          const float* diagonal, float alpha, const float* in,
                          float beta, float* out, int k, void* stream);
/* Tiled transposes between the interleaved layout (n x k) and k contiguous
 * columns, column c at columns[c * ld ... + n), ld >= n:
 *   interleave    out[i * k + c] = columns[c * ld + i]
 *   deinterleave  columns[c * ld + i] = in[i * k + c]
 * Source and destination must not overlap. */
int spmv_hip_interleave_f64(spmv_hip_ctx* ctx, int64_t n, int k,
                            const double* columns, int64_t ld, double* out,
                            void* stream);
int spmv_hip_interleave_f32(spmv_hip_ctx* ctx, int64_t n, int k,
                            const float* columns, int64_t ld, float* out,
                            void* stream);
int spmv_hip_deinterleave_f64(spmv_hip_ctx* ctx, int64_t n, int k, const double* in,
                              int64_t ld, double* columns, void* stream);
int spmv_hip_deinterleave_f32(spmv_hip_ctx* ctx, int64_t n, int k, const float* in,
                              int64_t ld, float* columns, void* stream);
/* Ghost pack of an interleaved block, the multi-vector form of spmv_hip_gather_*:
 * out[g * k + c] = in[indices[g] * k + c]. */
int spmv_hip_gather_block_f64(spmv_hip_ctx* ctx, int num_indices,
                              const int32_t* indices, int k, const double* in,
                              double* out, void* stream);
int spmv_hip_gather_block_f32(spmv_hip_ctx* ctx, int num_indices,
                              const int32_t* indices, int k, const float* in,
                              float* out, void* stream);

/* ---- ghost pack -------------------------------------------------------------
 * DeviceExecutor::gather_ghosts_run (device_executor.h:123-126;
 * reference_executor.cpp:150-164): out[i] = in[indices[i]]. */
int spmv_hip_gather_f64(spmv_hip_ctx* ctx, int num_indices,
                        const int32_t* indices, const double* in, double* out,
                        void* stream);
int spmv_hip_gather_f32(spmv_hip_ctx* ctx, int num_indices,
                        const int32_t* indices, const float* in, float* out,
                        void* stream);

/* ---- reverse halo accumulate -------------------------------------------------
 * The owner-side loop of L2GMap::reverse_update (L2GMap.cpp:921-922,947-948):
 * out[indices[i]] += in[i].  The indices of ONE call must be distinct (one
 * neighbour's segment of the index buffer); the caller issues one call per
 * neighbour, in neighbour order, which reproduces the reference's ascending-i
 * accumulation order bit for bit. */
int spmv_hip_scatter_add_f64(spmv_hip_ctx* ctx, int num_indices,
                             const int32_t* indices, const double* in,
                             double* out, void* stream);
int spmv_hip_scatter_add_f32(spmv_hip_ctx* ctx, int num_indices,
                             const int32_t* indices, const float* in,
                             float* out, void* stream);

/* ---- CG building blocks -----------------------------------------------------
 * spmv::cg (cg.cpp:21-98).  All scalars live on the device (precedent:
 * cuda/cg.cuda.cu:73-84); the host never waits inside an iteration.
 *
 * Reductions are two-stage and deterministic: a kernel writes
 * spmv_hip_dot_partials_len() per-block partial sums, then
 * spmv_hip_reduce_partials_f64 adds them in index order into one double.
 */
int spmv_hip_dot_partials_len(const spmv_hip_ctx* ctx, int* len);
int spmv_hip_dot_partial_f64(spmv_hip_ctx* ctx, int64_t n, const double* x,
                             const double* y, double* partials, void* stream);
int spmv_hip_reduce_partials_f64(spmv_hip_ctx* ctx, const double* partials,
                                 double* result, void* stream);

/* Device-resident CG state: scalar history + flags.
 *   rr[k]  = ||r_k||^2 (k = 0..kmax), pAp[k] = p_k . A p_k (k = 1..kmax)
 *   done   = 1 once sqrt(rr[k]) / sqrt(rr[0]) < rtol; kstop = that k.
 * After `done` every cg_* kernel and every SpMV issued through
 * spmv_hip_cg_guard_* is a no-op, so the host may enqueue iterations ahead
 * without reading anything back (cg.cpp:80-81 semantics: x, r updated, p not).
 */
int spmv_hip_cg_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_cg_ws** ws);
int spmv_hip_cg_ws_destroy(spmv_hip_cg_ws* ws);
int spmv_hip_cg_ws_reset(spmv_hip_cg_ws* ws, double rtol, void* stream);
/* device addresses of the scalar slots (for the all-reduce) */
int spmv_hip_cg_ws_rr(spmv_hip_cg_ws* ws, int k, double** slot);
int spmv_hip_cg_ws_pAp(spmv_hip_cg_ws* ws, int k, double** slot);
int spmv_hip_cg_ws_partials(spmv_hip_cg_ws* ws, double** partials);
int spmv_hip_cg_ws_done_flag(spmv_hip_cg_ws* ws, const int32_t** done);
/* kmax the workspace was created with: its history holds kmax + 1 doubles */
int spmv_hip_cg_ws_capacity(const spmv_hip_cg_ws* ws, int* kmax);
/* copies {done, kstop} (2 x int32) and rr[0..kmax] to the host (async on
 * stream).  `host_rr_len` = doubles the caller's `host_rr` can take: fewer than
 * kmax + 1 (spmv_hip_cg_ws_capacity) -> SPMV_HIP_EINVAL, nothing is copied.
 * Either destination may be NULL (then it is skipped; host_rr_len ignored).
 * (ABI 2: the length argument is new -- ABI 1 wrote kmax + 1 doubles into
 * whatever it was given.) */
int spmv_hip_cg_ws_read_async(spmv_hip_cg_ws* ws, int32_t* host_done_kstop,
                              double* host_rr, size_t host_rr_len,
                              void* stream);

/* x += alpha p ; r -= alpha Ap ; partials of r.r   (cg.cpp:66-73)
 * alpha = (s*s)/pAp[k] with s = sqrt(rr[k-1]), evaluated on the device. */
int spmv_hip_cg_update_xr_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                              int64_t n, const double* p, const double* Ap,
                              double* x, double* r, void* stream);
/* The same updates regrouped so that p is read once per iteration (8 vector
 * passes instead of 9); per-element arithmetic identical:
 *   update_r : r -= alpha Ap ; partials of r.r            (cg.cpp:66,70,73)
 *   update_xp: x += alpha p ; stop test ; p = beta p + r   (cg.cpp:69,77-85)
 * x still takes the update of the converging iteration, p does not. */
int spmv_hip_cg_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                             int64_t n, const double* Ap, double* r,
                             void* stream);
int spmv_hip_cg_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                              int64_t n, const double* r, double* x, double* p,
                              void* stream);
/* ---- consumer-side reductions (one rank) -----------------------------------------
 * The same two updates with the reducer launches folded into their prologues:
 * every workgroup adds the partials of the preceding producer itself, in the
 * reducers' order (bit-identical scalars), workgroup 0 stores pAp[k] / rr[k].
 *   update_r_cs : [p.Ap partials of the SpMV (+ pap_partials2, may be NULL)]
 *                 -> pAp[k]; stop test of iteration k-1; r -= alpha Ap;
 *                 partials of r.r into the workspace's second partial array
 *   update_xp_cs: [those r.r partials] -> rr[k]; x += alpha p; stop test;
 *                 p = beta p + r
 * For a single rank only: no all-reduce can be placed between producer and
 * consumer. */
int spmv_hip_cg_update_r_cs_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                                int64_t n, const double* Ap, double* r,
                                const double* pap_partials2, void* stream);
int spmv_hip_cg_update_xp_cs_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                                 int64_t n, const double* r, double* x,
                                 double* p, void* stream);
/* update_xp_cs with the x update deferred by one iteration: p lives in two
 * buffers that swap, x is read and written every second iteration (9 vector
 * passes per pair of iterations instead of 10; every element sees the same
 * operations in the same order, so the bits are those of update_xp_cs).
 *   update_p2_cs  (iteration k, k odd from a fresh start): [r.r partials] ->
 *                 rr[k]; stop test; p_out = beta p_in + r.  x is not touched
 *                 unless iteration k meets the tolerance: then x += alpha_k
 *                 p_in and nothing is pending.
 *   update_x2p_cs (iteration k >= 2 after an update_p2_cs of k-1, p_prev its
 *                 p_in and p_cur its p_out): -> rr[k]; x += alpha_(k-1) p_prev;
 *                 x += alpha_k p_cur; stop test; p_prev = beta p_cur + r.
 *   flush_x       after a loop that ended with update_p2_cs of iteration k:
 *                 x += alpha_k p (its p_in), unless the solve is done or
 *                 iteration k met the tolerance.
 * Every vector 16-byte aligned; p_in / p_out (p_prev / p_cur) distinct. */
int spmv_hip_cg_update_p2_cs_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                                 int64_t n, const double* r, double* x,
                                 const double* p_in, double* p_out,
                                 void* stream);
int spmv_hip_cg_update_x2p_cs_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                                  int64_t n, const double* r, double* x,
                                  double* p_prev, const double* p_cur,
                                  void* stream);
int spmv_hip_cg_flush_x_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                            int64_t n, const double* p, double* x,
                            void* stream);
/* CG start (cg.cpp:39-50) in one pass: r = p = b, x = 0, partials of r.r in
 * the workspace (then spmv_hip_cg_reduce_rr(0) installs rr[0]) */
int spmv_hip_cg_init_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int64_t n,
                         const double* b, double* r, double* p, double* x,
                         void* stream);
/* Mixed-precision CG support: fp32 copy of a value array;
 * y += a x; residual replacement r = b - Ax (Ax given) with the partials of
 * r.r left in the workspace (then spmv_hip_cg_reduce_rr(k) installs rr[k]).
 * respect_done = 1 inside the loop (no-op once converged), 0 for the closing
 * check of the true residual. */
int spmv_hip_convert_f64_f32(spmv_hip_ctx* ctx, int64_t n, const double* in,
                             float* out, void* stream);
int spmv_hip_axpy_f64(spmv_hip_ctx* ctx, int64_t n, double a, const double* x,
                      double* y, void* stream);
int spmv_hip_cg_residual_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws,
                             int respect_done, int64_t n, const double* b,
                             const double* Ax, double* r, void* stream);
/* convergence test on rr[k] then p = beta p + r  (cg.cpp:77-85) */
int spmv_hip_cg_update_p_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                             int64_t n, const double* r, double* p,
                             void* stream);
/* partials -> rr[k] / pAp[k] (local part; all-reduce it afterwards) */
int spmv_hip_cg_reduce_rr(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                          void* stream);
int spmv_hip_cg_reduce_pAp(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                           void* stream);
/* same, adding a second partial array (the remote block's share of p.Ap,
 * spmv_hip_dot_partials_len() doubles) */
int spmv_hip_cg_reduce_pAp2(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int k,
                            const double* partials2, void* stream);
/* r.r partials for k = 0 (cg.cpp:47) */
int spmv_hip_cg_dot_rr_f64(spmv_hip_ctx* ctx, spmv_hip_cg_ws* ws, int64_t n,
                           const double* r, void* stream);

/* ---- CG for a block of right-hand sides (spmv::cg_block) ------------------------
 * nrhs independent CG recurrences (cg.cpp:21-98 once per column) in lockstep on
 * INTERLEAVED blocks, the layout of the multi-vector product: element (i, c)
 * of a block lives at V[i * nrhs + c], M * nrhs doubles.  1 <= nrhs <=
 * SPMV_HIP_CGB_MAX_NRHS; anything else is SPMV_HIP_EINVAL.  nrhs = 2, 4, 8 run
 * streaming kernels on 16-byte elements (every block 16-byte aligned, except B
 * of init); the other widths run one thread per row with scalar accesses.
 *
 * Device state of a workspace:
 *   rr[k][c]  = ||r_k||^2 of column c (k = 0..kmax), pAp[k][c] = p_k . A p_k:
 *               the nrhs scalars of one k are contiguous, so one all-reduce of
 *               nrhs doubles on the slot address serves every column;
 *   done[c]   = 1 once column c has stopped, kstop[c] = its iteration count:
 *               sqrt(rr[k][c]) / sqrt(rr[0][c]) < rtol, or rr[0][c] == 0 (then
 *               kstop = 0 and x = 0);
 *   all_done  = 1 once every column has stopped.
 * The iteration in which a column meets the tolerance updates its x and r and
 * leaves its p (cg.cpp:80-81); from then on no kernel changes its x, r, p and
 * its scalars are not extended (slots beyond kstop[c] keep the zero of the
 * reset).  After all_done every cgb_* kernel returns at once, so the host may
 * enqueue iterations ahead.  The bits of column c depend on the matrix, on
 * column c of B, on nrhs and on c only. */
#define SPMV_HIP_CGB_MAX_NRHS 8
/* int32 words of the state copied by cgb_ws_read_async:
 * [0] all_done, [1 + c] done[c], [1 + SPMV_HIP_CGB_MAX_NRHS + c] kstop[c] */
#define SPMV_HIP_CGB_STATE_WORDS (1 + 2 * SPMV_HIP_CGB_MAX_NRHS)
int spmv_hip_cgb_ws_create(spmv_hip_ctx* ctx, int kmax, int nrhs,
                           spmv_hip_cgb_ws** ws);
int spmv_hip_cgb_ws_destroy(spmv_hip_cgb_ws* ws);
int spmv_hip_cgb_ws_reset(spmv_hip_cgb_ws* ws, double rtol, void* stream);
/* kmax and nrhs the workspace was created with */
int spmv_hip_cgb_ws_capacity(const spmv_hip_cgb_ws* ws, int* kmax, int* nrhs);
/* device addresses of the nrhs scalars of iteration k (for the all-reduce) */
int spmv_hip_cgb_ws_rr(spmv_hip_cgb_ws* ws, int k, double** slot);
int spmv_hip_cgb_ws_pAp(spmv_hip_cgb_ws* ws, int k, double** slot);
/* the partial array, [spmv_hip_dot_partials_len()][nrhs] */
int spmv_hip_cgb_ws_partials(spmv_hip_cgb_ws* ws, double** partials);
int spmv_hip_cgb_ws_done_flag(spmv_hip_cgb_ws* ws, const int32_t** all_done);
/* copies the state words (above) and rr[0..kmax][nrhs] to the host (async on
 * stream).  host_state_len < SPMV_HIP_CGB_STATE_WORDS or host_rr_len <
 * (kmax + 1) * nrhs (cgb_ws_capacity) -> SPMV_HIP_EINVAL, nothing is copied.
 * Either destination may be NULL (then it is skipped, its length ignored). */
int spmv_hip_cgb_ws_read_async(spmv_hip_cgb_ws* ws, int32_t* host_state,
                               size_t host_state_len, double* host_rr,
                               size_t host_rr_len, void* stream);
/* R = P = B ; X = 0 ; partials of r.r (then cgb_reduce_rr(0) installs rr[0]) */
int spmv_hip_cgb_init_f64(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int64_t M,
                          const double* B, double* R, double* P, double* X,
                          void* stream);
/* partials of p.Ap per column */
int spmv_hip_cgb_dot_f64(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int64_t M,
                         const double* P, const double* AP, void* stream);
/* partials -> pAp[k] / rr[k] (local part; all-reduce nrhs doubles afterwards).
 * reduce_pAp(k) first raises done[c] for the columns that stopped in iteration
 * k - 1 (at k = 1: the columns with rr[0][c] == 0), and all_done. */
int spmv_hip_cgb_reduce_pAp(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int k,
                            void* stream);
int spmv_hip_cgb_reduce_rr(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int k,
                           void* stream);
/* update_r : r -= alpha_c Ap ; partials of r.r            (cg.cpp:66,70,73)
 * update_xp: x += alpha_c p ; stop test ; p = beta_c p + r (cg.cpp:69,77-85)
 * per column, with the arithmetic of spmv_hip_cg_update_r_f64 / _xp_f64 */
int spmv_hip_cgb_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int k,
                              int64_t M, const double* AP, double* R,
                              void* stream);
int spmv_hip_cgb_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_cgb_ws* ws, int k,
                               int64_t M, const double* R, double* X, double* P,
                               void* stream);

/* ---- CG with a diagonal preconditioner (spmv::pcg) -------------------------------
 * The preconditioner is the vector `dinv` of its inverse; z = dinv * r
 * (elementwise) is never stored, every kernel that needs it forms it in
 * registers.  From x0 = 0, with `.` the global dot product:
 *   r0 = b; p1 = dinv*r0; rz[0] = r0.(dinv*r0); rr[0] = r0.r0
 *   k = 1..kmax:  alpha = rz[k-1] / pAp[k];  x += alpha p;  r -= alpha Ap;
 *                 rz[k] = r.(dinv*r); rr[k] = r.r;
 *                 stop when sqrt(rr[k]) / sqrt(rr[0]) < rtol (x, r updated, p not)
 *                 beta = rz[k] / rz[k-1];  p = beta p + dinv*r
 * Products and sums are separate roundings.
 *
 * Device state of a workspace:
 *   {rz[k], rr[k]} (k = 0..kmax) are ADJACENT, a pair of doubles per k: one
 *   all-reduce of 2 doubles on the pair's address serves both; pAp[k] (k =
 *   1..kmax); done = 1 once the solve has stopped, kstop = that k: the k whose
 *   rr[k] met the tolerance, or 0 when rr[0] == 0 (then x = 0: the rule of
 *   cg_block, not cg()'s run to kmax on NaNs);
 *   three partial arrays of spmv_hip_dot_partials_len() doubles: p.Ap (filled
 *   by the SpMV's fused dot or spmv_hip_dot_partial_f64), r.z and r.r.
 * After `done` every pcg_* kernel returns at once, so the host may enqueue
 * iterations ahead.  An iteration index outside its range (0..kmax for the
 * slots and reduce_rz_rr, 1..kmax elsewhere) is SPMV_HIP_EINVAL. */
int spmv_hip_pcg_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_pcg_ws** ws);
int spmv_hip_pcg_ws_destroy(spmv_hip_pcg_ws* ws);
int spmv_hip_pcg_ws_reset(spmv_hip_pcg_ws* ws, double rtol, void* stream);
/* kmax the workspace was created with: its history holds kmax + 1 pairs */
int spmv_hip_pcg_ws_capacity(const spmv_hip_pcg_ws* ws, int* kmax);
/* device addresses of the pair {rz[k], rr[k]} and of pAp[k] (all-reduce) */
int spmv_hip_pcg_ws_rz_rr(spmv_hip_pcg_ws* ws, int k, double** pair);
int spmv_hip_pcg_ws_pAp(spmv_hip_pcg_ws* ws, int k, double** slot);
/* the p.Ap partial array (for Matrix::mult_dot / spmv_hip_dot_partial_f64) */
int spmv_hip_pcg_ws_partials(spmv_hip_pcg_ws* ws, double** partials);
int spmv_hip_pcg_ws_done_flag(spmv_hip_pcg_ws* ws, const int32_t** done);
/* copies {done, kstop} (2 x int32) and the pairs {rz[k], rr[k]}, k = 0..kmax,
 * to the host (async on stream).  host_rz_rr_len = doubles `host_rz_rr` can
 * take: fewer than 2 * (kmax + 1) (pcg_ws_capacity) -> SPMV_HIP_EINVAL, nothing
 * is copied.  Either destination may be NULL (then it is skipped). */
int spmv_hip_pcg_ws_read_async(spmv_hip_pcg_ws* ws, int32_t* host_done_kstop,
                               double* host_rz_rr, size_t host_rz_rr_len,
                               void* stream);
/* start in one pass: r = b ; x = 0 ; p = dinv*b ; partials of r.z and r.r
 * (then pcg_reduce_rz_rr(0) installs the pair 0).  b, dinv: any alignment. */
int spmv_hip_pcg_init_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int64_t n,
                          const double* b, const double* dinv, double* r,
                          double* p, double* x, void* stream);
/* update_r : r -= alpha Ap ; partials of r.(dinv*r) and r.r
 * update_xp: x += alpha p ; stop test ; p = beta p + dinv*r
 * Every vector 16-byte aligned. */
int spmv_hip_pcg_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                              int64_t n, const double* Ap, const double* dinv,
                              double* r, void* stream);
int spmv_hip_pcg_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                               int64_t n, const double* r, const double* dinv,
                               double* x, double* p, void* stream);
/* single-workgroup reducers (local part; all-reduce the slot afterwards).
 * reduce_pAp(k) first raises `done` when iteration k - 1 met the tolerance (at
 * k = 1: when rr[0] == 0); _pAp2 adds a second partial array (the remote
 * block's share of p.Ap); reduce_rz_rr(k) installs the pair k. */
int spmv_hip_pcg_reduce_pAp(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                            void* stream);
int spmv_hip_pcg_reduce_pAp2(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                             const double* partials2, void* stream);
int spmv_hip_pcg_reduce_rz_rr(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                              void* stream);
/* consumer-side forms for ONE rank (see spmv_hip_cg_update_r_cs_f64): every
 * workgroup adds the preceding producer's partials itself, in the reducers'
 * order (the same bits), workgroup 0 stores pAp[k] / the pair k.
 *   update_r_cs : reduce_pAp (+ pap_partials2, may be NULL) + update_r
 *   update_xp_cs: reduce_rz_rr + update_xp */
int spmv_hip_pcg_update_r_cs_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                                 int64_t n, const double* Ap,
                                 const double* dinv, double* r,
                                 const double* pap_partials2, void* stream);
int spmv_hip_pcg_update_xp_cs_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                                  int64_t n, const double* r,
                                  const double* dinv, double* x, double* p,
                                  void* stream);
/* Setup of the Jacobi preconditioner.
 * csr_diagonal: d[i] = the sum of the entries of row i whose column is i, left
 * to right in storage order; 0 when the row has none.  One thread per row.
 * jacobi_invert: dinv[i] = 1.0 / d[i] for every i; *bad_count (a device
 * int32, overwritten) = the number of entries that are not finite or not > 0. */
int spmv_hip_csr_diagonal_f64(spmv_hip_ctx* ctx, int32_t num_rows,
                              const int32_t* rowptr, const int32_t* colind,
                              const double* values, double* d, void* stream);
int spmv_hip_csr_diagonal_f32(spmv_hip_ctx* ctx, int32_t num_rows,
                              const int32_t* rowptr, const int32_t* colind,
                              const float* values, float* d, void* stream);
int spmv_hip_jacobi_invert_f64(spmv_hip_ctx* ctx, int64_t n, const double* d,
                               double* dinv, int32_t* bad_count, void* stream);

/* ---- Chebyshev polynomial preconditioner (spmv::chebyshev_apply, pcg_chebyshev) --
 * z = q(dinv*A) dinv r: the `degree`-step Chebyshev iteration for A z = r from
 * z = 0.  a_j, b_j are the host's chebyshev_coefficients (host/cg.h), passed as
 * kernel arguments; `dinv` is the inverse of a diagonal or NULL (no multiply, no
 * dinv stream).  Elementwise, every product and sum a rounding of its own:
 *   step 0       d = b_0 * (dinv*r) ;                  z = d
 *   step j >= 1  w = A z (the caller's SpMV) ;
 *                d = a_j*d + b_j*(dinv*(r - w)) ;      z = z + d
 * The LAST step does not write d.  Every vector 16-byte aligned unless said.
 *
 * cheb_apply0: step 0 on a stored r; d == NULL: it is the last step (degree 1).
 * cheb_step  : step j >= 1 (`last` != 0: the last one).  ws == NULL: the plain
 *              step of chebyshev_apply.  With the workspace of a pcg_chebyshev
 *              solve it returns at once after `done`, and the last step leaves
 *              the partials of r.z (the new z) for pcg_reduce_rz_rr.
 *
 * pcg_chebyshev runs on a spmv_hip_pcg_ws and on the reducers of pcg
 * (pcg_reduce_pAp, _pAp2, pcg_reduce_rz_rr), with z = M(r) STORED:
 * cheb_init    : r = b ; x = 0 ; partials of r.r ; step 0 (b, dinv: any
 *                alignment).  d == NULL (degree 1): partials of r.z too.
 * cheb_update_r: r -= alpha Ap, alpha = rz[k-1] / pAp[k] ; partials of r.r ;
 *                step 0 on the new r.  d == NULL (degree 1): partials of r.z too.
 * cheb_update_xp: x += alpha p ; stop test of pcg_update_xp ; p = beta p + z.
 * k outside 1..kmax is SPMV_HIP_EINVAL.
 * cheb_scale   : out = dinv * (in / s), in / s when dinv == NULL (any alignment;
 *                `in` and `out` may be the same vector): setup work of
 *                lambda_max_estimate. */
int spmv_hip_cheb_scale_f64(spmv_hip_ctx* ctx, int64_t n, double s,
                            const double* dinv, const double* in, double* out,
                            void* stream);
int spmv_hip_cheb_apply0_f64(spmv_hip_ctx* ctx, int64_t n, double b0,
                             const double* r, const double* dinv, double* d,
                             double* z, void* stream);
int spmv_hip_cheb_step_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int64_t n,
                           double a, double b, int last, const double* w,
                           const double* r, const double* dinv, double* d,
                           double* z, void* stream);
int spmv_hip_cheb_init_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int64_t n,
                           double b0, const double* b, const double* dinv,
                           double* r, double* x, double* d, double* z,
                           void* stream);
int spmv_hip_cheb_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                               int64_t n, double b0, const double* Ap,
                               const double* dinv, double* r, double* d,
                               double* z, void* stream);
int spmv_hip_cheb_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                                int64_t n, const double* z, double* x, double* p,
                                void* stream);

/* ---- Multicolour symmetric Gauss-Seidel (spmv::SgsPreconditioner, pcg_sgs) --------
 * z = M^-1 r, M = (D + L) D^-1 (D + U) in the colour-major ordering of the rows
 * of the local diagonal block, fp64, every product and sum a rounding of its own:
 *   forward,  colours 0 .. C-1:  s = 0; for e in before(i): s = s + a_e * z[col_e]
 *                                z_i = (r_i - s) * dinv_i
 *   backward, colours C-2 .. 0:  t = 0; for e in after(i):  t = t + a_e * z[col_e]
 *                                z_i = z_i - dinv_i * t
 * before(i) / after(i): the off-diagonal entries of row i whose column wears a
 * smaller / larger colour, ascending by column.  One launch per colour and
 * direction (2C - 1); the order between colours is the stream's order alone.
 *
 * The plan is an upload of arrays the HOST built (host/sgs_build.h: colouring,
 * colour-major copy, slices of 64 rows stored column-major, a list of long rows):
 *   perm[pos]        the row at a colour-major position
 *   color_start      num_colors + 1 positions; every colour is worn
 *   dinv             1 / diagonal, by ROW
 *   per part: color_slice / color_long (num_colors + 1), slice_pos0, slice_ptr
 *   (slices + 1), len (by position; -1 = a long row), col / val (entry k of lane
 *   l of slice s at slice_ptr[s] + 64 k + l), long_pos, long_ptr, long_col /
 *   long_val (contiguous).  Columns are in the caller's numbering.
 * plan_create checks every index a kernel will use (SPMV_HIP_EINVAL) and copies;
 * the host arrays may go away afterwards.
 *
 * mcgs_apply: r, z device vectors of num_rows doubles, any alignment, not
 * overlapping.  ws == NULL: the plain application.  With the workspace of a
 * pcg_sgs solve every launch returns at once after `done`.
 *
 * pcg_sgs runs on a spmv_hip_pcg_ws, on the reducers of pcg and on
 * cheb_update_xp, with z = M^-1 r STORED:
 * sgs_init    : r = b ; x = 0 ; partials of r.r (b: any alignment)
 * sgs_update_r: r -= alpha Ap, alpha = rz[k-1] / pAp[k] ; partials of r.r
 * sgs_dot_rz  : partials of r.z for pcg_reduce_rz_rr
 * (r, Ap, z 16-byte aligned; k outside 1..kmax is SPMV_HIP_EINVAL). */
typedef struct spmv_hip_mcgs_plan spmv_hip_mcgs_plan;
typedef struct spmv_hip_mcgs_part {
  const int32_t* color_slice;
  const int32_t* slice_pos0;
  const int64_t* slice_ptr;
  const int32_t* len;
  const int32_t* col;
  const double* val;
  const int32_t* color_long;
  const int32_t* long_pos;
  const int64_t* long_ptr;
  const int32_t* long_col;
  const double* long_val;
} spmv_hip_mcgs_part;
typedef struct spmv_hip_mcgs_host {
  int32_t num_rows;
  int32_t num_colors;
  const int32_t* perm;
  const int32_t* color_start;
  const double* dinv;
  spmv_hip_mcgs_part before, after;
} spmv_hip_mcgs_host;
int spmv_hip_mcgs_plan_create(spmv_hip_ctx* ctx, const spmv_hip_mcgs_host* in,
                              spmv_hip_mcgs_plan** plan);
int spmv_hip_mcgs_plan_destroy(spmv_hip_mcgs_plan* plan);
int spmv_hip_mcgs_plan_bytes(const spmv_hip_mcgs_plan* plan, int64_t* bytes);
int spmv_hip_mcgs_apply_f64(spmv_hip_ctx* ctx, const spmv_hip_mcgs_plan* plan,
                            spmv_hip_pcg_ws* ws, const double* r, double* z,
                            void* stream);
int spmv_hip_sgs_init_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int64_t n,
                          const double* b, double* r, double* x, void* stream);
int spmv_hip_sgs_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int k,
                              int64_t n, const double* Ap, double* r,
                              void* stream);
int spmv_hip_sgs_dot_rz_f64(spmv_hip_ctx* ctx, spmv_hip_pcg_ws* ws, int64_t n,
                            const double* r, const double* z, void* stream);

/* ---- The setup of the multicolour sweeps on the device (additive, ABI 5) -----
 * Both entries read a block's CSR arrays where they lie (device pointers): the
 * rows of a rank with local column numbers, num_cols >= num_rows columns of
 * which those >= num_rows are ghosts and ignored; column == row is the
 * diagonal; symmetric != 0: only column < row is an off-diagonal entry and the
 * block stands for B + B^T.  rowptr may be NULL when nnz == 0.  Nothing of the
 * matrix is copied to the host; rowptr (from 0 to nnz, monotone) and the
 * columns are checked on the device before anything is indexed
 * (SPMV_HIP_EINVAL).  Both wait for the device.
 *
 * mcgs_color: greedy first-fit in a priority order over B + B^T, colour(i) =
 * the smallest colour not worn by a neighbour j with prio(j) > prio(i).
 * order SPMV_HIP_MCGS_NATURAL: prio(i) = -i, the colouring of the host's
 * sgs_color entry for entry (as many rounds as the longest ascending path:
 * slow on long dependency chains); SPMV_HIP_MCGS_HASHED: prio(i) =
 * mix64((i + 1) * 0x9E3779B97F4A7C15), unsigned.  Jones-Plassmann rounds, one
 * launch each, ordered by the stream alone; the result does not depend on
 * scheduling.  colors: num_rows int32 (device).  *rounds: launches until no row
 * was left (counted in batches read back together).  SPMV_HIP_ERANGE if
 * num_rows + 1 rounds did not suffice.
 *
 * mcgs_plan_build: the plan mcgs_plan_create would make from the host
 * builder's arrays for the same colours -- every array equal.  diagonal: the
 * diagonal array of symmetric storage (ignored otherwise: d_i is the sum of
 * the entries (i, i) in storage order).  long_threshold: 64 in the mirror.
 * info[SPMV_HIP_MCGS_INFO_WORDS]: [0] diagonal entries not finite or not > 0
 * (the plan is built all the same: the caller decides), [1] why
 * SPMV_HIP_EINVAL (SPMV_HIP_MCGS_BAD_*, 0: an argument), [2] peak bytes of the
 * temporaries, [3] a row of an improper colouring.  A failure leaves nothing
 * allocated.
 *
 * mcgs_plan_sizes / _export: a plan's arrays copied to host buffers, for
 * plans of either builder.  sizes[SPMV_HIP_MCGS_SIZES_WORDS] = {rows, colours,
 * slices, before: sliced entries, long rows, long entries, after: the same
 * three, device bytes}.  export: every pointer may be NULL; perm / dinv / len
 * rows entries, color_start / color_slice / color_long colours + 1, slice_pos0
 * slices, slice_ptr slices + 1, long_ptr long rows + 1. */
#define SPMV_HIP_MCGS_HASHED 0
#define SPMV_HIP_MCGS_NATURAL 1
#define SPMV_HIP_MCGS_INFO_WORDS 4
#define SPMV_HIP_MCGS_SIZES_WORDS 10
#define SPMV_HIP_MCGS_BAD_ROWPTR 1
#define SPMV_HIP_MCGS_BAD_COLUMN 2
#define SPMV_HIP_MCGS_BAD_COLOR 3
#define SPMV_HIP_MCGS_UNWORN_COLOR 4
#define SPMV_HIP_MCGS_IMPROPER 5
typedef struct spmv_hip_mcgs_export {
  int32_t* color_slice;
  int32_t* slice_pos0;
  int64_t* slice_ptr;
  int32_t* len;
  int32_t* col;
  double* val;
  int32_t* color_long;
  int32_t* long_pos;
  int64_t* long_ptr;
  int32_t* long_col;
  double* long_val;
} spmv_hip_mcgs_export;
int spmv_hip_mcgs_color(spmv_hip_ctx* ctx, int32_t num_rows, int32_t num_cols,
                        int64_t nnz, const int32_t* rowptr, const int32_t* colind,
                        int symmetric, int order, int32_t* colors,
                        int* num_colors, int* rounds, void* stream);
int spmv_hip_mcgs_plan_build(spmv_hip_ctx* ctx, int32_t num_rows,
                             int32_t num_cols, int64_t nnz, const int32_t* rowptr,
                             const int32_t* colind, const double* values,
                             const double* diagonal, int symmetric,
                             const int32_t* colors, int32_t num_colors,
                             int long_threshold, spmv_hip_mcgs_plan** plan,
                             int64_t* info, void* stream);
int spmv_hip_mcgs_plan_sizes(const spmv_hip_mcgs_plan* plan, int64_t* sizes);
int spmv_hip_mcgs_plan_export(const spmv_hip_mcgs_plan* plan, int32_t* perm,
                              int32_t* color_start, double* dinv,
                              const spmv_hip_mcgs_export* before,
                              const spmv_hip_mcgs_export* after);

/* ---- Preconditioned CG for a block of right-hand sides (spmv::pcg_block) ----------
 * pcg_sgs's recurrence with a stored Z = M^-1 R, once per column and in
 * lockstep, on INTERLEAVED blocks (V[i * nrhs + c], 1 <= nrhs <=
 * SPMV_HIP_CGB_MAX_NRHS, anything else SPMV_HIP_EINVAL), under the column rules
 * of cg_block above: own alpha, beta and stop per column, a stopped column
 * frozen, rr[0][c] == 0 stops at k = 0 with x = 0, the bits of column c depend
 * on the matrix, M, column c of B, nrhs and c only.
 *
 * mcgs_apply_block: Z = M^-1 R for the nrhs interleaved vectors on the plan as
 * it is (no second copy): 2 num_colors - 1 launches ordered by the stream
 * alone; column c has the bits of mcgs_apply on column c.  R, Z: num_rows *
 * nrhs doubles, any alignment (16-byte aligned ones take 16-byte gathers at
 * nrhs = 2, 4, 8), not overlapping.  ws == NULL: the plain application; with
 * the workspace of a solve (created for the same nrhs) every launch returns at
 * once after all_done.
 *
 * Device state of a workspace: per k the 2 nrhs contiguous doubles
 * {rz[k][0:nrhs], rr[k][0:nrhs]} (one all-reduce of 2 nrhs doubles) and
 * pAp[k][0:nrhs]; done[c], kstop[c], all_done as for cg_block, the state words
 * of SPMV_HIP_CGB_STATE_WORDS; two partial arrays [dot_partials_len][nrhs]
 * (p.Ap then r.z; r.r), added in index order per column.
 *   init         : R = B ; X = 0 ; partials of r.r (B: any alignment)
 *   dot_pAp      : partials of p.Ap
 *   dot_rz       : partials of r.z ; dinv == NULL: Z as the sweeps left it;
 *                  else Z = dinv * R first (dinv: num_rows doubles, row i's
 *                  for all its columns, any alignment), in the same pass
 *   reduce_pAp   : partials -> pAp[k] ; raises done[c] and all_done (k >= 1)
 *   reduce_rz_rr : partials -> {rz[k], rr[k]} (k >= 0)
 *   update_r     : r -= alpha_c Ap, alpha_c = rz[k-1][c] / pAp[k][c] ;
 *                  partials of r.r
 *   update_xp    : x += alpha_c p ; stop test sqrt(rr[k][c]) / sqrt(rr[0][c]) <
 *                  rtol ; p = beta_c p + z, beta_c = rz[k][c] / rz[k-1][c]
 * nrhs = 2, 4, 8 stream 16-byte elements (every block 16-byte aligned, except
 * B of init); k outside its range is SPMV_HIP_EINVAL. */
int spmv_hip_mcgs_apply_block_f64(spmv_hip_ctx* ctx,
                                  const spmv_hip_mcgs_plan* plan,
                                  spmv_hip_pcgb_ws* ws, const double* R,
                                  double* Z, int nrhs, void* stream);
int spmv_hip_pcgb_ws_create(spmv_hip_ctx* ctx, int kmax, int nrhs,
                            spmv_hip_pcgb_ws** ws);
int spmv_hip_pcgb_ws_destroy(spmv_hip_pcgb_ws* ws);
int spmv_hip_pcgb_ws_reset(spmv_hip_pcgb_ws* ws, double rtol, void* stream);
int spmv_hip_pcgb_ws_capacity(const spmv_hip_pcgb_ws* ws, int* kmax, int* nrhs);
/* device addresses of the scalars of iteration k (for the all-reduces): the
 * 2 nrhs doubles {rz[k], rr[k]}, the nrhs doubles pAp[k] */
int spmv_hip_pcgb_ws_rz_rr(spmv_hip_pcgb_ws* ws, int k, double** slot);
int spmv_hip_pcgb_ws_pAp(spmv_hip_pcgb_ws* ws, int k, double** slot);
/* copies the state words and {rz, rr}[0..kmax] (2 (kmax + 1) nrhs doubles of
 * the workspace's capacity) to the host, async on stream; a short destination
 * is SPMV_HIP_EINVAL and nothing is copied; either may be NULL. */
int spmv_hip_pcgb_ws_read_async(spmv_hip_pcgb_ws* ws, int32_t* host_state,
                                size_t host_state_len, double* host_rz_rr,
                                size_t host_rz_rr_len, void* stream);
int spmv_hip_pcgb_init_f64(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int64_t M,
                           const double* B, double* R, double* X, void* stream);
int spmv_hip_pcgb_dot_pAp_f64(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int64_t M,
                              const double* P, const double* AP, void* stream);
int spmv_hip_pcgb_dot_rz_f64(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int64_t M,
                             const double* dinv, const double* R, double* Z,
                             void* stream);
int spmv_hip_pcgb_reduce_pAp(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int k,
                             void* stream);
int spmv_hip_pcgb_reduce_rz_rr(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int k,
                               void* stream);
int spmv_hip_pcgb_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int k,
                               int64_t M, const double* AP, double* R,
                               void* stream);
int spmv_hip_pcgb_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_pcgb_ws* ws, int k,
                                int64_t M, const double* Z, double* X,
                                double* P, void* stream);

/* ---- Multicolour ILU(0) factored on the device (spmv::Ilu0Preconditioner) ---------
 * M = (D~ + L~) D~^-1 (D~ + U~) on the local diagonal block in the colour-major
 * ordering, fp64, every product, difference and quotient a rounding of its own.
 * before(i) / after(i) as above but ascending by the POSITION of the column;
 * rows in position order, rows of one colour never read each other:
 *   w = row i;  for k in before(i), ascending pos(k):
 *                 m = w[k] * dinv~[k]
 *                 for (j, u) in after~(k), in its order:
 *                   if j == i or j in the pattern of row i: w[j] = w[j] - m * u
 *   l~(i, .) = w on before(i); u~(i, .) = w on after(i); d~_i = w[i];
 *   dinv~_i = 1.0 / d~_i
 * Fill outside the pattern is dropped.  The application is mcgs_apply on the
 * inner plan (ilu0_mcgs_plan), whose values and dinv ilu0_factor writes.
 *
 * The plan is an upload of arrays the HOST built (host/ilu0_build.h): `mcgs`, the
 * sliced layout with the columns in position order (its values and dinv are
 * placeholders), and per part, in CSR over positions: ptr (num_rows + 1), cpos
 * (the column's position, strictly ascending in a row, of a smaller / larger
 * colour), src (index of the entry's value in the matrix's value array, below
 * num_values) and slot (>= 0: index into the part's sliced val; < 0: index ~slot
 * into its long_val).  plan_create checks every index a kernel will use
 * (SPMV_HIP_EINVAL) and copies.
 *
 * ilu0_factor: `values` the matrix's value array (num_values doubles), `diagonal`
 * the diagonal by ROW (num_rows doubles), both on the device; gather, one launch
 * per colour 1 .. C-1, finish; nothing waits.  It may be called again with other
 * values (the same pattern).  ilu0_pivots waits for the stream and returns how
 * many pivots d~ are not finite or zero, and how many are finite and negative.
 * ilu0_get_factor (waits): l~ and u~ in part-CSR order and d~ by position;
 * ilu0_get_pattern: the parts' ptr and cpos.  NULL outputs are skipped. */
typedef struct spmv_hip_ilu0_plan spmv_hip_ilu0_plan;
typedef struct spmv_hip_ilu0_part {
  const int64_t* ptr;
  const int32_t* cpos;
  const int32_t* src;
  const int64_t* slot;
} spmv_hip_ilu0_part;
typedef struct spmv_hip_ilu0_host {
  spmv_hip_mcgs_host mcgs;
  int64_t num_values;
  spmv_hip_ilu0_part before, after;
} spmv_hip_ilu0_host;
int spmv_hip_ilu0_plan_create(spmv_hip_ctx* ctx, const spmv_hip_ilu0_host* in,
                              spmv_hip_ilu0_plan** plan);
int spmv_hip_ilu0_plan_destroy(spmv_hip_ilu0_plan* plan);
int spmv_hip_ilu0_plan_bytes(const spmv_hip_ilu0_plan* plan, int64_t* bytes);
int spmv_hip_ilu0_mcgs_plan(const spmv_hip_ilu0_plan* plan,
                            spmv_hip_mcgs_plan** inner);
int spmv_hip_ilu0_factor(spmv_hip_ctx* ctx, spmv_hip_ilu0_plan* plan,
                         const double* values, const double* diagonal,
                         void* stream);
int spmv_hip_ilu0_pivots(spmv_hip_ctx* ctx, const spmv_hip_ilu0_plan* plan,
                         int64_t* not_usable, int64_t* negative, void* stream);
int spmv_hip_ilu0_get_pattern(spmv_hip_ctx* ctx, const spmv_hip_ilu0_plan* plan,
                              int64_t* before_ptr, int32_t* before_cpos,
                              int64_t* after_ptr, int32_t* after_cpos);
int spmv_hip_ilu0_get_factor(spmv_hip_ctx* ctx, const spmv_hip_ilu0_plan* plan,
                             double* l, double* u, double* d, void* stream);

/* ---- The symbolic setup of ILU(0) on the device (additive, ABI 5) --------------
 * ilu0_plan_build: the plan ilu0_plan_create would make from the arrays of
 * host/ilu0_build.h's ilu0_symbolic for the same colours -- every array equal --
 * from the block's CSR arrays where they lie, under the input rules of
 * mcgs_plan_build above (device pointers, ghosts ignored, rowptr may be NULL
 * when nnz == 0, the same checks and reason codes in info[1], info[2] the peak
 * bytes of the temporaries, info[3] a row of an improper colouring or of a
 * duplicate).  No value is read: the inner plan's values, padding and dinv are
 * +0.0 until ilu0_factor writes them, and a diagonal that is not positive is
 * the factorisation's to count (ilu0_pivots), not this call's.  The parts
 * ascend by the POSITION of the column.  Two entries of one row with the same
 * column -- in symmetric storage among the row's stored lower entries and the
 * mirror images of its column -- are SPMV_HIP_EINVAL with info[1] =
 * SPMV_HIP_ILU0_DUPLICATE: a factor entry has one source.  src of a mirror
 * image is the index of the stored lower entry.  A failure leaves nothing
 * allocated.  The plan serves ilu0_factor, _pivots, _get_pattern, _get_factor,
 * _mcgs_plan, _plan_bytes and _plan_destroy like one of ilu0_plan_create.
 *
 * ilu0_plan_sizes / _export: the part arrays copied to host buffers, for plans
 * of either builder (the inner plan: mcgs_plan_export on ilu0_mcgs_plan).
 * sizes[SPMV_HIP_ILU0_SIZES_WORDS] = {rows, entries of before, of after, device
 * bytes without the inner plan's}.  export: every pointer may be NULL; ptr rows
 * + 1 (none for 0 rows), cpos / src / slot the part's entries. */
#define SPMV_HIP_ILU0_DUPLICATE 6
#define SPMV_HIP_ILU0_SIZES_WORDS 4
typedef struct spmv_hip_ilu0_export {
  int64_t* ptr;
  int32_t* cpos;
  int32_t* src;
  int64_t* slot;
} spmv_hip_ilu0_export;
int spmv_hip_ilu0_plan_build(spmv_hip_ctx* ctx, int32_t num_rows,
                             int32_t num_cols, int64_t nnz, const int32_t* rowptr,
                             const int32_t* colind, int symmetric,
                             const int32_t* colors, int32_t num_colors,
                             int long_threshold, spmv_hip_ilu0_plan** plan,
                             int64_t* info, void* stream);
int spmv_hip_ilu0_plan_sizes(const spmv_hip_ilu0_plan* plan, int64_t* sizes);
int spmv_hip_ilu0_plan_export(const spmv_hip_ilu0_plan* plan,
                              const spmv_hip_ilu0_export* before,
                              const spmv_hip_ilu0_export* after);

/* ---- fp32 values in the sweep plans (additive, ABI 5) ---------------------------
 * A sweep plan may keep the off-diagonal values of both parts -- the sliced val
 * and the long rows' long_val -- as float: 8 bytes per stored entry (value and
 * column) cross the fabric in a sweep, not 12.  The stored value is the fp64
 * value rounded to nearest-even; dinv, r, z, the sums and every operation stay
 * fp64, and the kernels compute acc = acc + (double)v32 * z[col] in the
 * entries' order: mcgs_apply / mcgs_apply_block on such a plan have the bits of
 * the fp64 sweeps on a plan with the widened values.  Both applications take a
 * plan of either form; their argument rules do not change.
 *
 * Range.  A finite non-zero value whose rounding is +-Inf, zero or an fp32
 * subnormal is OUT OF RANGE, so that a plan never depends on a denormal mode:
 * |v| >= 2^128 - 2^103 or 0 < |v| < 2^-126 - 2^-150.  +-0, +-Inf and NaN
 * convert as IEEE says and are in range.  The values are counted on the device
 * as they are rounded.
 *
 * value_bits: 64 (the entry point without _ex, in every respect) or 32;
 * anything else is SPMV_HIP_EINVAL.
 *   mcgs_plan_create_ex / mcgs_plan_build_ex: the plan of mcgs_plan_create /
 *     mcgs_plan_build; with 32 each fp64 value array is then rounded into a
 *     float array by a kernel and freed, one array after the other (peak: the
 *     fp64 plan plus 4 bytes per entry of its largest value array), and the
 *     call waits for the count: *out_of_range != 0 is SPMV_HIP_ERANGE and no
 *     plan (build_ex returns SPMV_HIP_ERANGE with *out_of_range == 0 for the
 *     size limit of mcgs_plan_build).
 *   ilu0_plan_create_ex / ilu0_plan_build_ex: the inner plan keeps floats;
 *     ilu0_factor factors in fp64 as ever (the working copy, ilu0_get_factor
 *     and the pivot counts do not change) and rounds l~ and u~ as it scatters
 *     them into the inner plan, dinv~ stays fp64; every ilu0_factor rounds
 *     again.  ilu0_counts is ilu0_pivots with a third count from the same
 *     wait: the values of the last factorisation out of fp32's range (0 for an
 *     fp64 plan) -- a plan with such a count must not be applied.
 *   mcgs_plan_value_bits: 64 or 32.
 *   mcgs_plan_bytes of an fp32 plan = that of the fp64 plan of the same input
 *     - 4 * (sizes[3] + sizes[5] + sizes[6] + sizes[8]) of mcgs_plan_sizes: the
 *     sliced entries (padding included) and the long entries of both parts.
 *   mcgs_plan_export of an fp32 plan returns val / long_val WIDENED to double,
 *     entry for entry what the kernels multiply with. */
int spmv_hip_mcgs_plan_create_ex(spmv_hip_ctx* ctx, const spmv_hip_mcgs_host* in,
                                 int value_bits, spmv_hip_mcgs_plan** plan,
                                 int64_t* out_of_range);
int spmv_hip_mcgs_plan_build_ex(spmv_hip_ctx* ctx, int32_t num_rows,
                                int32_t num_cols, int64_t nnz,
                                const int32_t* rowptr, const int32_t* colind,
                                const double* values, const double* diagonal,
                                int symmetric, const int32_t* colors,
                                int32_t num_colors, int long_threshold,
                                int value_bits, spmv_hip_mcgs_plan** plan,
                                int64_t* info, int64_t* out_of_range,
                                void* stream);
int spmv_hip_mcgs_plan_value_bits(const spmv_hip_mcgs_plan* plan, int* bits);
int spmv_hip_ilu0_plan_create_ex(spmv_hip_ctx* ctx, const spmv_hip_ilu0_host* in,
                                 int value_bits, spmv_hip_ilu0_plan** plan);
int spmv_hip_ilu0_plan_build_ex(spmv_hip_ctx* ctx, int32_t num_rows,
                                int32_t num_cols, int64_t nnz,
                                const int32_t* rowptr, const int32_t* colind,
                                int symmetric, const int32_t* colors,
                                int32_t num_colors, int long_threshold,
                                int value_bits, spmv_hip_ilu0_plan** plan,
                                int64_t* info, void* stream);
int spmv_hip_ilu0_counts(spmv_hip_ctx* ctx, const spmv_hip_ilu0_plan* plan,
                         int64_t* not_usable, int64_t* negative,
                         int64_t* out_of_range, void* stream);

/* ---- Aggregation multigrid (spmv::AmgPreconditioner) ---------------------------
 * The device half of one coarsening step of a plain aggregation multigrid
 * hierarchy, fp64, every product, sum, difference and quotient a rounding of
 * its own.  The host describes the step (HOST arrays):
 *   agg[i]       the aggregate of fine row i, 0 <= agg[i] < coarse_rows
 *   member_ptr / member   the rows of every aggregate, ascending
 *   src_ptr / src         per entry E of the coarse operator P^T A P (P the
 *                piecewise-constant prolongation) the fine entries it adds, in
 *                the order they are added: src >= 0 is values[src] (below
 *                num_values), src < 0 is diagonal[~src] (below num_diagonal,
 *                which is 0 or fine_rows: symmetric storage keeps its diagonal
 *                in an array)
 *   xrow_ptr / xrow_src   optional (symmetric storage): the expanded rows of
 *                the fine level as source lists, for amg_diag
 * coarse_rows == 0 describes no step (the lists of the step are not read).
 * plan_create checks every index a kernel will use -- agg in range, the member
 * lists a partition of the rows, ascending and consistent with agg, src_ptr
 * strictly monotone from 0, every src in range -- and returns SPMV_HIP_EINVAL
 * otherwise.
 *
 *   galerkin  coarse_values[E] = v_0 + v_1 + ... over the list of E, left to
 *             right from the first one: one lane per coarse entry
 *   diag      per fine row i: d[i] = the sum of the row's entries on column i
 *             in storage order from 0.0 (entries with a column >= ncols_local
 *             are not part of the level), with a plan that has xrow lists
 *             diagonal[i]; dinv[i] = 1.0 / d[i]; g_i = (|a_0| + |a_1| + ...) *
 *             dinv[i] over the expanded row.  stat (a DEVICE array of
 *             SPMV_HIP_AMG_STAT_WORDS 8-byte words, overwritten): word 0 = the
 *             number of d that are not finite or not > 0, the other words = the
 *             bit patterns of the workgroups' maxima of g (>= 0.0); the row-sum
 *             bound of dinv*A is the maximum over them.  A g that is NaN never
 *             replaces a number; the maximum may be +Inf (dinv of a subnormal
 *             d, a sum that overflows), which word 0 does not count: the
 *             caller refuses a bound that is not finite and > 0.
 *   restrict  rc[I] = (t_0 + t_1) + ..., t_m = r[i_m] - w[i_m] over the members
 *             of I ascending: one lane per aggregate
 *   prolong   z[i] = z[i] + scale * e[agg[i]]            (z 16-byte aligned)
 *   post0     d = b0 * (dinv * (r - w)) ; z = z + d: step 0 of a Chebyshev
 *             iteration continued from the current z (steps >= 1: cheb_step).
 *             d == NULL: the only step, d is not written.  16-byte aligned.
 * No kernel waits on another workgroup; no floating-point atomics. */
#define SPMV_HIP_AMG_STAT_WORDS 257
typedef struct spmv_hip_amg_plan spmv_hip_amg_plan;
typedef struct spmv_hip_amg_host {
  int32_t fine_rows;
  int32_t coarse_rows;
  int64_t num_values;
  int32_t num_diagonal;
  int64_t coarse_nnz;
  const int32_t* agg;
  const int32_t* member_ptr;
  const int32_t* member;
  const int64_t* src_ptr;
  const int32_t* src;
  const int64_t* xrow_ptr;
  const int32_t* xrow_src;
} spmv_hip_amg_host;
int spmv_hip_amg_plan_create(spmv_hip_ctx* ctx, const spmv_hip_amg_host* in,
                             spmv_hip_amg_plan** plan);
int spmv_hip_amg_plan_destroy(spmv_hip_amg_plan* plan);
int spmv_hip_amg_plan_bytes(const spmv_hip_amg_plan* plan, int64_t* bytes);
int spmv_hip_amg_galerkin_f64(spmv_hip_ctx* ctx, const spmv_hip_amg_plan* plan,
                              const double* values, const double* diagonal,
                              double* coarse_values, void* stream);
int spmv_hip_amg_diag_f64(spmv_hip_ctx* ctx, const spmv_hip_amg_plan* plan,
                          int32_t n, int32_t ncols_local, const int32_t* rowptr,
                          const int32_t* colind, const double* values,
                          const double* diagonal, double* d, double* dinv,
                          uint64_t* stat, void* stream);
int spmv_hip_amg_restrict_f64(spmv_hip_ctx* ctx, const spmv_hip_amg_plan* plan,
                              const double* r, const double* w, double* rc,
                              void* stream);
int spmv_hip_amg_prolong_f64(spmv_hip_ctx* ctx, const spmv_hip_amg_plan* plan,
                             double scale, const double* e, double* z,
                             void* stream);
int spmv_hip_amg_post0_f64(spmv_hip_ctx* ctx, int64_t n, double b0,
                           const double* w, const double* r, const double* dinv,
                           double* d, double* z, void* stream);

/* ---- The symbolic setup of the hierarchy on the device ---------------------------
 * (hip/spmv_amg_build.hip; spmv::AmgOptions::setup = device.)  The block's CSR
 * arrays are DEVICE pointers, as a CSRMatrix holds them: num_rows rows, columns
 * in [0, num_cols), columns >= num_rows are ghosts and ignored; symmetric
 * storage: only the entries with a column < their row count, the diagonal is
 * an array.  rowptr == NULL with nnz == 0: an empty block.  Nothing of the
 * matrix crosses to the host, only counters.  Both entries wait for the device.
 *
 * spmv_hip_amg_aggregate: the aggregates of host/amg_build.h's three passes with
 * "i ascending" read as "i in descending priority" -- order
 * SPMV_HIP_MCGS_NATURAL: prio(i) = num_rows - i (row order; positive, since 0
 * stands for "no bid"), amg_aggregate's result entry for entry;
 * SPMV_HIP_MCGS_HASHED: the hash of spmv_hip_mcgs_color.  agg: num_rows ints on
 * the device; *n_agg the number of aggregates; rounds[2]: the rounds of pass 1
 * and of pass 3 (they depend on the matrix and the order alone).  `diagonal` is
 * accepted for symmetry with the block's arrays and not read (the diagonal
 * entry is nobody's neighbour).  theta outside [0, 1]: SPMV_HIP_EINVAL.
 * SPMV_HIP_ERANGE: num_rows + 1 rounds of a pass did not suffice (a fault of
 * the library, not of the input).
 *
 * spmv_hip_amg_plan_build: from an aggregate per row (a DEVICE array, the
 * caller's own or spmv_hip_amg_aggregate's; every aggregate of [0, n_agg) must
 * have a member) the plan spmv_hip_amg_plan_create makes from amg_coarsen's
 * lists for the same aggregates, array for array, with the same plan_bytes;
 * symmetric storage adds the xrow lists.  The coarse pattern: coarse_rowptr,
 * n_agg + 1 ints the caller has allocated on the device; *coarse_colind, a
 * device array of *coarse_nnz ints that becomes the caller's (spmv_hip_free;
 * NULL for none).  n_agg == 0 describes no step: symmetric storage still gets
 * its xrow lists.  Values are not read.
 *
 * Both check their input on the device before anything is indexed;
 * SPMV_HIP_EINVAL with info[0] = the reason, nothing is left allocated.
 * info (SPMV_HIP_AMG_INFO_WORDS): [0] reason, [1] the peak of the temporaries
 * in bytes, [2] the number of expanded entries (plan_build).
 *
 * spmv_hip_amg_plan_sizes / _export: a plan of either builder copied out (host
 * arrays, NULL skipped).  sizes (SPMV_HIP_AMG_SIZES_WORDS): fine_rows,
 * coarse_rows, num_values, num_diagonal, coarse_nnz, the length of src, whether
 * xrow lists exist, the length of xrow_src, plan_bytes.  Lengths: agg, member
 * fine_rows; member_ptr coarse_rows + 1; src_ptr coarse_nnz + 1; xrow_ptr
 * fine_rows + 1; a plan without a step has none of the first five. */
#define SPMV_HIP_AMG_INFO_WORDS 4
#define SPMV_HIP_AMG_SIZES_WORDS 9
#define SPMV_HIP_AMG_BAD_ROWPTR 1
#define SPMV_HIP_AMG_BAD_COLUMN 2
#define SPMV_HIP_AMG_BAD_AGG 3
#define SPMV_HIP_AMG_EMPTY_AGG 4
typedef struct spmv_hip_amg_export {
  int32_t* agg;
  int32_t* member_ptr;
  int32_t* member;
  int64_t* src_ptr;
  int32_t* src;
  int64_t* xrow_ptr;
  int32_t* xrow_src;
} spmv_hip_amg_export;
int spmv_hip_amg_aggregate(spmv_hip_ctx* ctx, int32_t num_rows, int32_t num_cols,
                           int64_t nnz, const int32_t* rowptr,
                           const int32_t* colind, const double* values,
                           const double* diagonal, int symmetric, double theta,
                           int order, int32_t* agg, int32_t* n_agg, int* rounds,
                           int64_t* info, void* stream);
int spmv_hip_amg_plan_build(spmv_hip_ctx* ctx, int32_t num_rows, int32_t num_cols,
                            int64_t nnz, const int32_t* rowptr,
                            const int32_t* colind, int symmetric,
                            const int32_t* agg, int32_t n_agg,
                            int32_t* coarse_rowptr, int32_t** coarse_colind,
                            int64_t* coarse_nnz, spmv_hip_amg_plan** plan,
                            int64_t* info, void* stream);
int spmv_hip_amg_plan_sizes(const spmv_hip_amg_plan* plan, int64_t* sizes);
int spmv_hip_amg_plan_export(const spmv_hip_amg_plan* plan,
                             const spmv_hip_amg_export* out);

/* ---- The V-cycle's vector kernels for nrhs INTERLEAVED vectors ------------------
 * (spmv::amg_apply_block).  Element (i, c) of a block at V[i * nrhs + c], 1 <=
 * nrhs <= SPMV_HIP_CGB_MAX_NRHS (anything else: SPMV_HIP_EINVAL); blocks of n *
 * nrhs doubles (restrict / prolong: the plan's fine_rows or coarse_rows times
 * nrhs); dinv (n doubles), agg and the member lists are shared by the columns.
 * Column c of every result has the bits of the single-vector entry point above
 * on column c, whatever the other columns hold.
 *   cheb_apply0_block  d = b0 * (dinv*r) ; z = d.  d == NULL: the only step.
 *   cheb_step_block    d = a*d + b*(dinv*(r - w)) ; z = z + d.  last != 0: d is
 *                      read, not written.  (No workspace form: no dot product.)
 *   amg_post0_block    d = b0 * (dinv*(r - w)) ; z = z + d.  d == NULL: the only
 *                      step.
 *   amg_restrict_block rc(I, c) = (t_0 + t_1) + ... over the members of I
 *                      ascending, t_m = r(i_m, c) - w(i_m, c)
 *   amg_prolong_block  z(i, c) = z(i, c) + scale * e(agg[i], c)
 * dinv is required.  Any alignment: nrhs = 2, 4, 8 with every block pointer
 * 16-byte aligned run the streaming form (16-byte accesses, non-temporal from
 * the context's blas1_nt_min_elems doubles per block on), everything else one
 * thread per row with scalar accesses -- the same bits.  n == 0 launches
 * nothing. */
int spmv_hip_cheb_apply0_block_f64(spmv_hip_ctx* ctx, int64_t n, int nrhs,
                                   double b0, const double* r, const double* dinv,
                                   double* d, double* z, void* stream);
int spmv_hip_cheb_step_block_f64(spmv_hip_ctx* ctx, int64_t n, int nrhs, double a,
                                 double b, int last, const double* w,
                                 const double* r, const double* dinv, double* d,
                                 double* z, void* stream);
int spmv_hip_amg_post0_block_f64(spmv_hip_ctx* ctx, int64_t n, int nrhs, double b0,
                                 const double* w, const double* r,
                                 const double* dinv, double* d, double* z,
                                 void* stream);
int spmv_hip_amg_restrict_block_f64(spmv_hip_ctx* ctx,
                                    const spmv_hip_amg_plan* plan, int nrhs,
                                    const double* r, const double* w, double* rc,
                                    void* stream);
int spmv_hip_amg_prolong_block_f64(spmv_hip_ctx* ctx,
                                   const spmv_hip_amg_plan* plan, int nrhs,
                                   double scale, const double* e, double* z,
                                   void* stream);

/* ---- The fused tail of the AMG V-cycle ------------------------------------------
 * The levels t .. last of one application -- small levels, where a launch costs
 * more than its work -- in ONE launch of one workgroup of 1024 threads: per
 * level the Chebyshev smoother from z = 0, the product and the restrict on the
 * way down, the coarsest level's iteration, then prolong and the continued
 * smoother on the way up.  In: levels[0].r.  Out: levels[0].z.  The arithmetic
 * per element is that of cheb_apply0 / cheb_step / amg_restrict / amg_prolong /
 * amg_post0 (one definition, hip/amg_elem.h), and a level's product w = A z
 * runs in the order `lanes_per_row` names:
 *   0        one lane per row, left to right from 0.0, the product rounded
 *            first (every plan form but the next one gives these bits)
 *   4 .. 64  SPMV_HIP_ALGO_VECTOR's: lane l of the row adds the products l,
 *            l + lanes, ... from 0.0, then lane l += lane l + off for off =
 *            lanes / 2 .. 1 (ask the level's plan: csr_plan_get "algo" and
 *            "lanes_per_row")
 * so the result has the bits of the separate launches.
 * All pointers of a level are DEVICE pointers except a and b (HOST, the
 * level's Chebyshev coefficients: smooth_degree of them below the last level,
 * coarse_degree on it).  rowptr / colind / values: the level's CSR block, square;
 * dinv, r, w, dd, z: rows doubles each, 8-byte aligned; step: the coarsening
 * step to the next level (NULL on the last), whose fine_rows / coarse_rows must
 * be the two levels' rows.  tail_create reads rowptr and colind back and checks
 * every index the kernel will use (the step's lists were checked by
 * spmv_hip_amg_plan_create); SPMV_HIP_EINVAL otherwise, nothing is launched or
 * written.  It waits for the device.  The arrays and steps must outlive the
 * tail.  tail_set_coefficients rewrites one level's a, b in the device table
 * (blocking; not while a run is in flight).  No second workgroup, no
 * floating-point atomics, no scratch. */
#define SPMV_HIP_AMG_TAIL_MAX_LEVELS 16
#define SPMV_HIP_AMG_TAIL_MAX_DEGREE 16
typedef struct spmv_hip_amg_tail spmv_hip_amg_tail;
typedef struct spmv_hip_amg_tail_level {
  int32_t rows;
  int32_t lanes_per_row;
  int64_t nnz;
  const int32_t* rowptr;
  const int32_t* colind;
  const double* values;
  const double* dinv;
  double* r;
  double* w;
  double* dd;
  double* z;
  const spmv_hip_amg_plan* step;
  const double* a;
  const double* b;
} spmv_hip_amg_tail_level;
typedef struct spmv_hip_amg_tail_host {
  int32_t num_levels;
  int32_t smooth_degree;
  int32_t coarse_degree;
  double coarse_scale;
  const spmv_hip_amg_tail_level* levels;
} spmv_hip_amg_tail_host;
int spmv_hip_amg_tail_create(spmv_hip_ctx* ctx, const spmv_hip_amg_tail_host* in,
                             spmv_hip_amg_tail** tail);
int spmv_hip_amg_tail_destroy(spmv_hip_amg_tail* tail);
int spmv_hip_amg_tail_bytes(const spmv_hip_amg_tail* tail, int64_t* bytes);
int spmv_hip_amg_tail_set_coefficients(spmv_hip_amg_tail* tail, int level,
                                       const double* a, const double* b);
int spmv_hip_amg_tail_run_f64(spmv_hip_ctx* ctx, const spmv_hip_amg_tail* tail,
                              void* stream);

/* ---- BiCGStab with an optional diagonal right preconditioner (spmv::bicgstab) ---
 * For nonsymmetric systems.  `dinv` is the inverse of the preconditioner's
 * diagonal or NULL; ph = dinv*p, sh = dinv*s (elementwise), p and s themselves
 * without it.  From x0 = 0, with `.` the global dot product:
 *   r0 = rhat = p1 = b; rho[0] = rr[0] = b.b
 *   k = 1..kmax:  v = A ph;  rv[k] = rhat.v;  rv[k] == 0 -> breakdown 1
 *                 alpha = rho[k-1] / rv[k];  s = r - alpha v
 *                 t = A sh;  ts[k] = t.s;  tt[k] = t.t
 *                 omega = tt[k] == 0 ? 0 : ts[k] / tt[k]
 *                 x += alpha ph;  x += omega sh;  r = s - omega t
 *                 rr[k] = r.r;  rho[k] = rhat.r
 *                 stop when sqrt(rr[k]) / sqrt(rr[0]) < rtol (x, r updated, p not)
 *                 omega == 0 or rho[k] == 0 -> breakdown 2 (x, r, rr[k] valid)
 *                 beta = (rho[k] / rho[k-1]) * (alpha / omega)
 *                 p = r + beta (p - omega v)
 * Products and sums are separate roundings.
 *
 * Device state of a workspace:
 *   rv[k]; the pairs {ts[k], tt[k]} and {rr[k], rho[k]} (k = 0..kmax), each
 *   pair ADJACENT, 16 bytes per k: one all-reduce of 2 doubles on the pair's
 *   address serves both;
 *   done = 1 once the solve has stopped, kstop = the iterations completed,
 *   status = 0 (the tolerance was met, or rr[0] == 0: kstop = 0, x = 0),
 *   1 (breakdown 1: kstop = k - 1, iteration k wrote nothing) or
 *   2 (breakdown 2: kstop = k);
 *   five partial arrays of spmv_hip_dot_partials_len() doubles (rhat.v, t.s,
 *   t.t, r.r, rhat.r).
 * `done` is raised by update_s (breakdown 1, rr[0] == 0) and update_p (the
 * rest); after it every bicg_* kernel returns at once, so the host may enqueue
 * iterations ahead.  An iteration index outside its range (0..kmax for the
 * slots and reduce_rr_rho, 1..kmax elsewhere) is SPMV_HIP_EINVAL. */
int spmv_hip_bicg_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_bicg_ws** ws);
int spmv_hip_bicg_ws_destroy(spmv_hip_bicg_ws* ws);
int spmv_hip_bicg_ws_reset(spmv_hip_bicg_ws* ws, double rtol, void* stream);
/* kmax the workspace was created with: its history holds kmax + 1 pairs */
int spmv_hip_bicg_ws_capacity(const spmv_hip_bicg_ws* ws, int* kmax);
/* device addresses of rv[k] and of the two pairs of k (all-reduce) */
int spmv_hip_bicg_ws_rv(spmv_hip_bicg_ws* ws, int k, double** slot);
int spmv_hip_bicg_ws_ts_tt(spmv_hip_bicg_ws* ws, int k, double** pair);
int spmv_hip_bicg_ws_rr_rho(spmv_hip_bicg_ws* ws, int k, double** pair);
int spmv_hip_bicg_ws_done_flag(spmv_hip_bicg_ws* ws, const int32_t** done);
/* copies {done, kstop, status} (3 x int32) and the pairs {rr[k], rho[k]}, k =
 * 0..kmax, to the host (async on stream).  host_rr_rho_len = doubles
 * `host_rr_rho` can take: fewer than 2 * (kmax + 1) (bicg_ws_capacity) ->
 * SPMV_HIP_EINVAL, nothing is copied.  Either destination may be NULL. */
int spmv_hip_bicg_ws_read_async(spmv_hip_bicg_ws* ws,
                                int32_t* host_done_kstop_status,
                                double* host_rr_rho, size_t host_rr_rho_len,
                                void* stream);
/* start in one pass: r = rhat = p = b ; ph = dinv*b (dinv != NULL) ; x = 0 ;
 * partials of b.b for both halves of the pair (then bicg_reduce_rr_rho(0)
 * installs the pair 0).  b, dinv: any alignment. */
int spmv_hip_bicg_init_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int64_t n,
                           const double* b, const double* dinv, double* r,
                           double* rhat, double* p, double* ph, double* x,
                           void* stream);
/* the two dot-product passes: partials of rhat.v ; of t.s and t.t */
int spmv_hip_bicg_dot_rv_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                             int64_t n, const double* rhat, const double* v,
                             void* stream);
int spmv_hip_bicg_dot_ts_tt_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                                int64_t n, const double* t, const double* s,
                                void* stream);
/* update_s : s = r - alpha v ; sh = dinv*s           (breakdown 1 -> done)
 * update_xr: x += alpha ph ; x += omega sh ; r = s - omega t ; partials of
 *            r.r and rhat.r
 * update_p : stop test, breakdown 2 (-> done) ; p = r + beta (p - omega v) ;
 *            ph = dinv*p
 * Every vector 16-byte aligned.  dinv == NULL (update_s, update_p) and sh ==
 * NULL (update_xr) select the unpreconditioned kernels: no dinv stream, sh /
 * ph are neither read nor written, and update_xr's `ph` is p, its sh is s. */
int spmv_hip_bicg_update_s_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                               int64_t n, const double* r, const double* v,
                               const double* dinv, double* s, double* sh,
                               void* stream);
int spmv_hip_bicg_update_xr_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                                int64_t n, const double* ph, const double* sh,
                                const double* s, const double* t,
                                const double* rhat, double* x, double* r,
                                void* stream);
int spmv_hip_bicg_update_p_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                               int64_t n, const double* r, const double* v,
                               const double* dinv, double* p, double* ph,
                               void* stream);
/* single-workgroup reducers (local part; all-reduce the slot afterwards) */
int spmv_hip_bicg_reduce_rv(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                            void* stream);
int spmv_hip_bicg_reduce_ts_tt(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                               void* stream);
int spmv_hip_bicg_reduce_rr_rho(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws, int k,
                                void* stream);
/* consumer-side forms for ONE rank (see spmv_hip_cg_update_r_cs_f64): every
 * workgroup adds the preceding producer's partials itself, in the reducers'
 * order (the same bits), workgroup 0 stores rv[k] / the pair k.
 *   update_s_cs : reduce_rv + update_s
 *   update_xr_cs: reduce_ts_tt + update_xr
 *   update_p_cs : reduce_rr_rho + update_p */
int spmv_hip_bicg_update_s_cs_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws,
                                  int k, int64_t n, const double* r,
                                  const double* v, const double* dinv,
                                  double* s, double* sh, void* stream);
int spmv_hip_bicg_update_xr_cs_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws,
                                   int k, int64_t n, const double* ph,
                                   const double* sh, const double* s,
                                   const double* t, const double* rhat,
                                   double* x, double* r, void* stream);
int spmv_hip_bicg_update_p_cs_f64(spmv_hip_ctx* ctx, spmv_hip_bicg_ws* ws,
                                  int k, int64_t n, const double* r,
                                  const double* v, const double* dinv,
                                  double* p, double* ph, void* stream);

/* ---- Restarted GMRES with right preconditioning (spmv::gmres) ----------------
 * For nonsymmetric systems; the recurrence is stated in host/cg.h.  The basis
 * is `nvec` vectors of n doubles at V, V + stride, ... (stride even, >= n, V
 * 16-byte aligned); 1 <= nvec <= SPMV_HIP_GMRES_MAX_RESTART.  One inner step
 * at basis size j + 1, w = A M^-1 v_j:
 *   multi_dot(j + 1) ; reduce(H, j + 1) ; [all-reduce of j + 1 at array H]
 *   multi_axpy(first) ; multi_dot(j + 1) ; reduce(C, j + 1) ; [all-reduce at C]
 *   multi_axpy(second: w -= sum c_i v_i ; h_i += c_i ; partials of w.w)
 *   [reduce(WW, 1) ; all-reduce of 1 at WW] ; givens(j, reduced)
 *   scale(w -> v_{j+1})
 * and per cycle: residual ; [reduce(WW, 1) ; all-reduce] ; start ; scale(r ->
 * v_0) ; the inner steps ; solve_y ; combine ; M^-1 ; add.
 *
 * Device state of a workspace: the arrays named below, `done` (raised by
 * givens -- tolerance, k == kmax, hn == 0 (status 1), R_jj == 0 (status 2) --
 * and by start when r.r == 0), kstop, status, k (inner steps completed), jn
 * (columns kept in the current cycle) and `finished`.  After `done`
 * multi_dot, reduce, multi_axpy, givens, scale and start return at once;
 * solve_y, combine and add run until `finished`, which the residual kernel
 * raises when it finds `done`: the cycle that stopped gets its update exactly
 * once however many cycles the host has enqueued behind it. */
#define SPMV_HIP_GMRES_MAX_RESTART 64
#define SPMV_HIP_GMRES_GROUP 8 /* basis vectors per group of the multi kernels */
enum {
  SPMV_HIP_GMRES_H = 0,       /* 64: first-pass, then summed coefficients      */
  SPMV_HIP_GMRES_C = 1,       /* 64: second-pass coefficients                  */
  SPMV_HIP_GMRES_WW = 2,      /* 1: w.w / r.r where a reducer put it           */
  SPMV_HIP_GMRES_CS = 3,      /* 64: rotation cosines                          */
  SPMV_HIP_GMRES_SN = 4,      /* 64: rotation sines                            */
  SPMV_HIP_GMRES_G = 5,       /* 65: the rotated right-hand side               */
  SPMV_HIP_GMRES_Y = 6,       /* 64                                            */
  SPMV_HIP_GMRES_R = 7,       /* 64 x 64: R_il at [l * 64 + i]                 */
  SPMV_HIP_GMRES_HIST = 8,    /* kmax + 1: hist[k]                             */
  SPMV_HIP_GMRES_INV = 9,     /* 1: what scale multiplies by                   */
  SPMV_HIP_GMRES_PART = 10,   /* 64 x dot_partials_len: [i][workgroup]         */
  SPMV_HIP_GMRES_PART_WW = 11 /* dot_partials_len: partials of w.w / r.r       */
};
int spmv_hip_gmres_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_gmres_ws** ws);
int spmv_hip_gmres_ws_destroy(spmv_hip_gmres_ws* ws);
/* kmax <= the capacity, 1 <= restart <= SPMV_HIP_GMRES_MAX_RESTART */
int spmv_hip_gmres_ws_reset(spmv_hip_gmres_ws* ws, double rtol, int kmax,
                            int restart, void* stream);
int spmv_hip_gmres_ws_capacity(const spmv_hip_gmres_ws* ws, int* kmax);
int spmv_hip_gmres_ws_done_flag(spmv_hip_gmres_ws* ws, const int32_t** done);
/* ---- TEST HOOKS, not part of the stable surface: spmv_hip_gmres_ws_array,
 * _ws_set_state and _ws_get_state exist so that a kernel can be launched alone
 * with chosen scalars (tests/test_gpu_gmres_kernels.py).  gmres() uses only
 * ws_array for the three all-reduce addresses H, C and WW.  set_state
 * overwrites done, k, jn and finished: never call it on a workspace of a
 * running solve. */
/* device address (and length, optional) of one of the arrays above */
int spmv_hip_gmres_ws_array(spmv_hip_gmres_ws* ws, int which, double** p,
                            int64_t* count);
/* copies {done, kstop, status, k} (4 x int32) and hist[0..kmax] to the host
 * (async on stream); a host_hist shorter than the capacity + 1 ->
 * SPMV_HIP_EINVAL, nothing is copied.  Either destination may be NULL. */
int spmv_hip_gmres_ws_read_async(spmv_hip_gmres_ws* ws,
                                 int32_t* host_done_kstop_status_k,
                                 double* host_hist, size_t host_hist_len,
                                 void* stream);
/* for driving single kernels: installs k, jn, done (kstop = k) and finished
 * (waits for the stream); reads {done, kstop, status, k, jn, finished} */
int spmv_hip_gmres_ws_set_state(spmv_hip_gmres_ws* ws, int k, int jn, int done,
                                int finished, void* stream);
int spmv_hip_gmres_ws_get_state(spmv_hip_gmres_ws* ws, int32_t* host_words6,
                                void* stream);
/* partials of v_i . w, i = 0..nvec-1, into PART */
int spmv_hip_gmres_multi_dot_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws,
                                 int64_t n, const double* V, int64_t stride,
                                 int nvec, const double* w, void* stream);
/* which = H or C: rows 0..nvec-1 of PART -> that array; WW (nvec = 1): PART_WW
 * -> WW.  One launch, one workgroup per row. */
int spmv_hip_gmres_reduce(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws, int which,
                          int nvec, void* stream);
/* w = w - coef_0 v_0 - ... in that order; second == 0: coef = H; otherwise
 * coef = C, H_i = H_i + C_i and the partials of w.w go to PART_WW */
int spmv_hip_gmres_multi_axpy_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws,
                                  int second, int64_t n, const double* V,
                                  int64_t stride, int nvec, double* w,
                                  void* stream);
/* reduced == 0: adds PART_WW itself; otherwise takes WW */
int spmv_hip_gmres_givens(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws, int j,
                          int reduced, void* stream);
int spmv_hip_gmres_start(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws, int first,
                         int reduced, void* stream);
/* dst = src * INV (dst may be src) */
int spmv_hip_gmres_scale_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws, int64_t n,
                             const double* src, double* dst, void* stream);
int spmv_hip_gmres_solve_y(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws,
                           void* stream);
/* u = Y_0 v_0 ; u = u + Y_i v_i, i = 1..jn-1 (jn == 0: u is not written) */
int spmv_hip_gmres_combine_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws,
                               int64_t n, const double* V, int64_t stride,
                               double* u, void* stream);
/* x = x + z (jn == 0: nothing) */
int spmv_hip_gmres_add_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws, int64_t n,
                           const double* z, double* x, void* stream);
/* r = b - Ax (Ax == NULL: r = b) ; partials of r.r into PART_WW */
int spmv_hip_gmres_residual_f64(spmv_hip_ctx* ctx, spmv_hip_gmres_ws* ws,
                                int64_t n, const double* b, const double* Ax,
                                double* r, void* stream);
/* z = dinv * v (elementwise): the diagonal right preconditioner */
int spmv_hip_gmres_diag_f64(spmv_hip_ctx* ctx, int64_t n, const double* dinv,
                            const double* v, double* z, void* stream);

/* ---- LOBPCG (spmv::lobpcg, host/cg.h) ----------------------------------------
 * Kernels of the block eigensolver on blocks of nev interleaved vectors (element
 * (i, c) at V[i * nev + c], 1 <= nev <= 8); hip/blas1_lobpcg.hip states the
 * arithmetic and the summation orders.  The basis of a step is S = [X, W, P]
 * (blocks = 3) or [X] (blocks = 1: the prologue), AS = [AX, AW, AP].
 *
 * Device state words (spmv_hip_lobpcg_ws_read_async): {done, kstop, status, it,
 * active, has_p, restarts, basis}.  Once `done` is raised every kernel returns
 * at once, except residual / norms called with final != 0 (the epilogue).
 *   gram         one pass over the 2 * blocks blocks -> per-workgroup partials
 *   gram_reduce  partials -> the slot SPMV_HIP_LOBPCG_GRAM (several ranks: the
 *                all-reduce of 2 m m doubles, m = blocks * nev, works on it).
 *                One thread per entry adds the workgroups' partials LEFT TO
 *                RIGHT in index order from 0.0.  This is NOT the order of
 *                sum_partials / spmv_block_sum (thread-strided sums, then the
 *                shuffle tree) that every dot product of the library uses: a
 *                reference written for those does not give these bits.  rr
 *                with reduced == 0 adds the partials in this same order.
 *   rr           one workgroup.  mode 0: Rayleigh-Ritz on (Ga, Gb) -> theta,
 *                the coefficients, the basis mask; mode 1: C = D R^-1 alone.
 *                reduced: read the slot, not the partials.  advance: a step
 *                that succeeds completes an iteration.  A collapsed basis
 *                (twice) raises done with status 1.
 *   update       X' = S C, P' = [W, P] C_wp, and with AX != NULL AX', AP', in
 *                place, one pass
 *   residual     R = AX - X diag(theta); W (may be NULL) = dinv * R, or R when
 *                dinv is NULL; partials of ||r_c||^2
 *   norms        phase 0: partials -> sums -> history, mask, done; phase 1: the
 *                sums alone into SPMV_HIP_LOBPCG_RN; phase 2: the decision from
 *                that slot.  final: sums into the slot's second half, nothing
 *                else. */
enum {
  SPMV_HIP_LOBPCG_HIST = 0,  /* (kmax + 1) * nev                              */
  SPMV_HIP_LOBPCG_THETA = 1, /* nev                                           */
  SPMV_HIP_LOBPCG_COEF = 2,  /* 3 nev * nev, row j = basis column j           */
  SPMV_HIP_LOBPCG_GRAM = 3,  /* 2 * m * m: Gb then Ga, upper triangles        */
  SPMV_HIP_LOBPCG_GPART = 4, /* the Gram kernel's partials, 2 m m per group   */
  SPMV_HIP_LOBPCG_RN = 5,    /* 2 * nev: ||r_c||^2, then the epilogue's       */
  SPMV_HIP_LOBPCG_RPART = 6  /* dot_partials_len * nev                        */
};
#define SPMV_HIP_LOBPCG_STATE_WORDS 8
int spmv_hip_lobpcg_ws_create(spmv_hip_ctx* ctx, int kmax, int nev,
                              spmv_hip_lobpcg_ws** ws);
int spmv_hip_lobpcg_ws_destroy(spmv_hip_lobpcg_ws* ws);
int spmv_hip_lobpcg_ws_reset(spmv_hip_lobpcg_ws* ws, double rtol, double atol,
                             int kmax, int largest, void* stream);
int spmv_hip_lobpcg_ws_capacity(const spmv_hip_lobpcg_ws* ws, int* kmax,
                                int* nev);
int spmv_hip_lobpcg_ws_array(spmv_hip_lobpcg_ws* ws, int which, double** p,
                             int64_t* len);
/* host_hist (may be NULL): at least (capacity kmax + 1) * nev doubles;
 * host_scalars (may be NULL): 3 nev doubles, theta then SPMV_HIP_LOBPCG_RN */
int spmv_hip_lobpcg_ws_read_async(spmv_hip_lobpcg_ws* ws, int32_t* host_state,
                                  double* host_hist, size_t host_hist_len,
                                  double* host_scalars, void* stream);
/* tests: install the words a kernel reads */
int spmv_hip_lobpcg_ws_set_state(spmv_hip_lobpcg_ws* ws, int active, int has_p,
                                 int it, int done, void* stream);
/* workgroups (= partials) of the Gram kernel for M rows */
int spmv_hip_lobpcg_gram_grid(const spmv_hip_lobpcg_ws* ws, int64_t M, int* grid);
int spmv_hip_lobpcg_gram_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                             int64_t M, int blocks, const double* X,
                             const double* W, const double* P, const double* AX,
                             const double* AW, const double* AP, void* stream);
int spmv_hip_lobpcg_gram_reduce(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                                int64_t M, int blocks, void* stream);
int spmv_hip_lobpcg_rr(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws, int64_t M,
                       int blocks, int mode, int reduced, int advance,
                       void* stream);
int spmv_hip_lobpcg_update_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                               int64_t M, int blocks, double* X, const double* W,
                               double* P, double* AX, const double* AW,
                               double* AP, void* stream);
int spmv_hip_lobpcg_residual_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                                 int64_t M, const double* X, const double* AX,
                                 const double* dinv, double* R, double* W,
                                 int final, void* stream);
int spmv_hip_lobpcg_norms(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws, int phase,
                          int final, void* stream);
/* The pencil A x = lambda B x (lobpcg() with B): a third triple BS = [BX, BW,
 * BP] beside S and AS.  gram_reduce, rr, norms and the workspace are the ones
 * above; the state words and `done` are honoured alike.
 *   gram_gen     one pass over the 3 * blocks blocks: Gb = S^T BS, Ga = S^T AS,
 *                entry (i, j), i <= j, the sum over the rows of s_i * (Bs)_j.
 *                Tiles, row groups, summation order and the layout of the
 *                partials are gram's: BX = X, BW = W, BP = P gives gram's bits.
 *   update_gen   update on the three triples, one triple per thread (the grid's
 *                y dimension): X' = S C, P' = [W, P] C_wp, likewise for AS and
 *                BS, in place; each of the nine blocks is read once, each of the
 *                six outputs written once.  AX == NULL skips the second triple
 *                (the prologue's X R^-1, BX R^-1).  Every output has the bits
 *                update gives the same operands.
 *   residual_gen R = AX - BX diag(theta): residual with BX in X's place (the
 *                same kernel; W, the partials and final as there) */
int spmv_hip_lobpcg_gram_gen_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                                 int64_t M, int blocks, const double* X,
                                 const double* W, const double* P,
                                 const double* AX, const double* AW,
                                 const double* AP, const double* BX,
                                 const double* BW, const double* BP,
                                 void* stream);
int spmv_hip_lobpcg_update_gen_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                                   int64_t M, int blocks, double* X,
                                   const double* W, double* P, double* AX,
                                   const double* AW, double* AP, double* BX,
                                   const double* BW, double* BP, void* stream);
int spmv_hip_lobpcg_residual_gen_f64(spmv_hip_ctx* ctx, spmv_hip_lobpcg_ws* ws,
                                     int64_t M, const double* AX,
                                     const double* BX, const double* dinv,
                                     double* R, double* W, int final,
                                     void* stream);

/* ---- Preconditioned MINRES (spmv::minres, host/cg.h) -------------------------
 * Vectors: n doubles, 16-byte aligned.  Every product, sum, difference,
 * quotient and square root is one rounding.  One iteration (the recurrence is
 * spelled out in host/cg.h):
 *   Av = A v with the partials of alfa = v.Av in PART_ALFA (the SpMV's fused dot
 *     or spmv_hip_dot_partial_f64)
 *   [several ranks: reduce(ALFA) ; all-reduce of the slot]
 *   update_r ; [M^-1 and spmv_hip_dot_partial_f64 into PART_RY] ; reduce(RY) ;
 *   [all-reduce of the slot] ; step ; update_xwv(k)
 * and once in front: init ; reduce(RY) ; start ; update_xwv(0).
 * Device state of a workspace: the 16 doubles of SPMV_HIP_MINRES_SCALARS, in
 * this order: rtol, alfa, ry, beta, oldb, dbar, epsln, phibar, cs, sn, bob
 * (= beta / oldb), oldeps, delta, inv_gamma, phi, inv_beta; the words done,
 * kstop, status (0 converged / kmax / running, 1 beta == 0, 2 ry < 0, 3 gamma
 * == 0), k (steps completed), kmax; hist[0..kmax]; two partial arrays of
 * spmv_hip_dot_partials_len() doubles.
 * `done` is raised by start or step; after it init, reduce, update_r, start
 * and step return at once.  update_xwv(k) runs only while the state's k equals
 * its own: the step that stopped with a new iterate still gets its x, once;
 * nothing afterwards writes x, the history or k. */
typedef struct spmv_hip_minres_ws spmv_hip_minres_ws; /* minres() scalars */
enum {
  SPMV_HIP_MINRES_ALFA = 0,      /* 1: v.Av where a reducer (or update_r) put it */
  SPMV_HIP_MINRES_RY = 1,        /* 1: r2.y where the reducer put it             */
  SPMV_HIP_MINRES_HIST = 2,      /* kmax + 1                                     */
  SPMV_HIP_MINRES_PART_ALFA = 3, /* dot_partials_len                             */
  SPMV_HIP_MINRES_PART_RY = 4,   /* dot_partials_len                             */
  SPMV_HIP_MINRES_SCALARS = 5    /* 16: see above (tests read and install them)  */
};
int spmv_hip_minres_ws_create(spmv_hip_ctx* ctx, int kmax,
                              spmv_hip_minres_ws** ws);
int spmv_hip_minres_ws_destroy(spmv_hip_minres_ws* ws);
/* kmax <= the capacity; zeroes the scalars and the history */
int spmv_hip_minres_ws_reset(spmv_hip_minres_ws* ws, double rtol, int kmax,
                             void* stream);
int spmv_hip_minres_ws_capacity(const spmv_hip_minres_ws* ws, int* kmax);
/* device address and length of one array of the state (the slots of ALFA and
 * RY for the all-reduce, the partial arrays for the dot kernels) */
int spmv_hip_minres_ws_array(spmv_hip_minres_ws* ws, int which, double** p,
                             int64_t* count);
/* copies {done, kstop, status} (3 x int32) and hist[0..capacity] to the host
 * (async; either may be NULL; host_hist_len >= capacity + 1 or nothing is
 * enqueued) */
int spmv_hip_minres_ws_read_async(spmv_hip_minres_ws* ws,
                                  int32_t* host_done_kstop_status,
                                  double* host_hist, size_t host_hist_len,
                                  void* stream);
/* TEST HOOKS: install k and done (kstop = k when done; status 0; waits), read
 * {done, kstop, status, k, kmax} */
int spmv_hip_minres_ws_set_state(spmv_hip_minres_ws* ws, int k, int done,
                                 void* stream);
int spmv_hip_minres_ws_get_state(spmv_hip_minres_ws* ws, int32_t* host_words5,
                                 void* stream);
/* y = dinv * r2 ; partials of r2.y into PART_RY (dinv == NULL: the partials of
 * r2.r2, y is not written and may be NULL) */
int spmv_hip_minres_init_f64(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws,
                             int64_t n, const double* r2, const double* dinv,
                             double* y, void* stream);
/* PART_ALFA (+ partials2, the remote block's share, may be NULL) -> ALFA, or
 * PART_RY -> RY (partials2 must be NULL); one workgroup */
int spmv_hip_minres_reduce(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws, int which,
                           const double* partials2, void* stream);
/* one wave: beta1 = sqrt(ry), hist[0], the state in front of the first step;
 * ry < 0: done, status 2; ry == 0: done, status 0 */
int spmv_hip_minres_start(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws,
                          void* stream);
/* t = (Av - bob * r1) - (alfa / beta) * r2, written over r1 (state k == 0: t =
 * Av - (alfa / beta) * r2, r1 is not read).  alfa: the slot (reduced != 0), or
 * PART_ALFA (+ partials2) added by every workgroup in the reducer's order and
 * left in the slot.  dinv != NULL: y = dinv * t.  want_dot: the partials of
 * t.y (dinv == NULL: of t.t) into PART_RY.  r1 must differ from r2 and Av. */
int spmv_hip_minres_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws,
                                 int64_t n, const double* Av, double* r1,
                                 const double* r2, const double* dinv, double* y,
                                 int reduced, const double* partials2,
                                 int want_dot, void* stream);
/* one wave: the scalar part of an iteration from the slots ALFA and RY */
int spmv_hip_minres_step(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws,
                         void* stream);
/* k >= 1, state k == k: w = ((v - oldeps * w1) - delta * w2) * inv_gamma,
 * written over w1 ; x = x + phi * w ; not done: v = y * inv_beta.
 * k == 0, state k == 0, not done: v = y * inv_beta alone (w1, w2, x unused). */
int spmv_hip_minres_update_xwv_f64(spmv_hip_ctx* ctx, spmv_hip_minres_ws* ws,
                                   int k, int64_t n, double* v, double* w1,
                                   const double* w2, double* x, const double* y,
                                   void* stream);

/* ---- LSQR (spmv::lsqr, host/cg.h) ---------------------------------------------
 * Vectors: doubles at any 8-byte aligned address; where every vector of a call
 * is 16-byte aligned the kernels use 16-byte accesses, otherwise pairs of 8-byte
 * ones, with the same bits.  Every product, sum, difference, quotient and
 * square root is one rounding.  ut (m doubles, the row space) and vt (n doubles,
 * the owned part of the column space) are the UN-NORMALISED vectors of the
 * bidiagonalisation, ib = 1 / beta and ia = 1 / alpha their scales.  One
 * iteration (the recurrence is spelled out in host/cg.h):
 *   Av = A vt ; update_u ; [several ranks: reduce(UU) ; all-reduce of the slot]
 *   Atu = A^T ut (+ reverse halo) ; update_v ;
 *   [reduce(VV) ; all-reduce of the slot] ; step ; update_xw(k)
 * and once in front: spmv_hip_dot_partial_f64(ut, ut) into PART_UU ; [reduce(UU)
 * ; all-reduce] ; Atu = A^T ut ; update_v(first) ; [reduce(VV) ; all-reduce] ;
 * start ; update_xw(0).
 * Device state of a workspace: the 15 doubles of SPMV_HIP_LSQR_SCALARS, in this
 * order: rtol, ltol, damp, uu, vv, alpha, beta, phibar, rhobar, anorm2, psi2,
 * ia, ib, t1 (= phi / rho), t2 (= theta / rho); the words done, kstop, status
 * (0 converged / kmax / running, 1 the least-squares test, 2 the
 * bidiagonalisation ended), k (steps completed), kmax; hist_r[0..kmax] and
 * hist_ar[0..kmax]; two partial arrays of spmv_hip_dot_partials_len() doubles.
 * `done` is raised by start or step; after it update_u, update_v, reduce, start
 * and step return at once.  update_xw(k) runs only while the state's k equals
 * its own: the step that stopped still gets its x, once; nothing afterwards
 * writes x, w, the histories or k. */
typedef struct spmv_hip_lsqr_ws spmv_hip_lsqr_ws; /* lsqr() scalars */
enum {
  SPMV_HIP_LSQR_UU = 0,      /* 1: ut.ut where a reducer (or update_v) put it     */
  SPMV_HIP_LSQR_VV = 1,      /* 1: vn.vn where a reducer (or start / step) put it */
  SPMV_HIP_LSQR_HIST_R = 2,  /* kmax + 1                                          */
  SPMV_HIP_LSQR_HIST_AR = 3, /* kmax + 1, right behind HIST_R                     */
  SPMV_HIP_LSQR_PART_UU = 4, /* dot_partials_len                                  */
  SPMV_HIP_LSQR_PART_VV = 5, /* dot_partials_len                                  */
  SPMV_HIP_LSQR_SCALARS = 6  /* 15: see above (tests read and install them)       */
};
int spmv_hip_lsqr_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_lsqr_ws** ws);
int spmv_hip_lsqr_ws_destroy(spmv_hip_lsqr_ws* ws);
/* kmax <= the capacity; zeroes the scalars and both histories */
int spmv_hip_lsqr_ws_reset(spmv_hip_lsqr_ws* ws, double rtol, double ltol,
                           double damp, int kmax, void* stream);
int spmv_hip_lsqr_ws_capacity(const spmv_hip_lsqr_ws* ws, int* kmax);
/* device address and length of one array of the state */
int spmv_hip_lsqr_ws_array(spmv_hip_lsqr_ws* ws, int which, double** p,
                           int64_t* count);
/* copies {done, kstop, status} (3 x int32) and hist_r[0..capacity] followed by
 * hist_ar[0..capacity] to the host (async; either may be NULL; host_hist_len >=
 * 2 * (capacity + 1) or nothing is enqueued) */
int spmv_hip_lsqr_ws_read_async(spmv_hip_lsqr_ws* ws,
                                int32_t* host_done_kstop_status,
                                double* host_hist, size_t host_hist_len,
                                void* stream);
/* TEST HOOKS: install k and done (kstop = k when done; status 0; waits), read
 * {done, kstop, status, k, kmax} */
int spmv_hip_lsqr_ws_set_state(spmv_hip_lsqr_ws* ws, int k, int done,
                               void* stream);
int spmv_hip_lsqr_ws_get_state(spmv_hip_lsqr_ws* ws, int32_t* host_words5,
                               void* stream);
/* ut = Av * ia - alpha * (ut * ib) in place ; partials of ut.ut into PART_UU */
int spmv_hip_lsqr_update_u_f64(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws,
                               int64_t n, const double* Av, double* ut,
                               void* stream);
/* uu: the slot (reduced != 0), or PART_UU added by every workgroup in the
 * reducer's order and left in the slot.  beta = sqrt(uu).  beta != 0: vn = Atu *
 * (1 / beta) - beta * (vt * ia), written over vt (first != 0: vn = Atu * (1 /
 * beta), vt is not read) ; partials of vn.vn into PART_VV.  beta == 0: vt stays
 * and the partials are zero. */
int spmv_hip_lsqr_update_v_f64(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws,
                               int64_t n, const double* Atu, double* vt,
                               int first, int reduced, void* stream);
/* PART_UU -> UU or PART_VV -> VV; one workgroup */
int spmv_hip_lsqr_reduce(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws, int which,
                         void* stream);
/* one workgroup: vv from the slot (reduced != 0) or from PART_VV in the
 * reducer's order; thread 0: beta = sqrt(uu), hist_r[0] = beta (0: done, status
 * 0), alpha = sqrt(vv), hist_ar[0] = alpha * beta (alpha == 0: done, status 2),
 * the state in front of the first step */
int spmv_hip_lsqr_start(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws, int reduced,
                        void* stream);
/* one workgroup: vv as in start; thread 0: the scalar part of an iteration */
int spmv_hip_lsqr_step(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws, int reduced,
                       void* stream);
/* k >= 1, state k == k: x = x + t1 * w ; not done: w = vt * ia - t2 * w.
 * k == 0, state k == 0, not done: w = vt * ia alone (x unused). */
int spmv_hip_lsqr_update_xw_f64(spmv_hip_ctx* ctx, spmv_hip_lsqr_ws* ws, int k,
                                int64_t n, const double* vt, double* w,
                                double* x, void* stream);

/* ---- multi-shift CG (spmv::cg_shifted, host/cg.h) ------------------------------
 * (A + sigma_s I) x_s = b for s < ns <= SPMV_HIP_CGS_MAX_NS on the Krylov space
 * of the seed A.  Vectors: doubles at any 8-byte aligned address; where every
 * vector of a call is 16-byte aligned (and the column strides are even) the
 * kernels use 16-byte accesses, otherwise pairs of 8-byte ones, with the same
 * bits.  x_s = X + s * ldx and p_s = PS + s * ldp are contiguous vectors.
 * Every product, sum, difference, quotient and square root is one rounding.
 * One iteration (the recurrence is spelled out in host/cg.h):
 *   q = A p with the partials of p.q in PART_PQ (+ a second array: the remote
 *   block's share) ; [several ranks: reduce(PQ) ; all-reduce of the slot] ;
 *   update_r ; [reduce(RRN) ; all-reduce of the slot] ; step ; update_xp(k)
 * and once in front: spmv_hip_dot_partial_f64(r, r) into PART_RRN ;
 * [reduce(RRN) ; all-reduce] ; start.
 * Device state of a workspace: the 48 doubles of SPMV_HIP_CGS_SCALARS, in this
 * order: rtol, pq, rrn, rr, a_old, b_old, bn, hist0, then 8 each of sigma, zeta,
 * rho, cx (= a * rho_n), cp (= bn * rho_n^2); the 32 words of get_words: done,
 * kstop, status (0 converged / kmax / running, 1 p.q was not positive),
 * its[8], k (steps completed), kmax, ns, n_act, n_upd, act[8] (the shifts the
 * next step moves, ascending), upd[8] (the shifts the last step moved: s, or
 * s | 8 where p_s moves too); hist_s[0..kmax] at s * (capacity + 1); two
 * partial arrays of spmv_hip_dot_partials_len() doubles.
 * `done` is raised by start or step; after it update_r, reduce, start and step
 * return at once.  update_xp(k) runs only while the state's k equals its own:
 * the step that stopped still gets its x updates, once; nothing afterwards
 * writes X, PS, p, the histories or k. */
typedef struct spmv_hip_cgs_ws spmv_hip_cgs_ws; /* cg_shifted() scalars */
#define SPMV_HIP_CGS_MAX_NS 8
/* {done, kstop, status, its[8]}: what read_async copies */
#define SPMV_HIP_CGS_STATE_WORDS (3 + SPMV_HIP_CGS_MAX_NS)
#define SPMV_HIP_CGS_WORDS 32
enum {
  SPMV_HIP_CGS_PQ = 0,       /* 1: p.q where a reducer (or update_r) put it    */
  SPMV_HIP_CGS_RRN = 1,      /* 1: r.r where a reducer (or start / step) put it */
  SPMV_HIP_CGS_HIST = 2,     /* 8 * (capacity + 1)                             */
  SPMV_HIP_CGS_PART_PQ = 3,  /* dot_partials_len                               */
  SPMV_HIP_CGS_PART_RRN = 4, /* dot_partials_len                               */
  SPMV_HIP_CGS_SCALARS = 5   /* 48: see above (tests read and install them)    */
};
int spmv_hip_cgs_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_cgs_ws** ws);
int spmv_hip_cgs_ws_destroy(spmv_hip_cgs_ws* ws);
/* kmax <= the capacity, 1 <= ns <= 8, host_shifts: ns doubles on the host
 * (copied before the call returns); the state in front of start: zeta = rho =
 * 1, a_old = 1, b_old = 0, every shift active; zeroes the histories */
int spmv_hip_cgs_ws_reset(spmv_hip_cgs_ws* ws, double rtol, int kmax, int ns,
                          const double* host_shifts, void* stream);
int spmv_hip_cgs_ws_capacity(const spmv_hip_cgs_ws* ws, int* kmax);
/* device address and length of one array of the state */
int spmv_hip_cgs_ws_array(spmv_hip_cgs_ws* ws, int which, double** p,
                          int64_t* count);
/* copies the SPMV_HIP_CGS_STATE_WORDS words and the histories to the host
 * (async; either may be NULL; host_hist_len >= 8 * (capacity + 1) or nothing
 * is enqueued) */
int spmv_hip_cgs_ws_read_async(spmv_hip_cgs_ws* ws, int32_t* host_state,
                               double* host_hist, size_t host_hist_len,
                               void* stream);
/* TEST HOOKS: install / read the SPMV_HIP_CGS_WORDS words (set waits; ns must
 * be the reset's, the list entries below it, k <= kmax <= the capacity) */
int spmv_hip_cgs_ws_set_words(spmv_hip_cgs_ws* ws, const int32_t* host_words,
                              void* stream);
int spmv_hip_cgs_ws_get_words(spmv_hip_cgs_ws* ws, int32_t* host_words,
                              void* stream);
/* pq: the slot (reduced != 0), or PART_PQ (+ pq_partials2, may be NULL) added
 * by every workgroup in the reducer's order and left in the slot.  pq > 0: a =
 * rr / pq ; r = r - a * q in place ; partials of r.r into PART_RRN.  Otherwise
 * (a NaN too) nothing is written: step ends the solve with status 1. */
int spmv_hip_cgs_update_r_f64(spmv_hip_ctx* ctx, spmv_hip_cgs_ws* ws, int64_t n,
                              const double* q, double* r,
                              const double* pq_partials2, int reduced,
                              void* stream);
/* PART_PQ (+ partials2) -> PQ or PART_RRN -> RRN; one workgroup */
int spmv_hip_cgs_reduce(spmv_hip_ctx* ctx, spmv_hip_cgs_ws* ws, int which,
                        const double* partials2, void* stream);
/* one workgroup: rr from the slot RRN (reduced != 0) or from PART_RRN in the
 * reducer's order; hist_s[0] = sqrt(rr) for s < ns; rr == 0: done, status 0 */
int spmv_hip_cgs_start(spmv_hip_ctx* ctx, spmv_hip_cgs_ws* ws, int reduced,
                       void* stream);
/* one workgroup: rrn as in start; thread 0: the scalar part of an iteration
 * for every shift of act[], upd[] and the next act[] */
int spmv_hip_cgs_step(spmv_hip_ctx* ctx, spmv_hip_cgs_ws* ws, int reduced,
                      void* stream);
/* k >= 1, state k == k: for every entry of upd[]: x_s = x_s + cx_s * p_s and,
 * with bit 3 and not done, p_s = zeta_s * r + cp_s * p_s; not done: p = r + bn
 * * p.  Columns outside upd[] are neither read nor written.  ldx, ldp >= n. */
int spmv_hip_cgs_update_xp_f64(spmv_hip_ctx* ctx, spmv_hip_cgs_ws* ws, int k,
                               int64_t n, const double* r, double* p, double* X,
                               int64_t ldx, double* PS, int64_t ldp,
                               void* stream);

/* ---- IDR(s) (spmv::idrs, host/cg.h) ----------------------------------------------
 * The biortho variant of van Gijzen and Sonneveld (2011), 1 <= s <=
 * SPMV_HIP_IDRS_MAX_S, on SIGN shadow vectors: p_j(i) = +1.0 where bit j of
 *   z = gi + seed*0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15   (uint64, wrapping)
 *   z = (z ^ z>>30) * 0xBF58476D1CE4E5B9 ; z = (z ^ z>>27) * 0x94D049BB133111EB
 *   z ^= z>>31
 * is clear and -1.0 where it is set, gi = row0 + i the GLOBAL row.  P is never
 * stored.  Vectors: doubles at any 8-byte aligned address; where every vector of
 * a call is 16-byte aligned (and ld is even) the kernels use 16-byte accesses,
 * otherwise pairs of 8-byte ones, with the same bits.  g_i = G + i * ld and
 * u_i = U + i * ld are contiguous vectors.  Every product, sum, difference,
 * quotient and square root is one rounding.  Launch sequence (the recurrence is
 * spelled out in host/cg.h; [..]: several ranks only, each followed by one
 * all-reduce of the slots named):
 *   sign_dot(b, with_ww) ; [reduce(HRR): s + 1] ; start
 *   inner step q: prep(q) ; g = A u ; sign_dot(g) ; [reduce(H): s] ; biortho(q)
 *                 ; update(q) ; [reduce(RR): 1] ; step(q)
 *   after q = s - 1: vh ; t = A vh ; omega_dot ; [reduce(OM): 2] ; omega ;
 *                 omega_update ; [reduce(HRR): s + 1] ; step(s)
 * Device state of a workspace: the SPMV_HIP_IDRS_DOUBLES doubles of
 * SPMV_HIP_IDRS_SCALARS, in this order: rtol, kappa, om, rr, hist0, be, f[8],
 * c[8], a[8], red[11], M[64] (M[i][j] at 8 i + j); the 6 words of get_words:
 * done, kstop, status (0 rtol / kmax / running, 1 a zero or non-finite pivot of
 * M, 2 t.t not positive or om zero or non-finite), k, kmax, s; hist[0..kmax];
 * the partial array, 11 rows of spmv_hip_dot_partials_len() doubles: rows 0..7
 * the sign sums, 8 r.r, 9 t.r, 10 t.t.  The reducers' slots `red`: the sign sums
 * at 0..s-1, r.r at [s], t.r and t.t at [9] and [10].
 * `done` is raised by start, step, biortho or omega; every kernel enqueued after
 * it returns at once, so x is exactly the iterate of the recorded k. */
typedef struct spmv_hip_idrs_ws spmv_hip_idrs_ws; /* idrs() scalars */
#define SPMV_HIP_IDRS_MAX_S 8
/* {done, kstop, status, k}: what read_async copies */
#define SPMV_HIP_IDRS_STATE_WORDS 4
#define SPMV_HIP_IDRS_WORDS 6
#define SPMV_HIP_IDRS_DOUBLES 105
#define SPMV_HIP_IDRS_ROWS 11
enum {
  SPMV_HIP_IDRS_RED = 0,    /* 11: the reducers' slots (all-reduced in place) */
  SPMV_HIP_IDRS_HIST = 1,   /* capacity + 1                                   */
  SPMV_HIP_IDRS_PART = 2,   /* 11 * dot_partials_len                          */
  SPMV_HIP_IDRS_SCALARS = 3 /* 105: see above (tests read and install them)   */
};
enum { /* spmv_hip_idrs_reduce: partial rows -> slots */
  SPMV_HIP_IDRS_REDUCE_H = 0,   /* rows 0..s-1 -> red[0..s-1]                  */
  SPMV_HIP_IDRS_REDUCE_RR = 1,  /* row 8 -> red[s]                             */
  SPMV_HIP_IDRS_REDUCE_OM = 2,  /* rows 9, 10 -> red[9], red[10]               */
  SPMV_HIP_IDRS_REDUCE_HRR = 3  /* rows 0..s-1, 8 -> red[0..s]                 */
};
enum { /* spmv_hip_idrs_prep_f64 */
  SPMV_HIP_IDRS_FUSED = 0,   /* out = om*(dinv*v) + c_q u_q + .. ; v = src - c_q
                                g_q - .. stays in registers (dinv may be NULL) */
  SPMV_HIP_IDRS_STORE_V = 1, /* out = v                                        */
  SPMV_HIP_IDRS_FROM_VH = 2, /* out = om*out + c_q u_q + .. (src == out)        */
  SPMV_HIP_IDRS_PLAIN = 3    /* out = dinv*src, or src (q == s)                */
};
int spmv_hip_idrs_ws_create(spmv_hip_ctx* ctx, int kmax, spmv_hip_idrs_ws** ws);
int spmv_hip_idrs_ws_destroy(spmv_hip_idrs_ws* ws);
/* kmax <= the capacity, 1 <= s <= 8; the state in front of start: M = I, om = 1,
 * everything else 0; zeroes the history */
int spmv_hip_idrs_ws_reset(spmv_hip_idrs_ws* ws, double rtol, double kappa,
                           int kmax, int s, uint64_t seed, void* stream);
int spmv_hip_idrs_ws_capacity(const spmv_hip_idrs_ws* ws, int* kmax);
/* device address and length of one array of the state */
int spmv_hip_idrs_ws_array(spmv_hip_idrs_ws* ws, int which, double** p,
                           int64_t* count);
/* copies the SPMV_HIP_IDRS_STATE_WORDS words and the history to the host (async;
 * either may be NULL; host_hist_len >= capacity + 1 or nothing is enqueued) */
int spmv_hip_idrs_ws_read_async(spmv_hip_idrs_ws* ws, int32_t* host_state,
                                double* host_hist, size_t host_hist_len,
                                void* stream);
/* TEST HOOKS: install / read the SPMV_HIP_IDRS_WORDS words (set waits; s must be
 * the reset's, 0 <= k <= kmax <= the capacity) */
int spmv_hip_idrs_ws_set_words(spmv_hip_idrs_ws* ws, const int32_t* host_words,
                               void* stream);
int spmv_hip_idrs_ws_get_words(spmv_hip_idrs_ws* ws, int32_t* host_words,
                               void* stream);
/* rows 0..s-1 of the partials: this rank's share of p_j . w, one hash per row,
 * w read once, each sum in the order of the streaming dot product; with_ww:
 * w.w in row 8 as well.  row0: the global index of w[0]. */
int spmv_hip_idrs_sign_dot_f64(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws,
                               int64_t n, int64_t row0, const double* w,
                               int with_ww, void* stream);
/* see the modes above; c and om are the state's.  ld >= n. */
int spmv_hip_idrs_prep_f64(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int q,
                           int mode, int64_t n, const double* src,
                           const double* G, const double* U, int64_t ld,
                           const double* dinv, double* out, void* stream);
/* g_q = g - a_0 g_0 - .. ; u_q = u - a_0 u_0 - .. ; r = r - be*g_q ; x = x +
 * be*u_q ; partials of r.r in row 8.  Columns other than 0..q are neither read
 * nor written. */
int spmv_hip_idrs_update_f64(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int q,
                             int64_t n, const double* g, const double* u,
                             double* G, double* U, int64_t ld, double* r,
                             double* x, void* stream);
/* partials of t.r (row 9) and t.t (row 10) in one pass */
int spmv_hip_idrs_omega_dot_f64(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws,
                                int64_t n, const double* t, const double* r,
                                void* stream);
/* r = r - om*t ; x = x + om*vh ; partials of r.r (row 8) and of the sign sums
 * of the new r (rows 0..s-1) in the same pass */
int spmv_hip_idrs_omega_update_f64(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws,
                                   int64_t n, int64_t row0, const double* t,
                                   const double* vh, double* r, double* x,
                                   void* stream);
/* one workgroup per row: partial rows -> the slots (SPMV_HIP_IDRS_REDUCE_*) */
int spmv_hip_idrs_reduce(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int which,
                         void* stream);
/* One workgroup; sums from the slots (reduced != 0) or from the partial rows in
 * the reducer's order.  q = -1 (start): f, rr, hist[0]; rr == 0 or kmax == 0:
 * done.  0 <= q < s: rr, k += 1, hist[k], the stop test, f_i -= be*M[i][q] for
 * i > q.  q = s: rr, f, k += 1, hist[k], the stop test.  Each leaves the
 * coefficients c of the step that follows. */
int spmv_hip_idrs_step(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int q,
                       int reduced, void* stream);
int spmv_hip_idrs_start(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int reduced,
                        void* stream); /* step(-1) */
/* one workgroup: a_0..a_{q-1}, column q of M, be = f_q / M[q][q]; a zero or
 * non-finite pivot: done, status 1 */
int spmv_hip_idrs_biortho(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int q,
                          int reduced, void* stream);
/* one workgroup: om from t.r, t.t and rr; status 2 exits */
int spmv_hip_idrs_omega(spmv_hip_ctx* ctx, spmv_hip_idrs_ws* ws, int reduced,
                        void* stream);

/* ---- 3-D Poisson generator (not in the reference)
 * 7-point stencil on an n^3 grid, natural ordering, diag 6, off-diag -1.
 * Generates, directly in device memory, the CSR block of global rows
 * [row_begin,row_end) in the local column numbering create_matrix would
 * produce (Matrix.cpp:295-318): owned columns first, then ghost columns in
 * ascending global order.  `part` selects which entries are kept:
 */
enum {
  SPMV_HIP_PART_ALL = 0,        /* every entry (blocking models, Matrix.cpp:357) */
  SPMV_HIP_PART_LOCAL = 1,      /* owned columns only (Matrix.cpp:350-353)       */
  SPMV_HIP_PART_REMOTE = 2,     /* ghost columns only (Matrix.cpp:354-355)       */
  SPMV_HIP_PART_LOCAL_LOWER = 3 /* owned columns, global_row > global_col
                                   (Matrix.cpp:337-347); diagonal separate       */
};
int spmv_hip_poisson3d_count(spmv_hip_ctx* ctx, int32_t n, int64_t row_begin,
                             int64_t row_end, int part, int32_t* rowptr,
                             int64_t* host_nnz, void* stream);
int spmv_hip_poisson3d_fill_f64(spmv_hip_ctx* ctx, int32_t n,
                                int64_t row_begin, int64_t row_end, int part,
                                const int32_t* rowptr, int32_t* colind,
                                double* values, double* diagonal,
                                void* stream);
/* number of ghost columns below / above the owned range for this row block */
int spmv_hip_poisson3d_ghosts(int32_t n, int64_t row_begin, int64_t row_end,
                              int64_t* ghosts_below, int64_t* ghosts_above);
/* The same matrix on ONE BOX of a 3-D block partition: rows =
 * the box's points (first[], len[] per axis; x fastest) in the rank-major
 * numbering of Matrix::create_poisson3d_boxes; owned columns 0 .. box points,
 * ghost columns behind them = the points one step outside the faces that have
 * a neighbour box, face by face in the order -z -y -x +x +y +z (ascending
 * global id), inside a face in the order of its two in-face coordinates.
 * box_count with rowptr == NULL only reports the number of ghosts. */
int spmv_hip_poisson3d_box_count(spmv_hip_ctx* ctx, int32_t n,
                                 const int32_t first[3], const int32_t len[3],
                                 int part, int32_t* rowptr, int64_t* host_nnz,
                                 int64_t* num_ghosts, void* stream);
int spmv_hip_poisson3d_box_fill_f64(spmv_hip_ctx* ctx, int32_t n,
                                    const int32_t first[3], const int32_t len[3],
                                    int part, const int32_t* rowptr,
                                    int32_t* colind, double* values,
                                    double* diagonal, void* stream);
/* Seeded unstructured test matrix, generated on the device (not in the
 * reference: a synthetic input for measuring the general kernels on a matrix
 * WITHOUT lattice or narrow-band structure).  Square, `per_row` (1..32)
 * entries per row; each entry's column is, with probability far_permille/1000,
 * anywhere, otherwise within `band` columns of the diagonal; columns ascending
 * within a row (repeats possible), values uniform in [-1, 1).  rowptr takes
 * num_rows + 1, colind / values num_rows * per_row entries.  The numpy twin is
 * spmv_amd/poisson.py:unstructured_csr. */
int spmv_hip_unstructured_fill_f64(spmv_hip_ctx* ctx, int64_t num_rows,
                                   int per_row, int64_t band, int far_permille,
                                   uint64_t seed, int32_t* rowptr,
                                   int32_t* colind, double* values,
                                   void* stream);
/* Seeded FEM-like test matrix, generated on the device (not in the reference:
 * a synthetic input with the row-length distribution and column layout of an
 * unstructured 3-D mesh matrix in a bandwidth-reducing order -- what
 * read_petsc_binary_matrix, spmv/read_petsc.cpp:40-228, typically delivers).
 * Square; short rows of min_len..max_len entries (skewed to the short side) in
 * three clusters around row - layer, row, row + layer, each within +-jitter
 * columns; tail_permille / 1000 of the rows are LONG: tail_min..tail_max
 * entries, one per tail_stride columns around the row.  Columns strictly
 * ascending, the diagonal always present (= entries of the row + 1, the other
 * values uniform in [-1, 1)).  fem_count writes the row pointer (num_rows + 1)
 * and reports the entry count (SPMV_HIP_ERANGE beyond int32); fem_fill writes
 * colind / values.  The numpy twin is spmv_amd/poisson.py:fem_like_csr. */
typedef struct spmv_hip_fem_params {
  int64_t num_rows;
  int32_t min_len, max_len;
  int32_t layer, jitter;
  int32_t tail_permille, tail_min, tail_max, tail_stride;
  uint64_t seed;
} spmv_hip_fem_params;
int spmv_hip_fem_count(spmv_hip_ctx* ctx, const spmv_hip_fem_params* params,
                       int32_t* rowptr, int64_t* host_nnz, void* stream);
int spmv_hip_fem_fill_f64(spmv_hip_ctx* ctx, const spmv_hip_fem_params* params,
                          int64_t num_non_zeros, const int32_t* rowptr,
                          int32_t* colind, double* values, void* stream);
/* Symmetric storage from a square general CSR block on the device, by the
 * reference's rule (spmv/Matrix.cpp:337-349: entries below the diagonal stay in
 * the block in their order, entries on the diagonal are summed into the
 * diagonal array, entries above it are dropped: the matrix is taken to be
 * symmetric).  lower_split_count writes the new row pointer (num_rows + 1) and
 * reports its entry count; lower_split_fill writes colind / values / diagonal.
 * (The reference splits on the host, inside create_matrix.) */
int spmv_hip_csr_lower_split_count(spmv_hip_ctx* ctx, int32_t num_rows,
                                   const int32_t* rowptr, const int32_t* colind,
                                   int32_t* lower_rowptr, int64_t* host_nnz,
                                   void* stream);
int spmv_hip_csr_lower_split_fill_f64(spmv_hip_ctx* ctx, int32_t num_rows,
                                      const int32_t* rowptr, const int32_t* colind,
                                      const double* values,
                                      const int32_t* lower_rowptr,
                                      int32_t* lower_colind, double* lower_values,
                                      double* diagonal, void* stream);
/* x_i = exp(-10 (5 (i/N - 1/2))^2), i = i_begin.. (demos/spmv.cpp:63-67) */
int spmv_hip_fill_gaussian_f64(spmv_hip_ctx* ctx, int64_t N, int64_t i_begin,
                               int64_t count, double* x, void* stream);
int spmv_hip_fill_const_f64(spmv_hip_ctx* ctx, int64_t count, double value,
                            double* x, void* stream);

/* ---- one-sided halo: peer stores into a neighbour's window -----------------
 * The reference's onesided_put_* models (MPI_Put into a window,
 * L2GMap.cpp:645-682).  Every rank owns a window = a staging buffer for its
 * ghost tail (stage_bytes, sized for 8-byte elements) + flag words; it is
 * exported as a HIP IPC handle (ranks in other processes) and by address (ranks
 * that are threads of this process).  A rank connects each neighbour once
 * (where its data goes in the neighbour's staging buffer, which slot it has in
 * the neighbour's flags, which segments it sends / receives; offsets and
 * counts in ELEMENTS), then every exchange is one kernel launch on `stream`:
 * signal "my segment is free", wait for the neighbour's, store the send
 * segment into the neighbour's window, raise its data flag, wait for mine, copy
 * the staging buffer into `ghost_tail`.  Waits are bounded (ctx option
 * "put_timeout_ms", 60 s by default): a neighbour that does not answer leaves
 * NaN in its ghost segment, and the context's next synchronisation
 * (spmv_hip_synchronize / stream_synchronize / event_synchronize) as well as
 * every later exchange of the window return SPMV_HIP_EPEER instead of hanging
 * or handing stale ghosts to the SpMV.
 * The window is FINE-GRAINED device memory where the runtime can export that
 * over IPC (put_fine_grained; peers on other devices store into it while the
 * owner's kernel polls); a coarse-grained window only connects peers on the
 * same device (put_connect: SPMV_HIP_ENOTSUP otherwise -- L2GMap then keeps
 * the two-sided exchange).  Validated on one device only (processes sharing a
 * GPU through IPC, and threads); see spmv_amd/csrc/hip/put.hip. */
#define SPMV_HIP_IPC_HANDLE_BYTES 64
#define SPMV_HIP_PUT_MAX_PEERS 16
typedef struct spmv_hip_put spmv_hip_put;
int spmv_hip_put_create(spmv_hip_ctx* ctx, size_t stage_bytes,
                        spmv_hip_put** put, void* ipc_handle,
                        uint64_t* raw_address, int64_t* process_id);
int spmv_hip_put_connect(spmv_hip_put* put, int k, const void* peer_ipc_handle,
                         uint64_t peer_raw_address, int64_t peer_process_id,
                         size_t peer_stage_bytes, int32_t dst_offset,
                         int32_t slot_at_peer, int32_t send_offset,
                         int32_t send_count, int32_t recv_offset,
                         int32_t recv_count, int peer_fine_grained);
int spmv_hip_put_fine_grained(const spmv_hip_put* put, int* fine_grained);
/* labels for the diagnosis below: my rank, and the rank behind neighbour slot
 * k (k = -1: my rank only) */
int spmv_hip_put_label(spmv_hip_put* put, int my_rank, int k, int peer_rank);
int spmv_hip_put_finish(spmv_hip_put* put);
int spmv_hip_put_exchange(spmv_hip_ctx* ctx, spmv_hip_put* put, size_t elem_bytes,
                          const void* send_buf, void* ghost_tail, void* stream);
int spmv_hip_put_status(const spmv_hip_put* put, int* failed);
int spmv_hip_put_destroy(spmv_hip_put* put);

/* After SPMV_HIP_EPEER: WHICH bounded wait gave up (ABI 5).  The first waiter
 * that times out -- a put kernel at its FREE or DATA flag, a reduction kernel
 * at a peer's slot -- records which wait it was, on which neighbour slot / rank,
 * the epoch it saw there and the epoch it wanted; this formats that record of
 * the context's first failed window into `buf` (empty string: none failed). */
int spmv_hip_peer_error_detail(const spmv_hip_ctx* ctx, char* buf, size_t len);

/* ---- deterministic peer reduction of the CG scalars -------------------------
 * The two MPI_Allreduce of cg() (cg.cpp:65,75; and :49) move ONE double each.
 * Instead of a ring all-reduce (two RCCL launches per iteration, a summation
 * order that is RCCL's business) every rank owns a small window, exported like
 * the put windows above; a reduction is one single-wave kernel per rank on
 * `stream`: store my value(s) and the epoch into my slot of EVERY rank's window
 * (system-scope release), wait for every rank's slot in mine, add the values in
 * RANK ORDER -- the same bits on every rank, run after run -- and write the sum
 * over `inout`.  count <= SPMV_HIP_REDUCE_MAX_COUNT doubles; nranks <=
 * SPMV_HIP_REDUCE_MAX_RANKS.  Slots are double-buffered by the epoch's parity
 * (a rank cannot be two reductions ahead of a peer: the one in between needs
 * that peer's value).  Waits are bounded like the put kernels' ("put_timeout_ms":
 * NaN in `inout`, SPMV_HIP_EPEER at the context's next synchronisation).  Every
 * rank connects every other rank (reduce_connect) before the first reduction.
 * Same memory rules as the put windows; validated on one device only (ranks as
 * threads: 2 / 3 / 8, and the 8-rank 512^3 rehearsal; ranks as processes over
 * IPC handles), with the two-sided halo models -- the pair with the one-sided
 * halo is not validated.  With ranks as THREADS of one process nothing that
 * waits for the whole device (hipMalloc, hipFree) may run between a rank's
 * reduction and its peers': size the CG workspace first. */
#define SPMV_HIP_REDUCE_MAX_RANKS 64
#define SPMV_HIP_REDUCE_MAX_COUNT 4
typedef struct spmv_hip_reduce spmv_hip_reduce;
int spmv_hip_reduce_create(spmv_hip_ctx* ctx, int nranks, int rank,
                           spmv_hip_reduce** reduce, void* ipc_handle,
                           uint64_t* raw_address, int64_t* process_id,
                           int* fine_grained);
int spmv_hip_reduce_connect(spmv_hip_reduce* reduce, int peer_rank,
                            const void* peer_ipc_handle, uint64_t peer_raw_address,
                            int64_t peer_process_id, int peer_fine_grained);
int spmv_hip_reduce_sum_f64(spmv_hip_ctx* ctx, spmv_hip_reduce* reduce,
                            double* inout, int count, void* stream);
int spmv_hip_reduce_destroy(spmv_hip_reduce* reduce);

/* ---- RCCL transport (L2GMap::update p2p models, L2GMap.cpp:564-642;
 *      MPI_Allreduce in cg.cpp:49,65,75) ---------------------------------- */
#define SPMV_HIP_UNIQUE_ID_BYTES 128
int spmv_hip_comm_unique_id(void* host_id_bytes);
int spmv_hip_comm_create(spmv_hip_ctx* ctx, int nranks, int rank,
                         const void* host_id_bytes, spmv_hip_comm** comm);
int spmv_hip_comm_destroy(spmv_hip_comm* comm);
int spmv_hip_comm_rank(const spmv_hip_comm* comm, int* rank, int* nranks);
/* What the transport really is: rank count and rank as RCCL reports them,
 * RCCL's version code, whether the reductions run on a communicator of their
 * own (split off the halo one), and the path of the RCCL library that was
 * loaded.  Any output pointer may be NULL. */
int spmv_hip_comm_info(const spmv_hip_comm* comm, int* nranks, int* rank,
                       int* rccl_version, int* separate_reduction_comm,
                       char* lib_path, int lib_path_len);
/* one grouped exchange: for every neighbour i, send send_counts[i] doubles
 * from send_buf + send_offsets[i] and receive recv_counts[i] doubles into
 * recv_base + recv_offsets[i] (offsets in elements). */
int spmv_hip_comm_neighbor_exchange_f64(spmv_hip_comm* comm, int num_neighbours,
                                        const int32_t* host_neighbours,
                                        const double* send_buf,
                                        const int32_t* host_send_counts,
                                        const int32_t* host_send_offsets,
                                        double* recv_base,
                                        const int32_t* host_recv_counts,
                                        const int32_t* host_recv_offsets,
                                        void* stream);
int spmv_hip_comm_neighbor_exchange_f32(spmv_hip_comm* comm, int num_neighbours,
                                        const int32_t* host_neighbours,
                                        const float* send_buf,
                                        const int32_t* host_send_counts,
                                        const int32_t* host_send_offsets,
                                        float* recv_base,
                                        const int32_t* host_recv_counts,
                                        const int32_t* host_recv_offsets,
                                        void* stream);
int spmv_hip_comm_allreduce_sum_f64(spmv_hip_comm* comm, double* inout,
                                    size_t count, void* stream);
/* byte-wise all-gather of small host-side setup data, staged through device
 * memory (plan construction only; L2GMap.cpp:353-354,387-388) */
int spmv_hip_comm_allgather_host(spmv_hip_comm* comm, const void* host_send,
                                 void* host_recv, size_t bytes_per_rank);

#ifdef __cplusplus
}
#endif
#endif /* SPMV_HIP_H */
