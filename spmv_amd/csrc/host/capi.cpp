// C facade over the host mirror: see include/spmv_host_c.h.
#include "spmv_host_c.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "cg.h"
#include "comm.h"
#include "csr.h"
#include "executor.h"
#include "l2gmap.h"
#include "matrix.h"
#include "read_petsc.h"
#include "amg_build.h"
#include "ilu0_build.h"
#include "sgs_build.h"
#include "spmv_hip.h"
#include "../hip/fp32_range.h"

using namespace spmv;

struct spmvh_exec {
  std::shared_ptr<HostExecutor> host;
  std::shared_ptr<HipExecutor> hip;
};
struct spmvh_comm {
  std::shared_ptr<const Comm> comm;
};
struct spmvh_matrix {
  std::unique_ptr<Matrix<double>> A;
};
struct spmvh_matrix_f32 {
  std::unique_ptr<Matrix<float>> A;
};
struct spmvh_l2g {
  std::unique_ptr<L2GMap> map;
};
struct spmvh_split {
  Matrix<double>::Split s;
};
struct spmvh_petsc_rows {
  PetscRows rows;
};
template <typename W>
struct WorkspaceHandle {
  std::shared_ptr<HipExecutor> exec; // keeps the executor alive
  std::unique_ptr<W> ws;
};
struct spmvh_cg_workspace : WorkspaceHandle<CgWorkspace> {};
struct spmvh_cg_block_workspace : WorkspaceHandle<CgBlockWorkspace> {};
struct spmvh_pcg_workspace : WorkspaceHandle<PcgWorkspace> {};
struct spmvh_chebyshev_workspace : WorkspaceHandle<ChebyshevWorkspace> {};
struct spmvh_bicgstab_workspace : WorkspaceHandle<BicgstabWorkspace> {};
struct spmvh_sgs_workspace : WorkspaceHandle<SgsWorkspace> {};
struct spmvh_pcg_block_workspace : WorkspaceHandle<PcgBlockWorkspace> {};
struct spmvh_gmres_workspace : WorkspaceHandle<GmresWorkspace> {};
struct spmvh_minres_workspace : WorkspaceHandle<MinresWorkspace> {};
struct spmvh_lsqr_workspace : WorkspaceHandle<LsqrWorkspace> {};
struct spmvh_cgs_workspace : WorkspaceHandle<CgShiftedWorkspace> {};
struct spmvh_idrs_workspace : WorkspaceHandle<IdrsWorkspace> {};
struct spmvh_lobpcg_workspace : WorkspaceHandle<LobpcgWorkspace> {};
struct spmvh_sgs_build {
  SgsHostPlan plan;
};
struct spmvh_ilu0_symbolic {
  Ilu0Symbolic sym;
};
struct spmvh_amg_symbolic {
  AmgExpanded x;
  AmgStep step;
};
struct spmvh_amg {
  std::unique_ptr<AmgPreconditioner> M;
};
struct spmvh_sgs {
  std::shared_ptr<HipExecutor> exec; // keeps the executor alive
  std::unique_ptr<SgsPreconditioner> M;
};

namespace
{
thread_local std::string g_last_error;

template <typename F>
int guarded(F&& f)
{
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
  } catch (...) {
    g_last_error = "unknown C++ exception";
  }
  return -1;
}

void require(bool ok, const char* what)
{
  if (!ok)
    throw std::invalid_argument(what);
}

CommunicationModel to_cm(int cm)
{
  require(cm >= 0 && cm <= 7, "unknown CommunicationModel");
  return static_cast<CommunicationModel>(cm);
}

void copy_plan(const L2GMap& m, int32_t* neighbours, int32_t* send_count,
               int32_t* recv_count, int32_t* send_offset, int32_t* recv_offset,
               int32_t* indexbuf)
{
  const size_t nn = m.neighbours().size();
  for (size_t i = 0; i < nn; ++i) {
    neighbours[i] = m.neighbours()[i];
    send_count[i] = m.send_count()[i];
    recv_count[i] = m.recv_count()[i];
  }
  for (size_t i = 0; i <= nn; ++i) {
    send_offset[i] = m.send_offset()[i];
    recv_offset[i] = m.recv_offset()[i];
  }
  std::copy(m.indexbuf().begin(), m.indexbuf().end(), indexbuf);
}

// spmvh_*_workspace_create / _reserve_timing of the five solver workspaces
template <typename W, typename H>
int workspace_create(spmvh_exec* exec, H** ws)
{
  return guarded([&] {
    require(exec && ws, "NULL argument");
    auto w = std::make_unique<H>();
    w->exec = exec->hip;
    w->ws.reset(new W(*exec->hip));
    *ws = w.release();
  });
}

template <typename H>
int workspace_reserve_timing(H* ws, int count)
{
  return guarded([&] {
    require(ws, "NULL argument");
    ws->ws->reserve_timing(count);
  });
}

// what every solver entry point hands back: the history and CgOptions::time_spmv
void copy_out(const std::vector<double>& hist, double* rnorm_history,
              const CgStats& st, double* spmv_ms_total, int* spmv_launches)
{
  if (rnorm_history)
    std::copy(hist.begin(), hist.end(), rnorm_history);
  if (spmv_ms_total)
    *spmv_ms_total = st.spmv_ms_total;
  if (spmv_launches)
    *spmv_launches = st.spmv_launches;
}
} // namespace

extern "C" {

const char* spmvh_last_error(void) { return g_last_error.c_str(); }

// ---- executor -------------------------------------------------------------------
int spmvh_exec_create(int device_id, spmvh_exec** exec)
{
  return guarded([&] {
    require(exec != nullptr, "exec == NULL");
    auto e = std::make_unique<spmvh_exec>();
    e->host = HostExecutor::create();
    e->hip = HipExecutor::create(device_id, e->host);
    *exec = e.release();
  });
}

int spmvh_exec_destroy(spmvh_exec* exec)
{
  return guarded([&] { delete exec; });
}

int spmvh_exec_alloc(spmvh_exec* exec, size_t num_bytes, void** ptr)
{
  return guarded([&] {
    require(exec && ptr, "NULL argument");
    *ptr = exec->hip->alloc<char>(num_bytes);
  });
}

int spmvh_exec_free(spmvh_exec* exec, void* ptr)
{
  return guarded([&] {
    require(exec, "NULL argument");
    exec->hip->free(ptr);
  });
}

int spmvh_exec_memset(spmvh_exec* exec, void* ptr, int value, size_t num_bytes)
{
  return guarded([&] {
    require(exec, "NULL argument");
    exec->hip->memset<char>(static_cast<char*>(ptr), value, num_bytes);
  });
}

int spmvh_exec_copy(spmvh_exec* exec, void* dst, const void* src,
                    size_t num_bytes)
{
  return guarded([&] {
    require(exec, "NULL argument");
    exec->hip->copy<char>(static_cast<char*>(dst),
                          static_cast<const char*>(src), num_bytes);
  });
}

int spmvh_exec_copy_from_host(spmvh_exec* exec, void* dst, const void* host_src,
                              size_t num_bytes)
{
  return guarded([&] {
    require(exec, "NULL argument");
    exec->hip->copy_from<char>(static_cast<char*>(dst), exec->hip->get_host(),
                               static_cast<const char*>(host_src), num_bytes);
  });
}

int spmvh_exec_copy_to_host(spmvh_exec* exec, void* host_dst, const void* src,
                            size_t num_bytes)
{
  return guarded([&] {
    require(exec, "NULL argument");
    exec->hip->copy_to<char>(static_cast<char*>(host_dst),
                             exec->hip->get_host(),
                             static_cast<const char*>(src), num_bytes);
  });
}

int spmvh_exec_synchronize(spmvh_exec* exec)
{
  return guarded([&] {
    require(exec, "NULL argument");
    exec->hip->synchronize();
  });
}

int spmvh_exec_num_cus(spmvh_exec* exec, int* num_cus)
{
  return guarded([&] {
    require(exec && num_cus, "NULL argument");
    *num_cus = exec->hip->get_num_cus();
  });
}

int spmvh_exec_device_type(spmvh_exec* exec, int* type)
{
  return guarded([&] {
    require(exec && type, "NULL argument");
    *type = static_cast<int>(exec->hip->get_device_type());
  });
}

int spmvh_exec_context(spmvh_exec* exec, void** ctx)
{
  return guarded([&] {
    require(exec && ctx, "NULL argument");
    *ctx = exec->hip->context();
  });
}

int spmvh_host_executor_rejects_compute(void)
{
  try {
    std::shared_ptr<DeviceExecutor> host = HostExecutor::create();
    const int32_t rowptr[2] = {0, 1}, colind[1] = {0};
    const double values[1] = {1.0};
    CSRMatrix<double> m(host, 1, 1, 1, rowptr, colind, values);
    (void)m;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return 0;
  }
  return 1;
}

// ---- communicators ----------------------------------------------------------------
int spmvh_comm_self(spmvh_comm** comm)
{
  return guarded([&] {
    require(comm != nullptr, "comm == NULL");
    auto c = std::make_unique<spmvh_comm>();
    c->comm = std::make_shared<SelfComm>();
    *comm = c.release();
  });
}

int spmvh_rccl_unique_id(void* id_bytes)
{
  return guarded([&] {
    require(id_bytes != nullptr, "id_bytes == NULL");
    std::vector<unsigned char> id = RcclComm::unique_id();
    std::memcpy(id_bytes, id.data(), id.size());
  });
}

int spmvh_comm_rccl(spmvh_exec* exec, int nranks, int rank, const void* id_bytes,
                    spmvh_comm** comm)
{
  return guarded([&] {
    require(exec && comm && id_bytes, "NULL argument");
    auto c = std::make_unique<spmvh_comm>();
    c->comm = std::make_shared<RcclComm>(*exec->hip, nranks, rank, id_bytes);
    *comm = c.release();
  });
}

int spmvh_comm_rccl_info(spmvh_comm* comm, int out[4], char* lib_path,
                         int lib_path_len)
{
  return guarded([&] {
    require(comm && out, "NULL argument");
    const auto* rc = dynamic_cast<const RcclComm*>(comm->comm.get());
    require(rc != nullptr, "not an RCCL communicator");
    const RcclComm::Info i = rc->info();
    out[0] = i.nranks;
    out[1] = i.rank;
    out[2] = i.rccl_version;
    out[3] = i.separate_reduction_comm;
    if (lib_path && lib_path_len > 0) {
      strncpy(lib_path, i.lib_path.c_str(), (size_t)lib_path_len - 1);
      lib_path[lib_path_len - 1] = 0;
    }
  });
}

int spmvh_comm_callback(int rank, int nranks, spmvh_allgather_fn allgather,
                        spmvh_exchange_fn exchange, spmvh_allreduce_fn allreduce,
                        void* user, spmvh_comm** comm)
{
  return guarded([&] {
    require(comm && allgather && nranks >= 1 && rank >= 0 && rank < nranks,
            "bad argument");
    CommCallbacks cb;
    cb.user = user;
    cb.allgather = allgather;
    cb.neighbor_exchange = exchange;
    cb.allreduce_sum = allreduce;
    auto c = std::make_unique<spmvh_comm>();
    c->comm = std::make_shared<CallbackComm>(rank, nranks, cb);
    *comm = c.release();
  });
}

int spmvh_comm_destroy(spmvh_comm* comm)
{
  return guarded([&] {
    if (comm && comm->comm)
      comm->comm->close_peer_reduce(); // (collective; a no-op without it)
    delete comm;
  });
}

int spmvh_comm_enable_peer_reduce(spmvh_comm* comm, spmvh_exec* exec, int* ok)
{
  return guarded([&] {
    require(comm && exec && ok && exec->hip, "NULL argument / not a HipExecutor");
    *ok = comm->comm->enable_peer_reduce(*exec->hip) ? 1 : 0;
  });
}

int spmvh_comm_ranks_share_a_process(spmvh_comm* comm, int* shared)
{
  return guarded([&] {
    require(comm && shared, "NULL argument");
    *shared = comm->comm->ranks_share_a_process() ? 1 : 0;
  });
}

int spmvh_comm_reduce_sum(spmvh_comm* comm, double* device_inout, int count,
                          void* stream)
{
  return guarded([&] {
    require(comm && device_inout && count >= 1, "NULL argument");
    comm->comm->reduce_sum(device_inout, static_cast<size_t>(count), stream);
  });
}

// ---- matrix -------------------------------------------------------------------------
int spmvh_matrix_create(spmvh_comm* comm, spmvh_exec* exec,
                        const int32_t* rowptr, const int32_t* colind,
                        const double* values, int64_t nrows_local,
                        int64_t ncols_local, const int64_t* row_ghosts,
                        int64_t num_row_ghosts, const int64_t* col_ghosts,
                        int64_t num_col_ghosts, int symmetric, int cm,
                        spmvh_matrix** A)
{
  return guarded([&] {
    require(comm && exec && A && rowptr, "NULL argument");
    std::vector<int64_t> rg, cg;
    if (num_row_ghosts > 0)
      rg.assign(row_ghosts, row_ghosts + num_row_ghosts);
    if (num_col_ghosts > 0)
      cg.assign(col_ghosts, col_ghosts + num_col_ghosts);
    auto m = std::make_unique<spmvh_matrix>();
    m->A.reset(Matrix<double>::create_matrix(comm->comm, exec->hip, rowptr,
                                             colind, values, nrows_local,
                                             ncols_local, rg, cg,
                                             symmetric != 0, to_cm(cm)));
    *A = m.release();
  });
}

int spmvh_matrix_create_poisson3d(spmvh_comm* comm, spmvh_exec* exec, int32_t n,
                                  int symmetric, int cm, spmvh_matrix** A)
{
  return guarded([&] {
    require(comm && exec && A, "NULL argument");
    auto m = std::make_unique<spmvh_matrix>();
    m->A.reset(Matrix<double>::create_poisson3d(comm->comm, exec->hip, n,
                                                symmetric != 0, to_cm(cm)));
    *A = m.release();
  });
}

int spmvh_matrix_create_unstructured(spmvh_comm* comm, spmvh_exec* exec,
                                     int64_t nrows, int per_row, int64_t band,
                                     int far_permille, uint64_t seed,
                                     spmvh_matrix** A)
{
  return guarded([&] {
    require(comm && exec && A, "NULL argument");
    auto m = std::make_unique<spmvh_matrix>();
    m->A.reset(Matrix<double>::create_unstructured(
        comm->comm, exec->hip, nrows, per_row, band, far_permille, seed));
    *A = m.release();
  });
}

int spmvh_matrix_create_fem_like(spmvh_comm* comm, spmvh_exec* exec,
                                 const struct spmv_hip_fem_params* params,
                                 spmvh_matrix** A)
{
  return guarded([&] {
    require(comm && exec && A && params, "NULL argument");
    auto m = std::make_unique<spmvh_matrix>();
    m->A.reset(Matrix<double>::create_fem_like(comm->comm, exec->hip, *params));
    *A = m.release();
  });
}

int spmvh_matrix_create_fem_like_sym(spmvh_comm* comm, spmvh_exec* exec,
                                     const struct spmv_hip_fem_params* params,
                                     spmvh_matrix** A)
{
  return guarded([&] {
    require(comm && exec && A && params, "NULL argument");
    auto m = std::make_unique<spmvh_matrix>();
    m->A.reset(
        Matrix<double>::create_fem_like(comm->comm, exec->hip, *params, true));
    *A = m.release();
  });
}

int spmvh_matrix_create_poisson3d_boxes(spmvh_comm* comm, spmvh_exec* exec,
                                        int32_t n, int px, int py, int pz,
                                        int symmetric, int cm, spmvh_matrix** A)
{
  return guarded([&] {
    require(comm && exec && A, "NULL argument");
    auto m = std::make_unique<spmvh_matrix>();
    m->A.reset(Matrix<double>::create_poisson3d_boxes(
        comm->comm, exec->hip, n, px, py, pz, symmetric != 0, to_cm(cm)));
    *A = m.release();
  });
}

int spmvh_poisson3d_box_rows(int32_t n, int px, int py, int pz, int rank,
                             int64_t sizes[7], int32_t* rowptr, int32_t* colind,
                             double* values, int64_t* col_ghosts)
{
  return guarded([&] {
    require(sizes, "NULL argument");
    auto b = Matrix<double>::poisson3d_box_rows(n, px, py, pz, rank);
    sizes[0] = b.rows.rows;
    sizes[1] = b.rows.non_zeros();
    sizes[2] = static_cast<int64_t>(b.col_ghosts.size());
    sizes[3] = b.global_row_offset;
    sizes[4] = b.box[0];
    sizes[5] = b.box[1];
    sizes[6] = b.box[2];
    if (rowptr)
      std::copy(b.rows.rowptr.begin(), b.rows.rowptr.end(), rowptr);
    if (colind)
      std::copy(b.rows.colind.begin(), b.rows.colind.end(), colind);
    if (values)
      std::copy(b.rows.values.begin(), b.rows.values.end(), values);
    if (col_ghosts)
      std::copy(b.col_ghosts.begin(), b.col_ghosts.end(), col_ghosts);
  });
}

int spmvh_matrix_destroy(spmvh_matrix* A)
{
  return guarded([&] { delete A; });
}

int spmvh_matrix_rows(spmvh_matrix* A, int* rows)
{
  return guarded([&] {
    require(A && rows, "NULL argument");
    *rows = A->A->rows();
  });
}

int spmvh_matrix_cols(spmvh_matrix* A, int* cols)
{
  return guarded([&] {
    require(A && cols, "NULL argument");
    *cols = A->A->cols();
  });
}

int spmvh_matrix_non_zeros(spmvh_matrix* A, int64_t* nnz)
{
  return guarded([&] {
    require(A && nnz, "NULL argument");
    *nnz = A->A->non_zeros();
  });
}

int spmvh_matrix_format_size(spmvh_matrix* A, size_t* bytes)
{
  return guarded([&] {
    require(A && bytes, "NULL argument");
    *bytes = A->A->format_size();
  });
}

int spmvh_matrix_symmetric(spmvh_matrix* A, int* symmetric)
{
  return guarded([&] {
    require(A && symmetric, "NULL argument");
    *symmetric = A->A->symmetric() ? 1 : 0;
  });
}

int spmvh_matrix_blocks(spmvh_matrix* A, int64_t out[6])
{
  return guarded([&] {
    require(A && out, "NULL argument");
    for (int i = 0; i < 6; ++i)
      out[i] = 0;
    if (const SubMatrix<double>* l = A->A->local_block()) {
      out[0] = l->rows();
      out[1] = l->cols();
      out[2] = l->non_zeros();
    }
    if (const SubMatrix<double>* r = A->A->remote_block()) {
      out[3] = r->rows();
      out[4] = r->cols();
      out[5] = r->non_zeros();
    }
  });
}

int spmvh_matrix_local_values(spmvh_matrix* A, double** values,
                              double** diagonal)
{
  return guarded([&] {
    require(A && values && diagonal, "NULL argument");
    const auto* blk = dynamic_cast<const CSRMatrix<double>*>(A->A->local_block());
    require(blk != nullptr, "the matrix has no local block");
    if (blk->csr_released())
      throw std::runtime_error(
          "spmvh_matrix_local_values - Error: the CSR arrays of this matrix "
          "were released (release_csr)");
    *values = const_cast<double*>(blk->values());
    *diagonal = const_cast<double*>(blk->diagonal());
  });
}

int spmvh_matrix_plan_values_changed(spmvh_matrix* A)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->plan_values_changed();
  });
}

int spmvh_matrix_plan_get(spmvh_matrix* A, int remote, const char* key,
                          int* value)
{
  return guarded([&] {
    require(A && key && value, "NULL argument");
    const SubMatrix<double>* b
        = remote ? A->A->remote_block() : A->A->local_block();
    const auto* csr = dynamic_cast<const CSRMatrix<double>*>(b);
    *value = csr ? csr->query(key) : 0;
  });
}

int spmvh_matrix_plan_set(spmvh_matrix* A, int remote, const char* key,
                          int value)
{
  return guarded([&] {
    require(A && key, "NULL argument");
    const SubMatrix<double>* b
        = remote ? A->A->remote_block() : A->A->local_block();
    const auto* csr = dynamic_cast<const CSRMatrix<double>*>(b);
    require(csr != nullptr, "no such block");
    csr->tune(key, value);
  });
}

int spmvh_matrix_release_csr(spmvh_matrix* A, int64_t* bytes_freed)
{
  return guarded([&] {
    require(A && bytes_freed, "NULL argument");
    *bytes_freed = 0;
    for (const SubMatrix<double>* b : {A->A->local_block(), A->A->remote_block()})
      if (const auto* csr = dynamic_cast<const CSRMatrix<double>*>(b))
        *bytes_freed += static_cast<int64_t>(csr->release_csr());
  });
}

int spmvh_matrix_enable_mixed(spmvh_matrix* A, int* ok)
{
  return guarded([&] {
    require(A && ok, "NULL argument");
    *ok = A->A->enable_mixed() ? 1 : 0;
  });
}

int spmvh_matrix_use_mixed(spmvh_matrix* A, int on)
{
  return guarded([&] {
    require(A, "NULL argument");
    A->A->use_mixed(on != 0);
  });
}

int spmvh_matrix_update(spmvh_matrix* A, double* x)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->col_map()->update(x);
  });
}

int spmvh_matrix_update_finalise(spmvh_matrix* A, double* x)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->col_map()->update_finalise(x);
  });
}

int spmvh_matrix_mult(spmvh_matrix* A, double* x, double* y)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->mult(x, y);
  });
}

int spmvh_matrix_transpmult(spmvh_matrix* A, double* b, double* y)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->transpmult(b, y);
  });
}

int spmvh_matrix_mult_block(spmvh_matrix* A, double* X, double* Y, int k)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->mult_block(X, Y, k);
  });
}

int spmvh_matrix_update_block(spmvh_matrix* A, double* X, int k)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->col_map()->update_block(X, k);
  });
}

int spmvh_matrix_update_finalise_block(spmvh_matrix* A, double* X, int k)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->col_map()->update_finalise_block(X, k);
  });
}

int spmvh_matrix_enable_transpose(spmvh_matrix* A)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->enable_transpose();
  });
}

int spmvh_split_create(const int32_t* rowptr, const int32_t* colind,
                       const double* values, int64_t nrows_local,
                       int64_t ncols_local, int64_t global_row_offset,
                       int64_t global_col_offset, const int64_t* col_ghosts,
                       int64_t num_col_ghosts, int symmetric, int cm,
                       spmvh_split** split, int64_t sizes[8])
{
  return guarded([&] {
    require(rowptr && split && sizes, "NULL argument");
    std::vector<int64_t> ghosts;
    if (num_col_ghosts > 0)
      ghosts.assign(col_ghosts, col_ghosts + num_col_ghosts);
    auto sp = std::make_unique<spmvh_split>();
    sp->s = Matrix<double>::split_rows(rowptr, colind, values, nrows_local,
                                       ncols_local, global_row_offset,
                                       global_col_offset, ghosts,
                                       symmetric != 0, to_cm(cm));
    const auto& s = sp->s;
    sizes[0] = s.local.rows;
    sizes[1] = s.local.cols;
    sizes[2] = s.local.non_zeros();
    sizes[3] = s.remote.rows;
    sizes[4] = s.remote.cols;
    sizes[5] = s.remote.non_zeros();
    sizes[6] = static_cast<int64_t>(s.col_ghosts.size());
    sizes[7] = s.nnz_full;
    *split = sp.release();
  });
}

int spmvh_matrix_f32_create(spmvh_comm* comm, spmvh_exec* exec,
                            const int32_t* rowptr, const int32_t* colind,
                            const float* values, int64_t nrows_local,
                            int64_t ncols_local, const int64_t* row_ghosts,
                            int64_t num_row_ghosts, const int64_t* col_ghosts,
                            int64_t num_col_ghosts, int symmetric, int cm,
                            spmvh_matrix_f32** A)
{
  return guarded([&] {
    require(comm && exec && A && rowptr, "NULL argument");
    std::vector<int64_t> rg, cg;
    if (num_row_ghosts > 0)
      rg.assign(row_ghosts, row_ghosts + num_row_ghosts);
    if (num_col_ghosts > 0)
      cg.assign(col_ghosts, col_ghosts + num_col_ghosts);
    auto m = std::make_unique<spmvh_matrix_f32>();
    m->A.reset(Matrix<float>::create_matrix(comm->comm, exec->hip, rowptr,
                                            colind, values, nrows_local,
                                            ncols_local, rg, cg, symmetric != 0,
                                            to_cm(cm)));
    *A = m.release();
  });
}

int spmvh_matrix_f32_destroy(spmvh_matrix_f32* A)
{
  return guarded([&] { delete A; });
}

int spmvh_matrix_f32_info(spmvh_matrix_f32* A, int* rows, int64_t* nnz,
                          int32_t* local_size, int32_t* num_ghosts)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    if (rows) *rows = A->A->rows();
    if (nnz) *nnz = A->A->non_zeros();
    if (local_size) *local_size = A->A->col_map()->local_size();
    if (num_ghosts) *num_ghosts = A->A->col_map()->num_ghosts();
  });
}

int spmvh_matrix_f32_update(spmvh_matrix_f32* A, float* x)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->col_map()->update(x);
  });
}

int spmvh_matrix_f32_mult(spmvh_matrix_f32* A, float* x, float* y)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->mult(x, y);
  });
}

int spmvh_matrix_f32_transpmult(spmvh_matrix_f32* A, float* b, float* y)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->transpmult(b, y);
  });
}

int spmvh_matrix_f32_mult_block(spmvh_matrix_f32* A, float* X, float* Y, int k)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->mult_block(X, Y, k);
  });
}

int spmvh_matrix_f32_update_block(spmvh_matrix_f32* A, float* X, int k)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->col_map()->update_block(X, k);
  });
}

int spmvh_matrix_f32_update_finalise_block(spmvh_matrix_f32* A, float* X, int k)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    A->A->col_map()->update_finalise_block(X, k);
  });
}

namespace
{
void fill_split_sizes(const Matrix<double>::Split& s, int64_t sizes[8])
{
  sizes[0] = s.local.rows;
  sizes[1] = s.local.cols;
  sizes[2] = s.local.non_zeros();
  sizes[3] = s.remote.rows;
  sizes[4] = s.remote.cols;
  sizes[5] = s.remote.non_zeros();
  sizes[6] = static_cast<int64_t>(s.col_ghosts.size());
  sizes[7] = s.nnz_full;
}
} // namespace

int spmvh_split_create_dist(spmvh_comm* comm, const int32_t* rowptr,
                            const int32_t* colind, const double* values,
                            int64_t nrows_local, int64_t ncols_local,
                            const int64_t* row_ghosts, int64_t num_row_ghosts,
                            const int64_t* col_ghosts, int64_t num_col_ghosts,
                            int symmetric, int cm, spmvh_split** split,
                            int64_t sizes[8])
{
  return guarded([&] {
    require(comm && rowptr && split && sizes, "NULL argument");
    std::vector<int64_t> rg, cg;
    if (num_row_ghosts > 0)
      rg.assign(row_ghosts, row_ghosts + num_row_ghosts);
    if (num_col_ghosts > 0)
      cg.assign(col_ghosts, col_ghosts + num_col_ghosts);
    auto sp = std::make_unique<spmvh_split>();
    sp->s = Matrix<double>::split_rows_distributed(
        *comm->comm, rowptr, colind, values, nrows_local, ncols_local, rg, cg,
        symmetric != 0, to_cm(cm));
    fill_split_sizes(sp->s, sizes);
    *split = sp.release();
  });
}

int spmvh_split_get(spmvh_split* split, int which, int32_t* rowptr,
                    int32_t* colind, double* values)
{
  return guarded([&] {
    require(split && (which == 0 || which == 1), "bad argument");
    const CsrHost<double>& m = which == 0 ? split->s.local : split->s.remote;
    if (rowptr)
      std::copy(m.rowptr.begin(), m.rowptr.end(), rowptr);
    if (colind)
      std::copy(m.colind.begin(), m.colind.end(), colind);
    if (values)
      std::copy(m.values.begin(), m.values.end(), values);
  });
}

int spmvh_split_extra(spmvh_split* split, double* diagonal, int64_t* ghosts)
{
  return guarded([&] {
    require(split != nullptr, "NULL argument");
    if (diagonal)
      std::copy(split->s.diagonal.begin(), split->s.diagonal.end(), diagonal);
    if (ghosts)
      std::copy(split->s.col_ghosts.begin(), split->s.col_ghosts.end(), ghosts);
  });
}

int spmvh_split_destroy(spmvh_split* split)
{
  return guarded([&] { delete split; });
}

// ---- L2GMap inspection ----------------------------------------------------------------
int spmvh_l2g_sizes(spmvh_matrix* A, int32_t* local_size, int32_t* num_ghosts,
                    int64_t* global_size, int64_t* global_offset,
                    int* overlapping, int* num_neighbours, int* num_indices,
                    int* packs)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    std::shared_ptr<const L2GMap> m = A->A->col_map();
    if (local_size) *local_size = m->local_size();
    if (num_ghosts) *num_ghosts = m->num_ghosts();
    if (global_size) *global_size = m->global_size();
    if (global_offset) *global_offset = m->global_offset();
    if (overlapping) *overlapping = m->overlapping() ? 1 : 0;
    if (num_neighbours) *num_neighbours = static_cast<int>(m->neighbours().size());
    if (num_indices) *num_indices = static_cast<int>(m->indexbuf().size());
    if (packs) *packs = m->packs() ? 1 : 0;
  });
}

int spmvh_l2g_onesided(spmvh_matrix* A, int* onesided)
{
  return guarded([&] {
    require(A && onesided, "NULL argument");
    *onesided = A->A->col_map()->onesided() ? 1 : 0;
  });
}

int spmvh_l2g_ghosts(spmvh_matrix* A, int64_t* ghosts)
{
  return guarded([&] {
    require(A && ghosts, "NULL argument");
    const std::vector<int64_t>& g = A->A->col_map()->ghosts();
    std::copy(g.begin(), g.end(), ghosts);
  });
}

int spmvh_l2g_plan(spmvh_matrix* A, int32_t* neighbours, int32_t* send_count,
                   int32_t* recv_count, int32_t* send_offset,
                   int32_t* recv_offset, int32_t* indexbuf)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    copy_plan(*A->A->col_map(), neighbours, send_count, recv_count, send_offset,
              recv_offset, indexbuf);
  });
}

int spmvh_l2g_global_to_local(spmvh_matrix* A, int64_t global, int32_t* local)
{
  return guarded([&] {
    require(A && local, "NULL argument");
    *local = A->A->col_map()->global_to_local(global);
  });
}

int spmvh_l2g_create(spmvh_comm* comm, spmvh_exec* exec, int use_host_exec,
                     int64_t local_size, const int64_t* ghosts,
                     int64_t num_ghosts, int cm, spmvh_l2g** map)
{
  return guarded([&] {
    require(comm && map && (use_host_exec || exec), "NULL argument");
    std::vector<int64_t> g;
    if (num_ghosts > 0)
      g.assign(ghosts, ghosts + num_ghosts);
    std::shared_ptr<DeviceExecutor> e;
    if (use_host_exec)
      e = HostExecutor::create();
    else
      e = exec->hip;
    auto m = std::make_unique<spmvh_l2g>();
    m->map.reset(new L2GMap(comm->comm, local_size, g, e, to_cm(cm)));
    *map = m.release();
  });
}

int spmvh_l2g_destroy(spmvh_l2g* map)
{
  return guarded([&] { delete map; });
}

int spmvh_l2g_map_sizes(spmvh_l2g* map, int* num_neighbours, int* num_indices,
                        int* packs)
{
  return guarded([&] {
    require(map != nullptr, "NULL argument");
    if (num_neighbours)
      *num_neighbours = static_cast<int>(map->map->neighbours().size());
    if (num_indices)
      *num_indices = static_cast<int>(map->map->indexbuf().size());
    if (packs)
      *packs = map->map->packs() ? 1 : 0;
  });
}

int spmvh_l2g_map_plan(spmvh_l2g* map, int32_t* neighbours, int32_t* send_count,
                       int32_t* recv_count, int32_t* send_offset,
                       int32_t* recv_offset, int32_t* indexbuf)
{
  return guarded([&] {
    require(map != nullptr, "NULL argument");
    copy_plan(*map->map, neighbours, send_count, recv_count, send_offset,
              recv_offset, indexbuf);
  });
}

int spmvh_l2g_map_update(spmvh_l2g* map, double* x)
{
  return guarded([&] {
    require(map != nullptr, "NULL argument");
    map->map->update(x);
  });
}

int spmvh_l2gmap_update_block(spmvh_l2g* map, double* X, int k)
{
  return guarded([&] {
    require(map != nullptr, "NULL argument");
    map->map->update_block(X, k);
  });
}

int spmvh_l2gmap_update_finalise_block(spmvh_l2g* map, double* X, int k)
{
  return guarded([&] {
    require(map != nullptr, "NULL argument");
    map->map->update_finalise_block(X, k);
  });
}

int spmvh_l2g_map_reverse_update(spmvh_l2g* map, double* x)
{
  return guarded([&] {
    require(map != nullptr, "NULL argument");
    map->map->reverse_update(x);
  });
}

int spmvh_l2g_map_reverse_update_f32(spmvh_l2g* map, float* x)
{
  return guarded([&] {
    require(map != nullptr, "NULL argument");
    map->map->reverse_update(x);
  });
}

// ---- cg ---------------------------------------------------------------------------------
int spmvh_cg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
             const double* b, double* x, int kmax, double rtol, int* num_its,
             double* rnorm_history)
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<double> hist;
    *num_its = cg(*comm->comm, *exec->hip, *A->A, b, x, kmax, rtol,
                  rnorm_history ? &hist : nullptr);
    if (rnorm_history)
      std::copy(hist.begin(), hist.end(), rnorm_history);
  });
}

int spmvh_read_petsc_matrix(spmvh_comm* comm, spmvh_exec* exec,
                            const char* filename, int symmetric, int cm,
                            spmvh_matrix** A)
{
  return guarded([&] {
    require(comm && exec && filename && A, "NULL argument");
    auto m = std::make_unique<spmvh_matrix>();
    m->A = read_petsc_binary_matrix(filename, comm->comm, exec->hip,
                                    symmetric != 0, to_cm(cm));
    *A = m.release();
  });
}

int spmvh_read_petsc_vector(spmvh_comm* comm, spmvh_exec* exec,
                            const char* filename, double** device_vec,
                            int64_t* nrows_local)
{
  return guarded([&] {
    require(comm && exec && filename && device_vec, "NULL argument");
    *device_vec = read_petsc_binary_vector(*comm->comm, exec->hip.get(),
                                           filename, nrows_local);
  });
}

int spmvh_petsc_rows_read(const char* filename, int rank, int size,
                          spmvh_petsc_rows** rows, int64_t sizes[7])
{
  return guarded([&] {
    require(filename && rows && sizes && size >= 1 && rank >= 0 && rank < size,
            "bad argument");
    auto r = std::make_unique<spmvh_petsc_rows>();
    r->rows = read_petsc_binary_rows(filename, rank, size);
    sizes[0] = r->rows.nrows_global;
    sizes[1] = r->rows.ncols_global;
    sizes[2] = r->rows.nnz_global;
    sizes[3] = r->rows.row_begin;
    sizes[4] = r->rows.row_end;
    sizes[5] = static_cast<int64_t>(r->rows.values.size());
    sizes[6] = static_cast<int64_t>(r->rows.col_ghosts.size());
    *rows = r.release();
  });
}

int spmvh_petsc_rows_get(spmvh_petsc_rows* rows, int32_t* rowptr,
                         int32_t* colind, double* values, int64_t* col_ghosts)
{
  return guarded([&] {
    require(rows != nullptr, "NULL argument");
    const PetscRows& r = rows->rows;
    if (rowptr)
      std::copy(r.rowptr.begin(), r.rowptr.end(), rowptr);
    if (colind)
      std::copy(r.colind.begin(), r.colind.end(), colind);
    if (values)
      std::copy(r.values.begin(), r.values.end(), values);
    if (col_ghosts)
      std::copy(r.col_ghosts.begin(), r.col_ghosts.end(), col_ghosts);
  });
}

int spmvh_petsc_rows_destroy(spmvh_petsc_rows* rows)
{
  return guarded([&] { delete rows; });
}

int spmvh_cg_workspace_create(spmvh_exec* exec, spmvh_cg_workspace** ws)
{
  return workspace_create<CgWorkspace>(exec, ws);
}

int spmvh_cg_workspace_destroy(spmvh_cg_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_cg_workspace_reserve_timing(spmvh_cg_workspace* ws, int iterations)
{
  return workspace_reserve_timing(ws, iterations);
}

int spmvh_cg_mixed(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                   const double* b, double* x, int kmax, double rtol,
                   int replace_every, int* num_its, double* rnorm_history,
                   int history_capacity, spmvh_cg_workspace* ws, int time_spmv,
                   double out_stats[6])
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (time_spmv & 1) != 0;
    opt.consumer_reductions = (time_spmv & 4) == 0;
    opt.defer_x = (time_spmv & 8) == 0;
    opt.mixed = true;
    opt.replace_every = replace_every;
    CgStats st;
    *num_its = cg(*comm->comm, *exec->hip, *A->A, b, x, kmax, rtol,
                  rnorm_history ? &hist : nullptr, &opt, &st,
                  ws ? ws->ws.get() : nullptr);
    if (rnorm_history)
      std::copy(hist.begin(),
                hist.begin()
                    + std::min<size_t>(hist.size(), (size_t)history_capacity),
                rnorm_history);
    if (out_stats) {
      out_stats[0] = st.spmv_ms_total;
      out_stats[1] = st.spmv_launches;
      out_stats[2] = st.replacements;
      out_stats[3] = st.true_rel_residual;
      out_stats[4] = st.continuation_iterations;
      out_stats[5] = st.final_true_rel_residual;
    }
  });
}

int spmvh_cg_ex(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                const double* b, double* x, int kmax, double rtol, int* num_its,
                double* rnorm_history, spmvh_cg_workspace* ws, int time_spmv,
                double* spmv_ms_total, int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (time_spmv & 1) != 0;
    opt.consumer_reductions = (time_spmv & 4) == 0; // bit 2 switches it off
    opt.defer_x = (time_spmv & 8) == 0;             // bit 3 likewise
    if ((time_spmv >> 8) & 0xff) // bits 8-15: CgOptions::poll_every (0 = default)
      opt.poll_every = (time_spmv >> 8) & 0xff;
    CgStats st;
    *num_its = cg(*comm->comm, *exec->hip, *A->A, b, x, kmax, rtol,
                  rnorm_history ? &hist : nullptr, &opt, &st,
                  ws ? ws->ws.get() : nullptr);
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

int spmvh_cg_block_workspace_create(spmvh_exec* exec,
                                    spmvh_cg_block_workspace** ws)
{
  return workspace_create<CgBlockWorkspace>(exec, ws);
}

int spmvh_cg_block_workspace_destroy(spmvh_cg_block_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_cg_block(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                   const double* B, double* X, int nrhs, int kmax, double rtol,
                   int* max_its, int* iterations, double* rnorm_history,
                   spmvh_cg_block_workspace* ws, int flags,
                   double* spmv_ms_total, int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && max_its && iterations, "NULL argument");
    std::vector<int> its;
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    if ((flags >> 8) & 0xff)
      opt.poll_every = (flags >> 8) & 0xff;
    CgStats st;
    *max_its = cg_block(*comm->comm, *exec->hip, *A->A, B, X, nrhs, kmax, rtol,
                        &its, rnorm_history ? &hist : nullptr, &opt, &st,
                        ws ? ws->ws.get() : nullptr);
    std::copy(its.begin(), its.end(), iterations);
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

// ---- Jacobi-preconditioned CG -----------------------------------------------------------
int spmvh_matrix_diagonal(spmvh_matrix* A, double* d)
{
  return guarded([&] {
    require(A != nullptr && d != nullptr, "NULL argument");
    A->A->diagonal(d);
  });
}

int spmvh_jacobi_inverse(spmvh_exec* exec, const double* d, double* dinv,
                         int64_t n)
{
  return guarded([&] {
    require(exec != nullptr, "NULL argument");
    require(n >= 0 && (n == 0 || (d && dinv)), "bad argument");
    jacobi_inverse(*exec->hip, d, dinv, n);
  });
}

int spmvh_pcg_workspace_create(spmvh_exec* exec, spmvh_pcg_workspace** ws)
{
  return workspace_create<PcgWorkspace>(exec, ws);
}

int spmvh_pcg_workspace_destroy(spmvh_pcg_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_pcg_workspace_reserve_timing(spmvh_pcg_workspace* ws, int iterations)
{
  return workspace_reserve_timing(ws, iterations);
}

int spmvh_pcg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
              const double* b, double* x, const double* dinv, int kmax,
              double rtol, int* num_its, double* rnorm_history,
              spmvh_pcg_workspace* ws, int flags, double* spmv_ms_total,
              int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    opt.consumer_reductions = (flags & 4) == 0; // bit 2 switches it off
    if ((flags >> 8) & 0xff) // bits 8-15: CgOptions::poll_every (0 = default)
      opt.poll_every = (flags >> 8) & 0xff;
    CgStats st;
    *num_its = pcg(*comm->comm, *exec->hip, *A->A, b, x, dinv, kmax, rtol,
                   rnorm_history ? &hist : nullptr, &opt, &st,
                   ws ? ws->ws.get() : nullptr);
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

// ---- Chebyshev polynomial preconditioner ------------------------------------------------
int spmvh_chebyshev_coefficients(int degree, double lmin, double lmax, double* a,
                                 double* b)
{
  return guarded([&] { chebyshev_coefficients(degree, lmin, lmax, a, b); });
}

int spmvh_chebyshev_workspace_create(spmvh_exec* exec,
                                     spmvh_chebyshev_workspace** ws)
{
  return workspace_create<ChebyshevWorkspace>(exec, ws);
}

int spmvh_chebyshev_workspace_destroy(spmvh_chebyshev_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_chebyshev_workspace_reserve_timing(spmvh_chebyshev_workspace* ws,
                                             int spmvs)
{
  return workspace_reserve_timing(ws, spmvs);
}

int spmvh_chebyshev_apply(spmvh_exec* exec, spmvh_matrix* A, const double* r,
                          double* z, const double* dinv, int degree, double lmin,
                          double lmax, spmvh_chebyshev_workspace* ws)
{
  return guarded([&] {
    require(exec && A && r && z, "NULL argument");
    chebyshev_apply(*exec->hip, *A->A, r, z, dinv, degree, lmin, lmax,
                    ws ? ws->ws.get() : nullptr);
  });
}

int spmvh_pcg_chebyshev(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                        const double* b, double* x, const double* dinv,
                        int degree, double lmin, double lmax, int kmax,
                        double rtol, int* num_its, double* rnorm_history,
                        spmvh_chebyshev_workspace* ws, int flags,
                        double* spmv_ms_total, int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    if ((flags >> 8) & 0xff) // bits 8-15: CgOptions::poll_every (0 = default)
      opt.poll_every = (flags >> 8) & 0xff;
    CgStats st;
    *num_its = pcg_chebyshev(*comm->comm, *exec->hip, *A->A, b, x, dinv, degree,
                             lmin, lmax, kmax, rtol,
                             rnorm_history ? &hist : nullptr, &opt, &st,
                             ws ? ws->ws.get() : nullptr);
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

int spmvh_lambda_max_estimate(spmvh_comm* comm, spmvh_exec* exec,
                              spmvh_matrix* A, const double* dinv,
                              const double* v0, int steps, double* lambda)
{
  return guarded([&] {
    require(comm && exec && A && v0 && lambda, "NULL argument");
    *lambda = lambda_max_estimate(*comm->comm, *exec->hip, *A->A, dinv, v0,
                                  steps);
  });
}

// ---- Multicolour symmetric Gauss-Seidel -------------------------------------------------
int spmvh_sgs_color(const int32_t* rowptr, const int32_t* colind, int64_t nrows,
                    int64_t ncols_local, int symmetric, int32_t* colors_out,
                    int* ncolors_out)
{
  return guarded([&] {
    require(nrows == 0 || colors_out, "NULL argument");
    int nc = 0;
    const std::vector<int32_t> c
        = sgs_color(rowptr, colind, nrows, ncols_local, symmetric != 0, &nc);
    std::copy(c.begin(), c.end(), colors_out);
    if (ncolors_out)
      *ncolors_out = nc;
  });
}

int spmvh_sgs_build_create(const int32_t* rowptr, const int32_t* colind,
                           const double* values, int64_t nrows,
                           int64_t ncols_local, int symmetric,
                           spmvh_sgs_build** build, int64_t* sizes)
{
  return guarded([&] {
    require(build && sizes, "NULL argument");
    auto b = std::make_unique<spmvh_sgs_build>();
    b->plan = sgs_build(rowptr, colind, values, nullptr, nrows, ncols_local,
                        symmetric != 0);
    sizes[0] = b->plan.num_colors;
    sizes[1] = (int64_t)b->plan.before.col.size();
    sizes[2] = (int64_t)b->plan.after.col.size();
    *build = b.release();
  });
}

int spmvh_sgs_build_get(spmvh_sgs_build* build, int32_t* colors, int32_t* perm,
                        int32_t* color_start, double* d, int64_t* before_ptr,
                        int32_t* before_col, double* before_val,
                        int64_t* after_ptr, int32_t* after_col,
                        double* after_val)
{
  return guarded([&] {
    require(build != nullptr, "NULL argument");
    auto out = [](const auto& v, auto* dst) {
      if (dst)
        std::copy(v.begin(), v.end(), dst);
    };
    const SgsHostPlan& p = build->plan;
    out(p.colors, colors);
    out(p.perm, perm);
    out(p.color_start, color_start);
    out(p.d, d);
    out(p.before.ptr, before_ptr);
    out(p.before.col, before_col);
    out(p.before.val, before_val);
    out(p.after.ptr, after_ptr);
    out(p.after.col, after_col);
    out(p.after.val, after_val);
  });
}

int spmvh_sgs_build_destroy(spmvh_sgs_build* build)
{
  return guarded([&] { delete build; });
}

int spmvh_sgs_create(spmvh_exec* exec, spmvh_matrix* A, spmvh_sgs** M)
{
  return guarded([&] {
    require(exec && A && M, "NULL argument");
    require(exec->hip != nullptr, "not a HipExecutor");
    auto m = std::make_unique<spmvh_sgs>();
    m->exec = exec->hip;
    m->M.reset(new SgsPreconditioner(*exec->hip, *A->A));
    *M = m.release();
  });
}

int spmvh_sgs_create_ex(spmvh_exec* exec, spmvh_matrix* A, int setup, int order,
                        const int32_t* colors, spmvh_sgs** M)
{
  return guarded([&] {
    // the rules of the options first: they need no handle
    require(setup == 0 || setup == 1, "setup: 0 (host) or 1 (device)");
    require(order >= -1 && order <= 1,
            "order: -1 (default), 0 (hashed) or 1 (natural)");
    // (an order given explicitly counts as given, the default included)
    require(setup == 1 || (order == -1 && !colors),
            "setup = host colours by itself: it takes neither colors nor an "
            "order");
    require(exec && A && M, "NULL argument");
    require(exec->hip != nullptr, "not a HipExecutor");
    SgsOptions opt;
    opt.setup = setup == 1 ? SgsSetup::device : SgsSetup::host;
    opt.order = order == 1 ? SgsOrder::natural : SgsOrder::hashed;
    opt.colors = colors;
    auto m = std::make_unique<spmvh_sgs>();
    m->exec = exec->hip;
    m->M.reset(new SgsPreconditioner(*exec->hip, *A->A, opt));
    *M = m.release();
  });
}

namespace
{
// the rules of SgsOptions, before any handle is looked at
SgsOptions sgs_options_of(int setup, int order, const int32_t* colors, int values)
{
  require(setup == 0 || setup == 1, "setup: 0 (host) or 1 (device)");
  require(order >= -1 && order <= 1,
          "order: -1 (default), 0 (hashed) or 1 (natural)");
  require(values == 0 || values == 1, "values: 0 (fp64) or 1 (fp32)");
  // (an order given explicitly counts as given, the default included)
  require(setup == 1 || (order == -1 && !colors),
          "setup = host colours by itself: it takes neither colors nor an "
          "order");
  SgsOptions opt;
  opt.setup = setup == 1 ? SgsSetup::device : SgsSetup::host;
  opt.order = order == 1 ? SgsOrder::natural : SgsOrder::hashed;
  opt.colors = colors;
  opt.values = values == 1 ? SgsValues::fp32 : SgsValues::fp64;
  return opt;
}
} // namespace

int spmvh_sgs_create_ex2(spmvh_exec* exec, spmvh_matrix* A, int setup, int order,
                         const int32_t* colors, int values, spmvh_sgs** M)
{
  return guarded([&] {
    const SgsOptions opt = sgs_options_of(setup, order, colors, values);
    require(exec && A && M, "NULL argument");
    require(exec->hip != nullptr, "not a HipExecutor");
    auto m = std::make_unique<spmvh_sgs>();
    m->exec = exec->hip;
    m->M.reset(new SgsPreconditioner(*exec->hip, *A->A, opt));
    *M = m.release();
  });
}

int spmvh_sgs_value_bits(spmvh_sgs* M, int* bits)
{
  return guarded([&] {
    require(M && bits, "NULL argument");
    *bits = M->M->value_bits();
  });
}

int spmvh_fp32_range_count(const double* values, int64_t n, int64_t* count)
{
  return guarded([&] {
    require(count && n >= 0 && (n == 0 || values), "NULL argument");
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i)
      bad += spmv_fp32_out_of_range(values[i]) ? 1 : 0;
    *count = bad;
  });
}

int spmvh_sgs_setup_info(spmvh_sgs* M, int* rounds, double* setup_ms)
{
  return guarded([&] {
    require(M != nullptr, "NULL argument");
    if (rounds)
      *rounds = M->M->rounds();
    if (setup_ms)
      *setup_ms = M->M->setup_ms();
  });
}

int spmvh_sgs_setup_detail(spmvh_sgs* M, double* color_ms, double* build_ms,
                           int64_t* temp_bytes)
{
  return guarded([&] {
    require(M != nullptr, "NULL argument");
    if (color_ms)
      *color_ms = M->M->color_ms();
    if (build_ms)
      *build_ms = M->M->build_ms();
    if (temp_bytes)
      *temp_bytes = M->M->setup_temp_bytes();
  });
}

int spmvh_sgs_export_sizes(spmvh_sgs* M, int64_t* sizes)
{
  return guarded([&] {
    require(M && sizes, "NULL argument");
    throw_on_error(spmv_hip_mcgs_plan_sizes(M->M->plan(), sizes),
                   "spmv_hip_mcgs_plan_sizes");
  });
}

int spmvh_sgs_export(spmvh_sgs* M, int32_t* perm, int32_t* color_start,
                     double* dinv, void* const* before, void* const* after)
{
  return guarded([&] {
    require(M != nullptr, "NULL argument");
    auto part_of = [](void* const* q) {
      return spmv_hip_mcgs_export{
          (int32_t*)q[0], (int32_t*)q[1], (int64_t*)q[2],  (int32_t*)q[3],
          (int32_t*)q[4], (double*)q[5],  (int32_t*)q[6],  (int32_t*)q[7],
          (int64_t*)q[8], (int32_t*)q[9], (double*)q[10]};
    };
    spmv_hip_mcgs_export b{}, a{};
    if (before)
      b = part_of(before);
    if (after)
      a = part_of(after);
    throw_on_error(spmv_hip_mcgs_plan_export(M->M->plan(), perm, color_start,
                                             dinv, before ? &b : nullptr,
                                             after ? &a : nullptr),
                   "spmv_hip_mcgs_plan_export");
  });
}

int spmvh_sgs_destroy(spmvh_sgs* M)
{
  return guarded([&] { delete M; });
}

int spmvh_sgs_info(spmvh_sgs* M, int* rows, int* num_colors, int64_t* plan_bytes)
{
  return guarded([&] {
    require(M != nullptr, "NULL argument");
    if (rows)
      *rows = M->M->rows();
    if (num_colors)
      *num_colors = M->M->num_colors();
    if (plan_bytes)
      *plan_bytes = M->M->plan_bytes();
  });
}

int spmvh_sgs_colors(spmvh_sgs* M, int32_t* colors)
{
  return guarded([&] {
    require(M != nullptr, "NULL argument");
    M->M->colors(colors);
  });
}

int spmvh_sgs_apply(spmvh_exec* exec, spmvh_sgs* M, const double* r, double* z)
{
  return guarded([&] {
    require(exec && M, "NULL argument");
    sgs_apply(*exec->hip, *M->M, r, z);
  });
}

// ---- Multicolour ILU(0) --------------------------------------------------------------
int spmvh_ilu0_symbolic_create(const int32_t* rowptr, const int32_t* colind,
                               int64_t nrows, int64_t ncols_local, int symmetric,
                               spmvh_ilu0_symbolic** sym, int64_t* sizes)
{
  return guarded([&] {
    require(sym && sizes, "NULL argument");
    auto s = std::make_unique<spmvh_ilu0_symbolic>();
    s->sym = ilu0_symbolic(rowptr, colind, nrows, ncols_local, symmetric != 0);
    const Ilu0Symbolic& y = s->sym;
    sizes[0] = y.num_colors;
    sizes[1] = (int64_t)y.before.cpos.size();
    sizes[2] = (int64_t)y.after.cpos.size();
    sizes[3] = (int64_t)y.sliced_before.col.size();
    sizes[4] = (int64_t)y.sliced_before.long_col.size();
    sizes[5] = (int64_t)y.sliced_after.col.size();
    sizes[6] = (int64_t)y.sliced_after.long_col.size();
    *sym = s.release();
  });
}

int spmvh_ilu0_symbolic_get(spmvh_ilu0_symbolic* sym, int32_t* colors,
                            int32_t* perm, int32_t* pos, int32_t* color_start,
                            int64_t* before_ptr, int32_t* before_cpos,
                            int32_t* before_src, int64_t* before_slot,
                            int32_t* before_sliced_col, int32_t* before_long_col,
                            int64_t* after_ptr, int32_t* after_cpos,
                            int32_t* after_src, int64_t* after_slot,
                            int32_t* after_sliced_col, int32_t* after_long_col)
{
  return guarded([&] {
    require(sym != nullptr, "NULL argument");
    auto out = [](const auto& v, auto* dst) {
      if (dst)
        std::copy(v.begin(), v.end(), dst);
    };
    const Ilu0Symbolic& y = sym->sym;
    out(y.colors, colors);
    out(y.perm, perm);
    out(y.pos, pos);
    out(y.color_start, color_start);
    out(y.before.ptr, before_ptr);
    out(y.before.cpos, before_cpos);
    out(y.before.src, before_src);
    out(y.before.slot, before_slot);
    out(y.sliced_before.col, before_sliced_col);
    out(y.sliced_before.long_col, before_long_col);
    out(y.after.ptr, after_ptr);
    out(y.after.cpos, after_cpos);
    out(y.after.src, after_src);
    out(y.after.slot, after_slot);
    out(y.sliced_after.col, after_sliced_col);
    out(y.sliced_after.long_col, after_long_col);
  });
}

int spmvh_ilu0_symbolic_destroy(spmvh_ilu0_symbolic* sym)
{
  return guarded([&] { delete sym; });
}

int spmvh_ilu0_create(spmvh_exec* exec, spmvh_matrix* A, spmvh_sgs** M)
{
  return guarded([&] {
    require(exec && A && M, "NULL argument");
    require(exec->hip != nullptr, "not a HipExecutor");
    auto m = std::make_unique<spmvh_sgs>();
    m->exec = exec->hip;
    m->M.reset(new Ilu0Preconditioner(*exec->hip, *A->A));
    *M = m.release();
  });
}

int spmvh_ilu0_create_ex(spmvh_exec* exec, spmvh_matrix* A, int setup, int order,
                         const int32_t* colors, spmvh_sgs** M)
{
  return guarded([&] {
    // the rules of spmvh_sgs_create_ex
    require(setup == 0 || setup == 1, "setup: 0 (host) or 1 (device)");
    require(order >= -1 && order <= 1,
            "order: -1 (default), 0 (hashed) or 1 (natural)");
    require(setup == 1 || (order == -1 && !colors),
            "setup = host colours by itself: it takes neither colors nor an "
            "order");
    require(exec && A && M, "NULL argument");
    require(exec->hip != nullptr, "not a HipExecutor");
    SgsOptions opt;
    opt.setup = setup == 1 ? SgsSetup::device : SgsSetup::host;
    opt.order = order == 1 ? SgsOrder::natural : SgsOrder::hashed;
    opt.colors = colors;
    auto m = std::make_unique<spmvh_sgs>();
    m->exec = exec->hip;
    m->M.reset(new Ilu0Preconditioner(*exec->hip, *A->A, opt));
    *M = m.release();
  });
}

int spmvh_ilu0_create_ex2(spmvh_exec* exec, spmvh_matrix* A, int setup,
                          int order, const int32_t* colors, int values,
                          spmvh_sgs** M)
{
  return guarded([&] {
    const SgsOptions opt = sgs_options_of(setup, order, colors, values);
    require(exec && A && M, "NULL argument");
    require(exec->hip != nullptr, "not a HipExecutor");
    auto m = std::make_unique<spmvh_sgs>();
    m->exec = exec->hip;
    m->M.reset(new Ilu0Preconditioner(*exec->hip, *A->A, opt));
    *M = m.release();
  });
}

namespace
{
Ilu0Preconditioner& ilu0_of(spmvh_sgs* M)
{
  require(M != nullptr, "NULL argument");
  auto* ilu = dynamic_cast<Ilu0Preconditioner*>(M->M.get());
  require(ilu != nullptr, "not an Ilu0Preconditioner");
  return *ilu;
}
} // namespace

int spmvh_ilu0_refactor(spmvh_sgs* M, spmvh_matrix* A)
{
  return guarded([&] {
    require(A != nullptr, "NULL argument");
    ilu0_of(M).refactor(*A->A);
  });
}

int spmvh_ilu0_info(spmvh_sgs* M, int64_t* info)
{
  return guarded([&] {
    require(info != nullptr, "NULL argument");
    const Ilu0Preconditioner& ilu = ilu0_of(M);
    info[0] = ilu.before_entries();
    info[1] = ilu.after_entries();
    info[2] = ilu.negative_pivots();
    info[3] = ilu.plan_bytes();
    info[4] = (int64_t)(ilu.symbolic_ms() * 1000.0);
    info[5] = (int64_t)(ilu.numeric_ms() * 1000.0);
  });
}

int spmvh_ilu0_pattern(spmvh_sgs* M, int64_t* before_ptr, int32_t* before_col,
                       int64_t* after_ptr, int32_t* after_col)
{
  return guarded([&] {
    ilu0_of(M).pattern(before_ptr, before_col, after_ptr, after_col);
  });
}

int spmvh_ilu0_factor(spmvh_sgs* M, double* l, double* u, double* d)
{
  return guarded([&] { ilu0_of(M).factor(l, u, d); });
}

int spmvh_ilu0_export_sizes(spmvh_sgs* M, int64_t* sizes)
{
  return guarded([&] {
    require(sizes != nullptr, "NULL argument");
    throw_on_error(spmv_hip_ilu0_plan_sizes(ilu0_of(M).ilu_plan(), sizes),
                   "spmv_hip_ilu0_plan_sizes");
  });
}

int spmvh_ilu0_export(spmvh_sgs* M, void* const* before, void* const* after)
{
  return guarded([&] {
    auto part_of = [](void* const* q) {
      return spmv_hip_ilu0_export{(int64_t*)q[0], (int32_t*)q[1], (int32_t*)q[2],
                                  (int64_t*)q[3]};
    };
    spmv_hip_ilu0_export b{}, a{};
    if (before)
      b = part_of(before);
    if (after)
      a = part_of(after);
    throw_on_error(spmv_hip_ilu0_plan_export(ilu0_of(M).ilu_plan(),
                                             before ? &b : nullptr,
                                             after ? &a : nullptr),
                   "spmv_hip_ilu0_plan_export");
  });
}

int spmvh_sgs_workspace_create(spmvh_exec* exec, spmvh_sgs_workspace** ws)
{
  return workspace_create<SgsWorkspace>(exec, ws);
}

int spmvh_sgs_workspace_destroy(spmvh_sgs_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_sgs_workspace_reserve_timing(spmvh_sgs_workspace* ws, int iterations)
{
  return workspace_reserve_timing(ws, iterations);
}

int spmvh_pcg_sgs(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                  spmvh_sgs* M, const double* b, double* x, int kmax,
                  double rtol, int* num_its, double* rnorm_history,
                  spmvh_sgs_workspace* ws, int flags, double* spmv_ms_total,
                  int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && M && num_its, "NULL argument");
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    if ((flags >> 8) & 0xff) // bits 8-15: CgOptions::poll_every (0 = default)
      opt.poll_every = (flags >> 8) & 0xff;
    CgStats st;
    *num_its = pcg_sgs(*comm->comm, *exec->hip, *A->A, *M->M, b, x, kmax, rtol,
                       rnorm_history ? &hist : nullptr, &opt, &st,
                       ws ? ws->ws.get() : nullptr);
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

// ---- Preconditioned CG for several right-hand sides -----------------------------------------
int spmvh_sgs_apply_block(spmvh_exec* exec, spmvh_sgs* M, const double* R,
                          double* Z, int nrhs)
{
  return guarded([&] {
    require(exec && M, "NULL argument");
    sgs_apply_block(*exec->hip, *M->M, R, Z, nrhs);
  });
}

int spmvh_pcg_block_workspace_create(spmvh_exec* exec,
                                     spmvh_pcg_block_workspace** ws)
{
  return workspace_create<PcgBlockWorkspace>(exec, ws);
}

int spmvh_pcg_block_workspace_destroy(spmvh_pcg_block_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_pcg_block_check_arguments(int nrhs, int kmax, int has_dinv,
                                    int has_sgs, int64_t sgs_rows,
                                    int64_t sgs_negative_pivots, int64_t rows,
                                    const double* B, const double* X,
                                    const double* dinv)
{
  return guarded([&] {
    pcg_block_check_rules(nrhs, kmax, has_dinv != 0, has_sgs != 0, sgs_rows,
                          sgs_negative_pivots, rows, B, X, dinv);
  });
}

int spmvh_pcg_block(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                    const double* B, double* X, int nrhs, const double* dinv,
                    spmvh_sgs* M, int kmax, double rtol, int* max_its,
                    int* iterations, double* rnorm_history,
                    spmvh_pcg_block_workspace* ws, int flags,
                    double* spmv_ms_total, int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && max_its && iterations, "NULL argument");
    std::vector<int> its;
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    if ((flags >> 8) & 0xff)
      opt.poll_every = (flags >> 8) & 0xff;
    CgStats st;
    BlockPreconditioner pre;
    pre.dinv = dinv;
    pre.sgs = M ? M->M.get() : nullptr;
    *max_its = pcg_block(*comm->comm, *exec->hip, *A->A, B, X, nrhs, pre, kmax,
                         rtol, &its, rnorm_history ? &hist : nullptr, &opt, &st,
                         ws ? ws->ws.get() : nullptr);
    std::copy(its.begin(), its.end(), iterations);
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

int spmvh_pcg_block_amg_check_arguments(int nrhs, int kmax, int has_dinv,
                                        int has_sgs, int has_amg,
                                        int64_t sgs_rows,
                                        int64_t sgs_negative_pivots,
                                        int64_t amg_rows, int64_t rows,
                                        const double* B, const double* X,
                                        const double* dinv)
{
  return guarded([&] {
    pcg_block_check_rules(nrhs, kmax, has_dinv != 0, has_sgs != 0, has_amg != 0,
                          sgs_rows, sgs_negative_pivots, amg_rows, rows, B, X,
                          dinv);
  });
}

int spmvh_amg_apply_block_check_arguments(int nrhs, int64_t rows,
                                          const double* R, const double* Z)
{
  return guarded([&] { amg_apply_block_check_rules(nrhs, rows, R, Z); });
}

int spmvh_pcg_block_amg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                        const double* B, double* X, int nrhs, spmvh_amg* M,
                        int kmax, double rtol, int* max_its, int* iterations,
                        double* rnorm_history, spmvh_pcg_block_workspace* ws,
                        int flags, double* spmv_ms_total, int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && max_its && iterations, "NULL argument");
    std::vector<int> its;
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    if ((flags >> 8) & 0xff)
      opt.poll_every = (flags >> 8) & 0xff;
    CgStats st;
    BlockPreconditioner pre;
    pre.amg = M ? M->M.get() : nullptr;
    *max_its = pcg_block(*comm->comm, *exec->hip, *A->A, B, X, nrhs, pre, kmax,
                         rtol, &its, rnorm_history ? &hist : nullptr, &opt, &st,
                         ws ? ws->ws.get() : nullptr);
    std::copy(its.begin(), its.end(), iterations);
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

// ---- Aggregation multigrid ---------------------------------------------------------------
int spmvh_amg_check_options(double theta, int max_levels,
                            int64_t min_coarse_rows, int smooth_degree,
                            int coarse_degree, double eig_ratio,
                            double coarse_scale)
{
  return guarded([&] {
    amg_check_options(theta, max_levels, min_coarse_rows, smooth_degree,
                      coarse_degree, eig_ratio, coarse_scale);
  });
}

int spmvh_amg_symbolic_create(const int32_t* rowptr, const int32_t* colind,
                              const double* values, const double* diagonal,
                              int64_t nrows, int64_t ncols_local, int symmetric,
                              double theta, spmvh_amg_symbolic** sym,
                              int64_t* sizes)
{
  return guarded([&] {
    require(sym && sizes, "NULL argument");
    require(!symmetric || nrows == 0 || diagonal, "NULL diagonal");
    amg_check_options(theta, 1, 1, 1, 1, 2.0, 1.0);
    auto s = std::make_unique<spmvh_amg_symbolic>();
    s->x = amg_expand(rowptr, colind, nrows, ncols_local, symmetric != 0);
    require(s->x.num_values == 0 || values, "NULL values");
    s->step = amg_coarsen(s->x, values, diagonal, theta);
    sizes[0] = s->step.n_agg;
    sizes[1] = (int64_t)s->step.colind.size();
    sizes[2] = (int64_t)s->step.src.size();
    sizes[3] = (int64_t)s->x.col.size();
    *sym = s.release();
  });
}

int spmvh_amg_symbolic_get(spmvh_amg_symbolic* sym, int32_t* agg,
                           int32_t* member_ptr, int32_t* member,
                           int32_t* rowptr, int32_t* colind, int64_t* src_ptr,
                           int32_t* src, int64_t* xrow_ptr, int32_t* xrow_col,
                           int32_t* xrow_src)
{
  return guarded([&] {
    require(sym != nullptr, "NULL argument");
    auto out = [](const auto& v, auto* dst) {
      if (dst)
        std::copy(v.begin(), v.end(), dst);
    };
    const AmgStep& t = sym->step;
    out(t.agg, agg);
    out(t.member_ptr, member_ptr);
    out(t.member, member);
    out(t.rowptr, rowptr);
    out(t.colind, colind);
    out(t.src_ptr, src_ptr);
    out(t.src, src);
    out(sym->x.ptr, xrow_ptr);
    out(sym->x.col, xrow_col);
    out(sym->x.src, xrow_src);
  });
}

int spmvh_amg_symbolic_destroy(spmvh_amg_symbolic* sym)
{
  return guarded([&] { delete sym; });
}

int spmvh_amg_create(spmvh_exec* exec, spmvh_matrix* A, const double* options,
                     spmvh_amg** M)
{
  return guarded([&] {
    require(exec && A && M, "NULL argument");
    require(exec->hip != nullptr, "not a HipExecutor");
    AmgOptions opt;
    if (options) {
      opt.theta = options[0];
      opt.max_levels = (int)options[1];
      opt.min_coarse_rows = (int64_t)options[2];
      opt.smooth_degree = (int)options[3];
      opt.coarse_degree = (int)options[4];
      opt.eig_ratio = options[5];
      opt.coarse_scale = options[6];
    }
    auto m = std::make_unique<spmvh_amg>();
    m->M.reset(new AmgPreconditioner(*exec->hip, *A->A, opt));
    *M = m.release();
  });
}

int spmvh_amg_create_ex(spmvh_exec* exec, spmvh_matrix* A, const double* options,
                        int setup, int order, spmvh_amg** M)
{
  return guarded([&] {
    require(exec && A && M, "NULL argument");
    require(exec->hip != nullptr, "not a HipExecutor");
    require(setup == 0 || setup == 1, "setup is 0 (host) or 1 (device)");
    require(order >= -1 && order <= 1,
            "order is -1 (none given), 0 (hashed) or 1 (natural)");
    if (setup == 0 && order >= 0)
      throw std::invalid_argument(
          "spmv::AmgPreconditioner - Error: setup = host aggregates in row "
          "order: it takes no order");
    AmgOptions opt;
    if (options) {
      opt.theta = options[0];
      opt.max_levels = (int)options[1];
      opt.min_coarse_rows = (int64_t)options[2];
      opt.smooth_degree = (int)options[3];
      opt.coarse_degree = (int)options[4];
      opt.eig_ratio = options[5];
      opt.coarse_scale = options[6];
    }
    opt.setup = setup == 1 ? SgsSetup::device : SgsSetup::host;
    opt.order = order == 1 ? SgsOrder::natural : SgsOrder::hashed;
    auto m = std::make_unique<spmvh_amg>();
    m->M.reset(new AmgPreconditioner(*exec->hip, *A->A, opt));
    *M = m.release();
  });
}

int spmvh_amg_setup_info(spmvh_amg* M, int64_t* info)
{
  return guarded([&] {
    require(M && info, "NULL argument");
    info[0] = (int64_t)(M->M->aggregate_ms() * 1000.0);
    info[1] = (int64_t)(M->M->build_ms() * 1000.0);
    info[2] = M->M->setup_temp_bytes();
    info[3] = M->M->options().setup == SgsSetup::device ? 1 : 0;
  });
}

int spmvh_amg_level_rounds(spmvh_amg* M, int level, int* rounds)
{
  return guarded([&] {
    require(M && rounds, "NULL argument");
    rounds[0] = M->M->rounds(level, 0);
    rounds[1] = M->M->rounds(level, 1);
  });
}

int spmvh_amg_step_sizes(spmvh_amg* M, int level, int64_t* sizes)
{
  return guarded([&] {
    require(M && sizes, "NULL argument");
    const spmv_hip_amg_plan* p = M->M->step_plan(level);
    for (int k = 0; k < SPMV_HIP_AMG_SIZES_WORDS; ++k)
      sizes[k] = 0;
    if (p)
      throw_on_error(spmv_hip_amg_plan_sizes(p, sizes), "spmv_hip_amg_plan_sizes");
  });
}

int spmvh_amg_step_export(spmvh_amg* M, int level, int32_t* agg,
                          int32_t* member_ptr, int32_t* member, int64_t* src_ptr,
                          int32_t* src, int64_t* xrow_ptr, int32_t* xrow_src)
{
  return guarded([&] {
    require(M != nullptr, "NULL argument");
    const spmv_hip_amg_plan* p = M->M->step_plan(level);
    require(p != nullptr, "the level has no plan");
    const spmv_hip_amg_export ex{agg, member_ptr, member, src_ptr,
                                 src, xrow_ptr,   xrow_src};
    throw_on_error(spmv_hip_amg_plan_export(p, &ex), "spmv_hip_amg_plan_export");
  });
}

int spmvh_amg_destroy(spmvh_amg* M)
{
  return guarded([&] { delete M; });
}

int spmvh_amg_refresh(spmvh_amg* M, spmvh_matrix* A)
{
  return guarded([&] {
    require(M && A, "NULL argument");
    M->M->refresh(*A->A);
  });
}

int spmvh_amg_info(spmvh_amg* M, int64_t* info)
{
  return guarded([&] {
    require(M && info, "NULL argument");
    info[0] = M->M->levels();
    info[1] = M->M->plan_bytes();
    info[2] = (int64_t)(M->M->symbolic_ms() * 1000.0);
    info[3] = (int64_t)(M->M->numeric_ms() * 1000.0);
  });
}

int spmvh_amg_level_info(spmvh_amg* M, int level, int64_t* sizes, double* lmax)
{
  return guarded([&] {
    require(M && sizes && lmax, "NULL argument");
    sizes[0] = M->M->rows(level);
    sizes[1] = M->M->non_zeros(level);
    *lmax = M->M->lmax(level);
  });
}

int spmvh_amg_aggregates(spmvh_amg* M, int level, int32_t* agg)
{
  return guarded([&] {
    require(M != nullptr, "NULL argument");
    M->M->aggregates(level, agg);
  });
}

int spmvh_amg_level_matrix(spmvh_amg* M, int level, int32_t* rowptr,
                           int32_t* colind, double* values)
{
  return guarded([&] {
    require(M != nullptr, "NULL argument");
    M->M->level_matrix(level, rowptr, colind, values);
  });
}

int spmvh_amg_check_tail_rows(int64_t max_rows)
{
  return guarded([&] { amg_check_tail_rows(max_rows); });
}

int spmvh_amg_set_tail_rows(spmvh_amg* M, int64_t max_rows)
{
  return guarded([&] {
    amg_check_tail_rows(max_rows); // (before the handle: no device is needed)
    require(M != nullptr, "NULL argument");
    M->M->set_tail_rows(max_rows);
  });
}

int spmvh_amg_tail_levels(spmvh_amg* M, int* tail_levels)
{
  return guarded([&] {
    require(M && tail_levels, "NULL argument");
    *tail_levels = M->M->tail_levels();
  });
}

int spmvh_amg_tail_lanes(spmvh_amg* M, int level, int* lanes)
{
  return guarded([&] {
    require(M && lanes, "NULL argument");
    *lanes = M->M->tail_lanes(level);
  });
}

int spmvh_amg_apply(spmvh_exec* exec, spmvh_amg* M, const double* r, double* z)
{
  return guarded([&] {
    require(exec && M, "NULL argument");
    amg_apply(*exec->hip, *M->M, r, z);
  });
}

int spmvh_amg_apply_block(spmvh_exec* exec, spmvh_amg* M, const double* R,
                          double* Z, int nrhs)
{
  return guarded([&] {
    require(exec && M, "NULL argument");
    amg_apply_block(*exec->hip, *M->M, R, Z, nrhs);
  });
}

int spmvh_amg_release_block_scratch(spmvh_amg* M)
{
  return guarded([&] {
    require(M, "NULL argument");
    M->M->release_block_scratch();
  });
}

int spmvh_pcg_amg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                  spmvh_amg* M, const double* b, double* x, int kmax,
                  double rtol, int* num_its, double* rnorm_history,
                  spmvh_sgs_workspace* ws, int flags, double* spmv_ms_total,
                  int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && M && num_its, "NULL argument");
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    if ((flags >> 8) & 0xff) // bits 8-15: CgOptions::poll_every (0 = default)
      opt.poll_every = (flags >> 8) & 0xff;
    CgStats st;
    *num_its = pcg_amg(*comm->comm, *exec->hip, *A->A, *M->M, b, x, kmax, rtol,
                       rnorm_history ? &hist : nullptr, &opt, &st,
                       ws ? ws->ws.get() : nullptr);
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

// ---- BiCGStab ---------------------------------------------------------------------------
int spmvh_bicgstab_workspace_create(spmvh_exec* exec,
                                    spmvh_bicgstab_workspace** ws)
{
  return workspace_create<BicgstabWorkspace>(exec, ws);
}

int spmvh_bicgstab_workspace_destroy(spmvh_bicgstab_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_bicgstab_workspace_reserve_timing(spmvh_bicgstab_workspace* ws,
                                            int iterations)
{
  return workspace_reserve_timing(ws, iterations);
}

int spmvh_bicgstab(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                   const double* b, double* x, const double* dinv, int kmax,
                   double rtol, int* num_its, int* status,
                   double* rnorm_history, spmvh_bicgstab_workspace* ws,
                   int flags, double* spmv_ms_total, int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    opt.consumer_reductions = (flags & 4) == 0; // bit 2 switches it off
    if ((flags >> 8) & 0xff) // bits 8-15: CgOptions::poll_every (0 = default)
      opt.poll_every = (flags >> 8) & 0xff;
    CgStats st;
    int how = 0;
    *num_its = bicgstab(*comm->comm, *exec->hip, *A->A, b, x, dinv, kmax, rtol,
                        rnorm_history ? &hist : nullptr, &opt, &st,
                        ws ? ws->ws.get() : nullptr, &how);
    if (status)
      *status = how;
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

// ---- GMRES ------------------------------------------------------------------------------
int spmvh_gmres_workspace_create(spmvh_exec* exec, spmvh_gmres_workspace** ws)
{
  return workspace_create<GmresWorkspace>(exec, ws);
}

int spmvh_gmres_workspace_destroy(spmvh_gmres_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_gmres_workspace_reserve_timing(spmvh_gmres_workspace* ws,
                                         int iterations)
{
  return workspace_reserve_timing(ws, iterations);
}

int spmvh_gmres_check_arguments(int restart, int kmax, int cheb_degree,
                                double lmin, double lmax)
{
  return guarded([&] {
    GmresPreconditioner pre;
    pre.cheb_degree = cheb_degree;
    pre.lmin = lmin;
    pre.lmax = lmax;
    gmres_check_arguments(&pre, restart, kmax, 0);
  });
}

int spmvh_gmres(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                const double* b, double* x, const double* dinv,
                int cheb_degree, double lmin, double lmax, spmvh_sgs* sgs,
                int restart, int kmax, double rtol, int* num_its, int* status,
                double* rnorm_history, spmvh_gmres_workspace* ws, int flags,
                double* spmv_ms_total, int* spmv_launches)
{
  return spmvh_gmres_amg(comm, exec, A, b, x, dinv, cheb_degree, lmin, lmax, sgs,
                         restart, kmax, rtol, num_its, status, rnorm_history, ws,
                         flags, spmv_ms_total, spmv_launches, nullptr);
}

int spmvh_gmres_amg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                    const double* b, double* x, const double* dinv,
                    int cheb_degree, double lmin, double lmax, spmvh_sgs* sgs,
                    int restart, int kmax, double rtol, int* num_its,
                    int* status, double* rnorm_history,
                    spmvh_gmres_workspace* ws, int flags, double* spmv_ms_total,
                    int* spmv_launches, spmvh_amg* amg)
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    if ((flags >> 8) & 0xff) // bits 8-15: CgOptions::poll_every (0 = default)
      opt.poll_every = (flags >> 8) & 0xff;
    GmresPreconditioner pre;
    pre.dinv = dinv;
    pre.cheb_degree = cheb_degree;
    pre.lmin = lmin;
    pre.lmax = lmax;
    pre.sgs = sgs ? sgs->M.get() : nullptr;
    pre.amg = amg ? amg->M.get() : nullptr;
    CgStats st;
    int how = 0;
    *num_its = gmres(*comm->comm, *exec->hip, *A->A, b, x, &pre, restart, kmax,
                     rtol, rnorm_history ? &hist : nullptr, &opt, &st,
                     ws ? ws->ws.get() : nullptr, &how);
    if (status)
      *status = how;
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

// ---- MINRES -----------------------------------------------------------------------------
int spmvh_minres_workspace_create(spmvh_exec* exec, spmvh_minres_workspace** ws)
{
  return workspace_create<MinresWorkspace>(exec, ws);
}

int spmvh_minres_workspace_destroy(spmvh_minres_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_minres_workspace_reserve_timing(spmvh_minres_workspace* ws,
                                          int iterations)
{
  return workspace_reserve_timing(ws, iterations);
}

int spmvh_minres_check_rules(int kmax, int has_dinv, int has_sgs, int has_amg,
                             int64_t sgs_rows, int64_t sgs_negative_pivots,
                             int64_t amg_rows, int64_t rows, const double* b,
                             const double* x, const double* dinv)
{
  return guarded([&] {
    minres_check_rules(kmax, has_dinv != 0, has_sgs != 0, has_amg != 0,
                       sgs_rows, sgs_negative_pivots, amg_rows, rows, b, x,
                       dinv);
  });
}

int spmvh_minres(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                 const double* b, double* x, const double* dinv,
                 spmvh_sgs* sgs, spmvh_amg* amg, int kmax, double rtol,
                 int* num_its, int* status, double* rnorm_history,
                 spmvh_minres_workspace* ws, int flags, double* spmv_ms_total,
                 int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    if ((flags >> 8) & 0xff) // bits 8-15: CgOptions::poll_every (0 = default)
      opt.poll_every = (flags >> 8) & 0xff;
    MinresPreconditioner pre;
    pre.dinv = dinv;
    pre.sgs = sgs ? sgs->M.get() : nullptr;
    pre.amg = amg ? amg->M.get() : nullptr;
    CgStats st;
    int how = 0;
    *num_its = minres(*comm->comm, *exec->hip, *A->A, b, x, &pre, kmax, rtol,
                      rnorm_history ? &hist : nullptr, &opt, &st,
                      ws ? ws->ws.get() : nullptr, &how);
    if (status)
      *status = how;
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

// ---- LSQR -------------------------------------------------------------------------------
int spmvh_lsqr_workspace_create(spmvh_exec* exec, spmvh_lsqr_workspace** ws)
{
  return workspace_create<LsqrWorkspace>(exec, ws);
}

int spmvh_lsqr_workspace_destroy(spmvh_lsqr_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_lsqr_workspace_reserve_timing(spmvh_lsqr_workspace* ws, int iterations)
{
  return workspace_reserve_timing(ws, iterations);
}

int spmvh_lsqr_check_rules(int kmax, double ltol, double damp, int64_t rows,
                           int64_t cols, const double* b, const double* x)
{
  return guarded([&] { lsqr_check_rules(kmax, ltol, damp, rows, cols, b, x); });
}

int spmvh_lsqr(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
               const double* b, double* x, int kmax, double rtol, double ltol,
               double damp, int* num_its, int* status, double* hist_r,
               double* hist_ar, spmvh_lsqr_workspace* ws, int flags,
               double* spmv_ms_total, int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<double> hr, har;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    if ((flags >> 8) & 0xff) // bits 8-15: CgOptions::poll_every (0 = default)
      opt.poll_every = (flags >> 8) & 0xff;
    CgStats st;
    int how = 0;
    *num_its = lsqr(*comm->comm, *exec->hip, *A->A, b, x, kmax, rtol, ltol, damp,
                    hist_r ? &hr : nullptr, hist_ar ? &har : nullptr, &how, &opt,
                    &st, ws ? ws->ws.get() : nullptr);
    if (status)
      *status = how;
    if (hist_ar)
      std::copy(har.begin(), har.end(), hist_ar);
    copy_out(hr, hist_r, st, spmv_ms_total, spmv_launches);
  });
}

// ---- LOBPCG -----------------------------------------------------------------------------
int spmvh_lobpcg_workspace_create(spmvh_exec* exec, spmvh_lobpcg_workspace** ws)
{
  return workspace_create<LobpcgWorkspace>(exec, ws);
}

int spmvh_lobpcg_workspace_destroy(spmvh_lobpcg_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_lobpcg_workspace_reserve_timing(spmvh_lobpcg_workspace* ws,
                                          int iterations)
{
  return workspace_reserve_timing(ws, iterations);
}

int spmvh_lobpcg_check_rules(int nev, int kmax, double rtol, double atol,
                             int has_dinv, int has_sgs, int has_amg,
                             int64_t sgs_rows, int64_t sgs_negative_pivots,
                             int64_t amg_rows, int64_t rows)
{
  return guarded([&] {
    lobpcg_check_rules(nev, kmax, rtol, atol, has_dinv != 0, has_sgs != 0,
                       has_amg != 0, sgs_rows, sgs_negative_pivots, amg_rows,
                       rows);
  });
}

int spmvh_lobpcg_check_pencil(int64_t rows_a, int64_t rows_b,
                              const int64_t* ghosts_a, int64_t num_ghosts_a,
                              const int64_t* ghosts_b, int64_t num_ghosts_b)
{
  return guarded([&] {
    require((ghosts_a || num_ghosts_a <= 0) && (ghosts_b || num_ghosts_b <= 0),
            "NULL argument");
    lobpcg_check_pencil(rows_a, rows_b, ghosts_a, num_ghosts_a, ghosts_b,
                        num_ghosts_b);
  });
}

int spmvh_lobpcg(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A, double* X,
                 int nev, const double* dinv, spmvh_sgs* sgs, spmvh_amg* amg,
                 int kmax, double rtol, double atol, int* num_its, int* status,
                 double* eigenvalues, double* resnorm_history,
                 double* true_resnorm, int* restarts, spmvh_lobpcg_workspace* ws,
                 int flags, double* spmv_ms_total, int* spmv_launches)
{
  return spmvh_lobpcg_gen(comm, exec, A, nullptr, X, nev, dinv, sgs, amg, kmax,
                          rtol, atol, num_its, status, eigenvalues,
                          resnorm_history, true_resnorm, restarts, ws, flags,
                          spmv_ms_total, spmv_launches);
}

int spmvh_lobpcg_gen(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                     spmvh_matrix* B, double* X, int nev, const double* dinv,
                     spmvh_sgs* sgs, spmvh_amg* amg, int kmax, double rtol,
                     double atol, int* num_its, int* status, double* eigenvalues,
                     double* resnorm_history, double* true_resnorm,
                     int* restarts, spmvh_lobpcg_workspace* ws, int flags,
                     double* spmv_ms_total, int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<double> eig, hist;
    LobpcgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    opt.largest = (flags & 2) != 0;
    if ((flags >> 8) & 0xff) // bits 8-15: poll_every (0 = default)
      opt.poll_every = (flags >> 8) & 0xff;
    LobpcgStats st;
    BlockPreconditioner pre;
    pre.dinv = dinv;
    pre.sgs = sgs ? sgs->M.get() : nullptr;
    pre.amg = amg ? amg->M.get() : nullptr;
    int how = 0;
    *num_its = lobpcg(*comm->comm, *exec->hip, *A->A, X, nev, pre, kmax, rtol,
                      atol, &eig, resnorm_history ? &hist : nullptr, &how, &opt,
                      &st, ws ? ws->ws.get() : nullptr,
                      B ? B->A.get() : nullptr);
    if (status)
      *status = how;
    if (eigenvalues)
      std::copy(eig.begin(), eig.end(), eigenvalues);
    if (true_resnorm)
      std::copy(st.true_resnorm.begin(), st.true_resnorm.end(), true_resnorm);
    if (restarts)
      *restarts = st.restarts;
    copy_out(hist, resnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

// ---- multi-shift CG ---------------------------------------------------------------------
int spmvh_cgs_workspace_create(spmvh_exec* exec, spmvh_cgs_workspace** ws)
{
  return workspace_create<CgShiftedWorkspace>(exec, ws);
}

int spmvh_cgs_workspace_destroy(spmvh_cgs_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_cgs_workspace_reserve_timing(spmvh_cgs_workspace* ws, int iterations)
{
  return workspace_reserve_timing(ws, iterations);
}

int spmvh_cgs_check_rules(int ns, int kmax, int64_t rows, int64_t ldx,
                          const double* shifts, const double* b, const double* X)
{
  return guarded([&] { cgs_check_rules(ns, kmax, rows, ldx, shifts, b, X); });
}

int spmvh_cg_shifted(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
                     const double* b, double* X, int64_t ldx,
                     const double* shifts, int ns, int kmax, double rtol,
                     int* num_its, int* iterations, double* rnorm_history,
                     int* status, spmvh_cgs_workspace* ws, int flags,
                     double* spmv_ms_total, int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<int> its;
    std::vector<double> hist;
    CgOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    if ((flags >> 8) & 0xff) // bits 8-15: CgOptions::poll_every (0 = default)
      opt.poll_every = (flags >> 8) & 0xff;
    CgStats st;
    int how = 0;
    *num_its = cg_shifted(*comm->comm, *exec->hip, *A->A, b, X, ldx, shifts, ns,
                          kmax, rtol, iterations ? &its : nullptr,
                          rnorm_history ? &hist : nullptr, &how, &opt, &st,
                          ws ? ws->ws.get() : nullptr);
    if (status)
      *status = how;
    if (iterations)
      std::copy(its.begin(), its.end(), iterations);
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

// ---- IDR(s) -----------------------------------------------------------------------------
int spmvh_idrs_workspace_create(spmvh_exec* exec, spmvh_idrs_workspace** ws)
{
  return workspace_create<IdrsWorkspace>(exec, ws);
}

int spmvh_idrs_workspace_destroy(spmvh_idrs_workspace* ws)
{
  return guarded([&] { delete ws; });
}

int spmvh_idrs_workspace_reserve_timing(spmvh_idrs_workspace* ws, int iterations)
{
  return workspace_reserve_timing(ws, iterations);
}

int spmvh_idrs_check_rules(int s, int kmax, double kappa, int has_dinv,
                           int cheb_degree, double lmin, double lmax,
                           int has_sgs, int has_amg, int64_t pre_rows,
                           int64_t rows, const double* b, const double* x,
                           const double* dinv)
{
  return guarded([&] {
    idrs_check_rules(s, kmax, kappa, has_dinv != 0, cheb_degree, lmin, lmax,
                     has_sgs != 0, has_amg != 0, pre_rows, rows, b, x, dinv);
  });
}

int spmvh_idrs(spmvh_comm* comm, spmvh_exec* exec, spmvh_matrix* A,
               const double* b, double* x, const double* dinv, int cheb_degree,
               double lmin, double lmax, spmvh_sgs* sgs, spmvh_amg* amg, int s,
               int kmax, double rtol, double kappa, uint64_t seed, int* num_its,
               int* status, double* rnorm_history, spmvh_idrs_workspace* ws,
               int flags, double* spmv_ms_total, int* spmv_launches)
{
  return guarded([&] {
    require(comm && exec && A && num_its, "NULL argument");
    std::vector<double> hist;
    IdrsOptions opt;
    opt.time_spmv = (flags & 1) != 0;
    if ((flags >> 8) & 0xff) // bits 8-15: poll_every (0 = default)
      opt.poll_every = (flags >> 8) & 0xff;
    opt.kappa = kappa;
    opt.seed = seed;
    GmresPreconditioner pre;
    pre.dinv = dinv;
    pre.cheb_degree = cheb_degree;
    pre.lmin = lmin;
    pre.lmax = lmax;
    pre.sgs = sgs ? sgs->M.get() : nullptr;
    pre.amg = amg ? amg->M.get() : nullptr;
    CgStats st;
    int how = 0;
    *num_its = idrs(*comm->comm, *exec->hip, *A->A, b, x, &pre, s, kmax, rtol,
                    rnorm_history ? &hist : nullptr, &opt, &st,
                    ws ? ws->ws.get() : nullptr, &how);
    if (status)
      *status = how;
    copy_out(hist, rnorm_history, st, spmv_ms_total, spmv_launches);
  });
}

} // extern "C"
