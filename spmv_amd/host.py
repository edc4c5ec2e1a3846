"""ctypes handles over the C facade (include/spmv_host_c.h) of the C++17 host
mirror: spmv::HipExecutor, L2GMap, Matrix<double>, cg.

Harness plumbing for tests/ and bench.py.  Method names follow the C++
classes so the parity tests read like the reference's tests/test_spmv.cpp.
Nothing here computes.
"""
import ctypes as C

import numpy as np

from . import _lib

P2P_BLOCKING, P2P_NONBLOCKING, COLLECTIVE_BLOCKING, COLLECTIVE_NONBLOCKING = 0, 1, 2, 3
ONESIDED_PUT_ACTIVE, ONESIDED_PUT_PASSIVE, SHMEM, SHMEM_NODUP = 4, 5, 6, 7

lib = _lib._load("libspmv_host.so")
lib.spmvh_last_error.restype = C.c_char_p

vp, i32, i64, f64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_size_t
PTR = C.POINTER

ALLGATHER_FN = C.CFUNCTYPE(C.c_int, vp, vp, vp, sz)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, vp, sz, C.c_int, PTR(C.c_int), vp,
                          PTR(i32), PTR(i32), vp, PTR(i32), PTR(i32), vp)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, vp, vp, sz, vp)

_PROTOS = {
    "spmvh_exec_create": [C.c_int, PTR(vp)],
    "spmvh_exec_destroy": [vp],
    "spmvh_exec_alloc": [vp, sz, PTR(vp)],
    "spmvh_exec_free": [vp, vp],
    "spmvh_exec_memset": [vp, vp, C.c_int, sz],
    "spmvh_exec_copy": [vp, vp, vp, sz],
    "spmvh_exec_copy_from_host": [vp, vp, vp, sz],
    "spmvh_exec_copy_to_host": [vp, vp, vp, sz],
    "spmvh_exec_synchronize": [vp],
    "spmvh_exec_num_cus": [vp, PTR(C.c_int)],
    "spmvh_exec_device_type": [vp, PTR(C.c_int)],
    "spmvh_exec_context": [vp, PTR(vp)],
    "spmvh_host_executor_rejects_compute": [],
    "spmvh_comm_self": [PTR(vp)],
    "spmvh_rccl_unique_id": [vp],
    "spmvh_comm_rccl": [vp, C.c_int, C.c_int, vp, PTR(vp)],
    "spmvh_comm_rccl_info": [vp, PTR(C.c_int), C.c_char_p, C.c_int],
    "spmvh_comm_callback": [C.c_int, C.c_int, ALLGATHER_FN, EXCHANGE_FN,
                            ALLREDUCE_FN, vp, PTR(vp)],
    "spmvh_comm_destroy": [vp],
    "spmvh_comm_enable_peer_reduce": [vp, vp, PTR(C.c_int)],
    "spmvh_comm_reduce_sum": [vp, vp, C.c_int, vp],
    "spmvh_comm_ranks_share_a_process": [vp, PTR(C.c_int)],
    "spmvh_matrix_create": [vp, vp, vp, vp, vp, i64, i64, vp, i64, vp, i64,
                            C.c_int, C.c_int, PTR(vp)],
    "spmvh_matrix_f32_create": [vp, vp, vp, vp, vp, i64, i64, vp, i64, vp, i64,
                                C.c_int, C.c_int, PTR(vp)],
    "spmvh_matrix_f32_destroy": [vp],
    "spmvh_matrix_f32_info": [vp, PTR(C.c_int), PTR(i64), PTR(i32), PTR(i32)],
    "spmvh_matrix_f32_update": [vp, vp],
    "spmvh_matrix_f32_mult": [vp, vp, vp],
    "spmvh_split_create_dist": [vp, vp, vp, vp, i64, i64, vp, i64, vp, i64,
                                C.c_int, C.c_int, PTR(vp), PTR(i64)],
    "spmvh_matrix_release_csr": [vp, PTR(i64)],
    "spmvh_matrix_create_poisson3d": [vp, vp, i32, C.c_int, C.c_int, PTR(vp)],
    "spmvh_matrix_create_unstructured": [vp, vp, i64, C.c_int, i64, C.c_int,
                                         C.c_uint64, PTR(vp)],
    "spmvh_matrix_create_fem_like": [vp, vp, vp, PTR(vp)],
    "spmvh_matrix_create_fem_like_sym": [vp, vp, vp, PTR(vp)],
    "spmvh_matrix_create_poisson3d_boxes": [vp, vp, i32, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_int, PTR(vp)],
    "spmvh_poisson3d_box_rows": [i32, C.c_int, C.c_int, C.c_int, C.c_int, vp,
                                 vp, vp, vp, vp],
    "spmvh_matrix_destroy": [vp],
    "spmvh_matrix_rows": [vp, PTR(C.c_int)],
    "spmvh_matrix_cols": [vp, PTR(C.c_int)],
    "spmvh_matrix_non_zeros": [vp, PTR(i64)],
    "spmvh_matrix_format_size": [vp, PTR(sz)],
    "spmvh_matrix_symmetric": [vp, PTR(C.c_int)],
    "spmvh_matrix_blocks": [vp, PTR(i64)],
    "spmvh_matrix_plan_get": [vp, C.c_int, C.c_char_p, PTR(C.c_int)],
    "spmvh_matrix_plan_set": [vp, C.c_int, C.c_char_p, C.c_int],
    "spmvh_matrix_enable_mixed": [vp, PTR(C.c_int)],
    "spmvh_matrix_use_mixed": [vp, C.c_int],
    "spmvh_matrix_update": [vp, vp],
    "spmvh_matrix_update_finalise": [vp, vp],
    "spmvh_matrix_mult": [vp, vp, vp],
    "spmvh_matrix_transpmult": [vp, vp, vp],
    "spmvh_matrix_enable_transpose": [vp],
    "spmvh_matrix_f32_transpmult": [vp, vp, vp],
    "spmvh_matrix_mult_block": [vp, vp, vp, C.c_int],
    "spmvh_matrix_update_block": [vp, vp, C.c_int],
    "spmvh_matrix_update_finalise_block": [vp, vp, C.c_int],
    "spmvh_matrix_f32_mult_block": [vp, vp, vp, C.c_int],
    "spmvh_matrix_f32_update_block": [vp, vp, C.c_int],
    "spmvh_matrix_f32_update_finalise_block": [vp, vp, C.c_int],
    "spmvh_l2gmap_update_block": [vp, vp, C.c_int],
    "spmvh_l2gmap_update_finalise_block": [vp, vp, C.c_int],
    "spmvh_split_create": [vp, vp, vp, i64, i64, i64, i64, vp, i64, C.c_int,
                           C.c_int, PTR(vp), PTR(i64)],
    "spmvh_split_get": [vp, C.c_int, vp, vp, vp],
    "spmvh_split_extra": [vp, vp, vp],
    "spmvh_split_destroy": [vp],
    "spmvh_l2g_sizes": [vp, PTR(i32), PTR(i32), PTR(i64), PTR(i64),
                        PTR(C.c_int), PTR(C.c_int), PTR(C.c_int), PTR(C.c_int)],
    "spmvh_l2g_ghosts": [vp, vp],
    "spmvh_l2g_onesided": [vp, vp],
    "spmvh_l2g_plan": [vp, vp, vp, vp, vp, vp, vp],
    "spmvh_l2g_global_to_local": [vp, i64, PTR(i32)],
    "spmvh_l2g_create": [vp, vp, C.c_int, i64, vp, i64, C.c_int, PTR(vp)],
    "spmvh_l2g_destroy": [vp],
    "spmvh_l2g_map_sizes": [vp, PTR(C.c_int), PTR(C.c_int), PTR(C.c_int)],
    "spmvh_l2g_map_plan": [vp, vp, vp, vp, vp, vp, vp],
    "spmvh_l2g_map_update": [vp, vp],
    "spmvh_l2g_map_reverse_update": [vp, vp],
    "spmvh_l2g_map_reverse_update_f32": [vp, vp],
    "spmvh_cg": [vp, vp, vp, vp, vp, C.c_int, f64, PTR(C.c_int), vp],
    "spmvh_read_petsc_matrix": [vp, vp, C.c_char_p, C.c_int, C.c_int, PTR(vp)],
    "spmvh_read_petsc_vector": [vp, vp, C.c_char_p, PTR(vp), PTR(i64)],
    "spmvh_petsc_rows_read": [C.c_char_p, C.c_int, C.c_int, PTR(vp), PTR(i64)],
    "spmvh_petsc_rows_get": [vp, vp, vp, vp, vp],
    "spmvh_petsc_rows_destroy": [vp],
    "spmvh_cg_workspace_create": [vp, PTR(vp)],
    "spmvh_cg_workspace_destroy": [vp],
    "spmvh_cg_mixed": [vp, vp, vp, vp, vp, C.c_int, C.c_double, C.c_int,
                       PTR(C.c_int), vp, C.c_int, vp, C.c_int,
                       PTR(C.c_double)],
    "spmvh_cg_workspace_reserve_timing": [vp, C.c_int],
    "spmvh_cg_ex": [vp, vp, vp, vp, vp, C.c_int, f64, PTR(C.c_int), vp, vp,
                    C.c_int, PTR(f64), PTR(C.c_int)],
    "spmvh_cg_block_workspace_create": [vp, PTR(vp)],
    "spmvh_cg_block_workspace_destroy": [vp],
    "spmvh_cg_block": [vp, vp, vp, vp, vp, C.c_int, C.c_int, f64, PTR(C.c_int),
                       vp, vp, vp, C.c_int, PTR(f64), PTR(C.c_int)],
    "spmvh_matrix_diagonal": [vp, vp],
    "spmvh_jacobi_inverse": [vp, vp, vp, i64],
    "spmvh_pcg_workspace_create": [vp, PTR(vp)],
    "spmvh_pcg_workspace_destroy": [vp],
    "spmvh_pcg_workspace_reserve_timing": [vp, C.c_int],
    "spmvh_pcg": [vp, vp, vp, vp, vp, vp, C.c_int, f64, PTR(C.c_int), vp, vp,
                  C.c_int, PTR(f64), PTR(C.c_int)],
    "spmvh_chebyshev_coefficients": [C.c_int, f64, f64, vp, vp],
    "spmvh_chebyshev_workspace_create": [vp, PTR(vp)],
    "spmvh_chebyshev_workspace_destroy": [vp],
    "spmvh_chebyshev_workspace_reserve_timing": [vp, C.c_int],
    "spmvh_chebyshev_apply": [vp, vp, vp, vp, vp, C.c_int, f64, f64, vp],
    "spmvh_pcg_chebyshev": [vp, vp, vp, vp, vp, vp, C.c_int, f64, f64, C.c_int,
                            f64, PTR(C.c_int), vp, vp, C.c_int, PTR(f64),
                            PTR(C.c_int)],
    "spmvh_lambda_max_estimate": [vp, vp, vp, vp, vp, C.c_int, PTR(f64)],
    "spmvh_sgs_color": [vp, vp, i64, i64, C.c_int, vp, PTR(C.c_int)],
    "spmvh_sgs_build_create": [vp, vp, vp, i64, i64, C.c_int, PTR(vp), vp],
    "spmvh_sgs_build_get": [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "spmvh_sgs_build_destroy": [vp],
    "spmvh_sgs_create": [vp, vp, PTR(vp)],
    "spmvh_sgs_create_ex": [vp, vp, C.c_int, C.c_int, vp, PTR(vp)],
    "spmvh_sgs_create_ex2": [vp, vp, C.c_int, C.c_int, vp, C.c_int, PTR(vp)],
    "spmvh_sgs_value_bits": [vp, PTR(C.c_int)],
    "spmvh_fp32_range_count": [vp, i64, PTR(i64)],
    "spmvh_sgs_setup_info": [vp, PTR(C.c_int), PTR(f64)],
    "spmvh_sgs_setup_detail": [vp, PTR(f64), PTR(f64), PTR(i64)],
    "spmvh_sgs_export_sizes": [vp, vp],
    "spmvh_sgs_export": [vp, vp, vp, vp, vp, vp],
    "spmvh_sgs_destroy": [vp],
    "spmvh_sgs_info": [vp, PTR(C.c_int), PTR(C.c_int), PTR(i64)],
    "spmvh_sgs_colors": [vp, vp],
    "spmvh_sgs_apply": [vp, vp, vp, vp],
    "spmvh_sgs_apply_block": [vp, vp, vp, vp, C.c_int],
    "spmvh_pcg_block_workspace_create": [vp, PTR(vp)],
    "spmvh_pcg_block_workspace_destroy": [vp],
    "spmvh_pcg_block_check_arguments": [C.c_int, C.c_int, C.c_int, C.c_int, i64,
                                        i64, i64, vp, vp, vp],
    "spmvh_pcg_block": [vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, f64,
                        PTR(C.c_int), vp, vp, vp, C.c_int, PTR(f64),
                        PTR(C.c_int)],
    "spmvh_matrix_local_values": [vp, PTR(vp), PTR(vp)],
    "spmvh_matrix_plan_values_changed": [vp],
    "spmvh_ilu0_symbolic_create": [vp, vp, i64, i64, C.c_int, PTR(vp), vp],
    "spmvh_ilu0_symbolic_get": [vp] * 17,
    "spmvh_ilu0_symbolic_destroy": [vp],
    "spmvh_ilu0_create": [vp, vp, PTR(vp)],
    "spmvh_ilu0_refactor": [vp, vp],
    "spmvh_ilu0_info": [vp, vp],
    "spmvh_ilu0_pattern": [vp, vp, vp, vp, vp],
    "spmvh_ilu0_factor": [vp, vp, vp, vp],
    "spmvh_ilu0_create_ex": [vp, vp, C.c_int, C.c_int, vp, PTR(vp)],
    "spmvh_ilu0_create_ex2": [vp, vp, C.c_int, C.c_int, vp, C.c_int, PTR(vp)],
    "spmvh_ilu0_export_sizes": [vp, vp],
    "spmvh_ilu0_export": [vp, vp, vp],
    "spmvh_amg_check_options": [f64, C.c_int, i64, C.c_int, C.c_int, f64, f64],
    "spmvh_amg_symbolic_create": [vp, vp, vp, vp, i64, i64, C.c_int, f64,
                                  PTR(vp), vp],
    "spmvh_amg_symbolic_get": [vp] * 11,
    "spmvh_amg_symbolic_destroy": [vp],
    "spmvh_amg_create": [vp, vp, vp, PTR(vp)],
    "spmvh_amg_create_ex": [vp, vp, vp, C.c_int, C.c_int, PTR(vp)],
    "spmvh_amg_setup_info": [vp, vp],
    "spmvh_amg_level_rounds": [vp, C.c_int, vp],
    "spmvh_amg_step_sizes": [vp, C.c_int, vp],
    "spmvh_amg_step_export": [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp],
    "spmvh_amg_destroy": [vp],
    "spmvh_amg_refresh": [vp, vp],
    "spmvh_amg_info": [vp, vp],
    "spmvh_amg_level_info": [vp, C.c_int, vp, PTR(f64)],
    "spmvh_amg_aggregates": [vp, C.c_int, vp],
    "spmvh_amg_level_matrix": [vp, C.c_int, vp, vp, vp],
    "spmvh_amg_apply": [vp, vp, vp, vp],
    "spmvh_amg_apply_block": [vp, vp, vp, vp, C.c_int],
    "spmvh_amg_apply_block_check_arguments": [C.c_int, i64, vp, vp],
    "spmvh_amg_release_block_scratch": [vp],
    "spmvh_pcg_block_amg": [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, f64,
                            PTR(C.c_int), vp, vp, vp, C.c_int, PTR(f64),
                            PTR(C.c_int)],
    "spmvh_pcg_block_amg_check_arguments": [C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, i64, i64, i64, i64, vp, vp,
                                            vp],
    "spmvh_amg_check_tail_rows": [i64],
    "spmvh_amg_set_tail_rows": [vp, i64],
    "spmvh_amg_tail_levels": [vp, PTR(C.c_int)],
    "spmvh_amg_tail_lanes": [vp, C.c_int, PTR(C.c_int)],
    "spmvh_pcg_amg": [vp, vp, vp, vp, vp, vp, C.c_int, f64, PTR(C.c_int), vp, vp,
                      C.c_int, PTR(f64), PTR(C.c_int)],
    "spmvh_gmres_amg": [vp, vp, vp, vp, vp, vp, C.c_int, f64, f64, vp, C.c_int,
                        C.c_int, f64, PTR(C.c_int), PTR(C.c_int), vp, vp,
                        C.c_int, PTR(f64), PTR(C.c_int), vp],
    "spmvh_sgs_workspace_create": [vp, PTR(vp)],
    "spmvh_sgs_workspace_destroy": [vp],
    "spmvh_sgs_workspace_reserve_timing": [vp, C.c_int],
    "spmvh_pcg_sgs": [vp, vp, vp, vp, vp, vp, C.c_int, f64, PTR(C.c_int), vp, vp,
                      C.c_int, PTR(f64), PTR(C.c_int)],
    "spmvh_bicgstab_workspace_create": [vp, PTR(vp)],
    "spmvh_bicgstab_workspace_destroy": [vp],
    "spmvh_bicgstab_workspace_reserve_timing": [vp, C.c_int],
    "spmvh_minres_workspace_create": [vp, PTR(vp)],
    "spmvh_minres_workspace_destroy": [vp],
    "spmvh_minres_workspace_reserve_timing": [vp, C.c_int],
    "spmvh_minres_check_rules": [C.c_int, C.c_int, C.c_int, C.c_int, i64, i64,
                                 i64, i64, vp, vp, vp],
    "spmvh_minres": [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, f64, PTR(C.c_int),
                     PTR(C.c_int), vp, vp, C.c_int, PTR(f64), PTR(C.c_int)],
    "spmvh_lobpcg_workspace_create": [vp, PTR(vp)],
    "spmvh_lobpcg_workspace_destroy": [vp],
    "spmvh_lobpcg_workspace_reserve_timing": [vp, C.c_int],
    "spmvh_lobpcg_check_rules": [C.c_int, C.c_int, f64, f64, C.c_int, C.c_int,
                                 C.c_int, i64, i64, i64, i64],
    "spmvh_lobpcg": [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, f64, f64,
                     PTR(C.c_int), PTR(C.c_int), vp, vp, vp, PTR(C.c_int), vp,
                     C.c_int, PTR(f64), PTR(C.c_int)],
    "spmvh_lobpcg_check_pencil": [i64, i64, vp, i64, vp, i64],
    "spmvh_lobpcg_gen": [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, f64,
                         f64, PTR(C.c_int), PTR(C.c_int), vp, vp, vp,
                         PTR(C.c_int), vp, C.c_int, PTR(f64), PTR(C.c_int)],
    "spmvh_lsqr_workspace_create": [vp, PTR(vp)],
    "spmvh_lsqr_workspace_destroy": [vp],
    "spmvh_lsqr_workspace_reserve_timing": [vp, C.c_int],
    "spmvh_lsqr_check_rules": [C.c_int, f64, f64, i64, i64, vp, vp],
    "spmvh_lsqr": [vp, vp, vp, vp, vp, C.c_int, f64, f64, f64, PTR(C.c_int),
                   PTR(C.c_int), vp, vp, vp, C.c_int, PTR(f64), PTR(C.c_int)],
    "spmvh_cgs_workspace_create": [vp, PTR(vp)],
    "spmvh_cgs_workspace_destroy": [vp],
    "spmvh_cgs_workspace_reserve_timing": [vp, C.c_int],
    "spmvh_cgs_check_rules": [C.c_int, C.c_int, i64, i64, vp, vp, vp],
    "spmvh_cg_shifted": [vp, vp, vp, vp, vp, i64, vp, C.c_int, C.c_int, f64,
                         PTR(C.c_int), vp, vp, PTR(C.c_int), vp, C.c_int,
                         PTR(f64), PTR(C.c_int)],
    "spmvh_idrs_workspace_create": [vp, PTR(vp)],
    "spmvh_idrs_workspace_destroy": [vp],
    "spmvh_idrs_workspace_reserve_timing": [vp, C.c_int],
    "spmvh_idrs_check_rules": [C.c_int, C.c_int, f64, C.c_int, C.c_int, f64, f64,
                               C.c_int, C.c_int, i64, i64, vp, vp, vp],
    "spmvh_idrs": [vp, vp, vp, vp, vp, vp, C.c_int, f64, f64, vp, vp, C.c_int,
                   C.c_int, f64, f64, C.c_uint64, PTR(C.c_int), PTR(C.c_int), vp,
                   vp, C.c_int, PTR(f64), PTR(C.c_int)],
    "spmvh_gmres_workspace_create": [vp, PTR(vp)],
    "spmvh_gmres_workspace_destroy": [vp],
    "spmvh_gmres_workspace_reserve_timing": [vp, C.c_int],
    "spmvh_gmres_check_arguments": [C.c_int, C.c_int, C.c_int, f64, f64],
    "spmvh_gmres": [vp, vp, vp, vp, vp, vp, C.c_int, f64, f64, vp, C.c_int,
                    C.c_int, f64, PTR(C.c_int), PTR(C.c_int), vp, vp, C.c_int,
                    PTR(f64), PTR(C.c_int)],
    "spmvh_bicgstab": [vp, vp, vp, vp, vp, vp, C.c_int, f64, PTR(C.c_int),
                       PTR(C.c_int), vp, vp, C.c_int, PTR(f64), PTR(C.c_int)],
}
for _n, _a in _PROTOS.items():
    _f = getattr(lib, _n)
    _f.argtypes = _a
    _f.restype = C.c_int
HOST_SYMBOLS = tuple(_PROTOS) + ("spmvh_last_error",)


class FemParams(C.Structure):
    """spmv_hip_fem_params (include/spmv_hip.h)"""
    _fields_ = [("num_rows", C.c_int64), ("min_len", C.c_int32),
                ("max_len", C.c_int32), ("layer", C.c_int32),
                ("jitter", C.c_int32), ("tail_permille", C.c_int32),
                ("tail_min", C.c_int32), ("tail_max", C.c_int32),
                ("tail_stride", C.c_int32), ("seed", C.c_uint64)]


class SpmvHostError(RuntimeError):
    pass


def call(name, *args):
    if getattr(lib, name)(*args) != 0:
        raise SpmvHostError(f"{name}: {lib.spmvh_last_error().decode()}")


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HipExecutor:
    """spmv::HipExecutor::create(device_id, HostExecutor::create())"""

    def __init__(self, device_id=0):
        h = vp()
        call("spmvh_exec_create", device_id, C.byref(h))
        self.h = h

    def close(self):
        if self.h:
            call("spmvh_exec_destroy", self.h)
            self.h = None

    def alloc(self, count, dtype=np.float64):
        p = vp()
        call("spmvh_exec_alloc", self.h, int(count) * np.dtype(dtype).itemsize,
             C.byref(p))
        return p.value or 0

    def free(self, ptr):
        call("spmvh_exec_free", self.h, ptr)

    def memset(self, ptr, value, nbytes):
        call("spmvh_exec_memset", self.h, ptr, value, nbytes)

    def copy(self, dst, src, nbytes):
        call("spmvh_exec_copy", self.h, dst, src, nbytes)

    def copy_from_host(self, dst, arr):
        arr = np.ascontiguousarray(arr)
        call("spmvh_exec_copy_from_host", self.h, dst, _np_ptr(arr), arr.nbytes)

    def copy_to_host(self, src, count, dtype=np.float64):
        out = np.empty(count, dtype)
        call("spmvh_exec_copy_to_host", self.h, _np_ptr(out), src, out.nbytes)
        return out

    def synchronize(self):
        call("spmvh_exec_synchronize", self.h)

    @property
    def num_cus(self):
        n = C.c_int()
        call("spmvh_exec_num_cus", self.h, C.byref(n))
        return n.value

    @property
    def device_type(self):
        t = C.c_int()
        call("spmvh_exec_device_type", self.h, C.byref(t))
        return t.value

    @property
    def context(self):
        """spmv_hip_ctx* behind the executor (timing events in bench.py)."""
        c = vp()
        call("spmvh_exec_context", self.h, C.byref(c))
        return c


class Comm:
    def __init__(self, h, keep=()):
        self.h, self._keep = h, keep

    @classmethod
    def self_comm(cls):
        h = vp()
        call("spmvh_comm_self", C.byref(h))
        return cls(h)

    @classmethod
    def rccl(cls, exec_, nranks, rank, unique_id):
        h = vp()
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
        call("spmvh_comm_rccl", exec_.h, nranks, rank, buf, C.byref(h))
        return cls(h)

    def rccl_info(self):
        """{nranks, rank, version, separate_reduction_comm, lib_path} as RCCL
        itself reports them"""
        out = (C.c_int * 4)()
        path = C.create_string_buffer(512)
        call("spmvh_comm_rccl_info", self.h, out, path, 512)
        v = out[2]
        return dict(nranks=out[0], rank=out[1], version_code=v,
                    version=f"{v // 10000}.{v // 100 % 100}.{v % 100}",
                    separate_reduction_comm=bool(out[3]),
                    lib_path=path.value.decode())

    @classmethod
    def callback(cls, rank, nranks, allgather, exchange=None, allreduce=None):
        """Transport supplied as Python callables (see spmv_host_c.h)."""
        ag = ALLGATHER_FN(allgather)
        ex = EXCHANGE_FN(exchange) if exchange else EXCHANGE_FN()
        ar = ALLREDUCE_FN(allreduce) if allreduce else ALLREDUCE_FN()
        h = vp()
        call("spmvh_comm_callback", rank, nranks, ag, ex, ar, None, C.byref(h))
        return cls(h, keep=(ag, ex, ar))

    def enable_peer_reduce(self, exec_):
        """Comm::enable_peer_reduce (collective): cg() then reduces its scalars
        through peer windows, added in rank order; False = not available."""
        ok = C.c_int()
        call("spmvh_comm_enable_peer_reduce", self.h, exec_.h, C.byref(ok))
        return bool(ok.value)

    def reduce_sum(self, device_ptr, count=1, stream=None):
        call("spmvh_comm_reduce_sum", self.h, device_ptr, int(count), stream)

    def ranks_share_a_process(self):
        """Comm::ranks_share_a_process (collective on its first call)"""
        v = C.c_int()
        call("spmvh_comm_ranks_share_a_process", self.h, C.byref(v))
        return bool(v.value)

    def close(self):
        if self.h:
            call("spmvh_comm_destroy", self.h)
            self.h = None


def rccl_unique_id():
    buf = (C.c_ubyte * 128)()
    call("spmvh_rccl_unique_id", buf)
    return bytes(buf)


class L2GPlanView:
    """Plan arrays of an L2GMap (reference member names, no underscore)."""

    def __init__(self, nn, ni, getter):
        self.neighbours = np.zeros(nn, np.int32)
        self.send_count = np.zeros(max(nn, 1), np.int32)
        self.recv_count = np.zeros(max(nn, 1), np.int32)
        self.send_offset = np.zeros(max(nn, 1) + 1, np.int32)
        self.recv_offset = np.zeros(max(nn, 1) + 1, np.int32)
        self.indexbuf = np.zeros(ni, np.int32)
        getter(_np_ptr(self.neighbours), _np_ptr(self.send_count),
               _np_ptr(self.recv_count), _np_ptr(self.send_offset),
               _np_ptr(self.recv_offset), _np_ptr(self.indexbuf))
        self.send_count = self.send_count[:nn]
        self.recv_count = self.recv_count[:nn]
        self.send_offset = self.send_offset[:nn + 1]
        self.recv_offset = self.recv_offset[:nn + 1]


class L2GMap:
    """Stand-alone spmv::L2GMap (plan tests)."""

    def __init__(self, comm, local_size, ghosts, exec_=None,
                 cm=COLLECTIVE_BLOCKING):
        g = np.ascontiguousarray(ghosts, dtype=np.int64)
        h = vp()
        call("spmvh_l2g_create", comm.h, exec_.h if exec_ else None,
             0 if exec_ else 1, int(local_size), _np_ptr(g), len(g), cm,
             C.byref(h))
        self.h = h

    def plan(self):
        nn, ni, packs = C.c_int(), C.c_int(), C.c_int()
        call("spmvh_l2g_map_sizes", self.h, C.byref(nn), C.byref(ni),
             C.byref(packs))
        v = L2GPlanView(nn.value, ni.value,
                        lambda *a: call("spmvh_l2g_map_plan", self.h, *a))
        v.packs = bool(packs.value)
        return v

    def update(self, x_ptr):
        call("spmvh_l2g_map_update", self.h, x_ptr)

    def update_block(self, x_ptr, k):
        """update() of a block of k interleaved fp64 vectors"""
        call("spmvh_l2gmap_update_block", self.h, x_ptr, int(k))

    def update_finalise_block(self, x_ptr, k):
        call("spmvh_l2gmap_update_finalise_block", self.h, x_ptr, int(k))

    def reverse_update(self, x_ptr, f32=False):
        call("spmvh_l2g_map_reverse_update_f32" if f32
             else "spmvh_l2g_map_reverse_update", self.h, x_ptr)

    def close(self):
        if self.h:
            call("spmvh_l2g_destroy", self.h)
            self.h = None


class ColMapView:
    """A.col_map() of a Matrix."""

    def __init__(self, A):
        self.A = A
        ls, ng, gs, go = i32(), i32(), i64(), i64()
        ov, nn, ni, pk = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        call("spmvh_l2g_sizes", A.h, C.byref(ls), C.byref(ng), C.byref(gs),
             C.byref(go), C.byref(ov), C.byref(nn), C.byref(ni), C.byref(pk))
        self._local_size, self._num_ghosts = ls.value, ng.value
        self._global_size, self._global_offset = gs.value, go.value
        self._overlapping, self._nn, self._ni = bool(ov.value), nn.value, ni.value
        self.packs = bool(pk.value)

    def local_size(self):
        return self._local_size

    def num_ghosts(self):
        return self._num_ghosts

    def global_size(self):
        return self._global_size

    def global_offset(self):
        return self._global_offset

    def overlapping(self):
        return self._overlapping

    def onesided(self):
        """the halo moves by peer stores (onesided_put_* models, > 1 rank)"""
        v = C.c_int()
        call("spmvh_l2g_onesided", self.A.h, C.byref(v))
        return bool(v.value)

    def ghosts(self):
        g = np.zeros(self._num_ghosts, np.int64)
        call("spmvh_l2g_ghosts", self.A.h, _np_ptr(g))
        return g

    def global_to_local(self, i):
        out = i32()
        call("spmvh_l2g_global_to_local", self.A.h, int(i), C.byref(out))
        return out.value

    def plan(self):
        return L2GPlanView(self._nn, self._ni,
                           lambda *a: call("spmvh_l2g_plan", self.A.h, *a))

    def update(self, x_ptr):
        call("spmvh_matrix_update", self.A.h, x_ptr)

    def update_finalise(self, x_ptr):
        call("spmvh_matrix_update_finalise", self.A.h, x_ptr)

    def update_block(self, x_ptr, k):
        """update() of a block of k interleaved vectors: element (i, c) at
        X[i * k + c], (local_size + num_ghosts) * k entries"""
        call("spmvh_matrix_update_block", self.A.h, x_ptr, int(k))

    def update_finalise_block(self, x_ptr, k):
        call("spmvh_matrix_update_finalise_block", self.A.h, x_ptr, int(k))


class Matrix:
    """spmv::Matrix<double>"""

    def __init__(self, h):
        self.h = h

    @classmethod
    def create_matrix(cls, comm, exec_, rowptr, colind, values, nrows_local,
                      ncols_local, row_ghosts, col_ghosts, symmetric=False,
                      cm=COLLECTIVE_BLOCKING):
        rp = np.ascontiguousarray(rowptr, np.int32)
        ci = np.ascontiguousarray(colind, np.int32)
        va = np.ascontiguousarray(values, np.float64)
        rg = np.ascontiguousarray(row_ghosts, np.int64)
        cg = np.ascontiguousarray(col_ghosts, np.int64)
        h = vp()
        call("spmvh_matrix_create", comm.h, exec_.h, _np_ptr(rp), _np_ptr(ci),
             _np_ptr(va), int(nrows_local), int(ncols_local), _np_ptr(rg),
             len(rg), _np_ptr(cg), len(cg), int(symmetric), cm, C.byref(h))
        return cls(h)

    @classmethod
    def create_poisson3d(cls, comm, exec_, n, symmetric=False,
                         cm=COLLECTIVE_BLOCKING):
        h = vp()
        call("spmvh_matrix_create_poisson3d", comm.h, exec_.h, n,
             int(symmetric), cm, C.byref(h))
        return cls(h)

    @classmethod
    def create_unstructured(cls, comm, exec_, nrows, per_row=7, band=2048,
                            far_permille=100, seed=0x5EED0003):
        """Seeded unstructured test matrix, generated on the device (one rank;
        numpy twin: spmv_amd.poisson.unstructured_csr)."""
        h = vp()
        call("spmvh_matrix_create_unstructured", comm.h, exec_.h, int(nrows),
             int(per_row), int(band), int(far_permille), int(seed), C.byref(h))
        return cls(h)

    @classmethod
    def create_fem_like(cls, comm, exec_, nrows, symmetric=False, **params):
        """Seeded FEM-like test matrix (ragged rows, optional tail of very long
        rows, bandwidth-reducing order), generated on the device (one rank;
        numpy twin and parameters: spmv_amd.poisson.fem_like_csr).  symmetric:
        its strictly lower part + diagonal in symmetric storage."""
        from .poisson import fem_params
        h = vp()
        p = FemParams(**fem_params(nrows, **params))
        call("spmvh_matrix_create_fem_like_sym" if symmetric
             else "spmvh_matrix_create_fem_like", comm.h, exec_.h, C.byref(p),
             C.byref(h))
        return cls(h)

    @classmethod
    def create_poisson3d_boxes(cls, comm, exec_, n, parts, symmetric=False,
                               cm=COLLECTIVE_BLOCKING):
        """The Poisson matrix on a 3-D block partition, parts = (px, py, pz)."""
        h = vp()
        call("spmvh_matrix_create_poisson3d_boxes", comm.h, exec_.h, n,
             int(parts[0]), int(parts[1]), int(parts[2]), int(symmetric), cm,
             C.byref(h))
        return cls(h)

    def close(self):
        if self.h:
            call("spmvh_matrix_destroy", self.h)
            self.h = None

    def release_csr(self):
        """CSRMatrix::release_csr on both blocks: frees the device copies of
        colind / values where the plan holds the matrix in its own format;
        returns the bytes given back (0: the plan still reads them)."""
        v = i64()
        call("spmvh_matrix_release_csr", self.h, C.byref(v))
        return v.value

    def rows(self):
        v = C.c_int()
        call("spmvh_matrix_rows", self.h, C.byref(v))
        return v.value

    def cols(self):
        v = C.c_int()
        call("spmvh_matrix_cols", self.h, C.byref(v))
        return v.value

    def non_zeros(self):
        v = i64()
        call("spmvh_matrix_non_zeros", self.h, C.byref(v))
        return v.value

    def format_size(self):
        v = sz()
        call("spmvh_matrix_format_size", self.h, C.byref(v))
        return v.value

    def symmetric(self):
        v = C.c_int()
        call("spmvh_matrix_symmetric", self.h, C.byref(v))
        return bool(v.value)

    def blocks(self):
        out = (i64 * 6)()
        call("spmvh_matrix_blocks", self.h, out)
        return dict(local=tuple(out[0:3]), remote=tuple(out[3:6]))

    def local_values(self):
        """-> (values_ptr, diagonal_ptr): device addresses of the local block's
        value array (blocks()["local"][2] doubles) and of its diagonal array
        (symmetric storage; None otherwise), for rewriting the coefficients in
        place on a fixed pattern; call plan_values_changed() afterwards (and
        Ilu0Preconditioner.refactor)"""
        v, d = vp(), vp()
        call("spmvh_matrix_local_values", self.h, C.byref(v), C.byref(d))
        return v.value, d.value

    def plan_values_changed(self):
        """Matrix::plan_values_changed: the arrays of local_values() were
        rewritten in place; every copy the SpMV plans keep is refreshed"""
        call("spmvh_matrix_plan_values_changed", self.h)

    def col_map(self):
        return ColMapView(self)

    def plan_get(self, key, remote=False):
        v = C.c_int()
        call("spmvh_matrix_plan_get", self.h, int(remote), key.encode(),
             C.byref(v))
        return v.value

    def enable_mixed(self):
        ok = C.c_int()
        call("spmvh_matrix_enable_mixed", self.h, C.byref(ok))
        return bool(ok.value)

    def use_mixed(self, on):
        call("spmvh_matrix_use_mixed", self.h, int(bool(on)))

    def plan_set(self, key, value, remote=False):
        call("spmvh_matrix_plan_set", self.h, int(remote), key.encode(),
             int(value))

    def mult(self, x_ptr, y_ptr):
        call("spmvh_matrix_mult", self.h, x_ptr, y_ptr)

    def mult_block(self, x_ptr, y_ptr, k):
        """Y = A X for k interleaved vectors (element (i, c) at X[i * k + c]): X
        holds (local_size + num_ghosts) * k entries, Y rows * k; column by
        column the bits of mult()."""
        call("spmvh_matrix_mult_block", self.h, x_ptr, y_ptr, int(k))

    def transpmult(self, b_ptr, y_ptr):
        """y = A^T b: b holds rows() entries, y local_size + num_ghosts (the
        ghost tail goes to its owners with col_map's reverse_update)."""
        call("spmvh_matrix_transpmult", self.h, b_ptr, y_ptr)

    def enable_transpose(self):
        """build the transposed maps now (before release_csr)"""
        call("spmvh_matrix_enable_transpose", self.h)

    def diagonal(self, d_ptr):
        """Matrix::diagonal: d (device, rows entries) = the diagonal of this
        rank's rows.  General storage: before release_csr only."""
        call("spmvh_matrix_diagonal", self.h, d_ptr)


class MatrixF32:
    """spmv::Matrix<float> (fp32 instantiation)"""

    def __init__(self, comm, exec_, rowptr, colind, values, nrows_local,
                 ncols_local, row_ghosts, col_ghosts, symmetric=False,
                 cm=COLLECTIVE_BLOCKING):
        rp = np.ascontiguousarray(rowptr, np.int32)
        ci = np.ascontiguousarray(colind, np.int32)
        va = np.ascontiguousarray(values, np.float32)
        rg = np.ascontiguousarray(row_ghosts, np.int64)
        cg = np.ascontiguousarray(col_ghosts, np.int64)
        h = vp()
        call("spmvh_matrix_f32_create", comm.h, exec_.h, _np_ptr(rp),
             _np_ptr(ci), _np_ptr(va), int(nrows_local), int(ncols_local),
             _np_ptr(rg), len(rg), _np_ptr(cg), len(cg), int(symmetric), cm,
             C.byref(h))
        self.h = h

    def info(self):
        rows, nnz, ls, ng = C.c_int(), i64(), i32(), i32()
        call("spmvh_matrix_f32_info", self.h, C.byref(rows), C.byref(nnz),
             C.byref(ls), C.byref(ng))
        return dict(rows=rows.value, nnz=nnz.value, local_size=ls.value,
                    num_ghosts=ng.value)

    def update(self, x_ptr):
        call("spmvh_matrix_f32_update", self.h, x_ptr)

    def mult(self, x_ptr, y_ptr):
        call("spmvh_matrix_f32_mult", self.h, x_ptr, y_ptr)

    def transpmult(self, b_ptr, y_ptr):
        call("spmvh_matrix_f32_transpmult", self.h, b_ptr, y_ptr)

    def mult_block(self, x_ptr, y_ptr, k):
        call("spmvh_matrix_f32_mult_block", self.h, x_ptr, y_ptr, int(k))

    def update_block(self, x_ptr, k):
        call("spmvh_matrix_f32_update_block", self.h, x_ptr, int(k))

    def update_finalise_block(self, x_ptr, k):
        call("spmvh_matrix_f32_update_finalise_block", self.h, x_ptr, int(k))

    def close(self):
        if self.h:
            call("spmvh_matrix_f32_destroy", self.h)
            self.h = None


def _split_result(h, sizes, nrows_local, symmetric):
    out = dict(nnz=sizes[7])
    for which, name in ((0, "local"), (1, "remote")):
        rows, cols, nnz = sizes[3 * which:3 * which + 3]
        brp = np.zeros(rows + 1, np.int32)
        bci = np.zeros(nnz, np.int32)
        bva = np.zeros(nnz, np.float64)
        call("spmvh_split_get", h, which, _np_ptr(brp), _np_ptr(bci),
             _np_ptr(bva))
        out[name] = (brp, bci, bva)
        out[name + "_cols"] = cols
    diag = np.zeros(nrows_local if symmetric else 0, np.float64)
    ghosts = np.zeros(sizes[6], np.int64)
    call("spmvh_split_extra", h, _np_ptr(diag) if symmetric else None,
         _np_ptr(ghosts))
    out["diagonal"] = diag if symmetric else None
    out["ghosts"] = ghosts
    call("spmvh_split_destroy", h)
    return out


def split_rows(rowptr, colind, values, nrows_local, ncols_local, row_offset,
               col_offset, col_ghosts, symmetric, cm):
    """Matrix<double>::split_rows: the host half of create_matrix (no GPU)."""
    rp = np.ascontiguousarray(rowptr, np.int32)
    ci = np.ascontiguousarray(colind, np.int32)
    va = np.ascontiguousarray(values, np.float64)
    cg = np.ascontiguousarray(col_ghosts, np.int64)
    h, sizes = vp(), (i64 * 8)()
    call("spmvh_split_create", _np_ptr(rp), _np_ptr(ci), _np_ptr(va),
         int(nrows_local), int(ncols_local), int(row_offset), int(col_offset),
         _np_ptr(cg), len(cg), int(symmetric), cm, C.byref(h), sizes)
    return _split_result(h, sizes, nrows_local, symmetric)


def split_rows_distributed(comm, rowptr, colind, values, nrows_local,
                           ncols_local, row_ghosts, col_ghosts, symmetric, cm):
    """Matrix<double>::split_rows_distributed: collective over `comm`, ships
    ghost rows to their owners (Matrix.cpp:188-292); no GPU."""
    rp = np.ascontiguousarray(rowptr, np.int32)
    ci = np.ascontiguousarray(colind, np.int32)
    va = np.ascontiguousarray(values, np.float64)
    rg = np.ascontiguousarray(row_ghosts, np.int64)
    cg = np.ascontiguousarray(col_ghosts, np.int64)
    h, sizes = vp(), (i64 * 8)()
    call("spmvh_split_create_dist", comm.h, _np_ptr(rp), _np_ptr(ci),
         _np_ptr(va), int(nrows_local), int(ncols_local), _np_ptr(rg), len(rg),
         _np_ptr(cg), len(cg), int(symmetric), cm, C.byref(h), sizes)
    return _split_result(h, sizes, nrows_local, symmetric)


def poisson3d_box_rows(n, parts, rank):
    """Host half of Matrix.create_poisson3d_boxes: (rowptr, colind, values,
    col_ghosts, global_row_offset, box extents) of one rank; no device."""
    sizes = (i64 * 7)()
    px, py, pz = (int(p) for p in parts)
    call("spmvh_poisson3d_box_rows", n, px, py, pz, rank, sizes, None, None,
         None, None)
    rowptr = np.empty(sizes[0] + 1, np.int32)
    colind = np.empty(sizes[1], np.int32)
    values = np.empty(sizes[1], np.float64)
    ghosts = np.empty(sizes[2], np.int64)
    call("spmvh_poisson3d_box_rows", n, px, py, pz, rank, sizes,
         _np_ptr(rowptr), _np_ptr(colind), _np_ptr(values), _np_ptr(ghosts))
    return rowptr, colind, values, ghosts, int(sizes[3]), tuple(sizes[4:7])


def cg(comm, exec_, A, b_ptr, x_ptr, kmax, rtol, history=True):
    """spmv::cg(comm, exec, A, b, x, kmax, rtol) -> (k, rnorm_history)"""
    k = C.c_int()
    hist = np.zeros(kmax + 1) if history else None
    call("spmvh_cg", comm.h, exec_.h, A.h, b_ptr, x_ptr, kmax, float(rtol),
         C.byref(k), _np_ptr(hist))
    return k.value, (hist[:k.value + 1] if history else None)


def cg_mixed(comm, exec_, A, b_ptr, x_ptr, kmax, rtol, replace_every=50,
             workspace=None, time_spmv=False, consumer_reductions=True,
             defer_x=True):
    """spmv::cg with CgOptions::mixed -> (k, rnorm_history, stats)"""
    k = C.c_int()
    hist = np.zeros(kmax + 2)
    st = (C.c_double * 6)()
    call("spmvh_cg_mixed", comm.h, exec_.h, A.h, b_ptr, x_ptr, kmax,
         float(rtol), int(replace_every), C.byref(k), _np_ptr(hist), len(hist),
         workspace.h if workspace else None,
         int(time_spmv) | (0 if consumer_reductions else 4)
         | (0 if defer_x else 8), st)
    stats = dict(spmv_ms_total=st[0], spmv_launches=int(st[1]),
                 replacements=int(st[2]), true_rel_residual=st[3],
                 continuation_iterations=int(st[4]),
                 final_true_rel_residual=st[5])
    return k.value, hist[:k.value + 1], stats


def read_petsc_binary_matrix(filename, comm, exec_, symmetric=False,
                             cm=COLLECTIVE_BLOCKING):
    """spmv::read_petsc_binary_matrix (spmv/read_petsc.cpp:40-228)"""
    h = vp()
    call("spmvh_read_petsc_matrix", comm.h, exec_.h, str(filename).encode(),
         int(symmetric), cm, C.byref(h))
    return Matrix(h)


def read_petsc_binary_vector(comm, exec_, filename):
    """-> (device pointer, local length); free with exec_.free()"""
    p, n = vp(), i64()
    call("spmvh_read_petsc_vector", comm.h, exec_.h, str(filename).encode(),
         C.byref(p), C.byref(n))
    return p.value or 0, n.value


def read_petsc_binary_rows(filename, rank, size):
    """Host-only parse of one rank's slice (no device)."""
    h, sizes = vp(), (i64 * 7)()
    call("spmvh_petsc_rows_read", str(filename).encode(), rank, size,
         C.byref(h), sizes)
    nloc = sizes[4] - sizes[3]
    rp = np.zeros(nloc + 1, np.int32)
    ci = np.zeros(sizes[5], np.int32)
    va = np.zeros(sizes[5], np.float64)
    gh = np.zeros(sizes[6], np.int64)
    call("spmvh_petsc_rows_get", h, _np_ptr(rp), _np_ptr(ci), _np_ptr(va),
         _np_ptr(gh))
    call("spmvh_petsc_rows_destroy", h)
    return dict(nrows=sizes[0], ncols=sizes[1], nnz=sizes[2],
                row_begin=sizes[3], row_end=sizes[4], rowptr=rp, colind=ci,
                values=va, col_ghosts=gh)


class _Workspace:
    """A solver's work vectors, kept across calls: the handle behind the
    spmvh_<_prefix>_workspace_create / _destroy symbols."""
    _prefix = None

    def __init__(self, exec_):
        h = vp()
        call(f"spmvh_{self._prefix}_workspace_create", exec_.h, C.byref(h))
        self.h = h

    def close(self):
        if self.h:
            call(f"spmvh_{self._prefix}_workspace_destroy", self.h)
            self.h = None


class _TimedWorkspace(_Workspace):
    def reserve_timing(self, count):
        """Creates the events of a time_spmv solve ahead of it: `count`
        iterations (ChebyshevWorkspace: SpMVs, iterations * degree)."""
        call(f"spmvh_{self._prefix}_workspace_reserve_timing", self.h,
             int(count))


class CgWorkspace(_TimedWorkspace):
    """spmv::CgWorkspace: work vectors kept across cg() calls."""
    _prefix = "cg"


def cg_ex(comm, exec_, A, b_ptr, x_ptr, kmax, rtol, workspace=None,
          time_spmv=False, history=False, consumer_reductions=True,
          poll_every=0, defer_x=True):
    """cg with the optional arguments: returns (k, history, spmv_ms_total,
    spmv_launches).  poll_every: CgOptions::poll_every (how many iterations the
    host may run ahead of the device's `done` flag; 0 = the default, 16).
    defer_x: CgOptions::defer_x (False = x updated in every iteration)."""
    k, n = C.c_int(), C.c_int()
    ms = f64()
    hist = np.zeros(kmax + 1) if history else None
    call("spmvh_cg_ex", comm.h, exec_.h, A.h, b_ptr, x_ptr, kmax, float(rtol),
         C.byref(k), _np_ptr(hist), workspace.h if workspace else None,
         int(time_spmv) | (0 if consumer_reductions else 4)
         | (0 if defer_x else 8) | ((int(poll_every) & 0xff) << 8), C.byref(ms),
         C.byref(n))
    return (k.value, hist[:k.value + 1] if history else None, ms.value,
            n.value)


class CgBlockWorkspace(_Workspace):
    """spmv::CgBlockWorkspace: work vectors kept across cg_block() calls."""
    _prefix = "cg_block"


def cg_block(comm, exec_, A, b_ptr, x_ptr, nrhs, kmax, rtol, workspace=None,
             time_spmv=False, poll_every=0):
    """spmv::cg_block: A X = B for nrhs interleaved right-hand sides (element
    (i, c) at B[i * nrhs + c]) -> (iterations[nrhs], history[nrhs, kmax + 1],
    stats).  history[c, j] = ||r_j|| of column c for j <= iterations[c], -1.0
    beyond.  stats: max_iterations, spmv_ms_total, spmv_launches."""
    nrhs, kmax = int(nrhs), int(kmax)
    kmx, n = C.c_int(), C.c_int()
    ms = f64()
    its = np.zeros(max(nrhs, 1), np.int32)
    hist = np.full((max(nrhs, 1), max(kmax, 0) + 1), -1.0)
    call("spmvh_cg_block", comm.h, exec_.h, A.h, b_ptr, x_ptr, nrhs, kmax,
         float(rtol), C.byref(kmx), _np_ptr(its), _np_ptr(hist),
         workspace.h if workspace else None,
         int(bool(time_spmv)) | ((int(poll_every) & 0xff) << 8), C.byref(ms),
         C.byref(n))
    return its, hist, dict(max_iterations=kmx.value, spmv_ms_total=ms.value,
                           spmv_launches=n.value)


def jacobi_inverse(exec_, d_ptr, dinv_ptr, n):
    """spmv::jacobi_inverse: dinv = 1 / d on the device (n doubles each; they
    may coincide).  Raises SpmvHostError ("diagonal is not positive") when an
    entry is not finite or not > 0."""
    call("spmvh_jacobi_inverse", exec_.h, d_ptr, dinv_ptr, int(n))


class PcgWorkspace(_TimedWorkspace):
    """spmv::PcgWorkspace: work vectors kept across pcg() calls."""
    _prefix = "pcg"


def pcg(comm, exec_, A, b_ptr, x_ptr, dinv_ptr, kmax, rtol, workspace=None,
        time_spmv=False, consumer_reductions=True, poll_every=0, stats=None):
    """spmv::pcg: CG from x0 = 0 with the diagonal preconditioner whose inverse
    is dinv -> (k, rnorm_history).  The history is that of the unpreconditioned
    residual, ||r_0|| .. ||r_k||, as cg()'s.  stats (optional dict) receives
    spmv_ms_total and spmv_launches of a time_spmv solve."""
    kmax = int(kmax)
    k, n = C.c_int(), C.c_int()
    ms = f64()
    hist = np.zeros(max(kmax, 0) + 1)
    call("spmvh_pcg", comm.h, exec_.h, A.h, b_ptr, x_ptr, dinv_ptr, kmax,
         float(rtol), C.byref(k), _np_ptr(hist),
         workspace.h if workspace else None,
         int(bool(time_spmv)) | (0 if consumer_reductions else 4)
         | ((int(poll_every) & 0xff) << 8), C.byref(ms), C.byref(n))
    if stats is not None:
        stats.update(spmv_ms_total=ms.value, spmv_launches=n.value)
    return k.value, hist[:k.value + 1]


def chebyshev_coefficients(degree, lmin, lmax):
    """spmv::chebyshev_coefficients -> (a, b), `degree` doubles each.  Raises
    SpmvHostError ("degree" / "bounds") for a degree outside 1..16 or bounds
    that are not finite with 0 < lmin < lmax.  Host only."""
    n = max(int(degree), 1)
    a, b = np.zeros(n), np.zeros(n)
    call("spmvh_chebyshev_coefficients", int(degree), float(lmin), float(lmax),
         _np_ptr(a), _np_ptr(b))
    return a, b


class ChebyshevWorkspace(_TimedWorkspace):
    """spmv::ChebyshevWorkspace: work vectors kept across pcg_chebyshev() and
    chebyshev_apply() calls."""
    _prefix = "chebyshev"


def chebyshev_apply(exec_, A, r_ptr, z_ptr, dinv_ptr, degree, lmin, lmax,
                    workspace=None):
    """spmv::chebyshev_apply: z = q(dinv*A) dinv r, the `degree`-step Chebyshev
    iteration for A z = r from z = 0 on [lmin, lmax].  dinv_ptr may be None."""
    call("spmvh_chebyshev_apply", exec_.h, A.h, r_ptr, z_ptr, dinv_ptr or None,
         int(degree), float(lmin), float(lmax),
         workspace.h if workspace else None)


def pcg_chebyshev(comm, exec_, A, b_ptr, x_ptr, dinv_ptr, degree, lmin, lmax,
                  kmax, rtol, workspace=None, time_spmv=False, poll_every=0,
                  stats=None):
    """spmv::pcg_chebyshev: CG from x0 = 0 with the Chebyshev polynomial
    preconditioner of `degree` in dinv*A on [lmin, lmax] -> (k, rnorm_history),
    the history that of the unpreconditioned residual.  dinv_ptr may be None.
    stats (optional dict) receives spmv_ms_total and spmv_launches of a
    time_spmv solve (`degree` SpMVs per iteration)."""
    kmax = int(kmax)
    k, n = C.c_int(), C.c_int()
    ms = f64()
    hist = np.zeros(max(kmax, 0) + 1)
    call("spmvh_pcg_chebyshev", comm.h, exec_.h, A.h, b_ptr, x_ptr,
         dinv_ptr or None, int(degree), float(lmin), float(lmax), kmax,
         float(rtol), C.byref(k), _np_ptr(hist),
         workspace.h if workspace else None,
         int(bool(time_spmv)) | ((int(poll_every) & 0xff) << 8), C.byref(ms),
         C.byref(n))
    if stats is not None:
        stats.update(spmv_ms_total=ms.value, spmv_launches=n.value)
    return k.value, hist[:k.value + 1]


def lambda_max_estimate(comm, exec_, A, dinv_ptr, v0_ptr, steps):
    """spmv::lambda_max_estimate: `steps` power iterations on dinv*A from v0
    with the generalised Rayleigh quotient -> the last estimate.  Advised:
    lmax = 1.1 * estimate(20 steps), lmin = lmax / 30."""
    lam = f64()
    call("spmvh_lambda_max_estimate", comm.h, exec_.h, A.h, dinv_ptr or None,
         v0_ptr, int(steps), C.byref(lam))
    return lam.value


def sgs_color(rowptr, colind, nrows, ncols_local=None, symmetric=False):
    """spmv::sgs_color: the greedy colouring of the local diagonal block over
    the pattern of B + B^T -> (colors[nrows], num_colors).  Host only."""
    rp = np.ascontiguousarray(rowptr, np.int32)
    ci = np.ascontiguousarray(colind, np.int32)
    nrows = int(nrows)
    colors = np.zeros(max(nrows, 1), np.int32)
    nc = C.c_int()
    call("spmvh_sgs_color", _np_ptr(rp), _np_ptr(ci), nrows,
         nrows if ncols_local is None else int(ncols_local), int(bool(symmetric)),
         _np_ptr(colors), C.byref(nc))
    return colors[:nrows], nc.value


def sgs_build(rowptr, colind, values, nrows, ncols_local=None, symmetric=False):
    """spmv::sgs_build: the colouring and the colour-major copy -> dict(colors,
    num_colors, perm, color_start, d, before=(ptr, col, val), after=(ptr, col,
    val)); the parts are CSR over positions (row perm[pos]).  Host only."""
    rp = np.ascontiguousarray(rowptr, np.int32)
    ci = np.ascontiguousarray(colind, np.int32)
    va = np.ascontiguousarray(values, np.float64)
    n = int(nrows)
    h = vp()
    sizes = np.zeros(3, np.int64)
    call("spmvh_sgs_build_create", _np_ptr(rp), _np_ptr(ci), _np_ptr(va), n,
         n if ncols_local is None else int(ncols_local), int(bool(symmetric)),
         C.byref(h), _np_ptr(sizes))
    try:
        nc, nb, na = (int(v) for v in sizes)
        colors, perm = np.zeros(n, np.int32), np.zeros(n, np.int32)
        start, d = np.zeros(nc + 1, np.int32), np.zeros(n)
        parts = [(np.zeros(n + 1, np.int64), np.zeros(m, np.int32), np.zeros(m))
                 for m in (nb, na)]
        call("spmvh_sgs_build_get", h, _np_ptr(colors), _np_ptr(perm),
             _np_ptr(start), _np_ptr(d), *[_np_ptr(a) for p in parts for a in p])
    finally:
        call("spmvh_sgs_build_destroy", h)
    return dict(colors=colors, num_colors=nc, perm=perm, color_start=start, d=d,
                before=parts[0], after=parts[1])


class SgsPreconditioner:
    """spmv::SgsPreconditioner: the multicolour symmetric Gauss-Seidel
    preconditioner of A's local diagonal block.  Owns its copy: A may
    release_csr() afterwards.  Raises SpmvHostError ("diagonal is not
    positive", "released", "same index range").

    setup="host" (the default) reads the block back and colours and reorders
    it on the host; setup="device" colours it and builds the plan where it
    lies.  order (device setup only): "hashed" (the default there: few rounds,
    more colours than the host's greedy) or "natural" (the host's colouring
    entry for entry; as many rounds as the longest ascending path of the
    pattern, slow on long dependency chains).  colors (device setup only):
    rows entries that replace the colouring, checked on the device ("not
    proper", "colour").  setup="host" with an order or colors raises.

    values="fp32" (with every setup, order and colors; "fp64" is the default
    and the object as it ever was) keeps the sweep plan's off-diagonal values
    as float, each rounded to nearest-even: a sweep streams 8 bytes per stored
    entry, not 12, and plan_bytes() drops by 4 per stored entry.  dinv, r, z
    and every operation stay fp64; M stays a fixed SPD operator every solver
    takes as before.  A value that rounds to Inf, zero or an fp32 subnormal
    raises SpmvHostError ("fp32 range"); any other string ValueError."""

    _SETUPS = {"host": 0, "device": 1}
    _ORDERS = {None: -1, "hashed": 0, "natural": 1}
    _VALUES = {"fp64": 0, "fp32": 1}
    _CREATE = "spmvh_sgs_create"

    def __init__(self, exec_, A, setup="host", order=None, colors=None,
                 values="fp64"):
        if values not in self._VALUES:
            raise ValueError(f"values {values!r}: 'fp64' or 'fp32'")
        h = vp()
        if (setup == "host" and order is None and colors is None
                and values == "fp64"):
            call(self._CREATE, exec_.h, A.h, C.byref(h))
        else:
            if setup not in self._SETUPS or order not in self._ORDERS:
                raise ValueError(f"setup {setup!r} / order {order!r}")
            keep = (None if colors is None
                    else np.ascontiguousarray(colors, np.int32))
            if values == "fp64":
                call(self._CREATE + "_ex", exec_.h, A.h, self._SETUPS[setup],
                     self._ORDERS[order], _np_ptr(keep), C.byref(h))
            else:
                call(self._CREATE + "_ex2", exec_.h, A.h, self._SETUPS[setup],
                     self._ORDERS[order], _np_ptr(keep), self._VALUES[values],
                     C.byref(h))
        self.h = h

    @property
    def value_bits(self):
        """64 or 32: the width of the sweep plan's off-diagonal values"""
        bits = C.c_int()
        call("spmvh_sgs_value_bits", self.h, C.byref(bits))
        return bits.value

    def close(self):
        if self.h:
            call("spmvh_sgs_destroy", self.h)
            self.h = None

    def _info(self):
        rows, nc, nbytes = C.c_int(), C.c_int(), i64()
        call("spmvh_sgs_info", self.h, C.byref(rows), C.byref(nc),
             C.byref(nbytes))
        return rows.value, nc.value, nbytes.value

    def rows(self):
        return self._info()[0]

    def num_colors(self):
        return self._info()[1]

    def plan_bytes(self):
        return self._info()[2]

    def colors(self):
        out = np.zeros(self.rows(), np.int32)
        call("spmvh_sgs_colors", self.h, _np_ptr(out))
        return out

    def rounds(self):
        """rounds of the device colouring (0: host setup or caller's colours)"""
        r, ms = C.c_int(), f64()
        call("spmvh_sgs_setup_info", self.h, C.byref(r), C.byref(ms))
        return r.value

    def setup_ms(self):
        """wall time of the constructor"""
        r, ms = C.c_int(), f64()
        call("spmvh_sgs_setup_info", self.h, C.byref(r), C.byref(ms))
        return ms.value

    def setup_detail(self):
        """device setup -> dict(color_ms, build_ms, temp_bytes); zeros otherwise"""
        cm, bm, tb = f64(), f64(), i64()
        call("spmvh_sgs_setup_detail", self.h, C.byref(cm), C.byref(bm),
             C.byref(tb))
        return dict(color_ms=cm.value, build_ms=bm.value, temp_bytes=tb.value)

    _PART_KEYS = (("color_slice", np.int32), ("slice_pos0", np.int32),
                  ("slice_ptr", np.int64), ("len", np.int32), ("col", np.int32),
                  ("val", np.float64), ("color_long", np.int32),
                  ("long_pos", np.int32), ("long_ptr", np.int64),
                  ("long_col", np.int32), ("long_val", np.float64))

    def plan_arrays(self):
        """the plan's arrays, copied from the device -> dict(perm, color_start,
        dinv, before, after); a part is a dict of the arrays of SgsSlicedPart
        (host/sgs_build.h)"""
        sizes = np.zeros(10, np.int64)
        call("spmvh_sgs_export_sizes", self.h, _np_ptr(sizes))
        n, nc, ns = (int(v) for v in sizes[:3])
        out = dict(perm=np.zeros(n, np.int32),
                   color_start=np.zeros(nc + 1, np.int32), dinv=np.zeros(n))
        ptrs = []
        for h, name in enumerate(("before", "after")):
            ent, nl, lent = (int(v) for v in sizes[3 + 3 * h:6 + 3 * h])
            count = dict(color_slice=nc + 1, slice_pos0=ns, slice_ptr=ns + 1,
                         len=n, col=ent, val=ent, color_long=nc + 1,
                         long_pos=nl, long_ptr=nl + 1, long_col=lent,
                         long_val=lent)
            out[name] = {k: np.zeros(count[k], t) for k, t in self._PART_KEYS}
            ptrs.append((vp * 11)(*[out[name][k].ctypes.data
                                    for k, _ in self._PART_KEYS]))
        call("spmvh_sgs_export", self.h, _np_ptr(out["perm"]),
             _np_ptr(out["color_start"]), _np_ptr(out["dinv"]), ptrs[0], ptrs[1])
        return out


def fp32_range_count(values):
    """how many of the doubles are finite, non-zero and round to +-Inf, zero
    or an fp32 subnormal: the rule by which values="fp32" refuses a value.
    Host only."""
    v = np.ascontiguousarray(values, np.float64)
    count = i64()
    call("spmvh_fp32_range_count", _np_ptr(v), v.size, C.byref(count))
    return count.value


def sgs_apply(exec_, M, r_ptr, z_ptr):
    """spmv::sgs_apply: z = M^-1 r on the executor's current stream; the host
    does not wait."""
    call("spmvh_sgs_apply", exec_.h, M.h, r_ptr, z_ptr)


def ilu0_symbolic(rowptr, colind, nrows, ncols_local=None, symmetric=False):
    """spmv::ilu0_symbolic: the colouring, the positions and the two parts in
    POSITION order -> dict(colors, num_colors, perm, pos, color_start, before,
    after); a part is dict(ptr, cpos, src, slot, sliced_col, long_col), CSR over
    positions (host/ilu0_build.h).  Host only.  Raises SpmvHostError
    ("duplicate")."""
    rp = np.ascontiguousarray(rowptr, np.int32)
    ci = np.ascontiguousarray(colind, np.int32)
    n = int(nrows)
    h = vp()
    sizes = np.zeros(7, np.int64)
    call("spmvh_ilu0_symbolic_create", _np_ptr(rp), _np_ptr(ci), n,
         n if ncols_local is None else int(ncols_local), int(bool(symmetric)),
         C.byref(h), _np_ptr(sizes))
    try:
        nc = int(sizes[0])
        colors, perm, pos = (np.zeros(n, np.int32) for _ in range(3))
        start = np.zeros(nc + 1, np.int32)
        parts = []
        for m, ns, nl in ((sizes[1], sizes[3], sizes[4]),
                          (sizes[2], sizes[5], sizes[6])):
            parts.append(dict(ptr=np.zeros(n + 1, np.int64),
                              cpos=np.zeros(int(m), np.int32),
                              src=np.zeros(int(m), np.int32),
                              slot=np.zeros(int(m), np.int64),
                              sliced_col=np.zeros(int(ns), np.int32),
                              long_col=np.zeros(int(nl), np.int32)))
        call("spmvh_ilu0_symbolic_get", h, _np_ptr(colors), _np_ptr(perm),
             _np_ptr(pos), _np_ptr(start),
             *[_np_ptr(a) for p in parts for a in p.values()])
    finally:
        call("spmvh_ilu0_symbolic_destroy", h)
    return dict(colors=colors, num_colors=nc, perm=perm, pos=pos,
                color_start=start, before=parts[0], after=parts[1])


class Ilu0Preconditioner(SgsPreconditioner):
    """spmv::Ilu0Preconditioner: multicolour ILU(0) of A's local diagonal block,
    factored on the device (IC(0) as L D L^T for a symmetric A).  Accepted
    wherever an SgsPreconditioner is (sgs_apply, pcg_sgs, gmres(sgs=...)).
    Raises SpmvHostError ("pivot", "duplicate", "released", "same index
    range").

    setup, order and colors are SgsPreconditioner's: setup="host" (the
    default) does the symbolic work on the host from the pattern read back;
    setup="device" colours the block and builds every array of the plan where
    the matrix lies (order="natural": the host-built object bit for bit).
    setup="host" with an order or colors raises.

    values="fp32": the factorisation stays fp64 (factor(), pattern() and the
    pivot counts do not change); l~ and u~ are rounded to float as they are
    scattered into the sweep plan, dinv~ stays fp64, refactor() rounds again.
    A factor entry out of fp32's range raises "fp32 range" from the
    constructor and from refactor(); after such a refactor() the object raises
    until a later one succeeds."""

    _CREATE = "spmvh_ilu0_create"

    _ILU_KEYS = (("ptr", np.int64), ("cpos", np.int32), ("src", np.int32),
                 ("slot", np.int64))

    def ilu_arrays(self):
        """the part arrays of the device plan, copied from the device ->
        dict(before, after); a part is dict(ptr, cpos, src, slot), CSR over
        positions (host/ilu0_build.h's Ilu0Part)"""
        sizes = np.zeros(4, np.int64)
        call("spmvh_ilu0_export_sizes", self.h, _np_ptr(sizes))
        n = int(sizes[0])
        out, ptrs = {}, []
        for name, m in (("before", int(sizes[1])), ("after", int(sizes[2]))):
            count = dict(ptr=n + 1 if n > 0 else 0, cpos=m, src=m, slot=m)
            out[name] = {k: np.zeros(count[k], t) for k, t in self._ILU_KEYS}
            ptrs.append((vp * 4)(*[out[name][k].ctypes.data
                                   for k, _ in self._ILU_KEYS]))
        call("spmvh_ilu0_export", self.h, ptrs[0], ptrs[1])
        return out

    def refactor(self, A):
        """the numeric factorisation again, on the device alone, for a matrix
        of the same pattern whose values have changed"""
        call("spmvh_ilu0_refactor", self.h, A.h)

    def _ilu_info(self):
        info = np.zeros(6, np.int64)
        call("spmvh_ilu0_info", self.h, _np_ptr(info))
        return [int(v) for v in info]

    def negative_pivots(self):
        return self._ilu_info()[2]

    def plan_bytes(self):
        return self._ilu_info()[3]

    def setup_ms(self):
        """-> (host symbolic, device numeric) wall time of the constructor"""
        info = self._ilu_info()
        return info[4] / 1000.0, info[5] / 1000.0

    def pattern(self):
        """-> ((before_ptr, before_col), (after_ptr, after_col)): CSR over
        colour-major positions, the entries ascending by the position of their
        column"""
        n, info = self.rows(), self._ilu_info()
        out = [(np.zeros(n + 1, np.int64), np.zeros(m, np.int32))
               for m in info[:2]]
        call("spmvh_ilu0_pattern", self.h, *[_np_ptr(a) for p in out for a in p])
        return out[0], out[1]

    def factor(self):
        """-> (l, u, d): the factor's entries in the order of pattern(), the
        pivots d by position"""
        n, info = self.rows(), self._ilu_info()
        l, u, d = np.zeros(info[0]), np.zeros(info[1]), np.zeros(n)
        call("spmvh_ilu0_factor", self.h, _np_ptr(l), _np_ptr(u), _np_ptr(d))
        return l, u, d


def ilu0_apply(exec_, M, r_ptr, z_ptr):
    """spmv::ilu0_apply = sgs_apply on the factor"""
    sgs_apply(exec_, M, r_ptr, z_ptr)


class SgsWorkspace(_TimedWorkspace):
    """spmv::SgsWorkspace: work vectors kept across pcg_sgs() calls."""
    _prefix = "sgs"


def pcg_sgs(comm, exec_, A, M, b_ptr, x_ptr, kmax, rtol, workspace=None,
            time_spmv=False, poll_every=0, stats=None):
    """spmv::pcg_sgs: CG from x0 = 0 with the multicolour symmetric
    Gauss-Seidel preconditioner M -> (k, rnorm_history), the history that of
    the unpreconditioned residual.  stats (optional dict) receives
    spmv_ms_total and spmv_launches of a time_spmv solve (one SpMV per
    iteration)."""
    kmax = int(kmax)
    k, n = C.c_int(), C.c_int()
    ms = f64()
    hist = np.zeros(max(kmax, 0) + 1)
    call("spmvh_pcg_sgs", comm.h, exec_.h, A.h, M.h, b_ptr, x_ptr, kmax,
         float(rtol), C.byref(k), _np_ptr(hist),
         workspace.h if workspace else None,
         int(bool(time_spmv)) | ((int(poll_every) & 0xff) << 8), C.byref(ms),
         C.byref(n))
    if stats is not None:
        stats.update(spmv_ms_total=ms.value, spmv_launches=n.value)
    return k.value, hist[:k.value + 1]


def sgs_apply_block(exec_, M, r_ptr, z_ptr, nrhs):
    """spmv::sgs_apply_block: Z = M^-1 R for nrhs interleaved vectors (element
    (i, c) at R[i * nrhs + c]) on the executor's current stream; M is an
    SgsPreconditioner or an Ilu0Preconditioner.  Column c has the bits of
    sgs_apply on column c."""
    call("spmvh_sgs_apply_block", exec_.h, M.h, r_ptr, z_ptr, int(nrhs))


class PcgBlockWorkspace(_Workspace):
    """spmv::PcgBlockWorkspace: work vectors kept across pcg_block() calls."""
    _prefix = "pcg_block"


def pcg_block(comm, exec_, A, b_ptr, x_ptr, nrhs, kmax, rtol, dinv=None,
              sgs=None, workspace=None, time_spmv=False, poll_every=0,
              amg=None):
    """spmv::pcg_block: preconditioned CG on A X = B for nrhs interleaved
    right-hand sides; exactly one of dinv (device pointer, rows doubles), sgs
    (an SgsPreconditioner or Ilu0Preconditioner) and amg (an
    AmgPreconditioner) -> (iterations[nrhs], history[nrhs, kmax + 1], stats),
    as cg_block returns them."""
    nrhs, kmax = int(nrhs), int(kmax)
    kmx, n = C.c_int(), C.c_int()
    ms = f64()
    its = np.zeros(max(nrhs, 1), np.int32)
    hist = np.full((max(nrhs, 1), max(kmax, 0) + 1), -1.0)
    tail = (kmax, float(rtol), C.byref(kmx), _np_ptr(its), _np_ptr(hist),
            workspace.h if workspace else None,
            int(bool(time_spmv)) | ((int(poll_every) & 0xff) << 8),
            C.byref(ms), C.byref(n))
    if amg is not None and dinv is None and sgs is None:
        call("spmvh_pcg_block_amg", comm.h, exec_.h, A.h, b_ptr, x_ptr, nrhs,
             amg.h, *tail)
    else:
        if amg is not None:  # more than one: the rule, without a device
            call("spmvh_pcg_block_amg_check_arguments", nrhs, kmax,
                 int(dinv is not None), int(sgs is not None), 1, 0, 0, 0, 0,
                 None, None, None)
        call("spmvh_pcg_block", comm.h, exec_.h, A.h, b_ptr, x_ptr, nrhs, dinv,
             sgs.h if sgs is not None else None, *tail)
    return its, hist, dict(max_iterations=kmx.value, spmv_ms_total=ms.value,
                           spmv_launches=n.value)


AMG_DEFAULTS = dict(theta=0.25, max_levels=10, min_coarse_rows=200,
                    smooth_degree=2, coarse_degree=8, eig_ratio=4.0,
                    coarse_scale=1.0)


def _amg_options(options):
    opt = dict(AMG_DEFAULTS)
    unknown = set(options) - set(opt)
    if unknown:
        raise TypeError(f"unknown AmgOptions field(s): {sorted(unknown)}")
    opt.update(options)
    return opt


def amg_check_options(**options):
    """the rules of spmv::AmgOptions; raises SpmvHostError naming the field"""
    o = _amg_options(options)
    call("spmvh_amg_check_options", float(o["theta"]), int(o["max_levels"]),
         int(o["min_coarse_rows"]), int(o["smooth_degree"]),
         int(o["coarse_degree"]), float(o["eig_ratio"]),
         float(o["coarse_scale"]))


def amg_check_tail_rows(max_rows):
    """the rule of AmgPreconditioner.set_tail_rows; raises SpmvHostError
    naming "tail_rows"; no device"""
    call("spmvh_amg_check_tail_rows", int(max_rows))


def amg_symbolic(rowptr, colind, values, nrows, ncols_local=None,
                 symmetric=False, diagonal=None, theta=0.25):
    """One coarsening step of host/amg_build.h -> dict(n_agg, agg, member_ptr,
    member, rowptr, colind, src_ptr, src, xrow_ptr, xrow_col, xrow_src).
    Symmetric input: the stored strictly lower block and `diagonal`.  A source
    >= 0 indexes values, < 0 is diagonal[~src].  Host only."""
    rp = np.ascontiguousarray(rowptr, np.int32)
    ci = np.ascontiguousarray(colind, np.int32)
    va = np.ascontiguousarray(values, np.float64)
    dg = None if diagonal is None else np.ascontiguousarray(diagonal, np.float64)
    n = int(nrows)
    h = vp()
    sizes = np.zeros(4, np.int64)
    call("spmvh_amg_symbolic_create", _np_ptr(rp), _np_ptr(ci), _np_ptr(va),
         _np_ptr(dg), n, n if ncols_local is None else int(ncols_local),
         int(bool(symmetric)), float(theta), C.byref(h), _np_ptr(sizes))
    try:
        na, nnz, ns, nx = (int(v) for v in sizes)
        out = dict(agg=np.zeros(n, np.int32),
                   member_ptr=np.zeros(na + 1, np.int32),
                   member=np.zeros(n, np.int32),
                   rowptr=np.zeros(na + 1, np.int32),
                   colind=np.zeros(nnz, np.int32),
                   src_ptr=np.zeros(nnz + 1, np.int64),
                   src=np.zeros(ns, np.int32),
                   xrow_ptr=np.zeros(n + 1, np.int64),
                   xrow_col=np.zeros(nx, np.int32),
                   xrow_src=np.zeros(nx, np.int32))
        call("spmvh_amg_symbolic_get", h, *[_np_ptr(a) for a in out.values()])
    finally:
        call("spmvh_amg_symbolic_destroy", h)
    out["n_agg"] = na
    return out


class AmgPreconditioner:
    """spmv::AmgPreconditioner: one V-cycle of plain aggregation multigrid on
    A's local diagonal block.  Options: the fields of spmv::AmgOptions as
    keywords.  Level 0 is A's own block: keep A alive (or refresh(A)).  An
    application is not reentrant.  Raises SpmvHostError ("diagonal is not
    positive"; "row-sum bound is not finite": a level's max_i |row i| / d_i is
    Inf or 0, from a diagonal entry too small to invert or entries whose sum
    overflows; "released", "same index range", an option's name).  After a
    refresh that raised, the object raises until a refresh succeeds.

    setup="host" (the default) reads every level back and aggregates on the
    host; setup="device" aggregates and builds every list of the hierarchy
    where the matrices lie.  order (device setup only): "hashed" (the default
    there: few rounds, other aggregates than the host's) or "natural" (the
    host's hierarchy bit for bit; as many rounds as the longest dependency
    chain).  setup="host" with an order raises."""

    _SETUPS = {"host": 0, "device": 1}
    _ORDERS = {None: -1, "hashed": 0, "natural": 1}

    def __init__(self, exec_, A, setup="host", order=None, **options):
        o = _amg_options(options)
        amg_check_options(**o)
        packed = np.array([o[k] for k in AMG_DEFAULTS], np.float64)
        h = vp()
        if setup == "host" and order is None:
            call("spmvh_amg_create", exec_.h, A.h, _np_ptr(packed), C.byref(h))
        else:
            if setup not in self._SETUPS or order not in self._ORDERS:
                raise ValueError(f"setup {setup!r} / order {order!r}")
            call("spmvh_amg_create_ex", exec_.h, A.h, _np_ptr(packed),
                 self._SETUPS[setup], self._ORDERS[order], C.byref(h))
        self.h = h
        self.options = o
        self.setup = setup

    def close(self):
        if self.h:
            call("spmvh_amg_destroy", self.h)
            self.h = None

    def refresh(self, A):
        """new values on the same pattern: the Galerkin sums, the diagonals
        and the bounds again, on the device alone"""
        call("spmvh_amg_refresh", self.h, A.h)

    def set_tail_rows(self, max_rows):
        """Run the longest suffix of levels >= 1 whose levels all have at most
        max_rows rows in ONE launch per application (0 = off, the default).
        Same bits.  Between applications only; it waits for the device."""
        call("spmvh_amg_set_tail_rows", self.h, int(max_rows))

    def release_block_scratch(self):
        """Frees the block scratch of amg_apply_block (it waits for the
        device); the next block application allocates it again."""
        call("spmvh_amg_release_block_scratch", self.h)

    def tail_levels(self):
        """levels the fused launch runs; 0 = no tail"""
        n = C.c_int()
        call("spmvh_amg_tail_levels", self.h, C.byref(n))
        return n.value

    def tail_lanes(self, level):
        """lanes per row of the level's product inside the tail, as its plan
        reported them (0 = one lane per row); -1 = not in the tail"""
        n = C.c_int()
        call("spmvh_amg_tail_lanes", self.h, int(level), C.byref(n))
        return n.value

    def _info(self):
        info = np.zeros(4, np.int64)
        call("spmvh_amg_info", self.h, _np_ptr(info))
        return [int(v) for v in info]

    def _level(self, level):
        sizes, lmax = np.zeros(2, np.int64), f64()
        call("spmvh_amg_level_info", self.h, int(level), _np_ptr(sizes),
             C.byref(lmax))
        return int(sizes[0]), int(sizes[1]), lmax.value

    def levels(self):
        return self._info()[0]

    def plan_bytes(self):
        return self._info()[1]

    def setup_ms(self):
        """-> (host symbolic, device numeric) wall time of the constructor (of
        the last refresh: numeric alone)"""
        info = self._info()
        return info[2] / 1000.0, info[3] / 1000.0

    def setup_detail(self):
        """the device setup's record -> dict(aggregate_ms, build_ms (both part
        of the symbolic time), temp_bytes: the peak of its temporaries); zeros
        for the host setup"""
        info = np.zeros(4, np.int64)
        call("spmvh_amg_setup_info", self.h, _np_ptr(info))
        return dict(aggregate_ms=int(info[0]) / 1000.0,
                    build_ms=int(info[1]) / 1000.0, temp_bytes=int(info[2]))

    def rounds(self, level):
        """-> (pass 1, pass 3): the rounds the device setup took to aggregate
        `level`; (0, 0) for setup="host" and for a level without a step"""
        r = (C.c_int * 2)()
        call("spmvh_amg_level_rounds", self.h, int(level), r)
        return int(r[0]), int(r[1])

    _STEP_KEYS = (("agg", np.int32), ("member_ptr", np.int32),
                  ("member", np.int32), ("src_ptr", np.int64), ("src", np.int32),
                  ("xrow_ptr", np.int64), ("xrow_src", np.int32))

    def step_arrays(self, level):
        """host copies of the device plan of `level` (spmv_hip_amg_plan_export)
        -> dict of the arrays that exist, plus coarse_rows, coarse_nnz and
        bytes; {} where the level has no plan"""
        s = np.zeros(9, np.int64)
        call("spmvh_amg_step_sizes", self.h, int(level), _np_ptr(s))
        n, nc, nnz_c, nsrc, has_x, nx = (int(s[0]), int(s[1]), int(s[4]),
                                         int(s[5]), int(s[6]), int(s[7]))
        if not (nc or has_x):
            return {}
        size = dict(agg=n, member_ptr=nc + 1, member=n, src_ptr=nnz_c + 1,
                    src=nsrc) if nc else {}
        if has_x:
            size.update(xrow_ptr=n + 1, xrow_src=nx)
        out = {k: np.zeros(size[k], t) for k, t in self._STEP_KEYS if k in size}
        call("spmvh_amg_step_export", self.h, int(level),
             *[_np_ptr(out.get(k)) for k, _ in self._STEP_KEYS])
        out.update(coarse_rows=nc, coarse_nnz=nnz_c, bytes=int(s[8]))
        return out

    def rows(self, level=0):
        return self._level(level)[0]

    def non_zeros(self, level):
        return self._level(level)[1]

    def lmax(self, level):
        return self._level(level)[2]

    def aggregates(self, level):
        out = np.zeros(self.rows(level), np.int32)
        call("spmvh_amg_aggregates", self.h, int(level), _np_ptr(out))
        return out

    def level_matrix(self, level):
        """-> (rowptr, colind, values) of the operator of a level >= 1"""
        n, nnz, _ = self._level(level)
        rp, ci = np.zeros(n + 1, np.int32), np.zeros(nnz, np.int32)
        va = np.zeros(nnz)
        call("spmvh_amg_level_matrix", self.h, int(level), _np_ptr(rp),
             _np_ptr(ci), _np_ptr(va))
        return rp, ci, va


def amg_apply(exec_, M, r_ptr, z_ptr):
    """spmv::amg_apply: z = M^-1 r on the executor's current stream; the host
    does not wait."""
    call("spmvh_amg_apply", exec_.h, M.h, r_ptr, z_ptr)


def amg_apply_block(exec_, M, r_ptr, z_ptr, nrhs):
    """spmv::amg_apply_block: Z = M^-1 R for nrhs interleaved vectors (element
    (i, c) at R[i * nrhs + c]) on the executor's current stream.  Column c has
    the bits of amg_apply on column c, whatever the other columns hold."""
    call("spmvh_amg_apply_block", exec_.h, M.h, r_ptr, z_ptr, int(nrhs))


AmgPcgWorkspace = SgsWorkspace


def pcg_amg(comm, exec_, A, M, b_ptr, x_ptr, kmax, rtol, workspace=None,
            time_spmv=False, poll_every=0, stats=None):
    """spmv::pcg_amg: CG from x0 = 0 with the AMG V-cycle M -> (k,
    rnorm_history); the arguments and the contract of pcg_sgs."""
    kmax = int(kmax)
    k, n = C.c_int(), C.c_int()
    ms = f64()
    hist = np.zeros(max(kmax, 0) + 1)
    call("spmvh_pcg_amg", comm.h, exec_.h, A.h, M.h, b_ptr, x_ptr, kmax,
         float(rtol), C.byref(k), _np_ptr(hist),
         workspace.h if workspace else None,
         int(bool(time_spmv)) | ((int(poll_every) & 0xff) << 8), C.byref(ms),
         C.byref(n))
    if stats is not None:
        stats.update(spmv_ms_total=ms.value, spmv_launches=n.value)
    return k.value, hist[:k.value + 1]


class BicgstabWorkspace(_TimedWorkspace):
    """spmv::BicgstabWorkspace: work vectors kept across bicgstab() calls."""
    _prefix = "bicgstab"


def bicgstab(comm, exec_, A, b_ptr, x_ptr, dinv_ptr, kmax, rtol, ws=None,
             time_spmv=False, consumer_reductions=True, poll_every=0,
             stats=None):
    """spmv::bicgstab: BiCGStab from x0 = 0 for a matrix that need not be
    symmetric -> (k, rnorm_history, status).  dinv_ptr: None, or the inverse
    diagonal of a right preconditioner (any finite nonzero device vector).
    status: 0 converged or kmax reached, 1 / 2 the breakdowns (host/cg.h).
    stats (optional dict) receives spmv_ms_total and spmv_launches of a
    time_spmv solve (two SpMVs per iteration)."""
    kmax = int(kmax)
    k, n, status = C.c_int(), C.c_int(), C.c_int()
    ms = f64()
    hist = np.zeros(max(kmax, 0) + 1)
    call("spmvh_bicgstab", comm.h, exec_.h, A.h, b_ptr, x_ptr, dinv_ptr or None,
         kmax, float(rtol), C.byref(k), C.byref(status), _np_ptr(hist),
         ws.h if ws else None,
         int(bool(time_spmv)) | (0 if consumer_reductions else 4)
         | ((int(poll_every) & 0xff) << 8), C.byref(ms), C.byref(n))
    if stats is not None:
        stats.update(spmv_ms_total=ms.value, spmv_launches=n.value)
    return k.value, hist[:k.value + 1], status.value


class GmresWorkspace(_TimedWorkspace):
    """spmv::GmresWorkspace: basis, work vectors and device scalars kept across
    gmres() calls."""
    _prefix = "gmres"


GMRES_MAX_RESTART = 64


def gmres(comm, exec_, A, b_ptr, x_ptr, restart, kmax, rtol, dinv_ptr=None,
          cheb=None, sgs=None, ws=None, time_spmv=False, poll_every=0,
          stats=None, amg=None):
    """spmv::gmres: restarted GMRES from x0 = 0 with a right preconditioner for
    a matrix that need not be symmetric -> (k, rnorm_history, status).
    Preconditioner: none; dinv_ptr (the inverse diagonal); cheb = (degree, lmin,
    lmax) for chebyshev_apply (with dinv_ptr or without); sgs, an
    SgsPreconditioner; or amg, an AmgPreconditioner.  status: 0 converged or kmax reached, 1 the lucky
    breakdown, 2 a zero pivot (host/cg.h).  stats (optional dict) receives
    spmv_ms_total and spmv_launches of a time_spmv solve (one SpMV per inner
    step)."""
    kmax = int(kmax)
    k, n, status = C.c_int(), C.c_int(), C.c_int()
    ms = f64()
    hist = np.zeros(max(kmax, 0) + 1)
    degree, lmin, lmax = cheb if cheb else (0, 0.0, 0.0)
    args = [comm.h, exec_.h, A.h, b_ptr, x_ptr, dinv_ptr or None,
            int(degree), float(lmin), float(lmax), sgs.h if sgs else None,
            int(restart), kmax, float(rtol), C.byref(k), C.byref(status),
            _np_ptr(hist), ws.h if ws else None,
            int(bool(time_spmv)) | ((int(poll_every) & 0xff) << 8), C.byref(ms),
            C.byref(n)]
    if amg is None:
        call("spmvh_gmres", *args)
    else:
        call("spmvh_gmres_amg", *args, amg.h)
    if stats is not None:
        stats.update(spmv_ms_total=ms.value, spmv_launches=n.value)
    return k.value, hist[:k.value + 1], status.value


class MinresWorkspace(_TimedWorkspace):
    """spmv::MinresWorkspace: work vectors and device scalars kept across
    minres() calls."""
    _prefix = "minres"


def minres_check_rules(kmax, has_dinv=False, has_sgs=False, has_amg=False,
                       sgs_rows=0, sgs_negative_pivots=0, amg_rows=0, rows=0,
                       b_ptr=None, x_ptr=None, dinv_ptr=None):
    """spmv::minres_check_rules alone (no device; the pointers are compared,
    never dereferenced); raises SpmvHostError naming the rule."""
    call("spmvh_minres_check_rules", int(kmax), int(bool(has_dinv)),
         int(bool(has_sgs)), int(bool(has_amg)), int(sgs_rows),
         int(sgs_negative_pivots), int(amg_rows), int(rows), b_ptr or None,
         x_ptr or None, dinv_ptr or None)


def minres(comm, exec_, A, b_ptr, x_ptr, kmax, rtol, dinv_ptr=None, sgs=None,
           amg=None, ws=None, time_spmv=False, poll_every=0, stats=None):
    """spmv::minres: preconditioned MINRES from x0 = 0 for a symmetric matrix
    that need not be definite -> (k, rnorm_history, status).  Preconditioner
    (symmetric positive definite, at most one): dinv_ptr, a positive device
    vector; sgs, an SgsPreconditioner or an Ilu0Preconditioner without negative
    pivots; amg, an AmgPreconditioner.  rnorm_history is the residual in the
    M^-1-norm (the 2-norm without a preconditioner).  status: 0 converged or
    kmax reached, 1 the Lanczos process ended, 2 r.M^-1 r < 0, 3 a singular
    direction (host/cg.h).  stats (optional dict) receives spmv_ms_total and
    spmv_launches of a time_spmv solve (one SpMV per iteration)."""
    kmax = int(kmax)
    k, n, status = C.c_int(), C.c_int(), C.c_int()
    ms = f64()
    hist = np.zeros(max(kmax, 0) + 1)
    call("spmvh_minres", comm.h, exec_.h, A.h, b_ptr, x_ptr, dinv_ptr or None,
         sgs.h if sgs else None, amg.h if amg else None, kmax, float(rtol),
         C.byref(k), C.byref(status), _np_ptr(hist), ws.h if ws else None,
         int(bool(time_spmv)) | ((int(poll_every) & 0xff) << 8), C.byref(ms),
         C.byref(n))
    if stats is not None:
        stats.update(spmv_ms_total=ms.value, spmv_launches=n.value)
    return k.value, hist[:k.value + 1], status.value


class LsqrWorkspace(_TimedWorkspace):
    """spmv::LsqrWorkspace: work vectors and device scalars kept across lsqr()
    calls."""
    _prefix = "lsqr"


def lsqr_check_rules(kmax, ltol=0.0, damp=0.0, rows=0, cols=0, b_ptr=None,
                     x_ptr=None):
    """spmv::lsqr_check_rules alone (no device; the pointers are compared, never
    dereferenced); raises SpmvHostError naming the rule."""
    call("spmvh_lsqr_check_rules", int(kmax), float(ltol), float(damp),
         int(rows), int(cols), b_ptr or None, x_ptr or None)


def lsqr(comm, exec_, A, b_ptr, x_ptr, kmax, rtol, ltol=0.0, damp=0.0, ws=None,
         time_spmv=False, poll_every=0, stats=None):
    """spmv::lsqr: LSQR from x0 = 0 for any matrix, rectangular or square ->
    (k, hist_r, hist_ar, status).  Minimises ||A x - b||^2 + damp^2 ||x||^2 on
    Matrix::mult and Matrix::transpmult; b_ptr: the matrix's local rows, x_ptr:
    its owned columns.  hist_r estimates ||b - A x|| (with damp:
    sqrt(||b - A x||^2 + damp^2 ||x||^2)), hist_ar ||A^T (b - A x) - damp^2 x||.
    status: 0 kmax reached or hist_r[k] / hist_r[0] < rtol, 1 the least-squares
    test hist_ar[k] / (||A|| hist_r[k]) < ltol, 2 the bidiagonalisation ended
    (host/cg.h).  stats (optional dict) receives spmv_ms_total and
    spmv_launches of a time_spmv solve (two products per iteration)."""
    kmax = int(kmax)
    k, n, status = C.c_int(), C.c_int(), C.c_int()
    ms = f64()
    hist_r = np.zeros(max(kmax, 0) + 1)
    hist_ar = np.zeros(max(kmax, 0) + 1)
    call("spmvh_lsqr", comm.h, exec_.h, A.h, b_ptr, x_ptr, kmax, float(rtol),
         float(ltol), float(damp), C.byref(k), C.byref(status), _np_ptr(hist_r),
         _np_ptr(hist_ar), ws.h if ws else None,
         int(bool(time_spmv)) | ((int(poll_every) & 0xff) << 8), C.byref(ms),
         C.byref(n))
    if stats is not None:
        stats.update(spmv_ms_total=ms.value, spmv_launches=n.value)
    return k.value, hist_r[:k.value + 1], hist_ar[:k.value + 1], status.value


class LobpcgWorkspace(_TimedWorkspace):
    """spmv::LobpcgWorkspace: work blocks and device scalars kept across
    lobpcg() calls."""
    _prefix = "lobpcg"


def lobpcg_check_rules(nev, kmax, rtol=1e-8, atol=0.0, has_dinv=False,
                       has_sgs=False, has_amg=False, sgs_rows=0,
                       sgs_negative_pivots=0, amg_rows=0, rows=0):
    """spmv::lobpcg_check_rules alone (no device); raises SpmvHostError naming
    the rule."""
    call("spmvh_lobpcg_check_rules", int(nev), int(kmax), float(rtol),
         float(atol), int(has_dinv), int(has_sgs), int(has_amg), int(sgs_rows),
         int(sgs_negative_pivots), int(amg_rows), int(rows))


def lobpcg_check_pencil(rows_a, rows_b, ghosts_a=(), ghosts_b=()):
    """spmv::lobpcg_check_pencil alone (no device): B must have A's local row
    count and exactly A's ghost list (global indices, same order); raises
    SpmvHostError naming the rule "pencil"."""
    ga = np.ascontiguousarray(ghosts_a, np.int64)
    gb = np.ascontiguousarray(ghosts_b, np.int64)
    call("spmvh_lobpcg_check_pencil", int(rows_a), int(rows_b), _np_ptr(ga),
         ga.size, _np_ptr(gb), gb.size)


def lobpcg(comm, exec_, A, x_ptr, nev, kmax, rtol, atol=0.0, dinv=None,
           sgs=None, amg=None, largest=False, workspace=None, time_spmv=False,
           poll_every=0, stats=None, B=None):
    """spmv::lobpcg: the nev smallest (largest=True: largest) eigenpairs of a
    symmetric A -> (k, eigenvalues[nev], history[nev, kmax + 1], status).
    B (optional, a Matrix): the pencil A x = lambda B x with a symmetric
    positive definite B that has A's rows and A's ghosts (rule "pencil"); X is
    then B-orthonormal on exit, the residual is A x - theta B x, and a B that
    is not positive definite ends with status 1.
    x_ptr: device block of rows * nev doubles (mult_block layout), the initial
    guess on entry, the Ritz vectors on exit.  At most one of dinv (device
    pointer, rows doubles), sgs (an SgsPreconditioner or Ilu0Preconditioner)
    and amg (an AmgPreconditioner).  history: -1.0 beyond the iteration at
    which a column met rn < max(rtol |theta|, atol).  status: 0, or 1 the basis
    collapsed (host/cg.h).  stats (optional dict) receives true_resnorm (from
    A X computed after the loop), restarts, spmv_ms_total and spmv_launches."""
    nev, kmax = int(nev), int(kmax)
    k, n, status, restarts = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    ms = f64()
    eig = np.zeros(max(nev, 1))
    true_rn = np.zeros(max(nev, 1))
    hist = np.full((max(nev, 1), max(kmax, 0) + 1), -1.0)
    entry = ("spmvh_lobpcg", comm.h, exec_.h, A.h) if B is None else (
        "spmvh_lobpcg_gen", comm.h, exec_.h, A.h, B.h)
    call(*entry, x_ptr, nev, dinv,
         sgs.h if sgs is not None else None, amg.h if amg is not None else None,
         kmax, float(rtol), float(atol), C.byref(k), C.byref(status),
         _np_ptr(eig), _np_ptr(hist), _np_ptr(true_rn), C.byref(restarts),
         workspace.h if workspace else None,
         int(bool(time_spmv)) | (int(bool(largest)) << 1)
         | ((int(poll_every) & 0xff) << 8), C.byref(ms), C.byref(n))
    if stats is not None:
        stats.update(true_resnorm=true_rn[:nev].copy(), restarts=restarts.value,
                     spmv_ms_total=ms.value, spmv_launches=n.value)
    return k.value, eig[:nev], hist[:nev], status.value


class CgShiftedWorkspace(_TimedWorkspace):
    """spmv::CgShiftedWorkspace: work vectors and device scalars kept across
    cg_shifted() calls."""
    _prefix = "cgs"


def cgs_check_rules(ns, kmax, rows=0, ldx=0, shifts=None, b_ptr=None,
                    x_ptr=None):
    """spmv::cgs_check_rules alone (no device; shifts: a sequence of floats or
    None, read on the host; the pointers are compared, never dereferenced);
    raises SpmvHostError naming the rule."""
    sh = None if shifts is None else np.ascontiguousarray(shifts, np.float64)
    call("spmvh_cgs_check_rules", int(ns), int(kmax), int(rows), int(ldx),
         _np_ptr(sh), b_ptr or None, x_ptr or None)


def cg_shifted(comm, exec_, A, b_ptr, x_ptr, ldx, shifts, kmax, rtol, ws=None,
               time_spmv=False, poll_every=0, stats=None):
    """spmv::cg_shifted: multi-shift CG, (A + shifts[s] I) x_s = b for every s
    from x_s = 0 with one product per iteration -> (k, iterations, history,
    status).  A symmetric positive definite, 1..8 shifts, each finite and >= 0;
    b_ptr: the matrix's local rows; solution s is the contiguous device vector
    x_ptr + 8 * s * ldx.  iterations: the ns counts (k is the largest);
    history: an array [ns, kmax + 1], row s holding ||r_s|| of iterations
    0..iterations[s] and -1.0 beyond; status: 0, or 1 when p.(A p) was not
    positive (host/cg.h).  stats (optional dict) receives spmv_ms_total and
    spmv_launches of a time_spmv solve."""
    kmax = int(kmax)
    sh = np.ascontiguousarray(shifts, np.float64).reshape(-1)
    ns = len(sh)
    k, n, status = C.c_int(), C.c_int(), C.c_int()
    ms = f64()
    its = np.zeros(max(ns, 1), np.int32)
    hist = np.zeros((max(ns, 1), max(kmax, 0) + 1))
    call("spmvh_cg_shifted", comm.h, exec_.h, A.h, b_ptr, x_ptr, int(ldx),
         _np_ptr(sh), ns, kmax, float(rtol), C.byref(k),
         its.ctypes.data_as(vp), _np_ptr(hist), C.byref(status),
         ws.h if ws else None,
         int(bool(time_spmv)) | ((int(poll_every) & 0xff) << 8), C.byref(ms),
         C.byref(n))
    if stats is not None:
        stats.update(spmv_ms_total=ms.value, spmv_launches=n.value)
    return k.value, its[:ns].copy(), hist[:ns], status.value


class IdrsWorkspace(_TimedWorkspace):
    """spmv::IdrsWorkspace: G, U, the work vectors and device scalars kept
    across idrs() calls."""
    _prefix = "idrs"


IDRS_MAX_S = 8


def idrs_check_rules(s, kmax, kappa=0.7, has_dinv=False, cheb=None,
                     has_sgs=False, has_amg=False, pre_rows=0, rows=0,
                     b_ptr=None, x_ptr=None, dinv_ptr=None):
    """spmv::idrs_check_rules alone (no device; the pointers are compared, never
    dereferenced); raises SpmvHostError naming the rule."""
    degree, lmin, lmax = cheb if cheb else (0, 0.0, 0.0)
    call("spmvh_idrs_check_rules", int(s), int(kmax), float(kappa),
         int(bool(has_dinv)), int(degree), float(lmin), float(lmax),
         int(bool(has_sgs)), int(bool(has_amg)), int(pre_rows), int(rows),
         b_ptr or None, x_ptr or None, dinv_ptr or None)


def idrs(comm, exec_, A, b_ptr, x_ptr, s, kmax, rtol, dinv_ptr=None, cheb=None,
         sgs=None, amg=None, ws=None, kappa=0.7, seed=0, time_spmv=False,
         poll_every=0, stats=None):
    """spmv::idrs: IDR(s), 1 <= s <= 8, from x0 = 0 on sign shadow vectors with a
    right preconditioner, for a matrix that need not be symmetric -> (k,
    rnorm_history, status).  Preconditioner: as gmres().  status: 0 rtol or kmax
    reached, 1 a zero pivot of M, 2 a zero or non-finite om (host/cg.h).  stats
    (optional dict) receives spmv_ms_total and spmv_launches of a time_spmv
    solve (one SpMV per step)."""
    kmax = int(kmax)
    k, n, status = C.c_int(), C.c_int(), C.c_int()
    ms = f64()
    hist = np.zeros(max(kmax, 0) + 1)
    degree, lmin, lmax = cheb if cheb else (0, 0.0, 0.0)
    call("spmvh_idrs", comm.h, exec_.h, A.h, b_ptr, x_ptr, dinv_ptr or None,
         int(degree), float(lmin), float(lmax), sgs.h if sgs else None,
         amg.h if amg else None, int(s), kmax, float(rtol), float(kappa),
         int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(k), C.byref(status),
         _np_ptr(hist), ws.h if ws else None,
         int(bool(time_spmv)) | ((int(poll_every) & 0xff) << 8), C.byref(ms),
         C.byref(n))
    if stats is not None:
        stats.update(spmv_ms_total=ms.value, spmv_launches=n.value)
    return k.value, hist[:k.value + 1], status.value


def host_executor_rejects_compute():
    return lib.spmvh_host_executor_rejects_compute() == 0
