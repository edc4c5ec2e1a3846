"""CPU checks of the transposed product's interface (Matrix::transpmult): the
new symbols are declared, exported and prototyped, and NULL handles are
refused before anything is launched."""
import os
import re

from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ("spmv_hip_csr_plan_build_transpose", "spmv_hip_csr_spmvt_f64",
           "spmv_hip_csr_spmvt_f32")
HOST_NEW = ("spmvh_matrix_transpmult", "spmvh_matrix_f32_transpmult",
            "spmvh_matrix_enable_transpose")


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(\w+)\s*\(", txt))


def test_transpose_symbols_declared_exported_prototyped():
    hip_decl, host_decl = _declared("spmv_hip.h"), _declared("spmv_host_c.h")
    for n in HIP_NEW:
        assert n in hip_decl and hasattr(_lib.hip, n) and n in _lib.HIP_SYMBOLS
    for n in HOST_NEW:
        assert n in host_decl and hasattr(host.lib, n) and n in host.HOST_SYMBOLS
    # the change is additive: the ABI version stays
    assert _lib.hip.spmv_hip_abi_version() == 5


def test_transpose_null_handles_rejected():
    h = _lib.hip
    assert h.spmv_hip_csr_plan_build_transpose(None, None, None, None, None, 8, 0,
                                               0, None) == -1
    assert h.spmv_hip_csr_spmvt_f64(None, None, 1, 1, 0, None, None, None, 1.0,
                                    None, 0.0, None, None) == -1
    assert h.spmv_hip_csr_spmvt_f32(None, None, 1, 1, 0, None, None, None, 1.0,
                                    None, 0.0, None, None) == -1
    for n in HOST_NEW:
        args = [None] * len(getattr(host.lib, n).argtypes)
        assert getattr(host.lib, n)(*args) != 0
        assert b"NULL" in host.lib.spmvh_last_error()


def test_host_executor_still_has_no_compute_path():
    # a HostExecutor cannot even hold a matrix, so neither mult nor transpmult
    # can run on it: the same error as before
    assert host.host_executor_rejects_compute()
    assert b"no CPU compute path" in host.lib.spmvh_last_error()
