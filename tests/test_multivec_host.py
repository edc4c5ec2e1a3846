"""CPU checks of the multi-vector product's interface (Matrix::mult_block): the
new symbols are declared, exported and prototyped, NULL handles and k < 1 are
refused before anything is launched, and the Python layer has the methods."""
import os
import re

from spmv_amd import _lib, hip, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ("spmv_hip_csr_spmm_f64", "spmv_hip_csr_spmm_f32f64",
           "spmv_hip_csr_spmm_f32", "spmv_hip_interleave_f64",
           "spmv_hip_interleave_f32", "spmv_hip_deinterleave_f64",
           "spmv_hip_deinterleave_f32", "spmv_hip_gather_block_f64",
           "spmv_hip_gather_block_f32")
HOST_NEW = ("spmvh_matrix_mult_block", "spmvh_matrix_update_block",
            "spmvh_matrix_update_finalise_block", "spmvh_matrix_f32_mult_block",
            "spmvh_matrix_f32_update_block",
            "spmvh_matrix_f32_update_finalise_block", "spmvh_l2gmap_update_block",
            "spmvh_l2gmap_update_finalise_block")


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(\w+)\s*\(", txt))


def test_multivec_symbols_declared_exported_prototyped():
    hip_decl, host_decl = _declared("spmv_hip.h"), _declared("spmv_host_c.h")
    for n in HIP_NEW:
        assert n in hip_decl and hasattr(_lib.hip, n) and n in _lib.HIP_SYMBOLS
    for n in HOST_NEW:
        assert n in host_decl and hasattr(host.lib, n) and n in host.HOST_SYMBOLS
    # the change is additive: the ABI version stays
    assert _lib.hip.spmv_hip_abi_version() == 5


def test_layout_is_stated_in_the_header():
    txt = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert "INTERLEAVED" in txt and "X[i * k + c]" in txt


def test_multivec_null_handles_and_bad_k_rejected():
    h = _lib.hip
    for name in ("spmv_hip_csr_spmm_f64", "spmv_hip_csr_spmm_f32f64",
                 "spmv_hip_csr_spmm_f32"):
        f = getattr(h, name)
        assert f(None, None, 1, 1, 0, None, None, None, None, 1.0, None, 0.0,
                 None, 2, None) == -1
        assert f(None, None, 1, 1, 0, None, None, None, None, 1.0, None, 0.0,
                 None, 0, None) == -1
    for name in HIP_NEW[3:7]:
        assert getattr(h, name)(None, 4, 2, None, 4, None, None) == -1
    for name in HIP_NEW[7:]:
        assert getattr(h, name)(None, 1, None, 2, None, None, None) == -1
    for n in HOST_NEW:
        args = [None] * (len(getattr(host.lib, n).argtypes) - 1) + [2]
        assert getattr(host.lib, n)(*args) != 0
        assert b"NULL" in host.lib.spmvh_last_error()


def test_python_layer_has_the_methods():
    for cls, names in ((host.Matrix, ("mult_block",)),
                       (host.MatrixF32, ("mult_block", "update_block")),
                       (host.ColMapView, ("update_block", "update_finalise_block")),
                       (host.L2GMap, ("update_block", "update_finalise_block")),
                       (hip.CsrBlock, ("multm",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    for n in ("interleave", "deinterleave", "gather_block"):
        assert callable(getattr(hip, n))
