"""CPU checks of the solver workspaces' device memory: the eleven solver files
allocate only through solver_ws.h, the ownership core under it stands alone,
and its stand-alone check program builds with the line in its header and passes
under the address and undefined-behaviour sanitizers (a program of its own:
nothing is loaded into this process)."""
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(ROOT, "spmv_amd", "csrc", "hip")
SOLVER_FILES = ("blas1.hip", "blas1_block.hip", "blas1_pcg.hip",
                "blas1_pcg_block.hip", "blas1_bicgstab.hip", "blas1_gmres.hip",
                "blas1_minres.hip", "blas1_lsqr.hip", "blas1_lobpcg.hip",
                "blas1_cgshift.hip", "blas1_idrs.hip")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_the_solver_files_allocate_through_one_header():
    for name in SOLVER_FILES:
        src = _read(HIP_DIR, name)
        assert "hipMalloc(" not in src and "hipFree(" not in src, name
        assert "solver_ws_create(" in src and "solver_ws_destroy(" in src, name
    binding = _read(HIP_DIR, "solver_ws.h")
    assert binding.count("hipMalloc(") == 1 and binding.count("hipFree(") == 1
    assert '#include "ws_core.h"' in binding
    mk = _read(ROOT, "spmv_amd", "csrc", "Makefile")
    assert "hip/ws_core.h" in mk and "hip/solver_ws.h" in mk


def test_the_ownership_core_stands_alone():
    src = _read(HIP_DIR, "ws_core.h")
    includes = re.findall(r"#\s*include\s*([<\"][^>\"]+[>\"])", src)
    assert sorted(includes) == ["<cstddef>", "<cstdlib>", "<cstring>", "<new>"], \
        includes


def test_the_check_program_builds_as_its_header_says_and_passes(tmp_path):
    path = os.path.join(ROOT, "tools", "ws_core_check.cpp")
    head = _read(path).split("#include", 1)[0]
    m = re.search(r"//\s+(g\+\+(?:.*\n)+?.*?)&& \./ws_core_check", head)
    assert m, "no build line in the header comment"
    words = shlex.split(re.sub(r"\n//", " ", m.group(1)))
    assert "-fsanitize=address,undefined" in words and "-std=c++17" in words
    exe = str(tmp_path / "ws_core_check")
    words[words.index("-o") + 1] = exe
    subprocess.run(words, cwd=ROOT, check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ws_core_check: OK"
    assert run.stderr == "", run.stderr  # (the sanitizers are silent)
