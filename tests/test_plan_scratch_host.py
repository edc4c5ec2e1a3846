"""CPU checks of the plan builders' device memory: the hipMalloc / hipFree
macros are gone, the ten plan-building files allocate only through
plan_scratch.h, the ownership header stands alone, and its stand-alone check
program builds with the line in its header and passes under the address and
undefined-behaviour sanitizers (a program of its own: nothing is loaded into
this process)."""
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(ROOT, "spmv_amd", "csrc", "hip")
PLAN_FILES = ("spmv_csr_plan.hip", "spmv_csr_forms.hip", "spmv_sjds_plan.hip",
              "spmv_wdia.hip", "spmv_symdia.hip", "spmv_sym.hip", "spmv_symlat.hip",
              "spmv_lat.hip", "spmv_mv.hip", "spmv_mcgs.hip")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_the_macros_are_gone_and_plan_files_allocate_through_one_header():
    assert not os.path.exists(os.path.join(HIP_DIR, "plan_malloc.h"))
    for name in sorted(os.listdir(HIP_DIR)):
        src = _read(HIP_DIR, name)
        assert not re.search(r"#\s*define\s+hipMalloc", src), name
        assert not re.search(r"#\s*define\s+hipFree", src), name
    for name in PLAN_FILES:
        src = _read(HIP_DIR, name)
        assert "hipMalloc(" not in src and "hipFree(" not in src, name
        assert '#include "plan_scratch.h"' in src, name
    scratch = _read(HIP_DIR, "plan_scratch.h")
    assert scratch.count("hipMalloc(") == 1 and scratch.count("hipFree(") == 1
    assert '#include "dev_scratch.h"' in scratch
    mk = _read(ROOT, "spmv_amd", "csrc", "Makefile")
    assert "hip/dev_scratch.h" in mk and "hip/plan_scratch.h" in mk
    assert "plan_malloc.h" not in mk


def test_the_ownership_header_stands_alone():
    src = _read(HIP_DIR, "dev_scratch.h")
    includes = re.findall(r"#\s*include\s*([<\"][^>\"]+[>\"])", src)
    assert sorted(includes) == ["<cstddef>", "<utility>"], includes


def test_the_check_program_builds_as_its_header_says_and_passes(tmp_path):
    path = os.path.join(ROOT, "tools", "plan_scratch_check.cpp")
    head = _read(path).split("#include", 1)[0]
    m = re.search(r"//\s+(g\+\+(?:.*\n)+?.*?)&& \./plan_scratch_check", head)
    assert m, "no build line in the header comment"
    words = shlex.split(re.sub(r"\n//", " ", m.group(1)))
    assert "-fsanitize=address,undefined" in words and "-std=c++17" in words
    exe = str(tmp_path / "plan_scratch_check")
    words[words.index("-o") + 1] = exe
    subprocess.run(words, cwd=ROOT, check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "plan_scratch_check: OK"
    assert run.stderr == "", run.stderr  # (the sanitizers are silent)
