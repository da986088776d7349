"""CPU checks for the one-pass median + Gram work:

- the odd-even merge schedule (hip/csrc/oem_sort.h) is proved on the host by
  tests/oem_sort_check.cpp, a stand-alone program built with the host
  compiler (with AddressSanitizer and UBSan where the toolchain has them);
- ``ext.colsel(..., gram=G)`` refuses its bad argument combinations before
  any device work. Without a GPU every call here is refused at the first
  check (X on the CPU); the mode / rows messages themselves are asserted on
  device tensors in test_gpu_median_gram.py.
"""
import os
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from byzpy_amd import hip

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "byzpy_amd" / "hip" / "csrc"
CHECK_SRC = Path(__file__).resolve().parent / "oem_sort_check.cpp"


def _host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cand and shutil.which(cand):
            return cand
    pytest.fail("no host C++ compiler found (tried $CXX, c++, g++, clang++)")


def test_oem_schedule_sorts_every_01_input(tmp_path):
    cxx = _host_compiler()
    exe = tmp_path / "oem_sort_check"
    base = [cxx, "-std=c++17", "-O1", f"-I{CSRC}", str(CHECK_SRC), "-o", str(exe)]
    san = subprocess.run(
        base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
        capture_output=True, text=True,
    )
    if san.returncode != 0:
        # toolchain without the sanitizer runtimes: the proof itself still runs
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout


@pytest.fixture(scope="module")
def ext():
    return hip.require()


def test_colsel_gram_rejects_cpu_matrix_first(ext):
    X = torch.randn(40, 8).to(torch.bfloat16)
    G = torch.zeros(40, 40)
    with pytest.raises(RuntimeError, match="device tensor"):
        ext.colsel(X, 0, 0, gram=G)
    # still the first refusal when the other arguments are bad as well
    with pytest.raises(RuntimeError, match="device tensor"):
        ext.colsel(X, 1, 0, gram=torch.zeros(3))


def test_colsel_gram_with_other_mode_raises(ext):
    X = torch.randn(40, 8).to(torch.bfloat16)
    G = torch.zeros(40, 40)
    for mode in (1, 2):
        with pytest.raises(RuntimeError):
            ext.colsel(X, mode, 1, gram=G)


def test_colsel_gram_with_rows_raises(ext):
    X = torch.randn(40, 8).to(torch.bfloat16)
    G = torch.zeros(40, 40)
    rows = torch.arange(40, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ext.colsel(X, 0, 0, rows, gram=G)
    with pytest.raises(RuntimeError):
        ext.colsel(X, 0, 0, rows=rows, gram=G)


def test_colsel_gram_is_keyword_only(ext):
    # the positional form stays (X, mode, f, rows): no fifth positional
    X = torch.randn(40, 8).to(torch.bfloat16)
    with pytest.raises(TypeError):
        ext.colsel(X, 0, 0, None, torch.zeros(40, 40))
    with pytest.raises(TypeError):
        ext.colsel(X, 0, 0, gramm=torch.zeros(40, 40))
