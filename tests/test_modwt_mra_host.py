"""CPU-side checks of the MODWT MRA entry points (wtmi_modwt_mra / wtmi_modwt_mra_rows):
argument validation without a GPU, and the register budgets of their hot instantiations read
from the built library's code-object metadata (scripts/kernel_meta.py)."""

import ctypes as C
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# kernel -> VGPR budget; spills must be 0
BUDGET = {
    # single series: a 1024-thread workgroup holds 64 KiB of LDS at n = 16384, two per CU = 8
    # waves per SIMD, so at most 64 VGPRs (the batch shape of scripts/mra_ab.py)
    "void wtmi::modwt_mra_vec_kernel<4, false>": 64,
    "void wtmi::modwt_mra_vec_kernel<1, false>": 64,
    "void wtmi::modwt_mra_kernel<4, false>": 64,
    # pairs: one 1024-thread workgroup per CU at 128 KiB of LDS, 4 waves per SIMD = 128 VGPRs;
    # the app's pair of 1333 samples runs modwt_mra_kernel<4, true> with 384 threads
    "void wtmi::modwt_mra_vec_kernel<4, true>": 128,
    "void wtmi::modwt_mra_vec_kernel<1, true>": 128,
    "void wtmi::modwt_mra_kernel<4, true>": 128,
    "void wtmi::modwt_mra_kernel<16, true>": 128,
    "void wtmi::modwt_mra_rows_kernel<16>": 64,  # two 1024-thread workgroups per CU
}


def banks():
    lo = (C.c_double * 8)(*([0.125] * 8))
    hi = (C.c_double * 8)(*([0.125, -0.125] * 4))
    return C.cast(lo, C.c_void_p), C.cast(hi, C.c_void_p), (lo, hi)


def test_modwt_mra_arguments_rejected_without_gpu():
    from wtmi import _lib
    lib = _lib.load()
    lo, hi, _keep = banks()
    N, one = None, C.c_void_p(16)  # a non-NULL pointer no rejected call dereferences
    mra = lambda *a: lib.wtmi_modwt_mra(*a)
    assert mra(N, N, 16, 0, 16, lo, hi, 8, 3, 1, N, N, N, N) == 0          # empty batch
    assert mra(N, N, 16, -1, 16, lo, hi, 8, 3, 1, N, N, N, N) == -1
    assert mra(N, N, 16, 0, 16, N, N, 8, 3, 1, N, N, N, N) == -1            # the bank is host data
    assert mra(N, N, 8, 0, 16, lo, hi, 8, 3, 1, N, N, N, N) == -1           # ld < n
    assert mra(N, N, 16, 0, 16, lo, hi, 8, 0, 1, N, N, N, N) == -1          # level < 1
    assert mra(one, N, 16, 1, 16, lo, hi, 8, 3, 1, N, N, N, N) == -1        # no output
    assert mra(one, N, 16, 1, 16, lo, hi, 8, 3, 1, one, N, one, N) == -1    # stats without y
    assert mra(N, N, 16, 1, 16, lo, hi, 8, 3, 1, one, N, N, N) == -1        # no x
    assert mra(one, N, 16385, 1, 16385, lo, hi, 8, 3, 1, one, N, N, N) == -2
    assert mra(one, N, 16, 1, 16, lo, hi, 41, 3, 1, one, N, N, N) == -2
    rows = lambda *a: lib.wtmi_modwt_mra_rows(*a)
    assert rows(N, 0, 16, lo, hi, 8, 3, N, N) == 0
    assert rows(N, -1, 16, lo, hi, 8, 3, N, N) == -1
    assert rows(N, 0, 16, N, N, 8, 3, N, N) == -1
    assert rows(N, 1, 16, lo, hi, 8, 3, one, N) == -1 and rows(one, 1, 16, lo, hi, 8, 3, N, N) == -1
    assert rows(one, 1, 16385, lo, hi, 8, 3, one, N) == -2
    assert rows(one, 1, 16, lo, hi, 41, 3, one, N) == -2


def test_modwt_mra_ops_registered_and_checked():
    import torch
    from wtmi import ops
    assert hasattr(torch.ops.wtmi, "modwt_mra") and hasattr(torch.ops.wtmi, "modwt_mra_rows")
    lo, hi = [0.5, 0.5], [0.5, -0.5]
    with pytest.raises(ValueError, match="level"):
        ops.modwt_mra(torch.zeros(2, 32), lo, hi, 0)
    with pytest.raises(ValueError, match="no output"):
        ops.modwt_mra(torch.zeros(2, 32), lo, hi, 2, want_components=False)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.modwt_mra_rows(torch.zeros(3, 32), lo, hi)


@pytest.fixture(scope="module")
def table():
    from kernel_meta import LIB, LLVM, kernel_table
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")) or not shutil.which("c++filt"):
        pytest.skip("llvm-readelf / c++filt not available")
    if not os.path.exists(LIB):
        pytest.skip("libwtmi.so not built")
    return kernel_table(LIB)


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_mra_kernel_registers(table, kernel):
    assert kernel in table, f"{kernel} not in libwtmi.so"
    r = table[kernel]
    assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (kernel, r)
    assert r["vgpr"] <= BUDGET[kernel], (kernel, r)
