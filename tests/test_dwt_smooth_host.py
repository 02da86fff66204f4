"""CPU-side checks of the DWT smoothing ladder's entry point (wtmi_dwt_smooth): argument
validation without a GPU, and the kernel's register budget read from the built library's
code-object metadata (scripts/kernel_meta.py)."""

import ctypes as C
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# The LDS formula of csrc/dwt_smooth.hip gives 39 KB at the app's shape (n = 1333, db4, J = 7):
# four 384-thread workgroups per CU of 160 KiB = 6 waves per SIMD, so at most 512 / 6 = 85 ->
# 80 VGPRs (allocated in eights).  At n = 8192 one chain takes 89 KiB: one 512-thread workgroup
# per CU, 2 waves per SIMD, which any budget meets.  The smaller bound holds for both kernels.
BUDGET = {"void wtmi::dwt_smooth_kernel<true>": 80, "void wtmi::dwt_smooth_kernel<false>": 80}


def test_dwt_smooth_arguments_rejected_without_gpu():
    from wtmi import _lib
    lib = _lib.load()
    taps = (C.c_double * 8)(*([0.125] * 8))
    lo = C.cast(taps, C.c_void_p)
    N, one = None, C.c_void_p(16)  # a non-NULL pointer no rejected call dereferences
    f = lambda *a: lib.wtmi_dwt_smooth(*a)
    assert f(N, N, 16, 0, 16, lo, lo, 8, 3, 1, N, N, N) == 0               # empty batch
    assert f(N, N, 16, -1, 16, lo, lo, 8, 3, 1, N, N, N) == -1
    assert f(one, N, 16, 1, 16, lo, lo, 8, 3, 1, N, N, N) == -1            # no output
    assert f(one, N, 16, 1, 16, lo, lo, 8, 3, 1, one, one, N) == -1        # stats without y
    assert f(one, N, 16, 1, 16, lo, lo, 8, 0, 1, one, N, N) == -1          # level < 1
    assert f(one, N, 8, 1, 16, lo, lo, 8, 3, 1, one, N, N) == -1           # ld < n
    assert f(one, N, 16, 1, 16, N, lo, 8, 3, 1, one, N, N) == -1           # the bank is host data
    assert f(one, N, 16, 1, 16, lo, N, 8, 3, 1, one, N, N) == -1
    assert f(one, N, 8193, 1, 8193, lo, lo, 8, 3, 1, one, N, N) == -2
    assert f(one, N, 16, 1, 16, lo, lo, 7, 3, 1, one, N, N) == -2          # odd n_taps
    assert f(one, N, 16, 1, 16, lo, lo, 42, 3, 1, one, N, N) == -2


def test_dwt_smooth_op_registered_and_checked():
    import torch
    from wtmi import ops
    assert hasattr(torch.ops.wtmi, "dwt_smooth")
    lo = [0.5, 0.5]
    with pytest.raises(ValueError, match="level"):
        ops.dwt_smooth(torch.zeros(2, 32), lo, lo, 0)
    with pytest.raises(ValueError, match="no output"):
        ops.dwt_smooth(torch.zeros(2, 32), lo, lo, 2, want_smooth=False)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.dwt_smooth(torch.zeros(2, 32), lo, lo, 2)


@pytest.fixture(scope="module")
def table():
    from kernel_meta import LIB, LLVM, kernel_table
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")) or not shutil.which("c++filt"):
        pytest.skip("llvm-readelf / c++filt not available")
    if not os.path.exists(LIB):
        pytest.skip("libwtmi.so not built")
    return kernel_table(LIB)


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_smooth_kernel_registers(table, kernel):
    assert kernel in table, f"{kernel} not in libwtmi.so"
    r = table[kernel]
    assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (kernel, r)
    assert r["vgpr"] <= BUDGET[kernel], (kernel, r)
