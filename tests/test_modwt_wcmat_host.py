"""CPU-side checks of the wavelet correlation matrix entry point (wtmi_modwt_wcmat): argument
validation without a GPU, and the register budgets of every instantiation its launcher can pick,
read from the built library's code-object metadata (scripts/kernel_meta.py)."""

import ctypes as C
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# 1024-thread workgroups, one per CU at M n = 32768 (128 KiB of rows): 4 waves per SIMD, hence at
# most 128 VGPRs, for each number of matrix steps a wave keeps in registers
KERNELS = [f"void wtmi::modwt_wcmat_kernel<{per}>" for per in (4, 16, 32, 64)]
VGPR_BUDGET = 128


def test_modwt_wcmat_arguments_rejected_without_gpu():
    from wtmi import _lib
    lib = _lib.load()
    lo = (C.c_double * 8)(*([0.125] * 8))
    hi = (C.c_double * 8)(*([0.125, -0.125] * 4))
    lo_p, hi_p = C.cast(lo, C.c_void_p), C.cast(hi, C.c_void_p)
    N, one = None, C.c_void_p(16)  # a non-NULL pointer no rejected call dereferences

    def wm(x=one, ld=16, batch=1, M=4, n=16, lo=lo_p, hi=hi_p, taps=8, level=3, boundary=1, cov=one, corr=N,
           r2=N, stats=N):
        return lib.wtmi_modwt_wcmat(x, ld, batch, M, n, lo, hi, taps, level, boundary, 1.96, cov, corr, r2, stats, N)

    assert wm(x=N, cov=N, batch=0) == 0                       # empty batch
    assert wm(x=N, cov=N, batch=0, M=16, n=2048, ld=2048) == 0  # the limits, accepted
    assert wm(x=N, cov=N, batch=0, M=2, n=16384, ld=16384, taps=40, level=62) == 0
    for bad in (dict(lo=N), dict(hi=N), dict(x=N), dict(cov=N), dict(ld=15), dict(M=1), dict(level=0),
                dict(level=63), dict(boundary=2), dict(batch=-1), dict(r2=one), dict(stats=one)):
        assert wm(**bad) == -1, bad
    for big in (dict(M=17), dict(M=16, n=2049, ld=2049), dict(M=2, n=16385, ld=16385), dict(taps=41)):
        assert wm(**big) == -2, big


def test_modwt_wcmat_op_registered_and_checked():
    import torch
    from wtmi import ops
    assert hasattr(torch.ops.wtmi, "modwt_wcmat") and len(ops.WCMAT_STATS) == 6
    assert (ops.WCMAT_MAX_SERIES, ops.WCMAT_MAX_SAMPLES) == (16, 32768)
    lo, hi, x = [0.5, 0.5], [0.5, -0.5], torch.zeros(2, 3, 32)
    with pytest.raises(ValueError, match="level"):
        ops.modwt_wcmat(x, lo, hi, 0)
    with pytest.raises(ValueError, match="boundary"):
        ops.modwt_wcmat(x, lo, hi, 2, boundary="reflect")
    with pytest.raises(ValueError, match="ci_level"):
        ops.modwt_wcmat(x, lo, hi, 2, ci_level=1.0)
    with pytest.raises(ValueError, match="series"):
        ops.modwt_wcmat(x[:, :1], lo, hi, 2)
    with pytest.raises(ValueError, match="same number of taps"):
        ops.modwt_wcmat(x, lo, [0.5], 2)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.modwt_wcmat(x, lo, hi, 2)


@pytest.fixture(scope="module")
def table():
    from kernel_meta import LIB, LLVM, kernel_table
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")) or not shutil.which("c++filt"):
        pytest.skip("llvm-readelf / c++filt not available")
    if not os.path.exists(LIB):
        pytest.skip("libwtmi.so not built")
    return kernel_table(LIB)


@pytest.mark.parametrize("kernel", KERNELS)
def test_wcmat_kernel_registers(table, kernel):
    assert kernel in table, f"{kernel} not in libwtmi.so"
    r = table[kernel]
    assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (kernel, r)
    assert r["vgpr"] <= VGPR_BUDGET, (kernel, r)
