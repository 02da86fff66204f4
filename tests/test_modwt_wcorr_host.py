"""CPU-side checks of the wavelet correlation entry point (wtmi_modwt_wcorr): argument
validation without a GPU, and the register budgets of its hot instantiations read from the
built library's code-object metadata (scripts/kernel_meta.py)."""

import ctypes as C
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# kernel -> VGPR budget; spills must be 0
BUDGET = {
    # single series: 64 KiB of LDS at n = 16384, two 1024-thread workgroups per CU = 8 waves per
    # SIMD, so at most 64 VGPRs (shorter rows: more, smaller workgroups under the same bound)
    "void wtmi::modwt_wcorr_vec_kernel<4, false, false>": 64,
    "void wtmi::modwt_wcorr_vec_kernel<1, false, false>": 64,
    "void wtmi::modwt_wcorr_kernel<4, false, false>": 64,
    # pairs without lags: two rows, 128 KiB at n = 16384 = one 1024-thread workgroup per CU, 4
    # waves per SIMD = 128 VGPRs; the batch shape 4096 x 1024 runs <1, true, false> with 256 threads
    "void wtmi::modwt_wcorr_vec_kernel<4, true, false>": 128,
    "void wtmi::modwt_wcorr_vec_kernel<1, true, false>": 128,
    "void wtmi::modwt_wcorr_kernel<16, true, false>": 128,
    # pairs with lags: four rows, 128 KiB at n = 8192 = one 1024-thread workgroup per CU, 128
    # VGPRs; the app's pair of 1333 samples runs modwt_wcorr_kernel<4, true, true> with 384 threads
    "void wtmi::modwt_wcorr_vec_kernel<2, true, true>": 128,
    "void wtmi::modwt_wcorr_vec_kernel<1, true, true>": 128,
    "void wtmi::modwt_wcorr_kernel<4, true, true>": 128,
    "void wtmi::modwt_wcorr_kernel<8, true, true>": 128,
}


def test_modwt_wcorr_arguments_rejected_without_gpu():
    from wtmi import _lib
    lib = _lib.load()
    lo = (C.c_double * 8)(*([0.125] * 8))
    hi = (C.c_double * 8)(*([0.125, -0.125] * 4))
    lo_p, hi_p = C.cast(lo, C.c_void_p), C.cast(hi, C.c_void_p)
    N, one = None, C.c_void_p(16)  # a non-NULL pointer no rejected call dereferences
    wc = lambda *a: lib.wtmi_modwt_wcorr(*a)
    assert wc(N, N, 16, 0, 16, lo_p, hi_p, 8, 3, 1, 0, 1.96, N, N, N) == 0         # empty batch
    assert wc(N, N, 16, 0, 16, lo_p, hi_p, 8, 3, 0, 5, 1.96, N, N, N) == 0
    assert wc(N, N, 16, -1, 16, lo_p, hi_p, 8, 3, 1, 0, 1.96, N, N, N) == -1
    assert wc(N, N, 16, 0, 16, N, N, 8, 3, 1, 0, 1.96, N, N, N) == -1              # the bank is host data
    assert wc(N, N, 8, 0, 16, lo_p, hi_p, 8, 3, 1, 0, 1.96, N, N, N) == -1         # ld < n
    assert wc(N, N, 16, 0, 16, lo_p, hi_p, 8, 0, 1, 0, 1.96, N, N, N) == -1        # level < 1
    assert wc(N, N, 16, 0, 16, lo_p, hi_p, 8, 63, 1, 0, 1.96, N, N, N) == -1       # level > 62
    assert wc(N, N, 16, 0, 16, lo_p, hi_p, 8, 3, 2, 0, 1.96, N, N, N) == -1        # boundary
    assert wc(N, N, 16, 0, 16, lo_p, hi_p, 8, 3, 1, -1, 1.96, N, N, N) == -1       # max_lag < 0
    assert wc(N, N, 16, 0, 16, lo_p, hi_p, 8, 3, 1, 16, 1.96, N, N, N) == -1       # max_lag >= n
    assert wc(one, one, 16, 1, 16, lo_p, hi_p, 8, 3, 1, 0, 1.96, N, N, N) == -1    # no stats
    assert wc(N, one, 16, 1, 16, lo_p, hi_p, 8, 3, 1, 0, 1.96, one, N, N) == -1    # no x
    assert wc(one, one, 16, 1, 16, lo_p, hi_p, 8, 3, 1, 0, 1.96, one, one, N) == -1  # xcorr without lags
    assert wc(one, one, 16, 1, 16, lo_p, hi_p, 8, 3, 1, 4, 1.96, one, N, N) == -1  # lags without xcorr
    assert wc(one, N, 16, 1, 16, lo_p, hi_p, 8, 3, 1, 4, 1.96, one, one, N) == -1  # xcorr without y
    assert wc(one, one, 16, 1, 16, lo_p, hi_p, 41, 3, 1, 0, 1.96, one, N, N) == -2
    assert wc(one, one, 16385, 1, 16385, lo_p, hi_p, 8, 3, 1, 0, 1.96, one, N, N) == -2
    assert wc(one, one, 8193, 1, 8193, lo_p, hi_p, 8, 3, 1, 4, 1.96, one, one, N) == -2
    assert wc(one, one, 4096, 1, 4096, lo_p, hi_p, 8, 3, 1, 65, 1.96, one, one, N) == -2


def test_modwt_wcorr_op_registered_and_checked():
    import torch
    from wtmi import ops
    assert hasattr(torch.ops.wtmi, "modwt_wcorr") and len(ops.WCORR_STATS) == 8
    lo, hi, x = [0.5, 0.5], [0.5, -0.5], torch.zeros(2, 32)
    with pytest.raises(ValueError, match="level"):
        ops.modwt_wcorr(x, lo, hi, 0)
    with pytest.raises(ValueError, match="boundary"):
        ops.modwt_wcorr(x, lo, hi, 2, y=x, boundary="reflect")
    with pytest.raises(ValueError, match="ci_level"):
        ops.modwt_wcorr(x, lo, hi, 2, y=x, ci_level=1.0)
    with pytest.raises(ValueError, match="max_lag"):
        ops.modwt_wcorr(x, lo, hi, 2, max_lag=3)  # no second series
    with pytest.raises(ValueError, match="max_lag"):
        ops.modwt_wcorr(x, lo, hi, 2, y=x, max_lag=32)
    with pytest.raises(ValueError, match="same shape"):
        ops.modwt_wcorr(x, lo, hi, 2, y=torch.zeros(2, 31))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.modwt_wcorr(x, lo, hi, 2, y=x)


@pytest.fixture(scope="module")
def table():
    from kernel_meta import LIB, LLVM, kernel_table
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")) or not shutil.which("c++filt"):
        pytest.skip("llvm-readelf / c++filt not available")
    if not os.path.exists(LIB):
        pytest.skip("libwtmi.so not built")
    return kernel_table(LIB)


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_wcorr_kernel_registers(table, kernel):
    assert kernel in table, f"{kernel} not in libwtmi.so"
    r = table[kernel]
    assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (kernel, r)
    assert r["vgpr"] <= BUDGET[kernel], (kernel, r)
