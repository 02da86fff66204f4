"""wtmi_dwt_denoise without a GPU: return codes (argument checks return before any launch), the ops
layer's operand errors, and the kernel's register budget from the built library (scripts/kernel_meta.py)."""

import ctypes as C
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# csrc/dwt_denoise.hip keeps about 2 n floats of LDS: 66 KB at n = 8192, two 512-thread workgroups
# per CU = 4 waves per SIMD, so at most 512 / 4 = 128 VGPRs.
KERNEL, BUDGET = "wtmi::dwt_denoise_kernel", 128


def test_dwt_denoise_return_codes_without_gpu():
    from wtmi import _lib
    lib = _lib.load()
    taps = (C.c_double * 42)(*([0.125] * 42))
    t = C.cast(taps, C.c_void_p)
    N, one, inf = None, C.c_void_p(16), float("inf")  # `one`: non-NULL, never dereferenced by a rejected call

    def f(x=one, ld=16, batch=1, n=16, lo=t, hi=t, F=8, level=3, rule=1, shrink=0, mult=1.0, thr=N, thr_ld=0,
          out=one, ld_out=16):
        return lib.wtmi_dwt_denoise(x, ld, batch, n, lo, hi, lo, hi, F, level, rule, shrink, mult, thr, thr_ld,
                                    out, ld_out, N, N, N)

    assert f(x=N, out=N, batch=0) == 0  # empty batch
    assert f(n=8192, ld=8192, ld_out=8192, F=40, level=60, batch=0) == 0  # exactly at the limits
    for bad in (dict(lo=N), dict(hi=N), dict(out=N), dict(ld=15), dict(ld_out=15), dict(level=0), dict(rule=-1),
                dict(rule=3), dict(shrink=-1), dict(shrink=3), dict(mult=-0.5), dict(mult=inf),
                dict(mult=float("nan")), dict(rule=0), dict(rule=0, thr=one, thr_ld=2), dict(batch=-1)):
        assert f(**bad) == -1, bad
    for big in (dict(n=8193, ld=8193, ld_out=8193), dict(F=7), dict(F=42), dict(level=61)):
        assert f(**big) == -2, big


def test_dwt_denoise_op_registered_and_checked():
    import torch
    from wtmi import ops
    assert hasattr(torch.ops.wtmi, "dwt_denoise")
    lo, x = [0.5, 0.5], torch.zeros(2, 32)
    for match, kw in (("rule", dict(rule="sure")), ("shrink", dict(shrink="firm")), ("mult", dict(mult=-1.0)),
                      ("mult", dict(mult=float("nan"))), ("thresholds", dict(rule="fixed")),
                      ("thresholds", dict(thresholds=[1.0, 1.0])),
                      ("thresholds", dict(rule="fixed", thresholds=[1.0, 1.0, 1.0])),
                      ("thresholds", dict(rule="fixed", thresholds=[[[1.0, 1.0]]]))):
        with pytest.raises(ValueError, match=match):
            ops.dwt_denoise(x, lo, lo, lo, lo, 2, **kw)
    for err, level in ((ValueError, 0), (RuntimeError, 2)):  # a bad level; a CPU tensor
        with pytest.raises(err, match="level" if level == 0 else "GPU"):
            ops.dwt_denoise(x, lo, lo, lo, lo, level)


def test_denoise_kernel_registers():
    from kernel_meta import LIB, LLVM, kernel_table
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")) or not shutil.which("c++filt"):
        pytest.skip("llvm-readelf / c++filt not available")
    if not os.path.exists(LIB):
        pytest.skip("libwtmi.so not built")
    r = kernel_table(LIB).get(KERNEL)
    assert r is not None, f"{KERNEL} not in libwtmi.so"
    assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, r
    assert r["vgpr"] <= BUDGET, r
