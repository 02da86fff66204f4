"""The size limits that wtmi/ops.py restates (TSR_*, SMOOTH_*, MRA_*, WCORR_*) against the ones the
fused entry points enforce.  Every entry point checks its limits before its empty-batch return, so
calls with batch = 0 and NULL data pointers touch no device: exactly at a Python limit the call
returns 0, one past it the entry point's own rejection (-2 unsupported size; -1 for the level
bounds that are argument errors)."""

import ctypes as C

import pytest


@pytest.fixture(scope="module")
def env():
    from wtmi import _lib, ops
    lo = (C.c_double * 42)(*([0.125] * 42))
    hi = (C.c_double * 42)(*([0.125, -0.125] * 21))
    return _lib.load(), ops, C.cast(lo, C.c_void_p), C.cast(hi, C.c_void_p)


N = None


def test_dwt_tsr_limits(env):
    lib, ops, lo, hi = env

    def tsr(n, taps, level):
        return lib.wtmi_dwt_tsr(N, N, n, 0, n, lo, hi, lo, hi, taps, level, 1, N, N, N)

    assert tsr(ops.TSR_MAX_N, ops.TSR_MAX_TAPS, ops.SMOOTH_MAX_LEVEL) == 0
    assert tsr(ops.TSR_MAX_N + 1, 8, 3) == -2
    assert tsr(64, ops.TSR_MAX_TAPS + 2, 3) == -2  # the next even length
    assert tsr(64, 8, ops.SMOOTH_MAX_LEVEL + 1) == -1  # the two pyramids share their level bound


def test_dwt_smooth_limits(env):
    lib, ops, lo, hi = env

    def smooth(n, taps, level):
        return lib.wtmi_dwt_smooth(N, N, n, 0, n, lo, lo, taps, level, 1, N, N, N)

    assert smooth(ops.TSR_MAX_N, ops.TSR_MAX_TAPS, ops.SMOOTH_MAX_LEVEL) == 0
    assert smooth(ops.TSR_MAX_N + 1, 8, 3) == -2
    assert smooth(64, ops.TSR_MAX_TAPS + 2, 3) == -2
    assert smooth(64, 8, ops.SMOOTH_MAX_LEVEL + 1) == -2


def test_modwt_mra_limits(env):
    lib, ops, lo, hi = env

    def mra(n, taps, level):
        return lib.wtmi_modwt_mra(N, N, n, 0, n, lo, hi, taps, level, 1, N, N, N, N)

    def rows(n, taps, level):
        return lib.wtmi_modwt_mra_rows(N, 0, n, lo, hi, taps, level, N, N)

    for fn in (mra, rows):
        assert fn(ops.MRA_MAX_N, ops.MRA_MAX_TAPS, ops.MRA_MAX_LEVEL) == 0
        assert fn(ops.MRA_MAX_N + 1, 8, 3) == -2
        assert fn(64, ops.MRA_MAX_TAPS + 1, 3) == -2
        assert fn(64, 8, ops.MRA_MAX_LEVEL + 1) == -1


def test_modwt_wcorr_limits(env):
    lib, ops, lo, hi = env

    def wcorr(n, taps, level, max_lag):
        return lib.wtmi_modwt_wcorr(N, N, n, 0, n, lo, hi, taps, level, 1, max_lag, 1.96, N, N, N)

    assert wcorr(ops.WCORR_MAX_N, ops.MRA_MAX_TAPS, ops.MRA_MAX_LEVEL, 0) == 0
    assert wcorr(ops.WCORR_MAX_LAG_N, ops.MRA_MAX_TAPS, ops.MRA_MAX_LEVEL, ops.WCORR_MAX_LAG) == 0
    assert wcorr(ops.WCORR_MAX_N + 1, 8, 3, 0) == -2
    assert wcorr(ops.WCORR_MAX_LAG_N + 1, 8, 3, 1) == -2
    assert wcorr(4096, 8, 3, ops.WCORR_MAX_LAG + 1) == -2
    assert wcorr(64, ops.MRA_MAX_TAPS + 1, 3, 0) == -2
    assert wcorr(64, 8, ops.MRA_MAX_LEVEL + 1, 0) == -1
