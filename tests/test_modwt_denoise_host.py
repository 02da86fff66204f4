"""wtmi_modwt_denoise without a GPU: the size limits that wtmi/ops.py restates against the entry
point's own (checked before the empty-batch return, so batch = 0 with NULL data pointers touches no
device), the workspace formula of include/wtmi.h, and the ops layer's operand errors."""

import ctypes as C

import pytest

N = None


def test_modwt_denoise_limits_and_workspace():
    from wtmi import _lib, ops
    lib = _lib.load()
    lo = C.cast((C.c_double * 42)(*([0.125] * 42)), C.c_void_p)

    def den(n, taps, level):
        return lib.wtmi_modwt_denoise(N, n, 0, n, lo, lo, taps, level, 1, 0, 1.0, N, 0, N, n, N, N, N, N)

    assert den(ops.MODWT_DENOISE_MAX_N, ops.MRA_MAX_TAPS, ops.MRA_MAX_LEVEL) == 0
    assert den(ops.MODWT_DENOISE_MAX_N + 1, 8, 3) == -2
    assert den(64, ops.MRA_MAX_TAPS + 1, 3) == -2
    assert den(64, 8, ops.MRA_MAX_LEVEL + 1) == -1
    for rule, shrink in ((-1, 0), (3, 0), (1, -1), (1, 3)):
        assert lib.wtmi_modwt_denoise(N, 64, 0, 64, lo, lo, 8, 3, rule, shrink, 1.0, N, 0, N, 64, N, N, N, N) == -1
    ws = lib.wtmi_modwt_denoise_workspace_bytes
    assert ws(3, 1333, 7) == 0  # V and all seven rows: 8 * 1336 floats of LDS
    # n = 16384: 36864 / 16384 - 1 = 1 resident row, S = level - 1 spilled rows of n floats per series
    assert ws(5, 16384, 10) == 5 * 9 * 16384 * 4
    assert ws(1, 4096, 8) == 0 and ws(2, 4096, 9) == 2 * 1 * 4096 * 4
    assert ws(1, 16385, 3) == -1


def test_modwt_denoise_operands_checked():
    import torch
    from wtmi import ops
    lo, x = [0.5, 0.5], torch.zeros(2, 32)
    for match, kw in (("rule", dict(rule="sure")), ("shrink", dict(shrink="firm")),
                      ("thresholds", dict(rule="fixed")), ("thresholds", dict(thresholds=[1.0, 1.0])),
                      ("thresholds", dict(rule="fixed", thresholds=[1.0, 1.0, 1.0])),
                      ("thresholds", dict(rule="fixed", thresholds=[[[1.0, 1.0]]]))):
        with pytest.raises(ValueError, match=match):
            ops.modwt_denoise(x, lo, lo, 2, **kw)
    with pytest.raises(RuntimeError, match="GPU"):  # a CPU tensor
        ops.modwt_denoise(x, lo, lo, 2)
