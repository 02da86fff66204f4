"""Host side of the time-localized wavelet correlation (no GPU): the window builders, the argument
checks of ops.modwt_lwcorr (raised before any device work), the effective counts of the interval
and the return codes of wtmi_modwt_lwcorr, reached with an empty batch as in
test_fused_limits_host."""

import ctypes as C

import numpy as np
import pytest
import torch


def test_window_builders():
    from wtmi.transforms import local_window
    np.testing.assert_array_equal(local_window("uniform", 3), [1, 1, 1, 1])
    np.testing.assert_allclose(local_window("bartlett", 3), [1, 0.75, 0.5, 0.25], rtol=1e-15)
    np.testing.assert_allclose(local_window("gaussian", 6), np.exp(-np.arange(7) ** 2 / 8.0), rtol=1e-15)
    np.testing.assert_array_equal(local_window("gaussian", 0), [1])
    np.testing.assert_array_equal(local_window([2, 1, 0], 2), [2, 1, 0])
    for bad, H in (("hann", 3), ([1, 1], 2), ("uniform", -1)):
        with pytest.raises(ValueError):
            local_window(bad, H)


@pytest.mark.parametrize("kw,msg", [
    (dict(window=[1, -0.5]), "finite and >= 0"), (dict(window=[0, 1]), "must be > 0"),
    (dict(window=[[1, 1]]), "half_width"), (dict(window=np.ones(5), boundary="periodic"), "count twice"),
    (dict(window=[1], boundary="reflect"), "boundary"), (dict(window=[1], y=None), "no output requested")])
def test_validation_comes_before_the_device(kw, msg):
    from wtmi import ops
    x = torch.zeros(8)  # a CPU tensor: reaching the device check would raise RuntimeError instead
    with pytest.raises(ValueError, match=msg):
        ops.modwt_lwcorr(x, [0.5, 0.5], [0.5, -0.5], 2, **{"y": x, **kw})


def test_effective_counts_and_result_shapes():
    from wtmi.transforms import LocalWaveletCorrelation, local_n_eff
    # uniform, H = 2, n = 8, haar: K(s) = the counted coefficients, t0 = 1 and 3 for the brick wall
    np.testing.assert_array_equal(local_n_eff(np.ones(3), 8, 2, 2), [[1, 1, 2, 2, 2, 2, 2, 1], [0, 0, 0, 0, 1, 1, 1, 0]])
    np.testing.assert_array_equal(local_n_eff(np.ones(3), 8, 2, 2, "periodic"), [[2] * 8, [1] * 8])
    for n, H in ((9, 4), (1001, 500)):  # the whole series, periodic: floor(n / 2^j)
        np.testing.assert_array_equal(local_n_eff(np.ones(H + 1), n, 8, 3, "periodic"),
                                      np.repeat([[n // 2], [n // 4], [n // 8]], n, 1))
    # weights (0.5, 1, 0.5): K = 2^2 / 1.5 = 2.67
    np.testing.assert_array_equal(local_n_eff([1, 0.5], 4, 2, 1, "periodic"), [[1] * 4])
    assert [f for f in LocalWaveletCorrelation.__dataclass_fields__] == [
        "names", "variance_x", "variance_y", "covariance", "correlation", "ci", "n_eff", "half_width"]


def test_c_abi_return_codes():
    from wtmi import _lib, ops
    lib = _lib.load()
    lo = C.cast((C.c_double * 42)(*([0.125] * 42)), C.c_void_p)
    p = C.cast((C.c_double * 4)(), C.c_void_p)  # never read: the batch is empty or the call is refused

    def lw(n=64, taps=8, level=3, boundary=1, H=4, window=p, y=p, corr=p, mom=p, ld=None, ld_out=None, bank=lo):
        return lib.wtmi_modwt_lwcorr(p, y, ld or n, 0, n, bank, lo, taps, level, boundary, window, H, corr, mom,
                                     ld_out or n, None)

    assert lw() == 0 and lw(corr=None) == 0 and lw(y=None, corr=None) == 0
    assert lw(ops.LWCORR_MAX_N, ops.MRA_MAX_TAPS, ops.MRA_MAX_LEVEL, H=ops.LWCORR_MAX_HALF_WIDTH) == 0
    assert lw(boundary=0, n=9, H=4) == 0
    bad = [dict(bank=None), dict(window=None), dict(ld=63), dict(ld_out=63), dict(level=0),
           dict(level=ops.MRA_MAX_LEVEL + 1), dict(boundary=2), dict(H=-1), dict(boundary=0, n=8, H=4),
           dict(corr=None, mom=None), dict(y=None)]
    assert [lw(**kw) for kw in bad] == [-1] * len(bad)
    assert lw(n=ops.LWCORR_MAX_N + 1) == -2 and lw(taps=ops.MRA_MAX_TAPS + 1) == -2
    assert lw(n=4096, H=ops.LWCORR_MAX_HALF_WIDTH + 1) == -2
