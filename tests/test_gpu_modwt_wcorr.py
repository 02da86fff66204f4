"""Fused MODWT wavelet variance / correlation / lagged cross-correlation (wtmi_modwt_wcorr,
ops.modwt_wcorr) against a plain fp64 statement of the estimators over
oracle.modwt_spec.modwt_direct rows of the fp32 inputs widened to fp64.

Error metric (``wcorr_err``): variances relative, covariance |d| / sqrt(var_x var_y),
correlation, its interval and the cross-correlations absolute; nobs, n_eff and the NaN
positions exact.

Gate, by the rule of test_gpu_dwt_tsr and test_gpu_modwt_mra.  E0 is the fp32 floor: the same
metric for the composed route that existed before -- fp64 numpy sums (``wcorr64``) over the fp32
rows of ops.modwt -- the largest value over CASES and both boundary modes.  GATE = 4 x E0 rounded
up to one significant digit.  Measured: E0 = 4.96e-6 (the composed rows of the series offset by
500, brick wall; every other case stays under 7.2e-7), gate 2e-5; the fused kernel's largest
error over the same cases is 6.5e-7 (it runs on x - x[0])."""

import functools
import math
from statistics import NormalDist

import numpy as np
import pytest
import torch

from gpu_helpers import gate, red_series
from oracle import modwt_spec as ms
from test_gpu_dwt_tsr import bank, strided

pytestmark = pytest.mark.gpu
E0 = 4.96e-6  # measured floor of the composed fp32 path, at (1333, db4, 6, offset 500), brick wall
GATE = 2e-5   # 4 * E0 = 1.98e-5, rounded up to one significant digit
Z = NormalDist().inv_cdf(0.975)

# (n, bank, J, K, batch, offset).  8: M_3 = 1 (corr = +-1, no interval); 13: brick wall L_2 = 22 > n
# (a NaN row with nobs 0), periodic lags wrap; 200: strided batch, M = 193, 179, 151, 95; sym10: 20
# taps; 1333 / offset 500: the app's length and the shift by x[0]; 4096: float4 path, K at its
# limit; 8192: the largest row with lags (M_10 = 1031); 8196 / 16384: lag-0 path above 8192 and at
# its limit; 16385 and 8196 with lags: the composed fallback
CASES = [(8, "haar", 3, 0, 1, 0), (13, "db4", 2, 3, 1, 0), (200, "db4", 4, 12, 3, 0),
         (1000, "sym10", 4, 36, 1, 0), (1333, "db4", 6, 36, 1, 500), (4096, "db4", 8, 64, 2, 0),
         (8192, "db4", 10, 64, 1, 0), (8196, "db4", 4, 0, 1, 0), (16384, "db4", 10, 0, 1, 0),
         (16385, "db4", 3, 0, 1, 0), (8196, "db4", 4, 8, 1, 0)]


def wcorr64(wx, wy, L, K, periodic):
    """stats [J, 8] and xcorr [J, 2K + 1] of detail rows wx, wy [J, n] (include/wtmi.h)."""
    J, n = wx.shape
    stats, xc = np.full((J, 8), np.nan), np.full((J, 2 * K + 1), np.nan)
    for j in range(1, J + 1):
        t0 = 0 if periodic else min(n, (2 ** j - 1) * (L - 1))
        M = n - t0
        stats[j - 1, 4] = max(M, 0)
        if M <= 0:
            continue
        a, b = wx[j - 1], wy[j - 1]
        vx, vy, cov = a[t0:] @ a[t0:] / M, b[t0:] @ b[t0:] / M, a[t0:] @ b[t0:] / M
        neff = n // 2 ** j - (0 if periodic else math.ceil((L - 2) * (1 - 2.0 ** -j)))
        den = np.sqrt(vx * vy) if vx > 0 and vy > 0 else np.nan
        corr, hw = cov / den, Z / np.sqrt(neff - 3) if neff > 3 else np.nan
        with np.errstate(all="ignore"):
            stats[j - 1] = [vx, vy, cov, corr, M, np.tanh(np.arctanh(corr) - hw), np.tanh(np.arctanh(corr) + hw), neff]
        for lag in range(-K, K + 1) if K else ():
            t = np.arange(n) if periodic else np.arange(max(t0, t0 - lag), min(n, n - lag))
            xc[j - 1, lag + K] = a[t] @ b[(t + lag) % n] / M / den
    return stats, xc


@functools.lru_cache(maxsize=None)
def case(n, name, J, K, batch, offset):
    """Pairs x, y [batch, n] (y lags x by 3 samples) and, per boundary mode, their fp64 tables."""
    rng = np.random.default_rng(n + J)
    x = np.stack([red_series(rng, n) + np.float32(offset) for _ in range(batch)])
    y = np.stack([(np.roll(0.8 * xb, 3) + 0.5 * red_series(rng, n)).astype(np.float32) for xb in x])
    f = bank(name)
    w = [[ms.modwt_direct(v, f["dec_lo"], f["dec_hi"], J)[:J] for v in s] for s in (x, y)]
    ref = {p: [wcorr64(wx, wy, len(f["dec_lo"]), K, p) for wx, wy in zip(*w)] for p in (False, True)}
    return x, y, ref


def wcorr_err(stats, xc, ref):
    """The largest error of one pair's tables against ``ref`` = (stats, xcorr)."""
    rs, rx = ref
    np.testing.assert_array_equal(stats[:, [4, 7]], rs[:, [4, 7]])
    np.testing.assert_array_equal(np.isnan(stats), np.isnan(rs))
    errs = [0.0, np.nanmax(np.abs(stats[:, :2] / rs[:, :2] - 1), initial=0.0),
            np.nanmax(np.abs(stats[:, 2] - rs[:, 2]) / np.sqrt(rs[:, 0] * rs[:, 1]), initial=0.0),
            np.nanmax(np.abs(stats[:, [3, 5, 6]] - rs[:, [3, 5, 6]]), initial=0.0)]
    if xc.shape[1]:  # none without lags
        np.testing.assert_array_equal(np.isnan(xc), np.isnan(rx))
        errs.append(np.nanmax(np.abs(xc - rx), initial=0.0))
    return max(errs)


@pytest.mark.parametrize("boundary", ["brickwall", "periodic"])
@pytest.mark.parametrize("n,name,J,K,batch,offset", CASES)
def test_stats_and_xcorr_match_fp64_reference(n, name, J, K, batch, offset, boundary):
    from wtmi import ops
    x, y, ref = case(n, name, J, K, batch, offset)
    f = bank(name)
    res = ops.modwt_wcorr(strided(x), f["dec_lo"], f["dec_hi"], J, y=strided(y), max_lag=K, boundary=boundary)
    assert res["stats"].shape == (batch, J, 8) and (res["xcorr"] is None) == (K == 0)
    stats = res["stats"].cpu().numpy()
    xc = res["xcorr"].cpu().numpy() if K else np.empty((batch, J, 0))
    assert xc.shape == (batch, J, 2 * K + 1 if K else 0)
    err = [wcorr_err(stats[b], xc[b], ref[boundary == "periodic"][b]) for b in range(batch)]
    if K:
        np.testing.assert_array_equal(stats[..., 3], xc[..., K])  # lag 0 is corr itself
        if n >= 200:  # y lags x by 3 samples: the fine scale peaks there
            assert (np.argmax(xc[:, 0], axis=-1) == K + 3).all()
    gate(f"wcorr[{boundary}]", err, GATE)


def test_single_series_gives_the_variance_alone():
    from wtmi import ops
    x, _, ref = case(200, "db4", 4, 12, 3, 0)
    f = bank("db4")
    res = ops.modwt_wcorr(strided(x), f["dec_lo"], f["dec_hi"], 4)
    got = res["stats"].cpu().numpy()
    assert res["xcorr"] is None and np.isnan(got[..., [1, 2, 3, 5, 6]]).all()
    want = np.stack([r[0] for r in ref[False]])
    np.testing.assert_array_equal(got[..., [4, 7]], want[..., [4, 7]])
    gate("variance alone", np.abs(got[..., 0] / want[..., 0] - 1), GATE)


def test_constant_series_has_zero_variance_and_no_correlation():
    from wtmi import ops
    _, y, _ = case(200, "db4", 4, 12, 3, 0)
    f = bank("db4")
    res = ops.modwt_wcorr(torch.full((1, 200), 500.25, device="cuda"), f["dec_lo"], f["dec_hi"], 4,
                          y=torch.tensor(y[:1], device="cuda"), max_lag=5)
    s = res["stats"][0].cpu().numpy()
    assert (s[:, [0, 2]] == 0).all() and (s[:, 1] > 0).all() and np.isnan(s[:, [3, 5, 6]]).all()
    assert np.isnan(res["xcorr"].cpu().numpy()).all()


def test_transform_and_src_layers_return_the_same_numbers():
    from src import modwt
    from wtmi import ops, transforms
    x, y, _ = case(1333, "db4", 6, 36, 1, 500)
    f = bank("db4")
    res = ops.modwt_wcorr(torch.tensor(x, device="cuda"), f["dec_lo"], f["dec_hi"], 6,
                          y=torch.tensor(y, device="cuda"), max_lag=36)
    s, c = res["stats"][0].cpu().numpy(), res["xcorr"][0].cpu().numpy()
    for r in (transforms.wavelet_correlation(x[0], y[0], 6, "db4", max_lag=36),
              modwt.wavelet_correlation_series(x[0], y[0], 6, max_lag=36)):
        assert r.names == [f"D_{j}" for j in range(1, 7)] and list(r.lags) == list(range(-36, 37))
        got = np.column_stack([r.variance_x, r.variance_y, r.covariance, r.correlation, r.nobs, r.ci])
        np.testing.assert_array_equal(got, s[:, :7])
        np.testing.assert_array_equal(r.cross_correlation, c)
    v = transforms.wavelet_variance(x, 6, "db4")
    assert isinstance(v, list) and np.isnan(v[0].correlation).all()
    np.testing.assert_array_equal(v[0].variance_x, s[:, 0])
