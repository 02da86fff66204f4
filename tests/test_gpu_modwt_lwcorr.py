"""Fused time-localized (rolling-window) wavelet correlation (wtmi_modwt_lwcorr, ops.modwt_lwcorr)
against a plain fp64 statement of its definition: np.convolve of the window with the counted
products of oracle.modwt_spec.modwt_direct rows of the fp32 inputs widened to fp64.

Error metric (``lw_err``): correlation absolute, the two local variances relative, the local
covariance |d| / sqrt(var_x var_y); every centre counts, NaN positions exact.

Gate, by the rule of test_gpu_modwt_wcorr.  E0 is the fp32 floor: the same
metric for the composed route (ops._lwcorr_composed: fp64 torch windowed sums over the fp32 rows of
ops.modwt), the largest value over the offset-0 CASES and both boundary modes, measured on the
MI355X.  GATE = 4 x E0 rounded up to one significant digit.  Measured: E0 = 2.66e-5 (at (8192, db4,
10, H = 64), brick wall: the relative error of a local variance where the cut window holds few,
small coefficients; every periodic case stays under 4.4e-6), gate 2e-4.  The fused kernel's figure
equals the composed route's in every case and mode to all printed digits (its fp32 rows are formed
by the same FMAs, and both round fp64 sums once), so its largest error is 2.66e-5 as well; the
offset-500 case gives 3.23e-6 (brick wall) and 4.6e-7 (periodic) on both routes and passes the
same gate.  The periodic mode of the last case asks for 2H + 1 = 2051 > n = 2048, which the
definition excludes: there the test checks the refusal."""

import functools
from statistics import NormalDist

import numpy as np
import pytest
import torch

from gpu_helpers import gate, red_series
from oracle import modwt_spec as ms
from test_gpu_dwt_tsr import bank, strided

pytestmark = pytest.mark.gpu
E0 = 2.66e-5  # measured floor of the composed fp32 path, at (8192, db4, 10, 64), brick wall
GATE = 2e-4   # 4 * E0 = 1.07e-4, rounded up to one significant digit

# (n, bank, J, H, window, batch, offset).  8: at j = 3 one counted coefficient, centres whose window
# holds none are NaN; 13: brick wall L_2 = 22 > n (a whole NaN level), periodic wraps with 2H + 1 = 7;
# 200: strided batch; sym10: 20 taps; 1333 / offset 500: the app's length and the shift by x[0];
# 4096: H at its limit; 8192: the largest row; 8196 and H = 1025: the composed fallback
CASES = [(8, "haar", 3, 2, "uniform", 1, 0), (13, "db4", 2, 3, "uniform", 1, 0), (200, "db4", 4, 12, "bartlett", 3, 0),
         (1000, "sym10", 4, 100, "gaussian", 1, 0), (1333, "db4", 6, 128, "uniform", 1, 500),
         (4096, "db4", 8, 1024, "gaussian", 2, 0), (8192, "db4", 10, 64, "uniform", 1, 0),
         (8196, "db4", 4, 16, "uniform", 1, 0), (2048, "db4", 3, 1025, "uniform", 1, 0)]


def theta(window, H):
    k = np.arange(H + 1.0)
    return {"uniform": np.ones(H + 1), "bartlett": 1 - k / (H + 1), "gaussian": np.exp(-k * k / (2 * (H / 3) ** 2))}[window]


def lw64(wx, wy, L, th, periodic):
    """corr [J, n] and moments [J, 3, n] of detail rows wx, wy [J, n] (include/wtmi.h)."""
    J, n = wx.shape
    H, sym = th.size - 1, np.concatenate((th[:0:-1], th))
    corr, mom = np.full((J, n), np.nan), np.full((J, 3, n), np.nan)

    def win(q):
        if periodic:
            return np.convolve(np.concatenate((q[n - H:], q, q[:H])), sym, "valid")
        return np.convolve(q, sym)[H:H + n]

    for j in range(1, J + 1):
        c = np.ones(n) if periodic else (np.arange(n) >= (2 ** j - 1) * (L - 1)).astype(float)
        sw, axx, ayy, axy = win(c), win(c * wx[j - 1] ** 2), win(c * wy[j - 1] ** 2), win(c * wx[j - 1] * wy[j - 1])
        with np.errstate(all="ignore"):
            mom[j - 1] = np.where(sw > 0, np.stack((axx, ayy, axy)) / sw, np.nan)
            corr[j - 1] = np.where((sw > 0) & (axx > 0) & (ayy > 0), np.clip(axy / np.sqrt(axx * ayy), -1, 1), np.nan)
    return corr, mom


@functools.lru_cache(maxsize=None)
def case(n, name, J, H, window, batch, offset):
    """Pairs x, y [batch, n] (y lags x by 3 samples) and, per boundary mode, their fp64 tables."""
    rng = np.random.default_rng(n + J)
    x = np.stack([red_series(rng, n) + np.float32(offset) for _ in range(batch)])
    y = np.stack([(np.roll(0.8 * xb, 3) + 0.5 * red_series(rng, n)).astype(np.float32) for xb in x])
    f = bank(name)
    w = [[ms.modwt_direct(v, f["dec_lo"], f["dec_hi"], J)[:J] for v in s] for s in (x, y)]
    ref = {p: [lw64(wx, wy, len(f["dec_lo"]), theta(window, H), p) for wx, wy in zip(*w)] for p in (False, True)}
    return x, y, ref


def lw_err(corr, mom, ref):
    """The largest error of one pair's tables against ``ref`` = (corr, moments)."""
    rc, rm = ref
    np.testing.assert_array_equal(np.isnan(corr), np.isnan(rc))
    np.testing.assert_array_equal(np.isnan(mom), np.isnan(rm))
    return max(np.nanmax(np.abs(corr - rc), initial=0.0), np.nanmax(np.abs(mom[:, :2] / rm[:, :2] - 1), initial=0.0),
               np.nanmax(np.abs(mom[:, 2] - rm[:, 2]) / np.sqrt(rm[:, 0] * rm[:, 1]), initial=0.0))


def run(x, y, name, J, H, window, boundary, fn=None):
    from wtmi import ops
    f = bank(name)
    if fn is not None:  # the composed route itself (the floor E0)
        return fn(x, y, f["dec_lo"], f["dec_hi"], J, theta(window, H), boundary == "periodic")
    r = ops.modwt_lwcorr(x, f["dec_lo"], f["dec_hi"], J, y=y, window=theta(window, H), boundary=boundary, moments=True)
    return r["corr"], r["moments"]


@pytest.mark.parametrize("boundary", ["brickwall", "periodic"])
@pytest.mark.parametrize("n,name,J,H,window,batch,offset", CASES)
def test_corr_and_moments_match_fp64_reference(n, name, J, H, window, batch, offset, boundary):
    x, y, ref = case(n, name, J, H, window, batch, offset)
    if boundary == "periodic" and 2 * H + 1 > n:  # a coefficient would count twice: refused
        with pytest.raises(ValueError, match="count twice"):
            run(strided(x), strided(y), name, J, H, window, boundary)
        return
    corr, mom = run(strided(x), strided(y), name, J, H, window, boundary)
    assert corr.shape == (batch, J, n) and mom.shape == (batch, J, 3, n) and corr.dtype == mom.dtype == torch.float32
    corr, mom = corr.cpu().numpy().astype(np.float64), mom.cpu().numpy().astype(np.float64)
    gate(f"lwcorr[{boundary}]", [lw_err(corr[b], mom[b], ref[boundary == "periodic"][b]) for b in range(batch)], GATE)


def test_whole_series_window_gives_the_wavelet_correlation_table():
    from wtmi import ops
    x, y, _ = case(1000, "sym10", 4, 100, "gaussian", 1, 0)
    f = bank("db4")
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    r = ops.modwt_lwcorr(xd, f["dec_lo"], f["dec_hi"], 4, y=yd, window=np.ones(1000), moments=True)
    s = ops.modwt_wcorr(xd, f["dec_lo"], f["dec_hi"], 4, y=yd)["stats"][0].cpu().numpy()  # var_x, var_y, cov, corr
    corr, mom = r["corr"][0].cpu().numpy().astype(np.float64), r["moments"][0].cpu().numpy().astype(np.float64)
    gate("corr", np.abs(corr - s[:, 3:4]), GATE)
    gate("variances", np.abs(mom[:, :2] / s[:, :2, None] - 1), GATE)
    gate("covariance", np.abs(mom[:, 2] - s[:, 2:3]) / np.sqrt(s[:, 0:1] * s[:, 1:2]), GATE)


def test_scaled_copy_constant_series_and_single_series():
    from wtmi import _lib, ops
    x, _, _ = case(200, "db4", 4, 12, "bartlett", 3, 0)
    f, th = bank("db4"), theta("bartlett", 12)
    xd = torch.tensor(x, device="cuda")
    pair = ops.modwt_lwcorr(xd, f["dec_lo"], f["dec_hi"], 4, y=-2 * xd, window=th, moments=True)
    corr = pair["corr"].cpu().numpy()
    assert np.isfinite(corr).sum() > 3 * 4 * 100
    gate("y = -2x", np.abs(corr[np.isfinite(corr)].astype(np.float64) + 1), GATE)
    flat = ops.modwt_lwcorr(torch.full((1, 200), 500.25, device="cuda"), f["dec_lo"], f["dec_hi"], 4, y=xd[:1],
                            window=th, moments=True)
    m = flat["moments"][0].cpu().numpy()
    assert np.isnan(flat["corr"].cpu().numpy()).all() and (m[:, 0][~np.isnan(m[:, 0])] == 0).all() and (m[:, 1] > 0).any()
    # a single series: plane 0 of moments alone is written, and there is no corr to ask for
    single = torch.full((3, 4, 3, 200), -7.0, device="cuda")
    args = [xd.data_ptr(), None, 200, 3, 200, f["dec_lo"].ctypes.data, f["dec_hi"].ctypes.data, 8, 4, 1,
            ops._f64_dev(th, xd.device).data_ptr(), 12]
    _lib.call("wtmi_modwt_lwcorr", *args, None, single.data_ptr(), 200, None)
    torch.testing.assert_close(single[:, :, 0], pair["moments"][:, :, 0], rtol=0, atol=0, equal_nan=True)
    assert (single[:, :, 1:] == -7.0).all()
    with pytest.raises(_lib.WtmiError, match="invalid argument"):
        _lib.call("wtmi_modwt_lwcorr", *args, single.data_ptr(), single.data_ptr(), 200, None)
    with pytest.raises(ValueError, match="no output requested"):
        ops.modwt_lwcorr(xd, f["dec_lo"], f["dec_hi"], 4, window=th)


def test_transform_and_src_layers_return_the_same_numbers_and_the_interval():
    from src import modwt
    from wtmi import ops, transforms
    x, y, _ = case(1333, "db4", 6, 128, "uniform", 1, 500)
    f = bank("db4")
    res = ops.modwt_lwcorr(torch.tensor(x, device="cuda"), f["dec_lo"], f["dec_hi"], 6, y=torch.tensor(y, device="cuda"),
                           window=np.ones(129), moments=True)
    corr, mom = res["corr"][0].cpu().numpy(), res["moments"][0].cpu().numpy()
    for r in (transforms.local_wavelet_correlation(x[0], y[0], 6, "db4", 128),
              modwt.local_wavelet_correlation_series(x[0], y[0], 6, 128)):
        assert r.names == [f"D_{j}" for j in range(1, 7)] and r.half_width == 128
        np.testing.assert_array_equal(np.stack((r.variance_x, r.variance_y, r.covariance), 1), mom)
        np.testing.assert_array_equal(r.correlation, corr)
    # level 3 by index sums: K(s) = the counted coefficients (uniform weights), n_eff = floor(K / 8)
    t = np.arange(1333)
    K = np.array([((t >= 49) & (abs(t - s) <= 128)).sum() for s in t])
    np.testing.assert_array_equal(r.n_eff[2], K // 8)
    hw = NormalDist().inv_cdf(0.975) / np.sqrt(np.where(K // 8 > 3, K // 8 - 3, np.nan))
    with np.errstate(all="ignore"):
        zr = np.arctanh(corr[2].astype(np.float64))
        np.testing.assert_allclose(r.ci[2], np.stack((np.tanh(zr - hw), np.tanh(zr + hw)), -1), rtol=1e-12, atol=0)
    v = transforms.local_wavelet_variance(x, 6, "db4", 128)
    assert isinstance(v, list) and np.isnan(v[0].correlation).all() and np.isnan(v[0].variance_y).all()
    np.testing.assert_array_equal(v[0].variance_x, mom[:, 0])
