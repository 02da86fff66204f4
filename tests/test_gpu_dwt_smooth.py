"""Fused DWT smoothing ladder with per-level OLS (wtmi_dwt_smooth) against an all-fp64 reference:
oracle.glue_spec.dwt_smooth_signal on oracle.dwt_spec.wavedec of x widened to fp64, then
np.linalg.lstsq and the textbook standard errors of the raw y on each smooth.

Statistics gate, by the rule of DESIGN.md section 4.  E0s is the fp32 floor: the same statistics
from fp64 lstsq over the fp32 smooths of the existing ops.wavedec + ops.waverec (level keep-masks,
trimmed), against the all-fp64 reference -- the largest value over the twelve cases below, params
and bse relative to |param| + bse, rsquared absolute.  Measured on an MI355X: E0s = 2.79e-7, at
(4096, db4, 9).  STATS_GATE = 4 x E0s = 1.12e-6 rounded up to one significant digit = 2e-6; the
fused kernel's own maximum over the cases is 2.79e-7, at the same case (profiles/r08/INDEX.md)."""

import functools
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_helpers import gate, red_series
from oracle import dwt_spec as ds
from oracle import glue_spec as gs

pytestmark = pytest.mark.gpu
TOL = 1e-5           # the DWT gate (tests/test_gpu_modwt_dwt.py), per smooth row, normwise
E0S = 2.79e-7        # measured floor of the composed fp32 path, at (4096, db4, 9)
STATS_GATE = 2e-6    # 4 * E0S = 1.12e-6, rounded up to one significant digit

# (n, bank, level, add_constant, batch)
CASES = [(5, "db4", 2, True, 1), (14, "db4", 1, True, 1), (64, "haar", 5, True, 1),
         (129, "db4", 3, True, 1), (1333, "db4", 7, True, 1), (1000, "sym10", 4, True, 1),
         (4096, "db4", 9, True, 1), (8191, "db4", 9, True, 1), (8192, "db4", 10, True, 1),
         (8193, "db4", 6, True, 1), (129, "db4", 3, False, 1), (1000, "db4", 4, True, 3)]


@functools.lru_cache(maxsize=None)
def bank(name):
    with open(GOLDEN + "/pywt_filters.json") as fh:
        return {k: np.asarray(v) for k, v in json.load(fh)["filters"][name].items()}


def ols64(xc, yc, const):
    """One STATS row from fp64 lstsq and the textbook standard errors."""
    X = np.column_stack([np.ones_like(xc), xc]) if const else xc[:, None]
    df = xc.size - X.shape[1]
    tss = float(((yc - yc.mean()) ** 2).sum()) if const else float(yc @ yc)
    beta = np.linalg.lstsq(X, yc, rcond=None)[0]
    ssr = float(((yc - X @ beta) ** 2).sum())
    bse = np.sqrt(ssr / df * np.diag(np.linalg.inv(X.T @ X)))
    pad = [] if const else [0.0]
    return np.array([*pad, *beta][:2] + [*pad, *bse][:2] + [1 - ssr / tss, ssr, xc.size, df])


def rows_stats64(smooths, y, const):
    """[B, level, n] smooths (any float type) and raw [B, n] outputs -> [B, level, 8] in fp64."""
    return np.array([[ols64(s.astype(np.float64), yb.astype(np.float64), const) for s in sb]
                     for sb, yb in zip(smooths, y)])


@functools.lru_cache(maxsize=None)
def case(n, name, level, const, batch):
    """Inputs x, outputs y ([batch, n] float32), the fp64 smooths [batch, level, n] and their fits."""
    rng = np.random.default_rng(n + level)
    x = np.stack([red_series(rng, n) for _ in range(batch)])
    y = np.stack([(0.8 * x[b] + 0.5 + 0.5 * red_series(rng, n)).astype(np.float32) for b in range(batch)])
    f = bank(name)
    sm = []
    for xb in x.astype(np.float64):
        d = gs.dwt_smooth_signal(ds.wavedec(xb, f["dec_lo"], f["dec_hi"], level), level, xb,
                                 f["rec_lo"], f["rec_hi"])
        sm.append([d[l]["signal"] for l in range(1, level + 1)])
    sm = np.array(sm)
    return x, y, sm, rows_stats64(sm, y, const)


def stats_err(got, ref):
    """Params and bse relative to |param| + bse, rsquared absolute; nobs and df_resid exact."""
    np.testing.assert_array_equal(got[..., 6:8], ref[..., 6:8])
    scale = np.abs(ref[..., 0:2]) + ref[..., 2:4]
    scale = np.where(scale > 0, scale, 1.0)  # const / bse_const of the no-constant model are 0
    return max(np.abs((got[..., 0:2] - ref[..., 0:2]) / scale).max(),
               np.abs((got[..., 2:4] - ref[..., 2:4]) / scale).max(),
               np.abs(got[..., 4] - ref[..., 4]).max())


def strided(a):
    """[B, n] on the device as a view of a wider buffer (ld = n + 5) when B > 1."""
    t = torch.zeros((a.shape[0], a.shape[1] + 5), device="cuda")
    t[:, :a.shape[1]] = torch.tensor(a, device="cuda")
    return t[:, :a.shape[1]] if a.shape[0] > 1 else t[:, :a.shape[1]].contiguous()


@pytest.mark.parametrize("n,name,level,const,batch", CASES)
def test_smooths_and_stats_match_fp64_reference(n, name, level, const, batch):
    from wtmi import ops
    x, y, want, ref = case(n, name, level, const, batch)
    f = bank(name)
    res = ops.dwt_smooth(strided(x), f["dec_lo"], f["rec_lo"], level, y=strided(y), add_constant=const)
    got = res["smooth"].cpu().numpy().astype(np.float64)
    assert got.shape == want.shape == (batch, level, n) and res["stats"].shape == (batch, level, 8)
    gate("smooth", np.linalg.norm(got - want, axis=-1) / np.linalg.norm(want, axis=-1), TOL)
    gate("stats", stats_err(res["stats"].cpu().numpy(), ref), STATS_GATE)
    only = ops.dwt_smooth(strided(x), f["dec_lo"], f["rec_lo"], level)  # the launch without moments
    assert only["stats"] is None and torch.equal(only["smooth"], res["smooth"])


def test_zero_input_gives_nan_slope_and_mean_intercept():
    from wtmi import ops
    n, f = 200, bank("db4")
    y = red_series(np.random.default_rng(1), n)
    s = ops.dwt_smooth(torch.zeros(1, n, device="cuda"), f["dec_lo"], f["rec_lo"], 3,
                       y=torch.tensor(y[None], device="cuda"), want_smooth=False)["stats"][0].cpu().numpy()
    assert np.isnan(s[:, [1, 2, 3]]).all()  # slope, bse_const, bse_slope
    np.testing.assert_allclose(s[:, 0], y.astype(np.float64).mean(), rtol=0, atol=TOL * np.abs(y).max())


def test_src_layers_return_the_same_smooths_and_fits():
    from src import dwt
    a, b = case(129, "db4", 3, True, 1), case(1333, "db4", 3, True, 1)
    data = [dwt.DataForDWT(c[0][0], "db4", 3) for c in (a, b)]
    for d, got in zip(data, dwt.smooth_signal_batch(data)):
        res = dwt.run_dwt(d)
        res.smooth_signal(d.y_values, d.mother_wavelet)
        assert list(got) == list(res.smoothed_signal_dict) == [3, 2, 1]
        for lvl, old in res.smoothed_signal_dict.items():
            np.testing.assert_allclose(got[lvl]["signal"], old["signal"], rtol=0,
                                       atol=2e-5 * np.abs(old["signal"]).max())
    fits = dwt.wavelet_approximation_batch([(a[0][0], a[1][0]), (b[0][0], b[1][0])], 3, "db4")
    for fit, c in zip(fits, (a, b)):
        assert fit.names == ["S_1", "S_2", "S_3"] and fit.nobs == c[0].shape[1]
        got = np.concatenate([fit.params, fit.bse, fit.rsquared[:, None], c[3][0][:, 5:8]], axis=1)
        gate("fit", stats_err(got, c[3][0]), STATS_GATE)
