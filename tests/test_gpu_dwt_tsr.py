"""Fused DWT time-scale regression (wtmi_dwt_tsr / wtmi_rows_ols) against an all-fp64
reference: oracle.dwt_spec wavedec / waverec of the inputs widened to fp64, np.linalg.lstsq and
the textbook standard errors.

Statistics gate.  E0 is the fp32 floor: the same statistics from fp64 lstsq over the fp32
components of the existing ops.wavedec + ops.waverec, against the all-fp64 reference -- the
largest value over every case below, params and bse relative to |param| + bse, rsquared
absolute.  STATS_GATE = 4 x E0 rounded up to one significant digit: room for the fused
kernel's own summation / FMA order (a few ulps per level, at most 11 levels), nowhere near a
wrong tap or edge sample (1e-2 or worse)."""

import functools

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_helpers import gate, red_series
from oracle import dwt_spec as ds

pytestmark = pytest.mark.gpu
TOL = 1e-5          # the DWT gate (tests/test_gpu_modwt_dwt.py)
E0 = 6.21e-6        # measured floor of the composed fp32 path, at (8191, db4, 9), related output
STATS_GATE = 3e-5   # 4 * E0 = 2.5e-5, rounded up to one significant digit

# (n, bank, level, add_constant, batch): 5 wraps the reflection more than once; 129 / 8191 / 8193
# are odd (nobs = n + 1); 8192 / 8193 sit either side of the fused / composed boundary; sym10
# has 20 taps; batch 3 goes in as a strided (ld > n) view
CASES = [(5, "db4", 2, True, 1), (14, "db4", 1, True, 1), (64, "haar", 6, True, 1),
         (129, "db4", 3, True, 1), (1333, "db4", 6, True, 1), (1000, "sym10", 4, True, 1),
         (8191, "db4", 9, True, 1), (8192, "db4", 10, True, 1), (8193, "db4", 6, True, 1),
         (100, "db4", 0, True, 1), (129, "db4", 3, False, 1), (1000, "db4", 4, True, 3)]


@functools.lru_cache(maxsize=None)
def bank(name):
    import json
    with open(GOLDEN + "/pywt_filters.json") as fh:
        return {k: np.asarray(v) for k, v in json.load(fh)["filters"][name].items()}


def ols64(xc, yc, const):
    """One STATS row from fp64 lstsq and the textbook standard errors."""
    X = np.column_stack([np.ones_like(xc), xc]) if const else xc[:, None]
    df = xc.size - X.shape[1]
    tss = float(((yc - yc.mean()) ** 2).sum()) if const else float(yc @ yc)
    if const and np.ptp(xc) <= 1e-9 * np.abs(xc).max():  # constant regressor (haar S_6 of 64
        return np.array([yc.mean(), np.nan, np.nan, np.nan, 0.0, tss, xc.size, df])  # samples)
    beta = np.linalg.lstsq(X, yc, rcond=None)[0]
    ssr = float(((yc - X @ beta) ** 2).sum())
    bse = np.sqrt(ssr / df * np.diag(np.linalg.inv(X.T @ X)))
    pad = [] if const else [0.0]
    return np.array([*pad, *beta][:2] + [*pad, *bse][:2] + [1 - ssr / tss, ssr, xc.size, df])


def components64(v, f, level):
    c = ds.wavedec(v.astype(np.float64), f["dec_lo"], f["dec_hi"], level)
    return np.stack([ds.waverec([a if k == j else np.zeros_like(a) for k, a in enumerate(c)],
                                f["rec_lo"], f["rec_hi"]) for j in range(level + 1)])


@functools.lru_cache(maxsize=None)
def case(n, name, level, const, batch):
    """Inputs x, the related and the unrelated outputs ([2, batch, n]) and their references."""
    rng = np.random.default_rng(n + level)
    x = np.stack([red_series(rng, n) for _ in range(batch)])
    rel = np.stack([(0.8 * x[b] + 0.5 + 0.5 * red_series(rng, n)).astype(np.float32) for b in range(batch)])
    unrel = np.stack([red_series(np.random.default_rng(7 * n + b), n) for b in range(batch)])
    f = bank(name)
    cx = np.stack([components64(x[b], f, level) for b in range(batch)])
    cy = np.stack([[components64(y[b], f, level) for b in range(batch)] for y in (rel, unrel)])
    stats = np.array([[[ols64(cx[b, k], cyo[b, k], const) for k in range(level + 1)]
                       for b in range(batch)] for cyo in cy])
    # columns 8, 9: the sizes of intercept and slope a component's data can resolve (stats_err)
    ymax, xmax = np.abs(cy).max(axis=-1), np.abs(cx).max(axis=-1)[None]
    return x, np.stack([rel, unrel]), cx, cy, np.concatenate([stats, np.stack([ymax, ymax / xmax], -1)], -1)


def stats_err(got, ref):
    """Params and bse relative to |param| + bse, rsquared absolute (nobs, df_resid and the
    NaNs of a constant regressor exact).  Where the reference fit is exact (haar D_6 of 64
    samples: two-valued components, ssr = bse = 0 and here const = 0 analytically) that scale
    vanishes; those components are measured against the sizes in ref's columns 8, 9 instead,
    the floor rule of the component rows."""
    np.testing.assert_array_equal(got[..., 6:8], ref[..., 6:8])
    np.testing.assert_array_equal(np.isnan(got[..., :8]), np.isnan(ref[..., :8]))
    scale = np.abs(ref[..., 0:2]) + np.nan_to_num(ref[..., 2:4])
    if ref.shape[-1] > 8:
        scale = scale + np.where(1 - ref[..., 4:5] <= 1e-12, ref[..., 8:10], 0.0)
    scale = np.where(scale > 0, scale, 1.0)  # const / bse_const of the no-constant model are 0
    return max(np.nanmax(np.abs((got[..., 0:2] - ref[..., 0:2]) / scale)),
               np.nanmax(np.abs((got[..., 2:4] - ref[..., 2:4]) / scale)),
               np.abs(got[..., 4] - ref[..., 4]).max())


def strided(a):
    """[B, n] on the device as a view of a wider buffer (ld = n + 5) when B > 1."""
    t = torch.zeros((a.shape[0], a.shape[1] + 5), device="cuda")
    t[:, :a.shape[1]] = torch.tensor(a, device="cuda")
    return t[:, :a.shape[1]] if a.shape[0] > 1 else t[:, :a.shape[1]].contiguous()


@pytest.mark.parametrize("n,name,level,const,batch", CASES)
def test_stats_and_components_match_fp64_reference(n, name, level, const, batch):
    from wtmi import ops
    x, ys, cx, cy, ref = case(n, name, level, const, batch)
    f = bank(name)
    for o in range(2):
        res = ops.dwt_time_scale_regression(strided(x), strided(ys[o]), f["dec_lo"], f["dec_hi"],
                                            f["rec_lo"], f["rec_hi"], level, add_constant=const,
                                            want_components=True)
        got, want = res["components"].cpu().numpy().astype(np.float64), np.stack([cx, cy[o]], axis=1)
        assert got.shape == want.shape and res["stats"].shape == (batch, level + 1, 8)
        # per row normwise, with the floor of test_gpu_modwt_dwt for rows that vanish analytically
        floor = 0.1 * np.abs(want).max(axis=(0, 2, 3))[None, :, None] * np.sqrt(want.shape[-1])
        gate(f"components[{o}]", np.linalg.norm(got - want, axis=-1) /
             (np.linalg.norm(want, axis=-1) + floor), TOL)
        gate(f"stats[{o}]", stats_err(res["stats"].cpu().numpy(), ref[o]), STATS_GATE)


def test_fused_matches_composed_pieces():
    from wtmi import ops
    n, name, level = 8192, "db4", 10
    x, ys, _, _, _ = case(n, name, level, True, 1)
    f = bank(name)
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(ys[0], device="cuda")
    fused = ops.dwt_time_scale_regression(xd, yd, f["dec_lo"], f["dec_hi"], f["rec_lo"], f["rec_hi"], level)
    masks = [1 << k for k in range(level + 1)]
    cxd, cyd = (ops.waverec(ops.wavedec(t, f["dec_lo"], f["dec_hi"], level)[0], n, f["rec_lo"],
                            f["rec_hi"], level, masks)[0] for t in (xd, yd))
    composed = ops.rows_ols(cxd, cyd).cpu().numpy()
    gate("fused vs composed", stats_err(fused["stats"][0].cpu().numpy(), composed), STATS_GATE)


def test_constant_input_gives_nan_slope_and_mean_intercept():
    from wtmi import ops
    n, name, level = 200, "db4", 3
    f = bank(name)
    y = red_series(np.random.default_rng(1), n)
    s = ops.dwt_time_scale_regression(torch.zeros(1, n, device="cuda"), torch.tensor(y[None], device="cuda"),
                                      f["dec_lo"], f["dec_hi"], f["rec_lo"], f["rec_hi"], level
                                      )["stats"][0].cpu().numpy()
    assert np.isnan(s[:, [1, 2, 3]]).all()  # slope, bse_const, bse_slope
    np.testing.assert_allclose(s[:, 0], components64(y, f, level).mean(axis=1), rtol=0,
                               atol=TOL * np.abs(y).max())


def test_src_layers_return_the_same_fits():
    """src.dwt.time_scale_regression_batch (pairs of two lengths, one launch each) and
    src.modwt.time_scale_regression_batch (rows_ols over existing component rows)."""
    from src import dwt, modwt
    a, b = case(129, "db4", 3, True, 1), case(1333, "db4", 3, True, 1)
    fits = dwt.time_scale_regression_batch([(a[0][0], a[1][0, 0]), (b[0][0], b[1][1, 0])], 3, "db4")
    assert fits[0].names == ["S_3", "D_3", "D_2", "D_1"] and (fits[0].nobs, fits[1].nobs) == (130, 1334)
    for fit, ref in ((fits[0], a[4][0, 0]), (fits[1], b[4][1, 0]),
                     (modwt.time_scale_regression_batch(a[2][0], a[3][0, 0]), a[4][0, 0])):
        got = np.concatenate([fit.params, fit.bse, fit.rsquared[:, None], ref[:, 5:8]], axis=1)
        gate("fit", stats_err(got, ref), STATS_GATE)
        np.testing.assert_allclose(fit.tvalues, fit.params / fit.bse, rtol=1e-15)
