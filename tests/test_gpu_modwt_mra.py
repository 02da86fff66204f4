"""Fused MODWT multiresolution analysis (wtmi_modwt_mra / wtmi_modwt_mra_rows) against the
all-fp64 reference oracle.modwt_spec.modwtmra(modwt_direct(x)) and smooth_signal of the fp32
inputs widened to fp64; statistics against ols64 of those fp64 rows.

Statistics gate, by the rule of test_gpu_dwt_tsr.  E0 is the fp32 floor: ols64 over the fp32
rows of the composed path that existed before (ops.modwt + one-bit-mask ops.imodwt) against
the all-fp64 reference, stats_err, the largest value over STATS_CASES and both outputs.
STATS_GATE = 4 x E0 rounded up to one significant digit.  Measured: E0 = 4.05e-5 (the composed
rows of the series offset by 500 carry 1.6e-5; every other case stays under 2.3e-6), gate 2e-4;
the fused kernel's largest statistics error over the same cases is 1.6e-5.

Rows that (nearly) vanish analytically hold little but rounding noise, in the composed path
as in the kernel; a regression on them is 0 / 0 in the limit and is left out of the statistics
checks (``resolved``, a rule on the fp64 reference alone), for E0 and for the kernel alike."""

import functools

import numpy as np
import pytest
import torch

from gpu_helpers import gate, red_series
from oracle import modwt_spec as ms
from test_gpu_dwt_tsr import bank, ols64, stats_err, strided

pytestmark = pytest.mark.gpu
TOL = 1e-5          # the MODWT gate (tests/test_gpu_modwt_dwt.py)
E0 = 4.05e-5        # measured floor of the composed fp32 path, at (1333, db4, 6, offset 500), unrelated output
STATS_GATE = 2e-4   # 4 * E0 = 1.6e-4, rounded up to one significant digit

# (n, bank, J, batch, offset).  13: odd, the 15 lags wrap n more than once; 64: dilations = 0 mod
# n; 200: strided batch, dilations past n; sym10: 39-tap autocorrelation; offset 500: the shift by
# x[0]; 4096 / 16384: float4 path with 1 / 4 groups per thread; 4099: 16 samples per thread of
# the any-n path; 4100 / 8196: a pair's float4 path with 4 groups and more than 64 KiB of LDS;
# 16385: just above the limit of both kernels (the composed path)
CASES = [(8, "haar", 3, 1, 0), (13, "db4", 4, 1, 0), (64, "db4", 9, 1, 0), (200, "db4", 10, 3, 0),
         (1000, "sym10", 4, 1, 0), (1333, "db4", 6, 1, 500), (4096, "db4", 10, 2, 0),
         (16384, "db4", 10, 1, 0), (4099, "db4", 3, 1, 0), (4100, "db4", 5, 1, 0),
         (8196, "db4", 4, 1, 0), (16385, "db4", 3, 1, 0)]
STATS_CASES = [c for c in CASES if c[0] not in (4096, 16384)]  # long pairs: 4100, 8196, 16385 (cheaper references)
FLOORED = {(13, "db4", 4), (64, "db4", 9), (200, "db4", 10)}  # J > log2 n: rows that (nearly) vanish


def mra64(v, f, J):
    w = ms.modwt_direct(v.astype(np.float64), f["dec_lo"], f["dec_hi"], J)
    sm = ms.smooth_signal(w, f["dec_lo"], f["dec_hi"], J)
    return ms.modwtmra(w, f["dec_lo"], f["dec_hi"]), np.stack([sm[l]["signal"] for l in range(1, J + 1)])


@functools.lru_cache(maxsize=None)
def case(n, name, J, batch, offset):
    """Inputs x [batch, n] with their fp64 MRA rows and smooths."""
    rng = np.random.default_rng(n + J)
    x = np.stack([red_series(rng, n) + np.float32(offset) for _ in range(batch)])
    ref = [mra64(x[b], bank(name), J) for b in range(batch)]
    return x, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])


@functools.lru_cache(maxsize=None)
def pair_case(n, name, J, batch, offset):
    """The related and the unrelated outputs ([2, batch, n]) of case's inputs and their rows."""
    x = case(n, name, J, batch, offset)[0]
    rng = np.random.default_rng(3 * n + J)
    rel = np.stack([(0.8 * x[b] + 0.5 + 0.5 * red_series(rng, n)).astype(np.float32) for b in range(batch)])
    unrel = np.stack([red_series(np.random.default_rng(7 * n + b), n) for b in range(batch)])
    ys = np.stack([rel, unrel])
    return ys, np.stack([[mra64(y[b], bank(name), J)[0] for b in range(batch)] for y in ys])


def stats64(cx, cy, const):
    """[.., rows, 10]: ols64 per row pair, then the sizes stats_err wants in columns 8, 9."""
    st = np.array([[ols64(a, b, const) for a, b in zip(rx, ry)] for rx, ry in zip(cx, cy)])
    ymax, xmax = np.abs(cy).max(axis=-1), np.abs(cx).max(axis=-1)
    return np.concatenate([st, np.stack([ymax, ymax / xmax], -1)], -1)


def resolved(cx, cy):
    """Rows of a pair whose regression fp32 rows can carry: the centred row's rms is at least
    1e-3 of the largest centred sample of its series' rows.  The component gate allows a row an
    error of TOL x 0.1 max|ref| sqrt(n); below this size that is 1e-3 of the row itself or more,
    in the regressor, and its statistics are not comparable at a 1e-5-class gate (they are 0 / 0
    in the limit: the S_J of n = 2^J samples is the constant mean, and rows whose dilation is
    = 0 mod n vanish).  A function of the fp64 reference alone."""
    def ok(c):
        c = c - c.mean(axis=-1, keepdims=True)
        return np.linalg.norm(c, axis=-1) > 1e-3 * np.abs(c).max() * np.sqrt(c.shape[-1])
    return (ok(cx) & ok(cy)).all(axis=0)


def row_err(got, ref, floored):
    floor = 0.1 * np.abs(ref).max() * np.sqrt(ref.shape[-1]) if floored else 0.0
    return np.linalg.norm(got - ref, axis=-1) / (np.linalg.norm(ref, axis=-1) + floor)


@pytest.mark.parametrize("n,name,J,batch,offset", CASES)
def test_components_and_smooths_match_fp64_reference(n, name, J, batch, offset):
    from wtmi import ops
    x, cx, sx = case(n, name, J, batch, offset)
    f = bank(name)
    res = ops.modwt_mra(strided(x), f["dec_lo"], f["dec_hi"], J, want_smooths=True)
    assert res["components"].shape == (batch, 1, J + 1, n) and res["smooths"].shape == (batch, 1, J, n)
    assert res["stats"] is None
    fl = (n, name, J) in FLOORED
    gate("components", row_err(res["components"][:, 0].cpu().numpy().astype(np.float64), cx, fl), TOL)
    gate("smooths", row_err(res["smooths"][:, 0].cpu().numpy().astype(np.float64), sx, fl), TOL)


@pytest.mark.parametrize("n,name,J,batch,offset", [c for c in CASES if c[0] in (13, 200, 1000, 4096, 16384, 16385)])
def test_rows_from_coefficients(n, name, J, batch, offset):
    from wtmi import ops
    x, cx, _ = case(n, name, J, batch, offset)
    f = bank(name)
    xd = strided(x)
    got = ops.modwt_mra_rows(ops.modwt(xd, f["dec_lo"], f["dec_hi"], J), f["dec_lo"], f["dec_hi"])
    fl = (n, name, J) in FLOORED
    gate("rows vs reference", row_err(got.cpu().numpy().astype(np.float64), cx, fl), TOL)
    fused = ops.modwt_mra(xd, f["dec_lo"], f["dec_hi"], J)["components"][:, 0]
    gate("rows vs fused", row_err(got.cpu().numpy().astype(np.float64), fused.cpu().numpy().astype(np.float64), fl), 2e-5)


def test_rows_from_arbitrary_coefficients():
    from wtmi import ops
    n, J, f = 333, 5, bank("db4")
    w = np.random.default_rng(5).standard_normal((2, J + 1, n)).astype(np.float32)
    ref = np.stack([ms.modwtmra(wb.astype(np.float64), f["dec_lo"], f["dec_hi"]) for wb in w])
    got = ops.modwt_mra_rows(torch.tensor(w, device="cuda"), f["dec_lo"], f["dec_hi"])
    gate("rows of random w", row_err(got.cpu().numpy().astype(np.float64), ref, False), TOL)


@pytest.mark.parametrize("n,name,J,batch,offset,const",
                         [(*c, True) for c in STATS_CASES] + [(1333, "db4", 6, 1, 500, False)])
def test_pair_stats_match_fp64_reference(n, name, J, batch, offset, const):
    from wtmi import ops
    x, cx, _ = case(n, name, J, batch, offset)
    ys, cy = pair_case(n, name, J, batch, offset)
    f = bank(name)
    for o in range(2):
        res = ops.modwt_mra(strided(x), f["dec_lo"], f["dec_hi"], J, y=strided(ys[o]), add_constant=const)
        assert res["components"].shape == (batch, 2, J + 1, n) and res["stats"].shape == (batch, J + 1, 8)
        gate(f"pair components[{o}]", row_err(res["components"].cpu().numpy().astype(np.float64),
                                              np.stack([cx, cy[o]], axis=1), (n, name, J) in FLOORED), TOL)
        keep = resolved(cx, cy[o])
        got = res["stats"].cpu().numpy()
        gate(f"stats[{o}]", stats_err(got[:, keep], stats64(cx[:, keep], cy[o][:, keep], const)), STATS_GATE)
        only = ops.modwt_mra(strided(x), f["dec_lo"], f["dec_hi"], J, y=strided(ys[o]), add_constant=const,
                             want_components=False)
        assert only["components"] is None
        np.testing.assert_array_equal(only["stats"].cpu().numpy(), got)
        ols = ops.rows_ols(res["components"][:, 0].reshape(-1, n), res["components"][:, 1].reshape(-1, n),
                           const).cpu().numpy().reshape(batch, J + 1, 8)
        gate(f"fused vs rows_ols[{o}]", stats_err(got[:, keep], ols[:, keep]), STATS_GATE)


def test_zero_input_gives_nan_slope_and_mean_intercept():
    from wtmi import ops
    n, J, f = 200, 3, bank("db4")
    y = red_series(np.random.default_rng(1), n)
    s = ops.modwt_mra(torch.zeros(1, n, device="cuda"), f["dec_lo"], f["dec_hi"], J,
                      y=torch.tensor(y[None], device="cuda"))["stats"][0].cpu().numpy()
    assert np.isnan(s[:, [1, 2, 3]]).all()  # slope, bse_const, bse_slope
    np.testing.assert_allclose(s[:, 0], mra64(y, f, J)[0].mean(axis=1), rtol=0, atol=TOL * np.abs(y).max())


def test_src_layer_returns_the_same_numbers():
    from src import modwt
    n, name, J = 1333, "db4", 6
    x, cx, sx = case(n, name, J, 1, 500)
    ys, cy = pair_case(n, name, J, 1, 500)
    rows, smooths = modwt.mra(x[0], name, J, smooths=True)
    assert rows.dtype == np.float32 and rows.shape == (J + 1, n) and smooths.shape == (J, n)
    assert modwt.mra(x[0].astype(np.float64), name, J).dtype == np.float64
    gate("src rows", row_err(rows.astype(np.float64), cx[0], False), TOL)
    gate("src smooths", row_err(smooths.astype(np.float64), sx[0], False), TOL)
    w = modwt.modwt(x[0], name, J)
    f = bank(name)
    gate("src rows from w", row_err(modwt.modwtmra_batch(w, name).astype(np.float64),
                                    ms.modwtmra(w.astype(np.float64), f["dec_lo"], f["dec_hi"]), False), TOL)
    fit = modwt.time_scale_regression_series(x[0], ys[0, 0], J, name)
    assert fit.names == [f"D_{j}" for j in range(1, J + 1)] + [f"S_{J}"] and fit.nobs == n
    ref = stats64(cx, cy[0], True)[0]
    got = np.concatenate([fit.params, fit.bse, fit.rsquared[:, None], ref[:, 5:8]], axis=1)
    gate("src fit", stats_err(got, ref), STATS_GATE)
