"""Fused MODWT wavelet correlation matrix / wavelet multiple correlation (wtmi_modwt_wcmat,
ops.modwt_wcmat) against a plain fp64 numpy statement of the estimators over
oracle.modwt_spec.modwt_direct rows of the fp32 inputs widened to fp64.

Error metric (``wcmat_err``): variances (cov diagonal) relative, covariances |d| / sqrt(var_a
var_b), corr, r2, wmc and its interval absolute; nobs, n_eff and the NaN positions exact; corr
symmetric bit for bit with a unit diagonal; target by r2[target] == max(r2) on the kernel's own
row (for M = 2 the two R^2 tie in exact arithmetic).

Gate, by the rule of test_gpu_modwt_wcorr.  E0 is the fp32 floor: the same
metric for the composed route -- fp64 torch Gram products and torch.linalg over the fp32 rows of
ops.modwt -- the largest value over the fused-size CASES and both boundary modes.  GATE = 4 x E0
rounded up to one significant digit.  Measured: E0 = 6.71e-7 ((16384, db4, 10) x 2 series, brick
wall), gate 3e-6; the fused kernel's largest error over the same cases is 6.71e-7 (the same case:
the two routes differ by less than 1e-14 there).  With this generator the fp64 reference has
cond(P_j) <= 1e2 at every computed level of the fused-size cases (R^2 amplifies the coefficient
error by the conditioning)."""

import functools
import math
from statistics import NormalDist

import numpy as np
import pytest
import torch

from gpu_helpers import gate, red_series
from oracle import modwt_spec as ms
from test_gpu_dwt_tsr import bank

pytestmark = pytest.mark.gpu
E0 = 6.71e-7  # measured floor of the composed fp32 path, at (16384, db4, 10, M = 2), brick wall
GATE = 3e-6   # 4 * E0 = 2.68e-6, rounded up to one significant digit
Z = NormalDist().inv_cdf(0.975)

# (n, bank, J, M, batch, offset).  8: R = 8 replicas, n below one matrix step's 32 samples, brick
# wall level 3 has nobs 1 < M (r2 / wmc NaN, cov / corr finite); 13: odd n, R = 5 with an idle row,
# level 2 has nobs 0; 200: strided batch; 1333 / offset 500: the app's length, the shift by x[0],
# R = 2; sym10: R = 1 with idle rows, 20 taps; 2048 x 16, 8192 x 4, 16384 x 2: M n at its limit;
# 2049 x 16 and M = 17: the composed route
CASES = [(8, "haar", 3, 2, 1, 0), (13, "db4", 2, 3, 1, 0), (200, "db4", 4, 5, 3, 0),
         (1333, "db4", 6, 7, 1, 500), (1000, "sym10", 4, 9, 1, 0), (2048, "db4", 6, 16, 2, 0),
         (8192, "db4", 8, 4, 1, 0), (16384, "db4", 10, 2, 1, 0), (2049, "db4", 3, 16, 1, 0),
         (64, "db4", 3, 17, 1, 0)]


def wcmat64(w, L, periodic):
    """cov, corr [J, M, M], r2 [J, M] and stats [J, 6] of detail rows w [M, J, n] (include/wtmi.h)."""
    M, J, n = w.shape
    cov, r2, stats = np.full((J, M, M), np.nan), np.full((J, M), np.nan), np.full((J, 6), np.nan)
    corr = cov.copy()
    for j in range(1, J + 1):
        t0 = 0 if periodic else min(n, (2 ** j - 1) * (L - 1))
        Mj = n - t0
        stats[j - 1, 4] = max(Mj, 0)
        if Mj <= 0:
            continue
        a = w[:, j - 1, t0:]
        c = a @ a.T / Mj
        var = np.diag(c)
        with np.errstate(all="ignore"):
            p = c / np.sqrt(np.outer(var, var))
        p[np.diag_indices(M)] = np.where(var > 0, 1.0, np.nan)
        cov[j - 1], corr[j - 1] = c, p
        neff = n // 2 ** j - (0 if periodic else math.ceil((L - 2) * (1 - 2.0 ** -j)))
        stats[j - 1, 5] = neff
        if Mj < M or not (var > 0).all():
            continue
        r = 1 - 1 / np.diag(np.linalg.inv(p))
        wmc, hw = np.sqrt(r.max()), Z / np.sqrt(neff - 3) if neff > 3 else np.nan
        r2[j - 1] = r
        with np.errstate(all="ignore"):
            stats[j - 1, :4] = [wmc, np.argmax(r), np.tanh(np.arctanh(wmc) - hw), np.tanh(np.arctanh(wmc) + hw)]
    return cov, corr, r2, stats


def group(rng, n, M, offset):
    c = red_series(rng, n)
    return np.stack([(0.8 * np.roll(c, a) + red_series(rng, n) + offset).astype(np.float32) for a in range(M)])


@functools.lru_cache(maxsize=None)
def case(n, name, J, M, batch, offset):
    """Groups x [batch, M, n] and, per boundary mode, their fp64 tables."""
    rng = np.random.default_rng(n + J + M)
    x = np.stack([group(rng, n, M, offset) for _ in range(batch)])
    f = bank(name)
    w = [np.stack([ms.modwt_direct(v, f["dec_lo"], f["dec_hi"], J)[:J] for v in g]) for g in x]
    return x, {p: [wcmat64(wg, len(f["dec_lo"]), p) for wg in w] for p in (False, True)}


def strided(a):
    """[B, M, n] on the device as a view of a wider buffer (ld = n + 5) when B > 1."""
    t = torch.zeros(a.shape[:2] + (a.shape[2] + 5,), device="cuda")
    t[..., :a.shape[2]] = torch.tensor(a, device="cuda")
    return t[..., :a.shape[2]] if a.shape[0] > 1 else t[..., :a.shape[2]].contiguous()


def wcmat_err(got, ref):
    """The largest error of one group's tables (cov, corr, r2, stats) against ``ref``."""
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r))
    (cov, corr, r2, st), (rc, rp, rr, rs) = got, ref
    np.testing.assert_array_equal(st[:, 4:], rs[:, 4:])
    np.testing.assert_array_equal(corr, corr.transpose(0, 2, 1))
    d = np.einsum("jaa->ja", corr)
    assert (d[~np.isnan(d)] == 1).all()
    for j in np.flatnonzero(~np.isnan(st[:, 1])):
        assert r2[j, int(st[j, 1])] == r2[j].max()
    var = np.einsum("jaa->ja", rc)
    with np.errstate(all="ignore"):
        e_cov = np.abs(cov - rc) / np.sqrt(var[:, :, None] * var[:, None, :])  # the diagonal: relative
    return max(np.nanmax(e, initial=0.0) for e in (e_cov, np.abs(corr - rp), np.abs(r2 - rr),
                                                   np.abs(st[:, [0, 2, 3]] - rs[:, [0, 2, 3]])))


def tables(res):
    return [res[k].cpu().numpy() for k in ("cov", "corr", "r2", "stats")]


@pytest.mark.parametrize("boundary", ["brickwall", "periodic"])
@pytest.mark.parametrize("n,name,J,M,batch,offset", CASES)
def test_matrices_and_multiple_correlation_match_fp64_reference(n, name, J, M, batch, offset, boundary):
    from wtmi import ops
    x, ref = case(n, name, J, M, batch, offset)
    f = bank(name)
    got = tables(ops.modwt_wcmat(strided(x), f["dec_lo"], f["dec_hi"], J, boundary=boundary))
    assert [g.shape for g in got] == [(batch, J, M, M), (batch, J, M, M), (batch, J, M), (batch, J, 6)]
    err = [wcmat_err([g[b] for g in got], ref[boundary == "periodic"][b]) for b in range(batch)]
    gate(f"wcmat[{boundary}]", err, GATE)


def test_two_series_reproduce_the_pair_kernel():
    from wtmi import ops
    x, _ = case(1333, "db4", 6, 7, 1, 500)
    f = bank("db4")
    xd = torch.tensor(x[:, :2], device="cuda")
    cov, corr, r2, st = tables(ops.modwt_wcmat(xd, f["dec_lo"], f["dec_hi"], 6))
    pair = ops.modwt_wcorr(xd[:, 0], f["dec_lo"], f["dec_hi"], 6, y=xd[:, 1])["stats"][0].cpu().numpy()
    den = np.sqrt(pair[:, 0] * pair[:, 1])
    gate("variances", np.abs(np.stack([cov[0, :, 0, 0] / pair[:, 0], cov[0, :, 1, 1] / pair[:, 1]]) - 1), GATE)
    gate("covariance", np.abs(cov[0, :, 0, 1] - pair[:, 2]) / den, GATE)
    gate("wmc = |corr|", np.abs(st[0, :, 0] - np.abs(pair[:, 3])), GATE)


def test_constant_series_has_zero_covariance_and_no_multiple_correlation():
    from wtmi import ops
    x, _ = case(200, "db4", 4, 5, 3, 0)
    f = bank("db4")
    g = x[0, :3].copy()
    g[1] = 500.25
    cov, corr, r2, st = tables(ops.modwt_wcmat(torch.tensor(g, device="cuda"), f["dec_lo"], f["dec_hi"], 4))
    assert (cov[0, :, 1] == 0).all() and (cov[0, :, :, 1] == 0).all()
    assert np.isnan(corr[0, :, 1]).all() and np.isnan(corr[0, :, :, 1]).all()
    assert np.isnan(r2).all() and np.isnan(st[0, :, :4]).all() and (st[0, :, 4:] > 0).all()
    assert np.isfinite(cov[0][:, [0, 2]][:, :, [0, 2]]).all() and np.isfinite(corr[0][:, [0, 2]][:, :, [0, 2]]).all()


def test_equal_inputs_give_equal_bits():
    from wtmi import ops
    x, _ = case(2048, "db4", 6, 16, 2, 0)
    f = bank("db4")
    xd = torch.tensor(x, device="cuda")
    a, b = (tables(ops.modwt_wcmat(xd, f["dec_lo"], f["dec_hi"], 6)) for _ in range(2))
    for p, q in zip(a, b):
        np.testing.assert_array_equal(p, q)


def test_transform_and_src_layers_return_the_same_numbers():
    from src import modwt
    from wtmi import ops, transforms
    x, _ = case(1333, "db4", 6, 7, 1, 500)
    f = bank("db4")
    cov, corr, r2, st = (t[0] for t in tables(ops.modwt_wcmat(torch.tensor(x, device="cuda"), f["dec_lo"], f["dec_hi"], 6)))
    for r in (transforms.wavelet_correlation_matrix(x[0], 6, "db4"), modwt.wavelet_correlation_matrix_series(list(x[0]), 6)):
        assert r.names == [f"D_{j}" for j in range(1, 7)]
        for got, want in ((r.covariance, cov), (r.correlation, corr), (r.r_squared, r2), (r.multiple_correlation, st[:, 0]),
                          (r.target, st[:, 1]), (r.ci, st[:, 2:4]), (r.nobs, st[:, 4])):
            np.testing.assert_array_equal(got, want)
