"""Fused DWT wavelet shrinkage (wtmi_dwt_denoise) against an all-fp64 reference written out here:
oracle.dwt_spec.wavedec of x widened to fp64, np.median of the detail magnitudes, the three
pywt.threshold formulas and the first n samples of oracle.dwt_spec.waverec.

Discontinuity condition: kept_j and the hard rule jump where |c| = lambda_j, so every case first
asserts, on the fp64 reference alone, that no detail coefficient lies within 1e-5 max(lambda_j,
max|cD_j|) of lambda_j (the elementwise DWT tolerance).  Nothing is masked or skipped.

sigma / lambda gate, by the rule of DESIGN.md section 4.  E0 is the fp32 floor: sigma and lambda
from fp64 np.median over the fp32 coefficients of the existing ops.wavedec, against the all-fp64
reference, the largest relative error over CASES x MODES.  Measured on an MI355X: E0 = 4.72e-7, at
(1000, db4, 5) x 3, rule "level", level 4.  SIGMA_GATE = 4 x E0 = 1.89e-6 rounded up to one
significant digit = 2e-6; the fused kernel's own maximum is 4.72e-7, at the same case
(profiles/r11/INDEX.md)."""

import functools
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_helpers import ROW_TOL, gate, red_series
from oracle import dwt_spec as ds

pytestmark = pytest.mark.gpu
SIGMA_GATE = 2e-6  # 4 * E0 = 1.89e-6, rounded up to one significant digit
MAD = 0.6744897501960817
# (n, bank, level, batch); 8193 takes the composed path beyond the kernel's limit
CASES = [(5, "db4", 2, 1), (14, "db4", 1, 1), (64, "haar", 5, 1), (129, "db4", 3, 1), (1333, "db4", 7, 1),
         (1000, "sym10", 4, 1), (4096, "db4", 9, 1), (8191, "db4", 9, 1), (8192, "db4", 10, 1),
         (8193, "db4", 6, 1), (1000, "db4", 5, 3)]
# (rule, shrink, mult); rule "fixed": thresholds mult * rms(cD_j) of the reference.  At mult = 1
# rule "level" zeroes every detail of these red-noise series, which would test nothing.  With
# 0.5 rms the closest coefficient of n = 8191 and 8192 clears the band below by 2 % and 10 %
# only (1.02e-5, 1.10e-5): their factors are the nearest that clear it well (7.8e-5, 1.2e-4).
FIXED = {8191: 0.52, 8192: 0.47}
MODES = [("universal", "soft", 1.0), ("universal", "hard", 1.0), ("universal", "garrote", 1.0),
         ("level", "soft", 0.3), ("fixed", "hard", 0.5)]


@functools.lru_cache(maxsize=None)
def bank(name):
    with open(GOLDEN + "/pywt_filters.json") as fh:
        return {k: np.asarray(v) for k, v in json.load(fh)["filters"][name].items()}


def shrink64(c, lam, shrink):
    if shrink == "hard":
        return np.where(np.abs(c) >= lam, c, 0.0)
    keep = np.abs(c) > lam
    safe = np.where(keep, c, 1.0)
    return np.where(keep, c - np.sign(c) * lam if shrink == "soft" else c * (1 - lam * lam / (safe * safe)), 0.0)


@functools.lru_cache(maxsize=None)
def series(n, name, level, batch):
    rng = np.random.default_rng(n + level)
    x = np.stack([red_series(rng, n) for _ in range(batch)])
    f = bank(name)
    return x, [ds.wavedec(xb, f["dec_lo"], f["dec_hi"], level) for xb in x.astype(np.float64)]


@functools.lru_cache(maxsize=None)
def case(n, name, level, batch, rule, shrink, mult):
    """x [batch, n] float32 and, in fp64: denoised [batch, n], info [batch, level, 4], the shrunk
    coefficient lists; the discontinuity condition is asserted here, before any device is used."""
    x, lists = series(n, name, level, batch)
    f = bank(name)
    mult = FIXED.get(n, mult) if rule == "fixed" else mult
    den, info, shrunk = [], np.zeros((batch, level, 4)), []
    for b, cs in enumerate(lists):
        out = [cs[0]]
        for j in range(level, 0, -1):
            d = cs[level + 1 - j]
            src = {"universal": cs[-1], "level": d}.get(rule)
            sigma = np.nan if src is None else np.median(np.abs(src)) / MAD
            lam = mult * np.sqrt(np.mean(d * d)) if src is None else mult * sigma * np.sqrt(2 * np.log(n))
            gap = np.abs(np.abs(d) - lam).min() / max(lam, np.abs(d).max())
            assert gap > 1e-5, ("a coefficient within the tolerance of its threshold", n, level, j, gap)
            out.append(shrink64(d, lam, shrink))
            info[b, j - 1] = sigma, lam, np.count_nonzero(out[-1]), d.size
        den.append(ds.waverec(out, f["rec_lo"], f["rec_hi"])[:n])
        shrunk.append(out)
    return x, np.array(den), info, shrunk, lists


def strided(a):  # [B, n] on the device, a view of a wider buffer (ld = n + 5) when B > 1
    t = torch.zeros((a.shape[0], a.shape[1] + 5), device="cuda")
    t[:, :a.shape[1]] = torch.tensor(a, device="cuda")
    return t[:, :a.shape[1]] if a.shape[0] > 1 else t[:, :a.shape[1]].contiguous()


def check(res, den, info, shrunk, lists):
    """The gates of every case: rows normwise, counts exact, sigma / lambda relative, and each shrunk
    array normwise on the scale of the array before shrinkage (a shrunk array may be all zero)."""
    got, gi = res["denoised"].cpu().numpy().astype(np.float64), res["info"].cpu().numpy()
    assert got.shape == den.shape and gi.shape == info.shape
    gate("denoised", np.linalg.norm(got - den, axis=-1) / np.linalg.norm(den, axis=-1), ROW_TOL)
    np.testing.assert_array_equal(gi[..., 2:], info[..., 2:])
    fin = np.isfinite(info[..., :2])
    assert np.array_equal(np.isfinite(gi[..., :2]), fin)
    gate("sigma_lambda", np.abs(gi[..., :2][fin] / info[..., :2][fin] - 1), SIGMA_GATE)
    gc = res["coeffs"].cpu().numpy().astype(np.float64)
    assert gc.shape == (len(shrunk), sum(a.size for a in shrunk[0]))
    for row, arrs, full in zip(gc, shrunk, lists):
        parts = np.split(row, np.cumsum([a.size for a in arrs])[:-1])
        gate("coeffs", [np.linalg.norm(p - a) / np.linalg.norm(c) for p, a, c in zip(parts, arrs, full)], ROW_TOL)


def run(x, name, level, **kw):
    from wtmi import ops
    f = bank(name)
    return ops.dwt_denoise(x, f["dec_lo"], f["dec_hi"], f["rec_lo"], f["rec_hi"], level, want_coeffs=True, **kw)


@pytest.mark.parametrize("rule,shrink,mult", MODES)
@pytest.mark.parametrize("n,name,level,batch", CASES)
def test_denoise_matches_fp64_reference(n, name, level, batch, rule, shrink, mult):
    x, den, info, shrunk, lists = case(n, name, level, batch, rule, shrink, mult)
    thr = info[:, :, 1] if rule == "fixed" else None
    check(run(strided(x), name, level, rule=rule, shrink=shrink, mult=mult, thresholds=thr),
          den, info, shrunk, lists)


@pytest.mark.parametrize("shrink", ["soft", "hard", "garrote"])
@pytest.mark.parametrize("n", [129, 1000])
def test_zero_thresholds_return_the_series(n, shrink):
    level = 3 if n == 129 else 4
    x, lists = series(n, "db4", level, 1)
    res = run(torch.tensor(x, device="cuda"), "db4", level, rule="fixed", shrink=shrink, thresholds=np.zeros(level))
    gate("identity", np.abs(res["denoised"].cpu().numpy() - x) / np.abs(x).max(), ROW_TOL)
    info, c = res["info"][0].cpu().numpy(), res["coeffs"][0].cpu().numpy()
    lens = [a.size for a in lists[0][:0:-1]]  # cD_1 .. cD_J
    np.testing.assert_array_equal(info[:, 3], lens)
    nz = [np.count_nonzero(p) for p in np.split(c, np.cumsum([a.size for a in lists[0]])[:-1])][:0:-1]
    np.testing.assert_array_equal(info[:, 2], lens if shrink == "hard" else nz)


@pytest.mark.parametrize("shrink", ["soft", "hard", "garrote"])
@pytest.mark.parametrize("n", [64, 256])  # cD_1 of 32 (ranked by one wave) and of 128 (radix select)
def test_ties_give_zero_sigma_and_no_nan(n, shrink):
    """A series constant on consecutive pairs: every haar cD_1 is 0.  The samples are signed powers
    of two, so that the fp32 tap products are exact and the zeros hold under fused multiply-add too."""
    rng = np.random.default_rng(3)
    x = np.repeat(np.ldexp(rng.choice([-1.0, 1.0], n // 2), rng.integers(-3, 4, n // 2)), 2).astype(np.float32)
    res = run(torch.tensor(x[None], device="cuda"), "haar", 5, rule="universal", shrink=shrink)
    info = res["info"][0].cpu().numpy()
    assert (info[:, :2] == 0.0).all() and not np.isnan(info).any()
    assert not torch.isnan(res["coeffs"]).any() and not torch.isnan(res["denoised"]).any()
    gate("ties", np.abs(res["denoised"][0].cpu().numpy() - x) / np.abs(x).max(), ROW_TOL)


def test_layers_agree_and_fallback_meets_the_same_gates():
    from src import dwt
    from wtmi import transforms
    for n, level in ((8192, 10), (8193, 6)):  # fused, and composed beyond the kernel's limit
        args = (n, "db4", level, 1, "universal", "soft", 1.0)
        check(run(torch.tensor(case(*args)[0], device="cuda"), "db4", level), *case(*args)[1:])
    a, b = case(129, "db4", 3, 1, "universal", "soft", 1.0), case(1333, "db4", 7, 1, "universal", "soft", 1.0)
    data = [dwt.DataForDWT(c[0][0], "db4", lv) for c, lv in ((a, 3), (b, 7))]
    for d, got in zip(data, dwt.denoise_signal_batch(data)):
        res = run(torch.tensor(d.y_values[None], device="cuda"), "db4", d.levels)
        info = res["info"][0].cpu().numpy()
        want = res["denoised"][0].cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(got["signal"], want)
        np.testing.assert_array_equal(transforms.dwt_denoise(d.y_values, "db4", d.levels), want)
        for k, col in (("sigma", 0), ("threshold", 1), ("kept", 2)):
            np.testing.assert_array_equal(got[k], info[:, col])
