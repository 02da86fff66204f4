"""ops.cwt_summary (wtmi_cwt_summary, K24) against plain fp64 numpy on the oracle's transform: the
global spectrum np.mean(|W|^2) over each scale's range, band power pw @ |W|^2 and band signal
rw @ Re W, W = oracle.pycwt_spec.cwt of the fp32 series widened to fp64.

Error measures: global power relative per (series, scale); band power rows normwise over t; band
signal rows normwise over t on the scale of the uncancelled sum || sum_j |rw[k, j]| |W_j| ||.  Every
gated denominator is asserted non-zero on the reference; a band holding no scale must be exactly 0.

Gates (DESIGN section 4's rule): E0 = the largest error over these cases of the same quantities
computed by fp64 numpy from the complex64 W of ops.cwt_morlet; gate = 4 E0 rounded up to one digit.
  global power  E0 1.62e-6  gate 7e-6  fused max 1.66e-6
  band power    E0 6.65e-7  gate 3e-6  fused max 6.67e-7
  band signal   E0 2.97e-7  gate 2e-6  fused max 2.79e-7
"""

import functools

import numpy as np
import pytest

from gpu_helpers import gate, red_series
from oracle import pycwt_spec as pc

pytestmark = pytest.mark.gpu

GATES = {"global_power": 7e-6, "band_power": 3e-6, "band_signal": 2e-6}
DT = 1.0
MOTHERS = {"morlet": lambda m: m.Morlet(6), "paul": lambda m: m.Paul(4), "dog": lambda m: m.DOG(2)}
# (n0, J (S = J + 1), batch, bands, t range, mother): see the issue's table of mechanisms
CASES = [
    (16, 4, 1, 1, None, "morlet"), (17, 6, 1, 2, None, "morlet"), (100, 20, 1, 2, "coi", "morlet"),
    (100, 20, 1, 1, None, "paul"), (100, 20, 1, 4, None, "dog"), (256, 12, 1, 0, None, "morlet"),
    (1333, 84, 1, 4, "empty", "morlet"), (1333, 84, 1, 2, "coi", "paul"), (1333, 84, 1, 1, None, "dog"),
    (1333, 129, 1, 2, None, "morlet"), (1333, 40, 3, 2, None, "morlet"), (4096, 8, 1, 4, None, "morlet"),
    (4097, 5, 1, 2, "coi", "morlet"), (16384, 3, 1, 2, None, "morlet"), (8, 2, 1, 1, None, "morlet"),
    (16385, 2, 1, 1, None, "morlet"), (16384, 69, 1, 2, None, "morlet"),
]


def summaries(W, lo, hi, pw, rw):
    """The three reductions of W [B, S, n0] in plain numpy (W complex128)."""
    P = np.abs(W) ** 2
    glob = np.array([[np.mean(P[b, j, lo[j]:hi[j]]) if hi[j] > lo[j] else np.nan for j in range(W.shape[1])]
                     for b in range(W.shape[0])])
    if pw is None:
        return glob, None, None, None
    return glob, pw @ P, rw @ W.real, np.abs(rw) @ np.abs(W)


@functools.lru_cache(maxsize=None)
def case(i):
    """Inputs and fp64 reference of CASES[i] (computed once, shared, never modified)."""
    from wtmi import transforms, wavelets
    n0, J, B, K, tr, mname = CASES[i]
    rng = np.random.default_rng(100 + i)
    x = np.stack([red_series(rng, n0) for _ in range(B)])
    aff = None
    if B > 1:  # the strided, standardised batch: (x - a0 - a1 t) * a2 rounded to fp32, as the kernel's load
        aff = np.stack([rng.uniform(-1, 1, B), rng.uniform(-1e-3, 1e-3, B), rng.uniform(0.5, 2, B)], axis=1)
    xs = x if aff is None else ((x.astype(np.float64) - aff[:, :1] - aff[:, 1:2] * np.arange(n0)) * aff[:, 2:]
                                ).astype(np.float32)
    dj = min(0.25, np.log2(max(2.0, n0 / 8)) / J)
    mo, wm = MOTHERS[mname](pc), MOTHERS[mname](wavelets)
    Ws = [pc.cwt(r.astype(np.float64), DT, dj, 2 * DT, J, mo) for r in xs]
    W, sj = np.stack([w[0] for w in Ws]), Ws[0][1]
    S, p = sj.size, wm.flambda() * sj
    bands = [(p[1], p[S // 2]), (p[S // 3], p[-1]), (4 * p[-1], 8 * p[-1]), (p[S // 2], p[S // 2])]
    bands = [(p[0], p[S // 2])] + bands[1:] if K >= 2 else bands  # K >= 2: two overlapping bands
    pw, rw = transforms.band_weights(sj, DT, dj, wm, bands[:K]) if K else (None, None)
    lo, hi = np.zeros(S, np.int32), np.full(S, n0, np.int32)
    if tr == "coi":
        lo, hi = transforms.coi_ranges(n0, DT, sj, wm)
    elif tr == "empty":
        lo[3] = hi[3] = 5
    ref = summaries(W, lo, hi, pw, rw)
    # denominators of the gated measures, checked before any device is used
    assert np.all(ref[0][~np.isnan(ref[0])] > 0)
    if K:
        live = pw.any(axis=1)
        assert live[:2].all() and (K < 4 or not live[2])
        assert np.all(np.linalg.norm(ref[1][:, live], axis=-1) > 0) and np.all(np.linalg.norm(ref[3][:, live], axis=-1) > 0)
    return dict(x=x, aff=aff, sj=sj, dj=dj, wm=wm, pw=pw, rw=rw, lo=lo, hi=hi, tr=tr, ref=ref)


def errors(got, c):
    """(global, band power, band signal) error arrays of got = (glob, bp, bs) against c's reference;
    asserts the NaN pattern and the exact zeros of empty bands."""
    glob, bp, bs, scale = c["ref"]
    out = {}
    if got[0] is not None:
        np.testing.assert_array_equal(np.isnan(got[0]), np.isnan(glob))
        ok = ~np.isnan(glob)
        out["global_power"] = np.abs(got[0][ok] - glob[ok]) / glob[ok]
    live = c["pw"].any(axis=1) if c["pw"] is not None else np.zeros(0, bool)
    for name, g, r, den in (("band_power", got[1], bp, bp), ("band_signal", got[2], bs, scale)):
        if g is None or r is None:
            continue
        assert not g[:, ~live].any(), f"{name}: a band without scales must be exactly 0"
        out[name] = (np.linalg.norm(g[:, live] - r[:, live], axis=-1) / np.linalg.norm(den[:, live], axis=-1)).ravel()
    return out


def run(c, **kw):
    """ops.cwt_summary on c's inputs (the batch as a strided view, ld = n0 + 5)."""
    import torch
    from wtmi import ops
    dev = torch.device("cuda", 0)
    B, n0 = c["x"].shape
    buf = torch.zeros((B, n0 + 5), dtype=torch.float32, device=dev)
    buf[:, :n0] = torch.as_tensor(c["x"], device=dev)
    kw.setdefault("power_weights", c["pw"])
    kw.setdefault("signal_weights", c["rw"])
    res = ops.cwt_summary(buf[:, :n0] if B > 1 else buf[0, :n0], c["sj"], DT, mother=c["wm"],
                          affine=None if c["aff"] is None else torch.as_tensor(c["aff"], device=dev),
                          t_range=None if c["tr"] is None else (c["lo"], c["hi"]), **kw)
    return tuple(None if res[k] is None else res[k].cpu().numpy().astype(np.float64)
                 for k in ("global_power", "band_power", "band_signal"))


@pytest.mark.parametrize("i", range(len(CASES)), ids=["-".join(map(str, c)) for c in CASES])
def test_cwt_summary_parity(i):
    c = case(i)
    for name, e in errors(run(c), c).items():
        gate(name, e, GATES[name])


@pytest.mark.parametrize("i", [2, 6, 12, 16])  # n0 = 100, 1333, 4097; 16384 with S > 64: split series
def test_signal_only_variant(i):
    c = case(i)
    got = run(c, power_weights=None, want_global=False)
    assert got[0] is None and got[1] is None
    gate("band_signal", errors(got, c)["band_signal"], GATES["band_signal"])
    full = run(c)[2]
    den = np.linalg.norm(c["ref"][3], axis=-1)
    live = den > 0
    gate("signal-only vs all outputs", (np.linalg.norm(got[2] - full, axis=-1)[live] / den[live]), GATES["band_signal"])


def test_repeat_launch_same_bits():
    c = case(6)  # 1 x 1333 x 85: several chunks, partial rows summed by the second kernel
    a, b = run(c), run(c)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_wrappers_return_the_op():
    from src import cwt as scwt
    from wtmi import ops, transforms
    import torch
    n0, dt, dj = 300, scwt.DT, scwt.DJ
    x = red_series(np.random.default_rng(7), n0)
    mother, dev = scwt.MOTHER, torch.device("cuda", 0)
    bands = [(0.5, 2.0), (1.0, 8.0)]

    def op(sj, dt_, dj_, **kw):
        pw, rw = transforms.band_weights(sj, dt_, dj_, mother, kw.pop("bands"))
        return ops.cwt_summary(torch.as_tensor(x, device=dev), sj, dt_, mother=mother, signal_weights=rw,
                               **({"power_weights": pw} if kw.pop("power", True) else {}), **kw)

    sj, _ = transforms.scales_for(n0, dt, dj, -1, -1, mother)
    ref = op(sj, dt, dj, bands=bands, t_range=transforms.coi_ranges(n0, dt, sj, mother))
    got = transforms.cwt_summary(x, dt, dj, wavelet=mother, bands=bands, coi=True)
    for k in ("global_power", "band_power", "band_signal"):
        np.testing.assert_array_equal(getattr(got, k), ref[k][0].cpu().numpy())
    bp = transforms.cwt_bandpass(x, dt, 1.0, 8.0, dj, wavelet=mother)
    np.testing.assert_array_equal(bp, op(sj, dt, dj, bands=bands[1:], power=False, want_global=False)
                                   ["band_signal"][0, 0].cpu().numpy())
    sj2, _ = transforms.scales_for(n0, scwt.DT, scwt.DJ, scwt.S0, scwt.J, mother)
    data = scwt.DataForCWT(np.datetime64("2000-01") + np.arange(n0), x.astype(np.float64), mother, scwt.DT,
                           scwt.DJ, scwt.S0, scwt.LEVELS)
    y = torch.as_tensor(x, device=dev).to(torch.float64).reshape(1, -1)
    for std, aff in ((False, None), (True, transforms.standardize_coefs(ops.series_moments(y)))):
        res = scwt.summarize_cwt_batch([data], bands, standardize=std)[0]
        ref2 = op(sj2, scwt.DT, scwt.DJ, bands=bands, affine=aff)
        for k in ("global_power", "band_power", "band_signal"):
            np.testing.assert_array_equal(getattr(res, k), ref2[k][0].cpu().numpy())
