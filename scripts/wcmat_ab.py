"""A/B of the fused wavelet correlation matrix / multiple correlation launch (wtmi_modwt_wcmat)
against the two routes that existed before it: (a) composed -- ops.modwt rows of all series, fp64
torch Gram products and torch.linalg (ops._wcmat_composed) -- and (b) one wtmi_modwt_wcorr pair
launch for each of the M (M - 1) / 2 pairs, which yields cov and corr only.  HIP events around
windows of back-to-back calls, the three routes alternating in one process after a warm-up of all.
Shapes (db4): 1024 groups x 16 series x 2048 samples and 1024 x 4 x 8192, J = 8; the app's 1 x 7 x
1333, J = 6.  Prints one JSON line per shape; with a path argument the records are also written
there (profiles/r13/wcmat_ab.json).

    python scripts/wcmat_ab.py [OUT.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "wavelet-transformer_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch

from gpu_helpers import red_batch
from wtmi import ops
from wtmi.wavelets import Wavelet

w = Wavelet("db4")
LO, HI = ops._bank("wcmat_ab", dec_lo=w.dec_lo, dec_hi=w.dec_hi)
Z = 1.959963984540054


def fused(x, level):
    r = ops.modwt_wcmat(x, LO, HI, level)
    return r["cov"], r["corr"], r["r2"], r["stats"]


def composed(x, level):
    return ops._wcmat_composed(x, LO, HI, level, False, Z)


def pairs(x, level):
    M = x.shape[1]
    return [ops.modwt_wcorr(x[:, a], LO, HI, level, y=x[:, b])["stats"] for a in range(M) for b in range(a + 1, M)]


def window(fn, x, level, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn(x, level)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us per call


ROUTES = (("fused", fused), ("composed", composed), ("pairs", pairs))
out = []
for B, M, n, level, calls, windows in ((1, 7, 1333, 6, 20, 9), (1024, 16, 2048, 8, 2, 7), (1024, 4, 8192, 8, 2, 7)):
    x = torch.tensor(red_batch(1, B * M, n).reshape(B, M, n), device="cuda")
    f, c = fused(x, level), composed(x, level)
    d = [(a - b).abs().nan_to_num().max().item() for a, b in zip(f, c)]
    del f, c
    for _, fn in ROUTES:
        window(fn, x, level, 1)  # warm-up of every route at this shape
    t = {k: [] for k, _ in ROUTES}
    for _ in range(windows):
        for name, fn in ROUTES:
            t[name].append(window(fn, x, level, calls))
    rec = {"groups": B, "series": M, "n": n, "level": level, "calls_per_window": calls, "windows": windows,
           "max_abs_diff_cov_corr_r2_stats": d, "fused_bytes_read": 4 * M * n * B,
           "fused_bytes_written": 8 * level * (2 * M * M + M + 6) * B,
           "composed_coefficient_bytes_written_and_read": 2 * 4 * (level + 1) * M * n * B,
           "pair_launches": M * (M - 1) // 2, "pairs_bytes_read": 4 * n * B * M * (M - 1)}
    for k, v in t.items():
        rec[k + "_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    for k in ("composed", "pairs"):
        rec[k + "_over_fused"] = rec[k + "_us"]["median"] / rec["fused_us"]["median"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
