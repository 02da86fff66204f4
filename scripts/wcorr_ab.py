"""A/B of the fused wavelet variance / correlation / cross-correlation launch (wtmi_modwt_wcorr)
against the composition it replaces (two ops.modwt launches and fp64 torch reductions over their
rows, 2 max_lag + 1 more passes for the lags): HIP events, the two paths alternating in one
process after a warm-up of both.  Shapes: the app's one pair of 1333 samples, J = 6, 36 lags; 4096
pairs of 1024 samples, J = 6, without lags and with 36; 1024 pairs of 8192 samples, J = 10, 64
lags.  Prints one JSON line per shape; with a path argument the records are also written there
(profiles/r09/wcorr_ab.json).

    python scripts/wcorr_ab.py [OUT.json]"""
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
Z = 1.959963984540054


def composed(x, y, level, K):
    return ops._wcorr_composed(x, y, w.dec_lo, w.dec_hi, level, K, False, Z)


def fused(x, y, level, K):
    r = ops.modwt_wcorr(x, w.dec_lo, w.dec_hi, level, y=y, max_lag=K)
    return r["stats"], r["xcorr"]


def window(fn, x, y, level, K, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn(x, y, level, K)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us per call


out = []
for B, n, level, K, calls, windows in ((1, 1333, 6, 36, 20, 9), (4096, 1024, 6, 0, 5, 9), (4096, 1024, 6, 36, 2, 7),
                                       (1024, 8192, 10, 64, 1, 5)):
    x = torch.tensor(red_batch(1, B, n), device="cuda")
    y = torch.tensor(red_batch(2, B, n), device="cuda")
    f, c = fused(x, y, level, K), composed(x, y, level, K)
    d = [(a - b).abs().nan_to_num().max().item() for a, b in zip(f, c) if a is not None]
    del f, c
    for fn in (fused, composed):
        window(fn, x, y, level, K, calls)  # warm-up of both paths at this shape
    t = {"fused": [], "composed": []}
    for _ in range(windows):
        for name, fn in (("fused", fused), ("composed", composed)):
            t[name].append(window(fn, x, y, level, K, calls))
    rec = {"batch": B, "n": n, "level": level, "max_lag": K, "calls_per_window": calls, "windows": windows,
           "max_abs_diff_stats_xcorr": d}
    for k, v in t.items():
        rec[k + "_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    rec["speedup_median"] = rec["composed_us"]["median"] / rec["fused_us"]["median"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
