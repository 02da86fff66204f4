"""A/B of the fused time-localized wavelet correlation launch (wtmi_modwt_lwcorr) against the
composition it replaces (two ops.modwt launches and fp64 torch windowed sums over their rows:
products of the padded rows with a banded Toeplitz block of the weights, ops._lwcorr_composed): HIP
events, the two paths alternating in one process after a warm-up of both.  Shapes: the app's one
pair of 1333 samples, J = 6, H = 64; 1024 pairs of 8192 samples, J = 10, uniform H = 64 and
gaussian H = 1024.  Prints one JSON line per shape; with a path argument the records are also
written there (profiles/r15/lwcorr_ab.json).

    python scripts/lwcorr_ab.py [OUT.json]"""
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
from wtmi.transforms import local_window
from wtmi.wavelets import Wavelet

w = Wavelet("db4")


def composed(x, y, level, th):
    return ops._lwcorr_composed(x, y, np.asarray(w.dec_lo, float), np.asarray(w.dec_hi, float), level, th, False)


def fused(x, y, level, th):
    r = ops.modwt_lwcorr(x, w.dec_lo, w.dec_hi, level, y=y, window=th, moments=True)
    return r["corr"], r["moments"]


def window(fn, x, y, level, th, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn(x, y, level, th)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us per call


out = []
for B, n, level, H, name, calls, windows in ((1, 1333, 6, 64, "uniform", 10, 7), (1024, 8192, 10, 64, "uniform", 1, 5),
                                             (1024, 8192, 10, 1024, "gaussian", 1, 3)):
    x = torch.tensor(red_batch(1, B, n), device="cuda")
    y = torch.tensor(red_batch(2, B, n), device="cuda")
    th = local_window(name, H)
    f, c = fused(x, y, level, th), composed(x, y, level, th)
    d = [(a - b).abs().nan_to_num().max().item() for a, b in zip(f, c)]
    del f, c
    for fn in (fused, composed):
        window(fn, x, y, level, th, calls)  # warm-up of both paths at this shape
    t = {"fused": [], "composed": []}
    for _ in range(windows):
        for key, fn in (("fused", fused), ("composed", composed)):
            t[key].append(window(fn, x, y, level, th, calls))
    rec = {"batch": B, "n": n, "level": level, "half_width": H, "window": name, "calls_per_window": calls,
           "windows": windows, "max_abs_diff_corr_moments": d}
    for k, v in t.items():
        rec[k + "_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    rec["speedup_median"] = rec["composed_us"]["median"] / rec["fused_us"]["median"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
