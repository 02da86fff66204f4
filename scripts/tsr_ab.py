"""A/B of the fused time-scale regression (wtmi_dwt_tsr) against the composition it replaces
(2 wavedec, 2 waverec with level + 1 masks, moments in torch): HIP events, the two paths
alternating in one process.  Prints one JSON line per shape; with a path argument the records
are also written there (profiles/r07/tsr_ab.json).

    python scripts/tsr_ab.py [OUT.json]"""
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


def composed(x, y, level):
    n = x.shape[1]
    masks = [1 << k for k in range(level + 1)]
    cx, cy = (ops.waverec(ops.wavedec(t, w.dec_lo, w.dec_hi, level)[0], n, w.rec_lo, w.rec_hi, level, masks).double()
              for t in (x, y))
    nobs = cx.shape[-1]
    mx, my = cx.mean(-1, keepdim=True), cy.mean(-1, keepdim=True)
    dx, dy = cx - mx, cy - my
    sxx, sxy, syy = (dx * dx).sum(-1), (dx * dy).sum(-1), (dy * dy).sum(-1)
    mx, my = mx[..., 0], my[..., 0]
    slope = sxy / sxx
    ssr = syy - slope * sxy
    s2 = ssr / (nobs - 2)
    return torch.stack([my - slope * mx, slope, torch.sqrt(s2 * (1 / nobs + mx * mx / sxx)), torch.sqrt(s2 / sxx),
                        1 - ssr / syy, ssr, torch.full_like(ssr, nobs), torch.full_like(ssr, nobs - 2)], dim=-1)


def fused(x, y, level):
    return ops.dwt_time_scale_regression(x, y, w.dec_lo, w.dec_hi, w.rec_lo, w.rec_hi, level)["stats"]


def window(fn, x, y, level, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn(x, y, level)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us per call


out = []
for B, n, level, calls in ((1, 1333, 6, 300), (4096, 1024, 6, 20)):
    x = torch.tensor(red_batch(1, B, n), device="cuda")
    y = torch.tensor(red_batch(2, B, n), device="cuda")
    d = (fused(x, y, level) - composed(x, y, level)).abs().max().item()
    for fn in (fused, composed):
        window(fn, x, y, level, calls)  # warm-up of both paths at this shape
    t = {"fused": [], "composed": []}
    for _ in range(15):
        for name, fn in (("fused", fused), ("composed", composed)):
            t[name].append(window(fn, x, y, level, calls))
    rec = {"batch": B, "n": n, "level": level, "calls_per_window": calls, "windows": 15,
           "max_abs_stats_diff": d}
    for k, v in t.items():
        rec[k + "_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    rec["speedup_median"] = rec["composed_us"]["median"] / rec["fused_us"]["median"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
