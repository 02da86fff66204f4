"""A/B of the fused MODWT multiresolution analysis (wtmi_modwt_mra) against the composition it
replaces (ops.modwt, level + 1 one-bit-mask ops.imodwt, and for a pair ops.rows_ols): HIP events,
the two paths alternating in one process.  Shapes: the app's one pair of 1333 samples, J = 6,
statistics only; and a batch of 8192 series of 16384 samples, J = 10, components of single
series (bytes written against the HBM roofline are recorded for it).  Prints one JSON line per
shape; with a path argument the records are also written there (profiles/r07/mra_ab.json).

    python scripts/mra_ab.py [OUT.json]"""
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
HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak


def composed_rows(x, level):
    c = ops.modwt(x, w.dec_lo, w.dec_hi, level)
    return [ops.imodwt(c, w.dec_lo, w.dec_hi, 1 << j) for j in range(level + 1)]


def composed(x, y, level):
    if y is None:
        return composed_rows(x, level)
    n = x.shape[1]
    cx, cy = (torch.stack(composed_rows(t, level), 1).reshape(-1, n) for t in (x, y))
    return ops.rows_ols(cx, cy)


def fused(x, y, level):
    if y is None:
        return ops.modwt_mra(x, w.dec_lo, w.dec_hi, level)["components"]
    return ops.modwt_mra(x, w.dec_lo, w.dec_hi, level, y=y, want_components=False)["stats"]


def window(fn, x, y, level, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn(x, y, level)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us per call


out = []
for B, n, level, pair, calls, windows in ((1, 1333, 6, True, 300, 15), (8192, 16384, 10, False, 3, 9)):
    x = torch.tensor(red_batch(1, B, n), device="cuda")
    y = torch.tensor(red_batch(2, B, n), device="cuda") if pair else None
    if pair:
        d = (fused(x, y, level) - composed(x, y, level).reshape(B, level + 1, 8)).abs().max().item()
    else:
        f = fused(x, y, level)
        d = max((f[:, 0, j] - r).abs().max().item() for j, r in enumerate(composed(x, y, level)))
        del f
    for fn in (fused, composed):
        window(fn, x, y, level, calls)  # warm-up of both paths at this shape
    t = {"fused": [], "composed": []}
    for _ in range(windows):
        for name, fn in (("fused", fused), ("composed", composed)):
            t[name].append(window(fn, x, y, level, calls))
    rec = {"batch": B, "n": n, "level": level, "pair_stats_only": pair, "calls_per_window": calls,
           "windows": windows, "max_abs_diff": d}
    for k, v in t.items():
        rec[k + "_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    rec["speedup_median"] = rec["composed_us"]["median"] / rec["fused_us"]["median"]
    if not pair:  # the fused launch reads x once and writes level + 1 rows per series
        rec["fused_bytes"] = B * n * 4 * (level + 2)
        rec["fused_hbm_floor_us"] = rec["fused_bytes"] / HBM_BYTES_PER_S * 1e6
        rec["fused_share_of_hbm_peak"] = rec["fused_hbm_floor_us"] / rec["fused_us"]["median"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
