"""A/B of the fused DWT smoothing ladder (wtmi_dwt_smooth) against the composition it replaces
(ops.wavedec, ops.waverec with the level keep-masks, the trim, ops.rows_ols against y repeated
per row): HIP events, the two paths alternating in one process.  Prints one JSON line per shape;
with a path argument the records are also written there (profiles/r08/smooth_ab.json).

    python scripts/smooth_ab.py [OUT.json]"""
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


def composed(x, y, level, want_smooth):
    B, n = x.shape
    masks = [(1 << (level + 1 - l)) - 1 for l in range(1, level + 1)]
    rec = ops.waverec(ops.wavedec(x, w.dec_lo, w.dec_hi, level)[0], n, w.rec_lo, w.rec_hi, level, masks)
    smooth = rec[:, :, rec.shape[-1] - n:].contiguous()
    stats = ops.rows_ols(smooth.reshape(-1, n), y[:, None, :].expand(B, level, n).reshape(-1, n))
    return smooth, stats.reshape(B, level, 8)


def fused(x, y, level, want_smooth):
    r = ops.dwt_smooth(x, w.dec_lo, w.rec_lo, level, y=y, want_smooth=want_smooth)
    return r["smooth"], r["stats"]


def window(fn, args, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn(*args)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us per call


out = []
for B, n, level, want_smooth, calls in ((1, 1333, 7, True, 300), (4096, 1024, 6, False, 20),
                                        (4096, 1024, 6, True, 20)):
    x = torch.tensor(red_batch(1, B, n), device="cuda")
    y = torch.tensor(red_batch(2, B, n), device="cuda")
    args = (x, y, level, want_smooth)
    (fs, ft), (cs, ct) = fused(*args), composed(*args)
    rec = {"batch": B, "n": n, "level": level, "smooths": want_smooth, "calls_per_window": calls,
           "windows": 15, "max_abs_stats_diff": (ft - ct).abs().max().item(),
           "max_abs_smooth_diff": (fs - cs).abs().max().item() if want_smooth else None}
    for fn in (fused, composed):
        window(fn, args, calls)  # warm-up of both paths at this shape
    t = {"fused": [], "composed": []}
    for _ in range(15):
        for name, fn in (("fused", fused), ("composed", composed)):
            t[name].append(window(fn, args, calls))
    for k, v in t.items():
        rec[k + "_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    rec["speedup_median"] = rec["composed_us"]["median"] / rec["fused_us"]["median"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
