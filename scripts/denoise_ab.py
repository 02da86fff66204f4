"""A/B of the fused wavelet-shrinkage launch (wtmi_dwt_denoise) against the composition it replaces
(ops.wavedec, a torch sort for the two middle order statistics and ``where`` per level,
ops.waverec): HIP events, the two paths alternating in one process after a warm-up of both.
Shapes (db4, soft): the app's one series of 1333 samples, J = 7; 4096 series of 1024 samples, J = 6;
1024 series of 8192 samples, J = 10, with the universal and with the level-dependent rule.  Prints
one JSON line per shape; with a path argument the records are also written there
(profiles/r11/denoise_ab.json).

    python scripts/denoise_ab.py [OUT.json]"""
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
TAPS = [np.ascontiguousarray(np.asarray(t, dtype=np.float64)) for t in (w.dec_lo, w.dec_hi, w.rec_lo, w.rec_hi)]


def composed(x, level, rule):
    return ops._denoise_composed(x, TAPS, level, ops.DENOISE_RULES[rule], 0, 1.0, None)[:2]


def fused(x, level, rule):
    r = ops.dwt_denoise(x, *TAPS, level, rule=rule)
    return r["denoised"], r["info"]


def window(fn, x, level, rule, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn(x, level, rule)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us per call


out = []
for B, n, level, rule, calls, windows in ((1, 1333, 7, "universal", 20, 9), (4096, 1024, 6, "universal", 5, 9),
                                          (1024, 8192, 10, "universal", 3, 7), (1024, 8192, 10, "level", 3, 7)):
    x = torch.tensor(red_batch(1, B, n), device="cuda")
    f, c = fused(x, level, rule), composed(x, level, rule)
    # rows whose kept counts agree (a coefficient at its threshold may fall either way in fp32)
    same = (f[1][..., 2] == c[1][..., 2]).all(dim=1)
    d = {"rows_with_equal_kept": int(same.sum()),
         "max_abs_diff_denoised": (f[0][same] - c[0][same]).abs().max().item(),
         "max_rel_diff_lambda": ((f[1][..., 1] - c[1][..., 1]).abs() / c[1][..., 1]).max().item()}
    del f, c
    for fn in (fused, composed):
        window(fn, x, level, rule, calls)  # warm-up of both paths at this shape
    t = {"fused": [], "composed": []}
    for _ in range(windows):
        for name, fn in (("fused", fused), ("composed", composed)):
            t[name].append(window(fn, x, level, rule, calls))
    rec = {"batch": B, "n": n, "level": level, "rule": rule, "calls_per_window": calls, "windows": windows, **d}
    for k, v in t.items():
        rec[k + "_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    rec["speedup_median"] = rec["composed_us"]["median"] / rec["fused_us"]["median"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
