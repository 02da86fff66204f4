"""A/B of the fused MODWT shrinkage launch (wtmi_modwt_denoise) against the composition it replaces
(ops.modwt, a torch sort for the two middle order statistics and ``where`` per level, ops.imodwt):
HIP events, the routes alternating window by window in one process after a warm-up of all.  Shapes
(db4, soft, universal): the app's one series of 1333 samples, J = 7; 1024 series of 2048 samples,
J = 8; 1024 series of 8192 samples, J = 10 (seven rows spilled), the last also with the synthesis
gathering its spilled rows from memory (option modwt_den_stage = 0) and with the level-dependent
rule.  Prints one JSON line per shape with the bytes per call of both routes; with a path argument
the records are also written there (profiles/r14/modwt_denoise_ab.json).

    python scripts/modwt_denoise_ab.py [OUT.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "wavelet-transformer_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch

from gpu_helpers import red_batch
from wtmi import _lib, ops
from wtmi.wavelets import Wavelet

w = Wavelet("db4")
LO, HI = ops._bank("modwt_denoise_ab", dec_lo=w.dec_lo, dec_hi=w.dec_hi)


def composed(x, level, rule):
    return ops._modwt_denoise_composed(x, LO, HI, level, ops.DENOISE_RULES[rule], 0, 1.0, None)[:2]


def fused(x, level, rule):
    r = ops.modwt_denoise(x, LO, HI, level, rule=rule)
    return r["denoised"], r["info"]


def fused_gather(x, level, rule):
    with _lib.option("modwt_den_stage", 0):
        return fused(x, level, rule)


def window(fn, x, level, rule, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn(x, level, rule)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us per call


def traffic(B, n, level, rule):
    """Bytes per call.  fused: x in, denoised and info out, and per spilled row one write and one
    read (two reads where a median is taken from it).  composed: modwt writes level + 1 rows; per
    level the magnitudes, the sort (keys in and out, at least), the comparison, the shrunk values
    and the copy back each pass over a row; imodwt reads level + 1 rows and writes the series."""
    S = _lib.call("wtmi_modwt_denoise_workspace_bytes", B, n, level) // (4 * B * n)
    raw = S if rule == "level" else min(S, 1)
    sorts = level if rule == "level" else 1
    row = 4 * B * n
    return {"fused": row * (2 + 2 * S + raw) + 32 * B * level,
            "composed": row * (1 + (level + 1) + 8 * level + 2 * sorts + (level + 1) + 1) + 32 * B * level,
            "spilled_rows": int(S)}


out = []
for B, n, level, rule, calls, windows in ((1, 1333, 7, "universal", 20, 9), (1024, 2048, 8, "universal", 3, 7),
                                          (1024, 8192, 10, "universal", 2, 7), (1024, 8192, 10, "level", 2, 7)):
    x = torch.tensor(red_batch(1, B, n), device="cuda")
    f, c = fused(x, level, rule), composed(x, level, rule)
    # rows whose kept counts agree (a coefficient at its threshold may fall either way in fp32)
    same = (f[1][..., 2] == c[1][..., 2]).all(dim=1)
    d = {"rows_with_equal_kept": int(same.sum()),
         "max_abs_diff_denoised": (f[0][same] - c[0][same]).abs().max().item(),
         "max_rel_diff_lambda": ((f[1][..., 1] - c[1][..., 1]).abs() / c[1][..., 1]).max().item()}
    del f, c
    routes = [("fused", fused), ("composed", composed)] + ([("fused_gather", fused_gather)] if n == 8192 else [])
    for _, fn in routes:
        window(fn, x, level, rule, calls)  # warm-up of every route at this shape
    t = {name: [] for name, _ in routes}
    for _ in range(windows):
        for name, fn in routes:
            t[name].append(window(fn, x, level, rule, calls))
    rec = {"batch": B, "n": n, "level": level, "rule": rule, "calls_per_window": calls, "windows": windows, **d,
           "bytes_per_call": traffic(B, n, level, rule)}
    for k, v in t.items():
        rec[k + "_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    rec["speedup_median"] = rec["composed_us"]["median"] / rec["fused_us"]["median"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
