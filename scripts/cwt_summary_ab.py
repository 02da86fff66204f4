"""A/B of the fused CWT summary launch (wtmi_cwt_summary) against what it replaces: ops.cwt_morlet
writing the [B, S, n0] power (and W where the band signal is asked for) followed by the torch
reductions.  HIP events around windows of back-to-back calls, both paths warmed, windows
alternating, one process.  Shapes: the app's 1 x 1333 x 85, C2's 1024 x 4096 x 128 with two bands
(all outputs and signal only), 256 x 8192 x 64.  Prints one JSON line per shape; with a path
argument the records are also written there (profiles/r12/cwt_summary_ab.json).

    python scripts/cwt_summary_ab.py [OUT.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "wavelet-transformer_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch

from gpu_helpers import red_batch
from wtmi import ops, transforms
from wtmi.wavelets import Morlet

DT = DJ = 1 / 12
M = Morlet(6)


def fused(x, sj, pw, rw, full):
    return ops.cwt_summary(x, sj, DT, power_weights=pw if full else None, signal_weights=rw, want_global=full)


def composed(x, sj, pw, rw, full):
    out = {}
    if full:
        P = ops.cwt_morlet(x, sj, DT, want_w=False, want_power=True)["power"]
        out["global_power"] = P.mean(dim=2)
        out["band_power"] = torch.einsum("kj,bjt->bkt", pw, P)
        del P
    W = ops.cwt_morlet(x, sj, DT)["w"]
    out["band_signal"] = torch.einsum("kj,bjt->bkt", rw, W.real)
    return out


def window(fn, args, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn(*args)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us per call


out = []
for B, n, S, full, calls, windows in ((1, 1333, 85, True, 20, 9), (1024, 4096, 128, True, 2, 7),
                                      (1024, 4096, 128, False, 2, 7), (256, 8192, 64, True, 2, 7)):
    x = torch.tensor(red_batch(1, B, n), device="cuda")
    sj = 2 * DT * 2 ** (np.arange(S) * DJ)
    per = M.flambda() * sj
    pw, rw = transforms.band_weights(sj, DT, DJ, M, [(per[S // 8], per[S // 2]), (per[S // 3], per[-2])])
    pwd, rwd = (torch.tensor(w, dtype=torch.float32, device="cuda") for w in (pw, rw))
    f, c = fused(x, sj, pw, rw, full), composed(x, sj, pwd, rwd, full)
    d = {"max_rel_diff_" + k: ((f[k] - c[k]).abs().max() / c[k].abs().max()).item() for k in c}
    del f, c
    pairs = (("fused", fused, (x, sj, pw, rw, full)), ("composed", composed, (x, sj, pwd, rwd, full)))
    for _, fn, args in pairs:
        window(fn, args, calls)  # warm-up of both paths at this shape
    t = {"fused": [], "composed": []}
    for _ in range(windows):
        for name, fn, args in pairs:
            t[name].append(window(fn, args, calls))
    rec = {"batch": B, "n": n, "scales": S, "outputs": "all" if full else "signal", "calls_per_window": calls,
           "windows": windows, **d}
    for k, v in t.items():
        rec[k + "_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    rec["speedup_median"] = rec["composed_us"]["median"] / rec["fused_us"]["median"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
