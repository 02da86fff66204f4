"""wtmi_cwt_summary without a GPU: the band weights and psi_0(0) against Torrence & Compo's formulas
and Table 2, the C ABI's argument errors (returned before any launch), the workspace size, and the
new kernels' registers from the built library (scripts/kernel_meta.py)."""

import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def test_band_weights_and_psi0():
    from wtmi import transforms
    from wtmi.wavelets import DOG, Morlet, Paul
    for w, v in ((Morlet(6), np.pi ** -0.25), (Paul(4), 1.079), (DOG(2), 0.867), (DOG(6), 0.884)):
        assert abs(w.psi0 - v) < 5e-4, (w, w.psi0)
    m, dt, dj = Morlet(6), 0.25, 0.5
    sj = np.array([1.0, 2.0, 4.0, 8.0])
    per = m.flambda() * sj
    pw, rw = transforms.band_weights(sj, dt, dj, m, [(per[1], per[2]), (100.0, 200.0)])  # ends included; empty
    np.testing.assert_allclose(pw, [[0, 0.5 * 0.25 / (0.776 * 2), 0.5 * 0.25 / (0.776 * 4), 0], [0] * 4], rtol=1e-15)
    np.testing.assert_allclose(rw[0, 1:3], 0.5 * 0.5 / (0.776 * np.pi ** -0.25 * np.sqrt([2.0, 4.0])), rtol=1e-15)
    assert not rw[1].any() and not rw[0, [0, 3]].any()
    with pytest.raises(ValueError, match="cdelta"):
        transforms.band_weights(sj, dt, dj, Morlet(8), [(1.0, 2.0)])


def test_coi_ranges_against_the_cone():
    from wtmi import transforms
    from wtmi.wavelets import Morlet
    m, n0, dt = Morlet(6), 11, 1.0
    sj = np.array([1.0, 2.0, 3.0, 50.0])
    lo, hi = transforms.coi_ranges(n0, dt, sj, m)
    coi = transforms.cone_of_influence(n0, dt, m)  # 0.730 * (0.5, 1.5, .., 5.5, .., 0.5)
    for j, s in enumerate(sj):
        inside = np.nonzero(m.flambda() * s <= coi)[0]
        assert (lo[j], hi[j]) == ((inside[0], inside[-1] + 1) if inside.size else (0, 0))
    assert (lo[0], hi[0]) == (1, 10) and (lo[1], hi[1]) == (3, 8) and (lo[3], hi[3]) == (0, 0)


def test_cwt_summary_return_codes_without_gpu():
    from wtmi import _lib
    lib = _lib.load()
    N, one = None, C.c_void_p(16)  # `one`: non-NULL, never dereferenced by a rejected call

    def f(ld=64, batch=1, n0=64, S=8, nb=1, pw=one, rw=one, g=one, bp=one, bs=one, ws=one, x=one):
        return lib.wtmi_cwt_summary(x, ld, batch, n0, N, one, S, 1.0, 0, 6.0, N, N, nb, pw, rw, g, bp, bs, ws, N)

    assert f(batch=0, x=N, g=N, bp=N, bs=N) == 0  # empty batch
    for bad in (dict(g=N, bp=N, bs=N), dict(nb=5), dict(nb=-1), dict(pw=N), dict(rw=N), dict(ld=63),
                dict(nb=0), dict(S=85, n0=1333, ld=1333, ws=N)):  # the last: split series, no workspace
        assert f(**bad) == -1, bad
    for big in (dict(n0=8, ld=8), dict(n0=16385, ld=16385), dict(n0=16384, ld=16384)):  # band power: N <= 8192
        assert f(**big) == -2, big
    wsb = lib.wtmi_cwt_summary_workspace_bytes
    sizes = [[wsb(b, 1333, 85, k) for b in (1, 2, 47, 64, 300)] for k in (1, 2, 4)]
    assert all(r == sorted(r) and r[0] > 0 for r in sizes) and all(a <= b for a, b in zip(sizes[0], sizes[2]))
    assert wsb(1024, 4096, 128, 2) == 0 and wsb(1, 1333, 85, 0) == 0  # one chunk per series; no bands


def test_cwt_summary_op_registered_and_checked():
    import torch
    from wtmi import ops
    assert hasattr(torch.ops.wtmi, "cwt_summary")
    x, sj = torch.zeros(2, 64), np.arange(1.0, 9.0)
    for match, kw in (("no output", dict(want_global=False)), ("power_weights", dict(power_weights=np.ones((5, 8)))),
                      ("signal_weights", dict(signal_weights=np.ones((1, 7)))),
                      ("signal_weights", dict(power_weights=np.ones((1, 8)), signal_weights=np.ones((2, 8)))),
                      ("t_range", dict(t_range=(np.zeros(8),)))):
        with pytest.raises(ValueError, match=match):
            ops.cwt_summary(x, sj, 1.0, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.cwt_summary(x, sj, 1.0)


def test_summary_kernel_registers():
    """No spills, no scratch; VGPRs within the occupancy the launch geometry counts on: 4 waves per
    SIMD (128) for the 1024-thread N = 16384 block and the bandless N = 8192 kernel (two workgroups
    per CU), 3 (168) for the other bandless kernels, 2 (256) once bands are accumulated."""
    from kernel_meta import LIB, LLVM, kernel_table
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")) or not shutil.which("c++filt"):
        pytest.skip("llvm-readelf / c++filt not available")
    if not os.path.exists(LIB):
        pytest.skip("libwtmi.so not built")
    tab = {k: r for k, r in kernel_table(LIB).items() if "cwt_summary_kernel" in k or "sum_chunks_kernel" in k}
    assert len(tab) == 1 + 10 * 14 + 4, sorted(tab)  # chunk sum; N <= 8192: 7 x 2 mothers; N = 16384: 2 x 2
    for name, r in tab.items():
        assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (name, r)
        if "sum_chunks" in name:
            continue
        logn, kb = (int(v) for v in name.split("<")[1].split(",")[:2])
        budget = 128 if logn == 14 or (logn == 13 and kb == 0) else (168 if kb == 0 else 256)
        assert r["vgpr"] <= budget, (name, r)
