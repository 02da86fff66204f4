"""Batched device-tensor API over libwtmi.so.

Every function takes/returns torch tensors resident on an MI355X (``cuda`` device
under ROCm), enqueues the HIP kernels on the current stream of that device and
returns without synchronising.  There is no CPU implementation: a CPU tensor or a
missing library raises.  The same functions are registered as torch custom ops
(``torch.ops.wtmi.*``, see ``_register``) so they compose with torch code.
"""

from __future__ import annotations

import ctypes as C
import threading
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

VP = C.c_void_p


def _ptr(t: Optional[torch.Tensor]):
    return VP(t.data_ptr()) if t is not None else VP(None)


def _stream(dev: torch.device):
    return VP(torch.cuda.current_stream(dev).cuda_stream)


def _check_dev(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                f"wtmi kernels run on the GPU only; got a tensor on {t.device} "
                "(no CPU fallback exists)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("all wtmi operands must be on the same device")
    return dev


def _rows(x: torch.Tensor, dtype=None) -> torch.Tensor:
    """[n] or [B, n] -> [B, n] with unit stride along time and a row stride >= n (the C ABI's
    ld).  A size-1 batch dimension may carry any stride in torch (NumPy's x[None, :] arrives
    with stride 0), so a one-row view is re-strided to ld = n; an expanded batch is copied."""
    if dtype is not None:
        x = x.to(dtype)
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2:
        raise ValueError("expected a [batch, n] tensor")
    B, n = x.shape
    if x.stride(1) != 1 or (B > 1 and x.stride(0) < n):
        x = x.contiguous()
    if B == 1 and x.stride(0) != n:
        x = x.as_strided((1, n), (n, 1), x.storage_offset())
    return x


_F64_CACHE: "dict[tuple, torch.Tensor]" = {}
_F64_CACHE_MAX = 256
_F64_LOCK = threading.Lock()


def _f64_dev(a, dev) -> Optional[torch.Tensor]:
    """Host arrays (scale vectors, significance multipliers) as device float64 tensors.
    A pageable host-to-device copy blocks the host until the stream drains, which
    serialises back-to-back transforms; the copies are therefore content-addressed and
    cached per device (the key is the array's bytes, so a changed array is a new entry)."""
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.float64).contiguous()
    h = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    key = (str(dev), h.shape, h.tobytes())
    with _F64_LOCK:
        t = _F64_CACHE.get(key)
    if t is None:
        t = torch.as_tensor(h, device=dev)
        with _F64_LOCK:
            if len(_F64_CACHE) >= _F64_CACHE_MAX:
                _F64_CACHE.pop(next(iter(_F64_CACHE)))
            _F64_CACHE[key] = t
    # the cached block may be read by kernels on several streams: tell the caching
    # allocator about this one, so an eviction cannot recycle it under a running kernel
    t.record_stream(torch.cuda.current_stream(dev))
    return t


# ------------------------------------------------------------------------ moments
def series_moments(x: torch.Tensor) -> torch.Tensor:
    """[B, 8] float64: mean, std(ddof 0), slope, intercept, c0, c1, n, 0."""
    x = _rows(x)
    dev = _check_dev(x)
    if x.dtype not in (torch.float32, torch.float64):
        x = _rows(x, torch.float64)
    out = torch.empty((x.shape[0], 8), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_series_moments", _ptr(x), int(x.dtype == torch.float64), x.stride(0),
                  x.shape[0], x.shape[1], _ptr(out), _stream(dev))
    return out


AFF_DETREND, AFF_REMOVE_MEAN, AFF_STANDARDIZE = 1, 2, 4
AFF_NORMALIZE = AFF_REMOVE_MEAN | AFF_STANDARDIZE  # pycwt xwt / wct: (y - mean) / std


def series_affine(x: torch.Tensor, mode: int = AFF_NORMALIZE) -> torch.Tensor:
    """[B, 3] float64 affine coefficients (x - a0 - a1 t) * a2 from one moments pass (mode bits:
    1 detrend, 2 remove mean, 4 standardize; 1 and 2 together raise ValueError)."""
    if (mode & AFF_DETREND) and (mode & AFF_REMOVE_MEAN):
        raise ValueError("Only standardize by either removing secular trend or mean, not both.")
    x = _rows(x)
    dev = _check_dev(x)
    if x.dtype not in (torch.float32, torch.float64):
        x = _rows(x, torch.float64)
    out = torch.empty((x.shape[0], 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_series_affine", _ptr(x), int(x.dtype == torch.float64), x.stride(0),
                  x.shape[0], x.shape[1], int(mode), None, _ptr(out), _stream(dev))
    return out


def affine(x: torch.Tensor, coef: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """y = (x - a0 - a1 t) * a2 per series (coef [B, 3] float64), computed in fp64."""
    x = _rows(x)
    dev = _check_dev(x, coef)
    if x.dtype not in (torch.float32, torch.float64):
        x = _rows(x, torch.float64)
    coef = coef.to(torch.float64).contiguous()
    y = torch.empty(x.shape, dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_affine", _ptr(x), int(x.dtype == torch.float64), x.stride(0), x.shape[0],
                  x.shape[1], _ptr(coef), _ptr(y), int(dtype == torch.float64), y.stride(0),
                  _stream(dev))
    return y


# ---------------------------------------------------------------------------- CWT
# Operand checks run BEFORE anything touches a device: a wrong-sized buffer must never
# reach a kernel that indexes it by batch and scale (the kernels trust their geometry).
def _shape(a):
    return tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)


def _n_scales(scales) -> int:
    shp = _shape(scales)
    if scales is None or len(shp) != 1 or shp[0] < 1:
        raise ValueError(f"scales must be a non-empty 1-D array, got shape {shp}")
    return shp[0]


def _check_affine(a, B, name):
    if a is not None and (not isinstance(a, torch.Tensor) or tuple(a.shape) != (B, 3)):
        raise ValueError(f"{name} must be a [{B}, 3] tensor, got "
                         f"{tuple(a.shape) if isinstance(a, torch.Tensor) else type(a).__name__}")


def _check_sig(sig_scale, B, S, want_sig):
    """sig_scale: [S] (every series) or [B, S] (per series); returns sig_ld."""
    if not want_sig:
        return 0
    if sig_scale is None:
        raise ValueError("want_sig needs sig_scale")
    shp = _shape(sig_scale)
    if shp == (S,):
        return 0
    if shp == (B, S):
        return S
    raise ValueError(f"sig_scale must have shape [{S}] or [{B}, {S}], got {shp}")


def _check_out(out, shape, dtype, name):
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape)
                            or out.dtype != dtype or not out.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got "
                         f"{_shape(out)} {getattr(out, 'dtype', type(out).__name__)}")


def _f64_arg(a, dev):
    return None if a is None else a.to(device=dev, dtype=torch.float64).contiguous()


def _mother_args(mother, f0):
    """(id, parameter) for wtmi_cwt_mother / wtmi_xwt_mother: None -> Morlet(f0); else a
    wtmi / pycwt mother object or an (id, parameter) pair (wavelets.kernel_mother)."""
    if mother is None:
        return 0, float(f0)
    if isinstance(mother, tuple):
        return int(mother[0]), float(mother[1])
    from .wavelets import kernel_mother
    return kernel_mother(mother)


def cwt_morlet(x: torch.Tensor, scales, dt: float, f0: float = 6.0, *,
               affine: Optional[torch.Tensor] = None, sig_scale=None,
               want_w: bool = True, want_power: bool = False, want_sig: bool = False,
               out_w: Optional[torch.Tensor] = None, mother=None):
    """CWT of every row of x (float32 [B, n0]) at the given scales: Morlet(f0), or the
    pycwt mother ``mother`` (Paul / DOG / MexicanHat objects, wavelets.kernel_mother).

    Returns a dict with any of ``w`` (complex64 [B, S, n0]), ``power`` and ``sig``
    (float32 [B, S, n0], sig = power * sig_scale[j], or sig_scale[b, j] for a [B, S]
    sig_scale).  Every caller-supplied operand is checked against the launch geometry
    (shape, dtype, device, contiguity) before the kernel sees it.
    """
    x = _rows(x)
    B, n0 = x.shape
    S = _n_scales(scales)
    sig_ld = _check_sig(sig_scale, B, S, want_sig)
    _check_affine(affine, B, "affine")
    _check_out(out_w, (B, S, n0), torch.complex64, "out_w")
    if out_w is not None and not want_w:
        raise ValueError("out_w given with want_w=False")
    if not (want_w or want_power or want_sig):
        raise ValueError("cwt_morlet: no output requested")
    dev = _check_dev(x, affine, out_w)
    x = _rows(x, torch.float32)
    sc = _f64_dev(scales, dev)
    ss = _f64_dev(sig_scale, dev) if want_sig else None
    aff = _f64_arg(affine, dev)
    res = {}
    if want_w:
        res["w"] = out_w if out_w is not None else torch.empty((B, S, n0), dtype=torch.complex64,
                                                               device=dev)
    if want_power:
        res["power"] = torch.empty((B, S, n0), dtype=torch.float32, device=dev)
    if want_sig:
        res["sig"] = torch.empty((B, S, n0), dtype=torch.float32, device=dev)
    mid, mpar = _mother_args(mother, f0)
    if mid != 0 and n0 > 16384:
        raise ValueError("non-Morlet mothers: series of at most 16384 samples")
    ws = _long_workspace(B, n0, S, 0, dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_cwt_mother", _ptr(x), x.stride(0), B, n0, _ptr(aff), _ptr(sc), S,
                  float(dt), mid, mpar, _ptr(ss), sig_ld, _ptr(res.get("w")),
                  _ptr(res.get("power")), _ptr(res.get("sig")), _ptr(ws), _stream(dev))
    return res


SUMMARY_MAX_BANDS = 4      # include/wtmi.h: wtmi_cwt_summary
SUMMARY_MIN_N, SUMMARY_MAX_N = 9, 16384  # rows of the fused kernel; beyond, the composed path
SUMMARY_MAX_POWER_N = 8192  # band power rides on the scale loop's registers up to N = 8192


def _summary_composed(x, scales, dt, f0, mother, affine, lo, hi, pw, rw, want_global):
    """The numbers of wtmi_cwt_summary from ops.cwt_morlet over slabs of scales and fp64 torch
    reductions (rows the fused kernel does not take), in the fused path's layout and dtypes."""
    B, n0 = x.shape
    sc = np.asarray(scales.cpu() if isinstance(scales, torch.Tensor) else scales, dtype=np.float64)
    S, dev = sc.size, x.device
    slab = max(1, min(S, (1 << 28) // max(1, 16 * B * n0)))
    glob = torch.empty((B, S), dtype=torch.float64, device=dev) if want_global else None
    bp = None if pw is None else torch.zeros((B, pw.shape[0], n0), dtype=torch.float64, device=dev)
    bs = None if rw is None else torch.zeros((B, rw.shape[0], n0), dtype=torch.float64, device=dev)
    tpos = torch.arange(n0, device=dev)
    for j0 in range(0, S, slab):
        j1 = min(S, j0 + slab)
        W = cwt_morlet(x, sc[j0:j1], dt, f0, affine=affine, mother=mother)["w"].to(torch.complex128)
        P = W.real ** 2 + W.imag ** 2
        if want_global:
            m = (tpos[None, :] >= lo[j0:j1, None]) & (tpos[None, :] < hi[j0:j1, None])
            glob[:, j0:j1] = (P * m).sum(-1) / m.sum(-1)  # an empty range: 0 / 0 = NaN
        if bp is not None:
            bp += torch.einsum("kj,bjt->bkt", pw[:, j0:j1], P)
        if bs is not None:
            bs += torch.einsum("kj,bjt->bkt", rw[:, j0:j1], W.real)
    return tuple(None if t is None else t.to(torch.float32) for t in (glob, bp, bs))


def cwt_summary(x: torch.Tensor, scales, dt: float, f0: float = 6.0, *, mother=None,
                affine: Optional[torch.Tensor] = None, t_range=None, power_weights=None,
                signal_weights=None, want_global: bool = True):
    """Summaries of the CWT of every row of x (float32 [B, n0]) with no [B, S, n0] array written:
    {"global_power": [B, S] mean over time of |W_j|^2 (t_range = (t_lo, t_hi), int [S] each: the
    mean over [t_lo[j], t_hi[j]) only, NaN for an empty range), "band_power": [B, K, n0] =
    sum_j power_weights[k, j] |W_j(t)|^2, "band_signal": [B, K, n0] = sum_j signal_weights[k, j]
    Re W_j(t)}, float32, None for what was not asked.  Weights are [K, S] with K <=
    ``SUMMARY_MAX_BANDS`` (transforms.band_weights makes Torrence & Compo's eq. 24 / eq. 11 rows).
    One fused launch (wtmi_cwt_summary) for rows of ``SUMMARY_MIN_N`` .. ``SUMMARY_MAX_N`` samples
    (longer rows up to ``SUMMARY_MAX_N``: band power alone is composed, the global spectrum and the
    band signal stay fused); other lengths run ops.cwt_morlet over slabs of scales and reduce in
    fp64.  signal_weights alone is the band-pass filter: K inverse transforms, not S."""
    what = "cwt_summary"
    x = _rows(x)
    B, n0 = x.shape
    S = _n_scales(scales)
    _check_affine(affine, B, "affine")
    K = 0
    for name, w in (("power_weights", power_weights), ("signal_weights", signal_weights)):
        if w is None:
            continue
        shp = _shape(w)
        if len(shp) != 2 or shp[1] != S or not 1 <= shp[0] <= SUMMARY_MAX_BANDS or (K and shp[0] != K):
            raise ValueError(f"{what}: {name} must be [K, {S}] with 1 <= K <= {SUMMARY_MAX_BANDS} (one K for "
                             f"both weight arrays), got shape {shp}")
        K = shp[0]
    if not (want_global or K):
        raise ValueError(f"{what}: no output requested")
    if t_range is not None and (len(t_range) != 2 or _shape(t_range[0]) != (S,) or _shape(t_range[1]) != (S,)):
        raise ValueError(f"{what}: t_range must be a (t_lo, t_hi) pair of [{S}] integer arrays")
    dev = _check_dev(x, affine)
    x = _rows(x, torch.float32)
    mid, mpar = _mother_args(mother, f0)
    if mid != 0 and n0 > 16384:
        raise ValueError("non-Morlet mothers: series of at most 16384 samples")
    aff = _f64_arg(affine, dev)
    pw, rw = _f64_dev(power_weights, dev), _f64_dev(signal_weights, dev)
    lo = hi = None
    if t_range is not None and want_global:
        lo, hi = (torch.as_tensor(np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t)).to(
            device=dev, dtype=torch.int32).contiguous() for t in t_range)
    keys = ("global_power", "band_power", "band_signal")
    if not SUMMARY_MIN_N <= n0 <= SUMMARY_MAX_N:
        if lo is None:
            lo = torch.zeros(S, dtype=torch.int32, device=dev)
            hi = torch.full((S,), n0, dtype=torch.int32, device=dev)
        return dict(zip(keys, _summary_composed(x, scales, dt, f0, (mid, mpar), aff, lo.clamp(min=0),
                                                hi.clamp(max=n0), pw, rw, want_global)))
    bp = None
    if pw is not None and n0 > SUMMARY_MAX_POWER_N:  # band power alone is composed at this length
        bp = _summary_composed(x, scales, dt, f0, (mid, mpar), aff, None, None, pw, None, False)[1]
        if not want_global and rw is None:
            return dict(zip(keys, (None, bp, None)))
        pw = None
    sc = _f64_dev(scales, dev)
    glob = torch.empty((B, S), dtype=torch.float32, device=dev) if want_global else None
    if pw is not None:
        bp = torch.empty((B, K, n0), dtype=torch.float32, device=dev)
    bs = torch.empty((B, K, n0), dtype=torch.float32, device=dev) if rw is not None else None
    need = int(_lib.call("wtmi_cwt_summary_workspace_bytes", B, n0, S, K))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need > 0 else None
    with torch.cuda.device(dev):
        _lib.call("wtmi_cwt_summary", _ptr(x), x.stride(0), B, n0, _ptr(aff), _ptr(sc), S, float(dt), mid, mpar,
                  _ptr(lo), _ptr(hi), K, _ptr(pw), _ptr(rw), _ptr(glob), _ptr(bp if pw is not None else None),
                  _ptr(bs), _ptr(ws), _stream(dev))
    return dict(zip(keys, (glob, bp, bs)))


MAX_SAMPLES = 1 << 20  # longest row the engine transforms (include/wtmi.h)


def cwt_workspace_bytes(batch: int, n0: int, n_scales: int, pair: bool = False) -> int:
    """Scratch bytes of a CWT / XWT launch (0 up to 16384 samples per row)."""
    return int(_lib.call("wtmi_cwt_workspace_bytes", batch, n0, n_scales, int(pair)))


def _long_workspace(B, n0, S, pair, dev):
    if n0 > MAX_SAMPLES:
        raise ValueError(f"series of {n0} samples: the engine transforms at most {MAX_SAMPLES}")
    need = cwt_workspace_bytes(B, n0, S, bool(pair))
    return torch.empty(need, dtype=torch.uint8, device=dev) if need > 0 else None


def _pair_rows(x1, x2):
    x1 = _rows(x1, torch.float32)
    x2 = _rows(x2, torch.float32)
    if x1.shape != x2.shape:
        raise ValueError("x1 and x2 must have the same shape")
    if x1.stride(0) != x2.stride(0):
        x1, x2 = x1.contiguous(), x2.contiguous()
    return x1, x2


def xwt_morlet(x1: torch.Tensor, x2: torch.Tensor, scales, dt: float, f0: float = 6.0, *,
               affine1=None, affine2=None, sig_scale=None, want_w12=False, want_power=False,
               want_sig=False, want_uv=False, mother=None):
    """Cross-wavelet outputs of row pairs: any of w12 (complex64), power, sig, u, v.
    sig_scale: [S] or per-pair [B, S] (1 / signif).  mother: as cwt_morlet."""
    x1, x2 = _pair_rows(x1, x2)
    B, n0 = x1.shape
    S = _n_scales(scales)
    sig_ld = _check_sig(sig_scale, B, S, want_sig)
    _check_affine(affine1, B, "affine1")
    _check_affine(affine2, B, "affine2")
    if not (want_w12 or want_power or want_sig or want_uv):
        raise ValueError("xwt_morlet: no output requested")
    dev = _check_dev(x1, x2, affine1, affine2)
    sc = _f64_dev(scales, dev)
    ss = _f64_dev(sig_scale, dev) if want_sig else None
    a1, a2 = _f64_arg(affine1, dev), _f64_arg(affine2, dev)
    shape = (B, S, n0)
    res = {}
    if want_w12:
        res["w12"] = torch.empty(shape, dtype=torch.complex64, device=dev)
    if want_power:
        res["power"] = torch.empty(shape, dtype=torch.float32, device=dev)
    if want_sig:
        res["sig"] = torch.empty(shape, dtype=torch.float32, device=dev)
    if want_uv:
        res["u"] = torch.empty(shape, dtype=torch.float32, device=dev)
        res["v"] = torch.empty(shape, dtype=torch.float32, device=dev)
    mid, mpar = _mother_args(mother, f0)
    if mid != 0 and n0 > 16384:
        raise ValueError("non-Morlet mothers: series of at most 16384 samples")
    ws = _long_workspace(B, n0, S, 1, dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_xwt_mother", _ptr(x1), _ptr(x2), x1.stride(0), B, n0, _ptr(a1), _ptr(a2),
                  _ptr(sc), S, float(dt), mid, mpar, _ptr(ss), sig_ld, _ptr(res.get("w12")),
                  _ptr(res.get("power")), _ptr(res.get("sig")), _ptr(res.get("u")),
                  _ptr(res.get("v")), _ptr(ws), _stream(dev))
    return res


def wct_workspace_bytes(batch: int, n0: int, n_scales: int) -> int:
    return int(_lib.call("wtmi_wct_workspace_bytes", batch, n0, n_scales))


def wct_morlet(x1: torch.Tensor, x2: torch.Tensor, scales, dt: float, f0: float = 6.0, *,
               boxcar: int, affine1=None, affine2=None, want_uv: bool = True,
               want_power: bool = False, want_phase: bool = False,
               workspace: Optional[torch.Tensor] = None, normalize: bool = False):
    """Wavelet coherence of row pairs; returns dict coh [B,S,n0] (+ u, v, power =
    |W1 W2*|^2, phase = angle(W1 W2*)).  normalize: pycwt's (y - mean) / std of each series,
    done inside the transform (wtmi_wct_morlet_norm; rows of 9..16384 samples, affine must
    then be None)."""
    x1, x2 = _pair_rows(x1, x2)
    B, n0 = x1.shape
    S = _n_scales(scales)
    _check_affine(affine1, B, "affine1")
    _check_affine(affine2, B, "affine2")
    if n0 > MAX_SAMPLES:
        raise ValueError(f"series of {n0} samples: the engine transforms at most {MAX_SAMPLES}")
    if int(boxcar) < 1:
        raise ValueError("boxcar must be >= 1")
    need = wct_workspace_bytes(B, n0, S)
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or
                                  workspace.dtype != torch.uint8 or not workspace.is_contiguous()
                                  or workspace.numel() < need):
        raise ValueError(f"workspace must be a contiguous uint8 tensor of >= {need} bytes")
    dev = _check_dev(x1, x2, affine1, affine2, workspace)
    sc = _f64_dev(scales, dev)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    shape = (B, S, n0)
    res = {"coh": torch.empty(shape, dtype=torch.float32, device=dev)}
    if want_power:
        res["power"] = torch.empty(shape, dtype=torch.float32, device=dev)
    if want_phase:
        res["phase"] = torch.empty(shape, dtype=torch.float32, device=dev)
    if want_uv:
        res["u"] = torch.empty(shape, dtype=torch.float32, device=dev)
        res["v"] = torch.empty(shape, dtype=torch.float32, device=dev)
    a1, a2 = _f64_arg(affine1, dev), _f64_arg(affine2, dev)
    if normalize and (a1 is not None or a2 is not None or not 8 < n0 <= 16384):
        raise ValueError("normalize=True: rows of 9..16384 samples and no affine coefficients")
    with torch.cuda.device(dev):
        if normalize:
            _lib.call("wtmi_wct_morlet_norm", _ptr(x1), _ptr(x2), x1.stride(0), B, n0, _ptr(sc), S,
                      float(dt), float(f0), int(boxcar), _ptr(workspace), _ptr(res["coh"]),
                      _ptr(res.get("power")), _ptr(res.get("phase")), _ptr(res.get("u")),
                      _ptr(res.get("v")), _stream(dev))
        else:
            _lib.call("wtmi_wct_morlet", _ptr(x1), _ptr(x2), x1.stride(0), B, n0, _ptr(a1), _ptr(a2),
                      _ptr(sc), S, float(dt), float(f0), int(boxcar), _ptr(workspace),
                      _ptr(res["coh"]), _ptr(res.get("power")), _ptr(res.get("phase")),
                      _ptr(res.get("u")), _ptr(res.get("v")), _stream(dev))
    return res


NOISE_MODES = ("pycwt", "red")


def rednoise(count: int, n: int, g: float, seed: int, *, first_series: int = 0,
             device=None, out: Optional[torch.Tensor] = None, noise: str = "pycwt") -> torch.Tensor:
    """[count, n] float32 Monte-Carlo noise, pycwt helpers.rednoise(n, g, 1) per row, drawn on
    the GPU from Philox4x32-10 stream (seed, first_series + row).  noise="pycwt" (default) is
    pycwt's literal behaviour: its lfilter runs along the length-1 axis of randn(n + tau, 1),
    so the rows are white normals (g sets only the burn-in tau); noise="red" applies the AR(1)
    filter the MATLAB original intends."""
    if noise not in NOISE_MODES:
        raise ValueError(f"noise must be one of {NOISE_MODES}, got {noise!r}")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.empty((count, n), dtype=torch.float32, device=dev)
    _check_dev(out)
    with torch.cuda.device(out.device):
        _lib.call("wtmi_rednoise", _ptr(out), out.stride(0), count, n, float(g), int(noise == "red"),
                  C.c_ulonglong(int(seed) & ((1 << 64) - 1)), C.c_ulonglong(int(first_series)),
                  _stream(out.device))
    return out


def wct_side_streams() -> int:
    """Side streams the full-row WCT has created in this process (the pool's size)."""
    return int(_lib.load().wtmi_wct_side_streams())


def coherence_histogram(coh: torch.Tensor, t_lo: torch.Tensor, t_hi: torch.Tensor,
                        n_hist_scales: int, nbins: int = 1000,
                        hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Accumulate floor(coh * nbins) counts of coh [B, S, n0] over t in [t_lo[s], t_hi[s])
    for s < n_hist_scales into hist [n_hist_scales, nbins] (int32 view of uint32)."""
    if coh.dim() == 2:
        coh = coh.unsqueeze(0)
    coh = coh.to(torch.float32).contiguous()
    dev = _check_dev(coh)
    B, S, n0 = coh.shape
    lo = t_lo.to(device=dev, dtype=torch.int32).contiguous()
    hi = t_hi.to(device=dev, dtype=torch.int32).contiguous()
    if lo.numel() < n_hist_scales or hi.numel() < n_hist_scales:
        raise ValueError("t_lo / t_hi need one entry per histogram scale")
    if hist is None:
        hist = torch.zeros((n_hist_scales, nbins), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_coherence_histogram", _ptr(coh), B, n0, S, _ptr(lo), _ptr(hi),
                  int(n_hist_scales), int(nbins), _ptr(hist), _stream(dev))
    return hist


def coherence_quantile(hist: torch.Tensor, n_scales: int, level: float) -> torch.Tensor:
    """Per-scale level of the Monte-Carlo counter hist [>= n_scales, nbins] (int32 view of
    uint32) at `level` (wct_significance's quantile step, on the device): float64 [n_scales]."""
    dev = _check_dev(hist)
    hist = hist.contiguous()
    if hist.dim() != 2 or hist.shape[0] < n_scales:
        raise ValueError("hist must be [>= n_scales, nbins]")
    out = torch.empty(max(n_scales, 1), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_coherence_quantile", _ptr(hist), int(n_scales), int(hist.shape[1]), float(level),
                  _ptr(out), _stream(dev))
    return out[:n_scales]


# -------------------------------------------------------------------------- MODWT
def _taps(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _tp(arr: np.ndarray):
    return arr.ctypes.data_as(VP)


def _out(out, shape, dev):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() \
            or out.device != dev:
        raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(shape)} on {dev}")
    return out


def modwt(x: torch.Tensor, dec_lo, dec_hi, level: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, n] float32 -> [B, level + 1, n] rows [W_1 .. W_J, V_J]."""
    x = _rows(x, torch.float32)
    dev = _check_dev(x)
    B, n = x.shape
    lo, hi = _taps(dec_lo), _taps(dec_hi)
    w = _out(out, (B, level + 1, n), dev)
    ws = _scratch(_lib.call("wtmi_modwt_workspace_bytes", B, n, int(level)), dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_modwt", _ptr(x), x.stride(0), B, n, _tp(lo), _tp(hi), lo.size, int(level),
                  _ptr(w), _ptr(ws), _stream(dev))
    return w


def _scratch(nbytes: int, dev):
    """Device scratch of a long-series launch (None when the call needs none)."""
    if nbytes < 0:
        raise ValueError("invalid geometry")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes > 0 else None


def imodwt(w: torch.Tensor, dec_lo, dec_hi, keep_mask: Optional[int] = None,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, J + 1, n] -> [B, n]; rows with a clear bit in keep_mask count as zero."""
    if w.dim() == 2:
        w = w.unsqueeze(0)
    w = w.to(torch.float32).contiguous()
    dev = _check_dev(w)
    B, R, n = w.shape
    lo, hi = _taps(dec_lo), _taps(dec_hi)
    keep = (1 << 64) - 1 if keep_mask is None else int(keep_mask)
    x = _out(out, (B, n), dev)
    ws = _scratch(_lib.call("wtmi_modwt_workspace_bytes", B, n, R - 1), dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_imodwt", _ptr(w), B, n, _tp(lo), _tp(hi),
                  lo.size, R - 1, C.c_ulonglong(keep), _ptr(x), x.stride(0), _ptr(ws), _stream(dev))
    return x


# ---------------------------------------------------------------------------- DWT
def dwt_lengths(n: int, n_taps: int, level: int) -> list:
    lens = (C.c_longlong * (level + 1))()
    total = _lib.call("wtmi_dwt_lengths", n, n_taps, level, C.cast(lens, VP))
    if total < 0:
        raise ValueError("invalid DWT geometry")
    return list(lens)


def wavedec(x: torch.Tensor, dec_lo, dec_hi, level: int):
    """Returns (coeffs [B, total] float32 in pywt order, lens)."""
    x = _rows(x, torch.float32)
    dev = _check_dev(x)
    B, n = x.shape
    lo, hi = _taps(dec_lo), _taps(dec_hi)
    lens = dwt_lengths(n, lo.size, level)
    coeffs = torch.empty((B, sum(lens)), dtype=torch.float32, device=dev)
    ws = _scratch(_lib.call("wtmi_dwt_workspace_bytes", B, n, lo.size, 1), dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_wavedec", _ptr(x), x.stride(0), B, n, _tp(lo), _tp(hi), lo.size, int(level),
                  _ptr(coeffs), _ptr(ws), _stream(dev))
    return coeffs, lens


def waverec(coeffs: torch.Tensor, n: int, rec_lo, rec_hi, level: int,
            keep_masks: Sequence[int]) -> torch.Tensor:
    """[B, total] -> [B, V, out_len]: one reconstruction per keep mask (bit k keeps
    list entry k of [cA_J, cD_J, ..., cD_1])."""
    if coeffs.dim() == 1:
        coeffs = coeffs.unsqueeze(0)
    coeffs = coeffs.to(torch.float32).contiguous()
    dev = _check_dev(coeffs)
    lo, hi = _taps(rec_lo), _taps(rec_hi)
    lens = dwt_lengths(n, lo.size, level)
    out_len = 2 * lens[-1] - lo.size + 2 if level > 0 else n
    masks = torch.as_tensor(np.asarray([int(m) & ((1 << 64) - 1) for m in keep_masks],
                                       dtype=np.uint64).view(np.int64), device=dev)
    B = coeffs.shape[0]
    out = torch.empty((B, len(keep_masks), out_len), dtype=torch.float32, device=dev)
    if level == 0 and n > 16384:  # nothing to invert: the kept cA_0 is the series
        keep = torch.tensor([float(int(m) & 1) for m in keep_masks], device=dev)
        return coeffs[:, None, :n] * keep[None, :, None]
    ws = _scratch(_lib.call("wtmi_dwt_workspace_bytes", B, n, lo.size, len(keep_masks)), dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_waverec", _ptr(coeffs), B, n, _tp(lo), _tp(hi), lo.size, int(level),
                  _ptr(masks), len(keep_masks),
                  _ptr(out), out_len, _ptr(ws), _stream(dev))
    return out


# ---------------------------------------------------------- time-scale regression
TSR_MAX_N = 8192   # longest row of the fused kernel (include/wtmi.h: wtmi_dwt_tsr)
TSR_MAX_TAPS = 40
STATS = ("const", "slope", "bse_const", "bse_slope", "rsquared", "ssr", "nobs", "df_resid")


def _ols_rows(x, y, what):
    """The operand checks of a regression's row pair (before any device is touched): tensors of
    equal shape, float32, [n] or [B, n]."""
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be float32 rows, got {t.dtype}")
    if x.shape != y.shape:
        raise ValueError(f"{what}: x and y must have the same shape, got {tuple(x.shape)} and "
                         f"{tuple(y.shape)}")
    if x.dim() not in (1, 2) or x.shape[-1] < 1:
        raise ValueError(f"{what}: expected [n] or [batch, n] rows, got shape {tuple(x.shape)}")


def _series_or_pair(x, y, what, has_output):
    """Operand checks and placement of "x alone or an (x, y) pair": (device, x rows, y rows or
    None).  has_output: whether anything is requested that a single series can deliver."""
    if y is None:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() not in (1, 2) \
                or x.shape[-1] < 1:
            raise ValueError(f"{what}: x must be float32 [n] or [batch, n] rows")
        if not has_output:
            raise ValueError(f"{what}: no output requested")
        return _check_dev(x), _rows(x), None
    _ols_rows(x, y, what)
    return (_check_dev(x, y), *_pair_rows(x, y))


def _int_level(level, lo, hi, what):
    """level as an int in lo..hi (hi None: unbounded); what: the message's prefix, or None."""
    if int(level) != level or level < lo or (hi is not None and level > hi):
        rng = f">= {lo}" if hi is None else f"in {lo}..{hi}"
        raise ValueError(f"{what + ': ' if what else ''}level must be an integer {rng}, got {level!r}")
    return int(level)


def _bank(what, **taps):
    """Two or four named tap arrays as contiguous float64: 1-D, the same number (>= 2) of taps."""
    arrs = [_taps(a) for a in taps.values()]
    F = arrs[0].size
    if any(t.ndim != 1 or t.size != F for t in arrs) or F < 2:
        names = list(taps)
        got = f"{arrs[0].shape} and {arrs[1].shape}" if len(arrs) == 2 else f"{[t.shape for t in arrs]}"
        raise ValueError(f"{what + ': ' if what else ''}{', '.join(names[:-1])} and {names[-1]} must hold the "
                         f"same number of taps (>= 2), got {got}")
    return arrs


def rows_ols(x_rows: torch.Tensor, y_rows: torch.Tensor, add_constant: bool = True) -> torch.Tensor:
    """OLS of y row r on [1, x row r] (or on the x row alone) for float32 [R, n] row pairs:
    [R, 8] float64 = ``STATS`` (wtmi_rows_ols; nobs = n)."""
    _ols_rows(x_rows, y_rows, "rows_ols")
    dev = _check_dev(x_rows, y_rows)
    x, y = _pair_rows(x_rows, y_rows)
    R, n = x.shape
    stats = torch.empty((R, 8), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_rows_ols", _ptr(x), _ptr(y), x.stride(0), R, n, int(bool(add_constant)),
                  _ptr(stats), _stream(dev))
    return stats


def dwt_time_scale_regression(x: torch.Tensor, y: torch.Tensor, dec_lo, dec_hi, rec_lo, rec_hi,
                              level: int, *, add_constant: bool = True,
                              want_components: bool = False):
    """Per-component OLS of y on x over the DWT components S_J, D_J .. D_1 (pywt list order):
    {"stats": [B, level + 1, 8] float64 (``STATS``), "components": [B, 2, level + 1, out_len]
    float32 (0 = x) or None}.  Rows of at most ``TSR_MAX_N`` samples (and even filters of at most
    ``TSR_MAX_TAPS`` taps) take ONE fused launch; longer ones compose wavedec, waverec with the
    level + 1 one-bit masks and rows_ols."""
    _ols_rows(x, y, "dwt_time_scale_regression")
    level = _int_level(level, 0, None, None)
    taps = _bank(None, dec_lo=dec_lo, dec_hi=dec_hi, rec_lo=rec_lo, rec_hi=rec_hi)
    F = taps[0].size
    dev = _check_dev(x, y)
    x, y = _pair_rows(x, y)
    B, n = x.shape
    if n > TSR_MAX_N or F % 2 or F > TSR_MAX_TAPS:
        masks = [1 << k for k in range(level + 1)]
        comps = torch.stack([waverec(wavedec(r, taps[0], taps[1], level)[0], n, taps[2], taps[3],
                                     level, masks) for r in (x, y)], dim=1).contiguous()
        out_len = comps.shape[-1]
        stats = rows_ols(comps[:, 0].reshape(-1, out_len), comps[:, 1].reshape(-1, out_len),
                         add_constant).reshape(B, level + 1, 8)
        return {"stats": stats, "components": comps if want_components else None}
    out_len = 2 * dwt_lengths(n, F, level)[-1] - F + 2 if level > 0 else n
    stats = torch.empty((B, level + 1, 8), dtype=torch.float64, device=dev)
    comps = torch.empty((B, 2, level + 1, out_len), dtype=torch.float32, device=dev) \
        if want_components else None
    with torch.cuda.device(dev):
        _lib.call("wtmi_dwt_tsr", _ptr(x), _ptr(y), x.stride(0), B, n, *map(_tp, taps),
                  F, level, int(bool(add_constant)), _ptr(stats), _ptr(comps), _stream(dev))
    return {"stats": stats, "components": comps}


SMOOTH_MAX_LEVEL = 60  # include/wtmi.h: wtmi_dwt_smooth (the fused path shares TSR_MAX_N / TSR_MAX_TAPS)


def dwt_smooth(x: torch.Tensor, dec_lo, rec_lo, level: int, *, y: Optional[torch.Tensor] = None,
               add_constant: bool = True, want_smooth: bool = True):
    """The DWT smoothing ladder of float32 rows x ([n] or [B, n]) and, with y, the OLS of the raw
    y on every smooth: {"smooth": [B, level, n] float32 (row l - 1 = the reference's
    smooth_signal(...)[l]["signal"], trimmed to n samples) or None, "stats": [B, level, 8]
    float64 (``STATS``, nobs = n) or None without y}.  Rows of at most ``TSR_MAX_N`` samples and
    even filters of at most ``TSR_MAX_TAPS`` taps take ONE fused launch (wtmi_dwt_smooth), which
    needs the low-pass pair alone; beyond, wavedec, waverec with the ``level`` keep-masks, the
    trim and rows_ols compose, with the high-pass pair taken as the quadrature mirror of the
    low-pass one (dec_hi[k] = (-1)^(k+1) rec_lo[k], rec_hi[k] = (-1)^k dec_lo[k]: every pywt bank)."""
    what = "dwt_smooth"
    level = _int_level(level, 1, SMOOTH_MAX_LEVEL, what)
    lo_d, lo_r = _bank(what, dec_lo=dec_lo, rec_lo=rec_lo)
    dev, x, y = _series_or_pair(x, y, what, want_smooth)
    B, n = x.shape
    F = lo_d.size
    if n > TSR_MAX_N or F % 2 or F > TSR_MAX_TAPS:
        sign = (-1.0) ** np.arange(F)
        masks = [(1 << (level + 1 - l)) - 1 for l in range(1, level + 1)]  # drop cD_1 .. cD_l
        rec = waverec(wavedec(x, lo_d, -sign * lo_r, level)[0], n, lo_r, sign * lo_d, level, masks)
        smooth = rec[:, :, rec.shape[-1] - n:].contiguous()  # trim_signal: odd n drops sample 0
        stats = None if y is None else rows_ols(
            smooth.reshape(-1, n), y[:, None, :].expand(B, level, n).reshape(-1, n),
            add_constant).reshape(B, level, 8)
        return {"smooth": smooth if want_smooth else None, "stats": stats}
    smooth = torch.empty((B, level, n), dtype=torch.float32, device=dev) if want_smooth else None
    stats = torch.empty((B, level, 8), dtype=torch.float64, device=dev) if y is not None else None
    with torch.cuda.device(dev):
        _lib.call("wtmi_dwt_smooth", _ptr(x), _ptr(y), x.stride(0), B, n, _tp(lo_d), _tp(lo_r), F,
                  level, int(bool(add_constant)), _ptr(smooth), _ptr(stats),
                  _stream(dev))
    return {"smooth": smooth, "stats": stats}


# ----------------------------------------------------------- wavelet shrinkage
DENOISE_RULES = {"fixed": 0, "universal": 1, "level": 2}
DENOISE_SHRINK = {"soft": 0, "hard": 1, "garrote": 2}
DENOISE_INFO = ("sigma", "threshold", "kept", "len")
MAD_SCALE = 0.6744897501960817  # the normal distribution's upper quartile: sigma = MAD / this


def _denoise_composed(x, taps, level, rule, shrink, mult, thr):
    """The numbers of wtmi_dwt_denoise from wavedec, torch order statistics and ``where`` per
    level, and waverec: (denoised [B, n], info [B, level, 4], shrunk coeffs [B, total])."""
    B, n = x.shape
    coeffs, lens = wavedec(x, taps[0], taps[1], level)
    info = torch.full((B, level, 4), float("nan"), dtype=torch.float64, device=x.device)
    scale = mult * float(np.sqrt(2.0 * np.log(n)))
    end, sigma = coeffs.shape[1], None
    for j in range(1, level + 1):  # cD_j is list entry level + 1 - j: the arrays run backwards
        m = lens[level + 1 - j]
        c = coeffs[:, end - m:end]
        end -= m
        mag = c.abs()
        if rule == 0:
            lam = thr[:, j - 1]
        else:
            if rule == 2 or j == 1:
                s = torch.sort(mag, dim=1).values[:, [(m - 1) // 2, m // 2]].to(torch.float64)
                sigma = 0.5 * (s[:, 0] + s[:, 1]) / MAD_SCALE
            lam = scale * sigma
            info[:, j - 1, 0] = sigma
        lf = lam.to(torch.float32)[:, None]
        keep = mag >= lf if shrink == 1 else mag > lf
        if shrink == 0:
            val = torch.copysign(mag - lf, c)
        elif shrink == 1:
            val = c
        else:
            val = c - lf * (lf / torch.where(keep, c, torch.ones_like(c)))
        c.copy_(torch.where(keep, val, torch.zeros_like(c)))
        info[:, j - 1, 1] = lam
        info[:, j - 1, 2] = keep.sum(dim=1)
        info[:, j - 1, 3] = m
    rec = waverec(coeffs, n, taps[2], taps[3], level, [(1 << (level + 1)) - 1])
    return rec[:, 0, :n].contiguous(), info, coeffs


def dwt_denoise(x: torch.Tensor, dec_lo, dec_hi, rec_lo, rec_hi, level: int, *, rule: str = "universal",
                shrink: str = "soft", mult: float = 1.0, thresholds=None, want_info: bool = True,
                want_coeffs: bool = False):
    """Wavelet shrinkage of float32 rows x ([n] or [B, n]): wavedec (mode symmetric), a threshold
    per detail level, pywt.threshold of the detail arrays and the first n samples of waverec:
    {"denoised": [B, n] float32, "info": [B, level, 4] float64 (``DENOISE_INFO``, row j - 1 =
    level j) or None, "coeffs": [B, total] float32 (the shrunk list, wavedec's layout) or None}.
    rule "universal": lambda = mult sigma sqrt(2 ln n) with sigma = median(|cD_1|) / ``MAD_SCALE``;
    "level": the same with sigma_j from cD_j; "fixed": ``thresholds`` ([level] or [B, level],
    float64) and mult ignored.  shrink: "soft", "hard" or "garrote" (non-negative garrote).  Rows
    of at most ``TSR_MAX_N`` samples, even filters of at most ``TSR_MAX_TAPS`` taps and levels up
    to ``SMOOTH_MAX_LEVEL`` take ONE fused launch (wtmi_dwt_denoise); beyond, wavedec, torch order
    statistics and waverec compose the same numbers."""
    what = "dwt_denoise"
    level = _int_level(level, 1, None, what)
    taps = _bank(what, dec_lo=dec_lo, dec_hi=dec_hi, rec_lo=rec_lo, rec_hi=rec_hi)
    if rule not in DENOISE_RULES:
        raise ValueError(f"{what}: rule must be one of {sorted(DENOISE_RULES)}, got {rule!r}")
    if shrink not in DENOISE_SHRINK:
        raise ValueError(f"{what}: shrink must be one of {sorted(DENOISE_SHRINK)}, got {shrink!r}")
    mult = float(mult)
    if not (mult >= 0.0 and np.isfinite(mult)):
        raise ValueError(f"{what}: mult must be finite and >= 0, got {mult!r}")
    fixed = rule == "fixed"
    if fixed != (thresholds is not None):
        raise ValueError(f"{what}: thresholds go with rule 'fixed' and with no other")
    if fixed and (len(_shape(thresholds)) not in (1, 2) or _shape(thresholds)[-1] != level):
        raise ValueError(f"{what}: thresholds must be [{level}] or [batch, {level}], got shape "
                         f"{_shape(thresholds)}")
    dev, x, _ = _series_or_pair(x, None, what, True)
    B, n = x.shape
    thr = _f64_dev(thresholds, dev)
    if fixed and thr.dim() == 2 and thr.shape[0] != B:
        raise ValueError(f"{what}: {thr.shape[0]} threshold rows for {B} series")
    F = taps[0].size
    r, s = DENOISE_RULES[rule], DENOISE_SHRINK[shrink]
    if n > TSR_MAX_N or F % 2 or F > TSR_MAX_TAPS or level > SMOOTH_MAX_LEVEL:
        den, info, coeffs = _denoise_composed(x, taps, level, r, s, mult,
                                              thr.reshape(-1, level).expand(B, level) if fixed else None)
        return {"denoised": den, "info": info if want_info else None, "coeffs": coeffs if want_coeffs else None}
    den = torch.empty((B, n), dtype=torch.float32, device=dev)
    info = torch.empty((B, level, 4), dtype=torch.float64, device=dev) if want_info else None
    coeffs = torch.empty((B, sum(dwt_lengths(n, F, level))), dtype=torch.float32, device=dev) \
        if want_coeffs else None
    with torch.cuda.device(dev):
        _lib.call("wtmi_dwt_denoise", _ptr(x), x.stride(0), B, n, *map(_tp, taps), F, level, r, s,
                  C.c_double(mult), _ptr(thr), level if fixed and thr.dim() == 2 else 0,
                  _ptr(den), n, _ptr(info), _ptr(coeffs), _stream(dev))
    return {"denoised": den, "info": info, "coeffs": coeffs}


# ------------------------------------------------------------------- MODWT MRA
MRA_MAX_N = 16384  # longest row of the fused kernels (include/wtmi.h: wtmi_modwt_mra)
MRA_MAX_TAPS = 40
MRA_MAX_LEVEL = 62  # the a-trous dilation 2^(level - 1) as a long long (wtmi_modwt_mra, _rows, wtmi_modwt_wcorr)


def _masked_rows(w, lo, hi):
    """[B, J + 1, n] coefficient rows -> MRA rows, one one-bit-mask inverse per row."""
    return torch.stack([imodwt(w, lo, hi, 1 << j) for j in range(w.shape[1])], dim=1)


def modwt_mra(x: torch.Tensor, dec_lo, dec_hi, level: int, *, y: Optional[torch.Tensor] = None,
              add_constant: bool = True, want_components: bool = True, want_smooths: bool = False):
    """MODWT multiresolution analysis of float32 rows x ([n] or [B, n]; with y, of the pairs
    (x, y)): {"components": [B, P, level + 1, n] rows [D_1 .. D_J, S_J] (P = 2 with y, 0 = x),
    "smooths": [B, P, level, n] (row l - 1 = the reference's smooth_signal key l),
    "stats": [B, level + 1, 8] float64 (``STATS``; OLS of y's row on x's row, MRA row order)};
    entries not requested (and stats without y) are None.  Rows of at most ``MRA_MAX_N``
    samples and filters of at most ``MRA_MAX_TAPS`` taps take ONE fused launch
    (wtmi_modwt_mra); beyond, modwt, one-bit-mask imodwt, suffix sums and rows_ols compose."""
    what = "modwt_mra"
    level = _int_level(level, 1, MRA_MAX_LEVEL, what)
    lo, hi = _bank(what, dec_lo=dec_lo, dec_hi=dec_hi)
    dev, x, y = _series_or_pair(x, y, what, want_components or want_smooths)
    B, n = x.shape
    P = 1 if y is None else 2
    if n > MRA_MAX_N or lo.size > MRA_MAX_TAPS:
        comps = torch.stack([_masked_rows(modwt(r, lo, hi, level), lo, hi)
                             for r in ((x,) if y is None else (x, y))], dim=1)
        stats = None if y is None else rows_ols(
            comps[:, 0].reshape(-1, n), comps[:, 1].reshape(-1, n), add_constant).reshape(B, level + 1, 8)
        smooths = comps.flip(2).cumsum(2).flip(2)[:, :, 1:].contiguous() if want_smooths else None
        return {"components": comps if want_components else None, "smooths": smooths, "stats": stats}
    comps = torch.empty((B, P, level + 1, n), dtype=torch.float32, device=dev) if want_components else None
    smooths = torch.empty((B, P, level, n), dtype=torch.float32, device=dev) if want_smooths else None
    stats = torch.empty((B, level + 1, 8), dtype=torch.float64, device=dev) if y is not None else None
    with torch.cuda.device(dev):
        _lib.call("wtmi_modwt_mra", _ptr(x), _ptr(y), x.stride(0), B, n, _tp(lo), _tp(hi), lo.size,
                  level, int(bool(add_constant)), _ptr(comps),
                  _ptr(smooths), _ptr(stats), _stream(dev))
    return {"components": comps, "smooths": smooths, "stats": stats}


def modwt_mra_rows(w: torch.Tensor, dec_lo, dec_hi) -> torch.Tensor:
    """MRA rows [D_1 .. D_J, S_J] of coefficient rows that already exist (the reference's
    modwtmra(w, filters)): float32 [J + 1, n] or [B, J + 1, n] -> [B, J + 1, n].  One launch
    (wtmi_modwt_mra_rows) within ``MRA_MAX_N`` / ``MRA_MAX_TAPS``; one-bit-mask imodwt beyond."""
    what = "modwt_mra_rows"
    lo, hi = _bank(what, dec_lo=dec_lo, dec_hi=dec_hi)
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() not in (2, 3) \
            or w.shape[-2] < 2 or w.shape[-1] < 1:
        raise ValueError(f"{what}: w must be float32 [levels + 1, n] or [batch, levels + 1, n] rows")
    dev = _check_dev(w)
    w = (w.unsqueeze(0) if w.dim() == 2 else w).contiguous()
    B, R, n = w.shape
    _int_level(R - 1, 1, MRA_MAX_LEVEL, what)
    if n > MRA_MAX_N or lo.size > MRA_MAX_TAPS:
        return _masked_rows(w, lo, hi)
    out = torch.empty_like(w)
    with torch.cuda.device(dev):
        _lib.call("wtmi_modwt_mra_rows", _ptr(w), B, n, _tp(lo), _tp(hi),
                  lo.size, R - 1, _ptr(out), _stream(dev))
    return out


# ------------------------------------------ MODWT translation-invariant shrinkage
MODWT_DENOISE_MAX_N = 16384  # longest row of the fused kernel (include/wtmi.h: wtmi_modwt_denoise)


def _modwt_denoise_composed(x, lo, hi, level, rule, shrink, mult, thr):
    """The numbers of wtmi_modwt_denoise from modwt rows, torch order statistics and ``where`` per
    level, and imodwt: (denoised [B, n], info [B, level, 4], shrunk rows [B, level + 1, n])."""
    B, n = x.shape
    w = modwt(x, lo, hi, level)
    info = torch.full((B, level, 4), float("nan"), dtype=torch.float64, device=x.device)
    scale = mult * float(np.sqrt(2.0 * np.log(n)))
    base = None
    for j in range(1, level + 1):
        c = w[:, j - 1]
        mag = c.abs()
        up = 2.0 ** (j // 2) * (float(np.sqrt(2.0)) if j & 1 else 1.0)  # 2^(j/2)
        if rule == 0:
            lam = thr[:, j - 1]
        else:
            if rule == 2 or j == 1:
                s = torch.sort(mag, dim=1).values[:, [(n - 1) // 2, n // 2]].to(torch.float64)
                s0 = 0.5 * (s[:, 0] + s[:, 1]) / MAD_SCALE
                base = float(np.sqrt(2.0)) * s0  # universal: sigma
            lam = scale * s0 if rule == 2 else scale * base / up
            info[:, j - 1, 0] = s0 * up if rule == 2 else base
        lf = lam.to(torch.float32)[:, None]
        keep = mag >= lf if shrink == 1 else mag > lf
        if shrink == 0:
            val = torch.copysign(mag - lf, c)
        elif shrink == 1:
            val = c
        else:
            val = c - lf * (lf / torch.where(keep, c, torch.ones_like(c)))
        c.copy_(torch.where(keep, val, torch.zeros_like(c)))
        info[:, j - 1, 1] = lam
        info[:, j - 1, 2] = keep.sum(dim=1)
        info[:, j - 1, 3] = n
    return imodwt(w, lo, hi), info, w


def modwt_denoise(x: torch.Tensor, dec_lo, dec_hi, level: int, *, rule: str = "universal",
                  shrink: str = "soft", mult: float = 1.0, thresholds=None, want_info: bool = True,
                  want_coeffs: bool = False):
    """Translation-invariant wavelet shrinkage of float32 rows x ([n] or [B, n]): modwt, a threshold
    per detail level, the shrink of ``dwt_denoise`` on every W~_j, and imodwt of the shrunk rows:
    {"denoised": [B, n] float32, "info": [B, level, 4] float64 (``DENOISE_INFO``, row j - 1 =
    level j) or None, "coeffs": [B, level + 1, n] float32 (the shrunk rows, modwt's row order) or
    None}.  rule "universal": lambda_j = mult sigma sqrt(2 ln n) / 2^(j/2) with sigma = sqrt2
    median(|W~_1|) / ``MAD_SCALE``; "level": the same with sigma_j = 2^(j/2) median(|W~_j|) /
    ``MAD_SCALE``; "fixed": ``thresholds`` ([level] or [B, level], float64) and mult ignored.
    shrink: "soft", "hard" or "garrote".  Rows of at most ``MODWT_DENOISE_MAX_N`` samples and
    filters of at most ``MRA_MAX_TAPS`` taps take ONE fused launch (wtmi_modwt_denoise); beyond,
    modwt, torch order statistics and imodwt compose the same numbers."""
    what = "modwt_denoise"
    level = _int_level(level, 1, MRA_MAX_LEVEL, what)
    lo, hi = _bank(what, dec_lo=dec_lo, dec_hi=dec_hi)
    if rule not in DENOISE_RULES:
        raise ValueError(f"{what}: rule must be one of {sorted(DENOISE_RULES)}, got {rule!r}")
    if shrink not in DENOISE_SHRINK:
        raise ValueError(f"{what}: shrink must be one of {sorted(DENOISE_SHRINK)}, got {shrink!r}")
    mult = float(mult)
    if not (mult >= 0.0 and np.isfinite(mult)):
        raise ValueError(f"{what}: mult must be finite and >= 0, got {mult!r}")
    fixed = rule == "fixed"
    if fixed != (thresholds is not None):
        raise ValueError(f"{what}: thresholds go with rule 'fixed' and with no other")
    if fixed and (len(_shape(thresholds)) not in (1, 2) or _shape(thresholds)[-1] != level):
        raise ValueError(f"{what}: thresholds must be [{level}] or [batch, {level}], got shape "
                         f"{_shape(thresholds)}")
    dev, x, _ = _series_or_pair(x, None, what, True)
    B, n = x.shape
    thr = _f64_dev(thresholds, dev)
    if fixed and thr.dim() == 2 and thr.shape[0] != B:
        raise ValueError(f"{what}: {thr.shape[0]} threshold rows for {B} series")
    r, s = DENOISE_RULES[rule], DENOISE_SHRINK[shrink]
    if n > MODWT_DENOISE_MAX_N or lo.size > MRA_MAX_TAPS:
        den, info, coeffs = _modwt_denoise_composed(x, lo, hi, level, r, s, mult,
                                                    thr.reshape(-1, level).expand(B, level) if fixed else None)
        return {"denoised": den, "info": info if want_info else None, "coeffs": coeffs if want_coeffs else None}
    den = torch.empty((B, n), dtype=torch.float32, device=dev)
    info = torch.empty((B, level, 4), dtype=torch.float64, device=dev) if want_info else None
    coeffs = torch.empty((B, level + 1, n), dtype=torch.float32, device=dev) if want_coeffs else None
    ws = None if want_coeffs else _scratch(_lib.call("wtmi_modwt_denoise_workspace_bytes", B, n, level), dev)
    with torch.cuda.device(dev):
        _lib.call("wtmi_modwt_denoise", _ptr(x), x.stride(0), B, n, _tp(lo), _tp(hi), lo.size, level, r, s,
                  C.c_double(mult), _ptr(thr), level if fixed and thr.dim() == 2 else 0,
                  _ptr(den), n, _ptr(info), _ptr(coeffs), _ptr(ws), _stream(dev))
    return {"denoised": den, "info": info, "coeffs": coeffs}


# ------------------------------------------- MODWT wavelet variance / correlation
WCORR_MAX_N = 16384      # longest row of the fused kernel (include/wtmi.h: wtmi_modwt_wcorr)
WCORR_MAX_LAG_N = 8192   # with max_lag > 0: the coefficient rows share the workgroup's LDS
WCORR_MAX_LAG = 64
WCORR_STATS = ("var_x", "var_y", "cov", "corr", "nobs", "ci_lo", "ci_hi", "n_eff")
WCORR_BOUNDARY = {"periodic": 0, "brickwall": 1}


def _wcorr_composed(x, y, lo, hi, level, K, periodic, z):
    """The numbers of wtmi_modwt_wcorr from modwt coefficient rows and fp64 torch reductions."""
    B, n = x.shape
    L = lo.size
    nan = float("nan")
    rows = [modwt(r - r[:, :1], lo, hi, level)[:, :level].to(torch.float64) for r in ((x,) if y is None else (x, y))]
    stats = torch.full((B, level, 8), nan, dtype=torch.float64, device=x.device)
    xcorr = torch.full((B, level, 2 * K + 1), nan, dtype=torch.float64, device=x.device) if K else None
    for j in range(1, level + 1):
        t0 = 0 if periodic else min(n, ((1 << j) - 1) * (L - 1))
        M = n - t0
        if M <= 0:
            stats[:, j - 1, 4] = 0.0
            continue
        wx = rows[0][:, j - 1]
        st = stats[:, j - 1]
        st[:, 0] = (wx[:, t0:] ** 2).sum(-1) / M
        st[:, 4] = M
        neff = (n >> j) - (0 if periodic else (L - 2) - ((L - 2) >> j))
        st[:, 7] = neff
        if y is None:
            continue
        wy = rows[1][:, j - 1]
        st[:, 1] = (wy[:, t0:] ** 2).sum(-1) / M
        st[:, 2] = (wx[:, t0:] * wy[:, t0:]).sum(-1) / M
        den = torch.sqrt(st[:, 0] * st[:, 1])
        den = torch.where(den > 0, den, torch.full_like(den, nan))
        st[:, 3] = st[:, 2] / den
        if neff > 3:
            zr, hw = torch.atanh(st[:, 3]), z / float(neff - 3) ** 0.5
            st[:, 5], st[:, 6] = torch.tanh(zr - hw), torch.tanh(zr + hw)
        for lag in range(-K, K + 1) if K else ():
            if lag == 0:
                s = st[:, 3] * den * M
            elif periodic:
                s = (wx * torch.roll(wy, -lag, dims=-1)).sum(-1)
            else:
                a, b = max(t0, t0 - lag), min(n, n - lag)
                s = (wx[:, a:b] * wy[:, a + lag:b + lag]).sum(-1) if b > a else torch.zeros_like(den)
            xcorr[:, j - 1, lag + K] = st[:, 3] if lag == 0 else s / M / den
    return stats, xcorr


def modwt_wcorr(x: torch.Tensor, dec_lo, dec_hi, level: int, *, y: Optional[torch.Tensor] = None,
                max_lag: int = 0, boundary: str = "brickwall", ci_level: float = 0.95):
    """Wavelet variance, covariance and correlation per MODWT detail level of float32 rows x
    ([n] or [B, n]) and, with y, of the pairs (x, y): {"stats": [B, level, 8] float64
    (``WCORR_STATS``, row j - 1 = level j), "xcorr": [B, level, 2 max_lag + 1] float64 (column
    lag + max_lag; a peak at lag > 0: x leads y) or None with max_lag = 0}.  boundary
    "brickwall" counts only the coefficients clear of the wrap (the unbiased estimator),
    "periodic" all of them.  Without y only var_x, nobs and n_eff are numbers.  Rows of at most
    ``WCORR_MAX_N`` samples (``WCORR_MAX_LAG_N`` with lags), ``MRA_MAX_TAPS`` taps and
    ``WCORR_MAX_LAG`` lags take ONE fused launch (wtmi_modwt_wcorr); beyond, modwt rows and fp64
    torch reductions compose the same numbers."""
    from statistics import NormalDist
    what = "modwt_wcorr"
    level = _int_level(level, 1, MRA_MAX_LEVEL, what)
    lo, hi = _bank(what, dec_lo=dec_lo, dec_hi=dec_hi)
    if boundary not in WCORR_BOUNDARY:
        raise ValueError(f"{what}: boundary must be one of {sorted(WCORR_BOUNDARY)}, got {boundary!r}")
    if not 0.0 < ci_level < 1.0:
        raise ValueError(f"{what}: ci_level must lie in (0, 1), got {ci_level!r}")
    if int(max_lag) != max_lag or max_lag < 0:
        raise ValueError(f"{what}: max_lag must be an integer >= 0, got {max_lag!r}")
    K = int(max_lag)
    # the lag checks come before the operands': those end on the device
    if K and y is None:
        raise ValueError(f"{what}: max_lag needs a second series y")
    if K and isinstance(x, torch.Tensor) and x.dim() and K >= x.shape[-1]:
        raise ValueError(f"{what}: max_lag must be below the series length {x.shape[-1]}, got {K}")
    z = NormalDist().inv_cdf(0.5 + 0.5 * ci_level)
    dev, x, y = _series_or_pair(x, y, what, True)
    B, n = x.shape
    if n > (WCORR_MAX_LAG_N if K else WCORR_MAX_N) or lo.size > MRA_MAX_TAPS or K > WCORR_MAX_LAG:
        stats, xcorr = _wcorr_composed(x, y, lo, hi, level, K, boundary == "periodic", z)
        return {"stats": stats, "xcorr": xcorr}
    stats = torch.empty((B, level, 8), dtype=torch.float64, device=dev)
    xcorr = torch.empty((B, level, 2 * K + 1), dtype=torch.float64, device=dev) if K else None
    with torch.cuda.device(dev):
        _lib.call("wtmi_modwt_wcorr", _ptr(x), _ptr(y), x.stride(0), B, n, _tp(lo), _tp(hi),
                  lo.size, level, WCORR_BOUNDARY[boundary], K, C.c_double(z),
                  _ptr(stats), _ptr(xcorr), _stream(dev))
    return {"stats": stats, "xcorr": xcorr}


# ------------------------- MODWT time-localized (rolling-window) wavelet correlation
LWCORR_MAX_N = 8192           # longest row of the fused kernel (include/wtmi.h: wtmi_modwt_lwcorr)
LWCORR_MAX_HALF_WIDTH = 1024  # widest window: the rows' halos and the weights share the workgroup's LDS
LWCORR_MOMENTS = ("var_x", "var_y", "cov")
_LWCORR_BLOCK = 1024          # centres per Toeplitz product of the composed route


def _lwcorr_composed(x, y, lo, hi, level, theta, periodic):
    """The numbers of wtmi_modwt_lwcorr from modwt coefficient rows and fp64 torch windowed sums
    (products of the padded rows with one banded Toeplitz block of the weights): (corr
    [B, level, n] or None without y, moments [B, level, 3, n]) float32; without y planes 1 and 2
    of moments are NaN."""
    B, n = x.shape
    L, H, dev, nan = lo.size, theta.size - 1, x.device, float("nan")
    th = torch.as_tensor(theta, dtype=torch.float64, device=dev)
    cb = min(n, _LWCORR_BLOCK)
    k = (torch.arange(cb + 2 * H, device=dev)[:, None] - H - torch.arange(cb, device=dev)[None, :]).abs()
    toep = torch.where(k <= H, th[k.clamp_max(H)], torch.zeros((), dtype=torch.float64, device=dev))

    def windowed(q):  # [R, n] -> [R, n]: sum_k theta(k) q[s + k], zeros (or the wrap) outside
        qp = torch.cat((q[:, n - H:], q, q[:, :H]), 1) if periodic else torch.nn.functional.pad(q, (H, H))
        out = torch.empty_like(q)
        for s in range(0, n, cb):
            c = min(cb, n - s)
            out[:, s:s + c] = qp[:, s:s + c + 2 * H] @ toep[:c + 2 * H, :c]
        return out

    rows = [modwt(r - r[:, :1], lo, hi, level)[:, :level].to(torch.float64) for r in ((x,) if y is None else (x, y))]
    corr = None if y is None else torch.full((B, level, n), nan, dtype=torch.float32, device=dev)
    mom = torch.full((B, level, 3, n), nan, dtype=torch.float32, device=dev)
    for j in range(1, level + 1):
        t0 = 0 if periodic else min(n, ((1 << j) - 1) * (L - 1))
        counted = torch.ones((1, n), dtype=torch.float64, device=dev)
        counted[:, :t0] = 0.0
        sw = windowed(counted)
        wx = rows[0][:, j - 1] * counted
        axx = windowed(wx * wx)
        mom[:, j - 1, 0] = torch.where(sw > 0, axx / sw, nan)
        if y is None:
            continue
        wy = rows[1][:, j - 1] * counted
        ayy, axy = windowed(wy * wy), windowed(wx * wy)
        mom[:, j - 1, 1] = torch.where(sw > 0, ayy / sw, nan)
        mom[:, j - 1, 2] = torch.where(sw > 0, axy / sw, nan)
        ok = (sw > 0) & (axx > 0) & (ayy > 0)
        corr[:, j - 1] = torch.where(ok, (axy / torch.sqrt(axx * ayy)).clamp(-1.0, 1.0), nan)
    return corr, mom


def _lwcorr_window(window, what):
    """The weights theta(0 .. H) as contiguous float64 (host): 1-D, finite, >= 0, theta(0) > 0."""
    if isinstance(window, torch.Tensor):
        window = window.detach().cpu().numpy()
    th = np.ascontiguousarray(np.asarray(window, dtype=np.float64))
    if th.ndim != 1 or th.size < 1:
        raise ValueError(f"{what}: window must hold the half_width + 1 weights theta(0 .. H), got shape {th.shape}")
    if not np.isfinite(th).all() or (th < 0).any():
        raise ValueError(f"{what}: window weights must be finite and >= 0")
    if not th[0] > 0:
        raise ValueError(f"{what}: the centre weight window[0] must be > 0, got {th[0]!r}")
    return th


def modwt_lwcorr(x: torch.Tensor, dec_lo, dec_hi, level: int, *, y: Optional[torch.Tensor] = None,
                 window, boundary: str = "brickwall", moments: bool = False):
    """Time-localized (rolling-window) wavelet variance, covariance and correlation per MODWT
    detail level of float32 rows x ([n] or [B, n]) and, with y, of the pairs (x, y).  window: the
    H + 1 weights theta(0 .. H) >= 0 of a symmetric window, theta(0) > 0.  For every centre s the
    counted coefficients C(s) are t in [max(t0, s - H), min(n - 1, s + H)] (boundary "brickwall":
    t0 = (2^j - 1)(taps - 1) as ``modwt_wcorr``; the window is cut, it never wraps) or (s + k) mod n
    for |k| <= H ("periodic"; needs 2 H + 1 <= n).  With Sw = sum_C theta and A^ab = sum_C theta
    W^a_j W^b_j in fp64: {"corr": [B, level, n] float32 = A^xy / sqrt(A^xx A^yy) clamped to
    [-1, 1] (None without y), "moments": [B, level, 3, n] float32 (``LWCORR_MOMENTS``: A^xx / Sw,
    A^yy / Sw, A^xy / Sw; None unless moments=True; without y planes 1 and 2 are NaN)}; row
    j - 1 = level j.  NaN: Sw = 0 (no counted coefficient in the window: all four), A^xx = 0 or
    A^yy = 0 (corr).  Rows of at most ``LWCORR_MAX_N`` samples, ``MRA_MAX_TAPS`` taps and windows
    of half width at most ``LWCORR_MAX_HALF_WIDTH`` take ONE fused launch (wtmi_modwt_lwcorr);
    beyond, modwt rows and fp64 torch windowed sums compose the same numbers."""
    what = "modwt_lwcorr"
    level = _int_level(level, 1, MRA_MAX_LEVEL, what)
    lo, hi = _bank(what, dec_lo=dec_lo, dec_hi=dec_hi)
    if boundary not in WCORR_BOUNDARY:
        raise ValueError(f"{what}: boundary must be one of {sorted(WCORR_BOUNDARY)}, got {boundary!r}")
    th = _lwcorr_window(window, what)
    H = th.size - 1
    # the window checks come before the operands': those end on the device
    if boundary == "periodic" and isinstance(x, torch.Tensor) and x.dim() and 2 * H + 1 > x.shape[-1]:
        raise ValueError(f"{what}: a periodic window of half width {H} needs 2 * {H} + 1 <= n = {x.shape[-1]} "
                         "(no coefficient may count twice)")
    dev, x, y = _series_or_pair(x, y, what, bool(moments))
    B, n = x.shape
    if n > LWCORR_MAX_N or lo.size > MRA_MAX_TAPS or H > LWCORR_MAX_HALF_WIDTH:
        corr, mom = _lwcorr_composed(x, y, lo, hi, level, th, boundary == "periodic")
        return {"corr": corr, "moments": mom if moments else None}
    corr = None if y is None else torch.empty((B, level, n), dtype=torch.float32, device=dev)
    mom = None
    if moments:  # a single series fills plane 0 only
        mom = torch.empty((B, level, 3, n), dtype=torch.float32, device=dev)
        if y is None:
            mom.fill_(float("nan"))
    with torch.cuda.device(dev):
        _lib.call("wtmi_modwt_lwcorr", _ptr(x), _ptr(y), x.stride(0), B, n, _tp(lo), _tp(hi), lo.size, level,
                  WCORR_BOUNDARY[boundary], _ptr(_f64_dev(th, dev)), H, _ptr(corr), _ptr(mom), n, _stream(dev))
    return {"corr": corr, "moments": mom}


# ------------------------- MODWT wavelet correlation matrix / multiple correlation
WCMAT_MAX_SERIES = 16      # series per group of the fused kernel (include/wtmi.h: wtmi_modwt_wcmat)
WCMAT_MAX_SAMPLES = 32768   # series x samples of a group: its smooth rows fill the workgroup's LDS
WCMAT_STATS = ("wmc", "target", "ci_lo", "ci_hi", "nobs", "n_eff")


def _wcmat_composed(x, lo, hi, level, periodic, z):
    """The numbers of wtmi_modwt_wcmat from modwt coefficient rows, fp64 torch Gram products and
    torch.linalg: (cov, corr [B, level, M, M], r2 [B, level, M], stats [B, level, 6])."""
    B, M, n = x.shape
    L = lo.size
    nan = float("nan")
    dev = x.device
    rows = modwt((x - x[..., :1]).reshape(B * M, n), lo, hi, level)[:, :level].to(torch.float64)
    rows = rows.reshape(B, M, level, n)
    cov = torch.full((B, level, M, M), nan, dtype=torch.float64, device=dev)
    corr, r2 = cov.clone(), cov[..., 0].clone()
    stats = torch.full((B, level, 6), nan, dtype=torch.float64, device=dev)
    eye = torch.eye(M, dtype=torch.float64, device=dev)
    for j in range(1, level + 1):
        t0 = 0 if periodic else min(n, ((1 << j) - 1) * (L - 1))
        Mj = n - t0
        stats[:, j - 1, 4] = max(Mj, 0)
        if Mj <= 0:
            continue
        w = rows[:, :, j - 1, t0:]
        c = w @ w.transpose(-1, -2) / Mj
        c = torch.triu(c) + torch.triu(c, 1).transpose(-1, -2)  # symmetric bit for bit
        var = torch.diagonal(c, dim1=-2, dim2=-1)
        p = c / torch.sqrt(var.unsqueeze(-1) * var.unsqueeze(-2))
        p = torch.where(eye.bool(), torch.where(var > 0, 1.0, nan).unsqueeze(-1).expand_as(p), p)
        cov[:, j - 1], corr[:, j - 1] = c, p
        neff = (n >> j) - (0 if periodic else (L - 2) - ((L - 2) >> j))
        stats[:, j - 1, 5] = neff
        ok = (var > 0).all(-1)
        if Mj < M or not bool(ok.any()):
            continue
        fac, info = torch.linalg.cholesky_ex(torch.where(ok[:, None, None], p, eye))
        ok = ok & (info == 0)
        inv = torch.linalg.solve_triangular(torch.where(ok[:, None, None], fac, eye), eye.expand(B, M, M), upper=False)
        r = torch.where(ok[:, None], 1.0 - 1.0 / (inv ** 2).sum(-2), nan)
        r2[:, j - 1] = r
        best, tgt = torch.nan_to_num(r, nan=-1.0).max(-1)
        wmc = torch.where(ok, torch.sqrt(best.clamp_min(0.0)), nan)
        stats[:, j - 1, 0], stats[:, j - 1, 1] = wmc, torch.where(ok, tgt.to(torch.float64), nan)
        if neff > 3:
            zr, hw = torch.atanh(wmc), z / float(neff - 3) ** 0.5
            stats[:, j - 1, 2], stats[:, j - 1, 3] = torch.tanh(zr - hw), torch.tanh(zr + hw)
    return cov, corr, r2, stats


def modwt_wcmat(x: torch.Tensor, dec_lo, dec_hi, level: int, *, boundary: str = "brickwall",
                ci_level: float = 0.95, want_corr: bool = True, want_multiple: bool = True):
    """Wavelet covariance / correlation matrices and the wavelet multiple correlation
    (Fernandez-Macho 2012) per MODWT detail level of groups of M float32 series x [B, M, n] (or
    [M, n]): {"cov", "corr": [B, level, M, M] float64, "r2": [B, level, M] (R^2 of series i on the
    others, 1 - 1 / (P^-1)_ii), "stats": [B, level, 6] (``WCMAT_STATS``: wmc = sqrt(max_i R^2_i),
    target = the maximising series, the Fisher interval of wmc, nobs, n_eff)}; row j - 1 = level
    j; entries not requested are None.  boundary and ci_level as ``modwt_wcorr``.  NaN rows: a
    level without coefficients (nobs 0); a series without variance (its corr row and column, the
    level's r2 / wmc / target / ci); fewer coefficients than series or a correlation matrix that
    is not positive definite (r2 / wmc / target / ci); n_eff <= 3 (ci).  Groups of at most
    ``WCMAT_MAX_SERIES`` series, ``WCMAT_MAX_SAMPLES`` series x samples and ``MRA_MAX_TAPS`` taps
    take ONE fused launch (wtmi_modwt_wcmat); beyond, modwt rows, fp64 torch Gram products and
    torch.linalg compose the same numbers."""
    from statistics import NormalDist
    what = "modwt_wcmat"
    level = _int_level(level, 1, MRA_MAX_LEVEL, what)
    lo, hi = _bank(what, dec_lo=dec_lo, dec_hi=dec_hi)
    if boundary not in WCORR_BOUNDARY:
        raise ValueError(f"{what}: boundary must be one of {sorted(WCORR_BOUNDARY)}, got {boundary!r}")
    if not 0.0 < ci_level < 1.0:
        raise ValueError(f"{what}: ci_level must lie in (0, 1), got {ci_level!r}")
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() not in (2, 3) \
            or x.shape[-2] < 2 or x.shape[-1] < 1:
        raise ValueError(f"{what}: x must be float32 [series >= 2, n] or [batch, series >= 2, n] rows")
    z = NormalDist().inv_cdf(0.5 + 0.5 * ci_level)
    dev = _check_dev(x)
    if x.dim() == 2:
        x = x.unsqueeze(0)
    B, M, n = x.shape
    if x.stride(2) != 1 or x.stride(1) < n or (B > 1 and x.stride(0) != M * x.stride(1)):
        x = x.contiguous()  # the C ABI's layout: [batch][series][ld]
    if M > WCMAT_MAX_SERIES or M * n > WCMAT_MAX_SAMPLES or lo.size > MRA_MAX_TAPS:
        cov, corr, r2, stats = _wcmat_composed(x, lo, hi, level, boundary == "periodic", z)
    else:
        cov = torch.empty((B, level, M, M), dtype=torch.float64, device=dev)
        corr = torch.empty_like(cov) if want_corr else None
        r2 = torch.empty((B, level, M), dtype=torch.float64, device=dev) if want_multiple else None
        stats = torch.empty((B, level, 6), dtype=torch.float64, device=dev) if want_multiple else None
        with torch.cuda.device(dev):
            _lib.call("wtmi_modwt_wcmat", _ptr(x), x.stride(1), B, M, n, _tp(lo), _tp(hi), lo.size, level,
                      WCORR_BOUNDARY[boundary], C.c_double(z), _ptr(cov), _ptr(corr), _ptr(r2),
                      _ptr(stats), _stream(dev))
    return {"cov": cov, "corr": corr if want_corr else None, "r2": r2 if want_multiple else None,
            "stats": stats if want_multiple else None}


# ------------------------------------------------------------ torch custom ops
# torch.ops.wtmi.* wrappers over the same HIP kernels (CUDA/ROCm dispatch only: a
# CPU tensor has no kernel and raises).  Filter taps travel as host float64 tensors.
def _register():
    lib = torch.library

    def _batch(x, nd=2):
        return x.shape[0] if x.dim() == nd else 1

    @lib.custom_op("wtmi::cwt", mutates_args=())
    def _cwt(x: torch.Tensor, scales: torch.Tensor, dt: float, f0: float) -> torch.Tensor:
        return cwt_morlet(x, scales, dt, f0)["w"]

    @_cwt.register_fake
    def _(x, scales, dt, f0):
        return x.new_empty((_batch(x), scales.numel(), x.shape[-1]),
                           dtype=torch.complex64)

    @lib.custom_op("wtmi::cwt_power", mutates_args=())
    def _cwt_power(x: torch.Tensor, scales: torch.Tensor, dt: float, f0: float) -> torch.Tensor:
        return cwt_morlet(x, scales, dt, f0, want_w=False, want_power=True)["power"]

    @_cwt_power.register_fake
    def _(x, scales, dt, f0):
        return x.new_empty((_batch(x), scales.numel(), x.shape[-1]),
                           dtype=torch.float32)

    @lib.custom_op("wtmi::cwt_summary", mutates_args=())
    def _cwt_summary(x: torch.Tensor, scales: torch.Tensor, dt: float, f0: float, power_weights: torch.Tensor,
                     signal_weights: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Global spectrum [B, S], band power and band signal [B, K, n0] of Morlet(f0) transforms."""
        r = cwt_summary(x, scales, dt, f0, power_weights=power_weights, signal_weights=signal_weights)
        return r["global_power"], r["band_power"], r["band_signal"]

    @_cwt_summary.register_fake
    def _(x, scales, dt, f0, power_weights, signal_weights):
        B, K, n = _batch(x), power_weights.shape[0], x.shape[-1]
        return (x.new_empty((B, scales.numel()), dtype=torch.float32),
                x.new_empty((B, K, n), dtype=torch.float32), x.new_empty((B, K, n), dtype=torch.float32))

    @lib.custom_op("wtmi::wct", mutates_args=())
    def _wct(x1: torch.Tensor, x2: torch.Tensor, scales: torch.Tensor, dt: float, f0: float,
             boxcar: int) -> torch.Tensor:
        return wct_morlet(x1, x2, scales, dt, f0, boxcar=boxcar, want_uv=False)["coh"]

    @_wct.register_fake
    def _(x1, x2, scales, dt, f0, boxcar):
        return x1.new_empty((_batch(x1), scales.numel(), x1.shape[-1]),
                            dtype=torch.float32)

    @lib.custom_op("wtmi::modwt", mutates_args=())
    def _modwt(x: torch.Tensor, dec_lo: torch.Tensor, dec_hi: torch.Tensor, level: int
               ) -> torch.Tensor:
        return modwt(x, dec_lo.cpu().numpy(), dec_hi.cpu().numpy(), level)

    @_modwt.register_fake
    def _(x, dec_lo, dec_hi, level):
        return x.new_empty((_batch(x), level + 1, x.shape[-1]),
                           dtype=torch.float32)

    @lib.custom_op("wtmi::imodwt", mutates_args=())
    def _imodwt(w: torch.Tensor, dec_lo: torch.Tensor, dec_hi: torch.Tensor) -> torch.Tensor:
        return imodwt(w, dec_lo.cpu().numpy(), dec_hi.cpu().numpy())

    @_imodwt.register_fake
    def _(w, dec_lo, dec_hi):
        return w.new_empty((_batch(w, 3), w.shape[-1]), dtype=torch.float32)

    def _bs(x, scales, dtype):
        return x.new_empty((_batch(x), scales.numel(), x.shape[-1]),
                           dtype=dtype)

    @lib.custom_op("wtmi::xwt", mutates_args=())
    def _xwt(x1: torch.Tensor, x2: torch.Tensor, scales: torch.Tensor, dt: float, f0: float
             ) -> torch.Tensor:
        """W1 W2* (complex64) of row pairs (pycwt.xwt before normalisation)."""
        return xwt_morlet(x1, x2, scales, dt, f0, want_w12=True)["w12"]

    @_xwt.register_fake
    def _(x1, x2, scales, dt, f0):
        return _bs(x1, scales, torch.complex64)

    @lib.custom_op("wtmi::xwt_power", mutates_args=())
    def _xwt_power(x1: torch.Tensor, x2: torch.Tensor, scales: torch.Tensor, dt: float, f0: float
                   ) -> torch.Tensor:
        return xwt_morlet(x1, x2, scales, dt, f0, want_power=True)["power"]

    @_xwt_power.register_fake
    def _(x1, x2, scales, dt, f0):
        return _bs(x1, scales, torch.float32)

    @lib.custom_op("wtmi::dwt", mutates_args=())
    def _dwt(x: torch.Tensor, dec_lo: torch.Tensor, dec_hi: torch.Tensor, level: int
             ) -> torch.Tensor:
        """pywt.wavedec (mode symmetric), coefficient lists back-to-back: [B, total]."""
        return wavedec(x, dec_lo.cpu().numpy(), dec_hi.cpu().numpy(), level)[0]

    @_dwt.register_fake
    def _(x, dec_lo, dec_hi, level):
        total = sum(dwt_lengths(x.shape[-1], dec_lo.numel(), level))
        return x.new_empty((_batch(x), total), dtype=torch.float32)

    @lib.custom_op("wtmi::idwt", mutates_args=())
    def _idwt(coeffs: torch.Tensor, n: int, rec_lo: torch.Tensor, rec_hi: torch.Tensor,
              level: int) -> torch.Tensor:
        """pywt.waverec of back-to-back coefficient lists: [B, out_len]."""
        full = (1 << (level + 1)) - 1
        return waverec(coeffs, n, rec_lo.cpu().numpy(), rec_hi.cpu().numpy(), level, [full])[:, 0]

    @_idwt.register_fake
    def _(coeffs, n, rec_lo, rec_hi, level):
        lens = dwt_lengths(n, rec_lo.numel(), level)
        out_len = 2 * lens[-1] - rec_lo.numel() + 2 if level > 0 else n
        return coeffs.new_empty((_batch(coeffs), out_len),
                                dtype=torch.float32)

    @lib.custom_op("wtmi::dwt_tsr", mutates_args=())
    def _dwt_tsr(x: torch.Tensor, y: torch.Tensor, dec_lo: torch.Tensor, dec_hi: torch.Tensor,
                 rec_lo: torch.Tensor, rec_hi: torch.Tensor, level: int, add_constant: bool
                 ) -> torch.Tensor:
        """Per-component OLS statistics of y on x over their DWT components: [B, level + 1, 8]."""
        banks = [t.cpu().numpy() for t in (dec_lo, dec_hi, rec_lo, rec_hi)]
        return dwt_time_scale_regression(x, y, *banks, level, add_constant=add_constant)["stats"]

    @_dwt_tsr.register_fake
    def _(x, y, dec_lo, dec_hi, rec_lo, rec_hi, level, add_constant):
        return x.new_empty((_batch(x), level + 1, 8), dtype=torch.float64)

    @lib.custom_op("wtmi::rows_ols", mutates_args=())
    def _rows_ols(x: torch.Tensor, y: torch.Tensor, add_constant: bool) -> torch.Tensor:
        return rows_ols(x, y, add_constant)

    @_rows_ols.register_fake
    def _(x, y, add_constant):
        return x.new_empty((_batch(x), 8), dtype=torch.float64)

    @lib.custom_op("wtmi::dwt_smooth", mutates_args=())
    def _dwt_smooth(x: torch.Tensor, dec_lo: torch.Tensor, rec_lo: torch.Tensor, level: int
                    ) -> torch.Tensor:
        """The smooths with cD_1 .. cD_l zeroed, l = 1 .. level: [B, level, n]."""
        return dwt_smooth(x, dec_lo.cpu().numpy(), rec_lo.cpu().numpy(), level)["smooth"]

    @_dwt_smooth.register_fake
    def _(x, dec_lo, rec_lo, level):
        return x.new_empty((_batch(x), level, x.shape[-1]), dtype=torch.float32)

    @lib.custom_op("wtmi::dwt_denoise", mutates_args=())
    def _dwt_denoise(x: torch.Tensor, dec_lo: torch.Tensor, dec_hi: torch.Tensor, rec_lo: torch.Tensor,
                     rec_hi: torch.Tensor, level: int, rule: str, shrink: str, mult: float) -> torch.Tensor:
        """Wavelet shrinkage with a MAD threshold (rule "universal" or "level"): [B, n]."""
        banks = [t.cpu().numpy() for t in (dec_lo, dec_hi, rec_lo, rec_hi)]
        return dwt_denoise(x, *banks, level, rule=rule, shrink=shrink, mult=mult, want_info=False)["denoised"]

    @_dwt_denoise.register_fake
    def _(x, dec_lo, dec_hi, rec_lo, rec_hi, level, rule, shrink, mult):
        return x.new_empty((_batch(x), x.shape[-1]), dtype=torch.float32)

    @lib.custom_op("wtmi::modwt_mra", mutates_args=())
    def _modwt_mra(x: torch.Tensor, dec_lo: torch.Tensor, dec_hi: torch.Tensor, level: int
                   ) -> torch.Tensor:
        """MRA rows [D_1 .. D_J, S_J] of every series: [B, level + 1, n]."""
        return modwt_mra(x, dec_lo.cpu().numpy(), dec_hi.cpu().numpy(), level)["components"][:, 0]

    @_modwt_mra.register_fake
    def _(x, dec_lo, dec_hi, level):
        return x.new_empty((_batch(x), level + 1, x.shape[-1]),
                           dtype=torch.float32)

    @lib.custom_op("wtmi::modwt_mra_rows", mutates_args=())
    def _modwt_mra_rows(w: torch.Tensor, dec_lo: torch.Tensor, dec_hi: torch.Tensor) -> torch.Tensor:
        return modwt_mra_rows(w, dec_lo.cpu().numpy(), dec_hi.cpu().numpy())

    @_modwt_mra_rows.register_fake
    def _(w, dec_lo, dec_hi):
        return w.new_empty((_batch(w, 3), w.shape[-2], w.shape[-1]),
                           dtype=torch.float32)

    @lib.custom_op("wtmi::modwt_wcorr", mutates_args=())
    def _modwt_wcorr(x: torch.Tensor, y: torch.Tensor, dec_lo: torch.Tensor, dec_hi: torch.Tensor,
                     level: int, periodic: bool) -> torch.Tensor:
        """Wavelet variance / covariance / correlation rows (``WCORR_STATS``): [B, level, 8]."""
        return modwt_wcorr(x, dec_lo.cpu().numpy(), dec_hi.cpu().numpy(), level, y=y,
                           boundary="periodic" if periodic else "brickwall")["stats"]

    @_modwt_wcorr.register_fake
    def _(x, y, dec_lo, dec_hi, level, periodic):
        return x.new_empty((_batch(x), level, 8), dtype=torch.float64)

    @lib.custom_op("wtmi::modwt_lwcorr", mutates_args=())
    def _modwt_lwcorr(x: torch.Tensor, y: torch.Tensor, dec_lo: torch.Tensor, dec_hi: torch.Tensor,
                      window: torch.Tensor, level: int, periodic: bool) -> tuple[torch.Tensor, torch.Tensor]:
        """Rolling-window wavelet correlation [B, level, n] and local variances / covariance
        (``LWCORR_MOMENTS``) [B, level, 3, n] of row pairs; window: the weights theta(0 .. H)."""
        r = modwt_lwcorr(x, dec_lo.cpu().numpy(), dec_hi.cpu().numpy(), level, y=y, window=window, moments=True,
                         boundary="periodic" if periodic else "brickwall")
        return r["corr"], r["moments"]

    @_modwt_lwcorr.register_fake
    def _(x, y, dec_lo, dec_hi, window, level, periodic):
        B, n = _batch(x), x.shape[-1]
        return (x.new_empty((B, level, n), dtype=torch.float32), x.new_empty((B, level, 3, n), dtype=torch.float32))

    @lib.custom_op("wtmi::modwt_wcmat", mutates_args=())
    def _modwt_wcmat(x: torch.Tensor, dec_lo: torch.Tensor, dec_hi: torch.Tensor, level: int, periodic: bool
                     ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """Wavelet covariance and correlation matrices [B, level, M, M], R^2 [B, level, M] and the
        multiple-correlation rows (``WCMAT_STATS``) [B, level, 6] of groups x [B, M, n]."""
        r = modwt_wcmat(x, dec_lo.cpu().numpy(), dec_hi.cpu().numpy(), level,
                        boundary="periodic" if periodic else "brickwall")
        return r["cov"], r["corr"], r["r2"], r["stats"]

    @_modwt_wcmat.register_fake
    def _(x, dec_lo, dec_hi, level, periodic):
        B, M = _batch(x, 3), x.shape[-2]
        return (x.new_empty((B, level, M, M), dtype=torch.float64), x.new_empty((B, level, M, M), dtype=torch.float64),
                x.new_empty((B, level, M), dtype=torch.float64), x.new_empty((B, level, 6), dtype=torch.float64))

    @lib.custom_op("wtmi::series_stats", mutates_args=())
    def _series_stats(x: torch.Tensor) -> torch.Tensor:
        """[B, 8] float64: mean, std, detrend slope, intercept, lag-0 / lag-1 covariance, n, 0."""
        return series_moments(x)

    @_series_stats.register_fake
    def _(x):
        return x.new_empty((_batch(x), 8), dtype=torch.float64)


try:
    torch.ops.wtmi.cwt  # already registered (module reloaded)
except (AttributeError, RuntimeError):
    _register()
