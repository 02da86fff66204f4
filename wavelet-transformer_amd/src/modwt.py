"""Maximal-overlap DWT (reference: src/modwt.py:56-285).

``modwt`` / ``imodwt`` run the a-trous cascades on the GPU (``wtmi_modwt`` /
``wtmi_imodwt``: one workgroup per series, all J levels LDS-resident, only the L
non-zero taps per level).  ``modwtmra`` and ``smooth_signal`` are masked inverse
transforms (row j of the MRA = inverse of the isolated row j, probe C.8b).
Row order is the reference's ``[W_1 .. W_J, V_J]``; output dtype follows the input
dtype (float32 in -> float32 out, quirk B.11).

The reference module also exports its single-level helpers (``upArrow_op``,
``period_list``, ``circular_convolve_{d,s,mra}``), the per-component OLS
``time_scale_regression`` and ``plot_smoothing``.  They are re-provided with the same
signatures and results for code that imports them; none of them is on the transform
path (the GPU cascades never call them).  The circular convolutions are written as
periodic index sums (Percival & Walden's form) on the host.
"""

from __future__ import annotations

import numpy as np
import numpy.typing as npt

from wtmi import transforms
from wtmi.wavelets import Wavelet

MOTHER = Wavelet("db4")


def modwt(x, filters, level):
    """filters: 'db1', 'db2', 'haar', ... (or a filter-bank object); returns [level+1, N]."""
    return transforms.modwt(x, filters, level)


def imodwt(w, filters):
    """Inverse MODWT of rows [W_1 .. W_J, V_J]."""
    return transforms.imodwt(w, filters)


def modwtmra(w, filters):
    """Multiresolution analysis [D_1 .. D_J, S_J]."""
    w = np.asarray(w)
    return np.vstack([transforms.imodwt(w, filters, keep_mask=1 << j) for j in range(w.shape[0])])


def smooth_signal(modwt_coeffs: npt.NDArray, mother_wavelet: str, levels: int
                  ) -> dict[int, dict[str, npt.NDArray]]:
    """signal_dict[l]: inverse with detail rows 0..l-1 zeroed (src/modwt.py:232-251)."""
    signals_dict = {}
    c = np.asarray(modwt_coeffs)
    full = (1 << c.shape[0]) - 1
    for lvl in range(levels, 0, -1):
        print(f"s_{lvl} stored with key {lvl}")
        smooth_coeffs = c.copy()
        smooth_coeffs[:lvl] = 0
        keep = full & ~((1 << lvl) - 1)
        signals_dict[lvl] = {"coeffs": smooth_coeffs,
                             "signal": transforms.imodwt(c, mother_wavelet, keep_mask=keep)}
    return signals_dict


# --------------------------------------------------- the reference's host-side helpers
def upArrow_op(li, j):
    """Filter ``li`` upsampled for level j: 2**(j-1) - 1 zeros between taps; [1] at j = 0
    (src/modwt.py:56-63)."""
    if j == 0:
        return [1]
    step = 2 ** (j - 1)
    out = np.zeros(step * (len(li) - 1) + 1)
    out[::step] = li
    return out


def period_list(li, N):
    """Periodise a filter to length N by summing its N-blocks (src/modwt.py:66-78).  A
    filter shorter than N comes back zero-padded to N (as a plain array)."""
    li = list(li)
    padded = np.array(li + [0] * (N - len(li) % N))
    if padded.size < 2 * N:
        return padded
    return padded.reshape(-1, N).sum(axis=0)


def _taps(h, d, n, sign):
    """Periodic gather positions (t + sign * d * l) mod n for every tap l."""
    t = np.arange(n)[None, :]
    return (t + sign * d * np.arange(len(h))[:, None]) % n


def circular_convolve_mra(h_j_o, w_j):
    """D_j[t] = sum_k h_j_o[k] w_j[(t + k) mod N] (src/modwt.py:81-83)."""
    h = np.asarray(h_j_o, dtype=np.float64)
    w = np.asarray(w_j)
    out = np.einsum("k,kt->t", h, w[_taps(h, 1, w.size, +1)])
    return out.astype(w.dtype) if w.dtype in (np.float32, np.float64) else out


def circular_convolve_d(h_t, v_j_1, j):
    """Level-j analysis: w_j[t] = sum_l h_t[l] v_{j-1}[(t - 2**(j-1) l) mod N]
    (src/modwt.py:86-102)."""
    h = np.asarray(h_t, dtype=np.float64)
    v = np.asarray(v_j_1)
    out = np.einsum("l,lt->t", h, v[_taps(h, 2 ** (j - 1), v.size, -1)])
    return out.astype(v.dtype) if v.dtype in (np.float32, np.float64) else out


def circular_convolve_s(h_t, g_t, w_j, v_j, j):
    """Level-j synthesis: v_{j-1}[t] = sum_l h_t[l] w_j[(t + 2**(j-1) l) mod N]
    + g_t[l] v_j[(t + 2**(j-1) l) mod N] (src/modwt.py:105-123)."""
    h = np.asarray(h_t, dtype=np.float64)
    g = np.asarray(g_t, dtype=np.float64)
    w, v = np.asarray(w_j), np.asarray(v_j)
    idx = _taps(h, 2 ** (j - 1), v.size, +1)
    out = np.einsum("l,lt->t", h, w[idx]) + np.einsum("l,lt->t", g, v[idx])
    return out.astype(v.dtype) if v.dtype in (np.float32, np.float64) else out


def time_scale_regression(input_coeffs: npt.NDArray, output_coeffs: npt.NDArray, levels: int,
                          add_constant: bool = True):
    """OLS of output on input for each component S_J, D_J, ..., D_1, summarised side by
    side (src/modwt.py:197-229).  Needs statsmodels, as the reference does."""
    import statsmodels.api as sm
    from statsmodels.iolib.summary2 import summary_col
    fits = {}
    for j in range(levels + 1):
        name = f"S_{levels}" if j == 0 else f"D_{levels - j + 1}"
        print(f"Regressing on component vector {name}")
        x = sm.add_constant(input_coeffs[j]) if add_constant else input_coeffs[j]
        fits[name] = sm.OLS(output_coeffs[j], x).fit()
    return summary_col(list(fits.values()), stars=True, model_names=list(fits))


def time_scale_regression_batch(input_rows: npt.NDArray, output_rows: npt.NDArray,
                                add_constant: bool = True):
    """The fits of ``time_scale_regression`` without statsmodels (engine extension): OLS of
    output row j on input row j for [levels + 1, N] component rows in the order the reference
    regresses them (row 0 named S_J, then D_J .. D_1), moments and solve in one GPU launch
    (``wtmi_rows_ols``).  [P, levels + 1, N] stacks of pairs give a list of P results."""
    import torch
    x, y = np.asarray(input_rows), np.asarray(output_rows)
    if x.shape != y.shape or x.ndim not in (2, 3):
        raise ValueError(f"expected equal [levels + 1, N] or [P, levels + 1, N] rows, got {x.shape} "
                         f"and {y.shape}")
    dev = transforms.device()
    xd = torch.as_tensor(x.reshape(-1, x.shape[-1]), device=dev).to(torch.float32)
    yd = torch.as_tensor(y.reshape(-1, y.shape[-1]), device=dev).to(torch.float32)
    stats = transforms.ops.rows_ols(xd, yd, add_constant).cpu().numpy().reshape(-1, x.shape[-2], 8)
    fits = [transforms.TimeScaleOLS.from_stats(s, add_constant) for s in stats]
    return fits[0] if x.ndim == 2 else fits


def mra(x, filters, level, smooths=False):
    """modwtmra(modwt(x, filters, level), filters) without the coefficient array, one fused
    launch (``wtmi_modwt_mra``): rows [D_1 .. D_J, S_J] of a series [N] or of a batch [B, N].
    smooths=True returns (rows, smooths), smooths[.., l - 1, :] = smooth_signal(...)[l]["signal"].
    Output dtype follows the input, as ``modwt``."""
    return transforms.modwt_mra(x, filters, level, smooths=smooths)


def modwtmra_batch(w, filters):
    """``modwtmra`` of coefficient rows [W_1 .. W_J, V_J] that already exist (e.g. thresholded),
    [J + 1, N] or [B, J + 1, N], in one launch (``wtmi_modwt_mra_rows``)."""
    return transforms.modwt_mra_rows(w, filters)


def time_scale_regression_series(input_series, output_series, levels: int, filters=MOTHER,
                                 add_constant: bool = True):
    """The fits of the MODWT workflow (modwt, modwtmra and ``time_scale_regression`` of an input
    and an output series) from the series themselves in one fused launch: a
    ``TimeScaleOLS`` ([B, N] inputs: a list) with rows named D_1 .. D_J, S_J."""
    return transforms.modwt_time_scale_regression(input_series, output_series, levels, filters,
                                                  add_constant)


def wavelet_correlation_series(input_series, output_series, levels: int, filters=MOTHER, max_lag: int = 0):
    """How strongly, and with what lead or lag, two series co-move at each MODWT scale (engine
    extension; the by-scale form of the correlation table): wavelet variance, covariance,
    correlation with its 95 % interval and the cross-correlation at lags -max_lag .. max_lag of
    the brick-wall coefficients, from the series themselves in one fused launch
    (``wtmi_modwt_wcorr``): a ``WaveletCorrelation`` ([B, N] inputs: a list), levels D_1 .. D_J."""
    return transforms.wavelet_correlation(input_series, output_series, levels, filters, max_lag=max_lag)


def local_wavelet_correlation_series(input_series, output_series, levels: int, half_width: int, filters=MOTHER,
                                     window="uniform"):
    """When the co-movement of two series at each MODWT scale changed (engine extension; the
    rolling form of ``wavelet_correlation_series``): the wavelet correlation, variances and
    covariance of the brick-wall coefficients under a window of 2 half_width + 1 samples ("uniform",
    "bartlett", "gaussian" or explicit weights) centred at every sample, with the 95 % interval,
    from the series themselves in one fused launch (``wtmi_modwt_lwcorr``): a
    ``LocalWaveletCorrelation`` ([B, N] inputs: a list), levels D_1 .. D_J."""
    return transforms.local_wavelet_correlation(input_series, output_series, levels, filters, half_width,
                                                window=window)


def wavelet_correlation_matrix_series(series_list, levels: int, filters=MOTHER):
    """How M series co-move at each MODWT scale (engine extension; the by-scale form of the
    correlation table for all series at once): the wavelet covariance and correlation matrices of
    the brick-wall coefficients and the wavelet multiple correlation with its 95 % interval, from
    the series themselves in one fused launch (``wtmi_modwt_wcmat``): a
    ``WaveletCorrelationMatrix`` ([B, M, N] input: a list), levels D_1 .. D_J."""
    return transforms.wavelet_correlation_matrix(series_list, levels, filters)


def denoise_signal_series(series_list, levels: int, filters=MOTHER, rule: str = "universal", shrink: str = "soft",
                          mult: float = 1.0):
    """Translation-invariant wavelet shrinkage of many series (engine extension; the MODWT
    counterpart of ``src.dwt.denoise_signal_batch``): per entry {"signal": the denoised series,
    "sigma", "threshold", "kept": one value per detail level 1 .. levels}.  rule "universal" or
    "level", shrink "soft", "hard" or "garrote", as ``wtmi.transforms.modwt_denoise``.  Series of
    one length share ONE fused launch (``wtmi_modwt_denoise``)."""
    out: list = [None] * len(series_list)
    groups: dict = {}
    for i, s in enumerate(series_list):
        groups.setdefault(len(s), []).append(i)
    for idx in groups.values():
        rows = np.stack([np.asarray(series_list[i], dtype=np.float64) for i in idx])
        sig, info = transforms.modwt_denoise(rows, filters, levels, rule, shrink, mult, return_info=True)
        for k, s, t in zip(idx, sig, info):
            out[k] = {"signal": s, "sigma": t[:, 0], "threshold": t[:, 1], "kept": t[:, 2].astype(np.int64)}
    return out


def plot_smoothing(smooth_signals: dict, original_t: npt.NDArray, original_y: npt.NDArray,
                   ascending: bool = False, **kwargs):
    """One panel per smoothed signal over the original (src/modwt.py:254-283)."""
    from src.dwt import plot_smoothing as _dwt_plot_smoothing
    return _dwt_plot_smoothing(smooth_signals, original_t, original_y, ascending=ascending,
                               **kwargs)
