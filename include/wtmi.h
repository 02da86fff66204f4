/*
 * wtmi.h -- C ABI of the MI355X wavelet-transform engine (libwtmi.so).
 *
 * Drop-in boundary for the numerics behind the reference's src.cwt / src.xwt /
 * src.wct / src.dwt / src.modwt modules.  The reference is pure Python; each entry
 * point below replaces a third-party call made from those modules (file:line into
 * the reference tree).  The Python host layer binds these with ctypes
 * (wavelet-transformer_amd/wtmi/_lib.py).
 *
 * Conventions (all entry points):
 *   - every array pointer is a DEVICE pointer (hipMalloc / torch CUDA tensor memory)
 *     owned by the caller; row-major, series-major batches; ld = elements between
 *     consecutive series (>= n);
 *   - complex outputs are interleaved float32 pairs (re, im);
 *   - work is enqueued on `stream` (a hipStream_t; NULL = default stream) and the
 *     call returns without synchronising; no allocation happens inside a call, so
 *     calls can be captured into a hipGraph;
 *   - return value: 0 success, -1 invalid argument, -2 unsupported size,
 *     > 0 a hipError_t from the kernel launch;
 *   - an empty batch (batch == 0, or no samples / scales where a size may be 0) is a
 *     no-op returning 0 once the sizes are valid, and its array pointers may then be NULL
 *     (an empty torch tensor has no storage; a rank's shard of a small batch can be empty);
 *   - calls are stateless and thread-safe.
 */
#ifndef WTMI_H
#define WTMI_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- CWT (K1+K2) --------------------------------------------------------------
 * Replaces pycwt.cwt(signal, dt, dj, s0, J, Morlet(f0)) as called from
 * src/cwt.py:110-112 (power |W|^2 at :114, significance ratio at :123-133).
 * x: [batch][ld] float32, n0 <= 2^20 samples used per series (above 16384 the long-row
 *    path runs: see wtmi_cwt_workspace_bytes).
 * affine: optional [batch][3] float64 (a0, a1, a2): x' = (x - a0 - a1*t) * a2 applied
 *         before the transform (standardize_series / pycwt normalisation), or NULL.
 * scales: [n_scales] float64 (s_j).  sig_scale: float64 1/signif_j, series b reading
 *         sig_scale[b * sig_ld + j] (sig_ld = 0: one [n_scales] row for every series,
 *         else >= n_scales: per-series AR(1) levels, one launch for a whole batch), or
 *         NULL when out_sig is NULL.
 * Outputs (any may be NULL, not all): out_w [batch][n_scales][n0] complex64,
 *         out_power / out_sig [batch][n_scales][n0] float32.                       */
int wtmi_cwt_morlet(const float* x, long long ld, long long batch, long long n0,
                    const double* affine, const double* scales, int n_scales, double dt,
                    double f0, const double* sig_scale, long long sig_ld, float* out_w,
                    float* out_power, float* out_sig, void* workspace, void* stream);

/* ---- CWT / XWT with any pycwt mother ------------------------------------------
 * The same transforms for the other mothers of the reference's MOTHER_DICT
 * (src/xwt.py:29-34, src/wct.py:36-41, constants/results_configs.py:53-58):
 * mother 0 = Morlet(f0 = param) (exactly wtmi_cwt_morlet / wtmi_xwt_morlet), 1 = Paul(m = param),
 * 2 = DOG(m = param) (pycwt MexicanHat = DOG(2)); orders 1..40.  pycwt's filter
 * sqrt(s w_1 N) conj(psi_hat(s w_k)) is evaluated in-register (full transforms: the band
 * pruning is Morlet's).  Rows up to 16384 samples for mothers 1 and 2 (-2 above).          */
int wtmi_cwt_mother(const float* x, long long ld, long long batch, long long n0,
                    const double* affine, const double* scales, int n_scales, double dt,
                    int mother, double param, const double* sig_scale, long long sig_ld,
                    float* out_w, float* out_power, float* out_sig, void* workspace, void* stream);
int wtmi_xwt_mother(const float* x1, const float* x2, long long ld, long long batch,
                    long long n0, const double* affine1, const double* affine2,
                    const double* scales, int n_scales, double dt, int mother, double param,
                    const double* sig_scale, long long sig_ld, float* out_w12, float* out_power,
                    float* out_sig, float* out_u, float* out_v, void* workspace, void* stream);

/* Device scratch a CWT (pair = 0) or XWT (pair = 1) call needs: 0 for n0 <= 16384 (one
 * workgroup holds a row; workspace may be NULL), else the four-step long-row path's
 * spectra and work rows (bounded: series and scales are processed in chunks of about
 * 1 GiB each).  Rows up to 2^20 samples; longer ones return kErrUnsupported.         */
long long wtmi_cwt_workspace_bytes(long long batch, long long n0, int n_scales, int pair);

/* ---- CWT summaries (K24) ---------------------------------------------------------
 * Three reductions of the [batch][n_scales][n0] transform of wtmi_cwt_mother in one launch,
 * with that array neither written nor read:
 *   out_global [batch][n_scales]: mean over t in [t_lo[j], t_hi[j]) (clipped to [0, n0); both
 *     NULL: the whole row; an empty range gives NaN) of |W_j(t)|^2 -- replaces
 *     power.mean(axis=1), the global wavelet spectrum;
 *   out_band_power [batch][n_bands][n0] = sum_j power_w[k][j] |W_j(t)|^2 -- the scale-averaged
 *     power of Torrence & Compo 1998 eq. 24 with power_w = dj dt / (Cdelta s_j) inside band k;
 *   out_band_signal [batch][n_bands][n0] = sum_j signal_w[k][j] Re W_j(t) -- eq. 11 / pycwt.icwt
 *     restricted to band k with signal_w = dj sqrt(dt) / (Cdelta psi_0(0) sqrt(s_j)).
 * power_w / signal_w: float64 [n_bands][n_scales] device arrays, zero outside a band; n_bands in
 * 0..4.  Any output may be NULL, not all; a band output needs its weights and n_bands >= 1.
 * out_band_signal alone costs n_bands inverse transforms (the band-pass filter), not n_scales.
 * n0 in 9..16384 (band power: up to 8192); other lengths return -2 (compose them from
 * wtmi_cwt_mother).  workspace: wtmi_cwt_summary_workspace_bytes bytes when that is non-zero
 * (partial rows of series split over several workgroups; NULL then returns -1).  That size is
 * non-decreasing in n_bands, and in batch only while a series is split: it falls to 0 once every
 * series is one chunk (512 series or more with at most 128 scales, 64 from 8193 samples), so a
 * buffer kept for several batch sizes takes the largest value over them, not the value at the
 * largest batch.  No floating-point atomics: equal inputs give equal bits.                  */
int wtmi_cwt_summary(const float* x, long long ld, long long batch, long long n0,
                     const double* affine, const double* scales, int n_scales, double dt,
                     int mother, double param, const int* t_lo, const int* t_hi, int n_bands,
                     const double* power_w, const double* signal_w, float* out_global,
                     float* out_band_power, float* out_band_signal, void* workspace, void* stream);
long long wtmi_cwt_summary_workspace_bytes(long long batch, long long n0, int n_scales, int n_bands);

/* ---- XWT / phase (K1+K2, pair mode) ------------------------------------------
 * Replaces the two pycwt.cwt calls and W1*conj(W2) inside pycwt.xwt
 * (src/xwt.py:93-101) and the phase angle(W12) of pycwt.wct used for the arrows
 * (src/xwt.py:122-137, src/wct.py:106-138).  Outputs: W12 complex64, |W12|^2,
 * |W12|^2 * sig_scale_j, and the arrow components u = cos(pi/2 - angle(W12)),
 * v = sin(pi/2 - angle(W12)) (calculate_phase_difference, src/xwt.py:142-154).   */
int wtmi_xwt_morlet(const float* x1, const float* x2, long long ld, long long batch,
                    long long n0, const double* affine1, const double* affine2,
                    const double* scales, int n_scales, double dt, double f0,
                    const double* sig_scale, long long sig_ld, float* out_w12, float* out_power,
                    float* out_sig, float* out_u, float* out_v, void* workspace, void* stream);

/* ---- WCT coherence + XWT power / phase (K1+K2+K7+K8) ---------------------------
 * Replaces pycwt.wct(..., sig=False) numerics (src/wct.py:106-118): two CWTs,
 * Morlet.smooth of |W1|^2/s, |W2|^2/s, W12/s (time Gaussian via FFT + scale boxcar of
 * `boxcar` rows), WCT = |S12|^2/(S1 S2), aWCT = angle(W12) and the phase arrows; the
 * same pass emits the cross-wavelet power |W1 W2*|^2 (pycwt.xwt, src/xwt.py:93).
 * workspace: device scratch of wtmi_wct_workspace_bytes(batch, n0, n_scales) bytes.
 * Outputs [batch][n_scales][n0] float32; all but out_coh may be NULL (u, v together). */
long long wtmi_wct_workspace_bytes(long long batch, long long n0, int n_scales);
int wtmi_wct_morlet(const float* x1, const float* x2, long long ld, long long batch, long long n0,
                    const double* affine1, const double* affine2, const double* scales,
                    int n_scales, double dt, double f0, int boxcar, void* workspace,
                    float* out_coh, float* out_power, float* out_phase, float* out_u,
                    float* out_v, void* stream);

/* Side-stream pool entries the full-row WCT (n0 = 2^k >= 1024) has created in this process:
 * a call takes ONE entry (two streams and five events, created together: the full-band rows'
 * chain and, when wct_pc_early selects it -- by default for batches of at most 256 pairs --
 * phase C's q windows) from a per-device pool and joins both before returning
 * (on error paths too), so the count is the most such calls that ever overlapped, not the
 * number of host threads that made one.                                             */
long long wtmi_wct_side_streams(void);

/* wtmi_wct_morlet with pycwt's own normalisation of both series, (y - mean) / std with the
 * moments in fp64 over each series (pycwt.wct / xwt normalize=True, src/wct.py:106-118), done
 * inside the transform's first kernel -- no separate moments / affine launches.  Rows of
 * 9 .. 16384 samples (-2 otherwise: normalise through wtmi_series_affine + affine1/2).    */
int wtmi_wct_morlet_norm(const float* x1, const float* x2, long long ld, long long batch,
                         long long n0, const double* scales, int n_scales, double dt, double f0,
                         int boxcar, void* workspace, float* out_coh, float* out_power,
                         float* out_phase, float* out_u, float* out_v, void* stream);

/* ---- WCT Monte-Carlo significance (K10 / K11) ---------------------------------
 * Replace the pieces of pycwt.wct_significance reached from src/wct.py:106-118 with
 * sig=True.
 * wtmi_rednoise: helpers.rednoise(n, g, 1) for `count` series into out[count][ld]:
 *   pycwt: yr = lfilter([1,0],[1,-g], randn(n + tau, 1))[tau:], tau = ceil(-2/ln|g|) (0 if
 *   g == 0), filtered along lfilter's default axis -1 -- of length 1 -- i.e. not at all:
 *   filtered = 0 (pycwt's literal behaviour) writes the white normals tau .. tau + n - 1;
 *   filtered = 1 applies the AR(1) recurrence y_i = g y_{i-1} + e_i over all n + tau normals
 *   (the MATLAB rednoise.m intent) and writes y[tau:].  |g| < 1 (-1 otherwise).
 *   Normals come from Philox4x32-10 keyed by `seed`; series c uses stream
 *   first_series + c, so batches can be drawn in pieces reproducibly; both modes draw the
 *   same normals.
 * wtmi_coherence_histogram: adds, for s < n_hist_scales, the counts of
 *   clamp(floor(coh[p][s][t] * nbins), 0, nbins-1) over all pairs p and
 *   t in [t_lo[s], t_hi[s]) (the points outside the cone of influence; t_lo/t_hi are
 *   device int arrays) into hist[n_hist_scales][nbins] (uint32, caller-zeroed).
 *   nbins <= 4096.
 * wtmi_coherence_quantile: the quantile step of wct_significance for the first n_scales
 *   rows of hist[.][nbins]: out[s] = np.interp(level, P, (bin + 1/2) / nbins) over the
 *   non-empty bins, P = (cumsum - 1/2) / total (0 for a row without counts); out is a device
 *   float64 [n_scales].                                                              */
int wtmi_rednoise(float* out, long long ld, long long count, long long n, double g, int filtered,
                  unsigned long long seed, unsigned long long first_series, void* stream);
int wtmi_coherence_histogram(const float* coh, long long batch, long long n0, int n_scales,
                             const int* t_lo, const int* t_hi, int n_hist_scales, int nbins,
                             unsigned int* hist, void* stream);
int wtmi_coherence_quantile(const unsigned int* hist, int n_scales, int nbins, double level, double* out,
                            void* stream);

/* ---- MODWT (K3 / K4) -----------------------------------------------------------
 * Replace src/modwt.py:126-144 (modwt: rows [W_1..W_J, V_J]) and :147-160 (imodwt).
 * dec_lo/dec_hi: HOST pointers to the n_taps analysis filters (pywt dec_lo/dec_hi);
 * the kernels use h~ = dec_hi/sqrt2, g~ = dec_lo/sqrt2 (n_taps <= 128).
 * w: [batch][level+1][n] float32.  keep_mask (imodwt): bit r set = row r used, others
 * treated as zero (modwtmra / smooth_signal, src/modwt.py:163-251); ~0ull = all.
 * workspace: NULL for n <= 16384 (a series lives in one workgroup's LDS); longer series
 * run one launch per level and need wtmi_modwt_workspace_bytes() of device scratch.  */
long long wtmi_modwt_workspace_bytes(long long batch, long long n, int level);
int wtmi_modwt(const float* x, long long ld, long long batch, long long n, const double* dec_lo,
               const double* dec_hi, int n_taps, int level, float* w, void* workspace,
               void* stream);
int wtmi_imodwt(const float* w, long long batch, long long n, const double* dec_lo,
                const double* dec_hi, int n_taps, int level, unsigned long long keep_mask,
                float* x, long long ld_out, void* workspace, void* stream);

/* ---- DWT (K5 / K6) -------------------------------------------------------------
 * Replace pywt.wavedec / pywt.waverec with mode "symmetric" (src/dwt.py:104,120;
 * src/utils/transform_helpers.py:96).  Coefficients of one series are stored
 * back-to-back in pywt list order [cA_J, cD_J, ..., cD_1]; wtmi_dwt_lengths() gives
 * the per-array lengths (host, lens[level+1]) and returns the total per series.
 * waverec: n_variants reconstructions per series, variant v keeps array k when bit k
 * of keep_masks[v] is set (ResultsFromDWT.smooth_signal, reconstruct_signal_component,
 * src/dwt.py:53-73,110-120); out: [batch][n_variants][out_len].
 * workspace: NULL for n <= 16384; longer series run one launch per level and need
 * wtmi_dwt_workspace_bytes(batch, n, n_taps, n_variants) (wavedec: n_variants = 1).  */
long long wtmi_dwt_lengths(long long n, int n_taps, int level, long long* lens);
long long wtmi_dwt_workspace_bytes(long long batch, long long n, int n_taps, int n_variants);
int wtmi_wavedec(const float* x, long long ld, long long batch, long long n, const double* dec_lo,
                 const double* dec_hi, int n_taps, int level, float* coeffs, void* workspace,
                 void* stream);
int wtmi_waverec(const float* coeffs, long long batch, long long n, const double* rec_lo,
                 const double* rec_hi, int n_taps, int level,
                 const unsigned long long* keep_masks, int n_variants, float* out,
                 long long out_len, void* workspace, void* stream);

/* ---- time-scale regression (K17 / K18) ---------------------------------------------
 * time_scale_regression (src/regression.py:91-126): wavedec (mode symmetric) of both series,
 * the level+1 single-array reconstructions of each (reconstruct_signal_component,
 * src/dwt.py:110-120), OLS of output component on input component per array.
 * x (input) / y (output): [batch][ld] float32; dec_* / rec_*: HOST pointers to the n_taps filters.
 * stats: [batch][level+1][8] float64, component k in pywt list order (k = 0: S_J, k: D_{J-k+1}) =
 *   const, slope, bse_const, bse_slope, rsquared, ssr, nobs, df_resid.
 *   add_constant != 0: statsmodels OLS of y on [1, x] (df_resid = nobs - 2); else on x alone
 *   (uncentred rsquared, df_resid = nobs - 1, const = bse_const = 0).  nobs = out_len, pywt's
 *   waverec length (n for even n and at level 0, n + 1 for odd n): the reference regresses the
 *   untrimmed components.  The moments are fp64 sums of the fp32 components.
 *   Degenerate regressor: when the (centred, or without a constant the raw) sum of squares of
 *   the input component is exactly 0 -- a constant component, e.g. every component of an
 *   all-zero series -- slope, bse_slope and bse_const are NaN, const = mean(y component)
 *   (0 without a constant), ssr = the total sum of squares and rsquared = 0.
 * comps: NULL, or [batch][2][level+1][out_len] float32 (the components themselves; 0 = input series).
 * n <= 8192 and even n_taps in 2..40 (-2 otherwise: compose wavedec / waverec / wtmi_rows_ols). */
int wtmi_dwt_tsr(const float* x, const float* y, long long ld, long long batch, long long n,
                 const double* dec_lo, const double* dec_hi, const double* rec_lo,
                 const double* rec_hi, int n_taps, int level, int add_constant,
                 double* stats, float* comps, void* stream);
/* The same regression of rows that already exist: y row r on x row r, r < rows, both [rows][ld]
 * float32 with n samples used (MODWT MRA rows, src/modwt.py:197-229; the components of series
 * longer than 8192 samples).  stats: [rows][8] float64 as above, nobs = n.                  */
int wtmi_rows_ols(const float* x, const float* y, long long ld, long long rows, long long n,
                  int add_constant, double* stats, void* stream);

/* ---- DWT smoothing ladder with per-level OLS (K21) ----------------------------------
 * ResultsFromDWT.smooth_signal (src/dwt.py:53-73) from the series itself and
 * wavelet_approximation (src/regression.py:66-88) in one launch.  smooth_l (cD_1 .. cD_l zeroed)
 * is cA_l pushed through l low-pass-only synthesis steps, so no detail coefficient is computed
 * and only the low-pass pair of the bank is needed.
 * x, y: [batch][ld] float32; y may be NULL when stats is NULL.  dec_lo / rec_lo: HOST pointers.
 * smooth: NULL, or [batch][level][n] float32; row l-1 is smoothed_signal_dict[l]["signal"]
 *   (already trimmed: n samples, for odd n the first reconstructed sample is dropped).
 * stats: NULL, or [batch][level][8] float64; row l-1 is the OLS of the raw y on [1, smooth_l(x)],
 *   or on smooth_l(x) alone when add_constant == 0.  Columns and the degenerate-regressor rule
 *   exactly as wtmi_dwt_tsr, nobs = n.
 * -1: both outputs NULL, stats without y, level < 1, ld < n, a NULL bank pointer.
 * -2: n > 8192, n_taps odd or > 40, level > 60 (compose wtmi_wavedec, wtmi_waverec with the
 *   level keep-masks and wtmi_rows_ols).  A level deeper than the series supports is exact.
 * One workgroup per series and group of chains; the chains of a series are split into groups
 * where their LDS rows exceed half a CU's 160 KiB (csrc/dwt_smooth.hip).                     */
int wtmi_dwt_smooth(const float* x, const float* y, long long ld, long long batch, long long n,
                    const double* dec_lo, const double* rec_lo, int n_taps, int level,
                    int add_constant, float* smooth, double* stats, void* stream);

/* ---- DWT wavelet shrinkage with MAD thresholds (K23) ---------------------------------
 * Denoising by wavelet shrinkage (Donoho & Johnstone 1994) in one launch: pywt.wavedec (mode
 * symmetric) of every series, a threshold per detail level, pywt.threshold of the detail
 * arrays and pywt.waverec of the shrunk list.  cA_J is never modified.
 * x: [batch][ld] float32; dec_* / rec_*: HOST pointers to the n_taps filters.
 * rule 0 (fixed): lambda_j = thresholds[b * thr_ld + j - 1], DEVICE float64; thr_ld = 0: one
 *   [level] row for every series, else thr_ld >= level.  mult is ignored, sigma_j is NaN.
 * rule 1 (universal, VisuShrink): sigma = median(|cD_1|) / 0.6744897501960817 and lambda_j =
 *   mult sigma sqrt(2 ln n) for every j, n the series length.
 * rule 2 (level-dependent universal, Johnstone & Silverman 1997, for coloured noise):
 *   sigma_j = median(|cD_j|) / 0.6744897501960817, lambda_j = mult sigma_j sqrt(2 ln n).
 *   The median is np.median of the fp32 coefficients' magnitudes, exactly (the middle order
 *   statistic, or the fp64 mean of the two middle ones; ties handled).  sigma and lambda are
 *   fp64; a coefficient is compared in fp32 against (float)lambda.
 * shrink 0 (soft): sign(c) max(|c| - lambda, 0).  shrink 1 (hard): c if |c| >= lambda, else 0.
 * shrink 2 (non-negative garrote): c (1 - lambda^2 / c^2) if |c| > lambda, else 0 (lambda = 0
 *   is the identity: 0 / 0 is never evaluated).
 * out: [batch][ld_out] float32, the FIRST n samples of the reconstruction (pywt's
 *   waverec(...)[:n]; not trim_signal, which drops sample 0 for odd n).  lambda = 0 returns x.
 * info: NULL, or [batch][level][4] float64, row j-1 = sigma_j, lambda_j, kept_j, len_j; kept_j
 *   counts the coefficients of cD_j that are non-zero by the rule's own inequality.
 * coeffs: NULL, or [batch][total] float32, the shrunk coefficients in wtmi_wavedec's layout.
 * -1: a NULL bank pointer or NULL out, ld < n, ld_out < n, level < 1, rule or shrink outside
 *   0..2, mult < 0 or not finite, rule 0 without thresholds or with 0 < thr_ld < level.
 * -2: n > 8192, n_taps odd or > 40, level > 60 (compose wtmi_wavedec, a shrink of the
 *   coefficient rows and wtmi_waverec).  A level deeper than the series supports is exact.
 *   Non-finite input samples are unspecified.
 * One workgroup per series; every detail array stays in LDS between analysis and synthesis,
 * about 2 n floats, so two workgroups share a CU up to n = 8192 (csrc/dwt_denoise.hip).    */
int wtmi_dwt_denoise(const float* x, long long ld, long long batch, long long n,
                     const double* dec_lo, const double* dec_hi, const double* rec_lo,
                     const double* rec_hi, int n_taps, int level, int rule, int shrink, double mult,
                     const double* thresholds, long long thr_ld, float* out, long long ld_out,
                     double* info, float* coeffs, void* stream);

/* ---- MODWT multiresolution analysis (K19 / K20) -------------------------------------
 * wtmi_modwt_mra replaces the MODWT workflow of src/modwt.py:466-487 in one launch: modwt
 * (:126-144) + modwtmra (:163-194) of x (and of y), smooth_signal (:232-251) and
 * time_scale_regression on the MRA rows (:197-229).  No coefficient array is formed: level j
 * applies the autocorrelations of h~ / g~ at dilation 2^(j-1) to the running smooth U_{j-1}.
 * x / y: [batch][ld] float32, y NULL for single series (P = 1; P = 2 with y, 0 = x).
 * mra: NULL, or [batch][P][level+1][n] float32, rows [D_1 .. D_J, S_J] (the reference's
 *   modwtmra(modwt(x)) row order).
 * smooth: NULL, or [batch][P][level][n]; row l-1 is U_l = smooth_signal(...)[l]["signal"]
 *   (for an orthonormal bank, as every pywt wavelet of the reference is).
 * stats: NULL, or [batch][level+1][8] float64 in MRA row order: OLS of y's row on x's row,
 *   columns, add_constant and the degenerate-regressor rules as wtmi_dwt_tsr, nobs = n.
 * -1: stats without y, or mra, smooth and stats all NULL.  level in 1..62.
 * n <= 16384 and n_taps in 2..40 (-2 otherwise: compose wtmi_modwt, one-bit-mask wtmi_imodwt
 * and wtmi_rows_ols).  A pair holds both series in LDS (2 n floats of the CU's 160 KiB): pairs
 * of at most 8192 samples run two or more workgroups per CU, longer ones one.              */
int wtmi_modwt_mra(const float* x, const float* y, long long ld, long long batch, long long n,
                   const double* dec_lo, const double* dec_hi, int n_taps, int level,
                   int add_constant, float* mra, float* smooth, double* stats, void* stream);
/* modwtmra(w, filters) (src/modwt.py:163-194) of coefficient rows that already exist (e.g.
 * thresholded ones): w and mra [batch][level+1][n] float32, rows [W_1 .. W_J, V_J] in and
 * [D_1 .. D_J, S_J] out; each row is inverted alone, the zero rows of the reference's masked
 * inverse are never read.  Limits and return codes as wtmi_modwt_mra.                     */
int wtmi_modwt_mra_rows(const float* w, long long batch, long long n, const double* dec_lo,
                        const double* dec_hi, int n_taps, int level, float* mra, void* stream);

/* ---- MODWT wavelet variance / correlation / cross-correlation (K22) -------------------
 * The by-scale co-movement table of a MODWT analysis (Percival & Walden ch. 8; Whitcher,
 * Guttorp & Percival 2000; the lead / lag analysis of Gencay, Selcuk & Whitcher ch. 7) -- the
 * per-scale counterpart of correlation_matrix_pvalues (src/statistical_analysis.py) -- from the
 * series themselves in one launch: the coefficients W_j of wtmi_modwt (detail levels 1..level)
 * are formed in LDS and never written out.
 * x / y: [batch][ld] float32; y NULL for a single series.  The passes run on x - x[0], y - y[0].
 * boundary 1 (brick wall, the unbiased estimator): only the coefficients t >= t0 = L_j - 1,
 *   L_j = (2^j - 1)(n_taps - 1) + 1, which never touch the wrap, count; M_j = n - t0.
 * boundary 0 (periodic): t0 = 0, M_j = n, lagged indices wrap mod n.
 * stats: [batch][level][8] float64, row j-1 = var_x, var_y, cov, corr, nobs, ci_lo, ci_hi, n_eff:
 *   (1/M_j) sums over t >= t0 of W^x W^x, W^y W^y, W^x W^y (no mean subtracted), corr =
 *   cov / sqrt(var_x var_y), nobs = M_j, ci = tanh(atanh(corr) -+ z / sqrt(n_eff - 3)) with
 *   n_eff = floor(n / 2^j) - ceil((n_taps - 2)(1 - 2^-j)) (brick wall) or floor(n / 2^j);
 *   z: the normal quantile of the caller's confidence level.
 * xcorr: NULL when max_lag == 0, else [batch][level][2 max_lag + 1] float64: column lag + max_lag =
 *   (1/M_j) sum_t W^x[t] W^y[t + lag] / sqrt(var_x var_y), brick wall: t and t + lag both in
 *   [t0, n - 1]; periodic: every t, index (t + lag) mod n.  A peak at lag > 0: x leads y.
 *   Column max_lag is corr itself.
 * Data-dependent rows (not errors): M_j <= 0: nobs = 0, every other column and the xcorr row NaN;
 *   var_x or var_y exactly 0 (a constant series): corr, ci and the xcorr row NaN; n_eff <= 3: ci
 *   NaN; without y only var_x, nobs and n_eff are numbers.
 * -1: a NULL bank, ld < n, level outside 1..62, boundary not 0 / 1, max_lag < 0 or >= n, stats
 *   NULL, xcorr without max_lag or max_lag without xcorr, xcorr without y.
 * -2: n_taps > 40, n > 16384, n > 8192 with max_lag > 0, max_lag > 64 (compose wtmi_modwt and
 *   reductions over its rows).  One workgroup per pair: two smooth rows and, with lags, two
 *   coefficient rows of n floats in LDS (128 KiB at n = 8192, one workgroup per CU).        */
int wtmi_modwt_wcorr(const float* x, const float* y, long long ld, long long batch, long long n,
                     const double* dec_lo, const double* dec_hi, int n_taps, int level,
                     int boundary, int max_lag, double z, double* stats, double* xcorr, void* stream);

/* ---- Time-localized (rolling-window) MODWT wavelet correlation (K27) --------------------
 * When the co-movement of wtmi_modwt_wcorr's table changed: the rolling-window wavelet correlation
 * (Ranta 2010; Gencay, Selcuk & Whitcher ch. 7 in rolling form) and its weighted generalisation,
 * the local wavelet correlation of Fernandez-Macho (2018; wlmc of the R package wavemulcor) for
 * one pair: a symmetric window theta(k), |k| <= H = half_width, slid over the coefficients W_j of
 * wtmi_modwt (detail levels 1..level), which are formed in LDS and never written out.
 * x / y: [batch][ld] float32; y NULL for a single series (the local wavelet variance only).  The
 *   passes run on x - x[0], y - y[0].  dec_*: HOST pointers to the n_taps filters.
 * window: DEVICE float64 [half_width + 1], window[k] = theta(k) >= 0, theta(0) > 0 (other values:
 *   unspecified results).
 * For every centre s in [0, n) the counted coefficients C(s) are
 *   boundary 1 (brick wall): t in [max(t0, s - H), min(n - 1, s + H)], t0 = (2^j - 1)(n_taps - 1) as
 *     wtmi_modwt_wcorr: the window is cut at the wall and at the series end and never wraps;
 *   boundary 0 (periodic): t = (s + k) mod n for every |k| <= H (2 H + 1 <= n: none counts twice).
 * In fp64 from the fp32 coefficients: Sw(s) = sum_C(s) theta(t - s) and A^ab(s) = sum_C(s)
 *   theta(t - s) W^a_j[t] W^b_j[t], ab in {xx, yy, xy}.
 * corr: NULL, or [batch][level][ld_out] float32, row j-1: A^xy / sqrt(A^xx A^yy) clamped to [-1, 1].
 * moments: NULL, or [batch][level][3][ld_out] float32, planes A^xx / Sw, A^yy / Sw, A^xy / Sw (the
 *   local wavelet variances and covariance).  Without y only plane 0 is written; planes 1 and 2
 *   are left untouched.  Both are computed in fp64 and rounded once.
 * Data-dependent values (not errors): Sw(s) = 0 (no counted coefficient in the window): all four
 *   NaN; A^xx = 0 or A^yy = 0 (a window without energy): corr NaN, that variance and the
 *   covariance 0.
 * -1: a NULL bank or window, ld < n, ld_out < n, level outside 1..62, boundary not 0 / 1,
 *   half_width < 0, periodic with 2 half_width + 1 > n, corr and moments both NULL, corr without y.
 * -2: n > 8192, n_taps > 40, half_width > 1024 (compose wtmi_modwt and windowed reductions over
 *   its rows).  One workgroup per pair: two smooth rows, two coefficient rows with a halo of
 *   half_width on either side and the weights in LDS (152 KiB at n = 8192, half_width = 1024, one
 *   workgroup per CU).  A series shorter than the dilated filter is exact (the offsets wrap).
 *   Equal inputs give equal bits (no atomics).                                                */
int wtmi_modwt_lwcorr(const float* x, const float* y, long long ld, long long batch, long long n,
                      const double* dec_lo, const double* dec_hi, int n_taps, int level,
                      int boundary, const double* window, int half_width,
                      float* corr, float* moments, long long ld_out, void* stream);

/* ---- MODWT wavelet correlation matrix / wavelet multiple correlation (K25) -------------
 * K22 for M series at once: the wavelet covariance and correlation matrices of all M series of a
 * group at every MODWT detail level (the by-scale correlation_matrix_pvalues table itself) and
 * the wavelet multiple correlation of Fernandez-Macho (2012; the R package wavemulcor), from the
 * series themselves in one launch.  The per-level Gram matrix W_j W_j^T is accumulated by the
 * fp64 16 x 16 x 4 matrix instruction in fp64 from the fp32 coefficients; W_j never leaves the
 * registers.
 * x: [batch][n_series][ld] float32 (M = n_series); the passes run on x - x[0] of every series.
 * boundary, z, t0, M_j and n_eff as wtmi_modwt_wcorr.
 * cov: [batch][level][M][M] float64, (1/M_j) sums over t >= t0 of W^a W^b, full and symmetric
 *   bit for bit.  corr: NULL or the same shape, cov_ab / sqrt(cov_aa cov_bb), symmetric bit for
 *   bit, the diagonal exactly 1 where the variance is not 0.
 * r2: [batch][level][M], R^2_i = 1 - 1 / (P_j^-1)_ii of series i regressed on the others, P_j =
 *   corr, from an fp64 Cholesky factor P = L L^T: (P^-1)_ii = sum_k (L^-1)_ki^2.
 * stats: [batch][level][6] float64 = wmc, target, ci_lo, ci_hi, nobs, n_eff: wmc = sqrt(max_i
 *   R^2_i) (a maximum below 0 by rounding counts as 0), target the first maximising i, ci =
 *   tanh(atanh(wmc) -+ z / sqrt(n_eff - 3)), nobs = M_j.  r2 and stats are NULL together or not at all.
 * Data-dependent rows (not errors): M_j <= 0: nobs = 0, everything else NaN; a series with
 *   variance exactly 0: its corr row and column and the level's r2, wmc, target and ci NaN;
 *   nobs < M, or a Cholesky pivot that is not > 0: r2, wmc, target and ci NaN; n_eff <= 3: ci NaN.
 *   A matrix that is singular only up to rounding may give either NaN or values near 1.
 * -1: a NULL bank, x or cov, ld < n, n_series < 2, level outside 1..62, boundary not 0 / 1, r2
 *   without stats or stats without r2.
 * -2: n_series > 16, n_series * n > 32768, n_taps > 40 (compose wtmi_modwt, Gram products and a
 *   factorisation of its rows).  One workgroup per group: M smooth rows in LDS (128 KiB at
 *   M n = 32768, one workgroup per CU): n <= 2048 at M = 16, 8192 at M = 4, 16384 at M = 2.   */
int wtmi_modwt_wcmat(const float* x, long long ld, long long batch, int n_series, long long n,
                     const double* dec_lo, const double* dec_hi, int n_taps, int level,
                     int boundary, double z, double* cov, double* corr, double* r2,
                     double* stats, void* stream);

/* ---- MODWT translation-invariant wavelet shrinkage with MAD thresholds (K26) -----------
 * The undecimated counterpart of wtmi_dwt_denoise (Coifman & Donoho's cycle spinning; Percival &
 * Walden 2000, ch. 10.5-10.6): wtmi_modwt of every series, a threshold per detail level, the
 * shrink of wtmi_dwt_denoise applied to every W~_j, and wtmi_imodwt of the shrunk rows, in one
 * launch.  V~_J is never modified.  The result does not depend on where the series starts.
 * x: [batch][ld] float32; dec_*: HOST pointers to the n_taps filters.  The passes run on
 * x - x[0]; x[0] returns at the end (a constant series comes back exactly).
 * rule 0 (fixed): lambda_j = thresholds[b * thr_ld + j - 1], DEVICE float64; thr_ld = 0: one
 *   [level] row for every series, else thr_ld >= level.  mult is ignored, sigma_j is NaN.
 * rule 1 (universal): sigma = sqrt2 median(|W~_1|) / 0.6744897501960817 (the series' own units)
 *   and lambda_j = mult sigma sqrt(2 ln n) / 2^(j/2).
 * rule 2 (level-dependent): sigma_j = 2^(j/2) median(|W~_j|) / 0.6744897501960817 and lambda_j =
 *   mult sigma_j sqrt(2 ln n) / 2^(j/2).  The median, sigma, lambda, the fp32 comparison against
 *   (float)lambda_j and shrink 0 / 1 / 2 (soft, hard, garrote) are those of wtmi_dwt_denoise.
 * out: [batch][ld_out] float32.  lambda = 0 returns x.
 * info: NULL, or [batch][level][4] float64, row j-1 = sigma_j, lambda_j, kept_j, n.
 * coeffs: NULL, or [batch][level+1][n] float32, the shrunk rows in wtmi_modwt's row order
 *   [W~_1 .. W~_J, V~_J].
 * workspace: DEVICE, wtmi_modwt_denoise_workspace_bytes(batch, n, level) bytes; may be NULL when
 *   that is 0 or when coeffs is given (the spilled rows then live in coeffs).  No allocation
 *   inside the call.  One workgroup per series keeps, in floats with np = n rounded up to 4, the
 *   V row [0, np) and the R = min(level, 36864 / np - 1) COARSEST coefficient rows in LDS, W~_j
 *   at [np (j - S), np (j - S + 1)); the S = level - R finest rows go to the workspace, series b's
 *   W~_j at float offset (b S + j - 1) n: batch * S * n * 4 bytes (0 for n = 1333, level 7;
 *   9 * 16384 * 4 per series for n = 16384, level 10).  -1 from the size query: bad geometry.
 * -1: a NULL bank pointer or NULL out, ld < n, ld_out < n, level outside 1..62, rule or shrink
 *   outside 0..2, mult < 0 or not finite, rule 0 without thresholds or with 0 < thr_ld < level,
 *   spilled rows with neither workspace nor coeffs.
 * -2: n > 16384 or n_taps > 40 (compose wtmi_modwt, a shrink of its rows and wtmi_imodwt).  A
 *   series shorter than the dilated filter is exact (the offsets wrap).  Non-finite input
 *   samples are unspecified.                                                                  */
long long wtmi_modwt_denoise_workspace_bytes(long long batch, long long n, int level);
int wtmi_modwt_denoise(const float* x, long long ld, long long batch, long long n,
                       const double* dec_lo, const double* dec_hi, int n_taps, int level, int rule,
                       int shrink, double mult, const double* thresholds, long long thr_ld,
                       float* out, long long ld_out, double* info, float* coeffs, void* workspace,
                       void* stream);

/* ---- per-series moments / affine (K9) -----------------------------------------
 * Replace standardize_series (src/utils/wavelet_helpers.py:22-57) and the
 * covariances of pycwt.ar1 (src/cwt.py:106).  out: [batch][8] float64 =
 * mean, std (ddof 0), slope, intercept, c0, c1, n, 0.                              */
int wtmi_series_moments(const void* x, int x_is_f64, long long ld, long long batch, long long n,
                        double* out, void* stream);
int wtmi_affine(const void* x, int x_is_f64, long long ld_in, long long batch, long long n,
                const double* coef, void* y, int y_is_f64, long long ld_out, void* stream);
/* The affine coefficients [batch][3] (a0, a1, a2: x' = (x - a0 - a1 t) a2) in one pass over the
 * series, for the transforms' `affine` arguments: mode bits 1 detrend (polyfit deg 1), 2 remove
 * the mean, 4 divide by the std -- standardize_series(detrend, standardize, remove_mean) of
 * src/utils/wavelet_helpers.py:22-57 (1 and 2 together: -1, as its ValueError), and 6 = pycwt's
 * xwt/wct normalisation (y - mean) / std.  moments: [batch][8] as above, or NULL. */
int wtmi_series_affine(const void* x, int x_is_f64, long long ld, long long batch, long long n, int mode,
                       double* moments, double* affine, void* stream);

/* ---- launch options (no reference counterpart) ----------------------------------
 * Launch-policy knobs, read from WTMI_<NAME> environment variables once at first use
 * and settable here: cwt_prune (2 band rows + narrowed entry passes, 1 band rows, 0 full
 * transforms), cwt_target_wg, wct_prune (2 band rows + decimated spectra of full rows, 1 band
 * rows, 0 full transforms), wct_target_wg, wct_min_rows and wct_dec_rows (scale rows per WCT
 * workgroup and decimated rows per phase-A workgroup; 0 = chosen by batch size), modwt_syn
 * (n = 8192 / 16384 synthesis: 1 hybrid kernel with the low levels staged through LDS, 0
 * dilation chains only), wct_wide (0: windows touching a full-band row always take the
 * time-domain path; 1..3: from which union-band exponent on they take the spectral route),
 * wct_side_stream (1: the full-band rows' kernel on a pooled side stream beside the
 * decimated rows' chain), wct_pc_early (phase C's q windows on a third pooled stream right
 * after the decimated spectra: 1 always, 0 never, 2 for batches of at most 256 pairs),
 * wct_dec_merge (the decimation classes M = 4096 .. 512 in one launch: 1 always, 0 never, 2 for
 * batches of at most 256 pairs), modwt_ana
 * (n = 16384 analysis geometry: 0 1024 threads x 4 float4 groups, 1 512 x 8, 2 256 x 16).  The prune and kernel switches exist so that tests can
 * compare the paths; results agree to fp32 resolution either way.  The environment gives the process
 * defaults; wtmi_set_option changes the CALLING thread's value only (thread-local), so it
 * never races a launch issued by another thread, and wtmi_get_option reads it back.
 * wtmi_set_option: 0, or -1 for an unknown name / out-of-range value;
 * wtmi_get_option: the value, or -1 for an unknown name.                             */
int wtmi_set_option(const char* name, long long value);
long long wtmi_get_option(const char* name);

#ifdef __cplusplus
}
#endif

#endif /* WTMI_H */
