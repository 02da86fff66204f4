// Fused CWT summaries (K24 of DESIGN.md): global wavelet spectrum, scale-averaged band power and
// band-pass reconstruction of a batch of series, with no [batch, scales, n0] array written or read.
//
// Replaces, on the arrays of wtmi_cwt_mother,
//   global[b, j]         = mean_t |W_j(t)|^2  over t in [t_lo[j], t_hi[j])      (power.mean(axis=1))
//   band_power[b, k, t]  = sum_j pw[k, j] |W_j(t)|^2                            (Torrence & Compo eq. 24)
//   band_signal[b, k, t] = sum_j rw[k, j] Re W_j(t)                             (eq. 11, pycwt.icwt)
// with host-made weights pw, rw (zero outside a band).
//
// Work split: the CWT kernel's (cwt.hip).  One workgroup = one series x a chunk of scales; the
// forward FFT runs once, the spectrum X stays in 16 complex registers per thread; each scale is a
// filter multiply + in-LDS inverse FFT after which thread t holds W_j at positions t + m NT, the
// same positions for every scale.  The epilogue stores nothing per row:
//  - |W_j|^2 is summed over the thread's positions inside [t_lo, t_hi), reduced over the row's
//    lanes by an xor butterfly, and each wave's partial goes to an LDS table slot of its own
//    (scale, wave): no barrier is added to the scale loop; after the loop the slots are summed in
//    wave order and divided by the count (an empty range: 0 / 0 = NaN, as np.mean of nothing);
//  - band power accumulates in 16 KB registers (KB = bands of the instantiation, 1 / 2 / 4) of the
//    thread that owns the positions;
//  - the band signal is NOT accumulated per scale: Re and the sum over scales commute with the
//    inverse transform, so after the loop the kernel forms Y_k = X sum_j rw[k, j] conj(psi_hat_j)
//    in registers (the filter gains are real up to the mother's constant phase, 16 KB floats, in
//    the registers the power accumulators just left) and runs ONE inverse FFT per band.  The
//    all-outputs launch therefore needs 16 KB accumulators, not 32 KB, and the signal-only launch
//    (POW = false: no scale loop at all) costs K inverse transforms instead of S.
// Workgroups that run several rows at once (ROWS > 1, N < 4096) give each row group its own scales
// (jl = g mod ROWS); the groups' rows are combined through LDS in group order.  A series split over
// several chunks writes partial rows to the workspace and sum_chunks_kernel adds them in chunk
// order.  No floating-point atomics anywhere: the same input gives the same bits.
// The scale loop issues no global load (weights, ranges and filter constants sit in LDS tables,
// see cwt_morlet_kernel).  Packed twiddle products: this kernel is bound by the transforms, not by
// a store stream (fft_lds.hpp, WTMI_PK_TWIDDLES).
#include "cwt_common.hpp"

namespace wtmi {

constexpr int kSumMaxBands = 4;

struct SumArgs {
  CwtArgs c;         // series, scales, mother and chunking (nchunks, chunk, prune)
  const int* t_lo;   // [S] or null: the global mean's range per scale, clipped to [0, n0)
  const int* t_hi;
  const double* pw;  // [K][S] weights of this launch's bands, or null
  const double* rw;
  float* out_global;  // [batch][S] or null
  float* out_bp;      // row (b * kstride + k) * n0 of this launch's band k, or null
  float* out_bs;
  float* ws;          // nchunks > 1: partial rows [batch][nchunks][wrows][n0]
  int K;              // bands of this launch (<= KB of the instantiation)
  int kstride;        // bands of the output arrays
  int wrows;          // partial rows per chunk: power rows first, signal rows from wsig
  int wsig;
};

template <int LOGN, int VAR>
struct SumGeom {
  using P = FftPlan<LOGN>;
  using G = CwtGeom<LOGN, 0, VAR>;
  static constexpr int WPR = P::NT > kWave ? P::NT / kWave : 1;  // waves per row
  // scales per workgroup (the per-scale LDS tables).  N >= 8192 takes 64: with the CWT's 128 the
  // tables push the bandless N = 8192 kernel past 80 KiB, i.e. from two workgroups per CU to one.
  static constexpr int MAXCHUNK = LOGN >= 13 ? 64 : G::MAXCHUNK;
  // registers: the CWT kernel's budget plus 16 KB accumulators.  256 threads (N <= 4096) and 512
  // (N = 8192) take two waves per SIMD (<= 256 VGPRs) once a band is accumulated; the
  // 1024-thread block of N = 16384 is four waves per SIMD by itself (<= 128 VGPRs): its scale
  // loop has room for the global sums only (one band's 16 accumulators spilled 51 VGPRs), and
  // its signal launches carry one band each (sum_kb_max).  Band power at N = 16384 is therefore
  // not fused (kErrUnsupported; ops composes it).
  static constexpr int minw(int kb) { return G::BLOCK >= 1024 ? 4 : (kb == 0 ? G::MINW : 2); }
};

// bands one launch accumulates in registers (more bands: several launches, see run_summary)
constexpr int sum_kb_max(int logn) { return logn >= 14 ? 1 : kSumMaxBands; }

// The scalar gain of morlet_filter / mother_filter at the thread's 16 bins (the filters are
// X[m] * gain[m], times the mother's constant phase for VAR = 1).
template <int LOGN, int VAR>
__device__ __forceinline__ void filter_gain(float (&psi)[16], cpx prm, const CwtArgs& a, float f0, int t) {
  using P = FftPlan<LOGN>;
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    const float kk = static_cast<float>(t + (m < 8 ? m : m - 16) * P::NT);
    if constexpr (VAR == 0) {
      const float e = fmaf(prm.x, kk, -f0);
      psi[m] = __builtin_amdgcn_exp2f(fmaf(e * (-0.5f * kLog2e), e, prm.y));
    } else {
      const float f = prm.x * kk;
      float p = __builtin_amdgcn_exp2f(fmaf(a.mA * f, f, fmaf(a.mB, f, fmaf(a.mP, __log2f(fabsf(f)), prm.y))));
      if (a.mgate == 1) p = f > 0.f ? p : 0.f;
      if (a.mgate == 2) p = f < 0.f ? -p : p;
      psi[m] = p;
    }
  }
}

// Rows held as acc[k][m] = value at position t + m NT of row group g -> dst + k * n0 (k < nrows).
// ROWS > 1: the groups' rows are summed through LDS (buf: ROWS * N floats, the FFT buffer) in
// group order.  Every thread of the workgroup must call this (barriers).
template <int LOGN, int VAR, int R>
__device__ __forceinline__ void emit_rows(const float (&acc)[R][16], int nrows, float* dst, int n0, int g,
                                          int t, float* buf) {
  using P = FftPlan<LOGN>;
  using G = CwtGeom<LOGN, 0, VAR>;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    if (k >= nrows) break;
    float* row = dst + static_cast<long long>(k) * n0;
    if constexpr (G::ROWS == 1) {
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const int pos = t + m * P::NT;
        if (pos < n0) row[pos] = acc[k][m];
      }
    } else {
      __syncthreads();  // the last transform's (or row's) readers are done with buf
#pragma unroll
      for (int m = 0; m < 16; ++m) buf[g * P::N + t + m * P::NT] = acc[k][m];
      __syncthreads();
      for (int p = threadIdx.x; p < P::N; p += G::BLOCK) {
        float s = 0.f;
        for (int gg = 0; gg < G::ROWS; ++gg) s += buf[gg * P::N + p];
        if (p < n0) row[p] = s;
      }
    }
  }
}

template <int LOGN, int KB, int VAR, bool POW>
__global__ void __launch_bounds__((CwtGeom<LOGN, 0, VAR>::BLOCK), (SumGeom<LOGN, VAR>::minw(KB)))
cwt_summary_kernel(SumArgs s) {
  using P = FftPlan<LOGN>;
  using G = CwtGeom<LOGN, 0, VAR>;
  using SG = SumGeom<LOGN, VAR>;
  constexpr int KA = KB > 0 ? KB : 1;
  const CwtArgs& a = s.c;
  constexpr int kBuf4 = (G::ROWS * P::PADN) / 2;
  // per-scale tables: filter constants, power weights, signal weights (float4 each), the
  // global mean's range, and the global sums' (scale, wave) slots
  constexpr int MC = SG::MAXCHUNK;
  constexpr int MCW = KB > 0 ? MC : 0;  // no weight tables without bands
  __shared__ float4 lds4[kBuf4 + MC + 2 * MCW + G::TWL_F4];
  __shared__ int2 rng[MC];
  __shared__ float gsum[POW ? MC * SG::WPR : 1];
  __shared__ float red[G::BLOCK / kWave];
  cpx* lds = reinterpret_cast<cpx*>(lds4);
  float4* prm_tab = lds4 + kBuf4;
  float4* pw_tab = prm_tab + MC;
  float4* rw_tab = pw_tab + MCW;
  float4* twl = rw_tab + MCW;
  const int tid = threadIdx.x;
  const int g = tid / P::NT;
  const int rt = tid - g * P::NT;
  const int t = fft_thread<LOGN>(rt);
  const long long blk = blockIdx.x;
  const long long b = blk / a.nchunks;
  const int ch = static_cast<int>(blk - b * a.nchunks);
  const int j0 = ch * a.chunk;
  const int nj = min(a.S, j0 + a.chunk) - j0;
  cpx* my = lds + g * P::PADN;
  constexpr int bufstride = G::ROWS * P::PADN;

  for (int i = tid; i < nj; i += G::BLOCK) {
    const int j = j0 + i;
    const double sc = a.scales[j];
    cpx mp = morlet_params(sc, a.dt, P::N);
    if constexpr (VAR == 1)
      mp.y = static_cast<float>(log2(sqrt(2.0 * kPi * sc / a.dt) / static_cast<double>(P::N)) + a.mlnorm);
    const int code = VAR == 0 ? row_code<LOGN>(sc, a.dt, a.f0, a.prune) : 0;
    prm_tab[i] = make_float4(mp.x, mp.y, 0.f, static_cast<float>(code));
    float w[2][kSumMaxBands];
#pragma unroll
    for (int k = 0; k < kSumMaxBands; ++k) {
      const long long o = static_cast<long long>(k) * a.S + j;
      w[0][k] = (k < s.K && s.pw) ? static_cast<float>(s.pw[o]) : 0.f;
      w[1][k] = (k < s.K && s.rw) ? static_cast<float>(s.rw[o]) : 0.f;
    }
    if constexpr (KB > 0) {
      pw_tab[i] = make_float4(w[0][0], w[0][1], w[0][2], w[0][3]);
      rw_tab[i] = make_float4(w[1][0], w[1][1], w[1][2], w[1][3]);
    }
    rng[i] = make_int2(s.t_lo ? max(s.t_lo[j], 0) : 0, s.t_hi ? min(s.t_hi[j], a.n0) : a.n0);
  }

  constexpr bool TWL = G::TWL;
  cpx tw[TWL ? P::NTW_REG : P::NTW_ALLOC];
  if constexpr (TWL) {
    fft_twiddle_table<LOGN>(twl, tid, G::BLOCK);
    fft_twiddles_tail<LOGN>(tw, t);
    __syncthreads();
  } else {
    fft_twiddles<LOGN>(tw, t);
  }
  int par = 0;

  cpx X[16];
  load_series<LOGN>(X, a.x, a.affine, b, a.ld, a.n0, t);
  const float mu = demean_row<LOGN>(X, a.n0, t, red);
  fft_row<LOGN, -1, 1, TWL>(X, my, bufstride, tw, t, par, twl);
  add_mean_spectrum<LOGN>(X, mu, a.n0, t);
  __syncthreads();  // tables visible (the FFT barriers may be absent for N = 16)

  const float f0 = static_cast<float>(a.f0);
  // partial rows of this (series, chunk), or the output rows themselves with one chunk
  const bool part = a.nchunks > 1;
  float* wsb = part ? s.ws + (b * a.nchunks + ch) * static_cast<long long>(s.wrows) * a.n0 : nullptr;
  const long long orow = b * s.kstride * static_cast<long long>(a.n0);
  float* fbuf = reinterpret_cast<float*>(lds4);

  if constexpr (POW) {
    float ap[KA][16];
#pragma unroll
    for (int k = 0; k < KA; ++k)
#pragma unroll
      for (int m = 0; m < 16; ++m) ap[k][m] = 0.f;
    const int iters = (nj + G::ROWS - 1) / G::ROWS;
    for (int it = 0; it < iters; ++it) {
      const int jl = it * G::ROWS + g;
      const bool valid = jl < nj;
      const float4 prm4 = prm_tab[valid ? jl : 0];
      const cpx prm = mkc(prm4.x, prm4.y);
      // the iteration's row code: the widest band among its rows (workgroup-uniform, the
      // transforms contain barriers)
      int q = 12;
#pragma unroll
      for (int gg = 0; gg < G::ROWS; ++gg) {
        const int jj = it * G::ROWS + gg;
        if (jj < nj) q = min(q, static_cast<int>(prm_tab[jj].w));
      }
      cpx v[16];
      if constexpr (VAR == 1) {
        mother_filter<LOGN>(v, X, prm, a, t);
        fft_row<LOGN, 1, 1, TWL>(v, my, bufstride, tw, t, par, twl);
      } else {
        inverse_row<LOGN, 1, TWL>(v, X, prm, f0, q, my, bufstride, tw, t, par, twl);
      }
      // rows past the chunk (!valid) add nothing: zero weights, an empty range, no slot written
      const float4 w4 = (KB > 0 && valid) ? pw_tab[jl] : make_float4(0.f, 0.f, 0.f, 0.f);
      const int2 r = valid ? rng[jl] : make_int2(0, 0);
      const float w[4] = {w4.x, w4.y, w4.z, w4.w};
      float gs = 0.f;
      // (an opaque copy of t keeps the 16 positions from being hoisted out of the scale loop
      // as 16 live VGPRs, as in cwt.hip's store_row)
      int tt = t;
      asm volatile("" : "+v"(tt));
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const float p2 = cabs2(v[m]);
        const int pos = tt + m * P::NT;
        gs += (pos >= r.x && pos < r.y) ? p2 : 0.f;
#pragma unroll
        for (int k = 0; k < KB; ++k) ap[k][m] = fmaf(w[k], p2, ap[k][m]);
      }
      constexpr int W = P::NT < kWave ? P::NT : kWave;
#pragma unroll
      for (int o = 1; o < W; o <<= 1) gs += __shfl_xor(gs, o, W);
      if (valid && (rt & (W - 1)) == 0) gsum[jl * SG::WPR + rt / kWave] = gs;  // rt / 64: the wave within the row
    }
    __syncthreads();
    if (s.out_global) {
      for (int i = tid; i < nj; i += G::BLOCK) {
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < SG::WPR; ++w) sum += gsum[i * SG::WPR + w];
        const int2 r = rng[i];
        s.out_global[b * a.S + j0 + i] = sum / static_cast<float>(max(r.y - r.x, 0));
      }
    }
    if (KB > 0 && s.out_bp) emit_rows<LOGN, VAR>(ap, s.K, part ? wsb : s.out_bp + orow, a.n0, g, t, fbuf);
  }

  if (KB > 0 && s.out_bs) {
    float cs[KA][16];
#pragma unroll
    for (int k = 0; k < KA; ++k)
#pragma unroll
      for (int m = 0; m < 16; ++m) cs[k][m] = 0.f;
    for (int jl = g; jl < nj; jl += G::ROWS) {  // this row group's scales (no barrier inside)
      const float4 w4 = rw_tab[jl];
      if (w4.x == 0.f && w4.y == 0.f && w4.z == 0.f && w4.w == 0.f) continue;  // outside every band
      const float4 prm4 = prm_tab[jl];
      const float w[4] = {w4.x, w4.y, w4.z, w4.w};
      float psi[16];
      filter_gain<LOGN, VAR>(psi, mkc(prm4.x, prm4.y), a, f0, t);
#pragma unroll
      for (int k = 0; k < KB; ++k)
#pragma unroll
        for (int m = 0; m < 16; ++m) cs[k][m] = fmaf(w[k], psi[m], cs[k][m]);
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      if (k >= s.K) break;
      cpx v[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        v[m] = cscale(X[m], cs[k][m]);
        if constexpr (VAR == 1) v[m] = cmul(v[m], mkc(a.mcre, a.mcim));
      }
      fft_row<LOGN, 1, 1, TWL>(v, my, bufstride, tw, t, par, twl);
#pragma unroll
      for (int m = 0; m < 16; ++m) cs[k][m] = v[m].x;
    }
    emit_rows<LOGN, VAR>(cs, s.K, part ? wsb + static_cast<long long>(s.wsig) * a.n0 : s.out_bs + orow, a.n0,
                         g, t, fbuf);
  }
}

// out row (b, k) = sum over chunks, in chunk order, of the partial rows (one thread per sample;
// grid.z steps over the series, so any batch fits the grid).
__global__ void __launch_bounds__(256) sum_chunks_kernel(const float* ws, long long batch, int nchunks,
                                                         int wrows, int wsig, int n0, int kstride,
                                                         float* out_bp, float* out_bs) {
  const int tpos = blockIdx.x * 256 + threadIdx.x;
  const int r = blockIdx.y;  // partial row: power rows [0, wsig), signal rows [wsig, wrows)
  if (tpos >= n0) return;
  float* out = r < wsig ? out_bp : out_bs;
  const int k = r < wsig ? r : r - wsig;
  for (long long b = blockIdx.z; b < batch; b += gridDim.z) {
    const float* p = ws + (b * nchunks * wrows + r) * static_cast<long long>(n0) + tpos;
    float acc = 0.f;
    for (int c = 0; c < nchunks; ++c) acc += p[static_cast<long long>(c) * wrows * n0];
    out[(b * kstride + k) * static_cast<long long>(n0) + tpos] = acc;
  }
}

static int log2_ceil(long long n) {
  int l = 0;
  while ((1ll << l) < n) ++l;
  return l;
}

// Chunks per series and scales per chunk.  The CWT's rule (launch_fft_cwt) keeps 2048 workgroups
// in flight because each one waits on its own row stores; this kernel stores nothing per row, so
// a workgroup's start-up (tables, twiddles, forward FFT) and its per-band tail (one inverse FFT
// and one row pass per band and chunk) are what splitting costs.  A series is therefore split
// only until the launch has two workgroups per CU (512), never below 4 row iterations per
// workgroup, and a batch of 512 or more series gets one chunk per series: no workspace, no
// second kernel.  The signal-only launch has no scale loop: one chunk per MAXCHUNK scales
// (the size of the per-scale LDS tables).
static void summary_plan(long long batch, int logn, int S, bool pow, int& nch, int& chunk) {
  const int nt = (1 << logn) / 16;
  const int rows = nt >= 256 ? 1 : 256 / nt;
  const int kMaxChunk = logn >= 13 ? 64 : 128;  // SumGeom::MAXCHUNK
  long long want = 1;
  if (pow && batch < 512) want = (512 + batch - 1) / batch;
  const int max_chunks = (S + 4 * rows - 1) / (4 * rows);
  nch = static_cast<int>(want > max_chunks ? max_chunks : want);
  if (nch < 1) nch = 1;
  chunk = (S + nch - 1) / nch;
  chunk = ((chunk + rows - 1) / rows) * rows;
  if (chunk > kMaxChunk) chunk = kMaxChunk;
  nch = (S + chunk - 1) / chunk;
}

template <int LOGN, int KB, int VAR, bool POW>
static int launch_summary(const SumArgs& s, hipStream_t st) {
  static_assert(SumGeom<LOGN, VAR>::MAXCHUNK == (LOGN >= 13 ? 64 : 128), "summary_plan's chunk limit");
  const long long grid = s.c.batch * s.c.nchunks;
  if (grid > 0x7fffffffll) return kErrUnsupported;
  hipLaunchKernelGGL((cwt_summary_kernel<LOGN, KB, VAR, POW>), dim3(static_cast<unsigned>(grid)),
                     dim3(CwtGeom<LOGN, 0, VAR>::BLOCK), 0, st, s);
  return launch_status();
}

template <int LOGN, int VAR>
static int launch_kb(const SumArgs& s, bool pow, hipStream_t st) {
  constexpr int KM = sum_kb_max(LOGN);
  const int kb = s.K <= 2 ? s.K : 4;
  if (pow) {
    if (kb == 0) return launch_summary<LOGN, 0, VAR, true>(s, st);
    if constexpr (KM >= 2) {
      if (kb == 1) return launch_summary<LOGN, 1, VAR, true>(s, st);
      if (kb == 2) return launch_summary<LOGN, 2, VAR, true>(s, st);
      return launch_summary<LOGN, 4, VAR, true>(s, st);
    }
  } else {
    if (kb == 1) return launch_summary<LOGN, 1, VAR, false>(s, st);
    if constexpr (KM >= 2) {
      if (kb == 2) return launch_summary<LOGN, 2, VAR, false>(s, st);
      return launch_summary<LOGN, 4, VAR, false>(s, st);
    }
  }
  return kErrArg;
}

static int launch_logn(const SumArgs& s, int logn, bool pow, hipStream_t st) {
#define WTMI_CASE(L) \
  case L:            \
    return s.c.mother ? launch_kb<L, 1>(s, pow, st) : launch_kb<L, 0>(s, pow, st);
  switch (logn) {
    WTMI_CASE(4) WTMI_CASE(5) WTMI_CASE(6) WTMI_CASE(7) WTMI_CASE(8) WTMI_CASE(9)
    WTMI_CASE(10) WTMI_CASE(11) WTMI_CASE(12) WTMI_CASE(13) WTMI_CASE(14)
    default:
      return kErrUnsupported;
  }
#undef WTMI_CASE
}

// One launch per group of sum_kb_max bands (the global spectrum rides on the first), each followed
// by its chunk sum when the series are split.  N = 16384: the scale loop carries no band, so the
// global spectrum takes a launch of its own and the band signals follow one per launch.
static int run_summary(SumArgs s, int K, hipStream_t st) {
  const int logn = log2_ceil(s.c.n0);
  bool pow = s.out_global || s.out_bp;
  s.c.prune = s.c.mother ? 0 : options().cwt_prune;
  {  // every grid of this call fits (the scale-loop plan has the most chunks): checked before any launch
    int n1, c1;
    summary_plan(s.c.batch, logn, s.c.S, true, n1, c1);
    if (s.c.batch * n1 > 0x7fffffffll) return kErrUnsupported;
  }
  if (pow && K > 0 && logn >= 14) {
    if (s.out_bp) return kErrUnsupported;
    SumArgs gl = s;
    gl.K = gl.wrows = gl.wsig = 0;
    gl.pw = gl.rw = nullptr;
    gl.out_bs = nullptr;
    summary_plan(s.c.batch, logn, s.c.S, true, gl.c.nchunks, gl.c.chunk);
    const int rc = launch_logn(gl, logn, true, st);
    if (rc != kOk) return rc;
    s.out_global = nullptr;
    pow = false;
  }
  summary_plan(s.c.batch, logn, s.c.S, pow, s.c.nchunks, s.c.chunk);
  const bool part = s.c.nchunks > 1;
  const int kmax = sum_kb_max(logn);
  const double *pw = s.pw, *rw = s.rw;
  float *bp = s.out_bp, *bs = s.out_bs;
  for (int k0 = 0; k0 == 0 || k0 < K; k0 += kmax) {
    s.K = K - k0 < kmax ? K - k0 : kmax;
    s.pw = pw ? pw + static_cast<long long>(k0) * s.c.S : nullptr;
    s.rw = rw ? rw + static_cast<long long>(k0) * s.c.S : nullptr;
    s.out_bp = bp ? bp + static_cast<long long>(k0) * s.c.n0 : nullptr;
    s.out_bs = bs ? bs + static_cast<long long>(k0) * s.c.n0 : nullptr;
    s.wsig = s.out_bp ? s.K : 0;
    s.wrows = s.wsig + (s.out_bs ? s.K : 0);
    if (k0 > 0) s.out_global = nullptr;  // later groups: no global
    int rc = launch_logn(s, logn, s.out_global || s.out_bp, st);
    if (rc != kOk) return rc;
    if (part && s.wrows > 0) {
      const unsigned gz = static_cast<unsigned>(s.c.batch < 65535 ? s.c.batch : 65535);
      hipLaunchKernelGGL(sum_chunks_kernel, dim3((s.c.n0 + 255) / 256, s.wrows, gz), dim3(256), 0, st, s.ws,
                         s.c.batch, s.c.nchunks, s.wrows, s.wsig, s.c.n0, s.kstride, s.out_bp, s.out_bs);
      rc = launch_status();
      if (rc != kOk) return rc;
    }
  }
  return kOk;
}

}  // namespace wtmi

using namespace wtmi;

// Partial rows' bytes.  The chunk count falls as the batch grows (summary_plan), so the exact
// batch * nchunks is not monotone in the batch; while a series is split this returns the bound
// max(batch * ceil(S / MAXCHUNK), min(batch * max_chunks, 512 + batch)) on it, which is, and 0
// once every series is one chunk (no workspace is read then).
extern "C" long long wtmi_cwt_summary_workspace_bytes(long long batch, long long n0, int n_scales,
                                                      int n_bands) {
  if (batch <= 0 || n0 < 9 || n0 > (1 << 14) || n_scales <= 0 || n_bands <= 0) return 0;
  if (n_bands > kSumMaxBands) n_bands = kSumMaxBands;
  const int logn = log2_ceil(n0);
  int nch, nch2, chunk;
  summary_plan(batch, logn, n_scales, true, nch, chunk);
  summary_plan(batch, logn, n_scales, false, nch2, chunk);  // = ceil(S / MAXCHUNK) <= nch
  if (nch <= 1) return 0;
  const int nt = (1 << logn) / 16;
  const int rows = nt >= 256 ? 1 : 256 / nt;
  const long long max_chunks = (n_scales + 4 * rows - 1) / (4 * rows);
  long long wg = batch * max_chunks < 512 + batch ? batch * max_chunks : 512 + batch;
  if (batch * nch2 > wg) wg = batch * nch2;
  const int k = n_bands < sum_kb_max(logn) ? n_bands : sum_kb_max(logn);
  return wg * 2ll * k * n0 * static_cast<long long>(sizeof(float));
}

extern "C" int wtmi_cwt_summary(const float* x, long long ld, long long batch, long long n0,
                                const double* affine, const double* scales, int n_scales, double dt,
                                int mother, double param, const int* t_lo, const int* t_hi, int n_bands,
                                const double* power_w, const double* signal_w, float* out_global,
                                float* out_band_power, float* out_band_signal, void* workspace,
                                void* stream) {
  if (n0 < 0 || batch < 0 || n_scales < 0 || ld < n0) return kErrArg;
  if (n_bands < 0 || n_bands > kSumMaxBands) return kErrArg;
  if ((t_lo == nullptr) != (t_hi == nullptr)) return kErrArg;
  if (batch == 0 || n0 == 0 || n_scales == 0) return kOk;  // empty batch: no-op (NULL arrays allowed)
  if (!x || !scales) return kErrArg;
  if (!out_global && !out_band_power && !out_band_signal) return kErrArg;
  if ((out_band_power || out_band_signal) && n_bands == 0) return kErrArg;
  if ((out_band_power && !power_w) || (out_band_signal && !signal_w)) return kErrArg;
  SumArgs s{};
  if (!mother_consts(s.c, mother, param)) return kErrArg;
  if (n0 < 9 || n0 > (1 << 14)) return kErrUnsupported;  // direct / long rows: composed by the caller
  if (n0 > (1 << 13) && out_band_power) return kErrUnsupported;  // N = 16384: see SumGeom
  if (!workspace && wtmi_cwt_summary_workspace_bytes(batch, n0, n_scales, n_bands) > 0) return kErrArg;
  s.c.x = x;
  s.c.ld = ld;
  s.c.batch = batch;
  s.c.n0 = static_cast<int>(n0);
  s.c.S = n_scales;
  s.c.affine = affine;
  s.c.scales = scales;
  s.c.dt = dt;
  s.t_lo = t_lo;
  s.t_hi = t_hi;
  s.pw = out_band_power ? power_w : nullptr;
  s.rw = out_band_signal ? signal_w : nullptr;
  s.out_global = out_global;
  s.out_bp = out_band_power;
  s.out_bs = out_band_signal;
  s.ws = static_cast<float*>(workspace);
  s.kstride = n_bands;
  const int K = (out_band_power || out_band_signal) ? n_bands : 0;
  return run_summary(s, K, static_cast<hipStream_t>(stream));
}
