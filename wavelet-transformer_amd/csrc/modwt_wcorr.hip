// MODWT wavelet variance, covariance, correlation and lagged cross-correlation per scale
// (K22 of DESIGN.md): Percival & Walden ch. 8, Whitcher, Guttorp & Percival (2000) and the
// lead / lag analysis of Gencay, Selcuk & Whitcher ch. 7, in one launch.
//
// One workgroup per series or per (x, y) pair.  Both running smooths V_{j-1} stay in LDS
// across all J levels, as in K19, but this analysis needs the coefficients W_j themselves, so
// the level pass is the direct L-tap a-trous step (g~ = dec_lo / sqrt2, h~ = dec_hi / sqrt2,
// d = 2^(j-1)):
//   W_j[t] = sum_l h~[l] V_{j-1}[(t - d l) mod n],   V_j[t] = sum_l g~[l] V_{j-1}[(t - d l) mod n]
// Every LDS read of V_{j-1} feeds the h~ and the g~ FMA of its series.  W_j never goes to HBM.
//
// Tap pass: threads own samples (or float4 groups) at stride blockDim and keep V_j in
// registers; the lag-0 moments sum W^x W^x, W^x W^y, W^y W^y accumulate in fp64 from the
// registers, masked by t >= t0 (brick wall: t0 = L_j - 1 = (2^j - 1)(L - 1), the coefficients
// that never touch the wrap; periodic: t0 = 0).  One workgroup reduction per level ends the
// level's reads of V_{j-1}; V_j then overwrites it from registers (no second smooth buffer).
//
// Lag pass (max_lag = K > 0): the tap pass also leaves W^x_j and W^y_j in two further LDS rows
// (four rows of n floats, 128 KiB at n = 8192: one workgroup per CU, hence that limit).  The
// 2K + 1 lags are dealt to the waves round-robin; a lane carries up to eight of its wave's lags
// as fp64 accumulators and walks t at stride 64, so each lag's read of W^y[t + lag] is a run of
// 64 consecutive LDS words, and the one read of W^x[t] serves all eight.  One wave reduction per
// lag finishes the sum: no cross-wave reduction, no atomics.  Column K (lag 0) is the level's
// corr itself, from the same sums.
//
// The passes run on x - x[0] and y - y[0]: the fp32-rounded h~ does not sum to exactly 0, so a
// large mean would leak into the detail rows; a constant series gives W = 0 exactly.
#include "common.hpp"
#include "modwt_rows.hpp"
#include "ols.hpp"

// fp32 arithmetic of this file stays on the scalar VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace wtmi {

constexpr int kWcMaxN = 16384;     // two smooth rows: 128 KiB of LDS
constexpr int kWcMaxLagN = 8192;   // with the two coefficient rows beside them
constexpr int kWcMaxTaps = kModwtRowsMaxTaps;
constexpr int kWcMaxLag = 64;
constexpr int kWcMaxThreads = 1024;
constexpr int kWcMaxLevel = kModwtRowsMaxLevel;
constexpr int kWcLagsPerPass = 8;  // fp64 accumulators a lane carries through one walk over t

struct WcArgs {
  int n, level, L, periodic, max_lag;
  double z;
  float h[kWcMaxTaps];  // dec_hi / sqrt2
  float g[kWcMaxTaps];  // dec_lo / sqrt2
};

// What a level's epilogue and its lag pass share (the same values in every thread).
struct WcLevel {
  int t0;       // first coefficient that counts
  double M;     // n - t0
  double den;   // sqrt(var_x var_y); NaN where the correlations are undefined
  double corr;
};

// One stats row (thread 0): var_x, var_y, cov, corr, nobs, ci_lo, ci_hi, n_eff.
template <bool PAIR>
__device__ __forceinline__ WcLevel wc_level(const Mom3& m, const WcArgs& a, int j, int t0,
                                            double* __restrict__ row) {
  const double nan = __builtin_nan("");
  WcLevel lv{t0, static_cast<double>(a.n - t0), nan, nan};
  double vx = nan, vy = nan, cov = nan, neff = nan, nobs = 0.0;
  if (a.n - t0 > 0) {
    nobs = lv.M;
    vx = m.sxx / lv.M;
    const int sh = j < 31 ? j : 31;  // n < 2^31
    neff = static_cast<double>((a.n >> sh) - (a.periodic ? 0 : (a.L - 2) - ((a.L - 2) >> sh)));
    if (PAIR) {
      vy = m.syy / lv.M;
      cov = m.sxy / lv.M;
      if (vx != 0.0 && vy != 0.0) {
        lv.den = sqrt(vx * vy);
        lv.corr = cov / lv.den;
      }
    }
  }
  if (threadIdx.x == 0) {
    row[0] = vx;
    row[1] = vy;
    row[2] = cov;
    row[3] = lv.corr;
    row[4] = nobs;
    row[5] = nan;  // wc_intervals
    row[6] = nan;
    row[7] = neff;
  }
  return lv;
}

// Fisher intervals of a pair's rows, tanh(atanh(corr) -+ z / sqrt(n_eff - 3)), by the thread that
// wrote them, after the level loop: inside it the fp64 polynomial constants of atanh / tanh
// would be held in registers across every level's tap pass.
__device__ __forceinline__ void wc_intervals(double* __restrict__ rows, int J, double z) {
  if (threadIdx.x == 0) {
    for (int j = 0; j < J; ++j) {
      const double corr = rows[8 * j + 3], neff = rows[8 * j + 7];
      if (neff > 3.0 && corr == corr) {
        const double zr = atanh(corr), hw = z / sqrt(neff - 3.0);
        rows[8 * j + 5] = tanh(zr - hw);
        rows[8 * j + 6] = tanh(zr + hw);
      }
    }
  }
}

// rho_j(lag) for the 2K + 1 lags of one level from its coefficient rows in LDS.  Lag index
// i = lag + K goes to wave i mod nw; a wave takes its lags kWcLagsPerPass at a time.
__device__ __forceinline__ void lag_pass(const float* __restrict__ Wx, const float* __restrict__ Wy,
                                         const WcArgs& a, const WcLevel& lv, double* __restrict__ xrow) {
  constexpr int G = kWcLagsPerPass;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nw = blockDim.x / kWave;
  const int n = a.n, K = a.max_lag, nl = 2 * K + 1, t0 = lv.t0;
  for (int base = wave; base < nl; base += nw * G) {  // wave-uniform
    const int left = (nl - base + nw - 1) / nw;       // lags of this wave from base on
    const int cnt = left < G ? left : G;
    double acc[G];
#pragma unroll
    for (int i = 0; i < G; ++i) acc[i] = 0.0;
    for (int t = t0 + lane; t < n; t += kWave) {
      const double xv = static_cast<double>(Wx[t]);
#pragma unroll
      for (int i = 0; i < G; ++i) {
        if (i < cnt) {
          int q = t + base + i * nw - K;  // |lag| < n
          if (a.periodic) q = q < 0 ? q + n : (q >= n ? q - n : q);
          const bool ok = q >= t0 && q < n;  // brick wall: both ends clear of the wrap
          const float yv = Wy[ok ? q : t];
          acc[i] = fma(xv, ok ? static_cast<double>(yv) : 0.0, acc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
      if (i < cnt) {
        const double s = wave_sum(acc[i]);
        const int col = base + i * nw;
        if (lane == 0) xrow[col] = col == K ? lv.corr : s / lv.M / lv.den;  // NaN den: NaN row
      }
    }
  }
}

// first coefficient clear of the wrap at the next level: t0 += 2^(j-1) (L - 1), saturating at n
__device__ __forceinline__ void next_t0(const WcArgs& a, int& t0, int& dsat) {
  if (!a.periodic) {
    const int t = t0 + dsat * (a.L - 1);  // <= n + n (L - 1)
    t0 = t < a.n ? t : a.n;
  }
  dsat = 2 * dsat < a.n ? 2 * dsat : a.n;
}

// ---- K22, any n and any bank: threads own PER samples, stride blockDim -------------------
template <int PER, bool PAIR, bool LAGS>
__global__ void __launch_bounds__(kWcMaxThreads, PAIR || PER >= 16 ? 4 : 8)
modwt_wcorr_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ld, WcArgs a,
                   double* __restrict__ stats, double* __restrict__ xcorr) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ double red[3 * (kWcMaxThreads / kWave)];
  __shared__ int soff[kWcMaxTaps];
  constexpr int P = PAIR ? 2 : 1;
  const int tid = threadIdx.x, T = blockDim.x, n = a.n, J = a.level, L = a.L;
  const int np = (n + 3) & ~3;
  const long long b = blockIdx.x;
  float* V[2] = {sm, sm + np};
  float* W[2] = {sm + 2 * np, sm + 3 * np};  // LAGS only
#pragma unroll
  for (int s = 0; s < P; ++s) load_shifted((s == 0 ? x : y) + b * ld, V[s], n);
  int d = 1 % n, t0 = 0, dsat = 1;
  for (int j = 1; j <= J; ++j) {
    if (tid == 0) tap_offsets(d, n, L, soff);
    __syncthreads();  // V_{j-1} and the offsets are in place; the last level's lag pass is over
    next_t0(a, t0, dsat);
    float u[P][PER];
    Mom3 mom{0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < PER; ++kk) {
      int p = tid + kk * T;
      asm volatile("" : "+v"(p));  // one sample's taps at a time: no address math hoisted
      if (p < n) {
        float aw[P], av[P];
#pragma unroll
        for (int s = 0; s < P; ++s) aw[s] = av[s] = 0.f;
        for (int l = 0; l < L; ++l) {
          const int o = soff[l];
          const int q = p - o < 0 ? p - o + n : p - o;
          const float hl = a.h[l], gl = a.g[l];
#pragma unroll
          for (int s = 0; s < P; ++s) {
            const float v = V[s][q];
            aw[s] = fmaf(hl, v, aw[s]);
            av[s] = fmaf(gl, v, av[s]);
          }
        }
#pragma unroll
        for (int s = 0; s < P; ++s) {
          u[s][kk] = av[s];
          if (LAGS) W[s][p] = aw[s];
        }
        if (p >= t0) {
          const double dx = static_cast<double>(aw[0]);
          mom.sxx = fma(dx, dx, mom.sxx);
          if (PAIR) {
            const double dy = static_cast<double>(aw[P - 1]);
            mom.sxy = fma(dx, dy, mom.sxy);
            mom.syy = fma(dy, dy, mom.syy);
          }
        }
      }
    }
    mom = block_sum3(mom, red);  // its barrier ends this level's reads of V_{j-1}
#pragma unroll
    for (int kk = 0; kk < PER; ++kk) {
      const int p = tid + kk * T;
      if (p < n) {
#pragma unroll
        for (int s = 0; s < P; ++s) V[s][p] = u[s][kk];
      }
    }
    d = 2 * d >= n ? 2 * d - n : 2 * d;
    const WcLevel lv = wc_level<PAIR>(mom, a, j, t0, stats + (b * J + j - 1) * 8);
    if (LAGS) lag_pass(W[0], W[1], a, lv, xcorr + (b * J + j - 1) * (2 * a.max_lag + 1));
  }
  if (PAIR) wc_intervals(stats + b * J * 8, J, a.z);
}

// ---- K22, 8-tap banks (db4, sym4), n % 4 == 0, n >= 64 ------------------------------------
// Threads own float4 groups (stride blockDim).  From level 3 on the dilation is a whole number
// of groups, so each tap is one aligned 16-byte LDS read per series; levels 1 and 2 (d = 1, 2)
// form their taps from a register window of 3 / 5 aligned groups ending at the thread's own.
template <int DM>
__device__ __forceinline__ void window_taps(const float4* __restrict__ V4, int q, int ng, const WcArgs& a,
                                            float4& wv, float4& uv) {
  constexpr int HB = (7 * DM + 3) / 4;  // groups behind q that the taps t - 7 DM reach
  float f[4 * (HB + 1)];
  load_window<HB, 0>(V4, q, ng, f);
  float rw[4], ru[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rw[i] = ru[i] = 0.f;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      const float c = f[4 * HB + i - l * DM];
      rw[i] = fmaf(a.h[l], c, rw[i]);
      ru[i] = fmaf(a.g[l], c, ru[i]);
    }
  }
  wv = make_float4(rw[0], rw[1], rw[2], rw[3]);
  uv = make_float4(ru[0], ru[1], ru[2], ru[3]);
}

template <int GROUPS, bool PAIR, bool LAGS>
__global__ void __launch_bounds__(kWcMaxThreads, PAIR ? 4 : 8)
modwt_wcorr_vec_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ld, WcArgs a,
                       double* __restrict__ stats, double* __restrict__ xcorr) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ double red[3 * (kWcMaxThreads / kWave)];
  constexpr int P = PAIR ? 2 : 1;
  const int tid = threadIdx.x, T = blockDim.x, n = a.n, J = a.level, ng = a.n >> 2;
  const long long b = blockIdx.x;
  float* V[2] = {sm, sm + n};
  float* W[2] = {sm + 2 * n, sm + 3 * n};  // LAGS only
#pragma unroll
  for (int s = 0; s < P; ++s) load_shifted((s == 0 ? x : y) + b * ld, V[s], n);
  int d = 1, t0 = 0, dsat = 1;  // n >= 64
  for (int j = 1; j <= J; ++j) {
    __syncthreads();  // V_{j-1} is in place; the last level's lag pass is over
    next_t0(a, t0, dsat);
    int tl = tid;
    asm volatile("" : "+v"(tl));  // per-level copy: keeps the address math out of LICM
    int off[8];                   // (d l) mod n in groups (levels >= 3), by repeated addition
    off[0] = 0;
#pragma unroll
    for (int l = 1; l < 8; ++l) off[l] = off[l - 1] + (d >> 2) >= ng ? off[l - 1] + (d >> 2) - ng : off[l - 1] + (d >> 2);
    float4 u[P][GROUPS];
    Mom3 mom{0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < GROUPS; ++kk) {
      const bool own = tl + kk * T < ng;
      const int q = min(tl + kk * T, ng - 1);
      float4 wv[P];
#pragma unroll
      for (int s = 0; s < P; ++s) {
        const float4* V4 = reinterpret_cast<const float4*>(V[s]);
        if (j == 1) {
          window_taps<1>(V4, q, ng, a, wv[s], u[s][kk]);
        } else if (j == 2) {
          window_taps<2>(V4, q, ng, a, wv[s], u[s][kk]);
        } else {
          float4 aw = make_float4(0.f, 0.f, 0.f, 0.f), au = aw;
#pragma unroll
          for (int l = 0; l < 8; ++l) {
            const int qs = q - off[l] < 0 ? q - off[l] + ng : q - off[l];
            const float4 v = V4[qs];
            fma4(aw, a.h[l], v);
            fma4(au, a.g[l], v);
          }
          wv[s] = aw;
          u[s][kk] = au;
        }
        if (LAGS && own) reinterpret_cast<float4*>(W[s])[q] = wv[s];
      }
      const float4 e = wv[P - 1];
      mom_add<PAIR>(mom, wv[0].x, e.x, own && 4 * q >= t0);
      mom_add<PAIR>(mom, wv[0].y, e.y, own && 4 * q + 1 >= t0);
      mom_add<PAIR>(mom, wv[0].z, e.z, own && 4 * q + 2 >= t0);
      mom_add<PAIR>(mom, wv[0].w, e.w, own && 4 * q + 3 >= t0);
    }
    mom = block_sum3(mom, red);  // its barrier ends this level's reads of V_{j-1}
#pragma unroll
    for (int kk = 0; kk < GROUPS; ++kk) {
      const int q = tl + kk * T;
      if (q < ng) {
#pragma unroll
        for (int s = 0; s < P; ++s) reinterpret_cast<float4*>(V[s])[q] = u[s][kk];
      }
    }
    d = 2 * d >= n ? 2 * d - n : 2 * d;
    const WcLevel lv = wc_level<PAIR>(mom, a, j, t0, stats + (b * J + j - 1) * 8);
    if (LAGS) lag_pass(W[0], W[1], a, lv, xcorr + (b * J + j - 1) * (2 * a.max_lag + 1));
  }
  if (PAIR) wc_intervals(stats + b * J * 8, J, a.z);
}

}  // namespace wtmi

#pragma clang attribute pop

using namespace wtmi;

extern "C" int wtmi_modwt_wcorr(const float* x, const float* y, long long ld, long long batch, long long n,
                                const double* dec_lo, const double* dec_hi, int n_taps, int level,
                                int boundary, int max_lag, double z, double* stats, double* xcorr,
                                void* stream) {
  if (batch < 0 || n < 1 || ld < n || level < 1 || level > kWcMaxLevel || n_taps < 2) return kErrArg;
  if (!dec_lo || !dec_hi || (boundary != 0 && boundary != 1) || max_lag < 0 || max_lag >= n) return kErrArg;
  if ((max_lag > 0) != (xcorr != nullptr) && batch > 0) return kErrArg;
  if (n_taps > kWcMaxTaps || n > kWcMaxN || (max_lag > 0 && n > kWcMaxLagN) || max_lag > kWcMaxLag ||
      batch > 0x7fffffffll)
    return kErrUnsupported;
  if (batch == 0) return kOk;  // empty batch: no-op (NULL arrays allowed)
  if (!x || !stats || (!y && xcorr)) return kErrArg;
  WcArgs a{};
  a.n = static_cast<int>(n);
  a.level = level;
  a.L = n_taps;
  a.periodic = boundary == 0;
  a.max_lag = max_lag;
  a.z = z;
  scaled_bank(dec_lo, dec_hi, n_taps, a.h, a.g);
  const bool pair = y != nullptr, lags = max_lag > 0;
  const int ni = a.n, rows = lags ? 4 : (pair ? 2 : 1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto launch = [&](auto kernel, int threads, size_t lds) {
    allow_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(batch)), dim3(threads), lds, st, x, y, ld, a, stats,
                       xcorr);
  };
  // one geometry per size class, three kernels each: series, pair, pair with lags
  auto pick = [&](auto single, auto both, auto lagged, int threads, size_t lds) {
    if (lags) launch(lagged, threads, lds); else if (pair) launch(both, threads, lds); else launch(single, threads, lds);
  };
  if (n_taps == 8 && ni >= 64 && (ni & 3) == 0) {
    const size_t lds = static_cast<size_t>(rows) * ni * sizeof(float);
    const int ng = ni / 4;
    if (ng <= kWcMaxThreads)
      pick(modwt_wcorr_vec_kernel<1, false, false>, modwt_wcorr_vec_kernel<1, true, false>,
           modwt_wcorr_vec_kernel<1, true, true>, threads_for(ng, 1, kWcMaxThreads), lds);
    else if (ng <= 2 * kWcMaxThreads)
      pick(modwt_wcorr_vec_kernel<2, false, false>, modwt_wcorr_vec_kernel<2, true, false>,
           modwt_wcorr_vec_kernel<2, true, true>, threads_for(ng, 2, kWcMaxThreads), lds);
    else  // n > 8192: no lag rows
      pick(modwt_wcorr_vec_kernel<4, false, false>, modwt_wcorr_vec_kernel<4, true, false>,
           modwt_wcorr_vec_kernel<4, true, false>, threads_for(ng, 4, kWcMaxThreads), lds);
  } else {
    const size_t lds = static_cast<size_t>(rows) * ((ni + 3) & ~3) * sizeof(float);
    if (ni <= 4 * kWcMaxThreads)
      pick(modwt_wcorr_kernel<4, false, false>, modwt_wcorr_kernel<4, true, false>,
           modwt_wcorr_kernel<4, true, true>, threads_for(ni, 4, kWcMaxThreads), lds);
    else if (ni <= 8 * kWcMaxThreads)
      pick(modwt_wcorr_kernel<8, false, false>, modwt_wcorr_kernel<8, true, false>,
           modwt_wcorr_kernel<8, true, true>, threads_for(ni, 8, kWcMaxThreads), lds);
    else  // n > 8192: no lag rows
      pick(modwt_wcorr_kernel<16, false, false>, modwt_wcorr_kernel<16, true, false>,
           modwt_wcorr_kernel<16, true, false>, threads_for(ni, 16, kWcMaxThreads), lds);
  }
  return launch_status();
}
