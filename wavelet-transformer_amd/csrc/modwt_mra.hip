// MODWT multiresolution analysis, smooths and per-row OLS (K19 / K20 of DESIGN.md).
//
// K19 replaces the MODWT workflow of src/modwt.py:466-487: modwt of an input and an output
// series (:126-144), modwtmra of each (:163-194), smooth_signal of each (:232-251) and
// time_scale_regression on the MRA rows (:197-229) -- one launch, one workgroup per series or
// per (input, output) pair, no coefficient array in HBM.
//
// Every MODWT operator is a circular convolution on Z/n, so analysis and synthesis commute and
// the MRA needs no synthesis cascade.  With g~ = dec_lo / sqrt2, h~ = dec_hi / sqrt2 and their
// autocorrelations r_g[m] = sum_l g~[l] g~[l + m], r_h likewise (2L - 1 taps, symmetric in m),
// U_0 = x and d = 2^(j-1) mod n:
//   D_j[t] = sum_m r_h[m] U_{j-1}[(t + d m) mod n]
//   U_j[t] = sum_m r_g[m] U_{j-1}[(t + d m) mod n]
// [D_1 .. D_J, S_J = U_J] is modwtmra(modwt(x)), and U_l is smooth_signal(...)[l]["signal"]
// for an orthonormal bank (r_g + r_h = delta): J passes instead of J + (J+1)(J+2)/2.
// The symmetry halves the multiplies (one tap per lag pair: r[m] (U[t + d m] + U[t - d m])),
// and the host drops the lags at which both autocorrelations vanish -- every even lag of an
// orthonormal bank, so db4 runs 4 lag pairs and the centre tap per sample and level.
//
// The fp32-rounded r_h does not sum to exactly 0, so a large mean would leak into the small
// detail rows: the passes run on x - x[0], and x[0] is added back to S_J and to the smooths (a
// constant series has D_j = 0 and S_J = the constant, exactly).
//
// The series stays in LDS across all J levels: read the taps -> barrier -> write U_j over
// U_{j-1} from registers (one LDS row per series, no second buffer).  D_j goes from registers
// straight to its HBM row.  Pair mode keeps both series in LDS, computes D_j of both at the
// same positions and feeds the fp64 moments of ols.hpp; one workgroup reduction and one stats
// row per level, then one for S_J.  With stats alone requested nothing else is written.
//
// Limits: a series of n <= kMraMaxN = 16384 samples (64 KiB of LDS; a pair takes two rows,
// 128 KiB of the CU's 160, so pairs of more than 8192 samples run one workgroup per CU and
// shorter ones two or more) and filters of 2 .. kMraMaxTaps = 40 taps; -2 beyond.
//
// K20 (wtmi_modwt_mra_rows) serves a caller who already holds coefficient rows, e.g. after
// thresholding them (the reference's modwtmra(w, filters)): one workgroup per (series, row)
// loads that one row, applies the h~ synthesis step of its level (g~ for row J) and the g~
// steps down to level 1.  The zero rows of the masked inverse are never read.
#include "common.hpp"
#include "modwt_rows.hpp"
#include "ols.hpp"

// fp32 arithmetic of this file stays on the scalar VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace wtmi {

constexpr int kMraMaxN = 16384;
constexpr int kMraMaxTaps = kModwtRowsMaxTaps;
constexpr int kMraMaxThreads = 1024;
constexpr int kMraMaxLevel = kModwtRowsMaxLevel;

struct MraArgs {
  int n, level, add_constant;
  int ntap;                   // lag pairs kept (m >= 1 with r_h[m] or r_g[m] non-zero)
  int mmax;                   // largest kept lag
  float h0, g0;               // r_h[0], r_g[0]
  int m[kMraMaxTaps - 1];     // kept lags, ascending
  float h[kMraMaxTaps - 1];   // r_h[m[t]]
  float g[kMraMaxTaps - 1];   // r_g[m[t]]
};

struct MraRowArgs {
  int n, level, L;
  float h[kMraMaxTaps];  // dec_hi / sqrt2
  float g[kMraMaxTaps];  // dec_lo / sqrt2
};

// Thread 0: offsets (d m) mod n of the kept lags, by repeated addition over the lags (d < n).
__device__ __forceinline__ void lag_offsets(const MraArgs& a, int d, int* __restrict__ soff) {
  if (threadIdx.x == 0) {
    int o = 0, t = 0;
    for (int m = 1; m <= a.mmax; ++m) {
      o += d;
      if (o >= a.n) o -= a.n;
      if (m == a.m[t]) soff[t++] = o;
    }
  }
}

// The S_J row: U_J + k to the last component row and, in pair mode, into the moments.
template <bool PAIR>
__device__ __forceinline__ void finish_rows(float* const* V, const float* k, float* const* comp,
                                            const MraArgs& a, double* __restrict__ srow, double* red) {
  const int n = a.n;
  Mom mom{0.0, 0.0, 0.0, 0.0, 0.0};
  for (int p = threadIdx.x; p < n; p += blockDim.x) {
    float v[2] = {0.f, 0.f};
#pragma unroll
    for (int s = 0; s < (PAIR ? 2 : 1); ++s) {
      v[s] = V[s][p] + k[s];
      if (comp[s]) comp[s][static_cast<long long>(a.level) * n + p] = v[s];
    }
    if (PAIR) mom.add(v[0], v[1], k[0], k[1]);
  }
  if (PAIR && srow) {
    mom = block_sum(mom, red);
    if (threadIdx.x == 0) ols_store(mom, k[0], k[1], static_cast<double>(n), a.add_constant, srow);
  }
}

// ---- K19, any n and any kept lags: threads own PER samples, stride blockDim ---------------
template <int PER, bool PAIR>
__global__ void __launch_bounds__(kMraMaxThreads)
modwt_mra_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ld, MraArgs a,
                 float* __restrict__ mra, float* __restrict__ smooth, double* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ double red[5 * (kMraMaxThreads / kWave)];
  __shared__ int soff[kMraMaxTaps];
  constexpr int P = PAIR ? 2 : 1;
  const int tid = threadIdx.x, T = blockDim.x, n = a.n, J = a.level;
  const long long b = blockIdx.x;
  float* V[2] = {sm, sm + ((n + 3) & ~3)};
  float* comp[2] = {nullptr, nullptr};
  float* smo[2] = {nullptr, nullptr};
  float k[2] = {0.f, 0.f};
#pragma unroll
  for (int s = 0; s < P; ++s) {
    k[s] = load_shifted((s == 0 ? x : y) + b * ld, V[s], n);
    if (mra) comp[s] = mra + (b * P + s) * static_cast<long long>(J + 1) * n;
    if (smooth) smo[s] = smooth + (b * P + s) * static_cast<long long>(J) * n;
  }
  int d = 1 % n;
  lag_offsets(a, d, soff);
  __syncthreads();
  const bool want_stats = PAIR && stats != nullptr;
  for (int j = 1; j <= J; ++j) {
    const long long row = static_cast<long long>(j - 1) * n;
    float u[P][PER];
    Mom mom{0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < PER; ++kk) {
      int p = tid + kk * T;
      asm volatile("" : "+v"(p));  // one sample's taps at a time: no address math hoisted (spills)
      if (p < n) {
        float ad[P], au[P];
#pragma unroll
        for (int s = 0; s < P; ++s) {
          const float c = V[s][p];
          ad[s] = a.h0 * c;
          au[s] = a.g0 * c;
        }
        for (int t = 0; t < a.ntap; ++t) {
          const int o = soff[t];
          const int ip = p + o >= n ? p + o - n : p + o;
          const int im = p - o < 0 ? p - o + n : p - o;
          const float ht = a.h[t], gt = a.g[t];
#pragma unroll
          for (int s = 0; s < P; ++s) {
            const float v = V[s][ip] + V[s][im];
            ad[s] = fmaf(ht, v, ad[s]);
            au[s] = fmaf(gt, v, au[s]);
          }
        }
#pragma unroll
        for (int s = 0; s < P; ++s) {
          u[s][kk] = au[s];
          if (comp[s]) comp[s][row + p] = ad[s];
          if (smo[s]) smo[s][row + p] = au[s] + k[s];
        }
        if (want_stats) mom.add(ad[0], ad[P - 1], 0.0, 0.0);
      }
    }
    if (want_stats) {  // its barrier also ends this level's LDS reads
      mom = block_sum(mom, red);
      if (tid == 0) ols_store(mom, 0.0, 0.0, static_cast<double>(n), a.add_constant, stats + (b * (J + 1) + j - 1) * 8);
    } else {
      __syncthreads();
    }
#pragma unroll
    for (int kk = 0; kk < PER; ++kk) {
      const int p = tid + kk * T;
      if (p < n) {
#pragma unroll
        for (int s = 0; s < P; ++s) V[s][p] = u[s][kk];
      }
    }
    d = 2 * d >= n ? 2 * d - n : 2 * d;
    lag_offsets(a, d, soff);
    __syncthreads();
  }
  finish_rows<PAIR>(V, k, comp, a, want_stats ? stats + (b * (J + 1) + J) * 8 : nullptr, red);
}

// ---- K19, orthonormal 8-tap banks (db4: lags 1, 3, 5, 7), n % 4 == 0 ----------------------
// Threads own float4 groups (stride blockDim).  From level 3 on the dilation is a whole number
// of groups, so each lag is one aligned 16-byte LDS read either side; levels 1 and 2 (d = 1, 2)
// form all their taps from a register window of 5 / 9 aligned groups.
template <int DM>
__device__ __forceinline__ void window_lags(const float4* __restrict__ V4, int q, int ng, const MraArgs& a,
                                            float4& dv, float4& uv) {
  constexpr int HB = (7 * DM + 3) / 4;  // groups either side that the lags +-7 DM reach
  float f[4 * (2 * HB + 1)];
  load_window<HB, HB>(V4, q, ng, f);
  float rd[4], ru[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float c = f[4 * HB + i];
    rd[i] = a.h0 * c;
    ru[i] = a.g0 * c;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float v = f[4 * HB + i + (2 * t + 1) * DM] + f[4 * HB + i - (2 * t + 1) * DM];
      rd[i] = fmaf(a.h[t], v, rd[i]);
      ru[i] = fmaf(a.g[t], v, ru[i]);
    }
  }
  dv = make_float4(rd[0], rd[1], rd[2], rd[3]);
  uv = make_float4(ru[0], ru[1], ru[2], ru[3]);
}

template <int GROUPS, bool PAIR>
__global__ void __launch_bounds__(kMraMaxThreads)
modwt_mra_vec_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ld, MraArgs a,
                     float* __restrict__ mra, float* __restrict__ smooth, double* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ double red[5 * (kMraMaxThreads / kWave)];
  constexpr int P = PAIR ? 2 : 1;
  const int tid = threadIdx.x, T = blockDim.x, n = a.n, J = a.level, ng = a.n >> 2;
  const long long b = blockIdx.x;
  float* V[2] = {sm, sm + n};
  float* comp[2] = {nullptr, nullptr};
  float* smo[2] = {nullptr, nullptr};
  float k[2] = {0.f, 0.f};
#pragma unroll
  for (int s = 0; s < P; ++s) {
    k[s] = load_shifted((s == 0 ? x : y) + b * ld, V[s], n);
    if (mra) comp[s] = mra + (b * P + s) * static_cast<long long>(J + 1) * n;
    if (smooth) smo[s] = smooth + (b * P + s) * static_cast<long long>(J) * n;
  }
  __syncthreads();
  const bool want_stats = PAIR && stats != nullptr;
  int d = 1;  // n >= 64
  for (int j = 1; j <= J; ++j) {
    const long long row = static_cast<long long>(j - 1) * n;
    int tl = tid;
    asm volatile("" : "+v"(tl));  // per-level copy: keeps the address math out of LICM
    int off[4];                   // lags 1, 3, 5, 7 in groups (levels >= 3), by repeated addition
    {
      const int dq = d >> 2, step = 2 * dq >= ng ? 2 * dq - ng : 2 * dq;
      off[0] = dq;
#pragma unroll
      for (int t = 1; t < 4; ++t) off[t] = off[t - 1] + step >= ng ? off[t - 1] + step - ng : off[t - 1] + step;
    }
    float4 u[P][GROUPS];
    Mom mom{0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < GROUPS; ++kk) {
      const bool own = tl + kk * T < ng;
      const int q = min(tl + kk * T, ng - 1);
      float4 dv[P];
#pragma unroll
      for (int s = 0; s < P; ++s) {
        const float4* V4 = reinterpret_cast<const float4*>(V[s]);
        if (d == 1) {
          window_lags<1>(V4, q, ng, a, dv[s], u[s][kk]);
        } else if (d == 2) {
          window_lags<2>(V4, q, ng, a, dv[s], u[s][kk]);
        } else {
          const float4 c = V4[q];
          float4 ad = make_float4(a.h0 * c.x, a.h0 * c.y, a.h0 * c.z, a.h0 * c.w);
          float4 au = make_float4(a.g0 * c.x, a.g0 * c.y, a.g0 * c.z, a.g0 * c.w);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int qp = q + off[t] >= ng ? q + off[t] - ng : q + off[t];
            const int qm = q - off[t] < 0 ? q - off[t] + ng : q - off[t];
            const float4 v = add4(V4[qp], V4[qm]);
            fma4(ad, a.h[t], v);
            fma4(au, a.g[t], v);
          }
          dv[s] = ad;
          u[s][kk] = au;
        }
        if (own) {
          if (comp[s]) reinterpret_cast<float4*>(comp[s] + row)[q] = dv[s];
          if (smo[s]) {
            const float4 w = u[s][kk];
            reinterpret_cast<float4*>(smo[s] + row)[q] = make_float4(w.x + k[s], w.y + k[s], w.z + k[s], w.w + k[s]);
          }
        }
      }
      if (want_stats && own) {
        const float4 e = PAIR ? dv[P - 1] : dv[0];
        mom.add(dv[0].x, e.x, 0.0, 0.0);
        mom.add(dv[0].y, e.y, 0.0, 0.0);
        mom.add(dv[0].z, e.z, 0.0, 0.0);
        mom.add(dv[0].w, e.w, 0.0, 0.0);
      }
    }
    if (want_stats) {  // its barrier also ends this level's LDS reads
      mom = block_sum(mom, red);
      if (tid == 0) ols_store(mom, 0.0, 0.0, static_cast<double>(n), a.add_constant, stats + (b * (J + 1) + j - 1) * 8);
    } else {
      __syncthreads();
    }
#pragma unroll
    for (int kk = 0; kk < GROUPS; ++kk) {
      const int q = tl + kk * T;
      if (q < ng) {
#pragma unroll
        for (int s = 0; s < P; ++s) reinterpret_cast<float4*>(V[s])[q] = u[s][kk];
      }
    }
    d = 2 * d >= n ? 2 * d - n : 2 * d;
    __syncthreads();
  }
  finish_rows<PAIR>(V, k, comp, a, want_stats ? stats + (b * (J + 1) + J) * 8 : nullptr, red);
}

// ---- K20: one MRA row from one coefficient row -------------------------------------------
template <int PER>
__global__ void __launch_bounds__(kMraMaxThreads)
modwt_mra_rows_kernel(const float* __restrict__ w, MraRowArgs a, float* __restrict__ mra) {
  extern __shared__ __attribute__((aligned(16))) float V[];
  __shared__ int soff[kMraMaxTaps];
  const int tid = threadIdx.x, T = blockDim.x, n = a.n, J = a.level;
  const long long b = blockIdx.x / (J + 1);
  const int r = static_cast<int>(blockIdx.x - b * (J + 1));
  const int jr = r < J ? r + 1 : J;  // the level this row was produced at
  const float* src = w + (b * (J + 1) + r) * static_cast<long long>(n);
  float* dst = mra + (b * (J + 1) + r) * static_cast<long long>(n);
#pragma unroll 4
  for (int i = tid; i < n; i += T) V[i] = src[i];
  for (int j = jr; j >= 1; --j) {
    const float* f = (j == jr && r < J) ? a.h : a.g;
    if (tid == 0) tap_offsets(static_cast<int>((1ll << (j - 1)) % n), n, a.L, soff);
    __syncthreads();
    float v[PER];
#pragma unroll
    for (int kk = 0; kk < PER; ++kk) {
      const int p = tid + kk * T;
      if (p < n) {
        float acc = 0.f;
        for (int l = 0; l < a.L; ++l) {
          const int q = p + soff[l];
          acc = fmaf(f[l], V[q >= n ? q - n : q], acc);
        }
        v[kk] = acc;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < PER; ++kk) {
      const int p = tid + kk * T;
      if (p < n) V[p] = v[kk];
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += T) dst[i] = V[i];
}

}  // namespace wtmi

#pragma clang attribute pop

using namespace wtmi;

extern "C" int wtmi_modwt_mra(const float* x, const float* y, long long ld, long long batch, long long n,
                              const double* dec_lo, const double* dec_hi, int n_taps, int level,
                              int add_constant, float* mra, float* smooth, double* stats, void* stream) {
  if (batch < 0 || n < 1 || ld < n || level < 1 || level > kMraMaxLevel || n_taps < 2) return kErrArg;
  if (!dec_lo || !dec_hi) return kErrArg;
  if (n > kMraMaxN || n_taps > kMraMaxTaps || batch > 0x7fffffffll) return kErrUnsupported;
  if (batch == 0) return kOk;  // empty batch: no-op (NULL arrays allowed)
  if (!x || (stats && !y) || (!mra && !smooth && !stats)) return kErrArg;
  MraArgs a{};
  a.n = static_cast<int>(n);
  a.level = level;
  a.add_constant = add_constant != 0;
  // autocorrelations of g~ = dec_lo / sqrt2 and h~ = dec_hi / sqrt2 in fp64, rounded once
  bool odd_only = true;
  for (int m = 0; m < n_taps; ++m) {
    double rh = 0.0, rg = 0.0;
    for (int l = 0; l + m < n_taps; ++l) {
      rh += dec_hi[l] * dec_hi[l + m];
      rg += dec_lo[l] * dec_lo[l + m];
    }
    rh *= 0.5;
    rg *= 0.5;
    if (m == 0) {
      a.h0 = static_cast<float>(rh);
      a.g0 = static_cast<float>(rg);
    } else if (fabs(rh) > 1e-12 || fabs(rg) > 1e-12) {  // an orthonormal bank's even lags are 0
      a.m[a.ntap] = m;
      a.h[a.ntap] = static_cast<float>(rh);
      a.g[a.ntap] = static_cast<float>(rg);
      ++a.ntap;
      a.mmax = m;
      odd_only = odd_only && (m & 1);
    }
  }
  const bool pair = y != nullptr;
  const int ni = a.n;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto launch = [&](auto kernel, int threads, size_t lds) {
    allow_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(batch)), dim3(threads), lds, st, x, y, ld, a, mra,
                       smooth, stats);
  };
  if (n_taps == 8 && odd_only && a.ntap == 4 && ni >= 64 && (ni & 3) == 0 && aligned16(mra) && aligned16(smooth)) {
    const size_t lds = static_cast<size_t>(pair ? 2 : 1) * ni * sizeof(float);
    const int ng = ni / 4;
    if (ng <= kMraMaxThreads) {
      const int t = threads_for(ng, 1, kMraMaxThreads);
      if (pair) launch(modwt_mra_vec_kernel<1, true>, t, lds); else launch(modwt_mra_vec_kernel<1, false>, t, lds);
    } else {
      const int t = threads_for(ng, 4, kMraMaxThreads);
      if (pair) launch(modwt_mra_vec_kernel<4, true>, t, lds); else launch(modwt_mra_vec_kernel<4, false>, t, lds);
    }
  } else {
    const size_t lds = static_cast<size_t>(pair ? 2 : 1) * ((ni + 3) & ~3) * sizeof(float);
    if (ni <= 4 * kMraMaxThreads) {
      const int t = threads_for(ni, 4, kMraMaxThreads);
      if (pair) launch(modwt_mra_kernel<4, true>, t, lds); else launch(modwt_mra_kernel<4, false>, t, lds);
    } else {
      const int t = threads_for(ni, 16, kMraMaxThreads);
      if (pair) launch(modwt_mra_kernel<16, true>, t, lds); else launch(modwt_mra_kernel<16, false>, t, lds);
    }
  }
  return launch_status();
}

extern "C" int wtmi_modwt_mra_rows(const float* w, long long batch, long long n, const double* dec_lo,
                                   const double* dec_hi, int n_taps, int level, float* mra, void* stream) {
  if (batch < 0 || n < 1 || level < 1 || level > kMraMaxLevel || n_taps < 2) return kErrArg;
  if (!dec_lo || !dec_hi) return kErrArg;
  if (n > kMraMaxN || n_taps > kMraMaxTaps || batch * (level + 1) > 0x7fffffffll) return kErrUnsupported;
  if (batch == 0) return kOk;  // empty batch: no-op (NULL arrays allowed)
  if (!w || !mra) return kErrArg;
  MraRowArgs a{};
  a.n = static_cast<int>(n);
  a.level = level;
  a.L = n_taps;
  scaled_bank(dec_lo, dec_hi, n_taps, a.h, a.g);
  const size_t lds = static_cast<size_t>((a.n + 3) & ~3) * sizeof(float);
  const unsigned grid = static_cast<unsigned>(batch * (level + 1));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.n <= 4 * kMraMaxThreads) {
    hipLaunchKernelGGL(modwt_mra_rows_kernel<4>, dim3(grid), dim3(threads_for(a.n, 4, kMraMaxThreads)), lds, st, w,
                       a, mra);
  } else {
    allow_lds(modwt_mra_rows_kernel<16>, lds);
    hipLaunchKernelGGL(modwt_mra_rows_kernel<16>, dim3(grid), dim3(threads_for(a.n, 16, kMraMaxThreads)), lds, st, w,
                       a, mra);
  }
  return launch_status();
}
