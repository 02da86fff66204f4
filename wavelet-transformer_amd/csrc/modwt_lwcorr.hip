// Time-localized (rolling-window) MODWT wavelet variance, covariance and correlation (K27 of
// DESIGN.md): the rolling wavelet correlation of Ranta (2010) and Gencay, Selcuk & Whitcher
// ch. 7, and its weighted form, the local wavelet correlation of Fernandez-Macho (2018), for one
// pair: a symmetric window theta(k), |k| <= H, slid over the coefficients W^x_j, W^y_j of every
// detail level, one correlation per level and time, in one launch.
//
// One workgroup per series or per (x, y) pair.  The level loop is K22's direct L-tap a-trous step
// (modwt_wcorr.hip): both running smooths V_{j-1} stay in LDS across all J levels, the tap pass
// keeps V_j in registers and leaves W^x_j and W^y_j in two further LDS rows; W never goes to HBM.
// The passes run on x - x[0] and y - y[0], as K22's.
//
// Coefficient rows with a halo.  A W row holds Hp + np + Hp floats (Hp = H and np = n rounded up
// to 4): sample t of the row is at Hp + t.  The tap pass stores 0 for t < t0 (brick wall: the
// coefficients that touch the wrap do not count); the halo and the pad hold 0 (brick wall, written
// once) or the row's own samples at (t mod n) (periodic, refreshed every level).  The window pass
// then reads every sample it needs, in range or not, from an aligned float4 group without a mask,
// a clamp or a branch: edges cost nothing in the inner loop, and a periodic row whose length is
// no multiple of 4 needs no second path.  At n = 8192, H = 1024 a pair takes 152 KiB of the CU's
// 160 KiB of LDS (four rows, two halos and the weights): one workgroup per CU, hence the limits.
//
// Window pass per level, O(n H) weighted fp64 sums.  A lane owns kLwR = 4 consecutive centres
// s0 .. s0 + 3 (s0 = 4 c, c at stride blockDim) and walks t over [s0 - Hp, s0 + 3 + Hp] one float4
// group of W^x and W^y at a time: lane c reads group c + m at step m, consecutive lanes read
// consecutive 16-byte groups (no bank conflict).  It forms the three products of a sample once,
// in fp64 from the fp32 coefficients (exact), and adds each to its four centres' accumulators
// with the weights theta(|t - s|).  The weight of centre s0 + r at step i is the weight of centre
// s0 at step i - r, so the lane keeps a sliding register window of four weights and reads ONE new
// weight per step from the float64 table in LDS; the table index is the same in every lane (a
// broadcast read), and its tail is padded with zeros so that the steps outside |k| <= H add 0.
// The sum of the counted weights Sw(s) is a fourth column: the "product" 1 where t counts, 0 where
// it does not.  Per sample and lane: 2 LDS values, 1 weight, 3 fp64 products, 16 fp64 FMAs.
// No atomics and no cross-lane reduction: equal inputs give equal bits.  A uniform window takes
// the same path.  The matrix instruction does not fit: the operand is a Toeplitz band against
// three product columns.
#include "common.hpp"
#include "modwt_rows.hpp"

// fp32 arithmetic of this file stays on the scalar VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace wtmi {

constexpr int kLwMaxN = 8192;
constexpr int kLwMaxTaps = kModwtRowsMaxTaps;
constexpr int kLwMaxLevel = kModwtRowsMaxLevel;
constexpr int kLwMaxHalf = 1024;
constexpr int kLwMaxThreads = 1024;
constexpr int kLwR = 4;  // centres per lane: one float4 of every output row

struct LwArgs {
  int n, level, L, periodic, H;
  float h[kLwMaxTaps];  // dec_hi / sqrt2
  float g[kLwMaxTaps];  // dec_lo / sqrt2
};

// Four consecutive outputs of one row: one 16-byte store where the row allows it.
__device__ __forceinline__ void store_centres(float* __restrict__ row, int s0, int n, bool vec,
                                              const float (&o)[kLwR]) {
  if (vec && s0 + kLwR <= n) {
    *reinterpret_cast<float4*>(row + s0) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int r = 0; r < kLwR; ++r)
      if (s0 + r < n) row[s0 + r] = o[r];
  }
}

// The window pass of one level.  Wx / Wy: the haloed coefficient rows; th: Hp + 4 weights, zero
// past H; [lo, hi]: the samples that count towards Sw (everything counts in the periodic mode);
// corr / mom: the level's output rows (mom: three planes ld_out apart), or NULL.
template <bool PAIR>
__device__ __forceinline__ void window_pass(const float* __restrict__ Wx, const float* __restrict__ Wy,
                                            const double* __restrict__ th, int n, int Hp, int lo, int hi,
                                            float* __restrict__ corr, float* __restrict__ mom,
                                            long long ld_out, bool vec) {
  const float4* X4 = reinterpret_cast<const float4*>(Wx);
  const float4* Y4 = reinterpret_cast<const float4*>(Wy);
  const int ngc = (n + kLwR - 1) / kLwR, steps = Hp / 2 + 1;  // float4 groups of [s0 - Hp, s0 + 3 + Hp]
  for (int c = threadIdx.x; c < ngc; c += blockDim.x) {
    const int s0 = kLwR * c;
    double axx[kLwR], ayy[kLwR], axy[kLwR], sw[kLwR];
#pragma unroll
    for (int r = 0; r < kLwR; ++r) axx[r] = ayy[r] = axy[r] = sw[r] = 0.0;
    double w1 = 0.0, w2 = 0.0, w3 = 0.0;  // the weights of centres s0 + 1 .. s0 + 3 (steps i - 1 .. i - 3)
    for (int m = 0; m < steps; ++m) {      // the same trip count and table index in every lane
      const float4 xv = X4[c + m];
      const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
      float ys[4] = {0.f, 0.f, 0.f, 0.f};
      if (PAIR) {
        const float4 yv = Y4[c + m];
        ys[0] = yv.x; ys[1] = yv.y; ys[2] = yv.z; ys[3] = yv.w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 4 * m + e - Hp, t = s0 + k;  // k: the offset from centre s0
        const double w0 = th[k < 0 ? -k : k];
        const double dx = static_cast<double>(xs[e]), pm = t >= lo && t <= hi ? 1.0 : 0.0;
        const double pxx = dx * dx;
        axx[0] = fma(w0, pxx, axx[0]); axx[1] = fma(w1, pxx, axx[1]);
        axx[2] = fma(w2, pxx, axx[2]); axx[3] = fma(w3, pxx, axx[3]);
        sw[0] = fma(w0, pm, sw[0]); sw[1] = fma(w1, pm, sw[1]);
        sw[2] = fma(w2, pm, sw[2]); sw[3] = fma(w3, pm, sw[3]);
        if (PAIR) {
          const double dy = static_cast<double>(ys[e]);
          const double pyy = dy * dy, pxy = dx * dy;
          ayy[0] = fma(w0, pyy, ayy[0]); ayy[1] = fma(w1, pyy, ayy[1]);
          ayy[2] = fma(w2, pyy, ayy[2]); ayy[3] = fma(w3, pyy, ayy[3]);
          axy[0] = fma(w0, pxy, axy[0]); axy[1] = fma(w1, pxy, axy[1]);
          axy[2] = fma(w2, pxy, axy[2]); axy[3] = fma(w3, pxy, axy[3]);
        }
        w3 = w2; w2 = w1; w1 = w0;
      }
    }
    const float nanf = __builtin_nanf("");
    float oc[kLwR], ox[kLwR], oy[kLwR], ov[kLwR];
#pragma unroll
    for (int r = 0; r < kLwR; ++r) {
      oc[r] = ox[r] = oy[r] = ov[r] = nanf;
      if (sw[r] != 0.0) {  // a window without a counted coefficient: NaN
        ox[r] = static_cast<float>(axx[r] / sw[r]);
        if (PAIR) {
          oy[r] = static_cast<float>(ayy[r] / sw[r]);
          ov[r] = static_cast<float>(axy[r] / sw[r]);
          if (axx[r] != 0.0 && ayy[r] != 0.0) {  // a window without energy in x or y: NaN
            const double rho = axy[r] / sqrt(axx[r] * ayy[r]);
            oc[r] = static_cast<float>(fmin(fmax(rho, -1.0), 1.0));
          }
        }
      }
    }
    if (mom) {
      store_centres(mom, s0, n, vec, ox);
      if (PAIR) {
        store_centres(mom + ld_out, s0, n, vec, oy);
        store_centres(mom + 2 * ld_out, s0, n, vec, ov);
      }
    }
    if (PAIR && corr) store_centres(corr, s0, n, vec, oc);
  }
}

// ---- K27: threads own PER samples of the tap pass at stride blockDim, any n and any bank ------
template <int PER, bool PAIR>
__global__ void __launch_bounds__(kLwMaxThreads)
modwt_lwcorr_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ld, LwArgs a,
                    const double* __restrict__ window, float* __restrict__ corr,
                    float* __restrict__ moments, long long ld_out) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ int soff[kLwMaxTaps];
  constexpr int P = PAIR ? 2 : 1;
  const int tid = threadIdx.x, T = blockDim.x, n = a.n, J = a.level, L = a.L;
  const int np = (n + 3) & ~3, Hp = (a.H + 3) & ~3, ne = np + 2 * Hp;
  const long long b = blockIdx.x;
  float* V[2] = {sm, sm + (P - 1) * np};
  float* W[2] = {sm + P * np, sm + P * np + (P - 1) * ne};
  double* th = reinterpret_cast<double*>(sm + P * (np + ne));  // Hp + 4 weights
#pragma unroll
  for (int s = 0; s < P; ++s) load_shifted((s == 0 ? x : y) + b * ld, V[s], n);
  for (int k = tid; k < Hp + 4; k += T) th[k] = k <= a.H ? window[k] : 0.0;
  // halo [-Hp, 0) and [n, np + Hp) of both rows: zeros for the brick wall, once
  const int nh = 2 * Hp + np - n;
  if (!a.periodic) {
    for (int e = tid; e < nh; e += T) {
      const int q = e < Hp ? e : e + n;
#pragma unroll
      for (int s = 0; s < P; ++s) W[s][q] = 0.f;
    }
  }
  const bool vec = (ld_out & 3) == 0 && aligned16(corr) && aligned16(moments);
  int d = 1 % n, t0 = 0, dsat = 1;
  for (int j = 1; j <= J; ++j) {
    if (tid == 0) tap_offsets(d, n, L, soff);
    __syncthreads();  // V_{j-1} and the offsets are in place; the last level's window pass is over
    if (!a.periodic) {  // first coefficient clear of the wrap: t0 += 2^(j-1) (L - 1), saturating at n
      const int t = t0 + dsat * (L - 1);  // <= n + n (L - 1)
      t0 = t < n ? t : n;
    }
    dsat = 2 * dsat < n ? 2 * dsat : n;
    float u[P][PER];
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
          W[s][Hp + p] = p >= t0 ? aw[s] : 0.f;
        }
      }
    }
    __syncthreads();  // this level's reads of V_{j-1} are over; W_j is complete
#pragma unroll
    for (int kk = 0; kk < PER; ++kk) {
      const int p = tid + kk * T;
      if (p < n) {
#pragma unroll
        for (int s = 0; s < P; ++s) V[s][p] = u[s][kk];
      }
    }
    if (a.periodic) {  // the halo wraps: sample t of it is the row's sample t mod n
      for (int e = tid; e < nh; e += T) {
        const int q = e < Hp ? e : e + n;
        int t = (q - Hp) % n;
        t = t < 0 ? t + n : t;
#pragma unroll
        for (int s = 0; s < P; ++s) W[s][q] = W[s][Hp + t];
      }
      __syncthreads();
    }
    d = 2 * d >= n ? 2 * d - n : 2 * d;
    const long long row = b * J + j - 1;
    window_pass<PAIR>(W[0], W[1], th, n, Hp, a.periodic ? -0x40000000 : t0, a.periodic ? 0x40000000 : n - 1,
                      corr ? corr + row * ld_out : nullptr, moments ? moments + row * 3 * ld_out : nullptr,
                      ld_out, vec);
  }
}

}  // namespace wtmi

#pragma clang attribute pop

using namespace wtmi;

extern "C" int wtmi_modwt_lwcorr(const float* x, const float* y, long long ld, long long batch, long long n,
                                 const double* dec_lo, const double* dec_hi, int n_taps, int level,
                                 int boundary, const double* window, int half_width, float* corr,
                                 float* moments, long long ld_out, void* stream) {
  if (batch < 0 || n < 1 || ld < n || ld_out < n || level < 1 || level > kLwMaxLevel || n_taps < 2) return kErrArg;
  if (!dec_lo || !dec_hi || !window || (boundary != 0 && boundary != 1) || half_width < 0) return kErrArg;
  if (boundary == 0 && 2ll * half_width + 1 > n) return kErrArg;  // a coefficient would count twice
  if ((!corr && !moments) || (corr && !y)) return kErrArg;
  if (n_taps > kLwMaxTaps || n > kLwMaxN || half_width > kLwMaxHalf || batch > 0x7fffffffll) return kErrUnsupported;
  if (batch == 0) return kOk;  // empty batch: no-op
  if (!x) return kErrArg;
  LwArgs a{};
  a.n = static_cast<int>(n);
  a.level = level;
  a.L = n_taps;
  a.periodic = boundary == 0;
  a.H = half_width;
  scaled_bank(dec_lo, dec_hi, n_taps, a.h, a.g);
  const bool pair = y != nullptr;
  const int ni = a.n, np = (ni + 3) & ~3, Hp = (half_width + 3) & ~3, P = pair ? 2 : 1;
  const size_t lds = static_cast<size_t>(P) * (2 * np + 2 * Hp) * sizeof(float) + (Hp + 4) * sizeof(double);
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto launch = [&](auto kernel, int per) {
    allow_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(batch)), dim3(threads_for(ni, per, kLwMaxThreads)), lds,
                       st, x, y, ld, a, window, corr, moments, ld_out);
  };
  if (ni <= 4 * kLwMaxThreads) {
    if (pair) launch(modwt_lwcorr_kernel<4, true>, 4); else launch(modwt_lwcorr_kernel<4, false>, 4);
  } else {
    if (pair) launch(modwt_lwcorr_kernel<8, true>, 8); else launch(modwt_lwcorr_kernel<8, false>, 8);
  }
  return launch_status();
}
