// MODWT wavelet correlation matrix and wavelet multiple correlation per scale (K25 of
// DESIGN.md): the covariance / correlation matrix P_j of M series at every MODWT detail level
// (the by-scale form of a correlation table) and the wavelet multiple correlation of
// Fernandez-Macho (2012): R^2_i = 1 - 1 / (P_j^-1)_ii, phi_j = sqrt(max_i R^2_i), in one launch.
//
// One workgroup per group of M series.  The M running smooths V_{j-1} stay in LDS across all J
// levels (loaded as x - x[0], for K22's reason); the level pass is K22's direct L-tap a-trous
// step, but its sums are a dense contraction: G_j = W_j W_j^T, [M x n] . [n x M], fp64 sums of
// fp32 coefficients.  That is what v_mfma_f64_16x16x4_f64 does for 16 series and 4 samples, and
// because the product is a Gram matrix both operands of a lane are the SAME register.
//
// Operand / result layout of the instruction, established on an MI355X with a known 16 x 4
// integer matrix fed as both operands (256 of 256 accumulator entries matched A A^T):
//   lane l supplies A[l % 16][l / 16]            (row = l % 16, sample k = l / 16)
//   accumulator r of lane l is D[l / 16 + 4 r][l % 16],  r = 0 .. 3
// so D[i][j] sits in lane 16 (i % 4) + j, accumulator i / 4.
//
// Virtual rows.  Row v = l % 16 of the instruction is series a = v % M of time replica r = v / M,
// R = floor(16 / M) replicas (rows >= R M feed 0).  Time is cut into chunks of 4 samples; step
// g = (q, e), e < M, of the workgroup gives replica r the chunk c = R M q + r M + e (every chunk
// exactly once), lane l the sample t = 4 c + l / 16 of series a.  The matrix unit does the
// exchange: no lane ever needs another series' coefficient, so no coefficient row exists in
// LDS.  The wanted sum is that of the R diagonal M x M blocks of the 16 x 16 tile; the
// off-diagonal blocks (products across replicas) are discarded.
//
// Banks.  The row stride S is = 4 mod 64 words, so lane l's word of tap offset o is
// a S + 4 c + k - o = 4 (a + r M + e + R M q) + k - o: 4 v + k plus a wave-uniform term mod 64
// -- the 64 lanes hit 64 distinct banks at every tap, for every M (the replica's chunk offset
// r M is what makes that hold below M = 16).
//
// Level j: tap pass (a lane forms W_j and V_j of its samples, keeps V_j in registers, widens
// W_j masked by t >= t0 and t < n to fp64 and issues one MFMA per step); barrier (the reads of
// V_{j-1} are over, the row region is dead); every wave leaves its 16 x 16 tile in the row
// region; barrier; entry (a, b) adds the R diagonal-block entries of the waves' tiles in wave
// order (no floating-point atomics: equal inputs give equal bits; (a, b) and (b, a) read the
// same slots, so cov is symmetric bit for bit) and writes cov = G / M_j; barrier; V_j over
// V_{j-1} from registers.  After the level loop a wave per level turns cov into corr, factors
// P = L L^T in its 2 KiB tile slot of the (now dead) row region, inverts L (lane c forms column
// c of L^-1) and forms (P^-1)_cc = sum_k (L^-1)_kc^2, R^2, the maximum and its Fisher interval
// -- there, so that the fp64 constants of sqrt / tanh / atanh stay out of the tap pass, and in
// LDS with run-time loops: 16 x 16 fp64 in registers, fully unrolled, spilled 44 VGPRs.
#include "common.hpp"
#include "modwt_rows.hpp"

// fp32 arithmetic of this file stays on the scalar VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace wtmi {

constexpr int kWmMaxSeries = 16;      // rows of the fp64 16 x 16 x 4 matrix instruction
constexpr int kWmMaxSamples = 32768;  // M n: 128 KiB of smooth rows
constexpr int kWmMaxTaps = kModwtRowsMaxTaps;
constexpr int kWmMaxLevel = kModwtRowsMaxLevel;
constexpr int kWmMaxThreads = 1024;
constexpr int kWmTile = 256;  // doubles of one wave's tile

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct WmArgs {
  int n, level, L, periodic;
  int M, R, S;  // series, time replicas floor(16 / M), row stride in floats (= 4 mod 64)
  int steps;    // matrix steps of a wave per level, <= PER
  double z;
  float h[kWmMaxTaps];  // dec_hi / sqrt2
  float g[kWmMaxTaps];  // dec_lo / sqrt2
};

// slot of D[i][j] in a wave's tile, stored accumulator-major: tile[64 r + lane]
__device__ __forceinline__ int tile_slot(int i, int j) { return 64 * (i >> 2) + 16 * (i & 3) + j; }

// first coefficient clear of the wrap at level j (brick wall: (2^j - 1)(L - 1), at most n)
__device__ __forceinline__ int wm_t0(const WmArgs& a, int j) {
  if (a.periodic) return 0;
  if (j >= 31) return a.n;  // n < 2^31 <= 2^j - 1
  const long long t = ((1ll << j) - 1) * (a.L - 1);
  return t < a.n ? static_cast<int>(t) : a.n;
}

// Orders a wave's LDS writes before its other lanes' reads of them (the hardware runs one wave's
// LDS operations in issue order; this keeps the compiler from moving them across).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Rows of one level (a wave): corr from cov, then R^2, the multiple correlation and its interval.
// P: the wave's 16 x 16 fp64 scratch (its tile slot).  The factor L lands in the lower triangle,
// column c of L^-1 below its diagonal in row c's upper triangle (lane c alone touches it).
__device__ __forceinline__ void wm_level(const WmArgs& a, int j, const double* __restrict__ C,
                                         double* __restrict__ corr, double* __restrict__ r2,
                                         double* __restrict__ st, double* P) {
  constexpr int N = kWmMaxSeries;
  const double nan = __builtin_nan("");
  const int lane = threadIdx.x & (kWave - 1), M = a.M;
  const int t0 = wm_t0(a, j), Mj = a.n - t0;
  const int sh = j < 31 ? j : 31;
  const double neff = Mj > 0 ? static_cast<double>((a.n >> sh) - (a.periodic ? 0 : (a.L - 2) - ((a.L - 2) >> sh))) : nan;
  bool flat = false;  // a series without variance (or no coefficients at all)
  wave_sync();        // the wave's last level is done with P
  for (int p = lane; p < N * N; p += kWave) {
    const int ia = p >> 4, ib = p & (N - 1);
    if (ia < M && ib < M) {
      const double da = C[ia * M + ia], db = C[ib * M + ib];
      double v = C[ia * M + ib] / sqrt(da * db);  // 0 / 0 = NaN beside a constant series
      if (ia == ib) {
        v = da > 0.0 ? 1.0 : nan;
        flat = flat || !(da > 0.0);
      }
      P[p] = v;
      if (corr) corr[ia * M + ib] = v;
    }
  }
  if (!r2) return;
  bool ok = Mj >= M && !__any(flat);
  wave_sync();
  // P = L L^T, right-looking, lane (i, c0) = (lane % 16, lane / 16) updates columns c0 + 4 m of row i
  const int i = lane & (N - 1), c0 = lane >> 4;
  for (int k = 0; k < M; ++k) {  // wave-uniform
    const double piv = P[k * N + k];
    ok = ok && piv > 0.0;
    const double lk = sqrt(piv);
    wave_sync();
    if (lane < N && i >= k && i < M) P[i * N + k] = i == k ? lk : P[i * N + k] / lk;
    wave_sync();
    for (int c = c0; c <= i; c += 4)
      if (c > k && i < M) P[i * N + c] = fma(-P[i * N + k], P[c * N + k], P[i * N + c]);
    wave_sync();
  }
  // column c = lane of X = L^-1 by forward substitution; (P^-1)_cc = sum_k X[k][c]^2
  double pinv = nan;
  if (lane < M) {
    const int c = lane;
    const double xd = 1.0 / P[c * N + c];
    pinv = xd * xd;
    for (int k = c + 1; k < M; ++k) {
      double s = -P[k * N + c] * xd;
      for (int m = c + 1; m < k; ++m) s = fma(-P[k * N + m], P[c * N + m], s);
      const double xk = s / P[k * N + k];
      P[c * N + k] = xk;
      pinv = fma(xk, xk, pinv);
    }
  }
  const double r2i = ok ? 1.0 - 1.0 / pinv : nan;
  if (lane < M) r2[lane] = r2i;
  double best = nan, tgt = nan;
  for (int c = 0; c < M; ++c) {  // wave-uniform
    const double rc = __shfl(r2i, c);
    if (ok && !(rc <= best)) {  // the first maximum
      best = rc;
      tgt = static_cast<double>(c);
    }
  }
  if (lane == 0) {
    const double wmc = ok ? sqrt(best > 0.0 ? best : 0.0) : nan;
    double lo = nan, hi = nan;
    if (neff > 3.0 && wmc == wmc) {
      const double zr = atanh(wmc), hw = a.z / sqrt(neff - 3.0);
      lo = tanh(zr - hw);
      hi = tanh(zr + hw);
    }
    st[0] = wmc;
    st[1] = tgt;
    st[2] = lo;
    st[3] = hi;
    st[4] = Mj > 0 ? static_cast<double>(Mj) : 0.0;
    st[5] = neff;
  }
}

// ---- K25: a wave runs up to PER matrix steps per level, a lane keeps their V_j in registers ----
template <int PER>
__global__ void __launch_bounds__(kWmMaxThreads, 4)
modwt_wcmat_kernel(const float* __restrict__ x, long long ld, WmArgs a, double* cov,
                   double* __restrict__ corr, double* __restrict__ r2, double* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ int soff[kWmMaxTaps];
  const int tid = threadIdx.x, T = blockDim.x, n = a.n, J = a.level, L = a.L, M = a.M, S = a.S;
  const int lane = tid & (kWave - 1), wave = tid / kWave, nw = T / kWave;
  const long long b = blockIdx.x;
  const int v = lane & 15, k = lane >> 4;
  const int r = v / M, s = v - r * M, RM = a.R * M;
  const bool rowok = v < RM;
  float* Vs = sm + (rowok ? s : 0) * S;
  double* red = reinterpret_cast<double*>(sm);  // the waves' tiles, while the rows are dead
  for (int i = 0; i < M; ++i) load_shifted(x + (b * M + i) * ld, sm + i * S, n);
  // a wave's steps g = wave + kk nw as (q, e) = (g / M, g % M), advanced by (nw / M, nw % M)
  const int q0 = wave / M, e0 = wave - q0 * M, dq = nw / M, de = nw - dq * M;
  int d = 1 % n;
  for (int j = 1; j <= J; ++j) {
    if (tid == 0) tap_offsets(d, n, L, soff);
    __syncthreads();  // V_{j-1} and the offsets are in place
    const int t0 = wm_t0(a, j);
    float u[PER];
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    int q = q0, e = e0;
    asm volatile("" : "+v"(q), "+v"(e));  // per-level copies: no address math hoisted out of the level loop
#pragma unroll
    for (int kk = 0; kk < PER; ++kk) {
      if (kk < a.steps) {  // wave-uniform
        const int t = 4 * (RM * q + r * M + e) + k;
        const bool own = rowok && t < n;
        float aw = 0.f, av = 0.f;
        if (own) {
          for (int l = 0; l < L; ++l) {
            const int o = soff[l];
            const float val = Vs[t - o < 0 ? t - o + n : t - o];
            aw = fmaf(a.h[l], val, aw);
            av = fmaf(a.g[l], val, av);
          }
        }
        u[kk] = av;
        const double w = own && t >= t0 ? static_cast<double>(aw) : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(w, w, acc, 0, 0, 0);
        e += de;
        q += dq;
        if (e >= M) {
          e -= M;
          ++q;
        }
      }
    }
    __syncthreads();  // the reads of V_{j-1} are over: the row region is scratch
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave * kWmTile + 64 * i + lane] = acc[i];
    __syncthreads();
    const int Mj = n - t0;
    for (int p = tid; p < M * M; p += T) {
      const int ia = p / M, ib = p - ia * M;
      const int lo = ia < ib ? ia : ib, hi = ia < ib ? ib : ia;
      double sum = 0.0;
      for (int w = 0; w < nw; ++w)
        for (int rr = 0; rr < a.R; ++rr) sum += red[w * kWmTile + tile_slot(lo + rr * M, hi + rr * M)];
      cov[((b * J + j - 1) * M + ia) * M + ib] = Mj > 0 ? sum / Mj : __builtin_nan("");
    }
    __syncthreads();  // the tiles are read: V_j may land
    q = q0;
    e = e0;
#pragma unroll
    for (int kk = 0; kk < PER; ++kk) {
      if (kk < a.steps) {
        const int t = 4 * (RM * q + r * M + e) + k;
        if (rowok && t < n) Vs[t] = u[kk];
        e += de;
        q += dq;
        if (e >= M) {
          e -= M;
          ++q;
        }
      }
    }
    d = 2 * d >= n ? 2 * d - n : 2 * d;
  }
  if (!corr && !r2) return;
  __syncthreads();  // the workgroup's cov rows are written
  for (int j = wave; j < J; j += nw) {  // wave-uniform
    const long long lv = b * J + j;
    wm_level(a, j + 1, cov + lv * M * M, corr ? corr + lv * M * M : nullptr, r2 ? r2 + lv * M : nullptr,
             stats + lv * 6, red + wave * kWmTile);
  }
}

}  // namespace wtmi

#pragma clang attribute pop

using namespace wtmi;

extern "C" int wtmi_modwt_wcmat(const float* x, long long ld, long long batch, int n_series, long long n,
                                const double* dec_lo, const double* dec_hi, int n_taps, int level,
                                int boundary, double z, double* cov, double* corr, double* r2,
                                double* stats, void* stream) {
  if (batch < 0 || n < 1 || ld < n || n_series < 2 || level < 1 || level > kWmMaxLevel || n_taps < 2)
    return kErrArg;
  if (!dec_lo || !dec_hi || (boundary != 0 && boundary != 1) || (r2 != nullptr) != (stats != nullptr))
    return kErrArg;
  if (n_series > kWmMaxSeries || n_series * n > kWmMaxSamples || n_taps > kWmMaxTaps || batch > 0x7fffffffll)
    return kErrUnsupported;
  if (batch == 0) return kOk;  // empty batch: no-op (NULL arrays allowed)
  if (!x || !cov) return kErrArg;
  WmArgs a{};
  a.n = static_cast<int>(n);
  a.level = level;
  a.L = n_taps;
  a.periodic = boundary == 0;
  a.M = n_series;
  a.R = kWmMaxSeries / a.M;
  a.S = ((a.n > 4 ? a.n : 4) - 4 + 63) / 64 * 64 + 4;
  a.z = z;
  scaled_bank(dec_lo, dec_hi, n_taps, a.h, a.g);
  // matrix steps of the workgroup: M per R M chunks of 4 samples; dealt to at most 16 waves
  const int chunks = (a.n + 3) / 4, rm = a.R * a.M;
  const int total = a.M * ((chunks + rm - 1) / rm);  // <= 1024 at M n = 32768
  const int max_waves = kWmMaxThreads / kWave;
  a.steps = (total + max_waves - 1) / max_waves;
  const int waves = (total + a.steps - 1) / a.steps;
  const size_t rows = static_cast<size_t>(a.M) * a.S * sizeof(float), tiles = static_cast<size_t>(waves) * kWmTile * sizeof(double);
  const size_t lds = rows > tiles ? rows : tiles;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto launch = [&](auto kernel) {
    allow_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(batch)), dim3(waves * kWave), lds, st, x, ld, a, cov,
                       corr, r2, stats);
  };
  if (a.steps <= 4) launch(modwt_wcmat_kernel<4>);
  else if (a.steps <= 16) launch(modwt_wcmat_kernel<16>);
  else if (a.steps <= 32) launch(modwt_wcmat_kernel<32>);
  else launch(modwt_wcmat_kernel<64>);
  return launch_status();
}
