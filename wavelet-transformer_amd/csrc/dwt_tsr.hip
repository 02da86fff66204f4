// Time-scale regression on DWT components (K17 / K18 of DESIGN.md).
//
// Replaces the numeric path of time_scale_regression (src/regression.py:91-126): pywt.wavedec
// (mode "symmetric") of an input and an output series, the level + 1 single-array
// reconstructions of each (reconstruct_signal_component, src/dwt.py:110-120) and the OLS of
// output component on [1, input component] per array -- in ONE launch, one workgroup per
// (pair, component).  A component-k workgroup analyses only as deep as its array lies (D_j: j
// levels, S_J: J), keeps one approximation ping-pong and the one array it reconstructs from,
// and runs the synthesis in polyphase form on that single array (the other arrays are zero):
//   analysis : c[i] = sum_{p<F/2} f[2p] xe[2i+1-2p] + f[2p+1] xe[2i-2p]     (one filter per level)
//   synthesis: y[2u] = sum_{w<F/2} c[u+w] f[F-2-2w],  y[2u+1] = sum_w c[u+w] f[F-1-2w]
// Every level row lives in LDS with its symmetric extension written out once per level, so the
// tap loops are straight reads.  The last synthesis step of both series is computed per thread
// from the two penultimate rows and feeds the fp64 moments directly; the final rows never
// touch LDS.  rows_ols_kernel (K18) regresses row pairs that already exist (MODWT MRA rows,
// src/modwt.py:197-229, and the composed path of series longer than kTsrMaxN) with the same
// accumulators and the same epilogue.
#include "common.hpp"
#include "dwt_rows.hpp"
#include "ols.hpp"

// fp32 arithmetic of this file stays on the scalar VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace wtmi {

constexpr int kTsrMaxTaps = kPyrMaxTaps;
constexpr int kTsrMaxN = 8192;       // 2 n floats of LDS: two workgroups per CU
constexpr int kTsrMaxThreads = 512;
constexpr int kTsrMaxLevel = kPyrMaxLevel;
constexpr int kOlsThreads = 256;

enum : int { kDecLo = 0, kDecHi = 1, kRecLo = 2, kRecHi = 3 };

struct TsrArgs {
  int F, level, add_constant, out_len;
  int len[kTsrMaxLevel + 1];  // len[0] = n, len[j] = len(cD_j) = (len[j-1] + F - 1) / 2
  float taps[4][kTsrMaxTaps];  // dec_lo, dec_hi, rec_lo, rec_hi: only the first F of each are read
};

// ---- K17: fused analysis / single-array synthesis / regression ---------------------------
__global__ void __launch_bounds__(kTsrMaxThreads)
dwt_tsr_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ld, TsrArgs a,
               double* __restrict__ stats, float* __restrict__ comps, int ext, int cap0, int cap1) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ double red[5 * (kTsrMaxThreads / kWave)];
  const int tid = threadIdx.x, T = blockDim.x;
  const int F = a.F, H = a.F / 2, n = a.len[0], ncomp = a.level + 1;
  const long long b = blockIdx.x / ncomp;
  const int kc = static_cast<int>(blockIdx.x - b * ncomp);  // pywt list index: 0 = cA_J, k = cD_{J-k+1}
  const bool detail = kc > 0;
  const int jt = detail ? a.level - kc + 1 : a.level;  // levels this component needs
  const float* gx = x + b * ld;
  const float* gy = y + b * ld;
  float* cx = comps ? comps + ((b * 2 + 0) * ncomp + kc) * static_cast<long long>(a.out_len) : nullptr;
  float* cy = comps ? comps + ((b * 2 + 1) * ncomp + kc) * static_cast<long long>(a.out_len) : nullptr;
  Mom mom{0.0, 0.0, 0.0, 0.0, 0.0};
  double kx, ky;

  if (jt == 0) {  // level 0: the only component is the series itself
    kx = gx[0];
    ky = gy[0];
    for (int i = tid; i < n; i += T) {
      const float vx = gx[i], vy = gy[i];
      mom.add(vx, vy, kx, ky);
      if (comps) {
        cx[i] = vx;
        cy[i] = vy;
      }
    }
  } else {
    // rows start `ext` floats into their region: F - 2 extension samples before, F - 1 after
    float* const R0 = sm + ext;                // level input (n) and one side of the ping-pong
    float* const R1 = sm + cap0 + ext;         // the other side (<= len[1] + 1)
    float* const R2 = sm + cap0 + cap1 + ext;  // penultimate row of the input series
    const float* pen[2] = {nullptr, nullptr};
    bool prev_small = false;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
      const float* g = s == 0 ? gx : gy;
      float* cur = R0;
      step_sync(prev_small, false);  // the other series' last step has read R0 / R1
      load_row(cur, g, n);
      // analysis: approximations down to level jt, where the component's own array is kept
      for (int j = 1; j <= jt; ++j) {
        const int m = a.len[j - 1], M = a.len[j];
        const bool small = M <= kWave;
        step_sync(prev_small, small);
        extend_row(cur, m, F, small ? kWave : T);
        step_sync(prev_small, small);
        float* dst = (s == 0 && jt == 1) ? R2 : (cur == R0 ? R1 : R0);
        const int bank = (j == jt && detail) ? kDecHi : kDecLo;
        for (int i = tid; i < M; i += T) {
          const float2* p2 = reinterpret_cast<const float2*>(cur + 2 * i);  // (xe[2i], xe[2i+1])
          float acc = 0.f;
          for (int p = 0; p < H; ++p) {
            const float2 v = p2[-p];
            acc = fmaf(a.taps[bank][2 * p], v.y, acc);
            acc = fmaf(a.taps[bank][2 * p + 1], v.x, acc);
          }
          dst[i] = acc;
        }
        cur = dst;
      }
      // synthesis down to the penultimate row: rec_hi on the first step of a detail array,
      // rec_lo on every other one (the other input of each step is zero)
      for (int j = jt; j >= 2; --j) {
        const int P = a.len[j] - H + 1;  // output pairs: 2 P = 2 len[j] - F + 2 samples
        const bool small = P <= kWave;
        step_sync(prev_small, small);
        float* dst = (s == 0 && j == 2) ? R2 : (cur == R0 ? R1 : R0);
        const int bank = (j == jt && detail) ? kRecHi : kRecLo;
        for (int u = tid; u < P; u += T) {
          float ye = 0.f, yo = 0.f;
          for (int w = 0; w < H; ++w) {
            const float c = cur[u + w];
            ye = fmaf(c, a.taps[bank][F - 2 - 2 * w], ye);
            yo = fmaf(c, a.taps[bank][F - 1 - 2 * w], yo);
          }
          *reinterpret_cast<float2*>(dst + 2 * u) = make_float2(ye, yo);
        }
        cur = dst;
      }
      if (s == 0) pen[0] = cur; else pen[1] = cur;
    }
    __syncthreads();
    // last synthesis step of both series in registers, straight into the moments
    const float* px = pen[0];
    const float* py = pen[1];
    const int P = a.len[1] - H + 1;
    const int bank = (jt == 1 && detail) ? kRecHi : kRecLo;
    {
      float x0 = 0.f, y0 = 0.f;  // sample 0 of both components: the moments' shift
      for (int w = 0; w < H; ++w) {
        x0 = fmaf(px[w], a.taps[bank][F - 2 - 2 * w], x0);
        y0 = fmaf(py[w], a.taps[bank][F - 2 - 2 * w], y0);
      }
      kx = x0;
      ky = y0;
    }
    for (int u = tid; u < P; u += T) {
      float xe = 0.f, xo = 0.f, ye = 0.f, yo = 0.f;
      for (int w = 0; w < H; ++w) {
        const float fe = a.taps[bank][F - 2 - 2 * w], fo = a.taps[bank][F - 1 - 2 * w];
        const float vx = px[u + w], vy = py[u + w];
        xe = fmaf(vx, fe, xe);
        xo = fmaf(vx, fo, xo);
        ye = fmaf(vy, fe, ye);
        yo = fmaf(vy, fo, yo);
      }
      mom.add(xe, ye, kx, ky);
      mom.add(xo, yo, kx, ky);
      if (comps) {  // out_len is even here and comps 8-byte aligned (checked by the host)
        *reinterpret_cast<float2*>(cx + 2 * u) = make_float2(xe, xo);
        *reinterpret_cast<float2*>(cy + 2 * u) = make_float2(ye, yo);
      }
    }
  }
  mom = block_sum(mom, red);
  if (tid == 0)
    ols_store(mom, kx, ky, static_cast<double>(a.out_len), a.add_constant,
              stats + (b * ncomp + kc) * 8);
}

// ---- K18: OLS of existing row pairs -------------------------------------------------------
// WAVE_ROW: one wave per row (four rows per workgroup, no barrier); else one workgroup per row.
template <bool WAVE_ROW>
__global__ void __launch_bounds__(kOlsThreads)
rows_ols_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ld, long long rows,
                long long n, int add_constant, double* __restrict__ stats) {
  __shared__ double red[5 * (kOlsThreads / kWave)];
  const int t = WAVE_ROW ? threadIdx.x & (kWave - 1) : threadIdx.x;
  constexpr int T = WAVE_ROW ? kWave : kOlsThreads;
  const long long row = WAVE_ROW ? blockIdx.x * static_cast<long long>(kOlsThreads / kWave) + threadIdx.x / kWave
                                 : static_cast<long long>(blockIdx.x);
  if (WAVE_ROW && row >= rows) return;
  const float* xr = x + row * ld;
  const float* yr = y + row * ld;
  const double kx = xr[0], ky = yr[0];
  Mom m{0.0, 0.0, 0.0, 0.0, 0.0};
  long long done = 0;
  if (aligned16(xr) && aligned16(yr)) {
    const long long n4 = n >> 2;
#pragma unroll 2
    for (long long i = t; i < n4; i += T) {
      const float4 vx = reinterpret_cast<const float4*>(xr)[i];
      const float4 vy = reinterpret_cast<const float4*>(yr)[i];
      m.add(vx.x, vy.x, kx, ky);
      m.add(vx.y, vy.y, kx, ky);
      m.add(vx.z, vy.z, kx, ky);
      m.add(vx.w, vy.w, kx, ky);
    }
    done = 4 * n4;
  }
  for (long long i = done + t; i < n; i += T) m.add(xr[i], yr[i], kx, ky);
  if (WAVE_ROW) {
    m = wave_sum(m);
  } else {
    m = block_sum(m, red);
  }
  if (t == 0) ols_store(m, kx, ky, static_cast<double>(n), add_constant, stats + row * 8);
}

}  // namespace wtmi

#pragma clang attribute pop

using namespace wtmi;

extern "C" int wtmi_dwt_tsr(const float* x, const float* y, long long ld, long long batch, long long n,
                            const double* dec_lo, const double* dec_hi, const double* rec_lo,
                            const double* rec_hi, int n_taps, int level, int add_constant,
                            double* stats, float* comps, void* stream) {
  if (batch < 0 || n < 1 || ld < n || level < 0 || level > kTsrMaxLevel || n_taps < 2) return kErrArg;
  if (!dec_lo || !dec_hi || !rec_lo || !rec_hi) return kErrArg;
  if (n > kTsrMaxN || (n_taps & 1) || n_taps > kTsrMaxTaps) return kErrUnsupported;
  if (batch * (level + 1) > 0x7fffffffll) return kErrUnsupported;
  if (batch == 0) return kOk;  // empty batch: no-op (NULL arrays allowed)
  if (!x || !y || !stats) return kErrArg;
  if (reinterpret_cast<unsigned long long>(comps) & 7ull) return kErrArg;
  TsrArgs a;
  a.F = n_taps;
  a.level = level;
  a.add_constant = add_constant != 0;
  pad_taps(dec_lo, n_taps, a.taps[kDecLo]);
  pad_taps(dec_hi, n_taps, a.taps[kDecHi]);
  pad_taps(rec_lo, n_taps, a.taps[kRecLo]);
  pad_taps(rec_hi, n_taps, a.taps[kRecHi]);
  pyramid_lengths(static_cast<int>(n), n_taps, level, a.len);
  a.out_len = level > 0 ? 2 * a.len[1] - n_taps + 2 : a.len[0];  // pywt waverec length
  const int ext = (n_taps + 3) & ~3;
  const int cap0 = ((a.len[0] + 3) & ~3) + 2 * ext;
  const int cap1 = ((a.len[1] + 1 + 3) & ~3) + 2 * ext;
  const size_t lds = level > 0 ? static_cast<size_t>(cap0 + 2 * cap1) * sizeof(float) : 0;
  allow_lds(dwt_tsr_kernel, lds);
  const int threads = threads_for(n, 4, kTsrMaxThreads);  // about two output pairs of the finest level each
  hipLaunchKernelGGL(dwt_tsr_kernel, dim3(static_cast<unsigned>(batch * (level + 1))), dim3(threads), lds,
                     static_cast<hipStream_t>(stream), x, y, ld, a, stats, comps, ext, cap0, cap1);
  return launch_status();
}

extern "C" int wtmi_rows_ols(const float* x, const float* y, long long ld, long long rows, long long n,
                             int add_constant, double* stats, void* stream) {
  if (rows < 0 || n < 1 || ld < n) return kErrArg;
  if (rows > 0x7fffffffll) return kErrUnsupported;
  if (rows == 0) return kOk;  // empty batch: no-op (NULL arrays allowed)
  if (!x || !y || !stats) return kErrArg;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n <= 2048) {  // at most 8 float4 groups per lane: a wave per row
    const long long per = kOlsThreads / kWave;
    hipLaunchKernelGGL(rows_ols_kernel<true>, dim3(static_cast<unsigned>((rows + per - 1) / per)),
                       dim3(kOlsThreads), 0, st, x, y, ld, rows, n, add_constant != 0, stats);
  } else {
    hipLaunchKernelGGL(rows_ols_kernel<false>, dim3(static_cast<unsigned>(rows)), dim3(kOlsThreads), 0, st,
                       x, y, ld, rows, n, add_constant != 0, stats);
  }
  return launch_status();
}
