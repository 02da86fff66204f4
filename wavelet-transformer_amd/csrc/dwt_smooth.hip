// DWT smoothing ladder with per-level OLS (K21 of DESIGN.md).
//
// Replaces ResultsFromDWT.smooth_signal (src/dwt.py:53-73) computed from the series itself and
// wavelet_approximation (src/regression.py:66-88) in ONE launch.  smooth_l zeroes cD_1 .. cD_l;
// by perfect reconstruction the pyramid above level l rebuilds cA_l, so smooth_l is cA_l pushed
// through l low-pass-only synthesis steps with pywt's one-sample trim between steps.  No detail
// coefficient is computed, stored or read: only dec_lo and rec_lo enter the kernel.
//
// "Chain l" is the sequence of rows cA_l = r_l -> r_{l-1} -> .. -> r_1 -> smooth_l.  A workgroup
// owns one series and the chains l0 .. l1 of it:
//   phase A  cA_1 .. cA_{l1} by the low-pass filter alone, every level resident in LDS, the
//            symmetric extension written out once per level (straight 8-byte pair reads):
//              c[i] = sum_{p<F/2} lo[2p] xe[2i+1-2p] + lo[2p+1] xe[2i-2p]
//   phase B  all chains in lockstep by level.  Stage k (l1 .. 2) maps the level-k row of every
//            chain l >= k to its level-(k-1) row, chain k entering from the resident cA_k:
//              y[2u] = sum_{w<F/2} c[u+w] g[F-2-2w],  y[2u+1] = sum_w c[u+w] g[F-1-2w]
//            one pass over (row, output pair), so the synthesis costs l1 stage barriers, not
//            l1 (l1 + 1) / 2 cascaded steps, and the coarse stages fill the lanes with several
//            rows.  pywt's trim (2 len[k] - F + 2 = len[k-1] + 1) is done by never reading the
//            extra last sample.
//   stage 1  per chain, the final row is produced per thread from the chain's level-1 row
//            (cA_1 itself for chain 1), written out if asked for and fed to the fp64 shifted
//            moments of ols.hpp against the RAW y, which is staged once in x's dead LDS row.
//            For odd n sample 0 of the n + 1 reconstructed ones is dropped (trim_signal).
//
// LDS, in floats, with E = F rounded up to 4 and r4(m) = m rounded up to 4:
//   x / y row            r4(n) + 2 E
//   pyramid              sum_{j=1..J} r4(len[j]) + 2 E         (about n + 2 E J)
//   chain ping-pong      nch (s_odd + s_even),  s_p = r4(1 + max len[j] over j >= 1 of parity p)
//                        (len[1] + len[2] unless the level exceeds what the series supports)
// Grouping rule: nch = the most chains that keep the sum within 79 KiB (two workgroups per CU of
// 160 KiB, the static reduction rows included), at least 1; the J chains are split evenly into
// ceil(J / nch) groups, the grid is batch x groups, and group g redoes the cheap low-pass
// pyramid to its own depth l1.  A single chain of n = 8192 needs about 92 KiB: one workgroup
// per CU, the dynamic LDS limit raised for the launch.
#include "common.hpp"
#include "dwt_rows.hpp"
#include "ols.hpp"

// fp32 arithmetic of this file stays on the scalar VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace wtmi {

constexpr int kSmoothMaxTaps = kPyrMaxTaps;
constexpr int kSmoothMaxN = 8192;
constexpr int kSmoothMaxThreads = 512;
constexpr int kSmoothMaxLevel = kPyrMaxLevel;
constexpr int kSmoothLdsBudget = 79 * 1024;  // bytes of dynamic LDS: two workgroups per CU
constexpr int kSmoothLdsMax = 159 * 1024;     // (1 KiB each left for the reduction rows)

struct SmoothArgs {
  int F, level, add_constant;
  int nch, groups;              // chains per workgroup, workgroups per series
  int ext;                      // floats kept free on either side of an analysed row
  int buf[2], stride[2];        // chain rows of even / odd level: offset of slot 0, slot pitch
  int len[kSmoothMaxLevel + 1];  // len[0] = n, len[j] = len(cA_j) = (len[j-1] + F - 1) / 2
  int off[kSmoothMaxLevel + 1];  // LDS offset of sample 0 of the level-j row (0: the x / y row)
  float dec_lo[kSmoothMaxTaps], rec_lo[kSmoothMaxTaps];  // only the first F of each are read
};

// both samples of output pair u of one polyphase low-pass synthesis step
__device__ __forceinline__ float2 syn_pair(const float* __restrict__ c, int u, const SmoothArgs& a) {
  const int F = a.F, H = a.F / 2;
  float ye = 0.f, yo = 0.f;
  for (int w = 0; w < H; ++w) {
    const float v = c[u + w];
    ye = fmaf(v, a.rec_lo[F - 2 - 2 * w], ye);
    yo = fmaf(v, a.rec_lo[F - 1 - 2 * w], yo);
  }
  return make_float2(ye, yo);
}

// Six waves per SIMD is what the app's shape can hold (n = 1333, db4, J = 7: 39 KB of LDS, four
// 384-thread workgroups per CU).  Without the bound the scheduler hoists every LDS read of
// block_sum's thread-0 loop and allocates 116 VGPRs for the whole kernel.
template <bool STATS>
__global__ void __launch_bounds__(kSmoothMaxThreads) __attribute__((amdgpu_waves_per_eu(6, 8)))
dwt_smooth_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ld, SmoothArgs a,
                  float* __restrict__ smooth, double* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ double red[2][5 * (kSmoothMaxThreads / kWave)];
  const int tid = threadIdx.x, T = blockDim.x;
  const int F = a.F, H = a.F / 2, n = a.len[0];
  const long long b = blockIdx.x / a.groups;
  const int l0 = 1 + static_cast<int>(blockIdx.x - b * a.groups) * a.nch;  // chains l0 .. l1
  const int l1 = min(a.level, l0 + a.nch - 1);
  float* const X = sm + a.off[0];

  // ---- phase A: the approximation pyramid down to level l1 ----
  load_row(X, x + b * ld, n);
  bool prev_small = false;
  for (int j = 1; j <= l1; ++j) {
    float* const cur = sm + a.off[j - 1];
    float* const dst = sm + a.off[j];
    const int m = a.len[j - 1], M = a.len[j];
    const bool small = M <= kWave;
    step_sync(prev_small, small);
    extend_row(cur, m, F, small ? kWave : T);
    step_sync(prev_small, small);
    for (int i = tid; i < M; i += T) {
      const float2* p2 = reinterpret_cast<const float2*>(cur + 2 * i);  // (xe[2i], xe[2i+1])
      float acc = 0.f;
      for (int p = 0; p < H; ++p) {
        const float2 v = p2[-p];
        acc = fmaf(a.dec_lo[2 * p], v.y, acc);
        acc = fmaf(a.dec_lo[2 * p + 1], v.x, acc);
      }
      dst[i] = acc;
    }
  }

  // ---- phase B: every chain one level down per stage ----
  for (int k = l1; k >= 2; --k) {
    const int P = a.len[k] - H + 1;   // output pairs: 2 P = 2 len[k] - F + 2 samples
    const int lo = max(k, l0);        // chains lo .. l1 have a level-k row
    const int rows = l1 - lo + 1;
    const bool small = rows * P <= kWave;
    step_sync(prev_small, small);
    const float* const src = sm + a.buf[k & 1];
    float* const dst = sm + a.buf[(k - 1) & 1];
    const int ss = a.stride[k & 1], ds = a.stride[(k - 1) & 1];
    int r = 0, u = tid;
    while (u >= P && r < rows) {
      u -= P;
      ++r;
    }
    while (r < rows) {
      const int l = lo + r;
      const float* c = l == k ? sm + a.off[k] : src + (l - l0) * ss;
      *reinterpret_cast<float2*>(dst + (l - l0) * ds + 2 * u) = syn_pair(c, u, a);
      u += T;
      while (u >= P && r < rows) {
        u -= P;
        ++r;
      }
    }
  }

  // ---- stage 1: the smooths, in registers, into global memory and the moments ----
  __syncthreads();
  float* const Y = X;  // x is dead once cA_1 exists
  if (STATS) {
    load_row(Y, y + b * ld, n);
    __syncthreads();
  }
  const int odd = n & 1;  // trim_signal: the first of the n + 1 samples goes
  const int P = a.len[1] - H + 1;
  const double ky = STATS ? static_cast<double>(Y[0]) : 0.0;
  for (int l = l0; l <= l1; ++l) {
    const float* c = l == 1 ? sm + a.off[1] : sm + a.buf[1] + (l - l0) * a.stride[1];
    float* out = smooth ? smooth + (b * a.level + (l - 1)) * static_cast<long long>(n) : nullptr;
    // pair u holds samples 2u - odd and 2u + 1 - odd of the smooth: 8-byte stores where that
    // address is even in floats
    const bool vec = ((reinterpret_cast<unsigned long long>(out) >> 2) & 1ull) == static_cast<unsigned>(odd);
    Mom mom{0.0, 0.0, 0.0, 0.0, 0.0};
    double kx = 0.0;
    if (STATS) {  // sample 0 of this smooth: the moments' shift
      const float2 v = syn_pair(c, 0, a);
      kx = odd ? v.y : v.x;
    }
    for (int u = tid; u < P; u += T) {
      const float2 v = syn_pair(c, u, a);
      const int i0 = 2 * u - odd;
      if (STATS) {
        if (i0 >= 0) mom.add(v.x, Y[i0], kx, ky);
        mom.add(v.y, Y[i0 + 1], kx, ky);
      }
      if (out) {
        if (vec && i0 >= 0) {
          *reinterpret_cast<float2*>(out + i0) = v;
        } else {
          if (i0 >= 0) out[i0] = v.x;
          out[i0 + 1] = v.y;
        }
      }
    }
    if (STATS) {
      // two reduction rows in turn: a wave may enter chain l + 1's sum while thread 0 still
      // reads chain l's, but not chain l + 2's (the barrier inside block_sum)
      mom = block_sum(mom, red[(l - l0) & 1]);
      if (tid == 0)
        ols_store(mom, kx, ky, static_cast<double>(n), a.add_constant, stats + (b * a.level + (l - 1)) * 8);
    }
  }
}

}  // namespace wtmi

#pragma clang attribute pop

using namespace wtmi;

extern "C" int wtmi_dwt_smooth(const float* x, const float* y, long long ld, long long batch, long long n,
                               const double* dec_lo, const double* rec_lo, int n_taps, int level,
                               int add_constant, float* smooth, double* stats, void* stream) {
  if (batch < 0 || n < 1 || ld < n || level < 1 || n_taps < 2) return kErrArg;
  if (!dec_lo || !rec_lo) return kErrArg;
  if (n > kSmoothMaxN || (n_taps & 1) || n_taps > kSmoothMaxTaps || level > kSmoothMaxLevel)
    return kErrUnsupported;
  if (batch == 0) return kOk;  // empty batch: no-op (NULL arrays allowed)
  if (!x || (!smooth && !stats) || (stats && !y)) return kErrArg;
  SmoothArgs a;
  a.F = n_taps;
  a.level = level;
  a.add_constant = add_constant != 0;
  pad_taps(dec_lo, n_taps, a.dec_lo);
  pad_taps(rec_lo, n_taps, a.rec_lo);
  pyramid_lengths(static_cast<int>(n), n_taps, level, a.len);
  auto r4 = [](int m) { return (m + 3) & ~3; };
  a.ext = r4(n_taps);
  a.off[0] = a.ext;
  int smax[2] = {0, 0};
  for (int j = 1; j <= kSmoothMaxLevel; ++j) {
    a.off[j] = a.off[j - 1] + r4(a.len[j - 1]) + 2 * a.ext;
    if (j <= level && a.len[j] + 1 > smax[j & 1]) smax[j & 1] = a.len[j] + 1;
  }
  const int base = a.off[level] + r4(a.len[level]) + a.ext;  // the x / y row and the pyramid
  a.stride[0] = r4(smax[0]);
  a.stride[1] = r4(smax[1]);
  const int per = a.stride[0] + a.stride[1];
  int fit = (kSmoothLdsBudget / static_cast<int>(sizeof(float)) - base) / per;
  fit = fit < 1 ? 1 : fit > level ? level : fit;
  a.groups = (level + fit - 1) / fit;
  a.nch = (level + a.groups - 1) / a.groups;
  a.buf[1] = base;
  a.buf[0] = base + a.nch * a.stride[1];
  const size_t lds = static_cast<size_t>(base + a.nch * per) * sizeof(float);
  if (lds > static_cast<size_t>(kSmoothLdsMax) || batch * a.groups > 0x7fffffffll) return kErrUnsupported;
  auto* kern = stats ? dwt_smooth_kernel<true> : dwt_smooth_kernel<false>;
  allow_lds(kern, lds);
  const int threads = threads_for(n, 4, kSmoothMaxThreads);  // about two output pairs of the finest level each
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(batch * a.groups)), dim3(threads), lds,
                     static_cast<hipStream_t>(stream), x, y, ld, a, smooth, stats);
  return launch_status();
}
