// Order statistics and shrinkage shared by the wavelet-shrinkage kernels (dwt_denoise.hip: K23;
// modwt_denoise.hip: K26): the exact median of a row's magnitudes by radix select on the bit
// patterns, and pywt.threshold of one coefficient.
#pragma once

#include "common.hpp"

// fp32 arithmetic of these kernels stays on the scalar VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace wtmi {

constexpr double kMadScale = 0.6744897501960817;  // the normal distribution's upper quartile

enum : int { kRuleFixed = 0, kRuleUniversal = 1, kRuleLevel = 2 };
enum : int { kSoft = 0, kHard = 1, kGarrote = 2 };

__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// median(|c[0 .. m)|) in fp64, the same value in every thread.  Called by the whole workgroup;
// c is only read, and a barrier separates the last read from the caller's next statement.  c may
// be an LDS or a global-memory row: it is read with plain loads only (the histograms and `above`
// are the LDS words the atomics go to), and a global row written by this workgroup before the
// caller's last barrier is visible to these loads.
__device__ double median_abs(const float* __restrict__ c, int m, unsigned (*hist)[256], unsigned* above) {
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & (kWave - 1);
  const int k0 = (m - 1) >> 1, k1 = m >> 1;  // the two middle order statistics (equal for odd m)
  unsigned v0, v1;
  if (m <= kWave) {
    const unsigned u = lane < m ? abs_bits(c[lane]) : 0xffffffffu;
    int rank = 0;  // position of this lane's value in the sorted row, ties by lane
    for (int j = 0; j < kWave; ++j) {
      const unsigned o = __shfl(u, j);
      rank += (o < u || (o == u && j < lane)) ? 1 : 0;
    }
    v0 = __shfl(u, __ffsll(__ballot(rank == k0)) - 1);
    v1 = __shfl(u, __ffsll(__ballot(rank == k1)) - 1);
    __syncthreads();
  } else {
    for (int i = tid; i < 256; i += T) hist[0][i] = 0u;  // a workgroup may be one wave
    __syncthreads();
    unsigned prefix = 0u, mask = 0u;
    int k = k0, eq = 0;  // rank still to go inside the prefix's bin; size of the chosen bin
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      unsigned* const h = hist[pass & 1];
      for (int i = tid; i < m; i += T) {
        const unsigned u = abs_bits(c[i]);
        if ((u & mask) == prefix) atomicAdd(&h[(u >> shift) & 255u], 1u);
      }
      __syncthreads();
      for (int i = tid; i < 256; i += T) hist[(pass + 1) & 1][i] = 0u;
      // every wave scans the 256 bins for itself: four bins per lane, then across the lanes
      const uint4 q = reinterpret_cast<const uint4*>(h)[lane];
      const int s = static_cast<int>(q.x + q.y + q.z + q.w);
      int incl = s;
      for (int d = 1; d < kWave; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
      }
      int r = k - (incl - s);
      const bool found = r >= 0 && k < incl;
      int bin = 4 * lane, cnt = static_cast<int>(q.x);
      if (found) {
        if (r >= cnt) { r -= cnt; ++bin; cnt = static_cast<int>(q.y);
          if (r >= cnt) { r -= cnt; ++bin; cnt = static_cast<int>(q.z);
            if (r >= cnt) { r -= cnt; ++bin; cnt = static_cast<int>(q.w); } } }
      }
      const int src = __ffsll(__ballot(found)) - 1;
      bin = __shfl(bin, src);
      k = __shfl(r, src);
      eq = __shfl(cnt, src);
      prefix |= static_cast<unsigned>(bin) << shift;
      mask |= 255u << shift;
      __syncthreads();
    }
    v0 = v1 = prefix;
    if (k1 >= k0 - k + eq) {  // count(<= v0) does not reach rank k1: the smallest element above v0
      if (tid == 0) *above = 0xffffffffu;
      __syncthreads();
      unsigned mn = 0xffffffffu;
      for (int i = tid; i < m; i += T) {
        const unsigned u = abs_bits(c[i]);
        if (u > v0 && u < mn) mn = u;
      }
      if (mn != 0xffffffffu) atomicMin(above, mn);
      __syncthreads();
      v1 = *above;
    }
  }
  const double f0 = __uint_as_float(v0), f1 = __uint_as_float(v1);
  return 0.5 * (f0 + f1);
}

// pywt.threshold of one coefficient against lf = (float)lambda; keep: non-zero by the rule
__device__ __forceinline__ float shrink_one(float c, float lf, int shrink, bool& keep) {
  const float ac = fabsf(c);
  keep = shrink == kHard ? ac >= lf : ac > lf;
  if (!keep) return 0.f;
  if (shrink == kHard) return c;
  if (shrink == kSoft) return copysignf(ac - lf, c);
  return fmaf(-lf, lf / c, c);  // c (1 - lambda^2 / c^2), |c| > lambda >= 0: no 0 / 0
}

}  // namespace wtmi

#pragma clang attribute pop
