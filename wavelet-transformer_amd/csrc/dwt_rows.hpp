// Row helpers of the fused pyramid-DWT kernels (dwt_tsr.hip: K17; dwt_smooth.hip: K21), whose
// level rows live in LDS with their symmetric extension written out once per level: the row
// load, the extension, the step barrier, and the host side's length table and tap arrays.  The
// tap loops themselves stay in the two kernels: routed through shared helpers, dwt_tsr_kernel
// compiled to different code and measured 0.6 .. 0.9 % slower (profiles/r10/INDEX.md).
#pragma once

#include "common.hpp"

namespace wtmi {

constexpr int kPyrMaxTaps = 40;   // size of a tap array in a kernel's argument block
constexpr int kPyrMaxLevel = 60;  // size of its length table, less one

// General half-sample reflection of any index onto [0, m): exact also where the extension
// wraps the row more than once (m < F - 2).  Used by the few threads that write a level's
// extension, never inside a tap loop.
__device__ __forceinline__ int reflect(int j, int m) {
  const int p = 2 * m;
  int r = j % p;
  if (r < 0) r += p;
  return r < m ? r : p - 1 - r;
}

// Between two steps of the cascade.  A step with at most one wave of outputs is done by wave 0
// alone (the strided loops leave the other waves nothing), so between two such steps only that
// wave has to see its own LDS writes: no workgroup barrier across the coarse levels.
__device__ __forceinline__ void step_sync(bool& prev_small, bool small) {
  if (prev_small && small) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
  prev_small = small;
}

// Global row g[0 .. n) into the 16-byte aligned LDS row dst, as float4 where g is aligned too.
__device__ __forceinline__ void load_row(float* __restrict__ dst, const float* __restrict__ g, int n) {
  const int tid = threadIdx.x, T = blockDim.x;
  if (aligned16(g)) {
    const int n4 = n >> 2;
    for (int i = tid; i < n4; i += T)
      reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(g)[i];
    for (int i = 4 * n4 + tid; i < n; i += T) dst[i] = g[i];
  } else {
    for (int i = tid; i < n; i += T) dst[i] = g[i];
  }
}

// Symmetric extension of the m-sample row cur, by the first lim threads: F - 2 samples before
// the row, F - 1 after.
__device__ __forceinline__ void extend_row(float* cur, int m, int F, int lim) {
  const int tid = threadIdx.x;
  if (tid < lim)
    for (int e = tid; e < 2 * F - 3; e += lim) {
      const int idx = e < F - 2 ? e - (F - 2) : m + e - (F - 2);
      cur[idx] = cur[reflect(idx, m)];
    }
}

// Host: pywt's coefficient lengths in mode "symmetric", len[0] = n and len[j] = len(cA_j) =
// len(cD_j) = (len[j-1] + F - 1) / 2 up to `level`, 0 beyond.
inline void pyramid_lengths(int n, int F, int level, int (&len)[kPyrMaxLevel + 1]) {
  len[0] = n;
  for (int j = 1; j <= kPyrMaxLevel; ++j) len[j] = j <= level ? (len[j - 1] + F - 1) / 2 : 0;
}

// Host: F taps as floats, zero-padded (only the first F are read).
inline void pad_taps(const double* src, int F, float (&dst)[kPyrMaxTaps]) {
  for (int k = 0; k < kPyrMaxTaps; ++k) dst[k] = k < F ? static_cast<float>(src[k]) : 0.f;
}

}  // namespace wtmi
