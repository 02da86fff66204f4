// Row helpers of the fused a-trous MODWT kernels (modwt_mra.hip: K19 / K20; modwt_wcorr.hip:
// K22), whose series stay in LDS across all levels and whose threads own samples or float4
// groups at stride blockDim.
#pragma once

#include "common.hpp"

// fp32 arithmetic of these kernels stays on the scalar VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace wtmi {

constexpr int kModwtRowsMaxTaps = 40;
constexpr int kModwtRowsMaxLevel = 62;  // 2^(j-1) as a long long, as wtmi_modwt

// Row g into LDS, shifted by its first sample (returned).
__device__ __forceinline__ float load_shifted(const float* __restrict__ g, float* __restrict__ V, int n) {
  const float k = g[0];
#pragma unroll 4
  for (int i = threadIdx.x; i < n; i += blockDim.x) V[i] = g[i] - k;
  return k;
}

// One thread: soff[l] = (d l) mod n for the L taps, by repeated addition (d < n).
__device__ __forceinline__ void tap_offsets(int d, int n, int L, int* soff) {
  int o = 0;
  for (int l = 0; l < L; ++l) {
    soff[l] = o;
    o += d;
    if (o >= n) o -= n;
  }
}

__device__ __forceinline__ float4 add4(const float4& p, const float4& q) {
  return make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w);
}

__device__ __forceinline__ void fma4(float4& acc, float c, const float4& v) {
  acc.x = fmaf(c, v.x, acc.x);
  acc.y = fmaf(c, v.y, acc.y);
  acc.z = fmaf(c, v.z, acc.z);
  acc.w = fmaf(c, v.w, acc.w);
}

// Register window of the aligned float4 groups q - BEFORE .. q + AFTER of a circular row of ng
// groups (ng >= 16 > BEFORE, AFTER): sample 4 q + i of the row is f[4 BEFORE + i].
template <int BEFORE, int AFTER>
__device__ __forceinline__ void load_window(const float4* __restrict__ V4, int q, int ng,
                                            float (&f)[4 * (BEFORE + AFTER + 1)]) {
#pragma unroll
  for (int w = 0; w < BEFORE + AFTER + 1; ++w) {
    int qs = q - BEFORE + w;
    qs = qs < 0 ? qs + ng : (AFTER > 0 && qs >= ng ? qs - ng : qs);
    const float4 v = V4[qs];
    f[4 * w] = v.x; f[4 * w + 1] = v.y; f[4 * w + 2] = v.z; f[4 * w + 3] = v.w;
  }
}

#pragma clang attribute pop

// Host: the MODWT bank h~ = dec_hi / sqrt2, g~ = dec_lo / sqrt2 in fp64, rounded once.
inline void scaled_bank(const double* dec_lo, const double* dec_hi, int n_taps, float* h, float* g) {
  const double r = 1.0 / sqrt(2.0);
  for (int l = 0; l < n_taps; ++l) {
    h[l] = static_cast<float>(dec_hi[l] * r);
    g[l] = static_cast<float>(dec_lo[l] * r);
  }
}

}  // namespace wtmi
