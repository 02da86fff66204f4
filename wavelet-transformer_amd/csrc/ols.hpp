// fp64 moments of a float32 row pair, their workgroup reductions and the OLS epilogue on the
// five-sum form, shared by the fused kernels: Mom / block_sum / ols_store by dwt_tsr.hip (K17 /
// K18), modwt_mra.hip (K19) and dwt_smooth.hip (K21); Mom3 / block_sum3 by modwt_wcorr.hip (K22).
#pragma once

#include "common.hpp"

// fp32 -> fp64 conversions and the sums stay on the scalar VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace wtmi {

// ---- fp64 moments of a row pair, shifted by the rows' first samples ----------------------
// (a constant row then has every shifted sum exactly 0, and the centred sums lose nothing to
// a large mean)
struct Mom {
  double sx, sy, sxx, sxy, syy;
  __device__ __forceinline__ void add(float x, float y, double kx, double ky) {
    const double dx = static_cast<double>(x) - kx, dy = static_cast<double>(y) - ky;
    sx += dx;
    sy += dy;
    sxx = fma(dx, dx, sxx);
    sxy = fma(dx, dy, sxy);
    syy = fma(dy, dy, syy);
  }
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

__device__ __forceinline__ Mom wave_sum(Mom m) {
  return Mom{wave_sum(m.sx), wave_sum(m.sy), wave_sum(m.sxx), wave_sum(m.sxy), wave_sum(m.syy)};
}

// The two block sums below keep their own wave-to-LDS halves: written once over a parameter
// pack, the register moves around the shuffle calls changed in every kernel that reduces.
// sum over the workgroup, valid in thread 0; red: 5 doubles per wave
__device__ __forceinline__ Mom block_sum(Mom m, double* red) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  m = wave_sum(m);
  if (lane == 0) {
    red[5 * wave + 0] = m.sx;
    red[5 * wave + 1] = m.sy;
    red[5 * wave + 2] = m.sxx;
    red[5 * wave + 3] = m.sxy;
    red[5 * wave + 4] = m.syy;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + kWave - 1) / kWave;
    for (int w = 1; w < nw; ++w) {
      m.sx += red[5 * w + 0];
      m.sy += red[5 * w + 1];
      m.sxx += red[5 * w + 2];
      m.sxy += red[5 * w + 3];
      m.syy += red[5 * w + 4];
    }
  }
  return m;
}

// ---- the three lag-0 sums of a coefficient row pair (no shift: the rows are details) ------
struct Mom3 {
  double sxx, sxy, syy;
};

template <bool PAIR>
__device__ __forceinline__ void mom_add(Mom3& m, float wx, float wy, bool in) {
  if (in) {
    const double dx = static_cast<double>(wx);
    m.sxx = fma(dx, dx, m.sxx);
    if (PAIR) {
      const double dy = static_cast<double>(wy);
      m.sxy = fma(dx, dy, m.sxy);
      m.syy = fma(dy, dy, m.syy);
    }
  }
}

// Sum over the workgroup, valid (and bitwise the same) in every thread; red: 3 doubles per wave.
// Its barrier ends the caller's LDS reads and publishes its LDS writes.
__device__ __forceinline__ Mom3 block_sum3(Mom3 m, double* red) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  m.sxx = wave_sum(m.sxx);
  m.sxy = wave_sum(m.sxy);
  m.syy = wave_sum(m.syy);
  if (lane == 0) {
    red[3 * wave + 0] = m.sxx;
    red[3 * wave + 1] = m.sxy;
    red[3 * wave + 2] = m.syy;
  }
  __syncthreads();
  Mom3 r{0.0, 0.0, 0.0};
  const int nw = blockDim.x / kWave;
  for (int w = 0; w < nw; ++w) {
    r.sxx += red[3 * w + 0];
    r.sxy += red[3 * w + 1];
    r.syy += red[3 * w + 2];
  }
  return r;
}

// The regression of y on [1, x] (add_constant) or on x alone, from the shifted moments of nobs
// samples (one thread): const, slope, bse_const, bse_slope, rsquared, ssr, nobs, df_resid.
__device__ void ols_store(const Mom& m, double kx, double ky, double nobs, int add_constant,
                          double* __restrict__ out) {
  const double mx = m.sx / nobs, my = m.sy / nobs;
  const double xbar = kx + mx, ybar = ky + my;
  double sxx = m.sxx - m.sx * mx, sxy = m.sxy - m.sx * my, syy = m.syy - m.sy * my;
  double c0 = 0.0, bse0 = 0.0, df = nobs - 1.0, q = 0.0;  // q: the x' x^-1 term of bse_const
  if (add_constant) {
    df = nobs - 2.0;
    q = 1.0 / nobs + xbar * xbar / sxx;
  } else {  // statsmodels' no-constant model: uncentred sums
    sxx = fma(nobs * xbar, xbar, sxx);
    sxy = fma(nobs * xbar, ybar, sxy);
    syy = fma(nobs * ybar, ybar, syy);
  }
  const double nan = __builtin_nan("");
  double slope = nan, bse1 = nan, ssr = syy, r2 = 0.0;
  if (sxx != 0.0) {
    slope = sxy / sxx;
    ssr = fmax(syy - slope * sxy, 0.0);
    r2 = 1.0 - ssr / syy;
    bse1 = sqrt(ssr / df / sxx);
  }
  if (add_constant) {
    c0 = sxx != 0.0 ? ybar - slope * xbar : ybar;
    bse0 = sxx != 0.0 ? sqrt(ssr / df * q) : nan;
  }
  out[0] = c0;
  out[1] = slope;
  out[2] = bse0;
  out[3] = bse1;
  out[4] = r2;
  out[5] = ssr;
  out[6] = nobs;
  out[7] = df;
}

}  // namespace wtmi

#pragma clang attribute pop
