// DWT wavelet shrinkage with MAD thresholds (K23 of DESIGN.md).
//
// pywt.wavedec (mode "symmetric") of a series, a noise scale from the median absolute deviation
// of its detail coefficients, pywt.threshold of every detail array and pywt.waverec of the
// shrunk list, in ONE launch with one workgroup per series.  Unlike K17 / K21, which rebuild
// from a single array, every detail array of the pyramid stays resident in LDS from the
// analysis to the synthesis:
//   analysis   level j reads the extended cA_{j-1} once and forms both cA_j and cD_j from the
//              same 8-byte pair reads (two accumulators per output):
//                c[i] = sum_{p<F/2} f[2p] xe[2i+1-2p] + f[2p+1] xe[2i-2p]
//   select     median(|cD_j|) by exact radix select on the bit patterns of |c| (non-negative
//              floats order as their uint32 patterns): four 8-bit passes, each a 256-bin LDS
//              histogram (LDS atomics) of the elements that match the prefix found so far and a
//              scan of it that EVERY wave does for itself from the same histogram, so the
//              prefix and the remaining rank stay in registers, uniform over the workgroup, and
//              a pass costs two barriers.  The rank bookkeeping gives count(<= v_k); only where
//              the next order statistic is not v_k again (even lengths) one LDS atomic-min over
//              the elements above v_k follows.  No copy of the row, no sort.  Arrays of at most
//              64 coefficients are ranked by cross-lane reads, one coefficient per lane, by
//              every wave for itself.  Rule 1 selects once (cD_1), rule 2 once per level.
//   shrink     one in-place pass over cD_j as soon as lambda_j is known: each coefficient is
//              shrunk once (not F/2 times inside the synthesis tap loops), kept_j is counted by
//              wave ballots in the same pass and the shrunk value goes to `coeffs` if asked.
//   synthesis  the two-input polyphase step, the trim of pywt's waverec done by never reading
//              the extra last sample of the rebuilt approximation:
//                y[2u]   = sum_{w<F/2} a[u+w] rec_lo[F-2-2w] + d[u+w] rec_hi[F-2-2w]
//                y[2u+1] = sum_{w<F/2} a[u+w] rec_lo[F-1-2w] + d[u+w] rec_hi[F-1-2w]
//              The last step writes out[0 .. n) from registers, 8 bytes at a time where the row
//              is aligned.
//
// LDS, in floats, with E = F rounded up to 4 and r4(m) = m rounded up to 4.  Approximations of
// even level (the series is level 0) live in region A, of odd level in region B, both with room
// for the symmetric extension; the rebuilt approximation of level j returns to the slot of cA_j.
//   A   E + max(r4(n), r4(1 + max len[even j])) + E, then cD_2, cD_3 .. packed behind the even
//       slot: they are written from level 2 on, when the series is dead, so the region is
//       max(r4(n) + 2 E, 2 E + r4(1 + max len[even j >= 2]) + sum_{j>=2} r4(len[j]))
//   B   E + r4(1 + max len[odd j]) + E
//   C   r4(len[1]): cD_1 (detail arrays need no extension: the synthesis reads c[u+w], w < F/2)
// About 2 n + 4 E: 66.3 KB at n = 8192, F = 40 and 65.9 KB for db4, plus 2.3 KB static (two
// histograms, the kept counters), so two 512-thread workgroups share a CU's 160 KiB.
#include <math.h>

#include "common.hpp"
#include "dwt_rows.hpp"
#include "select.hpp"

// fp32 arithmetic of this file stays on the scalar VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace wtmi {

constexpr int kDenMaxN = 8192;
constexpr int kDenMaxThreads = 512;

enum : int { kDecLo = 0, kDecHi = 1, kRecLo = 2, kRecHi = 3 };

struct DenArgs {
  int F, level, rule, shrink;
  int offA, offB;                // LDS offset of sample 0 of the even / odd approximation slot
  int len[kPyrMaxLevel + 1];     // len[0] = n, len[j] = len(cA_j) = len(cD_j)
  int doff[kPyrMaxLevel + 1];    // LDS offset of cD_j, j >= 1
  long long thr_ld, total;       // row pitch of thresholds (0: one row), coefficients per series
  double lam_scale;              // mult * sqrt(2 ln n)
  float taps[4][kPyrMaxTaps];    // dec_lo, dec_hi, rec_lo, rec_hi: only the first F of each are read
};

__global__ void __launch_bounds__(kDenMaxThreads)
dwt_denoise_kernel(const float* __restrict__ x, long long ld, DenArgs a, const double* __restrict__ thr,
                   float* __restrict__ out, long long ld_out, double* __restrict__ info,
                   float* __restrict__ coeffs) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ __attribute__((aligned(16))) unsigned hist[2][256];
  __shared__ int kept_s[kWave];
  __shared__ unsigned above;
  const int tid = threadIdx.x, T = blockDim.x;
  const int F = a.F, H = a.F / 2, n = a.len[0], J = a.level;
  const long long b = blockIdx.x;
  float* const A = sm + a.offA;
  float* const B = sm + a.offB;
  float* const gc = coeffs ? coeffs + b * a.total : nullptr;

  // ---- analysis: cA_j to the slot of its parity, cD_j to its own row ----
  load_row(A, x + b * ld, n);
  if (tid < kWave) kept_s[tid] = 0;
  bool prev_small = false;
  for (int j = 1; j <= J; ++j) {
    float* const cur = (j & 1) ? A : B;
    float* const dst_a = (j & 1) ? B : A;
    float* const dst_d = sm + a.doff[j];
    const int m = a.len[j - 1], M = a.len[j];
    const bool small = M <= kWave;
    step_sync(prev_small, small);
    extend_row(cur, m, F, small ? kWave : T);
    step_sync(prev_small, small);
    for (int i = tid; i < M; i += T) {
      const float2* p2 = reinterpret_cast<const float2*>(cur + 2 * i);  // (xe[2i], xe[2i+1])
      float lo = 0.f, hi = 0.f;
      for (int p = 0; p < H; ++p) {
        const float2 v = p2[-p];
        lo = fmaf(a.taps[kDecLo][2 * p], v.y, lo);
        lo = fmaf(a.taps[kDecLo][2 * p + 1], v.x, lo);
        hi = fmaf(a.taps[kDecHi][2 * p], v.y, hi);
        hi = fmaf(a.taps[kDecHi][2 * p + 1], v.x, hi);
      }
      dst_a[i] = lo;
      dst_d[i] = hi;
    }
  }
  __syncthreads();
  if (gc) {  // cA_J is never modified
    const float* ca = (J & 1) ? B : A;
    for (int i = tid; i < a.len[J]; i += T) gc[i] = ca[i];
  }

  // ---- thresholds and the in-place shrink, level by level ----
  double sigma = __builtin_nan(""), lam = 0.0;
  long long goff = a.total;  // cD_j ends where cD_{j-1} begins; cD_1 is the last array
  for (int j = 1; j <= J; ++j) {
    float* const c = sm + a.doff[j];
    const int m = a.len[j];
    goff -= m;
    if (a.rule == kRuleFixed) {
      lam = thr[b * a.thr_ld + (j - 1)];
    } else if (a.rule == kRuleLevel || j == 1) {
      sigma = median_abs(c, m, hist, &above) / kMadScale;
      lam = a.lam_scale * sigma;
    }
    const float lf = static_cast<float>(lam);
    int cnt = 0;  // per wave
    for (int i0 = 0; i0 < m; i0 += T) {
      const int i = i0 + tid;
      bool keep = false;
      if (i < m) {
        const float s = shrink_one(c[i], lf, a.shrink, keep);
        c[i] = s;
        if (gc) gc[goff + i] = s;
      }
      cnt += __popcll(__ballot(keep));
    }
    if ((tid & (kWave - 1)) == 0 && cnt) atomicAdd(&kept_s[j], cnt);
    if (info && tid == 0) {
      double* r = info + (b * J + (j - 1)) * 4;
      r[0] = sigma;
      r[1] = lam;
      r[3] = static_cast<double>(m);
    }
  }
  __syncthreads();
  if (info && tid >= 1 && tid <= J) info[(b * J + (tid - 1)) * 4 + 2] = static_cast<double>(kept_s[tid]);

  // ---- synthesis: the rebuilt cA_{j-1} returns to its slot; the last step goes to global ----
  prev_small = false;
  for (int j = J; j >= 2; --j) {
    const int P = a.len[j] - H + 1;  // output pairs: 2 P = 2 len[j] - F + 2 samples
    const bool small = P <= kWave;
    step_sync(prev_small, small);
    const float* ca = (j & 1) ? B : A;
    const float* cd = sm + a.doff[j];
    float* const dst = (j & 1) ? A : B;
    for (int u = tid; u < P; u += T) {
      float ye = 0.f, yo = 0.f;
      for (int w = 0; w < H; ++w) {
        const float va = ca[u + w], vd = cd[u + w];
        ye = fmaf(va, a.taps[kRecLo][F - 2 - 2 * w], ye);
        yo = fmaf(va, a.taps[kRecLo][F - 1 - 2 * w], yo);
        ye = fmaf(vd, a.taps[kRecHi][F - 2 - 2 * w], ye);
        yo = fmaf(vd, a.taps[kRecHi][F - 1 - 2 * w], yo);
      }
      *reinterpret_cast<float2*>(dst + 2 * u) = make_float2(ye, yo);
    }
  }
  step_sync(prev_small, false);
  {
    const float* ca = B;
    const float* cd = sm + a.doff[1];
    float* const o = out + b * ld_out;
    const bool vec = (reinterpret_cast<unsigned long long>(o) & 7ull) == 0;
    const int P = a.len[1] - H + 1;  // 2 P >= n: the first n samples are pywt's waverec(...)[:n]
    for (int u = tid; u < P; u += T) {
      float ye = 0.f, yo = 0.f;
      for (int w = 0; w < H; ++w) {
        const float va = ca[u + w], vd = cd[u + w];
        ye = fmaf(va, a.taps[kRecLo][F - 2 - 2 * w], ye);
        yo = fmaf(va, a.taps[kRecLo][F - 1 - 2 * w], yo);
        ye = fmaf(vd, a.taps[kRecHi][F - 2 - 2 * w], ye);
        yo = fmaf(vd, a.taps[kRecHi][F - 1 - 2 * w], yo);
      }
      const int i0 = 2 * u;
      if (vec && i0 + 1 < n) {
        *reinterpret_cast<float2*>(o + i0) = make_float2(ye, yo);
      } else {
        if (i0 < n) o[i0] = ye;
        if (i0 + 1 < n) o[i0 + 1] = yo;
      }
    }
  }
}

}  // namespace wtmi

#pragma clang attribute pop

using namespace wtmi;

extern "C" int wtmi_dwt_denoise(const float* x, long long ld, long long batch, long long n,
                                const double* dec_lo, const double* dec_hi, const double* rec_lo,
                                const double* rec_hi, int n_taps, int level, int rule, int shrink, double mult,
                                const double* thresholds, long long thr_ld, float* out, long long ld_out,
                                double* info, float* coeffs, void* stream) {
  if (batch < 0 || n < 1 || ld < n || ld_out < n || level < 1 || n_taps < 2) return kErrArg;
  if (!dec_lo || !dec_hi || !rec_lo || !rec_hi) return kErrArg;
  if (rule < kRuleFixed || rule > kRuleLevel || shrink < kSoft || shrink > kGarrote) return kErrArg;
  if (!(mult >= 0.0) || !isfinite(mult)) return kErrArg;
  if (rule == kRuleFixed && (!thresholds || thr_ld < 0 || (thr_ld > 0 && thr_ld < level))) return kErrArg;
  if (n > kDenMaxN || (n_taps & 1) || n_taps > kPyrMaxTaps || level > kPyrMaxLevel || batch > 0x7fffffffll)
    return kErrUnsupported;
  if (batch == 0) return kOk;  // empty batch: no-op (NULL arrays allowed)
  if (!x || !out) return kErrArg;
  DenArgs a;
  a.F = n_taps;
  a.level = level;
  a.rule = rule;
  a.shrink = shrink;
  a.thr_ld = thr_ld;
  a.lam_scale = mult * sqrt(2.0 * log(static_cast<double>(n)));
  pad_taps(dec_lo, n_taps, a.taps[kDecLo]);
  pad_taps(dec_hi, n_taps, a.taps[kDecHi]);
  pad_taps(rec_lo, n_taps, a.taps[kRecLo]);
  pad_taps(rec_hi, n_taps, a.taps[kRecHi]);
  pyramid_lengths(static_cast<int>(n), n_taps, level, a.len);
  auto r4 = [](int m) { return (m + 3) & ~3; };
  const int E = r4(n_taps);
  int slot[2] = {0, 0};  // the longest approximation of either parity, rebuilt: one sample more
  a.total = a.len[level];
  for (int j = 1; j <= level; ++j) {
    if (a.len[j] + 1 > slot[j & 1]) slot[j & 1] = a.len[j] + 1;
    a.total += a.len[j];
  }
  a.offA = E;
  int behind = E + r4(slot[0]) + E;  // cD_2 .. cD_J behind the even slot
  for (int j = 0; j <= kPyrMaxLevel; ++j) a.doff[j] = 0;
  for (int j = 2; j <= level; ++j) {
    a.doff[j] = behind;
    behind += r4(a.len[j]);
  }
  const int sizeA = behind > r4(a.len[0]) + 2 * E ? behind : r4(a.len[0]) + 2 * E;
  a.offB = sizeA + E;
  a.doff[1] = sizeA + E + r4(slot[1]) + E;
  const size_t lds = static_cast<size_t>(a.doff[1] + r4(a.len[1])) * sizeof(float);
  allow_lds(dwt_denoise_kernel, lds);
  const int threads = threads_for(n, 4, kDenMaxThreads);  // about two output pairs of the finest level each
  hipLaunchKernelGGL(dwt_denoise_kernel, dim3(static_cast<unsigned>(batch)), dim3(threads), lds,
                     static_cast<hipStream_t>(stream), x, ld, a, thresholds, out, ld_out, info, coeffs);
  return launch_status();
}
