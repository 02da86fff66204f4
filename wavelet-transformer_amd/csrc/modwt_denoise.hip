// MODWT translation-invariant wavelet shrinkage with MAD thresholds (K26 of DESIGN.md).
//
// Coifman & Donoho's cycle spinning in its MODWT form (Percival & Walden 2000, ch. 10.5-10.6):
// modwt of a series, a noise scale from the median absolute deviation of its coefficient rows,
// pywt.threshold of every W~_j and imodwt of the shrunk rows, in ONE launch with one workgroup
// per series.  g~ = dec_lo / sqrt2, h~ = dec_hi / sqrt2, d = 2^(j-1) mod n, everything circular:
//   analysis   W~_j[t] = sum_l h~[l] V_{j-1}[(t - d l) mod n],  V_j likewise with g~.  The V row
//              stays in LDS across all levels as in K19 / K22: read the taps, barrier, write V_j
//              over V_{j-1} from registers.  Every LDS read feeds the h~ and the g~ FMA.
//   residency  unlike K23's pyramid, every W~_j is n samples long, so the J rows do not fit the
//              CU's LDS beyond small n J.  LDS holds the V row and the R coarsest rows, R =
//              min(J, kMdnLdsFloats / r4(n) - 1); the S = J - R FINEST rows spill to memory
//              (the caller's workspace, or `coeffs` itself when it is requested: they are
//              written there anyway).  They are written first and read last, so the rest of the
//              cascade lies between a spilled row's store and its load.
//   shrink     at the source where the rule allows: `fixed` needs no median and `universal`
//              only median|W~_1|, so from level 1 (fixed) or 2 (universal) on, W~_j is shrunk in
//              registers as it is produced and stored once, already shrunk; kept_j is counted
//              by wave ballots in the same pass.  Only the rows a median is taken from (every
//              row under `level`, W~_1 under `universal`) are stored raw, selected (select.hpp,
//              reading the row where it lives: a spilled row costs one extra read, no extra
//              write) and shrunk in place.
//   synthesis  in place on the V row from j = J down to 1:
//                V^_{j-1}[t] = sum_l g~[l] V^_j[(t + d l) mod n] + h~[l] W~_j[(t + d l) mod n]
//              A spilled row is first copied (coalesced) into the LDS slot of W~_J, which is
//              free from level J - 1 on, so the tap loop reads LDS at every level; with option
//              modwt_den_stage = 0 the tap loop gathers the row from memory instead
//              (profiles/r14/INDEX.md records the A/B).  Level 1 writes `denoised` from
//              registers with x[0] added: consecutive lanes store consecutive samples.
//
// The passes run on x - x[0]: the fp32-rounded h~ does not sum to exactly 0, so a large mean
// would leak into the rows the medians are taken from; x[0] returns in V_J (`coeffs`) and in the
// last synthesis step.  A constant series has W~ = 0 and comes back exactly.
//
// LDS, in floats, with np = r4(n) = n rounded up to 4 (kMdnLdsFloats = 36864, 144 KiB):
//   [0, np)                       the V row
//   [np (j - S), np (j - S + 1))  W~_j for the resident levels S < j <= J
// plus 2 480 B static: the two 256-bin histograms of the select, the kept counters, the tap
// offsets and the select's `above` word.  n = 1333, J = 7: 8 rows, 42 KiB, nothing spilled;
// n = 4096: J <= 8 resident; n = 8192: V and 3 rows; n = 16384: V and one row.
#include <math.h>

#include "common.hpp"
#include "modwt_rows.hpp"
#include "select.hpp"

// fp32 arithmetic of this file stays on the scalar VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace wtmi {

constexpr int kMdnMaxN = 16384;  // as K19: the V row and one coefficient row are 128 KiB
constexpr int kMdnMaxTaps = kModwtRowsMaxTaps;
constexpr int kMdnMaxLevel = kModwtRowsMaxLevel;
constexpr int kMdnMaxThreads = 1024;
constexpr int kMdnLdsFloats = 36864;  // dynamic LDS of a workgroup: 144 of the CU's 160 KiB

struct MdnArgs {
  int n, level, L, rule, shrink;
  int spilled;           // S: W~_1 .. W~_S live in memory, W~_{S+1} .. W~_J in LDS
  int stage;             // synthesis: copy a spilled row to LDS first (1) or gather from memory (0)
  long long thr_ld;      // row pitch of thresholds (0: one row)
  double lam_scale;      // mult * sqrt(2 ln n)
  float h[kMdnMaxTaps];  // dec_hi / sqrt2
  float g[kMdnMaxTaps];  // dec_lo / sqrt2
};

// 2^(e j / 2), e = +-1: a power of two, times sqrt2 or 1 / sqrt2 for odd j
__device__ __forceinline__ double pow2_half(int j, int e) {
  const double odd = e > 0 ? 1.4142135623730951 : 0.7071067811865476;
  return ldexp((j & 1) ? odd : 1.0, e > 0 ? (j >> 1) : -(j >> 1));
}

// In-place shrink of a raw row (LDS or memory) and its copy to `copy` (NULL: none); kept per wave.
__device__ __forceinline__ int shrink_row(float* __restrict__ row, float* __restrict__ copy, int n, float lf,
                                          int shrink) {
  int cnt = 0;
  for (int i0 = 0; i0 < n; i0 += blockDim.x) {
    const int i = i0 + threadIdx.x;
    bool keep = false;
    if (i < n) {
      const float s = shrink_one(row[i], lf, shrink, keep);
      row[i] = s;
      if (copy) copy[i] = s;
    }
    cnt += __popcll(__ballot(keep));
  }
  return cnt;
}

// One synthesis step into registers: W is the level's coefficient row, in LDS or in memory.
template <int PER>
__device__ __forceinline__ void syn_taps(const float* __restrict__ V, const float* __restrict__ W,
                                         const MdnArgs& a, const int* __restrict__ soff, float (&v)[PER]) {
  const int n = a.n;
#pragma unroll
  for (int kk = 0; kk < PER; ++kk) {
    int p = threadIdx.x + kk * blockDim.x;
    asm volatile("" : "+v"(p));  // one sample's taps at a time: no address math hoisted
    float acc = 0.f;
    if (p < n) {
      for (int l = 0; l < a.L; ++l) {
        const int o = p + soff[l];
        const int q = o >= n ? o - n : o;
        acc = fmaf(a.g[l], V[q], acc);
        acc = fmaf(a.h[l], W[q], acc);
      }
    }
    v[kk] = acc;
  }
}

template <int PER>
__global__ void __launch_bounds__(kMdnMaxThreads)
modwt_denoise_kernel(const float* __restrict__ x, long long ld, MdnArgs a, const double* __restrict__ thr,
                     float* __restrict__ out, long long ld_out, double* __restrict__ info,
                     float* __restrict__ coeffs, float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ __attribute__((aligned(16))) unsigned hist[2][256];
  __shared__ int kept_s[kWave];  // kept_s[j], j <= 62
  __shared__ int soff[kMdnMaxTaps];
  __shared__ unsigned above;
  const int tid = threadIdx.x, T = blockDim.x;
  const int n = a.n, J = a.level, L = a.L, S = a.spilled, np = (n + 3) & ~3;
  const long long b = blockIdx.x;
  float* const V = sm;
  float* const gc = coeffs ? coeffs + b * (J + 1) * n : nullptr;
  float* const spill = gc ? gc : ws + b * S * n;  // row j - 1 is W~_j, j <= S

  // ---- analysis: V_j over V_{j-1}; W~_j to its LDS slot or its spill row ----
  const float k = load_shifted(x + b * ld, V, n);
  if (tid < kWave) kept_s[tid] = 0;
  if (tid == 0) tap_offsets(1 % n, n, L, soff);
  __syncthreads();
  double sigma = __builtin_nan(""), base = 0.0;  // universal: base = lam_scale * sigma
  for (int j = 1; j <= J; ++j) {
    const bool res = j > S;
    float* const rowL = sm + np * (res ? j - S : 0);
    float* const rowG = spill + static_cast<long long>(j - 1) * n;
    float* const rowC = res && gc ? gc + static_cast<long long>(j - 1) * n : nullptr;
    const bool at_source = a.rule == kRuleFixed || (a.rule == kRuleUniversal && j >= 2);
    double lam = 0.0;
    if (at_source) lam = a.rule == kRuleFixed ? thr[b * a.thr_ld + (j - 1)] : base * pow2_half(j, -1);
    float lf = static_cast<float>(lam);
    float u[PER];
    int cnt = 0;  // per wave
#pragma unroll
    for (int kk = 0; kk < PER; ++kk) {
      int p = tid + kk * T;
      asm volatile("" : "+v"(p));  // one sample's taps at a time: no address math hoisted
      bool keep = false;
      if (p < n) {
        float aw = 0.f, av = 0.f;
        for (int l = 0; l < L; ++l) {
          const int o = p - soff[l];
          const float v = V[o < 0 ? o + n : o];
          aw = fmaf(a.h[l], v, aw);
          av = fmaf(a.g[l], v, av);
        }
        u[kk] = av;
        const float s = at_source ? shrink_one(aw, lf, a.shrink, keep) : aw;
        if (res) {
          rowL[p] = s;
          if (rowC) rowC[p] = s;
        } else {
          rowG[p] = s;
        }
      }
      if (at_source) cnt += __popcll(__ballot(keep));
    }
    __syncthreads();  // ends this level's reads of V_{j-1} and of the offsets
#pragma unroll
    for (int kk = 0; kk < PER; ++kk) {
      const int p = tid + kk * T;
      if (p < n) V[p] = u[kk];
    }
    if (tid == 0 && j < J) tap_offsets(static_cast<int>((1ll << j) % n), n, L, soff);
    if (!at_source) {
      __syncthreads();  // the raw row is complete (a spilled one: visible to the whole workgroup)
      const double s0 = (res ? median_abs(rowL, n, hist, &above) : median_abs(rowG, n, hist, &above)) / kMadScale;
      if (a.rule == kRuleLevel) {
        sigma = s0 * pow2_half(j, +1);
        lam = a.lam_scale * s0;
      } else {  // universal, j = 1
        sigma = 1.4142135623730951 * s0;
        base = a.lam_scale * sigma;
        lam = base * pow2_half(1, -1);
      }
      lf = static_cast<float>(lam);
      cnt = res ? shrink_row(rowL, rowC, n, lf, a.shrink) : shrink_row(rowG, nullptr, n, lf, a.shrink);
    }
    if ((tid & (kWave - 1)) == 0 && cnt) atomicAdd(&kept_s[j], cnt);
    if (info && tid == 0) {
      double* r = info + (b * J + (j - 1)) * 4;
      r[0] = sigma;
      r[1] = lam;
      r[3] = static_cast<double>(n);
    }
    __syncthreads();
  }
  if (info && tid >= 1 && tid <= J) info[(b * J + (tid - 1)) * 4 + 2] = static_cast<double>(kept_s[tid]);
  if (gc) {  // V~_J is never modified
    for (int i = tid; i < n; i += T) gc[static_cast<long long>(J) * n + i] = V[i] + k;
  }

  // ---- synthesis: V^_{j-1} over V^_j; the last step goes to memory ----
  float* const slot = sm + np * (J - S);  // W~_J's row: free once level J is rebuilt (S < J)
  for (int j = J; j >= 1; --j) {
    const bool res = j > S;
    const float* rowG = spill + static_cast<long long>(j - 1) * n;
    if (tid == 0) tap_offsets(static_cast<int>((1ll << (j - 1)) % n), n, L, soff);
    if (!res && a.stage) {
#pragma unroll 4
      for (int i = tid; i < n; i += T) slot[i] = rowG[i];
    }
    __syncthreads();  // V^_j, the offsets and the staged row are in place
    float v[PER];
    if (res || a.stage) {
      syn_taps<PER>(V, res ? sm + np * (j - S) : slot, a, soff, v);
    } else {
      syn_taps<PER>(V, rowG, a, soff, v);
    }
    if (j > 1) {
      __syncthreads();  // ends this level's reads of V^_j, W~_j and the offsets
#pragma unroll
      for (int kk = 0; kk < PER; ++kk) {
        const int p = tid + kk * T;
        if (p < n) V[p] = v[kk];
      }
    } else {
      float* const o = out + b * ld_out;
#pragma unroll
      for (int kk = 0; kk < PER; ++kk) {
        const int p = tid + kk * T;
        if (p < n) o[p] = v[kk] + k;
      }
    }
  }
}

// Coefficient rows that stay in LDS beside the V row: the coarsest min(level, this) levels.
inline int mdn_resident(int n, int level) {
  const int rows = kMdnLdsFloats / ((n + 3) & ~3) - 1;  // >= 1 for n <= kMdnMaxN
  return level < rows ? level : rows;
}

}  // namespace wtmi

#pragma clang attribute pop

using namespace wtmi;

extern "C" long long wtmi_modwt_denoise_workspace_bytes(long long batch, long long n, int level) {
  if (batch < 0 || n < 1 || n > kMdnMaxN || level < 1 || level > kMdnMaxLevel) return -1;
  const int S = level - mdn_resident(static_cast<int>(n), level);
  return batch * S * n * static_cast<long long>(sizeof(float));
}

extern "C" int wtmi_modwt_denoise(const float* x, long long ld, long long batch, long long n,
                                  const double* dec_lo, const double* dec_hi, int n_taps, int level, int rule,
                                  int shrink, double mult, const double* thresholds, long long thr_ld,
                                  float* out, long long ld_out, double* info, float* coeffs, void* workspace,
                                  void* stream) {
  if (batch < 0 || n < 1 || ld < n || ld_out < n || level < 1 || level > kMdnMaxLevel || n_taps < 2) return kErrArg;
  if (!dec_lo || !dec_hi) return kErrArg;
  if (rule < kRuleFixed || rule > kRuleLevel || shrink < kSoft || shrink > kGarrote) return kErrArg;
  if (!(mult >= 0.0) || !isfinite(mult)) return kErrArg;
  if (rule == kRuleFixed && (!thresholds || thr_ld < 0 || (thr_ld > 0 && thr_ld < level))) return kErrArg;
  if (n > kMdnMaxN || n_taps > kMdnMaxTaps || batch > 0x7fffffffll) return kErrUnsupported;
  if (batch == 0) return kOk;  // empty batch: no-op (NULL arrays allowed)
  if (!x || !out) return kErrArg;
  MdnArgs a{};
  a.n = static_cast<int>(n);
  a.level = level;
  a.L = n_taps;
  a.rule = rule;
  a.shrink = shrink;
  const int R = mdn_resident(a.n, level);
  a.spilled = level - R;
  a.stage = options().modwt_den_stage;
  a.thr_ld = thr_ld;
  a.lam_scale = mult * sqrt(2.0 * log(static_cast<double>(n)));
  scaled_bank(dec_lo, dec_hi, n_taps, a.h, a.g);
  if (a.spilled > 0 && !coeffs && !workspace) return kErrArg;
  const size_t lds = static_cast<size_t>(R + 1) * ((a.n + 3) & ~3) * sizeof(float);
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto launch = [&](auto kernel, int per) {
    allow_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(batch)), dim3(threads_for(a.n, per, kMdnMaxThreads)), lds,
                       st, x, ld, a, thresholds, out, ld_out, info, coeffs, static_cast<float*>(workspace));
  };
  if (a.n <= 4 * kMdnMaxThreads) launch(modwt_denoise_kernel<4>, 4);
  else if (a.n <= 8 * kMdnMaxThreads) launch(modwt_denoise_kernel<8>, 8);
  else launch(modwt_denoise_kernel<16>, 16);
  return launch_status();
}
