// Row helpers of the fused pyramid-DWT kernels (dwt_tsr.hip: K17; dwt_smooth.hip: K21), whose
// level rows live in LDS with their symmetric extension written out once per level.
#pragma once

#include "common.hpp"

namespace wtmi {

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

__device__ __forceinline__ bool aligned16(const void* p) {
  return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0;
}

}  // namespace wtmi
