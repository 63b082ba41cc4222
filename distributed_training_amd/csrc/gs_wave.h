// Device helpers shared by the one-wavefront-per-row kernels (gs_eval_kernels.hip,
// gs_loss_kernels.hip): a logit load by dtype, the wave-64 butterflies and the per-lane
// balanced tree of partial sums.  HIP translation units only.
#pragma once

#include <hip/hip_runtime.h>

#include "gs_common.h"

namespace gs {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = kBlock / kWave;
constexpr int kTreeLevels = 26;  // a lane adds at most 2^25 terms: K <= 2^30 (checked by the entries)

template <int DT>
__device__ __forceinline__ float ld_logit(const void* base, int64_t i) {
  if constexpr (DT == GS_F32) {
    return static_cast<const float*>(base)[i];
  } else if constexpr (DT == GS_BF16) {
    return __uint_as_float(static_cast<uint32_t>(static_cast<const uint16_t*>(base)[i]) << 16);
  } else {
    return static_cast<float>(static_cast<const _Float16*>(base)[i]);
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v = v + __shfl_xor(v, o, kWave);  // both partners form a + b: all lanes agree
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// The pairwise sum of a lane's terms, all in registers: acc[l] holds a finished subtree of
// 2^l terms where bit l of the count is set.  cnt, the number of terms pushed so far, is
// wave-uniform (a lane past the row's end pushes an exact 0), so no branch diverges.
struct LaneTree {
  float acc[kTreeLevels];
  __device__ __forceinline__ LaneTree() {
#pragma unroll
    for (int l = 0; l < kTreeLevels; ++l) acc[l] = 0.f;
  }
  __device__ __forceinline__ void push(float e, uint32_t cnt) {
    bool placed = false;
#pragma unroll
    for (int l = 0; l < kTreeLevels; ++l) {
      if (!placed) {
        if (cnt & (1u << l)) {
          e = acc[l] + e;
        } else {
          acc[l] = e;
          placed = true;
        }
      }
    }
  }
  // folds what is left, small subtrees first (cnt = the number of terms pushed)
  __device__ __forceinline__ float fold(uint32_t cnt) const {
    float s = 0.f;
    bool any = false;
#pragma unroll
    for (int l = 0; l < kTreeLevels; ++l) {
      if (cnt & (1u << l)) {
        s = any ? acc[l] + s : acc[l];
        any = true;
      }
    }
    return s;
  }
};

}  // namespace gs
