// What the factored optimizers' kernel files share (gs_adafactor_kernels.hip, gs_came_kernels.hip):
// the LDS stage of the kAfStaged regime, a workgroup's view of its tile in the tiled regime, and
// the grouped launch through the plan's stream bookkeeping.
#pragma once

#include "gs_seg.h"

namespace gs {
namespace {

// the stage of kAfStaged: kBlock matrices of 7x7 (pitch 49); a shape whose kBlock matrices do
// not fit (8x8: pitch 65) goes through it in two halves of 128
constexpr int kAfStageFloats = kBlock * 49;
template <int RC>
struct AfStage {
  static constexpr int pitch = (RC & 1) ? RC : RC + 1;
  static constexpr int mats = kBlock * pitch <= kAfStageFloats ? kBlock : kBlock / 2;
  static_assert(mats * pitch <= kAfStageFloats, "the stage holds a round of matrices");
};

// ------------------------------------------------------------------ tiled regime
// A workgroup owns a kAfTileRows x kAfTileCols tile of one matrix: wave w the strip of 16 rows
// w*16.., a lane 4 consecutive columns, so a row of the tile is one 16-B access per lane.
struct AfTile {
  int64_t base;   // the matrix's first element
  int row0, col;  // the wave's first row, the lane's first column
  bool vec;       // 16-B accesses: aligned slots, every row on a multiple of 4 elements
};
__device__ __forceinline__ AfTile af_tile(const PlanArgs& A, const AfDesc& d, const AfTask& task, uint32_t slots) {
  AfTile x;
  x.base = static_cast<int64_t>(task.b / d.I) * d.so + static_cast<int64_t>(task.b % d.I) * d.si;
  x.row0 = task.i * kAfTileRows + static_cast<int>(threadIdx.x >> 6) * (kAfTileRows / 4);
  x.col = task.j * kAfTileCols + static_cast<int>(threadIdx.x & 63) * 4;
  x.vec = (A.align[task.t] & slots) == slots && ((d.so | d.si | d.sr) & 3) == 0;
  return x;
}
// 4 columns of a row from column c; past the row's end: zeros
__device__ __forceinline__ void af_ld4(const float* row, int c, int C, bool vec, float (&x)[4]) {
  if (vec && c + 4 <= C) {
    const gf4 v = *gptr<gf4>(row + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = v[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = c + k < C ? row[c + k] : 0.f;
  }
}

// One grouped launch through the plan's stream bookkeeping (as PowerSGD's): pointer-table
// flush, the launch timer's event pair (one record of `kind`), the last-stream mark.
template <class K, class... Args>
int af_launch(gs_plan* p, int kind, int grid, void* stream, K kernel, Args... args) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (grid <= 0) return GS_OK;
  GS_TRY_RET(hip_plan_flush(p, stream));
  const bool capturing = stream_capturing(s);
  const int nslots = capturing ? 0 : static_cast<int>(p->timer_ev.size() / 2);
  const int tk = p->timer_next;
  if (nslots)
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, static_cast<hipEvent_t>(p->timer_ev[2 * tk]),
                          static_cast<hipEvent_t>(p->timer_ev[2 * tk + 1]), 0, args...);
  else
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, args...);
  HIP_RET(hipGetLastError());
  if (nslots) {
    p->timer_kind[tk] = kind;
    p->timer_next = (tk + 1) % nslots;
    p->timer_count = std::min(p->timer_count + 1, nslots);
  }
  p->last_stream = stream;
  p->last_captured = capturing;
  return GS_OK;
}

}  // namespace
}  // namespace gs
