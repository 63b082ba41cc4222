// Adafactor's device kernels (include/gsync.h, gs_adafactor_*): factored second moments of a
// ragged list of fp32 tensors, each a batch of O x I matrices of R x C elements at arbitrary
// element strides.  Nothing here multiplies matrices: every pass is bound by its sweep over g
// (and p), and the work goes into reading each element along its unit-stride dimension and
// into sums whose order the layout alone fixes.  Every stage is one grouped launch:
// blockIdx.x indexes a task table built by gs_adafactor_layout.
//
//   af_lane_kernel<false>  matrices of <= kAfLaneElems elements and vectors: a lane owns a whole
//                          matrix (registers for the listed shapes), so row sums, column sums,
//                          both lerps and m need no cross-lane traffic; the workgroup's partial
//                          Σp², Σu² of its kBlock matrices
//   af_tile_sums           larger matrices in kAfTileRows x kAfTileCols tiles: row partials per
//                          column block, column partials per row block
//   af_tile_fold           the partials in block order, the division, the lerps, m per matrix
//   af_tile_usum           a tile's partial Σp², Σu²
//   af_sum_fold            a tensor's partial pairs -> sums[2t], sums[2t + 1]
//   af_lane_kernel<true>   the update of the lane regimes (u recomputed from g and the factors)
//   af_tile_apply          the update of the tiled regime
//
// A lane regime reads a matrix where it lies (kAfLane: channels_last filters, where consecutive
// lanes take consecutive i and every one of the R*C loads is coalesced as it stands; 1x1
// filters; vectors) or, for a contiguous batch (kAfStaged), through LDS: the workgroup's
// matrices are one contiguous span, swept with 16-B coalesced loads into a stage whose pitch
// is R*C rounded up to odd, so the lanes' read-back of element k (addresses pitch apart)
// touches 32 different banks.

#include "gs_factored.h"

namespace gs {

namespace {

struct AfArgs {
  AfHyper h;
  float rho, decay, eps2, d;
  int32_t maximize;
};

// ------------------------------------------------------------------ lane regimes
// The lane's work on its matrix.  get(r, c) is g; STEP: put(r, c, u) takes the update
// direction, else the factors advance and su gathers Σu².  R, C > 0: the shape is static, the
// factors sit in registers; 0: run-time bounds, the factors are re-read where they were stored.
template <int R, int C, bool STEP, class Get, class Put>
__device__ __forceinline__ void af_matrix(const AfDesc& d, const AfHyper& h, float* rvp, float* cvp, float& su, Get get,
                                          Put put) {
  constexpr bool ST = R > 0;
  if constexpr (R == 1 && C == 1) {
    if (d.vec) {
      const float g = get(0, 0);
      float var = rvp[0];
      if constexpr (!STEP) {
        var = ema_lerp(h.high, h.w, h.wm1, var, g * g);
        rvp[0] = var;
      }
      const float u = af_u(g, af_v_vec(h, var));
      if constexpr (STEP) put(0, 0, u);
      else su = su + u * u;
      return;
    }
  }
  const int Rr = ST ? R : d.R, Cc = ST ? C : d.C;
  float rv[ST ? R : 1], cv[ST ? C : 1];
  float rsum = 0.f;
#pragma unroll
  for (int r = 0; r < Rr; ++r) {
    float x = rvp[r];
    if constexpr (!STEP) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < Cc; ++c) {
        const float g = get(r, c);
        s = s + g * g;
      }
      x = af_factor(h, x, s, Cc);
      rvp[r] = x;
    }
    if constexpr (ST) rv[r] = x;
    rsum = rsum + x;
  }
#pragma unroll
  for (int c = 0; c < Cc; ++c) {
    float x = cvp[c];
    if constexpr (!STEP) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < Rr; ++r) {
        const float g = get(r, c);
        s = s + g * g;
      }
      x = af_factor(h, x, s, Rr);
      cvp[c] = x;
    }
    if constexpr (ST) cv[c] = x;
  }
  const float m = af_m(h, rsum, Rr);
#pragma unroll
  for (int r = 0; r < Rr; ++r) {
#pragma unroll
    for (int c = 0; c < Cc; ++c) {
      float rr, cc;
      if constexpr (ST) {
        rr = rv[r];
        cc = cv[c];
      } else {
        rr = rvp[r];
        cc = cvp[c];
      }
      const float u = af_u(get(r, c), af_v(h, rr, cc, m));
      if constexpr (STEP) put(r, c, u);
      else su = su + u * u;
    }
  }
}

template <int R, int C, bool STEP>
__device__ __forceinline__ void af_lane(const PlanArgs& A, const AfDesc& d, const AfTask& task, const AfArgs& a,
                                        float* ws, const float* sums, float* s_stage, float* s_red) {
  constexpr bool ST = R > 0;
  constexpr int RC = ST ? R * C : 1;
  const int t = task.t, tid = threadIdx.x;
  const float* G = static_cast<const float*>(slot_ptr(A, 1, t));
  float* P = static_cast<float*>(slot_ptr(A, 0, t));
  const int64_t B = static_cast<int64_t>(d.O) * d.I;
  const int64_t b = static_cast<int64_t>(task.b) + tid;
  const bool active = b < B;
  const int64_t bb = active ? b : 0;  // an idle lane's addresses stay inside the tensor
  const int64_t base = (bb / d.I) * d.so + (bb % d.I) * d.si;
  float* rvp = static_cast<float*>(slot_ptr(A, 2, t)) + bb * d.R;
  float* cvp = d.vec ? nullptr : static_cast<float*>(slot_ptr(A, 3, t)) + bb * d.C;
  float scale = 0.f;
  if constexpr (STEP) scale = af_scale(sums[2 * t], sums[2 * t + 1], d.numel, a.eps2, a.rho, a.d);
  const bool maximize = a.maximize != 0;
  float v[2] = {0.f, 0.f};  // Σp², Σu²
  bool staged = false;
  if constexpr (ST && RC > 1) staged = d.regime == kAfStaged;  // uniform over the workgroup
  if (!staged) {
    if (active) {
      auto put = [&](int r, int c, float u) {
        const int64_t e = base + r * d.sr + c * d.sc;
        P[e] = af_param(P[e], a.decay, scale, u, maximize);
      };
      if constexpr (ST) {
        float g[RC];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int c = 0; c < C; ++c) g[r * C + c] = G[base + r * d.sr + c * d.sc];
        af_matrix<R, C, STEP>(d, a.h, rvp, cvp, v[1], [&](int r, int c) { return g[r * C + c]; }, put);
      } else {
        af_matrix<R, C, STEP>(d, a.h, rvp, cvp, v[1], [&](int r, int c) { return G[base + r * d.sr + c * d.sc]; }, put);
      }
      if constexpr (!STEP) {
        const int Rr = ST ? R : d.R, Cc = ST ? C : d.C;
#pragma unroll
        for (int r = 0; r < Rr; ++r)
#pragma unroll
          for (int c = 0; c < Cc; ++c) {
            const float x = P[base + r * d.sr + c * d.sc];
            v[0] = v[0] + x * x;
          }
      }
    }
  } else if constexpr (ST && RC > 1) {
    using S = AfStage<RC>;
    const int nm = static_cast<int>(B - task.b < kBlock ? B - task.b : kBlock);  // the workgroup's matrices
    const bool vec = slot_vec(A, 0, t) && slot_vec(A, 1, t);  // a round starts on a multiple of 4 elements
    for (int h0 = 0; h0 < nm; h0 += S::mats) {  // uniform
      const int ns = nm - h0 < S::mats ? nm - h0 : S::mats;
      const int span = ns * RC;
      const int64_t e0 = (static_cast<int64_t>(task.b) + h0) * RC;
      if (h0) __syncthreads();  // the previous round's sweep is done with the stage
      for (int e = tid * 4; e < span; e += kBlock * 4) {
        float x[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
        const int n = span - e < 4 ? span - e : 4;
        if (vec && n == 4) {
          const gf4 gv = *gptr<gf4>(G + e0 + e);
#pragma unroll
          for (int k = 0; k < 4; ++k) x[k] = gv[k];
          if constexpr (!STEP) {
            const gf4 pv = *gptr<gf4>(P + e0 + e);
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = pv[k];
          }
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < n) {
              x[k] = G[e0 + e + k];
              if constexpr (!STEP) q[k] = P[e0 + e + k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < n) {
            s_stage[((e + k) / RC) * S::pitch + (e + k) % RC] = x[k];
            if constexpr (!STEP) v[0] = v[0] + q[k] * q[k];
          }
      }
      __syncthreads();
      if (tid >= h0 && tid < h0 + ns) {
        float* mine = s_stage + (tid - h0) * S::pitch;
        float g[RC];
#pragma unroll
        for (int k = 0; k < RC; ++k) g[k] = mine[k];
        af_matrix<R, C, STEP>(d, a.h, rvp, cvp, v[1], [&](int r, int c) { return g[r * C + c]; },
                              [&](int r, int c, float u) { mine[r * C + c] = u; });
      }
      if constexpr (STEP) {
        __syncthreads();  // the stage holds u now: the update goes out as the loads came in
        for (int e = tid * 4; e < span; e += kBlock * 4) {
          const int n = span - e < 4 ? span - e : 4;
          float u[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) u[k] = k < n ? s_stage[((e + k) / RC) * S::pitch + (e + k) % RC] : 0.f;
          if (vec && n == 4) {
            gf4 pv = *gptr<gf4>(P + e0 + e);
#pragma unroll
            for (int k = 0; k < 4; ++k) pv[k] = af_param(pv[k], a.decay, scale, u[k], maximize);
            *gptr_w<gf4>(P + e0 + e) = pv;
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (k < n) P[e0 + e + k] = af_param(P[e0 + e + k], a.decay, scale, u[k], maximize);
          }
        }
      }
    }
  }
  if constexpr (!STEP) {
    lars_block_sum<2>(v, s_red);
    if (tid == 0) {
      float* part = ws + d.part_off + 2 * static_cast<int64_t>(task.part);
      part[0] = v[0];
      part[1] = v[1];
    }
  }
}

template <bool STEP>
__global__ void __launch_bounds__(kBlock) af_lane_kernel(PlanArgs A, AfTables T, AfArgs a, float* ws,
                                                         const float* sums) {
  __shared__ __attribute__((aligned(16))) float s_stage[kAfStageFloats];
  __shared__ float s_red[2 * (kBlock / 64)];
  const AfTask task = T.lane[blockIdx.x];
  const AfDesc d = T.desc[task.t];
  switch (d.shape) {  // af_shape_id's list; uniform over the workgroup
    case 1: af_lane<1, 1, STEP>(A, d, task, a, ws, sums, s_stage, s_red); break;
    case 2: af_lane<3, 3, STEP>(A, d, task, a, ws, sums, s_stage, s_red); break;
    case 3: af_lane<5, 5, STEP>(A, d, task, a, ws, sums, s_stage, s_red); break;
    case 4: af_lane<7, 7, STEP>(A, d, task, a, ws, sums, s_stage, s_red); break;
    case 5: af_lane<8, 8, STEP>(A, d, task, a, ws, sums, s_stage, s_red); break;
    default: af_lane<0, 0, STEP>(A, d, task, a, ws, sums, s_stage, s_red); break;
  }
}

// ------------------------------------------------------------------ tiled regime
// A workgroup owns a kAfTileRows x kAfTileCols tile of one matrix: wave w the strip of 16 rows
// w*16.., a lane 4 consecutive columns, so a row of the tile is one 16-B access per lane.
__global__ void __launch_bounds__(kBlock) af_tile_sums(PlanArgs A, AfTables T, float* ws) {
  __shared__ float s_col[(kBlock / 64) * kAfTileCols];
  const AfTask task = T.tile[blockIdx.x];
  const AfDesc d = T.desc[task.t];
  const float* G = static_cast<const float*>(slot_ptr(A, 1, task.t));
  const AfTile x = af_tile(A, d, task, 2u);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float cacc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int k = 0; k < kAfTileRows / 4; ++k) {
    const int row = x.row0 + k;  // uniform over the wave
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < d.R) af_ld4(G + x.base + static_cast<int64_t>(row) * d.sr, x.col, d.C, x.vec, g);
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float sq = g[q] * g[q];
      cacc[q] = cacc[q] + sq;
      s = s + sq;
    }
    s = wave_sum(s);
    if (lane == 0 && row < d.R) ws[d.rp_off + (static_cast<int64_t>(task.b) * d.R + row) * d.ncb + task.j] = s;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) s_col[w * kAfTileCols + lane * 4 + q] = cacc[q];
  __syncthreads();
  const int c = task.j * kAfTileCols + static_cast<int>(threadIdx.x);
  if (c < d.C) {
    float s = s_col[threadIdx.x];
#pragma unroll
    for (int k = 1; k < kBlock / 64; ++k) s = s + s_col[k * kAfTileCols + threadIdx.x];
    ws[d.cp_off + (static_cast<int64_t>(task.b) * d.nrb + task.i) * d.C + c] = s;
  }
}

__global__ void __launch_bounds__(kBlock) af_tile_fold(PlanArgs A, AfTables T, AfArgs a, float* ws) {
  __shared__ float s_red[kBlock / 64];
  const AfTask task = T.fold[blockIdx.x];
  const AfDesc d = T.desc[task.t];
  float* rvp = static_cast<float*>(slot_ptr(A, 2, task.t)) + static_cast<int64_t>(task.b) * d.R;
  float* cvp = static_cast<float*>(slot_ptr(A, 3, task.t)) + static_cast<int64_t>(task.b) * d.C;
  float acc[1] = {0.f};
  for (int r = threadIdx.x; r < d.R; r += kBlock) {
    const float* part = ws + d.rp_off + (static_cast<int64_t>(task.b) * d.R + r) * d.ncb;
    float s = part[0];
    for (int j = 1; j < d.ncb; ++j) s = s + part[j];
    const float x = af_factor(a.h, rvp[r], s, d.C);
    rvp[r] = x;
    acc[0] = acc[0] + x;
  }
  for (int c = threadIdx.x; c < d.C; c += kBlock) {
    const float* part = ws + d.cp_off + static_cast<int64_t>(task.b) * d.nrb * d.C + c;
    float s = part[0];
    for (int i = 1; i < d.nrb; ++i) s = s + part[static_cast<int64_t>(i) * d.C];
    cvp[c] = af_factor(a.h, cvp[c], s, d.R);
  }
  lars_block_sum<1>(acc, s_red);
  if (threadIdx.x == 0) ws[d.m_off + task.b] = af_m(a.h, acc[0], d.R);
}

// the tile's update directions: STEP applies them, else their squares and p's are summed
template <bool STEP>
__global__ void __launch_bounds__(kBlock) af_tile_update(PlanArgs A, AfTables T, AfArgs a, float* ws,
                                                         const float* sums) {
  __shared__ float s_red[2 * (kBlock / 64)];
  const AfTask task = T.tile[blockIdx.x];
  const AfDesc d = T.desc[task.t];
  const float* G = static_cast<const float*>(slot_ptr(A, 1, task.t));
  float* P = static_cast<float*>(slot_ptr(A, 0, task.t));
  const float* rvp = static_cast<const float*>(slot_ptr(A, 2, task.t)) + static_cast<int64_t>(task.b) * d.R;
  const float* cvp = static_cast<const float*>(slot_ptr(A, 3, task.t)) + static_cast<int64_t>(task.b) * d.C;
  const AfTile x = af_tile(A, d, task, 3u);
  const float m = ws[d.m_off + task.b];
  float scale = 0.f;
  if constexpr (STEP) scale = af_scale(sums[2 * task.t], sums[2 * task.t + 1], d.numel, a.eps2, a.rho, a.d);
  const bool maximize = a.maximize != 0;
  float cv[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) cv[q] = x.col + q < d.C ? cvp[x.col + q] : 1.f;
  float v[2] = {0.f, 0.f};
#pragma unroll 2
  for (int k = 0; k < kAfTileRows / 4; ++k) {
    const int row = x.row0 + k;
    if (row >= d.R) break;  // uniform over the wave; no barrier inside
    const int64_t ro = x.base + static_cast<int64_t>(row) * d.sr;
    const float rv = rvp[row];
    float g[4], p[4];
    af_ld4(G + ro, x.col, d.C, x.vec, g);
    af_ld4(P + ro, x.col, d.C, x.vec, p);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (x.col + q < d.C) {
        const float u = af_u(g[q], af_v(a.h, rv, cv[q], m));
        if constexpr (STEP) {
          p[q] = af_param(p[q], a.decay, scale, u, maximize);
        } else {
          v[0] = v[0] + p[q] * p[q];
          v[1] = v[1] + u * u;
        }
      }
    }
    if constexpr (STEP) {
      if (x.vec && x.col + 4 <= d.C) {
        gf4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = p[q];
        *gptr_w<gf4>(P + ro + x.col) = o;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (x.col + q < d.C) P[ro + x.col + q] = p[q];
      }
    }
  }
  if constexpr (!STEP) {
    lars_block_sum<2>(v, s_red);
    if (threadIdx.x == 0) {
      float* part = ws + d.part_off + 2 * static_cast<int64_t>(task.part);
      part[0] = v[0];
      part[1] = v[1];
    }
  }
}

// one workgroup per tensor: thread k adds the pairs k, k + 256, .. in order, then the wave tree
// and the 4 waves in order
__global__ void __launch_bounds__(kBlock) af_sum_fold(AfTables T, const float* ws, float* sums) {
  __shared__ float s_red[2 * (kBlock / 64)];
  const AfDesc d = T.desc[blockIdx.x];
  const float* part = ws + d.part_off;
  float v[2] = {0.f, 0.f};
  for (int k = threadIdx.x; k < d.nparts; k += kBlock) {
    v[0] = v[0] + part[2 * static_cast<int64_t>(k)];
    v[1] = v[1] + part[2 * static_cast<int64_t>(k) + 1];
  }
  lars_block_sum<2>(v, s_red);
  if (threadIdx.x == 0) {
    sums[2 * blockIdx.x] = v[0];
    sums[2 * blockIdx.x + 1] = v[1];
  }
}

}  // namespace

// desc | lane | tile | fold in one allocation
int hip_adafactor_upload(gs_plan* p, const AfTaskLists& l) {
  DeviceGuard g(p->device);
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const std::vector<AfTask>* lists[3] = {&l.lane, &l.tile, &l.fold};
  size_t offs[4];
  offs[0] = al(sizeof(AfDesc) * p->af.size());
  for (int i = 0; i < 3; ++i) offs[i + 1] = offs[i] + al(sizeof(AfTask) * lists[i]->size());
  if (p->d_af) {
    HIP_RET(hipDeviceSynchronize());  // a launch in flight may still read the old tables
    HIP_RET(hipFree(p->d_af));
    p->d_af = nullptr;
  }
  p->af_tab = AfTables{};
  if (p->af.empty()) return GS_OK;
  char* dmem = nullptr;
  HIP_RET(hipMalloc(reinterpret_cast<void**>(&dmem), std::max<size_t>(offs[3], 256)));
  p->d_af = dmem;
  HIP_RET(hipMemcpy(dmem, p->af.data(), sizeof(AfDesc) * p->af.size(), hipMemcpyHostToDevice));
  for (int i = 0; i < 3; ++i)
    if (!lists[i]->empty())
      HIP_RET(hipMemcpy(dmem + offs[i], lists[i]->data(), sizeof(AfTask) * lists[i]->size(), hipMemcpyHostToDevice));
  AfTables& T = p->af_tab;
  T.desc = reinterpret_cast<const AfDesc*>(dmem);
  T.lane = reinterpret_cast<const AfTask*>(dmem + offs[0]);
  T.tile = reinterpret_cast<const AfTask*>(dmem + offs[1]);
  T.fold = reinterpret_cast<const AfTask*>(dmem + offs[2]);
  T.n_lane = static_cast<int32_t>(l.lane.size());
  T.n_tile = static_cast<int32_t>(l.tile.size());
  T.n_fold = static_cast<int32_t>(l.fold.size());
  return GS_OK;
}

int hip_adafactor_stats(gs_plan* p, const AfHyper& h, float* sums, float* ws, void* stream) {
  DeviceGuard g(p->device);
  const AfTables& T = p->af_tab;
  const AfArgs a{h, 0.f, 1.f, 0.f, 1.f, 0};
  const PlanArgs A = p->args();
  const float* none = nullptr;
  GS_TRY_RET(af_launch(p, GS_OP_ADAFACTOR_STATS, T.n_lane, stream, af_lane_kernel<false>, A, T, a, ws, none));
  GS_TRY_RET(af_launch(p, GS_OP_ADAFACTOR_STATS, T.n_tile, stream, af_tile_sums, A, T, ws));
  GS_TRY_RET(af_launch(p, GS_OP_ADAFACTOR_STATS, T.n_fold, stream, af_tile_fold, A, T, a, ws));
  GS_TRY_RET(af_launch(p, GS_OP_ADAFACTOR_STATS, T.n_tile, stream, af_tile_update<false>, A, T, a, ws, none));
  return af_launch(p, GS_OP_ADAFACTOR_STATS, p->n, stream, af_sum_fold, T, static_cast<const float*>(ws), sums);
}

int hip_adafactor_step(gs_plan* p, const AfHyper& h, float rho, float decay, float eps2, float d, int maximize,
                       const float* sums, const float* ws, void* stream) {
  DeviceGuard g(p->device);
  const AfTables& T = p->af_tab;
  const AfArgs a{h, rho, decay, eps2, d, maximize};
  const PlanArgs A = p->args();
  float* w = const_cast<float*>(ws);  // the update kernels only read it
  GS_TRY_RET(af_launch(p, GS_OP_ADAFACTOR_STEP, T.n_lane, stream, af_lane_kernel<true>, A, T, a, w, sums));
  return af_launch(p, GS_OP_ADAFACTOR_STEP, T.n_tile, stream, af_tile_update<true>, A, T, a, w, sums);
}

}  // namespace gs
