// CAME's device kernels (include/gsync.h, gs_came_*): Adafactor's factored second moment, a
// full-size momentum m of the clipped direction û, and a second pair of factors over the
// instability (û - m)², for a ragged list of fp32 tensors in the descriptors, regimes and task
// tables of gs_adafactor_layout.  Nothing here multiplies matrices, so no matrix instruction
// fits: every pass is bound by its sweep over g, m and p, and the work goes into reading each
// element along its unit-stride dimension and into sums whose order the layout alone fixes.
// û exists only once the tensor-wide Σu² is known, and the second factors only once every û of
// a matrix is, so a step is three dependent stages.  Every launch is grouped: blockIdx.x
// indexes a task table.
//
//   gs_came_stats    came_lane_kernel<false>  stage 1 of the lane regimes (matrices of <= 64
//                                             elements, vectors): r, c advance in registers,
//                                             the workgroup's partial Σu²
//                    came_tile_sums           tiled regime: row / column partials of g² + eps1
//                    came_tile_fold           partials in block order, the β2 EMAs, mean(r)
//                    came_tile_usum           a tile's partial Σu²
//                    came_sum_fold            a tensor's partials -> sums[t]
//   gs_came_moment   came_tile_moment         stage 2, tiled: reads g and m, writes m, leaves the
//                                             row / column partials of q = (û - m)² + eps2
//                    came_tile_fold           the β3 EMAs, mean(R)
//   gs_came_step     came_lane_kernel<true>   stages 2 and 3 of the lane regimes in one launch:
//                                             after Σu² a lane needs nothing from another lane
//                    came_tile_apply          stage 3, tiled: reads m and p, writes p
//
// 9 launches for a list with both kinds of tensors, 3 for lane regimes only (lane stats, sum
// fold, lane update), 7 for tiled tensors only; no atomics, nothing read back by the host.
//
// The fused lane launch keeps the matrix in registers: x[] holds g and then the new m, and the
// row / column sums of q are taken while m advances, so g, m and p are each read once and m and
// p written once.  A contiguous batch (kAfStaged) moves through ONE LDS stage of kBlock odd-
// pitched matrices (49 KiB) that g, the old m, the new m and the update direction occupy in
// turn, each swept with 16-B coalesced accesses: three workgroups fit a CU's 160 KiB, where a
// stage per stream (g and m: 98 KiB) would leave one.  channels_last filters and vectors are
// read where they lie (consecutive lanes, consecutive addresses).  A shape outside
// af_shape_id's list is walked with run-time bounds and recomputes an element's (m, q) per
// pass instead of indexing registers dynamically.

#include "gs_factored.h"

namespace gs {

namespace {

// ------------------------------------------------------------------ lane regimes
// Stage 1 on the lane's matrix: get(r, c) is g; r and c advance where they are stored, su
// gathers Σu².  R, C > 0: a static shape; 0: run-time bounds, factors re-read from memory.
template <int R, int C, class Get>
__device__ __forceinline__ void came_lane_stats(const AfDesc& d, const CameHyper& h, float* rvp, float* cvp, float& su,
                                                Get get) {
  constexpr bool ST = R > 0;
  if constexpr (R == 1 && C == 1) {
    if (d.vec) {
      const float g = get(0, 0);
      const float v = came_ema(rvp[0], came_sq(g, h.eps1), h.b2, h.omb2);
      rvp[0] = v;
      const float u = g * came_cf(v);
      su = su + u * u;
      return;
    }
  }
  const int Rr = ST ? R : d.R, Cc = ST ? C : d.C;
  float rv[ST ? R : 1], cf[ST ? C : 1];
  float rsum = 0.f;
#pragma unroll
  for (int r = 0; r < Rr; ++r) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < Cc; ++c) s = s + came_sq(get(r, c), h.eps1);
    const float x = came_factor(rvp[r], s, Cc, h.b2, h.omb2);
    rvp[r] = x;
    if constexpr (ST) rv[r] = x;
    rsum = rsum + x;
  }
#pragma unroll
  for (int c = 0; c < Cc; ++c) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < Rr; ++r) s = s + came_sq(get(r, c), h.eps1);
    const float x = came_factor(cvp[c], s, Rr, h.b2, h.omb2);
    cvp[c] = x;
    if constexpr (ST) cf[c] = came_cf(x);
  }
  const float mean = came_mean(rsum, Rr);
#pragma unroll
  for (int r = 0; r < Rr; ++r) {
    const float rf = came_rf(ST ? rv[r] : rvp[r], mean);
#pragma unroll
    for (int c = 0; c < Cc; ++c) {
      const float u = came_dir(get(r, c), rf, ST ? cf[c] : came_cf(cvp[c]));
      su = su + u * u;
    }
  }
}

// Stages 2 and 3 of a static shape, up to the update direction: x[] comes in as g and leaves
// as the new m (getm(k) is the old one); R and C advance where they are stored; Rf, Cf are the
// factors of upd = m * (Rf * Cf).
template <int R, int C, class GetM>
__device__ __forceinline__ void came_advance(const CameHyper& h, float denom, const float* rvp, const float* cvp,
                                             float* Rvp, float* Cvp, float (&x)[R * C], float (&Rf)[R], float (&Cf)[C],
                                             GetM getm) {
  float rf[R], cf[C], qc[C];
  float rsum = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    rf[r] = rvp[r];
    rsum = rsum + rf[r];
  }
  const float mean = came_mean(rsum, R);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    cf[c] = came_cf(cvp[c]);
    qc[c] = 0.f;
  }
  float Rsum = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float f = came_rf(rf[r], mean);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int k = r * C + c;
      const float uh = came_dir(x[k], f, cf[c]) / denom;
      const float m = came_ema(getm(k), uh, h.b1, h.omb1);
      const float q = came_res(uh, m, h.eps2);
      s = s + q;
      qc[c] = qc[c] + q;
      x[k] = m;
    }
    const float X = came_factor(Rvp[r], s, C, h.b3, h.omb3);
    Rvp[r] = X;
    Rf[r] = X;
    Rsum = Rsum + X;
  }
  const float Mean = came_mean(Rsum, R);
#pragma unroll
  for (int r = 0; r < R; ++r) Rf[r] = came_rf(Rf[r], Mean);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float X = came_factor(Cvp[c], qc[c], R, h.b3, h.omb3);
    Cvp[c] = X;
    Cf[c] = came_cf(X);
  }
}

// ... and of any other shape of at most kAfLaneElems elements, where the matrix lies: an
// element's (m, q) is recomputed in each of the three passes (the same operations, so the same
// bits), and m is written in the last one only
__device__ __forceinline__ void came_lane_dyn(const AfDesc& d, const CameHyper& h, float denom, const float* G, float* M,
                                              float* P, int64_t base, const float* rvp, const float* cvp, float* Rvp,
                                              float* Cvp) {
  float rsum = 0.f;
  for (int r = 0; r < d.R; ++r) rsum = rsum + rvp[r];
  const float mean = came_mean(rsum, d.R);
  auto elem = [&](int r, int c, float& m) {
    const int64_t e = base + r * d.sr + c * d.sc;
    const float uh = came_dir(G[e], came_rf(rvp[r], mean), came_cf(cvp[c])) / denom;
    m = came_ema(M[e], uh, h.b1, h.omb1);
    return came_res(uh, m, h.eps2);
  };
  float m, Rsum = 0.f;
  for (int r = 0; r < d.R; ++r) {
    float s = 0.f;
    for (int c = 0; c < d.C; ++c) s = s + elem(r, c, m);
    const float X = came_factor(Rvp[r], s, d.C, h.b3, h.omb3);
    Rvp[r] = X;
    Rsum = Rsum + X;
  }
  for (int c = 0; c < d.C; ++c) {
    float s = 0.f;
    for (int r = 0; r < d.R; ++r) s = s + elem(r, c, m);
    Cvp[c] = came_factor(Cvp[c], s, d.R, h.b3, h.omb3);
  }
  const float Mean = came_mean(Rsum, d.R);
  for (int r = 0; r < d.R; ++r) {
    const float Rf = came_rf(Rvp[r], Mean);
    for (int c = 0; c < d.C; ++c) {
      const int64_t e = base + r * d.sr + c * d.sc;
      elem(r, c, m);
      M[e] = m;
      P[e] = came_param(h, P[e], came_dir(m, Rf, came_cf(Cvp[c])));
    }
  }
}

// The workgroup's span of `span` elements from element e0 of a contiguous batch, global ->
// stage (a matrix every S::pitch floats), in 16-B accesses where the slot is aligned.
template <int RC>
__device__ __forceinline__ void came_stage_in(const float* src, int64_t e0, int span, bool vec, float* s_stage) {
  using S = AfStage<RC>;
  for (int e = threadIdx.x * 4; e < span; e += kBlock * 4) {
    const int n = span - e < 4 ? span - e : 4;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec && n == 4) {
      const gf4 v = *gptr<gf4>(src + e0 + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = v[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) x[k] = src[e0 + e + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) s_stage[((e + k) / RC) * S::pitch + (e + k) % RC] = x[k];
  }
}
// ... and stage -> global as the loads came in: dst = f(dst, staged) (READ) or f(0, staged)
template <int RC, bool READ, class F>
__device__ __forceinline__ void came_stage_out(float* dst, int64_t e0, int span, bool vec, const float* s_stage, F f) {
  using S = AfStage<RC>;
  for (int e = threadIdx.x * 4; e < span; e += kBlock * 4) {
    const int n = span - e < 4 ? span - e : 4;
    float u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = k < n ? s_stage[((e + k) / RC) * S::pitch + (e + k) % RC] : 0.f;
    if (vec && n == 4) {
      gf4 v = {0.f, 0.f, 0.f, 0.f};
      if constexpr (READ) v = *gptr<gf4>(dst + e0 + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = f(v[k], u[k]);
      *gptr_w<gf4>(dst + e0 + e) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) dst[e0 + e + k] = f(READ ? dst[e0 + e + k] : 0.f, u[k]);
    }
  }
}

template <int R, int C, bool STEP>
__device__ __forceinline__ void came_lane(const PlanArgs& A, const AfDesc& d, const AfTask& task, const CameHyper& h,
                                          float* ws, const float* sums, float* s_stage, float* s_red) {
  constexpr bool ST = R > 0;
  constexpr int RC = ST ? R * C : 1;
  const int t = task.t, tid = threadIdx.x;
  const float* G = static_cast<const float*>(slot_ptr(A, 1, t));
  float* P = static_cast<float*>(slot_ptr(A, 0, t));
  float* M = static_cast<float*>(slot_ptr(A, 4, t));
  const int64_t B = static_cast<int64_t>(d.O) * d.I;
  const int64_t b = static_cast<int64_t>(task.b) + tid;
  const bool active = b < B;
  const int64_t bb = active ? b : 0;  // an idle lane's addresses stay inside the tensor
  const int64_t base = (bb / d.I) * d.so + (bb % d.I) * d.si;
  float* rvp = static_cast<float*>(slot_ptr(A, 2, t)) + bb * d.R;
  float* cvp = d.vec ? nullptr : static_cast<float*>(slot_ptr(A, 3, t)) + bb * d.C;
  float* Rvp = d.vec ? nullptr : static_cast<float*>(slot_ptr(A, 5, t)) + bb * d.R;
  float* Cvp = d.vec ? nullptr : static_cast<float*>(slot_ptr(A, 6, t)) + bb * d.C;
  float denom = 1.f;
  if constexpr (STEP) denom = came_denom(sums[t], d.numel, h.d);
  float v[1] = {0.f};  // Σu²
  bool staged = false;
  if constexpr (ST && RC > 1) staged = d.regime == kAfStaged;  // uniform over the workgroup
  if (!staged) {
    if (active) {
      if constexpr (!ST) {
        if constexpr (STEP)
          came_lane_dyn(d, h, denom, G, M, P, base, rvp, cvp, Rvp, Cvp);
        else
          came_lane_stats<0, 0>(d, h, rvp, cvp, v[0], [&](int r, int c) { return G[base + r * d.sr + c * d.sc]; });
      } else {
        float x[RC];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int c = 0; c < C; ++c) x[r * C + c] = G[base + r * d.sr + c * d.sc];
        if constexpr (!STEP) {
          came_lane_stats<R, C>(d, h, rvp, cvp, v[0], [&](int r, int c) { return x[r * C + c]; });
        } else {
          if (RC == 1 && d.vec) {  // not factored: upd = m
            const float uh = x[0] * came_cf(rvp[0]) / denom;
            const float m = came_ema(M[base], uh, h.b1, h.omb1);
            M[base] = m;
            P[base] = came_param(h, P[base], m);
          } else {
            float Rf[R], Cf[C];
            came_advance<R, C>(h, denom, rvp, cvp, Rvp, Cvp, x, Rf, Cf,
                               [&](int k) { return M[base + (k / C) * d.sr + (k % C) * d.sc]; });
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
              for (int c = 0; c < C; ++c) {
                const int64_t e = base + r * d.sr + c * d.sc;
                M[e] = x[r * C + c];
                P[e] = came_param(h, P[e], came_dir(x[r * C + c], Rf[r], Cf[c]));
              }
          }
        }
      }
    }
  } else if constexpr (ST && RC > 1) {
    using S = AfStage<RC>;
    const int nm = static_cast<int>(B - task.b < kBlock ? B - task.b : kBlock);  // the workgroup's matrices
    for (int h0 = 0; h0 < nm; h0 += S::mats) {  // uniform; a round starts on a multiple of 4 elements
      const int ns = nm - h0 < S::mats ? nm - h0 : S::mats;
      const int span = ns * RC;
      const int64_t e0 = (static_cast<int64_t>(task.b) + h0) * RC;
      const bool on = tid >= h0 && tid < h0 + ns;  // the lane's matrix is in this round
      float* mine = s_stage + (on ? tid - h0 : 0) * S::pitch;
      if (h0) __syncthreads();  // the previous round's sweep is done with the stage
      came_stage_in<RC>(G, e0, span, slot_vec(A, 1, t), s_stage);
      __syncthreads();
      float x[RC];
      if (on) {
#pragma unroll
        for (int k = 0; k < RC; ++k) x[k] = mine[k];
        if constexpr (!STEP) came_lane_stats<R, C>(d, h, rvp, cvp, v[0], [&](int r, int c) { return x[r * C + c]; });
      }
      if constexpr (STEP) {
        float Rf[R], Cf[C];
        __syncthreads();  // g is in registers: the stage takes the old m
        came_stage_in<RC>(M, e0, span, slot_vec(A, 4, t), s_stage);
        __syncthreads();
        if (on) {
          came_advance<R, C>(h, denom, rvp, cvp, Rvp, Cvp, x, Rf, Cf, [&](int k) { return mine[k]; });
#pragma unroll
          for (int k = 0; k < RC; ++k) mine[k] = x[k];
        }
        __syncthreads();  // the stage holds the new m: it goes out as the loads came in
        came_stage_out<RC, false>(M, e0, span, slot_vec(A, 4, t), s_stage, [](float, float m) { return m; });
        __syncthreads();
        if (on) {
#pragma unroll
          for (int k = 0; k < RC; ++k) mine[k] = came_dir(x[k], Rf[k / C], Cf[k % C]);
        }
        __syncthreads();  // ... and now the update direction
        came_stage_out<RC, true>(P, e0, span, slot_vec(A, 0, t), s_stage,
                                 [&](float p, float upd) { return came_param(h, p, upd); });
      }
    }
  }
  if constexpr (!STEP) {
    lars_block_sum<1>(v, s_red);
    if (tid == 0) ws[d.part_off + task.part] = v[0];
  }
}

template <bool STEP>
__global__ void __launch_bounds__(kBlock) came_lane_kernel(PlanArgs A, AfTables T, CameHyper h, float* ws,
                                                           const float* sums) {
  __shared__ __attribute__((aligned(16))) float s_stage[kAfStageFloats];
  __shared__ float s_red[kBlock / 64];
  const AfTask task = T.lane[blockIdx.x];
  const AfDesc d = T.desc[task.t];
  switch (d.shape) {  // af_shape_id's list; uniform over the workgroup
    case 1: came_lane<1, 1, STEP>(A, d, task, h, ws, sums, s_stage, s_red); break;
    case 2: came_lane<3, 3, STEP>(A, d, task, h, ws, sums, s_stage, s_red); break;
    case 3: came_lane<5, 5, STEP>(A, d, task, h, ws, sums, s_stage, s_red); break;
    case 4: came_lane<7, 7, STEP>(A, d, task, h, ws, sums, s_stage, s_red); break;
    case 5: came_lane<8, 8, STEP>(A, d, task, h, ws, sums, s_stage, s_red); break;
    default: came_lane<0, 0, STEP>(A, d, task, h, ws, sums, s_stage, s_red); break;
  }
}

// ------------------------------------------------------------------ tiled regime
// The tile's elements s (MOMENT: q = (û - m)² + eps2 while m advances; else g² + eps1) summed
// into a row partial per column block and a column partial per row block.
template <bool MOMENT>
__global__ void __launch_bounds__(kBlock) came_tile_sums(PlanArgs A, AfTables T, CameHyper h, float* ws,
                                                         const float* sums) {
  __shared__ float s_col[(kBlock / 64) * kAfTileCols];
  const AfTask task = T.tile[blockIdx.x];
  const AfDesc d = T.desc[task.t];
  const float* G = static_cast<const float*>(slot_ptr(A, 1, task.t));
  float* M = static_cast<float*>(slot_ptr(A, 4, task.t));
  const AfTile x = af_tile(A, d, task, MOMENT ? 18u : 2u);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* rvp = static_cast<const float*>(slot_ptr(A, 2, task.t)) + static_cast<int64_t>(task.b) * d.R;
  float denom = 1.f, mean = 1.f;
  float cf[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (MOMENT) {
    const float* cvp = static_cast<const float*>(slot_ptr(A, 3, task.t)) + static_cast<int64_t>(task.b) * d.C;
    denom = came_denom(sums[task.t], d.numel, h.d);
    mean = ws[d.m_off + task.b];
#pragma unroll
    for (int q = 0; q < 4; ++q) cf[q] = x.col + q < d.C ? came_cf(cvp[x.col + q]) : 0.f;
  }
  float cacc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int k = 0; k < kAfTileRows / 4; ++k) {
    const int row = x.row0 + k;  // uniform over the wave
    float s = 0.f;
    if (row < d.R) {
      const int64_t ro = x.base + static_cast<int64_t>(row) * d.sr;
      float g[4], m[4];
      af_ld4(G + ro, x.col, d.C, x.vec, g);
      float rf = 0.f;
      if constexpr (MOMENT) {
        af_ld4(M + ro, x.col, d.C, x.vec, m);
        rf = came_rf(rvp[row], mean);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (x.col + q < d.C) {
          float sq;
          if constexpr (MOMENT) {
            const float uh = came_dir(g[q], rf, cf[q]) / denom;
            m[q] = came_ema(m[q], uh, h.b1, h.omb1);
            sq = came_res(uh, m[q], h.eps2);
          } else {
            sq = came_sq(g[q], h.eps1);
          }
          cacc[q] = cacc[q] + sq;
          s = s + sq;
        }
      if constexpr (MOMENT) {
        if (x.vec && x.col + 4 <= d.C) {
          gf4 o;
#pragma unroll
          for (int q = 0; q < 4; ++q) o[q] = m[q];
          *gptr_w<gf4>(M + ro + x.col) = o;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (x.col + q < d.C) M[ro + x.col + q] = m[q];
        }
      }
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

// a matrix's partials in block order, the EMAs onto slots (sr, sc) with weight b, the row
// factor's mean
__global__ void __launch_bounds__(kBlock) came_tile_fold(PlanArgs A, AfTables T, int sr, int sc, float b, float omb,
                                                         float* ws) {
  __shared__ float s_red[kBlock / 64];
  const AfTask task = T.fold[blockIdx.x];
  const AfDesc d = T.desc[task.t];
  float* rvp = static_cast<float*>(slot_ptr(A, sr, task.t)) + static_cast<int64_t>(task.b) * d.R;
  float* cvp = static_cast<float*>(slot_ptr(A, sc, task.t)) + static_cast<int64_t>(task.b) * d.C;
  float acc[1] = {0.f};
  for (int r = threadIdx.x; r < d.R; r += kBlock) {
    const float* part = ws + d.rp_off + (static_cast<int64_t>(task.b) * d.R + r) * d.ncb;
    float s = part[0];
    for (int j = 1; j < d.ncb; ++j) s = s + part[j];
    const float x = came_factor(rvp[r], s, d.C, b, omb);
    rvp[r] = x;
    acc[0] = acc[0] + x;
  }
  for (int c = threadIdx.x; c < d.C; c += kBlock) {
    const float* part = ws + d.cp_off + static_cast<int64_t>(task.b) * d.nrb * d.C + c;
    float s = part[0];
    for (int i = 1; i < d.nrb; ++i) s = s + part[static_cast<int64_t>(i) * d.C];
    cvp[c] = came_factor(cvp[c], s, d.R, b, omb);
  }
  lars_block_sum<1>(acc, s_red);
  if (threadIdx.x == 0) ws[d.m_off + task.b] = came_mean(acc[0], d.R);
}

// the tile's x * (rf * cf): APPLY: x = m, the factors R and C, p takes the update; else
// x = g, the factors r and c, and the squares are summed
template <bool APPLY>
__global__ void __launch_bounds__(kBlock) came_tile_dir(PlanArgs A, AfTables T, CameHyper h, float* ws) {
  __shared__ float s_red[kBlock / 64];
  const AfTask task = T.tile[blockIdx.x];
  const AfDesc d = T.desc[task.t];
  const float* X = static_cast<const float*>(slot_ptr(A, APPLY ? 4 : 1, task.t));
  float* P = static_cast<float*>(slot_ptr(A, 0, task.t));
  const float* rvp = static_cast<const float*>(slot_ptr(A, APPLY ? 5 : 2, task.t)) + static_cast<int64_t>(task.b) * d.R;
  const float* cvp = static_cast<const float*>(slot_ptr(A, APPLY ? 6 : 3, task.t)) + static_cast<int64_t>(task.b) * d.C;
  const AfTile x = af_tile(A, d, task, APPLY ? 17u : 2u);
  const float mean = ws[d.m_off + task.b];
  float cf[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) cf[q] = x.col + q < d.C ? came_cf(cvp[x.col + q]) : 0.f;
  float v[1] = {0.f};
#pragma unroll 2
  for (int k = 0; k < kAfTileRows / 4; ++k) {
    const int row = x.row0 + k;
    if (row >= d.R) break;  // uniform over the wave; no barrier inside
    const int64_t ro = x.base + static_cast<int64_t>(row) * d.sr;
    const float rf = came_rf(rvp[row], mean);
    float a[4], p[4];
    af_ld4(X + ro, x.col, d.C, x.vec, a);
    if constexpr (APPLY) af_ld4(P + ro, x.col, d.C, x.vec, p);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (x.col + q < d.C) {
        const float u = came_dir(a[q], rf, cf[q]);
        if constexpr (APPLY) p[q] = came_param(h, p[q], u);
        else v[0] = v[0] + u * u;
      }
    if constexpr (APPLY) {
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
  if constexpr (!APPLY) {
    lars_block_sum<1>(v, s_red);
    if (threadIdx.x == 0) ws[d.part_off + task.part] = v[0];
  }
}

// one workgroup per tensor: thread k adds the partials k, k + 256, .. in order, then the wave
// tree and the 4 waves in order
__global__ void __launch_bounds__(kBlock) came_sum_fold(AfTables T, const float* ws, float* sums) {
  __shared__ float s_red[kBlock / 64];
  const AfDesc d = T.desc[blockIdx.x];
  float v[1] = {0.f};
  for (int k = threadIdx.x; k < d.nparts; k += kBlock) v[0] = v[0] + ws[d.part_off + k];
  lars_block_sum<1>(v, s_red);
  if (threadIdx.x == 0) sums[blockIdx.x] = v[0];
}

}  // namespace

int hip_came_stats(gs_plan* p, const CameHyper& h, float* sums, float* ws, void* stream) {
  DeviceGuard g(p->device);
  const AfTables& T = p->af_tab;
  const PlanArgs A = p->args();
  const float* none = nullptr;
  GS_TRY_RET(af_launch(p, GS_OP_CAME_STATS, T.n_lane, stream, came_lane_kernel<false>, A, T, h, ws, none));
  GS_TRY_RET(af_launch(p, GS_OP_CAME_STATS, T.n_tile, stream, came_tile_sums<false>, A, T, h, ws, none));
  GS_TRY_RET(af_launch(p, GS_OP_CAME_STATS, T.n_fold, stream, came_tile_fold, A, T, 2, 3, h.b2, h.omb2, ws));
  GS_TRY_RET(af_launch(p, GS_OP_CAME_STATS, T.n_tile, stream, came_tile_dir<false>, A, T, h, ws));
  return af_launch(p, GS_OP_CAME_STATS, p->n, stream, came_sum_fold, T, static_cast<const float*>(ws), sums);
}

int hip_came_moment(gs_plan* p, const CameHyper& h, const float* sums, float* ws, void* stream) {
  DeviceGuard g(p->device);
  const AfTables& T = p->af_tab;
  const PlanArgs A = p->args();
  GS_TRY_RET(af_launch(p, GS_OP_CAME_MOMENT, T.n_tile, stream, came_tile_sums<true>, A, T, h, ws, sums));
  return af_launch(p, GS_OP_CAME_MOMENT, T.n_fold, stream, came_tile_fold, A, T, 5, 6, h.b3, h.omb3, ws);
}

int hip_came_step(gs_plan* p, const CameHyper& h, const float* sums, const float* ws, void* stream) {
  DeviceGuard g(p->device);
  const AfTables& T = p->af_tab;
  const PlanArgs A = p->args();
  float* w = const_cast<float*>(ws);  // the update kernels only read it
  GS_TRY_RET(af_launch(p, GS_OP_CAME_STEP, T.n_lane, stream, came_lane_kernel<true>, A, T, h, w, sums));
  return af_launch(p, GS_OP_CAME_STEP, T.n_tile, stream, came_tile_dir<true>, A, T, h, w);
}

}  // namespace gs
