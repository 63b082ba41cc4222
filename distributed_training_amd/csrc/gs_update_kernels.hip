// gfx950 (CDNA4) fused SGD / Adam(W) / LARS updates of libgsync (gs_sgd_step / gs_adam_step /
// gs_lars_step[_lowp]): the chunk-map engine of gs_engine.h with SgdOp / AdamOp / LarsOp, the
// grad-load policy per launch; the segmented per-tensor-sum pass over the same chunk map
// (seg_sum_kernel), one skeleton with two lane policies: LarsLanes, LARS's Σp², Σg²
// (gs_lars_norms), and LambLanes, LAMB's Σp², Σu² fused with the moments' read-modify-write
// (gs_lamb_moments); LambOp on the engine (gs_lamb_step); and the EMA / SWA weight average
// (gs_ema_step / gs_ema_hyper): EmaOp on the engine.

#include "gs_seg.h"

namespace gs {

// grads a Σg² pass of this plan read just before (the clip path) stay in the caches
// when they fit in the Infinity Cache: cached loads then, non-temporal otherwise
// (the flag is consumed by the update)
static bool nt_grad(gs_plan* p, int gdt) {
  const bool hot = p->grads_read && p->elems * dtype_bytes(gdt) <= kInfinityCacheBytes;
  p->grads_read = false;
  return !hot;
}

template <bool NTG>
static int sgd_nt(gs_plan* p, int gdt, int ldt, const SgdHyper& h, const float* gsc, const float* fi,
                  const ClipArgs* clip, void* stream) {
  GS_DISPATCH_FLOAT(gdt, GD, GS_DISPATCH_LOWP(ldt, LD, {
    SgdOp<kUnit, GD, LD, NTG> op;
    op.h = h; op.gscale = gsc; op.found_inf = fi; op.hyper = p->hyper;
    if (clip) { op.clip = *clip; op.clip_on = true; }
    return launch(p, op, stream);
  }));
  return GS_OK;
}

int hip_sgd(gs_plan* p, int gdt, int ldt, const SgdHyper& h, const float* gsc, const float* fi,
            const ClipArgs* clip, void* stream) {
  DeviceGuard g(p->device);
  return nt_grad(p, gdt) ? sgd_nt<true>(p, gdt, ldt, h, gsc, fi, clip, stream)
                         : sgd_nt<false>(p, gdt, ldt, h, gsc, fi, clip, stream);
}

template <bool NTG>
static int adam_nt(gs_plan* p, int gdt, int ldt, const AdamHyper& h, const float* gsc, const float* fi,
                   const ClipArgs* clip, void* stream) {
  GS_DISPATCH_FLOAT(gdt, GD, GS_DISPATCH_LOWP(ldt, LD, {
    AdamOp<kUnit, GD, LD, NTG> op;
    op.h = h; op.gscale = gsc; op.found_inf = fi; op.hyper = p->hyper;
    if (clip) { op.clip = *clip; op.clip_on = true; }
    return launch(p, op, stream);
  }));
  return GS_OK;
}

int hip_adam(gs_plan* p, int gdt, int ldt, const AdamHyper& h, const float* gsc, const float* fi,
             const ClipArgs* clip, void* stream) {
  DeviceGuard g(p->device);
  return nt_grad(p, gdt) ? adam_nt<true>(p, gdt, ldt, h, gsc, fi, clip, stream)
                         : adam_nt<false>(p, gdt, ldt, h, gsc, fi, clip, stream);
}

// -------------------------------------------------------------------- EMA
// gs_ema_step: EmaOp on the engine, one instantiation per (source dtype, copy dtype).  The
// average takes cached loads (a read-modify-write stream); the source, read once by this
// launch, follows the engine's size rule (nt_read_once): non-temporal above the Infinity Cache.
template <bool NTS>
static int ema_nt(gs_plan* p, int sdt, int ldt, float w, int copy, void* stream) {
  GS_DISPATCH_FLOAT(sdt, SD, GS_DISPATCH_LOWP(ldt, LD, {
    EmaOp<kUnit, SD, LD, NTS> op;
    op.w = w; op.copy = copy; op.hyper = p->hyper;
    return launch(p, op, stream);
  }));
  return GS_OK;
}

int hip_ema(gs_plan* p, int sdt, int ldt, float w, int copy, void* stream) {
  DeviceGuard g(p->device);
  return nt_read_once(p->elems * dtype_bytes(sdt)) ? ema_nt<true>(p, sdt, ldt, w, copy, stream)
                                                   : ema_nt<false>(p, sdt, ldt, w, copy, stream);
}

__global__ void ema_hyper_kernel(int64_t* n_averaged, int mode, double decay, float* hyper) {
  if (threadIdx.x == 0) ema_hyper_update(n_averaged, mode, decay, hyper);
}

int hip_ema_hyper(int64_t* n_averaged, int mode, double decay, float* hyper, void* stream) {
  hipLaunchKernelGGL(ema_hyper_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), n_averaged, mode,
                     decay, hyper);
  HIP_RET(hipGetLastError());
  return GS_OK;
}

// ------------------------------------------------- segmented per-tensor sums: gs_seg.h

int hip_lars_set_adapt(gs_plan* p) {
  DeviceGuard g(p->device);
  if (p->n == 0) return GS_OK;
  if (!p->d_lars) return lars_prepare(p, nullptr);  // uploads p->adapt
  HIP_RET(hipMemcpy(lars_adapt_ptr(p), p->adapt.data(), sizeof(int32_t) * p->n, hipMemcpyHostToDevice));
  return GS_OK;
}

// ------------------------------------------------------------------- LARS
// gs_lars_norms: Σp², Σg², two streams and no stores.  Both take plain cached loads: the
// update re-reads the same bytes right behind, and a ResNet-50's p + g (204 MB) fit the
// Infinity Cache.  A group of kLarsG full chunks has all 2 * kLarsG accesses of a lane in
// flight before one barrier pair.
#ifndef GS_G_LARS_NORM
#define GS_G_LARS_NORM 4
#endif
constexpr int kLarsG = GS_G_LARS_NORM;

template <int GD_>
struct LarsLanes {
  static constexpr int G = kLarsG, S = 2, W = 2, GD = GD_;
  static constexpr bool NTG = false, NTS = false;
  __device__ __forceinline__ bool begin() { return true; }
  template <bool U>
  __device__ __forceinline__ void lane(int, int, float (&r)[S][4], float& sp, float& sg) const {
    sp = lars_sq4(r[0]);
    sg = lars_sq4(r[1]);
  }
};

int hip_lars_norms(gs_plan* p, int gdt, float* norms, void* stream) {
  DeviceGuard g(p->device);
  if (p->n == 0) return GS_OK;
  GS_DISPATCH_FLOAT(gdt, GD, return lars_segmented(p, norms, stream, GS_OP_LARS_NORM, LarsLanes<GD>{}));
  return GS_OK;
}

// ldt = -1: LarsOp<.., -1, ..>, the op without a copy stream (gs_lars_step)
template <bool NTG>
static int lars_nt(gs_plan* p, int gdt, int ldt, const LarsHyper& h, const float* norms, const float* gsc,
                   const float* fi, void* stream) {
  GS_DISPATCH_FLOAT(gdt, GD, GS_DISPATCH_LOWP(ldt, LD, {
    LarsOp<kUnit, GD, LD, NTG> op;
    op.h = h; op.norms = norms; op.adapt = reinterpret_cast<const int32_t*>(lars_adapt_ptr(p));
    op.gscale = gsc; op.found_inf = fi; op.hyper = p->hyper;
    return launch(p, op, stream);
  }));
  return GS_OK;
}

int hip_lars(gs_plan* p, int gdt, int ldt, const LarsHyper& h, const float* norms, const float* gsc,
             const float* fi, void* stream) {
  DeviceGuard g(p->device);
  if (p->n == 0) return GS_OK;
  GS_TRY_RET(lars_prepare(p, stream));
  return nt_grad(p, gdt) ? lars_nt<true>(p, gdt, ldt, h, norms, gsc, fi, stream)
                         : lars_nt<false>(p, gdt, ldt, h, norms, gsc, fi, stream);
}

// ------------------------------------------------------------------- LAMB
// gs_lamb_moments: LAMB's trust ratio needs the norm of the Adam update u, so the norm
// pass is also the moments pass — the segmented pass over four streams (p, g, m, v) with
// an element-wise read-modify-write of (m, v), and u² in place of LARS's g².  m', v' are
// stored; u is not: LambOp recomputes it from (p, m', v') by the same text (lamb_update).
// Load policy (measured: profiles/lamb/): non-temporal loads of g (dead
// after this pass), cached loads of p, m, v (re-read by the update).  GS_LAMB_NT is the
// compile-time switch of the A/B library variants: bit 0 = g, bit 1 = p, m, v.
#ifndef GS_LAMB_NT
#define GS_LAMB_NT 1
#endif
#ifndef GS_G_LAMB_MOMENTS
#define GS_G_LAMB_MOMENTS 4
#endif
constexpr int kLambG = GS_G_LAMB_MOMENTS;

template <int GD_>
struct LambLanes {
  static constexpr int G = kLambG, S = 4, W = 2, GD = GD_;
  static constexpr bool NTG = (GS_LAMB_NT & 1) != 0, NTS = (GS_LAMB_NT & 2) != 0;
  LambHyper h;
  const int32_t* adapt;  // [n]
  const float* gscale;
  const float* found_inf;
  const float* hyper;  // [lr, bc1, bc2s] in device memory (gs_plan_set_hyper_source) or NULL
  float mul;           // *gscale, read by begin()
  __device__ __forceinline__ bool begin() {
    if (found_inf != nullptr && *found_inf != 0.f) return false;
    if (hyper) {
      h.bc1 = hyper[1];
      h.bc2s = hyper[2];
    }
    mul = gscale != nullptr ? *gscale : 1.f;
    return true;
  }
  // the new moments in place and the lane's Σp², Σu² (the elements past `valid` add
  // nothing: with eps = 0 their u would be 0/0)
  template <bool U>
  __device__ __forceinline__ void lane(int t, int valid, float (&r)[S][4], float& sp, float& su) const {
    const float wd_t = (U ? cload(adapt, t) : adapt[t]) != 0 ? h.wd : 0.f;
    float u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float gi = r[1][i];
      if (gscale != nullptr) gi = gi * mul;
      lamb_moments(h, gi, &r[2][i], &r[3][i]);
      const float ui = lamb_update(h, r[0][i], r[2][i], r[3][i], wd_t);
      u[i] = i < valid ? ui : 0.f;
    }
    sp = lars_sq4(r[0]);
    su = lars_sq4(u);
  }
};

int hip_lamb_moments(gs_plan* p, int gdt, const LambHyper& h, float* norms, const float* gsc, const float* fi,
                     void* stream) {
  DeviceGuard g(p->device);
  if (p->n == 0) return GS_OK;
  GS_TRY_RET(lars_prepare(p, stream));  // adapt below points into the scratch
  const int32_t* adapt = reinterpret_cast<const int32_t*>(lars_adapt_ptr(p));
  GS_DISPATCH_FLOAT(gdt, GD, return lars_segmented(p, norms, stream, GS_OP_LAMB_MOMENTS,
                                                   LambLanes<GD>{h, adapt, gsc, fi, p->hyper, 1.f}));
  return GS_OK;
}

int hip_lamb(gs_plan* p, int ldt, const LambHyper& h, const float* norms, const float* fi, void* stream) {
  DeviceGuard g(p->device);
  if (p->n == 0) return GS_OK;
  GS_TRY_RET(lars_prepare(p, stream));
  GS_DISPATCH_LOWP(ldt, LD, {
    LambOp<kUnit, LD> op;
    op.h = h; op.norms = norms; op.adapt = reinterpret_cast<const int32_t*>(lars_adapt_ptr(p));
    op.found_inf = fi; op.hyper = p->hyper;
    return launch(p, op, stream);
  });
  return GS_OK;
}

}  // namespace gs
