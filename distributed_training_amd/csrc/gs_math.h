// The arithmetic of libgsync, written once: dtype conversions, the optimizer updates
// element by element, the per-tensor coefficients of LARS and LAMB and the clip
// coefficient.  The device ops (gs_engine.h, gs_update_kernels.hip) and the host backend
// (gs_host.cpp) compile these same texts, so a CPU run and a GPU run agree bit for bit by
// construction; oracle/gs_oracle.c stays the independent restatement the tests compare
// against.  Everything is value in / value out (scalars by value, results returned or
// written to the caller's locals): the host loops vectorise and the device code stays in
// registers.  Fused multiply-adds are explicit fmaf (the build sets -ffp-contract=off;
// with -mfma the host's fmaf is one vfmadd, bit-identical to the software fmaf).
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/gsync.h"

#ifdef __HIPCC__
#define GS_HD_INL __host__ __device__ inline
#else
#define GS_HD_INL inline
#endif

namespace gs {

// ---------------------------------------------------------------- dtype conversions
GS_HD_INL float bf16_to_f32(uint16_t h) {
  const uint32_t u = static_cast<uint32_t>(h) << 16;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
// round-to-nearest-even; NaN -> 0x7FC0 (c10::BFloat16 round_to_nearest_even)
GS_HD_INL uint16_t f32_to_bf16(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7FC0;
  return static_cast<uint16_t>((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
GS_HD_INL float f16_to_f32(uint16_t h) {
  _Float16 x;
  __builtin_memcpy(&x, &h, 2);
  return static_cast<float>(x);
}
// fp32 -> fp16, round-to-nearest-even of the fp32 VALUE (torch: opmath in fp32, then the cast)
GS_HD_INL uint16_t f32_to_f16(float f) {
#ifdef __HIP_DEVICE_COMPILE__
  // The empty asm pins f as an fp32 register value: without it LLVM folds the producing
  // fma / mul into v_fma_mixlo_f16, which rounds the exact result once, straight to fp16 —
  // a different fp16 wherever the fp32 rounding lands on an fp16 tie (ZeRO fp16 params,
  // fp16 buckets, fp16 unscale; found as master.half() != the fp16 param in
  // test_colossal_low_level_zero_fp16_gpu)
  __asm__("" : "+v"(f));
#endif
  _Float16 x = static_cast<_Float16>(f);
  uint16_t h;
  __builtin_memcpy(&h, &x, 2);
  return h;
}
template <int DT>
GS_HD_INL float to_f32(uint16_t h) {
  if constexpr (DT == GS_BF16) return bf16_to_f32(h);
  else return f16_to_f32(h);
}
template <int DT>
GS_HD_INL uint16_t from_f32(float f) {
  if constexpr (DT == GS_BF16) return f32_to_bf16(f);
  else return f32_to_f16(f);
}
// value as it would read back after a store in DT (used for norms / casts)
template <int DT>
GS_HD_INL float round_to(float f) {
  if constexpr (DT == GS_F32) return f;
  else return to_f32<DT>(from_f32<DT>(f));
}

// ---------------------------------------------------------------- SGD
// optimizer hyper-parameters, rounded to fp32 where torch rounds them
struct SgdHyper {
  float lr, mom, omd, wd;  // omd = float(1 - dampening) formed in double
  int nesterov, maximize, first;
};
inline SgdHyper make_sgd(double lr, double mom, double damp, double wd, int nest, int maxi,
                         int first) {
  return SgdHyper{static_cast<float>(lr), static_cast<float>(mom),
                  static_cast<float>(1.0 - damp), static_cast<float>(wd), nest, maxi, first};
}
// One element of torch's SGD: g the loaded grad, mul the grad multiplier (has_mul).  *b is
// the momentum buffer: read only with a momentum after the first step and written only
// with a momentum, so a caller without one hands in any local.
GS_HD_INL void sgd_update(const SgdHyper& h, bool has_mul, float mul, float g, float* p, float* b) {
  if (has_mul) g = g * mul;                      // clip_grad_norm_ / unscale: grads *= coef
  if (h.maximize) g = -g;
  if (h.wd != 0.f) g = fmaf(h.wd, *p, g);        // grad.add(param, alpha=wd)
  float d = g;
  if (h.mom != 0.f) {
    // buf = clone(g) on the first step, else buf.mul_(mom).add_(g, alpha=1-damp)
    const float nb = h.first ? g : fmaf(h.omd, g, *b * h.mom);
    *b = nb;
    d = h.nesterov ? fmaf(h.mom, nb, g) : nb;    // g.add(buf, alpha=mom)
  }
  *p = fmaf(-h.lr, d, *p);                       // param.add_(d, alpha=-lr)
}

// ---------------------------------------------------------------- Adam / AdamW
struct AdamHyper {
  float b2, w1, w2, eps, wd, step_size, bc2s, decay;  // w1 = float(1-b1), decay = float(1-lr*wd)
  int adamw, maximize;
};
inline AdamHyper make_adam(double lr, double b1, double b2, double eps, double wd, int adamw,
                           int maxi, double step_size, double bc2s) {
  return AdamHyper{static_cast<float>(b2), static_cast<float>(1.0 - b1),
                   static_cast<float>(1.0 - b2), static_cast<float>(eps),
                   static_cast<float>(wd), static_cast<float>(step_size),
                   static_cast<float>(bc2s), static_cast<float>(1.0 - lr * wd), adamw, maxi};
}
// One element of torch's Adam / AdamW: *m = exp_avg, *v = exp_avg_sq
GS_HD_INL void adam_update(const AdamHyper& h, bool has_mul, float mul, float g, float* p, float* m, float* v) {
  if (has_mul) g = g * mul;
  if (h.maximize) g = -g;
  float x = *p;
  if (h.wd != 0.f) {
    if (h.adamw) x = x * h.decay;                         // param.mul_(1 - lr*wd)
    else g = fmaf(h.wd, x, g);                            // grad.add(param, alpha=wd)
  }
  const float nm = fmaf(h.w1, g - *m, *m);                // exp_avg.lerp_(g, 1-b1)  (w<0.5)
  const float nv = fmaf(h.w2 * g, g, *v * h.b2);          // mul_(b2).addcmul_(g, g, 1-b2)
  const float denom = sqrtf(nv) / h.bc2s + h.eps;         // sqrt(v)/bc2_sqrt + eps
  *p = fmaf(h.step_size, nm / denom, x);                  // addcdiv_(m, denom, -lr/bc1)
  *m = nm;
  *v = nv;
}

// ---------------------------------------------------------------- LARS
// LARS (gs_lars_step): eta = the trust coefficient
struct LarsHyper {
  float lr, mom, wd, eta, eps;
};
// The per-tensor learning rate and weight decay of LARS from the tensor's Σp², Σg²
// (include/gsync.h, gs_lars_step): every multiply and add rounded once, no fma (IEEE sqrt
// and division on the host and the device).
// m: the grad multiplier (has_m), which scales ‖g‖ as it scales every g.
GS_HD_INL void lars_coef(const LarsHyper& h, float sp, float sg, int adapt, bool has_m, float m, float* slr,
                         float* wd) {
  float ratio = 1.f;
  *wd = 0.f;
  if (adapt != 0) {
    *wd = h.wd;
    const float wn = sqrtf(sp);
    float gn = sqrtf(sg);
    if (has_m) gn = gn * m;
    if (wn > 0.f && gn > 0.f) ratio = (h.eta * wn) / ((gn + h.wd * wn) + h.eps);
  }
  *slr = h.lr * ratio;
}
// One element of the LARS step with its tensor's (slr, wd_t): SGD with momentum, no fma.
// *b as in sgd_update: touched only with a momentum.
GS_HD_INL void lars_update(const LarsHyper& h, float slr, float wd_t, bool has_m, float m, float g, float* p,
                           float* b) {
  if (has_m) g = g * m;
  if (wd_t != 0.f) g = g + wd_t * *p;
  float d = g;
  if (h.mom != 0.f) {
    const float nb = *b * h.mom + g;
    *b = nb;
    d = nb;
  }
  *p = *p - slr * d;
}

// ---------------------------------------------------------------- LAMB
// LAMB (gs_lamb_moments / gs_lamb_step): w1 = float(1-b1), w2 = float(1-b2), bc2s = float(sqrt(1-b2^step));
// lo, hi = the trust-ratio clamp (0, +inf: none)
struct LambHyper {
  float b1, b2, w1, w2, bc1, bc2s, eps, wd, lr, lo, hi;
};
inline LambHyper make_lamb(double b1, double b2, double bc1, double bc2s, double eps, double wd, double lr, double lo,
                           double hi) {
  return LambHyper{static_cast<float>(b1), static_cast<float>(b2), static_cast<float>(1.0 - b1),
                   static_cast<float>(1.0 - b2), static_cast<float>(bc1), static_cast<float>(bc2s),
                   static_cast<float>(eps), static_cast<float>(wd), static_cast<float>(lr),
                   static_cast<float>(lo), static_cast<float>(hi)};
}
// LAMB's update direction of one element from (p, m', v') (include/gsync.h, gs_lamb_moments):
// the moments pass sums its square and the update pass recomputes it from the stored
// moments, so the recomputed value is the summed one bit for bit.  Every operation rounded
// once, no fma.
GS_HD_INL float lamb_update(const LambHyper& h, float p, float m, float v, float wd_t) {
  float u = (m / h.bc1) / (sqrtf(v) / h.bc2s + h.eps);
  if (wd_t != 0.f) u = u + wd_t * p;
  return u;
}
// ... and the moments themselves: g is already multiplied
GS_HD_INL void lamb_moments(const LambHyper& h, float g, float* m, float* v) {
  *m = *m * h.b1 + h.w1 * g;
  *v = *v * h.b2 + (h.w2 * g) * g;
}
// The per-tensor learning rate of LAMB from the tensor's Σp², Σu² (gs_lamb_step)
GS_HD_INL float lamb_coef(const LambHyper& h, float sp, float su, int adapt) {
  float ratio = 1.f;
  if (adapt != 0) {
    const float wn = sqrtf(sp), un = sqrtf(su);
    if (wn > 0.f && un > 0.f) {
      ratio = wn / un;
      if (ratio < h.lo) ratio = h.lo;
      if (ratio > h.hi) ratio = h.hi;
    }
  }
  return h.lr * ratio;
}

// ---------------------------------------------------------------- EMA / SWA
// a' = lerp(a, s, w) in torch's CPU form (include/gsync.h, gs_ema_step): below |w| = 0.5
// anchored on a (the form adam_update uses for exp_avg.lerp_), at or above it on s with
// wm1 = w - 1.  ema_form derives (wm1, high) from w once per launch.
GS_HD_INL void ema_form(float w, float* wm1, bool* high) {
  *wm1 = w - 1.0f;
  *high = fabsf(w) >= 0.5f;
}
GS_HD_INL float ema_lerp(bool high, float w, float wm1, float a, float s) {
  return high ? fmaf(wm1, s - a, s) : fmaf(w, s - a, a);
}

// ---------------------------------------------------------------- gradient-norm clip
// Gradient-norm clip folded into an update launch (gs_plan_set_clip): the
// update's workgroups form the coefficient themselves, so no coefficient
// launch (and, with the plan's own group sums, no combine launch) sits between
// the Σg² kernel and the update.
struct ClipArgs {
  const float* sq;     // a finished Σg² (groups == 0) or `groups` group sums, `stride` floats apart
  int32_t groups;
  int32_t stride;      // floats between consecutive group sums (1: contiguous; the plan's own copy and a caller's buffer)
  float max_norm, eps;
  float sq_mul, coef_mul;  // host multipliers (ZeRO's loss scale): 1 = none
  float* out;          // [sq, coef, norm] written by workgroup 0 (nullable)
  // 0: DeepSpeed's `if coef < 1: clip` (a NaN coefficient clips nothing); 1: torch's
  // clamp(coef, max=1) (clip_grad_norm_, T:nn/utils/clip_grad.py:172 — NaN stays NaN)
  int32_t torch_clamp;
};
// min(1, max_norm / (norm + eps)) from norm = sqrtf(Σg²) (gs_clip_coef,
// T:nn/utils/clip_grad.py:165-174); torch_clamp as in ClipArgs
GS_HD_INL float clip_coef(float norm, float max_norm, float eps, int torch_clamp) {
  const float c = max_norm / (norm + eps);
  return torch_clamp ? (c >= 1.f ? 1.f : c) : (c < 1.f ? c : 1.f);
}
// The folded clip's grad multiplier from the folded Σg² in *sq: the norm is that of the
// unscaled grads (gscale, nullable: the AMP / loss scale the update also applies), and the
// multiplier carries the scale with it.  *sq and *norm come back as published in ClipArgs::out.
// The quotient is clip_coef's, so the folded and the separate path agree bit for bit.
GS_HD_INL float clip_factor(const ClipArgs& c, const float* gscale, float* sq, float* norm) {
  const float s = gscale ? *gscale : 1.f;
  if (gscale) *sq = *sq * (s * s);
  *sq = *sq * c.sq_mul;
  *norm = sqrtf(*sq);
  float coef = clip_coef(*norm, c.max_norm, c.eps, c.torch_clamp);
  if (gscale) coef = coef * s;
  return coef * c.coef_mul;
}

}  // namespace gs
