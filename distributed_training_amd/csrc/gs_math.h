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

// ---------------------------------------------------------------- Muon
// Muon (gs_muon_prep): w1 = float(1-momentum) formed in double.  The momentum and the
// Nesterov look-ahead are two torch.lerp's (buf.lerp_(g, 1-mu), g.lerp(buf, mu)), each in
// ema_lerp's form, so the buffer is torch's bit for bit.
struct MuonHyper {
  float w1, mu, eps;
  int nesterov;
};
GS_HD_INL float muon_buf(const MuonHyper& h, float g, float b) {
  float wm1;
  bool high;
  ema_form(h.w1, &wm1, &high);
  return ema_lerp(high, h.w1, wm1, b, g);
}
// the update direction from the grad and the NEW buffer: the segmented pass sums its
// square, the X pass recomputes it from the stored buffer — the same bits
GS_HD_INL float muon_u(const MuonHyper& h, float g, float nb) {
  if (!h.nesterov) return nb;
  float wm1;
  bool high;
  ema_form(h.mu, &wm1, &high);
  return ema_lerp(high, h.mu, wm1, g, nb);
}
// s = 1 / max(sqrt(Σu²), eps)
GS_HD_INL float muon_scale(float su, float eps) {
  const float nrm = sqrtf(su);
  return 1.f / (nrm > eps ? nrm : eps);
}
// the three epilogues of the Newton-Schulz stages (acc: the fp32 sum of bf16 products)
// and the parameter update; one fma each where torch's addmm rounds once
GS_HD_INL float muon_gram_out(float alpha, float acc) { return alpha * acc; }
GS_HD_INL float muon_poly_out(float b, float c, float acc, float d) { return fmaf(c, acc, b * d); }
GS_HD_INL float muon_apply_out(float a, float acc, float x) { return fmaf(a, x, acc); }
GS_HD_INL float muon_param(float p, float decay, float adj_lr, float o) { return p * decay - adj_lr * o; }

// ---------------------------------------------------------------- Adafactor
// Adafactor (gs_adafactor_stats / gs_adafactor_step; include/gsync.h): the factored second
// moment's element-wise pieces.  Every operation is rounded once; the divisions and the
// square roots are IEEE (rsqrt is 1 / sqrtf, torch's CPU form).
struct AfHyper {
  float w, wm1;  // the lerp weight and ema_form's w - 1
  bool high;     // ema_form's switch
  float eps1, eps1sq;
};
GS_HD_INL AfHyper af_hyper(double w, double eps1) {
  AfHyper h;
  h.w = static_cast<float>(w);
  ema_form(h.w, &h.wm1, &h.high);
  h.eps1 = static_cast<float>(eps1);
  h.eps1sq = static_cast<float>(eps1 * eps1);
  return h;
}
// factor' = lerp(factor, sum / n, w): the sum first, then one true division
GS_HD_INL float af_factor(const AfHyper& h, float old, float sum, int n) {
  return ema_lerp(h.high, h.w, h.wm1, old, sum / static_cast<float>(n));
}
// m = max(Σ row_var / R, eps1); a NaN stays a NaN, as torch's clamp keeps it
GS_HD_INL float af_m(const AfHyper& h, float rv_sum, int R) {
  const float m = rv_sum / static_cast<float>(R);
  return m < h.eps1 ? h.eps1 : m;
}
GS_HD_INL float af_v(const AfHyper& h, float rv, float cv, float m) {
  const float v = rv * cv / m;
  return v < h.eps1sq ? h.eps1sq : v;
}
GS_HD_INL float af_v_vec(const AfHyper& h, float variance) { return variance < h.eps1sq ? h.eps1sq : variance; }
// u without its sign (Σu² does not see it; af_param applies it)
GS_HD_INL float af_u(float g, float v) { return g * (1.0f / sqrtf(v)); }
// alpha / denom of a tensor from its Σp² (before the decay) and Σu²
GS_HD_INL float af_scale(float sp, float su, float numel, float eps2, float rho, float d) {
  const float rms = sqrtf(sp / numel);
  const float alpha = (rms > eps2 ? rms : eps2) * rho;
  const float clip = sqrtf(su / numel) / d;
  return alpha / (clip > 1.f ? clip : 1.f);
}
GS_HD_INL float af_param(float p, float decay, float scale, float u, bool maximize) {
  return maximize ? p * decay + scale * u : p * decay - scale * u;
}

// ---------------------------------------------------------------- CAME
// CAME (gs_came_stats / gs_came_moment / gs_came_step; include/gsync.h): the element-wise
// pieces.  Every operation is rounded once; divisions and square roots are IEEE.
struct CameHyper {
  float b1, omb1, b2, omb2, b3, omb3;  // the betas and 1 - beta (formed in double)
  float eps1, eps2, d;
  float lr, wdlr;  // lr, -weight_decay * lr (formed in double)
  bool decay;      // weight_decay != 0
};
GS_HD_INL CameHyper came_hyper(double b1, double b2, double b3, double eps1, double eps2, double d, double lr,
                               double wd) {
  CameHyper h;
  h.b1 = static_cast<float>(b1), h.omb1 = static_cast<float>(1.0 - b1);
  h.b2 = static_cast<float>(b2), h.omb2 = static_cast<float>(1.0 - b2);
  h.b3 = static_cast<float>(b3), h.omb3 = static_cast<float>(1.0 - b3);
  h.eps1 = static_cast<float>(eps1), h.eps2 = static_cast<float>(eps2), h.d = static_cast<float>(d);
  h.lr = static_cast<float>(lr), h.wdlr = static_cast<float>(-wd * lr);
  h.decay = wd != 0.0;
  return h;
}
GS_HD_INL float came_ema(float old, float x, float b, float omb) { return old * b + x * omb; }
GS_HD_INL float came_sq(float g, float eps1) { return g * g + eps1; }
GS_HD_INL float came_mean(float sum, int n) { return sum / static_cast<float>(n); }
// factor' = factor*b + (sum / n)*(1 - b): the sum first, then one true division
GS_HD_INL float came_factor(float old, float sum, int n, float b, float omb) {
  return came_ema(old, came_mean(sum, n), b, omb);
}
GS_HD_INL float came_rf(float r, float mean) { return 1.0f / sqrtf(r / mean); }  // a row's factor
GS_HD_INL float came_cf(float c) { return 1.0f / sqrtf(c); }                     // a column's (or a vector's v)
GS_HD_INL float came_dir(float x, float rf, float cf) { return x * (rf * cf); }  // u from g, upd from m
// max(1, sqrt(Σu² / numel) / d); a NaN stays a NaN, as clamp_ keeps it
GS_HD_INL float came_denom(float su, float numel, float d) {
  const float x = sqrtf(su / numel) / d;
  return x < 1.f ? 1.f : x;
}
GS_HD_INL float came_res(float uh, float m, float eps2) {
  const float e = uh - m;
  return e * e + eps2;
}
GS_HD_INL float came_param(const CameHyper& h, float p, float upd) {
  if (h.decay) p = p + p * h.wdlr;
  return p - h.lr * upd;
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

// ---------------------------------------------------------------- uint8 quantization (gs_quant_*)
// torch's MinMaxObserver qparams and quantize / dequantize in fp32
// (T:ao/quantization/observer.py _calculate_qparams, quint8 affine;
// T:distributed/algorithms/ddp_comm_hooks/quantization_hooks.py), every step one correctly
// rounded operation: both divisions are true divisions and nothing is fused.
struct QuantParams {
  float scale;
  int32_t zp;
};
// one value folded into a channel's running (lo, hi), which start at 0: a value that is not
// finite opens the range to (-inf, +inf), which quant_params turns into a NaN scale
GS_HD_INL void quant_fold(float v, float* lo, float* hi) {
  if (!(v - v == 0.f)) {
    *lo = -INFINITY;
    *hi = INFINITY;
  }
  *lo = fminf(*lo, v);
  *hi = fmaxf(*hi, v);
}
// lo = min(min x, 0), hi = max(max x, 0)
GS_HD_INL QuantParams quant_params(float lo, float hi) {
  QuantParams q;
  if (!(lo > -INFINITY && hi < INFINITY)) {
    q.scale = NAN;
    q.zp = 0;
    return q;
  }
  const float s = (hi - lo) / 255.0f;
  q.scale = s > 1.1920928955078125e-07f ? s : 1.1920928955078125e-07f;  // FLT_EPSILON
  const int z = 0 - static_cast<int>(rintf(lo / q.scale));
  q.zp = z < 0 ? 0 : (z > 255 ? 255 : z);
  return q;
}
// the byte of x; zpf = (float)zp.  A NaN (a NaN scale) becomes 0.
GS_HD_INL uint32_t quant_value(float x, float scale, float zpf) {
  const float y = rintf(x / scale) + zpf;
  return static_cast<uint32_t>(fminf(fmaxf(y, 0.f), 255.f));
}
GS_HD_INL float dequant_value(uint32_t q, float scale, float zpf) { return scale * (static_cast<float>(q) - zpf); }

}  // namespace gs
