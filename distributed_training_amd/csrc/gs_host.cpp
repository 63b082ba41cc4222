// Host implementation of the plan ops, used for CPU tensors (the CPU/gloo
// configuration: BASELINE config 1).  The arithmetic is the device ops', element
// for element: both sides compile the update, clip and conversion functions of
// gs_math.h (-ffp-contract=off), so a CPU run and a GPU run of the engine agree
// bit for bit on the pack / unpack / optimizer math.  A HIP plan never reaches
// this file.
//
// Speed: loops are instantiated per dtype combination (no per-element type
// switch) so the compiler vectorises them (built with -mavx2 -mfma: fmaf
// is one vfmadd, bit-identical to the software fmaf), and large plans are
// split over gs_set_host_threads() threads (torch's intra-op thread count).
// Elementwise results do not depend on the split; the Σg² reductions stay
// serial (their double-precision order is the oracle's).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>

#include "gs_common.h"

namespace gs {
namespace {

template <int DT>
inline float ldT(const void* base, int64_t i) {
  if constexpr (DT == GS_F32) return static_cast<const float*>(base)[i];
  else return to_f32<DT>(static_cast<const uint16_t*>(base)[i]);
}
template <int DT>
inline void stT(void* base, int64_t i, float v) {
  if constexpr (DT == GS_F32) static_cast<float*>(base)[i] = v;
  else static_cast<uint16_t*>(base)[i] = from_f32<DT>(v);
}
inline void* slot(gs_plan* p, int s, int t) { return p->h_ptrs[static_cast<size_t>(s) * p->n + t]; }

int check_float(int dt) {
  if (!is_float_dtype(dt)) return fail(GS_EINVAL, "unsupported floating dtype");
  return GS_OK;
}

std::atomic<int> g_threads{1};
constexpr int64_t kChunk = int64_t(1) << 16;     // elements per work item
constexpr int64_t kParallelMin = int64_t(1) << 19;  // below this, one thread

// fn(t, i0, i1) over every tensor's element range, split into chunks and
// spread over the host threads (static round-robin: deterministic, and the
// elementwise results do not depend on it anyway)
template <class F>
void for_ranges(const gs_plan* p, F&& fn) {
  int64_t total = 0;
  for (int t = 0; t < p->n; ++t) total += p->numel[t];
  const int nt = std::max(1, std::min<int>(g_threads.load(), static_cast<int>(total / kChunk) + 1));
  if (nt == 1 || total < kParallelMin) {
    for (int t = 0; t < p->n; ++t)
      if (p->numel[t]) fn(t, int64_t(0), p->numel[t]);
    return;
  }
  std::vector<std::tuple<int, int64_t, int64_t>> items;
  for (int t = 0; t < p->n; ++t)
    for (int64_t i = 0; i < p->numel[t]; i += kChunk) items.emplace_back(t, i, std::min(p->numel[t], i + kChunk));
  auto work = [&](int k) {
    for (size_t j = k; j < items.size(); j += nt) fn(std::get<0>(items[j]), std::get<1>(items[j]), std::get<2>(items[j]));
  };
  std::vector<std::thread> pool;
  for (int k = 1; k < nt; ++k) pool.emplace_back(work, k);
  work(0);
  for (auto& th : pool) th.join();
}

}  // namespace

int host_pack(gs_plan* p, int src_slot, int src_dt, void* flat, int flat_dt, float s, int mode) {
  GS_DISPATCH_FLOAT(src_dt, SD, GS_DISPATCH_FLOAT(flat_dt, FD, {
    const int fsz = dtype_size(FD);
    for_ranges(p, [&](int t, int64_t i0, int64_t i1) {
      const void* src = slot(p, src_slot, t);
      void* dst = static_cast<char*>(flat) + p->off[t] * fsz;
      if (!src) {
        const float z = mode == GS_SCALE_MUL ? 0.f * s : (mode == GS_SCALE_DIV ? 0.f / s : 0.f);
        for (int64_t i = i0; i < i1; ++i) stT<FD>(dst, i, z);  // unused parameter: zeros, as the kernel
      } else if (mode == GS_SCALE_MUL) {
        for (int64_t i = i0; i < i1; ++i) stT<FD>(dst, i, ldT<SD>(src, i) * s);
      } else if (mode == GS_SCALE_DIV) {
        for (int64_t i = i0; i < i1; ++i) stT<FD>(dst, i, round_to<FD>(ldT<SD>(src, i)) / s);
      } else {
        for (int64_t i = i0; i < i1; ++i) stT<FD>(dst, i, ldT<SD>(src, i));
      }
    });
  }));
  return GS_OK;
}

int host_unpack(gs_plan* p, const void* flat, int flat_dt, int dst_slot, int dst_dt, float* sq,
                int acc) {
  GS_DISPATCH_FLOAT(flat_dt, FD, GS_DISPATCH_FLOAT(dst_dt, DD, {
    const int fsz = dtype_size(FD);
    if (sq) {  // serial: the double-precision Σ order is the oracle's
      double total = 0.0;
      for (int t = 0; t < p->n; ++t) {
        const void* src = static_cast<const char*>(flat) + p->off[t] * fsz;
        void* dst = slot(p, dst_slot, t);
        if (dst == nullptr) continue;
        for (int64_t i = 0; i < p->numel[t]; ++i) {
          const float v = ldT<FD>(src, i);
          stT<DD>(dst, i, v);
          const float r = round_to<DD>(v);
          total += static_cast<double>(r) * r;
        }
      }
      sq[0] = acc ? sq[0] + static_cast<float>(total) : static_cast<float>(total);
    } else {
      for_ranges(p, [&](int t, int64_t i0, int64_t i1) {
        const void* src = static_cast<const char*>(flat) + p->off[t] * fsz;
        void* dst = slot(p, dst_slot, t);
        if (dst == nullptr) return;
        for (int64_t i = i0; i < i1; ++i) stT<DD>(dst, i, ldT<FD>(src, i));
      });
    }
  }));
  return GS_OK;
}

int host_unpack_check(gs_plan* p, const void* flat, int flat_dt, int dst_slot, int dst_dt, float* found) {
  std::atomic<int> bad{found[0] != 0.f ? 1 : 0};
  GS_DISPATCH_FLOAT(flat_dt, FD, GS_DISPATCH_FLOAT(dst_dt, DD, {
    const int fsz = dtype_size(FD);
    for_ranges(p, [&](int t, int64_t i0, int64_t i1) {
      const void* src = static_cast<const char*>(flat) + p->off[t] * fsz;
      void* dst = slot(p, dst_slot, t);
      if (dst == nullptr) return;
      int b = 0;
      for (int64_t i = i0; i < i1; ++i) {
        const float v = ldT<FD>(src, i);
        stT<DD>(dst, i, v);
        b |= !std::isfinite(round_to<DD>(v));
      }
      if (b) bad.store(1);
    });
  }));
  found[0] = bad.load() ? 1.f : 0.f;
  return GS_OK;
}

int host_scale(gs_plan* p, int s_, int dt, float s, int mode) {
  GS_DISPATCH_FLOAT(dt, DT, {
    for_ranges(p, [&](int t, int64_t i0, int64_t i1) {
      void* x = slot(p, s_, t);
      if (mode == GS_SCALE_DIV)
        for (int64_t i = i0; i < i1; ++i) stT<DT>(x, i, ldT<DT>(x, i) / s);
      else
        for (int64_t i = i0; i < i1; ++i) stT<DT>(x, i, ldT<DT>(x, i) * s);
    });
  });
  return GS_OK;
}

int host_clip_scale(gs_plan* p, int s_, int dt, const ClipArgs& clip) {
  const float cf = host_clip_factor(clip, nullptr);
  if (cf == 1.f) return GS_OK;  // x * 1 == x: nothing to write (the device grid exits too)
  return host_scale(p, s_, dt, cf, GS_SCALE_MUL);
}

int host_sqnorm(gs_plan* p, int s_, int dt, float* sq, int acc) {
  GS_DISPATCH_FLOAT(dt, DT, {
    double total = 0.0;
    for (int t = 0; t < p->n; ++t) {
      const void* x = slot(p, s_, t);
      for (int64_t i = 0; i < p->numel[t]; ++i) {
        const double v = ldT<DT>(x, i);
        total += v * v;
      }
    }
    sq[0] = acc ? sq[0] + static_cast<float>(total) : static_cast<float>(total);
  });
  return GS_OK;
}

int host_sum(gs_plan* p, int s_, int dt, float* out, int acc) {
  GS_DISPATCH_FLOAT(dt, DT, {
    double total = 0.0;
    for (int t = 0; t < p->n; ++t) {
      const void* x = slot(p, s_, t);
      for (int64_t i = 0; i < p->numel[t]; ++i) total += ldT<DT>(x, i);
    }
    out[0] = acc ? out[0] + static_cast<float>(total) : static_cast<float>(total);
  });
  return GS_OK;
}

int host_clip_coef(const float* sq, float max_norm, float eps, float* coef, float* norm) {
  const float nrm = sqrtf(sq[0]);
  if (norm) norm[0] = nrm;
  coef[0] = clip_coef(nrm, max_norm, eps, 0);
  return GS_OK;
}

int host_unscale_check(gs_plan* p, int s_, int dt, const float* inv, float* found) {
  std::atomic<int> bad{found[0] != 0.f ? 1 : 0};
  const bool scale = inv && inv[0] != 1.f;
  const float sc = scale ? inv[0] : 1.f;
  GS_DISPATCH_FLOAT(dt, DT, {
    for_ranges(p, [&](int t, int64_t i0, int64_t i1) {
      void* x = slot(p, s_, t);
      int b = 0;
      for (int64_t i = i0; i < i1; ++i) {
        const float v = ldT<DT>(x, i);
        b |= !std::isfinite(v);
        if (scale) stT<DT>(x, i, v * sc);
      }
      if (b) bad.store(1);
    });
  });
  found[0] = bad.load() ? 1.f : 0.f;
  return GS_OK;
}

// gs_kernels.hip wave_reduce<false>: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
// row_mirror, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3; lane 63.
// A lane a step does not write adds 0 (the DPP `old` operand is the identity).
float host_wave_sum(const float* x, int n, int stride) {
  float v[64], t[64];
  // lane l first adds x[l], x[l + 64], ... in order (clip_multiplier's fold of up to
  // GS_RED_PARTIALS partials), then the tree
  for (int l = 0; l < 64; ++l) {
    float a = 0.f;
    for (int j = l; j < n; j += 64) a = a + x[static_cast<int64_t>(j) * stride];
    v[l] = 0.f + a;
  }
  auto step = [&](auto src, unsigned row_mask) {
    for (int l = 0; l < 64; ++l) t[l] = ((row_mask >> (l >> 4)) & 1u) ? v[src(l)] : 0.f;
    for (int l = 0; l < 64; ++l) v[l] = v[l] + t[l];
  };
  static const int q1[4] = {1, 0, 3, 2}, q2[4] = {2, 3, 0, 1};
  step([](int l) { return (l & ~3) | q1[l & 3]; }, 0xFu);
  step([](int l) { return (l & ~3) | q2[l & 3]; }, 0xFu);
  step([](int l) { return (l & ~7) | (7 - (l & 7)); }, 0xFu);
  step([](int l) { return (l & ~15) | (15 - (l & 15)); }, 0xFu);
  step([](int l) { return (l & ~15) - 1; }, 0xAu);  // rows 1, 3 <- lane 15 of the row below
  step([](int) { return 31; }, 0xCu);                // rows 2, 3 <- lane 31
  return v[63];
}

float host_clip_factor(const ClipArgs& c, const float* gsc) {
  float sq = c.groups > 0 ? host_wave_sum(c.sq, c.groups, c.stride) : c.sq[0];
  float nrm;
  const float coef = clip_factor(c, gsc, &sq, &nrm);
  if (c.out) {
    c.out[0] = sq;
    c.out[1] = coef;
    c.out[2] = nrm;
  }
  return coef;
}

int host_sgd(gs_plan* p, int gdt, int ldt, const SgdHyper& h, const float* gsc, const float* fi,
             const ClipArgs* clip) {
  const float cf = clip ? host_clip_factor(*clip, gsc) : 1.f;  // published even on a skipped step
  if (fi && fi[0] != 0.f) {
    GS_TRY_RET(check_float(gdt));
    return GS_OK;
  }
  const bool has_gs = gsc != nullptr || clip != nullptr;
  const float gs = clip ? cf : (gsc ? gsc[0] : 1.f);
  GS_DISPATCH_FLOAT(gdt, GD, GS_DISPATCH_LOWP(ldt, LD, {
    for_ranges(p, [&](int t, int64_t i0, int64_t i1) {
      float* pp = static_cast<float*>(slot(p, 0, t));
      const void* gp = slot(p, 1, t);
      float* bp = static_cast<float*>(slot(p, 2, t));
      void* lp = slot(p, 3, t);
      // a local copy: no store of the loop can alias it, so its branches are loop-invariant
      const SgdHyper hh = h;
      const bool has_b = hh.mom != 0.f, rd_b = has_b && !hh.first;  // bp is NULL without a momentum
      for (int64_t i = i0; i < i1; ++i) {
        float x = pp[i], b = 0.f;
        if (rd_b) b = bp[i];
        sgd_update(hh, has_gs, gs, ldT<GD>(gp, i), &x, &b);
        pp[i] = x;
        if (has_b) bp[i] = b;
        if constexpr (LD >= 0) stT<LD>(lp, i, x);
      }
    });
  }));
  return GS_OK;
}

int host_adam(gs_plan* p, int gdt, int ldt, const AdamHyper& h, const float* gsc,
              const float* fi, const ClipArgs* clip) {
  const float cf = clip ? host_clip_factor(*clip, gsc) : 1.f;  // published even on a skipped step
  if (fi && fi[0] != 0.f) {
    GS_TRY_RET(check_float(gdt));
    return GS_OK;
  }
  const bool has_gs = gsc != nullptr || clip != nullptr;
  const float gs = clip ? cf : (gsc ? gsc[0] : 1.f);
  GS_DISPATCH_FLOAT(gdt, GD, GS_DISPATCH_LOWP(ldt, LD, {
    for_ranges(p, [&](int t, int64_t i0, int64_t i1) {
      float* pp = static_cast<float*>(slot(p, 0, t));
      const void* gp = slot(p, 1, t);
      float* mp = static_cast<float*>(slot(p, 2, t));
      float* vp = static_cast<float*>(slot(p, 3, t));
      void* lp = slot(p, 4, t);
      for (int64_t i = i0; i < i1; ++i) {
        float x = pp[i], m = mp[i], v = vp[i];
        adam_update(h, has_gs, gs, ldT<GD>(gp, i), &x, &m, &v);
        pp[i] = x;
        mp[i] = m;
        vp[i] = v;
        if constexpr (LD >= 0) stT<LD>(lp, i, x);
      }
    });
  }));
  return GS_OK;
}

// EMA / SWA averaging on the host (include/gsync.h, gs_ema_step): EmaOp's arithmetic
// (ema_form / ema_lerp).  Copy mode with an fp32 source is a memcpy: no float register sees the
// words, so integer buffers and NaN patterns pass unchanged.
int host_ema(gs_plan* p, int sdt, int ldt, float w, int copy) {
  float wm1;
  bool high;
  ema_form(w, &wm1, &high);
  GS_DISPATCH_FLOAT(sdt, SD, GS_DISPATCH_LOWP(ldt, LD, {
    for_ranges(p, [&](int t, int64_t i0, int64_t i1) {
      float* ap = static_cast<float*>(slot(p, 0, t));
      const void* sp = slot(p, 1, t);
      void* lp = slot(p, 2, t);
      if (copy) {
        if constexpr (SD == GS_F32) {
          std::memcpy(ap + i0, static_cast<const float*>(sp) + i0, sizeof(float) * static_cast<size_t>(i1 - i0));
        } else {
          for (int64_t i = i0; i < i1; ++i) ap[i] = ldT<SD>(sp, i);
        }
      } else if (high) {
        for (int64_t i = i0; i < i1; ++i) ap[i] = ema_lerp(true, w, wm1, ap[i], ldT<SD>(sp, i));
      } else {
        for (int64_t i = i0; i < i1; ++i) ap[i] = ema_lerp(false, w, wm1, ap[i], ldT<SD>(sp, i));
      }
      if constexpr (LD >= 0)
        for (int64_t i = i0; i < i1; ++i) stT<LD>(lp, i, ap[i]);
    });
  }));
  return GS_OK;
}

// LARS on the host (include/gsync.h, gs_lars_step): the same contract as the device
// kernels — fp32, every multiply and add rounded once, no fma.  The per-tensor sums of
// LARS and LAMB are one loop: element order, 1 Ki-element blocks folded front to back — a
// fixed order (serial, so the thread count does not enter), not the device's.
// tensor(t) returns the element function of tensor t: (i, a, b) -> the operands of the
// two squares of element i.
template <class Tensor>
static void blockwise_sq_sums(const gs_plan* p, float* norms, Tensor&& tensor) {
  constexpr int64_t kBlk = 1024;
  for (int t = 0; t < p->n; ++t) {
    auto elem = tensor(t);
    float sa = 0.f, sb = 0.f;
    for (int64_t i0 = 0; i0 < p->numel[t]; i0 += kBlk) {
      const int64_t i1 = std::min(p->numel[t], i0 + kBlk);
      float ba = 0.f, bb = 0.f;
      for (int64_t i = i0; i < i1; ++i) {
        float a, b;
        elem(i, a, b);
        ba = ba + a * a;
        bb = bb + b * b;
      }
      sa = sa + ba;
      sb = sb + bb;
    }
    norms[2 * t] = sa;
    norms[2 * t + 1] = sb;
  }
}

int host_lars_norms(gs_plan* p, int gdt, float* norms) {
  GS_DISPATCH_FLOAT(gdt, GD, {
    blockwise_sq_sums(p, norms, [&](int t) {
      const float* pp = static_cast<const float*>(slot(p, 0, t));
      const void* gp = slot(p, 1, t);
      return [=](int64_t i, float& x, float& g) { x = pp[i]; g = ldT<GD>(gp, i); };
    });
  });
  return GS_OK;
}

int host_lars(gs_plan* p, int gdt, int ldt, const LarsHyper& h, const float* norms, const float* gsc,
              const float* fi) {
  GS_TRY_RET(check_float(gdt));
  if (fi && fi[0] != 0.f) return GS_OK;
  const bool has_m = gsc != nullptr;
  const float m = gsc ? gsc[0] : 1.f;
  std::vector<float> slr(p->n), wdt(p->n);
  for (int t = 0; t < p->n; ++t)
    lars_coef(h, norms[2 * t], norms[2 * t + 1], p->adapt.empty() ? 1 : p->adapt[t], has_m, m, &slr[t], &wdt[t]);
  GS_DISPATCH_FLOAT(gdt, GD, GS_DISPATCH_LOWP(ldt, LD, {
    for_ranges(p, [&](int t, int64_t i0, int64_t i1) {
      float* pp = static_cast<float*>(slot(p, 0, t));
      const void* gp = slot(p, 1, t);
      float* bp = static_cast<float*>(slot(p, 2, t));
      [[maybe_unused]] void* lp = slot(p, 3, t);
      const float lr_t = slr[t], wd_t = wdt[t];
      for (int64_t i = i0; i < i1; ++i) {
        float x = pp[i], b = 0.f;
        if (h.mom != 0.f) b = bp[i];  // bp may be NULL without a momentum
        lars_update(h, lr_t, wd_t, has_m, m, ldT<GD>(gp, i), &x, &b);
        pp[i] = x;
        if (h.mom != 0.f) bp[i] = b;
        if constexpr (LD >= 0) stT<LD>(lp, i, x);
      }
    });
  }));
  return GS_OK;
}

// LAMB on the host (include/gsync.h, gs_lamb_moments / gs_lamb_step): the device kernels'
// contract and the same text of the update (lamb_moments / lamb_update / lamb_coef,
// gs_common.h).  The sums are host_lars_norms' loop, with u in place of g; the element
// function also writes m', v'.
int host_lamb_moments(gs_plan* p, int gdt, const LambHyper& h, float* norms, const float* gsc, const float* fi) {
  GS_TRY_RET(check_float(gdt));
  if (fi && fi[0] != 0.f) return GS_OK;
  const bool has_m = gsc != nullptr;
  const float mul = gsc ? gsc[0] : 1.f;
  GS_DISPATCH_FLOAT(gdt, GD, {
    blockwise_sq_sums(p, norms, [&](int t) {
      const float* pp = static_cast<const float*>(slot(p, 0, t));
      const void* gp = slot(p, 1, t);
      float* mp = static_cast<float*>(slot(p, 2, t));
      float* vp = static_cast<float*>(slot(p, 3, t));
      const float wd_t = (p->adapt.empty() || p->adapt[t] != 0) ? h.wd : 0.f;
      return [=](int64_t i, float& x, float& u) {
        float g = ldT<GD>(gp, i);
        if (has_m) g = g * mul;
        lamb_moments(h, g, &mp[i], &vp[i]);
        x = pp[i];
        u = lamb_update(h, x, mp[i], vp[i], wd_t);
      };
    });
  });
  return GS_OK;
}

int host_lamb(gs_plan* p, int ldt, const LambHyper& h, const float* norms, const float* fi) {
  if (fi && fi[0] != 0.f) return GS_OK;
  std::vector<float> slr(p->n), wdt(p->n);
  for (int t = 0; t < p->n; ++t) {
    const int ad = p->adapt.empty() ? 1 : p->adapt[t];
    slr[t] = lamb_coef(h, norms[2 * t], norms[2 * t + 1], ad);
    wdt[t] = ad != 0 ? h.wd : 0.f;
  }
  GS_DISPATCH_LOWP(ldt, LD, {
    for_ranges(p, [&](int t, int64_t i0, int64_t i1) {
      float* pp = static_cast<float*>(slot(p, 0, t));
      const float* mp = static_cast<const float*>(slot(p, 2, t));
      const float* vp = static_cast<const float*>(slot(p, 3, t));
      [[maybe_unused]] void* lp = slot(p, 4, t);
      const float lr_t = slr[t], wd_t = wdt[t];
      for (int64_t i = i0; i < i1; ++i) {
        pp[i] = pp[i] - lr_t * lamb_update(h, pp[i], mp[i], vp[i], wd_t);
        if constexpr (LD >= 0) stT<LD>(lp, i, pp[i]);
      }
    });
  });
  return GS_OK;
}

// Muon on the host (include/gsync.h, gs_muon_*): the device stages restated as plain loops
// on the same padded workspace, with the same rounding points (gs_math.h's muon_* texts).
// A product is summed over ascending k, one fp32 add per bf16 x bf16 product — a fixed
// order that is not the MFMA kernels', so host and device agree to the accumulation order
// only.  Serial: the sizes that reach the host backend are test sizes.
int host_muon_prep(gs_plan* p, int gdt, const MuonHyper& h, float* norms, void* ws) {
  GS_TRY_RET(check_float(gdt));
  GS_DISPATCH_FLOAT(gdt, GD, {
    blockwise_sq_sums(p, norms, [&](int t) {
      const void* gp = slot(p, 1, t);
      float* bp = static_cast<float*>(slot(p, 2, t));
      return [=](int64_t i, float& b, float& u) {
        bp[i] = muon_buf(h, ldT<GD>(gp, i), bp[i]);
        b = bp[i];
        u = muon_u(h, ldT<GD>(gp, i), b);
      };
    });
    uint16_t* w = static_cast<uint16_t*>(ws);
    for (int t = 0; t < p->n; ++t) {
      const MuonDesc& d = p->muon[t];
      const void* gp = slot(p, 1, t);
      const float* bp = static_cast<const float*>(slot(p, 2, t));
      const float s = muon_scale(norms[2 * t + 1], h.eps);
      for (int64_t r = 0; r < d.A; ++r)
        for (int64_t c = 0; c < d.B; ++c) {
          const int64_t e = r * d.B + c;
          w[d.x[0] + (d.tr ? c * d.np + r : r * d.np + c)] = f32_to_bf16(muon_u(h, ldT<GD>(gp, e), bp[e]) * s);
        }
    }
  });
  return GS_OK;
}

// rows [0, rows) x k [0, K) of a bf16 matrix of pitch ld, as fp32
static std::vector<float> muon_widen(const uint16_t* m, int64_t rows, int64_t K, int64_t ld) {
  std::vector<float> f(static_cast<size_t>(rows * K));
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t k = 0; k < K; ++k) f[r * K + k] = bf16_to_f32(m[r * ld + k]);
  return f;
}

int host_muon_syrk(gs_plan* p, void* ws, int poly, int xsel, float alpha, float beta) {
  uint16_t* w = static_cast<uint16_t*>(ws);
  for (int t = 0; t < p->n; ++t) {
    const MuonDesc& d = p->muon[t];
    const int64_t K = poly ? d.mp : d.np, m = d.mp;
    const uint16_t* X = w + (poly ? d.a : d.x[xsel]);
    uint16_t* C = w + (poly ? d.b : d.a);
    const std::vector<float> f = muon_widen(X, m, K, K);
    for (int64_t i = 0; i < m; ++i)
      for (int64_t j = i; j < m; ++j) {
        float acc = 0.f;
        for (int64_t k = 0; k < K; ++k) acc = acc + f[i * K + k] * f[j * K + k];
        const float o = poly ? muon_poly_out(beta, alpha, acc, f[i * K + j]) : muon_gram_out(alpha, acc);
        C[i * m + j] = C[j * m + i] = f32_to_bf16(o);
      }
  }
  return GS_OK;
}

int host_muon_apply(gs_plan* p, void* ws, int xsel, float a) {
  uint16_t* w = static_cast<uint16_t*>(ws);
  for (int t = 0; t < p->n; ++t) {
    const MuonDesc& d = p->muon[t];
    const int64_t m = d.mp, n = d.np;
    const std::vector<float> P = muon_widen(w + d.b, m, m, m), X = muon_widen(w + d.x[xsel], m, n, n);
    uint16_t* Y = w + d.x[xsel ^ 1];
    std::vector<float> acc(static_cast<size_t>(n));
    for (int64_t i = 0; i < m; ++i) {
      std::fill(acc.begin(), acc.end(), 0.f);
      for (int64_t k = 0; k < m; ++k) {  // ascending k for every (i, j)
        const float pk = P[i * m + k];
        for (int64_t j = 0; j < n; ++j) acc[j] = acc[j] + pk * X[k * n + j];
      }
      for (int64_t j = 0; j < n; ++j) Y[i * n + j] = f32_to_bf16(muon_apply_out(a, acc[j], X[i * n + j]));
    }
  }
  return GS_OK;
}

int host_muon_update(gs_plan* p, void* ws, int xsel, double lr, double wd, int adjust) {
  const uint16_t* w = static_cast<const uint16_t*>(ws);
  const float decay = static_cast<float>(1.0 - lr * wd);
  for (int t = 0; t < p->n; ++t) {
    const MuonDesc& d = p->muon[t];
    float* pp = static_cast<float*>(slot(p, 0, t));
    const float adj = static_cast<float>(lr * d.ratio[adjust]);
    for (int64_t r = 0; r < d.A; ++r)
      for (int64_t c = 0; c < d.B; ++c) {
        const float o = bf16_to_f32(w[d.x[xsel] + (d.tr ? c * d.np + r : r * d.np + c)]);
        pp[r * d.B + c] = muon_param(pp[r * d.B + c], decay, adj, o);
      }
  }
  return GS_OK;
}

// PowerSGD on the host (include/gsync.h, gs_psgd_*): the device stages restated as plain loops
// with the same rounding points (every sum of products in fp64, rounded to fp32 once where it
// is stored; the division and the square root of the orthogonalisation), every sum in
// ascending index order — a fixed order that is not the kernels', so host and device agree
// to the accumulation order of the fp64 sums only.  Serial: the sizes
// that reach the host backend are test sizes and gloo rehearsals.
int host_psgd_orthogonalize(gs_plan* p, int which, float* mem, float eps) {
  for (const PsgdDesc& d : p->psgd) {
    const int64_t rows = which ? d.m : d.n, r = d.r;
    float* X = mem + (which ? d.q_off : d.p_off);
    for (int64_t i = 0; i < r; ++i) {
      double nn = 0.0;  // the sums in fp64, rounded once, as on the device
      for (int64_t k = 0; k < rows; ++k) nn = nn + static_cast<double>(X[k * r + i]) * static_cast<double>(X[k * r + i]);
      const float nrm = static_cast<float>(std::sqrt(nn)) + eps;
      for (int64_t k = 0; k < rows; ++k) X[k * r + i] = X[k * r + i] / nrm;
      for (int64_t j = i + 1; j < r; ++j) {
        double dd = 0.0;
        for (int64_t k = 0; k < rows; ++k) dd = dd + static_cast<double>(X[k * r + i]) * static_cast<double>(X[k * r + j]);
        const float dot = static_cast<float>(dd);
        for (int64_t k = 0; k < rows; ++k) X[k * r + j] = X[k * r + j] - dot * X[k * r + i];
      }
    }
  }
  return GS_OK;
}

int host_psgd_project(gs_plan* p, int use_error, float* pmem, const float* qmem) {
  for (int t = 0; t < p->n; ++t) {
    const PsgdDesc& d = p->psgd[t];
    const float* M = static_cast<const float*>(slot(p, 0, t));
    float* E = static_cast<float*>(slot(p, 1, t));
    const float* Q = qmem + d.q_off;
    for (int64_t i = 0; i < d.n; ++i) {
      double acc[kPsgdMaxRank] = {};
      for (int64_t c = 0; c < d.m; ++c) {
        const float e = use_error ? M[i * d.m + c] + E[i * d.m + c] : M[i * d.m + c];
        E[i * d.m + c] = e;
        for (int j = 0; j < d.r; ++j) acc[j] = acc[j] + static_cast<double>(e) * static_cast<double>(Q[c * d.r + j]);
      }
      for (int j = 0; j < d.r; ++j) pmem[d.p_off + i * d.r + j] = static_cast<float>(acc[j]);
    }
  }
  return GS_OK;
}

int host_psgd_backproject(gs_plan* p, const float* pmem, float* qmem) {
  for (int t = 0; t < p->n; ++t) {
    const PsgdDesc& d = p->psgd[t];
    const float* E = static_cast<const float*>(slot(p, 1, t));
    const float* P = pmem + d.p_off;
    float* Q = qmem + d.q_off;
    std::vector<double> acc(static_cast<size_t>(d.m) * d.r, 0.0);
    for (int64_t i = 0; i < d.n; ++i)
      for (int64_t c = 0; c < d.m; ++c)
        for (int j = 0; j < d.r; ++j)
          acc[c * d.r + j] = acc[c * d.r + j] + static_cast<double>(E[i * d.m + c]) * static_cast<double>(P[i * d.r + j]);
    for (size_t e = 0; e < acc.size(); ++e) Q[e] = static_cast<float>(acc[e]);
  }
  return GS_OK;
}

int host_psgd_reconstruct(gs_plan* p, const float* pmem, float* qmem, float inv_ws) {
  for (int t = 0; t < p->n; ++t) {
    const PsgdDesc& d = p->psgd[t];
    float* G = static_cast<float*>(slot(p, 0, t));
    float* E = static_cast<float*>(slot(p, 1, t));
    const float* P = pmem + d.p_off;
    float* Q = qmem + d.q_off;
    for (int64_t e = 0; e < static_cast<int64_t>(d.m) * d.r; ++e) Q[e] = Q[e] * inv_ws;
    for (int64_t i = 0; i < d.n; ++i)
      for (int64_t c = 0; c < d.m; ++c) {
        double s = 0.0;  // fp64 products are exact; one rounding to fp32, as on the device
        for (int j = 0; j < d.r; ++j) s = s + static_cast<double>(P[i * d.r + j]) * static_cast<double>(Q[c * d.r + j]);
        const float a = static_cast<float>(s);
        G[i * d.m + c] = a;
        E[i * d.m + c] = E[i * d.m + c] - a;
      }
  }
  return GS_OK;
}

// Adafactor on the host (include/gsync.h, gs_adafactor_*): the device stages restated as plain
// loops over the descriptor, every sum in ascending index order (a row's sum over c, a column's
// over r, m over r, Σp² and Σu² over (o, i, r, c)) — the lane regimes' order for the factors,
// not the tiled regime's nor the device's order for the two per-tensor sums.  Serial: test sizes.
template <class F>
static void af_each(gs_plan* p, int t, F f) {
  const AfDesc& d = p->af[t];
  const float* G = static_cast<const float*>(slot(p, 1, t));
  float* P = static_cast<float*>(slot(p, 0, t));
  float* rv = static_cast<float*>(slot(p, 2, t));
  float* cv = static_cast<float*>(slot(p, 3, t));
  for (int64_t o = 0; o < d.O; ++o)
    for (int64_t i = 0; i < d.I; ++i) {
      const int64_t b = o * d.I + i, base = o * d.so + i * d.si;
      f(d, b, G + base, P + base, rv + b * d.R, d.vec ? nullptr : cv + b * d.C);
    }
}

int host_adafactor_stats(gs_plan* p, const AfHyper& h, float* sums) {
  for (int t = 0; t < p->n; ++t) {
    float sp = 0.f, su = 0.f;
    af_each(p, t, [&](const AfDesc& d, int64_t, const float* G, float* P, float* rv, float* cv) {
      if (d.vec) {
        const float g = G[0];
        rv[0] = ema_lerp(h.high, h.w, h.wm1, rv[0], g * g);
        const float u = af_u(g, af_v_vec(h, rv[0]));
        sp = sp + P[0] * P[0];
        su = su + u * u;
        return;
      }
      float rsum = 0.f;
      for (int64_t r = 0; r < d.R; ++r) {
        float s = 0.f;
        for (int64_t c = 0; c < d.C; ++c) s = s + G[r * d.sr + c * d.sc] * G[r * d.sr + c * d.sc];
        rv[r] = af_factor(h, rv[r], s, d.C);
        rsum = rsum + rv[r];
      }
      for (int64_t c = 0; c < d.C; ++c) {
        float s = 0.f;
        for (int64_t r = 0; r < d.R; ++r) s = s + G[r * d.sr + c * d.sc] * G[r * d.sr + c * d.sc];
        cv[c] = af_factor(h, cv[c], s, d.R);
      }
      const float m = af_m(h, rsum, d.R);
      for (int64_t r = 0; r < d.R; ++r)
        for (int64_t c = 0; c < d.C; ++c) {
          const int64_t e = r * d.sr + c * d.sc;
          const float u = af_u(G[e], af_v(h, rv[r], cv[c], m));
          sp = sp + P[e] * P[e];
          su = su + u * u;
        }
    });
    sums[2 * t] = sp;
    sums[2 * t + 1] = su;
  }
  return GS_OK;
}

int host_adafactor_step(gs_plan* p, const AfHyper& h, float rho, float decay, float eps2, float dclip, int maximize,
                        const float* sums) {
  for (int t = 0; t < p->n; ++t) {
    const float scale = af_scale(sums[2 * t], sums[2 * t + 1], p->af[t].numel, eps2, rho, dclip);
    af_each(p, t, [&](const AfDesc& d, int64_t, const float* G, float* P, float* rv, float* cv) {
      if (d.vec) {
        P[0] = af_param(P[0], decay, scale, af_u(G[0], af_v_vec(h, rv[0])), maximize);
        return;
      }
      float rsum = 0.f;
      for (int64_t r = 0; r < d.R; ++r) rsum = rsum + rv[r];
      const float m = af_m(h, rsum, d.R);
      for (int64_t r = 0; r < d.R; ++r)
        for (int64_t c = 0; c < d.C; ++c) {
          const int64_t e = r * d.sr + c * d.sc;
          P[e] = af_param(P[e], decay, scale, af_u(G[e], af_v(h, rv[r], cv[c], m)), maximize);
        }
    });
  }
  return GS_OK;
}

// CAME on the host (include/gsync.h, gs_came_*): the three stages as plain loops over the
// descriptor, every sum in ascending index order, as host_adafactor_* above.  gs_came_moment
// advances m, R and C of every tensor here (on the device the lane regimes do that inside
// gs_came_step); gs_came_step then only writes p.  Serial: test sizes.
struct CameMat {
  const float* G;
  float *P, *M, *rv, *cv, *Rv, *Cv;
};
template <class F>
static void came_each(gs_plan* p, int t, F f) {
  const AfDesc& d = p->af[t];
  const float* G = static_cast<const float*>(slot(p, 1, t));
  float* P = static_cast<float*>(slot(p, 0, t));
  float* M = static_cast<float*>(slot(p, 4, t));
  float* s[4] = {static_cast<float*>(slot(p, 2, t)), static_cast<float*>(slot(p, 3, t)),
                 static_cast<float*>(slot(p, 5, t)), static_cast<float*>(slot(p, 6, t))};
  for (int64_t o = 0; o < d.O; ++o)
    for (int64_t i = 0; i < d.I; ++i) {
      const int64_t b = o * d.I + i, base = o * d.so + i * d.si;
      if (d.vec)
        f(d, CameMat{G + base, P + base, M + base, s[0] + b, nullptr, nullptr, nullptr});
      else
        f(d, CameMat{G + base, P + base, M + base, s[0] + b * d.R, s[1] + b * d.C, s[2] + b * d.R, s[3] + b * d.C});
    }
}
static float came_row_mean(const AfDesc& d, const float* rv) {
  float s = 0.f;
  for (int64_t r = 0; r < d.R; ++r) s = s + rv[r];
  return came_mean(s, d.R);
}

int host_came_stats(gs_plan* p, const CameHyper& h, float* sums) {
  for (int t = 0; t < p->n; ++t) {
    float su = 0.f;
    came_each(p, t, [&](const AfDesc& d, const CameMat& x) {
      if (d.vec) {
        x.rv[0] = came_ema(x.rv[0], came_sq(x.G[0], h.eps1), h.b2, h.omb2);
        const float u = x.G[0] * came_cf(x.rv[0]);
        su = su + u * u;
        return;
      }
      for (int64_t r = 0; r < d.R; ++r) {
        float s = 0.f;
        for (int64_t c = 0; c < d.C; ++c) s = s + came_sq(x.G[r * d.sr + c * d.sc], h.eps1);
        x.rv[r] = came_factor(x.rv[r], s, d.C, h.b2, h.omb2);
      }
      for (int64_t c = 0; c < d.C; ++c) {
        float s = 0.f;
        for (int64_t r = 0; r < d.R; ++r) s = s + came_sq(x.G[r * d.sr + c * d.sc], h.eps1);
        x.cv[c] = came_factor(x.cv[c], s, d.R, h.b2, h.omb2);
      }
      const float mean = came_row_mean(d, x.rv);
      for (int64_t r = 0; r < d.R; ++r)
        for (int64_t c = 0; c < d.C; ++c) {
          const float u = came_dir(x.G[r * d.sr + c * d.sc], came_rf(x.rv[r], mean), came_cf(x.cv[c]));
          su = su + u * u;
        }
    });
    sums[t] = su;
  }
  return GS_OK;
}

int host_came_moment(gs_plan* p, const CameHyper& h, const float* sums) {
  std::vector<float> qc;
  for (int t = 0; t < p->n; ++t) {
    const float denom = came_denom(sums[t], p->af[t].numel, h.d);
    came_each(p, t, [&](const AfDesc& d, const CameMat& x) {
      if (d.vec) {
        x.M[0] = came_ema(x.M[0], x.G[0] * came_cf(x.rv[0]) / denom, h.b1, h.omb1);
        return;
      }
      const float mean = came_row_mean(d, x.rv);
      qc.assign(d.C, 0.f);
      for (int64_t r = 0; r < d.R; ++r) {
        float s = 0.f;
        for (int64_t c = 0; c < d.C; ++c) {
          const int64_t e = r * d.sr + c * d.sc;
          const float uh = came_dir(x.G[e], came_rf(x.rv[r], mean), came_cf(x.cv[c])) / denom;
          x.M[e] = came_ema(x.M[e], uh, h.b1, h.omb1);
          const float q = came_res(uh, x.M[e], h.eps2);
          s = s + q;
          qc[c] = qc[c] + q;
        }
        x.Rv[r] = came_factor(x.Rv[r], s, d.C, h.b3, h.omb3);
      }
      for (int64_t c = 0; c < d.C; ++c) x.Cv[c] = came_factor(x.Cv[c], qc[c], d.R, h.b3, h.omb3);
    });
  }
  return GS_OK;
}

int host_came_step(gs_plan* p, const CameHyper& h) {
  for (int t = 0; t < p->n; ++t)
    came_each(p, t, [&](const AfDesc& d, const CameMat& x) {
      if (d.vec) {
        x.P[0] = came_param(h, x.P[0], x.M[0]);
        return;
      }
      const float Mean = came_row_mean(d, x.Rv);
      for (int64_t r = 0; r < d.R; ++r)
        for (int64_t c = 0; c < d.C; ++c) {
          const int64_t e = r * d.sr + c * d.sc;
          x.P[e] = came_param(h, x.P[e], came_dir(x.M[e], came_rf(x.Rv[r], Mean), came_cf(x.Cv[c])));
        }
    });
  return GS_OK;
}

// A pairwise sum of terms pushed one by one: a binary counter of finished subtrees, small ones
// folded first, so at most ceil(log2 n) roundings lie on any path, as in the device's tree
// (gs_wave.h); its order differs from the device's.
struct PairSum {
  float acc[32];
  // j: how many terms were pushed before this one
  void push(float e, uint32_t j) {
    int l = 0;
    for (; j & (1u << l); ++l) e = acc[l] + e;
    acc[l] = e;
  }
  float fold(uint32_t n) const {
    float s = 0.f;
    bool any = false;
    for (int l = 0; l < 31; ++l) {
      if (n & (1u << l)) {
        s = any ? acc[l] + s : acc[l];
        any = true;
      }
    }
    return s;
  }
};

// gs_eval_accumulate on the host: the rules of include/gsync.h row by row.  The sum of the
// exponentials is a PairSum: the losses may differ from the device's by a few ulps, the counts
// do not.
template <int DT>
void host_eval_rows(const void* logits, const int64_t* labels, int64_t B, int K, int64_t row_stride,
                    int64_t n_valid, int64_t ignore_index, EvalRow* ws) {
  for (int64_t row = 0; row < B; ++row) {
    const int64_t y = labels[row];
    if (row >= n_valid || y == ignore_index) {
      ws[row] = EvalRow{0.f, kEvalSkip};
      continue;
    }
    if (y < 0 || y >= K) {
      ws[row] = EvalRow{0.f, kEvalBad};
      continue;
    }
    const int64_t base = row * row_stride;
    const float zy = ldT<DT>(logits, base + y);
    float m = -INFINITY;
    bool nan = false;
    for (int j = 0; j < K; ++j) {
      const float z = ldT<DT>(logits, base + j);
      nan |= z != z;
      m = z > m ? z : m;
    }
    if (nan) {
      ws[row] = EvalRow{std::nanf(""), kEvalNanRow};
      continue;
    }
    PairSum se;
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const float z = ldT<DT>(logits, base + j);
      rank += (z > zy) || (z == zy && j < y);
      se.push(expf(z - m), static_cast<uint32_t>(j));
    }
    ws[row] = EvalRow{eval_loss(m, se.fold(static_cast<uint32_t>(K)), zy), rank};
  }
}

int host_eval_accumulate(const void* logits, int dt, const int64_t* labels, int64_t B, int K, int64_t row_stride,
                         int64_t n_valid, const EvalTopk& topk, int64_t ignore_index, void* ws, void* acc) {
  EvalRow* wp = static_cast<EvalRow*>(ws);
  GS_DISPATCH_FLOAT(dt, DT, host_eval_rows<DT>(logits, labels, B, K, row_stride, n_valid, ignore_index, wp));
  int64_t* ap = static_cast<int64_t*>(acc);
  double total = 0.0;
  for (int64_t r = 0; r < B; ++r) {  // ascending row order
    const EvalRow w = wp[r];
    if (w.code >= 0) {
      total += static_cast<double>(w.loss);
      ap[0] += 1;
      for (int i = 0; i < topk.n; ++i) ap[4 + i] += w.code < topk.k[i];
    } else if (w.code == kEvalBad) {
      ap[1] += 1;
    }
  }
  double cur;
  std::memcpy(&cur, ap + 2, 8);
  cur = cur + total;
  std::memcpy(ap + 2, &cur, 8);
  return GS_OK;
}

// gs_xent_fwd and (labels_b, lam not null) gs_xent_mix_fwd on the host: the rules of include/gsync.h row by
// row, the sums as PairSums.
template <int DT>
void host_xent_rows(const void* logits, const int64_t* labels, const int64_t* labels_b, const float* lamv, int64_t B,
                    int K, int64_t row_stride, int64_t ignore_index, float eps, XentRow* rows, double* nll) {
  for (int64_t row = 0; row < B; ++row) {
    int64_t y = labels[row];  // the label the rank is counted against
    const int64_t ya = y;
    int64_t yb = y;
    float lam = 1.f;
    bool one = true;
    nll[row] = 0.0;
    if (labels_b) {
      yb = labels_b[row], lam = lamv[row];
      const int32_t code = xent_mix_code(ya, yb, lam, K, ignore_index);
      if (code < 0) {
        rows[row] = XentRow{0.f, 0.f, 0.f, code};
        continue;
      }
      one = xent_mix_one(ya, yb, lam);
      y = one ? ya : xent_mix_dominant(ya, yb, lam);
    } else if (y == ignore_index || y < 0 || y >= K) {
      rows[row] = XentRow{0.f, 0.f, 0.f, y == ignore_index ? kEvalSkip : kEvalBad};
      continue;
    }
    const int64_t base = row * row_stride;
    const float zy = ldT<DT>(logits, base + y);
    float m = -INFINITY;
    bool nan = false;
    for (int j = 0; j < K; ++j) {
      const float z = ldT<DT>(logits, base + j);
      nan |= z != z;
      m = z > m ? z : m;
    }
    if (nan) {
      const float q = std::nanf("");
      rows[row] = XentRow{q, q, q, kEvalNanRow};
      nll[row] = q;
      continue;
    }
    PairSum se, sz;
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const float z = ldT<DT>(logits, base + j);
      rank += (z > zy) || (z == zy && j < y);
      se.push(expf(z - m), static_cast<uint32_t>(j));
      if (eps != 0.f) sz.push(z, static_cast<uint32_t>(j));
    }
    const float logS = logf(se.fold(static_cast<uint32_t>(K)));
    const float t = eps != 0.f ? sz.fold(static_cast<uint32_t>(K)) : 0.f;
    if (!one) {
      const float za = ldT<DT>(logits, base + ya), zb = ldT<DT>(logits, base + yb);
      rows[row] = XentRow{xent_mix_loss(m, logS, za, zb, lam, t, K, eps), m, logS, rank};
      nll[row] = static_cast<double>(xent_mix_loss(m, logS, za, zb, lam, 0.f, 1, 0.f));
      continue;
    }
    rows[row] = XentRow{xent_loss(m, logS, zy, t, K, eps), m, logS, rank};
    nll[row] = static_cast<double>((m - zy) + logS);
  }
}

int host_xent_mix_fwd(const void* logits, int dt, const int64_t* labels, const int64_t* labels_b, const float* lam,
                      int64_t B, int K, int64_t row_stride, int64_t ignore_index, float eps, void* rows, void* red,
                      const EvalTopk& topk, void* acc) {
  XentRow* rp = static_cast<XentRow*>(rows);
  std::vector<double> nll(static_cast<size_t>(B));
  GS_DISPATCH_FLOAT(dt, DT, host_xent_rows<DT>(logits, labels, labels_b, lam, B, K, row_stride, ignore_index, eps, rp,
                                               nll.data()));
  int64_t* ap = B > 0 ? static_cast<int64_t*>(acc) : nullptr;
  int64_t counted = 0, bad = 0;
  double total = 0.0, total_nll = 0.0;
  for (int64_t r = 0; r < B; ++r) {  // ascending row order
    const XentRow w = rp[r];
    if (w.code >= 0) {
      total += static_cast<double>(w.loss);
      total_nll += nll[r];
      counted += 1;
      if (ap)
        for (int i = 0; i < topk.n; ++i) ap[4 + i] += w.code < topk.k[i];
    } else if (w.code == kEvalBad) {
      bad += 1;
    }
  }
  *static_cast<XentRed*>(red) = xent_reduce(total, counted, bad);
  if (ap) {
    ap[0] += counted;
    ap[1] += bad;
    double cur;
    std::memcpy(&cur, ap + 2, 8);
    cur = cur + total_nll;
    std::memcpy(ap + 2, &cur, 8);
  }
  return GS_OK;
}

template <int DT>
void host_xent_grad(const void* logits, const int64_t* labels, const int64_t* labels_b, const float* lamv, int64_t B,
                    int K, int64_t row_stride, float eps, int reduction, const XentRow* rows, const XentRed* red, const float* grad_out, void* dlogits,
                    int64_t d_row_stride) {
  const float q_off = eps / static_cast<float>(K);
  const float q_on = (1.f - eps) + q_off;
  for (int64_t row = 0; row < B; ++row) {
    const XentRow w = rows[row];
    const int64_t zb = row * row_stride, db = row * d_row_stride;
    if (w.code < 0) {
      for (int j = 0; j < K; ++j) stT<DT>(dlogits, db + j, 0.f);
      continue;
    }
    const int64_t y = labels[row];
    int64_t yb = -1;  // a mixed row's second label, with targets qa at y and qb at yb
    float qa = q_on, qb = q_off;
    if (labels_b && !xent_mix_one(y, labels_b[row], lamv[row])) {
      yb = labels_b[row];
      qa = xent_mix_q(eps, lamv[row], q_off);
      qb = xent_mix_q(eps, 1.f - lamv[row], q_off);
    }
    const float g = grad_out[reduction == kXentNone ? row : 0];
    const float c = reduction == kXentMean ? g / static_cast<float>(red->counted) : g;
    for (int j = 0; j < K; ++j) {
      const float q = j == y ? qa : j == yb ? qb : q_off;
      stT<DT>(dlogits, db + j, xent_grad(ldT<DT>(logits, zb + j), w.m, w.logS, q, c));
    }
  }
}

int host_xent_mix_bwd(const void* logits, int dt, const int64_t* labels, const int64_t* labels_b, const float* lam,
                      int64_t B, int K, int64_t row_stride, float eps, int reduction, const void* rows,
                      const void* red, const float* grad_out, void* dlogits, int64_t d_row_stride) {
  GS_DISPATCH_FLOAT(dt, DT, host_xent_grad<DT>(logits, labels, labels_b, lam, B, K, row_stride, eps, reduction,
                                               static_cast<const XentRow*>(rows), static_cast<const XentRed*>(red),
                                               grad_out, dlogits, d_row_stride));
  return GS_OK;
}

// ------------------------------------------------------------------------------------------------
// gs_quant_perchannel / gs_quant_pertensor / gs_dequant_mean on the host: the rules of
// include/gsync.h channel by channel, on gs_math.h's per-element functions.
int host_quant(const float* x, int64_t n, int bucket_size, void* payload) {
  const QuantLayout l = quant_layout(n, bucket_size);
  uint8_t* q = static_cast<uint8_t*>(payload);
  float* scales = reinterpret_cast<float*>(q + l.Q);
  int32_t* zps = reinterpret_cast<int32_t*>(q + l.Q + 4 * l.C);
  const int64_t width = bucket_size ? bucket_size : n;
  for (int64_t c = 0; c < l.C; ++c) {
    const int64_t e0 = c * width, e1 = std::min(n, e0 + width);
    float lo = 0.f, hi = 0.f;
    for (int64_t e = e0; e < e1; ++e) quant_fold(x[e], &lo, &hi);
    const QuantParams qp = quant_params(lo, hi);
    const float zpf = static_cast<float>(qp.zp);
    for (int64_t e = e0; e < e1; ++e) q[e] = static_cast<uint8_t>(quant_value(x[e], qp.scale, zpf));
    for (int64_t e = e1; e < e0 + width; ++e) q[e] = static_cast<uint8_t>(quant_value(0.f, qp.scale, zpf));
    scales[c] = qp.scale;
    zps[c] = qp.zp;
  }
  return GS_OK;
}

int host_dequant_mean(const void* gathered, int world_size, float* out, int64_t n, int bucket_size) {
  const QuantLayout l = quant_layout(n, bucket_size);
  const uint8_t* g = static_cast<const uint8_t*>(gathered);
  const float d = static_cast<float>(world_size);
  for (int64_t e = 0; e < n; ++e) {
    const int64_t c = bucket_size ? e / bucket_size : 0;
    float a = 0.f;
    for (int r = 0; r < world_size; ++r) {
      const uint8_t* p = g + r * l.bytes();
      const float scale = reinterpret_cast<const float*>(p + l.Q)[c];
      const float zpf = static_cast<float>(reinterpret_cast<const int32_t*>(p + l.Q + 4 * l.C)[c]);
      const float t = dequant_value(p[e], scale, zpf);
      a = r ? a + t : t;
    }
    out[e] = a / d;
  }
  return GS_OK;
}

}  // namespace gs

extern "C" int gs_set_host_threads(int n) {
  gs::g_threads.store(n < 1 ? 1 : (n > 256 ? 256 : n));
  return GS_OK;
}
