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

}  // namespace gs

extern "C" int gs_set_host_threads(int n) {
  gs::g_threads.store(n < 1 ? 1 : (n > 256 ? 256 : n));
  return GS_OK;
}
