// gfx950 (CDNA4) fused SGD / Adam(W) / LARS updates of libgsync (gs_sgd_step / gs_adam_step /
// gs_lars_step[_lowp]): the chunk-map engine of gs_engine.h with SgdOp / AdamOp / LarsOp, the
// grad-load policy per launch; LARS's per-tensor Σp², Σg² (gs_lars_norms), a segmented
// reduction over the same chunk map; and LAMB (gs_lamb_moments / gs_lamb_step): that
// reduction fused with the moments' read-modify-write, then LambOp on the engine; and the
// EMA / SWA weight average (gs_ema_step / gs_ema_hyper): EmaOp on the engine.

#include "gs_engine.h"

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

// ------------------------------------------------------------------- LARS
// Per-tensor Σp², Σg² (gs_lars_norms): a segmented reduction on the chunk map.  The
// host numbers one partial slot per (chunk, tensor intersecting it) pair, in chunk
// order then tensor order — a full chunk has one, a mixed chunk of span k has k —
// so a tensor's slots are the contiguous range [first, first + count).  Every slot
// is written by exactly one workgroup, with a sum whose order the chunk alone fixes:
//   full chunk   each lane squares its 4 + 4 elements in element order, then the
//                fixed DPP tree per wave and the 4 wave sums in wave order;
//   mixed chunk  each lane leaves its two sums in LDS; lanes of one tensor are
//                contiguous, and thread i adds up tensor t0 + i's lane range in
//                lane order (any span: threads stride over it, nothing is staged
//                per tensor, so spans above kMixedStage take the same path).
// lars_norm_finish then folds each tensor's slots with one workgroup: thread j adds slots
// j, j + 256, ... in order, then the same fixed tree.  Nothing depends on the grid or on
// arrival order and there are no floating-point atomics: replicas holding the same
// p and g publish the same bits.
// Both streams take plain cached loads: the update re-reads the same bytes right
// behind, and a ResNet-50's p + g (204 MB) fit the Infinity Cache.
struct LarsMap {
  const int32_t* cb;  // [n_chunks]: first partial slot of each chunk
  const int32_t* tb;  // [2n]: first slot, slot count of each tensor
  float* part;        // [2 * slots]: Σp², Σg² per slot
};

template <int K>
__device__ __forceinline__ void lars_block_sum(float (&v)[K], float* s_red) {
  // result in thread 0's v
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_red[w * K + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float r = s_red[k];
#pragma unroll
      for (int i = 1; i < kBlock / 64; ++i) r = r + s_red[i * K + k];
      v[k] = r;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ float lars_sq4(const float (&x)[4]) {
  float s = x[0] * x[0];
  s = s + x[1] * x[1];
  s = s + x[2] * x[2];
  s = s + x[3] * x[3];
  return s;
}

// the lane's 4 + 4 elements of full chunk c of tensor t (uniform descriptor loads)
template <int GD>
__device__ __forceinline__ void lars_full_load(const PlanArgs& P, int t, int64_t c, float (&x)[4], float (&g)[4]) {
  const void* pp = cload(P.ptrs, t);
  const void* gp = cload(P.ptrs, static_cast<int64_t>(P.n) + t);
  const uint32_t a = cload(P.align, t);
  const int64_t e0 = c * kChunkElems - cload(P.voff, t);
  const uint32_t lo = threadIdx.x * kUnit;
  if ((a & 3u) == 3u) {
    load4F<GS_F32>(elem_at<GS_F32>(pp, e0), lo, x);
    load4F<GD>(elem_at<GD>(gp, e0), lo, g);
  } else {
    const int64_t n = cload(P.numel, t);
    loadN<GS_F32, 4>(pp, e0 + lo, n, false, x);
    loadN<GD, 4>(gp, e0 + lo, n, false, g);
  }
}

template <int GD>
__device__ __forceinline__ void lars_mixed(const PlanArgs& P, const LarsMap& M, int t0, int span, int64_t c,
                                           float* s_p, float* s_g) {
  const int64_t cs = c * kChunkElems;
  const int64_t e = cs + static_cast<int>(threadIdx.x) * kUnit;
  int lo = t0, hi = t0 + span - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (P.voff[mid] <= e) lo = mid; else hi = mid - 1;
  }
  float sp = 0.f, sg = 0.f;
  const int64_t local = e - P.voff[lo];
  const int64_t n = P.numel[lo];
  if (local >= 0 && local < n) {  // else: an alignment gap between tensors
    const uint32_t a = P.align[lo];
    float x[4], g[4];
    loadN<GS_F32, 4>(P.ptrs[lo], local, n, (a & 1u) != 0, x);
    loadN<GD, 4>(P.ptrs[static_cast<int64_t>(P.n) + lo], local, n, (a & 2u) != 0, g);
    sp = lars_sq4(x);
    sg = lars_sq4(g);
  }
  __syncthreads();  // the previous mixed chunk's readers are done with the stage
  s_p[threadIdx.x] = sp;
  s_g[threadIdx.x] = sg;
  __syncthreads();
  const int slot0 = M.cb[c];
  for (int i = static_cast<int>(threadIdx.x); i < span; i += kBlock) {
    const int t = t0 + i;
    const int64_t b = P.voff[t] - cs, end = b + P.numel[t];  // the tensor's range, relative to the chunk
    const int l0 = b <= 0 ? 0 : static_cast<int>(std::min<int64_t>(kBlock, b / kUnit));
    const int l1 = end <= 0 ? 0 : static_cast<int>(std::min<int64_t>(kBlock, (end + kUnit - 1) / kUnit));
    float ap = 0.f, ag = 0.f;
    for (int l = l0; l < l1; ++l) {
      ap = ap + s_p[l];
      ag = ag + s_g[l];
    }
    M.part[2 * static_cast<int64_t>(slot0 + i)] = ap;
    M.part[2 * static_cast<int64_t>(slot0 + i) + 1] = ag;
  }
}

// chunks per workgroup iteration: a group of kLarsG full chunks (of one tensor or
// several: every chunk has its own slot) has all 2 * kLarsG accesses of a lane in
// flight before one barrier pair
#ifndef GS_G_LARS_NORM
#define GS_G_LARS_NORM 4
#endif
constexpr int kLarsG = GS_G_LARS_NORM;

template <int GD>
__global__ void __launch_bounds__(kBlock) GS_SGPR_ATTR lars_norm_kernel(PlanArgs P, LarsMap M) {
  constexpr int G = kLarsG;
  __shared__ float s_p[kBlock], s_g[kBlock], s_red[2 * G * (kBlock / 64)];
  const int* cw = &P.chunks[0].t0;  // [t0, code] pairs
  const int64_t n_groups = (static_cast<int64_t>(P.n_chunks) + G - 1) / G;
  for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int64_t c0 = G * g;
    int t[G], code[G];
    bool all_full = true;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const bool in = c0 + j < P.n_chunks;
      t[j] = in ? cload(cw, 2 * (c0 + j)) : -1;
      code[j] = in ? cload(cw, 2 * (c0 + j) + 1) : -1;
      all_full = all_full && code[j] == 0;
    }
    if (all_full) {
      float x[G][4], y[G][4], v[2 * G];
#pragma unroll
      for (int j = 0; j < G; ++j) lars_full_load<GD>(P, t[j], c0 + j, x[j], y[j]);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        v[2 * j] = lars_sq4(x[j]);
        v[2 * j + 1] = lars_sq4(y[j]);
      }
      lars_block_sum<2 * G>(v, s_red);
      if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
          const int64_t s = cload(M.cb, c0 + j);
          M.part[2 * s] = v[2 * j];
          M.part[2 * s + 1] = v[2 * j + 1];
        }
      }
      continue;
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int64_t c = c0 + j;
      if (code[j] == 0) {
        float x[4], y[4];
        lars_full_load<GD>(P, t[j], c, x, y);
        float v[2] = {lars_sq4(x), lars_sq4(y)};
        lars_block_sum<2>(v, s_red);
        if (threadIdx.x == 0) {
          const int64_t s = cload(M.cb, c);
          M.part[2 * s] = v[0];
          M.part[2 * s + 1] = v[1];
        }
      } else if (code[j] > 0) {
        lars_mixed<GD>(P, M, t[j], code[j], c, s_p, s_g);
      }
    }
  }
}

// One workgroup per tensor folds the tensor's slots: thread j adds slots j, j + 256, ...
// in order (4 loads in flight per round; an absent slot adds +0, and the sums are never
// -0), then the DPP tree per wave and the 4 wave sums in wave order.
__global__ void __launch_bounds__(kBlock) lars_norm_finish(const int32_t* tb, const float* part, int n,
                                                           float* norms) {
  __shared__ float s_red[2 * (kBlock / 64)];
  const int t = blockIdx.x;
  if (t >= n) return;  // whole workgroups
  const int cnt = tb[2 * t + 1];
  const float2* p2 = reinterpret_cast<const float2*>(part) + tb[2 * t];  // hipMalloc'd, 256-B aligned: 8-B pairs
  float v[2] = {0.f, 0.f};
  for (int base = threadIdx.x; base < cnt; base += 4 * kBlock) {
    float2 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = base + u * kBlock < cnt ? p2[base + u * kBlock] : make_float2(0.f, 0.f);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[0] = v[0] + x[u].x;
      v[1] = v[1] + x[u].y;
    }
  }
  lars_block_sum<2>(v, s_red);
  if (threadIdx.x == 0) {
    norms[2 * t] = v[0];
    norms[2 * t + 1] = v[1];
  }
}

// The plan's LARS scratch: chunk slot bases | per-tensor [first, count] | adapt | partial
// slots.  Built and uploaded once, at gs_plan_set_adapt or the first gs_lars_norms.
static size_t lars_al(size_t x) { return (x + 255) & ~size_t(255); }
static size_t lars_tb_off(const gs_plan* p) { return lars_al(sizeof(int32_t) * std::max<size_t>(1, p->chunks.size())); }
static size_t lars_adapt_off(const gs_plan* p) { return lars_tb_off(p) + lars_al(sizeof(int32_t) * 2 * p->n); }
static size_t lars_part_off(const gs_plan* p) { return lars_adapt_off(p) + lars_al(sizeof(int32_t) * p->n); }
static char* lars_tb_ptr(const gs_plan* p) { return static_cast<char*>(p->d_lars) + lars_tb_off(p); }
static char* lars_adapt_ptr(const gs_plan* p) { return static_cast<char*>(p->d_lars) + lars_adapt_off(p); }
static char* lars_part_ptr(const gs_plan* p) { return static_cast<char*>(p->d_lars) + lars_part_off(p); }

static int lars_prepare(gs_plan* p, void* stream) {
  if (p->d_lars || p->n == 0) return GS_OK;
  if (stream_capturing(stream))
    return fail(GS_ESTATE, "LARS scratch of the plan is not allocated yet: call gs_plan_set_adapt or one "
                           "gs_lars_norms outside the capture first");
  const size_t nc = p->chunks.size();
  std::vector<int32_t> cb(std::max<size_t>(1, nc), 0), tb(2 * static_cast<size_t>(p->n), 0);
  int64_t slots = 0;
  for (size_t c = 0; c < nc; ++c) {
    cb[c] = static_cast<int32_t>(slots);
    const ChunkDesc& d = p->chunks[c];
    const int k = d.code == 0 ? 1 : (d.code > 0 ? d.code : 0);
    for (int i = 0; i < k; ++i) {
      const int t = d.t0 + i;
      if (tb[2 * t + 1] == 0) tb[2 * t] = static_cast<int32_t>(slots + i);
      // contiguous: a tensor spanning chunks is the last of its first chunk's span and
      // the first of every later one
      if (tb[2 * t] + tb[2 * t + 1] != slots + i) return fail(GS_ESTATE, "LARS slot map: a tensor's slots are not contiguous");
      ++tb[2 * t + 1];
    }
    slots += k;
    if (slots > (int64_t(1) << 30)) return fail(GS_EINVAL, "LARS slot map: plan too large");
  }
  p->lars_slots = slots;
  const size_t total = lars_part_off(p) + sizeof(float) * 2 * static_cast<size_t>(std::max<int64_t>(1, slots));
  void* d = nullptr;
  HIP_RET(hipMalloc(&d, total));
  p->d_lars = d;
  std::vector<int32_t> ad(p->n, 1);
  if (!p->adapt.empty()) ad = p->adapt;
  hipError_t e = hipMemcpy(p->d_lars, cb.data(), sizeof(int32_t) * cb.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(lars_tb_ptr(p), tb.data(), sizeof(int32_t) * tb.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(lars_adapt_ptr(p), ad.data(), sizeof(int32_t) * ad.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(p->d_lars);
    p->d_lars = nullptr;
    return fail(GS_EHIP, std::string("LARS scratch upload failed: ") + hipGetErrorString(e));
  }
  return GS_OK;
}

int hip_lars_set_adapt(gs_plan* p) {
  DeviceGuard g(p->device);
  if (p->n == 0) return GS_OK;
  if (!p->d_lars) return lars_prepare(p, nullptr);  // uploads p->adapt
  HIP_RET(hipMemcpy(lars_adapt_ptr(p), p->adapt.data(), sizeof(int32_t) * p->n, hipMemcpyHostToDevice));
  return GS_OK;
}

// A chunk pass that writes the plan's partial slots (G chunks per workgroup iteration),
// then lars_norm_finish: the launch timer takes the pair as one record of `kind`, the
// chunk pass's start and the fold's stop.  pass(grid, s, ev0, a, m) launches the chunk
// pass (ev0 != NULL: with that start event).
template <class Pass>
static int lars_segmented(gs_plan* p, float* norms, void* stream, int kind, int G, Pass&& pass) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  GS_TRY_RET(lars_prepare(p, stream));
  GS_TRY_RET(hip_plan_flush(p, stream));
  const bool capturing = stream_capturing(s);
  const int nslots = capturing ? 0 : static_cast<int>(p->timer_ev.size() / 2);
  const int tk = p->timer_next;
  hipEvent_t ev0 = nslots ? static_cast<hipEvent_t>(p->timer_ev[2 * tk]) : nullptr;
  hipEvent_t ev1 = nslots ? static_cast<hipEvent_t>(p->timer_ev[2 * tk + 1]) : nullptr;
  const LarsMap m{reinterpret_cast<const int32_t*>(p->d_lars), reinterpret_cast<const int32_t*>(lars_tb_ptr(p)),
                  reinterpret_cast<float*>(lars_part_ptr(p))};
  const int64_t groups = (static_cast<int64_t>(p->chunks.size()) + G - 1) / G;
  if (groups > 0) {
    const int grid = static_cast<int>(std::min<int64_t>(groups, p->grid_cap));
    const PlanArgs a = p->args();
    GS_TRY_RET(pass(grid, s, ev0, a, m));
    HIP_RET(hipGetLastError());
    ev0 = nullptr;
  }
  const int fgrid = p->n;
  if (nslots)
    hipExtLaunchKernelGGL(lars_norm_finish, dim3(fgrid), dim3(kBlock), 0, s, ev0, ev1, 0, m.tb,
                          (const float*)m.part, p->n, norms);
  else
    hipLaunchKernelGGL(lars_norm_finish, dim3(fgrid), dim3(kBlock), 0, s, m.tb, (const float*)m.part, p->n, norms);
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

int hip_lars_norms(gs_plan* p, int gdt, float* norms, void* stream) {
  DeviceGuard g(p->device);
  if (p->n == 0) return GS_OK;
  return lars_segmented(p, norms, stream, GS_OP_LARS_NORM, kLarsG,
                        [&](int grid, hipStream_t s, hipEvent_t ev0, const PlanArgs& a, const LarsMap& m) -> int {
    GS_DISPATCH_FLOAT(gdt, GD, {
      if (ev0)
        hipExtLaunchKernelGGL((lars_norm_kernel<GD>), dim3(grid), dim3(kBlock), 0, s, ev0, nullptr, 0, a, m);
      else
        hipLaunchKernelGGL((lars_norm_kernel<GD>), dim3(grid), dim3(kBlock), 0, s, a, m);
    });
    return GS_OK;
  });
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
// pass is also the moments pass — an element-wise read-modify-write of (m, v) and the
// segmented reduction of gs_lars_norms in one kernel.  The slot map, the order inside a
// chunk and the fold (lars_norm_finish) are LARS's, with u² in place of g²: per full
// chunk each lane squares its 4 + 4 values in element order, then the DPP tree and the
// 4 wave sums in wave order; per mixed chunk thread i adds up tensor t0 + i's lanes in
// lane order.  m', v' are stored (non-temporal, as every store of the engine); u is not:
// LambOp recomputes it from (p, m', v') by the same text (lamb_update).
// Load policy (measured: profiles/lamb/): non-temporal loads of g (dead
// after this pass), cached loads of p, m, v (re-read by the update).  GS_LAMB_NT is the
// compile-time switch of the A/B library variants: bit 0 = g, bit 1 = p, m, v.
#ifndef GS_LAMB_NT
#define GS_LAMB_NT 1
#endif
constexpr bool kLambNTG = (GS_LAMB_NT & 1) != 0, kLambNTS = (GS_LAMB_NT & 2) != 0;
struct LambMomArgs {
  LambHyper h;
  const int32_t* adapt;  // [n]
  const float* gscale;
  const float* found_inf;
  const float* hyper;  // [lr, bc1, bc2s] in device memory (gs_plan_set_hyper_source) or NULL
};

#ifndef GS_G_LAMB_MOMENTS
#define GS_G_LAMB_MOMENTS 4
#endif
constexpr int kLambG = GS_G_LAMB_MOMENTS;

// the lane's 4 elements: the new moments in place and the lane's Σp², Σu² (`valid`
// elements are the tensor's; the rest were loaded as zeros and add nothing: with eps = 0
// their u would be 0/0)
__device__ __forceinline__ void lamb_lane(const LambHyper& h, bool has_m, float mul, float wd_t, int valid,
                                          const float (&x)[4], const float (&g)[4], float (&m)[4], float (&v)[4],
                                          float& sp, float& su) {
  float u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float gi = g[i];
    if (has_m) gi = gi * mul;
    lamb_moments(h, gi, &m[i], &v[i]);
    const float ui = lamb_update(h, x[i], m[i], v[i], wd_t);
    u[i] = i < valid ? ui : 0.f;
  }
  sp = lars_sq4(x);
  su = lars_sq4(u);
}

// the lane's 4 + 4 + 4 + 4 elements of full chunk c of tensor t (uniform descriptor loads)
template <int GD, bool NTG, bool NTS>
__device__ __forceinline__ void lamb_full_load(const PlanArgs& P, int t, int64_t c, float (&x)[4], float (&g)[4],
                                               float (&m)[4], float (&v)[4]) {
  const int64_t n1 = P.n;
  const void* pp = cload(P.ptrs, t);
  const void* gp = cload(P.ptrs, n1 + t);
  const void* mp = cload(P.ptrs, 2 * n1 + t);
  const void* vp = cload(P.ptrs, 3 * n1 + t);
  const int64_t e0 = c * kChunkElems - cload(P.voff, t);
  const uint32_t lo = threadIdx.x * kUnit;
  if ((cload(P.align, t) & 15u) == 15u) {
    load4F<GS_F32, NTS>(elem_at<GS_F32>(pp, e0), lo, x);
    load4F<GD, NTG>(elem_at<GD>(gp, e0), lo, g);
    load4F<GS_F32, NTS>(elem_at<GS_F32>(mp, e0), lo, m);
    load4F<GS_F32, NTS>(elem_at<GS_F32>(vp, e0), lo, v);
  } else {
    const int64_t n = cload(P.numel, t);
    loadN<GS_F32, 4, NTS>(pp, e0 + lo, n, false, x);
    loadN<GD, 4, NTG>(gp, e0 + lo, n, false, g);
    loadN<GS_F32, 4, NTS>(mp, e0 + lo, n, false, m);
    loadN<GS_F32, 4, NTS>(vp, e0 + lo, n, false, v);
  }
}
__device__ __forceinline__ void lamb_full_store(const PlanArgs& P, int t, int64_t c, const float (&m)[4],
                                                const float (&v)[4]) {
  const int64_t n1 = P.n;
  void* mp = cload(P.ptrs, 2 * n1 + t);
  void* vp = cload(P.ptrs, 3 * n1 + t);
  const int64_t e0 = c * kChunkElems - cload(P.voff, t);
  const uint32_t lo = threadIdx.x * kUnit;
  if ((cload(P.align, t) & 15u) == 15u) {
    store4F<GS_F32>(const_cast<void*>(elem_at<GS_F32>(mp, e0)), lo, m);
    store4F<GS_F32>(const_cast<void*>(elem_at<GS_F32>(vp, e0)), lo, v);
  } else {
    const int64_t n = cload(P.numel, t);
    storeN<GS_F32, 4>(mp, e0 + lo, n, false, m);
    storeN<GS_F32, 4>(vp, e0 + lo, n, false, v);
  }
}

// a mixed chunk (tensor tails, runs of small tensors, any span): lars_mixed with the
// moments' read-modify-write; loadN / storeN mask the tensor's tail and take the scalar
// path on an unaligned stream
template <int GD, bool NTG, bool NTS>
__device__ __forceinline__ void lamb_mixed(const PlanArgs& P, const LarsMap& M, const LambMomArgs& A,
                                           const LambHyper& h, bool has_m, float mul, int t0, int span, int64_t c,
                                           float* s_p, float* s_u) {
  const int64_t cs = c * kChunkElems;
  const int64_t e = cs + static_cast<int>(threadIdx.x) * kUnit;
  int lo = t0, hi = t0 + span - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (P.voff[mid] <= e) lo = mid; else hi = mid - 1;
  }
  float sp = 0.f, su = 0.f;
  const int64_t local = e - P.voff[lo];
  const int64_t n = P.numel[lo];
  if (local >= 0 && local < n) {  // else: an alignment gap between tensors
    const uint32_t a = P.align[lo];
    const int64_t n1 = P.n;
    void* mp = P.ptrs[2 * n1 + lo];
    void* vp = P.ptrs[3 * n1 + lo];
    float x[4], g[4], m[4], v[4];
    loadN<GS_F32, 4, NTS>(P.ptrs[lo], local, n, (a & 1u) != 0, x);
    loadN<GD, 4, NTG>(P.ptrs[n1 + lo], local, n, (a & 2u) != 0, g);
    loadN<GS_F32, 4, NTS>(mp, local, n, (a & 4u) != 0, m);
    loadN<GS_F32, 4, NTS>(vp, local, n, (a & 8u) != 0, v);
    const int valid = static_cast<int>(std::min<int64_t>(4, n - local));
    lamb_lane(h, has_m, mul, A.adapt[lo] != 0 ? h.wd : 0.f, valid, x, g, m, v, sp, su);
    storeN<GS_F32, 4>(mp, local, n, (a & 4u) != 0, m);
    storeN<GS_F32, 4>(vp, local, n, (a & 8u) != 0, v);
  }
  __syncthreads();  // the previous mixed chunk's readers are done with the stage
  s_p[threadIdx.x] = sp;
  s_u[threadIdx.x] = su;
  __syncthreads();
  const int slot0 = M.cb[c];
  for (int i = static_cast<int>(threadIdx.x); i < span; i += kBlock) {
    const int t = t0 + i;
    const int64_t b = P.voff[t] - cs, end = b + P.numel[t];  // the tensor's range, relative to the chunk
    const int l0 = b <= 0 ? 0 : static_cast<int>(std::min<int64_t>(kBlock, b / kUnit));
    const int l1 = end <= 0 ? 0 : static_cast<int>(std::min<int64_t>(kBlock, (end + kUnit - 1) / kUnit));
    float ap = 0.f, au = 0.f;
    for (int l = l0; l < l1; ++l) {
      ap = ap + s_p[l];
      au = au + s_u[l];
    }
    M.part[2 * static_cast<int64_t>(slot0 + i)] = ap;
    M.part[2 * static_cast<int64_t>(slot0 + i) + 1] = au;
  }
}

template <int GD, bool NTG, bool NTS>
__global__ void __launch_bounds__(kBlock) GS_SGPR_ATTR lamb_moments_kernel(PlanArgs P, LarsMap M, LambMomArgs A) {
  constexpr int G = kLambG;
  __shared__ float s_p[kBlock], s_u[kBlock], s_red[2 * G * (kBlock / 64)];
  if (A.found_inf != nullptr && *A.found_inf != 0.f) return;  // uniform across the grid: nothing is written
  LambHyper h = A.h;
  if (A.hyper) {
    h.bc1 = A.hyper[1];
    h.bc2s = A.hyper[2];
  }
  const bool has_m = A.gscale != nullptr;
  const float mul = has_m ? *A.gscale : 1.f;
  const int* cw = &P.chunks[0].t0;  // [t0, code] pairs
  const int64_t n_groups = (static_cast<int64_t>(P.n_chunks) + G - 1) / G;
  for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int64_t c0 = G * g;
    int t[G], code[G];
    bool all_full = true;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const bool in = c0 + j < P.n_chunks;
      t[j] = in ? cload(cw, 2 * (c0 + j)) : -1;
      code[j] = in ? cload(cw, 2 * (c0 + j) + 1) : -1;
      all_full = all_full && code[j] == 0;
    }
    if (all_full) {
      // all 4 * G loads of a lane in flight, then per chunk: moments, stores, the two sums
      float x[G][4], y[G][4], m[G][4], v[G][4], r[2 * G];
#pragma unroll
      for (int j = 0; j < G; ++j) lamb_full_load<GD, NTG, NTS>(P, t[j], c0 + j, x[j], y[j], m[j], v[j]);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const float wd_t = cload(A.adapt, t[j]) != 0 ? h.wd : 0.f;
        lamb_lane(h, has_m, mul, wd_t, 4, x[j], y[j], m[j], v[j], r[2 * j], r[2 * j + 1]);
        lamb_full_store(P, t[j], c0 + j, m[j], v[j]);
      }
      lars_block_sum<2 * G>(r, s_red);
      if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
          const int64_t s = cload(M.cb, c0 + j);
          M.part[2 * s] = r[2 * j];
          M.part[2 * s + 1] = r[2 * j + 1];
        }
      }
      continue;
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int64_t c = c0 + j;
      if (code[j] == 0) {
        float x[4], y[4], m[4], v[4], r[2];
        lamb_full_load<GD, NTG, NTS>(P, t[j], c, x, y, m, v);
        lamb_lane(h, has_m, mul, cload(A.adapt, t[j]) != 0 ? h.wd : 0.f, 4, x, y, m, v, r[0], r[1]);
        lamb_full_store(P, t[j], c, m, v);
        lars_block_sum<2>(r, s_red);
        if (threadIdx.x == 0) {
          const int64_t s = cload(M.cb, c);
          M.part[2 * s] = r[0];
          M.part[2 * s + 1] = r[1];
        }
      } else if (code[j] > 0) {
        lamb_mixed<GD, NTG, NTS>(P, M, A, h, has_m, mul, t[j], code[j], c, s_p, s_u);
      }
    }
  }
}

int hip_lamb_moments(gs_plan* p, int gdt, const LambHyper& h, float* norms, const float* gsc, const float* fi,
                     void* stream) {
  DeviceGuard g(p->device);
  if (p->n == 0) return GS_OK;
  GS_TRY_RET(lars_prepare(p, stream));  // A.adapt below points into the scratch
  const LambMomArgs A{h, reinterpret_cast<const int32_t*>(lars_adapt_ptr(p)), gsc, fi, p->hyper};
  return lars_segmented(p, norms, stream, GS_OP_LAMB_MOMENTS, kLambG,
                        [&](int grid, hipStream_t s, hipEvent_t ev0, const PlanArgs& a, const LarsMap& m) -> int {
    GS_DISPATCH_FLOAT(gdt, GD, {
      if (ev0)
        hipExtLaunchKernelGGL((lamb_moments_kernel<GD, kLambNTG, kLambNTS>), dim3(grid), dim3(kBlock), 0, s, ev0,
                              nullptr, 0, a, m, A);
      else
        hipLaunchKernelGGL((lamb_moments_kernel<GD, kLambNTG, kLambNTS>), dim3(grid), dim3(kBlock), 0, s, a, m, A);
    });
    return GS_OK;
  });
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
