// gfx950 (CDNA4) fused SGD / Adam(W) / LARS updates of libgsync (gs_sgd_step / gs_adam_step /
// gs_lars_step[_lowp]): the chunk-map engine of gs_engine.h with SgdOp / AdamOp / LarsOp, the
// grad-load policy per launch; the segmented per-tensor-sum pass over the same chunk map
// (seg_sum_kernel), one skeleton with two lane policies: LarsLanes, LARS's Σp², Σg²
// (gs_lars_norms), and LambLanes, LAMB's Σp², Σu² fused with the moments' read-modify-write
// (gs_lamb_moments); LambOp on the engine (gs_lamb_step); and the EMA / SWA weight average
// (gs_ema_step / gs_ema_hyper): EmaOp on the engine.

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

// ------------------------------------------------- segmented per-tensor sums
// Two sums per tensor (LARS: Σp², Σg²; LAMB: Σp², Σu²): a segmented reduction on the chunk
// map.  The host numbers one partial slot per (chunk, tensor intersecting it) pair, in
// chunk order then tensor order — a full chunk has one, a mixed chunk of span k has k —
// so a tensor's slots are the contiguous range [first, first + count).  Every slot
// is written by exactly one workgroup, with a sum whose order the chunk alone fixes:
//   full chunk   each lane squares its 4 + 4 values in element order, then the
//                fixed DPP tree per wave and the 4 wave sums in wave order;
//   mixed chunk  each lane leaves its two sums in LDS; lanes of one tensor are
//                contiguous, and thread i adds up tensor t0 + i's lane range in
//                lane order (any span: threads stride over it, nothing is staged
//                per tensor, so spans above kMixedStage take the same path).
// lars_norm_finish then folds each tensor's slots with one workgroup: thread j adds slots
// j, j + 256, ... in order, then the same fixed tree.  Nothing depends on the grid or on
// arrival order and there are no floating-point atomics: replicas holding the same
// inputs publish the same bits.
// The walk, the order and the slot writes are seg_sum_kernel's, written once.  A lane
// policy L says what a lane does with its 4 elements:
//   S, GD, NTG, NTS  its streams: the plan's slots 0..S-1, fp32 but for the grads (slot 1,
//                    dtype GD); non-temporal loads of the grads / of the others.  A chunk
//                    takes the 16-B accesses when the align bits of all S streams are set
//   W                streams W..S-1 are stored back (non-temporal, as every store of the engine)
//   G                chunks per workgroup iteration (sizes s_red)
//   begin()          at kernel entry, uniform over the grid: false = nothing to do
//   lane<U>(t, valid, r, a, b)  the lane's two sums from its registers r[S][4], of which
//                    `valid` elements are the tensor's (the rest were loaded as zeros); may
//                    rewrite r.  U: t is wave-uniform (a full chunk), per-tensor values are
//                    then scalar loads (cload)
struct LarsMap {
  const int32_t* cb;  // [n_chunks]: first partial slot of each chunk
  const int32_t* tb;  // [2n]: first slot, slot count of each tensor
  float* part;        // [2 * slots]: the two sums per slot
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

// The lane's 4 elements of streams K..S-1 of policy L (loads) or W..S-1 (stores): F = the
// full chunk's 16-B accesses at e0 + lo, else loadN / storeN with bit k of `vec` = stream
// k's base is 16-B aligned.  K is a template index: non-temporal is a property of the load
// instruction, and two arms under a run-time k are merged into one cached load.
template <class L, bool F, int K = 0>
__device__ __forceinline__ void seg_load(void* const (&ptr)[L::S], int64_t e0, uint32_t lo, int64_t n, uint32_t vec,
                                         float (&r)[L::S][4]) {
  if constexpr (K < L::S) {
    ld<K == 1 ? L::GD : GS_F32, 4, F, K == 1 ? L::NTG : L::NTS>(ptr[K], e0, lo, n, ((vec >> K) & 1u) != 0, r[K]);
    seg_load<L, F, K + 1>(ptr, e0, lo, n, vec, r);
  }
}
template <class L, bool F, int K = L::W>
__device__ __forceinline__ void seg_store(void* const (&ptr)[L::S], int64_t e0, uint32_t lo, int64_t n, uint32_t vec,
                                          const float (&r)[L::S][4]) {
  if constexpr (K < L::S) {
    st<GS_F32, 4, F>(ptr[K], e0, lo, n, ((vec >> K) & 1u) != 0, r[K]);
    seg_store<L, F, K + 1>(ptr, e0, lo, n, vec, r);
  }
}

template <int S>
struct SegChunk {  // full chunk c of tensor t, S streams (uniform descriptor loads: SGPRs)
  void* ptr[S];
  int64_t e0, n;  // the chunk's first element inside the tensor; numel (read only when !vec)
  bool vec;       // the align bits of all S streams are set
};
template <int S>
__device__ __forceinline__ SegChunk<S> seg_chunk(const PlanArgs& P, int t, int64_t c) {
  constexpr uint32_t kAll = (1u << S) - 1;
  SegChunk<S> d;
#pragma unroll
  for (int k = 0; k < S; ++k) d.ptr[k] = cload(P.ptrs, k * static_cast<int64_t>(P.n) + t);
  d.e0 = c * kChunkElems - cload(P.voff, t);
  d.vec = (cload(P.align, t) & kAll) == kAll;
  d.n = d.vec ? 0 : cload(P.numel, t);
  return d;
}

// K full chunks c0, c0 + 1, ... of tensors t[0..K): all S * K loads of a lane in flight,
// then per chunk the lane's work and stores, then one barrier pair for the 2 * K sums and
// the K slot writes
template <class L, int K>
__device__ __forceinline__ void seg_full(const PlanArgs& P, const LarsMap& M, const L& lanes, const int* t,
                                         int64_t c0, float* s_red) {
  constexpr int S = L::S;
  const uint32_t lo = threadIdx.x * kUnit;
  float r[K][S][4], v[2 * K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const SegChunk<S> d = seg_chunk<S>(P, t[j], c0 + j);
    if (d.vec) seg_load<L, true>(d.ptr, d.e0, lo, 0, 0, r[j]);
    else seg_load<L, false>(d.ptr, d.e0, lo, d.n, 0, r[j]);
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    lanes.template lane<true>(t[j], 4, r[j], v[2 * j], v[2 * j + 1]);
    if constexpr (L::W < S) {
      const SegChunk<S> d = seg_chunk<S>(P, t[j], c0 + j);
      if (d.vec) seg_store<L, true>(d.ptr, d.e0, lo, 0, 0, r[j]);
      else seg_store<L, false>(d.ptr, d.e0, lo, d.n, 0, r[j]);
    }
  }
  lars_block_sum<2 * K>(v, s_red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int64_t s = cload(M.cb, c0 + j);
      M.part[2 * s] = v[2 * j];
      M.part[2 * s + 1] = v[2 * j + 1];
    }
  }
}

// a mixed chunk (tensor tails, runs of small tensors, any span): per-lane descriptor
// loads; loadN / storeN mask the tensor's tail and take the scalar path on an unaligned
// stream
template <class L>
__device__ __forceinline__ void seg_mixed(const PlanArgs& P, const LarsMap& M, const L& lanes, int t0, int span,
                                          int64_t c, float* s_a, float* s_b) {
  constexpr int S = L::S;
  const int64_t cs = c * kChunkElems;
  const int64_t e = cs + static_cast<int>(threadIdx.x) * kUnit;
  int lo = t0, hi = t0 + span - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (P.voff[mid] <= e) lo = mid; else hi = mid - 1;
  }
  float sa = 0.f, sb = 0.f;
  const int64_t local = e - P.voff[lo];
  const int64_t n = P.numel[lo];
  if (local >= 0 && local < n) {  // else: an alignment gap between tensors
    const uint32_t a = P.align[lo];
    void* ptr[S];  // all pointers first: a pointer load between two data loads would wait for the first
#pragma unroll
    for (int k = 0; k < S; ++k) ptr[k] = P.ptrs[k * static_cast<int64_t>(P.n) + lo];
    float r[S][4];
    seg_load<L, false>(ptr, local, 0, n, a, r);
    lanes.template lane<false>(lo, static_cast<int>(std::min<int64_t>(4, n - local)), r, sa, sb);
    seg_store<L, false>(ptr, local, 0, n, a, r);
  }
  __syncthreads();  // the previous mixed chunk's readers are done with the stage
  s_a[threadIdx.x] = sa;
  s_b[threadIdx.x] = sb;
  __syncthreads();
  const int slot0 = M.cb[c];
  for (int i = static_cast<int>(threadIdx.x); i < span; i += kBlock) {
    const int t = t0 + i;
    const int64_t b = P.voff[t] - cs, end = b + P.numel[t];  // the tensor's range, relative to the chunk
    const int l0 = b <= 0 ? 0 : static_cast<int>(std::min<int64_t>(kBlock, b / kUnit));
    const int l1 = end <= 0 ? 0 : static_cast<int>(std::min<int64_t>(kBlock, (end + kUnit - 1) / kUnit));
    float ta = 0.f, tb = 0.f;
    for (int l = l0; l < l1; ++l) {
      ta = ta + s_a[l];
      tb = tb + s_b[l];
    }
    M.part[2 * static_cast<int64_t>(slot0 + i)] = ta;
    M.part[2 * static_cast<int64_t>(slot0 + i) + 1] = tb;
  }
}

// a workgroup iteration takes a group of G chunks: G full chunks (of one tensor or
// several: every chunk has its own slot) go through seg_full at once; otherwise chunk by
// chunk, skipping the empty ones (code < 0: inside the plan, or past its end)
template <class L>
__global__ void __launch_bounds__(kBlock) GS_SGPR_ATTR seg_sum_kernel(PlanArgs P, LarsMap M, L lanes) {
  constexpr int G = L::G;
  __shared__ float s_a[kBlock], s_b[kBlock], s_red[2 * G * (kBlock / 64)];
  if (!lanes.begin()) return;  // ahead of every barrier: nothing is written
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
      seg_full<L, G>(P, M, lanes, t, c0, s_red);
      continue;
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if (code[j] == 0) seg_full<L, 1>(P, M, lanes, &t[j], c0 + j, s_red);
      else if (code[j] > 0) seg_mixed(P, M, lanes, t[j], code[j], c0 + j, s_a, s_b);
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

// seg_sum_kernel<L> over the plan's chunks, then lars_norm_finish: the launch timer takes
// the pair as one record of `kind`, the chunk pass's start and the fold's stop.
template <class L>
static int lars_segmented(gs_plan* p, float* norms, void* stream, int kind, const L& lanes) {
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
  const int64_t groups = (static_cast<int64_t>(p->chunks.size()) + L::G - 1) / L::G;
  if (groups > 0) {
    const int grid = static_cast<int>(std::min<int64_t>(groups, p->grid_cap));
    const PlanArgs a = p->args();
    if (ev0)
      hipExtLaunchKernelGGL((seg_sum_kernel<L>), dim3(grid), dim3(kBlock), 0, s, ev0, nullptr, 0, a, m, lanes);
    else
      hipLaunchKernelGGL((seg_sum_kernel<L>), dim3(grid), dim3(kBlock), 0, s, a, m, lanes);
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
