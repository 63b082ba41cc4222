// Muon's device kernels (include/gsync.h, gs_muon_*): the only contractions of libgsync,
// so the only MFMA code.  A plan holds a ragged list of matrices; every stage is one
// grouped launch whose workgroups read a task table of (tensor, tile) pairs, heaviest K
// first, so the long tiles start first and the short ones fill the tail.
//
//   muon_xwrite   prep's second half: u from (g, buf'), X0 = bf16(u*s), transposed through
//                 an LDS tile where A > B
//   muon_syrk     C = bf16(alpha * X·Xᵀ [+ beta * D]) on the tiles on or above the
//                 diagonal, the mirror tile written from the same accumulators: the Gram
//                 stage (X, K = np) and the polynomial stage (X = D = Agram, K = mp)
//   muon_apply    X' = bf16(fma(a, X, Bpoly·X)): Bpoly K-contiguous, X K-strided and
//                 transposed on its way into LDS
//   muon_update   p = p*decay - adj_lr*O, O read back through the LDS transpose
//
// GEMM tiling (both kernels): a 256-thread workgroup owns a 128 x 128 output tile, wave w
// the 64 x 64 quadrant (w / 2, w % 2) as 2 x 2 blocks of v_mfma_f32_32x32x16_bf16 — 64
// accumulator registers per lane.  K advances in slabs of 32: both operand slabs
// (128 x 32 bf16 each) are staged in LDS as [row][k] with the row pitch padded from 64 to
// 80 bytes (16-B fragment reads of 32 consecutive rows then spread over all banks), double
// buffered: the global loads of slab s + 1 are issued before the MFMAs of slab s and stored
// to the other buffer after them, one barrier per slab.  The workspace is padded to the
// tile in both dimensions (gs_muon_layout), so no load or store is predicated.
//
// An MFMA lane holds, for operand A, row (lane % 32) and the 8 consecutive k of group
// (lane / 32); for B the same of its column; of the 32 x 32 result, column (lane % 32)
// and rows 8 * (v / 4) + 4 * (lane / 32) + v % 4, v = 0..15.

#include "gs_seg.h"

namespace gs {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kT = kMuonTile;   // 128
constexpr int kBK = 32;         // K slab
constexpr int kPitch = 40;      // LDS row pitch in bf16 (80 B)
constexpr int kSlab = kT * kPitch;  // one operand slab in LDS (bf16 elements)

__device__ __forceinline__ gu4 ldg16(const uint16_t* p) { return *gptr<gu4>(p); }

// this wave's 2 x 2 MFMA blocks over one K slab
__device__ __forceinline__ void mma_slab(const uint16_t* sA, const uint16_t* sB, int wr, int wc, int lane,
                                         f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int kk = 0; kk < kBK; kk += 16) {
    const int ko = kk + 8 * (lane >> 5);
    bf16x8 a[2], b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const gu4 ra = *reinterpret_cast<const gu4*>(sA + (wr * 64 + i * 32 + (lane & 31)) * kPitch + ko);
      const gu4 rb = *reinterpret_cast<const gu4*>(sB + (wc * 64 + i * 32 + (lane & 31)) * kPitch + ko);
      a[i] = __builtin_bit_cast(bf16x8, ra);
      b[i] = __builtin_bit_cast(bf16x8, rb);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
  }
}

// a K-contiguous operand slab: rows [row0, row0 + 128) x k [k0, k0 + 32) of M (pitch ld);
// thread -> (row = tid / 2, 16 k of half tid % 2): two 16-B loads, two 16-B LDS stores
struct RowSlab {
  gu4 v[2];
  __device__ __forceinline__ void load(const uint16_t* M, int64_t ld, int row0, int k0) {
    const uint16_t* src = M + static_cast<int64_t>(row0 + (threadIdx.x >> 1)) * ld + k0 + (threadIdx.x & 1) * 16;
    v[0] = ldg16(src);
    v[1] = ldg16(src + 8);
  }
  __device__ __forceinline__ void store(uint16_t* s) const {
    uint16_t* dst = s + (threadIdx.x >> 1) * kPitch + (threadIdx.x & 1) * 16;
    *reinterpret_cast<gu4*>(dst) = v[0];
    *reinterpret_cast<gu4*>(dst + 8) = v[1];
  }
};

// a K-strided operand slab: k rows [k0, k0 + 32) x columns [col0, col0 + 128) of M, stored
// to LDS as [column][k].  thread -> (k pair tid / 16, 8 columns of segment tid % 16): two
// 16-B loads (rows k, k + 1), then 8 4-B LDS stores of the (k, k + 1) pair of a column
struct ColSlab {
  gu4 v[2];
  __device__ __forceinline__ void load(const uint16_t* M, int64_t ld, int k0, int col0) {
    const uint16_t* src = M + static_cast<int64_t>(k0 + 2 * (threadIdx.x >> 4)) * ld + col0 + (threadIdx.x & 15) * 8;
    v[0] = ldg16(src);
    v[1] = ldg16(src + ld);
  }
  __device__ __forceinline__ void store(uint16_t* s) const {
    uint32_t* dst = reinterpret_cast<uint32_t*>(s) + ((threadIdx.x & 15) * 8) * (kPitch / 2) + (threadIdx.x >> 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t lo = (v[0][e >> 1] >> ((e & 1) * 16)) & 0xffffu;
      const uint32_t hi = (v[1][e >> 1] >> ((e & 1) * 16)) & 0xffffu;
      dst[e * (kPitch / 2)] = lo | (hi << 16);
    }
  }
};

// The K loop shared by both GEMM kernels: LA / LB load the slab of step k0 (functors),
// double buffered through s_a / s_b.
template <class SA, class SB, class FA, class FB>
__device__ __forceinline__ void gemm_loop(int K, uint16_t* s_a, uint16_t* s_b, FA&& la, FB&& lb, int wr, int wc,
                                          int lane, f32x16 (&acc)[2][2]) {
  SA ra;
  SB rb;
  la(ra, 0);
  lb(rb, 0);
  ra.store(s_a);
  rb.store(s_b);
  __syncthreads();
  const int n_slab = K / kBK;
  for (int s = 0; s < n_slab; ++s) {
    const int cur = s & 1;
    const bool more = s + 1 < n_slab;
    if (more) {
      la(ra, (s + 1) * kBK);
      lb(rb, (s + 1) * kBK);
    }
    mma_slab(s_a + cur * kSlab, s_b + cur * kSlab, wr, wc, lane, acc);
    if (more) {
      ra.store(s_a + (cur ^ 1) * kSlab);
      rb.store(s_b + (cur ^ 1) * kSlab);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;
}

// row / column inside the workgroup tile of accumulator element v of block (i, j)
__device__ __forceinline__ int acc_row(int wr, int i, int lane, int v) {
  return wr * 64 + i * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
}
__device__ __forceinline__ int acc_col(int wc, int j, int lane) { return wc * 64 + j * 32 + (lane & 31); }

template <bool POLY>
__global__ void __launch_bounds__(kBlock) muon_syrk_kernel(MuonTables T, uint16_t* ws, int xsel, float alpha,
                                                           float beta) {
  __shared__ __attribute__((aligned(16))) uint16_t s_a[2 * kSlab], s_b[2 * kSlab];
  const MuonTask task = (POLY ? T.poly : T.gram)[blockIdx.x];
  const MuonDesc d = T.desc[task.t];
  const uint16_t* X = ws + (POLY ? d.a : (xsel ? d.x[1] : d.x[0]));
  const int64_t ld = POLY ? d.mp : d.np;
  uint16_t* C = ws + (POLY ? d.b : d.a);
  const int row0 = task.ti * kT, col0 = task.tj * kT;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
  f32x16 acc[2][2];
  zero_acc(acc);
  gemm_loop<RowSlab, RowSlab>(
      static_cast<int>(ld), s_a, s_b, [&](RowSlab& r, int k0) { r.load(X, ld, row0, k0); },
      [&](RowSlab& r, int k0) { r.load(X, ld, col0, k0); }, wr, wc, lane, acc);
  const int64_t ldc = d.mp;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t r = row0 + acc_row(wr, i, lane, v), c = col0 + acc_col(wc, j, lane);
        float o;
        if constexpr (POLY) o = muon_poly_out(beta, alpha, acc[i][j][v], bf16_to_f32(X[r * ld + c]));
        else o = muon_gram_out(alpha, acc[i][j][v]);
        const uint16_t h = f32_to_bf16(o);
        C[r * ldc + c] = h;
        if (task.ti != task.tj) C[c * ldc + r] = h;
      }
}

__global__ void __launch_bounds__(kBlock) muon_apply_kernel(MuonTables T, uint16_t* ws, int xsel, float a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_a[2 * kSlab], s_b[2 * kSlab];
  const MuonTask task = T.apply[blockIdx.x];
  const MuonDesc d = T.desc[task.t];
  const uint16_t* P = ws + d.b;
  const uint16_t* X = ws + (xsel ? d.x[1] : d.x[0]);
  uint16_t* Y = ws + (xsel ? d.x[0] : d.x[1]);
  const int64_t ldp = d.mp, ldx = d.np;
  const int row0 = task.ti * kT, col0 = task.tj * kT;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
  f32x16 acc[2][2];
  zero_acc(acc);
  gemm_loop<RowSlab, ColSlab>(
      d.mp, s_a, s_b, [&](RowSlab& r, int k0) { r.load(P, ldp, row0, k0); },
      [&](ColSlab& r, int k0) { r.load(X, ldx, k0, col0); }, wr, wc, lane, acc);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t e = static_cast<int64_t>(row0 + acc_row(wr, i, lane, v)) * ldx + col0 + acc_col(wc, j, lane);
        Y[e] = f32_to_bf16(muon_apply_out(a, acc[i][j][v], bf16_to_f32(X[e])));
      }
}

// ---- the element-wise passes: a workgroup takes a 64 x 64 tile of the [A, B] matrix,
// thread -> column tid % 64, rows tid / 64 + 4 * it.  Where the tensor is stored
// transposed (A > B) the tile crosses an LDS stage, so both the fp32 side and the bf16
// side move along their contiguous dimension.
constexpr int kE = kMuonEw;

template <int GD>
__global__ void __launch_bounds__(kBlock) muon_xwrite_kernel(PlanArgs P, MuonTables T, MuonHyper h, const float* norms,
                                                             uint16_t* ws) {
  __shared__ uint16_t s_t[kE][kE + 2];
  const MuonTask task = T.ew[blockIdx.x];
  const MuonDesc d = T.desc[task.t];
  const void* g = slot_ptr(P, 1, task.t);
  const float* buf = static_cast<const float*>(slot_ptr(P, 2, task.t));
  const float s = muon_scale(norms[2 * task.t + 1], h.eps);
  uint16_t* X = ws + d.x[0];
  const int cl = threadIdx.x & 63, rl0 = threadIdx.x >> 6;
  const int r0 = task.ti * kE, c0 = task.tj * kE;
#pragma unroll 4
  for (int it = 0; it < kE / 4; ++it) {
    const int rl = rl0 + 4 * it, r = r0 + rl, c = c0 + cl;
    uint16_t x = 0;
    if (r < d.A && c < d.B) {
      const int64_t e = static_cast<int64_t>(r) * d.B + c;
      float gv;
      if constexpr (GD == GS_F32) gv = static_cast<const float*>(g)[e];
      else gv = to_f32<GD>(static_cast<const uint16_t*>(g)[e]);
      x = f32_to_bf16(muon_u(h, gv, buf[e]) * s);
      if (!d.tr) X[static_cast<int64_t>(r) * d.np + c] = x;
    }
    if (d.tr) s_t[rl][cl] = x;
  }
  if (!d.tr) return;  // uniform over the workgroup
  __syncthreads();
#pragma unroll 4
  for (int it = 0; it < kE / 4; ++it) {
    // X is [B, A]: row = the tile's column c0 + (tid / 64 + 4 it), column = its row r0 + tid % 64
    const int xr = c0 + rl0 + 4 * it, xc = r0 + cl;
    if (xr < d.B && xc < d.A) X[static_cast<int64_t>(xr) * d.np + xc] = s_t[cl][rl0 + 4 * it];
  }
}

__global__ void __launch_bounds__(kBlock) muon_update_kernel(PlanArgs P, MuonTables T, const uint16_t* ws, int xsel,
                                                             double lr, float decay, int adjust) {
  __shared__ uint16_t s_t[kE][kE + 2];
  const MuonTask task = T.ew[blockIdx.x];
  const MuonDesc d = T.desc[task.t];
  float* p = static_cast<float*>(slot_ptr(P, 0, task.t));
  const float adj = static_cast<float>(lr * (adjust ? d.ratio[1] : d.ratio[0]));
  const uint16_t* X = ws + (xsel ? d.x[1] : d.x[0]);
  const int cl = threadIdx.x & 63, rl0 = threadIdx.x >> 6;
  const int r0 = task.ti * kE, c0 = task.tj * kE;
  if (d.tr) {
#pragma unroll 4
    for (int it = 0; it < kE / 4; ++it) {
      const int xr = c0 + rl0 + 4 * it, xc = r0 + cl;
      s_t[rl0 + 4 * it][cl] = (xr < d.B && xc < d.A) ? X[static_cast<int64_t>(xr) * d.np + xc] : uint16_t(0);
    }
    __syncthreads();
  }
#pragma unroll 4
  for (int it = 0; it < kE / 4; ++it) {
    const int rl = rl0 + 4 * it, r = r0 + rl, c = c0 + cl;
    if (r < d.A && c < d.B) {
      const uint16_t o = d.tr ? s_t[cl][rl] : X[static_cast<int64_t>(r) * d.np + c];
      const int64_t e = static_cast<int64_t>(r) * d.B + c;
      p[e] = muon_param(p[e], decay, adj, bf16_to_f32(o));
    }
  }
}

// gs_muon_prep's first half: the segmented pass (gs_seg.h) over (p, g, buf) that advances
// the momentum buffer in place and publishes Σbuf'², Σu² of the update direction u per
// tensor.  p is a stream of the policy only because the slots are numbered from 0: its
// registers are never read, so its loads are dropped by the compiler.  g and buf take
// cached loads: the X pass re-reads both right behind.
template <int GD_>
struct MuonLanes {
  static constexpr int G = 4, S = 3, W = 2, GD = GD_;
  static constexpr bool NTG = false, NTS = false;
  MuonHyper h;
  __device__ __forceinline__ bool begin() { return true; }
  template <bool U>
  __device__ __forceinline__ void lane(int, int valid, float (&r)[S][4], float& sb, float& su) const {
    float u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      r[2][i] = muon_buf(h, r[1][i], r[2][i]);
      const float ui = muon_u(h, r[1][i], r[2][i]);
      u[i] = i < valid ? ui : 0.f;
    }
    sb = lars_sq4(r[2]);
    su = lars_sq4(u);
  }
};

// One grouped launch through the plan's stream bookkeeping: pointer-table flush, the
// launch timer's event pair (one record of `kind`), the last-stream mark.
template <class K, class... Args>
int muon_launch(gs_plan* p, int kind, int grid, void* stream, K kernel, Args... args) {
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

// desc | gram | poly | apply | ew in one allocation, each part 256-B aligned
int hip_muon_upload(gs_plan* p, const MuonTaskLists& l) {
  DeviceGuard g(p->device);
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t o_gram = al(sizeof(MuonDesc) * p->muon.size());
  const size_t o_poly = o_gram + al(sizeof(MuonTask) * l.gram.size());
  const size_t o_apply = o_poly + al(sizeof(MuonTask) * l.poly.size());
  const size_t o_ew = o_apply + al(sizeof(MuonTask) * l.apply.size());
  const size_t total = o_ew + al(sizeof(MuonTask) * l.ew.size());
  if (p->d_muon) {
    HIP_RET(hipDeviceSynchronize());  // a launch in flight may still read the old tables
    HIP_RET(hipFree(p->d_muon));
    p->d_muon = nullptr;
  }
  p->muon_tab = MuonTables{};
  if (p->muon.empty()) return GS_OK;
  char* dmem = nullptr;
  HIP_RET(hipMalloc(reinterpret_cast<void**>(&dmem), std::max<size_t>(total, 256)));
  p->d_muon = dmem;
  HIP_RET(hipMemcpy(dmem, p->muon.data(), sizeof(MuonDesc) * p->muon.size(), hipMemcpyHostToDevice));
  const std::vector<MuonTask>* lists[4] = {&l.gram, &l.poly, &l.apply, &l.ew};
  const size_t offs[4] = {o_gram, o_poly, o_apply, o_ew};
  for (int i = 0; i < 4; ++i)
    if (!lists[i]->empty())
      HIP_RET(hipMemcpy(dmem + offs[i], lists[i]->data(), sizeof(MuonTask) * lists[i]->size(), hipMemcpyHostToDevice));
  p->muon_tab = MuonTables{reinterpret_cast<const MuonDesc*>(dmem),
                           reinterpret_cast<const MuonTask*>(dmem + o_gram),
                           reinterpret_cast<const MuonTask*>(dmem + o_poly),
                           reinterpret_cast<const MuonTask*>(dmem + o_apply),
                           reinterpret_cast<const MuonTask*>(dmem + o_ew),
                           static_cast<int32_t>(l.gram.size()),
                           static_cast<int32_t>(l.apply.size()),
                           static_cast<int32_t>(l.ew.size())};
  return GS_OK;
}

int hip_muon_moments(gs_plan* p, int gdt, const MuonHyper& h, float* norms, void* stream) {
  DeviceGuard g(p->device);
  GS_DISPATCH_FLOAT(gdt, GD, return lars_segmented(p, norms, stream, GS_OP_MUON_PREP, MuonLanes<GD>{h}));
  return GS_OK;
}

int hip_muon_xwrite(gs_plan* p, int gdt, const MuonHyper& h, const float* norms, void* ws, void* stream) {
  DeviceGuard g(p->device);
  const MuonTables& T = p->muon_tab;
  GS_DISPATCH_FLOAT(gdt, GD, return muon_launch(p, GS_OP_MUON_PREP, T.n_ew, stream, muon_xwrite_kernel<GD>, p->args(), T,
                                                h, norms, static_cast<uint16_t*>(ws)));
  return GS_OK;
}

int hip_muon_syrk(gs_plan* p, void* ws, int poly, int xsel, float alpha, float beta, void* stream) {
  DeviceGuard g(p->device);
  const MuonTables& T = p->muon_tab;
  if (poly)
    return muon_launch(p, GS_OP_MUON_POLY, T.n_sym, stream, muon_syrk_kernel<true>, T, static_cast<uint16_t*>(ws), xsel,
                       alpha, beta);
  return muon_launch(p, GS_OP_MUON_GRAM, T.n_sym, stream, muon_syrk_kernel<false>, T, static_cast<uint16_t*>(ws), xsel,
                     alpha, beta);
}

int hip_muon_apply(gs_plan* p, void* ws, int xsel, float a, void* stream) {
  DeviceGuard g(p->device);
  const MuonTables& T = p->muon_tab;
  return muon_launch(p, GS_OP_MUON_APPLY, T.n_apply, stream, muon_apply_kernel, T, static_cast<uint16_t*>(ws), xsel, a);
}

int hip_muon_update(gs_plan* p, void* ws, int xsel, double lr, double wd, int adjust, void* stream) {
  DeviceGuard g(p->device);
  const MuonTables& T = p->muon_tab;
  return muon_launch(p, GS_OP_MUON_UPDATE, T.n_ew, stream, muon_update_kernel, p->args(), T,
                     static_cast<const uint16_t*>(ws), xsel, lr, static_cast<float>(1.0 - lr * wd), adjust);
}

}  // namespace gs
