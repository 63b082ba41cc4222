// PowerSGD's device kernels (include/gsync.h, gs_psgd_*): rank-r factorisation of a ragged
// list of fp32 gradient matrices, r <= 8.  With N = r the MFMA tiles would be at most a
// quarter full and the operands must stay fp32, so there is no matrix instruction here:
// every pass is bound by the one sweep it makes over M or E, and the work goes into moving
// each element once, along its contiguous dimension, and into sums whose order the layout
// alone fixes.  Every stage is one grouped launch: blockIdx.x indexes a task table of
// (tensor, row block, column strip) built by gs_psgd_layout, heaviest tasks first.
//
//   psgd_orth         modified Gram-Schmidt of one [rows, r] factor per workgroup, the factor
//                     resident in LDS column-major (<= kPsgdOrthLds floats) or streamed
//   psgd_project      E = M (+ E), P = E·Q: rows over waves, float4 along the row, Q's slab
//                     of kPsgdCols columns transposed into LDS, short rows share a wave
//   psgd_backproject  Q partials = Eᵀ·P of a (row block, 64-column strip): r accumulators a
//                     column in registers, P's rows broadcast from LDS
//   psgd_fold         Q = the row blocks' partials added in block order
//   psgd_reconstruct  Q *= inv_ws (written by the strip's only workgroup), G = P·Qᵀ,
//                     E -= P·Qᵀ over all rows of a 64-column strip
//
// RP is the plan's rank rounded up to 1, 2, 4 or 8: accumulators are RP registers with
// static indices, and a tensor whose r is smaller (clipped by its shape) carries zeros.

#include "gs_seg.h"

namespace gs {

namespace {

// Every sum of products here is accumulated in fp64 — the products of fp32 operands are
// exact there — and rounded to fp32 once, where it is stored: the passes are bound by
// memory, the fp64 adds ride along, and a stored P, Q or G is then one rounding away from
// the exact value whatever the order of the sum (which is still fixed).
//
// the sum over the `sub` lanes that share a row (a power of two): the xor butterfly, both
// partners forming a + b, so every lane of the group ends with the same bits
__device__ __forceinline__ double psgd_group_sum(double v, int sub) {
  for (int o = 1; o < sub; o <<= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// K fp64 sums over the workgroup, left in every thread: the xor butterfly of a wave (both
// partners form a + b, so all lanes agree), then the 4 wave sums in wave order
template <int K>
__device__ __forceinline__ void psgd_block_sum(double (&v)[K], double* s_red) {
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v[k] = v[k] + __shfl_xor(v[k], o, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_red[w * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double r = s_red[k];
#pragma unroll
    for (int i = 1; i < kBlock / 64; ++i) r = r + s_red[i * K + k];
    v[k] = r;
  }
  __syncthreads();
}

// rows [row0, row0 + kPsgdRows) of P into s_p[row][RP], zeros past the tensor's rows and rank
template <int RP, class F>
__device__ __forceinline__ void psgd_stage_p(F* s_p, const float* P, const PsgdDesc& d, int row0) {
  for (int e = threadIdx.x; e < kPsgdRows * RP; e += kBlock) {
    const int lr = e / RP, j = e % RP;
    s_p[e] = (row0 + lr < d.n && j < d.r) ? P[static_cast<int64_t>(row0 + lr) * d.r + j] : 0.f;
  }
}

// ------------------------------------------------------------------ orthogonalize
// torch's _orthogonalize_gram_schmidt on X [rows, r]: c_i /= ‖c_i‖ + eps, then
// c_j -= (c_iᵀc_j) c_i for j > i.  Thread k owns rows k, k + 256, ...; a column step is two
// sweeps: (normalise c_i, the r - i - 1 dot products), then (the r - i - 1 updates, the
// next column's Σx²).  The sums (Σx², Σc_i·c_j) are taken in fp64 — every product exact,
// one rounding to fp32 at the end — because a factor with r = rows is square and can be
// ill-conditioned: the last columns are differences of nearly equal vectors, and an fp32
// dot product's rounding is amplified by the condition number.  RES: X is the LDS copy
// [j][rows] (conflict-free along rows), else the factor itself in global memory [row][r].
template <int RP, bool RES>
__device__ __forceinline__ void psgd_mgs(float* X, int rows, int r, float eps, double* s_red) {
  auto at = [&](int row, int j) -> float& {
    return RES ? X[static_cast<int64_t>(j) * rows + row] : X[static_cast<int64_t>(row) * r + j];
  };
  double nn[1] = {0.0};
  for (int row = threadIdx.x; row < rows; row += kBlock) {
    const double v = at(row, 0);
    nn[0] = nn[0] + v * v;
  }
  psgd_block_sum<1>(nn, s_red);
  for (int i = 0; i < r; ++i) {
    const float nrm = static_cast<float>(sqrt(nn[0])) + eps;
    double dot[RP];
#pragma unroll
    for (int j = 0; j < RP; ++j) dot[j] = 0.0;
    for (int row = threadIdx.x; row < rows; row += kBlock) {
      const float xi = at(row, i) / nrm;
      at(row, i) = xi;
#pragma unroll
      for (int j = 1; j < RP; ++j)
        if (j > i && j < r) dot[j] = dot[j] + static_cast<double>(xi) * static_cast<double>(at(row, j));
    }
    if (i + 1 == r) break;
    psgd_block_sum<RP>(dot, s_red);
    nn[0] = 0.0;
    for (int row = threadIdx.x; row < rows; row += kBlock) {
      const float xi = at(row, i);
#pragma unroll
      for (int j = 1; j < RP; ++j)
        if (j > i && j < r) {
          const float xj = at(row, j) - static_cast<float>(dot[j]) * xi;
          at(row, j) = xj;
          if (j == i + 1) nn[0] = nn[0] + static_cast<double>(xj) * static_cast<double>(xj);
        }
    }
    psgd_block_sum<1>(nn, s_red);
  }
}

template <int RP>
__global__ void __launch_bounds__(kBlock) psgd_orth_kernel(PsgdTables T, float* mem, int which, float eps) {
  extern __shared__ __attribute__((aligned(16))) float s_x[];
  __shared__ double s_red[(kBlock / 64) * RP];
  const PsgdDesc d = T.desc[T.orth[which][blockIdx.x].t];
  const int rows = which ? d.m : d.n, r = d.r;
  float* X = mem + (which ? d.q_off : d.p_off);
  const int total = rows * r;
  if (total > kPsgdOrthLds) {  // uniform over the workgroup
    psgd_mgs<RP, false>(X, rows, r, eps, s_red);
    return;
  }
  for (int e = threadIdx.x; e < total; e += kBlock) s_x[(e % r) * rows + e / r] = X[e];
  __syncthreads();
  psgd_mgs<RP, true>(s_x, rows, r, eps, s_red);
  __syncthreads();
  for (int e = threadIdx.x; e < total; e += kBlock) X[e] = s_x[(e % r) * rows + e / r];
}

// ------------------------------------------------------------------ project
// A workgroup owns d.prb rows.  A row is swept by `sub` lanes, 4 columns a lane: a whole wave
// (4 sweeps of 256 columns per slab) or, for m <= 128, the power of two of lanes that
// covers it, so 64 / sub rows ride in one wave.  Q's slab is staged as s_q[j][column]: a
// lane's 4 columns of one j are one 16-B LDS read, consecutive over the lanes.  A row's r
// sums are folded over its lanes per slab and added into s_p in slab order by the one lane
// group that owns the row.
template <int RP>
__global__ void __launch_bounds__(kBlock) psgd_project_kernel(PlanArgs A, PsgdTables T, float* pmem,
                                                              const float* qmem, int use_error) {
  __shared__ __attribute__((aligned(16))) float s_q[RP * kPsgdCols];
  __shared__ double s_p[kPsgdRows * RP];
  const PsgdTask task = T.proj[blockIdx.x];
  const PsgdDesc d = T.desc[task.t];
  const float* M = static_cast<const float*>(slot_ptr(A, 0, task.t));
  float* E = static_cast<float*>(slot_ptr(A, 1, task.t));
  const float* Q = qmem + d.q_off;
  const bool vec = (d.m & 3) == 0 && slot_vec(A, 0, task.t) && slot_vec(A, 1, task.t);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = d.sub, G = 64 / sub, g = lane / sub, cl = lane & (sub - 1);
  const int cw = sub < 64 ? sub * 4 : kPsgdCols;  // columns of a slab
  const int row0 = task.i * d.prb;
  for (int e = threadIdx.x; e < d.prb * RP; e += kBlock) s_p[e] = 0.0;
  for (int c0 = 0; c0 < d.m; c0 += cw) {
    __syncthreads();  // the previous slab's readers are done
    for (int e = threadIdx.x; e < cw * RP; e += kBlock) {
      const int c = e / RP, j = e % RP;
      s_q[j * kPsgdCols + c] = (j < d.r && c0 + c < d.m) ? Q[static_cast<int64_t>(c0 + c) * d.r + j] : 0.f;
    }
    __syncthreads();
    for (int lr = w * G + g; lr < d.prb; lr += 4 * G) {  // uniform trip count: prb % (4 G) == 0
      const int row = row0 + lr;
      double acc[RP];
#pragma unroll
      for (int j = 0; j < RP; ++j) acc[j] = 0.0;
      for (int cc = cl * 4; cc < cw; cc += sub * 4) {
        const int c = c0 + cc;
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        if (row < d.n && c < d.m) {
          const int64_t o = static_cast<int64_t>(row) * d.m + c;
          if (vec) {
            gf4 v = *gptr<gf4>(M + o);
            if (use_error) v = v + *gptr<gf4>(E + o);
            *gptr_w<gf4>(E + o) = v;
#pragma unroll
            for (int i = 0; i < 4; ++i) e[i] = v[i];
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (c + i < d.m) {
                float v = M[o + i];
                if (use_error) v = v + E[o + i];
                E[o + i] = v;
                e[i] = v;
              }
          }
        }
#pragma unroll
        for (int j = 0; j < RP; ++j) {
          const gf4 q = *reinterpret_cast<const gf4*>(&s_q[j * kPsgdCols + cc]);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[j] = acc[j] + static_cast<double>(e[i]) * static_cast<double>(q[i]);
        }
      }
#pragma unroll
      for (int j = 0; j < RP; ++j) acc[j] = psgd_group_sum(acc[j], sub);
      if (cl == 0) {
#pragma unroll
        for (int j = 0; j < RP; ++j) s_p[lr * RP + j] = s_p[lr * RP + j] + acc[j];
      }
    }
  }
  __syncthreads();
  const int rows = min(d.prb, d.n - row0);
  float* P = pmem + d.p_off + static_cast<int64_t>(row0) * d.r;
  for (int e = threadIdx.x; e < rows * d.r; e += kBlock) P[e] = static_cast<float>(s_p[(e / d.r) * RP + e % d.r]);
}

// ------------------------------------------------------------------ backproject
// thread -> column strip's lane, rows w, w + 4, ... of the row block; the 4 row groups are
// added in wave order, then the block's partial goes to its own slot of the scratch
template <int RP>
__global__ void __launch_bounds__(kBlock) psgd_backproject_kernel(PlanArgs A, PsgdTables T, const float* pmem) {
  __shared__ double s_p[kPsgdRows * RP];
  __shared__ double s_acc[(kBlock / 64 - 1) * RP * 64];
  const PsgdTask task = T.back[blockIdx.x];
  const PsgdDesc d = T.desc[task.t];
  const float* E = static_cast<const float*>(slot_ptr(A, 1, task.t));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row0 = task.i * kPsgdRows, rows = min(kPsgdRows, d.n - row0);
  const int c = task.j * kPsgdStrip + lane;
  psgd_stage_p<RP>(s_p, pmem + d.p_off, d, row0);
  __syncthreads();
  double acc[RP];
#pragma unroll
  for (int j = 0; j < RP; ++j) acc[j] = 0.0;
  if (c < d.m) {
    const float* col = E + static_cast<int64_t>(row0) * d.m + c;
#pragma unroll 4
    for (int lr = w; lr < rows; lr += 4) {
      const double e = col[static_cast<int64_t>(lr) * d.m];
#pragma unroll
      for (int j = 0; j < RP; ++j) acc[j] = acc[j] + e * s_p[lr * RP + j];
    }
  }
  if (w > 0) {
#pragma unroll
    for (int j = 0; j < RP; ++j) s_acc[((w - 1) * RP + j) * 64 + lane] = acc[j];
  }
  __syncthreads();
  if (w == 0 && c < d.m) {
    double* out = T.part + d.part_off + (static_cast<int64_t>(task.i) * d.m + c) * d.r;
#pragma unroll
    for (int j = 0; j < RP; ++j)
      if (j < d.r) {
        double s = acc[j];
#pragma unroll
        for (int k = 0; k < kBlock / 64 - 1; ++k) s = s + s_acc[(k * RP + j) * 64 + lane];
        out[j] = s;
      }
  }
}

__global__ void __launch_bounds__(kBlock) psgd_fold_kernel(PsgdTables T, float* qmem) {
  const PsgdTask task = T.fold[blockIdx.x];
  const PsgdDesc d = T.desc[task.t];
  const int64_t mr = static_cast<int64_t>(d.m) * d.r, e = static_cast<int64_t>(task.i) * kBlock + threadIdx.x;
  if (e >= mr) return;
  const double* part = T.part + d.part_off + e;
  double s = part[0];
  for (int b = 1; b < d.nrb; ++b) s = s + part[b * mr];
  qmem[d.q_off + e] = static_cast<float>(s);
}

// ------------------------------------------------------------------ reconstruct
// A workgroup owns a 64-column strip over ALL rows, so it is the only reader of its Q rows
// and can scale them in place: every wave loads them, a barrier, wave 0 stores them.  P
// comes through LDS a row block at a time; thread -> the strip's lane, rows w, w + 4, ...
template <int RP>
__global__ void __launch_bounds__(kBlock) psgd_reconstruct_kernel(PlanArgs A, PsgdTables T, const float* pmem,
                                                                  float* qmem, float inv_ws) {
  __shared__ float s_p[kPsgdRows * RP];
  const PsgdTask task = T.recon[blockIdx.x];
  const PsgdDesc d = T.desc[task.t];
  float* Gm = static_cast<float*>(slot_ptr(A, 0, task.t));
  float* E = static_cast<float*>(slot_ptr(A, 1, task.t));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = task.j * kPsgdStrip + lane;
  const bool cok = c < d.m;
  float* Qrow = qmem + d.q_off + static_cast<int64_t>(cok ? c : 0) * d.r;
  float q[RP];
#pragma unroll
  for (int j = 0; j < RP; ++j) q[j] = (cok && j < d.r) ? Qrow[j] * inv_ws : 0.f;
  __syncthreads();
  if (w == 0 && cok) {
#pragma unroll
    for (int j = 0; j < RP; ++j)
      if (j < d.r) Qrow[j] = q[j];
  }
  for (int row0 = 0; row0 < d.n; row0 += kPsgdRows) {
    if (row0) __syncthreads();
    psgd_stage_p<RP>(s_p, pmem + d.p_off, d, row0);
    __syncthreads();
    const int rows = min(kPsgdRows, d.n - row0);
    if (cok) {
#pragma unroll 4
      for (int lr = w; lr < rows; lr += 4) {
        const int64_t o = static_cast<int64_t>(row0 + lr) * d.m + c;
        // the r products can cancel: G and E = M' - G are each one rounding from the exact values
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < RP; ++j) s = s + static_cast<double>(s_p[lr * RP + j]) * static_cast<double>(q[j]);
        const float a = static_cast<float>(s);
        const float e = E[o];
        Gm[o] = a;
        E[o] = e - a;
      }
    }
  }
}

// One grouped launch through the plan's stream bookkeeping (as Muon's): pointer-table
// flush, the launch timer's event pair (one record of `kind`), the last-stream mark.
template <class K, class... Args>
int psgd_launch(gs_plan* p, int kind, int grid, size_t lds, void* stream, K kernel, Args... args) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (grid <= 0) return GS_OK;
  GS_TRY_RET(hip_plan_flush(p, stream));
  const bool capturing = stream_capturing(s);
  const int nslots = capturing ? 0 : static_cast<int>(p->timer_ev.size() / 2);
  const int tk = p->timer_next;
  if (nslots)
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, static_cast<hipEvent_t>(p->timer_ev[2 * tk]),
                          static_cast<hipEvent_t>(p->timer_ev[2 * tk + 1]), 0, args...);
  else
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, args...);
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

#define PSGD_DISPATCH_RP(RPV, NAME, ...)                         \
  switch (RPV) {                                                 \
    case 1: { constexpr int NAME = 1; __VA_ARGS__; break; }      \
    case 2: { constexpr int NAME = 2; __VA_ARGS__; break; }      \
    case 4: { constexpr int NAME = 4; __VA_ARGS__; break; }      \
    case 8: { constexpr int NAME = 8; __VA_ARGS__; break; }      \
    default: return fail(GS_ESTATE, "gs_psgd: no layout");       \
  }

}  // namespace

// desc | proj | back | fold | recon | orth P | orth Q | partial sums in one allocation
int hip_psgd_upload(gs_plan* p, const PsgdTaskLists& l) {
  DeviceGuard g(p->device);
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const std::vector<PsgdTask>* lists[6] = {&l.proj, &l.back, &l.fold, &l.recon, &l.orth[0], &l.orth[1]};
  size_t offs[7];
  offs[0] = al(sizeof(PsgdDesc) * p->psgd.size());
  for (int i = 0; i < 6; ++i) offs[i + 1] = offs[i] + al(sizeof(PsgdTask) * lists[i]->size());
  const size_t total = offs[6] + al(sizeof(double) * static_cast<size_t>(l.part_elems));
  if (p->d_psgd) {
    HIP_RET(hipDeviceSynchronize());  // a launch in flight may still read the old tables
    HIP_RET(hipFree(p->d_psgd));
    p->d_psgd = nullptr;
  }
  p->psgd_tab = PsgdTables{};
  if (p->psgd.empty()) return GS_OK;
  char* dmem = nullptr;
  HIP_RET(hipMalloc(reinterpret_cast<void**>(&dmem), std::max<size_t>(total, 256)));
  p->d_psgd = dmem;
  HIP_RET(hipMemcpy(dmem, p->psgd.data(), sizeof(PsgdDesc) * p->psgd.size(), hipMemcpyHostToDevice));
  for (int i = 0; i < 6; ++i)
    if (!lists[i]->empty())
      HIP_RET(hipMemcpy(dmem + offs[i], lists[i]->data(), sizeof(PsgdTask) * lists[i]->size(), hipMemcpyHostToDevice));
  PsgdTables& T = p->psgd_tab;
  T.desc = reinterpret_cast<const PsgdDesc*>(dmem);
  auto tab = [&](int i) { return reinterpret_cast<const PsgdTask*>(dmem + offs[i]); };
  T.proj = tab(0);
  T.back = tab(1);
  T.fold = tab(2);
  T.recon = tab(3);
  T.orth[0] = tab(4);
  T.orth[1] = tab(5);
  T.part = reinterpret_cast<double*>(dmem + offs[6]);
  T.n_proj = static_cast<int32_t>(l.proj.size());
  T.n_back = static_cast<int32_t>(l.back.size());
  T.n_fold = static_cast<int32_t>(l.fold.size());
  T.n_recon = static_cast<int32_t>(l.recon.size());
  T.n_orth = static_cast<int32_t>(l.orth[0].size());
  for (int which = 0; which < 2; ++which) {
    int64_t most = 0;  // the largest factor that stays resident
    for (const PsgdDesc& d : p->psgd) {
      const int64_t e = static_cast<int64_t>(which ? d.m : d.n) * d.r;
      if (e <= kPsgdOrthLds) most = std::max(most, e);
    }
    T.orth_lds[which] = static_cast<int32_t>(most * sizeof(float));
  }
  return GS_OK;
}

int hip_psgd_orthogonalize(gs_plan* p, int which, float* mem, float eps, void* stream) {
  DeviceGuard g(p->device);
  const PsgdTables& T = p->psgd_tab;
  const size_t lds = static_cast<size_t>(T.orth_lds[which]);
  PSGD_DISPATCH_RP(p->psgd_rp, RP, {
    // above the 64 KiB every kernel may take, the launch needs the kernel's limit raised
    if (lds > 65536)
      HIP_RET(hipFuncSetAttribute(reinterpret_cast<const void*>(psgd_orth_kernel<RP>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    return psgd_launch(p, GS_OP_PSGD_ORTH, T.n_orth, lds, stream, psgd_orth_kernel<RP>, T, mem, which, eps);
  });
  return GS_OK;
}

int hip_psgd_project(gs_plan* p, int use_error, float* pmem, const float* qmem, void* stream) {
  DeviceGuard g(p->device);
  const PsgdTables& T = p->psgd_tab;
  PSGD_DISPATCH_RP(p->psgd_rp, RP,
                   return psgd_launch(p, GS_OP_PSGD_PROJECT, T.n_proj, 0, stream, psgd_project_kernel<RP>, p->args(), T,
                                      pmem, qmem, use_error));
  return GS_OK;
}

int hip_psgd_backproject(gs_plan* p, const float* pmem, float* qmem, void* stream) {
  DeviceGuard g(p->device);
  const PsgdTables& T = p->psgd_tab;
  PSGD_DISPATCH_RP(p->psgd_rp, RP,
                   GS_TRY_RET(psgd_launch(p, GS_OP_PSGD_BACKPROJECT, T.n_back, 0, stream, psgd_backproject_kernel<RP>,
                                          p->args(), T, pmem)));
  return psgd_launch(p, GS_OP_PSGD_BACKPROJECT, T.n_fold, 0, stream, psgd_fold_kernel, T, qmem);
}

int hip_psgd_reconstruct(gs_plan* p, const float* pmem, float* qmem, float inv_ws, void* stream) {
  DeviceGuard g(p->device);
  const PsgdTables& T = p->psgd_tab;
  PSGD_DISPATCH_RP(p->psgd_rp, RP,
                   return psgd_launch(p, GS_OP_PSGD_RECONSTRUCT, T.n_recon, 0, stream, psgd_reconstruct_kernel<RP>,
                                      p->args(), T, pmem, qmem, inv_ws));
  return GS_OK;
}

}  // namespace gs
