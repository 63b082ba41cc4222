// gfx950 kernels of the training criterion (include/gsync.h, gs_xent_fwd / gs_xent_bwd):
// the cross-entropy of a batch of logits with label smoothing, its reduced value, and the
// gradient with respect to the logits, with no [B, K] fp32 temporary and nothing read back.
//
// Forward, two launches, no atomics:
//   xent_rows_kernel: one wavefront per row, as eval_rows_kernel.  Two passes over the row's K
//     logits (the second is served from cache): the maximum and a NaN flag, then the sum of
//     expf(z - max), the sum of z (label smoothing only) and the two counts of the label's
//     rank.  Both sums are the balanced tree of gs_wave.h.  The row's result is 16 bytes:
//     {loss, m, logS, code}: what the backward needs to rebuild the softmax.
//   xent_fold_kernel: one workgroup.  The integer counts in any order (they are exact), the
//     losses in ascending row order in fp64 by one thread from LDS, then the 16-byte reduced
//     result and, if asked for, the Metrics accumulator's words (the unsmoothed loss is
//     rebuilt from m, logS and the label's logit).
// Backward, one launch:
//   xent_bwd_kernel: a wavefront takes kBwdChunk consecutive elements of a row and writes
//     c * (softmax - q) in the logits' dtype, 16 bytes per lane and access where the
//     pointers and row strides allow it, one element otherwise.  The row's tail past the
//     last whole vector, and nothing past K, is handled element by element.
// The three kernels take a MIX template parameter for gs_xent_mix_fwd / gs_xent_mix_bwd: the pair
// targets of a MixUp / CutMix batch (labels a and b and a's weight lam per row, read on the device).
#include <hip/hip_runtime.h>

#include <climits>
#include <type_traits>

#include "gs_common.h"
#include "gs_wave.h"

namespace gs {
namespace {

#define HIP_RET(expr)                                                               \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess)                                                           \
      return fail(GS_EHIP, std::string(#expr " failed: ") + hipGetErrorString(_e)); \
  } while (0)

constexpr int kBwdChunk = 2048;     // elements of a row per wavefront of the backward
constexpr int kBwdMaxGrid = 65536;  // workgroups; beyond it the wavefronts stride over the tasks

// The targets of a batch: the labels, or with MIX the pair targets of gs_xent_mix_fwd / _bwd:
// labels a and b and a's weight lam, all read on the device.  The one-label instantiations
// keep their signature.
struct XentPair {
  const int64_t* a;
  const int64_t* b;
  const float* lam;
};
template <bool MIX>
using XentTarget = std::conditional_t<MIX, XentPair, const int64_t* __restrict__>;

template <int DT, bool SMOOTH, bool MIX>
__global__ void __launch_bounds__(kBlock)
xent_rows_kernel(const void* __restrict__ logits, const XentTarget<MIX> labels, int64_t B, int K,
                 int64_t row_stride, int64_t ignore_index, float eps, XentRow* __restrict__ rows) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= B) return;  // wave-uniform
  int64_t y;  // the label the rank is counted against
  int64_t ya = 0, yb = 0;
  float lam = 1.f;
  bool one = true;
  if constexpr (MIX) {
    ya = labels.a[row], yb = labels.b[row], lam = labels.lam[row];
    const int32_t code = xent_mix_code(ya, yb, lam, K, ignore_index);
    if (code < 0) {
      if (lane == 0) rows[row] = XentRow{0.f, 0.f, 0.f, code};
      return;
    }
    one = xent_mix_one(ya, yb, lam);
    y = one ? ya : xent_mix_dominant(ya, yb, lam);
  } else {
    y = labels[row];
    if (y == ignore_index || y < 0 || y >= K) {
      if (lane == 0) rows[row] = XentRow{0.f, 0.f, 0.f, y == ignore_index ? kEvalSkip : kEvalBad};
      return;
    }
  }
  const int64_t base = row * row_stride;
  const float zy = ld_logit<DT>(logits, base + y);
  float m = -INFINITY;
  bool nan = false;
  for (int j = lane; j < K; j += kWave) {
    const float z = ld_logit<DT>(logits, base + j);
    nan |= z != z;
    m = fmaxf(m, z);
  }
  m = wave_max(m);
  if (__any(nan)) {
    const float q = __uint_as_float(0x7FC00000u);
    if (lane == 0) rows[row] = XentRow{q, q, q, kEvalNanRow};
    return;
  }
  LaneTree se, sz;
  int gt = 0, eq = 0;
  uint32_t cnt = 0;  // wave-uniform: a lane past the row's end adds an exact 0
  for (int j0 = 0; j0 < K; j0 += kWave, ++cnt) {
    const int j = j0 + lane;
    float e = 0.f, z = 0.f;
    if (j < K) {
      z = ld_logit<DT>(logits, base + j);
      e = expf(z - m);
      gt += z > zy;
      eq += (z == zy) & (j < y);
    }
    se.push(e, cnt);
    if constexpr (SMOOTH) sz.push(z, cnt);
  }
  const float s = wave_sum(se.fold(cnt));
  float t = 0.f;
  if constexpr (SMOOTH) t = wave_sum(sz.fold(cnt));
  const int rank = wave_sum_i(gt) + wave_sum_i(eq);
  const float logS = logf(s);
  if constexpr (MIX) {
    if (!one) {
      const float za = ld_logit<DT>(logits, base + ya), zb = ld_logit<DT>(logits, base + yb);
      if (lane == 0) rows[row] = XentRow{xent_mix_loss(m, logS, za, zb, lam, t, K, SMOOTH ? eps : 0.f), m, logS, rank};
      return;
    }
  }
  if (lane == 0) rows[row] = XentRow{xent_loss(m, logS, zy, t, K, SMOOTH ? eps : 0.f), m, logS, rank};
}

__device__ __forceinline__ float ld_logit_rt(const void* base, int dt, int64_t i) {
  return dt == GS_F32 ? ld_logit<GS_F32>(base, i) : dt == GS_BF16 ? ld_logit<GS_BF16>(base, i)
                                                                   : ld_logit<GS_F16>(base, i);
}

template <bool MIX>
__global__ void __launch_bounds__(kBlock)
xent_fold_kernel(const XentRow* __restrict__ rows, const void* __restrict__ logits, int dt,
                 const XentTarget<MIX> labels, int64_t B, int64_t row_stride, float eps, EvalTopk topk,
                 int64_t* __restrict__ acc, XentRed* __restrict__ red) {
  __shared__ double s_loss[kBlock];
  __shared__ double s_nll[kBlock];
  __shared__ int s_on[kBlock];
  __shared__ int64_t s_cnt[kBlock][6];
  const int t = threadIdx.x;
  int64_t c[6] = {0, 0, 0, 0, 0, 0};  // counted, bad, correct@topk[0..3]
  double total = 0.0, total_nll = 0.0;  // thread 0's
  for (int64_t r0 = 0; r0 < B; r0 += kBlock) {
    const int64_t r = r0 + t;
    double l = 0.0, n = 0.0;
    int on = 0;
    if (r < B) {
      const XentRow w = rows[r];
      if (w.code >= 0) {
        on = 1;
        l = static_cast<double>(w.loss);
        n = l;
        // the unsmoothed loss of the accumulator: gs_eval_accumulate's expression
        if (acc != nullptr && eps != 0.f) {
          if constexpr (MIX) {
            const int64_t ya = labels.a[r], yb = labels.b[r];
            const float lam = labels.lam[r];
            const float za = ld_logit_rt(logits, dt, r * row_stride + ya);
            n = static_cast<double>(
                xent_mix_one(ya, yb, lam)
                    ? (w.m - za) + w.logS
                    : xent_mix_loss(w.m, w.logS, za, ld_logit_rt(logits, dt, r * row_stride + yb), lam, 0.f, 1, 0.f));
          } else {
            n = static_cast<double>((w.m - ld_logit_rt(logits, dt, r * row_stride + labels[r])) + w.logS);
          }
        }
        c[0] += 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) c[2 + i] += (i < topk.n && w.code < topk.k[i]);
      } else if (w.code == kEvalBad) {
        c[1] += 1;
      }
    }
    __syncthreads();
    s_loss[t] = l;
    s_nll[t] = n;
    s_on[t] = on;
    __syncthreads();
    if (t == 0) {
      const int cn = static_cast<int>(B - r0 < kBlock ? B - r0 : kBlock);
      for (int k = 0; k < cn; ++k) {
        // a row that is not counted adds nothing (its 0 would turn a -0 total into +0)
        if (s_on[k]) {
          total += s_loss[k];
          total_nll += s_nll[k];
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) s_cnt[t][i] = c[i];
  __syncthreads();
  if (t < 6) {
    int64_t a = 0;
    for (int k = 0; k < kBlock; ++k) a += s_cnt[k][t];
    s_cnt[0][t] = a;  // column t of row 0 is read by thread t alone above
    if (acc != nullptr) acc[t < 2 ? t : t + 2] += a;
  }
  __syncthreads();
  if (t == 0) {
    *red = xent_reduce(total, s_cnt[0][0], s_cnt[0][1]);
    if (acc != nullptr) {
      double* lp = reinterpret_cast<double*>(acc + 2);
      *lp = *lp + total_nll;
    }
  }
}

// the 16-byte access: 4 fp32 or 8 16-bit elements
template <int DT>
struct Vec {
  static constexpr int kElems = DT == GS_F32 ? 4 : 8;
  uint32_t w[4];
  __device__ __forceinline__ float get(int i) const {
    if constexpr (DT == GS_F32) return __uint_as_float(w[i]);
    else return to_f32<DT>(static_cast<uint16_t>(w[i >> 1] >> ((i & 1) * 16)));
  }
  __device__ __forceinline__ void set(int i, float v) {
    if constexpr (DT == GS_F32) {
      w[i] = __float_as_uint(v);
    } else {
      const uint32_t h = from_f32<DT>(v);
      w[i >> 1] = (i & 1) ? (w[i >> 1] | (h << 16)) : h;
    }
  }
};

template <int DT>
__device__ __forceinline__ void st_grad(void* base, int64_t i, float v) {
  if constexpr (DT == GS_F32) static_cast<float*>(base)[i] = v;
  else static_cast<uint16_t*>(base)[i] = from_f32<DT>(v);
}

template <int DT, bool VEC, bool MIX>
__global__ void __launch_bounds__(kBlock)
xent_bwd_kernel(const void* __restrict__ logits, const XentTarget<MIX> labels, int K, int64_t row_stride,
                float eps, int reduction, const XentRow* __restrict__ rows, const XentRed* __restrict__ red,
                const float* __restrict__ grad_out, void* __restrict__ dlogits, int64_t d_row_stride,
                int chunks_per_row, int64_t n_tasks) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kRowsPerBlock;
  const float q_off = eps / static_cast<float>(K);
  const float q_on = (1.f - eps) + q_off;
  // task = (row, chunk of the row): wave-uniform
  for (int64_t task = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + (threadIdx.x >> 6); task < n_tasks;
       task += n_waves) {
    const int64_t row = task / chunks_per_row;
    const int j_begin = static_cast<int>(task % chunks_per_row) * kBwdChunk;
    const int j_end = K - j_begin < kBwdChunk ? K : j_begin + kBwdChunk;
    const XentRow w = rows[row];
    const bool on = w.code >= 0;
    float c = 0.f;
    int64_t y = -1;
    int64_t yb = -1;  // MIX: a mixed row's second label, with targets qa at y and qb at yb
    float qa = q_on, qb = q_off;
    if (on) {
      if constexpr (MIX) {
        y = labels.a[row];
        const int64_t b = labels.b[row];
        const float lam = labels.lam[row];
        if (!xent_mix_one(y, b, lam)) {
          yb = b;
          qa = xent_mix_q(eps, lam, q_off);
          qb = xent_mix_q(eps, 1.f - lam, q_off);
        }
      } else {
        y = labels[row];
      }
      const float g = grad_out[reduction == kXentNone ? row : 0];
      c = reduction == kXentMean ? g / static_cast<float>(red->counted) : g;
    }
    const int64_t zb = row * row_stride, db = row * d_row_stride;
    auto elem = [&](float z, int j) {
      if constexpr (MIX) return xent_grad(z, w.m, w.logS, j == y ? qa : j == yb ? qb : q_off, c);
      else return xent_grad(z, w.m, w.logS, j == y ? q_on : q_off, c);
    };
    if constexpr (VEC) {
      constexpr int V = Vec<DT>::kElems;
      constexpr int64_t kElemBytes = 16 / V;
      for (int j = j_begin + lane * V; j < j_end; j += kWave * V) {
        if (j + V <= K) {  // a chunk is a multiple of V: a whole vector inside the row is inside the chunk
          Vec<DT> v;
          if (on) {
            const uint4 in = *reinterpret_cast<const uint4*>(static_cast<const char*>(logits) + (zb + j) * kElemBytes);
            v.w[0] = in.x, v.w[1] = in.y, v.w[2] = in.z, v.w[3] = in.w;
            Vec<DT> o;
#pragma unroll
            for (int i = 0; i < V; ++i) o.set(i, elem(v.get(i), j + i));
            v = o;
          } else {
            v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0u;
          }
          *reinterpret_cast<uint4*>(static_cast<char*>(dlogits) + (db + j) * kElemBytes) =
              make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
        } else {
          for (int jj = j; jj < K; ++jj)
            st_grad<DT>(dlogits, db + jj, on ? elem(ld_logit<DT>(logits, zb + jj), jj) : 0.f);
        }
      }
    } else {
      for (int j = j_begin + lane; j < j_end; j += kWave)
        st_grad<DT>(dlogits, db + j, on ? elem(ld_logit<DT>(logits, zb + j), j) : 0.f);
    }
  }
}

template <bool MIX>
int launch_xent_fwd(const void* logits, int dt, XentTarget<MIX> labels, int64_t B, int K, int64_t row_stride,
                    int64_t ignore_index, float eps, void* rows, void* red, const EvalTopk& topk, void* acc,
                    void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(kBlock);
  XentRow* rp = static_cast<XentRow*>(rows);
  if (B > 0) {
    const dim3 grid(static_cast<unsigned>((B + kRowsPerBlock - 1) / kRowsPerBlock));
    GS_DISPATCH_FLOAT(dt, DT, {
      if (eps != 0.f)
        hipLaunchKernelGGL((xent_rows_kernel<DT, true, MIX>), grid, block, 0, s, logits, labels, B, K, row_stride,
                           ignore_index, eps, rp);
      else
        hipLaunchKernelGGL((xent_rows_kernel<DT, false, MIX>), grid, block, 0, s, logits, labels, B, K, row_stride,
                           ignore_index, eps, rp);
    });
    HIP_RET(hipGetLastError());
  }
  hipLaunchKernelGGL(xent_fold_kernel<MIX>, dim3(1), block, 0, s, rp, logits, dt, labels, B, row_stride, eps, topk,
                     B > 0 ? static_cast<int64_t*>(acc) : nullptr, static_cast<XentRed*>(red));
  HIP_RET(hipGetLastError());
  return GS_OK;
}

template <bool MIX>
int launch_xent_bwd(const void* logits, int dt, XentTarget<MIX> labels, int64_t B, int K, int64_t row_stride, float eps,
                    int reduction, const void* rows, const void* red, const float* grad_out, void* dlogits,
                    int64_t d_row_stride, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int chunks = (K + kBwdChunk - 1) / kBwdChunk;
  const int64_t n_tasks = B * chunks;
  const int64_t want = (n_tasks + kRowsPerBlock - 1) / kRowsPerBlock;
  const dim3 grid(static_cast<unsigned>(want < kBwdMaxGrid ? want : kBwdMaxGrid)), block(kBlock);
  const int64_t es = dtype_size(dt);
  const bool vec = ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(dlogits) |
                     static_cast<uintptr_t>(row_stride * es) | static_cast<uintptr_t>(d_row_stride * es)) & 15u) == 0;
  const XentRow* rp = static_cast<const XentRow*>(rows);
  const XentRed* dp = static_cast<const XentRed*>(red);
  GS_DISPATCH_FLOAT(dt, DT, {
    if (vec)
      hipLaunchKernelGGL((xent_bwd_kernel<DT, true, MIX>), grid, block, 0, s, logits, labels, K, row_stride, eps,
                         reduction, rp, dp, grad_out, dlogits, d_row_stride, chunks, n_tasks);
    else
      hipLaunchKernelGGL((xent_bwd_kernel<DT, false, MIX>), grid, block, 0, s, logits, labels, K, row_stride, eps,
                         reduction, rp, dp, grad_out, dlogits, d_row_stride, chunks, n_tasks);
  });
  HIP_RET(hipGetLastError());
  return GS_OK;
}

}  // namespace

int hip_xent_fwd(const void* logits, int dt, const int64_t* labels, int64_t B, int K, int64_t row_stride,
                 int64_t ignore_index, float eps, void* rows, void* red, const EvalTopk& topk, void* acc,
                 void* stream) {
  return launch_xent_fwd<false>(logits, dt, labels, B, K, row_stride, ignore_index, eps, rows, red, topk, acc, stream);
}

int hip_xent_mix_fwd(const void* logits, int dt, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                     int64_t B, int K, int64_t row_stride, int64_t ignore_index, float eps, void* rows, void* red,
                     const EvalTopk& topk, void* acc, void* stream) {
  return launch_xent_fwd<true>(logits, dt, XentPair{labels_a, labels_b, lam}, B, K, row_stride, ignore_index, eps,
                               rows, red, topk, acc, stream);
}

int hip_xent_bwd(const void* logits, int dt, const int64_t* labels, int64_t B, int K, int64_t row_stride, float eps,
                 int reduction, const void* rows, const void* red, const float* grad_out, void* dlogits,
                 int64_t d_row_stride, void* stream) {
  return launch_xent_bwd<false>(logits, dt, labels, B, K, row_stride, eps, reduction, rows, red, grad_out, dlogits,
                                d_row_stride, stream);
}

int hip_xent_mix_bwd(const void* logits, int dt, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                     int64_t B, int K, int64_t row_stride, float eps, int reduction, const void* rows, const void* red,
                     const float* grad_out, void* dlogits, int64_t d_row_stride, void* stream) {
  return launch_xent_bwd<true>(logits, dt, XentPair{labels_a, labels_b, lam}, B, K, row_stride, eps, reduction, rows,
                               red, grad_out, dlogits, d_row_stride, stream);
}

}  // namespace gs

using namespace gs;

namespace {
// the checks gs_xent_fwd and gs_xent_bwd share, in gs_eval_accumulate's order
int xent_check_shape(const std::string& w, int device_kind, int logits_dtype, int64_t B, int64_t K,
                     int64_t row_stride, float eps) {
  GS_CHECK_ARG(device_kind == GS_DEV_HOST || device_kind == GS_DEV_HIP, w + ": unknown device kind");
  GS_CHECK_ARG(is_float_dtype(logits_dtype), w + ": logits must be f32, bf16 or f16");
  GS_CHECK_ARG(B >= 0 && B <= (int64_t(1) << 31) - 64, w + ": B out of range");
  GS_CHECK_ARG(K >= 1 && K <= (int64_t(1) << 30), w + ": K must be in [1, 2^30]");
  GS_CHECK_ARG(row_stride >= K && row_stride <= (INT64_MAX / 8) / (B > 0 ? B : 1), w + ": row_stride < K or too large");
  GS_CHECK_ARG(eps >= 0.f && eps <= 1.f, w + ": label_smoothing must be in [0, 1]");
  return GS_OK;
}
bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
}  // namespace

namespace {
// gs_xent_fwd (labels_b and lam null) and gs_xent_mix_fwd
int xent_fwd_entry(const std::string& w, bool mix, int device_kind, const void* logits, int logits_dtype,
                   const int64_t* labels, const int64_t* labels_b, const float* lam, int64_t B, int64_t K,
                   int64_t row_stride, int64_t ignore_index, float label_smoothing, void* rows, void* red,
                   const int32_t* topk, int n_topk, void* acc, void* stream) {
  GS_TRY_RET(xent_check_shape(w, device_kind, logits_dtype, B, K, row_stride, label_smoothing));
  GS_CHECK_ARG(n_topk >= 0 && n_topk <= 4 && (n_topk == 0 || topk), w + ": at most 4 top-k values");
  EvalTopk tk{};
  tk.n = n_topk;
  for (int i = 0; i < n_topk; ++i) {
    GS_CHECK_ARG(topk[i] >= 1, w + ": a top-k value must be >= 1");
    tk.k[i] = topk[i];
  }
  GS_CHECK_ARG(red && aligned(red, 16), w + ": red must be a 16-byte aligned pointer");
  GS_CHECK_ARG(aligned(acc, 8), w + ": acc must be null or an 8-byte aligned pointer");
  if (B > 0) {
    GS_CHECK_ARG(logits && labels && rows && (!mix || (labels_b && lam)), w + ": null pointer");
    GS_CHECK_ARG(aligned(rows, 16) && aligned(labels, 8) && aligned(labels_b, 8) && aligned(lam, 4) &&
                     reinterpret_cast<uintptr_t>(logits) % dtype_size(logits_dtype) == 0,
                 w + ": misaligned pointer");
  }
  const int k = static_cast<int>(K);
  if (device_kind == GS_DEV_HOST)
    return host_xent_mix_fwd(logits, logits_dtype, labels, labels_b, lam, B, k, row_stride, ignore_index,
                             label_smoothing, rows, red, tk, acc);
  if (mix)
    return hip_xent_mix_fwd(logits, logits_dtype, labels, labels_b, lam, B, k, row_stride, ignore_index,
                            label_smoothing, rows, red, tk, acc, stream);
  return hip_xent_fwd(logits, logits_dtype, labels, B, k, row_stride, ignore_index, label_smoothing, rows, red, tk, acc,
                      stream);
}

// gs_xent_bwd (labels_b and lam null) and gs_xent_mix_bwd
int xent_bwd_entry(const std::string& w, bool mix, int device_kind, const void* logits, int logits_dtype,
                   const int64_t* labels, const int64_t* labels_b, const float* lam, int64_t B, int64_t K,
                   int64_t row_stride, float label_smoothing, int reduction, const void* rows, const void* red,
                   const float* grad_out, void* dlogits, int64_t d_row_stride, void* stream) {
  GS_TRY_RET(xent_check_shape(w, device_kind, logits_dtype, B, K, row_stride, label_smoothing));
  GS_CHECK_ARG(d_row_stride >= K && d_row_stride <= (INT64_MAX / 8) / (B > 0 ? B : 1),
               w + ": d_row_stride < K or too large");
  GS_CHECK_ARG(reduction == kXentNone || reduction == kXentMean || reduction == kXentSum, w + ": unknown reduction");
  if (B == 0) return GS_OK;
  GS_CHECK_ARG(logits && labels && rows && red && grad_out && dlogits && (!mix || (labels_b && lam)),
               w + ": null pointer");
  const uintptr_t es = static_cast<uintptr_t>(dtype_size(logits_dtype));
  GS_CHECK_ARG(aligned(rows, 16) && aligned(red, 16) && aligned(labels, 8) && aligned(labels_b, 8) && aligned(lam, 4) &&
                   aligned(grad_out, 4) && reinterpret_cast<uintptr_t>(logits) % es == 0 &&
                   reinterpret_cast<uintptr_t>(dlogits) % es == 0,
               w + ": misaligned pointer");
  const uintptr_t z0 = reinterpret_cast<uintptr_t>(logits), d0 = reinterpret_cast<uintptr_t>(dlogits);
  const uintptr_t z1 = z0 + static_cast<uintptr_t>((B - 1) * row_stride + K) * es;
  const uintptr_t d1 = d0 + static_cast<uintptr_t>((B - 1) * d_row_stride + K) * es;
  GS_CHECK_ARG(d1 <= z0 || z1 <= d0, w + ": dlogits overlaps logits");
  const int k = static_cast<int>(K);
  if (device_kind == GS_DEV_HOST)
    return host_xent_mix_bwd(logits, logits_dtype, labels, labels_b, lam, B, k, row_stride, label_smoothing, reduction,
                             rows, red, grad_out, dlogits, d_row_stride);
  if (mix)
    return hip_xent_mix_bwd(logits, logits_dtype, labels, labels_b, lam, B, k, row_stride, label_smoothing, reduction,
                            rows, red, grad_out, dlogits, d_row_stride, stream);
  return hip_xent_bwd(logits, logits_dtype, labels, B, k, row_stride, label_smoothing, reduction, rows, red, grad_out,
                      dlogits, d_row_stride, stream);
}
}  // namespace

extern "C" int gs_xent_fwd(int device_kind, const void* logits, int logits_dtype, const int64_t* labels, int64_t B,
                           int64_t K, int64_t row_stride, int64_t ignore_index, float label_smoothing, void* rows,
                           void* red, const int32_t* topk, int n_topk, void* acc, void* stream) {
  return xent_fwd_entry("gs_xent_fwd", false, device_kind, logits, logits_dtype, labels, nullptr, nullptr, B, K,
                        row_stride, ignore_index, label_smoothing, rows, red, topk, n_topk, acc, stream);
}

extern "C" int gs_xent_mix_fwd(int device_kind, const void* logits, int logits_dtype, const int64_t* labels_a,
                               const int64_t* labels_b, const float* lam, int64_t B, int64_t K, int64_t row_stride,
                               int64_t ignore_index, float label_smoothing, void* rows, void* red, const int32_t* topk,
                               int n_topk, void* acc, void* stream) {
  return xent_fwd_entry("gs_xent_mix_fwd", true, device_kind, logits, logits_dtype, labels_a, labels_b, lam, B, K,
                        row_stride, ignore_index, label_smoothing, rows, red, topk, n_topk, acc, stream);
}

extern "C" int gs_xent_bwd(int device_kind, const void* logits, int logits_dtype, const int64_t* labels, int64_t B,
                           int64_t K, int64_t row_stride, int64_t ignore_index, float label_smoothing, int reduction,
                           const void* rows, const void* red, const float* grad_out, void* dlogits,
                           int64_t d_row_stride, void* stream) {
  (void)ignore_index;  // the rows' codes already say which rows it skipped
  return xent_bwd_entry("gs_xent_bwd", false, device_kind, logits, logits_dtype, labels, nullptr, nullptr, B, K,
                        row_stride, label_smoothing, reduction, rows, red, grad_out, dlogits, d_row_stride, stream);
}

extern "C" int gs_xent_mix_bwd(int device_kind, const void* logits, int logits_dtype, const int64_t* labels_a,
                               const int64_t* labels_b, const float* lam, int64_t B, int64_t K, int64_t row_stride,
                               int64_t ignore_index, float label_smoothing, int reduction, const void* rows,
                               const void* red, const float* grad_out, void* dlogits, int64_t d_row_stride,
                               void* stream) {
  (void)ignore_index;
  return xent_bwd_entry("gs_xent_mix_bwd", true, device_kind, logits, logits_dtype, labels_a, labels_b, lam, B, K,
                        row_stride, label_smoothing, reduction, rows, red, grad_out, dlogits, d_row_stride, stream);
}
