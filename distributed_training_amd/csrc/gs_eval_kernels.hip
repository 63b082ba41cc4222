// gfx950 kernels of the evaluation metrics (include/gsync.h, gs_eval_accumulate): the
// cross-entropy and the top-k hits of a batch of logits, added to an accumulator that
// stays on the device until the end of the evaluation.
//
// Two launches, no atomics, nothing read back:
//   eval_rows_kernel: one wavefront per row.  Two passes over the row's K logits (the
//     second is served from cache): the maximum and a NaN flag, then the sum of
//     expf(z - max), #{z_j > z_y} and #{j < y : z_j == z_y}.  The row's result is one
//     8-byte word of the caller's scratch: {fp32 loss, int32 code}, code = the label's
//     rank, kEvalNanRow for a row that holds a NaN, kEvalSkip / kEvalBad for a row that
//     is not counted.
//   eval_fold_kernel: one workgroup.  The integer counts in any order (they are exact),
//     the loss terms in ascending row order in fp64 by one thread from LDS, then the
//     accumulator's eight words are advanced.
// The sum of the exponentials is a balanced tree: every lane adds its terms pairwise
// (a binary counter of partial sums, all in registers), then the wave's 6-level
// butterfly; ceil(log2 K) roundings lie on any path, which is what the tests' bound
// counts.  The host backend (gs_host.cpp) restates the rules with the same tree depth.
#include <hip/hip_runtime.h>

#include <climits>

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

template <int DT>
__global__ void __launch_bounds__(kBlock)
eval_rows_kernel(const void* __restrict__ logits, const int64_t* __restrict__ labels, int64_t B, int K,
                 int64_t row_stride, int64_t n_valid, int64_t ignore_index, EvalRow* __restrict__ ws) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= B) return;  // wave-uniform
  const int64_t y = labels[row];
  if (row >= n_valid || y == ignore_index || y < 0 || y >= K) {
    if (lane == 0) ws[row] = EvalRow{0.f, (row >= n_valid || y == ignore_index) ? kEvalSkip : kEvalBad};
    return;
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
    if (lane == 0) ws[row] = EvalRow{__uint_as_float(0x7FC00000u), kEvalNanRow};
    return;
  }
  // pass 2: the pairwise sum of the lane's terms (LaneTree), the two counts of the rank
  LaneTree tree;
  int gt = 0, eq = 0;
  uint32_t cnt = 0;  // wave-uniform: a lane past the row's end adds an exact 0
  for (int j0 = 0; j0 < K; j0 += kWave, ++cnt) {
    const int j = j0 + lane;
    float e = 0.f;
    if (j < K) {
      const float z = ld_logit<DT>(logits, base + j);
      e = expf(z - m);
      gt += z > zy;
      eq += (z == zy) & (j < y);
    }
    tree.push(e, cnt);
  }
  float s = tree.fold(cnt);
  s = wave_sum(s);
  const int rank = wave_sum_i(gt) + wave_sum_i(eq);
  if (lane == 0) ws[row] = EvalRow{eval_loss(m, s, zy), rank};
}

__global__ void __launch_bounds__(kBlock)
eval_fold_kernel(const EvalRow* __restrict__ ws, int64_t B, EvalTopk topk, int64_t* __restrict__ acc) {
  __shared__ double s_loss[kBlock];
  __shared__ int64_t s_cnt[kBlock][6];
  const int t = threadIdx.x;
  int64_t c[6] = {0, 0, 0, 0, 0, 0};  // counted, bad, correct@topk[0..3]
  double total = 0.0;                 // thread 0's
  for (int64_t r0 = 0; r0 < B; r0 += kBlock) {
    const int64_t r = r0 + t;
    double l = 0.0;
    if (r < B) {
      const EvalRow w = ws[r];
      if (w.code >= 0) {
        l = static_cast<double>(w.loss);
        c[0] += 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) c[2 + i] += (i < topk.n && w.code < topk.k[i]);
      } else if (w.code == kEvalBad) {
        c[1] += 1;
      }
    }
    __syncthreads();
    s_loss[t] = l;
    __syncthreads();
    if (t == 0) {
      const int n = static_cast<int>(B - r0 < kBlock ? B - r0 : kBlock);
      for (int k = 0; k < n; ++k) {
        // a row that is not counted adds nothing (its 0 would turn a -0 total into +0)
        if (ws[r0 + k].code >= 0) total += s_loss[k];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) s_cnt[t][i] = c[i];
  __syncthreads();
  if (t < 6) {
    int64_t a = 0;
    for (int k = 0; k < kBlock; ++k) a += s_cnt[k][t];
    acc[t < 2 ? t : t + 2] += a;
  }
  if (t == 0) {
    double* lp = reinterpret_cast<double*>(acc + 2);
    *lp = *lp + total;
  }
}

}  // namespace

int hip_eval_accumulate(const void* logits, int dt, const int64_t* labels, int64_t B, int K, int64_t row_stride,
                        int64_t n_valid, const EvalTopk& topk, int64_t ignore_index, void* ws, void* acc,
                        void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((B + kRowsPerBlock - 1) / kRowsPerBlock)), block(kBlock);
  EvalRow* wp = static_cast<EvalRow*>(ws);
  switch (dt) {
    case GS_F32:
      hipLaunchKernelGGL((eval_rows_kernel<GS_F32>), grid, block, 0, s, logits, labels, B, K, row_stride, n_valid,
                         ignore_index, wp);
      break;
    case GS_BF16:
      hipLaunchKernelGGL((eval_rows_kernel<GS_BF16>), grid, block, 0, s, logits, labels, B, K, row_stride, n_valid,
                         ignore_index, wp);
      break;
    default:
      hipLaunchKernelGGL((eval_rows_kernel<GS_F16>), grid, block, 0, s, logits, labels, B, K, row_stride, n_valid,
                         ignore_index, wp);
      break;
  }
  HIP_RET(hipGetLastError());
  hipLaunchKernelGGL(eval_fold_kernel, dim3(1), block, 0, s, wp, B, topk, static_cast<int64_t*>(acc));
  HIP_RET(hipGetLastError());
  return GS_OK;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_eval_accumulate(int device_kind, const void* logits, int logits_dtype, const int64_t* labels,
                                  int64_t B, int64_t K, int64_t row_stride, int64_t n_valid, const int32_t* topk,
                                  int n_topk, int64_t ignore_index, void* ws, void* acc, void* stream) {
  const std::string w("gs_eval_accumulate");
  GS_CHECK_ARG(device_kind == GS_DEV_HOST || device_kind == GS_DEV_HIP, w + ": unknown device kind");
  GS_CHECK_ARG(is_float_dtype(logits_dtype), w + ": logits must be f32, bf16 or f16");
  GS_CHECK_ARG(B >= 0 && B <= (int64_t(1) << 31) - 64, w + ": B out of range");
  GS_CHECK_ARG(K >= 1 && K <= (int64_t(1) << 30), w + ": K must be in [1, 2^30]");
  GS_CHECK_ARG(row_stride >= K && row_stride <= (INT64_MAX / 8) / (B > 0 ? B : 1), w + ": row_stride < K or too large");
  GS_CHECK_ARG(n_valid >= 0 && n_valid <= B, w + ": n_valid must be in [0, B]");
  GS_CHECK_ARG(n_topk >= 0 && n_topk <= 4 && (n_topk == 0 || topk), w + ": at most 4 top-k values");
  EvalTopk tk{};
  tk.n = n_topk;
  for (int i = 0; i < n_topk; ++i) {
    GS_CHECK_ARG(topk[i] >= 1, w + ": a top-k value must be >= 1");
    tk.k[i] = topk[i];
  }
  GS_CHECK_ARG(acc && (reinterpret_cast<uintptr_t>(acc) & 7u) == 0, w + ": acc must be an 8-byte aligned pointer");
  if (B == 0) return GS_OK;
  GS_CHECK_ARG(logits && labels && ws, w + ": null pointer");
  GS_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(labels) & 7u) == 0 &&
                   reinterpret_cast<uintptr_t>(logits) % dtype_size(logits_dtype) == 0,
               w + ": misaligned pointer");
  if (device_kind == GS_DEV_HOST)
    return host_eval_accumulate(logits, logits_dtype, labels, B, static_cast<int>(K), row_stride, n_valid, tk,
                                ignore_index, ws, acc);
  return hip_eval_accumulate(logits, logits_dtype, labels, B, static_cast<int>(K), row_stride, n_valid, tk,
                             ignore_index, ws, acc, stream);
}
