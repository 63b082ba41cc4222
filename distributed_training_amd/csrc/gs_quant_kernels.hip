// gfx950 kernels of the uint8 quantization comm hooks (include/gsync.h, gs_quant_* and
// gs_dequant_mean): a bucket of fp32 gradients to bytes with torch's MinMaxObserver qparams,
// per channel of bucket_size elements or for the whole bucket, and the mean of the ranks'
// dequantized payloads back into the bucket.  The arithmetic is gs_math.h's (quant_fold,
// quant_params, quant_value, dequant_value), the host backend's too; min and max are exact,
// so no order of the reductions can change a bit.
//
//   quant_perchannel  one launch.  A channel is W lanes of one wave, 4 elements (one 16-B load)
//                     a lane: W = the power of two covering bucket_size / 4 for channels of
//                     <= 256 elements, 64 / W of them side by side in a wave and a butterfly
//                     that stops at the group's width; above that a wave per channel, NJ <= 16
//                     loads a lane.  The values stay in registers from the min/max to the
//                     quantization; a lane's 4 bytes leave as one dword, the group's first lane
//                     writes the scale and the zero point.  A workgroup is 4 waves over
//                     consecutive channels; the grid covers the bucket once.
//   quant_minmax      per tensor, pass 1: a grid-stride sweep of at most GS_QUANT_PARTIALS
//                     workgroups, one (lo, hi) pair each (butterfly, then the 4 waves through LDS).
//   quant_pertensor   pass 2: every workgroup folds the pairs itself (a strided read, the same
//                     butterfly and LDS step), forms the qparams and quantizes its slices;
//                     workgroup 0 writes the qparams.  No atomics, no counter, no host read.
//   dequant_mean      one launch for both forms: a lane reads one dword of each rank's payload
//                     (base + rank * stride), adds the 4 dequantized terms in rank order in
//                     registers, divides by the world size and stores 16 bytes.  When a wave's
//                     256 elements lie in one channel its index is made wave-uniform, so the
//                     qparams come through the scalar cache.
//
// Alignment: bucket_size is a multiple of 16, so with a 16-B aligned bucket every lane's 4
// elements are one aligned 16-B access; a bucket that is only 4-B aligned, and the elements
// of the last channel around n, go element by element in the same kernels.
#include <hip/hip_runtime.h>

#include <algorithm>

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

constexpr int kQuantLane = 4;                      // elements of a lane's access
constexpr int kQuantChunk = kBlock * kQuantLane;   // elements of a workgroup's sweep step

// elements e .. e + 3: one 16-B load where vec, else those below n one by one (zeros past n)
__device__ __forceinline__ float4 quant_ld4(const float* __restrict__ x, int64_t e, int64_t n, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(x + e);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e < n) v.x = x[e];
  if (e + 1 < n) v.y = x[e + 1];
  if (e + 2 < n) v.z = x[e + 2];
  if (e + 3 < n) v.w = x[e + 3];
  return v;
}
__device__ __forceinline__ void quant_fold4(const float4& v, float* lo, float* hi) {
  quant_fold(v.x, lo, hi);
  quant_fold(v.y, lo, hi);
  quant_fold(v.z, lo, hi);
  quant_fold(v.w, lo, hi);
}
__device__ __forceinline__ uint32_t quant_pack4(const float4& v, float scale, float zpf) {
  return quant_value(v.x, scale, zpf) | (quant_value(v.y, scale, zpf) << 8) | (quant_value(v.z, scale, zpf) << 16) |
         (quant_value(v.w, scale, zpf) << 24);
}
__device__ __forceinline__ void quant_store_params(uint8_t* payload, int64_t Q, int64_t C, int64_t c,
                                                   const QuantParams& qp) {
  reinterpret_cast<float*>(payload + Q)[c] = qp.scale;
  reinterpret_cast<int32_t*>(payload + Q + 4 * C)[c] = qp.zp;
}

// ------------------------------------------------------------------ per channel
template <int NJ>
__global__ void __launch_bounds__(kBlock)
quant_perchannel_kernel(const float* __restrict__ x, int64_t n, int bs, int W, int64_t C, int64_t Q, int aligned,
                        uint8_t* __restrict__ payload) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int seg = lane / W, sl = lane & (W - 1);
  const int64_t c = (static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + wave) * (kWave / W) + seg;
  const int nf = bs / kQuantLane;  // 16-B accesses of a channel
  const bool live = c < C;         // a lane past the last channel still takes part in the butterfly
  float4 v[NJ];
  float lo = 0.f, hi = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int f = j * kWave + sl;
    v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && f < nf) {
      const int64_t e = c * bs + f * kQuantLane;
      v[j] = quant_ld4(x, e, n, aligned && e + kQuantLane <= n);
      quant_fold4(v[j], &lo, &hi);
    }
  }
  lo = seg_min(lo, W);
  hi = seg_max(hi, W);
  if (!live) return;
  const QuantParams qp = quant_params(lo, hi);
  const float zpf = static_cast<float>(qp.zp);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int f = j * kWave + sl;
    if (f < nf) *reinterpret_cast<uint32_t*>(payload + c * bs + f * kQuantLane) = quant_pack4(v[j], qp.scale, zpf);
  }
  if (sl == 0) quant_store_params(payload, Q, C, c, qp);
}

// ------------------------------------------------------------------ per tensor
// (lo, hi) over the workgroup, left in every thread
__device__ __forceinline__ void quant_block_minmax(float* lo, float* hi, float (*s_mm)[2]) {
  *lo = seg_min(*lo, kWave);
  *hi = seg_max(*hi, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_mm[threadIdx.x >> 6][0] = *lo;
    s_mm[threadIdx.x >> 6][1] = *hi;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kBlock / kWave; ++w) {
    *lo = fminf(*lo, s_mm[w][0]);
    *hi = fmaxf(*hi, s_mm[w][1]);
  }
}

__global__ void __launch_bounds__(kBlock)
quant_minmax_kernel(const float* __restrict__ x, int64_t n, int aligned, float2* __restrict__ pairs) {
  __shared__ float s_mm[kBlock / kWave][2];
  float lo = 0.f, hi = 0.f;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kQuantChunk;
  for (int64_t e = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * kQuantLane; e < n; e += step) {
    const float4 v = quant_ld4(x, e, n, aligned && e + kQuantLane <= n);
    quant_fold4(v, &lo, &hi);
  }
  quant_block_minmax(&lo, &hi, s_mm);
  if (threadIdx.x == 0) pairs[blockIdx.x] = make_float2(lo, hi);
}

__global__ void __launch_bounds__(kBlock)
quant_pertensor_kernel(const float* __restrict__ x, int64_t n, int aligned, const float2* __restrict__ pairs,
                       int n_pairs, int64_t Q, uint8_t* __restrict__ payload) {
  __shared__ float s_mm[kBlock / kWave][2];
  float lo = 0.f, hi = 0.f;
  for (int i = threadIdx.x; i < n_pairs; i += kBlock) {
    const float2 p = pairs[i];
    lo = fminf(lo, p.x);
    hi = fmaxf(hi, p.y);
  }
  quant_block_minmax(&lo, &hi, s_mm);
  const QuantParams qp = quant_params(lo, hi);
  const float zpf = static_cast<float>(qp.zp);
  const int64_t step = static_cast<int64_t>(gridDim.x) * kQuantChunk;
  for (int64_t e = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * kQuantLane; e < n; e += step) {
    const float4 v = quant_ld4(x, e, n, aligned && e + kQuantLane <= n);
    *reinterpret_cast<uint32_t*>(payload + e) = quant_pack4(v, qp.scale, zpf);  // e + 3 < Q: Q rounds n up to 16
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) quant_store_params(payload, Q, 1, 0, qp);
}

// ------------------------------------------------------------------ dequantize and average
// b16 = bucket_size / 16 (0: per tensor).  uniform: bucket_size is a multiple of 256 (or 0), a
// wave's 256 elements share a channel.
__global__ void __launch_bounds__(kBlock)
dequant_mean_kernel(const uint8_t* __restrict__ gathered, int64_t stride, int64_t Q, int64_t C, int ws,
                    float* __restrict__ out, int64_t n, uint32_t b16, int uniform, int aligned) {
  const int lane = threadIdx.x & (kWave - 1);
  // the wave's index in units of 256 elements: < 2^26 (n <= GS_QUANT_MAX_NUMEL), so * 16 fits 32 bits
  const uint32_t wi = __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6));
  const int64_t e = static_cast<int64_t>(wi) * (kWave * kQuantLane) + lane * kQuantLane;
  if (e >= n) return;
  uint32_t c = 0;
  if (b16) {
    const uint32_t u = wi * 16u;  // the wave's first element in units of 16
    c = u / b16 + (u % b16 + static_cast<uint32_t>(lane >> 2)) / b16;
    if (uniform) c = __builtin_amdgcn_readfirstlane(c);
  }
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 2
  for (int r = 0; r < ws; ++r) {
    const uint8_t* p = gathered + r * stride;
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p + e);
    const float scale = reinterpret_cast<const float*>(p + Q)[c];
    const float zpf = static_cast<float>(reinterpret_cast<const int32_t*>(p + Q + 4 * C)[c]);
    const float t0 = dequant_value(w & 255u, scale, zpf), t1 = dequant_value((w >> 8) & 255u, scale, zpf);
    const float t2 = dequant_value((w >> 16) & 255u, scale, zpf), t3 = dequant_value(w >> 24, scale, zpf);
    a0 = r ? a0 + t0 : t0;  // the sum starts from rank 0's term
    a1 = r ? a1 + t1 : t1;
    a2 = r ? a2 + t2 : t2;
    a3 = r ? a3 + t3 : t3;
  }
  const float d = static_cast<float>(ws);
  const float4 o = make_float4(a0 / d, a1 / d, a2 / d, a3 / d);
  if (aligned && e + kQuantLane <= n) {
    *reinterpret_cast<float4*>(out + e) = o;
  } else {
    out[e] = o.x;
    if (e + 1 < n) out[e + 1] = o.y;
    if (e + 2 < n) out[e + 2] = o.z;
    if (e + 3 < n) out[e + 3] = o.w;
  }
}

inline int is_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int sweep_grid(int64_t n) {
  return static_cast<int>(std::min<int64_t>(GS_QUANT_PARTIALS, (n + kQuantChunk - 1) / kQuantChunk));
}

int hip_quant_perchannel(const float* x, int64_t n, int bs, uint8_t* payload, hipStream_t s) {
  const QuantLayout l = quant_layout(n, bs);
  const int nf = bs / kQuantLane;
  int W = 4, nj = 1;
  while (W < nf && W < kWave) W <<= 1;
  while (nj * kWave < nf) nj <<= 1;
  const int64_t per_block = static_cast<int64_t>(kBlock / kWave) * (kWave / W);  // channels of a workgroup
  const dim3 grid(static_cast<unsigned>((l.C + per_block - 1) / per_block)), block(kBlock);
  const int al = is_aligned16(x);
#define GS_QUANT_LAUNCH(NJ) \
  hipLaunchKernelGGL(quant_perchannel_kernel<NJ>, grid, block, 0, s, x, n, bs, W, l.C, l.Q, al, payload)
  switch (nj) {
    case 1: GS_QUANT_LAUNCH(1); break;
    case 2: GS_QUANT_LAUNCH(2); break;
    case 4: GS_QUANT_LAUNCH(4); break;
    case 8: GS_QUANT_LAUNCH(8); break;
    default: GS_QUANT_LAUNCH(16); break;
  }
#undef GS_QUANT_LAUNCH
  HIP_RET(hipGetLastError());
  return GS_OK;
}

int hip_quant_pertensor(const float* x, int64_t n, uint8_t* payload, float2* pairs, hipStream_t s) {
  const QuantLayout l = quant_layout(n, 0);
  const int g = sweep_grid(n), al = is_aligned16(x);
  hipLaunchKernelGGL(quant_minmax_kernel, dim3(g), dim3(kBlock), 0, s, x, n, al, pairs);
  HIP_RET(hipGetLastError());
  hipLaunchKernelGGL(quant_pertensor_kernel, dim3(g), dim3(kBlock), 0, s, x, n, al, pairs, g, l.Q, payload);
  HIP_RET(hipGetLastError());
  return GS_OK;
}

int hip_dequant_mean(const uint8_t* gathered, int ws, float* out, int64_t n, int bs, hipStream_t s) {
  const QuantLayout l = quant_layout(n, bs);
  const dim3 grid(static_cast<unsigned>((n + kQuantChunk - 1) / kQuantChunk)), block(kBlock);
  hipLaunchKernelGGL(dequant_mean_kernel, grid, block, 0, s, gathered, l.bytes(), l.Q, l.C, ws, out, n,
                     static_cast<uint32_t>(bs / 16), bs % (kWave * kQuantLane) == 0, is_aligned16(out));
  HIP_RET(hipGetLastError());
  return GS_OK;
}

int quant_check(const std::string& w, int device_kind, int64_t n, int bs, bool per_tensor) {
  GS_CHECK_ARG(device_kind == GS_DEV_HOST || device_kind == GS_DEV_HIP, w + ": unknown device kind");
  GS_CHECK_ARG(n >= 0 && n <= GS_QUANT_MAX_NUMEL, w + ": n out of range");
  GS_CHECK_ARG(per_tensor ? bs == 0 : (bs >= 16 && bs <= 4096 && bs % 16 == 0),
               w + ": bucket_size must be a multiple of 16 in 16..4096");
  return GS_OK;
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" int64_t gs_quant_payload_bytes(int64_t n, int bucket_size) {
  GS_TRY_RET(quant_check("gs_quant_payload_bytes", GS_DEV_HOST, n, bucket_size, bucket_size == 0));
  return quant_layout(n, bucket_size).bytes();
}

static int quant_entry(const std::string& w, int device_kind, const float* x, int64_t n, int bs, void* payload,
                       int64_t payload_bytes, void* scratch, void* stream) {
  GS_TRY_RET(quant_check(w, device_kind, n, bs, bs == 0));
  if (n == 0) return GS_OK;
  GS_CHECK_ARG(x && payload, w + ": null pointer");
  GS_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3u) == 0 && (reinterpret_cast<uintptr_t>(payload) & 15u) == 0 &&
                   (reinterpret_cast<uintptr_t>(scratch) & 7u) == 0,
               w + ": misaligned pointer");
  GS_CHECK_ARG(payload_bytes >= quant_layout(n, bs).bytes(), w + ": the payload is smaller than gs_quant_payload_bytes");
  if (device_kind == GS_DEV_HOST) return host_quant(x, n, bs, payload);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (bs) return hip_quant_perchannel(x, n, bs, static_cast<uint8_t*>(payload), s);
  GS_CHECK_ARG(scratch, w + ": null scratch");
  return hip_quant_pertensor(x, n, static_cast<uint8_t*>(payload), static_cast<float2*>(scratch), s);
}

extern "C" int gs_quant_perchannel(int device_kind, const float* x, int64_t n, int bucket_size, void* payload,
                                   int64_t payload_bytes, void* stream) {
  GS_CHECK_ARG(bucket_size != 0, "gs_quant_perchannel: bucket_size must be a multiple of 16 in 16..4096");
  return quant_entry("gs_quant_perchannel", device_kind, x, n, bucket_size, payload, payload_bytes, nullptr, stream);
}

extern "C" int gs_quant_pertensor(int device_kind, const float* x, int64_t n, void* payload, int64_t payload_bytes,
                                  void* scratch, void* stream) {
  return quant_entry("gs_quant_pertensor", device_kind, x, n, 0, payload, payload_bytes, scratch, stream);
}

extern "C" int gs_dequant_mean(int device_kind, const void* gathered, int64_t gathered_bytes, int world_size,
                               float* out, int64_t n, int bucket_size, void* stream) {
  const std::string w("gs_dequant_mean");
  GS_TRY_RET(quant_check(w, device_kind, n, bucket_size, bucket_size == 0));
  GS_CHECK_ARG(world_size >= 1, w + ": world_size must be >= 1");
  if (n == 0) return GS_OK;
  GS_CHECK_ARG(gathered && out, w + ": null pointer");
  GS_CHECK_ARG((reinterpret_cast<uintptr_t>(gathered) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0,
               w + ": misaligned pointer");
  GS_CHECK_ARG(gathered_bytes / world_size >= quant_layout(n, bucket_size).bytes(),
               w + ": gathered is smaller than world_size payloads");
  if (device_kind == GS_DEV_HOST) return host_dequant_mean(gathered, world_size, out, n, bucket_size);
  return hip_dequant_mean(static_cast<const uint8_t*>(gathered), world_size, out, n, bucket_size,
                          static_cast<hipStream_t>(stream));
}
