// gfx950 kernels of the NHWC BatchNorm backward fused with the ReLU mask and
// the residual add (include/gsync.h, gs_bn_bwd_reduce / gs_bn_bwd_dx /
// gs_add_relu_fwd).  They replace MIOpen's BatchNormBwdSpatial pair plus ATen's
// threshold_backward, and the in-place add + ReLU at the end of a residual block.
//
// An activation is a row-major [R, C] bf16 matrix.  A thread owns 8 consecutive
// channels (one 16-B access) and walks down the rows; a 256-thread workgroup is
// tx x ty threads over a channel tile of tx vectors (tx = 8: 64 channels, one
// 128-B line per row) and ty = 256 / tx rows per step.  The grid is
// (channel tiles, P row-blocks): wide layers fill the chip from the channel
// axis, the stem and layer1 from the row axis (bn_geom).
//
// HBM-bound streaming, passes over the activation per BN backward:
//   reduce: x, dy (, y) in (, g out)         dx: x, dy|g (, y) in, dx out
// The per-channel sums (of g and of g * (x - mean)) cross workgroups through a [P, C, 2] fp32 workspace:
// every reduce workgroup stores its partial, every dx workgroup folds the P
// partials of its own channel tile in a fixed order (L2-served, P*P*8 / (6*R) of
// the streamed bytes, bounded by bn_geom) - the folded-partials idiom of the
// clipped update in gs_update_kernels.hip.  No atomics, so the result is
// deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "gs_common.h"

// 1: non-temporal loads of the streams a kernel reads for the last time
#ifndef GS_BN_NT
#define GS_BN_NT 0
#endif
// How dx becomes bf16.  0 (default): as the MIOpen kernels this path replaces convert it, by
// truncation, so that a training step computes what it computed with them (round-to-nearest dx
// is closer to the exact gradient, and moves ResNet-50's first SGD step by up to 3 % of the
// parameters' scale against the MIOpen path: DESIGN §3a).  1: round to nearest even.
#ifndef GS_BN_DX_RNE
#define GS_BN_DX_RNE 0
#endif

namespace gs {
namespace {

#define HIP_RET(expr)                                                               \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess)                                                           \
      return fail(GS_EHIP, std::string(#expr " failed: ") + hipGetErrorString(_e)); \
  } while (0)

typedef uint32_t bu4 __attribute__((ext_vector_type(4)));
typedef float bf4 __attribute__((ext_vector_type(4)));

constexpr int kBnTileVecs = 8;         // vectors (of 8 channels) per channel tile, at most
constexpr int kBnMaxP = 512;           // row-blocks, at most
constexpr int kBnTargetBlocks = 1024;  // 4 workgroups per CU
constexpr int kBnUnroll = 4;           // rows in flight per thread and stream

// The decomposition of (R, C), the same for both backward kernels.
//   P <= ceil(R / ty): a row-block has at least one step of rows;
//   P <= sqrt(R / 2): the fold (P * P * 8 bytes per channel) stays under half the
//        bytes streamed (R * 6 per channel), and it is read from L2;
//   tiles * P near kBnTargetBlocks, a multiple of 256 CUs where it exceeds them.
struct BnGeom {
  int tx_log2;
  int ctiles;
  int P;
  int64_t rpb;  // rows per row-block
};

BnGeom bn_geom(int64_t R, int C) {
  const int V = C / 8;
  int l2 = 0;
  while ((1 << l2) < V && (1 << l2) < kBnTileVecs) ++l2;
  const int tx = 1 << l2, ty = kBlock / tx;
  const int64_t ctiles = (V + tx - 1) / tx;
  int64_t P = std::min<int64_t>(kBnMaxP, (R + ty - 1) / ty);
  P = std::min<int64_t>(P, static_cast<int64_t>(std::sqrt(0.5 * static_cast<double>(R))));
  P = std::min<int64_t>(P, kBnTargetBlocks / ctiles);
  P = std::max<int64_t>(P, 1);
  if (ctiles * P > 256) {
    const int64_t step = 256 / std::min<int64_t>(256, ctiles & -ctiles);
    if (P >= step) P -= P % step;
  }
  const int64_t rpb = (R + P - 1) / P;
  P = (R + rpb - 1) / rpb;  // no empty row-block
  return BnGeom{l2, static_cast<int>(ctiles), static_cast<int>(P), rpb};
}

__device__ __forceinline__ uint32_t to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7FC0u;
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ void unpack8(const bu4& v, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(v[i] << 16);
    f[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
  }
}

// 8 floats that hold bf16 values exactly -> 8 bf16
__device__ __forceinline__ bu4 pack8_exact(const float (&f)[8]) {
  bu4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = (__float_as_uint(f[2 * i]) >> 16) | (__float_as_uint(f[2 * i + 1]) & 0xffff0000u);
  return v;
}

// fp32 -> bf16 by truncation; an Inf / NaN pattern with low mantissa bits stays a NaN
__device__ __forceinline__ uint32_t to_bf16_trunc(float f) {
  uint32_t u = __float_as_uint(f);
  if ((~u & 0x7f800000u) == 0 && (u & 0xffffu) != 0) u |= 0x10000u;
  return u >> 16;
}

__device__ __forceinline__ bu4 pack8_dx(const float (&f)[8]) {
  bu4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (GS_BN_DX_RNE) v[i] = to_bf16(f[2 * i]) | (to_bf16(f[2 * i + 1]) << 16);
    else v[i] = to_bf16_trunc(f[2 * i]) | (to_bf16_trunc(f[2 * i + 1]) << 16);
  }
  return v;
}

template <bool NT>
__device__ __forceinline__ bu4 ld16(const uint16_t* p) {
  const bu4* q = reinterpret_cast<const bu4*>(p);
  if constexpr (NT) return __builtin_nontemporal_load(q);
  else return *q;
}

__device__ __forceinline__ void st16(uint16_t* p, const bu4& v) { *reinterpret_cast<bu4*>(p) = v; }

// g = dy * [y > 0] as threshold_backward(dy, y, 0) forms it: y <= 0 ? 0 : dy (a NaN y passes dy)
__device__ __forceinline__ void relu_mask(float (&g)[8], const bu4& yv) {
  float yf[8];
  unpack8(yv, yf);
#pragma unroll
  for (int i = 0; i < 8; ++i) g[i] = yf[i] <= 0.f ? 0.f : g[i];
}

// ---- pass 1: per-workgroup partial sums of g and g * xhat (and g itself) ----
template <bool RELU, bool WRITE_G>
__global__ void __launch_bounds__(kBlock)
bn_bwd_reduce_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
                     uint16_t* __restrict__ gout, const float* __restrict__ mean, float* __restrict__ ws, int64_t R, int C, int tx_log2, int64_t rpb) {
  __shared__ float s_red[kBlock * 16];  // [ty][F], F = 16 * tx: (channel, {sum g, sum g*(x-mean)})
  __shared__ double s_grp[kBlock];      // [ty / 16][F]
  const int t = threadIdx.x;
  const int tx = 1 << tx_log2, ty = kBlock >> tx_log2;
  const int tx_i = t & (tx - 1), ty_i = t >> tx_log2;
  const int v = blockIdx.x * tx + tx_i;
  const bool active = v < (C >> 3);
  const int c0 = v * 8;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rpb;
  const int64_t r1 = std::min<int64_t>(R, r0 + rpb);

  float sg[8], sq[8], m[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sg[i] = 0.f;
    sq[i] = 0.f;
    m[i] = active ? mean[c0 + i] : 0.f;
  }
  // one row's vector: sum g, sum g * (x - mean); invstd scales the second sum once, after the dx pass's fold
  auto body = [&](const bu4& xv, const bu4& dv, const bu4& yv, int64_t off) {
    float xf[8], g[8];
    unpack8(xv, xf);
    unpack8(dv, g);
    if constexpr (RELU) relu_mask(g, yv);
    if constexpr (WRITE_G) st16(gout + off, pack8_exact(g));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sg[i] += g[i];
      sq[i] = fmaf(g[i], xf[i] - m[i], sq[i]);
    }
  };
  if (active) {
    const int64_t step = static_cast<int64_t>(ty) * C;
    int64_t r = r0 + ty_i;
    int64_t off = r * C + c0;
    for (; r + (kBnUnroll - 1) * ty < r1; r += kBnUnroll * ty, off += kBnUnroll * step) {
      bu4 xv[kBnUnroll], dv[kBnUnroll], yv[kBnUnroll] = {};
#pragma unroll
      for (int k = 0; k < kBnUnroll; ++k) {
        xv[k] = ld16<false>(x + off + k * step);  // read again by the dx pass
        dv[k] = ld16<GS_BN_NT && WRITE_G>(dy + off + k * step);
        if constexpr (RELU) yv[k] = ld16<GS_BN_NT && WRITE_G>(y + off + k * step);
      }
#pragma unroll
      for (int k = 0; k < kBnUnroll; ++k) body(xv[k], dv[k], yv[k], off + k * step);
    }
    for (; r < r1; r += ty, off += step) {
      bu4 yv = {0u, 0u, 0u, 0u};
      const bu4 xv = ld16<false>(x + off), dv = ld16<false>(dy + off);
      if constexpr (RELU) yv = ld16<false>(y + off);
      body(xv, dv, yv, off);
    }
  }
  // fold over the ty rows of the workgroup in a fixed order: 16 rows per thread, then the groups.
  // The folds here and in the dx pass add in fp64 (a few hundred adds per workgroup), so what is
  // left of the summation error is the threads' own fp32 accumulation over their rows.
  const int F = 16 << tx_log2;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s_red[t * 16 + 2 * i] = sg[i];
    s_red[t * 16 + 2 * i + 1] = sq[i];
  }
  __syncthreads();
  {
    const int o = t & (F - 1), grp = t >> (tx_log2 + 4);
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) a += static_cast<double>(s_red[(grp * 16 + k) * F + o]);
    s_grp[t] = a;
  }
  __syncthreads();
  if (t < F) {
    const int G = kBlock / F;
    double a = 0.0;
    for (int k = 0; k < G; ++k) a += s_grp[k * F + t];
    const int ch = blockIdx.x * (tx * 8) + (t >> 1);
    if (ch < C) ws[(static_cast<int64_t>(blockIdx.y) * C + ch) * 2 + (t & 1)] = static_cast<float>(a);
  }
}

// ---- pass 2: fold the partials, dx, and (row-block 0) grad_weight / grad_bias ----
template <bool RELU>
__global__ void __launch_bounds__(kBlock)
bn_bwd_dx_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
                 const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ weight,
                 const float* __restrict__ ws, int P, uint16_t* __restrict__ dx, float* __restrict__ gw,
                 float* __restrict__ gb, int64_t R, int C, int tx_log2, int64_t rpb, double inv_R) {
  __shared__ double s_fold[kBlock * 4];       // [groups][F4][4], F4 = 4 * tx float4 per partial row of the tile
  __shared__ double s_sum[16 * kBnTileVecs];  // [F]: (channel, {sum g, sum g*(x-mean)})
  const int t = threadIdx.x;
  const int tx = 1 << tx_log2, ty = kBlock >> tx_log2;
  const int tx_i = t & (tx - 1), ty_i = t >> tx_log2;
  const int tile_c0 = blockIdx.x * (tx * 8);
  {
    // thread (grp, q) adds float4 q of partials grp, grp + G4, ...; then the groups in order
    const int F4 = 4 << tx_log2, G4 = kBlock / F4;
    const int q = t & (F4 - 1), grp = t >> (tx_log2 + 2);
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (tile_c0 + 2 * q < C) {
      const bf4* base = reinterpret_cast<const bf4*>(ws + static_cast<int64_t>(tile_c0) * 2) + q;
      const int64_t stride = C >> 1;  // float4 per partial row
#pragma unroll 8
      for (int p = grp; p < P; p += G4) {
        const bf4 w4 = base[p * stride];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += static_cast<double>(w4[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s_fold[t * 4 + j] = a[j];
    __syncthreads();
    if (t < 4 * F4) {  // one (channel, sum) each
      double b = 0.0;
      for (int k = 0; k < G4; ++k) b += s_fold[k * 4 * F4 + t];
      s_sum[t] = b;
    }
    __syncthreads();
  }
  if (blockIdx.y == 0 && t < tx * 8 && tile_c0 + t < C) {
    gb[tile_c0 + t] = static_cast<float>(s_sum[2 * t]);
    gw[tile_c0 + t] = static_cast<float>(static_cast<double>(invstd[tile_c0 + t]) * s_sum[2 * t + 1]);
  }
  const int v = blockIdx.x * tx + tx_i;
  if (v >= (C >> 3)) return;
  const int c0 = v * 8;
  // dx = a * (g - m1 - (x - mean) * k2), a = w * invstd, m1 = sum g / R,
  // k2 = invstd * sum(g*xhat) / R = invstd^2 * sum(g*(x-mean)) / R
  float m[8], a[8], m1[8], k2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float is = invstd[c0 + i];
    m[i] = mean[c0 + i];
    a[i] = weight[c0 + i] * is;
    m1[i] = static_cast<float>(s_sum[tx_i * 16 + 2 * i] * inv_R);
    k2[i] = static_cast<float>(static_cast<double>(is) * is * s_sum[tx_i * 16 + 2 * i + 1] * inv_R);
  }
  auto body = [&](const bu4& xv, const bu4& dv, const bu4& yv, int64_t off) {
    float xf[8], g[8];
    unpack8(xv, xf);
    unpack8(dv, g);
    if constexpr (RELU) relu_mask(g, yv);
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = a[i] * fmaf(m[i] - xf[i], k2[i], g[i] - m1[i]);
    st16(dx + off, pack8_dx(g));
  };
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rpb;
  const int64_t r1 = std::min<int64_t>(R, r0 + rpb);
  const int64_t step = static_cast<int64_t>(ty) * C;
  int64_t r = r0 + ty_i;
  int64_t off = r * C + c0;
  for (; r + (kBnUnroll - 1) * ty < r1; r += kBnUnroll * ty, off += kBnUnroll * step) {
    bu4 xv[kBnUnroll], dv[kBnUnroll], yv[kBnUnroll] = {};
#pragma unroll
    for (int k = 0; k < kBnUnroll; ++k) {
      xv[k] = ld16<GS_BN_NT>(x + off + k * step);
      dv[k] = ld16<GS_BN_NT>(dy + off + k * step);
      if constexpr (RELU) yv[k] = ld16<GS_BN_NT>(y + off + k * step);
    }
#pragma unroll
    for (int k = 0; k < kBnUnroll; ++k) body(xv[k], dv[k], yv[k], off + k * step);
  }
  for (; r < r1; r += ty, off += step) {
    bu4 yv = {0u, 0u, 0u, 0u};
    const bu4 xv = ld16<false>(x + off), dv = ld16<false>(dy + off);
    if constexpr (RELU) yv = ld16<false>(y + off);
    body(xv, dv, yv, off);
  }
}

// ---- forward tail of a residual block: t = relu(t + identity), in place ----
// the sum in fp32 rounded once to bf16 (ATen's add_), then NaN ? NaN : max(., 0) (relu_ = clamp_min_)
__global__ void __launch_bounds__(kBlock)
add_relu_fwd_kernel(uint16_t* __restrict__ t, const uint16_t* __restrict__ id, int64_t nvec) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * (kBlock * kBnUnroll) + threadIdx.x;
  bu4 a[kBnUnroll], b[kBnUnroll];
#pragma unroll
  for (int k = 0; k < kBnUnroll; ++k) {
    const int64_t i = base + k * kBlock;
    if (i < nvec) {
      a[k] = ld16<false>(t + i * 8);
      b[k] = ld16<false>(id + i * 8);
    }
  }
#pragma unroll
  for (int k = 0; k < kBnUnroll; ++k) {
    const int64_t i = base + k * kBlock;
    if (i < nvec) {
      float af[8], bf[8];
      unpack8(a[k], af);
      unpack8(b[k], bf);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float s = __uint_as_float(to_bf16(af[j] + bf[j]) << 16);
        af[j] = s != s ? s : fmaxf(s, 0.f);
      }
      st16(t + i * 8, pack8_exact(af));
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_shape(int64_t R, int C) {
  GS_CHECK_ARG(R > 0 && C > 0 && C % 8 == 0, "bn: R > 0, C > 0 and C % 8 == 0 required");
  GS_CHECK_ARG(R <= (INT64_MAX / 4) / C, "bn: R * C too large");
  return GS_OK;
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" int gs_bn_bwd_partials(int64_t R, int C) {
  GS_TRY_RET(check_shape(R, C));
  return bn_geom(R, C).P;
}

extern "C" int gs_bn_bwd_reduce(const void* x, const void* dy, const void* y, void* g_out, const float* mean,
                                float* ws, int64_t ws_floats, int64_t R, int C, void* stream) {
  GS_TRY_RET(check_shape(R, C));
  GS_CHECK_ARG(x && dy && mean && ws, "gs_bn_bwd_reduce: null pointer");
  GS_CHECK_ARG(!g_out || y, "gs_bn_bwd_reduce: g_out needs y");
  GS_CHECK_ARG(aligned16(x) && aligned16(dy) && aligned16(y) && aligned16(g_out) && aligned16(ws),
               "gs_bn_bwd_reduce: pointers must be 16-byte aligned");
  const BnGeom g = bn_geom(R, C);
  GS_CHECK_ARG(ws_floats >= static_cast<int64_t>(g.P) * C * 2, "gs_bn_bwd_reduce: workspace too small");
  const dim3 grid(g.ctiles, g.P), block(kBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint16_t* dp = static_cast<const uint16_t*>(dy);
  const uint16_t* yp = static_cast<const uint16_t*>(y);
  uint16_t* gp = static_cast<uint16_t*>(g_out);
  if (gp)
    hipLaunchKernelGGL((bn_bwd_reduce_kernel<true, true>), grid, block, 0, s, xp, dp, yp, gp, mean, ws, R, C,
                       g.tx_log2, g.rpb);
  else if (yp)
    hipLaunchKernelGGL((bn_bwd_reduce_kernel<true, false>), grid, block, 0, s, xp, dp, yp, gp, mean, ws, R, C,
                       g.tx_log2, g.rpb);
  else
    hipLaunchKernelGGL((bn_bwd_reduce_kernel<false, false>), grid, block, 0, s, xp, dp, yp, gp, mean, ws, R, C,
                       g.tx_log2, g.rpb);
  HIP_RET(hipGetLastError());
  return GS_OK;
}

extern "C" int gs_bn_bwd_dx(const void* x, const void* dy, const void* y, const float* mean, const float* invstd,
                            const float* weight, const float* ws, int64_t ws_floats, void* dx, float* grad_weight,
                            float* grad_bias, int64_t R, int C, void* stream) {
  GS_TRY_RET(check_shape(R, C));
  GS_CHECK_ARG(x && dy && mean && invstd && weight && ws && dx && grad_weight && grad_bias,
               "gs_bn_bwd_dx: null pointer");
  GS_CHECK_ARG(aligned16(x) && aligned16(dy) && aligned16(y) && aligned16(dx) && aligned16(ws),
               "gs_bn_bwd_dx: pointers must be 16-byte aligned");
  const BnGeom g = bn_geom(R, C);
  GS_CHECK_ARG(ws_floats >= static_cast<int64_t>(g.P) * C * 2, "gs_bn_bwd_dx: workspace too small");
  const dim3 grid(g.ctiles, g.P), block(kBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint16_t* dp = static_cast<const uint16_t*>(dy);
  const uint16_t* yp = static_cast<const uint16_t*>(y);
  uint16_t* op = static_cast<uint16_t*>(dx);
  const double inv_R = 1.0 / static_cast<double>(R);
  if (yp)
    hipLaunchKernelGGL((bn_bwd_dx_kernel<true>), grid, block, 0, s, xp, dp, yp, mean, invstd, weight, ws, g.P, op,
                       grad_weight, grad_bias, R, C, g.tx_log2, g.rpb, inv_R);
  else
    hipLaunchKernelGGL((bn_bwd_dx_kernel<false>), grid, block, 0, s, xp, dp, yp, mean, invstd, weight, ws, g.P, op,
                       grad_weight, grad_bias, R, C, g.tx_log2, g.rpb, inv_R);
  HIP_RET(hipGetLastError());
  return GS_OK;
}

extern "C" int gs_add_relu_fwd(void* t, const void* identity, int64_t n, void* stream) {
  GS_CHECK_ARG(t && identity && n > 0 && n % 8 == 0, "gs_add_relu_fwd: n > 0, n % 8 == 0 and pointers required");
  GS_CHECK_ARG(aligned16(t) && aligned16(identity), "gs_add_relu_fwd: pointers must be 16-byte aligned");
  const int64_t nvec = n / 8;
  const int64_t blocks = (nvec + kBlock * kBnUnroll - 1) / (kBlock * kBnUnroll);
  GS_CHECK_ARG(blocks <= INT_MAX, "gs_add_relu_fwd: n too large");
  hipLaunchKernelGGL(add_relu_fwd_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), static_cast<uint16_t*>(t),
                     static_cast<const uint16_t*>(identity), nvec);
  HIP_RET(hipGetLastError());
  return GS_OK;
}
