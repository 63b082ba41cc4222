// gfx950 kernels of the NHWC BatchNorm backward fused with the ReLU mask and
// the residual add (include/gsync.h, gs_bn_bwd_reduce / gs_bn_bwd_dx /
// gs_add_relu_fwd).  They replace MIOpen's BatchNormBwdSpatial pair plus ATen's
// threshold_backward, and the in-place add + ReLU at the end of a residual block.
//
// An activation is a row-major [R, C] bf16 matrix.  A thread owns 8 consecutive
// channels (one 16-B access) and walks down the rows; a workgroup of the backward
// passes is tx x ty threads over a channel tile of tx vectors (tx = 32 from C = 256
// on: 512 contiguous bytes of a row, a wave covers 2 rows) and ty = max(32, 256 / tx)
// rows per step: 256 threads up to C = 64, 512 at C = 128, 1024 from C = 256 on
// (bn_geom halves the tile where so large a workgroup would leave CUs without one).
// The grid is (channel tiles, P row-blocks): wide layers fill the chip from the
// channel axis, the stem and layer1 from the row axis (bn_geom).
//
// HBM-bound streaming, passes over the activation per BN backward:
//   reduce: x, dy (, y) in (, g out)         dx: x, dy|g (, y) in, dx out
// The per-channel sums (of g and of g * (x - mean)) cross workgroups through a [P, C, 2] fp32 workspace:
// every reduce workgroup stores its partial, every dx workgroup folds the P
// partials of its own channel tile in a fixed order (L2-served, P*P*8 / (6*R) of
// the streamed bytes, bounded by bn_geom) - the folded-partials idiom of the
// clipped update in gs_update_kernels.hip.  No atomics, so the result is
// deterministic.
//
// gs_bn_bwd_reduce_fork is the reduce pass fed the two halves of a fork's gradient
// (one more stream in, ATen's bf16 add in registers).  The stem's tail has its own
// pair: relu_maxpool_fwd_kernel (ReLU taken while pooling, a byte per output for
// the winner) and maxpool_bwd_kernel (dx written once from those bytes).
//
// The *_bits / *_mask entries move the ReLU mask as one bit per element instead of the bf16 y: the forward
// tails (relu, add + relu, the stem's pool) write one byte per 16-B vector while they hold it, the backward
// passes load that byte where they loaded the vector of y (2 B an element become 0.125 B).
//
// Inference (gs_bn_infer_act, gs_bn_infer_relu_maxpool): a BatchNorm in evaluation is a per-channel
// affine map, so BatchNorm + add + ReLU is one pass on the same (channel tile x row-block) grid: a thread
// forms s and t of its 8 channels once from the running statistics and streams rows, kBnUnroll in flight.
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

// Vectors (of 8 channels) per channel tile of the backward passes, at most: 8, 16 or 32.  A workgroup
// touches tx * 16 contiguous bytes of a row and rows lie 2 C bytes apart; 512 bytes stream faster than
// 128.  -DGS_BN_TILE_VECS=8 rebuilds the 8-vector tile in 256-thread workgroups.
#ifndef GS_BN_TILE_VECS
#define GS_BN_TILE_VECS 32
#endif
constexpr int kBnTileVecs = GS_BN_TILE_VECS;
static_assert(kBnTileVecs == 8 || kBnTileVecs == 16 || kBnTileVecs == 32, "GS_BN_TILE_VECS: 8, 16 or 32");
constexpr int kBnMinRows = 32;         // rows per workgroup step, at least: bounds a thread's fp32 chain
constexpr int kBnMaxP = 512;           // row-blocks, at most
constexpr int kBnTargetBlocks = 1024;  // 4 workgroups of 256 threads per CU, or as many waves in larger ones
constexpr int kBnUnroll = 4;           // rows in flight per thread and stream
#ifndef GS_BN_FORK_UNROLL
#define GS_BN_FORK_UNROLL 4
#endif
constexpr int kBnForkUnroll = GS_BN_FORK_UNROLL;  // the same, for the reduce that sums two gradients

// The decomposition of (R, C), the same for both backward kernels.
//   P <= ceil(R / ty): a row-block has at least one step of rows;
//   P <= sqrt(R / 2): the fold (P * P * 8 bytes per channel) stays under half the
//        bytes streamed (R * 6 per channel), and it is read from L2;
//   units * P near kBnTargetBlocks, units = tiles * (threads / 256) the workgroups of a row-block counted
//        in 256 threads: the resident waves do not depend on the tile's width (a 32-vector tile has a
//        quarter of the 8-vector tiles, in workgroups four times as large, so P is what the 8-vector
//        tile gave wherever C / 8 is a power of two);
//   units * P a multiple of 256 CUs where it exceeds them.
// The tile: tx = min(kBnTileVecs, pow2ceil(C / 8)) vectors, halved (not below 8) while the grid has fewer
// workgroups than the 256 CUs although every thread has an unrolled step of rows to stream: a 1024-thread
// workgroup is alone on its CU, so 128 of them leave half the chip idle, and P cannot grow past sqrt(R / 2)
// (50176 x 256 and 12544 x 512 of ResNet-50 x 256 run 256 workgroups of a 16-vector tile: DESIGN §3e).
struct BnGeom {
  int tx_log2;
  int ctiles;
  int P;
  int64_t rpb;         // rows per row-block
  int block = kBlock;  // threads per workgroup: tx * ty
};

BnGeom bn_geom_tile(int64_t R, int C, int l2) {
  const int V = C / 8;
  const int tx = 1 << l2, ty = std::max(kBnMinRows, kBlock / tx);
  const int block = tx * ty;  // 256 up to tx = 8, then 512, 1024
  const int64_t ctiles = (V + tx - 1) / tx;
  int64_t P = std::min<int64_t>(kBnMaxP, (R + ty - 1) / ty);
  P = std::min<int64_t>(P, static_cast<int64_t>(std::sqrt(0.5 * static_cast<double>(R))));
  const int64_t units = ctiles * (block / kBlock);
  P = std::min<int64_t>(P, kBnTargetBlocks / units);
  P = std::max<int64_t>(P, 1);
  if (units * P > 256) {
    const int64_t step = 256 / std::min<int64_t>(256, units & -units);
    if (P >= step) P -= P % step;
  }
  const int64_t rpb = (R + P - 1) / P;
  P = (R + rpb - 1) / rpb;  // no empty row-block
  return BnGeom{l2, static_cast<int>(ctiles), static_cast<int>(P), rpb, block};
}

BnGeom bn_geom(int64_t R, int C) {
  const int V = C / 8;
  int l2 = 0;
  while ((1 << l2) < V && (1 << l2) < kBnTileVecs) ++l2;
  BnGeom g = bn_geom_tile(R, C, l2);
  while (l2 > 3 && static_cast<int64_t>(g.ctiles) * g.P < 256 && g.rpb >= kBnUnroll * kBnMinRows)
    g = bn_geom_tile(R, C, --l2);
  return g;
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

// Where the ReLU mask comes from: nowhere, the saved bf16 output y, or one bit per element
// (byte i of the mask belongs to the 16-B vector i, bit j set iff !(v[8 i + j] <= 0)).
enum : int { kMaskNone = 0, kMaskY = 1, kMaskBits = 2 };

// the same g from the vector's mask byte: a cleared bit gives +0, a set bit passes dy
__device__ __forceinline__ void relu_mask_bits(float (&g)[8], uint32_t mb) {
#pragma unroll
  for (int i = 0; i < 8; ++i) g[i] = (mb >> i) & 1u ? g[i] : 0.f;
}

// the mask byte of 8 values: bit j = !(f[j] <= 0), relu_mask()'s predicate (a NaN sets it, +-0 clear it)
__device__ __forceinline__ uint8_t mask_byte(const float (&f)[8]) {
  uint32_t mb = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) mb |= (f[j] <= 0.f ? 0u : 1u) << j;
  return static_cast<uint8_t>(mb);
}

// dy = dy_a + dy_b as ATen's bf16 add forms it: the sum in fp32, rounded once to bf16
__device__ __forceinline__ void fork_sum(float (&g)[8], const bu4& bv) {
  float b[8];
  unpack8(bv, b);
#pragma unroll
  for (int i = 0; i < 8; ++i) g[i] = __uint_as_float(to_bf16(g[i] + b[i]) << 16);
}

// ---- pass 1: per-workgroup partial sums of g and g * xhat (and g itself) ----
// FORK: the gradient arrives as the two halves of a fork (dy, dy2) and is summed here
// MASK: kMaskY reads y, kMaskBits one byte of mask per vector where kMaskY loads the vector of y
// The plain reduce from bits is asked for 5 waves per SIMD, what the same pass from y has: it reaches them at
// 96 VGPRs without scratch, and lands a few registers above without the bound.
// BLOCK = tx * ty threads (bn_geom): a 1024-thread workgroup is 4 waves per SIMD, 128 VGPRs at most, and
// the only one on its CU; its 72 KiB of LDS are under gfx950's 160 KiB per workgroup.
template <int BLOCK, int MASK, bool WRITE_G, bool FORK>
__global__ void __launch_bounds__(BLOCK, (BLOCK == kBlock && MASK == kMaskBits && !WRITE_G) ? 5 : 1)
bn_bwd_reduce_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy, const uint16_t* __restrict__ dy2,
                     const uint16_t* __restrict__ y, const uint8_t* __restrict__ mask, uint16_t* __restrict__ gout,
                     const float* __restrict__ mean, float* __restrict__ ws, int64_t R, int C, int tx_log2,
                     int64_t rpb) {
  constexpr int U = FORK ? kBnForkUnroll : kBnUnroll;
  __shared__ float s_red[BLOCK * 16];  // [ty][F], F = 16 * tx: (channel, {sum g, sum g*(x-mean)})
  __shared__ double s_grp[BLOCK];      // [ty / 16][F]
  const int t = threadIdx.x;
  const int tx = 1 << tx_log2, ty = BLOCK >> tx_log2;
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
  auto body = [&](const bu4& xv, const bu4& dv, const bu4& bv, const bu4& yv, uint32_t mb, int64_t off) {
    float xf[8], g[8];
    unpack8(xv, xf);
    unpack8(dv, g);
    if constexpr (FORK) fork_sum(g, bv);
    if constexpr (MASK == kMaskY) relu_mask(g, yv);
    if constexpr (MASK == kMaskBits) relu_mask_bits(g, mb);
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
    for (; r + (U - 1) * ty < r1; r += U * ty, off += U * step) {
      bu4 xv[U], dv[U], bv[U] = {}, yv[U] = {};
      uint32_t mb[U] = {};
#pragma unroll
      for (int k = 0; k < U; ++k) {
        xv[k] = ld16<false>(x + off + k * step);  // read again by the dx pass
        dv[k] = ld16<GS_BN_NT && WRITE_G>(dy + off + k * step);
        if constexpr (FORK) bv[k] = ld16<GS_BN_NT>(dy2 + off + k * step);
        if constexpr (MASK == kMaskY) yv[k] = ld16<GS_BN_NT && WRITE_G>(y + off + k * step);
        if constexpr (MASK == kMaskBits) mb[k] = mask[(off + k * step) >> 3];
      }
      // every load of the step is issued before its first use: left to itself the scheduler trades the loads
      // in flight for registers here (one load, one wait), which costs more than the mask saves
      if constexpr (MASK == kMaskBits) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < U; ++k) body(xv[k], dv[k], bv[k], yv[k], mb[k], off + k * step);
    }
    for (; r < r1; r += ty, off += step) {
      bu4 bv = {0u, 0u, 0u, 0u}, yv = {0u, 0u, 0u, 0u};
      uint32_t mb = 0;
      const bu4 xv = ld16<false>(x + off), dv = ld16<false>(dy + off);
      if constexpr (FORK) bv = ld16<false>(dy2 + off);
      if constexpr (MASK == kMaskY) yv = ld16<false>(y + off);
      if constexpr (MASK == kMaskBits) mb = mask[off >> 3];
      body(xv, dv, bv, yv, mb, off);
    }
  }
  // fold over the ty rows of the workgroup in a fixed order: 16 rows per thread, then the groups
  // (ty is a multiple of 16 and F = 16 * tx <= BLOCK for every tx: ty / 16 groups of F threads).
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
    const int G = BLOCK / F;
    double a = 0.0;
    for (int k = 0; k < G; ++k) a += s_grp[k * F + t];
    const int ch = blockIdx.x * (tx * 8) + (t >> 1);
    if (ch < C) ws[(static_cast<int64_t>(blockIdx.y) * C + ch) * 2 + (t & 1)] = static_cast<float>(a);
  }
}

// ---- pass 2: fold the partials, dx, and (row-block 0) grad_weight / grad_bias ----
template <int BLOCK, int MASK>
__global__ void __launch_bounds__(BLOCK)
bn_bwd_dx_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
                 const uint8_t* __restrict__ mask, const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ weight,
                 const float* __restrict__ ws, int P, uint16_t* __restrict__ dx, float* __restrict__ gw,
                 float* __restrict__ gb, int64_t R, int C, int tx_log2, int64_t rpb, double inv_R) {
  __shared__ double s_fold[BLOCK * 4];        // [groups][F4][4], F4 = 4 * tx float4 per partial row of the tile
  __shared__ double s_sum[BLOCK / 2];         // [F]: (channel, {sum g, sum g*(x-mean)}), F = 16 * tx <= BLOCK / 2
  const int t = threadIdx.x;
  const int tx = 1 << tx_log2, ty = BLOCK >> tx_log2;
  const int tx_i = t & (tx - 1), ty_i = t >> tx_log2;
  const int tile_c0 = blockIdx.x * (tx * 8);
  {
    // thread (grp, q) adds float4 q of partials grp, grp + G4, ...; then the groups in order
    // (G4 = ty / 4 groups of F4 threads; the second round's 4 * F4 = 16 * tx threads are at most half of BLOCK)
    const int F4 = 4 << tx_log2, G4 = BLOCK / F4;
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
  auto body = [&](const bu4& xv, const bu4& dv, const bu4& yv, uint32_t mb, int64_t off) {
    float xf[8], g[8];
    unpack8(xv, xf);
    unpack8(dv, g);
    if constexpr (MASK == kMaskY) relu_mask(g, yv);
    if constexpr (MASK == kMaskBits) relu_mask_bits(g, mb);
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
    uint32_t mb[kBnUnroll] = {};
#pragma unroll
    for (int k = 0; k < kBnUnroll; ++k) {
      xv[k] = ld16<GS_BN_NT>(x + off + k * step);
      dv[k] = ld16<GS_BN_NT>(dy + off + k * step);
      if constexpr (MASK == kMaskY) yv[k] = ld16<GS_BN_NT>(y + off + k * step);
      if constexpr (MASK == kMaskBits) mb[k] = mask[(off + k * step) >> 3];
    }
    if constexpr (MASK == kMaskBits) __builtin_amdgcn_sched_barrier(0);  // as in the reduce pass
#pragma unroll
    for (int k = 0; k < kBnUnroll; ++k) body(xv[k], dv[k], yv[k], mb[k], off + k * step);
  }
  for (; r < r1; r += ty, off += step) {
    bu4 yv = {0u, 0u, 0u, 0u};
    uint32_t mb = 0;
    const bu4 xv = ld16<false>(x + off), dv = ld16<false>(dy + off);
    if constexpr (MASK == kMaskY) yv = ld16<false>(y + off);
    if constexpr (MASK == kMaskBits) mb = mask[off >> 3];
    body(xv, dv, yv, mb, off);
  }
}

// relu_ (= clamp_min_(0)): a NaN stays, everything not above 0 (-0 too) becomes +0
__device__ __forceinline__ float relu1(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }

// ---- forward tail of a residual block: t = relu(t + identity), in place ----
// the sum in fp32 rounded once to bf16 (ATen's add_), then NaN ? NaN : max(., 0) (relu_ = clamp_min_)
// ADD = false: the tail of a plain BatchNorm + ReLU, t = relu(t) as relu_ forms it (relu1).
// MASK: the mask byte of every vector of the result is written as well (the backward's kMaskBits).
template <bool ADD, bool MASK>
__global__ void __launch_bounds__(kBlock)
add_relu_fwd_kernel(uint16_t* __restrict__ t, const uint16_t* __restrict__ id, uint8_t* __restrict__ mask,
                    int64_t nvec) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * (kBlock * kBnUnroll) + threadIdx.x;
  bu4 a[kBnUnroll], b[kBnUnroll] = {};
#pragma unroll
  for (int k = 0; k < kBnUnroll; ++k) {
    const int64_t i = base + k * kBlock;
    if (i < nvec) {
      a[k] = ld16<false>(t + i * 8);
      if constexpr (ADD) b[k] = ld16<false>(id + i * 8);
    }
  }
#pragma unroll
  for (int k = 0; k < kBnUnroll; ++k) {
    const int64_t i = base + k * kBlock;
    if (i < nvec) {
      float af[8];
      unpack8(a[k], af);
      if constexpr (ADD) {
        float bf[8];
        unpack8(b[k], bf);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float s = __uint_as_float(to_bf16(af[j] + bf[j]) << 16);
          af[j] = s != s ? s : fmaxf(s, 0.f);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) af[j] = relu1(af[j]);
      }
      st16(t + i * 8, pack8_exact(af));
      if constexpr (MASK) mask[i] = mask_byte(af);
    }
  }
}

// ---- the stem: ReLU + MaxPool2d(3, 2, 1) forward, and the pool's backward ----
// NHWC bf16, a thread owns 8 channels of one pixel (C = 64: one 128-B line per pixel, 8 threads).
// Window of output (oh, ow): rows 2 oh - 1 .. 2 oh + 1, columns 2 ow - 1 .. 2 ow + 1, clipped.

// pooled = max over the window of relu(y), idx = the winner's position 3 * kh + kw in the unclipped
// window.  Scanned rows outer, columns inner; a later value wins only if it is > the current one or
// is NaN (ATen's max_pool_forward_nhwc): ties keep the first, the last NaN of the window wins.
// MASK: window positions 4, 5, 7, 8 are the 2 x 2 quad of input pixels (2 oh + dh, 2 ow + dw); the quads
// partition the input, so the thread writes those pixels' mask bytes (of the un-ReLU'd y) exactly once.
template <bool MASK>
__global__ void __launch_bounds__(kBlock)
relu_maxpool_fwd_kernel(const uint16_t* __restrict__ y, uint16_t* __restrict__ pooled, uint8_t* __restrict__ idx,
                        uint8_t* __restrict__ mask, int64_t nvec, int H, int W, int OH, int OW, int V) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= nvec) return;
  const int cv = static_cast<int>(i % V);
  int64_t p = i / V;
  const int ow = static_cast<int>(p % OW);
  p /= OW;
  const int oh = static_cast<int>(p % OH);
  const int64_t n = p / OH;
  const int h0 = 2 * oh - 1, w0 = 2 * ow - 1;
  const int64_t C = static_cast<int64_t>(V) * 8;
  bu4 in[9];
  bool ok[9];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int ih = h0 + kh, iw = w0 + kw, k = 3 * kh + kw;
      ok[k] = ih >= 0 && ih < H && iw >= 0 && iw < W;
      in[k] = bu4{0u, 0u, 0u, 0u};
      if (ok[k]) in[k] = ld16<false>(y + ((n * H + ih) * W + iw) * C + cv * 8);
    }
  }
  float best[8];
  uint32_t code[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    best[j] = -INFINITY;
    code[j] = 0;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float f[8];
    unpack8(in[k], f);
    if constexpr (MASK) {
      if ((k == 4 || k == 5 || k == 7 || k == 8) && ok[k])
        mask[((n * H + h0 + k / 3) * W + w0 + k % 3) * V + cv] = mask_byte(f);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = relu1(f[j]);
      const bool take = ok[k] && (v > best[j] || v != v);  // relu(v) >= 0 > -inf: the first valid one is taken
      best[j] = take ? v : best[j];
      code[j] = take ? static_cast<uint32_t>(k) : code[j];
    }
  }
  st16(pooled + i * 8, pack8_exact(best));
  uint2 c;
  c.x = code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24);
  c.y = code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24);
  *reinterpret_cast<uint2*>(idx + i * 8) = c;
}

// dx of the pool for every input element: the gradients of the (at most 4) windows that contain it and
// name it their winner, windows visited rows outer, columns inner, ascending; added in fp32 from +0 and
// rounded once to bf16.  An element inside a single window takes that window's gradient as it is (a -0
// stays -0), as ATen's max_pool_backward_nhwc does; a 1 x 1 image is NCHW-contiguous as well, ATen runs
// its NCHW kernel on it, and that one adds to +0.  FORK: a window's gradient is bf16(dA + dB).
// A thread owns 8 channels of the 2 x 2 input pixels (2a + dh, 2b + dw): the windows that contain them are
// (a + al, b + be), al <= dh, be <= dw, where pixel (dh, dw) sits at position 3 (dh + 1 - 2 al) + (dw + 1 - 2 be);
// the four windows' bytes and gradients are read once for the four pixels.
template <bool FORK>
__global__ void __launch_bounds__(kBlock)
maxpool_bwd_kernel(const uint16_t* __restrict__ da, const uint16_t* __restrict__ db, const uint8_t* __restrict__ idx,
                   uint16_t* __restrict__ dx, int64_t nquad, int H, int W, int OH, int OW, int V) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= nquad) return;  // the quads are as many as the windows: (H + 1) / 2 = OH, (W + 1) / 2 = OW
  const int cv = static_cast<int>(i % V);
  int64_t p = i / V;
  const int b = static_cast<int>(p % OW);
  p /= OW;
  const int a = static_cast<int>(p % OH);
  const int64_t n = p / OH;
  const bool more_h = a + 1 < OH, more_w = b + 1 < OW;
  uint2 cw[4];
  int64_t ovec[4];
  bool ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int al = k >> 1, be = k & 1;
    ok[k] = (al == 0 || more_h) && (be == 0 || more_w);
    ovec[k] = ((n * OH + a + al) * OW + b + be) * V + cv;
    cw[k] = uint2{0xffffffffu, 0xffffffffu};  // no position is 255
    if (ok[k]) cw[k] = *reinterpret_cast<const uint2*>(idx + ovec[k] * 8);
  }
  // a byte of w equal to c?  (a zero byte of w ^ cccc)
  auto has = [](const uint2& w, uint32_t c) {
    const uint32_t x0 = w.x ^ (c * 0x01010101u), x1 = w.y ^ (c * 0x01010101u);
    return ((((x0 - 0x01010101u) & ~x0) | ((x1 - 0x01010101u) & ~x1)) & 0x80808080u) != 0;
  };
  bool hit[4];
  hit[0] = true;  // positions 4, 5, 7, 8 of window (a, b): nearly always one of the 8 channels
  hit[1] = ok[1] && (has(cw[1], 3u) || has(cw[1], 6u));
  hit[2] = ok[2] && (has(cw[2], 1u) || has(cw[2], 2u));
  hit[3] = ok[3] && has(cw[3], 0u);
  bu4 av[4], bv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    av[k] = bv[k] = bu4{0u, 0u, 0u, 0u};
    if (hit[k]) {
      av[k] = ld16<false>(da + ovec[k] * 8);
      if constexpr (FORK) bv[k] = ld16<false>(db + ovec[k] * 8);
    }
  }
  const bool many = H * W > 1;
  float acc[4][8];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[q][j] = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int al = k >> 1, be = k & 1;
    float g[8];
    unpack8(av[k], g);
    if constexpr (FORK) fork_sum(g, bv[k]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int dh = q >> 1, dw = q & 1;
      if (dh < al || dw < be) continue;  // compile-time: the window does not contain the pixel
      const uint32_t want = static_cast<uint32_t>(3 * (dh + 1 - 2 * al) + (dw + 1 - 2 * be));
      // the pixel's windows: 1 + [dh and a row of windows below] times 1 + [dw and a column to the right]
      const bool single = many && !(dh == 1 && more_h) && !(dw == 1 && more_w);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t cj = ((j < 4 ? cw[k].x : cw[k].y) >> (8 * (j & 3))) & 0xffu;
        const bool m = hit[k] && cj == want;
        acc[q][j] = m ? (single ? g[j] : acc[q][j] + g[j]) : acc[q][j];
      }
    }
  }
  const int64_t C = static_cast<int64_t>(V) * 8;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ih = 2 * a + (q >> 1), iw = 2 * b + (q & 1);
    if (ih < H && iw < W) {
      bu4 out;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[r] = to_bf16(acc[q][2 * r]) | (to_bf16(acc[q][2 * r + 1]) << 16);
      st16(dx + ((n * H + ih) * W + iw) * C + cv * 8, out);
    }
  }
}

// ---- inference: BatchNorm as a per-channel affine map (+ residual add) (+ ReLU), one pass ----
// The decomposition of (R, C) for a pass with no cross-workgroup sums: bn_geom's channel tiles, and
// as many row-blocks as give every thread at least one unrolled step, up to kBnInferBlocks workgroups.
constexpr int kBnInferBlocks = 2048;  // 8 workgroups per CU
// Vectors per channel tile of the inference kernels, at most (a power of two): a workgroup touches
// tx * 16 contiguous bytes of a row.  With no per-tile sums to fold a wide tile costs nothing, and 512
// contiguous bytes instead of bn_geom's 128 stream 5 to 15 % faster at C = 256 .. 1024.
#ifndef GS_BN_INFER_TILE_VECS
#define GS_BN_INFER_TILE_VECS 32
#endif
constexpr int kBnInferTileVecs = GS_BN_INFER_TILE_VECS;

BnGeom bn_infer_geom(int64_t R, int C) {
  const int V = C / 8;
  int l2 = 0;
  while ((1 << l2) < V && (1 << l2) < kBnInferTileVecs) ++l2;
  const int tx = 1 << l2, ty = kBlock / tx;
  const int64_t ctiles = (V + tx - 1) / tx;
  const int64_t per = static_cast<int64_t>(ty) * kBnUnroll;
  int64_t P = std::min<int64_t>((R + per - 1) / per, std::max<int64_t>(1, kBnInferBlocks / ctiles));
  P = std::max<int64_t>(P, 1);
  const int64_t rpb = (R + P - 1) / P;
  P = (R + rpb - 1) / rpb;  // no empty row-block
  return BnGeom{l2, static_cast<int>(ctiles), static_cast<int>(P), rpb};
}

// s = weight / sqrt(var + eps), t = bias - mean * s of 8 channels, in the order include/gsync.h fixes
__device__ __forceinline__ void infer_affine(const float* __restrict__ rm, const float* __restrict__ rv,
                                             const float* __restrict__ w, const float* __restrict__ b, float eps,
                                             int c0, float (&s)[8], float (&t)[8]) {
  const bf4 m0 = *reinterpret_cast<const bf4*>(rm + c0), m1 = *reinterpret_cast<const bf4*>(rm + c0 + 4);
  const bf4 v0 = *reinterpret_cast<const bf4*>(rv + c0), v1 = *reinterpret_cast<const bf4*>(rv + c0 + 4);
  const bf4 w0 = *reinterpret_cast<const bf4*>(w + c0), w1 = *reinterpret_cast<const bf4*>(w + c0 + 4);
  const bf4 b0 = *reinterpret_cast<const bf4*>(b + c0), b1 = *reinterpret_cast<const bf4*>(b + c0 + 4);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float m = i < 4 ? m0[i & 3] : m1[i & 3], v = i < 4 ? v0[i & 3] : v1[i & 3];
    const float wi = i < 4 ? w0[i & 3] : w1[i & 3], bi = i < 4 ? b0[i & 3] : b1[i & 3];
    s[i] = wi * (1.0f / sqrtf(v + eps));
    t[i] = fmaf(-m, s[i], bi);
  }
}

__device__ __forceinline__ bu4 pack8_rne(const float (&f)[8]) {
  bu4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = to_bf16(f[2 * i]) | (to_bf16(f[2 * i + 1]) << 16);
  return v;
}

// y = bf16(relu(fma(x, s, t) + r)), rounded once.  y may be x: a thread reads and writes its own elements only,
// every load of an unrolled step before its stores (no __restrict__ on the pair).
template <bool RES, bool RELU>
__global__ void __launch_bounds__(kBlock)
bn_infer_act_kernel(const uint16_t* x, const uint16_t* __restrict__ res, const float* __restrict__ rm,
                    const float* __restrict__ rv, const float* __restrict__ w, const float* __restrict__ b, float eps,
                    uint16_t* y, int64_t R, int C, int tx_log2, int64_t rpb) {
  const int t_ = threadIdx.x;
  const int tx = 1 << tx_log2, ty = kBlock >> tx_log2;
  const int tx_i = t_ & (tx - 1), ty_i = t_ >> tx_log2;
  const int v = blockIdx.x * tx + tx_i;
  if (v >= (C >> 3)) return;
  const int c0 = v * 8;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rpb;
  const int64_t r1 = std::min<int64_t>(R, r0 + rpb);
  const int64_t step = static_cast<int64_t>(ty) * C;
  int64_t r = r0 + ty_i;
  int64_t off = r * C + c0;
  float s[8], t[8];
  infer_affine(rm, rv, w, b, eps, c0, s, t);
  auto body = [&](const bu4& xv, const bu4& rvv, int64_t off) {
    float f[8], r[8];
    unpack8(xv, f);
    if constexpr (RES) unpack8(rvv, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float a = fmaf(f[i], s[i], t[i]);
      if constexpr (RES) a = a + r[i];
      if constexpr (RELU) a = relu1(a);
      f[i] = a;
    }
    st16(y + off, pack8_rne(f));
  };
  for (; r + (kBnUnroll - 1) * ty < r1; r += kBnUnroll * ty, off += kBnUnroll * step) {
    bu4 xv[kBnUnroll], rr[kBnUnroll] = {};
#pragma unroll
    for (int k = 0; k < kBnUnroll; ++k) {
      xv[k] = ld16<GS_BN_NT>(x + off + k * step);
      if constexpr (RES) rr[k] = ld16<false>(res + off + k * step);  // the identity: the next block reads it again
    }
#pragma unroll
    for (int k = 0; k < kBnUnroll; ++k) body(xv[k], rr[k], off + k * step);
  }
  for (; r < r1; r += ty, off += step) {
    bu4 rr = {0u, 0u, 0u, 0u};
    const bu4 xv = ld16<false>(x + off);
    if constexpr (RES) rr = ld16<false>(res + off);
    body(xv, rr, off);
  }
}

// the stem in inference: pooled = MaxPool2d(3, 2, 1)(bf16(relu(fma(x, s, t)))).  A thread keeps its 8 channels
// and strides over output pixels (rows of the [N * OH * OW, C] output), nine 16-B loads in flight per pixel;
// window, scan order and NaN rule are relu_maxpool_fwd_kernel's.
__global__ void __launch_bounds__(kBlock)
bn_infer_relu_maxpool_kernel(const uint16_t* __restrict__ x, const float* __restrict__ rm,
                             const float* __restrict__ rv, const float* __restrict__ w, const float* __restrict__ b,
                             float eps, uint16_t* __restrict__ pooled, int64_t OR, int H, int W, int OH, int OW, int C,
                             int tx_log2, int64_t rpb) {
  const int t_ = threadIdx.x;
  const int tx = 1 << tx_log2, ty = kBlock >> tx_log2;
  const int tx_i = t_ & (tx - 1), ty_i = t_ >> tx_log2;
  const int v = blockIdx.x * tx + tx_i;
  if (v >= (C >> 3)) return;
  const int c0 = v * 8;
  float s[8], t[8];
  infer_affine(rm, rv, w, b, eps, c0, s, t);
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rpb;
  const int64_t r1 = std::min<int64_t>(OR, r0 + rpb);
  for (int64_t p = r0 + ty_i; p < r1; p += ty) {
    const int ow = static_cast<int>(p % OW);
    const int64_t q = p / OW;
    const int oh = static_cast<int>(q % OH);
    const int64_t n = q / OH;
    const int h0 = 2 * oh - 1, w0 = 2 * ow - 1;
    bu4 in[9];
    bool ok[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ih = h0 + kh, iw = w0 + kw, k = 3 * kh + kw;
        ok[k] = ih >= 0 && ih < H && iw >= 0 && iw < W;
        in[k] = bu4{0u, 0u, 0u, 0u};
        if (ok[k]) in[k] = ld16<false>(x + ((n * H + ih) * W + iw) * C + c0);
      }
    }
    float best[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) best[j] = -INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      float f[8];
      unpack8(in[k], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a = __uint_as_float(to_bf16(relu1(fmaf(f[j], s[j], t[j]))) << 16);
        const bool take = ok[k] && (a > best[j] || a != a);  // relu(.) >= 0 > -inf: the first valid one is taken
        best[j] = take ? a : best[j];
      }
    }
    st16(pooled + p * C + c0, pack8_exact(best));
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

namespace gs {
namespace {

// [p, p + pbytes) and [q, q + qbytes) share a byte (a null pointer overlaps nothing)
bool overlap(const void* p, int64_t pbytes, const void* q, int64_t qbytes) {
  if (!p || !q) return false;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + static_cast<uintptr_t>(qbytes) && b < a + static_cast<uintptr_t>(pbytes);
}
bool overlap(const void* p, const void* q, int64_t bytes) { return overlap(p, bytes, q, bytes); }

// MaxPool2d(3, 2, 1) over [N, H, W, C]: the output's height and width, and the shape checks of both entries
struct PoolGeom {
  int OH, OW;
  int64_t in_vecs, out_vecs;  // vectors of 8 channels
};

int pool_geom(const std::string& w, int64_t N, int H, int W, int C, PoolGeom* g) {
  GS_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, w + ": N, H, W, C > 0 and C % 8 == 0 required");
  GS_CHECK_ARG(N <= ((INT64_MAX / 4) / C / H) / W, w + ": N * H * W * C too large");
  g->OH = (H - 1) / 2 + 1;
  g->OW = (W - 1) / 2 + 1;
  g->in_vecs = N * H * W * (C / 8);
  g->out_vecs = N * g->OH * g->OW * (C / 8);
  GS_CHECK_ARG((g->in_vecs + kBlock - 1) / kBlock <= INT_MAX, w + ": N * H * W * C too large");
  return GS_OK;
}

// dy_b != NULL: the fork form (g_out required); the checks of all four entries.  bits: the mask comes
// from `mask` (R * C / 8 bytes, any alignment, required) and y is NULL.
int bn_reduce(const char* who, const void* x, const void* dy, const void* dy_b, const void* y, bool bits,
              const void* mask, void* g_out, const float* mean, float* ws, int64_t ws_floats, int64_t R, int C,
              void* stream) {
  const std::string w(who);
  GS_TRY_RET(check_shape(R, C));
  GS_CHECK_ARG(x && dy && mean && ws && (!bits || mask), w + ": null pointer");
  GS_CHECK_ARG(!g_out || y || mask || dy_b, w + ": g_out needs y");
  GS_CHECK_ARG(!dy_b || g_out, w + ": two gradients need g_out");
  GS_CHECK_ARG(aligned16(x) && aligned16(dy) && aligned16(dy_b) && aligned16(y) && aligned16(g_out) && aligned16(ws),
               w + ": pointers must be 16-byte aligned");
  if (dy_b) {
    const int64_t bytes = R * C * 2;
    GS_CHECK_ARG(!overlap(g_out, x, bytes) && !overlap(g_out, dy, bytes) && !overlap(g_out, dy_b, bytes) &&
                     !overlap(g_out, y, bytes),
                 w + ": g_out overlaps an input");
  }
  GS_CHECK_ARG(!overlap(g_out, R * C * 2, mask, R * C / 8), w + ": g_out overlaps the mask");
  const BnGeom g = bn_geom(R, C);
  GS_CHECK_ARG(ws_floats >= static_cast<int64_t>(g.P) * C * 2, w + ": workspace too small");
  const dim3 grid(g.ctiles, g.P), block(g.block);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint16_t* dp = static_cast<const uint16_t*>(dy);
  const uint16_t* bp = static_cast<const uint16_t*>(dy_b);
  const uint16_t* yp = static_cast<const uint16_t*>(y);
  const uint8_t* mp = static_cast<const uint8_t*>(mask);
  uint16_t* gp = static_cast<uint16_t*>(g_out);
  // the workgroup size follows the tile (bn_geom); the sizes kBnTileVecs rules out are not compiled
#define GS_BN_REDUCE_B(BLOCK, MASK, WRITE_G, FORK)                                                                    \
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<BLOCK, MASK, WRITE_G, FORK>), grid, block, 0, s, xp, dp, bp, yp, mp, gp, \
                     mean, ws, R, C, g.tx_log2, g.rpb)
#define GS_BN_REDUCE(MASK, WRITE_G, FORK)                                 \
  do {                                                                    \
    if constexpr (kBnTileVecs >= 32) {                                    \
      if (g.block == 4 * kBlock) {                                        \
        GS_BN_REDUCE_B(4 * kBlock, MASK, WRITE_G, FORK);                  \
        break;                                                            \
      }                                                                   \
    }                                                                     \
    if constexpr (kBnTileVecs >= 16) {                                    \
      if (g.block == 2 * kBlock) {                                        \
        GS_BN_REDUCE_B(2 * kBlock, MASK, WRITE_G, FORK);                  \
        break;                                                            \
      }                                                                   \
    }                                                                     \
    GS_BN_REDUCE_B(kBlock, MASK, WRITE_G, FORK);                          \
  } while (0)
  if (mp && bp) GS_BN_REDUCE(kMaskBits, true, true);
  else if (mp && gp) GS_BN_REDUCE(kMaskBits, true, false);
  else if (mp) GS_BN_REDUCE(kMaskBits, false, false);
  else if (bp && yp) GS_BN_REDUCE(kMaskY, true, true);
  else if (bp) GS_BN_REDUCE(kMaskNone, true, true);
  else if (gp) GS_BN_REDUCE(kMaskY, true, false);
  else if (yp) GS_BN_REDUCE(kMaskY, false, false);
  else GS_BN_REDUCE(kMaskNone, false, false);
#undef GS_BN_REDUCE
#undef GS_BN_REDUCE_B
  HIP_RET(hipGetLastError());
  return GS_OK;
}

}  // namespace
}  // namespace gs

extern "C" int gs_bn_bwd_reduce(const void* x, const void* dy, const void* y, void* g_out, const float* mean,
                                float* ws, int64_t ws_floats, int64_t R, int C, void* stream) {
  return bn_reduce("gs_bn_bwd_reduce", x, dy, nullptr, y, false, nullptr, g_out, mean, ws, ws_floats, R, C, stream);
}

extern "C" int gs_bn_bwd_reduce_bits(const void* x, const void* dy, const void* mask, void* g_out, const float* mean,
                                     float* ws, int64_t ws_floats, int64_t R, int C, void* stream) {
  return bn_reduce("gs_bn_bwd_reduce_bits", x, dy, nullptr, nullptr, true, mask, g_out, mean, ws, ws_floats, R, C,
                   stream);
}

extern "C" int gs_bn_bwd_reduce_fork(const void* x, const void* dy_a, const void* dy_b, const void* y, void* g_out,
                                     const float* mean, float* ws, int64_t ws_floats, int64_t R, int C,
                                     void* stream) {
  return bn_reduce("gs_bn_bwd_reduce_fork", x, dy_a, dy_b, y, false, nullptr, g_out, mean, ws, ws_floats, R, C,
                   stream);
}

extern "C" int gs_bn_bwd_reduce_fork_bits(const void* x, const void* dy_a, const void* dy_b, const void* mask,
                                          void* g_out, const float* mean, float* ws, int64_t ws_floats, int64_t R,
                                          int C, void* stream) {
  return bn_reduce("gs_bn_bwd_reduce_fork_bits", x, dy_a, dy_b, nullptr, true, mask, g_out, mean, ws, ws_floats, R, C,
                   stream);
}

namespace gs {
namespace {

// bits: the mask comes from `mask` (required, any alignment, overlaps neither dx) and y is NULL
int bn_dx(const std::string& w, const void* x, const void* dy, const void* y, bool bits, const void* mask,
          const float* mean, const float* invstd, const float* weight, const float* ws, int64_t ws_floats, void* dx,
          float* grad_weight, float* grad_bias, int64_t R, int C, void* stream) {
  GS_TRY_RET(check_shape(R, C));
  GS_CHECK_ARG(x && dy && mean && invstd && weight && ws && dx && grad_weight && grad_bias && (!bits || mask),
               w + ": null pointer");
  GS_CHECK_ARG(aligned16(x) && aligned16(dy) && aligned16(y) && aligned16(dx) && aligned16(ws),
               w + ": pointers must be 16-byte aligned");
  GS_CHECK_ARG(!overlap(dx, R * C * 2, mask, R * C / 8), w + ": dx overlaps the mask");
  const BnGeom g = bn_geom(R, C);
  GS_CHECK_ARG(ws_floats >= static_cast<int64_t>(g.P) * C * 2, w + ": workspace too small");
  const dim3 grid(g.ctiles, g.P), block(g.block);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint16_t* dp = static_cast<const uint16_t*>(dy);
  const uint16_t* yp = static_cast<const uint16_t*>(y);
  const uint8_t* mp = static_cast<const uint8_t*>(mask);
  uint16_t* op = static_cast<uint16_t*>(dx);
  const double inv_R = 1.0 / static_cast<double>(R);
#define GS_BN_DX_B(BLOCK, MASK)                                                                                     \
  hipLaunchKernelGGL((bn_bwd_dx_kernel<BLOCK, MASK>), grid, block, 0, s, xp, dp, yp, mp, mean, invstd, weight, ws, \
                     g.P, op, grad_weight, grad_bias, R, C, g.tx_log2, g.rpb, inv_R)
#define GS_BN_DX(MASK)                     \
  do {                                     \
    if constexpr (kBnTileVecs >= 32) {     \
      if (g.block == 4 * kBlock) {         \
        GS_BN_DX_B(4 * kBlock, MASK);      \
        break;                             \
      }                                    \
    }                                      \
    if constexpr (kBnTileVecs >= 16) {     \
      if (g.block == 2 * kBlock) {         \
        GS_BN_DX_B(2 * kBlock, MASK);      \
        break;                             \
      }                                    \
    }                                      \
    GS_BN_DX_B(kBlock, MASK);              \
  } while (0)
  if (mp) GS_BN_DX(kMaskBits);
  else if (yp) GS_BN_DX(kMaskY);
  else GS_BN_DX(kMaskNone);
#undef GS_BN_DX
#undef GS_BN_DX_B
  HIP_RET(hipGetLastError());
  return GS_OK;
}

// t = relu(t (+ identity)) in place (+ the mask bytes); identity and mask are optional per entry
int relu_tail(const std::string& w, void* t, const void* identity, bool add, void* mask, bool bits, int64_t n,
              void* stream) {
  GS_CHECK_ARG(t && (!add || identity) && (!bits || mask) && n > 0 && n % 8 == 0,
               w + ": n > 0, n % 8 == 0 and pointers required");
  GS_CHECK_ARG(aligned16(t) && aligned16(identity), w + ": pointers must be 16-byte aligned");
  GS_CHECK_ARG(n <= INT64_MAX / 4, w + ": n too large");
  GS_CHECK_ARG(!overlap(mask, n / 8, t, n * 2) && !overlap(mask, n / 8, identity, n * 2),
               w + ": the mask overlaps an activation");
  const int64_t nvec = n / 8;
  const int64_t blocks = (nvec + kBlock * kBnUnroll - 1) / (kBlock * kBnUnroll);
  GS_CHECK_ARG(blocks <= INT_MAX, w + ": n too large");
  const dim3 grid(static_cast<unsigned>(blocks)), block(kBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint16_t* tp = static_cast<uint16_t*>(t);
  const uint16_t* ip = static_cast<const uint16_t*>(identity);
  uint8_t* mp = static_cast<uint8_t*>(mask);
  if (!add) hipLaunchKernelGGL((add_relu_fwd_kernel<false, true>), grid, block, 0, s, tp, ip, mp, nvec);
  else if (bits) hipLaunchKernelGGL((add_relu_fwd_kernel<true, true>), grid, block, 0, s, tp, ip, mp, nvec);
  else hipLaunchKernelGGL((add_relu_fwd_kernel<true, false>), grid, block, 0, s, tp, ip, mp, nvec);
  HIP_RET(hipGetLastError());
  return GS_OK;
}

// mask != NULL: the mask bytes of the un-ReLU'd input are written as well (in_vecs bytes)
int relu_maxpool(const std::string& w, const void* y, void* pooled, void* idx, void* mask, bool bits, int64_t N, int H,
                 int W, int C, void* stream) {
  PoolGeom g;
  GS_TRY_RET(pool_geom(w, N, H, W, C, &g));
  GS_CHECK_ARG(y && pooled && idx && (!bits || mask), w + ": null pointer");
  GS_CHECK_ARG(aligned16(y) && aligned16(pooled) && aligned16(idx), w + ": pointers must be 16-byte aligned");
  const int64_t ib = g.in_vecs * 16, ob = g.out_vecs * 16, xb = g.out_vecs * 8, mb = g.in_vecs;
  GS_CHECK_ARG(!overlap(y, ib, pooled, ob) && !overlap(y, ib, idx, xb) && !overlap(pooled, ob, idx, xb) &&
                   !overlap(mask, mb, y, ib) && !overlap(mask, mb, pooled, ob) && !overlap(mask, mb, idx, xb),
               w + ": buffers overlap");
  const dim3 grid(static_cast<unsigned>((g.out_vecs + kBlock - 1) / kBlock)), block(kBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint16_t* yp = static_cast<const uint16_t*>(y);
  uint16_t* pp = static_cast<uint16_t*>(pooled);
  uint8_t* ip = static_cast<uint8_t*>(idx);
  uint8_t* mp = static_cast<uint8_t*>(mask);
  if (mp)
    hipLaunchKernelGGL((relu_maxpool_fwd_kernel<true>), grid, block, 0, s, yp, pp, ip, mp, g.out_vecs, H, W, g.OH, g.OW,
                       C / 8);
  else
    hipLaunchKernelGGL((relu_maxpool_fwd_kernel<false>), grid, block, 0, s, yp, pp, ip, mp, g.out_vecs, H, W, g.OH,
                       g.OW, C / 8);
  HIP_RET(hipGetLastError());
  return GS_OK;
}

}  // namespace
}  // namespace gs

extern "C" int gs_bn_bwd_dx(const void* x, const void* dy, const void* y, const float* mean, const float* invstd,
                            const float* weight, const float* ws, int64_t ws_floats, void* dx, float* grad_weight,
                            float* grad_bias, int64_t R, int C, void* stream) {
  return bn_dx("gs_bn_bwd_dx", x, dy, y, false, nullptr, mean, invstd, weight, ws, ws_floats, dx, grad_weight,
               grad_bias, R, C, stream);
}

extern "C" int gs_bn_bwd_dx_bits(const void* x, const void* dy, const void* mask, const float* mean,
                                 const float* invstd, const float* weight, const float* ws, int64_t ws_floats,
                                 void* dx, float* grad_weight, float* grad_bias, int64_t R, int C, void* stream) {
  return bn_dx("gs_bn_bwd_dx_bits", x, dy, nullptr, true, mask, mean, invstd, weight, ws, ws_floats, dx, grad_weight,
               grad_bias, R, C, stream);
}

extern "C" int gs_add_relu_fwd(void* t, const void* identity, int64_t n, void* stream) {
  return relu_tail("gs_add_relu_fwd", t, identity, true, nullptr, false, n, stream);
}

extern "C" int gs_add_relu_mask_fwd(void* t, const void* identity, void* mask, int64_t n, void* stream) {
  return relu_tail("gs_add_relu_mask_fwd", t, identity, true, mask, true, n, stream);
}

extern "C" int gs_relu_mask_fwd(void* t, void* mask, int64_t n, void* stream) {
  return relu_tail("gs_relu_mask_fwd", t, nullptr, false, mask, true, n, stream);
}

extern "C" int gs_relu_maxpool_fwd(const void* y, void* pooled, void* idx, int64_t N, int H, int W, int C,
                                   void* stream) {
  return relu_maxpool("gs_relu_maxpool_fwd", y, pooled, idx, nullptr, false, N, H, W, C, stream);
}

extern "C" int gs_relu_maxpool_mask_fwd(const void* y, void* pooled, void* idx, void* mask, int64_t N, int H, int W,
                                        int C, void* stream) {
  return relu_maxpool("gs_relu_maxpool_mask_fwd", y, pooled, idx, mask, true, N, H, W, C, stream);
}

extern "C" int gs_maxpool_bwd(const void* d_a, const void* d_b, const void* idx, void* dx, int64_t N, int H, int W,
                              int C, void* stream) {
  const std::string w("gs_maxpool_bwd");
  PoolGeom g;
  GS_TRY_RET(pool_geom(w, N, H, W, C, &g));
  GS_CHECK_ARG(d_a && idx && dx, w + ": null pointer");
  GS_CHECK_ARG(aligned16(d_a) && aligned16(d_b) && aligned16(idx) && aligned16(dx),
               w + ": pointers must be 16-byte aligned");
  const int64_t ib = g.in_vecs * 16, ob = g.out_vecs * 16, xb = g.out_vecs * 8;
  GS_CHECK_ARG(!overlap(dx, ib, d_a, ob) && !overlap(dx, ib, d_b, ob) && !overlap(dx, ib, idx, xb),
               w + ": dx overlaps an input");
  const dim3 grid(static_cast<unsigned>((g.out_vecs + kBlock - 1) / kBlock)), block(kBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint16_t* ap = static_cast<const uint16_t*>(d_a);
  const uint16_t* bp = static_cast<const uint16_t*>(d_b);
  const uint8_t* ip = static_cast<const uint8_t*>(idx);
  uint16_t* op = static_cast<uint16_t*>(dx);
  if (bp)
    hipLaunchKernelGGL((maxpool_bwd_kernel<true>), grid, block, 0, s, ap, bp, ip, op, g.out_vecs, H, W, g.OH, g.OW,
                       C / 8);
  else
    hipLaunchKernelGGL((maxpool_bwd_kernel<false>), grid, block, 0, s, ap, bp, ip, op, g.out_vecs, H, W, g.OH, g.OW,
                       C / 8);
  HIP_RET(hipGetLastError());
  return GS_OK;
}

extern "C" int gs_bn_infer_act(const void* x, const void* residual, const float* running_mean,
                               const float* running_var, const float* weight, const float* bias, double eps, int relu,
                               void* y, int64_t R, int C, void* stream) {
  const std::string w("gs_bn_infer_act");
  GS_TRY_RET(check_shape(R, C));
  GS_CHECK_ARG(x && running_mean && running_var && weight && bias && y, w + ": null pointer");
  GS_CHECK_ARG(eps >= 0.0 && eps == eps, w + ": eps must be >= 0");
  GS_CHECK_ARG(aligned16(x) && aligned16(residual) && aligned16(y) && aligned16(running_mean) &&
                   aligned16(running_var) && aligned16(weight) && aligned16(bias),
               w + ": pointers must be 16-byte aligned");
  const int64_t bytes = R * C * 2;
  GS_CHECK_ARG(x == y || !overlap(x, y, bytes), w + ": y overlaps x without being x");
  GS_CHECK_ARG(!overlap(residual, y, bytes), w + ": y overlaps the residual");
  const BnGeom g = bn_infer_geom(R, C);
  const dim3 grid(g.ctiles, g.P), block(kBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint16_t* rp = static_cast<const uint16_t*>(residual);
  uint16_t* yp = static_cast<uint16_t*>(y);
  const float e = static_cast<float>(eps);
#define GS_BN_INFER(RES, RELU)                                                                                   \
  hipLaunchKernelGGL((bn_infer_act_kernel<RES, RELU>), grid, block, 0, s, xp, rp, running_mean, running_var, weight, \
                     bias, e, yp, R, C, g.tx_log2, g.rpb)
  if (rp && relu) GS_BN_INFER(true, true);
  else if (rp) GS_BN_INFER(true, false);
  else if (relu) GS_BN_INFER(false, true);
  else GS_BN_INFER(false, false);
#undef GS_BN_INFER
  HIP_RET(hipGetLastError());
  return GS_OK;
}

extern "C" int gs_bn_infer_relu_maxpool(const void* x, const float* running_mean, const float* running_var,
                                        const float* weight, const float* bias, double eps, void* pooled, int64_t N,
                                        int H, int W, int C, void* stream) {
  const std::string w("gs_bn_infer_relu_maxpool");
  PoolGeom pg;
  GS_TRY_RET(pool_geom(w, N, H, W, C, &pg));
  GS_CHECK_ARG(x && running_mean && running_var && weight && bias && pooled, w + ": null pointer");
  GS_CHECK_ARG(eps >= 0.0 && eps == eps, w + ": eps must be >= 0");
  GS_CHECK_ARG(aligned16(x) && aligned16(pooled) && aligned16(running_mean) && aligned16(running_var) &&
                   aligned16(weight) && aligned16(bias),
               w + ": pointers must be 16-byte aligned");
  GS_CHECK_ARG(!overlap(x, pg.in_vecs * 16, pooled, pg.out_vecs * 16), w + ": buffers overlap");
  const int64_t OR = N * pg.OH * pg.OW;
  const BnGeom g = bn_infer_geom(OR, C);
  hipLaunchKernelGGL(bn_infer_relu_maxpool_kernel, dim3(g.ctiles, g.P), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), static_cast<const uint16_t*>(x), running_mean, running_var,
                     weight, bias, static_cast<float>(eps), static_cast<uint16_t*>(pooled), OR, H, W, pg.OH, pg.OW, C,
                     g.tx_log2, g.rpb);
  HIP_RET(hipGetLastError());
  return GS_OK;
}
