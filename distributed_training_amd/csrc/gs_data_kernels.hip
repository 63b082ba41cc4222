// gfx950 kernel of the input step: the whole uint8 image
// set stays resident in HBM ([N, H, W, C], CIFAR-10 train = 153.6 MB) and one
// launch per batch gathers the sampled images and applies Pad -> hflip ->
// crop -> ToTensor (x / 255) (+ bf16 cast), writing the training tensor in
// NCHW or NHWC, with the labels gathered alongside.  Replaces the reference's
// per-sample PIL transforms + default_collate + H2D copy
// (R:resnet/pytorch_ddp/ddp_train.py:25-48, 62-63).
//
// HBM-bound streaming: per sample C*oh*ow*(1 + 4) bytes (uint8 read, f32
// write).  Each lane produces 4 consecutive output elements and stores them
// with one 16-B (f32) / 8-B (bf16) access; the uint8 reads are byte gathers
// served from L2 (a sample's 3 KiB image is touched by 12 lanes at most per
// row).  The per-sample params (index, flip, top, left) arrive as one small
// device array.  With MIX (gs_image_augment_mix) a second record per sample names
// a partner in the batch, and the same launch blends or pastes the partner's
// augmented image into the sample's (MixUp / CutMix).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "gs_common.h"

namespace gs {
namespace {

#define HIP_RET(expr)                                                               \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess)                                                           \
      return fail(GS_EHIP, std::string(#expr " failed: ") + hipGetErrorString(_e)); \
  } while (0)

typedef float gf4 __attribute__((ext_vector_type(4)));
typedef uint32_t gu2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint16_t to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7FC0;
  return static_cast<uint16_t>((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// the kernels' argument: gs_image_augment's, or with MIX gs_image_augment_mix's (the unmixed
// instantiations keep their signature)
template <bool MIX>
using AugArgs = std::conditional_t<MIX, ImageMixAugArgs, ImageAugArgs>;

__device__ __forceinline__ MixRec mix_record(const ImageMixAugArgs& a, int64_t b) {
  const int4 m = reinterpret_cast<const int4*>(a.mix)[b];
  return mix_decode(m.x, m.y, m.z, m.w, b, a.B, a.out_h, a.out_w);
}

template <int LAYOUT, bool MIX>
__device__ __forceinline__ float elem(const AugArgs<MIX>& a, int64_t e, int64_t per) {
  const int64_t b = e / per;
  const int64_t k = e - b * per;
  int c, y, x;
  if constexpr (LAYOUT == GS_LAYOUT_NCHW) {
    x = static_cast<int>(k % a.out_w);
    y = static_cast<int>((k / a.out_w) % a.out_h);
    c = static_cast<int>(k / (static_cast<int64_t>(a.out_w) * a.out_h));
  } else {
    c = static_cast<int>(k % a.C);
    x = static_cast<int>((k / a.C) % a.out_w);
    y = static_cast<int>(k / (static_cast<int64_t>(a.C) * a.out_w));
  }
  const int4 p = reinterpret_cast<const int4*>(a.params)[b];
  if constexpr (MIX) {
    const float va =
        (p.x < 0 || p.x >= a.n_src) ? 0.f : aug_pixel(a.src, p.x, a.H, a.W, a.C, a.pad, p.y, p.z, p.w, c, y, x);
    const MixRec r = mix_record(a, b);
    if (!r.need_b) return va;
    const int4 pb = reinterpret_cast<const int4*>(a.params)[r.partner];
    const float vb = (pb.x < 0 || pb.x >= a.n_src)
                         ? 0.f
                         : aug_pixel(a.src, pb.x, a.H, a.W, a.C, a.pad, pb.y, pb.z, pb.w, c, y, x);
    return mix_pixel(va, vb, r, y, x);
  } else {
    if (p.x < 0 || p.x >= a.n_src) return 0.f;  // never read outside the image set
    return aug_pixel(a.src, p.x, a.H, a.W, a.C, a.pad, p.y, p.z, p.w, c, y, x);
  }
}

template <int LAYOUT, int DT, bool MIX>
__global__ void __launch_bounds__(256) augment_kernel(AugArgs<MIX> a, int64_t total, bool vec) {
  const int64_t per = static_cast<int64_t>(a.C) * a.out_h * a.out_w;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (a.out_labels && gid < a.B) {
    const int idx = reinterpret_cast<const int4*>(a.params)[gid].x;
    a.out_labels[gid] = (a.labels && idx >= 0 && idx < a.n_src) ? a.labels[idx] : 0;
  }
  if constexpr (MIX) {
    if (gid < a.B) {
      const MixRec r = mix_record(a, gid);
      const int idx = reinterpret_cast<const int4*>(a.params)[r.partner].x;
      if (a.out_labels_b) a.out_labels_b[gid] = (a.labels && idx >= 0 && idx < a.n_src) ? a.labels[idx] : 0;
      if (a.out_lam) a.out_lam[gid] = r.lam;
    }
  }
  for (int64_t q = gid; q * 4 < total; q += stride) {
    const int64_t e = q * 4;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (e + i < total) ? elem<LAYOUT, MIX>(a, e + i, per) : 0.f;
    if constexpr (DT == GS_F32) {
      float* o = static_cast<float*>(a.out) + e;
      if (vec && e + 4 <= total) {
        gf4 w;
        w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3];
        *reinterpret_cast<gf4*>(o) = w;
      } else {
        for (int i = 0; i < 4; ++i)
          if (e + i < total) o[i] = v[i];
      }
    } else {
      uint16_t* o = static_cast<uint16_t*>(a.out) + e;
      if (vec && e + 4 <= total) {
        gu2 w;
        w.x = static_cast<uint32_t>(to_bf16(v[0])) | (static_cast<uint32_t>(to_bf16(v[1])) << 16);
        w.y = static_cast<uint32_t>(to_bf16(v[2])) | (static_cast<uint32_t>(to_bf16(v[3])) << 16);
        *reinterpret_cast<gu2*>(o) = w;
      } else {
        for (int i = 0; i < 4; ++i)
          if (e + i < total) o[i] = to_bf16(v[i]);
      }
    }
  }
}

// One workgroup per sample (grid-stride over samples): the sample's uint8
// image is staged in LDS with coalesced 16-B loads, then every lane builds
// 4 consecutive output elements from LDS (32-bit index math only) and writes
// them with one 16-B / 8-B store.  Used when the image fits the LDS budget
// (CIFAR: 3 KiB); larger images take augment_kernel (L2-served gathers).
// MIX: a sample whose record needs its partner stages the partner's image behind its own
// (a workgroup-uniform branch between the same two barriers), so two images must fit.
constexpr int kAugLdsBytes = 48 * 1024;

template <int LAYOUT, int DT, bool MIX>
__global__ void __launch_bounds__(256) augment_lds_kernel(AugArgs<MIX> a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_img[];
  const int img_bytes = a.H * a.W * a.C;
  const int per = a.C * a.out_h * a.out_w;
  const int quads = per >> 2;  // per % 4 == 0 (host checks)
  const int wp = a.W + 2 * a.pad;
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    const int4 p = reinterpret_cast<const int4*>(a.params)[b];
    const bool ok = p.x >= 0 && p.x < a.n_src;
    if (threadIdx.x == 0 && a.out_labels) a.out_labels[b] = (ok && a.labels) ? a.labels[p.x] : 0;
    MixRec r{};
    int4 pb = p;
    bool okb = false;
    if constexpr (MIX) {
      r = mix_record(a, b);
      pb = reinterpret_cast<const int4*>(a.params)[r.partner];
      okb = pb.x >= 0 && pb.x < a.n_src;
      if (threadIdx.x == 0) {
        if (a.out_labels_b) a.out_labels_b[b] = (okb && a.labels) ? a.labels[pb.x] : 0;
        if (a.out_lam) a.out_lam[b] = r.lam;
      }
    }
    __syncthreads();  // previous sample's LDS reads are done
    if (ok) {
      const uint8_t* src = a.src + static_cast<int64_t>(p.x) * img_bytes;
      for (int o = threadIdx.x * 16; o < img_bytes; o += 256 * 16)
        *reinterpret_cast<uint4*>(s_img + o) = *reinterpret_cast<const uint4*>(src + o);
    }
    if constexpr (MIX) {
      if (r.need_b && okb) {
        const uint8_t* src = a.src + static_cast<int64_t>(pb.x) * img_bytes;
        for (int o = threadIdx.x * 16; o < img_bytes; o += 256 * 16)
          *reinterpret_cast<uint4*>(s_img + img_bytes + o) = *reinterpret_cast<const uint4*>(src + o);
      }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < quads; q += 256) {
      const int k0 = q << 2;
      // (c, y, x) of the quad's first element, then step through the layout's order
      int c, y, x;
      if constexpr (LAYOUT == GS_LAYOUT_NCHW) {
        x = k0 % a.out_w;
        const int r = k0 / a.out_w;
        y = r % a.out_h;
        c = r / a.out_h;
      } else {
        c = k0 % a.C;
        const int pix = k0 / a.C;
        x = pix % a.out_w;
        y = pix / a.out_w;
      }
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int px = p.y ? (wp - 1 - (x + p.w)) : (x + p.w);
        const int sy = y + p.z - a.pad, sx = px - a.pad;
        v[i] = (ok && sy >= 0 && sy < a.H && sx >= 0 && sx < a.W)
                   ? static_cast<float>(s_img[(sy * a.W + sx) * a.C + c]) / 255.f
                   : 0.f;
        if constexpr (MIX) {
          if (r.need_b) {
            const int qx = pb.y ? (wp - 1 - (x + pb.w)) : (x + pb.w);
            const int ty = y + pb.z - a.pad, tx = qx - a.pad;
            const float vb = (okb && ty >= 0 && ty < a.H && tx >= 0 && tx < a.W)
                                 ? static_cast<float>(s_img[img_bytes + (ty * a.W + tx) * a.C + c]) / 255.f
                                 : 0.f;
            v[i] = mix_pixel(v[i], vb, r, y, x);
          }
        }
        if constexpr (LAYOUT == GS_LAYOUT_NCHW) {
          if (++x == a.out_w) { x = 0; if (++y == a.out_h) { y = 0; ++c; } }
        } else {
          if (++c == a.C) { c = 0; if (++x == a.out_w) { x = 0; ++y; } }
        }
      }
      const int64_t e = b * per + k0;
      if constexpr (DT == GS_F32) {
        gf4 w;
        w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3];
        *reinterpret_cast<gf4*>(static_cast<float*>(a.out) + e) = w;
      } else {
        gu2 w;
        w.x = static_cast<uint32_t>(to_bf16(v[0])) | (static_cast<uint32_t>(to_bf16(v[1])) << 16);
        w.y = static_cast<uint32_t>(to_bf16(v[2])) | (static_cast<uint32_t>(to_bf16(v[3])) << 16);
        *reinterpret_cast<gu2*>(static_cast<uint16_t*>(a.out) + e) = w;
      }
    }
  }
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) (void)hipSetDevice(dev);
    else prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// both entries' launch: the LDS kernel when the images it stages (one, with MIX two) fit the
// budget and the 16-byte conditions hold, else the global-gather kernel
template <bool MIX>
int launch_augment(int device, const AugArgs<MIX>& a, void* stream) {
  DeviceGuard g(device);
  const int64_t total = a.B * a.C * a.out_h * a.out_w;
  const int64_t quads = (total + 3) / 4;
  const int blocks = static_cast<int>(std::max<int64_t>(
      (a.B + 255) / 256, std::min<int64_t>((quads + 255) / 256, 8192)));
  const bool vec = (reinterpret_cast<uintptr_t>(a.out) & 15u) == 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t img_bytes = static_cast<int64_t>(a.H) * a.W * a.C;
  const int64_t per = static_cast<int64_t>(a.C) * a.out_h * a.out_w;
  const int64_t staged = MIX ? 2 * img_bytes : img_bytes;
  bool aligned = (reinterpret_cast<uintptr_t>(a.src) & 15u) == 0;
  if constexpr (MIX) aligned = aligned && (reinterpret_cast<uintptr_t>(a.mix) & 15u) == 0;
  if (vec && staged <= kAugLdsBytes && img_bytes % 16 == 0 && per % 4 == 0 && aligned) {
    const int g2 = static_cast<int>(std::min<int64_t>(a.B, 65535));
    const size_t lds = static_cast<size_t>(staged);
    if (a.layout == GS_LAYOUT_NCHW) {
      if (a.out_dtype == GS_F32)
        hipLaunchKernelGGL((augment_lds_kernel<GS_LAYOUT_NCHW, GS_F32, MIX>), dim3(g2), dim3(256), lds, s, a);
      else
        hipLaunchKernelGGL((augment_lds_kernel<GS_LAYOUT_NCHW, GS_BF16, MIX>), dim3(g2), dim3(256), lds, s, a);
    } else {
      if (a.out_dtype == GS_F32)
        hipLaunchKernelGGL((augment_lds_kernel<GS_LAYOUT_NHWC, GS_F32, MIX>), dim3(g2), dim3(256), lds, s, a);
      else
        hipLaunchKernelGGL((augment_lds_kernel<GS_LAYOUT_NHWC, GS_BF16, MIX>), dim3(g2), dim3(256), lds, s, a);
    }
    HIP_RET(hipGetLastError());
    return GS_OK;
  }
  if (a.layout == GS_LAYOUT_NCHW) {
    if (a.out_dtype == GS_F32)
      hipLaunchKernelGGL((augment_kernel<GS_LAYOUT_NCHW, GS_F32, MIX>), dim3(blocks), dim3(256), 0, s, a, total, vec);
    else
      hipLaunchKernelGGL((augment_kernel<GS_LAYOUT_NCHW, GS_BF16, MIX>), dim3(blocks), dim3(256), 0, s, a, total, vec);
  } else {
    if (a.out_dtype == GS_F32)
      hipLaunchKernelGGL((augment_kernel<GS_LAYOUT_NHWC, GS_F32, MIX>), dim3(blocks), dim3(256), 0, s, a, total, vec);
    else
      hipLaunchKernelGGL((augment_kernel<GS_LAYOUT_NHWC, GS_BF16, MIX>), dim3(blocks), dim3(256), 0, s, a, total, vec);
  }
  HIP_RET(hipGetLastError());
  return GS_OK;
}

// ---- gs_image_resample: bilinear resized crop of a per-sample box + hflip + ToTensor
// (+ Normalize) (+ bf16 cast); the arithmetic is gs_common.h's resample_* helpers on both backends.
//
// Per sample h*w*C bytes are read and C*oh*ow*(2|4) written, so the kernel is a streaming one
// whose reads are a 2-D window of a larger image: rows of w*C bytes at an arbitrary byte
// offset, W*C apart.  resample_band_kernel gives one workgroup a (sample, band of output rows)
// pair: it stages the source rows the band's taps touch (the first output row's i0 to the last
// one's i1), bytes [left*C, (left + w)*C) of each, into LDS with 16-byte loads aligned in global
// memory (an LDS row starts at the row's address rounded down to 16, so a tap is at
// (address & 15) + x*C + c of its row), and then every lane builds 4 consecutive output
// elements from LDS and writes them with one 16-B / 8-B store.  Neighbouring bands re-read at
// most two boundary rows.  A tap's quotient u8 / 255.f is resample_unit's two fused operations (an
// LDS table of the 256 quotients cost four more dependent, bank-conflicting reads per output).
// resample_gather_kernel reads the four taps of every element from global memory (L2-served
// byte loads) and takes what the band scheme does not: see hip_image_resample.
#ifndef GS_RESAMPLE_BAND
#define GS_RESAMPLE_BAND 32  // output rows per band, before it shrinks to fit the LDS budget
#endif

// v[c] by compares, so that the kernel argument stays in scalar registers
__device__ __forceinline__ float pick4(const float (&v)[4], int c) {
  return c == 0 ? v[0] : c == 1 ? v[1] : c == 2 ? v[2] : v[3];
}

template <int DT>
__device__ __forceinline__ void store_quad(void* out, int64_t e, const float* v) {
  if constexpr (DT == GS_F32) {
    gf4 w;
    w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3];
    *reinterpret_cast<gf4*>(static_cast<float*>(out) + e) = w;
  } else {
    gu2 w;
    w.x = static_cast<uint32_t>(to_bf16(v[0])) | (static_cast<uint32_t>(to_bf16(v[1])) << 16);
    w.y = static_cast<uint32_t>(to_bf16(v[2])) | (static_cast<uint32_t>(to_bf16(v[3])) << 16);
    *reinterpret_cast<gu2*>(static_cast<uint16_t*>(out) + e) = w;
  }
}

template <int LAYOUT, int DT>
__global__ void __launch_bounds__(256)
resample_band_kernel(ImageResampleArgs a, int band_rows, int n_bands, int rows_cap, int pitch) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_res[];
  uint8_t* rows = s_res;
  const int per = a.C * a.out_h * a.out_w;  // < 2^31 (host checks)
  const int row_bytes = a.W * a.C;
  const uintptr_t set_lo = reinterpret_cast<uintptr_t>(a.src);
  const uintptr_t set_hi = set_lo + static_cast<uint64_t>(a.n_src) * a.H * row_bytes;
  const int rowelems = LAYOUT == GS_LAYOUT_NHWC ? a.out_w * a.C : a.out_w;
  const int64_t items = a.B * n_bands;
  for (int64_t wi = blockIdx.x; wi < items; wi += gridDim.x) {
    const int64_t b = wi / n_bands;
    const int band = static_cast<int>(wi - b * n_bands);
    const int4 w = reinterpret_cast<const int4*>(a.rec)[b];
    const ResampleBox r = resample_decode(w.x, w.y, w.z, w.w, a.n_src, a.H, a.W);
    if (band == 0 && threadIdx.x == 0 && a.out_labels) a.out_labels[b] = (r.ok && a.labels) ? a.labels[r.idx] : 0;
    const int y0 = band * band_rows;
    const int y1 = min(y0 + band_rows, a.out_h);
    const float sy = resample_scale(r.h, a.virt_h), sx = resample_scale(r.w, a.virt_w);
    // the band's source rows [row0, row0 + nrows) of the box; rows_cap is the host's bound for any
    // box, and every LDS row index below is clamped to it all the same
    const int row0 = resample_tap(y0 + a.off_y, sy, r.h).i0;
    const int nrows = min(resample_tap(y1 - 1 + a.off_y, sy, r.h).i1 - row0 + 1, rows_cap);
    const int wc = r.w * a.C;
    const uintptr_t g0 =
        set_lo + ((static_cast<int64_t>(r.idx) * a.H + r.top + row0) * a.W + r.left) * static_cast<int64_t>(a.C);
    __syncthreads();  // the previous item's LDS reads are done
    if (r.ok) {
      const int chunks = (wc + 30) >> 4;  // 16-byte chunks that cover wc bytes at any misalignment
      for (int i = threadIdx.x; i < nrows * chunks; i += 256) {
        const int rr = i / chunks, k = i - rr * chunks;
        const uintptr_t g = g0 + static_cast<uintptr_t>(rr) * row_bytes;
        const uintptr_t p = (g & ~static_cast<uintptr_t>(15)) + 16u * k;
        if (p >= g + wc) continue;  // past this row's span
        uint4 v;
        if (p >= set_lo && p + 16 <= set_hi) {
          v = *reinterpret_cast<const uint4*>(p);
        } else {  // a chunk that straddles an end of the image set: its bytes inside the set only
          uint32_t t[4] = {0u, 0u, 0u, 0u};
          for (int j = 0; j < 16; ++j) {
            const uintptr_t q = p + j;
            if (q >= set_lo && q < set_hi)
              t[j >> 2] |= static_cast<uint32_t>(*reinterpret_cast<const uint8_t*>(q)) << (8 * (j & 3));
          }
          v = make_uint4(t[0], t[1], t[2], t[3]);
        }
        *reinterpret_cast<uint4*>(rows + rr * pitch + 16 * k) = v;
      }
    }
    __syncthreads();
    // the band's output elements: one contiguous run (NHWC) or one per channel (NCHW), each a
    // multiple of 4 long and 4-aligned in the sample (host checks)
    const int run = (y1 - y0) * rowelems;
    const int quads_run = run >> 2;
    const int n_quads = LAYOUT == GS_LAYOUT_NHWC ? quads_run : quads_run * a.C;
    const uint32_t g0lo = static_cast<uint32_t>(g0);
    for (int q = threadIdx.x; q < n_quads; q += 256) {
      int c, y, x, e;
      if constexpr (LAYOUT == GS_LAYOUT_NCHW) {
        c = q / quads_run;
        const int k0 = (q - c * quads_run) << 2;
        y = y0 + k0 / a.out_w;
        x = k0 % a.out_w;
        e = (c * a.out_h + y0) * a.out_w + k0;
      } else {
        const int k0 = q << 2;
        const int pix = k0 / a.C;
        c = k0 - pix * a.C;
        y = y0 + pix / a.out_w;
        x = pix % a.out_w;
        e = y0 * rowelems + k0;
      }
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (r.ok) {
        ResampleTap ty, tx;
        int b0, b1;  // LDS offsets of the two rows' first box byte
        auto set_y = [&](int yy) {
          ty = resample_tap(yy + a.off_y, sy, r.h);
          const int la = max(0, min(ty.i0 - row0, nrows - 1)), lb = max(0, min(ty.i1 - row0, nrows - 1));
          b0 = la * pitch + static_cast<int>((g0lo + static_cast<uint32_t>(la * row_bytes)) & 15u);
          b1 = lb * pitch + static_cast<int>((g0lo + static_cast<uint32_t>(lb * row_bytes)) & 15u);
        };
        auto set_x = [&](int xx) { tx = resample_tap((r.flip ? a.out_w - 1 - xx : xx) + a.off_x, sx, r.w); };
        set_y(y);
        set_x(x);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int o0 = tx.i0 * a.C + c, o1 = tx.i1 * a.C + c;
          const float o = resample_blend(resample_unit(rows[b0 + o0]), resample_unit(rows[b0 + o1]),
                                         resample_unit(rows[b1 + o0]), resample_unit(rows[b1 + o1]), ty, tx);
          v[i] = a.normalize ? resample_norm(o, pick4(a.mean, c), pick4(a.std, c)) : o;
          if (i == 3) break;
          if constexpr (LAYOUT == GS_LAYOUT_NCHW) {
            if (++x == a.out_w) { x = 0; set_y(++y); }  // y < y1: the run is a whole number of quads
            set_x(x);
          } else {
            if (++c == a.C) {
              c = 0;
              if (++x == a.out_w) { x = 0; set_y(++y); }
              set_x(x);
            }
          }
        }
      }
      store_quad<DT>(a.out, b * per + e, v);
    }
  }
}

template <int LAYOUT, int DT>
__global__ void __launch_bounds__(256) resample_gather_kernel(ImageResampleArgs a, int64_t total, bool vec) {
  __shared__ float tab[256];
  tab[threadIdx.x] = static_cast<float>(threadIdx.x) / 255.f;
  __syncthreads();
  const int64_t per = static_cast<int64_t>(a.C) * a.out_h * a.out_w;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (a.out_labels && gid < a.B) {
    const int idx = reinterpret_cast<const int4*>(a.rec)[gid].x;
    a.out_labels[gid] = (a.labels && idx >= 0 && idx < a.n_src) ? a.labels[idx] : 0;
  }
  for (int64_t q = gid; q * 4 < total; q += stride) {
    const int64_t e = q * 4;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = 0.f;
      if (e + i >= total) continue;
      const int64_t b = (e + i) / per;
      const int4 w = reinterpret_cast<const int4*>(a.rec)[b];
      const ResampleBox r = resample_decode(w.x, w.y, w.z, w.w, a.n_src, a.H, a.W);
      if (!r.ok) continue;  // never read outside the image set
      int c, y, x;
      resample_cyx(LAYOUT, (e + i) - b * per, a.C, a.out_h, a.out_w, &c, &y, &x);
      v[i] = resample_pixel(a, r, resample_scale(r.h, a.virt_h), resample_scale(r.w, a.virt_w), tab, c, y, x);
    }
    if (vec && e + 4 <= total) {
      store_quad<DT>(a.out, e, v);
    } else {
      for (int i = 0; i < 4; ++i) {
        if (e + i >= total) break;
        if constexpr (DT == GS_F32) static_cast<float*>(a.out)[e + i] = v[i];
        else static_cast<uint16_t*>(a.out)[e + i] = to_bf16(v[i]);
      }
    }
  }
}

template <int LAYOUT, int DT>
int launch_resample(const ImageResampleArgs& a, hipStream_t s) {
  const int64_t per = static_cast<int64_t>(a.C) * a.out_h * a.out_w;
  const int64_t total = a.B * per;
  const bool vec = (reinterpret_cast<uintptr_t>(a.out) & 15u) == 0;
  // The band kernel needs 4-aligned runs: per % 4 == 0 (NHWC), out_h * out_w % 4 == 0 (NCHW), and a
  // band of R < out_h rows a multiple of 4 elements per run.  It is not worth staging whole rows
  // when the taps skip most of them: past a 2x downscale on either axis the gather kernel reads less.
  const int rowelems = LAYOUT == GS_LAYOUT_NHWC ? a.out_w * a.C : a.out_w;
  const bool runs_ok = LAYOUT == GS_LAYOUT_NHWC ? per % 4 == 0 : (static_cast<int64_t>(a.out_h) * a.out_w) % 4 == 0;
  const int64_t row_bytes = static_cast<int64_t>(a.W) * a.C;
  int band = 0, rows_cap = 0, pitch = 0;
  if (vec && runs_ok && per <= INT32_MAX && a.H <= 2 * a.virt_h && a.W <= 2 * a.virt_w &&
      row_bytes + 64 <= kAugLdsBytes) {
    pitch = 16 * static_cast<int>((row_bytes + 30) >> 4);
    if (pitch % 128 == 0) pitch += 16;  // rows i0 and i1 of a wave's taps on different banks
    for (int cand = std::min(GS_RESAMPLE_BAND, a.out_h); cand >= 1; --cand) {
      if (cand < a.out_h && (static_cast<int64_t>(cand) * rowelems) % 4 != 0) continue;
      // source rows under cand output rows: the coordinates of the first and the last differ by
      // (cand - 1) * scale, scale <= H / virt_h for any box; + 2 for i0's floor and i1, + 1 for
      // the fp32 coordinate's rounding
      const int64_t need = std::min<int64_t>(
          a.H, (static_cast<int64_t>(cand - 1) * a.H + a.virt_h - 1) / a.virt_h + 3);
      if (need * pitch <= kAugLdsBytes) {
        band = cand;
        rows_cap = static_cast<int>(need);
        break;
      }
    }
  }
  if (band > 0) {
    const int n_bands = (a.out_h + band - 1) / band;
    const int grid = static_cast<int>(std::min<int64_t>(a.B * n_bands, 1 << 20));
    const size_t lds = static_cast<size_t>(rows_cap) * pitch;
    hipLaunchKernelGGL((resample_band_kernel<LAYOUT, DT>), dim3(grid), dim3(256), lds, s, a, band, n_bands, rows_cap,
                       pitch);
  } else {
    const int64_t quads = (total + 3) / 4;
    const int blocks = static_cast<int>(std::max<int64_t>(
        (a.B + 255) / 256, std::min<int64_t>((quads + 255) / 256, 65536)));
    hipLaunchKernelGGL((resample_gather_kernel<LAYOUT, DT>), dim3(blocks), dim3(256), 0, s, a, total, vec);
  }
  HIP_RET(hipGetLastError());
  return GS_OK;
}

}  // namespace

int hip_image_resample(int device, const ImageResampleArgs& a, void* stream) {
  DeviceGuard g(device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a.layout == GS_LAYOUT_NCHW)
    return a.out_dtype == GS_F32 ? launch_resample<GS_LAYOUT_NCHW, GS_F32>(a, s)
                                 : launch_resample<GS_LAYOUT_NCHW, GS_BF16>(a, s);
  return a.out_dtype == GS_F32 ? launch_resample<GS_LAYOUT_NHWC, GS_F32>(a, s)
                               : launch_resample<GS_LAYOUT_NHWC, GS_BF16>(a, s);
}

int hip_image_augment(int device, const ImageAugArgs& a, void* stream) {
  return launch_augment<false>(device, a, stream);
}
int hip_image_augment_mix(int device, const ImageMixAugArgs& a, void* stream) {
  return launch_augment<true>(device, a, stream);
}

}  // namespace gs
