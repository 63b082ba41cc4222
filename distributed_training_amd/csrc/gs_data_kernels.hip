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

}  // namespace

int hip_image_augment(int device, const ImageAugArgs& a, void* stream) {
  return launch_augment<false>(device, a, stream);
}
int hip_image_augment_mix(int device, const ImageMixAugArgs& a, void* stream) {
  return launch_augment<true>(device, a, stream);
}

}  // namespace gs
