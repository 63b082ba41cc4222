// Internal declarations shared by the libgsync translation units.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gsync.h"
#include "gs_math.h"

namespace gs {

// ---- roctx ranges (SURVEY.md §5 tracing): host-side ranges around every
// pack / collective / unpack / update enqueue, visible in
// `rocprofv3 --marker-trace`; off unless GSYNC_ROCTX=1 (one cached getenv)
bool roctx_enabled();
void roctx_push(const char* name);
void roctx_pop();
struct GsRange {
  bool on;
  explicit GsRange(const char* name) : on(roctx_enabled()) {
    if (on) roctx_push(name);
  }
  ~GsRange() {
    if (on) roctx_pop();
  }
  GsRange(const GsRange&) = delete;
  GsRange& operator=(const GsRange&) = delete;
};

// ---- error plumbing: thread-local message, int codes across the ABI ----
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

#define GS_CHECK_ARG(cond, msg)                                   \
  do {                                                            \
    if (!(cond)) return ::gs::fail(GS_EINVAL, std::string(msg));  \
  } while (0)

#define GS_TRY_RET(expr)          \
  do {                            \
    int _rc = (expr);             \
    if (_rc != GS_OK) return _rc; \
  } while (0)

inline int dtype_size(int dt) {
  switch (dt) {
    case GS_F32: return 4;
    case GS_BF16: return 2;
    case GS_F16: return 2;
    case GS_F64: return 8;
    case GS_I64: return 8;
    case GS_I32: return 4;
    case GS_U8: return 1;
    default: return 0;
  }
}
inline bool is_float_dtype(int dt) { return dt == GS_F32 || dt == GS_BF16 || dt == GS_F16; }

// ---- engine constants ----
// 1 unit = 4 elements: one 16-B fp32 access of a lane.  The streaming kernels walk the
// chunk map below; the plan's task decomposition (gs_plan_n_tasks / gs_plan_task_units)
// is public metadata that gs_plan.cpp counts and no kernel reads.
constexpr int kUnit = 4;
constexpr int kBlock = 256;         // 4 waves of 64
// default grid: one workgroup per group of chunks up to kGridLimit (the dispatcher refills
// CUs faster than a resident grid loops: profiles/r1r_copy_micro.jsonl,
// r1r_grid_sweep.jsonl)
constexpr int kMaxGrid = 65536;
constexpr int kGridLimit = 65536;   // hard cap (partials buffer)
// fused reductions: at most kRedMaxGroups group sums (one per lane of the
// folding wave), each counter / group sum on its own 128-B line
constexpr int kRedMaxGroups = GS_RED_GROUPS;
constexpr int kRedSyncStride = 32;

// ---- chunk-map engine (streaming ops) ----
// The plan's tensors are laid end to end in a VIRTUAL element space (voff):
// a tensor of >= kGroupElems elements starts on a kGroupElems boundary, one of
// >= kChunkElems on a kChunkElems boundary, a smaller one on a 4-element
// boundary.  The space is cut into chunks of kChunkElems (one 16-B access per
// lane of a 256-lane workgroup); a workgroup takes G consecutive chunks per
// iteration (G per op, gs_kernels.hip) and grid-strides.  A group of chunks
// that lies wholly inside one tensor is streamed with no per-lane lookup and
// no bounds checks: a wave-uniform base pointer (SGPRs) plus a 32-bit lane
// offset, G accesses per stream in flight; the rest (tensor tails, runs of
// small tensors) go chunk by chunk, resolving each lane's tensor by binary
// search over voff.
constexpr int kChunkElems = 256 * kUnit;    // 1 Ki elements
constexpr int kGroupElems = 4 * kChunkElems;  // largest group (G = 4)
struct ChunkDesc {
  int32_t t0;    // first tensor intersecting the chunk
  int32_t code;  // 0: full chunk inside t0; k > 0: k tensors intersect; -1: empty
};
static_assert(sizeof(ChunkDesc) == 8, "ChunkDesc layout");

// Arguments handed to a device kernel (by value).
struct PlanArgs {
  const int64_t* numel;       // [n]
  const int64_t* off;         // [n] flat offsets (elements)
  void* const* ptrs;          // [GS_PLAN_SLOTS * n]
  const uint32_t* align;      // [n] bit s = slot s pointer is 16-B aligned
  const ChunkDesc* chunks;    // [n_chunks]
  const int64_t* voff;        // [n] virtual offsets (chunk-map engine)
  uint32_t* ticket;           // arrival counters of the fused reduction (0 between launches)
  float* red_out;             // fused reduction target (chunk engine), NULL = none
  int32_t red_acc;            // accumulate into red_out
  int32_t red_fuse;           // R > 0: combine in-kernel (two-level ticket, R groups), no combine launch
  int32_t red_groups_only;    // stop after the group level: the R group sums stay for a clipped update
  int32_t red_raw;            // one partial per workgroup straight to red_out (no counters, no combine)
  int32_t n;
  int32_t n_chunks;
};

// One instantiation per dtype: NAME is a constexpr GS_* dtype inside the body.  For use
// in functions of namespace gs that return an int status.
#define GS_DISPATCH_FLOAT(DT, NAME, ...)                                \
  switch (DT) {                                                         \
    case GS_F32: { constexpr int NAME = GS_F32; __VA_ARGS__; break; }   \
    case GS_BF16: { constexpr int NAME = GS_BF16; __VA_ARGS__; break; } \
    case GS_F16: { constexpr int NAME = GS_F16; __VA_ARGS__; break; }   \
    default: return fail(GS_EINVAL, "unsupported floating dtype");      \
  }
// ... and the optional low-precision copy: -1 = none
#define GS_DISPATCH_LOWP(DT, NAME, ...)                                  \
  switch (DT) {                                                          \
    case -1: { constexpr int NAME = -1; __VA_ARGS__; break; }            \
    case GS_BF16: { constexpr int NAME = GS_BF16; __VA_ARGS__; break; }  \
    case GS_F16: { constexpr int NAME = GS_F16; __VA_ARGS__; break; }    \
    default: return fail(GS_EINVAL, "unsupported low-precision dtype");  \
  }

}  // namespace gs

// The opaque plan (visible to every TU of the library).
struct gs_plan {
  int kind = GS_DEV_HOST;
  int device = 0;
  int n = 0;
  int64_t align_elems = 0;
  int64_t flat_numel = 0;
  int64_t elems = 0;                   // Σ numel (the load policy's stream sizes)
  std::vector<int64_t> numel, off;
  std::vector<int64_t> voff;           // chunk-map engine: virtual offsets
  std::vector<gs::ChunkDesc> chunks;   // chunk-map engine: one per kChunkElems elements of voff space
  int grid_cap = gs::kMaxGrid;         // the streaming ops' grid cap
  // the public work decomposition (gs_plan_task_units / gs_plan_n_tasks): reported, not acted on
  int64_t task_units = 0;
  int n_tasks = 0;
  // host shadow of the pointer table
  std::vector<void*> h_ptrs;       // [SLOTS * n]
  std::vector<uint32_t> h_align;   // [n]
  bool dirty = true;
  // device side (HIP plans only)
  void* d_static = nullptr;  // numel | off | chunks | voff
  void* d_table = nullptr;   // ptrs | align
  float* d_partials = nullptr;  // [kGridLimit] partials + the fused reduction's sync words
  void* pinned = nullptr;       // staging ring for table uploads
  int ring = 0;
  void* ring_events[4] = {nullptr, nullptr, nullptr, nullptr};
  void* last_stream = nullptr;
  void* last_event = nullptr;   // recorded on last_stream only when a launch moves to another stream
  bool last_captured = false;   // the last launch was recorded into a stream capture
  // one-shot HIP events for the next launch (the bucketer's timeline): written by
  // that kernel's own dispatch (hipExtLaunchKernel start / stop), not as packets
  void* once_start = nullptr;
  void* once_stop = nullptr;
  // a collective's watchdog mark rides on this plan's next eager launch (its stop event):
  // the communicator that deferred it there (gs_allreduce_marked & co.), or NULL
  void* watch_comm = nullptr;
  unsigned long long table_capture_id = 0;  // capture that last recorded a table write
  bool in_graph = false;        // a graph holds a table write: re-upload before eager launches
  const float* hyper = nullptr; // device hyper-parameter source of sgd/adam (gs_plan_set_hyper_source)
  // clip folded into sgd/adam (gs_plan_set_clip); clip_own: Σg² from this plan's
  // group sums, left by its last gs_sqnorm_partial (red_groups of them)
  bool clip_on = false, clip_own = false;
  gs::ClipArgs clip{};
  int red_groups = 0;
  bool red_valid = false;       // a gs_sqnorm_partial has run on this plan
  bool grads_read = false;      // a Σg² pass read slot 1 since the last update (load policy)
  int read_hint = 0;            // Σg² loads: 0 the size rule, 1 non-temporal, 2 cached (gs_plan_set_read_hint)
  float h_red = 0.f;            // host plans: the Σg² of gs_sqnorm_partial
  // LARS and LAMB (gs_lars_norms / gs_lars_step, gs_lamb_moments / gs_lamb_step): the per-tensor adaptation flags (empty = all 1)
  // and, on HIP plans, the segmented reduction's scratch, allocated on first use:
  // d_lars = chunk slot bases | per-tensor [first slot, count] | adapt | partial slots
  std::vector<int32_t> adapt;
  void* d_lars = nullptr;
  int64_t lars_slots = 0;
  // launch timer ring (gs_plan_timer_enable)
  std::vector<void*> timer_ev;  // [2 * slots]: start, stop
  std::vector<int32_t> timer_kind;  // [slots]: GS_OP_* of the timed launch
  int timer_next = 0, timer_count = 0;
  gs::PlanArgs args() const;
};

namespace gs {
// ---- input step (gs_data.cpp / gs_data_kernels.hip) ----
#ifdef __HIPCC__
#define GS_HD __host__ __device__
#else
#define GS_HD
#endif
struct ImageAugArgs {
  const uint8_t* src;     // [n_src, H, W, C] uint8
  const int64_t* labels;  // [n_src] or NULL
  int64_t n_src;
  int H, W, C, pad, out_h, out_w;
  const int32_t* params;  // [B, 4] = (sample index, flip, top, left)
  int64_t B;
  void* out;              // [B, C, out_h, out_w] (NCHW) or [B, out_h, out_w, C] (NHWC)
  int out_dtype, layout;
  int64_t* out_labels;    // [B] or NULL
};
// Pad(pad, fill 0) -> hflip (of the padded image) -> crop(top, left) -> x/255
// for one output element (c, y, x) of sample idx; the same expression on the
// host and the device (IEEE division on both).
GS_HD inline float aug_pixel(const uint8_t* src, int64_t idx, int H, int W, int C, int pad, int flip,
                             int top, int left, int c, int y, int x) {
  const int wp = W + 2 * pad;
  const int px = flip ? (wp - 1 - (x + left)) : (x + left);
  const int sy = y + top - pad, sx = px - pad;
  if (sy < 0 || sy >= H || sx < 0 || sx >= W) return 0.f;
  return static_cast<float>(src[((idx * H + sy) * W + sx) * C + c]) / 255.f;
}
int hip_image_augment(int device, const ImageAugArgs& a, void* stream);

// gs_image_augment_mix: the batch of ImageAugArgs with a MixUp / CutMix record per sample.
struct ImageMixAugArgs : ImageAugArgs {
  const int32_t* mix;      // [B, 4] = (partner, lam as fp32 bits, y0 | y1 << 16, x0 | x1 << 16)
  int64_t* out_labels_b;   // [B] or NULL
  float* out_lam;          // [B] or NULL
};
// A sample's record as both backends read it.  The host backend has rejected what is invalid;
// the device cannot, so here a partner outside [0, B) or a lam outside [0, 1] (or NaN) makes
// the sample its own partner with lam 1, and a box is clamped to the output extent.
struct MixRec {
  int partner;
  float lam;
  int y0, y1, x0, x1;
  bool box;     // a non-empty box: paste the partner inside it
  bool need_b;  // the partner's image is read
};
GS_HD inline MixRec mix_decode(int32_t w0, int32_t w1, int32_t w2, int32_t w3, int64_t i, int64_t B, int out_h,
                               int out_w) {
  MixRec r;
  uint32_t lb = static_cast<uint32_t>(w1);
  float lam;
  __builtin_memcpy(&lam, &lb, 4);
  const bool ok = w0 >= 0 && w0 < B && lam >= 0.f && lam <= 1.f;
  r.partner = ok ? w0 : static_cast<int>(i);
  r.lam = ok ? lam : 1.f;
  const uint32_t ys = static_cast<uint32_t>(w2), xs = static_cast<uint32_t>(w3);
  const int y0 = static_cast<int>(ys & 0xffffu), y1 = static_cast<int>(ys >> 16);
  const int x0 = static_cast<int>(xs & 0xffffu), x1 = static_cast<int>(xs >> 16);
  r.y0 = y0 < out_h ? y0 : out_h;
  r.y1 = y1 < out_h ? y1 : out_h;
  r.x0 = x0 < out_w ? x0 : out_w;
  r.x1 = x1 < out_w ? x1 : out_w;
  r.box = ok && r.y0 < r.y1 && r.x0 < r.x1;
  r.need_b = r.partner != i && (r.box || r.lam != 1.f);
  return r;
}
// One output element from the sample's pixel a and the partner's pixel b (need_b holds):
// paste inside a box, else the blend, each multiply and the add rounded once.
GS_HD inline float mix_pixel(float a, float b, const MixRec& r, int y, int x) {
  if (r.box) return (y >= r.y0 && y < r.y1 && x >= r.x0 && x < r.x1) ? b : a;
  const float lam1 = 1.f - r.lam;
  return a * r.lam + b * lam1;
}
int hip_image_augment_mix(int device, const ImageMixAugArgs& a, void* stream);

// gs_image_resample: bilinear resized crop of a per-sample box (+ hflip, ToTensor, Normalize, bf16 cast).
struct ImageResampleArgs {
  const uint8_t* src;     // [n_src, H, W, C] uint8
  const int64_t* labels;  // [n_src] or NULL
  int64_t n_src;
  int H, W, C, out_h, out_w;
  int virt_h, virt_w, off_y, off_x;  // the virtual output frame: d_y = y + off_y, d_x = x' + off_x
  const int32_t* rec;     // [B, 4] = (sample index, flip, top | left << 16, h | w << 16)
  int64_t B;
  void* out;              // [B, C, out_h, out_w] (NCHW) or [B, out_h, out_w, C] (NHWC)
  int out_dtype, layout;
  int64_t* out_labels;    // [B] or NULL
  int normalize;          // (o - mean[c]) / std[c] follows the blend (C <= 4)
  float mean[4], std[4];
};
// A sample's record as both backends read it.  The host backend has rejected what is invalid; the
// device cannot, so here an index outside the set clears ok (zeros and label 0) and the box is
// clamped into the image: top <= H - 1, left <= W - 1, 1 <= h <= H - top, 1 <= w <= W - left.
struct ResampleBox {
  int idx, flip, top, left, h, w;
  bool ok;
};
GS_HD inline ResampleBox resample_decode(int32_t w0, int32_t w1, int32_t w2, int32_t w3, int64_t n_src, int H,
                                         int W) {
  ResampleBox r;
  r.ok = w0 >= 0 && w0 < n_src;
  r.idx = r.ok ? w0 : 0;
  r.flip = w1 != 0;
  const uint32_t tl = static_cast<uint32_t>(w2), hw = static_cast<uint32_t>(w3);
  const int top = static_cast<int>(tl & 0xffffu), left = static_cast<int>(tl >> 16);
  const int h = static_cast<int>(hw & 0xffffu), w = static_cast<int>(hw >> 16);
  r.top = top < H - 1 ? top : H - 1;
  r.left = left < W - 1 ? left : W - 1;
  r.h = h < 1 ? 1 : (h < H - r.top ? h : H - r.top);
  r.w = w < 1 ? 1 : (w < W - r.left ? w : W - r.left);
  return r;
}
// The two taps and weights of output coordinate d along an axis whose box extent is n, with
// scale = resample_scale(n, V) for the virtual output extent V (torch's bilinear,
// align_corners=False, antialias=False): every operation rounded once in fp32, no fma.
struct ResampleTap {
  int i0, i1;
  float l0, l1;
};
GS_HD inline float resample_scale(int n, int V) { return static_cast<float>(n) / static_cast<float>(V); }
GS_HD inline ResampleTap resample_tap(int d, float scale, int n) {
  ResampleTap t;
  float s = (static_cast<float>(d) + 0.5f) * scale - 0.5f;
  s = s > 0.f ? s : 0.f;
  const int i = static_cast<int>(s);
  t.i0 = i < n - 1 ? i : n - 1;
  t.i1 = t.i0 + 1 < n - 1 ? t.i0 + 1 : n - 1;
  t.l1 = s - static_cast<float>(t.i0);
  t.l0 = 1.f - t.l1;
  return t;
}
// float(u8) / 255.f without the division: the product with fl(1 / 255) and one Newton correction
// (the remainder is exact in the fma).  Equal to the IEEE quotient, bit for bit, for all 256 bytes;
// the host backend keeps a table of true quotients, which the tests compare the device against.
GS_HD inline float resample_unit(uint8_t v) {
  const float x = static_cast<float>(v), r = 1.f / 255.f;
  const float q = x * r;
  return fmaf(fmaf(-q, 255.f, x), r, q);
}
// One output value from the four taps' quotients u8 / 255.f (p00 p01 on row i0, p10 p11 on row i1)
GS_HD inline float resample_blend(float p00, float p01, float p10, float p11, const ResampleTap& ty,
                                  const ResampleTap& tx) {
  const float t = p00 * tx.l0 + p01 * tx.l1;
  const float u = p10 * tx.l0 + p11 * tx.l1;
  return t * ty.l0 + u * ty.l1;
}
GS_HD inline float resample_norm(float o, float mean, float std) { return (o - mean) / std; }
// output element k of a sample -> (c, y, x) in the layout's order
GS_HD inline void resample_cyx(int layout, int64_t k, int C, int out_h, int out_w, int* c, int* y, int* x) {
  if (layout == GS_LAYOUT_NCHW) {
    *x = static_cast<int>(k % out_w);
    *y = static_cast<int>((k / out_w) % out_h);
    *c = static_cast<int>(k / (static_cast<int64_t>(out_w) * out_h));
  } else {
    *c = static_cast<int>(k % C);
    *x = static_cast<int>((k / C) % out_w);
    *y = static_cast<int>(k / (static_cast<int64_t>(C) * out_w));
  }
}
// One output element (c, y, x) of a decoded sample, its taps read from the image set through
// tab[u8] = float(u8) / 255.f (the quotients' bits, without four divisions per output)
GS_HD inline float resample_pixel(const ImageResampleArgs& a, const ResampleBox& r, float scale_y, float scale_x,
                                  const float* tab, int c, int y, int x) {
  const ResampleTap ty = resample_tap(y + a.off_y, scale_y, r.h);
  const ResampleTap tx = resample_tap((r.flip ? a.out_w - 1 - x : x) + a.off_x, scale_x, r.w);
  const uint8_t* img = a.src + static_cast<int64_t>(r.idx) * a.H * a.W * a.C;
  const uint8_t* r0 = img + (static_cast<int64_t>(r.top + ty.i0) * a.W + r.left) * a.C + c;
  const uint8_t* r1 = img + (static_cast<int64_t>(r.top + ty.i1) * a.W + r.left) * a.C + c;
  const float o = resample_blend(tab[r0[tx.i0 * a.C]], tab[r0[tx.i1 * a.C]], tab[r1[tx.i0 * a.C]],
                                 tab[r1[tx.i1 * a.C]], ty, tx);
  return a.normalize ? resample_norm(o, a.mean[c], a.std[c]) : o;
}
int hip_image_resample(int device, const ImageResampleArgs& a, void* stream);

// Adam's step-varying hyper-parameters from a device step counter (torch's
// capturable=True): step += 1 unless found_inf; then, in double as the host
// path forms them, hyper = [-(lr/bc1), sqrt(bc2), 1 - lr*wd] rounded to fp32.
GS_HD inline void adam_hyper_update(double* step, const double* lr, double beta1, double beta2,
                                    double wd, const float* found_inf, float* hyper) {
  double s = step[0];
  if (found_inf == nullptr || found_inf[0] == 0.f) s += 1.0;
  step[0] = s;
  const double bc1 = 1.0 - pow(beta1, s), bc2 = 1.0 - pow(beta2, s);
  hyper[0] = static_cast<float>((lr[0] / bc1) * -1.0);
  hyper[1] = static_cast<float>(sqrt(bc2));
  hyper[2] = static_cast<float>(1.0 - lr[0] * wd);
}
// LAMB's counterpart (gs_lamb_hyper): hyper = [lr, 1 - b1^step, sqrt(1 - b2^step)] rounded
// to fp32 (both corrections 1 when bias correction is off)
GS_HD inline void lamb_hyper_update(double* step, const double* lr, double beta1, double beta2,
                                    int bias_correction, const float* found_inf, float* hyper) {
  double s = step[0];
  if (found_inf == nullptr || found_inf[0] == 0.f) s += 1.0;
  step[0] = s;
  hyper[0] = static_cast<float>(lr[0]);
  hyper[1] = bias_correction ? static_cast<float>(1.0 - pow(beta1, s)) : 1.f;
  hyper[2] = bias_correction ? static_cast<float>(sqrt(1.0 - pow(beta2, s))) : 1.f;
}
int hip_adam_hyper(double* step, const double* lr, double beta1, double beta2, double wd,
                   const float* found_inf, float* hyper, void* stream);
// The averaging weight of gs_ema_step from the device update counter (gs_ema_hyper):
// hyper = [w, copy flag]; n_averaged advances.  EMA and the warm-up form their weight in
// double as Python does (1 - decay), SWA with the one fp32 division of 1 / (n + 1) on an
// int64 tensor.
GS_HD inline void ema_hyper_update(int64_t* n_averaged, int mode, double decay, float* hyper) {
  const int64_t n = n_averaged[0];
  float w;
  if (mode == GS_EMA_SWA) {
    w = 1.0f / static_cast<float>(n + 1);
  } else if (mode == GS_EMA_WARMUP) {
    const double ramp = (1.0 + static_cast<double>(n)) / (10.0 + static_cast<double>(n));
    w = static_cast<float>(1.0 - (decay < ramp ? decay : ramp));
  } else {
    w = static_cast<float>(1.0 - decay);
  }
  hyper[0] = w;
  hyper[1] = n == 0 ? 1.f : 0.f;
  n_averaged[0] = n + 1;
}
int hip_ema_hyper(int64_t* n_averaged, int mode, double decay, float* hyper, void* stream);
int hip_ema(gs_plan* p, int sdt, int ldt, float w, int copy, void* stream);
int host_ema(gs_plan* p, int sdt, int ldt, float w, int copy);

// ---- evaluation metrics (gs_eval_accumulate: gs_eval_kernels.hip / gs_host.cpp) ----
// A row's result in the caller's scratch: its loss and its label's rank, or why it is not counted.
struct EvalRow {
  float loss;
  int32_t code;  // >= 0: the rank (kEvalNanRow: a NaN in the row, never a hit); < 0: not counted
};
static_assert(sizeof(EvalRow) == 8, "EvalRow layout");
constexpr int32_t kEvalSkip = -1;  // past n_valid, or the label is ignore_index
constexpr int32_t kEvalBad = -2;   // the label is outside [0, K)
constexpr int32_t kEvalNanRow = INT32_MAX;
struct EvalTopk {
  int32_t n;
  int32_t k[4];
};
// logsumexp(z) - z_y from the row's maximum m, S = sum expf(z - m) and z_y, in fp32
GS_HD inline float eval_loss(float m, float s, float zy) { return (m - zy) + logf(s); }
int hip_eval_accumulate(const void* logits, int dt, const int64_t* labels, int64_t B, int K, int64_t row_stride,
                        int64_t n_valid, const EvalTopk& topk, int64_t ignore_index, void* ws, void* acc,
                        void* stream);
int host_eval_accumulate(const void* logits, int dt, const int64_t* labels, int64_t B, int K, int64_t row_stride,
                         int64_t n_valid, const EvalTopk& topk, int64_t ignore_index, void* ws, void* acc);

// ---- training criterion (gs_xent_fwd / gs_xent_bwd: gs_loss_kernels.hip / gs_host.cpp) ----
// A row's forward result: what the backward needs to rebuild the softmax, and the row's code
// (EvalRow's rules).  A skipped or bad row is {0, 0, 0, code}; a NaN row is all NaN.
struct XentRow {
  float loss, m, logS;
  int32_t code;
};
static_assert(sizeof(XentRow) == 16, "XentRow layout");
struct XentRed {
  float loss_sum, loss_mean;
  int32_t counted, bad;
};
static_assert(sizeof(XentRed) == 16, "XentRed layout");
constexpr int kXentNone = 0, kXentMean = 1, kXentSum = 2;
// the smoothed loss of a counted row from nll = (m - z_y) + logS and T = sum z_j; every
// multiply and add is its own rounding (-ffp-contract=off).  eps == 0: T is not looked at.
GS_HD inline float xent_loss(float m, float logS, float zy, float T, int K, float eps) {
  const float nll = (m - zy) + logS;
  if (eps == 0.f) return nll;
  const float smooth = (m + logS) - T / static_cast<float>(K);
  return (1.f - eps) * nll + eps * smooth;
}
// the reduced loss from the fp64 total of the counted rows' losses
GS_HD inline XentRed xent_reduce(double total, int64_t counted, int64_t bad) {
  XentRed r;
  const float nanf32 = static_cast<float>(NAN);
  r.loss_sum = bad ? nanf32 : static_cast<float>(total);
  r.loss_mean = (bad || counted == 0) ? nanf32 : static_cast<float>(total / static_cast<double>(counted));
  r.counted = static_cast<int32_t>(counted);
  r.bad = static_cast<int32_t>(bad);
  return r;
}
// a gradient element: c * (p - q), p = expf((z - m) - logS), each step rounded once
GS_HD inline float xent_grad(float z, float m, float logS, float q, float c) {
  const float p = expf((z - m) - logS);
  return c * (p - q);
}
// ---- pair targets (gs_xent_mix_fwd / gs_xent_mix_bwd): labels a and b and a's weight lam ----
// the code of a row that is not counted, or 0: skipped if either label is ignore_index, else bad
// if either is outside [0, K) or lam is outside [0, 1] or NaN
GS_HD inline int32_t xent_mix_code(int64_t a, int64_t b, float lam, int K, int64_t ignore_index) {
  if (a == ignore_index || b == ignore_index) return kEvalSkip;
  if (a < 0 || a >= K || b < 0 || b >= K || !(lam >= 0.f && lam <= 1.f)) return kEvalBad;
  return 0;
}
// a one-label row: exactly the one-label entries' row for label a
GS_HD inline bool xent_mix_one(int64_t a, int64_t b, float lam) { return lam == 1.f || a == b; }
// the label Metrics count top-k against
GS_HD inline int64_t xent_mix_dominant(int64_t a, int64_t b, float lam) { return lam >= 0.5f ? a : b; }
// a mixed row's loss from its two one-label losses
GS_HD inline float xent_mix_loss(float m, float logS, float za, float zb, float lam, float T, int K, float eps) {
  const float lam1 = 1.f - lam;
  return lam * xent_loss(m, logS, za, T, K, eps) + lam1 * xent_loss(m, logS, zb, T, K, eps);
}
// a mixed row's target at one of its two labels, w = lam or 1 - lam
GS_HD inline float xent_mix_q(float eps, float w, float q_off) { return (1.f - eps) * w + q_off; }
int hip_xent_fwd(const void* logits, int dt, const int64_t* labels, int64_t B, int K, int64_t row_stride,
                 int64_t ignore_index, float eps, void* rows, void* red, const EvalTopk& topk, void* acc,
                 void* stream);
int hip_xent_bwd(const void* logits, int dt, const int64_t* labels, int64_t B, int K, int64_t row_stride, float eps,
                 int reduction, const void* rows, const void* red, const float* grad_out, void* dlogits,
                 int64_t d_row_stride, void* stream);
// pair targets; the host functions serve the one-label entries too (labels_b and lam null)
int hip_xent_mix_fwd(const void* logits, int dt, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                     int64_t B, int K, int64_t row_stride, int64_t ignore_index, float eps, void* rows, void* red,
                     const EvalTopk& topk, void* acc, void* stream);
int host_xent_mix_fwd(const void* logits, int dt, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                      int64_t B, int K, int64_t row_stride, int64_t ignore_index, float eps, void* rows, void* red,
                      const EvalTopk& topk, void* acc);
int hip_xent_mix_bwd(const void* logits, int dt, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                     int64_t B, int K, int64_t row_stride, float eps, int reduction, const void* rows, const void* red,
                     const float* grad_out, void* dlogits, int64_t d_row_stride, void* stream);
int host_xent_mix_bwd(const void* logits, int dt, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                      int64_t B, int K, int64_t row_stride, float eps, int reduction, const void* rows,
                      const void* red, const float* grad_out, void* dlogits, int64_t d_row_stride);

// Deferred watchdog marks (gs_comm.cpp): a consumer plan's launch carries the mark of
// the collectives deferred to it.  comm_mark_take: 0 = nothing to do (the
// communicator is gone or not watching), 1 = carry *ev as the launch's stop event
// (*ev NULL: every mark of the ring is still pending — comm_mark_commit then records a
// pooled packet after the launch instead).  comm_mark_commit hands the carried event
// (or that packet) to the watchdog.
int comm_mark_take(gs_comm* c, void** ev);
// a destroyed communicator's stream (its work finished before the destroy, which
// synchronises it): a plan whose last launch ran there records nothing on it
bool stream_destroyed(void* stream);
// consumer: the launching plan — the collectives deferred to it are covered by its mark,
// timed from the oldest one's enqueue (a deferral whose consumer has not launched within
// about a second gets a packet from the watchdog instead)
int comm_mark_commit(gs_comm* c, void* ev, void* stream, const gs_plan* consumer);
// a plan being destroyed: collectives deferred to it keep only the watchdog's packet
void comm_forget_consumer(const gs_plan* consumer);

// HIP-side implementations (gs_kernels.hip)
int hip_plan_upload_static(gs_plan* p);
int hip_plan_release(gs_plan* p);
int hip_plan_flush(gs_plan* p, void* stream);
bool stream_capturing(void* stream);  // hipStreamIsCapturing: recording into a hipGraph
int hip_plan_timer_enable(gs_plan* p, int n_slots);
int hip_plan_timer_read(gs_plan* p, float* ms_out, int32_t* kind_out, int cap);
int hip_pack(gs_plan* p, int src_slot, int src_dt, void* flat, int flat_dt, float s, int mode,
             void* stream);
int hip_unpack(gs_plan* p, const void* flat, int flat_dt, int dst_slot, int dst_dt, float* sq,
               int acc, void* stream);
int hip_unpack_check(gs_plan* p, const void* flat, int flat_dt, int dst_slot, int dst_dt, float* found,
                     void* stream);
int hip_scale(gs_plan* p, int slot, int dt, float s, int mode, void* stream);
int hip_sqnorm(gs_plan* p, int slot, int dt, float* sq, int acc, void* stream);
int hip_sum(gs_plan* p, int slot, int dt, float* out, int acc, void* stream);
int hip_clip_coef(const float* sq, float max_norm, float eps, float* coef, float* norm,
                  void* stream);
int hip_unscale_check(gs_plan* p, int slot, int dt, const float* inv, float* found,
                      void* stream);
int hip_clip_scale(gs_plan* p, int slot, int dt, const ClipArgs& clip, void* stream);
int hip_sqnorm_partial(gs_plan* p, int slot, int dt, float* groups_out, int32_t* n_groups, void* stream);
const float* hip_plan_red_groups(const gs_plan* p);  // the <= 64 group sums of gs_sqnorm_partial, contiguous
float* hip_plan_red_scalar(const gs_plan* p);        // its finished Σ when red_groups == 0
int hip_sgd(gs_plan* p, int gdt, int ldt, const SgdHyper& h, const float* gs, const float* fi,
            const ClipArgs* clip, void* stream);
int hip_adam(gs_plan* p, int gdt, int ldt, const AdamHyper& h, const float* gs, const float* fi,
             const ClipArgs* clip, void* stream);
int hip_lars_set_adapt(gs_plan* p);  // upload p->adapt (allocates the LARS scratch on first use)
int hip_lars_norms(gs_plan* p, int gdt, float* norms, void* stream);
int hip_lars(gs_plan* p, int gdt, int ldt, const LarsHyper& h, const float* norms, const float* gs, const float* fi,
             void* stream);
int hip_lamb_moments(gs_plan* p, int gdt, const LambHyper& h, float* norms, const float* gs, const float* fi,
                     void* stream);
int hip_lamb(gs_plan* p, int ldt, const LambHyper& h, const float* norms, const float* fi, void* stream);
int hip_lamb_hyper(double* step, const double* lr, double beta1, double beta2, int bias_correction,
                   const float* found_inf, float* hyper, void* stream);
int hip_device_count();
int hip_memset_async(void* dst, int value, size_t bytes, void* stream);
int hip_stream_wait(void* waiter, void* signaler);

// host-side implementations (gs_host.cpp)
int host_pack(gs_plan* p, int src_slot, int src_dt, void* flat, int flat_dt, float s, int mode);
int host_unpack(gs_plan* p, const void* flat, int flat_dt, int dst_slot, int dst_dt, float* sq,
                int acc);
int host_unpack_check(gs_plan* p, const void* flat, int flat_dt, int dst_slot, int dst_dt, float* found);
int host_scale(gs_plan* p, int slot, int dt, float s, int mode);
int host_clip_scale(gs_plan* p, int slot, int dt, const ClipArgs& clip);
int host_sqnorm(gs_plan* p, int slot, int dt, float* sq, int acc);
int host_sum(gs_plan* p, int slot, int dt, float* out, int acc);
int host_clip_coef(const float* sq, float max_norm, float eps, float* coef, float* norm);
int host_unscale_check(gs_plan* p, int slot, int dt, const float* inv, float* found);
int host_sgd(gs_plan* p, int gdt, int ldt, const SgdHyper& h, const float* gs, const float* fi,
             const ClipArgs* clip);
int host_adam(gs_plan* p, int gdt, int ldt, const AdamHyper& h, const float* gs, const float* fi,
              const ClipArgs* clip);
int host_lars_norms(gs_plan* p, int gdt, float* norms);
int host_lars(gs_plan* p, int gdt, int ldt, const LarsHyper& h, const float* norms, const float* gs, const float* fi);
int host_lamb_moments(gs_plan* p, int gdt, const LambHyper& h, float* norms, const float* gs, const float* fi);
int host_lamb(gs_plan* p, int ldt, const LambHyper& h, const float* norms, const float* fi);
// the clip coefficient of ClipArgs on the host (groups == 0: *sq is final)
float host_clip_factor(const ClipArgs& c, const float* gs);
// the device's 64-lane DPP fold (gs_kernels.hip wave_reduce) restated on the
// host: lane l holds x[l * stride] (l < n), zeros elsewhere
float host_wave_sum(const float* x, int n, int stride);
}  // namespace gs
