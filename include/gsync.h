/*
 * gsync.h — C-ABI of libgsync, the MI355X-native data-parallel
 * gradient-synchronisation engine (bucketer + RCCL collectives + fused
 * multi-tensor optimizer) behind the reference's DDP / ZeRO training wrappers.
 *
 * Every entry point replaces a native piece of the reference's path (the
 * reference itself is Python; its hot path lives in torch's c10d Reducer,
 * ProcessGroupNCCL and the ATen foreach/fused optimizer kernels — see
 * SURVEY.md §2.4 / §8a).  The "replaces:" line on each declaration names the
 * reference-side interface (file:line; R: = /root/reference,
 * T: = torch 2.10 under dist-packages/torch).
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = error (GS_E*); the message is
 *     in gs_last_error() (thread-local).  No C++ exception crosses the ABI.
 *   - device memory is owned by the caller (torch caching allocator); the
 *     library only receives raw pointers.  The library owns communicators,
 *     streams, events and its own small metadata tables.
 *   - `stream` arguments are hipStream_t passed as void* (NULL = legacy
 *     default stream).  No entry point synchronises the host with the device
 *     except *_destroy and gs_comm_create.
 *   - device_kind GS_DEV_HIP runs hand-written gfx950 kernels; GS_DEV_HOST
 *     runs the host implementation used for CPU tensors (the gloo/CPU
 *     config).  A HIP plan never falls back to the host implementation.
 */
#ifndef GSYNC_H
#define GSYNC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSYNC_VERSION 1000 /* 0.1.0 */

/* ---- error codes ---- */
#define GS_OK 0
#define GS_EINVAL (-1)   /* bad argument (TORCH_CHECK equivalent) */
#define GS_EHIP (-2)     /* HIP runtime error */
#define GS_ERCCL (-3)    /* RCCL error */
#define GS_ESTATE (-4)   /* call out of protocol order (Reducer REDUCER_CHECK equivalent) */
#define GS_ENOMEM (-5)
#define GS_ENODEV (-6)   /* HIP requested but no device / library built without it */

/* ---- dtypes ---- */
#define GS_F32 0
#define GS_BF16 1
#define GS_F16 2
#define GS_F64 3
#define GS_I64 4
#define GS_I32 5
#define GS_U8 6

/* threads the host implementation (GS_DEV_HOST plans) may use; torch's
 * intra-op thread count is passed by the Python layer (default 1) */
int gs_set_host_threads(int n);

/* ---- device kinds ---- */
#define GS_DEV_HOST 0
#define GS_DEV_HIP 1

/* ---- reduce ops (ncclRedOp_t order) ---- */
#define GS_SUM 0
#define GS_PROD 1
#define GS_MAX 2
#define GS_MIN 3
#define GS_AVG 4

/* ---- scale modes for pack / scale ---- */
#define GS_SCALE_NONE 0
#define GS_SCALE_MUL 1 /* x * s  — Reducer pack: at::mul_out(bucket_view, grad, 1/div_factor) */
#define GS_SCALE_DIV 2 /* x / s  — Reducer view mode: bucket_view.div_(div_factor) */

typedef struct gs_comm gs_comm;
typedef struct gs_plan gs_plan;
typedef struct gs_bucketer gs_bucketer;

/* ======================================================================
 * library
 * ==================================================================== */
int gs_version(void);
const char* gs_last_error(void);
/* number of HIP devices visible (0 on a CPU-only host) */
int gs_device_count(void);

/* ======================================================================
 * communicator: RCCL over xGMI with a library-owned stream
 * replaces: T:include/torch/csrc/distributed/c10d/ProcessGroupNCCL.hpp:849
 *           (allreduce), :836 (broadcast), :872 (_allgather_base),
 *           :887-892 (reduce_scatter / _reduce_scatter_base),
 *           per-device NCCL streams ncclStreams_ :1398
 * ==================================================================== */
int gs_comm_unique_id_bytes(void); /* 128 */
int gs_comm_get_unique_id(uint8_t* out /* [gs_comm_unique_id_bytes()] */);
int gs_comm_create(int rank, int world, const uint8_t* uid, int device, gs_comm** out);
/* The same with RCCL's per-collective workgroup (CTA) cap (ncclConfig_t
 * maxCTAs; <= 0: RCCL's default): fewer CUs taken from the backward kernels the
 * in-step collectives overlap.  Replaces ProcessGroupNCCL's Options::config
 * (an ncclConfig_t handed to ncclCommInitRankConfig,
 * T:include/torch/csrc/distributed/c10d/ProcessGroupNCCL.hpp:531). */
int gs_comm_create_ex(int rank, int world, const uint8_t* uid, int device, int max_ctas, gs_comm** out);
int gs_comm_destroy(gs_comm* c);
/* ncclCommAbort: for the failure path (timeout / peer death) */
int gs_comm_abort(gs_comm* c);
/* failure detection: with timeout_ms > 0 a watchdog thread aborts the
 * communicator (ncclCommAbort) when a collective enqueued through it has been
 * in flight longer than timeout_ms, or RCCL reports an asynchronous error;
 * later calls then fail with GS_ERCCL.  0 disables the timeout.  A
 * collective called through this API is followed by an event on its stream
 * for the watchdog to poll; the bucketer's collectives are instead watched
 * through the stop event their unpack kernel carries (no event packet between
 * a bucket's collective and its unpack).
 * replaces: ProcessGroupNCCL's watchdog / TORCH_NCCL_ASYNC_ERROR_HANDLING
 *           (T:include/torch/csrc/distributed/c10d/ProcessGroupNCCL.hpp:59-68, :156) */
int gs_comm_set_timeout(gs_comm* c, int64_t timeout_ms);
/* Pause (1) / resume (0) every communicator's watchdog event polling,
 * process-wide and counted: bracket a global-mode hipGraph capture with it,
 * since event queries from the watchdog thread are illegal while another
 * thread records (collectives recorded into a graph are not tracked).
 * replaces: ProcessGroupNCCL's capture-time watchdog exclusion
 *           (T:.../c10d/ProcessGroupNCCL.cpp, "graph capture" handling) */
int gs_watchdog_pause(int pause);
/* 1 if aborted (reason copied into `reason`, NUL-terminated), 0 if live */
int gs_comm_status(gs_comm* c, char* reason, int cap);
int gs_comm_rank(gs_comm* c);
int gs_comm_world(gs_comm* c);
/* the dedicated collective stream (hipStream_t) */
int gs_comm_stream(gs_comm* c, void** stream_out);
/* make `waiter` wait for all work queued so far on `signaler` (event edge) */
int gs_stream_wait(void* waiter, void* signaler);

/* collectives on `stream` (NULL = the legacy default stream, like every
 * stream argument; gs_comm_stream() gives the communicator's own stream).
 * count in elements. */
int gs_allreduce(gs_comm* c, const void* send, void* recv, int64_t count, int dtype, int op,
                 void* stream);
int gs_reduce_scatter(gs_comm* c, const void* send, void* recv, int64_t recv_count, int dtype,
                      int op, void* stream);
int gs_all_gather(gs_comm* c, const void* send, void* recv, int64_t send_count, int dtype,
                  void* stream);
/* The same collectives with their watchdog mark deferred to a consumer kernel:
 * with a watchdog running, no event packet follows the collective (~4.7 µs of
 * stream time on the step's end each); `consumer`'s next launch
 * carries the communicator's mark as its own stop event instead and hands it
 * to the watchdog.  The caller guarantees that launch is stream-ordered after
 * the collective (ZeRO: the partials all-reduce before the clipped update on the
 * same stream; the parameter all-gather before the next backward's first pack).
 * If that launch has not come within half the timeout (at most 1 s), the watchdog
 * records a packet on `stream` itself and times the collective from its enqueue, so
 * `stream` must outlive that window (as a plan's last stream, gs_plan_destroy).
 * NULL consumer (or an empty plan, a capture): a packet, as the entry points above.
 * replaces: ProcessGroupNCCL's per-work end event (T:.../ProcessGroupNCCL.hpp:424
 *           ncclEndEvent_), recorded after every collective */
int gs_allreduce_marked(gs_comm* c, const void* send, void* recv, int64_t count, int dtype, int op,
                        void* stream, gs_plan* consumer);
int gs_all_gather_marked(gs_comm* c, const void* send, void* recv, int64_t send_count, int dtype,
                         void* stream, gs_plan* consumer);
int gs_broadcast(gs_comm* c, const void* send, void* recv, int64_t count, int dtype, int root,
                 void* stream);

/* ======================================================================
 * multi-tensor plan: a static list of tensor shapes laid out in one flat
 * buffer (per-tensor offsets aligned to `align_elems`, 0 = packed back to
 * back like torch's _flatten_dense_tensors / Reducer bucket), plus up to
 * GS_PLAN_SLOTS per-tensor pointer tables (param / grad / state...).
 * The chunk map the kernels walk is built once on the host and uploaded
 * once; pointer tables are re-uploaded only when they change.
 * replaces: T:include/ATen/native/cuda/MultiTensorApply.cuh:14-21 launch
 *           geometry (kILP 4, 64Ki-element chunks, <=110 tensors/launch)
 * ==================================================================== */
#define GS_PLAN_SLOTS 5
int gs_plan_create(int device_kind, int device, int n_tensors, const int64_t* numels,
                   int64_t align_elems, gs_plan** out);
/* as gs_plan_create, with the work decomposition's task size pinned
 * (task_units units of 4 elements per task; 0 = automatic: ~1920 tasks).
 * The value is reported (gs_plan_task_units, gs_plan_n_tasks), not acted
 * on: the kernels walk the chunk map whatever the task size. */
int gs_plan_create_ex(int device_kind, int device, int n_tensors, const int64_t* numels,
                      int64_t align_elems, int64_t task_units, gs_plan** out);
/* Stream lifetime: a plan orders a launch on a new stream after its previous
 * launch by recording an event on the PREVIOUS launch's stream at that point
 * (no packet after every launch), and gs_plan_destroy synchronises on it.  So
 * the stream of a plan's last launch must stay alive until the plan's next
 * launch on another stream, or until gs_plan_destroy. */
int gs_plan_destroy(gs_plan* p);
int64_t gs_plan_flat_numel(gs_plan* p);
int gs_plan_offsets(gs_plan* p, int64_t* out /* [n_tensors] */);
int gs_plan_n_tasks(gs_plan* p);
/* units (4 elements) per task of the plan's work decomposition */
int64_t gs_plan_task_units(gs_plan* p);
/* launch timer: when enabled (n_slots > 0) every kernel launched through the
 * plan is bracketed by a pair of timing HIP events recorded on the launch
 * stream, immediately around the kernel (after any pointer-table upload), in
 * a ring of n_slots pairs; n_slots = 0 disables and frees them.
 * gs_plan_timer_read waits for the recorded pairs and writes up to `cap`
 * durations (ms, oldest first) and, if kind_out is not NULL, the GS_OP_* of
 * each timed launch; returns how many it wrote, then clears.
 * (bench.py's roofline.avg_launch_ms; no torch counterpart.) */
#define GS_OP_PACK 1
#define GS_OP_UNPACK 2
#define GS_OP_SCALE 3
#define GS_OP_SQNORM 4
#define GS_OP_UNSCALE 5
#define GS_OP_SGD 6
#define GS_OP_ADAM 7
#define GS_OP_SUM 8
#define GS_OP_LARS_NORM 9 /* gs_lars_norms: the segmented reduction and its finishing kernel, one record */
#define GS_OP_LARS 10
#define GS_OP_LAMB_MOMENTS 11 /* gs_lamb_moments: the chunk pass and its fold, one record */
#define GS_OP_LAMB 12
#define GS_OP_EMA 13
int gs_plan_timer_enable(gs_plan* p, int n_slots);
int gs_plan_timer_read(gs_plan* p, float* ms_out, int32_t* kind_out, int cap);
/* register the per-tensor pointers of one slot (uploads on change, ordered on `stream`) */
int gs_plan_set_ptrs(gs_plan* p, int slot, void* const* ptrs, void* stream);

/* flatten + fused scale + dtype cast: flat[off_t + i] = cast(src_t[i] (*|/) scale)
 * replaces: Reducer::mark_variable_ready_dense (T:.../c10d/reducer.hpp:275,
 *           upstream at::mul_out(bucket_view, grad, 1/div_factor_));
 *           T:_utils.py:558 _flatten_dense_tensors */
int gs_pack(gs_plan* p, int src_slot, int src_dtype, void* flat, int flat_dtype, float scale,
            int scale_mode, void* stream);
/* unflatten + cast: dst_t[i] = cast(flat[off_t + i]); if sqnorm_dev != NULL,
 * Σ dst² (fp32) is written (accumulate=0) or added (accumulate=1) to sqnorm_dev[0]
 * replaces: Reducer::copy_bucket_to_grad / finalize_bucket_dense (T:reducer.hpp:283,329);
 *           T:_utils.py:578 _unflatten_dense_tensors */
int gs_unpack(gs_plan* p, const void* flat, int flat_dtype, int dst_slot, int dst_dtype,
              float* sqnorm_dev, int accumulate, void* stream);
/* unflatten + cast with the AMP non-finite check of the written grads fused:
 * found_inf[0] = max(found_inf[0], any dst non-finite ? 1 : 0)
 * replaces: copy_bucket_to_grad + GradScaler's _amp_foreach_non_finite_check_and_unscale_
 *           check pass (T:amp/grad_scaler.py:280) over the same grads */
int gs_unpack_check(gs_plan* p, const void* flat, int flat_dtype, int dst_slot, int dst_dtype,
                    float* found_inf, void* stream);
/* in-place x = x (*|/) s on one slot (view-mode bucket_view.div_(div_factor)) */
int gs_scale(gs_plan* p, int slot, int dtype, float s, int scale_mode, void* stream);
/* Σ x² over all tensors of one slot into sqnorm_dev[0] (fp32, deterministic order)
 * replaces: T:nn/utils/clip_grad.py:96 torch._foreach_norm (+ vector_norm of norms) */
int gs_sqnorm(gs_plan* p, int slot, int dtype, float* sqnorm_dev, int accumulate, void* stream);
/* Σ x over every tensor of a slot (fp32 accumulation, deterministic order):
 * the bucket checksum of the GSYNC_DEBUG mode (gs_bucketer_set_debug) */
int gs_sum(gs_plan* p, int slot, int dtype, float* sum_dev, int accumulate, void* stream);
/* Σ x² of one slot left inside the plan as partial sums (no combine launch,
 * nothing written to caller memory), for the next clipped gs_sgd_step /
 * gs_adam_step on the same plan and stream (gs_plan_set_clip with
 * sqnorm_dev = NULL): the update's workgroups fold the partials themselves.
 * replaces: T:nn/utils/clip_grad.py:96-109 (_foreach_norm + the norm of norms)
 *           when the norm only feeds the clip */
int gs_sqnorm_partial(gs_plan* p, int slot, int dtype, void* stream);
/* Gradient-norm clip folded into every later gs_sgd_step / gs_adam_step on
 * this plan (max_norm <= 0 turns it off).  The update forms, in every workgroup,
 *   sq   = sqnorm_dev[0]   (sqnorm_dev = NULL: the plan's gs_sqnorm_partial sums)
 *   sq  *= grad_scale² (if grad_scale_dev) * sq_mul;  norm = sqrt(sq)
 *   coef = min(1, max_norm/(norm + eps)) * grad_scale * coef_mul
 * and multiplies the grads by coef — the arithmetic of gs_clip_coef plus the
 * caller's scale multiplies, bit for bit, without the coefficient launch.
 * out_dev (nullable, fp32[3]) receives [sq, coef, norm] (written even when
 * found_inf skips the step).  sq_mul / coef_mul: host-side loss-scale factors
 * (ZeRO: (1/scale)², 1/scale), 1 = none.
 * replaces: T:nn/utils/clip_grad.py:165-174 (clip_coef, clamp, _foreach_mul_)
 *           DeepSpeed gradient_clipping (R:resnet/deepspeed/deepspeed_train.py:195) */
/* How the plan's Σg² kernels (gs_sqnorm, gs_sqnorm_partial, gs_sqnorm_partial_out)
 * load their slot: 0 (default) cached below the 256 MiB Infinity Cache and
 * non-temporal above it; 1 non-temporal (the grads were just written by
 * non-temporal stores — libgsync's unpack — or by backward, and are read once);
 * 2 cached (e.g. a shard RCCL's reduce-scatter just wrote).  Bits never change.
 * GS_NT_SQNORM in the environment overrides.  No reference counterpart (a load
 * policy of this implementation). */
int gs_plan_set_read_hint(gs_plan* p, int hint);
int gs_plan_set_clip(gs_plan* p, const float* sqnorm_dev, float max_norm, float eps, float sq_mul,
                     float coef_mul, float* out_dev);
/* The partial sums of Σx² over the plan, written out for a sharded optimizer:
 * groups_out (device memory of the plan's kind) must hold GS_RED_PARTIALS
 * floats; *n_groups (host) receives how many are valid, 1..GS_RED_PARTIALS,
 * and the call sets the slots past them to 0.
 * A plan of at most 4 Ki chunks (a ZeRO shard at N = 8: 3.2 M elements)
 * writes one partial per workgroup of a balanced grid (<= 1024 workgroups) —
 * no arrival counters, no in-kernel combine, nothing after the
 * streaming but one store per workgroup; a larger plan writes the fused
 * reduction's <= 64 group sums (gs_sqnorm_partial's kernel); 1 = a finished Σ
 * (host plans, a reduction without the in-kernel combine).  A sharded
 * optimizer SUM-all-reduces the whole GS_RED_PARTIALS-float buffer across its
 * ranks (a rank's n follows its own chunk map, so only a fixed length is the
 * same on every rank; the zero slots past a rank's n add nothing) and hands it
 * to gs_plan_set_clip_groups
 * (n_groups = GS_RED_PARTIALS): the global ‖g‖
 * of every shard with no combine launch and no scalar coefficient launch on the
 * step's exposed end.
 * replaces: DeepSpeed stage_1_and_2 get_grad_norm_direct (per-rank Σg² of the
 *           partition, all_reduce of the scalar, U) for gradient_clipping
 *           (R:resnet/deepspeed/deepspeed_train.py:195) */
#define GS_RED_GROUPS 64
#define GS_RED_PARTIALS 1024
int gs_sqnorm_partial_out(gs_plan* p, int slot, int dtype, float* groups_out, int32_t* n_groups,
                          void* stream);
/* gs_plan_set_clip with ‖g‖² = the fold of n_groups (<= GS_RED_PARTIALS)
 * partial sums at groups_dev (contiguous; typically gs_sqnorm_partial_out's,
 * summed over ranks): every update workgroup folds them in a fixed order —
 * lane l of one wave adds partials l, l + 64, l + 128, ..., then the fused
 * reduction's own 64-lane tree — so every rank forms the same coefficient. */
int gs_plan_set_clip_groups(gs_plan* p, const float* groups_dev, int32_t n_groups, float max_norm,
                            float eps, float sq_mul, float coef_mul, float* out_dev);
/* clip_grad_norm_'s scale pass: slot `slot` (dtype) *= the clip coefficient of
 * the plan's clip (gs_plan_set_clip / gs_plan_set_clip_groups, consumed as by a
 * clipped update), torch.clamp(max_norm / (‖g‖ + eps), max = 1): every
 * workgroup folds the Σg² partial sums itself, workgroup 0 publishes
 * [Σg², coef, norm] to the clip's out; a coefficient of exactly 1 writes
 * nothing (x * 1 == x).  With gs_sqnorm_partial before it, clip_grad_norm_ is
 * two launches: no combine, no coefficient kernel, no flag fill.
 * replaces: T:nn/utils/clip_grad.py:165-174 (clip_coef, clamp, _foreach_mul_) */
int gs_clip_scale(gs_plan* p, int slot, int dtype, void* stream);
/* coef_dev[0] = min(1, max_norm / (sqrt(sqnorm_dev[0]) + eps)); norm_dev (nullable) = sqrt
 * replaces: T:nn/utils/clip_grad.py:165-174 clip_coef / clamp */
int gs_clip_coef(int device_kind, const float* sqnorm_dev, float max_norm, float eps,
                 float* coef_dev, float* norm_dev, void* stream);
/* found_inf_dev[0] = 1.0 if any non-finite in slot, and (if inv_scale_dev) x *= inv_scale
 * replaces: T:amp/grad_scaler.py:280 _amp_foreach_non_finite_check_and_unscale_ */
int gs_unscale_check(gs_plan* p, int slot, int dtype, const float* inv_scale_dev,
                     float* found_inf_dev, void* stream);

/* fused SGD momentum / weight decay, one pass over (p, g, buf[, p_lowp]):
 *   g' = g*gscale (+ wd*p);  buf = first ? g' : mom*buf + (1-damp)*g';
 *   d = nesterov ? g' + mom*buf : buf;  p -= lr*d;  p_lowp = cast(p)
 * slots: 0 = param (f32), 1 = grad (grad_dtype), 2 = momentum buffer (f32, unused if mom==0),
 *        3 = optional low-precision param copy (lowp_dtype, -1 = none)
 * grad_scale_dev (nullable): multiplies g (clip coefficient / AMP unscale);
 * found_inf_dev (nullable): skip the whole step when *found_inf != 0.
 * replaces: T:optim/sgd.py:322-381 _single_tensor_sgd, :383-470 _multi_tensor_sgd */
int gs_sgd_step(gs_plan* p, int grad_dtype, int lowp_dtype, double lr, double momentum,
                double dampening, double weight_decay, int nesterov, int maximize, int first_step,
                const float* grad_scale_dev, const float* found_inf_dev, void* stream);
/* fused Adam / AdamW, one pass over (p, g, m, v[, p_lowp]) with torch's foreach arithmetic:
 *   (adamw) p *= 1 - lr*wd  |  (adam) g += wd*p
 *   m = lerp(m, g, 1-b1);  v = b2*v + (1-b2)*g*g;
 *   p += step_size * m / (sqrt(v)/bc2_sqrt + eps)       (step_size = -lr/bc1)
 * slots: 0 = p, 1 = g, 2 = exp_avg, 3 = exp_avg_sq, 4 = optional low-precision copy
 * Hyper-parameters are Python floats (double) and are rounded to fp32 exactly
 * where torch rounds them: 1-b1, 1-b2, 1-lr*wd are formed in double first.
 * replaces: T:optim/adam.py:554-800 _multi_tensor_adam (reference GPU default);
 *           T:include/ATen/native/cuda/fused_adam_utils.cuh:11-88 */
int gs_adam_step(gs_plan* p, int grad_dtype, int lowp_dtype, double lr, double beta1,
                 double beta2, double eps, double weight_decay, int adamw, int maximize,
                 double step_size, double bias_correction2_sqrt, const float* grad_scale_dev,
                 const float* found_inf_dev, void* stream);
/* LARS (You et al. 2017, layer-wise adaptive rate scaling; the MLPerf ResNet-50
 * large-batch optimizer): SGD with momentum whose learning rate is multiplied,
 * per tensor, by the trust ratio eta*‖w‖ / (‖g‖ + wd*‖w‖).  Three entry points:
 * the per-tensor adaptation flags, the per-tensor Σp² / Σg² (one pass over slots
 * 0 and 1, 8 B/param with fp32 grads), and the update (one pass over p, g, buf,
 * 20 B/param), each update workgroup forming its tensor's ratio itself.
 *
 * Arithmetic (all fp32; every multiply and add rounded once, NO fma, so a
 * float32 restatement is exact op for op).  Per tensor t:
 *   sp = Σ p_i*p_i   sg = Σ g_i*g_i    (g converted from grad_dtype, before any
 *                                       multiplier; fp32 sums in the plan's fixed order)
 *   wn = sqrt(sp)    gn = sqrt(sg);    if grad_scale_dev (m = *grad_scale_dev): gn = gn*m
 *   adapt[t] != 0:  wd_t = wd; ratio = (wn > 0 && gn > 0) ? (eta*wn) / ((gn + wd*wn) + eps) : 1
 *   adapt[t] == 0:  wd_t = 0;  ratio = 1
 *   slr = lr * ratio
 * per element:
 *   g = g_i; if (m) g = g*m; if (wd_t != 0) g = g + wd_t*p
 *   mom != 0: b = b*mom + g; d = b    (the buffer starts as zeros: no first-step branch)
 *   mom == 0: d = g                   (slot 2 is not touched)
 *   p = p - slr*d
 * sqrt and / are the correctly rounded IEEE forms; m is assumed positive (an AMP
 * inverse scale); non-finite norms get no special handling.  A tensor of 0
 * elements has sums of 0 and is otherwise untouched.
 *
 * Determinism: the per-tensor sums are formed in an order fixed by the plan alone
 * (one partial per (1 Ki-element chunk, tensor) pair, a fixed tree inside it, then
 * a fixed fold of the tensor's partials) — no floating-point atomics, nothing
 * that depends on the grid or on arrival order — so data-parallel replicas that
 * hold the same averaged grads form the same ratios and stay bit-identical.  The
 * host backend's order is fixed too (element order) but is not the device's.
 *
 * Sharded tensors (ZeRO): a plan may hold the pieces of tensors that fall into one
 * rank's shard (entries of 0 elements for tensors the rank holds nothing of).  The
 * sums of a piece are partial; the caller SUM-all-reduces the fp32[2n] vector between
 * gs_lars_norms and the update, after which every rank holds the same bits and forms
 * the same ratios.  The order stays fixed: per rank by its plan, across ranks by the
 * collective's.
 *
 * Not part of LARS here: gradient-norm clipping (a clip set on the plan is
 * GS_ESTATE), nesterov.
 *
 * gs_plan_set_adapt: per-tensor adaptation flags (int32[n], host memory), static
 * for the plan; default all 1.  Not capturable (it uploads synchronously); on a
 * HIP plan it also allocates the plan's LARS scratch, which otherwise happens at
 * the first gs_lars_norms (plans that never call either pay nothing).
 * replaces: the `if p.ndim > 1` / exclude-list test of a Python LARS loop */
int gs_plan_set_adapt(gs_plan* p, const int32_t* adapt);
/* norms_out: fp32[2*n] in the plan's memory kind: [2t] = Σp², [2t+1] = Σg² of tensor t
 * (slot 0 = params, fp32; slot 1 = grads, grad_dtype).  Two launches (the chunk pass,
 * the per-tensor fold), no host sync; recordable into a hipGraph once the scratch exists.
 * replaces: the per-parameter torch.norm(p), torch.norm(p.grad) pair of a Python
 *           LARS (torch._foreach_norm x 2: T:nn/utils/clip_grad.py:96 is its only
 *           fused form, and that collapses to one scalar) */
int gs_lars_norms(gs_plan* p, int grad_dtype, float* norms_out, void* stream);
/* the update above; slots: 0 = param (f32), 1 = grad (grad_dtype), 2 = momentum
 * buffer (f32, unused if momentum == 0).  norms: gs_lars_norms' output for these
 * p and g.  found_inf_dev (nullable): *found_inf != 0 writes nothing.  With a
 * hyper source on the plan (gs_plan_set_hyper_source) lr is hyper[0], as for SGD.
 * replaces: the foreach update of a Python LARS (per parameter: trust ratio,
 *           grad.add(p, alpha=wd), buf.mul_(mom).add_(g), p.add_(buf, alpha=-lr*ratio)) */
int gs_lars_step(gs_plan* p, int grad_dtype, double lr, double momentum, double weight_decay,
                 double trust_coefficient, double eps, const float* norms,
                 const float* grad_scale_dev, const float* found_inf_dev, void* stream);
/* gs_lars_step that also writes slot 3 = a low-precision copy of the new p (lowp_dtype
 * GS_BF16 / GS_F16; -1 = none, and then this IS gs_lars_step: the same kernel).  The
 * fp32 arithmetic is gs_lars_step's, unchanged; p_lowp[i] = cast(p_new[i]), round to
 * nearest even, as gs_sgd_step / gs_adam_step write theirs.  The copy pointer may be
 * 2-byte aligned (a stream that is not 16-B aligned takes the element-wise path).
 * *found_inf != 0 writes nothing, the copy included.  A clip on the plan stays GS_ESTATE.
 * replaces: the `p_lowp.copy_(p_master)` (torch._foreach_copy_) behind a Python LARS on
 *           fp32 master weights (DeepSpeed / ColossalAI mixed-precision optimizers) */
int gs_lars_step_lowp(gs_plan* p, int grad_dtype, int lowp_dtype, double lr, double momentum,
                      double weight_decay, double trust_coefficient, double eps, const float* norms,
                      const float* grad_scale_dev, const float* found_inf_dev, void* stream);
/* Step-varying hyper-parameters from memory instead of the arguments: with a
 * non-NULL source, every later gs_sgd_step / gs_adam_step on this plan reads
 *   SGD:  hyper[0] = lr; hyper[1] = "first step" flag (buf = g) when gs_sgd_step
 *         is called with first_step = -1 — the AMP path keeps it on the device
 *         (cleared by the caller after a step that was not skipped)
 *   Adam: hyper[0] = step_size (-lr/bc1), hyper[1] = bias_correction2_sqrt,
 *         hyper[2] = 1 - lr*wd (AdamW decay)
 *   LARS: hyper[0] = lr
 *   LAMB: hyper[0] = lr, hyper[1] = bc1, hyper[2] = bc2_sqrt (gs_lamb_hyper)
 *   EMA:  hyper[0] = w, hyper[1] != 0 = copy mode (gs_ema_hyper)
 * (fp32, device memory for HIP plans, host memory for host plans) when the
 * kernel runs, so a step recorded into a hipGraph follows an LR schedule and
 * Adam's bias corrections on replay; the argument values are then ignored.
 * NULL restores argument hyper-parameters.  The buffer must outlive its use.
 * replaces: T:optim/adam.py capturable=True (device step / tensor lr) */
int gs_plan_set_hyper_source(gs_plan* p, const float* hyper);
/* Adam hyper source update on the stream (one thread; graph-capturable):
 *   if (!found_inf || *found_inf == 0) *step += 1;
 *   hyper = [-(lr/bc1), sqrt(bc2), 1 - lr*wd]  with bcK = 1 - betaK^step, in double
 * step, lr: fp64 scalars; hyper: fp32[3] (the plan's hyper source).
 * replaces: T:optim/adam.py:640-668 (capturable branch: device step, bias corrections) */
int gs_adam_hyper(int device_kind, double* step, const double* lr, double beta1, double beta2,
                  double weight_decay, const float* found_inf, float* hyper, void* stream);
/* LAMB (You et al. 2019, layer-wise adaptive moments; DeepSpeed's FusedLamb, ColossalAI's
 * Lamb / FusedLAMB): Adam whose update u is multiplied, per tensor, by the trust ratio
 * ‖w‖ / ‖u‖.  The ratio needs the norm of the Adam update, not of the gradient, so the
 * norm pass also advances the moments: gs_lamb_moments is one pass over (p, g, m, v) that
 * stores m', v' and publishes the per-tensor Σp², Σu² (24 B/param with fp32 grads: reads
 * 16, writes 8), gs_lamb_step one pass over (p, m', v') that recomputes u and writes p
 * (16 B/param).  u is recomputed, not stored: the same 40 B/param either way, and no
 * 4 B/param scratch.  Both use the per-tensor flags of gs_plan_set_adapt and the
 * segmented reduction of gs_lars_norms (same slot map, same summation order).
 *
 * Slots: 0 = p (f32), 1 = g (grad_dtype: f32, bf16 or f16), 2 = exp_avg (f32),
 * 3 = exp_avg_sq (f32).  Arithmetic (all fp32; every multiply, add, divide and sqrt
 * rounded once, NO fma).  Formed on the host in double, then rounded to fp32: b1, b2,
 * w1 = 1-beta1, w2 = 1-beta2, bc1 = 1-beta1^step, bc2s = sqrt(1-beta2^step) (both 1 when
 * bias correction is off: the caller passes them), lr, eps, wd, lo, hi (the trust-ratio
 * clamp; 0 and +inf mean none).
 *   per tensor t:   wd_t = adapt[t] ? wd : 0
 *   pass 1 (gs_lamb_moments), per element (m = *grad_scale_dev if given):
 *       g  = float(g_i);  if (m) g = g*m
 *       m' = m_i*b1 + w1*g
 *       v' = v_i*b2 + (w2*g)*g
 *       u  = (m'/bc1) / (sqrt(v')/bc2s + eps);   if (wd_t != 0) u = u + wd_t*p_i
 *       store m', v';   sp += p_i*p_i;  su += u*u       (fixed order, as gs_lars_norms)
 *   pass 2 (gs_lamb_step), per tensor:
 *       wn = sqrt(sp); un = sqrt(su); ratio = 1
 *       if (adapt[t] && wn > 0 && un > 0) { ratio = wn/un; if (ratio < lo) ratio = lo; if (ratio > hi) ratio = hi; }
 *       slr = lr*ratio
 *   pass 2, per element:  u recomputed from (p_i, m', v') by the same expression;  p = p_i - slr*u
 * Both passes and the host backend compile one text of u (lamb_update, gs_common.h), so
 * the recomputed u is the one whose square was summed, bit for bit.  eps, wd, bc1 and
 * bc2s must be the same in both calls.
 *
 * found_inf_dev (nullable): *found_inf != 0 and neither pass writes p, m or v; the norms
 * vector is then unspecified.  A clip set on the plan (gs_plan_set_clip*) is GS_ESTATE:
 * a global pre-normalisation of the grads goes in as grad_scale_dev.  With a hyper
 * source on the plan (gs_plan_set_hyper_source) both kernels read hyper = [lr, bc1, bc2s]
 * from it when they run, as Adam reads its own; the argument values are then ignored.
 * Determinism: as gs_lars_norms; sharded tensors as there (the caller SUM-all-reduces
 * the vector between the two passes).  Not part of LAMB here: amsgrad, a plan clip.
 *
 * norms_out: fp32[2n] in the plan's memory kind: [2t] = Σp², [2t+1] = Σu² of tensor t.
 * Two launches (the chunk pass, the per-tensor fold), one timer record (GS_OP_LAMB_MOMENTS).
 * replaces: of a Python LAMB, the foreach moments (exp_avg.lerp_ / mul_().add_(),
 *           exp_avg_sq.mul_().addcmul_(), the addcdiv that forms the update, add(p, alpha=wd))
 *           and the per-parameter torch.norm(p), torch.norm(update) pair */
int gs_lamb_moments(gs_plan* p, int grad_dtype, double beta1, double beta2, double eps, double weight_decay,
                    double bc1, double bc2_sqrt, float* norms_out, const float* grad_scale_dev,
                    const float* found_inf_dev, void* stream);
/* pass 2 above on slots 0, 2, 3; norms: gs_lamb_moments' output for this step.
 * replaces: of a Python LAMB, the per-parameter trust ratio (where / clamp) and
 *           p.add_(update, alpha=-lr*ratio) */
int gs_lamb_step(gs_plan* p, double lr, double eps, double weight_decay, double bc1, double bc2_sqrt,
                 double min_ratio, double max_ratio, const float* norms, const float* found_inf_dev, void* stream);
/* gs_lamb_step that also writes slot 4 = a low-precision copy of the new p (lowp_dtype
 * GS_BF16 / GS_F16; -1 = none, and then this IS gs_lamb_step: the same kernel).  The fp32
 * arithmetic is unchanged; p_lowp[i] = cast(p_new[i]), round to nearest even; the copy
 * pointer may be 2-byte aligned; *found_inf != 0 writes nothing, the copy included.
 * replaces: the `p_lowp.copy_(p_master)` behind a Python LAMB on fp32 master weights
 *           (ColossalAI DistributedLamb under its mixed-precision ZeRO optimizer) */
int gs_lamb_step_lowp(gs_plan* p, int lowp_dtype, double lr, double eps, double weight_decay,
                      double bc1, double bc2_sqrt, double min_ratio, double max_ratio,
                      const float* norms, const float* found_inf_dev, void* stream);
/* LAMB hyper source update on the stream (one thread; graph-capturable), gs_adam_hyper's
 * counterpart:
 *   if (!found_inf || *found_inf == 0) *step += 1;
 *   hyper = [lr, 1 - beta1^step, sqrt(1 - beta2^step)]  in double, rounded to fp32
 *           (bias_correction == 0: [lr, 1, 1])
 * step, lr: fp64 scalars; hyper: fp32[3] (the plan's hyper source).
 * replaces: the host-side `state["step"] += 1` and bias corrections of a Python LAMB */
int gs_lamb_hyper(int device_kind, double* step, const double* lr, double beta1, double beta2, int bias_correction,
                  const float* found_inf, float* hyper, void* stream);

/* EMA / SWA weight averaging: one pass a' = lerp(a, s, w) over a whole model.
 * Slots: 0 = the average a (f32), 1 = the source s (src_dtype: f32, bf16 or f16, converted
 * to fp32 on load), 2 = a low-precision copy of the new a (lowp_dtype GS_BF16 / GS_F16;
 * -1 = none, and then slot 2 is not touched).  12 B/param with an fp32 source (reads 8,
 * writes 4), 10 with a 16-bit one, + 2 with the copy.
 * Arithmetic (all fp32; w = the weight rounded to fp32), the same on both backends:
 *   copy mode:    a' = s                         (bits moved; no arithmetic touches the value)
 *   |w| <  0.5:   a' = fmaf(w, s - a, a)
 *   |w| >= 0.5:   a' = fmaf(w - 1.0f, s - a, s)  (w - 1.0f one fp32 subtraction)
 *   lowp copy:    cast(a'), round to nearest even of the STORED fp32 a'
 * which is torch.lerp's CPU kernel bit for bit on either side of the 0.5 switch.  In copy
 * mode with an fp32 source any 32-bit word is moved unchanged, so an int64 tensor can ride
 * along as 2*numel fp32 words (NaN-patterned halves are not quieted); a 16-bit source is
 * converted (bf16 exactly).
 * With a hyper source on the plan (gs_plan_set_hyper_source) the kernel reads
 * hyper[0] = w and hyper[1] != 0 = copy mode when it runs (gs_ema_hyper writes both), and
 * the weight / copy arguments are ignored (the weight is still range-checked).
 * GS_EINVAL before any launch: a dtype outside the lists above, a weight outside [0, 1] or
 * NaN, an unbound slot of a non-empty tensor.  A clip set on the plan is GS_ESTATE.
 * replaces: T:optim/swa_utils.py AveragedModel.update_parameters (the per-parameter copy_
 *           of the first update, torch._foreach_lerp_ of the later ones, the per-buffer
 *           copy_ that keeps buffers in sync), get_ema_multi_avg_fn, get_swa_multi_avg_fn */
int gs_ema_step(gs_plan* p, int src_dtype, int lowp_dtype /* -1 none */, double weight, int copy,
                void* stream);
/* The averaging weight from the device-side update counter (one thread; graph-capturable),
 * gs_adam_hyper's counterpart:
 *   n = *n_averaged;  hyper[1] = (n == 0)                       (the first update copies)
 *   GS_EMA_EMA:     hyper[0] = (float)(1 - decay)               (the difference in double)
 *   GS_EMA_SWA:     hyper[0] = 1.0f / (float)(n + 1)            (one fp32 division)
 *   GS_EMA_WARMUP:  hyper[0] = (float)(1 - min(decay, (1 + n) / (10 + n)))   (in double)
 *   *n_averaged = n + 1
 * n_averaged: int64 scalar, hyper: fp32[>= 2], both where device_kind says.  GS_EMA_SWA
 * does not use decay (pass 0).  GS_EINVAL: NULL pointers, an unknown mode, decay outside [0, 1].
 * replaces: T:optim/swa_utils.py AveragedModel.update_parameters (`bool(n_averaged == 0)`,
 *           `n_averaged > 0`, `n_averaged += 1`), get_ema_multi_avg_fn (1 - decay),
 *           get_swa_multi_avg_fn (1 / (num_averaged + 1)) */
#define GS_EMA_EMA 0
#define GS_EMA_SWA 1
#define GS_EMA_WARMUP 2
int gs_ema_hyper(int device_kind, int64_t* n_averaged, int mode, double decay, float* hyper /*[2]*/,
                 void* stream);

/* ======================================================================
 * bucket assignment (greedy by size per dtype, first-bucket cap)
 * replaces: T:.../c10d/reducer.hpp:590-595 compute_bucket_assignment_by_size
 *           (dist._compute_bucket_assignment_by_size)
 * order: NULL -> tensors in index order and buckets sorted by min index;
 *        else the gradient-ready order (no sort), as Reducer::rebuild_buckets.
 * Writes bucket_of[n] (bucket id per tensor position in `order`/index order) and
 * returns the bucket count (>=0) or an error.
 * ==================================================================== */
int gs_compute_bucket_assignment(int n, const int64_t* nbytes, const int32_t* dtype_keys,
                                 const int32_t* order, int n_limits, const int64_t* limits,
                                 int32_t* bucket_of /* [n], indexed by tensor id */,
                                 int32_t* bucket_members /* [n] concatenated, bucket order */,
                                 int32_t* bucket_counts /* [n] */);

/* ======================================================================
 * bucketer: the Reducer state machine
 * replaces: T:.../c10d/reducer.hpp:52-63 Reducer ctor, :73 autograd_hook,
 *           :275 mark_variable_ready_dense, :111-116 run_comm_hook,
 *           :283 finalize_bucket_dense, :346-402 Bucket
 * ==================================================================== */
#define GS_BKT_AUTO_COLLECTIVE 1 /* library launches the collective itself (needs comm) */
#define GS_BKT_GRAD_VIEW 2       /* grads already alias the bucket: scale in place, no unpack */
#define GS_BKT_NO_SCALE 4        /* a comm hook owns the averaging: copy without 1/ws */
#define GS_BKT_REDUCE_SCATTER 8  /* ZeRO-2: reduce-scatter into shard buffers instead of allreduce */
#define GS_BKT_NO_UNPACK 16      /* caller consumes the bucket directly (ZeRO / fused step) */

int gs_bucketer_create(gs_comm* comm, int device_kind, int device, int n_params,
                       const int64_t* numels, int grad_dtype, int n_buckets,
                       const int32_t* bucket_counts, const int32_t* bucket_members,
                       int bucket_dtype, int64_t align_elems, float div_factor, int flags,
                       gs_bucketer** out);
int gs_bucketer_destroy(gs_bucketer* b);
int gs_bucketer_bucket_numel(gs_bucketer* b, int bucket, int64_t* out);
/* padded numel of the reduce-scatter output shard for a bucket (ZeRO-2) */
int gs_bucketer_shard_numel(gs_bucketer* b, int bucket, int64_t* out);
int gs_bucketer_param_location(gs_bucketer* b, int param, int32_t* bucket, int64_t* offset);
/* per-bucket dtypes (torch's Reducer buckets per dtype: a model with params of
 * several floating dtypes gets buckets of each; create() sets the defaults) */
int gs_bucketer_set_bucket_dtype(gs_bucketer* b, int bucket, int grad_dtype, int bucket_dtype);
/* storage for bucket `bucket` (torch-owned, bucket_numel elements of its bucket dtype) */
int gs_bucketer_set_bucket_buffer(gs_bucketer* b, int bucket, void* ptr);
/* ZeRO-2 output shard storage for bucket */
int gs_bucketer_set_shard_buffer(gs_bucketer* b, int bucket, void* ptr);
/* start of a backward pass that will synchronise (Reducer::prepare_for_backward).
 * sqnorm_dev (nullable): receives Σ g² of the averaged grads, fused into unpack. */
int gs_bucketer_prepare(gs_bucketer* b, float* sqnorm_dev);
/* autograd hook: param's grad (grad_ptr) is final for this backward.
 * ready_out[*n_ready] receives the buckets that became launchable, in launch
 * order; with GS_BKT_AUTO_COLLECTIVE their collectives are already enqueued. */
int gs_bucketer_mark_ready(gs_bucketer* b, int param, const void* grad, void* stream,
                           int32_t* ready_out, int32_t* n_ready);
/* mark every not-yet-ready param as unused (zero its slot) — find_unused_parameters */
int gs_bucketer_mark_unused(gs_bucketer* b, void* stream, int32_t* ready_out, int32_t* n_ready);
/* end of backward: unpack (unless view / no-unpack) and order `stream` after
 * the collectives (Reducer::finalize_backward). */
int gs_bucketer_finalize(gs_bucketer* b, void* stream);
/* unpack one bucket (external-collective mode: after the caller's collective) */
/* AMP: fuse the non-finite check of the averaged grads into each bucket's
 * unpack (found_inf[0] = max(found_inf[0], non-finite ? 1 : 0); the caller
 * zeroes it before backward); NULL disables.  Replaces the check pass of
 * GradScaler._unscale_grads_ (T:amp/grad_scaler.py:280) for these grads. */
int gs_bucketer_set_found_inf(gs_bucketer* b, float* found_inf);
/* The divisor of the next backward's packs (grad x float(1/div_factor)),
 * between backwards: DDP.join(divide_by_initial_world_size=False) divides by
 * the ranks still training, as the Reducer's div_factor_ set from the forward
 * pass work handle (T:include/torch/csrc/distributed/c10d/reducer.hpp:499,
 * _set_forward_pass_work_handle). */
int gs_bucketer_set_div_factor(gs_bucketer* b, float div_factor);
int gs_bucketer_unpack_bucket(gs_bucketer* b, int bucket, void* stream);
/* Sharded buckets (NO_UNPACK / REDUCE_SCATTER, the ZeRO engine): the
 * bucket collectives' watchdog marks ride on `consumer`'s next launch (the
 * sharded update, stream-ordered after finalize) instead of a packet after
 * each collective; NULL restores the packets.  GS_EINVAL on unpacking buckets
 * (their unpack kernels already carry the marks).
 * replaces: ProcessGroupNCCL's per-work end event, as gs_allreduce_marked */
int gs_bucketer_set_mark_consumer(gs_bucketer* b, gs_plan* consumer);
/* the plan of bucket 0's pack — the first libgsync kernel of the next
 * synchronising backward, a consumer for collectives issued after a step
 * (ZeRO's parameter all-gather) */
int gs_bucketer_first_pack_plan(gs_bucketer* b, gs_plan** out);
/* timing of the library's own collective launches (ms of the last iteration, via events) */
int gs_bucketer_last_comm_ms(gs_bucketer* b, int bucket, float* ms);
/* per-bucket timeline of the last iteration (HIP events; -1 where untimed:
 * host buckets, external collectives, hipGraph capture), ms:
 *   out[0] queue      bucket ready on the producer -> its pack kernel starts
 *   out[1] pack       out[2] collective (pack end -> unpack start)
 *   out[3] unpack (+ fused checks)
 *   out[4] ready -> every bucket finished: for the last bucket this is the
 *          exposed end-of-backward tail */
int gs_bucketer_last_timing(gs_bucketer* b, int bucket, float* out /* [5] */);
/* which timing marks the bucketer takes: 0 none; 1 (default) the last bucket's
 * ready event + the "every chain done" mark — out[4] of the last bucket, the
 * tail; 2 every bucket's full timeline (and gs_bucketer_last_comm_ms).  The
 * ready mark is an event packet (~4.7 µs of stream time on the exposed chain);
 * every other mark rides on the chain's own kernels (hipExtLaunchKernel start /
 * stop events, ~2.4 µs) and becomes a packet only where no kernel runs */
int gs_bucketer_set_timeline(gs_bucketer* b, int level);
/* the HIP stream bucket `bucket`'s chain (pack -> collective -> unpack) was
 * enqueued on in this backward (the comm stream, or the producer stream for the
 * last bucket); NULL before its launch, on the host and with external
 * collectives.  Work enqueued there after the chain sees the averaged grads —
 * the overlapped optimizer (DDP._register_fused_optim) steps each bucket so.
 * replaces: the Future of run_comm_hook that _hook_then_optimizer chains on
 *           (T:distributed/algorithms/ddp_comm_hooks/optimizer_overlap_hooks.py) */
int gs_bucketer_bucket_stream(gs_bucketer* b, int bucket, void** stream);
/* Debug mode (checksum each bucket before and after the
 * collective): with a non-NULL device (host, for host buckets) buffer of
 * 3 * n_buckets floats, every backward writes sums[3b] = Σx of bucket b after
 * its pack (before the collective), sums[3b+1] = Σx after the collective
 * (before the unpack) and sums[3b+2] = Σx² after the pack.  Across ranks
 * Σ_r sums_r[3b] must equal sums[3b+1] up to fp32 rounding and sums[3b+1]
 * must be identical on every rank
 * (distributed_training_amd.ddp.DistributedDataParallel.verify_bucket_checksums).
 * NULL disables. */
int gs_bucketer_set_debug(gs_bucketer* b, float* sums);

/* ====================================================================
 * Input step of the CIFAR configuration
 * replaces: torch.utils.data.DistributedSampler.__iter__
 *           (T:utils/data/distributed.py:107-138) and the per-sample
 *           torchvision 0.15.2 transforms Pad(4) / RandomHorizontalFlip /
 *           RandomCrop(32) / ToTensor + default_collate, driven by
 *           DataLoader(num_workers=0) (R:resnet/pytorch_ddp/ddp_train.py:25-48)
 * ==================================================================== */
#define GS_LAYOUT_NCHW 0
#define GS_LAYOUT_NHWC 1
/* size of torch.get_rng_state() for a CPU generator (MT19937 + caches) */
int gs_rng_state_bytes(void);
/* n raw 32-bit MT19937 outputs from torch's serialized CPU generator state,
 * advancing the state in place exactly as n torch draws would */
int gs_rng_draw_u32(uint8_t* state, int64_t state_bytes, int64_t n, uint32_t* out);
/* torch.randperm(n, generator=torch.Generator().manual_seed(seed)) */
int gs_randperm(uint64_t seed, int64_t n, int64_t* out);
/* DistributedSampler(n, num_replicas, rank, shuffle, seed, drop_last) with
 * set_epoch(epoch): this rank's indices (out = NULL: *count only) */
int gs_distributed_sampler_indices(int64_t n, int num_replicas, int rank, int shuffle, uint64_t seed,
                                   int64_t epoch, int drop_last, int64_t* out, int64_t cap,
                                   int64_t* count);
/* per-sample (index, flip, top, left) for a batch, consuming torch's global
 * generator state in the reference's order: flip draw (if flip), then the
 * crop's two draws (unless the padded image equals the crop) per sample */
int gs_crop_flip_params(const int64_t* indices, int64_t B, int in_h, int in_w, int pad, int out_h,
                        int out_w, int flip, uint8_t* rng_state, int64_t state_bytes,
                        int32_t* params /* [B,4] */);
/* one batch: gather + pad + flip + crop + uint8->float /255 (+ bf16 cast),
 * labels gathered alongside; device_kind HIP runs one gfx950 kernel on
 * `stream` (src, labels, params, out in device memory) */
int gs_image_augment(int device_kind, int device, const uint8_t* src, const int64_t* labels, int64_t n_src,
                     int H, int W, int C, int pad, int out_h, int out_w, const int32_t* params, int64_t B,
                     void* out, int out_dtype, int out_layout, int64_t* out_labels, void* stream);
/* gs_image_augment with MixUp / CutMix (Zhang et al. 2018; Yun et al. 2019) in the same launch.
 * mix: [B, 4] int32 beside params, one record per batch position i:
 *   (partner, lam as fp32 bits, y0 | y1 << 16, x0 | x1 << 16)
 * partner is a batch position; its image is that position's augmented image, made with its own
 * params record.  With a = the sample's pixel, b = the partner's pixel at the same (c, y, x) and
 * lam1 = 1.f - lam, an output element is
 *   a non-empty box (y0 < y1 and x0 < x1):  b inside [y0, y1) x [x0, x1), a outside
 *   an empty box, lam != 1:                 a * lam + b * lam1, each multiply and the add rounded
 *                                           once in fp32, no fma
 *   an empty box and lam == 1, or partner == i:  a; the partner's image is not read
 * and the bf16 cast (round to nearest even) follows the blend.  out_labels[i] is the sample's
 * label, out_labels_b[i] the partner's, out_lam[i] = lam (each nullable).
 * GS_DEV_HOST rejects with GS_EINVAL, before writing anything, what gs_image_augment rejects and
 * a partner outside [0, B), lam outside [0, 1] or NaN, a box with y0 > y1, y1 > out_h, x0 > x1
 * or x1 > out_w; out_h and out_w are at most 65535.  GS_DEV_HIP cannot read the records on the
 * host: a partner outside [0, B) or such a lam makes the sample its own partner (out_lam = 1,
 * out_labels_b = out_labels), a box is clamped to the output, and nothing outside the image
 * set or the batch is read; mix is 16-byte aligned.  One launch on `stream`: one workgroup per
 * sample that stages the sample's image in LDS, and the partner's behind it when the record
 * needs it, if two images fit 48 KiB and gs_image_augment's alignment conditions hold; the
 * global-gather kernel with the same arithmetic otherwise. */
int gs_image_augment_mix(int device_kind, int device, const uint8_t* src, const int64_t* labels, int64_t n_src,
                         int H, int W, int C, int pad, int out_h, int out_w, const int32_t* params,
                         const int32_t* mix, int64_t B, void* out, int out_dtype, int out_layout,
                         int64_t* out_labels, int64_t* out_labels_b, float* out_lam, void* stream);
/* The resize-based input step in one launch: gather + bilinear resized crop of a per-sample box +
 * hflip + ToTensor (+ Normalize) (+ bf16 cast), labels gathered alongside.
 * replaces: torchvision RandomResizedCrop / Resize + CenterCrop / RandomHorizontalFlip / ToTensor /
 *           Normalize on tensors, i.e. F.interpolate(x / 255, mode="bilinear", align_corners=False,
 *           antialias=False) of each sample's box, flipped and normalised.
 * rec: [B, 4] int32, one record per batch position: (index, flip, top | left << 16, h | w << 16),
 * the box [top, top + h) x [left, left + w) of image `index`; H, W, out_h, out_w <= 65535.
 * (virt_h, virt_w) and (off_y, off_x) are the launch's virtual output frame: output (y, x) is
 * coordinate d_y = y + off_y, d_x = x' + off_x of a virt_h x virt_w resize of the box, where
 * x' = out_w - 1 - x with flip set, else x.  Training: virt = out, off = 0.  Resize(S) +
 * CenterCrop(c): the whole image as the box, virt = the resized extent, off = the crop's offset.
 * Along an axis with box extent n and virtual extent V, every operation rounded once in fp32, no fma:
 *   scale = float(n) / float(V)
 *   s  = max((float(d) + 0.5f) * scale - 0.5f, 0.f)
 *   i0 = min(int(s), n - 1);  i1 = min(i0 + 1, n - 1);  l1 = s - float(i0);  l0 = 1.f - l1
 * With the taps p = float(u8) / 255.f at (y.i0, x.i0), (y.i0, x.i1), (y.i1, x.i0), (y.i1, x.i1) = a, b, c, d:
 *   t = a * x.l0 + b * x.l1;  u = c * x.l0 + d * x.l1;  o = t * y.l0 + u * y.l1
 * then, if mean and std are given (host arrays of C floats, C <= 4; both or neither),
 * (o - mean[c]) / std[c], then the bf16 cast (round to nearest even).
 * GS_DEV_HOST rejects with GS_EINVAL, before writing anything: an index outside the set, an empty
 * box, a box outside the image, std[c] == 0, and a frame with off < 0 or off + out > virt.
 * GS_DEV_HIP checks the launch-uniform arguments the same way but cannot read the records on the
 * host: an index outside the set writes zeros and label 0, a box is clamped into the image
 * (top <= H - 1, left <= W - 1, 1 <= h <= H - top, 1 <= w <= W - left), and nothing outside the
 * image set is read; rec is 16-byte aligned.  One launch on `stream`, no temporaries: one workgroup
 * per (sample, band of output rows) stages the band's source rows in LDS; a global-gather kernel
 * with the same arithmetic when a one-row band does not fit 48 KiB, C * out_h * out_w is not a
 * multiple of 4 (NCHW: out_h * out_w), out is not 16-byte aligned, or H > 2 * virt_h or
 * W > 2 * virt_w (the taps skip most of the rows a band would stage). */
int gs_image_resample(int device_kind, int device, const uint8_t* src, const int64_t* labels, int64_t n_src,
                      int H, int W, int C, int out_h, int out_w, int virt_h, int virt_w, int off_y, int off_x,
                      const int32_t* rec, int64_t B, const float* mean, const float* std, void* out,
                      int out_dtype, int out_layout, int64_t* out_labels, void* stream);

/* ======================================================================
 * NHWC BatchNorm backward fused with the ReLU mask and the residual add
 * (csrc/gs_bn_kernels.hip; autograd glue: distributed_training_amd/fused_bn.py)
 * replaces: miopen_batch_norm_backward + threshold_backward (+ the in-place
 *           add and ReLU of the block's tail in the forward)
 *
 * An activation is a row-major [R, C] bf16 matrix (R = N*H*W, NHWC), C % 8 == 0,
 * every pointer 16-byte aligned; mean / invstd / weight / grad_* are fp32 [C].
 * HIP only: each entry launches on `stream` of the current device, allocates
 * nothing and never synchronises, so it can be recorded into a hipGraph.
 * Results are deterministic: fixed reduction order, no float atomics.
 * ==================================================================== */
/* P, the number of per-workgroup partial sums of (R, C): the workspace both
 * backward entries take holds P * C * 2 floats ([P, C, 2]) */
int gs_bn_bwd_partials(int64_t R, int C);
/* partial sums of g and g * (x - mean) per channel into ws, with
 * g = dy * [y > 0] (y != NULL) or dy (xhat = (x - mean) * invstd: the dx
 * pass scales the folded sum by invstd once).
 * g_out != NULL: g is also written as bf16 (bit-identical to
 * threshold_backward(dy, y, 0)), the gradient of a residual branch. */
int gs_bn_bwd_reduce(const void* x, const void* dy, const void* y, void* g_out, const float* mean, float* ws,
                     int64_t ws_floats, int64_t R, int C, void* stream);
/* the same for an activation whose gradient arrives as the two halves of a fork:
 * dy = bf16(float(dy_a) + float(dy_b)), rounded to nearest even (bit-identical to
 * ATen's bf16 add), then the mask (y != NULL), g_out and the sums as above.
 * g_out is required (with or without y) and overlaps no input: it is the
 * gradient the dx pass reads, with y = NULL.  dy_b = NULL: gs_bn_bwd_reduce. */
int gs_bn_bwd_reduce_fork(const void* x, const void* dy_a, const void* dy_b, const void* y, void* g_out,
                          const float* mean, float* ws, int64_t ws_floats, int64_t R, int C, void* stream);
/* folds the partials in index order and writes
 * dx = weight * invstd * (g - sum(g)/R - xhat * sum(g*xhat)/R) as bf16
 * (truncated, as the MIOpen kernels it replaces convert it),
 * grad_weight = sum(g*xhat), grad_bias = sum(g); g = dy * [y > 0] (y != NULL) or dy */
int gs_bn_bwd_dx(const void* x, const void* dy, const void* y, const float* mean, const float* invstd,
                 const float* weight, const float* ws, int64_t ws_floats, void* dx, float* grad_weight,
                 float* grad_bias, int64_t R, int C, void* stream);
/* t = relu(t + identity) in place over n bf16 elements (n % 8 == 0): the sum
 * formed in fp32 and rounded once to bf16, then max with 0; bit-identical to
 * ATen's add_ followed by relu_ */
int gs_add_relu_fwd(void* t, const void* identity, int64_t n, void* stream);
/* the stem's tail: pooled = MaxPool2d(3, stride 2, padding 1)(relu(y)) over an NHWC bf16 activation
 * [N, H, W, C] -> [N, OH, OW, C], OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1, and idx [N, OH, OW, C]
 * uint8: the winner's position 3 * kh + kw (0..8) in its unclipped 3 x 3 window.  y is left as it is.
 * The winner is chosen as ATen's relu_ + max_pool2d choose it (rows outer, columns inner, a later
 * value wins only if it is greater or NaN), so pooled is bit-identical to theirs. */
int gs_relu_maxpool_fwd(const void* y, void* pooled, void* idx, int64_t N, int H, int W, int C, void* stream);
/* the pool's backward from idx: dx [N, H, W, C] bf16, every element written (no zero fill, no
 * atomics): the sum of the gradients of the windows that name the element, windows in ascending
 * (oh, ow) order, added in fp32 and rounded once to bf16; bit-identical to ATen's
 * max_pool2d_with_indices_backward.  d_b != NULL: a window's gradient is bf16(d_a + d_b), the two
 * halves of a fork of the pooled output (ATen's bf16 add). */
int gs_maxpool_bwd(const void* d_a, const void* d_b, const void* idx, void* dx, int64_t N, int H, int W, int C,
                   void* stream);
/* The ReLU mask as bits.  For an activation v of n bf16 elements the mask is n / 8 bytes: byte i
 * belongs to the 16-byte vector i (elements 8 i .. 8 i + 7), bit j is set iff !(v[8 i + j] <= 0)
 * (a NaN sets it, +-0 and negatives clear it): the predicate of g = dy * [y > 0] above.  The mask
 * pointer is required, needs no alignment and overlaps no other buffer of the call.
 *
 * Forward producers: the arithmetic of their siblings, plus the byte per vector.
 *   gs_relu_mask_fwd: t = relu(t) in place, bit-identical to ATen's relu_ (a NaN stays, -0 -> +0);
 *     the mask of the result.
 *   gs_add_relu_mask_fwd: gs_add_relu_fwd; the mask of the result.
 *   gs_relu_maxpool_mask_fwd: gs_relu_maxpool_fwd; the mask of the un-ReLU'd input y
 *     (N * H * W * C / 8 bytes), every byte written exactly once. */
int gs_relu_mask_fwd(void* t, void* mask, int64_t n, void* stream);
int gs_add_relu_mask_fwd(void* t, const void* identity, void* mask, int64_t n, void* stream);
int gs_relu_maxpool_mask_fwd(const void* y, void* pooled, void* idx, void* mask, int64_t N, int H, int W, int C,
                             void* stream);
/* Backward consumers: gs_bn_bwd_reduce, gs_bn_bwd_reduce_fork and gs_bn_bwd_dx with the mask
 * (R * C / 8 bytes) in place of y.  For a mask formed from y every output (the workspace, g_out,
 * dx, grad_weight, grad_bias) is bit for bit what the y-taking entry writes. */
int gs_bn_bwd_reduce_bits(const void* x, const void* dy, const void* mask, void* g_out, const float* mean, float* ws,
                          int64_t ws_floats, int64_t R, int C, void* stream);
int gs_bn_bwd_reduce_fork_bits(const void* x, const void* dy_a, const void* dy_b, const void* mask, void* g_out,
                               const float* mean, float* ws, int64_t ws_floats, int64_t R, int C, void* stream);
int gs_bn_bwd_dx_bits(const void* x, const void* dy, const void* mask, const float* mean, const float* invstd,
                      const float* weight, const float* ws, int64_t ws_floats, void* dx, float* grad_weight,
                      float* grad_bias, int64_t R, int C, void* stream);

/* ======================================================================
 * Evaluation: inference BatchNorm fused with its tail, and exact metrics
 * (csrc/gs_bn_kernels.hip, csrc/gs_eval_kernels.hip; Python: fused_bn.fused_eval,
 * distributed_training_amd/evaluation.py)
 * replaces: of an eval-mode forward, miopen_batch_norm (inference) + add_ + relu_
 *           per residual block and relu_ + max_pool2d_with_indices in the stem;
 *           of a validation loop, F.cross_entropy + topk + eq + sum + .item()
 *           per batch (the reference builds its test_dataloader and never drains it:
 *           R:resnet/pytorch_ddp/ddp_train.py:47, R:resnet/colossalai/colossal_train.py:77)
 * ==================================================================== */
/* y = relu(bn(x) + residual) for a BatchNorm in evaluation, where it is a per-channel
 * affine map of its running statistics: one pass, x (and the residual) in, y out.
 * x, residual (nullable), y: NHWC bf16 [R, C], C % 8 == 0; running_mean, running_var,
 * weight, bias: fp32 [C]; every pointer 16-byte aligned.  y may be x (in place);
 * otherwise y overlaps neither x nor the residual.  relu != 0 applies the ReLU.
 * Arithmetic, all fp32, in this order (a restatement is exact op for op):
 *   s_c = weight_c * (1.0f / sqrtf(var_c + (float)eps))     sqrt and / correctly rounded
 *   t_c = fmaf(-mean_c, s_c, bias_c)
 *   v   = fmaf(x, s_c, t_c);  residual: v = v + r;  relu: v = v > 0 ? v : (v is NaN ? v : +0)
 *   y   = bf16(v), round to nearest even, once (a NaN becomes 0x7FC0); no intermediate bf16
 * The statistics are read when the kernel runs and nothing else is touched: no folded
 * weights to refresh after a training step.  HIP only, one launch on `stream`, no
 * allocation, no host synchronisation, capturable.  GS_EINVAL before the launch: a null
 * or misaligned pointer, R <= 0, C <= 0 or C % 8 != 0, eps < 0 or NaN, a forbidden overlap. */
int gs_bn_infer_act(const void* x, const void* residual, const float* running_mean, const float* running_var,
                    const float* weight, const float* bias, double eps, int relu, void* y, int64_t R, int C,
                    void* stream);
/* the stem in evaluation, one launch: pooled = MaxPool2d(3, stride 2, padding 1) over
 * bf16(relu(fmaf(x, s_c, t_c))), s and t as above; x NHWC bf16 [N, H, W, C], pooled
 * [N, OH, OW, C] (OH, OW as gs_relu_maxpool_fwd).  No un-pooled output and no indices are
 * written.  Window clipping, scan order and the NaN rule are gs_relu_maxpool_fwd's, and
 * rounding is monotonic, so pooled is bit for bit the pool of gs_bn_infer_act's output.
 * pooled does not overlap x. */
int gs_bn_infer_relu_maxpool(const void* x, const float* running_mean, const float* running_var, const float* weight,
                             const float* bias, double eps, void* pooled, int64_t N, int H, int W, int C,
                             void* stream);
/* Adds one batch to an evaluation's accumulator.  logits: [B, K] (logits_dtype GS_F32,
 * GS_BF16 or GS_F16), row r at logits + r * row_stride elements (row_stride >= K);
 * labels: int64 [B]; topk: n_topk <= 4 values k >= 1 in host memory; ws: scratch of
 * 8 * B bytes; acc: eight 8-byte words, zeroed by the caller before the first batch:
 *   [0] rows counted (int64)        [1] rows whose label is outside [0, K) and is not
 *   [2] sum of the losses (double)      ignore_index (int64): they count nowhere else
 *   [3] reserved                    [4 + i] rows correct at topk[i] (int64)
 * logits, labels, ws and acc live where device_kind says.  Rows >= n_valid (the padding
 * a DistributedSampler appends) and rows whose label is ignore_index are skipped.  For
 * every other row, with z the row converted to fp32 and y its label:
 *   m = max z;  S = sum_j expf(z_j - m) (fp32, a balanced tree: at most ceil(log2 K)
 *   roundings on a path);  loss = (m - z_y) + logf(S)
 *   rank = #{j : z_j > z_y} + #{j < y : z_j == z_y}   (ties go to the lower index)
 *   correct at k iff rank < k
 * A row that holds a NaN is correct for no k and adds a NaN to the loss sum.  The call's
 * losses are added in ascending row order in fp64 and the total is added to acc[2]; the
 * counts are exact integers.  Bitwise repeatable: no floating-point atomics.  GS_DEV_HIP:
 * two launches on `stream` (one wavefront per row, then one workgroup that folds the
 * rows), no allocation, no host synchronisation, capturable.  GS_DEV_HOST: the same
 * rules; the tree of S has the same depth but another order, so a loss may differ from
 * the device's by a few fp32 ulps while every count is the same.
 * GS_EINVAL before any launch: an unknown device kind or dtype, B < 0, K outside
 * [1, 2^30], row_stride < K, n_valid outside [0, B], n_topk outside [0, 4], a k < 1,
 * a null or misaligned pointer.  B == 0 is a no-op. */
int gs_eval_accumulate(int device_kind, const void* logits, int logits_dtype, const int64_t* labels, int64_t B,
                       int64_t K, int64_t row_stride, int64_t n_valid, const int32_t* topk, int n_topk,
                       int64_t ignore_index, void* ws, void* acc, void* stream);

/* ======================================================================
 * Training criterion: cross-entropy with label smoothing, forward and backward
 * (csrc/gs_loss_kernels.hip; Python: distributed_training_amd/loss.py)
 * replaces: of a training step under autocast, the cast of the logits to fp32 +
 *           log_softmax + nll_loss (+ a row sum and elementwise ops with label
 *           smoothing), their backwards and the cast back, and the per-step
 *           loss.item() a running loss needs
 * ==================================================================== */
/* The loss of one batch.  logits, labels, row_stride, ignore_index: as gs_eval_accumulate.
 * label_smoothing = eps in [0, 1].  rows: output, 16 bytes per row:
 *   {fp32 loss, fp32 m, fp32 logS, int32 code}
 * code follows gs_eval_accumulate's rules: the label's rank >= 0 (ties to the lower index),
 * INT32_MAX for a row that holds a NaN, -1 for a row whose label is ignore_index, -2 for a
 * label outside [0, K).  red: output, 16 bytes:
 *   {fp32 loss_sum, fp32 loss_mean, int32 counted, int32 bad}
 * A counted row (code >= 0), with z the row converted to fp32 and y its label:
 *   m = max z;  S = sum_j expf(z_j - m) (gs_eval_accumulate's balanced tree: at most
 *   ceil(log2 K) roundings on a path);  logS = logf(S);  nll = (m - z_y) + logS
 *   eps > 0:  T = sum_j z_j on the same tree;  smooth = (m + logS) - T / (float)K
 *             loss = (1 - eps) * nll + eps * smooth
 *   eps == 0: loss = nll; the smoothing term is not formed, so a -inf logit on a masked
 *             class leaves the loss finite
 * every multiply and add rounded once, no fma.  A row that holds a NaN has loss, m and logS
 * NaN.  A row that is not counted gets {0, 0, 0, code}.  A label outside [0, K) that is not
 * ignore_index is tallied in red.bad (and acc[1]) and makes loss_sum and loss_mean NaN:
 * that is the visible signal; there is no device assert and no host read.
 * The counted rows' losses are added in ascending row order in fp64 and rounded once:
 * loss_sum = (float)total, loss_mean = (float)(total / counted); counted == 0 gives
 * sum 0 and mean NaN.
 * acc (nullable) with topk / n_topk: an accumulator with gs_eval_accumulate's layout; it is
 * advanced by this batch's counted and bad rows, its top-k hits and the sum of the UNSMOOTHED
 * losses nll (ascending row order, fp64), as gs_eval_accumulate with n_valid = B would.
 * rows, red, acc live where device_kind says.  Bitwise repeatable: no floating-point atomics.
 * GS_DEV_HIP: two launches on `stream` (one wavefront per row, then one workgroup that
 * folds), no allocation, no host synchronisation, capturable.  GS_DEV_HOST: the same rules;
 * the trees have the same depth but another order and expf / logf are the host's, so a loss
 * may differ from the device's by a few fp32 ulps while every code and count is the same.
 * GS_EINVAL before any launch: an unknown device kind or dtype, B < 0, K outside [1, 2^30],
 * row_stride < K, eps outside [0, 1] or NaN, n_topk outside [0, 4], a k < 1, a null or
 * misaligned pointer (rows and red 16 bytes, acc 8 bytes).  B == 0 writes
 * red = {0, NaN, 0, 0} and touches nothing else. */
int gs_xent_fwd(int device_kind, const void* logits, int logits_dtype, const int64_t* labels, int64_t B, int64_t K,
                int64_t row_stride, int64_t ignore_index, float label_smoothing, void* rows, void* red,
                const int32_t* topk, int n_topk, void* acc, void* stream);
/* The gradient of that loss with respect to the logits.  logits, labels, label_smoothing:
 * what the forward saw; rows, red: what it wrote.  reduction: 0 none, 1 mean, 2 sum.
 * grad_out: fp32 where device_kind says, one element for mean and sum, [B] for none; it is
 * read by the kernel, never on the host.  dlogits: [B, K] in the logits' dtype, row r at
 * dlogits + r * d_row_stride elements; it does not overlap logits.  A counted row:
 *   c = g / (float)counted (mean), g (sum), g[r] (none)
 *   q_off = eps / (float)K;  q_on = (1 - eps) + q_off;  q_j = q_on if j == y else q_off
 *   p_j = expf((z_j - m) - logS);  dz_j = c * (p_j - q_j)
 * each step rounded once, no fma, then dz_j rounded once to the logits' dtype.  A row that is
 * not counted (code < 0) gets K zeros; a NaN row gets K NaNs.  Elements K ... row_stride - 1
 * of a row are never read as data and never written.
 * GS_DEV_HIP: one launch on `stream`; a wavefront takes 2048 consecutive elements of a row,
 * so a row of K <= 2048 is one wavefront's and a longer one several.  Loads and stores are
 * 16 bytes wide when logits, dlogits and both row strides in bytes are multiples of 16, and
 * one element wide otherwise.  Repeatable, capturable, no allocation.
 * GS_EINVAL before the launch: as gs_xent_fwd, an unknown reduction, d_row_stride < K,
 * dlogits overlapping logits.  B == 0 is a no-op. */
int gs_xent_bwd(int device_kind, const void* logits, int logits_dtype, const int64_t* labels, int64_t B, int64_t K,
                int64_t row_stride, int64_t ignore_index, float label_smoothing, int reduction, const void* rows,
                const void* red, const float* grad_out, void* dlogits, int64_t d_row_stride, void* stream);
/* gs_xent_fwd for pair targets (MixUp / CutMix): row r has labels a = labels_a[r], b = labels_b[r]
 * and a's weight lam = lam[r] (fp32 [B]), all three where device_kind says and read by the
 * kernels only, so a captured graph replays with new targets.  Everything not said here is
 * gs_xent_fwd's.  A row is
 *   skipped (code -1)  if a or b is ignore_index;
 *   bad (code -2)      else if a or b is outside [0, K), or lam is outside [0, 1] or NaN;
 *   a one-label row    else if lam == 1 or a == b: exactly gs_xent_fwd's row for label a, the
 *                      same expressions and so the same 16 bytes;
 *   a mixed row        otherwise, with loss(y) gs_xent_fwd's loss for label y and lam1 = 1 - lam:
 *                        loss = lam * loss(a) + lam1 * loss(b), each operation rounded once;
 *                        code = the rank of the dominant label, a if lam >= 0.5 else b.
 * acc's loss word is advanced by the same expression at eps = 0, its top-k hits by code.
 * GS_DEV_HIP: two launches, as gs_xent_fwd.  GS_EINVAL: as gs_xent_fwd, and a null or
 * misaligned labels_b (8 bytes) or lam (4 bytes). */
int gs_xent_mix_fwd(int device_kind, const void* logits, int logits_dtype, const int64_t* labels_a,
                    const int64_t* labels_b, const float* lam, int64_t B, int64_t K, int64_t row_stride,
                    int64_t ignore_index, float label_smoothing, void* rows, void* red, const int32_t* topk,
                    int n_topk, void* acc, void* stream);
/* The gradient of that loss: gs_xent_bwd with, for a mixed row,
 *   q_j = q_off, (1 - eps) * lam + q_off at j == a, (1 - eps) * lam1 + q_off at j == b
 * each operation rounded once; a one-label row's q is gs_xent_bwd's for label a, and so are
 * its gradient's bits.  labels_a, labels_b and lam are what the forward saw; the row scratch
 * stays 16 bytes.  One launch. */
int gs_xent_mix_bwd(int device_kind, const void* logits, int logits_dtype, const int64_t* labels_a,
                    const int64_t* labels_b, const float* lam, int64_t B, int64_t K, int64_t row_stride,
                    int64_t ignore_index, float label_smoothing, int reduction, const void* rows, const void* red,
                    const float* grad_out, void* dlogits, int64_t d_row_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSYNC_H */
