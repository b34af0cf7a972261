/* libvpdhip -- C ABI of the MI355X-native VPD student train / apply path.
 *
 * The reference (jhong93/vpd) has no FFI: its boundary for this path is a Python
 * object surface.  Each entry point below names the reference
 * code whose device work it replaces; vpd_amd/ (Python) mirrors the reference
 * classes on top of these calls and INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a raw DEVICE pointer owned by the caller (torch tensors'
 *     data_ptr()); the library never allocates or frees caller-visible memory;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every call only enqueues work on it (no host sync), so calls are hipGraph-capturable;
 *   - return value 0 = ok, negative = error; vpd_last_error() gives the message
 *     (thread-local).  Shape/channel violations are the wrapper's AssertionError
 *     (models/rgb.py:80-82), not error codes.
 *   - flat buffers: `params`/`grads`/`adam_m`/`adam_v` are fp32 arrays of
 *     vpd_plan_param_numel() elements holding every trainable tensor in the
 *     reference's state_dict order and native layout (conv OIHW, linear [out][in]):
 *     encoder tensors first, then the motion decoder's.  `bn_running` holds
 *     running_mean / running_var of every BatchNorm in module order.
 */
#ifndef VPD_HIP_H
#define VPD_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct vpd_plan vpd_plan_t;

const char* vpd_last_error(void);
int vpd_abi_version(void);
/* Element type of activations / packed weights / activation gradients this library was built with: "bf16" (libvpdhip.so: training and
 * inference) or "fp16" (libvpdhip_f16.so, the same sources with -DVPD_ELEM_F16).
 * fp16 is the reference's own GPU precision (torch.cuda.amp.autocast + GradScaler: train_vpd_model.py:79,105; models/util.py:55-57);
 * fp16 TRAINING uses a loss scale (vpd_plan_set_loss_scale). */
const char* vpd_elem_dtype(void);

/* Network + workspace description for one (arch, input, head) configuration.
 * Replaces the module construction of RGBF_EmbeddingModel.__init__ (models/rgb.py:46-66),
 * ResNet.__init__/_make_layer (models/module.py:35-110) and, when motion != 0,
 * FCNet(emb_dim,[128,128],2*emb_dim) (train_vpd_model.py:61-65).
 * arch: "resnet18" | "resnet34" (BasicBlock) | "resnet50" | "resnet101" | "wide_resnet50_2" | "wide_resnet101_2"
 * (Bottleneck) -- the ResNet entries of ENCODER_ARCH (models/module.py:17-32).  train != 0 reserves the
 * activations / gradients a train step needs. */
int vpd_plan_create(const char* arch, int c_in, int img_h, int img_w, int emb_dim, int motion,
                    int max_batch, int train, vpd_plan_t** out);
/* `train`: 0 = inference plan, 1 = train plan; OR-ed with VPD_TRAIN_EARLY_BUCKET0 for data-parallel runs: the weight gradients of
 * layer4 are launched at the end of layer4's backward instead of together with layer3's, so gradient bucket 0 (fc + layer4 +
 * motion head, 61 % of the bytes) is final -- and its event recorded -- with three quarters of backward still ahead. */
#define VPD_TRAIN_EARLY_BUCKET0 2
void vpd_plan_destroy(vpd_plan_t* plan);

/* Trainable-tensor table in reference state_dict order (SURVEY.md 8b "state_dict schema").
 * kind: 0 conv weight OIHW, 1 BN weight, 2 BN bias, 3 linear weight [out][in], 4 linear bias.
 * is_decoder: 1 for the motion head's tensors (state_dict keys layers.{0,2,5}.*). */
int vpd_plan_num_tensors(const vpd_plan_t* plan);
int vpd_plan_tensor_info(const vpd_plan_t* plan, int i, int* kind, int* is_decoder, long long* offset,
                         long long* numel, int* ndim, int dims[4]);
long long vpd_plan_param_numel(const vpd_plan_t* plan);        /* multiple of 4 (tail padding) */
/* BatchNorm running statistics: BN i has C channels, running_mean at rm_off, running_var at rv_off. */
int vpd_plan_num_bn(const vpd_plan_t* plan);
int vpd_plan_bn_info(const vpd_plan_t* plan, int i, int* channels, long long* rm_off, long long* rv_off);
long long vpd_plan_bn_numel(const vpd_plan_t* plan);

/* Gradient buckets for data-parallel all-reduce (no reference counterpart: the
 * reference is single-device).  Bucket 0 is complete first during backward. */
int vpd_plan_num_buckets(const vpd_plan_t* plan);
int vpd_plan_bucket_range(const vpd_plan_t* plan, int bucket, long long* offset, long long* numel);

size_t vpd_plan_workspace_bytes(const vpd_plan_t* plan);
/* Zero the workspace (activation borders rely on it) and upload descriptor tables. */
int vpd_plan_init_workspace(vpd_plan_t* plan, void* workspace, void* stream);

/* fp32 master weights -> packed bf16 tap-major weights (+ dgrad layout), and the
 * eval-mode BN fold (scale/shift from running stats).  Call after every change
 * of `params` / `bn_running` (optimizer step, load_state_dict).  Replaces the
 * implicit weight reads of every conv/BN module call. */
int vpd_pack_weights(vpd_plan_t* plan, const float* params, const float* bn_running, void* workspace, void* stream);

/* Eval-mode forward: RGBF_EmbeddingModel.forward under eval()/no_grad, i.e. the
 * device part of embed() (models/rgb.py:72-86) and of ModelTrainer.epoch with
 * optimizer=None (train_vpd_model.py:70-76).  x: f32 [N][c_in][H][W] (NCHW, the
 * DataLoader batch layout, vpd_dataset/single_frame.py:206); emb_out: f32 [N][emb_dim].
 * If target != NULL also runs the motion head (if any) and adds sum-MSE to the
 * loss outputs (train_vpd_model.py:85-87, :93). */
int vpd_forward_eval(vpd_plan_t* plan, const float* params, const float* x, int n, float* emb_out,
                     const float* target, float* loss_step, double* loss_accum, void* workspace, void* stream);

/* x == NULL in vpd_forward_eval / vpd_forward_train: the input batch was already written to the plan's stem staging
 * buffer by vpd_plan_stage_crops (below); the fp32 NCHW batch is then never materialised. */

/* Train-mode forward + loss: encoder(img) -> [fcn_time] -> F.mse_loss(reduction='sum')
 * (train_vpd_model.py:83-88) with train-mode BatchNorm (batch statistics, running-stat
 * update momentum 0.1).  target: f32 [N][emb_dim or 2*emb_dim].  loss_step[0] = this
 * batch's sum-MSE; loss_accum[0] += it (the epoch accumulator of :93 kept on device).
 * n == 0 is legal (a data-parallel rank whose shard of a ragged last batch is empty): loss_step[0] = 0, nothing else
 * is touched; the matching vpd_backward(n = 0) zeroes `grads` and records every bucket event, so the rank still joins
 * the gradient all-reduce with zeros. */
int vpd_forward_train(vpd_plan_t* plan, const float* params, float* bn_running, const float* x,
                      const float* target, int n, float* emb_out, float* loss_step, double* loss_accum,
                      void* workspace, void* stream);

/* loss.backward() of models/util.py:52 for the graph built by vpd_forward_train:
 * writes d loss / d param for every trainable tensor into `grads` (overwrites;
 * the reference zero_grad()s after every step, models/util.py:58).
 * bucket_events: optional array of vpd_plan_num_buckets() hipEvent_t handles, each
 * recorded on `stream` as soon as that bucket's range of `grads` is final. */
int vpd_backward(vpd_plan_t* plan, const float* params, float* grads, int n, void** bucket_events,
                 void* workspace, void* stream);

/* loss.backward() of models/util.py:52 for ANY loss of the embeddings: the backward pass of the graph built by the preceding
 * vpd_forward_train (which may have been called with target == NULL) from the caller's d(loss)/d(emb) instead of the fused sum-MSE's
 * -- what torch autograd hands to the encoder's output when the reference module is trained with a weighted, cosine or contrastive
 * loss, reduction='mean', a head on top of the embeddings or torch's GradScaler.  The plan must be a train plan without the motion
 * head.  d_emb: f32 [n][emb_dim], dense, on the device; it is copied into the plan's d(pred) slot and taken as it is (neither
 * vpd_plan_set_loss_scale nor vpd_plan_set_scale_state applies: a scaled loss arrives scaled).  `grads` is overwritten as by
 * vpd_backward; lazy gradients do not apply (a pending vpd_plan_set_lazy_grads is cleared); bucket_events as in vpd_backward.
 * dx_nchw: NULL, or f32 [n][c_in][H][W] receiving d(loss)/d(x) (the forward's rounding of x to the element type taken as the
 * identity) -- the stem convolution's data gradient, which training never needs; only after a forward that took an x (a batch
 * staged by vpd_plan_stage_crops has no fp32 input).  n == 0 as in vpd_backward; dx_nchw is then not written.
 * Fails on the host, before anything is launched, for a null plan / params / grads / d_emb / workspace, a plan with train == 0,
 * a plan with the motion head, n outside 0..max_batch, a workspace that is not the bound one, a dx_nchw that is not 8-byte aligned
 * and a dx_nchw after a forward that took no x. */
int vpd_backward_ext(vpd_plan_t* plan, const float* params, float* grads, const float* d_emb, int n, float* dx_nchw,
                     void** bucket_events, void* workspace, void* stream);

/* optimizer.step() of models/util.py:53 for torch.optim.AdamW(lr) with torch defaults
 * (train_vpd_model.py:104): decoupled weight decay on every tensor. `step` is 1-based. */
int vpd_adamw_step(float* params, const float* grads, float* adam_m, float* adam_v, long long numel,
                   double lr, double beta1, double beta2, double eps, double weight_decay, int step, void* stream);

/* The same optimizer.step(), fused with the refresh of `plan`'s packed bf16 weights (what vpd_pack_weights would do on
 * the next forward): one pass over params / grads / adam_m / adam_v (16-byte aligned, numel >= the plan's
 * vpd_plan_param_numel; tensors beyond the plan's are updated too).  After it `plan` needs no vpd_pack_weights until
 * the parameters are written by someone else; other plans over the same parameters (the eval plan) still do. */
int vpd_plan_adamw_step(vpd_plan_t* plan, float* params, const float* grads, float* adam_m, float* adam_v,
                        long long numel, double lr, double beta1, double beta2, double eps, double weight_decay,
                        int step, void* workspace, void* stream);

/* Loss scale of this plan's following backward passes and optimizer steps (default 1 = none).  Replaces torch.cuda.amp.GradScaler
 * (train_vpd_model.py:105; scaler.scale(loss).backward() / scaler.step(optimizer): models/util.py:55-57) for fp16 training on
 * libvpdhip_f16.so: vpd_backward multiplies d(loss)/d(pred) by `scale` -- every gradient it produces is scale x its value --
 * and vpd_plan_adamw_step reads gradients x 1 / scale.  A caller that reads the flat gradient buffer itself divides by the scale. */
int vpd_plan_set_loss_scale(vpd_plan_t* plan, float scale);

/* ---- dynamic loss scaling, decided on the device ----
 * torch.cuda.amp.GradScaler() at its defaults is what the reference trains with (train_vpd_model.py:105; scaler.scale(loss)
 * .backward(); scaler.step(optimizer); scaler.update(): models/util.py:55-57): look for inf / NaN in the gradients, skip the
 * optimizer step when one is found and multiply the scale by the backoff factor, multiply it by the growth factor after
 * `growth_interval` clean steps in a row.  Here the whole decision lives in one block of DEVICE memory owned by the caller
 * (32 bytes, 16-byte aligned); every entry point below reads and writes it in stream order and none synchronises the host. */
typedef struct vpd_scale_state {
    float scale;                 /* the loss scale of the next backward pass / optimizer step */
    unsigned int found;          /* non-zero: an inf or NaN was seen in the gradients of the step in flight */
    int growth_tracker;          /* clean steps in a row since the scale last changed */
    int applied_steps;           /* optimizer steps actually applied (the `step` of AdamW's bias corrections, 0-based) */
    int skipped_steps;           /* optimizer steps skipped because of a non-finite gradient */
    int reserved[3];
} vpd_scale_state;

/* scaler.scale(loss) of models/util.py:55 with the scale on the device: while `state` is set, vpd_backward multiplies
 * d(loss)/d(pred) by state->scale as it stands when the pass runs, instead of by the host value of vpd_plan_set_loss_scale
 * (which keeps its meaning once `state` is NULL again).  NULL switches back. */
int vpd_plan_set_scale_state(vpd_plan_t* plan, const vpd_scale_state* state);

/* The inf / NaN search of scaler.step() (models/util.py:56; torch's _amp_foreach_non_finite_check_and_unscale_): ORs 1 into
 * state->found if any gradient the optimizer step of `plan` is about to read is not finite.  After a lazy backward
 * (vpd_plan_grads_pending() == 1) these are the conv weight gradients in the plan's scratch plus the ranges of `grads` that are
 * not conv weights (BatchNorm, fc, motion head, the stem conv); otherwise grads[0 .. numel).  Elements of `grads` beyond the
 * plan's vpd_plan_param_numel are checked in both cases.  Under data parallelism call it after the all-reduce. */
int vpd_plan_check_grads(vpd_plan_t* plan, const float* grads, long long numel, vpd_scale_state* state, void* workspace,
                         void* stream);
/* The same kernel over one plain range x[0 .. n) (any alignment, n >= 0). */
int vpd_op_check_finite(const float* x, long long n, vpd_scale_state* state, void* stream);

/* optimizer.step() as scaler.step(optimizer) runs it (models/util.py:56): vpd_adamw_step / vpd_plan_adamw_step with the gradients
 * read x 1 / state->scale, the 1-based step of the bias corrections taken as state->applied_steps + 1 -- and NOTHING written
 * (parameters, moments, packed weights) when state->found is set.  Neither touches `state`: vpd_scale_state_update does. */
int vpd_adamw_step_scaled(float* params, const float* grads, float* adam_m, float* adam_v, long long numel, double lr,
                          double beta1, double beta2, double eps, double weight_decay, const vpd_scale_state* state,
                          void* stream);
int vpd_plan_adamw_step_scaled(vpd_plan_t* plan, float* params, const float* grads, float* adam_m, float* adam_v,
                               long long numel, double lr, double beta1, double beta2, double eps, double weight_decay,
                               const vpd_scale_state* state, void* workspace, void* stream);

/* scaler.update() of models/util.py:57, torch's rule (_amp_update_scale_) without a clamp: found set -> scale *= backoff,
 * growth_tracker = 0, skipped_steps += 1; else applied_steps += 1, growth_tracker += 1 and, when it reaches growth_interval,
 * scale *= growth, growth_tracker = 0.  Then found = 0. */
int vpd_scale_state_update(vpd_scale_state* state, float growth, float backoff, int growth_interval, void* stream);

/* Exponential moving average of the weights (torch.optim.swa_utils.AveragedModel / timm's ModelEmaV2), one launch over up to four
 * ranges: dst[i][j] = fmaf(omd, src[i][j] - dst[i][j], dst[i][j]) in fp32 for j < n[i], omd = (float)(1 - d) with d computed in
 * double: d = decay, or min(decay, (1 + t) / (10 + t)) when warmup != 0 (timm's rule; t = updates applied before this one).
 * The ranges are DEVICE float ranges of any 4-byte alignment and any length >= 0 (the fast path wants src[i] and dst[i] to share
 * their 16-byte phase); src[i] and dst[i] must not overlap.  The arrays src / dst / n themselves are HOST arrays, copied into the
 * kernel's arguments: no upload, no synchronisation, capturable into a graph.
 * state == NULL: `t` is the caller's count, t0 is ignored.  state != NULL (the block of the dynamic loss scaler whose optimizer
 * step is in flight; call between the AdamW and vpd_scale_state_update): NOTHING is written when state->found is set, and
 * t = state->applied_steps - t0, the caller's `t` being ignored -- t0 is the applied-step count when averaging began.
 * Refused on the host, nothing launched: count outside 0..4 (0 returns 0 and looks at nothing else but decay, t, t0), decay outside
 * [0, 1] or NaN, negative t or t0, null src / dst / n or a null entry, negative n[i], src[i] == dst[i]. */
int vpd_ema_update(const float* const* src, float* const* dst, const long long* n, int count, double decay, int warmup, int t,
                   int t0, const vpd_scale_state* state, void* stream);

/* ---- gradient-norm clipping, decided on the device ----
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm) between backward() and optimizer.step(), for the fused step, where the conv
 * weight gradients never reach .grad: ONE pass over the gradients the optimizer step is about to read takes their sum of squares
 * (every element widened to double; fixed-order reductions, no atomics: the same input gives the same bits on every launch and on
 * every data-parallel rank), and a one-block kernel writes the caller's DEVICE block below (16-byte aligned, vpd_clip_state_bytes()
 * bytes -- the struct and the pass's partial sums behind it; zero it once):
 *   norm = sqrt(sum) / scale            scale: src->scale, or host_scale when src is NULL (1 without a loss scale)
 *   coef = min(1, max_norm / (norm + 1e-6))                                  (torch's formula, clamped as torch clamps)
 *   eff.scale = scale / coef            eff.found = (src ? src->found : 0) | (sum is inf or NaN)
 * all in double, each stored value rounded to float once.  The step is then vpd_plan_adamw_step_scaled / vpd_adamw_step_scaled
 * (and vpd_ema_update) called with &clip->eff: gradients x 1 / eff.scale = coef / scale.
 * With src (a dynamic loss scaler's step in flight) eff.applied_steps is copied from it and a non-finite sum is OR-ed into src->found
 * as the non-finite search would have done -- the search need not run: a sum of squares is non-finite exactly when an element is.
 * Without src the block counts its own steps: eff.applied_steps is left alone; advance it with
 * vpd_scale_state_update(&clip->eff, 1, 1, INT_MAX) after the step.  A non-finite norm without a dynamic scaler therefore SKIPS the
 * step (parameters, moments, packed weights, EMA untouched) and counts it -- torch would write NaN into every weight. */
typedef struct vpd_clip_state {
    vpd_scale_state eff;         /* what this step's AdamW and EMA read */
    float total_norm;            /* the last step's un-scaled gradient norm */
    float norm_max;              /* running maximum of the finite norms (reset by writing 0) */
    float coef;                  /* the last step's clip coefficient (1 when the norm was not finite) */
    int clipped_steps;           /* steps with coef < 1 */
    int nonfinite_steps;         /* steps whose norm was inf or NaN */
    int reserved[3];
} vpd_clip_state;
size_t vpd_clip_state_bytes(void);

/* The norm pass over `count` plain DEVICE float ranges x[i][0 .. n[i]) of any 4-byte alignment and any length >= 0 (x and n are
 * HOST arrays; more than 96 ranges take more than one launch), then the one-block kernel.  max_norm = +inf measures only.
 * Refused on the host, nothing launched: null clip, null x / n with count > 0, a null entry, negative n[i] or count, clip not
 * 16-byte aligned, src or an entry not 4-byte aligned, max_norm not > 0 or NaN, host_scale not positive and finite when src is
 * NULL. */
int vpd_op_grad_norm(const float* const* x, const long long* n, int count, double max_norm, const vpd_scale_state* src,
                     float host_scale, vpd_clip_state* clip, void* stream);
/* The same over exactly the ranges vpd_plan_check_grads enumerates (the plan's scratch and the non-conv ranges of `grads` while
 * vpd_plan_grads_pending(), else grads[0 .. numel)).  Floats of `grads` between tensors must be zero (they are in a buffer that was
 * zeroed once: no pass writes them).  Also refused: null plan / grads / workspace, an unbound workspace, numel not a multiple of 4
 * or below the plan's, grads not 16-byte aligned. */
int vpd_plan_grad_norm(vpd_plan_t* plan, const float* grads, long long numel, double max_norm, vpd_scale_state* src,
                       float host_scale, vpd_clip_state* clip, void* workspace, void* stream);

/* ---- AdamW parameter groups (torch.optim.AdamW's param_groups): lr and weight decay per group, betas and eps shared ----
 * Up to 16 groups.  The kernels find an element's group in a SEGMENT TABLE, a block of DEVICE memory owned by the caller
 * (vpd_adam_groups_bytes(nseg) bytes, 16-byte aligned), written once by vpd_adam_groups_init: segment s is the element range
 * [seg_begin[s], seg_begin[s + 1]) of the flat buffers and belongs to group seg_group[s]; adjacent tensors of one group form one
 * segment, and the padding floats between tensors (zero in every buffer, and zero after any step) belong to the segment in front.
 * Per group the step computes exactly what the ungrouped entry points compute from (lr[g], weight_decay[g]): with one group, or
 * with equal entries, the results are the same bits.  A group with lr = 0 and weight_decay = 0 keeps its parameters bit for bit
 * (p * 1.0f is exact and fma(-0, m / den, p) = p since den >= eps > 0); its moments are still updated, as torch's are. */
size_t vpd_adam_groups_bytes(int nseg);
/* Validates the HOST arrays seg_begin[nseg + 1] / seg_group[nseg] and copies them into `table` (the stream is synchronised before
 * the call returns: the host arrays may be freed).  Refused, nothing launched or copied: a null table / seg_begin / seg_group,
 * nseg < 1, ngroups outside 1..16, seg_begin[0] != 0, offsets not strictly ascending, seg_begin[nseg] != numel, numel not a multiple
 * of 4, a group id outside 0..ngroups-1, a table that is not 16-byte aligned.  With a plan (NULL: none) also a boundary strictly
 * inside one of the plan's conv weights (the fused kernel looks a conv's group up once per block) and numel !=
 * vpd_plan_param_numel(plan). */
int vpd_adam_groups_init(const vpd_plan_t* plan_or_null, void* table, const long long* seg_begin, const int* seg_group, int nseg,
                         long long numel, int ngroups, void* stream);
/* vpd_adamw_step / vpd_adamw_step_scaled with groups: lr[ngroups] and weight_decay[ngroups] are HOST arrays, copied into the
 * kernel's arguments.  state == NULL: `step` (1-based) and `gscale` (a factor on every gradient read: 1 / loss scale, or 1) are the
 * host's; else the device block decides as in vpd_adamw_step_scaled and both are ignored.  Refused on the host: a null buffer /
 * table / lr / weight_decay, ngroups outside 1..16, a negative or NaN lr or weight_decay (as torch refuses them), step < 1 without
 * a state, numel not a multiple of 4, a buffer or table that is not 16-byte aligned. */
int vpd_adamw_step_groups(float* params, const float* grads, float* adam_m, float* adam_v, long long numel, const void* table,
                          const double* lr, const double* weight_decay, int ngroups, double beta1, double beta2, double eps,
                          int step, float gscale, const vpd_scale_state* state, void* stream);
/* vpd_plan_adamw_step (state == NULL: the plan's loss scale applies) / vpd_plan_adamw_step_scaled with groups: the same launches --
 * the fused AdamW + repack reading the scratch while gradients are pending, then the stem repack -- and the same refusals, plus those
 * above.  numel must EQUAL vpd_plan_param_numel(plan): tensors beyond the plan's take vpd_adamw_step_groups. */
int vpd_plan_adamw_step_groups(vpd_plan_t* plan, float* params, const float* grads, float* adam_m, float* adam_v, long long numel,
                               const void* table, const double* lr, const double* weight_decay, int ngroups, double beta1,
                               double beta2, double eps, int step, const vpd_scale_state* state, void* workspace, void* stream);

/* Lazy gradients for the fused train step (reference: models/util.py:50-58, where nothing looks at .grad between
 * loss.backward() and optimizer.step()).  vpd_plan_set_lazy_grads(plan, 1) arms the NEXT vpd_backward: the conv weight
 * gradients then stay in the kernels' own fp32 scratch layout and vpd_plan_adamw_step reads them there, so the layout pass
 * into `grads` (170 MB of traffic per step) is skipped; every other tensor's gradient, and the stem's, is in `grads` as usual.
 * vpd_plan_grads_pending() tells whether `grads` is incomplete; vpd_plan_materialize_grads() completes it on demand (no-op
 * otherwise).  Under data parallelism (bucket events given) a lazy backward leaves bucket b's conv gradients in the workspace
 * range vpd_plan_bucket_scratch_range(plan, b) (byte offset into the workspace, fp32 count): a SUM all-reduce is layout-
 * agnostic (train_vpd_model.py:87: the loss is a sum over crops), so the reducer sums that range and the non-conv tensors
 * (+ the stem) of the flat buffer; bucket b's event is recorded when both are final.  While vpd_plan_grads_pending() == 1 an
 * all-reduce of the FLAT buffer's bucket ranges is invalid: the conv ranges of `grads` are stale and vpd_plan_adamw_step reads
 * the scratch -- a reducer must pick its buffers by vpd_plan_grads_pending(), not by its caller's word (vpd_amd/ddp.py does). */
int vpd_plan_set_lazy_grads(vpd_plan_t* plan, int on);
int vpd_plan_bucket_scratch_range(const vpd_plan_t* plan, int bucket, long long* ws_byte_offset, long long* numel);
int vpd_plan_grads_pending(const vpd_plan_t* plan);
int vpd_plan_materialize_grads(vpd_plan_t* plan, float* grads, void* workspace, void* stream);

/* ---- gradient accumulation over micro-batches (K backward passes per optimizer step) ----
 * The loss is a SUM over crops (train_vpd_model.py:87), so the gradient of a batch is the sum of its micro-batches' gradients: no
 * 1/K factor.  The backward passes overwrite; a caller-owned ACCUMULATOR holds the window's sum so far, and the last micro-batch's
 * live gradients take it in place, after which the non-finite search, the norm pass, every AdamW and the EMA run as always.
 *
 * vpd_op_grad_accumulate: dst[i][j] = add ? dst[i][j] + src[i][j] : src[i][j] for j < n[i], a plain fp32 add (correctly rounded,
 * no contraction, no scaling) over `count` pairs of DEVICE float ranges of any 4-byte alignment and any length >= 0 (the fast path
 * wants dst[i] and src[i] to share their 16-byte phase); a pair must not overlap.  add == 0 never reads dst.  dst / src / n are HOST
 * arrays, copied into the kernel's arguments; more than 64 pairs take more than one launch.  Refused on the host, nothing launched:
 * negative count (0 returns 0 and looks at nothing else), null dst / src / n, a null entry, negative n[i], an entry off a 4-byte
 * boundary, dst[i] == src[i]. */
int vpd_op_grad_accumulate(float* const* dst, const float* const* src, const long long* n, int count, int add, void* stream);
/* Floats of the accumulator of `plan`: an image of the weight-gradient scratch behind the stem's gradients (the union of the
 * vpd_plan_bucket_scratch_range ranges, in workspace order) followed by an image of the flat buffer (vpd_plan_param_numel). */
long long vpd_plan_grad_accum_numel(const vpd_plan_t* plan);
/* Acts over exactly the ranges vpd_plan_check_grads enumerates -- the scratch behind the stem and the non-conv ranges of `grads`
 * while vpd_plan_grads_pending(), else grads[0 .. numel) -- each paired with its place in `accum`, so an accumulator holds ONE
 * layout at a time and the caller keeps track of which.  mode 0: accum := live; mode 1: accum += live; both leave
 * vpd_plan_grads_pending() == 0 (the gradients are consumed without the layout pass; the conv ranges of `grads` stay stale).
 * mode 2: live += accum, the pending state left as it is: call it after the window's last backward, in the layout the accumulator
 * was filled in.  Refused on the host: null plan / grads / accum / workspace, a mode outside 0..2, accum or grads not 16-byte
 * aligned, an unbound workspace, numel not equal to vpd_plan_param_numel(plan). */
int vpd_plan_grad_accumulate(vpd_plan_t* plan, float* grads, long long numel, float* accum, int mode, void* workspace, void* stream);

/* Frozen BatchNorm for a TRAIN plan (the reference gets it from model.eval() with grad enabled: F.batch_norm(training=False) under
 * autograd): while on, vpd_forward_train normalises every BatchNorm with bn_running -- mean = running_mean, 1 / std =
 * 1 / sqrt(running_var + 1e-5) -- reads bn_running (now required) and leaves it unwritten; the convolutions still add their batch
 * sums to the plan's accumulator rows, which are consumed as always.  The forward records the mode it ran in on the plan, and
 * vpd_backward / vpd_backward_ext of that graph use the RECORDED mode (dz = gamma / std * g; dgamma, dbeta as ever), whatever the
 * flag says by then.  n == 0 stays legal.  Fails on the host for a null plan and for a plan with train == 0 (vpd_forward_eval runs
 * on folded running statistics already). */
int vpd_plan_set_bn_frozen(vpd_plan_t* plan, int on);

/* Parameter gradients of vpd_backward_ext (default 1 = on).  Off: the pass computes data gradients only -- d(loss)/d(x) into
 * dx_nchw, bit-identical to the full pass's -- and launches no weight-gradient kernel, slab sum, gradient unpack or head weight
 * gradient.  `grads` must still be non-null (the documented refusal stays) but is not written, for n == 0 too; the BatchNorm
 * launches store dgamma / dbeta into the plan's idle weight-gradient scratch.  bucket_events, if given, are still recorded.
 * vpd_backward is not affected.  Works in both BatchNorm modes.  Fails for a null plan and for a plan with train == 0. */
int vpd_plan_set_param_grads(vpd_plan_t* plan, int on);

/* hipGraph-captured eval forward for a fixed batch size (apply_vpd_model.py:152-168 inner
 * loop at BATCH_SIZE crops per call).  Capture binds the pointers given here. */
/* ---- train-time input pipeline on the device (the step right before the hot path) ----
 * One item of GenericDataset.__getitem__ (vpd_dataset/single_frame.py:168-206) from the decoded PNGs on:
 * u8 RGB -> /255 -> ColorJitter(brightness .2, contrast .2, saturation .05, hue .05) -> Normalize(mean, std)
 * (vpd_dataset/common.py:52-60, :87-92), mask noise (single_frame.py:178-191), flow decode u8/255 - 0.5
 * (common.py:62-69), concat + h-flip with x-flow negation (single_frame.py:193-203), RandomResizedCrop = crop +
 * bilinear resize to out_dim (common.py:49-50, :80).  The random DECISIONS are the caller's (one vpd_aug_params per
 * crop, sampled on the host in torchvision's order of draws); the device work is deterministic given them. */
typedef struct vpd_aug_params {
    int order[4];        /* ColorJitter ops in application order: 0 brightness, 1 contrast, 2 saturation, 3 hue; -1 = none */
    float factor[4];     /* brightness, contrast, saturation factors, hue shift (indexed by op id) */
    int flip;            /* h-flip (and negate flow x) */
    int noise;           /* add noise_sd * N(0,1) to the normalised RGB where mask != 0 */
    int crop_i, crop_j, crop_h, crop_w;   /* crop window (top, left, height, width) in the flipped image */
    unsigned int seed_lo, seed_hi;        /* Philox key of the device noise generator (when noise == NULL) */
} vpd_aug_params;

/* rgb_u8 [n][height][width][3] (RGB), flow_u8 [n][height][width][2] (x, y) or NULL (3-channel model), mask_u8
 * [n][height][width] or NULL, noise f32 [n][3][height][width] standard-normal draws or NULL (device Philox),
 * params: DEVICE array of n; mean_std6: HOST array {mean r,g,b, std r,g,b}; scratch: 8 * n floats on the device.
 * out_nchw: f32 [n][3 or 5][out_dim][out_dim] = the reference's batch['img'] (single_frame.py:206). */
int vpd_augment_crops(const unsigned char* rgb_u8, const unsigned char* flow_u8, const unsigned char* mask_u8,
                      const float* noise, const vpd_aug_params* params, int n, int height, int width, int out_dim,
                      const float* mean_std6, float noise_sd, float* out_nchw, float* scratch, void* stream);
/* Same pipeline, written straight into the plan's stem staging buffer (bf16 NHWC, zero border): follow with
 * vpd_forward_train / vpd_forward_eval with x == NULL.  out_dim is the plan's img size. */
int vpd_plan_stage_crops(vpd_plan_t* plan, const unsigned char* rgb_u8, const unsigned char* flow_u8,
                         const unsigned char* mask_u8, const float* noise, const vpd_aug_params* params, int n,
                         int height, int width, const float* mean_std6, float noise_sd, float* scratch,
                         void* workspace, void* stream);

/* Inference views of decoded u8 frames (apply_vpd_model.py:94-118 builds them through FrameDataset,
 * vpd_dataset/single_frame.py:377-400): view 0 = the frame, view 1 (k_views == 2) = its horizontal flip with the x-flow
 * negated; normalised like vpd_plan_stage_crops with identity parameters (bit-identical), no resize (height / width must be
 * the plan's), written to the stem staging buffer as n_frames * k_views crops in the order [f0 v0, f0 v1, f1 v0, ...].
 * Follow with vpd_forward_eval / vpd_graph_capture_eval with x == NULL. */
int vpd_plan_stage_views(vpd_plan_t* plan, const unsigned char* rgb_u8, const unsigned char* flow_u8, int n_frames,
                         int k_views, int height, int width, const float* mean_std6, void* workspace, void* stream);

/* Jittered inference views (apply_vpd_model.py --jitter J; FrameDataset, vpd_dataset/single_frame.py:373-400).  Per frame, in
 * the reference's order: [frame, J x jitter(frame), J x jitter(flip(frame)), flip(frame)] when flip, else [frame, J x
 * jitter(frame)]: K = (1 + jitter) * (1 + flip) views, n_frames * K crops in the order [f0 v0, f0 v1, ..., f1 v0, ...].
 * As in the reference, ColorJitter acts on the NORMALISED image (u8 / 255 - mean) / std, unclamped; every op clamps to [0, 1]
 * and the result is not normalised again; the jittered views of the flipped frame carry the UNFLIPPED, un-negated flow, only
 * the last view has the mirrored flow with x negated.  Views 0 and K - 1 are bit-identical to vpd_plan_stage_views' two.
 * params: DEVICE array of n_frames * jitter * (1 + flip) rows, frame-major in view order; only `order` and `factor` are read
 * (order[k] = -1 skips a slot); may be NULL when jitter == 0.  scratch: 8 floats per parameter row on the device (partial
 * sums of the contrast op's grey mean, added in a fixed order: the output is reproducible from launch to launch).
 * width must be a multiple of 4; at most 65535 views per call.  out_nchw: f32 [n_frames * K][3 or 5][height][width]. */
int vpd_augment_views(const unsigned char* rgb_u8, const unsigned char* flow_u8, const vpd_aug_params* params, int n_frames,
                      int jitter, int flip, int height, int width, const float* mean_std6, float* out_nchw, float* scratch,
                      void* stream);
/* Same views, written straight into the EVAL plan's stem staging buffer (height == width == the plan's image size): follow
 * with vpd_forward_eval / vpd_graph_capture_eval with x == NULL. */
int vpd_plan_stage_views_jitter(vpd_plan_t* plan, const unsigned char* rgb_u8, const unsigned char* flow_u8,
                                const vpd_aug_params* params, int n_frames, int jitter, int flip, int height, int width,
                                const float* mean_std6, float* scratch, void* workspace, void* stream);

int vpd_graph_capture_eval(vpd_plan_t* plan, const float* params, const float* x, int n, float* emb_out,
                           void* workspace, void* stream);
int vpd_graph_launch_eval(vpd_plan_t* plan, int n, void* stream);

/* The fused BatchNorm-backward launches synchronise their (fully resident) grid in the launch; every wait is bounded
 * (1 s) and a time-out is counted in a sticky word of the workspace instead of hanging the GPU.  Copies that count to
 * the host (synchronises `stream`); non-zero means the results of the step(s) since vpd_plan_init_workspace are not
 * to be trusted.  No reference counterpart (torch launches one kernel per BatchNorm pass). */
int vpd_plan_sync_errors(vpd_plan_t* plan, void* workspace, void* stream, unsigned* count_out);

/* Per-kernel-class timing for the roofline report (bench.py): when enabled, every conv launch is
 * bracketed by HIP events on its own stream.  One class per kernel family: 0 conv3x3_c64_persistent_kernel<224>,
 * 1 conv3x3_pws_kernel<256,128,352>, 2 conv3x3_pws_kernel<256,64,416> and <128,128,288>, 3 conv3x3_pws_kernel<128,64,288>
 * (conv3x3_ws_kernel, their one-tile-per-block twin, with VPD_PWS=0), 4 conv_igemm_kernel (gather), the ring GEMM conv1x1_ws_kernel
 * and the streaming 1x1 kernels, 5 conv_wgrad128_persistent_kernel / conv_wgrad_halo_grouped_kernel (stride-1 3x3, per stage, without the slab reduce),
 * 6 per-conv weight-gradient launches (stride-2 3x3 on conv_wgrad_halo_kernel, 1x1 on conv_wgrad_kernel),
 * 7 conv_stem_persistent_kernel.  vpd_plan_read_timing (nclasses >= 8) waits for the events, writes out[3*cls + {0,1,2}] = {launches, milliseconds, algorithmic FLOPs} and clears. */
int vpd_plan_set_timing(vpd_plan_t* plan, int enable);
int vpd_plan_read_timing(vpd_plan_t* plan, double* out, int nclasses);

/* ---- single-operator entry points (used by the parity tests; same kernels) ---- */
/* One implicit-GEMM conv launch on padded-NHWC bf16 tensors (forward conv or data-gradient conv).
 * tapset9 = {nr, nc, dy0, dys, dx0, dxs, w0, wrs, wcs}: tap (ir,ic) gathers input pixel
 * (y*istr + dy0 + ir*dys, x*istr + dx0 + ic*dxs) in padded coordinates and uses weight slice
 * w0 + ir*wrs + ic*wcs of w_bf16 [slice][Co][Kc].  stats (optional, pre-zeroed): f64 [16][2][Co] accumulator
 * rows (block b adds its per-channel sum / sum of squares into row b % 16 with fp64 atomics). */
int vpd_op_conv2d(const void* x_bf16, const void* w_bf16, void* y_bf16, double* stats, int n, int xHp, int xWp,
                  int xC, int yHp, int yWp, int yC, int ypad, int Hs, int Ws, int osub, int oph, int opw, int istr,
                  int Kc, int Co, const int* tapset9, int accumulate, void* stream);
int vpd_op_conv_bm(int M, int Co);
/* The same launch with the epilogues the plan uses besides store / statistics (stride-1 output grid, osub 1):
 *  - eval (models/module.py:41-47 folded: BatchNorm's running statistics as scale / shift [Co] floats, the block's identity
 *    path, ReLU): y = relu?(ep_scale * conv + ep_shift (+ res)), res = bf16 NHWC padded by 1 with Co channels or null;
 *  - accumulate onto a dense y (a data gradient on top of the identity path), the OLD value first multiplied by the ReLU
 *    bit map acc_mask [M][Co/8] (bit j of byte (m, c8) keeps channel 8 c8 + j) when given. */
int vpd_op_conv2d_ep(const void* x_bf16, const void* w_bf16, void* y_bf16, int n, int xHp, int xWp, int xC, int yHp, int yWp,
                     int yC, int ypad, int Hs, int Ws, int istr, int Kc, int Co, const int* tapset9, const float* ep_scale,
                     const float* ep_shift, const void* res_padded_bf16, int ep_relu, int accumulate,
                     const unsigned char* acc_mask, void* stream);
/* The same launch as a DATA GRADIENT that also takes the sums of the BatchNorm backward consuming its output d (epilogue
 * modes 6 / 7, reference: the reductions inside torch's batch_norm backward for models/module.py:41-43): g = d * mask with
 * mask = the ReLU bit map [M][Co/8] of that BatchNorm's activation, rows f64 [4][2][Co] (pre-zeroed) receive sum g and
 * sum g * z per channel (z: the BatchNorm's dense bf16 input [M][Co]).  y must be dense (ypad 0, yC == Co). */
int vpd_op_conv2d_bnsums(const void* x_bf16, const void* w_bf16, void* y_bf16, const void* bst_z_bf16,
                         const unsigned char* bst_mask, double* rows, int n, int xHp, int xWp, int xC, int Hs, int Ws,
                         int Kc, int Co, const int* tapset9, int accumulate, void* stream);
/* ... accumulating onto y, with the sums of TWO BatchNorms fed by the same g (epilogue mode 8: the first block of a stage,
 * whose input gradient goes to the bn2 of the block before and to the 1x1 branch's BatchNorm): rows as above, rows2 f64
 * [4][2][Co] (pre-zeroed) receive sum g and sum g * z2. */
int vpd_op_conv2d_bnsums2(const void* x_bf16, const void* w_bf16, void* y_bf16, const void* bst_z_bf16,
                          const unsigned char* bst_mask, double* rows, const void* bst_z2_bf16, double* rows2, int n, int xHp,
                          int xWp, int xC, int Hs, int Ws, int Kc, int Co, const int* tapset9, void* stream);
/* Host-only: what the convolution launcher decides, by its own code, for the arguments of a vpd_op_conv2d* call on the current
 * device.  flags: 1 statistics rows, 2 eval epilogue, 4 acc_mask, 8 BatchNorm sums, 16 of two BatchNorms.  out12 = {kernel class
 * (0 conv3x3_c64_persistent, 1 256 x 128, 2 128 x 128, 3 128 x 64, 6 256 x 64 tiles of conv3x3_ws / conv3x3_pws, 4 gather family,
 * 5 stem), persistent conv3x3_pws_kernel, image width of its compile-time-geometry instantiation or 0, conv3x3_c64x2 twin,
 * conv1x1_ws_kernel, conv1x1_stream_kernel, legacy conv3x3_halo_kernel, tile pixels, tile channels, epilogue mode, pixel tiles
 * of the busiest block, flags & 8: a kernel takes the sums}. */
int vpd_op_conv2d_dispatch(int n, int xHp, int xWp, int xC, int yHp, int yWp, int yC, int ypad, int Hs, int Ws, int osub, int oph,
                           int opw, int istr, int Kc, int Co, const int* tapset9, int accumulate, int flags, int* out12);
/* ... and, for the same arguments, whether the launch runs conv3x3_pws_kernel with its interior loaders (tiles of whole images on the
 * compile-time-geometry instantiations, VPD_PWS_INTERIOR): *out = 1 or 0. */
int vpd_op_conv2d_interior(int n, int xHp, int xWp, int xC, int yHp, int yWp, int yC, int ypad, int Hs, int Ws, int osub, int oph,
                           int opw, int istr, int Kc, int Co, const int* tapset9, int accumulate, int flags, int* out);
/* BatchNorm2d in training mode as the plan runs it (one launch: finalize + apply; models/module.py:41-43 + nn.BatchNorm2d):
 * rows f64 [4][2][C] hold the per-channel sum / sum of squares of z as the producing convolution's epilogue left them;
 * writes mean, rstd, scale = gamma rstd, shift = beta - mean scale, updates running_mean / running_var (momentum, unbiased
 * variance) when given, and out = relu?(scale z + shift (+ residual)) into the bf16 NHWC tensor padded by 1
 * ([n][H+2][W+2][C]; residual: same layout or null), plus the ReLU bit map [n H W][C/8] when mask_bits is given.
 * n, H, W >= 1, C a multiple of 8 in 8..4096 (vpd_op_bn_forward2 likewise): anything else is refused before the launch. */
int vpd_op_bn_forward(const void* z_bf16, const double* rows, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, float* mean, float* rstd, float* scale, float* shift, const void* res_padded_bf16,
                      void* out_padded_bf16, unsigned char* mask_bits, int n, int H, int W, int C, int relu, float momentum,
                      float eps, void* stream);
/* Frozen BatchNorm for the single-operator entry points (a test hook; process-wide, default off; read by these entry points
 * only, never by a plan: vpd_plan_set_bn_frozen is the plan's switch).  While on:
 *  vpd_op_bn_forward, vpd_op_bn_forward2, vpd_op_bn_finalize, vpd_op_conv1x1_bn / vpd_op_conv1x1_bn2 mode 1: mean = running_mean,
 *      rstd = 1 / sqrt(running_var + eps) (the launch's own instruction), scale / shift from those; all four vectors are written
 *      as always; running_mean / running_var are REQUIRED, read, and not written; the rows are not used (vpd_op_bn_finalize still
 *      zeroes them)
 *  vpd_op_bn_backward (both paths), vpd_op_bn_backward_pair, vpd_op_bn_backward_apply, vpd_op_stem_pool_backward,
 *      vpd_op_conv1x1_bn / vpd_op_conv1x1_bn2 mode 3: dz = gamma rstd g -- the two batch-mean terms are dropped; dgamma = sum g xhat
 *      and dbeta = sum g as always, with the mean / rstd the caller passes (the frozen forward's)
 * Modes 0 and 2 of the streaming entry points only take sums and do not depend on it.  Returns 0. */
int vpd_op_set_bn_frozen(int on);
/* vpd_op_bn_forward with the BatchNorm of a down-sampling branch in the same launch (bn_fwd_fused_kernel, res_kind 2):
 * out = relu?(BatchNorm(z) + BatchNorm2(z2)), z2 dense like z, rows2 / gamma2 / ... its own; running statistics of both
 * BatchNorms or of neither. */
int vpd_op_bn_forward2(const void* z_bf16, const double* rows, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, float* mean, float* rstd, float* scale, float* shift, const void* z2_bf16,
                       const double* rows2, const float* gamma2, const float* beta2, float* running_mean2, float* running_var2,
                       float* mean2, float* rstd2, float* scale2, float* shift2, void* out_padded_bf16, unsigned char* mask_bits,
                       int n, int H, int W, int C, int relu, float momentum, float eps, void* stream);
/* The finalize launch of the stem's BatchNorm and of the VPD_FUSED_BN=0 path (bn_finalize_kernel): rows f64 [16][2][C] hold the
 * sum / sum of squares over `count` pixels and are left zeroed; writes mean, rstd (fp64 1 / sqrt), scale, shift and updates
 * running_mean / running_var (both or neither) as vpd_op_bn_forward does. */
int vpd_op_bn_finalize(double* rows, const float* gamma, const float* beta, float* running_mean, float* running_var, float* mean,
                       float* rstd, float* scale, float* shift, int count, int C, float momentum, float eps, void* stream);
/* The apply launch of the VPD_FUSED_BN=0 path (bn_apply_kernel; test-only addition under ABI 5, tests/test_bn_forward_ops_gpu.py):
 * out = relu?(scale z + shift (+ residual)) into the NHWC tensor padded by 1, from coefficient vectors the caller supplies.
 * res_kind 0: no residual; 1: res padded by 1 like out; 2: res dense like z with its own rscale / rshift (a down-sampling branch).
 * n, H, W >= 1, C a multiple of 8 in 8..4096; refusals return non-zero with a message before anything is launched. */
int vpd_op_bn_apply(const void* z_bf16, const float* scale, const float* shift, const void* res_bf16, const float* rscale,
                    const float* rshift, int res_kind, void* out_padded_bf16, int n, int H, int W, int C, int relu, void* stream);
/* BatchNorm backward, finalize + apply in one launch (bn_bwd_apply_fused_kernel): rows f64 [4][2][C] hold sum g and sum g * z
 * with g = dy * mask (what vpd_op_conv2d_bnsums leaves there); writes dz = gamma rstd (g - mean(g) - xhat mean(g xhat)) into
 * the bf16 NHWC tensor padded by 1, dgamma = sum g xhat, dbeta = sum g. */
int vpd_op_bn_backward_apply(const void* dy_bf16, const void* z_bf16, const unsigned char* mask_bits, const double* rows,
                             const float* gamma, const float* mean, const float* rstd, void* dz_padded_bf16, float* dgamma,
                             float* dbeta, int n, int H, int W, int C, void* stream);
/* The same launch for TWO BatchNorms fed with one masked gradient (bn_bwd_apply_fused_kernel<true>: the last BatchNorm of a
 * down-sampling block and its 1x1 branch's): z2 dense like z; rows2 f64 [4][2][C] holds sum g again and sum g * z2 (as
 * vpd_op_conv2d_bnsums2 leaves them); its own gamma2 / mean2 / rstd2 and outputs dz2_padded / dgamma2 / dbeta2. */
int vpd_op_bn_backward_apply2(const void* dy_bf16, const void* z_bf16, const unsigned char* mask_bits, const double* rows,
                              const float* gamma, const float* mean, const float* rstd, void* dz_padded_bf16, float* dgamma,
                              float* dbeta, const void* z2_bf16, const double* rows2, const float* gamma2, const float* mean2,
                              const float* rstd2, void* dz2_padded_bf16, float* dgamma2, float* dbeta2, int n, int H, int W, int C,
                              void* stream);
/* A Bottleneck's closing 1x1 convolution TOGETHER with its train-mode BatchNorm, the convolution recomputed in every pass
 * instead of stored (conv1x1_bn_stream_kernel and its statistics pass; models/module.py:41-47 for a Bottleneck identity block).
 * x: bf16 NHWC padded by 1 ([n][H istr + 2][W istr + 2][Kc]), w: [Co][Kc]; z = conv(x) is never written.  rows: f64 [4][2][Co].
 *  mode 0  rows (pre-zeroed) receive sum z and sum z^2 of the element-rounded z
 *  mode 1  rows read; writes mean, rstd, scale, shift, updates running_mean / running_var (both or neither), out_padded =
 *          relu(scale z + shift + res_padded) ([n][H+2][W+2][Co], res the same layout) and, when given, its ReLU bit map mask_bits
 *          [n H W][Co/8]
 *  mode 2  dout (dense [n H W][Co]) and mask_bits read: rows (pre-zeroed) receive sum g and sum g z, g = dout * mask
 *  mode 3  those rows, gamma, mean, rstd, dout, mask_bits read; writes dz_padded ([n][H+2][W+2][Co]), dgamma, dbeta
 * Returns non-zero, and launches nothing, for a null argument the mode needs and for every shape the launcher's own
 * vpd_conv1x1_bn_eligible refuses (Kc not 64 / 128, Co no multiple of 256, stride 2, W not a divisor of 64, fewer pixel tiles
 * than twice the CU budget, VPD_BNECK_RECOMPUTE=0). */
int vpd_op_conv1x1_bn(int mode, const void* x_padded, const void* w, int n, int H, int W, int istr, int Kc, int Co, double* rows,
                      const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                      float* mean, float* rstd, float* scale, float* shift, const void* res_padded, void* out_padded,
                      unsigned char* mask_bits, const void* dout, void* dz_padded, float* dgamma, float* dbeta, void* stream);
/* The same for a down-sampling Bottleneck whose closing convolution (x, w) and 1x1 branch (x2, w2) both have 64 input channels and
 * stride 1 (conv1x1_bn2_stream_kernel): out = relu(BatchNorm(conv(x)) + BatchNorm2(conv2(x2))), Co = 256.  Modes 1..3 as above with
 * one set of BatchNorm arguments per convolution (mode 2: rows and rows2 receive sum g, sum g z and sum g, sum g z2); the two
 * statistics passes are two mode-0 calls of vpd_op_conv1x1_bn.  Refuses what vpd_conv1x1_bn2_eligible refuses. */
int vpd_op_conv1x1_bn2(int mode, const void* x_padded, const void* w, const void* x2_padded, const void* w2, int n, int H, int W,
                       int Kc, int Kc2, int Co, double* rows, double* rows2, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, float* mean, float* rstd, float* scale, float* shift,
                       const float* gamma2, const float* beta2, float* running_mean2, float* running_var2, float* mean2, float* rstd2,
                       float* scale2, float* shift2, float momentum, float eps, void* out_padded, unsigned char* mask_bits,
                       const void* dout, void* dz_padded, void* dz2_padded, float* dgamma, float* dbeta, float* dgamma2,
                       float* dbeta2, void* stream);
/* Host-only: what those launchers decide for n crops of H x W pixels on the current device, by their own code.  two: the
 * two-convolution kernel.  out5 = {eligible, pixel lanes, channel tiles, pixel tiles of the busiest block, stages of the LDS ring}
 * (all but the first 0 when not eligible). */
int vpd_op_conv1x1_bn_dispatch(int n, int H, int W, int Kc, int Co, int two, int* out5);
/* Stem BatchNorm + ReLU + MaxPool 3x3 s2 p1 in one launch (stem_pool_kernel / stem_pool_pair_kernel): z dense NHWC
 * [n][Hz][Wz][C] -> out, NHWC padded by opad ([n][Ho+2 opad][Wo+2 opad][C], Ho = (Hz-1)/2+1; the border is not written), and,
 * when idx is given (training), the window tap r*3+t of the FIRST maximum per output element, u8 dense [n][Ho][Wo][C]. */
int vpd_op_stem_pool_forward(const void* z, const float* scale, const float* shift, void* out_padded, unsigned char* idx,
                             int n, int Hz, int Wz, int C, int opad, void* stream);
/* The stem convolution's data gradient (conv_stem_dgrad_kernel, the launch vpd_backward_ext makes for dx_nchw; reference: the
 * input-gradient half of loss.backward(), models/util.py:52, through the 7x7 stride-2 padding-3 conv1 of models/module.py:58):
 * dx = conv_transpose2d(dz, w, stride 2, padding 3, output_padding 1).  dz: element type, dense NHWC [n][H/2][W/2][64]; w_oihw: the
 * fp32 master weight [64][c_in][7][7], rounded to the element type by the kernel (to the values vpd_pack_weights packs); dx_nchw:
 * f32 [n][c_in][H][W], 8-byte aligned, fp32 accumulation.  Refuses null pointers, c_in outside 1..8, H or W odd or below 32, n < 1,
 * a dx_nchw that is not 8-byte aligned. */
int vpd_op_stem_dgrad(const void* dz, const float* w_oihw, float* dx_nchw, int n, int c_in, int H, int W, void* stream);
/* Backward of the same through the pool, the ReLU and the train-mode BatchNorm (vpd_launch_stem_pool_bwd: sums, finalize,
 * dz): dpool dense [n][Ho][Wo][C], idx as written by the forward, dz dense like z.  pooled_padded (the forward's output,
 * opad 1) or null: with it (and VPD_STEM_POOLSUMS on) the sums are taken over the pooled positions.  rows: f64 [16][2][C],
 * zeroed (left zeroed); coef: fp32 [3][C] scratch; dgamma = sum g xhat, dbeta = sum g. */
int vpd_op_stem_pool_backward(const void* dpool, const unsigned char* idx, const void* z, const float* mean, const float* rstd,
                              const float* scale, const float* shift, const float* gamma, const float* beta,
                              const void* pooled_padded, double* rows, float* coef, void* dz, float* dgamma, float* dbeta,
                              int n, int Hz, int Wz, int C, void* stream);
/* BatchNorm backward with its own reduction: fused = 0 the three launches (reduce, finalize, apply; rows f64 [16][2][C] zeroed,
 * coef fp32 [3][C]), fused = 1 the single launch with a grid barrier (rows f64 [4][2][C] zeroed, sync: 2304 zeroed bytes, err:
 * the sticky time-out counter).  ReLU mask, one at most: act_padded (the stored activation, NHWC padded by 1; with write_g the
 * masked gradient is written back over dy), mask_bits ([n H W][C/8], fused only), mscale / mshift (mask = mscale z + mshift > 0).
 * dy_pooled (fused with mask_bits only): dy does not exist yet, it is elem(dy_pooled[b][c] / (H W)), which the launch also
 * writes to dy.  dz: NHWC padded by dzpad. */
int vpd_op_bn_backward(void* dy, const void* z, const void* act_padded, const unsigned char* mask_bits, const float* mscale,
                       const float* mshift, const float* dy_pooled, double* rows, float* coef, void* sync, unsigned* err,
                       const float* gamma, const float* mean, const float* rstd, void* dz, int dzpad, float* dgamma,
                       float* dbeta, int n, int H, int W, int C, int write_g, int fused, void* stream);
/* The two BatchNorms of a down-sampling block in one launch (bn_bwd_fused2_kernel): same dy, same activation mask, each its
 * own z, statistics, gamma, rows (f64 [4][2][C], zeroed) and outputs; dzA / dzB NHWC padded by 1.  dy is overwritten with the
 * masked gradient when it does not stay in LDS. */
int vpd_op_bn_backward_pair(void* dy, const void* act_padded, const void* zA, const float* meanA, const float* rstdA,
                            const float* gammaA, double* rowsA, void* dzA, float* dgammaA, float* dbetaA, const void* zB,
                            const float* meanB, const float* rstdB, const float* gammaB, double* rowsB, void* dzB,
                            float* dgammaB, float* dbetaB, void* sync, unsigned* err, int n, int H, int W, int C, void* stream);
/* Host-only: what the fused backward launcher derives for M pixels of C channels on the current device, by the launcher's own
 * code: out4 = {blocks, g stays in LDS, z stays in LDS (pair: the first z), pair: the second z stays in LDS}. */
int vpd_op_bn_backward_residency(int M, int C, int pair, int* out4);
/* Head (fp32): global average pool over the interior of an NHWC activation padded by pad and its gradient
 * dact = elem(dpooled / (H W)), dense; Y[M][N] = op(A) op(B) (+ bias[N]) (ReLU), ta: A stored [K][M], tb: B stored [N][K];
 * out[n] = sum_m A[m][n]; d = act > 0 ? d : 0; sum-MSE: loss_step = sum (e - t)^2, loss_accum += the same, de = 2 (e - t)
 * (de, loss_step, loss_accum: each optional). */
int vpd_op_avgpool(const void* act_padded, int n, int H, int W, int C, int pad, float* pooled, void* stream);
int vpd_op_avgpool_bwd(const float* dpooled, int n, int H, int W, int C, void* dact, void* stream);
int vpd_op_sgemm(const float* A, const float* B, float* Y, const float* bias, int M, int N, int K, int ta, int tb, int relu,
                 void* stream);
int vpd_op_colsum(const float* A, int M, int N, float* out, void* stream);
int vpd_op_relu_mask(float* d, const float* act, long long n, void* stream);
int vpd_op_mse(const float* e, const float* t, long long n, float* de, float* loss_step, double* loss_accum, void* stream);
/* dw[slice][Co][Kc] (fp32) += sum over output pixels of dz[m][co] * x[gather(m, tap)][kc].
 * slab: optional fp32 scratch of vpd_op_wgrad_slab_bytes() bytes; when given, eligible 3x3 stride-1 shapes use
 * the halo kernel (split partials in the slab + reduce), otherwise the generic kernel (fp32 atomics). */
int vpd_op_wgrad(const void* dz_bf16, const void* x_bf16, float* dw, int n, int dzHp, int dzWp, int dzC, int dzpad,
                 int xHp, int xWp, int xC, int Hs, int Ws, int istr, int Kc, int Co, const int* tapset9,
                 float* slab, void* stream);
size_t vpd_op_wgrad_slab_bytes(void);
/* Host-only: what the launcher behind vpd_op_wgrad decides for that geometry, by its own routing and split code; nothing is
 * launched and no device is needed.  has_slab: a slab is given; prefer_halo_1x1: the wish vpd_backward states for the 1x1
 * convolutions of the BasicBlock students (VPD_WGRAD_1X1=0 / 1 overrides it).  out9 = {kernel: 0 atomics, 1 stem, 2 halo 3x3,
 * 3 halo 1x1; pass instantiation (halo: 3, 4, 5, 10 or 13; stem: 4; atomics: 0); ring stages (atomics: its 2 LDS buffers); TR;
 * multi; NHP (halo: padded input pixels of a chunk's halo; stem: input pixels a chunk stages; atomics: 0); ksplit = grid.y;
 * cpb, chunks per split (64-pixel chunks; atomics: 128-pixel); grid.x}. */
int vpd_op_wgrad_dispatch(int n, int dzHp, int dzWp, int dzC, int dzpad, int xHp, int xWp, int xC, int Hs, int Ws, int istr, int Kc,
                          int Co, const int* tapset9, int has_slab, int prefer_halo_1x1, int* out9);
/* Grouped 64 x 64 weight gradients (conv_wgrad_halo_grouped_kernel) of `nprob` 3x3 stride-1 pad-1 convolutions in ONE launch: the
 * form vpd_backward uses for every such convolution whose output channels are no multiple of 128.  dims: 5 ints per problem
 * {n, H, W, Co, Ci}; dz[i], x[i]: zero-bordered NHWC [n][H+2][W+2][Co | Ci]; dw[i]: fp32 [9][Co][Ci], OVERWRITTEN; slab[i]: fp32
 * scratch of vpd_op_wgrad_group_slab_floats(Co, Ci) floats.  Refuses, before anything is launched: nprob outside 1..18, null
 * pointers, channels that are no multiple of 64, a plane the halo tiling does not take, problems whose halo pass counts differ.
 * vpd_op_wgrad_group_dispatch (host-only, the launcher's own split chooser): out = {pass instantiation, tasks, grid, halo passes}
 * followed by {ksplit, cpb, tiles} per problem, 4 + 3 nprob ints. */
size_t vpd_op_wgrad_group_slab_floats(int Co, int Ci);
int vpd_op_wgrad_group_dispatch(int nprob, const int* dims, int* out);
int vpd_op_wgrad_group(int nprob, const void* const* dz, const void* const* x, float* const* dw, float* const* slab, const int* dims,
                       void* stream);
/* A down-sampling BasicBlock's two weight gradients in ONE launch (the form vpd_backward uses at the three stage boundaries of
 * ResNet-18/34): the 3x3 stride-2 pad-1 conv1 (dz, dw [9][Co][Kc], tapset9 = its taps as for vpd_op_wgrad) and the 1x1 stride-2 pad-0
 * branch (dz2, dw2 [Co][Kc]) read the same x; dz2 has dz's geometry.  The branch rides on conv1's staged halo as a tenth tap.
 * Both gradients are OVERWRITTEN, bit for bit what the two vpd_op_wgrad calls on the halo path give.  slab, slab2: fp32 scratch of
 * vpd_op_wgrad_slab_bytes() bytes each (both required).  Fails -- nothing is launched -- for shapes the halo form does not take,
 * with VPD_WGRAD_DS_RIDE=0, and for an LDS layout over 160 KB. */
int vpd_op_wgrad_pair(const void* dz_bf16, const void* dz2_bf16, const void* x_bf16, float* dw, float* dw2, int n, int dzHp, int dzWp,
                      int dzC, int dzpad, int xHp, int xWp, int xC, int Hs, int Ws, int istr, int Kc, int Co, const int* tapset9,
                      float* slab, float* slab2, void* stream);
/* Host-only: dynamic LDS bytes of that launch for an Hs x Ws output (input 2 Hs x 2 Ws).  ns: stages of the dz + halo ring, 0 = the
 * launcher's own choice.  Returns 0: fits; 1: over the 160 KB of a compute unit (the launcher refuses such a layout); -1: the output
 * size has no halo geometry.  *bytes is set unless -1. */
int vpd_op_wgrad_pair_lds_bytes(int Hs, int Ws, int ns, long long* bytes);
/* dumps the ds_read_b64_tr_b16 fragments of one [128][64] bf16 tile: out [4][4][64][8] bf16 */
int vpd_op_tr_read_probe(const void* tile_bf16, void* out_bf16, void* stream);
/* Grouped weight gradients of `nprob` 3x3 pad-1 / 1x1 pad-0 convolutions (stride 1 or 2) on 128-channel-wide tiles in ONE persistent launch (the
 * form vpd_backward uses per ResNet stage; reference: the weight half of loss.backward(), models/util.py:52).
 * dims: 7 ints per problem {n, H, W, Co, Ci, stride, k} (H, W: output size; stride 1 or 2; k = 3: 3x3 pad 1, k = 1: 1x1 pad 0);
 * dz[i]: zero-bordered bf16 NHWC [n][H+2][W+2][Co]; x[i]: zero-bordered bf16 NHWC [n][stride*H+2][stride*W+2][Ci]; dw[i]: fp32
 * [k*k][Co][Ci]; slab[i]: vpd_op_wgrad128_slab_floats(Co, Ci) floats; dev_table: vpd_op_wgrad128_table_bytes() bytes.
 * A problem with k = 1, stride 1, Co no multiple of 128 and Ci a multiple of 128 runs with its operands swapped and its tiles stored
 * transposed, as vpd_backward states it; dw keeps the [Co][Ci] layout.
 * The schedule is rebuilt, uploaded into `table` and the stream synchronised on EVERY call (no cache keyed by the table's address:
 * a freed and re-allocated table would be taken for uploaded): not usable under stream capture, and not a timing entry point. */
size_t vpd_op_wgrad128_table_bytes(void);
size_t vpd_op_wgrad128_slab_floats(int Co, int Ci);
int vpd_op_wgrad128_group(int nprob, const void* const* dz, const void* const* x, float* const* dw, float* const* slab,
                          const int* dims, void* dev_table, void* stream);
/* Host-only: the schedule vpd_op_wgrad128_group would build for `n` problems given as {M, Co, Ci, halo pixels} quadruples on
 * a device of G compute units (pixel split per problem, LPT deal of the (problem, tile, split) tasks to G persistent blocks).
 * Returns the number of tasks (-1: bad argument / more than `cap`); tasks: 4 ints each (problem, tile, split, 0). */
int vpd_op_wgrad128_schedule(int n, const int* dims4, int G, int* ksplit, int* blk_begin, int* tasks, int cap,
                             double* est_us);

/* ---- the reference boundary one launch at a time (test-only additions under ABI 5; tests/test_boundary_ops_gpu.py).  Element
 * pointers are void* of the build's element type.  Every call returns non-zero with a vpd_last_error message on null or malformed
 * arguments, before anything is launched.  The three that need descriptors build them, and their block maps, with the code
 * vpd_plan_create uses, upload them for the launch and synchronise the stream before they return. ---- */
/* x: f32 [n][c][H][W] (c in 1..8, 4-byte aligned) -> out: elements [n][Hp][Wp][8], 16-byte aligned; pixel (y, x) goes to
 * (y + pad, x + pad), channels c..7 of it are zeroed, nothing else is written (Hp >= H + pad, Wp >= W + pad). */
int vpd_op_pack_input(const float* x_f32_nchw, int n, int c, int H, int W, void* out, int Hp, int Wp, int pad, void* stream);
/* master: f32 OIHW [Co][Ci][k][k] -> fwd_out: elements [tap][Co][Ci], dgr_out (or null): elements [tap][Ci][Co]; Co, Ci multiples
 * of 32, k in 1..3.  stem = 1 (k = 7, Ci in 1..8, dgr_out null): fwd_out is [r][Co][64], entry t * 8 + c, zero for t = 7 or c >= Ci. */
int vpd_op_pack_weights(const float* master, int Co, int Ci, int k, int stem, void* fwd_out, void* dgr_out, void* stream);
/* wg: f32 weight-gradient scratch [tap][Co][Kc] (the stem: [r][Co][Kc], entry t * 8 + c) -> grads_out: f32 OIHW [Co][Ci][k][k]. */
int vpd_op_unpack_grads(const float* wg, int Co, int Ci, int k, int Kc, int stem, float* grads_out, void* stream);
/* The fused AdamW + repack launch of vpd_plan_adamw_step (and nothing else: no stem repack) over a synthetic flat buffer of `numel`
 * floats (a multiple of 4): conv i has dims3[3i .. 3i+2] = {Co, Ci, k} and lies at offsets[i] (a multiple of 4 floats, ascending,
 * no overlap); whatever lies in front of, between and behind the convs is updated as plain ranges.  params, grads, adam_m, adam_v:
 * 16-byte aligned f32 [numel].  arena: elements, conv i's forward layout at 2 (n_0 + .. + n_{i-1}), n_i = Co Ci k k, its
 * data-gradient layout n_i behind it.  wg (or null): f32 scratch, conv i's [tap][Co][Ci] gradient at n_0 + .. + n_{i-1}; with it
 * the convs' gradients are read there and `grads` only over the plain ranges.  gscale multiplies every gradient read. */
int vpd_op_adamw_pack(int nconv, const int* dims3, const long long* offsets, long long numel, float* params, const float* grads,
                      float* adam_m, float* adam_v, void* arena, const float* wg, double lr, double beta1, double beta2, double eps,
                      double weight_decay, int step, float gscale, void* stream);
/* vpd_op_adamw_pack with parameter groups (vpd_adam_groups_init's HOST arrays over the synthetic buffer, lr[ngroups] /
 * weight_decay[ngroups]): the entry builds and uploads its own segment table and refuses a boundary inside a synthetic conv.
 * state (or null): a device block that decides as in vpd_plan_adamw_step_scaled; step and gscale are then ignored. */
int vpd_op_adamw_pack_groups(int nconv, const int* dims3, const long long* offsets, long long numel, float* params,
                             const float* grads, float* adam_m, float* adam_v, void* arena, const float* wg,
                             const long long* seg_begin, const int* seg_group, int nseg, const double* lr,
                             const double* weight_decay, int ngroups, double beta1, double beta2, double eps, int step,
                             float gscale, const vpd_scale_state* state, void* stream);
/* The weight gradients' slab sums, nprob (1..18) problems in one launch: dws[i][e] = sum over s < ksplits[i] of
 * slabs[i][s * nfloats[i] + e]; nfloats[i] a multiple of 4, pointers 16-byte aligned. */
int vpd_op_wgrad_reduce(int nprob, const float* const* slabs, float* const* dws, const long long* nfloats, const int* ksplits,
                        void* stream);
/* Zeroes count (0..16; 0: no launch) ranges of n4s[i] float4 at the 16-byte aligned ptrs[i] in one launch. */
int vpd_op_zero_ranges(float* const* ptrs, const long long* n4s, int count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
