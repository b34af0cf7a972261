// Host side of the optimizer step (no kernel: those are optim.hip's): AdamW over a plan or over flat buffers, the loss scale and
// the dynamic scaler's block, the non-finite search, the gradient norm of the clipping and the EMA of the weights.  Of the plan it
// reads the pack tables, the arena and the weight-gradient scratch -- never the topology.
#include <algorithm>
#include <utility>
#include <vector>

#include "plan.h"

namespace {

// What the step entries of a plan refuse alike once their own pointers are known: a workspace that is not the bound one, a numel
// that does not cover the plan's parameters, gradients off a 16-byte boundary (grads16 null: not looked at).  vpd_plan_grad_norm
// takes the workspace refusal last (ws_first = false).
int check_step_call(const vpd_plan* p, const void* workspace, long long numel, const float* grads16 = nullptr, bool ws_first = true) {
    const char* unbound = "workspace not initialised with vpd_plan_init_workspace";
    if (ws_first && p->bound_ws != workspace) return fail(unbound);
    if (numel % 4 || numel < p->nparam_padded) return fail("numel must be a multiple of 4 and cover the plan's parameters");
    if (reinterpret_cast<size_t>(grads16) & 15) return fail("grads must be 16-byte aligned");
    if (!ws_first && p->bound_ws != workspace) return fail(unbound);
    return 0;
}

// One body per AdamW pair: `a` says where step and gradient factor come from (AdamArgs, kernels.h)
int adamw_flat(float* params, const float* grads, float* adam_m, float* adam_v, long long numel, const AdamArgs& a, void* stream) {
    if (numel % 4) return fail("numel must be a multiple of 4 (use vpd_plan_param_numel)");
    if (!a.st && a.step < 1) return fail("step is 1-based");
    LCHECK(vpd_launch_adamw(params, grads, adam_m, adam_v, (long)numel, a, (hipStream_t)stream));
    return 0;
}
// (the stem repack runs either way: after a step the device block skipped it rewrites the values the arena already holds)
int adamw_plan(vpd_plan_t* p, float* params, const float* grads, float* adam_m, float* adam_v, long long numel, const AdamArgs& a,
               void* workspace, void* stream) {
    if (check_step_call(p, workspace, numel)) return -1;
    if (!a.st && a.step < 1) return fail("step is 1-based");
    hipStream_t s = (hipStream_t)stream;
    bf16_t* arena = plan_arena(p, workspace);
    LCHECK(vpd_launch_adamw_pack(plan_descs(p, workspace), plan_bmap_adam(p, workspace), (int)p->bmap_adam.size() / 2, params, grads,
                                 adam_m, adam_v, arena, a, s, p->grads_in_scratch ? plan_wg(p, workspace) : nullptr));
    p->grads_in_scratch = false;      // consumed, applied or not (the scratch is rewritten by the next backward)
    LCHECK(vpd_launch_pack_weights(plan_descs(p, workspace), (int)p->descs.size(), plan_bmap_pack(p, workspace),
                                   p->nstem_pack_blocks, params, arena, s));
    const long long done = p->nparam_padded;
    if (numel > done)      // tensors the plan does not use (a motion head on a plan built without it)
        LCHECK(vpd_launch_adamw(params + done, grads + done, adam_m + done, adam_v + done, (long)(numel - done), a, s));
    return 0;
}

int adamw_plan_groups(vpd_plan_t* p, float* params, const float* grads, float* adam_m, float* adam_v, long long numel,
                      const AdamGroupArgs& a, void* workspace, void* stream) {
    if (check_step_call(p, workspace, numel)) return -1;
    if (numel != p->nparam_padded) return fail("numel must equal vpd_plan_param_numel (tensors beyond the plan's: vpd_adamw_step_groups)");
    hipStream_t s = (hipStream_t)stream;
    bf16_t* arena = plan_arena(p, workspace);
    LCHECK(vpd_launch_adamw_pack_groups(plan_descs(p, workspace), plan_bmap_adam(p, workspace), (int)p->bmap_adam.size() / 2, params,
                                        grads, adam_m, adam_v, arena, a, s, p->grads_in_scratch ? plan_wg(p, workspace) : nullptr));
    p->grads_in_scratch = false;
    LCHECK(vpd_launch_pack_weights(plan_descs(p, workspace), (int)p->descs.size(), plan_bmap_pack(p, workspace),
                                   p->nstem_pack_blocks, params, arena, s));
    return 0;
}
// what both grouped step entries refuse of their buffers
int check_group_buffers(const float* params, const float* grads, const float* adam_m, const float* adam_v, const void* table,
                        long long numel) {
    if (!params || !grads || !adam_m || !adam_v || !table) return fail("null argument");
    if (numel % 4) return fail("numel must be a multiple of 4 (use vpd_plan_param_numel)");
    if ((reinterpret_cast<size_t>(params) | reinterpret_cast<size_t>(grads) | reinterpret_cast<size_t>(adam_m) |
         reinterpret_cast<size_t>(adam_v) | reinterpret_cast<size_t>(table)) & 15)
        return fail("params, grads, adam_m, adam_v and the group table must be 16-byte aligned");
    return 0;
}

// The ranges a pass reads (empty ones are dropped), handed to `launch` in FiniteRanges batches of at most FR_MAX
struct RangeBatcher {
    std::vector<std::pair<const float*, long>> ranges;
    void add(const float* x, long long n) {
        if (n > 0) ranges.emplace_back(x, (long)n);
    }
    size_t nlaunch() const { return (ranges.size() + FR_MAX - 1) / FR_MAX; }
    template <class Launch>
    hipError_t each(Launch&& launch) const {
        for (size_t at = 0; at < ranges.size(); at += FR_MAX) {
            FiniteRanges r;
            memset(&r, 0, sizeof r);
            for (size_t i = at; i < ranges.size() && i < at + FR_MAX; ++i) {
                r.ptr[r.count] = ranges[i].first;
                r.n[r.count++] = ranges[i].second;
            }
            const hipError_t e = launch(r);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
};

// Exactly what the optimizer step that follows will read: vpd_plan_adamw_step_scaled takes the conv weight gradients from the
// scratch while grads_in_scratch (everything behind the stem's: the stem is always unpacked into the flat buffer) and the ranges
// of the `stem == 2` descriptors from `grads`; otherwise all of `grads`.  The conv ranges of `grads` are STALE after a lazy
// backward and are not looked at.
RangeBatcher step_grad_ranges(const vpd_plan_t* p, const float* grads, long long numel, void* workspace) {
    RangeBatcher b;
    if (p->grads_in_scratch) {
        const long long stem_end = (long long)p->stem.ntaps * p->stem.Co * p->stem.Kc;
        b.add(plan_wg(p, workspace) + stem_end, p->wg_elems - stem_end);
        for (const PackDesc& d : p->descs)
            if (d.stem == 2) b.add(grads + d.src_off, d.numel);
        b.add(grads + p->nparam_padded, numel - p->nparam_padded);
    } else {
        b.add(grads, numel);
    }
    return b;
}

// One launch over the ranges (more than FR_MAX of them: one launch per FR_MAX)
int launch_check_finite(const RangeBatcher& b, vpd_scale_state* state, void* stream) {
    LCHECK(b.each([&](const FiniteRanges& r) { return vpd_launch_check_finite(r, state, (hipStream_t)stream); }));
    return 0;
}

int check_clip_args(double max_norm, const vpd_scale_state* src, float host_scale, const vpd_clip_state* clip) {
    if (!clip) return fail("grad norm: null clip state");
    if (reinterpret_cast<size_t>(clip) & 15) return fail("grad norm: clip state must be 16-byte aligned");
    if (reinterpret_cast<size_t>(src) & 3) return fail("grad norm: scale state must be 4-byte aligned");
    if (!(max_norm > 0.0)) return fail("grad norm: max_norm must be > 0 (+inf measures only)");
    if (!src && (!(host_scale > 0.f) || !(host_scale < 3.0e38f))) return fail("grad norm: host_scale must be a positive finite number");
    return 0;
}
// FR_MAX ranges per launch; launch l stores its blocks' sums in the slots behind launch l - 1's.  The grids depend on the ranges'
// lengths alone, so the bits of the result do too.
int launch_grad_norm(const RangeBatcher& b, double max_norm, vpd_scale_state* src, float host_scale, vpd_clip_state* clip,
                     void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const size_t nlaunch = b.nlaunch();
    if (nlaunch > CLIP_SLOTS) return fail("grad norm: too many ranges");
    const int cap = nlaunch ? (int)std::min<size_t>(2048, CLIP_SLOTS / nlaunch) : 0;
    double* partials = reinterpret_cast<double*>(clip + 1);
    int used = 0;
    LCHECK(b.each([&](const FiniteRanges& r) {
        const int grid = vpd_grad_sqsum_grid(r.n, r.count, cap);
        double* mine = partials + used;
        used += grid;
        return vpd_launch_grad_sqsum(r, grid, mine, s);
    }));
    LCHECK(vpd_launch_clip_finalize(clip, used, max_norm, src, host_scale, s));
    return 0;
}

// Gradient accumulation: (dst, src, n) pairs (empty ones are dropped), GA_MAX per launch
struct AccumBatcher {
    struct Pair { float* dst; const float* src; long n; };
    std::vector<Pair> pairs;
    void add(float* dst, const float* src, long long n) {
        if (n > 0) pairs.push_back(Pair{dst, src, (long)n});
    }
    int launch(bool add_mode, void* stream) const {
        for (size_t at = 0; at < pairs.size(); at += GA_MAX) {
            AccumRanges r;
            memset(&r, 0, sizeof r);
            for (size_t i = at; i < pairs.size() && i < at + GA_MAX; ++i) {
                r.dst[r.count] = pairs[i].dst;
                r.src[r.count] = pairs[i].src;
                r.n[r.count++] = pairs[i].n;
            }
            LCHECK(vpd_launch_grad_accum(r, add_mode, (hipStream_t)stream));
        }
        return 0;
    }
};

}  // namespace

// ---- gradient accumulation over micro-batches: the caller's accumulator and the live gradients of a plan ----
extern "C" int vpd_op_grad_accumulate(float* const* dst, const float* const* src, const long long* n, int count, int add,
                                      void* stream) {
    if (count < 0) return fail("grad accumulate: negative count");
    if (count == 0) return 0;
    if (!dst || !src || !n) return fail("grad accumulate: null argument");
    AccumBatcher b;
    for (int i = 0; i < count; ++i) {
        if (!dst[i] || !src[i]) return fail("grad accumulate: null range");
        if (n[i] < 0) return fail("grad accumulate: negative length");
        if ((reinterpret_cast<size_t>(dst[i]) | reinterpret_cast<size_t>(src[i])) & 3)
            return fail("grad accumulate: ranges must be 4-byte aligned");
        if (dst[i] == src[i]) return fail("grad accumulate: dst and src must differ");
        b.add(dst[i], src[i], n[i]);
    }
    return b.launch(add != 0, stream);
}

// the scratch behind the stem's gradients (the stem is always unpacked into the flat buffer), in floats
static long long accum_scratch_numel(const vpd_plan_t* p) {
    const long long stem_end = (long long)p->stem.ntaps * p->stem.Co * p->stem.Kc;
    return p->wg_elems > stem_end ? p->wg_elems - stem_end : 0;
}
extern "C" long long vpd_plan_grad_accum_numel(const vpd_plan_t* p) { return p ? accum_scratch_numel(p) + p->nparam_padded : 0; }

extern "C" int vpd_plan_grad_accumulate(vpd_plan_t* p, float* grads, long long numel, float* accum, int mode, void* workspace,
                                        void* stream) {
    if (!p || !grads || !accum || !workspace) return fail("null argument");
    if (mode < 0 || mode > 2) return fail("grad accumulate: mode outside 0..2");
    if (reinterpret_cast<size_t>(accum) & 15) return fail("grad accumulate: accum must be 16-byte aligned");
    if (check_step_call(p, workspace, numel, grads)) return -1;
    if (numel != p->nparam_padded) return fail("grad accumulate: numel must equal vpd_plan_param_numel (the accumulator holds the plan's tensors)");
    // every live range the step would read, paired with its image in the accumulator: [scratch behind the stem][flat buffer]
    const long long nscratch = accum_scratch_numel(p);
    const float* scratch = plan_wg(p, workspace) + (p->wg_elems - nscratch);
    AccumBatcher b;
    for (const auto& rg : step_grad_ranges(p, grads, numel, workspace).ranges) {
        float* live = const_cast<float*>(rg.first);
        const bool in_scratch = rg.first >= scratch && rg.first < scratch + nscratch;
        float* image = in_scratch ? accum + (rg.first - scratch) : accum + nscratch + (rg.first - grads);
        if (mode == 2) b.add(live, image, rg.second); else b.add(image, live, rg.second);
    }
    if (b.launch(mode != 0, stream)) return -1;
    if (mode != 2) p->grads_in_scratch = false;      // consumed: the next backward's materialize is a no-op
    return 0;
}

// ---- AdamW parameter groups: the segment table and the hyper-parameters of a grouped step (declared in plan.h) ----
int adam_groups_check(const long long* seg_begin, const int* seg_group, int nseg, long long numel, int ngroups) {
    if (!seg_begin || !seg_group) return fail("adam groups: null argument");
    if (nseg < 1) return fail("adam groups: nseg must be >= 1");
    if (ngroups < 1 || ngroups > VPD_MAX_PARAM_GROUPS) return fail("adam groups: ngroups outside 1..16");
    if (seg_begin[0] != 0) return fail("adam groups: seg_begin[0] must be 0");
    for (int i = 0; i < nseg; ++i)
        if (seg_begin[i + 1] <= seg_begin[i]) return fail("adam groups: seg_begin must ascend strictly");
    if (seg_begin[nseg] != numel) return fail("adam groups: seg_begin[nseg] must equal numel");
    if (numel % 4) return fail("adam groups: numel must be a multiple of 4");
    for (int i = 0; i < nseg; ++i)
        if (seg_group[i] < 0 || seg_group[i] >= ngroups) return fail("adam groups: group id outside 0..ngroups-1");
    return 0;
}
int adam_groups_check_convs(const std::vector<PackDesc>& descs, const long long* seg_begin, int nseg) {
    for (const PackDesc& d : descs) {
        if (d.stem == 2) continue;
        const long long a = d.src_off, b = a + (long long)d.Co * d.Ci * d.kh * d.kw;
        const long long* it = std::upper_bound(seg_begin, seg_begin + nseg + 1, a);      // the first boundary behind the conv's begin
        if (it != seg_begin + nseg + 1 && *it < b) return fail("adam groups: a segment boundary lies inside a conv weight");
    }
    return 0;
}
int adam_groups_upload(void* table, const long long* seg_begin, const int* seg_group, int nseg, int ngroups, hipStream_t s) {
    std::vector<char> host(vpd_adam_table_bytes(nseg), 0);
    int* hd = reinterpret_cast<int*>(host.data());
    hd[0] = nseg; hd[1] = ngroups;
    long long* begin = reinterpret_cast<long long*>(hd + 4);
    memcpy(begin, seg_begin, (size_t)(nseg + 1) * sizeof(long long));
    memcpy(begin + nseg + 1, seg_group, (size_t)nseg * sizeof(int));
    HCHECK(hipMemcpyAsync(table, host.data(), host.size(), hipMemcpyHostToDevice, s));
    HCHECK(hipStreamSynchronize(s));      // (`host` goes away)
    return 0;
}
int adam_group_args_check(const double* lr, const double* weight_decay, int ngroups, int step, const vpd_scale_state* state) {
    if (!lr || !weight_decay) return fail("adam groups: null lr or weight_decay");
    if (ngroups < 1 || ngroups > VPD_MAX_PARAM_GROUPS) return fail("adam groups: ngroups outside 1..16");
    for (int i = 0; i < ngroups; ++i) {
        if (!(lr[i] >= 0.0)) return fail("adam groups: lr must not be negative or NaN");
        if (!(weight_decay[i] >= 0.0)) return fail("adam groups: weight_decay must not be negative or NaN");
    }
    if (!state && step < 1) return fail("step is 1-based");
    if (reinterpret_cast<size_t>(state) & 3) return fail("scale state must be 4-byte aligned");
    return 0;
}

extern "C" size_t vpd_adam_groups_bytes(int nseg) { return nseg < 1 ? 0 : vpd_adam_table_bytes(nseg); }

extern "C" int vpd_adam_groups_init(const vpd_plan_t* p, void* table, const long long* seg_begin, const int* seg_group, int nseg,
                                    long long numel, int ngroups, void* stream) {
    if (!table) return fail("adam groups: null argument");
    if (adam_groups_check(seg_begin, seg_group, nseg, numel, ngroups)) return -1;
    if (reinterpret_cast<size_t>(table) & 15) return fail("adam groups: the table must be 16-byte aligned");
    if (p) {
        if (numel != p->nparam_padded) return fail("adam groups: numel must equal vpd_plan_param_numel");
        if (adam_groups_check_convs(p->descs, seg_begin, nseg)) return -1;
    }
    return adam_groups_upload(table, seg_begin, seg_group, nseg, ngroups, (hipStream_t)stream);
}

extern "C" int vpd_adamw_step_groups(float* params, const float* grads, float* adam_m, float* adam_v, long long numel,
                                     const void* table, const double* lr, const double* weight_decay, int ngroups, double beta1,
                                     double beta2, double eps, int step, float gscale, const vpd_scale_state* state, void* stream) {
    if (check_group_buffers(params, grads, adam_m, adam_v, table, numel)) return -1;
    if (adam_group_args_check(lr, weight_decay, ngroups, step, state)) return -1;
    LCHECK(vpd_launch_adamw_groups(params, grads, adam_m, adam_v, (long)numel,
                                   AdamGroupArgs{table, lr, weight_decay, ngroups, beta1, beta2, eps, step, gscale, state},
                                   (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_plan_adamw_step_groups(vpd_plan_t* p, float* params, const float* grads, float* adam_m, float* adam_v,
                                          long long numel, const void* table, const double* lr, const double* weight_decay,
                                          int ngroups, double beta1, double beta2, double eps, int step,
                                          const vpd_scale_state* state, void* workspace, void* stream) {
    if (!p || !workspace) return fail("null argument");
    if (check_group_buffers(params, grads, adam_m, adam_v, table, numel)) return -1;
    if (adam_group_args_check(lr, weight_decay, ngroups, step, state)) return -1;
    return adamw_plan_groups(p, params, grads, adam_m, adam_v, numel,
                             AdamGroupArgs{table, lr, weight_decay, ngroups, beta1, beta2, eps, step, 1.0f / p->loss_scale, state},
                             workspace, stream);
}

extern "C" int vpd_adamw_step(float* params, const float* grads, float* adam_m, float* adam_v, long long numel,
                              double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                              void* stream) {
    if (!params || !grads || !adam_m || !adam_v) return fail("null argument");
    return adamw_flat(params, grads, adam_m, adam_v, numel, AdamArgs{lr, beta1, beta2, eps, weight_decay, step, 1.f, nullptr}, stream);
}

extern "C" int vpd_plan_adamw_step(vpd_plan_t* p, float* params, const float* grads, float* adam_m, float* adam_v,
                                   long long numel, double lr, double beta1, double beta2, double eps,
                                   double weight_decay, int step, void* workspace, void* stream) {
    if (!p || !params || !grads || !adam_m || !adam_v || !workspace) return fail("null argument");
    return adamw_plan(p, params, grads, adam_m, adam_v, numel,
                      AdamArgs{lr, beta1, beta2, eps, weight_decay, step, 1.0f / p->loss_scale, nullptr}, workspace, stream);
}

// Loss scale of the NEXT backward passes of this plan and of vpd_plan_adamw_step (fp16 training; the reference's GradScaler,
// models/util.py:55-57, train_vpd_model.py:105): vpd_backward multiplies d(loss)/d(pred) by `scale`, so every gradient it leaves --
// flat buffer, weight-gradient scratch, what a reducer sums -- is scale x its value (no fp16 activation gradient underflows), and
// vpd_plan_adamw_step multiplies the gradients it reads by 1 / scale.  1 (the default) is exact arithmetic: nothing changes.
extern "C" int vpd_plan_set_loss_scale(vpd_plan_t* p, float scale) {
    if (!p) return fail("null plan");
    if (!(scale > 0.f) || !(scale < 3.0e38f)) return fail("loss scale must be a positive finite number");
    p->loss_scale = scale;
    return 0;
}

// ---- dynamic loss scaling: every decision is taken on the device, from the caller's vpd_scale_state block (include/vpd_hip.h) ----
extern "C" int vpd_plan_set_scale_state(vpd_plan_t* p, const vpd_scale_state* state) {
    if (!p) return fail("null plan");
    if (reinterpret_cast<size_t>(state) & 3) return fail("scale state must be 4-byte aligned");
    p->scale_state = state;
    return 0;
}

extern "C" int vpd_op_check_finite(const float* x, long long n, vpd_scale_state* state, void* stream) {
    if (!x || !state) return fail("null argument");
    if (n < 0) return fail("negative length");
    if (reinterpret_cast<size_t>(x) & 3) return fail("x must be 4-byte aligned");
    RangeBatcher b;
    b.add(x, n);
    return launch_check_finite(b, state, stream);
}

extern "C" int vpd_plan_check_grads(vpd_plan_t* p, const float* grads, long long numel, vpd_scale_state* state, void* workspace,
                                    void* stream) {
    if (!p || !grads || !state || !workspace) return fail("null argument");
    if (check_step_call(p, workspace, numel, grads)) return -1;
    return launch_check_finite(step_grad_ranges(p, grads, numel, workspace), state, stream);
}

// ---- gradient-norm clipping: the norm pass over the same ranges, then the one-block kernel that writes the caller's vpd_clip_state ----
extern "C" size_t vpd_clip_state_bytes(void) { return sizeof(vpd_clip_state) + (size_t)CLIP_SLOTS * sizeof(double); }

extern "C" int vpd_op_grad_norm(const float* const* x, const long long* n, int count, double max_norm, const vpd_scale_state* src,
                                float host_scale, vpd_clip_state* clip, void* stream) {
    if (check_clip_args(max_norm, src, host_scale, clip)) return -1;
    if (count < 0) return fail("grad norm: negative count");
    if (count > 0 && (!x || !n)) return fail("grad norm: null argument");
    RangeBatcher b;
    for (int i = 0; i < count; ++i) {
        if (!x[i]) return fail("grad norm: null range");
        if (n[i] < 0) return fail("grad norm: negative length");
        if (reinterpret_cast<size_t>(x[i]) & 3) return fail("grad norm: ranges must be 4-byte aligned");
        b.add(x[i], n[i]);
    }
    return launch_grad_norm(b, max_norm, const_cast<vpd_scale_state*>(src), host_scale, clip, stream);
}

extern "C" int vpd_plan_grad_norm(vpd_plan_t* p, const float* grads, long long numel, double max_norm, vpd_scale_state* src,
                                  float host_scale, vpd_clip_state* clip, void* workspace, void* stream) {
    if (!p || !grads || !workspace) return fail("null argument");
    if (check_clip_args(max_norm, src, host_scale, clip)) return -1;
    if (check_step_call(p, workspace, numel, grads, false)) return -1;
    return launch_grad_norm(step_grad_ranges(p, grads, numel, workspace), max_norm, src, host_scale, clip, stream);
}

extern "C" int vpd_adamw_step_scaled(float* params, const float* grads, float* adam_m, float* adam_v, long long numel,
                                     double lr, double beta1, double beta2, double eps, double weight_decay,
                                     const vpd_scale_state* state, void* stream) {
    if (!params || !grads || !adam_m || !adam_v || !state) return fail("null argument");
    return adamw_flat(params, grads, adam_m, adam_v, numel, AdamArgs{lr, beta1, beta2, eps, weight_decay, 1, 1.f, state}, stream);
}

// vpd_plan_adamw_step with the device block deciding
extern "C" int vpd_plan_adamw_step_scaled(vpd_plan_t* p, float* params, const float* grads, float* adam_m, float* adam_v,
                                          long long numel, double lr, double beta1, double beta2, double eps,
                                          double weight_decay, const vpd_scale_state* state, void* workspace, void* stream) {
    if (!p || !params || !grads || !adam_m || !adam_v || !state || !workspace) return fail("null argument");
    return adamw_plan(p, params, grads, adam_m, adam_v, numel, AdamArgs{lr, beta1, beta2, eps, weight_decay, 1, 1.f, state},
                      workspace, stream);
}

extern "C" int vpd_scale_state_update(vpd_scale_state* state, float growth, float backoff, int growth_interval, void* stream) {
    if (!state) return fail("null argument");
    if (!(growth >= 1.f) || !(growth < 3.0e38f)) return fail("growth factor must be finite and >= 1");
    if (!(backoff > 0.f) || !(backoff <= 1.f)) return fail("backoff factor must be in (0, 1]");
    if (growth_interval < 1) return fail("growth interval must be >= 1");
    LCHECK(vpd_launch_scale_update(state, growth, backoff, growth_interval, (hipStream_t)stream));
    return 0;
}

// Exponential moving average of the weights: every refusal is taken here, before anything is launched
extern "C" int vpd_ema_update(const float* const* src, float* const* dst, const long long* n, int count, double decay,
                              int warmup, int t, int t0, const vpd_scale_state* state, void* stream) {
    if (count < 0 || count > EMA_MAX) return fail("vpd_ema_update: count outside 0..4");
    if (!(decay >= 0.0 && decay <= 1.0)) return fail("vpd_ema_update: decay must be in [0, 1]");
    if (t < 0 || t0 < 0) return fail("vpd_ema_update: t and t0 must not be negative");
    if (reinterpret_cast<size_t>(state) & 3) return fail("vpd_ema_update: scale state must be 4-byte aligned");
    if (count == 0) return 0;
    if (!src || !dst || !n) return fail("vpd_ema_update: null argument");
    EmaRanges r;
    memset(&r, 0, sizeof r);
    for (int i = 0; i < count; ++i) {
        if (!src[i] || !dst[i]) return fail("vpd_ema_update: null argument");
        if (n[i] < 0) return fail("vpd_ema_update: negative length");
        if ((reinterpret_cast<size_t>(src[i]) | reinterpret_cast<size_t>(dst[i])) & 3)
            return fail("vpd_ema_update: src and dst must be 4-byte aligned");
        if (src[i] == dst[i]) return fail("vpd_ema_update: src and dst must differ");
        r.src[i] = src[i];
        r.dst[i] = dst[i];
        r.n[i] = (long)n[i];
    }
    r.count = count;
    LCHECK(vpd_launch_ema_update(r, decay, warmup != 0, t, t0, state, (hipStream_t)stream));
    return 0;
}
