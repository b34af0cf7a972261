// Network plan: owns the static description of the student (ResNet-18/34 BasicBlock or
// ResNet-50/101 / wide Bottleneck encoder + optional motion MLP), the workspace layout and tables, and the query, setter
// and workspace entry points of include/vpd_hip.h.  The passes that launch on it: step.hip; the optimizer step's host side:
// optim_step.hip; the single-operator entry points of the parity tests: ops.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <algorithm>
#include <vector>

#include "plan.h"

static thread_local std::string g_err;
int fail(const char* what, hipError_t e) {
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return -1;
}

extern "C" const char* vpd_last_error(void) { return g_err.c_str(); }
extern "C" const char* vpd_elem_dtype(void) { return VPD_ELEM_NAME; }      // "bf16" (libvpdhip.so) or "fp16" (libvpdhip_f16.so)
extern "C" int vpd_abi_version(void) { return 5; }      // 5: vpd_op_conv2d_dispatch, vpd_op_conv2d_bnsums2 (+ vpd_op_wgrad_pair, vpd_op_wgrad_pair_lds_bytes, vpd_op_conv1x1_bn, vpd_op_conv1x1_bn2, vpd_op_conv1x1_bn_dispatch, vpd_op_pack_input, vpd_op_pack_weights, vpd_op_unpack_grads, vpd_op_adamw_pack, vpd_op_wgrad_reduce, vpd_op_zero_ranges: test-only additions, no existing signature changed, number kept); 2: round 5/6 entry points (vpd_op_conv2d_ep, train flag word, 8 timing classes); 3: dynamic loss scaling (vpd_scale_state); 4: operator entry points of the stem pool, the BatchNorm backward launchers and the head

namespace {

struct Bump {
    size_t cur = 0;
    size_t take(size_t bytes) {
        size_t o = cur;
        cur += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

inline size_t padded_elems(int n, int H, int W, int C, int pad) {
    return (size_t)n * (H + 2 * pad) * (W + 2 * pad) * C;
}

void add_tensor(vpd_plan* p, int kind, int is_dec, long long numel, int ndim, int d0, int d1, int d2, int d3,
                long long* off_out) {
    TensorRow r;
    r.kind = kind; r.is_dec = is_dec; r.off = p->nparam; r.numel = numel; r.ndim = ndim;
    r.dims[0] = d0; r.dims[1] = d1; r.dims[2] = d2; r.dims[3] = d3;
    p->tensors.push_back(r);
    *off_out = p->nparam;
    p->nparam += numel;
}

}  // namespace

// packed-weight geometry of a conv: the stem keeps one tap per kernel ROW, its 7 column taps x 8 channels in a 64-wide K
void set_pack_geom(ConvInfo& c, int Ci, int Co, int k, bool stem) {
    c.Ci = Ci; c.Co = Co; c.k = k; c.stem = stem;
    if (stem) { c.Kc = 64; c.ntaps = k; } else { c.Kc = Ci; c.ntaps = k * k; }
}

// ---- pack descriptors + block maps: the tables of pack_weights_kernel, unpack_grads_kernel and adamw_pack_kernel (optim.hip).
// vpd_plan_create builds the plan's with these two functions, the vpd_op_pack_weights / vpd_op_unpack_grads / vpd_op_adamw_pack
// entry points build a test's: one construction, so that an operator test runs the maps the train step runs ----
// Appends c's descriptor, its blocks of the pack map and of `bmap_unpack` (a bucket's unpack map); returns the descriptor's index.
int push_pack_desc(std::vector<PackDesc>& descs, std::vector<int>& bmap_pack, std::vector<int>& bmap_unpack, const ConvInfo& c) {
    PackDesc d;
    d.src_off = c.w_off; d.fwd_off = c.fwd_off; d.dgr_off = c.dgr_off; d.wg_off = c.wg_off;
    d.Co = c.Co; d.Ci = c.Ci; d.kh = c.k; d.kw = c.k; d.Kc = c.Kc; d.ntaps = c.ntaps; d.stem = c.stem ? 1 : 0;
    d.numel = 0;
    const int id = (int)descs.size();
    descs.push_back(d);
    const long long nf = (long long)c.ntaps * c.Co * c.Kc;
    const long long ns = (long long)c.Co * c.Ci * c.k * c.k;
    const long long npk = nf > ns ? nf : ns;
    // pack kernel: 32x32 (co x ci) tiles for ordinary convs, PACK_CHUNK element chunks for the stem
    const long long npack = c.stem ? (npk + 1023) / 1024 : (long long)(c.Co / 32) * (c.Ci / 32);
    for (long long ch = 0; ch < npack; ++ch) { bmap_pack.push_back(id); bmap_pack.push_back((int)ch); }
    const long long uchunk = 1024;     // PACK_CHUNK of unpack_grads_kernel
    for (long long ch = 0; ch * uchunk < ns; ++ch) { bmap_unpack.push_back(id); bmap_unpack.push_back((int)ch); }
    return id;
}
// Block map of the fused AdamW + repack launch over [0, nparam_padded): every conv tile as in the pack map -- not descriptor
// `stem_id`'s (-1: there is none), whose blocks are counted into nstem_pack_blocks instead -- then the ranges that are not one of
// the other descriptors' conv weights, in 2048-float chunks (ADAM_PLAIN_CHUNK of optim.hip), as `stem == 2` descriptors appended
// to `descs`.
void build_adam_map(std::vector<PackDesc>& descs, const std::vector<int>& bmap_pack, int stem_id, long long nparam_padded,
                    std::vector<int>& bmap_adam, int& nstem_pack_blocks) {
    const int nconv = (int)descs.size();
    // (the stem is a plain range here, packed by a 28-block pack_weights_kernel launch afterwards.  Round 4 tried ONE
    //  block of this launch for it -- update, then the row-tap packing, which gathers across the whole tensor: its ~30 dependent
    //  round trips under the launch's 5 TB/s of traffic made it the launch's pole, 155 vs 131 us, profiles/r04_small_folds.txt)
    for (size_t i = 0; i + 1 < bmap_pack.size(); i += 2) {
        if (bmap_pack[i] == stem_id) { nstem_pack_blocks++; continue; }
        bmap_adam.push_back(bmap_pack[i]); bmap_adam.push_back(bmap_pack[i + 1]);
    }
    std::vector<std::pair<long long, long long>> convs;                   // (offset, numel), ascending
    for (int i = 0; i < nconv; ++i)
        if (i != stem_id) convs.push_back({descs[i].src_off, (long long)descs[i].Co * descs[i].Ci * descs[i].kh * descs[i].kw});
    std::sort(convs.begin(), convs.end());
    long long pos = 0;
    auto plain = [&](long long a, long long b) {
        if (b <= a) return;
        PackDesc d = {};
        d.src_off = a; d.numel = b - a; d.stem = 2; d.kh = d.kw = 1; d.dgr_off = -1;
        const int id = (int)descs.size();
        descs.push_back(d);
        for (long long ch = 0; ch * 2048 < b - a; ++ch) { bmap_adam.push_back(id); bmap_adam.push_back((int)ch); }
    };
    for (auto& cv : convs) { plain(pos, cv.first); pos = cv.first + cv.second; }
    plain(pos, nparam_padded);
}

namespace {

void add_conv(vpd_plan* p, ConvInfo& c, int Ci, int Co, int k, int stride, int pad, int Hin, int Win, bool stem) {
    set_pack_geom(c, Ci, Co, k, stem);
    c.stride = stride; c.pad = pad; c.Hin = Hin; c.Win = Win;
    c.Hout = (Hin + 2 * pad - k) / stride + 1;
    c.Wout = (Win + 2 * pad - k) / stride + 1;
    add_tensor(p, 0, 0, (long long)Co * Ci * k * k, 4, Co, Ci, k, k, &c.w_off);
    c.bn.C = Co;
    add_tensor(p, 1, 0, Co, 1, Co, 0, 0, 0, &c.bn.w_off);
    add_tensor(p, 2, 0, Co, 1, Co, 0, 0, 0, &c.bn.b_off);
    c.bn.rm_off = p->nbn; c.bn.rv_off = p->nbn + Co;
    p->nbn += 2 * Co;
    c.fwd_off = p->arena_elems;
    p->arena_elems += (long long)c.ntaps * Co * c.Kc;
    if (!stem) {
        c.dgr_off = p->arena_elems;
        p->arena_elems += (long long)k * k * Ci * Co;
    }
    c.wg_off = p->wg_elems;
    p->wg_elems += (long long)c.ntaps * Co * c.Kc;
    // split slabs of the single (not grouped) halo launches: TWO regions of the maximum size -- region 0 for the stem and the
    // 3x3 convs, region 1 for the 1x1 convs, so that a down-sampling block's two weight gradients can both wait for their
    // stage's slab-reduce launch (round 4); a region is summed before it is written again
    if (stem && p->train && p->slab_elems == 0)
        p->slab_elems += 2 * (long long)(vpd_wgrad_slab_bytes() / 4);
    if (!stem && ((k == 3 && pad == 1) || (k == 1 && pad == 0)) && (stride == 1 || stride == 2) && p->train &&
        vpd_wgrad_halo_shape_ok(c.Hout, c.Wout, stride, Hin, Win)) {
        // halo wgrad conv: ONE shared slab, summed right after each wgrad launch while it is still in the Infinity
        // Cache (per-conv slabs summed once per bucket were measured 4 % slower: 490 MB fall out of the cache)
        c.slab_off = k == 1 ? (long long)(vpd_wgrad_slab_bytes() / 4) : 0;
    }
}

}  // namespace

// ---------------------------------------------------------------------------
extern "C" int vpd_plan_create(const char* arch, int c_in, int img_h, int img_w, int emb_dim, int motion,
                               int max_batch, int train, vpd_plan_t** out) {
    if (!arch || !out) return fail("null argument");
    std::vector<int> layers;
    int bottleneck = 0, base_width = 64;          // reference models/module.py:17-32 (ENCODER_ARCH)
    if (!strcmp(arch, "resnet18")) layers = {2, 2, 2, 2};
    else if (!strcmp(arch, "resnet34")) layers = {3, 4, 6, 3};
    else if (!strcmp(arch, "resnet50")) { layers = {3, 4, 6, 3}; bottleneck = 1; }
    else if (!strcmp(arch, "resnet101")) { layers = {3, 4, 23, 3}; bottleneck = 1; }
    else if (!strcmp(arch, "wide_resnet50_2")) { layers = {3, 4, 6, 3}; bottleneck = 1; base_width = 128; }
    else if (!strcmp(arch, "wide_resnet101_2")) { layers = {3, 4, 23, 3}; bottleneck = 1; base_width = 128; }
    else return fail("unsupported arch (resnet18 | resnet34 | resnet50 | resnet101 | wide_resnet50_2 | wide_resnet101_2)");
    if (c_in < 1 || c_in > 8) return fail("c_in must be in 1..8");
    if (img_h < 32 || img_w < 32 || (img_h % 2) || (img_w % 2)) return fail("img dims must be even and >= 32");
    if (emb_dim < 1 || max_batch < 1) return fail("bad emb_dim / max_batch");

    vpd_plan* p = new vpd_plan();
    p->c_in = c_in; p->H = img_h; p->W = img_w; p->D = emb_dim; p->motion = motion ? 1 : 0;
    p->max_batch = max_batch; p->train = train ? 1 : 0; p->layers = layers;
    p->early_bucket0 = (train & VPD_TRAIN_EARLY_BUCKET0) != 0;
    p->bottleneck = bottleneck; p->base_width = base_width; p->feat = bottleneck ? 2048 : 512;

    // ---- topology + flat tables (reference module order) ----
    add_conv(p, p->stem, c_in, 64, 7, 2, 3, img_h, img_w, true);
    p->bns.push_back(&p->stem.bn);
    p->H0 = p->stem.Hout; p->W0 = p->stem.Wout;
    p->H1 = (p->H0 + 2 - 3) / 2 + 1; p->W1 = (p->W0 + 2 - 3) / 2 + 1;
    int inplanes = 64, h = p->H1, w = p->W1;
    const int widths[4] = {64, 128, 256, 512};
    long long stage_first_tensor_off[5];
    int nblocks_total = 0;
    for (int s = 0; s < 4; ++s) nblocks_total += layers[s];
    p->blocks.resize(nblocks_total);
    int bi = 0;
    for (int s = 0; s < 4; ++s) {
        stage_first_tensor_off[s] = p->nparam;
        for (int b = 0; b < layers[s]; ++b, ++bi) {
            BlockInfo& B = p->blocks[bi];
            const int stride = (b == 0 && s > 0) ? 2 : 1;
            B.stage = s;
            if (!bottleneck) {
                add_conv(p, B.c1, inplanes, widths[s], 3, stride, 1, h, w, false);
                add_conv(p, B.c2, widths[s], widths[s], 3, 1, 1, B.c1.Hout, B.c1.Wout, false);
                B.ds = (stride != 1 || inplanes != widths[s]);
                if (B.ds) add_conv(p, B.cd, inplanes, widths[s], 1, stride, 0, h, w, false);
                h = B.c1.Hout; w = B.c1.Wout; inplanes = widths[s];
            } else {
                // torchvision Bottleneck ("v1.5": the 3x3 carries the stride), state_dict order conv1 bn1 conv2 bn2
                // conv3 bn3 downsample.0 downsample.1
                const int width = widths[s] * base_width / 64, outc = widths[s] * 4;
                add_conv(p, B.c1, inplanes, width, 1, 1, 0, h, w, false);
                add_conv(p, B.c2, width, width, 3, stride, 1, h, w, false);
                add_conv(p, B.c3, width, outc, 1, 1, 0, B.c2.Hout, B.c2.Wout, false);
                B.ds = (stride != 1 || inplanes != outc);
                if (B.ds) add_conv(p, B.cd, inplanes, outc, 1, stride, 0, h, w, false);
                h = B.c2.Hout; w = B.c2.Wout; inplanes = outc;
            }
        }
        p->stages[s].H = h; p->stages[s].W = w; p->stages[s].C = inplanes;
    }
    for (auto& B : p->blocks) {     // BN module order: bn1, bn2, (bn3,) downsample.1
        p->bns.push_back(&B.c1.bn);
        p->bns.push_back(&B.c2.bn);
        if (bottleneck) p->bns.push_back(&B.c3.bn);
        if (B.ds) p->bns.push_back(&B.cd.bn);
    }
    // data-only backward (vpd_plan_set_param_grads): every BatchNorm's dgamma / dbeta land in [2][C] floats of its own at the front of
    // the weight-gradient scratch (each BatchNorm follows a convolution with more than 2 weights per output channel: it fits)
    {
        long long at = 0;
        for (BnInfo* b : p->bns) { b->sink_off = at; at += 2LL * b->C; }
    }
    if (h < 1 || w < 1) { delete p; return fail("image too small for 5 stride-2 stages"); }
    stage_first_tensor_off[4] = p->nparam;
    p->fc.in = p->feat; p->fc.out = emb_dim;
    add_tensor(p, 3, 0, (long long)emb_dim * p->feat, 2, emb_dim, p->feat, 0, 0, &p->fc.w_off);
    add_tensor(p, 4, 0, emb_dim, 1, emb_dim, 0, 0, 0, &p->fc.b_off);
    if (p->motion) {
        const int dims[4] = {emb_dim, 128, 128, 2 * emb_dim};
        for (int i = 0; i < 3; ++i) {
            p->dec[i].in = dims[i]; p->dec[i].out = dims[i + 1];
            add_tensor(p, 3, 1, (long long)dims[i + 1] * dims[i], 2, dims[i + 1], dims[i], 0, 0, &p->dec[i].w_off);
            add_tensor(p, 4, 1, dims[i + 1], 1, dims[i + 1], 0, 0, 0, &p->dec[i].b_off);
        }
    }
    p->nparam_padded = (p->nparam + 3) & ~3LL;
    // buckets in completion order
    p->bucket_off[0] = stage_first_tensor_off[3]; p->bucket_numel[0] = p->nparam - stage_first_tensor_off[3];
    p->bucket_off[1] = stage_first_tensor_off[2]; p->bucket_numel[1] = stage_first_tensor_off[3] - stage_first_tensor_off[2];
    p->bucket_off[2] = stage_first_tensor_off[1]; p->bucket_numel[2] = stage_first_tensor_off[2] - stage_first_tensor_off[1];
    p->bucket_off[3] = 0; p->bucket_numel[3] = stage_first_tensor_off[1];

    // ---- pack descriptors + block maps (push_pack_desc, build_adam_map above) ----
    auto push_desc = [&](const ConvInfo& c, int bucket) { push_pack_desc(p->descs, p->bmap_pack, p->bmap_unpack[bucket], c); };
    push_desc(p->stem, 3);
    p->nstem_unpack_blocks = (int)p->bmap_unpack[3].size() / 2;
    for (int b = 0; b < 4; ++b) { p->bucket_wg_off[b] = -1; p->bucket_wg_numel[b] = 0; }
    for (auto& B : p->blocks) {
        const int bucket = 3 - B.stage;
        push_desc(B.c1, bucket);
        push_desc(B.c2, bucket);
        if (bottleneck) push_desc(B.c3, bucket);
        if (B.ds) push_desc(B.cd, bucket);
        // the scratch is laid out in construction order (add_conv), stage after stage: a bucket's convs are ONE range
        auto take = [&](const ConvInfo& cv) {
            const long long n = (long long)cv.ntaps * cv.Co * cv.Kc;
            if (p->bucket_wg_off[bucket] < 0) p->bucket_wg_off[bucket] = cv.wg_off;
            p->bucket_wg_off[bucket] = std::min(p->bucket_wg_off[bucket], (long long)cv.wg_off);
            p->bucket_wg_numel[bucket] += n;
        };
        take(B.c1); take(B.c2);
        if (bottleneck) take(B.c3);
        if (B.ds) take(B.cd);
    }
    {
        // contiguity check: the four ranges tile [stem's end, wg_elems) in bucket order 3, 2, 1, 0
        long long at = (long long)p->stem.ntaps * p->stem.Co * p->stem.Kc;
        for (int b = 3; b >= 0; --b) {
            if (p->bucket_wg_off[b] != at) { delete p; return fail("internal: weight-gradient scratch is not bucket-contiguous"); }
            at += p->bucket_wg_numel[b];
        }
        if (at != p->wg_elems) { delete p; return fail("internal: weight-gradient scratch size mismatch"); }
    }
    // block map of vpd_plan_adamw_step (descs[0] is the stem)
    build_adam_map(p->descs, p->bmap_pack, 0, p->nparam_padded, p->bmap_adam, p->nstem_pack_blocks);

    // ---- workspace layout ----
    Bump bp;
    const int NB = max_batch;
    p->xHp = img_h + 6; p->xWp = img_w + 8;
    p->xin_off = bp.take(((size_t)NB * p->xHp * p->xWp * 8 + 256) * 2);
    p->arena_off = bp.take((size_t)p->arena_elems * 2);
    p->wg_off = bp.take((size_t)p->wg_elems * 4);
    for (BnInfo* b : p->bns) b->fl_off = bp.take((size_t)9 * b->C * 4);
    p->fused_bn = vpd_switches().fused_bn;
    {
        const size_t start = bp.cur;
        for (BnInfo* b : p->bns) {
            b->rows_off = bp.take((size_t)VPD_FUSED_ROWS * 2 * b->C * sizeof(double));
            b->sync_off = bp.take(VPD_GRID_SYNC_BYTES);
        }
        p->fused_off = start; p->fused_bytes = bp.cur - start;      // (Bump rounds every piece to 256 B: 16-byte multiples)
        p->syncerr_off = bp.take(256);
    }
    p->desc_off = bp.take(p->descs.size() * sizeof(PackDesc));
    p->bmap_pack_off = bp.take(p->bmap_pack.size() * sizeof(int));
    p->bmap_adam_off = bp.take(p->bmap_adam.size() * sizeof(int));
    for (int i = 0; i < 4; ++i) p->bmap_unpack_off[i] = bp.take(p->bmap_unpack[i].size() * sizeof(int) + 16);
    // statistics partials: producers accumulate atomically into VPD_STAT_ROWS rows of [2][C]
    p->partial_bytes = (size_t)VPD_STAT_ROWS * 2 * p->feat * sizeof(double);
    p->partial_off = bp.take(p->partial_bytes);
    p->z0_off = bp.take((size_t)NB * p->H0 * p->W0 * 64 * 2);
    p->p0_off = bp.take(padded_elems(NB, p->H1, p->W1, 64, 1) * 2);
    for (auto& B : p->blocks) {
        B.a1_off = bp.take(padded_elems(NB, B.c1.Hout, B.c1.Wout, B.c1.Co, 1) * 2);
        if (bottleneck) {
            B.a2_off = bp.take(padded_elems(NB, B.c2.Hout, B.c2.Wout, B.c2.Co, 1) * 2);
            B.out_off = bp.take(padded_elems(NB, B.c3.Hout, B.c3.Wout, B.c3.Co, 1) * 2);
        } else {
            B.out_off = bp.take(padded_elems(NB, B.c1.Hout, B.c1.Wout, B.c1.Co, 1) * 2);
        }
    }
    for (int s = 0; s < 4; ++s) {
        StageInfo& S = p->stages[s];
        S.idn_off = bp.take(padded_elems(NB, S.H, S.W, S.C, 1) * 2);
    }
    p->pooled_off = bp.take((size_t)NB * p->feat * 4);
    p->emb_off = bp.take((size_t)NB * emb_dim * 4);
    p->h1_off = bp.take((size_t)NB * 128 * 4);
    p->h2_off = bp.take((size_t)NB * 128 * 4);
    p->pred_off = bp.take((size_t)NB * 2 * emb_dim * 4);
    if (p->train) {
        p->idx_off = bp.take((size_t)NB * p->H1 * p->W1 * 64);
        size_t maxact = (size_t)NB * p->H1 * p->W1 * 64;
        for (auto& B : p->blocks) {
            B.c1.z_off = bp.take((size_t)NB * B.c1.Hout * B.c1.Wout * B.c1.Co * 2);
            B.c2.z_off = bp.take((size_t)NB * B.c2.Hout * B.c2.Wout * B.c2.Co * 2);
            if (bottleneck) B.c3.z_off = bp.take((size_t)NB * B.c3.Hout * B.c3.Wout * B.c3.Co * 2);
            if (B.ds) B.cd.z_off = bp.take((size_t)NB * B.cd.Hout * B.cd.Wout * B.cd.Co * 2);
            size_t e = (size_t)NB * B.c1.Hout * B.c1.Wout * B.c1.Co;
            maxact = e > maxact ? e : maxact;
            if (bottleneck) {      // gradients w.r.t. the block input / output and both inner activations
                e = (size_t)NB * B.c1.Hin * B.c1.Win * B.c1.Ci; maxact = e > maxact ? e : maxact;
                e = (size_t)NB * B.c2.Hout * B.c2.Wout * B.c2.Co; maxact = e > maxact ? e : maxact;
                e = (size_t)NB * B.c3.Hout * B.c3.Wout * B.c3.Co; maxact = e > maxact ? e : maxact;
            }
        }
        for (int s = 0; s < 4; ++s) {
            StageInfo& S = p->stages[s];
            for (int k = 0; k < 2; ++k) {
                S.dz2_off[k] = bp.take(padded_elems(NB, S.H, S.W, S.C, 1) * 2);
                S.dz1_off[k] = bp.take(padded_elems(NB, S.H, S.W, S.C, 1) * 2);
            }
            S.dzd_off = bp.take(padded_elems(NB, S.H, S.W, S.C, 1) * 2);
        }
        if (bottleneck) {      // per-stage dz buffers sized for the largest conv output of the stage's blocks
            for (int s = 0; s < 4; ++s) {
                size_t m1 = 0, m2 = 0, m3 = 0;
                for (auto& B : p->blocks) {
                    if (B.stage != s) continue;
                    size_t e1 = padded_elems(NB, B.c1.Hout, B.c1.Wout, B.c1.Co, 1), e2 = padded_elems(NB, B.c2.Hout, B.c2.Wout, B.c2.Co, 1),
                           e3 = padded_elems(NB, B.c3.Hout, B.c3.Wout, B.c3.Co, 1);
                    m1 = e1 > m1 ? e1 : m1; m2 = e2 > m2 ? e2 : m2; m3 = e3 > m3 ? e3 : m3;
                }
                StageInfo& S = p->stages[s];
                S.dz1_off[0] = S.dz1_off[1] = bp.take(m1 * 2);
                S.dz2_off[0] = S.dz2_off[1] = bp.take(m2 * 2);
                S.dz3_off = bp.take(m3 * 2);
            }
            for (int i = 0; i < 2; ++i) p->T_off[i] = bp.take(maxact * 2);
        }
        // grouped weight gradients: every eligible 3x3 stride-1 conv keeps its own dz until the
        // stage's grouped launch; the stage's slab holds every problem's splits at once
        p->wg_group = vpd_switches().wg_group;
        // data parallel (VPD_TRAIN_EARLY_BUCKET0): layer4's weight gradients get a launch of their own at the end of layer4's
        // backward, so that bucket 0 -- fc + layer4, 61 % of the gradient bytes -- is handed to the reducer there instead of
        // together with bucket 1 behind layer3 (single GPU: the merged launch fills the chip, +0.5 % on the step)
        p->wg_merge34 = vpd_switches().wg_merge && !p->early_bucket0;
        if (p->wg_group) {
            // slabs of one LAUNCH live side by side: with wg_merge34 the stages 2 and 3 (layer3, layer4) share a launch
            size_t stage_slab[4] = {0, 0, 0, 0};
            for (auto& B : p->blocks) {
                std::vector<ConvInfo*> cvs = {&B.c1, &B.c2};
                if (bottleneck) cvs.push_back(&B.c3);
                if (B.ds) cvs.push_back(&B.cd);
                for (ConvInfo* cv : cvs) {
                    if (cv->slab_off < 0) continue;
                    if (cv->k == 1) {
                        // 1x1 convolutions: tasks of the stage's persistent launch when it takes them (Co % 128 == 0 ...).
                        // Bottleneck students: ResNet-50 step 9.32 -> 8.74 ms (36 launches of the atomics kernel at 47 us each
                        // become tasks; no atomics left).  BasicBlock students keep their three down-sampling convs on
                        // launches of their own (same-box: 3.945 vs 3.951 ms grouped).
                        if (!bottleneck || !vpd_wgrad128_eligible(grouped_wgrad_params(*cv, NB, nullptr, nullptr))) continue;
                    } else if (cv->k != 3) {
                        continue;
                    } else if (cv->stride != 1) {
                        // stride-2 3x3: launches of their own (inside the stage's launch the three stride-2 problems cost 86 us
                        // per step against 78 us: their 55-66 KB per chunk leave room for a two-stage ring only)
                        continue;
                    }
                    cv->dz_own_off = bp.take(padded_elems(NB, cv->Hout, cv->Wout, cv->Co, 1) * 2);
                    const int grp = (p->wg_merge34 && B.stage == 3) ? 2 : B.stage;
                    cv->gslab_off = (long long)stage_slab[grp];
                    stage_slab[grp] += vpd_wgrad_group_slab_floats(NB * cv->Hout * cv->Wout, cv->Co, cv->Kc, cv->k == 1 ? 1 : 9);
                }
            }
            size_t mx = 16;
            for (int s2 = 0; s2 < 4; ++s2) mx = stage_slab[s2] > mx ? stage_slab[s2] : mx;
            p->gslab_off = bp.take(mx * 4);
            for (int s2 = 0; s2 < 8; ++s2) p->wg2_tbl_off[s2] = bp.take(vpd_wgrad128_table_bytes());
        }
        p->relu_bits = vpd_switches().relu_bits;
        if (p->relu_bits)
            for (auto& B : p->blocks) {
                const ConvInfo& last = bottleneck ? B.c3 : B.c2;      // the conv whose BatchNorm feeds the block-output ReLU
                B.mask_off = bp.take((size_t)NB * last.Hout * last.Wout * last.Co / 8 + 16);
            }
        // BasicBlock students: every block.  Bottleneck students: layer3 / layer4 only, the BatchNorms of conv1 / conv2 -- there the
        // backward launches sit on the grid barrier's latency chain (14-16 us for 2-8 MB) like a BasicBlock student's; in layer1 /
        // layer2 the tensors are 4-16x larger, the launches run at the memory system's rate, and the second read of z in the data
        // gradients' epilogues costs what the shorter BatchNorm launch saves (ResNet-50 8.73 -> 8.76 ms with all stages, rounds 2 / 4)
        p->dgrad_sums = p->relu_bits && p->fused_bn && vpd_switches().dgrad_sums;
        if (p->dgrad_sums)
            for (auto& B : p->blocks) {
                if (bottleneck && B.stage < 2) continue;
                B.mask1_off = bp.take((size_t)NB * B.c1.Hout * B.c1.Wout * B.c1.Co / 8 + 16);
                if (bottleneck) B.mask2_off = bp.take((size_t)NB * B.c2.Hout * B.c2.Wout * B.c2.Co / 8 + 16);
            }
        for (int i = 0; i < 3; ++i) p->G_off[i] = bp.take(maxact * 2);
        p->slab_off = bp.take((size_t)(p->slab_elems > 0 ? p->slab_elems : 1) * 4);
        p->g0_off = bp.take((size_t)NB * p->H0 * p->W0 * 64 * 2);
        p->dz0_off = bp.take((size_t)NB * p->H0 * p->W0 * 64 * 2);
        p->dpred_off = bp.take((size_t)NB * 2 * emb_dim * 4);
        p->dh2_off = bp.take((size_t)NB * 128 * 4);
        p->dh1_off = bp.take((size_t)NB * 128 * 4);
        p->demb_off = bp.take((size_t)NB * emb_dim * 4);
        p->dpooled_off = bp.take((size_t)NB * p->feat * 4);
    }
    p->ws_bytes = bp.cur;
    *out = p;
    return 0;
}

extern "C" void vpd_plan_destroy(vpd_plan_t* p) {
    if (!p) return;
    for (auto& g : p->graphs) {
        (void)hipGraphExecDestroy(g.e);
        (void)hipGraphDestroy(g.g);
    }
    for (auto& t : p->timed) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    for (auto e : p->ev_pool) (void)hipEventDestroy(e);
    for (int i = 0; i < 8; ++i)
        if (p->wg2_cache[i]) vpd_wgrad128_cache_free(p->wg2_cache[i]);
    delete p;
}

extern "C" int vpd_plan_num_tensors(const vpd_plan_t* p) { return (int)p->tensors.size(); }
extern "C" int vpd_plan_tensor_info(const vpd_plan_t* p, int i, int* kind, int* is_decoder, long long* offset,
                                    long long* numel, int* ndim, int dims[4]) {
    if (i < 0 || i >= (int)p->tensors.size()) return fail("tensor index out of range");
    const TensorRow& r = p->tensors[i];
    *kind = r.kind; *is_decoder = r.is_dec; *offset = r.off; *numel = r.numel; *ndim = r.ndim;
    for (int k = 0; k < 4; ++k) dims[k] = r.dims[k];
    return 0;
}
extern "C" long long vpd_plan_param_numel(const vpd_plan_t* p) { return p->nparam_padded; }
extern "C" int vpd_plan_num_bn(const vpd_plan_t* p) { return (int)p->bns.size(); }
extern "C" int vpd_plan_bn_info(const vpd_plan_t* p, int i, int* channels, long long* rm_off, long long* rv_off) {
    if (i < 0 || i >= (int)p->bns.size()) return fail("bn index out of range");
    *channels = p->bns[i]->C; *rm_off = p->bns[i]->rm_off; *rv_off = p->bns[i]->rv_off;
    return 0;
}
extern "C" long long vpd_plan_bn_numel(const vpd_plan_t* p) { return p->nbn; }
extern "C" int vpd_plan_num_buckets(const vpd_plan_t*) { return 4; }
extern "C" int vpd_plan_bucket_range(const vpd_plan_t* p, int b, long long* offset, long long* numel) {
    if (b < 0 || b >= 4) return fail("bucket index out of range");
    *offset = p->bucket_off[b]; *numel = p->bucket_numel[b];
    return 0;
}
extern "C" int vpd_plan_bucket_scratch_range(const vpd_plan_t* p, int b, long long* ws_byte_offset, long long* numel) {
    if (b < 0 || b >= 4) return fail("bucket index out of range");
    if (!p->train) return fail("plan was created with train=0");
    *ws_byte_offset = (long long)p->wg_off + p->bucket_wg_off[b] * 4;
    *numel = p->bucket_wg_numel[b];
    return 0;
}
extern "C" size_t vpd_plan_workspace_bytes(const vpd_plan_t* p) { return p->ws_bytes; }

extern "C" int vpd_plan_init_workspace(vpd_plan_t* p, void* ws, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    HCHECK(hipMemsetAsync(ws, 0, p->ws_bytes, s));
    HCHECK(hipMemcpyAsync(w + p->desc_off, p->descs.data(), p->descs.size() * sizeof(PackDesc), hipMemcpyHostToDevice, s));
    HCHECK(hipMemcpyAsync(w + p->bmap_pack_off, p->bmap_pack.data(), p->bmap_pack.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HCHECK(hipMemcpyAsync(w + p->bmap_adam_off, p->bmap_adam.data(), p->bmap_adam.size() * sizeof(int), hipMemcpyHostToDevice, s));
    for (int i = 0; i < 4; ++i)
        if (!p->bmap_unpack[i].empty())
            HCHECK(hipMemcpyAsync(w + p->bmap_unpack_off[i], p->bmap_unpack[i].data(),
                                  p->bmap_unpack[i].size() * sizeof(int), hipMemcpyHostToDevice, s));
    HCHECK(hipStreamSynchronize(s));   // host vectors may be re-read only now; one-time setup
    p->bound_ws = ws;
    return 0;
}

int check_call(const vpd_plan* p, const void* ws, int n, int min_n) {
    if (!p || !ws) return fail("null plan / workspace");
    if (p->bound_ws != ws) return fail("workspace not initialised with vpd_plan_init_workspace");
    if (n < min_n || n > p->max_batch) return fail(min_n ? "batch size outside 1..max_batch" : "batch size outside 0..max_batch");
    return 0;
}

extern "C" int vpd_augment_crops(const unsigned char* rgb_u8, const unsigned char* flow_u8, const unsigned char* mask_u8,
                                 const float* noise, const vpd_aug_params* params, int n, int height, int width,
                                 int out_dim, const float* mean_std6, float noise_sd, float* out_nchw, float* scratch,
                                 void* stream) {
    if (!rgb_u8 || !params || !mean_std6 || !out_nchw || !scratch) return fail("null argument");
    if (n < 1 || height < 1 || width < 1 || out_dim < 1) return fail("bad shape");
    LCHECK(vpd_launch_augment(rgb_u8, flow_u8, mask_u8, noise, params, n, height, width, out_dim, mean_std6, noise_sd,
                              out_nchw, nullptr, 0, 0, 0, scratch, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_plan_stage_crops(vpd_plan_t* p, const unsigned char* rgb_u8, const unsigned char* flow_u8,
                                    const unsigned char* mask_u8, const float* noise, const vpd_aug_params* params,
                                    int n, int height, int width, const float* mean_std6, float noise_sd,
                                    float* scratch, void* workspace, void* stream) {
    if (n > 65535) return fail("more than 65535 crops per staging call");      // (aug_apply_kernel: one grid row per crop)
    if (check_call(p, workspace, n)) return -1;
    if (!rgb_u8 || !params || !mean_std6 || !scratch) return fail("null argument");
    if (p->H != p->W) return fail("the input pipeline resizes to a square img_dim");
    if ((p->c_in == 5) != (flow_u8 != nullptr)) return fail("flow_u8 must be given exactly when the plan has 5 input channels");
    char* ws = (char*)workspace;
    LCHECK(vpd_launch_augment(rgb_u8, flow_u8, mask_u8, noise, params, n, height, width, p->H, mean_std6, noise_sd,
                              nullptr, reinterpret_cast<bf16_t*>(ws + p->xin_off), p->xHp, p->xWp, 3, scratch,
                              (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_plan_stage_views(vpd_plan_t* p, const unsigned char* rgb_u8, const unsigned char* flow_u8, int n_frames,
                                    int k_views, int height, int width, const float* mean_std6, void* workspace,
                                    void* stream) {
    if (n_frames < 0 || (k_views != 1 && k_views != 2)) return fail("k_views must be 1 (frame) or 2 (frame, h-flip)");
    // (aug_views_kernel: one grid row per view; a launch fails opaquely beyond gridDim.y = 65535)
    if ((long)n_frames * k_views > 65535) return fail("n_frames * k_views exceeds 65535 views per staging call");
    if (check_call(p, workspace, n_frames * k_views)) return -1;
    if (!rgb_u8 || !mean_std6) return fail("null argument");
    if (height != p->H || width != p->W) return fail("inference views are not resized: the frames must have the plan's size");
    if (width % 4) return fail("width must be a multiple of 4");
    if ((p->c_in == 5) != (flow_u8 != nullptr)) return fail("flow_u8 must be given exactly when the plan has 5 input channels");
    if (p->c_in != 3 && p->c_in != 5) return fail("inference views: 3 or 5 input channels");
    if (n_frames == 0) return 0;
    char* ws = (char*)workspace;
    LCHECK(vpd_launch_views(rgb_u8, flow_u8, n_frames, k_views, height, width, mean_std6,
                            reinterpret_cast<bf16_t*>(ws + p->xin_off), p->xHp, p->xWp, 3, (hipStream_t)stream));
    return 0;
}

// shared argument checks of the two jittered-view entry points (nothing is launched when one fails)
static int check_jitter_views(const unsigned char* rgb_u8, const vpd_aug_params* params, int n_frames, int jitter, int height,
                              int width, const float* mean_std6, const float* scratch) {
    if (n_frames < 0 || jitter < 0) return fail("n_frames and jitter must not be negative");
    if (!rgb_u8 || !mean_std6) return fail("null argument");
    if (jitter > 0 && (!params || !scratch)) return fail("jittered views need params and scratch");
    if (height < 1 || width < 1) return fail("bad shape");
    if (width % 4) return fail("width must be a multiple of 4");
    return 0;
}

extern "C" int vpd_augment_views(const unsigned char* rgb_u8, const unsigned char* flow_u8, const vpd_aug_params* params,
                                 int n_frames, int jitter, int flip, int height, int width, const float* mean_std6,
                                 float* out_nchw, float* scratch, void* stream) {
    if (check_jitter_views(rgb_u8, params, n_frames, jitter, height, width, mean_std6, scratch)) return -1;
    if (!out_nchw) return fail("null argument");
    // (one grid row per frame / per parameter row: both stay below the view count)
    if ((long)n_frames * (1 + jitter) * (flip ? 2 : 1) > 65535) return fail("n_frames * views exceeds 65535 views per call");
    if (n_frames == 0) return 0;
    LCHECK(vpd_launch_views_jitter(rgb_u8, flow_u8, params, n_frames, jitter, flip, height, width, mean_std6, out_nchw,
                                   nullptr, 0, 0, 0, scratch, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_plan_stage_views_jitter(vpd_plan_t* p, const unsigned char* rgb_u8, const unsigned char* flow_u8,
                                           const vpd_aug_params* params, int n_frames, int jitter, int flip, int height,
                                           int width, const float* mean_std6, float* scratch, void* workspace,
                                           void* stream) {
    if (check_jitter_views(rgb_u8, params, n_frames, jitter, height, width, mean_std6, scratch)) return -1;
    const long views = (long)n_frames * (1 + jitter) * (flip ? 2 : 1);
    if (views > 65535) return fail("n_frames * views exceeds 65535 views per staging call");
    if (check_call(p, workspace, (int)views)) return -1;
    if (height != p->H || width != p->W) return fail("inference views are not resized: the frames must have the plan's size");
    if ((p->c_in == 5) != (flow_u8 != nullptr)) return fail("flow_u8 must be given exactly when the plan has 5 input channels");
    if (p->c_in != 3 && p->c_in != 5) return fail("inference views: 3 or 5 input channels");
    if (n_frames == 0) return 0;
    char* ws = (char*)workspace;
    LCHECK(vpd_launch_views_jitter(rgb_u8, flow_u8, params, n_frames, jitter, flip, height, width, mean_std6, nullptr,
                                   reinterpret_cast<bf16_t*>(ws + p->xin_off), p->xHp, p->xWp, 3, scratch,
                                   (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_plan_set_lazy_grads(vpd_plan_t* p, int on) {
    if (!p) return fail("null plan");
    p->lazy_next = on != 0;
    return 0;
}
extern "C" int vpd_plan_set_bn_frozen(vpd_plan_t* p, int on) {
    if (!p) return fail("null plan");
    if (!p->train) return fail("vpd_plan_set_bn_frozen: plan was created with train=0 (an inference plan folds the running statistics already)");
    p->bn_frozen = on != 0;
    return 0;
}
extern "C" int vpd_plan_set_param_grads(vpd_plan_t* p, int on) {
    if (!p) return fail("null plan");
    if (!p->train) return fail("vpd_plan_set_param_grads: plan was created with train=0");
    p->param_grads = on != 0;
    return 0;
}
extern "C" int vpd_plan_grads_pending(const vpd_plan_t* p) { return p && p->grads_in_scratch ? 1 : 0; }
extern "C" int vpd_plan_materialize_grads(vpd_plan_t* p, float* grads, void* workspace, void* stream) {
    if (!p || !grads || !workspace) return fail("null argument");
    if (p->bound_ws != workspace) return fail("workspace not initialised with vpd_plan_init_workspace");
    if (!p->grads_in_scratch) return 0;
    for (int b = 0; b < 4; ++b) {
        const int nb = (int)p->bmap_unpack[b].size() / 2;
        const int skip = b == 3 ? p->nstem_unpack_blocks : 0;      // the stem was unpacked by the backward itself
        if (nb > skip)
            LCHECK(vpd_launch_unpack_grads(plan_descs(p, workspace), (int)p->descs.size(), plan_bmap_unpack(p, workspace, b) + 2 * skip,
                                           nb - skip, plan_wg(p, workspace), grads, (hipStream_t)stream));
    }
    p->grads_in_scratch = false;
    return 0;
}

extern "C" int vpd_plan_sync_errors(vpd_plan_t* p, void* workspace, void* stream, unsigned* count_out) {
    if (!p || !workspace || !count_out) return fail("null argument");
    if (p->bound_ws != workspace) return fail("workspace not initialised with vpd_plan_init_workspace");
    hipStream_t s = (hipStream_t)stream;
    unsigned v = 0;
    HCHECK(hipMemcpyAsync(&v, (char*)workspace + p->syncerr_off, sizeof v, hipMemcpyDeviceToHost, s));
    HCHECK(hipStreamSynchronize(s));
    *count_out = v;
    return 0;
}

extern "C" int vpd_plan_set_timing(vpd_plan_t* p, int enable) {
    if (!p) return fail("null plan");
    p->timing = enable != 0;
    return 0;
}

// Sums (and clears) the recorded launches: out[4*cls + {0,1,2}] = {launches, milliseconds, flops}
extern "C" int vpd_plan_read_timing(vpd_plan_t* p, double* out, int nclasses) {
    if (!p || !out || nclasses < 8) return fail("bad argument");
    for (int i = 0; i < 3 * nclasses; ++i) out[i] = 0.0;
    for (auto& t : p->timed) {
        HCHECK(hipEventSynchronize(t.b));
        float ms = 0.f;
        HCHECK(hipEventElapsedTime(&ms, t.a, t.b));
        const int cls = t.cls;
        p->ev_pool.push_back(t.a); p->ev_pool.push_back(t.b);
        if (cls < 0 || cls >= nclasses) continue;
        out[3 * cls + 0] += 1.0; out[3 * cls + 1] += ms; out[3 * cls + 2] += t.flops;
    }
    p->timed.clear();
    return 0;
}

