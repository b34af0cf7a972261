// Private to plan.hip (the plan: topology, workspace layout, tables, query / setter entry points), step.hip (the passes that
// launch on it), optim_step.hip (the optimizer step's host side) and ops.hip (the single-operator entry points).  Not part of
// the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "../../include/vpd_hip.h"
#include "common.h"
#include "kernels.h"

int fail(const char* what, hipError_t e = hipSuccess);     // sets vpd_last_error, returns -1
#define HCHECK(expr)                                   \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) return fail(#expr, _e);  \
    } while (0)
#define LCHECK(expr)                                   \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) return fail(#expr, _e);  \
    } while (0)

constexpr float kBnEps = 1e-5f;
constexpr float kBnMomentum = 0.1f;

struct BnInfo {
    int C = 0;
    long long w_off = 0, b_off = 0;      // gamma / beta in the flat param buffer
    long long rm_off = 0, rv_off = 0;    // in the running-stat buffer
    size_t fl_off = 0;                   // float scratch in ws: mean,rstd,scale,shift,coef[3],escale,eshift (9C)
    size_t rows_off = 0;                 // fused passes: this BatchNorm's own accumulator rows [VPD_FUSED_ROWS][2][C] doubles
    size_t sync_off = 0;                 // ... and the grid-barrier words of its fused backward launch
    long long sink_off = 0;              // data-only backward: this BatchNorm's [2][C] floats (dgamma, dbeta) in the weight-gradient scratch
};
struct ConvInfo {
    int Ci = 0, Co = 0, k = 0, stride = 1, pad = 0;
    int Hin = 0, Win = 0, Hout = 0, Wout = 0;
    bool stem = false;
    int Kc = 0, ntaps = 0;
    long long w_off = 0;                 // OIHW offset in flat params/grads
    long long fwd_off = 0, dgr_off = -1; // bf16 element offsets in the weight arena
    long long wg_off = 0;                // fp32 element offset in the wgrad scratch
    long long slab_off = -1;             // fp32 element offset of this conv's split slabs (3x3 s1 convs) or -1
    size_t dz_own_off = 0;               // grouped weight gradients: this conv's own padded dz buffer (kept until the stage's launch)
    long long gslab_off = 0;             // ... and its slab inside the stage's grouped slab (floats)
    BnInfo bn;
    size_t z_off = 0;                    // dense bf16 conv output (train)
};
struct BlockInfo {
    ConvInfo c1, c2, c3, cd;             // c3: Bottleneck's closing 1x1 conv (BasicBlock: unused)
    bool ds = false;
    int stage = 0;
    size_t a1_off = 0, a2_off = 0, out_off = 0;      // padded bf16 activations (a2: Bottleneck only)
    size_t mask_off = 0;                             // train, BasicBlock: [M][C/8] ReLU mask bits of the block output
    size_t mask1_off = 0;                            // train with dgrad_sums: ReLU mask bits of a1 (0: none)
    size_t mask2_off = 0;                            // ... of a2 (Bottleneck students, layer3 / layer4)
};
struct StageInfo {
    int H = 0, W = 0, C = 0;
    size_t dz2_off[2] = {0, 0}, dz1_off[2] = {0, 0}, dzd_off = 0, idn_off = 0;   // dz buffers ping-pong by block parity
    size_t dz3_off = 0;                  // Bottleneck: dz of the closing 1x1 conv
};
struct TensorRow {
    int kind, is_dec;
    long long off, numel;
    int ndim, dims[4];
};
struct LinInfo {
    int in = 0, out = 0;
    long long w_off = 0, b_off = 0;
};

struct vpd_plan {
    int c_in, H, W, D, motion, max_batch, train;
    int bottleneck = 0, base_width = 64, feat = 512;     // Bottleneck archs: expansion 4, feat = 2048
    std::vector<int> layers;
    ConvInfo stem;
    std::vector<BlockInfo> blocks;
    StageInfo stages[4];
    LinInfo fc, dec[3];
    std::vector<TensorRow> tensors;
    std::vector<BnInfo*> bns;
    long long nparam = 0, nparam_padded = 0, nbn = 0;
    long long arena_elems = 0, wg_elems = 0, slab_elems = 0;
    // gradient buckets (flat-buffer ranges) -- bucket 0 = layer4+fc+decoder ... bucket 3 = stem+layer1
    long long bucket_off[4], bucket_numel[4];
    // ... and the part of the weight-gradient scratch (fp32 elements from wg_off) that holds bucket b's conv gradients, the
    // stem excluded (its row-tap packing is always undone into the flat buffer): vpd_plan_bucket_scratch_range
    long long bucket_wg_off[4], bucket_wg_numel[4];
    // workspace offsets (bytes)
    size_t ws_bytes = 0;
    size_t xin_off = 0, arena_off = 0, wg_off = 0, partial_off = 0, z0_off = 0, p0_off = 0, idx_off = 0;
    size_t g0_off = 0, dz0_off = 0, G_off[3] = {0, 0, 0}, T_off[2] = {0, 0}, slab_off = 0;
    size_t pooled_off = 0, emb_off = 0, h1_off = 0, h2_off = 0, pred_off = 0;
    size_t dpred_off = 0, dh2_off = 0, dh1_off = 0, demb_off = 0, dpooled_off = 0;
    size_t desc_off = 0, bmap_pack_off = 0, bmap_unpack_off[4] = {0, 0, 0, 0};
    int xHp = 0, xWp = 0;
    int H0 = 0, W0 = 0, H1 = 0, W1 = 0;   // stem conv output, pooled output
    // descriptor tables (host copies, uploaded by init_workspace)
    std::vector<PackDesc> descs;
    std::vector<int> bmap_pack;
    std::vector<int> bmap_adam;            // fused AdamW + repack: conv tiles, the stem (one block), plain ranges
    size_t bmap_adam_off = 0;
    int nstem_pack_blocks = 0;             // leading entries of bmap_pack that belong to the stem
    std::vector<int> bmap_unpack[4];
    size_t partial_bytes = 0;
    // captured eval graphs keyed by batch size
    struct Graph { int n; hipGraph_t g; hipGraphExec_t e; };
    std::vector<Graph> graphs;
    void* bound_ws = nullptr;
    bool fused_bn = true;       // one launch per BatchNorm and direction (VPD_FUSED_BN=0: finalize / reduce / apply launches)
    size_t fused_off = 0, fused_bytes = 0;      // rows + barrier words of every BatchNorm: zeroed at the start of each pass
    size_t syncerr_off = 0;                     // sticky counter of grid-barrier time-outs (zeroed by init_workspace only)
    bool wg_group = true;       // per-stage grouped weight gradients (VPD_WG_GROUP=0: one launch per conv)
    size_t gslab_off = 0;       // grouped slab region (bytes offset), sized for the largest launch group
    // lazy gradients (vpd_plan_set_lazy_grads): the next vpd_backward leaves the conv weight gradients in the scratch
    // (only the stem's are unpacked), vpd_plan_adamw_step reads them there; vpd_plan_materialize_grads unpacks on demand
    bool dgrad_sums = true;     // BatchNorm-backward sums in the producing data gradient's epilogue (VPD_DGRAD_SUMS=0: in the BatchNorm launch)
    bool relu_bits = true;      // block-output ReLU masks as bit maps (VPD_RELU_BITS=0: masks from the stored activation, g written back)
    bool lazy_next = false, grads_in_scratch = false;
    // frozen BatchNorm (vpd_plan_set_bn_frozen): vpd_forward_train normalises with the running statistics and leaves them alone.
    // fwd_bn_frozen is the mode the last forward RAN in: the backward of that graph reads it, not the current flag
    bool bn_frozen = false, fwd_bn_frozen = false;
    bool param_grads = true;    // vpd_plan_set_param_grads(0): vpd_backward_ext computes data gradients only and leaves `grads` alone
    bool fwd_had_x = false;     // the last vpd_forward_train took an fp32 x (vpd_backward_ext: an input gradient exists only then)
    int nstem_unpack_blocks = 0;           // leading entries of bmap_unpack[3] that belong to the stem
    bool wg_merge34 = true;     // layer4's grouped weight gradients wait for layer3's and share its launch (VPD_WG_MERGE=0, or the
                                // data-parallel creation flag VPD_TRAIN_EARLY_BUCKET0: per stage)
    bool early_bucket0 = false;
    float loss_scale = 1.f;     // vpd_plan_set_loss_scale: fp16 training (the reference's GradScaler, models/util.py:55-57)
    const vpd_scale_state* scale_state = nullptr;      // vpd_plan_set_scale_state: the scale is read on the device instead (dynamic loss scaling)
    size_t wg2_tbl_off[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // task tables of the persistent weight-gradient launches (two per stage)
    void* wg2_cache[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // optional per-kernel-class timing (bench.py roofline): HIP events around every conv launch
    bool timing = false;
    struct TimedLaunch { int cls; double flops; hipEvent_t a, b; };
    std::vector<TimedLaunch> timed;
    std::vector<hipEvent_t> ev_pool;
};

// the tables and buffers of a plan inside its workspace `ws` (uploaded by vpd_plan_init_workspace)
template <class T>
inline T* plan_at(void* ws, size_t off) { return reinterpret_cast<T*>((char*)ws + off); }
inline const PackDesc* plan_descs(const vpd_plan* p, void* ws) { return plan_at<const PackDesc>(ws, p->desc_off); }
inline const int* plan_bmap_pack(const vpd_plan* p, void* ws) { return plan_at<const int>(ws, p->bmap_pack_off); }
inline const int* plan_bmap_adam(const vpd_plan* p, void* ws) { return plan_at<const int>(ws, p->bmap_adam_off); }
inline const int* plan_bmap_unpack(const vpd_plan* p, void* ws, int bucket) { return plan_at<const int>(ws, p->bmap_unpack_off[bucket]); }
inline bf16_t* plan_arena(const vpd_plan* p, void* ws) { return plan_at<bf16_t>(ws, p->arena_off); }
inline float* plan_wg(const vpd_plan* p, void* ws) { return plan_at<float>(ws, p->wg_off); }      // the weight-gradient scratch

// min_n = 0 for the train-step entry points: a data-parallel rank whose shard of a ragged last batch is empty still
// takes part in the step (zero loss, zero gradients, bucket events recorded) so that the collective stays matched
int check_call(const vpd_plan* p, const void* ws, int n, int min_n = 1);

// plan.hip: the pack descriptors and block maps of a plan, and -- one construction -- of the operator entry points (ops.hip)
void set_pack_geom(ConvInfo& c, int Ci, int Co, int k, bool stem);
int push_pack_desc(std::vector<PackDesc>& descs, std::vector<int>& bmap_pack, std::vector<int>& bmap_unpack, const ConvInfo& c);
void build_adam_map(std::vector<PackDesc>& descs, const std::vector<int>& bmap_pack, int stem_id, long long nparam_padded,
                    std::vector<int>& bmap_adam, int& nstem_pack_blocks);

// optim_step.hip: AdamW's parameter groups -- what vpd_adam_groups_init and vpd_op_adamw_pack_groups (ops.hip) share.  Each returns 0
// or fail(): the host arrays of a segment table (layout: kernels.h); no boundary strictly inside a conv weight of `descs`; the
// table built and copied to `table`, the stream synchronised; the hyper-parameters of a grouped step
int adam_groups_check(const long long* seg_begin, const int* seg_group, int nseg, long long numel, int ngroups);
int adam_groups_check_convs(const std::vector<PackDesc>& descs, const long long* seg_begin, int nseg);
int adam_groups_upload(void* table, const long long* seg_begin, const int* seg_group, int nseg, int ngroups, hipStream_t s);
int adam_group_args_check(const double* lr, const double* weight_decay, int ngroups, int step, const vpd_scale_state* state);

inline TapSet conv_taps_fwd(const ConvInfo& c) {
    TapSet t;
    if (c.stem) {
        // one tap per kernel row; the 7 column taps x 8 channels are 56 (of 64) contiguous values
        t.nr = c.k; t.nc = 1; t.dy0 = 0; t.dys = 1; t.dx0 = 0; t.dxs = 0; t.w0 = 0; t.wrs = 1; t.wcs = 0;
    } else {
        // input tensors carry a 1-pixel border: padded coord = y*stride + r - pad + 1
        t.nr = c.k; t.nc = c.k; t.dy0 = 1 - c.pad; t.dys = 1; t.dx0 = 1 - c.pad; t.dxs = 1;
        t.w0 = 0; t.wrs = c.k; t.wcs = 1;
    }
    return t;
}

// The weight-gradient problem of a (non-stem) conv over n images: dz and x padded by 1; dw / slab are the caller's.
inline WgradParams wgrad_params(const ConvInfo& cv, int n, const bf16_t* dz, const bf16_t* x) {
    WgradParams q;
    memset(&q, 0, sizeof q);
    q.dz = dz; q.dzHp = cv.Hout + 2; q.dzWp = cv.Wout + 2; q.dzC = cv.Co; q.dzpad = 1;
    q.x = x; q.xHp = cv.Hin + 2; q.xWp = cv.Win + 2; q.xC = cv.Ci;
    q.N = n; q.Hs = cv.Hout; q.Ws = cv.Wout; q.istr = cv.stride; q.Kc = cv.Kc; q.Co = cv.Co;
    q.M = n * cv.Hout * cv.Wout;
    q.taps = conv_taps_fwd(cv);
    return q;
}
// ... as a task of a stage's grouped launch: a 1x1 conv with < 128 output but >= 128 input channels (layer1's 256 -> 64) joins
// with its operands swapped, its result stored transposed (WgradParams::transposed).  The plan sizes the grouped slabs with it.
inline WgradParams grouped_wgrad_params(const ConvInfo& cv, int n, const bf16_t* dz, const bf16_t* x) {
    WgradParams q = wgrad_params(cv, n, dz, x);
    vpd_wgrad_swap_1x1(q);
    return q;
}
