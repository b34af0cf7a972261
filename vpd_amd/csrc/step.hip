// The passes on a plan (plan.hip): eval forward, train forward + loss, backward, the weight re-pack and the captured eval
// graphs -- the launch sequences behind the step entry points of include/vpd_hip.h.
//
// How to read it: every launcher takes a small request struct filled by name at the call site (ConvFwd, ConvDgrad, BnFwd, BnBwd); a
// request that asks for something its launch cannot do is refused with hipErrorInvalidValue, never run in a weaker form.  What a
// block's passes do -- which launches are merged, recomputed or masked by a bit map -- is decided once per pass by block_route;
// the forward and the backward read the same BlockRoute.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "plan.h"

// ---------------------------------------------------------------------------
namespace {

constexpr int kStemPad = 3, kStemCp = 8;      // the packed input: border of 3 pixels, channels padded to 8
constexpr int kDzPad = 1;                     // every dz has a border of 1: the weight and data gradients read it through 3x3 windows
constexpr int kRelu = 1, kNoRelu = 0;

// what a conv launch's epilogue does to its result: scale * z + shift (a folded BatchNorm), + res (padded by 1), ReLU
struct ConvEpilogue { const float* scale = nullptr; const float* shift = nullptr; const bf16_t* res = nullptr; int relu = kNoRelu; };

struct Ctx {
    vpd_plan* p;
    char* ws;
    hipStream_t s;
    const float* params;
    int n;
    bool train = false;              // a pass of a training graph (vpd_forward_train, the backward); false: the eval forward
    bool frozen = false;             // BatchNorm on running statistics: the plan's flag in a forward, the forward's recorded mode in a backward
    bool data_only = false;          // backward without parameter gradients (vpd_plan_set_param_grads): dgamma / dbeta go to the sink
    bf16_t* b16(size_t off) const { return reinterpret_cast<bf16_t*>(ws + off); }
    float* f32(size_t off) const { return reinterpret_cast<float*>(ws + off); }
    unsigned char* u8(size_t off) const { return reinterpret_cast<unsigned char*>(ws + off); }
    // a conv's dz: its own buffer when its weight gradient joins the stage's grouped launch (dz_own_off is set only then),
    // else the stage's shared buffer `shared_off`
    bf16_t* dz(const ConvInfo& cv, size_t shared_off) const { return b16(cv.dz_own_off ? cv.dz_own_off : shared_off); }
    bf16_t* weights(long long arena_elem_off) const { return b16(p->arena_off) + arena_elem_off; }
    unsigned* sync_errors() const { return reinterpret_cast<unsigned*>(ws + p->syncerr_off); }
    double* stat_rows() const { return reinterpret_cast<double*>(ws + p->partial_off); }
    double* bn_rows(const BnInfo& b) const { return reinterpret_cast<double*>(ws + b.rows_off); }
    bool fused(const ConvInfo& cv) const { return p->fused_bn && !cv.stem; }
    float* bn_mean(const BnInfo& b) const { return f32(b.fl_off); }
    float* bn_rstd(const BnInfo& b) const { return f32(b.fl_off) + b.C; }
    float* bn_scale(const BnInfo& b) const { return f32(b.fl_off) + 2 * b.C; }
    float* bn_shift(const BnInfo& b) const { return f32(b.fl_off) + 3 * b.C; }
    float* bn_coef(const BnInfo& b) const { return f32(b.fl_off) + 4 * b.C; }
    float* bn_escale(const BnInfo& b) const { return f32(b.fl_off) + 7 * b.C; }
    float* bn_eshift(const BnInfo& b) const { return f32(b.fl_off) + 8 * b.C; }
    // conv `cv` in eval mode: its BatchNorm on running statistics, folded by vpd_pack_weights, as the conv's epilogue
    ConvEpilogue eval_epilogue(const ConvInfo& cv, int relu, const bf16_t* res = nullptr) const {
        return ConvEpilogue{bn_escale(cv.bn), bn_eshift(cv.bn), res, relu};
    }
    // where a BatchNorm backward stores dgamma / dbeta: the flat gradient buffer, or -- data_only -- the BatchNorm's own slot of
    // the weight-gradient scratch, which no launch of such a pass touches otherwise
    float* bn_dgamma(const BnInfo& b, float* grads) const { return data_only ? f32(p->wg_off) + b.sink_off : grads + b.w_off; }
    float* bn_dbeta(const BnInfo& b, float* grads) const { return data_only ? f32(p->wg_off) + b.sink_off + b.C : grads + b.b_off; }
};

// Timing classes of vpd_plan_set_timing.  bench.py and vpd_plan_read_timing (include/vpd_hip.h) index by these numbers.  A conv
// launch's class follows its kernel class (vpd_conv_kernel_class, conv_igemm.hip: 0..4 as here, 5 the stem kernel, 6 the 256 x 64
// tile) through conv_timing_class; the weight-gradient launches name theirs.
enum TimeClass {
    TC_C64 = 0,             // conv3x3_c64_persistent_kernel<224>; layer1's 64 -> 64 convs stay here when they run on the 256 x 64 tile
    TC_PWS_256x128 = 1,     // conv3x3_pws_kernel<256,128,352>
    TC_PWS_256x64 = 2,      // conv3x3_pws_kernel<256,64,416> and <128,128,288>
    TC_PWS_128x64 = 3,      // conv3x3_pws_kernel<128,64,288>   (1..3 with VPD_PWS=0: conv3x3_ws_kernel, their one-tile-per-block twin)
    TC_GATHER = 4,          // conv_igemm_kernel (gather), the ring GEMM conv1x1_ws_kernel, the streaming 1x1 and Bottleneck-tail kernels
    TC_WGRAD_STAGE = 5,     // conv_wgrad128_persistent_kernel / conv_wgrad_halo_grouped_kernel per stage, and a single stride-1 launch of
                            // conv_wgrad_halo_kernel; without the slab reduce
    TC_WGRAD_CONV = 6,      // the other per-conv weight gradients: stride-2 3x3 on conv_wgrad_halo_kernel (two output tiles, 128 splits:
                            // another regime than class 5), 1x1 on conv_wgrad_kernel, a down-sampling block's pair launch
    TC_STEM = 7,            // conv_stem_persistent_kernel, and the stem's weight-gradient kernel
};
struct TimeScope {
    vpd_plan* p; hipStream_t s; int idx = -1;
    TimeScope(vpd_plan* p_, hipStream_t s_, TimeClass cls, double flops) : p(p_), s(s_) {
        if (!p->timing) return;
        auto get = [&]() {
            hipEvent_t e;
            if (!p->ev_pool.empty()) { e = p->ev_pool.back(); p->ev_pool.pop_back(); }
            else (void)hipEventCreate(&e);
            return e;
        };
        vpd_plan::TimedLaunch t{cls, flops, get(), get()};
        p->timed.push_back(t);
        idx = (int)p->timed.size() - 1;
        vpd_launch_events() = {t.a, t.b};       // the scope's first matrix-kernel launch carries them (common.h)
    }
    ~TimeScope() {
        if (idx < 0) return;
        if (vpd_launch_events().start) {        // nothing was launched through VPD_LAUNCH: bracket the scope instead
            vpd_launch_events().start = nullptr;
            (void)hipEventRecord(p->timed[idx].a, s);
            (void)hipEventRecord(p->timed[idx].b, s);
        }
    }
};
inline double conv_flops(const ConvInfo& cv, int n) {      // algorithmic: real taps and channels
    return 2.0 * n * cv.Hout * cv.Wout * cv.Co * (double)cv.Ci * cv.k * cv.k;
}
inline TimeClass conv_timing_class(int kc, const ConvInfo& cv) {
    if (kc == 5) return TC_STEM;
    if (kc == 6) return cv.Co == 64 && cv.Ci == 64 ? TC_C64 : TC_PWS_256x64;
    return (TimeClass)kc;
}

// ---- forward convolution ----
// second convolution of the same launch (ConvParams::alt_*): a BasicBlock's 1x1 down-sampling branch beside its first 3x3; its
// epilogue has no residual
struct AltConv { const ConvInfo* cv; bf16_t* y; ConvEpilogue ep; };
// input: padded activation `x` (border 1; stem: the packed input); output `y`, padded by ypad.  stats: per-channel statistics of
// a train pass, to the BatchNorm's own rows when fused, else to the shared rows.  pool_y: the eval stem with scale / shift / ReLU /
// max-pool in the conv's epilogue (ConvParams::pool_y) when the stem kernel takes the shape; run_conv_fwd's *pooled then tells the
// caller whether it did (false: plain conv into y, the pooling launch follows)
struct ConvFwd {
    const bf16_t* x = nullptr; bf16_t* y = nullptr; int ypad = 0; bool stats = false;
    ConvEpilogue ep;
    const AltConv* alt = nullptr;
    bf16_t* pool_y = nullptr;
};
// can `cd` ride in `c1`'s launch (forward, and the data gradients of a train pass)?  Same input, same output geometry and channel
// count; a BasicBlock; train mode needs per-BatchNorm statistics rows (the shared rows serve one conv at a time).  VPD_DS_MERGE=0
// keeps the two launches.
bool conv_pair_ok(const Ctx& c, const ConvInfo& c1, const ConvInfo& cd) {
    if (!vpd_switches().ds_merge || c.p->bottleneck || c1.k != 3 || cd.k != 1 || c1.stride != 2 || cd.stride != 2) return false;
    if (c1.Hin != cd.Hin || c1.Win != cd.Win || c1.Hout != cd.Hout || c1.Wout != cd.Wout || c1.Ci != cd.Ci || c1.Co != cd.Co)
        return false;
    return !c.train || (c.fused(c1) && c.fused(cd));
}

hipError_t run_conv_fwd(const Ctx& c, const ConvInfo& cv, const ConvFwd& r, bool* pooled = nullptr) {
    // refused: a pooled output nobody asks about; an alt conv with a residual, or with statistics but no rows of its own
    if ((r.pool_y != nullptr) != (pooled != nullptr)) return hipErrorInvalidValue;
    if (r.alt && (r.alt->ep.res || (r.stats && !(c.fused(cv) && c.fused(*r.alt->cv))))) return hipErrorInvalidValue;
    ConvParams q;
    memset(&q, 0, sizeof q);
    q.x = r.x;
    if (cv.stem) { q.xHp = c.p->xHp; q.xWp = c.p->xWp; q.xC = kStemCp; }
    else { q.xHp = cv.Hin + 2; q.xWp = cv.Win + 2; q.xC = cv.Ci; }
    q.w = c.weights(cv.fwd_off);
    q.y = r.y; q.yHp = cv.Hout + 2 * r.ypad; q.yWp = cv.Wout + 2 * r.ypad; q.yC = cv.Co; q.ypad = r.ypad;
    q.stats = r.stats ? (c.fused(cv) ? c.bn_rows(cv.bn) : c.stat_rows()) : nullptr;
    q.stat_rows = c.fused(cv) ? VPD_FUSED_ROWS : 0;
    q.ep_scale = r.ep.scale; q.ep_shift = r.ep.shift; q.res = r.ep.res; q.ep_relu = r.ep.relu;
    q.rHp = cv.Hout + 2; q.rWp = cv.Wout + 2; q.rC = cv.Co; q.rpad = 1;
    q.N = c.n; q.Hs = cv.Hout; q.Ws = cv.Wout; q.osub = 1; q.oph = 0; q.opw = 0; q.istr = cv.stride;
    q.Kc = cv.Kc; q.Co = cv.Co; q.M = c.n * cv.Hout * cv.Wout; q.accumulate = 0;
    q.taps = conv_taps_fwd(cv);
    q.err = c.sync_errors();
    double flops = conv_flops(cv, c.n);
    if (r.alt) {
        const ConvInfo& av = *r.alt->cv;
        q.alt_w = c.weights(av.fwd_off); q.alt_y = r.alt->y; q.alt_taps = conv_taps_fwd(av);
        q.alt_stats = r.stats ? c.bn_rows(av.bn) : nullptr;
        q.alt_ep_scale = r.alt->ep.scale; q.alt_ep_shift = r.alt->ep.shift; q.alt_ep_relu = r.alt->ep.relu;
        flops += conv_flops(av, c.n);
    }
    if (r.pool_y) {
        q.pool_y = r.pool_y;
        *pooled = vpd_conv_kernel_class(q) == 5;
        if (!*pooled) { q.pool_y = nullptr; q.ep_scale = nullptr; q.ep_shift = nullptr; q.ep_relu = 0; }
    }
    TimeScope ts(c.p, c.s, conv_timing_class(vpd_conv_kernel_class(q), cv), flops);
    return vpd_launch_conv(q, c.s);
}

hipError_t run_bn_finalize(const Ctx& c, const ConvInfo& cv, float* bn_running) {
    const int M = c.n * cv.Hout * cv.Wout;
    const int T = VPD_STAT_ROWS;     // unused accumulator rows are zero; the producer's tile size is its own business
    return vpd_launch_bn_finalize(c.stat_rows(), T, cv.Co, (float)M, c.params + cv.bn.w_off,
                                  c.params + cv.bn.b_off, bn_running ? bn_running + cv.bn.rm_off : nullptr,
                                  bn_running ? bn_running + cv.bn.rv_off : nullptr, kBnMomentum, kBnEps,
                                  c.bn_mean(cv.bn), c.bn_rstd(cv.bn), c.bn_scale(cv.bn), c.bn_shift(cv.bn), c.s, c.frozen);
}

// ---- data gradient ----
// launch descriptor of a conv's data gradient: dz (padded, border 1) -> dx (dense [n][Hin][Win][Ci]).  Stride 2: the caller
// fills in the parity classes (run_conv_dgrad)
ConvParams conv_dgrad_params(const Ctx& c, const ConvInfo& cv, const bf16_t* dz, bf16_t* dx, bool accumulate) {
    ConvParams q;
    memset(&q, 0, sizeof q);
    q.x = dz; q.xHp = cv.Hout + 2; q.xWp = cv.Wout + 2; q.xC = cv.Co;
    q.w = c.weights(cv.dgr_off);
    q.y = dx; q.yHp = cv.Hin; q.yWp = cv.Win; q.yC = cv.Ci; q.ypad = 0;
    q.N = c.n; q.Kc = cv.Co; q.Co = cv.Ci; q.accumulate = accumulate ? 1 : 0; q.istr = 1;
    if (cv.stride != 1) { q.osub = 2; return q; }
    // dx[y][x] = sum_{r,t} dz[y + pad - r][x + pad - t] W[r][t]; padded coord adds 1
    q.Hs = cv.Hin; q.Ws = cv.Win; q.osub = 1; q.oph = 0; q.opw = 0;
    q.M = c.n * q.Hs * q.Ws;
    q.taps.nr = cv.k; q.taps.nc = cv.k;
    q.taps.dy0 = cv.pad + 1; q.taps.dys = -1; q.taps.dx0 = cv.pad + 1; q.taps.dxs = -1;
    q.taps.w0 = 0; q.taps.wrs = cv.k; q.taps.wcs = 1;
    q.err = c.sync_errors();
    return q;
}

// The sums of a BatchNorm backward (sum g, sum g * z with g = d * mask) taken in the epilogue of the data gradient that
// produces d (ConvParams::bst_z); the BatchNorm launch is then finalize + apply only (run_bn_bwd_apply).
// z2 / rows2: a second BatchNorm fed with the same g (the 1x1 branch of a down-sampling block), or null
struct BnSums { const bf16_t* z; const unsigned char* mask; double* rows; const bf16_t* z2 = nullptr; double* rows2 = nullptr; };
void conv_set_bn_sums(ConvParams& q, const BnSums& sm) {
    q.bst_z = sm.z; q.bst_mask = sm.mask;
    vpd_conv_set_bn_rows(q, sm.rows);
    q.bst_z2 = sm.z2; q.stats2 = sm.rows2;
}
bool dgrad_takes_sums(const Ctx& c, const ConvInfo& cv, bool accumulate, bool pair = false) {
    if (!c.p->dgrad_sums) return false;
    // a stride-2 conv's merged parity classes (plain store; even input dims: the classes tile the input exactly)
    if (cv.stride != 1) return vpd_switches().dgrad_sums_s2 && cv.stride == 2 && cv.k == 3 && !accumulate && !pair && cv.Hin % 2 == 0 && cv.Win % 2 == 0;
    ConvParams q = conv_dgrad_params(c, cv, c.b16(0), c.b16(0), accumulate);
    // The answer depends on which sums are asked for, not on where they go: the probe has no mask and no rows.  It carries
    // stat_rows = VPD_FUSED_ROWS with null rows, as conv_set_bn_sums leaves it; no host decision reads stat_rows (the kernels do),
    // and conv_ep_mode reads bst_z / bst_z2 / accumulate alone once bst_z is set.
    BnSums probe{c.b16(0), /*mask*/ nullptr, /*rows*/ nullptr};
    if (pair) { probe.z2 = c.b16(0); probe.rows2 = c.stat_rows(); }
    conv_set_bn_sums(q, probe);
    return vpd_conv_takes_bn_sums(q);
}

// ds / dzd: the block's 1x1 stride-2 down-sampling conv and its dz -- its data gradient lands on the even-even input pixels,
// which are class 0 of the 3x3's: extra K-steps of those blocks instead of a read-modify-write launch of its own (stride 2 only).
// accumulate: dx += (stride 1 only: a stride-2 launch's classes store); acc_mask: ... onto dx masked by this ReLU bit map.
// sums: the BatchNorm whose dy this launch produces has its backward sums taken here.  The caller has asked dgrad_takes_sums;
// vpd_launch_conv refuses sums that its kernel does not take (vpd_conv_takes_bn_sums on the launch's own descriptor).
struct ConvDgrad {
    const bf16_t* dz = nullptr; bf16_t* dx = nullptr; bool accumulate = false;
    const ConvInfo* ds = nullptr; const bf16_t* dzd = nullptr;
    const unsigned char* acc_mask = nullptr;
    const BnSums* sums = nullptr;
};
hipError_t run_conv_dgrad(const Ctx& c, const ConvInfo& cv, const ConvDgrad& r) {
    ConvParams q = conv_dgrad_params(c, cv, r.dz, r.dx, r.accumulate);
    if (r.acc_mask && !r.accumulate) return hipErrorInvalidValue;      // (a mask is applied to what is accumulated onto)
    if (r.sums) conv_set_bn_sums(q, *r.sums);
    if (cv.stride == 1) {
        if (r.ds) return hipErrorInvalidValue;
        q.acc_mask = r.acc_mask;
        TimeScope ts(c.p, c.s, conv_timing_class(vpd_conv_kernel_class(q), cv), conv_flops(cv, c.n));
        return vpd_launch_conv(q, c.s);
    }
    // stride 2: the four input-pixel parity classes are ONE launch (grid.z = class).  Only taps r with
    // (ph + pad - r) even contribute: r = rf, rf+2, ... reading dz row  y + (ph + pad - r)/2  (+1 for the border).
    if (r.acc_mask || (r.sums && r.sums->z2)) return hipErrorInvalidValue;      // (no masked store, no second BatchNorm)
    TimeScope ts(c.p, c.s, TC_GATHER, conv_flops(cv, c.n) + (r.ds ? conv_flops(*r.ds, c.n) : 0.0));
    int ncls = 0;
    for (int ph = 0; ph < 2; ++ph)
        for (int pw = 0; pw < 2; ++pw) {
            ConvClass k;
            k.geo.Hs = (cv.Hin - ph + 1) / 2; k.geo.Ws = (cv.Win - pw + 1) / 2;
            if (k.geo.Hs <= 0 || k.geo.Ws <= 0) continue;
            k.geo.oph = ph; k.geo.opw = pw;
            k.geo.M = c.n * k.geo.Hs * k.geo.Ws;
            const int rf = (ph + cv.pad) % 2, tf = (pw + cv.pad) % 2;
            k.taps.nr = rf < cv.k ? (cv.k - rf + 1) / 2 : 0;
            k.taps.nc = tf < cv.k ? (cv.k - tf + 1) / 2 : 0;
            if (k.taps.nr == 0 || k.taps.nc == 0) continue;   // caller zero-fills / overwrites those pixels
            k.taps.dy0 = (ph + cv.pad - rf) / 2 + 1; k.taps.dys = -1;
            k.taps.dx0 = (pw + cv.pad - tf) / 2 + 1; k.taps.dxs = -1;
            k.taps.w0 = rf * cv.k + tf; k.taps.wrs = 2 * cv.k; k.taps.wcs = 2;
            if (ncls == 0) {
                q.Hs = k.geo.Hs; q.Ws = k.geo.Ws; q.M = k.geo.M; q.oph = ph; q.opw = pw; q.taps = k.taps;
            } else {
                q.cls[ncls - 1] = k;
            }
            ++ncls;
        }
    if (ncls == 0) return hipSuccess;
    q.ncls = ncls;
    if (r.ds) {
        if (q.oph != 0 || q.opw != 0 || q.taps.nr != 1 || q.taps.nc != 1 || r.ds->Co != cv.Co) return hipErrorInvalidValue;
        q.x2 = r.dzd; q.w2 = c.weights(r.ds->dgr_off); q.Kc2 = r.ds->Co;
    }
    return vpd_launch_conv(q, c.s);      // (sums: the four classes together write every pixel of dx exactly once)
}

// ---- weight gradient ----
// A conv's weight-gradient problem as its own launch takes it: dw, the slab region, the halo wish of a 1x1, the stem's geometry;
// whether that launch overwrites dw.  The generic kernel accumulates with atomics instead: its range of the scratch is zeroed at
// the start of the backward (wgrad_zero_range).  The route depends on the shapes alone, not on dz / x.
struct WgradProblem { WgradParams q; bool overwrites; };
WgradProblem conv_wgrad_problem(const Ctx& c, const ConvInfo& cv, const bf16_t* dz, const bf16_t* x) {
    WgradProblem w;
    WgradParams& q = w.q;
    q = wgrad_params(cv, c.n, dz, x);
    if (cv.stem) { q.dzHp = cv.Hout; q.dzWp = cv.Wout; q.dzpad = 0; q.xHp = c.p->xHp; q.xWp = c.p->xWp; q.xC = kStemCp; }
    q.dw = c.f32(c.p->wg_off) + cv.wg_off;
    float* slab = c.f32(c.p->slab_off);
    q.slab = cv.slab_off >= 0 ? slab + cv.slab_off : (cv.stem ? slab : nullptr);
    q.prefer_halo_1x1 = !c.p->bottleneck;      // BasicBlock students: the three down-sampling 1x1 convs without atomics
    w.overwrites = vpd_wgrad_overwrites(q);       // (no slab: never)
    if (cv.slab_off >= 0 && !w.overwrites) q.slab = nullptr;      // (an A/B switch turned the halo form off: generic kernel)
    return w;
}
void wgrad_zero_range(const Ctx& c, const ConvInfo& cv, ZeroRanges& z) {
    const WgradProblem w = conv_wgrad_problem(c, cv, /*dz*/ nullptr, /*x*/ nullptr);
    if (w.overwrites || z.count >= ZR_MAX) return;
    z.ptr[z.count] = w.q.dw;
    z.n4[z.count++] = (long)cv.ntaps * cv.Co * cv.Kc / 4;
}
// weight gradient of a conv in launches of its own
hipError_t run_conv_wgrad(const Ctx& c, const ConvInfo& cv, const bf16_t* dz, const bf16_t* x) {
    WgradProblem w = conv_wgrad_problem(c, cv, dz, x);
    if (w.overwrites && !cv.stem) {      // time the MFMA kernel alone, then sum its slab
        hipError_t e;
        {
            TimeScope ts(c.p, c.s, cv.stride == 1 ? TC_WGRAD_STAGE : TC_WGRAD_CONV, conv_flops(cv, c.n));
            w.q.defer_reduce = 1;
            e = vpd_launch_wgrad(w.q, c.s);
        }
        if (e != hipSuccess) return e;
        return vpd_launch_wgrad_reduce(w.q, c.s);
    }
    TimeScope ts(c.p, c.s, cv.stem ? TC_STEM : (w.overwrites ? TC_WGRAD_STAGE : TC_WGRAD_CONV), conv_flops(cv, c.n));
    return vpd_launch_wgrad(w.q, c.s);
}
// A down-sampling BasicBlock's conv1 (3x3 stride 2) and 1x1 branch can run as ONE launch, the branch riding on conv1's staged halo
// (vpd_wgrad_pair_ok; VPD_WGRAD_DS_RIDE=0: two launches).  Each problem stays what conv_wgrad_problem states.
bool wgrad_pair_ok(const Ctx& c, const ConvInfo& c1, const ConvInfo& cd) {
    if (c1.stem || cd.stem || c1.dz_own_off || cd.dz_own_off) return false;
    return vpd_wgrad_pair_ok(conv_wgrad_problem(c, c1, c.b16(0), c.b16(0)).q, conv_wgrad_problem(c, cd, c.b16(0), c.b16(0)).q);
}
hipError_t run_conv_wgrad_pair(const Ctx& c, const ConvInfo& c1, const ConvInfo& cd, const bf16_t* dz1, const bf16_t* dzd, const bf16_t* x) {
    WgradParams q3 = conv_wgrad_problem(c, c1, dz1, x).q;
    const WgradParams q1 = conv_wgrad_problem(c, cd, dzd, x).q;
    hipError_t e;
    {
        TimeScope ts(c.p, c.s, TC_WGRAD_CONV, conv_flops(c1, c.n) + conv_flops(cd, c.n));      // (as each of the two launches it replaces)
        q3.defer_reduce = 1;
        e = vpd_launch_wgrad_pair(q3, q1, c.s);
    }
    if (e != hipSuccess) return e;
    return vpd_launch_wgrad_pair_reduce(q3, q1, c.s);
}

// ---- BatchNorm forward (train mode) ----
// conv `cv`'s dense z -> BatchNorm -> (+ residual) -> ReLU -> `out`, padded by 1.  The residual: `res` alone is a padded activation;
// with res_cv, `res` is that conv's dense z (the down-sampling branch), normalised by its own BatchNorm in the same launch.
// mask_out: the ReLU bit map of `out`, written by the fused launch only (nothing reads it when the BatchNorm is not fused)
struct BnFwd { bf16_t* out = nullptr; unsigned char* mask_out = nullptr; const bf16_t* res = nullptr; const ConvInfo* res_cv = nullptr; };
BnApplyParams bn_apply_params(const Ctx& c, const ConvInfo& cv, const BnFwd& r) {
    const int res_kind = r.res_cv ? 2 : (r.res ? 1 : 0);
    return vpd_bn_apply_params(c.b16(cv.z_off), res_kind, r.res, r.out, c.n, cv.Hout, cv.Wout, cv.Co, kRelu);
}
hipError_t run_bn_apply(const Ctx& c, const ConvInfo& cv, const BnFwd& r) {
    BnApplyParams a = bn_apply_params(c, cv, r);
    a.scale = c.bn_scale(cv.bn); a.shift = c.bn_shift(cv.bn);
    if (r.res_cv) { a.rscale = c.bn_scale(r.res_cv->bn); a.rshift = c.bn_shift(r.res_cv->bn); }
    return vpd_launch_bn_apply(a, c.s);
}

// train-mode convolution: dense z + per-channel statistics.  Unfused BatchNorm: the statistics go to the SHARED rows,
// which the finalize launch right behind the conv consumes and re-zeroes; fused: to the BatchNorm's own rows.
hipError_t run_conv_train(const Ctx& c, const ConvInfo& cv, const bf16_t* x, float* bn_running, const AltConv* alt = nullptr) {
    ConvFwd f;
    f.x = x; f.y = c.b16(cv.z_off); f.stats = true; f.alt = alt;
    hipError_t e = run_conv_fwd(c, cv, f);
    if (e != hipSuccess || c.fused(cv)) return e;
    return run_bn_finalize(c, cv, bn_running);
}

// Pixel tile of the pipelined 3x3 launches next to conv `cv`'s BatchNorm (its own forward / data gradient, and -- same stage, same
// shape -- its neighbours'), when they run in their XCD-affine tile order: the fused BatchNorm launches then take their items in
// the matching block order (bn.hip, vpd_bn_virtual_block).  3x3 stride-1 convolutions with Ci == Co only; 0 otherwise.
int bn_xcd_tile_px(const Ctx& c, const ConvInfo& cv) {
    if (cv.k != 3 || cv.stride != 1 || cv.stem || cv.Ci != cv.Co) return 0;
    const ConvParams q = conv_dgrad_params(c, cv, c.b16(0), c.b16(0), false);
    return vpd_conv_xcd_tile_px(q);
}

// conv `cv`'s BatchNorm as one side of a fused forward launch
BnFwdSide bn_fwd_side(const Ctx& c, const ConvInfo& cv, float* bn_running) {
    const BnInfo& b = cv.bn;
    BnFwdSide f;
    f.rows = c.bn_rows(b); f.gamma = c.params + b.w_off; f.beta = c.params + b.b_off;
    f.rm = bn_running ? bn_running + b.rm_off : nullptr; f.rv = bn_running ? bn_running + b.rv_off : nullptr;
    f.mean = c.bn_mean(b); f.rstd = c.bn_rstd(b); f.scale = c.bn_scale(b); f.shift = c.bn_shift(b);
    return f;
}
// the fused forward launch: conv `cv`'s BatchNorm and, when given, the residual branch's (`cv2`, same shape)
BnFusedFwd bn_fused_fwd(const Ctx& c, const ConvInfo& cv, float* bn_running, const ConvInfo* cv2 = nullptr) {
    BnFusedFwd f;
    memset(&f, 0, sizeof f);
    f.s[0] = bn_fwd_side(c, cv, bn_running);
    if (cv2) f.s[1] = bn_fwd_side(c, *cv2, bn_running);
    f.count = (float)(c.n * cv.Hout * cv.Wout); f.momentum = kBnMomentum; f.eps = kBnEps; f.frozen = c.frozen;
    return f;
}
// BatchNorm (+ residual, ReLU) of a train-mode forward: statistics -> normalised padded activation.  A residual branch's BatchNorm
// (BnFwd::res_cv) is finalized here too.  One launch when fused.
hipError_t run_bn_fwd(const Ctx& c, const ConvInfo& cv, float* bn_running, const BnFwd& r) {
    if (!c.fused(cv)) return run_bn_apply(c, cv, r);      // (finalized by run_conv_train)
    BnApplyParams a = bn_apply_params(c, cv, r);
    a.mask_out = r.mask_out;
    a.xcd_tile_px = bn_xcd_tile_px(c, cv);
    return vpd_launch_bn_fwd_fused(a, bn_fused_fwd(c, cv, bn_running, r.res_cv), c.s);
}

// ---- BatchNorm backward ----
// geometry of conv cv's BatchNorm backward: dy (dense) -> dz (padded by 1)
BnBwdParams bn_bwd_params(const Ctx& c, const ConvInfo& cv, const bf16_t* dy, bf16_t* dz) {
    return vpd_bn_bwd_params(dy, c.b16(cv.z_off), c.bn_mean(cv.bn), c.bn_rstd(cv.bn), dz, kDzPad, c.n, cv.Hout, cv.Wout, cv.Co);
}
// conv `cv`'s BatchNorm as one side of a fused backward launch; dz: where a launch that reads the side's own writes it
BnBwdSide bn_bwd_side(const Ctx& c, const ConvInfo& cv, float* grads, bf16_t* dz) {
    return BnBwdSide{c.bn_rows(cv.bn), c.params + cv.bn.w_off, c.bn_dgamma(cv.bn, grads), c.bn_dbeta(cv.bn, grads),
                     c.b16(cv.z_off), c.bn_mean(cv.bn), c.bn_rstd(cv.bn), dz};
}
// the fused backward launch of cv's BatchNorm and, when given, a second one of the same shape (launches with a grid barrier add
// sync / err)
BnFusedBwd bn_fused_bwd(const Ctx& c, const ConvInfo& cv, float* grads, bf16_t* dz = nullptr, const ConvInfo* cvB = nullptr,
                        bf16_t* dzB = nullptr) {
    BnFusedBwd f;
    memset(&f, 0, sizeof f);
    f.s[0] = bn_bwd_side(c, cv, grads, dz);
    if (cvB) f.s[1] = bn_bwd_side(c, *cvB, grads, dzB);
    f.count = (float)(c.n * cv.Hout * cv.Wout); f.frozen = c.frozen;
    return f;
}
void bn_bwd_barrier(const Ctx& c, const ConvInfo& cv, BnFusedBwd& f) {
    f.sync = c.ws + cv.bn.sync_off; f.err = c.sync_errors();
}

// the fused launch with a ReLU bit map takes cv's BatchNorm (the condition under which a block output's mask is a bit map)
bool relu_bits_ok(const Ctx& c, const ConvInfo& cv) {
    return c.p->relu_bits && c.fused(cv) && vpd_bn_bwd_fused_ok(c.n * cv.Hout * cv.Wout, cv.Co, /*mask_act*/ false, /*write_g*/ false);
}
// dy -> dz.  The ReLU between the BatchNorm and dy is at most one of:
//   act          the stored activation (needed when a residual was added before the ReLU); write_g: g = dy * mask is written back to dy
//   relu_from_z  the mask recomputed as scale * z + shift > 0 (plain conv-BN-ReLU), which saves reading the activation
//   mask_bits    the forward's bit map: fused launch only, dy stays unmasked (the consumer of the identity path masks it itself)
// and none of them when dy already holds g.
// dy_pooled: dy has not been produced yet -- it is the gradient of the global average pool over cv's output (the last block of
// the network); the fused launch with a ReLU bit map produces it itself, every other path gets the avgpool_bwd launch first
struct BnBwd {
    bf16_t* dy = nullptr; bf16_t* dz = nullptr;
    const bf16_t* act = nullptr; bool write_g = false;
    bool relu_from_z = false;
    const unsigned char* mask_bits = nullptr;
    const float* dy_pooled = nullptr;
};
hipError_t run_bn_bwd(const Ctx& c, const ConvInfo& cv, const BnBwd& r, float* grads) {
    if ((r.act != nullptr) + (r.relu_from_z ? 1 : 0) + (r.mask_bits != nullptr) > 1 || (r.write_g && !r.act)) return hipErrorInvalidValue;
    BnBwdParams b = bn_bwd_params(c, cv, r.dy, r.dz);
    vpd_bn_bwd_set_act(b, r.dy, r.act);
    b.coef = c.bn_coef(cv.bn); b.partials = c.stat_rows(); b.write_g = r.write_g ? 1 : 0;
    b.mask_bits = r.mask_bits;
    if (r.relu_from_z) { b.mscale = c.bn_scale(cv.bn); b.mshift = c.bn_shift(cv.bn); }
    const bool fused = c.fused(cv) && vpd_bn_bwd_fused_ok(b.M, b.C, b.act != nullptr, b.write_g != 0);
    if (r.mask_bits && !fused) return hipErrorInvalidValue;      // (the three-launch path has no bit-map form: it would run unmasked)
    if (r.dy_pooled) {
        // (the fold multiplies by 1 / (H W), exact for a power-of-two map; any other map takes avgpool_bwd_kernel's division)
        const int hw = cv.Hout * cv.Wout;
        if (fused && r.mask_bits && vpd_switches().poolbwd_fold && (hw & (hw - 1)) == 0) { b.dy_pooled = r.dy_pooled; b.dy_pool_scale = 1.f / (float)hw; }
        else {
            hipError_t e = vpd_launch_avgpool_bwd(r.dy_pooled, cv.Hout, cv.Wout, cv.Co, c.n, r.dy, c.s);
            if (e != hipSuccess) return e;
        }
    }
    if (fused) {
        BnFusedBwd f = bn_fused_bwd(c, cv, grads);
        bn_bwd_barrier(c, cv, f);
        return vpd_launch_bn_bwd_fused(b, f, c.s);
    }
    return vpd_launch_bn_bwd(b, (float)b.M, c.params + cv.bn.w_off, c.bn_dgamma(cv.bn, grads), c.bn_dbeta(cv.bn, grads), c.s, c.frozen);
}

// BatchNorm backward whose sums were taken by the producing data gradient (BnSums): finalize + apply
// cvB / dzB: a second BatchNorm fed with the same masked gradient (a down-sampling block's 1x1 branch), same launch
hipError_t run_bn_bwd_apply(const Ctx& c, const ConvInfo& cv, const bf16_t* dy, bf16_t* dz, float* grads,
                            const unsigned char* mask_bits, const ConvInfo* cvB = nullptr, bf16_t* dzB = nullptr) {
    BnBwdParams b = bn_bwd_params(c, cv, dy, dz);
    b.mask_bits = mask_bits;
    b.xcd_tile_px = bn_xcd_tile_px(c, cv);
    return vpd_launch_bn_bwd_apply_fused(b, bn_fused_bwd(c, cv, grads, dz, cvB, dzB), c.s);
}

// block-output BatchNorm (A: the block's last conv) and the down-sampling branch's BatchNorm (Bc) in one launch: same dy,
// same ReLU mask (bn_bwd_fused2_kernel).  Not applicable (bn_bwd_pair_ok false): the caller runs them one after the other
bool bn_bwd_pair_ok(const Ctx& c, const ConvInfo& A, const ConvInfo& Bc) {
    return c.fused(A) && c.fused(Bc) && A.Co == Bc.Co && vpd_bn_bwd_fused2_ok(c.n * A.Hout * A.Wout, A.Co);
}
hipError_t run_bn_bwd_pair(const Ctx& c, const ConvInfo& A, const ConvInfo& Bc, bf16_t* dy, const bf16_t* act, bf16_t* dzA,
                           bf16_t* dzB, float* grads) {
    BnBwdParams b = bn_bwd_params(c, A, dy, dzA);
    vpd_bn_bwd_set_act(b, dy, act);
    BnFusedBwd f = bn_fused_bwd(c, A, grads, dzA, &Bc, dzB);
    bn_bwd_barrier(c, A, f);
    return vpd_launch_bn_bwd_fused2(b, f, c.s);
}

// ---- a Bottleneck's closing 1x1 convolution together with its BatchNorm, the convolution recomputed instead of written and read
// back (conv_stream.hip, conv1x1_bn_stream_kernel; VPD_BNECK_RECOMPUTE=0: conv + BatchNorm launches) ----
enum BlockTail {
    TAIL_STORED,                // conv, then BatchNorm launches on the stored z
    TAIL_RECOMPUTED,            // an identity block: z3 is never stored
    TAIL_RECOMPUTED_BRANCH,     // a DOWN-SAMPLING block whose closing 1x1 conv and 1x1 branch both have 64 input channels and stride 1
                                // (layer1's first block): both convolutions and both BatchNorms in the same launches
                                // (conv1x1_bn2_stream_kernel); neither z3 nor zd is stored
};
ConvParams conv3_params(const Ctx& c, const ConvInfo& cv, const bf16_t* x) {
    return vpd_conv1x1_params(x, c.weights(cv.fwd_off), c.n, cv.Hout, cv.Wout, cv.stride, cv.Kc, cv.Co);
}
ConvParams conv3d_params(const Ctx& c, const BlockInfo& B, const bf16_t* xin) {
    ConvParams q = conv3_params(c, B.c3, c.b16(B.a2_off));
    q.x2 = xin; q.w2 = c.weights(B.cd.fwd_off); q.Kc2 = B.cd.Kc;
    return q;
}
// relu_bits: relu_bits_ok of B.c3 (the backward passes of the tail read the bit map)
BlockTail block_tail(const Ctx& c, const BlockInfo& B, bool relu_bits) {
    if (!c.p->bottleneck || !c.train || !relu_bits || !c.fused(B.c3) || B.c3.k != 1 || B.c3.stride != 1) return TAIL_STORED;
    if (!B.ds) return vpd_conv1x1_bn_eligible(conv3_params(c, B.c3, c.b16(B.a2_off))) ? TAIL_RECOMPUTED : TAIL_STORED;
    if (!c.fused(B.cd) || B.cd.k != 1 || B.cd.stride != 1 || B.c3.Ci != B.cd.Ci || B.c3.Co != B.cd.Co) return TAIL_STORED;
    if (B.c3.Hin != B.cd.Hin || B.c3.Win != B.cd.Win) return TAIL_STORED;
    return vpd_conv1x1_bn2_eligible(conv3d_params(c, B, c.b16(B.a2_off))) ? TAIL_RECOMPUTED_BRANCH : TAIL_STORED;
}
BnTailLaunch tail_pass(BnTailPass pass) {
    BnTailLaunch t;
    memset(&t, 0, sizeof t);
    t.pass = pass;
    return t;
}
// one pass of the tail (two: the pair launch of a down-sampling block), in the gather kernels' timing class
hipError_t launch_tail(const Ctx& c, const ConvParams& q, const BnTailLaunch& t, bool two, double flops) {
    TimeScope ts(c.p, c.s, TC_GATHER, flops);
    return two ? vpd_launch_conv1x1_bn2(q, t, c.s) : vpd_launch_conv1x1_bn(q, t, c.s);
}
constexpr double kNoFlops = 0.0;      // a recomputation or a BatchNorm pass: its time counts, algorithmic matrix FLOPs it has none
// the statistics pass of conv `cv` on x
hipError_t run_conv3_bn_stats(const Ctx& c, const ConvInfo& cv, const bf16_t* x) {
    ConvParams q = conv3_params(c, cv, x);
    vpd_conv_set_bn_rows(q, c.bn_rows(cv.bn));
    return launch_tail(c, q, tail_pass(BN_TAIL_STATS), false, kNoFlops);
}
// forward: the statistics passes, then relu(BatchNorm(conv(a2)) + residual) -> out (padded) + the ReLU bit map.  The residual: the
// block input xin (TAIL_RECOMPUTED), or BatchNorm(1x1 branch(xin)) (TAIL_RECOMPUTED_BRANCH)
hipError_t run_tail_fwd(const Ctx& c, const BlockInfo& B, bool two, const bf16_t* xin, bf16_t* out, unsigned char* mask_out,
                        float* bn_running) {
    hipError_t e = run_conv3_bn_stats(c, B.c3, c.b16(B.a2_off));
    if (e == hipSuccess && two) e = run_conv3_bn_stats(c, B.cd, xin);
    if (e != hipSuccess) return e;
    ConvParams q = two ? conv3d_params(c, B, xin) : conv3_params(c, B.c3, c.b16(B.a2_off));
    vpd_conv_set_y(q, out, 1);
    if (!two) vpd_conv_set_res(q, xin);
    const BnFusedFwd f = bn_fused_fwd(c, B.c3, bn_running, two ? &B.cd : nullptr);
    BnTailLaunch t = tail_pass(BN_TAIL_FWD);
    t.fwd = &f; t.mask_out = mask_out;
    return launch_tail(c, q, t, two, conv_flops(B.c3, c.n) + (two ? conv_flops(B.cd, c.n) : 0.0));
}
// backward: the sums of g = dout * mask and g * z, then dz = A g + B z + D -> every side's dz (padded by 1), dgamma, dbeta
hipError_t run_tail_bwd(const Ctx& c, const BlockInfo& B, bool two, const bf16_t* xin, bf16_t* dout, const unsigned char* mask_bits,
                        bf16_t* dz3, bf16_t* dzd, float* grads) {
    ConvParams q = two ? conv3d_params(c, B, xin) : conv3_params(c, B.c3, c.b16(B.a2_off));
    q.y = dout; q.acc_mask = mask_bits;
    const BnFusedBwd f = two ? bn_fused_bwd(c, B.c3, grads, dz3, &B.cd, dzd) : bn_fused_bwd(c, B.c3, grads, dz3);
    BnTailLaunch t = tail_pass(BN_TAIL_BWD_SUMS);
    t.bwd = &f;
    hipError_t e = launch_tail(c, q, t, two, kNoFlops);
    if (e != hipSuccess) return e;
    t.pass = BN_TAIL_BWD_APPLY; t.dzpad = kDzPad;
    return launch_tail(c, q, t, two, kNoFlops);
}

// ---- what the passes of a block do ----
// Decided once per pass (it depends on n and on the pass being a training one); the train forward, the eval forward (conv_pair
// alone) and the backward read it.  The BasicBlock-only routes say so here, not by a predicate that happens to fail elsewhere.
struct BlockRoute {
    bool conv_pair = false;         // forward: the down-sampling 1x1 rides in conv1's launch (conv_pair_ok)
    bool dgrad_pair = false;        // backward: ... and its data gradient in conv1's merged stride-2 data gradient
    BlockTail tail = TAIL_STORED;   // the closing conv + BatchNorm (Bottleneck)
    bool bn_pair = false;           // backward: the closing BatchNorm and the branch's in one launch (bn_bwd_pair_ok)
    bool wgrad_pair = false;        // backward: the branch's weight gradient rides in conv1's launch (wgrad_pair_ok)
    bool relu_bits = false;         // the closing BatchNorm's backward can read its ReLU as the forward's bit map (relu_bits_ok)
    bool mask_in_dgrad = false;     // ... and does (identity blocks): d(out) stays unmasked, conv1's data gradient masks it when it adds it
    bool sums_pair = false;         // a down-sampling block: the next block's data gradient may take the sums of both closing BatchNorms
};
BlockRoute block_route(const Ctx& c, const BlockInfo& B) {
    BlockRoute R;
    R.conv_pair = B.ds && conv_pair_ok(c, B.c1, B.cd);
    if (!c.train) return R;      // (eval: every BatchNorm is a conv epilogue)
    const bool basic = !c.p->bottleneck;
    const ConvInfo& last = basic ? B.c2 : B.c3;
    R.dgrad_pair = basic && R.conv_pair;
    R.relu_bits = relu_bits_ok(c, last);
    R.mask_in_dgrad = !B.ds && R.relu_bits;
    R.tail = block_tail(c, B, R.relu_bits);
    R.bn_pair = B.ds && bn_bwd_pair_ok(c, last, B.cd);
    R.wgrad_pair = basic && B.ds && wgrad_pair_ok(c, B.c1, B.cd);
    R.sums_pair = basic && B.ds && vpd_switches().dgrad_sums_pair && c.fused(B.c2) && c.fused(B.cd) && B.c2.Co == B.cd.Co;
    return R;
}

// ---- head ----
long pred_numel(const vpd_plan* p, int n) { return (long)n * (p->motion ? 2 * p->D : p->D); }      // elements of the prediction
// a linear layer L in exact fp32 (head.hip): y = x W^T + b (ReLU); dW = dy^T x, db = column sums of dy; dx = dy W
hipError_t linear_fwd(const Ctx& c, const LinInfo& L, const float* x, float* y, int relu) {
    return vpd_launch_sgemm(x, c.params + L.w_off, y, c.params + L.b_off, c.n, L.out, L.in, /*ta*/ 0, /*tb*/ 1, relu, c.s);
}
hipError_t linear_bwd_params(const Ctx& c, const LinInfo& L, const float* dy, const float* x, float* grads) {
    hipError_t e = vpd_launch_sgemm(dy, x, grads + L.w_off, /*bias*/ nullptr, L.out, L.in, c.n, /*ta*/ 1, /*tb*/ 0, kNoRelu, c.s);
    if (e != hipSuccess) return e;
    return vpd_launch_colsum(dy, c.n, L.out, grads + L.b_off, c.s);
}
hipError_t linear_bwd_data(const Ctx& c, const LinInfo& L, const float* dy, float* dx) {
    return vpd_launch_sgemm(dy, c.params + L.w_off, dx, /*bias*/ nullptr, c.n, L.in, L.out, /*ta*/ 0, /*tb*/ 0, kNoRelu, c.s);
}
// the motion head's buffers: layer i (vpd_plan::dec[i]) maps act[i] to act[i + 1]; dact[i] is the gradient of act[i]
struct MotionBufs { float* act[4]; float* dact[4]; };
MotionBufs motion_bufs(const Ctx& c) {
    const vpd_plan* p = c.p;
    return MotionBufs{{c.f32(p->emb_off), c.f32(p->h1_off), c.f32(p->h2_off), c.f32(p->pred_off)},
                      {c.f32(p->demb_off), c.f32(p->dh1_off), c.f32(p->dh2_off), c.f32(p->dpred_off)}};
}

// encoder head shared by eval / train: avgpool + fc (+ motion MLP) (+ loss)
int run_head(const Ctx& c, const bf16_t* last_act, float* emb_out, const float* target, bool need_grad,
             float* loss_step, double* loss_accum) {
    vpd_plan* p = c.p;
    const StageInfo& S = p->stages[3];
    LCHECK(vpd_launch_avgpool(last_act, S.H + 2, S.W + 2, 1, S.H, S.W, p->feat, c.n, c.f32(p->pooled_off), c.s));
    // without the motion head nothing re-reads the embedding (the fc backward uses the pooled features and d(emb)): the fc
    // GEMM writes the caller's buffer directly; with it, the head's first layer and its weight gradient read the workspace copy
    float* emb = (emb_out && !p->motion) ? emb_out : c.f32(p->emb_off);
    LCHECK(linear_fwd(c, p->fc, c.f32(p->pooled_off), emb, kNoRelu));
    if (emb_out && emb != emb_out) LCHECK(hipMemcpyAsync(emb_out, emb, (size_t)c.n * p->D * 4, hipMemcpyDeviceToDevice, c.s));
    if (!target) return 0;
    const float* pred = emb;
    if (p->motion) {
        const MotionBufs mb = motion_bufs(c);
        for (int i = 0; i < 3; ++i) LCHECK(linear_fwd(c, p->dec[i], mb.act[i], mb.act[i + 1], i < 2 ? kRelu : kNoRelu));
        pred = mb.act[3];
    }
    LCHECK(vpd_launch_mse(pred, target, pred_numel(p, c.n), need_grad ? c.f32(p->dpred_off) : nullptr, loss_step,
                          loss_accum, c.s));
    return 0;
}

// accumulator rows (and, fused, every BatchNorm's rows and barrier words): zeroed at the start of each train pass
ZeroRanges accumulator_zero_ranges(const Ctx& c) {
    ZeroRanges z;
    memset(&z, 0, sizeof z);
    z.ptr[0] = c.f32(c.p->partial_off); z.n4[0] = (long)c.p->partial_bytes / 16; z.count = 1;
    if (c.p->fused_bn) { z.ptr[1] = c.f32(c.p->fused_off); z.n4[1] = (long)c.p->fused_bytes / 16; z.count = 2; }
    return z;
}

hipError_t pack_input(const Ctx& c, const float* x) {
    const vpd_plan* p = c.p;
    return vpd_launch_pack_input(x, c.n, p->c_in, p->H, p->W, c.b16(p->xin_off), p->xHp, p->xWp, kStemPad, kStemCp, c.s);
}
// the stem's BatchNorm + ReLU + max-pool launch; idx: the argmax map of a train pass (eval: null)
StemPoolParams stem_pool_params(const Ctx& c, const float* scale, const float* shift, unsigned char* idx) {
    StemPoolParams sp;
    memset(&sp, 0, sizeof sp);
    sp.z = c.b16(c.p->z0_off); sp.Hz = c.p->H0; sp.Wz = c.p->W0;
    sp.scale = scale; sp.shift = shift;
    sp.out = c.b16(c.p->p0_off); sp.opad = 1; sp.idx = idx; sp.N = c.n; sp.Ho = c.p->H1; sp.Wo = c.p->W1; sp.C = c.p->stem.Co;
    return sp;
}

int run_eval_forward(vpd_plan* p, const float* params, const float* x, int n, float* emb_out, const float* target,
                     float* loss_step, double* loss_accum, char* ws, hipStream_t s) {
    Ctx c{p, ws, s, params, n};
    if (x) LCHECK(pack_input(c, x));
    // stem: conv + folded BatchNorm + ReLU + max-pool in ONE launch when the stem kernel takes the shape and there are enough
    // images for its image-per-block walk (VPD_STEM_POOL_FUSED=0: conv, then the pooling launch)
    const ConvEpilogue stem_ep = c.eval_epilogue(p->stem, kRelu);
    ConvFwd f0;
    f0.x = c.b16(p->xin_off); f0.y = c.b16(p->z0_off);
    bool pooled = false;
    if (vpd_switches().stem_pool_fused && n >= 64) {
        f0.ep = stem_ep; f0.pool_y = c.b16(p->p0_off);
        LCHECK(run_conv_fwd(c, p->stem, f0, &pooled));
    } else {
        LCHECK(run_conv_fwd(c, p->stem, f0));
    }
    if (!pooled) LCHECK(vpd_launch_stem_pool(stem_pool_params(c, stem_ep.scale, stem_ep.shift, nullptr), s));
    const bf16_t* cur = c.b16(p->p0_off);
    // a conv with its folded BatchNorm (+ residual) (+ ReLU) into a padded activation
    auto conv = [&](const ConvInfo& cv, const bf16_t* in, bf16_t* out, const ConvEpilogue& ep, const AltConv* alt = nullptr) {
        ConvFwd f;
        f.x = in; f.y = out; f.ypad = 1; f.ep = ep; f.alt = alt;
        return run_conv_fwd(c, cv, f);
    };
    for (auto& B : p->blocks) {
        const BlockRoute R = block_route(c, B);
        bf16_t* a1 = c.b16(B.a1_off);
        bf16_t* idb = c.b16(p->stages[B.stage].idn_off);      // the down-sampling branch's output
        const AltConv alt{&B.cd, idb, c.eval_epilogue(B.cd, kNoRelu)};      // the down-sampling 1x1 rides in conv1's launch
        LCHECK(conv(B.c1, cur, a1, c.eval_epilogue(B.c1, kRelu), R.conv_pair ? &alt : nullptr));
        const bf16_t* last_in = a1;
        if (p->bottleneck) {
            last_in = c.b16(B.a2_off);
            LCHECK(conv(B.c2, a1, c.b16(B.a2_off), c.eval_epilogue(B.c2, kRelu)));
        }
        if (B.ds && !R.conv_pair) LCHECK(conv(B.cd, cur, idb, alt.ep));
        const ConvInfo& last = p->bottleneck ? B.c3 : B.c2;
        LCHECK(conv(last, last_in, c.b16(B.out_off), c.eval_epilogue(last, kRelu, B.ds ? idb : cur)));
        cur = c.b16(B.out_off);
    }
    return run_head(c, cur, emb_out, target, false, loss_step, loss_accum);
}

// ---- backward ----
// Weight gradients of the convs that keep their own dz (ConvInfo::dz_own_off) wait in `pending` for their stage's grouped
// launch; every other conv's runs at once.  A stage's gradient bucket is handed over -- unpacked, its event recorded -- only
// behind that launch.  (Running weight gradients or their slab sums on a second stream was measured 6 % slower in round 2 and,
// with the persistent kernels, 1.4 % slower in round 6; confined to a CU partition 40-50 % slower:
// profiles/r06_ab_wgrad_overlap.txt, tools/probe/wg_overlap.patch)
struct WgradQueue {
    const Ctx& c;
    float* grads;
    void** bucket_events;
    // lazy: the caller asked for it (vpd_plan_set_lazy_grads).  With bucket events the reducer then sums the scratch ranges
    // (vpd_plan_bucket_scratch_range) and the non-conv tensors of the flat buffer instead of the whole flat buffer
    bool lazy;
    struct Pending { const ConvInfo* cv; const bf16_t* dz; const bf16_t* x; };
    std::vector<Pending> pending;
    std::vector<int> deferred_buckets;

    // wgrad of `cv` may start once everything enqueued on the stream so far (its dz: Ctx::dz) is done
    hipError_t queue(const ConvInfo& cv, const bf16_t* dz, const bf16_t* x) {
        if (c.data_only) return hipSuccess;      // no parameter asks for a gradient: dz feeds the data gradient only
        if (cv.dz_own_off) {
            pending.push_back({&cv, dz, x});
            return hipSuccess;
        }
        return run_conv_wgrad(c, cv, dz, x);
    }
    WgradParams task(const Pending& pd) const {
        WgradParams q = grouped_wgrad_params(*pd.cv, c.n, pd.dz, pd.x);
        q.dw = c.f32(c.p->wg_off) + pd.cv->wg_off;
        q.slab = c.f32(c.p->gslab_off) + pd.cv->gslab_off;
        return q;
    }
    // `slot`: the stage whose table / schedule cache the 128 x 64 launch uses
    hipError_t flush(int slot) {
        if (pending.empty()) return hipSuccess;
        vpd_plan* p = c.p;
        hipError_t r = hipSuccess;
        // persistent 128-wide tiles (conv_wgrad128_persistent_kernel) for every conv it takes: one launch per 18 problems
        // (a ResNet-50 stage has up to 19: two balanced launches)
        std::vector<Pending> rest;
        {
            std::vector<WgradParams> elig;
            std::vector<double> fl;
            for (const Pending& pd : pending) {
                const WgradParams q = task(pd);
                if (vpd_wgrad128_eligible(q)) { elig.push_back(q); fl.push_back(conv_flops(*pd.cv, c.n)); }
                else rest.push_back(pd);
            }
            const int total = (int)elig.size();
            const int nl = (total + 17) / 18;
            int at = 0;
            for (int l = 0; l < nl && r == hipSuccess; ++l) {
                const int cnt = (total - at + (nl - l) - 1) / (nl - l);
                double flops = 0.0;
                for (int i = 0; i < cnt; ++i) flops += fl[at + i];
                const int sl = (2 * slot + (l & 1)) & 7;
                if (l >= 2) {      // more than 36 problems (ResNet-101's layer3): the table slots are reused -- new shapes per launch
                    if (p->wg2_cache[sl]) { vpd_wgrad128_cache_free(p->wg2_cache[sl]); p->wg2_cache[sl] = nullptr; }
                }
                if (!p->wg2_cache[sl]) p->wg2_cache[sl] = vpd_wgrad128_cache_new();
                TimeScope ts(p, c.s, TC_WGRAD_STAGE, flops);
                r = vpd_launch_wgrad128_group(elig.data() + at, cnt, p->wg2_cache[sl], c.ws + p->wg2_tbl_off[sl], c.s);
                at += cnt;
            }
        }
        size_t done = 0;
        while (done < rest.size() && r == hipSuccess) {
            WgradParams qs[12];
            const int cnt = (int)std::min<size_t>(12, rest.size() - done);
            double flops = 0.0;
            // one launch of the 64 x 64 grouped kernel: one halo geometry (stage)
            int take = 0;
            for (int i = 0; i < cnt; ++i) {
                if (i > 0 && rest[done + i].cv->Hout != rest[done].cv->Hout) break;
                qs[take++] = task(rest[done + i]);
                flops += conv_flops(*rest[done + i].cv, c.n);
            }
            {
                TimeScope ts(p, c.s, TC_WGRAD_STAGE, flops);
                r = vpd_launch_wgrad_group(qs, take, c.s);
            }
            done += take;
        }
        pending.clear();
        return r;
    }
    int unpack_bucket(int b) {
        const vpd_plan* p = c.p;
        int nb = (int)p->bmap_unpack[b].size() / 2;
        if (c.data_only) nb = 0;      // nothing to hand over; the bucket's event is still recorded
        if (lazy) nb = b == 3 ? p->nstem_unpack_blocks : 0;      // the stem's row-tap packing is undone here either way
        if (nb > 0)
            LCHECK(vpd_launch_unpack_grads(plan_descs(p, c.ws), (int)p->descs.size(), plan_bmap_unpack(p, c.ws, b), nb,
                                           plan_wg(p, c.ws), grads, c.s));
        if (bucket_events && bucket_events[b]) LCHECK(hipEventRecord((hipEvent_t)bucket_events[b], c.s));
        return 0;
    }
    // End of a stage's backward (called after every block): launch the stage's grouped weight gradients and hand its
    // gradient bucket over -- except that layer4's (stage 3) wait for layer3's when wg_merge34: one launch then carries both
    // stages (their tasks fill the chip together where each stage alone leaves CUs idle), and bucket 0 follows it.
    int stage_end(int bi) {
        const vpd_plan* p = c.p;
        const BlockInfo& B = p->blocks[bi];
        const bool last_of_stage = bi == 0 || p->blocks[bi - 1].stage != B.stage;
        if (!last_of_stage) return 0;
        if (p->wg_group && p->wg_merge34 && B.stage == 3 && bi > 0) { deferred_buckets.push_back(3 - B.stage); return 0; }
        LCHECK(flush(B.stage));
        for (int b : deferred_buckets)
            if (unpack_bucket(b)) return -1;
        deferred_buckets.clear();
        if (bi > 0) return unpack_bucket(3 - B.stage);
        return 0;
    }
};

// One backward pass: the head, the blocks in reverse order, the stem.  d(out) of the current block is in G[gi]; a block
// leaves d(out) of the previous one in G[gi] (identity: accumulated onto it) or in G[(gi + 2) % 3] (down-sampling: gi moves).
struct Backward {
    const Ctx& c;
    float* grads;
    WgradQueue wq;
    bf16_t* G[3];
    int gi = 0;
    bool pool_pending = false;      // d(out) of the last block has not been written yet: d(pooled) is what there is
    std::vector<BlockRoute> routes;      // of every block, for this pass
    std::vector<char> bn2_sums_for;      // block bi's bn2 sums were taken by the next block's conv1 data gradient (BnSums)

    Backward(const Ctx& c_, float* grads_, void** bucket_events, bool lazy)
        : c(c_), grads(grads_), wq{c_, grads_, bucket_events, lazy},
          G{c_.b16(c_.p->G_off[0]), c_.b16(c_.p->G_off[1]), c_.b16(c_.p->G_off[2])}, bn2_sums_for(c_.p->blocks.size(), 0) {
        routes.reserve(c.p->blocks.size());
        for (const BlockInfo& B : c.p->blocks) routes.push_back(block_route(c, B));
    }

    const bf16_t* block_input(int bi) const { return bi == 0 ? c.b16(c.p->p0_off) : c.b16(c.p->blocks[bi - 1].out_off); }

    // scaled: d(loss)/d(pred) is the fused sum-MSE's and takes the plan's loss scale (vpd_backward); the caller's own d(loss)/d(emb)
    // of vpd_backward_ext is taken as it is
    int head(bool scaled = true) {
        vpd_plan* p = c.p;
        const int n = c.n;
        hipStream_t s = c.s;
        if (scaled) {
            if (p->scale_state)            // (fp16 training, dynamic scaler: vpd_plan_set_scale_state)
                LCHECK(vpd_launch_scale_by_state(c.f32(p->dpred_off), pred_numel(p, n), p->scale_state, s));
            else if (p->loss_scale != 1.f)      // (fp16 training: vpd_plan_set_loss_scale)
                LCHECK(vpd_launch_scale(c.f32(p->dpred_off), pred_numel(p, n), p->loss_scale, s));
        }
        const float* demb = c.f32(p->dpred_off);
        if (p->motion) {
            const MotionBufs mb = motion_bufs(c);
            for (int i = 2; i >= 0; --i) {      // the layer's parameters, then its input; the ReLU in front of it (layers 1, 2)
                LCHECK(linear_bwd_params(c, p->dec[i], mb.dact[i + 1], mb.act[i], grads));
                LCHECK(linear_bwd_data(c, p->dec[i], mb.dact[i + 1], mb.dact[i]));
                if (i > 0) LCHECK(vpd_launch_relu_mask(mb.dact[i], mb.act[i], (long)n * p->dec[i].in, s));
            }
            demb = mb.dact[0];
        }
        // (data_only comes through vpd_backward_ext, which refuses the motion head: the branch above is not taken)
        if (!c.data_only) LCHECK(linear_bwd_params(c, p->fc, demb, c.f32(p->pooled_off), grads));
        LCHECK(linear_bwd_data(c, p->fc, demb, c.f32(p->dpooled_off)));
        const StageInfo& S = p->stages[3];
        // BasicBlock students: the last block's BatchNorm backward produces d(out) from d(pooled) itself (run_bn_bwd)
        if (!p->bottleneck && !p->blocks.back().ds) pool_pending = true;
        else LCHECK(vpd_launch_avgpool_bwd(c.f32(p->dpooled_off), S.H, S.W, p->feat, n, G[gi], s));
        return 0;
    }

    // Conv `cv`'s data gradient dz -> dx, then the backward of the BatchNorm of `bc` (the conv whose output, after BatchNorm and
    // ReLU, is cv's input) into dzb.  bc's sums ride in cv's data gradient when that launch takes them (mask_off: bc's ReLU bit
    // map, vpd_plan_create's dgrad_sums); its BatchNorm launch then only finalizes and applies.
    int inner_bn_bwd(const ConvInfo& cv, const bf16_t* dz, bf16_t* dx, const ConvInfo& bc, size_t mask_off, bf16_t* dzb) {
        ConvDgrad d;
        d.dz = dz; d.dx = dx;
        if (mask_off && dgrad_takes_sums(c, cv, false)) {
            const BnSums sm{c.b16(bc.z_off), c.u8(mask_off), c.bn_rows(bc.bn)};
            d.sums = &sm;
            LCHECK(run_conv_dgrad(c, cv, d));
            LCHECK(run_bn_bwd_apply(c, bc, dx, dzb, grads, c.u8(mask_off)));
        } else {
            LCHECK(run_conv_dgrad(c, cv, d));
            BnBwd b;
            b.dy = dx; b.dz = dzb; b.relu_from_z = true;
            LCHECK(run_bn_bwd(c, bc, b, grads));
        }
        return 0;
    }

    // BasicBlock students only: block bi's conv1 data gradient produces d(out) of block bi-1 -- with a plain store when bi is a
    // down-sampling block (its merged stride-2 launch), accumulated onto the identity path otherwise.  It takes the sums of block
    // bi-1's bn2 (and of its 1x1 branch's BatchNorm, which sees the same g) when it can; that block's BatchNorm backward is then
    // finalize + apply only.  Returns the sums to pass, or null, and sets bn2_sums_for[bi - 1].
    const BnSums* prev_bn2_sums(int bi, BnSums& sm) {
        if (c.p->bottleneck || bi == 0) return nullptr;
        const BlockInfo& B = c.p->blocks[bi];
        const BlockInfo& Bp = c.p->blocks[bi - 1];
        const BlockRoute& Rp = routes[bi - 1];
        if (!Rp.relu_bits || (Bp.ds && !Rp.sums_pair)) return nullptr;
        if (!dgrad_takes_sums(c, B.c1, !B.ds, Bp.ds)) return nullptr;      // (a stride-2 launch takes no second BatchNorm)
        sm = BnSums{c.b16(Bp.c2.z_off), c.u8(Bp.mask_off), c.bn_rows(Bp.c2.bn), Bp.ds ? c.b16(Bp.cd.z_off) : nullptr,
                    Bp.ds ? c.bn_rows(Bp.cd.bn) : nullptr};
        bn2_sums_for[bi - 1] = true;
        return &sm;
    }

    // One block: the closing BatchNorm by its route; down the conv chain "queue the weight gradient, data gradient + the BatchNorm
    // in front of it"; then the block's input gradient, which is conv1's data gradient plus the identity path or the 1x1 branch.
    // BasicBlock and Bottleneck differ in the chain (c2, c1 / c3, c2, c1, and where the inner data gradients go) and in the routes
    // that block_route and prev_bn2_sums grant to BasicBlocks only.
    int block(int bi) {
        const vpd_plan* p = c.p;
        const BlockInfo& B = p->blocks[bi];
        const StageInfo& S = p->stages[B.stage];
        const BlockRoute& R = routes[bi];
        const bf16_t* xin = block_input(bi);
        bf16_t* dout = G[gi];
        bf16_t* dnew = G[(gi + 2) % 3];
        // the chain, closing conv first.  x: the conv's input; x_mask_off: that activation's ReLU bit map (0: none); dx: where the
        // data gradient w.r.t. x goes -- a temporary; conv1's is the block's and is handled below
        struct Link { const ConvInfo* cv; bf16_t* dz; const bf16_t* x; size_t x_mask_off; bf16_t* dx; };
        Link chain[3];
        int nlinks = 0;
        if (p->bottleneck) {
            chain[nlinks++] = Link{&B.c3, c.dz(B.c3, S.dz3_off), c.b16(B.a2_off), B.mask2_off, c.b16(p->T_off[0])};
            chain[nlinks++] = Link{&B.c2, c.dz(B.c2, S.dz2_off[bi & 1]), c.b16(B.a1_off), B.mask1_off, c.b16(p->T_off[1])};
        } else {
            chain[nlinks++] = Link{&B.c2, c.dz(B.c2, S.dz2_off[bi & 1]), c.b16(B.a1_off), B.mask1_off, G[(gi + 1) % 3]};
        }
        chain[nlinks++] = Link{&B.c1, c.dz(B.c1, S.dz1_off[bi & 1]), xin, /*x_mask_off*/ 0, /*dx: the block's, below*/ nullptr};
        const ConvInfo& last = *chain[0].cv;
        bf16_t* dzl = chain[0].dz;
        bf16_t* dz1 = chain[nlinks - 1].dz;
        bf16_t* dzd = B.ds ? c.dz(B.cd, S.dzd_off) : nullptr;

        // the closing BatchNorm (+ ReLU of the block output).  Identity blocks with the ReLU bit map: g = dout * mask is neither
        // written back nor re-read -- conv1's data gradient, which adds the identity path, masks dout itself (ConvParams::acc_mask);
        // every other route leaves g = dout * [out > 0] in dout
        const unsigned char* mbits = R.mask_in_dgrad ? c.u8(B.mask_off) : nullptr;
        bool branch_bn_done = false;      // the 1x1 branch's BatchNorm ran in the closing launch (same dy, same ReLU mask)
        if (bn2_sums_for[bi]) {
            // the next block's conv1 data gradient took the sums (a down-sampling block: both): one finalize + apply launch
            LCHECK(run_bn_bwd_apply(c, last, dout, dzl, grads, c.u8(B.mask_off), B.ds ? &B.cd : nullptr, dzd));
            branch_bn_done = B.ds;
        } else if (R.tail != TAIL_STORED) {
            const bool two = R.tail == TAIL_RECOMPUTED_BRANCH;
            LCHECK(run_tail_bwd(c, B, two, xin, dout, c.u8(B.mask_off), dzl, dzd, grads));
            branch_bn_done = two;
        } else if (R.bn_pair) {
            LCHECK(run_bn_bwd_pair(c, last, B.cd, dout, c.b16(B.out_off), dzl, dzd, grads));
            branch_bn_done = true;
        } else {
            BnBwd b;
            b.dy = dout; b.dz = dzl;
            if (mbits) b.mask_bits = mbits;
            else { b.act = c.b16(B.out_off); b.write_g = true; }
            if (pool_pending) b.dy_pooled = c.f32(p->dpooled_off);
            LCHECK(run_bn_bwd(c, last, b, grads));
            pool_pending = false;
        }
        // down the chain (layer3 / layer4 of the Bottleneck students, every BasicBlock: the sums of the inner BatchNorms ride in
        // the data gradients that produce their dy -- vpd_plan_create, dgrad_sums)
        for (int i = 0; i + 1 < nlinks; ++i) {
            const Link& L = chain[i];
            LCHECK(wq.queue(*L.cv, L.dz, L.x));
            if (inner_bn_bwd(*L.cv, L.dz, L.dx, *chain[i + 1].cv, L.x_mask_off, chain[i + 1].dz)) return -1;
        }
        // conv1, and the branch.  wgrad_pair: the 1x1 branch's weight gradient rides in conv1's launch, which then waits for the
        // branch's dz
        if (!R.wgrad_pair) LCHECK(wq.queue(B.c1, dz1, xin));
        ConvDgrad d1;
        d1.dz = dz1;
        BnSums sm;
        if (B.ds) {
            if (!branch_bn_done) {      // (dout holds g)
                BnBwd b;
                b.dy = dout; b.dz = dzd;
                LCHECK(run_bn_bwd(c, B.cd, b, grads));
            }
            if (R.wgrad_pair && !c.data_only) LCHECK(run_conv_wgrad_pair(c, B.c1, B.cd, dz1, dzd, xin));
            else LCHECK(wq.queue(B.cd, dzd, xin));
            d1.dx = dnew;
            if (R.dgrad_pair) {
                // one launch: the 1x1 branch's data gradient is extra K-steps of the even-even class
                d1.ds = &B.cd; d1.dzd = dzd; d1.sums = prev_bn2_sums(bi, sm);
                LCHECK(run_conv_dgrad(c, B.c1, d1));
            } else {
                LCHECK(run_conv_dgrad(c, B.c1, d1));      // writes every input pixel (3x3 covers all classes; 1x1 stride 1)
                ConvDgrad dd;
                dd.dz = dzd; dd.dx = dnew; dd.accumulate = true;      // adds onto the pixels the strided 1x1 reads
                LCHECK(run_conv_dgrad(c, B.cd, dd));
            }
            gi = (gi + 2) % 3;
        } else {
            // dout holds g (or, with the bit map, d(out) and the mask is applied here): identity path + conv path = d(out) of the
            // previous block
            d1.dx = dout; d1.accumulate = true; d1.acc_mask = mbits;
            if (mbits) d1.sums = prev_bn2_sums(bi, sm);
            LCHECK(run_conv_dgrad(c, B.c1, d1));
        }
        return wq.stage_end(bi);
    }

    int stem() {
        const vpd_plan* p = c.p;
        StemPoolBwdParams sb;
        memset(&sb, 0, sizeof sb);
        sb.dpool = G[gi]; sb.idx = c.u8(p->idx_off); sb.z = c.b16(p->z0_off);
        sb.mean = c.bn_mean(p->stem.bn); sb.rstd = c.bn_rstd(p->stem.bn);
        sb.scale = c.bn_scale(p->stem.bn); sb.shift = c.bn_shift(p->stem.bn);
        sb.g = c.b16(p->g0_off); sb.partials = c.stat_rows();
        sb.pooled = c.b16(p->p0_off); sb.ppad = 1;
        sb.gamma_p = c.params + p->stem.bn.w_off; sb.beta_p = c.params + p->stem.bn.b_off;
        sb.M = c.n * p->H0 * p->W0; sb.Hz = p->H0; sb.Wz = p->W0; sb.Ho = p->H1; sb.Wo = p->W1; sb.C = p->stem.Co;
        LCHECK(vpd_launch_stem_pool_bwd(sb, (float)sb.M, c.params + p->stem.bn.w_off, c.bn_dgamma(p->stem.bn, grads),
                                        c.bn_dbeta(p->stem.bn, grads), c.bn_coef(p->stem.bn), c.b16(p->dz0_off), c.s, c.frozen));
        LCHECK(wq.queue(p->stem, c.b16(p->dz0_off), c.b16(p->xin_off)));
        return wq.unpack_bucket(3);
    }
};

}  // namespace

// ---------------------------------------------------------------------------
extern "C" int vpd_pack_weights(vpd_plan_t* p, const float* params, const float* bn_running, void* workspace,
                                void* stream) {
    if (!p || !workspace || !params) return fail("null argument");
    if (p->bound_ws != workspace) return fail("workspace not initialised with vpd_plan_init_workspace");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    Ctx c{p, ws, s, params, 1};
    LCHECK(vpd_launch_pack_weights(plan_descs(p, ws), (int)p->descs.size(), plan_bmap_pack(p, ws), (int)p->bmap_pack.size() / 2,
                                   params, plan_arena(p, ws), s));
    if (bn_running)
        for (BnInfo* b : p->bns)
            LCHECK(vpd_launch_bn_fold(params + b->w_off, params + b->b_off, bn_running + b->rm_off,
                                      bn_running + b->rv_off, kBnEps, c.bn_escale(*b), c.bn_eshift(*b), b->C, s));
    return 0;
}

extern "C" int vpd_forward_eval(vpd_plan_t* p, const float* params, const float* x, int n, float* emb_out,
                                const float* target, float* loss_step, double* loss_accum, void* workspace,
                                void* stream) {
    if (check_call(p, workspace, n)) return -1;
    return run_eval_forward(p, params, x, n, emb_out, target, loss_step, loss_accum, (char*)workspace,
                            (hipStream_t)stream);
}

extern "C" int vpd_forward_train(vpd_plan_t* p, const float* params, float* bn_running, const float* x,
                                 const float* target, int n, float* emb_out, float* loss_step, double* loss_accum,
                                 void* workspace, void* stream) {
    if (check_call(p, workspace, n, 0)) return -1;
    if (!p->train) return fail("plan was created with train=0");
    if (p->bn_frozen && !bn_running) return fail("vpd_forward_train: a frozen BatchNorm (vpd_plan_set_bn_frozen) needs bn_running");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    p->fwd_bn_frozen = p->bn_frozen;      // the mode of THIS graph: its backward asks here, whatever the flag says by then
    if (n == 0) {      // empty shard: no crops, no statistics update, zero loss (the running buffers stay as they are)
        if (loss_step) HCHECK(hipMemsetAsync(loss_step, 0, sizeof(float), s));
        return 0;
    }
    Ctx c{p, ws, s, params, n};
    c.train = true; c.frozen = p->bn_frozen;
    p->fwd_had_x = x != nullptr;
    LCHECK(vpd_launch_zero_ranges(accumulator_zero_ranges(c), s));
    if (x) LCHECK(pack_input(c, x));
    // stem: conv -> batch stats -> BN+ReLU+maxpool
    ConvFwd f0;
    f0.x = c.b16(p->xin_off); f0.y = c.b16(p->z0_off); f0.stats = true;
    LCHECK(run_conv_fwd(c, p->stem, f0));
    LCHECK(run_bn_finalize(c, p->stem, bn_running));
    LCHECK(vpd_launch_stem_pool(stem_pool_params(c, c.bn_scale(p->stem.bn), c.bn_shift(p->stem.bn), c.u8(p->idx_off)), s));
    const bf16_t* cur = c.b16(p->p0_off);
    // BatchNorm -> ReLU of a conv's z into a padded activation, with the activation's ReLU bit map where the plan keeps one
    auto bn_relu = [&](const ConvInfo& cv, bf16_t* out, size_t mask_off) {
        BnFwd b;
        b.out = out; b.mask_out = mask_off ? c.u8(mask_off) : nullptr;
        return run_bn_fwd(c, cv, bn_running, b);
    };
    for (auto& B : p->blocks) {
        const BlockRoute R = block_route(c, B);
        bf16_t* a1 = c.b16(B.a1_off);
        bf16_t* outp = c.b16(B.out_off);
        // conv1 -- and the down-sampling 1x1 in the same launch (both read `cur`; statistics to their own rows)
        const AltConv alt{&B.cd, c.b16(B.cd.z_off), ConvEpilogue{}};
        LCHECK(run_conv_train(c, B.c1, cur, bn_running, R.conv_pair ? &alt : nullptr));
        LCHECK(bn_relu(B.c1, a1, B.mask1_off));
        const bf16_t* last_in = a1;
        if (p->bottleneck) {
            last_in = c.b16(B.a2_off);
            LCHECK(run_conv_train(c, B.c2, a1, bn_running));
            LCHECK(bn_relu(B.c2, c.b16(B.a2_off), B.mask2_off));
        }
        // the block's last conv, its BatchNorm + residual + ReLU (and the down-sampling branch's conv and BatchNorm)
        const ConvInfo& last = p->bottleneck ? B.c3 : B.c2;
        unsigned char* mbits = p->relu_bits ? c.u8(B.mask_off) : nullptr;
        if (R.tail != TAIL_STORED) {
            LCHECK(run_tail_fwd(c, B, R.tail == TAIL_RECOMPUTED_BRANCH, cur, outp, mbits, bn_running));
        } else {
            LCHECK(run_conv_train(c, last, last_in, bn_running));
            if (B.ds && !R.conv_pair) LCHECK(run_conv_train(c, B.cd, cur, bn_running));
            BnFwd b;
            b.out = outp; b.mask_out = mbits;
            if (B.ds) { b.res = c.b16(B.cd.z_off); b.res_cv = &B.cd; }
            else b.res = cur;
            LCHECK(run_bn_fwd(c, last, bn_running, b));
        }
        cur = outp;
    }
    return run_head(c, cur, emb_out, target, true, loss_step, loss_accum);
}

// loss.backward() for the graph of the preceding vpd_forward_train.  d_emb == null: from the fused sum-MSE's d(loss)/d(pred) in the
// workspace (vpd_backward); else from the caller's d(loss)/d(emb) (vpd_backward_ext), with d(loss)/d(x) into dx_nchw when given
namespace {
int run_backward(vpd_plan* p, const float* params, float* grads, int n, void** bucket_events, char* ws, hipStream_t s, bool lazy,
                 const float* d_emb, float* dx_nchw) {
    p->grads_in_scratch = lazy;
    // data gradients only (vpd_plan_set_param_grads(0), vpd_backward_ext): no weight-gradient launch, no slab sum, no unpack, no
    // head weight gradient; `grads` is not written -- the BatchNorm launches store dgamma / dbeta into the idle weight-gradient scratch
    const bool data_only = d_emb && !p->param_grads;
    if (n == 0) {      // empty shard: the gradient of a sum over no crops is zero; every bucket is "ready" at once
        // (lazy: the reducer sums the scratch ranges, and the optimizer step reads them there afterwards)
        if (!data_only) HCHECK(hipMemsetAsync(grads, 0, (size_t)p->nparam_padded * sizeof(float), s));
        if (lazy) HCHECK(hipMemsetAsync(ws + p->wg_off, 0, (size_t)p->wg_elems * sizeof(float), s));
        for (int b = 0; b < 4; ++b)
            if (bucket_events && bucket_events[b]) HCHECK(hipEventRecord((hipEvent_t)bucket_events[b], s));
        return 0;
    }
    Ctx c{p, ws, s, params, n};
    c.train = true; c.frozen = p->fwd_bn_frozen; c.data_only = data_only;
    if (d_emb) HCHECK(hipMemcpyAsync(c.f32(p->dpred_off), d_emb, (size_t)n * p->D * sizeof(float), hipMemcpyDeviceToDevice, s));
    // one launch zeroes the accumulator rows and every weight-gradient range the atomics kernel will add into
    ZeroRanges zr = accumulator_zero_ranges(c);
    if (!data_only) {
        for (auto& B : p->blocks) {
            wgrad_zero_range(c, B.c1, zr); wgrad_zero_range(c, B.c2, zr);
            if (p->bottleneck) wgrad_zero_range(c, B.c3, zr);
            if (B.ds) wgrad_zero_range(c, B.cd, zr);
        }
        wgrad_zero_range(c, p->stem, zr);
    }
    if (zr.count >= ZR_MAX) {      // too many ranges (Bottleneck nets: 30-100 1x1 convs): zero the whole scratch in one range
        const int k = p->fused_bn ? 2 : 1;
        zr.ptr[k] = c.f32(p->wg_off); zr.n4[k] = (long)(p->wg_elems + 3) / 4; zr.count = k + 1;
    }
    LCHECK(vpd_launch_zero_ranges(zr, s));

    Backward bw(c, grads, bucket_events, lazy);
    if (bw.head(!d_emb)) return -1;
    for (int bi = (int)p->blocks.size() - 1; bi >= 0; --bi)
        if (bw.block(bi)) return -1;
    if (bw.stem()) return -1;
    // the one data gradient training never needs: d(loss)/d(x) from the stem's dz (conv_stem_dgrad.hip)
    if (dx_nchw)
        LCHECK(vpd_launch_stem_dgrad(c.b16(p->dz0_off), params + p->stem.w_off, dx_nchw, n, p->c_in, p->H, p->W, s));
    return 0;
}
}  // namespace

extern "C" int vpd_backward(vpd_plan_t* p, const float* params, float* grads, int n, void** bucket_events,
                            void* workspace, void* stream) {
    if (check_call(p, workspace, n, 0)) return -1;
    if (!p->train) return fail("plan was created with train=0");
    const bool lazy = p->lazy_next;
    p->lazy_next = false;
    return run_backward(p, params, grads, n, bucket_events, (char*)workspace, (hipStream_t)stream, lazy, /*d_emb*/ nullptr,
                        /*dx_nchw*/ nullptr);
}

extern "C" int vpd_backward_ext(vpd_plan_t* p, const float* params, float* grads, const float* d_emb, int n, float* dx_nchw,
                                void** bucket_events, void* workspace, void* stream) {
    if (!p || !params || !grads || !d_emb || !workspace) return fail("vpd_backward_ext: null plan / params / grads / d_emb / workspace");
    if (!p->train) return fail("plan was created with train=0");
    if (p->motion) return fail("vpd_backward_ext: the plan has the motion head (d_emb is the gradient of the encoder's output)");
    if (n < 0 || n > p->max_batch) return fail("batch size outside 0..max_batch");
    if (p->bound_ws != workspace) return fail("workspace not initialised with vpd_plan_init_workspace");
    if (dx_nchw && (reinterpret_cast<size_t>(dx_nchw) & 7)) return fail("vpd_backward_ext: dx_nchw must be 8-byte aligned");
    if (dx_nchw && !p->fwd_had_x)
        return fail("vpd_backward_ext: dx_nchw needs a forward that took x (a batch staged by vpd_plan_stage_crops has no fp32 input)");
    p->lazy_next = false;      // lazy gradients belong to the fused step
    const bool lazy = false;
    return run_backward(p, params, grads, n, bucket_events, (char*)workspace, (hipStream_t)stream, lazy, d_emb, dx_nchw);
}

extern "C" int vpd_graph_capture_eval(vpd_plan_t* p, const float* params, const float* x, int n, float* emb_out,
                                      void* workspace, void* stream) {
    if (check_call(p, workspace, n)) return -1;
    hipStream_t s = (hipStream_t)stream;
    for (size_t i = 0; i < p->graphs.size(); ++i)
        if (p->graphs[i].n == n) {
            (void)hipGraphExecDestroy(p->graphs[i].e);
            (void)hipGraphDestroy(p->graphs[i].g);
            p->graphs.erase(p->graphs.begin() + i);
            break;
        }
    HCHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = run_eval_forward(p, params, x, n, emb_out, /*target*/ nullptr, /*loss_step*/ nullptr, /*loss_accum*/ nullptr,
                                    (char*)workspace, s);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(s, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return -1; }
    if (e != hipSuccess) return fail("hipStreamEndCapture", e);
    hipGraphExec_t ge = nullptr;
    e = hipGraphInstantiate(&ge, g, /*error node*/ nullptr, /*log buffer*/ nullptr, /*its size*/ 0);
    if (e != hipSuccess) { (void)hipGraphDestroy(g); return fail("hipGraphInstantiate", e); }
    p->graphs.push_back({n, g, ge});
    return 0;
}

extern "C" int vpd_graph_launch_eval(vpd_plan_t* p, int n, void* stream) {
    for (auto& g : p->graphs)
        if (g.n == n) {
            HCHECK(hipGraphLaunch(g.e, (hipStream_t)stream));
            return 0;
        }
    return fail("no captured eval graph for this batch size");
}
