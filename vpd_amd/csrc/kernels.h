// Host-side launcher declarations for the HIP kernels (internal to libvpdhip).
#pragma once
#include <string.h>

#include <vector>

#include "common.h"

struct BnApplyParams {
    const bf16_t* z;                    // dense [M][C]
    const float* scale; const float* shift;
    int res_kind;                       // 0 none, 1 padded activation, 2 dense z with rscale/rshift
    const bf16_t* res; int rHp, rWp, rpad;
    const float* rscale; const float* rshift;
    bf16_t* out; int oHp, oWp, opad;    // padded output
    int M, H, W, C, relu;
    unsigned char* mask_out;            // fused forward only: [M][C/8] bytes, bit j of byte (m, c8) = out[m][8*c8 + j] > 0, or null
    int xcd_tile_px;                    // fused forward only: pixel tile of the neighbouring 3x3 launches (vpd_bn_virtual_block) or 0
};

struct StemPoolParams {
    const bf16_t* z; int Hz, Wz;        // dense conv output
    const float* scale; const float* shift;
    bf16_t* out; int opad;              // padded pooled output
    unsigned char* idx;                 // dense argmax (train) or null
    int N, Ho, Wo, C;
};

struct BnBwdParams {
    const bf16_t* dy;                   // dense [M][C] gradient w.r.t. the BN(+ReLU) output
    bf16_t* dy_rw;                      // same buffer, written with g when write_g
    const bf16_t* z;                    // dense conv output saved by forward
    const bf16_t* act; int aHp, aWp, apad;   // padded post-ReLU activation (mask) or null
    const float* mean; const float* rstd;
    float* coef;                        // [3][C] scratch
    double* partials;                   // [VPD_STAT_ROWS][2][C] fp64 accumulator rows
    bf16_t* dz; int dzHp, dzWp, dzpad;  // output (padded or dense)
    int M, H, W, C, write_g, ppb;
    const float* mscale; const float* mshift;   // when act == null and these are set: ReLU mask = (mscale*z + mshift > 0)
    // fused backward only: the ReLU mask as ONE BIT per element ([M][C/8] bytes, written by the fused forward) instead of
    // the stored activation; g is then neither read back from nor written to dy (the consumer of the identity path masks
    // dy itself: ConvParams::acc_mask)
    const unsigned char* mask_bits;
    // fused backward with mask_bits only: dy does not exist yet -- it is the gradient of the global average pool, dy[b][y][x][c] =
    // bf16(dy_pooled[b][c] * dy_pool_scale) (avgpool_bwd_kernel's value).  The kernel computes it, uses it, and writes it to dy_rw
    // (unmasked: the identity path of the block adds onto it later) -- the avgpool_bwd launch in front of it is gone
    const float* dy_pooled; float dy_pool_scale;
    int xcd_tile_px;                    // bn_bwd_apply_fused_kernel only: as BnApplyParams::xcd_tile_px
};

struct StemPoolBwdParams {
    const bf16_t* dpool;                // dense [N][Ho][Wo][C]
    const unsigned char* idx;
    const bf16_t* z;                    // dense [N][Hz][Wz][C]
    const float* mean; const float* rstd; const float* scale; const float* shift;
    bf16_t* g;                          // unused (g is recomputed, never stored)
    double* partials;
    int M, Hz, Wz, Ho, Wo, C, ppb;
    int pass; const float* coef; bf16_t* dz;    // filled by the launcher
    // pooled post-ReLU activation (padded NHWC, border ppad) and the BN affine parameters: the backward sums are taken
    // over the POOLED positions (4x fewer than z pixels), where xhat of the arg-max pixel is (a - beta) / gamma
    const bf16_t* pooled; int ppad; const float* gamma_p; const float* beta_p;
};

struct PackDesc {                       // one convolution's weight tensors
    long long src_off;                  // fp32 OIHW master / grad offset (elements) in the flat buffers
    long long fwd_off;                  // bf16 [ntaps][Co][Kc] offset in the packed-weight arena
    long long dgr_off;                  // bf16 [kh*kw][Ci][Co] offset (dgrad layout) or -1
    long long wg_off;                   // fp32 [ntaps][Co][Kc] offset in the wgrad scratch
    int Co, Ci, kh, kw, Kc, ntaps, stem;   // stem: 1 = 7x7 row-tap packing; 2 = not a conv: plain range (AdamW only)
    long long numel;                    // stem == 2: length of the range at src_off
};
struct AdamHyper { float decay, omb1, b2, omb2, step_size, inv_sqrt_bc2, eps, gscale; };      // gscale: 1 / loss scale (fp16 training), else 1
// ... under a dynamic loss scaler (vpd_scale_state, include/vpd_hip.h): step_size, inv_sqrt_bc2 and gscale come from the device block
struct vpd_scale_state;
struct AdamHyperDyn { AdamHyper h; const vpd_scale_state* st; double lr, b1, b2; };
// What the two AdamW launchers take.  st == null: `step` (1-based) and `gscale` are the host's (adamw_kernel<AdamHyper>); else the
// device block decides and both are ignored (<AdamHyperDyn>)
struct AdamArgs { double lr, b1, b2, eps, wd; int step; float gscale; const vpd_scale_state* st; };
// Parameter groups (torch.optim.AdamW's param_groups): lr and weight decay per group, everything else shared.  The kernels find an
// element's group in the SEGMENT TABLE, a block of device memory (vpd_adam_groups_init, include/vpd_hip.h):
//   int nseg, ngroups, pad[2];  long long begin[nseg + 1];  int group[nseg];
// begin[0] = 0 < ... < begin[nseg] = numel; segment s is [begin[s], begin[s + 1]) of the flat buffers and belongs to group[s].
#define VPD_MAX_PARAM_GROUPS 16
inline size_t vpd_adam_table_bytes(int nseg) {
    return (16 + (size_t)(nseg + 1) * sizeof(long long) + (size_t)nseg * sizeof(int) + 15) & ~(size_t)15;
}
// ... AdamHyper with decay = (float)(1 - lr_g wd_g) and step_size = (float)(lr_g / bc1) per group (h.decay / h.step_size: unused; the
// slots behind the last group hold decay 1, step_size 0: a parameter that reached one would stay as it is)
struct AdamGroupHyper { AdamHyper h; const void* table; float decay[VPD_MAX_PARAM_GROUPS], step_size[VPD_MAX_PARAM_GROUPS]; };
// ... under a device block: every group's step_size is formed from its double lr and the block's applied-step count
struct AdamGroupHyperDyn { AdamGroupHyper g; const vpd_scale_state* st; double lr[VPD_MAX_PARAM_GROUPS], b1, b2; };
// What the two grouped launchers take (AdamArgs with lr[] / wd[] of `ngroups` groups and the table)
struct AdamGroupArgs { const void* table; const double* lr; const double* wd; int ngroups; double b1, b2, eps; int step; float gscale;
                       const vpd_scale_state* st; };
#define FR_MAX 96
struct FiniteRanges {                   // float ranges of any alignment and length (vpd_launch_check_finite)
    const float* ptr[FR_MAX];
    long n[FR_MAX];
    int count;
};

hipError_t vpd_launch_conv(const ConvParams& p, hipStream_t stream);
hipError_t vpd_launch_scale(float* x, long n, float s, hipStream_t stream);      // head.hip: x *= s (the loss scale on d(loss)/d(pred))
// conv_stream.hip: persistent streaming kernel for 1x1 convolutions with <= 256 input channels on many pixels
bool vpd_conv1x1_stream_eligible(const ConvParams& p);
hipError_t vpd_launch_conv1x1_stream(const ConvParams& p, hipStream_t stream);
void vpd_conv1x1_stream_grid(const ConvParams& p, int* bm, int* bn, int* lanes);      // (reporting: its tile and pixel lanes)
int vpd_conv_kernel_class(const ConvParams& p);      // 0..6, see conv_igemm.hip
bool vpd_conv_takes_bn_sums(const ConvParams& p);      // epilogue can take the consuming BatchNorm's backward sums (bst_z)
// What vpd_launch_conv does with `p` on the current device; the launcher branches on this very struct (conv_igemm.hip)
struct ConvDispatch {
    int kclass;             // vpd_conv_kernel_class
    int pws;                // classes 1, 2, 3, 6: conv3x3_pws_kernel (persistent blocks) instead of conv3x3_ws_kernel
    int geo;                // ... its compile-time-geometry instantiation: the image width, or 0
    int interior;           // ... with the interior loaders (HaloGeom::interior)
    int c64x2;              // class 0: the two-group inference twin conv3x3_c64x2_persistent_kernel
    int ws1x1, stream1x1;   // class 4: conv1x1_ws_kernel (ring GEMM) / conv1x1_stream_kernel
    int halo;               // class 4: the legacy conv3x3_halo_kernel
    int bm, bn;             // tile (pixels x channels)
    int mode;               // conv_ep_mode
    int tiles_per_block;    // pixel tiles the busiest block walks
};
ConvDispatch vpd_conv_dispatch(const ConvParams& p);
// pixels per tile when `p` runs on conv3x3_pws_kernel with its XCD-affine tile order (pixel tile t on XCD t % 8), else 0
int vpd_conv_xcd_tile_px(const ConvParams& p);
hipError_t vpd_launch_wgrad_reduce(const WgradParams& p, hipStream_t stream);   // slab sum of a deferred halo wgrad
extern "C" int vpd_conv_bm(int M, int Co);
hipError_t vpd_launch_wgrad(const WgradParams& p, hipStream_t stream);
size_t vpd_wgrad_slab_bytes();
// grouped (per-stage, deferred) weight gradients: see WgGroup in conv_wgrad.hip
bool vpd_wgrad_group_eligible(const WgradParams& p);
size_t vpd_wgrad_group_slab_floats(int M, int Co, int Kc, int ntaps = 9);
hipError_t vpd_launch_wgrad_group(const WgradParams* ps, int n, hipStream_t stream);
bool vpd_wgrad_overwrites(const WgradParams& p);
// host only, by the launchers' own decision code (conv_wgrad.hip).  vpd_wgrad_dispatch: what vpd_launch_wgrad does with p, out9 =
// {kernel: 0 atomics / 1 stem / 2 halo 3x3 / 3 halo 1x1, pass instantiation, ring stages, TR, multi, NHP, ksplit, cpb, grid.x}; false
// where it refuses p.  vpd_wgrad_group_dispatch: what vpd_launch_wgrad_group does with ps[0..n), head4 = {pass instantiation,
// tasks, grid, halo passes}, per3 = {ksplit, cpb, tiles} per problem; 0, or -1 n outside 1..vpd_wgrad_group_max(), 1 a plane the
// halo tiling does not take, 2 pass counts differ.
bool vpd_wgrad_dispatch(const WgradParams& p, int* out9);
int vpd_wgrad_group_dispatch(const WgradParams* ps, int n, int* head4, int* per3);
int vpd_wgrad_group_max();
// A down-sampling BasicBlock's 3x3 stride-2 conv1 (p3) and its 1x1 stride-2 branch (p1, prefer_halo_1x1 set) in ONE halo launch: the
// branch rides as a tenth tap on conv1's staged halo (conv_wgrad_halo_pair_kernel; VPD_WGRAD_DS_RIDE=0: never).  _ok: both take the
// halo path and share input, shapes and split.  The launch leaves both slabs unsummed when p3.defer_reduce; _reduce sums both in one
// launch.  hipErrorInvalidValue when the pair does not qualify or its LDS layout is over 160 KB.
bool vpd_wgrad_pair_ok(const WgradParams& p3, const WgradParams& p1);
hipError_t vpd_launch_wgrad_pair(const WgradParams& p3, const WgradParams& p1, hipStream_t stream);
hipError_t vpd_launch_wgrad_pair_reduce(const WgradParams& p3, const WgradParams& p1, hipStream_t stream);
int vpd_wgrad_pair_lds_query(int H, int W, int ns, long long* bytes);
// 128 x 64 tiles, persistent blocks, host-built schedule (conv_wgrad128_persistent_kernel in conv_wgrad.hip)
bool vpd_wgrad128_eligible(const WgradParams& p);
size_t vpd_wgrad128_table_bytes();
void* vpd_wgrad128_cache_new();
void vpd_wgrad128_cache_free(void* cache);
hipError_t vpd_launch_wgrad128_group(const WgradParams* ps, int n, void* cache, void* dev_table, hipStream_t stream);
bool vpd_wgrad_halo_shape_ok(int Hout, int Wout, int stride = 1, int Hin = 0, int Win = 0);

// frozen (vpd_launch_bn_finalize, vpd_launch_bn_bwd, vpd_launch_stem_pool_bwd): the BatchNorm runs on its running statistics --
// forward: mean / rstd from rm / rv, which are not written; backward: c2 = c3 = 0
hipError_t vpd_launch_bn_finalize(double* partials, int T, int C, float count, const float* gamma,
                                  const float* beta, float* rm, float* rv, float momentum, float eps,
                                  float* mean, float* rstd, float* scale, float* shift, hipStream_t s, bool frozen = false);
hipError_t vpd_launch_bn_fold(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                              float* scale, float* shift, int C, hipStream_t s);
hipError_t vpd_launch_bn_apply(const BnApplyParams& p, hipStream_t s);
hipError_t vpd_launch_stem_pool(const StemPoolParams& p, hipStream_t s);
int vpd_bn_bwd_blocks(int M, int C, int* ppb_out);
hipError_t vpd_launch_bn_bwd(const BnBwdParams& p, float count, const float* gamma, float* dgamma, float* dbeta,
                             hipStream_t s, bool frozen = false);
hipError_t vpd_launch_stem_pool_bwd(const StemPoolBwdParams& p, float count, const float* gamma, float* dgamma,
                                    float* dbeta, float* coef, bf16_t* dz, hipStream_t s, bool frozen = false);

// fused BatchNorm passes (bn.hip, conv_stream.hip).  A launch serves one BatchNorm or two (a down-sampling block's own and its 1x1
// branch's: s[1], absent when its rows are null); what the kernels take once -- count, frozen, the barrier words -- the launch owns.
// rows: per-BatchNorm accumulator rows [VPD_FUSED_ROWS][2][C] of doubles, zeroed by the caller
struct BnFwdSide {
    double* rows; const float* gamma; const float* beta; float* rm; float* rv;
    float* mean; float* rstd; float* scale; float* shift;
};
struct BnFusedFwd {
    BnFwdSide s[2];
    float count, momentum, eps;
    // frozen BatchNorm: mean = rm, rstd = 1 / sqrt(rv + eps) (every side; rm / rv are then required, read and left unwritten);
    // mean / rstd / scale / shift are stored as always, so the backward's masks and xhat see what the forward used
    int frozen;
};
// z / mean / rstd / dz: the bn.hip launchers take s[0]'s from their BnBwdParams (a kernel argument) and read these for s[1] only, dz in
// the same padded geometry; the Bottleneck-tail launchers recompute z and read mean / rstd / dz of every side
struct BnBwdSide {
    double* rows; const float* gamma; float* dgamma; float* dbeta;
    const bf16_t* z; const float* mean; const float* rstd; bf16_t* dz;
};
struct BnFusedBwd {
    BnBwdSide s[2];
    float count;
    int frozen;                                 // the forward was frozen: dz = gamma rstd g (the batch-mean terms drop out), dgamma / dbeta unchanged
    void* sync; unsigned* err;                  // launches with a grid barrier: VPD_GRID_SYNC_BYTES, zeroed; sticky time-out counter
};
#define VPD_GRID_SYNC_BYTES (18 * 128)
hipError_t vpd_launch_bn_fwd_fused(const BnApplyParams& p, const BnFusedFwd& f, hipStream_t s);
// conv_stream.hip: a Bottleneck's closing 1x1 convolution with its train-mode BatchNorm, the convolution recomputed instead of
// written and read back, one pass per launch
enum BnTailPass {
    BN_TAIL_STATS = 0,          // statistics of z = conv(x) into p.stats (VPD_FUSED_ROWS rows), nothing stored
    BN_TAIL_FWD = 1,            // out = relu(BatchNorm(z) + p.res) into p.y (padded) + ReLU bit map; finalizes fwd's rows
    BN_TAIL_BWD_SUMS = 2,       // sums of the BatchNorm backward (g = p.y * p.acc_mask; p.y dense d(out)) into bwd's rows
    BN_TAIL_BWD_APPLY = 3,      // dz = A g + B z + D into each side's dz (padded by dzpad); dgamma / dbeta
};
struct BnTailLaunch {
    BnTailPass pass;
    const BnFusedFwd* fwd; unsigned char* mask_out;      // BN_TAIL_FWD (mask_out [M][Co / 8] may be null)
    const BnFusedBwd* bwd; int dzpad;                    // BN_TAIL_BWD_*
};
bool vpd_conv1x1_bn_eligible(const ConvParams& p);
// ... of a down-sampling Bottleneck whose closing 1x1 conv (p.x, p.w) and 1x1 branch (p.x2, p.w2) both have 64 input channels, stride 1
bool vpd_conv1x1_bn2_eligible(const ConvParams& p);
hipError_t vpd_launch_conv1x1_bn(const ConvParams& p, const BnTailLaunch& t, hipStream_t stream);
hipError_t vpd_launch_conv1x1_bn2(const ConvParams& p, const BnTailLaunch& t, hipStream_t stream);      // (no BN_TAIL_STATS: two launches of the above)
// (reporting) the grid of those launches for an eligible p: {pixel lanes, channel tiles, pixel tiles of the busiest block, ring depth}
void vpd_conv1x1_bn_grid(const ConvParams& p, bool two, int out4[4]);
bool vpd_bn_bwd_fused_ok(int M, int C, bool mask_act, bool write_g);
// what both fused backward launchers derive from (M, C) on this device: blocks, pixels per block, pixel iterations per thread, which
// of g / z (/ the second z) stay in LDS across the grid barrier, dynamic LDS bytes (nt = 2: one BatchNorm, 3: the pair kernel)
struct BnBwdFusedGeom { int G, ppb, iters, keep[3]; size_t lds; };
BnBwdFusedGeom vpd_bn_bwd_fused_geom(int M, int C, int nt);
hipError_t vpd_launch_bn_bwd_fused(const BnBwdParams& p, const BnFusedBwd& f, hipStream_t s);
// BatchNorm backward whose sums (sum g, sum g * z) the producing data gradient's epilogue has already added to the rows
// (ConvParams::bst_z): finalize + apply in one launch, no reduction pass, no grid barrier.  p.mask_bits is required.
// f.s[1] present: a second BatchNorm fed with the same masked gradient
hipError_t vpd_launch_bn_bwd_apply_fused(const BnBwdParams& p, const BnFusedBwd& f, hipStream_t s);
// two BatchNorm backwards sharing dy and the ReLU mask (a down-sampling block's conv2 BN + its 1x1 branch's BN) in one launch
bool vpd_bn_bwd_fused2_ok(int M, int C);
hipError_t vpd_launch_bn_bwd_fused2(const BnBwdParams& p, const BnFusedBwd& f, hipStream_t s);

// ---- geometry constructors: the descriptors above as the step (step.hip) and the operator entry points (ops.hip) fill them ----
// dense z [n][H][W][C] -> BatchNorm (+ res, ReLU) -> out padded by 1; res: padded by 1 (res_kind 1) or dense like z (2)
inline BnApplyParams vpd_bn_apply_params(const bf16_t* z, int res_kind, const bf16_t* res, bf16_t* out, int n, int H, int W, int C,
                                         int relu) {
    BnApplyParams a;
    memset(&a, 0, sizeof a);
    a.z = z;
    a.res_kind = res_kind; a.res = res; a.rHp = H + 2; a.rWp = W + 2; a.rpad = 1;
    a.out = out; a.oHp = H + 2; a.oWp = W + 2; a.opad = 1;
    a.M = n * H * W; a.H = H; a.W = W; a.C = C; a.relu = relu;
    return a;
}
// dense dy [n][H][W][C] -> BatchNorm backward -> dz padded by dzpad
inline BnBwdParams vpd_bn_bwd_params(const bf16_t* dy, const bf16_t* z, const float* mean, const float* rstd, bf16_t* dz, int dzpad,
                                     int n, int H, int W, int C) {
    BnBwdParams b;
    memset(&b, 0, sizeof b);
    b.dy = dy; b.z = z; b.mean = mean; b.rstd = rstd;
    b.dz = dz; b.dzHp = H + 2 * dzpad; b.dzWp = W + 2 * dzpad; b.dzpad = dzpad;
    b.M = n * H * W; b.H = H; b.W = W; b.C = C;
    return b;
}
// ... whose dy may be rewritten with g, its ReLU mask the stored activation (padded by 1) or null
inline void vpd_bn_bwd_set_act(BnBwdParams& b, bf16_t* dy_rw, const bf16_t* act) {
    b.dy_rw = dy_rw; b.act = act; b.aHp = b.H + 2; b.aWp = b.W + 2; b.apad = 1;
}
// padded x -> Hs x Ws output pixels per image through `taps`, every pixel of a dense y [n][Hs][Ws][Co] (y itself: the caller's)
inline ConvParams vpd_conv_params(const bf16_t* x, int xHp, int xWp, int xC, const bf16_t* w, int n, int Hs, int Ws, int istr, int Kc,
                                  int Co, const TapSet& taps) {
    ConvParams q;
    memset(&q, 0, sizeof q);
    q.x = x; q.xHp = xHp; q.xWp = xWp; q.xC = xC; q.w = w;
    q.yHp = Hs; q.yWp = Ws; q.yC = Co; q.ypad = 0;
    q.N = n; q.Hs = Hs; q.Ws = Ws; q.osub = 1; q.istr = istr;
    q.Kc = Kc; q.Co = Co; q.M = n * Hs * Ws;
    q.taps = taps;
    return q;
}
inline void vpd_conv_set_y(ConvParams& q, bf16_t* y, int ypad) {      // y padded by ypad
    q.y = y; q.yHp = q.Hs + 2 * ypad; q.yWp = q.Ws + 2 * ypad; q.ypad = ypad;
}
inline void vpd_conv_set_res(ConvParams& q, const bf16_t* res) {      // residual shaped like the output, padded by 1
    q.res = res; q.rHp = q.Hs + 2; q.rWp = q.Ws + 2; q.rC = q.Co; q.rpad = 1;
}
inline void vpd_conv_set_bn_rows(ConvParams& q, double* rows) {       // statistics into a fused BatchNorm's own rows
    q.stats = rows; q.stat_rows = VPD_FUSED_ROWS;
}
inline TapSet vpd_taps_1x1() {      // one tap at padded offset (1, 1): a 1x1 convolution of an input with a border of 1
    TapSet t;
    t.nr = 1; t.nc = 1; t.dy0 = 1; t.dys = 1; t.dx0 = 1; t.dxs = 1; t.w0 = 0; t.wrs = 1; t.wcs = 1;
    return t;
}
// A 1x1 stride-1 weight-gradient problem with fewer than 128 output but a multiple of 128 input channels (layer1's 256 -> 64), restated
// for the 128-wide grouped launch: operands swapped, result stored transposed (WgradParams::transposed), so dw keeps the
// convolution's own [Co][Ci] layout.  Input and output planes are the same size at stride 1.  false: q is not such a problem (unchanged).
inline bool vpd_wgrad_swap_1x1(WgradParams& q) {
    if (!(q.taps.nr == 1 && q.taps.nc == 1 && q.istr == 1 && q.Co % 128 != 0 && q.xC % 128 == 0) || q.transposed) return false;
    const bf16_t* dz = q.dz;
    const int co = q.Co, ci = q.xC;
    q.dz = q.x; q.dzC = ci; q.x = dz; q.xC = co; q.Co = ci; q.Kc = co; q.transposed = 1;
    return true;
}
// a Bottleneck's closing 1x1 convolution (the tail launchers above): x padded by 1 with Kc channels, H x W output pixels
inline ConvParams vpd_conv1x1_params(const bf16_t* x, const bf16_t* w, int n, int H, int W, int istr, int Kc, int Co) {
    return vpd_conv_params(x, H * istr + 2, W * istr + 2, Kc, w, n, H, W, istr, Kc, Co, vpd_taps_1x1());
}

// conv_stem_dgrad.hip: the stem convolution's data gradient, dz dense NHWC [N][H/2][W/2][64] -> dx fp32 NCHW [N][Cin][H][W]
// (H, W even and >= 32, Cin <= 8; w_oihw: the fp32 master weight, rounded to the element type in the kernel)
hipError_t vpd_launch_stem_dgrad(const bf16_t* dz, const float* w_oihw, float* dx_nchw, int N, int Cin, int H, int W,
                                 hipStream_t s);

// head.hip
hipError_t vpd_launch_avgpool(const bf16_t* act, int Hp, int Wp, int pad, int H, int W, int C, int N, float* pooled,
                              hipStream_t s);
hipError_t vpd_launch_avgpool_bwd(const float* dpooled, int H, int W, int C, int N, bf16_t* dact, hipStream_t s);
// Y[M][N] (=|+=) op(A)[M][K] * op(B)[K][N] (+ bias[N]) (relu?)   fp32, row-major
//   ta: A is stored [K][M];  tb: B is stored [N][K]
hipError_t vpd_launch_sgemm(const float* A, const float* B, float* Y, const float* bias, int M, int N, int K, int ta,
                            int tb, int relu, hipStream_t s);
hipError_t vpd_launch_colsum(const float* A, int M, int N, float* out, hipStream_t s);
hipError_t vpd_launch_relu_mask(float* d, const float* act, long n, hipStream_t s);
hipError_t vpd_launch_mse(const float* e, const float* t, long n, float* de, float* loss_step, double* loss_accum,
                          hipStream_t s);

// optim.hip
hipError_t vpd_launch_pack_input(const float* x, int N, int C, int H, int W, bf16_t* out, int Hp, int Wp, int pad,
                                 int Cp, hipStream_t s);
hipError_t vpd_launch_pack_weights(const PackDesc* d_descs, int ndesc, const int* d_blockmap, int nblocks,
                                   const float* master, bf16_t* arena, hipStream_t s);
hipError_t vpd_launch_adamw_pack(const PackDesc* d_descs, const int* d_blockmap, int nblocks, float* p, const float* g,
                                 float* m, float* v, bf16_t* arena, const AdamArgs& a, hipStream_t s,
                                 const float* wg = nullptr);      // wg: conv gradients still in the scratch
hipError_t vpd_launch_unpack_grads(const PackDesc* d_descs, int ndesc, const int* d_blockmap, int nblocks,
                                   const float* wg, float* grads, hipStream_t s);
hipError_t vpd_launch_adamw(float* p, const float* g, float* m, float* v, long n, const AdamArgs& a, hipStream_t s);
// the same two launches with parameter groups: the grouped instantiations of the same kernels (the ungrouped ones are untouched)
hipError_t vpd_launch_adamw_pack_groups(const PackDesc* d_descs, const int* d_blockmap, int nblocks, float* p, const float* g,
                                        float* m, float* v, bf16_t* arena, const AdamGroupArgs& a, hipStream_t s,
                                        const float* wg = nullptr);
hipError_t vpd_launch_adamw_groups(float* p, const float* g, float* m, float* v, long n, const AdamGroupArgs& a, hipStream_t s);
// dynamic loss scaling (vpd_scale_state): the two AdamW launches above reading scale / applied steps / the non-finite word from
// the device block (AdamArgs::st), the inf / NaN search, the update rule; head.hip: d(loss)/d(pred) x the block's scale
hipError_t vpd_launch_check_finite(const FiniteRanges& r, vpd_scale_state* st, hipStream_t s);
hipError_t vpd_launch_scale_update(vpd_scale_state* st, float growth, float backoff, int interval, hipStream_t s);
// gradient-norm clipping (vpd_clip_state): one launch of the sum-of-squares pass over up to FR_MAX ranges -- `grid` blocks (from
// vpd_grad_sqsum_grid: 0 = nothing to read, nothing launched), block b stores its double at partials[b] -- and the one-block
// kernel that sums the first `used` slots behind the caller's block and writes norm, coefficient, statistics and clip->eff
struct vpd_clip_state;
#define CLIP_SLOTS 8192                 // doubles behind the struct: 2048 per launch, up to 4 launches at the full grid
int vpd_grad_sqsum_grid(const long* n, int count, int cap);      // (the grid of every streaming range kernel: count lengths)
hipError_t vpd_launch_grad_sqsum(const FiniteRanges& r, int grid, double* partials, hipStream_t s);
hipError_t vpd_launch_clip_finalize(vpd_clip_state* clip, int used, double max_norm, vpd_scale_state* src, float host_scale,
                                    hipStream_t s);
hipError_t vpd_launch_scale_by_state(float* x, long n, const vpd_scale_state* st, hipStream_t stream);

// exponential moving average of the weights (vpd_ema_update): float ranges of any alignment and length, passed by value
#define EMA_MAX 4
struct EmaRanges {
    const float* src[EMA_MAX];
    float* dst[EMA_MAX];
    long n[EMA_MAX];
    int count;
};
hipError_t vpd_launch_ema_update(const EmaRanges& r, double decay, int warmup, int t, int t0, const vpd_scale_state* st,
                                 hipStream_t s);

// gradient accumulation (vpd_op_grad_accumulate, vpd_plan_grad_accumulate): dst[j] = add ? dst[j] + src[j] : src[j] over up to GA_MAX
// pairs of float ranges of any alignment and length per launch, passed by value; the store mode never reads dst
#define GA_MAX 64
struct AccumRanges {
    float* dst[GA_MAX];
    const float* src[GA_MAX];
    long n[GA_MAX];
    int count;
};
hipError_t vpd_launch_grad_accum(const AccumRanges& r, bool add, hipStream_t s);

#define ZR_MAX 16
struct ZeroRanges {                    // 16-byte aligned ranges, lengths in float4
    float* ptr[ZR_MAX];
    long n4[ZR_MAX];
    int count;
};
hipError_t vpd_launch_zero_ranges(const ZeroRanges& z, hipStream_t s);
// conv_wgrad.hip: the slab sums of up to vpd_wgrad_reduce_max() problems in one launch (wg_launch_reduce from flat arguments)
int vpd_wgrad_reduce_max();
hipError_t vpd_launch_wgrad_reduce(int nprob, const float* const* slabs, float* const* dws, const long long* nfloats,
                                   const int* ksplits, hipStream_t stream);

// augment.hip (declared with the public vpd_aug_params of include/vpd_hip.h)
struct vpd_aug_params;
hipError_t vpd_launch_augment(const unsigned char* rgb, const unsigned char* flow, const unsigned char* mask,
                              const float* noise, const vpd_aug_params* params, int N, int H, int W, int out_dim,
                              const float* mean_std6, float noise_sd, float* out_nchw, bf16_t* xin, int xHp, int xWp,
                              int xpad, float* cmean_scratch, hipStream_t s);
hipError_t vpd_launch_views(const unsigned char* rgb, const unsigned char* flow, int F, int K, int H, int W,
                            const float* mean_std6, bf16_t* xin, int xHp, int xWp, int xpad, hipStream_t s);
hipError_t vpd_launch_views_jitter(const unsigned char* rgb, const unsigned char* flow, const vpd_aug_params* params, int F,
                                   int J, int flip, int H, int W, const float* mean_std6, float* out_nchw, bf16_t* xin,
                                   int xHp, int xWp, int xpad, float* cmean_scratch, hipStream_t s);
