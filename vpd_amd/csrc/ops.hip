// Single-operator entry points of include/vpd_hip.h for the parity tests: one launcher each, its descriptors built from flat
// arguments by the constructors the step uses (kernels.h).  No plan is involved; fail() / LCHECK are plan.hip's.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "plan.h"

// frozen BatchNorm for the BatchNorm entry points below (vpd_op_set_bn_frozen): process-wide, read by them alone -- no plan looks here
static int g_op_bn_frozen = 0;
extern "C" int vpd_op_set_bn_frozen(int on) { g_op_bn_frozen = on != 0; return 0; }

extern "C" int vpd_op_conv_bm(int M, int Co) { return vpd_conv_bm(M, Co); }
extern "C" size_t vpd_op_wgrad_slab_bytes(void) { return vpd_wgrad_slab_bytes(); }

static TapSet tapset_from(const int* t) {
    TapSet ts;
    ts.nr = t[0]; ts.nc = t[1]; ts.dy0 = t[2]; ts.dys = t[3]; ts.dx0 = t[4]; ts.dxs = t[5];
    ts.w0 = t[6]; ts.wrs = t[7]; ts.wcs = t[8];
    return ts;
}
// vpd_conv_params with the output tensor's own geometry (a dense y is the constructor's)
static ConvParams op_conv_params(const void* x, const void* w, void* y, int n, int xHp, int xWp, int xC, int yHp, int yWp, int yC,
                                 int ypad, int Hs, int Ws, int istr, int Kc, int Co, const int* tapset9) {
    ConvParams q = vpd_conv_params((const bf16_t*)x, xHp, xWp, xC, (const bf16_t*)w, n, Hs, Ws, istr, Kc, Co, tapset_from(tapset9));
    q.y = (bf16_t*)y; q.yHp = yHp; q.yWp = yWp; q.yC = yC; q.ypad = ypad;
    return q;
}
// one BatchNorm of a fused launch from flat arguments
static BnFwdSide op_fwd_side(const double* rows, const float* gamma, const float* beta, float* rm, float* rv, float* mean, float* rstd,
                             float* scale, float* shift) {
    return BnFwdSide{const_cast<double*>(rows), gamma, beta, rm, rv, mean, rstd, scale, shift};
}
static BnBwdSide op_bwd_side(const double* rows, const float* gamma, float* dgamma, float* dbeta, const void* z, const float* mean,
                             const float* rstd, void* dz) {
    return BnBwdSide{const_cast<double*>(rows), gamma, dgamma, dbeta, (const bf16_t*)z, mean, rstd, (bf16_t*)dz};
}
// the launch of one BatchNorm over M pixels under the hook's mode; a second side is the caller's to add
static BnFusedFwd op_fused_fwd(const BnFwdSide& s0, int M, float momentum, float eps) {
    BnFusedFwd f;
    memset(&f, 0, sizeof f);
    f.s[0] = s0; f.count = (float)M; f.momentum = momentum; f.eps = eps; f.frozen = g_op_bn_frozen;
    return f;
}
static BnFusedBwd op_fused_bwd(const BnBwdSide& s0, int M, void* sync = nullptr, unsigned* err = nullptr) {
    BnFusedBwd f;
    memset(&f, 0, sizeof f);
    f.s[0] = s0; f.count = (float)M; f.frozen = g_op_bn_frozen; f.sync = sync; f.err = err;
    return f;
}

extern "C" int vpd_op_conv2d(const void* x, const void* w, void* y, double* stats, int n, int xHp, int xWp, int xC,
                             int yHp, int yWp, int yC, int ypad, int Hs, int Ws, int osub, int oph, int opw, int istr,
                             int Kc, int Co, const int* tapset9, int accumulate, void* stream) {
    ConvParams q = op_conv_params(x, w, y, n, xHp, xWp, xC, yHp, yWp, yC, ypad, Hs, Ws, istr, Kc, Co, tapset9);
    q.stats = stats; q.osub = osub; q.oph = oph; q.opw = opw; q.accumulate = accumulate;
    if (q.taps.nr < 1 || q.taps.nc < 1) return fail("empty tap set");
    LCHECK(vpd_launch_conv(q, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_conv2d_ep(const void* x, const void* w, void* y, int n, int xHp, int xWp, int xC, int yHp, int yWp,
                                int yC, int ypad, int Hs, int Ws, int istr, int Kc, int Co, const int* tapset9,
                                const float* ep_scale, const float* ep_shift, const void* res_padded, int ep_relu,
                                int accumulate, const unsigned char* acc_mask, void* stream) {
    if ((ep_scale == nullptr) != (ep_shift == nullptr)) return fail("ep_scale and ep_shift come together");
    if (ep_scale && accumulate) return fail("eval epilogue or accumulate, not both");
    if (res_padded && !ep_scale) return fail("a residual needs the eval epilogue");
    if (acc_mask && (!accumulate || ypad != 0 || yC != Co || yHp != Hs || yWp != Ws)) return fail("acc_mask: accumulate onto a dense y");
    ConvParams q = op_conv_params(x, w, y, n, xHp, xWp, xC, yHp, yWp, yC, ypad, Hs, Ws, istr, Kc, Co, tapset9);
    q.accumulate = accumulate; q.acc_mask = acc_mask;
    q.ep_scale = ep_scale; q.ep_shift = ep_shift; q.ep_relu = ep_relu;
    if (res_padded) vpd_conv_set_res(q, (const bf16_t*)res_padded);
    if (q.taps.nr < 1 || q.taps.nc < 1) return fail("empty tap set");
    LCHECK(vpd_launch_conv(q, (hipStream_t)stream));
    return 0;
}

static int op_conv2d_bnsums(const void* x, const void* w, void* y, const void* bst_z, const unsigned char* bst_mask, double* rows,
                            const void* bst_z2, double* rows2, int n, int xHp, int xWp, int xC, int Hs, int Ws, int Kc, int Co,
                            const int* tapset9, int accumulate, void* stream) {
    if (!x || !w || !y || !bst_z || !bst_mask || !rows || !tapset9) return fail("null argument");
    if (n < 1 || Hs < 1 || Ws < 1 || Kc < 64 || Kc % 64 || Co < 64 || Co % 64) return fail("bad argument");
    ConvParams q = op_conv_params(x, w, y, n, xHp, xWp, xC, Hs, Ws, Co, 0, Hs, Ws, 1, Kc, Co, tapset9);
    q.accumulate = accumulate;
    q.bst_z = (const bf16_t*)bst_z; q.bst_mask = bst_mask; vpd_conv_set_bn_rows(q, rows);
    q.bst_z2 = (const bf16_t*)bst_z2; q.stats2 = rows2;
    if (q.taps.nr < 1 || q.taps.nc < 1) return fail("empty tap set");
    if (!vpd_conv_takes_bn_sums(q)) return fail("no kernel takes the BatchNorm sums for this shape");
    LCHECK(vpd_launch_conv(q, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_conv2d_bnsums(const void* x, const void* w, void* y, const void* bst_z, const unsigned char* bst_mask,
                                    double* rows, int n, int xHp, int xWp, int xC, int Hs, int Ws, int Kc, int Co,
                                    const int* tapset9, int accumulate, void* stream) {
    return op_conv2d_bnsums(x, w, y, bst_z, bst_mask, rows, nullptr, nullptr, n, xHp, xWp, xC, Hs, Ws, Kc, Co, tapset9, accumulate, stream);
}

// epilogue mode 8: the accumulating data gradient of a stage's first block, whose d feeds TWO BatchNorms (bn2 of the block before
// through z / rows, the 1x1 branch's through z2 / rows2) under the same ReLU bit map
extern "C" int vpd_op_conv2d_bnsums2(const void* x, const void* w, void* y, const void* bst_z, const unsigned char* bst_mask,
                                     double* rows, const void* bst_z2, double* rows2, int n, int xHp, int xWp, int xC, int Hs,
                                     int Ws, int Kc, int Co, const int* tapset9, void* stream) {
    if (!bst_z2 || !rows2) return fail("null argument");
    return op_conv2d_bnsums(x, w, y, bst_z, bst_mask, rows, bst_z2, rows2, n, xHp, xWp, xC, Hs, Ws, Kc, Co, tapset9, 1, stream);
}

// host-only: what vpd_launch_conv decides for these arguments on the current device (ConvDispatch, kernels.h).  flags: 1 statistics
// rows, 2 eval epilogue, 4 ReLU bit map on the old value, 8 BatchNorm sums (vpd_op_conv2d_bnsums), 16 of two BatchNorms.
// out12 = {class, pws, geo width, c64x2, 1x1 ring GEMM, 1x1 streaming, legacy halo, tile pixels, tile channels, epilogue mode,
// tiles per block, takes BatchNorm sums}
static int op_conv2d_dispatch(int n, int xHp, int xWp, int xC, int yHp, int yWp, int yC, int ypad, int Hs, int Ws, int osub, int oph, int opw,
                              int istr, int Kc, int Co, const int* tapset9, int accumulate, int flags, ConvDispatch* d, int* takes_sums) {
    if (n < 1 || Hs < 1 || Ws < 1 || xHp < 1 || xWp < 1 || xC < 1 || yC < Co || Kc < 64 || Kc % 64 || Co < 64 || Co % 64 || osub < 1 ||
        istr < 1 || (long long)n * Hs * Ws >= (1ll << 31) || (flags & ~31))
        return fail("bad argument");
    if ((flags & 16) && !(flags & 8)) return fail("a second BatchNorm needs the first");
    static const double present = 0.0;      // the launcher's decisions read pointers only as present / absent
    ConvParams q = op_conv_params(nullptr, nullptr, nullptr, n, xHp, xWp, xC, yHp, yWp, yC, ypad, Hs, Ws, istr, Kc, Co, tapset9);
    q.osub = osub; q.oph = oph; q.opw = opw; q.accumulate = accumulate;
    if (flags & 1) q.stats = const_cast<double*>(&present);
    if (flags & 2) { q.ep_scale = (const float*)&present; q.ep_shift = (const float*)&present; }
    if (flags & 4) q.acc_mask = (const unsigned char*)&present;
    if (flags & 8) { q.bst_z = (const bf16_t*)&present; q.bst_mask = (const unsigned char*)&present; vpd_conv_set_bn_rows(q, const_cast<double*>(&present)); }
    if (flags & 16) { q.bst_z2 = (const bf16_t*)&present; q.stats2 = const_cast<double*>(&present); }
    if (q.taps.nr < 1 || q.taps.nc < 1) return fail("empty tap set");
    *d = vpd_conv_dispatch(q);
    *takes_sums = (flags & 8) ? (int)vpd_conv_takes_bn_sums(q) : 0;
    return 0;
}
extern "C" int vpd_op_conv2d_dispatch(int n, int xHp, int xWp, int xC, int yHp, int yWp, int yC, int ypad, int Hs, int Ws, int osub,
                                      int oph, int opw, int istr, int Kc, int Co, const int* tapset9, int accumulate, int flags,
                                      int* out12) {
    if (!tapset9 || !out12) return fail("null argument");
    ConvDispatch d;
    int sums;
    const int rc = op_conv2d_dispatch(n, xHp, xWp, xC, yHp, yWp, yC, ypad, Hs, Ws, osub, oph, opw, istr, Kc, Co, tapset9, accumulate, flags, &d, &sums);
    if (rc) return rc;
    const int v[12] = {d.kclass, d.pws, d.geo, d.c64x2, d.ws1x1, d.stream1x1, d.halo, d.bm, d.bn, d.mode, d.tiles_per_block, sums};
    memcpy(out12, v, sizeof v);
    return 0;
}
// ... and whether that launch takes the interior loaders of conv3x3_pws_kernel (ConvDispatch::interior): *out = 1 / 0
extern "C" int vpd_op_conv2d_interior(int n, int xHp, int xWp, int xC, int yHp, int yWp, int yC, int ypad, int Hs, int Ws, int osub,
                                      int oph, int opw, int istr, int Kc, int Co, const int* tapset9, int accumulate, int flags,
                                      int* out) {
    if (!tapset9 || !out) return fail("null argument");
    ConvDispatch d;
    int sums;
    const int rc = op_conv2d_dispatch(n, xHp, xWp, xC, yHp, yWp, yC, ypad, Hs, Ws, osub, oph, opw, istr, Kc, Co, tapset9, accumulate, flags, &d, &sums);
    if (rc) return rc;
    *out = d.interior;
    return 0;
}

extern "C" int vpd_op_bn_forward(const void* z, const double* rows, const float* gamma, const float* beta, float* running_mean,
                                 float* running_var, float* mean, float* rstd, float* scale, float* shift, const void* res,
                                 void* out, unsigned char* mask_bits, int n, int H, int W, int C, int relu, float momentum,
                                 float eps, void* stream) {
    if (!z || !rows || !gamma || !beta || !mean || !rstd || !scale || !shift || !out) return fail("null argument");
    if (n < 1 || H < 1 || W < 1 || C < 8 || C % 8 || C > 4096) return fail("bad shape");
    BnApplyParams a = vpd_bn_apply_params((const bf16_t*)z, res ? 1 : 0, (const bf16_t*)res, (bf16_t*)out, n, H, W, C, relu);
    a.mask_out = mask_bits;
    const BnFusedFwd f = op_fused_fwd(op_fwd_side(rows, gamma, beta, running_mean, running_var, mean, rstd, scale, shift), a.M, momentum, eps);
    if (f.frozen && (!running_mean || !running_var)) return fail("a frozen BatchNorm needs running_mean and running_var");
    LCHECK(vpd_launch_bn_fwd_fused(a, f, (hipStream_t)stream));
    return 0;
}

// ... with the BatchNorm of a down-sampling branch in the same launch (res_kind 2): out = relu?(BatchNorm(z) + BatchNorm2(z2)), z2
// dense like z, no ReLU of its own.  Both BatchNorms take the hook's mode; running statistics of both or of neither.
extern "C" int vpd_op_bn_forward2(const void* z, const double* rows, const float* gamma, const float* beta, float* running_mean,
                                  float* running_var, float* mean, float* rstd, float* scale, float* shift, const void* z2,
                                  const double* rows2, const float* gamma2, const float* beta2, float* running_mean2,
                                  float* running_var2, float* mean2, float* rstd2, float* scale2, float* shift2, void* out,
                                  unsigned char* mask_bits, int n, int H, int W, int C, int relu, float momentum, float eps,
                                  void* stream) {
    if (!z || !rows || !gamma || !beta || !mean || !rstd || !scale || !shift || !out || !z2 || !rows2 || !gamma2 || !beta2 || !mean2 ||
        !rstd2 || !scale2 || !shift2)
        return fail("null argument");
    const int nrun = (running_mean != nullptr) + (running_var != nullptr) + (running_mean2 != nullptr) + (running_var2 != nullptr);
    if (nrun != 0 && nrun != 4) return fail("running statistics of both BatchNorms or of neither");
    if (g_op_bn_frozen && nrun != 4) return fail("a frozen BatchNorm needs running_mean and running_var");
    if (n < 1 || H < 1 || W < 1 || C < 8 || C % 8 || C > 4096) return fail("bad shape");
    BnApplyParams a = vpd_bn_apply_params((const bf16_t*)z, 2, (const bf16_t*)z2, (bf16_t*)out, n, H, W, C, relu);
    a.mask_out = mask_bits;
    BnFusedFwd f = op_fused_fwd(op_fwd_side(rows, gamma, beta, running_mean, running_var, mean, rstd, scale, shift), a.M, momentum, eps);
    f.s[1] = op_fwd_side(rows2, gamma2, beta2, running_mean2, running_var2, mean2, rstd2, scale2, shift2);
    LCHECK(vpd_launch_bn_fwd_fused(a, f, (hipStream_t)stream));
    return 0;
}

// the stem's and the VPD_FUSED_BN=0 path's finalize launch (bn_finalize_kernel) on the shared rows [VPD_STAT_ROWS][2][C], which it
// zeroes: mean / rstd / scale / shift, and the running statistics -- updated, or under the hook read and left alone
extern "C" int vpd_op_bn_finalize(double* rows, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                  float* mean, float* rstd, float* scale, float* shift, int count, int C, float momentum, float eps,
                                  void* stream) {
    if (!rows || !gamma || !beta || !mean || !rstd || !scale || !shift) return fail("null argument");
    if ((running_mean == nullptr) != (running_var == nullptr)) return fail("running_mean and running_var come together");
    if (g_op_bn_frozen && !running_mean) return fail("a frozen BatchNorm needs running_mean and running_var");
    if (count < 1 || C < 1) return fail("bad shape");
    LCHECK(vpd_launch_bn_finalize(rows, VPD_STAT_ROWS, C, (float)count, gamma, beta, running_mean, running_var, momentum, eps, mean,
                                  rstd, scale, shift, (hipStream_t)stream, g_op_bn_frozen != 0));
    return 0;
}

// the VPD_FUSED_BN=0 path's apply launch (bn_apply_kernel) on coefficient vectors the caller supplies: no statistics are involved.
// res_kind 0: out = relu?(scale z + shift); 1: + res, padded by 1 like out; 2: + rscale res + rshift, res dense like z
extern "C" int vpd_op_bn_apply(const void* z, const float* scale, const float* shift, const void* res, const float* rscale,
                               const float* rshift, int res_kind, void* out, int n, int H, int W, int C, int relu, void* stream) {
    if (!z || !scale || !shift || !out) return fail("null argument");
    if (res_kind < 0 || res_kind > 2) return fail("res_kind is 0, 1 or 2");
    if (res_kind != 0 && !res) return fail("null argument");
    if (res_kind == 2 && (!rscale || !rshift)) return fail("null argument");
    if (n < 1 || H < 1 || W < 1 || C < 8 || C % 8 || C > 4096) return fail("bad shape");
    if ((long long)n * H * W >= (1ll << 31)) return fail("bad shape");
    BnApplyParams a = vpd_bn_apply_params((const bf16_t*)z, res_kind, (const bf16_t*)res, (bf16_t*)out, n, H, W, C, relu);
    a.scale = scale; a.shift = shift; a.rscale = rscale; a.rshift = rshift;
    LCHECK(vpd_launch_bn_apply(a, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_bn_backward_apply(const void* dy, const void* z, const unsigned char* mask_bits, const double* rows,
                                        const float* gamma, const float* mean, const float* rstd, void* dz, float* dgamma,
                                        float* dbeta, int n, int H, int W, int C, void* stream) {
    if (!dy || !z || !mask_bits || !rows || !gamma || !mean || !rstd || !dz || !dgamma || !dbeta) return fail("null argument");
    BnBwdParams b = vpd_bn_bwd_params((const bf16_t*)dy, (const bf16_t*)z, mean, rstd, (bf16_t*)dz, 1, n, H, W, C);
    b.mask_bits = mask_bits;
    const BnFusedBwd f = op_fused_bwd(op_bwd_side(rows, gamma, dgamma, dbeta, z, mean, rstd, dz), b.M);
    LCHECK(vpd_launch_bn_bwd_apply_fused(b, f, (hipStream_t)stream));
    return 0;
}

// ... for TWO BatchNorms fed with the same masked gradient (bn_bwd_apply_fused_kernel<true>: a down-sampling block's last BatchNorm
// and its 1x1 branch's, whose sums the next block's data gradient took): rows2 holds sum g (unused) and sum g * z2
extern "C" int vpd_op_bn_backward_apply2(const void* dy, const void* z, const unsigned char* mask_bits, const double* rows,
                                         const float* gamma, const float* mean, const float* rstd, void* dz, float* dgamma,
                                         float* dbeta, const void* z2, const double* rows2, const float* gamma2, const float* mean2,
                                         const float* rstd2, void* dz2, float* dgamma2, float* dbeta2, int n, int H, int W, int C,
                                         void* stream) {
    if (!dy || !z || !mask_bits || !rows || !gamma || !mean || !rstd || !dz || !dgamma || !dbeta || !z2 || !rows2 || !gamma2 || !mean2 ||
        !rstd2 || !dz2 || !dgamma2 || !dbeta2)
        return fail("null argument");
    if (n < 1 || H < 1 || W < 1 || C < 8 || C % 8) return fail("bad shape");
    BnBwdParams b = vpd_bn_bwd_params((const bf16_t*)dy, (const bf16_t*)z, mean, rstd, (bf16_t*)dz, 1, n, H, W, C);
    b.mask_bits = mask_bits;
    BnFusedBwd f = op_fused_bwd(op_bwd_side(rows, gamma, dgamma, dbeta, z, mean, rstd, dz), b.M);
    f.s[1] = op_bwd_side(rows2, gamma2, dgamma2, dbeta2, z2, mean2, rstd2, dz2);
    LCHECK(vpd_launch_bn_bwd_apply_fused(b, f, (hipStream_t)stream));
    return 0;
}

// ---- a Bottleneck's closing 1x1 convolution with its BatchNorm (conv_stream.hip): the launchers of step.hip's run_conv3_bn_* /
// run_conv3d_bn_* from flat arguments.  Every refusal is the launcher's own predicate, asked before anything is launched ----
static bool op_conv1x1_bn_shape_ok(int n, int H, int W, int istr, int Kc, int Co) {
    return n >= 1 && H >= 1 && W >= 1 && istr >= 1 && Kc >= 64 && Kc % 64 == 0 && Co >= 64 && Co % 64 == 0 &&
           (long long)n * H * W < (1ll << 31);
}

extern "C" int vpd_op_conv1x1_bn(int mode, const void* x, const void* w, int n, int H, int W, int istr, int Kc, int Co, double* rows,
                                 const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                                 float eps, float* mean, float* rstd, float* scale, float* shift, const void* res, void* out,
                                 unsigned char* mask_bits, const void* dout, void* dz, float* dgamma, float* dbeta, void* stream) {
    if (mode < 0 || mode > 3) return fail("mode 0 .. 3");
    if (!x || !w || !rows) return fail("null argument");
    if (mode == 1 && (!gamma || !beta || !mean || !rstd || !scale || !shift || !res || !out || (running_mean == nullptr) != (running_var == nullptr)))
        return fail("null argument");
    if (mode >= 2 && (!dout || !mask_bits)) return fail("null argument");
    if (mode == 3 && (!gamma || !mean || !rstd || !dz || !dgamma || !dbeta)) return fail("null argument");
    if (!op_conv1x1_bn_shape_ok(n, H, W, istr, Kc, Co)) return fail("bad argument");
    ConvParams q = vpd_conv1x1_params((const bf16_t*)x, (const bf16_t*)w, n, H, W, istr, Kc, Co);
    if (!vpd_conv1x1_bn_eligible(q)) return fail("conv1x1_bn_stream_kernel does not take this shape");
    const BnFusedFwd f = op_fused_fwd(op_fwd_side(rows, gamma, beta, running_mean, running_var, mean, rstd, scale, shift), q.M, momentum, eps);
    const BnFusedBwd b = op_fused_bwd(op_bwd_side(rows, gamma, dgamma, dbeta, nullptr, mean, rstd, dz), q.M);
    const BnTailPass pass = (BnTailPass)mode;      // (0 .. 3 are the enum's values, checked above)
    BnTailLaunch t = {pass, nullptr, nullptr, nullptr, 0};
    if (pass == BN_TAIL_STATS) vpd_conv_set_bn_rows(q, rows);
    else if (pass == BN_TAIL_FWD) {
        vpd_conv_set_y(q, (bf16_t*)out, 1);
        vpd_conv_set_res(q, (const bf16_t*)res);
        t.fwd = &f; t.mask_out = mask_bits;
        if (f.frozen && !running_mean) return fail("a frozen BatchNorm needs running_mean and running_var");
    } else {
        q.y = (bf16_t*)const_cast<void*>(dout); q.acc_mask = mask_bits;
        t.bwd = &b; t.dzpad = pass == BN_TAIL_BWD_APPLY ? 1 : 0;
    }
    LCHECK(vpd_launch_conv1x1_bn(q, t, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_conv1x1_bn2(int mode, const void* x, const void* w, const void* x2, const void* w2, int n, int H, int W, int Kc,
                                  int Kc2, int Co, double* rows, double* rows2, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, float* mean, float* rstd, float* scale, float* shift,
                                  const float* gamma2, const float* beta2, float* running_mean2, float* running_var2, float* mean2,
                                  float* rstd2, float* scale2, float* shift2, float momentum, float eps, void* out,
                                  unsigned char* mask_bits, const void* dout, void* dz, void* dz2, float* dgamma, float* dbeta,
                                  float* dgamma2, float* dbeta2, void* stream) {
    if (mode < 1 || mode > 3) return fail("mode 1 .. 3");
    if (!x || !w || !x2 || !w2 || !rows || !rows2) return fail("null argument");
    if (mode == 1 && (!gamma || !beta || !mean || !rstd || !scale || !shift || !gamma2 || !beta2 || !mean2 || !rstd2 || !scale2 || !shift2 ||
                      !out || (running_mean == nullptr) != (running_var == nullptr) || (running_mean == nullptr) != (running_mean2 == nullptr) ||
                      (running_mean2 == nullptr) != (running_var2 == nullptr)))
        return fail("null argument");
    if (mode >= 2 && (!dout || !mask_bits)) return fail("null argument");
    if (mode == 3 && (!gamma || !mean || !rstd || !gamma2 || !mean2 || !rstd2 || !dz || !dz2 || !dgamma || !dbeta || !dgamma2 || !dbeta2))
        return fail("null argument");
    if (!op_conv1x1_bn_shape_ok(n, H, W, 1, Kc, Co) || Kc2 < 1) return fail("bad argument");
    ConvParams q = vpd_conv1x1_params((const bf16_t*)x, (const bf16_t*)w, n, H, W, 1, Kc, Co);
    q.x2 = (const bf16_t*)x2; q.w2 = (const bf16_t*)w2; q.Kc2 = Kc2;
    if (!vpd_conv1x1_bn2_eligible(q)) return fail("conv1x1_bn2_stream_kernel does not take this shape");
    BnFusedFwd f = op_fused_fwd(op_fwd_side(rows, gamma, beta, running_mean, running_var, mean, rstd, scale, shift), q.M, momentum, eps);
    f.s[1] = op_fwd_side(rows2, gamma2, beta2, running_mean2, running_var2, mean2, rstd2, scale2, shift2);
    BnFusedBwd b = op_fused_bwd(op_bwd_side(rows, gamma, dgamma, dbeta, nullptr, mean, rstd, dz), q.M);
    b.s[1] = op_bwd_side(rows2, gamma2, dgamma2, dbeta2, nullptr, mean2, rstd2, dz2);
    const BnTailPass pass = (BnTailPass)mode;      // (1 .. 3 are the enum's values, checked above)
    BnTailLaunch t = {pass, nullptr, nullptr, nullptr, 0};
    if (pass == BN_TAIL_FWD) {
        vpd_conv_set_y(q, (bf16_t*)out, 1);
        t.fwd = &f; t.mask_out = mask_bits;
        if (f.frozen && !running_mean) return fail("a frozen BatchNorm needs running_mean and running_var");
    } else {
        q.y = (bf16_t*)const_cast<void*>(dout); q.acc_mask = mask_bits;
        t.bwd = &b; t.dzpad = pass == BN_TAIL_BWD_APPLY ? 1 : 0;
    }
    LCHECK(vpd_launch_conv1x1_bn2(q, t, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_conv1x1_bn_dispatch(int n, int H, int W, int Kc, int Co, int two, int* out5) {
    if (!out5) return fail("null argument");
    if (!op_conv1x1_bn_shape_ok(n, H, W, 1, Kc, Co)) return fail("bad argument");
    static const double present = 0.0;      // (the predicates read pointers only as present / absent)
    ConvParams q = vpd_conv1x1_params(nullptr, nullptr, n, H, W, 1, Kc, Co);
    if (two) { q.x2 = (const bf16_t*)&present; q.w2 = (const bf16_t*)&present; q.Kc2 = Kc; }
    int v[5] = {0, 0, 0, 0, 0};
    v[0] = two ? (int)vpd_conv1x1_bn2_eligible(q) : (int)vpd_conv1x1_bn_eligible(q);
    if (v[0]) vpd_conv1x1_bn_grid(q, two != 0, v + 1);
    memcpy(out5, v, sizeof v);
    return 0;
}

// ---- stem pool, BatchNorm backward launchers, head: the product launchers unchanged, parameters from flat arguments ----
extern "C" int vpd_op_stem_pool_forward(const void* z, const float* scale, const float* shift, void* out_padded,
                                        unsigned char* idx, int n, int Hz, int Wz, int C, int opad, void* stream) {
    if (!z || !scale || !shift || !out_padded) return fail("null argument");
    if (n < 1 || Hz < 1 || Wz < 1 || C < 8 || C % 8 || opad < 0) return fail("bad shape");
    StemPoolParams q;
    memset(&q, 0, sizeof q);
    q.z = (const bf16_t*)z; q.Hz = Hz; q.Wz = Wz; q.scale = scale; q.shift = shift;
    q.out = (bf16_t*)out_padded; q.opad = opad; q.idx = idx;
    q.N = n; q.Ho = (Hz - 1) / 2 + 1; q.Wo = (Wz - 1) / 2 + 1; q.C = C;
    LCHECK(vpd_launch_stem_pool(q, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_stem_pool_backward(const void* dpool, const unsigned char* idx, const void* z, const float* mean,
                                         const float* rstd, const float* scale, const float* shift, const float* gamma,
                                         const float* beta, const void* pooled_padded, double* rows, float* coef, void* dz,
                                         float* dgamma, float* dbeta, int n, int Hz, int Wz, int C, void* stream) {
    if (!dpool || !idx || !z || !mean || !rstd || !scale || !shift || !gamma || !beta || !rows || !coef || !dz || !dgamma || !dbeta)
        return fail("null argument");
    if (n < 1 || Hz < 1 || Wz < 1 || C < 8 || C % 8 || 256 % (C / 8)) return fail("bad shape");
    StemPoolBwdParams sb;
    memset(&sb, 0, sizeof sb);
    sb.dpool = (const bf16_t*)dpool; sb.idx = idx; sb.z = (const bf16_t*)z;
    sb.mean = mean; sb.rstd = rstd; sb.scale = scale; sb.shift = shift; sb.partials = rows;
    sb.pooled = (const bf16_t*)pooled_padded; sb.ppad = 1; sb.gamma_p = gamma; sb.beta_p = beta;
    sb.M = n * Hz * Wz; sb.Hz = Hz; sb.Wz = Wz; sb.Ho = (Hz - 1) / 2 + 1; sb.Wo = (Wz - 1) / 2 + 1; sb.C = C;
    LCHECK(vpd_launch_stem_pool_bwd(sb, (float)sb.M, gamma, dgamma, dbeta, coef, (bf16_t*)dz, (hipStream_t)stream, g_op_bn_frozen != 0));
    return 0;
}

// the stem convolution's data gradient (conv_stem_dgrad.hip): the launch vpd_backward_ext makes, from flat arguments
extern "C" int vpd_op_stem_dgrad(const void* dz, const float* w_oihw, float* dx_nchw, int n, int c_in, int H, int W, void* stream) {
    if (!dz || !w_oihw || !dx_nchw) return fail("null argument");
    if (n < 1) return fail("n must be at least 1");
    if (c_in < 1 || c_in > 8) return fail("c_in outside 1..8");
    if (H < 32 || W < 32 || (H & 1) || (W & 1)) return fail("H and W must be even and at least 32");
    if (reinterpret_cast<size_t>(dx_nchw) & 7) return fail("dx_nchw must be 8-byte aligned");
    LCHECK(vpd_launch_stem_dgrad((const bf16_t*)dz, w_oihw, dx_nchw, n, c_in, H, W, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_bn_backward(void* dy, const void* z, const void* act_padded, const unsigned char* mask_bits,
                                  const float* mscale, const float* mshift, const float* dy_pooled, double* rows, float* coef,
                                  void* sync, unsigned* err, const float* gamma, const float* mean, const float* rstd, void* dz,
                                  int dzpad, float* dgamma, float* dbeta, int n, int H, int W, int C, int write_g, int fused,
                                  void* stream) {
    if (!dy || !z || !rows || !gamma || !mean || !rstd || !dz || !dgamma || !dbeta) return fail("null argument");
    if (n < 1 || H < 1 || W < 1 || C < 8 || C % 8 || dzpad < 0) return fail("bad shape");
    if ((mscale == nullptr) != (mshift == nullptr)) return fail("mscale and mshift come together");
    if ((act_padded != nullptr) + (mask_bits != nullptr) + (mscale != nullptr) > 1) return fail("one ReLU mask at most");
    if (write_g && !act_padded) return fail("write_g goes with the activation mask");
    BnBwdParams b = vpd_bn_bwd_params((const bf16_t*)dy, (const bf16_t*)z, mean, rstd, (bf16_t*)dz, dzpad, n, H, W, C);
    vpd_bn_bwd_set_act(b, (bf16_t*)dy, (const bf16_t*)act_padded);
    b.coef = coef; b.partials = rows; b.write_g = write_g; b.mscale = mscale; b.mshift = mshift; b.mask_bits = mask_bits;
    if (!fused) {
        if (mask_bits || dy_pooled) return fail("the three-launch path takes neither a ReLU bit map nor a pooled gradient");
        if (!coef) return fail("the three-launch path needs coef");
        LCHECK(vpd_launch_bn_bwd(b, (float)b.M, gamma, dgamma, dbeta, (hipStream_t)stream, g_op_bn_frozen != 0));
        return 0;
    }
    if (!sync || !err) return fail("the fused launch needs sync and err");
    if (!vpd_bn_bwd_fused_ok(b.M, C, act_padded != nullptr, write_g != 0)) return fail("no fused BatchNorm backward for this shape");
    if (dy_pooled) {
        if (!mask_bits) return fail("the folded average-pool gradient needs the ReLU bit map");
        if ((H * W) & (H * W - 1)) return fail("the folded average-pool gradient takes a power-of-two H W (vpd_op_avgpool_bwd first otherwise)");
        b.dy_pooled = dy_pooled; b.dy_pool_scale = 1.f / (float)(H * W);
    }
    const BnFusedBwd f = op_fused_bwd(op_bwd_side(rows, gamma, dgamma, dbeta, z, mean, rstd, dz), b.M, sync, err);
    LCHECK(vpd_launch_bn_bwd_fused(b, f, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_bn_backward_pair(void* dy, const void* act_padded, const void* zA, const float* meanA, const float* rstdA,
                                       const float* gammaA, double* rowsA, void* dzA, float* dgammaA, float* dbetaA,
                                       const void* zB, const float* meanB, const float* rstdB, const float* gammaB,
                                       double* rowsB, void* dzB, float* dgammaB, float* dbetaB, void* sync, unsigned* err, int n,
                                       int H, int W, int C, void* stream) {
    if (!dy || !act_padded || !zA || !meanA || !rstdA || !gammaA || !rowsA || !dzA || !dgammaA || !dbetaA || !zB || !meanB ||
        !rstdB || !gammaB || !rowsB || !dzB || !dgammaB || !dbetaB || !sync || !err)
        return fail("null argument");
    if (n < 1 || H < 1 || W < 1) return fail("bad shape");
    if (!vpd_bn_bwd_fused2_ok(n * H * W, C)) return fail("no paired BatchNorm backward for this shape");
    BnBwdParams b = vpd_bn_bwd_params((const bf16_t*)dy, (const bf16_t*)zA, meanA, rstdA, (bf16_t*)dzA, 1, n, H, W, C);
    vpd_bn_bwd_set_act(b, (bf16_t*)dy, (const bf16_t*)act_padded);
    BnFusedBwd f = op_fused_bwd(op_bwd_side(rowsA, gammaA, dgammaA, dbetaA, zA, meanA, rstdA, dzA), b.M, sync, err);
    f.s[1] = op_bwd_side(rowsB, gammaB, dgammaB, dbetaB, zB, meanB, rstdB, dzB);
    LCHECK(vpd_launch_bn_bwd_fused2(b, f, (hipStream_t)stream));
    return 0;
}

// host-only: out4 = {blocks, g resident, z (pair: zA) resident, pair: zB resident} of the fused backward of n H W x C on this device
extern "C" int vpd_op_bn_backward_residency(int M, int C, int pair, int* out4) {
    if (!out4 || M < 1 || C < 64 || C > 2048 || C % 8 || 1024 % (C / 8)) return fail("bad argument");
    const BnBwdFusedGeom q = vpd_bn_bwd_fused_geom(M, C, pair ? 3 : 2);
    out4[0] = q.G; out4[1] = q.keep[0]; out4[2] = q.keep[1]; out4[3] = q.keep[2];
    return 0;
}

extern "C" int vpd_op_avgpool(const void* act_padded, int n, int H, int W, int C, int pad, float* pooled, void* stream) {
    if (!act_padded || !pooled) return fail("null argument");
    if (n < 1 || H < 1 || W < 1 || C < 8 || C % 8 || pad < 0) return fail("bad shape");
    LCHECK(vpd_launch_avgpool((const bf16_t*)act_padded, H + 2 * pad, W + 2 * pad, pad, H, W, C, n, pooled, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_avgpool_bwd(const float* dpooled, int n, int H, int W, int C, void* dact, void* stream) {
    if (!dpooled || !dact) return fail("null argument");
    if (n < 1 || H < 1 || W < 1 || C < 8 || C % 8) return fail("bad shape");
    LCHECK(vpd_launch_avgpool_bwd(dpooled, H, W, C, n, (bf16_t*)dact, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_sgemm(const float* A, const float* B, float* Y, const float* bias, int M, int N, int K, int ta, int tb,
                            int relu, void* stream) {
    if (!A || !B || !Y) return fail("null argument");
    if (M < 1 || N < 1 || K < 1) return fail("bad shape");
    LCHECK(vpd_launch_sgemm(A, B, Y, bias, M, N, K, ta, tb, relu, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_colsum(const float* A, int M, int N, float* out, void* stream) {
    if (!A || !out || M < 1 || N < 1) return fail("bad argument");
    LCHECK(vpd_launch_colsum(A, M, N, out, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_relu_mask(float* d, const float* act, long long n, void* stream) {
    if (!d || !act || n < 1) return fail("bad argument");
    LCHECK(vpd_launch_relu_mask(d, act, (long)n, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_mse(const float* e, const float* t, long long n, float* de, float* loss_step, double* loss_accum,
                          void* stream) {
    if (!e || !t || n < 1) return fail("bad argument");
    LCHECK(vpd_launch_mse(e, t, (long)n, de, loss_step, loss_accum, (hipStream_t)stream));
    return 0;
}

static WgradParams op_wgrad_params(const void* dz, const void* x, float* dw, int n, int dzHp, int dzWp, int dzC, int dzpad, int xHp,
                                   int xWp, int xC, int Hs, int Ws, int istr, int Kc, int Co, const int* tapset9, float* slab) {
    WgradParams q;
    memset(&q, 0, sizeof q);
    q.dz = (const bf16_t*)dz; q.dzHp = dzHp; q.dzWp = dzWp; q.dzC = dzC; q.dzpad = dzpad;
    q.x = (const bf16_t*)x; q.xHp = xHp; q.xWp = xWp; q.xC = xC; q.dw = dw; q.slab = slab;
    q.N = n; q.Hs = Hs; q.Ws = Ws; q.istr = istr; q.Kc = Kc; q.Co = Co; q.M = n * Hs * Ws;
    q.taps = tapset_from(tapset9);
    return q;
}
extern "C" int vpd_op_wgrad(const void* dz, const void* x, float* dw, int n, int dzHp, int dzWp, int dzC, int dzpad,
                            int xHp, int xWp, int xC, int Hs, int Ws, int istr, int Kc, int Co, const int* tapset9,
                            float* slab, void* stream) {
    const WgradParams q = op_wgrad_params(dz, x, dw, n, dzHp, dzWp, dzC, dzpad, xHp, xWp, xC, Hs, Ws, istr, Kc, Co, tapset9, slab);
    if (q.taps.nr < 1 || q.taps.nc < 1) return fail("empty tap set");
    LCHECK(vpd_launch_wgrad(q, (hipStream_t)stream));
    return 0;
}
// host-only: what vpd_launch_wgrad decides for the geometry of a vpd_op_wgrad call (has_slab: a slab is given; prefer_halo_1x1: the
// caller's wish the plan states for the BasicBlock students' 1x1 convs).  out9: vpd_wgrad_dispatch (kernels.h)
extern "C" int vpd_op_wgrad_dispatch(int n, int dzHp, int dzWp, int dzC, int dzpad, int xHp, int xWp, int xC, int Hs, int Ws, int istr,
                                     int Kc, int Co, const int* tapset9, int has_slab, int prefer_halo_1x1, int* out9) {
    if (!tapset9 || !out9) return fail("null argument");
    if (n < 1 || Hs < 1 || Ws < 1 || (long long)n * Hs * Ws >= (1ll << 31)) return fail("bad argument");
    static float present = 0.f;             // (the route reads the slab only as present / absent)
    WgradParams q = op_wgrad_params(nullptr, nullptr, nullptr, n, dzHp, dzWp, dzC, dzpad, xHp, xWp, xC, Hs, Ws, istr, Kc, Co, tapset9,
                                    has_slab ? &present : nullptr);
    q.prefer_halo_1x1 = prefer_halo_1x1 != 0;
    if (q.taps.nr < 1 || q.taps.nc < 1) return fail("empty tap set");
    if (!vpd_wgrad_dispatch(q, out9)) return fail("the weight-gradient launcher refuses this shape (channels not a multiple of 64)");
    return 0;
}

// ---- the grouped 64 x 64 launch (conv_wgrad_halo_grouped_kernel) of `nprob` 3x3 stride-1 pad-1 convolutions: what
// WgradQueue::flush (step.hip) gives vpd_launch_wgrad_group.  dims: 5 ints per problem {n, H, W, Co, Ci}; layouts as
// vpd_op_wgrad128_group documents them; slab[i]: vpd_op_wgrad_group_slab_floats(Co, Ci) floats ----
static const char* op_wgrad_group_params(int nprob, const void* const* dz, const void* const* x, float* const* dw, float* const* slab,
                                         const int* dims, WgradParams* qs) {
    if (nprob < 1 || nprob > vpd_wgrad_group_max()) return "nprob outside 1..18";
    if (!dims) return "null argument";
    for (int i = 0; i < nprob; ++i) {
        const int n = dims[5 * i], H = dims[5 * i + 1], W = dims[5 * i + 2], Co = dims[5 * i + 3], Ci = dims[5 * i + 4];
        if (n < 1 || H < 1 || W < 1 || (long long)n * H * W >= (1ll << 31)) return "bad argument";
        if (Co < 64 || Co % 64 || Ci < 64 || Ci % 64) return "Co and Ci must be multiples of 64";
        static float present = 0.f;
        const int taps[9] = {3, 3, 0, 1, 0, 1, 0, 3, 1};
        qs[i] = op_wgrad_params(dz ? dz[i] : nullptr, x ? x[i] : nullptr, dw ? dw[i] : nullptr, n, H + 2, W + 2, Co, 1, H + 2, W + 2, Ci,
                                H, W, 1, Ci, Co, taps, slab ? slab[i] : &present);
        if (!vpd_wgrad_group_eligible(qs[i])) return "the halo tiling does not take this plane";
    }
    return nullptr;
}
extern "C" size_t vpd_op_wgrad_group_slab_floats(int Co, int Ci) { return vpd_wgrad_group_slab_floats(0, Co, Ci, 9); }
// host-only: out = {pass instantiation, tasks, grid, halo passes} then {ksplit, cpb, tiles} per problem (4 + 3 nprob ints)
extern "C" int vpd_op_wgrad_group_dispatch(int nprob, const int* dims, int* out) {
    if (!out) return fail("null argument");
    WgradParams qs[18];
    if (const char* e = op_wgrad_group_params(nprob, nullptr, nullptr, nullptr, nullptr, dims, qs)) return fail(e);
    const int rc = vpd_wgrad_group_dispatch(qs, nprob, out, out + 4);
    if (rc == 2) return fail("the problems of a group must stage the same number of halo passes");
    if (rc != 0) return fail("the halo tiling does not take this plane");
    return 0;
}
extern "C" int vpd_op_wgrad_group(int nprob, const void* const* dz, const void* const* x, float* const* dw, float* const* slab,
                                  const int* dims, void* stream) {
    if (!dz || !x || !dw || !slab || !dims) return fail("null argument");
    WgradParams qs[18];
    if (const char* e = op_wgrad_group_params(nprob, dz, x, dw, slab, dims, qs)) return fail(e);
    int head[4], per[3 * 18];
    const int rc = vpd_wgrad_group_dispatch(qs, nprob, head, per);
    if (rc == 2) return fail("the problems of a group must stage the same number of halo passes");
    if (rc != 0) return fail("the halo tiling does not take this plane");
    for (int i = 0; i < nprob; ++i) {
        if (!dz[i] || !x[i] || !dw[i]) return fail("null argument");
        // (a problem of one split stores into dw; the others need their slab)
        if (per[3 * i] > 1 && !slab[i]) return fail("null argument");
        if ((reinterpret_cast<size_t>(dw[i]) | reinterpret_cast<size_t>(slab[i])) & 15) return fail("dw and slab must be 16-byte aligned");
    }
    LCHECK(vpd_launch_wgrad_group(qs, nprob, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_wgrad_pair(const void* dz, const void* dz2, const void* x, float* dw, float* dw2, int n, int dzHp, int dzWp,
                                 int dzC, int dzpad, int xHp, int xWp, int xC, int Hs, int Ws, int istr, int Kc, int Co,
                                 const int* tapset9, float* slab, float* slab2, void* stream) {
    if (!dz || !dz2 || !x || !dw || !dw2 || !tapset9 || !slab || !slab2) return fail("null argument");
    if (n < 1 || Hs < 1 || Ws < 1) return fail("bad argument");
    WgradParams q;
    memset(&q, 0, sizeof q);
    q.dz = (const bf16_t*)dz; q.dzHp = dzHp; q.dzWp = dzWp; q.dzC = dzC; q.dzpad = dzpad;
    q.x = (const bf16_t*)x; q.xHp = xHp; q.xWp = xWp; q.xC = xC; q.dw = dw; q.slab = slab;
    q.N = n; q.Hs = Hs; q.Ws = Ws; q.istr = istr; q.Kc = Kc; q.Co = Co; q.M = n * Hs * Ws;
    WgradParams q1 = q;                       // the branch: one tap at padded offset (1, 1)
    q1.dz = (const bf16_t*)dz2; q1.dw = dw2; q1.slab = slab2; q1.prefer_halo_1x1 = 1;
    q1.taps = vpd_taps_1x1();
    q.taps = tapset_from(tapset9);
    if (!vpd_wgrad_pair_ok(q, q1)) return fail("not a pair the halo weight-gradient launch takes (shapes, or VPD_WGRAD_DS_RIDE=0 / VPD_WGRAD_1X1=0 / VPD_WGRAD_S2=0)");
    LCHECK(vpd_launch_wgrad_pair(q, q1, (hipStream_t)stream));
    return 0;
}
extern "C" int vpd_op_wgrad_pair_lds_bytes(int Hs, int Ws, int ns, long long* bytes) {
    return vpd_wgrad_pair_lds_query(Hs, Ws, ns, bytes);
}

// Grouped 128 x 64 weight gradients (conv_wgrad128_persistent_kernel) of `nprob` 3x3 stride-1 pad-1 convolutions in ONE
// launch.  dims: 7 ints per problem {n, H, W, Co, Ci, stride, k} (H, W: OUTPUT size; stride 1 or 2; k = 3: 3x3 pad 1, k = 1: 1x1
// pad 0); dz[i]: padded bf16 [n][H+2][W+2][Co]; x[i]: padded bf16 [n][stride*H+2][stride*W+2][Ci]; dw[i]: fp32 [k*k][Co][Ci]; slab[i]: fp32 scratch of vpd_op_wgrad128_slab_floats(Co, Ci) floats;
// dev_table: vpd_op_wgrad128_table_bytes() of device memory.
extern "C" size_t vpd_op_wgrad128_table_bytes(void) { return vpd_wgrad128_table_bytes(); }
extern "C" size_t vpd_op_wgrad128_slab_floats(int Co, int Ci) { return vpd_wgrad_group_slab_floats(0, Co, Ci, 1) > vpd_wgrad_group_slab_floats(0, Co, Ci, 9) ? vpd_wgrad_group_slab_floats(0, Co, Ci, 1) : vpd_wgrad_group_slab_floats(0, Co, Ci, 9); }
extern "C" int vpd_op_wgrad128_group(int nprob, const void* const* dz, const void* const* x, float* const* dw,
                                     float* const* slab, const int* dims, void* dev_table, void* stream) {
    if (nprob < 1 || nprob > 18 || !dz || !x || !dw || !slab || !dims || !dev_table) return fail("bad argument");
    WgradParams qs[18];
    for (int i = 0; i < nprob; ++i) {
        const int n = dims[7 * i], H = dims[7 * i + 1], W = dims[7 * i + 2], Co = dims[7 * i + 3], Ci = dims[7 * i + 4];
        const int S = dims[7 * i + 5], ksz = dims[7 * i + 6];
        if ((S != 1 && S != 2) || (ksz != 1 && ksz != 3)) return fail("stride must be 1 or 2, k 1 or 3");
        WgradParams q;
        memset(&q, 0, sizeof q);
        q.dz = (const bf16_t*)dz[i]; q.dzHp = H + 2; q.dzWp = W + 2; q.dzC = Co; q.dzpad = 1;
        q.x = (const bf16_t*)x[i]; q.xHp = S * H + 2; q.xWp = S * W + 2; q.xC = Ci;
        q.dw = dw[i]; q.slab = slab[i];
        q.N = n; q.Hs = H; q.Ws = W; q.istr = S; q.Kc = Ci; q.Co = Co; q.M = n * H * W;
        if (ksz == 3) {
            q.taps.nr = 3; q.taps.nc = 3; q.taps.dy0 = 0; q.taps.dys = 1; q.taps.dx0 = 0; q.taps.dxs = 1;
            q.taps.w0 = 0; q.taps.wrs = 3; q.taps.wcs = 1;
        } else q.taps = vpd_taps_1x1();
        vpd_wgrad_swap_1x1(q);      // 1x1, < 128 outputs, a multiple of 128 inputs: as the step's grouped launch states it
        if (!vpd_wgrad128_eligible(q)) return fail("shape not eligible for the 128 x 64 weight-gradient kernel");
        qs[i] = q;
    }
    // no schedule cache: a cache skips the upload when shapes and table ADDRESS repeat, and a test that frees its table and gets the
    // same address back from the allocator, overwritten in between, would launch on a stale task table (an illegal access)
    LCHECK(vpd_launch_wgrad128_group(qs, nprob, nullptr, dev_table, (hipStream_t)stream));
    return 0;
}

// ---- the reference boundary one launch at a time (optim.hip: input packing, weight repack, gradient unpack, AdamW + repack,
// range zeroing) and the weight gradients' slab sums (conv_wgrad.hip).  The descriptors and block maps are push_pack_desc's and
// build_adam_map's, uploaded for the one launch: the stream is synchronised before they are freed (not timing entry points) ----
namespace {
struct DevTables {
    PackDesc* descs = nullptr;
    int* bmap = nullptr;
    ~DevTables() { (void)hipFree(descs); (void)hipFree(bmap); }
    hipError_t upload(const std::vector<PackDesc>& d, const std::vector<int>& m, hipStream_t s) {
        hipError_t e = hipMalloc((void**)&descs, d.size() * sizeof(PackDesc));
        if (e == hipSuccess) e = hipMalloc((void**)&bmap, m.size() * sizeof(int));
        if (e == hipSuccess) e = hipMemcpyAsync(descs, d.data(), d.size() * sizeof(PackDesc), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(bmap, m.data(), m.size() * sizeof(int), hipMemcpyHostToDevice, s);
        return e;
    }
};
inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }
// the shapes the tile kernels take: 32 x 32 (co x ci) tiles of at most 9 taps; the stem: 7 x 7 with at most 8 channels
const char* op_conv_shape_error(int Co, int Ci, int k, int stem) {
    if (stem != 0 && stem != 1) return "stem is 0 or 1";
    if (stem) return (k == 7 && Ci >= 1 && Ci <= 8 && Co >= 1) ? nullptr : "the stem is 7x7 with 1..8 input channels";
    if (Co < 32 || Co % 32 || Ci < 32 || Ci % 32) return "Co and Ci must be multiples of 32";
    if (k < 1 || k > 3) return "k must be 1, 2 or 3";
    return nullptr;
}
}  // namespace

extern "C" int vpd_op_pack_input(const float* x_f32_nchw, int n, int c, int H, int W, void* out, int Hp, int Wp, int pad,
                                 void* stream) {
    if (!x_f32_nchw || !out) return fail("null argument");
    if (c < 1 || c > 8) return fail("c outside 1..8");
    if (n < 1 || H < 1 || W < 1 || pad < 0 || Hp < H + pad || Wp < W + pad) return fail("bad shape");
    if ((long long)n * Hp * Wp >= (1ll << 31) || (long long)n * H * W >= (1ll << 31)) return fail("bad shape");
    if (!aligned(x_f32_nchw, 4) || !aligned(out, 16)) return fail("x must be 4-byte aligned, out 16-byte aligned");
    LCHECK(vpd_launch_pack_input(x_f32_nchw, n, c, H, W, (bf16_t*)out, Hp, Wp, pad, 8, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_pack_weights(const float* master, int Co, int Ci, int k, int stem, void* fwd_out, void* dgr_out,
                                   void* stream) {
    if (!master || !fwd_out) return fail("null argument");
    if (const char* e = op_conv_shape_error(Co, Ci, k, stem)) return fail(e);
    if (stem && dgr_out) return fail("the stem has no data-gradient layout");
    if (!aligned(master, 4) || !aligned(fwd_out, 16) || !aligned(dgr_out, 16)) return fail("master must be 4-byte aligned, the layouts 16-byte aligned");
    // one arena pointer, element offsets from it: the lower of the two outputs
    bf16_t* f = (bf16_t*)fwd_out;
    bf16_t* d = (bf16_t*)dgr_out;
    bf16_t* arena = (d && d < f) ? d : f;
    ConvInfo cv;
    set_pack_geom(cv, Ci, Co, k, stem != 0);
    cv.w_off = 0; cv.fwd_off = f - arena; cv.dgr_off = d ? d - arena : -1;
    std::vector<PackDesc> descs;
    std::vector<int> bmap, unused;
    push_pack_desc(descs, bmap, unused, cv);
    hipStream_t s = (hipStream_t)stream;
    DevTables t;
    HCHECK(t.upload(descs, bmap, s));
    LCHECK(vpd_launch_pack_weights(t.descs, (int)descs.size(), t.bmap, (int)bmap.size() / 2, master, arena, s));
    HCHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int vpd_op_unpack_grads(const float* wg, int Co, int Ci, int k, int Kc, int stem, float* grads_out, void* stream) {
    if (!wg || !grads_out) return fail("null argument");
    if (const char* e = op_conv_shape_error(Co, Ci, k, stem)) return fail(e);
    if (stem ? Kc < 8 * k : Kc < Ci) return fail("Kc is too small for the scratch layout");
    if (!aligned(wg, 4) || !aligned(grads_out, 4)) return fail("wg and grads_out must be 4-byte aligned");
    ConvInfo cv;
    set_pack_geom(cv, Ci, Co, k, stem != 0);
    cv.Kc = Kc;
    cv.w_off = 0; cv.wg_off = 0;
    std::vector<PackDesc> descs;
    std::vector<int> unused, bmap;
    push_pack_desc(descs, unused, bmap, cv);
    hipStream_t s = (hipStream_t)stream;
    DevTables t;
    HCHECK(t.upload(descs, bmap, s));
    LCHECK(vpd_launch_unpack_grads(t.descs, (int)descs.size(), t.bmap, (int)bmap.size() / 2, wg, grads_out, s));
    HCHECK(hipStreamSynchronize(s));
    return 0;
}

namespace {
// the descriptors and the block map of vpd_op_adamw_pack's synthetic buffer (0, or fail())
int op_adam_tables(int nconv, const int* dims3, const long long* offsets, long long numel, const void* arena, const float* wg,
                   std::vector<PackDesc>& descs, std::vector<int>& bmap_adam) {
    if (nconv > 0 && (!dims3 || !offsets)) return fail("null argument");
    if (nconv < 0 || nconv > 64) return fail("nconv outside 0..64");
    if (numel < 4 || numel % 4) return fail("numel must be a positive multiple of 4");
    if (!aligned(arena, 16) || !aligned(wg, 16)) return fail("arena and wg must be 16-byte aligned");
    std::vector<int> bmap_pack, unused;
    long long arena_at = 0, wg_at = 0, prev_end = 0;
    for (int i = 0; i < nconv; ++i) {
        const int Co = dims3[3 * i], Ci = dims3[3 * i + 1], k = dims3[3 * i + 2];
        if (const char* e = op_conv_shape_error(Co, Ci, k, 0)) return fail(e);
        const long long ns = (long long)Co * Ci * k * k;
        // (adamw_pack_kernel reads and writes a conv's OIHW rows 16 bytes at a time and has no unaligned fallback)
        if (offsets[i] % 4) return fail("a conv's offset must be a multiple of 4 floats");
        if (offsets[i] < prev_end || offsets[i] + ns > numel) return fail("conv ranges must ascend, not overlap and lie inside numel");
        prev_end = offsets[i] + ns;
        ConvInfo cv;
        set_pack_geom(cv, Ci, Co, k, false);
        cv.w_off = offsets[i];
        cv.fwd_off = arena_at; cv.dgr_off = arena_at + ns; arena_at += 2 * ns;      // as add_conv lays the arena out
        cv.wg_off = wg_at; wg_at += ns;
        push_pack_desc(descs, bmap_pack, unused, cv);
    }
    int nstem = 0;
    build_adam_map(descs, bmap_pack, -1, numel, bmap_adam, nstem);
    return 0;
}
}  // namespace

extern "C" int vpd_op_adamw_pack(int nconv, const int* dims3, const long long* offsets, long long numel, float* params,
                                 const float* grads, float* adam_m, float* adam_v, void* arena, const float* wg, double lr,
                                 double beta1, double beta2, double eps, double weight_decay, int step, float gscale,
                                 void* stream) {
    if (!params || !grads || !adam_m || !adam_v || !arena) return fail("null argument");
    if (step < 1) return fail("step is 1-based");
    std::vector<PackDesc> descs;
    std::vector<int> bmap_adam;
    if (op_adam_tables(nconv, dims3, offsets, numel, arena, wg, descs, bmap_adam)) return -1;
    hipStream_t s = (hipStream_t)stream;
    DevTables t;
    HCHECK(t.upload(descs, bmap_adam, s));
    LCHECK(vpd_launch_adamw_pack(t.descs, t.bmap, (int)bmap_adam.size() / 2, params, grads, adam_m, adam_v, (bf16_t*)arena,
                                 AdamArgs{lr, beta1, beta2, eps, weight_decay, step, gscale, nullptr}, s, wg));
    HCHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int vpd_op_adamw_pack_groups(int nconv, const int* dims3, const long long* offsets, long long numel, float* params,
                                        const float* grads, float* adam_m, float* adam_v, void* arena, const float* wg,
                                        const long long* seg_begin, const int* seg_group, int nseg, const double* lr,
                                        const double* weight_decay, int ngroups, double beta1, double beta2, double eps, int step,
                                        float gscale, const vpd_scale_state* state, void* stream) {
    if (!params || !grads || !adam_m || !adam_v || !arena) return fail("null argument");
    std::vector<PackDesc> descs;
    std::vector<int> bmap_adam;
    if (op_adam_tables(nconv, dims3, offsets, numel, arena, wg, descs, bmap_adam)) return -1;
    if (adam_group_args_check(lr, weight_decay, ngroups, step, state)) return -1;
    if (adam_groups_check(seg_begin, seg_group, nseg, numel, ngroups)) return -1;
    if (adam_groups_check_convs(descs, seg_begin, nseg)) return -1;
    hipStream_t s = (hipStream_t)stream;
    DevTables t;
    struct Table { void* p = nullptr; ~Table() { (void)hipFree(p); } } table;
    HCHECK(hipMalloc(&table.p, vpd_adam_table_bytes(nseg)));
    if (adam_groups_upload(table.p, seg_begin, seg_group, nseg, ngroups, s)) return -1;
    HCHECK(t.upload(descs, bmap_adam, s));
    LCHECK(vpd_launch_adamw_pack_groups(t.descs, t.bmap, (int)bmap_adam.size() / 2, params, grads, adam_m, adam_v, (bf16_t*)arena,
                                        AdamGroupArgs{table.p, lr, weight_decay, ngroups, beta1, beta2, eps, step, gscale, state}, s,
                                        wg));
    HCHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int vpd_op_wgrad_reduce(int nprob, const float* const* slabs, float* const* dws, const long long* nfloats,
                                   const int* ksplits, void* stream) {
    if (!slabs || !dws || !nfloats || !ksplits) return fail("null argument");
    if (nprob < 1 || nprob > vpd_wgrad_reduce_max()) return fail("nprob outside 1..18");
    for (int i = 0; i < nprob; ++i) {
        if (!slabs[i] || !dws[i]) return fail("null argument");
        if (nfloats[i] < 4 || nfloats[i] % 4 || ksplits[i] < 1) return fail("a problem needs a positive multiple of 4 floats and ksplit >= 1");
        if (!aligned(slabs[i], 16) || !aligned(dws[i], 16)) return fail("slabs and dws must be 16-byte aligned");
    }
    LCHECK(vpd_launch_wgrad_reduce(nprob, slabs, dws, nfloats, ksplits, (hipStream_t)stream));
    return 0;
}

extern "C" int vpd_op_zero_ranges(float* const* ptrs, const long long* n4s, int count, void* stream) {
    if (count < 0 || count > ZR_MAX) return fail("count outside 0..16");
    if (count == 0) return 0;
    if (!ptrs || !n4s) return fail("null argument");
    ZeroRanges z;
    memset(&z, 0, sizeof z);
    for (int i = 0; i < count; ++i) {
        if (!ptrs[i]) return fail("null argument");
        if (n4s[i] < 0 || !aligned(ptrs[i], 16)) return fail("ranges must be 16-byte aligned, lengths not negative");
        z.ptr[i] = ptrs[i]; z.n4[i] = (long)n4s[i];
    }
    z.count = count;
    LCHECK(vpd_launch_zero_ranges(z, (hipStream_t)stream));
    return 0;
}
