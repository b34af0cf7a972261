"""Plain float64 PyTorch references, input generators and derived error bounds shared by the operator parity tests
(test_stem_ops_gpu.py, test_bn_backward_ops_gpu.py, test_head_ops_gpu.py, test_conv_ops_gpu.py, test_bneck_tail_ops_gpu.py,
test_boundary_ops_gpu.py).  Nothing here touches the GPU or the library:
tests/test_opref_cpu.py pins what these references rest on, so that a failure on the GPU points at the kernel."""
import math

import torch
import torch.nn.functional as F

# element type -> (torch dtype, significand bits including the hidden one, log2 of the smallest positive value)
ELEM = {"bf16": (torch.bfloat16, 8, -133), "fp16": (torch.float16, 11, -24)}
BN_EPS = 1e-5


def elem_round(t, name):
    """round to the element type, back to float32 (what the existing tests do with bf16_round)"""
    return t.to(ELEM[name][0]).to(torch.float32)


def ulp(x, name):
    """spacing of the element type at |x| (float64 tensor in, float64 out); the subnormal spacing below the normal range"""
    _, p, emin = ELEM[name]
    e = torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -300)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - (p - 1)).clamp_min(emin))


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------
# stem: BatchNorm + ReLU + MaxPool 3x3 s2 p1
# ---------------------------------------------------------------------------
STEM_FWD_SHAPES = {"g64": (3, 64, 64), "g32": (8, 32, 32), "odd": (5, 33, 31), "e48": (4, 48, 48)}
STEM_BIG = (512, 64, 64)                     # 512 * 32 * 16 * 8 = 2^21 items in the pair kernel: the 64-bit division path
STEM_BWD_SHAPES = {"g64": (3, 64, 64), "g32": (8, 32, 32), "odd": (5, 33, 31), "e48": (4, 48, 48), "odd2": (2, 17, 35)}
STEM_C = 64
REGIMES = ("init", "drift")


def stem_grid_inputs(n, H, W, C, seed):
    """z = k/16 (|k| <= 127), scale in {0.5 .. 1.5}, shift = j/8 (|j| <= 16): z * scale + shift is exact in fp32, the result
    is representable in bf16 and fp16 only sometimes -- but its rounding is the same single rounding from an exact value in
    fp32 and in float64 -- and 3x3 windows tie all the time"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randint(-127, 128, (n, C, H, W), generator=g).float() / 16.0
    scale = torch.tensor([0.5, 0.75, 1.0, 1.25, 1.5])[torch.randint(0, 5, (C,), generator=g)]
    shift = torch.randint(-16, 17, (C,), generator=g).float() / 8.0
    return z, scale, shift


def stem_params(C, regime, g):
    """init: gamma in [0.5, 1.5], beta ~ 0.3 N(0, 1); drift: |gamma| in [0.05, 1.5] of either sign, beta in [-1, 1]"""
    if regime == "init":
        return torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    mag = 0.05 + 1.45 * torch.rand(C, generator=g)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    return mag * sign, torch.rand(C, generator=g) * 2.0 - 1.0


def stem_stats(z):
    zd = z.double()
    mean = zd.mean(dim=(0, 2, 3))
    rstd = (zd.var(dim=(0, 2, 3), unbiased=False) + BN_EPS).rsqrt()
    return mean, rstd


def stem_random_inputs(n, H, W, C, seed, name, regime="init"):
    """element-rounded randn z, fp32 gamma / beta, float64 batch statistics and the fp32 (mean, rstd, scale, shift) the kernels get"""
    g = torch.Generator().manual_seed(seed)
    z = elem_round(torch.randn(n, C, H, W, generator=g) * 1.3 - 0.2, name)
    gamma, beta = stem_params(C, regime, g)
    mean, rstd = stem_stats(z)
    scale = gamma.double() * rstd
    shift = beta.double() - mean * scale
    return {"z": z, "gamma": gamma, "beta": beta, "mean": mean, "rstd": rstd, "scale": scale.float(), "shift": shift.float(), "gen": g}


def taps_from_flat(flat, W):
    """torch's flat arg-max index (y * W + x of the input plane) -> window tap r * 3 + t of a 3x3 s2 p1 pooling"""
    Ho, Wo = flat.shape[-2:]
    oy = torch.arange(Ho).view(Ho, 1)
    ox = torch.arange(Wo).view(1, Wo)
    r = flat // W - (2 * oy - 1)
    t = flat % W - (2 * ox - 1)
    return r * 3 + t


def stem_forward_ref(z, scale, shift, name):
    """float64: a = elem(relu(z * scale + shift)) per pixel, then max_pool2d(3, 2, 1) with torch's first-maximum indices.
    Returns pooled [n,C,Ho,Wo] float64, taps (int64, r*3+t), a."""
    a = (z.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).clamp_min(0)
    a = a.to(ELEM[name][0]).double()
    p, fi = F.max_pool2d(a, 3, 2, 1, return_indices=True)
    return p, taps_from_flat(fi, z.shape[3]), a


def first_max_loop(a):
    """literal row-major scan of every 3x3 s2 p1 window of a [H][W] plane: value and tap of the FIRST maximum"""
    H, W = a.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    val = torch.empty(Ho, Wo, dtype=a.dtype)
    tap = torch.empty(Ho, Wo, dtype=torch.int64)
    for oy in range(Ho):
        for ox in range(Wo):
            best, bi = -math.inf, 0
            for r in range(3):
                for t in range(3):
                    y, x = 2 * oy - 1 + r, 2 * ox - 1 + t
                    if 0 <= y < H and 0 <= x < W and float(a[y, x]) > best:
                        best, bi = float(a[y, x]), r * 3 + t
            val[oy, ox], tap[oy, ox] = best, bi
    return val, tap


def stem_dpool(inp, name):
    """an incoming gradient correlated with the pooled xhat, so that the mean(g * xhat) term carries weight"""
    z = inp["z"].double()
    xhat = (z - inp["mean"].view(1, -1, 1, 1)) * inp["rstd"].view(1, -1, 1, 1)
    px = F.max_pool2d(xhat, 3, 2, 1)
    return elem_round(torch.randn(px.shape, generator=inp["gen"]) + 0.9 * px.float() + 0.3, name)


def stem_backward_ref_A(z, gamma, beta, dpool):
    """independent: float64 autograd of max_pool2d(relu(batch_norm(z, training=True)), 3, 2, 1) contracted with dpool.
    Returns dz, dgamma, dbeta and torch's own window taps."""
    zt = z.double().requires_grad_(True)
    gt = gamma.double().requires_grad_(True)
    bt = beta.double().requires_grad_(True)
    a = F.batch_norm(zt, None, None, gt, bt, training=True, eps=BN_EPS).clamp_min(0)
    p, fi = F.max_pool2d(a, 3, 2, 1, return_indices=True)
    (p * dpool.double()).sum().backward()
    return zt.grad, gt.grad, bt.grad, taps_from_flat(fi, z.shape[3])


def route(dpool, taps, H, W):
    """g[y][x] = sum of dpool over the windows whose tap points at (y, x)"""
    n, C, Ho, Wo = dpool.shape
    oy = torch.arange(Ho).view(Ho, 1)
    ox = torch.arange(Wo).view(1, Wo)
    flat = (2 * oy - 1 + taps // 3) * W + (2 * ox - 1 + taps % 3)
    g = torch.zeros(n, C, H * W, dtype=torch.float64)
    g.scatter_add_(2, flat.view(n, C, -1), dpool.double().reshape(n, C, -1))
    return g.view(n, C, H, W)


def stem_backward_ref_B(z, gamma, beta, mean, rstd, dpool, taps):
    """closed form, routed by the given taps: g = route(dpool) * [a > 0], dz = gamma rstd (g - mean(g) - xhat mean(g xhat))"""
    n, C, H, W = z.shape
    v = lambda t: t.double().view(1, -1, 1, 1)
    xhat = (z.double() - v(mean)) * v(rstd)
    a = v(gamma) * xhat + v(beta)
    routed = route(dpool, taps, H, W)
    g = routed * (a > 0)
    M = n * H * W
    s1, s2 = g.sum(dim=(0, 2, 3)), (g * xhat).sum(dim=(0, 2, 3))
    dz = v(gamma) * v(rstd) * (g - v(s1) / M - xhat * v(s2) / M)
    return {"dz": dz, "dgamma": s2, "dbeta": s1, "g": g, "routed": routed, "xhat": xhat, "a": a,
            "abs1": g.abs().sum(dim=(0, 2, 3)), "abs2": (g * xhat).abs().sum(dim=(0, 2, 3))}


def relu_band(z, scale, shift, a):
    """elements whose ReLU mask an fp32 evaluation of z * scale + shift could flip: |a| < 2^-20 (|z scale| + |shift|)"""
    v = lambda t: t.double().view(1, -1, 1, 1)
    return a.abs() < 2.0 ** -20 * ((z.double() * v(scale)).abs() + v(shift).abs())


SUM_TOL = 2e-5            # sums kept in fp32 partials, combined in fp64 (test_conv_epilogue_batchnorm_sums)
BAND_CAP = 1e-5           # share of elements that may be left out of a per-element comparison


def dz_l2_gate(name):
    """rel-L2 gate of an element-type dz: 3e-3 for bf16 (test_batchnorm_backward_op_matches_autograd), scaled by the ratio of the half-ulps"""
    return 3e-3 * 2.0 ** (ELEM["bf16"][1] - ELEM[name][1])


def bn_dz_bound(ref_dz, gamma, rstd, mean, z, g, xhat, s1, s2, ds1, ds2, M, name):
    """per-element bound on an element-type dz = c1 (g - c2 - xhat c3): one output ulp, the propagated error bounds of the two
    sums (ds1, ds2, per channel), and the fp32 evaluation itself -- eight roundings of 2^-24 relative to the magnitudes that
    enter (xhat from the fp32 mean / rstd included: (|z| + |mean|) rstd in place of |xhat|)"""
    v = lambda t: t.double().view(1, -1, 1, 1)
    c1 = (v(gamma) * v(rstd)).abs()
    prop = c1 * (v(ds1) + xhat.abs() * v(ds2)) / M
    xmag = (z.double().abs() + v(mean).abs()) * v(rstd)
    f32 = 8 * 2.0 ** -24 * c1 * (g.abs() + v(s1).abs() / M + xmag * v(s2).abs() / M)
    return ulp(ref_dz, name) + prop + f32


# ---------------------------------------------------------------------------
# BatchNorm backward (the construction of test_batchnorm_backward_op_matches_autograd)
# ---------------------------------------------------------------------------
def bn_backward_case(n, h, w, c, seed, name, relu=True, residual=False, autograd=True):
    """z, a dy correlated with xhat, gamma / beta; float64 autograd of relu?(batch_norm(z) (+ res)) contracted with dy.
    residual: the activation (and with it the mask) includes a residual, as at a block output.  autograd=False (the large
    cases): the closed form instead, which test_opref_cpu.py holds equal to autograd to 1e-12."""
    g = torch.Generator().manual_seed(seed)
    z = elem_round(torch.randn(n, c, h, w, generator=g) * 1.3 - 0.2, name)
    zn = (z - z.mean(dim=(0, 2, 3), keepdim=True)) / z.std(dim=(0, 2, 3), keepdim=True)
    dy = elem_round(torch.randn(n, c, h, w, generator=g) + 0.9 * zn + 0.3, name)
    del zn
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    res = elem_round(torch.randn(n, c, h, w, generator=g), name) if residual else None
    mean, rstd = stem_stats(z)
    out = {"z": z, "dy": dy, "gamma": gamma, "beta": beta, "mean": mean, "rstd": rstd, "gen": g}
    if autograd:
        zt = z.double().requires_grad_(True)
        gt = gamma.double().requires_grad_(True)
        bt = beta.double().requires_grad_(True)
        y = F.batch_norm(zt, None, None, gt, bt, training=True, eps=BN_EPS)
        if residual:
            y = y + res.double()
        act = y.clamp_min(0) if relu else y
        (act * dy.double()).sum().backward()
        y = y.detach()
        out.update(dz=zt.grad, dgamma=gt.grad, dbeta=bt.grad)
    else:
        v = lambda t: t.double().view(1, -1, 1, 1)
        y = (z.double() - v(mean)) * v(rstd) * v(gamma) + v(beta)
        if residual:
            y = y + res.double()
    mask = (y > 0) if relu else torch.ones_like(y, dtype=torch.bool)
    out.update(mask=mask, act=(y.clamp_min(0) if relu else y))
    if not autograd:
        gm = dy.double() * mask
        xhat = (z.double() - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)
        out.update(dz=bn_dz_closed_form(z, gamma, mean, rstd, gm), dgamma=(gm * xhat).sum(dim=(0, 2, 3)), dbeta=gm.sum(dim=(0, 2, 3)))
    return out


def bn_dz_closed_form(z, gamma, mean, rstd, gm, c3_factor=1.0):
    """dz = gamma rstd (g - mean(g) - c3_factor xhat mean(g xhat)) in float64; c3_factor = 1.02: the resolution check's faulty reference"""
    v = lambda t: t.double().view(1, -1, 1, 1)
    xhat = (z.double() - v(mean)) * v(rstd)
    gm = gm.double()
    return v(gamma) * v(rstd) * (gm - gm.mean(dim=(0, 2, 3), keepdim=True)
                                 - c3_factor * xhat * (gm * xhat).mean(dim=(0, 2, 3), keepdim=True))


def bn_case_with_mask(cs, mask):
    """the case's reference for another ReLU mask (the sign of the STORED activation: a positive value below the element type's
    smallest one is stored as zero), by the closed form"""
    if torch.equal(mask, cs["mask"]):
        return cs
    v = lambda t: t.double().view(1, -1, 1, 1)
    gm = cs["dy"].double() * mask
    xhat = (cs["z"].double() - v(cs["mean"])) * v(cs["rstd"])
    out = dict(cs)
    out.update(mask=mask, dz=bn_dz_closed_form(cs["z"], cs["gamma"], cs["mean"], cs["rstd"], gm),
               dgamma=(gm * xhat).sum(dim=(0, 2, 3)), dbeta=gm.sum(dim=(0, 2, 3)))
    return out


def mask_bits(mask_bool):
    """[M][C] bool -> [M][C/8] bytes, bit j of byte (m, c8) = element (m, 8 c8 + j)"""
    m, c = mask_bool.shape
    w = (2 ** torch.arange(8, dtype=torch.int32)).view(1, 1, 8)
    return (mask_bool.view(m, c // 8, 8).to(torch.int32) * w).sum(dim=2).to(torch.uint8)


# ---------------------------------------------------------------------------
# head (fp32): integer inputs whose sums stay below 2^24 are exact in any order of additions
# ---------------------------------------------------------------------------
def int_matrix(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# (M, N, K, ta, tb, bias, relu): every call shape of the train step's head -- forward fc (tb = 1; feat 512 / 2048; D 32 / 128 / a
# ragged 40), the motion MLP (K = 32 falls back to sgemm_small_kernel), backward weight gradients (ta = 1, K = the batch) and
# data gradients (ta = tb = 0)
def sgemm_cases():
    cases = []
    for n in (1, 5, 17, 256, 1000):
        for feat, D in ((512, 32), (512, 128), (2048, 40), (2048, 128)):
            if n in (256, 1000) and feat == 2048 and D == 40:
                continue
            cases.append(("fc_n%d_f%d_d%d" % (n, feat, D), n, D, feat, 0, 1, 1, 0))
        for D in (32, 128, 40):
            cases.append(("mlp0_n%d_d%d" % (n, D), n, 128, D, 0, 1, 1, 1))
            cases.append(("mlp2_n%d_d%d" % (n, D), n, 2 * D, 128, 0, 1, 1, 0))
        cases.append(("mlp1_n%d" % n, n, 128, 128, 0, 1, 1, 1))
    for k in (5, 6, 37, 256, 1000):                       # backward: K = the batch
        cases.append(("wg_fc_k%d" % k, 32, 512, k, 1, 0, 0, 0))
        cases.append(("wg_mlp2_k%d" % k, 80, 128, k, 1, 0, 0, 0))
        cases.append(("wg_mlp0_k%d" % k, 128, 40, k, 1, 0, 0, 0))
        cases.append(("dg_fc_n%d" % k, k, 512, 40, 0, 0, 0, 0))
        cases.append(("dg_mlp_n%d" % k, k, 128, 256, 0, 0, 0, 0))
    return cases


def sgemm_operands(case, g, integer):
    _, M, N, K, ta, tb, bias, relu = case
    if integer:
        # |a|, |b| <= 7: |sum| <= 49 K + 64 < 2^24 for every K here (K <= 2048)
        A, B = int_matrix((M, K), -7, 7, g), int_matrix((K, N), -7, 7, g)
        bv = int_matrix((N,), -64, 64, g) if bias else None
    else:
        A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
        bv = torch.randn(N, generator=g) if bias else None
    return A, B, bv


MSE_SIZES = (4, 7, 1023, 4096, 32768, 32771, 128000)


def mse_int_operands(n, g):
    """integer e, t with |e - t| <= 6: sum d^2 <= 36 * 128000 < 2^24, two calls accumulated < 2^24 as well"""
    t = int_matrix((n,), -100, 100, g)
    return t + int_matrix((n,), -6, 6, g), t


# ---------------------------------------------------------------------------
# convolution family (tests/test_conv_ops_gpu.py, tests/conv_ops_child.py)
# ---------------------------------------------------------------------------
# Shapes are chosen by the kernel class vpd_launch_conv gives them on a 256-CU device; the GPU test asserts that class through
# vpd_op_conv2d_dispatch before it launches.  blk_px: the most pixels ONE block accumulates statistics over in any run of the
# case (tiles per block x tile pixels; few-blocks runs included), which bounds the fp32 per-block partial sums.
#            crops Ci   Co   H   W  k stride
CONV_CASES = {
    "c0_w32":        dict(n=64,  ci=64,  co=64,  h=32, w=32, blk_px=2 * 128, wgrad="no_group"),   # layer1's rows: 512 tiles, two per block; eval: 256 tiles of c64x2
    "c0_w16":        dict(n=203, ci=64,  co=64,  h=16, w=16, blk_px=2 * 128),       # 406 tiles of half an image
    # c0_w32 again for a budget of 16 CUs (VPD_RESERVE_CUS=240): 32 tiles per block (eval: 16 of c64x2), every halo buffer reused
    "c0_w32_walk":   dict(n=64,  ci=64,  co=64,  h=32, w=32, blk_px=32 * 128, wgrad="no_group"),
    "c1_w16":        dict(n=203, ci=128, co=128, h=16, w=16, blk_px=9 * 256),       # 203 tiles of one image each: 256 x 128 with VPD_PWS=0 or few blocks
    "c1_w16_device": dict(n=300, ci=128, co=128, h=16, w=16, blk_px=2 * 256),       # 300 > 256 tiles: the eight-wave persistent kernel, two tiles per block
    "c6_w16":        dict(n=150, ci=128, co=128, h=16, w=16, blk_px=7 * 256, wgrad=True),  # 150 < 200 tiles of 256 x 128: 256 x 64, 128 lanes x 2 channel tiles
    "c6_w8_ragged":  dict(n=203, ci=256, co=256, h=8,  w=8,  blk_px=9 * 256),       # 50.75 tiles of four images x 4 channel tiles
    "c6_w8_device":  dict(n=300, ci=256, co=256, h=8,  w=8,  blk_px=2 * 256),       # 75 tiles on 64 lanes
    "c2_w4_ragged":  dict(n=403, ci=512, co=512, h=4,  w=4,  blk_px=9 * 128),       # 50.4 tiles of eight images x 4 channel tiles
    "c3_w4":         dict(n=37,  ci=512, co=512, h=4,  w=4,  blk_px=2 * 128, wgrad=True),   # 4.6 tiles x 8 channel tiles
    "c3_w4_device":  dict(n=320, ci=512, co=512, h=4,  w=4,  blk_px=2 * 128),       # 40 tiles on 32 lanes
    "c3_two_chunks": dict(n=21,  ci=128, co=128, h=4,  w=4,  blk_px=3 * 128),       # two 64-channel chunks: 18 K-steps per tile
    # stride 2 at the stage boundaries: the forward is the ring GEMM's, the data gradient four parity classes of conv_igemm_kernel
    # in its three tile shapes (128 x 64: 64 output channels; 64 x 64: few tiles; 128 x 128: 384 tiles and more)
    "s2_w32":        dict(n=100, ci=64,  co=128, h=32, w=32, stride=2, blk_px=256, wgrad=True),
    "s2_w8":         dict(n=5,   ci=256, co=512, h=8,  w=8,  stride=2, blk_px=256),
    "s2_w16_big":    dict(n=768, ci=128, co=256, h=16, w=16, stride=2, blk_px=256),
    # stem (class 5, conv_stem_persistent_kernel): 7x7 stride 2 on the 5-channel input at the student's real size, 512 tiles of two
    # output rows, two per block; and a 32 x 32 input (eight output rows per tile)
    "stem_w128":     dict(n=16,  ci=5,   co=64,  h=128, w=128, k=7, stride=2, stem=True, blk_px=2 * 128),
    "stem_w32":      dict(n=6,   ci=5,   co=64,  h=32, w=32, k=7, stride=2, stem=True, blk_px=128, wgrad="stem"),
    "stem_w128_walk": dict(n=16, ci=5,   co=64,  h=128, w=128, k=7, stride=2, stem=True, blk_px=32 * 128),   # 16 CUs: 32 tiles per block
    # 1x1 ring GEMM (conv1x1_ws_kernel): K = 512, 200 tiles of 256 x 128
    "ring_1x1":      dict(n=50,  ci=512, co=128, h=32, w=32, k=1, blk_px=256),
    # 1x1 streaming kernel (conv1x1_stream_kernel).  st_*: sized for a budget of 8 CUs (VPD_RESERVE_CUS=248: 8 pixel lanes, eligible
    # from 16 pixel tiles), so that every block walks more tiles than its LDS ring has stages; the forward takes the instantiation of
    # (ci, co), the data gradient that of (co, ci).  blk_px = tiles per block x tile pixels
    "st_64_64":      dict(n=67,  ci=64,  co=64,  h=8,  w=16, k=1, blk_px=9 * 128),      # 67 tiles of one image, 9 per block
    "st_64_128":     dict(n=67,  ci=64,  co=128, h=8,  w=16, k=1, blk_px=9 * 128),
    "st_64_256":     dict(n=93,  ci=64,  co=256, h=8,  w=8,  k=1, blk_px=12 * 64),      # 93 tiles of one image, 12 per block
    "st_64_256_w16": dict(n=23,  ci=64,  co=256, h=16, w=16, k=1, blk_px=12 * 64),      # four-row tiles, four tiles per image
    "st_128_128":    dict(n=67,  ci=128, co=128, h=8,  w=16, k=1, blk_px=9 * 128),
    "st_128_256":    dict(n=93,  ci=128, co=256, h=8,  w=8,  k=1, blk_px=12 * 64),      # (data gradient: 186 tiles of 32 pixels, 24 per block)
    "st_256_512_s2": dict(n=47,  ci=256, co=512, h=16, w=32, k=1, stride=2, blk_px=24 * 32),   # 188 tiles of two output rows
    "st_64_256_w32": dict(n=40,  ci=64,  co=256, h=32, w=32, k=1, blk_px=3 * 64),       # the whole device: 640 tiles on 256 lanes
}
for _c in CONV_CASES.values():
    _c.setdefault("k", 3)
    _c.setdefault("stride", 1)
CONV_SEEDS = (11,)
CONV_ZMAX = 3                      # |z|, |old|, |res|, |shift| of the integer regime


def conv_geom(cs):
    k, st = cs["k"], cs["stride"]
    pad = k // 2
    ho, wo = (cs["h"] + 2 * pad - k) // st + 1, (cs["w"] + 2 * pad - k) // st + 1
    return k, st, pad, ho, wo


def _sparse_int(shape, density, g, lo=1):
    """integers: 0 with probability 1 - density, else +-1 .. +-lo"""
    v = torch.randint(1, lo + 1, shape, generator=g).double() * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return v * (torch.rand(shape, generator=g) < density)


def conv_operands(cs, seed, regime, name="bf16"):
    """x, w, dz and the epilogue operands (NCHW, float64 values that the element type holds exactly).
    integer: x, dz in {-1, 0, 1} with density 1/2, w in {-1, 0, 1} with density 288 / K (K = taps x the larger channel count:
    a sum of K products has standard deviation 12, 2^8 is beyond twenty sigma), old / res / z / shift integers up to CONV_ZMAX,
    scale 1 or 2.  random: randn rounded to the element type, He-scaled weights, scale in [0.5, 1.5]."""
    k, st, pad, ho, wo = conv_geom(cs)
    n, ci, co, h, w = cs["n"], cs["ci"], cs["co"], cs["h"], cs["w"]
    g = torch.Generator().manual_seed(seed * 1000 + n + ci + h)
    o = {}
    if regime == "int":
        dens = min(0.5, 288.0 / (k * k * (ci if cs.get("stem") else max(ci, co))))
        o["x"], o["dz"] = _sparse_int((n, ci, h, w), 0.5, g), _sparse_int((n, co, ho, wo), 0.5, g)
        o["w"] = _sparse_int((co, ci, k, k), dens, g)
        small = lambda shape: torch.randint(-CONV_ZMAX, CONV_ZMAX + 1, shape, generator=g).double()
        o["scale"] = torch.randint(0, 2, (co,), generator=g).double() + 1.0
        o["shift"] = small((co,))
        er = lambda t: t
    else:
        er = lambda t: elem_round(t, name).double()
        o["x"], o["dz"] = er(torch.randn(n, ci, h, w, generator=g)), er(torch.randn(n, co, ho, wo, generator=g))
        o["w"] = er(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
        small = lambda shape: er(torch.randn(shape, generator=g))
        o["scale"] = (torch.rand(co, generator=g) + 0.5).float().double()
        o["shift"] = (torch.randn(co, generator=g) * 0.3).float().double()
    # forward side (output [n, co, ho, wo]): residual, old value; data-gradient side (output [n, ci, h, w]): old value, z, z2
    o["res"], o["old_y"] = small((n, co, ho, wo)), small((n, co, ho, wo))
    o["old_dx"], o["z"], o["z2"] = small((n, ci, h, w)), small((n, ci, h, w)), small((n, ci, h, w))
    o["keep_y"] = torch.rand((n, co, ho, wo), generator=g) > 0.4          # ReLU bit maps
    o["keep_dx"] = torch.rand((n, ci, h, w), generator=g) > 0.4
    return o


def conv_fwd(x, w, cs):
    k, st, pad, _, _ = conv_geom(cs)
    return F.conv2d(x.double(), w.double(), None, stride=st, padding=pad)


def conv_dgrad(dz, w, cs):
    k, st, pad, ho, wo = conv_geom(cs)
    oph, opw = cs["h"] - ((ho - 1) * st + k - 2 * pad), cs["w"] - ((wo - 1) * st + k - 2 * pad)
    return F.conv_transpose2d(dz.double(), w.double(), None, stride=st, padding=pad, output_padding=(oph, opw))


def conv_wgrad(x, dz, cs):
    k, st, pad, _, _ = conv_geom(cs)
    return torch.nn.grad.conv2d_weight(x.double(), (cs["co"], cs["ci"], k, k), dz.double(), stride=st, padding=pad)


def conv_eval_ep(conv, o, res, relu):
    v = lambda t: t.double().view(1, -1, 1, 1)
    y = conv * v(o["scale"]) + v(o["shift"])
    if res:
        y = y + o["res"]
    return y.clamp_min(0) if relu else y


# The MFMA accumulator.  Products of two element-type values are exact in fp32 (8 + 8 or 11 + 11 significand bits).  Nothing
# public states that the bf16 / fp16 MFMA of gfx950 rounds every internal addition to nearest, so the bound assumes the weaker
# thing a hardware adder tree can do: each of the K additions (and the few that join partial accumulators: + 4) may TRUNCATE,
# losing up to one ulp = 2^-23 of a partial sum whose magnitude conv(|x|, |w|) bounds.  c = 2 against round-to-nearest's 1.
CONV_ACC_C = 2.0


def conv_gamma(mag, K):
    return CONV_ACC_C * (K + 4) * 2.0 ** -24 * mag


def conv_bound(ref, gamma, name, extra=0.0):
    """|got - ref| <= half an element ulp at |ref| + what the fp32 value may be off by, + that; extra: the epilogue's own fp32 terms"""
    gm = gamma + extra
    return 0.5 * ulp(ref.abs() + gm, name) + gm


def conv_alter_tap(ref, x, w, cs, row=None):
    """(i) tap (0, k - 1) left out for the pixels of one output row of image 0"""
    k, st, pad, ho, wo = conv_geom(cs)
    row = ho // 2 if row is None else row
    w1 = torch.zeros_like(w)
    w1[:, :, 0, k - 1] = w[:, :, 0, k - 1]
    out = ref.clone()
    out[0, :, row, :] -= conv_fwd(x[0:1], w1, cs)[0, :, row, :]
    return out


def conv_alter_chunks(ref, x, w, cs):
    """(ii) two neighbouring 64-channel chunks of the weights swapped (fewer than 128 input channels: the two halves), image 0"""
    c = 64 if cs["ci"] >= 128 else cs["ci"] // 2
    w1 = w.clone()
    w1[:, :c], w1[:, c:2 * c] = w[:, c:2 * c], w[:, :c]
    out = ref.clone()
    out[0:1] = conv_fwd(x[0:1], w1, cs)
    return out


def conv_alter_shift(conv, other):
    """(iii) the residual / old value (already masked, where a bit map applies) one pixel to the right"""
    return conv + torch.roll(other, 1, dims=3)


def conv_alter_tile(ref, tile_px, tile=1):
    """(iv) the pixels of one tile (NHWC pixel order) taken from one image further on"""
    n, c, h, w = ref.shape
    flat = nhwc(ref).reshape(n * h * w, c).clone()
    px = min(tile_px, n * h * w - h * w)                 # (a case smaller than two tiles: as many pixels as there are)
    lo = max(0, min(tile * px, n * h * w - px - h * w))
    flat[lo:lo + px] = flat[lo + h * w:lo + h * w + px].clone()
    return nchw(flat.view(n, h, w, c))


# ---------------------------------------------------------------------------
# A Bottleneck's closing 1x1 convolution fused with its BatchNorm (conv1x1_bn_stream_kernel, conv1x1_bn2_stream_kernel;
# tests/test_bneck_tail_ops_gpu.py, tests/bneck_tail_child.py)
# ---------------------------------------------------------------------------
# few: run with a budget of 8 CUs (VPD_RESERVE_CUS=248): 8 pixel lanes walk the 64-pixel tiles, more per block than the ring is
# deep (8 stages for 64 input channels, 5 for 128 and for the two-convolution kernel).  two: the down-sampling block's kernel,
# out = relu(BatchNorm(conv(x)) + BatchNorm2(conv2(x2))), 64 input channels each.
TAIL_CASES = {
    "k64_w8":      dict(n=93, ci=64,  co=256, h=8,  w=8,  few=True),      # 93 tiles, 11-12 per block
    "k64_w16":     dict(n=23, ci=64,  co=256, h=16, w=16, few=True),      # 92 tiles of four rows, four per image
    "k64_co512":   dict(n=93, ci=64,  co=512, h=8,  w=8,  few=True),      # two channel tiles
    "k128_w8":     dict(n=61, ci=128, co=256, h=8,  w=8,  few=True),      # 61 tiles, 7-8 per block
    "k128_co512":  dict(n=61, ci=128, co=512, h=8,  w=8,  few=True),
    "two_w8":      dict(n=61, ci=64,  co=256, h=8,  w=8,  few=True, two=True),
    "two_w16":     dict(n=23, ci=64,  co=256, h=16, w=16, few=True, two=True),
    "k64_w32":     dict(n=40, ci=64,  co=256, h=32, w=32, few=False),     # the whole device: 640 tiles, 2-3 per block
    "k128_w32":    dict(n=40, ci=128, co=256, h=32, w=32, few=False),     # ... on the 5-stage ring: fewer tiles than it runs ahead
    "two_w32":     dict(n=40, ci=64,  co=256, h=32, w=32, few=False, two=True),
}
for _c in TAIL_CASES.values():
    _c.setdefault("two", False)
    _c.update(k=1, stride=1)
TAIL_TILE = 64                     # pixels per tile of both kernels
TAIL_LANES = 8                     # pixel lanes of a few-CU run
BN_MOMENTUM = 0.1
BN_RTOL, BN_MEAN_ATOL = 1e-5, 1e-6          # test_batchnorm_forward_op's gates on mean / rstd / scale / running statistics


def tail_ring(cs):
    return 5 if cs["two"] or cs["ci"] == 128 else 8


def tail_operands(cs, seed, regime, name="bf16"):
    """conv_operands' two regimes for the fused tail: x, w (x2, w2 of the branch), the residual (one-convolution kernel), d(out), a
    random ReLU bit map, fp32 gamma / beta / running statistics per BatchNorm (suffix 2: the branch's)"""
    n, ci, co, h, w = cs["n"], cs["ci"], cs["co"], cs["h"], cs["w"]
    g = torch.Generator().manual_seed(seed * 1000 + n + ci + h + co)
    o = {}
    if regime == "int":
        dens = min(0.5, 288.0 / max(ci, co))
        xs, ws = (lambda: _sparse_int((n, ci, h, w), 0.5, g)), (lambda: _sparse_int((co, ci, 1, 1), dens, g))
        small = lambda shape: torch.randint(-CONV_ZMAX, CONV_ZMAX + 1, shape, generator=g).double()
        o["dout"] = _sparse_int((n, co, h, w), 0.5, g)
    else:
        er = lambda t: elem_round(t, name).double()
        xs, ws = (lambda: er(torch.randn(n, ci, h, w, generator=g))), (lambda: er(torch.randn(co, ci, 1, 1, generator=g) * (2.0 / ci) ** 0.5))
        small = lambda shape: er(torch.randn(shape, generator=g))
        o["dout"] = er(torch.randn(n, co, h, w, generator=g))
    o["x"], o["w"] = xs(), ws()
    if cs["two"]:
        o["x2"], o["w2"] = xs(), ws()
    else:
        o["res"] = small((n, co, h, w))
    o["keep"] = torch.rand((n, co, h, w), generator=g) > 0.4
    for sfx in ("", "2") if cs["two"] else ("",):
        o["gamma" + sfx], o["beta" + sfx] = stem_params(co, "init", g)
        o["rm" + sfx], o["rv" + sfx] = torch.randn(co, generator=g) * 0.1, torch.rand(co, generator=g) + 0.5
    return o


def tail_conv(x, w, name=None):
    """z = conv1x1(x, w) in float64; name: rounded to that element type (the CPU stand-in for the unfused launch's stored z)"""
    z = F.conv2d(x.double(), w.double())
    return z if name is None else z.to(ELEM[name][0]).double()


def _cv(t):
    return t.double().view(1, -1, 1, 1)


def tail_stats(z, gamma, beta, rm, rv):
    """float64: the two rows (sum z, sum z^2), batch statistics, scale / shift, updated running statistics; abs1: sum |z|"""
    M = z.shape[0] * z.shape[2] * z.shape[3]
    s1, s2 = z.sum(dim=(0, 2, 3)), (z * z).sum(dim=(0, 2, 3))
    mean = s1 / M
    var = (s2 / M - mean * mean).clamp_min(0)
    rstd = (var + BN_EPS).rsqrt()
    scale = gamma.double() * rstd
    return {"s1": s1, "s2": s2, "abs1": z.abs().sum(dim=(0, 2, 3)), "M": M, "mean": mean, "var": var, "rstd": rstd, "scale": scale,
            "shift": beta.double() - mean * scale, "gamma": gamma.double(), "beta": beta.double(),
            "rm": (1 - BN_MOMENTUM) * rm.double() + BN_MOMENTUM * mean,
            "rv": (1 - BN_MOMENTUM) * rv.double() + BN_MOMENTUM * var * M / (M - 1)}


def tail_pre(z, st, idx=None):
    """z scale + shift; idx: the channel each channel takes its coefficients from (fault iii)"""
    sc, sh = (st["scale"], st["shift"]) if idx is None else (st["scale"][idx], st["shift"][idx])
    return z * _cv(sc) + _cv(sh)


def tail_pre_err(z, st, exact_rows):
    """What an fp32 evaluation of z scale + shift from fp32 coefficients may be off by, per element.
    Coefficients (bn_finalize_channel): the rows hold sum z and sum z^2 to SUM_TOL of the sums of magnitudes (exact_rows: exactly,
    the integer regime), mean and variance are formed in fp64; then four fp32 roundings on the way to scale (var + eps, the 1-ulp
    reciprocal square root = two half-ulps, the product with gamma) and three more to shift (mean, mean scale, the subtraction).
    Element: the fused multiply-add rounds once (two allowed, on |z scale| + |shift|)."""
    u = 2.0 ** -24
    tol = 0.0 if exact_rows else SUM_TOL
    dmean = tol * st["abs1"] / st["M"]
    dvar = tol * st["s2"] / st["M"] + 2 * st["mean"].abs() * dmean
    dsc = st["gamma"].abs() * 0.5 * st["rstd"] ** 3 * dvar + 4 * u * st["scale"].abs()
    dsh = st["scale"].abs() * (dmean + u * st["mean"].abs()) + st["mean"].abs() * dsc + 2 * u * (st["beta"].abs() + (st["mean"] * st["scale"]).abs())
    return z.abs() * _cv(dsc) + _cv(dsh) + 2 * u * ((z * _cv(st["scale"])).abs() + _cv(st["shift"]).abs())


def tail_out_bound(pre, err, other, name):
    """|stored out - relu(pre)| for pre = (z scale + shift) + other (the residual, or the branch's z2 scale2 + shift2): err = the
    terms' tail_pre_err, one more fp32 addition (two roundings allowed), half an element ulp (|relu(a) - relu(b)| <= |a - b|)"""
    e = err + 2 * 2.0 ** -24 * ((pre - other).abs() + other.abs())
    return 0.5 * ulp(pre.abs() + e, name) + e


def tail_bwd(z, st, gm, idx=None):
    """float64 backward of one BatchNorm for the masked gradient gm: rows (sum g, sum g z), dz in the kernel's form A g + B z + D
    (equal to bn_dz_closed_form: tests/test_opref_cpu.py), dgamma, dbeta and the sums of magnitudes their tolerances scale with"""
    M = st["M"]
    xhat = (z - _cv(st["mean"])) * _cv(st["rstd"])
    r1, r2 = gm.sum(dim=(0, 2, 3)), (gm * z).sum(dim=(0, 2, 3))
    sx = (r2 - st["mean"] * r1) * st["rstd"]
    A = st["gamma"] * st["rstd"]
    B = -A * st["rstd"] * sx / M
    D = -A * r1 / M - B * st["mean"]
    if idx is not None:
        A, B, D = A[idx], B[idx], D[idx]
    return {"r1": r1, "r2": r2, "dz": _cv(A) * gm + _cv(B) * z + _cv(D), "dgamma": sx, "dbeta": r1, "xhat": xhat,
            "abs1": gm.abs().sum(dim=(0, 2, 3)), "abs2": (gm * xhat).abs().sum(dim=(0, 2, 3)), "absz": (gm * z).abs().sum(dim=(0, 2, 3))}


def tail_dz_bound(z, st, gm, b, name):
    """bn_dz_bound for this BatchNorm, the sums good to SUM_TOL of their sums of magnitudes"""
    return bn_dz_bound(b["dz"], st["gamma"], st["rstd"], st["mean"], z, gm, b["xhat"], b["dbeta"], b["dgamma"], SUM_TOL * b["abs1"],
                       SUM_TOL * b["abs2"], st["M"], name)


def tail_forward(cs, o, z, z2, exact_rows, name, idx=None, res=None):
    """the forward chain of a case from z (and the branch's z2): statistics per BatchNorm, out = relu(pre) in float64 and the
    per-element bound of the stored out.  idx: fault (iii); res: another residual (fault v)"""
    st = tail_stats(z, o["gamma"], o["beta"], o["rm"], o["rv"])
    t, err = tail_pre(z, st, idx), tail_pre_err(z, st, exact_rows)
    if cs["two"]:
        st2 = tail_stats(z2, o["gamma2"], o["beta2"], o["rm2"], o["rv2"])
        other, err = tail_pre(z2, st2, idx), err + tail_pre_err(z2, st2, exact_rows)
    else:
        st2, other = None, (o["res"] if res is None else res)
    pre = t + other
    return {"st": st, "st2": st2, "pre": pre, "out": pre.clamp_min(0), "bound": tail_out_bound(pre, err, other, name)}


def tail_backward(cs, o, z, z2, fw, mask, name, idx=None, dout=None):
    """the backward chain under the ReLU map `mask`: per BatchNorm the rows, dz with its bound, dgamma, dbeta"""
    gm = (o["dout"] if dout is None else dout) * mask
    out = {"gm": gm, "b": tail_bwd(z, fw["st"], gm, idx)}
    out["bound"] = tail_dz_bound(z, fw["st"], gm, out["b"], name)
    if cs["two"]:
        out["b2"] = tail_bwd(z2, fw["st2"], gm, idx)
        out["bound2"] = tail_dz_bound(z2, fw["st2"], gm, out["b2"], name)
    return out


def tail_stored_mask(out, name):
    """the forward's own bit map: the stored out is not zero"""
    return out.to(ELEM[name][0]) != 0


# the five faults a streaming kernel can have, as altered inputs of the chain above
def tail_alter_tile(z, lanes, ring, tile=1):
    """(i) one 64-pixel tile (NHWC pixel order) of z computed from the input of the tile ring x lanes further on: a ring stage
    overwritten before it was read (a tensor with fewer tiles: from the last tile)"""
    n, c, h, w = z.shape
    flat = nhwc(z).reshape(n * h * w, c).clone()
    src = min(tile + ring * lanes, n * h * w // TAIL_TILE - 1)
    flat[tile * TAIL_TILE:(tile + 1) * TAIL_TILE] = flat[src * TAIL_TILE:(src + 1) * TAIL_TILE].clone()
    return nchw(flat.view(n, h, w, c))


def tail_alter_chunks(cs, o, name=None):
    """(ii) image 0 with the two 64-channel chunks of the weights swapped (64 input channels: the two halves); two-convolution
    kernel: x and x2 swapped.  -> altered (z, z2)"""
    if cs["two"]:
        return tail_conv(o["x2"], o["w"], name), tail_conv(o["x"], o["w2"], name)
    z = tail_conv(o["x"], o["w"])
    z = conv_alter_chunks(z, o["x"], o["w"], cs)
    return (z if name is None else z.to(ELEM[name][0]).double()), None


def tail_alter_coef(co, c0=8):
    """(iii) channels c0 .. c0 + 3 take their coefficients from 16 channels further on: the index map"""
    idx = torch.arange(co)
    idx[c0:c0 + 4] = torch.arange(c0 + 16, c0 + 20)
    return idx


def tail_alter_mask(mask, tile=1):
    """(iv) the bit map of one tile read 4 channels off"""
    n, c, h, w = mask.shape
    flat = nhwc(mask).reshape(n * h * w, c).clone()
    flat[tile * TAIL_TILE:(tile + 1) * TAIL_TILE] = torch.roll(flat[tile * TAIL_TILE:(tile + 1) * TAIL_TILE], -4, dims=1)
    return nchw(flat.view(n, h, w, c))
# (v) the residual / d(out) one pixel to the right: conv_alter_shift


# ---------------------------------------------------------------------------
# the reference boundary (tests/test_boundary_ops_gpu.py): input packing, weight repack, gradient unpack, AdamW, slab sums, range zeroing
# ---------------------------------------------------------------------------
# sentinel bit patterns no operation here can produce: a NaN with a payload (element buffers; no input is a NaN) and an odd float
SENTINEL_BITS = {"bf16": 0x7FA5, "fp16": 0x7E55}
SENTINEL_F32 = 12345.678


def sentinel_elems(shape, name):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), SENTINEL_BITS[name], dtype=torch.int16).view(ELEM[name][0])


def bits(t):
    """the bit pattern of an element-type or fp32 tensor as integers"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


#                   n  H  W   -> which kernel vpd_launch_pack_input takes (16-byte aligned x)
PACK_INPUT_ROWS = ((3, 4, 64), (2, 8, 128))            # W % 64 == 0 and H W % 256 == 0, C in 3, 5, 6: pack_input_rows_kernel
PACK_INPUT_ROWS_FALLBACK = ((2, 6, 64),)               # W % 64 == 0 but H W % 256 != 0: pack_input_kernel
PACK_INPUT_QUAD = ((3, 5, 12), (2, 7, 20))             # W % 4 == 0: pack_input_kernel<3|5|6>, <0> for C 1, 4, 8
PACK_INPUT_PIXEL = ((2, 5, 31), (1, 3, 33))            # W % 4 != 0: pack_input_px_kernel
PACK_INPUT_MISALIGNED = ((2, 4, 16),)                  # ... and any W behind an x that is not 16-byte aligned
# the quad kernel's items are n H W / 4: below 2^21 the float-reciprocal split (vpd_fdiv), from 2^21 on 64-bit divisions
PACK_INPUT_BELOW = (8097, 37, 28)                      # 2,097,123 items, W / 4 = 7
PACK_INPUT_WORKLOAD = (512, 128, 128)                  # 2^21 pixel quads: the rows kernel at the workload's size
PACK_INPUT_ABOVE = (2400, 30, 120)                     # 2,160,000 items, W % 64 != 0: the quad kernel's 64-bit path
FDIV_MAX = 1 << 21


def pack_input_geoms(H, W):
    """(Hp, Wp, pad): the plan's input geometry and a symmetric one"""
    return ((H + 6, W + 8, 3), (H + 2, W + 2, 1))


def pack_input_values(shape, name, g):
    """randn mixed with what a conversion gets wrong: exact ties of the element type (half-way between two neighbours: round to
    even), +-0, element-type subnormals and their ties, values around and beyond the fp16 maximum (65504; 65520 is the tie that
    rounds to inf), fp32's largest.  Large tensors draw from a pool of 2^20 such values."""
    n = 1
    for s in shape:
        n *= s
    m = min(n, 1 << 20)
    x = torch.randn(m, generator=g)
    kind = torch.randint(0, 16, (m,), generator=g)
    base = elem_round(x, name).double()
    tie = (base + 0.5 * ulp(base, name)).float()                    # p + 1 significand bits: exact in fp32
    x = torch.where(kind == 0, tie, x)
    x = torch.where(kind == 1, torch.zeros(m), x)
    x = torch.where(kind == 2, -torch.zeros(m), x)
    tiny = 2.0 ** ELEM[name][2]
    k = torch.randint(-15, 16, (m,), generator=g).double() * 0.5    # multiples of half the subnormal step
    x = torch.where(kind == 3, (k * tiny).float(), x)
    big = torch.tensor([65504.0, 65519.0, 65520.0, -65520.0, 65536.0, 7.0e4, -1.0e5, 3.4028235e38, -3.0e38, 65488.0, 65512.0])
    x = torch.where(kind == 4, big[torch.randint(0, big.numel(), (m,), generator=g)], x)
    if m < n:
        x = x[torch.randint(0, m, (n,), generator=g)]
    return x.view(shape)


def pack_input_ref(x, Hp, Wp, pad, name):
    """out[b][y + pad][x + pad][c] = elem(x[b][c][y][x]), channels C..7 of those pixels zero; everything else untouched.
    Returns (out [n][Hp][Wp][8] in the element type, zero where untouched; written [n][Hp][Wp] bool)"""
    n, C, H, W = x.shape
    out = torch.zeros(n, Hp, Wp, 8, dtype=ELEM[name][0])
    out[:, pad:pad + H, pad:pad + W, :C] = x.permute(0, 2, 3, 1).to(ELEM[name][0])
    written = torch.zeros(n, Hp, Wp, dtype=torch.bool)
    written[:, pad:pad + H, pad:pad + W] = True
    return out, written


PACK_WEIGHTS_CASES = ((32, 32, 3), (64, 96, 3), (96, 32, 1), (64, 64, 1))      # (Co, Ci, k)
PACK_STEM_CI = (3, 5, 6)
UNPACK_CASES = ((32, 32, 3, 32, 0), (64, 32, 1, 32, 0), (64, 5, 7, 64, 1))     # (Co, Ci, k, Kc, stem): 9 whole chunks; 2; a ragged last one


def stem_rowtap(w, Kc=64):
    """OIHW [Co][c][7][7] -> [r][Co][Kc], entry t * 8 + c (zero elsewhere): the stem's row-tap layout, in w's dtype"""
    Co, Ci, kh, kw = w.shape
    out = torch.zeros(kh, Co, Kc // 8, 8, dtype=w.dtype)
    out[:, :, :kw, :Ci] = w.permute(2, 0, 3, 1)                     # [r][co][t][c]
    return out.view(kh, Co, Kc)


def pack_weights_ref(w, name, stem=False):
    """fp32 OIHW -> (forward layout [tap][Co][Ci], data-gradient layout [tap][Ci][Co]) in the element type, tap = r * k + t.
    The stem: ([r][Co][t * 8 + c] with zero fill for t = 7 and c >= Ci, None)."""
    dt = ELEM[name][0]
    if stem:
        return stem_rowtap(w).to(dt), None
    Co, Ci, k, _ = w.shape
    return (w.permute(2, 3, 0, 1).reshape(k * k, Co, Ci).to(dt).contiguous(),
            w.permute(2, 3, 1, 0).reshape(k * k, Ci, Co).to(dt).contiguous())


def wgrad_scratch_layout(gr, Kc, stem=False, fill=0.0):
    """fp32 OIHW gradient -> the weight-gradient scratch [tap][Co][Kc] (entries ci < Ci; the stem: stem_rowtap), `fill` elsewhere"""
    Co, Ci, k, _ = gr.shape
    if stem:
        out = torch.full((k, Co, Kc // 8, 8), fill, dtype=gr.dtype)
        out[:, :, :k, :Ci] = gr.permute(2, 0, 3, 1)
        return out.view(k, Co, Kc)
    out = torch.full((k * k, Co, Kc), fill, dtype=gr.dtype)
    out[:, :, :Ci] = gr.permute(2, 3, 0, 1).reshape(k * k, Co, Ci)
    return out


def unpack_grads_ref(wg, Co, Ci, k, Kc, stem=False):
    """the inverse on fp32: scratch [tap][Co][Kc] -> OIHW [Co][Ci][k][k]"""
    if stem:
        return wg.view(k, Co, Kc // 8, 8)[:, :, :k, :Ci].permute(1, 3, 0, 2).contiguous()
    return wg.view(k, k, Co, Kc)[:, :, :, :Ci].permute(2, 3, 0, 1).contiguous()


# ---- AdamW ----
U32 = 2.0 ** -24
ADAM_HYPERS = {"torch": dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.01),       # train_vpd_model.py's: torch's defaults
               "strong": dict(lr=1e-2, b1=0.8, b2=0.99, eps=1e-6, wd=0.1)}        # lr wd = 1e-3: a 0.1 % change of wd is 4 u of p
ADAM_STEPS = (1, 2, 3, 1000, 100000)
ADAM_N = 1 << 18                             # elements per regime: 256 blocks of the flat kernel
ADAM_LONG = 4 * (256 * 4096 + 5)             # more than one pass of the flat kernel's capped grid (4096 blocks x 256 float4)


def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0):
    """One AdamW step in float64 from the fp32 operands and the double hyper-parameters, as torch.optim.AdamW states it
    (decoupled decay, lerp of the first moment, denominator sqrt(v) / sqrt(bc2) + eps).  Returns float64 (p', m', v')."""
    p, m, v = p.double(), m.double(), v.double()
    G = g.double() * gscale
    p = p * (1.0 - lr * wd)
    m = m + (G - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * G * G
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * m / denom, m, v


def adamw_bounds(p, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0):
    """Per-element bounds of |fp32 kernel - adamw_ref| for (p', m', v'): first-order running errors of adamw1 (optim.hip), u = 2^-24,
    G = g gscale (exact: gscale is a power of two), one rounding (relative u) per fp32 operation and per double hyper-parameter
    rounded to float; fmaf rounds once, division and square root are correctly rounded, nothing is contracted or reassociated.
      m' = fma(fl(G - m), fl(1 - b1), m): the difference and the factor each put u (1 - b1) |G - m| on the product, the fma u |m'|:
           e_m = u (2 (1 - b1) |G - m| + |m'|).
      v' = fma(fl(fl(1 - b2) G), G, fl(v fl(b2))): both addends are non-negative and carry 2 u each (factor, product), the fma u v':
           e_v = 2 u v' + u v' = 3 u v'.
      p1 = fl(p fl(1 - lr wd)): 2 u |decay p|.
      den = fma(fl(sqrt(v')), fl(1 / sqrt(bc2)), eps): v' is 3 u off, its root 1.5 u, + u (sqrt) + u (factor) on the first addend,
           u (fl(eps)) on the second, u for the fma: at most 4.5 u den.
      p' = fma(-fl(lr / bc1), fl(m' / den), p1): the update U = step_size m' / den carries u (factor) + u (division) + 4.5 u (den)
           relative and step_size / den e_m from m'; the fma u |p'|:
           e_p = u (2 |decay p| + |p'| + step_size / den (2 (1 - b1) |G - m| + 7.5 |m'|)), stated with 8 |m'|.
    Each is multiplied by 1.25 for the second-order terms (products of these, u^2), plus one fp32 subnormal step for results
    that round in the subnormal range."""
    pd, md, vd = p.double(), m.double(), v.double()
    G = g.double() * gscale
    p1, m1, v1 = adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, gscale)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    den = v1.sqrt() / math.sqrt(bc2) + eps
    dm = 2.0 * (1.0 - b1) * (G - md).abs()
    e_m = U32 * (dm + m1.abs())
    e_v = 3.0 * U32 * v1
    e_p = U32 * (2.0 * (pd * (1.0 - lr * wd)).abs() + p1.abs() + (lr / bc1) / den * (dm + 8.0 * m1.abs()))
    sub = 2.0 ** -149
    return 1.25 * e_p + sub, 1.25 * e_m + sub, 1.25 * e_v + sub


def adamw_inputs(n, step, seed):
    """fp32 (p, g, m, v) of n elements for the regime of `step`: per-element gradient scales 10^-6 .. 100, moments of the size a
    run at that scale has after step - 1 steps (zero before the first), a tenth of the gradients zero, a tenth of the moments zero"""
    g_ = torch.Generator().manual_seed(seed * 1000003 + step)
    scale = torch.pow(torch.tensor(10.0), torch.rand(n, generator=g_) * 8.0 - 6.0)
    p = torch.randn(n, generator=g_) * torch.where(torch.rand(n, generator=g_) < 0.5, 0.05, 1.0)
    g = torch.randn(n, generator=g_) * scale
    g = torch.where(torch.rand(n, generator=g_) < 0.1, torch.zeros(n), g)
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        fill = min(1.0, (step - 1) / 10.0)
        m = torch.randn(n, generator=g_) * scale * 0.5 * fill
        v = (torch.randn(n, generator=g_) * scale) ** 2 * min(1.0, (step - 1) / 1000.0) + (m * m) * 1e-3
        z = torch.rand(n, generator=g_) < 0.1
        m, v = torch.where(z, torch.zeros(n), m), torch.where(z, torch.zeros(n), v)
    return p, g, m, v


# two synthetic flat buffers of vpd_op_adamw_pack: ((Co, Ci, k) ...) with the plain ranges in front of, between and behind them:
# one shorter than a 2048-float chunk, one that is no multiple of 256, one longer than a chunk; k = 2 takes the general gather
ADAM_PACK_BUFFERS = {
    "a": dict(convs=((32, 32, 3), (64, 32, 1), (32, 64, 2)), gaps=(100, 2048 + 700, 4, 36)),
    "b": dict(convs=((64, 64, 1), (32, 96, 3)), gaps=(0, 5000, 2048)),
}


def adam_pack_layout(name):
    """-> (dims [(Co, Ci, k)], offsets, numel): gap i lies in front of conv i, the last one behind; every gap is a multiple of 4"""
    b = ADAM_PACK_BUFFERS[name]
    offs, at = [], 0
    for (Co, Ci, k), gap in zip(b["convs"], b["gaps"]):
        at += gap
        offs.append(at)
        at += Co * Ci * k * k
    at += b["gaps"][-1]
    assert at % 4 == 0 and all(o % 4 == 0 for o in offs)
    return list(b["convs"]), offs, at


# ---- slab sums ----
SLAB_KSPLITS = (1, 2, 3, 15, 16, 17, 33)
SLAB_LENGTHS = (9 * 64 * 64, 64 * 64, 4 * 100)
SLAB_GROUP = ((9 * 64 * 64, 1), (64 * 64, 5), (4 * 100, 33))      # one launch: the thread groups of the widest serve all


def slab_partials(n, ksplit, integer, g):
    """[ksplit][n] fp32 partials: integers with |sum| <= 33 * 1000 < 2^24 (every fp32 sum exact in any order), or randn"""
    if integer:
        return torch.randint(-1000, 1001, (ksplit, n), generator=g).float()
    return torch.randn(ksplit, n, generator=g)


def slab_sum_ref(slab):
    """float64 sum over the splits, and the bound of an fp32 sum of ksplit terms in any order: ksplit u sum |partials|"""
    return slab.double().sum(0), slab.shape[0] * U32 * slab.double().abs().sum(0)


ZERO_RANGE_CASES = {1: (1,), 3: (1, 512 * 256 + 77, 300), 16: tuple([1, 7, 256, 257, 1000, 3, 64, 5000] * 2)}      # float4 per range


# ---------------------------------------------------------------------------
# 64-wide weight-gradient kernels, route by route (tests/test_wgrad_routes_gpu.py, tests/wgrad_routes_child.py,
# tests/test_wgrad_routes_cpu.py).  Every number below is asserted through vpd_op_wgrad_dispatch / vpd_op_wgrad_group_dispatch.
# ---------------------------------------------------------------------------
WG_KERNELS = ("atomics", "stem", "halo3x3", "halo1x1")        # out9[0] of vpd_op_wgrad_dispatch
WG_OUT9 = ("kernel", "inst", "stages", "TR", "multi", "NHP", "ksplit", "cpb", "grid_x")
# grouped launch (conv_wgrad_halo_grouped_kernel): problems (n, H, W, Co, Ci) of 3x3 stride-1 pad-1 convolutions; head = (pass
# instantiation, tasks, grid, halo passes); per problem (ksplit, cpb, tiles)
WG_GROUPS = {
    # six splits of 8 chunks; one split of two chunks, the second ragged (80 pixels), stored straight into dw; 4 splits x 2 tiles.
    # 15 tasks on a grid of 16: one padded block returns early; a multi problem (4 x 4 planes) beside row problems
    "np5_mixed":       ([(3, 32, 32, 64, 64), (5, 4, 4, 64, 64), (2, 32, 32, 128, 64)], (5, 15, 16, 5), [(6, 8, 1), (1, 2, 1), (4, 8, 2)]),
    # the four-pass instantiation: 16-wide rows and 8 x 8 planes
    "np4_mixed":       ([(3, 16, 16, 64, 64), (5, 8, 8, 128, 64), (7, 16, 16, 64, 128)], (4, 12, 16, 4), [(2, 6, 1), (1, 5, 2), (4, 7, 2)]),
    # short last splits: 200 chunks in 25 splits of 8; 37 chunks in 5 splits of 8, the last holds 5
    "np4_short_last":  ([(50, 16, 16, 64, 64), (37, 8, 8, 64, 64)], (4, 30, 32, 4), [(25, 8, 1), (5, 8, 1)]),
    # two tasks on a grid of 8: six idle blocks
    "np5_one":         ([(1, 32, 32, 64, 64)], (5, 2, 8, 5), [(2, 8, 1)]),
    # four equal layer1 problems at 7 crops: 14 splits each, 56 tasks, exactly 7 per XCD
    "np5_layer1_x4":   ([(7, 32, 32, 64, 64)] * 4, (5, 56, 56, 5), [(14, 8, 1)] * 4),
}
# stem (conv_wgrad_stem_kernel): (crops, H, W of the input) -> (TR, ksplit, cpb); 130 crops: 520 chunks in 174 splits of three, the
# last holds one
WG_STEM = {
    "w128_n2":   ((2, 128, 128), (1, 128, 1)),
    "w64_n3":    ((3, 64, 64), (2, 48, 1)),
    "w32_n3":    ((3, 32, 32), (4, 12, 1)),
    "w32_n130":  ((130, 32, 32), (4, 174, 3)),
}
WG_STEM_REFUSED = {"w34_n3": (3, 34, 34), "w48_n3": (3, 48, 48)}      # odd output size; 24-wide rows: neither divides a 64-pixel chunk


# single launches (vpd_op_wgrad with a slab; without one every case takes the atomics kernel): kernel and pass instantiation.
# tests/test_ops_gpu.py::CONV_CASES -- its 1x1 cases take the atomics kernel in both passes of that test's loop: the operator entry
# states no wish for the halo route and VPD_WGRAD_1X1 is unset
WG_ROUTES_OPS = {
    "l1_3x3_s1": ("halo3x3", 4), "l2_3x3_s2": ("halo3x3", 10), "l2_1x1_s2": ("atomics", 0), "l3_3x3_s1_ragged": ("halo3x3", 5),
    "l4_3x3_s1_tiny": ("atomics", 0),                     # 2 x 2 planes: 32 images per chunk, a halo of 256 pixels is refused
    "l2_3x3_s1_big": ("halo3x3", 4), "l2_3x3_s2_32to16": ("halo3x3", 10), "l4_3x3_s2_8to4_ragged": ("halo3x3", 13),
    "b1_1x1_s1_256to64": ("atomics", 0), "b3_1x1_s1_128to512_ragged": ("atomics", 0), "ds_1x1_s2_32to16": ("atomics", 0),
    "b_1x1_s1_512to128_t256": ("atomics", 0), "b_1x1_s1_1024to256_t128": ("atomics", 0),
}
# the cases of CONV_CASES above that carry a weight gradient (tests/conv_ops_child.py)
WG_ROUTES_CONV = {"c0_w32": ("halo3x3", 5), "c0_w32_walk": ("halo3x3", 5), "c6_w16": ("halo3x3", 4), "c3_w4": ("halo3x3", 5),
                  "s2_w32": ("halo3x3", 10), "stem_w32": ("stem", 4)}
# tests/wgrad_pair_child.py::CASES: conv1 on the halo 3x3 route, the branch (VPD_WGRAD_1X1=1) on the halo 1x1 route, same instantiation
WG_ROUTES_PAIR = {"l2_n5": 10, "l2_n70": 10, "l3_n6": 10, "l3_n37": 10, "l4_n5": 13, "l4_n6": 13, "l4_n67": 13}


def wg_dispatch(L, geom13, taps9, has_slab, prefer_halo_1x1=0):
    """vpd_op_wgrad_dispatch for the 13 geometry arguments of a vpd_op_wgrad call -> dict of WG_OUT9, the kernel by name"""
    import ctypes as C
    out = (C.c_int * 9)()
    if L.vpd_op_wgrad_dispatch(*geom13, taps9, int(bool(has_slab)), prefer_halo_1x1, out) != 0:
        return {"error": L.vpd_last_error().decode()}
    d = dict(zip(WG_OUT9, list(out)))
    d["kernel"] = WG_KERNELS[d["kernel"]]
    return d


def wg_route_errors(d, what, **want):
    """[] when the dispatch answer d holds every expected field, else one line per field that differs"""
    return ["dispatch of %s: %s = %r, expected %r (%r)" % (what, k, d.get(k), v, d) for k, v in want.items() if d.get(k) != v]


def wg_operands(n, ci, co, h, w, stride, regime, name, g):
    """x [n][ci][h][w] and dz [n][co][h/stride][w/stride], float64 values the element type holds exactly.  int: {-1, 0, 1} at
    density 1/2 (every partial sum of at most 2^24 products is an integer that fp32 holds); randn: element-rounded"""
    sx, sz = (n, ci, h, w), (n, co, h // stride, w // stride)
    if regime == "int":
        return _sparse_int(sx, 0.5, g), _sparse_int(sz, 0.5, g)
    return elem_round(torch.randn(sx, generator=g), name).double(), elem_round(torch.randn(sz, generator=g), name).double()


def wg_bound(x, dz, cs):
    """the per-element randn bound of a weight gradient as tests/conv_ops_child.py applies it: fp32 output, M + 64 additions"""
    _, _, _, ho, wo = conv_geom(cs)
    return conv_gamma(conv_wgrad(x.abs(), dz.abs(), cs), x.shape[0] * ho * wo + 64)


def stem_wgrad_view(dw, ci):
    """the stem kernel's dw [7][64][8 column taps x 8 channels] -> [co][ci][7][7] (the eighth tap and channels ci.. are scratch)"""
    return dw.view(7, 64, 8, 8)[:, :, :7, :ci].permute(1, 3, 0, 2)


def wg_chunk_mask(dz, chunk):
    """dz with everything but the pixels of one 64-pixel chunk (NHW pixel order) zeroed"""
    n, c, h, w = dz.shape
    keep = torch.zeros(n * h * w, dtype=torch.bool)
    keep[chunk * 64:(chunk + 1) * 64] = True
    return dz * keep.view(n, 1, h, w)


def wg_alter_last_chunk(ref, x, dz, cs, ksplit, cpb, split=0):
    """(i) the last chunk of one split left out (an off-by-one in wg_chunk_range's end)"""
    nch = (dz.shape[0] * dz.shape[2] * dz.shape[3] + 63) // 64
    last = min((split + 1) * cpb, nch) - 1
    return ref - conv_wgrad(x, wg_chunk_mask(dz, last), cs)


def wg_alter_tap(ref, x, dz, cs, chunk=0, tap=(0, 2)):
    """(ii) one tap left out for the pixels of one chunk"""
    out = ref.clone()
    out[:, :, tap[0], tap[1]] -= conv_wgrad(x, wg_chunk_mask(dz, chunk), cs)[:, :, tap[0], tap[1]]
    return out


def wg_alter_transposed(ref):
    """(iv) the [Co][Ci] result of a 1x1 convolution stored as [Ci][Co]: the same memory read back in the convolution's own layout"""
    co, ci = ref.shape[:2]
    return ref[:, :, 0, 0].t().contiguous().view(co, ci)[:, :, None, None]


def wg_fp32_accumulated(x, dz, cs, chunk=64):
    """the weight gradient summed the way the kernels do: exact products, fp32 running sum over 64-pixel chunks in order"""
    n, c, h, w = dz.shape
    acc = torch.zeros(cs["co"], cs["ci"], cs["k"], cs["k"], dtype=torch.float32)
    for ch in range((n * h * w + chunk - 1) // chunk):
        acc = (acc + conv_wgrad(x, wg_chunk_mask(dz, ch), cs).float()).float()
    return acc.double()
