"""The BatchNorm backward launches that do their own reduction, one launch at a time through vpd_op_bn_backward /
vpd_op_bn_backward_pair: the three-launch path (bn_bwd_reduce_kernel<0|1|2>, bn_bwd_finalize_kernel, bn_bwd_apply_kernel), the
single launch with a grid barrier (bn_bwd_fused_kernel<0|1|2|3>) in each of its LDS-residency branches, the folded average-pool
gradient, and the pair kernel of a down-sampling block (bn_bwd_fused2_kernel).

Reference and tolerances are those of test_batchnorm_backward_op_matches_autograd (tests/test_ops_gpu.py): float64 autograd of
relu(batch_norm(z)) on the same element-rounded operands, an incoming gradient correlated with xhat, dz rel-L2 < 3e-3 (bf16; fp16
scaled by the ratio of the half-ulps) with the 2 %-off resolution check; dgamma / dbeta, summed here by the kernels in fp32
partials, within 2e-5 sum|terms| per channel (test_conv_epilogue_batchnorm_sums).  The largest cases use the closed form, which
tests/test_opref_cpu.py holds equal to autograd to 1e-12."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import opref as R
from tests.test_ops_gpu import BN_SHAPES, ptr, stream

pytestmark = pytest.mark.gpu

SYNC_BYTES = 18 * 128
SHAPES = BN_SHAPES + [(3, 7, 5, 64), (3, 5, 7, 256)]      # ragged: n H W is no multiple of the pixels per block iteration (32 .. 128 / 8 .. 32)
SHAPE_IDS = ["l3", "l2", "l1", "l4", "ragged64", "ragged256"]
MODES = ["none", "act", "z", "bits"]


def _lib(name):
    from vpd_amd._lib import lib
    return lib(name)


def _check(rc, name):
    from vpd_amd._lib import check
    check(rc, "op", name)


def _padded(t_nchw, name, border):
    """NCHW float -> device NHWC element tensor padded by 1, the border filled with `border`"""
    n, c, h, w = t_nchw.shape
    buf = torch.full((n, h + 2, w + 2, c), float(border))
    buf[:, 1:-1, 1:-1] = R.nhwc(t_nchw.float())
    return buf.to(R.ELEM[name][0]).cuda()


def _interior(buf, pad):
    t = buf[:, pad:-pad, pad:-pad] if pad else buf
    return R.nchw(t.cpu().double())


def _border_is(buf, pad, value):
    if not pad:
        return True
    o = buf.float()
    return bool((o[:, 0] == value).all() and (o[:, -1] == value).all() and (o[:, :, 0] == value).all() and (o[:, :, -1] == value).all())


def run_bn_backward(name, cs, mode, fused, dzpad=1, dy_pooled=None, dy_dev=None):
    """One vpd_op_bn_backward launch on the case's operands.  The ReLU mask reaches the kernel as `mode` says: the stored activation
    (border 9: only the interior may be read; write_g), mscale / mshift, a bit map, or none."""
    L = _lib(name)
    dt = R.ELEM[name][0]
    n, c, h, w = cs["z"].shape
    M = n * h * w
    mask = cs["mask"]
    dev = lambda t: R.nhwc(t).to(dt).cuda()
    f32 = lambda t: t.float().cuda()
    zd = dev(cs["z"])
    dyd = dy_dev if dy_dev is not None else dev(cs["dy"])
    act = bits = msc = msh = None
    if mode == "act":
        act = _padded(cs["act"], name, 9.0)
    elif mode == "bits":
        bits = R.mask_bits(R.nhwc(mask).reshape(M, c)).cuda()
    elif mode == "z":
        sc = cs["gamma"].double() * cs["rstd"]
        msc, msh = f32(sc), f32(cs["beta"].double() - cs["mean"] * sc)
    rows = torch.zeros(4 if fused else 16, 2, c, dtype=torch.float64, device="cuda")
    coef = torch.zeros(3, c, device="cuda")
    sync = torch.zeros(SYNC_BYTES, dtype=torch.uint8, device="cuda")          # barrier words zeroed before every launch
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    dz = torch.full((n, h + 2 * dzpad, w + 2 * dzpad, c), 3.0, dtype=dt, device="cuda")
    dgamma, dbeta = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    gam, mu, rs = f32(cs["gamma"]), f32(cs["mean"]), f32(cs["rstd"])
    dyp = dy_pooled.cuda() if dy_pooled is not None else None
    _check(L.vpd_op_bn_backward(ptr(dyd), ptr(zd), ptr(act) if act is not None else None, ptr(bits) if bits is not None else None,
                                ptr(msc) if msc is not None else None, ptr(msh) if msh is not None else None,
                                ptr(dyp) if dyp is not None else None, ptr(rows), ptr(coef), ptr(sync), ptr(err), ptr(gam), ptr(mu),
                                ptr(rs), ptr(dz), dzpad, ptr(dgamma), ptr(dbeta), n, h, w, c, 1 if mode == "act" else 0,
                                1 if fused else 0, stream()), name)
    torch.cuda.synchronize()
    assert int(err.cpu()[0]) == 0, "the grid barrier timed out"
    assert _border_is(dz, dzpad, 3.0), "dz border written"
    return {"dz": _interior(dz, dzpad), "dz_raw": dz, "dgamma": dgamma.cpu().double(), "dbeta": dbeta.cpu().double(), "dy_after": dyd}


def check_against_reference(name, cs, out, flip=None):
    """the gates of the module docstring; flip: elements whose mask the kernel's fp32 evaluation may legitimately flip"""
    mask, dy = cs["mask"], cs["dy"]
    v = lambda t: t.double().view(1, -1, 1, 1)
    xhat = (cs["z"].double() - v(cs["mean"])) * v(cs["rstd"])
    gm = dy.double() * mask
    abs1, abs2 = gm.abs().sum(dim=(0, 2, 3)), (gm * xhat).abs().sum(dim=(0, 2, 3))
    b1, b2 = R.SUM_TOL * abs1, R.SUM_TOL * abs2
    if flip is not None:
        assert float(flip.double().mean()) <= R.BAND_CAP
        b1 = b1 + (dy.double().abs() * flip).sum(dim=(0, 2, 3))
        b2 = b2 + ((dy.double() * xhat).abs() * flip).sum(dim=(0, 2, 3))
    e1, e2 = (out["dbeta"] - cs["dbeta"]).abs(), (out["dgamma"] - cs["dgamma"]).abs()
    assert bool((e1 <= b1).all()), float((e1 / b1).max())
    assert bool((e2 <= b2).all()), float((e2 / b2).max())
    gate = R.dz_l2_gate(name)
    l2 = R.rel_l2(out["dz"], cs["dz"])
    assert l2 < gate, l2
    off = R.bn_dz_closed_form(cs["z"], cs["gamma"], cs["mean"], cs["rstd"], gm, 1.02)
    assert R.rel_l2(out["dz"], off) > 2 * gate          # resolution: a 2 % error in one coefficient fails the same gate
    return l2


# the three-launch path has no bit-map form (the entry point refuses it: test_entry_point_refuses_what_no_launcher_takes)
PATHS = [(m, f) for m in MODES for f in (0, 1) if not (m == "bits" and f == 0)]


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("mode,fused", PATHS, ids=["%s-%s" % (m, "fused" if f else "three_launch") for m, f in PATHS])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_bn_backward_paths_match_autograd(shape, mode, fused, name):
    n, h, w, c = shape
    cs = R.bn_backward_case(n, h, w, c, 7 * n + c + len(mode), name, relu=mode != "none", residual=mode == "act")
    mask, flip = cs["mask"], None
    if mode == "act":
        # the kernel's mask is the sign of the STORED activation: a positive value that rounds to zero (fp16, below 2^-25) differs
        mask = R.elem_round(cs["act"].float(), name) > 0
        cs = R.bn_case_with_mask(cs, mask)
    if mode == "z":
        sc = (cs["gamma"].double() * cs["rstd"]).float()
        v = lambda t: t.double().view(1, -1, 1, 1)
        y = (cs["z"].double() - v(cs["mean"])) * v(cs["rstd"]) * v(cs["gamma"]) + v(cs["beta"])
        flip = R.relu_band(cs["z"], sc, (cs["beta"].double() - cs["mean"] * sc.double()).float(), y)
    out = run_bn_backward(name, cs, mode, fused, dzpad=0 if mode == "none" else 1)
    l2 = check_against_reference(name, cs, out, flip=flip)
    print(shape, mode, "fused" if fused else "three-launch", name, "dz rel-L2 %.3e" % l2)
    dy_before = R.nhwc(cs["dy"]).to(R.ELEM[name][0])
    if mode == "act":
        # write_g: the masked gradient is written back over dy, exactly
        want = torch.where(R.nhwc(mask), dy_before, torch.zeros_like(dy_before))
        assert torch.equal(out["dy_after"].cpu(), want)
    else:
        assert torch.equal(out["dy_after"].cpu(), dy_before)


def test_entry_point_refuses_what_no_launcher_takes():
    L = _lib("bf16")
    t = torch.zeros(4096, device="cuda")
    p = ptr(t)
    args = lambda **k: [k.get("dy", p), p, k.get("act"), k.get("bits"), None, None, k.get("dyp"), p, p, p, p, p, p, p, p, 0, p, p,
                        1, 4, 4, 64, k.get("write_g", 0), k.get("fused", 1), stream()]
    assert L.vpd_op_bn_backward(*args(bits=p, fused=0)) != 0 and b"three-launch" in L.vpd_last_error()
    assert L.vpd_op_bn_backward(*args(act=p, bits=p)) != 0 and b"one ReLU mask" in L.vpd_last_error()
    assert L.vpd_op_bn_backward(*args(act=p, write_g=0)) != 0 and b"no fused" in L.vpd_last_error()
    assert L.vpd_op_bn_backward(*args(dyp=p)) != 0 and b"bit map" in L.vpd_last_error()
    assert L.vpd_op_bn_backward(*args(dy=None)) != 0


def _residency(name, M, c, pair=0):
    out = (C.c_int * 4)()
    _check(_lib(name).vpd_op_bn_backward_residency(M, c, pair, out), name)
    return tuple(out)


# (channels, H = W, mask mode): equal bytes per crop; the mode varies with the width so that every mask form meets a
# non-resident g somewhere (bits and z recompute it from dy, act re-reads what write_g parked in dy)
RESIDENCY = [(64, 32, "bits"), (256, 16, "act")]
CROPS = (8, 64, 128, 192, 256, 320, 384, 512, 640, 768)


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("c,hw,mode", RESIDENCY, ids=["c64", "c256"])
def test_fused_backward_in_every_lds_residency_branch(c, hw, mode, name):
    """vpd_launch_bn_bwd_fused keeps g and z in LDS across the barrier when they fit (8 crops), g only (~256 crops), or neither
    (>= 512 crops).  The sizes come from the launcher's own arithmetic (vpd_op_bn_backward_residency); the test fails if one of
    the three branches is not reached on this device."""
    picked = {}
    for n in CROPS:
        _, keep_g, keep_z, _ = _residency(name, n * hw * hw, c)
        picked.setdefault((keep_g, keep_z), n)
    assert set(picked) == {(1, 1), (1, 0), (0, 0)}, picked
    for branch, n in sorted(picked.items(), reverse=True):
        cs = R.bn_backward_case(n, hw, hw, c, n + c, name, relu=True, residual=mode == "act", autograd=False)
        out = run_bn_backward(name, cs, mode, 1)
        # (the stored activation's sign is the kernel's mask: a positive value below fp16's 2^-25 is stored as zero)
        stored = R.elem_round(cs["act"].float(), name) > 0 if mode == "act" else cs["mask"]
        cs = R.bn_case_with_mask(cs, stored)
        l2 = check_against_reference(name, cs, out)
        print("C %d, %d crops, keep_g %d keep_z %d, %s: dz rel-L2 %.3e" % (c, n, branch[0], branch[1], name, l2))
        if mode == "act":
            dy_before = R.nhwc(cs["dy"]).to(R.ELEM[name][0])
            assert torch.equal(out["dy_after"].cpu(), torch.where(R.nhwc(stored), dy_before, torch.zeros_like(dy_before)))
        del cs, out


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_fused_backward_mask_from_z_without_resident_g(name):
    """mscale / mshift (mask recomputed from z) in the branch where phase 2 recomputes g from dy and z: the smallest size of
    that branch, C = 128"""
    c, hw = 128, 16
    n = next(n for n in CROPS if _residency(name, n * hw * hw, c)[1] == 0)
    cs = R.bn_backward_case(n, hw, hw, c, n + c, name, relu=True, autograd=False)
    sc = (cs["gamma"].double() * cs["rstd"]).float()
    v = lambda t: t.double().view(1, -1, 1, 1)
    y = (cs["z"].double() - v(cs["mean"])) * v(cs["rstd"]) * v(cs["gamma"]) + v(cs["beta"])
    flip = R.relu_band(cs["z"], sc, (cs["beta"].double() - cs["mean"] * sc.double()).float(), y)
    out = run_bn_backward(name, cs, "z", 1)
    check_against_reference(name, cs, out, flip=flip)


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(5, 4, 4, 512), (3, 4, 4, 2048), (6, 2, 2, 512)], ids=["c512", "c2048", "c512_2x2"])
def test_folded_average_pool_gradient(shape, name):
    """dy_pooled: the last BatchNorm backward produces dy = elem(dpooled / (H W)) itself.  Against autograd of
    relu(bn(z)).mean((2, 3)) contracted with dpooled -- dpooled is drawn so that dpooled / (H W) is an element-type value, the
    operands of the reference are then the kernel's -- and the dy it leaves behind equal to avgpool_bwd's output bit for bit."""
    n, h, w, c = shape
    L = _lib(name)
    dt = R.ELEM[name][0]
    g = torch.Generator().manual_seed(n + c + h)
    z = R.elem_round(torch.randn(n, c, h, w, generator=g) * 1.3 - 0.2, name)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    dy1 = R.elem_round(torch.randn(n, c, generator=g) + 0.3, name)                 # the per-pixel gradient, an element-type value
    dpooled = dy1 * (h * w)                                                        # exact: H W is a power of two
    zt, gt, bt = z.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.batch_norm(zt, None, None, gt, bt, training=True, eps=R.BN_EPS)
    (y.clamp_min(0).mean(dim=(2, 3)) * dpooled.double()).sum().backward()
    mean, rstd = R.stem_stats(z)
    dy = dy1.view(n, c, 1, 1).expand(n, c, h, w).contiguous()
    cs = {"z": z, "dy": dy, "gamma": gamma, "beta": beta, "mean": mean, "rstd": rstd, "mask": y.detach() > 0,
          "dz": zt.grad, "dgamma": gt.grad, "dbeta": bt.grad}
    dy_dev = torch.full((n, h, w, c), 5.0, dtype=dt, device="cuda")               # does not exist yet: the launch writes it
    out = run_bn_backward(name, cs, "bits", 1, dy_pooled=dpooled, dy_dev=dy_dev)
    check_against_reference(name, cs, out)
    # the unfolded pair of launches: avgpool_bwd, then the same BatchNorm backward reading its output
    dact = torch.full((n, h, w, c), 6.0, dtype=dt, device="cuda")
    dpd = dpooled.cuda()
    _check(L.vpd_op_avgpool_bwd(ptr(dpd), n, h, w, c, ptr(dact), stream()), name)
    torch.cuda.synchronize()
    assert torch.equal(out["dy_after"], dact)
    assert torch.equal(dact.cpu(), R.nhwc(dy).to(dt))
    out2 = run_bn_backward(name, cs, "bits", 1, dy_dev=dact)
    assert torch.equal(out2["dz_raw"], out["dz_raw"])
    assert torch.equal(out2["dgamma"], out["dgamma"]) and torch.equal(out2["dbeta"], out["dbeta"])


def _pair_case(n, h, w, c, seed, name, autograd):
    g = torch.Generator().manual_seed(seed)
    zA = R.elem_round(torch.randn(n, c, h, w, generator=g) * 1.3 - 0.2, name)
    zB = R.elem_round(torch.randn(n, c, h, w, generator=g) * 0.8 + 0.4, name)
    std = lambda t: (t - t.mean(dim=(0, 2, 3), keepdim=True)) / t.std(dim=(0, 2, 3), keepdim=True)
    dy = R.elem_round(torch.randn(n, c, h, w, generator=g) + 0.6 * std(zA) + 0.6 * std(zB) + 0.3, name)
    gA, bA = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    gB, bB = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    (mA, rA), (mB, rB) = R.stem_stats(zA), R.stem_stats(zB)
    A = {"z": zA, "dy": dy, "gamma": gA, "beta": bA, "mean": mA, "rstd": rA}
    B = {"z": zB, "dy": dy, "gamma": gB, "beta": bB, "mean": mB, "rstd": rB}
    v = lambda t: t.double().view(1, -1, 1, 1)
    if autograd:
        # two independent references: each BatchNorm's own graph, the other branch entering as a constant
        yA0 = (zA.double() - v(mA)) * v(rA) * v(gA) + v(bA)
        yB0 = (zB.double() - v(mB)) * v(rB) * v(gB) + v(bB)
        for side, other in ((A, yB0), (B, yA0)):
            zt, gt, bt = side["z"].double().requires_grad_(True), side["gamma"].double().requires_grad_(True), side["beta"].double().requires_grad_(True)
            y = F.batch_norm(zt, None, None, gt, bt, training=True, eps=R.BN_EPS) + other
            (y.clamp_min(0) * dy.double()).sum().backward()
            side.update(dz=zt.grad, dgamma=gt.grad, dbeta=bt.grad, mask=y.detach() > 0, act=y.detach().clamp_min(0))
    else:
        y = (zA.double() - v(mA)) * v(rA) * v(gA) + v(bA) + (zB.double() - v(mB)) * v(rB) * v(gB) + v(bB)
        mask = y > 0
        gm = dy.double() * mask
        for side in (A, B):
            xhat = (side["z"].double() - v(side["mean"])) * v(side["rstd"])
            side.update(dz=R.bn_dz_closed_form(side["z"], side["gamma"], side["mean"], side["rstd"], gm),
                        dgamma=(gm * xhat).sum(dim=(0, 2, 3)), dbeta=gm.sum(dim=(0, 2, 3)), mask=mask, act=y.clamp_min(0))
    return A, B


def _stored_mask(A, B, name):
    """both references under the mask the kernel sees: the sign of the stored block output"""
    stored = R.elem_round(A["act"].float(), name) > 0
    return R.bn_case_with_mask(A, stored), R.bn_case_with_mask(B, stored)


def _run_pair(name, A, B):
    L = _lib(name)
    dt = R.ELEM[name][0]
    n, c, h, w = A["z"].shape
    dev = lambda t: R.nhwc(t).to(dt).cuda()
    f32 = lambda t: t.float().cuda()
    dyd, act = dev(A["dy"]), _padded(A["act"], name, 9.0)
    sync = torch.zeros(SYNC_BYTES, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    keep, outs, args = [], [], []
    for side in (A, B):
        zd, mu, rs, gam = dev(side["z"]), f32(side["mean"]), f32(side["rstd"]), f32(side["gamma"])
        rows = torch.zeros(4, 2, c, dtype=torch.float64, device="cuda")
        dz = torch.full((n, h + 2, w + 2, c), 3.0, dtype=dt, device="cuda")
        dgamma, dbeta = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
        keep += [zd, mu, rs, gam, rows]
        outs.append((dz, dgamma, dbeta))
        args += [ptr(zd), ptr(mu), ptr(rs), ptr(gam), ptr(rows), ptr(dz), ptr(dgamma), ptr(dbeta)]
    _check(L.vpd_op_bn_backward_pair(ptr(dyd), ptr(act), *args, ptr(sync), ptr(err), n, h, w, c, stream()), name)
    torch.cuda.synchronize()
    assert int(err.cpu()[0]) == 0, "the grid barrier timed out"
    res = []
    for dz, dgamma, dbeta in outs:
        assert _border_is(dz, 1, 3.0)
        res.append({"dz": _interior(dz, 1), "dgamma": dgamma.cpu().double(), "dbeta": dbeta.cpu().double()})
    return res


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(4, 8, 8, 128), (3, 4, 4, 512), (5, 16, 16, 128), (3, 7, 5, 64)], ids=["l2", "l4", "l2_16", "ragged"])
def test_pair_kernel_matches_two_autograd_references(shape, name):
    n, h, w, c = shape
    A, B = _stored_mask(*_pair_case(n, h, w, c, n * 13 + c, name, True), name)
    oA, oB = _run_pair(name, A, B)
    print(shape, name, "dzA %.3e dzB %.3e" % (check_against_reference(name, A, oA), check_against_reference(name, B, oB)))


def test_pair_kernel_in_every_lds_residency_branch():
    """bn_bwd_fused2_kernel keeps g, zA and zB in LDS while they fit: all three, g + zA, g only, none (g parked in dy).  Sizes from
    the launcher's own arithmetic; layer2's 16 x 16 x 128 block output."""
    name, c, hw = "bf16", 128, 16
    picked = {}
    for n in CROPS:
        picked.setdefault(_residency(name, n * hw * hw, c, 1)[1:], n)
    assert set(picked) == {(1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 0, 0)}, picked
    for branch, n in sorted(picked.items(), reverse=True):
        A, B = _stored_mask(*_pair_case(n, hw, hw, c, n + 5, name, False), name)
        oA, oB = _run_pair(name, A, B)
        print("pair, %d crops, resident %s: dzA %.3e dzB %.3e" % (n, branch, check_against_reference(name, A, oA),
                                                                  check_against_reference(name, B, oB)))
        del A, B, oA, oB
