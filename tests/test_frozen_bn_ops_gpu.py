"""Frozen BatchNorm one launch at a time: every launch that finalizes a train-plan BatchNorm, through the vpd_op_* entry points
with the hook vpd_op_set_bn_frozen on, in both libraries, against the float64 closed forms of tests/opref_frozen.py on the same
element-rounded operands (tests/test_frozen_bn_cpu.py holds those equal to autograd of F.batch_norm(training=False)).

Statistics: running_mean ~ 0.5 N(0, 1), running_var in [0.25, 2], |gamma| in [0.05, 1.5] of either sign -- far from the operands' own
batch statistics (z ~ 1.3 N(0, 1) - 0.2) and from 0 / 1: a launch that normalises with the batch, or keeps the two batch-mean terms
of the train-mode backward, reads tens of bounds off (test_bounds_resolve_a_kernel_on_the_wrong_statistics).
Bounds (tests/opref.py): stored outputs and dz per element within one ulp of the element type at the reference
plus the fp32 arithmetic of the closed form (opref_frozen.out_bound / dz_bound); dgamma / dbeta within 2e-5 sum |terms|
(opref.SUM_TOL); a recomputed ReLU mask may flip inside opref.relu_band.  Running statistics handed to a frozen launch must come
back bit for bit; with the hook off again the launches reproduce their unfrozen results bit for bit."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import opref as R
from tests import opref_frozen as Z
from tests.test_bn_backward_ops_gpu import CROPS, SYNC_BYTES, _border_is, _interior, _padded, _residency, _run_pair, run_bn_backward
from tests.test_ops_gpu import ptr, stream

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bf16", "fp16"]
F = C.c_float


def _lib(name):
    from vpd_amd._lib import lib
    return lib(name)


def _check(rc, name):
    from vpd_amd._lib import check
    check(rc, "op", name)


@contextlib.contextmanager
def frozen(name):
    L = _lib(name)
    _check(L.vpd_op_set_bn_frozen(1), name)
    try:
        yield L
    finally:
        _check(L.vpd_op_set_bn_frozen(0), name)


def _batch_rows(z, nrows):
    """the rows as the producing convolution leaves them: the BATCH sums of z, spread over the rows -- a frozen launch must not use them"""
    zd = z.double()
    rows = torch.zeros(nrows, 2, z.shape[1], dtype=torch.float64)
    rows[1, 0], rows[nrows - 1, 1] = zd.sum(dim=(0, 2, 3)), (zd * zd).sum(dim=(0, 2, 3))
    return rows.cuda()


def _stats_ok(got, cs, sfx=""):
    b = Z.stats_bounds(cs["gamma" + sfx], cs["beta" + sfx], cs["rm" + sfx], cs["rv" + sfx])
    rs = Z.rstd_of(cs["rv" + sfx])
    sc = cs["gamma" + sfx].double() * rs
    want = {"mean": cs["rm" + sfx].double(), "rstd": rs, "scale": sc, "shift": cs["beta" + sfx].double() - cs["rm" + sfx].double() * sc}
    for k, v in want.items():
        err = (got[k].cpu().double() - v).abs()
        assert bool((err <= b[k]).all()), (k + sfx, float(err.max()))


def _bn_vectors(c):
    return {k: torch.full((c,), 7.0, device="cuda") for k in ("mean", "rstd", "scale", "shift")}


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("shape", [(3, 9, 7, 64), (2, 16, 16, 64)], ids=["3x9x7", "2x16x16"])
def test_forward_on_running_statistics(shape, residual, name):
    """bn_fwd_fused_kernel through vpd_op_bn_forward: out, the four saved vectors, the ReLU bit map; rm / rv untouched"""
    n, h, w, c = shape
    cs = Z.case(n, h, w, c, 31 * n + h + residual, name, residual=residual)
    dt = R.ELEM[name][0]
    zd = R.nhwc(cs["z"]).to(dt).cuda()
    rows = _batch_rows(cs["z"], 4)
    gam, bet, rm, rv = (cs[k].float().cuda() for k in ("gamma", "beta", "rm", "rv"))
    rm0, rv0 = rm.clone(), rv.clone()
    v = _bn_vectors(c)
    out = torch.full((n, h + 2, w + 2, c), 3.0, dtype=dt, device="cuda")
    bits = torch.zeros(n * h * w * c // 8, dtype=torch.uint8, device="cuda")
    resp = _padded(cs["res"], name, 9.0) if residual else None
    with frozen(name) as L:
        _check(L.vpd_op_bn_forward(ptr(zd), ptr(rows), ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(v["mean"]), ptr(v["rstd"]), ptr(v["scale"]),
                                   ptr(v["shift"]), ptr(resp) if residual else None, ptr(out), ptr(bits), n, h, w, c, 1, F(0.1), F(R.BN_EPS),
                                   stream()), name)
        # running statistics are required
        assert L.vpd_op_bn_forward(ptr(zd), ptr(rows), ptr(gam), ptr(bet), None, None, ptr(v["mean"]), ptr(v["rstd"]), ptr(v["scale"]),
                                   ptr(v["shift"]), None, ptr(out), None, n, h, w, c, 1, F(0.1), F(R.BN_EPS), stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    assert _border_is(out, 1, 3.0)
    got = _interior(out, 1)
    bound = Z.out_bound(cs["out"], cs["z"], cs["gamma"], cs["beta"], cs["rm"], cs["rv"], name, res=cs["res"])
    ratio = float(((got - cs["out"]).abs() / bound).max())
    print(shape, residual, name, "out max err / bound %.3f" % ratio)
    assert ratio <= 1.0
    _stats_ok(v, cs)
    M = n * h * w
    assert torch.equal(bits.cpu().view(M, c // 8), R.mask_bits((R.nhwc(got) > 0).reshape(M, c)))


@pytest.mark.parametrize("name", NAMES)
def test_forward_with_the_second_batchnorm(name):
    """res_kind 2 (a down-sampling block): out = relu(BN(z) + BN2(z2)), both on their running statistics, through vpd_op_bn_forward2"""
    n, h, w, c = 3, 9, 7, 64
    A, B = Z.case(n, h, w, c, 41, name, relu=False), Z.case(n, h, w, c, 43, name, relu=False)
    dt = R.ELEM[name][0]
    dev = lambda t: R.nhwc(t).to(dt).cuda()
    args, keep, vecs, runs = [], [], [], []
    for cs in (A, B):
        zd, rows = dev(cs["z"]), _batch_rows(cs["z"], 4)
        gam, bet, rm, rv = (cs[k].float().cuda() for k in ("gamma", "beta", "rm", "rv"))
        v = _bn_vectors(c)
        keep += [zd, rows, gam, bet]
        vecs.append(v)
        runs.append((rm, rv, rm.clone(), rv.clone()))
        args.append([ptr(zd), ptr(rows), ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(v["mean"]), ptr(v["rstd"]), ptr(v["scale"]), ptr(v["shift"])])
    out = torch.full((n, h + 2, w + 2, c), 3.0, dtype=dt, device="cuda")
    bits = torch.zeros(n * h * w * c // 8, dtype=torch.uint8, device="cuda")
    with frozen(name) as L:
        _check(L.vpd_op_bn_forward2(*args[0], *args[1], ptr(out), ptr(bits), n, h, w, c, 1, F(0.1), F(R.BN_EPS), stream()), name)
    torch.cuda.synchronize()
    for rm, rv, rm0, rv0 in runs:
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    ref = (A["pre"] + B["pre"]).clamp_min(0)
    bound = Z.out_bound(ref, A["z"], A["gamma"], A["beta"], A["rm"], A["rv"], name, second=(B["z"], B["gamma"], B["beta"], B["rm"], B["rv"]))
    got = _interior(out, 1)
    ratio = float(((got - ref).abs() / bound).max())
    print(name, "out max err / bound %.3f" % ratio)
    assert ratio <= 1.0 and _border_is(out, 1, 3.0)
    _stats_ok(vecs[0], A)
    _stats_ok(vecs[1], B)
    M = n * h * w
    assert torch.equal(bits.cpu().view(M, c // 8), R.mask_bits((R.nhwc(got) > 0).reshape(M, c)))


@pytest.mark.parametrize("name", NAMES)
def test_finalize_launch_of_the_stem_and_the_unfused_path(name):
    """vpd_launch_bn_finalize, frozen: the four vectors from the running statistics (rstd by the launch's own fp64 1 / sqrt), the
    sixteen shared rows consumed -- left zeroed -- and rm / rv untouched"""
    c = 64
    cs = Z.case(3, 9, 7, c, 47, name)
    rows = _batch_rows(cs["z"], 16)
    gam, bet, rm, rv = (cs[k].float().cuda() for k in ("gamma", "beta", "rm", "rv"))
    rm0, rv0 = rm.clone(), rv.clone()
    v = _bn_vectors(c)
    with frozen(name) as L:
        _check(L.vpd_op_bn_finalize(ptr(rows), ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(v["mean"]), ptr(v["rstd"]), ptr(v["scale"]),
                                    ptr(v["shift"]), 3 * 9 * 7, c, F(0.1), F(R.BN_EPS), stream()), name)
        assert L.vpd_op_bn_finalize(ptr(rows), ptr(gam), ptr(bet), None, None, ptr(v["mean"]), ptr(v["rstd"]), ptr(v["scale"]),
                                    ptr(v["shift"]), 3 * 9 * 7, c, F(0.1), F(R.BN_EPS), stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and float(rows.abs().max()) == 0.0
    _stats_ok(v, cs)
    # hook off: the same launch is train mode again -- batch statistics, running statistics updated
    rows = _batch_rows(cs["z"], 16)
    _check(_lib(name).vpd_op_bn_finalize(ptr(rows), ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(v["mean"]), ptr(v["rstd"]), ptr(v["scale"]),
                                         ptr(v["shift"]), 3 * 9 * 7, c, F(0.1), F(R.BN_EPS), stream()), name)
    torch.cuda.synchronize()
    mean, rstd = R.stem_stats(cs["z"])
    assert torch.allclose(v["mean"].cpu().double(), mean, rtol=1e-5, atol=1e-6) and torch.allclose(v["rstd"].cpu().double(), rstd, rtol=1e-5)
    assert not torch.equal(rm, rm0) and not torch.equal(rv, rv0)


# ---- backward --------------------------------------------------------------------------------------------------------------------
def _check_backward(name, cs, out, flip=None, what=""):
    b1, b2 = Z.sum_bounds(cs, flip)
    e1, e2 = (out["dbeta"] - cs["dbeta"]).abs(), (out["dgamma"] - cs["dgamma"]).abs()
    assert bool((e1 <= b1).all()), (what, "dbeta", float((e1 / b1).max()))
    assert bool((e2 <= b2).all()), (what, "dgamma", float((e2 / b2).max()))
    err, bound = (out["dz"] - cs["dz"]).abs(), Z.dz_bound(cs["dz"], name)
    if flip is not None:      # an element whose mask may legitimately flip holds gamma rstd dy or 0
        assert float(flip.double().mean()) <= R.BAND_CAP
        err = torch.where(flip, torch.zeros_like(err), err)
    ratio = float((err / bound).max())
    print(what, name, "dz max err / bound %.3f" % ratio)
    assert ratio <= 1.0, (what, ratio)
    # resolution: the train-mode formula on the same statistics is far outside
    train = R.bn_dz_closed_form(cs["z"], cs["gamma"], cs["mean"], cs["rstd"], cs["gm"])
    assert float(((train - cs["dz"]).abs() > 10 * bound).double().mean()) > 0.1


def _mode_case(n, h, w, c, seed, name, mode):
    """a frozen case under the mask form `mode` (none | act | z | bits) as the kernel sees it; returns (case, flip band or None)"""
    cs = Z.case(n, h, w, c, seed, name, relu=mode != "none", residual=mode == "act")
    flip = None
    if mode == "act":      # the sign of the STORED activation
        cs = Z.with_mask(cs, R.elem_round(cs["act"].float(), name) > 0)
    if mode == "z":        # scale z + shift recomputed in fp32
        sc = (cs["gamma"].double() * cs["rstd"].double()).float()
        flip = R.relu_band(cs["z"], sc, (cs["beta"].double() - cs["mean"].double() * sc.double()).float(), cs["pre"])
    return cs, flip


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", ["none", "act", "z"])
def test_three_launch_backward(mode, name):
    """bn_bwd_reduce_kernel + bn_bwd_finalize_kernel (c2 = c3 = 0) + bn_bwd_apply_kernel"""
    cs, flip = _mode_case(3, 9, 7, 64, 53 + len(mode), name, mode)
    with frozen(name):
        out = run_bn_backward(name, cs, mode, 0, dzpad=0 if mode == "none" else 1)
    _check_backward(name, cs, out, flip, "three-launch " + mode)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", ["none", "act", "z", "bits"])
def test_grid_barrier_backward_in_every_mask_form(mode, name):
    """bn_bwd_fused_kernel<0|1|2|3>"""
    cs, flip = _mode_case(3, 9, 7, 64, 59 + len(mode), name, mode)
    with frozen(name):
        out = run_bn_backward(name, cs, mode, 1, dzpad=0 if mode == "none" else 1)
    _check_backward(name, cs, out, flip, "grid-barrier " + mode)


@pytest.mark.parametrize("name", NAMES)
def test_grid_barrier_backward_with_the_folded_pool_gradient(name):
    n, h, w, c = 5, 4, 4, 64
    cs = Z.case(n, h, w, c, 61, name)
    g = torch.Generator().manual_seed(62)
    dy1 = R.elem_round(torch.randn(n, c, generator=g) + 0.3, name)
    dpooled = dy1 * (h * w)
    cs = dict(cs, dy=Z.pooled_gradient(dpooled, h, w, name))
    cs = Z.with_mask(cs, cs["mask"])
    dy_dev = torch.full((n, h, w, c), 5.0, dtype=R.ELEM[name][0], device="cuda")          # does not exist yet: the launch writes it
    with frozen(name):
        out = run_bn_backward(name, cs, "bits", 1, dy_pooled=dpooled, dy_dev=dy_dev)
    _check_backward(name, cs, out, None, "folded pool gradient")
    assert torch.equal(out["dy_after"].cpu(), R.nhwc(cs["dy"]).to(R.ELEM[name][0]))


@pytest.mark.parametrize("name", NAMES)
def test_grid_barrier_backward_resident_and_not(name):
    """the LDS-residency branches of bn_bwd_fused_body, NB = 1: g and z resident across the barrier, and neither (g recomputed from dy
    and the bit map in phase 2).  Sizes from the launcher's own arithmetic; the test fails if a branch is not reached."""
    c, hw = 64, 32
    picked = {}
    for n in CROPS:
        _, keep_g, keep_z, _ = _residency(name, n * hw * hw, c)
        picked.setdefault((keep_g, keep_z), n)
    assert {(1, 1), (0, 0)} <= set(picked), picked
    for branch in ((1, 1), (0, 0)):
        cs = Z.case(picked[branch], hw, hw, c, 67 + picked[branch], name)
        with frozen(name):
            out = run_bn_backward(name, cs, "bits", 1)
        _check_backward(name, cs, out, None, "NB 1 resident %s" % (branch,))
        del cs, out


def _pair_cases(n, h, w, c, seed, name):
    """two frozen BatchNorms under one gradient and the mask of the stored sum of their outputs"""
    A, B = Z.case(n, h, w, c, seed, name, relu=False), Z.case(n, h, w, c, seed + 1, name, relu=False)
    act = (A["pre"] + B["pre"]).clamp_min(0)
    mask = R.elem_round(act.float(), name) > 0
    A, B = dict(A, act=act), dict(B, act=act, dy=A["dy"])
    return Z.with_mask(A, mask), Z.with_mask(B, mask)


@pytest.mark.parametrize("name", NAMES)
def test_pair_backward_resident_and_not(name):
    """bn_bwd_fused2_kernel (NB = 2): everything resident, and nothing (g parked in dy)"""
    c, hw = 64, 32
    picked = {}
    for n in CROPS:
        picked.setdefault(_residency(name, n * hw * hw, c, 1)[1:], n)
    assert {(1, 1, 1), (0, 0, 0)} <= set(picked), picked
    for branch in ((1, 1, 1), (0, 0, 0)):
        A, B = _pair_cases(picked[branch], hw, hw, c, 71 + picked[branch], name)
        with frozen(name):
            oA, oB = _run_pair(name, A, B)
        _check_backward(name, A, oA, None, "NB 2 resident %s, A" % (branch,))
        _check_backward(name, B, oB, None, "NB 2 resident %s, B" % (branch,))
        del A, B, oA, oB


def _apply_args(name, cs, keep):
    """one BatchNorm's arguments of vpd_op_bn_backward_apply(2): z, rows with sum g and sum g z, gamma, mean, rstd, dz, dgamma, dbeta"""
    dt = R.ELEM[name][0]
    n, c, h, w = cs["z"].shape
    zd = R.nhwc(cs["z"]).to(dt).cuda()
    rows = torch.zeros(4, 2, c, dtype=torch.float64)
    rows[1, 0], rows[2, 1] = cs["gm"].sum(dim=(0, 2, 3)), (cs["gm"] * cs["z"].double()).sum(dim=(0, 2, 3))
    rows = rows.cuda()
    gam, mu, rs = cs["gamma"].float().cuda(), cs["mean"].float().cuda(), cs["rstd"].float().cuda()
    dz = torch.full((n, h + 2, w + 2, c), 3.0, dtype=dt, device="cuda")
    dg, db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    keep += [zd, rows, gam, mu, rs]
    return (zd, rows, gam, mu, rs), (dz, dg, db)


def _apply_result(outs):
    dz, dg, db = outs
    assert _border_is(dz, 1, 3.0)
    return {"dz": _interior(dz, 1), "dgamma": dg.cpu().double(), "dbeta": db.cpu().double()}


@pytest.mark.parametrize("name", NAMES)
def test_finalize_and_apply_launch_single_and_pair(name):
    """bn_bwd_apply_fused_kernel<false> and <true>: the sums come from a data gradient's epilogue; B = D = 0"""
    n, h, w, c = 3, 9, 7, 64
    dt = R.ELEM[name][0]
    A, B = _pair_cases(n, h, w, c, 73, name)
    M = n * h * w
    dyd = R.nhwc(A["dy"]).to(dt).cuda()
    bits = R.mask_bits(R.nhwc(A["mask"]).reshape(M, c)).cuda()
    keep = []
    (zA, rA, gA, mA, sA), outA = _apply_args(name, A, keep)
    with frozen(name) as L:
        _check(L.vpd_op_bn_backward_apply(ptr(dyd), ptr(zA), ptr(bits), ptr(rA), ptr(gA), ptr(mA), ptr(sA), ptr(outA[0]), ptr(outA[1]),
                                          ptr(outA[2]), n, h, w, c, stream()), name)
    torch.cuda.synchronize()
    _check_backward(name, A, _apply_result(outA), None, "apply, single")
    (zA, rA, gA, mA, sA), outA = _apply_args(name, A, keep)
    (zB, rB, gB, mB, sB), outB = _apply_args(name, B, keep)
    with frozen(name) as L:
        _check(L.vpd_op_bn_backward_apply2(ptr(dyd), ptr(zA), ptr(bits), ptr(rA), ptr(gA), ptr(mA), ptr(sA), ptr(outA[0]), ptr(outA[1]),
                                           ptr(outA[2]), ptr(zB), ptr(rB), ptr(gB), ptr(mB), ptr(sB), ptr(outB[0]), ptr(outB[1]), ptr(outB[2]),
                                           n, h, w, c, stream()), name)
    torch.cuda.synchronize()
    _check_backward(name, A, _apply_result(outA), None, "apply, pair A")
    _check_backward(name, B, _apply_result(outB), None, "apply, pair B")


@pytest.mark.parametrize("name", NAMES)
def test_stem_pool_backward(name):
    """vpd_launch_stem_pool_bwd at 3 x 17 x 35 (odd: the pixel-at-a-time pass 2): sums over z, bn_bwd_finalize_kernel frozen, dz.
    The window taps are the forward launch's own (vpd_op_stem_pool_forward on the frozen scale / shift)."""
    n, H, W, c = 3, 17, 35, 64
    L = _lib(name)
    dt = R.ELEM[name][0]
    g = torch.Generator().manual_seed(79)
    z = R.elem_round(torch.randn(n, c, H, W, generator=g) * 1.3 - 0.2, name)
    rm, rv, gamma, beta = Z.frozen_params(c, g)
    mean, rstd = rm.clone(), Z.rstd_of(rv).float()
    scale = (gamma.double() * rstd.double()).float()
    shift = (beta.double() - mean.double() * scale.double()).float()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    zd = R.nhwc(z).to(dt).cuda()
    f32 = lambda t: t.float().cuda()
    scd, shd = f32(scale), f32(shift)
    pooled = torch.zeros(n, Ho + 2, Wo + 2, c, dtype=dt, device="cuda")
    idx = torch.zeros(n, Ho, Wo, c, dtype=torch.uint8, device="cuda")
    _check(L.vpd_op_stem_pool_forward(ptr(zd), ptr(scd), ptr(shd), ptr(pooled), ptr(idx), n, H, W, c, 1, stream()), name)
    torch.cuda.synchronize()
    taps = R.nchw(idx.cpu().long())
    xhat = (z.double() - Z._v(mean)) * Z._v(rstd)
    dpool = R.elem_round(torch.randn(n, c, Ho, Wo, generator=g) + 0.3, name)
    a = z.double() * Z._v(scale) + Z._v(shift)
    routed = R.route(dpool, taps, H, W)
    flip = R.relu_band(z, scale, shift, a) & (routed != 0)
    cs = {"z": z, "dy": routed, "gamma": gamma, "beta": beta, "mean": mean, "rstd": rstd}
    cs = Z.with_mask(cs, a > 0)
    dpd = R.nhwc(dpool).to(dt).cuda()
    rows = torch.zeros(16, 2, c, dtype=torch.float64, device="cuda")
    coef = torch.zeros(3, c, device="cuda")
    dz = torch.full((n, H, W, c), 3.0, dtype=dt, device="cuda")
    dg, db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    gam, bet, mu, rs = f32(gamma), f32(beta), f32(mean), f32(rstd)
    with frozen(name):
        _check(L.vpd_op_stem_pool_backward(ptr(dpd), ptr(idx), ptr(zd), ptr(mu), ptr(rs), ptr(scd), ptr(shd), ptr(gam), ptr(bet), None,
                                           ptr(rows), ptr(coef), ptr(dz), ptr(dg), ptr(db), n, H, W, c, stream()), name)
    torch.cuda.synchronize()
    assert float(rows.abs().max()) == 0.0                            # consumed: left zeroed
    assert float(coef[1:].abs().max()) == 0.0                        # c2 = c3 = 0
    out = {"dz": R.nchw(dz.cpu().double()), "dgamma": dg.cpu().double(), "dbeta": db.cpu().double()}
    _check_backward(name, cs, out, flip if bool(flip.any()) else None, "stem pool backward")


# ---- the hook leaks nothing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_hook_off_reproduces_the_unfrozen_launches_bit_for_bit(name):
    n, h, w, c = 4, 8, 8, 256
    cs = R.bn_backward_case(n, h, w, c, 7 * n + c, name, relu=True)

    def forward():
        L = _lib(name)
        dt = R.ELEM[name][0]
        zd, rows = R.nhwc(cs["z"]).to(dt).cuda(), _batch_rows(cs["z"], 4)
        gam, bet = cs["gamma"].float().cuda(), cs["beta"].float().cuda()
        rm, rv = torch.full((c,), 0.25, device="cuda"), torch.full((c,), 0.75, device="cuda")
        v = _bn_vectors(c)
        out = torch.full((n, h + 2, w + 2, c), 3.0, dtype=dt, device="cuda")
        _check(L.vpd_op_bn_forward(ptr(zd), ptr(rows), ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(v["mean"]), ptr(v["rstd"]), ptr(v["scale"]),
                                   ptr(v["shift"]), None, ptr(out), None, n, h, w, c, 1, F(0.1), F(R.BN_EPS), stream()), name)
        torch.cuda.synchronize()
        return [out, rm, rv] + [v[k] for k in sorted(v)]

    def backward():
        o = run_bn_backward(name, cs, "bits", 1)
        return [o["dz_raw"], o["dgamma"], o["dbeta"]]

    before = forward() + backward()
    with frozen(name):
        mid = forward() + backward()
    after = forward() + backward()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert not torch.equal(before[0], mid[0]) and not torch.equal(before[-3], mid[-3])      # (the hook did act in between)
    # unfrozen means train mode: against the batch-statistics reference of tests/test_bn_backward_ops_gpu.py
    assert R.rel_l2(_interior(after[-3], 1), cs["dz"]) < R.dz_l2_gate(name)


# ---- the streaming Bottleneck tails ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k64_w8", "two_w8"])
def test_streaming_tail_modes_under_the_hook(case):
    """conv1x1_bn_stream_kernel / conv1x1_bn2_stream_kernel, modes 0 .. 3, both libraries, on a budget of 8 CUs (the smallest
    grids vpd_op_conv1x1_bn_dispatch accepts: tests/bneck_tail_child.py's few-CU cases); a refused dispatch fails the test"""
    from tests.conv_ops_child import FEW
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "frozen_tail_child.py"), case], env=dict(os.environ, **FEW),
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    print(case, out["dispatch"], out["record"])
    assert out["dispatch"]["eligible"] == 1 and not out["fail"], "\n".join(out["fail"])
    for name in NAMES:
        assert out["record"]["%s/mode1/out" % name] <= 1.0 and out["record"]["%s/mode3/dz" % name] <= 1.0
