"""Frozen BatchNorm without a GPU: the float64 closed forms of tests/opref_frozen.py against torch autograd of
F.batch_norm(training=False), the new entry points in header == bindings == both libraries, and their host-side refusals."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import opref as R
from tests import opref_frozen as Z
from tests.test_abi_cpu import header_functions

NEW_SYMBOLS = ("vpd_plan_set_bn_frozen", "vpd_plan_set_param_grads", "vpd_op_set_bn_frozen", "vpd_op_bn_forward2",
               "vpd_op_bn_finalize", "vpd_op_bn_backward_apply2")
TOL = 1e-12


def _close(a, b):
    return float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


def _autograd(z, gamma, beta, rm, rv, dy, res=None, relu=True, pool=False):
    zt, gt, bt = z.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.batch_norm(zt, rm.double(), rv.double(), gt, bt, training=False, eps=R.BN_EPS)
    if res is not None:
        y = y + res.double()
    a = y.clamp_min(0) if relu else y
    if pool:
        (a.mean(dim=(2, 3)) * dy.double()).sum().backward()
    else:
        (a * dy.double()).sum().backward()
    return a.detach(), y.detach(), zt.grad, gt.grad, bt.grad


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("relu,residual", [(True, False), (True, True), (False, False)], ids=["relu", "relu_res", "plain"])
def test_closed_forms_equal_autograd_of_eval_mode_batch_norm(relu, residual, name):
    cs = Z.case(3, 9, 7, 64, 11, name, relu=relu, residual=residual)
    a, y, dz, dgamma, dbeta = _autograd(cs["z"], cs["gamma"], cs["beta"], cs["rm"], cs["rv"], cs["dy"], cs["res"], relu)
    assert _close(cs["out"], a) and _close(cs["pre"], y)
    # the backward references take the saved statistics: in float64 here, so that only the formula is compared
    gm = cs["dy"].double() * (y > 0 if relu else torch.ones_like(y, dtype=torch.bool))
    rdz, rdg, rdb = Z.backward(cs["z"], cs["gamma"], cs["rm"], Z.rstd_of(cs["rv"]), gm)
    assert _close(rdz, dz) and _close(rdg, dgamma) and _close(rdb, dbeta)
    # ... and with the fp32 rstd the kernels get, the case's own references move by that rounding only
    assert float((cs["dz"] - dz).abs().max()) <= 2.0 ** -23 * float(dz.abs().max())
    # frozen is not train mode: the running statistics are far from the batch's own
    mean, rstd = R.stem_stats(cs["z"])
    assert float((mean - cs["rm"].double()).abs().mean()) > 0.2
    assert float((rstd / Z.rstd_of(cs["rv"]) - 1).abs().mean()) > 0.1


def test_pair_form_is_two_backwards_of_one_masked_gradient():
    """out = relu(BN_A(zA) + BN_B(zB)): both BatchNorms see g = dy * [out > 0]"""
    g = torch.Generator().manual_seed(5)
    n, c, h, w = 3, 64, 7, 5
    zA, zB = torch.randn(n, c, h, w, generator=g) * 1.3 - 0.2, torch.randn(n, c, h, w, generator=g) * 0.8 + 0.4
    pA, pB = Z.frozen_params(c, g), Z.frozen_params(c, g)
    dy = torch.randn(n, c, h, w, generator=g)
    ts = [t.double().requires_grad_(True) for t in (zA, pA[2], pA[3], zB, pB[2], pB[3])]
    y = (F.batch_norm(ts[0], pA[0].double(), pA[1].double(), ts[1], ts[2], training=False, eps=R.BN_EPS)
         + F.batch_norm(ts[3], pB[0].double(), pB[1].double(), ts[4], ts[5], training=False, eps=R.BN_EPS))
    (y.clamp_min(0) * dy.double()).sum().backward()
    outA, preA = Z.forward(zA, pA[2], pA[3], pA[0], pA[1], relu=False)
    outB, _ = Z.forward(zB, pB[2], pB[3], pB[0], pB[1], relu=False)
    assert _close(outA + outB, y.detach())
    gm = dy.double() * (y.detach() > 0)
    (dzA, dgA, dbA), (dzB, dgB, dbB) = Z.backward_pair(zA, pA[2], pA[0], Z.rstd_of(pA[1]), zB, pB[2], pB[0], Z.rstd_of(pB[1]), gm)
    for got, t in zip((dzA, dgA, dbA, dzB, dgB, dbB), ts):
        assert _close(got, t.grad)
    assert torch.equal(dbA, dbB)


def test_folded_average_pool_gradient_is_the_pooled_gradient_spread():
    g = torch.Generator().manual_seed(9)
    n, c, h, w = 5, 64, 4, 4
    z = torch.randn(n, c, h, w, generator=g)
    rm, rv, gamma, beta = Z.frozen_params(c, g)
    dy1 = R.elem_round(torch.randn(n, c, generator=g), "bf16")
    dpooled = dy1 * (h * w)                                    # exact: H W is a power of two
    dy = Z.pooled_gradient(dpooled, h, w, "bf16")
    assert torch.equal(dy[:, :, 2, 3], dy1)
    _, y, dz, dgamma, dbeta = _autograd(z, gamma, beta, rm, rv, dpooled, relu=True, pool=True)
    rdz, rdg, rdb = Z.backward(z, gamma, rm, Z.rstd_of(rv), dy.double() * (y > 0))
    assert _close(rdz, dz) and _close(rdg, dgamma) and _close(rdb, dbeta)


def test_bounds_resolve_a_kernel_on_the_wrong_statistics():
    """what the GPU test relies on: the batch-statistics result and the rm = 0 / rv = 1 result lie far outside the bounds -- ten
    bounds and more on a quarter of the elements (about half of them are zero behind the ReLU either way)"""
    name = "bf16"
    cs = Z.case(2, 16, 16, 64, 3, name)
    mean, rstd = R.stem_stats(cs["z"])
    bound = Z.out_bound(cs["out"], cs["z"], cs["gamma"], cs["beta"], cs["rm"], cs["rv"], name)
    train = (Z._v(cs["gamma"]) * (cs["z"].double() - Z._v(mean)) * Z._v(rstd) + Z._v(cs["beta"])).clamp_min(0)
    default, _ = Z.forward(cs["z"], cs["gamma"], cs["beta"], torch.zeros(64), torch.ones(64))
    for wrong in (train, default):
        assert float(((wrong - cs["out"]).abs() > 10 * bound).double().mean()) > 0.25
    gm = cs["gm"]
    wrong_dz = R.bn_dz_closed_form(cs["z"], cs["gamma"], cs["mean"], cs["rstd"], gm)       # the train-mode formula on frozen statistics
    assert float(((wrong_dz - cs["dz"]).abs() > 10 * Z.dz_bound(cs["dz"], name)).double().mean()) > 0.25


def test_new_symbols_in_header_bindings_and_both_libraries():
    from vpd_amd import _lib
    names = header_functions()
    for sym in NEW_SYMBOLS:
        assert sym in names and sym in _lib.SIGNATURES
        for dtype in ("bf16", "fp16"):
            assert getattr(_lib.lib(dtype), sym) is not None
    assert _lib.ABI_VERSION == 5 and _lib.lib().vpd_abi_version() == 5 and _lib.lib("fp16").vpd_abi_version() == 5


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_host_refusals(dtype):
    from vpd_amd import _lib
    L = _lib.lib(dtype)
    assert L.vpd_plan_set_bn_frozen(None, 1) != 0 and b"null plan" in L.vpd_last_error()
    assert L.vpd_plan_set_param_grads(None, 0) != 0 and b"null plan" in L.vpd_last_error()
    p = C.c_void_p()
    _lib.check(L.vpd_plan_create(b"resnet18", 5, 64, 64, 32, 0, 8, 0, C.byref(p)), "create", dtype)      # an inference plan
    assert L.vpd_plan_set_bn_frozen(p, 1) != 0 and b"train=0" in L.vpd_last_error()
    assert L.vpd_plan_set_bn_frozen(p, 0) != 0
    assert L.vpd_plan_set_param_grads(p, 0) != 0 and b"train=0" in L.vpd_last_error()
    L.vpd_plan_destroy(p)
    _lib.check(L.vpd_plan_create(b"resnet50", 5, 64, 64, 32, 0, 8, 1, C.byref(p)), "create", dtype)      # a train plan takes both
    for on in (1, 0):
        assert L.vpd_plan_set_bn_frozen(p, on) == 0 and L.vpd_plan_set_param_grads(p, on) == 0
    L.vpd_plan_destroy(p)
    assert L.vpd_op_set_bn_frozen(1) == 0 and L.vpd_op_set_bn_frozen(0) == 0
