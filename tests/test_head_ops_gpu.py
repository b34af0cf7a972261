"""The embedding head one launch at a time (avgpool_kernel, avgpool_bwd_kernel, sgemm_small_kernel, sgemm_nt_splitk_kernel,
colsum_kernel, relu_mask_kernel, mse_kernel; vpd_amd/csrc/head.hip) through the vpd_op_* entry points, against float64 PyTorch on
the CPU.  The head is fp32: integer inputs whose sums stay below 2^24 make every fp32 sum exact in any order, so the assertion is
EQUALITY -- a dropped, duplicated or misplaced element changes a result by at least 1 -- and randn inputs check the arithmetic
against the running-error bound of an fp32 dot product, |got - ref| <= (K + 4) 2^-24 (|A| |B|)[m][n]."""
import ctypes as C
import math

import pytest
import torch

from tests import opref as R
from tests.test_ops_gpu import ptr, stream

pytestmark = pytest.mark.gpu


def _lib(name="bf16"):
    from vpd_amd._lib import lib
    return lib(name)


def _check(rc, name="bf16"):
    from vpd_amd._lib import check
    check(rc, "op", name)


def _sgemm(case, A, B, bv):
    """A [M][K], B [K][N] as mathematical operands; stored as the case's ta / tb ask.  Y is over-allocated and pre-filled with
    NaN: nothing beyond M x N may be written."""
    _, M, N, K, ta, tb, bias, relu = case
    Ad = (A.t().contiguous() if ta else A.contiguous()).cuda()
    Bd = (B.t().contiguous() if tb else B.contiguous()).cuda()
    Y = torch.full((M * N + 64,), float("nan"), device="cuda")
    bd = bv.cuda() if bv is not None else None
    _check(_lib().vpd_op_sgemm(ptr(Ad), ptr(Bd), ptr(Y), ptr(bd) if bd is not None else None, M, N, K, ta, tb, relu, stream()))
    torch.cuda.synchronize()
    y = Y.cpu()
    assert bool(torch.isnan(y[M * N:]).all()), "wrote beyond Y"
    return y[:M * N].view(M, N).double()


def _sgemm_ref(case, A, B, bv):
    ref = A.double() @ B.double()
    if bv is not None:
        ref = ref + bv.double()
    return ref.clamp_min(0) if case[7] else ref


SGEMM = R.sgemm_cases()


@pytest.mark.parametrize("case", SGEMM, ids=[c[0] for c in SGEMM])
def test_sgemm_integer_inputs_equal_and_randn_within_the_dot_product_bound(case):
    _, M, N, K, ta, tb, bias, relu = case
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A, B, bv = R.sgemm_operands(case, g, True)
    got, ref = _sgemm(case, A, B, bv), _sgemm_ref(case, A, B, bv)
    assert torch.equal(got, ref), "%d of %d elements differ" % (int((got != ref).sum()), got.numel())
    A, B, bv = R.sgemm_operands(case, g, False)
    got, ref = _sgemm(case, A, B, bv), _sgemm_ref(case, A, B, bv)
    mag = A.double().abs() @ B.double().abs() + (bv.double().abs() if bv is not None else 0.0)
    bound = (K + 4) * 2.0 ** -24 * mag
    err = (got - ref).abs()
    print(case[0], "max err / bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())
    # resolution: the product 2 % off is outside the bound
    off = _sgemm_ref(case, A * 1.02, B, bv)
    assert not bool(((got - off).abs() <= bound).all())


def test_sgemm_kernel_choice_follows_the_k_tail():
    """K % 64 == 0 with tb = 1 is the split-K kernel's shape, everything else the small kernel's (K = 32: one 32-wide trip;
    K = 40, 37, 5: a tail inside the trip): both agree with each other where only the layout differs"""
    g = torch.Generator().manual_seed(3)
    for K in (32, 40, 64, 128, 192):
        A, B = R.int_matrix((17, K), -7, 7, g), R.int_matrix((K, 40), -7, 7, g)
        a = _sgemm(("nt", 17, 40, K, 0, 1, 0, 0), A, B, None)
        b = _sgemm(("nn", 17, 40, K, 0, 0, 0, 0), A, B, None)
        c = _sgemm(("tn", 17, 40, K, 1, 0, 0, 0), A, B, None)
        ref = A.double() @ B.double()
        assert torch.equal(a, ref) and torch.equal(b, ref) and torch.equal(c, ref), K


def _mse(e, t, want_de=True, accum=None):
    n = e.numel()
    ed, td = e.cuda(), t.cuda()
    de = torch.full((n + 8,), float("nan"), device="cuda")
    step = torch.full((1,), float("nan"), device="cuda")
    acc = accum if accum is not None else torch.zeros(1, dtype=torch.float64, device="cuda")
    _check(_lib().vpd_op_mse(ptr(ed), ptr(td), n, ptr(de) if want_de else None, ptr(step), ptr(acc), stream()))
    torch.cuda.synchronize()
    return de.cpu(), float(step.cpu()[0]), acc


@pytest.mark.parametrize("n", R.MSE_SIZES)
def test_mse_loss_and_gradient(n):
    g = torch.Generator().manual_seed(n)
    e, t = R.mse_int_operands(n, g)
    d = (e - t).double()
    want = float((d * d).sum())
    de, step, acc = _mse(e, t)
    assert step == want
    assert torch.equal(de[:n].double(), 2 * d) and bool(torch.isnan(de[n:]).all())
    de2, step2, acc = _mse(e, t, want_de=False, accum=acc)
    assert step2 == want and float(acc.cpu()[0]) == 2 * want            # loss_accum adds up over calls
    assert bool(torch.isnan(de2).all())                                 # de null: nothing written
    # randn: de is 2 (e - t) evaluated in fp32, the loss within the longest chain of additions of the kernel
    e, t = torch.randn(n, generator=g), torch.randn(n, generator=g)
    de, step, _ = _mse(e, t)
    assert torch.equal(de[:n], 2.0 * (e - t))
    d = (e - t).double()                                                # (fp32 difference, as the kernel forms it, squared in float64)
    want = float((d * d).sum())
    bound = (math.ceil(n / 1024) + 32) * 2.0 ** -24 * want
    print("n %d: loss err / bound %.3f" % (n, abs(step - want) / bound))
    assert abs(step - want) <= bound
    assert abs(step - 1.02 * want) > bound                              # resolution


AVG_CASES = [(5, 4, 4, 512), (3, 4, 4, 2048), (7, 2, 2, 512), (2, 8, 8, 512), (5, 3, 5, 2048), (37, 4, 4, 512)]


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("case", AVG_CASES, ids=["n%d_%dx%d_c%d" % c for c in AVG_CASES])
def test_avgpool_forward_and_backward(case, name):
    n, H, W, c = case
    L = _lib(name)
    dt = R.ELEM[name][0]
    g = torch.Generator().manual_seed(n * 100 + H * 10 + W + c)
    # small-integer activations: every partial sum is exact; the mean is exact when H W is a power of two.  The border is NOT
    # zero: only the interior may be read
    for integer in (True, False):
        act = R.int_matrix((n, H, W, c), -8, 8, g) if integer else R.elem_round(torch.randn(n, H, W, c, generator=g), name)
        buf = torch.full((n, H + 2, W + 2, c), 99.0)
        buf[:, 1:-1, 1:-1] = act
        bd = buf.to(dt).cuda()
        pooled = torch.full((n * c + 8,), float("nan"), device="cuda")
        _check(L.vpd_op_avgpool(ptr(bd), n, H, W, c, 1, ptr(pooled), stream()), name)
        torch.cuda.synchronize()
        got = pooled.cpu()
        assert bool(torch.isnan(got[n * c:]).all())
        got = got[:n * c].view(n, c).double()
        ref = act.double().mean(dim=(1, 2))
        if integer and (H * W) & (H * W - 1) == 0:
            assert torch.equal(got, ref)
        else:
            # H W fp32 additions and one multiplication by fl(1 / (H W))
            bound = (H * W + 2) * 2.0 ** -24 * act.double().abs().mean(dim=(1, 2)) + 1e-30
            assert bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() / bound).max())
            assert not bool(((got - 1.02 * ref).abs() <= bound).all())
    # backward: dact = elem(dpooled / (H W)), dense, every pixel of an image the same
    dp = torch.randn(n, c, generator=g)
    dact = torch.full((n * H * W * c + 8,), 5.0, dtype=dt, device="cuda")
    dpd = dp.cuda()
    _check(L.vpd_op_avgpool_bwd(ptr(dpd), n, H, W, c, ptr(dact), stream()), name)
    torch.cuda.synchronize()
    got = dact.cpu()
    assert bool((got[n * H * W * c:].float() == 5.0).all())
    want = (dp.double() / (H * W)).to(dt).view(n, 1, 1, c).expand(n, H, W, c)      # elem(dpooled / (H W))
    g_ = got[:n * H * W * c].view(n, H, W, c)
    print("avgpool_bwd %s: %d of %d elements differ from elem(dpooled / (H W))" % (name, int((g_ != want).sum()), g_.numel()))
    assert torch.equal(g_, want)


@pytest.mark.parametrize("shape", [(1, 1), (5, 40), (17, 128), (256, 33), (1000, 256), (37, 2048), (9, 31)])
def test_colsum_and_relu_mask(shape):
    M, N = shape
    L = _lib()
    g = torch.Generator().manual_seed(M + N)
    A = R.int_matrix((M, N), -50, 50, g)                                # |column sum| <= 50,000 < 2^24
    out = torch.full((N + 8,), float("nan"), device="cuda")
    Ad = A.cuda()
    _check(L.vpd_op_colsum(ptr(Ad), M, N, ptr(out), stream()))
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[:N].double(), A.double().sum(0)) and bool(torch.isnan(got[N:]).all())
    Ar = torch.randn(M, N, generator=g)
    Ard = Ar.cuda()
    _check(L.vpd_op_colsum(ptr(Ard), M, N, ptr(out), stream()))
    torch.cuda.synchronize()
    err = (out.cpu()[:N].double() - Ar.double().sum(0)).abs()
    assert bool((err <= (M / 8 + 12) * 2.0 ** -24 * Ar.double().abs().sum(0)).all())      # chains of M / 8 + 8 additions
    # ReLU mask of the MLP's hidden gradients: d = act > 0 ? d : 0, in place, nothing beyond n
    n = M * N
    d = R.int_matrix((n + 8,), -9, 9, g)
    act = R.int_matrix((n + 8,), -2, 2, g)                              # zeros and negatives among them
    dd, ad = d.cuda(), act.cuda()
    _check(L.vpd_op_relu_mask(ptr(dd), ptr(ad), n, stream()))
    torch.cuda.synchronize()
    want = d.clone()
    want[:n] = torch.where(act[:n] > 0, d[:n], torch.zeros(n))
    assert torch.equal(dd.cpu(), want)


def test_relu_mask_many_trips():
    """more elements than the launch has threads (1,024 blocks x 256): the grid-stride loop's second and third trips"""
    n = 3 * 1024 * 256 + 77
    g = torch.Generator().manual_seed(n)
    d, act = R.int_matrix((n,), -9, 9, g), R.int_matrix((n,), -2, 2, g)
    dd, ad = d.cuda(), act.cuda()
    _check(_lib().vpd_op_relu_mask(ptr(dd), ptr(ad), n, stream()))
    torch.cuda.synchronize()
    assert torch.equal(dd.cpu(), torch.where(act > 0, d, torch.zeros(n)))
