"""The stem convolution's data gradient one launch at a time (conv_stem_dgrad_kernel, vpd_amd/csrc/conv_stem_dgrad.hip) through
vpd_op_stem_dgrad, in both libraries, against float64 conv_transpose2d on the CPU (tests/opref_autograd.py; what that reference
and the bound rest on: tests/test_autograd_cpu.py).

Integer operands make every partial sum exact in fp32, so the assertion is EQUALITY: a dropped, transposed or misplaced tap, a
swapped column parity or a wrong border changes a result by at least 1/8.  randn operands check the arithmetic against the fp32
accumulator's running-error bound over the launch's longest sum (K = 1024), per element, none left out."""
import pytest
import torch

from tests import opref as R
from tests import opref_autograd as A
from tests.test_ops_gpu import ptr, stream

pytestmark = pytest.mark.gpu

GUARD = 256        # floats of NaN behind dx: nothing beyond the tensor may be written


def _stem_dgrad(name, dz, w, shift=0):
    """dz float64 NCHW [n][64][H/2][W/2] (values the element type holds), w [64][c_in][7][7] -> dx float64 NCHW.
    shift: floats by which dx is moved off its 16-byte alignment"""
    from vpd_amd._lib import check, lib
    n, _, hz, wz = dz.shape
    ci = w.shape[1]
    dzd = R.nhwc(dz).to(R.ELEM[name][0]).cuda()
    wd = w.float().contiguous().cuda()
    numel = n * ci * 4 * hz * wz
    buf = torch.full((GUARD + numel + GUARD,), float("nan"), device="cuda")
    out = buf[GUARD + shift:]
    assert out.data_ptr() % 16 == (4 * shift) % 16
    check(lib(name).vpd_op_stem_dgrad(ptr(dzd), ptr(wd), ptr(out), n, ci, 2 * hz, 2 * wz, stream()), "vpd_op_stem_dgrad", name)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD + shift]).all()), "wrote in front of dx"
    o = out.cpu()
    assert bool(torch.isnan(o[numel:]).all()), "wrote beyond dx"
    return o[:numel].view(n, ci, 2 * hz, 2 * wz).double()


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("case", list(A.STEM_DGRAD_CASES))
def test_stem_dgrad_integer_operands_equal_the_reference(case, name):
    dz, w, ref = A.stem_dgrad_int_operands(case)
    got = _stem_dgrad(name, dz, w)
    assert not bool(torch.isnan(got).any()), "%d elements not written" % int(torch.isnan(got).sum())
    assert torch.equal(got, ref), "%d of %d elements differ" % (int((got != ref).sum()), got.numel())


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("case", list(A.STEM_DGRAD_CASES))
def test_stem_dgrad_randn_operands_within_the_accumulator_bound(case, name):
    dz, w, ref, bound = A.stem_dgrad_randn_operands(case, name)
    got = _stem_dgrad(name, dz, w)
    err = (got - ref).abs()
    print(case, name, "max err / bound %.3f" % float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all()), "%d elements outside, worst err / bound %.3f" % (
        int((err > bound).sum()), float((err / bound.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_stem_dgrad_on_a_dx_that_is_only_8_byte_aligned(name):
    """W % 4 == 0 but dx 8 bytes off a 16-byte boundary: the launcher takes the 8-byte store path; 4 bytes off is refused"""
    from vpd_amd._lib import lib
    dz, w, ref = A.stem_dgrad_int_operands("h32_w48_c3")
    got = _stem_dgrad(name, dz, w, shift=2)
    assert torch.equal(got, ref), "%d of %d elements differ" % (int((got != ref).sum()), got.numel())
    buf = torch.zeros(ref.numel() + 8, device="cuda")
    h = lib(name)
    rc = h.vpd_op_stem_dgrad(ptr(buf), ptr(buf), ptr(buf[1:]), 2, 3, 32, 48, stream())      # refused on the host: nothing is read
    assert rc != 0 and b"8-byte aligned" in h.vpd_last_error()
