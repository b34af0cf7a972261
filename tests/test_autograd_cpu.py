"""Host-side checks of the autograd path's library additions (vpd_backward_ext, vpd_op_stem_dgrad: declared, bound, exported under
ABI 5; every refusal happens on the host with its message, before anything is launched) and of what the GPU tests of the stem
convolution's data gradient rest on: the float64 reference, the kernel's parity decomposition and a bound that is not vacuous."""
import ctypes as C

import pytest
import torch

from tests import opref as R
from tests import opref_autograd as A
from tests.test_abi_cpu import header_functions

FAKE = C.c_void_p(64)          # never dereferenced: every call below is rejected on the host


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_new_entry_points_are_declared_bound_and_exported(dtype):
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    assert h.vpd_abi_version() == _lib.ABI_VERSION == 5
    for n, nargs in (("vpd_backward_ext", 9), ("vpd_op_stem_dgrad", 8)):
        assert n in header_functions() and len(_lib.SIGNATURES[n][1]) == nargs and getattr(h, n).argtypes == _lib.SIGNATURES[n][1]


def _plan(h, dtype, train, motion, max_batch=4):
    from vpd_amd import _lib
    p = C.c_void_p()
    _lib.check(h.vpd_plan_create(b"resnet18", 5, 64, 64, 32, motion, max_batch, train, C.byref(p)), "create", dtype)
    return p


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_backward_ext_refuses_on_the_host(dtype):
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    p = _plan(h, dtype, 1, 0)
    good = [p, FAKE, FAKE, FAKE, 4, None, None, FAKE, None]
    for pos in (0, 1, 2, 3, 7):                                  # plan, params, grads, d_emb, workspace
        args = list(good)
        args[pos] = None
        assert h.vpd_backward_ext(*args) != 0 and b"null" in h.vpd_last_error(), pos
    for n in (-1, 5):
        args = list(good)
        args[4] = n
        assert h.vpd_backward_ext(*args) != 0 and b"batch size" in h.vpd_last_error(), n
    # every argument in order, the workspace never bound by vpd_plan_init_workspace (n == 0 included)
    assert h.vpd_backward_ext(*good) != 0 and b"workspace not initialised" in h.vpd_last_error()
    args = list(good)
    args[4] = 0
    assert h.vpd_backward_ext(*args) != 0 and b"workspace not initialised" in h.vpd_last_error()
    h.vpd_plan_destroy(p)
    p = _plan(h, dtype, 0, 0)
    assert h.vpd_backward_ext(p, FAKE, FAKE, FAKE, 4, None, None, FAKE, None) != 0 and b"train=0" in h.vpd_last_error()
    h.vpd_plan_destroy(p)
    p = _plan(h, dtype, 1, 1)
    assert h.vpd_backward_ext(p, FAKE, FAKE, FAKE, 4, None, None, FAKE, None) != 0 and b"motion head" in h.vpd_last_error()
    h.vpd_plan_destroy(p)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_stem_dgrad_refuses_on_the_host(dtype):
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    good = [FAKE, FAKE, FAKE, 2, 5, 32, 32, None]
    for pos in (0, 1, 2):
        args = list(good)
        args[pos] = None
        assert h.vpd_op_stem_dgrad(*args) != 0 and b"null argument" in h.vpd_last_error(), pos
    for pos, bad, msg in ((3, 0, b"n must"), (3, -2, b"n must"), (4, 0, b"c_in"), (4, 9, b"c_in"), (5, 33, b"even"), (5, 30, b"even"),
                          (6, 47, b"even"), (6, 16, b"even")):
        args = list(good)
        args[pos] = bad
        assert h.vpd_op_stem_dgrad(*args) != 0 and msg in h.vpd_last_error(), (pos, bad)
    args = list(good)
    args[2] = C.c_void_p(68)                                     # 4 bytes off: the kernel's pair stores are 8 bytes wide
    assert h.vpd_op_stem_dgrad(*args) != 0 and b"8-byte aligned" in h.vpd_last_error()


@pytest.mark.parametrize("case", ["min32_c5", "h32_w48_c3", "min32_c1"])
def test_transposed_convolution_autograd_and_the_parity_decomposition_agree(case):
    """float64: conv_transpose2d(dz, w, 2, 3, output_padding 1) == autograd of conv2d(x, w, stride 2, padding 3) == the sum over
    (row parity, column parity, dox, ky) the kernel runs"""
    n, ci, h, w_ = A.STEM_DGRAD_CASES[case]
    g = torch.Generator().manual_seed(h * 5 + w_)
    dz = torch.randn(n, 64, h // 2, w_ // 2, generator=g, dtype=torch.float64)
    w = torch.randn(64, ci, 7, 7, generator=g, dtype=torch.float64)
    ref = A.stem_dgrad_ref(dz, w)
    scale = float(ref.abs().max())
    assert float((A.stem_dgrad_autograd(dz, w) - ref).abs().max()) <= 1e-12 * scale
    assert float((A.stem_dgrad_parity(dz, w) - ref).abs().max()) <= 1e-12 * scale
    # even rows take 3 kernel rows, odd rows 4; 7 of the 8 (xpar, dox) slots are real
    assert [len(range((Y + 1) % 2, 7, 2)) for Y in (0, 1)] == [3, 4]
    assert sum(0 <= xp + 3 - 2 * d <= 6 for xp in range(2) for d in range(-1, 3)) == 7


def test_integer_operands_are_exact_and_asymmetric():
    dz, w, ref = A.stem_dgrad_int_operands("min32_c5")
    assert float(dz.abs().max()) == 3 and bool((dz == dz.round()).all()) and 0.3 < float((dz != 0).double().mean()) < 0.7
    assert bool((w * 8 == (w * 8).round()).all()) and float(w.abs().max()) == 1.0
    for name in ("bf16", "fp16"):
        assert torch.equal(R.elem_round(dz.float(), name).double(), dz) and torch.equal(R.elem_round(w.float(), name).double(), w)
    # a transposed tap, a mirrored kernel or exchanged channels give another result
    assert not torch.equal(w, w.transpose(2, 3)) and not torch.equal(w, w.flip(2)) and not torch.equal(w, w.flip(3))
    assert not torch.equal(w[:, 0], w[:, 1]) and not torch.equal(w[0], w[1])
    for alt in (w.transpose(2, 3), w.flip(3), w.flip(1)):
        assert not torch.equal(A.stem_dgrad_ref(dz, alt), ref)
    # the largest sum of magnitudes stays where fp32 is exact in eighths: below 2^24 / 8
    assert float(A.stem_dgrad_ref(dz.abs(), w.abs()).max()) <= 3072 < 2 ** 21
    assert torch.equal(ref.float().double(), ref)


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("case", ["min32_c5", "h32_w48_c3"])
def test_the_bound_rejects_a_missing_tap_and_swapped_parities(case, name):
    """The randn operands of the GPU test: the float64 result with one tap (ky, kx) left out on one output row, and the one with
    the parities of one column pair exchanged, are outside the bound somewhere; the reference itself, rounded to fp32 (the best a
    kernel can return), is inside everywhere."""
    dz, w, ref, bound = A.stem_dgrad_randn_operands(case, name)
    wq = R.elem_round(w, name).double()
    assert bool(((ref.float().double() - ref).abs() <= bound).all())
    assert float((A.stem_dgrad_parity(dz, wq) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    n, ci, h, w_ = A.STEM_DGRAD_CASES[case]
    for Y, tap in ((h // 2, (1, 2)), (h // 2 + 1, (6, 0)), (0, (3, 6))):
        assert (Y + 1 - tap[0]) % 2 == 0                          # the tap belongs to the row's parity
        alt = A.stem_dgrad_parity(dz, wq, skip_tap=tap, skip_row=Y)
        bad = (alt - ref).abs() > bound
        assert bool(bad.any()) and bool(bad[:, :, Y].any()) and not bool(bad[:, :, :Y].any()) and not bool(bad[:, :, Y + 1:].any())
    for j in (0, w_ // 4, w_ // 2 - 1):
        alt = A.stem_dgrad_parity(dz, wq, swap_pair=j)
        bad = (alt - ref).abs() > bound
        assert bool(bad[:, :, :, 2 * j:2 * j + 2].any()) and int(bad.sum()) == int(bad[:, :, :, 2 * j:2 * j + 2].sum())
    # the bound is tight in relative terms: far below the result's own size
    assert float(bound.max()) <= 1e-3 * float(ref.abs().max())
