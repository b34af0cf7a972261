"""CPU-side checks of the C-ABI boundary: the shared library loads, exports
every symbol include/vpd_hip.h declares, and its host-only plan functions
describe the reference's state_dict layout (no GPU compute is called)."""
import ctypes as C
import os
import re

import pytest

from oracle import vpd_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(REPO, "include", "vpd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vpd_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from vpd_amd import _lib
    names = header_functions()
    assert len(names) >= 20
    assert sorted(_lib.SIGNATURES.keys()) == names
    h = _lib.lib()
    for n in names:
        assert getattr(h, n) is not None
    assert h.vpd_abi_version() == _lib.ABI_VERSION
    assert h.vpd_elem_dtype() == b"bf16"


def test_fp16_library_exports_the_same_abi():
    """libvpdhip_f16.so = the same sources with fp16 elements: same symbols, same ABI version, its own element type; the loss
    scale (fp16 training) is validated on the host."""
    from vpd_amd import _lib
    h = _lib.lib("fp16")
    for n in header_functions():
        assert getattr(h, n) is not None
    assert h.vpd_abi_version() == _lib.ABI_VERSION and h.vpd_elem_dtype() == b"fp16"
    p = C.c_void_p()
    _lib.check(h.vpd_plan_create(b"resnet34", 5, 128, 128, 128, 0, 4, 1, C.byref(p)), "create", "fp16")
    assert h.vpd_plan_param_numel(p) == 21356608      # (host-only call on the fp16 plan: ResNet-34, 5 channels, D = 128, no motion head)
    assert h.vpd_plan_set_loss_scale(p, 256.0) == 0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert h.vpd_plan_set_loss_scale(p, bad) != 0 and b"loss scale" in h.vpd_last_error()
    h.vpd_plan_destroy(p)
    with pytest.raises(_lib.VpdHipError):
        _lib.lib("fp32")


@pytest.mark.parametrize("arch,c_in,D,motion", [("resnet34", 5, 128, 1), ("resnet18", 3, 32, 0)])
def test_plan_layout_matches_reference_schema(arch, c_in, D, motion):
    from vpd_amd._lib import check, lib
    L = lib()
    h = C.c_void_p()
    check(L.vpd_plan_create(arch.encode(), c_in, 128, 128, D, motion, 4, 1, C.byref(h)), "create")
    sch = O.encoder_schema(arch, c_in, D)
    names = O.trainable_keys(sch)
    shapes = [tuple(sch[k][0]) for k in names]
    if motion:
        ds = O.decoder_schema(D)
        names += list(ds.keys())
        shapes += [tuple(v[0]) for v in ds.values()]
    assert L.vpd_plan_num_tensors(h) == len(names)
    kind, dec, off, numel, ndim = C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong(), C.c_int()
    dims = (C.c_int * 4)()
    expect_off = 0
    for i, shp in enumerate(shapes):
        check(L.vpd_plan_tensor_info(h, i, C.byref(kind), C.byref(dec), C.byref(off), C.byref(numel), C.byref(ndim), dims), "info")
        assert tuple(dims[k] for k in range(ndim.value)) == shp, names[i]
        assert off.value == expect_off
        expect_off += numel.value
    total = expect_off
    if arch == "resnet34" and c_in == 5 and D == 128:
        assert total == 21356608 + 66048            # SURVEY.md 2.3 parameter counts
    assert L.vpd_plan_param_numel(h) == (total + 3) // 4 * 4
    # buckets tile the flat buffer exactly, in reverse stage order
    rng = []
    o, m = C.c_longlong(), C.c_longlong()
    for b in range(L.vpd_plan_num_buckets(h)):
        check(L.vpd_plan_bucket_range(h, b, C.byref(o), C.byref(m)), "bucket")
        rng.append((o.value, m.value))
    rng_sorted = sorted(rng)
    assert rng_sorted[0][0] == 0 and sum(m for _, m in rng) == total
    for (o1, m1), (o2, _) in zip(rng_sorted, rng_sorted[1:]):
        assert o1 + m1 == o2
    assert rng[0][0] > rng[1][0] > rng[2][0] > rng[3][0] == 0
    nbn = sum(1 for k, (_, kind_) in sch.items() if kind_ == "bn_rm")
    assert L.vpd_plan_num_bn(h) == nbn
    assert L.vpd_plan_workspace_bytes(h) > 0
    L.vpd_plan_destroy(h)


def test_plan_rejects_bad_arguments():
    from vpd_amd._lib import lib
    L = lib()
    h = C.c_void_p()
    assert L.vpd_plan_create(b"effnet-b0", 5, 128, 128, 128, 0, 4, 1, C.byref(h)) != 0      # EfficientNet: out of scope
    assert b"unsupported arch" in L.vpd_last_error()
    for arch in (b"resnet50", b"wide_resnet101_2"):          # Bottleneck archs plan without a GPU too
        assert L.vpd_plan_create(arch, 5, 128, 128, 128, 0, 4, 1, C.byref(h)) == 0
        assert L.vpd_plan_param_numel(h) > 20000000
        L.vpd_plan_destroy(h)
    assert L.vpd_plan_create(b"resnet34", 9, 128, 128, 128, 0, 4, 1, C.byref(h)) != 0
    assert L.vpd_plan_create(b"resnet34", 5, 127, 128, 128, 0, 4, 1, C.byref(h)) != 0


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_conv_dispatch_and_two_batchnorm_sums_reject_bad_arguments(dtype):
    """ABI 5: vpd_op_conv2d_dispatch (host-only) and vpd_op_conv2d_bnsums2 return non-zero with a message on null or malformed
    arguments, before anything is launched."""
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    out = (C.c_int * 12)()
    taps = (C.c_int * 9)(3, 3, 0, 1, 0, 1, 0, 3, 1)
    good = [4, 18, 18, 128, 16, 16, 128, 0, 16, 16, 1, 0, 0, 1, 128, 128]
    assert h.vpd_op_conv2d_dispatch(*good, taps, 0, 1, out) == 0 and out[9] == 1 and out[7] in (128, 256)
    assert h.vpd_op_conv2d_dispatch(*good, None, 0, 1, out) != 0 and b"null argument" in h.vpd_last_error()
    assert h.vpd_op_conv2d_dispatch(*good, taps, 0, 1, None) != 0 and b"null argument" in h.vpd_last_error()
    for pos, bad in ((0, 0), (14, 96), (15, 32), (10, 0), (13, 0), (6, 64)):      # crops, Kc, Co, osub, istr, yC < Co
        args = list(good)
        args[pos] = bad
        assert h.vpd_op_conv2d_dispatch(*args, taps, 0, 1, out) != 0 and b"bad argument" in h.vpd_last_error(), pos
    assert h.vpd_op_conv2d_dispatch(*good, taps, 0, 64, out) != 0 and b"bad argument" in h.vpd_last_error()
    assert h.vpd_op_conv2d_dispatch(*good, taps, 1, 16, out) != 0 and b"second BatchNorm" in h.vpd_last_error()
    assert h.vpd_op_conv2d_dispatch(*good, (C.c_int * 9)(0, 3, 0, 1, 0, 1, 0, 3, 1), 0, 1, out) != 0 and b"empty tap set" in h.vpd_last_error()
    p = C.c_void_p(64)                                    # never dereferenced: every call below is rejected on the host
    assert h.vpd_op_conv2d_bnsums2(p, p, p, p, p, p, None, p, 4, 18, 18, 128, 16, 16, 128, 128, taps, None) != 0
    assert b"null argument" in h.vpd_last_error()
    assert h.vpd_op_conv2d_bnsums2(p, p, p, p, p, p, p, None, 4, 18, 18, 128, 16, 16, 128, 128, taps, None) != 0
    assert h.vpd_op_conv2d_bnsums2(None, p, p, p, p, p, p, p, 4, 18, 18, 128, 16, 16, 128, 128, taps, None) != 0
    assert h.vpd_op_conv2d_bnsums2(p, p, p, p, p, p, p, p, 4, 18, 18, 128, 16, 16, 100, 128, taps, None) != 0
    assert b"bad argument" in h.vpd_last_error()
    assert h.vpd_op_conv2d_bnsums2(p, p, p, p, p, p, p, p, 4, 18, 18, 128, 16, 16, 128, 128, None, None) != 0


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_fused_tail_entry_points_are_declared_bound_and_exported(dtype):
    """vpd_op_conv1x1_bn, vpd_op_conv1x1_bn2 and the host-only vpd_op_conv1x1_bn_dispatch: test-only additions under ABI 5 (their
    refusals: tests/test_bneck_tail_cpu.py)"""
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    assert h.vpd_abi_version() == _lib.ABI_VERSION == 5
    for n, nargs in (("vpd_op_conv1x1_bn", 28), ("vpd_op_conv1x1_bn2", 41), ("vpd_op_conv1x1_bn_dispatch", 7)):
        assert n in header_functions() and len(_lib.SIGNATURES[n][1]) == nargs and getattr(h, n).argtypes == _lib.SIGNATURES[n][1]
    out = (C.c_int * 5)()
    assert h.vpd_op_conv1x1_bn_dispatch(256, 32, 32, 64, 256, 1, out) == 0 and out[0] == 1 and out[4] == 5


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_weight_gradient_route_entry_points_are_declared_bound_and_exported(dtype):
    """vpd_op_wgrad_dispatch, vpd_op_wgrad_group, vpd_op_wgrad_group_slab_floats and vpd_op_wgrad_group_dispatch: test-only additions
    under ABI 5 (their answers and refusals: tests/test_wgrad_routes_cpu.py)"""
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    assert h.vpd_abi_version() == _lib.ABI_VERSION == 5
    for n, nargs in (("vpd_op_wgrad_dispatch", 17), ("vpd_op_wgrad_group", 7), ("vpd_op_wgrad_group_slab_floats", 2),
                     ("vpd_op_wgrad_group_dispatch", 3)):
        assert n in header_functions() and len(_lib.SIGNATURES[n][1]) == nargs and getattr(h, n).argtypes == _lib.SIGNATURES[n][1]
    out = (C.c_int * 9)()
    assert h.vpd_op_wgrad_dispatch(3, 18, 18, 64, 1, 18, 18, 64, 16, 16, 1, 64, 64, (C.c_int * 9)(3, 3, 0, 1, 0, 1, 0, 3, 1), 1, 0, out) == 0
    assert list(out) == [2, 4, 3, 4, 0, 108, 12, 1, 1]      # halo 3x3, four passes, three stages, TR 4, 108 halo pixels, 12 splits of one
    assert h.vpd_op_wgrad_group_slab_floats(64, 64) == 64 * 9 * 64 * 64 and h.vpd_op_wgrad_group_slab_floats(512, 512) == 0


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_boundary_entry_points_are_bound_and_reject_bad_arguments(dtype):
    """vpd_op_pack_input, vpd_op_pack_weights, vpd_op_unpack_grads, vpd_op_adamw_pack, vpd_op_wgrad_reduce, vpd_op_zero_ranges:
    test-only additions under ABI 5; every refusal is taken on the host, with a message, before anything is launched"""
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    assert h.vpd_abi_version() == _lib.ABI_VERSION == 5
    for n, nargs in (("vpd_op_pack_input", 10), ("vpd_op_pack_weights", 8), ("vpd_op_unpack_grads", 8), ("vpd_op_adamw_pack", 18),
                     ("vpd_op_wgrad_reduce", 6), ("vpd_op_zero_ranges", 4)):
        assert n in header_functions() and len(_lib.SIGNATURES[n][1]) == nargs and getattr(h, n).argtypes == _lib.SIGNATURES[n][1]
    p = C.c_void_p(64)                                    # never dereferenced: every call below is rejected on the host
    odd = C.c_void_p(72)                                  # 8-byte aligned only

    def refused(rc, msg):
        return rc != 0 and msg in h.vpd_last_error()
    # pack_input
    assert refused(h.vpd_op_pack_input(None, 2, 5, 4, 8, p, 10, 16, 3, None), b"null argument")
    assert refused(h.vpd_op_pack_input(p, 2, 5, 4, 8, None, 10, 16, 3, None), b"null argument")
    assert refused(h.vpd_op_pack_input(p, 2, 9, 4, 8, p, 10, 16, 3, None), b"c outside 1..8")
    assert refused(h.vpd_op_pack_input(p, 2, 0, 4, 8, p, 10, 16, 3, None), b"c outside 1..8")
    for bad in ((0, 4, 8, 10, 16, 3), (2, 0, 8, 10, 16, 3), (2, 4, 0, 10, 16, 3), (2, 4, 8, 6, 16, 3), (2, 4, 8, 10, 10, 3),
                (2, 4, 8, 10, 16, -1), (70000, 200, 200, 206, 208, 3)):
        n, H, W, Hp, Wp, pad = bad
        assert refused(h.vpd_op_pack_input(p, n, 5, H, W, p, Hp, Wp, pad, None), b"bad shape"), bad
    assert refused(h.vpd_op_pack_input(C.c_void_p(66), 2, 5, 4, 8, p, 10, 16, 3, None), b"aligned")
    assert refused(h.vpd_op_pack_input(p, 2, 5, 4, 8, odd, 10, 16, 3, None), b"aligned")
    # pack_weights / unpack_grads
    assert refused(h.vpd_op_pack_weights(None, 32, 32, 3, 0, p, p, None), b"null argument")
    assert refused(h.vpd_op_pack_weights(p, 32, 32, 3, 0, None, p, None), b"null argument")
    for Co, Ci, k, stem, msg in ((48, 32, 3, 0, b"multiples of 32"), (32, 16, 3, 0, b"multiples of 32"), (32, 32, 4, 0, b"k must be"),
                                 (32, 32, 0, 0, b"k must be"), (64, 9, 7, 1, b"the stem is"), (64, 5, 3, 1, b"the stem is"),
                                 (64, 5, 7, 2, b"stem is 0 or 1")):
        assert refused(h.vpd_op_pack_weights(p, Co, Ci, k, stem, p, None, None), msg), (Co, Ci, k, stem)
        assert refused(h.vpd_op_unpack_grads(p, Co, Ci, k, 64, stem, p, None), msg), (Co, Ci, k, stem)
    assert refused(h.vpd_op_pack_weights(p, 64, 5, 7, 1, p, p, None), b"no data-gradient layout")
    assert refused(h.vpd_op_pack_weights(p, 32, 32, 3, 0, odd, None, None), b"aligned")
    assert refused(h.vpd_op_pack_weights(p, 32, 32, 3, 0, p, odd, None), b"aligned")
    assert refused(h.vpd_op_unpack_grads(None, 32, 32, 3, 32, 0, p, None), b"null argument")
    assert refused(h.vpd_op_unpack_grads(p, 32, 32, 3, 32, 0, None, None), b"null argument")
    assert refused(h.vpd_op_unpack_grads(p, 32, 64, 3, 32, 0, p, None), b"Kc is too small")
    assert refused(h.vpd_op_unpack_grads(p, 64, 5, 7, 48, 1, p, None), b"Kc is too small")
    # adamw_pack
    dims = (C.c_int * 6)(32, 32, 3, 64, 32, 1)
    offs = (C.c_longlong * 2)(100, 100 + 9216 + 8)
    numel = 100 + 9216 + 8 + 2048 + 4
    hyp = (5e-4, 0.9, 0.999, 1e-8, 0.01)

    def adam(nconv=2, dims=dims, offs=offs, numel=numel, ptrs=(p, p, p, p, p, None), step=1):
        return h.vpd_op_adamw_pack(nconv, dims, offs, numel, *ptrs, *hyp, step, 1.0, None)
    for i in range(5):
        ptrs = [p, p, p, p, p, None]
        ptrs[i] = None
        assert refused(adam(ptrs=ptrs), b"null argument"), i
    assert refused(adam(dims=None), b"null argument") and refused(adam(offs=None), b"null argument")
    assert refused(adam(nconv=-1), b"nconv outside") and refused(adam(nconv=65), b"nconv outside")
    assert refused(adam(numel=numel + 2), b"multiple of 4") and refused(adam(numel=0), b"multiple of 4")
    assert refused(adam(step=0), b"1-based")
    assert refused(adam(ptrs=(p, p, p, p, odd, None)), b"16-byte aligned") and refused(adam(ptrs=(p, p, p, p, p, odd)), b"16-byte aligned")
    assert refused(adam(dims=(C.c_int * 6)(32, 32, 3, 64, 48, 1)), b"multiples of 32")
    assert refused(adam(offs=(C.c_longlong * 2)(102, 9400)), b"multiple of 4 floats")
    assert refused(adam(offs=(C.c_longlong * 2)(100, 9000)), b"ascend")                 # overlap
    assert refused(adam(offs=(C.c_longlong * 2)(9400, 100)), b"ascend")
    assert refused(adam(numel=10000), b"ascend")                                      # the last conv ends behind numel
    # wgrad_reduce
    pp = (C.c_void_p * 2)(64, 128)
    nf = (C.c_longlong * 2)(400, 4096)
    ks = (C.c_int * 2)(3, 1)
    assert refused(h.vpd_op_wgrad_reduce(2, None, pp, nf, ks, None), b"null argument")
    assert refused(h.vpd_op_wgrad_reduce(2, pp, None, nf, ks, None), b"null argument")
    assert refused(h.vpd_op_wgrad_reduce(2, pp, pp, None, ks, None), b"null argument")
    assert refused(h.vpd_op_wgrad_reduce(2, pp, pp, nf, None, None), b"null argument")
    assert refused(h.vpd_op_wgrad_reduce(2, (C.c_void_p * 2)(64, None), pp, nf, ks, None), b"null argument")
    assert refused(h.vpd_op_wgrad_reduce(0, pp, pp, nf, ks, None), b"nprob outside") and refused(h.vpd_op_wgrad_reduce(19, pp, pp, nf, ks, None), b"nprob outside")
    assert refused(h.vpd_op_wgrad_reduce(2, pp, pp, (C.c_longlong * 2)(402, 4096), ks, None), b"multiple of 4")
    assert refused(h.vpd_op_wgrad_reduce(2, pp, pp, (C.c_longlong * 2)(400, 0), ks, None), b"multiple of 4")
    assert refused(h.vpd_op_wgrad_reduce(2, pp, pp, nf, (C.c_int * 2)(3, 0), None), b"ksplit >= 1")
    assert refused(h.vpd_op_wgrad_reduce(2, (C.c_void_p * 2)(64, 72), pp, nf, ks, None), b"16-byte aligned")
    # zero_ranges
    assert h.vpd_op_zero_ranges(None, None, 0, None) == 0                             # count 0: nothing to do, nothing looked at
    assert refused(h.vpd_op_zero_ranges(pp, nf, -1, None), b"count outside") and refused(h.vpd_op_zero_ranges(pp, nf, 17, None), b"count outside")
    assert refused(h.vpd_op_zero_ranges(None, nf, 2, None), b"null argument") and refused(h.vpd_op_zero_ranges(pp, None, 2, None), b"null argument")
    assert refused(h.vpd_op_zero_ranges((C.c_void_p * 2)(64, None), nf, 2, None), b"null argument")
    assert refused(h.vpd_op_zero_ranges((C.c_void_p * 2)(64, 72), nf, 2, None), b"16-byte aligned")
    assert refused(h.vpd_op_zero_ranges(pp, (C.c_longlong * 2)(4, -1), 2, None), b"not negative")
    # the public flat AdamW refuses a length that is no multiple of 4
    assert refused(h.vpd_adamw_step(p, p, p, p, 4102, *hyp, 1, None), b"multiple of 4")
    assert refused(h.vpd_adamw_step_scaled(p, p, p, p, 4102, *hyp, p, None), b"multiple of 4")


ARCHS = ("resnet18", "resnet34", "resnet50", "resnet101", "wide_resnet50_2", "wide_resnet101_2")


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("c_in", [3, 5])
def test_every_conv_tensor_of_a_plan_starts_at_a_multiple_of_four_floats(arch, c_in):
    """adamw_pack_kernel reads and writes a conv's OIHW rows 16 bytes at a time and -- unlike pack_weights_kernel -- has no
    unaligned fallback: every 4-dimensional tensor of every architecture the plan accepts lies at a multiple of 4 floats"""
    from vpd_amd._lib import check, lib
    L = lib()
    h = C.c_void_p()
    check(L.vpd_plan_create(arch.encode(), c_in, 128, 128, 128, 1, 4, 1, C.byref(h)), "create")
    kind, dec, off, numel, ndim = C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong(), C.c_int()
    dims = (C.c_int * 4)()
    convs = 0
    for i in range(L.vpd_plan_num_tensors(h)):
        check(L.vpd_plan_tensor_info(h, i, C.byref(kind), C.byref(dec), C.byref(off), C.byref(numel), C.byref(ndim), dims), "info")
        if ndim.value == 4:
            assert kind.value == 0 and off.value % 4 == 0, (i, off.value)
            assert numel.value == dims[0] * dims[1] * dims[2] * dims[3]
            convs += 1
    assert convs >= 20 and L.vpd_plan_param_numel(h) % 4 == 0
    L.vpd_plan_destroy(h)


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vpd_amd.engine import StudentEngine
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StudentEngine("resnet18", 5, 32)


def test_product_does_not_import_oracle():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-c",
                          "import sys; import vpd_amd, vpd_amd.engine, vpd_amd.trainer, vpd_amd.models.rgb, vpd_amd.ddp;"
                          "print(any(m.startswith('oracle') for m in sys.modules))"],
                         cwd=REPO, capture_output=True, text=True)
    assert out.stdout.strip() == "False", out.stdout + out.stderr


def test_library_shares_torchs_hip_runtime():
    """Loading the library before anything imports torch must still leave ONE HIP runtime in the process: a second copy (the
    system ROCm's next to torch's) sees no device, and the library's first GPU call fails."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-c",
                          "from vpd_amd import _lib; _lib.lib(); import torch;"
                          "print(len({l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}))"],
                         cwd=REPO, capture_output=True, text=True)
    assert out.stdout.strip() == "1", out.stdout + out.stderr
