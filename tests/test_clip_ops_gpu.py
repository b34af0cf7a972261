"""The norm pass and the one-block kernel of the gradient-norm clipping (vpd_op_grad_norm; grad_sqsum_kernel and clip_finalize_kernel
in vpd_amd/csrc/optim.hip) against the float64 reference of tests/opref_clip.py, in both libraries.

Bounds.  Integer elements in [-8, 8]: every square and every partial sum is an integer below 2^53, so the kernel's double sum is exact
whatever its order, and the three stored floats equal the reference's IN BITS.  randn: the double sums differ by at most n * 2^-53
relative, far below half a float32 ulp, so each stored float is within 1 ulp of the reference's.  inf / NaN are VALUES planted in
data."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import opref_clip as R

pytestmark = pytest.mark.gpu

FR_MAX = 96
INT_MAX = 2 ** 31 - 1
LENGTHS = [0, 1, 3, 4, 5, 1023, 4099]
BIG = 2048 * 256 * 16 + 7            # past the grid cap x the unrolled tile: both loops wrap


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def L(request):
    from vpd_amd import _lib
    return _lib.lib(request.param)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _new_clip(L, applied=0):
    clip = torch.zeros(L.vpd_clip_state_bytes() // 4, dtype=torch.int32, device="cuda")
    clip[3] = applied
    return clip


def _new_src(scale, found=0, applied=0):
    host = torch.zeros(8, dtype=torch.int32)
    host.view(torch.float32)[0] = scale
    host[1], host[3] = found, applied
    return host.cuda()


def _read(clip):
    h = clip[:16].cpu()
    f = h.view(torch.float32)
    return dict(eff_scale=f[0].numpy().copy(), found=int(h[1]), tracker=int(h[2]), applied=int(h[3]), skipped=int(h[4]),
                total_norm=f[8].numpy().copy(), norm_max=f[9].numpy().copy(), coef=f[10].numpy().copy(), clipped=int(h[11]),
                nonfinite=int(h[12]))


def _run(L, ranges, max_norm, clip, src=None, host_scale=1.0):
    x = (C.c_void_p * max(len(ranges), 1))(*[t.data_ptr() if t.numel() else 64 + 4 * (i % 4) for i, t in enumerate(ranges)])      # (empty: any non-null address)
    n = (C.c_longlong * max(len(ranges), 1))(*[t.numel() for t in ranges])
    assert L.vpd_op_grad_norm(x, n, len(ranges), max_norm, _ptr(src), host_scale, _ptr(clip), _stream()) == 0, L.vpd_last_error()
    return _read(clip)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).item()


def _same_bits(got, ref):
    return (_bits(got["total_norm"]), _bits(got["coef"]), _bits(got["eff_scale"])) == \
        (_bits(ref["total_norm_f32"]), _bits(ref["coef_f32"]), _bits(ref["eff_scale_f32"]))


def _within_one_ulp(got, ref):
    for k, r in (("total_norm", "total_norm_f32"), ("coef", "coef_f32"), ("eff_scale", "eff_scale_f32")):
        assert abs(float(got[k]) - float(ref[r])) <= R.ulp32(float(ref[r])), (k, got[k], ref[r])


def _ints(n, seed, phase=0):
    """n integers in [-8, 8] as float32, starting `phase` floats behind a 16-byte aligned address"""
    g = torch.Generator().manual_seed(seed)
    base = torch.zeros(n + 4, dtype=torch.float32)
    base[phase:phase + n] = torch.randint(-8, 9, (n,), generator=g).float()
    return base.cuda()[phase:phase + n]


# ---- integers: bit equality ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_integer_ranges_every_length_and_phase(L, n):
    for phase in range(4):
        x = _ints(n, 100 + n + phase, phase)
        assert n == 0 or x.data_ptr() % 16 == 4 * phase                     # (an empty tensor has no address)
        xs = [x.cpu().numpy()]
        norm = float(np.sqrt(R.sqsum(xs)))
        for max_norm in (0.5 * norm + 0.25, 2.0 * norm + 1.0):               # binding, not binding
            ref = R.clip_ref(xs, max_norm)
            got = _run(L, [x], max_norm, _new_clip(L))
            assert _same_bits(got, ref), (n, phase, max_norm, got, ref)
            assert got["found"] == 0 and got["nonfinite"] == 0 and got["clipped"] == (1 if ref["coef"] < 1.0 else 0)


@pytest.fixture(scope="module")
def big_ints():
    x = _ints(BIG, 7, 1)
    return x, R.sqsum([x.cpu().numpy()])


def test_integer_range_past_the_grid_cap(L, big_ints):
    x, s = big_ints
    ref = R.clip_ref([x.cpu().numpy()], 1000.0)
    assert ref["sum"] == s and ref["coef"] < 1.0
    got = _run(L, [x], 1000.0, _new_clip(L))
    assert _same_bits(got, ref), (got, ref)


@pytest.mark.parametrize("count", [5, FR_MAX + 3])
def test_integer_ranges_many(L, count):
    """5 ranges: one launch; FR_MAX + 3: a second launch that takes the next block of slots.  Lengths cycle through LENGTHS (empty
    ranges included), phases through 0..3."""
    ranges = [_ints(LENGTHS[i % len(LENGTHS)] + (2100 if i == 2 else 0), 300 + i, i % 4) for i in range(count)]
    xs = [t.cpu().numpy() for t in ranges]
    for scale, from_src in ((1.0, True), (256.0, True), (65536.0, True), (256.0, False)):
        max_norm = 0.5 * R.clip_ref(xs, float("inf"), scale=scale)["norm"]
        ref = R.clip_ref(xs, max_norm, scale=scale)
        assert ref["coef"] < 1.0
        src = _new_src(scale, applied=41) if from_src else None
        clip = _new_clip(L, applied=7)
        got = _run(L, ranges, max_norm, clip, src=src, host_scale=1.0 if from_src else scale)
        assert _same_bits(got, ref), (count, scale, from_src, got, ref)
        assert got["applied"] == (41 if from_src else 7)                   # copied from the source, else left alone
        assert got["found"] == 0 and got["clipped"] == 1
        if from_src:
            assert int(src.cpu()[1]) == 0
    # a range count of zero is legal: norm 0, coefficient 1
    got = _run(L, [], 1.0, _new_clip(L))
    assert float(got["total_norm"]) == 0.0 and float(got["coef"]) == 1.0 and float(got["eff_scale"]) == 1.0


# ---- randn: 1 ulp, and the same bits from launch to launch -------------------------------------------------------------------
def test_randn_within_one_ulp_and_reproducible(L):
    g = torch.Generator(device="cuda").manual_seed(5)
    base = torch.randn(2 ** 21 + 64, generator=g, device="cuda")
    ranges = [base[1:2 ** 21 - 2], base[2 ** 21 + 3:2 ** 21 + 60]] + [base[64 * i + (i % 4):64 * i + 40] for i in range(FR_MAX + 1)]
    xs = [t.cpu().numpy() for t in ranges]
    norm = float(np.sqrt(R.sqsum(xs)))
    for max_norm, scale in ((0.37 * norm, 1.0), (0.37 * norm, 1024.0), (3.0 * norm, 1.0)):
        ref = R.clip_ref(xs, max_norm, scale=scale)
        clip = _new_clip(L)
        a = _run(L, ranges, max_norm, clip, host_scale=scale)
        _within_one_ulp(a, ref)
        b = _run(L, ranges, max_norm, clip, host_scale=scale)
        assert (_bits(a["total_norm"]), _bits(a["coef"]), _bits(a["eff_scale"])) == \
            (_bits(b["total_norm"]), _bits(b["coef"]), _bits(b["eff_scale"]))
        assert b["clipped"] == (2 if ref["coef"] < 1.0 else 0) and _bits(b["norm_max"]) == _bits(b["total_norm"])
    # max_norm = +inf: measure only
    got = _run(L, ranges, float("inf"), _new_clip(L))
    assert float(got["coef"]) == 1.0 and float(got["eff_scale"]) == 1.0 and got["clipped"] == 0
    assert abs(float(got["total_norm"]) - norm) <= R.ulp32(norm)


# ---- non-finite values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_non_finite_value_is_found_and_counted(L, bad):
    n = 4099 + 2048 * 4
    x = _ints(n, 9, 3)                                                      # 1 float of head, 2 of tail
    assert x.data_ptr() % 16 == 12 and (n - 1) % 4 == 2
    for pos in (0, n - 1, n - 2, 4097):                                    # first (the head), last and a tail float, the middle
        keep = float(x[pos])
        x[pos] = bad
        src = _new_src(256.0, applied=3)
        clip = _new_clip(L)
        got = _run(L, [x], 1.0, clip, src=src)
        assert got["found"] == 1 and got["nonfinite"] == 1 and got["clipped"] == 0, (pos, got)
        assert int(src.cpu()[1]) == 1 and float(got["coef"]) == 1.0 and float(got["eff_scale"]) == 256.0
        assert not np.isfinite(float(got["total_norm"])) and float(got["norm_max"]) == 0.0
        got = _run(L, [x], 1.0, clip, host_scale=1.0)                      # without a source: found is the block's own
        assert got["found"] == 1 and got["nonfinite"] == 2 and got["clipped"] == 0
        x[pos] = keep
        got = _run(L, [x], 1.0, clip, host_scale=1.0)
        assert got["found"] == 0 and got["nonfinite"] == 2 and got["clipped"] == 1
    # a word that is set in the source survives a clean range, in the source and in eff
    src = _new_src(256.0, found=1)
    got = _run(L, [x], 1.0, _new_clip(L), src=src)
    assert got["found"] == 1 and got["nonfinite"] == 0 and int(src.cpu()[1]) == 1


def test_large_finite_elements_do_not_overflow(L):
    x = torch.full((1000,), 1e20, dtype=torch.float32, device="cuda")       # squares (1e40) leave fp32's range, not double's
    ref = R.clip_ref([x.cpu().numpy()], 1.0)
    got = _run(L, [x], 1.0, _new_clip(L))
    assert np.isfinite(float(got["total_norm"])) and got["found"] == 0 and got["nonfinite"] == 0
    _within_one_ulp(got, ref)
    assert abs(float(got["total_norm"]) - 1e20 * np.sqrt(1000.0)) <= 4 * R.ulp32(3.1e21)


# ---- the block counts its own steps without a source --------------------------------------------------------------------------
def test_block_counts_its_own_steps(L):
    x = _ints(1023, 1)
    clip = _new_clip(L, applied=5)
    got = _run(L, [x], 1e30, clip)
    assert got["applied"] == 5 and got["found"] == 0
    assert L.vpd_scale_state_update(_ptr(clip), 1.0, 1.0, INT_MAX, _stream()) == 0
    got = _read(clip)
    assert (got["applied"], got["skipped"], got["found"]) == (6, 0, 0) and float(got["eff_scale"]) == 1.0
    x[17] = float("nan")
    got = _run(L, [x], 1e30, clip)
    assert got["found"] == 1 and got["applied"] == 6
    assert L.vpd_scale_state_update(_ptr(clip), 1.0, 1.0, INT_MAX, _stream()) == 0
    got = _read(clip)
    assert (got["applied"], got["skipped"], got["found"]) == (6, 1, 0)      # skipped and counted; found cleared
