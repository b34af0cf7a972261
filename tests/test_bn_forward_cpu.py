"""What tests/test_bn_forward_ops_gpu.py rests on, without a GPU: the float64 closed forms of tests/opref_bn_fwd.py equal
F.batch_norm(training=True); a float32 transcription of the kernels' arithmetic stays inside the derived bounds on every launch of
the GPU file; each of a list of planted faults reads outside them; every case takes the path its id names; the float-reciprocal
division is exact for the new shapes' divisors; the XCD block map is a permutation."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import opref as R
from tests import opref_bn_fwd as B

NAMES = ["bf16", "fp16"]
VEC = ("mean", "rstd", "scale", "shift", "rm", "rv")


@functools.lru_cache(maxsize=None)
def _small(cid, name, relu=1, residual=0, second=0):
    assert cid not in B.LARGE
    return B.case(cid, name, bool(relu), bool(residual), bool(second))


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(B.CASES))
def test_closed_forms_equal_torch_batch_norm_in_float64(cid):
    cs = B.case(cid, "bf16", residual=cid in B.PLANTED)
    M, ref = cs["M"], cs["ref"]
    zd = cs["z"].double()
    if M == 1:      # torch refuses a single value per channel: the formula itself
        # (the uneven rows hold +K and -K: their fp64 total is the single value to 1e-15, not to the bit)
        assert torch.allclose(ref["mean"], zd[0], rtol=1e-14, atol=1e-15) and float(ref["var"].abs().max()) <= 1e-14
        assert torch.allclose(ref["rstd"], torch.full_like(ref["rstd"], B.EPS ** -0.5), rtol=1e-8)
        assert torch.allclose(ref["rv"], (1 - B.MOM) * cs["rv"].double(), rtol=1e-12, atol=1e-14)
        assert torch.allclose(cs["out"], (cs["beta"].double().view(1, -1)).clamp_min(0), rtol=1e-12, atol=1e-12)
        return
    rm, rv = cs["rm"].double().clone(), cs["rv"].double().clone()
    y = F.batch_norm(zd, rm, rv, cs["gamma"].double(), cs["beta"].double(), training=True, momentum=B.MOM, eps=B.EPS)
    if cs["res"] is not None:
        y = y + cs["res"].double().view(M, -1)
    y = y.clamp_min(0)
    # (E[z^2] - mu^2 against torch's two-pass variance: the planted mean-40 channel loses 1600 / 0.0156 = 1e5 of fp64's 1e-16)
    scale = float((y.abs().max()))
    assert float((cs["out"] - y).abs().max()) <= 1e-12 * max(scale, 1.0) * (1e2 if cs["planted"] else 1.0)
    keep = torch.ones_like(rm, dtype=torch.bool)
    if cs["planted"]:
        keep[B.CH_CANCEL] = False
        assert torch.allclose(ref["rv"][B.CH_CANCEL], rv[B.CH_CANCEL], rtol=1e-9)
    assert torch.allclose(ref["rm"], rm, rtol=1e-12, atol=1e-14) and torch.allclose(ref["rv"][keep], rv[keep], rtol=1e-12, atol=1e-14)
    assert torch.allclose(ref["mean"], zd.mean(0), rtol=1e-12, atol=1e-14)
    assert torch.allclose(ref["rstd"][keep], (zd.var(0, unbiased=False) + B.EPS).rsqrt()[keep], rtol=1e-12)


def test_rows_are_uneven_and_no_subset_of_them_gives_the_sums():
    cs = _small("one_trip_3x9x7", "bf16")
    for rows in (cs["rows"], cs["rows16"]):
        tot = rows.sum(0)
        assert torch.allclose(tot[0], cs["S1"], rtol=1e-12, atol=1e-9) and torch.allclose(tot[1], cs["S2"], rtol=1e-12)
        for t in range(rows.shape[0]):
            part = tot - rows[t]
            assert bool(((part[1] - tot[1]).abs() > 0.01 * tot[1].abs()).all()), t
    assert not torch.allclose(cs["rows16"][:4].sum(0)[1], cs["S2"], rtol=0.5)      # four of the sixteen rows are not the sums either


# ---- the transcription stays inside the bounds ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("launch", B.LAUNCHES, ids=B.launch_id)
def test_float32_transcription_is_within_the_bounds(launch, name):
    cid, relu, residual, second = launch
    cs = B.case(cid, name, bool(relu), bool(residual), bool(second))
    M = cs["M"]
    worst = {}
    sides = [cs] + ([cs["b2"]] if second else [])
    coef = {}
    for flavour in (("fused", -1, False), ("fused", 0, False), ("fused", 1, False), ("finalize", 0, False), ("finalize", 0, True)):
        kind, ulps, contract = flavour
        for si, s in enumerate(sides):
            rows = s["rows"] if kind == "fused" else s["rows16"]
            t = B.transcribe_vectors(rows, M, s["gamma"], s["beta"], s["rm"], s["rv"], kind, ulps, contract)
            bnd = B.vector_bounds(s["ref"], rows, M, s["gamma"], s["beta"], s["rm"], s["rv"], kind)
            for k in VEC:
                key = "%s/%s" % (kind, k)
                worst[key] = max(worst.get(key, 0.0), B.ratio(torch.from_numpy(t[k]), s["ref"][k], bnd[k]))
            coef[(flavour, si)] = (t["scale"], t["shift"])
    bound = B.case_out_bound(cs)
    res = cs["res"].view(M, -1) if residual else None
    # the apply, with and without contraction, on the coefficient sets furthest apart
    for flavour, contract in ((("fused", -1, False), False), (("fused", 1, False), True), (("finalize", 0, False), False)):
        sc, sh = coef[(flavour, 0)]
        sec = (cs["b2"]["z"],) + coef[(flavour, 1)] if second else None
        got = B.transcribe_apply(cs["z"], sc, sh, relu, name, res, sec, contract)
        worst["out"] = max(worst.get("out", 0.0), B.ratio(got, cs["out"], bound))
        del got
    print(B.launch_id(launch), name, " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("cid", ["one_trip_3x9x7", "generic_cv_3"])
@pytest.mark.parametrize("res_kind", [0, 1, 2])
def test_apply_from_given_coefficients_is_within_its_bound(res_kind, cid, name):
    cs = _small(cid, name, 1, int(res_kind == 1), int(res_kind == 2))
    M = cs["M"]
    f32 = lambda t: t.float()
    sc, sh = f32(cs["ref"]["scale"]), f32(cs["ref"]["shift"])
    res = cs["res"].view(M, -1) if res_kind == 1 else None
    sec = (cs["b2"]["z"], f32(cs["b2"]["ref"]["scale"]), f32(cs["b2"]["ref"]["shift"])) if res_kind == 2 else None
    ref, _ = B.apply_ref(cs["z"], sc, sh, 1, res, sec)
    bound = B.apply_bound(ref, name, cs["z"], sc, sh, res, sec)
    for contract in (False, True):
        got = B.transcribe_apply(cs["z"], sc.numpy(), sh.numpy(), 1, name, res, (sec[0], sec[1].numpy(), sec[2].numpy()) if sec else None, contract)
        assert B.ratio(got, ref, bound) <= 1.0
    # resolution: the coefficients of the channel next door are outside
    off, _ = B.apply_ref(cs["z"], sc.roll(-1), sh.roll(-1), 1, res, sec)
    assert B.ratio(off, ref, bound) > 1.0


# ---- the bounds resolve faults ---------------------------------------------------------------------------------------------------
def _vector_ratio(cs, alt, kind="fused", keys=VEC):
    rows = cs["rows"] if kind == "fused" else cs["rows16"]
    bnd = B.vector_bounds(cs["ref"], rows, cs["M"], cs["gamma"], cs["beta"], cs["rm"], cs["rv"], kind)
    return max(B.ratio(alt[k], cs["ref"][k], bnd[k]) for k in keys)


@pytest.mark.parametrize("name", NAMES)
def test_bounds_resolve_the_planted_faults(name):
    cs = _small("one_trip_3x9x7", name, 1, 1, 0)
    M, (n, h, w, c) = cs["M"], cs["shape"]
    ref = cs["ref"]
    bound = B.case_out_bound(cs)
    res = cs["res"].view(M, c)
    reads = {}

    def out_of(alt):
        return B.apply_ref(cs["z"], alt["scale"], alt["shift"], 1, res)[0]

    # the biased variance in rv'
    alt = dict(ref, rv=(1 - B.MOM) * cs["rv"].double() + B.MOM * ref["var"])
    reads["biased variance"] = _vector_ratio(cs, alt, keys=("rv",))
    assert _vector_ratio(cs, alt, "finalize", keys=("rv",)) > 1.0
    # one accumulator row dropped
    for t in range(B.FUSED_ROWS):
        S1, S2 = B.row_sums(torch.cat([cs["rows"][:t], cs["rows"][t + 1:]]))
        alt = B.closed_form(S1, S2, M, cs["gamma"], cs["beta"], cs["rm"], cs["rv"])
        reads["row %d dropped" % t] = min(_vector_ratio(cs, alt, keys=("rstd",)), B.ratio(out_of(alt), cs["out"], bound))
    # count off by one image
    alt = B.closed_form(cs["S1"], cs["S2"], M - h * w, cs["gamma"], cs["beta"], cs["rm"], cs["rv"])
    reads["count off by one image"] = min(_vector_ratio(cs, alt, keys=("mean",)), B.ratio(out_of(alt), cs["out"], bound))
    # shift = beta + mu * scale
    alt = dict(ref, shift=cs["beta"].double() + ref["mean"] * ref["scale"])
    reads["shift sign"] = min(_vector_ratio(cs, alt, keys=("shift",)), B.ratio(out_of(alt), cs["out"], bound))
    # statistics of channel c + 1
    alt = B.closed_form(cs["S1"].roll(-1), cs["S2"].roll(-1), M, cs["gamma"], cs["beta"], cs["rm"], cs["rv"])
    reads["channel c + 1"] = min(_vector_ratio(cs, alt, keys=("mean",)), B.ratio(out_of(alt), cs["out"], bound))
    # the residual read without its border offset: the padded tensor's (y, x) in (y + 1, x + 1)'s place
    padded = torch.zeros(n, h + 2, w + 2, c)
    padded[:, 1:-1, 1:-1] = cs["res"]
    shifted = padded[:, :h, :w].reshape(M, c)
    reads["residual without its offset"] = B.ratio(B.apply_ref(cs["z"], ref["scale"], ref["shift"], 1, shifted)[0], cs["out"], bound)
    # the second BatchNorm's coefficients applied to the first
    two = _small("one_trip_3x9x7", name, 1, 0, 1)
    b2 = two["b2"]
    swapped, _ = B.apply_ref(two["z"], b2["ref"]["scale"], b2["ref"]["shift"], 1, None, (b2["z"], two["ref"]["scale"], two["ref"]["shift"]))
    reads["coefficients swapped"] = B.ratio(swapped, two["out"], B.case_out_bound(two))
    print(name, " ".join("%s: %.3g;" % kv for kv in reads.items()))
    assert all(v > 1.0 for v in reads.values()), reads


def test_bit_map_is_of_the_stored_value_not_of_the_value_before_rounding():
    """gamma = 0, beta = +1e-9 under the ReLU: fp16 stores +0 (bit 0), bf16 stores 1e-9 (bit 1); a map taken before the store differs
    from the stored one in the fp16 build, in that channel and nowhere else in it"""
    got = {}
    for name in NAMES:
        cs = _small("one_trip_3x9x7", name)
        stored, before = B.stored_mask(cs["out"], name), cs["pre"] > 0
        got[name] = (stored[:, B.CH_FLUSH], before[:, B.CH_FLUSH])
        assert bool(before[:, B.CH_FLUSH].all())
    assert bool(got["bf16"][0].all()) and not bool(got["fp16"][0].any())
    assert not torch.equal(R.mask_bits(got["fp16"][0].view(-1, 1).expand(-1, 8).contiguous()),
                           R.mask_bits(got["fp16"][1].view(-1, 1).expand(-1, 8).contiguous()))
    # relu = 0, beta = -1e-9: fp16 stores -0, which is not > 0; bf16 stores a negative value
    for name in NAMES:
        cs = _small("one_trip_3x9x7", name, 0)
        st = R.elem_round(cs["out"][:, B.CH_FLUSH].float(), name)
        assert not bool((st > 0).any())
        assert bool((st == 0).all()) == (name == "fp16")
        if name == "fp16":
            assert bool(torch.signbit(st).all())


# ---- declared paths --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(B.CASES))
def test_every_case_takes_the_path_its_id_names(cid):
    (n, h, w, c), want = B.CASES[cid]
    M = n * h * w
    geo = B.fused_geometry(M, c)
    for k, v in want.items():
        assert geo[k] == v, (k, geo)
    assert geo["lds_bytes"] <= 65536 and c <= 4096
    if geo["fast"]:      # the cached coefficients: a thread keeps its channel slice
        assert geo["stride"] % (c // 8) == 0
    if geo["trips"] > 1:
        assert geo["items"] % geo["stride"] != 0                                       # a ragged last trip
    if cid == "generic_cv_12":
        assert geo["stride"] % (c // 8) != 0                                           # the channel slice changes per item
    if cid == "fast_at_the_limit":
        assert M < B.FDIV_MAX <= M + h * w * 4 and (h * w) & (h * w - 1)
    if cid == "generic_m":
        assert M >= B.FDIV_MAX
        ag = B.apply_geometry(M, c)
        assert ag["capped"] and ag["grid"] == 4096 and ag["trips"] == 3
    if cid == "three_trips_capped":
        assert geo["items"] == 557056 and c > 64
    assert B.apply_geometry(M, c)["items"] == geo["items"]


def test_item_decode_of_both_paths_agrees_with_integer_division():
    """the fast path's shift / mask / vpd_fdiv decode of every item of the fast cases equals the generic path's divisions"""
    for cid in ("three_trips_capped", "fast_at_the_limit", "one_trip_3x9x7"):
        (n, h, w, c), _ = B.CASES[cid]
        cv, M = c // 8, n * h * w
        m = np.arange(M, dtype=np.int64)
        b = B.fdiv(m, h * w)
        assert np.array_equal(b, m // (h * w)), cid
        r = m - b * (h * w)
        assert np.array_equal(B.fdiv(r, w), r // w), cid
        it = np.arange(0, M * cv, 977, dtype=np.int64)
        assert np.array_equal(it >> (cv.bit_length() - 1), it // cv) and np.array_equal(it & (cv - 1), it % cv)


def test_float_reciprocal_division_is_exact_for_the_new_divisors():
    divs = set()
    for (n, h, w, c), _ in B.CASES.values():
        divs |= {h * w, w}
    assert {23, 529, 61, 3721} <= divs
    m = np.arange(2 ** 21, dtype=np.int64)
    for d in sorted(divs):
        assert np.array_equal(B.fdiv(m, d), m // d), d


# ---- the XCD block map -----------------------------------------------------------------------------------------------------------
def test_virtual_block_is_a_permutation():
    for r in (1, 2, 4, 8, 16, 32):
        v = [B.virtual_block(b, 256, r) for b in range(256)]
        assert sorted(v) == list(range(256)), r
        assert (v == list(range(256))) == (r == 1), r
        # the R virtual blocks of a tile run on physical blocks of one XCD (b % 8)
        by_tile = {}
        for b, vb in enumerate(v):
            by_tile.setdefault(vb // r, set()).add(b & 7)
        assert all(len(s) == 1 for s in by_tile.values()), r
    for grid in (1, 8, 255, 257):
        assert [B.virtual_block(b, grid, 4) for b in range(grid)] == list(range(grid))
    assert [B.virtual_block(b, 256, 0) for b in range(256)] == list(range(256))
    assert B.xcd_r(128, 64, 256) == 1 and B.xcd_r(256, 128, 256) == 4 and B.xcd_r(256, 128, 255) == 0
    assert B.xcd_r(0, 128, 256) == 0 and B.xcd_r(96, 128, 256) == 0 and B.xcd_r(256, 24, 256) == 0


# ---- the entry points' refusals are taken on the host ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", NAMES)
def test_entry_points_refuse_bad_shapes_on_the_host(dtype):
    """vpd_op_bn_apply (a test-only addition under ABI 5) is declared, bound and exported; it, vpd_op_bn_forward and vpd_op_bn_forward2
    refuse n, H, W < 1, C < 8, C % 8 != 0 and C > 4096 with a message before anything is launched (no GPU is needed to be refused)"""
    import ctypes as C
    from tests.test_abi_cpu import header_functions
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    assert h.vpd_abi_version() == _lib.ABI_VERSION == 5
    assert "vpd_op_bn_apply" in header_functions() and len(_lib.SIGNATURES["vpd_op_bn_apply"][1]) == 14
    assert h.vpd_op_bn_apply.argtypes == _lib.SIGNATURES["vpd_op_bn_apply"][1]
    p = C.c_void_p(64)                                    # never dereferenced: every call below is rejected on the host
    f = C.c_float(0.1)
    for bad in ((0, 4, 4, 64), (2, 0, 4, 64), (2, 4, 0, 64), (2, 4, 4, 0), (2, 4, 4, 4), (2, 4, 4, 100), (2, 4, 4, 4104), (-3, 4, 4, 64)):
        assert h.vpd_op_bn_forward(*[p] * 13, *bad, 1, f, f, None) != 0 and b"bad shape" in h.vpd_last_error(), bad
        assert h.vpd_op_bn_forward2(*[p] * 22, *bad, 1, f, f, None) != 0 and b"bad shape" in h.vpd_last_error(), bad
        for kind in (0, 1, 2):
            assert h.vpd_op_bn_apply(*[p] * 6, kind, p, *bad, 1, None) != 0 and b"bad shape" in h.vpd_last_error(), bad
    assert h.vpd_op_bn_apply(*[p] * 6, 2, p, 70000, 200, 200, 8, 1, None) != 0 and b"bad shape" in h.vpd_last_error()      # 2^31 pixels and more
    for i in (0, 1, 2, 7):
        args = [p] * 6 + [0, p]
        args[i] = None
        assert h.vpd_op_bn_apply(*args, 2, 4, 4, 64, 1, None) != 0 and b"null argument" in h.vpd_last_error(), i
    assert h.vpd_op_bn_apply(p, p, p, None, p, p, 1, p, 2, 4, 4, 64, 1, None) != 0 and b"null argument" in h.vpd_last_error()
    assert h.vpd_op_bn_apply(p, p, p, p, None, p, 2, p, 2, 4, 4, 64, 1, None) != 0 and b"null argument" in h.vpd_last_error()
    assert h.vpd_op_bn_apply(p, p, p, p, p, None, 2, p, 2, 4, 4, 64, 1, None) != 0 and b"null argument" in h.vpd_last_error()
    for kind in (-1, 3):
        assert h.vpd_op_bn_apply(*[p] * 6, kind, p, 2, 4, 4, 64, 1, None) != 0 and b"res_kind" in h.vpd_last_error()
