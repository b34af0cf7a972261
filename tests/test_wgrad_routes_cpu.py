"""Host side of the 64-wide weight-gradient tests (tests/test_wgrad_routes_gpu.py), without a device:
 * the two dispatch queries, which answer with the launchers' own routing and split code, for every case the GPU tests run;
 * which pass instantiations a plane can reach at all;
 * the refusals of vpd_op_wgrad_group;
 * the resolution of the integer-regime equality: each modelled fault moves the float64 reference by at least 1 somewhere;
 * the margin of the randn bound: fp32 accumulation of the exact products stays inside it at every element."""
import ctypes as C

import pytest
import torch

from tests import opref as R
from tests import wgrad_routes_child as W

DTYPES = ["bf16", "fp16"]


def _lib(dtype):
    from vpd_amd import _lib
    return _lib.lib(dtype)


def _group(h, probs):
    k = len(probs)
    out = (C.c_int * (4 + 3 * k))()
    rc = h.vpd_op_wgrad_group_dispatch(k, (C.c_int * (5 * k))(*[v for p in probs for v in p]), out)
    return rc, tuple(out[:4]), [tuple(out[4 + 3 * i:7 + 3 * i]) for i in range(k)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_dispatch_gives_the_split_tables_the_gpu_runs_name(dtype):
    h = _lib(dtype)
    for gid, (probs, head, per) in R.WG_GROUPS.items():
        rc, got_head, got_per = _group(h, probs)
        assert rc == 0 and got_head == tuple(head) and got_per == [tuple(p) for p in per], (gid, got_head, got_per)
        # what the table must hold for the branches the group is there for
        tasks = sum(ks * tiles for ks, _, tiles in got_per)
        assert tasks == got_head[1] and got_head[2] == (tasks + 7) // 8 * 8 and got_head[0] == got_head[3]
        for (n, hh, ww, co, ci), (ks, cpb, tiles) in zip(probs, got_per):
            nch = (n * hh * ww + 63) // 64
            assert tiles == (co // 64) * (ci // 64) and (ks - 1) * cpb < nch <= ks * cpb
            assert ks * 9 * co * ci <= max(int(h.vpd_op_wgrad_group_slab_floats(co, ci)), 9 * co * ci)      # the slab holds every split
    per = {gid: v[2] for gid, v in R.WG_GROUPS.items()}
    probs = {gid: v[0] for gid, v in R.WG_GROUPS.items()}
    assert R.WG_GROUPS["np5_mixed"][1][1] % 8 != 0                                   # a padded grid: blocks that return early
    assert per["np5_mixed"][1][0] == 1 and 5 * 4 * 4 % 64 != 0                        # direct store into dw, ragged last chunk
    assert per["np5_mixed"][0][0] > 1 and per["np5_mixed"][2][2] == 2                 # slab; two tiles
    n, hh, ww = probs["np4_short_last"][1][:3]
    ks, cpb, _ = per["np4_short_last"][1]
    assert 0 < (n * hh * ww // 64) - (ks - 1) * cpb < cpb                             # short last split
    assert R.WG_GROUPS["np5_one"][1][1:3] == (2, 8)                                   # six idle blocks
    assert R.WG_GROUPS["np5_layer1_x4"][1][1:3] == (56, 56)                           # seven tasks per XCD, no padding
    assert {v[1][0] for v in R.WG_GROUPS.values()} == {4, 5}


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_launch_routes_of_every_gpu_case(dtype):
    h = _lib(dtype)
    fail = []
    for sid, ((n, hh, ww), (tr, ks, cpb)) in R.WG_STEM.items():
        d = R.wg_dispatch(h, W.stem_geometry(n, hh, ww), W.TSTEM, 1)
        fail += R.wg_route_errors(d, sid, kernel="stem", inst=4, stages=3, TR=tr, ksplit=ks, cpb=cpb, grid_x=1)
        nch = n * (hh // 2) * (ww // 2) // 64
        assert (ks - 1) * cpb < nch <= ks * cpb
        fail += R.wg_route_errors(R.wg_dispatch(h, W.stem_geometry(n, hh, ww), W.TSTEM, 0), sid + " without a slab", kernel="atomics")
    assert R.WG_STEM["w32_n130"][1][2] > 1 and 130 * 256 // 64 % R.WG_STEM["w32_n130"][1][2] == 1      # cpb > 1, a last split of one chunk
    for sid, (n, hh, ww) in R.WG_STEM_REFUSED.items():
        fail += R.wg_route_errors(R.wg_dispatch(h, W.stem_geometry(n, hh, ww), W.TSTEM, 1), sid, kernel="atomics", inst=0, TR=0, NHP=0)
    from tests.test_ops_gpu import CONV_CASES
    assert {c[0] for c in CONV_CASES} == set(R.WG_ROUTES_OPS)
    for (name, n, ci, co, hh, ww, k, st, pad) in CONV_CASES:
        geom, taps = W.conv_geometry(n, ci, co, hh, ww, st), (W.T3 if k == 3 else W.T1)
        kern, inst = R.WG_ROUTES_OPS[name]
        fail += R.wg_route_errors(R.wg_dispatch(h, geom, taps, 1), name, kernel=kern, inst=inst)
        fail += R.wg_route_errors(R.wg_dispatch(h, geom, taps, 0), name + " without a slab", kernel="atomics", inst=0)
        if k == 1:      # the wish the plan states for the BasicBlock students' 1x1 convs: the halo route, given a slab
            fail += R.wg_route_errors(R.wg_dispatch(h, geom, taps, 1, 1), name + " preferred", kernel="halo1x1", inst=W.HALO_1X1_INST[name])
            fail += R.wg_route_errors(R.wg_dispatch(h, geom, taps, 0, 1), name + " preferred, no slab", kernel="atomics")
    for name, (kern, inst) in R.WG_ROUTES_CONV.items():
        cs = R.CONV_CASES[name]
        if cs.get("stem"):
            d = R.wg_dispatch(h, W.stem_geometry(cs["n"], cs["h"], cs["w"]), W.TSTEM, 1)
        else:
            d = R.wg_dispatch(h, W.conv_geometry(cs["n"], cs["ci"], cs["co"], cs["h"], cs["w"], cs["stride"]), W.T3, 1)
        fail += R.wg_route_errors(d, name, kernel=kern, inst=inst)
    assert set(R.WG_ROUTES_CONV) == {k for k, v in R.CONV_CASES.items() if v.get("wgrad")}
    from tests.wgrad_pair_child import CASES
    for name, (ci, co, ho, n) in CASES.items():
        geom = W.conv_geometry(n, ci, co, 2 * ho, 2 * ho, 2)
        inst = R.WG_ROUTES_PAIR[name]
        fail += R.wg_route_errors(R.wg_dispatch(h, geom, W.T3, 1), name, kernel="halo3x3", inst=inst, stages=2 if inst == 13 else 3)
        fail += R.wg_route_errors(R.wg_dispatch(h, geom, W.T1, 1, 1), name + " branch", kernel="halo1x1", inst=inst)
    assert not fail, "\n".join(fail)


def test_reachable_pass_instantiations():
    """Every H x W plane with W in 1..64, H in 1..128 (and, at stride 2, its 2H x 2W input): the instantiations the launchers can
    pick.  Stride 1: 4 and 5 only, in the single launch and in the group; stride 2: 10 and 13.  The 3-pass instantiation is dead."""
    h = _lib("bf16")
    single = {1: set(), 2: set()}
    grouped = set()
    nhp = {1: set(), 2: set()}
    for ww in range(1, 65):
        for hh in range(1, 129):
            for st in (1, 2):
                d = R.wg_dispatch(h, W.conv_geometry(2, 64, 64, st * hh, st * ww, st), W.T3, 1)
                if d["kernel"] == "halo3x3":
                    single[st].add((d["inst"], d["stages"]))
                    nhp[st].add(d["NHP"])
                    assert {4: 96, 5: 128, 10: 160, 13: 320}[d["inst"]] < d["NHP"] <= 32 * d["inst"]
                else:
                    assert d["kernel"] == "atomics"
            rc, head, _ = _group(h, [(2, hh, ww, 64, 64)])
            if rc == 0:
                grouped.add(head[0])
                assert head[0] == head[3]
    assert single[1] == {(4, 3), (5, 3)} and grouped == {4, 5}
    assert single[2] == {(10, 3), (13, 2)}
    assert min(nhp[1]) > 96 and max(nhp[1]) <= 160 and min(nhp[2]) > 160 and max(nhp[2]) <= 416


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_entry_refusals(dtype):
    h = _lib(dtype)
    p = C.c_void_p(64)                                    # never dereferenced: every call below is refused before a launch
    arr = lambda k: (C.c_void_p * k)(*([64] * k))
    dims = lambda *v: (C.c_int * len(v))(*v)
    good = dims(3, 16, 16, 64, 64)
    refused = lambda rc, msg: rc != 0 and msg in h.vpd_last_error()
    for pos in range(4):
        args = [arr(1)] * 4
        args[pos] = None
        assert refused(h.vpd_op_wgrad_group(1, *args, good, None), b"null argument"), pos
    assert refused(h.vpd_op_wgrad_group(1, arr(1), arr(1), arr(1), arr(1), None, None), b"null argument")
    assert refused(h.vpd_op_wgrad_group(1, (C.c_void_p * 1)(None), arr(1), arr(1), arr(1), good, None), b"null argument")
    assert refused(h.vpd_op_wgrad_group(1, arr(1), arr(1), (C.c_void_p * 1)(None), arr(1), good, None), b"null argument")
    assert refused(h.vpd_op_wgrad_group(1, arr(1), arr(1), arr(1), (C.c_void_p * 1)(None), good, None), b"null argument")      # two splits need the slab
    assert refused(h.vpd_op_wgrad_group(1, arr(1), arr(1), (C.c_void_p * 1)(72), arr(1), good, None), b"16-byte aligned")
    assert refused(h.vpd_op_wgrad_group(0, arr(1), arr(1), arr(1), arr(1), good, None), b"nprob outside")
    many = dims(*([3, 16, 16, 64, 64] * 19))
    assert refused(h.vpd_op_wgrad_group(19, arr(19), arr(19), arr(19), arr(19), many, None), b"nprob outside")
    for bad, msg in ((dims(3, 16, 16, 96, 64), b"multiples of 64"), (dims(3, 16, 16, 64, 32), b"multiples of 64"),
                     (dims(3, 16, 16, 0, 64), b"multiples of 64"), (dims(0, 16, 16, 64, 64), b"bad argument"),
                     (dims(3, 12, 12, 64, 64), b"halo tiling"), (dims(3, 64, 64, 64, 64), b"halo tiling"), (dims(3, 2, 2, 64, 64), b"halo tiling")):
        assert refused(h.vpd_op_wgrad_group(1, arr(1), arr(1), arr(1), arr(1), bad, None), msg), list(bad)
        assert refused(h.vpd_op_wgrad_group_dispatch(1, bad, (C.c_int * 7)()), msg), list(bad)
    two = dims(3, 16, 16, 64, 64, 3, 32, 32, 64, 64)      # four passes beside five
    assert refused(h.vpd_op_wgrad_group(2, arr(2), arr(2), arr(2), arr(2), two, None), b"same number of halo passes")
    assert refused(h.vpd_op_wgrad_group_dispatch(2, two, (C.c_int * 10)()), b"same number of halo passes")
    assert refused(h.vpd_op_wgrad_group_dispatch(1, good, None), b"null argument")
    out9 = (C.c_int * 9)()
    taps = W.T3
    geom = list(W.conv_geometry(3, 64, 64, 16, 16, 1))
    assert h.vpd_op_wgrad_dispatch(*geom, taps, 1, 0, out9) == 0
    assert refused(h.vpd_op_wgrad_dispatch(*geom, None, 1, 0, out9), b"null argument") and refused(h.vpd_op_wgrad_dispatch(*geom, taps, 1, 0, None), b"null argument")
    for pos, bad in ((0, 0), (11, 96), (12, 32)):
        g2 = list(geom)
        g2[pos] = bad
        assert h.vpd_op_wgrad_dispatch(*g2, taps, 1, 0, out9) != 0, pos


# ---- resolution of the integer-regime equality ----
def _int_problem(n, hh, ww, co, ci, k=3, seed=5):
    g = torch.Generator().manual_seed(seed)
    cs = dict(ci=ci, co=co, k=k, stride=1, h=hh, w=ww)
    x, dz = R.wg_operands(n, ci, co, hh, ww, 1, "int", "bf16", g)
    return cs, x, dz, R.conv_wgrad(x, dz, cs)


def test_every_modelled_fault_moves_the_integer_reference_by_at_least_one():
    moved = lambda a, b: float((a - b).abs().max())
    # (i) the last chunk of a split left out: a slab problem, the direct-store problem's ragged chunk, a short last split
    for gid, pi, split in (("np5_mixed", 0, 2), ("np5_mixed", 1, 0), ("np4_short_last", 1, 4)):
        n, hh, ww, co, ci = R.WG_GROUPS[gid][0][pi]
        ks, cpb, _ = R.WG_GROUPS[gid][2][pi]
        cs, x, dz, ref = _int_problem(n, hh, ww, co, ci)
        alt = R.wg_alter_last_chunk(ref, x, dz, cs, ks, cpb, split)
        assert moved(alt, ref) >= 1 and float((alt - ref).abs().max()) == round(moved(alt, ref)), (gid, pi)
        assert int((alt != ref).sum()) > ref.numel() // 2, (gid, pi)
    # (ii) one tap left out for one chunk, every tap in turn; the stem: one kernel row
    cs, x, dz, ref = _int_problem(3, 16, 16, 64, 64)
    for r in range(3):
        for t in range(3):
            alt = R.wg_alter_tap(ref, x, dz, cs, chunk=5, tap=(r, t))
            assert moved(alt, ref) >= 1 and bool((alt[:, :, r, t] != ref[:, :, r, t]).any())
            keep = torch.ones(3, 3, dtype=torch.bool)
            keep[r, t] = False
            assert torch.equal(alt[:, :, keep], ref[:, :, keep])
    g = torch.Generator().manual_seed(9)
    cs7 = dict(ci=5, co=64, k=7, stride=2, h=32, w=32)
    x7, dz7 = R.wg_operands(3, 5, 64, 32, 32, 2, "int", "bf16", g)
    ref7 = R.conv_wgrad(x7, dz7, cs7)
    for r in range(7):
        assert moved(R.wg_alter_tap(ref7, x7, dz7, cs7, chunk=2, tap=(r, 3)), ref7) >= 1
    # (iii) two problems' gradients exchanged (the four equal problems of a group draw different operands)
    refs = [_int_problem(7, 32, 32, 64, 64, seed=20 + i)[3] for i in range(2)]
    assert moved(refs[0], refs[1]) >= 1 and int((refs[0] != refs[1]).sum()) > refs[0].numel() // 2
    # (iv) [Co][Ci] stored as [Ci][Co]: the swapped-operand problems of WG128_GROUPS
    for (n, hh, ww, co, ci) in ((3, 32, 32, 64, 256), (5, 8, 8, 64, 128)):
        cs, x, dz, ref = _int_problem(n, hh, ww, co, ci, k=1)
        alt = R.wg_alter_transposed(ref)
        assert alt.shape == ref.shape and moved(alt, ref) >= 1 and int((alt != ref).sum()) > ref.numel() // 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp32_accumulation_stays_inside_the_randn_bound_at_every_element(dtype):
    """The float64 reference perturbed the way the kernels perturb it -- exact products, an fp32 running sum chunk by chunk -- lies
    within opref.wg_bound everywhere (no element left out), with room: the bound allows truncating adders (opref.CONV_ACC_C)."""
    g = torch.Generator().manual_seed(3)
    for (n, ci, co, hh, ww, k, st) in ((3, 64, 64, 16, 16, 3, 1), (5, 64, 64, 4, 4, 3, 1), (3, 5, 64, 32, 32, 7, 2), (5, 128, 64, 8, 8, 1, 1)):
        cs = dict(ci=ci, co=co, k=k, stride=st, h=hh, w=ww)
        x, dz = R.wg_operands(n, ci, co, hh, ww, st, "randn", dtype, g)
        ref, bound = R.conv_wgrad(x, dz, cs), R.wg_bound(x, dz, cs)
        err = (R.wg_fp32_accumulated(x, dz, cs) - ref).abs()
        assert bool((bound > 0).all()) and bool((err <= bound).all()), (cs, float((err / bound).max()))
        assert float((err / bound).max()) < 0.5
        # and the bound is no blanket: an error of one part in 2^12 of the element's magnitude is outside it
        assert bool((bound < 2.0 ** -12 * R.conv_wgrad(x.abs(), dz.abs(), cs)).all())
