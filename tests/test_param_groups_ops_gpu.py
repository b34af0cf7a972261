"""AdamW parameter groups one launch at a time: the grouped instantiations of adamw_pack_kernel (vpd_op_adamw_pack_groups) and of
adamw_kernel (vpd_adamw_step_groups) over the synthetic flat buffers of tests/opref.py with the segment tables of
tests/opref_groups.py, in both builds.  The grouped launch must equal, IN BITS, what four ungrouped launches -- one per group's
(lr, wd) -- give on each group's segments (parameters, moments and, conv by conv, both layouts of the arena), lie inside the
per-element bounds of the float64 reference, and the flat grouped kernel must equal the fused one.  Host step and device block,
conv gradients from the flat buffer and from the kernels' scratch layout."""
import ctypes as C
import functools

import pytest
import torch

from tests import opref as R
from tests import opref_groups as G
from tests.test_boundary_ops_gpu import (NAMES, SLACK, _adamw_pack, _check, _f32_sentinel, _flat, _lib, _same_bits, _scale_state)
from tests.test_model_gpu import _dump
from tests.test_ops_gpu import ptr, stream

pytestmark = pytest.mark.gpu
RATIOS = {}
CASES = [("a", "torch", 1), ("a", "strong", 1000), ("b", "torch", 1000), ("b", "strong", 1)]
LR = [lr for lr, _ in G.GROUP_LR_WD]
WD = [wd for _, wd in G.GROUP_LR_WD]


def _record(name, key, value):
    RATIOS.setdefault(name, {})[key] = value
    _dump("param_groups_ops_%s" % name, RATIOS[name])


def dbls(v):
    return (C.c_double * len(v))(*v)


@functools.lru_cache(maxsize=None)
def _case(buf, hyper, step):
    """inputs, table, every element's group, the float64 expectation and its bounds: computed once, shared, never written"""
    layout = R.adam_pack_layout(buf)
    numel = layout[2]
    table = G.segment_table(buf)
    eg = G.element_groups(table, numel)
    ins = R.adamw_inputs(numel, step, 11)
    shared = R.ADAM_HYPERS[hyper]
    return layout, table, eg, ins, G.grouped_ref(ins, eg, G.GROUP_LR_WD, shared, step), G.grouped_bounds(ins, eg, G.GROUP_LR_WD, shared, step)


def _scratch(layout, g):
    """the conv gradients in the weight-gradient kernels' layout, and the flat gradients with NaN over the convs"""
    dims, offs, _ = layout
    g_nan, pieces = g.clone(), []
    for (Co, Ci, k), o in zip(dims, offs):
        ns = Co * Ci * k * k
        pieces.append(R.wgrad_scratch_layout(g[o:o + ns].view(Co, Ci, k, k), Ci).flatten())
        g_nan[o:o + ns] = float("nan")
    return g_nan, torch.cat(pieces)


def _device_bufs(ins, numel):
    p, g, m, v = ins
    bufs = []
    for t in (p, m, v):
        b = _f32_sentinel(numel + SLACK)
        b[:numel] = t.cuda()
        bufs.append(b)
    return bufs, g.cuda()


def _collect(bufs, numel):
    out = [b.cpu() for b in bufs]
    for b in out:
        assert bool((b[numel:] == R.SENTINEL_F32).all()), "wrote beyond [0, numel)"
    return [b[:numel] for b in out]


def _pack_groups(name, layout, ins, table, shared, step, wg=None, gscale=1.0, state=None, lr=LR, wd=WD):
    """vpd_op_adamw_pack_groups -> (p, m, v) [numel] and the arena on the CPU; state: (scale, applied steps, found) or None"""
    dims, offs, numel = layout
    begin, group = table
    bufs, gd = _device_bufs(ins, numel)
    na = 2 * sum(Co * Ci * k * k for Co, Ci, k in dims)
    arena = R.sentinel_elems(na + SLACK, name).cuda()
    wgd = wg.cuda() if wg is not None else None
    st = _scale_state(*state) if state is not None else None
    _check(_lib(name).vpd_op_adamw_pack_groups(
        len(dims), (C.c_int * (3 * len(dims)))(*[x for d in dims for x in d]), (C.c_longlong * len(offs))(*offs), numel,
        ptr(bufs[0]), ptr(gd), ptr(bufs[1]), ptr(bufs[2]), ptr(arena), ptr(wgd) if wgd is not None else None,
        (C.c_longlong * len(begin))(*begin), (C.c_int * len(group))(*group), len(group), dbls(lr), dbls(wd), len(lr),
        shared["b1"], shared["b2"], shared["eps"], step, gscale, ptr(st) if st is not None else None, stream()), name)
    torch.cuda.synchronize()
    return _collect(bufs, numel), arena.cpu()


def _flat_groups(name, ins, table, shared, step, gscale=1.0, state=None, lr=LR, wd=WD):
    """vpd_adam_groups_init (no plan) + vpd_adamw_step_groups -> (p, m, v) on the CPU"""
    begin, group = table
    numel = ins[0].numel()
    L = _lib(name)
    bufs, gd = _device_bufs(ins, numel)
    tbl = torch.zeros(L.vpd_adam_groups_bytes(len(group)) // 4 + SLACK, dtype=torch.int32, device="cuda")
    _check(L.vpd_adam_groups_init(None, ptr(tbl), (C.c_longlong * len(begin))(*begin), (C.c_int * len(group))(*group), len(group),
                                  numel, len(lr), stream()), name)
    assert not bool(tbl[L.vpd_adam_groups_bytes(len(group)) // 4:].any()), "the table is longer than vpd_adam_groups_bytes says"
    st = _scale_state(*state) if state is not None else None
    _check(L.vpd_adamw_step_groups(ptr(bufs[0]), ptr(gd), ptr(bufs[1]), ptr(bufs[2]), numel, ptr(tbl), dbls(lr), dbls(wd), len(lr),
                                   shared["b1"], shared["b2"], shared["eps"], step, gscale, ptr(st) if st is not None else None,
                                   stream()), name)
    torch.cuda.synchronize()
    return _collect(bufs, numel)


def _from_ungrouped(name, layout, ins, eg, shared, step, wg, gscale):
    """the expectation of (a): one ungrouped vpd_op_adamw_pack per group's (lr, wd), every element -- and every conv's two arena
    layouts -- taken from the launch of its own group"""
    dims, offs, numel = layout
    runs = [_adamw_pack(name, layout, ins, dict(shared, lr=lr, wd=wd), step, wg=wg, gscale=gscale) for lr, wd in G.GROUP_LR_WD]
    pmv = [torch.empty(numel) for _ in range(3)]
    for gid, (got, _) in enumerate(runs):
        for o, t in zip(pmv, got):
            o[eg == gid] = t[eg == gid]
    arena = R.bits(runs[0][1]).clone()
    at = 0
    for (Co, Ci, k), o in zip(dims, offs):
        ns = Co * Ci * k * k
        gid = int(eg[o])
        assert bool((eg[o:o + ns] == gid).all())
        arena[at:at + 2 * ns] = R.bits(runs[gid][1])[at:at + 2 * ns]
        at += 2 * ns
    return pmv, arena


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("buf,hyper,step", CASES)
def test_grouped_pack_equals_four_ungrouped_launches_the_reference_and_the_flat_kernel(buf, hyper, step, name):
    layout, table, eg, ins, ref, bnd = _case(buf, hyper, step)
    shared = R.ADAM_HYPERS[hyper]
    p, g, m, v = ins
    g_nan, wg = _scratch(layout, g)
    k = 3 + step % 11
    still = eg == G.STILL
    assert bool(still.any())
    for mode in ("host", "block"):
        scale = 1.0 if mode == "host" else 2.0 ** k
        state = None if mode == "host" else (scale, step - 1, 0)
        step_arg = step if mode == "host" else 0      # (behind a block the step argument is ignored: the block's count + 1)
        for with_wg in (False, True):
            gin = (g_nan if with_wg else g) * scale
            wgin = wg * scale if with_wg else None
            what = "%s %s%s" % (name, mode, " wg" if with_wg else "")
            got, arena = _pack_groups(name, layout, (p, gin, m, v), table, shared, step_arg, wg=wgin, state=state)
            # (a) in bits against the ungrouped launches (host step, the gradient factor 1 / scale: the block's own arithmetic)
            want, want_arena = _from_ungrouped(name, layout, (p, gin, m, v), eg, shared, step, wgin, 1.0 / scale)
            for w_, a, b in zip("pmv", got, want):
                _same_bits(a, b, "(a) %s of the grouped launch vs its groups' ungrouped launches, %s" % (w_, what))
            _same_bits(arena, want_arena, "(a) arena, conv by conv, %s" % what)
            # (b) within the per-element bounds of the float64 reference
            ratios, outside = G.within(got, ref, bnd)
            print("adamw_pack_groups %s %s %s step %d: max error / bound p %.3f m %.3f v %.3f" % ((what, buf, hyper, step) + tuple(ratios)))
            _record(name, "pack_groups_%s_%s_%s%s" % (buf, hyper, mode, "_wg" if with_wg else ""), ratios)
            assert outside == 0, (what, ratios)
            # (d) the (0, 0) group keeps its parameters in bits; its moments move
            _same_bits(got[0][still], p[still], "(d) p of the still group, %s" % what)
            assert not torch.equal(got[1][still], m[still]) and not torch.equal(got[2][still], v[still])
            # (c) the flat grouped kernel on the same table (it reads the flat gradients)
            if not with_wg:
                flat = _flat_groups(name, (p, gin, m, v), table, shared, step_arg, state=state)
                for w_, a, b in zip("pmv", flat, got):
                    _same_bits(a, b, "(c) %s of the flat grouped kernel vs the fused one, %s" % (w_, what))


@pytest.mark.parametrize("name", NAMES)
def test_found_word_makes_both_grouped_kernels_write_nothing(name):
    layout, table, eg, ins, _, _ = _case("a", "torch", 1000)
    shared = R.ADAM_HYPERS["torch"]
    p, g, m, v = ins
    got, arena = _pack_groups(name, layout, ins, table, shared, 0, state=(8.0, 999, 1))
    for w_, a, b in zip("pmv", got, (p, m, v)):
        _same_bits(a, b, "(e) %s after a skipped fused step" % w_)
    assert bool((R.bits(arena) == R.SENTINEL_BITS[name]).all()), "(e) the arena was written"
    for w_, a, b in zip("pmv", _flat_groups(name, ins, table, shared, 0, state=(8.0, 999, 1)), (p, m, v)):
        _same_bits(a, b, "(e) %s after a skipped flat step" % w_)


@pytest.mark.parametrize("name", NAMES)
def test_one_segment_one_group_equals_the_ungrouped_launches(name):
    layout, _, _, ins, _, _ = _case("b", "strong", 1000)
    hp = R.ADAM_HYPERS["strong"]
    one = ([0, layout[2]], [0])
    want, want_arena = _adamw_pack(name, layout, ins, hp, 1000)
    got, arena = _pack_groups(name, layout, ins, one, hp, 1000, lr=[hp["lr"]], wd=[hp["wd"]])
    for w_, a, b in zip("pmv", got, want):
        _same_bits(a, b, "(f) %s of the one-group fused launch" % w_)
    _same_bits(arena, want_arena, "(f) arena of the one-group fused launch")
    for w_, a, b in zip("pmv", _flat_groups(name, ins, one, hp, 1000, lr=[hp["lr"]], wd=[hp["wd"]]), _flat(name, ins, hp, 1000)):
        _same_bits(a, b, "(f) %s of the one-group flat launch" % w_)


@pytest.mark.parametrize("name", NAMES)
def test_flat_grouped_kernel_beyond_one_pass_of_its_grid(name):
    """opref.ADAM_LONG elements, three segments: a boundary 2 mod 4 in the first pass of the capped grid and one 1 mod 4 among the
    elements of the second pass; against one ungrouped launch per group, in bits"""
    n = R.ADAM_LONG
    cut1, cut2 = n // 3 // 4 * 4 + 2, 4 * 256 * 4096 + 9
    assert cut1 % 4 == 2 and cut2 % 4 == 1 and cut2 < n
    table = ([0, cut1, cut2, n], [1, 3, 0])
    shared = R.ADAM_HYPERS["torch"]
    ins = R.adamw_inputs(n, 3, 5)
    got = _flat_groups(name, ins, table, shared, 3)
    runs = {gid: _flat(name, ins, dict(shared, lr=LR[gid], wd=WD[gid]), 3) for gid in (0, 1, 3)}
    for s, gid in enumerate(table[1]):
        a, b = table[0][s], table[0][s + 1]
        for w_, x, y in zip("pmv", got, runs[gid]):
            _same_bits(x[a:b], y[a:b], "%s of segment %d" % (w_, s))
    _same_bits(got[0][cut1:cut2], ins[0][cut1:cut2], "p of the still segment")
