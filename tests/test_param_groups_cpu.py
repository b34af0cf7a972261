"""AdamW parameter groups, the part that needs no GPU: the new entry points are declared, bound and exported and refuse bad arguments
on the host (never-dereferenced pointers, as tests/test_abi_cpu.py does), FusedAdamW turns torch's param_groups into the engine's
calls (a recording stub library, as tests/test_adamw_step_cpu.py does), ModelTrainer.param_groups partitions every tensor once, and
the per-segment float64 reference with its bounds (tests/opref_groups.py) holds a float32 transcription of the grouped update and
tells two groups' hyper-parameters apart."""
import ctypes as C

import pytest
import torch

from tests import opref as R
from tests import opref_groups as G
from tests.engine_stub import NUMEL, stub_engine
from tests.test_abi_cpu import header_functions
from tests.test_opref_cpu import _adamw1_f32

DTYPES = ("bf16", "fp16")
NEW = {"vpd_adam_groups_bytes": 1, "vpd_adam_groups_init": 8, "vpd_adamw_step_groups": 16, "vpd_plan_adamw_step_groups": 17,
       "vpd_op_adamw_pack_groups": 23}


def _lib(dtype):
    from vpd_amd import _lib
    return _lib.lib(dtype)


def _refused(h, rc, msg):
    return rc != 0 and msg in h.vpd_last_error()


def lls(*v):
    return (C.c_longlong * len(v))(*v)


def ints(*v):
    return (C.c_int * len(v))(*v)


def dbls(*v):
    return (C.c_double * len(v))(*v)


# ---------------------------------------------------------------------------
# 1, 2: the ABI
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_entry_points_are_declared_bound_and_exported(dtype):
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    assert h.vpd_abi_version() == _lib.ABI_VERSION == 5
    for n, nargs in NEW.items():
        assert n in header_functions() and len(_lib.SIGNATURES[n][1]) == nargs and getattr(h, n).argtypes == _lib.SIGNATURES[n][1]
    # header, 8-byte offsets, 4-byte group ids, rounded up to 16 bytes
    assert h.vpd_adam_groups_bytes(1) == 48 and h.vpd_adam_groups_bytes(3) == 64 and h.vpd_adam_groups_bytes(100) == 1232
    assert h.vpd_adam_groups_bytes(0) == 0


# ---------------------------------------------------------------------------
# 3: vpd_adam_groups_init
# ---------------------------------------------------------------------------
def _plan(h, dtype):
    from vpd_amd import _lib
    p = C.c_void_p()
    _lib.check(h.vpd_plan_create(b"resnet18", 3, 64, 64, 32, 1, 8, 1, C.byref(p)), "create", dtype)
    return p


def _tensors(h, p):
    kind, dec, off, numel, ndim = C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong(), C.c_int()
    dims = (C.c_int * 4)()
    rows = []
    for i in range(h.vpd_plan_num_tensors(p)):
        assert h.vpd_plan_tensor_info(p, i, C.byref(kind), C.byref(dec), C.byref(off), C.byref(numel), C.byref(ndim), dims) == 0
        rows.append((kind.value, off.value, numel.value, ndim.value))
    return rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_groups_init_refuses_bad_tables_on_the_host(dtype):
    h = _lib(dtype)
    t = C.c_void_p(64)                                    # never dereferenced: every call below is refused before the copy
    odd = C.c_void_p(72)
    begin, group = lls(0, 100, 4096), ints(1, 0)

    def init(plan=None, table=t, begin=begin, group=group, nseg=2, numel=4096, ngroups=2):
        return h.vpd_adam_groups_init(plan, table, begin, group, nseg, numel, ngroups, None)
    assert _refused(h, init(table=None), b"null argument")
    assert _refused(h, init(begin=None), b"null argument") and _refused(h, init(group=None), b"null argument")
    assert _refused(h, init(nseg=0), b"nseg must be >= 1") and _refused(h, init(nseg=-3), b"nseg must be >= 1")
    assert _refused(h, init(ngroups=0), b"ngroups outside 1..16") and _refused(h, init(ngroups=17), b"ngroups outside 1..16")
    assert _refused(h, init(begin=lls(4, 100, 4096)), b"seg_begin[0] must be 0")
    assert _refused(h, init(begin=lls(0, 0, 4096)), b"ascend") and _refused(h, init(begin=lls(0, 4096, 100)), b"ascend")
    assert _refused(h, init(begin=lls(0, 100, 4092)), b"must equal numel")
    assert _refused(h, init(begin=lls(0, 100, 4098), numel=4098), b"multiple of 4")
    assert _refused(h, init(group=ints(0, 2)), b"group id outside") and _refused(h, init(group=ints(-1, 0)), b"group id outside")
    assert _refused(h, init(table=odd), b"16-byte aligned")
    # with a plan (host-only): numel is the plan's, and no boundary cuts a conv weight -- at a tensor's begin or end it may lie
    p = _plan(h, dtype)
    numel = h.vpd_plan_param_numel(p)
    rows = _tensors(h, p)
    convs = [(off, n) for kind, off, n, ndim in rows if ndim == 4]
    assert len(convs) >= 20
    assert _refused(h, init(plan=p), b"must equal vpd_plan_param_numel")
    for off, n in (convs[0], convs[3], convs[-1]):       # the stem conv too
        for cut in (off + 4, off + 1, off + n - 1):
            assert _refused(h, init(plan=p, begin=lls(0, cut, numel), numel=numel), b"inside a conv weight"), (off, cut)
    h.vpd_plan_destroy(p)


# ---------------------------------------------------------------------------
# 4: the step entries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_grouped_step_entries_refuse_bad_arguments_on_the_host(dtype):
    h = _lib(dtype)
    p = C.c_void_p(64)
    odd = C.c_void_p(72)
    lr, wd = dbls(5e-4, 1e-3), dbls(0.01, 0.0)
    plan = _plan(h, dtype)
    numel = h.vpd_plan_param_numel(plan)

    def flat(bufs=(p, p, p, p), numel=4096, table=p, lr=lr, wd=wd, ngroups=2, step=1, state=None):
        return h.vpd_adamw_step_groups(*bufs, numel, table, lr, wd, ngroups, 0.9, 0.999, 1e-8, step, 1.0, state, None)

    def fused(bufs=(p, p, p, p), numel=numel, table=p, lr=lr, wd=wd, ngroups=2, step=1, state=None, plan=plan, ws=p):
        return h.vpd_plan_adamw_step_groups(plan, *bufs, numel, table, lr, wd, ngroups, 0.9, 0.999, 1e-8, step, state, ws, None)
    for fn in (flat, fused):
        for i in range(4):
            bufs = [p, p, p, p]
            bufs[i] = None
            assert _refused(h, fn(bufs=bufs), b"null argument"), i
            bufs[i] = odd
            assert _refused(h, fn(bufs=bufs), b"16-byte aligned"), i
        assert _refused(h, fn(table=None), b"null argument") and _refused(h, fn(table=odd), b"16-byte aligned")
        assert _refused(h, fn(lr=None), b"null lr or weight_decay") and _refused(h, fn(wd=None), b"null lr or weight_decay")
        assert _refused(h, fn(ngroups=0), b"ngroups outside 1..16") and _refused(h, fn(ngroups=17), b"ngroups outside 1..16")
        assert _refused(h, fn(lr=dbls(5e-4, -1e-3)), b"lr must not be negative or NaN")
        assert _refused(h, fn(lr=dbls(float("nan"), 1e-3)), b"lr must not be negative or NaN")
        assert _refused(h, fn(wd=dbls(0.01, -0.5)), b"weight_decay must not be negative or NaN")
        assert _refused(h, fn(wd=dbls(0.01, float("nan"))), b"weight_decay must not be negative or NaN")
        assert _refused(h, fn(step=0), b"1-based")
        assert _refused(h, fn(numel=4102), b"multiple of 4")
    assert _refused(h, fused(plan=None), b"null argument") and _refused(h, fused(ws=None), b"null argument")
    assert _refused(h, fused(), b"workspace not initialised")       # (a plan whose workspace was never bound: host-only)
    # the synthetic-buffer entry: its own table is checked, and a boundary inside a synthetic conv is refused
    dims = ints(32, 32, 3, 64, 32, 1)
    offs = lls(100, 100 + 9216 + 8)
    n = 100 + 9216 + 8 + 2048 + 4

    def pack(begin=lls(0, 100, 9316, n), group=ints(0, 1, 0), nseg=3, lr=lr, wd=wd, ngroups=2, step=1, ptrs=(p, p, p, p, p, None)):
        return h.vpd_op_adamw_pack_groups(2, dims, offs, n, *ptrs, begin, group, nseg, lr, wd, ngroups, 0.9, 0.999, 1e-8, step, 1.0,
                                          None, None)
    assert _refused(h, pack(ptrs=(p, None, p, p, p, None)), b"null argument")
    assert _refused(h, pack(begin=None), b"null argument") and _refused(h, pack(lr=None), b"null lr or weight_decay")
    assert _refused(h, pack(step=0), b"1-based") and _refused(h, pack(ngroups=17), b"ngroups outside")
    assert _refused(h, pack(group=ints(0, 2, 0)), b"group id outside")
    assert _refused(h, pack(begin=lls(0, 100, 9316, n - 4)), b"must equal numel")
    assert _refused(h, pack(begin=lls(0, 104, 9316, n)), b"inside a conv weight")
    assert _refused(h, pack(begin=lls(0, 100, 9324 + 2047, n)), b"inside a conv weight")
    h.vpd_plan_destroy(plan)


# ---------------------------------------------------------------------------
# 5: FusedAdamW on a recording library
# ---------------------------------------------------------------------------
# a toy layout in the engine's terms: name -> (kind, is_decoder, offset, numel, shape); 2 padding floats at the end
LAYOUT = [("resnet.conv1.weight", 0, 0, 0, 16), ("resnet.bn1.weight", 1, 0, 16, 4), ("resnet.bn1.bias", 2, 0, 20, 4),
          ("resnet.layer1.0.conv1.weight", 0, 0, 24, 16), ("resnet.fc.weight", 3, 0, 40, 8), ("resnet.fc.bias", 4, 0, 48, 4),
          ("decoder.layers.0.weight", 3, 1, 52, 8), ("decoder.layers.0.bias", 4, 1, 60, 2)]
ENC = 52


def _stub_engine(plan_numel=NUMEL):
    return stub_engine(plan_numel, LAYOUT)


def _tensors_of(eng, decoder=True):
    """name -> a Parameter that views the engine's flat buffer where the layout says"""
    return {n: torch.nn.Parameter(eng.params[o:o + m]) for n, k, d, o, m in LAYOUT if decoder or not d}


def _steps(eng):
    return [c for c in eng.L.calls if c[0] not in ("vpd_plan_grads_pending", "vpd_adam_groups_bytes")]


def _ptr(t):
    return t.data_ptr()


def test_one_group_gives_exactly_the_calls_of_the_ungrouped_step(monkeypatch):
    from vpd_amd.trainer import FusedAdamW
    monkeypatch.setenv("VPD_FUSED_ADAMW", "1")
    eng = _stub_engine()
    t = _tensors_of(eng)
    opt = FusedAdamW([{"params": list(t.values())}], eng, lr=1e-3)
    opt.step()
    pl = eng._step_plan
    base = (_ptr(eng.params), _ptr(eng._grads), _ptr(eng.adam_m), _ptr(eng.adam_v), NUMEL, 1e-3, 0.9, 0.999, 1e-8, 0.01)
    assert eng.L.calls == [("vpd_plan_adamw_step", (pl.handle.value,) + base + (7, _ptr(pl.workspace), None))]
    assert eng.group_table_builds == 0 and eng._group_table is None


def _two_groups(t, wd_lr=None):
    decay = [q for n, q in t.items() if not (n.endswith(".bias") or ".bn" in n)]
    no_decay = [q for n, q in t.items() if n.endswith(".bias") or ".bn" in n]
    return [{"params": decay}, dict({"params": no_decay, "weight_decay": 0.0}, **(wd_lr or {}))]


def test_two_groups_give_the_grouped_entry_with_merged_segments_and_schedulers_move_lr_only(monkeypatch):
    from vpd_amd.trainer import FusedAdamW
    monkeypatch.setenv("VPD_FUSED_ADAMW", "1")
    eng = _stub_engine()
    t = _tensors_of(eng)
    opt = FusedAdamW(_two_groups(t, {"lr": 2e-3}), eng, lr=1e-3)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 0.5 ** e, lambda e: 0.1 ** e])
    opt.step()
    pl = eng._step_plan
    calls = _steps(eng)
    assert [c[0] for c in calls] == ["vpd_adam_groups_init", "vpd_plan_adamw_step_groups"]
    # conv1 | bn1.weight + bn1.bias | layer1 conv + fc.weight | fc.bias | decoder weight | decoder bias (+ the padding)
    begin, group = [0, 16, 24, 48, 52, 60, 64], [0, 1, 0, 1, 0, 1]
    table = _ptr(eng._group_table)
    assert calls[0][1] == (pl.handle.value, table, begin, group, 6, NUMEL, 2, None)
    bufs = (_ptr(eng.params), _ptr(eng._grads), _ptr(eng.adam_m), _ptr(eng.adam_v), NUMEL, table)
    assert calls[1][1] == (pl.handle.value,) + bufs + ([1e-3, 2e-3], [0.01, 0.0], 2, 0.9, 0.999, 1e-8, 7, None, _ptr(pl.workspace), None)
    assert pl.packed_version == eng.weights_version() and eng._adam_step == 7
    # a LambdaLR step changes the next call's lr[] and does not rebuild the table
    eng.L.calls.clear()
    sched.step()
    opt.step()
    calls = _steps(eng)
    assert [c[0] for c in calls] == ["vpd_plan_adamw_step_groups"] and eng.group_table_builds == 1
    assert calls[0][1][7] == pytest.approx([5e-4, 2e-4]) and calls[0][1][8] == [0.01, 0.0] and calls[0][1][13] == 8
    # add_param_group rebuilds it: the decoder's bias moves out of group 1 into a group of its own, held still
    eng2 = _stub_engine()
    t2 = _tensors_of(eng2)
    groups = _two_groups({n: q for n, q in t2.items() if n != "decoder.layers.0.bias"})
    with pytest.raises(ValueError, match="missing: decoder.layers.0.bias.*lr=0, weight_decay=0"):
        FusedAdamW(groups, eng2, lr=1e-3)                                                   # a missing tensor
    opt2 = FusedAdamW(_two_groups(t2), eng2, lr=1e-3)
    opt2.step()
    opt2.param_groups[1]["params"] = [q for q in opt2.param_groups[1]["params"] if q is not t2["decoder.layers.0.bias"]]
    opt2.add_param_group({"params": [t2["decoder.layers.0.bias"]], "lr": 0.0, "weight_decay": 0.0})
    eng2.L.calls.clear()
    opt2.step()
    calls = _steps(eng2)
    assert [c[0] for c in calls] == ["vpd_adam_groups_init", "vpd_plan_adamw_step_groups"] and eng2.group_table_builds == 2
    assert calls[0][1][2:7] == ([0, 16, 24, 48, 52, 60, 64], [0, 1, 0, 1, 0, 2], 6, NUMEL, 3)
    assert calls[1][1][7:10] == ([1e-3, 1e-3, 0.0], [0.01, 0.0, 0.0], 3)


def test_group_refusals_of_the_optimizer():
    from vpd_amd.trainer import FusedAdamW
    eng = _stub_engine()
    t = _tensors_of(eng)
    with pytest.raises(ValueError, match="betas and eps must be the same"):
        FusedAdamW(_two_groups(t, {"betas": (0.8, 0.999)}), eng, lr=1e-3)
    with pytest.raises(ValueError, match="betas and eps must be the same"):
        FusedAdamW(_two_groups(t, {"eps": 1e-6}), eng, lr=1e-3)
    opt = FusedAdamW(_two_groups(t), eng, lr=1e-3)
    opt.param_groups[1]["betas"] = (0.9, 0.99)                                              # ... and at step()
    with pytest.raises(ValueError, match="betas and eps must be the same"):
        opt.step()
    assert _steps(eng) == []
    qs = list(t.values())
    extra = [torch.nn.Parameter(eng.params[o:o + 1]) for o in range(1, 10)]
    assert len(qs) + len(extra) == 17
    with pytest.raises(ValueError, match="17 parameter groups, at most 16"):
        FusedAdamW([{"params": [q]} for q in qs + extra], eng, lr=1e-3)
    with pytest.raises(ValueError, match="not one of the engine's tensors"):
        FusedAdamW(_two_groups(t) + [{"params": extra[:1]}], eng, lr=1e-3)


@pytest.mark.parametrize("path", ["no_decoder", "env", "stale", "clip"])
def test_the_flat_path_carries_its_groups(monkeypatch, path):
    """an optimizer without the motion head behind a plan that trains it, VPD_FUSED_ADAMW=0 and stale packed weights all take the
    flat grouped kernel over the leading numel elements; the clip norm pass and the clip block's own count stay where they were"""
    from vpd_amd.trainer import FusedAdamW
    monkeypatch.setenv("VPD_FUSED_ADAMW", "0" if path == "env" else "1")
    eng = _stub_engine()
    t = _tensors_of(eng, decoder=path != "no_decoder")
    opt = FusedAdamW(_two_groups(t), eng, lr=1e-3)
    numel = ENC if path == "no_decoder" else NUMEL
    assert opt._numel == numel
    if path == "stale":
        eng._hip_version += 1
    if path == "clip":
        eng._clip = torch.zeros(24, dtype=torch.int32)
        eng._clip_max_norm = 2.5
        eng._dyn_state = eng._clip
    stale = eng._step_plan.packed_version
    opt.step()
    calls = _steps(eng)
    table = _ptr(eng._group_table)
    bufs = (_ptr(eng.params), _ptr(eng._grads), _ptr(eng.adam_m), _ptr(eng.adam_v), numel, table)
    if path == "clip":      # the fused path, reading the clip block
        pl = eng._step_plan
        assert [c[0] for c in calls] == ["vpd_plan_grad_norm", "vpd_adam_groups_init", "vpd_plan_adamw_step_groups", "vpd_scale_state_update"]
        assert calls[2][1] == (pl.handle.value,) + bufs + ([1e-3, 1e-3], [0.01, 0.0], 2, 0.9, 0.999, 1e-8, 1, _ptr(eng._clip),
                                                           _ptr(pl.workspace), None)
        return
    assert [c[0] for c in calls] == ["vpd_adam_groups_init", "vpd_adamw_step_groups"]
    want_begin = [0, 16, 24, 48, 52] if path == "no_decoder" else [0, 16, 24, 48, 52, 60, 64]
    assert calls[0][1] == (None, table, want_begin, [0, 1, 0, 1, 0, 1][:len(want_begin) - 1], len(want_begin) - 1, numel, 2, None)
    assert calls[1][1] == bufs + ([1e-3, 1e-3], [0.01, 0.0], 2, 0.9, 0.999, 1e-8, 7, 1.0, None, None)
    assert eng._step_plan.packed_version is stale


# ---------------------------------------------------------------------------
# 6: ModelTrainer.param_groups
# ---------------------------------------------------------------------------
class _Named:
    def __init__(self, t, strip):
        self._t, self._strip = t, strip

    def get_parameter(self, k):
        return self._t[self._strip + k]


@pytest.mark.parametrize("motion", [False, True])
@pytest.mark.parametrize("decay_bn_bias", [True, False])
@pytest.mark.parametrize("scale", [1.0, 0.1])
def test_trainer_param_groups_partition_every_tensor_once(monkeypatch, scale, decay_bn_bias, motion):
    import vpd_amd.models.module as M
    from vpd_amd.trainer import ModelTrainer
    eng = _stub_engine()
    eng.enc_names = [n for n, k, d, o, m in LAYOUT if not d]
    t = _tensors_of(eng)
    tr = ModelTrainer.__new__(ModelTrainer)
    tr.encoder = _Named(t, "")
    tr.encoder.engine = eng
    if motion:
        tr.fcn_time = _Named(t, "decoder.")
    monkeypatch.setattr(M, "DECODER_PARAM_NAMES", ["layers.0.weight", "layers.0.bias"])      # (the toy layout's motion head)
    groups = tr.param_groups(weight_decay=0.05, decay_bn_bias=decay_bn_bias, backbone_lr_scale=scale, lr=1e-3)
    want = [n for n, k, d, o, m in LAYOUT if motion or not d]
    by_id = {id(q): n for n, q in t.items()}
    seen = [by_id[id(q)] for g in groups for q in g["params"]]
    assert sorted(seen) == sorted(want) and len(groups) == (1 if decay_bn_bias else 2) * (1 if scale == 1.0 else 2)
    kinds = {n: k for n, k, d, o, m in LAYOUT}
    for g in groups:
        for q in g["params"]:
            n = by_id[id(q)]
            head = n.startswith("resnet.fc.") or n.startswith("decoder.")
            assert g["weight_decay"] == (0.05 if decay_bn_bias or kinds[n] not in (1, 2, 4) else 0.0), n
            assert g["lr"] == pytest.approx(1e-3 if head else 1e-3 * scale), n
    with pytest.raises(ValueError, match="needs lr"):
        tr.param_groups(backbone_lr_scale=0.1)


# ---------------------------------------------------------------------------
# 7, 8: the reference and its bounds
# ---------------------------------------------------------------------------
def _grouped_f32(ins, elem_group, shared, step):
    """the grouped update in numpy float32: test_opref_cpu's transcription of adamw1 with every element's own (lr, wd)"""
    out = None
    for gid, (lr, wd) in enumerate(G.GROUP_LR_WD):
        res = _adamw1_f32(*ins, lr=lr, wd=wd, b1=shared["b1"], b2=shared["b2"], eps=shared["eps"], step=step)
        if out is None:
            out = [torch.zeros_like(x) for x in res]
        for o, x in zip(out, res):
            o[elem_group == gid] = x[elem_group == gid]
    return out


@pytest.mark.parametrize("buf,hyper,step", [("a", "torch", 1), ("a", "strong", 1000), ("b", "torch", 1000), ("b", "strong", 1)])
def test_grouped_reference_holds_the_float32_transcription_and_tells_groups_apart(buf, hyper, step):
    shared = R.ADAM_HYPERS[hyper]
    _, _, numel = R.adam_pack_layout(buf)
    table = G.segment_table(buf)
    begin, group = table
    assert begin[0] == 0 and begin[-1] == numel and all(a < b for a, b in zip(begin, begin[1:])) and set(group) == {0, 1, 2, 3}
    assert any(a == b for a, b in zip(group, group[1:])) and any(b - a == 1 for a, b in zip(begin, begin[1:]))
    assert any(x % 4 for x in begin)
    eg = G.element_groups(table, numel)
    ins = R.adamw_inputs(numel, step, 11)
    got = _grouped_f32(ins, eg, shared, step)
    ref = G.grouped_ref(ins, eg, G.GROUP_LR_WD, shared, step)
    bnd = G.grouped_bounds(ins, eg, G.GROUP_LR_WD, shared, step)
    ratios, outside = G.within(got, ref, bnd)
    print("grouped transcription %s %s step %d: max error / bound p %.3f m %.3f v %.3f" % ((buf, hyper, step) + tuple(ratios)))
    assert outside == 0 and max(ratios) <= 1.0
    # the still group keeps p in bits, and its moments moved
    still = eg == G.STILL
    assert torch.equal(R.bits(got[0][still]), R.bits(ins[0][still])) and not torch.equal(got[1][still], ins[2][still])
    # 8: two groups' hyper-parameters swapped: the elements of both leave the bounds (m and v do not depend on lr / wd)
    for a, b in ((0, 1), (0, 2), (2, 3), (1, 3)):
        swapped = list(G.GROUP_LR_WD)
        swapped[a], swapped[b] = swapped[b], swapped[a]
        off = G.grouped_ref(ins, eg, swapped, shared, step)
        sel = (eg == a) | (eg == b)
        bad = ((got[0].double() - off[0]).abs() > bnd[0])[sel].float().mean()
        assert float(bad) >= 0.25, (a, b, float(bad))
        assert not bool(((got[0].double() - off[0]).abs() > bnd[0])[~sel].any())
