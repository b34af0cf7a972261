"""AdamW parameter groups end to end (FusedAdamW over a list of dicts, ModelTrainer.param_groups, StudentEngine.adamw_step(groups=))
on the smallest shapes: ResNet-18, 3 channels, 64 x 64, D = 32, the motion head, 8 crops, both element types, three steps.
Four groups: the stem (conv1, bn1) held still at (0, 0); BatchNorm tensors and every bias at (lr, 0); the other backbone weights at
(0.1 lr, 0.01); the head's weights (fc, motion head) at (lr, 0.01).

Bounds: a single step lies, element by element, inside opref.adamw_bounds of opref.adamw_ref with the element's own group's
(lr, wd), from a snapshot of (p, m, v) and the materialised gradients taken right before that step, so drift does not enter (the
float64 reference is evaluated on the device); equality of bits where the arithmetic is the same -- the still group, the lazy fused
path against the flat one, the fused repack against a repack from the parameters; test_clip_gpu's one float32 ulp for the norm."""
import pytest
import torch

from tests import opref_clip as RC
from tests import opref_groups as G
from tests.test_clip_gpu import LR, _bits, _build, _train_step

pytestmark = pytest.mark.gpu
MODES = ("bf16", "fp16_static", "fp16_dynamic")
LR_WD = ((0.0, 0.0), (LR, 0.0), (0.1 * LR, 0.01), (LR, 0.01))
SHARED = dict(b1=0.9, b2=0.999, eps=1e-8)
STEM = ("resnet.conv1.weight", "resnet.bn1.weight", "resnet.bn1.bias")


def _named(enc, tr):
    from vpd_amd.engine import DECODER_PARAM_NAMES
    return ([(k, enc.get_parameter(k)) for k in enc.engine.enc_names] +
            [("decoder." + k, tr.fcn_time.get_parameter(k)) for k in DECODER_PARAM_NAMES])


def _group_of(eng, name):
    if name in STEM:
        return 0
    if eng.layout[name][0] in (1, 2, 4):      # BatchNorm weight, BatchNorm bias, linear bias
        return 1
    return 3 if name.startswith("resnet.fc.") or name.startswith("decoder.") else 2


def _four_groups(enc, tr):
    """torch's list of dicts, and every element's group on the device (padding floats: the group in front of them)"""
    eng = enc.engine
    groups = [dict(params=[], lr=lr, weight_decay=wd) for lr, wd in LR_WD]
    ids = []
    for name, q in _named(enc, tr):
        ids.append(_group_of(eng, name))
        groups[ids[-1]]["params"].append(q)
    return groups, _element_groups(eng, [name for name, _ in _named(enc, tr)], ids)


def _element_groups(eng, names, ids):
    eg = torch.full((eng.param_numel,), ids[-1], dtype=torch.int64)
    for name, gid in zip(names, ids):
        _, _, off, n, _ = eng.layout[name]
        eg[off:off + n] = gid
    return eg.cuda()


def _build_mode(mode, **kw):
    from vpd_amd.models.util import DynamicLossScaler
    enc, tr, img, tgt = _build("bf16" if mode == "bf16" else "fp16", motion=True, **kw)
    make_scaler = None
    if mode == "fp16_dynamic":      # (start 256: nothing overflows on these shapes, tests/test_dynscale_gpu.py)
        make_scaler = lambda: DynamicLossScaler(enc.engine, init_scale=256, growth_interval=10 ** 6)
    return enc, tr, img, tgt, make_scaler


def _optimizer(tr, groups, make_scaler, **kw):
    opt, scaler = tr.get_optimizer(LR, param_groups=groups, **kw)
    return opt, (make_scaler() if make_scaler is not None else scaler)


def _snapshot_step(tr, opt, scaler, img, tgt):
    """one step with the plain backward -> (p, g, m, v) as they stood right before optimizer.step(), and the loss scale in g"""
    eng = tr.encoder.engine
    tr.encoder.train()
    tr.fcn_time.train()
    loss = tr._forward_loss(img, tgt, train=True)
    (loss if scaler is None else scaler.scale(loss)).backward()
    scale = 1.0 if scaler is None else scaler.get_scale()
    zero = torch.zeros_like(eng.params)
    before = (eng.params.clone(), eng.grads.clone(), zero if eng.adam_m is None else eng.adam_m.clone(),
              zero if eng.adam_v is None else eng.adam_v.clone())
    if scaler is None:
        opt.step()
    else:
        scaler.step(opt)
        scaler.update()
    opt.zero_grad()
    torch.cuda.synchronize()
    return before, scale


def _assert_within(eng, before, eg, lr_wd, step, scale, what):
    got = (eng.params, eng.adam_m, eng.adam_v)
    ref = G.grouped_ref(before, eg, lr_wd, SHARED, step, gscale=1.0 / scale)
    bnd = G.grouped_bounds(before, eg, lr_wd, SHARED, step, gscale=1.0 / scale)
    ratios, outside = G.within(got, ref, bnd)
    print("%s step %d: max error / bound p %.3f m %.3f v %.3f" % ((what, step) + tuple(ratios)))
    assert outside == 0, (what, step, ratios, outside)
    return ref, bnd


@pytest.mark.parametrize("mode", MODES)
def test_every_single_step_is_adamw_with_each_elements_own_group(mode):
    enc, tr, img, tgt, make_scaler = _build_mode(mode)
    eng = enc.engine
    groups, eg = _four_groups(enc, tr)
    opt, scaler = _optimizer(tr, groups, make_scaler)
    p0 = eng.params.clone()
    for step in (1, 2, 3):
        before, scale = _snapshot_step(tr, opt, scaler, img, tgt)
        assert scale == (1.0 if mode == "bf16" else 256.0)
        ref, bnd = _assert_within(eng, before, eg, LR_WD, step, scale, mode)
        # ... and the bound tells the groups apart: with the backbone's and the head's hyper-parameters swapped it does not hold
        swapped = (LR_WD[0], LR_WD[1], LR_WD[3], LR_WD[2])
        off = G.grouped_ref(before, eg, swapped, SHARED, step, gscale=1.0 / scale)
        sel = eg >= 2
        assert float(((eng.params.double() - off[0]).abs() > bnd[0])[sel].float().mean()) >= 0.25
    assert eng.adam_step == 3 and eng.group_table_builds == 1
    # the stem stands still, bit for bit; its moments moved; everything else moved
    still = eg == 0
    assert torch.equal(_bits(eng.params[still]), _bits(p0[still]))
    assert float((eng.adam_m[still] != 0).float().mean()) > 0.5 and float((eng.adam_v[still] != 0).float().mean()) > 0.5
    assert float((eng.params[~still] != p0[~still]).float().mean()) > 0.9


def _three_lazy_steps(mode, grouped, fused, monkeypatch):
    monkeypatch.setenv("VPD_FUSED_ADAMW", "1" if fused else "0")
    enc, tr, img, tgt, make_scaler = _build_mode(mode)
    groups = _four_groups(enc, tr)[0] if grouped else None
    opt, scaler = _optimizer(tr, groups, make_scaler)
    names = []
    record = lambda name, fn: (lambda *a: (names.append(name), fn(*a))[1])
    L = enc.engine.L
    for name in ("vpd_plan_adamw_step_groups", "vpd_adamw_step_groups", "vpd_plan_adamw_step", "vpd_plan_adamw_step_scaled",
                 "vpd_adamw_step", "vpd_adamw_step_scaled"):
        monkeypatch.setattr(L, name, record(name, getattr(L, name)))
    for _ in range(3):
        _train_step(tr, opt, scaler, img, tgt)      # models.util.step(): the lazy backward
    return enc, tr, img, tgt, set(names)


@pytest.mark.parametrize("grouped", [False, True], ids=["one_group", "four_groups"])
@pytest.mark.parametrize("mode", ["bf16", "fp16_dynamic"])
def test_lazy_fused_path_equals_the_flat_path_in_bits_and_repacks_what_it_wrote(mode, grouped, monkeypatch):
    """one_group: the property as the ungrouped step has it on this input (the launches of always); four_groups: the grouped one"""
    a = _three_lazy_steps(mode, grouped, True, monkeypatch)
    b = _three_lazy_steps(mode, grouped, False, monkeypatch)
    dyn = mode == "fp16_dynamic"
    if grouped:
        assert a[4] == {"vpd_plan_adamw_step_groups"} and b[4] == {"vpd_adamw_step_groups"}
    else:
        assert a[4] == {"vpd_plan_adamw_step_scaled" if dyn else "vpd_plan_adamw_step"}
        assert b[4] == {"vpd_adamw_step_scaled" if dyn else "vpd_adamw_step"}
    ea, eb = a[0].engine, b[0].engine
    for what in ("params", "adam_m", "adam_v"):
        x, y = getattr(ea, what), getattr(eb, what)
        assert torch.equal(_bits(x), _bits(y)), "%s: fused and flat differ in %d elements" % (what, int((_bits(x) != _bits(y)).sum()))
    if not grouped:
        return
    # the repack: the fused engine's train plan computes with the arena the step wrote (its packed weights are current: no
    # repack happens), a fresh engine loaded from the state_dicts packs from the parameters
    enc, tr, img, tgt = a[:4]
    assert ea._step_plan.packed_version == ea.weights_version()
    from tests.test_clip_gpu import _build as build
    enc2, tr2, _, _ = build("bf16" if mode == "bf16" else "fp16", motion=True)
    enc2.load_state_dict(enc.state_dict())
    tr2.fcn_time.load_state_dict(tr.fcn_time.state_dict())
    assert torch.equal(_bits(enc2.engine.params), _bits(ea.params))
    x, t = img.cuda(), tgt.cuda()
    e1 = ea.forward_train(x, t, motion=True, accumulate_loss=False)
    e2 = enc2.engine.forward_train(x, t, motion=True, accumulate_loss=False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(e1), _bits(e2)), "the train plan's packed weights are not what the parameters say"
    assert torch.equal(_bits(ea.loss_step), _bits(enc2.engine.loss_step))
    enc.eval(), enc2.eval()
    assert torch.equal(_bits(torch.from_numpy(enc.embed(img.numpy()))), _bits(torch.from_numpy(enc2.embed(img.numpy()))))


def test_a_scheduler_moves_each_groups_lr():
    enc, tr, img, tgt, _ = _build_mode("bf16")
    eng = enc.engine
    groups = tr.param_groups(weight_decay=0.01, decay_bn_bias=False, lr=LR)
    assert len(groups) == 2 and groups[0]["weight_decay"] == 0.01 and groups[1]["weight_decay"] == 0.0
    names = [name for name, _ in _named(enc, tr)]
    eg = _element_groups(eng, names, [1 if eng.layout[name][0] in (1, 2, 4) else 0 for name in names])
    opt, scaler = tr.get_optimizer(LR, param_groups=groups)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 0.5 ** e, lambda e: 0.1 ** e])
    before, _ = _snapshot_step(tr, opt, scaler, img, tgt)
    base = ((LR, 0.01), (LR, 0.0))
    _assert_within(eng, before, eg, base, 1, 1.0, "scheduler, epoch 0")
    sched.step()
    before, _ = _snapshot_step(tr, opt, scaler, img, tgt)
    moved = ((0.5 * LR, 0.01), (0.1 * LR, 0.0))
    _, bnd = _assert_within(eng, before, eg, moved, 2, 1.0, "scheduler, epoch 1")
    assert eng.group_table_builds == 1
    stale = G.grouped_ref(before, eg, base, SHARED, 2)
    for gid in (0, 1):
        assert float(((eng.params.double() - stale[0]).abs() > bnd[0])[eg == gid].float().mean()) >= 0.25, gid


def test_clipping_takes_the_norm_of_all_gradients():
    enc, tr, img, tgt, _ = _build_mode("bf16")
    eng = enc.engine
    groups, eg = _four_groups(enc, tr)
    opt, scaler = _optimizer(tr, groups, None, max_grad_norm=float("inf"))
    before, _ = _snapshot_step(tr, opt, scaler, img, tgt)
    st = opt.clip_stats()
    ref = RC.clip_ref([before[1].cpu().numpy()], float("inf"))
    print("norm %.9g, float64 over all the flat gradients %.9g" % (st["total_norm"], ref["norm"]))
    assert abs(st["total_norm"] - float(ref["total_norm_f32"])) <= RC.ulp32(ref["norm"])
    assert st["coef"] == 1.0 and eng.adam_step == 1
    _assert_within(eng, before, eg, LR_WD, 1, 1.0, "with the clip block")
