"""Gradient-norm clipping in the fused step, end to end (StudentEngine.enable_grad_clip, FusedAdamW(max_grad_norm=),
ModelTrainer.get_optimizer(max_grad_norm=), train_vpd_model.py --clip_grad_norm) on the smallest shapes: ResNet-18, 3 channels,
64 x 64, 8 crops, D = 32, and one ResNet-50 case for the Bottleneck ranges.

Bounds: equality of bits where the arithmetic is the same (a coefficient of 1 multiplies nothing; a skipped step writes nothing);
1 float32 ulp between two orders of the same double sum; the per-element AdamW bounds of tests/opref.py, widened by the gradient
factor's relative error 5 * 2^-24 (the rounding of eff.scale, the up to 2.5 ulp of 1.0f / x, one product), for the binding step.
inf is a VALUE planted in a target."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vpd_oracle as O
from tests import opref as P
from tests import opref_clip as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_IN, D, N, HW, LR = 3, 32, 8, 64, 5e-4
HYP = dict(lr=LR, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)
G_REL = 5 * 2.0 ** -24


def _bits(t):
    return t.contiguous().view(torch.int32)


def _build(dtype="bf16", motion=False, arch="resnet18", seed=60, **kw):
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    enc = RGBF_EmbeddingModel(arch, D, False, "cuda", dtype=dtype)
    enc.load_state_dict(O.procedural_state_dict(O.encoder_schema(arch, C_IN, D), seed))
    tr = ModelTrainer(enc, motion, **kw)
    if motion:
        tr.fcn_time.load_state_dict(O.procedural_state_dict(O.decoder_schema(D), seed + 7))
    return enc, tr, O.synthetic_crops(N, C_IN, HW, seed + 1), O.synthetic_targets(N, D, motion, seed + 2)


def _train_step(tr, opt, scaler, img, tgt):
    from vpd_amd.models.util import step
    tr.encoder.train()
    if hasattr(tr, "fcn_time"):
        tr.fcn_time.train()
    step(opt, scaler, tr._forward_loss(img, tgt, train=True))
    torch.cuda.synchronize()


def _optimizer(tr, mode, max_grad_norm):
    """mode: 'bf16' | 'fp16_static' | 'fp16_dynamic' (start 256: nothing overflows on these shapes, tests/test_dynscale_gpu.py)"""
    from vpd_amd.models.util import DynamicLossScaler
    opt, scaler = tr.get_optimizer(LR, max_grad_norm=max_grad_norm)
    if mode == "fp16_dynamic":
        scaler = DynamicLossScaler(tr.encoder.engine, init_scale=256, growth_interval=10 ** 6)
    return opt, scaler


def _measured_norm(arch="resnet18"):
    """the first step's gradient norm, measured without clipping (max_norm = +inf)"""
    enc, tr, img, tgt = _build(arch=arch)
    opt, scaler = tr.get_optimizer(LR, max_grad_norm=float("inf"))
    _train_step(tr, opt, scaler, img, tgt)
    st = opt.clip_stats()
    assert st["coef"] == 1.0 and st["clipped_steps"] == 0 and st["nonfinite_steps"] == 0 and np.isfinite(st["total_norm"])
    assert st["total_norm"] > 0 and st["norm_max"] == st["total_norm"]
    return st["total_norm"]


@pytest.fixture(scope="module")
def first_norm():
    return _measured_norm()


# ---- not binding: nothing changes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp16_static", "fp16_dynamic"])
def test_clipping_that_does_not_bind_changes_no_bit(mode):
    res = []
    for max_grad_norm in (1e30, None):
        enc, tr, img, tgt = _build("bf16" if mode == "bf16" else "fp16")
        eng = enc.engine
        opt, scaler = _optimizer(tr, mode, max_grad_norm)
        assert eng.grad_clip_enabled == (max_grad_norm is not None)
        for _ in range(3):
            _train_step(tr, opt, scaler, img, tgt)
        assert eng.adam_step == 3
        if max_grad_norm is not None:
            st = opt.clip_stats()
            assert st["coef"] == 1.0 and st["clipped_steps"] == 0 and st["nonfinite_steps"] == 0
            assert 0 < st["total_norm"] <= st["norm_max"] < float("inf")
        else:
            assert eng._clip is None
        assert eng._step_plan.packed_version == eng.weights_version()
        enc.train()
        with torch.no_grad():
            e_train = enc(img.cuda()).cpu()                                 # what the train plan's packed weights compute
        res.append([t.clone().cpu() for t in (eng.params, eng.adam_m, eng.adam_v)] + [e_train])
    for what, a, b in zip(("parameters", "adam_m", "adam_v", "packed weights (train embeddings)"), *res):
        assert torch.equal(_bits(a), _bits(b)), "%s: %s differ, max |diff| %.3e" % (mode, what, float((a - b).abs().max()))


# ---- binding: AdamW on coef x the eager gradients of a twin -----------------------------------------------------------------------
def _binding_case(arch, norm, lazy=True, per_element=True):
    """lazy: the step of models.util.step() (norm over the scratch + the small ranges), its gradients taken from a twin engine
    with the same seed that ran the plain backward; else the engine's own plain backward, whose flat buffer the step then reads."""
    max_norm = 0.5 * norm
    enc, tr, img, tgt = _build(arch=arch)
    eng = enc.engine
    p0 = eng.params.clone().cpu()
    opt, scaler = tr.get_optimizer(LR, max_grad_norm=max_norm)
    if lazy:
        _train_step(tr, opt, scaler, img, tgt)
        enc2, tr2, _, _ = _build(arch=arch)
        enc2.train()
        tr2._forward_loss(img, tgt, train=True).backward()
        torch.cuda.synchronize()
        g = enc2.engine.grads.clone().cpu()
        assert torch.equal(_bits(p0), _bits(enc2.engine.params.cpu()))
    else:
        enc.train()
        tr._forward_loss(img, tgt, train=True).backward()
        g = eng.grads.clone().cpu()
        opt.step()
        torch.cuda.synchronize()
    st = opt.clip_stats()
    ref = R.clip_ref([g.numpy()], max_norm)
    print("%s: norm %.9g (float64 over the flat gradients: %.9g), coef %.9g (reference %.9g)" % (arch, st["total_norm"], ref["norm"], st["coef"], ref["coef"]))
    assert abs(st["total_norm"] - float(ref["total_norm_f32"])) <= R.ulp32(ref["norm"])
    assert abs(st["coef"] - float(ref["coef_f32"])) <= R.ulp32(ref["coef"]) and st["coef"] < 1.0
    assert st["clipped_steps"] == 1 and st["nonfinite_steps"] == 0 and eng.adam_step == 1
    if not per_element:
        return
    zero = torch.zeros_like(p0)
    want = P.adamw_ref(p0, g, zero, zero, step=1, gscale=ref["coef"], **HYP)
    bound = list(P.adamw_bounds(p0, g, zero, zero, step=1, gscale=ref["coef"], **HYP))
    # the gradient factor is off by at most G_REL relative: what that moves the reference by, to first order from both sides
    moved = [P.adamw_ref(p0, g, zero, zero, step=1, gscale=ref["coef"] * s, **HYP) for s in (1.0 + G_REL, 1.0 - G_REL)]
    free = P.adamw_ref(p0, g, zero, zero, step=1, gscale=1.0, **HYP)
    for i, (what, got) in enumerate((("parameters", eng.params), ("adam_m", eng.adam_m), ("adam_v", eng.adam_v))):
        bd = bound[i] + 1.25 * torch.maximum((moved[0][i] - want[i]).abs(), (moved[1][i] - want[i]).abs())
        err = (got.cpu().double() - want[i]).abs()
        worst = float((err / bd).max())
        print("%s: binding step, %s: largest error / bound %.3f" % (arch, what, worst))
        assert not bool((err > bd).any()), "%s: %d of %d outside their bound, worst %.3f" % (what, int((err > bd).sum()), err.numel(), worst)
        # ... and the step is not the unclipped one.  (Adam's first update is lr * g / (|g| + eps): the coefficient shows in the
        # parameters only where |g| is near eps, in the first moment wherever g is not zero.)
        off = int(((got.cpu().double() - free[i]).abs() > bd).sum())
        print("%s: %s: %d of %d elements tell the clipped step from the unclipped one" % (arch, what, off, err.numel()))
        assert off > (0 if i == 0 else err.numel() // 10)


def test_binding_step_equals_adamw_on_the_clipped_gradients(first_norm):
    _binding_case("resnet18", first_norm)


def test_binding_step_on_a_bottleneck_student():
    """ResNet-50: more plain ranges than one launch of the norm pass takes, and the 1x1 weight gradients in the scratch.
    The lazy step's norm and coefficient against the float64 norm of a twin's flat gradients; the per-element AdamW check from
    the engine's OWN plain backward.  A twin cannot serve there: this student's 1x1 weight gradients of layer1 are summed with
    atomics, so their last bits differ from run to run -- measured on three identical engines, 1,325 to 1,879 of 23,602,592
    gradient elements differ in bits (up to 1.1e-4 relative), where ResNet-18's 11,221,920 are the same bits every time -- and 7
    first moments of a lazy step sat 1.1 to 8.7 bounds from a twin's.  No bound on AdamW's arithmetic covers another run's
    gradient; the norm does not see it (below 1e-9 relative)."""
    norm = _measured_norm("resnet50")
    _binding_case("resnet50", norm, lazy=True, per_element=False)
    _binding_case("resnet50", norm, lazy=False)


# ---- the same multiset in another order ------------------------------------------------------------------------------------------
def test_norm_over_scratch_equals_norm_over_the_flat_buffer(first_norm):
    enc, tr, img, tgt = _build()
    opt, _ = tr.get_optimizer(LR, max_grad_norm=float("inf"))
    enc.train()
    tr._forward_loss(img, tgt, train=True).backward()                       # eager: the step reads the completed flat buffer
    eng = enc.engine
    assert not eng.L.vpd_plan_grads_pending(eng._step_plan.handle)
    g = eng.grads.clone().cpu()
    opt.step()
    torch.cuda.synchronize()
    eager = opt.clip_stats()["total_norm"]
    ref = R.clip_ref([g.numpy()], float("inf"))
    print("norm: lazy %.9g, eager %.9g, float64 %.9g" % (first_norm, eager, ref["norm"]))
    assert abs(eager - float(ref["total_norm_f32"])) <= R.ulp32(ref["norm"])
    assert abs(first_norm - eager) <= R.ulp32(eager)


# ---- a non-finite norm: skipped, counted, nothing written -------------------------------------------------------------------------
def _snapshot(eng):
    return [t.clone() for t in (eng.params, eng.adam_m, eng.adam_v, eng.ema_params, eng.ema_bn_running)]


def _poisoned(tgt):
    bad = tgt.clone()
    bad[1, 3] = float("inf")
    return bad


def test_fp16_dynamic_scaler_with_clipping_skips_on_the_device(monkeypatch, first_norm):
    from vpd_amd.models.util import DynamicLossScaler
    enc, tr, img, tgt = _build("fp16", ema_decay=0.5)
    eng = enc.engine
    opt = tr.get_optimizer(LR, max_grad_norm=1e-3 * first_norm)[0]      # (binds whatever fp16's rounding does to the norm)
    sc = DynamicLossScaler(eng, init_scale=256, growth_interval=10 ** 6)

    def no_search(*a):
        raise AssertionError("the non-finite search was launched although the norm pass covers it")
    monkeypatch.setattr(eng.L, "vpd_plan_check_grads", no_search)
    monkeypatch.setattr(eng.L, "vpd_op_check_finite", no_search)
    _train_step(tr, opt, sc, img, tgt)
    assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps) == (256.0, 0, 1)
    st = opt.clip_stats()
    assert st["clipped_steps"] == 1 and st["nonfinite_steps"] == 0 and 0 < st["total_norm"] < float("inf")
    assert 1e-2 * first_norm < st["total_norm"] < 1e2 * first_norm            # un-scaled: the size of the bf16 run's, not 256 x it
    kept = _snapshot(eng)
    _train_step(tr, opt, sc, img, _poisoned(tgt))
    for what, a, b in zip(("parameters", "adam_m", "adam_v", "ema_params", "ema_bn_running"), kept, _snapshot(eng)):
        assert torch.equal(_bits(a), _bits(b)), what
    assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps) == (128.0, 1, 1)
    st = opt.clip_stats()
    assert st["nonfinite_steps"] == 1 and st["clipped_steps"] == 1 and not np.isfinite(st["total_norm"])
    _train_step(tr, opt, sc, img, tgt)                                       # the next clean step applies
    assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps) == (128.0, 1, 2) and eng.adam_step == 2
    assert not torch.equal(eng.params, kept[0]) and not torch.equal(eng.ema_params, kept[3])
    assert bool(torch.isfinite(eng.params).all()) and opt.clip_stats()["clipped_steps"] == 2


def test_bf16_static_with_clipping_skips_and_counts(first_norm):
    enc, tr, img, tgt = _build(ema_decay=0.5)
    eng = enc.engine
    opt, scaler = tr.get_optimizer(LR, max_grad_norm=1e-3 * first_norm)
    assert scaler is None
    _train_step(tr, opt, scaler, img, tgt)
    assert eng.adam_step == 1
    kept = _snapshot(eng)
    _train_step(tr, opt, scaler, img, _poisoned(tgt))
    for what, a, b in zip(("parameters", "adam_m", "adam_v", "ema_params", "ema_bn_running"), kept, _snapshot(eng)):
        assert torch.equal(_bits(a), _bits(b)), what
    st = opt.clip_stats()
    assert st["nonfinite_steps"] == 1 and st["clipped_steps"] == 1
    assert eng.adam_step == 1 and int(eng._clip[4]) == 1                     # not advanced; the block counts the skipped step
    _train_step(tr, opt, scaler, img, tgt)
    assert eng.adam_step == 2 and bool(torch.isfinite(eng.params).all())
    assert not torch.equal(eng.params, kept[0]) and not torch.equal(eng.ema_params, kept[3])


# ---- an optimizer without the motion head -----------------------------------------------------------------------------------------
def test_norm_covers_only_what_the_optimizer_updates():
    from vpd_amd.trainer import FusedAdamW
    enc, tr, img, tgt = _build(motion=True)
    eng = enc.engine
    opt = FusedAdamW(list(enc.parameters()), eng, lr=LR, max_grad_norm=float("inf"))
    dec0 = eng.params[eng.encoder_numel:].clone()
    _train_step(tr, opt, None, img, tgt)
    g = eng.grads.clone().cpu()                                               # (still the step's: nothing zeroes the buffer)
    ne = eng.encoder_numel
    ref = R.clip_ref([g[:ne].numpy()], float("inf"))
    whole = R.clip_ref([g.numpy()], float("inf"))
    st = opt.clip_stats()
    print("norm: %.9g, encoder only %.9g, with the motion head %.9g" % (st["total_norm"], ref["norm"], whole["norm"]))
    assert whole["norm"] - ref["norm"] > 8 * R.ulp32(ref["norm"])             # the head's gradients would show
    assert abs(st["total_norm"] - float(ref["total_norm_f32"])) <= R.ulp32(ref["norm"])
    assert torch.equal(eng.params[ne:], dec0)                                 # the head was not updated either


# ---- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [True, False], ids=["with_flag", "without_flag"])
def test_train_cli_reports_the_norm_only_with_the_flag(tmp_path, flag):
    out = str(tmp_path / "run")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_vpd_model.py"), "diving48", "--save_dir", out, "--synthetic", "64",
                        "--num_epochs", "1", "--batch_size", "16", "--encoder_arch", "resnet18"]
                       + (["--clip_grad_norm", "1.0"] if flag else []), cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = json.load(open(os.path.join(out, "loss.json")))
    cfg = json.load(open(os.path.join(out, "config.json")))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Epoch ")][0]
    if flag:
        assert np.isfinite(losses[0]["grad_norm_max"]) and losses[0]["grad_norm_max"] > 0
        assert 0 <= losses[0]["clipped_steps"] <= 4 and cfg["clip_grad_norm"] == 1.0
        assert "grad_norm_max:" in line and "clipped_steps:" in line
    else:
        assert "grad_norm_max" not in losses[0] and "clipped_steps" not in losses[0] and "clip_grad_norm" not in cfg
        assert "grad_norm_max" not in line and "clipped_steps" not in line
