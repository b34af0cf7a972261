"""Exponential moving average of the student's weights, end to end (StudentEngine.enable_ema / use_ema, ModelTrainer(ema_decay=),
ema_weights(), ema_state_dict(), train_vpd_model.py --ema_decay, apply_vpd_model.py --ema) on the smallest shapes: ResNet-18,
3 channels, 64 x 64, 6 crops, D = 32.  The average is held to the derived running-error bound of tests/opref_ema.py against a
float64 replay from the live parameters; everything that should not move is held to equality of bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vpd_oracle as O
from tests import opref_ema as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH, C_IN, D, N, HW, LR = "resnet18", 3, 32, 6, 64, 5e-4


def _bits(t):
    return t.contiguous().view(torch.int32)


def _build(dtype="bf16", motion=True, seed=50, **ema):
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    enc = RGBF_EmbeddingModel(ARCH, D, False, "cuda", dtype=dtype)
    enc.load_state_dict(O.procedural_state_dict(O.encoder_schema(ARCH, C_IN, D), seed))
    tr = ModelTrainer(enc, motion, **ema)
    if motion:
        tr.fcn_time.load_state_dict(O.procedural_state_dict(O.decoder_schema(D), seed + 7))
    img = O.synthetic_crops(N, C_IN, HW, seed + 1)
    tgt = O.synthetic_targets(N, D, motion, seed + 2)
    return enc, tr, img, tgt


def _train_step(tr, opt, scaler, img, tgt):
    from vpd_amd.models.util import step
    tr.encoder.train()
    if hasattr(tr, "fcn_time"):
        tr.fcn_time.train()
    step(opt, scaler, tr._forward_loss(img, tgt, train=True))
    torch.cuda.synchronize()


def _live(eng):
    return torch.cat([eng.params, eng.bn_running[:eng.bn_numel]]).cpu()


def _avg(eng):
    return torch.cat([eng.ema_params, eng.ema_bn_running[:eng.bn_numel]]).cpu()


def _assert_within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    out = err > bound
    worst = float((err / bound).max())
    print("%s: largest error / bound %.3f" % (what, worst))
    assert not bool(out.any()), "%s: %d of %d elements outside their bound, worst %.3f" % (what, int(out.sum()), out.numel(), worst)


def test_three_fused_steps_stay_within_the_running_error_bound():
    enc, tr, img, tgt = _build(ema_decay=0.5)
    eng = enc.engine
    assert not eng.ema_enabled                                              # averaging starts with the optimizer ...
    opt, scaler = tr.get_optimizer(LR)
    assert eng.ema_enabled and scaler is None
    start = _live(eng)
    assert torch.equal(_bits(_avg(eng)), _bits(start))                      # ... from copies of the live buffers
    ref, bound = start.double(), torch.zeros(start.numel(), dtype=torch.float64)
    for k in range(3):
        _train_step(tr, opt, scaler, img, tgt)
        live = _live(eng)
        bound = E.ema_bound_step(bound, ref, live, 0.5)
        ref = E.ema_ref(ref, live, 0.5)
        _assert_within(_avg(eng), ref, bound, "step %d" % (k + 1))
    assert eng._ema_t == 3
    moved = (_avg(eng) - start).abs()
    assert float(moved[:eng.param_numel].max()) > 1e-5 and float(moved[eng.param_numel:].max()) > 1e-5
    assert not torch.equal(_avg(eng), _live(eng))


def test_ema_weights_context_serves_the_average_and_restores_the_live_weights():
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    enc, tr, img, tgt = _build(ema_decay=0.5)
    eng = enc.engine
    opt, scaler = tr.get_optimizer(LR)
    for _ in range(2):
        _train_step(tr, opt, scaler, img, tgt)
    x = img.numpy()
    before = enc.embed(x)
    kept = [t.clone() for t in (eng.params, eng.bn_running, eng.adam_m, eng.adam_v, eng.num_batches_tracked)]
    with tr.ema_weights() as same:
        assert same is tr
        inside = enc.embed(x)
        again = enc.embed(x)
        enc.train()
        with pytest.raises(RuntimeError, match="use_ema"):
            with torch.no_grad():
                enc(img.cuda())
        enc.eval()
    fresh = RGBF_EmbeddingModel(ARCH, D, False, "cuda")
    sd = enc.ema_state_dict()
    assert list(sd.keys()) == list(enc.state_dict().keys())
    assert all(sd[k].shape == v.shape and sd[k].dtype == v.dtype for k, v in enc.state_dict().items())
    fresh.load_state_dict(sd)
    assert np.array_equal(inside.view(np.int32), fresh.embed(x).view(np.int32))
    assert np.array_equal(inside.view(np.int32), again.view(np.int32))
    assert not np.array_equal(inside, before)
    after = enc.embed(x)
    assert np.array_equal(after.view(np.int32), before.view(np.int32))
    for a, b in zip(kept, (eng.params, eng.bn_running, eng.adam_m, eng.adam_v, eng.num_batches_tracked)):
        assert torch.equal(a, b)
    # the motion head's average, and num_batches_tracked the live one
    dsd = tr.fcn_time.ema_state_dict()
    assert list(dsd.keys()) == list(tr.fcn_time.state_dict().keys())
    assert torch.equal(dsd["layers.0.weight"], eng.view("decoder.layers.0.weight", eng.ema_params))
    live_sd = enc.state_dict()
    assert all(torch.equal(sd[k], live_sd[k]) for k in sd if k.endswith("num_batches_tracked"))
    assert not torch.equal(sd["resnet.bn1.running_mean"], live_sd["resnet.bn1.running_mean"])
    # the manual call counts like the automatic one
    eng.ema_update()
    assert eng._ema_t == 3
    with pytest.raises(RuntimeError):
        _build(motion=False)[0].engine.use_ema(True)                        # never enabled


def _set_scale(scaler, value):
    scaler.state[:1] = torch.tensor([value], dtype=torch.float32).view(torch.int32).cuda()


def test_fp16_dynamic_scaler_skipped_step_leaves_the_average_alone():
    """clean step, a step whose target holds an inf (skipped on the device), clean step -- against a twin that never saw the
    poisoned batch (its scale is halved by hand where the first run's scaler backed off, so both run the same arithmetic).
    BatchNorm running statistics: the poisoned FORWARD updates the live ones, as the reference's does, so after it only their
    average across the skipped step is held to bits, and the float64 replay to the bound afterwards."""
    from vpd_amd.models.util import DynamicLossScaler
    decay = 0.9
    runs = []
    for poisoned in (True, False):
        enc, tr, img, tgt = _build("fp16", ema_decay=decay, ema_warmup=True)
        eng = enc.engine
        opt = tr.get_optimizer(LR)[0]
        sc = DynamicLossScaler(eng, init_scale=256, growth_interval=10 ** 6)
        start = _live(eng)
        _train_step(tr, opt, sc, img, tgt)
        live1 = _live(eng)
        avg1 = _avg(eng)
        if poisoned:
            bad = tgt.clone()
            bad[1, 3] = float("inf")
            _train_step(tr, opt, sc, img, bad)
            assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps) == (128.0, 1, 1)
            assert torch.equal(_bits(_live(eng))[:eng.param_numel], _bits(live1)[:eng.param_numel])
            assert torch.equal(_bits(_avg(eng)), _bits(avg1)), "the average moved across a skipped step"
        else:
            _set_scale(sc, 128.0)
        _train_step(tr, opt, sc, img, tgt)
        assert sc.applied_steps == 2 and eng.adam_step == 2
        runs.append((start, live1, avg1, _live(eng), _avg(eng), eng.param_numel))
    (start, live1, avg1, live2, avg2, npar), twin = runs
    assert torch.equal(_bits(start), _bits(twin[0])) and torch.equal(_bits(avg1), _bits(twin[2]))
    assert torch.equal(_bits(live2)[:npar], _bits(twin[3])[:npar])          # training itself is the twin's
    assert torch.equal(_bits(avg2)[:npar], _bits(twin[4])[:npar]), "the average after the skipped step is not the twin's"
    # t is the number of APPLIED steps (second update: t = 1, d = 2/11), not the number of calls (t = 2, d = 1/4)
    bound = E.ema_bound_step(torch.zeros(start.numel(), dtype=torch.float64), start.double(), live1, decay, True, 0)
    ref = E.ema_ref(start, live1, decay, True, 0)
    _assert_within(avg1, ref, bound, "fp16 update 1")
    by_calls = E.ema_ref(ref, live2, decay, True, 2)
    bound = E.ema_bound_step(bound, ref, live2, decay, True, 1)
    ref = E.ema_ref(ref, live2, decay, True, 1)
    _assert_within(avg2, ref, bound, "fp16 update 2 (t = applied steps)")
    assert int(((avg2.double() - by_calls).abs() > bound).sum()) > npar // 2


def test_averaging_does_not_perturb_training():
    """the same three steps with and without the average: live parameters, moments, running statistics and what the packed
    weights of both plans compute (train-mode and eval-mode embeddings) agree in bits"""
    res = []
    for ema in (dict(ema_decay=0.5), {}):
        enc, tr, img, tgt = _build(motion=False, **ema)      # (no motion head: enc(x) below runs on the plan the steps packed)
        eng = enc.engine
        opt, scaler = tr.get_optimizer(LR)
        assert eng.ema_enabled == bool(ema)
        for _ in range(3):
            _train_step(tr, opt, scaler, img, tgt)
        pl = eng._step_plan
        assert pl.packed_version == eng.weights_version()                    # the fused step kept the train plan's packed weights fresh
        enc.train()
        with torch.no_grad():
            e_train = enc(img.cuda()).cpu()
        e_eval = torch.from_numpy(enc.embed(img.numpy()))
        res.append([t.clone().cpu() for t in (eng.params, eng.adam_m, eng.adam_v, eng.bn_running)] + [e_train, e_eval])
        assert eng.adam_step == 3
    for what, a, b in zip(("parameters", "adam_m", "adam_v", "bn_running", "train embeddings", "eval embeddings"), *res):
        assert torch.equal(_bits(a), _bits(b)), what


def test_train_cli_writes_the_averaged_checkpoints_and_apply_loads_them(tmp_path):
    out = str(tmp_path / "run")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_vpd_model.py"), "diving48", "--save_dir", out, "--synthetic", "64",
                        "--num_epochs", "2", "--batch_size", "16", "--ema_decay", "0.9", "--encoder_arch", "resnet18"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    files = set(os.listdir(out))
    assert {"best_epoch.encoder.pt", "best_epoch_ema.encoder.pt", "epoch0002.encoder.pt", "epoch0002_ema.encoder.pt",
            "loss.json", "config.json"} <= files, files
    assert not any(f.endswith(".decoder.pt") for f in files)                 # (no --motion)
    losses = json.load(open(os.path.join(out, "loss.json")))
    assert len(losses) == 2 and all(np.isfinite(l["val_ema"]) and np.isfinite(l["val"]) for l in losses)
    cfg = json.load(open(os.path.join(out, "config.json")))
    assert cfg["ema_decay"] == 0.9 and cfg["ema_warmup"] is False
    import apply_vpd_model
    name = apply_vpd_model.checkpoint_name(None, True)
    enc = apply_vpd_model.load_encoder(out, name, cfg["encoder_arch"], cfg["emb_dim"], cfg["use_flow"], "cuda")
    live = torch.load(os.path.join(out, "epoch0002.encoder.pt"), map_location="cpu")
    avg = torch.load(os.path.join(out, "epoch0002_ema.encoder.pt"), map_location="cpu")
    assert list(avg.keys()) == list(live.keys())
    assert not torch.equal(avg["resnet.conv1.weight"], live["resnet.conv1.weight"])
    assert torch.equal(avg["resnet.bn1.num_batches_tracked"], live["resnet.bn1.num_batches_tracked"])
    emb = enc.embed(O.synthetic_crops(2, 3, cfg["img_dim"], 9).numpy())
    assert emb.shape == (2, cfg["emb_dim"]) and np.isfinite(emb).all()
