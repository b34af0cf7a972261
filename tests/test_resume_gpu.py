"""Resumable training end to end (ModelTrainer.save_state / load_state, FusedAdamW / LossScaler / DynamicLossScaler state_dict,
StudentEngine.ema_state / clip_state, train_vpd_model.py --state_frequency / --resume / --seed) on the smallest shapes: ResNet-18,
3 channels, 64 x 64, 6 crops, D = 32.  The yardstick is equality of bits: four optimizer steps in one go against two steps, a
file, a FRESH model / trainer / optimizer / scaler (other initial weights), and two more steps.  Every step has its own batch, so
a wrong step count or a lost moment shows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vpd_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH, C_IN, D, N, HW, LR = "resnet18", 3, 32, 6, 64, 5e-4
SEED = 70
_BATCHES = {}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _batch(k, motion):
    """the batch of micro-step k (computed once, never changed)"""
    if (k, motion) not in _BATCHES:
        _BATCHES[(k, motion)] = (O.synthetic_crops(N, C_IN, HW, SEED + 100 + k), O.synthetic_targets(N, D, motion, SEED + 200 + k))
    return _BATCHES[(k, motion)]


CONFIGS = {
    "a_bf16": dict(),
    "b_bf16_motion_ema_groups_clip": dict(motion=True, ema=dict(ema_decay=0.5, ema_warmup=True), groups=True, clip=True),
    "c_fp16_static": dict(dtype="fp16"),
    "d_fp16_dynamic_ema_clip_skip_at_2": dict(dtype="fp16", dynamic=True, ema=dict(ema_decay=0.5, ema_warmup=True), clip=True, poison=1),
    # (not in the issue's list: the overflow one step earlier, so that the growth tracker is mid-count at the save and the scale
    #  grows at step 4 -- a lost tracker changes the scale)
    "d_fp16_dynamic_ema_clip_skip_at_1": dict(dtype="fp16", dynamic=True, ema=dict(ema_decay=0.5, ema_warmup=True), clip=True, poison=0),
    "e_bf16_accum2": dict(accum=2),
}


def _make(cfg, seed=SEED, max_grad_norm=None, arch=ARCH):
    """model, trainer, optimizer, scaler of a configuration, from the procedural weights of `seed`"""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import DynamicLossScaler
    from vpd_amd.trainer import ModelTrainer
    motion = cfg.get("motion", False)
    enc = RGBF_EmbeddingModel(arch, D, False, "cuda", dtype=cfg.get("dtype", "bf16"))
    enc.load_state_dict(O.procedural_state_dict(O.encoder_schema(arch, C_IN, D), seed))
    tr = ModelTrainer(enc, motion, accum_steps=cfg.get("accum", 1), **cfg.get("ema", {}))
    if motion:
        tr.fcn_time.load_state_dict(O.procedural_state_dict(O.decoder_schema(D), seed + 7))
    groups = None
    if cfg.get("groups"):
        groups = tr.param_groups(weight_decay=0.05, decay_bn_bias=False, lr=LR)
        assert len(groups) == 2
        groups[1]["lr"] = 2 * LR                            # two groups, lr and weight_decay both different
    opt, sc = tr.get_optimizer(LR, max_grad_norm=max_grad_norm if cfg.get("clip") else None, param_groups=groups)
    if cfg.get("dynamic"):
        sc = DynamicLossScaler(enc.engine, init_scale=256, growth_interval=3)
    return enc, tr, opt, sc


def _steps(cfg, tr, opt, sc, first, last, norms=None):
    """optimizer steps first .. last-1 (each `accum` micro-batches, each micro-batch its own batch)"""
    from vpd_amd.models.util import step
    motion, accum = cfg.get("motion", False), cfg.get("accum", 1)
    tr.encoder.train()
    if motion:
        tr.fcn_time.train()
    for s in range(first, last):
        for j in range(accum):
            img, tgt = _batch(s * accum + j, motion)
            if cfg.get("poison") == s:
                tgt = tgt.clone()
                tgt[1, 3] = float("inf")
            step(opt, sc, tr._forward_loss(img, tgt, train=True), accumulate=j < accum - 1)
        if norms is not None:
            norms.append(opt.clip_stats()["total_norm"])
    torch.cuda.synchronize()


def _snapshot(cfg, enc, opt, sc):
    eng = enc.engine
    t = dict(params=eng.params, bn_running=eng.bn_running, num_batches_tracked=eng.num_batches_tracked, adam_m=eng.adam_m,
             adam_v=eng.adam_v)
    n = dict(adam_step=eng.adam_step)
    if eng.ema_enabled:
        t.update(ema_params=eng.ema_params, ema_bn_running=eng.ema_bn_running)
        n["num_updates"] = eng.ema_state()["num_updates"]
    if cfg.get("dynamic"):
        n["scaler"] = (sc.get_scale(), sc.growth_tracker, sc.applied_steps, sc.skipped_steps)
    elif sc is not None:
        n["scaler"] = sc.get_scale()
    if cfg.get("clip"):
        n["clip"] = opt.clip_stats()
    t = {k: v.detach().clone().cpu() for k, v in t.items()}
    t["embed"] = torch.from_numpy(enc.embed(_batch(0, False)[0].numpy()))
    return t, n


def _assert_same(got, ref, what):
    (gt, gn), (rt, rn) = got, ref
    assert set(gt) == set(rt) and set(gn) == set(rn)
    for k in rt:
        same = torch.equal(_bits(gt[k]) if gt[k].dtype == torch.float32 else gt[k], _bits(rt[k]) if rt[k].dtype == torch.float32 else rt[k])
        assert same, "%s: %s differs (%d of %d elements)" % (what, k, int((gt[k] != rt[k]).sum()), rt[k].numel())
    for k in rn:
        assert gn[k] == rn[k], "%s: %s is %r, the straight run's %r" % (what, k, gn[k], rn[k])


def _max_norm_that_always_binds(cfg):
    """half the smallest of the four steps' gradient norms, from a measuring run (max_norm = +inf); printed"""
    enc, tr, opt, sc = _make(cfg, max_grad_norm=float("inf"))
    norms = []
    _steps(cfg, tr, opt, sc, 0, 4, norms)
    finite = [x for x in norms if np.isfinite(x)]
    print("gradient norms of the measuring run:", norms)
    assert len(finite) >= 3 and min(finite) > 0
    return 0.5 * min(finite)


def test_precondition_two_fresh_trainers_agree_in_bits():
    """what the continuation tests stand on; a failure here is a finding about the step, not about the checkpoint"""
    cfg = CONFIGS["a_bf16"]
    snaps = []
    for _ in range(2):
        enc, tr, opt, sc = _make(cfg)
        _steps(cfg, tr, opt, sc, 0, 4)
        snaps.append(_snapshot(cfg, enc, opt, sc))
    _assert_same(snaps[1], snaps[0], "second fresh trainer")
    assert snaps[0][1]["adam_step"] == 4


@pytest.mark.parametrize("name", list(CONFIGS))
def test_two_steps_save_load_two_steps_equals_four_steps_in_bits(name, tmp_path):
    cfg = CONFIGS[name]
    max_norm = _max_norm_that_always_binds(cfg) if cfg.get("clip") else None
    enc, tr, opt, sc = _make(cfg, max_grad_norm=max_norm)
    _steps(cfg, tr, opt, sc, 0, 4)
    straight = _snapshot(cfg, enc, opt, sc)
    if cfg.get("clip"):
        st = straight[1]["clip"]
        print("clip statistics of the straight run:", st)
        assert st["clipped_steps"] == (3 if cfg.get("dynamic") else 4), st          # every step with a finite norm clips
    # two steps, the file, everything fresh (other initial weights), two more steps
    enc, tr, opt, sc = _make(cfg, max_grad_norm=max_norm)
    _steps(cfg, tr, opt, sc, 0, 2)
    if cfg.get("dynamic"):      # one step skipped, the scale halved, applied != calls
        assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps) == (128.0, 1, 1)
        assert sc.growth_tracker == (0 if cfg["poison"] == 1 else 1)
        assert enc.engine.adam_step == 1
    path = str(tmp_path / "train_state.pt")
    tr.save_state(path, opt, sc, extra={"epoch": 2, "note": "x"})
    assert sorted(os.listdir(tmp_path)) == ["train_state.pt"]
    torch.load(path, map_location="cpu", weights_only=True)
    del enc, tr, opt, sc
    enc, tr, opt, sc = _make(cfg, seed=SEED + 1, max_grad_norm=max_norm)
    if cfg.get("groups"):      # what the file holds wins over what the fresh optimizer was built with, as in torch
        opt.param_groups[0]["lr"] = 123.0
    extra = tr.load_state(path, opt, sc)
    assert extra == {"epoch": 2, "note": "x"}
    _steps(cfg, tr, opt, sc, 2, 4)
    _assert_same(_snapshot(cfg, enc, opt, sc), straight, name)
    if cfg.get("dynamic") and cfg["poison"] == 0:
        assert straight[1]["scaler"][0] == 256.0             # grew at step 4: the tracker was carried over


def test_weights_alone_do_not_reproduce_the_run():
    """sensitivity: the same split with the encoder's state_dict only and a fresh optimizer ends elsewhere"""
    cfg = CONFIGS["a_bf16"]
    enc, tr, opt, sc = _make(cfg)
    _steps(cfg, tr, opt, sc, 0, 4)
    straight = _snapshot(cfg, enc, opt, sc)
    enc, tr, opt, sc = _make(cfg)
    _steps(cfg, tr, opt, sc, 0, 2)
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    enc, tr, opt, sc = _make(cfg, seed=SEED + 1)
    enc.load_state_dict(sd)
    _steps(cfg, tr, opt, sc, 2, 4)
    got = _snapshot(cfg, enc, opt, sc)
    assert torch.equal(got[0]["num_batches_tracked"], straight[0]["num_batches_tracked"])
    assert not torch.equal(_bits(got[0]["params"]), _bits(straight[0]["params"]))
    assert not torch.equal(_bits(got[0]["adam_m"]), _bits(straight[0]["adam_m"]))
    assert got[1]["adam_step"] == 2


def test_fused_state_loads_into_torch_adamw():
    cfg = CONFIGS["a_bf16"]
    enc, tr, opt, sc = _make(cfg)
    eng = enc.engine
    assert opt.state_dict()["state"] == {}                   # before the first step, as torch's
    _steps(cfg, tr, opt, sc, 0, 2)
    sd = opt.state_dict()
    params = list(enc.parameters())
    assert len(sd["state"]) == len(params) == len(eng.enc_names)
    topt = torch.optim.AdamW(params, lr=1.0)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]["lr"] == LR and topt.param_groups[0]["weight_decay"] == 0.01
    for name, p in zip(eng.enc_names, params):
        s = topt.state[p]
        assert float(s["step"]) == 2.0
        assert s["exp_avg"].shape == p.shape
        assert torch.equal(_bits(s["exp_avg"]), _bits(eng.view(name, eng.adam_m))), name
        assert torch.equal(_bits(s["exp_avg_sq"]), _bits(eng.view(name, eng.adam_v))), name
    # the dictionary's tensors are views of the engine's buffers
    assert sd["state"][0]["exp_avg"].data_ptr() == eng.adam_m.data_ptr()
    assert sd["state"][0]["step"].dtype == torch.float32 and sd["state"][0]["step"].shape == ()


def test_torch_adamw_state_loads_into_the_fused_optimizer_and_both_step_alike():
    from vpd_amd.models.util import step
    from vpd_amd.trainer import FusedAdamW
    cfg = CONFIGS["a_bf16"]
    enc, tr, _, _ = _make(cfg)
    eng = enc.engine
    params = list(enc.parameters())
    topt = torch.optim.AdamW(params, lr=LR)
    enc.train()
    for k in range(2):      # (a torch optimizer gets the plain backward: every p.grad is complete)
        img, tgt = _batch(k, False)
        step(topt, None, tr._forward_loss(img, tgt, train=True))
    torch.cuda.synchronize()
    fopt = FusedAdamW(params, eng, lr=1.0)
    fopt.load_state_dict(topt.state_dict())
    assert eng.adam_step == 2 and fopt.param_groups[0]["lr"] == LR
    for name, p in zip(eng.enc_names, params):
        assert torch.equal(_bits(eng.view(name, eng.adam_m)), _bits(topt.state[p]["exp_avg"])), name
        assert torch.equal(_bits(eng.view(name, eng.adam_v)), _bits(topt.state[p]["exp_avg_sq"])), name
    # one identical injected gradient through both: torch first, then the fused kernel from the same starting point
    g = torch.Generator(device="cuda").manual_seed(5)
    grads = eng.grads
    grads.zero_()
    for name in eng.enc_names:
        v = eng.view(name, grads)
        v.copy_(torch.randn(v.shape, device="cuda", generator=g) * 1e-2)
    tr._reattach_grads()
    start = eng.params.clone()
    topt.step()
    by_torch = eng.params.clone()
    with torch.no_grad():
        eng.params.copy_(start)
    eng.mark_weights_changed()
    fopt.step()
    torch.cuda.synchronize()
    assert eng.adam_step == 3
    ne = eng.encoder_numel
    moved = float((by_torch[:ne] - start[:ne]).abs().max())
    err = float((eng.params[:ne] - by_torch[:ne]).abs().max())
    print("injected gradient: largest move %.3e, largest |fused - torch| %.3e" % (moved, err))
    assert moved > 1e-4 and err <= 1e-6


def test_refusals(tmp_path):
    from vpd_amd.models.util import step
    cfg = dict(ema=dict(ema_decay=0.5), accum=2)
    enc, tr, opt, sc = _make(cfg)
    img, tgt = _batch(0, False)
    enc.train()
    path = str(tmp_path / "train_state.pt")
    step(opt, sc, tr._forward_loss(img, tgt, train=True), accumulate=True)
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.save_state(path, opt, sc)
    step(opt, sc, tr._forward_loss(img, tgt, train=True))
    with tr.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.save_state(path, opt, sc)
    with pytest.raises(TypeError, match="FusedAdamW"):
        tr.save_state(path, torch.optim.AdamW(list(enc.parameters()), lr=LR), sc)
    assert not os.path.exists(path)
    tr.save_state(path, opt, sc)
    kept = enc.engine.params.clone()

    def refused(match, cfg2, **kw):
        enc2, tr2, opt2, sc2 = _make(cfg2, seed=SEED + 1, **kw)
        before = enc2.engine.params.clone()
        with pytest.raises(ValueError, match=match):
            tr2.load_state(path, opt2, sc2)
        assert torch.equal(before, enc2.engine.params)       # refused before anything was written
    refused("EMA", dict(accum=2))                            # a file with the average into a trainer without
    refused("arch differs .*resnet18.*resnet34", cfg, arch="resnet34")
    refused("dtype differs .*bf16.*fp16", dict(cfg, dtype="fp16"))
    refused("motion differs", dict(cfg, motion=True))
    refused("gradient clipping", dict(cfg, clip=True), max_grad_norm=1.0)
    refused("parameter groups", dict(cfg, groups=True))
    refused("EMA.*decay", dict(cfg, ema=dict(ema_decay=0.9)))
    assert torch.equal(kept, enc.engine.params)


COMMON = ["diving48", "--synthetic", "64", "--batch_size", "16", "--encoder_arch", "resnet18", "--seed", "7", "--state_frequency", "1",
          "--ema_decay", "0.9"]


def _cli(save_dir, *more):
    return subprocess.run([sys.executable, os.path.join(ROOT, "train_vpd_model.py")] + COMMON + ["--save_dir", save_dir] + list(more),
                          cwd=ROOT, capture_output=True, text=True, timeout=900)


def test_train_cli_resumed_run_equals_the_uninterrupted_one(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for r in (_cli(a, "--num_epochs", "4"), _cli(b, "--num_epochs", "2"), _cli(b, "--resume", "--num_epochs", "4")):
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Resuming after epoch 2" in r.stdout
    for name in ("epoch0004.encoder.pt", "epoch0004_ema.encoder.pt", "best_epoch.encoder.pt"):
        sa = torch.load(os.path.join(a, name), map_location="cpu")
        sb = torch.load(os.path.join(b, name), map_location="cpu")
        assert list(sa) == list(sb)
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k].view(torch.uint8).reshape(-1) if sa[k].dim() else sa[k],
                                                              sb[k].view(torch.uint8).reshape(-1) if sb[k].dim() else sb[k]), (name, k)
    la, lb = json.load(open(os.path.join(a, "loss.json"))), json.load(open(os.path.join(b, "loss.json")))
    assert len(la) == 4 and la == lb
    files = set(os.listdir(b))
    assert "train_state.pt" in files and not any(f.endswith(".tmp") for f in files)
    cfg = json.load(open(os.path.join(b, "config.json")))
    assert cfg["seed"] == 7 and cfg["state_frequency"] == 1 and cfg["num_epochs"] == 2
    state = torch.load(os.path.join(b, "train_state.pt"), map_location="cpu", weights_only=True)
    assert state["extra"]["epoch"] == 4 and state["extra"]["split_seed"] == 7 and len(state["extra"]["losses"]) == 4
    # nothing left: exit 0; without --resume the directory is refused exactly as before
    r = _cli(b, "--resume", "--num_epochs", "4")
    assert r.returncode == 0 and "Nothing left" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    r = _cli(b, "--num_epochs", "4")
    assert r.returncode != 0 and "FileExistsError" in r.stderr
