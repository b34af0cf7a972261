"""Resumable training, the part that needs no device (vpd_amd/checkpoint.py): the flat moments against a real torch.optim.AdamW,
the loss scaler's eight words against GradScaler's dictionary, the random number generators, the atomic file, the refusals the
command line makes before it touches a GPU, and the per-rank generator states on two gloo ranks."""
import copy
import os
import random
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from vpd_amd import checkpoint as K  # noqa: E402

# a layout in miniature, rows as StudentEngine.layout's (kind, is_decoder, offset, numel, shape), with floats between the tensors
LAYOUT = OrderedDict([("a.weight", (0, 0, 0, 6, (2, 3))), ("a.bias", (4, 0, 8, 5, (5,))), ("b.weight", (3, 1, 16, 4, (2, 2)))])
NUMEL = 20
NAMES = list(LAYOUT)
PADDING = [6, 7, 13, 14, 15]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _views(flat):
    return [flat[off:off + n].view(shape) for _, _, off, n, shape in LAYOUT.values()]


def _torch_adamw(steps=2, groups=None, seed=0):
    """torch.optim.AdamW over views of one flat buffer, `steps` steps on seeded gradients"""
    g = torch.Generator().manual_seed(seed)
    flat = torch.zeros(NUMEL)
    params = [torch.nn.Parameter(v) for v in _views(flat)]
    for p in params:
        p.data.copy_(torch.randn(p.shape, generator=g))
    if groups is None:
        opt = torch.optim.AdamW(params, lr=1e-2)
    else:
        opt = torch.optim.AdamW([dict(params=[params[i] for i in idx], **kw) for idx, kw in groups], lr=1e-2)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return flat, params, opt


def test_adamw_state_dict_to_flat_and_back_is_equal_in_bits():
    flat, params, opt = _torch_adamw(2, groups=[([0, 2], dict(weight_decay=0.1)), ([1], dict(lr=3e-3, weight_decay=0.0))])
    sd = opt.state_dict()
    order = [0, 2, 1]                                       # the optimizer's own order: group 0 holds tensors 0 and 2
    names = [NAMES[i] for i in order]
    m, v = torch.zeros(NUMEL), torch.zeros(NUMEL)
    assert K.adamw_load_flat(sd, LAYOUT, names, m, v) == 2
    # the flat moments are the exp_avg tensors at their offsets, zeros in between
    for i, name in enumerate(names):
        _, _, off, n, _ = LAYOUT[name]
        assert torch.equal(_bits(m[off:off + n]), _bits(sd["state"][i]["exp_avg"].reshape(-1)))
        assert torch.equal(_bits(v[off:off + n]), _bits(sd["state"][i]["exp_avg_sq"].reshape(-1)))
    assert float(m[PADDING].abs().max()) == 0.0 and float(v[PADDING].abs().max()) == 0.0
    assert float(m[[0, 8, 16]].abs().min()) > 0.0
    back = K.adamw_state_dict(LAYOUT, m, v, 2, names, opt.param_groups)
    assert set(back) == {"state", "param_groups"} and set(back["state"]) == set(sd["state"])
    for i in sd["state"]:
        a, b = sd["state"][i], back["state"][i]
        assert set(b) == {"step", "exp_avg", "exp_avg_sq"}
        assert b["step"].dtype == torch.float32 and b["step"].shape == () and float(b["step"]) == float(a["step"]) == 2.0
        for key in ("exp_avg", "exp_avg_sq"):
            assert b[key].shape == a[key].shape and torch.equal(_bits(b[key]), _bits(a[key]))
        # views of the flat buffers, as parameters are views of engine.params
        assert b["exp_avg"].data_ptr() == m.data_ptr() + 4 * LAYOUT[names[i]][2]
    for ga, gb in zip(sd["param_groups"], back["param_groups"]):
        assert gb["params"] == ga["params"]
        assert all(gb[k] == ga[k] for k in ("lr", "eps", "weight_decay")) and tuple(gb["betas"]) == tuple(ga["betas"])
    # ... which torch.optim.AdamW loads, and then steps exactly as the optimizer it came from
    flat2, params2, opt2 = _torch_adamw(0, groups=[([0, 2], dict(weight_decay=0.5)), ([1], dict(lr=1.0))])
    flat2.copy_(flat)
    opt2.load_state_dict(back)
    assert opt2.param_groups[0]["weight_decay"] == 0.1 and opt2.param_groups[1]["lr"] == 3e-3
    g = torch.Generator().manual_seed(9)
    for p, q in zip(params, params2):
        p.grad = torch.randn(p.shape, generator=g)
        q.grad = p.grad.clone()
    opt.step()
    opt2.step()
    assert torch.equal(_bits(flat), _bits(flat2))
    assert all(float(s["step"]) == 3.0 for s in opt2.state_dict()["state"].values())


def test_adamw_state_is_empty_before_the_first_step_and_loads_as_zero():
    flat, params, opt = _torch_adamw(0)
    assert opt.state_dict()["state"] == {}
    assert K.adamw_state_dict(LAYOUT, None, None, 0, NAMES, opt.param_groups)["state"] == {}
    assert K.adamw_state_dict(LAYOUT, torch.zeros(NUMEL), torch.zeros(NUMEL), 0, NAMES, opt.param_groups)["state"] == {}
    m, v = torch.ones(NUMEL), torch.ones(NUMEL)
    assert K.adamw_load_flat(opt.state_dict(), LAYOUT, NAMES, m, v) == 0
    assert float(m[[0, 8, 16]].abs().max()) == 0.0 and float(v[[0, 12, 19]].abs().max()) == 0.0


def test_adamw_load_refuses_and_writes_nothing():
    flat, params, opt = _torch_adamw(2)
    keep = torch.full((NUMEL,), 7.0)

    def refused(sd, match, names=NAMES):
        m, v = keep.clone(), keep.clone()
        with pytest.raises(ValueError, match=match):
            K.adamw_load_flat(sd, LAYOUT, names, m, v)
        assert torch.equal(m, keep) and torch.equal(v, keep)

    sd = copy.deepcopy(opt.state_dict())      # (torch hands out its own per-parameter dictionaries)
    sd["state"][1]["step"] = torch.tensor(3.0)
    refused(sd, "steps differ")
    sd = copy.deepcopy(opt.state_dict())
    del sd["state"][2]
    refused(sd, "no optimizer state for parameter b.weight")
    sd = copy.deepcopy(opt.state_dict())
    sd["state"][0]["exp_avg"] = torch.zeros(3, 2)
    refused(sd, r"exp_avg of parameter a.weight has shape \(3, 2\)")
    sd = opt.state_dict()
    refused(sd, "this optimizer has 2", names=NAMES[:2])
    _, _, opt2 = _torch_adamw(2, groups=[([0, 1], dict(betas=(0.9, 0.999))), ([2], dict(betas=(0.8, 0.999)))])
    refused(opt2.state_dict(), "betas and eps must be the same")
    _, _, opt3 = _torch_adamw(2, groups=[([0, 1], dict(eps=1e-8)), ([2], dict(eps=1e-6))])
    refused(opt3.state_dict(), "betas and eps must be the same")


GRADSCALER_KEYS = {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}


def _words(scale, found, tracker, applied, skipped):
    w = torch.zeros(8, dtype=torch.int32)
    w.view(torch.float32)[0] = scale
    w[1], w[2], w[3], w[4] = found, tracker, applied, skipped
    return w


def test_scaler_words_and_dictionary_round_trip():
    w = _words(1024.0, 1, 7, 42, 3)
    d = K.scaler_state_dict(w, 2.0, 0.5, 2000)
    assert set(d) == GRADSCALER_KEYS | {"skipped_steps"}
    assert d == {"scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 7,
                 "skipped_steps": 3}
    back = K.scaler_words(d, applied_steps=42)
    assert back.dtype == torch.int32 and torch.equal(back, _words(1024.0, 0, 7, 42, 3))      # the found word is cleared
    assert torch.equal(K.scaler_words(d), _words(1024.0, 0, 7, 0, 3))                        # the step is the optimizer's
    # a scale that is no power of two keeps its bits
    odd = _words(float(np.float32(1000.1)), 0, 0, 0, 0)
    assert torch.equal(K.scaler_words(K.scaler_state_dict(odd, 2.0, 0.5, 3)), odd)


def test_a_plain_gradscaler_dictionary_loads():
    plain = {"scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 11}
    assert set(plain) == GRADSCALER_KEYS
    assert torch.equal(K.scaler_words(plain, 5), _words(65536.0, 0, 11, 5, 0))
    with pytest.raises(ValueError, match="_growth_tracker"):
        K.scaler_words({k: v for k, v in plain.items() if k != "_growth_tracker"})
    with pytest.raises(ValueError, match="positive"):
        K.scaler_words(dict(plain, scale=0.0))


def _draws():
    return torch.rand(5), [random.random() for _ in range(5)], random.gauss(0, 1), np.random.rand(5), np.random.randn(3)


def test_rng_capture_and_restore_reproduce_the_draws():
    torch.manual_seed(123)
    random.seed(5)
    np.random.seed(6)
    random.gauss(0, 1)                                      # (leaves a cached second value: part of the state)
    np.random.randn(1)
    state = K.capture_rng()
    first = _draws()
    K.restore_rng(state)
    second = _draws()
    assert torch.equal(first[0], second[0]) and first[1] == second[1] and first[2] == second[2]
    assert np.array_equal(first[3], second[3]) and np.array_equal(first[4], second[4])
    assert not torch.equal(first[0], _draws()[0])

    def plain(x):      # tensors, numbers, strings, lists and dicts only
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        if isinstance(x, list):
            return all(plain(v) for v in x)
        return x is None or isinstance(x, (torch.Tensor, int, float, str))
    assert plain(state)


def _state_like_a_checkpoint():
    flat, params, opt = _torch_adamw(2)
    m, v = torch.zeros(NUMEL), torch.zeros(NUMEL)
    step = K.adamw_load_flat(opt.state_dict(), LAYOUT, NAMES, m, v)
    return {"fingerprint": K.fingerprint("resnet18", 3, 32, False, "bf16", NUMEL),
            "encoder": {n: t for n, t in zip(NAMES, _views(flat))}, "decoder": None,
            "optimizer": K.adamw_state_dict(LAYOUT, m, v, step, NAMES, opt.param_groups),
            "scaler_kind": "dynamic", "scaler": K.scaler_state_dict(_words(512.0, 0, 1, 2, 1), 2.0, 0.5, 3),
            "ema": {"params": flat.clone(), "bn_running": torch.ones(4), "decay": 0.5, "warmup": True, "num_updates": 2},
            "clip": {"max_norm": float("inf"), "norm_max": 1.5, "clipped_steps": 0, "nonfinite_steps": 1},
            "bn_frozen": False, "accum_steps": 1, "rng": [K.capture_rng()], "world_size": 1,
            "extra": {"epoch": 2, "losses": [{"epoch": 1, "train": 0.5, "dataset_train": [("diving48", 0.5)]}],
                      "best_val_loss": float("inf"), "split_seed": 7, "args": {"flow_img": None, "motion": False, "lr": 5e-4}}}


def test_write_atomic_and_weights_only_load(tmp_path, monkeypatch):
    path = str(tmp_path / K.STATE_FILE)
    state = _state_like_a_checkpoint()
    K.write_atomic(state, path)
    assert os.listdir(tmp_path) == [K.STATE_FILE]
    got = torch.load(path, map_location="cpu", weights_only=True)
    assert got["fingerprint"] == state["fingerprint"] and got["extra"] == state["extra"] and got["clip"] == state["clip"]
    assert got["scaler"] == state["scaler"]
    for i, s in state["optimizer"]["state"].items():
        assert all(torch.equal(_bits(got["optimizer"]["state"][i][k]), _bits(s[k])) for k in s)
    assert got["optimizer"]["param_groups"] == state["optimizer"]["param_groups"]
    assert torch.equal(got["rng"][0]["torch"], state["rng"][0]["torch"])
    K.restore_rng(got["rng"][0])
    # a save that fails leaves the previous file as it was, and no .tmp
    before = open(path, "rb").read()

    def broken(obj, f, *a, **kw):
        with open(f, "wb") as fh:
            fh.write(b"half a file")
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", broken)
    with pytest.raises(OSError, match="disk full"):
        K.write_atomic({"other": 1}, path)
    assert open(path, "rb").read() == before
    assert os.listdir(tmp_path) == [K.STATE_FILE]


def test_fingerprint_mismatch_names_the_field_and_both_values():
    a = K.fingerprint("resnet18", 3, 32, False, "bf16", 1000)
    assert set(a) == set(K.FINGERPRINT_KEYS)
    K.check_fingerprint(a, dict(a))
    for key, other in (("arch", "resnet34"), ("c_in", 5), ("emb_dim", 128), ("motion", True), ("dtype", "fp16"),
                       ("param_numel", 1004), ("format_version", K.FORMAT_VERSION + 1)):
        with pytest.raises(ValueError) as e:
            K.check_fingerprint(a, dict(a, **{key: other}))
        assert key in str(e.value) and repr(a[key]) in str(e.value) and repr(other) in str(e.value)


def test_resume_argument_mismatch_names_the_key():
    stored = {"dataset": "diving48", "num_epochs": 2, "checkpoint_frequency": None, "state_frequency": 1, "batch_size": 16,
              "seed": 7, "resume": False, "save_dir": "a"}
    K.check_resume_args(stored, dict(stored, num_epochs=4, checkpoint_frequency=2, state_frequency=5, resume=True, save_dir="b"))
    with pytest.raises(ValueError, match=r"batch_size differs \(stored run: 16, now: 32\)"):
        K.check_resume_args(stored, dict(stored, batch_size=32))
    with pytest.raises(ValueError, match="seed"):
        K.check_resume_args(stored, dict(stored, seed=None))
    with pytest.raises(ValueError, match="ema_decay"):
        K.check_resume_args(stored, dict(stored, ema_decay=0.9))


def test_resume_names_what_is_missing_before_any_gpu_work(tmp_path):
    missing = str(tmp_path / "nowhere")
    with pytest.raises(FileNotFoundError, match="does not exist"):
        K.check_resume_dir(missing)
    run = tmp_path / "run"
    run.mkdir()
    with pytest.raises(FileNotFoundError, match="train_state.pt"):
        K.check_resume_dir(str(run))
    (run / K.STATE_FILE).write_bytes(b"x")
    with pytest.raises(FileNotFoundError, match="config.json"):
        K.check_resume_dir(str(run))
    (run / "config.json").write_text("{}")
    assert K.check_resume_dir(str(run)) == str(run / K.STATE_FILE)
    # main() makes these checks first: on a machine without a GPU it still gets as far as the refusal
    import train_vpd_model
    kw = dict(dataset="diving48", num_epochs=4, batch_size=16, learning_rate=5e-4, img_dim=128, flow_img=None, motion=False,
              encoder_arch="resnet18", model_select_window=5, checkpoint_frequency=None, pretrained=False, emb_dir=None,
              penn_dir=None, no_test_video=False, min_pose_score=None, synthetic=64, resume=True)
    with pytest.raises(FileNotFoundError, match="does not exist"):
        train_vpd_model.main(save_dir=missing, **kw)
    assert not os.path.exists(missing)
    # a stored run that is complete: nothing left, no error; other arguments: refused by name
    defaults = dict(synthetic_emb_dim=128, gpu_augment=False, no_augment=False, dtype="bf16", loss_scale="static", ema_decay=None,
                    ema_warmup=False, clip_grad_norm=None, weight_decay=None, no_bn_bias_decay=False, backbone_lr_scale=None,
                    accum_steps=None, seed=None)
    stored_args = dict(kw, save_dir="elsewhere", resume=False, state_frequency=1, **defaults)
    K.write_atomic({"extra": {"epoch": 4, "args": stored_args}}, str(run / K.STATE_FILE))
    assert train_vpd_model.main(save_dir=str(run), **kw) is None
    with pytest.raises(ValueError, match="batch_size"):
        train_vpd_model.main(save_dir=str(run), **dict(kw, batch_size=32))


# -- the optimizer, the scalers and the engine's state on the stub engine of tests/test_param_groups_cpu.py (CPU tensors, a library
#    that records) ----------------------------------------------------------------------------------------------------------
def _stub_optimizer(two_groups=False):
    from tests.test_param_groups_cpu import LAYOUT as ROWS, _stub_engine, _tensors_of, _two_groups
    from vpd_amd.trainer import FusedAdamW
    eng = _stub_engine()
    t = _tensors_of(eng)
    g = torch.Generator().manual_seed(3)
    for _, _, _, off, n in ROWS:                            # moments where tensors are, zeros in the two padding floats
        eng.adam_m[off:off + n] = torch.randn(n, generator=g)
        eng.adam_v[off:off + n] = torch.rand(n, generator=g)
    groups = _two_groups(t) if two_groups else [{"params": list(t.values())}]
    return eng, t, FusedAdamW(groups, eng, lr=1e-3), groups


@pytest.mark.parametrize("two_groups", [False, True], ids=["one_group", "two_groups"])
def test_fused_adamw_state_dict_is_torchs_and_comes_back(two_groups):
    from vpd_amd.models.util import DynamicLossScaler
    eng, t, opt, groups = _stub_optimizer(two_groups)
    sd = opt.state_dict()
    order = [q for g in opt.param_groups for q in g["params"]]
    assert sorted(sd["state"]) == list(range(len(order))) and len(sd["param_groups"]) == len(opt.param_groups)
    ptr0 = eng.params.data_ptr()
    for i, q in enumerate(order):
        s = sd["state"][i]
        assert float(s["step"]) == 6.0 and s["step"].dtype == torch.float32      # the stub engine's adam_step
        assert s["exp_avg"].shape == q.shape and s["exp_avg"].data_ptr() - eng.adam_m.data_ptr() == q.data_ptr() - ptr0
        assert s["exp_avg_sq"].data_ptr() - eng.adam_v.data_ptr() == q.data_ptr() - ptr0
    # torch.optim.AdamW over the same parameters in the same order loads it
    topt = torch.optim.AdamW([dict(g) for g in groups], lr=1.0)
    topt.load_state_dict(sd)
    assert all(torch.equal(topt.state[q]["exp_avg"], sd["state"][i]["exp_avg"]) for i, q in enumerate(order))
    assert [g["lr"] for g in topt.param_groups] == [g["lr"] for g in opt.param_groups]
    # ... and its dictionary comes back: moments, the step (through the setter: an attached device block receives it), hyper-parameters
    back = copy.deepcopy(topt.state_dict())
    for s in back["state"].values():
        s["step"] = torch.tensor(9.0)
        s["exp_avg"] = s["exp_avg"] * 2
    back["param_groups"][0]["lr"] = 0.25
    m_before = eng.adam_m.clone()
    scaler = DynamicLossScaler(eng, init_scale=512.0)
    assert int(scaler.state[3]) == 6
    opt._grouping = "stale"
    opt.load_state_dict(back)
    assert eng.adam_step == 9 and int(scaler.state[3]) == 9 and eng._adam_step == 9
    assert torch.equal(eng.adam_m, m_before * 2) and opt.param_groups[0]["lr"] == 0.25 and opt._grouping is None
    # refusals leave everything as it was
    bad = copy.deepcopy(topt.state_dict())
    bad["state"][1]["step"] = torch.tensor(4.0)
    with pytest.raises(ValueError, match="steps differ"):
        opt.load_state_dict(bad)
    bad = copy.deepcopy(topt.state_dict())
    bad["param_groups"] = bad["param_groups"] + [dict(bad["param_groups"][0], params=[])]
    with pytest.raises(ValueError, match="parameter groups"):
        opt.load_state_dict(bad)
    assert eng.adam_step == 9 and torch.equal(eng.adam_m, m_before * 2)
    # before the first step: empty, and moments are allocated on load
    eng.adam_m = eng.adam_v = None
    assert opt.state_dict()["state"] == {}
    opt.load_state_dict(back)
    assert torch.equal(eng.adam_m, m_before * 2)


def test_scalers_keep_their_words_and_leave_the_step_to_the_optimizer():
    from tests.test_param_groups_cpu import _stub_engine
    from vpd_amd.models.util import DynamicLossScaler, LossScaler
    eng = _stub_engine()
    static = LossScaler(eng, 64.0)
    assert static.state_dict() == {"scale": 64.0}
    static.load_state_dict({"scale": 1024.0})
    assert static.get_scale() == 1024.0
    sc = DynamicLossScaler(eng, init_scale=256.0, growth_interval=3)
    sc.state[1], sc.state[2], sc.state[4] = 1, 2, 5
    d = sc.state_dict()
    assert set(d) == GRADSCALER_KEYS | {"skipped_steps"}
    assert d == {"scale": 256.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 3, "_growth_tracker": 2, "skipped_steps": 5}
    other = DynamicLossScaler(_stub_engine(), init_scale=65536.0)
    other.state[1], other.state[3] = 1, 77
    other.load_state_dict(d)
    assert torch.equal(other.state, _words(256.0, 0, 2, 77, 5))      # found cleared, the applied-step word left alone
    assert (other._growth, other._backoff, other._interval) == (2.0, 0.5, 3)
    other.load_state_dict({k: v for k, v in d.items() if k != "skipped_steps"})      # a plain GradScaler dictionary
    assert other.skipped_steps == 0 and other.applied_steps == 77


def test_engine_ema_and_clip_state_round_trip_in_both_counting_modes():
    from tests.test_param_groups_cpu import NUMEL as N_STUB, _stub_engine

    def engine(device_block):
        eng = _stub_engine()
        eng.ema_params, eng.ema_bn_running = torch.arange(float(N_STUB)), torch.arange(8.0)
        eng._ema, eng._ema_t, eng._ema_t0 = (0.5, True), 0, 0
        if device_block:
            eng.L.vpd_clip_state_bytes = lambda: 256
            eng.enable_grad_clip(2.5)                        # the step count moves into the clip block
        return eng
    src = engine(False)
    src._ema_t, src._ema_t0, src._adam_step = 4, 2, 6        # host mode: four updates since step 2
    st = src.ema_state()
    assert st["num_updates"] == 4 and st["decay"] == 0.5 and st["warmup"] is True and st["params"] is src.ema_params
    for device_block in (False, True):
        dst = engine(device_block)
        dst.ema_params, dst.ema_bn_running = torch.zeros(N_STUB), torch.zeros(8)
        dst.adam_step = 6
        version = dst._ema_version
        dst.load_ema_state(st)
        assert (dst._ema_t, dst._ema_t0, dst._ema_version) == (4, 2, version + 1)
        assert torch.equal(dst.ema_params, src.ema_params) and torch.equal(dst.ema_bn_running, src.ema_bn_running)
        assert dst.ema_state()["num_updates"] == 4           # one number whichever side counts
    dst.adam_step = 9                                        # behind the block the count follows the applied steps
    assert dst.ema_state()["num_updates"] == 7
    # the clip block: max_norm and the statistics, the step word follows adam_step
    dst._clip[8:13] = torch.tensor([0, 0, 0, 3, 1], dtype=torch.int32)
    dst._clip[9:10] = torch.tensor([7.5]).view(torch.int32)
    cs = dst.clip_state()
    assert cs == {"max_norm": 2.5, "norm_max": 7.5, "clipped_steps": 3, "nonfinite_steps": 1}
    fresh = engine(True)
    fresh._clip_max_norm = 1.0
    fresh.adam_step = 9
    fresh.load_clip_state(cs)
    assert fresh.clip_state() == cs and int(fresh._clip[3]) == 9 and fresh.clip_stats()["norm_max"] == 7.5
    with pytest.raises(RuntimeError, match="enable_ema"):
        _stub_engine().load_ema_state(st)
    with pytest.raises(RuntimeError, match="enable_grad_clip"):
        _stub_engine().load_clip_state(cs)


def _rng_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(100 + rank)
    random.seed(200 + rank)
    np.random.seed(300 + rank)
    states = K.gather_rng(rank, world)
    after_capture = _draws()
    mine = K.pick_rng(states, rank, world)
    other = K.pick_rng(states, 1 - rank, world)
    K.restore_rng(mine)
    again = _draws()
    K.restore_rng(other)
    others = _draws()
    refused = None
    try:
        K.pick_rng(states, rank, 3)
    except ValueError as e:
        refused = str(e)
    q.put((rank, len(states), after_capture[0].numpy(), again[0].numpy(), others[0].numpy(), after_capture[1] == again[1],
           bool(np.array_equal(after_capture[3], again[3])), refused))
    dist.barrier()
    dist.destroy_process_group()


def test_every_rank_gets_its_own_generator_state_world2():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_rng_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=120) for _ in range(world)], key=lambda o: o[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, n, first, again, others, py_same, np_same, refused in outs:
        assert n == world
        assert np.array_equal(first, again) and py_same and np_same           # its own entry continues its own stream
        assert np.array_equal(others, outs[1 - rank][2])                       # the other entry is the other rank's
        assert not np.array_equal(first, others)
        assert refused is not None and "world size" in refused and "2 rank" in refused and "3" in refused
    with pytest.raises(ValueError, match="world size"):
        K.pick_rng([K.capture_rng()], 0, 2)
