"""Dynamic loss scaling for fp16 training, decided on the device (vpd_amd.models.util.DynamicLossScaler; vpd_scale_state and the
entry points around it in include/vpd_hip.h) -- what torch.cuda.amp.GradScaler() is to the reference (train_vpd_model.py:105;
models/util.py:55-57): the non-finite search, torch's update rule, a skipped step that writes nothing, recovery after it, the
reference's default start of 65,536, two data-parallel ranks deciding alike, and the command line.

Tests plant inf / NaN / 1e18 VALUES in data; that is arithmetic.  Bounds: bit equality where the arithmetic is the same; where
only the bias corrections' origin differs (host pow against device pow, both in double and rounded to float) the project's AdamW
tolerance, 2e-6 absolute (tests/test_fullsize_gpu.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vpd_oracle as O
from tests.test_fp16_gpu import build_fp16

pytestmark = pytest.mark.gpu

ADAMW_TOL = 2e-6
FIX = {
    ("resnet18", True): dict(arch="resnet18", c_in=5, emb_dim=32, motion=True, n=8, hw=128, lr=5e-4, seed=130),
    ("resnet18", False): dict(arch="resnet18", c_in=3, emb_dim=128, motion=False, n=5, hw=64, lr=1e-3, seed=140),
    ("resnet34", True): dict(arch="resnet34", c_in=5, emb_dim=128, motion=True, n=8, hw=128, lr=5e-4, seed=100),
    ("resnet34", False): dict(arch="resnet34", c_in=5, emb_dim=128, motion=False, n=5, hw=128, lr=5e-4, seed=110),
}
# flavour -> (planted target entry, fixture with the motion head?): with 1e18 the fp32 loss (1e36) and d(loss)/d(pred) stay finite
# and only the fp16 activation gradients overflow -- the case a look at the forward loss cannot see
FLAVOURS = {"inf": (float("inf"), True), "1e18": (1e18, False)}


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _new_state(scale=65536.0):
    host = torch.zeros(8, dtype=torch.int32)
    host.view(torch.float32)[0] = scale
    return host.cuda()


def _read(state):
    h = state.cpu()
    return dict(scale=float(h.view(torch.float32)[0]), found=int(h[1]), tracker=int(h[2]), applied=int(h[3]), skipped=int(h[4]))


# ---- 2. the non-finite search alone ----------------------------------------------------------------------------------------
def _found_by_kernel(L, x, preset=0):
    st = _new_state()
    st[1] = preset
    assert L.vpd_op_check_finite(_ptr(x), x.numel(), _ptr(st), _stream()) == 0, L.vpd_last_error()
    return _read(st)["found"]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 2 ** 20 + 1, 21356608])
def test_check_kernel_agrees_with_torch_isfinite(n):
    from vpd_amd import _lib
    L = _lib.lib("fp16")
    g = torch.Generator(device="cuda").manual_seed(n)
    base = torch.randn(n + 1, generator=g, device="cuda")
    rnd = int(torch.randint(0, n, (1,), generator=torch.Generator().manual_seed(n)).item())
    for off in (0, 1):                                                    # a 16-byte aligned start and one 4 bytes behind it
        x = base[off:off + n]
        assert _found_by_kernel(L, x) == 0 and bool(torch.isfinite(x).all())
        for pos in sorted({0, n - 1, rnd}):
            for bad in (float("inf"), float("-inf"), float("nan")):
                keep = float(x[pos])
                x[pos] = bad
                assert not bool(torch.isfinite(x).all())
                assert _found_by_kernel(L, x) == 1, (n, off, pos, bad)
                x[pos] = keep
        assert _found_by_kernel(L, x) == 0
    # the largest finite floats, subnormals and zeros are finite; a word that is set stays set
    x = base[:n]
    fmax = torch.finfo(torch.float32).max                                  # 3.4028235e38
    for fill in (fmax, -fmax, 1e-45, -1e-40, 0.0, -0.0):
        x.fill_(fill)
        assert bool(torch.isfinite(x).all()) and _found_by_kernel(L, x) == 0, fill
    assert _found_by_kernel(L, x, preset=1) == 1
    assert L.vpd_op_check_finite(_ptr(x), 0, _ptr(_new_state()), _stream()) == 0      # an empty range is legal


# ---- 3. the update rule against torch.amp.GradScaler -------------------------------------------------------------------------
def _drive_both(seq, **kw):
    from vpd_amd import _lib
    L = _lib.lib("fp16")
    ref = torch.amp.GradScaler("cpu", **kw)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=1e-3)
    st = _new_state(kw.get("init_scale", 65536.0))
    growth, backoff, interval = kw.get("growth_factor", 2.0), kw.get("backoff_factor", 0.5), kw.get("growth_interval", 2000)
    skipped = 0
    for i, found in enumerate(seq):
        ref.scale(torch.zeros(1))
        p.grad = torch.tensor([float("inf") if found else 1.0])
        ref.step(opt)
        ref.update()
        if found:
            st[1] = 1
            skipped += 1
        assert L.vpd_scale_state_update(_ptr(st), growth, backoff, interval, _stream()) == 0
        got = _read(st)
        ref_step = int(opt.state[p]["step"]) if p in opt.state and "step" in opt.state[p] else 0
        assert got["scale"] == float(ref.get_scale()), (i, got, ref.get_scale())
        assert got["applied"] == ref_step and got["skipped"] == skipped and got["found"] == 0, (i, got, ref_step, skipped)
    return _read(st)


def test_update_rule_equals_torch_gradscaler_interval_5():
    rng = np.random.RandomState(7)
    seq = (rng.rand(200) < 0.15).tolist()
    end = _drive_both(seq, init_scale=65536.0, growth_interval=5)
    assert end["skipped"] == sum(seq) and end["applied"] == 200 - sum(seq)


def test_update_rule_equals_torch_gradscaler_defaults():
    end = _drive_both([False] * 2001 + [True])
    assert end["scale"] == 65536.0 and end["applied"] == 2001 and end["skipped"] == 1      # doubled at 2,000, halved by the last


# ---- 4.-6. a skipped step is a no-op; nothing changes without an overflow; recovery -----------------------------------------
def _fresh_eval_embeddings(meta, enc, img):
    """eval embeddings through a NEW model (new engine, new eval plan) loaded from enc's state_dict"""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    enc2 = RGBF_EmbeddingModel(meta["arch"], meta["emb_dim"], meta["c_in"] != 3, "cuda",
                               in_channels=None if meta["c_in"] in (3, 5) else meta["c_in"], dtype="fp16")
    enc2.load_state_dict(enc.state_dict())
    return enc2.embed(img.numpy())


def _train_step(tr, opt, scaler, img, tgt):
    from vpd_amd.models.util import step
    tr.encoder.train()
    if hasattr(tr, "fcn_time"):
        tr.fcn_time.train()
    loss = tr._forward_loss(img, tgt, train=True)
    step(opt, scaler, loss)
    torch.cuda.synchronize()
    return loss


def _all_params(tr):
    ps = list(tr.encoder.parameters())
    if hasattr(tr, "fcn_time"):
        ps += list(tr.fcn_time.parameters())
    return ps


def _moments(eng, opt, fused):
    if fused:
        return [eng.adam_m.clone(), eng.adam_v.clone()]
    out = []
    for q in opt.param_groups[0]["params"]:
        s = opt.state[q]
        out += [s["exp_avg"].clone(), s["exp_avg_sq"].clone(), torch.as_tensor(s["step"]).clone().float().cuda()]
    return out


def _max_diff(a, b):
    return float((a - b).abs().max())


def _same_or_within_adamw_tol(a, b, what):
    """bit equality expected; the one permitted difference is the device-computed bias correction (2e-6 absolute)"""
    equal = torch.equal(a, b)
    d = _max_diff(a, b)
    print("%s: bit-identical %s, max |diff| %.3e" % (what, equal, d))
    assert equal or d <= ADAMW_TOL, (what, d)
    return equal


@pytest.mark.parametrize("fused", [True, False], ids=["fused_adamw", "torch_adamw"])
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
@pytest.mark.parametrize("arch", ["resnet18", "resnet34"])
def test_skipped_step_is_a_noop_and_training_recovers(arch, flavour, fused):
    from vpd_amd.models.util import DynamicLossScaler, LossScaler
    value, motion = FLAVOURS[flavour]
    meta = FIX[(arch, motion)]
    enc, tr, _, _, img, tgt = build_fp16(meta)
    eng = enc.engine
    opt = tr.get_optimizer(meta["lr"])[0] if fused else torch.optim.AdamW(_all_params(tr), lr=meta["lr"])
    sc = DynamicLossScaler(eng, init_scale=256, growth_interval=10 ** 6)
    _train_step(tr, opt, sc, img, tgt)                                    # one clean step
    assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps) == (256.0, 0, 1)
    p0, bn0, mom0 = eng.params.clone(), eng.bn_running.clone(), _moments(eng, opt, fused)
    assert bool(torch.isfinite(p0).all()) and _max_diff(p0, torch.zeros_like(p0)) > 0
    e0 = _fresh_eval_embeddings(meta, enc, img)
    bad = tgt.clone()
    bad[1, 3] = value
    loss = _train_step(tr, opt, sc, img, bad)                             # the poisoned step
    if flavour == "1e18":
        lv = float(eng.loss_step.item())
        assert np.isfinite(lv) and lv > 1e35, lv                          # the forward loss does not give it away
    del loss
    assert torch.equal(eng.params, p0), _max_diff(eng.params, p0)
    for a, b in zip(_moments(eng, opt, fused), mom0):
        assert torch.equal(a, b)
    eng.bn_running.copy_(bn0)                 # the forward updated the running statistics, as the reference's does
    e1 = _fresh_eval_embeddings(meta, enc, img)
    assert np.array_equal(e0, e1) and np.isfinite(e1).all()
    assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps) == (128.0, 1, 1)
    if fused:
        assert eng.adam_step == 1
    # recovery: a clean step at 128 = the second step of a twin that never saw the poisoned batch
    _train_step(tr, opt, sc, img, tgt)
    assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps) == (128.0, 1, 2)
    enc_t, tr_t, _, _, _, _ = build_fp16(meta)
    opt_t = tr_t.get_optimizer(meta["lr"])[0] if fused else torch.optim.AdamW(_all_params(tr_t), lr=meta["lr"])
    _train_step(tr_t, opt_t, LossScaler(enc_t.engine, 256.0), img, tgt)
    _train_step(tr_t, opt_t, LossScaler(enc_t.engine, 128.0), img, tgt)
    _same_or_within_adamw_tol(eng.params, enc_t.engine.params, "recovery %s %s fused=%s: parameters" % (arch, flavour, fused))
    assert _max_diff(eng.params, p0) > 1e-5                               # ... and it did move


@pytest.mark.parametrize("arch", ["resnet18", "resnet34"])
def test_static_scaler_lets_the_overflow_into_the_parameters(arch):
    """What the feature prevents, on record: the same poisoned step behind the static scaler (the default) leaves non-finite
    parameters."""
    from vpd_amd.models.util import LossScaler
    meta = FIX[(arch, False)]
    enc, tr, _, _, img, tgt = build_fp16(meta)
    opt = tr.get_optimizer(meta["lr"])[0]
    sc = LossScaler(enc.engine, 256.0)
    _train_step(tr, opt, sc, img, tgt)
    assert bool(torch.isfinite(enc.engine.params).all())
    bad = tgt.clone()
    bad[1, 3] = 1e18
    _train_step(tr, opt, sc, img, bad)
    assert np.isfinite(float(enc.engine.loss_step.item()))
    assert not bool(torch.isfinite(enc.engine.params).all())


@pytest.mark.parametrize("arch,motion", [("resnet18", True), ("resnet34", False), ("resnet34", True)])
def test_nothing_changes_when_nothing_overflows(arch, motion):
    """Three steps behind DynamicLossScaler(256) and three behind LossScaler(256) from the same state: parameters and moments.
    Measured (printed): whether the bits agree; the bound if not is ADAMW_TOL."""
    from vpd_amd.models.util import DynamicLossScaler, LossScaler
    meta = FIX[(arch, motion)]
    res = []
    for dyn in (True, False):
        enc, tr, _, _, img, tgt = build_fp16(meta)
        opt = tr.get_optimizer(meta["lr"])[0]
        sc = DynamicLossScaler(enc.engine, init_scale=256) if dyn else LossScaler(enc.engine, 256.0)
        for _ in range(3):
            _train_step(tr, opt, sc, img, tgt)
        if dyn:
            assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps, sc.growth_tracker) == (256.0, 0, 3, 3)
        assert enc.engine.adam_step == 3
        res.append((enc.engine.params.clone(), enc.engine.adam_m.clone(), enc.engine.adam_v.clone()))
    for name, a, b in zip(("parameters", "adam_m", "adam_v"), res[0], res[1]):
        _same_or_within_adamw_tol(a, b, "dynamic vs static, 3 steps, %s motion=%s: %s" % (arch, motion, name))


# ---- 7. the reference's default start ---------------------------------------------------------------------------------------
def test_default_start_settles_within_eight_halvings():
    """GradScaler's default 65,536 on the ResNet-34 fixture: static 256 and 1,024 are known finite here (tests/test_fp16_gpu.py),
    so at most 8 halvings can be needed."""
    from vpd_amd.models.util import DynamicLossScaler
    meta = FIX[("resnet34", True)]
    enc, tr, _, _, img, tgt = build_fp16(meta)
    opt = tr.get_optimizer(meta["lr"])[0]
    sc = DynamicLossScaler(enc.engine)
    assert sc.get_scale() == 65536.0
    for _ in range(12):
        _train_step(tr, opt, sc, img, tgt)
    print("default start: settled scale %g after %d skipped / %d applied steps" % (sc.get_scale(), sc.skipped_steps, sc.applied_steps))
    assert sc.skipped_steps <= 8 and sc.applied_steps >= 4 and sc.skipped_steps + sc.applied_steps == 12
    assert sc.get_scale() == 65536.0 * 0.5 ** sc.skipped_steps
    assert bool(torch.isfinite(enc.engine.params).all()) and enc.engine.adam_step == sc.applied_steps


def test_get_optimizer_loss_scale_argument():
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import DynamicLossScaler, LossScaler
    from vpd_amd.trainer import ModelTrainer
    enc, tr, _, _, _, _ = build_fp16(FIX[("resnet18", False)])
    _, sc = tr.get_optimizer(1e-3)
    assert type(sc) is LossScaler and sc.get_scale() == 256.0            # the default stays the static scaler
    _, sc = tr.get_optimizer(1e-3, loss_scale=1024)
    assert type(sc) is LossScaler and sc.get_scale() == 1024.0
    _, sc = tr.get_optimizer(1e-3, loss_scale="dynamic")
    assert type(sc) is DynamicLossScaler and sc.get_scale() == 65536.0 and sc.applied_steps == 0 and sc.skipped_steps == 0
    with pytest.raises(ValueError):
        tr.get_optimizer(1e-3, loss_scale="sometimes")
    tr16 = ModelTrainer(RGBF_EmbeddingModel("resnet18", 32, True, "cuda"), False)
    assert tr16.get_optimizer(1e-3)[1] is None
    for ask in ("dynamic", 256.0):
        with pytest.raises(ValueError):
            tr16.get_optimizer(1e-3, loss_scale=ask)


# ---- 8. two ranks decide alike -------------------------------------------------------------------------------------------------
def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, q, wire):
    if wire:
        os.environ["VPD_DDP_WIRE"] = wire
    import torch.distributed as dist
    from vpd_amd.ddp import shard_slice
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import DynamicLossScaler
    from vpd_amd.trainer import ModelTrainer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        sd = O.procedural_state_dict(O.encoder_schema("resnet18", 5, 32), 2)
        img = O.synthetic_crops(10, 5, 64, 3)
        tgt = O.synthetic_targets(10, 32, False, 4)
        sl = shard_slice(10, rank, world)
        enc = RGBF_EmbeddingModel("resnet18", 32, True, "cuda", dtype="fp16")
        enc.load_state_dict(sd)
        tr = ModelTrainer(enc, False, process_group=dist.group.WORLD)
        opt = tr.get_optimizer(5e-4)[0]
        sc = DynamicLossScaler(enc.engine, init_scale=256, growth_interval=10 ** 6)
        out = [enc.engine.params.clone().cpu().numpy()]
        mine = tgt[sl].clone()
        if rank == 1:
            mine[0, 0] = float("inf")                                     # only rank 1's shard is poisoned
        for t in (mine, tgt[sl]):
            _train_step(tr, opt, sc, img[sl], t)
            out.append(enc.engine.params.clone().cpu().numpy())
            out.append((sc.get_scale(), sc.skipped_steps, sc.applied_steps))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("wire", ["", "bf16"], ids=["fp32_wire", "bf16_wire"])
def test_two_ranks_skip_together(wire):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q, wire)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, a), (_, b) = res
    assert a[2] == b[2] == (128.0, 1, 0)                                  # both skipped, both scales halved
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], a[0])      # ... and nothing was written on either rank
    assert a[4] == b[4] == (128.0, 1, 1)
    assert np.array_equal(a[3], b[3]) and np.isfinite(a[3]).all() and not np.array_equal(a[3], a[1])


# ---- 9. the command line ------------------------------------------------------------------------------------------------------
def test_train_cli_with_dynamic_loss_scale(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "run")
    r = subprocess.run([sys.executable, os.path.join(root, "train_vpd_model.py"), "diving48", "--save_dir", out, "--flow_img", "flow",
                        "--synthetic", "64", "--batch_size", "32", "--num_epochs", "2", "--dtype", "fp16", "--loss_scale", "dynamic"],
                       cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout[-1500:])
    losses = json.load(open(os.path.join(out, "loss.json")))
    assert len(losses) == 2 and all(np.isfinite(l["train"]) and np.isfinite(l["val"]) for l in losses)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Epoch ")]
    assert len(lines) == 2 and all("loss scale:" in ln and "skipped steps:" in ln for ln in lines), r.stdout
    assert json.load(open(os.path.join(out, "config.json")))["loss_scale"] == "dynamic"
