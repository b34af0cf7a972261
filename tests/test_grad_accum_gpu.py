"""Gradient accumulation through the engine, the trainer, the scaler, the clipping, the EMA and the bucket reducer.  The student is
ResNet-18 with 5 channels, 64 x 64 crops, emb 32; the micro-batches are 4, 4 and 2 crops (the ragged last one)."""
import os

import numpy as np
import pytest
import torch

from oracle import vpd_oracle as O

pytestmark = pytest.mark.gpu
ARCH, C_IN, HW, D, LR = "resnet18", 5, 64, 32, 5e-4
MICRO = (slice(0, 4), slice(4, 8), slice(8, 10))


@pytest.fixture(scope="module")
def data():
    sd = O.procedural_state_dict(O.encoder_schema(ARCH, C_IN, D), 2)
    return sd, O.synthetic_crops(10, C_IN, HW, 3), O.synthetic_targets(10, D, False, 4)


def _build(sd, dtype="bf16", **kw):
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    enc = RGBF_EmbeddingModel(ARCH, D, True, "cuda", dtype=dtype)
    enc.load_state_dict(sd)
    return enc, ModelTrainer(enc, False, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pending(eng):
    pl = eng._step_plan
    return int(eng.L.vpd_plan_grads_pending(pl.handle))


def _live(eng, lazy):
    """the gradients the step would read, as the plan exposes them: every bucket's scratch view + the small ranges of the flat
    buffer after a lazy backward, the whole flat buffer after an eager one"""
    pl = eng._step_plan
    torch.cuda.synchronize()
    if lazy:
        return [v.clone() for v in pl.scratch_views] + [eng._grads[pl.small_idx].clone()]
    return [eng._grads.clone()]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("lazy", [True, False], ids=["lazy", "eager"])
def test_fold_is_the_fp32_sum_of_what_the_backward_passes_wrote(data, dtype, lazy):
    """the reference is the snapshots of the same run, so the atomics' summation order does not enter: every bit must agree"""
    sd, img, tgt = data
    enc, tr = _build(sd, dtype)
    eng = enc.engine
    if dtype == "fp16":
        eng.loss_scale = 256.0
    assert eng._accum is None
    snaps = []
    for i, sl in enumerate(MICRO):
        loss = tr._forward_loss(img[sl], tgt[sl], train=True)
        (loss.backward_for_step if lazy else loss.backward)()
        assert _pending(eng) == int(lazy)
        snaps.append(_live(eng, lazy))
        if i < 2:
            eng.accumulate_grads()
            assert _pending(eng) == 0 and eng._accum_count == i + 1
    assert eng._accum_layout == ("scratch" if lazy else "flat") and eng._accum.numel() == eng._step_plan.accum_numel
    eng.fold_accumulated_grads()
    assert _pending(eng) == int(lazy) and eng._accum_count == 0
    got = _live(eng, lazy)
    for k, (g, a, b, c) in enumerate(zip(got, *snaps)):
        want = (a + b) + c                                              # torch's fp32 adds: correctly rounded
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        bad = int((_bits(g) != _bits(want)).sum())
        assert bad == 0, "piece %d: %d of %d elements differ from (s1 + s2) + s3" % (k, bad, want.numel())
        assert not torch.equal(g, c)                                    # (the fold did add something)
    eng.fold_accumulated_grads()                                        # nothing held: a no-op
    for g, g2 in zip(got, _live(eng, lazy)):
        assert torch.equal(_bits(g), _bits(g2))


def test_mixing_layouts_inside_a_window_raises(data):
    sd, img, tgt = data
    enc, tr = _build(sd)
    eng = enc.engine
    tr._forward_loss(img[MICRO[0]], tgt[MICRO[0]], train=True).backward_for_step()
    eng.accumulate_grads()
    tr._forward_loss(img[MICRO[1]], tgt[MICRO[1]], train=True).backward()          # eager: the other layout
    with pytest.raises(RuntimeError, match="layout"):
        eng.accumulate_grads()
    with pytest.raises(RuntimeError, match="layout"):
        eng.fold_accumulated_grads()
    assert eng._accum_count == 1
    eng.drop_accumulated_grads()
    eng.fold_accumulated_grads()


def test_window_equals_a_hand_made_twin(data):
    """three micro-batches through step(..., accumulate=True / False) against a twin whose three eager gradients torch sums and one
    non-lazy FusedAdamW step applies.  adam_m after step 1 is 0.1 g: it exposes the gradient where the parameter update is
    sign-like.  rel L2 < 1e-3 is the project's bound for two separately run backward passes (tests/test_ddp_gpu.py, measured
    ~1e-6); a dropped or doubled micro-batch misses it by orders of magnitude."""
    from vpd_amd.models.util import step
    sd, img, tgt = data
    enc, tr = _build(sd)
    opt, sc = tr.get_optimizer(LR)
    for i, sl in enumerate(MICRO):
        step(opt, sc, tr._forward_loss(img[sl], tgt[sl], train=True), accumulate=i < 2)
    eng = enc.engine
    assert eng.adam_step == 1 and eng._accum_count == 0
    enc2, tr2 = _build(sd)
    eng2 = enc2.engine
    opt2, _ = tr2.get_optimizer(LR)
    total = None
    for sl in MICRO:
        tr2._forward_loss(img[sl], tgt[sl], train=True).backward()
        g = eng2.grads.clone()
        total = g if total is None else total + g
    eng2._grads.copy_(total)
    opt2.step()
    torch.cuda.synchronize()
    assert eng2.adam_step == 1 and eng2._accum is None
    rel = float((eng.adam_m - eng2.adam_m).norm() / eng2.adam_m.norm())
    print("window vs twin: adam_m rel L2 %.3e, bit-identical %s; params bit-identical %s"
          % (rel, torch.equal(_bits(eng.adam_m), _bits(eng2.adam_m)), torch.equal(_bits(eng.params), _bits(eng2.params))))
    assert rel < 1e-3, rel
    # a single micro-batch is NOT the window: the bound tells them apart
    one = 0.1 * g
    assert float((one - eng2.adam_m).norm() / eng2.adam_m.norm()) > 0.1


def test_torch_optimizer_finds_the_folded_sum_in_grad(data):
    """step() with an optimizer that reads p.grad: eager backwards, the flat layout, the fold in front of optimizer.step().  SGD with
    lr = 1 and no momentum makes p0 - p1 the gradient it read (to the rounding of p); against the twin's summed gradients at
    rel L2 < 1e-3, the bound for separately run backward passes used above"""
    from vpd_amd.models.util import step
    sd, img, tgt = data
    enc, tr = _build(sd)
    eng = enc.engine
    opt = torch.optim.SGD(list(enc.parameters()), lr=1.0)
    p0 = eng.params.clone()
    for i, sl in enumerate(MICRO):
        step(opt, None, tr._forward_loss(img[sl], tgt[sl], train=True), accumulate=i < 2)
        assert eng._accum_count == (i + 1 if i < 2 else 0) and (i == 2 or eng._accum_layout == "flat")
    torch.cuda.synchronize()
    read = p0 - eng.params
    enc2, tr2 = _build(sd)
    total = None
    for sl in MICRO:
        tr2._forward_loss(img[sl], tgt[sl], train=True).backward()
        g = enc2.engine.grads.clone()
        total = g if total is None else total + g
    rel = float((read - total).norm() / total.norm())
    print("torch optimizer: gradient read by SGD against the twin's sum, rel L2 %.3e" % rel)
    assert rel < 1e-3, rel
    assert float((read - g).norm() / total.norm()) > 0.1               # (the last micro-batch alone is told apart)


def test_abandoned_window_does_not_leak_into_the_next_epoch(data):
    from vpd_amd.models.util import step
    sd, img, tgt = data
    res = []
    for abandon in (True, False):
        enc, tr = _build(sd)
        opt, sc = tr.get_optimizer(LR)
        if abandon:      # a micro-batch accumulated by hand, no final step
            step(opt, sc, tr._forward_loss(img[MICRO[1]], tgt[MICRO[1]], train=True), accumulate=True)
            assert enc.engine._accum_count == 1
        tr.epoch(_batches(img, tgt, (0,)), optimizer=opt, scaler=sc)
        torch.cuda.synchronize()
        assert enc.engine.adam_step == 1 and enc.engine._accum_count == 0
        res.append(enc.engine.adam_m.clone())
    rel = float((res[0] - res[1]).norm() / res[1].norm())
    assert rel < 1e-3, rel


def _batches(img, tgt, order):
    return [{"img": img[MICRO[k]], "emb": tgt[MICRO[k]]} for k in order]


def test_trainer_epoch_steps_on_every_third_batch_and_on_the_last(data):
    sd, img, tgt = data
    enc, tr = _build(sd, accum_steps=3)
    eng = enc.engine
    opt, sc = tr.get_optimizer(LR)
    first = _batches(img, tgt, (0, 1, 2))
    seen = []
    v3 = tr.epoch(first, optimizer=opt, scaler=sc, progress_cb=seen.append)
    assert eng.adam_step == 1 and seen == [4, 4, 2] and eng._accum_count == 0
    nbt0 = int(eng.num_batches_tracked[0].item())
    assert nbt0 == 3
    tr.epoch(_batches(img, tgt, (0, 1, 2, 0, 1, 2, 0)), optimizer=opt, scaler=sc)
    assert eng.adam_step == 1 + 3                                       # batches 3, 6 and 7
    assert int(eng.num_batches_tracked[0].item()) == nbt0 + 7           # BatchNorm statistics per micro-batch
    assert eng._accum_count == 0 and eng._accum is not None
    # the first window ran at the initial weights: its epoch value is that of a K = 1 run whose weights stand still (lr = 0,
    # decay factor 1 - 0 * wd = 1), the sum of the same three forward losses over the same 10 crops.  1e-4 relative is the
    # project's bound for the loss of two runs of one forward (tests/test_ddp_gpu.py: the BatchNorm sums' atomics)
    enc1, tr1 = _build(sd)
    opt1, sc1 = tr1.get_optimizer(0.0)
    v1 = tr1.epoch(first, optimizer=opt1, scaler=sc1)
    print("epoch value, first window: K=3 %.9g, K=1 frozen %.9g" % (v3, v1))
    assert np.isfinite(v3) and abs(v3 - v1) <= 1e-4 * abs(v1)
    assert enc1.engine.adam_step == 3 and enc1.engine._accum is None    # accum_steps = 1: no accumulator, ever


@pytest.mark.parametrize("value", [float("inf"), 1e18], ids=["inf", "1e18"])
def test_dynamic_scaler_skips_the_window_an_overflow_falls_into(data, value):
    from vpd_amd.models.util import DynamicLossScaler, step
    sd, img, tgt = data
    enc, tr = _build(sd, "fp16")
    eng = enc.engine
    opt = tr.get_optimizer(LR)[0]
    sc = DynamicLossScaler(eng, init_scale=256, growth_interval=10 ** 6)
    assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps) == (256.0, 0, 0)
    p0 = eng.params.clone()
    bad = tgt[MICRO[0]].clone()
    bad[1, 3] = value
    step(opt, sc, tr._forward_loss(img[MICRO[0]], bad, train=True), accumulate=True)         # micro-batch 1: poisoned
    assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps) == (256.0, 0, 0)               # no update() inside the window
    step(opt, sc, tr._forward_loss(img[MICRO[1]], tgt[MICRO[1]], train=True))                  # micro-batch 2: clean
    assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps) == (128.0, 1, 0)
    assert torch.equal(_bits(eng.params), _bits(p0))
    assert int((_bits(eng.adam_m) != 0).sum()) == 0 and int((_bits(eng.adam_v) != 0).sum()) == 0
    assert eng.adam_step == 0 and eng._accum_count == 0
    # a clean window applies one step; update() ran once per window
    step(opt, sc, tr._forward_loss(img[MICRO[0]], tgt[MICRO[0]], train=True), accumulate=True)
    step(opt, sc, tr._forward_loss(img[MICRO[1]], tgt[MICRO[1]], train=True))
    assert (sc.get_scale(), sc.skipped_steps, sc.applied_steps, sc.growth_tracker) == (128.0, 1, 1, 1)
    assert bool(torch.isfinite(eng.params).all()) and not torch.equal(eng.params, p0)


def test_clip_norm_is_the_norm_of_the_folded_gradients(data):
    """the pass sums in double and rounds once to float (2^-24 = 6e-8 relative), the reference below is float64 over the same
    values: 1e-6 relative is derived, not measured"""
    from vpd_amd.models.util import step
    sd, img, tgt = data
    enc, tr = _build(sd)
    eng = enc.engine
    opt, sc = tr.get_optimizer(LR, max_grad_norm=float("inf"))
    step(opt, sc, tr._forward_loss(img[MICRO[0]], tgt[MICRO[0]], train=True), accumulate=True)
    tr._forward_loss(img[MICRO[1]], tgt[MICRO[1]], train=True).backward_for_step()
    alone = float(torch.sqrt(sum((p.double() ** 2).sum() for p in _live(eng, True))))
    eng.fold_accumulated_grads()
    want = float(torch.sqrt(sum((p.double() ** 2).sum() for p in _live(eng, True))))
    opt.step()
    opt.zero_grad()
    got = opt.clip_stats()["total_norm"]
    print("clip: total_norm %.9g, float64 norm of the folded gradients %.9g (the last micro-batch alone: %.9g)" % (got, want, alone))
    assert abs(got - want) <= 1e-6 * want
    assert abs(alone - want) > 1e-3 * want                              # (the two are told apart)
    assert eng.adam_step == 1


def test_ema_updates_once_per_window(data):
    from vpd_amd.models.util import step
    sd, img, tgt = data
    enc, tr = _build(sd, ema_decay=0.9, accum_steps=2)
    eng = enc.engine
    opt, sc = tr.get_optimizer(LR)
    assert eng.ema_enabled and eng._ema_t == 0
    e0 = eng.ema_params.clone()
    step(opt, sc, tr._forward_loss(img[MICRO[0]], tgt[MICRO[0]], train=True), accumulate=True)
    torch.cuda.synchronize()
    assert eng._ema_t == 0 and torch.equal(_bits(eng.ema_params), _bits(e0))
    step(opt, sc, tr._forward_loss(img[MICRO[1]], tgt[MICRO[1]], train=True))
    torch.cuda.synchronize()
    assert eng._ema_t == 1 and not torch.equal(eng.ema_params, e0)
    tr.epoch(_batches(img, tgt, (0, 1, 2)), optimizer=opt, scaler=sc)   # windows of 2: steps at batches 2 and 3
    assert eng._ema_t == 3 and eng.adam_step == 3


# ---- two ranks on one GPU over gloo ----
GLOBAL = (slice(0, 6), slice(6, 10))          # the two micro-batches of the window, each sharded over the ranks


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main_accum(rank, world, port, q, ddp_lazy, overlap, glob):
    os.environ["VPD_DDP_LAZY"] = ddp_lazy
    os.environ["VPD_DDP_OVERLAP"] = overlap
    import torch.distributed as dist
    from vpd_amd.ddp import shard_slice
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import step
    from vpd_amd.trainer import ModelTrainer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        sd = O.procedural_state_dict(O.encoder_schema(ARCH, C_IN, D), 2)
        img, tgt = O.synthetic_crops(10, C_IN, HW, 3), O.synthetic_targets(10, D, False, 4)
        enc = RGBF_EmbeddingModel(ARCH, D, True, "cuda")
        enc.load_state_dict(sd)
        tr = ModelTrainer(enc, False, process_group=dist.group.WORLD)
        eng = enc.engine
        opt, sc = tr.get_optimizer(LR)
        calls = [0]
        plain = dist.all_reduce

        def counted(*a, **k):
            calls[0] += 1
            return plain(*a, **k)
        dist.all_reduce = counted
        shards = []
        for g in glob:
            sl = shard_slice(g.stop - g.start, rank, world)
            shards.append((img[g][sl], tgt[g][sl]))
        step(opt, sc, tr._forward_loss(*shards[0], train=True), accumulate=True)
        after_first = calls[0]
        loss = tr._forward_loss(*shards[1], train=True)
        loss.backward_for_step()                    # the window's last backward: fold + all-reduce (lazy unless VPD_DDP_LAZY=0)
        after_last = calls[0]
        held = eng._accum_count
        gsum = eng.grads.clone().cpu().numpy()      # (completes the flat buffer; the step below then reads it there)
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        assert eng.sync_errors() == 0
        q.put((rank, after_first, after_last, held, gsum, eng.params.clone().cpu().numpy(), int(eng.adam_step)))
    finally:
        dist.destroy_process_group()


RAGGED = (slice(0, 6), slice(6, 7))           # ... whose last micro-batch leaves rank 1 without crops


@pytest.mark.parametrize("ddp_lazy,overlap,glob", [("1", "1", GLOBAL), ("0", "1", GLOBAL), ("1", "0", GLOBAL), ("1", "1", RAGGED)],
                         ids=["lazy", "eager", "lazy_inline", "lazy_empty_shard"])
def test_two_ranks_reduce_once_per_window(data, ddp_lazy, overlap, glob):
    """K = 2 under data parallelism: the non-final micro-step starts no collective; the final one folds on the comm stream (or in
    line) and reduces; both ranks end with equal bits, and the summed gradient is that of one process accumulating the four
    shards (rel < 1e-3: two separately run backward passes, as tests/test_ddp_gpu.py).  lazy_empty_shard: rank 1 has no crop in
    the final micro-batch and folds onto the zeros its backward wrote."""
    import torch.multiprocessing as mp
    from vpd_amd.ddp import shard_slice
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main_accum, args=(r, 2, port, q, ddp_lazy, overlap, glob)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, first0, last0, held0, g0, w0, n0), (_, first1, last1, held1, g1, w1, n1) = res
    assert first0 == 0 and first1 == 0                                   # no collective on the non-final micro-step
    assert last0 == last1 and last0 > 0
    assert held0 == 0 and held1 == 0 and n0 == 1 and n1 == 1
    assert np.array_equal(g0, g1) and np.isfinite(g0).all()
    assert np.allclose(w0, w1, rtol=0, atol=1e-7)
    sd, img, tgt = data
    enc, tr = _build(sd)
    total = None
    for g in glob:
        for r in range(2):
            sl = shard_slice(g.stop - g.start, r, 2)
            if sl.stop == sl.start:
                continue                                                 # (an empty shard adds zeros)
            tr._forward_loss(img[g][sl], tgt[g][sl], train=True).backward()
            torch.cuda.synchronize()
            one = enc.engine.grads.clone().cpu().numpy()
            total = one if total is None else total + one
    rel = np.linalg.norm(g0 - total) / np.linalg.norm(total)
    print("two ranks, VPD_DDP_LAZY=%s VPD_DDP_OVERLAP=%s: %d collectives at the window's end, summed gradient rel %.3e" % (ddp_lazy, overlap, last0, rel))
    assert rel < 1e-3, rel
