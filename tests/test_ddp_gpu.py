"""The bucketed all-reduce path (HIP events recorded by vpd_backward -> side stream -> RCCL) on ONE GPU:
a world_size-1 nccl group makes SUM all-reduce the identity, so gradients and the loss trajectory must equal
the plain single-GPU run bit for bit, while every event / stream hand-off is exercised."""
import os

import numpy as np
import pytest
import torch

from oracle import vpd_oracle as O

pytestmark = pytest.mark.gpu


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bucket_reducer_world1_matches_plain_run():
    import torch.distributed as dist
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        sd = O.procedural_state_dict(O.encoder_schema("resnet18", 5, 32), 2)
        img = O.synthetic_crops(6, 5, 64, 3)
        tgt = O.synthetic_targets(6, 32, False, 4)
        res = []
        for use_group in (False, True):
            enc = RGBF_EmbeddingModel("resnet18", 32, True, "cuda")
            enc.load_state_dict(sd)
            tr = ModelTrainer(enc, False, process_group=dist.group.WORLD if use_group else None)
            assert (tr._reducer is not None) == use_group
            opt, sc = tr.get_optimizer(5e-4)
            enc.train()
            loss = tr._forward_loss(img, tgt, train=True)
            loss.backward()
            torch.cuda.synchronize()
            g = enc.engine.grads.clone()
            opt.step()
            traj = [tr.epoch([{"img": img, "emb": tgt}], optimizer=opt, scaler=sc) for _ in range(2)]
            res.append((g.cpu().numpy(), traj))
            if use_group:
                # the reducer takes its mode from the plan: a caller's word that disagrees is an error, not a
                # silent all-reduce of stale ranges
                # (compared with an EAGER backward + reduce of the same batch at the same weights -- a lazy reduce that
                #  summed stale flat-buffer ranges instead of the scratch would differ by the whole gradient, not by rounding)
                tr._forward_loss(img, tgt, train=True)
                pe = enc.engine.backward(tr._reducer.event_handles(len(enc.engine._last[0].buckets)), lazy=False)
                tr._reducer.reduce(pe)
                torch.cuda.synchronize()
                g_eager = enc.engine.grads.clone()
                enc.engine._grads.zero_()                   # nothing of the eager result may survive into the comparison
                tr._forward_loss(img, tgt, train=True)
                pl = enc.engine.backward(tr._reducer.event_handles(len(enc.engine._last[0].buckets)), lazy=True)
                with pytest.raises(RuntimeError):
                    tr._reducer.reduce(pl, lazy=False)
                tr._reducer.reduce(pl)                      # lazy, as the plan says
                enc.engine.materialize_grads()
                torch.cuda.synchronize()
                rel2 = float((enc.engine.grads - g_eager).norm() / g_eager.norm())
                assert rel2 < 1e-3, rel2                    # (fp32 atomics of the BatchNorm rows: summation order, ~1e-6)
        # BN statistics and the generic weight-gradient kernel use fp32 atomics (summation order varies run to run,
        # measured 1e-6 .. 3e-5 on these gradients): a tight tolerance, not bitwise
        rel = np.linalg.norm(res[0][0] - res[1][0]) / np.linalg.norm(res[0][0])
        assert rel < 1e-3, rel
        assert np.allclose(res[0][1], res[1][1], rtol=1e-3)
    finally:
        dist.destroy_process_group()


def _rank_main_ragged(rank, world, port, q, ddp_lazy="1", overlap="1"):
    """An epoch whose last batch leaves rank 1 without crops: batches of 6 (3 + 3) and 1 (1 + 0) crops."""
    os.environ["VPD_DDP_LAZY"] = ddp_lazy          # 1: the reducer sums the weight-gradient scratch ranges (default); 0: flat buffer
    os.environ["VPD_DDP_OVERLAP"] = overlap
    import torch.distributed as dist
    from vpd_amd.ddp import shard_slice
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        sd = O.procedural_state_dict(O.encoder_schema("resnet18", 5, 32), 2)
        img = O.synthetic_crops(7, 5, 64, 3)
        tgt = O.synthetic_targets(7, 32, False, 4)
        enc = RGBF_EmbeddingModel("resnet18", 32, True, "cuda")
        enc.load_state_dict(sd)
        tr = ModelTrainer(enc, False, process_group=dist.group.WORLD)
        opt, sc = tr.get_optimizer(5e-4)
        batches = []
        for lo, hi in ((0, 6), (6, 7)):
            sl = shard_slice(hi - lo, rank, world)
            batches.append({"img": img[lo:hi][sl], "emb": tgt[lo:hi][sl]})
        assert batches[1]["img"].shape[0] == (1 if rank == 0 else 0)
        ep = tr.epoch(batches, optimizer=opt, scaler=sc)
        torch.cuda.synchronize()
        assert enc.engine.sync_errors() == 0
        q.put((rank, enc.engine.grads.clone().cpu().numpy(), ep, enc.engine.params.clone().cpu().numpy(),
               int(enc.engine.num_batches_tracked[0].item())))
    finally:
        dist.destroy_process_group()


def test_lazy_gradients_under_data_parallelism_equal_the_eager_path():
    """VERDICT r2 #5a: with a reducer the conv weight gradients stay in the weight-gradient kernels' scratch layout and the
    reducer sums THOSE ranges (+ one small message for BatchNorm / fc / stem): a SUM all-reduce is layout-agnostic
    (train_vpd_model.py:87).  Two ranks on this GPU over gloo, two optimizer steps incl. the zero-crop batch: the parameters
    equal the eager flat-buffer path (VPD_DDP_LAZY=0) bit for bit, on both ranks, with and without comm / compute overlap."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    runs = {}
    for tag, lazy, overlap, port in (("eager", "0", "1", _free_port()), ("lazy", "1", "1", _free_port()), ("lazy_inline", "1", "0", _free_port())):
        q = ctx.Queue()
        procs = [ctx.Process(target=_rank_main_ragged, args=(r, 2, port, q, lazy, overlap)) for r in range(2)]
        for p in procs:
            p.start()
        res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        runs[tag] = res
        print("VPD_DDP_LAZY=%s VPD_DDP_OVERLAP=%s epoch value %.6f" % (lazy, overlap, res[0][2]))
    for tag in ("lazy", "lazy_inline"):
        for r in range(2):
            assert np.array_equal(runs[tag][r][3], runs["eager"][r][3]), (tag, r)      # parameters after the epoch
            assert runs[tag][r][2] == runs["eager"][r][2]                               # all-reduced epoch value
    assert np.array_equal(runs["lazy"][0][3], runs["lazy"][1][3])                       # replicas agree


def test_zero_crop_rank_joins_the_collective():
    """a rank with an empty shard of the ragged last batch still takes part in the step: vpd_forward_train /
    vpd_backward accept n = 0 (zero loss, zero gradients, bucket events recorded), both ranks end the epoch with the
    SAME gradients (rank 0's, since rank 1 added zeros), the same weights and the same epoch value over 7 crops."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main_ragged, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, g0, ep0, w0, nbt0), (_, g1, ep1, w1, nbt1) = res
    assert np.array_equal(g0, g1) and np.isfinite(g0).all() and np.abs(g0).max() > 0
    assert ep0 == ep1 and np.isfinite(ep0)
    assert np.allclose(w0, w1, rtol=0, atol=1e-7)
    assert (nbt0, nbt1) == (2, 1)               # the empty batch is not a BatchNorm step on rank 1


def _rank_main(rank, world, port, q, dtype="bf16"):
    import torch.distributed as dist
    from vpd_amd.ddp import shard_slice
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)      # gloo moves the CUDA buckets through the host
    try:
        torch.cuda.set_device(0)
        sd = O.procedural_state_dict(O.encoder_schema("resnet18", 5, 32), 2)
        img = O.synthetic_crops(10, 5, 64, 3)
        tgt = O.synthetic_targets(10, 32, False, 4)
        sl = shard_slice(10, rank, world)
        enc = RGBF_EmbeddingModel("resnet18", 32, True, "cuda", dtype=dtype)
        enc.load_state_dict(sd)
        tr = ModelTrainer(enc, False, process_group=dist.group.WORLD)
        opt, sc = tr.get_optimizer(5e-4)
        assert (sc is None) == (dtype == "bf16")
        enc.train()
        loss = tr._forward_loss(img[sl], tgt[sl], train=True)
        loss.backward()
        torch.cuda.synchronize()
        g = enc.engine.grads.clone().cpu().numpy()
        ep = tr.epoch([{"img": img[sl], "emb": tgt[sl]}], optimizer=opt, scaler=sc)      # all-reduced loss / count
        w = enc.engine.params.clone().cpu().numpy()
        q.put((rank, g, ep, w))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_two_ranks_on_one_gpu_sum_their_shard_gradients(dtype):
    """world_size 2 (two processes, both on this GPU, gloo transport): after the bucketed all-reduce every rank holds
    the SUM of the two shards' gradients (per-shard BatchNorm statistics, as SURVEY 8e), the epoch value is the
    global sum-MSE per crop, and both ranks take the same AdamW step.  fp16: the step inside epoch() runs through the
    LossScaler -- the reducer sums gradients that are 256 x their value and the fused AdamW reads them x 1 / 256."""
    import torch.multiprocessing as mp
    from vpd_amd.ddp import shard_slice
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q, dtype)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, g0, ep0, w0), (_, g1, ep1, w1) = res
    assert np.array_equal(g0, g1) and ep0 == ep1
    assert np.allclose(w0, w1, rtol=0, atol=1e-7)
    # single-process emulation: each shard alone (its own batch statistics), gradients summed
    sd = O.procedural_state_dict(O.encoder_schema("resnet18", 5, 32), 2)
    img, tgt = O.synthetic_crops(10, 5, 64, 3), O.synthetic_targets(10, 32, False, 4)
    total, loss_sum = None, 0.0
    for r in range(2):
        sl = shard_slice(10, r, 2)
        enc = RGBF_EmbeddingModel("resnet18", 32, True, "cuda", dtype=dtype)
        enc.load_state_dict(sd)
        tr = ModelTrainer(enc, False)
        enc.train()
        loss = tr._forward_loss(img[sl], tgt[sl], train=True)
        loss_sum += loss.item()
        loss.backward()
        torch.cuda.synchronize()
        g = enc.engine.grads.clone().cpu().numpy()
        total = g if total is None else total + g
    rel = np.linalg.norm(g0 - total) / np.linalg.norm(total)
    assert rel < 1e-3, rel                      # fp32 atomics: order of summation varies run to run (measured ~1e-6)
    assert abs(ep0 - loss_sum / 10) <= 1e-4 * abs(ep0)


def _rank_main_bottleneck(rank, world, port, q):
    """ResNet-50 student, reducer attached: every BatchNorm backward of a Bottleneck student is a grid-barrier launch (42 per
    step), the bucket all-reduces run on the comm stream beside them."""
    import torch.distributed as dist
    from vpd_amd.ddp import shard_slice
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        sd = O.procedural_state_dict(O.encoder_schema("resnet50", 5, 32), 12)
        img, tgt = O.synthetic_crops(12, 5, 64, 13), O.synthetic_targets(12, 32, False, 14)
        sl = shard_slice(12, rank, world)
        enc = RGBF_EmbeddingModel("resnet50", 32, True, "cuda")
        enc.load_state_dict(sd)
        tr = ModelTrainer(enc, False, process_group=dist.group.WORLD)
        assert tr._reducer is not None
        opt, sc = tr.get_optimizer(5e-4)
        eps = [tr.epoch([{"img": img[sl], "emb": tgt[sl]}], optimizer=opt, scaler=sc) for _ in range(3)]
        torch.cuda.synchronize()
        assert enc.engine.sync_errors() == 0
        q.put((rank, eps, enc.engine.params.clone().cpu().numpy(), bool(tr._reducer.overlap)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_a_bottleneck_student_with_the_reducer_attached():
    """the grid-barrier BatchNorm launches of a Bottleneck student and the comm stream's bucket all-reduces
    together, two ranks sharing this GPU: no barrier time-out, replicas bit-identical after three steps, finite losses that
    both ranks agree on and that go down."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main_bottleneck, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, e0, w0, ov0), (_, e1, w1, ov1) = res
    assert ov0 and ov1                                     # overlapped path (the default)
    assert e0 == e1 and np.isfinite(e0).all() and e0[2] < e0[0]
    assert np.array_equal(w0, w1)


def test_train_cli_two_ranks_keep_identical_replicas(tmp_path):
    """train_vpd_model.py under two ranks (both on this GPU, gloo) with the motion head: the CLI broadcasts rank 0's
    initial weights (encoder AND motion head), all-reduces the gradients, and at the end compares a parameter checksum
    across ranks -- a diverged replica makes the run fail."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "run")
    env = dict(os.environ, VPD_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2",
               LOCAL_RANK="0")
    args = [sys.executable, os.path.join(root, "train_vpd_model.py"), "diving48", "--save_dir", out, "--flow_img", "flow",
            "--synthetic", "64", "--num_epochs", "2", "--batch_size", "16", "--motion", "--encoder_arch", "resnet18"]
    procs = [subprocess.Popen(args, env=dict(env, RANK=str(r)), cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode(errors="replace") for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert os.path.exists(os.path.join(out, "epoch0002.encoder.pt")) and os.path.exists(os.path.join(out, "epoch0002.decoder.pt"))


def test_bench_self_launches_two_ranks_from_a_bare_shell():
    """`python bench.py --gpus 2` with no torchrun environment spawns its own ranks (before anything
    touches the GPU) and rank 0 prints the one JSON line.  On this 1-GPU box the ranks share the device and exchange
    the gradient buckets over gloo; on an 8-GPU node the same command runs RCCL (backend "nccl")."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["VPD_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full",
                        "--repeats", "2", "--batch", "16", "--profile-steps", "1", "--no-cpu-baseline", "--no-apply"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 32 and out["scaling"] == "weak"
    assert out["steps"] == 3 and out["repeats"]["n"] == 2 and out["value"] > 0 and np.isfinite(out["config"]["loss_last_step"])
    # the multi-GPU leg validates itself: communicator as it reports itself, bus bandwidth of an all-reduce of
    # every gradient bucket's size, and the same steps with the all-reduces not overlapped with backward
    mg = out["multi_gpu"]
    assert mg["backend"] == "gloo" and mg["world_size"] == 2 and mg["lazy_gradients"] is True
    assert len(mg["allreduce_per_bucket"]) == 4 and all(b["busbw_GBps"] > 0 and b["ms"] > 0 for b in mg["allreduce_per_bucket"])
    assert abs(sum(b["MB"] for b in mg["allreduce_per_bucket"]) - 21.36 * 4) < 1.0      # the ResNet-34 student's 21.4 M parameters
    assert mg["ms_per_step_overlap_on"] > 0 and mg["ms_per_step_overlap_off"] > 0
    # configs[2] under its own name: 6-channel input + motion head, 2 ranks
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--config", "c3", "--steps", "2", "--warmup", "1",
                        "--repeats", "1", "--batch", "8", "--profile-steps", "0", "--no-cpu-baseline", "--no-apply"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out3 = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out3["config"]["workload"].startswith("configs[2]") and out3["config"]["global_batch"] == 16
    assert np.isfinite(out3["config"]["loss_last_step"]) and out3["config"]["flop_per_crop"] > out["config"]["flop_per_crop"]
    # a failing rank fails the launcher
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--arch", "no_such_arch", "--no-cpu-baseline", "--no-apply"], cwd=root, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0


def _rank_main_c4(rank, world, port, q, early):
    """BASELINE configs[3] per rank (fs normalisation, motion head, ResNet-34), scaled to 64 crops per rank so that four ranks share the
    one GPU of this box: one full global batch and the RAGGED final one (3,616 = 8 x 452 in the config; here 4 x 57 of 4 x 64)
    through ModelTrainer.epoch with the bucket reducer attached."""
    import hashlib
    import torch.distributed as dist
    from vpd_amd.data import RGB_MEAN_STD
    from vpd_amd.ddp import shard_slice
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    import bench
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["VPD_DDP_EARLY_BUCKET0"] = early
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        torch.manual_seed(0)
        enc = RGBF_EmbeddingModel("resnet34", bench.EMB_DIM, True, "cuda")
        enc.reset_parameters(seed=0)
        tr = ModelTrainer(enc, True, process_group=dist.group.WORLD)
        dist.broadcast(enc.engine.params, 0)            # the motion head is initialised in the trainer: rank 0's everywhere
        enc.engine.mark_weights_changed()
        opt, sc = tr.get_optimizer(5e-4)
        per, ragged = 64, 57
        batches = []
        for gb, n in ((0, per * world), (1, ragged * world)):
            img, emb = bench.synthetic_batch(n, "cuda", seed=10 + gb, c_in=5, mean_std=RGB_MEAN_STD["fs"], target_dim=2 * bench.EMB_DIM)
            sl = shard_slice(n, rank, world)
            batches.append({"img": img[sl], "emb": emb[sl]})
        ep = tr.epoch(batches, optimizer=opt, scaler=sc)
        torch.cuda.synchronize()
        assert enc.engine.sync_errors() == 0
        pl = enc.engine._step_plan
        digest = hashlib.sha256(enc.engine.params.cpu().numpy().tobytes()).hexdigest()
        q.put((rank, ep, digest, bool(pl.early_bucket0), int(batches[1]["img"].shape[0])))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("early", ["0"], ids=["bucket0_merged"])      # (bucket 0 early: test_bench_c4_four_ranks_reports_its_multi_gpu_block)
def test_four_ranks_ragged_final_batch_keep_identical_replicas(early):
    """VERDICT r4 #7 (as far as one GPU goes: the pool allows at most six processes on a card and the test runner is one of them,
    so four ranks here; all eight run on the CPU in tests/test_ddp_cpu.py::test_eight_ranks_ragged_final_batch_and_lazy_exchange): the
    configs[3] recipe -- fs normalisation, motion head -- over a full and a ragged global batch through ModelTrainer.epoch, every rank
    with the reducer attached and lazy gradients; all replicas hold the same bits afterwards, the epoch value is the same on
    every rank, and the data-parallel creation flag (layer4's weight gradients launched at layer4's end: bucket 0 early) is set
    with VPD_DDP_EARLY_BUCKET0=1 and not otherwise (the flag only moves launches: the two settings agree to rounding)."""
    import torch.multiprocessing as mp
    world = 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main_c4, args=(r, world, port, q, early)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=900) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert len({r[2] for r in res}) == 1, [r[2][:12] for r in res]          # bit-identical replicas
    assert len({r[1] for r in res}) == 1 and np.isfinite(res[0][1])           # the all-reduced epoch value
    assert all(r[3] == (early == "1") for r in res)
    assert all(r[4] == 57 for r in res)
    # (the two settings split layer3 / layer4's weight-gradient sums over blocks differently -- the cost model sees other launches --
    #  so their fp32 partial sums round differently: the epoch values agree closely, the bits need not)
    _C4_EPOCH[early] = res[0][1]
    if len(_C4_EPOCH) == 2:
        assert abs(_C4_EPOCH["1"] / _C4_EPOCH["0"] - 1) < 1e-3, _C4_EPOCH


_C4_EPOCH = {}


def test_bench_c4_four_ranks_reports_its_multi_gpu_block():
    """`bench.py --config c4 --gpus 4 --full` (gloo, shared GPU, 32 crops per rank): one JSON line whose multi_gpu block is well formed --
    backend, world size, per-bucket all-reduce timings, overlap on / off, the early-bucket-0 flag and `replicas_identical`."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["VPD_DIST_BACKEND"] = "gloo"
    env["VPD_DDP_EARLY_BUCKET0"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--config", "c4", "--steps", "2", "--warmup", "1",
                        "--full", "--repeats", "1", "--batch", "32", "--profile-steps", "0", "--no-cpu-baseline", "--no-apply"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 4 and out["config"]["global_batch"] == 128 and out["config"]["workload"].startswith("configs[3]")
    mg = out["multi_gpu"]
    assert mg["backend"] == "gloo" and mg["world_size"] == 4 and mg["lazy_gradients"] is True
    assert mg["early_bucket0"] is True and mg["replicas_identical"] is True      # (VPD_DDP_EARLY_BUCKET0=1 in this run's environment)
    assert len(mg["allreduce_per_bucket"]) == 4 and all(b["busbw_GBps"] > 0 for b in mg["allreduce_per_bucket"])
    assert mg["ms_per_step_overlap_on"] > 0 and mg["ms_per_step_overlap_off"] > 0
