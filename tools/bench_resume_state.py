#!/usr/bin/env python3
"""What a resumable state costs: ModelTrainer.save_state / load_state by wall clock, and the file's size.

  ResNet-34 student, 256 crops of 5 x 128 x 128, fused AdamW with the EMA on (bench.py's flagship workload plus the average), --dtype
  bf16 or fp16 (fp16: behind a DynamicLossScaler).  After --warmup steps (the moments exist, the average has moved) a region of
  --steps steps is timed with device events -- the step time the ratios are quoted against -- then --reps times: synchronise,
  save_state into --dir (wall clock around the call, which ends with the file in place), synchronise, load_state from it (wall
  clock, then a synchronise inside the timed span: the copies to the device are part of it).  The file is written where --dir
  says: the figures are those of that file system.  Nothing here touches a kernel: the time is device-to-host copies, pickling and
  the file."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the state file is written (default: a temporary directory)")
    args = ap.parse_args()

    import torch
    import bench
    from vpd_amd.data import RGB_MEAN_STD
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import step
    from vpd_amd.trainer import ModelTrainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_resume_state.py measures on the GPU: none found")
    device = "cuda"
    img, emb = bench.synthetic_batch(args.batch, device, seed=1, c_in=5, mean_std=RGB_MEAN_STD["diving48"], target_dim=bench.EMB_DIM)
    torch.manual_seed(0)
    enc = RGBF_EmbeddingModel("resnet34", bench.EMB_DIM, True, device, dtype=args.dtype)
    enc.reset_parameters(seed=0)
    tr = ModelTrainer(enc, motion=False, ema_decay=0.999)
    opt, scaler = tr.get_optimizer(5e-4, loss_scale="dynamic" if args.dtype == "fp16" else None)
    eng = enc.engine
    enc.train()

    def run(n):
        for _ in range(n):
            step(opt, scaler, tr._forward_loss(img, emb, train=True))

    run(args.warmup)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(args.steps)
    e1.record()
    e1.synchronize()
    step_ms = e0.elapsed_time(e1) / args.steps
    print("%s step: %.3f ms (%d steps between two events, %d crops)" % (args.dtype, step_ms, args.steps, args.batch))

    med = lambda v: sorted(v)[len(v) // 2]
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, "train_state.pt")
        saves, loads = [], []
        for r in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.save_state(path, opt, scaler, extra={"epoch": r})
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            extra = tr.load_state(path, opt, scaler)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            assert extra == {"epoch": r}
            saves.append((t1 - t0) * 1e3)
            loads.append((t3 - t2) * 1e3)
            print("rep %d: save_state %8.1f ms   load_state %8.1f ms" % (r, saves[-1], loads[-1]))
        size = os.path.getsize(path)
        assert os.listdir(d) == ["train_state.pt"]
    print("file: %d bytes (%.1f MB); flat parameter buffer %d floats (%.1f MB): parameters, two moments and the average are four of them"
          % (size, size / 1e6, eng.param_numel, 4.0 * eng.param_numel / 1e6))
    print("save_state: median %.1f ms, min %.1f, max %.1f = %.1f steps" % (med(saves), min(saves), max(saves), med(saves) / step_ms))
    print("load_state: median %.1f ms, min %.1f, max %.1f = %.1f steps" % (med(loads), min(loads), max(loads), med(loads) / step_ms))
    run(2)      # the restored trainer steps on
    torch.cuda.synchronize()
    print("loss of the last step %.4f; optimizer steps applied %d" % (float(eng.loss_step.item()), eng.adam_step))


if __name__ == "__main__":
    main()
