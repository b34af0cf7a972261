#!/usr/bin/env python3
"""What a train step through torch autograd costs against the fused step, in ONE process and one call (the method of
tools/bench_loss_scale.py):

  ResNet-34 student, 256 crops of 5 x 128 x 128, bf16 elements (bench.py's flagship workload).  Three students from the same
  initial weights:
    fused     ModelTrainer's step: forward + sum-MSE + lazy backward + FusedAdamW, no torch in between
    autograd  enc(img); F.mse_loss(reduction='sum'); loss.backward(); FusedAdamW.step(); zero_grad()
    autograd+dx  the same with img.requires_grad (the stem convolution's data gradient is launched too)
    frozen       autograd+dx after freeze_bn(): BatchNorm on running statistics (the same launches, no statistics update)
    frozen-noopt frozen without the optimizer step (backward + zero_grad only): what frozen-data is to be compared with
    frozen-data  frozen with every parameter requires_grad_(False): d(loss)/d(img) alone (vpd_plan_set_param_grads(0): no
                 weight-gradient launch, no optimizer step -- the gradient of a fixed student)
  The frozen students first take --warmup train-mode steps, so that their running statistics are those of a trained network and not
  the 0 / 1 of a fresh one (activations that vanish or blow up run at other clocks on a power-limited device).
  After all are warm, regions of --steps steps alternate fused, autograd, autograd+dx, frozen, frozen-noopt, frozen-data, fused, ...  A region is timed with device
  events, with one synchronise at its end.  Printed: every region, the spread among the fused regions (the yardstick's own noise)
  and the differences, which count as real only where they exceed that spread.

  --trace-steps N: instead, run N autograd+dx steps (after warm-up) and exit -- the command to put behind
  `rocprofv3 --kernel-trace --stats` for conv_stem_dgrad_kernel's own time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--regions", type=int, default=5, help="timed regions per kind (at least 5)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--trace-steps", type=int, default=0)
    args = ap.parse_args()
    if args.regions < 5 and not args.trace_steps:
        ap.error("--regions must be at least 5")

    import torch
    import torch.nn.functional as F
    import bench
    from vpd_amd.boxid import gpu_unique_id
    from vpd_amd.data import RGB_MEAN_STD
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import step
    from vpd_amd.trainer import ModelTrainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_autograd_step.py measures on the GPU: none found")
    device = "cuda"
    img, emb = bench.synthetic_batch(args.batch, device, seed=1, c_in=5, mean_std=RGB_MEAN_STD["diving48"], target_dim=bench.EMB_DIM)
    img_dx = img.clone().requires_grad_()

    def make(kind="fused"):
        torch.manual_seed(0)
        enc = RGBF_EmbeddingModel("resnet34", bench.EMB_DIM, True, device)
        enc.reset_parameters(seed=0)
        tr = ModelTrainer(enc, motion=False)
        opt = tr.get_optimizer(5e-4)[0]
        enc.train()
        return enc, tr, opt

    def freeze(kind, m):
        m[0].freeze_bn()
        if kind == "frozen-data":
            for q in m[0].parameters():
                q.requires_grad_(False)

    def run(kind, m, n):
        enc, tr, opt = m
        for _ in range(n):
            if kind == "fused":
                step(opt, None, tr._forward_loss(img, emb, train=True))
            elif kind in ("frozen-data", "frozen-noopt"):
                F.mse_loss(enc(img_dx), emb, reduction="sum").backward()
                opt.zero_grad()
                img_dx.grad = None
            else:
                x = img if kind == "autograd" else img_dx
                F.mse_loss(enc(x), emb, reduction="sum").backward()
                opt.step()
                opt.zero_grad()
                if x.grad is not None:
                    x.grad = None

    kinds = ("fused", "autograd", "autograd+dx", "frozen", "frozen-noopt", "frozen-data")
    if args.trace_steps:
        m = make()
        run("autograd+dx", m, args.warmup)
        torch.cuda.synchronize()
        run("autograd+dx", m, args.trace_steps)
        torch.cuda.synchronize()
        print(json.dumps({"traced_autograd_dx_steps": args.trace_steps, "stem_dgrad_launches": m[0].engine.stem_dgrad_launches}))
        return
    ms = {k: make(k) for k in kinds}
    for k in kinds:
        if k.startswith("frozen"):
            run("autograd", ms[k], args.warmup)      # train-mode steps: realistic running statistics to freeze
            freeze(k, ms[k])
        run(k, ms[k], args.warmup)
    torch.cuda.synchronize()
    print("box", gpu_unique_id(0))
    times = {k: [] for k in kinds}
    for r in range(args.regions):
        for k in kinds:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(k, ms[k], args.steps)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / args.steps)      # us per step
            print("region %2d %-12s %9.2f us/step" % (r, k, times[k][-1]))
    med = lambda v: sorted(v)[len(v) // 2]
    f = times["fused"]
    spread = max(f) - min(f)
    print("fused      : median %.2f us/step, min %.2f, max %.2f, spread %.2f us (%.2f %%)" % (med(f), min(f), max(f), spread, 100 * spread / med(f)))
    for k in kinds[1:]:
        d = med(times[k]) - med(f)
        print("%-11s: median %.2f us/step, min %.2f, max %.2f; minus fused: %.2f us/step (%.2f %% of the fused step), which %s the fused regions' own spread"
              % (k, med(times[k]), min(times[k]), max(times[k]), d, 100 * d / med(f), "exceeds" if abs(d) > spread else "is within"))
    print("autograd+dx - autograd: %.2f us/step" % (med(times["autograd+dx"]) - med(times["autograd"])))
    a = times["autograd+dx"]
    n = times["frozen-noopt"]
    print("frozen - autograd+dx: %.2f us/step (autograd+dx's own spread: %.2f us); frozen-data - frozen-noopt: %.2f us/step (frozen-noopt's own spread: %.2f us)"
          % (med(times["frozen"]) - med(a), max(a) - min(a), med(times["frozen-data"]) - med(n), max(n) - min(n)))
    print("fused loss at the end: %.4f" % float(ms["fused"][0].engine.loss_step.item()))
    assert all(ms[k][0].engine.sync_errors() == 0 for k in kinds)


if __name__ == "__main__":
    main()
