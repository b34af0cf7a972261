#!/usr/bin/env python3
"""What the dynamic loss scaler costs per step, against the static one, in ONE process and one call:

  ResNet-34 student, 256 crops of 5 x 128 x 128, fp16 elements, fused AdamW (bench.py's flagship workload with --dtype fp16).
  Two trainers from the same initial weights, one behind LossScaler(256) and one behind DynamicLossScaler(256); after both are
  warm, regions of --steps steps alternate static, dynamic, static, dynamic ...  A region is timed with device events, with one
  synchronise at its end.  Printed: every region, the spread among the static regions (the yardstick's own noise), and the
  dynamic-minus-static difference, which counts as real only where it exceeds that spread.

  --trace-steps N: instead, run N dynamic steps (after warm-up) and exit -- the command to put behind
  `rocprofv3 --kernel-trace --stats` for check_finite_kernel's own time; tools/bench_loss_scale.py --kernel-stats <csv> then prints
  its achieved bytes/s."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FABRIC_TBPS = 8.0          # the HBM3E figure the project quotes its bandwidth shares against


def kernel_stats(path, numel):
    rows = list(csv.DictReader(open(path)))
    print("kernel                                   calls   avg us   share of the trace")
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        if any(k in name for k in ("check_finite_kernel", "scale_update_kernel", "scale_by_state_kernel", "adamw_pack_kernel")):
            avg_us = float(r["AverageNs"]) / 1e3
            print("%-40s %5d %8.2f   %5.2f %%" % (name[:40], int(r["Calls"]), avg_us, float(r["Percentage"])))
            if "check_finite_kernel" in name:
                bps = numel * 4 / (avg_us * 1e-6)
                print("  check_finite_kernel reads %d fp32 gradients = %.1f MB per call: %.2f TB/s achieved, %.0f %% of the %.0f TB/s figure"
                      % (numel, numel * 4 / 1e6, bps / 1e12, 100 * bps / (FABRIC_TBPS * 1e12), FABRIC_TBPS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=6, help="timed regions per scaler (at least 5)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--kernel-stats", type=str, help="a rocprofv3 kernel_stats.csv of a --trace-steps run: print the new kernels' rows")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, 21356608)
    if args.regions < 5 and not args.trace_steps:
        ap.error("--regions must be at least 5")

    import torch
    import bench
    from vpd_amd.data import RGB_MEAN_STD
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import DynamicLossScaler, LossScaler, step
    from vpd_amd.trainer import ModelTrainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_scale.py measures on the GPU: none found")
    device = "cuda"
    img, emb = bench.synthetic_batch(args.batch, device, seed=1, c_in=5, mean_std=RGB_MEAN_STD["diving48"], target_dim=bench.EMB_DIM)

    def make(dynamic):
        torch.manual_seed(0)
        enc = RGBF_EmbeddingModel("resnet34", bench.EMB_DIM, True, device, dtype="fp16")
        enc.reset_parameters(seed=0)
        tr = ModelTrainer(enc, motion=False)
        opt = tr.get_optimizer(5e-4)[0]
        sc = DynamicLossScaler(enc.engine, init_scale=256.0) if dynamic else LossScaler(enc.engine, 256.0)
        enc.train()
        return enc, tr, opt, sc

    def run(m, n):
        _, tr, opt, sc = m
        for _ in range(n):
            step(opt, sc, tr._forward_loss(img, emb, train=True))

    dyn = make(True)
    if args.trace_steps:
        run(dyn, args.warmup)
        torch.cuda.synchronize()
        run(dyn, args.trace_steps)
        torch.cuda.synchronize()
        print(json.dumps({"traced_dynamic_steps": args.trace_steps, "scale": dyn[3].get_scale(), "skipped": dyn[3].skipped_steps,
                          "applied": dyn[3].applied_steps, "param_numel": dyn[0].engine.param_numel}))
        return
    sta = make(False)
    for m in (sta, dyn):
        run(m, args.warmup)
    torch.cuda.synchronize()
    times = {"static": [], "dynamic": []}
    for r in range(args.regions):
        for tag, m in (("static", sta), ("dynamic", dyn)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(m, args.steps)
            b.record()
            b.synchronize()
            times[tag].append(a.elapsed_time(b) * 1e3 / args.steps)      # us per step
            print("region %2d %-7s %9.2f us/step" % (r, tag, times[tag][-1]))
    med = lambda v: sorted(v)[len(v) // 2]
    s, d = times["static"], times["dynamic"]
    spread = max(s) - min(s)
    diff = med(d) - med(s)
    pair = [y - x for x, y in zip(s, d)]
    print("static : median %.2f us/step, min %.2f, max %.2f, spread %.2f us (%.2f %%)" % (med(s), min(s), max(s), spread, 100 * spread / med(s)))
    print("dynamic: median %.2f us/step, min %.2f, max %.2f" % (med(d), min(d), max(d)))
    print("dynamic - static: %.2f us/step (%.2f %% of the static step); per adjacent pair: %s"
          % (diff, 100 * diff / med(s), " ".join("%.2f" % p for p in pair)))
    print("the difference %s the static regions' own spread" % ("exceeds" if abs(diff) > spread else "is within"))
    sc = dyn[3]
    print("dynamic scaler at the end: scale %g, applied %d, skipped %d; losses static %.4f dynamic %.4f"
          % (sc.get_scale(), sc.applied_steps, sc.skipped_steps, float(sta[0].engine.loss_step.item()),
             float(dyn[0].engine.loss_step.item())))


if __name__ == "__main__":
    main()
