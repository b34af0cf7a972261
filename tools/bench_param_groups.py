#!/usr/bin/env python3
"""What AdamW parameter groups cost per step, in ONE process and one call:

  ResNet-34 student, 256 crops of 5 x 128 x 128, fused AdamW (bench.py's flagship workload).  For bf16 (no scaler) and for fp16
  behind a DynamicLossScaler, one trainer each and TWO optimizers over its parameters: the one-group step (the launches of always)
  and the grouping of `--no_bn_bias_decay --backbone_lr_scale 0.1` (ModelTrainer.param_groups: four groups, the grouped
  instantiation of adamw_pack_kernel).  After both are warm, regions of --steps steps alternate one group, groups, one group ...
  A region is timed with device events, with one synchronise at its end.  Printed: every region, the spread among the one-group
  regions (the yardstick's own noise) and the groups-minus-one-group difference, which counts as real only where it exceeds that
  spread.  Both optimizers step the same parameters and moments: the regions differ in the AdamW launch and in nothing else."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=5, help="timed regions per setting (at least 3)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    if args.regions < 3:
        ap.error("--regions must be at least 3")

    import torch
    import bench
    from vpd_amd.data import RGB_MEAN_STD
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import step
    from vpd_amd.trainer import FusedAdamW, ModelTrainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_param_groups.py measures on the GPU: none found")
    device = "cuda"
    img, emb = bench.synthetic_batch(args.batch, device, seed=1, c_in=5, mean_std=RGB_MEAN_STD["diving48"], target_dim=bench.EMB_DIM)
    med = lambda v: sorted(v)[len(v) // 2]

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(n)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / n      # us per iteration

    for dtype in ("bf16", "fp16"):
        torch.manual_seed(0)
        enc = RGBF_EmbeddingModel("resnet34", bench.EMB_DIM, True, device, dtype=dtype)
        enc.reset_parameters(seed=0)
        tr = ModelTrainer(enc, motion=False)
        loss_scale = "dynamic" if dtype == "fp16" else None
        one, scaler = tr.get_optimizer(5e-4, loss_scale=loss_scale)
        groups = tr.param_groups(weight_decay=0.01, decay_bn_bias=False, backbone_lr_scale=0.1, lr=5e-4)
        many = FusedAdamW(groups, enc.engine, lr=5e-4)      # (the scaler is the trainer's one: get_optimizer would make a second)
        eng = enc.engine
        enc.train()
        name = "bf16" if dtype == "bf16" else "fp16 dynamic"
        opts = {"one": one, "groups": many}

        def run(opt):
            def go(n):
                for _ in range(n):
                    step(opt, scaler, tr._forward_loss(img, emb, train=True))
            return go

        run(one)(args.warmup)
        run(many)(args.warmup)
        torch.cuda.synchronize()
        nseg = len(many._groups()["seg_group"])
        print("%s: %d groups %s, %d segments; table builds %d" % (name, len(groups), [(g["lr"], g["weight_decay"]) for g in groups], nseg,
                                                                  eng.group_table_builds))
        times = {"one": [], "groups": []}
        for r in range(args.regions):
            for tag in ("one", "groups"):
                torch.cuda.synchronize()
                times[tag].append(timed(run(opts[tag]), args.steps))
                print("%s region %2d %-6s %9.2f us/step" % (name, r, tag, times[tag][-1]))
        off, on = times["one"], times["groups"]
        spread = max(off) - min(off)
        diff = med(on) - med(off)
        print("%s one group: median %.2f us/step, min %.2f, max %.2f, spread %.2f us (%.2f %%)"
              % (name, med(off), min(off), max(off), spread, 100 * spread / med(off)))
        print("%s groups   : median %.2f us/step, min %.2f, max %.2f" % (name, med(on), min(on), max(on)))
        print("%s groups - one group: %.2f us/step (%.2f %% of the step); per adjacent pair: %s"
              % (name, diff, 100 * diff / med(off), " ".join("%.2f" % (y - x) for x, y in zip(off, on))))
        print("%s: the difference %s the one-group regions' own spread" % (name, "exceeds" if abs(diff) > spread else "is within"))
        print("%s: loss of the last step %.4f, table builds %d%s" % (name, float(eng.loss_step.item()), eng.group_table_builds,
              "" if scaler is None or not hasattr(scaler, "skipped_steps") else "; loss scale %g, skipped %d" % (scaler.get_scale(), scaler.skipped_steps)))
        del enc, tr, one, many, scaler, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
