#!/usr/bin/env python3
"""What the weight average costs per step, in ONE process and one call:

  ResNet-34 student, 256 crops of 5 x 128 x 128, bf16 elements, fused AdamW (bench.py's flagship workload).  One trainer; after it
  is warm, regions of --steps steps alternate EMA off, on, off, on ...  (off: StudentEngine.disable_ema(), the step launches what
  it launched before the feature; on: enable_ema(0.999), one more launch per step).  A region is timed with device events, with
  one synchronise at its end.  Printed: every region, the spread among the off regions (the yardstick's own noise), and the
  on-minus-off difference, which counts as real only where it exceeds that spread.

  Then ema_update_kernel alone: --kernel-reps back-to-back launches over the engine's own buffers between two events, and, for
  scale, the same number of check_finite_kernel launches over the gradient buffer (the project's other streaming pass over 85 MB:
  profiles/dynscale_kernel_stats.txt).  The average reads both operands and writes one: 12 bytes per element."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FABRIC_TBPS = 8.0          # the HBM3E figure the project quotes its bandwidth shares against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=5, help="timed regions per setting (at least 3)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--kernel-reps", type=int, default=50)
    args = ap.parse_args()
    if args.regions < 3:
        ap.error("--regions must be at least 3")

    import torch
    import bench
    from vpd_amd.data import RGB_MEAN_STD
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import step
    from vpd_amd.trainer import ModelTrainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema.py measures on the GPU: none found")
    device = "cuda"
    img, emb = bench.synthetic_batch(args.batch, device, seed=1, c_in=5, mean_std=RGB_MEAN_STD["diving48"], target_dim=bench.EMB_DIM)
    torch.manual_seed(0)
    enc = RGBF_EmbeddingModel("resnet34", bench.EMB_DIM, True, device)
    enc.reset_parameters(seed=0)
    tr = ModelTrainer(enc, motion=False)
    opt, scaler = tr.get_optimizer(5e-4)
    eng = enc.engine
    enc.train()

    def run(n):
        for _ in range(n):
            step(opt, scaler, tr._forward_loss(img, emb, train=True))

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(n)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / n      # us per iteration

    run(args.warmup)
    eng.enable_ema(0.999)
    run(args.warmup)
    torch.cuda.synchronize()
    times = {"off": [], "on": []}
    for r in range(args.regions):
        for tag in ("off", "on"):
            if tag == "off":
                eng.disable_ema()
            else:
                eng.enable_ema(0.999)
            torch.cuda.synchronize()
            times[tag].append(timed(run, args.steps))
            print("region %2d %-3s %9.2f us/step" % (r, tag, times[tag][-1]))
    med = lambda v: sorted(v)[len(v) // 2]
    off, on = times["off"], times["on"]
    spread = max(off) - min(off)
    diff = med(on) - med(off)
    print("EMA off: median %.2f us/step, min %.2f, max %.2f, spread %.2f us (%.2f %%)" % (med(off), min(off), max(off), spread, 100 * spread / med(off)))
    print("EMA on : median %.2f us/step, min %.2f, max %.2f" % (med(on), min(on), max(on)))
    print("on - off: %.2f us/step (%.2f %% of the step); per adjacent pair: %s"
          % (diff, 100 * diff / med(off), " ".join("%.2f" % (y - x) for x, y in zip(off, on))))
    print("the difference %s the off regions' own spread" % ("exceeds" if abs(diff) > spread else "is within"))

    # the kernel alone, and check_finite_kernel over the gradients beside it
    numel = eng.param_numel + eng.bn_numel
    us = timed(lambda n: [eng.ema_update() for _ in range(n)], args.kernel_reps)
    us = min(us, timed(lambda n: [eng.ema_update() for _ in range(n)], args.kernel_reps))
    bps = 12.0 * numel / (us * 1e-6)
    print("ema_update_kernel: %d elements, %.1f MB moved per launch, %.2f us per launch back to back: %.2f TB/s, %.0f %% of the %.0f TB/s figure"
          % (numel, 12.0 * numel / 1e6, us, bps / 1e12, 100 * bps / (FABRIC_TBPS * 1e12), FABRIC_TBPS))
    st = torch.zeros(8, dtype=torch.int32, device=device)
    g = eng.grads
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def finite(n):
        for _ in range(n):
            eng.check(eng.L.vpd_op_check_finite(ptr(g), eng.param_numel, ptr(st), eng.stream()), "vpd_op_check_finite")
    us_f = min(timed(finite, args.kernel_reps), timed(finite, args.kernel_reps))
    bps_f = 4.0 * eng.param_numel / (us_f * 1e-6)
    print("check_finite_kernel: %.1f MB read per launch, %.2f us per launch back to back: %.2f TB/s"
          % (4.0 * eng.param_numel / 1e6, us_f, bps_f / 1e12))
    print("loss of the last step %.4f; average updates applied %d" % (float(eng.loss_step.item()), eng.ema_state()["num_updates"]))


if __name__ == "__main__":
    main()
