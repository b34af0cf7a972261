#!/usr/bin/env python3
"""What gradient-norm clipping costs per step, in ONE process and one call:

  ResNet-34 student, 256 crops of 5 x 128 x 128, fused AdamW (bench.py's flagship workload).  For bf16 (no scaler) and for fp16
  behind a DynamicLossScaler, one trainer each; after it is warm, regions of --steps steps alternate clipping off, on, off, on ...
  (off: StudentEngine.disable_grad_clip(), the step launches what it launched before the feature; on: enable_grad_clip(1.0)).
  A region is timed with device events, with one synchronise at its end.  Printed: every region, the spread among the off regions
  (the yardstick's own noise) and the on-minus-off difference, which counts as real only where it exceeds that spread.
  bf16: on adds the norm pass, the one-block kernel and the block's step counter.  fp16 dynamic: the norm pass replaces the
  non-finite search, so on adds the one-block kernel only.

  Then the norm pass alone (grad_sqsum_kernel + clip_finalize_kernel: vpd_plan_grad_norm) against check_finite_kernel
  (vpd_plan_check_grads) over the same ranges, --kernel-reps launches back to back between two events, in alternating regions,
  and the one-block kernel alone (vpd_op_grad_norm over no ranges) to tell the two launches of the pair apart."""
import argparse
import ctypes as C
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
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--max-norm", type=float, default=1.0)
    args = ap.parse_args()
    if args.regions < 3:
        ap.error("--regions must be at least 3")

    import torch
    import bench
    from vpd_amd.data import RGB_MEAN_STD
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import DynamicLossScaler, step
    from vpd_amd.trainer import ModelTrainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip.py measures on the GPU: none found")
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
        opt, scaler = tr.get_optimizer(5e-4, loss_scale="dynamic" if dtype == "fp16" else None)
        eng = enc.engine
        enc.train()
        name = "bf16" if dtype == "bf16" else "fp16 dynamic"

        def run(n):
            for _ in range(n):
                step(opt, scaler, tr._forward_loss(img, emb, train=True))

        run(args.warmup)
        eng.enable_grad_clip(args.max_norm)
        run(args.warmup)
        torch.cuda.synchronize()
        times = {"off": [], "on": []}
        for r in range(args.regions):
            for tag in ("off", "on"):
                if tag == "off":
                    eng.disable_grad_clip()
                else:
                    eng.enable_grad_clip(args.max_norm)
                torch.cuda.synchronize()
                times[tag].append(timed(run, args.steps))
                print("%s region %2d clip %-3s %9.2f us/step" % (name, r, tag, times[tag][-1]))
        off, on = times["off"], times["on"]
        spread = max(off) - min(off)
        diff = med(on) - med(off)
        print("%s clip off: median %.2f us/step, min %.2f, max %.2f, spread %.2f us (%.2f %%)"
              % (name, med(off), min(off), max(off), spread, 100 * spread / med(off)))
        print("%s clip on : median %.2f us/step, min %.2f, max %.2f" % (name, med(on), min(on), max(on)))
        print("%s on - off: %.2f us/step (%.2f %% of the step); per adjacent pair: %s"
              % (name, diff, 100 * diff / med(off), " ".join("%.2f" % (y - x) for x, y in zip(off, on))))
        print("%s: the difference %s the off regions' own spread" % (name, "exceeds" if abs(diff) > spread else "is within"))
        stats = eng.clip_stats()
        print("%s: last norm %.6g, coefficient %.6g, steps clipped %d, non-finite %d; loss of the last step %.4f%s"
              % (name, stats["total_norm"], stats["coef"], stats["clipped_steps"], stats["nonfinite_steps"],
                 float(eng.loss_step.item()), "" if scaler is None else "; loss scale %g, skipped %d" % (scaler.get_scale(), scaler.skipped_steps)))

        if dtype == "bf16":
            # the passes alone, over the same ranges (the flat gradient buffer: the step above consumed the scratch)
            pl = eng.step_plan
            ptr = lambda t: C.c_void_p(t.data_ptr())
            st = torch.zeros(8, dtype=torch.int32, device=device)
            st.view(torch.float32)[0] = 1.0
            clip = torch.zeros(int(eng.L.vpd_clip_state_bytes()) // 4, dtype=torch.int32, device=device)
            g = eng.grads

            def finite(n):
                for _ in range(n):
                    eng.check(eng.L.vpd_plan_check_grads(pl.handle, ptr(g), eng.param_numel, ptr(st), ptr(pl.workspace),
                                                         eng.stream()), "vpd_plan_check_grads")

            def norm(n):
                for _ in range(n):
                    eng.check(eng.L.vpd_plan_grad_norm(pl.handle, ptr(g), eng.param_numel, args.max_norm, None, 1.0, ptr(clip),
                                                       ptr(pl.workspace), eng.stream()), "vpd_plan_grad_norm")

            def finalize(n):      # no ranges: nothing but the one-block kernel is launched
                for _ in range(n):
                    eng.check(eng.L.vpd_op_grad_norm(None, None, 0, args.max_norm, None, 1.0, ptr(clip), eng.stream()),
                              "vpd_op_grad_norm")
            finite(args.kernel_reps)
            norm(args.kernel_reps)
            finalize(args.kernel_reps)
            torch.cuda.synchronize()
            tf, tn, tz = [], [], []
            for r in range(args.regions):
                tf.append(timed(finite, args.kernel_reps))
                tn.append(timed(norm, args.kernel_reps))
                tz.append(timed(finalize, args.kernel_reps))
                print("kernel region %2d check_finite %8.2f us  grad norm (+ finalize) %8.2f us  finalize alone %8.2f us" % (r, tf[-1], tn[-1], tz[-1]))
            mb = 4.0 * eng.param_numel / 1e6
            sp = max(tf) - min(tf)
            print("check_finite_kernel: %.1f MB read per launch, median %.2f us back to back (%.2f TB/s), region-to-region spread %.2f us"
                  % (mb, med(tf), mb / med(tf), sp))
            print("grad_sqsum_kernel + clip_finalize_kernel: median %.2f us back to back (%.2f TB/s); minus check_finite: %.2f us = %.1f x its spread"
                  % (med(tn), mb / med(tn), med(tn) - med(tf), (med(tn) - med(tf)) / sp if sp > 0 else float("inf")))
            print("clip_finalize_kernel alone (no partial sums to add): median %.2f us back to back; the pair minus that: %.2f us (%.2f TB/s)"
                  % (med(tz), med(tn) - med(tz), mb / (med(tn) - med(tz))))
        del enc, tr, opt, scaler, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
