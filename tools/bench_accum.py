#!/usr/bin/env python3
"""What gradient accumulation costs per micro-step, in ONE process and one call:

  ResNet-34 student, 256 crops of 5 x 128 x 128, fused AdamW (bench.py's flagship workload), --dtype bf16 or fp16 (fp16: behind a
  DynamicLossScaler).  One trainer; after it is warm, regions of --steps micro-steps alternate K = 1 and K = 2 (K = 2: every other
  micro-step is step(..., accumulate=True), the one behind it the step of always, which folds first).  A region is timed with
  device events, with one synchronise at its end.  Printed: every region, the spread among the K = 1 regions (the yardstick's own
  noise) and the K = 2 minus K = 1 difference per micro-step, which counts as real only where it exceeds that spread.  Then the
  two kinds of micro-step apart: regions of non-final micro-steps only (forward, lazy backward, store into the accumulator -- no
  optimizer step) and of final ones only (forward, lazy backward, fold, optimizer step; the accumulator is marked as held before
  each, its contents zeroed once so that nothing grows).

  Expectation, written down before the first run: the student has 21.4 M parameters = 85.7 MB of fp32 gradients.  The store pass
  of a window's first micro-step moves 2 x 85.7 MB (read live, write accumulator), an add pass and the fold 3 x 85.7 MB (read
  both, write one): at the 6.7 TB/s on record for ema_update_kernel's same two-reads-one-write traffic that is about 26 us and
  38 us.  A non-final micro-step also SAVES the optimizer step (AdamW + repack), so it should come out cheaper than a K = 1 step;
  a final one should cost a K = 1 step plus the fold.

  Then grad_accum_kernel alone, both modes, beside ema_update_kernel in the same run: --kernel-reps back-to-back launches between
  two events over buffers of the engine's own size."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBPS = 8.0             # the HBM3E peak the project quotes its bandwidth shares against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=3, help="timed regions per setting (at least 3)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--kernel-reps", type=int, default=50)
    args = ap.parse_args()
    if args.regions < 3:
        ap.error("--regions must be at least 3")
    if args.steps % 2:
        ap.error("--steps must be even (K = 2 windows)")

    import torch
    import bench
    from vpd_amd.data import RGB_MEAN_STD
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import DynamicLossScaler, step
    from vpd_amd.trainer import ModelTrainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_accum.py measures on the GPU: none found")
    device = "cuda"
    img, emb = bench.synthetic_batch(args.batch, device, seed=1, c_in=5, mean_std=RGB_MEAN_STD["diving48"], target_dim=bench.EMB_DIM)
    torch.manual_seed(0)
    enc = RGBF_EmbeddingModel("resnet34", bench.EMB_DIM, True, device, dtype=args.dtype)
    enc.reset_parameters(seed=0)
    tr = ModelTrainer(enc, motion=False)
    opt, scaler = tr.get_optimizer(5e-4, loss_scale="dynamic" if args.dtype == "fp16" else None)
    assert (args.dtype == "fp16") == isinstance(scaler, DynamicLossScaler)
    eng = enc.engine
    enc.train()

    def run(n, k=1):
        for i in range(n):
            step(opt, scaler, tr._forward_loss(img, emb, train=True), accumulate=(i + 1) % k != 0)

    def run_nonfinal(n):
        for _ in range(n):
            eng.drop_accumulated_grads()      # every one is a window's first: the store pass
            step(opt, scaler, tr._forward_loss(img, emb, train=True), accumulate=True)

    def run_add(n):
        for _ in range(n):
            step(opt, scaler, tr._forward_loss(img, emb, train=True), accumulate=True)      # onto what is held: the add pass

    def hold():
        """mark the accumulator as holding one micro-batch in the lazy layout (what the warm-up's K = 2 windows left it in:
        every backward of this tool is lazy) without a backward of its own"""
        eng.hold_accumulated_grads("scratch")      # (raises unless a K = 2 window ran first)

    def run_final(n):
        for _ in range(n):
            hold()                            # a window's last: fold, then the step (the accumulator holds zeros)
            step(opt, scaler, tr._forward_loss(img, emb, train=True))

    def timed(fn, n, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(n, *a)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n      # us per iteration

    run(args.warmup)
    run(args.warmup, 2)
    torch.cuda.synchronize()
    med = lambda v: sorted(v)[len(v) // 2]
    times = {1: [], 2: []}
    for r in range(args.regions):
        for k in (1, 2):
            torch.cuda.synchronize()
            times[k].append(timed(run, args.steps, k))
            print("region %2d K=%d %9.2f us/micro-step" % (r, k, times[k][-1]))
    k1, k2 = times[1], times[2]
    spread = max(k1) - min(k1)
    diff = med(k2) - med(k1)
    print("%s K=1: median %.2f us/step, min %.2f, max %.2f, spread %.2f us (%.2f %%)" % (args.dtype, med(k1), min(k1), max(k1), spread, 100 * spread / med(k1)))
    print("%s K=2: median %.2f us/micro-step, min %.2f, max %.2f" % (args.dtype, med(k2), min(k2), max(k2)))
    print("K=2 - K=1: %.2f us/micro-step (%.2f %%); per adjacent pair: %s"
          % (diff, 100 * diff / med(k1), " ".join("%.2f" % (y - x) for x, y in zip(k1, k2))))
    print("the difference %s the K=1 regions' own spread" % ("exceeds" if abs(diff) > spread else "is within"))

    # the kinds of micro-step apart, against the K = 1 step
    eng.drop_accumulated_grads()
    run_nonfinal(2)
    eng.accumulator.zero_()
    kinds = {"non-final (store)": [], "non-final (add)": [], "final (fold + step)": []}
    for r in range(args.regions):
        eng.drop_accumulated_grads()
        kinds["non-final (store)"].append(timed(run_nonfinal, args.steps // 2))
        eng.accumulator.zero_()
        hold()
        kinds["non-final (add)"].append(timed(run_add, args.steps // 2))
        eng.accumulator.zero_()
        kinds["final (fold + step)"].append(timed(run_final, args.steps // 2))
        eng.drop_accumulated_grads()
    for name, v in kinds.items():
        print("%-20s median %.2f us, min %.2f, max %.2f; minus the K=1 step: %+.2f us" % (name, med(v), min(v), max(v), med(v) - med(k1)))

    # the kernel alone, both modes, beside ema_update_kernel over buffers of the same size
    numel = eng.param_numel
    a = torch.randn(numel, device=device)
    b = torch.randn(numel, device=device) * 1e-3
    ptr = lambda t: (C.c_void_p * 1)(t.data_ptr())
    n1 = (C.c_longlong * 1)(numel)

    def accum(n, add):
        for _ in range(n):
            eng.check(eng.L.vpd_op_grad_accumulate(ptr(a), ptr(b), n1, 1, add, eng.stream()), "vpd_op_grad_accumulate")

    def ema(n):
        for _ in range(n):
            eng.check(eng.L.vpd_ema_update(ptr(b), ptr(a), n1, 1, 0.999, 0, 0, 0, None, eng.stream()), "vpd_ema_update")
    for name, fn, fa, nbytes in (("grad_accum_kernel<store>", accum, (0,), 8.0), ("grad_accum_kernel<add>", accum, (1,), 12.0),
                                 ("ema_update_kernel", ema, (), 12.0)):
        us = min(timed(fn, args.kernel_reps, *fa) for _ in range(3))
        bps = nbytes * numel / (us * 1e-6)
        print("%-26s %d elements, %.1f MB moved per launch, %.2f us per launch back to back: %.2f TB/s, %.0f %% of the %.0f TB/s figure"
              % (name + ":", numel, nbytes * numel / 1e6, us, bps / 1e12, 100 * bps / (HBM_TBPS * 1e12), HBM_TBPS))
    pl = eng.step_plan
    nscratch = pl.accum_numel - pl.param_numel
    print("accumulator: %d floats (%.1f MB): scratch image %d + flat image %d" % (pl.accum_numel, 4.0 * pl.accum_numel / 1e6, nscratch, pl.param_numel))
    print("loss of the last step %.4f; optimizer steps applied %d" % (float(eng.loss_step.item()), eng.adam_step))


if __name__ == "__main__":
    main()
