#!/usr/bin/env python3
"""apply_vpd_model.py --jitter J: the two input routes of the same loop, A/B on one GPU in one process, alternating.

  host    FrameDataset(augment_jitter=J): DataLoader workers decode the PNGs and build all K = (1 + J)(1 + flip) fp32 views
          (vpd_amd.data.color_jitter on the normalised image), 328 KB per VIEW cross PCIe        (apply --jitter J --host_fp32)
  device  FrameDataset(raw_u8=True): workers decode the PNGs, 82 KB of u8 per FRAME cross PCIe, every view is built on the
          device straight into the stem's staging buffer (vpd_plan_stage_views_jitter)           (apply --jitter J)

Both sides read the same seeded PNG crops (written to --crop_dir first), use the same DataLoader settings and the same
embed_dataset loop (hipGraph forward, streaming D2H of the embeddings).  Each round times one pass over all frames per
side; the order of the sides alternates from round to round.  Prints one JSON line: views/s per round and side, median
and spread (min .. max).

--kernels: no loop; the staging kernels alone on device-resident frames, timed with device events over --reps launches --
the jittered-view launches (K = 6) beside the plain [orig, flip] launch -- with their algorithmic bytes (u8 read once per
frame + K staging rows written) as achieved bytes/s.  Under `rocprofv3 --kernel-trace --stats -- python3 tools/bench_apply_jitter.py
--kernels` the same launches give the per-kernel split.

  python tools/bench_apply_jitter.py [--frames 1992] [--jitter 2] [--rounds 3] [--workers 12]
  python tools/bench_apply_jitter.py --kernels [--reps 50]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARCH, EMB_DIM, HW = "resnet34", 128, 128


def write_crops(crop_dir, n_frames, frames_per_video=166):
    from PIL import Image
    rs = np.random.RandomState(0)
    for f in range(n_frames):
        d = os.path.join(crop_dir, "video%04d" % (f // frames_per_video))
        os.makedirs(d, exist_ok=True)
        # smooth-ish content (PNG decode time depends on it): a random low-resolution image scaled up, plus noise
        low = rs.randint(0, 256, (16, 16, 3)).astype(np.uint8)
        img = np.asarray(Image.fromarray(low).resize((HW, HW), Image.BILINEAR), dtype=np.int16)
        img = np.clip(img + rs.randint(-8, 9, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(d, "%d.png" % (f % frames_per_video)))
        fl = np.clip(np.round(124 + 12 * rs.randn(HW, HW, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(fl).save(os.path.join(d, "%d.flow.png" % (f % frames_per_video)))


def kernels_only(args):
    from vpd_amd.augment import CropAugmenter, sample_view_params
    from vpd_amd.data import RGB_MEAN_STD
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    dev = torch.device("cuda", 0)
    enc = RGBF_EmbeddingModel("resnet18", 32, True, dev)
    enc.eval()
    aug = CropAugmenter(dev, RGB_MEAN_STD["diving48"], HW, True)
    g = torch.Generator().manual_seed(1)
    J, flip = args.jitter, True
    K = (1 + J) * 2
    res = {}
    for name, frames, jit in (("views_jitter", 996 // (1 + J), J), ("views_plain", 498, 0)):
        rgb = torch.randint(0, 256, (frames, HW, HW, 3), generator=g, dtype=torch.uint8).to(dev)
        flow = torch.randint(100, 150, (frames, HW, HW, 2), generator=g, dtype=torch.uint8).to(dev)
        params = sample_view_params(frames, jit, flip, generator=g) if jit else None
        pdev = torch.from_numpy(params.view(np.uint8).reshape(len(params), 64)).to(dev) if jit else None
        run = lambda: aug.stage_views(enc.engine, rgb, flow, flip, jitter=jit, params=pdev)
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / args.reps
        k = K if jit else 2
        nbytes = frames * HW * HW * (5 + k * 16)          # u8 RGB + flow read once per frame, k staging rows of 16 B per pixel
        res[name] = {"frames": frames, "views": frames * k, "us_per_call": us, "us_per_1000_frames": us * 1000 / frames,
                     "us_per_1000_views": us * 1000 / (frames * k), "algorithmic_bytes": nbytes,
                     "achieved_TBps": nbytes / us / 1e6}
    print(json.dumps({"what": "staging launches alone, device events (launch overhead included)", "jitter": J, "K": K,
                      "reps": args.reps, **res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1992)
    ap.add_argument("--jitter", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--crop_dir", default=None, help="where the seeded PNG crops are written (default: a temporary directory)")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_apply_jitter.py measures on the GPU: no device found")
    if args.kernels:
        return kernels_only(args)
    from torch.utils.data import DataLoader
    from vpd_amd.apply import apply_batch_size, embed_dataset
    from vpd_amd.augment import CropAugmenter
    from vpd_amd.data import RGB_MEAN_STD, FrameDataset, list_crop_dir

    crop_dir = args.crop_dir or tempfile.mkdtemp(prefix="vpd_jitter_crops_")
    write_crops(crop_dir, args.frames)
    videos, tasks = list_crop_dir(crop_dir)
    assert len(tasks) == args.frames
    ms = RGB_MEAN_STD["diving48"]
    dev = torch.device("cuda", 0)
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    enc = RGBF_EmbeddingModel(ARCH, EMB_DIM, True, dev)
    enc.reset_parameters(seed=0)
    enc.eval()
    aug = CropAugmenter(dev, ms, HW, True)
    J = args.jitter
    K = (1 + J) * 2
    bs = apply_batch_size(J, False)

    def loader(raw):
        ds = FrameDataset(tasks, HW, ms, augment_jitter=0 if raw else J, augment_flip=True, flow_img_name="flow", raw_u8=raw)
        return DataLoader(ds, batch_size=bs, shuffle=False, num_workers=args.workers, pin_memory=True)

    def one_pass(side):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if side == "device":
            embs = embed_dataset(enc, loader(True), len(videos), augmenter=aug, flip=True, jitter=J)
        else:
            embs = embed_dataset(enc, loader(False), len(videos))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert sum(len(v) for v in embs) == args.frames and embs[0][0][1].shape == (K, EMB_DIM)
        return args.frames * K / dt

    for side in ("device", "host"):                          # warm-up: plans, graphs (full batch + tail), pinned buffers
        one_pass(side)
    rates = {"host": [], "device": []}
    for r in range(args.rounds):
        for side in (("host", "device") if r % 2 == 0 else ("device", "host")):
            rates[side].append(one_pass(side))
    if args.crop_dir is None:
        shutil.rmtree(crop_dir, ignore_errors=True)
    summ = lambda v: {"median": float(np.median(v)), "min": min(v), "max": max(v), "rounds": v}
    print(json.dumps({"metric": "views/s through apply's loop (PNG decode in DataLoader workers included on both sides)",
                      "workload": "%d frames x K=%d views (jitter %d, flip), %s 5x%dx%d, D=%d, bf16, batches of %d frames, %d workers"
                                  % (args.frames, K, J, ARCH, HW, HW, EMB_DIM, bs, args.workers),
                      "host_fp32_route": summ(rates["host"]), "device_u8_route": summ(rates["device"]),
                      "speedup_of_medians": float(np.median(rates["device"]) / np.median(rates["host"]))}))


if __name__ == "__main__":
    main()
