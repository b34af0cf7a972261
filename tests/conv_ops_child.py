"""Child process of tests/test_conv_ops_gpu.py (and, with "dispatch", of tests/test_opref_cpu.py): the convolution launcher reads its
switches (VPD_PWS, VPD_PWS_GEO, VPD_PWS_BLOCKS, VPD_NO_WS, VPD_RESERVE_CUS) once per process, so each setting of a case gets a fresh interpreter.
usage: conv_ops_child.py <run id[,run id...]> <dispatch|full|light>
  dispatch  no launch: what vpd_op_conv2d_dispatch says for every operation of the run (works without a GPU: 256 CUs assumed)
  full      both libraries, both input regimes, every operation against the float64 reference
  light     (a switch variant of a run checked in full) integer regime against the reference, random regime as digests only
Prints one line "RESULT <json>": {"fail": [...], "dispatch": {...}, "record": {...}, "digest": {...}}; the parent asserts on it."""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import opref as R  # noqa: E402

SENT = -12352.0              # bf16 and fp16 hold it; no integer-regime value (|v| <= 2^8) and no randn value comes near
SLACK = 4096                 # elements behind every output buffer
REL_TOL = 4e-3               # the whole-tensor gate of tests/test_ops_gpu.py, kept beside the per-element bound

# run id -> (case of opref.CONV_CASES, environment, expected dispatch of the forward launch, of the data-gradient launch or None
# for "the same").  tiles: pixel tiles of the busiest block; nsa: stages of the kernel's LDS ring, which `tiles` must exceed (a stage
# is overwritten from a block's (nsa + 1)-th tile on); c64x2_tiles: tiles per block of the eval epilogue's c64x2 launch, 1 when not
# given.  Expectations hold for a 256-CU device.
FEW = {"VPD_RESERVE_CUS": "248"}       # a budget of 8 CUs: 8 pixel lanes, so a small tensor gives every block a long walk
WALK = {"VPD_RESERVE_CUS": "240"}      # 16 CUs: the resident-weight kernels reuse each halo buffer 16 times (8 CUs: c0_w32's sums leave 2^24)
RUNS = {
    "c0_w32-device":        ("c0_w32", {}, dict(kclass=0, bm=128, bn=64, tiles=2), None),
    "c0_w16-device":        ("c0_w16", {}, dict(kclass=0, bm=128, bn=64, tiles=2), None),
    "c0_w32_walk-walk":     ("c0_w32_walk", WALK, dict(kclass=0, bm=128, bn=64, tiles=32, c64x2_tiles=16), None),
    "c1_w16-ws":            ("c1_w16", {"VPD_PWS": "0"}, dict(kclass=1, pws=0, bm=256, bn=128, tiles=1), None),
    "c1_w16-few_blocks":    ("c1_w16", {"VPD_PWS_BLOCKS": "24"}, dict(kclass=1, pws=1, geo=0, bm=256, bn=128, tiles=9), None),
    "c1_w16_device-device": ("c1_w16_device", {}, dict(kclass=1, pws=1, geo=0, bm=256, bn=128, tiles=2), None),
    "c6_w16-device":        ("c6_w16", {}, dict(kclass=6, pws=1, geo=16, bm=256, bn=64, tiles=2), None),
    "c6_w16-few_blocks":    ("c6_w16", {"VPD_PWS_BLOCKS": "48"}, dict(kclass=6, pws=1, geo=16, bm=256, bn=64, tiles=7), None),
    "c6_w16-geo_off":       ("c6_w16", {"VPD_PWS_GEO": "0"}, dict(kclass=6, pws=1, geo=0, bm=256, bn=64, tiles=2), None),
    "c6_w16-ws":            ("c6_w16", {"VPD_PWS": "0"}, dict(kclass=6, pws=0, bm=256, bn=64, tiles=1), None),
    "c6_w8_ragged-few_blocks": ("c6_w8_ragged", {"VPD_PWS_BLOCKS": "24"}, dict(kclass=6, pws=1, geo=8, bm=256, bn=64, tiles=9), None),
    "c6_w8_ragged-geo_off": ("c6_w8_ragged", {"VPD_PWS_BLOCKS": "24", "VPD_PWS_GEO": "0"}, dict(kclass=6, pws=1, geo=0, bm=256, bn=64, tiles=9), None),
    "c6_w8_ragged-ws":      ("c6_w8_ragged", {"VPD_PWS": "0"}, dict(kclass=6, pws=0, bm=256, bn=64, tiles=1), None),
    "c6_w8_device-device":  ("c6_w8_device", {}, dict(kclass=6, pws=1, geo=8, bm=256, bn=64, tiles=2), None),
    "c2_w4_ragged-few_blocks": ("c2_w4_ragged", {"VPD_PWS_BLOCKS": "24"}, dict(kclass=2, pws=1, geo=0, bm=128, bn=128, tiles=9), None),
    "c2_w4_ragged-device":  ("c2_w4_ragged", {}, dict(kclass=2, pws=1, geo=0, bm=128, bn=128, tiles=2), None),
    "c2_w4_ragged-ws":      ("c2_w4_ragged", {"VPD_PWS": "0"}, dict(kclass=2, pws=0, bm=128, bn=128, tiles=1), None),
    "c3_w4-few_blocks":     ("c3_w4", {"VPD_PWS_BLOCKS": "24"}, dict(kclass=3, pws=1, geo=4, bm=128, bn=64, tiles=2), None),
    "c3_w4-geo_off":        ("c3_w4", {"VPD_PWS_BLOCKS": "24", "VPD_PWS_GEO": "0"}, dict(kclass=3, pws=1, geo=0, bm=128, bn=64, tiles=2), None),
    "c3_w4-ws":             ("c3_w4", {"VPD_PWS": "0"}, dict(kclass=3, pws=0, bm=128, bn=64, tiles=1), None),
    "c3_w4_device-device":  ("c3_w4_device", {}, dict(kclass=3, pws=1, geo=4, bm=128, bn=64, tiles=2), None),
    "c3_two_chunks-few_blocks": ("c3_two_chunks", {"VPD_PWS_BLOCKS": "2"}, dict(kclass=3, pws=1, geo=4, bm=128, bn=64, tiles=3), None),
    # gather family.  The stride-2 3x3 forward of 64-multiple channel counts is the ring GEMM's (conv1x1_ws_eligible, istr == 2);
    # its data gradient runs as four parity-class launches of conv_igemm_kernel with the tile vpd_conv_bm picks
    "s2_w32-device":        ("s2_w32", {}, dict(kclass=4, ws1x1=1, bm=128, bn=128), dict(kclass=4, ws1x1=0, halo=0, stream1x1=0, bm=128, bn=64)),
    "s2_w8-device":         ("s2_w8", {}, dict(kclass=4, ws1x1=1, bm=128, bn=64), dict(kclass=4, ws1x1=0, halo=0, stream1x1=0, bm=64, bn=64)),
    "s2_w16_big-device":    ("s2_w16_big", {}, dict(kclass=4, ws1x1=1, bm=256, bn=128), dict(kclass=4, ws1x1=0, halo=0, stream1x1=0, bm=128, bn=128)),
    # with the ring GEMM switched off the stride-2 3x3 forward is the gather kernel's too (no other run reaches its forward
    # epilogue): one ragged tile of 64 x 64
    "s2_w8-ring_off":       ("s2_w8", {"VPD_CONV_S2_WS": "0"}, dict(kclass=4, ws1x1=0, halo=0, stream1x1=0, bm=64, bn=64),
                             dict(kclass=4, ws1x1=0, halo=0, stream1x1=0, bm=64, bn=64)),
    "c3_w4-no_ws":          ("c3_w4", {"VPD_NO_WS": "1"},dict(kclass=4, halo=1, bm=64, bn=128), None),
    "c0_w16-no_ws":         ("c0_w16", {"VPD_NO_WS": "1"}, dict(kclass=4, halo=1, bm=128, bn=64), None),
    "c1_w16-no_ws":         ("c1_w16", {"VPD_NO_WS": "1"}, dict(kclass=4, halo=1, bm=128, bn=128), None),
    # (its data gradient, 128 -> 512 channels on 51,200 pixels, is conv1x1_stream_kernel's: tests/test_ops_gpu.py has that kernel's cases)
    "stem_w128-device":     ("stem_w128", {}, dict(kclass=5, bm=128, bn=64, tiles=2), None),
    "stem_w32-device":      ("stem_w32", {}, dict(kclass=5, bm=128, bn=64, tiles=1), None),
    "stem_w128_walk-walk":  ("stem_w128_walk", WALK, dict(kclass=5, bm=128, bn=64, tiles=32), None),
    "ring_1x1-device":      ("ring_1x1", {}, dict(kclass=4, ws1x1=1, bm=256, bn=128), dict(kclass=4, ws1x1=0, stream1x1=1)),
    # conv1x1_stream_kernel<KC, BM, BN, NSA>: every instantiation of the launcher's table on a ring that wraps (8 CUs), forward and
    # data gradient with their accumulate / eval epilogues; the last run on the whole device
    "st_64_64-few":         ("st_64_64", FEW, dict(kclass=4, stream1x1=1, bm=128, bn=64, tiles=9, nsa=6), None),
    "st_64_128-few":        ("st_64_128", FEW, dict(kclass=4, stream1x1=1, bm=128, bn=128, tiles=9, nsa=6),
                             dict(kclass=4, stream1x1=1, bm=128, bn=64, tiles=9, nsa=4)),
    "st_64_256-few":        ("st_64_256", FEW, dict(kclass=4, stream1x1=1, bm=64, bn=256, tiles=12, nsa=8),
                             dict(kclass=4, stream1x1=1, bm=64, bn=64, tiles=12, nsa=4)),
    "st_64_256_w16-few":    ("st_64_256_w16", FEW, dict(kclass=4, stream1x1=1, bm=64, bn=256, tiles=12, nsa=8),
                             dict(kclass=4, stream1x1=1, bm=64, bn=64, tiles=12, nsa=4)),
    "st_128_128-few":       ("st_128_128", FEW, dict(kclass=4, stream1x1=1, bm=128, bn=128, tiles=9, nsa=4), None),
    "st_128_256-few":       ("st_128_256", FEW, dict(kclass=4, stream1x1=1, bm=64, bn=256, tiles=12, nsa=6),
                             dict(kclass=4, stream1x1=1, bm=32, bn=128, tiles=24, nsa=6)),
    "st_256_512_s2-few":    ("st_256_512_s2", FEW, dict(kclass=4, stream1x1=1, bm=32, bn=128, tiles=24, nsa=6), None),
    "st_64_256_w32-device": ("st_64_256_w32", {}, dict(kclass=4, stream1x1=1, bm=64, bn=256, tiles=3),
                             dict(kclass=4, stream1x1=1, bm=64, bn=64, tiles=3)),
}
# switch variants whose outputs must be bit-identical to another run's (same products, same order of additions)
SAME_BITS = {"c6_w16-geo_off": "c6_w16-device", "c6_w16-ws": "c6_w16-device", "c6_w8_ragged-geo_off": "c6_w8_ragged-few_blocks",
             "c6_w8_ragged-ws": "c6_w8_ragged-few_blocks", "c2_w4_ragged-ws": "c2_w4_ragged-few_blocks",
             "c2_w4_ragged-device": "c2_w4_ragged-few_blocks", "c3_w4-geo_off": "c3_w4-few_blocks", "c3_w4-ws": "c3_w4-few_blocks",
             "c1_w16-few_blocks": "c1_w16-ws", "c6_w16-few_blocks": "c6_w16-device"}
OUT12 = ("kclass", "pws", "geo", "c64x2", "ws1x1", "stream1x1", "halo", "bm", "bn", "mode", "tiles", "takes_sums")


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


from tests.test_ops_gpu import tapset  # noqa: E402


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


class Geo:
    """argument lists of one case: forward (x -> y) and data gradient (dz -> dx; stride 2: four parity classes)"""

    def __init__(self, cs):
        self.cs = cs
        self.k, self.st, self.pad, self.ho, self.wo = R.conv_geom(cs)
        self.n, self.ci, self.co, self.h, self.w = cs["n"], cs["ci"], cs["co"], cs["h"], cs["w"]
        k, pad = self.k, self.pad
        self.fwd_taps = tapset(k, k, 1 - pad, 1, 1 - pad, 1, 0, k, 1)
        self.dg_taps = tapset(k, k, pad + 1, -1, pad + 1, -1, 0, k, 1)

    def fwd_args(self, ypad):
        """(n, xHp, xWp, xC, yHp, yWp, yC, ypad, Hs, Ws, osub, oph, opw, istr, Kc, Co, taps)"""
        if self.cs.get("stem"):
            # 5 channels stored as 8 behind a border of 3 (right: 5); a kernel row is ONE 64-deep tap: 8 column taps x 8 channels
            return (self.n, self.h + 6, self.w + 8, 8, self.ho, self.wo, self.co, 0, self.ho, self.wo, 1, 0, 0, 2, 64, self.co,
                    tapset(7, 1, 0, 1, 0, 0, 0, 1, 0))
        return (self.n, self.h + 2, self.w + 2, self.ci, self.ho + 2 * ypad, self.wo + 2 * ypad, self.co, ypad, self.ho, self.wo,
                1, 0, 0, self.st, self.ci, self.co, self.fwd_taps)

    def wgrad_args(self):
        """(n, dzHp, dzWp, dzC, dzpad, xHp, xWp, xC, Hs, Ws, istr, Kc, Co), taps: of vpd_op_wgrad and vpd_op_wgrad_dispatch"""
        if self.cs.get("stem"):      # dz dense; the input as the forward reads it
            return (self.n, self.ho, self.wo, self.co, 0, self.h + 6, self.w + 8, 8, self.ho, self.wo, 2, 64, self.co), tapset(7, 1, 0, 1, 0, 0, 0, 1, 0)
        return (self.n, self.ho + 2, self.wo + 2, self.co, 1, self.h + 2, self.w + 2, self.ci, self.ho, self.wo, self.st, self.ci,
                self.co), self.fwd_taps

    def dgrad_launches(self):
        """stride 1: one launch; stride 2: the parity classes (ph, pw) of the input pixels (tests/test_ops_gpu.py)"""
        n, h, w, k, pad = self.n, self.h, self.w, self.k, self.pad
        if self.st == 1:
            return [(n, self.ho + 2, self.wo + 2, self.co, h, w, self.ci, 0, h, w, 1, 0, 0, 1, self.co, self.ci, self.dg_taps)]
        out = []
        for ph in range(2):
            for pw in range(2):
                hs, ws = (h - ph + 1) // 2, (w - pw + 1) // 2
                rf, tf = (ph + pad) % 2, (pw + pad) % 2
                nr = (k - rf + 1) // 2 if rf < k else 0
                nc = (k - tf + 1) // 2 if tf < k else 0
                if nr == 0 or nc == 0:
                    continue
                taps = tapset(nr, nc, (ph + pad - rf) // 2 + 1, -1, (pw + pad - tf) // 2 + 1, -1, rf * k + tf, 2 * k, 2)
                out.append((n, self.ho + 2, self.wo + 2, self.co, h, w, self.ci, 0, hs, ws, 2, ph, pw, 1, self.co, self.ci, taps))
        return out


class Ops:
    def __init__(self, name):
        from vpd_amd import _lib
        from tests import test_ops_gpu as T
        self.name, self.L, self._lib, self.T = name, _lib.lib(name), _lib, T
        assert self.L.vpd_elem_dtype().decode() == name
        self.dt = R.ELEM[name][0]

    def check(self, rc):
        self._lib.check(rc, "op", self.name)

    def dispatch(self, args, accumulate=0, flags=0):
        out = (C.c_int * 12)()
        self.check(self.L.vpd_op_conv2d_dispatch(*args, accumulate, flags, out))
        return dict(zip(OUT12, list(out)))

    # ---- buffers ----
    def padded(self, t):
        return self.T.to_padded_nhwc(t.float(), 1, 1, 1, 1, dtype=self.dt)

    def out_buffer(self, n, hh, ww, c, ypad, old=None):
        """flat [n][hh + 2 ypad][ww + 2 ypad][c] + SLACK, sentinel everywhere; old (NCHW): the interior's starting value"""
        hp, wp = hh + 2 * ypad, ww + 2 * ypad
        y = torch.full((n * hp * wp * c + SLACK,), SENT, dtype=self.dt)
        if old is not None:
            v = y[:n * hp * wp * c].view(n, hp, wp, c)
            v[:, ypad:ypad + hh, ypad:ypad + ww] = R.nhwc(old).to(self.dt)
        return y.cuda()

    def read(self, y, n, hh, ww, c, ypad):
        """-> (interior as float64 NCHW, 'outside the interior is still the sentinel')"""
        hp, wp = hh + 2 * ypad, ww + 2 * ypad
        yc = y.cpu()
        v = yc[:n * hp * wp * c].view(n, hp, wp, c)
        inner = v[:, ypad:ypad + hh, ypad:ypad + ww]
        sent = torch.tensor(SENT, dtype=self.dt)
        kept = bool((yc[n * hp * wp * c:] == sent).all())
        if ypad:
            mask = torch.ones(n, hp, wp, dtype=torch.bool)
            mask[:, ypad:ypad + hh, ypad:ypad + ww] = False
            kept = kept and bool((v[mask] == sent).all())
        return R.nchw(inner.double()), kept


def run_ops(ops, G, o, want):
    """every operation of the case on the operands o -> {op: (got float64 NCHW, border kept, device tensor)} + statistics"""
    L, T, cs = ops.L, ops.T, G.cs
    n, ci, co, h, w, ho, wo = G.n, G.ci, G.co, G.h, G.w, G.ho, G.wo
    res = {}
    if cs.get("stem"):                                  # the layout of tests/test_ops_gpu.py::test_stem_conv_and_wgrad
        x8 = torch.zeros(n, 8, h, w)
        x8[:, :ci] = o["x"].float()
        xp = T.to_padded_nhwc(x8, 3, 3, 3, 5, slack=256, dtype=ops.dt)
        w8 = torch.zeros(7, co, 8, 8)
        w8[:, :, :7, :ci] = o["w"].float().permute(2, 0, 3, 1)       # [r][co][t][c]
        wf = w8.reshape(7, co, 64).to(ops.dt).cuda()
        dzp = wd = None
    else:
        xp, dzp = ops.padded(o["x"]), ops.padded(o["dz"])
        wf = T.pack_fwd(o["w"].float(), dtype=ops.dt)
        wd = T.pack_dgrad(o["w"].float(), dtype=ops.dt)
    f32 = lambda t: t.float().cuda()

    def finish(key, y, shape, ypad, extra=None):
        torch.cuda.synchronize()
        got, kept = ops.read(y, *shape, ypad)
        res[key] = {"got": got, "kept": kept, "sha": sha(y)}
        if extra:
            res[key].update(extra)

    # forward + statistics, dense
    if "fwd" in want:
        y = ops.out_buffer(n, ho, wo, co, 0)
        stats = torch.zeros(16, 2, co, dtype=torch.float64, device="cuda")
        a = G.fwd_args(0)
        ops.check(L.vpd_op_conv2d(ptr(xp), ptr(wf), ptr(y), ptr(stats), *a, 0, stream()))
        finish("fwd", y, (n, ho, wo, co), 0, {"rows": stats.sum(dim=0).cpu()})
    if "fwd_plain" in want:                              # the same without statistics (epilogue mode 0), dense
        y = ops.out_buffer(n, ho, wo, co, 0)
        ops.check(L.vpd_op_conv2d(ptr(xp), ptr(wf), ptr(y), None, *G.fwd_args(0), 0, stream()))
        finish("fwd_plain", y, (n, ho, wo, co), 0)
    # forward, plain store into a padded output
    if "fwd_padded" in want:
        y = ops.out_buffer(n, ho, wo, co, 1)
        ops.check(L.vpd_op_conv2d(ptr(xp), ptr(wf), ptr(y), None, *G.fwd_args(1), 0, stream()))
        finish("fwd_padded", y, (n, ho, wo, co), 1)
    # eval epilogue into a padded activation
    for key, with_res, relu in (("ep", 0, 0), ("ep_relu", 0, 1), ("ep_res", 1, 0), ("ep_res_relu", 1, 1)):
        if key not in want:
            continue
        y = ops.out_buffer(n, ho, wo, co, 1)
        a = G.fwd_args(1)
        resp = ops.padded(o["res"]) if with_res else None
        sc, sh = f32(o["scale"]), f32(o["shift"])
        ops.check(L.vpd_op_conv2d_ep(ptr(xp), ptr(wf), ptr(y), *a[:10], a[13], a[14], a[15], a[16], ptr(sc), ptr(sh), ptr(resp), relu, 0,
                                     None, stream()))
        finish(key, y, (n, ho, wo, co), 1)
    if cs.get("stem"):
        if "wgrad" in want:                              # the atomics kernel, then conv_wgrad_stem_kernel + slab; dz dense
            dzd = R.nhwc(o["dz"]).contiguous().to(ops.dt).cuda()
            slab = torch.empty(L.vpd_op_wgrad_slab_bytes() // 4, dtype=torch.float32, device="cuda")
            wa, wt = G.wgrad_args()
            for key, use_slab in (("wgrad_atomics", False), ("wgrad_slab", True)):
                dw = torch.zeros(7, co, 64, dtype=torch.float32, device="cuda")
                ops.check(L.vpd_op_wgrad(ptr(dzd), ptr(xp), ptr(dw), *wa, wt, ptr(slab) if use_slab else None, stream()))
                torch.cuda.synchronize()
                res[key] = {"got": R.stem_wgrad_view(dw.cpu().double(), ci), "kept": True, "sha": sha(dw)}
        return res
    # data gradient: store, accumulate, masked accumulate
    launches = G.dgrad_launches()
    for key, acc, masked in (("dgrad", 0, 0), ("acc", 1, 0), ("macc", 1, 1)):
        if key not in want:
            continue
        y = ops.out_buffer(n, h, w, ci, 0, o["old_dx"] if acc else None)
        bits = R.mask_bits(R.nhwc(o["keep_dx"]).reshape(-1, ci)).cuda() if masked else None
        for a in launches:
            if masked:
                ops.check(L.vpd_op_conv2d_ep(ptr(dzp), ptr(wd), ptr(y), *a[:10], a[13], a[14], a[15], a[16], None, None, None, 0, 1,
                                             ptr(bits), stream()))
            else:
                ops.check(L.vpd_op_conv2d(ptr(dzp), ptr(wd), ptr(y), None, *a, acc, stream()))
        finish(key, y, (n, h, w, ci), 0)
    # data gradient + the sums of the consuming BatchNorm(s): modes 6, 7, 8
    for key, acc, two in (("sums", 0, 0), ("sums_acc", 1, 0), ("sums2", 1, 1)):
        if key not in want:
            continue
        a = launches[0]
        y = ops.out_buffer(n, h, w, ci, 0, o["old_dx"] if acc else None)
        flat = lambda t: R.nhwc(t).reshape(-1, ci).to(ops.dt).cuda().contiguous()
        zd, z2d = flat(o["z"]), flat(o["z2"])
        bits = R.mask_bits(R.nhwc(o["keep_dx"]).reshape(-1, ci)).cuda()
        rows, rows2 = (torch.zeros(4, 2, ci, dtype=torch.float64, device="cuda") for _ in range(2))
        if two:
            ops.check(L.vpd_op_conv2d_bnsums2(ptr(dzp), ptr(wd), ptr(y), ptr(zd), ptr(bits), ptr(rows), ptr(z2d), ptr(rows2),
                                              a[0], a[1], a[2], a[3], a[8], a[9], a[14], a[15], a[16], stream()))
        else:
            ops.check(L.vpd_op_conv2d_bnsums(ptr(dzp), ptr(wd), ptr(y), ptr(zd), ptr(bits), ptr(rows), a[0], a[1], a[2], a[3], a[8], a[9],
                                             a[14], a[15], a[16], acc, stream()))
        finish(key, y, (n, h, w, ci), 0, {"rows": rows.sum(dim=0).cpu(), "rows2": rows2.sum(dim=0).cpu() if two else None})
    # weight gradients (fp32): the atomics kernel, the halo + slab kernel (check_wgrad_dispatch asserts both routes), the grouped
    # persistent kernel
    if "wgrad" in want:
        k, st = G.k, G.st
        slab = torch.empty(L.vpd_op_wgrad_slab_bytes() // 4, dtype=torch.float32, device="cuda")
        for key, use_slab in (("wgrad_atomics", False), ("wgrad_slab", True)):
            dw = torch.zeros(k * k, co, ci, dtype=torch.float32, device="cuda")
            wa, wt = G.wgrad_args()
            ops.check(L.vpd_op_wgrad(ptr(dzp), ptr(xp), ptr(dw), *wa, wt, ptr(slab) if use_slab else None, stream()))
            torch.cuda.synchronize()
            res[key] = {"got": dw.cpu().double().view(k, k, co, ci).permute(2, 3, 0, 1), "kept": True, "sha": sha(dw)}
        if cs["wgrad"] == "no_group":                   # (64 -> 64 channels: no 128 x 64 tile)
            return res
        dw = torch.full((k * k, co, ci), float("nan"), dtype=torch.float32, device="cuda")
        gslab = torch.empty(max(int(L.vpd_op_wgrad128_slab_floats(co, ci)), 4), dtype=torch.float32, device="cuda")
        table = torch.empty(int(L.vpd_op_wgrad128_table_bytes()), dtype=torch.uint8, device="cuda")
        one = lambda t: (C.c_void_p * 1)(t.data_ptr())
        ops.check(L.vpd_op_wgrad128_group(1, one(dzp), one(xp), one(dw), one(gslab), (C.c_int * 7)(n, ho, wo, co, ci, st, k), ptr(table),
                                          stream()))
        torch.cuda.synchronize()
        res["wgrad_group"] = {"got": dw.cpu().double().view(k, k, co, ci).permute(2, 3, 0, 1), "kept": True, "sha": sha(dw)}
    return res


def references(cs, o, want, name, regime):
    """{op: (float64 reference, per-element bound or None)}; integer regime: bound None = equality"""
    k = cs["k"]
    Kf, Kd = k * k * cs["ci"], k * k * cs["co"]
    rnd = regime == "rand"
    ref = {}
    conv = mag = dx = dmag = None
    if any(t in want for t in ("fwd", "fwd_plain", "fwd_padded", "ep", "ep_relu", "ep_res", "ep_res_relu")):
        conv = R.conv_fwd(o["x"], o["w"], cs)
        mag = R.conv_gamma(R.conv_fwd(o["x"].abs(), o["w"].abs(), cs), Kf) if rnd else None
    if any(t in want for t in ("dgrad", "acc", "macc", "sums", "sums_acc", "sums2")):
        dx = R.conv_dgrad(o["dz"], o["w"], cs)
        dmag = R.conv_gamma(R.conv_dgrad(o["dz"].abs(), o["w"].abs(), cs), Kd) if rnd else None
    B = lambda r, g, extra=0.0: R.conv_bound(r, g, name, extra) if rnd else None
    v = lambda t: t.double().view(1, -1, 1, 1)
    for key in ("fwd", "fwd_plain", "fwd_padded"):
        if key in want:
            ref[key] = (conv, B(conv, mag))
    for key, with_res, relu in (("ep", 0, 0), ("ep_relu", 0, 1), ("ep_res", 1, 0), ("ep_res_relu", 1, 1)):
        if key in want:
            pre = R.conv_eval_ep(conv, o, with_res, False)
            # fp32 epilogue: the multiplication, two additions (four roundings allowed) on the magnitudes that enter
            extra = 4 * 2.0 ** -24 * ((conv * v(o["scale"])).abs() + v(o["shift"]).abs() + (o["res"].abs() if with_res else 0.0)) if rnd else 0.0
            b = B(pre, mag * v(o["scale"]).abs(), extra) if rnd else None
            ref[key] = (pre.clamp_min(0) if relu else pre, b)          # (|relu(a) - relu(b)| <= |a - b|)
    for key, old in (("dgrad", None), ("acc", o["old_dx"]), ("macc", o["old_dx"] * o["keep_dx"]), ("sums", None), ("sums_acc", o["old_dx"]),
                     ("sums2", o["old_dx"])):
        if key in want:
            r = dx if old is None else dx + old
            extra = 2 * 2.0 ** -24 * (dx.abs() + old.abs()) if (rnd and old is not None) else 0.0      # one more fp32 addition
            ref[key] = (r, B(r, dmag, extra))
    if "wgrad" in want:
        wg = R.conv_wgrad(o["x"], o["dz"], cs)
        M = cs["n"] * R.conv_geom(cs)[3] * R.conv_geom(cs)[4]
        # fp32 out: no final element rounding; split sums are added in fp32 (slab / atomics: a handful more roundings)
        b = R.conv_gamma(R.conv_wgrad(o["x"].abs(), o["dz"].abs(), cs), M + 64) if rnd else None
        for key in ("wgrad_atomics", "wgrad_slab") + (() if cs["wgrad"] in ("no_group", "stem") else ("wgrad_group",)):
            ref[key] = (wg, b)
    return ref


def wanted(G, disp):
    """the operations of a case: what its kernels implement"""
    cs = G.cs
    if cs.get("stem"):                                   # (the stem's data gradient is never taken)
        return ["fwd", "fwd_plain"] + (["wgrad"] if cs.get("wgrad") else [])
    want = ["fwd", "dgrad"]
    if G.k == 1 and G.st == 2:
        return ["fwd"]                                   # (its data gradient writes one pixel in four: no dense store to pin here)
    if G.st == 1:
        want += ["acc", "macc", "fwd_padded", "ep", "ep_relu", "ep_res", "ep_res_relu"]
    if cs.get("wgrad"):
        want.append("wgrad")
    if G.st == 1 and G.k == 3:
        a = G.dgrad_launches()[0]
        for key, acc, fl in (("sums", 0, 8), ("sums_acc", 1, 8), ("sums2", 1, 24)):
            if disp(a, acc, fl)["takes_sums"]:
                want.append(key)
    return want


def dispatch_table(ops, G):
    if G.cs.get("stem"):
        return {"fwd": ops.dispatch(G.fwd_args(0), 0, 1), "fwd_plain": ops.dispatch(G.fwd_args(0), 0, 0)}
    d = {"fwd": ops.dispatch(G.fwd_args(0), 0, 1), "fwd_padded": ops.dispatch(G.fwd_args(1), 0, 0), "ep": ops.dispatch(G.fwd_args(1), 0, 2)}
    if not (G.k == 1 and G.st == 2):
        launches = G.dgrad_launches()
        a = launches[0]
        d["dgrad"] = ops.dispatch(a, 0, 0)
        for i, b in enumerate(launches[1:]):             # the other parity classes of a stride-2 data gradient
            d["dgrad_p%d" % (i + 1)] = ops.dispatch(b, 0, 0)
        if G.st == 1:
            d["acc"], d["macc"] = ops.dispatch(a, 1, 0), ops.dispatch(a, 1, 4)
            if G.k == 3:
                d["sums"], d["sums_acc"], d["sums2"] = ops.dispatch(a, 0, 8), ops.dispatch(a, 1, 8), ops.dispatch(a, 1, 24)
    return d


def check_dispatch(run, table, fail):
    _, _, exp_f, exp_d = RUNS[run]
    exp_d = exp_d or exp_f
    for op, d in table.items():
        exp = exp_f if op in ("fwd", "fwd_plain", "fwd_padded", "ep") else exp_d
        if d["c64x2"]:
            # the inference twin: 256-pixel tiles, one per block at 256 x 256 pixels
            exp = dict(kclass=0, bm=256, bn=64, tiles=exp_f.get("c64x2_tiles", 1))
        for key, val in exp.items():
            if key == "c64x2_tiles":
                continue
            if key == "nsa":
                if d["tiles"] <= val:
                    fail.append("dispatch of %s: %d tiles per block do not wrap a ring of %d stages (%r)" % (op, d["tiles"], val, d))
                continue
            if key == "geo" and val and op in ("fwd_padded",):
                val = 0                                  # (no compile-time-geometry instantiation of the plain forward store)
            if d[key] != val:
                fail.append("dispatch of %s: %s = %d, the run expects %d (%r)" % (op, key, d[key], val, d))
    # the c64x2 inference twin takes layer1's eval epilogue from 256 x 256 pixels up
    if run == "c0_w32-device" and not table["ep"]["c64x2"]:
        fail.append("c64x2 does not take the eval epilogue of c0_w32")
    want_mode = {"fwd": 1, "fwd_padded": 0, "ep": 3, "dgrad": 0, "acc": 2, "macc": 2, "sums": 6, "sums_acc": 7, "sums2": 8}
    for op, d in table.items():
        if d["mode"] != want_mode.get(op, 0):
            fail.append("epilogue mode of %s: %d" % (op, d["mode"]))


def check_wgrad_dispatch(run, ops, G, fail):
    """the two vpd_op_wgrad launches of a case with a weight gradient: the atomics kernel without a slab, with one the kernel and pass
    instantiation opref.WG_ROUTES_CONV names; asked of both libraries before anything is launched"""
    if not G.cs.get("wgrad"):
        return {}
    kern, inst = R.WG_ROUTES_CONV[RUNS[run][0]]
    wa, wt = G.wgrad_args()
    table = {}
    for name, op in ops.items():
        d0, d1 = R.wg_dispatch(op.L, wa, wt, 0), R.wg_dispatch(op.L, wa, wt, 1)
        fail += R.wg_route_errors(d0, "%s wgrad_atomics" % name, kernel="atomics", inst=0)
        fail += R.wg_route_errors(d1, "%s wgrad_slab" % name, kernel=kern, inst=inst)
        table[name] = {"wgrad_atomics": d0, "wgrad_slab": d1}
    return table


def main():
    run, mode = sys.argv[1], sys.argv[2]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ops = {name: Ops(name) for name in ("bf16", "fp16")}
    if mode == "dispatch":                               # several runs of one environment, comma-separated
        for one in run.split(","):
            G, fail = Geo(R.CONV_CASES[RUNS[one][0]]), []
            table = dispatch_table(ops["bf16"], G)
            if table != dispatch_table(ops["fp16"], G):
                fail.append("the two libraries dispatch differently")
            check_dispatch(one, table, fail)
            wtable = check_wgrad_dispatch(one, ops, G, fail)
            print("RESULT " + json.dumps({"run": one, "fail": fail, "dispatch": table, "wgrad_dispatch": wtable}))
        return
    cs = R.CONV_CASES[RUNS[run][0]]
    G = Geo(cs)
    fail, record, digest = [], {}, {}
    table = dispatch_table(ops["bf16"], G)
    if table != dispatch_table(ops["fp16"], G):
        fail.append("the two libraries dispatch differently")
    check_dispatch(run, table, fail)
    wtable = check_wgrad_dispatch(run, ops, G, fail)
    if fail:                                             # a moved dispatch fails the run before anything is launched
        print("RESULT " + json.dumps({"fail": fail, "dispatch": table, "wgrad_dispatch": wtable, "record": record, "digest": digest}))
        return
    want = wanted(G, ops["bf16"].dispatch)
    seed = R.CONV_SEEDS[0]
    t0 = time.time()
    for regime in ("int", "rand"):
        shared = None
        for name, op in ops.items():
            o = R.conv_operands(cs, seed, regime, name)
            got = run_ops(op, G, o, want)
            for key, r in got.items():
                digest["%s/%s/%s" % (name, regime, key)] = r["sha"]
                if not r["kept"]:
                    fail.append("%s/%s/%s: wrote outside the interior" % (name, regime, key))
            if regime == "rand" and mode == "light":
                continue
            if regime == "int":
                shared = shared or references(cs, o, want, name, regime)      # the integer operands are the same for both libraries
                ref = shared
            else:
                ref = references(cs, o, want, name, regime)
            for key, r in got.items():
                want_t, bound = ref[key]
                tag = "%s/%s/%s" % (name, regime, key)
                g = r["got"]
                if regime == "int":
                    nbad = int((g != want_t).sum())
                    record[tag] = {"differ": nbad, "of": g.numel()}
                    if nbad:
                        fail.append("%s: %d of %d elements differ from the float64 reference (max |diff| %g)"
                                    % (tag, nbad, g.numel(), float((g - want_t).abs().max())))
                else:
                    err = (g - want_t).abs()
                    ratio = float((err / bound.clamp_min(1e-300)).max())
                    l2 = R.rel_l2(g, want_t)
                    record[tag] = {"max_err_over_bound": ratio, "rel_l2": l2}
                    print("%s %s max err / bound %.3f rel-L2 %.2e" % (run, tag, ratio, l2))
                    if not bool((err <= bound).all()) or not bool(torch.isfinite(g).all()):
                        fail.append("%s: %d elements beyond their bound (worst %.2f x)" % (tag, int((err > bound).sum()), ratio))
                    if l2 >= REL_TOL:
                        fail.append("%s: rel-L2 %.3e" % (tag, l2))
                # statistics rows: sums over the STORED output
                if "rows" in r:
                    stored = g
                    if key == "fwd":
                        w1, w2 = stored.sum(dim=(0, 2, 3)), (stored * stored).sum(dim=(0, 2, 3))
                        a1, a2 = stored.abs().sum(dim=(0, 2, 3)), w2
                    else:
                        gm = stored * o["keep_dx"]
                        w1, w2 = gm.sum(dim=(0, 2, 3)), (gm * o["z"]).sum(dim=(0, 2, 3))
                        a1, a2 = gm.abs().sum(dim=(0, 2, 3)), (gm * o["z"]).abs().sum(dim=(0, 2, 3))
                    pairs = [("rows", r["rows"], w1, w2, a1, a2)]
                    if r.get("rows2") is not None:
                        pairs.append(("rows2", r["rows2"], w1, (gm * o["z2"]).sum(dim=(0, 2, 3)), a1, (gm * o["z2"]).abs().sum(dim=(0, 2, 3))))
                    for rn, rows, s1, s2, m1, m2 in pairs:
                        e1, e2 = (rows[0] - s1).abs(), (rows[1] - s2).abs()
                        if regime == "int":
                            if float(e1.max()) != 0.0 or float(e2.max()) != 0.0:
                                fail.append("%s: %s differ from the sums over the stored output by %g / %g" % (tag, rn, float(e1.max()), float(e2.max())))
                        elif bool((e1 > R.SUM_TOL * m1).any()) or bool((e2 > R.SUM_TOL * m2).any()):
                            fail.append("%s: %s off by %.2e / %.2e of the absolute sums" % (tag, rn, float((e1 / m1).max()), float((e2 / m2).max())))
            del got
    record["seconds"] = time.time() - t0
    print("RESULT " + json.dumps({"fail": fail, "dispatch": table, "wgrad_dispatch": wtable, "record": record, "digest": digest}))


if __name__ == "__main__":
    main()
