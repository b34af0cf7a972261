"""Child process of tests/test_wgrad_pair_gpu.py: vpd_op_wgrad_pair (a down-sampling BasicBlock's 3x3 stride-2 conv1 and its 1x1
stride-2 branch in one halo launch) in one library, every case of CASES in both input regimes.  The parent sets VPD_WGRAD_1X1=1, so
that the 1x1 reference call of vpd_op_wgrad takes the halo + slab path the step uses (the library reads its switches once).
usage: wgrad_pair_child.py <bf16|fp16>
Prints one line "RESULT <json>": {case: {"fail": [...], "figures": {...}}}; the parent asserts on it."""
import ctypes as C
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import opref as R  # noqa: E402

SENT = -12352.0              # no integer-regime sum (|v| <= 2^15 here, an integer) and no randn sum comes near it by accident
SLACK = 4096                 # floats behind every gradient buffer
REL_TOL = 4e-3               # whole-tensor gate of tests/test_ops_gpu.py (fp32 accumulation of exact products sits far below it)

# The three stage boundaries of ResNet-18/34 on 128 x 128 crops: (Ci, Co, output H = W, crops).  Splits (vpd_wgrad_split: 256 / tiles,
# 64-pixel chunks): l2 two tiles, 128 splits; l3 eight tiles, 32 splits; l4 32 tiles, 8 splits, four images per chunk.
CASES = {
    "l2_n5":  (64, 128, 16, 5),      # 20 chunks, 20 splits of one
    "l2_n70": (64, 128, 16, 70),     # 280 chunks: 94 splits of three, the last one holds ONE chunk
    "l3_n6":  (128, 256, 8, 6),      # 6 splits of one
    "l3_n37": (128, 256, 8, 37),     # 37 chunks: 19 splits of two, the last one holds one
    "l4_n5":  (256, 512, 4, 5),      # two chunks, the second one ragged (one image of four)
    "l4_n6":  (256, 512, 4, 6),      # ragged: two images of four
    "l4_n67": (256, 512, 4, 67),     # 17 chunks: 6 splits of three, the last one holds two, the last chunk three images
}


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def padded(t, dt):
    """float64 NCHW -> element-type NHWC behind a zero border of 1, flat, on the GPU"""
    n, c, h, w = t.shape
    buf = torch.zeros(n, h + 2, w + 2, c, dtype=dt)
    buf[:, 1:-1, 1:-1, :] = t.permute(0, 2, 3, 1).to(dt)
    return buf.flatten().cuda()


def operands(ci, co, ho, n, regime, name, seed):
    g = torch.Generator().manual_seed(seed * 1000 + n + ci + ho)
    shapes = ((n, ci, 2 * ho, 2 * ho), (n, co, ho, ho), (n, co, ho, ho))
    if regime == "int":      # {-1, 0, 1}, density 1/2: every partial sum an integer below 2^24
        return [R._sparse_int(s, 0.5, g) for s in shapes]
    return [R.elem_round(torch.randn(s, generator=g), name).double() for s in shapes]


def run_case(L, check, name, cid, ci, co, ho, n):
    dt = R.ELEM[name][0]
    fail, fig = [], {}
    taps3 = (C.c_int * 9)(3, 3, 0, 1, 0, 1, 0, 3, 1)
    taps1 = (C.c_int * 9)(1, 1, 1, 1, 1, 1, 0, 1, 1)
    nslab = L.vpd_op_wgrad_slab_bytes() // 4
    slab = torch.empty(nslab, dtype=torch.float32, device="cuda")
    slab2 = torch.empty(nslab, dtype=torch.float32, device="cuda")
    geom = (n, ho + 2, ho + 2, co, 1, 2 * ho + 2, 2 * ho + 2, ci, ho, ho, 2, ci, co)
    n3, n1 = 9 * co * ci, co * ci
    # the two reference launches: conv1 on the halo 3x3 route, the branch (VPD_WGRAD_1X1=1) on the halo 1x1 route, both on the pass
    # instantiation the case names (13 passes: the two-stage ring); nothing is launched when the launcher says otherwise
    inst = R.WG_ROUTES_PAIR[cid]
    fail += R.wg_route_errors(R.wg_dispatch(L, geom, taps3, 1), "%s wgrad 3x3" % cid, kernel="halo3x3", inst=inst, stages=2 if inst == 13 else 3)
    fail += R.wg_route_errors(R.wg_dispatch(L, geom, taps1, 1), "%s wgrad 1x1" % cid, kernel="halo1x1", inst=inst, stages=2 if inst == 13 else 3)
    if fail:
        return {"fail": fail, "figures": fig}
    for regime in ("int", "randn"):
        x, dz, dz2 = operands(ci, co, ho, n, regime, name, 17)
        xp, dzp, dz2p = padded(x, dt), padded(dz, dt), padded(dz2, dt)
        new = lambda m: torch.full((m + SLACK,), SENT, dtype=torch.float32, device="cuda")
        dw, dwb, rdw, rdwb = new(n3), new(n1), new(n3), new(n1)
        slab.fill_(SENT)
        slab2.fill_(SENT)
        check(L.vpd_op_wgrad_pair(ptr(dzp), ptr(dz2p), ptr(xp), ptr(dw), ptr(dwb), *geom, taps3, ptr(slab), ptr(slab2), stream()),
              "wgrad_pair", name)
        torch.cuda.synchronize()
        # the two launches it replaces, as the step states them (the 1x1 on the halo path: VPD_WGRAD_1X1=1)
        slab.fill_(SENT)
        check(L.vpd_op_wgrad(ptr(dzp), ptr(xp), ptr(rdw), *geom, taps3, ptr(slab), stream()), "wgrad 3x3", name)
        check(L.vpd_op_wgrad(ptr(dz2p), ptr(xp), ptr(rdwb), *geom, taps1, ptr(slab2), stream()), "wgrad 1x1", name)
        torch.cuda.synchronize()
        for key, got, ref, m in (("dw", dw, rdw, n3), ("dw2", dwb, rdwb, n1)):
            if not bool((got[m:] == SENT).all()) or not bool((ref[m:] == SENT).all()):
                fail.append("%s %s: the slack behind the gradient lost its sentinel" % (regime, key))
            if bool((got[:m] == SENT).any()):
                fail.append("%s %s: elements left unwritten" % (regime, key))
            nd = int((got[:m].view(torch.int32) != ref[:m].view(torch.int32)).sum())
            fig["%s/%s/bits_differ" % (regime, key)] = nd
            if nd:
                fail.append("%s %s: %d of %d elements differ in bits from the two-launch path (max |d| %.3e)"
                            % (regime, key, nd, m, float((got[:m] - ref[:m]).abs().max())))
        # float64 conv2d backward on the CPU
        cs3 = dict(ci=ci, co=co, k=3, stride=2, h=2 * ho, w=2 * ho)
        cs1 = dict(ci=ci, co=co, k=1, stride=2, h=2 * ho, w=2 * ho)
        w3 = R.conv_wgrad(x, dz, cs3).permute(2, 3, 0, 1).reshape(9, co, ci)
        w1 = R.conv_wgrad(x, dz2, cs1).reshape(co, ci)
        for key, got, ref in (("dw", dw[:n3].cpu().double().view(9, co, ci), w3), ("dw2", dwb[:n1].cpu().double().view(co, ci), w1)):
            if regime == "int":
                bad = int((got != ref).sum())
                fig["int/%s/not_equal" % key] = bad
                if bad:
                    fail.append("int %s: %d elements differ from float64 (max |d| %g)" % (key, bad, float((got - ref).abs().max())))
            else:
                rl = R.rel_l2(got, ref)
                fig["randn/%s/rel_l2" % key] = rl
                if not rl <= REL_TOL:
                    fail.append("randn %s: rel-L2 %.3e > %.1e" % (key, rl, REL_TOL))
    return {"fail": fail, "figures": fig}


def main():
    name = sys.argv[1]
    from vpd_amd._lib import check, lib
    L = lib(name)
    out = {}
    for cid, (ci, co, ho, n) in CASES.items():
        out[cid] = run_case(L, check, name, cid, ci, co, ho, n)
        print(cid, name, json.dumps(out[cid]["figures"]), flush=True)
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
