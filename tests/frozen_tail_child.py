"""Child process of tests/test_frozen_bn_ops_gpu.py: the fused Bottleneck-tail kernels (vpd_op_conv1x1_bn, vpd_op_conv1x1_bn2) under
the frozen-BatchNorm hook, modes 0 .. 3, in both libraries.  The kernels size their grids by the CU budget, which is read once per
process (VPD_RESERVE_CUS), so the few-CU runs need a fresh interpreter -- as tests/bneck_tail_child.py, whose cases these are.
usage: frozen_tail_child.py <case of opref.TAIL_CASES>
z is never stored by these kernels; the references are the float64 closed forms of tests/opref_frozen.py on the unfused launch's
stored z (vpd_op_conv2d: the element type's rounding of the same accumulators, which test_bneck_tail_ops_gpu.py pins).
Prints "RESULT <json>": {"case", "fail": [...], "dispatch": {...}, "record": {...}}."""
import ctypes as C
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import opref as R  # noqa: E402
from tests import opref_frozen as Z  # noqa: E402
from tests.bneck_tail_child import MASK_SENT, Vec, dispatch, op_tail, op_tail2  # noqa: E402
from tests.conv_ops_child import SLACK, Geo, Ops, ptr, stream  # noqa: E402


def run_case(ops, cs, name, fail, record):
    L, T = ops.L, ops.T
    n, ci, co, h, w, two = cs["n"], cs["ci"], cs["co"], cs["h"], cs["w"], cs["two"]
    M, G = n * h * w, Geo(cs)
    dims = (n, h, w, ci, co)
    sides = ("", "2") if two else ("",)
    bad = lambda what: fail.append("%s: %s" % (name, what))
    o = R.tail_operands(cs, R.CONV_SEEDS[0], "rand", name)
    g = torch.Generator().manual_seed(co + n)
    for s in sides:      # statistics far from the batch's own and from 0 / 1, gamma of either sign
        o["rm" + s], o["rv" + s], o["gamma" + s], o["beta" + s] = Z.frozen_params(co, g)
    f32 = lambda t: t.float().cuda()
    xp, wf, z = {}, {}, {}
    for s in sides:
        xp[s], wf[s] = ops.padded(o["x" + s]), T.pack_fwd(o["w" + s].float(), dtype=ops.dt)
        y = ops.out_buffer(n, h, w, co, 0)
        ops.check(L.vpd_op_conv2d(ptr(xp[s]), ptr(wf[s]), ptr(y), None, *G.fwd_args(0), 0, stream()))
        torch.cuda.synchronize()
        z[s], _ = ops.read(y, n, h, w, co, 0)
    gam, bet = {s: f32(o["gamma" + s]) for s in sides}, {s: f32(o["beta" + s]) for s in sides}
    vec = {s: {k: Vec(co, o[k + s] if k in ("rm", "rv") else None) for k in ("mean", "rstd", "scale", "shift", "rm", "rv")} for s in sides}
    vec_t = lambda s: {k: v.t for k, v in vec[s].items()}
    before = {s: {k: vec[s][k].t.clone() for k in ("rm", "rv")} for s in sides}

    def rows_check(what, rows, want, mags):
        err = (rows.sum(dim=0).cpu() - want).abs()
        ratio = float((err / (R.SUM_TOL * mags).clamp_min(1e-300)).max())
        record["%s/%s" % (name, what)] = ratio
        if not ratio <= 1:
            bad("%s: off by %.2f x SUM_TOL of the sums of magnitudes" % (what, ratio))

    ops.check(L.vpd_op_set_bn_frozen(1))
    try:
        # ---- mode 0: the statistics pass(es); frozen or not they only take sums, which mode 1 then ignores ----
        rows = {}
        for s in sides:
            rows[s] = torch.zeros(4, 2, co, dtype=torch.float64, device="cuda")
            op_tail(ops, 0, dims, xp[s], wf[s], rows[s])
            torch.cuda.synchronize()
            zz = z[s]
            rows_check("mode0/rows" + s, rows[s], torch.stack([zz.sum(dim=(0, 2, 3)), (zz * zz).sum(dim=(0, 2, 3))]),
                       torch.stack([zz.abs().sum(dim=(0, 2, 3)), (zz * zz).sum(dim=(0, 2, 3))]))
        # ---- mode 1 ----
        out = ops.out_buffer(n, h, w, co, 1)
        maskb = torch.full((M * co // 8 + SLACK,), MASK_SENT, dtype=torch.uint8, device="cuda")
        resp = None if two else ops.padded(o["res"])
        fwd_side = lambda s: dict(vec_t(s), gamma=gam[s], beta=bet[s])
        if two:
            op_tail2(ops, 1, dims, xp, wf, rows, fwd_side(""), fwd_side("2"), out=out, mask=maskb)
        else:
            op_tail(ops, 1, dims, xp[""], wf[""], rows[""], fwd_side(""), res=resp, out=out, mask=maskb)
        torch.cuda.synchronize()
        got, kept = ops.read(out, n, h, w, co, 1)
        if not kept:
            bad("out: wrote outside the interior")
        if two:
            preA = Z.forward(z[""], o["gamma"], o["beta"], o["rm"], o["rv"], relu=False)[0]
            preB = Z.forward(z["2"], o["gamma2"], o["beta2"], o["rm2"], o["rv2"], relu=False)[0]
            ref = (preA + preB).clamp_min(0)
            bound = Z.out_bound(ref, z[""], o["gamma"], o["beta"], o["rm"], o["rv"], name,
                                second=(z["2"], o["gamma2"], o["beta2"], o["rm2"], o["rv2"]))
        else:
            ref = Z.forward(z[""], o["gamma"], o["beta"], o["rm"], o["rv"], res=o["res"])[0]
            bound = Z.out_bound(ref, z[""], o["gamma"], o["beta"], o["rm"], o["rv"], name, res=o["res"])
        ratio = float(((got - ref).abs() / bound).max())
        record[name + "/mode1/out"] = ratio
        if not ratio <= 1 or not bool(torch.isfinite(got).all()):
            bad("mode 1 out: worst element %.2f x its bound" % ratio)
        own = got != 0
        mb = maskb.cpu()
        if not bool((mb[M * co // 8:] == MASK_SENT).all()) or not torch.equal(mb[:M * co // 8].view(M, co // 8), R.mask_bits(R.nhwc(own).reshape(M, co))):
            bad("mode 1 bit map: not [stored out != 0], or written behind the map")
        saved = {}
        for s in sides:
            b = Z.stats_bounds(o["gamma" + s], o["beta" + s], o["rm" + s], o["rv" + s])
            rs = Z.rstd_of(o["rv" + s])
            sc = o["gamma" + s].double() * rs
            want = {"mean": o["rm" + s].double(), "rstd": rs, "scale": sc, "shift": o["beta" + s].double() - o["rm" + s].double() * sc}
            saved[s] = {}
            for k in want:
                v, k_kept = vec[s][k].read()
                saved[s][k] = v
                if not k_kept or not bool(((v - want[k]).abs() <= b[k]).all()):
                    bad("mode 1 %s%s: beyond its bound (or written behind the vector)" % (k, s))
            for k in ("rm", "rv"):
                if not torch.equal(vec[s][k].t, before[s][k]):
                    bad("mode 1 wrote %s%s" % (k, s))
        # ---- modes 2 and 3 under the forward's own bit map ----
        dt_dout = R.nhwc(o["dout"]).reshape(M, co).to(ops.dt).contiguous()
        doutd = dt_dout.cuda()
        bits = R.mask_bits(R.nhwc(own).reshape(M, co)).cuda()
        gm = o["dout"].double() * own
        brow = {s: torch.zeros(4, 2, co, dtype=torch.float64, device="cuda") for s in sides}
        dz = {s: ops.out_buffer(n, h, w, co, 1) for s in sides}
        dg, db = {s: Vec(co) for s in sides}, {s: Vec(co) for s in sides}
        for mode in (2, 3):
            m3 = mode == 3
            bwd_side = lambda s: dict(gamma=gam[s], mean=vec[s]["mean"].t, rstd=vec[s]["rstd"].t, dz=dz[s] if m3 else None,
                                      dgamma=dg[s].t, dbeta=db[s].t)
            if two:
                op_tail2(ops, mode, dims, xp, wf, brow, bwd_side(""), bwd_side("2"), mask=bits, dout=doutd)
            else:
                op_tail(ops, mode, dims, xp[""], wf[""], brow[""], bwd_side(""), mask=bits, dout=doutd)
            torch.cuda.synchronize()
            if not m3:
                for s in sides:
                    rows_check("mode2/rows" + s, brow[s], torch.stack([gm.sum(dim=(0, 2, 3)), (gm * z[s]).sum(dim=(0, 2, 3))]),
                               torch.stack([gm.abs().sum(dim=(0, 2, 3)), (gm * z[s]).abs().sum(dim=(0, 2, 3))]))
        if not torch.equal(doutd.cpu(), dt_dout):
            bad("d(out) was written")
        for s in sides:
            # the backward reads the vectors mode 1 stored: the references take those very fp32 values
            rdz, rdg, rdb = Z.backward(z[s], o["gamma" + s], saved[s]["mean"], saved[s]["rstd"], gm)
            gdz, kept = ops.read(dz[s], n, h, w, co, 1)
            ratio = float(((gdz - rdz).abs() / Z.dz_bound(rdz, name)).max())
            record["%s/mode3/dz%s" % (name, s)] = ratio
            if not kept or not ratio <= 1 or not bool(torch.isfinite(gdz).all()):
                bad("mode 3 dz%s: worst element %.2f x its bound (or written outside the interior)" % (s, ratio))
            (vg, kg), (vb, kb) = dg[s].read(), db[s].read()
            xhat = (z[s] - Z._v(saved[s]["mean"])) * Z._v(saved[s]["rstd"])
            b1, b2 = R.SUM_TOL * gm.abs().sum(dim=(0, 2, 3)), R.SUM_TOL * (gm * xhat).abs().sum(dim=(0, 2, 3))
            # (a channel that the ReLU switched off everywhere has no terms: its sums and their bounds are exactly zero)
            r1 = float(((vb - rdb).abs() / b1.clamp_min(1e-300)).max())
            r2 = float(((vg - rdg).abs() / b2.clamp_min(1e-300)).max())
            record["%s/mode3/dbeta_dgamma%s" % (name, s)] = [r1, r2]
            if not (kg and kb and r1 <= 1 and r2 <= 1):
                bad("mode 3 dbeta%s / dgamma%s: %.2f / %.2f x their bounds" % (s, s, r1, r2))
    finally:
        ops.check(L.vpd_op_set_bn_frozen(0))


def main():
    case = sys.argv[1]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cs = R.TAIL_CASES[case]
    ops = {name: Ops(name) for name in ("bf16", "fp16")}
    fail, record = [], {}
    d = dispatch(ops["bf16"], cs)
    if not d["eligible"]:
        fail.append("the launcher refuses this shape: %r" % (d,))
    else:
        for name, op in ops.items():
            run_case(op, cs, name, fail, record)
    print("RESULT " + json.dumps({"case": case, "fail": fail, "dispatch": d, "record": record}))


if __name__ == "__main__":
    main()
