"""Child process of tests/test_bneck_tail_ops_gpu.py (and, with "dispatch", of tests/test_bneck_tail_cpu.py): the fused Bottleneck-tail
kernels size their grids by the CU budget, and VPD_RESERVE_CUS is read once per process, so each run gets a fresh interpreter.
usage: bneck_tail_child.py <run id[,run id...]> <dispatch|full>
  dispatch  no launch: what vpd_op_conv1x1_bn_dispatch says for the run (works without a GPU: 256 CUs assumed)
  full      both libraries, both input regimes, every mode of vpd_op_conv1x1_bn / vpd_op_conv1x1_bn2 against the float64 chain of
            tests/opref.py (tail_forward, tail_backward)
Prints one line "RESULT <json>" per run: {"run", "fail": [...], "dispatch": {...}, "record": {...}}; the parent asserts on it.
record["<library>/<regime>/digests"]: sha256 of every buffer the fused launches wrote, slack included -- not asserted on; it is what
lets two builds of the libraries (VPD_LIB_PATH / VPD_LIB_PATH_F16) be compared bit for bit."""
import ctypes as C
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import opref as R  # noqa: E402
from tests.conv_ops_child import FEW, SENT, SLACK, Geo, Ops, ptr, sha, stream  # noqa: E402

OUT5 = ("eligible", "lanes", "channel_tiles", "tiles", "ring")
# run id -> (case of opref.TAIL_CASES, environment, what vpd_op_conv1x1_bn_dispatch must report on a 256-CU device)
RUNS = {
    "k64_w8-few":       ("k64_w8", FEW, dict(eligible=1, lanes=8, channel_tiles=1, tiles=12, ring=8)),
    "k64_w16-few":      ("k64_w16", FEW, dict(eligible=1, lanes=8, channel_tiles=1, tiles=12, ring=8)),
    "k64_co512-few":    ("k64_co512", FEW, dict(eligible=1, lanes=8, channel_tiles=2, tiles=12, ring=8)),
    "k128_w8-few":      ("k128_w8", FEW, dict(eligible=1, lanes=8, channel_tiles=1, tiles=8, ring=5)),
    "k128_co512-few":   ("k128_co512", FEW, dict(eligible=1, lanes=8, channel_tiles=2, tiles=8, ring=5)),
    "two_w8-few":       ("two_w8", FEW, dict(eligible=1, lanes=8, channel_tiles=1, tiles=8, ring=5)),
    "two_w16-few":      ("two_w16", FEW, dict(eligible=1, lanes=8, channel_tiles=1, tiles=12, ring=5)),
    "k64_w32-device":   ("k64_w32", {}, dict(eligible=1, lanes=256, channel_tiles=1, tiles=3, ring=8)),
    "k128_w32-device":  ("k128_w32", {}, dict(eligible=1, lanes=256, channel_tiles=1, tiles=3, ring=5)),
    "two_w32-device":   ("two_w32", {}, dict(eligible=1, lanes=256, channel_tiles=1, tiles=3, ring=5)),
}
MASK_SENT = 0xA5
F = C.c_float


def dispatch(ops, cs):
    out = (C.c_int * 5)()
    ops.check(ops.L.vpd_op_conv1x1_bn_dispatch(cs["n"], cs["h"], cs["w"], cs["ci"], cs["co"], 1 if cs["two"] else 0, out))
    return dict(zip(OUT5, list(out)))


def check_dispatch(run, d, fail):
    cs, _, exp = R.TAIL_CASES[RUNS[run][0]], RUNS[run][1], RUNS[run][2]
    for key, val in exp.items():
        if d[key] != val:
            fail.append("dispatch: %s = %d, the run expects %d (%r)" % (key, d[key], val, d))
    if d["ring"] != R.tail_ring(cs):
        fail.append("ring depth %d, the references assume %d" % (d["ring"], R.tail_ring(cs)))
    if cs["few"] and (d["tiles"] <= d["ring"] or d["lanes"] != R.TAIL_LANES):
        fail.append("%d tiles per block on %d lanes do not wrap a ring of %d stages" % (d["tiles"], d["lanes"], d["ring"]))


class Vec:
    """an fp32 [co] device vector with sentinel slack behind it"""

    def __init__(self, co, init=None):
        t = torch.full((co + 64,), SENT, dtype=torch.float32)
        if init is not None:
            t[:co] = init.float()
        self.co, self.t = co, t.cuda()

    def read(self):
        c = self.t.cpu()
        return c[:self.co].double(), bool((c[self.co:] == SENT).all())


def _side(side, *names):
    """a BatchNorm's device pointers in the order named; what the dict does not hold goes as null"""
    return [ptr((side or {}).get(k)) for k in names]


def op_tail(ops, mode, dims, x, w, rows, side=None, res=None, out=None, mask=None, dout=None):
    """vpd_op_conv1x1_bn (stride 1): dims = (n, h, w, ci, co); side: the BatchNorm's tensors by name among gamma beta rm rv mean rstd
    scale shift dz dgamma dbeta, each mode passing the ones it wants read or written"""
    n, h, wd, ci, co = dims
    ops.check(ops.L.vpd_op_conv1x1_bn(mode, ptr(x), ptr(w), n, h, wd, 1, ci, co, ptr(rows), *_side(side, "gamma", "beta", "rm", "rv"),
                                      F(R.BN_MOMENTUM), F(R.BN_EPS), *_side(side, "mean", "rstd", "scale", "shift"), ptr(res), ptr(out),
                                      ptr(mask), ptr(dout), *_side(side, "dz", "dgamma", "dbeta"), stream()))


def op_tail2(ops, mode, dims, x, w, rows, side, side2, out=None, mask=None, dout=None):
    """vpd_op_conv1x1_bn2: x / w / rows map a side key ("" the closing convolution, "2" the branch) to its tensor; side / side2 as op_tail's"""
    n, h, wd, ci, co = dims
    fwd = ("gamma", "beta", "rm", "rv", "mean", "rstd", "scale", "shift")
    ops.check(ops.L.vpd_op_conv1x1_bn2(mode, ptr(x[""]), ptr(w[""]), ptr(x["2"]), ptr(w["2"]), n, h, wd, ci, ci, co, ptr(rows[""]), ptr(rows["2"]),
                                       *_side(side, *fwd), *_side(side2, *fwd), F(R.BN_MOMENTUM), F(R.BN_EPS), ptr(out), ptr(mask), ptr(dout),
                                       *_side(side, "dz"), *_side(side2, "dz"), *_side(side, "dgamma", "dbeta"), *_side(side2, "dgamma", "dbeta"),
                                       stream()))


def close(got, want, rtol, atol=0.0):
    return bool(((got - want).abs() <= atol + rtol * want.abs()).all())


def run_case(ops, cs, o, regime, name, fail, record):
    """every mode of the case in one library and one regime"""
    L, T = ops.L, ops.T
    n, ci, co, h, w, two = cs["n"], cs["ci"], cs["co"], cs["h"], cs["w"], cs["two"]
    M, G, exact = n * h * w, Geo(cs), regime == "int"
    dims = (n, h, w, ci, co)
    tag = "%s/%s/" % (name, regime)
    sides = ("", "2") if two else ("",)
    bad = lambda what: fail.append(tag + what)
    nul = None
    dig = record.setdefault(tag + "digests", {})

    # ---- operands on the device; z: the unfused launch's stored output, itself checked against the float64 convolution ----
    xp, wf, zdev, z = {}, {}, {}, {}
    for s in sides:
        xp[s], wf[s] = ops.padded(o["x" + s]), T.pack_fwd(o["w" + s].float(), dtype=ops.dt)
        y = ops.out_buffer(n, h, w, co, 0)
        ops.check(L.vpd_op_conv2d(ptr(xp[s]), ptr(wf[s]), ptr(y), None, *G.fwd_args(0), 0, stream()))
        torch.cuda.synchronize()
        stored, kept = ops.read(y, n, h, w, co, 0)
        conv = R.tail_conv(o["x" + s], o["w" + s])
        if not kept:
            bad("z%s: wrote outside the tensor" % s)
        if exact:
            nbad = int((stored != conv).sum())
            record[tag + "z" + s] = {"differ": nbad, "of": conv.numel()}
            if nbad:
                bad("z%s: %d elements of the unfused convolution differ from float64" % (s, nbad))
            z[s] = conv
        else:
            b = R.conv_bound(conv, R.conv_gamma(R.tail_conv(o["x" + s].abs(), o["w" + s].abs()), ci), name)
            ratio = float(((stored - conv).abs() / b).max())
            record[tag + "z" + s] = {"max_err_over_bound": ratio}
            if ratio > 1 or not bool(torch.isfinite(stored).all()):
                bad("z%s: the unfused convolution is %.2f x its bound off float64" % (s, ratio))
            z[s] = stored
        zdev[s] = y
    fw = R.tail_forward(cs, o, z[""], z.get("2"), exact, name)
    stat = {"": fw["st"], "2": fw["st2"]}

    def rows_check(what, rows, want, mags):
        got = rows.sum(dim=0).cpu()
        err = (got - want).abs()
        if exact:
            nbad = int((err != 0).sum())
            record[tag + what] = {"differ": nbad, "of": err.numel()}
            if nbad:
                bad("%s: %d sums differ from the float64 sums (max %g)" % (what, nbad, float(err.max())))
        else:
            ratio = float((err / (R.SUM_TOL * mags).clamp_min(1e-300)).max())
            record[tag + what] = {"max_err_over_tol": ratio}
            if ratio > 1 or not bool(torch.isfinite(got).all()):
                bad("%s: off by %.2f x SUM_TOL of the sums of magnitudes" % (what, ratio))

    # ---- mode 0: the statistics pass(es) ----
    rows = {}
    for s in sides:
        rows[s] = torch.zeros(4, 2, co, dtype=torch.float64, device="cuda")
        op_tail(ops, 0, dims, xp[s], wf[s], rows[s])
        torch.cuda.synchronize()
        dig["rows" + s] = sha(rows[s])
        st = stat[s]
        rows_check("rows" + s, rows[s], torch.stack([st["s1"], st["s2"]]), torch.stack([st["abs1"], st["s2"]]))

    # ---- mode 1: finalize + out + bit map ----
    f32 = lambda t: t.float().cuda()
    gam, bet = {s: f32(o["gamma" + s]) for s in sides}, {s: f32(o["beta" + s]) for s in sides}
    vec = {s: {k: Vec(co, o[k + s] if k in ("rm", "rv") else None) for k in ("mean", "rstd", "scale", "shift", "rm", "rv")} for s in sides}
    out = ops.out_buffer(n, h, w, co, 1)
    maskb = torch.full((M * co // 8 + SLACK,), MASK_SENT, dtype=torch.uint8, device="cuda")
    resp = None if two else ops.padded(o["res"])
    vp = lambda s, k: ptr(vec[s][k].t)
    vec_t = lambda s: {k: v.t for k, v in vec[s].items()}
    fwd_side = lambda s: dict(vec_t(s), gamma=gam[s], beta=bet[s])
    if two:
        op_tail2(ops, 1, dims, xp, wf, rows, fwd_side(""), fwd_side("2"), out=out, mask=maskb)
    else:
        op_tail(ops, 1, dims, xp[""], wf[""], rows[""], fwd_side(""), res=resp, out=out, mask=maskb)
    torch.cuda.synchronize()
    dig.update({"out": sha(out), "mask": sha(maskb)})
    dig.update({k + s: sha(t.t) for s in sides for k, t in vec[s].items()})
    got, kept = ops.read(out, n, h, w, co, 1)
    if not kept:
        bad("out: wrote outside the interior")
    ratio = float(((got - fw["out"]).abs() / fw["bound"]).max())
    record[tag + "out"] = {"max_err_over_bound": ratio, "rel_l2": R.rel_l2(got, fw["out"])}
    print("%s%s max err / bound %.3f" % (tag, "out", ratio))
    if ratio > 1 or not bool(torch.isfinite(got).all()):
        bad("out: %d elements beyond their bound (worst %.2f x)" % (int(((got - fw["out"]).abs() > fw["bound"]).sum()), ratio))
    mb = maskb.cpu()
    own = got != 0
    if not bool((mb[M * co // 8:] == MASK_SENT).all()):
        bad("bit map: wrote behind the map")
    if not torch.equal(mb[:M * co // 8].view(M, co // 8), R.mask_bits(R.nhwc(own).reshape(M, co))):
        bad("bit map: not [stored out != 0]")
    for s in sides:
        st, v = stat[s], {}
        for k, t in vec[s].items():
            v[k], k_kept = t.read()
            if not k_kept:
                bad("%s%s: wrote behind the vector" % (k, s))
        ok = (close(v["mean"], st["mean"], R.BN_RTOL, R.BN_MEAN_ATOL) and close(v["rstd"], st["rstd"], R.BN_RTOL)
              and close(v["scale"], st["scale"], R.BN_RTOL) and close(v["shift"], st["shift"], R.BN_RTOL, R.BN_MEAN_ATOL)
              and close(v["rm"], st["rm"], R.BN_RTOL, R.BN_MEAN_ATOL) and close(v["rv"], st["rv"], R.BN_RTOL))
        if not ok:
            bad("BatchNorm%s: mean / rstd / scale / shift / running statistics beyond the gates of test_batchnorm_forward_op" % s)
    # ... bit for bit what the unfused BatchNorm launch makes of the stored z and the same rows
    same = True
    for s in sides:
        u = {k: Vec(co, o[k + s] if k in ("rm", "rv") else None) for k in ("mean", "rstd", "scale", "shift", "rm", "rv")}
        out_u = ops.out_buffer(n, h, w, co, 1)
        mask_u = torch.full((M * co // 8 + SLACK,), MASK_SENT, dtype=torch.uint8, device="cuda")
        ops.check(L.vpd_op_bn_forward(ptr(zdev[s]), ptr(rows[s]), ptr(gam[s]), ptr(bet[s]), ptr(u["rm"].t), ptr(u["rv"].t), ptr(u["mean"].t),
                                      ptr(u["rstd"].t), ptr(u["scale"].t), ptr(u["shift"].t), nul if two else ptr(resp), ptr(out_u),
                                      nul if two else ptr(mask_u), n, h, w, co, 0 if two else 1, F(R.BN_MOMENTUM), F(R.BN_EPS), stream()))
        torch.cuda.synchronize()
        for k in u:
            same = same and torch.equal(u[k].t, vec[s][k].t)
        if not two:          # (the unfused launch has no two-BatchNorm operator form: its coefficients are compared, out is not)
            inner = lambda t: t[:n * (h + 2) * (w + 2) * co].view(n, h + 2, w + 2, co)[:, 1:-1, 1:-1]
            same = same and torch.equal(inner(out_u), inner(out)) and torch.equal(mask_u, maskb)
    record[tag + "fwd_bit_identical_to_unfused"] = bool(same)
    if not same:
        bad("forward: not bit-identical to vpd_op_bn_forward on the stored z and the same rows")

    # ---- modes 2 and 3 under a random bit map and under the forward's own ----
    dt_dout = R.nhwc(o["dout"]).reshape(M, co).to(ops.dt).contiguous()
    doutd = dt_dout.cuda()
    for which, mask in (("rand_map", o["keep"]), ("own_map", own)):
        bw = R.tail_backward(cs, o, z[""], z.get("2"), fw, mask, name)
        side_ref = {"": (bw["b"], bw["bound"]), "2": (bw.get("b2"), bw.get("bound2"))}
        bits = R.mask_bits(R.nhwc(mask).reshape(M, co)).cuda()
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
                    dig["%s/rows%s" % (which, s)] = sha(brow[s])
                    b = side_ref[s][0]
                    rows_check("%s/rows%s" % (which, s), brow[s], torch.stack([b["r1"], b["r2"]]), torch.stack([b["abs1"], b["absz"]]))
        if not torch.equal(doutd.cpu(), dt_dout):
            bad(which + ": d(out) was written")
        same = True
        for s in sides:
            b, bound = side_ref[s]
            dig.update({"%s/dz%s" % (which, s): sha(dz[s]), "%s/dgamma%s" % (which, s): sha(dg[s].t), "%s/dbeta%s" % (which, s): sha(db[s].t)})
            gdz, kept = ops.read(dz[s], n, h, w, co, 1)
            if not kept:
                bad("%s/dz%s: wrote outside the interior" % (which, s))
            ratio = float(((gdz - b["dz"]).abs() / bound).max())
            record["%s%s/dz%s" % (tag, which, s)] = {"max_err_over_bound": ratio, "rel_l2": R.rel_l2(gdz, b["dz"])}
            print("%s%s/dz%s max err / bound %.3f" % (tag, which, s, ratio))
            if ratio > 1 or not bool(torch.isfinite(gdz).all()):
                bad("%s/dz%s: %d elements beyond their bound (worst %.2f x)" % (which, s, int(((gdz - b["dz"]).abs() > bound).sum()), ratio))
            (vg, kg), (vb, kb) = dg[s].read(), db[s].read()
            if not (kg and kb):
                bad("%s/dgamma%s, dbeta%s: wrote behind the vector" % (which, s, s))
            e1, e2 = (vb - b["dbeta"]).abs(), (vg - b["dgamma"]).abs()
            r1 = float((e1 / (R.SUM_TOL * b["abs1"]).clamp_min(1e-300)).max())
            r2 = float((e2 / (R.SUM_TOL * b["abs2"]).clamp_min(1e-300)).max())
            record["%s%s/dgamma_dbeta%s" % (tag, which, s)] = {"dbeta_err_over_tol": r1, "dgamma_err_over_tol": r2}
            if r1 > 1 or r2 > 1:
                bad("%s: dbeta%s / dgamma%s off by %.2f / %.2f x SUM_TOL of the sums of magnitudes" % (which, s, s, r1, r2))
            # measured, not gated: does mode 3 reproduce the unfused apply launch bit for bit?
            dz_u, dg_u, db_u = ops.out_buffer(n, h, w, co, 1), Vec(co), Vec(co)
            ops.check(L.vpd_op_bn_backward_apply(ptr(doutd), ptr(zdev[s]), ptr(bits), ptr(brow[s]), ptr(gam[s]), vp(s, "mean"), vp(s, "rstd"),
                                                 ptr(dz_u), ptr(dg_u.t), ptr(db_u.t), n, h, w, co, stream()))
            torch.cuda.synchronize()
            inner = lambda t: t[:n * (h + 2) * (w + 2) * co].view(n, h + 2, w + 2, co)[:, 1:-1, 1:-1]
            same = same and torch.equal(inner(dz_u), inner(dz[s])) and torch.equal(dg_u.t, dg[s].t) and torch.equal(db_u.t, db[s].t)
        record["%s%s/bwd_bit_identical_to_unfused" % (tag, which)] = bool(same)


def main():
    runs, mode = sys.argv[1].split(","), sys.argv[2]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ops = {name: Ops(name) for name in ("bf16", "fp16")}
    for run in runs:
        cs = R.TAIL_CASES[RUNS[run][0]]
        fail, record = [], {}
        d = dispatch(ops["bf16"], cs)
        if d != dispatch(ops["fp16"], cs):
            fail.append("the two libraries dispatch differently")
        check_dispatch(run, d, fail)
        if mode == "dispatch" or fail:                    # a moved dispatch fails the run before anything is launched
            print("RESULT " + json.dumps({"run": run, "fail": fail, "dispatch": d, "record": record}))
            continue
        t0 = time.time()
        for regime in ("int", "rand"):
            for name, op in ops.items():
                o = R.tail_operands(cs, R.CONV_SEEDS[0], regime, name)
                run_case(op, cs, o, regime, name, fail, record)
        record["seconds"] = time.time() - t0
        print("RESULT " + json.dumps({"run": run, "fail": fail, "dispatch": d, "record": record}))


if __name__ == "__main__":
    main()
