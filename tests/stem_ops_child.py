"""Child process of tests/test_stem_ops_gpu.py: the stem-pool switches (VPD_STEM_PAIR, VPD_STEM_QUAD, VPD_STEM_POOLSUMS) are read
once per process, so each setting gets a fresh interpreter.  usage: stem_ops_child.py <bf16|fp16> <forward|backward>
Prints one line "RESULT <json>": {"fail": [...], "digest": {...}, "record": {...}}; the parent asserts on it."""
import ctypes as C
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import opref as R  # noqa: E402

CHUNK = 64                                   # crops per float64 reference chunk


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


class Ops:
    def __init__(self, name):
        from vpd_amd import _lib
        self.name, self.L, self._lib = name, _lib.lib(name), _lib
        assert self.L.vpd_elem_dtype().decode() == name
        self.dt = R.ELEM[name][0]

    def check(self, rc):
        self._lib.check(rc, "op", self.name)

    def forward(self, zd, scale, shift, train, opad=1):
        """zd: device NHWC element tensor.  out is pre-filled with 7 (the border must keep it), idx with 255."""
        n, H, W, c = zd.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out = torch.full((n, Ho + 2 * opad, Wo + 2 * opad, c), 7.0, dtype=self.dt, device="cuda")
        idx = torch.full((n, Ho, Wo, c), 255, dtype=torch.uint8, device="cuda") if train else None
        sc, sh = scale.float().cuda(), shift.float().cuda()
        self.check(self.L.vpd_op_stem_pool_forward(ptr(zd), ptr(sc), ptr(sh), ptr(out), ptr(idx), n, H, W, c, opad, stream()))
        torch.cuda.synchronize()
        return out, idx

    def backward(self, dpool_d, idx, zd, inp, pooled):
        n, H, W, c = zd.shape
        f = lambda t: t.float().cuda()
        mean, rstd, scale, shift, gamma, beta = (f(inp[k]) for k in ("mean", "rstd", "scale", "shift", "gamma", "beta"))
        rows = torch.zeros(16, 2, c, dtype=torch.float64, device="cuda")
        coef = torch.zeros(3, c, device="cuda")
        dz = torch.full((n, H, W, c), float("nan"), dtype=self.dt, device="cuda")
        dgamma, dbeta = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
        self.check(self.L.vpd_op_stem_pool_backward(ptr(dpool_d), ptr(idx), ptr(zd), ptr(mean), ptr(rstd), ptr(scale), ptr(shift),
                                                    ptr(gamma), ptr(beta), ptr(pooled), ptr(rows), ptr(coef), ptr(dz), ptr(dgamma),
                                                    ptr(dbeta), n, H, W, c, stream()))
        torch.cuda.synchronize()
        assert float(rows.abs().max()) == 0.0          # the accumulator rows are handed back zeroed
        return dz, dgamma.cpu().double(), dbeta.cpu().double()


def border_kept(out, opad):
    if opad == 0:
        return True
    o = out.float()
    return bool((o[:, :opad] == 7).all() and (o[:, -opad:] == 7).all() and (o[:, :, :opad] == 7).all() and (o[:, :, -opad:] == 7).all())


def run_forward(ops, fail, digest, record):
    name = ops.name
    shapes = dict(R.STEM_FWD_SHAPES, big=R.STEM_BIG)
    for key, (n, H, W) in shapes.items():
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        # ---- exact-grid inputs: equality ----
        zd = torch.empty(n, H, W, R.STEM_C, dtype=ops.dt, device="cuda")
        chunks = []
        _, scale, shift = R.stem_grid_inputs(1, 1, 1, R.STEM_C, 1000 + n)
        for b0 in range(0, n, CHUNK):
            zc, _, _ = R.stem_grid_inputs(min(CHUNK, n - b0), H, W, R.STEM_C, 77 * n + H + b0)
            zd[b0:b0 + zc.shape[0]] = R.nhwc(zc).to(ops.dt).cuda()
            chunks.append((b0, zc))
        out_t, idx = ops.forward(zd, scale, shift, True)
        out_e, _ = ops.forward(zd, scale, shift, False)
        tag = "%s/grid" % key
        if not (border_kept(out_t, 1) and border_kept(out_e, 1)):
            fail.append(tag + ": border written")
        if not torch.equal(out_t, out_e):
            fail.append(tag + ": eval output differs from train output")
        bad_v = bad_i = 0
        for b0, zc in chunks:
            p, taps, _ = R.stem_forward_ref(zc, scale, shift, name)
            m = zc.shape[0]
            got = R.nchw(out_t[b0:b0 + m, 1:-1, 1:-1].cpu().double())
            bad_v += int((got != p).sum())
            bad_i += int((R.nchw(idx[b0:b0 + m].cpu().long()) != taps).sum())
        if bad_v or bad_i:
            fail.append("%s: %d values, %d arg-max taps differ from the float64 reference" % (tag, bad_v, bad_i))
        digest[tag] = sha(out_t, idx)
        record[tag] = {"values_differ": bad_v, "taps_differ": bad_i, "windows": n * Ho * Wo * R.STEM_C}
        del zd, out_t, out_e, idx, chunks
        if key == "big":
            continue
        # ---- randn inputs, realistic scale / shift: values within one element ulp (+ the fp32 error of the affine map) ----
        for regime in R.REGIMES:
            inp = R.stem_random_inputs(n, H, W, R.STEM_C, 5 * n + W, name, regime)
            zd = R.nhwc(inp["z"]).to(ops.dt).cuda()
            out_t, idx = ops.forward(zd, inp["scale"], inp["shift"], True)
            out_e, _ = ops.forward(zd, inp["scale"], inp["shift"], False, opad=0)
            tag = "%s/randn/%s" % (key, regime)
            if not border_kept(out_t, 1):
                fail.append(tag + ": border written")
            if not torch.equal(out_t[:, 1:-1, 1:-1], out_e):
                fail.append(tag + ": eval output differs from train output")
            p, _, _ = R.stem_forward_ref(inp["z"], inp["scale"], inp["shift"], name)
            v = lambda t: t.double().view(1, -1, 1, 1)
            f32 = 2.0 ** -23 * ((inp["z"].double() * v(inp["scale"])).abs() + v(inp["shift"]).abs())
            bound = R.ulp(p, name) + torch.nn.functional.max_pool2d(f32, 3, 2, 1)
            got = R.nchw(out_t[:, 1:-1, 1:-1].cpu().double())
            err = (got - p).abs()
            nbad = int((err > bound).sum())
            if nbad or int(idx.max()) > 8:
                fail.append("%s: %d values beyond one ulp, max tap %d" % (tag, nbad, int(idx.max())))
            digest[tag] = sha(out_t, idx)
            record[tag] = {"beyond_bound": nbad, "max_err_over_bound": float((err / bound).max()), "exact_share": float((err == 0).double().mean())}


def run_backward(ops, fail, digest, record):
    name = ops.name
    poolsums = os.environ.get("VPD_STEM_POOLSUMS", "1") != "0"
    half_ulp_rel = 2.0 ** -(R.ELEM[name][1] + 1)          # 2^-9 (bf16), 2^-12 (fp16)
    gate = R.dz_l2_gate(name)
    for key, (n, H, W) in R.STEM_BWD_SHAPES.items():
        for regime in R.REGIMES:
            tag = "%s/%s" % (key, regime)
            c = R.STEM_C
            inp = R.stem_random_inputs(n, H, W, c, 5 * n + W, name, regime)
            dpool = R.stem_dpool(inp, name)
            zd = R.nhwc(inp["z"]).to(ops.dt).cuda()
            pooled, idx = ops.forward(zd, inp["scale"], inp["shift"], True)
            pooled[:, 0] = 0; pooled[:, -1] = 0; pooled[:, :, 0] = 0; pooled[:, :, -1] = 0      # the product's zero border
            dpool_d = R.nhwc(dpool).to(ops.dt).cuda()
            dz_d, dgamma, dbeta = ops.backward(dpool_d, idx, zd, inp, pooled)
            taps = R.nchw(idx.cpu().long())
            if int(taps.max()) > 8:
                fail.append(tag + ": arg-max tap out of range")
                continue
            ref = R.stem_backward_ref_B(inp["z"], inp["gamma"], inp["beta"], inp["mean"], inp["rstd"], dpool, taps)
            band = R.relu_band(inp["z"], inp["scale"], inp["shift"], ref["a"])
            share = float(band.double().mean())
            if share > R.BAND_CAP:
                fail.append("%s: %.2e of the elements in the ReLU band (cap %.0e)" % (tag, share, R.BAND_CAP))
            flip1 = (ref["routed"].abs() * band).sum(dim=(0, 2, 3))                      # what a flipped mask could move
            flip2 = ((ref["routed"] * ref["xhat"]).abs() * band).sum(dim=(0, 2, 3))
            ds1 = R.SUM_TOL * ref["abs1"] + flip1
            ds2 = R.SUM_TOL * ref["abs2"] + flip2
            rec = {"poolsums": poolsums, "band_share": share}
            if poolsums:
                # the pooled-side sums replace xhat by (a - beta) / gamma of the STORED activation: worst case per channel
                a_pool = torch.nn.functional.max_pool2d(ref["a"].clamp_min(0), 3, 2, 1)
                widen = half_ulp_rel * (dpool.double() * a_pool).abs().sum(dim=(0, 2, 3)) / inp["gamma"].double().abs()
                rec["dgamma_bound_zsums_max"] = float(ds2.max())
                ds2 = ds2 + widen
            e1, e2 = (dbeta - ref["dbeta"]).abs(), (dgamma - ref["dgamma"]).abs()
            ds1, ds2 = ds1.clamp_min(1e-300), ds2.clamp_min(1e-300)      # (a channel whose ReLU passes nothing: error and bound are both 0)
            rec.update(dbeta_err_max=float(e1.max()), dbeta_err_over_bound=float((e1 / ds1).max()),
                       dgamma_err_max=float(e2.max()), dgamma_bound_max=float(ds2.max()), dgamma_err_over_bound=float((e2 / ds2).max()),
                       dgamma_rel_l2=R.rel_l2(dgamma, ref["dgamma"]), dgamma_abs_max=float(ref["dgamma"].abs().max()))
            if bool((e1 > ds1).any()):
                fail.append("%s: dbeta off by %.3e x its bound" % (tag, float((e1 / ds1).max())))
            if bool((e2 > ds2).any()):
                fail.append("%s: dgamma off by %.3e x its bound" % (tag, float((e2 / ds2).max())))
            got = R.nchw(dz_d.cpu().double())
            if not bool(torch.isfinite(got).all()):
                fail.append(tag + ": dz not written everywhere")
                continue
            M = n * H * W
            bound = R.bn_dz_bound(ref["dz"], inp["gamma"], inp["rstd"], inp["mean"], inp["z"], ref["g"], ref["xhat"],
                                  ref["dbeta"], ref["dgamma"], ds1, ds2, M, name)

            def compare(want):
                err = (got - want).abs()
                over = (err / bound)[~band]
                return R.rel_l2(got, want), float(over.max()), int((over > 1).sum())
            l2, worst, nbad = compare(ref["dz"])
            rec.update(dz_rel_l2=l2, dz_gate=gate, dz_err_over_bound=worst, dz_beyond_bound=nbad)
            if l2 >= gate or nbad:
                fail.append("%s: dz rel-L2 %.3e (gate %.1e), %d elements beyond their bound (worst %.2f x)" % (tag, l2, gate, nbad, worst))
            # resolution: the same comparison against a reference whose xhat coefficient is 2 % off must fail
            off = R.bn_dz_closed_form(inp["z"], inp["gamma"], inp["mean"], inp["rstd"], ref["g"], 1.02)
            l2o, worsto, nbado = compare(off)
            rec.update(off_rel_l2=l2o, off_beyond_bound=nbado)
            if regime == "init" and not (l2o >= gate or nbado > 0):
                fail.append("%s: a 2 %% coefficient error passes (rel-L2 %.3e, gate %.1e, %d beyond bound)" % (tag, l2o, gate, nbado))
            digest[tag] = sha(dz_d)
            record[tag] = rec


def main():
    name, what = sys.argv[1], sys.argv[2]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ops = Ops(name)
    fail, digest, record = [], {}, {}
    (run_forward if what == "forward" else run_backward)(ops, fail, digest, record)
    print("RESULT " + json.dumps({"fail": fail, "digest": digest, "record": record}))


if __name__ == "__main__":
    main()
