"""Child process of tests/test_wgrad_routes_gpu.py: the 64-wide weight-gradient kernels of one library, route by route.  The library
reads its switches once, so the run that needs VPD_WGRAD_1X1=1 gets a process of its own.
usage: wgrad_routes_child.py <bf16|fp16> <group|stem|halo1x1>
  group    vpd_op_wgrad_group (conv_wgrad_halo_grouped_kernel): every group of opref.WG_GROUPS
  stem     vpd_op_wgrad on the stem layout: conv_wgrad_stem_kernel at every TR, and the shapes it refuses on the atomics kernel
  halo1x1  (the parent sets VPD_WGRAD_1X1=1) the 1x1 cases of tests/test_ops_gpu.py::CONV_CASES as the centre tap of the halo kernel
Every run first asks the dispatch query and launches nothing when the answer is not what the run names.  Two regimes: integer
operands from {-1, 0, 1} (M < 2^24: every partial sum is an integer fp32 holds, so the result must EQUAL float64 conv2d backward),
and element-rounded randn within opref.wg_bound per element.  Gradient buffers are pre-filled with a sentinel (the atomics kernel's:
zeros), every element must be written and the 4,096 floats behind each must keep the sentinel.
Prints one line "RESULT <json>": {case: {"fail": [...], "figures": {...}, "dispatch": ...}}; the parent asserts on it."""
import ctypes as C
import json
import os
import sys
import zlib

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import opref as R  # noqa: E402

SENT = -12352.0              # no integer-regime sum (an integer, |v| < 2^24) and no randn sum comes near it by accident
SLACK = 4096                 # floats behind every gradient buffer
T3 = (C.c_int * 9)(3, 3, 0, 1, 0, 1, 0, 3, 1)
T1 = (C.c_int * 9)(1, 1, 1, 1, 1, 1, 0, 1, 1)
TSTEM = (C.c_int * 9)(7, 1, 0, 1, 0, 0, 0, 1, 0)


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


def new_dw(m, fill=SENT):
    dw = torch.full((m + SLACK,), SENT, dtype=torch.float32, device="cuda")
    dw[:m] = fill
    return dw


def seed_of(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode()) % (1 << 31)


def conv_geometry(n, ci, co, h, w, st):
    """the geometry arguments of vpd_op_wgrad / vpd_op_wgrad_dispatch for x [n][ci][h][w] behind a border of 1"""
    ho, wo = h // st, w // st
    return (n, ho + 2, wo + 2, co, 1, h + 2, w + 2, ci, ho, wo, st, ci, co)


def stem_geometry(n, h, w):
    """... for the stem: dz dense, 8 channels behind a border of 3 (right: 5), one 64-deep tap per kernel row"""
    return (n, h // 2, w // 2, 64, 0, h + 6, w + 8, 8, h // 2, w // 2, 2, 64, 64)


def dispatch(L, geom, taps, has_slab, prefer=0):
    return R.wg_dispatch(L, geom, taps, has_slab, prefer)


def expect(d, fail, what, **want):
    fail.extend(R.wg_route_errors(d, what, **want))


def check_buffer(dw, m, tag, fail, zeroed=False):
    """sentinel rules of a gradient buffer -> its m floats on the CPU"""
    buf = dw.cpu()
    if not bool((buf[m:] == SENT).all()):
        fail.append("%s: the slack behind the gradient lost its sentinel" % tag)
    if not zeroed and bool((buf[:m] == SENT).any()):
        fail.append("%s: %d elements left unwritten" % (tag, int((buf[:m] == SENT).sum())))
    return buf[:m]


def compare(tag, got, ref, bound, fail, fig):
    """got, ref: float64 [co][ci][k][k]; bound None: equality (integer regime)"""
    if not bool(torch.isfinite(got).all()):
        fail.append("%s: not finite" % tag)
        return
    if bound is None:
        bad = int((got != ref).sum())
        fig[tag + "/not_equal"] = bad
        if bad:
            fail.append("%s: %d of %d elements differ from float64 (max |d| %g)" % (tag, bad, got.numel(), float((got - ref).abs().max())))
        return
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    fig[tag + "/max_err_over_bound"] = ratio
    print("%s max err / bound %.4f" % (tag, ratio), flush=True)
    if not bool((err <= bound).all()):
        fail.append("%s: %d elements beyond their bound (worst %.2f x)" % (tag, int((err > bound).sum()), ratio))


def run_group(L, check, name, gid):
    probs, head, per = R.WG_GROUPS[gid]
    dt = R.ELEM[name][0]
    fail, fig = [], {}
    k = len(probs)
    dims = (C.c_int * (5 * k))(*[v for p in probs for v in p])
    out = (C.c_int * (4 + 3 * k))()
    check(L.vpd_op_wgrad_group_dispatch(k, dims, out), "wgrad_group_dispatch", name)
    got_head, got_per = tuple(out[:4]), [tuple(out[4 + 3 * i:7 + 3 * i]) for i in range(k)]
    disp = {"head": got_head, "per": got_per}
    if got_head != tuple(head) or got_per != [tuple(p) for p in per]:
        fail.append("group dispatch %r %r, the run expects %r %r" % (got_head, got_per, head, per))
    alone = [dispatch(L, conv_geometry(n, ci, co, h, w, 1), T3, 1) for (n, h, w, co, ci) in probs]
    for d in alone:
        expect(d, fail, "the problem alone", kernel="halo3x3", inst=head[0], stages=3)
    if fail:
        return {"fail": fail, "figures": fig, "dispatch": disp}
    arr = lambda v: (C.c_void_p * k)(*v)
    one_slab = torch.empty(L.vpd_op_wgrad_slab_bytes() // 4, dtype=torch.float32, device="cuda")
    for regime in ("int", "randn"):
        g = torch.Generator().manual_seed(seed_of(gid, regime))
        keep, refs, bounds = [], [], []
        for (n, h, w, co, ci) in probs:
            assert n * h * w < (1 << 24)
            cs = dict(ci=ci, co=co, k=3, stride=1, h=h, w=w)
            x, dz = R.wg_operands(n, ci, co, h, w, 1, regime, name, g)
            refs.append(R.conv_wgrad(x, dz, cs))
            bounds.append(R.wg_bound(x, dz, cs) if regime == "randn" else None)
            slab = torch.full((max(int(L.vpd_op_wgrad_group_slab_floats(co, ci)), 4),), SENT, dtype=torch.float32, device="cuda")
            keep.append((padded(x, dt), padded(dz, dt), new_dw(9 * co * ci), slab))
        check(L.vpd_op_wgrad_group(k, arr([t[1].data_ptr() for t in keep]), arr([t[0].data_ptr() for t in keep]),
                                   arr([t[2].data_ptr() for t in keep]), arr([t[3].data_ptr() for t in keep]), dims, stream()),
              "wgrad_group", name)
        torch.cuda.synchronize()
        for i, (n, h, w, co, ci) in enumerate(probs):
            m = 9 * co * ci
            tag = "%s/p%d" % (regime, i)
            buf = check_buffer(keep[i][2], m, tag, fail)
            compare(tag, buf.double().view(3, 3, co, ci).permute(2, 3, 0, 1), refs[i], bounds[i], fail, fig)
            if regime != "int":
                continue
            # the same problem alone through vpd_op_wgrad with a slab (conv_wgrad_halo_kernel): both routes are integer-exact
            rdw = new_dw(m)
            check(L.vpd_op_wgrad(ptr(keep[i][1]), ptr(keep[i][0]), ptr(rdw), *conv_geometry(n, ci, co, h, w, 1), T3, ptr(one_slab), stream()),
                  "wgrad", name)
            torch.cuda.synchronize()
            rbuf = check_buffer(rdw, m, tag + "/alone", fail)
            nd = int((rbuf.view(torch.int32) != buf.view(torch.int32)).sum())
            fig[tag + "/bits_differ_from_alone"] = nd
            if nd:
                fail.append("%s: %d elements differ in bits from the single launch" % (tag, nd))
    return {"fail": fail, "figures": fig, "dispatch": disp}


def stem_buffers(x, dz, dt):
    """the layout of tests/test_ops_gpu.py::test_stem_conv_and_wgrad"""
    from tests.test_ops_gpu import to_padded_nhwc
    n, c, h, w = x.shape
    x8 = torch.zeros(n, 8, h, w)
    x8[:, :c] = x.float()
    return to_padded_nhwc(x8, 3, 3, 3, 5, slack=256, dtype=dt), dz.permute(0, 2, 3, 1).contiguous().to(dt).cuda()


def run_stem(L, check, name, sid):
    dt = R.ELEM[name][0]
    fail, fig = [], {}
    refused = sid in R.WG_STEM_REFUSED
    n, h, w = R.WG_STEM_REFUSED[sid] if refused else R.WG_STEM[sid][0]
    ci, co = 5, 64
    geom = stem_geometry(n, h, w)
    d = dispatch(L, geom, TSTEM, 1)
    if refused:
        expect(d, fail, sid, kernel="atomics", inst=0)
    else:
        tr, ksplit, cpb = R.WG_STEM[sid][1]
        expect(d, fail, sid, kernel="stem", inst=4, stages=3, TR=tr, ksplit=ksplit, cpb=cpb, grid_x=1)
    if fail:
        return {"fail": fail, "figures": fig, "dispatch": d}
    cs = dict(ci=ci, co=co, k=7, stride=2, h=h, w=w)
    slab = torch.empty(L.vpd_op_wgrad_slab_bytes() // 4, dtype=torch.float32, device="cuda")
    m = 7 * 64 * 64
    for regime in ("int", "randn"):
        g = torch.Generator().manual_seed(seed_of(sid, regime))
        assert n * (h // 2) * (w // 2) < (1 << 24)
        x, dz = R.wg_operands(n, ci, co, h, w, 2, regime, name, g)
        xp, dzd = stem_buffers(x, dz, dt)
        dw = new_dw(m, 0.0 if refused else SENT)             # the atomics kernel adds onto zeros
        check(L.vpd_op_wgrad(ptr(dzd), ptr(xp), ptr(dw), *geom, TSTEM, ptr(slab), stream()), "wgrad", name)
        torch.cuda.synchronize()
        buf = check_buffer(dw, m, regime, fail, zeroed=refused)
        got = R.stem_wgrad_view(buf.double(), ci)
        compare(regime, got, R.conv_wgrad(x, dz, cs), R.wg_bound(x, dz, cs) if regime == "randn" else None, fail, fig)
    return {"fail": fail, "figures": fig, "dispatch": d}


def one_by_one_cases():
    from tests.test_ops_gpu import CONV_CASES
    return {c[0]: c[1:] for c in CONV_CASES if c[6] == 1}


# pass instantiation of the halo 1x1 route per case (stride 2: the 10-pass halo of a 16 x 16 / 8 x 8 output)
HALO_1X1_INST = {"l2_1x1_s2": 10, "b1_1x1_s1_256to64": 4, "b3_1x1_s1_128to512_ragged": 5, "ds_1x1_s2_32to16": 10,
                 "b_1x1_s1_512to128_t256": 5, "b_1x1_s1_1024to256_t128": 4}


def run_halo1x1(L, check, name, cid):
    n, ci, co, h, w, k, st, pad = one_by_one_cases()[cid]
    dt = R.ELEM[name][0]
    fail, fig = [], {}
    geom = conv_geometry(n, ci, co, h, w, st)
    d = dispatch(L, geom, T1, 1)
    expect(d, fail, cid, kernel="halo1x1", inst=HALO_1X1_INST[cid], stages=3)
    expect(dispatch(L, geom, T1, 0), fail, cid + " without a slab", kernel="atomics", inst=0)
    if fail:
        return {"fail": fail, "figures": fig, "dispatch": d}
    cs = dict(ci=ci, co=co, k=1, stride=st, h=h, w=w)
    slab = torch.empty(L.vpd_op_wgrad_slab_bytes() // 4, dtype=torch.float32, device="cuda")
    m = co * ci
    for regime in ("int", "randn"):
        g = torch.Generator().manual_seed(seed_of(cid, regime))
        assert n * (h // st) * (w // st) < (1 << 24)
        x, dz = R.wg_operands(n, ci, co, h, w, st, regime, name, g)
        dw, xp, dzp = new_dw(m), padded(x, dt), padded(dz, dt)
        check(L.vpd_op_wgrad(ptr(dzp), ptr(xp), ptr(dw), *geom, T1, ptr(slab), stream()), "wgrad", name)
        torch.cuda.synchronize()
        buf = check_buffer(dw, m, regime, fail)
        compare(regime, buf.double().view(co, ci, 1, 1), R.conv_wgrad(x, dz, cs), R.wg_bound(x, dz, cs) if regime == "randn" else None,
                fail, fig)
    return {"fail": fail, "figures": fig, "dispatch": d}


def main():
    name, mode = sys.argv[1], sys.argv[2]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from vpd_amd._lib import check, lib
    L = lib(name)
    assert L.vpd_elem_dtype().decode() == name
    out = {}
    if mode == "group":
        cases, run = list(R.WG_GROUPS), lambda c: run_group(L, check, name, c)
    elif mode == "stem":
        cases, run = list(R.WG_STEM) + list(R.WG_STEM_REFUSED), lambda c: run_stem(L, check, name, c)
    else:
        assert mode == "halo1x1" and os.environ.get("VPD_WGRAD_1X1") == "1"
        cases, run = list(one_by_one_cases()), lambda c: run_halo1x1(L, check, name, c)
    for c in cases:
        out[c] = run(c)
        print(c, name, json.dumps(out[c]["figures"]), flush=True)
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
