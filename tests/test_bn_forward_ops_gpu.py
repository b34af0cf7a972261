"""The train-mode BatchNorm forward one launch at a time, hook off, in both libraries, through the entry points only:
bn_fwd_fused_kernel<false> (vpd_op_bn_forward, vpd_op_bn_forward2), bn_finalize_kernel (vpd_op_bn_finalize) and the VPD_FUSED_BN=0
path's bn_apply_kernel (vpd_op_bn_apply), against the float64 closed forms of tests/opref_bn_fwd.py on the same element-rounded
operands and accumulator rows.  tests/test_bn_forward_cpu.py holds those closed forms equal to F.batch_norm(training=True), a
float32 transcription of the kernels inside the bounds, the planted faults outside them and every case on the path its id names.

Every launch: out, the bit map, the four vectors and rm / rv lie in buffers with slack on both sides, pre-filled with a sentinel; the
WHOLE padded output is looked at -- the interior per element against opref_bn_fwd.out_bound, all four sides of the border and the slack
for the sentinel's bits; the bit map equals mask_bits(stored value > 0); the rows come back bit for bit; a second identical launch
gives identical bits."""
import ctypes as C
import time

import pytest
import torch

from tests import opref as R
from tests import opref_bn_fwd as B
from tests.test_ops_gpu import ptr, stream

pytestmark = pytest.mark.gpu

NAMES = ["bf16", "fp16"]
F = C.c_float
SLACK = 64                      # elements / floats / bytes on either side of every output buffer
BYTE_SENTINEL = 0xA5
RES_BORDER = 9.0                # the residual's border: read in an interior pixel's place it is tens of bounds off
VEC = ("mean", "rstd", "scale", "shift")


def _lib(name):
    from vpd_amd._lib import lib
    return lib(name)


def _check(rc, name):
    from vpd_amd._lib import check
    check(rc, "op", name)


class Guarded:
    """a device buffer of `numel` values with SLACK sentinels on either side; .t is the part handed to the launch"""

    def __init__(self, numel, kind, name=None, init=None):
        if kind == "elem":
            full = R.sentinel_elems(numel + 2 * SLACK, name).cuda()
        elif kind == "f32":
            full = torch.full((numel + 2 * SLACK,), R.SENTINEL_F32, device="cuda")
        else:
            full = torch.full((numel + 2 * SLACK,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
        self.full, self.t, self.kind = full, full[SLACK:SLACK + numel], kind
        self.fill = full[0].clone()
        if init is not None:
            self.t.copy_(init)

    def untouched(self):
        return bool((R.bits(self.t) == R.bits(self.fill.view(1))).all()) if self.kind != "u8" else bool((self.t == BYTE_SENTINEL).all())

    def slack_intact(self):
        a, b = self.full[:SLACK], self.full[-SLACK:]
        if self.kind == "u8":
            return bool((a == BYTE_SENTINEL).all() and (b == BYTE_SENTINEL).all())
        f = R.bits(self.fill.view(1))
        return bool((R.bits(a) == f).all() and (R.bits(b) == f).all())


def _padded_res(res, name):
    n, h, w, c = res.shape
    buf = torch.full((n, h + 2, w + 2, c), RES_BORDER)
    buf[:, 1:-1, 1:-1] = res
    return buf.to(R.ELEM[name][0]).cuda()


def _side_buffers(s, name, running=True):
    c = s["gamma"].numel()
    dt = R.ELEM[name][0]
    d = dict(z=s["z"].to(dt).cuda(), rows=s["rows"].cuda(), gamma=s["gamma"].float().cuda(), beta=s["beta"].float().cuda())
    d["rows0"] = d["rows"].clone()
    for k in VEC:
        d[k] = Guarded(c, "f32")
    d["rm"] = Guarded(c, "f32", init=s["rm"].float().cuda()) if running else None
    d["rv"] = Guarded(c, "f32", init=s["rv"].float().cuda()) if running else None
    return d


def _side_args(d):
    run = [ptr(d["rm"].t), ptr(d["rv"].t)] if d["rm"] is not None else [None, None]
    return [ptr(d["z"]), ptr(d["rows"]), ptr(d["gamma"]), ptr(d["beta"])] + run + [ptr(d[k].t) for k in VEC]


def launch_fused(name, cs, running=True, want_bits=True):
    """one vpd_op_bn_forward / vpd_op_bn_forward2 launch on the case's operands; returns the device buffers"""
    L = _lib(name)
    n, h, w, c = cs["shape"]
    M = cs["M"]
    bufs = dict(a=_side_buffers(cs, name, running), b=_side_buffers(cs["b2"], name, running) if cs["b2"] else None)
    bufs["out"] = Guarded(n * (h + 2) * (w + 2) * c, "elem", name)
    bufs["bits"] = Guarded(M * c // 8, "u8")
    bufs["res"] = _padded_res(cs["res"], name) if cs["res"] is not None else None
    tail = [n, h, w, c, int(cs["relu"]), F(B.MOM), F(B.EPS), stream()]
    mb = ptr(bufs["bits"].t) if want_bits else None
    if cs["b2"]:
        rc = L.vpd_op_bn_forward2(*_side_args(bufs["a"]), *_side_args(bufs["b"]), ptr(bufs["out"].t), mb, *tail)
    else:
        rc = L.vpd_op_bn_forward(*_side_args(bufs["a"]), ptr(bufs["res"]) if bufs["res"] is not None else None, ptr(bufs["out"].t), mb, *tail)
    _check(rc, name)
    torch.cuda.synchronize()
    return bufs


def _device_parts(bufs):
    parts = [bufs["out"].full, bufs["bits"].full]
    for side in ("a", "b"):
        d = bufs[side]
        if d is not None:
            parts += [d[k].full for k in VEC] + [d[k].full for k in ("rm", "rv") if d[k] is not None]
    return parts


def same_bits(b1, b2):
    return all(torch.equal(R.bits(x) if x.dtype != torch.uint8 else x, R.bits(y) if y.dtype != torch.uint8 else y)
               for x, y in zip(_device_parts(b1), _device_parts(b2)))


def check_padded_output(guard, shape, name, want, bound, what):
    """the whole padded tensor: interior per element, border and slack in bits; returns (stored interior [M][C] float64, ratio)"""
    n, h, w, c = shape
    assert guard.slack_intact(), what + ": slack overwritten"
    o4 = guard.t.view(n, h + 2, w + 2, c)
    sent = R.bits(guard.fill.view(1))
    ob = R.bits(o4)
    for side, part in (("top", ob[:, 0]), ("bottom", ob[:, -1]), ("left", ob[:, :, 0]), ("right", ob[:, :, -1])):
        assert bool((part == sent).all()), "%s: %s border overwritten" % (what, side)
    got = o4[:, 1:-1, 1:-1].reshape(n * h * w, c).cpu().double()
    assert bool(torch.isfinite(got).all()), what + ": an interior element was not written"
    err = (got - want).abs_()
    ratio = float((err / bound).max())
    return got, ratio


def check_vectors(d, s, M, name, kind, rows, what, record):
    ref = s["ref"]
    run = d["rm"] is not None
    bnd = B.vector_bounds(ref, rows, M, s["gamma"], s["beta"], s["rm"] if run else None, s["rv"] if run else None, kind)
    for k in VEC + (("rm", "rv") if run else ()):
        assert d[k].slack_intact(), "%s: slack of %s overwritten" % (what, k)
        r = B.ratio(d[k].t.cpu(), ref[k], bnd[k])
        record[k] = max(record.get(k, 0.0), r)
        assert r <= 1.0, (what, k, r)


def verify_fused(name, cs, bufs, what):
    n, h, w, c = cs["shape"]
    M = cs["M"]
    record = {}
    got, ratio = check_padded_output(bufs["out"], cs["shape"], name, cs["out"], B.case_out_bound(cs), what)
    record["out"] = ratio
    print("\nRATIO", what, name, "out %.3f" % ratio, end=" ")
    assert ratio <= 1.0, (what, ratio)
    assert bufs["bits"].slack_intact()
    assert torch.equal(bufs["bits"].t.cpu().view(M, c // 8), R.mask_bits(got > 0)), what + ": bit map"
    for side, s in (("a", cs), ("b", cs["b2"])):
        if s is not None:
            assert torch.equal(bufs[side]["rows"], bufs[side]["rows0"]), what + ": the fused launch wrote its rows"
            check_vectors(bufs[side], s, M, name, "fused", s["rows"], what + "/" + side, record)
    print(" ".join("%s %.3f" % kv for kv in sorted(record.items()) if kv[0] != "out"))
    return got


# ---- the fused launch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("launch", B.LAUNCHES, ids=B.launch_id)
def test_fused_forward_per_element(launch, name):
    t0 = time.time()
    cid, relu, residual, second = launch
    cs = B.case(cid, name, bool(relu), bool(residual), bool(second))
    what = B.launch_id(launch)
    b1, b2 = launch_fused(name, cs), launch_fused(name, cs)
    assert same_bits(b1, b2), what + ": two identical launches differ"
    del b2
    got = verify_fused(name, cs, b1, what)
    if cs["planted"]:
        mu = b1["a"]["mean"].t.cpu()
        assert float(mu[B.CH_CONST]) == 0.75 and abs(float(mu[B.CH_CANCEL]) - 40.125) < 0.05
    if cs["planted"] and not residual and not second:      # (nothing is added to the planted channel's 1e-9)
        col = R.elem_round(got[:, B.CH_FLUSH].float(), name)
        if relu:      # gamma = 0, beta = +1e-9: fp16 stores +0 (bit 0), bf16 stores 1e-9 (bit 1)
            assert bool((col > 0).all()) == (name == "bf16") and bool((col == 0).all()) == (name == "fp16")
        else:         # beta = -1e-9, no ReLU: fp16 stores -0, bf16 a negative value: bit 0 either way
            assert not bool((col > 0).any()) and (name == "bf16" or bool(torch.signbit(col).all()))
    if second:      # side 0's vectors are what the single launch stores for the same rows
        one = launch_fused(name, dict(cs, b2=None), want_bits=False)
        for k in VEC + ("rm", "rv"):
            assert torch.equal(R.bits(one["a"][k].t), R.bits(b1["a"][k].t)), (what, k)
    print("\nTIME", what, name, "%.2f s" % (time.time() - t0))


@pytest.mark.parametrize("name", NAMES)
def test_null_running_statistics_and_null_bit_map(name):
    """rm / rv null: the vectors and out are written, nothing else; forward2 takes both sides' running statistics or neither"""
    cs = B.case("one_trip_3x9x7", name)
    bufs = launch_fused(name, cs, running=False, want_bits=False)
    verify_bits = bufs["bits"].untouched() and bufs["bits"].slack_intact()
    assert verify_bits, "a null bit map was written"
    full = launch_fused(name, cs)
    assert torch.equal(R.bits(bufs["out"].full), R.bits(full["out"].full))
    for k in VEC:
        assert torch.equal(R.bits(bufs["a"][k].full), R.bits(full["a"][k].full)), k
    two = B.case("one_trip_3x9x7", name, second=True)
    b = launch_fused(name, two, running=False)
    verify_fused(name, two, b, "two, no running statistics")
    # one, two or three of the four: refused, nothing launched
    L = _lib(name)
    n, h, w, c = two["shape"]
    for drop in ((0,), (1,), (2,), (3,), (0, 1), (2, 3), (0, 3), (1, 2, 3)):
        bb = dict(a=_side_buffers(two, name), b=_side_buffers(two["b2"], name))
        out, bits = Guarded(n * (h + 2) * (w + 2) * c, "elem", name), Guarded(two["M"] * c // 8, "u8")
        args = [_side_args(bb["a"]), _side_args(bb["b"])]
        for i in drop:
            args[i // 2][4 + i % 2] = None
        rc = L.vpd_op_bn_forward2(*args[0], *args[1], ptr(out.t), ptr(bits.t), n, h, w, c, 1, F(B.MOM), F(B.EPS), stream())
        torch.cuda.synchronize()
        assert rc != 0 and b"running statistics" in L.vpd_last_error(), drop
        assert out.untouched() and bits.untouched() and all(bb[s][k].untouched() for s in "ab" for k in VEC), drop


# ---- the finalize launch ---------------------------------------------------------------------------------------------------------
def _finalize_case(c, count, seed):
    """per-channel statistics -> sums over `count` values -> sixteen uneven rows; no tensor of that many values is needed"""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(c, generator=g).double() * 0.7      # (no fp32 value: the stored mean is rounded)
    var = (0.1 + 2.0 * torch.rand(c, generator=g)).double() if count > 1 else torch.zeros(c, dtype=torch.float64)
    rows = B.uneven_rows(mu * count, (var + mu * mu) * count, B.STAT_ROWS)
    gamma, beta = R.stem_params(c, "drift", g)
    rm, rv = 0.5 * torch.randn(c, generator=g), 0.25 + 1.75 * torch.rand(c, generator=g)
    S1, S2 = B.row_sums(rows)
    return dict(gamma=gamma, beta=beta, rm=rm, rv=rv, rows=rows, ref=B.closed_form(S1, S2, count, gamma, beta, rm, rv))


def _finalize_launch(name, s, count, running=True, drop=None):
    L = _lib(name)
    c = s["gamma"].numel()
    d = dict(rows=s["rows"].cuda(), gamma=s["gamma"].float().cuda(), beta=s["beta"].float().cuda())
    for k in VEC:
        d[k] = Guarded(c, "f32")
    d["rm"] = Guarded(c, "f32", init=s["rm"].float().cuda()) if running else None
    d["rv"] = Guarded(c, "f32", init=s["rv"].float().cuda()) if running else None
    run = [ptr(d["rm"].t), ptr(d["rv"].t)] if running else [None, None]
    if drop is not None:
        run[drop] = None
    rc = L.vpd_op_bn_finalize(ptr(d["rows"]), ptr(d["gamma"]), ptr(d["beta"]), *run, *[ptr(d[k].t) for k in VEC], count, c, F(B.MOM),
                              F(B.EPS), stream())
    torch.cuda.synchronize()
    return rc, d


@pytest.mark.parametrize("name", NAMES)
def test_finalize_launch(name):
    """bn_finalize_kernel: C in {8, 24, 100, 2048} (part of a wave, a ragged last block, 32 blocks) x count in {1, 189, 2^21 + 5}"""
    L = _lib(name)
    for c in (8, 24, 100, 2048):
        for count in (1, 189, 2 ** 21 + 5):
            s = _finalize_case(c, count, 7 * c + count % 1000)
            what = "finalize C %d count %d" % (c, count)
            rc, d = _finalize_launch(name, s, count)
            _check(rc, name)
            assert float(d["rows"].abs().max()) == 0.0, what + ": the rows are consumed"
            record = {}
            check_vectors(d, s, count, name, "finalize", s["rows"], what, record)
            print("\nRATIO", what, name, " ".join("%s %.3f" % kv for kv in sorted(record.items())))
    s = _finalize_case(24, 189, 5)
    rc, d = _finalize_launch(name, s, 189, running=False)
    _check(rc, name)
    check_vectors(d, s, 189, name, "finalize", s["rows"], "finalize, no running statistics", {})
    assert float(d["rows"].abs().max()) == 0.0
    for drop in (0, 1):
        rc, d = _finalize_launch(name, s, 189, drop=drop)
        assert rc != 0 and b"come together" in L.vpd_last_error()
        assert all(d[k].untouched() for k in VEC) and torch.equal(d["rows"].cpu(), s["rows"])
        assert torch.equal(d["rm"].t.cpu(), s["rm"].float()) and torch.equal(d["rv"].t.cpu(), s["rv"].float())


# ---- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bad_shapes_are_refused_before_anything_is_launched(name):
    L = _lib(name)
    cs = B.case("one_trip_3x9x7", name, second=True)
    n, h, w, c = cs["shape"]
    M = cs["M"]
    bb = dict(a=_side_buffers(cs, name), b=_side_buffers(cs["b2"], name))
    out, bits = Guarded(n * (h + 2) * (w + 2) * c, "elem", name), Guarded(M * c // 8, "u8")
    res = _padded_res(torch.zeros(n, h, w, c), name)

    def intact():
        torch.cuda.synchronize()
        ok = out.untouched() and bits.untouched() and all(bb[s][k].untouched() for s in "ab" for k in VEC)
        return ok and all(torch.equal(bb[s][k].t.cpu(), (cs if s == "a" else cs["b2"])[k].float()) for s in "ab" for k in ("rm", "rv"))

    for bad in ((0, h, w, c), (n, 0, w, c), (n, h, 0, c), (-1, h, w, c), (n, h, w, 0), (n, h, w, 4), (n, h, w, 60), (n, h, w, 4104),
                (n, h, w, 8192)):
        tail = list(bad) + [1, F(B.MOM), F(B.EPS), stream()]
        assert L.vpd_op_bn_forward(*_side_args(bb["a"]), None, ptr(out.t), ptr(bits.t), *tail) != 0 and b"bad shape" in L.vpd_last_error(), bad
        assert L.vpd_op_bn_forward(*_side_args(bb["a"]), ptr(res), ptr(out.t), ptr(bits.t), *tail) != 0, bad
        assert L.vpd_op_bn_forward2(*_side_args(bb["a"]), *_side_args(bb["b"]), ptr(out.t), ptr(bits.t), *tail) != 0 and \
            b"bad shape" in L.vpd_last_error(), bad
        z, sc, sh = ptr(bb["a"]["z"]), ptr(bb["a"]["gamma"]), ptr(bb["a"]["beta"])
        for kind in (0, 1, 2):
            assert L.vpd_op_bn_apply(z, sc, sh, ptr(res), sc, sh, kind, ptr(out.t), *bad, 1, stream()) != 0 and b"bad shape" in L.vpd_last_error()
        assert intact(), bad
    z, sc, sh = ptr(bb["a"]["z"]), ptr(bb["a"]["gamma"]), ptr(bb["a"]["beta"])
    for args, msg in (((None, sc, sh, None, None, None, 0, ptr(out.t)), b"null argument"), ((z, None, sh, None, None, None, 0, ptr(out.t)), b"null argument"),
                      ((z, sc, None, None, None, None, 0, ptr(out.t)), b"null argument"), ((z, sc, sh, None, None, None, 0, None), b"null argument"),
                      ((z, sc, sh, None, None, None, 1, ptr(out.t)), b"null argument"), ((z, sc, sh, ptr(res), None, sh, 2, ptr(out.t)), b"null argument"),
                      ((z, sc, sh, ptr(res), sc, None, 2, ptr(out.t)), b"null argument"), ((z, sc, sh, ptr(res), sc, sh, 3, ptr(out.t)), b"res_kind"),
                      ((z, sc, sh, ptr(res), sc, sh, -1, ptr(out.t)), b"res_kind")):
        assert L.vpd_op_bn_apply(*args, n, h, w, c, 1, stream()) != 0 and msg in L.vpd_last_error(), args[6]
    assert intact()
    # the largest width is accepted (test_fused_forward_per_element[wide_4096]); a null operand is not
    a = _side_args(bb["a"])
    for i in (0, 1, 2, 3, 6, 7, 8, 9):
        aa = list(a)
        aa[i] = None
        assert L.vpd_op_bn_forward(*aa, None, ptr(out.t), ptr(bits.t), n, h, w, c, 1, F(B.MOM), F(B.EPS), stream()) != 0 and \
            b"null argument" in L.vpd_last_error(), i
    assert L.vpd_op_bn_forward(*a, None, None, ptr(bits.t), n, h, w, c, 1, F(B.MOM), F(B.EPS), stream()) != 0
    assert intact()


# ---- the fallback's apply launch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("cid", ["one_trip_3x9x7", "generic_cv_3", "generic_cv_12", "generic_m"])
def test_apply_launch_of_the_unfused_path(cid, name):
    """bn_apply_kernel through vpd_op_bn_apply, res_kind 0 / 1 / 2, on the coefficient vectors a fused launch stored: per element
    against elem(relu(scale z + shift + ...)) formed in float64 from those fp32 vectors -- the finalize is not in play"""
    t0 = time.time()
    L = _lib(name)
    cs = B.case(cid, name, True, True, True)
    n, h, w, c = cs["shape"]
    M = cs["M"]
    if cid == "generic_m":
        geo = B.apply_geometry(M, c)
        assert geo["capped"] and geo["trips"] == 3
    src = launch_fused(name, dict(cs, res=None), want_bits=False)
    sc, sh, rsc, rsh = (src[s][k].t for s in "ab" for k in ("scale", "shift"))
    del src["out"]
    z2 = src["b"]["z"]
    resp = _padded_res(cs["res"], name)
    host = [t.cpu() for t in (sc, sh, rsc, rsh)]
    for kind in (0, 1, 2):
        what = "apply %s res_kind %d" % (cid, kind)
        res = cs["res"].view(M, c) if kind == 1 else None
        sec = (cs["b2"]["z"], host[2], host[3]) if kind == 2 else None
        ref, _ = B.apply_ref(cs["z"], host[0], host[1], 1, res, sec)
        bound = B.apply_bound(ref, name, cs["z"], host[0], host[1], res, sec)
        out = Guarded(n * (h + 2) * (w + 2) * c, "elem", name)
        rp = [None, ptr(resp), ptr(z2)][kind]
        _check(L.vpd_op_bn_apply(ptr(src["a"]["z"]), ptr(sc), ptr(sh), rp, ptr(rsc) if kind == 2 else None, ptr(rsh) if kind == 2 else None,
                                 kind, ptr(out.t), n, h, w, c, 1, stream()), name)
        torch.cuda.synchronize()
        _, ratio = check_padded_output(out, cs["shape"], name, ref, bound, what)
        print("\nRATIO", what, name, "out %.3f" % ratio)
        assert ratio <= 1.0, (what, ratio)
        del out, ref, bound
    # relu = 0 keeps the sign
    if cid == "one_trip_3x9x7":
        ref, _ = B.apply_ref(cs["z"], host[0], host[1], 0)
        out = Guarded(n * (h + 2) * (w + 2) * c, "elem", name)
        _check(L.vpd_op_bn_apply(ptr(src["a"]["z"]), ptr(sc), ptr(sh), None, None, None, 0, ptr(out.t), n, h, w, c, 0, stream()), name)
        torch.cuda.synchronize()
        got, ratio = check_padded_output(out, cs["shape"], name, ref, B.apply_bound(ref, name, cs["z"], host[0], host[1]), "apply, no ReLU")
        assert ratio <= 1.0 and bool((got < 0).any())
    print("\nTIME apply", cid, name, "%.2f s" % (time.time() - t0))
