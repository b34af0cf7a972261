"""What the references of the operator parity tests (tests/opref.py) rest on, checked without a GPU, so that a failure of
tests/test_stem_ops_gpu.py, test_bn_backward_ops_gpu.py, test_head_ops_gpu.py or test_conv_ops_gpu.py points at the kernel and not
at its reference."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import opref as R


@pytest.mark.parametrize("shape", [(9, 7), (8, 8), (5, 12), (1, 1), (2, 3)])
def test_torch_max_pool_keeps_the_first_maximum_on_ties_and_borders(shape):
    """tie-heavy planes (three distinct values) of odd and even sizes: torch's CPU max_pool2d indices, turned into window taps,
    equal a literal row-major scan that replaces the maximum on `>` only"""
    H, W = shape
    g = torch.Generator().manual_seed(H * 31 + W)
    for dtype in (torch.float64, torch.float32):
        total = 0
        for _ in range(6):
            a = torch.randint(0, 3, (H, W), generator=g).to(dtype) * 0.5
            p, fi = F.max_pool2d(a.view(1, 1, H, W), 3, 2, 1, return_indices=True)
            val, tap = R.first_max_loop(a)
            assert torch.equal(p[0, 0], val)
            assert torch.equal(R.taps_from_flat(fi, W)[0, 0], tap)
            total += tap.numel()
        assert total > 0


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_grid_inputs_are_exact_and_representable(name):
    z, scale, shift = R.stem_grid_inputs(4, 33, 31, 64, 5)
    dt = R.ELEM[name][0]
    assert torch.equal(z.to(dt).float(), z)                                   # z = k/16 is an element-type value
    v = lambda t: t.view(1, -1, 1, 1)
    a32 = z * v(scale) + v(shift)                                             # two fp32 roundings
    a64 = z.double() * v(scale).double() + v(shift).double()
    assert torch.equal(a32.double(), a64)                                     # ... that round nothing
    assert torch.equal(torch.addcmul(v(shift).expand_as(z), z, v(scale).expand_as(z)).double(), a64)
    assert torch.equal(a32.clamp_min(0).to(dt).double(), a64.clamp_min(0).to(dt).double())
    # ties are the rule: the activations fall on a few hundred distinct values and half of them are zero
    r = a64.clamp_min(0).to(dt)
    assert 0.3 < float((r == 0).double().mean()) < 0.7
    assert r.unique().numel() < 1000
    p, taps, _ = R.stem_forward_ref(z, scale, shift, name)
    assert int(taps.min()) >= 0 and int(taps.max()) <= 8
    # every tap value occurs: first-maximum ties reach all nine positions
    assert set(taps.unique().tolist()) == set(range(9))


def test_ulp_is_the_spacing_of_the_element_type():
    for name, (dt, p, emin) in R.ELEM.items():
        x = torch.tensor([1.0, 1.5, 0.75, 3.0, 100.0, 2.0 ** -10], dtype=torch.float64)
        nxt = (x.to(dt).view(torch.int16) + 1).view(dt).double()
        assert torch.equal(R.ulp(x, name), nxt - x), name
    assert float(R.ulp(torch.tensor([1e-9]), "fp16")) == 2.0 ** -24            # fp16's subnormal spacing
    assert R.dz_l2_gate("bf16") == 3e-3 and R.dz_l2_gate("fp16") == 3e-3 / 8


def _stem_cases():
    return [(key, regime, name) for key in R.STEM_BWD_SHAPES for regime in R.REGIMES for name in R.ELEM]


@pytest.mark.parametrize("key,regime,name", _stem_cases(), ids=["%s-%s-%s" % c for c in _stem_cases()])
def test_stem_backward_references_agree_and_the_band_is_empty_enough(key, regime, name):
    """reference A (autograd) == reference B (closed form) routed by torch's own arg-max, to 1e-12; the share of elements whose
    ReLU mask an fp32 evaluation could flip stays below its cap for every seeded case of the GPU test"""
    n, H, W = R.STEM_BWD_SHAPES[key]
    inp = R.stem_random_inputs(n, H, W, R.STEM_C, 5 * n + W, name, regime)
    dpool = R.stem_dpool(inp, name)
    dzA, dgA, dbA, taps = R.stem_backward_ref_A(inp["z"], inp["gamma"], inp["beta"], dpool)
    B = R.stem_backward_ref_B(inp["z"], inp["gamma"], inp["beta"], inp["mean"], inp["rstd"], dpool, taps)
    scale = float(dzA.abs().max())
    assert float((B["dz"] - dzA).abs().max()) <= 1e-12 * max(scale, 1.0)
    assert float((B["dgamma"] - dgA).abs().max()) <= 1e-12 * float(B["abs2"].max())
    assert float((B["dbeta"] - dbA).abs().max()) <= 1e-12 * float(B["abs1"].max())
    band = R.relu_band(inp["z"], inp["scale"], inp["shift"], B["a"])
    assert float(band.double().mean()) <= R.BAND_CAP
    # the mean(g xhat) term carries weight: a 2 % error in it is visible at the gate
    off = R.bn_dz_closed_form(inp["z"], inp["gamma"], inp["mean"], inp["rstd"], B["g"], 1.02)
    if regime == "init":
        assert R.rel_l2(off, B["dz"]) > 2 * R.dz_l2_gate("bf16")


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_dz_bound_accepts_an_fp32_evaluation_and_rejects_a_two_per_cent_error(name):
    """the per-element bound of the GPU tests on a stand-in for the kernel: the closed form evaluated in fp32 from fp32 statistics
    and sums, rounded to the element type, passes; the reference with its xhat coefficient 2 % off does not"""
    n, H, W = R.STEM_BWD_SHAPES["g32"]
    inp = R.stem_random_inputs(n, H, W, R.STEM_C, 5 * n + W, name, "init")
    dpool = R.stem_dpool(inp, name)
    _, taps, _ = R.stem_forward_ref(inp["z"], inp["scale"], inp["shift"], name)
    B = R.stem_backward_ref_B(inp["z"], inp["gamma"], inp["beta"], inp["mean"], inp["rstd"], dpool, taps)
    M = n * H * W
    v = lambda t: t.float().view(1, -1, 1, 1)
    g = B["g"].float()
    xh = (inp["z"] - v(inp["mean"])) * v(inp["rstd"])
    c1 = v(inp["gamma"]) * v(inp["rstd"])
    c2, c3 = v(B["dbeta"] / M), v(B["dgamma"] / M)
    got = R.elem_round(c1 * (g - c2 - xh * c3), name).double()
    ds1, ds2 = R.SUM_TOL * B["abs1"], R.SUM_TOL * B["abs2"]
    bound = R.bn_dz_bound(B["dz"], inp["gamma"], inp["rstd"], inp["mean"], inp["z"], B["g"], B["xhat"], B["dbeta"], B["dgamma"],
                          ds1, ds2, M, name)
    assert int(((got - B["dz"]).abs() > bound).sum()) == 0
    assert R.rel_l2(got, B["dz"]) < R.dz_l2_gate(name)
    off = R.bn_dz_closed_form(inp["z"], inp["gamma"], inp["mean"], inp["rstd"], B["g"], 1.02)
    assert int(((got - off).abs() > bound).sum()) > 0 and R.rel_l2(got, off) > R.dz_l2_gate(name)


def test_bn_backward_case_closed_form_matches_autograd():
    for relu, residual in ((True, False), (True, True), (False, False)):
        cs = R.bn_backward_case(3, 8, 8, 64, 11, "bf16", relu=relu, residual=residual)
        gm = cs["dy"].double() * cs["mask"]
        dz = R.bn_dz_closed_form(cs["z"], cs["gamma"], cs["mean"], cs["rstd"], gm)
        assert float((dz - cs["dz"]).abs().max()) <= 1e-12 * float(cs["dz"].abs().max())
        assert R.rel_l2(R.bn_dz_closed_form(cs["z"], cs["gamma"], cs["mean"], cs["rstd"], gm, 1.02), cs["dz"]) > 2 * 3e-3


def test_integer_head_inputs_sum_exactly_in_fp32():
    g = torch.Generator().manual_seed(1)
    for case in R.sgemm_cases():
        _, M, N, K, ta, tb, bias, relu = case
        assert 49 * K + 64 < 2 ** 24
    # the sums of |products| actually drawn stay below 2^24 as well (every partial sum is then an exactly representable integer)
    for case in R.sgemm_cases()[::7]:
        A, B, bv = R.sgemm_operands(case, g, True)
        worst = float((A.abs().double() @ B.abs().double()).max()) + (float(bv.abs().max()) if bv is not None else 0.0)
        assert worst < 2 ** 24
        assert torch.equal(A, A.round()) and torch.equal(B, B.round())
    for n in R.MSE_SIZES:
        e, t = R.mse_int_operands(n, g)
        d = (e - t).double()
        assert float(d.abs().max()) <= 6 and 2 * float((d * d).sum()) < 2 ** 24
        assert float(e.abs().max()) < 2 ** 24 and torch.equal(e, e.round())
    assert len({c[0] for c in R.sgemm_cases()}) == len(R.sgemm_cases())


def test_float_reciprocal_division_is_exact_below_2_pow_21():
    """vpd_fdiv(m, 1/d) = int((m + 0.5) * fl(1/d)) in fp32 equals m // d for every m < 2^21 (the fast path's limit) and every
    divisor the stem shapes of the GPU test produce, plus a few large ones"""
    divs = set()
    for n, H, W in list(R.STEM_FWD_SHAPES.values()) + list(R.STEM_BWD_SHAPES.values()) + [R.STEM_BIG]:
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        divs |= {Wo // 2, Ho, H // 2, W // 2, Ho * Wo, Wo}
    divs |= {1, 3, 599, 1024, 4096, 65535, 2 ** 20 + 1}
    m = np.arange(2 ** 21, dtype=np.int64)
    mf = m.astype(np.float32) + np.float32(0.5)
    for d in sorted(x for x in divs if x >= 1):
        rcp = np.float32(1.0) / np.float32(d)
        q = (mf * rcp).astype(np.int64)                      # fp32 product, truncated
        assert np.array_equal(q, m // d), d


# ---------------------------------------------------------------------------
# convolution family
# ---------------------------------------------------------------------------
CONV_IDS = list(R.CONV_CASES)


def _tile_px(cs):
    return 256 if cs["blk_px"] % 256 == 0 else 128


@pytest.mark.parametrize("case", CONV_IDS)
@pytest.mark.parametrize("seed", R.CONV_SEEDS)
def test_conv_integer_regime_is_exact_and_representable_and_sees_the_four_faults(case, seed):
    """From the reference alone, no element left out: every operand is a bf16 and an fp16 value; every result of every operation the
    GPU test runs (forward, the four eval epilogues, data gradient, accumulate, masked accumulate) has magnitude <= 2^8 (bf16's
    integers; fp16's reach 2^11); every fp32 partial sum stays below 2^24 -- a convolution's by the sum of |products|, a block's
    statistics by (pixels it accumulates) x max^2, the BatchNorm sums by x max x |z|, a weight gradient's by the pixel count.
    And each of the four altered references differs from the right one."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cs = R.CONV_CASES[case]
    o = R.conv_operands(cs, seed, "int")
    for key in ("x", "w", "dz", "res", "old_y", "old_dx", "z", "z2", "scale", "shift"):
        for name in ("bf16", "fp16"):
            assert torch.equal(R.elem_round(o[key].float(), name).double(), o[key]), (key, name)
    cap = 2.0 ** R.ELEM["bf16"][1]
    conv, dx = R.conv_fwd(o["x"], o["w"], cs), R.conv_dgrad(o["dz"], o["w"], cs)
    # (operands in {-1, 0, 1}: the sum of |products| of a convolution is at most its K)
    assert max(float(o[k].abs().max()) for k in ("x", "w", "dz")) == 1.0 and cs["k"] ** 2 * max(cs["ci"], cs["co"]) < 2 ** 24
    results = {"fwd": conv, "dgrad": dx, "acc": dx + o["old_dx"], "macc": dx + o["old_dx"] * o["keep_dx"]}
    for res in (0, 1):
        for relu in (0, 1):
            results["ep%d%d" % (res, relu)] = R.conv_eval_ep(conv, o, res, relu)
    pre = R.conv_eval_ep(conv, o, 1, 0)
    for key, t in results.items():
        assert float(t.abs().max()) <= cap, (key, float(t.abs().max()))
        assert torch.equal(t, t.round())
    fmax, dmax = float(conv.abs().max()), float(results["acc"].abs().max())
    assert cs["blk_px"] * fmax * fmax < 2.0 ** 24                       # per-block sum of squares of the forward statistics
    assert cs["blk_px"] * dmax * R.CONV_ZMAX < 2.0 ** 24                # per-block sum g z of the BatchNorm sums
    assert cs["n"] * conv.shape[2] * conv.shape[3] < 2 ** 24            # weight gradient: at most one unit per output pixel
    # the four faults, each visible to equality
    assert not torch.equal(R.conv_alter_tap(conv, o["x"], o["w"], cs), conv)
    assert not torch.equal(R.conv_alter_chunks(conv, o["x"], o["w"], cs), conv)
    assert not torch.equal(R.conv_alter_tile(conv, _tile_px(cs)), conv)
    assert not torch.equal(R.conv_alter_tile(dx, _tile_px(cs)), dx)
    assert not torch.equal(R.conv_alter_shift(pre - o["res"], o["res"]), pre)
    assert not torch.equal(R.conv_alter_shift(dx, o["old_dx"]), results["acc"])
    assert not torch.equal(R.conv_alter_shift(dx, o["old_dx"] * o["keep_dx"]), results["macc"])
    assert not torch.equal(dx + o["old_dx"] * torch.roll(o["keep_dx"], 1, dims=3), results["macc"])


@pytest.mark.parametrize("case", CONV_IDS)
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_conv_random_regime_bound_rejects_the_four_faults(case, name):
    """The per-element bound of the randn regime accepts the reference evaluated in fp32 (what a correct kernel may do) and puts each
    altered reference outside it in at least one element: a tap left out for one image row, two weight chunks swapped, the
    residual one pixel off, one tile's pixels taken from the next image; on the data-gradient side a tile from the next image and the
    old value / the ReLU bit map of the accumulate modes one pixel off."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cs = R.CONV_CASES[case]
    o = R.conv_operands(cs, R.CONV_SEEDS[0], "rand", name)
    K = cs["k"] ** 2 * cs["ci"]
    conv = R.conv_fwd(o["x"], o["w"], cs)
    gamma = R.conv_gamma(R.conv_fwd(o["x"].abs(), o["w"].abs(), cs), K)
    bound = R.conv_bound(conv, gamma, name)
    stored32 = R.elem_round(F.conv2d(o["x"].float(), o["w"].float(), None, stride=cs["stride"], padding=cs["k"] // 2), name).double()
    assert bool(((stored32 - conv).abs() <= bound).all())
    outside = lambda alt, ref, b: bool(((alt - ref).abs() > b).any())
    assert outside(R.conv_alter_tap(conv, o["x"], o["w"], cs), conv, bound)
    assert outside(R.conv_alter_chunks(conv, o["x"], o["w"], cs), conv, bound)
    assert outside(R.conv_alter_tile(conv, _tile_px(cs)), conv, bound)
    v = lambda t: t.double().view(1, -1, 1, 1)
    pre = R.conv_eval_ep(conv, o, 1, 0)
    extra = 4 * 2.0 ** -24 * ((conv * v(o["scale"])).abs() + v(o["shift"]).abs() + o["res"].abs())
    assert outside(R.conv_alter_shift(pre - o["res"], o["res"]), pre, R.conv_bound(pre, gamma * v(o["scale"]).abs(), name, extra))
    if cs.get("stem"):
        return
    # data-gradient side: a tile from the next image, the old value and the ReLU bit map one pixel off
    dx = R.conv_dgrad(o["dz"], o["w"], cs)
    dgamma = R.conv_gamma(R.conv_dgrad(o["dz"].abs(), o["w"].abs(), cs), cs["k"] ** 2 * cs["co"])
    assert outside(R.conv_alter_tile(dx, _tile_px(cs)), dx, R.conv_bound(dx, dgamma, name))
    acc, macc = dx + o["old_dx"], dx + o["old_dx"] * o["keep_dx"]
    extra = 2 * 2.0 ** -24 * (dx.abs() + o["old_dx"].abs())
    assert outside(R.conv_alter_shift(dx, o["old_dx"]), acc, R.conv_bound(acc, dgamma, name, extra))
    assert outside(dx + o["old_dx"] * torch.roll(o["keep_dx"], 1, dims=3), macc, R.conv_bound(macc, dgamma, name, extra))


def test_conv_runs_dispatch_to_the_kernels_their_ids_name():
    """vpd_op_conv2d_dispatch is host-only; without a device the launcher assumes 256 CUs, an MI355X's count: every run of the GPU
    test must already dispatch as its id says here.  One child per switch setting (the switches are read once per process)."""
    from tests.conv_ops_child import RUNS
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    by_env = {}
    for run, (_, env, _, _) in RUNS.items():
        by_env.setdefault(json.dumps(env, sort_keys=True), []).append(run)
    seen = set()
    for env, runs in by_env.items():
        r = subprocess.run([sys.executable, os.path.join(repo, "tests", "conv_ops_child.py"), ",".join(runs), "dispatch"],
                           env=dict(os.environ, **json.loads(env)), capture_output=True, text=True, timeout=300, cwd=repo)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        for ln in r.stdout.splitlines():
            if ln.startswith("RESULT "):
                out = json.loads(ln[len("RESULT "):])
                assert not out["fail"], (out["run"], out["fail"])
                seen.add(out["run"])
    assert seen == set(RUNS)
    # every 3x3 class in both forms, the geometry instantiations of all three widths, the gather family's tiles
    forms = {(e["kclass"], e.get("pws"), e.get("geo")) for _, _, e, _ in RUNS.values()}
    assert {(1, 0, None), (1, 1, 0), (2, 1, 0), (2, 0, None), (3, 1, 4), (3, 1, 0), (3, 0, None), (6, 1, 16), (6, 1, 8), (6, 1, 0),
            (6, 0, None)} <= forms
    assert {(d["bm"], d["bn"]) for _, _, _, d in RUNS.values() if d and d.get("ws1x1") == 0 and "bm" in d} == {(128, 128), (64, 64), (128, 64)}


# ---------------------------------------------------------------------------
# the fused Bottleneck tail (conv1x1_bn_stream_kernel, conv1x1_bn2_stream_kernel)
# ---------------------------------------------------------------------------
TAIL_IDS = list(R.TAIL_CASES)


def test_tail_chain_is_batch_norm_and_its_autograd():
    """the float64 chain of the tail references -- statistics from the two sums, running statistics, the kernel's A g + B z + D form of
    dz, dgamma = (sum g z - mean sum g) rstd -- equals torch's batch_norm and its autograd to 1e-12, residual and ReLU included"""
    cs = dict(R.TAIL_CASES["k64_w8"], n=5)
    o = R.tail_operands(cs, 3, "rand", "bf16")
    z = R.tail_conv(o["x"], o["w"], "bf16")
    fw = R.tail_forward(cs, o, z, None, False, "bf16")
    rm, rv = o["rm"].double().clone(), o["rv"].double().clone()
    zt, gt, bt = z.clone().requires_grad_(True), o["gamma"].double().requires_grad_(True), o["beta"].double().requires_grad_(True)
    y = F.batch_norm(zt, rm, rv, gt, bt, training=True, momentum=R.BN_MOMENTUM, eps=R.BN_EPS) + o["res"]
    (y.clamp_min(0) * o["dout"]).sum().backward()
    st = fw["st"]
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(fw["pre"], y.detach()) and close(st["rm"], rm) and close(st["rv"], rv)
    bw = R.tail_backward(cs, o, z, None, fw, y.detach() > 0, "bf16")
    assert close(bw["b"]["dz"], zt.grad) and close(bw["b"]["dgamma"], gt.grad) and close(bw["b"]["dbeta"], bt.grad)
    assert close(bw["b"]["dz"], R.bn_dz_closed_form(z, o["gamma"], st["mean"], st["rstd"], bw["gm"]))
    assert torch.equal(R.tail_alter_coef(256)[:32], torch.tensor(list(range(8)) + [24, 25, 26, 27] + list(range(12, 32))))


def _tail_faults(cs, o, z, z2, fw, mask, name, regime):
    """{fault: [(altered, right, bound or None = equality), ...]} over every output the GPU test compares"""
    exact = regime == "int"
    ring, zname = R.tail_ring(cs), (None if exact else name)
    bw = R.tail_backward(cs, o, z, z2, fw, mask, name)
    rows = lambda st: torch.stack([st["s1"], st["s2"]])
    rows_tol = lambda st: None if exact else R.SUM_TOL * torch.stack([st["abs1"], st["s2"]])
    brows = lambda b: torch.stack([b["r1"], b["r2"]])
    brows_tol = lambda b: None if exact else R.SUM_TOL * torch.stack([b["abs1"], b["absz"]])

    def everything(fz, fz2, idx=None, res=None, fmask=None, dout=None):
        """a faulted launch sequence against the right one: the statistics rows come from the faulted z, the element-wise passes
        apply the RIGHT coefficients (each pass is a launch of its own) to the faulted operands"""
        f = dict(fw)
        pre = R.tail_pre(fz, fw["st"], idx) + (R.tail_pre(fz2, fw["st2"], idx) if cs["two"] else (o["res"] if res is None else res))
        pairs = [(pre.clamp_min(0), fw["out"], fw["bound"])]
        fst = R.tail_stats(fz, o["gamma"], o["beta"], o["rm"], o["rv"])
        pairs.append((rows(fst), rows(fw["st"]), rows_tol(fw["st"])))
        gm = (o["dout"] if dout is None else dout) * (mask if fmask is None else fmask)
        sides = [(fz, z, fw["st"], bw["b"], bw["bound"])] + ([(fz2, z2, fw["st2"], bw["b2"], bw["bound2"])] if cs["two"] else [])
        for a, right, st, b, bound in sides:
            fb = R.tail_bwd(a, st, gm, None)
            pairs.append((brows(fb), brows(b), brows_tol(b)))
            # mode 3 applies the coefficients of the RIGHT sums to the faulted operands
            A = st["gamma"] * st["rstd"]
            B = -A * st["rstd"] * b["dgamma"] / st["M"]
            D = -A * b["r1"] / st["M"] - B * st["mean"]
            if idx is not None:
                A, B, D = A[idx], B[idx], D[idx]
            v = lambda t: t.view(1, -1, 1, 1)
            pairs.append((v(A) * gm + v(B) * a + v(D), b["dz"], bound))
        return pairs

    fz, fz2 = R.tail_alter_tile(z, R.TAIL_LANES, ring), (R.tail_alter_tile(z2, R.TAIL_LANES, ring) if cs["two"] else None)
    cz, cz2 = R.tail_alter_chunks(cs, o, zname)
    faults = {"tile": everything(fz, fz2), "chunks": everything(cz, cz2), "coef": everything(z, z2, idx=R.tail_alter_coef(cs["co"])),
              "mask": everything(z, z2, fmask=R.tail_alter_mask(mask)), "dout": everything(z, z2, dout=torch.roll(o["dout"], 1, dims=3))}
    if not cs["two"]:
        faults["res"] = everything(z, z2, res=torch.roll(o["res"], 1, dims=3))
    # what each fault must show in: a stale tile and swapped chunks everywhere, coefficients in out and dz, the bit map and d(out) in
    # the backward sums and dz, the residual in out
    nside = 2 if cs["two"] else 1
    fwd, stat = [0], [1]
    bsum, dz = [2 + 2 * i for i in range(nside)], [3 + 2 * i for i in range(nside)]
    where = {"tile": fwd + stat + bsum + dz, "chunks": fwd + stat + bsum + dz, "coef": fwd + dz, "mask": bsum + dz, "dout": bsum + dz, "res": fwd}
    return faults, where


def _outside(alt, ref, bound):
    return (not torch.equal(alt, ref)) if bound is None else bool(((alt - ref).abs() > bound).any())


@pytest.mark.parametrize("case", TAIL_IDS)
def test_tail_integer_regime_is_exact_and_sees_the_five_faults(case):
    """Integer operands: x, w, residual and d(out) are bf16 and fp16 values, |z| <= 2^8, so z is the exact convolution in either
    library; every statistics row (sum z, sum z^2, sum g, sum g z -- sums of magnitudes taken) is an integer below 2^24 and must be
    EQUAL.  Each fault changes a row, or puts out / dz outside its bound, in every output it can reach."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cs = R.TAIL_CASES[case]
    o = R.tail_operands(cs, R.CONV_SEEDS[0], "int")
    for key in ("x", "w", "x2", "w2", "res", "dout"):
        if key in o:
            for name in ("bf16", "fp16"):
                assert torch.equal(R.elem_round(o[key].float(), name).double(), o[key]), (key, name)
    z = R.tail_conv(o["x"], o["w"])
    z2 = R.tail_conv(o["x2"], o["w2"]) if cs["two"] else None
    for t in (z, z2) if cs["two"] else (z,):
        assert float(t.abs().max()) <= 2.0 ** R.ELEM["bf16"][1] and torch.equal(t, t.round())
        assert float((t * t).sum(dim=(0, 2, 3)).max()) < 2.0 ** 24
        assert float((o["dout"].abs() * t.abs()).sum(dim=(0, 2, 3)).max()) < 2.0 ** 24
    fw = R.tail_forward(cs, o, z, z2, True, "bf16")
    own = R.tail_stored_mask(fw["out"], "bf16")
    assert 0.2 < float(own.double().mean()) < 0.8
    for mask in (o["keep"], own) if cs["few"] else (own,):          # (the whole-device cases: the same kernels, one map)
        faults, where = _tail_faults(cs, o, z, z2, fw, mask, "bf16", "int")
        for fault, pairs in faults.items():
            for i in where[fault]:
                assert _outside(*pairs[i]), (fault, i)


@pytest.mark.parametrize("case", TAIL_IDS)
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_tail_random_regime_bounds_accept_fp32_and_reject_the_five_faults(case, name):
    """randn operands, z rounded to the element type (on the GPU: the unfused launch's stored z).  The bounds accept a stand-in for
    the kernels -- fp32 coefficients from the float64 sums, fp32 element arithmetic, rounded to the element type -- and put every
    faulted reference outside in at least one element of every output the fault can reach."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cs = R.TAIL_CASES[case]
    o = R.tail_operands(cs, R.CONV_SEEDS[0], "rand", name)
    z = R.tail_conv(o["x"], o["w"], name)
    z2 = R.tail_conv(o["x2"], o["w2"], name) if cs["two"] else None
    fw = R.tail_forward(cs, o, z, z2, False, name)
    f32 = lambda t: t.float().view(1, -1, 1, 1)

    def pre32(zz, st, sfx):
        sc = o["gamma" + sfx].float() * (st["var"] + R.BN_EPS).float().rsqrt()
        return zz.float() * f32(sc) + f32(o["beta" + sfx].float() - st["mean"].float() * sc)
    v32 = pre32(z, fw["st"], "") + (pre32(z2, fw["st2"], "2") if cs["two"] else o["res"].float())
    got = R.elem_round(v32.clamp_min(0), name).double()
    assert bool(((got - fw["out"]).abs() <= fw["bound"]).all())
    mask = R.tail_stored_mask(fw["out"], name)
    bw = R.tail_backward(cs, o, z, z2, fw, mask, name)
    for zz, st, b, bound in [(z, fw["st"], bw["b"], bw["bound"])] + ([(z2, fw["st2"], bw["b2"], bw["bound2"])] if cs["two"] else []):
        A = (st["gamma"] * st["rstd"].float().double())
        B = -A * st["rstd"].float().double() * b["dgamma"] / st["M"]
        D = -A * b["r1"] / st["M"] - B * st["mean"].float().double()
        dz32 = f32(A) * bw["gm"].float() + (f32(B) * zz.float() + f32(D))
        assert bool(((R.elem_round(dz32, name).double() - b["dz"]).abs() <= bound).all())
    for mk in (o["keep"], mask) if cs["few"] else (mask,):
        faults, where = _tail_faults(cs, o, z, z2, fw, mk, name, "rand")
        for fault, pairs in faults.items():
            for i in where[fault]:
                assert _outside(*pairs[i]), (fault, i)


# ---------------------------------------------------------------------------
# the reference boundary (tests/test_boundary_ops_gpu.py)
# ---------------------------------------------------------------------------
def _pack_input_shapes():
    return (R.PACK_INPUT_ROWS + R.PACK_INPUT_ROWS_FALLBACK + R.PACK_INPUT_QUAD + R.PACK_INPUT_PIXEL + R.PACK_INPUT_MISALIGNED +
            (R.PACK_INPUT_BELOW, R.PACK_INPUT_WORKLOAD, R.PACK_INPUT_ABOVE))


def test_pack_input_cases_take_the_routes_they_are_named_for():
    """the launcher's conditions (vpd_launch_pack_input) restated on the case tables, and the item counts around 2^21"""
    for n, H, W in R.PACK_INPUT_ROWS + (R.PACK_INPUT_WORKLOAD,):
        assert W % 64 == 0 and (H * W) % 256 == 0
    for n, H, W in R.PACK_INPUT_ROWS_FALLBACK:
        assert W % 64 == 0 and (H * W) % 256 != 0
    for n, H, W in R.PACK_INPUT_QUAD + (R.PACK_INPUT_BELOW, R.PACK_INPUT_ABOVE):
        assert W % 4 == 0 and W % 64 != 0
    for n, H, W in R.PACK_INPUT_PIXEL:
        assert W % 4 != 0
    items = lambda s: s[0] * s[1] * s[2] // 4
    assert items(R.PACK_INPUT_BELOW) < R.FDIV_MAX <= items(R.PACK_INPUT_WORKLOAD) and R.PACK_INPUT_BELOW[2] // 4 == 7
    assert R.FDIV_MAX - items(R.PACK_INPUT_BELOW) < 64                     # the last items of the fast path are reached
    assert items(R.PACK_INPUT_ABOVE) >= R.FDIV_MAX


def test_float_reciprocal_division_is_exact_for_the_pack_input_divisors():
    """vpd_fdiv in numpy float32: int((m + 0.5f) * (1.0f / d)) == m // d for every m < 2^21, for d = 1 .. 128 and every divisor
    (W / 4 and H) of the quad-kernel cases -- so the 64-bit path is needed from 2^21 items on, and only there"""
    divs = set(range(1, 129))
    for n, H, W in _pack_input_shapes():
        divs |= {H, max(W // 4, 1)}
    m = np.arange(R.FDIV_MAX, dtype=np.int64)
    mf = m.astype(np.float32) + np.float32(0.5)
    for d in sorted(divs):
        q = (mf * (np.float32(1.0) / np.float32(d))).astype(np.int64)
        assert np.array_equal(q, m // d), d


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_pack_input_reference_is_a_literal_loop_and_sees_a_channel_left_unzeroed(name):
    g = torch.Generator().manual_seed(3)
    dt = R.ELEM[name][0]
    x = R.pack_input_values((2, 5, 3, 6), name, g)
    out, written = R.pack_input_ref(x, 3 + 6, 6 + 8, 3, name)
    for b in range(2):
        for yy in range(9):
            for xx in range(14):
                inside = 3 <= yy < 6 and 3 <= xx < 9
                assert bool(written[b, yy, xx]) == inside
                for c in range(8):
                    want = x[b, c, yy - 3, xx - 3].to(dt) if inside and c < 5 else torch.zeros((), dtype=dt)
                    assert int(R.bits(out[b, yy, xx, c].view(1))[0]) == int(R.bits(want.view(1))[0])
    # the inputs hold what they promise: ties, both zeros, element-type subnormals, fp16 overflow to inf as torch rounds it
    big = R.pack_input_values((1 << 16,), name, g)
    e = big.to(dt)
    assert bool((R.bits(big) == 0).any()) and bool((R.bits(big) == -2 ** 31).any())      # +0 and -0
    assert bool(((big != 0) & (big.abs() < 2.0 ** (R.ELEM[name][2] + R.ELEM[name][1] - 1))).any())
    assert bool(torch.isinf(e).any()) and not bool(torch.isnan(e).any())
    assert float(torch.tensor(65519.0).to(torch.float16)) == 65504.0 and bool(torch.isinf(torch.tensor(65520.0).to(torch.float16)))
    assert not bool((R.bits(e) == R.SENTINEL_BITS[name]).any())
    # resolution: channel 5 of the interior not zeroed (it keeps the sentinel) is seen by the whole-buffer comparison of bits
    sent = R.sentinel_elems((2, 9, 14, 8), name)
    want = torch.where(written.unsqueeze(-1), out, sent)
    wrong = want.clone()
    wrong[:, 3:6, 3:9, 5] = sent[:, 3:6, 3:9, 5]
    assert not torch.equal(R.bits(wrong), R.bits(want))
    assert bool((R.bits(want)[:, 3:6, 3:9, 5:] == 0).all()) and bool((R.bits(want)[:, 0] == R.SENTINEL_BITS[name]).all())


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_pack_weights_reference_is_a_literal_loop_unpack_is_its_inverse_and_a_transposed_tap_shows(name):
    g = torch.Generator().manual_seed(5)
    dt = R.ELEM[name][0]
    w = torch.randn(4, 3, 3, 3, generator=g)
    fwd, dgr = R.pack_weights_ref(w, name)
    for r in range(3):
        for t in range(3):
            for co in range(4):
                for ci in range(3):
                    assert fwd[r * 3 + t, co, ci] == w[co, ci, r, t].to(dt) == dgr[r * 3 + t, ci, co]
    ws = torch.randn(6, 5, 7, 7, generator=g)
    sf, none = R.pack_weights_ref(ws, name, stem=True)
    assert none is None and sf.shape == (7, 6, 64)
    for r in range(7):
        for co in range(6):
            for t in range(8):
                for c in range(8):
                    want = ws[co, c, r, t].to(dt) if t < 7 and c < 5 else 0.0
                    assert sf[r, co, t * 8 + c] == want
    # unpack(pack-layout(x)) == x on fp32, whatever fills the unused columns
    for Co, Ci, k, Kc, stem in R.UNPACK_CASES + ((32, 32, 2, 40, 0),):
        gr = torch.randn(Co, Ci, k, k, generator=g)
        wg = R.wgrad_scratch_layout(gr, Kc, bool(stem), fill=float("nan"))
        assert torch.equal(R.unpack_grads_ref(wg, Co, Ci, k, Kc, bool(stem)), gr)
    assert torch.equal(R.wgrad_scratch_layout(ws, 64, True), R.stem_rowtap(ws))
    # resolution: ONE tap transposed ((r, t) = (0, 1) <-> (1, 0)) changes both layouts, in those two taps only
    wt = w.clone()
    wt[:, :, 0, 1], wt[:, :, 1, 0] = w[:, :, 1, 0], w[:, :, 0, 1]
    f2, d2 = R.pack_weights_ref(wt, name)
    assert not torch.equal(R.bits(f2), R.bits(fwd)) and not torch.equal(R.bits(d2), R.bits(dgr))
    assert torch.equal(f2[1], fwd[3]) and torch.equal(f2[3], fwd[1]) and torch.equal(f2[4:], fwd[4:])


def _adamw1_f32(p, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0):
    """adamw1 + adam_hyper of vpd_amd/csrc/optim.hip in numpy float32, operation by operation (fmaf: the exact product of two
    floats in float64, one addition, rounded to float)"""
    f = np.float32
    decay, omb1, b2f, omb2 = f(1.0 - lr * wd), f(1.0 - b1), f(b2), f(1.0 - b2)
    step_size, isb, epsf = f(lr / (1.0 - b1 ** step)), f(1.0 / np.sqrt(1.0 - b2 ** step)), f(eps)
    fma = lambda a, b, c: (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f)
    p, g, m, v = (t.numpy().astype(f) for t in (p, g, m, v))
    g = g * f(gscale)
    p = p * decay
    m = fma(g - m, omb1, m)
    v = fma(omb2 * g, g, v * b2f)
    den = fma(np.sqrt(v), isb, epsf)
    p = fma(-step_size, m / den, p)
    return torch.from_numpy(p), torch.from_numpy(m), torch.from_numpy(v)


def test_adamw_reference_is_torch_optim_adamw_in_float64():
    g = torch.Generator().manual_seed(9)
    for hp in R.ADAM_HYPERS.values():
        p0 = torch.randn(4096, generator=g)
        ref = torch.nn.Parameter(p0.double().clone())
        opt = torch.optim.AdamW([ref], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
        p, m, v = p0.double(), torch.zeros(4096, dtype=torch.float64), torch.zeros(4096, dtype=torch.float64)
        for t in (1, 2, 3):
            gr = torch.randn(4096, generator=g) * 10.0 ** (t - 2)
            ref.grad = gr.double()
            opt.step()
            p, m, v = R.adamw_ref(p, gr, m, v, step=t, **hp)
            st = opt.state[ref]
            for a, b in ((p, ref.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                assert float(((a - b).abs() / b.abs().clamp_min(1e-300)).max()) <= 1e-12


ADAM_REGIMES = [(h, s) for h in R.ADAM_HYPERS for s in R.ADAM_STEPS]


@pytest.mark.parametrize("hyper,step", ADAM_REGIMES)
def test_adamw_bounds_hold_an_fp32_transcription_and_reject_perturbed_hyper_parameters(hyper, step):
    """on the GPU tests' own inputs: the fp32 transcription of adamw1 stays inside every bound (ratio <= 1), and a reference with
    one hyper-parameter 0.1 % off (the step number: 1 off) leaves at least a quarter of some output outside its bound -- where the
    change exists in exact arithmetic at all: weight decay moves p by lr wd / 1000 relative, 5e-9 = u / 12 for torch's defaults
    (the `strong` set makes it 1e-6 = 17 u), and the bias corrections of steps t and t - 1 are the same doubles at t = 100,000"""
    hp = R.ADAM_HYPERS[hyper]
    ins = R.adamw_inputs(R.ADAM_N, step, 1)
    got = _adamw1_f32(*ins, step=step, **hp)
    ref = R.adamw_ref(*ins, step=step, **hp)
    bnd = R.adamw_bounds(*ins, step=step, **hp)
    ratios = [float(((a.double() - b).abs() / c).max()) for a, b, c in zip(got, ref, bnd)]
    print("adamw %s step %d: max error / bound p %.3f m %.3f v %.3f" % ((hyper, step) + tuple(ratios)))
    assert max(ratios) <= 1.0, ratios

    def outside(**change):
        h2 = dict(hp, step=step)
        h2.update(change)
        off = R.adamw_ref(*ins, **h2)
        return max(float(((a.double() - b).abs() > c).float().mean()) for a, b, c in zip(got, off, bnd))
    for key in ("lr", "b1", "b2"):
        assert outside(**{key: hp[key] * 1.001}) >= 0.25, key
        assert outside(**{key: hp[key] * 0.999}) >= 0.25, key
    if hyper == "strong":
        assert outside(wd=hp["wd"] * 1.001) >= 0.25 and outside(wd=hp["wd"] * 0.999) >= 0.25
    # the step number: wherever a bias correction of the neighbouring step differs by more than 1e-5 relative (170 u) in exact
    # arithmetic -- steps 1, 2, 3 of both sets and step 1,000 with b2 = 0.999 (0.999^1000 = 0.37); beyond, they converge to 1
    def corrections(t):
        return (1.0 / (1.0 - hp["b1"] ** t), 1.0 / np.sqrt(1.0 - hp["b2"] ** t))
    for other in (step + 1, step - 1):
        if other < 1:
            continue
        rel = max(abs(a / b - 1.0) for a, b in zip(corrections(other), corrections(step)))
        assert (rel >= 1e-5) == (step <= 3 or (hyper, step) == ("torch", 1000)), (other, rel)
        if rel >= 1e-5:
            assert outside(step=other) >= 0.25, other                          # (step - 1: the bias correction of step t - 1)


def test_adamw_gradient_scale_by_a_power_of_two_is_exact_in_the_transcription():
    hp = R.ADAM_HYPERS["torch"]
    p, g, m, v = R.adamw_inputs(1 << 14, 3, 2)
    a = _adamw1_f32(p, g, m, v, step=3, **hp)
    b = _adamw1_f32(p, g * 4096.0, m, v, step=3, gscale=2.0 ** -12, **hp)
    assert all(torch.equal(R.bits(x), R.bits(y)) for x, y in zip(a, b))


def test_adam_pack_buffers_have_the_plain_ranges_the_cases_ask_for():
    for name in R.ADAM_PACK_BUFFERS:
        dims, offs, numel = R.adam_pack_layout(name)
        assert numel % 4 == 0 and all(o % 4 == 0 for o in offs)
        assert {k for _, _, k in dims} >= {1, 3}
    gaps = [x for b in R.ADAM_PACK_BUFFERS.values() for x in b["gaps"]]
    assert any(0 < x < 2048 for x in gaps) and any(x % 256 for x in gaps) and any(x > 2048 for x in gaps)
    assert any(k == 2 for b in R.ADAM_PACK_BUFFERS.values() for _, _, k in b["convs"])   # khw = 4: the general gather


@pytest.mark.parametrize("ksplit", R.SLAB_KSPLITS)
def test_slab_sum_reference_is_exact_on_integers_and_its_bound_sees_a_dropped_split(ksplit):
    g = torch.Generator().manual_seed(ksplit)
    n = R.SLAB_LENGTHS[-1]
    s = R.slab_partials(n, ksplit, True, g)
    ref, _ = R.slab_sum_ref(s)
    assert float(s.abs().sum(0).max()) < 2 ** 24
    for order in (range(ksplit), reversed(range(ksplit))):                     # fp32 sums of these integers: exact in any order
        acc = torch.zeros(n)
        for i in order:
            acc = acc + s[i]
        assert torch.equal(acc.double(), ref)
    s = R.slab_partials(n, ksplit, False, g)
    ref, bound = R.slab_sum_ref(s)
    acc = torch.zeros(n)
    for i in range(ksplit):
        acc = acc + s[i]
    assert bool(((acc.double() - ref).abs() <= bound).all())
    if ksplit > 1:                                                             # one split dropped: outside nearly everywhere
        dropped = s[:-1].double().sum(0)
        assert float(((dropped - ref).abs() > bound).float().mean()) > 0.95
        si = R.slab_partials(n, ksplit, True, g)
        assert float((si[:-1].double().sum(0) != si.double().sum(0)).float().mean()) > 0.99
