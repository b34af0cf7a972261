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
