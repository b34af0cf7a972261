"""Stem BatchNorm + ReLU + MaxPool (stem_pool_kernel, stem_pool_pair_kernel) and its backward (stem_pool_bwd_kernel pass 1 / 2,
stem_pool_bwd_quad_kernel, stem_pool_bwd_sums_kernel) one launch at a time, through vpd_op_stem_pool_forward / _backward, against
float64 PyTorch on the CPU (tests/opref.py; tests/test_opref_cpu.py pins the references themselves).

Forward: inputs on an exact grid (z = k/16, scale in {0.5 .. 1.5}, shift = j/8) make every intermediate exact, so values AND
arg-max taps must EQUAL the reference -- the windows tie all the time, which is what exercises the first-maximum rule -- at even,
odd and non-power-of-two sizes and at 512 crops (>= 2^21 items: the 64-bit division path).  randn inputs: within one element ulp.
Backward: closed form routed by the kernel's own arg-max taps (equal to autograd when routed by torch's: CPU test), dbeta /
dgamma within 2e-5 sum|terms|, dz within rel-L2 3e-3 (bf16) and per element within one output ulp + the propagated sum error;
with the pooled-side sums (VPD_STEM_POOLSUMS=1) the dgamma bound is widened by that approximation's derived worst case
half_ulp * sum |d a| / |gamma|.  Measured against it (dumped to parity_stem_ops_<dtype>.json, table in DESIGN.md): dgamma of the
pooled-side sums is 2e-4 (bf16) / 3e-5 (fp16) off in rel-L2 where the sums over z are 4e-8 off, at most 0.96 of the widened bound
(nearly dead channels with 3-7 live windows, negative gamma among them; a float64 restatement of the formula errs the same).

The switches are read once per process: every setting runs in a fresh child (tests/stem_ops_child.py), one after the other."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(REPO, "tests", "stem_ops_child.py")


def _run(dtype, what, env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, CHILD, dtype, what], env=env, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_stem_pool_forward_equals_reference_on_exact_inputs(dtype):
    from tests.test_model_gpu import _dump
    res = {}
    for pair in ("1", "0"):
        res[pair] = _run(dtype, "forward", {"VPD_STEM_PAIR": pair})
        print("VPD_STEM_PAIR=%s" % pair, json.dumps(res[pair]["record"]))
    _dump("stem_forward_%s" % dtype, {p: res[p]["record"] for p in res})
    for pair in res:
        assert res[pair]["fail"] == [], (pair, res[pair]["fail"])
    # the pair kernel orders candidates by the raw bits of the packed element pair: same outputs and taps as one output per thread
    assert res["1"]["digest"] == res["0"]["digest"]
    assert len(res["1"]["digest"]) == 13                   # 5 grid cases (the 512-crop one among them) + 4 shapes x 2 regimes of randn


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_stem_pool_backward_matches_float64_closed_form(dtype):
    from tests.test_model_gpu import _dump
    res = {}
    for poolsums in ("1", "0"):
        for quad in ("1", "0"):
            key = "poolsums%s_quad%s" % (poolsums, quad)
            res[key] = _run(dtype, "backward", {"VPD_STEM_POOLSUMS": poolsums, "VPD_STEM_QUAD": quad})
            print(key, json.dumps(res[key]["record"]))
    _dump("stem_ops_%s" % dtype, {k: v["record"] for k, v in res.items()})
    for key, v in res.items():
        assert v["fail"] == [], (key, v["fail"])
        assert len(v["record"]) == 10                      # 5 shapes x 2 regimes, none skipped
        assert all(rec["poolsums"] == key.startswith("poolsums1") for rec in v["record"].values())
    # pass 1 decides the sums only: with the same pass 2, the two settings' dz may differ by what the sums differ, no more -- and an
    # odd-sized stem takes the pixel-at-a-time pass 2 whatever VPD_STEM_QUAD says: identical bits
    for ps in ("1", "0"):
        a, b = res["poolsums%s_quad1" % ps]["digest"], res["poolsums%s_quad0" % ps]["digest"]
        for tag in a:
            if tag.startswith("odd"):
                assert a[tag] == b[tag], tag
