"""The fused Bottleneck tail one launch at a time: conv1x1_bn_stream_kernel<KC, NSA, 1|2|3>, its statistics pass
conv1x1_stream_kernel<.., 4> and the two-convolution conv1x1_bn2_stream_kernel<NSA, 1|2|3> (conv_stream.hip) through
vpd_op_conv1x1_bn / vpd_op_conv1x1_bn2, in the bf16 and the fp16 library, against the float64 chain of tests/opref.py (pinned by
tests/test_opref_cpu.py).

A block of these kernels walks its 64-pixel tiles through an LDS ring of 8 (64 input channels) or 5 stages; a stage is reused only
from the block's ninth / sixth tile on.  The few-CU runs (VPD_RESERVE_CUS=248: 8 pixel lanes) give every block 8 to 12 tiles of a
tensor of a few MB; the child asserts that through vpd_op_conv1x1_bn_dispatch before it launches anything.  Three more runs use the
whole device; one of them gives K = 128 blocks fewer tiles (2-3) than the 5-stage ring runs ahead.

Integer operands: the statistics rows of modes 0 and 2 must be EQUAL to the float64 sums.  Both regimes: out and dz per element
within bounds derived from the fp32 arithmetic (opref.tail_out_bound, bn_dz_bound), the bit map equal to [stored out != 0], the
forward bit-identical to vpd_op_bn_forward on the unfused launch's stored z and the same rows, sentinels intact around every
output.  Whether mode 3 reproduces vpd_op_bn_backward_apply bit for bit is recorded, not gated."""
import json
import os
import subprocess
import sys

import pytest

from tests.bneck_tail_child import RUNS

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("run", list(RUNS), ids=list(RUNS))
def test_tail_run_dispatches_as_named_and_matches_float64(run):
    env = dict(os.environ, **RUNS[run][1])
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "bneck_tail_child.py"), run, "full"], env=env, capture_output=True,
                       text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print("\n".join("%s %s" % (run, ln) for ln in r.stdout.splitlines() if "max err / bound" in ln))
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    print(run, "dispatch", out["dispatch"])
    print(run, {k: v for k, v in out["record"].items() if "bit_identical" in k})
    assert not out["fail"], "\n".join(out["fail"])
    rec = out["record"]
    assert rec, "nothing was compared"
    # integer regime: every statistics row and the unfused z equal to float64, in both libraries
    exact = [k for k, v in rec.items() if isinstance(v, dict) and "differ" in v]
    assert len(exact) >= 2 * 4 and all(rec[k]["differ"] == 0 for k in exact), {k: rec[k] for k in exact if rec[k]["differ"]}
    for name in ("bf16", "fp16"):
        for regime in ("int", "rand"):
            assert rec["%s/%s/out" % (name, regime)]["max_err_over_bound"] <= 1.0
            for which in ("rand_map", "own_map"):
                assert rec["%s/%s/%s/dz" % (name, regime, which)]["max_err_over_bound"] <= 1.0
            assert rec["%s/%s/fwd_bit_identical_to_unfused" % (name, regime)] is True
    d = out["dispatch"]
    if RUNS[run][1]:
        assert d["tiles"] > d["ring"], d
