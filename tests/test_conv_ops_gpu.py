"""The convolution family one launch at a time (conv_igemm.hip, conv_pws.h, conv_pws_geo.hip, conv_epilogue.h, conv_wgrad.hip), in the
bf16 and the fp16 library, against float64 PyTorch on the CPU (tests/opref.py, pinned by tests/test_opref_cpu.py).

Every run is a case of opref.CONV_CASES under one setting of the launcher's switches, in a child process (tests/conv_ops_child.py).
Before anything is launched the child asks vpd_op_conv2d_dispatch what the launcher decides for each operation -- kernel class,
persistent form, compile-time-geometry instantiation, tile, epilogue mode, tiles per block -- and fails when that is not what the
run's id names: a changed threshold cannot move a case to another kernel unnoticed.

Two input regimes.  Integer operands ({-1, 0, 1}, small integers in the epilogues) make every product and partial sum an integer
below 2^24 and every result an element-type value: forward, data gradient, accumulate, masked accumulate, eval epilogue, the
statistics rows and the fp32 weight gradients must be EQUAL to the reference -- a dropped, doubled or misplaced tap, chunk, pixel
or mask bit changes a sum by at least 1.  randn operands check the arithmetic against a per-element bound derived from the fp32
accumulator (opref.conv_bound).  Every output buffer is pre-filled with a sentinel: borders of padded outputs and the slack
behind the buffer must keep it.  Switch variants of a run (geometry off, conv3x3_ws_kernel) must reproduce its outputs bit for
bit."""
import json
import os
import subprocess
import sys

import pytest

from tests.conv_ops_child import RUNS, SAME_BITS

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_results = {}


def _run(run):
    if run not in _results:
        # a variant is compared with its base bit for bit in both regimes; the base carries the random regime's references
        mode = "light" if run in SAME_BITS else "full"
        env = dict(os.environ, **RUNS[run][1])
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "conv_ops_child.py"), run, mode], env=env,
                           capture_output=True, text=True, timeout=900, cwd=REPO)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        print("\n".join(ln for ln in r.stdout.splitlines() if "max err / bound" in ln))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        _results[run] = json.loads(line[len("RESULT "):])
    return _results[run]


@pytest.mark.parametrize("run", list(RUNS), ids=list(RUNS))
def test_conv_run_dispatches_as_named_and_matches_float64(run):
    out = _run(run)
    assert not out["fail"], "\n".join(out["fail"])
    assert out["record"], "nothing was compared"
    base = SAME_BITS.get(run)
    if base:
        ref = _run(base)
        assert not ref["fail"], "the base run %s fails" % base
        keys = [k for k in out["digest"] if not k.split("/")[-1].startswith("wgrad")]      # (fp32 atomics: order-dependent in randn)
        assert keys and set(keys) <= set(ref["digest"])
        differ = [k for k in keys if out["digest"][k] != ref["digest"][k]]
        assert not differ, "not bit-identical to %s: %s" % (base, differ)
