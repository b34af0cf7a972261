"""The down-sampling BasicBlock's two weight gradients in one launch (conv_wgrad_halo_pair_kernel, VPD_WGRAD_DS_RIDE): the 1x1
stride-2 branch rides on the halo that the 3x3 stride-2 conv1 stages.

Operator (vpd_op_wgrad_pair, tests/wgrad_pair_child.py, one child per library): the three boundary shapes of ResNet-18/34 with batch
sizes that give one chunk per split, a short last split and ragged last chunks.  Every output is pre-filled with a sentinel.  On
randn operands both gradients must be EQUAL IN BITS to the two vpd_op_wgrad launches the pair replaces -- same pixel split, same
chunk order, same MFMA K order per accumulator, same grouping in the slab sum -- and on integer operands in {-1, 0, 1} EQUAL to
float64 conv2d backward (every partial sum is an integer below 2^24).

Whole step: tools/step_digest.py prints the same line with VPD_WGRAD_DS_RIDE=1 and =0, for ResNet-34 and ResNet-18 on 256 crops, in
the bf16 and the fp16 library."""
import json
import os
import subprocess
import sys

import pytest

from tests.wgrad_pair_child import CASES

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_results = {}


def _child(dtype):
    if dtype not in _results:
        env = dict(os.environ, VPD_WGRAD_1X1="1", VPD_WGRAD_DS_RIDE="1")
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "wgrad_pair_child.py"), dtype], env=env,
                           capture_output=True, text=True, timeout=900, cwd=REPO)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        _results[dtype] = json.loads(line[len("RESULT "):])
    return _results[dtype]


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_pair_equals_the_two_launches_in_bits_and_float64_on_integers(dtype, case):
    out = _child(dtype)[case]
    print(json.dumps(out["figures"]))
    assert out["figures"], "nothing was compared"
    assert not out["fail"], "\n".join(out["fail"])


def _digest(arch, dtype, ride):
    env = dict(os.environ, VPD_WGRAD_DS_RIDE=str(ride))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "step_digest.py"), "--arch", arch, "--batch", "256",
                        "--dtype", dtype], env=env, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("losses ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("arch", ["resnet34", "resnet18"])
def test_step_digest_is_the_same_with_and_without_the_ride(arch, dtype):
    new, old = _digest(arch, dtype, 1), _digest(arch, dtype, 0)
    print(new)
    assert "nan" not in new and "inf" not in new, new
    assert new == old, "VPD_WGRAD_DS_RIDE=1: %s\nVPD_WGRAD_DS_RIDE=0: %s" % (new, old)
