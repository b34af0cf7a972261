"""The 64-wide weight-gradient kernels of conv_wgrad.hip per element, route by route, in both libraries
(tests/wgrad_routes_child.py, one child per library and mode; the operands and references are opref's).

group    vpd_op_wgrad_group, the launch WgradQueue::flush makes for every 3x3 stride-1 convolution whose output channels are no
         multiple of 128 (conv_wgrad_halo_grouped_kernel: task table, XCD remap over a padded grid, a split per problem from the
         cost model; one split stores straight into dw, more go through the slab).  The split table of every group is asserted
         through vpd_op_wgrad_group_dispatch.  In the integer regime each problem must also equal, in bits, vpd_op_wgrad with a slab
         on that problem alone.
stem     conv_wgrad_stem_kernel at TR = 1, 2 and 4, with more than 256 chunks (cpb 3, a last split of one chunk), and two shapes
         it refuses, which the atomics kernel takes.
halo1x1  the 1x1 cases of test_ops_gpu.py::CONV_CASES with VPD_WGRAD_1X1=1: the centre tap of the halo kernel.

Pass instantiations.  tests/test_wgrad_routes_cpu.py enumerates every H x W plane with W in 1..64 and H up to 128: stride-1 planes
reach the 4-pass (NHP 100..128) and the 5-pass (NHP 136..160) instantiation only, both covered by the groups; no plane gives
NHP <= 96, so conv_wgrad_halo_kernel<3> and conv_wgrad_halo_grouped_kernel<3> are unreachable.  Stride 2 reaches the 10-pass and
the 13-pass (two-stage) instantiations, covered by halo1x1 here and by tests/test_wgrad_pair_gpu.py; the 3/4/5-pass ones are
unreachable at stride 2."""
import json
import os
import subprocess
import sys

import pytest

from tests import opref as R
from tests.wgrad_routes_child import HALO_1X1_INST

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_results = {}


def _child(dtype, mode):
    if (dtype, mode) not in _results:
        env = dict(os.environ)
        env.pop("VPD_WGRAD_1X1", None)
        if mode == "halo1x1":
            env["VPD_WGRAD_1X1"] = "1"
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "wgrad_routes_child.py"), dtype, mode], env=env,
                           capture_output=True, text=True, timeout=900, cwd=REPO)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        _results[(dtype, mode)] = json.loads(line[len("RESULT "):])
    return _results[(dtype, mode)]


def _assert_case(out):
    print(json.dumps(out["dispatch"]), json.dumps(out["figures"]))
    assert not out["fail"], "\n".join(out["fail"])
    assert any(k.startswith("int") for k in out["figures"]) and any(k.startswith("randn") for k in out["figures"]), "nothing was compared"


@pytest.mark.parametrize("group", list(R.WG_GROUPS), ids=list(R.WG_GROUPS))
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_grouped_64_wide_launch_per_element(dtype, group):
    _assert_case(_child(dtype, "group")[group])


@pytest.mark.parametrize("case", list(R.WG_STEM) + list(R.WG_STEM_REFUSED), ids=list(R.WG_STEM) + list(R.WG_STEM_REFUSED))
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_stem_weight_gradient_per_element(dtype, case):
    _assert_case(_child(dtype, "stem")[case])


@pytest.mark.parametrize("case", list(HALO_1X1_INST), ids=list(HALO_1X1_INST))
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_one_by_one_on_the_halo_route_per_element(dtype, case):
    _assert_case(_child(dtype, "halo1x1")[case])
