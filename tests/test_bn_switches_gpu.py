"""The two BatchNorm switches at plan level, each setting in a fresh process (the switches are read once):
VPD_BN_XCD (the XCD-affine block order of the fused launches, bn.hip's vpd_bn_virtual_block: claimed bit-identical either way) and
VPD_FUSED_BN=0 (the fallback trainer.py names when a grid-barrier time-out is counted: bn_finalize_kernel + bn_apply_kernel and the
three-launch backward), which must pass exactly what the default path passes."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from tests import opref_bn_fwd as B

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the BasicBlock stages of resnet18 on the digest's 128 x 128 crops: (H = W, C) of every 3x3 stride-1 convolution's BatchNorm
STAGES = {"layer1": (32, 64), "layer2": (16, 128), "layer3": (8, 256), "layer4": (4, 512)}
_digests = {}


def stage_r(batch):
    """R of vpd_bn_virtual_block per stage at `batch` crops: the neighbouring 3x3 launch's pixel tile (vpd_op_conv2d_dispatch, host
    only) through the transcription of vpd_bn_xcd_r, at the grid vpd_launch_bn_fwd_fused takes"""
    from vpd_amd._lib import check, lib
    L = lib()
    taps = (C.c_int * 9)(3, 3, 0, 1, 0, 1, 0, 3, 1)
    out = (C.c_int * 12)()
    rs = {}
    for stage, (hw, c) in STAGES.items():
        check(L.vpd_op_conv2d_dispatch(batch, hw + 2, hw + 2, c, hw, hw, c, 0, hw, hw, 1, 0, 0, 1, c, c, taps, 0, 1, out), "dispatch")
        tile = out[7] if out[1] else 0      # (the XCD-affine tile order is the pipelined kernel's)
        rs[stage] = B.xcd_r(tile, c, B.fused_geometry(batch * hw * hw, c)["grid"])
    return rs


def smallest_permuting_batch():
    for batch in range(8, 257, 8):
        rs = stage_r(batch)
        if sum(1 for r in rs.values() if r >= 2) >= 2:
            return batch, rs
    raise AssertionError("no batch up to 256 crops gives two stages R >= 2: %s" % (stage_r(256),))


def _digest(dtype, batch, **env):
    key = (dtype, batch, tuple(sorted(env.items())))
    if key not in _digests:
        r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "step_digest.py"), "--arch", "resnet18", "--batch", str(batch),
                            "--dtype", dtype], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900, cwd=REPO)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("losses ")]
        assert len(lines) == 1, r.stdout[-2000:]
        assert "nan" not in lines[0] and "inf" not in lines[0], lines[0]
        _digests[key] = lines[0]
    return _digests[key]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_step_digest_is_the_same_in_either_block_order(dtype):
    batch, rs = smallest_permuting_batch()
    print("batch", batch, rs)
    assert sum(1 for r in rs.values() if r >= 2) >= 2 and all(sorted(B.virtual_block(b, 256, r) for b in range(256)) == list(range(256))
                                                              for r in rs.values())
    on, off = _digest(dtype, batch, VPD_BN_XCD="1"), _digest(dtype, batch, VPD_BN_XCD="0")
    print(on)
    assert on == off, "VPD_BN_XCD=1: %s\nVPD_BN_XCD=0: %s" % (on, off)


def test_unfused_path_passes_the_gates_of_the_default_path():
    """VPD_FUSED_BN=0: the whole-network gates of tests/test_model_gpu.py, unchanged, in a child under that environment; and the
    switch did take -- the step digest differs from the default path's (fp64 1 / sqrt against v_rsq_f32, three-launch sums against
    the barrier kernels' order)"""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "bn_switches_child.py"), "gates"], env=dict(os.environ, VPD_FUSED_BN="0"),
                       capture_output=True, text=True, timeout=900, cwd=REPO)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(lines[-1][len("RESULT "):])
    print(out["ran"], out["engines"], out["sync_errors"])
    assert not out["fail"], "\n".join(out["fail"])
    assert r.returncode == 0 and out["fused_bn"] == "0" and len(out["ran"]) == 3
    assert out["engines"] >= 3 and out["sync_errors"] == 0
    batch, _ = smallest_permuting_batch()
    default, unfused = _digest("bf16", batch, VPD_BN_XCD="1"), _digest("bf16", batch, VPD_FUSED_BN="0")
    print(default)
    print(unfused)
    assert default != unfused, "VPD_FUSED_BN=0 printed the default path's digest: the switch did not take"
