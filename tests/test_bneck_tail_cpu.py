"""The operator entry points of the fused Bottleneck tail (vpd_op_conv1x1_bn, vpd_op_conv1x1_bn2, vpd_op_conv1x1_bn_dispatch), the part
that needs no GPU: what they refuse -- on the host, before anything is launched -- and what the launchers decide for the runs of
tests/test_bneck_tail_ops_gpu.py on a 256-CU device (the count the library assumes without one)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_float
P = C.c_void_p(64)                                        # never dereferenced: every call below is rejected before a launch


def _bn(h, mode, n=40, H=32, W=32, istr=1, Kc=64, Co=256, drop=()):
    """vpd_op_conv1x1_bn with every pointer present but those named in drop"""
    names = ("x", "w", "rows", "gamma", "beta", "rm", "rv", "mean", "rstd", "scale", "shift", "res", "out", "mask", "dout", "dz", "dgamma", "dbeta")
    a = {k: (None if k in drop else P) for k in names}
    return h.vpd_op_conv1x1_bn(mode, a["x"], a["w"], n, H, W, istr, Kc, Co, a["rows"], a["gamma"], a["beta"], a["rm"], a["rv"], F(0.1), F(1e-5),
                               a["mean"], a["rstd"], a["scale"], a["shift"], a["res"], a["out"], a["mask"], a["dout"], a["dz"], a["dgamma"],
                               a["dbeta"], None)


def _bn2(h, mode, n=40, H=32, W=32, Kc=64, Kc2=64, Co=256, drop=()):
    names = ("x", "w", "x2", "w2", "rows", "rows2", "gamma", "beta", "rm", "rv", "mean", "rstd", "scale", "shift", "gamma2", "beta2", "rm2", "rv2",
             "mean2", "rstd2", "scale2", "shift2", "out", "mask", "dout", "dz", "dz2", "dgamma", "dbeta", "dgamma2", "dbeta2")
    a = [None if k in drop else P for k in names]
    return h.vpd_op_conv1x1_bn2(mode, *a[:4], n, H, W, Kc, Kc2, Co, *a[4:22], F(0.1), F(1e-5), *a[22:], None)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_tail_entry_points_refuse_what_the_launchers_refuse(dtype):
    """40 crops of 32 x 32 (640 pixel tiles) are a shape both launchers take at the default budget of 256 CUs, as the query says
    first; every call below differs from it in the one argument named and is refused on the host."""
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    out = (C.c_int * 5)()
    assert h.vpd_op_conv1x1_bn_dispatch(40, 32, 32, 64, 256, 0, out) == 0 and list(out) == [1, 256, 1, 3, 8]
    shape = lambda rc: rc != 0 and b"does not take this shape" in h.vpd_last_error()
    for mode in (0, 1, 2, 3):
        assert shape(_bn(h, mode, Kc=256)), mode                       # 256 input channels
        assert shape(_bn(h, mode, Co=128)), mode                       # no 256-channel tile
        assert shape(_bn(h, mode, istr=2)), mode                       # stride 2
        assert shape(_bn(h, mode, n=60, H=32, W=24)), mode             # a width that does not divide 64
        assert shape(_bn(h, mode, n=4)), mode                          # 64 pixel tiles: fewer than two per CU
    for mode, needs in ((0, ("x", "w", "rows")), (1, ("rows", "gamma", "beta", "mean", "rstd", "scale", "shift", "res", "out", "rm", "rv")),
                        (2, ("rows", "dout", "mask")), (3, ("rows", "dout", "mask", "gamma", "mean", "rstd", "dz", "dgamma", "dbeta"))):
        for k in needs:
            assert _bn(h, mode, drop=(k,)) != 0 and b"null argument" in h.vpd_last_error(), (mode, k)
    assert _bn(h, 4) != 0 and _bn(h, -1) != 0 and b"mode" in h.vpd_last_error()
    assert _bn(h, 0, n=0) != 0 and b"bad argument" in h.vpd_last_error()
    assert _bn(h, 0, Kc=96) != 0 and b"bad argument" in h.vpd_last_error()
    # the two-convolution kernel: 64 + 64 input channels, 256 output channels, and everything the one-convolution launcher refuses
    for mode in (1, 2, 3):
        assert shape(_bn2(h, mode, Kc=128, Kc2=128)) and shape(_bn2(h, mode, Kc2=128)) and shape(_bn2(h, mode, Co=512)), mode
        assert shape(_bn2(h, mode, n=4)) and shape(_bn2(h, mode, n=60, W=24)), mode
    for mode, needs in ((1, ("x2", "w2", "rows2", "gamma2", "beta2", "mean2", "rstd2", "scale2", "shift2", "out", "rm2", "rv")),
                        (2, ("rows", "rows2", "dout", "mask")), (3, ("gamma2", "mean2", "rstd2", "dz", "dz2", "dgamma2", "dbeta"))):
        for k in needs:
            assert _bn2(h, mode, drop=(k,)) != 0 and b"null argument" in h.vpd_last_error(), (mode, k)
    assert _bn2(h, 0) != 0 and b"mode" in h.vpd_last_error()           # (its statistics passes are two mode-0 calls of the other)
    # the host-only query: not eligible is an answer, not an error
    for args in ((40, 32, 32, 256, 256, 0), (40, 32, 32, 64, 128, 0), (4, 32, 32, 64, 256, 0), (60, 32, 24, 64, 256, 0), (40, 32, 32, 128, 256, 1),
                 (40, 32, 32, 64, 512, 1)):
        assert h.vpd_op_conv1x1_bn_dispatch(*args, out) == 0 and list(out) == [0, 0, 0, 0, 0], args
    assert h.vpd_op_conv1x1_bn_dispatch(40, 32, 32, 128, 512, 0, out) == 0 and list(out) == [1, 128, 2, 5, 5]
    assert h.vpd_op_conv1x1_bn_dispatch(40, 32, 32, 64, 256, 0, None) != 0 and b"null argument" in h.vpd_last_error()
    assert h.vpd_op_conv1x1_bn_dispatch(0, 32, 32, 64, 256, 0, out) != 0 and b"bad argument" in h.vpd_last_error()


def test_tail_entry_points_refuse_everything_with_the_recompute_switch_off():
    """VPD_BNECK_RECOMPUTE=0 (read once per process): the step runs conv + BatchNorm launches, and the entry points refuse"""
    code = ("import ctypes as C\n"
            "from tests.test_bneck_tail_cpu import _bn, _bn2\n"
            "from vpd_amd import _lib\n"
            "for dtype in ('bf16', 'fp16'):\n"
            "    h = _lib.lib(dtype)\n"
            "    out = (C.c_int * 5)()\n"
            "    assert h.vpd_op_conv1x1_bn_dispatch(40, 32, 32, 64, 256, 0, out) == 0 and list(out) == [0] * 5\n"
            "    assert h.vpd_op_conv1x1_bn_dispatch(40, 32, 32, 64, 256, 1, out) == 0 and list(out) == [0] * 5\n"
            "    for mode in (0, 1, 2, 3):\n"
            "        assert _bn(h, mode) != 0 and b'does not take this shape' in h.vpd_last_error()\n"
            "    for mode in (1, 2, 3):\n"
            "        assert _bn2(h, mode) != 0 and b'does not take this shape' in h.vpd_last_error()\n"
            "print('refused')\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VPD_BNECK_RECOMPUTE="0"), capture_output=True, text=True,
                       timeout=300, cwd=REPO)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stdout[-2000:] + r.stderr[-2000:]


def test_tail_runs_dispatch_as_their_ids_name():
    """vpd_op_conv1x1_bn_dispatch is host-only: every run of the GPU test must already report its pixel lanes, channel tiles, tiles
    per block and ring depth here, and every few-CU run more tiles per block than its ring is deep.  One child per switch setting."""
    from tests.bneck_tail_child import RUNS
    by_env = {}
    for run, (_, env, _) in RUNS.items():
        by_env.setdefault(json.dumps(env, sort_keys=True), []).append(run)
    seen = {}
    for env, runs in by_env.items():
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "bneck_tail_child.py"), ",".join(runs), "dispatch"],
                           env=dict(os.environ, **json.loads(env)), capture_output=True, text=True, timeout=300, cwd=REPO)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        for ln in r.stdout.splitlines():
            if ln.startswith("RESULT "):
                out = json.loads(ln[len("RESULT "):])
                assert not out["fail"], (out["run"], out["fail"])
                seen[out["run"]] = out["dispatch"]
    assert set(seen) == set(RUNS)
    few = [d for run, d in seen.items() if RUNS[run][1]]
    assert len(few) == 7 and all(d["tiles"] > d["ring"] and d["lanes"] == 8 for d in few)
    # both ring depths of the one-convolution kernel, one and two channel tiles, the two-convolution kernel
    assert {(d["ring"], d["channel_tiles"]) for d in few} == {(8, 1), (8, 2), (5, 1), (5, 2)}
