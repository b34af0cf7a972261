"""Interior loaders of conv3x3_pws_kernel's compile-time-geometry instantiations (vpd_amd/csrc/conv_pws.h, "interior mode"): on tiles
of whole images the MFMA waves zero the border slots of the two LDS halo buffers once per launch and the loader waves stream interior
row segments only.  No bit may change: every case runs forward with statistics, data gradient and accumulate (the child of tests/test_pws_gpu.py)
with VPD_PWS_INTERIOR=1, with =0 (the border-reading instantiation of the same kernel) and with VPD_PWS=0 (conv3x3_ws_kernel), and
the outputs must be equal -- the checksums of that child and a SHA-256 over the bytes.

One child process per setting runs ALL cases one after the other (the switches are read once per process), with VPD_PWS_BLOCKS = 2 =
the number of 64-channel tiles of every case: one block then walks every pixel tile of its channel tile, so the zeroed borders must
survive every tile and chunk hand-over.  The child first runs a shape that is not compared, and every case follows a case of another
shape, so no compared launch starts on a clean LDS.

Which kernel a shape reaches (vpd_conv_kernel_class; recorded from a kernel trace in profiles/pws_interior_ab.txt): with Co = 128 a
W = 8 / W = 16 shape takes the 256 x 64 tile of the compile-time-geometry kernels only from 200 pixel tiles of 128 on -- the 13- and
5-crop shapes run the generic loop on 128 x 64 tiles (old loader; they must still match) -- so 401 crops of 8 x 8 (100.25 tiles of four
images) and 101 crops of 16 x 16 are the smallest that reach them with a ragged / odd tile count.  The W = 4 shape reaches its kernel
(128 x 64 tile, eight images) as it is.  The child asks vpd_op_conv2d_dispatch and vpd_op_conv2d_interior (host-only: the launcher's own
decision), and the test asserts the width and the loader each case must get: a gate that never opened would pass every comparison.
Reference shapes: models/module.py:61-67 (3x3 stride-1 convs of layer2 / layer3 / layer4)."""
import json
import os
import subprocess
import sys

import pytest

from tests.test_pws_gpu import _CHILD, REPO

pytestmark = pytest.mark.gpu

# name: ((crops, Ci, Co, H, W), image width of the compile-time-geometry instantiation the forward must reach (0: none),
#        1: the forward must take the interior loaders with VPD_PWS_INTERIOR=1)
CASES = {
    "w8_two_chunks_ragged": ((401, 128, 128, 8, 8), 8, 1),    # 100.25 tiles of four images, two chunks
    "w16": ((101, 128, 128, 16, 16), 16, 1),                  # 101 tiles of one image, two row segments per row
    "w4_ragged": ((21, 128, 128, 4, 4), 4, 1),                # 2.6 tiles of eight images
    "w8_one_chunk": ((401, 64, 128, 8, 8), 8, 1),             # one chunk: the next TILE's halo rides in every chunk
    "w8_small_generic_loop": ((13, 128, 128, 8, 8), 0, 0),    # 3.25 tiles of 128 x 64: generic loop, old loader
    "w16_small_generic_loop": ((5, 128, 128, 16, 16), 0, 0),
    "gate_tiles_cut_images": ((3, 128, 128, 24, 16), 0, 0),   # eight-row tiles of a 24-row image: old loader
    "gate_geo_tiles_cut_images": ((51, 128, 128, 32, 16), 16, 0),   # compile-time-geometry kernel, tile = half an image: old loader
}

_DRIVER = r"""
import ctypes as C, hashlib, json, sys
sys.path.insert(0, {repo!r})
cases = {cases!r}
body = {body!r}
exec(compile(body.format(repo={repo!r}, case={warm!r}), "warm-up", "exec"), {{}})      # (not compared: the LDS is used from here on)
for name, (case, _, _) in cases.items():
    print("CASE " + name, flush=True)
    ns = {{}}
    exec(compile(body.format(repo={repo!r}, case=case), name, "exec"), ns)
    import torch
    from vpd_amd import _lib
    n, ci, co, h, w = case
    out = (C.c_int * 12)()
    args = (n, h + 2, w + 2, ci, h, w, co, 0, h, w, 1, 0, 0, 1, ci, co, ns["taps"], 0, 1)
    inter = (C.c_int * 1)()
    assert _lib.lib().vpd_op_conv2d_dispatch(*args, out) == 0 and _lib.lib().vpd_op_conv2d_interior(*args, inter) == 0
    sha = lambda t: hashlib.sha256(t.view(torch.int16).cpu().numpy().tobytes()).hexdigest()
    print("EXTRA " + json.dumps({{"dispatch": list(out), "interior": inter[0], "y_sha": sha(ns["y"]), "dx_sha": sha(ns["dx"])}}), flush=True)
"""

_WARM_UP = (2, 128, 128, 8, 16)     # the child's first launches: a shape of no case

_SETTINGS = {
    "interior": {"VPD_PWS": "1", "VPD_PWS_INTERIOR": "1", "VPD_PWS_BLOCKS": "2"},
    "border": {"VPD_PWS": "1", "VPD_PWS_INTERIOR": "0", "VPD_PWS_BLOCKS": "2"},
    "ws": {"VPD_PWS": "0"},
}


def _run_all(env_extra):
    env = dict(os.environ, **env_extra)
    src = _DRIVER.format(repo=REPO, cases=CASES, body=_CHILD, warm=_WARM_UP)
    r = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res, name = {}, None
    for ln in r.stdout.splitlines():
        if ln.startswith("CASE "):
            name = ln[5:]
            res[name] = {}
        elif name is None:
            continue                                                 # (the warm-up shape's line)
        elif ln.startswith("RESULT "):
            res[name].update(json.loads(ln[len("RESULT "):]))
        elif ln.startswith("EXTRA "):
            res[name].update(json.loads(ln[len("EXTRA "):]))
    assert set(res) == set(CASES), sorted(res)
    return res


@pytest.fixture(scope="module")
def runs():
    """{setting: {case: results}}: three child processes in all, one after the other; a child that fails stops the rest"""
    return {s: _run_all(e) for s, e in _SETTINGS.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_interior_loader_changes_no_bit(runs, case):
    new, old, ws = runs["interior"][case], runs["border"][case], runs["ws"][case]
    print(case, json.dumps({"interior": new, "border": old, "ws": ws}))
    # the kernel the shape reaches (out12 of vpd_op_conv2d_dispatch: class, pws, geo width, ...)
    assert new["dispatch"][1] == 1 and new["dispatch"][2] == CASES[case][1], new["dispatch"]
    assert old["dispatch"] == new["dispatch"] and ws["dispatch"][1] == 0, (old["dispatch"], ws["dispatch"])
    # ... and the loader: interior exactly where the tile holds whole images on such a kernel, never with the switch off
    assert new["interior"] == CASES[case][2] and old["interior"] == 0 and ws["interior"] == 0, (new["interior"], old["interior"], ws["interior"])
    for r in (new, old):      # against fp32 PyTorch on the same operands, as tests/test_pws_gpu.py
        assert r["fwd"] < 4e-3 and r["dgrad"] < 4e-3 and r["acc"] < 8e-3, r
        assert r["sum"] < 1e-4 and r["sumsq"] < 1e-4, r
        assert r["repeat"], r
    assert ws["fwd"] < 4e-3 and ws["dgrad"] < 4e-3, ws
    # same products, same order of additions: identical outputs, whichever loader filled the halo
    for key in ("y_crc", "dx_crc", "y_sha", "dx_sha"):
        assert new[key] == old[key] == ws[key], (key, new[key], old[key], ws[key])
