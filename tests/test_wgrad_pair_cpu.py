"""LDS layouts of the pair weight-gradient launch (conv_wgrad_halo_pair_kernel), from the host-only query
vpd_op_wgrad_pair_lds_bytes: a stage is (64 dz rows + the halo's 32-row passes) x 128 B, the branch's dz tiles are two more 8 KB
tiles.  The launcher asks the same function and refuses what it refuses: a compute unit of gfx950 has 160 KB."""
import ctypes as C

import pytest

LDS_CU = 160 * 1024
ROW = 128


def _query(h, dtype, hw, ns):
    b = C.c_longlong(-7)
    rc = h.vpd_op_wgrad_pair_lds_bytes(hw, hw, ns, C.byref(b))
    return rc, b.value


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_boundary_layouts_fit_and_larger_rings_are_refused(dtype):
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    # output 16 x 16 and 8 x 8 (layer2.0, layer3.0): 306 halo pixels, ten passes; 4 x 4 (layer4.0): 400 pixels, thirteen passes
    for hw, passes, own in ((16, 10, None), (8, 10, None), (4, 13, 2)):
        rows = 64 + 32 * passes
        rc, own_bytes = _query(h, dtype, hw, 0)
        assert rc == 0 and 0 < own_bytes <= LDS_CU, (hw, rc, own_bytes)
        if own:
            assert own_bytes == own * rows * ROW + 2 * 8192, (hw, own_bytes)
        else:      # ten passes: three stages + the branch's two tiles (exactly 160 KB), or two stages of everything
            assert own_bytes in (3 * rows * ROW + 2 * 8192, 2 * rows * ROW + 2 * 8192), (hw, own_bytes)
        for ns in (2, 3, 4):
            rc, b = _query(h, dtype, hw, ns)
            assert b == ns * rows * ROW + 2 * 8192, (hw, ns, b)
            assert rc == (0 if b <= LDS_CU else 1), (hw, ns, rc, b)
    assert _query(h, dtype, 16, 3) == (0, 163840) and _query(h, dtype, 16, 2) == (0, 114688)
    assert _query(h, dtype, 4, 2) == (0, 139264)
    assert _query(h, dtype, 4, 3)[0] == 1 and _query(h, dtype, 16, 4)[0] == 1      # 200,704 B and 212,992 B: refused
    # no halo geometry: rows that do not divide a 64-pixel chunk, a halo beyond 416 pixels
    assert h.vpd_op_wgrad_pair_lds_bytes(12, 12, 0, None) == -1
    assert h.vpd_op_wgrad_pair_lds_bytes(2, 2, 0, None) == -1
    assert h.vpd_op_wgrad_pair_lds_bytes(0, 0, 0, None) == -1


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_pair_entry_rejects_bad_arguments_on_the_host(dtype):
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    p = C.c_void_p(64)                                    # never dereferenced: every call below is rejected before a launch
    taps = (C.c_int * 9)(3, 3, 0, 1, 0, 1, 0, 3, 1)
    good = [5, 18, 18, 128, 1, 34, 34, 64, 16, 16, 2, 64, 128]
    assert h.vpd_op_wgrad_pair(p, None, p, p, p, *good, taps, p, p, None) != 0 and b"null argument" in h.vpd_last_error()
    assert h.vpd_op_wgrad_pair(p, p, p, p, p, *good, taps, p, None, None) != 0 and b"null argument" in h.vpd_last_error()
    for pos, bad in ((10, 1), (11, 96), (5, 36), (0, 0)):      # stride 1, Kc not a multiple of 64, input not twice the output, no crops
        args = list(good)
        args[pos] = bad
        assert h.vpd_op_wgrad_pair(p, p, p, p, p, *args, taps, p, p, None) != 0, pos
    assert h.vpd_op_wgrad_pair(p, p, p, p, p, *good, (C.c_int * 9)(1, 1, 1, 1, 1, 1, 0, 1, 1), p, p, None) != 0      # conv1 must be the 3x3
