"""vpd_amd.state_words against include/vpd_hip.h: the ctypes mirrors of vpd_scale_state and vpd_clip_state have the header's fields,
in its order, with its 4-byte types, and fit the block the library asks for.  The header is parsed here, as tests/test_abi_cpu.py
parses its functions."""
import ctypes as C
import os
import re

import torch

from vpd_amd import state_words as W

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vpd_hip.h")
CTYPES = {"float": C.c_float, "unsigned int": C.c_uint, "int": C.c_int, "vpd_scale_state": W.ScaleState}


def header_struct(name):
    """[(field, ctypes type)] of `typedef struct name { ... } name;`, comments stripped, `int x[3]` as c_int * 3"""
    src = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, field, count = re.fullmatch(r"([a-z_ ]+?)\s+(\w+)(?:\[(\d+)\])?", decl).groups()
        fields.append((field, CTYPES[ctype] * int(count) if count else CTYPES[ctype]))
    return fields


def test_the_mirrors_have_the_headers_fields_in_order_with_4_byte_types():
    for name, mirror in (("vpd_scale_state", W.ScaleState), ("vpd_clip_state", W.ClipState)):
        want = header_struct(name)
        assert len(want) >= 6
        assert [(f, t) for f, t in mirror._fields_] == want, name
        for f, t in mirror._fields_:
            assert C.sizeof(t) % 4 == 0 and getattr(mirror, f).offset % 4 == 0, (name, f)
        assert C.sizeof(mirror) == sum(C.sizeof(t) for _, t in want), name      # no padding: every field is its own words
    assert C.sizeof(W.ScaleState) == 32 and W.words(W.ScaleState) == 8


def test_the_clip_mirror_fits_the_block_the_library_asks_for():
    from vpd_amd import _lib
    for dtype in ("bf16", "fp16"):
        assert C.sizeof(W.ClipState) <= _lib.lib(dtype).vpd_clip_state_bytes()      # (a host-only call)


def test_word_indices_and_the_host_round_trip():
    # the indices the tests and the kernels' documentation use, derived from the mirrors
    assert [W.word(W.ScaleState, f) for f in ("scale", "found", "growth_tracker", "applied_steps", "skipped_steps")] == [0, 1, 2, 3, 4]
    assert [W.word(W.ClipState, f) for f in ("applied_steps", "total_norm", "norm_max", "coef", "clipped_steps", "nonfinite_steps")] \
        == [3, 8, 9, 10, 11, 12]
    block = torch.arange(100, 124, dtype=torch.int32)      # a clip block with its partial sums behind the struct
    W.write(block, W.ClipState, norm_max=7.5, applied_steps=9, clipped_steps=3, nonfinite_steps=1)
    want = torch.arange(100, 124, dtype=torch.int32)
    want[3], want[11], want[12] = 9, 3, 1
    want[9:10] = torch.tensor([7.5]).view(torch.int32)
    assert torch.equal(block, want)                        # the named words and no other
    h = W.read(block, W.ClipState)
    assert (h.eff.applied_steps, h.norm_max, h.clipped_steps, h.nonfinite_steps) == (9, 7.5, 3, 1)
    host = W.host_block(W.ScaleState, scale=512.0, applied_steps=6)
    assert host.dtype == torch.int32 and host.tolist() == [torch.tensor([512.0]).view(torch.int32).item(), 0, 0, 6, 0, 0, 0, 0]
    assert W.from_words(host, W.ScaleState).scale == 512.0
