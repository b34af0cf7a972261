"""The optimizer step's device blocks by name: ctypes mirrors of vpd_scale_state and vpd_clip_state (include/vpd_hip.h).

A block is an int32 tensor (the kernels' own words; a float field holds its bits).  Python indexes it only through `word()` and
moves several fields at once only through `read()` / `write()`; tests/test_state_words_cpu.py holds the mirrors against the header.
A clip block BEGINS with a vpd_scale_state (`eff`: what AdamW and the EMA read), so ScaleState's words address both blocks."""
import ctypes as C

import torch


class ScaleState(C.Structure):
    _fields_ = [("scale", C.c_float), ("found", C.c_uint), ("growth_tracker", C.c_int), ("applied_steps", C.c_int),
                ("skipped_steps", C.c_int), ("reserved", C.c_int * 3)]


class ClipState(C.Structure):
    _fields_ = [("eff", ScaleState), ("total_norm", C.c_float), ("norm_max", C.c_float), ("coef", C.c_float),
                ("clipped_steps", C.c_int), ("nonfinite_steps", C.c_int), ("reserved", C.c_int * 3)]


assert ClipState.eff.offset == 0


def words(struct):
    """int32 words of the struct"""
    return C.sizeof(struct) // 4


def _leading(struct, field):
    """a ClipState also answers for the fields of its leading ScaleState"""
    return struct is ClipState and not hasattr(ClipState, field)


def word(struct, field):
    """index of `field` in a block of int32 words"""
    return getattr(ScaleState if _leading(struct, field) else struct, field).offset // 4


def host_block(struct, nwords=None, **fields):
    """a host int32 tensor of `nwords` (default: the struct's) zero words with `fields` in their places"""
    st = struct()
    for k, v in fields.items():
        setattr(st.eff if _leading(struct, k) else st, k, v)
    out = torch.zeros(words(struct) if nwords is None else nwords, dtype=torch.int32)
    out[:words(struct)] = torch.frombuffer(bytearray(st), dtype=torch.int32)
    return out


def from_words(host, struct):
    """a host int32 tensor that begins with the struct's words, as a `struct` instance: fields by name, floats as floats"""
    return struct.from_buffer_copy(host[:words(struct)].contiguous().numpy().tobytes())


def read(block, struct):
    """ONE .cpu() of the block's leading struct (synchronises), as from_words gives it"""
    return from_words(block[:words(struct)].cpu(), struct)


def write(block, struct, **fields):
    """Write `fields` into a device block from the host: one host image goes to the block's device, then one slice copy per run of
    neighbouring words; the other words are left alone and the host never waits for the device."""
    image = host_block(struct, **fields).to(block.device)
    idx = sorted(word(struct, k) for k in fields)
    while idx:
        n = 1
        while n < len(idx) and idx[n] == idx[0] + n:
            n += 1
        block[idx[0]:idx[0] + n] = image[idx[0]:idx[0] + n]
        idx = idx[n:]
