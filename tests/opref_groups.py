"""Helpers of the AdamW parameter-group tests (no device): segment tables over opref.ADAM_PACK_BUFFERS built by rule, the four
groups' hyper-parameters, and the float64 expectation / per-element bound of a grouped step -- opref.adamw_ref / adamw_bounds per
segment with that segment's (lr, wd).  Nothing here involves the code under test."""
import torch

from tests import opref as R

CHUNK = 2048                              # ADAM_PLAIN_CHUNK of optim.hip: the plain-range block of the fused kernel
# (lr, weight_decay) of groups 0..3; the last one holds its parameters still
GROUP_LR_WD = ((5e-4, 0.01), (1e-2, 0.1), (5e-5, 0.0), (0.0, 0.0))
STILL = 3


def segment_table(name):
    """-> (seg_begin [nseg + 1], seg_group [nseg]) over opref.adam_pack_layout(name).  Boundaries: 0 and numel; every conv's begin
    and end (so the 4-float gap of "a" is a segment of its own); in the first gap longer than a chunk, at gap start + 2048 (the
    chunk edge), + 2049 (a one-element segment) and + 2055 (inside a float4).  Groups: round-robin over the four, except that the
    segment behind the first conv takes the first conv's group (two adjacent segments of one group, left unmerged)."""
    dims, offs, numel = R.adam_pack_layout(name)
    cuts = {0, numel}
    convs = []
    for (Co, Ci, k), o in zip(dims, offs):
        convs.append((o, o + Co * Ci * k * k))
        cuts.update(convs[-1])
    ends = [0] + [e for _, e in convs]
    starts = [b for b, _ in convs] + [numel]
    long_gap = next((a for a, b in zip(ends, starts) if b - a > CHUNK))
    cuts.update((long_gap + CHUNK, long_gap + CHUNK + 1, long_gap + CHUNK + 7))
    begin = sorted(cuts)
    group = [i % 4 for i in range(len(begin) - 1)]
    first_conv = begin.index(convs[0][0])
    group[first_conv + 1] = group[first_conv]
    return begin, group


def element_groups(table, numel):
    """int64 [numel]: every element's group"""
    begin, group = table
    out = torch.empty(numel, dtype=torch.int64)
    for s, g in enumerate(group):
        out[begin[s]:begin[s + 1]] = g
    return out


def _per_group(fn, ins, elem_group, lr_wd, shared, step, gscale):
    """fn = adamw_ref | adamw_bounds with every element's own (lr, wd): both are element-wise, so the two hyper-parameters go in as
    float64 tensors -- what fn gives segment by segment with each segment's scalars, in one evaluation (on the operands' device)"""
    table = torch.tensor(lr_wd, dtype=torch.float64, device=elem_group.device)[elem_group]
    return list(fn(*ins, lr=table[:, 0], wd=table[:, 1], b1=shared["b1"], b2=shared["b2"], eps=shared["eps"], step=step, gscale=gscale))


def grouped_ref(ins, elem_group, lr_wd, shared, step, gscale=1.0):
    """float64 (p', m', v') of one grouped AdamW step"""
    return _per_group(R.adamw_ref, ins, elem_group, lr_wd, shared, step, gscale)


def grouped_bounds(ins, elem_group, lr_wd, shared, step, gscale=1.0):
    """per-element bounds of |fp32 kernel - grouped_ref|"""
    return _per_group(R.adamw_bounds, ins, elem_group, lr_wd, shared, step, gscale)


def within(got, ref, bnd):
    """largest error / bound of (p, m, v), and the number of elements outside"""
    ratios = [float(((a.double() - b).abs() / c).max()) for a, b, c in zip(got, ref, bnd)]
    outside = sum(int(((a.double() - b).abs() > c).sum()) for a, b, c in zip(got, ref, bnd))
    return ratios, outside
