"""vpd_op_grad_accumulate (vpd_amd/csrc/optim.hip: grad_accum_kernel) alone, in both builds.  The expected result is torch's own
fp32 `dst + src` (add mode) or `src` (store mode): an fp32 add is correctly rounded, so the kernel must give the same BITS.  Every
dst lies between guard bands filled with a sentinel; the whole buffer -- bands included -- is compared, so a write outside a range
fails the test rather than the machine."""
import ctypes as C

import pytest
import torch

from tests.test_ops_gpu import stream

pytestmark = pytest.mark.gpu
NAMES = ("bf16", "fp16")
GUARD = 64                       # floats in front of and behind every dst that must keep the sentinel
SENTINEL = -7.25e30              # no sum of randn values comes near it
GA_MAX = 64                      # range pairs per launch (kernels.h)
# the launcher caps the grid at 2048 blocks and a block takes 16 KB tiles of 1024 float4: with more than 2048 tiles some blocks
# loop; 777 float4 behind the last tile go to the one-float4-per-thread loop, 3 floats to the tail, 3 (offset 1) to the head
LONG_N = 3 + 4 * (1024 * (2048 + 37) + 777) + 3


def _lib(name):
    from vpd_amd._lib import lib
    return lib(name)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Pairs:
    """(dst, src) ranges on the device: dst k lives `dst_off[k]` floats behind GUARD sentinel floats in a 16-byte aligned buffer of
    its own, GUARD more behind it; src k `src_off[k]` floats into another"""

    def __init__(self, dsts, srcs, dst_off, src_off):
        self.n = [int(d.numel()) for d in dsts]
        self.dst_buf, self.src_buf, self.lo, self.so = [], [], [], list(src_off)
        for d, s, do, so in zip(dsts, srcs, dst_off, src_off):
            lo = GUARD + do
            db = torch.full((lo + d.numel() + GUARD,), SENTINEL)
            db[lo:lo + d.numel()] = d
            sb = torch.zeros(s.numel() + 8)
            sb[so:so + s.numel()] = s
            self.dst_buf.append(db.cuda())
            self.src_buf.append(sb.cuda())
            self.lo.append(lo)
        self.want = [b.cpu().clone() for b in self.dst_buf]      # the whole buffers as they must look, kept up to date on the CPU
        self.srcs = [s.clone() for s in srcs]

    def run(self, name, add):
        k = len(self.n)
        dst = (C.c_void_p * k)(*[b.data_ptr() + 4 * lo for b, lo in zip(self.dst_buf, self.lo)])
        src = (C.c_void_p * k)(*[b.data_ptr() + 4 * so for b, so in zip(self.src_buf, self.so)])
        n = (C.c_longlong * k)(*self.n)
        L = _lib(name)
        assert L.vpd_op_grad_accumulate(dst, src, n, k, int(add), stream()) == 0, L.vpd_last_error()
        for w, s, lo, m in zip(self.want, self.srcs, self.lo, self.n):
            w[lo:lo + m] = w[lo:lo + m] + s if add else s      # torch's fp32 add on the CPU: correctly rounded

    def check(self, what):
        torch.cuda.synchronize()
        for k, (b, w) in enumerate(zip(self.dst_buf, self.want)):
            got = b.cpu()
            lo, m = self.lo[k], self.n[k]
            assert torch.equal(_bits(got[:lo]), _bits(w[:lo])), "%s, range %d: wrote in front of dst" % (what, k)
            assert torch.equal(_bits(got[lo + m:]), _bits(w[lo + m:])), "%s, range %d: wrote behind dst" % (what, k)
            bad = int((_bits(got) != _bits(w)).sum())
            assert bad == 0, "%s, range %d (n %d, dst +%d, src +%d): %d elements differ in bits" % (what, k, m, lo - GUARD, self.so[k], bad)


def _randn(lens, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in lens]


def _store_then_add_twice(name, lens, dst_off, src_off, seed):
    """store over NaN (none may survive: the store never reads dst), then two adds, the whole buffers compared after each"""
    p = Pairs([torch.full((n,), float("nan")) for n in lens], _randn(lens, seed), dst_off, src_off)
    p.run(name, add=False)
    p.check("store")
    for k in range(len(lens)):
        assert not bool(torch.isnan(p.want[k]).any())
    for u in range(2):
        fresh = _randn(lens, seed + 1 + u)
        for k, s in enumerate(fresh):
            p.src_buf[k][p.so[k]:p.so[k] + s.numel()] = s.cuda()
            p.srcs[k] = s
        p.run(name, add=True)
        p.check("add %d" % u)


@pytest.mark.parametrize("name", NAMES)
def test_short_ranges_at_every_offset_equal_torch_in_bits(name):
    """lengths 0, 1, 3, 4, 5 and 1027 at start offsets of 0 to 3 floats; src shares dst's 16-byte phase (the 16-byte path) or does
    not (the float-by-float reads of src)"""
    lens = (0, 1, 3, 4, 5, 1027)
    cases = [(n, off) for n in lens for off in range(4)]
    ns, offs = [c[0] for c in cases], [c[1] for c in cases]
    _store_then_add_twice(name, ns, offs, offs, 100)
    _store_then_add_twice(name, ns, offs, [(o + 1 + i) % 4 for i, o in enumerate(offs)], 200)
    _store_then_add_twice(name, (1027,), (0,), (0,), 300)
    _store_then_add_twice(name, (4100, 3), (1, 2), (1, 2), 301)              # one full 16 KB tile + what is left of the middle
    _store_then_add_twice(name, (4100,), (2,), (3,), 302)                    # the same length, phases apart


@pytest.mark.parametrize("name", NAMES)
def test_more_ranges_than_one_launch_takes(name):
    """GA_MAX + 5 ranges of mixed short lengths in ONE call: the second launch takes the last five"""
    lens = [(0, 1, 3, 4, 5, 1027, 260, 17)[i % 8] for i in range(GA_MAX + 5)]
    lens[-1] = 1027
    offs = [i % 4 for i in range(GA_MAX + 5)]
    _store_then_add_twice(name, lens, offs, offs, 400)
    _store_then_add_twice(name, lens, offs, [(o + 1) % 4 for o in offs], 401)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("add", [False, True], ids=["store", "add"])
def test_long_range_runs_tiles_remainder_head_and_tail(name, add):
    """more tiles than blocks of the capped grid (looping blocks), the left-over middle, a 3-float head and a 3-float tail, next to
    a short second range"""
    lens = (LONG_N, 5)
    dsts = [torch.full((n,), float("nan")) for n in lens] if not add else _randn(lens, 500)
    p = Pairs(dsts, _randn(lens, 501), (1, 0), (1, 0))
    p.run(name, add=add)
    p.check("long")
    assert not bool(torch.isnan(p.want[0]).any())


@pytest.mark.parametrize("name", NAMES)
def test_non_finite_values_keep_their_class(name):
    """inf + 1 stays inf, inf + (-inf) is NaN, 3e38 + 3e38 is inf: compared by class, not by NaN payload; the store passes them on"""
    inf = float("inf")
    d = torch.tensor([inf, inf, 3e38, -inf, 1.0, float("nan"), -3e38, 2.0] * 130 + [inf, inf, 3e38])      # 1043 floats: tile-less middle + tail
    s = torch.tensor([1.0, -inf, 3e38, -1.0, inf, 1.0, -3e38, 3.0] * 130 + [1.0, -inf, 3e38])
    for add in (True, False):
        p = Pairs([d], [s], (1,), (1,))
        k = len(p.n)
        dst = (C.c_void_p * k)(p.dst_buf[0].data_ptr() + 4 * p.lo[0])
        src = (C.c_void_p * k)(p.src_buf[0].data_ptr() + 4)
        L = _lib(name)
        assert L.vpd_op_grad_accumulate(dst, src, (C.c_longlong * 1)(d.numel()), 1, int(add), stream()) == 0, L.vpd_last_error()
        torch.cuda.synchronize()
        got = p.dst_buf[0].cpu()[p.lo[0]:p.lo[0] + d.numel()]
        want = d + s if add else s
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(torch.isinf(got), torch.isinf(want))
        fin = torch.isfinite(want)
        assert torch.equal(_bits(got[fin]), _bits(want[fin])) and torch.equal(torch.sign(got[~fin & ~torch.isnan(want)]),
                                                                               torch.sign(want[~fin & ~torch.isnan(want)]))
        if add:
            assert bool(torch.isinf(got[0])) and bool(torch.isnan(got[1])) and bool(torch.isinf(got[2])) and got[2] > 0
