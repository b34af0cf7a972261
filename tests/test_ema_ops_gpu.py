"""vpd_ema_update (vpd_amd/csrc/optim.hip: ema_update_kernel) alone, in both builds, against the float64 reference and the derived
running-error bound of tests/opref_ema.py.  Every dst lies between guard bands filled with a sentinel no update can produce; the
whole buffer -- bands included -- is compared, so a write outside a range fails the test rather than the machine."""
import ctypes as C

import pytest
import torch

from tests import opref_ema as E
from tests.test_ops_gpu import ptr, stream

pytestmark = pytest.mark.gpu
NAMES = ("bf16", "fp16")
GUARD = 64                       # floats in front of and behind every dst that must keep the sentinel
# the launcher caps the grid at 2048 blocks and a block takes 16 KB tiles of 1024 float4: with more than 2048 tiles some blocks
# loop; 777 float4 behind the last tile go to the one-float4-per-thread loop, 3 floats to the tail, 3 (offset 1) to the head
LONG_N = 3 + 4 * (1024 * (2048 + 37) + 777) + 3


def _lib(name):
    from vpd_amd._lib import lib
    return lib(name)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _state(found, applied):
    st = torch.zeros(8, dtype=torch.int32)
    st.view(torch.float32)[0] = 256.0
    st[1], st[3] = found, applied
    return st.cuda()


class Ranges:
    """up to four (src, dst) ranges on the device; dst k lives at `dst_off[k]` floats into a 16-byte aligned buffer of its own,
    GUARD sentinel floats on either side, src k at `src_off[k]` floats into another"""

    def __init__(self, srcs, dsts, src_off, dst_off):
        self.n = [int(d.numel()) for d in dsts]
        self.src_buf, self.dst_buf, self.lo = [], [], []
        for s, d, so, do in zip(srcs, dsts, src_off, dst_off):
            sb = torch.zeros(s.numel() + 8, device="cuda")
            sb[so:so + s.numel()] = s.cuda()
            lo = 4 * (GUARD // 4) + do
            db = torch.full((lo + d.numel() + GUARD,), E.SENTINEL, device="cuda")
            db[lo:lo + d.numel()] = d.cuda()
            self.src_buf.append((sb, so))
            self.dst_buf.append(db)
            self.lo.append(lo)

    def set_src(self, k, s):
        sb, so = self.src_buf[k]
        sb[so:so + s.numel()] = s.cuda()

    def update(self, name, decay, warmup=0, t=0, t0=0, state=None):
        k = len(self.n)
        src = (C.c_void_p * k)(*[sb.data_ptr() + 4 * so for sb, so in self.src_buf])
        dst = (C.c_void_p * k)(*[db.data_ptr() + 4 * lo for db, lo in zip(self.dst_buf, self.lo)])
        n = (C.c_longlong * k)(*self.n)
        L = _lib(name)
        rc = L.vpd_ema_update(src, dst, n, k, decay, warmup, t, t0, ptr(state) if state is not None else None, stream())
        assert rc == 0, L.vpd_last_error()

    def dst(self, k):
        """dst k on the CPU, after checking that both guard bands still hold the sentinel"""
        torch.cuda.synchronize()
        b = self.dst_buf[k].cpu()
        lo, n = self.lo[k], self.n[k]
        assert bool((b[:lo] == E.SENTINEL).all()), "range %d: wrote in front of dst" % k
        assert bool((b[lo + n:] == E.SENTINEL).all()), "range %d: wrote behind dst" % k
        return b[lo:lo + n].clone()

    def whole(self, k):
        torch.cuda.synchronize()
        return self.dst_buf[k].cpu()


def _even_ints(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (2 * torch.randint(-2047, 2048, (n,), generator=g)).float()      # even, |x| <= 4094 < 2^12


def _exact_four_updates(name, lens, src_off, dst_off, seed):
    """decay 0.5 on even integers below 2^12, four updates: every difference, product and sum is exact in fp32 (after k updates
    the values are multiples of 2^(1-k) below 2^12), so the kernel must equal the float64 reference in every bit"""
    dsts = [_even_ints(n, seed + 10 * k) for k, n in enumerate(lens)]
    srcs = [[_even_ints(n, seed + 10 * k + u + 1) for u in range(4)] for k, n in enumerate(lens)]
    r = Ranges([s[0] for s in srcs], dsts, src_off, dst_off)
    ref = [d.double() for d in dsts]
    for u in range(4):
        for k in range(len(lens)):
            r.set_src(k, srcs[k][u])
            ref[k] = E.ema_ref(ref[k], srcs[k][u], 0.5)
        r.update(name, 0.5, t=u)
    for k in range(len(lens)):
        got = r.dst(k)
        want = ref[k].float()
        assert torch.equal(want.double(), ref[k])                            # the reference itself is exact in fp32
        assert torch.equal(_bits(got), _bits(want)), "range %d (n %d, src +%d, dst +%d): %d elements differ" % (
            k, lens[k], src_off[k], dst_off[k], int((_bits(got) != _bits(want)).sum()))


@pytest.mark.parametrize("name", NAMES)
def test_short_ranges_at_every_offset_are_exact_and_stay_inside(name):
    """lengths 0, 1, 3, 4, 5 and 1027 at start offsets of 0 to 3 floats, four ranges per launch; src and dst of a range share the
    offset (the 16-byte path) or differ in it (the float-by-float reads of src)"""
    lens = (0, 1, 3, 4, 5, 1027)
    cases = [(n, off) for n in lens for off in range(4)]                    # 24 (length, offset) pairs, four per launch
    for j in range(0, len(cases), 4):
        four = cases[j:j + 4]
        ns, offs = [c[0] for c in four], [c[1] for c in four]
        _exact_four_updates(name, ns, offs, offs, 100 + j)
        _exact_four_updates(name, ns, [(o + 1 + i) % 4 for i, o in enumerate(offs)], offs, 200 + j)
    # mixed lengths in one launch, and fewer than four ranges
    _exact_four_updates(name, (1027, 0, 5, 1), (3, 0, 2, 1), (3, 0, 2, 1), 300)
    _exact_four_updates(name, (1027,), (0,), (0,), 301)
    _exact_four_updates(name, (4100, 3), (1, 2), (1, 2), 302)               # one full 16 KB tile + what is left of the middle


@pytest.mark.parametrize("name", NAMES)
def test_long_range_runs_tiles_remainder_head_and_tail(name):
    """more tiles than blocks of the capped grid, a partial tile, a 3-float head and a 3-float tail, next to a short second range"""
    _exact_four_updates(name, (LONG_N, 5), (1, 0), (1, 0), 400)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("warmup", [0, 1])
def test_randn_fifty_updates_within_the_running_error_bound(name, warmup):
    g = torch.Generator().manual_seed(7 + warmup)
    lens, offs = (4099, 1027, 5), (1, 2, 0)
    dsts = [torch.randn(n, generator=g) for n in lens]
    r = Ranges(dsts, dsts, offs, offs)
    sources = [[] for _ in lens]
    for u in range(50):
        for k, n in enumerate(lens):
            s = torch.randn(n, generator=g) * (1.0 + 0.1 * u)
            sources[k].append(s)
            r.set_src(k, s)
        r.update(name, 0.999, warmup=warmup, t=u)
    worst = 0.0
    for k in range(len(lens)):
        ref, bound = E.ema_run(dsts[k], sources[k], 0.999, bool(warmup))
        err = (r.dst(k).double() - ref).abs()
        assert bool((bound > 0).all())
        out = err > bound
        assert not bool(out.any()), "range %d: %d of %d elements outside their bound, worst %.3f" % (
            k, int(out.sum()), out.numel(), float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    print("ema %s warmup %d, 50 updates: largest error / bound %.3f" % (name, warmup, worst))


@pytest.mark.parametrize("name", NAMES)
def test_state_block_skips_and_counts(name):
    g = torch.Generator().manual_seed(11)
    lens, offs = (1027, 4100, 3), (1, 0, 3)
    dsts = [torch.randn(n, generator=g) for n in lens]
    srcs = [torch.randn(n, generator=g) for n in lens]
    # found = 1: nothing is written, guard bands and dst alike
    r = Ranges(srcs, dsts, offs, offs)
    before = [r.whole(k).clone() for k in range(len(lens))]
    r.update(name, 0.9, warmup=1, t=0, t0=2, state=_state(1, 7))
    for k in range(len(lens)):
        assert torch.equal(_bits(r.whole(k)), _bits(before[k])), "range %d was written under found = 1" % k
    # found = 0, applied_steps 7, t0 2, warmup: t = 5 whatever the caller's t says
    r.update(name, 0.9, warmup=1, t=0, t0=2, state=_state(0, 7))
    plain = Ranges(srcs, dsts, offs, offs)
    plain.update(name, 0.9, warmup=1, t=5)
    other = Ranges(srcs, dsts, offs, offs)
    other.update(name, 0.9, warmup=1, t=0)
    for k in range(len(lens)):
        a, b = r.dst(k), plain.dst(k)
        assert torch.equal(_bits(a), _bits(b)), "range %d: the block's t is not applied_steps - t0" % k
        assert not torch.equal(a, dsts[k])
        if lens[k] > 3:
            assert not torch.equal(a, other.dst(k))                          # (t = 0 gives d = 0.1, t = 5 gives 0.4)
        ref, bound = E.ema_run(dsts[k], [srcs[k]], 0.9, True, 5)
        assert bool(((a.double() - ref).abs() <= bound).all())
