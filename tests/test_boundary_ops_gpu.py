"""The reference boundary one launch at a time (vpd_amd/csrc/optim.hip: pack_input_kernel<3|5|6|0>, pack_input_px_kernel,
pack_input_rows_kernel<3|5|6>, pack_weights_kernel, unpack_grads_kernel, adamw_kernel, adamw_pack_kernel, zero_ranges_kernel;
conv_wgrad.hip: wgrad_slab_reduce_group_kernel) through the vpd_op_* entry points and the public flat AdamW, in both builds,
against the references of tests/opref.py (pinned without a GPU in tests/test_opref_cpu.py).  The layout operations are exact:
the assertion is EQUALITY OF BITS over the whole over-allocated buffer, which is pre-filled with a sentinel no operation can
produce -- so every element the reference leaves alone must still hold it, the slack behind the buffer included, and every element
it writes must have lost it.  AdamW is held to per-element running-error bounds (opref.adamw_bounds), the slab sums to equality on
integers and to ksplit 2^-24 sum |partials| on randn.  The largest error / bound of every case is printed and dumped."""
import ctypes as C

import pytest
import torch

from tests import opref as R
from tests.test_model_gpu import _dump
from tests.test_ops_gpu import ptr, stream

pytestmark = pytest.mark.gpu
NAMES = ("bf16", "fp16")
SLACK = 256                      # elements behind (and between) the buffers that must keep the sentinel
RATIOS = {}


def _lib(name):
    from vpd_amd._lib import lib
    return lib(name)


def _check(rc, name):
    from vpd_amd._lib import check
    check(rc, "op", name)


def _record(name, key, value):
    RATIOS.setdefault(name, {})[key] = value
    _dump("boundary_ops_%s" % name, RATIOS[name])


def _f32_sentinel(n):
    return torch.full((n,), R.SENTINEL_F32, device="cuda")


def _same_bits(got, want, what):
    """whole-buffer equality of bit patterns (compared on the GPU: the large cases are 200 MB)"""
    g, w = R.bits(got), R.bits(want).to(got.device)
    assert g.shape == w.shape
    if not torch.equal(g, w):
        bad = (g != w).flatten().nonzero().flatten()
        raise AssertionError("%s: %d of %d elements differ, first at %d (got %#x, want %#x)"
                             % (what, bad.numel(), g.numel(), int(bad[0]), int(g.flatten()[bad[0]]) & 0xffffffff,
                                int(w.flatten()[bad[0]]) & 0xffffffff))


# ---------------------------------------------------------------------------
# pack_input
# ---------------------------------------------------------------------------
def _pack_input(name, x, geom, misalign=False):
    n, c, H, W = x.shape
    Hp, Wp, pad = geom
    xbuf = torch.zeros(x.numel() + 4, device="cuda")
    off = 1 if misalign else 0                                  # one float behind a 16-byte boundary: the pixel kernel
    xbuf[off:off + x.numel()] = x.flatten().cuda()
    total = n * Hp * Wp * 8
    out = R.sentinel_elems(total + SLACK, name).cuda()
    _check(_lib(name).vpd_op_pack_input(C.c_void_p(xbuf.data_ptr() + 4 * off), n, c, H, W, ptr(out), Hp, Wp, pad, stream()), name)
    torch.cuda.synchronize()
    ref, written = R.pack_input_ref(x, Hp, Wp, pad, name)
    want = R.bits(R.sentinel_elems(total + SLACK, name)).clone()
    wv = want[:total].view(n, Hp, Wp, 8)
    wv[:, pad:pad + H, pad:pad + W] = R.bits(ref)[:, pad:pad + H, pad:pad + W]
    assert int(written.sum()) == n * H * W
    _same_bits(out, want, "pack_input %s n%d c%d %dx%d pad %d%s" % (name, n, c, H, W, pad, " misaligned" if misalign else ""))


PACK_INPUT_SMALL = ([("rows", s, (3, 5, 6), False) for s in R.PACK_INPUT_ROWS] +
                    [("rows_fallback", s, (3, 5, 6), False) for s in R.PACK_INPUT_ROWS_FALLBACK] +
                    [("quad", s, (3, 5, 6, 1, 4, 8), False) for s in R.PACK_INPUT_QUAD] +
                    [("pixel", s, (3, 5, 6, 1, 8), False) for s in R.PACK_INPUT_PIXEL] +
                    [("misaligned", s, (3, 5, 8), True) for s in R.PACK_INPUT_MISALIGNED])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", PACK_INPUT_SMALL, ids=["%s_n%d_%dx%d" % ((c[0],) + c[1]) for c in PACK_INPUT_SMALL])
def test_pack_input_equals_the_reference_in_bits_on_every_route(case, name):
    route, (n, H, W), channels, misalign = case
    g = torch.Generator().manual_seed(n * 1000 + H * 10 + W)
    for c in channels:
        x = R.pack_input_values((n, c, H, W), name, g)
        for geom in R.pack_input_geoms(H, W):
            _pack_input(name, x, geom, misalign)


BIG = {"below_2p21": (R.PACK_INPUT_BELOW, 0), "workload_2p21": (R.PACK_INPUT_WORKLOAD, 0), "above_2p21": (R.PACK_INPUT_ABOVE, 1)}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("which", list(BIG))
def test_pack_input_at_the_item_count_boundary(which, name):
    """C = 5: just below 2^21 pixel quads (the last items of the float-reciprocal split), the rows kernel at the workload's size, and
    the quad kernel's 64-bit divisions above 2^21"""
    (n, H, W), geo = BIG[which]
    g = torch.Generator().manual_seed(n)
    _pack_input(name, R.pack_input_values((n, 5, H, W), name, g), R.pack_input_geoms(H, W)[geo])


@pytest.mark.parametrize("name", NAMES)
def test_pack_input_refuses_nine_channels(name):
    x = torch.zeros(2 * 9 * 4 * 8 + 4, device="cuda")
    out = R.sentinel_elems(2 * 10 * 16 * 8, name).cuda()
    L = _lib(name)
    assert L.vpd_op_pack_input(ptr(x), 2, 9, 4, 8, ptr(out), 10, 16, 3, stream()) != 0 and b"c outside" in L.vpd_last_error()
    torch.cuda.synchronize()
    assert bool((R.bits(out) == R.SENTINEL_BITS[name]).all())


# ---------------------------------------------------------------------------
# pack_weights / unpack_grads
# ---------------------------------------------------------------------------
def _pack_weights(name, w, stem, with_dgr, off, dgr_first=False):
    Co, Ci, k, _ = w.shape
    mbuf = torch.zeros(w.numel() + 4, device="cuda")
    mbuf[off:off + w.numel()] = w.flatten().cuda()
    fwd, dgr = R.pack_weights_ref(w, name, stem)
    nf = fwd.numel()
    nd = dgr.numel() if with_dgr else 0
    # one buffer: [slack][first layout][slack][second layout][slack], all sentinel
    buf = R.sentinel_elems(3 * SLACK + nf + nd, name).cuda()
    want = R.bits(R.sentinel_elems(3 * SLACK + nf + nd, name)).clone()
    at_f, at_d = (SLACK + nd + SLACK, SLACK) if dgr_first else (SLACK, SLACK + nf + SLACK)
    want[at_f:at_f + nf] = R.bits(fwd).flatten()
    if with_dgr:
        want[at_d:at_d + nd] = R.bits(dgr).flatten()
    es = buf.element_size()
    _check(_lib(name).vpd_op_pack_weights(C.c_void_p(mbuf.data_ptr() + 4 * off), Co, Ci, k, 1 if stem else 0,
                                         C.c_void_p(buf.data_ptr() + es * at_f),
                                         C.c_void_p(buf.data_ptr() + es * at_d) if with_dgr else None, stream()), name)
    torch.cuda.synchronize()
    _same_bits(buf, want, "pack_weights %s %s stem %d dgr %d offset %d" % (name, (Co, Ci, k), stem, with_dgr, off))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", R.PACK_WEIGHTS_CASES, ids=["co%d_ci%d_k%d" % c for c in R.PACK_WEIGHTS_CASES])
def test_pack_weights_both_layouts_equal_the_reference_in_bits(case, name):
    """with and without the data-gradient layout; the master 16-byte aligned (16-byte loads) and 1 and 3 floats off (scalar loads)"""
    Co, Ci, k = case
    g = torch.Generator().manual_seed(Co + Ci + k)
    w = R.pack_input_values((Co, Ci, k, k), name, g)            # ties, zeros, subnormals, fp16 overflow among randn
    for with_dgr in (True, False):
        for off in (0, 1, 3):
            _pack_weights(name, w, False, with_dgr, off, dgr_first=(off == 1))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("ci", R.PACK_STEM_CI)
def test_pack_weights_stem_row_taps(ci, name):
    g = torch.Generator().manual_seed(ci)
    w = R.pack_input_values((64, ci, 7, 7), name, g)
    for off in (0, 1):
        _pack_weights(name, w, True, False, off)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", R.UNPACK_CASES, ids=["co%d_ci%d_k%d_kc%d_stem%d" % c for c in R.UNPACK_CASES])
def test_unpack_grads_inverts_the_scratch_layout(case, name):
    """unpack(pack-layout(x)) == x in bits; the scratch's unused columns hold NaN and must not be read into the result"""
    Co, Ci, k, Kc, stem = case
    g = torch.Generator().manual_seed(Co + Ci + k)
    gr = torch.randn(Co, Ci, k, k, generator=g)
    wg = R.wgrad_scratch_layout(gr, Kc, bool(stem), fill=float("nan"))
    assert torch.equal(R.unpack_grads_ref(wg, Co, Ci, k, Kc, bool(stem)), gr)
    wgd = wg.cuda()
    out = _f32_sentinel(gr.numel() + SLACK)
    _check(_lib(name).vpd_op_unpack_grads(ptr(wgd), Co, Ci, k, Kc, stem, ptr(out), stream()), name)
    torch.cuda.synchronize()
    want = torch.full((gr.numel() + SLACK,), R.SENTINEL_F32)
    want[:gr.numel()] = gr.flatten()
    _same_bits(out, want, "unpack_grads %s %s" % (name, case))


# ---------------------------------------------------------------------------
# AdamW: the flat kernel
# ---------------------------------------------------------------------------
def _scale_state(scale, applied, found=0):
    st = torch.zeros(8, dtype=torch.int32)
    st[0:1] = torch.tensor([scale], dtype=torch.float32).view(torch.int32)
    st[1], st[3] = found, applied
    return st.cuda()


def _flat(name, ins, hp, step, scale=None, found=0):
    """vpd_adamw_step, or vpd_adamw_step_scaled behind a state block (scale, step - 1 applied steps) -> (p, m, v) on the CPU;
    the slack behind every buffer keeps its sentinel"""
    p, g, m, v = ins
    n = p.numel()
    bufs = []
    for t in (p, m, v):
        b = _f32_sentinel(n + SLACK)
        b[:n] = t.cuda()
        bufs.append(b)
    gd = g.cuda()
    L = _lib(name)
    args = (hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"])
    if scale is None:
        _check(L.vpd_adamw_step(ptr(bufs[0]), ptr(gd), ptr(bufs[1]), ptr(bufs[2]), n, *args, step, stream()), name)
    else:
        st = _scale_state(scale, step - 1, found)
        _check(L.vpd_adamw_step_scaled(ptr(bufs[0]), ptr(gd), ptr(bufs[1]), ptr(bufs[2]), n, *args, ptr(st), stream()), name)
    torch.cuda.synchronize()
    out = [b.cpu() for b in bufs]
    for b in out:
        assert bool((b[n:] == R.SENTINEL_F32).all()), "wrote beyond the buffer"
    return [b[:n] for b in out]


def _within_bounds(got, ins, hp, step, gscale=1.0):
    """largest error / bound of (p, m, v); asserts every element inside"""
    ref = R.adamw_ref(*ins, step=step, gscale=gscale, **hp)
    bnd = R.adamw_bounds(*ins, step=step, gscale=gscale, **hp)
    ratios = [float(((a.double() - b).abs() / c).max()) for a, b, c in zip(got, ref, bnd)]
    for what, a, b, c in zip("pmv", got, ref, bnd):
        out = (a.double() - b).abs() > c
        assert not bool(out.any()), "%s: %d of %d elements outside their bound, worst %.3f" % (
            what, int(out.sum()), out.numel(), float(((a.double() - b).abs() / c).max()))
    return ratios


ADAM_REGIMES = [(h, s) for h in R.ADAM_HYPERS for s in R.ADAM_STEPS]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("hyper,step", ADAM_REGIMES)
def test_flat_adamw_within_the_running_error_bounds(hyper, step, name):
    hp = R.ADAM_HYPERS[hyper]
    ins = R.adamw_inputs(R.ADAM_N, step, 1)
    r = _within_bounds(_flat(name, ins, hp, step), ins, hp, step)
    print("adamw %s %s step %d: max error / bound p %.3f m %.3f v %.3f" % ((name, hyper, step) + tuple(r)))
    _record(name, "adamw_flat_%s_step%d" % (hyper, step), r)
    # behind a loss scaler's state block of scale 2^k: gradients k binades up, read x 2^-k; the step number from the block
    k = 3 + step % 11
    p, g, m, v = ins
    r = _within_bounds(_flat(name, (p, g * 2.0 ** k, m, v), hp, step, scale=2.0 ** k), ins, hp, step)
    print("adamw scaled 2^%d %s %s step %d: max error / bound p %.3f m %.3f v %.3f" % ((k, name, hyper, step) + tuple(r)))
    _record(name, "adamw_flat_scaled_%s_step%d" % (hyper, step), r)


@pytest.mark.parametrize("name", NAMES)
def test_flat_adamw_lengths_gradient_scale_and_skipped_step(name):
    hp = R.ADAM_HYPERS["torch"]
    L = _lib(name)
    # 4 floats: one thread; ADAM_LONG: more float4 than one pass of the capped grid (4096 blocks x 256 threads) takes
    for n in (4, R.ADAM_LONG):
        ins = R.adamw_inputs(n, 3, n)
        r = _within_bounds(_flat(name, ins, hp, 3), ins, hp, 3)
        print("adamw %s n %d: max error / bound p %.3f m %.3f v %.3f" % ((name, n) + tuple(r)))
        _record(name, "adamw_flat_n%d" % n, r)
    # a length that is no multiple of 4 is refused and nothing is written
    ins = R.adamw_inputs(4104, 3, 7)
    bufs = [t.cuda() for t in ins]
    for fn, tail in ((L.vpd_adamw_step, (3, stream())), (L.vpd_adamw_step_scaled, (ptr(_scale_state(1.0, 2)), stream()))):
        assert fn(ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), 4102, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], *tail) != 0
        assert b"multiple of 4" in L.vpd_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(R.bits(a.cpu()), R.bits(b)) for a, b in zip(bufs, ins))
    # gscale = 2^-12 on gradients 2^12 up == gscale 1 on the plain gradients, in bits
    ins = R.adamw_inputs(R.ADAM_N, 1000, 5)
    p, g, m, v = ins
    plain = _flat(name, ins, hp, 1000)
    for a, b in zip(plain, _flat(name, (p, g * 4096.0, m, v), hp, 1000, scale=4096.0)):
        # (the block's bias corrections are the device's double pow, the host launch's the C library's: the same floats)
        _same_bits(a, b, "adamw gscale 2^-12")
    # found != 0: the launch writes nothing
    for a, b in zip(_flat(name, ins, hp, 1000, scale=4096.0, found=1), (p, m, v)):
        _same_bits(a, b, "adamw skipped step")


# ---------------------------------------------------------------------------
# AdamW + repack over a synthetic flat buffer
# ---------------------------------------------------------------------------
def _adamw_pack(name, layout, ins, hp, step, wg=None, gscale=1.0):
    """-> (p, m, v) [numel] and the arena (elements) on the CPU, slack checked"""
    dims, offs, numel = layout
    p, g, m, v = ins
    bufs = []
    for t in (p, m, v):
        b = _f32_sentinel(numel + SLACK)
        b[:numel] = t.cuda()
        bufs.append(b)
    gd = g.cuda()
    na = 2 * sum(Co * Ci * k * k for Co, Ci, k in dims)
    arena = R.sentinel_elems(na + SLACK, name).cuda()
    wgd = wg.cuda() if wg is not None else None
    flat_dims = (C.c_int * (3 * len(dims)))(*[x for d in dims for x in d])
    _check(_lib(name).vpd_op_adamw_pack(len(dims), flat_dims, (C.c_longlong * len(offs))(*offs), numel, ptr(bufs[0]), ptr(gd),
                                       ptr(bufs[1]), ptr(bufs[2]), ptr(arena), ptr(wgd) if wgd is not None else None,
                                       hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step, gscale, stream()), name)
    torch.cuda.synchronize()
    out = [b.cpu() for b in bufs]
    for b in out:
        assert bool((b[numel:] == R.SENTINEL_F32).all()), "wrote beyond [0, numel)"          # (e)
    return [b[:numel] for b in out], arena.cpu()


def _arena_ref(layout, p_new, name):
    dims, offs, numel = layout
    na = 2 * sum(Co * Ci * k * k for Co, Ci, k in dims)
    want = R.bits(R.sentinel_elems(na + SLACK, name)).clone()
    at = 0
    for (Co, Ci, k), o in zip(dims, offs):
        ns = Co * Ci * k * k
        fwd, dgr = R.pack_weights_ref(p_new[o:o + ns].view(Co, Ci, k, k), name)
        want[at:at + ns] = R.bits(fwd).flatten()
        want[at + ns:at + 2 * ns] = R.bits(dgr).flatten()
        at += 2 * ns
    return want


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("buf,hyper,step", [("a", "torch", 3), ("b", "strong", 1000)])
def test_adamw_pack_equals_the_flat_kernel_the_reference_and_repacks_what_it_wrote(buf, hyper, step, name):
    layout = R.adam_pack_layout(buf)
    dims, offs, numel = layout
    hp = R.ADAM_HYPERS[hyper]
    ins = R.adamw_inputs(numel, step, 11)
    p, g, m, v = ins
    flat = _flat(name, ins, hp, step)
    got, arena = _adamw_pack(name, layout, ins, hp, step)
    for what, a, b in zip("pmv", got, flat):
        _same_bits(a, b, "(a) %s of adamw_pack vs the flat kernel" % what)
    r = _within_bounds(got, ins, hp, step)                                                  # (b)
    print("adamw_pack %s %s: max error / bound p %.3f m %.3f v %.3f" % ((name, buf) + tuple(r)))
    _record(name, "adamw_pack_%s" % buf, r)
    _same_bits(arena, _arena_ref(layout, got[0], name), "(c) arenas vs pack_weights_ref(new p)")
    # (d) conv gradients from the [tap][Co][Kc] scratch, the OIHW gradient buffer NaN over the convs: the same bits
    g_nan, pieces = g.clone(), []
    for (Co, Ci, k), o in zip(dims, offs):
        ns = Co * Ci * k * k
        pieces.append(R.wgrad_scratch_layout(g[o:o + ns].view(Co, Ci, k, k), Ci).flatten())
        g_nan[o:o + ns] = float("nan")
    got_s, arena_s = _adamw_pack(name, layout, (p, g_nan, m, v), hp, step, wg=torch.cat(pieces))
    for what, a, b in zip("pmv", got_s, got):
        _same_bits(a, b, "(d) %s with the gradients in the scratch" % what)
    _same_bits(arena_s, arena, "(d) arenas with the gradients in the scratch")
    # the gradient factor reaches both paths: 2^-12 on gradients 2^12 up, the same bits
    got_g, arena_g = _adamw_pack(name, layout, (p, g_nan * 4096.0, m, v), hp, step, wg=torch.cat(pieces) * 4096.0, gscale=2.0 ** -12)
    for what, a, b in zip("pmv", got_g, got):
        _same_bits(a, b, "%s with gscale 2^-12" % what)
    _same_bits(arena_g, arena, "arenas with gscale 2^-12")


# ---------------------------------------------------------------------------
# slab sums
# ---------------------------------------------------------------------------
def _reduce(name, slabs):
    """one launch over the [ksplit][n] slabs -> their sums (CPU); every dw has slack that keeps the sentinel"""
    sd = [s.cuda() for s in slabs]
    dws = [_f32_sentinel(s.shape[1] + SLACK) for s in slabs]
    k = len(slabs)
    _check(_lib(name).vpd_op_wgrad_reduce(k, (C.c_void_p * k)(*[t.data_ptr() for t in sd]), (C.c_void_p * k)(*[t.data_ptr() for t in dws]),
                                         (C.c_longlong * k)(*[s.shape[1] for s in slabs]), (C.c_int * k)(*[s.shape[0] for s in slabs]),
                                         stream()), name)
    torch.cuda.synchronize()
    out = []
    for s, d in zip(slabs, dws):
        d = d.cpu()
        assert bool((d[s.shape[1]:] == R.SENTINEL_F32).all()), "wrote beyond dw"
        out.append(d[:s.shape[1]])
    return out


def _check_sums(name, key, shapes, g):
    worst = 0.0
    for integer in (True, False):
        slabs = [R.slab_partials(n, ks, integer, g) for n, ks in shapes]
        for s, got in zip(slabs, _reduce(name, slabs)):
            ref, bound = R.slab_sum_ref(s)
            if integer:
                assert torch.equal(got.double(), ref), "%d of %d sums differ" % (int((got.double() != ref).sum()), ref.numel())
            else:
                err = (got.double() - ref).abs()
                assert bool((err <= bound).all()), float((err / bound).max())
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print("slab sums %s %s: max error / bound %.3f" % (name, key, worst))
    _record(name, "slab_sums_%s" % key, worst)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("ksplit", R.SLAB_KSPLITS)
def test_slab_sums_single_launches(ksplit, name):
    g = torch.Generator().manual_seed(ksplit)
    for n in R.SLAB_LENGTHS:
        _check_sums(name, "k%d_n%d" % (ksplit, n), [(n, ksplit)], g)


@pytest.mark.parametrize("name", NAMES)
def test_slab_sums_grouped_launches(name):
    g = torch.Generator().manual_seed(77)
    _check_sums(name, "group_1_5_33", list(R.SLAB_GROUP), g)              # the thread groups of the widest (16) serve all
    _check_sums(name, "group_17_2_16_3", [(4 * 100, 17), (9 * 64 * 64, 2), (64 * 64, 16), (64 * 64, 3)], g)
    _check_sums(name, "group_of_18", [(4 * (7 + i), 1 + i) for i in range(18)], g)


# ---------------------------------------------------------------------------
# zero_ranges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("count", sorted(R.ZERO_RANGE_CASES))
def test_zero_ranges_zeroes_the_ranges_and_nothing_else(count, name):
    n4s = R.ZERO_RANGE_CASES[count]
    assert len(n4s) == count and 1 in n4s and (count != 3 or max(n4s) > 512 * 256)
    starts, at = [], 8
    for i, n4 in enumerate(n4s):
        starts.append(at)
        at += 4 * n4 + 4 * (1 + i % 3)                                    # 1 .. 3 float4 of sentinel between the ranges
    buf = _f32_sentinel(at + SLACK)
    want = torch.full((at + SLACK,), R.SENTINEL_F32)
    for s, n4 in zip(starts, n4s):
        want[s:s + 4 * n4] = 0.0
    L = _lib(name)
    ptrs = (C.c_void_p * count)(*[buf.data_ptr() + 4 * s for s in starts])
    lens = (C.c_longlong * count)(*n4s)
    _check(L.vpd_op_zero_ranges(ptrs, lens, 0, stream()), name)           # count = 0 launches nothing
    torch.cuda.synchronize()
    assert bool((buf == R.SENTINEL_F32).all())
    _check(L.vpd_op_zero_ranges(ptrs, lens, count, stream()), name)
    torch.cuda.synchronize()
    _same_bits(buf, want, "zero_ranges %s %d" % (name, count))
