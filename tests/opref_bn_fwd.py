"""float64 closed forms of the TRAIN-mode BatchNorm forward from its accumulator rows, the case generator, the derived bounds and
the launch geometry of tests/test_bn_forward_ops_gpu.py.  Nothing here touches the GPU or the library; tests/test_bn_forward_cpu.py
holds the closed forms equal to F.batch_norm(training=True) in float64, a float32 transcription of the kernels inside the bounds,
and a list of planted faults outside them.

    mu = S1 / M;  var = max(S2 / M - mu^2, 0);  rstd = 1 / sqrt(var + eps);  scale = gamma rstd;  shift = beta - mu scale
    out = relu?(scale z + shift (+ res | + scale2 z2 + shift2))
    rm' = (1 - m) rm + m mu;  rv' = (1 - m) rv + m var M / (M - 1)        (M = 1: the factor is dropped, as the kernels do)

Every per-pixel tensor here is NHWC flattened to [M][C] (M = n H W), which is the kernels' own layout; eps and the momentum are the
float32 values the entry points receive, widened.

Roundings (u = 2^-24, half an ulp of fp32; the fp64 part is carried as e_mu / e_var below and is ~1e-9 of u):
  fused launch, common.h::bn_finalize_channel
    mean  = (float)mu                                         1u on |mu|
    rstd  = v_rsq_f32((float)(var + eps))                     u/2 (the argument's rounding, halved) + 3u: the instruction is taken
                                                              to be within 1 ulp (2u) of the CORRECTLY ROUNDED value (1u)   -> 4u
    scale = fl(gamma rstd)                                    + 1u                                                 -> 5u
    shift = fma(-mean, scale, beta)                           (1 + 4.5)u on |mu scale|, then 1u on |beta| + |mu scale| -> 7u, 1u
  bn_finalize_kernel (fp64 sqrt)
    rstd  = (float)(1 / sqrt(var + eps))                      1u
    scale = fl(gamma rstd)                                    2u
    shift = fl(beta - fl(mean scale))                         (1 + 2 + 1)u on |mu scale|, then 1u on both          -> 5u, 1u
  both
    rm'   = fl(fl(fl(1 - m) rm) + fl(m mean))                 2u on each term, 1u on the sum                       -> 3u
    rv'   = the same with (float)(var M / (M - 1))            3u
  apply (bn_fwd_fused_kernel's loop, bn_apply_kernel), v = fl(fl(z scale) + shift), contracted to one fma or not
    |z scale|: 4.5u (scale) + 1u (product) + 1u (sum)         6.5u        |mu scale|: 6.5u + 1u = 7.5u       |beta|: 1u + 1u = 2u
    + res: one more rounding of the sum, 1u on every term     7.5u / 8.5u / 3u / 1u on |res|
    + the second BatchNorm (res_kind 2): its own 6.5u / 7.5u / 2u, then the sum's 1u on every term
    -> 9u on the magnitudes that enter covers each form; the ReLU is 1-Lipschitz; the store rounds once to the element type:
       half an ulp at the computed value, one ulp at the reference.
  apply from GIVEN fp32 coefficients (vpd_op_bn_apply): product 1u, sum 1u, residual sum 1u                       -> 3u"""
import numpy as np
import torch

from tests import opref as R

F32 = 2.0 ** -24                     # half an ulp of fp32, relative
F64 = 2.0 ** -53
TINY = 2.0 ** -126                   # a flushed fp32 subnormal
EPS = float(np.float32(1e-5))        # what a float argument of 1e-5 is
MOM = float(np.float32(0.1))
FDIV_MAX = 1 << 21
FUSED_ROWS, STAT_ROWS = 4, 16
K_OUT, K_APPLY = 9, 3

# id -> (n, H, W, C) and the path the id names: trips of the busiest thread, grid at its cap of 256, fast index path
CASES = {
    "one_trip_3x9x7": ((3, 9, 7, 64), dict(trips=1, capped=False, fast=True)),
    "one_trip_2x16x16": ((2, 16, 16, 64), dict(trips=1, capped=False, fast=True)),
    "three_trips_capped": ((17, 32, 32, 256), dict(trips=3, capped=True, fast=True)),
    "generic_cv_3": ((3, 9, 7, 24), dict(trips=1, capped=False, fast=False)),
    "generic_cv_12": ((6, 61, 61, 96), dict(trips=2, capped=True, fast=False)),
    "fast_at_the_limit": ((3964, 23, 23, 8), dict(trips=8, capped=True, fast=True)),
    "generic_m": ((33, 256, 256, 8), dict(trips=9, capped=True, fast=False)),
    "wide_2048": ((5, 4, 4, 2048), dict(trips=1, capped=False, fast=True, passes=2)),
    "wide_4096": ((2, 2, 2, 4096), dict(trips=1, capped=False, fast=True, passes=4)),
    "count_one": ((1, 1, 1, 64), dict(trips=1, capped=False, fast=True)),
}
LARGE = ("fast_at_the_limit", "generic_m")          # the two 2M-pixel cases
PLANTED = ("one_trip_3x9x7", "one_trip_2x16x16", "three_trips_capped")
# planted channels (cases in PLANTED)
CH_CONST, CH_CANCEL, CH_FLUSH, CH_NEG = 0, 1, 2, 3


# ---- launch geometry, transcribed from bn.hip ------------------------------------------------------------------------------------
def fused_geometry(M, C):
    """vpd_launch_bn_fwd_fused / bn_fwd_fused_kernel: 1024-thread blocks over items of 8 channels, at most 256 blocks"""
    cv = C // 8
    items = M * cv
    want = (items + 1023) // 1024
    grid = max(1, min(256, want))
    stride = grid * 1024
    return dict(items=items, grid=grid, capped=want >= 256 and grid == 256, stride=stride, trips=-(-items // stride),
                fast=(cv & (cv - 1)) == 0 and M < FDIV_MAX and items < (1 << 31), passes=-(-C // 1024), lds_bytes=16 * C)


def apply_geometry(M, C):
    """vpd_launch_bn_apply / bn_apply_kernel: 256-thread blocks, at most 4096 of them (ew_grid)"""
    items = M * (C // 8)
    want = (items + 255) // 256
    grid = max(1, min(4096, want))
    return dict(items=items, grid=grid, capped=want >= 4096, stride=grid * 256, trips=-(-items // (grid * 256)))


def xcd_r(tile_px, C, grid):
    """vpd_bn_xcd_r"""
    cv = C // 8
    if tile_px <= 0 or grid != 256 or cv <= 0 or 1024 % cv != 0:
        return 0
    pb = 1024 // cv
    if tile_px % pb != 0:
        return 0
    r = tile_px // pb
    return r if 1 <= r <= 32 and 32 % r == 0 else 0


def virtual_block(b, grid, r):
    """vpd_bn_virtual_block"""
    if r <= 0 or grid != 256:
        return b
    x, jj = b & 7, b >> 3
    u, rr = jj // r, jj % r
    return (u * 8 + x) * r + rr


def fdiv(m, d):
    """vpd_fdiv(m, 1.0f / d) on integer arrays: (int)(((float)m + 0.5f) * rcp)"""
    rcp = np.float32(1.0) / np.float32(d)
    return ((m.astype(np.float32) + np.float32(0.5)) * rcp).astype(np.int64)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def row_sums(rows):
    """the rows' totals, added in the kernels' order"""
    s = torch.zeros_like(rows[0])
    for t in range(rows.shape[0]):
        s = s + rows[t]
    return s[0], s[1]


def closed_form(S1, S2, M, gamma, beta, rm=None, rv=None, mom=MOM, eps=EPS):
    mu = S1.double() / M
    var = (S2.double() / M - mu * mu).clamp_min(0)
    rstd = (var + eps).rsqrt()
    scale = gamma.double() * rstd
    out = dict(mean=mu, var=var, rstd=rstd, scale=scale, shift=beta.double() - mu * scale)
    if rm is not None:
        unb = var * M / (M - 1) if M > 1 else var
        out.update(rm=(1 - mom) * rm.double() + mom * mu, rv=(1 - mom) * rv.double() + mom * unb)
    return out


def apply_ref(z, scale, shift, relu, res=None, second=None):
    """[M][C] float64: (out, pre); res [M][C] already at the interior's place; second = (z2, scale2, shift2)"""
    pre = z.double() * scale.double() + shift.double()
    if res is not None:
        pre = pre + res.double()
    if second is not None:
        pre = pre + second[0].double() * second[1].double() + second[2].double()
    return (pre.clamp_min(0) if relu else pre), pre


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
def _fp64_terms(rows, M, mu):
    """what the fp64 sums, the division and E[z^2] - mu^2 can be off by: eight roundings of 2^-53 on the magnitudes that enter"""
    a1, a2 = rows[:, 0].abs().sum(0), rows[:, 1].abs().sum(0)
    return 8 * F64 * a1 / M, 8 * F64 * (a2 / M + 2 * mu.abs() * a1 / M + mu * mu)


def vector_bounds(ref, rows, M, gamma, beta, rm=None, rv=None, kind="fused", mom=MOM, eps=EPS):
    """per-channel bounds on mean / rstd / scale / shift (and rm' / rv'); kind: fused (v_rsq_f32, fma) | finalize (fp64 sqrt)"""
    k_r, k_sc, k_sh = (4, 5, 7) if kind == "fused" else (1, 2, 5)
    e_mu, e_var = _fp64_terms(rows, M, ref["mean"])
    rel_var = e_var / (ref["var"] + eps)
    mu, sc = ref["mean"].abs(), ref["scale"].abs()
    b = dict(mean=F32 * mu + e_mu + TINY,
             rstd=ref["rstd"] * (k_r * F32 + rel_var) + TINY,
             scale=sc * (k_sc * F32 + rel_var) + TINY,
             shift=F32 * beta.double().abs() + mu * sc * (k_sh * F32 + rel_var) + sc * e_mu + TINY)
    if rm is not None:
        unb = ref["var"] * M / (M - 1) if M > 1 else ref["var"]
        fac = M / (M - 1) if M > 1 else 1.0
        b["rm"] = 3 * F32 * ((1 - mom) * rm.double().abs() + mom * mu) + mom * e_mu + TINY
        b["rv"] = 3 * F32 * ((1 - mom) * rv.double().abs() + mom * unb) + mom * fac * e_var + TINY
    return b


def _side_mags(z, ref, beta, rows, M, eps=EPS):
    e_mu, e_var = _fp64_terms(rows, M, ref["mean"])
    sc = ref["scale"].abs()
    zs, ms = z.double().abs() * sc, ref["mean"].abs() * sc
    return zs + ms + beta.double().abs(), (zs + ms) * (e_var / (ref["var"] + eps)) + sc * e_mu


def out_bound(out_ref, name, z, ref, beta, rows, M, res=None, second=None):
    """one ulp of the element type at the reference + 9u (|z||scale| + |mu||scale| + |beta| (+ |res|) (+ the second side's three));
    second = (z2, ref2, beta2, rows2)"""
    m, e = _side_mags(z, ref, beta, rows, M)
    if res is not None:
        m = m + res.double().abs()
    if second is not None:
        m2, e2 = _side_mags(second[0], second[1], second[2], second[3], M)
        m, e = m + m2, e + e2
    return R.ulp(out_ref, name) + K_OUT * F32 * m + e


def apply_bound(out_ref, name, z, scale, shift, res=None, second=None):
    """vpd_op_bn_apply on given fp32 coefficients: one ulp + 3u on the magnitudes; second = (z2, rscale, rshift)"""
    m = z.double().abs() * scale.double().abs() + shift.double().abs()
    if res is not None:
        m = m + res.double().abs()
    if second is not None:
        m = m + second[0].double().abs() * second[1].double().abs() + second[2].double().abs()
    return R.ulp(out_ref, name) + K_APPLY * F32 * m


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def uneven_rows(S1, S2, nrows):
    """[nrows][2][C] float64 whose totals are (S1, S2), spread unevenly; one pair of rows holds +K and (its share) - K with K a few
    times the total: a launch that reads fewer than all rows, or other rows, is far off"""
    w = torch.tensor([(t % 5 + 1.0) * (1.5 if t & 1 else 0.5) for t in range(nrows)], dtype=torch.float64)
    w = w / w.sum()
    rows = torch.stack([torch.stack([S1 * f, S2 * f]) for f in w])
    rows[nrows - 1] = torch.stack([S1, S2]) - rows[:nrows - 1].sum(0)
    K = 3.0 * torch.stack([S1, S2]).abs() + 1.0
    rows[1] = rows[1] + K
    rows[nrows - 1] = rows[nrows - 1] - K
    return rows.contiguous()


def _side(M, c, g, name, planted, relu):
    z = torch.randn(M, c, generator=g) * 1.3 - 0.2
    if planted and M > 1:
        z[:, CH_CONST] = 0.75
        z[:, CH_CANCEL] = 40.0 + 0.25 * (torch.rand(M, generator=g) < 0.5).float()
    z = R.elem_round(z, name)
    gamma, beta = R.stem_params(c, "drift", g)
    if planted:
        gamma[CH_FLUSH], beta[CH_FLUSH] = 0.0, (1e-9 if relu else -1e-9)
        gamma[CH_NEG] = -0.8
    rm, rv = 0.5 * torch.randn(c, generator=g), 0.25 + 1.75 * torch.rand(c, generator=g)
    zd = z.double()
    S1, S2 = zd.sum(0), (zd * zd).sum(0)
    del zd
    rows, rows16 = uneven_rows(S1, S2, FUSED_ROWS), uneven_rows(S1, S2, STAT_ROWS)
    S1, S2 = row_sums(rows)
    return dict(z=z, gamma=gamma, beta=beta, rm=rm, rv=rv, rows=rows, rows16=rows16, S1=S1, S2=S2,
                ref=closed_form(S1, S2, M, gamma, beta, rm, rv))


def case(cid, name, relu=True, residual=False, second=False, seed=0):
    """operands and references of one launch: element-rounded z [M][C] (1.3 N(0, 1) - 0.2, with the planted channels), gamma of
    either sign, rm / rv away from 0 / 1, the uneven rows, res [n][H][W][C] or a second BatchNorm `b2`; out / pre float64"""
    shape = CASES[cid][0] if isinstance(cid, str) else cid
    n, h, w, c = shape
    M = n * h * w
    g = torch.Generator().manual_seed(1000 * n + 7 * h + c + 131 * relu + 17 * residual + 29 * second + seed)
    planted = cid in PLANTED
    cs = _side(M, c, g, name, planted, relu)
    cs.update(shape=shape, M=M, name=name, relu=relu, planted=planted, res=None, b2=None)
    sec = None
    if residual:
        cs["res"] = R.elem_round(torch.randn(n, h, w, c, generator=g), name)
    if second:
        cs["b2"] = _side(M, c, g, name, False, relu)
        sec = (cs["b2"]["z"], cs["b2"]["ref"]["scale"], cs["b2"]["ref"]["shift"])
    cs["out"], cs["pre"] = apply_ref(cs["z"], cs["ref"]["scale"], cs["ref"]["shift"], relu,
                                     cs["res"].view(M, c) if residual else None, sec)
    return cs


def case_out_bound(cs, out_ref=None):
    b2 = cs["b2"]
    return out_bound(cs["out"] if out_ref is None else out_ref, cs["name"], cs["z"], cs["ref"], cs["beta"], cs["rows"], cs["M"],
                     res=cs["res"].view(cs["M"], -1) if cs["res"] is not None else None,
                     second=(b2["z"], b2["ref"], b2["beta"], b2["rows"]) if b2 else None)


def stored_mask(out, name):
    """the bit map's definition: the STORED element is > 0"""
    return R.elem_round(out.float(), name) > 0


# ---- float32 transcription of the kernels (numpy) -------------------------------------------------------------------------------
def _f32(t):
    return t.detach().cpu().numpy().astype(np.float32)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two fp32 values is exact in fp64; the fp64 sum's own rounding is 2^-29 of fp32's"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def transcribe_vectors(rows, M, gamma, beta, rm, rv, kind, rsq_ulps=0, contract=False, mom=MOM, eps=EPS):
    """bn_finalize_channel + the fused kernel's running update (kind fused; rsq_ulps moves v_rsq_f32's result by that many ulps),
    or bn_finalize_kernel (kind finalize; contract: beta - mean scale as one fma).  float32 numpy arrays."""
    r64 = rows.numpy()
    s1, s2 = np.zeros_like(r64[0, 0]), np.zeros_like(r64[0, 1])
    for t in range(r64.shape[0]):
        s1, s2 = s1 + r64[t, 0], s2 + r64[t, 1]
    count = float(np.float32(M))
    ga, be, eps32, m32 = _f32(gamma), _f32(beta), np.float32(eps), np.float32(mom)
    if kind == "fused":
        inv = 1.0 / count
        mu = s1 * inv
        var = np.maximum(s2 * inv - mu * mu, 0.0)
        arg = (var + float(eps32)).astype(np.float32)
        r = (1.0 / np.sqrt(arg.astype(np.float64))).astype(np.float32)
        for _ in range(abs(rsq_ulps)):
            r = np.nextafter(r, np.float32(np.inf if rsq_ulps > 0 else 0.0))
        sc = ga * r
        mu32 = mu.astype(np.float32)
        sh = _fma32(-mu32, sc, be)
    else:
        mu = s1 / count
        var = np.maximum(s2 / count - mu * mu, 0.0)
        r = (1.0 / np.sqrt(var + float(eps32))).astype(np.float32)
        sc = ga * r
        mu32 = mu.astype(np.float32)
        sh = _fma32(-mu32, sc, be) if contract else be - mu32 * sc
    out = dict(mean=mu32, rstd=r, scale=sc, shift=sh)
    if rm is not None:
        unb = (var * count / (count - 1.0) if count > 1.0 else var).astype(np.float32)
        one_m = np.float32(1.0) - m32
        if contract:
            out["rm"], out["rv"] = _fma32(one_m, _f32(rm), m32 * mu32), _fma32(one_m, _f32(rv), m32 * unb)
        else:
            out["rm"], out["rv"] = one_m * _f32(rm) + m32 * mu32, one_m * _f32(rv) + m32 * unb
    return out


def transcribe_apply(z, sc, sh, relu, name, res=None, second=None, contract=False):
    """the apply loop on float32 numpy coefficient vectors; returns the stored values as a float64 torch tensor [M][C]"""
    zz = _f32(z)
    v = _fma32(zz, sc, sh) if contract else zz * sc + sh
    if res is not None:
        v = v + _f32(res)
    if second is not None:
        z2 = _f32(second[0])
        v = v + (_fma32(z2, second[1], second[2]) if contract else z2 * second[1] + second[2])
    if relu:
        v = np.where(v > 0, v, np.float32(0.0))
    return R.elem_round(torch.from_numpy(v), name).double()


def ratio(got, want, bound):
    return float(((torch.as_tensor(got).double() - want).abs() / bound).max())


# every fused launch of tests/test_bn_forward_ops_gpu.py: (case id, relu, residual, second BatchNorm)
LAUNCHES = [(cid, 1, 0, 0) for cid in CASES]
LAUNCHES += [(cid, 1, 1, 0) for cid in PLANTED] + [(cid, 0, 0, 0) for cid in PLANTED[:2]]
LAUNCHES += [(cid, 1, 0, 1) for cid in ("one_trip_3x9x7", "three_trips_capped", "wide_4096")]


def launch_id(launch):
    cid, relu, residual, second = launch
    return cid + ("" if relu else "-norelu") + ("-residual" if residual else "") + ("-two" if second else "")
