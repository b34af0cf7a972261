"""float64 closed forms of FROZEN BatchNorm (running statistics in the batch statistics' place, F.batch_norm(training=False)),
the operand generators and the derived bounds of tests/test_frozen_bn_ops_gpu.py.  Nothing here touches the GPU or the library;
tests/test_frozen_bn_cpu.py holds every closed form equal to torch autograd in float64.

    forward   out = relu?(gamma (z - rm) rstd + beta (+ res)),  rstd = 1 / sqrt(rv + eps)
    backward  g = dy * mask;  dz = gamma rstd g;  dgamma = sum g (z - rm) rstd;  dbeta = sum g
(the batch-mean terms of the train-mode backward are gone: mean and rstd do not depend on z)"""
import torch

from tests import opref as R

F32 = 2.0 ** -24          # half an ulp of fp32, relative


def _v(t):
    return t.double().view(1, -1, 1, 1)


def frozen_params(c, g):
    """running statistics and affine parameters far from both a batch's own statistics and the 0 / 1 defaults:
    rm ~ 0.5 N(0, 1), rv in [0.25, 2], |gamma| in [0.05, 1.5] of either sign, beta in [-1, 1]"""
    rm = 0.5 * torch.randn(c, generator=g)
    rv = 0.25 + 1.75 * torch.rand(c, generator=g)
    gamma, beta = R.stem_params(c, "drift", g)
    return rm, rv, gamma, beta


def rstd_of(rv, eps=R.BN_EPS):
    return (rv.double() + eps).rsqrt()


def forward(z, gamma, beta, rm, rv, res=None, relu=True, eps=R.BN_EPS):
    """float64 pre-activation free form: returns (out, pre) with pre the value in front of the ReLU"""
    pre = _v(gamma) * (z.double() - _v(rm)) * _v(rstd_of(rv, eps)) + _v(beta)
    if res is not None:
        pre = pre + res.double()
    return (pre.clamp_min(0) if relu else pre), pre


def backward(z, gamma, mean, rstd, g):
    """dz, dgamma, dbeta for the masked gradient g; mean / rstd as the forward saved them (running_mean, 1 / sqrt(rv + eps))"""
    g = g.double()
    xhat = (z.double() - _v(mean)) * _v(rstd)
    return _v(gamma) * _v(rstd) * g, (g * xhat).sum(dim=(0, 2, 3)), g.sum(dim=(0, 2, 3))


def backward_pair(zA, gammaA, meanA, rstdA, zB, gammaB, meanB, rstdB, g):
    """two BatchNorms fed by ONE masked gradient (a down-sampling block's last BatchNorm and its 1x1 branch's)"""
    return backward(zA, gammaA, meanA, rstdA, g), backward(zB, gammaB, meanB, rstdB, g)


def pooled_gradient(dpooled, h, w, name):
    """the folded average-pool gradient: dy[b][c][y][x] = elem(dpooled[b][c] / (H W)), float32 values of the element type"""
    n, c = dpooled.shape
    return R.elem_round(dpooled.float() / float(h * w), name).view(n, c, 1, 1).expand(n, c, h, w).contiguous()


# ---- bounds (one ulp of the stored element type on the reference + the fp32 arithmetic of the closed form) ----
def dz_bound(ref_dz, name):
    """dz = fl(fl(gamma rstd) g): the coefficient is rounded once (twice where it is formed in fp32 from two fp32 factors), the
    product once -- at most four half-ulps of fp32 on |dz| -- then the store rounds to the element type"""
    return R.ulp(ref_dz, name) + 4 * F32 * ref_dz.abs()


def out_bound(ref_out, z, gamma, beta, rm, rv, name, res=None, second=None):
    """out = relu(scale z + shift (+ res | + scale2 z2 + shift2)): rstd carries 1 ulp of v_rsq_f32 and the rounding of rv + eps,
    scale one more rounding, shift = fl(beta - fl(mean scale)) two, the apply two per BatchNorm: eight half-ulps of fp32 on the
    magnitudes that enter cover it.  The ReLU does not widen anything: it is 1-Lipschitz."""
    def mags(z_, gamma_, beta_, rm_, rv_):
        sc = (_v(gamma_) * _v(rstd_of(rv_))).abs()
        return z_.double().abs() * sc + _v(rm_).abs() * sc + _v(beta_).abs()
    m = mags(z, gamma, beta, rm, rv)
    if res is not None:
        m = m + res.double().abs()
    if second is not None:
        m = m + mags(*second)
    return R.ulp(ref_out, name) + 8 * F32 * m


def stats_bounds(gamma, beta, rm, rv):
    """per-channel bounds on the stored fp32 vectors against their float64 values: mean is running_mean itself (0); rstd: v_rsq_f32
    is good to 1 ulp and its argument was rounded once -- 4 half-ulps; scale one more; shift two more on its two terms"""
    rs = rstd_of(rv)
    sc = gamma.double() * rs
    return {"mean": torch.zeros_like(rs), "rstd": 4 * F32 * rs, "scale": 6 * F32 * sc.abs(),
            "shift": 8 * F32 * (beta.double().abs() + (rm.double() * sc).abs())}


def case(n, h, w, c, seed, name, relu=True, residual=False):
    """operands of one frozen BatchNorm, forward and backward: element-rounded z (1.3 N(0, 1) - 0.2: its batch mean and variance
    are nowhere near rm / rv), a dy correlated with xhat, a residual when asked; the float64 references; `mean` / `rstd` are what
    the backward entry points get -- the frozen forward's saved vectors, as fp32"""
    g = torch.Generator().manual_seed(seed)
    z = R.elem_round(torch.randn(n, c, h, w, generator=g) * 1.3 - 0.2, name)
    rm, rv, gamma, beta = frozen_params(c, g)
    mean, rstd = rm.clone(), rstd_of(rv).float()
    xhat = (z.double() - _v(mean)) * _v(rstd)
    dy = R.elem_round(torch.randn(n, c, h, w, generator=g) + 0.9 * xhat.float() + 0.3, name)
    res = R.elem_round(torch.randn(n, c, h, w, generator=g), name) if residual else None
    out, pre = forward(z, gamma, beta, rm, rv, res, relu)
    mask = (pre > 0) if relu else torch.ones_like(pre, dtype=torch.bool)
    cs = {"z": z, "dy": dy, "gamma": gamma, "beta": beta, "rm": rm, "rv": rv, "mean": mean, "rstd": rstd, "res": res,
          "out": out, "pre": pre, "act": out, "mask": mask, "gen": g}
    return with_mask(cs, mask)


def with_mask(cs, mask):
    """the case's backward references under `mask` (the kernel's: the sign of the STORED activation, or a recomputed one)"""
    gm = cs["dy"].double() * mask
    dz, dgamma, dbeta = backward(cs["z"], cs["gamma"], cs["mean"], cs["rstd"], gm)
    out = dict(cs)
    out.update(mask=mask, gm=gm, dz=dz, dgamma=dgamma, dbeta=dbeta)
    return out


def sum_bounds(cs, flip=None):
    """2e-5 sum |terms| per channel for dbeta / dgamma (fp32 partials combined in fp64); flip: elements whose recomputed mask an
    fp32 evaluation may legitimately flip, each of which may add or drop its whole term"""
    xhat = (cs["z"].double() - _v(cs["mean"])) * _v(cs["rstd"])
    gm, dy = cs["gm"], cs["dy"].double()
    b1 = R.SUM_TOL * gm.abs().sum(dim=(0, 2, 3))
    b2 = R.SUM_TOL * (gm * xhat).abs().sum(dim=(0, 2, 3))
    if flip is not None:
        b1 = b1 + (dy.abs() * flip).sum(dim=(0, 2, 3))
        b2 = b2 + ((dy * xhat).abs() * flip).sum(dim=(0, 2, 3))
    return b1, b2
