"""Float64 reference of the weight average (vpd_ema_update, vpd_amd/csrc/optim.hip: ema_update_kernel) and its per-element
running-error bound.  Pinned without a GPU in tests/test_ema_cpu.py; used on the GPU by tests/test_ema_ops_gpu.py and
tests/test_ema_gpu.py.

The update, exactly:  Y' = Y + (1 - d) (S - Y),  d = decay, or with warmup min(decay, (1 + t) / (10 + t)) after t updates.

The kernel computes, in fp32,  y' = fma(omd, s - y, y)  with omd = (float)(1 - d), d in double.  With u = 2^-24:
    omd       = (1 - d) (1 + e0)                      |e0| <= u      (rounding of omd)
    fl(s - y) = (s - y) (1 + e1)                      |e1| <= u      (a floating-point difference never underflows)
    y'        = (omd fl(s - y) + y) (1 + e2) + h      |e2| <= u, |h| <= 2^-150  (one rounding of the fma; h: a subnormal result)
Let B >= |y - Y| be the bound carried in from the updates before.  Then
    y' - Y' = d (y - Y)  +  (1 - d) (s - y) (e0 + e1 + e0 e1)  +  e2 (omd fl(s - y) + y)  +  h
and with |s - y| <= |S - Y| + B (the source is the same fp32 value on both sides) and |y| <= |Y| + B:
    B' = d B + (1 - d) D (2u + u^2) + u ((1 - d) (1 + u)^2 D + |Y| + B) + 2^-150,      D = |S - Y| + B.
Nothing here is fitted to the kernel's output.  The bound itself is evaluated in float64 from the float64 reference; the factor
1 + 2^-30 on it covers that evaluation's own rounding (relative 2^-52 per operation)."""
import torch

U = 2.0 ** -24
SENTINEL = 12345.678          # what the guard bands around every dst are filled with (tests/opref.py: SENTINEL_F32)


def ema_decay(decay, warmup, t):
    """the decay of the update that follows t earlier ones (timm's warmup rule)"""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + t) / (10.0 + t))
    return d


def ema_ref(dst, src, decay, warmup=False, t=0):
    """one update in float64: dst, src any float tensors -> new dst (float64)"""
    d = ema_decay(decay, warmup, t)
    y, s = dst.double(), src.double()
    return y + (1.0 - d) * (s - y)


def ema_bound_step(bound, ref_before, src, decay, warmup=False, t=0):
    """B -> B' of the module docstring: `bound` (float64, >= 0) holds for the state before the update, whose float64 reference is
    `ref_before`; `src` is the update's source"""
    d = ema_decay(decay, warmup, t)
    Y, S = ref_before.double(), src.double()
    D = (S - Y).abs() + bound
    b = d * bound + (1.0 - d) * D * (2.0 * U + U * U) + U * ((1.0 - d) * (1.0 + U) ** 2 * D + Y.abs() + bound) + 2.0 ** -150
    return b * (1.0 + 2.0 ** -30)


def ema_run(dst0, sources, decay, warmup=False, t_first=0):
    """every update of `sources` in turn from dst0 (fp32 values, error 0) -> (float64 reference, running-error bound)"""
    ref = dst0.double()
    bound = torch.zeros_like(ref)
    for k, s in enumerate(sources):
        bound = ema_bound_step(bound, ref, s, decay, warmup, t_first + k)
        ref = ema_ref(ref, s, decay, warmup, t_first + k)
    return ref, bound
