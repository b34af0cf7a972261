"""float64 reference of the gradient-norm clipping block (include/vpd_hip.h, vpd_clip_state): what clip_finalize_kernel stores, from
the exact sum of squares.  Everything in double; each stored value is rounded to float32 once, in the kernel's order."""
import math

import numpy as np


def sqsum(tensors):
    """sum of squares of every element in float64: a square of a float32 is exact in float64, numpy's pairwise sum adds at most
    log2(n) * 2^-53 relative (nothing for the integer inputs, whose partial sums are exact), math.fsum joins the tensors exactly"""
    out = []
    for t in tensors:
        a = np.asarray(t, dtype=np.float64).ravel()
        with np.errstate(all="ignore"):
            out.append(float(np.sum(a * a)))
    return math.fsum(out) if all(math.isfinite(v) for v in out) else float(np.sum(np.array(out)))


def clip_ref(tensors, max_norm, scale=1.0):
    """-> dict(sum, norm, coef, eff_scale: float64; total_norm_f32, coef_f32, eff_scale_f32: np.float32; nonfinite)"""
    s = sqsum(tensors)
    scale = float(np.float32(scale))
    bad = not math.isfinite(s)
    with np.errstate(all="ignore"):
        norm = float(np.sqrt(np.float64(s)) / np.float64(scale))
        coef = 1.0 if bad else min(1.0, float(np.float64(max_norm) / (np.float64(norm) + np.float64(1e-6))))
        eff = float(np.float64(scale) / np.float64(coef))
        return dict(sum=s, norm=norm, coef=coef, eff_scale=eff, nonfinite=bad, total_norm_f32=np.float32(norm),
                    coef_f32=np.float32(coef), eff_scale_f32=np.float32(eff))


def ulp32(x):
    """one unit in the last place of float32 at |x|"""
    return float(np.spacing(np.float32(abs(x))))
