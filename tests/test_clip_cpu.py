"""Gradient-norm clipping (vpd_clip_state in include/vpd_hip.h; StudentEngine.enable_grad_clip), the part that needs no GPU: both
libraries export the entry points under ABI 5 and take every refusal on the host, the float64 reference of tests/opref_clip.py
against torch.nn.utils.clip_grad_norm_, the Python arguments and the command line."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from tests import opref_clip as R
from tests.test_abi_cpu import header_functions

NEW = ("vpd_clip_state_bytes", "vpd_op_grad_norm", "vpd_plan_grad_norm")
INF = float("inf")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_both_libraries_export_the_clip_entry_points(dtype):
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    assert h.vpd_abi_version() == _lib.ABI_VERSION == 5
    for n in NEW:
        assert n in header_functions() and n in _lib.SIGNATURES
        assert getattr(h, n).argtypes == _lib.SIGNATURES[n][1]
    assert len(_lib.SIGNATURES["vpd_op_grad_norm"][1]) == 8 and len(_lib.SIGNATURES["vpd_plan_grad_norm"][1]) == 9
    # the struct (64 bytes: the embedded vpd_scale_state + the statistics) and room for the partial sums behind it
    nbytes = h.vpd_clip_state_bytes()
    assert nbytes > 64 and nbytes % 16 == 0


def test_clip_state_layout_in_the_header():
    """The Python layer reads the block as int32 words: eff in 0..7 (vpd_scale_state), total_norm 8, norm_max 9, coef 10,
    clipped_steps 11, nonfinite_steps 12."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vpd_hip.h")).read()
    body = src[src.index("typedef struct vpd_clip_state {"):src.index("} vpd_clip_state;")]
    order = [body.index(k) for k in ("vpd_scale_state eff;", "float total_norm;", "float norm_max;", "float coef;",
                                     "int clipped_steps;", "int nonfinite_steps;", "int reserved[3];")]
    assert order == sorted(order)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_every_refusal_is_taken_on_the_host(dtype):
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    # never dereferenced: every call below is rejected before anything is launched
    x = (C.c_void_p * 3)(64, 132, 200)
    n = (C.c_longlong * 3)(4, 0, 7)
    clip, src = C.c_void_p(4096), C.c_void_p(8192)

    def op(x=x, n=n, count=3, max_norm=1.0, src=None, host_scale=1.0, clip=clip):
        return h.vpd_op_grad_norm(x, n, count, max_norm, src, host_scale, clip, None)

    def refused(rc, msg):
        return rc != 0 and msg in h.vpd_last_error()
    assert refused(op(clip=None), b"null clip state")
    assert refused(op(clip=C.c_void_p(4096 + 8)), b"16-byte aligned")
    assert refused(op(src=C.c_void_p(8194)), b"4-byte aligned")
    for bad in (0.0, -1.0, -INF, float("nan")):
        assert refused(op(max_norm=bad), b"max_norm must be > 0"), bad
    for bad in (0.0, -256.0, INF, float("nan")):
        assert refused(op(host_scale=bad), b"host_scale"), bad
    assert refused(op(x=None), b"null argument") and refused(op(n=None), b"null argument")
    assert refused(op(x=(C.c_void_p * 3)(64, None, 200)), b"null range")
    assert refused(op(n=(C.c_longlong * 3)(4, -1, 7)), b"negative length")
    assert refused(op(count=-1), b"negative count")
    assert refused(op(x=(C.c_void_p * 3)(64, 130, 200)), b"4-byte aligned")

    p = C.c_void_p()
    _lib.check(h.vpd_plan_create(b"resnet18", 5, 64, 64, 32, 0, 4, 1, C.byref(p)), "create", dtype)
    numel = h.vpd_plan_param_numel(p)
    grads, ws = C.c_void_p(1 << 20), C.c_void_p(1 << 30)

    def plan(p=p, grads=grads, numel=numel, max_norm=1.0, src=None, host_scale=1.0, clip=clip, ws=ws):
        return h.vpd_plan_grad_norm(p, grads, numel, max_norm, src, host_scale, clip, ws, None)
    assert refused(plan(p=None), b"null argument") and refused(plan(grads=None), b"null argument")
    assert refused(plan(ws=None), b"null argument") and refused(plan(clip=None), b"null clip state")
    assert refused(plan(), b"workspace not initialised")                  # nothing was bound to this plan
    assert refused(plan(numel=numel + 2), b"multiple of 4") and refused(plan(numel=numel - 4), b"multiple of 4")
    assert refused(plan(clip=C.c_void_p(4096 + 4)), b"16-byte aligned")
    assert refused(plan(src=C.c_void_p(8193)), b"4-byte aligned")
    assert refused(plan(grads=C.c_void_p((1 << 20) + 4)), b"grads must be 16-byte aligned")
    for bad in (0.0, -2.0, float("nan")):
        assert refused(plan(max_norm=bad), b"max_norm must be > 0"), bad
    for bad in (0.0, -1.0, INF, float("nan")):
        assert refused(plan(host_scale=bad), b"host_scale"), bad
    assert refused(plan(src=src, host_scale=0.0), b"workspace not initialised")      # with a source the host scale is not looked at
    h.vpd_plan_destroy(p)


@pytest.mark.parametrize("case", ["binding", "not_binding"])
def test_reference_agrees_with_torch_clip_grad_norm(case):
    """5 fp32 tensors, 4,000 elements in all.  torch sums n squares in fp32: relative (n + 2) * 2^-24 covers its summation, the
    square root and the division."""
    g = torch.Generator().manual_seed(11)
    shapes = [(7, 3, 3, 3), (64,), (1, 1023), (33, 50), (1074,)]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    n = sum(p.numel() for p in params)
    assert n <= 4096
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)
    grads = [p.grad.clone().numpy() for p in params]
    norm = float(np.sqrt(R.sqsum(grads)))
    max_norm = 0.5 * norm if case == "binding" else 2.0 * norm
    ref = R.clip_ref(grads, max_norm)
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    tol = (n + 2) * 2.0 ** -24
    assert abs(total - ref["norm"]) <= tol * ref["norm"]
    if case == "binding":
        assert ref["coef"] < 1.0 and abs(ref["coef"] - 0.5) < 1e-6
    else:
        assert ref["coef"] == 1.0 and ref["eff_scale"] == 1.0
    for p, g0 in zip(params, grads):
        want = g0.astype(np.float64) * ref["coef"]
        assert np.all(np.abs(p.grad.numpy() - want) <= tol * np.abs(want) + 1e-45)
    # the un-scaling rides in the same factor: gradients x 256 behind scale 256 give the same norm and coefficient
    ref256 = R.clip_ref([g0 * np.float32(256.0) for g0 in grads], max_norm, scale=256.0)
    assert ref256["norm"] == ref["norm"] and ref256["coef"] == ref["coef"] and ref256["eff_scale"] == 256.0 / ref["coef"]


def test_reference_edge_cases():
    assert R.clip_ref([np.zeros(5, np.float32)], 1.0)["coef"] == 1.0
    assert R.clip_ref([np.ones(4, np.float32)], INF)["coef"] == 1.0
    big = R.clip_ref([np.full(100, 1e20, np.float32)], 1.0)                # squares overflow fp32, not double
    assert not big["nonfinite"] and big["total_norm_f32"] == np.float32(np.float64(np.float32(1e20)) * 10.0)
    for bad in (INF, -INF, float("nan")):
        r = R.clip_ref([np.array([1.0, bad, 2.0], np.float32)], 1.0)
        assert r["nonfinite"] and r["coef"] == 1.0
    assert R.ulp32(1.0) == 2.0 ** -23


class _Eng:
    """what FusedAdamW touches of an engine before it would enable anything"""
    encoder_numel = 8
    param_numel = 8

    def __init__(self):
        self.params = torch.zeros(8)
        self.enabled = []

    def enable_grad_clip(self, v):
        self.enabled.append(float(v))


def test_fused_adamw_and_get_optimizer_validate_max_grad_norm():
    from vpd_amd.trainer import FusedAdamW, ModelTrainer
    eng = _Eng()
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdamW([torch.nn.Parameter(eng.params[:4])], eng, lr=1e-3, max_grad_norm=bad)
        with pytest.raises(ValueError, match="max_grad_norm"):
            ModelTrainer.get_optimizer(object(), 1e-3, max_grad_norm=bad)
    assert eng.enabled == []
    FusedAdamW([torch.nn.Parameter(eng.params[:4])], eng, lr=1e-3)          # off by default: nothing is enabled
    assert eng.enabled == []
    FusedAdamW([torch.nn.Parameter(eng.params[:4])], eng, lr=1e-3, max_grad_norm=2.5)
    FusedAdamW([torch.nn.Parameter(eng.params[:4])], eng, lr=1e-3, max_grad_norm=INF)
    assert eng.enabled == [2.5, INF]
    sig = inspect.signature(ModelTrainer.get_optimizer).parameters
    assert sig["max_grad_norm"].default is None and sig["loss_scale"].default is None


def test_train_cli_parses_clip_grad_norm(monkeypatch):
    import train_vpd_model
    base = ["train_vpd_model.py", "diving48", "--save_dir", "out"]
    monkeypatch.setattr(sys, "argv", base)
    assert train_vpd_model.get_args().clip_grad_norm is None
    monkeypatch.setattr(sys, "argv", base + ["--clip_grad_norm", "1.5"])
    assert train_vpd_model.get_args().clip_grad_norm == 1.5
    for bad in ("0", "-1", "nan"):
        monkeypatch.setattr(sys, "argv", base + ["--clip_grad_norm", bad])
        with pytest.raises(SystemExit):
            train_vpd_model.get_args()
    assert "clip_grad_norm" in inspect.signature(train_vpd_model.main).parameters
