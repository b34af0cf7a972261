"""Dynamic loss scaling (vpd_amd.models.util.DynamicLossScaler, vpd_scale_state in include/vpd_hip.h), the part that needs no GPU:
both libraries export the entry points (ABI 3 onwards; 5 today), host-side argument validation, and the command line."""
import ctypes as C
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vpd_plan_set_scale_state", "vpd_plan_check_grads", "vpd_op_check_finite", "vpd_adamw_step_scaled",
       "vpd_plan_adamw_step_scaled", "vpd_scale_state_update")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_both_libraries_export_the_dynamic_scaling_entry_points(dtype):
    from vpd_amd import _lib
    from vpd_amd.models.util import DynamicLossScaler, LossScaler
    assert issubclass(DynamicLossScaler, LossScaler)
    assert _lib.ABI_VERSION == 5
    h = _lib.lib(dtype)
    assert h.vpd_abi_version() == 5
    for n in NEW:
        assert n in _lib.SIGNATURES and getattr(h, n) is not None
    # the set-state entry point: a NULL plan is an error with a message; NULL state on a plan switches back (host only)
    assert h.vpd_plan_set_scale_state(None, None) != 0 and b"null plan" in h.vpd_last_error()
    p = C.c_void_p()
    _lib.check(h.vpd_plan_create(b"resnet18", 5, 64, 64, 32, 0, 4, 1, C.byref(p)), "create", dtype)
    assert h.vpd_plan_set_scale_state(p, None) == 0
    assert h.vpd_plan_set_scale_state(p, C.c_void_p(6)) != 0 and b"aligned" in h.vpd_last_error()
    assert h.vpd_plan_set_loss_scale(p, 256.0) == 0                     # keeps its meaning and its validation
    assert h.vpd_plan_set_loss_scale(p, float("inf")) != 0
    # host validation of the other entry points (nothing is launched)
    assert h.vpd_op_check_finite(None, 4, None, None) != 0
    assert h.vpd_scale_state_update(None, 2.0, 0.5, 2000, None) != 0
    for growth, backoff, interval in ((0.5, 0.5, 10), (2.0, 0.0, 10), (2.0, 1.5, 10), (2.0, 0.5, 0), (float("nan"), 0.5, 10)):
        assert h.vpd_scale_state_update(C.c_void_p(64), growth, backoff, interval, None) != 0, (growth, backoff, interval)
    assert h.vpd_plan_check_grads(p, None, 0, None, None, None) != 0
    assert h.vpd_plan_adamw_step_scaled(p, None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.01, None, None, None) != 0
    assert h.vpd_adamw_step_scaled(None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.01, None, None) != 0
    h.vpd_plan_destroy(p)


def test_scale_state_layout_in_the_header():
    """The Python scaler builds the block as int32[8] with the scale's bits in element 0, found in 1, tracker 2, applied 3,
    skipped 4: the struct of the header, field for field."""
    src = open(os.path.join(REPO, "include", "vpd_hip.h")).read()
    body = src[src.index("typedef struct vpd_scale_state {"):src.index("} vpd_scale_state;")]
    order = [body.index(k) for k in ("float scale;", "unsigned int found;", "int growth_tracker;", "int applied_steps;",
                                     "int skipped_steps;", "int reserved[3];")]
    assert order == sorted(order)


def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(REPO, "train_vpd_model.py")] + list(args), cwd=REPO,
                          capture_output=True, text=True, timeout=300)


def test_train_cli_lists_loss_scale():
    r = _cli("--help")
    assert r.returncode == 0 and "--loss_scale" in r.stdout and "dynamic" in r.stdout


def test_train_cli_rejects_dynamic_with_bf16_at_argument_parsing(tmp_path):
    out = str(tmp_path / "run")
    for extra in ([], ["--dtype", "bf16"]):
        r = _cli("diving48", "--save_dir", out, "--synthetic", "8", "--loss_scale", "dynamic", *extra)
        assert r.returncode == 2 and "--loss_scale dynamic needs --dtype fp16" in r.stderr, r.stderr
        assert not os.path.exists(out)                                   # rejected before anything ran
    r = _cli("diving48", "--save_dir", out, "--synthetic", "8", "--loss_scale", "sometimes")
    assert r.returncode == 2
