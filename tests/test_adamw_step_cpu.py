"""StudentEngine.adamw_step, the part that needs no GPU and no native library: which entry points it calls, in which order and with
which state block, along its two axes -- path (the fused pass over the last backward's train plan / the flat buffers) and mode
(no device state / a DynamicLossScaler's block in flight / the clip block).  The library is a stub that records every call."""
import pytest
import torch

from tests.engine_stub import BN_NUMEL, NUMEL, stub_engine

HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.01)      # lr, beta1, beta2, eps, weight_decay as adamw_step passes them on


def _engine(path, mode, ema):
    # the plan: current for the fused path ("fused_small": built without the motion head, fewer parameters than the buffers)
    eng = stub_engine(None if path == "flat_no_plan" else NUMEL - 8 if path == "fused_small" else NUMEL)
    eng.scale_state = torch.zeros(8, dtype=torch.int32) if mode == "scaler" or mode == "clip+scaler" else None
    eng._clip = torch.zeros(24, dtype=torch.int32) if mode.startswith("clip") else None
    eng._clip_max_norm = 2.5 if eng._clip is not None else None
    if eng.scale_state is not None:
        eng._dyn_state = eng.scale_state
    elif eng._clip is not None:
        eng._dyn_state = eng._clip
    if eng._dyn_state is not None:
        eng._dyn_state[3] = 6
    if ema:
        eng._ema = (0.99, False)
        eng.ema_params, eng.ema_bn_running = torch.zeros(NUMEL), torch.zeros(BN_NUMEL)
    return eng


def _run(monkeypatch, path, mode, ema=False):
    monkeypatch.setenv("VPD_FUSED_ADAMW", "0" if path == "flat_env" else "1")
    eng = _engine(path, mode, ema)
    pl = eng._step_plan
    packed0 = None if pl is None else pl.packed_version
    numel = NUMEL - 8 if path == "flat_short" else None      # an optimizer that was not given the plan's last tensors
    eng.adamw_step(HYPER[0], (HYPER[1], HYPER[2]), HYPER[3], HYPER[4], numel=numel)
    calls = [c for c in eng.L.calls if c[0] != "vpd_plan_grads_pending"]
    return eng, pl, packed0, calls, NUMEL if numel is None else numel


FUSED = ("fused", "fused_small")
FLAT = ("flat_no_plan", "flat_short", "flat_env")
MODES = ("none", "scaler", "clip", "clip+scaler")


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", FUSED + FLAT)
def test_adamw_step_launch_sequence(monkeypatch, path, mode, ema):
    eng, pl, packed0, calls, numel = _run(monkeypatch, path, mode, ema)
    st, clip = eng.scale_state, eng._clip
    state = clip if clip is not None else st      # the block the AdamW and the EMA read
    fused = path in FUSED
    base = (_ptr(eng.params), _ptr(eng._grads), _ptr(eng.adam_m), _ptr(eng.adam_v), numel) + HYPER
    want = []
    if fused:
        assert numel == max(numel, pl.param_numel)
        ws = _ptr(pl.workspace)
        h = pl.handle.value
        if clip is not None:
            want.append(("vpd_plan_grad_norm", (h, _ptr(eng._grads), numel, 2.5, _ptr(st), 1.0, _ptr(clip), ws, None)))
        elif st is not None:
            want.append(("vpd_plan_check_grads", (h, _ptr(eng._grads), numel, _ptr(st), ws, None)))
        if state is not None:
            want.append(("vpd_plan_adamw_step_scaled", (h,) + base + (_ptr(state), ws, None)))
        else:
            want.append(("vpd_plan_adamw_step", (h,) + base + (7, ws, None)))      # previous adam_step + 1
    else:
        if clip is not None:
            got = calls[0]
            assert got[0] == "vpd_op_grad_norm"
            x, n = got[1][0], got[1][1]
            assert list(x) == [_ptr(eng._grads)] and list(n) == [numel]
            assert got[1][2:] == (1, 2.5, _ptr(st), 1.0, _ptr(clip), None)
            want.append(got)
        elif st is not None:
            want.append(("vpd_op_check_finite", (_ptr(eng._grads), numel, _ptr(st), None)))
        if state is not None:
            want.append(("vpd_adamw_step_scaled", base + (_ptr(state), None)))
        else:
            want.append(("vpd_adamw_step", base + (7, None)))      # the host step
    if ema:
        got = calls[len(want)]
        assert got[0] == "vpd_ema_update"
        assert list(got[1][0]) == [_ptr(eng.params), _ptr(eng.bn_running)]
        assert list(got[1][1]) == [_ptr(eng.ema_params), _ptr(eng.ema_bn_running)]
        assert list(got[1][2]) == [NUMEL, 8]
        assert got[1][3:] == (2, 0.99, 0, 0, 0, _ptr(state), None)
        want.append(got)
    if clip is not None and st is None:
        want.append(("vpd_scale_state_update", (_ptr(clip), 1.0, 1.0, 2 ** 31 - 1, None)))
    assert [c[0] for c in calls] == [w[0] for w in want]
    assert calls == want
    # the host step counter advances only without a device block; the device blocks are not written from the host
    assert eng._adam_step == (7 if mode == "none" else 6)
    if eng._dyn_state is not None:
        assert int(eng._dyn_state[3]) == 6
    assert eng._hip_version == 4
    assert eng._ema_t == (1 if ema and state is None else 0) and eng._ema_version == (1 if ema else 0)
    if pl is not None:
        if fused:
            assert pl.packed_version == eng.weights_version() and pl.packed_version != packed0
        else:
            assert pl.packed_version is packed0


def test_fused_path_needs_current_packed_weights(monkeypatch):
    """a plan whose packed weights are stale (the parameters changed behind its back) is not stepped through: flat update"""
    monkeypatch.setenv("VPD_FUSED_ADAMW", "1")
    eng = _engine("fused", "none", False)
    eng._hip_version += 1
    stale = eng._step_plan.packed_version
    eng.adamw_step(*HYPER[:1])
    assert [c[0] for c in eng.L.calls if c[0] != "vpd_plan_grads_pending"] == ["vpd_adamw_step"]
    assert eng._step_plan.packed_version is stale and eng._hip_version == 5


def test_adam_buffers_are_created_on_first_use(monkeypatch):
    monkeypatch.setenv("VPD_FUSED_ADAMW", "1")
    eng = _engine("flat_no_plan", "none", False)
    eng.adam_m = eng.adam_v = None
    eng.adamw_step(HYPER[0])
    assert eng.adam_m.shape == eng.params.shape and eng.adam_v.shape == eng.params.shape
    name, args = eng.L.calls[-1]
    assert name == "vpd_adamw_step" and args[2:4] == (eng.adam_m.data_ptr(), eng.adam_v.data_ptr())
