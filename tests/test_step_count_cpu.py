"""Where the applied-step count and the EMA's update count live, transition by transition (StudentEngine.adam_step, ema_state):
after every move both the value and its home are asserted -- the host integer, word `applied_steps` of a DynamicLossScaler's
block, word `applied_steps` of the clip block.  A stub library and CPU tensors (tests/engine_stub.py): no kernel runs, so a
block's word moves only when the host writes it or the test plays the device."""
import torch

from tests.engine_stub import BN_NUMEL, NUMEL, stub_engine
from vpd_amd.models.util import DynamicLossScaler

APPLIED = 3      # int applied_steps of vpd_scale_state (include/vpd_hip.h), which a vpd_clip_state begins with


def _host(eng):
    return eng._steps.host


def _counting(eng):
    """the device block that holds the count, or None = the host"""
    return eng._steps.block


def _homes(eng, scaler=None):
    """(adam_step, the host integer, the scaler's word, the clip block's word)"""
    return (eng.adam_step, _host(eng), None if scaler is None else int(scaler.state[APPLIED]),
            None if eng._clip is None else int(eng._clip[APPLIED]))


def _step(eng):
    eng.adamw_step(1e-3)


def test_the_step_count_without_a_block_then_clip_then_a_scaler_that_takes_over():
    eng = stub_engine(plan_numel=None)
    assert _homes(eng) == (6, 6, None, None) and _counting(eng) is None
    _step(eng)                                               # no block: the host counts
    assert _homes(eng) == (7, 7, None, None) and _counting(eng) is None
    eng.enable_grad_clip(2.5)                                # without a scaler: the clip block is seeded and counts
    assert _homes(eng) == (7, 7, None, 7) and _counting(eng) is eng._clip
    _step(eng)                                               # behind a block the host neither counts nor writes the word
    assert _homes(eng) == (7, 7, None, 7)
    eng.enable_grad_clip(3.0)                                # again: max_norm only, the block is not seeded twice
    assert _homes(eng) == (7, 7, None, 7) and _counting(eng) is eng._clip and eng.clip_state()["max_norm"] == 3.0
    eng.adam_step = 9                                        # the host value and the counting block
    assert _homes(eng) == (9, 9, None, 9)
    scaler = DynamicLossScaler(eng, init_scale=512.0)        # after clipping was enabled: seeded from the count, takes over
    assert _homes(eng, scaler) == (9, 9, 9, 9) and _counting(eng) is scaler.state
    eng.adam_step = 11                                       # ... the counting block ONLY: the clip block's word stays
    assert _homes(eng, scaler) == (11, 11, 11, 9)
    eng.load_clip_state(dict(eng.clip_state(), max_norm=2.5))      # the clip block's word follows adam_step
    assert _homes(eng, scaler) == (11, 11, 11, 11) and _counting(eng) is scaler.state
    scaler.state[APPLIED] = 12                               # (the device applied a step)
    assert _homes(eng, scaler) == (12, 11, 12, 11)
    eng.disable_grad_clip()                                  # the clip block did not hold the count: nothing comes back
    assert _homes(eng, scaler) == (12, 11, 12, None) and _counting(eng) is scaler.state and not eng.grad_clip_enabled


def test_the_step_count_behind_a_scaler_stays_there_when_clipping_comes_and_goes():
    eng = stub_engine(plan_numel=None)
    _step(eng)
    scaler = DynamicLossScaler(eng, init_scale=512.0)        # seeded from the current count, authoritative from now on
    assert _homes(eng, scaler) == (7, 7, 7, None) and _counting(eng) is scaler.state
    _step(eng)                                               # (no scaled step in flight: the host's +1 goes through the setter)
    assert _homes(eng, scaler) == (8, 8, 8, None)
    eng.enable_grad_clip(2.5)                                # seeds the clip block; the scaler's block keeps the count
    assert _homes(eng, scaler) == (8, 8, 8, 8) and _counting(eng) is scaler.state
    eng.adam_step = 9
    assert _homes(eng, scaler) == (9, 9, 9, 8)
    eng.load_clip_state(eng.clip_state())
    assert _homes(eng, scaler) == (9, 9, 9, 9)
    eng.disable_grad_clip()
    assert _homes(eng, scaler) == (9, 9, 9, None) and _counting(eng) is scaler.state


def test_the_step_count_comes_back_to_the_host_exactly_when_the_clip_block_held_it():
    eng = stub_engine(plan_numel=None)
    eng.enable_grad_clip(float("inf"))
    assert _homes(eng) == (6, 6, None, 6) and _counting(eng) is eng._clip
    eng._clip[APPLIED] = 8                                   # (the device applied two steps)
    assert _homes(eng) == (8, 6, None, 8)
    eng.disable_grad_clip()
    assert _homes(eng) == (8, 8, None, None) and _counting(eng) is None
    eng.disable_grad_clip()                                  # a second call: nothing to do
    assert _homes(eng) == (8, 8, None, None)
    _step(eng)
    assert _homes(eng) == (9, 9, None, None)


def _ema_update_args(eng):
    """(t, t0, state) of the last vpd_ema_update"""
    name, args = [c for c in eng.L.calls if c[0] == "vpd_ema_update"][-1]
    return args[6:9]


def test_the_ema_update_count_on_the_host_and_behind_a_block_before_and_after_a_load():
    eng = stub_engine(plan_numel=None)
    eng.enable_ema(0.5)                                      # averaging begins at step 6
    assert (eng._ema_t, eng._ema_t0, eng.ema_state()["num_updates"]) == (0, 6, 0)
    _step(eng)
    _step(eng)                                               # the host counts: `_ema_t`
    assert (eng._ema_t, eng._ema_t0, eng.ema_state()["num_updates"]) == (2, 6, 2) and eng.adam_step == 8
    assert _ema_update_args(eng) == (1, 6, None)
    stored = {"params": torch.ones(NUMEL), "bn_running": torch.ones(BN_NUMEL), "decay": 0.5, "warmup": False, "num_updates": 5}
    eng.load_ema_state(stored)                               # both sides are written: t0 = adam_step - num_updates
    assert (eng._ema_t, eng._ema_t0, eng.ema_state()["num_updates"]) == (5, 3, 5)
    eng.enable_grad_clip(2.5)                                # a block counts: applied steps - `_ema_t0`
    assert (eng._ema_t, eng._ema_t0, eng.ema_state()["num_updates"]) == (5, 3, 5)
    eng._clip[APPLIED] = 10                                  # (the device applied two steps)
    assert (eng._ema_t, eng.ema_state()["num_updates"]) == (5, 7)
    _step(eng)                                               # behind the block the host's count stands still
    assert (eng._ema_t, eng.ema_state()["num_updates"]) == (5, 7)
    assert _ema_update_args(eng) == (0, 3, eng._clip.data_ptr())
    eng.load_ema_state(dict(stored, num_updates=4))
    assert (eng._ema_t, eng._ema_t0, eng.ema_state()["num_updates"]) == (4, 6, 4)
    eng.ema_update()                                         # the manual update counts on the host whatever holds the step count
    assert eng._ema_t == 5 and _ema_update_args(eng) == (4, 6, None) and eng.ema_state()["num_updates"] == 4
    eng.disable_grad_clip()                                  # back on the host: `_ema_t` again
    assert eng.adam_step == 10 and eng.ema_state()["num_updates"] == 5
    eng.load_ema_state(dict(stored, num_updates=12))         # more updates than steps: t0 stops at 0
    assert (eng._ema_t, eng._ema_t0, eng.ema_state()["num_updates"]) == (12, 0, 12)
