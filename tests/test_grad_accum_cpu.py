"""Gradient accumulation, the part that needs no GPU: the host-side refusals of vpd_op_grad_accumulate and vpd_plan_grad_accumulate,
the accumulator's size, the schedule of ModelTrainer.epoch, the CLI flag and the argument handling of step(..., accumulate=True)."""
import ctypes as C
import inspect
import sys

import pytest
import torch

NAMES = ("bf16", "fp16")


def _lib(name):
    from vpd_amd import _lib
    return _lib.lib(name)


def _arrs(dst, src, n):
    k = len(n)
    return (C.c_void_p * k)(*dst), (C.c_void_p * k)(*src), (C.c_longlong * k)(*n), k


@pytest.mark.parametrize("name", NAMES)
def test_op_grad_accumulate_refusals(name):
    """every refusal is taken on the host, with a message, before anything is launched (the pointers are never dereferenced)"""
    h = _lib(name)

    def refused(rc, msg):
        return rc != 0 and msg in h.vpd_last_error()
    d, s, n, k = _arrs([64, 4096], [8192, 12288], [5, 7])
    assert h.vpd_op_grad_accumulate(None, None, None, 0, 1, None) == 0            # count 0: nothing to do, nothing looked at
    assert h.vpd_op_grad_accumulate(d, s, n, 0, 0, None) == 0
    assert refused(h.vpd_op_grad_accumulate(d, s, n, -1, 1, None), b"negative count")
    assert refused(h.vpd_op_grad_accumulate(None, s, n, k, 1, None), b"null argument")
    assert refused(h.vpd_op_grad_accumulate(d, None, n, k, 1, None), b"null argument")
    assert refused(h.vpd_op_grad_accumulate(d, s, None, k, 1, None), b"null argument")
    for add in (0, 1):
        assert refused(h.vpd_op_grad_accumulate(*_arrs([64, None], [8192, 12288], [5, 7]), add, None), b"null range")
        assert refused(h.vpd_op_grad_accumulate(*_arrs([64, 4096], [None, 12288], [5, 7]), add, None), b"null range")
        assert refused(h.vpd_op_grad_accumulate(*_arrs([64, 4096], [8192, 12288], [5, -1]), add, None), b"negative length")
        assert refused(h.vpd_op_grad_accumulate(*_arrs([66, 4096], [8192, 12288], [5, 7]), add, None), b"4-byte aligned")
        assert refused(h.vpd_op_grad_accumulate(*_arrs([64, 4096], [8192, 12289], [5, 7]), add, None), b"4-byte aligned")
        assert refused(h.vpd_op_grad_accumulate(*_arrs([64, 4096], [8192, 4096], [5, 7]), add, None), b"must differ")
        assert refused(h.vpd_op_grad_accumulate(*_arrs([64, 4096], [8192, 4096], [5, 0]), add, None), b"must differ")   # (even when empty)


def _plan(h, name, arch="resnet18", train=1, motion=0):
    from vpd_amd import _lib
    p = C.c_void_p()
    _lib.check(h.vpd_plan_create(arch.encode(), 5, 64, 64, 32, motion, 4, train, C.byref(p)), "create", name)
    return p


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("arch,motion", [("resnet18", 0), ("resnet34", 1), ("resnet50", 0)])
def test_accumulator_is_the_scratch_behind_the_stem_plus_the_flat_buffer(name, arch, motion):
    h = _lib(name)
    p = _plan(h, name, arch, 1, motion)
    o, m = C.c_longlong(), C.c_longlong()
    scratch, lo, hi = 0, None, 0
    for b in range(h.vpd_plan_num_buckets(p)):
        assert h.vpd_plan_bucket_scratch_range(p, b, C.byref(o), C.byref(m)) == 0
        scratch += m.value
        if m.value:
            lo = o.value if lo is None else min(lo, o.value)
            hi = max(hi, o.value + 4 * m.value)
    assert scratch > 0 and hi - lo == 4 * scratch                                # the bucket ranges tile one piece of the workspace
    assert h.vpd_plan_grad_accum_numel(p) == scratch + h.vpd_plan_param_numel(p)
    assert h.vpd_plan_grad_accum_numel(p) % 4 == 0 and scratch % 4 == 0          # the flat image starts on a 16-byte boundary
    # ... and so does the scratch behind the stem inside the workspace: its image at accum[0] shares its 16-byte phase, so the
    # 85 MB range takes the kernel's 16-byte path and not the float-by-float reads of src
    assert lo % 16 == 0
    h.vpd_plan_destroy(p)
    assert h.vpd_plan_grad_accum_numel(None) == 0


@pytest.mark.parametrize("name", NAMES)
def test_plan_grad_accumulate_refusals(name):
    h = _lib(name)
    p = _plan(h, name)
    numel = h.vpd_plan_param_numel(p)
    q = C.c_void_p(4096)                                  # never dereferenced: every call below is rejected on the host

    def refused(rc, msg):
        return rc != 0 and msg in h.vpd_last_error()
    for i in (0, 1, 3, 5):
        args = [p, q, numel, q, 0, q, None]
        args[i] = None
        assert refused(h.vpd_plan_grad_accumulate(*args), b"null argument"), i
    for mode in (-1, 3, 7):
        assert refused(h.vpd_plan_grad_accumulate(p, q, numel, q, mode, q, None), b"mode outside 0..2")
    for mode in (0, 1, 2):
        assert refused(h.vpd_plan_grad_accumulate(p, q, numel, C.c_void_p(4100), mode, q, None), b"accum must be 16-byte aligned")
        # the refusals of the other plan step entries: a workspace that vpd_plan_init_workspace never saw
        assert refused(h.vpd_plan_grad_accumulate(p, q, numel, C.c_void_p(8192), mode, q, None), b"workspace not initialised")
    assert h.vpd_plan_grads_pending(p) == 0
    h.vpd_plan_destroy(p)


def test_entry_points_are_declared_and_bound():
    from tests.test_abi_cpu import header_functions
    from vpd_amd import _lib
    for n, nargs in (("vpd_op_grad_accumulate", 6), ("vpd_plan_grad_accum_numel", 1), ("vpd_plan_grad_accumulate", 7)):
        assert n in header_functions() and len(_lib.SIGNATURES[n][1]) == nargs
        for name in NAMES:
            assert getattr(_lib.lib(name), n).argtypes == _lib.SIGNATURES[n][1]
    assert _lib.SIGNATURES["vpd_plan_grad_accum_numel"][0] is C.c_longlong


def test_schedule_steps_on_every_kth_batch_and_on_the_last():
    from vpd_amd.trainer import accumulation_schedule as sched
    assert list(sched(range(4), 1)) == [(0, True), (1, True), (2, True), (3, True)]
    got = list(sched(range(1, 8), 3))
    assert [b for b, _ in got] == [1, 2, 3, 4, 5, 6, 7]
    assert [b for b, s in got if s] == [3, 6, 7]                                  # the ragged last window steps too
    assert [b for b, s in sched(range(1, 7), 3) if s] == [3, 6]                   # (a last batch that is a K-th one steps once)
    assert [b for b, s in sched(range(1, 3), 5) if s] == [2]                      # fewer batches than K: one step, at the end
    assert list(sched([], 3)) == [] and list(sched(iter(()), 1)) == []            # an empty loader

    def gen():                                                                    # an iterable without a length: one-item look-ahead
        yield from "abcde"
    assert list(sched(gen(), 2)) == [("a", False), ("b", True), ("c", False), ("d", True), ("e", True)]
    for bad in (0, -2):
        with pytest.raises(ValueError, match="accum_steps"):
            list(sched(range(3), bad))


def test_trainer_validates_accum_steps():
    from vpd_amd.trainer import ModelTrainer
    sig = inspect.signature(ModelTrainer.__init__).parameters
    assert sig["accum_steps"].default == 1

    class _Enc:
        device = "cpu"

        def to(self, device):
            return self
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="accum_steps"):
            ModelTrainer(_Enc(), False, accum_steps=bad)


def test_train_cli_parses_accum_steps(monkeypatch):
    import train_vpd_model
    base = ["train_vpd_model.py", "diving48", "--save_dir", "out"]
    monkeypatch.setattr(sys, "argv", base)
    assert train_vpd_model.get_args().accum_steps is None
    monkeypatch.setattr(sys, "argv", base + ["--accum_steps", "4"])
    assert train_vpd_model.get_args().accum_steps == 4
    for bad in ("0", "-3", "1.5"):
        monkeypatch.setattr(sys, "argv", base + ["--accum_steps", bad])
        with pytest.raises(SystemExit):
            train_vpd_model.get_args()
    assert inspect.signature(train_vpd_model.main).parameters["accum_steps"].default is None


class _Rec:
    """a loss / optimizer / scaler that records what step() calls"""

    def __init__(self, lazy_opt=True):
        self.calls = []
        self.consumes_lazy_grads = lazy_opt

    def backward(self):
        self.calls.append("backward")

    def backward_for_step(self):
        self.calls.append("backward_for_step")

    def backward_for_accumulation(self, lazy=False):
        self.calls.append(("backward_for_accumulation", lazy))

    def step(self):
        self.calls.append("opt.step")

    def zero_grad(self):
        self.calls.append("zero_grad")


def test_step_accumulate_runs_the_backward_and_nothing_else():
    from vpd_amd.models import util
    assert inspect.signature(util.step).parameters["accumulate"].default is False
    for lazy_opt in (True, False):
        loss, opt = _Rec(), _Rec(lazy_opt)
        util.step(opt, None, loss, accumulate=True)
        assert loss.calls == [("backward_for_accumulation", bool(lazy_opt and util._LAZY))] and opt.calls == []
    # the final call of a window is the step of always
    loss, opt = _Rec(), _Rec(True)
    util.step(opt, None, loss)
    assert loss.calls == ["backward_for_step" if util._LAZY else "backward"] and opt.calls == ["opt.step", "zero_grad"]
    # a scaler scales, and is neither stepped nor updated
    class _Scaler(util.LossScaler):
        def __init__(self):
            self.calls = []

        def scale(self, loss):
            self.calls.append("scale")
            return loss

        def step(self, optimizer):
            self.calls.append("step")

        def update(self):
            self.calls.append("update")
    loss, opt, sc = _Rec(), _Rec(True), _Scaler()
    util.step(opt, sc, loss, accumulate=True)
    assert sc.calls == ["scale"] and opt.calls == [] and len(loss.calls) == 1
    # refused: a loss that cannot accumulate (a torch tensor accumulates into .grad by itself), a foreign scaler
    with pytest.raises(TypeError, match="accumulate=True"):
        util.step(opt, None, torch.zeros(1), accumulate=True)
    with pytest.raises(ValueError, match="scaler"):
        util.step(opt, object(), loss, accumulate=True)


def test_engine_without_an_accumulator_folds_nothing():
    """K = 1: fold_accumulated_grads() launches nothing and allocates nothing; accumulate / fold before any backward raise"""
    from vpd_amd.engine import StudentEngine
    eng = StudentEngine.__new__(StudentEngine)

    class _NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library call %s" % name)
    eng.L = _NoCalls()
    eng._step_plan = None
    eng.fold_accumulated_grads()
    assert eng._accum is None and eng._accum_count == 0
    with pytest.raises(RuntimeError, match="without a preceding backward"):
        eng.accumulate_grads()
    eng._accum_count = 1
    with pytest.raises(RuntimeError, match="without a preceding backward"):
        eng.fold_accumulated_grads()
