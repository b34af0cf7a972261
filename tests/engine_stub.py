"""A StudentEngine that needs no GPU and no native library, for the tests of its host-side logic: CPU tensors, a library that records
every call, and only what a train plan shows adamw_step.  The step state is the engine's own (StudentEngine._reset_step_state): a
test sets what its case varies and nothing else."""
import ctypes as C
from collections import OrderedDict

import torch

from vpd_amd.engine import StudentEngine

NUMEL, BN_NUMEL = 64, 8


class RecLib:
    """every attribute is an entry point that records (name, arguments) and returns 0; the two size queries answer a size"""
    SIZES = {"vpd_adam_groups_bytes": 64, "vpd_clip_state_bytes": 256}

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            conv = lambda a: a.value if isinstance(a, C.c_void_p) else (list(a) if isinstance(a, C.Array) else a)
            self.calls.append((name, tuple(conv(a) for a in args)))
            return self.SIZES.get(name, 0)
        return entry


class StubPlan:
    """what adamw_step touches of the train plan of the last backward"""

    def __init__(self, param_numel):
        self.handle = C.c_void_p(0x1000)
        self.workspace = torch.zeros(16)
        self.param_numel = param_numel
        self.packed_version = None
        self.motion = True


def stub_engine(plan_numel=NUMEL, layout=None):
    """An engine 6 steps into training with NUMEL parameters; plan_numel: the parameters of the current train plan of its last
    backward (None: no plan); layout: rows (name, kind, is_decoder, offset, numel) of a toy StudentEngine.layout"""
    eng = StudentEngine.__new__(StudentEngine)
    eng.L = RecLib()
    eng.check = lambda rc, what="": None
    eng._stream = lambda: None
    eng.device = torch.device("cpu")
    eng._reset_step_state()
    eng.param_numel, eng.bn_numel = NUMEL, BN_NUMEL
    eng.params, eng._grads = torch.zeros(NUMEL), torch.zeros(NUMEL)
    eng.adam_m, eng.adam_v = torch.zeros(NUMEL), torch.zeros(NUMEL)
    eng.bn_running = torch.zeros(BN_NUMEL)
    eng.adam_step = 6
    eng._hip_version = 3
    if layout is not None:
        eng.layout = OrderedDict((n, (k, d, o, m, (m,))) for n, k, d, o, m in layout)
    eng._step_plan = None if plan_numel is None else StubPlan(plan_numel)
    if eng._step_plan is not None:
        eng._step_plan.packed_version = eng.weights_version()
    return eng
