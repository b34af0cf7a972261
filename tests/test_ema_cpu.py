"""Exponential moving average of the weights, the part that needs no GPU: vpd_ema_update is declared, bound and exported by both
libraries under ABI 5 and takes every refusal on the host; the float64 reference of tests/opref_ema.py against sequences worked
out by hand; timm's warmup schedule; the new flags of both command lines; the file names save_model(..., ema=True) writes."""
import ctypes as C
import os
import sys

import pytest
import torch

from tests import opref_ema as E
from tests.test_abi_cpu import header_functions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_entry_point_is_declared_bound_and_exported(dtype):
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    assert h.vpd_abi_version() == _lib.ABI_VERSION == 5
    assert "vpd_ema_update" in header_functions()
    assert len(_lib.SIGNATURES["vpd_ema_update"][1]) == 10
    assert h.vpd_ema_update.argtypes == _lib.SIGNATURES["vpd_ema_update"][1] and h.vpd_ema_update.restype is C.c_int


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_every_refusal_is_taken_on_the_host(dtype):
    from vpd_amd import _lib
    h = _lib.lib(dtype)
    # never dereferenced: every call below is rejected before anything is launched (or has nothing to launch)
    src = (C.c_void_p * 4)(64, 128, 192, 256)
    dst = (C.c_void_p * 4)(1024, 2048, 3072, 4096)
    n = (C.c_longlong * 4)(4, 0, 7, 1)

    def call(src=src, dst=dst, n=n, count=4, decay=0.999, warmup=0, t=0, t0=0, state=None):
        return h.vpd_ema_update(src, dst, n, count, decay, warmup, t, t0, state, None)

    def refused(rc, msg):
        return rc != 0 and msg in h.vpd_last_error()
    assert refused(call(src=None), b"null argument") and refused(call(dst=None), b"null argument") and refused(call(n=None), b"null argument")
    assert refused(call(src=(C.c_void_p * 4)(64, None, 192, 256)), b"null argument")
    assert refused(call(dst=(C.c_void_p * 4)(1024, 2048, 3072, None)), b"null argument")
    assert refused(call(count=-1), b"count outside 0..4") and refused(call(count=5), b"count outside 0..4")
    assert call(count=0) == 0 and call(src=None, dst=None, n=None, count=0) == 0      # nothing to do, nothing looked at
    assert refused(call(n=(C.c_longlong * 4)(4, 0, -1, 1)), b"negative length")
    for bad in (-1e-9, 1.0 + 1e-9, 2.0, float("inf"), float("-inf"), float("nan")):
        assert refused(call(decay=bad), b"decay must be in [0, 1]"), bad
        assert refused(call(decay=bad, count=0), b"decay must be in [0, 1]"), bad
    assert refused(call(t=-1), b"must not be negative") and refused(call(t0=-1), b"must not be negative")
    assert refused(call(dst=(C.c_void_p * 4)(1024, 128, 3072, 4096)), b"src and dst must differ")
    assert refused(call(src=(C.c_void_p * 4)(66, 128, 192, 256)), b"4-byte aligned")
    assert refused(call(state=C.c_void_p(66)), b"4-byte aligned")


def test_reference_against_sequences_worked_out_by_hand():
    src = [torch.tensor([1.0]), torch.tensor([2.0]), torch.tensor([4.0])]
    # decay 0.5 from 0: 0 + .5 (1 - 0) = .5;  .5 + .5 (2 - .5) = 1.25;  1.25 + .5 (4 - 1.25) = 2.625
    y = torch.zeros(1)
    seen = []
    for s in src:
        y = E.ema_ref(y, s, 0.5)
        seen.append(float(y))
    assert seen == [0.5, 1.25, 2.625]
    # warmup under decay 0.999: d = 1/10, 2/11, 3/12:  0 + .9 = .9;  .9 + (9/11)(1.1) = 1.8;  1.8 + .75 (2.2) = 3.45
    y = torch.zeros(1)
    seen = []
    for t, s in enumerate(src):
        y = E.ema_ref(y, s, 0.999, True, t)
        seen.append(float(y))
    assert seen == pytest.approx([0.9, 1.8, 3.45], rel=1e-15)
    ref, bound = E.ema_run(torch.zeros(1), src, 0.5)
    assert float(ref) == 2.625
    # exact operands: the bound is what three updates' roundings may add, a few units of 2^-24 of the values passing through
    assert 0.0 < float(bound) < 3 * 4 * E.U * 4.0
    # decay 1 leaves dst alone, decay 0 copies src
    assert float(E.ema_ref(torch.tensor([7.0]), torch.tensor([3.0]), 1.0)) == 7.0
    assert float(E.ema_ref(torch.tensor([7.0]), torch.tensor([3.0]), 0.0)) == 3.0


def test_warmup_schedule():
    assert E.ema_decay(0.9999, True, 0) == 0.1
    assert E.ema_decay(0.9999, True, 1) == 2.0 / 11.0
    assert E.ema_decay(0.9999, True, 89) == 90.0 / 99.0
    assert E.ema_decay(0.9999, True, 10 ** 6) == 0.9999                    # (1e6 + 1) / (1e6 + 10) = 0.999991 > decay
    assert E.ema_decay(0.5, True, 0) == 0.1 and E.ema_decay(0.5, True, 1) == 2.0 / 11.0
    assert E.ema_decay(0.5, True, 89) == 0.5 and E.ema_decay(0.5, True, 10 ** 6) == 0.5
    for t in (0, 1, 89, 10 ** 6):
        assert E.ema_decay(0.9999, False, t) == 0.9999


def test_both_command_lines_parse_the_new_flags(monkeypatch):
    import apply_vpd_model
    import train_vpd_model
    base = ["train_vpd_model.py", "diving48", "--save_dir", "out"]
    monkeypatch.setattr(sys, "argv", base)
    a = train_vpd_model.get_args()
    assert a.ema_decay is None and a.ema_warmup is False
    monkeypatch.setattr(sys, "argv", base + ["--ema_decay", "0.999", "--ema_warmup"])
    a = train_vpd_model.get_args()
    assert a.ema_decay == 0.999 and a.ema_warmup is True
    for bad in (["--ema_decay", "1.5"], ["--ema_decay", "-0.1"], ["--ema_warmup"]):
        monkeypatch.setattr(sys, "argv", base + bad)
        with pytest.raises(SystemExit):
            train_vpd_model.get_args()
    monkeypatch.setattr(sys, "argv", ["apply_vpd_model.py", "model", "-d", "fx"])
    assert apply_vpd_model.get_args().ema is False
    monkeypatch.setattr(sys, "argv", ["apply_vpd_model.py", "model", "-d", "fx", "--ema", "-m", "12"])
    a = apply_vpd_model.get_args()
    assert a.ema is True
    assert apply_vpd_model.checkpoint_name(a.model_epoch, a.ema) == "epoch0012_ema"
    assert apply_vpd_model.checkpoint_name(None, True) == "best_epoch_ema" and apply_vpd_model.checkpoint_name(None) == "best_epoch"
    # every parsed flag is an argument of main()
    import inspect
    assert {"ema_decay", "ema_warmup"} <= set(inspect.signature(train_vpd_model.main).parameters)
    assert "ema" in inspect.signature(apply_vpd_model.main).parameters


class _Stub:
    def __init__(self, tag):
        self.tag = tag

    def state_dict(self):
        return {"w": torch.tensor([1.0]), "from": self.tag + ".live"}

    def ema_state_dict(self):
        return {"w": torch.tensor([2.0]), "from": self.tag + ".ema"}


@pytest.mark.parametrize("motion", [False, True])
def test_save_model_file_names(tmp_path, motion):
    from vpd_amd.trainer import ModelTrainer

    class T:
        encoder = _Stub("encoder")
    t = T()
    if motion:
        t.fcn_time = _Stub("decoder")
    ModelTrainer.save_model(t, str(tmp_path), "best_epoch")
    ModelTrainer.save_model(t, str(tmp_path), "best_epoch", ema=True)
    ModelTrainer.save_model(t, str(tmp_path), "epoch0007", ema=True)
    want = {"best_epoch.encoder.pt", "best_epoch_ema.encoder.pt", "epoch0007_ema.encoder.pt"}
    if motion:
        want |= {"best_epoch.decoder.pt", "best_epoch_ema.decoder.pt", "epoch0007_ema.decoder.pt"}
    assert set(os.listdir(tmp_path)) == want
    for f in want:
        sd = torch.load(os.path.join(tmp_path, f))
        part = "encoder" if ".encoder." in f else "decoder"
        assert sd["from"] == part + (".ema" if "_ema." in f else ".live"), f
        assert float(sd["w"]) == (2.0 if "_ema." in f else 1.0)
