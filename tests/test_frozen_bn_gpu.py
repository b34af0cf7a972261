"""Frozen BatchNorm through the module (RGBF_EmbeddingModel.freeze_bn -> vpd_plan_set_bn_frozen) and the data-gradient-only
backward (vpd_plan_set_param_grads): gradients and embeddings of a train-mode forward on RUNNING statistics against the CPU
oracle's eval-mode autograd, the state that must not move, the fused path as a self-check, the mode recorded at forward, and a
backward that launches no weight-gradient kernel.  Every test fails without the feature: freeze_bn does not exist.

Recipe (shared): O.reference_init_state_dict(arch, 5, 32, 3) with every .bn2.weight / .bn3.weight x 0.1, running statistics warmed
by 30 oracle train-mode forwards over synthetic_crops(8, 5, 64, 20 + s) -- on ResNet-18 |running_mean| reaches 0.9 and running_var
lies in 0.26 .. 0.45, far from 0 / 1 and from the test batch's own statistics: train-mode and eval-mode gradients of this recipe
have per-stage cosine 0.22 .. 0.51, so a pass that silently uses batch statistics fails every gate here.  Batch
synthetic_crops(8, 5, 64, 5), targets synthetic_targets(8, 32, False, 6), loss = the weighted cosine loss of test_autograd_gpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import vpd_oracle as O
from tests import opref_autograd as A
from tests.test_autograd_gpu import FP16_SCALE, _assert_same, _done, _fused, _grads, _model, _mse_de
from tests.test_fp16_gpu import FP16_LOSS_TOL
from tests.test_model_gpu import COS_MIN, PROJ_TOL, _dump, _group_metrics, cosine, per_sample_rel, rel_l2

pytestmark = pytest.mark.gpu

C_IN, D, N, HW = 5, 32, 8, 64
BF16_EMB_TOL = 2e-2        # the project's bf16 eval gate (smoke(), test_student_matches_reference_and_oracle)
# fp16 embeddings of the frozen train plan against the fp32 oracle, per sample: twice the measured maximum, but no looser than 2 x the
# eval plan's 1.5e-3 -- the train plan rounds each conv output to the element type before BatchNorm and again after, where the folded
# eval plan rounds once.  Measured (profiles/frozen_bn_parity.txt): 1.85e-3 against the oracle, 1.69e-3 against forward_eval (which is
# itself 1.76e-3 off the oracle on this recipe); twice that is 3.7e-3, so the cap holds: 3e-3
FP16_EMB_TOL_FROZEN = 3e-3


@functools.lru_cache(maxsize=None)
def _recipe(arch):
    sd = O.reference_init_state_dict(arch, C_IN, D, 3)
    for k in sd:
        if k.endswith(".bn2.weight") or k.endswith(".bn3.weight"):
            sd[k] = sd[k] * 0.1
    with torch.no_grad():
        for s in range(30):
            O.encoder_forward(sd, O.synthetic_crops(N, C_IN, HW, 20 + s), arch, True)
    return sd


def _loss(emb, tgt):
    return A.weighted_cosine_loss(emb, tgt, A.crop_weights(N, 9).to(emb.device))


@functools.lru_cache(maxsize=None)
def _oracle(arch, emulate, seed):
    """eval-mode CPU autograd through the oracle: (loss, {name: grad}, d loss / d img, embeddings, img, tgt)"""
    sd = {k: v.clone() for k, v in _recipe(arch).items()}
    keys = O.trainable_keys(O.encoder_schema(arch, C_IN, D))
    for k in keys:
        sd[k].requires_grad_(True)
    img, tgt = O.synthetic_crops(N, C_IN, HW, seed), O.synthetic_targets(N, D, False, seed + 1)
    x = img.clone().requires_grad_(True)
    emb = O.encoder_forward(sd, x, arch, False, emulate_bf16=emulate)
    loss = _loss(emb, tgt)
    loss.backward()
    return float(loss.detach()), {k: sd[k].grad.detach().clone() for k in keys}, x.grad.detach().clone(), emb.detach().clone(), img, tgt


def _frozen_model(arch, dtype):
    enc = _model(arch, dtype, _recipe(arch))
    assert enc.freeze_bn() is enc and enc.bn_frozen and enc.training
    return enc


def _bn_state(enc):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in enc.state_dict().items()
            if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked")}


def _same_state(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


# -- 1. fp16 against the fp32 oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_frozen_gradients_match_the_eval_mode_oracle_fp16(arch):
    """fp16 library against fp32 eval-mode autograd: loss within FP16_LOSS_TOL, per stage cos >= 0.99 and projection 1 +- 2 % (the
    gates of test_weighted_cosine_loss_matches_the_oracle_gradients), x.grad under test_fp16_gpu.py's per-tensor gates (rel-L2 <=
    0.45, cos >= 0.88).  The loss is scaled by 256."""
    l_ref, g_ref, dx_ref, _, img, tgt = _oracle(arch, False, 5)
    enc = _frozen_model(arch, "fp16")
    state = _bn_state(enc)
    x = img.cuda().requires_grad_()
    enc.zero_grad()
    emb = enc(x)
    assert emb.requires_grad and emb.grad_fn is not None
    loss = _loss(emb, tgt.cuda())
    l_hip = loss.item()
    (loss * FP16_SCALE).backward()
    ga = {n: v / FP16_SCALE for n, v in _grads(enc).items()}
    dx = (x.grad / FP16_SCALE).cpu().numpy()
    res = _group_metrics(lambda n: ga[n].cpu(), lambda n: g_ref[n], list(g_ref))
    rec = {"arch": arch, "loss": [l_hip, l_ref], "columns": ["rel_l2", "cos", "projection"],
           "hip_vs_oracle": {k: [round(v, 4) for v in t] for k, t in res.items()},
           "img_grad": [rel_l2(dx, dx_ref.numpy()), cosine(dx, dx_ref.numpy())]}
    _dump("frozen_bn_fp16_%s" % arch, rec)
    print(rec)
    assert abs(l_hip - l_ref) <= FP16_LOSS_TOL * abs(l_ref), rec["loss"]
    assert all(c >= 0.99 and abs(pj - 1) <= 0.02 for _, c, pj in res.values()), res
    assert np.isfinite(dx).all() and rec["img_grad"][0] <= 0.45 and rec["img_grad"][1] >= 0.88, rec
    assert _same_state(state, _bn_state(enc))
    _done(enc)


# -- 2. bf16 against the bf16 emulation ----------------------------------------------------------------------------------------
def test_frozen_gradients_match_the_bf16_emulation():
    """bf16 library, ResNet-18, against the oracle's emulate_bf16 eval-mode gradients summed over three batches, under
    test_backward_matches_bf16_emulation_directly's PROJ_TOL / COS_MIN per stage."""
    arch = "resnet18"
    enc = _frozen_model(arch, "bf16")
    names = [n for n, _ in enc.named_parameters()]
    g_hip, g_emu = {n: 0.0 for n in names}, {n: 0.0 for n in names}
    for b in range(3):
        _, ge, _, _, img, tgt = _oracle(arch, True, 5 + 10 * b)
        enc.zero_grad()
        _loss(enc(img.cuda()), tgt.cuda()).backward()
        for n, v in _grads(enc).items():
            g_hip[n] = g_hip[n] + v.cpu().double()
            g_emu[n] = g_emu[n] + ge[n].double()
    res = _group_metrics(lambda n: g_hip[n], lambda n: g_emu[n], names)
    rec = {"columns": ["rel_l2", "cos", "projection"], "hip_vs_emulation": {k: [round(v, 5) for v in t] for k, t in res.items()}}
    _dump("frozen_bn_bf16_emulation", rec)
    print(rec)
    for k, (err, cos, proj) in res.items():
        assert abs(proj - 1) <= PROJ_TOL and cos >= COS_MIN, (k, err, cos, proj)
    _done(enc)


# -- 3. the function itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [("bf16", BF16_EMB_TOL), ("fp16", FP16_EMB_TOL_FROZEN)])
def test_frozen_embeddings_match_the_eval_function(dtype, tol):
    """A frozen train-mode forward computes what embed() computes: per-sample rel-L2 against the fp32 oracle's eval embeddings and
    against forward_eval of the same model, under one bound.  bf16: the project's eval gate, 2e-2 (measured 1.51e-2 / 9.9e-3).  fp16:
    FP16_EMB_TOL_FROZEN = 3e-3 (measured 1.85e-3 against the oracle, 1.69e-3 against forward_eval)."""
    _, _, _, e_ref, img, _ = _oracle("resnet18", False, 5)
    enc = _frozen_model("resnet18", dtype)
    with torch.no_grad():
        e_frozen = enc(img.cuda()).cpu().numpy()
    e_eval = enc.engine.forward_eval(img.cuda()).cpu().numpy()
    assert enc.training and enc.bn_frozen
    r_oracle, r_eval = per_sample_rel(e_frozen, e_ref.numpy()), per_sample_rel(e_frozen, e_eval)
    rec = {"dtype": dtype, "frozen_vs_oracle_max": float(np.max(r_oracle)), "frozen_vs_forward_eval_max": float(np.max(r_eval)),
           "forward_eval_vs_oracle_max": float(np.max(per_sample_rel(e_eval, e_ref.numpy())))}
    _dump("frozen_bn_embeddings_%s" % dtype, rec)
    print(rec)
    assert np.max(r_oracle) <= tol and np.max(r_eval) <= tol, rec
    _done(enc)


# -- 4. state --------------------------------------------------------------------------------------------------------------------
def test_frozen_passes_leave_the_batchnorm_state_alone():
    enc = _frozen_model("resnet18", "bf16")
    eng = enc.engine
    _, _, _, _, img, tgt = _oracle("resnet18", False, 5)
    img, tgt = img.cuda(), tgt.cuda()
    state = _bn_state(enc)
    version = eng._hip_version
    enc.zero_grad()
    _loss(enc(img), tgt).backward()                                    # the autograd route
    _fused(enc, img, tgt)                                              # the fused route: the flag lives on the plan
    with torch.no_grad():
        enc(img)                                                       # the plain route
    assert _same_state(state, _bn_state(enc))
    assert eng._hip_version == version and eng._nbt_pending == 0       # the packed eval fold stays valid, nothing was tracked
    # eval() is what it was: the inference plan, a plain tensor
    enc.eval()
    e = enc(img)
    assert e.grad_fn is None and not e.requires_grad
    enc.train()
    assert enc.freeze_bn(False) is enc and not enc.bn_frozen
    with torch.no_grad():
        enc(img)
    after = _bn_state(enc)
    assert all(not torch.equal(after[k], state[k]) for k in state)
    _done(enc)


# -- 5. self-consistency with the fused path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,dtype,n,hw", [("resnet18", "bf16", N, HW), ("resnet18", "fp16", N, HW), ("resnet50", "bf16", 64, 128)])
def test_frozen_autograd_gradients_equal_the_frozen_fused_path(arch, dtype, n, hw):
    """test_autograd_gradients_equal_the_fused_path, frozen: autograd with the library's own d(sum-MSE)/d(emb) against
    forward_train(target) + backward(), tensor by tensor, under that test's rules.  ResNet-50 at 64 crops of 128: the Bottleneck
    tails are recomputed (the streaming kernels' frozen modes 1 and 3)."""
    enc = _frozen_model(arch, dtype)
    g = torch.Generator().manual_seed(5)
    img, tgt = torch.randn(n, C_IN, hw, hw, generator=g).cuda(), torch.randn(n, D, generator=g).cuda()
    state = _bn_state(enc)
    fused = [_fused(enc, img, tgt) for _ in range(3)]
    enc.zero_grad()
    emb = enc(img)
    assert emb.requires_grad and tuple(emb.shape) == (n, D)
    emb.backward(_mse_de(enc, emb, tgt))
    ga = _grads(enc)
    assert set(ga) == set(fused[0]) and all(float(v.abs().max()) > 0 for v in ga.values())
    _assert_same(ga, fused, arch, "frozen %s %s" % (arch, dtype))
    # ... and it is not the train-mode pass
    enc.freeze_bn(False)
    unfrozen = _fused(enc, img, tgt)
    assert not torch.equal(unfrozen["resnet.conv1.weight"], fused[0]["resnet.conv1.weight"])
    enc.freeze_bn(True)
    assert not _same_state(state, _bn_state(enc))      # (the unfrozen pass moved the statistics, the frozen ones had not)
    _done(enc)


# -- 6. the mode is recorded at forward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,n,hw", [("resnet18", N, HW), ("resnet50", 64, 128)])
def test_backward_uses_the_mode_its_forward_ran_in(arch, n, hw):
    enc = _frozen_model(arch, "bf16")
    eng = enc.engine
    g = torch.Generator().manual_seed(7)
    img, tgt = torch.randn(n, C_IN, hw, hw, generator=g).cuda(), torch.randn(n, D, generator=g).cuda()

    def run(flip):
        enc.freeze_bn(True)
        enc.zero_grad()
        x = img.clone().requires_grad_()
        emb = enc(x)
        de = _mse_de(enc, emb, tgt)
        if flip:      # the module's flag and the plan's: neither may reach the backward of a forward that ran frozen
            enc.freeze_bn(False)
            pl = eng._last_fwd[0]
            eng.check(eng.L.vpd_plan_set_bn_frozen(pl.handle, 0), "vpd_plan_set_bn_frozen")
            pl.bn_frozen = False
        emb.backward(de)
        return _grads(enc), x.grad.clone()

    (g0, dx0), (g1, dx1) = run(False), run(True)
    assert torch.equal(dx0, dx1)
    loose = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert all(arch == "resnet50" and g0[k].dim() == 4 for k in loose), loose      # (fp32 atomics: _may_differ_run_to_run)
    _done(enc)


# -- 7. data gradients only ------------------------------------------------------------------------------------------------------
def _timed_counts(eng, pl):
    out = (C.c_double * 24)()
    eng.check(eng.L.vpd_plan_read_timing(pl.handle, out, 8), "vpd_plan_read_timing")
    return [int(out[3 * i]) for i in range(8)]


@pytest.mark.parametrize("frozen", [True, False], ids=["frozen", "train_mode"])
@pytest.mark.parametrize("arch,dtype", [("resnet18", "bf16"), ("resnet18", "fp16"), ("resnet50", "bf16")])
def test_data_only_backward_writes_no_parameter_gradient(arch, dtype, frozen):
    """every parameter requires_grad_(False): x.grad bit-identical to the full pass's, the flat buffer (sentinel-filled) and every
    .grad untouched, no second buffer, no launch in the weight-gradient timing classes 5 / 6 and the same launches in classes 0..4"""
    enc = _model(arch, dtype, _recipe(arch))
    enc.freeze_bn(frozen)
    eng = enc.engine
    _, _, _, _, img, tgt = _oracle("resnet18", False, 5)
    img, tgt = img.cuda(), tgt.cuda()
    scale = FP16_SCALE if dtype == "fp16" else 1.0
    enc.zero_grad()
    with torch.no_grad():
        enc(img)                                                      # creates the plan
    pl = eng._last_fwd[0]
    eng.set_timing(pl, True)
    x = img.clone().requires_grad_()
    (_loss(enc(x), tgt) * scale).backward()
    torch.cuda.synchronize()
    full = _timed_counts(eng, pl)
    assert full[5] + full[6] > 0 and eng.sync_errors() == 0
    SENT = -123.25
    eng._grads.fill_(SENT)
    for q in enc.parameters():
        q.requires_grad_(False)
    state = _bn_state(enc)
    y = img.clone().requires_grad_()
    (_loss(enc(y), tgt) * scale).backward()
    torch.cuda.synchronize()
    only = _timed_counts(eng, pl)
    eng.set_timing(pl, False)
    assert torch.equal(y.grad, x.grad) and float(y.grad.abs().max()) > 0
    assert bool((eng._grads == SENT).all()) and eng._grads2 is None
    assert all(q.grad is None or bool((q.grad == SENT).all()) for q in enc.parameters())
    assert only[5] == 0 and only[6] == 0 and only[:5] == full[:5], (full, only)
    assert _same_state(state, _bn_state(enc)) == frozen
    # back on: a full pass overwrites the sentinel again
    for q in enc.parameters():
        q.requires_grad_(True)
    enc.zero_grad()
    (_loss(enc(img), tgt) * scale).backward()
    torch.cuda.synchronize()
    assert all(q.grad is not None and not bool((q.grad == SENT).any()) for q in enc.parameters())
    _done(enc)
