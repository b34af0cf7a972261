"""torch autograd through RGBF_EmbeddingModel.forward (vpd_amd/models/rgb.py: _StudentFunction over vpd_backward_ext): the same
gradients as the fused path where the fused path can express the loss, the CPU oracle's where it cannot, torch's accumulate
semantics of .grad, a torch optimizer end to end, the input gradient (conv_stem_dgrad_kernel) and the guards of a plan that holds
one forward's activations.  Every case fails on a library / module without the autograd path: emb.requires_grad is False there."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vpd_oracle as O
from tests import opref_autograd as A
from tests.test_fp16_gpu import FP16_LOSS_TOL
from tests.test_model_gpu import _dump, _group_metrics, cosine, rel_l2
from tests.test_ops_gpu import ptr, stream

pytestmark = pytest.mark.gpu

ARCH, C_IN, D, N, HW = "resnet18", 5, 32, 8, 64
FP16_SCALE = 256.0        # the project's static fp16 loss scale (models.util.LossScaler): activation gradients are fp16

# The FUSED path itself does not reproduce every gradient bit for bit from run to run: some of ResNet-50's convolution weight
# gradients are summed with fp32 atomics (conv_wgrad_kernel; first seen: resnet.layer1.0.conv1.weight, the 64 -> 64 1x1).  A
# weight gradient feeds nothing else in the pass, so only convolution weights of the Bottleneck student may differ run to run;
# those are held to the fused path's own run-to-run difference (with a floor), every other tensor to torch.equal.
def _may_differ_run_to_run(arch, name, t):
    return arch == "resnet50" and t.dim() == 4 and name.endswith(".weight")


def _model(arch=ARCH, dtype="bf16", sd=None):
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    enc = RGBF_EmbeddingModel(arch, D, True, "cuda", dtype=dtype)
    enc.load_state_dict(sd if sd is not None else O.procedural_state_dict(O.encoder_schema(arch, C_IN, D), 1))
    enc.train()
    return enc


def _batch(seed, n=N, hw=HW):
    return O.synthetic_crops(n, C_IN, hw, seed).cuda(), O.synthetic_targets(n, D, False, seed + 1).cuda()


def _grads(enc):
    torch.cuda.synchronize()
    return {n: q.grad.detach().clone() for n, q in enc.named_parameters()}


def _done(enc):
    torch.cuda.synchronize()
    assert enc.engine.sync_errors() == 0


def _fused(enc, img, tgt):
    enc.engine.forward_train(img, tgt, motion=False, accumulate_loss=False)
    enc.engine.backward()
    return _grads(enc)


def _mse_de(enc, emb, tgt):
    """d(sum-MSE)/d(emb) by the library's own loss kernel: the very dpred the fused forward leaves in the workspace"""
    de = torch.empty_like(emb)
    eng = enc.engine
    eng.check(eng.L.vpd_op_mse(ptr(emb.detach()), ptr(tgt), emb.numel(), ptr(de), None, None, stream()), "vpd_op_mse")
    return de


# fp32 atomics add a block's partial sum onto the element in the order the blocks arrive: at most ~1,000 additions per element, each
# rounded to 2^-24 of a running sum that cancellation may leave ~100 x larger than the result: 1,000 x 100 x 6e-8 = 6e-6 of the
# tensor's norm at the very worst -- the floor under the measured run-to-run difference, and the cap on it
ATOMIC_ORDER_REL = 1e-5


def _assert_same(got, refs, arch, what):
    """got against the fused path's gradients (refs: three fused runs), tensor by tensor.  A tensor that _may_differ_run_to_run
    names -- whether or not the three runs happened to agree on it -- is held to the fused runs' own largest pairwise rel-L2 x 4,
    with the floor above; every other tensor to torch.equal, among the fused runs too.  Returns the tensors the fused runs
    differed in."""
    loose = []
    ref = refs[0]
    for n in ref:
        same = all(torch.equal(ref[n], r[n]) for r in refs[1:])
        if not same:
            loose.append(n)
        if _may_differ_run_to_run(arch, n, ref[n]):
            c = [r[n].cpu().numpy() for r in refs]
            own = max(rel_l2(c[1], c[0]), rel_l2(c[2], c[0]), rel_l2(c[2], c[1]))
            mine = rel_l2(got[n].cpu().numpy(), c[0])
            assert own <= ATOMIC_ORDER_REL and mine <= max(4 * own, ATOMIC_ORDER_REL), (what, n, own, mine)
        else:
            assert same, "%s: the fused path is not bitwise reproducible in %s" % (what, n)
            assert torch.equal(got[n], ref[n]), "%s: %s differs (%d elements, max %.3e)" % (
                what, n, int((got[n] != ref[n]).sum()), float((got[n] - ref[n]).abs().max()))
    return loose


# -- 1. equivalence with the fused path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,dtype,n,hw", [("resnet18", "bf16", N, HW), ("resnet18", "fp16", N, HW), ("resnet50", "bf16", 64, 128)])
def test_autograd_gradients_equal_the_fused_path(arch, dtype, n, hw):
    """fused: forward_train(img, tgt) + backward(); autograd: emb = enc(img), de = the library's d(sum-MSE)/d(emb), emb.backward(de):
    the same kernels on the same dpred.  ResNet-50 at 64 crops of 128: the Bottleneck tails are recomputed (vpd_op_conv1x1_bn)."""
    enc = _model(arch, dtype)
    if arch == "resnet50":
        g = torch.Generator().manual_seed(5)
        img, tgt = torch.randn(n, C_IN, hw, hw, generator=g).cuda(), torch.randn(n, D, generator=g).cuda()
    else:
        img, tgt = _batch(3, n, hw)
    fused = [_fused(enc, img, tgt) for _ in range(3)]
    enc.zero_grad()
    emb = enc(img)
    assert emb.requires_grad and emb.grad_fn is not None and tuple(emb.shape) == (n, D)
    emb.backward(_mse_de(enc, emb, tgt))
    ga = _grads(enc)
    assert set(ga) == set(fused[0]) and all(float(v.abs().max()) > 0 for v in ga.values())
    loose = _assert_same(ga, fused, arch, "%s %s" % (arch, dtype))
    _dump("autograd_vs_fused_%s_%s" % (arch, dtype), {"tensors": len(ga), "fused_differs_run_to_run": loose})
    print("the fused path differs run to run in:", loose)
    _done(enc)


# -- 2. a loss the fused path cannot express ----------------------------------------------------------------------------------
def _wellcond_sd(arch=ARCH):
    sd = O.reference_init_state_dict(arch, C_IN, D, 3)
    for k in sd:
        if k.endswith(".bn2.weight"):
            sd[k] = sd[k] * 0.1
    return sd


@functools.lru_cache(maxsize=None)
def _oracle_cosine(recipe):
    """fp32 CPU autograd of sum_i w_i (1 - cos(emb_i, t_i)) through the oracle's encoder: (loss, {name: grad}, d loss / d img)"""
    if recipe == "wellcond128":
        sd, img, tgt = _wellcond_sd(), O.synthetic_crops(N, C_IN, 128, 5), O.synthetic_targets(N, D, False, 6)
    else:
        sd = O.procedural_state_dict(O.encoder_schema(ARCH, C_IN, D), 1)
        img, tgt = O.synthetic_crops(N, C_IN, HW, 3), O.synthetic_targets(N, D, False, 4)
    orc = O.StudentOracle(ARCH, C_IN, D, False, sd)
    ps = [orc.enc[k].requires_grad_(True) for k in orc.enc_keys]
    x = img.clone().requires_grad_(True)
    loss = A.weighted_cosine_loss(O.encoder_forward(orc.enc, x, ARCH, True), tgt, A.crop_weights(N, 9))
    loss.backward()
    return float(loss.detach()), {k: p.grad.detach().clone() for k, p in zip(orc.enc_keys, ps)}, x.grad.detach().clone(), sd, img, tgt


def test_weighted_cosine_loss_matches_the_oracle_gradients():
    """fp16 library, the well-conditioned recipe of test_fp16_backward_matches_the_reference_gradients (reference init, last
    BatchNorm gamma of every block x 0.1, 8 crops of 128), held to that test's gates per stage: cos >= 0.99, projection 1 +- 2 %.
    Measured: cos 0.9982 (stem, layer1) ... 1.0000 (fc), projection 0.9958 (layer1) ... 1.0000 (fc), loss 9.99818 against 9.99884."""
    l_ref, g_ref, _, sd, img, tgt = _oracle_cosine("wellcond128")
    enc = _model(dtype="fp16", sd=sd)
    enc.zero_grad()
    emb = enc(img.cuda())
    loss = A.weighted_cosine_loss(emb, tgt.cuda(), A.crop_weights(N, 9).cuda())
    l_hip = loss.item()
    (loss * FP16_SCALE).backward()
    ga = {n: v / FP16_SCALE for n, v in _grads(enc).items()}
    res = _group_metrics(lambda n: ga[n].cpu(), lambda n: g_ref[n], list(g_ref))
    rec = {"loss": [l_hip, l_ref], "columns": ["rel_l2", "cos", "projection"], "hip_vs_oracle": {k: [round(x, 4) for x in v] for k, v in res.items()}}
    _dump("autograd_cosine_loss", rec)
    print(rec)
    assert abs(l_hip - l_ref) <= FP16_LOSS_TOL * abs(l_ref), rec["loss"]
    assert all(c >= 0.99 and abs(pj - 1) <= 0.02 for _, c, pj in res.values()), res
    _done(enc)


# -- 3. accumulation ----------------------------------------------------------------------------------------------------------
def _autograd_mse(enc, img, tgt):
    F.mse_loss(enc(img), tgt, reduction="sum").backward()


def test_backward_accumulates_as_torch_defines_it():
    from vpd_amd.trainer import ModelTrainer
    enc = _model()
    b1, b2 = _batch(3), _batch(13)
    enc.zero_grad()
    _autograd_mse(enc, *b1)
    g1 = _grads(enc)
    enc.zero_grad()
    _autograd_mse(enc, *b2)
    g2 = _grads(enc)
    assert not any(torch.equal(g1[n], g2[n]) for n in g1)
    # no clearing in between: one fp32 add per element
    enc.zero_grad()
    _autograd_mse(enc, *b1)
    _autograd_mse(enc, *b2)
    acc = _grads(enc)
    for n in g1:
        assert torch.equal(acc[n], g1[n] + g2[n]), n
    # zero_grad(set_to_none=True) in between: the views come back and hold the second batch's gradients alone
    enc.zero_grad()
    _autograd_mse(enc, *b1)
    enc.zero_grad(set_to_none=True)
    assert all(q.grad is None for q in enc.parameters())
    _autograd_mse(enc, *b2)
    g = _grads(enc)
    ptr0, eng = enc.engine._grads.data_ptr(), enc.engine
    assert all(ptr0 <= q.grad.data_ptr() < ptr0 + 4 * eng.param_numel for q in enc.parameters())
    for n in g2:
        assert torch.equal(g[n], g2[n]), n
    # zero_grad(set_to_none=False): zeros in place, the next backward adds onto them
    enc.zero_grad(set_to_none=False)
    _autograd_mse(enc, *b1)
    g = _grads(enc)
    for n in g1:
        assert torch.equal(g[n], g1[n]), n
    # FusedAdamW.zero_grad() touches no memory: the next autograd backward overwrites
    opt, _ = ModelTrainer(enc, False).get_optimizer(5e-4)
    opt.zero_grad()
    _autograd_mse(enc, *b2)
    g = _grads(enc)
    for n in g2:
        assert torch.equal(g[n], g2[n]), n
    _done(enc)


# -- 4. a torch optimizer end to end -----------------------------------------------------------------------------------------
def test_three_steps_of_torch_adamw_equal_the_fused_backward():
    from vpd_amd.trainer import ModelTrainer
    img, tgt = _batch(3)
    out = {}
    for kind in ("autograd", "fused"):
        enc = _model()
        tr = ModelTrainer(enc, False)
        opt = torch.optim.AdamW(enc.parameters(), lr=5e-4)
        for _ in range(3):
            if kind == "autograd":
                F.mse_loss(enc(img), tgt, reduction="sum").backward()
            else:
                tr._forward_loss(img, tgt, train=True).backward()
            opt.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        out[kind] = {n: q.detach().clone() for n, q in enc.named_parameters()}
        _done(enc)
    sd0 = O.procedural_state_dict(O.encoder_schema(ARCH, C_IN, D), 1)
    assert max(float((out["autograd"][n].cpu() - sd0[n]).abs().max()) for n in out["autograd"]) > 5e-4      # it moved
    for n in out["fused"]:
        assert torch.equal(out["autograd"][n], out["fused"][n]), n


# -- 5. the input gradient --------------------------------------------------------------------------------------------------
def test_input_gradient_matches_the_oracle_and_is_not_launched_unasked():
    """fp16 library, the 64-pixel fixture, the weighted cosine loss: img.grad as one more tensor under test_fp16_gpu.py's per-tensor
    gates (rel-L2 <= 0.45, cos >= 0.88).  Measured: rel-L2 0.144, cos 0.9897 (the stem convolution's weight gradient of the same pass:
    0.142, 0.9900).  Without requires_grad on the input the stem data gradient is not launched."""
    _, g_ref, dx_ref, sd, img, tgt = _oracle_cosine("fixture64")
    enc = _model(dtype="fp16", sd=sd)
    eng = enc.engine
    x = img.cuda().requires_grad_()
    enc.zero_grad()
    loss = A.weighted_cosine_loss(enc(x), tgt.cuda(), A.crop_weights(N, 9).cuda())
    assert eng.stem_dgrad_launches == 0
    (loss * FP16_SCALE).backward()
    torch.cuda.synchronize()
    assert eng.stem_dgrad_launches == 1 and x.grad is not None and tuple(x.grad.shape) == tuple(img.shape)
    dx = (x.grad / FP16_SCALE).cpu().numpy()
    gw = (enc.get_parameter("resnet.conv1.weight").grad / FP16_SCALE).cpu().numpy()
    rec = {"img_grad": [rel_l2(dx, dx_ref.numpy()), cosine(dx, dx_ref.numpy())],
           "conv1_weight_grad": [rel_l2(gw, g_ref["resnet.conv1.weight"].numpy()), cosine(gw, g_ref["resnet.conv1.weight"].numpy())],
           "columns": ["rel_l2", "cos"]}
    _dump("autograd_input_grad", rec)
    print(rec)
    assert np.isfinite(dx).all() and rec["img_grad"][0] <= 0.45 and rec["img_grad"][1] >= 0.88, rec
    # not asked for: no dx, no launch
    y = img.cuda()
    loss = A.weighted_cosine_loss(enc(y), tgt.cuda(), A.crop_weights(N, 9).cuda())
    (loss * FP16_SCALE).backward()
    torch.cuda.synchronize()
    assert eng.stem_dgrad_launches == 1 and y.grad is None
    # frozen parameters: the input gradient alone, .grad untouched
    before = _grads(enc)
    for q in enc.parameters():
        q.requires_grad_(False)
    z = img.cuda().requires_grad_()
    (A.weighted_cosine_loss(enc(z), tgt.cuda(), A.crop_weights(N, 9).cuda()) * FP16_SCALE).backward()
    torch.cuda.synchronize()
    assert eng.stem_dgrad_launches == 2 and torch.equal(z.grad, x.grad)
    assert all(torch.equal(q.grad, before[n]) for n, q in enc.named_parameters())
    _done(enc)


# -- 6. guards ---------------------------------------------------------------------------------------------------------------
def test_guards_of_a_plan_that_holds_one_forward():
    enc = _model()
    (ia, ta), (ib, tb) = _batch(3), _batch(13)
    la = F.mse_loss(enc(ia), ta, reduction="sum")
    eb = enc(ib)
    lb = F.mse_loss(eb, tb, reduction="sum")
    with pytest.raises(RuntimeError, match="later train-mode forward overwrote the activations"):
        la.backward()
    enc.zero_grad()
    lb.backward(retain_graph=True)
    gb = _grads(enc)
    with pytest.raises(RuntimeError, match="ran already"):
        lb.backward()
    enc.zero_grad()
    _autograd_mse(enc, ib, tb)
    g = _grads(enc)
    assert all(torch.equal(g[n], gb[n]) for n in g)
    # eval mode and no_grad: plain tensors, as before
    with torch.no_grad():
        e = enc(ia)
    assert e.grad_fn is None and not e.requires_grad
    enc.eval()
    e = enc(ia)
    assert e.grad_fn is None and not e.requires_grad
    enc.train()
    # a non-contiguous grad_output is made contiguous on the host
    enc.zero_grad()
    emb = enc(ib)
    de = (2 * (emb.detach() - tb)).t().contiguous().t()
    assert not de.is_contiguous()
    emb.backward(de)
    g = _grads(enc)
    assert all(torch.equal(g[n], gb[n]) for n in g)
    # a wrong shape / dtype / device cannot come from autograd: the engine's own check
    eng = enc.engine
    enc(ib)
    for bad in (torch.zeros(N, D + 1, device="cuda"), torch.zeros(N - 1, D, device="cuda"), torch.zeros(N, D, device="cuda", dtype=torch.float64),
                torch.zeros(N, D), torch.zeros(D, N, device="cuda").t()):
        with pytest.raises(AssertionError):
            eng.backward_ext(bad)
    eng.backward_ext(torch.zeros(N, D, device="cuda"))            # (the forward was not consumed by the refused calls)
    with pytest.raises(RuntimeError, match="ran already"):
        eng.backward_ext(torch.zeros(N, D, device="cuda"))
    # some .grad dropped, others kept: one pass cannot add onto some tensors and overwrite others
    enc.zero_grad(set_to_none=False)
    enc.get_parameter("resnet.fc.bias").grad = None
    with pytest.raises(RuntimeError, match="dropped and others kept"):
        _autograd_mse(enc, ib, tb)
    enc.zero_grad()
    # a forward that took no fp32 x (a staged batch: here what the last forward left in the staging buffer) has no input
    # gradient: the engine refuses, and so does the library, on the host
    eng.forward_train(None, None, motion=False, staged=(N, HW))
    with pytest.raises(RuntimeError, match="no fp32 x"):
        eng.backward_ext(torch.zeros(N, D, device="cuda"), want_dx=True)
    pl, de, dx = eng._last_fwd[0], torch.zeros(N, D, device="cuda"), torch.zeros(N, C_IN, HW, HW, device="cuda")
    rc = eng.L.vpd_backward_ext(pl.handle, ptr(eng.params), ptr(eng._grads), ptr(de), N, ptr(dx), None, ptr(pl.workspace), stream())
    assert rc != 0 and b"took x" in eng.L.vpd_last_error()
    eng.backward_ext(de)                                            # (without dx the staged forward differentiates)
    # the engine's own entry refuses a forward that a later one overwrote, too
    enc(ia)
    stale = eng._last_fwd
    enc(ib)
    with pytest.raises(RuntimeError, match="overwrote the activations"):
        eng.backward_ext(torch.zeros(N, D, device="cuda"), ticket=stale)
    _done(enc)
