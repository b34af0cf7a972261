"""End-to-end parity of the HIP student (through vpd_amd's reference-shaped
classes and the C ABI) against (a) the committed golden vectors produced by the
reference itself and (b) the CPU oracle on the same seeded inputs.

Tolerances (bf16 operands, fp32 accumulation / statistics / loss; the oracle
and the reference are fp32):
  embeddings ....... per-sample ||e - e_ref|| / ||e_ref||  <= EMB_TOL  = 2e-2
  loss ............. relative                               <= LOSS_TOL = 1e-2
  BN batch stats ... rel-L2                                 <= 1e-2
  gradients ........ bf16 storage of activations and of their gradients makes the
                     per-tensor gradient error vs the fp32 oracle LARGE on these tiny
                     batches (ReLU masks flip where |pre-activation| < 1 bf16 ulp; the
                     error compounds to 0.3-0.7 rel-L2 at the stem).  That is a property
                     of the precision, not of the kernels: the oracle's own
                     emulate_bf16 mode (same algorithm, same rounding points, computed
                     on the CPU) shows the same error.  Gate, for every trainable tensor:
                        err_hip  = relL2(g_hip,  g_fp32)
                        err_emul = relL2(g_emul, g_fp32)
                        err_hip <= 1.3 * err_emul + 0.15,  cos_hip >= cos_emul - 0.15
                     (loose: BN tensors have 64..512 elements and are individually noisy),
                     on average over the tensors  mean(err_hip - err_emul) <= 0.03 and
                     mean(cos_emul - cos_hip) <= 0.03, and over the whole flat gradient
                        err_hip_all <= 1.15 * err_emul_all + 0.01.
                     Kernel-level gradient parity at 4e-3 is in tests/test_ops_gpu.py.
  AdamW ............ injected identical grads: <= 1e-6 absolute (fp32 kernel)
"""
import glob
import json
import os

import numpy as np
import pytest
import torch

from oracle import vpd_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
# (c2_ / c3_ / c5_: the full-size cases of tests/test_fullsize_gpu.py -- minutes of CPU oracle time each, not run here)
CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*r[0-9]*_c[0-9]_*.npz"))
               if not os.path.basename(p).startswith(("c2_", "c3_", "c5_")))
EMB_TOL, LOSS_TOL = 2e-2, 1e-2
OUT = os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out")


def rel_l2(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def cosine(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))


def per_sample_rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-30)


def build(meta):
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    enc_sd = O.procedural_state_dict(O.encoder_schema(meta["arch"], meta["c_in"], meta["emb_dim"]), meta["seed"])
    dec_sd = O.procedural_state_dict(O.decoder_schema(meta["emb_dim"]), meta["seed"] + 7) if meta["motion"] else None
    img = O.synthetic_crops(meta["n"], meta["c_in"], meta["hw"], meta["seed"] + 1)
    tgt = O.synthetic_targets(meta["n"], meta["emb_dim"], meta["motion"], meta["seed"] + 2)
    enc = RGBF_EmbeddingModel(meta["arch"], meta["emb_dim"], meta["c_in"] != 3, "cuda",
                              in_channels=None if meta["c_in"] in (3, 5) else meta["c_in"])
    enc.load_state_dict(enc_sd)
    tr = ModelTrainer(enc, meta["motion"])
    if meta["motion"]:
        tr.fcn_time.load_state_dict(dec_sd)
    orc = O.StudentOracle(meta["arch"], meta["c_in"], meta["emb_dim"], meta["motion"], enc_sd, dec_sd)
    return enc, tr, orc, img, tgt


def build_oracle(meta):
    enc_sd = O.procedural_state_dict(O.encoder_schema(meta["arch"], meta["c_in"], meta["emb_dim"]), meta["seed"])
    dec_sd = O.procedural_state_dict(O.decoder_schema(meta["emb_dim"]), meta["seed"] + 7) if meta["motion"] else None
    return O.StudentOracle(meta["arch"], meta["c_in"], meta["emb_dim"], meta["motion"], enc_sd, dec_sd)


def _dump(name, rec):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "parity_%s.json" % name), "w") as fp:
        json.dump(rec, fp, indent=1)


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_student_matches_reference_and_oracle(path):
    g = np.load(path)
    meta = json.loads(str(g["meta"]))
    rec = {"meta": meta}
    enc, tr, orc, img, tgt = build(meta)

    # state_dict schema: same keys, shapes, dtypes as the reference's
    sd = enc.state_dict()
    sch = O.encoder_schema(meta["arch"], meta["c_in"], meta["emb_dim"])
    assert list(sd.keys()) == list(sch.keys())
    for k, (shape, kind) in sch.items():
        assert tuple(sd[k].shape) == tuple(shape)
        assert sd[k].dtype == (torch.int64 if kind == "bn_nbt" else torch.float32)

    # (1) eval-mode embed(): numpy f32 [N, D] vs the reference's golden output
    e = enc.embed(img.numpy())
    assert isinstance(e, np.ndarray) and e.dtype == np.float32 and e.shape == g["emb_eval"].shape
    rec["emb_eval_per_sample"] = per_sample_rel(e, g["emb_eval"]).tolist()
    # eval epoch value (optimizer=None)
    ev = tr.epoch([{"img": img, "emb": tgt}])
    rec["epoch_eval"] = [ev, float(g["epoch_eval"])]

    # (2) train-mode forward + loss + backward, gradients vs the oracle (full tensors)
    enc, tr, orc, img, tgt = build(meta)
    enc.train()
    loss = tr._forward_loss(img, tgt, train=True)
    l_hip = loss.item()
    loss.backward()
    torch.cuda.synchronize()
    l_ref, emb_ref, out_ref, grads_ref = orc.forward_loss(img, tgt, train=True, need_grad=True)
    orc2 = build_oracle(meta)
    l_emu, _, _, grads_emu = orc2.forward_loss(img, tgt, train=True, need_grad=True, emulate_bf16=True)
    rec["loss_train"] = [l_hip, l_ref, float(g["loss_train"]), l_emu]
    grad_err, grad_bad = {}, {}
    flat = {"hip": [], "emu": [], "ref": []}
    for name, gref in grads_ref.items():
        if name.startswith("enc."):
            got = enc.get_parameter(name[4:]).grad
        else:
            got = tr.fcn_time.get_parameter(name[4:]).grad
        got = got.detach().cpu().numpy()
        e_hip, e_emu = rel_l2(got, gref.numpy()), rel_l2(grads_emu[name].numpy(), gref.numpy())
        c_hip, c_emu = cosine(got, gref.numpy()), cosine(grads_emu[name].numpy(), gref.numpy())
        grad_err[name] = [round(e_hip, 4), round(e_emu, 4), round(c_hip, 4), round(c_emu, 4)]
        # where the emulation itself is noise-dominated (error > 0.7: deep students on these tiny batches, and the stem's
        # BatchNorm bias of the 8-crop 64-pixel case, 0.74) the direction carries no information: only the magnitude is gated
        # there, and the backward pass is pinned by test_gradient_is_derivative_of_loss instead; the stem's own kernels (pool routing,
        # ReLU mask, dgamma / dbeta sums, dz) are pinned per launch against float64 by tests/test_stem_ops_gpu.py.  (Round 6: with the K chunks of a
        # 3x3 tile summed in rotated order -- HaloGeom::rot -- that tensor's cosine moved from 0.66 to 0.62 against the
        # emulation's 0.79: two samples of the same rounding noise, the summation order is the only difference.)
        ok = e_hip <= 1.3 * e_emu + 0.15 and (c_hip >= c_emu - 0.15 or e_emu > 0.7)
        if not ok:
            grad_bad[name] = grad_err[name]
        flat["hip"].append(got.ravel()); flat["emu"].append(grads_emu[name].numpy().ravel()); flat["ref"].append(gref.numpy().ravel())
        # golden: gradient norms recorded from the reference itself pin the fp32 oracle's gradients (this host's
        # CPU convolutions vs the authoring container's: 1e-3; the 50-layer Bottleneck cases at 64x64 end in 2x2
        # maps whose batch statistics are over 20-24 values, which amplifies that rounding difference: 1e-2)
        gn_tol = 1e-2 if meta["arch"] in ("resnet50", "resnet101", "wide_resnet50_2", "wide_resnet101_2") else 1e-3
        assert abs(float(gref.double().norm()) - float(g["gnorm/" + name])) <= gn_tol * float(g["gnorm/" + name]) + 1e-9
    rec["grad_err_hip_emul_cos"] = grad_err
    ge = np.asarray(list(grad_err.values()))
    rec["grad_mean_excess_err"] = float((ge[:, 0] - ge[:, 1]).mean())
    rec["grad_mean_cos_deficit"] = float((ge[:, 3] - ge[:, 2]).mean())
    fl = {k: np.concatenate(v) for k, v in flat.items()}
    rec["grad_flat_err"] = [rel_l2(fl["hip"], fl["ref"]), rel_l2(fl["emu"], fl["ref"])]
    # running statistics after one train-mode forward vs golden (reference after one step)
    rs_err, rs_emu = {}, {}
    sd = enc.state_dict()
    for k in [k for k in g.files if k.startswith("post/")]:
        name = k.split("/", 1)[1]
        if name.endswith("num_batches_tracked"):
            assert int(sd[name]) == int(g[k])
        else:
            rs_err[name] = rel_l2(sd[name].cpu().numpy(), g[k])
            rs_emu[name] = rel_l2(orc2.enc[name].numpy(), g[k])      # the bf16 emulation's running stats
    rec["running_stats_rel_l2_max"] = max(rs_err.values())
    rec["running_stats_rel_l2_max_emul"] = max(rs_emu.values())

    # (3) three train steps through ModelTrainer.epoch / get_optimizer / step
    enc, tr, orc, img, tgt = build(meta)
    optimizer, scaler = tr.get_optimizer(meta["lr"])
    assert scaler is None
    traj = [tr.epoch([{"img": img, "emb": tgt}], optimizer=optimizer, scaler=scaler) for _ in range(3)]
    rec["epoch_traj"] = [traj, g["epoch_traj"].tolist()]
    _dump(meta["name"], rec)

    assert max(rec["emb_eval_per_sample"]) <= EMB_TOL, rec["emb_eval_per_sample"]
    assert abs(ev - float(g["epoch_eval"])) <= LOSS_TOL * abs(float(g["epoch_eval"]))
    assert abs(l_hip - float(g["loss_train"])) <= LOSS_TOL * abs(float(g["loss_train"]))
    # 2e-2 for the 18/34-layer students; deeper ones are held to what the bf16 emulation of the same algorithm shows
    assert rec["running_stats_rel_l2_max"] <= max(2e-2, 1.3 * rec["running_stats_rel_l2_max_emul"]), \
        (rec["running_stats_rel_l2_max"], rec["running_stats_rel_l2_max_emul"])
    assert not grad_bad, grad_bad
    # (the 50-layer cases sit in the chaotic regime described in test_backward_in_a_well_conditioned_regime, where
    #  HIP and the emulation are two different samples of the same noise: a wider band there)
    band = 0.06 if gn_tol == 1e-2 else 0.03
    assert rec["grad_mean_excess_err"] <= band and rec["grad_mean_cos_deficit"] <= band, rec
    assert rec["grad_flat_err"][0] <= 1.15 * rec["grad_flat_err"][1] + 0.01, rec["grad_flat_err"]
    assert abs(traj[0] - float(g["epoch_traj"][0])) <= LOSS_TOL * abs(traj[0])
    # later steps depend on sign-like Adam updates: the trajectory must fall alike, within 5 % of
    # the initial loss at every step
    assert np.max(np.abs(np.asarray(traj) - g["epoch_traj"])) <= 0.05 * float(g["epoch_traj"][0]), \
        (traj, g["epoch_traj"].tolist())


@pytest.mark.parametrize("arch", ["resnet18", "resnet34", "resnet50", "wide_resnet50_2"])
def test_backward_in_a_well_conditioned_regime(arch):
    """Whole-network backward parity where bf16 rounding cannot hide an orchestration error.

    At the reference's initialisation an untrained ResNet is chaotic in its early-layer gradients: rounding only the
    conv WEIGHTS to bf16 (what any mixed-precision run does, the reference's fp16 autocast included) already turns the
    stem/layer1 gradient of ResNet-50 to cos 0.36 against fp32 (0.92 for ResNet-34), rounding the stored activations
    to 0.12 (0.82); rounding the activation GRADIENTS changes nothing (cos 1.000) -- measured with the CPU oracle's
    emulate_bf16 switches, and the same for the HIP path (tests above compare the two).  Scaling the last BatchNorm
    gamma of every residual branch to 0.1 (a "nearly zero-init-residual" network) removes the chaos -- the emulation then
    agrees with fp32 to cos >= 0.96 in every stage -- while every conv, BN, residual add and downsample branch still
    receives gradient.  In that regime the HIP gradients must match the fp32 oracle group by group:
    cos >= 0.93 and projection <g_hip, g_ref> / |g_ref|^2 within 10 % of 1."""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    sd = O.reference_init_state_dict(arch, 5, 32, 3)
    last = ".bn3.weight" if O.arch_expansion(arch) == 4 else ".bn2.weight"
    for k in sd:
        if k.endswith(last):
            sd[k] = sd[k] * 0.1
    enc = RGBF_EmbeddingModel(arch, 32, True, "cuda")
    enc.load_state_dict(sd)
    tr = ModelTrainer(enc, False)
    orc = O.StudentOracle(arch, 5, 32, False, sd, None)
    img, tgt = O.synthetic_crops(8, 5, 128, 5), O.synthetic_targets(8, 32, False, 6)
    enc.train()
    loss = tr._forward_loss(img, tgt, train=True)
    l_hip = loss.item()
    loss.backward()
    torch.cuda.synchronize()
    l_ref, _, _, grads_ref = orc.forward_loss(img, tgt, train=True, need_grad=True)
    assert abs(l_hip - l_ref) <= 5e-3 * l_ref, (l_hip, l_ref)
    acc = {k: [0.0, 0.0, 0.0] for k in ("stem", "layer1", "layer2", "layer3", "layer4", "fc")}
    for name, p in enc.named_parameters():
        key = "fc" if ".fc." in name else (name.split(".")[1] if name.split(".")[1].startswith("layer") else "stem")
        r = grads_ref["enc." + name].double().flatten()
        gh = p.grad.detach().cpu().double().flatten()
        acc[key][0] += float((gh * r).sum()); acc[key][1] += float((r * r).sum()); acc[key][2] += float((gh * gh).sum())
    res = {k: (round(v[0] / (v[1] * v[2]) ** 0.5, 3), round(v[0] / v[1], 3)) for k, v in acc.items()}      # (cos, projection)
    assert all(c >= 0.93 and 0.9 <= b <= 1.1 for c, b in res.values()), res


def test_reset_parameters_matches_reference_init_statistics():
    """Rows a3 / a4: the PRODUCT's initialisation (RGBF_EmbeddingModel.reset_parameters, FCNet) against
    statistics of freshly constructed reference models (tests/golden/init_stats.json from oracle/gen_golden.py;
    reference models/rgb.py:8-43, models/module.py:71-76, :139-150): per-tensor kaiming std, the identical stem slices
    of add_flow_to_model, nn.Linear bounds of replace_last_layer / FCNet, BN tensors and buffers exactly."""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    ref = json.load(open(os.path.join(GOLDEN, "init_stats.json")))
    for tag, (arch, c_in, D) in {"r34_c5_d128": ("resnet34", 5, 128), "r18_c3_d32": ("resnet18", 3, 32),
                                 "r50_c5_d32": ("resnet50", 5, 32)}.items():
        rows = ref[tag]
        torch.manual_seed(99)
        enc = RGBF_EmbeddingModel(arch, D, c_in == 5, "cuda")      # the constructor initialises (no explicit reset)
        sd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
        assert list(sd.keys()) == [k for k in O.encoder_schema(arch, c_in, D).keys()]
        assert set(sd.keys()) == {k for k in rows if not k.startswith("__")}
        for k, v in sd.items():
            r = rows[k]
            kind = O.encoder_schema(arch, c_in, D)[k][1]
            assert list(v.shape) == r["shape"] and str(v.dtype) == r["dtype"], (tag, k)
            if kind == "conv":
                n = v.numel() // (c_in if (k == "resnet.conv1.weight" and c_in != 3) else 1)
                assert abs(float(v.double().std()) / r["std"] - 1) < 10.0 / (2 * n) ** 0.5 + 0.02, (tag, k)
                assert abs(float(v.double().mean()) - r["mean"]) < 6 * r["std"] / n ** 0.5, (tag, k)
            elif kind.startswith("bn"):
                assert float(v.double().min()) == r["min"] and float(v.double().max()) == r["max"], (tag, k)
            else:
                b = rows["__fc__"]["bound"]
                assert float(v.min()) >= -b and float(v.max()) <= b, (tag, k)
                if v.numel() >= 4096:
                    assert float(v.max()) > 0.9 * b and abs(float(v.double().std()) / r["std"] - 1) < 0.05, (tag, k)
        w = sd["resnet.conv1.weight"]
        if c_in != 3:
            assert rows["__stem__"]["slices_identical"] and bool((w == w[:, :1]).all())
            assert abs(float(w.double().std()) / rows["resnet.conv1.weight"]["std"] - 1) < 0.1
    enc = RGBF_EmbeddingModel("resnet18", 128, True, "cuda")
    tr = ModelTrainer(enc, True)
    fr = ref["fcnet_d128"]
    dsd = {k: v.detach().cpu() for k, v in tr.fcn_time.state_dict().items()}
    assert list(dsd.keys()) == list(O.decoder_schema(128).keys()) and set(dsd.keys()) == set(fr.keys())
    for k, v in dsd.items():
        fan_in = v.shape[1] if v.dim() == 2 else {"layers.0.bias": 128, "layers.2.bias": 128, "layers.5.bias": 128}[k]
        b = 1.0 / fan_in ** 0.5
        assert list(v.shape) == fr[k]["shape"] and float(v.min()) >= -b and float(v.max()) <= b
        assert fr[k]["min"] >= -b and fr[k]["max"] <= b
        if v.numel() >= 4096:
            assert abs(float(v.double().std()) / fr[k]["std"] - 1) < 0.05, k
    # 6-channel variant (BASELINE configs[2]): the same stem recipe with 6 slices
    enc6 = RGBF_EmbeddingModel("resnet18", 32, True, "cuda", in_channels=6)
    w6 = enc6.state_dict()["resnet.conv1.weight"].cpu()
    assert tuple(w6.shape) == (64, 6, 7, 7) and bool((w6 == w6[:, :1]).all())
    with pytest.raises(AssertionError):
        enc6.embed(np.zeros((1, 5, 64, 64), np.float32))
    assert enc6.embed(np.zeros((6, 64, 64), np.float32)).shape == (1, 32)


_STEP_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, {repo!r})
from oracle import vpd_oracle as O
from vpd_amd.models.rgb import RGBF_EmbeddingModel
from vpd_amd.trainer import ModelTrainer
sd = O.reference_init_state_dict({arch!r}, 5, 32, 3)
enc = RGBF_EmbeddingModel({arch!r}, 32, True, "cuda")
enc.load_state_dict(sd)
tr = ModelTrainer(enc, False)
g = torch.Generator(device="cuda").manual_seed(4)
img = torch.randn(({n}, 5, 128, 128), generator=g, device="cuda")
tgt = torch.randn(({n}, 32), generator=g, device="cuda")
enc.train()
loss = tr._forward_loss(img, tgt, train=True)
loss.backward()
torch.cuda.synchronize()
assert enc.engine.sync_errors() == 0
np.save({out!r}, enc.engine.grads.cpu().numpy())
print("LOSS", loss.item())
"""


@pytest.mark.parametrize("arch,n", [("resnet34", 256), ("resnet50", 64)])
def test_batchnorm_backward_sums_taken_by_the_data_gradient(tmp_path, arch, n):
    """Default path: the stride-1 3x3 data gradients of layers 2-4 add sum g and sum g*z of the BatchNorm that consumes
    their output to its rows (conv_epilogue.h, EPM 6 / 7) and the BatchNorm launch only finalizes and applies
    (bn_bwd_apply_fused_kernel); VPD_DGRAD_SUMS=0 is the separate reduce + barrier + apply launch.  Same g, same bf16
    rounding points; the sums differ in their summation order and in sum g*xhat being formed from sum g*z in fp64.
    resnet50: layer3 / layer4's conv3 and conv2 data gradients -- 1x1 on the ring GEMM / gather kernel (mode 6) and
    3x3 -- carry the sums of bn2 / bn1 there."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for flag in ("0", "1"):
        out = str(tmp_path / ("g%s.npy" % flag))
        env = dict(os.environ, VPD_DGRAD_SUMS=flag)
        r = subprocess.run([sys.executable, "-c", _STEP_SCRIPT.format(repo=repo, out=out, arch=arch, n=n)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        outs.append((np.load(out), float(r.stdout.split("LOSS")[1].split()[0])))
    (g0, l0), (g1, l1) = outs
    assert l0 == l1
    assert np.isfinite(g1).all() and np.abs(g1).max() > 0
    cos = float(np.dot(g0.astype(np.float64), g1.astype(np.float64)) / (np.linalg.norm(g0) * np.linalg.norm(g1)))
    assert cos > 0.999 and abs(np.linalg.norm(g1) / np.linalg.norm(g0) - 1) < 1e-2, (cos, rel_l2(g1, g0))


def _wc_sample_idx(numel, k=512):
    return np.unique(np.linspace(0, numel - 1, k).astype(np.int64))      # oracle/gen_golden.py::sample_idx


# Gate of test_backward_matches_the_reference_gradients: HIP (bf16 operands) against the REFERENCE's fp32 gradients, per stage
WC_COS_MIN, WC_PROJ_TOL = 0.95, 0.06


@pytest.mark.parametrize("arch", ["resnet18", "resnet34", "resnet50"])
def test_backward_matches_the_reference_gradients(arch):
    """VERDICT r2 (parity soft spot 1): the HIP gradients against numbers the REFERENCE itself produced -- not the oracle's
    restatement: tests/golden/wc_grads_<arch>.npz holds 512 evenly spaced elements of every parameter's gradient from the
    reference's own modules (oracle/gen_golden.py::wellcond_case: models/rgb.py:46-70, models/module.py:35-130, sum-MSE
    train_vpd_model.py:87), summed over three 8-crop batches, in the well-conditioned regime (last BatchNorm gamma of every
    residual branch x 0.1) where bf16 rounding noise is small against the gradient.  Per network stage, on the sampled
    coordinates (10-20 k per stage: the sampling error of a projection is ~1e-3): cosine >= 0.95 and projection
    <g_hip, g_ref> / |g_ref|^2 = 1 +- 6 % (fp32 reference vs bf16 path; the same-precision gate is the emulation test below),
    losses within 5e-3."""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    g = np.load(os.path.join(GOLDEN, "wc_grads_%s.npz" % arch))
    sd = O.reference_init_state_dict(arch, 5, 32, 3)
    last = ".bn3.weight" if O.arch_expansion(arch) == 4 else ".bn2.weight"
    for k in sd:
        if k.endswith(last):
            sd[k] = sd[k] * 0.1
    enc = RGBF_EmbeddingModel(arch, 32, True, "cuda")
    tr = ModelTrainer(enc, False)
    acc, losses = {}, []
    for b in range(3):
        enc.load_state_dict(sd)                               # fresh running statistics, as in the golden
        enc.train()
        img, tgt = O.synthetic_crops(8, 5, 128, 5 + 10 * b), O.synthetic_targets(8, 32, False, 6 + 10 * b)
        loss = tr._forward_loss(img, tgt, train=True)
        losses.append(loss.item())
        loss.backward()
        torch.cuda.synchronize()
        for n, q in enc.named_parameters():
            acc[n] = acc.get(n, 0.0) + q.grad.detach().cpu().double()
    for lh, lr in zip(losses, g["losses"]):
        assert abs(lh - lr) <= 5e-3 * lr, (losses, g["losses"])
    stage = {}
    for n in acc:
        ref = g["gsamp/" + n].astype(np.float64)
        mine = acc[n].reshape(-1)[torch.from_numpy(_wc_sample_idx(acc[n].numel()))].numpy()
        v = stage.setdefault(_group_of(n), [0.0, 0.0, 0.0])
        v[0] += float((mine * ref).sum()); v[1] += float((ref * ref).sum()); v[2] += float((mine * mine).sum())
    res = {k: (round(v[0] / (v[1] * v[2]) ** 0.5, 4), round(v[0] / v[1], 4)) for k, v in stage.items()}      # (cos, projection)
    _dump("reference_grads_%s" % arch, {"arch": arch, "columns": ["cos", "projection"], "hip_vs_reference": res})
    print(res)
    assert all(c >= WC_COS_MIN and abs(pj - 1) <= WC_PROJ_TOL for c, pj in res.values()), res


_BUSY_SCRIPT = r"""
import sys, json, numpy as np, torch
sys.path.insert(0, {repo!r})
from oracle import vpd_oracle as O
from vpd_amd.models.rgb import RGBF_EmbeddingModel
from vpd_amd.trainer import ModelTrainer
sd = O.reference_init_state_dict({arch!r}, 5, 32, 3)
g = torch.Generator(device="cuda").manual_seed(4)
img = torch.randn(({n}, 5, 128, 128), generator=g, device="cuda")
tgt = torch.randn(({n}, 32), generator=g, device="cuda")
side = torch.cuda.Stream()
a = torch.randn((8192, 8192), device="cuda")
b = torch.randn((8192, 8192), device="cuda")
c = torch.empty_like(a)
res = {{}}
for mode in ("quiet", "busy"):
    enc = RGBF_EmbeddingModel({arch!r}, 32, True, "cuda")
    enc.load_state_dict(sd)
    tr = ModelTrainer(enc, False)
    opt, sc = tr.get_optimizer(5e-4)
    enc.train()
    tr._forward_loss(img, tgt, train=True).backward()       # plan + workspace outside the contended region
    enc.load_state_dict(sd)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]      # side start / end, steps start / end
    if mode == "busy":
        with torch.cuda.stream(side):                        # fp32 GEMMs of 1.1 TFLOP each: every CU busy for ~1 s
            ev[0].record(side)
            for _ in range(150):
                torch.mm(a, b, out=c)
            ev[1].record(side)
    ev[2].record()
    losses = []
    from vpd_amd.models.util import step
    for it in range(4):
        loss = tr._forward_loss(img, tgt, train=True)
        step(opt, sc, loss)
        losses.append(loss.item())                           # host sync per step, like the reference loop
    ev[3].record()
    torch.cuda.synchronize()
    steps_ms = ev[2].elapsed_time(ev[3])
    # share of the steps' time during which the side stream was still working
    shared = max(0.0, min(ev[2].elapsed_time(ev[1]), steps_ms) - max(ev[2].elapsed_time(ev[0]), 0.0)) / steps_ms if mode == "busy" else 0.0
    res[mode] = dict(losses=losses, steps_ms=steps_ms, shared=shared, errors=enc.engine.sync_errors(),
                     params=float(enc.engine.params.double().norm().item()))
print("RESULT " + json.dumps(res))
"""


@pytest.mark.parametrize("arch,n,env", [("resnet34", 256, {"VPD_DGRAD_SUMS": "0"}), ("resnet50", 64, {"VPD_DGRAD_SUMS": "0"}),
                                        # the same with 16 CUs reserved (vpd_cu_budget: every persistent grid and the
                                        # grid barrier sized to 240 CUs) -- the co-runner finds CUs whose LDS the step never takes
                                        ("resnet34", 256, {"VPD_DGRAD_SUMS": "0", "VPD_RESERVE_CUS": "16"})],
                         ids=["r34_every_bn_backward_with_a_barrier", "r50_every_bn_backward_with_a_barrier",
                              "r34_every_bn_backward_with_a_barrier_16_cus_reserved"])
def test_grid_barrier_kernels_on_a_busy_device(arch, n, env):
    """VERDICT r2 #5b: the fused BatchNorm backward (bn_bwd_fused_kernel, vpd_amd/csrc/sync.h) is an ordinary launch with an
    in-launch grid barrier: its blocks must all become resident while another stream's kernels (RCCL's all-reduce under
    data parallelism, here something far heavier: a queue of fp32 GEMMs that keeps every CU busy for the whole time) compete
    for the CUs.  Four optimizer steps run while the side stream is busy (checked with events: the GEMM queue is at work during
    most of the steps' time, and the steps take longer than alone): no barrier time-out (vpd_plan_sync_errors), and the losses equal the quiet run's --
    a block that left the barrier early would read incomplete sums.  VPD_DGRAD_SUMS=0 routes EVERY BatchNorm backward
    through the barrier kernel (~36 launches per ResNet-34 step instead of one)."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _BUSY_SCRIPT.format(repo=repo, arch=arch, n=n)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(res)
    # contended: the side stream worked during most of the steps' time, and the steps took visibly longer than alone
    assert res["busy"]["shared"] > 0.6 and res["busy"]["steps_ms"] > 1.5 * res["quiet"]["steps_ms"], res
    assert res["quiet"]["errors"] == 0 and res["busy"]["errors"] == 0, res
    # (the fp64 row atomics arrive in another order under contention: last-bit differences that an untrained network
    #  amplifies from step to step -- DESIGN.md, "Run-to-run reproducibility"; the first loss precedes any backward)
    assert res["quiet"]["losses"][0] == res["busy"]["losses"][0], res
    for lq, lb in zip(res["quiet"]["losses"], res["busy"]["losses"]):
        assert abs(lq - lb) <= 1e-2 * abs(lq), res
    assert abs(res["busy"]["params"] / res["quiet"]["params"] - 1) < 1e-4, res


def _group_of(name):
    return "fc" if ".fc." in name else (name.split(".")[1] if name.split(".")[1].startswith("layer") else "stem")


def _group_metrics(get_a, get_b, names):
    """per network stage over the concatenated tensors of the stage: (rel-L2 of a against b, cosine, projection
    <a, b> / <b, b>)"""
    acc = {}
    for name in names:
        a, b = get_a(name).double().flatten(), get_b(name).double().flatten()
        v = acc.setdefault(_group_of(name), [0.0, 0.0, 0.0, 0.0])
        v[0] += float(((a - b) ** 2).sum()); v[1] += float((b * b).sum()); v[2] += float((a * b).sum()); v[3] += float((a * a).sum())
    return {k: ((v[0] / v[1]) ** 0.5, v[2] / (v[1] * v[3]) ** 0.5, v[2] / v[1]) for k, v in acc.items()}


# Gate of test_backward_matches_bf16_emulation_directly: per stage, the PROJECTION of the HIP gradient on the emulation's
# gradient must be 1 within PROJ_TOL and the cosine at least COS_MIN.
PROJ_TOL, COS_MIN = 0.025, 0.985


@pytest.mark.parametrize("arch", ["resnet18", "resnet34", "resnet50"])
def test_backward_matches_bf16_emulation_directly(arch):
    """the HIP gradients DIRECTLY against the oracle's emulate_bf16 gradients (same algorithm, same
    rounding points, on the CPU), stage by stage, in the well-conditioned regime, summed over three independent batches.

    What can be gated.  Measured (profiles/r02_parity_direct.json): the two gradients differ by 0.07-0.14 rel-L2 per
    stage at cos 0.990-0.997 -- NOT the 2e-2 one might expect from "same rounding points".  The fp32 accumulation order
    differs between an MFMA tile loop and a CPU convolution, so ~1 % of the bf16-rounded activations differ by one ulp,
    and every such flip re-draws the downstream rounding noise (the same chaos that separates either of them from fp32
    by 0.1-0.2): HIP and the emulation are two SAMPLES of one noise distribution, not two computations of one number.
    That noise is zero-mean and incoherent with the gradient, while an orchestration error (a residual path scaled
    wrongly, a missing term) is a coherent bias; so the gate is on the projection <g_hip, g_emu> / |g_emu|^2 per stage,
    in which the incoherent part averages out over 10^5-10^7 elements and three batches: it must be 1 +- 2.5 %.
    Resolution of the gate, proven here: the same metric applied to an emulation whose layer2.1 identity-path
    gradient is scaled by 1.05 (a 5 % error in ONE residual path) reads 1.044-1.050 on the stages upstream of the fault:
    red."""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    sd = O.reference_init_state_dict(arch, 5, 32, 3)
    last_bn = ".bn3.weight" if any(k.endswith(".bn3.weight") for k in sd) else ".bn2.weight"      # Bottleneck / BasicBlock
    for k in sd:
        if k.endswith(last_bn):
            sd[k] = sd[k] * 0.1
    enc = RGBF_EmbeddingModel(arch, 32, True, "cuda")
    enc.load_state_dict(sd)
    tr = ModelTrainer(enc, False)
    names = [n for n, _ in enc.named_parameters()]
    g_hip = {n: 0.0 for n in names}
    g_emu = {n: 0.0 for n in names}
    g_bad = {n: 0.0 for n in names}
    for b in range(3):
        img, tgt = O.synthetic_crops(8, 5, 128, 5 + 10 * b), O.synthetic_targets(8, 32, False, 6 + 10 * b)
        enc.load_state_dict(sd)                               # fresh running statistics: every batch from the same state
        enc.train()
        loss = tr._forward_loss(img, tgt, train=True)
        loss.backward()
        torch.cuda.synchronize()
        emu = O.StudentOracle(arch, 5, 32, False, sd, None)
        _, _, _, ge = emu.forward_loss(img, tgt, train=True, need_grad=True, emulate_bf16=True)
        O.GRAD_FAULT["resnet.layer2.1"] = 1.05              # the faulty emulation: identical except for one residual path
        try:
            bad = O.StudentOracle(arch, 5, 32, False, sd, None)
            _, _, _, gb = bad.forward_loss(img, tgt, train=True, need_grad=True, emulate_bf16=True)
        finally:
            O.GRAD_FAULT.clear()
        for n, p in enc.named_parameters():
            g_hip[n] = g_hip[n] + p.grad.detach().cpu().double()
            g_emu[n] = g_emu[n] + ge["enc." + n].double()
            g_bad[n] = g_bad[n] + gb["enc." + n].double()
    direct = _group_metrics(lambda n: g_hip[n], lambda n: g_emu[n], names)
    fault = _group_metrics(lambda n: g_bad[n], lambda n: g_emu[n], names)
    rec = {"arch": arch, "columns": ["rel_l2", "cos", "projection"],
           "hip_vs_emulation": {k: [round(x, 5) for x in v] for k, v in direct.items()},
           "faulty_emulation_vs_emulation": {k: [round(x, 5) for x in v] for k, v in fault.items()}}
    _dump("direct_%s" % arch, rec)
    print(rec)
    for k, (err, cos, proj) in direct.items():
        assert abs(proj - 1) <= PROJ_TOL and cos >= COS_MIN, (k, err, cos, proj, rec)
    # resolution: the 5 % fault in one residual path is caught by the same gate
    red = [k for k, (err, cos, proj) in fault.items() if abs(proj - 1) > PROJ_TOL]
    assert {"stem", "layer1"} <= set(red), rec


@pytest.mark.parametrize("motion", [False, True])
def test_training_trajectory_tracks_fp32_oracle(motion):
    """Twelve real AdamW steps (3 epochs x 4 batches of 16 crops, ResNet-18, the well-conditioned initialisation of the
    test above) through ModelTrainer.epoch, against the fp32 oracle taking the same steps on the CPU: per-epoch train
    loss within 1 %, the eval-mode loss afterwards (running statistics after 12 updates) within 1 %.  Adam's first
    steps are sign-like (m/sqrt(v) = +-1), so rounding noise in near-zero gradient coordinates moves those weights by a
    full +-lr: the trained weights and the held-out embeddings are therefore gated against what the oracle's own bf16
    emulation (same algorithm, same rounding points, CPU) shows for the same 12 steps --
    err_hip <= 1.5 * err_emulation + 1e-2 for both."""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    D = 32
    sd = O.reference_init_state_dict("resnet18", 5, D, 11)
    for k in sd:
        if k.endswith(".bn2.weight"):
            sd[k] = sd[k] * 0.1
    dec_sd = O.procedural_state_dict(O.decoder_schema(D), 12) if motion else None
    enc = RGBF_EmbeddingModel("resnet18", D, True, "cuda")
    enc.load_state_dict(sd)
    tr = ModelTrainer(enc, motion)
    if motion:
        tr.fcn_time.load_state_dict(dec_sd)
    orc = O.StudentOracle("resnet18", 5, D, motion, sd, dec_sd)
    batches = [{"img": O.synthetic_crops(16, 5, 64, 20 + i), "emb": O.synthetic_targets(16, D, motion, 40 + i)}
               for i in range(4)]
    held = [{"img": O.synthetic_crops(16, 5, 64, 77), "emb": O.synthetic_targets(16, D, motion, 78)}]
    opt, sc = tr.get_optimizer(5e-4)
    orc.get_optimizer(5e-4)
    emu = O.StudentOracle("resnet18", 5, D, motion, sd, dec_sd)
    emu.get_optimizer(5e-4)
    got, ref = [], []
    for _ in range(3):
        got.append(tr.epoch(batches, optimizer=opt, scaler=sc))
        ref.append(orc.epoch(batches, train=True))
        for b in batches:
            _, _, _, g = emu.forward_loss(b["img"], b["emb"], train=True, need_grad=True, emulate_bf16=True)
            O.adamw_update(emu.params(), g, emu.opt, 5e-4)
    got.append(tr.epoch(held))
    ref.append(orc.epoch(held, train=False))
    rel = [abs(a - b) / abs(b) for a, b in zip(got, ref)]
    e_ref = O.embed(orc.enc, held[0]["img"], "resnet18", True)
    with torch.no_grad():
        e_emu = O.encoder_forward(emu.enc, held[0]["img"], "resnet18", False, None, True).numpy()
    emb_hip = float(per_sample_rel(enc.embed(held[0]["img"]), e_ref).max())
    emb_emu = float(per_sample_rel(e_emu, e_ref).max())

    def weight_err(get):
        num = den = 0.0
        for name in orc.enc_keys:
            r = orc.enc[name].double()
            num += float(((get(name).double() - r) ** 2).sum())
            den += float((r ** 2).sum())
        return (num / den) ** 0.5
    w_hip = weight_err(lambda n: enc.get_parameter(n).detach().cpu())
    w_emu = weight_err(lambda n: emu.enc[n])
    print("trajectory", dict(motion=motion, hip=got, ref=ref, rel=rel, emb=(emb_hip, emb_emu), w=(w_hip, w_emu)))
    assert ref[2] < ref[0]                                       # the oracle itself is learning on these batches
    assert max(rel) <= 1e-2, (got, ref)
    assert emb_hip <= 1.5 * emb_emu + 1e-2, (emb_hip, emb_emu)
    assert w_hip <= 1.5 * w_emu + 1e-2, (w_hip, w_emu)


@pytest.mark.parametrize("arch,motion", [("resnet18", True), ("resnet50", False)])
def test_fused_adamw_repack_equals_separate_kernels(arch, motion):
    """optimizer.step() of the train loop is ONE kernel (AdamW + refresh of the plan's packed bf16 weights,
    vpd_plan_adamw_step); it must leave the parameters, both moments and the NEXT forward exactly as the flat AdamW
    kernel followed by vpd_pack_weights does."""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    D = 32
    sd = O.reference_init_state_dict(arch, 5, D, 21)
    last = ".bn3.weight" if O.arch_expansion(arch) == 4 else ".bn2.weight"
    for k in sd:                   # well-conditioned regime (see above): the BN statistics' fp32 atomics make an untrained
        if k.endswith(last):       # ResNet-50's loss bimodal at the 2 % level, which would hide a stale weight
            sd[k] = sd[k] * 0.1
    dec_sd = O.procedural_state_dict(O.decoder_schema(D), 22) if motion else None
    img, tgt = O.synthetic_crops(6, 5, 64, 23), O.synthetic_targets(6, D, motion, 24)
    out, g0 = [], None
    for fused in (True, False):
        enc = RGBF_EmbeddingModel(arch, D, True, "cuda")
        enc.load_state_dict(sd)
        tr = ModelTrainer(enc, motion)
        if motion:
            tr.fcn_time.load_state_dict(dec_sd)
        opt, _ = tr.get_optimizer(5e-4)
        eng = enc.engine
        enc.train()
        losses = []
        for it in range(3):
            loss = tr._forward_loss(img, tgt, train=True)
            losses.append(loss.item())
            loss.backward()
            if g0 is None:
                g0 = eng.grads.clone()
            eng.grads.copy_(g0)                  # identical gradients in both runs (BN statistics use fp32 atomics)
            assert eng._step_plan is not None
            if not fused:
                eng._step_plan = None
            opt.step()
        torch.cuda.synchronize()
        out.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), losses))
    (p1, m1, v1, l1), (p0, m0, v0, l0) = out
    for name, a, b in (("m", m1, m0), ("v", v1, v0), ("p", p1, p0)):
        bad = (a != b).nonzero().flatten()
        assert bad.numel() == 0, (name, int(bad.numel()), bad[:8].tolist(), float((a - b).abs().max()))
    assert np.allclose(l1, l0, rtol=2e-3), (l1, l0)          # the next forwards ran on the same packed weights
    assert abs(l1[1] - l1[0]) > 0.01 * l1[0]                  # ... and one step moves the loss far more than that


def test_adamw_kernel_injected_grads():
    """Fused AdamW kernel vs torch.optim.AdamW on identical injected gradients (golden from torch)."""
    import ctypes as C
    from vpd_amd._lib import check, lib
    g = np.load(os.path.join(GOLDEN, "adamw_injected.npz"))
    p = torch.from_numpy(g["p0"].copy()).cuda()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for t in range(3):
        gr = torch.from_numpy(g["grads"][t].copy()).cuda()
        check(lib().vpd_adamw_step(C.c_void_p(p.data_ptr()), C.c_void_p(gr.data_ptr()), C.c_void_p(m.data_ptr()),
                                   C.c_void_p(v.data_ptr()), p.numel(), float(g["lr"]), 0.9, 0.999, 1e-8, 0.01,
                                   t + 1, s), "adamw")
        torch.cuda.synchronize()
        assert np.allclose(p.cpu().numpy(), g["p_hist"][t], rtol=0, atol=1e-6)
    assert np.allclose(m.cpu().numpy(), g["m"], rtol=1e-5, atol=1e-8)
    assert np.allclose(v.cpu().numpy(), g["v"], rtol=1e-5, atol=1e-10)


def test_embed_contract_and_errors():
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    enc = RGBF_EmbeddingModel("resnet18", 32, True, "cuda")
    x = O.synthetic_crops(2, 5, 64, 3)
    e1 = enc.embed(x[0])                      # 3-D input gets a batch dim
    assert e1.shape == (1, 32) and e1.dtype == np.float32
    e2 = enc.embed(x.numpy())
    assert np.allclose(e1[0], e2[0], rtol=1e-5, atol=1e-6)
    with pytest.raises(AssertionError):
        enc.embed(x[:, :3])
    enc3 = RGBF_EmbeddingModel("resnet18", 32, False, "cuda")
    with pytest.raises(AssertionError):
        enc3.embed(x)


def test_pretrained_backbone_from_a_local_checkpoint(tmp_path, monkeypatch):
    """pretrained=True (reference models/rgb.py:57-61) with the torchvision-format checkpoint read from disk: backbone tensors as
    they are, the 3-channel stem turned into its channel mean over 5 channels (add_flow_to_model, :19-23), the 1000-way fc
    replaced by a fresh embedding layer (replace_last_layer, :40-43); without a checkpoint the flag fails with instructions."""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    monkeypatch.setenv("VPD_PRETRAINED_WEIGHTS", str(tmp_path))
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "no_hub"))
    with pytest.raises(FileNotFoundError):
        RGBF_EmbeddingModel("resnet18", 32, True, "cuda", pretrained=True)
    ref = O.procedural_state_dict(O.encoder_schema("resnet18", 3, 1000), 41)
    tv = {k[len("resnet."):]: v for k, v in ref.items()}            # torchvision names: conv1.weight, layer1.0.bn1.running_var, fc.*
    assert tv["fc.weight"].shape == (1000, 512) and tv["conv1.weight"].shape == (64, 3, 7, 7)
    torch.save(tv, str(tmp_path / "resnet18-deadbeef.pth"))
    enc = RGBF_EmbeddingModel("resnet18", 32, True, "cuda", pretrained=True)
    sd = enc.state_dict()
    stem = tv["conv1.weight"].mean(dim=1, keepdim=True).expand(-1, 5, -1, -1)
    assert torch.equal(sd["resnet.conv1.weight"].cpu(), stem)
    for k in ("layer1.0.conv1.weight", "layer4.1.bn2.weight", "layer3.0.downsample.1.running_var", "bn1.running_mean"):
        assert torch.equal(sd["resnet." + k].cpu(), tv[k]), k
    assert sd["resnet.fc.weight"].shape == (32, 512) and float(sd["resnet.fc.weight"].abs().max()) <= 1 / np.sqrt(512) + 1e-6
    # the forward uses them: eval embeddings == the oracle's with the same tensors
    x = O.synthetic_crops(3, 5, 64, 8)
    want = O.embed({k: v.cpu() for k, v in sd.items()}, x, "resnet18", True)
    got = enc.embed(x)
    assert (np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)).max() <= 2e-2
    enc3 = RGBF_EmbeddingModel("resnet18", 32, False, "cuda", pretrained=True)      # 3 channels: the stem as it is
    assert torch.equal(enc3.state_dict()["resnet.conv1.weight"].cpu(), tv["conv1.weight"])
    # torchvision's ImageNet-V1 files were saved before BatchNorm had num_batches_tracked: they load like nn.BatchNorm loads them
    legacy = {k: v for k, v in tv.items() if not k.endswith("num_batches_tracked")}
    assert len(legacy) < len(tv)
    torch.save(legacy, str(tmp_path / "resnet18-deadbeef.pth"))
    enc4 = RGBF_EmbeddingModel("resnet18", 32, True, "cuda", pretrained=True)
    sd4 = enc4.state_dict()
    assert torch.equal(sd4["resnet.layer2.0.bn1.running_var"].cpu(), tv["layer2.0.bn1.running_var"])
    assert int(sd4["resnet.bn1.num_batches_tracked"]) == 0
    assert np.array_equal(enc4.embed(x)[:, :4].shape, (3, 4))


def test_ragged_batches_and_graph():
    """Ragged last batch (20000 mod B) and the hipGraph-captured eval forward give the same embeddings."""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    enc = RGBF_EmbeddingModel("resnet18", 32, True, "cuda")
    enc.load_state_dict(O.procedural_state_dict(O.encoder_schema("resnet18", 5, 32), 9))
    x = O.synthetic_crops(11, 5, 64, 4).cuda()
    enc.eval()
    full = enc(x).cpu().numpy()
    part = enc(x[:3].contiguous()).cpu().numpy()
    assert np.allclose(full[:3], part, rtol=1e-5, atol=1e-6)
    out = torch.empty(11, 32, device="cuda")
    pl = enc.engine.capture_eval_graph(x, out)
    out.zero_()
    enc.engine.launch_eval_graph(pl, 11)
    torch.cuda.synchronize()
    assert np.allclose(out.cpu().numpy(), full, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("cfg", [("resnet18", 96, 5, 3), ("resnet18", 160, 3, 2), ("resnet34", 32, 5, 7), ("resnet18", 224, 5, 1),
                                 ("resnet50", 96, 5, 2)],
                         ids=["r18_96px_n3", "r18_160px_rgb_n2", "r34_32px_n7", "r18_224px_n1", "r50_96px_n2"])
def test_other_image_sizes_and_tiny_batches(cfg):
    """Image sizes whose feature maps do not fit the halo tilings (96 -> 24/12/6/3 pixel rows, 160 -> 40/20/10/5,
    224 -> 56/28/14/7, 32 -> 8/4/2/1) take the generic kernels; batches of 1..7 crops leave most tiles ragged.
    Eval embeddings and the train-mode loss against the fp32 oracle, and the backward pass in the well-conditioned
    regime of test_backward_in_a_well_conditioned_regime."""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.trainer import ModelTrainer
    arch, hw, c_in, n = cfg
    sd = O.reference_init_state_dict(arch, c_in, 32, 11)
    last = ".bn3.weight" if O.arch_expansion(arch) == 4 else ".bn2.weight"
    for k in sd:
        if k.endswith(last):
            sd[k] = sd[k] * 0.1
        elif k.endswith("running_var"):
            sd[k] = sd[k] * 0.5 + 0.25          # non-trivial eval-mode statistics
    enc = RGBF_EmbeddingModel(arch, 32, c_in == 5, "cuda")
    enc.load_state_dict(sd)
    tr = ModelTrainer(enc, False)
    orc = O.StudentOracle(arch, c_in, 32, False, sd, None)
    img, tgt = O.synthetic_crops(n, c_in, hw, 5), O.synthetic_targets(n, 32, False, 6)
    e = enc.embed(img.numpy())
    e_ref = O.embed(orc.enc, img, arch, c_in == 5)
    assert per_sample_rel(e, e_ref).max() <= EMB_TOL, per_sample_rel(e, e_ref)
    if n * (hw // 32) ** 2 < 8:
        return                                   # train-mode BN over fewer than 8 values per channel in layer4: eval only
    enc.train()
    loss = tr._forward_loss(img, tgt, train=True)
    l_hip = loss.item()
    loss.backward()
    torch.cuda.synchronize()
    l_ref, _, _, grads_ref = orc.forward_loss(img, tgt, train=True, need_grad=True)
    assert abs(l_hip - l_ref) <= LOSS_TOL * l_ref, (l_hip, l_ref)
    num = den = nh = 0.0
    for name, p in enc.named_parameters():
        r = grads_ref["enc." + name].double().flatten()
        gh = p.grad.detach().cpu().double().flatten()
        num += float((gh * r).sum()); den += float((r * r).sum()); nh += float((gh * gh).sum())
    cos, proj = num / (den * nh) ** 0.5, num / den
    assert cos >= 0.9 and 0.9 <= proj <= 1.1, (cos, proj)


def test_lazy_gradients_of_the_fused_step_match_the_eager_path():
    """models.util.step() hands the conv weight gradients to the optimizer in the kernels' layout (no unpack pass): the
    parameters after the step are bit-identical to loss.backward(); optimizer.step(), and reading engine.grads after a lazy
    backward completes the flat buffer with the same values as the eager backward."""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import step
    from vpd_amd.trainer import ModelTrainer
    g = torch.Generator().manual_seed(5)
    img = torch.randn(6, 5, 64, 64, generator=g).cuda()
    tgt = torch.randn(6, 64, generator=g).cuda()
    out = []
    for lazy in (False, True):
        enc = RGBF_EmbeddingModel("resnet18", 32, True, torch.device("cuda:0"))
        enc.reset_parameters(seed=1)
        tr = ModelTrainer(enc, motion=True)
        for q in tr.fcn_time.parameters():
            with torch.no_grad():
                q.copy_(torch.randn(q.shape, generator=torch.Generator().manual_seed(q.numel())).to(q.device) * 0.05)
        opt, sc = tr.get_optimizer(5e-4)
        enc.train()
        grads = None
        for it in range(3):
            loss = tr._forward_loss(img, tgt, train=True)
            if lazy:
                if it == 1:      # look at the gradients between a lazy backward and the step: the property completes them
                    loss.backward_for_step()
                    assert enc.engine._step_plan is not None
                    grads = enc.engine.grads.clone()
                    opt.step()
                else:
                    step(opt, sc, loss)
            else:
                loss.backward()
                if it == 1:
                    grads = enc.engine.grads.clone()
                opt.step()
        torch.cuda.synchronize()
        out.append((enc.engine.params.cpu().numpy(), grads.cpu().numpy(), enc.engine.adam_m.cpu().numpy()))
    (p0, g0, m0), (p1, g1, m1) = out
    # every reduction of the BasicBlock step runs in a fixed order (fp64 statistic rows, slab sums; the 1x1 down-sampling
    # weight gradients take the halo kernel, not the atomics kernel): two runs agree to the last bit
    assert np.array_equal(g1, g0), rel_l2(g1, g0)
    assert np.array_equal(m1, m0) and np.array_equal(p1, p0), (rel_l2(m1, m0), rel_l2(p1, p0))


def test_step_with_a_torch_optimizer_reads_complete_gradients():
    """models.util.step() accepts ANY optimizer (reference models/util.py:50-58).  Only FusedAdamW may get the lazy
    backward; torch.optim.AdamW over the same parameters must see complete p.grad views:
    * ONE step with it equals one step with FusedAdamW to 1e-6 (same gradients, same AdamW arithmetic in another kernel;
      later steps cannot be compared: a 6e-8 difference in the weights flips bf16 roundings of an untrained network);
    * three step() calls equal three explicit `loss.backward(); opt.step(); opt.zero_grad()` rounds bit for bit -- step()
      hands a torch optimizer the eager gradients, and its zero_grad(set_to_none=True) does not lose the gradient views."""
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    from vpd_amd.models.util import step
    from vpd_amd.trainer import ModelTrainer
    g = torch.Generator().manual_seed(11)
    img = torch.randn(6, 5, 64, 64, generator=g).cuda()
    tgt = torch.randn(6, 64, generator=g).cuda()
    out = {}
    for kind in ("fused", "torch_step", "torch_explicit"):
        enc = RGBF_EmbeddingModel("resnet18", 32, True, torch.device("cuda:0"))
        enc.reset_parameters(seed=3)
        tr = ModelTrainer(enc, motion=True)
        for q in tr.fcn_time.parameters():
            with torch.no_grad():
                q.copy_(torch.randn(q.shape, generator=torch.Generator().manual_seed(q.numel())).to(q.device) * 0.05)
        if kind == "fused":
            opt, sc = tr.get_optimizer(5e-4)
        else:
            opt, sc = torch.optim.AdamW(list(enc.parameters()) + list(tr.fcn_time.parameters()), lr=5e-4), None
            assert not getattr(opt, "consumes_lazy_grads", False)
        enc.train()
        hist = []
        for it in range(3):
            loss = tr._forward_loss(img, tgt, train=True)
            if kind == "torch_explicit":
                loss.backward()
                assert not lib_pending(enc.engine)
                opt.step()
                opt.zero_grad()
            else:
                step(opt, sc, loss)
            torch.cuda.synchronize()
            hist.append(enc.engine.params.detach().cpu().numpy().copy())
        out[kind] = hist
    assert np.isfinite(out["torch_step"][2]).all()
    # a stale (never unpacked) conv gradient would leave the conv weights where weight decay alone puts them: ~5e-4 away
    assert np.abs(out["fused"][0] - out["torch_step"][0]).max() < 1e-6, np.abs(out["fused"][0] - out["torch_step"][0]).max()
    for it in range(3):
        assert np.array_equal(out["torch_step"][it], out["torch_explicit"][it]), it


def lib_pending(engine):
    from vpd_amd._lib import lib
    pl = engine._step_plan
    return bool(pl is not None and lib().vpd_plan_grads_pending(pl.handle))


_R50_STEP_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, {repo!r})
from oracle import vpd_oracle as O
from vpd_amd.models.rgb import RGBF_EmbeddingModel
from vpd_amd.trainer import ModelTrainer
sd = O.reference_init_state_dict({arch!r}, 5, 32, 3)
for k in sd:
    if k.endswith(".bn3.weight"):
        sd[k] = sd[k] * 0.1                      # the well-conditioned regime of the wc_grads goldens
enc = RGBF_EmbeddingModel({arch!r}, 32, True, "cuda")
enc.load_state_dict(sd)
tr = ModelTrainer(enc, False)
g = torch.Generator(device="cuda").manual_seed(4)
img = torch.randn((64, 5, 128, 128), generator=g, device="cuda")
tgt = torch.randn((64, 32), generator=g, device="cuda")
enc.train()
loss = tr._forward_loss(img, tgt, train=True)
loss.backward()
torch.cuda.synchronize()
assert enc.engine.sync_errors() == 0
np.save({out!r}, enc.engine.grads.cpu().numpy())
np.save({out!r} + ".bn.npy", enc.engine.bn_running.cpu().numpy())
np.savez({out!r} + ".t.npz", **{{n: q.grad.detach().cpu().numpy() for n, q in enc.named_parameters()}})
print("LOSS", loss.item())
"""


@pytest.mark.parametrize("arch", ["resnet50", "wide_resnet50_2"])
def test_bottleneck_tail_recomputed_instead_of_stored(tmp_path, arch):
    """Default path from 64 crops per step up (layer1 of a ResNet-50; layer2 from 256): an identity Bottleneck's closing 1x1
    convolution and its BatchNorm run as conv1x1_bn_stream_kernel -- z3 is computed twice (statistics pass, apply pass) and never
    stored, in the backward twice more (sums, apply).  VPD_BNECK_RECOMPUTE=0 is conv + BatchNorm launches with z3 in memory, which
    the goldens pin.  Forward: same bf16 rounding points, same sums -- the loss and the running statistics must be EQUAL.  Backward:
    bn_bwd_apply_fused_kernel's arithmetic (sum g z in fp64 -> A g + B z + D) instead of bn_bwd_fused_kernel's: same gradient to
    rounding -- whole gradient: cosine > 0.999, norm within 1 %; EVERY parameter tensor: rel-L2 <= 2e-2 (measured <= 0.8e-2; a
    coefficient of one recomputed BatchNorm 2 % off shows as >= 2e-2 in that block's and every earlier tensor) -- in the
    well-conditioned regime of the wc_grads goldens.  resnet50: layer1's three blocks at 64 crops (K = 64 kernels, the down-sampling
    block's two-convolution launches); wide_resnet50_2: K = 128 kernels (layer1's closing convs are 128 -> 256)."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for flag in ("0", "1"):
        out = str(tmp_path / ("g%s.npy" % flag))
        env = dict(os.environ, VPD_BNECK_RECOMPUTE=flag)
        r = subprocess.run([sys.executable, "-c", _R50_STEP_SCRIPT.format(repo=repo, out=out, arch=arch)], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        outs.append((np.load(out), np.load(out + ".bn.npy"), float(r.stdout.split("LOSS")[1].split()[0]), dict(np.load(out + ".t.npz"))))
    (g0, b0, l0, t0), (g1, b1, l1, t1) = outs
    assert l0 == l1
    assert np.array_equal(b0, b1)
    worst = max((rel_l2(t1[n], t0[n]), n) for n in t0 if np.linalg.norm(t0[n]) > 0)
    assert worst[0] <= 2e-2, worst
    assert np.isfinite(g1).all() and np.abs(g1).max() > 0
    cos = float(np.dot(g0.astype(np.float64), g1.astype(np.float64)) / (np.linalg.norm(g0) * np.linalg.norm(g1)))
    assert cos > 0.999 and abs(np.linalg.norm(g1) / np.linalg.norm(g0) - 1) < 1e-2, (cos, rel_l2(g1, g0))
