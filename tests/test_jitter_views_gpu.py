"""Jittered inference views built on the device (apply --jitter; vpd_augment_views / vpd_plan_stage_views_jitter) against the CPU
oracle's ColorJitter ops applied to the NORMALISED fp32 image, the way the reference's FrameDataset composes them
(vpd_dataset/single_frame.py:373-400; the host path is pinned the same way in test_host_cpu.test_frame_dataset_jitter_views).

Tolerance of the jittered RGB: fp32 elementwise arithmetic in torchvision's operation order (FMA contraction is off in
augment.hip); what differs is the summation order of the contrast op's grey mean -> the 2e-5 absolute of test_augment_gpu.py.
(The oracle against itself with the mean summed in 8 strided fp32 partials differs by at most 1.7e-6 on these frames.)"""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import augment_oracle as AO
from oracle import vpd_oracle as O

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ATOL = 2e-5
MEAN_STD = ((0.3411329922282787, 0.46349889258964044, 0.5162481674015696),
            (0.16302619019820488, 0.17092395707914718, 0.19266662199338647))


def _crops(n, h, w, seed):
    """The seeded frames of test_augment_gpu._crops: grey, white and black blocks give ties and clamped pixels."""
    rs = np.random.RandomState(seed)
    rgb = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    rgb[:, : h // 4, : w // 4, :] = rgb[:, : h // 4, : w // 4, :1]           # grey block
    rgb[:, h // 2:, : w // 8, :] = 255                                          # white block
    rgb[:, : h // 8, w // 2:, :] = 0                                            # black block
    flow = np.clip(np.round(124 + 12 * rs.randn(n, h, w, 2)), 0, 255).astype(np.uint8)
    return rgb, flow


def _rows(n, jitter, flip, seed):
    """Parameter rows that cover all 24 orders (hue first and contrast first among them) and a partial order."""
    from vpd_amd import augment as A
    p = A.sample_view_params(n, jitter, flip, generator=torch.Generator().manual_seed(seed))
    perms = list(itertools.permutations(range(4)))
    assert len(p) >= 25, "not enough rows for the 24 orders and the partial one"
    for i, o in enumerate(perms):
        p["order"][i] = o
    p["order"][24] = (1, -1, -1, 3)
    firsts = {int(o[0]) for o in p["order"]}
    assert 3 in firsts and 1 in firsts
    return p


def _jit(img, row):
    f = tuple(float(v) for v in row["factor"])
    for op in (int(v) for v in row["order"]):
        if op >= 0:
            img = AO._OPS[op](img, f[op])
    return img


def _plain(rgb, flow):
    """The fp32 expressions of test_no_augmentation_is_bit_exact_loader: (u8 / 255 - mean) / std; u8 / 255 - 0.5 in double."""
    m = torch.tensor(MEAN_STD[0], dtype=torch.float32).view(3, 1, 1)
    s = torch.tensor(MEAN_STD[1], dtype=torch.float32).view(3, 1, 1)
    base = (torch.as_tensor(rgb).float().permute(2, 0, 1) / 255. - m) / s
    fl = None
    if flow is not None:
        fl = torch.as_tensor((torch.as_tensor(flow).double() / 255) - 0.5).float().permute(2, 0, 1)
    return base, fl


def _ref_views(rgb, flow, params, jitter, flip):
    """[F, K, C, H, W]: FrameDataset's item per frame, from the oracle's ops."""
    rows = jitter * (2 if flip else 1)
    out = []
    for f in range(rgb.shape[0]):
        base, fl = _plain(rgb[f], None if flow is None else flow[f])
        cat = (lambda x, y: x) if fl is None else (lambda x, y: torch.cat((x, y)))
        views = [cat(base, fl)]
        pr = params[f * rows:(f + 1) * rows]
        views += [cat(_jit(base, pr[j]), fl) for j in range(jitter)]
        if flip:
            fb = torch.flip(base, (2,))
            views += [cat(_jit(fb, pr[jitter + j]), fl) for j in range(jitter)]      # jittered flips: UNFLIPPED flow
            ff = None
            if fl is not None:
                ff = torch.flip(fl, (2,))
                ff[0, :, :] *= -1
            views.append(cat(fb, ff))
        out.append(torch.stack(views))
    return torch.stack(out)


CASES = [(7, 128, True, True), (13, 128, True, False), (7, 64, False, True), (13, 64, False, False)]
IDS = ["128_flow_flip", "128_flow_noflip", "64_rgb_flip", "64_rgb_noflip"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_views_match_the_oracle_per_element(case):
    from vpd_amd import augment as A
    n, hw, use_flow, flip = case
    J = 2
    K = (1 + J) * (2 if flip else 1)
    rgb, flow = _crops(n, hw, hw, seed=n * 7 + hw)
    if not use_flow:
        flow = None
    params = _rows(n, J, flip, seed=hw + n)
    aug = A.CropAugmenter("cuda:0", MEAN_STD, hw, use_flow)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    got = aug.views(dev(rgb), dev(flow), J, flip, params).cpu()
    C = 5 if use_flow else 3
    assert got.shape == (n * K, C, hw, hw)
    got = got.view(n, K, C, hw, hw)
    exp = _ref_views(rgb, flow, params, J, flip)
    assert exp.shape == got.shape
    # plain views (the frame; with flip also the last view, its mirror): bit for bit
    assert torch.equal(got[:, 0], exp[:, 0])
    if flip:
        assert torch.equal(got[:, K - 1], exp[:, K - 1])
    # flow of every view: bit for bit (jittered flips carry the unflipped flow, only the last view the mirrored one)
    if use_flow:
        assert torch.equal(got[:, :, 3:], exp[:, :, 3:])
        if flip:
            assert torch.equal(got[:, J + 1, 3:], got[:, 0, 3:]) and not torch.equal(got[:, K - 1, 3:], got[:, 0, 3:])
            assert torch.equal(got[:, K - 1, 3], -torch.flip(got[:, 0, 3], (2,)))
    jit = slice(1, K - 1) if flip else slice(1, K)
    g, e = got[:, jit, :3], exp[:, jit, :3]
    assert float(g.min()) >= 0.0 and float(g.max()) <= 1.0
    err = (g - e).abs()
    worst = float(err.max())
    print("jittered RGB max abs err %.3g (%s)" % (worst, IDS[CASES.index(case)]))
    assert worst <= ATOL, "max abs err %.3g at %s" % (worst, np.unravel_index(int(err.argmax()), err.shape))
    # the jitter did something in every jittered view
    src = got[:, :1, :3] if not flip else torch.cat([got[:, :1, :3].expand(-1, J, -1, -1, -1),
                                                     got[:, K - 1:, :3].expand(-1, J, -1, -1, -1)], dim=1)
    assert float((g - src).abs().amax(dim=(2, 3, 4)).min()) > 1e-3


@pytest.mark.parametrize("use_flow", [True, False], ids=["flow", "rgb"])
def test_jittered_flip_is_the_mirror_of_the_jittered_frame(use_flow):
    """Every op is pointwise but the mean: with the same decisions, jitter(flip(x)) is flip(jitter(x)) within the bound."""
    from vpd_amd import augment as A
    n, hw, J = 7, (128 if use_flow else 64), 2
    rgb, flow = _crops(n, hw, hw, seed=5)
    if not use_flow:
        flow = None
    params = _rows(n, J, True, seed=17).reshape(n, 2, J)
    params[:, 1] = params[:, 0]                               # the flipped frame's rows = the frame's own
    first = params[:, 0].reshape(-1)["order"][:, 0]
    assert 1 in first and 3 in first                          # contrast first and hue first are still among them
    params = params.reshape(-1)
    aug = A.CropAugmenter("cuda:0", MEAN_STD, hw, use_flow)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    got = aug.views(dev(rgb), dev(flow), J, True, params).cpu().view(n, 6, -1, hw, hw)
    for j in range(J):
        err = float((got[:, 1 + J + j, :3] - torch.flip(got[:, 1 + j, :3], (3,))).abs().max())
        assert err <= ATOL, err


def test_two_calls_are_bit_identical():
    """Fixed-order partial sums of the grey mean, no atomics: the same inputs give the same bits."""
    from vpd_amd import augment as A
    n, hw, J = 7, 128, 2
    rgb, flow = _crops(n, hw, hw, seed=9)
    params = _rows(n, J, True, seed=3)
    aug = A.CropAugmenter("cuda:0", MEAN_STD, hw, True)
    r, f = torch.from_numpy(rgb).cuda(), torch.from_numpy(flow).cuda()
    a = aug.views(r, f, J, True, params).clone()
    junk = torch.randn(1 << 20, device="cuda")               # other work in between
    b = aug.views(r, f, J, True, params)
    assert torch.equal(a, b) and bool(torch.isfinite(junk).all())
    # and another set of decisions gives other values
    c = aug.views(r, f, J, True, A.sample_view_params(n, J, True, generator=torch.Generator().manual_seed(99)))
    assert not torch.equal(a, c)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("c_in", [5, 3])
def test_staged_views_equal_the_fp32_batch_path(c_in, dtype):
    """vpd_plan_stage_views_jitter + forward_eval(x = NULL) == vpd_augment_views -> fp32 batch -> forward_eval(x): the same
    embeddings, bit for bit in eval mode (both round the same fp32 values to the element type once)."""
    from vpd_amd import augment as A
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    n, hw, J = 7, 128, 2
    rgb, flow = _crops(n, hw, hw, seed=3)
    enc = RGBF_EmbeddingModel("resnet18", 32, c_in == 5, torch.device("cuda:0"), dtype=dtype)
    enc.reset_parameters(seed=0)
    enc.eval()
    eng = enc.engine
    aug = A.CropAugmenter("cuda:0", MEAN_STD, hw, c_in == 5)
    r = torch.from_numpy(rgb).cuda()
    f = torch.from_numpy(flow).cuda() if c_in == 5 else None
    for flip in (True, False):
        params = A.sample_view_params(n, J, flip, generator=torch.Generator().manual_seed(9))
        img = aug.views(r, f, J, flip, params, dtype=dtype)
        e1 = eng.forward_eval(img).clone()
        staged = aug.stage_views(eng, r, f, flip, jitter=J, params=params)
        assert staged == (n * (1 + J) * (2 if flip else 1), hw)
        e2 = eng.forward_eval(None, staged=staged).clone()
        assert bool(torch.isfinite(e1).all()) and float(e1.abs().max()) > 0
        assert torch.equal(e1, e2), float((e1 - e2).abs().max())
        # the plain views of the jittered staging are those of today's staging call
        k0 = 2 if flip else 1
        e0 = eng.forward_eval(None, staged=aug.stage_views(eng, r, f, flip)).view(n, k0, -1)
        e2 = e2.view(n, staged[0] // n, -1)
        assert torch.equal(e2[:, 0], e0[:, 0]) and (not flip or torch.equal(e2[:, -1], e0[:, -1]))


def test_embed_dataset_builds_the_jittered_views_on_the_device():
    from vpd_amd import augment as A
    from vpd_amd.apply import embed_dataset
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    g = np.load(os.path.join(REPO, "tests", "golden", "format_case.npz"))
    arch, D, c_in, hw, J = "resnet18", 32, 5, 64, 2
    enc = RGBF_EmbeddingModel(arch, D, True, "cuda")
    enc.load_state_dict(O.procedural_state_dict(O.encoder_schema(arch, c_in, D), 5))
    aug = A.CropAugmenter("cuda", MEAN_STD, hw, True)
    tasks = g["tasks"]
    rgb, flow = O.synthetic_crops_u8(len(tasks), c_in, hw, 21)
    cuts = list(range(0, len(tasks), 5))                      # 5 + 5 + 2: a tail batch
    mk = lambda: [{"video": torch.tensor(tasks[s:s + 5, 0]), "frame": torch.tensor(tasks[s:s + 5, 1]),
                   "rgb_u8": rgb[s:s + 5], "flow_u8": flow[s:s + 5]} for s in cuts]
    by_frame = lambda embs: {(v, t[0]): t[1] for v, lst in enumerate(embs) for t in lst}
    plain = by_frame(embed_dataset(enc, mk(), 3, augmenter=aug, flip=True))
    seed = lambda: torch.Generator().manual_seed(123)
    graph = by_frame(embed_dataset(enc, mk(), 3, augmenter=aug, flip=True, jitter=J, generator=seed()))
    eager = by_frame(embed_dataset(enc, mk(), 3, augmenter=aug, flip=True, jitter=J, generator=seed(), use_graph=False))
    assert set(graph) == set(plain) == set(eager) and len(graph) == len(tasks)
    for key, e in graph.items():
        assert e.shape == (6, D) and e.dtype == np.float32
        assert np.array_equal(e[0], plain[key][0]) and np.array_equal(e[5], plain[key][1])
        assert np.array_equal(e, eager[key])                  # graph replay == direct launches
        assert not np.array_equal(e[1], e[0]) and not np.array_equal(e[1], e[2])
    # the fp32 host route fed CPU-built views with the same decisions (the generator's stream, batch by batch)
    gen, batches = seed(), []
    for s in cuts:
        nb = len(tasks[s:s + 5])
        p = A.sample_view_params(nb, J, True, generator=gen)
        views = _ref_views(rgb[s:s + 5].numpy(), flow[s:s + 5].numpy(), p, J, True)
        batches.append({"video": torch.tensor(tasks[s:s + 5, 0]), "frame": torch.tensor(tasks[s:s + 5, 1]), "img": views})
    host = by_frame(embed_dataset(enc, batches, 3))
    worst = 0.0
    for key, e in graph.items():
        rel = float(np.linalg.norm(e - host[key]) / np.linalg.norm(host[key]))
        worst = max(worst, rel)
    print("u8 jitter route vs fp32 host route: worst per-frame rel-L2 %.3g" % worst)
    assert worst <= 2e-2, worst                               # the project's sanity bound (test_apply_gpu), not a precision claim


def _write_model_and_crops(tmp_path, use_flow, hw, n_frames):
    from PIL import Image
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    D = 16
    model = tmp_path / "model"
    model.mkdir()
    json.dump({"emb_dim": D, "encoder_arch": "resnet18", "img_dim": hw, "use_flow": use_flow, "motion": False,
               "rgb_mean_std": [list(MEAN_STD[0]), list(MEAN_STD[1])]}, open(model / "config.json", "w"))
    enc = RGBF_EmbeddingModel("resnet18", D, use_flow, "cuda")
    enc.reset_parameters(seed=4)
    torch.save(enc.state_dict(), model / "best_epoch.encoder.pt")
    crops = tmp_path / "crops"
    rs = np.random.RandomState(0)
    for vid, nf in (("va", n_frames), ("vb", 3)):
        (crops / vid).mkdir(parents=True)
        for f in range(nf):
            Image.fromarray(rs.randint(0, 256, (hw, hw, 3)).astype(np.uint8)).save(crops / vid / ("%d.png" % f))
            if use_flow:
                Image.fromarray(rs.randint(96, 160, (hw, hw, 3)).astype(np.uint8)).save(crops / vid / ("%d.flow.png" % f))
    return model, crops, D


def test_cli_jitter_stages_on_the_device(tmp_path, monkeypatch):
    """apply_vpd_model.py ... --jitter 1 writes (4, D) entries and builds every view on the device; with --host_fp32 the same
    command takes the reference's host route."""
    sys.path.insert(0, REPO)
    import apply_vpd_model
    from vpd_amd.engine import StudentEngine
    from vpd_amd.io import load_pickle
    model, crops, D = _write_model_and_crops(tmp_path, True, 64, 5)
    monkeypatch.setitem(apply_vpd_model.dataset_paths.CROPS, "fs", str(crops))
    monkeypatch.setattr(os, "cpu_count", lambda: 2)           # (one DataLoader worker for eight frames)
    calls = {"jitter": 0, "plain": 0}
    orig_j, orig_p = StudentEngine.stage_views_jitter, StudentEngine.stage_views

    def count_j(self, *a, **k):
        calls["jitter"] += 1
        return orig_j(self, *a, **k)

    def count_p(self, *a, **k):
        calls["plain"] += 1
        return orig_p(self, *a, **k)
    monkeypatch.setattr(StudentEngine, "stage_views_jitter", count_j)
    monkeypatch.setattr(StudentEngine, "stage_views", count_p)
    for extra, tag in (([], "dev"), (["--host_fp32"], "host")):
        calls.update(jitter=0, plain=0)
        monkeypatch.setattr(sys, "argv", ["apply_vpd_model.py", str(model), "-d", "fs", "-o", str(tmp_path / tag),
                                          "--jitter", "1", "--flow_img", "flow"] + extra)
        apply_vpd_model.main(**vars(apply_vpd_model.get_args()))
        for vid, nf in (("va", 5), ("vb", 3)):
            embs = load_pickle(str(tmp_path / tag / ("%s.emb.pkl" % vid)))
            assert [t[0] for t in embs] == list(range(nf))
            assert all(t[1].shape == (4, D) and t[1].dtype == np.float32 and t[2] == {} for t in embs)
        if tag == "dev":
            assert calls["jitter"] >= 1 and calls["plain"] == 0, calls
        else:
            assert calls == {"jitter": 0, "plain": 0}, calls
    # both routes embed the same plain views (rows 0 and 3): bit for bit, as test_u8_apply_path pins for k = 2
    for vid in ("va", "vb"):
        a, b = load_pickle(str(tmp_path / "dev" / ("%s.emb.pkl" % vid))), load_pickle(str(tmp_path / "host" / ("%s.emb.pkl" % vid)))
        for (fa, ea, _), (fb, eb, _) in zip(a, b):
            assert fa == fb and np.array_equal(ea[0], eb[0]) and np.array_equal(ea[3], eb[3])


def test_rejected_geometry_launches_nothing():
    """A frame size other than the plan's, or a width that is no multiple of 4, is an error message, not a launch."""
    import ctypes as C
    from vpd_amd import augment as A
    from vpd_amd._lib import VpdHipError, check, lib
    from vpd_amd.models.rgb import RGBF_EmbeddingModel
    enc = RGBF_EmbeddingModel("resnet18", 32, True, "cuda")
    eng = enc.engine
    pl = eng.plan(64, 64, 24, False, False)
    ms = (C.c_float * 6)(*[0.5] * 6)
    p = lambda t: C.c_void_p(t.data_ptr())
    rgb = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device="cuda")
    flow = torch.zeros((2, 64, 64, 2), dtype=torch.uint8, device="cuda")
    rows = A.sample_view_params(2, 2, True)
    pdev = torch.from_numpy(rows.view(np.uint8).reshape(len(rows), 64)).cuda()
    scratch = torch.zeros(8 * len(rows), dtype=torch.float32, device="cuda")
    sentinel = torch.full((2 * 6, 5, 64, 64), -7.0, device="cuda")
    call = lambda h, w: lib().vpd_plan_stage_views_jitter(pl.handle, p(rgb), p(flow), p(pdev), 2, 2, 1, h, w, ms, p(scratch),
                                                         p(pl.workspace), None)
    check(call(64, 64), "stage")                              # the good call goes through
    with pytest.raises(VpdHipError, match="plan's size"):
        check(call(32, 32), "stage")
    with pytest.raises(VpdHipError, match="plan's size"):
        check(call(64, 32), "stage")
    with pytest.raises(VpdHipError, match="multiple of 4"):
        check(call(62, 62), "stage")
    with pytest.raises(VpdHipError, match="65535"):
        check(lib().vpd_plan_stage_views_jitter(pl.handle, p(rgb), p(flow), p(pdev), 10923, 2, 1, 64, 64, ms, p(scratch),
                                                p(pl.workspace), None), "stage")
    with pytest.raises(VpdHipError, match="max_batch"):       # more views than the plan holds: refused for the plan, not the grid
        check(lib().vpd_plan_stage_views_jitter(pl.handle, p(rgb), p(flow), p(pdev), 5, 2, 1, 64, 64, ms, p(scratch),
                                                p(pl.workspace), None), "stage")
    with pytest.raises(VpdHipError, match="flow_u8"):
        check(lib().vpd_plan_stage_views_jitter(pl.handle, p(rgb), None, p(pdev), 2, 2, 1, 64, 64, ms, p(scratch),
                                                p(pl.workspace), None), "stage")
    # the fp32 entry point: a width that is no multiple of 4 writes nothing
    rc = lib().vpd_augment_views(p(rgb), p(flow), p(pdev), 2, 2, 1, 64, 62, ms, p(sentinel), p(scratch), None)
    assert rc != 0 and b"multiple of 4" in lib().vpd_last_error()
    torch.cuda.synchronize()
    assert bool((sentinel == -7.0).all())
    # the Python layer refuses missing decisions
    aug = A.CropAugmenter("cuda", MEAN_STD, 64, True)
    with pytest.raises(ValueError):
        aug.views(rgb, flow, 2, True, None)
