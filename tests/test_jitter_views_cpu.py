"""Host side of the device-built jittered inference views (apply --jitter): the sampled ColorJitter decisions, the C-ABI
table rows of the two new entry points, and the CLI's routing of --jitter to the u8 path.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_view_params_layout_and_ranges():
    from vpd_amd.augment import AUG_DTYPE, JITTER_KWARGS, sample_view_params, view_count
    for n, j, flip in ((7, 2, True), (5, 3, False), (1, 1, True)):
        p = sample_view_params(n, j, flip, generator=torch.Generator().manual_seed(n))
        assert p.dtype == AUG_DTYPE and p.shape == (n * j * (2 if flip else 1),)       # one row per JITTERED view
        assert view_count(j, flip) == (1 + j) * (2 if flip else 1)
        assert (np.sort(p["order"], axis=1) == np.arange(4)).all()                    # every order is a permutation
        f = p["factor"].astype(np.float64)
        eps = 1e-6                                                                     # (float32 rounding of the range ends)
        for op, key in enumerate(("brightness", "contrast", "saturation")):
            assert (f[:, op] >= 1 - JITTER_KWARGS[key] - eps).all() and (f[:, op] <= 1 + JITTER_KWARGS[key] + eps).all()
        assert (np.abs(f[:, 3]) <= JITTER_KWARGS["hue"] + eps).all()
        # the fields the device does not read stay at their identity values
        assert (p["flip"] == 0).all() and (p["noise"] == 0).all() and (p["crop"] == 0).all() and (p["seed"] == 0).all()
    # nothing to jitter: no rows
    assert sample_view_params(9, 0, True).shape == (0,) and view_count(0, True) == 2 and view_count(None, False) == 1


def test_sample_view_params_statistics_reproducibility_and_freshness():
    from vpd_amd.augment import JITTER_KWARGS, sample_view_params
    g = torch.Generator().manual_seed(11)
    a = sample_view_params(2000, 2, True, generator=g)
    b = sample_view_params(2000, 2, True, generator=g)                               # the next batch: fresh decisions
    c = sample_view_params(2000, 2, True, generator=torch.Generator().manual_seed(11))
    assert a.tobytes() == c.tobytes() and a.tobytes() != b.tobytes()
    # uniform over the 24 orders and over the factor ranges (8000 rows: 333 +- 18 per order)
    codes = (a["order"] * np.array([64, 16, 4, 1])).sum(axis=1)
    counts = np.unique(codes, return_counts=True)[1]
    assert len(counts) == 24 and counts.min() > 250 and counts.max() < 420
    f = a["factor"].astype(np.float64)
    assert abs(f[:, 0].mean() - 1.0) < 0.01 and abs(f[:, 0].std() - 0.4 / np.sqrt(12)) < 0.005
    assert abs(f[:, 3].mean()) < 0.003 and f[:, 3].min() < -0.9 * JITTER_KWARGS["hue"] and f[:, 3].max() > 0.9 * JITTER_KWARGS["hue"]
    # the global RNG when no generator is given
    torch.manual_seed(3)
    d = sample_view_params(4, 1, False)
    torch.manual_seed(3)
    assert d.tobytes() == sample_view_params(4, 1, False).tobytes()


_CTYPE = {"int": C.c_int, "float": C.c_float}


def _header_signature(name):
    src = open(os.path.join(REPO, "include", "vpd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ret, args = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src).groups()
    out = []
    for a in args.split(","):
        a = a.strip()
        if a.startswith("const float*") and a.endswith("mean_std6"):
            out.append(C.POINTER(C.c_float))                 # a HOST array, passed as a ctypes float array
        elif "*" in a:
            out.append(C.c_void_p)
        else:
            out.append(_CTYPE[a.split()[-2]])
    return _CTYPE[ret], out


def test_new_entry_points_are_bound_with_the_headers_signature():
    from vpd_amd import _lib
    for name in ("vpd_augment_views", "vpd_plan_stage_views_jitter"):
        assert name in _lib.SIGNATURES
        res, args = _header_signature(name)
        assert _lib.SIGNATURES[name][0] is res
        assert list(_lib.SIGNATURES[name][1]) == args, name
    # the parser reads a neighbour's row the same way (so a mismatch above is the table's, not the parser's)
    res, args = _header_signature("vpd_plan_stage_views")
    assert list(_lib.SIGNATURES["vpd_plan_stage_views"][1]) == args
    for dtype in ("bf16", "fp16"):
        h = _lib.lib(dtype)
        assert h.vpd_augment_views is not None and h.vpd_plan_stage_views_jitter is not None


def test_entry_points_reject_bad_arguments_on_the_host():
    """Rejected before anything is launched: no GPU is needed to see the error."""
    from vpd_amd import _lib
    h = _lib.lib()
    ms = (C.c_float * 6)(*[0.5] * 6)
    p = C.c_void_p(64)                                       # never dereferenced
    assert h.vpd_augment_views(p, p, p, 2, 2, 1, 64, 62, ms, p, p, None) != 0 and b"multiple of 4" in h.vpd_last_error()
    assert h.vpd_augment_views(None, p, p, 2, 2, 1, 64, 64, ms, p, p, None) != 0 and b"null" in h.vpd_last_error()
    assert h.vpd_augment_views(p, p, None, 2, 2, 1, 64, 64, ms, p, p, None) != 0 and b"params" in h.vpd_last_error()
    assert h.vpd_augment_views(p, p, p, 2, -1, 1, 64, 64, ms, p, p, None) != 0
    assert h.vpd_augment_views(p, p, p, 10923, 2, 1, 64, 64, ms, p, p, None) != 0 and b"65535" in h.vpd_last_error()
    assert h.vpd_plan_stage_views_jitter(None, p, p, p, 2, 2, 1, 64, 64, ms, p, p, None) != 0


def test_apply_batch_size_is_unchanged():
    from vpd_amd.apply import BATCH_SIZE, apply_batch_size
    assert BATCH_SIZE == 500
    assert apply_batch_size(None, False) == 500 and apply_batch_size(2, False) == 166 and apply_batch_size(2, True) == 332
    assert apply_batch_size(1, False) == 250 and apply_batch_size(0, False) == 500


def test_cli_routes_jitter_to_the_u8_path(monkeypatch):
    sys.path.insert(0, REPO)
    import apply_vpd_model
    monkeypatch.setattr(sys, "argv", ["x", "model", "-d", "fs", "--jitter", "2"])
    a = apply_vpd_model.get_args()
    assert a.jitter == 2 and not a.host_fp32
    assert apply_vpd_model.input_route(a.host_fp32, a.jitter) == (True, 2)           # raw_u8=True, jitter on the device
    monkeypatch.setattr(sys, "argv", ["x", "model", "-d", "fs", "--jitter", "2", "--host_fp32"])
    a = apply_vpd_model.get_args()
    assert apply_vpd_model.input_route(a.host_fp32, a.jitter) == (False, 0)          # the host builds the views, jitter too
    monkeypatch.setattr(sys, "argv", ["x", "model", "-d", "fs"])
    a = apply_vpd_model.get_args()
    assert apply_vpd_model.input_route(a.host_fp32, a.jitter) == (True, 0)


def test_cli_builds_the_raw_dataset_without_jitter_and_hands_the_count_on(tmp_path, monkeypatch):
    """main() up to the model: with --jitter 2 the FrameDataset is raw (augment_jitter=0) and embed_dataset gets jitter=2;
    with --host_fp32 the dataset carries the jittered views and embed_dataset gets jitter=0."""
    import json
    sys.path.insert(0, REPO)
    import apply_vpd_model
    (tmp_path / "crops" / "vid").mkdir(parents=True)
    (tmp_path / "model").mkdir()
    json.dump({"emb_dim": 8, "encoder_arch": "resnet18", "img_dim": 64, "use_flow": False, "motion": False,
               "rgb_mean_std": [[0.3, 0.4, 0.5], [0.2, 0.2, 0.2]]}, open(tmp_path / "model" / "config.json", "w"))
    monkeypatch.setitem(apply_vpd_model.dataset_paths.CROPS, "fs", str(tmp_path / "crops"))
    seen = {}

    class Model:
        def __init__(self, *a, **k):
            pass

        def load_state_dict(self, sd):
            pass

        def to(self, device):
            return self

    def fake_embed(encoder, loader, n_videos, **kw):
        seen.update(kw, raw_u8=loader.dataset.raw_u8, ds_jitter=loader.dataset.jitter_count)

    monkeypatch.setattr(apply_vpd_model, "RGBF_EmbeddingModel", Model)
    monkeypatch.setattr(apply_vpd_model.torch, "load", lambda *a, **k: {})
    monkeypatch.setattr(apply_vpd_model, "embed_dataset", fake_embed)
    monkeypatch.setattr(os, "cpu_count", lambda: 2)
    import vpd_amd.augment
    monkeypatch.setattr(vpd_amd.augment.CropAugmenter, "__init__", lambda self, *a, **k: None)
    common = dict(dataset="fs", model_dir=str(tmp_path / "model"), out_dir=str(tmp_path / "out"), model_epoch=None,
                  flow_img=None, no_flip=False)
    apply_vpd_model.main(jitter=2, **common)
    assert seen["raw_u8"] is True and seen["ds_jitter"] == 0 and seen["jitter"] == 2 and seen["augmenter"] is not None
    apply_vpd_model.main(jitter=2, host_fp32=True, **common)
    assert seen["raw_u8"] is False and seen["ds_jitter"] == 2 and seen["jitter"] == 0 and seen["augmenter"] is None
