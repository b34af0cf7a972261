"""Resumable training: pure functions between the engine's flat state and the dictionaries a checkpoint holds.

Nothing here needs a GPU or the library: tensors may live on either side, the layout rows are StudentEngine.layout's
(kind, is_decoder, offset, numel, shape).  The formats are torch's own where torch has one -- torch.optim.AdamW.state_dict(),
torch.amp.GradScaler.state_dict() -- so that a state trained elsewhere loads here and the other way round.  Everything a
checkpoint file holds is tensors, numbers, strings, lists, tuples and dicts: it loads with torch.load(path, weights_only=True)."""
import os
import random

import numpy as np
import torch

from . import state_words as W

FORMAT_VERSION = 1
STATE_FILE = "train_state.pt"

# what torch.optim.AdamW keeps in every group besides lr / betas / eps / weight_decay: written into the dictionary so that
# torch.optim.AdamW.load_state_dict() finds its own keys (decoupled_weight_decay: AdamW is Adam with this flag in newer torch)
TORCH_ADAMW_GROUP_DEFAULTS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                                  decoupled_weight_decay=True)
SCALER_KEYS = ("scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker")      # GradScaler.state_dict()
FINGERPRINT_KEYS = ("format_version", "arch", "c_in", "emb_dim", "motion", "dtype", "param_numel")


# -- AdamW: flat moments <-> torch.optim.AdamW.state_dict() ------------------------------------------------------------
def _view(layout, name, buf):
    _, _, off, numel, shape = layout[name]
    return buf[off:off + numel].view(shape)


def _shared_hypers(groups):
    g0 = groups[0]
    for i, g in enumerate(groups[1:], start=1):
        if tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"]:
            raise ValueError("betas and eps must be the same in every parameter group (group %d has betas=%r, eps=%r, group 0 "
                             "betas=%r, eps=%r)" % (i, tuple(g["betas"]), g["eps"], tuple(g0["betas"]), g0["eps"]))


def adamw_state_dict(layout, adam_m, adam_v, step, names, param_groups):
    """torch.optim.AdamW.state_dict() of the flat moments.  names: the layout names of the optimizer's parameters in the
    optimizer's own order (index i of the dictionary is names[i]); param_groups: the optimizer's groups, 'params' replaced by
    their indices or absent (then filled in group order).  step == 0 or adam_m None: `state` is empty, as torch's is before the
    first step.  exp_avg / exp_avg_sq are VIEWS of adam_m / adam_v in the parameter's shape; step is a float32 scalar."""
    state = {}
    if adam_m is not None and int(step) > 0:
        for i, name in enumerate(names):
            state[i] = {"step": torch.tensor(float(int(step)), dtype=torch.float32),
                        "exp_avg": _view(layout, name, adam_m), "exp_avg_sq": _view(layout, name, adam_v)}
    groups, first = [], 0
    for g in param_groups:
        out = {k: v for k, v in g.items() if k != "params"}
        out["betas"] = tuple(out["betas"])
        for k, v in TORCH_ADAMW_GROUP_DEFAULTS.items():
            out.setdefault(k, v)
        n = len(g["params"])
        out["params"] = list(range(first, first + n))
        first += n
        groups.append(out)
    if first != len(names):
        raise ValueError("the parameter groups hold %d parameters, the order names %d" % (first, len(names)))
    return {"state": state, "param_groups": groups}


def adamw_load_flat(state_dict, layout, names, adam_m, adam_v):
    """The inverse: writes every exp_avg / exp_avg_sq of `state_dict` into its range of the flat adam_m / adam_v (floats between
    tensors are left as they are: zero in a buffer that was zeroed once) and returns the step all parameters share.  An empty
    `state` returns 0 and writes zeros.  ValueError: steps that differ, a parameter without state (or state for one the order
    does not name), a shape that is not the layout's, betas or eps that differ between groups, a group structure that does not
    cover the order."""
    groups = state_dict["param_groups"]
    _shared_hypers(groups)
    idx = [i for g in groups for i in g["params"]]
    if sorted(idx) != list(range(len(names))):
        raise ValueError("the dictionary's groups hold %d parameters, this optimizer has %d" % (len(idx), len(names)))
    state = state_dict["state"]
    if not state:
        for name in names:
            _view(layout, name, adam_m).zero_()
            _view(layout, name, adam_v).zero_()
        return 0
    extra = [k for k in state if not (isinstance(k, int) and 0 <= k < len(names))]
    if extra:
        raise ValueError("state for parameter %r, which this optimizer does not have" % (extra[0],))
    missing = [names[i] for i in range(len(names)) if i not in state]
    if missing:
        raise ValueError("no optimizer state for parameter %s%s" % (missing[0], "" if len(missing) == 1 else " (and %d more)" % (len(missing) - 1)))
    steps = {}
    for i, name in enumerate(names):
        s = state[i]
        for key in ("step", "exp_avg", "exp_avg_sq"):
            if key not in s:
                raise ValueError("the state of parameter %s lacks %r" % (name, key))
        steps.setdefault(float(s["step"]), name)
        shape = tuple(layout[name][4])
        for key in ("exp_avg", "exp_avg_sq"):
            if tuple(s[key].shape) != shape:
                raise ValueError("%s of parameter %s has shape %s, the layout says %s" % (key, name, tuple(s[key].shape), shape))
    if len(steps) != 1:
        (s0, n0), (s1, n1) = list(steps.items())[:2]
        raise ValueError("the parameters' steps differ (%s: %g, %s: %g): the fused step keeps one count for all" % (n0, s0, n1, s1))
    step = next(iter(steps))
    if step != int(step) or step < 0:
        raise ValueError("step %r is not a step count" % (step,))
    with torch.no_grad():
        for i, name in enumerate(names):
            _view(layout, name, adam_m).copy_(state[i]["exp_avg"])
            _view(layout, name, adam_v).copy_(state[i]["exp_avg_sq"])
    return int(step)


# -- the dynamic loss scaler: vpd_scale_state (vpd_amd.state_words) <-> GradScaler.state_dict() ----------------------------------
def scaler_state_dict(words, growth_factor, backoff_factor, growth_interval):
    """words: vpd_scale_state -- the host's int32[8], or state_words.read()'s struct -- -> GradScaler's five keys plus
    'skipped_steps'.  The applied-step word is the optimizer's `step`: not here."""
    if not isinstance(words, W.ScaleState):
        words = W.from_words(torch.as_tensor(words, dtype=torch.int32).cpu(), W.ScaleState)
    return {"scale": words.scale, "growth_factor": float(growth_factor), "backoff_factor": float(backoff_factor),
            "growth_interval": int(growth_interval), "_growth_tracker": words.growth_tracker, "skipped_steps": words.skipped_steps}


def scaler_fields(state):
    """The inverse, by name: the fields of vpd_scale_state a scaler dictionary holds.  A plain GradScaler dictionary (no
    'skipped_steps') gives skipped_steps = 0."""
    for k in SCALER_KEYS:
        if k not in state:
            raise ValueError("the scaler dictionary lacks %r" % (k,))
    scale = float(state["scale"])
    if not scale > 0.0:
        raise ValueError("loss scale must be positive, not %r" % (scale,))
    return dict(scale=scale, growth_tracker=int(state["_growth_tracker"]), skipped_steps=int(state.get("skipped_steps", 0)))


def scaler_words(state, applied_steps=0):
    """... as int32[8] on the host with the found word clear and `applied_steps` (the optimizer's step) in its word"""
    return W.host_block(W.ScaleState, applied_steps=int(applied_steps), **scaler_fields(state))


# -- random number generators --------------------------------------------------------------------------------------------
def capture_rng():
    """torch (CPU, and the current device when there is one), Python's `random` and numpy's global generator, as tensors, numbers,
    strings and lists"""
    out = {"torch": torch.get_rng_state().clone()}
    if torch.cuda.is_available():
        out["cuda"] = torch.cuda.get_rng_state().clone()
    version, internal, gauss = random.getstate()
    out["python"] = {"version": int(version), "state": [int(x) for x in internal], "gauss": None if gauss is None else float(gauss)}
    name, keys, pos, has_gauss, cached = np.random.get_state()
    out["numpy"] = {"name": str(name), "keys": torch.from_numpy(np.asarray(keys).astype(np.int64)), "pos": int(pos),
                    "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}
    return out


def restore_rng(state):
    torch.set_rng_state(state["torch"].cpu().to(torch.uint8))
    if "cuda" in state and torch.cuda.is_available():
        torch.cuda.set_rng_state(state["cuda"].cpu().to(torch.uint8))
    py = state["python"]
    random.setstate((py["version"], tuple(py["state"]), py["gauss"]))
    n = state["numpy"]
    np.random.set_state((n["name"], n["keys"].cpu().numpy().astype(np.uint32), n["pos"], n["has_gauss"], n["cached_gaussian"]))


def gather_rng(rank=0, world=1, group=None):
    """Every rank's capture_rng() as a list by rank (all_gather_object; one entry without data parallelism)"""
    mine = capture_rng()
    if world <= 1:
        return [mine]
    out = [None] * world
    torch.distributed.all_gather_object(out, mine, group=group)
    return out


def pick_rng(states, rank=0, world=1):
    """This rank's entry of a stored list; a list written by another world size raises"""
    if len(states) != world:
        raise ValueError("world size: the file was written by %d rank(s), this run has %d (changing the world size on resume is "
                         "not supported)" % (len(states), world))
    return states[rank]


# -- files -----------------------------------------------------------------------------------------------------------------
def write_atomic(obj, path):
    """torch.save to path + '.tmp', then os.replace: a failure while saving leaves the previous file as it was and no .tmp"""
    tmp = path + ".tmp"
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise


def read_state(path):
    return torch.load(path, map_location="cpu", weights_only=True)


# -- what a file belongs to --------------------------------------------------------------------------------------------------
def fingerprint(arch, c_in, emb_dim, motion, dtype, param_numel):
    return {"format_version": FORMAT_VERSION, "arch": str(arch), "c_in": int(c_in), "emb_dim": int(emb_dim), "motion": bool(motion),
            "dtype": str(dtype), "param_numel": int(param_numel)}


def check_fingerprint(stored, current):
    """ValueError naming the first field of FINGERPRINT_KEYS that differs, with both values"""
    for k in FINGERPRINT_KEYS:
        if k not in stored:
            raise ValueError("checkpoint fingerprint: no field %r in the file" % (k,))
        if stored[k] != current[k]:
            raise ValueError("checkpoint fingerprint: %s differs (file: %r, this trainer: %r)" % (k, stored[k], current[k]))


# -- the command line ----------------------------------------------------------------------------------------------------------
# (resume itself is what differs between the two invocations; save_dir says where the run lies, not what it is: a directory that
#  was moved, or is named by another path, still holds the same run)
RESUME_MAY_DIFFER = ("num_epochs", "checkpoint_frequency", "state_frequency", "resume", "save_dir")


def check_resume_dir(save_dir):
    """--resume: save_dir must exist and hold train_state.pt and config.json; FileNotFoundError names what is missing"""
    if not os.path.isdir(save_dir):
        raise FileNotFoundError("--resume: save_dir %r does not exist" % (save_dir,))
    for name in (STATE_FILE, "config.json"):
        if not os.path.isfile(os.path.join(save_dir, name)):
            raise FileNotFoundError("--resume: %r holds no %s" % (save_dir, name))
    return os.path.join(save_dir, STATE_FILE)


def check_resume_args(stored, current):
    """--resume: every argument but num_epochs, checkpoint_frequency and state_frequency must be what the stored run was given;
    ValueError names the key"""
    for k in sorted(set(stored) | set(current)):
        if k in RESUME_MAY_DIFFER:
            continue
        if k not in stored or k not in current:
            raise ValueError("--resume: argument %s is %s" % (k, "not in the stored run" if k not in stored else "not known to this script"))
        if stored[k] != current[k]:
            raise ValueError("--resume: argument %s differs (stored run: %r, now: %r)" % (k, stored[k], current[k]))
