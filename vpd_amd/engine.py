"""StudentEngine: device buffers + one libvpdhip plan for a student network.

PyTorch is used for device memory, streams and (in ddp.py) torch.distributed
only; every arithmetic step of the hot path is a hand-written HIP kernel behind
the C ABI (include/vpd_hip.h).  There is no fallback path.
"""
import ctypes as C
import os
from collections import OrderedDict

import torch

from . import state_words as W
from ._lib import check, has, lib, require

# reference: models/module.py:17-32 (ENCODER_ARCH): BasicBlock archs and the Bottleneck archs
ENCODER_LAYERS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3), "resnet50": (3, 4, 6, 3),
                  "resnet101": (3, 4, 23, 3), "wide_resnet50_2": (3, 4, 6, 3), "wide_resnet101_2": (3, 4, 23, 3)}
BOTTLENECK_ARCHS = ("resnet50", "resnet101", "wide_resnet50_2", "wide_resnet101_2")
_STAGE_WIDTH = (64, 128, 256, 512)


def _world_size():
    """Ranks of the default process group (1 when torch.distributed is not initialised)."""
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def encoder_param_names(arch):
    """Trainable tensors / BN buffers of the encoder in reference state_dict order."""
    if arch not in ENCODER_LAYERS:
        raise KeyError("unsupported encoder_arch %r (%s)" % (arch, " | ".join(ENCODER_LAYERS)))
    train, bns = ["resnet.conv1.weight", "resnet.bn1.weight", "resnet.bn1.bias"], ["resnet.bn1"]
    inpl = 64
    exp = 4 if arch in BOTTLENECK_ARCHS else 1
    for li, (nblk, planes) in enumerate(zip(ENCODER_LAYERS[arch], _STAGE_WIDTH), start=1):
        for bi in range(nblk):
            p = "resnet.layer%d.%d" % (li, bi)
            stride = 2 if (bi == 0 and li > 1) else 1
            train += [p + ".conv1.weight", p + ".bn1.weight", p + ".bn1.bias",
                      p + ".conv2.weight", p + ".bn2.weight", p + ".bn2.bias"]
            bns += [p + ".bn1", p + ".bn2"]
            if exp == 4:
                train += [p + ".conv3.weight", p + ".bn3.weight", p + ".bn3.bias"]
                bns.append(p + ".bn3")
            if stride != 1 or inpl != planes * exp:
                train += [p + ".downsample.0.weight", p + ".downsample.1.weight", p + ".downsample.1.bias"]
                bns.append(p + ".downsample.1")
            inpl = planes * exp
    train += ["resnet.fc.weight", "resnet.fc.bias"]
    return train, bns


DECODER_PARAM_NAMES = ["layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias",
                       "layers.5.weight", "layers.5.bias"]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class _Plan:
    """One vpd_plan_t + its workspace for a fixed (H, W, max_batch, train, motion)."""

    def __init__(self, eng, h, w, max_batch, train, motion):
        L = self.L = eng.L
        check = self.check = eng.check
        self.h, self.w, self.max_batch, self.train, self.motion = h, w, max_batch, train, motion
        handle = C.c_void_p()
        # data parallel, VPD_DDP_EARLY_BUCKET0=1: bucket 0 (fc + layer4, 61 % of the gradient bytes) is handed to the reducer at the
        # end of layer4's backward instead of behind layer3's (include/vpd_hip.h, VPD_TRAIN_EARLY_BUCKET0).  OFF by default: the two
        # weight-gradient launches it takes cost 3.1 % of a rank's step (profiles/r05_ab_wg_unmerge.txt) for certain, what the earlier
        # all-reduce buys is unmeasured until a multi-GPU node runs bench.py with the switch both ways
        flags = int(bool(train))
        self.early_bucket0 = bool(train) and _world_size() > 1 and os.environ.get("VPD_DDP_EARLY_BUCKET0", "0") == "1"
        if self.early_bucket0:
            flags |= 2
        check(L.vpd_plan_create(eng.arch.encode(), eng.c_in, h, w, eng.emb_dim, int(motion), max_batch, flags,
                                C.byref(handle)), "vpd_plan_create")
        self.handle = handle
        # the C side is the source of truth for the flat layout: verify ours
        n = L.vpd_plan_num_tensors(handle)
        rows = []
        kind, dec, off, numel, ndim = C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong(), C.c_int()
        dims = (C.c_int * 4)()
        for i in range(n):
            check(L.vpd_plan_tensor_info(handle, i, C.byref(kind), C.byref(dec), C.byref(off), C.byref(numel),
                                         C.byref(ndim), dims), "vpd_plan_tensor_info")
            rows.append((kind.value, dec.value, off.value, numel.value, tuple(dims[k] for k in range(ndim.value))))
        self.rows = rows
        self.param_numel = L.vpd_plan_param_numel(handle)
        self.ws_bytes = L.vpd_plan_workspace_bytes(handle)
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=eng.device)
        check(L.vpd_plan_init_workspace(handle, _ptr(self.workspace), eng._stream()), "vpd_plan_init_workspace")
        self.buckets = []
        o, m = C.c_longlong(), C.c_longlong()
        for b in range(L.vpd_plan_num_buckets(handle)):
            check(L.vpd_plan_bucket_range(handle, b, C.byref(o), C.byref(m)), "vpd_plan_bucket_range")
            self.buckets.append((o.value, m.value))
        self.packed_version = None
        self.graph_sizes = set()
        # a train plan holds ONE forward's activations: every train-mode forward bumps `fwd_count`, an autograd backward checks
        # the count its forward saw and marks it consumed (StudentEngine.backward_ext)
        self.fwd_count = 0
        self.consumed = None
        # what the plan was last told (vpd_plan_set_bn_frozen / vpd_plan_set_param_grads): the library's defaults
        self.bn_frozen, self.param_grads = False, True
        # lazy gradients under data parallelism: bucket b's conv weight gradients as a view of the workspace (the kernels' own
        # layout), and the flat-buffer positions of everything else (BatchNorm, fc, motion head, the stem conv)
        self.scratch_views, self.small_idx = [], None
        # gradient accumulation: where bucket b's scratch view lies in the accumulator's image of the scratch (floats; the bucket
        # ranges tile the scratch behind the stem's gradients), and the floats of the whole accumulator
        self.scratch_image_off, self.accum_numel = [], None
        if train:
            ranges = []
            for b in range(len(self.buckets)):
                check(L.vpd_plan_bucket_scratch_range(handle, b, C.byref(o), C.byref(m)), "vpd_plan_bucket_scratch_range")
                self.scratch_views.append(self.workspace[o.value:o.value + 4 * m.value].view(torch.float32))
                ranges.append((o.value, m.value))
            base = min([o_ for o_, m_ in ranges if m_ > 0] or [0])
            assert base % 16 == 0, "the scratch behind the stem must share the accumulator's 16-byte phase"
            self.scratch_image_off = [(o_ - base) // 4 if m_ > 0 else 0 for o_, m_ in ranges]
            if has(L, "vpd_plan_grad_accum_numel"):
                self.accum_numel = int(L.vpd_plan_grad_accum_numel(handle))
                assert self.accum_numel == sum(m_ for _, m_ in ranges) + self.param_numel, "accumulator != scratch ranges + param_numel"
            small = [(off_, n_) for i, (kind_, _, off_, n_, _) in enumerate(rows) if kind_ != 0 or i == 0]
            self.small_ranges = small
            # the C side is the source of truth: together the scratch views (every conv but the stem) and the small ranges
            # must cover the flat parameter buffer exactly once
            conv_numel = sum(n_ for i, (kind_, _, _, n_, _) in enumerate(rows) if kind_ == 0 and i != 0)
            assert sum(v.numel() for v in self.scratch_views) == conv_numel, "bucket scratch ranges != conv weight tensors"
            assert conv_numel + sum(n_ for _, n_ in small) == self.param_numel, "small ranges + conv tensors != param_numel"
            self.small_idx = torch.cat([torch.arange(a, a + n_, dtype=torch.int64) for a, n_ in small]).to(eng.device)

    def bn_table(self):
        L, check = self.L, self.check
        out = []
        ch, rm, rv = C.c_int(), C.c_longlong(), C.c_longlong()
        for i in range(L.vpd_plan_num_bn(self.handle)):
            check(L.vpd_plan_bn_info(self.handle, i, C.byref(ch), C.byref(rm), C.byref(rv)), "vpd_plan_bn_info")
            out.append((ch.value, rm.value, rv.value))
        return out

    def close(self):
        if self.handle:
            self.L.vpd_plan_destroy(self.handle)
            self.handle = None
        # whoever still holds this _Plan (apply's graph table, a reducer's last plan) must not pin its workspace
        self.workspace, self.scratch_views, self.small_idx = None, [], None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _StepCount:
    """The optimizer steps applied so far (AdamW's `step`), in its one home: the host integer, or -- once a device block counts, a
    DynamicLossScaler's or the clip block, because only the device knows whether a step was skipped -- that block's applied_steps."""

    def __init__(self):
        self.host, self.block = 0, None

    def get(self):
        """synchronises only when a block counts"""
        return self.host if self.block is None else int(self.block[_APPLIED].item())

    def set(self, value):
        self.host = int(value)
        if self.block is not None:
            self.block[_APPLIED] = int(value)

    def to_host(self):
        """the count comes back from the block (synchronises)"""
        self.host, self.block = self.get(), None


_APPLIED = W.word(W.ScaleState, "applied_steps")      # (a clip block begins with a vpd_scale_state: the same word in both)


class StudentEngine:
    """Flat fp32 parameter / gradient / optimizer-state buffers in the
    reference's state_dict order and layout, plus lazily created plans."""

    # accumulate_grads() / fold_accumulated_grads(): the sum of a window's micro-batches so far.  The accumulator (allocated on
    # first use: a K = 1 run never has one) holds an image of the weight-gradient scratch and one of the flat buffer
    _accum = None
    _accum_count = 0          # micro-batches held
    _accum_layout = None      # "scratch" (lazy backwards: scratch + the small ranges of the flat buffer) | "flat"

    def __init__(self, arch, c_in, emb_dim, device="cuda", dtype="bf16"):
        if not torch.cuda.is_available():
            raise RuntimeError("vpd_amd needs a ROCm GPU (MI355X): torch.cuda.is_available() is False; "
                               "there is no CPU fallback for the student path")
        # dtype: element type of activations / packed weights -- "bf16" (libvpdhip.so: training and inference) or "fp16"
        # (libvpdhip_f16.so: the reference's own GPU precision, train_vpd_model.py:79; training goes through a loss scaler)
        self.dtype = dtype
        self.L = lib(dtype)   # fail loudly right here if the HIP library is missing
        self.check = lambda rc, what="": check(rc, what, dtype)
        self.arch, self.c_in, self.emb_dim = arch, int(c_in), int(emb_dim)
        self.device = torch.device(device)
        self.enc_names, self.bn_names = encoder_param_names(arch)
        # a throw-away 1-crop plan tells us the flat layout (shapes/offsets) without duplicating it here
        probe = _Plan(self, 64, 64, 1, False, True)
        assert len(probe.rows) == len(self.enc_names) + len(DECODER_PARAM_NAMES)
        self.layout = OrderedDict()
        for name, row in zip(self.enc_names + ["decoder." + k for k in DECODER_PARAM_NAMES], probe.rows):
            self.layout[name] = row
        self.param_numel = probe.param_numel
        self.bn_layout = OrderedDict(zip(self.bn_names, probe.bn_table()))
        self.bn_numel = sum(2 * c for c, _, _ in self.bn_layout.values())
        probe.close()

        z = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(self.param_numel, **z)
        self._grads = torch.zeros(self.param_numel, **z)      # see the `grads` property
        self.bn_running = torch.zeros(max(self.bn_numel, 1), **z)
        # nn.BatchNorm2d.num_batches_tracked of every BatchNorm: counted on the host and added to the device tensor when it is
        # read (the property below, state_dict()) -- a one-element-per-BatchNorm add per step is a 5 us launch of its own
        self._nbt = torch.zeros(len(self.bn_names), dtype=torch.int64, device=self.device)
        self._nbt_pending = 0
        self.loss_step = torch.zeros(1, **z)
        self.loss_accum = torch.zeros(1, dtype=torch.float64, device=self.device)
        self._plans = {}
        self._hip_version = 0          # bumped when a HIP kernel (AdamW) rewrites params behind torch's back
        self._last = None              # (plan, n) of the last train forward, consumed by backward
        self._step_plan = None         # plan of the last backward: its packed weights are refreshed by adamw_step
        self.bucket_events = None
        # the autograd path (models/rgb.py, backward_ext): torch's accumulate semantics of .grad on top of kernels that overwrite
        self._last_fwd = None          # (plan, n, forward count, took an fp32 x) of the last train forward
        self._grads_cleared = True     # nothing to add onto: the flat buffer is fresh, or an optimizer's zero_grad() said so
        self._grads2 = None            # second flat buffer an accumulating backward writes before it is added (first use)
        self.stem_dgrad_launches = 0   # input gradients asked for (conv_stem_dgrad_kernel launches)
        self.bn_frozen = False         # freeze_bn(): train-mode forwards normalise with the running statistics and leave them alone
        self._reset_step_state()

    def _reset_step_state(self):
        """What the optimizer step keeps from one call to the next, as a new engine has it"""
        self.adam_m = None
        self.adam_v = None
        self._steps = _StepCount()     # see the `adam_step` property
        self.loss_scale = 1.0          # set by models.util.LossScaler around a backward pass + optimizer step (fp16 training)
        # models.util.DynamicLossScaler: its device block (vpd_scale_state) while a scaled backward pass + optimizer step are in
        # flight (the scale is then read on the device)
        self.scale_state = None
        # enable_grad_clip(): the device block of the gradient-norm clipping (vpd_clip_state + partial sums, int32 words)
        self._clip = None
        self._clip_max_norm = None
        # enable_ema(): exponential moving average of `params` / `bn_running`, updated by one kernel at the end of adamw_step
        self.ema_params = None
        self.ema_bn_running = None
        self._ema = None               # (decay, warmup)
        self._ema_t = 0                # updates enqueued without a device block (behind one the device counts: see _ema_t_host)
        self._ema_t0 = 0               # adam_step when averaging began
        self._ema_version = 0          # bumped by every update: plans packed from the EMA buffers repack
        self._use_ema = False          # use_ema(): eval forwards read the EMA buffers
        # adamw_step(groups=...): the device segment table of the last grouping (vpd_adam_groups_init) and what it was built from
        self._group_table = None
        self._group_table_key = None
        self.group_table_builds = 0
        self._accum, self._accum_count, self._accum_layout = None, 0, None      # (the class attributes above)

    def _count_half(name):
        """`_adam_step` / `_dyn_state`: the two halves of `_steps` under the names of before it, for an engine that a test builds
        without __init__ and fills by hand"""
        def put(self, value):
            if "_steps" not in self.__dict__:
                self._steps = _StepCount()
            setattr(self._steps, name, value)
        return property(lambda self: getattr(self._steps, name), put)
    _adam_step, _dyn_state = _count_half("host"), _count_half("block")

    # -- helpers -------------------------------------------------------------
    @property
    def adam_step(self):
        """Optimizer steps applied so far (1-based `step` of the last AdamW).  Behind a device block only the device knows it
        after a skipped step: read from the block (synchronises)."""
        return self._steps.get()

    @adam_step.setter
    def adam_step(self, value):
        self._steps.set(value)

    def attach_scale_state(self, state):
        """models.util.DynamicLossScaler: from now on the applied-step count lives in `state` (it starts at adam_step)."""
        self._steps.block = state

    def scale_state_update(self, block, growth, backoff, interval):
        """The one-thread kernel that closes a step behind `block`: counts it as applied or skipped, moves the scale
        (DynamicLossScaler.update(); the clip block's own count in adamw_step passes factors of 1)"""
        self.check(self.L.vpd_scale_state_update(_ptr(block), growth, backoff, interval, self._stream()), "vpd_scale_state_update")

    def unscale_grads_by_block_(self, block):
        """The flat gradient buffer x 1 / the scale in `block`, the reciprocal taken on the device: no synchronisation"""
        scale = W.word(W.ScaleState, "scale")
        self._grads.mul_(1.0 / block[scale:scale + 1].view(torch.float32))

    def check_grads_finite_(self, state):
        """The non-finite search over the completed flat gradient buffer (a scaler in front of an optimizer that reads p.grad)."""
        self.materialize_grads()
        self.check(self.L.vpd_op_check_finite(_ptr(self._grads), self.param_numel, _ptr(state), self._stream()),
                   "vpd_op_check_finite")

    # -- gradient-norm clipping -----------------------------------------------------
    def enable_grad_clip(self, max_norm):
        """torch.nn.utils.clip_grad_norm_(parameters, max_norm) inside adamw_step(), decided on the device: one pass takes the norm
        of exactly the gradients the step reads (after a lazy backward: the weight-gradient scratch + the small ranges of the flat
        buffer), a one-block kernel turns it into coef = min(1, max_norm / (norm + 1e-6)) and into the block AdamW and the EMA
        read (include/vpd_hip.h, vpd_clip_state).  Under a DynamicLossScaler the pass replaces the non-finite search.  Without one
        a non-finite norm SKIPS the step and counts it (torch would write NaN into every weight).  As attach_scale_state does,
        this moves the applied-step count to the device.  float('inf') measures without clipping."""
        max_norm = float(max_norm)
        if not max_norm > 0.0:
            raise ValueError("max_grad_norm must be > 0 (float('inf') measures only), not %r" % (max_norm,))
        require(self.L, "vpd_plan_grad_norm")
        if self._clip is None:
            step = int(self.adam_step)
            self._clip = torch.zeros(int(self.L.vpd_clip_state_bytes()) // 4, dtype=torch.int32, device=self.device)
            self._clip[_APPLIED] = step
            if self._steps.block is None:
                self._steps.block = self._clip      # (a DynamicLossScaler's block keeps the count when there is one)
        self._clip_max_norm = max_norm

    def disable_grad_clip(self):
        """adamw_step launches what it launched before enable_grad_clip(); the step count comes back to the host when the clip
        block held it (synchronises)."""
        if self._clip is None:
            return
        if self._steps.block is self._clip:
            self._steps.to_host()
        self._clip = None
        self._clip_max_norm = None

    @property
    def grad_clip_enabled(self):
        return self._clip is not None

    @property
    def clip_max_norm(self):
        return self._clip_max_norm

    def clip_stats(self, reset_max=False):
        """The statistics of the clip block (synchronises): the last step's norm and coefficient, the running maximum of the
        finite norms, the steps clipped and the steps whose norm was not finite.  reset_max: norm_max starts again at 0."""
        if self._clip is None:
            raise RuntimeError("clip_stats() before enable_grad_clip()")
        h = W.read(self._clip, W.ClipState)
        if reset_max:
            self._clip[W.word(W.ClipState, "norm_max")] = 0
        return dict(total_norm=h.total_norm, norm_max=h.norm_max, coef=h.coef, clipped_steps=h.clipped_steps,
                    nonfinite_steps=h.nonfinite_steps)

    def _clip_norm(self, pl, numel, src):
        """enqueue the norm pass + the one-block kernel over what the step that follows reads (pl: its plan, or None = the flat
        buffer); src: the DynamicLossScaler's block in flight, or None = the host's static loss scale"""
        clip = self._clip
        if pl is not None:
            self.check(self.L.vpd_plan_grad_norm(pl.handle, _ptr(self._grads), numel, self._clip_max_norm, _ptr(src),
                                                 float(self.loss_scale), _ptr(clip), _ptr(pl.workspace), self._stream()),
                       "vpd_plan_grad_norm")
        else:
            x = (C.c_void_p * 1)(self._grads.data_ptr())
            n = (C.c_longlong * 1)(numel)
            self.check(self.L.vpd_op_grad_norm(x, n, 1, self._clip_max_norm, _ptr(src), float(self.loss_scale), _ptr(clip),
                                               self._stream()), "vpd_op_grad_norm")

    @property
    def num_batches_tracked(self):
        """int64[len(bn_names)] on the device, up to date (train-mode forwards since the last read are added first)"""
        if self._nbt_pending:
            self._nbt += self._nbt_pending
            self._nbt_pending = 0
        return self._nbt

    @property
    def grads(self):
        """The flat fp32 gradient buffer (reference layouts; every p.grad is a view of it).  After a LAZY backward -- the one
        models.util.step() runs between forward and optimizer step, where the reference never looks at .grad either -- the
        conv weight gradients are still in the kernels' own layout: reading this property completes the buffer first."""
        self.materialize_grads()
        return self._grads

    @property
    def flat_grads(self):
        """The same buffer as it stands: after a lazy backward its conv weight ranges are stale (a reducer that sums the scratch
        instead, a p.grad view that is completed before anybody reads it)"""
        return self._grads

    @property
    def grads_cleared(self):
        """nothing to add onto: the flat buffer is fresh, or mark_grads_cleared() said so (the autograd path's accumulate rule)"""
        return self._grads_cleared

    def mark_grads_cleared(self):
        """an optimizer's zero_grad(): the next autograd backward overwrites the flat buffer instead of adding onto it"""
        self._grads_cleared = True

    @property
    def step_plan(self):
        """the train plan of the last backward (adamw_step goes through it), or None"""
        return self._step_plan

    def materialize_grads(self):
        pl = self._step_plan
        if pl is not None and pl.handle and self.L.vpd_plan_grads_pending(pl.handle):
            self.check(self.L.vpd_plan_materialize_grads(pl.handle, _ptr(self._grads), _ptr(pl.workspace), self._stream()),
                  "vpd_plan_materialize_grads")

    # -- gradient accumulation over micro-batches ---------------------------------------
    def _accum_check(self, pl, what):
        """the plan whose live gradients `what` is about to pair with the accumulator, and the layout they are in"""
        if pl is None or not pl.handle:
            raise RuntimeError("%s without a preceding backward" % what)
        require(self.L, "vpd_plan_grad_accumulate", "gradient accumulation")
        layout = "scratch" if self.L.vpd_plan_grads_pending(pl.handle) else "flat"
        if self._accum_count:
            if layout != self._accum_layout:
                raise RuntimeError("%s: the accumulator holds %d micro-batch(es) in the %s layout, the live gradients are in the %s "
                                   "layout (lazy and eager backwards do not mix inside a window)"
                                   % (what, self._accum_count, self._accum_layout, layout))
            if pl.accum_numel != self._accum.numel():
                raise RuntimeError("%s: the accumulator holds %d floats, this plan's takes %d"
                                   % (what, self._accum.numel(), pl.accum_numel))
        return layout

    def _accum_call(self, pl, mode):
        self.check(self.L.vpd_plan_grad_accumulate(pl.handle, _ptr(self._grads), pl.param_numel, _ptr(self._accum), mode,
                                                   _ptr(pl.workspace), self._stream()), "vpd_plan_grad_accumulate")

    def accumulate_grads(self):
        """A non-final micro-batch of an accumulation window: the live gradients of the last backward -- in whichever layout it
        left them -- are stored into the accumulator (first micro-batch of the window: the store never reads it) or added onto
        it, one streaming launch; the pending state is consumed without the layout pass.  The loss is a sum over crops, so the
        window's sum is the big batch's gradient: no 1/K."""
        pl = self._step_plan
        layout = self._accum_check(pl, "accumulate_grads()")
        if self._accum is None or (not self._accum_count and self._accum.numel() != pl.accum_numel):
            self._accum = torch.zeros(pl.accum_numel, dtype=torch.float32, device=self.device)
        self._accum_call(pl, 1 if self._accum_count else 0)
        self._accum_count += 1
        self._accum_layout = layout

    def fold_accumulated_grads(self):
        """The final micro-batch: live += accumulator, in place, in the layout the last backward left; everything that reads the
        live gradients afterwards (search, norm pass, AdamW, a torch optimizer through `grads`) runs unchanged.  A no-op when
        nothing is held; the accumulator is empty afterwards.  adamw_step() calls it first."""
        if not self._accum_count:
            return
        pl = self._step_plan
        self._accum_check(pl, "fold_accumulated_grads()")
        self._accum_call(pl, 2)
        self._accum_count = 0

    def accum_images(self, pl):
        """(per-bucket views of the accumulator's image of the scratch, its image of the flat buffer) for a reducer that folds
        bucket by bucket on its own stream; checks layout and size as fold_accumulated_grads() does"""
        self._accum_check(pl, "GradBucketReducer.reduce()")
        nscratch = pl.accum_numel - pl.param_numel
        views = [self._accum[a:a + v.numel()] for a, v in zip(pl.scratch_image_off, pl.scratch_views)]
        return views, self._accum[nscratch:nscratch + pl.param_numel]

    def drop_accumulated_grads(self):
        """Forget what the accumulator holds (the memory stays)."""
        self._accum_count = 0

    def hold_accumulated_grads(self, layout):
        """The inverse, for a measurement of the fold alone: what the accumulator last held, in `layout`, counts as ONE micro-batch
        again"""
        if self._accum is None or self._accum_layout != layout:
            raise RuntimeError("hold_accumulated_grads(%r): the accumulator last held %r" % (layout, self._accum_layout))
        self._accum_count = 1

    @property
    def accumulator(self):
        """the accumulator's buffer (None before the first accumulate_grads())"""
        return self._accum

    @property
    def held_micro_batches(self):
        """micro-batches of the current accumulation window that the accumulator holds"""
        return self._accum_count

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def stream(self):
        """the current stream of the engine's device, as the library's entry points take it"""
        return self._stream()

    def view(self, name, buf=None):
        kind, dec, off, numel, shape = self.layout[name]
        return (self.params if buf is None else buf)[off:off + numel].view(shape)

    def bn_views(self, name):
        c, rm, rv = self.bn_layout[name]
        return self.bn_running[rm:rm + c], self.bn_running[rv:rv + c]

    def weights_version(self):
        """What a plan's packed weights were made from: the live buffers' versions, and -- while use_ema() is on -- the source flag
        and the EMA buffers' version (0 otherwise: an EMA update does not make the packed LIVE weights stale)."""
        return (self.params._version, self.bn_running._version, self._hip_version, self._use_ema,
                self._ema_version if self._use_ema else 0)

    # -- exponential moving average of the weights ---------------------------------
    def enable_ema(self, decay, warmup=False):
        """Keep an exponential moving average of the parameters and of the BatchNorm running statistics (timm's ModelEmaV2 averages
        buffers too; num_batches_tracked stays the live one): ema += (1 - d) * (live - ema) after every applied optimizer step,
        d = decay, or min(decay, (1 + t) / (10 + t)) with warmup, t = updates so far.  `ema_params` / `ema_bn_running` start as
        copies of the live buffers.  adamw_step() then ends with ONE more launch (vpd_ema_update) over both buffers; under a
        DynamicLossScaler it reads the scaler's block, so a skipped step leaves the average alone and costs no synchronisation."""
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError("ema decay must be in [0, 1], not %r" % (decay,))
        require(self.L, "vpd_ema_update")
        self.ema_params = self.params.clone()
        self.ema_bn_running = self.bn_running.clone()
        self._ema = (decay, bool(warmup))
        self._ema_t = 0
        self._ema_t0 = int(self.adam_step)      # (read once; synchronises when a DynamicLossScaler is attached)
        self._ema_version += 1

    def disable_ema(self):
        """Stop averaging (adamw_step launches what it launched before enable_ema); the buffers keep their values."""
        self._ema = None
        self._use_ema = False

    @property
    def ema_enabled(self):
        return self._ema is not None

    @property
    def ema_config(self):
        """(decay, warmup) of enable_ema(), or None"""
        return self._ema

    @property
    def ema_in_use(self):
        """use_ema() is on: eval forwards read the averaged weights"""
        return self._use_ema

    def _ema_t_host(self, block):
        """Which side counts the EMA's updates behind `block` (the device block of a step, or None): `_ema_t` -- without a block
        the host counts -- or None: the device does, as the block's applied steps - `_ema_t0`, so that a skipped step leaves the
        count alone and costs no synchronisation"""
        return self._ema_t if block is None else None

    def _ema_enqueue(self, state):
        decay, warmup = self._ema
        t = self._ema_t_host(state)
        src = (C.c_void_p * 2)(self.params.data_ptr(), self.bn_running.data_ptr())
        dst = (C.c_void_p * 2)(self.ema_params.data_ptr(), self.ema_bn_running.data_ptr())
        n = (C.c_longlong * 2)(self.param_numel, self.bn_numel)
        self.check(self.L.vpd_ema_update(src, dst, n, 2, decay, int(warmup), 0 if t is None else t, self._ema_t0, _ptr(state),
                                         self._stream()), "vpd_ema_update")
        if t is not None:
            self._ema_t += 1
        self._ema_version += 1

    def ema_update(self):
        """One update of the average from the live buffers as they stand: the manual call for a torch optimizer on the autograd
        path, where the host knows whether it stepped (adamw_step() calls it by itself)."""
        if self._ema is None:
            raise RuntimeError("ema_update() before enable_ema()")
        self._ema_enqueue(None)

    def use_ema(self, on=True):
        """Eval forwards compute with the averaged weights while on (every plan repacks when the source changes, and only then);
        train-mode forwards refuse to run until it is off again.  The live buffers are not touched."""
        if on and self._ema is None:
            raise RuntimeError("use_ema() before enable_ema()")
        self._use_ema = bool(on)

    def _source(self):
        """(params, bn_running) the eval forwards read"""
        return (self.ema_params, self.ema_bn_running) if self._use_ema else (self.params, self.bn_running)

    # -- state for a checkpoint (ModelTrainer.save_state / load_state) -----------------------------------------------
    def ema_state(self):
        """The average as a checkpoint holds it: the two buffers (themselves, not copies), decay, warmup and `num_updates` -- one
        number whichever side counts: `_ema_t` on the host, applied steps - `_ema_t0` behind a device block (synchronises)."""
        if self._ema is None:
            raise RuntimeError("ema_state() before enable_ema()")
        n = self._ema_t_host(self._steps.block)
        if n is None:
            n = int(self.adam_step) - self._ema_t0
        return {"params": self.ema_params, "bn_running": self.ema_bn_running, "decay": self._ema[0], "warmup": self._ema[1],
                "num_updates": int(n)}

    def load_ema_state(self, state):
        """Restore ema_state() into an engine whose averaging is on.  Call it AFTER the optimizer's load: the count behind a device
        block is relative to adam_step (`_ema_t0 = adam_step - num_updates`; the host's `_ema_t = num_updates` serves the other
        mode)."""
        if self._ema is None:
            raise RuntimeError("load_ema_state() before enable_ema()")
        p, b = state["params"], state["bn_running"]
        if p.numel() != self.ema_params.numel() or b.numel() != self.ema_bn_running.numel():
            raise ValueError("EMA: the stored buffers hold %d + %d floats, this engine's %d + %d"
                             % (p.numel(), b.numel(), self.ema_params.numel(), self.ema_bn_running.numel()))
        n = int(state["num_updates"])
        if n < 0:
            raise ValueError("EMA: num_updates %d" % n)
        self.ema_params.copy_(p)
        self.ema_bn_running.copy_(b)
        self._ema = (float(state["decay"]), bool(state["warmup"]))
        self._ema_t, self._ema_t0 = n, max(int(self.adam_step) - n, 0)      # (both sides of _ema_t_host)
        self._ema_version += 1

    def clip_state(self):
        """What of the clip block outlives a step: max_norm and the statistics clip_stats() accumulates (synchronises)"""
        if self._clip is None:
            raise RuntimeError("clip_state() before enable_grad_clip()")
        st = self.clip_stats()
        return {"max_norm": float(self._clip_max_norm), "norm_max": st["norm_max"], "clipped_steps": st["clipped_steps"],
                "nonfinite_steps": st["nonfinite_steps"]}

    def load_clip_state(self, state):
        """Restore clip_state() into the words clip_stats() reads; the block's step word follows adam_step, so call it AFTER the
        optimizer's load."""
        if self._clip is None:
            raise RuntimeError("load_clip_state() before enable_grad_clip()")
        max_norm = float(state["max_norm"])
        if not max_norm > 0.0:
            raise ValueError("max_grad_norm must be > 0, not %r" % (max_norm,))
        W.write(self._clip, W.ClipState, norm_max=float(state["norm_max"]), applied_steps=int(self.adam_step),
                clipped_steps=int(state["clipped_steps"]), nonfinite_steps=int(state["nonfinite_steps"]))
        self._clip_max_norm = max_norm

    def mark_weights_changed(self):
        """Call after writing `params` / `bn_running` by a path torch's version counters do not see (a collective, a
        raw pointer): every plan repacks its bf16 weights before its next forward."""
        self._hip_version += 1

    def plan(self, h, w, n, train, motion):
        key = (h, w, bool(train), bool(motion))
        pl = self._plans.get(key)
        if pl is None or pl.max_batch < n:
            if pl is not None:
                if self._step_plan is pl:
                    self.materialize_grads()       # a pending lazy backward lives in the workspace that is about to go
                    self._step_plan = None
                pl.close()
            pl = _Plan(self, h, w, max(n, pl.max_batch if pl else 0), train, motion)
            assert pl.param_numel <= self.param_numel      # plans without the motion head omit its tensors
            self._plans[key] = pl
        return pl

    def _ensure_packed(self, pl):
        v = self.weights_version()
        if pl.packed_version != v:
            # the eval-mode BN fold is only needed by eval plans
            params, bn_running = self._source()
            self.check(self.L.vpd_pack_weights(pl.handle, _ptr(params), None if pl.train else _ptr(bn_running),
                                         _ptr(pl.workspace), self._stream()), "vpd_pack_weights")
            pl.packed_version = v

    @staticmethod
    def _check_input(x, c_in):
        assert x.dim() == 4 and x.shape[1] == c_in, "expected f32 [N,%d,H,W], got %s" % (c_in, tuple(x.shape))
        assert x.dtype == torch.float32 and x.is_contiguous() and x.is_cuda

    def freeze_bn(self, mode=True):
        """Frozen BatchNorm for the train plans (vpd_plan_set_bn_frozen): from the next train-mode forward on, every BatchNorm
        normalises with its running statistics and does not update them; the backward of a forward uses the mode that forward
        ran in.  Eval plans are not concerned (they fold the running statistics already)."""
        if mode:
            require(self.L, "vpd_plan_set_bn_frozen", "frozen BatchNorm")
        self.bn_frozen = bool(mode)

    def _plan_flag(self, pl, attr, setter, on):
        if getattr(pl, attr) != on:
            self.check(getattr(self.L, setter)(pl.handle, int(on)), setter)
            setattr(pl, attr, on)

    # -- forward / backward / step ---------------------------------------------
    def _batch_shape(self, x, staged):
        """(n, h, w) of a forward's batch: of x, or -- staged = (n, img_dim) -- of what stage_crops / stage_views left in the
        plan's staging buffer"""
        if staged is not None:
            n, h = staged
            return n, h, h
        self._check_input(x, self.c_in)
        n, _, h, w = x.shape
        return n, h, w

    def forward_eval(self, x, target=None, motion=False, out=None, accumulate_loss=True, staged=None):
        n, h, w = self._batch_shape(x, staged)
        pl = self.plan(h, w, n, False, motion)
        self._ensure_packed(pl)
        emb = out if out is not None else torch.empty((n, self.emb_dim), dtype=torch.float32, device=self.device)
        self.check(self.L.vpd_forward_eval(pl.handle, _ptr(self._source()[0]), _ptr(x), n, _ptr(emb), _ptr(target),
                                     _ptr(self.loss_step) if target is not None else None,
                                     _ptr(self.loss_accum) if (target is not None and accumulate_loss) else None,
                                     _ptr(pl.workspace), self._stream()), "vpd_forward_eval")
        return emb

    def _stage_target(self, rgb_u8, mean_std6, views=1, img_dim=None, train=False, motion=False):
        """what the three stagings share: (the plan whose staging buffer takes `views` views of every frame -- at img_dim, default
        the frames' own size --, n, h, w of the frames, mean_std6 as the C array)"""
        n, h, w, _ = rgb_u8.shape
        pl = self.plan(img_dim or h, img_dim or w, n * views, train, motion)
        return pl, n, h, w, (C.c_float * 6)(*mean_std6)

    def stage_crops(self, rgb_u8, flow_u8, mask_u8, params_dev, noise, img_dim, mean_std6, noise_sd, scratch, train,
                    motion=False):
        """Device input pipeline (vpd_amd.augment) writing straight into the plan's stem staging buffer; follow with
        forward_train / forward_eval(x=None, staged=(n, img_dim))."""
        pl, n, h, w, ms = self._stage_target(rgb_u8, mean_std6, 1, img_dim, train, motion)
        self.check(self.L.vpd_plan_stage_crops(pl.handle, _ptr(rgb_u8), _ptr(flow_u8), _ptr(mask_u8), _ptr(noise),
                                         _ptr(params_dev), n, h, w, ms, float(noise_sd), _ptr(scratch),
                                         _ptr(pl.workspace), self._stream()), "vpd_plan_stage_crops")
        return pl

    def stage_views(self, rgb_u8, flow_u8, k_views, mean_std6):
        """Inference views [frame, h-flip] of decoded u8 frames straight into the EVAL plan's stem staging buffer
        (vpd_plan_stage_views: table-driven normalisation, bit-identical to stage_crops with identity parameters)."""
        pl, n, h, w, ms = self._stage_target(rgb_u8, mean_std6, k_views)
        self.check(self.L.vpd_plan_stage_views(pl.handle, _ptr(rgb_u8), _ptr(flow_u8), n, k_views, h, w, ms,
                                         _ptr(pl.workspace), self._stream()), "vpd_plan_stage_views")
        return pl

    def stage_views_jitter(self, rgb_u8, flow_u8, params_dev, jitter, flip, mean_std6, scratch):
        """Jittered inference views [frame, J x jitter(frame), J x jitter(flip), flip] of decoded u8 frames straight into the
        EVAL plan's stem staging buffer (vpd_plan_stage_views_jitter; params_dev: device rows of vpd_aug_params, frame-major
        in view order)."""
        pl, n, h, w, ms = self._stage_target(rgb_u8, mean_std6, (1 + jitter) * (2 if flip else 1))
        self.check(self.L.vpd_plan_stage_views_jitter(pl.handle, _ptr(rgb_u8), _ptr(flow_u8), _ptr(params_dev), n, jitter,
                                                      1 if flip else 0, h, w, ms, _ptr(scratch), _ptr(pl.workspace),
                                                      self._stream()), "vpd_plan_stage_views_jitter")
        return pl

    def forward_train(self, x, target=None, motion=False, accumulate_loss=True, staged=None):
        n, h, w = self._batch_shape(x, staged)
        if self._use_ema:
            raise RuntimeError("train-mode forward while use_ema() is on: the averaged weights are for evaluation; "
                               "call use_ema(False) (or leave ModelTrainer.ema_weights()) first")
        pl = self.plan(h, w, n, True, motion)
        self._ensure_packed(pl)
        emb = torch.empty((n, self.emb_dim), dtype=torch.float32, device=self.device)
        if target is not None:
            want = (n, self.emb_dim * (2 if motion else 1))
            assert tuple(target.shape) == want and target.dtype == torch.float32 and target.is_contiguous(), \
                "target must be f32 %s" % (want,)
        frozen = self.bn_frozen
        self._plan_flag(pl, "bn_frozen", "vpd_plan_set_bn_frozen", frozen)
        self.check(self.L.vpd_forward_train(pl.handle, _ptr(self.params), _ptr(self.bn_running), _ptr(x), _ptr(target), n,
                                      _ptr(emb), _ptr(self.loss_step),
                                      _ptr(self.loss_accum) if accumulate_loss else None,
                                      _ptr(pl.workspace), self._stream()), "vpd_forward_train")
        if not frozen:      # (a frozen forward read the running statistics and left them: nothing is stale, nothing was tracked)
            # BN running stats were rewritten by HIP kernels: packed eval scale/shift are stale
            self._hip_version += 1
            pl.packed_version = self.weights_version()
            if n > 0:
                self._nbt_pending += 1
        self._last = (pl, n) if target is not None else None
        pl.fwd_count += 1
        self._last_fwd = (pl, n, pl.fwd_count, x is not None)
        return emb

    def pending_forward_buckets(self):
        """gradient buckets of the plan whose train forward backward() is about to consume (0: there is none, backward() raises)"""
        return len(self._last[0].buckets) if self._last is not None else 0

    def forward_ticket(self):
        """what identifies the last train-mode forward to backward_ext(ticket=): take it right after the forward"""
        return self._last_fwd

    def backward(self, events=None, lazy=False):
        """lazy: leave the conv weight gradients in the weight-gradient kernels' scratch layout for the fused optimizer step
        (with bucket events, i.e. under data parallelism, the reducer must then be told: reduce(plan, lazy=True))."""
        if self._last is None:
            raise RuntimeError("backward() without a preceding train-mode forward with a target")
        pl, n = self._last
        self._last = None
        self.materialize_grads()           # a pending lazy backward of the PREVIOUS step plan (possibly another plan) first
        self._step_plan = pl
        ev = None
        if events is not None:
            ev = (C.c_void_p * len(events))(*[C.c_void_p(e) for e in events])
        if self.loss_scale != 1.0 or has(self.L, "vpd_plan_set_loss_scale"):
            self.check(self.L.vpd_plan_set_loss_scale(pl.handle, float(self.loss_scale)), "vpd_plan_set_loss_scale")
        want = None if self.scale_state is None else self.scale_state.data_ptr()
        if getattr(pl, "scale_state_ptr", None) != want:      # (never called without a dynamic scaler)
            self.check(self.L.vpd_plan_set_scale_state(pl.handle, _ptr(self.scale_state)), "vpd_plan_set_scale_state")
            pl.scale_state_ptr = want
        if lazy:      # (with bucket events the reducer sums the scratch ranges: GradBucketReducer.reduce(plan, lazy=True))
            self.check(self.L.vpd_plan_set_lazy_grads(pl.handle, 1), "vpd_plan_set_lazy_grads")
        self.check(self.L.vpd_backward(pl.handle, _ptr(self.params), _ptr(self._grads), n, ev, _ptr(pl.workspace),
                                 self._stream()), "vpd_backward")
        pl.consumed = pl.fwd_count
        self._grads_cleared = False        # (an autograd backward that follows without a zero_grad() adds onto these)
        return pl

    def backward_ext(self, d_emb, want_dx=False, ticket=None, accumulate=False, discard=False):
        """loss.backward() from the caller's d(loss)/d(emb) (vpd_backward_ext) through the activations of a train-mode forward of
        the plan WITHOUT the motion head -- `ticket`: forward_ticket() right after that forward (default: the last one).
        d_emb: f32 [n, emb_dim] on the engine's device, contiguous; no loss scale is passed (a scaled loss arrives scaled).
        accumulate: add onto the flat gradient buffer instead of overwriting it (backward into a second buffer + one add);
        discard: leave the flat buffer alone (no parameter asks for a gradient): the pass then computes data gradients only
        (vpd_plan_set_param_grads(0): no weight-gradient launch, nothing written to a gradient buffer).  want_dx: also return d(loss)/d(x), f32
        [n, c_in, H, W] (the stem convolution's data gradient; only after a forward that took x).  Returns dx or None.
        Raises RuntimeError when a later train-mode forward overwrote the activations, and on a second backward through the same
        forward (the pass consumes them: retain_graph does not apply)."""
        if ticket is None:
            ticket = self._last_fwd
        if ticket is None:
            raise RuntimeError("backward_ext() without a preceding train-mode forward")
        pl, n, count, had_x = ticket
        if pl.motion:
            raise RuntimeError("backward_ext() differentiates the encoder: the forward must be forward_train(..., motion=False)")
        if pl.handle is None or pl.fwd_count != count:
            raise RuntimeError("a later train-mode forward overwrote the activations of this forward (a train plan holds one "
                               "forward's activations): call backward() before the next train-mode forward")
        if pl.consumed == count:
            raise RuntimeError("backward through this forward ran already: the pass consumes the plan's activations "
                               "(retain_graph=True does not apply; run the forward again)")
        assert isinstance(d_emb, torch.Tensor) and tuple(d_emb.shape) == (n, self.emb_dim), \
            "d_emb must be f32 [%d, %d], got %s" % (n, self.emb_dim, tuple(getattr(d_emb, "shape", ())))
        assert d_emb.dtype == torch.float32 and d_emb.device == self.params.device and d_emb.is_contiguous(), \
            "d_emb must be a contiguous float32 tensor on %s" % (self.params.device,)
        if want_dx and not had_x:
            raise RuntimeError("no input gradient for a batch staged on the device (stage_crops): the forward took no fp32 x")
        self.materialize_grads()           # a pending lazy backward (of the fused step) completes the flat buffer first
        self._last = None                  # the fused backward() of the same forward would find its activations consumed
        pl.consumed = count
        into = self._grads
        data_only = discard and has(self.L, "vpd_plan_set_param_grads")
        if has(self.L, "vpd_plan_set_param_grads"):
            self._plan_flag(pl, "param_grads", "vpd_plan_set_param_grads", not data_only)
        if accumulate or (discard and not data_only):      # (data_only: `into` must be non-null but is not written)
            if self._grads2 is None:
                self._grads2 = torch.zeros_like(self._grads)
            into = self._grads2
        dx = None
        if want_dx and n > 0:
            dx = torch.empty((n, self.c_in, pl.h, pl.w), dtype=torch.float32, device=self.device)
            self.stem_dgrad_launches += 1
        elif want_dx:
            dx = torch.zeros((0, self.c_in, pl.h, pl.w), dtype=torch.float32, device=self.device)
        self.check(self.L.vpd_backward_ext(pl.handle, _ptr(self.params), _ptr(into), _ptr(d_emb), n,
                                           _ptr(dx) if n > 0 else None, None, _ptr(pl.workspace), self._stream()),
                   "vpd_backward_ext")
        if not discard:
            self._step_plan = pl
            if accumulate:
                self._grads.add_(self._grads2)
            self._grads_cleared = False
        return dx

    def unscale_grads_(self):
        """LossScaler.step() for an optimizer that reads p.grad: the flat gradient buffer (completed first) x 1 / loss scale."""
        if self.loss_scale != 1.0:
            self.materialize_grads()
            self._grads.mul_(1.0 / self.loss_scale)
            if self._step_plan is not None:
                self.check(self.L.vpd_plan_set_loss_scale(self._step_plan.handle, 1.0), "vpd_plan_set_loss_scale")
            self.loss_scale = 1.0

    @property
    def encoder_numel(self):
        """Elements of the flat buffers that belong to the encoder (a multiple of 4: the decoder's tensors follow)."""
        off = self.layout["decoder." + DECODER_PARAM_NAMES[0]][2]
        return (off + 3) & ~3

    def _adamw_fused(self, pl, numel, hyper, state):
        """vpd_plan_adamw_step through the plan of the last backward; state: the device block that decides, or None = the host step"""
        bufs = (pl.handle, _ptr(self.params), _ptr(self._grads), _ptr(self.adam_m), _ptr(self.adam_v), numel) + hyper
        if state is not None:
            self.check(self.L.vpd_plan_adamw_step_scaled(*bufs, _ptr(state), _ptr(pl.workspace), self._stream()),
                       "vpd_plan_adamw_step_scaled")
        else:
            self.check(self.L.vpd_plan_adamw_step(*bufs, self.adam_step, _ptr(pl.workspace), self._stream()), "vpd_plan_adamw_step")

    def _adamw_flat(self, numel, hyper, state):
        """... over the leading `numel` elements of the (completed) flat buffers"""
        bufs = (_ptr(self.params), _ptr(self._grads), _ptr(self.adam_m), _ptr(self.adam_v), numel) + hyper
        if state is not None:
            self.check(self.L.vpd_adamw_step_scaled(*bufs, _ptr(state), self._stream()), "vpd_adamw_step_scaled")
        else:
            self.check(self.L.vpd_adamw_step(*bufs, self.adam_step, self._stream()), "vpd_adamw_step")

    def _adam_group_table(self, groups, numel, pl):
        """the device segment table of `groups` over the leading `numel` elements: built on first use, rebuilt when the grouping
        (which tensor is in which group: groups['key']) or numel changes -- never because an lr moved.  pl: the plan of a fused
        step (the library then also checks that no boundary cuts a conv weight), or None"""
        key = (groups["key"], numel)
        if self._group_table_key != key:
            require(self.L, "vpd_plan_adamw_step_groups", "AdamW parameter groups")
            begin, group = groups["seg_begin"], groups["seg_group"]
            nseg = len(group)
            table = torch.zeros(max(int(self.L.vpd_adam_groups_bytes(nseg)) // 4, 1), dtype=torch.int32, device=self.device)
            self.check(self.L.vpd_adam_groups_init(None if pl is None else pl.handle, _ptr(table), (C.c_longlong * (nseg + 1))(*begin),
                                                   (C.c_int * nseg)(*group), nseg, numel, len(groups["lr"]), self._stream()),
                       "vpd_adam_groups_init")
            self._group_table, self._group_table_key = table, key
            self.group_table_builds += 1
        return self._group_table

    def _adamw_groups(self, pl, numel, groups, betas, eps, state):
        """the grouped step: vpd_plan_adamw_step_groups through `pl`, or (pl None) vpd_adamw_step_groups over the flat buffers"""
        n = len(groups["lr"])
        table = self._adam_group_table(groups, numel, pl)
        lr = (C.c_double * n)(*groups["lr"])
        wd = (C.c_double * n)(*groups["weight_decay"])
        step = 1 if state is not None else self.adam_step      # (ignored behind a device block)
        bufs = (_ptr(self.params), _ptr(self._grads), _ptr(self.adam_m), _ptr(self.adam_v), numel, _ptr(table), lr, wd, n,
                betas[0], betas[1], eps, step)
        if pl is not None:
            self.check(self.L.vpd_plan_adamw_step_groups(pl.handle, *bufs, _ptr(state), _ptr(pl.workspace), self._stream()),
                       "vpd_plan_adamw_step_groups")
        else:      # (the loss scale is out of the buffer already: unscale_grads_, or the device block takes it out)
            self.check(self.L.vpd_adamw_step_groups(*bufs, 1.0, _ptr(state), self._stream()), "vpd_adamw_step_groups")

    def adamw_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, numel=None, groups=None):
        """numel: leading elements of the flat buffers to update (default: all).  An optimizer built without the motion head's
        parameters passes encoder_numel, as torch.optim.AdamW never touches tensors it was not given.

        groups: None -- one (lr, weight_decay) for every element, the launches of always -- or torch.optim.AdamW's parameter
        groups as FusedAdamW states them: {'lr': [..], 'weight_decay': [..] (one entry per group, at most 16; `lr` and
        `weight_decay` above are then not read), 'seg_begin': [0, .., numel], 'seg_group': [..] (element ranges of the flat
        buffers and their groups, same-group neighbours merged), 'key': hashable, changes with the grouping}.  The same two paths
        (fused through the last backward's plan -- only when numel is exactly the plan's --, else flat), the same search / norm
        pass / EMA around them.  A group with lr = 0 and weight_decay = 0 keeps its parameters bit for bit (p * 1.0f is exact,
        fma(-0, m / den, p) = p as den >= eps > 0); its moments still move, as torch's do.  Clipping takes the norm of ALL
        gradients, which is what clip_grad_norm_ over all the optimizer's parameters gives."""
        numel = self.param_numel if numel is None else int(numel)
        self.fold_accumulated_grads()      # (an accumulation window's sum first: nothing is launched when none is held)
        if self.adam_m is None:
            self.adam_m = torch.zeros_like(self.params)
            self.adam_v = torch.zeros_like(self.params)
        st = self.scale_state      # a DynamicLossScaler's step in flight: search + AdamW decided on the device, no host count
        clip = self._clip          # enable_grad_clip(): the norm pass (instead of the search) + AdamW reading the clip block
        state = clip if clip is not None else st      # the device block AdamW and the EMA read (None: the host's step count)
        if state is None:
            self._steps.set(self._steps.get() + 1)      # (the host counts; behind a block the device does)
        # the train plan of the last backward: AdamW + refresh of its packed bf16 weights in one pass.  Not for an optimizer that
        # was NOT given the motion head, behind a plan that trains it: the fused pass would update the head's tensors too
        # (torch.optim.AdamW never touches tensors it was not given) -- plain flat update of the leading `numel` elements
        # instead; the plan repacks its bf16 weights before its next forward
        pl = self._step_plan
        fused = (pl is not None and numel >= pl.param_numel and pl.packed_version == self.weights_version()
                 and os.environ.get("VPD_FUSED_ADAMW", "1") != "0")
        if groups is not None and fused and numel != pl.param_numel:
            fused = False      # (tensors beyond the plan's: the grouped fused entry has no flat tail; flat, and the plan repacks)
        if not fused:
            pl = None
            self.materialize_grads()
            if state is None:
                self.unscale_grads_()      # (the flat kernel has no plan to ask for the loss scale; through a device block the
                                           #  kernel takes it out, and the buffer stays as the backward left it)
        if clip is not None:
            self._clip_norm(pl, numel, st)
        elif st is not None and fused:
            self.check(self.L.vpd_plan_check_grads(pl.handle, _ptr(self._grads), numel, _ptr(st), _ptr(pl.workspace),
                                                   self._stream()), "vpd_plan_check_grads")
        elif st is not None:
            self.check(self.L.vpd_op_check_finite(_ptr(self._grads), numel, _ptr(st), self._stream()), "vpd_op_check_finite")
        hyper = (lr, betas[0], betas[1], eps, weight_decay)
        if groups is not None:
            self._adamw_groups(pl, numel, groups, betas, eps, state)
        elif fused:
            self._adamw_fused(pl, numel, hyper, state)
        else:
            self._adamw_flat(numel, hyper, state)
        self._hip_version += 1
        if fused:
            pl.packed_version = self.weights_version()
        if self._ema is not None:
            # after the AdamW, before the scaler's update(): `found` and `applied_steps` are still those of this step
            self._ema_enqueue(state)
        if clip is not None and st is None:
            # no scaler's update() follows: the clip block counts its own steps (applied, or skipped on a non-finite norm)
            self.scale_state_update(clip, 1.0, 1.0, 2 ** 31 - 1)

    def capture_eval_graph(self, x, out):
        """hipGraph of the eval forward for this batch size, bound to x / out (capture needs a
        non-default stream; the graph itself is launched on the current stream)."""
        return self._capture_eval_graph(x, None, out)

    def capture_eval_graph_staged(self, n, img_dim, out):
        """hipGraph of the eval forward for n crops whose input is ALREADY in the plan's stem staging buffer (stage_crops /
        CropAugmenter.stage_views): the graph starts at the stem convolution."""
        return self._capture_eval_graph(None, (n, img_dim), out)

    def _capture_eval_graph(self, x, staged, out):
        self._no_graph_under_ema()
        n, h, w = self._batch_shape(x, staged)
        pl = self.plan(h, w, n, False, False)
        self._ensure_packed(pl)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        self.check(self.L.vpd_graph_capture_eval(pl.handle, _ptr(self.params), _ptr(x), n, _ptr(out), _ptr(pl.workspace),
                                           C.c_void_p(side.cuda_stream)), "vpd_graph_capture_eval")
        torch.cuda.current_stream(self.device).wait_stream(side)
        pl.graph_sizes.add(n)
        return pl

    def _no_graph_under_ema(self):
        if self._use_ema:
            raise RuntimeError("eval graphs are bound to the live parameter buffer: not available while use_ema() is on "
                               "(load ema_state_dict() into a student of its own to serve the averaged weights)")

    def sync_errors(self):
        """Grid-barrier time-outs counted by the train plans since their workspaces were initialised (host sync).
        Non-zero = a fused BatchNorm launch gave up waiting for its grid: results are not to be trusted."""
        total = 0
        out = C.c_uint(0)
        for pl in self._plans.values():
            if pl.train and pl.handle:
                self.check(self.L.vpd_plan_sync_errors(pl.handle, _ptr(pl.workspace), self._stream(), C.byref(out)),
                      "vpd_plan_sync_errors")
                total += out.value
        return total

    def set_timing(self, pl, enable):
        self.check(self.L.vpd_plan_set_timing(pl.handle, int(enable)), "vpd_plan_set_timing")

    def read_timing(self, pl):
        out = (C.c_double * 24)()
        self.check(self.L.vpd_plan_read_timing(pl.handle, out, 8), "vpd_plan_read_timing")
        # (class 1 -> conv3x3_pws_kernel<256,128,352> only with > 1 tile per block, else the class-6 tile; the non-persistent
        #  conv3x3_ws_kernel twins of every class remain behind VPD_PWS=0)
        names = ["conv3x3_c64_persistent_kernel<224>", "conv3x3_pws_kernel<256,128,352>", "conv3x3_pws_kernel<256,64,416> | <128,128,288>",
                 "conv3x3_pws_kernel<128,64,288>", "conv1x1_ws_kernel (stride-2 / 1x1 ring GEMM) + conv1x1_stream_kernel (Bottleneck 1x1, streaming / recompute) + conv_igemm_kernel (gather)", "conv_wgrad128_persistent_kernel (layer2-4) + conv_wgrad_halo_grouped_kernel (layer1)",
                 "conv_wgrad_halo_kernel<10|13> (stride 2) + conv_wgrad_kernel (1x1)",
                 "conv_stem_persistent_kernel<160> + conv_wgrad_stem_kernel"]
        return {names[i]: dict(launches=out[3 * i], ms=out[3 * i + 1], flops=out[3 * i + 2]) for i in range(8)}

    def launch_eval_graph(self, pl, n):
        self._no_graph_under_ema()
        self._ensure_packed(pl)
        self.check(self.L.vpd_graph_launch_eval(pl.handle, n, self._stream()), "vpd_graph_launch_eval")
