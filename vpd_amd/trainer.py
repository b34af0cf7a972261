"""ModelTrainer: the reference's training driver (train_vpd_model.py:53-112)
on the HIP engine.  Same methods, same epoch() return value (sum of per-batch
sum-MSE / number of crops), same checkpoint files."""
import contextlib
import os

import torch

from . import checkpoint as ckpt
from .ddp import GradBucketReducer
from .models.module import FCNet
from .models.util import DynamicLossScaler, LossScaler, step


class _Loss:
    """What `F.mse_loss(...)` returns in the reference loop, for the fused path:
    supports .backward() (models/util.py:52) and .item() (train_vpd_model.py:93)."""

    def __init__(self, trainer):
        self._t = trainer

    def backward(self):
        self._t._backward()

    def backward_for_step(self):
        """backward() as models.util.step() runs it: the optimizer step follows immediately and nothing reads .grad in
        between (reference models/util.py:52-58), so the conv weight gradients may stay in the kernels' layout."""
        self._t._backward(lazy=True)

    def backward_for_accumulation(self, lazy=False):
        """A non-final micro-batch of models.util.step(..., accumulate=True): the backward (no collective under data parallelism),
        then the live gradients go into the engine's accumulator."""
        self._t._backward(lazy=lazy, final=False)
        self._t.encoder.engine.accumulate_grads()

    def item(self):
        return float(self._t.encoder.engine.loss_step.item())   # host sync, as in the reference


MAX_PARAM_GROUPS = 16      # VPD_MAX_PARAM_GROUPS of the library


def accumulation_schedule(batches, accum_steps):
    """(batch, step_now) for every batch of `batches`: step_now on every accum_steps-th batch and on the LAST one, found with a
    one-item look-ahead (a loader need not know its length), so that no gradient crosses an epoch boundary and none is dropped.
    accum_steps = 1: every batch steps.  A pure function of the iterable."""
    k = int(accum_steps)
    if k < 1:
        raise ValueError("accum_steps must be >= 1, not %r" % (accum_steps,))
    it = iter(batches)
    try:
        cur = next(it)
    except StopIteration:
        return
    i = 0
    for nxt in it:
        i += 1
        yield cur, i % k == 0
        cur = nxt
    yield cur, True


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW(params, lr) with torch defaults (train_vpd_model.py:104) as ONE HIP kernel over the engine's flat fp32
    buffers.  `params` is what torch takes: the tensors (one group, weight decay on every tensor), or a list of dicts --
    parameter groups, at most 16, each with its own 'lr' and 'weight_decay'; `betas` and `eps` must be the same in all (ValueError
    otherwise, here and at step()).  Every entry of `param_groups` is read at every step(), so torch.optim.lr_scheduler and
    add_param_group work.  With more than one group every tensor of the engine must be in exactly one (the motion head may be
    absent altogether): a tensor is held still with a group of lr=0, weight_decay=0 -- its parameters then keep every bit
    (p * 1.0f is exact, fma(-0, m / den, p) = p), its moments still move, as torch's do.  Clipping (max_grad_norm) takes the norm of
    all gradients, as clip_grad_norm_ over all the optimizer's parameters does; EMA and data parallelism need nothing new."""

    consumes_lazy_grads = True      # models.util.step(): this optimizer reads the weight-gradient kernels' own layout

    def __init__(self, params, engine, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=None):
        """max_grad_norm: torch.nn.utils.clip_grad_norm_(params, max_grad_norm) before every step, decided on the device over
        exactly the gradients the step reads (StudentEngine.enable_grad_clip); None (the default): nothing is added."""
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be > 0 (float('inf') measures only), not %r" % (max_grad_norm,))
        params = list(params)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._engine = engine
        self._grouping = None           # (membership signature, the `groups` description without lr / weight_decay)
        self._shared_hypers()
        # like torch.optim.AdamW, touch only the tensors that were passed in: without the motion head's parameters the
        # update stops where the encoder's tensors end in the flat buffers
        self._name_at = None            # flat offset -> layout name (first use: the layout never changes)
        enc_end = engine.encoder_numel
        self._has_dec = any(self._offset(q) >= enc_end for g in self.param_groups for q in g["params"])
        self._numel = engine.param_numel if self._has_dec else enc_end
        if len(self.param_groups) > 1:
            self._groups()              # (a missing tensor or too many groups: refused here, not at the first step)
        if max_grad_norm is not None:
            engine.enable_grad_clip(max_grad_norm)

    def clip_stats(self, reset_max=False):
        """{'total_norm', 'norm_max', 'coef', 'clipped_steps', 'nonfinite_steps'} of the clip block; synchronises, as
        DynamicLossScaler.get_scale() does"""
        return self._engine.clip_stats(reset_max)

    def _offset(self, q):
        """where a parameter begins in the engine's flat buffers"""
        return (q.data_ptr() - self._engine.params.data_ptr()) // 4

    def _locate(self, q):
        """(_offset, layout name -- None for a tensor that is not one of the engine's) of a parameter"""
        if self._name_at is None:
            self._name_at = {row[2]: name for name, row in self._engine.layout.items()}      # (row: kind, is_dec, offset, ...)
        off = self._offset(q)
        return off, self._name_at.get(off)

    def _shared_hypers(self):
        """(betas, eps) of every group: the kernels share them"""
        g0 = self.param_groups[0]
        betas, eps = tuple(g0["betas"]), g0["eps"]
        for i, g in enumerate(self.param_groups[1:], start=1):
            if tuple(g["betas"]) != betas or g["eps"] != eps:
                raise ValueError("FusedAdamW: betas and eps must be the same in every parameter group (group %d has betas=%r, eps=%r, "
                                 "group 0 betas=%r, eps=%r); only lr and weight_decay are per group" % (i, g["betas"], g["eps"], betas, eps))
        return betas, eps

    def _groups(self):
        """The engine's `groups` description of param_groups (StudentEngine.adamw_step) with this step's lr / weight_decay.  The
        segments -- every tensor's offset from its data_ptr, sorted, same-group neighbours merged; padding floats belong to the
        segment in front of them -- are rebuilt only when the membership changes (add_param_group), never for an lr."""
        pgs = self.param_groups
        if len(pgs) > MAX_PARAM_GROUPS:
            raise ValueError("FusedAdamW: %d parameter groups, at most %d" % (len(pgs), MAX_PARAM_GROUPS))
        sig = tuple(tuple(id(q) for q in g["params"]) for g in pgs)
        if self._grouping is None or self._grouping[0] != sig:
            where = [(gi,) + self._locate(q) for gi, g in enumerate(pgs) for q in g["params"]]
            rows = [(name, row[2]) for name, row in self._engine.layout.items() if self._has_dec or not row[1]]
            known = {name for name, _ in rows}
            if any(name not in known for _, _, name in where):
                raise ValueError("FusedAdamW: a parameter that is not one of the engine's tensors")
            group_of = {off: gi for gi, off, _ in where}
            missing = [name for name, off in rows if off not in group_of]
            if missing:
                raise ValueError("FusedAdamW: with parameter groups every tensor must be in exactly one group; missing: %s%s.  A tensor is "
                                 "held still with a group of lr=0, weight_decay=0"
                                 % (", ".join(missing[:4]), " ... (%d in all)" % len(missing) if len(missing) > 4 else ""))
            begin, group = [], []
            for _, off in sorted(rows, key=lambda r: r[1]):
                if not group or group[-1] != group_of[off]:
                    begin.append(off if group else 0)
                    group.append(group_of[off])
            begin.append(self._numel)
            self._grouping = (sig, dict(seg_begin=begin, seg_group=group, key=(tuple(begin), tuple(group), len(pgs))))
        return dict(self._grouping[1], lr=[float(g["lr"]) for g in pgs], weight_decay=[float(g["weight_decay"]) for g in pgs])

    @torch.no_grad()
    def step(self, closure=None):
        g = self.param_groups[0]
        if len(self.param_groups) == 1:      # one group: the launches of always
            self._engine.adamw_step(g["lr"], g["betas"], g["eps"], g["weight_decay"], numel=self._numel)
            return
        betas, eps = self._shared_hypers()
        self._engine.adamw_step(g["lr"], betas, eps, g["weight_decay"], numel=self._numel, groups=self._groups())

    def _names(self):
        """the layout names of the parameters, in the optimizer's own order (the indices of state_dict())"""
        names = [self._locate(q)[1] for g in self.param_groups for q in g["params"]]
        if None in names:
            raise ValueError("FusedAdamW: a parameter that is not one of the engine's tensors")
        return names

    def state_dict(self):
        """torch.optim.AdamW.state_dict() of the engine's flat moments (vpd_amd.checkpoint.adamw_state_dict): `state` is empty
        before the first step, afterwards every parameter has `step` (engine.adam_step: read from the device block when one holds
        the count -- synchronises), `exp_avg` and `exp_avg_sq`, views of engine.adam_m / adam_v.  torch.optim.AdamW over the same
        parameters loads it."""
        eng = self._engine
        step = int(eng.adam_step) if eng.adam_m is not None else 0
        return ckpt.adamw_state_dict(eng.layout, eng.adam_m, eng.adam_v, step, self._names(), self.param_groups)

    def load_state_dict(self, state_dict):
        """The inverse, also for a dictionary of torch.optim.AdamW over the same parameters in the same order: the moments go into
        engine.adam_m / adam_v (allocated when need be), the step into engine.adam_step -- through its setter, so the device block
        of a DynamicLossScaler or of the clipping receives it: load the optimizer BEFORE the scaler, the EMA and the clip state --
        and every group's lr, betas, eps and weight_decay are restored, as torch does.  Everything is checked before anything is
        written (ValueError: group structure, steps that differ, a missing parameter, a shape, betas / eps that differ)."""
        eng = self._engine
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups):
            raise ValueError("FusedAdamW: the dictionary has %d parameter groups, this optimizer %d" % (len(groups), len(self.param_groups)))
        for i, (g, ng) in enumerate(zip(self.param_groups, groups)):
            if len(g["params"]) != len(ng["params"]):
                raise ValueError("FusedAdamW: group %d holds %d parameters in the dictionary, %d here" % (i, len(ng["params"]), len(g["params"])))
            if ng.get("amsgrad") or ng.get("maximize"):
                raise ValueError("FusedAdamW: amsgrad / maximize are not implemented (group %d of the dictionary asks for one)" % i)
        allocated = eng.adam_m is None
        if allocated:
            eng.adam_m = torch.zeros_like(eng.params)
            eng.adam_v = torch.zeros_like(eng.params)
        try:
            step = ckpt.adamw_load_flat(state_dict, eng.layout, self._names(), eng.adam_m, eng.adam_v)
        except Exception:
            if allocated:
                eng.adam_m = eng.adam_v = None
            raise
        eng.adam_step = step
        for g, ng in zip(self.param_groups, groups):
            g["lr"], g["weight_decay"] = ng["lr"], ng["weight_decay"]
            g["betas"], g["eps"] = tuple(ng["betas"]), ng["eps"]
        self._grouping = None

    def zero_grad(self, set_to_none=False):
        # gradients live in the engine's flat buffer and are overwritten (not accumulated) by the next fused backward, which is
        # what zero_grad-after-every-step amounts to: no memory is touched.  The autograd path (RGBF_EmbeddingModel.forward)
        # accumulates as torch does: it is told here that the buffer counts as cleared
        self._engine.mark_grads_cleared()
        self._engine.drop_accumulated_grads()      # the accumulation window is over (after a step the fold emptied it already)
        return None


class ModelTrainer:
    """Class for training the encoder. Discarded after training"""

    accum_steps = 1

    def __init__(self, encoder, motion, process_group=None, augmenter=None, augment=True, ema_decay=None, ema_warmup=False,
                 accum_steps=1):
        """accum_steps: K >= 1 micro-batches per optimizer step (gradient accumulation).  epoch() steps on every K-th batch and on
        the last batch of the loader; in between the gradients are summed in the engine's accumulator (no 1/K: the loss is a sum
        over crops), BatchNorm statistics are per micro-batch, a loss scale stays fixed across the window, and under data
        parallelism only the window's last backward all-reduces.  1 (the default) is the step of always.

        ema_decay: keep an exponential moving average of the weights (and of the BatchNorm running statistics) with this
        decay; ema_warmup: timm's rule min(decay, (1 + t) / (10 + t)).  Averaging starts in get_optimizer() -- from the weights as
        they stand then, i.e. after a checkpoint was loaded -- and every fused optimizer step ends with one more launch
        (StudentEngine.enable_ema).  ema_weights() evaluates with the average, save_model(..., ema=True) writes it.  Under data
        parallelism every rank averages its own (identical) parameters: no collective is added.

        augmenter: a vpd_amd.augment.CropAugmenter -> epoch() also accepts RAW batches
        {'rgb_u8': u8[B,H,W,3], 'flow_u8': u8[B,H,W,2], 'mask_u8': u8[B,H,W] (optional), 'flip': int[B] (optional,
        decided by the dataset because it selects the teacher row), 'emb'} and runs the reference's per-item
        transforms (vpd_dataset/single_frame.py:168-206) on the device, straight into the stem's staging buffer."""
        device = encoder.device
        self.augmenter, self.augment = augmenter, bool(augment)
        self.encoder = encoder.to(device)
        self.motion = bool(motion)
        if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError("ema_decay must be in [0, 1], not %r" % (ema_decay,))
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        if int(accum_steps) != accum_steps or int(accum_steps) < 1:
            raise ValueError("accum_steps must be an integer >= 1, not %r" % (accum_steps,))
        self.accum_steps = int(accum_steps)
        if motion:
            self.fcn_time = FCNet(encoder.engine, encoder.emb_dim, [128, 128], 2 * encoder.emb_dim, dropout=0)
        self._reducer = None
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()
                                         and torch.distributed.get_world_size() > 1):
            self._reducer = GradBucketReducer(encoder.engine, process_group)

    # -- pieces of the reference loop body (train_vpd_model.py:79-91) -------------------
    def _forward_loss(self, img, gt_emb, train):
        eng = self.encoder.engine
        img = img.to(eng.device, dtype=torch.float32, non_blocking=True).contiguous()
        gt = gt_emb.to(eng.device, dtype=torch.float32, non_blocking=True).contiguous()
        if train:
            eng.forward_train(img, gt, motion=self.motion)
        else:
            eng.forward_eval(img, gt, motion=self.motion)
        return _Loss(self)

    def _forward_loss_raw(self, batch, train):
        from .augment import sample_params
        if self.augmenter is None:
            raise RuntimeError("raw u8 batches need ModelTrainer(..., augmenter=CropAugmenter(...))")
        eng = self.encoder.engine
        dev = lambda t: None if t is None else t.to(eng.device, non_blocking=True).contiguous()
        rgb = dev(batch['rgb_u8'])
        n, h, w, _ = rgb.shape
        # like the reference validation batches are augmented too: augmentation is a property
        # of the dataset objects, which are all built with augment=True (vpd_dataset/single_frame.py:267-272)
        # seed=None: a fresh Philox key for the device-side mask noise of THIS batch (drawn from torch's global RNG)
        params = sample_params(n, h, w, augment=self.augment, flip=False)
        self.last_aug_params = params
        if 'flip' in batch:
            params['flip'] = batch['flip'].numpy() if hasattr(batch['flip'], 'numpy') else batch['flip']
        staged = self.augmenter.stage(eng, rgb, dev(batch.get('flow_u8')), dev(batch.get('mask_u8')), params,
                                      train=train, motion=self.motion)
        gt = batch['emb'].to(eng.device, dtype=torch.float32, non_blocking=True).contiguous()
        if train:
            eng.forward_train(None, gt, motion=self.motion, staged=staged)
        else:
            eng.forward_eval(None, gt, motion=self.motion, staged=staged)
        return _Loss(self)

    def _backward(self, lazy=False, final=True):
        """final=False: a non-final micro-batch of an accumulation window -- under data parallelism the backward records no bucket
        events and starts no collective (the window's last backward reduces the folded sum: 1/K of the all-reduces)"""
        eng = self.encoder.engine
        if self._reducer is not None and not final:
            lazy = lazy and os.environ.get("VPD_DDP_LAZY", "1") != "0"      # (one layout per window: the final backward's rule)
            eng.backward(lazy=lazy)
        elif self._reducer is not None:
            nb = eng.pending_forward_buckets()      # (0 without a forward: backward() raises)
            # lazy gradients stay on under data parallelism: a SUM all-reduce is layout-agnostic, so the reducer sums the
            # weight-gradient scratch ranges + the small tensors of the flat buffer (VPD_DDP_LAZY=0: flat buffer, eager unpack)
            lazy = lazy and os.environ.get("VPD_DDP_LAZY", "1") != "0"
            pl = eng.backward(self._reducer.event_handles(nb), lazy=lazy)
            self._reducer.reduce(pl, lazy=lazy)
        else:
            eng.backward(lazy=lazy)
        if not lazy:
            self._reattach_grads()

    def _reattach_grads(self):
        """A torch optimizer's zero_grad() drops .grad (set_to_none=True is torch's default): every plain backward() makes
        sure the parameters' .grad are the views of the engine's flat gradient buffer again."""
        eng = self.encoder.engine
        first = next(iter(self.encoder.parameters()))
        if first.grad is not None and (not hasattr(self, 'fcn_time') or next(iter(self.fcn_time.parameters())).grad is not None):
            return
        g = eng.grads
        for k in eng.enc_names:
            self.encoder.get_parameter(k).grad = eng.view(k, g)
        if hasattr(self, 'fcn_time'):
            from .models.module import DECODER_PARAM_NAMES
            for k in DECODER_PARAM_NAMES:
                self.fcn_time.get_parameter(k).grad = eng.view("decoder." + k, g)

    def epoch(self, data_loader, optimizer=None, scaler=None, progress_cb=None):
        eng = self.encoder.engine
        self.encoder.eval() if optimizer is None else self.encoder.train()
        if hasattr(self, 'fcn_time'):
            self.fcn_time.eval() if optimizer is None else self.fcn_time.train()

        eng.loss_accum.zero_()          # the epoch accumulator of train_vpd_model.py:73,93 lives on device
        if optimizer is not None:
            # every train epoch ends with a step, so nothing is held here unless a window was abandoned (an exception in the
            # middle of an epoch, accumulate=True by hand without a final step): its sum must not leak into this epoch's first window
            eng.drop_accumulated_grads()
        epoch_emb_n = 0
        for batch, step_now in accumulation_schedule(data_loader, self.accum_steps if optimizer is not None else 1):
            if 'rgb_u8' in batch:
                n = batch['rgb_u8'].shape[0]
                loss = self._forward_loss_raw(batch, train=optimizer is not None)
            else:
                n = batch['img'].shape[0]
                loss = self._forward_loss(batch['img'], batch['emb'], train=optimizer is not None)
            if optimizer is not None:
                step(optimizer, scaler, loss, accumulate=not step_now)
            epoch_emb_n += n
            if progress_cb is not None:
                progress_cb(n)
        epoch_emb_loss = float(eng.loss_accum.item())   # ONE host sync per epoch
        if optimizer is not None and eng.sync_errors():
            raise RuntimeError("a fused BatchNorm launch timed out at its in-launch grid barrier (the grid was not "
                               "resident): this epoch's results are invalid; set VPD_FUSED_BN=0 to use separate launches")
        # (a DynamicLossScaler skipped the steps whose gradients overflowed: like the reference, the epoch value is reported as it is)
        if optimizer is not None and scaler is not None and not isinstance(scaler, DynamicLossScaler) \
                and epoch_emb_loss != epoch_emb_loss:
            raise FloatingPointError("non-finite training loss under fp16 with loss scale %g: an activation gradient left fp16's range "
                                     "(the reference's GradScaler would have skipped those steps); use LossScaler(engine, init_scale=<smaller>) or get_optimizer(lr, loss_scale='dynamic')"
                                     % scaler.get_scale())
        if self._reducer is not None:
            epoch_emb_loss, epoch_emb_n = self._reducer.all_reduce_scalars(epoch_emb_loss, epoch_emb_n)
        return epoch_emb_loss / epoch_emb_n

    def param_groups(self, weight_decay=0.01, decay_bn_bias=True, backbone_lr_scale=1.0, lr=None):
        """torch-style parameter groups for get_optimizer(..., param_groups=...): the usual fine-tuning split.  The head is `fc.*`
        plus the motion head, the backbone everything else; BatchNorm weights, BatchNorm biases and linear biases (kinds 1, 2, 4 of
        vpd_plan_tensor_info) get weight_decay 0 unless decay_bn_bias; the backbone runs at backbone_lr_scale * lr (which then
        must be given), the head at the optimizer's lr.  Empty groups are left out: the defaults give ONE group, i.e. the step of
        always."""
        eng = self.encoder.engine
        if backbone_lr_scale != 1.0 and lr is None:
            raise ValueError("param_groups(backbone_lr_scale=%r) needs lr" % (backbone_lr_scale,))
        named = [(k, self.encoder.get_parameter(k)) for k in eng.enc_names]
        if hasattr(self, 'fcn_time'):
            from .models.module import DECODER_PARAM_NAMES
            named += [("decoder." + k, self.fcn_time.get_parameter(k)) for k in DECODER_PARAM_NAMES]
        buckets = {}      # (head, decays) -> tensors, in layout order
        for name, q in named:
            head = name.startswith("resnet.fc.") or name.startswith("decoder.")
            decays = decay_bn_bias or eng.layout[name][0] not in (1, 2, 4)
            buckets.setdefault((head and backbone_lr_scale != 1.0, decays), []).append(q)
        out = []
        for (head, decays), tensors in sorted(buckets.items(), key=lambda kv: (kv[0][0], not kv[0][1])):
            g = dict(params=tensors, weight_decay=float(weight_decay) if decays else 0.0)
            if lr is not None:
                g["lr"] = float(lr) * (1.0 if head or backbone_lr_scale == 1.0 else float(backbone_lr_scale))
            out.append(g)
        return out

    def get_optimizer(self, learning_rate, loss_scale=None, max_grad_norm=None, param_groups=None):
        """param_groups: None -- one group over every tensor, torch's defaults -- or a torch-style list of dicts (param_groups()
        above, or any other: FusedAdamW) whose entries without 'lr' run at learning_rate.
        max_grad_norm: clip the global gradient norm before every step (FusedAdamW); None: no clipping, nothing added.
        loss_scale: None -- the default scaler of the student's element type (bf16: none; fp16: the static LossScaler, 256);
        'dynamic' -- a DynamicLossScaler (GradScaler's defaults: skip on overflow, decided on the device); a number -- a static
        LossScaler with that scale.  A scaler is an fp16 matter: asking for one on a bf16 student raises."""
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be > 0 (float('inf') measures only), not %r" % (max_grad_norm,))
        params = list(self.encoder.parameters())
        if hasattr(self, 'fcn_time'):
            params.extend(self.fcn_time.parameters())
        # bf16 operands with fp32 accumulation need no GradScaler: scaler None.  A student built with dtype="fp16" gets the static
        # LossScaler (the reference: GradScaler() on 'cuda', train_vpd_model.py:104-105)
        eng = self.encoder.engine
        if self.ema_decay is not None and not eng.ema_enabled:
            eng.enable_ema(self.ema_decay, self.ema_warmup)      # (before a DynamicLossScaler takes the step count to the device)
        if loss_scale is None:
            scaler = LossScaler(eng) if eng.dtype == "fp16" else None
        elif eng.dtype != "fp16":
            raise ValueError("loss_scale=%r: loss scaling belongs to a student built with dtype='fp16' (this one: %s)"
                             % (loss_scale, eng.dtype))
        elif isinstance(loss_scale, str):
            if loss_scale != "dynamic":
                raise ValueError("loss_scale must be None, 'dynamic' or a number, not %r" % (loss_scale,))
            scaler = DynamicLossScaler(eng)
        else:
            scaler = LossScaler(eng, float(loss_scale))
        if param_groups is not None:
            params = list(param_groups)
        eng.drop_accumulated_grads()      # a new optimizer begins a new accumulation window (an abandoned one is forgotten)
        return FusedAdamW(params, eng, lr=learning_rate, max_grad_norm=max_grad_norm), scaler

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context every eval forward (embed(), epoch() without an optimizer) computes with the averaged weights; the
        live ones are back on exit, untouched.  Train-mode forwards refuse to run inside."""
        eng = self.encoder.engine
        eng.use_ema(True)
        try:
            yield self
        finally:
            eng.use_ema(False)

    # -- resumable training ---------------------------------------------------------------------------------------------
    def _fingerprint(self):
        eng = self.encoder.engine
        return ckpt.fingerprint(eng.arch, eng.c_in, eng.emb_dim, self.motion, eng.dtype, eng.param_numel)

    @staticmethod
    def _scaler_kind(scaler):
        return "none" if scaler is None else "dynamic" if isinstance(scaler, DynamicLossScaler) else "static"

    def _rank_world(self):
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return dist.get_rank(), dist.get_world_size()
        return 0, 1

    def save_state(self, path, optimizer, scaler, extra=None):
        """Everything the next optimizer step depends on, in one file written atomically (vpd_amd.checkpoint.write_atomic; it loads
        with torch.load(path, weights_only=True)): the fingerprint (arch, input channels, emb_dim, motion, dtype, param_numel,
        format version), the encoder's and the motion head's state_dicts (num_batches_tracked included), the optimizer's and the
        scaler's dictionaries, the EMA and the clip state when enabled, bn_frozen, accum_steps, every rank's random number
        generators, and `extra` (the caller's bookkeeping: tensors, numbers, strings, lists, dicts).  Under data parallelism every
        rank calls it (the generator states are gathered), rank 0 writes.  Raises in the middle of an accumulation window (a
        partial sum is nothing to resume from), inside ema_weights(), and for an optimizer that is not this engine's FusedAdamW."""
        eng = self.encoder.engine
        if not isinstance(optimizer, FusedAdamW) or optimizer._engine is not eng:
            raise TypeError("save_state() takes the FusedAdamW of this trainer's engine (get_optimizer), not %s" % type(optimizer).__name__)
        if eng.held_micro_batches != 0:
            raise RuntimeError("save_state() in the middle of an accumulation window (%d micro-batch(es) held): save at a window "
                               "boundary, after the optimizer step" % eng.held_micro_batches)
        if eng.ema_in_use:
            raise RuntimeError("save_state() inside ema_weights(): leave the context first")
        if scaler is not None and not isinstance(scaler, LossScaler):
            raise TypeError("save_state() takes scaler=None or a vpd_amd.models.util.LossScaler, not %s" % type(scaler).__name__)
        rank, world = self._rank_world()
        state = {
            "fingerprint": self._fingerprint(),
            "encoder": dict(self.encoder.state_dict()),
            "decoder": dict(self.fcn_time.state_dict()) if hasattr(self, "fcn_time") else None,
            "optimizer": optimizer.state_dict(),
            "scaler_kind": self._scaler_kind(scaler),
            "scaler": None if scaler is None else scaler.state_dict(),
            "ema": eng.ema_state() if eng.ema_enabled else None,
            "clip": eng.clip_state() if eng.grad_clip_enabled else None,
            "bn_frozen": bool(eng.bn_frozen), "accum_steps": int(self.accum_steps),
            "rng": ckpt.gather_rng(rank, world), "world_size": world,
            "extra": extra,
        }
        if rank == 0:
            ckpt.write_atomic(state, path)

    def load_state(self, path, optimizer, scaler, state=None):
        """Restore what save_state() wrote into a trainer, optimizer and scaler built as the saving run built them, and return
        `extra`.  The order matters and is fixed here: weights, then the optimizer (its step goes to the device blocks), the
        scaler, the EMA (its count is relative to the step), the clip block, the generators.  Everything is compared before
        anything is written: a file from another arch / input / emb_dim / motion / dtype (ValueError naming the field), the EMA
        on one side only or with another decay / warmup, clipping on one side only or with another max_norm, another kind of
        scaler, another number of parameter groups, another world size.  state: the file's content when the caller has read it
        already (vpd_amd.checkpoint.read_state)."""
        eng = self.encoder.engine
        if not isinstance(optimizer, FusedAdamW) or optimizer._engine is not eng:
            raise TypeError("load_state() takes the FusedAdamW of this trainer's engine (get_optimizer), not %s" % type(optimizer).__name__)
        if state is None:
            state = ckpt.read_state(path)
        ckpt.check_fingerprint(state["fingerprint"], self._fingerprint())
        ema, clip = state["ema"], state["clip"]
        if (ema is not None) != eng.ema_enabled:
            raise ValueError("EMA: the file %s an average, this trainer %s (ModelTrainer(ema_decay=))"
                             % (("holds", "keeps none") if ema is not None else ("holds no", "keeps one")))
        if ema is not None and (float(ema["decay"]), bool(ema["warmup"])) != eng.ema_config:
            raise ValueError("EMA: the file's average has decay=%r, warmup=%r, this trainer decay=%r, warmup=%r"
                             % ((float(ema["decay"]), bool(ema["warmup"])) + eng.ema_config))
        if (clip is not None) != eng.grad_clip_enabled:
            raise ValueError("gradient clipping: %s in the file, %s in this optimizer (max_grad_norm=)"
                             % (("on", "off") if clip is not None else ("off", "on")))
        if clip is not None and float(clip["max_norm"]) != eng.clip_max_norm:
            raise ValueError("gradient clipping: max_norm %r in the file, %r in this optimizer" % (float(clip["max_norm"]), eng.clip_max_norm))
        if state["scaler_kind"] != self._scaler_kind(scaler):
            raise ValueError("loss scaler: the file was written with %s, this run has %s" % (state["scaler_kind"], self._scaler_kind(scaler)))
        if len(state["optimizer"]["param_groups"]) != len(optimizer.param_groups):
            raise ValueError("parameter groups: %d in the file, %d in this optimizer"
                             % (len(state["optimizer"]["param_groups"]), len(optimizer.param_groups)))
        rank, world = self._rank_world()
        rng = ckpt.pick_rng(state["rng"], rank, world)
        self.encoder.load_state_dict(state["encoder"])
        if hasattr(self, "fcn_time"):
            self.fcn_time.load_state_dict(state["decoder"])
        eng.mark_weights_changed()
        optimizer.load_state_dict(state["optimizer"])
        if scaler is not None:
            scaler.load_state_dict(state["scaler"])
        if ema is not None:
            eng.load_ema_state(ema)
        if clip is not None:
            eng.load_clip_state(clip)
        eng.freeze_bn(bool(state["bn_frozen"]))
        eng.drop_accumulated_grads()
        ckpt.restore_rng(rng)
        return state["extra"]

    def save_model(self, save_dir, name, ema=False):
        """ema: write the averaged weights instead, as <name>_ema.encoder.pt / <name>_ema.decoder.pt -- ordinary state_dicts"""
        if ema:
            name = '{}_ema'.format(name)
        torch.save(self.encoder.ema_state_dict() if ema else self.encoder.state_dict(),
                   os.path.join(save_dir, '{}.encoder.pt'.format(name)))
        if hasattr(self, 'fcn_time'):
            torch.save(self.fcn_time.ema_state_dict() if ema else self.fcn_time.state_dict(),
                       os.path.join(save_dir, '{}.decoder.pt'.format(name)))
