"""step(): same call sequence as reference models/util.py:50-58; LossScaler / DynamicLossScaler: the GradScaler of the fp16 build."""
import os

from .. import state_words as W

_LAZY = os.environ.get("VPD_LAZY_GRADS", "1") != "0"      # A/B switch: 0 = step() runs the plain loss.backward()


class LossScaler:
    """What torch.cuda.amp.GradScaler is to the reference's CUDA path (train_vpd_model.py:105; models/util.py:55-57) for a student
    built with dtype="fp16": `scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()`.

    The scale is STATIC (a power of two, default 256): activation gradients are stored in fp16 (6e-5 smallest normal), the loss is a
    SUM over crops (train_vpd_model.py:87) so d(loss)/d(emb) is O(1) per element whatever the batch, and weight gradients, BatchNorm
    sums and AdamW are fp32 -- 256 keeps the stem's activation gradients normal with 2^8 of head-room below fp16's 65,504.
    scale(loss).backward() leaves every .grad scaled, as GradScaler does; step() un-scales: the fused AdamW reads gradients x 1 / scale
    in its kernel, any other optimizer gets the flat gradient buffer multiplied by 1 / scale first.  A non-finite epoch loss is
    reported by ModelTrainer.epoch (there is no per-step inf check here: DynamicLossScaler has one, on the device)."""

    def __init__(self, engine, init_scale=256.0):
        if float(init_scale) <= 0:
            raise ValueError("loss scale must be positive")
        self._engine = engine
        self._scale = float(init_scale)

    def get_scale(self):
        return self._scale

    def scale(self, loss):
        if not hasattr(loss, "_t"):
            raise TypeError("LossScaler.scale() takes the loss object of ModelTrainer's forward")
        self._engine.loss_scale = self._scale
        return loss

    def step(self, optimizer):
        eng = self._engine
        if getattr(optimizer, "consumes_lazy_grads", False):
            optimizer.step()                       # (FusedAdamW: engine.adamw_step un-scales in the kernel)
        else:
            eng.unscale_grads_()
            optimizer.step()
        eng.loss_scale = 1.0

    def update(self):
        return None

    def state_dict(self):
        """the static scaler's state: its scale"""
        return {"scale": self._scale}

    def load_state_dict(self, state):
        if float(state["scale"]) <= 0:
            raise ValueError("loss scale must be positive")
        self._scale = float(state["scale"])


class DynamicLossScaler(LossScaler):
    """torch.cuda.amp.GradScaler() as the reference runs it (train_vpd_model.py:105, its defaults): look for inf / NaN in the
    gradients, SKIP the optimizer step when one is found and halve the scale, double it after `growth_interval` clean steps in a row.

    The whole decision runs on the device.  The scaler owns one vpd_scale_state block (include/vpd_hip.h: scale, non-finite word,
    growth tracker, applied and skipped steps); the backward pass reads the scale from it, the non-finite search ORs into it, the
    fused AdamW reads it -- gradients x 1 / scale, bias corrections from the APPLIED step count, nothing written when the word is
    set -- and update() is a one-thread kernel.  With the fused optimizer (`consumes_lazy_grads`) a step costs no host
    synchronisation; get_scale(), skipped_steps and applied_steps read the block and synchronise when asked.  Any other optimizer
    gets the flat gradient buffer un-scaled, and the word is read on the host to call or skip optimizer.step(), as torch does.
    Under data parallelism the search runs after the all-reduce (inf and NaN survive a sum), so every replica decides alike."""

    def __init__(self, engine, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        super().__init__(engine, init_scale)
        if not float(growth_factor) >= 1.0 or not 0.0 < float(backoff_factor) <= 1.0 or int(growth_interval) < 1:
            raise ValueError("growth_factor >= 1, 0 < backoff_factor <= 1 and growth_interval >= 1 are required")
        self._growth, self._backoff, self._interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._state = W.host_block(W.ScaleState, scale=float(init_scale), applied_steps=int(engine.adam_step)).to(engine.device)
        engine.attach_scale_state(self._state)

    @property
    def state(self):
        """the device block (vpd_scale_state as int32[8]; element 0 holds the scale's float bits)"""
        return self._state

    def _host(self):
        return W.read(self._state, W.ScaleState)      # synchronises

    def get_scale(self):
        return self._host().scale

    @property
    def growth_tracker(self):
        return self._host().growth_tracker

    @property
    def applied_steps(self):
        return self._host().applied_steps

    @property
    def skipped_steps(self):
        return self._host().skipped_steps

    def scale(self, loss):
        if not hasattr(loss, "_t"):
            raise TypeError("LossScaler.scale() takes the loss object of ModelTrainer's forward")
        self._engine.scale_state = self._state      # the backward pass and the optimizer step in flight read the block
        return loss

    def step(self, optimizer):
        eng = self._engine
        if eng.scale_state is not self._state:
            raise RuntimeError("DynamicLossScaler.step() without scale(loss).backward() before it")
        try:
            if getattr(optimizer, "consumes_lazy_grads", False):
                optimizer.step()                   # (FusedAdamW -> engine.adamw_step: non-finite search + skipping AdamW, enqueued)
            else:
                eng.check_grads_finite_(self._state)
                eng.unscale_grads_by_block_(self._state)                       # device-side reciprocal: no sync
                if int(self._state[W.word(W.ScaleState, "found")].item()) == 0:      # the one host read of this path, as torch's
                    optimizer.step()
        finally:
            eng.scale_state = None

    def update(self):
        self._engine.scale_state_update(self._state, self._growth, self._backoff, self._interval)

    def state_dict(self):
        """torch.amp.GradScaler.state_dict()'s keys (scale, growth_factor, backoff_factor, growth_interval, _growth_tracker) plus
        skipped_steps, read from the device block (synchronises).  The applied-step count is the optimizer's `step`: not here."""
        from ..checkpoint import scaler_state_dict
        return scaler_state_dict(self._host(), self._growth, self._backoff, self._interval)

    def load_state_dict(self, state):
        """Scale, growth tracker and skipped steps go into the device block, the non-finite word is cleared, the three factors are
        taken over.  A plain GradScaler dictionary loads (skipped_steps = 0).  The applied-step word is NOT written: it is the
        optimizer's `step`, which FusedAdamW.load_state_dict() puts there through engine.adam_step -- load the optimizer first or
        afterwards, the two do not touch each other's words."""
        from ..checkpoint import scaler_fields
        fields = scaler_fields(state)
        growth, backoff, interval = float(state["growth_factor"]), float(state["backoff_factor"]), int(state["growth_interval"])
        if not growth >= 1.0 or not 0.0 < backoff <= 1.0 or interval < 1:
            raise ValueError("growth_factor >= 1, 0 < backoff_factor <= 1 and growth_interval >= 1 are required")
        W.write(self._state, W.ScaleState, found=0, **fields)
        self._growth, self._backoff, self._interval = growth, backoff, interval
        self._scale = float(state["scale"])


def step(optimizer, scaler, loss, accumulate=False):
    """The reference's step() (models/util.py:50-58): loss.backward(); optimizer.step() -- or, with a scaler,
    scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update() -- then optimizer.zero_grad().

    accumulate=True: a non-final micro-batch of a gradient-accumulation window -- scaler.scale(loss) when a scaler is given, the
    backward, then the gradients go into the engine's accumulator (StudentEngine.accumulate_grads); optimizer.step(), scaler.step(),
    scaler.update() and zero_grad() are NOT called, so the scale stays fixed across the window, as torch's does.  The window's last
    call (accumulate=False) takes the sum: FusedAdamW's step folds it in by itself, any other optimizer gets it folded into the flat
    buffer before optimizer.step() / scaler.step().  The loss is a sum over crops: no 1/K.

    The bf16 build computes with fp32 accumulation and needs no loss scaling: get_optimizer() returns scaler=None there; a student
    built with dtype="fp16" (the reference's own GPU precision) gets a LossScaler (static) or a DynamicLossScaler."""
    if scaler is not None and not isinstance(scaler, LossScaler):
        raise ValueError("the HIP path takes scaler=None (bf16) or a vpd_amd.models.util.LossScaler (fp16), not %r" % type(scaler))
    # The fused loss object offers a backward that leaves the conv weight gradients in the kernels' own layout -- ONLY an
    # optimizer that reads that layout may get it (FusedAdamW: `consumes_lazy_grads`).  Any other optimizer (the reference's
    # step() accepts any: torch.optim.AdamW over encoder.parameters(), a wrapper that looks at p.grad) gets the plain
    # loss.backward(), which completes every p.grad view of the flat gradient buffer.
    lazy = _LAZY and getattr(optimizer, "consumes_lazy_grads", False) and hasattr(loss, "backward_for_step")
    if accumulate:
        if not hasattr(loss, "backward_for_accumulation"):
            raise TypeError("step(accumulate=True) takes the loss object of ModelTrainer's forward (a torch loss accumulates into "
                            ".grad by itself: call loss.backward())")
        (loss if scaler is None else scaler.scale(loss)).backward_for_accumulation(lazy=bool(lazy))
        return
    # the sum of the window's earlier micro-batches, for an optimizer that reads p.grad (FusedAdamW's step folds by itself)
    fold = None if lazy or not hasattr(loss, "_t") else loss._t.encoder.engine.fold_accumulated_grads
    if scaler is None:
        (loss.backward_for_step if lazy else loss.backward)()
        if fold is not None:
            fold()
        optimizer.step()
    else:
        scaled = scaler.scale(loss)
        (scaled.backward_for_step if lazy else scaled.backward)()
        if fold is not None:
            fold()
        scaler.step(optimizer)
        scaler.update()
    optimizer.zero_grad()
