"""Exponential moving average of the weights of the fused trainers, kept by the AdamW launch itself.

``torch.optim.swa_utils.AveragedModel`` with an EMA ``multi_avg_fn``, ``torch-ema`` and timm's ``ModelEma`` make a second pass over
every parameter after ``optimizer.step()``.  The fused trainers have no place for that pass - and it would know nothing of a step
the gradient guard skipped on the device.  With ``ema_decay=`` the one flat AdamW launch also updates the average
(``ops.adamw*(..., ema=...)``; include/dosx.h: DosxAdamWEma, dosx_adamw_ema / _f64): the thread that holds the new parameter in
registers reads and writes one more buffer.  This module is the host side: :class:`WeightEma`, the mixin
``trainer_base.TrainerBase`` carries - the buffer and its re-homing, ``ema_weights()`` (evaluate under the average: one
``dosx_swap_buffers`` launch in, one out), ``ema_state_dict()`` and the checkpoint keys.
"""
from __future__ import annotations

import contextlib
import math
from typing import Optional

import torch

from . import ops
from ._lib import DosxError

BLOCK = "with trainer.ema_weights():"


def check_decay(who: str, decay) -> Optional[float]:
    if decay is None:
        return None
    decay = float(decay)
    if math.isnan(decay) or not 0.0 <= decay < 1.0:
        raise ValueError(f"{who}: ema_decay must be in [0, 1) or None, got {decay}")
    return decay


def schedule(decay: float, warmup: bool, t: int) -> float:
    """d_t after ``t`` steps of averaging, in double: ``min(decay, (1 + t) / (10 + t))`` under warm-up, else ``decay`` - the host
    twin of the kernel's expression (csrc/adamw_scalars.h: adamw_ema_decay), before its rounding to the buffer's type."""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


class WeightEma:
    """The weight average of a trainer (mixed into ``trainer_base.TrainerBase``).  Expects ``model``, ``dist``, ``_who`` (what
    the driver calls itself in its refusals), ``_fp``, ``_state`` and ``_applied_steps``.  ``_ema`` is laid out like ``fp.flat``,
    in its dtype; ``_ema_t0`` is AdamW's time when averaging began."""

    _ema_decay: Optional[float] = None
    ema_warmup: bool = True
    _ema = None
    _ema_t0 = 0
    _ema_block = False                # True inside ema_weights(): flat holds the average, _ema the parameters

    def _init_ema(self, ema_decay, ema_warmup) -> None:
        self._ema_decay = check_decay(self._who, ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._ema, self._ema_t0, self._ema_block = None, 0, False
        if self._ema_decay is not None and self.dist is not None:
            raise DosxError(f"{self._who}(ema_decay=...) is a single-GPU mode: not with dist (data parallelism)")

    @property
    def ema_decay(self) -> Optional[float]:
        """None: no average (fixed at construction).  Else the decay the optimizer step reads at EVERY step: assigning it
        between steps is a decay schedule, as ``param_groups[k]["lr"]`` is a learning-rate schedule."""
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, value) -> None:
        if self._ema_decay is None:
            raise DosxError(f"{self._who}: built without ema_decay=, there is no average to set a decay for")
        value = check_decay(self._who, value)
        if value is None:
            raise ValueError(f"{self._who}: ema_decay cannot be switched off on a running trainer")
        self._ema_decay = value

    def _ema_refuse(self, what: str) -> None:
        if self._ema_block:
            raise DosxError(f"{self._who}.{what} inside `{BLOCK}` - the model holds the averaged weights there, and the "
                            f"trained ones come back when the block ends; nothing trains, freezes or checkpoints in between")

    def _ema_rehome(self, fp, old) -> None:
        """``_state``'s part: the average follows the layout ``fp`` BY NAME, as the moments do.  A parameter new to the layout
        (and every one when averaging starts here, at ``t0`` = the applied steps) starts at its current value; a frozen one is
        never touched by a launch, so its average stays the parameter itself."""
        if self._ema_decay is None:
            return
        ema = fp.flat.clone()
        if old is not None and self._ema is not None:
            old_off = dict(zip(old.names, old.offsets))
            with torch.no_grad():
                for n, o in zip(fp.names, fp.offsets):
                    oo = old_off.get(n)
                    if oo is not None:
                        k = fp.P[n].numel()
                        ema[o:o + k].copy_(self._ema[oo:oo + k])
        else:
            self._ema_t0 = int(self._applied_steps())
        self._ema = ema

    def _ema_operand(self):
        """``ema=`` of the ``ops.adamw*`` functions for this step, None without an average."""
        if self._ema_decay is None:
            return None
        return (self._ema, self._ema_decay, self.ema_warmup, self._ema_t0)

    def _ema_require(self, what: str):
        if self._ema_decay is None:
            raise DosxError(f"{self._who}.{what}: this trainer keeps no weight average (ema_decay=)")
        fp = self._fp if self._fp is not None else self.model.flat_params()
        if not self._ema_block:
            self._state(fp)
        return self._fp

    @contextlib.contextmanager
    def ema_weights(self):
        """``with trainer.ema_weights():`` - the model holds the AVERAGED weights inside the block: one ``dosx_swap_buffers``
        launch over the flat parameters on entry and one on exit, also when the body raises.  Parameters are views of the flat
        buffer, which every recorded launch addresses by pointer, so everything that reads the model sees the average and
        nothing is re-recorded: ``Predictor`` / ``Predictor64``, ``evaluate.test*``, ``model.state_dict()``,
        ``checkpoint.save(path, model)``.  Inside, ``step``, ``step_dataset``, ``forward_backward``, ``optimizer_step``,
        ``state_dict`` / ``load_state_dict`` raise :class:`DosxError`, and so does the end of a block in which the model's
        frozen set was changed (the trained parameters are put back first).  The block does not nest.  A module that is not
        on the GPU is refused: the swap is a device launch."""
        who = self._who
        if self._ema_block:
            raise DosxError(f"{who}.ema_weights: `{BLOCK}` does not nest")
        dev = self.model._module_device()
        if self._ema_decay is not None and dev.type != "cuda":
            raise DosxError(f"{who}.ema_weights: the module is on {dev}; the average is swapped in by a device launch "
                            f"(move the module with .to('cuda') first)")
        fp = self._ema_require("ema_weights")
        ops.swap_buffers(fp.flat, self._ema)
        self._ema_block = True
        failed = True
        try:
            yield self
            failed = False
        finally:
            self._ema_block = False
            ops.swap_buffers(fp.flat, self._ema)
            now = self.model._flat
            if now is not fp and now is not None:          # freeze() / update_trainable() inside: the new layout was filled with the
                with torch.no_grad():                      # average - give it the trained values back, by name
                    for n in now.names:
                        if n in fp.P:
                            now.P[n].copy_(fp.P[n])
                if not failed:
                    raise DosxError(f"{who}: the model's flat parameters were laid out anew (freeze / train_only / "
                                    f"update_trainable, a device move) inside `{BLOCK}`; the trained parameters have been put "
                                    f"back - change the frozen set outside the block")

    def ema_state_dict(self) -> dict:
        """The averaged weights under the model's ``state_dict()`` keys (the reference's layout), as CPU tensors, without a swap:
        ``plain_model.load_state_dict(trainer.ema_state_dict())``.  Entries the average does not cover (buffers, parameters no
        program reads) are the model's own."""
        fp = self._ema_require("ema_state_dict")
        sd = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        if self._ema_block:                                # the model holds the average right now
            return sd
        for n, o in zip(fp.names, fp.offsets):
            if n in sd:
                sd[n] = self._ema[o:o + fp.P[n].numel()].view(fp.P[n].shape).detach().cpu().clone()
        return sd

    # ---- checkpoint -------------------------------------------------------------------------------------------------------
    def _ema_save(self, sd: dict, views) -> None:
        """``state_dict()``'s part: two more keys, only with an average (a run without writes the file it always wrote)."""
        if self._ema_decay is None:
            return
        sd["ema"] = views(self._ema)
        sd["ema_hyper"] = {"decay": self._ema_decay, "warmup": self.ema_warmup, "t0": self._ema_t0}

    def _ema_load(self, sd: dict, fp) -> None:
        """``load_state_dict()``'s part (the model's parameters are loaded first, as ``checkpoint.load`` does): a file with an
        average restores it - the resumed run is bitwise the uninterrupted one; a file without starts the average at the loaded
        parameters with ``t0`` = the file's step; a trainer without an average ignores the keys."""
        if self._ema_decay is None:
            return
        saved = sd.get("ema")
        with torch.no_grad():
            if saved is None:
                self._ema.copy_(fp.flat)
                self._ema_t0 = int(sd["step"])
                return
            missing = [n for n in fp.names if n not in saved]
            if missing:
                raise KeyError(f"weight average lacks {missing[:3]}{'...' if len(missing) > 3 else ''}")
            for n, o in zip(fp.names, fp.offsets):
                k = fp.P[n].numel()
                self._ema[o:o + k].copy_(saved[n].reshape(-1).to(self._ema.device, self._ema.dtype))
        h = sd.get("ema_hyper", {})
        self._ema_decay = check_decay(self._who, h.get("decay", self._ema_decay))
        self.ema_warmup, self._ema_t0 = bool(h.get("warmup", self.ema_warmup)), int(h.get("t0", 0))
