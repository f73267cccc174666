"""Guarded optimizer step of the fused trainers: gradient-norm clipping and "skip if non-finite", decided on the device.

The fused trainers run backward and AdamW back to back, so there is no place for ``torch.nn.utils.clip_grad_norm_`` or a
``GradScaler``-style skip in between.  With ``max_grad_norm=`` / ``skip_nonfinite=`` a trainer issues one statistics launch over
its flat gradient (``ops.grad_guard``) and an AdamW that reads the verdict from a device-resident record
(``ops.adamw_guarded`` / ``ops.adamw64_guarded``; include/dosx.h: DosxStepGuard) - no host read in the step.  This module is
the host side: :class:`StepGuard`, the mixin ``trainer_base.TrainerBase`` carries, and :class:`GuardReport`, what one
read-back of the record says.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _abi, ops
from ._lib import DosxError

REASONS = ((_abi.DOSX_GUARD_NONFINITE, "non-finite gradient"), (_abi.DOSX_GUARD_OVERFLOW, "gradient norm overflowed"),
           (_abi.DOSX_GUARD_STALLED, "exchange stalled"))


def reason_names(bits: int) -> Tuple[str, ...]:
    return tuple(name for bit, name in REASONS if bits & bit)


@dataclass(frozen=True)
class GuardReport:
    """One read-back of a trainer's guard record.  ``norm`` / ``clip`` / ``skipped_last`` / ``reasons`` / ``n_bad`` /
    ``first_bad`` describe the LAST step (``first_bad``: (parameter name, index inside it) of the lowest non-finite gradient
    element, None: none); ``applied`` / ``skipped`` count the steps since the last ``check()`` that raised (or the start);
    ``first_skip_*`` describe the first skipped one of them (``first_skip_step``: the trainer's step number, applied steps
    before it + 1)."""
    norm: float
    clip: float
    skipped_last: bool
    reasons: Tuple[str, ...]
    n_bad: int
    first_bad: Optional[Tuple[Optional[str], int]]
    applied: int
    skipped: int
    first_skip_step: Optional[int]
    first_skip_reasons: Tuple[str, ...]
    first_skip_bad: Optional[Tuple[Optional[str], int]]


def locate(fp, index: int) -> Optional[Tuple[Optional[str], int]]:
    """(parameter name, index inside it) of flat index ``index`` (< 0: None); an index in the alignment gap behind a
    parameter has no name."""
    if index < 0:
        return None
    for n, o in zip(fp.names, fp.offsets):
        if o <= index < o + fp.P[n].numel():
            return n, index - o
    return None, index


class StepGuard:
    """The guard of a trainer (mixed into ``trainer_base.TrainerBase``).  Expects ``dist``, ``_who``, ``_fp``, ``_slots``,
    ``step_count``, ``_adamw_launch`` and the AdamW hyper-parameters.  ``step_count`` counts ATTEMPTS since the record was last
    zeroed plus the applied steps before that: the record's ``skipped`` is the difference to the applied count, and
    ``_guard_settle`` folds it in."""

    max_grad_norm: Optional[float] = None
    skip_nonfinite: bool = False
    _guard_rec = _guard_ws = None
    _guard_status = None              # device address of the exchanges' stall status on the record's device

    def _init_guard(self, max_grad_norm, skip_nonfinite) -> None:
        who = self._who
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if math.isnan(max_grad_norm) or max_grad_norm < 0.0:
                raise ValueError(f"{who}: max_grad_norm must be a non-negative number or None, got {max_grad_norm}")
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, bool(skip_nonfinite)
        self._guard_rec = self._guard_ws = None
        if self.guarded and self.dist is not None:
            raise DosxError(f"{who}(max_grad_norm / skip_nonfinite) is a single-GPU mode: not with dist (data parallelism)")

    @property
    def guarded(self) -> bool:
        """True: the optimizer step runs behind the gradient guard (either constructor argument switches it on;
        ``max_grad_norm`` alone still skips non-finite steps - a NaN coefficient would poison every parameter)."""
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _guard_buffers(self, device):
        if self._guard_rec is None or self._guard_rec.device != device:
            self._guard_rec, self._guard_ws = ops.guard_buffers(device)
            self._guard_status = ops.exchange_status_address(device)
        return self._guard_rec, self._guard_ws

    def _guarded_optimizer_step(self, fp, m, v) -> None:
        """statistics launch + the AdamW launch behind its record (``trainer_base.TrainerBase._adamw_launch``)"""
        rec, ws = self._guard_buffers(fp.flat.device)
        self.step_count += 1
        ops.grad_guard(fp.grad, fp.n_train, rec, ws, self.max_grad_norm, self.lr, self.betas[0], self.betas[1], self.step_count,
                       self._guard_status)
        self._adamw_launch(fp, m, v, rec)

    @property
    def grad_norm(self) -> torch.Tensor:
        """Norm of the last step's gradient before clipping (over its finite elements): a 0-dim float64 device view of the
        guard record - reading it does not synchronise; ``.item()`` does."""
        if not self.guarded:
            raise DosxError("grad_norm: this trainer has no gradient guard (max_grad_norm= / skip_nonfinite=)")
        fp = self._fp if self._fp is not None else self.model.flat_params()
        return self._guard_buffers(fp.flat.device)[0][1]

    def _applied_steps(self) -> int:
        """AdamW steps applied so far: ``step_count`` without the skipped attempts (a read-back when the guard has run)."""
        if self._guard_rec is None:
            return self.step_count
        return self.step_count - int(ops.guard_read(self._guard_rec).skipped)

    def _guard_reset(self) -> None:
        if self._guard_rec is not None:
            self._guard_rec.zero_()

    def guard_report(self) -> GuardReport:
        """What the guard's record says, in one read-back (which waits for the device)."""
        if not self.guarded:
            raise DosxError("guard_report: this trainer has no gradient guard (max_grad_norm= / skip_nonfinite=)")
        fp = self._fp if self._fp is not None else self.model.flat_params()
        r = ops.guard_read(self._guard_buffers(fp.flat.device)[0])
        return GuardReport(
            norm=float(r.norm), clip=float(r.clip), skipped_last=bool(r.skip), reasons=reason_names(int(r.reason)),
            n_bad=int(r.n_bad), first_bad=locate(fp, int(r.first_bad)), applied=int(r.applied), skipped=int(r.skipped),
            first_skip_step=int(r.first_skip_step) if r.skipped else None, first_skip_reasons=reason_names(int(r.first_skip_reason)),
            first_skip_bad=locate(fp, int(r.first_skip_bad)) if r.skipped else None)

    def _guard_settle(self) -> Optional[str]:
        """``check()``'s part: None when no step was skipped since the last check; else the message to raise with - after
        ``step_count`` has become the applied count, the sticky fields are zeroed and the slots dropped (a static buffer may
        hold a stale non-finite value: the next step of each shape rebuilds and re-records it)."""
        if not self.guarded or self._guard_rec is None:
            return None
        fp = self._fp
        r = ops.guard_read(self._guard_rec)
        if int(r.skipped) == 0:
            return None
        skipped, step, reasons = int(r.skipped), int(r.first_skip_step), reason_names(int(r.first_skip_reason))
        where = locate(fp, int(r.first_skip_bad)) if fp is not None else None
        self.step_count -= skipped
        self._guard_rec.zero_()
        self._slots = OrderedDict()
        if where is not None:
            what = f"gradient of {where[0]}[{where[1]}] is not finite" if where[0] is not None else \
                f"flat gradient element {where[1]} is not finite"
            if len(reasons) > 1:
                what += f" ({', '.join(reasons)})"
        else:
            what = ", ".join(reasons)
        return (f"step {step}: {what}; {skipped} step{'s' if skipped != 1 else ''} skipped since the last check, parameters and "
                f"moments are those after {self.step_count} applied steps.  The guard's counts are zeroed and the recorded "
                f"slots dropped: the next step of each shape rebuilds its static buffers.")
