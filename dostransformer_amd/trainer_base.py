"""What the fused trainers share (train.Trainer, train64.Trainer64, train64.GraphnetworkTrainer64): :class:`TrainerBase`.

State: the AdamW moments laid out like the model's flat parameters with their checkpoint, the gradient guard
(``guard.StepGuard``), the weight average (``ema.WeightEma``), parameter groups, the objective (``loss=``) with its sample and
energy-bin weights and its linear functionals, the accumulation window and the bucket table (``slots.SlotCache``).

Driver: the public step methods - ``step``, ``step_accumulate``, ``step_dataset``, ``step_dataset_accumulate`` - and the two slot
flows behind them (a batch object copied into its bucket; a dataset selection collated straight into it), written once.  A
driver answers a small set of hooks: the program's dtype, what a step cannot run on, whether a step goes through a slot, the
step's context, the slot key, and the program itself - eager and on a slot."""
from __future__ import annotations

import struct
from collections import OrderedDict
from typing import Optional

import torch

from . import _abi
from . import functional as Fn
from . import functional64 as F64
from . import functionals as _fn
from . import ops
from . import param_groups as _pg
from ._lib import DosxError
from ._models import _SEED_MOD, rank_seed_offset
from .batch import bucket_sizes, pad_batch
from .ema import WeightEma
from .guard import StepGuard
from .slots import Slot, SlotCache


class _Width:
    """Stands in for a batch where only the node-feature width matters (FusedModel._extra_dead reads ``g.x.shape[1]``)."""

    def __init__(self, width: int):
        self.x = torch.empty(0, int(width))


class TrainerBase(StepGuard, WeightEma, SlotCache):
    """State and step driver of the fused trainers: the AdamW moments laid out like the model's flat parameters (in the flat
    buffer's dtype), their checkpoint in ``torch.optim.AdamW`` vocabulary, the per-step bump of the dropout seed, the
    gradient guard of the optimizer step (``guard.StepGuard``: ``max_grad_norm`` / ``skip_nonfinite``), the exponential moving
    average of the weights the AdamW launch keeps (``ema.WeightEma``: ``ema_decay`` / ``ema_warmup``, re-homed by name with the
    moments), the objective, the accumulation window and the public step methods.  Expects ``model``, ``dist``, ``bucket``,
    ``_fp``, ``_m``, ``_v``, ``_slots``, ``step_count``, the hyper-parameters ``lr``, ``betas``, ``eps``, ``wd``, ``beta`` and
    what ``slots.SlotCache`` expects.

    A driver sets ``_who`` and ``_dtype`` and answers ``_refuse`` (extended, not replaced), ``_slotted``, ``_prepare``,
    ``_extra``, ``_key``, ``_slot_meta``, ``_eager`` and ``_run_slot``."""

    _who = "trainer"                  # what the driver calls itself in its refusals
    _dtype = None                     # the program's dtype, fixed per driver class: torch.float32 or torch.float64

    # ---- what follows from the program's dtype, chosen here and nowhere else -------------------------------------------------
    def _tables(self, ds):
        """The resident tables of a ``loader.DeviceDataset`` in the program's dtype."""
        return ds._f32_tables() if self._dtype == torch.float32 else ds._f64_tables()

    def _cast(self, t):
        """A target or weight field in the program's dtype (a slot's static buffer comes back as it is)."""
        return Fn._f32(t) if self._dtype == torch.float32 else F64._f64(t)

    def _state(self, fp):
        """AdamW moments laid out like ``fp``.  When the parameters are re-homed (module moved to another device after
        ``load_state_dict``, a different dead-parameter set, ...) the moments follow BY NAME instead of being reset:
        ``step_count`` keeps counting, so zeroed moments would silently corrupt the bias correction."""
        if self._ema_block:                # (also what a freeze() / update_trainable() inside the block runs into)
            self._ema_refuse("_state (step, forward_backward, optimizer_step, state_dict, load_state_dict)")
        if self._fp is not fp:
            if self.dist is not None and fp.n_train != fp.total:
                raise DosxError(f"{type(self).__name__}(dist=...) with frozen parameters ({len(fp.frozen)} of {len(fp.names)}): "
                                f"fine-tuning is a single-GPU mode, not with dist (data parallelism)")
            m, v = torch.zeros_like(fp.flat), torch.zeros_like(fp.flat)
            old = self._fp
            if old is not None and self._m is not None:
                old_off = dict(zip(old.names, old.offsets))
                with torch.no_grad():
                    for n, o in zip(fp.names, fp.offsets):
                        oo = old_off.get(n)
                        if oo is None:
                            continue
                        k = fp.P[n].numel()
                        if old.P[n].numel() != k:
                            raise RuntimeError(f"parameter {n} changed size under a running optimizer")
                        m[o:o + k].copy_(self._m[oo:oo + k])
                        v[o:o + k].copy_(self._v[oo:oo + k])
            self._ema_rehome(fp, old)
            self._m, self._v, self._fp = m, v, fp
            self._acc = self._acc_loss = None      # (the window's accumulator belongs to the layout: made anew at the next window)
            self._slots = OrderedDict()
            if self._groups is not None:       # the chunk map belongs to the layout: rebuilt wherever the moments are re-homed
                self._chunk_group = _pg.chunk_map(fp, _pg.assignment(self._groups)).to(fp.flat.device)
        return self._m, self._v

    # ---- the flat parameters of a step ---------------------------------------------------------------------------------------
    _first_width_fixes_dead = False   # True (the GNN-only baselines, whose live node encoder follows the input width): the
    _dead = None                      # dead-parameter set of the first batch's width, kept in _dead, is the trainer's for good

    def _who_with_model(self) -> str:
        """What the driver calls itself where a refusal is about the model it drives."""
        return self._who

    def _flat_for(self, dev, g, width: Optional[int] = None):
        """The model's flat parameters for a batch (or, a dataset step, an input width).  Baselines: which node encoder is dead
        follows the width; the first batch fixes it for this trainer."""
        model = self.model
        if not self._first_width_fixes_dead:
            return model._ensure_flat(dev, g)
        if g is None:
            g = _Width(width)
        dead = model._extra_dead(g)
        if self._dead is None:
            self._dead = dead
        elif dead != self._dead:
            raise DosxError(f"{self._who_with_model()}: this batch has node features of width {g.x.shape[1]}, which selects the "
                            f"other node encoder than the trainer's first batch did - its dead-parameter set (and the "
                            f"optimizer's layout) is fixed by the first batch")
        return model._ensure_flat(dev, g)

    # ---- parameter groups (param_groups.py; include/dosx.h: DosxAdamWGroups) -------------------------------------------
    _groups = None                    # None: one lr / weight_decay, the ungrouped launch; else [{"lr", "weight_decay", "names"}]
    _chunk_group = None               # uint8 device tensor, one entry per 64 elements of flat[:n_train], of the layout in _fp
    _groups_host = None               # the kernel's host struct, filled from _groups at every optimizer step

    def _init_param_groups(self, groups) -> None:
        """``param_groups=`` of a trainer's constructor; call it once ``model``, ``dist``, ``lr`` and ``wd`` are set."""
        self._groups = self._chunk_group = self._groups_host = None
        if groups is None:
            return
        if self.dist is not None:
            raise DosxError(f"{self._who}(param_groups=...) is a single-GPU mode: not with dist (data parallelism)")
        self._groups = _pg.resolve(self.model, groups, self.lr, self.wd)
        self._groups_host = _abi.AdamWGroups()

    @property
    def param_groups(self):
        """None without ``param_groups=``; else the list of ``{"lr", "weight_decay", "names"}`` the optimizer step reads at
        EVERY step - entry 0 the parameters no group names (at the ``lr`` / ``weight_decay`` of construction), entry ``i + 1``
        the constructor's group ``i``.  Assigning ``trainer.param_groups[k]["lr"]`` between steps is a learning-rate schedule:
        nothing is re-recorded, nothing waits for the device.  ``names`` are fixed at construction."""
        return self._groups

    # ---- optimizer -------------------------------------------------------------------------------------------------------
    def _adamw_launch(self, fp, m, v, rec=None) -> None:
        """The optimizer's one launch for ``step_count``, the only place that chooses among the ``ops.adamw*`` functions: fp32 or
        float64 by the flat buffer, behind the guard's record ``rec`` or not, with the trainer's parameter groups or its one
        ``lr`` / ``wd``, keeping the weight average (``ema=``) or not.  ``flat[n_train:]`` are the frozen parameters, nothing steps
        them (nor their average, which is the parameter itself): no launch when everything is frozen."""
        if not fp.n_train:
            return
        grouped, guarded = self._groups is not None, rec is not None
        name = ("adamw" if fp.flat.dtype == torch.float32 else "adamw64") + ("_grouped" if grouped else "") + ("_guarded" if guarded else "")
        if grouped:
            st = ops.adamw_groups([(grp["lr"], grp["weight_decay"]) for grp in self._groups], into=self._groups_host)
            args = (self._chunk_group, st, self.betas[0], self.betas[1], self.eps, self.step_count)
        else:
            args = (self.lr, self.betas[0], self.betas[1], self.eps, self.wd) + (() if guarded else (self.step_count,))
        kw = {}
        if self._ema_decay is not None:
            kw["ema"] = self._ema_operand()
            if guarded and not grouped:       # (the other three forms take the step anyway)
                kw["step"] = self.step_count
        getattr(ops, name)(fp.flat, fp.grad, m, v, fp.n_train, *args, *((rec,) if guarded else ()), **kw)

    def _reduce_gradients(self, fp) -> None:
        """Between the backward and the unguarded optimizer launch: nothing here; Trainer finishes its ``dist`` all-reduces."""

    def optimizer_step(self) -> None:
        """The flat AdamW launch, issued behind the (recorded) program: ``step`` changes every step."""
        self._ema_refuse("optimizer_step")
        fp = self._fp if self._fp is not None else self.model.flat_params()
        m, v = self._state(fp)
        if self.guarded:                              # (never with dist: refused at construction)
            return self._guarded_optimizer_step(fp, m, v)
        self._reduce_gradients(fp)
        self.step_count += 1
        self._adamw_launch(fp, m, v)

    # ---- checkpoint / resume (absent upstream) ------------------------------------
    def state_dict(self) -> dict:
        """Optimizer state keyed by the reference's parameter names, in ``torch.optim.AdamW`` vocabulary
        (``exp_avg`` / ``exp_avg_sq`` / ``step``); together with ``model.state_dict()`` (reference key
        layout) this is a complete resume point.  Every live parameter has an entry, frozen ones included (their
        moments are whatever they were when they were frozen: zero if they never trained), so a file loads into a trainer with
        another frozen set, by name; with anything frozen, ``trainable`` lists the names that were training (no such key: all).

        The trainer keeps ONE ``step`` for all parameters: a parameter unfrozen in the middle of a run starts from zero moments
        under the run's bias correction, where ``torch.optim.AdamW`` would start a step count of its own for it.

        With ``ema_decay``, and only then: ``ema`` (the averaged weights, by name) and ``ema_hyper`` (``decay``, ``warmup``, ``t0``)."""
        self._ema_refuse("state_dict")
        fp = self._fp if self._fp is not None else self.model.flat_params()
        m, v = self._state(fp)
        views = lambda buf: {n: buf[o:o + fp.P[n].numel()].view(fp.P[n].shape).detach().cpu().clone()
                             for n, o in zip(fp.names, fp.offsets)}
        # the dropout seed is stored WITHOUT the saving rank's offset (rank-independent base + steps taken): every rank of a
        # resumed data-parallel job re-applies its own offset and goes on drawing the masks its uninterrupted self would have
        seed = getattr(self.model, "_drop_seed", None)
        sd = {"step": self._applied_steps(), "exp_avg": views(m), "exp_avg_sq": views(v),
              "drop_seed_base": None if seed is None else (int(seed.item()) - rank_seed_offset()) % _SEED_MOD,
              "hyper": {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd, "beta": self.beta}}
        if fp.frozen:                      # (an all-trainable run writes the file it always wrote: no key = every name trains)
            sd["trainable"] = fp.trainable_names()
        if self._groups is not None:       # (a run without groups writes the file it always wrote)
            sd["param_groups"] = [{"lr": grp["lr"], "weight_decay": grp["weight_decay"], "names": list(grp["names"])}
                                  for grp in self._groups]
        self._ema_save(sd, views)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        self._ema_refuse("load_state_dict")
        fp = self._fp if self._fp is not None else self.model.flat_params()
        m, v = self._state(fp)
        missing = [n for n in fp.names if n not in sd["exp_avg"] or n not in sd["exp_avg_sq"]]
        if missing:
            raise KeyError(f"optimizer state lacks {missing[:3]}{'...' if len(missing) > 3 else ''}")
        with torch.no_grad():
            for n, o in zip(fp.names, fp.offsets):
                k = fp.P[n].numel()
                m[o:o + k].copy_(sd["exp_avg"][n].reshape(-1).to(m.device, m.dtype))
                v[o:o + k].copy_(sd["exp_avg_sq"][n].reshape(-1).to(v.device, v.dtype))
        self.step_count = int(sd["step"])
        self._guard_reset()                # (the applied count starts here: nothing skipped since)
        val = None
        if sd.get("drop_seed_base") is not None:     # resume draws the masks THIS rank's uninterrupted run would have drawn
            val = (int(sd["drop_seed_base"]) + rank_seed_offset()) % _SEED_MOD
        elif sd.get("drop_seed") is not None:        # (files of round 3: the saving rank's own seed)
            val = int(sd["drop_seed"])
        if val is not None:
            object.__setattr__(self.model, "_drop_seed", torch.tensor([val], dtype=torch.int64, device=m.device))
        h = sd.get("hyper", {})
        self.lr, self.eps, self.wd = h.get("lr", self.lr), h.get("eps", self.eps), h.get("weight_decay", self.wd)
        self.betas, self.beta = tuple(h.get("betas", self.betas)), h.get("beta", self.beta)
        saved = sd.get("param_groups")
        if self._groups is not None and saved is not None and len(saved) == len(self._groups):
            for grp, old in zip(self._groups, saved):      # by group index; another number of groups: the trainer keeps its own
                grp["lr"], grp["weight_decay"] = float(old["lr"]), float(old["weight_decay"])
        self._ema_load(sd, fp)

    def check(self) -> None:
        """Raise :class:`DosxError` if a column-split exchange of any step since the last clean check reported a stall
        (``ops.check_exchanges``): one small read-back, so call it where the host waits for the device anyway - per evaluation,
        before a checkpoint - not per step.  A module that is not on the GPU has launched nothing: nothing to check.

        A guarded trainer (``max_grad_norm`` / ``skip_nonfinite``) also raises when steps were skipped since the last check,
        naming the first one and the parameter whose gradient was not finite; by then ``step_count`` is the applied count, the
        guard's counts are zeroed and the slots dropped, so the process can go on.

        Also raises when the model's ``requires_grad`` flags no longer match the snapshot the flat buffer was laid out from
        (``FusedModel.update_trainable()`` is the missing call)."""
        if self.model.trainable_stale():
            raise DosxError(f"{type(self.model).__name__}: requires_grad changed since the flat parameters were laid out, and the "
                            f"steps since then trained the earlier set - call model.update_trainable() after changing the flags "
                            f"(model.freeze() / model.train_only() do)")
        dev = self.model._module_device()
        if dev.type != "cuda":
            return
        skipped = self._guard_settle()
        try:
            ops.check_exchanges(dev)
        except DosxError as e:
            if skipped is None:
                raise
            raise DosxError(f"{e}  {skipped}") from None
        if skipped is not None:
            raise DosxError(skipped)

    def _bump_dropout_seed(self) -> None:
        """Attention dropout draws its masks from a device-resident seed inside the (possibly recorded) program; one bump
        per step, issued here so that it is never part of a recording."""
        seed = getattr(self.model, "_drop_seed", None)
        if seed is not None and self.model.training and getattr(self.model, "_attn_drop", 0.0) > 0.0:
            seed.add_(1)

    # ---- the objective (ops.LOSS_KINDS; include/dosx.h: dosx_loss_rows / dosx_loss_rows_f64) ----------------------------------
    loss = None                       # None: the reference driver's loss, the launches the step always issued; else a key of LOSS_KINDS
    huber_delta = None
    crystal_losses = None             # [B] device tensor, the last step's l_b (valid until the next step); None under the default

    def _init_loss(self, loss, huber_delta) -> None:
        """``loss=`` / ``huber_delta=`` of a trainer's constructor.  Constructor arguments like ``beta``: not part of ``state_dict()``."""
        who = self._who
        self.loss = self.huber_delta = self.crystal_losses = None
        names = ", ".join(repr(k) for k in ops.LOSS_KINDS)
        if loss is not None and loss not in ops.LOSS_KINDS:
            raise ValueError(f"{who}(loss={loss!r}): not one of {names} (or None: the reference's loss)")
        if loss == "huber":
            if huber_delta is None or not 0.0 < float(huber_delta) < float("inf"):
                raise ValueError(f"{who}(loss='huber') needs a finite huber_delta > 0, got {huber_delta}")
        elif huber_delta is not None:
            raise ValueError(f"{who}(loss={loss!r}, huber_delta={huber_delta}): huber_delta belongs to loss='huber' alone "
                             f"(loss is None or one of {names})")
        if loss is not None and self.dist is not None:
            raise DosxError(f"{who}(loss=...) is a single-GPU mode: not with dist (data parallelism)")
        self.loss, self.huber_delta = loss, None if huber_delta is None else float(huber_delta)

    def _loss_count(self, B: int) -> int:
        """The count a per-crystal loss launch divides by: the batch's own outside an accumulation window, the window's total
        inside one."""
        return int(B) if self._window_total is None else self._window_total

    def _loss_rows(self, alloc, dev, pg, ps, y, clamp: bool, dpg, dps, B_global: Optional[int] = None, weights=(None, None)):
        """The one launch site of the per-crystal losses: -> (per-crystal l_b [B], loss 0-dim), both on static buffers when
        the step is being recorded.  ``ps = dps = None``: a one-output model (``beta`` is not read then).  ``B_global``: the
        count the mean is taken over - the batch's own outside an accumulation window, the window's total inside one.
        ``weights``: what ``_batch_weights`` returned for the batch; with them or with ``bin_weights=`` the weighted entry."""
        B = int(pg.shape[0])
        if B_global is None:
            B_global = self._loss_count(B)
        per, loss = alloc(dev, B), alloc(dev, 1)
        fn = ops.loss_rows if self._dtype == torch.float32 else ops.loss_rows64
        fn(pg, ps, y, self.loss, clamp_target=clamp, beta=self.beta, delta=self.huber_delta, dpg=dpg, dps=dps, per_crystal=per,
           loss=loss, B_global=int(B_global), weights=weights[0], weight_index=weights[1],
           bin_weights=self._bin_operand(dev), **self._functional_operands(dev))
        return per, loss[0]

    # ---- sample weights and energy-bin weights (include/dosx.h: dosx_loss_rows_w / dosx_loss_rows_w_f64) --------
    sample_weights = False            # True: every batch carries a [B] field `weight`, step_dataset reads the dataset's table
    bin_weights = None                # None, or the [S] energy-bin weights as given (float64, on the host)
    _bin_dev = None                   # ... on the device in the program's dtype, moved there once

    def _init_weights(self, sample_weights, bin_weights) -> None:
        """``sample_weights=`` / ``bin_weights=`` of a trainer's constructor; call it after ``_init_loss``.  Constructor arguments
        like ``beta`` and ``loss``: not part of ``state_dict()``."""
        who = self._who
        self.sample_weights, self.bin_weights, self._bin_dev = bool(sample_weights), None, None
        if not self.sample_weights and bin_weights is None:
            return
        what = " and ".join(n for n, on in (("sample_weights=True", self.sample_weights), ("bin_weights=...", bin_weights is not None)) if on)
        if self.dist is not None:
            raise DosxError(f"{who}({what}) is a single-GPU mode: not with dist (data parallelism)")
        if self.loss is None:
            raise ValueError(f"{who}({what}) weighs the per-crystal losses: pass loss=\"crystal_rmse\" (on an eDOS model the default "
                             f"objective, bit for bit) or another of {', '.join(repr(k) for k in ops.LOSS_KINDS)}")
        if bin_weights is None:
            return
        v = bin_weights if torch.is_tensor(bin_weights) else torch.as_tensor(bin_weights, dtype=torch.float64)
        v = v.detach().to("cpu", torch.float64).clone()
        S = int(self.model._cfg.S)
        if v.dim() != 1 or v.numel() != S:
            raise ValueError(f"{who}(bin_weights=...): shape {tuple(v.shape)}, want [S] = [{S}], one weight per energy bin")
        if not bool(torch.isfinite(v).all()) or bool((v < 0).any()):
            raise ValueError(f"{who}(bin_weights=...): every bin weight must be finite and >= 0")
        if not float(v.sum()) > 0.0:
            raise ValueError(f"{who}(bin_weights=...): the bin weights sum to 0 - no bin would be left in the loss")
        self.bin_weights = v

    def _bin_operand(self, dev):
        if self.bin_weights is None:
            return None
        if self._bin_dev is None or self._bin_dev.device != dev:
            if self._bin_dev is not None:      # (the module moved: the recordings hold the old buffer's address)
                self._slots = OrderedDict()
            self._bin_dev = self.bin_weights.to(dev, self._dtype).contiguous()
        return self._bin_dev

    # ---- linear functionals of the DOS in the loss (include/dosx.h: dosx_loss_rows_fn / dosx_loss_rows_fn_f64) ----
    # ---- and rows of the table over one floored denominator functional (dosx_loss_rows_fn_norm / _f64) -----------
    functionals = None                # None, or the functionals.Functionals whose table the loss reads (float64, on the host)
    functional_kind = "sq"
    functional_weight = 1.0           # lam: recorded with the launch, fixed for the trainer's life
    _fn_dev = None                    # the table (and behind it the denominator) on the device in the program's dtype: ONE buffer,
    #                                   written in place ever after

    def _init_functionals(self, functionals, functional_kind="sq", functional_weight=1.0) -> None:
        """``functionals=`` / ``functional_kind=`` / ``functional_weight=`` of a trainer's constructor; call it after
        ``_init_weights``.  Constructor arguments like ``loss``: not part of ``state_dict()``."""
        who = self._who
        self.functionals, self.functional_kind, self.functional_weight, self._fn_dev = None, "sq", 1.0, None
        if functionals is None:
            if functional_kind != "sq" or float(functional_weight) != 1.0:
                raise ValueError(f"{who}(functional_kind={functional_kind!r}, functional_weight={functional_weight}) without "
                                 f"functionals=...: there is no table they could apply to")
            return
        if self.dist is not None:
            raise DosxError(f"{who}(functionals=...) is a single-GPU mode: not with dist (data parallelism)")
        if self.loss is None:
            raise ValueError(f"{who}(functionals=...) adds a term to the per-crystal losses: pass loss=\"crystal_rmse\" (on an eDOS "
                             f"model the default objective, bit for bit) or another of {', '.join(repr(k) for k in ops.LOSS_KINDS)}")
        if functional_kind not in ops.FUNCTIONAL_KINDS:
            raise ValueError(f"{who}(functional_kind={functional_kind!r}): not one of "
                             f"{', '.join(repr(k) for k in ops.FUNCTIONAL_KINDS)}")
        lam = float(functional_weight)
        if not 0.0 <= lam < float("inf"):
            raise ValueError(f"{who}(functional_weight={functional_weight}): must be finite and >= 0")
        self.functionals = self._checked_functionals(f"{who}(functionals=...)", functionals)
        self.functional_kind, self.functional_weight = functional_kind, lam

    def _checked_functionals(self, what: str, fn):
        fn = _fn.as_functionals(fn)                   # (2-D and finite: its constructor)
        S, top = int(self.model._cfg.S), ops.FUNCTIONAL_MAX
        if fn.S != S:
            raise ValueError(f"{what}: the table has {fn.S} columns, the model {S} energy bins - want [K,S] = [K,{S}]")
        if fn.K > top or fn.S > top:
            raise ValueError(f"{what}: [K,S] = [{fn.K},{fn.S}], the loss takes at most {top} functionals of at most {top} bins")
        return fn

    def set_functionals(self, functionals) -> None:
        """Replace the table by another of the SAME shape, in place: the trainer's one device buffer is overwritten, nothing is
        re-recorded, and the next step - replayed or not - reads the new values.  A schedule on the term is a rescaled table
        (``fn.scaled(c)``: ``"sq"`` scales with c^2, ``"abs"`` with c); ``functional_weight`` itself stays what was recorded.
        With normalised rows (``functionals.centre`` ...; include/dosx.h: dosx_loss_rows_fn_norm) the table AND the denominator are
        written; their count and the floor are part of the recorded launch, so another count or floor is refused."""
        if self.functionals is None:
            raise ValueError(f"{self._who}.set_functionals: the trainer was built without functionals=...")
        fn = self._checked_functionals(f"{self._who}.set_functionals", functionals)
        if fn.K != self.functionals.K:
            raise ValueError(f"{self._who}.set_functionals: [K,S] = [{fn.K},{fn.S}], the trainer's table is "
                             f"[{self.functionals.K},{self.functionals.S}] - the recorded launches hold its shape")
        if fn.K_norm != self.functionals.K_norm:
            raise ValueError(f"{self._who}.set_functionals: {fn.K_norm} normalised rows, the trainer's table has "
                             f"{self.functionals.K_norm} - the recorded launches hold their count")
        if fn.K_norm and struct.pack("<d", fn.floor) != struct.pack("<d", self.functionals.floor):
            raise ValueError(f"{self._who}.set_functionals: floor {fn.floor!r}, the trainer's is {self.functionals.floor!r} - the "
                             f"recorded launches hold the floor (the table and the denominator are what is written in place)")
        self.functionals = fn
        if self._fn_dev is not None:
            self._fn_dev.copy_(self._fn_host(fn))

    def _fn_host(self, fn) -> torch.Tensor:
        """What the device buffer holds, in the program's dtype: the table, plain rows first (``Functionals.device_layout``), and
        with normalised rows the denominator as one more row behind it.  Without any: the table as it is, the buffer of 9.12."""
        if not fn.K_norm:
            return fn.table.to(self._dtype)
        return torch.cat([fn.device_layout()[0], fn.denominator[None, :]]).to(self._dtype)

    def _functional_operands(self, dev) -> dict:
        """The keyword operands of ``ops.loss_rows`` for the term; none without a table: the call it always was."""
        if self.functionals is None:
            return {}
        if self._fn_dev is None or self._fn_dev.device != dev:
            if self._fn_dev is not None:       # (the module moved: the recordings hold the old buffer's address)
                self._slots = OrderedDict()
            self._fn_dev = self._fn_host(self.functionals).to(dev).contiguous()
        fn, K = self.functionals, self.functionals.K
        kw = {"functionals": self._fn_dev, "functional_kind": self.functional_kind, "functional_weight": self.functional_weight}
        if fn.K_norm:                          # K_norm and the floor are recorded with the launch; table and denominator are read
            kw.update(functionals=self._fn_dev[:K], functional_denominator=self._fn_dev[K], functional_norm_rows=fn.K_norm,
                      functional_floor=fn.floor)
        return kw

    def _require_weight(self, what: str, g) -> None:
        """``sample_weights=True``: the batch must carry ``weight`` - raised before anything is launched."""
        if self.sample_weights and not (hasattr(g, "weight") and torch.is_tensor(g.weight) and g.weight.is_floating_point()
                                        and g.weight.numel() == self._crystals_of(g)):
            raise ValueError(f"{self._who}.{what}: sample_weights=True, but the batch has no floating-point graph-level field "
                             f"`weight` of [B] = [{self._crystals_of(g)}] entries (DeviceDataset crystals with a \"weight\", or "
                             f"g.weight = ...)")

    def _require_weight_table(self, what: str, ds):
        """``sample_weights=True``: the dataset's resident weight table in the program's dtype, or the refusal."""
        if not self.sample_weights:
            return None
        w = self._tables(ds).get("weight")
        if w is None:
            raise ValueError(f"{self._who}.{what}: sample_weights=True, but the dataset holds no weights (crystals with a "
                             f"\"weight\", or ds.set_weights(w))")
        return w

    def _batch_weights(self, g):
        """(w, w_index) of batch ``g`` for ``_loss_rows``: ``g.weight`` converted as the target is (``_cast``), with
        ``g.weight_index`` where a dataset step left its table and the bucket's selection."""
        if not self.sample_weights:
            return (None, None)
        wi = getattr(g, "weight_index", None)
        if wi is None:
            self._require_weight("step", g)
        return (self._cast(g.weight).reshape(-1), wi)

    def _whole_or_window(self, B: int, n_global) -> bool:
        """True when ``n_global`` is the batch's own count - or, inside an accumulation window, the window's total (the internal
        route by which a micro-batch is normalised by a count that is not its own; callers cannot reach it)."""
        return int(n_global) == int(B) or (self._window_total is not None and int(n_global) == self._window_total)

    def _require_whole_batch(self, B: int, n_global) -> None:
        if self.loss is not None and not self._whole_or_window(B, n_global):
            raise ValueError(f"{type(self).__name__}(loss={self.loss!r}): n_global={n_global} but the batch holds {B} crystals "
                             f"(the per-crystal losses are a single-GPU mode)")

    # ---- gradient accumulation: several batches, one optimizer step (include/dosx.h: dosx_grad_accumulate) -----
    _acc = None                       # the window's accumulator, laid out like the moments; made at the first window with K > 1
    _acc_loss = None                  # [1]: the window's loss, summed by the same launches
    _window_total = None              # inside a window: T, the crystals of all its micro-batches; None outside.  The ONE route by
                                      # which a micro-batch's program learns the count its loss divides by

    def _window_checks(self, what: str, K: int) -> None:
        """What a window cannot run on and that its length alone decides - raised before the dropout seed, the accumulator or
        any slot is touched."""
        who = self._who
        self._ema_refuse(what)
        if K == 0:
            raise ValueError(f"{who}.{what}: an empty window - pass at least one batch")
        if self.dist is not None:
            raise DosxError(f"{who}.{what} is a single-GPU mode: not with dist (data parallelism)")
        if K > 1 and self.loss is None and self.model._cfg.kind == "phonon":
            raise DosxError(f"{who}.{what}: the reference's phonon loss is ONE RMSE pooled over the batch - its gradient needs "
                            f"every micro-batch's squared error before any backward, so it does not accumulate over {K} batches; "
                            f"build the trainer with loss=\"crystal_rmse\" (the reference's own objective at its batch size 1) or "
                            f"another per-crystal loss")
        if K > 1 and not self.model.trainable_names():
            raise DosxError(f"{who}.{what}: every parameter is frozen - there is no gradient to accumulate")

    @staticmethod
    def _crystals_of(g) -> int:
        """crystals in a batch object, without a host read (``system`` has one entry per crystal)"""
        return int(g.num_graphs if hasattr(g, "num_graphs") else g.system.shape[0])

    def _window_sizes(self, what: str, counts) -> list:
        sizes = [int(c) for c in counts]
        for k, B in enumerate(sizes):
            if B < 1:
                raise ValueError(f"{self._who}.{what}: batch {k} of the window is empty")
        return sizes

    def _window(self, what: str, sizes, run) -> torch.Tensor:
        """One optimizer step on the micro-batches ``k < len(sizes)`` (``sizes[k]`` crystals each, at least two of them):
        ``run(k)`` issues micro-batch k's ordinary program - normalised by the window's total, which ``_window_total`` carries -
        and returns its loss; behind each program ONE ``dosx_grad_accumulate`` launch on the main stream, outside the recording,
        where the optimizer launch goes: copy into the accumulator (k = 0: nothing stale is ever read), accumulator += gradient,
        and for the last one gradient = accumulator + gradient - the flat gradient buffer then holds ((G1 + G2) + G3) + ..., and
        the guard, AdamW, ``.grad`` and ``guard_report()`` work on it unchanged.  The same launches sum the losses.  Nothing of the
        optimizer's is touched before the last launch: an exception in between leaves parameters, moments, average and
        ``step_count`` alone, and the next window starts with a copy."""
        K, T = len(sizes), sum(sizes)
        accumulate = ops.grad_accumulate if self._dtype == torch.float32 else ops.grad_accumulate64
        crystals, off, fp0 = None, 0, None
        self._window_total = T
        try:
            for k in range(K):
                loss = run(k)
                fp = self._fp
                if k == 0:
                    fp0 = fp
                    if self._acc is None:
                        self._acc, self._acc_loss = torch.empty_like(fp.flat), torch.empty(1, dtype=fp.flat.dtype, device=fp.flat.device)
                    accumulate(self._acc, fp.grad, None, fp.n_train, sdst=self._acc_loss, sa=loss)
                elif fp is not fp0:
                    raise DosxError(f"{self._who}.{what}: the flat parameters were laid out anew inside a window (batch {k})")
                else:
                    accumulate(self._acc if k < K - 1 else fp.grad, self._acc, fp.grad, fp.n_train, sdst=self._acc_loss,
                               sa=self._acc_loss, sb=loss)
                if self.crystal_losses is not None:          # (a slot's [B] buffer is overwritten when the slot runs again)
                    if crystals is None:
                        crystals = torch.empty(T, dtype=self.crystal_losses.dtype, device=self.crystal_losses.device)
                    crystals[off:off + sizes[k]].copy_(self.crystal_losses)
                off += sizes[k]
        finally:
            self._window_total = None
        self.crystal_losses = crystals
        self.optimizer_step()
        return self._acc_loss[0]

    # ---- the hooks of a driver -----------------------------------------------------------------------------------------------
    def _refuse(self, what: str, g) -> None:
        """What a step cannot run on - raised before anything (the dropout seed included) has changed.  ``g`` is None for a
        dataset step, whose batch does not exist yet.  A driver with more to refuse extends this."""
        if g is not None:
            self._require_weight(what, g)

    def _slotted(self, dataset: bool) -> bool:
        """True: this step - on a batch object, or (``dataset``) on a selection of a device-resident dataset - runs on the
        static buffers of a slot.  Read per step: ``replay`` may be assigned on a live trainer."""
        raise NotImplementedError

    def _prepare(self, g, ds, B: int, n_global: Optional[int]):
        """-> (flat parameters, the count the step's loss is normalised by): every refusal that needs more than the batch
        object - the program's dtype, the input width, ``n_global`` - raised before the dropout seed is bumped or made, and
        what may touch the host or a collective (first use: flattening), in front of any recording.  ``g`` is None for a
        dataset step, which passes ``ds``; ``B``: the crystals of the batch."""
        raise NotImplementedError

    def _extra(self, fp, count: int):
        """The driver's own operand of the step, made behind the seed bump (a first step makes the dropout seed here, from
        torch's RNG) and in front of any recording: handed to ``_key``, ``_eager`` and ``_run_slot``."""
        raise NotImplementedError

    def _key(self, n: int, e: int, B: int, n_max: int, extra, tiled: bool) -> tuple:
        """What decides the launch list of a slot, the (padded) shape first."""
        raise NotImplementedError

    def _slot_meta(self, g, dev):
        """The metadata of a batch object that goes into a slot, or the refusal of one whose edges are not in the kernels'
        order."""
        raise NotImplementedError

    def _eager(self, fp, g, extra) -> torch.Tensor:
        """forward program, loss, backward program issued from Python on batch ``g``: -> loss."""
        raise NotImplementedError

    def _run_slot(self, slot: Slot, fp, extra, fresh: bool) -> torch.Tensor:
        """The step on a slot whose static buffers hold the batch: recorded (or captured) on first use, replayed afterwards."""
        raise NotImplementedError

    # ---- the step up to the optimizer ------------------------------------------------------------------------------------------
    _tiled = False                    # True: the slots of a dataset step carry the message-GEMM tile table (the fp32 program's)

    def _context(self, g, ds, B: int, n_global: Optional[int], bump: bool = True):
        """-> (flat parameters, extra) of a step, in the one order that keeps two facts: a refused step leaves the dropout
        seed alone (``_prepare`` first), and the step's bump is issued outside the recording and before the seed is made - on
        the very first step it is a no-op (``_extra`` last)."""
        fp, count = self._prepare(g, ds, B, n_global)
        if bump:
            self._bump_dropout_seed()
        return fp, self._extra(fp, count)

    def _batch_program(self, g, n_global: Optional[int], bump: bool = True) -> torch.Tensor:
        """The program of one batch object with the step's seed bump, eager or on its slot: a batch that is not padded yet is
        padded on the fly to its bucket, copied into the bucket's static buffers (made from it on first use), and the slot runs."""
        slotted = self._slotted(dataset=False)
        m = self._slot_meta(g, self.model._module_device()) if slotted else None        # (refused before any collective)
        fp, extra = self._context(g, None, self._crystals_of(g), n_global, bump)
        if not slotted:
            return self._eager(fp, g, extra)
        if self.bucket is not None and getattr(g, "real_nodes", None) is None:       # not padded yet: pad on the fly
            g = pad_batch(g, *bucket_sizes(m.num_nodes, m.num_edges, *self.bucket))
            m = g.meta
        key = self._key(m.num_nodes, m.num_edges, m.num_graphs, m.n_max, extra, m.seg_tile is not None)
        if self.sample_weights:               # (the last field of a dataset step's key is its table: this batch brings its own)
            key += (None,)
        slot = self._lookup(key)
        fresh = slot is None
        if fresh:                             # (graph mode captures on the slot's own copy of this batch)
            slot = Slot(g, m, self.model._cfg.kind, self._dtype, weights=self.sample_weights)
        elif m is getattr(g, "meta", None):   # (the batch's own metadata: what Slot.load takes by itself)
            slot.load(g)
        else:                                 # (a batch object of another library, float64 drivers: no ``meta`` of its own)
            slot.load(g, m)
        loss = self._run_slot(slot, fp, extra, fresh)
        if fresh:                             # (registered once recorded: a failed first step leaves no empty recording behind)
            self._slots[key] = slot
        return loss

    def _dataset_program(self, ds, indices, n_global: Optional[int], n_max: Optional[int]) -> torch.Tensor:
        """A slotted ``step_dataset`` up to the optimizer: refuse, bump the seed, collate into the bucket, run the slot."""
        self._refuse("step_dataset", None)
        table = self._require_weight_table("step_dataset", ds)
        idx, N, E, n_max = ds.bucket_dims(indices, n_max)
        B = int(idx.shape[0])
        n_pad, e_pad = bucket_sizes(N, E, *self.bucket)
        fp, extra = self._context(None, ds, B, n_global)
        tiled = self._tiled
        key = self._key(n_pad, e_pad, B, n_max, extra, tiled)
        if table is not None:                 # another dataset's table: slots of its own, never a stale pointer
            key += (table.data_ptr(),)
        slot = self._lookup(key, allow_promote=True)
        fresh = slot is None
        if fresh:
            t = self._tables(ds)
            slot = Slot.empty(self.model._cfg.kind, fp.flat.device, self._dtype, B, n_pad, e_pad, n_max, int(t["x"].shape[1]),
                              int(t["edge"].shape[1]), int(t["target"].shape[1]), tiled=tiled, weight_table=table)
        ds.collate_into(slot.g, idx, slot.collate_scratch())
        slot._loaded = None                                        # (the static buffers now hold a batch no object stands for)
        slot.set_real_nodes(N)
        loss = self._run_slot(slot, fp, extra, fresh)
        if fresh:
            self._slots[key] = slot
        return loss

    # ---- the public step methods -----------------------------------------------------------------------------------------------
    def step(self, g, n_global: Optional[int] = None) -> torch.Tensor:
        """One training step on the batch ``g``: program, optimizer; returns the loss, a 0-dim device tensor.  ``n_global``: the
        crystals of the un-sharded batch under data parallelism (``train.Trainer(dist=...)``); the batch's own count otherwise."""
        self._ema_refuse("step")
        self._refuse("step", g)
        loss = self._batch_program(g, n_global)
        self.optimizer_step()
        return loss

    def step_dataset(self, ds, indices, n_global: Optional[int] = None, n_max: Optional[int] = None) -> torch.Tensor:
        """One training step on the crystals ``indices`` of a device-resident ``loader.DeviceDataset`` (for a float64 driver one
        with float64 tables: ``DeviceDataset(..., dtype=torch.float64)`` holds them without a copy).  Where the step is slotted
        (``train.Trainer``: ``replay`` or ``graph``; ``train64.Trainer64``: ``replay`` with ``bucket``) the batch is collated by
        ``dosx_collate_padded`` / ``dosx_collate_padded_f64`` STRAIGHT INTO the static buffers of its shape bucket (ghost padding
        included) and the bucket's recorded program is replayed (recorded on first use, or - ``promote`` - run in a live larger
        bucket) — no intermediate batch object, no padding ops, no slot copy: bitwise
        ``step(pad_batch(ds.collate(indices, n_max=n_max), *bucket_sizes(N, E, *bucket)))``.  Otherwise it is
        ``step(ds.collate(indices, n_max=n_max))`` (the counterpart of the loop body `main_phDOS.py:104-118` with a shuffling
        DataLoader).  ``n_max`` may exceed the selection's largest crystal, so that one value serves a whole dataset (with
        per-crystal keys and no dropout the numbers do not depend on it)."""
        self._ema_refuse("step_dataset")
        if not self._slotted(dataset=True):
            return self.step(ds.collate(indices, n_max=n_max), n_global)
        loss = self._dataset_program(ds, indices, n_global, n_max)
        self.optimizer_step()
        return loss

    # ---- gradient accumulation ---------------------------------------------------------------------
    def step_accumulate(self, batches) -> torch.Tensor:
        """ONE optimizer step on the objective of the concatenated batch, computed micro-batch by micro-batch: what a torch loop
        gets from ``backward()`` on several batches before one ``optimizer.step()`` - with every loss normalised by the window's
        crystal count ``T = sum B_k``, not by its own, so that ragged batches still give the mean over crystals.  Each batch
        runs its ordinary program (eager, ``replay`` or ``graph``; the slots an epoch recorded are reused, keyed with ``T``) and
        one ``dosx_grad_accumulate`` (``_f64``) launch behind it sums the flat gradients in the fixed order
        ``((G1 + G2) + G3) + ...``;
        then one guard verdict (on the SUM: a non-finite value in any micro-batch skips the whole window), one AdamW launch, one
        update of the weight average, ``step_count + 1``.  Returns the window's loss, a 0-dim device tensor (a trainer-owned
        scalar, valid until the next window); ``crystal_losses`` is the ``[T]`` concatenation in micro-batch order,
        ``last_outputs`` / ``program_stats()`` describe the last micro-batch, the dropout seed advances once per micro-batch.
        One batch is ``step()`` bit for bit.  Every objective that is a sum over crystals divided by a count: the eDOS default loss
        and every ``loss=``; the reference's pooled phonon RMSE is refused for more than one batch (``loss="crystal_rmse"`` is
        the reference's own batch-1 objective).  Not under data parallelism, not inside ``ema_weights()``.  Whatever can be known
        before a launch raises before anything has changed; an exception in the middle of a window leaves parameters, moments,
        average and ``step_count`` untouched."""
        batches = list(batches)
        self._window_checks("step_accumulate", len(batches))
        sizes = self._window_sizes("step_accumulate", (self._crystals_of(g) for g in batches))
        for g in batches:
            self._refuse("step_accumulate", g)
        if len(batches) == 1:
            return self.step(batches[0])

        return self._window("step_accumulate", sizes, lambda k: self._batch_program(batches[k], None))

    def step_dataset_accumulate(self, ds, index_lists, n_max: Optional[int] = None) -> torch.Tensor:
        """``step_accumulate`` on selections of a device-resident ``loader.DeviceDataset``: each ``indices`` of ``index_lists`` is
        collated straight into its bucket as ``step_dataset`` does; bitwise ``step_accumulate([ds.collate(i) ...])``."""
        index_lists = list(index_lists)
        self._window_checks("step_dataset_accumulate", len(index_lists))
        sizes = self._window_sizes("step_dataset_accumulate", (len(i) for i in index_lists))
        self._refuse("step_dataset_accumulate", None)
        if len(index_lists) == 1:
            return self.step_dataset(ds, index_lists[0], n_max=n_max)
        if not self._slotted(dataset=True):
            return self.step_accumulate([ds.collate(i, n_max=n_max) for i in index_lists])
        return self._window("step_dataset_accumulate", sizes, lambda k: self._dataset_program(ds, index_lists[k], None, n_max))
