"""Fused training step of the reference callers (`main_phDOS.py:101-118`, `main_eDOS.py:101-127`):
forward program -> loss kernel -> backward program -> (RCCL all-reduce) -> flat AdamW kernel.

No autograd graph, no per-parameter optimizer loop, no host synchronisation: the loss stays on the
device (the reference prints it every step, `main_eDOS.py:129`; read ``.item()`` only when needed).

``Trainer(replay=True)`` re-issues a RECORDED launch sequence (``ops.Program``): the first step on a shape
bucket runs normally while every libdosx call is recorded with its marshalled arguments on static
buffers; later steps copy the batch into the bucket's input buffers and replay the list — no Python
marshalling, no allocator, two real HIP streams (weight-gradient kernels overlap the dgrad chain).

``Trainer(graph=True)`` instead replays the step from captured HIP graphs: batches are padded
with ghost nodes / edges to a small set of (N, E) buckets (``batch.pad_batch`` — exact, not
approximate), every launch of the forward / loss / backward programs for a bucket is captured once,
and a step is then "copy the batch into the bucket's static buffers, replay, AdamW".  The ~160
launches of a step cost the host ~20 us each when issued from Python; replay removes that.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch

from . import _abi
from . import functional as Fn
from . import ops
from . import param_groups as _pg
from ._lib import DosxError, from_environ
from ._models import DOSTransformerBase, GraphnetworkBase, _SEED_MOD, rank_seed_offset
from .batch import CrystalBatch, bucket_sizes, graph_meta, pad_batch
from .ema import WeightEma
from .guard import StepGuard
from .slots import Slot, SlotCache

# Data parallel: a THIRD gradient bucket (GN_decoder + message-passing layers L-1 .. 1: 1.9 of the GNN trunk's 3.0 MB at the
# headline shape) all-reduced from the flush at layer 0, under layer 0's backward, so that only 1.1 MB stay behind the step
# (VERDICT r5 item 6).  Built, tested (tests/test_dp_gpu.py, tests/test_dp_gloo.py) - and OFF: on a 1-rank RCCL group the extra
# collective point costs 55 us per step (1.1118 -> 1.1667 ms, three interleaved rounds, tools/exp/r6_dp1.sh) - the communicator
# stream's wait for the weight-gradient stream lands in a hardware queue it shares with the main stream (more hardware queues,
# GPU_MAX_HW_QUEUES = 6 / 8, make the step 35 % slower: tools/exp/r6_dp2.sh) - while 1.9 MB less exposed traffic is worth about
# 15 us on 8 xGMI-connected GPUs.  To be re-measured on a real multi-GPU node.
_DP_MID_BUCKET = from_environ("DOSX_DP_MID_BUCKET", "0") == "1"
_DP_CHECK = from_environ("DOSX_DP_CHECK", "0") == "1"


class _AdamWState(StepGuard, WeightEma):
    """What Trainer and train64.Trainer64 share: the AdamW moments laid out like the model's flat parameters (in the flat
    buffer's dtype), their checkpoint in ``torch.optim.AdamW`` vocabulary, the per-step bump of the dropout seed and the
    gradient guard of the optimizer step (``guard.StepGuard``: ``max_grad_norm`` / ``skip_nonfinite``) and the exponential moving
    average of the weights the AdamW launch keeps (``ema.WeightEma``: ``ema_decay`` / ``ema_warmup``, re-homed by name with the
    moments).  Expects
    ``model``, ``_fp``, ``_m``, ``_v``, ``_slots``, ``step_count`` and the hyper-parameters ``lr``, ``betas``, ``eps``, ``wd``, ``beta``."""

    def _state(self, fp):
        """AdamW moments laid out like ``fp``.  When the parameters are re-homed (module moved to another device after
        ``load_state_dict``, a different dead-parameter set, ...) the moments follow BY NAME instead of being reset:
        ``step_count`` keeps counting, so zeroed moments would silently corrupt the bias correction."""
        if self._ema_block:                # (also what a freeze() / update_trainable() inside the block runs into)
            self._ema_refuse("_state (step, forward_backward, optimizer_step, state_dict, load_state_dict)")
        if self._fp is not fp:
            if getattr(self, "dist", None) is not None and fp.n_train != fp.total:
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

    # ---- parameter groups (param_groups.py; include/dosx.h: DosxAdamWGroups) -------------------------------------------
    _groups = None                    # None: one lr / weight_decay, the ungrouped launch; else [{"lr", "weight_decay", "names"}]
    _chunk_group = None               # uint8 device tensor, one entry per 64 elements of flat[:n_train], of the layout in _fp
    _groups_host = None               # the kernel's host struct, filled from _groups at every optimizer step

    def _init_param_groups(self, who: str, groups, dist=None) -> None:
        """``param_groups=`` of a trainer's constructor; call it once ``model``, ``lr`` and ``wd`` are set."""
        self._groups = self._chunk_group = self._groups_host = None
        if groups is None:
            return
        if dist is not None:
            raise DosxError(f"{who}(param_groups=...) is a single-GPU mode: not with dist (data parallelism)")
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

    def _init_loss(self, who: str, loss, huber_delta, dist=None) -> None:
        """``loss=`` / ``huber_delta=`` of a trainer's constructor.  Constructor arguments like ``beta``: not part of ``state_dict()``."""
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
        if loss is not None and dist is not None:
            raise DosxError(f"{who}(loss=...) is a single-GPU mode: not with dist (data parallelism)")
        self.loss, self.huber_delta = loss, None if huber_delta is None else float(huber_delta)

    def _loss_rows(self, alloc, dev, pg, ps, y, clamp: bool, dpg, dps, B_global: Optional[int] = None, weights=(None, None)):
        """The one launch site of the per-crystal losses: -> (per-crystal l_b [B], loss 0-dim), both on static buffers when
        the step is being recorded.  ``ps = dps = None``: a one-output model (``beta`` is not read then).  ``B_global``: the
        count the mean is taken over - the batch's own outside an accumulation window, the window's total inside one.
        ``weights``: what ``_batch_weights`` returned for the batch; with them or with ``bin_weights=`` the weighted entry."""
        B = int(pg.shape[0])
        if B_global is None:
            B_global = B if self._window_total is None else self._window_total
        per, loss = alloc(dev, B), alloc(dev, 1)
        fn = ops.loss_rows if pg.dtype == torch.float32 else ops.loss_rows64
        fn(pg, ps, y, self.loss, clamp_target=clamp, beta=self.beta, delta=self.huber_delta, dpg=dpg, dps=dps, per_crystal=per,
           loss=loss, B_global=int(B_global), weights=weights[0], weight_index=weights[1],
           bin_weights=self._bin_operand(dev, pg.dtype))
        return per, loss[0]

    # ---- sample weights and energy-bin weights (include/dosx.h: dosx_loss_rows_w / dosx_loss_rows_w_f64) --------
    sample_weights = False            # True: every batch carries a [B] field `weight`, step_dataset reads the dataset's table
    bin_weights = None                # None, or the [S] energy-bin weights as given (float64, on the host)
    _bin_dev = None                   # ... on the device in the program's dtype, moved there once

    def _init_weights(self, who: str, sample_weights, bin_weights, dist=None) -> None:
        """``sample_weights=`` / ``bin_weights=`` of a trainer's constructor; call it after ``_init_loss``.  Constructor arguments
        like ``beta`` and ``loss``: not part of ``state_dict()``."""
        self.sample_weights, self.bin_weights, self._bin_dev = bool(sample_weights), None, None
        if not self.sample_weights and bin_weights is None:
            return
        what = " and ".join(n for n, on in (("sample_weights=True", self.sample_weights), ("bin_weights=...", bin_weights is not None)) if on)
        if dist is not None:
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

    def _bin_operand(self, dev, dtype):
        if self.bin_weights is None:
            return None
        if self._bin_dev is None or self._bin_dev.device != dev or self._bin_dev.dtype != dtype:
            if self._bin_dev is not None:      # (the module moved: the recordings hold the old buffer's address)
                self._slots = OrderedDict()
            self._bin_dev = self.bin_weights.to(dev, dtype).contiguous()
        return self._bin_dev

    def _require_weight(self, what: str, g) -> None:
        """``sample_weights=True``: the batch must carry ``weight`` - raised before anything is launched."""
        if self.sample_weights and not (hasattr(g, "weight") and torch.is_tensor(g.weight) and g.weight.is_floating_point()
                                        and g.weight.numel() == self._crystals_of(g)):
            raise ValueError(f"{self._ema_who}.{what}: sample_weights=True, but the batch has no floating-point graph-level field "
                             f"`weight` of [B] = [{self._crystals_of(g)}] entries (DeviceDataset crystals with a \"weight\", or "
                             f"g.weight = ...)")

    def _require_weight_table(self, what: str, ds, tables):
        """``sample_weights=True``: the dataset's resident weight table in the program's dtype, or the refusal."""
        if not self.sample_weights:
            return None
        w = tables.get("weight")
        if w is None:
            raise ValueError(f"{self._ema_who}.{what}: sample_weights=True, but the dataset holds no weights (crystals with a "
                             f"\"weight\", or ds.set_weights(w))")
        return w

    def _batch_weights(self, g, cast):
        """(w, w_index) of batch ``g`` for ``_loss_rows``: ``g.weight`` converted as the target is (``cast``; a slot's static
        buffer comes back as it is), with ``g.weight_index`` where a dataset step left its table and the bucket's selection."""
        if not self.sample_weights:
            return (None, None)
        wi = getattr(g, "weight_index", None)
        if wi is None:
            self._require_weight("step", g)
        return (cast(g.weight).reshape(-1), wi)

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
    _window_total = None              # inside a window: T, the crystals of all its micro-batches; None outside

    def _window_checks(self, what: str, K: int) -> None:
        """What a window cannot run on and that its length alone decides - raised before the dropout seed, the accumulator or
        any slot is touched."""
        who = self._ema_who
        self._ema_refuse(what)
        if K == 0:
            raise ValueError(f"{who}.{what}: an empty window - pass at least one batch")
        if getattr(self, "dist", None) is not None:
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
                raise ValueError(f"{self._ema_who}.{what}: batch {k} of the window is empty")
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
        accumulate = None
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
                    accumulate = ops.grad_accumulate if fp.flat.dtype == torch.float32 else ops.grad_accumulate64
                    accumulate(self._acc, fp.grad, None, fp.n_train, sdst=self._acc_loss, sa=loss)
                elif fp is not fp0:
                    raise DosxError(f"{self._ema_who}.{what}: the flat parameters were laid out anew inside a window (batch {k})")
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


class _Width:
    """Stands in for a batch where only the node-feature width matters (FusedModel._extra_dead reads ``g.x.shape[1]``)."""

    def __init__(self, width: int):
        self.x = torch.empty(0, int(width))


class Trainer(_AdamWState, SlotCache):
    """AdamW(lr, weight_decay=1e-2) training of a DOSTransformer(_phonon) module, all on libdosx.

    ``dist``: optional :class:`dostransformer_amd.dist.DataParallel` — shards are per-rank batches,
    gradients are summed over ranks (loss kernels already divide by the GLOBAL element/crystal
    count), the phonon loss exchanges its two SSE scalars before the backward pass.

    ``per_crystal_keys=True`` (same spelling as :class:`dostransformer_amd.predict.Predictor`): ``transformer`` and
    ``transformer_source`` attend over each crystal's own atoms, forward and backward, instead of the rows that pad it to the
    batch's largest crystal - the step then learns what the reference computes at ``batch_size = 1``, where it trains the
    phonon model and evaluates both (`main_phDOS.py:52-55`, `main_eDOS.py:55-56`); for eDOS the phantom node counts as an atom, as
    it does there.  Eager, ``replay=True`` and ``graph=True`` alike (the bucket's own ``graph_ptr`` is the operand).  The switch does
    not touch the loss: the default phonon loss is still ONE RMSE pooled over the batch, whose gradient is not the mean of the
    batch-1 gradients - ``loss="crystal_rmse"`` is the objective that matches batch-1 training.  Not under data parallelism.

    The GNN-only baselines - ``Graphnetwork``, ``Graphnetwork_phonon`` (fp32 parameters) and ``embedder_eDOS.mlp.mlp`` - train through
    the same step (eager, ``replay=True``, ``graph=True``, ``step_dataset``, checkpoints) with their output head on its rank
    structure (``functional.graphnetwork_fwd(factored_head=True)``) and the drivers' loss on their ONE output: phonon
    ``sqrt(mean_all (dos - y)^2)`` (`main_phDOS.py:109-111`), eDOS ``mean_b sqrt(mean_s (dos - max(y, 0))^2)`` (`main_eDOS.py:111-118`).
    With one output there is no ``beta`` to weigh (anything but 1.0 is refused), no attention to give per-crystal keys, and no
    data parallelism yet; ``n_global`` must be the batch's own count.  Which node encoder is dead follows the input width and is
    fixed by the first batch: a later batch of the other width is refused.

    ``max_grad_norm=X`` / ``skip_nonfinite=True`` put the optimizer step behind a gradient guard (``guard.StepGuard``): what
    ``torch.nn.utils.clip_grad_norm_(params, X)`` between ``backward()`` and ``optimizer.step()`` and a GradScaler-style "skip
    if non-finite" do, decided on the device - one statistics launch over the flat gradient and an AdamW that reads the
    verdict, no host read.  A step whose gradient holds a NaN / inf (or that follows a reported exchange stall) leaves
    parameters and moments untouched and does not advance AdamW's time; ``grad_norm`` / ``guard_report()`` say what happened,
    ``check()`` raises.  Every mode; not under data parallelism.  Off by default: the step then issues exactly the launches it issued without these arguments.

    Fine-tuning: ``requires_grad`` decides which parameters train (``model.freeze(...)`` / ``model.train_only(...)``, or the flags
    themselves followed by ``model.update_trainable()``).  A frozen parameter and its two moments are bitwise untouched by a step,
    weight decay included - torch's behaviour for ``grad is None`` - and the guard's norm covers the trainable gradient only.  The
    flags are read when the flat buffer is laid out, never per step; the backward program drops the weight-gradient jobs of frozen
    Linears, ends in front of a frozen GNN trunk (and a frozen first encoder), and runs a cross attention over frozen keys without
    its key gradient (functional.wgrad_needed / trunk_cut / first_encoder_cut / attention_query_only); ``program_stats()`` shows
    what is left.  Every model and mode; not under data parallelism.  With nothing frozen the layout, the launches and the bits
    are what they were.

    ``param_groups=[{"params": prefix | [prefixes], "lr": ..., "weight_decay": ...}]``: ``torch.optim.AdamW``'s parameter groups
    with name prefixes for tensors (``param_groups.py``: ``resolve``, ``no_decay``, ``layerwise``) - still ONE flat AdamW launch,
    which looks decay and step size up per 64-element chunk of the flat buffer; bit for bit the ungrouped kernel applied tensor by
    tensor with each tensor's values.  ``trainer.param_groups`` is read at every step: assigning ``["lr"]`` is a schedule.  With
    the guard, with frozen parameters, every mode; not under data parallelism.  None (the default): the launch it always was.

    ``ema_decay=d`` (``ema_warmup=True``): the AdamW launch also keeps an exponential moving average of the weights
    (``ema.WeightEma``; ``ema' = ema + (p' - ema)(1 - d_t)``, ``d_t = min(d, (1 + t) / (10 + t))`` under warm-up) - a step the guard
    skips leaves it alone.  ``with trainer.ema_weights():`` evaluates under it, ``trainer.ema_state_dict()`` exports it,
    ``state_dict()`` carries it.  Every mode, with the guard, frozen parameters and groups; not under data parallelism.  None
    (the default): the launch and the checkpoint it always was.

    ``loss="crystal_rmse" | "mse" | "mae" | "huber"`` (``huber_delta=X`` with the last, and only with it) replaces the driver's loss
    by the mean over crystals of each crystal's own RMSE, MSE, MAE or ``torch.nn.HuberLoss(delta=X)`` term, ``f(dos_global) + beta
    f(dos_system)`` for the two-output models - one entry, ``dosx_loss_rows`` (csrc/loss_rows.hip), in place of the loss launches;
    eDOS models keep their target clamp.  ``"crystal_rmse"`` is the reference's phonon objective at its ``batch_size = 1`` (with
    ``per_crystal_keys=True`` a step on B crystals follows the mean of the B batch-1 gradients); on an eDOS model it is the default
    objective and trains the same bits.  ``trainer.crystal_losses`` is then the last step's per-crystal losses, a ``[B]`` device
    tensor (under replay a view of the bucket's static buffer) valid until the next step.  Every mode, with the guard, frozen
    parameters, groups and the average; ``n_global`` must be the batch's own count; not under data parallelism.  A constructor
    argument like ``beta``: not in ``state_dict()``.  None (the default): the reference's loss, the launches it always issued.

    ``step_accumulate([g1, g2, ...])`` / ``step_dataset_accumulate(ds, [idx1, idx2, ...])``: gradient accumulation - ONE optimizer
    step on the objective of the concatenated batch, every micro-batch through its ordinary program with the loss divided by the
    window's crystal count, one ``dosx_grad_accumulate`` launch behind each (see ``step_accumulate``).  ``step`` and
    ``step_dataset`` issue the launches they always issued.

    ``sample_weights=True`` / ``bin_weights=[S]`` (with one of the four ``loss=`` kinds): torch's ``(w * per_sample_loss).mean()`` -
    ``loss = sum_b w_b l_b / B`` with the per-crystal terms ``sum_s v_s e(r) / sum_s v_s`` under energy-bin weights ``v`` - through
    ``dosx_loss_rows_w`` in place of ``dosx_loss_rows``, no other launch.  ``step(g)`` reads the batch's ``[B]`` field
    ``g.weight``; ``step_dataset`` hands the kernel the dataset's resident table (``DeviceDataset.set_weights``: checked on the
    host once, written in place, read at every step) and the bucket's selection, and the launch gathers.  All-ones weights train
    the unweighted bits; a weight of exactly 0 takes a crystal out whatever it holds (a NaN target included: the guard does not
    trip); ``crystal_losses`` stay the crystals' own unweighted losses.  Every mode, windows, the guard, frozen parameters, groups
    and the average; constructor arguments like ``loss``: not in ``state_dict()``; not under data parallelism.
    """

    def __init__(self, model: DOSTransformerBase, lr: float = 1e-4, beta: float = 1.0, weight_decay: float = 1e-2,
                 betas=(0.9, 0.999), eps: float = 1e-8, dist=None, graph: bool = False, replay: bool = False,
                 bucket=(8, 128), max_slots: int = 32, promote: float = 0.0, per_crystal_keys: bool = False,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, param_groups=None,
                 ema_decay: Optional[float] = None, ema_warmup: bool = True, loss: Optional[str] = None,
                 huber_delta: Optional[float] = None, sample_weights: bool = False, bin_weights=None):
        if not isinstance(model, (DOSTransformerBase, GraphnetworkBase)):
            raise TypeError("Trainer drives DOSTransformer / DOSTransformer_phonon / Graphnetwork / Graphnetwork_phonon / mlp modules")
        model._require_fp32_program("Trainer")
        self._baseline = isinstance(model, GraphnetworkBase)
        self._dead = None                 # baselines: the dead-parameter set of the first batch's input width
        if self._baseline:
            name = type(model).__name__
            if float(beta) != 1.0:
                raise ValueError(f"Trainer({name}): beta={beta} - the model has ONE output and its loss no second term to weigh; "
                                 f"only the default 1.0 is accepted")
            if per_crystal_keys:
                raise DosxError(f"Trainer({name}, per_crystal_keys=True): the model has no attention - a crystal's output "
                                f"never depends on its batch mates")
            if dist is not None:
                raise DosxError(f"Trainer({name}, dist=...): data parallelism is not implemented for the GNN-only baselines")
        if per_crystal_keys and dist is not None:
            raise DosxError("Trainer(per_crystal_keys=True) is a single-GPU mode: not with dist (data parallelism)")
        if dist is not None and len(model.trainable_names()) != len(model._live_named()):
            raise DosxError("Trainer(dist=...) with frozen parameters: fine-tuning is a single-GPU mode, not with dist (data "
                            "parallelism)")
        self._per_crystal_keys = bool(per_crystal_keys)
        self._init_guard("Trainer", max_grad_norm, skip_nonfinite, dist)
        self.model, self.lr, self.beta, self.wd, self.betas, self.eps = model, lr, beta, weight_decay, betas, eps
        self._init_param_groups("Trainer", param_groups, dist)
        self._init_ema("Trainer", ema_decay, ema_warmup, dist)
        self._init_loss("Trainer", loss, huber_delta, dist)
        self._init_weights("Trainer", sample_weights, bin_weights, dist)
        self.dist = dist
        self.graph = graph
        self.replay = replay
        # (node, edge) granularity of the shape buckets unpadded batches are ghost-padded to in graph / replay mode: a
        # coarser grid means fewer distinct launch lists to record when batches are reshuffled every epoch
        self.bucket = tuple(bucket)
        self.bucketed = dist is not None and not graph       # early-bucket overlap (eager and replay modes)
        self._early_work = None
        self._mid_work = None
        self._early_side = None
        self._rec_parts = []
        self.step_count = 0
        self._m = self._v = None
        self._fp = None
        self.kind = model._cfg.kind
        self.last_outputs = None
        # shape buckets seen so far -> static buffers + recorded program, least recently used first; bounded: with
        # per-epoch shuffling new (N, E) buckets keep appearing, each holding a step's worth of activations
        self._slots: "OrderedDict[tuple, Slot]" = OrderedDict()
        self.max_slots = int(max_slots)
        self.slot_hits = self.slot_misses = self.slot_promoted = 0
        # largest relative excess of nodes / edges a first-time bucket accepts from a live one (step_dataset; 0 = every
        # bucket records its own launch list: bitwise the step on the batch padded to its own bucket)
        self.promote = float(promote)
        self._seen = {}
        self.kernel_timer = None          # ops._KernelTimer: replayed programs then run through dosx_replay_timed
        self._ds_checked = []             # datasets whose per-rank size was compared across the ranks (step_dataset)

    @property
    def per_crystal_keys(self) -> bool:
        """True: the two cross attentions attend over each crystal's own atoms (fixed at construction)."""
        return self._per_crystal_keys

    # ---- the step, split where the data-parallel collectives go --------------------------------
    def _part_a(self, fp, g, m, st_n_global: Optional[int] = None):
        """forward program (+ the phonon SSE pair).  Returns the state part B needs.  st_n_global: crystals in the un-sharded
        batch (None: this batch is the whole batch)."""
        if st_n_global is None:
            st_n_global = m.num_graphs
        model, dev, cfg = self.model, fp.flat.device, self.model._cfg
        B, S = m.num_graphs, cfg.S
        self._require_whole_batch(B, st_n_global)
        w = self._batch_weights(g, Fn._f32)          # (refuses a batch without `weight` before anything is launched)
        if self._baseline:
            out = model._program_fwd(fp.P, g, m, factored_head=True)
            y = Fn._f32(g.phdos).reshape(B, S) if self.kind == "phonon" else Fn._f32(g.y_ft).reshape(-1)
            return {"ctx": out[-1], "dos": out[0], "out": out[:-1] if model._returns_x else out[0], "B": B, "S": S, "y": y, "w": w}
        dg, xL, ds, (ctx, dos) = model._program_fwd(fp.P, g, m, bump_seed=False,     # (step() bumps the dropout seed)
                                                    per_crystal_keys=self._per_crystal_keys)
        st = {"ctx": ctx, "dos": dos, "out": (dg, xL, ds), "B": B, "S": S, "w": w}
        if self.kind == "phonon":
            st["y"] = Fn._f32(g.phdos).reshape(B, S)
            if self.loss is not None:      # a per-crystal loss: one entry in _part_b, no SSE pair
                st["split_loss"] = False
                return st
            st["sse"] = Fn._empty(dev, 2)
            st["split_loss"] = self.dist is not None or int(st_n_global) != B
            if st["split_loss"]:           # two-phase loss: ranks exchange the SSE pair in between, and / or the loss is
                ops.sse2(dos[:B], dos[B:], st["y"], st["sse"], B * S)      # normalised by a GLOBAL count that is not B
        else:
            st["y"] = Fn._f32(g.y_ft).reshape(-1)
        return st

    def _part_b(self, fp, m, st, n_global: int):
        """loss gradient + backward program.  n_global: crystals in the un-sharded batch."""
        dev, cfg = fp.flat.device, self.model._cfg
        B, S, dos = st["B"], st["S"], st["dos"]
        if self._baseline:
            return self._part_b_baseline(fp, m, st, n_global)
        ddos = Fn._empty(dev, *dos.shape)
        if self.loss is not None:          # eDOS clamps its target at 0 (main_eDOS.py:113), phonon does not; n_global == B (_part_a)
            st["crystal"], loss = self._loss_rows(Fn._empty, dev, dos[:B], dos[B:], st["y"], self.kind != "phonon", ddos[:B], ddos[B:],
                                                  B_global=n_global,         # ... or, inside a window, the window's total
                                                  weights=st["w"])
        elif self.kind == "phonon":
            loss = Fn._empty(dev, 1)
            if st["split_loss"] or int(n_global) != B:
                if not st["split_loss"]:
                    raise RuntimeError("n_global differs between the two halves of the step")
                ops.loss_phonon_bwd(dos[:B], dos[B:], st["y"], st["sse"], self.beta, float(n_global * S), ddos[:B],
                                    ddos[B:], loss, B * S)
            else:                          # one launch: SSE pair, loss and gradient (normalised by B*S: n_global == B)
                ops.loss_phonon(dos[:B], dos[B:], st["y"], st["sse"], self.beta, ddos[:B], ddos[B:], loss, B * S)
            loss = loss[0]
        else:
            lp = Fn._empty(dev, B + 1)
            ops.loss_edos(dos[:B], dos[B:], st["y"], self.beta, B, S, n_global, ddos[:B], ddos[B:], lp)
            ops.sum_to(lp, B, lp[B:])
            loss = lp[B]
        sink = ops.GradSink(dev)
        sink.gnn_hook = self._gnn_hook(fp)          # (functional.gnn_bwd calls it behind the flush that completes layers L-1 .. 1)
        Fn.dostransformer_bwd(fp.P, fp.G, cfg, m, st["ctx"], ddos, None, sink, mid_hook=self._mid_hook(fp))
        self._wgrad_keys = sink.wgrad_keys
        sink.release()
        return loss

    def _part_b_baseline(self, fp, m, st, n_global: int):
        """One-output loss + backward program of a GNN-only baseline.  The loss entries in their one-output use (include/dosx.h:
        ps = pg, beta = 0: the loss is rmse(pg) exactly, the second gradient goes to scratch); with ``loss=...`` the per-crystal
        entry in its own one-output form (ps == NULL)."""
        dev = fp.flat.device
        B, S, dos = st["B"], st["S"], st["dos"]
        if not self._whole_or_window(B, n_global):
            raise ValueError(f"Trainer({type(self.model).__name__}): n_global={n_global} but the batch holds {B} crystals "
                             f"(no data parallelism for the GNN-only baselines)")
        if self.loss is not None:          # the one-output form of the entry: no second gradient, no scratch
            ddos = Fn._empty(dev, B, S)
            st["crystal"], loss = self._loss_rows(Fn._empty, dev, dos, None, st["y"], self.kind != "phonon", ddos, None,
                                                  B_global=n_global, weights=st["w"])
            return self._bwd_baseline(fp, m, st, ddos, loss)
        ddos, scr = Fn._empty(dev, B, S), Fn._empty(dev, B, S)
        if self.kind == "phonon":
            loss = Fn._empty(dev, 1)
            ops.loss_phonon(dos, dos, st["y"], None, 0.0, ddos, scr, loss, B * S)
            loss = loss[0]
        else:
            lp = Fn._empty(dev, B + 1)
            ops.loss_edos(dos, dos, st["y"], 0.0, B, S, int(n_global), ddos, scr, lp)     # (B, or a window's total)
            ops.sum_to(lp, B, lp[B:])
            loss = lp[B]
        return self._bwd_baseline(fp, m, st, ddos, loss)

    def _bwd_baseline(self, fp, m, st, ddos, loss):
        sink = ops.GradSink(fp.flat.device)
        self.model._bwd_fn(fp.P, fp.G, self.model._cfg, m, st["ctx"], ddos, None, sink, factored_head=True)
        self._wgrad_keys = sink.wgrad_keys
        sink.release()
        return loss

    def _flat_for(self, dev, g, width: Optional[int] = None):
        """The model's flat parameters for a batch (or, step_dataset, an input width).  Baselines: which node encoder is dead
        follows the width; the first batch fixes it for this trainer."""
        model = self.model
        if not self._baseline:
            return model._ensure_flat(dev, g)
        if g is None:
            g = _Width(width)
        dead = model._extra_dead(g)
        if self._dead is None:
            self._dead = dead
        elif dead != self._dead:
            raise DosxError(f"Trainer({type(model).__name__}): this batch has node features of width {g.x.shape[1]}, which selects "
                            f"the other node encoder than the trainer's first batch did - its dead-parameter set (and the "
                            f"optimizer's layout) is fixed by the first batch")
        return model._ensure_flat(dev, g)

    # ---- data parallel: early gradient bucket ------------------------------------------------------
    def _mid_hook(self, fp):
        """Backward reaches the GNN trunk: reduce the early bucket's slabs on the side stream and start its
        all-reduce there, underneath the GNN backward (xGMI traffic overlaps compute; only the GNN bucket's
        all-reduce stays exposed at the end of the step)."""
        if self.dist is None:
            # single GPU: the early bucket's weight gradients + slab reduction run HERE (replay: on the side stream,
            # underneath the GNN backward; eager: inline), while their operands are still in L2 - not at the tail
            return lambda sink: sink.flush_on_side()
        if not self.bucketed or fp.n_late <= 0 or fp.n_late >= fp.total:
            return None

        def hook(sink):
            sink.flush_on_side()
            rec = ops.RECORDER.active
            if rec:                                   # the collective is not a libdosx call: split the recording
                self._rec_parts.append((ops.RECORDER.end(), "early"))
            self._start_early(fp, sink.wside)
            if rec:
                ops.RECORDER.begin()
        return hook

    def _gnn_hook(self, fp):
        """Backward reaches message-passing layer 0 and the weight-gradient group of the layers behind it has been flushed
        (functional.gnn_bwd): the MID bucket - GN_decoder + layers L-1 .. 1, two thirds of the GNN trunk's gradient bytes - is
        final, so its all-reduce starts on the gradient stream NOW, underneath layer 0's backward, the encoders' backward and the
        last weight-gradient group; only the last bucket (encoders + layer 0) is reduced behind the step."""
        if self.dist is None or not self.bucketed or not (0 < fp.n_late < fp.total) or not (0 < fp.n_last < fp.n_late) or not _DP_MID_BUCKET:
            return None

        def hook(sink):
            rec = ops.RECORDER.active
            if rec:
                self._rec_parts.append((ops.RECORDER.end(), "mid"))
            self._start_mid(fp, sink.wside)
            if rec:
                ops.RECORDER.begin()
        return hook

    def _start_early(self, fp, side) -> None:
        stream = side if side is not None else torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            self._early_work = self.dist.all_reduce_grads_async(fp.grad[fp.n_late:])
        self._early_side = side

    def _start_mid(self, fp, side) -> None:
        stream = side if side is not None else torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            self._mid_work = self.dist.all_reduce_grads_async(fp.grad[fp.n_last:fp.n_late])

    def _n_global(self, B: int, n_global: Optional[int], g=None) -> int:
        """Crystals in the un-sharded batch: the caller's value, else what the sharder recorded on the batch
        (``dist.shard_batch``), else — last resort, a blocking collective + host read — the sum over ranks."""
        if n_global is not None:
            return int(n_global)
        ng = getattr(g, "n_global", None) if g is not None else None
        if ng is not None:
            return int(ng)
        return self.dist.global_count(B) if self.dist is not None else B

    # ---- eager path ------------------------------------------------------------------------------
    def forward_backward(self, g, n_global: Optional[int] = None, _bump: bool = True) -> torch.Tensor:
        """Forward + loss + backward; leaves the gradients in the flat buffer.  Returns the loss
        (0-dim device tensor; for eDOS under data parallelism it is this rank's share)."""
        self._ema_refuse("forward_backward")
        if _bump:                      # a direct forward_backward() + optimizer_step() loop draws fresh dropout masks too
            self._bump_dropout_seed()
        model = self.model
        dev = model._module_device()
        model._require_fp32_program("Trainer")
        fp = self._flat_for(dev, g)
        self._state(fp)
        m = graph_meta(g, dev)
        ng = self._n_global(m.num_graphs, n_global, g)
        with torch.no_grad(), ops.call_log() as names:
            st = self._part_a(fp, g, m, ng)
            self.last_outputs = st["out"]
            if self.kind == "phonon" and self.dist is not None:
                self.dist.all_reduce_sse(st["sse"])
            loss = self._part_b(fp, m, st, ng)
        self._stats = self._make_stats(names)
        self.crystal_losses = st.get("crystal")
        return loss

    # ---- graph path ------------------------------------------------------------------------------
    def _capture(self, slot: Slot, fp, ng: int) -> None:
        g, m = slot.g, slot.g.meta
        split = self.dist is not None and self.kind == "phonon"
        with ops.recording_scope(), torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                       # eager warm-up (lazy kernel attributes etc.)
                st = self._part_a(fp, g, m, ng)
                self._part_b(fp, m, st, ng)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            slot.graph_a = torch.cuda.CUDAGraph()
            with ops.call_log() as names:
                with torch.cuda.graph(slot.graph_a):
                    st = self._part_a(fp, g, m, ng)
                    if not split:
                        loss = self._part_b(fp, m, st, ng)
                if split:
                    slot.graph_b = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(slot.graph_b, pool=slot.graph_a.pool()):
                        loss = self._part_b(fp, m, st, ng)
        slot.stats = self._make_stats(names)
        slot.keep = (st, loss)            # keeps the graph-owned outputs from being recycled
        slot.loss, slot.out, slot.sse, slot.crystal = loss, st["out"], st.get("sse"), st.get("crystal")

    def _record(self, slot: Slot, fp, ng: int) -> None:
        """Run the step once on the slot's static buffers while recording every launch."""
        g, m = slot.g, slot.g.meta
        split = self.dist is not None and self.kind == "phonon"
        # (replay is cheap enough on the host to feed two streams)
        with ops.recording_scope(side_stream=True), torch.no_grad():
            # the plan of a replayed step: recorded programs separated by the collectives (which are not
            # libdosx calls): [fwd] (sse) [bwd up to the GNN] (early bucket all-reduce) [GNN bwd]
            plan = []
            self._rec_parts = []
            ops.RECORDER.begin()
            st = self._part_a(fp, g, m, ng)
            if split:
                plan.append(("prog", ops.RECORDER.end()))
                plan.append(("sse", None))
                self.dist.all_reduce_sse(st["sse"])
                ops.RECORDER.begin()
            loss = self._part_b(fp, m, st, ng)
            last = ops.RECORDER.end()
            for part, coll in self._rec_parts:    # (_mid_hook / _gnn_hook closed these while recording)
                plan.append(("prog", part))
                plan.append((coll, None))
            plan.append(("prog", last))
            self._rec_parts = []
        slot.plan, slot.prog = plan, plan[0][1]
        slot.stats = self._make_stats([fn.__name__ for kind, prog in plan if kind == "prog" for fn, _ in prog.prog])
        slot.keep = (st, loss)
        slot.loss, slot.out, slot.sse, slot.crystal = loss, st["out"], st.get("sse"), st.get("crystal")

    def _run_slot(self, slot: Slot, fp, ng: int, fresh: bool) -> torch.Tensor:
        """The step on a bucket whose static buffers hold the batch: record / capture on first use, replay afterwards."""
        if fresh and self.replay:
            self._record(slot, fp, ng)       # this IS the step for this batch (run + record)
            self.last_outputs, self._stats, self.crystal_losses = slot.out, slot.stats, slot.crystal
            return slot.loss
        if fresh:
            self._capture(slot, fp, ng)
        self._stats = getattr(slot, "stats", None)
        if self.replay:
            for kind, prog in slot.plan:
                if kind == "prog":
                    if self.kernel_timer is not None:      # bench.py: event pair around every replayed launch
                        prog.run_timed(self.kernel_timer)
                    else:
                        prog.run()
                elif kind == "sse":
                    self.dist.all_reduce_sse(slot.sse)
                elif kind == "mid":
                    self._start_mid(fp, ops.GradSink.grad_stream(fp.flat.device))
                else:
                    self._start_early(fp, ops.GradSink.grad_stream(fp.flat.device))
        else:
            slot.graph_a.replay()
            if slot.graph_b is not None:
                self.dist.all_reduce_sse(slot.sse)
                slot.graph_b.replay()
        self.last_outputs, self.crystal_losses = slot.out, slot.crystal
        return slot.loss

    def _graph_step(self, g: CrystalBatch, n_global: Optional[int]) -> torch.Tensor:
        model = self.model
        dev = model._module_device()
        model._require_fp32_program("Trainer")
        fp = self._flat_for(dev, g)
        self._state(fp)
        m = g.meta
        if m is None or m.edge_perm is not None:
            raise ValueError("graph mode needs batches from collate(sort_edges=True) (+ pad_batch)")
        if getattr(g, "real_nodes", None) is None:               # not padded yet: pad on the fly
            g = pad_batch(g, *bucket_sizes(m.num_nodes, m.num_edges, *self.bucket))
            m = g.meta
        ng = self._n_global(m.num_graphs, n_global, g)
        self._require_whole_batch(m.num_graphs, ng)              # (before a slot is made, not inside its recording)
        self._require_weight("step", g)
        key = (m.num_nodes, m.num_edges, m.num_graphs, m.n_max, ng, m.seg_tile is not None)
        if self.sample_weights:               # (the last field of a dataset step's key is its table: this batch brings its own)
            key += (None,)
        slot = self._lookup(key)
        fresh = slot is None
        if fresh:                             # (graph mode captures on the slot's own copy of this batch)
            slot = Slot(g, m, self.kind, torch.float32, weights=self.sample_weights)
        else:
            slot.load(g)
        loss = self._run_slot(slot, fp, ng, fresh)
        if fresh:                             # (registered once recorded: a failed first step leaves no empty recording behind)
            self._slots[key] = slot
        return loss

    def step_dataset(self, ds, indices, n_global: Optional[int] = None, n_max: Optional[int] = None) -> torch.Tensor:
        """One training step on the crystals ``indices`` of a device-resident ``loader.DeviceDataset``: the batch is
        collated by ``dosx_collate_padded`` STRAIGHT INTO the static buffers of its shape bucket (ghost padding
        included) and the bucket's recorded program is replayed — no intermediate batch object, no padding ops, no
        slot copy.  Same numbers as ``step(ds.collate(indices))`` (the counterpart of the loop body `main_phDOS.py:104-118`
        with a shuffling DataLoader)."""
        self._ema_refuse("step_dataset")
        if not (self.replay or self.graph):
            return self.step(ds.collate(indices, n_max=n_max), n_global)
        loss = self._dataset_program(ds, indices, n_global, n_max)
        self.optimizer_step()
        return loss

    def _dataset_program(self, ds, indices, n_global: Optional[int], n_max: Optional[int]) -> torch.Tensor:
        """``step_dataset`` (replay / graph mode) up to the optimizer: collate into the bucket, bump the seed, run the slot."""
        model = self.model
        dev = model._module_device()
        model._require_fp32_program("Trainer")
        table = self._require_weight_table("step_dataset", ds, ds._f32_tables())
        fp = self._flat_for(dev, None, int(ds._f32_tables()["x"].shape[1]))
        self._state(fp)
        idx, N, E, n_max = ds.bucket_dims(indices, n_max)
        B = int(idx.shape[0])
        n_pad, e_pad = bucket_sizes(N, E, *self.bucket)
        # No per-step collective and no host read: without an explicit n_global the ranks of a data-parallel job must draw
        # EQUALLY sized shards every step, then n_global = B * world.  That holds for every batch of an epoch, the last one
        # included, iff all ranks hold equally many crystals and cut them with the same batch size - checked ONCE per
        # dataset (one blocking min/max over ranks at its first step); ragged shards must pass the true n_global, or the
        # loss would be normalised by the wrong count (`main_phDOS.py:109-114` is ONE rmse over the un-sharded batch).
        # DOSX_DP_CHECK=1 cross-checks B itself across the ranks on every step (debugging; blocking).
        if n_global is not None:
            ng = int(n_global)
        elif self.dist is None:
            ng = B
        else:
            if not any(d is ds for d in self._ds_checked):
                lo, hi = self.dist.min_max(len(ds))
                if lo != hi:
                    raise ValueError(f"data-parallel ranks hold {lo}..{hi} crystals: with ragged shards the last batches of "
                                     f"an epoch differ in size across ranks - pass the global batch size as n_global")
                self._ds_checked.append(ds)
            if _DP_CHECK:
                lo, hi = self.dist.min_max(B)
                if lo != hi:
                    raise ValueError(f"ranks stepped on {lo}..{hi} crystals without an explicit n_global")
            ng = B * self.dist.world
        self._require_whole_batch(B, ng)
        tiled = True
        key = (n_pad, e_pad, B, n_max, ng, tiled)
        if table is not None:                 # another dataset's table: slots of its own, never a stale pointer
            key += (table.data_ptr(),)
        slot = self._lookup(key, allow_promote=True)
        fresh = slot is None
        if fresh:
            t = ds._f32_tables()
            slot = Slot.empty(self.kind, dev, torch.float32, B, n_pad, e_pad, n_max, int(t["x"].shape[1]),
                              int(t["edge"].shape[1]), int(t["target"].shape[1]), tiled=tiled, weight_table=table)
        ds.collate_into(slot.g, idx, slot.collate_scratch())
        slot._loaded = None                                        # (the static buffers now hold a batch no object stands for)
        self._bump_dropout_seed()
        loss = self._run_slot(slot, fp, ng, fresh)
        if fresh:
            self._slots[key] = slot
        return loss

    # ---- what the step launched ------------------------------------------------------------------
    def _make_stats(self, entries) -> dict:
        entries = list(entries)
        keys = list(getattr(self, "_wgrad_keys", ()))
        return {"launches": sum(1 for e in entries if e.startswith("dosx_")), "wgrad_jobs": len(keys), "entries": entries,
                "wgrad_keys": keys}

    def program_stats(self) -> dict:
        """What the last step's program (forward, loss, backward; not the optimizer) consisted of - of the recording when the step
        was replayed, of the capture when it ran from HIP graphs, else of the eagerly issued step itself: ``entries`` the names
        of its entries in issue order (a recorded program's ``Program.prog``: libdosx entry points plus the stream fork / join
        operations), ``launches`` how many of them are libdosx calls, ``wgrad_jobs`` how many weight-gradient jobs the backward
        deferred to its GradSink and ``wgrad_keys`` the weight each of them serves.  What a frozen set pruned shows here."""
        st = getattr(self, "_stats", None)
        if st is None:
            raise DosxError("program_stats: no step has run yet")
        return dict(st)

    # ---- optimizer -------------------------------------------------------------------------------
    def _reduce_gradients(self, fp) -> None:
        if self.dist is not None:
            if self._early_work is not None:          # early (+ mid) bucket already in flight: only the last bucket is exposed
                if self._mid_work is not None:
                    self.dist.all_reduce_grads(fp.grad[:fp.n_last])
                    self._mid_work.wait()
                    self._mid_work = None
                else:
                    self.dist.all_reduce_grads(fp.grad[:fp.n_late])
                self._early_work.wait()
                self._early_work = None
            else:
                assert self._mid_work is None
                self.dist.all_reduce_grads(fp.grad)

    def step(self, g, n_global: Optional[int] = None) -> torch.Tensor:
        self._ema_refuse("step")
        self._require_weight("step", g)
        self._bump_dropout_seed()
        loss = self._graph_step(g, n_global) if (self.graph or self.replay) else self.forward_backward(g, n_global, _bump=False)
        self.optimizer_step()
        return loss

    # ---- gradient accumulation ---------------------------------------------------------------------
    def step_accumulate(self, batches) -> torch.Tensor:
        """ONE optimizer step on the objective of the concatenated batch, computed micro-batch by micro-batch: what a torch loop
        gets from ``backward()`` on several batches before one ``optimizer.step()`` - with every loss normalised by the window's
        crystal count ``T = sum B_k``, not by its own, so that ragged batches still give the mean over crystals.  Each batch
        runs its ordinary program (eager, ``replay`` or ``graph``; the slots an epoch recorded are reused, keyed with ``T``) and
        one ``dosx_grad_accumulate`` launch behind it sums the flat gradients in the fixed order ``((G1 + G2) + G3) + ...``;
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
            self._require_weight("step_accumulate", g)
        if len(batches) == 1:
            return self.step(batches[0])
        T = sum(sizes)

        def run(k):
            self._bump_dropout_seed()
            if self.graph or self.replay:
                return self._graph_step(batches[k], T)
            return self.forward_backward(batches[k], T, _bump=False)
        return self._window("step_accumulate", sizes, run)

    def step_dataset_accumulate(self, ds, index_lists, n_max: Optional[int] = None) -> torch.Tensor:
        """``step_accumulate`` on selections of a device-resident ``loader.DeviceDataset``: each ``indices`` of ``index_lists`` is
        collated straight into its bucket as ``step_dataset`` does; bitwise ``step_accumulate([ds.collate(i) ...])``."""
        index_lists = list(index_lists)
        self._window_checks("step_dataset_accumulate", len(index_lists))
        sizes = self._window_sizes("step_dataset_accumulate", (len(i) for i in index_lists))
        if len(index_lists) == 1:
            return self.step_dataset(ds, index_lists[0], n_max=n_max)
        if not (self.replay or self.graph):
            return self.step_accumulate([ds.collate(i, n_max=n_max) for i in index_lists])
        T = sum(sizes)
        return self._window("step_dataset_accumulate", sizes, lambda k: self._dataset_program(ds, index_lists[k], T, n_max))
