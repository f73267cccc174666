"""Fused float64 training step of ``DOSTransformer_phonon`` (the phonon reference trains in float64, `main_phDOS.py:15-16,
101-118`): the float64 forward program -> float64 loss kernel -> float64 backward program into the flat gradient buffer ->
flat float64 AdamW kernel.  No autograd graph, no torch loss ops, no per-parameter optimizer loop, no host synchronisation.

``Trainer64(replay=True)`` re-issues a RECORDED launch sequence (``ops.Program``), as ``train.Trainer(replay=True)`` does for
the fp32 program: the first step on a batch shape runs normally on static buffers while every libdosx call is recorded;
later steps of that shape copy the batch into the buffers and replay the list from C.

Slots are keyed by the batch's EXACT shape (N, E, B, n_max) by default, and ghost-padded batches are refused.
``Trainer64(bucket=(node_step, edge_step))`` keys them by shape BUCKET instead, as the fp32 ``Trainer`` does: the float64
program is padding-safe (functional64), so an unpadded batch is ghost-padded (``batch.pad_batch`` - exact) to
``batch.bucket_sizes(N, E, *bucket)`` and every batch of a bucket replays one recording; without ``replay`` an already padded
batch is run as it is.  ``step_dataset(ds, indices)`` collates a selection of a device-resident float64
``loader.DeviceDataset`` straight into the bucket's static buffers (``dosx_collate_padded_f64``) - a shuffled epoch then
replays - and ``promote`` lets a bucket that is asked for the first time run in a slightly larger live one instead of
recording.  ``predict.Predictor64`` is the forward-only counterpart.

``GraphnetworkTrainer64`` is the same step for the GNN-only baseline ``Graphnetwork_phonon`` with float64 parameters (the
reference trains every phonon embedder in float64, `main_phDOS.py:15-16,70-72`): the factored float64 program
(``functional64.graphnetwork_phonon_fwd(factored_head=True)``), the loss entry on the model's one output, the flat AdamW.

Limits: single GPU (no ``dist``), no HIP-graph mode.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch

from . import functional64 as F64
from . import ops
from ._lib import DosxError
from ._models import DOSTransformerBase, GraphnetworkBase
from .batch import GraphMeta, graph_meta
from .slots import Slot
from .trainer_base import TrainerBase


class Trainer64(TrainerBase):
    """AdamW(lr, weight_decay=1e-2) training of a ``DOSTransformer_phonon`` set to the float64 program
    (``model.double().set_program_dtype(torch.float64)``), all on libdosx: what ``model(batch)`` -> torch loss ->
    ``loss.backward()`` -> ``torch.optim.AdamW`` computes, without autograd and the per-tensor optimizer.

    Per-crystal keys stay the module's own switch (``model.set_per_crystal_keys``): read at every step, and part of a
    recorded slot's key.  ``step(g)`` returns the loss as a 0-dim float64 device tensor; ``state_dict()`` /
    ``load_state_dict()`` use ``train.Trainer``'s vocabulary with float64 moments.  ``slot_hits`` / ``slot_misses`` count the
    replayed and the recorded steps of ``replay=True``; at most ``max_slots`` shapes stay recorded (least recently used out).

    ``bucket=None``: one slot per exact batch shape, ghost-padded batches are refused.  ``bucket=(node_step, edge_step)``: with
    ``replay`` an unpadded batch is ghost-padded to ``bucket_sizes(N, E, *bucket)`` (a batch that carries ``real_nodes`` is taken
    as it is) and slots are keyed by the padded shape; without ``replay`` a padded batch is run as it is and nothing is padded.
    ``promote``: the largest relative excess of node / edge rows at which ``step_dataset`` runs a bucket it sees for the first
    time in a live larger one instead of recording it (``slot_promoted`` counts those steps; 0: never).
    ``max_grad_norm`` / ``skip_nonfinite``: the optimizer step behind the gradient guard (``guard.StepGuard``), as on
    ``train.Trainer``: clipping and "skip if non-finite" decided on the device, ``grad_norm`` / ``guard_report()`` / ``check()``.
    ``param_groups``: per-group ``lr`` / ``weight_decay`` in the one flat float64 AdamW launch, as on ``train.Trainer``.
    ``ema_decay`` / ``ema_warmup``: a float64 exponential moving average of the weights kept by that launch, as on
    ``train.Trainer``: ``ema_weights()``, ``ema_state_dict()``, the ``ema`` keys of ``state_dict()``.
    ``loss`` / ``huber_delta``: a per-crystal objective in place of the pooled RMSE (``"crystal_rmse"``, ``"mse"``, ``"mae"``,
    ``"huber"``: ``dosx_loss_rows_f64``), as on ``train.Trainer``; ``crystal_losses`` is then the last step's ``[B]`` float64
    per-crystal losses.  With ``set_per_crystal_keys(True)`` a ``"crystal_rmse"`` step follows the mean of the reference's
    batch-1 gradients.  None (the default): the launches it always issued.
    ``step_accumulate`` / ``step_dataset_accumulate``: several micro-batches, one optimizer step on the objective of the
    concatenated batch, as on ``train.Trainer`` (needs ``loss=`` for more than one batch).
    ``sample_weights`` / ``bin_weights``: float64 per-crystal weights (the batch's ``weight`` field, or - ``step_dataset`` - the
    dataset's resident table gathered by the loss launch) and ``[S]`` energy-bin weights in the per-crystal loss
    (``dosx_loss_rows_w_f64``), as on ``train.Trainer``; they need ``loss=``.  With sample weights a slot's key ends in the table's
    address (``None`` for a batch-object slot).
    ``functionals`` / ``functional_kind`` / ``functional_weight``: a ``[K,S]`` table of linear functionals of the DOS penalised next
    to the pointwise term (``dosx_loss_rows_fn_f64``; with normalised rows ``dosx_loss_rows_fn_norm_desc_f64``),
    ``set_functionals(table)`` in place, as on ``train.Trainer``; they need ``loss=``.
    ``step(g, n_global=None)`` / ``step_dataset(ds, indices, n_global=None, n_max=None)`` are the drivers' shared methods
    (``trainer_base.TrainerBase``) and carry ``train.Trainer``'s ``n_global``: this driver is single-GPU and refuses any value
    but the batch's own count - pass ``n_max`` by keyword.
    """

    _who = "Trainer64"
    _dtype = torch.float64
    dist = None                   # single GPU

    def __init__(self, model, lr: float = 1e-4, beta: float = 1.0, weight_decay: float = 1e-2, betas=(0.9, 0.999),
                 eps: float = 1e-8, replay: bool = False, max_slots: int = 32, bucket=None, promote: float = 0.0,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, param_groups=None,
                 ema_decay: Optional[float] = None, ema_warmup: bool = True, loss: Optional[str] = None,
                 huber_delta: Optional[float] = None, sample_weights: bool = False, bin_weights=None,
                 functionals=None, functional_kind: str = "sq", functional_weight: float = 1.0):
        self._require_model(model)
        self._init_guard(max_grad_norm, skip_nonfinite)
        self.model, self.lr, self.beta, self.wd, self.betas, self.eps = model, lr, beta, weight_decay, tuple(betas), eps
        self._init_param_groups(param_groups)
        self._init_ema(ema_decay, ema_warmup)
        self._init_loss(loss, huber_delta)
        self._init_weights(sample_weights, bin_weights)
        self._init_functionals(functionals, functional_kind, functional_weight)
        self._crystal = None              # the per-crystal losses of the program just issued (loss=...), else None
        self.replay = bool(replay)
        self.max_slots = int(max_slots)
        if self.max_slots < 1:
            raise ValueError(f"Trainer64: max_slots must be at least 1, got {max_slots}")
        self.bucket = None if bucket is None else tuple(int(b) for b in bucket)
        if self.bucket is not None and (len(self.bucket) != 2 or min(self.bucket) < 1):
            raise ValueError(f"Trainer64: bucket is None or (node_step, edge_step), both at least 1, got {bucket}")
        self.promote = float(promote)
        if self.promote < 0.0:
            raise ValueError(f"Trainer64: promote must not be negative, got {promote}")
        self.step_count = 0
        self._m = self._v = self._fp = None
        self.last_outputs = None
        self._slots: "OrderedDict[tuple, Slot]" = OrderedDict()
        self.slot_hits = self.slot_misses = self.slot_promoted = 0
        self._seen = {}

    # ---- what the shared driver (trainer_base.TrainerBase) asks ----------------------------------------------------------------
    def _require_model(self, model) -> None:
        """The one model check of this driver - at construction and again in front of every step: a DOSTransformer_phonon set
        to the float64 program.  A subclass that drives another module overrides it."""
        DOSTransformerBase._require_f64_program(model, self._who)

    def _refuse(self, what: str, g) -> None:
        self._require_model(self.model)
        super()._refuse(what, g)
        if self.bucket is None and getattr(g, "real_nodes", None) is not None:
            raise DosxError(f"{self._who}: ghost-padded batches (batch.pad_batch) are refused without bucket=(node_step, "
                            "edge_step) - slots are keyed by the exact shape of an unpadded batch")

    def _slotted(self, dataset: bool) -> bool:
        return bool(self.replay and (self.bucket is not None or not dataset))

    def _prepare(self, g, ds, B: int, n_global: Optional[int]):
        """-> (flat parameters, the batch's own count).  Single GPU: any other ``n_global`` is refused."""
        if n_global is not None and not self._whole_or_window(B, n_global):
            raise ValueError(f"{self._who}: n_global={n_global} but the batch holds {B} crystals (a single-GPU driver: no data "
                             f"parallelism)")
        dev = self.model._module_device()
        fp = self._flat_for(dev, g, None if ds is None else int(ds._f64_tables()["x"].shape[1]))
        self._state(fp)
        return fp, B

    def _extra(self, fp, count: int):
        """The dropout operand: None in eval mode / p = 0, else (p, seed) - the first use makes the seed."""
        return self.model._dropout(fp.flat.device, False)

    def _key(self, n: int, e: int, B: int, n_max: int, drop, tiled: bool) -> tuple:
        """What decides the launch list: the (padded) shape, then per-crystal keys, dropout on / off (train / eval mode, p > 0),
        the tests' fp64-softmax switch, the loss weight and - last - the count the recorded loss launch divides by (the batch's
        own, or an accumulation window's total) - a slot recorded under one setting is never replayed under another.  (The
        message-GEMM tile table is the fp32 program's: ``tiled`` decides nothing here.)"""
        return (n, e, B, n_max, bool(self.model.per_crystal_keys), drop is not None, None if drop is None else drop[0],
                bool(F64.SOFTMAX64), float(self.beta), self._loss_count(B))

    def _slot_meta(self, g, dev):
        m = graph_meta(g, dev)
        if m.edge_perm is not None:
            raise ValueError(f"{self._who}(replay=True) needs batches with destination-sorted edges (collate(sort_edges=True))")
        return m

    # ---- the program ---------------------------------------------------------------------------------------------------
    def _loss_launch(self, dev, pg, ps, y, w, beta: float):
        """The loss of the step with its gradient, for both output counts: -> (ddos, loss).  Two outputs: ``pg``, ``ps`` are
        the halves of ``dos`` and ``ddos`` is laid out like it.  One output (the GNN-only baseline): ``ps is pg`` and
        ``beta = 0`` - the loss entry in its one-output use (the loss is rmse(pg) exactly, the second gradient goes to scratch);
        with ``loss=...`` the per-crystal entry in its own one-output form (ps == NULL: no second gradient, no scratch)."""
        B, S = pg.shape
        one = ps is pg
        ddos = ops.alloc64(dev, B if one else 2 * B, S)
        dpg = ddos if one else ddos[:B]
        if self.loss is not None:
            self._crystal, loss = self._loss_rows(ops.alloc64, dev, pg, None if one else ps, y, False, dpg,
                                                  None if one else ddos[B:], weights=w)
            return ddos, loss
        dps, loss = ops.alloc64(dev, B, S) if one else ddos[B:], ops.alloc64(dev, 1)
        ops.loss_phonon64(pg, ps, y, beta, dpg, dps, loss)
        return ddos, loss[0]

    def _program(self, fp, g, m: GraphMeta, drop):
        """forward program, loss kernel, backward program on the batch ``g``: -> (loss, outputs)."""
        model, cfg = self.model, self.model._cfg
        B, S = m.num_graphs, cfg.S
        w = self._batch_weights(g)                   # (refuses a batch without `weight` before anything is launched)
        dos, xL, ctx = F64.dostransformer_phonon_fwd(fp.P, cfg, g, m, drop=drop, per_crystal_keys=model.per_crystal_keys)
        ddos, loss = self._loss_launch(fp.flat.device, dos[:B], dos[B:], F64._f64(g.phdos).reshape(B, S), w, self.beta)
        F64.dostransformer_phonon_bwd(fp.P, fp.G, cfg, m, ctx, ddos, None)
        return loss, (dos[:B], xL, dos[B:])

    def _set_outputs(self, out, n_real: Optional[int]) -> None:
        """(dos_global, x_L, dos_system) of the step; the ghost rows of a padded batch's x_L are cut off."""
        self.last_outputs = out if n_real is None else (out[0], out[1][:n_real], out[2])

    def forward_backward(self, g, _bump: bool = True) -> torch.Tensor:
        """Forward + loss + backward; leaves the gradients in the flat buffer.  Returns the loss (0-dim float64 device tensor)."""
        self._ema_refuse("forward_backward")
        if _bump:                      # a direct forward_backward() + optimizer_step() loop draws fresh dropout masks too
            self._refuse("step", g)
        return self._batch_program(g, None, _bump)

    def _eager(self, fp, g, drop) -> torch.Tensor:
        with torch.no_grad():
            loss, out = self._program(fp, g, graph_meta(g, fp.flat.device), drop)
        self._set_outputs(out, getattr(g, "real_nodes", None))
        self.crystal_losses = self._crystal
        return loss

    # ---- replay --------------------------------------------------------------------------------------------------------
    def _run_slot(self, slot: Slot, fp, drop, fresh: bool) -> torch.Tensor:
        """The step on a slot whose static buffers hold the batch: recorded on first use, replayed afterwards."""
        if fresh:
            self._record(slot, fp, drop)                       # this IS the step for this batch (run + record)
        else:
            slot.prog.run()
        self._set_outputs(slot.out, getattr(slot.g, "real_nodes", None))
        self.crystal_losses = slot.crystal
        return slot.loss

    def _record(self, slot: Slot, fp, drop) -> None:
        """Run the step once on the slot's static buffers while recording every launch."""
        g, m = slot.g, slot.g.meta
        F64.require_replayable(g, slot.fields, fp.flat.device, self._who)
        with ops.recording_scope(), torch.no_grad():
            ops.RECORDER.begin()
            slot.loss, slot.out = self._program(fp, g, m, drop)
            slot.prog = ops.RECORDER.end()
        slot.crystal = self._crystal


class GraphnetworkTrainer64(Trainer64):
    """``Trainer64`` for the GNN-only baseline: AdamW training of a ``Graphnetwork_phonon`` whose live parameters are all float64
    (``model.double()``, hidden <= functional64.MAX_HIDDEN), all on libdosx.  The step is the factored float64 program
    (``functional64.graphnetwork_phonon_fwd / _bwd(factored_head=True)``: the output head on its rank structure,
    csrc/pair_head_f64.hip), the float64 loss entry in its one-output use (``ps = pg``, ``beta = 0``: the loss is
    ``sqrt(mean (dos - y)^2)`` exactly, `main_phDOS.py:109-111`) and the flat float64 AdamW - what ``model(batch)`` -> torch loss
    -> ``loss.backward()`` -> ``torch.optim.AdamW`` computes, to float64 rounding.  ``last_outputs`` is ``dos`` [B, S].

    The model has ONE output, so there is no ``beta`` to weigh (passing one raises), no attention - no per-crystal keys, no
    dropout, no softmax switch: a slot's key is its (padded) shape.  Which node encoder is dead (``node_encoder`` against
    ``node_encoder_prompt``) follows the node-feature width and is fixed by the first batch or dataset; a batch of the other
    width is refused.  ``replay``, ``bucket``, ``promote``, ``step_dataset``, ``state_dict`` / ``load_state_dict`` and
    ``max_slots`` are ``Trainer64``'s, and so are ``loss`` / ``huber_delta`` (the entry's one-output form: ``ps == NULL``, no scratch
    gradient) with ``crystal_losses``.  Limits: single GPU, no HIP-graph mode."""
    _who = "GraphnetworkTrainer64"
    _first_width_fixes_dead = True

    def __init__(self, model, lr: float = 1e-4, weight_decay: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8,
                 replay: bool = False, max_slots: int = 32, bucket=None, promote: float = 0.0,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, param_groups=None,
                 ema_decay: Optional[float] = None, ema_warmup: bool = True, loss: Optional[str] = None,
                 huber_delta: Optional[float] = None, sample_weights: bool = False, bin_weights=None,
                 functionals=None, functional_kind: str = "sq", functional_weight: float = 1.0, **unknown):
        if "beta" in unknown:
            raise ValueError(f"GraphnetworkTrainer64: beta={unknown['beta']} - the model has ONE output and its loss no second "
                             f"term to weigh")
        if unknown:
            raise TypeError(f"GraphnetworkTrainer64() got an unexpected keyword argument {sorted(unknown)[0]!r}")
        super().__init__(model, lr=lr, beta=1.0, weight_decay=weight_decay, betas=betas, eps=eps, replay=replay,
                         max_slots=max_slots, bucket=bucket, promote=promote, max_grad_norm=max_grad_norm,
                         skip_nonfinite=skip_nonfinite, param_groups=param_groups, ema_decay=ema_decay, ema_warmup=ema_warmup,
                         loss=loss, huber_delta=huber_delta, sample_weights=sample_weights, bin_weights=bin_weights,
                         functionals=functionals, functional_kind=functional_kind, functional_weight=functional_weight)

    def _require_model(self, model) -> None:
        GraphnetworkBase._require_f64_baseline(model, self._who)

    def _extra(self, fp, count: int):
        return None                   # (no attention, no dropout)

    def _program(self, fp, g, m: GraphMeta, drop):
        cfg = self.model._cfg
        w = self._batch_weights(g)
        dos, ctx = F64.graphnetwork_phonon_fwd(fp.P, cfg, g, m, factored_head=True)
        ddos, loss = self._loss_launch(fp.flat.device, dos, dos, F64._f64(g.phdos).reshape(m.num_graphs, cfg.S), w, 0.0)
        F64.graphnetwork_phonon_bwd(fp.P, fp.G, cfg, m, ctx, ddos, factored_head=True)
        return loss, dos

    def _set_outputs(self, out, n_real: Optional[int]) -> None:
        self.last_outputs = out

    def _key(self, n: int, e: int, B: int, n_max: int, drop, tiled: bool) -> tuple:
        return (n, e, B, n_max, self._loss_count(B))
