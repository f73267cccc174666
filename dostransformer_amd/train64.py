"""Fused float64 training step of ``DOSTransformer_phonon`` (the phonon reference trains in float64, `main_phDOS.py:15-16,
101-118`): the float64 forward program -> float64 loss kernel -> float64 backward program into the flat gradient buffer ->
flat float64 AdamW kernel.  No autograd graph, no torch loss ops, no per-parameter optimizer loop, no host synchronisation.

``Trainer64(replay=True)`` re-issues a RECORDED launch sequence (``ops.Program``), as ``train.Trainer(replay=True)`` does for
the fp32 program: the first step on a batch shape runs normally on static buffers while every libdosx call is recorded;
later steps of that shape copy the batch into the buffers and replay the list from C.

Limits: single GPU (no ``dist``), no HIP-graph mode, no ``Predictor`` counterpart, and slots are keyed by the batch's EXACT
shape (N, E, B, n_max).  The float64 program is not padding-safe - ``rows_add64(..., ia=node_graph)`` would read row B of a
[B, H] buffer for a ghost node - so ghost-padded batches (``batch.pad_batch``) are refused and there is no ``bucket`` /
``promote`` / ``step_dataset``.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import functional64 as F64
from . import ops
from ._lib import DosxError
from ._models import DOSTransformerBase
from .batch import CrystalBatch, GraphMeta, graph_meta
from .train import _AdamWState, _Loaded, _META_TENSORS

_F64_FIELDS = ("x", "edge_vec", "phdos")


class _Slot64:
    """Static buffers + recorded program of one exact batch shape: what the float64 program reads, in the dtype it reads it
    (float64 contiguous features and targets, int32 ``system``, clones of the GraphMeta tensors) - so that the casts in the
    body of ``functional64`` are no-ops on them and the recording holds libdosx calls only."""

    def __init__(self, g, m: GraphMeta, device):
        f = {k: torch.empty(g[k].shape, dtype=torch.float64, device=device) for k in _F64_FIELDS}
        f["system"] = torch.empty(g["system"].shape, dtype=torch.int32, device=device)
        meta = GraphMeta(num_nodes=m.num_nodes, num_edges=m.num_edges, num_graphs=m.num_graphs, n_max=m.n_max, edge_perm=None,
                         seg_tile=None, **{k: torch.empty_like(getattr(m, k), device=device) for k in _META_TENSORS})
        self.g = CrystalBatch(f, m.num_graphs, meta)
        self.prog = self.loss = self.out = None
        self._loaded = None

    @staticmethod
    def _signature(g, m: GraphMeta) -> _Loaded:
        """Identity + in-place version of everything load() copies (train._Slot._signature)."""
        return _Loaded(g, [g[k] for k in _F64_FIELDS + ("system",)] + [getattr(m, k) for k in _META_TENSORS])

    def load(self, g, m: GraphMeta) -> None:
        """Copy a batch of this shape into the static buffers (nothing when they hold this very batch, unwritten since): one
        launch for everything already in the buffers' format, ``Tensor.copy_`` for what needs a dtype conversion (an fp32
        batch, the int64 ``system``) or comes from another device."""
        sig = self._signature(g, m)
        if sig == self._loaded:
            return
        self._loaded = None
        pairs = []
        sm = self.g.meta
        for dst, src in [(self.g[k], g[k]) for k in _F64_FIELDS + ("system",)] + [(getattr(sm, k), getattr(m, k)) for k in _META_TENSORS]:
            if src.shape != dst.shape:
                raise ValueError(f"batch field of shape {tuple(src.shape)} loaded into a slot recorded with {tuple(dst.shape)}")
            if src.dtype == dst.dtype and src.device == dst.device and src.is_contiguous():
                pairs.append((dst.view(torch.int32), src.view(torch.int32)) if dst.element_size() == 8 else (dst, src))
            else:
                dst.copy_(src, non_blocking=True)
        ops.copy_many(pairs)
        self._loaded = sig


class Trainer64(_AdamWState):
    """AdamW(lr, weight_decay=1e-2) training of a ``DOSTransformer_phonon`` set to the float64 program
    (``model.double().set_program_dtype(torch.float64)``), all on libdosx: what ``model(batch)`` -> torch loss ->
    ``loss.backward()`` -> ``torch.optim.AdamW`` computes, without autograd and the per-tensor optimizer.

    Per-crystal keys stay the module's own switch (``model.set_per_crystal_keys``): read at every step, and part of a
    recorded slot's key.  ``step(g)`` returns the loss as a 0-dim float64 device tensor; ``state_dict()`` /
    ``load_state_dict()`` use ``train.Trainer``'s vocabulary with float64 moments.  ``slot_hits`` / ``slot_misses`` count the
    replayed and the recorded steps of ``replay=True``; at most ``max_slots`` shapes stay recorded (least recently used out).
    """

    def __init__(self, model, lr: float = 1e-4, beta: float = 1.0, weight_decay: float = 1e-2, betas=(0.9, 0.999),
                 eps: float = 1e-8, replay: bool = False, max_slots: int = 32):
        self._require_f64(model)
        self.model, self.lr, self.beta, self.wd, self.betas, self.eps = model, lr, beta, weight_decay, tuple(betas), eps
        self.replay = bool(replay)
        self.max_slots = int(max_slots)
        if self.max_slots < 1:
            raise ValueError(f"Trainer64: max_slots must be at least 1, got {max_slots}")
        self.step_count = 0
        self._m = self._v = self._fp = None
        self.last_outputs = None
        self._slots: "OrderedDict[tuple, _Slot64]" = OrderedDict()
        self.slot_hits = self.slot_misses = 0

    @staticmethod
    def _require_f64(model) -> None:
        ok = isinstance(model, DOSTransformerBase) and model._cfg.kind == "phonon" and model.program_dtype == torch.float64
        if not ok:
            raise DosxError(f"Trainer64 drives a DOSTransformer_phonon set to the float64 program "
                            f"(model.double().set_program_dtype(torch.float64)), got {type(model).__name__}"
                            + (f" with program_dtype {model.program_dtype}" if isinstance(model, DOSTransformerBase) else "")
                            + ": the fp32 program is train.Trainer's")

    # ---- the step ------------------------------------------------------------------------------------------------------
    def _refuse(self, g) -> None:
        """What a step cannot run on - raised before anything (the dropout seed included) has changed."""
        self._require_f64(self.model)
        if getattr(g, "real_nodes", None) is not None:
            raise DosxError("Trainer64: ghost-padded batches (batch.pad_batch) are refused - the float64 program is not "
                            "padding-safe (a ghost node's node_graph entry indexes past the per-crystal rows)")

    def _prepare(self, g):
        """-> (flat parameters, GraphMeta on the device, dropout operand); everything that may touch the host or torch's
        RNG (first use: flattening, the dropout seed) happens here, in front of any recording."""
        model = self.model
        dev = model._module_device()
        fp = model._ensure_flat(dev, g)
        self._state(fp)
        return fp, graph_meta(g, dev), model._dropout(dev, False)

    def _program(self, fp, g, m: GraphMeta, drop):
        """forward program, loss kernel, backward program on the batch ``g``: -> (loss, outputs)."""
        model, cfg, dev = self.model, self.model._cfg, fp.flat.device
        B, S = m.num_graphs, cfg.S
        dos, xL, ctx = F64.dostransformer_phonon_fwd(fp.P, cfg, g, m, drop=drop, per_crystal_keys=model.per_crystal_keys)
        y = F64._f64(g.phdos).reshape(B, S)
        ddos, loss = ops.alloc64(dev, 2 * B, S), ops.alloc64(dev, 1)
        ops.loss_phonon64(dos[:B], dos[B:], y, self.beta, ddos[:B], ddos[B:], loss)
        F64.dostransformer_phonon_bwd(fp.P, fp.G, cfg, m, ctx, ddos, None)
        return loss[0], (dos[:B], xL, dos[B:])

    def forward_backward(self, g, _bump: bool = True) -> torch.Tensor:
        """Forward + loss + backward; leaves the gradients in the flat buffer.  Returns the loss (0-dim float64 device tensor)."""
        if _bump:                      # a direct forward_backward() + optimizer_step() loop draws fresh dropout masks too
            self._refuse(g)
            self._bump_dropout_seed()
        fp, m, drop = self._prepare(g)
        with torch.no_grad():
            if self.replay:
                return self._slot_step(fp, g, m, drop)
            loss, self.last_outputs = self._program(fp, g, m, drop)
            return loss

    # ---- replay --------------------------------------------------------------------------------------------------------
    def _slot_step(self, fp, g, m: GraphMeta, drop) -> torch.Tensor:
        if m.edge_perm is not None:
            raise ValueError("Trainer64(replay=True) needs batches with destination-sorted edges (collate(sort_edges=True))")
        # what decides the launch list besides the shape: per-crystal keys, dropout on / off (train / eval mode, p > 0), the
        # tests' fp64-softmax switch - a slot recorded under one setting is never replayed under another
        key = (m.num_nodes, m.num_edges, m.num_graphs, m.n_max, bool(self.model.per_crystal_keys), drop is not None,
               None if drop is None else drop[0], bool(F64.SOFTMAX64), float(self.beta))
        slot = self._slots.get(key)
        if slot is None:
            self.slot_misses += 1
            while len(self._slots) >= self.max_slots:          # evict the least recently used shape
                self._slots.popitem(last=False)
            slot = _Slot64(g, m, fp.flat.device)
            slot.load(g, m)
            self._record(slot, fp, drop)                       # this IS the step for this batch (run + record)
            self._slots[key] = slot
        else:
            self.slot_hits += 1
            self._slots.move_to_end(key)
            slot.load(g, m)
            slot.prog.run()
        self.last_outputs = slot.out
        return slot.loss

    def _record(self, slot: _Slot64, fp, drop) -> None:
        """Run the step once on the slot's static buffers while recording every launch."""
        g, m = slot.g, slot.g.meta
        dev = fp.flat.device
        # a recorded program replays libdosx calls only: the torch casts in the body of functional64 must hand back the
        # very tensors they are given
        same = all(F64._f64(g[k]) is g[k] for k in _F64_FIELDS) and \
            g.system.to(device=dev, dtype=torch.int32).contiguous() is g.system
        if not same:
            raise DosxError("Trainer64: a slot buffer is not in the dtype / layout the float64 program reads")
        timer_on = ops.KERNEL_TIMER.enabled
        ops.KERNEL_TIMER.enabled = False
        try:
            ops.RECORDER.begin()
            slot.loss, slot.out = self._program(fp, g, m, drop)
            slot.prog = ops.RECORDER.end()
        finally:
            if ops.RECORDER.active:
                ops.RECORDER.end()
            ops.KERNEL_TIMER.enabled = timer_on

    # ---- optimizer -----------------------------------------------------------------------------------------------------
    def optimizer_step(self) -> None:
        """The flat AdamW launch, issued behind the (recorded) program: ``step`` changes every step."""
        fp = self._fp if self._fp is not None else self.model.flat_params()
        m, v = self._state(fp)
        self.step_count += 1
        ops.adamw64(fp.flat, fp.grad, m, v, fp.total, self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self.step_count)

    def step(self, g) -> torch.Tensor:
        self._refuse(g)
        self._bump_dropout_seed()
        loss = self.forward_backward(g, _bump=False)
        self.optimizer_step()
        return loss
