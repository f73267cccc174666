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

Limits: single GPU (no ``dist``), no HIP-graph mode.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch

from . import functional64 as F64
from . import ops
from ._lib import DosxError
from ._models import DOSTransformerBase
from .batch import GraphMeta, bucket_sizes, graph_meta, pad_batch
from .slots import Slot, SlotCache
from .train import _AdamWState


class Trainer64(_AdamWState, SlotCache):
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
    """

    def __init__(self, model, lr: float = 1e-4, beta: float = 1.0, weight_decay: float = 1e-2, betas=(0.9, 0.999),
                 eps: float = 1e-8, replay: bool = False, max_slots: int = 32, bucket=None, promote: float = 0.0):
        DOSTransformerBase._require_f64_program(model, "Trainer64")
        self.model, self.lr, self.beta, self.wd, self.betas, self.eps = model, lr, beta, weight_decay, tuple(betas), eps
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

    # ---- the step ------------------------------------------------------------------------------------------------------
    def _refuse(self, g) -> None:
        """What a step cannot run on - raised before anything (the dropout seed included) has changed."""
        DOSTransformerBase._require_f64_program(self.model, "Trainer64")
        if self.bucket is None and getattr(g, "real_nodes", None) is not None:
            raise DosxError("Trainer64: ghost-padded batches (batch.pad_batch) are refused without bucket=(node_step, "
                            "edge_step) - slots are keyed by the exact shape of an unpadded batch")

    def _prepare(self, g):
        """-> (flat parameters, dropout operand); everything that may touch the host or torch's RNG (first use: flattening, the
        dropout seed) happens here, in front of any recording."""
        model = self.model
        dev = model._module_device()
        fp = model._ensure_flat(dev, g)
        self._state(fp)
        return fp, model._dropout(dev, False)

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

    def _set_outputs(self, out, n_real: Optional[int]) -> None:
        """(dos_global, x_L, dos_system) of the step; the ghost rows of a padded batch's x_L are cut off."""
        self.last_outputs = out if n_real is None else (out[0], out[1][:n_real], out[2])

    def forward_backward(self, g, _bump: bool = True) -> torch.Tensor:
        """Forward + loss + backward; leaves the gradients in the flat buffer.  Returns the loss (0-dim float64 device tensor)."""
        if _bump:                      # a direct forward_backward() + optimizer_step() loop draws fresh dropout masks too
            self._refuse(g)
            self._bump_dropout_seed()
        fp, drop = self._prepare(g)
        m = graph_meta(g, fp.flat.device)
        with torch.no_grad():
            if self.replay:
                return self._slot_step(fp, g, m, drop)
            loss, out = self._program(fp, g, m, drop)
            self._set_outputs(out, getattr(g, "real_nodes", None))
            return loss

    # ---- replay --------------------------------------------------------------------------------------------------------
    def _key(self, n: int, e: int, B: int, n_max: int, drop) -> tuple:
        """What decides the launch list: the (padded) shape, then per-crystal keys, dropout on / off (train / eval mode, p > 0),
        the tests' fp64-softmax switch - a slot recorded under one setting is never replayed under another."""
        return (n, e, B, n_max, bool(self.model.per_crystal_keys), drop is not None, None if drop is None else drop[0],
                bool(F64.SOFTMAX64), float(self.beta))

    def _run_slot(self, slot: Slot, fp, drop, fresh: bool) -> torch.Tensor:
        """The step on a slot whose static buffers hold the batch: recorded on first use, replayed afterwards."""
        if fresh:
            self._record(slot, fp, drop)                       # this IS the step for this batch (run + record)
        else:
            slot.prog.run()
        self._set_outputs(slot.out, getattr(slot.g, "real_nodes", None))
        return slot.loss

    def _slot_step(self, fp, g, m: GraphMeta, drop) -> torch.Tensor:
        if m.edge_perm is not None:
            raise ValueError("Trainer64(replay=True) needs batches with destination-sorted edges (collate(sort_edges=True))")
        if self.bucket is not None and getattr(g, "real_nodes", None) is None:       # not padded yet: pad on the fly
            g = pad_batch(g, *bucket_sizes(m.num_nodes, m.num_edges, *self.bucket))
            m = g.meta
        key = self._key(m.num_nodes, m.num_edges, m.num_graphs, m.n_max, drop)
        slot = self._lookup(key)
        fresh = slot is None
        if fresh:
            slot = Slot(g, m, "phonon", torch.float64)
        else:
            slot.load(g, m)
        loss = self._run_slot(slot, fp, drop, fresh)
        if fresh:
            self._slots[key] = slot
        return loss

    def _record(self, slot: Slot, fp, drop) -> None:
        """Run the step once on the slot's static buffers while recording every launch."""
        g, m = slot.g, slot.g.meta
        F64.require_replayable(g, slot.fields, fp.flat.device, "Trainer64")
        with ops.recording_scope():
            ops.RECORDER.begin()
            slot.loss, slot.out = self._program(fp, g, m, drop)
            slot.prog = ops.RECORDER.end()

    def step_dataset(self, ds, indices, n_max: Optional[int] = None) -> torch.Tensor:
        """One training step on the crystals ``indices`` of a device-resident ``loader.DeviceDataset`` (float64 tables:
        ``DeviceDataset(..., dtype=torch.float64)`` holds them without a copy).  With ``replay`` and ``bucket`` the batch is
        collated by ``dosx_collate_padded_f64`` STRAIGHT INTO the static buffers of its shape bucket, ghost padding included, and
        the bucket's recorded program is replayed (recorded on first use, or - ``promote`` - run in a live larger bucket):
        bitwise ``step(pad_batch(ds.collate(indices, n_max=n_max), *bucket_sizes(N, E, *bucket)))``.  Otherwise it is
        ``step(ds.collate(indices, n_max=n_max))``.  ``n_max`` may exceed the selection's largest crystal, so that one value
        serves a whole dataset (with per-crystal keys and no dropout the numbers do not depend on it)."""
        if not (self.replay and self.bucket is not None):
            return self.step(ds.collate(indices, n_max=n_max))
        DOSTransformerBase._require_f64_program(self.model, "Trainer64")
        idx, N, E, n_max = ds.bucket_dims(indices, n_max)
        B = int(idx.shape[0])
        n_pad, e_pad = bucket_sizes(N, E, *self.bucket)
        self._bump_dropout_seed()
        fp, drop = self._prepare(None)
        key = self._key(n_pad, e_pad, B, n_max, drop)
        slot = self._lookup(key, allow_promote=True)
        fresh = slot is None
        if fresh:
            t = ds._f64_tables()
            slot = Slot.empty("phonon", fp.flat.device, torch.float64, B, n_pad, e_pad, n_max, int(t["x"].shape[1]),
                              int(t["edge"].shape[1]), int(t["target"].shape[1]))
        ds.collate_into(slot.g, idx, slot.collate_scratch())
        slot._loaded = None                                        # (the static buffers now hold a batch no object stands for)
        slot.set_real_nodes(N)
        with torch.no_grad():
            loss = self._run_slot(slot, fp, drop, fresh)
        if fresh:
            self._slots[key] = slot
        self.optimizer_step()
        return loss

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
