"""Replayed inference (small-batch / batch-1 prediction is launch-bound).

``Predictor(model)(batch)`` returns what ``model(batch)`` returns under ``torch.no_grad()`` —
(dos_global, x, dos_system), `DOSTransformer_phonon.py:66-119` / `DOSTransformer.py` forward — but issues the
forward program from a recorded launch list (``ops.Program`` -> ``dosx_replay``) on static buffers of the
batch's (N, E, B, n_max) bucket: the first call on a bucket runs eagerly while recording, later calls are
"copy the batch in, replay".  Ghost padding is exact (``batch.pad_batch``), so the outputs are bitwise those
of the eager forward.  The returned tensors alias the bucket's buffers and are overwritten by the next call
that lands in the same bucket; ``.clone()`` them to keep them.

It quacks like the module for the evaluation loops: ``evaluate.test(Predictor(model), loader)``.

``Predictor(model, per_crystal_keys=True)``: the reference validates and tests at ``batch_size = 1`` (`main_eDOS.py:55-56`,
`utils.py:61-143`), and its outputs depend on the batch's Nmax (the zero-padded atoms take part in the softmax,
`DOSTransformer_phonon.py:86`), so reference metrics need batch-1 forwards - 300 us each, launch-bound.  With this flag the two
cross attentions of a BATCHED forward attend over each crystal's own atoms only (``DosxAttn.key_ptr`` = the batch's graph_ptr):
B crystals in one pass give what B batch-1 forwards give (to fp32 rounding), at the batched rate.

``Predictor64(model)`` is the same for a ``DOSTransformer_phonon`` set to the float64 program
(``model.double().set_program_dtype(torch.float64)``): the float64 forward program on ghost-padded buckets, outputs in float64,
bitwise those of ``model(batch)``.  Per-crystal keys stay the module's own switch (``model.set_per_crystal_keys``).
"""
from __future__ import annotations

import torch

from . import functional64 as F64
from . import ops
from ._models import DOSTransformerBase
from .batch import CrystalBatch, graph_meta
from .slots import Slot, padded_to_bucket


class _Predictor:
    """What Predictor and Predictor64 share: the buckets and their recorded forward programs.  A subclass supplies the model
    check (``_require``), the dtype of its slots (``_dtype``), the tail of a slot's key (``_key_tail``) and the forward call
    on a slot (``_forward`` -> (outputs, what to keep alive)).  ``slot_misses`` / ``slot_hits`` count the recorded
    and the replayed calls."""
    _dtype: torch.dtype

    def __init__(self, model: DOSTransformerBase, bucket=(8, 128)):
        self._require(model)
        self.model = model
        self.bucket = tuple(bucket)
        self.kind = model._cfg.kind
        self._fp = None
        self._slots = {}
        self.slot_hits = self.slot_misses = 0

    def eval(self):
        self.model.eval()
        return self

    def _key_tail(self) -> tuple:
        return ()

    def _record(self, slot: Slot, fp) -> None:
        with ops.recording_scope(), torch.no_grad():
            ops.RECORDER.begin()
            slot.out, slot.keep = self._forward(fp, slot)        # (the program's intermediates live as long as the recording)
            slot.prog = ops.RECORDER.end()

    def __call__(self, g: CrystalBatch):
        model, who = self.model, type(self).__name__
        self._require(model)
        if model.training and getattr(model, "_attn_drop", 0.0) > 0.0:
            raise RuntimeError(f"{who} replays an inference program: call model.eval() first (attention dropout is "
                               "active in training mode)")
        dev = model._module_device()
        if dev.type != "cuda":
            raise RuntimeError(f"{who} runs only on an MI355X through libdosx (no CPU fallback)")
        fp = model._ensure_flat(dev, g)
        if fp is not self._fp:                # parameters were re-homed: recorded pointers are stale
            self._fp, self._slots = fp, {}
        m = graph_meta(g, dev)
        if m.edge_perm is not None:
            raise ValueError(f"{who} needs batches from collate(sort_edges=True) / DeviceDataset.collate")
        n_real = getattr(g, "real_nodes", None)
        if n_real is None:
            n_real = m.num_nodes
            g = padded_to_bucket(g, m, self.bucket)
            m = g.meta
        key = (m.num_nodes, m.num_edges, m.num_graphs, m.n_max) + self._key_tail()
        slot = self._slots.get(key)
        if slot is None:
            self.slot_misses += 1
            slot = Slot(g, m, self.kind, self._dtype, targets=False)
            self._record(slot, fp)
            self._slots[key] = slot
        else:
            self.slot_hits += 1
            slot.load(g, m)
            slot.prog.run()
        dg, xL, ds = slot.out
        return dg, xL[:n_real], ds


class Predictor(_Predictor):
    _dtype = torch.float32

    def __init__(self, model: DOSTransformerBase, bucket=(8, 128), per_crystal_keys: bool = False):
        super().__init__(model, bucket)
        self.per_crystal_keys = bool(per_crystal_keys)

    @staticmethod
    def _require(model) -> None:
        if not isinstance(model, DOSTransformerBase):
            raise TypeError("Predictor drives DOSTransformer / DOSTransformer_phonon modules")
        model._require_fp32_program("Predictor")

    def _forward(self, fp, slot):
        g = slot.g
        dg, xL, ds, keep = self.model._program_fwd(fp.P, g, g.meta, per_crystal_keys=self.per_crystal_keys)
        return (dg, xL, ds), keep


class Predictor64(_Predictor):
    """``Predictor`` for a module set to the float64 program: ``Predictor64(model)(batch)`` returns
    ``(dos_global, x[:n_real], dos_system)`` in float64, what ``model(batch)`` returns under ``torch.no_grad()``, from a launch
    list recorded on the static buffers of the batch's ghost-padded bucket (first call recorded, later calls replayed).  The
    module's per-crystal-keys switch and ``functional64.SOFTMAX64`` are part of a slot's key."""
    _dtype = torch.float64

    @staticmethod
    def _require(model) -> None:
        DOSTransformerBase._require_f64_program(model, "Predictor64")

    def _key_tail(self) -> tuple:
        return (bool(self.model.per_crystal_keys), bool(F64.SOFTMAX64))

    def _forward(self, fp, slot):
        g, B = slot.g, slot.g.meta.num_graphs
        F64.require_replayable(g, slot.fields, fp.flat.device, "Predictor64")
        dos, xL, ctx = F64.dostransformer_phonon_fwd(fp.P, self.model._cfg, g, g.meta, drop=None,
                                                     per_crystal_keys=self.model.per_crystal_keys)
        return (dos[:B], xL, dos[B:]), ctx
