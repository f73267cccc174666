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

``Predictor(model)`` also takes the GNN-only baselines - ``Graphnetwork``, ``Graphnetwork_phonon`` (fp32 parameters) and
``embedder_eDOS.mlp.mlp`` - and returns what THEIR forward returns: ``(dos, x)`` for ``Graphnetwork``, ``dos`` for the other two,
bitwise the eval-mode ``functional.graphnetwork_fwd(factored_head=True)`` (the output head on its rank structure, as
``train.Trainer`` runs it).  They have no attention, so ``per_crystal_keys=True`` is refused and ``batch_independent`` is True:
``evaluate.test_per_crystal`` takes such a predictor as it is.

``Predictor64(model)`` is the same for a ``DOSTransformer_phonon`` set to the float64 program
(``model.double().set_program_dtype(torch.float64)``): the float64 forward program on ghost-padded buckets, outputs in float64,
bitwise those of ``model(batch)``.  Per-crystal keys stay the module's own switch (``model.set_per_crystal_keys``).

``Predictor64(model)`` also takes a ``Graphnetwork_phonon`` with float64 parameters (``model.double()``), as ``Predictor`` takes
the fp32 baselines: it returns ``dos`` in float64, bitwise ``functional64.graphnetwork_phonon_fwd(factored_head=True)`` (the
output head on its rank structure, as ``train64.GraphnetworkTrainer64`` runs it) on the ghost-padded bucket, and
``batch_independent`` is True.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import functional64 as F64
from . import ops
from ._lib import DosxError
from ._models import DOSTransformerBase, GraphnetworkBase
from .batch import CrystalBatch, bucket_sizes, graph_meta
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

    def check(self) -> None:
        """Raise :class:`DosxError` if a column-split exchange reported a stall since the last clean check (``ops.check_exchanges``);
        one small read-back: call it once per evaluation."""
        dev = self.model._module_device()
        if dev.type == "cuda":
            ops.check_exchanges(dev)

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
        return self._outputs(slot, n_real)

    def _outputs(self, slot: Slot, n_real: int):
        """What the module's forward returns, from a bucket's output buffers (node rows cut to the real ones)."""
        dg, xL, ds = slot.out
        return dg, xL[:n_real], ds

    def _eval_outputs(self, slot: Slot):
        """(the DOS prediction the metrics are computed from [B,S], node embeddings [N_pad,H]) of a bucket (evaluate.test_per_crystal)."""
        _, x, dos_system = slot.out
        return dos_system, x

    @property
    def batch_independent(self) -> bool:
        """True when a crystal's outputs do not depend on its batch mates whatever the flags (models without attention)."""
        return bool(getattr(self.model, "batch_independent", False))

    def _tables(self, ds):
        """The dataset's feature tables in the dtype of this predictor's slots."""
        return ds._f32_tables()

    def _width_batch(self, ds):
        """What ``_ensure_flat`` gets for a dataset pass in place of a batch (None: the model's parameters do not depend on it)."""
        return None

    def forward_dataset(self, ds, indices, n_max: Optional[int] = None):
        """The forward pass on the crystals ``indices`` of a device-resident ``loader.DeviceDataset``, what ``step_dataset`` is
        for training: the batch is collated STRAIGHT INTO the static buffers of its (ghost-padded) shape bucket, targets included,
        and the bucket's program runs - recorded on the bucket's first visit, replayed afterwards.  Returns
        ``((dos_global, x[:n_real], dos_system), target)``: the outputs of ``self(ds.collate(indices, n_max=n_max))`` and the
        bucket's target buffer (``phdos`` [B,S] / ``y_ft`` [B*S]), all aliasing static buffers that the next call on the bucket
        overwrites.  ``n_max`` may exceed the selection's largest crystal, so that one value serves a whole split; only with
        per-crystal keys do the outputs not depend on it.  These buckets are kept apart from those of ``__call__``."""
        slot, N = self._run_dataset(ds, indices, n_max)
        return self._outputs(slot, N), self._target(slot)

    def _target(self, slot: Slot) -> torch.Tensor:
        return slot.g["phdos" if self.kind == "phonon" else "y_ft"]

    def _run_dataset(self, ds, indices, n_max: Optional[int] = None):
        """forward_dataset's work; returns (the bucket - outputs in ``slot.out``, metadata in ``slot.g.meta`` -, real node count)."""
        model, who = self.model, type(self).__name__
        self._require(model)
        if model.training and getattr(model, "_attn_drop", 0.0) > 0.0:
            raise RuntimeError(f"{who} replays an inference program: call model.eval() first (attention dropout is "
                               "active in training mode)")
        dev = model._module_device()
        if dev.type != "cuda":
            raise RuntimeError(f"{who} runs only on an MI355X through libdosx (no CPU fallback)")
        fp = model._ensure_flat(dev, self._width_batch(ds))
        if fp is not self._fp:                # parameters were re-homed: recorded pointers are stale
            self._fp, self._slots = fp, {}
        idx, N, E, n_max = ds.bucket_dims(indices, n_max)
        B = int(idx.shape[0])
        n_pad, e_pad = bucket_sizes(N, E, *self.bucket)
        key = (n_pad, e_pad, B, n_max) + self._key_tail() + ("dataset",)
        slot = self._slots.get(key)
        fresh = slot is None
        if fresh:
            t = self._tables(ds)
            slot = Slot.empty(self.kind, dev, self._dtype, B, n_pad, e_pad, n_max, int(t["x"].shape[1]), int(t["edge"].shape[1]),
                              int(t["target"].shape[1]), tiled=self._dtype == torch.float32)
        ds.collate_into(slot.g, idx, slot.collate_scratch())
        slot._loaded = None                                        # (the static buffers now hold a batch no object stands for)
        slot.set_real_nodes(N)
        if fresh:
            self.slot_misses += 1
            self._record(slot, fp)
            self._slots[key] = slot
        else:
            self.slot_hits += 1
            slot.prog.run()
        return slot, N


class Predictor(_Predictor):
    _dtype = torch.float32

    def __init__(self, model, bucket=(8, 128), per_crystal_keys: bool = False):
        super().__init__(model, bucket)
        self._baseline = isinstance(model, GraphnetworkBase)
        if self._baseline and per_crystal_keys:
            raise DosxError(f"Predictor({type(model).__name__}, per_crystal_keys=True): the model has no attention - a crystal's "
                            f"output never depends on its batch mates (Predictor(model).batch_independent)")
        self.per_crystal_keys = bool(per_crystal_keys)

    @staticmethod
    def _require(model) -> None:
        if not isinstance(model, (DOSTransformerBase, GraphnetworkBase)):
            raise TypeError("Predictor drives DOSTransformer / DOSTransformer_phonon / Graphnetwork / Graphnetwork_phonon / mlp modules")
        model._require_fp32_program("Predictor")

    def _width_batch(self, ds):
        if not self._baseline:
            return None
        from .trainer_base import _Width            # (which node encoder is live follows the dataset's node-feature width)
        return _Width(int(ds._f32_tables()["x"].shape[1]))

    def _outputs(self, slot: Slot, n_real: int):
        if not self._baseline:
            return super()._outputs(slot, n_real)
        out = slot.out
        return (out[0], out[1][:n_real]) if self.model._returns_x else out[0]

    def _eval_outputs(self, slot: Slot):
        if not self._baseline:
            return super()._eval_outputs(slot)
        return slot.out[0], slot.keep.xL       # (mlp: its encoder output - what its decoder pools)

    def _forward(self, fp, slot):
        g = slot.g
        if self._baseline:
            out = self.model._program_fwd(fp.P, g, g.meta, factored_head=True)
            return out[:-1], out[-1]
        dg, xL, ds, keep = self.model._program_fwd(fp.P, g, g.meta, per_crystal_keys=self.per_crystal_keys)
        return (dg, xL, ds), keep


class Predictor64(_Predictor):
    """``Predictor`` for a module set to the float64 program: ``Predictor64(model)(batch)`` returns
    ``(dos_global, x[:n_real], dos_system)`` in float64, what ``model(batch)`` returns under ``torch.no_grad()``, from a launch
    list recorded on the static buffers of the batch's ghost-padded bucket (first call recorded, later calls replayed).  The
    module's per-crystal-keys switch and ``functional64.SOFTMAX64`` are part of a slot's key."""
    _dtype = torch.float64

    def __init__(self, model, bucket=(8, 128)):
        super().__init__(model, bucket)
        self._baseline = isinstance(model, GraphnetworkBase)

    @staticmethod
    def _require(model) -> None:
        if isinstance(model, GraphnetworkBase):
            GraphnetworkBase._require_f64_baseline(model, "Predictor64")
        else:
            DOSTransformerBase._require_f64_program(model, "Predictor64")

    def _key_tail(self) -> tuple:
        if self._baseline:                     # no attention: the (padded) shape alone decides the launch list
            return ()
        return (bool(self.model.per_crystal_keys), bool(F64.SOFTMAX64))

    def _tables(self, ds):
        return ds._f64_tables()

    def _width_batch(self, ds):
        if not self._baseline:
            return None
        from .trainer_base import _Width            # (which node encoder is live follows the dataset's node-feature width)
        return _Width(int(ds._f64_tables()["x"].shape[1]))

    def _outputs(self, slot: Slot, n_real: int):
        return slot.out[0] if self._baseline else super()._outputs(slot, n_real)

    def _eval_outputs(self, slot: Slot):
        return (slot.out[0], slot.keep.xL) if self._baseline else super()._eval_outputs(slot)

    def _forward(self, fp, slot):
        g, B = slot.g, slot.g.meta.num_graphs
        F64.require_replayable(g, slot.fields, fp.flat.device, "Predictor64")
        if self._baseline:
            dos, ctx = F64.graphnetwork_phonon_fwd(fp.P, self.model._cfg, g, g.meta, factored_head=True)
            return (dos,), ctx
        dos, xL, ctx = F64.dostransformer_phonon_fwd(fp.P, self.model._cfg, g, g.meta, drop=None,
                                                     per_crystal_keys=self.model.per_crystal_keys)
        return (dos[:B], xL, dos[B:]), ctx
