"""What the replayed drivers share (train.Trainer, train64.Trainer64, predict.Predictor / Predictor64): the static buffers
of a shape bucket with their recording (``Slot``), the bounded bucket table with its LRU / promotion bookkeeping
(``SlotCache``) and the cached ghost-padded copy of a batch (``padded_to_bucket``).  fp32 and float64 differ only in the
dtype of the feature buffers."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .batch import CrystalBatch, GraphMeta, bucket_sizes, pad_batch, seg_tile_bound

META_TENSORS = ("src", "dst", "rowptr_dst", "perm_src", "rowptr_src", "graph_ptr", "node_graph", "dense_row", "inv_deg")


class Loaded:
    """What a bucket's static buffers currently hold: see Slot._signature."""
    __slots__ = ("g", "ts", "versions")

    def __init__(self, g, ts):
        self.g, self.ts, self.versions = g, tuple(ts), tuple(t._version for t in ts)

    def __eq__(self, other):
        return (isinstance(other, Loaded) and self.g is other.g and len(self.ts) == len(other.ts)
                and all(a is b for a, b in zip(self.ts, other.ts)) and self.versions == other.versions)

    __hash__ = None


class Slot:
    """Static buffers + recording (launch lists or captured graphs) of one shape bucket.

    The buffers hold exactly what the kernels read: contiguous features and targets in ``dtype`` (torch.float32 for the fp32
    program, torch.float64 for functional64), int32 ``system``, clones of the GraphMeta tensors.  load() converts while it
    copies (the phonon pipeline is fp64 upstream, main_phDOS.py:15-16), so the recorded program never needs a cast of its own
    - a torch cast inside the recording would not be replayed.  The buffers of a padded shape carry ``real_nodes`` (the real
    node count of the batch they hold), like a ``pad_batch`` batch."""

    def __init__(self, g, m: GraphMeta, kind: str, dtype: torch.dtype, targets: bool = True, weights: bool = False):
        """Buffers made from (and holding) batch ``g`` with metadata ``m``, on the device of ``m``; torch copies only.
        ``weights``: also a static ``weight`` buffer, [B] sample weights filled with the other fields (trainers' sample_weights)."""
        dev = m.src.device
        fields = ["x", "system"] + (["edge_vec"] if kind == "phonon" else ["edge_attr", "glob"])
        if targets:
            fields.append("phdos" if kind == "phonon" else "y_ft")
        if weights:
            fields.append("weight")
        f = {k: torch.empty(g[k].shape, dtype=dtype if g[k].is_floating_point() else torch.int32, device=dev).copy_(g[k])
             for k in fields}
        f["edge_index"], f["batch"] = getattr(g, "edge_index", None), getattr(g, "batch", None)     # never read by the kernels
        # (the message-GEMM tile table belongs to the fp32 program: DeviceDataset.collate_into refuses a float64 bucket with one)
        tiled = dtype == torch.float32 and m.seg_tile is not None
        meta = GraphMeta(num_nodes=m.num_nodes, num_edges=m.num_edges, num_graphs=m.num_graphs, n_max=m.n_max,
                         edge_perm=None, seg_tile=m.seg_tile.clone() if tiled else None,
                         **{k: getattr(m, k).clone() for k in META_TENSORS})
        self._setup(CrystalBatch(f, m.num_graphs, meta), fields)
        self.set_real_nodes(getattr(g, "real_nodes", None))
        self._loaded = self._signature(g, m)       # the static buffers hold THIS batch (copied above)

    def _setup(self, g: CrystalBatch, fields) -> None:
        self.fields = list(fields)
        self.g = g
        self.graph_a = self.graph_b = None         # train.Trainer(graph=True)
        self.prog = None                           # the first (or only) recorded program
        self.plan = []                             # train.Trainer(replay=True): programs separated by the collectives
        self.keep = self.loss = self.out = self.sse = None
        self.crystal = None                        # per-crystal losses of the step (trainers' loss=...), else None
        self.scratch = None
        self._loaded = None

    @classmethod
    def empty(cls, kind: str, device, dtype: torch.dtype, B: int, n_pad: int, e_pad: int, n_max: int, Fa: int, Fe: int,
              S: int, tiled: bool = False, weight_table: Optional[torch.Tensor] = None) -> "Slot":
        """Uninitialised static buffers of a bucket, to be filled by ``DeviceDataset.collate_into`` (no source batch).
        ``weight_table``: the dataset's resident [C] sample weights in ``dtype`` - the bucket then carries the table itself as
        ``weight`` and the selection ``collate_into`` leaves in its index scratch as ``weight_index``: the loss launch gathers,
        no [B] staging buffer and nothing for the collate kernels to do."""
        flt = lambda *s: torch.empty(*s, dtype=dtype, device=device)
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=device)
        f = {"x": flt(n_pad, Fa), "system": i32(B)}
        if kind == "phonon":
            f["edge_vec"], f["phdos"] = flt(e_pad, Fe), flt(B, S)
        else:
            f["edge_attr"], f["glob"], f["y_ft"] = flt(e_pad, Fe), flt(2 * B), flt(B * S)
        fields = list(f)
        f["edge_index"] = f["batch"] = None
        meta = GraphMeta(num_nodes=n_pad, num_edges=e_pad, num_graphs=B, n_max=n_max, edge_perm=None,
                         src=i32(e_pad), dst=i32(e_pad), rowptr_dst=i32(n_pad + 1), perm_src=i32(e_pad),
                         rowptr_src=i32(n_pad + 1), graph_ptr=i32(B + 1), node_graph=i32(n_pad), dense_row=i32(n_pad),
                         inv_deg=torch.empty(n_pad, dtype=torch.float32, device=device),
                         seg_tile=i32(3, seg_tile_bound(n_pad, e_pad, B) + 1) if tiled else None)
        self = cls.__new__(cls)
        self._setup(CrystalBatch(f, B, meta), fields)
        if weight_table is not None:
            self.g["weight"], self.g["weight_index"] = weight_table, self.collate_scratch()["small"][:B]
        return self

    def collate_scratch(self):
        """Index scratch of ``DeviceDataset.collate_into``, made on first use and sized from the SLOT's own padded counts: a
        promoted host bucket is larger than the requested one, and the collate kernels write node_row / edge_row up to them."""
        if self.scratch is None:
            m = self.g.meta
            i32 = lambda n: torch.empty(n, dtype=torch.int32, device=m.src.device)
            self.scratch = {"small": i32(4 * m.num_graphs + 3), "node_row": i32(m.num_nodes), "edge_row": i32(m.num_edges)}
        return self.scratch

    def set_real_nodes(self, n: Optional[int]) -> None:
        object.__setattr__(self.g, "real_nodes", n)

    @property
    def real_nodes(self) -> int:
        n = getattr(self.g, "real_nodes", None)
        return self.g.meta.num_nodes if n is None else n

    def _signature(self, g, m: GraphMeta) -> Loaded:
        """Identity + version of everything load() would copy from batch ``g``: the batch object and its source tensors
        THEMSELVES (strong references, compared with ``is``) with torch's in-place version counters (any in-place write to a field
        since the last load changes one).  Addresses are not identities: a batch collated after the previous one was freed gets the
        same ``id()`` and - from the caching allocator - the same device pointers with version 0; holding the objects is what
        keeps a later batch from being mistaken for this one (tests/test_gpu_step.py: an epoch of freshly collated batches)."""
        ts = [g[k] for k in self.fields] + [getattr(m, k) for k in META_TENSORS]
        if self.g.meta.seg_tile is not None and m.seg_tile is not None:
            ts.append(m.seg_tile)
        return Loaded(g, ts)

    def _source(self, g, k: str) -> torch.Tensor:
        """Field k of a batch as load() copies it.  The int64 -> int32 copy of `system` (the reference's crystal-system
        index, [B]) is cached on the batch object: batches are revisited every epoch, and a cast per visit is one more kernel
        in front of every step."""
        t = g[k]
        if k != "system" or t.dtype == torch.int32 or not isinstance(g, CrystalBatch):
            return t
        c = getattr(g, "_system32", None)
        if c is None or c[0] is not t:
            c = (t, t.to(torch.int32))
            object.__setattr__(g, "_system32", c)
        return c[1]

    def load(self, g, m: Optional[GraphMeta] = None) -> None:
        """Copy a batch of this bucket's shape into the static buffers (``m``: its metadata, default ``g.meta``): ONE launch
        for everything that is already in the buffers' format (contiguous, on the device); what needs a dtype conversion (an
        fp64 batch into fp32 buffers or the reverse, int64 ``system``) or comes from elsewhere goes through ``Tensor.copy_``."""
        if m is None:
            m = g.meta
        # The bucket already holds this very batch (same object, no field written in place since): nothing to copy.  An epoch loop
        # over pre-collated device-resident batches revisits each of them every epoch - the copy was one launch in front of every
        # step (round 6); a batch that shares its bucket with another one is copied as before.
        sig = self._signature(g, m)
        if sig == self._loaded:
            return
        self._loaded = None
        self.set_real_nodes(getattr(g, "real_nodes", None))
        sm = self.g.meta
        items = [(self.g[k], self._source(g, k)) for k in self.fields] + [(getattr(sm, k), getattr(m, k)) for k in META_TENSORS]
        if sm.seg_tile is not None:
            if m.seg_tile is None or m.seg_tile.shape != sm.seg_tile.shape:
                raise ValueError("batch without (matching) message-GEMM tile table loaded into a bucket recorded with one")
            items.append((sm.seg_tile, m.seg_tile))
        pairs = []
        for dst, src in items:
            if src.shape != dst.shape:
                if src.numel() != dst.numel():          # (never let copy_ broadcast)
                    raise ValueError(f"batch field of shape {tuple(src.shape)} loaded into a slot recorded with {tuple(dst.shape)}")
                src = src.reshape(dst.shape)
            if src.dtype == dst.dtype and src.device == dst.device and src.is_contiguous():
                pairs.append((dst.view(torch.int32), src.view(torch.int32)) if dst.element_size() == 8 else (dst, src))
            else:
                dst.copy_(src, non_blocking=True)
        ops.copy_many(pairs)
        self._loaded = sig


def promote_key(live_keys, key, tol: float):
    """The live bucket key a batch of bucket ``key`` = (n_pad, e_pad, *rest) can run in: same ``rest`` (batch size, key-slot
    count, global count, tiling), at least as many node and edge rows, at most ``tol`` (relative) more of either; the
    smallest such by (edges, nodes), or None."""
    n, e, rest = key[0], key[1], tuple(key[2:])
    best = None
    for k in live_keys:
        if tuple(k[2:]) != rest or k[0] < n or k[1] < e:
            continue
        if k[0] > n * (1.0 + tol) + 1e-9 or k[1] > e * (1.0 + tol) + 1e-9:
            continue
        if best is None or (k[1], k[0]) < (best[1], best[0]):
            best = k
    return best


class SlotCache:
    """The bucket table of a trainer.  Expects ``_slots`` (OrderedDict key -> Slot, least recently used first), ``_seen``,
    ``max_slots``, ``promote`` and the counters ``slot_hits`` / ``slot_misses`` / ``slot_promoted``."""

    def _lookup(self, key, allow_promote: bool = False):
        """(slot or None) of a bucket key, with the LRU / hit-rate bookkeeping; the caller registers a fresh slot under ``key``
        once its first step has returned.  ``allow_promote`` (step_dataset: the batch is collated straight into whatever
        bucket it gets): a bucket that is asked for the FIRST time runs in the smallest live bucket that holds it with at most
        ``promote`` more nodes / edges, if there is one (ghost padding is exact whatever the bucket): recording a launch list
        costs two to three steps, so the rare shapes of a reshuffled epoch - seen once - never pay it, and a shape that comes
        back is recorded on its second visit."""
        slot = self._slots.get(key)
        if slot is None and allow_promote and self.promote > 0:
            seen = self._seen.get(key, 0)
            self._seen[key] = seen + 1
            if seen == 0:
                host = promote_key(self._slots.keys(), key, self.promote)
                if host is not None:
                    self.slot_hits += 1
                    self.slot_promoted += 1
                    self._slots.move_to_end(host)
                    return self._slots[host]
        if slot is None:
            self.slot_misses += 1
            while len(self._slots) >= self.max_slots:          # evict the least recently used bucket
                self._slots.popitem(last=False)
        else:
            self.slot_hits += 1
            self._slots.move_to_end(key)
        return slot


def padded_to_bucket(g, m: GraphMeta, bucket):
    """``g`` ghost-padded to its shape bucket.  Evaluation loops revisit the same batch objects: the padded copy (≈20 small
    torch ops) is cached on the batch, per bucket grid; ``CrystalBatch`` drops it when the batch is written to."""
    cached = getattr(g, "_dosx_padded", None)
    if cached is None or cached[0] != bucket:
        cached = (bucket, pad_batch(g, *bucket_sizes(m.num_nodes, m.num_edges, *bucket)))
        try:
            object.__setattr__(g, "_dosx_padded", cached)
        except (AttributeError, TypeError):
            pass
    return cached[1]
