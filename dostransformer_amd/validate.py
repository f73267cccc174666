"""Batch validation: the fail-loudly path in front of everything that dereferences a batch.

``install_dropin()`` invites foreign PyG batches, ``collate()`` and ``DeviceDataset`` take user dicts - and the kernels index with
what they are given: ``prompt_token[g.system]`` has no range test, every message-passing launch gathers ``edge_index``, the
crystal-aligned tilings assume that no edge joins two crystals, that ``batch`` is sorted and that no crystal is empty.  The
reference raises ``IndexError`` or a device assert in these cases; here :func:`check_batch` does, BEFORE any metadata is derived:

====  ===========================================================================  ========
rule  violation                                                                    offender
====  ===========================================================================  ========
R1    an edge endpoint outside ``[0, N)``                                          edge
R2    both endpoints in range but ``batch[src] != batch[dst]``                     edge
R3    ``batch[i]`` outside ``[0, B)``, or ``batch[i] < batch[i-1]``, or            node
      ``batch[0] != 0``
R4    a crystal in ``[0, B)`` that owns no node                                    crystal
R5    ``system[b]`` outside ``[0, prompts)``                                       crystal
R6    ``n_max`` given and a crystal has more atoms than ``n_max``                  crystal
R7    sorted edges required and ``dst[e] < dst[e-1]``                              edge
====  ===========================================================================  ========

Device tensors are checked by ``dosx_batch_check`` / ``dosx_finite_check_*`` (csrc/validate.hip) with one read-back of the report;
CPU tensors by the numpy twin :func:`check_batch_host`, rule for rule and word for word the same report.  Everything is OFF unless
asked for: :func:`enable` is the process-wide switch that makes ``graph_meta()``, ``collate()`` and ``DeviceDataset`` check what
they are handed (the example drivers turn it on)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi
from ._lib import DosxError

PROMPTS = 7                      # rows of prompt_token in both models (DOSTransformer_phonon.py:21, DOSTransformer.py:20)
NUM_RULES = _abi.DOSX_CHECK_RULES
INT32_MAX = 2 ** 31 - 1
RULE_TEXT = {
    1: "edge endpoint outside [0, N)",
    2: "edge joins two crystals",
    3: "batch vector out of range, unsorted or not starting at 0",
    4: "crystal without atoms",
    5: "crystal-system label outside the prompt table",
    6: "crystal larger than n_max",
    7: "edges not sorted by destination",
}
FINITE_FIELDS = ("x", "edge_vec", "edge_attr", "glob", "phdos", "y_ft")

ENABLED = False                  # validate.enable(): graph_meta / collate / DeviceDataset check what they are handed
FINITE = False                   # ... and the floating-point fields for NaN / inf as well


def enable(on: bool = True, finite: bool = False) -> None:
    """Process-wide switch (off by default: nothing changes unless it is asked for).  On: ``graph_meta()`` checks every batch
    object it derives metadata for, ``collate()`` its concatenated arrays, ``DeviceDataset.__init__`` each crystal's local arrays."""
    global ENABLED, FINITE
    ENABLED, FINITE = bool(on), bool(on and finite)


def empty_report(slots: int = NUM_RULES) -> np.ndarray:
    """``slots`` {count, first} pairs in their initial state {0, INT32_MAX}."""
    w = np.zeros(2 * slots, np.int32)
    w[1::2] = INT32_MAX
    return w


class Report:
    """What a check found: ``words`` = the rules' {count, first} pairs (rule r at words[2(r-1)]), then one pair per entry of
    ``fields`` (the finite checks).  ``count`` saturates at INT32_MAX; ``first`` is the smallest offending index, INT32_MAX if none."""

    def __init__(self, words: np.ndarray, fields: Sequence[str] = ()):
        self.words = np.asarray(words, np.int32)
        self.fields = tuple(fields)
        assert self.words.shape == (2 * (NUM_RULES + len(self.fields)),)

    def count(self, rule: int) -> int:
        return int(self.words[2 * (rule - 1)])

    def first(self, rule: int) -> int:
        return int(self.words[2 * (rule - 1) + 1])

    def nonfinite(self, field: str) -> Tuple[int, int]:
        k = 2 * (NUM_RULES + self.fields.index(field))
        return int(self.words[k]), int(self.words[k + 1])

    @property
    def ok(self) -> bool:
        return not self.words[0::2].any()

    def __repr__(self):
        bad = [f"R{r}: {self.count(r)} (first {self.first(r)})" for r in range(1, NUM_RULES + 1) if self.count(r)]
        bad += [f"{f}: {self.nonfinite(f)[0]} non-finite (first {self.nonfinite(f)[1]})" for f in self.fields if self.nonfinite(f)[0]]
        return f"Report({', '.join(bad) if bad else 'clean'})"


def check_batch_host(edge_index, batch, system=None, num_graphs: Optional[int] = None, n_max: Optional[int] = None,
                     require_sorted: bool = False, prompts: int = PROMPTS) -> np.ndarray:
    """The numpy twin of ``dosx_batch_check``: int32 [2 * NUM_RULES] = {count, first} per rule."""
    ei = np.asarray(edge_index).astype(np.int64).reshape(2, -1)
    bv = np.asarray(batch).astype(np.int64).reshape(-1)
    N, E = int(bv.shape[0]), int(ei.shape[1])
    sysv = None if system is None else np.asarray(system).astype(np.int64).reshape(-1)
    B = int(num_graphs) if num_graphs is not None else (int(sysv.shape[0]) if sysv is not None else (int(bv.max()) + 1 if N else 0))
    rep = empty_report()

    def put(rule, mask):
        idx = np.flatnonzero(mask)
        if idx.size:
            rep[2 * (rule - 1)] = min(int(idx.size), INT32_MAX)
            rep[2 * (rule - 1) + 1] = min(int(idx[0]), INT32_MAX - 1)

    src, dst = ei[0], ei[1]
    r1 = (src < 0) | (src >= N) | (dst < 0) | (dst >= N)
    put(1, r1)
    r2 = np.zeros(E, bool)
    okk = ~r1
    r2[okk] = bv[src[okk]] != bv[dst[okk]]          # batch[src] is read only behind src's range test
    put(2, r2)
    r3 = (bv < 0) | (bv >= B)
    if N:
        r3[0] |= bv[0] != 0
        r3[1:] |= bv[1:] < bv[:-1]
    put(3, r3)
    counts = np.bincount(bv[~((bv < 0) | (bv >= B))], minlength=B)[:B] if B else np.zeros(0, np.int64)
    put(4, counts == 0)
    if sysv is not None:
        if sysv.shape[0] != B:
            raise ValueError(f"system has {sysv.shape[0]} entries for {B} crystals")
        put(5, (sysv < 0) | (sysv >= prompts))
    if n_max:
        put(6, counts > int(n_max))
    if require_sorted and E:
        r7 = np.zeros(E, bool)
        r7[1:] = dst[1:] < dst[:-1]
        put(7, r7)
    return rep


def _num_graphs(g, bv, system) -> int:
    ng = getattr(g, "num_graphs", None)
    if isinstance(ng, (int, np.integer)):
        return int(ng)
    if system is not None:
        return int(system.shape[0])
    return int(bv.max()) + 1 if bv.numel() else 0          # (a read of the device when nothing else says it)


def _field(g, name):
    try:
        v = g[name] if name in g else None
    except TypeError:
        v = getattr(g, name, None)
    return v if torch.is_tensor(v) else None


def finite_check_device(t: torch.Tensor, slot: torch.Tensor) -> None:
    """Count the non-finite elements of a contiguous fp32 / float64 device tensor into ``slot`` ({count, first}, int32, on the device)."""
    from . import ops
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"finite check: fp32 or float64 tensors, got {t.dtype}")
    if not t.is_contiguous():
        t = t.contiguous()
    ops._call("dosx_finite_check_f32" if t.dtype == torch.float32 else "dosx_finite_check_f64", t.data_ptr(), t.numel(),
              slot.data_ptr(), ops._stream(), w=lambda: ("finite_check", "finite_check_kernel", "hbm", float(t.numel() * t.element_size())))


def batch_check_device(edge_index: torch.Tensor, batch: torch.Tensor, system: Optional[torch.Tensor], num_graphs: int,
                       n_max: Optional[int], require_sorted: bool, report: torch.Tensor, prompts: int = PROMPTS) -> None:
    """One ``dosx_batch_check`` call on int64 device tensors; ``report``: int32 device words initialised by :func:`empty_report`."""
    from . import _lib, ops
    assert edge_index.is_cuda and edge_index.dtype == torch.int64 and batch.dtype == torch.int64 and edge_index.dim() == 2
    ei, bv = edge_index.contiguous(), batch.contiguous()
    d = _lib.BatchCheck()
    d.N, d.E, d.B = int(bv.shape[0]), int(ei.shape[1]), int(num_graphs)
    d.n_max, d.prompts, d.require_sorted = int(n_max or 0), int(prompts), int(bool(require_sorted))
    d.edge_index = ei.data_ptr() if d.E else None
    d.batch = bv.data_ptr() if d.N else None
    sv = None
    if system is not None:
        if int(system.shape[0]) != d.B:
            raise ValueError(f"system has {int(system.shape[0])} entries for {d.B} crystals")
        sv = system.to(torch.int64).contiguous()
        d.system = sv.data_ptr() if d.B else None
    cnt = torch.empty(max(d.B, 1), dtype=torch.int32, device=ei.device)
    d.crystal_count = cnt.data_ptr()
    ops._call("dosx_batch_check", C.byref(d), report.data_ptr(), ops._stream(),
              w=lambda: ("batch_check", "batch_check_kernel", "hbm", 16.0 * d.E + 8.0 * d.N))


def _value(t, *idx):
    return int(t[idx].item())


def describe(rule: int, first: int, count: int, ei, bv, system, B: int, n_max, prompts: int = PROMPTS) -> str:
    """The message of a violated rule: the rule, how often, the first offender and its value."""
    N = int(bv.shape[0])
    head = f"R{rule} ({RULE_TEXT[rule]}), {count} violation{'s' if count != 1 else ''}; first: "
    if rule == 1:
        s, d = _value(ei, 0, first), _value(ei, 1, first)
        which, v = ("source", s) if (s < 0 or s >= N) else ("destination", d)
        return head + f"edge {first}: {which} {v} outside [0, {N})"
    if rule == 2:
        s, d = _value(ei, 0, first), _value(ei, 1, first)
        return head + f"edge {first}: source {s} is in crystal {_value(bv, s)}, destination {d} in crystal {_value(bv, d)}"
    if rule == 3:
        v = _value(bv, first)
        if v < 0 or v >= B:
            return head + f"node {first}: batch {v} outside [0, {B})"
        if first == 0:
            return head + f"node 0: batch {v}, must be 0"
        return head + f"node {first}: batch {v} below batch {_value(bv, first - 1)} of node {first - 1}"
    if rule == 4:
        return head + f"crystal {first}: owns no node"
    if rule == 5:
        return head + f"crystal {first}: system {_value(system, first)} outside [0, {prompts})"
    if rule == 6:
        return head + f"crystal {first}: {int((bv == first).sum().item())} atoms, n_max {int(n_max)}"
    return head + f"edge {first}: destination {_value(ei, 1, first)} below destination {_value(ei, 1, first - 1)} of edge {first - 1}"


def check_batch(g, n_max: Optional[int] = None, require_sorted: bool = False, finite: bool = False, raise_: bool = True) -> Report:
    """Check a batch object (``edge_index``, ``batch``, optional ``system`` and the floating-point fields) against R1-R7, and with
    ``finite`` its ``x``, ``edge_vec`` / ``edge_attr``, ``glob``, ``phdos`` / ``y_ft`` (fp32 or float64 as they are) for NaN / inf.
    Device tensors: the kernels and ONE read-back of the report; CPU tensors: the numpy twin.  A violation raises
    :class:`DosxError` naming rule, count, first offender and its value (``raise_=False``: only the :class:`Report`)."""
    ei, bv = g.edge_index, g.batch
    if not (torch.is_tensor(ei) and torch.is_tensor(bv)) or ei.dim() != 2 or ei.shape[0] != 2 or bv.dim() != 1:
        raise DosxError(f"check_batch: edge_index must be a [2, E] tensor and batch a [N] tensor, got "
                        f"{tuple(getattr(ei, 'shape', ()))} and {tuple(getattr(bv, 'shape', ()))}")
    system = getattr(g, "system", None)
    system = system if torch.is_tensor(system) and system.dim() > 0 else None
    B = _num_graphs(g, bv, system)
    fields = []
    if finite:
        for k in FINITE_FIELDS:
            t = _field(g, k)
            if t is not None and t.is_floating_point():
                fields.append((k, t))
    names = tuple(k for k, _ in fields)
    if ei.is_cuda:
        rep_dev = torch.from_numpy(empty_report(NUM_RULES + len(fields))).to(ei.device)
        batch_check_device(ei.to(torch.int64), bv.to(torch.int64), system, B, n_max, require_sorted, rep_dev)
        for i, (k, t) in enumerate(fields):
            finite_check_device(t, rep_dev[2 * (NUM_RULES + i):])
        words = rep_dev.cpu().numpy()                      # the one read-back
    else:
        words = empty_report(NUM_RULES + len(fields))
        words[:2 * NUM_RULES] = check_batch_host(ei.numpy(), bv.numpy(), None if system is None else system.numpy(), B, n_max,
                                                 require_sorted)
        for i, (k, t) in enumerate(fields):
            bad = np.flatnonzero(~np.isfinite(t.detach().reshape(-1).numpy()))
            if bad.size:
                words[2 * (NUM_RULES + i):2 * (NUM_RULES + i) + 2] = (min(int(bad.size), INT32_MAX), min(int(bad[0]), INT32_MAX - 1))
    rep = Report(words, names)
    if raise_ and not rep.ok:
        msgs = [describe(r, rep.first(r), rep.count(r), ei, bv, system, B, n_max) for r in range(1, NUM_RULES + 1) if rep.count(r)]
        for k, t in fields:
            c, f = rep.nonfinite(k)
            if c:
                msgs.append(f"{k}: {c} non-finite element{'s' if c != 1 else ''}; first: element {f} = {float(t.reshape(-1)[f].item())}")
        raise DosxError("invalid batch: " + " | ".join(msgs))
    return rep
