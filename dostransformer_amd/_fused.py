"""Glue between ``torch.nn.Module`` parameter storage / autograd and the libdosx programs in
``functional.py``.

* live parameters are re-homed (lazily, on the device the module lives on) into ONE flat fp32
  buffer, with a same-shaped flat gradient buffer — the layout the fused AdamW kernel and the
  data-parallel RCCL all-reduce want.  ``state_dict()`` keys/shapes are unchanged.
* parameters the reference never uses (``self_attn.in_proj_*``, ``self_attn.out_proj.*``,
  ``node_mlp_1.*``, ``alpha`` — SURVEY.md §0.2/§0.6) stay outside: they get ``grad = None`` and are
  therefore skipped by AdamW exactly like upstream.
* fine-tuning: ``requires_grad`` is read when the buffer is laid out - trainable parameters first, frozen ones behind them
  (``FlatParams.n_train``); a frozen parameter keeps its views, gets ``grad = None`` and is stepped by nobody
  (``FusedModel.freeze`` / ``train_only`` / ``update_trainable``).
* one ``torch.autograd.Function`` spans the whole model: forward runs the forward program and keeps
  its activations, backward runs the backward program and publishes ``param.grad`` as views of the
  flat gradient buffer (no per-parameter copies).
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import functional as Fn
from . import ops
from ._lib import DosxError
from .batch import GraphMeta, graph_meta

_DEAD = re.compile(r"(\.self_attn\.)|(\.node_mlp_1\.)|(^alpha$)")
_ALIGN = 64   # floats; keeps every parameter 256-B aligned inside the flat buffer


def is_dead_param(name: str) -> bool:
    return _DEAD.search(name) is not None


_LATE = ("GN_encoder.", "stacked_processor.", "GN_decoder.")
_LAST = ("GN_encoder.", "stacked_processor.0.")


def is_late_param(name: str) -> bool:
    """Parameters of the GNN trunk: their gradients are complete only at the very end of the backward pass.  All
    others (transformer stacks, heads, embeddings) are final once the backward reaches the GNN, so their slice of
    the flat gradient buffer can be all-reduced while the GNN backward still runs (dist / train.Trainer)."""
    return name.startswith(_LATE)


def is_last_param(name: str) -> bool:
    """The part of the GNN trunk whose gradients exist only at the END of the backward pass: the node / edge / global encoders and
    message-passing layer 0.  The rest of the trunk (GN_decoder, layers 1 .. L-1: the MID bucket) is final once the backward reaches
    layer 0 - its all-reduce starts there, under layer 0's backward, and only this bucket stays exposed behind the step."""
    return name.startswith(_LAST)


class GradViews(dict):
    """The gradient views of a :class:`FlatParams`, name -> view, with the frozen set the backward programs prune by
    (functional: ``wgrad_needed`` / ``trunk_cut`` / ``first_encoder_cut``).  The two cuts are decided once, when the views are
    made: the per-step path reads two attributes and scans nothing."""

    def __init__(self, views, frozen=()):
        super().__init__(views)
        self.frozen = frozenset(frozen)
        self.cut_trunk = Fn.trunk_cut(self.keys(), self.frozen)
        self.cut_first = Fn.first_encoder_cut(self.keys(), self.frozen)


def frozen_live_names(module: nn.Module, extra_dead=()) -> frozenset:
    """Names of the live parameters whose ``requires_grad`` is off (one scan of the module: not for the per-step path)."""
    return frozenset(n for n, p in module.named_parameters()
                     if not p.requires_grad and not (is_dead_param(n) or n in extra_dead))


class FlatParams:
    """Flat parameter + gradient storage for the live parameters of a module: fp32, or fp64 for a module that runs the
    float64 program (FusedModel._flat_dtype).

    ``requires_grad`` is read HERE, once: the trainable parameters come first, ``flat[:n_train]``, the frozen ones behind them.
    Everything that steps or measures "the gradient" takes ``(buffer, n_train)``; a frozen parameter keeps its ``P`` view (the
    forward reads it) and its ``G`` view (fused launches write partial rows there: no null destinations) and nothing reads
    the latter.  ``frozen`` is the snapshot; ``FusedModel.update_trainable()`` takes a new one."""

    def __init__(self, module: nn.Module, device: torch.device, extra_dead=(), dtype: torch.dtype = torch.float32):
        live = [(n, p) for n, p in module.named_parameters() if not (is_dead_param(n) or n in extra_dead)]
        frozen = [x for x in live if not x[1].requires_grad]
        live = [x for x in live if x[1].requires_grad]
        # layout: [ last bucket (encoders + layer 0) | mid bucket (rest of the GNN trunk) | early bucket (everything else) ],
        # each in module order; [last | mid] together are the "late" slice flat[:n_late]; then the frozen parameters
        ordered = [x for x in live if is_last_param(x[0])] + [x for x in live if is_late_param(x[0]) and not is_last_param(x[0])] + \
                  [x for x in live if not is_late_param(x[0])]
        n_live = len(ordered)
        ordered += frozen
        names, params = [n for n, _ in ordered], [p for _, p in ordered]
        offs, tot, n_late, n_last, n_train = [], 0, 0, 0, 0
        for i, (n, p) in enumerate(ordered):
            offs.append(tot)
            tot += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
            if i < n_live:
                n_train = tot
                if is_late_param(n):
                    n_late = tot
                if is_last_param(n):
                    n_last = tot
        self.names, self.offsets, self.total = names, offs, tot
        self.n_train = n_train        # floats: flat[:n_train] the trainable parameters, flat[n_train:] the frozen ones
        self.frozen = frozenset(n for n, _ in frozen)
        self.n_late = n_late          # floats: flat[:n_late] is the GNN trunk, flat[n_late:] the early bucket
        self.n_last = n_last          # floats: flat[:n_last] the last bucket, flat[n_last:n_late] the mid bucket
        self.dtype = dtype
        self.flat = torch.zeros(tot, device=device, dtype=dtype)
        self.grad = torch.zeros(tot, device=device, dtype=dtype)
        self.P: Dict[str, torch.Tensor] = {}
        G: Dict[str, torch.Tensor] = {}
        self.params: Dict[str, nn.Parameter] = {}
        with torch.no_grad():
            for n, p, o in zip(names, params, offs):
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.detach().to(device=device, dtype=dtype))
                p.data = view
                self.P[n] = view
                G[n] = self.grad[o:o + p.numel()].view(p.shape)
                self.params[n] = p
        self.G = GradViews(G, self.frozen)
        for n, p in module.named_parameters():       # dead parameters just follow the module's device
            if n not in self.P and p.device != device:
                p.data = p.data.to(device)
        self.anchor = params[0]
        self.anchor_ptr = self.flat.data_ptr() + self.flat.element_size() * offs[0]

    def intact(self, device: torch.device) -> bool:
        return self.flat.device == device and self.anchor.data_ptr() == self.anchor_ptr and \
            self.anchor.dtype == self.dtype

    def trainable_names(self) -> List[str]:
        return [n for n in self.names if n not in self.frozen]

    def publish_grads(self, G: Dict[str, torch.Tensor], accumulate_into_existing: bool) -> None:
        """``param.grad`` of the trainable parameters; a frozen one keeps ``grad is None``, as under autograd."""
        frozen = self.frozen
        for n, p in self.params.items():
            if n in frozen:
                continue
            if p.grad is None or not accumulate_into_existing:
                p.grad = G[n]
            else:
                p.grad = p.grad + G[n]


class _ModelFn(torch.autograd.Function):
    """Whole-model autograd node (see module docstring)."""

    @staticmethod
    def forward(ctx, anchor, model, g, m):
        fp: FlatParams = model._flat
        out = model._program_fwd(fp.P, g, m)
        ctx.model, ctx.m, ctx.saved, ctx.fp = model, m, out[-1], fp
        res = out[:-1]
        ctx.n_out = len(res)
        ctx.set_materialize_grads(False)
        return res

    @staticmethod
    def backward(ctx, *grads):
        model, fp = ctx.model, ctx.fp
        busy = any(p.grad is not None for p in fp.params.values())
        if busy:
            # true accumulation (two backward() calls without zero_grad): use a scratch gradient buffer
            gbuf = torch.zeros_like(fp.grad)
            G = GradViews({n: gbuf[o:o + fp.P[n].numel()].view(fp.P[n].shape) for n, o in zip(fp.names, fp.offsets)}, fp.frozen)
        else:
            G = fp.G
        sink = ops.GradSink(fp.flat.device)
        model._program_bwd(fp.P, G, ctx.m, ctx.saved, grads, sink)
        sink.release()
        fp.publish_grads(G, busy)
        ctx.saved = None
        return None, None, None, None


class FusedModel(nn.Module):
    """Base class of the drop-in model modules: lazily flattens parameters and routes forward /
    backward through the libdosx programs."""

    _flat: Optional[FlatParams] = None
    _has_f64_program = False      # a float64 phonon module of this class runs functional64 (else: the fp32 program, as before)

    def _extra_dead(self, g) -> Tuple[str, ...]:
        return ()

    def _flat_dtype(self, g=None) -> torch.dtype:
        """float64 for a Graphnetwork_phonon whose live parameters are all float64 (the reference's phonon setup,
        main_phDOS.py:15-16), float32 otherwise - as before for every other module: eDOS modules compute in fp32 whatever
        their dtype (their reference is fp32, data/mat2graph.py:127-131), and DOSTransformer_phonon has no float64 program
        yet, so a float64 one keeps today's fp32 computation with float64 outputs.  Raises DosxError where a module that
        would run the float64 program cannot."""
        if not self._has_f64_program or self._cfg.kind != "phonon":
            return torch.float32
        dead = self._extra_dead(g)
        dts = {p.dtype for n, p in self.named_parameters() if not (is_dead_param(n) or n in dead)}
        if torch.float64 not in dts:
            return torch.float32
        name = type(self).__name__
        if len(dts) > 1:
            raise DosxError(f"{name}: live parameters mix {sorted(str(d) for d in dts)}; a float64 module needs all of them "
                            f"float64 (.double())")
        from .functional64 import MAX_HIDDEN
        if self._cfg.H > MAX_HIDDEN:
            raise DosxError(f"{name}: the float64 program takes hidden <= {MAX_HIDDEN}, got {self._cfg.H}")
        return torch.float64

    def _wanted_flat_dtype(self) -> Optional[torch.dtype]:
        """The flat dtype a module's program switch asks for (DOSTransformerBase.set_program_dtype), None: no switch."""
        return None

    def _ensure_flat(self, device: torch.device, g) -> FlatParams:
        dead = self._extra_dead(g)
        fp = self._flat
        want = self._wanted_flat_dtype()
        if fp is None or not fp.intact(device) or getattr(self, "_flat_dead", ()) != dead or (want is not None and fp.dtype != want):
            fp = FlatParams(self, device, dead, self._flat_dtype(g))
            object.__setattr__(self, "_flat", fp)
            object.__setattr__(self, "_flat_dead", dead)
        return fp

    def _module_device(self) -> torch.device:
        return next(self.parameters()).device

    def flat_params(self, g=None) -> FlatParams:
        return self._ensure_flat(self._module_device(), g)

    # ---- fine-tuning: which parameters train (host only) ---------------------------------------------------------------
    # ``requires_grad`` is the single source of truth.  It is READ when the flat buffer is built or rebuilt and by
    # update_trainable(); no step scans the parameters.  freeze() / train_only() call update_trainable() themselves; after a bare
    # ``p.requires_grad_(...)`` the caller does, and a trainer's check() reports a snapshot that went stale.
    def _live_named(self):
        dead = getattr(self, "_flat_dead", ())
        return [(n, p) for n, p in self.named_parameters() if not (is_dead_param(n) or n in dead)]

    def _match(self, who: str, prefixes) -> None:
        if not prefixes:
            raise ValueError(f"{type(self).__name__}.{who}: no prefix given")
        names = [n for n, _ in self._live_named()]
        for pre in prefixes:
            if not isinstance(pre, str) or not any(n.startswith(pre) for n in names):
                raise ValueError(f"{type(self).__name__}.{who}: prefix {pre!r} matches no live parameter")

    def freeze(self, *prefixes: str):
        """``requires_grad_(False)`` on every live parameter whose name starts with one of ``prefixes`` (a prefix that matches
        none raises ValueError naming it), then update_trainable().  Returns self."""
        self._match("freeze", prefixes)
        for n, p in self._live_named():
            if n.startswith(tuple(prefixes)):
                p.requires_grad_(False)
        self.update_trainable()
        return self

    def train_only(self, *prefixes: str):
        """Exactly the live parameters whose name starts with one of ``prefixes`` train, every other one is frozen (a prefix
        that matches none raises ValueError naming it), then update_trainable().  Returns self."""
        self._match("train_only", prefixes)
        for n, p in self._live_named():
            p.requires_grad_(n.startswith(tuple(prefixes)))
        self.update_trainable()
        return self

    def trainable_names(self) -> List[str]:
        """Names of the live parameters that train, in module order (read from ``requires_grad``, not from the snapshot)."""
        return [n for n, p in self._live_named() if p.requires_grad]

    def update_trainable(self) -> bool:
        """Re-read ``requires_grad`` and rebuild the flat buffer if the frozen set changed (values are carried over; a trainer
        re-homes its moments by name and drops its recorded slots at its next step).  True: rebuilt.  Nothing to do before the
        first forward: the buffer is laid out from the flags when it is built."""
        fp = self._flat
        if fp is None:
            return False
        dead = getattr(self, "_flat_dead", ())
        if frozen_live_names(self, dead) == fp.frozen:
            return False
        new = FlatParams(self, fp.flat.device, dead, fp.dtype)
        object.__setattr__(self, "_flat", new)
        return True

    def trainable_stale(self) -> bool:
        """True: ``requires_grad`` changed since the flat buffer was laid out and update_trainable() has not run (one scan)."""
        fp = self._flat
        return fp is not None and frozen_live_names(self, getattr(self, "_flat_dead", ())) != fp.frozen

    def _run(self, g):
        dev = self._module_device()
        if dev.type != "cuda":
            raise RuntimeError(
                f"{type(self).__name__} runs only on an MI355X through libdosx (no CPU fallback): "
                f"move the module with .to('cuda') first (it is on {dev}).")
        fp = self._ensure_flat(dev, g)
        m = graph_meta(g, dev)
        if torch.is_grad_enabled():
            out = _ModelFn.apply(fp.anchor, self, g, m)
        else:
            out = self._program_fwd(fp.P, g, m)[:-1]
        if fp.dtype == torch.float64:
            return out              # the float64 program: float64 outputs whatever the batch dtype
        # The kernels compute in fp32.  A float64 batch (the phonon reference sets the default dtype to float64,
        # main_phDOS.py:15-16) gets float64 outputs back, like upstream: the caller's MSELoss against its float64 target
        # then back-propagates a float64 gradient, which this (autograd-aware) cast turns into the fp32 one the backward
        # program takes.
        dt = g.x.dtype if torch.is_tensor(getattr(g, "x", None)) else torch.float32
        if dt.is_floating_point and dt != torch.float32:
            out = tuple(t.to(dt) for t in out)
        return out
