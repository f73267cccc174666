"""Optimizer parameter groups of the fused trainers: per-group ``lr`` and ``weight_decay`` in the one flat AdamW launch.

``torch.optim.AdamW`` takes a list of group dicts; ``Trainer(param_groups=...)`` (``Trainer64``, ``GraphnetworkTrainer64``) takes
the same list with parameter-name PREFIXES in place of tensors::

    Trainer(model, lr=1e-4, param_groups=[{"params": ["GN_encoder.", "stacked_processor."], "lr": 1e-5},
                                          {"params": param_groups.no_decay(model), "weight_decay": 0.0}])

The flat buffer does not move: every parameter starts on a 64-element boundary (``_fused._ALIGN``), so one byte per 64-element
chunk names its group (:func:`chunk_map`; include/dosx.h: DosxAdamWGroups, dosx_adamw_grouped*), and the kernel looks decay and
step size up per chunk.  This module is the host side - everything in it runs without a GPU:

* :func:`resolve` - the user's list -> ``[{"lr", "weight_decay", "names"}]``, group 0 being the parameters no group names;
* :func:`chunk_map` - a flat layout and an assignment -> the uint8 chunk map;
* :func:`no_decay`, :func:`layerwise`, :func:`with_no_decay` - helpers that only produce such lists.
"""
from __future__ import annotations

import math
import re
from typing import Dict, List, Sequence

import torch
from torch import nn

from . import _abi

MAX_GROUPS = _abi.DOSX_ADAMW_MAX_GROUPS
CHUNK = _abi.DOSX_ADAMW_GROUP_CHUNK


def _live_names(model) -> List[str]:
    return [n for n, _ in model._live_named()]


def _rate(who: str, key: str, value) -> float:
    value = float(value)
    if math.isnan(value) or value < 0.0:
        raise ValueError(f"{who}: {key} must be a non-negative number, got {value}")
    return value


def resolve(model, groups, lr: float, weight_decay: float) -> List[dict]:
    """The user's ``groups`` - dicts ``{"params": prefix | [prefixes], "lr": ..., "weight_decay": ...}`` - resolved against the
    live parameters of ``model`` (frozen ones included, dead ones not): a list of ``{"lr", "weight_decay", "names"}``.

    Entry 0 is the IMPLICIT group: every live parameter no group matches, at the trainer's ``lr`` / ``weight_decay`` (its
    ``names`` may be empty); the user's group ``i`` is entry ``i + 1``.  A missing ``lr`` / ``weight_decay`` inherits the
    trainer's.  Groups with equal values are not merged: the indices stay the user's.  ValueError: a prefix that matches no live
    parameter (naming it - the rule of ``FusedModel.freeze``), a parameter two groups match (naming it and both groups), more
    than ``MAX_GROUPS`` entries with the implicit one, a key other than the three, a NaN or negative value."""
    who = "param_groups"
    groups = list(groups)
    if len(groups) + 1 > MAX_GROUPS:
        raise ValueError(f"{who}: {len(groups)} groups and the implicit one are more than the {MAX_GROUPS} one launch takes")
    names = _live_names(model)
    out = [{"lr": _rate(who, "lr", lr), "weight_decay": _rate(who, "weight_decay", weight_decay), "names": []}]
    owner: Dict[str, int] = {}
    for i, grp in enumerate(groups):
        if not isinstance(grp, dict) or "params" not in grp:
            raise ValueError(f"{who}: group {i} is not a dict with a 'params' entry")
        unknown = sorted(set(grp) - {"params", "lr", "weight_decay"})
        if unknown:
            raise ValueError(f"{who}: group {i} has the key {unknown[0]!r}; a group sets 'lr' and 'weight_decay' only "
                             f"(betas, eps and the step count are shared)")
        prefixes = [grp["params"]] if isinstance(grp["params"], str) else list(grp["params"])
        if not prefixes:
            raise ValueError(f"{who}: group {i} names no prefix")
        mine = []
        for pre in prefixes:
            hit = [n for n in names if n.startswith(pre)] if isinstance(pre, str) else []
            if not hit:
                raise ValueError(f"{who}: prefix {pre!r} of group {i} matches no live parameter")
            mine += [n for n in hit if n not in mine]
        for n in mine:
            if n in owner:
                raise ValueError(f"{who}: parameter {n!r} is matched by group {owner[n]} and by group {i}")
            owner[n] = i
        out.append({"lr": _rate(who, f"lr of group {i}", grp.get("lr", lr)),
                    "weight_decay": _rate(who, f"weight_decay of group {i}", grp.get("weight_decay", weight_decay)),
                    "names": [n for n in names if n in set(mine)]})
    out[0]["names"] = [n for n in names if n not in owner]
    return out


def assignment(resolved: Sequence[dict]) -> Dict[str, int]:
    """name -> index of its entry in a resolved list."""
    return {n: k for k, grp in enumerate(resolved) for n in grp["names"]}


def chunk_map(fp, assign: Dict[str, int]) -> torch.Tensor:
    """The chunk map of a flat layout: a uint8 CPU tensor of ``fp.n_train // CHUNK`` entries, entry ``c`` the group of the
    flat elements ``[CHUNK c, CHUNK c + CHUNK)``.  Every chunk of a trainable parameter, its padded last one included,
    carries that parameter's group (a name the assignment lacks: group 0); frozen parameters lie behind ``n_train`` and have no
    entry.  A pure function of ``fp.names``, ``fp.offsets``, the parameter sizes and the assignment."""
    if fp.n_train % CHUNK:
        raise ValueError(f"chunk_map: n_train = {fp.n_train} is not a multiple of {CHUNK}")
    out = torch.zeros(fp.n_train // CHUNK, dtype=torch.uint8)
    for n, o in zip(fp.names, fp.offsets):
        if o >= fp.n_train:
            continue
        if o % CHUNK:
            raise ValueError(f"chunk_map: parameter {n} starts at {o}, off a {CHUNK}-element boundary")
        k = int(assign.get(n, 0))
        if not 0 <= k < MAX_GROUPS:
            raise ValueError(f"chunk_map: group {k} of parameter {n} is outside [0, {MAX_GROUPS})")
        out[o // CHUNK:(o + fp.P[n].numel() + CHUNK - 1) // CHUNK] = k
    return out


def no_decay(model) -> List[str]:
    """Names of the live parameters transformer practice keeps out of the weight decay: every bias, the weight and bias of every
    ``nn.LayerNorm``, every ``nn.PReLU`` slope, every ``nn.Embedding`` weight (the energy embeddings) and the prompt tokens.  For
    one group: ``{"params": no_decay(model), "weight_decay": 0.0}``."""
    special = set()
    for mn, mod in model.named_modules():
        if isinstance(mod, (nn.LayerNorm, nn.PReLU, nn.Embedding)):
            special.update(f"{mn}.{pn}" if mn else pn for pn, _ in mod.named_parameters(recurse=False))
    prompt = getattr(getattr(model, "_cfg", None), "prompt_key", None)      # (the Electron-DOS reference spells it `promt_token`)
    return [n for n in _live_names(model)
            if n in special or n == "bias" or n.endswith(".bias") or "prompt_token" in n or n == prompt]


_TRUNK = re.compile(r"^(GN_encoder|GN_decoder|stacked_processor\.(\d+))\.")


def layerwise(model, lr: float, decay: float) -> List[dict]:
    """Layer-wise learning-rate decay towards the input, for a model with ``L`` message-passing layers
    (``stacked_processor.0 .. L-1``).  The ladder, top to bottom::

        everything outside the GNN trunk (heads, transformer stacks, embeddings, prompt tokens)    lr
        GN_decoder.                                                                               lr * decay
        stacked_processor.(L-1).                                                                  lr * decay^2
        ...
        stacked_processor.0.                                                                      lr * decay^(L+1)
        GN_encoder.                                                                               lr * decay^(L+2)

    Returns ``L + 3`` groups in that order (groups whose prefix matches no live parameter are left out), each with ``lr`` only:
    the weight decay stays the trainer's."""
    lr, decay = _rate("layerwise", "lr", lr), _rate("layerwise", "decay", decay)
    names = _live_names(model)
    layers = sorted({int(m.group(2)) for m in map(_TRUNK.match, names) if m and m.group(2) is not None})
    L = layers[-1] + 1 if layers else 0
    top = []
    for n in names:
        if _TRUNK.match(n):
            continue
        pre = n.split(".", 1)[0] + "." if "." in n else n
        if pre not in top:
            top.append(pre)
    ladder = [(top, 0), (["GN_decoder."], 1)] + [([f"stacked_processor.{i}."], 1 + L - i) for i in range(L - 1, -1, -1)] + \
             [(["GN_encoder."], L + 2)]
    out = []
    for prefixes, power in ladder:
        prefixes = [p for p in prefixes if any(n.startswith(p) for n in names)]
        if prefixes:
            out.append({"params": prefixes, "lr": lr * decay ** power})
    return out


def with_no_decay(model, groups: Sequence[dict]) -> List[dict]:
    """``groups`` with the :func:`no_decay` names taken out of the weight decay: every group is split into its decayed names and a
    sibling at ``weight_decay = 0`` (same ``lr``), and the no-decay names no group matches form one more group.  What
    ``layerwise`` and ``no_decay`` give together, without one parameter in two groups.  The result names parameters exactly."""
    names, nd = _live_names(model), set(no_decay(model))
    out, seen = [], set()
    for grp in groups:
        prefixes = [grp["params"]] if isinstance(grp["params"], str) else list(grp["params"])
        mine = [n for n in names if n.startswith(tuple(prefixes))]
        seen.update(mine)
        rest = {k: v for k, v in grp.items() if k != "params"}
        keep, drop = [n for n in mine if n not in nd], [n for n in mine if n in nd]
        if keep or not drop:
            out.append({**rest, "params": keep if keep else prefixes})
        if drop:
            out.append({**rest, "params": drop, "weight_decay": 0.0})
    left = [n for n in names if n in nd and n not in seen]
    if left:
        out.append({"params": left, "weight_decay": 0.0})
    return out


# ---- command-line form (examples/train_phonon.py, examples/train_edos.py) -----------------------------------------------------
def parse_group(spec: str) -> dict:
    """``PREFIX[,PREFIX...]:lr=X[:wd=Y]`` (either value, in any order) -> a group dict."""
    head, *rest = spec.split(":")
    prefixes = [p for p in head.split(",") if p]
    grp = {"params": prefixes}
    for item in rest:
        key, _, val = item.partition("=")
        if key not in ("lr", "wd") or not val or ("lr" if key == "lr" else "weight_decay") in grp:
            raise ValueError(f"--group {spec!r}: expected PREFIX[,PREFIX...]:lr=X[:wd=Y], got {item!r}")
        grp["lr" if key == "lr" else "weight_decay"] = float(val)
    if not prefixes or len(grp) == 1:
        raise ValueError(f"--group {spec!r}: expected PREFIX[,PREFIX...]:lr=X[:wd=Y]")
    return grp


def add_arguments(ap) -> None:
    """The three options of the example drivers."""
    ap.add_argument("--group", action="append", default=None, type=parse_group, metavar="PREFIX[,PREFIX...]:lr=X[:wd=Y]",
                    help="fused trainers: an optimizer parameter group - the parameters whose names start with one of the prefixes "
                         "train at this lr / weight decay (repeatable; a missing value is the run's)")
    ap.add_argument("--no-decay-norms", action="store_true",
                    help="fused trainers: no weight decay on biases, LayerNorm weights and biases, PReLU slopes, embeddings and "
                         "prompt tokens (param_groups.no_decay)")
    ap.add_argument("--layerwise-lr-decay", type=float, default=None, metavar="D",
                    help="fused trainers: heads and transformer stacks at --lr, GN_decoder at lr*D, message-passing layer L-1 .. 0 at "
                         "lr*D^2 .. lr*D^(L+1), GN_encoder at lr*D^(L+2) (param_groups.layerwise)")


def wanted(args) -> bool:
    return bool(args.group) or args.no_decay_norms or args.layerwise_lr_decay is not None


def from_args(model, args, lr: float):
    """The ``param_groups=`` of a trainer from the options of :func:`add_arguments` (None: none of them given).  --group lists
    come first, the layer-wise ladder behind them; --no-decay-norms then splits every group (:func:`with_no_decay`)."""
    if not wanted(args):
        return None
    groups = list(args.group or [])
    if args.layerwise_lr_decay is not None:
        groups += layerwise(model, lr, args.layerwise_lr_decay)
    return with_no_decay(model, groups) if args.no_decay_norms else groups
