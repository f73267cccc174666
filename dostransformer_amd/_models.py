"""Shared implementation of the four drop-in model classes (phonon / eDOS x DOSTransformer /
Graphnetwork).  The public modules under ``embedder_phDOS`` / ``embedder_eDOS`` only fix the
constructor signatures and parameter creation order of their reference counterparts."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import functional as Fn
from . import functional64 as F64
from ._fused import FusedModel, is_dead_param
from ._lib import DosxError


_SEED_MOD = 2 ** 62


def rank_seed_offset() -> int:
    """What a data-parallel rank adds to the (rank-independent) dropout base seed: ranks seeded alike must not draw the
    same masks for their different shards.  0 outside torch.distributed."""
    import torch.distributed as td
    if td.is_available() and td.is_initialized():
        return (0x9E3779B97F4A7C15 * (td.get_rank() + 1)) % _SEED_MOD
    return 0


def dos_device(P):
    return P["embeddings.weight"].device


class DOSTransformerBase(FusedModel):
    """forward(g) -> (dos_global [B,S], x [N,H], dos_system [B,S])   (`DOSTransformer_phonon.py:66-119`)."""
    _cfg: Fn.ModelCfg
    _program_dtype = torch.float32
    _per_crystal_keys = False

    # ---- which program the module runs ----------------------------------------------------------------------------------
    @property
    def program_dtype(self) -> torch.dtype:
        """The dtype the next forward computes in: torch.float32 (the default, whatever the parameters' dtype) or
        torch.float64 after set_program_dtype(torch.float64) (functional64: the phonon reference's float64 training)."""
        return self._program_dtype

    def set_program_dtype(self, dtype: torch.dtype):
        """Select the fp32 program (torch.float32, the default) or the float64 one (torch.float64: DOSTransformer_phonon
        with float64 live parameters and hidden <= functional64.MAX_HIDDEN).  The flat parameters are re-homed on the next
        call.  Returns self."""
        if dtype == torch.float64:
            self._check_f64_program()
        elif dtype != torch.float32:
            raise DosxError(f"{type(self).__name__}.set_program_dtype: torch.float32 or torch.float64, got {dtype}")
        object.__setattr__(self, "_program_dtype", dtype)
        if dtype != torch.float64:
            object.__setattr__(self, "_per_crystal_keys", False)        # a switch of the float64 program only
        return self

    @property
    def per_crystal_keys(self) -> bool:
        """True: the float64 program attends over each crystal's own atoms (set_per_crystal_keys)."""
        return self._per_crystal_keys

    def set_per_crystal_keys(self, flag: bool):
        """float64 program only.  True: the two encoders that attend over atoms (transformer, transformer_source) see each
        crystal's own atoms, not the rows that pad it to the batch's largest crystal, so a batch of B crystals gives the B
        DOS vectors the reference gives at batch_size = 1 (main_phDOS.py:52-55) and its gradient is the sum of those B
        per-sample gradients - forward and backward, attention dropout included.  False (the default): the reference's
        batched forward, padding rows as keys.  Returns self."""
        if flag and self._program_dtype != torch.float64:
            raise DosxError(f"{type(self).__name__}.set_per_crystal_keys: a switch of the float64 program "
                            f"(set_program_dtype(torch.float64), DOSTransformer_phonon only); the fp32 program has it as "
                            f"Predictor(model, per_crystal_keys=True) and Trainer(model, per_crystal_keys=True)")
        object.__setattr__(self, "_per_crystal_keys", bool(flag))
        return self

    def _check_f64_program(self) -> None:
        name = type(self).__name__
        if self._cfg.kind != "phonon":
            raise DosxError(f"{name}: only DOSTransformer_phonon has a float64 program (the eDOS reference trains in fp32)")
        dts = {p.dtype for n, p in self.named_parameters() if not is_dead_param(n)}
        if dts != {torch.float64}:
            raise DosxError(f"{name}: the float64 program needs every live parameter float64 (.double()), got "
                            f"{sorted(str(d) for d in dts)}")
        if self._cfg.H > F64.MAX_HIDDEN:
            raise DosxError(f"{name}: the float64 program takes hidden <= {F64.MAX_HIDDEN}, got {self._cfg.H}")

    def _flat_dtype(self, g=None) -> torch.dtype:
        if self._program_dtype != torch.float64:
            return torch.float32
        self._check_f64_program()
        return torch.float64

    def _wanted_flat_dtype(self):
        return self._program_dtype

    def _require_fp32_program(self, who: str) -> None:
        """The drivers that run the fp32 program on the flat buffer (train.Trainer, predict.Predictor) refuse a module set to
        float64."""
        if self._program_dtype == torch.float64:
            raise DosxError(f"{who} runs the fp32 program; {type(self).__name__} is set to float64 (set_program_dtype): train "
                            f"it with train64.Trainer64, or with model(batch), loss.backward() and torch.optim.AdamW")

    def _require_f64_program(self, who: str) -> None:
        """The drivers of the float64 program (train64.Trainer64, predict.Predictor64) take a DOSTransformer_phonon set to it and
        nothing else; called on the class (``DOSTransformerBase._require_f64_program(model, who)``) for whatever they are given."""
        ours = isinstance(self, DOSTransformerBase)
        if not (ours and self._cfg.kind == "phonon" and self._program_dtype == torch.float64):
            raise DosxError(f"{who} drives a DOSTransformer_phonon set to the float64 program "
                            f"(model.double().set_program_dtype(torch.float64)), got {type(self).__name__}"
                            + (f" with program_dtype {self._program_dtype}" if ours else "")
                            + ": the fp32 program is train.Trainer's / predict.Predictor's"
                            + ("; a float64 Graphnetwork_phonon is train64.GraphnetworkTrainer64's / predict.Predictor64's"
                               if isinstance(self, GraphnetworkBase) else ""))

    def _check_train_flags(self):
        pass          # (kept for callers of round 1: attention dropout is implemented now)

    # ---- attention dropout (`utils.py:40` --attn_drop -> TransformerEncoder(attn_dropout=...), multihead_attention.py:70)
    def _dropout(self, device, bump: bool):
        """None in eval mode / p = 0, else (p, seed_dev).  The seed lives in a device scalar so that a recorded program
        draws fresh masks on every replay; it starts from torch's RNG (follows torch.manual_seed) and is bumped once per
        forward pass (``bump``: the autograd path; train.Trainer bumps it itself, outside the recorded program)."""
        p = float(getattr(self, "_attn_drop", 0.0) or 0.0)
        if not self.training or p <= 0.0:
            return None
        seed = getattr(self, "_drop_seed", None)
        if seed is None or seed.device != device:
            val = (int(torch.randint(0, _SEED_MOD, (1,), dtype=torch.int64).item()) + rank_seed_offset()) % _SEED_MOD
            seed = torch.tensor([val], dtype=torch.int64).to(device)
            object.__setattr__(self, "_drop_seed", seed)
        elif bump:
            seed.add_(1)
        return p, seed

    def _program_fwd(self, P, g, m, bump_seed: bool = True, per_crystal_keys: bool = False):
        if P["embeddings.weight"].dtype == torch.float64:
            # (the per_crystal_keys argument is predict.Predictor's and train.Trainer's and reaches the fp32 program only: the
            #  float64 program follows the module's own switch)
            dos, xL, ctx = F64.dostransformer_phonon_fwd(P, self._cfg, g, m, drop=self._dropout(dos_device(P), bump_seed),
                                                         per_crystal_keys=self._per_crystal_keys)
            B = m.num_graphs
            return dos[:B], xL, dos[B:], (ctx, dos)
        dos, xL, ctx = Fn.dostransformer_fwd(P, self._cfg, g, m, drop=self._dropout(dos_device(P), bump_seed),
                                             per_crystal_keys=per_crystal_keys)
        B = m.num_graphs
        return dos[:B], xL, dos[B:], (ctx, dos)

    def _program_bwd(self, P, G, m, saved, grads, sink):
        ctx, dos = saved
        dg, dx, ds = grads
        B = m.num_graphs
        ddos = torch.zeros_like(dos)
        if dg is not None:
            ddos[:B].copy_(dg)
        if ds is not None:
            ddos[B:].copy_(ds)
        if dos.dtype == torch.float64:
            F64.dostransformer_phonon_bwd(P, G, self._cfg, m, ctx, ddos, dx)
            return
        Fn.dostransformer_bwd(P, G, self._cfg, m, ctx, ddos, None if dx is None else dx.float().contiguous(), sink)

    def forward(self, g):
        self._check_train_flags()
        return self._run(g)


class GraphnetworkBase(FusedModel):
    _cfg: Fn.ModelCfg
    _returns_x: bool
    _has_f64_program = True       # Graphnetwork_phonon (the kind check of _flat_dtype keeps the eDOS Graphnetwork in fp32)

    def _extra_dead(self, g) -> Tuple[str, ...]:
        # Encoder picks node_encoder or node_encoder_prompt by input width
        # (graphnetwork_phonon.py:150-153, graphnetwork.py:96-99); the other one is dead for this run.
        expected = 118 if self._cfg.kind == "phonon" else 200
        width = g.x.shape[1] if g is not None else expected
        unused = "GN_encoder.node_encoder_prompt" if width == expected else "GN_encoder.node_encoder"
        return tuple(f"{unused}.{s}" for s in ("0.weight", "0.bias", "1.weight", "2.weight", "2.bias"))

    # the fp32 programs of this family (functional.graphnetwork_fwd / _bwd; embedder_eDOS.mlp overrides them)
    _fwd_fn = staticmethod(Fn.graphnetwork_fwd)

    @staticmethod
    def _bwd_fn(P, G, cfg, m, saved, ddos, dx, sink, factored_head=False):
        Fn.graphnetwork_bwd(P, G, cfg, m, saved, ddos, dx, sink, factored_head=factored_head)

    # A crystal's outputs do not depend on its batch mates: no dense key batch, no attention (evaluate.test_per_crystal)
    batch_independent = True

    def _require_fp32_program(self, who: str) -> None:
        """train.Trainer / predict.Predictor run the fp32 program on the flat buffer: a float64 Graphnetwork_phonon (float64
        live parameters: functional64) is train64.GraphnetworkTrainer64's and predict.Predictor64's."""
        if self._flat_dtype(None) == torch.float64:
            raise DosxError(f"{who} runs the fp32 program; this {type(self).__name__} has float64 parameters and runs the "
                            f"float64 one: train it with train64.GraphnetworkTrainer64 and predict with predict.Predictor64")

    def _require_f64_baseline(self, who: str) -> None:
        """The float64 drivers of the GNN-only baseline (train64.GraphnetworkTrainer64, predict.Predictor64) take a
        Graphnetwork_phonon whose live parameters are all float64 (``model.double()``) and whose hidden width the float64 program
        takes, and nothing else; called on the class (``GraphnetworkBase._require_f64_baseline(model, who)``) for whatever they
        are given."""
        ours = isinstance(self, GraphnetworkBase) and self._cfg.kind == "phonon"
        if not (ours and self._flat_dtype(None) == torch.float64):          # (mixed dtypes, hidden > MAX_HIDDEN: its own DosxError)
            raise DosxError(f"{who} drives a Graphnetwork_phonon with float64 parameters (model.double()), got "
                            f"{type(self).__name__}" + (" with fp32 parameters: that is train.Trainer's / predict.Predictor's"
                                                        if ours else ""))

    def _program_fwd(self, P, g, m, factored_head: bool = False):
        if P["embeddings.weight"].dtype == torch.float64:
            dos, ctx = F64.graphnetwork_phonon_fwd(P, self._cfg, g, m)
            return dos, ctx
        dos, xL, ctx = self._fwd_fn(P, self._cfg, g, m, factored_head=factored_head)
        return (dos, xL, ctx) if self._returns_x else (dos, ctx)

    def _program_bwd(self, P, G, m, saved, grads, sink):
        ddos = grads[0]
        if P["embeddings.weight"].dtype == torch.float64:
            if ddos is None:
                ddos = torch.zeros(m.num_graphs, self._cfg.S, device=P["embeddings.weight"].device, dtype=torch.float64)
            F64.graphnetwork_phonon_bwd(P, G, self._cfg, m, saved, ddos)
            return
        dx = grads[1] if self._returns_x else None
        if ddos is None:
            ddos = torch.zeros(m.num_graphs, self._cfg.S, device=P["embeddings.weight"].device)
        self._bwd_fn(P, G, self._cfg, m, saved, ddos.float().contiguous(),
                     None if dx is None else dx.float().contiguous(), sink)

    def forward(self, g):
        out = self._run(g)
        return out if self._returns_x else out[0]
