"""Fused training step of the reference callers (`main_phDOS.py:101-118`, `main_eDOS.py:101-127`):
forward program -> loss kernel -> backward program -> (RCCL all-reduce) -> flat AdamW kernel.

No autograd graph, no per-parameter optimizer loop, no host synchronisation: the loss stays on the
device (the reference prints it every step, `main_eDOS.py:129`; read ``.item()`` only when needed).

``Trainer(replay=True)`` re-issues a RECORDED launch sequence (``ops.Program``): the first step on a shape
bucket runs normally while every libdosx call is recorded with its marshalled arguments on static
buffers; later steps copy the batch into the bucket's input buffers and replay the list — no Python
marshalling, no allocator, two real HIP streams (weight-gradient kernels overlap the dgrad chain).

``Trainer(graph=True)`` instead replays the step from captured HIP graphs: batches are padded
with ghost nodes / edges to a small set of (N, E) buckets (``batch.pad_batch`` — exact, not
approximate), every launch of the forward / loss / backward programs for a bucket is captured once,
and a step is then "copy the batch into the bucket's static buffers, replay, AdamW".  The ~160
launches of a step cost the host ~20 us each when issued from Python; replay removes that.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch

from . import functional as Fn
from . import ops
from ._lib import DosxError, from_environ
from ._models import DOSTransformerBase, GraphnetworkBase
from .batch import graph_meta
from .slots import Slot
from .trainer_base import TrainerBase

# Data parallel: a THIRD gradient bucket (GN_decoder + message-passing layers L-1 .. 1: 1.9 of the GNN trunk's 3.0 MB at the
# headline shape) all-reduced from the flush at layer 0, under layer 0's backward, so that only 1.1 MB stay behind the step
# (VERDICT r5 item 6).  Built, tested (tests/test_dp_gpu.py, tests/test_dp_gloo.py) - and OFF: on a 1-rank RCCL group the extra
# collective point costs 55 us per step (1.1118 -> 1.1667 ms, three interleaved rounds, tools/exp/r6_dp1.sh) - the communicator
# stream's wait for the weight-gradient stream lands in a hardware queue it shares with the main stream (more hardware queues,
# GPU_MAX_HW_QUEUES = 6 / 8, make the step 35 % slower: tools/exp/r6_dp2.sh) - while 1.9 MB less exposed traffic is worth about
# 15 us on 8 xGMI-connected GPUs.  To be re-measured on a real multi-GPU node.
_DP_MID_BUCKET = from_environ("DOSX_DP_MID_BUCKET", "0") == "1"
_DP_CHECK = from_environ("DOSX_DP_CHECK", "0") == "1"


class Trainer(TrainerBase):
    """AdamW(lr, weight_decay=1e-2) training of a DOSTransformer(_phonon) module, all on libdosx.

    ``dist``: optional :class:`dostransformer_amd.dist.DataParallel` — shards are per-rank batches,
    gradients are summed over ranks (loss kernels already divide by the GLOBAL element/crystal
    count), the phonon loss exchanges its two SSE scalars before the backward pass.

    ``per_crystal_keys=True`` (same spelling as :class:`dostransformer_amd.predict.Predictor`): ``transformer`` and
    ``transformer_source`` attend over each crystal's own atoms, forward and backward, instead of the rows that pad it to the
    batch's largest crystal - the step then learns what the reference computes at ``batch_size = 1``, where it trains the
    phonon model and evaluates both (`main_phDOS.py:52-55`, `main_eDOS.py:55-56`); for eDOS the phantom node counts as an atom, as
    it does there.  Eager, ``replay=True`` and ``graph=True`` alike (the bucket's own ``graph_ptr`` is the operand).  The switch does
    not touch the loss: the default phonon loss is still ONE RMSE pooled over the batch, whose gradient is not the mean of the
    batch-1 gradients - ``loss="crystal_rmse"`` is the objective that matches batch-1 training.  Not under data parallelism.

    The GNN-only baselines - ``Graphnetwork``, ``Graphnetwork_phonon`` (fp32 parameters) and ``embedder_eDOS.mlp.mlp`` - train through
    the same step (eager, ``replay=True``, ``graph=True``, ``step_dataset``, checkpoints) with their output head on its rank
    structure (``functional.graphnetwork_fwd(factored_head=True)``) and the drivers' loss on their ONE output: phonon
    ``sqrt(mean_all (dos - y)^2)`` (`main_phDOS.py:109-111`), eDOS ``mean_b sqrt(mean_s (dos - max(y, 0))^2)`` (`main_eDOS.py:111-118`).
    With one output there is no ``beta`` to weigh (anything but 1.0 is refused), no attention to give per-crystal keys, and no
    data parallelism yet; ``n_global`` must be the batch's own count.  Which node encoder is dead follows the input width and is
    fixed by the first batch: a later batch of the other width is refused.

    ``max_grad_norm=X`` / ``skip_nonfinite=True`` put the optimizer step behind a gradient guard (``guard.StepGuard``): what
    ``torch.nn.utils.clip_grad_norm_(params, X)`` between ``backward()`` and ``optimizer.step()`` and a GradScaler-style "skip
    if non-finite" do, decided on the device - one statistics launch over the flat gradient and an AdamW that reads the
    verdict, no host read.  A step whose gradient holds a NaN / inf (or that follows a reported exchange stall) leaves
    parameters and moments untouched and does not advance AdamW's time; ``grad_norm`` / ``guard_report()`` say what happened,
    ``check()`` raises.  Every mode; not under data parallelism.  Off by default: the step then issues exactly the launches it issued without these arguments.

    Fine-tuning: ``requires_grad`` decides which parameters train (``model.freeze(...)`` / ``model.train_only(...)``, or the flags
    themselves followed by ``model.update_trainable()``).  A frozen parameter and its two moments are bitwise untouched by a step,
    weight decay included - torch's behaviour for ``grad is None`` - and the guard's norm covers the trainable gradient only.  The
    flags are read when the flat buffer is laid out, never per step; the backward program drops the weight-gradient jobs of frozen
    Linears, ends in front of a frozen GNN trunk (and a frozen first encoder), and runs a cross attention over frozen keys without
    its key gradient (functional.wgrad_needed / trunk_cut / first_encoder_cut / attention_query_only); ``program_stats()`` shows
    what is left.  Every model and mode; not under data parallelism.  With nothing frozen the layout, the launches and the bits
    are what they were.

    ``param_groups=[{"params": prefix | [prefixes], "lr": ..., "weight_decay": ...}]``: ``torch.optim.AdamW``'s parameter groups
    with name prefixes for tensors (``param_groups.py``: ``resolve``, ``no_decay``, ``layerwise``) - still ONE flat AdamW launch,
    which looks decay and step size up per 64-element chunk of the flat buffer; bit for bit the ungrouped kernel applied tensor by
    tensor with each tensor's values.  ``trainer.param_groups`` is read at every step: assigning ``["lr"]`` is a schedule.  With
    the guard, with frozen parameters, every mode; not under data parallelism.  None (the default): the launch it always was.

    ``ema_decay=d`` (``ema_warmup=True``): the AdamW launch also keeps an exponential moving average of the weights
    (``ema.WeightEma``; ``ema' = ema + (p' - ema)(1 - d_t)``, ``d_t = min(d, (1 + t) / (10 + t))`` under warm-up) - a step the guard
    skips leaves it alone.  ``with trainer.ema_weights():`` evaluates under it, ``trainer.ema_state_dict()`` exports it,
    ``state_dict()`` carries it.  Every mode, with the guard, frozen parameters and groups; not under data parallelism.  None
    (the default): the launch and the checkpoint it always was.

    ``loss="crystal_rmse" | "mse" | "mae" | "huber"`` (``huber_delta=X`` with the last, and only with it) replaces the driver's loss
    by the mean over crystals of each crystal's own RMSE, MSE, MAE or ``torch.nn.HuberLoss(delta=X)`` term, ``f(dos_global) + beta
    f(dos_system)`` for the two-output models - one entry, ``dosx_loss_rows`` (csrc/loss_rows.hip), in place of the loss launches;
    eDOS models keep their target clamp.  ``"crystal_rmse"`` is the reference's phonon objective at its ``batch_size = 1`` (with
    ``per_crystal_keys=True`` a step on B crystals follows the mean of the B batch-1 gradients); on an eDOS model it is the default
    objective and trains the same bits.  ``trainer.crystal_losses`` is then the last step's per-crystal losses, a ``[B]`` device
    tensor (under replay a view of the bucket's static buffer) valid until the next step.  Every mode, with the guard, frozen
    parameters, groups and the average; ``n_global`` must be the batch's own count; not under data parallelism.  A constructor
    argument like ``beta``: not in ``state_dict()``.  None (the default): the reference's loss, the launches it always issued.

    ``step_accumulate([g1, g2, ...])`` / ``step_dataset_accumulate(ds, [idx1, idx2, ...])``: gradient accumulation - ONE optimizer
    step on the objective of the concatenated batch, every micro-batch through its ordinary program with the loss divided by the
    window's crystal count, one ``dosx_grad_accumulate`` launch behind each (see ``step_accumulate``).  ``step`` and
    ``step_dataset`` issue the launches they always issued.

    ``sample_weights=True`` / ``bin_weights=[S]`` (with one of the four ``loss=`` kinds): torch's ``(w * per_sample_loss).mean()`` -
    ``loss = sum_b w_b l_b / B`` with the per-crystal terms ``sum_s v_s e(r) / sum_s v_s`` under energy-bin weights ``v`` - through
    ``dosx_loss_rows_w`` in place of ``dosx_loss_rows``, no other launch.  ``step(g)`` reads the batch's ``[B]`` field
    ``g.weight``; ``step_dataset`` hands the kernel the dataset's resident table (``DeviceDataset.set_weights``: checked on the
    host once, written in place, read at every step) and the bucket's selection, and the launch gathers.  All-ones weights train
    the unweighted bits; a weight of exactly 0 takes a crystal out whatever it holds (a NaN target included: the guard does not
    trip); ``crystal_losses`` stay the crystals' own unweighted losses.  Every mode, windows, the guard, frozen parameters, groups
    and the average; constructor arguments like ``loss``: not in ``state_dict()``; not under data parallelism.

    ``functionals=<functionals.Functionals | [K,S] tensor>`` with ``functional_kind="sq" | "abs"`` and ``functional_weight=lam``
    (with one of the four ``loss=`` kinds): a penalty on K linear functionals of the DOS next to the pointwise term, ``l_b += lam / K
    sum_k e(F_k(p_b) - F_k(t_b))`` per output (``beta`` on the second), ``e = u^2`` or ``|u|`` - with ``functionals.cumulative(S)``
    the Cramer or the Wasserstein-1 distance between the cumulative DOS curves - through ``dosx_loss_rows_fn`` in place of the
    loss launch, no other launch.  K, S <= 512.  The table lives in ONE trainer-owned device buffer:
    ``set_functionals(table)`` of the same shape writes it in place, nothing is re-recorded, the next replayed step reads it
    (a schedule on the term is a rescaled table); ``lam`` is recorded with the launch.  ``crystal_losses`` include the term.
    ``functional_weight=0`` trains the bits of the trainer without a table.  Every mode, windows, the guard, frozen parameters,
    groups, the average and the weights; constructor arguments: not in ``state_dict()``; not under data parallelism.
    A ``Functionals`` with normalised rows (``functionals.centre``, ``normalised_cumulative``, ``normalised``: rows over one floored
    denominator functional, ``u_k = F_k(p) / max(D(p), floor) - F_k(t) / max(D(t), floor)``) trains on the ratios through
    ``dosx_loss_rows_fn_norm_desc``: the buffer holds table and denominator, ``set_functionals`` writes both and
    refuses another K, number of normalised rows or floor.  Such rows alone leave the scale of the prediction free.
    """

    _who = "Trainer"
    _dtype = torch.float32
    _tiled = True

    def __init__(self, model: DOSTransformerBase, lr: float = 1e-4, beta: float = 1.0, weight_decay: float = 1e-2,
                 betas=(0.9, 0.999), eps: float = 1e-8, dist=None, graph: bool = False, replay: bool = False,
                 bucket=(8, 128), max_slots: int = 32, promote: float = 0.0, per_crystal_keys: bool = False,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, param_groups=None,
                 ema_decay: Optional[float] = None, ema_warmup: bool = True, loss: Optional[str] = None,
                 huber_delta: Optional[float] = None, sample_weights: bool = False, bin_weights=None,
                 functionals=None, functional_kind: str = "sq", functional_weight: float = 1.0):
        if not isinstance(model, (DOSTransformerBase, GraphnetworkBase)):
            raise TypeError("Trainer drives DOSTransformer / DOSTransformer_phonon / Graphnetwork / Graphnetwork_phonon / mlp modules")
        model._require_fp32_program("Trainer")
        self._baseline = isinstance(model, GraphnetworkBase)
        if self._baseline:
            name = type(model).__name__
            self._first_width_fixes_dead = True
            if float(beta) != 1.0:
                raise ValueError(f"Trainer({name}): beta={beta} - the model has ONE output and its loss no second term to weigh; "
                                 f"only the default 1.0 is accepted")
            if per_crystal_keys:
                raise DosxError(f"Trainer({name}, per_crystal_keys=True): the model has no attention - a crystal's output "
                                f"never depends on its batch mates")
            if dist is not None:
                raise DosxError(f"Trainer({name}, dist=...): data parallelism is not implemented for the GNN-only baselines")
        if per_crystal_keys and dist is not None:
            raise DosxError("Trainer(per_crystal_keys=True) is a single-GPU mode: not with dist (data parallelism)")
        if dist is not None and len(model.trainable_names()) != len(model._live_named()):
            raise DosxError("Trainer(dist=...) with frozen parameters: fine-tuning is a single-GPU mode, not with dist (data "
                            "parallelism)")
        self._per_crystal_keys = bool(per_crystal_keys)
        self.dist = dist
        self._init_guard(max_grad_norm, skip_nonfinite)
        self.model, self.lr, self.beta, self.wd, self.betas, self.eps = model, lr, beta, weight_decay, betas, eps
        self._init_param_groups(param_groups)
        self._init_ema(ema_decay, ema_warmup)
        self._init_loss(loss, huber_delta)
        self._init_weights(sample_weights, bin_weights)
        self._init_functionals(functionals, functional_kind, functional_weight)
        self.graph = graph
        self.replay = replay
        # (node, edge) granularity of the shape buckets unpadded batches are ghost-padded to in graph / replay mode: a
        # coarser grid means fewer distinct launch lists to record when batches are reshuffled every epoch
        self.bucket = tuple(bucket)
        self.bucketed = dist is not None and not graph       # early-bucket overlap (eager and replay modes)
        self._early_work = None
        self._mid_work = None
        self._early_side = None
        self._rec_parts = []
        self.step_count = 0
        self._m = self._v = None
        self._fp = None
        self.kind = model._cfg.kind
        self.last_outputs = None
        # shape buckets seen so far -> static buffers + recorded program, least recently used first; bounded: with
        # per-epoch shuffling new (N, E) buckets keep appearing, each holding a step's worth of activations
        self._slots: "OrderedDict[tuple, Slot]" = OrderedDict()
        self.max_slots = int(max_slots)
        self.slot_hits = self.slot_misses = self.slot_promoted = 0
        # largest relative excess of nodes / edges a first-time bucket accepts from a live one (step_dataset; 0 = every
        # bucket records its own launch list: bitwise the step on the batch padded to its own bucket)
        self.promote = float(promote)
        self._seen = {}
        self.kernel_timer = None          # ops._KernelTimer: replayed programs then run through dosx_replay_timed
        self._ds_checked = []             # datasets whose per-rank size was compared across the ranks (step_dataset)

    @property
    def per_crystal_keys(self) -> bool:
        """True: the two cross attentions attend over each crystal's own atoms (fixed at construction)."""
        return self._per_crystal_keys

    # ---- the step, split where the data-parallel collectives go --------------------------------
    def _part_a(self, fp, g, m, st_n_global: Optional[int] = None):
        """forward program (+ the phonon SSE pair).  Returns the state part B needs.  st_n_global: crystals in the un-sharded
        batch (None: this batch is the whole batch)."""
        if st_n_global is None:
            st_n_global = m.num_graphs
        model, dev, cfg = self.model, fp.flat.device, self.model._cfg
        B, S = m.num_graphs, cfg.S
        w = self._batch_weights(g)                   # (refuses a batch without `weight` before anything is launched)
        if self._baseline:
            out = model._program_fwd(fp.P, g, m, factored_head=True)
            y = Fn._f32(g.phdos).reshape(B, S) if self.kind == "phonon" else Fn._f32(g.y_ft).reshape(-1)
            return {"ctx": out[-1], "dos": out[0], "out": out[:-1] if model._returns_x else out[0], "B": B, "S": S, "y": y, "w": w}
        dg, xL, ds, (ctx, dos) = model._program_fwd(fp.P, g, m, bump_seed=False,     # (step() bumps the dropout seed)
                                                    per_crystal_keys=self._per_crystal_keys)
        st = {"ctx": ctx, "dos": dos, "out": (dg, xL, ds), "B": B, "S": S, "w": w}
        if self.kind == "phonon":
            st["y"] = Fn._f32(g.phdos).reshape(B, S)
            if self.loss is not None:      # a per-crystal loss: one entry in _loss_launch, no SSE pair
                st["split_loss"] = False
                return st
            st["sse"] = Fn._empty(dev, 2)
            st["split_loss"] = self.dist is not None or int(st_n_global) != B
            if st["split_loss"]:           # two-phase loss: ranks exchange the SSE pair in between, and / or the loss is
                ops.sse2(dos[:B], dos[B:], st["y"], st["sse"], B * S)      # normalised by a GLOBAL count that is not B
        else:
            st["y"] = Fn._f32(g.y_ft).reshape(-1)
        return st

    def _loss_launch(self, dev, st, pg, ps, beta: float, n_global: int):
        """The loss of the step with its gradient, for both output counts: -> (ddos, loss).  Two outputs: ``pg``, ``ps`` are
        the halves of ``dos`` and ``ddos`` is laid out like it.  One output (the GNN-only baselines): ``ps is pg`` and
        ``beta = 0`` - the drivers' loss entries in their one-output use (include/dosx.h: the loss is rmse(pg) exactly, the
        second gradient goes to scratch); with ``loss=...`` the per-crystal entry in its own one-output form (ps == NULL: no
        second gradient, no scratch)."""
        B, S, y = st["B"], st["S"], st["y"]
        one = ps is pg
        ddos = Fn._empty(dev, B if one else 2 * B, S)
        dpg = ddos if one else ddos[:B]
        if self.loss is not None:          # eDOS clamps its target at 0 (main_eDOS.py:113), phonon does not; n_global == B
            st["crystal"], loss = self._loss_rows(Fn._empty, dev, pg, None if one else ps, y, self.kind != "phonon", dpg,
                                                  None if one else ddos[B:],
                                                  B_global=n_global,         # ... or, inside a window, the window's total
                                                  weights=st["w"])
            return ddos, loss
        dps = Fn._empty(dev, B, S) if one else ddos[B:]
        if self.kind == "phonon":
            loss = Fn._empty(dev, 1)
            split = st.get("split_loss", False)
            if split or int(n_global) != B:
                if not split:
                    raise RuntimeError("n_global differs between the two halves of the step")
                ops.loss_phonon_bwd(pg, ps, y, st["sse"], beta, float(n_global * S), dpg, dps, loss, B * S)
            else:                          # one launch: SSE pair, loss and gradient (normalised by B*S: n_global == B)
                ops.loss_phonon(pg, ps, y, st.get("sse"), beta, dpg, dps, loss, B * S)
            return ddos, loss[0]
        lp = Fn._empty(dev, B + 1)
        ops.loss_edos(pg, ps, y, beta, B, S, int(n_global), dpg, dps, lp)     # (B, the global count, or a window's total)
        ops.sum_to(lp, B, lp[B:])
        return ddos, lp[B]

    def _part_b(self, fp, m, st, n_global: int):
        """loss gradient + backward program.  n_global: crystals in the un-sharded batch."""
        dev, cfg = fp.flat.device, self.model._cfg
        B, dos = st["B"], st["dos"]
        if self._baseline and not self._whole_or_window(B, n_global):
            raise ValueError(f"{self._who_with_model()}: n_global={n_global} but the batch holds {B} crystals "
                             f"(no data parallelism for the GNN-only baselines)")
        pg, ps, beta = (dos, dos, 0.0) if self._baseline else (dos[:B], dos[B:], self.beta)
        ddos, loss = self._loss_launch(dev, st, pg, ps, beta, n_global)
        sink = ops.GradSink(dev)
        if self._baseline:
            self.model._bwd_fn(fp.P, fp.G, cfg, m, st["ctx"], ddos, None, sink, factored_head=True)
        else:
            sink.gnn_hook = self._gnn_hook(fp)      # (functional.gnn_bwd calls it behind the flush that completes layers L-1 .. 1)
            Fn.dostransformer_bwd(fp.P, fp.G, cfg, m, st["ctx"], ddos, None, sink, mid_hook=self._mid_hook(fp))
        self._wgrad_keys = sink.wgrad_keys
        sink.release()
        return loss

    # ---- data parallel: early gradient bucket ------------------------------------------------------
    def _mid_hook(self, fp):
        """Backward reaches the GNN trunk: reduce the early bucket's slabs on the side stream and start its
        all-reduce there, underneath the GNN backward (xGMI traffic overlaps compute; only the GNN bucket's
        all-reduce stays exposed at the end of the step)."""
        if self.dist is None:
            # single GPU: the early bucket's weight gradients + slab reduction run HERE (replay: on the side stream,
            # underneath the GNN backward; eager: inline), while their operands are still in L2 - not at the tail
            return lambda sink: sink.flush_on_side()
        if not self.bucketed or fp.n_late <= 0 or fp.n_late >= fp.total:
            return None

        def hook(sink):
            sink.flush_on_side()
            rec = ops.RECORDER.active
            if rec:                                   # the collective is not a libdosx call: split the recording
                self._rec_parts.append((ops.RECORDER.end(), "early"))
            self._start_early(fp, sink.wside)
            if rec:
                ops.RECORDER.begin()
        return hook

    def _gnn_hook(self, fp):
        """Backward reaches message-passing layer 0 and the weight-gradient group of the layers behind it has been flushed
        (functional.gnn_bwd): the MID bucket - GN_decoder + layers L-1 .. 1, two thirds of the GNN trunk's gradient bytes - is
        final, so its all-reduce starts on the gradient stream NOW, underneath layer 0's backward, the encoders' backward and the
        last weight-gradient group; only the last bucket (encoders + layer 0) is reduced behind the step."""
        if self.dist is None or not self.bucketed or not (0 < fp.n_late < fp.total) or not (0 < fp.n_last < fp.n_late) or not _DP_MID_BUCKET:
            return None

        def hook(sink):
            rec = ops.RECORDER.active
            if rec:
                self._rec_parts.append((ops.RECORDER.end(), "mid"))
            self._start_mid(fp, sink.wside)
            if rec:
                ops.RECORDER.begin()
        return hook

    def _start_early(self, fp, side) -> None:
        stream = side if side is not None else torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            self._early_work = self.dist.all_reduce_grads_async(fp.grad[fp.n_late:])
        self._early_side = side

    def _start_mid(self, fp, side) -> None:
        stream = side if side is not None else torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            self._mid_work = self.dist.all_reduce_grads_async(fp.grad[fp.n_last:fp.n_late])

    def _n_global(self, B: int, n_global: Optional[int], g=None, ds=None) -> int:
        """Crystals in the un-sharded batch: the caller's value, else - inside an accumulation window - the window's total, else
        what the sharder recorded on the batch (``dist.shard_batch``), else — a batch object's last resort, a blocking
        collective + host read — the sum over ranks.  A dataset step (``ds``) has neither collective nor host read:

        without an explicit n_global the ranks of a data-parallel job must draw EQUALLY sized shards every step, then
        n_global = B * world.  That holds for every batch of an epoch, the last one included, iff all ranks hold equally many
        crystals and cut them with the same batch size - checked ONCE per dataset (one blocking min/max over ranks at its first
        step); ragged shards must pass the true n_global, or the loss would be normalised by the wrong count
        (`main_phDOS.py:109-114` is ONE rmse over the un-sharded batch).  DOSX_DP_CHECK=1 cross-checks B itself across the
        ranks on every step (debugging; blocking)."""
        if n_global is not None:
            return int(n_global)
        if self._window_total is not None:
            return self._window_total
        ng = getattr(g, "n_global", None)
        if ng is not None:
            return int(ng)
        if self.dist is None:
            return B
        if ds is None:
            return self.dist.global_count(B)
        if not any(d is ds for d in self._ds_checked):
            lo, hi = self.dist.min_max(len(ds))
            if lo != hi:
                raise ValueError(f"data-parallel ranks hold {lo}..{hi} crystals: with ragged shards the last batches of "
                                 f"an epoch differ in size across ranks - pass the global batch size as n_global")
            self._ds_checked.append(ds)
        if _DP_CHECK:
            lo, hi = self.dist.min_max(B)
            if lo != hi:
                raise ValueError(f"ranks stepped on {lo}..{hi} crystals without an explicit n_global")
        return B * self.dist.world

    # ---- what the shared driver (trainer_base.TrainerBase) asks -----------------------------------
    def _slotted(self, dataset: bool) -> bool:
        return bool(self.graph or self.replay)

    def _who_with_model(self) -> str:
        return f"Trainer({type(self.model).__name__})"

    def _prepare(self, g, ds, B: int, n_global: Optional[int]):
        """-> (flat parameters, n_global resolved): see ``_n_global``."""
        model = self.model
        model._require_fp32_program("Trainer")
        fp = self._flat_for(model._module_device(), g, None if ds is None else int(ds._f32_tables()["x"].shape[1]))
        self._state(fp)
        ng = self._n_global(B, n_global, g, ds)
        self._require_whole_batch(B, ng)              # (before a slot is made, not inside its recording)
        return fp, ng

    def _extra(self, fp, ng: int) -> int:
        return ng                     # (the fp32 program makes its dropout seed itself, inside the step)

    def _key(self, n: int, e: int, B: int, n_max: int, ng: int, tiled: bool) -> tuple:
        return (n, e, B, n_max, ng, tiled)

    def _slot_meta(self, g, dev):
        m = g.meta
        if m is None or m.edge_perm is not None:
            raise ValueError("graph mode needs batches from collate(sort_edges=True) (+ pad_batch)")
        return m

    # ---- eager path ------------------------------------------------------------------------------
    def forward_backward(self, g, n_global: Optional[int] = None, _bump: bool = True) -> torch.Tensor:
        """Forward + loss + backward; leaves the gradients in the flat buffer.  Returns the loss
        (0-dim device tensor; for eDOS under data parallelism it is this rank's share)."""
        self._ema_refuse("forward_backward")
        # (_bump: a direct forward_backward() + optimizer_step() loop draws fresh dropout masks too)
        fp, ng = self._context(g, None, self._crystals_of(g), n_global, _bump)
        return self._eager(fp, g, ng)

    def _eager(self, fp, g, ng: int) -> torch.Tensor:
        m = graph_meta(g, fp.flat.device)
        with torch.no_grad(), ops.call_log() as names:
            st = self._part_a(fp, g, m, ng)
            self.last_outputs = st["out"]
            if self.kind == "phonon" and self.dist is not None:
                self.dist.all_reduce_sse(st["sse"])
            loss = self._part_b(fp, m, st, ng)
        self._stats = self._make_stats(names)
        self.crystal_losses = st.get("crystal")
        return loss

    # ---- graph path ------------------------------------------------------------------------------
    def _capture(self, slot: Slot, fp, ng: int) -> None:
        g, m = slot.g, slot.g.meta
        split = self.dist is not None and self.kind == "phonon"
        with ops.recording_scope(), torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                       # eager warm-up (lazy kernel attributes etc.)
                st = self._part_a(fp, g, m, ng)
                self._part_b(fp, m, st, ng)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            slot.graph_a = torch.cuda.CUDAGraph()
            with ops.call_log() as names:
                with torch.cuda.graph(slot.graph_a):
                    st = self._part_a(fp, g, m, ng)
                    if not split:
                        loss = self._part_b(fp, m, st, ng)
                if split:
                    slot.graph_b = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(slot.graph_b, pool=slot.graph_a.pool()):
                        loss = self._part_b(fp, m, st, ng)
        slot.stats = self._make_stats(names)
        slot.keep = (st, loss)            # keeps the graph-owned outputs from being recycled
        slot.loss, slot.out, slot.sse, slot.crystal = loss, st["out"], st.get("sse"), st.get("crystal")

    def _record(self, slot: Slot, fp, ng: int) -> None:
        """Run the step once on the slot's static buffers while recording every launch."""
        g, m = slot.g, slot.g.meta
        split = self.dist is not None and self.kind == "phonon"
        # (replay is cheap enough on the host to feed two streams)
        with ops.recording_scope(side_stream=True), torch.no_grad():
            # the plan of a replayed step: recorded programs separated by the collectives (which are not
            # libdosx calls): [fwd] (sse) [bwd up to the GNN] (early bucket all-reduce) [GNN bwd]
            plan = []
            self._rec_parts = []
            ops.RECORDER.begin()
            st = self._part_a(fp, g, m, ng)
            if split:
                plan.append(("prog", ops.RECORDER.end()))
                plan.append(("sse", None))
                self.dist.all_reduce_sse(st["sse"])
                ops.RECORDER.begin()
            loss = self._part_b(fp, m, st, ng)
            last = ops.RECORDER.end()
            for part, coll in self._rec_parts:    # (_mid_hook / _gnn_hook closed these while recording)
                plan.append(("prog", part))
                plan.append((coll, None))
            plan.append(("prog", last))
            self._rec_parts = []
        slot.plan, slot.prog = plan, plan[0][1]
        slot.stats = self._make_stats([fn.__name__ for kind, prog in plan if kind == "prog" for fn, _ in prog.prog])
        slot.keep = (st, loss)
        slot.loss, slot.out, slot.sse, slot.crystal = loss, st["out"], st.get("sse"), st.get("crystal")

    def _run_slot(self, slot: Slot, fp, ng: int, fresh: bool) -> torch.Tensor:
        """The step on a bucket whose static buffers hold the batch: record / capture on first use, replay afterwards."""
        if fresh and self.replay:
            self._record(slot, fp, ng)       # this IS the step for this batch (run + record)
            self.last_outputs, self._stats, self.crystal_losses = slot.out, slot.stats, slot.crystal
            return slot.loss
        if fresh:
            self._capture(slot, fp, ng)
        self._stats = getattr(slot, "stats", None)
        if self.replay:
            for kind, prog in slot.plan:
                if kind == "prog":
                    if self.kernel_timer is not None:      # bench.py: event pair around every replayed launch
                        prog.run_timed(self.kernel_timer)
                    else:
                        prog.run()
                elif kind == "sse":
                    self.dist.all_reduce_sse(slot.sse)
                elif kind == "mid":
                    self._start_mid(fp, ops.GradSink.grad_stream(fp.flat.device))
                else:
                    self._start_early(fp, ops.GradSink.grad_stream(fp.flat.device))
        else:
            slot.graph_a.replay()
            if slot.graph_b is not None:
                self.dist.all_reduce_sse(slot.sse)
                slot.graph_b.replay()
        self.last_outputs, self.crystal_losses = slot.out, slot.crystal
        return slot.loss

    # ---- what the step launched ------------------------------------------------------------------
    def _make_stats(self, entries) -> dict:
        entries = list(entries)
        keys = list(getattr(self, "_wgrad_keys", ()))
        return {"launches": sum(1 for e in entries if e.startswith("dosx_")), "wgrad_jobs": len(keys), "entries": entries,
                "wgrad_keys": keys}

    def program_stats(self) -> dict:
        """What the last step's program (forward, loss, backward; not the optimizer) consisted of - of the recording when the step
        was replayed, of the capture when it ran from HIP graphs, else of the eagerly issued step itself: ``entries`` the names
        of its entries in issue order (a recorded program's ``Program.prog``: libdosx entry points plus the stream fork / join
        operations), ``launches`` how many of them are libdosx calls, ``wgrad_jobs`` how many weight-gradient jobs the backward
        deferred to its GradSink and ``wgrad_keys`` the weight each of them serves.  What a frozen set pruned shows here."""
        st = getattr(self, "_stats", None)
        if st is None:
            raise DosxError("program_stats: no step has run yet")
        return dict(st)

    # ---- optimizer -------------------------------------------------------------------------------
    def _reduce_gradients(self, fp) -> None:
        if self.dist is not None:
            if self._early_work is not None:          # early (+ mid) bucket already in flight: only the last bucket is exposed
                if self._mid_work is not None:
                    self.dist.all_reduce_grads(fp.grad[:fp.n_last])
                    self._mid_work.wait()
                    self._mid_work = None
                else:
                    self.dist.all_reduce_grads(fp.grad[:fp.n_late])
                self._early_work.wait()
                self._early_work = None
            else:
                assert self._mid_work is None
                self.dist.all_reduce_grads(fp.grad)
