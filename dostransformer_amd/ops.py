"""Thin torch-tensor wrappers over the libdosx C ABI (one Python function per entry point).

Tensors are only used as device-memory handles (``data_ptr()``) and every launch goes to
``torch.cuda.current_stream()`` so the calls are stream-ordered with the rest of the program and
capturable in a HIP graph.  No arithmetic happens in Python.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import weakref
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi, _lib
from ._lib import Ffn, BIG, Attn, Gemm, ReduceJob, RowMap, Seg, Wgrad

# include/dosx.h's enumerators under the package's names (the values come from the generated _abi.py, never from a literal here)
PRO_NONE, PRO_PRELU, PRO_LN_PRELU, PRO_ROWLN = _abi.DOSX_PRO_NONE, _abi.DOSX_PRO_PRELU, _abi.DOSX_PRO_LN_PRELU, _abi.DOSX_PRO_ROWLN
EPI_BIAS_ACT, EPI_LN, EPI_PRELU_LN_BWD, EPI_RELU_MASK = _abi.DOSX_EPI_BIAS_ACT, _abi.DOSX_EPI_LN, _abi.DOSX_EPI_PRELU_LN_BWD, _abi.DOSX_EPI_RELU_MASK
EPI_ROWLN_BWD, EPI_PRELU_BWD, EPI_SEGSUM = _abi.DOSX_EPI_ROWLN_BWD, _abi.DOSX_EPI_PRELU_BWD, _abi.DOSX_EPI_SEGSUM
EPI_PRELU_LN_BWD_SEG = _abi.DOSX_EPI_PRELU_LN_BWD_SEG
ATTN_RAW_Q, ATTN_NO_RESIDUAL = _abi.DOSX_ATTN_RAW_Q, _abi.DOSX_ATTN_NO_RESIDUAL
ATTN_BWD_DKV_HALF, ATTN_BWD_DQ_HALF = _abi.DOSX_ATTN_BWD_DKV_HALF, _abi.DOSX_ATTN_BWD_DQ_HALF
# DosxGemm.act has no enumerator: the header gives its values in the comment of DOSX_EPI_BIAS_ACT ("act: 0 none, 1 relu, 2 leaky(slope)"),
# which tests/test_lib_abi.py reads
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


class _KernelTimer:
    """HIP-event timing of EVERY libdosx launch (events are recorded on torch's current stream, the stream the call
    is issued on — under ``torch.cuda.stream(side)`` that is the side stream).  Each wrapper below hands ``_call`` a
    work record ``(site, kernel, bound, work)``: ``site`` names the launch family + shape, ``kernel`` the device symbol
    (what rocprofv3 lists), ``bound`` 'mfma' | 'hbm' and ``work`` the ALGORITHMIC flops / bytes of the launch.  bench.py
    turns the records into the ``roofline`` object: the dominant site is the one with the largest total time."""

    def __init__(self):
        self.enabled = False
        self.records = []

    def reset(self, enabled: bool):
        self.enabled = enabled
        self.records = []

    def start(self):
        if not self.enabled:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def stop(self, ev, tag: str, kernel: str, bound: str, work: float, kernels: int = 1):
        """work: algorithmic flops (bound == 'mfma') or bytes (bound == 'hbm') of this launch; kernels: device kernels the
        bracketed call launched (dosx_grad_flush: one per table of 8 jobs)."""
        if ev is None:
            return
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        self.records.append((tag, kernel, bound, float(work), ev, end, int(kernels)))

    def add_ms(self, tag: str, kernel: str, bound: str, work: float, ms: float, kernels: int = 1):
        """a launch whose duration was measured elsewhere (Program.run_timed)"""
        self.records.append((tag, kernel, bound, float(work), None, float(ms), int(kernels)))

    def roofline(self, hbm_peak_gbs: float, mfma_peak_tflops: float):
        agg = {}
        for tag, kernel, bound, work, s, e, nk in self.records:
            ms = e if s is None else s.elapsed_time(e)
            a = agg.setdefault(tag, {"kernel": kernel, "bound": bound, "work": 0.0, "ms": 0.0, "n": 0, "k": 0})
            a["work"] += work
            a["ms"] += ms
            a["n"] += 1
            a["k"] += nk
        out = []
        for tag, a in agg.items():
            if a["ms"] <= 0:
                continue
            if a["bound"] == "mfma":
                ach, peak, unit = a["work"] / (a["ms"] * 1e-3) / 1e12, mfma_peak_tflops, "TFLOP/s"
            else:
                ach, peak, unit = a["work"] / (a["ms"] * 1e-3) / 1e9, hbm_peak_gbs, "GB/s"
            out.append({"site": tag, "kernel": a["kernel"], "bound": a["bound"], "achieved": round(ach, 3),
                        "peak": peak, "unit": unit, "frac": round(ach / peak, 5), "traffic": None,
                        "launches": a["n"], "kernel_launches": a["k"], "avg_us": round(1e3 * a["ms"] / a["n"], 3),
                        "work_per_launch": a["work"] / a["n"], "total_ms": round(a["ms"], 3)})
        out.sort(key=lambda r: -r["total_ms"])
        dom = dict(out[0]) if out else None
        return {"dominant": dom, "all": out}


KERNEL_TIMER = _KernelTimer()

# bench.py: ghost-padded row count -> real rows of the batch whose step is being recorded, so that the ALGORITHMIC work of a
# site counts real rows only (the launches themselves run on the padded bucket).  Empty outside the bench.  The mapping
# applies ONLY to launches issued inside a ``graph_rows()`` scope - the GNN trunk, whose row counts are nodes / edges: a
# transformer GEMM whose M = S * 2B happens to equal a padded edge count keeps its own M.
REAL_ROWS: dict = {}
_GRAPH_SCOPE = [0]


class graph_rows:
    """Scope whose launches have per-node / per-edge row counts (functional.gnn_trunk_fwd / _bwd)."""

    def __enter__(self):
        _GRAPH_SCOPE[0] += 1

    def __exit__(self, *exc):
        _GRAPH_SCOPE[0] -= 1


def _real(M) -> int:
    return REAL_ROWS.get(int(M), int(M)) if _GRAPH_SCOPE[0] else int(M)


class _Recorder:
    """Launch recorder: while active, every libdosx call (function pointer + fully marshalled ctypes
    arguments, stream handle included) and every stream fork/join is appended to ``prog`` and every
    tensor allocated through :func:`alloc` is kept alive, so the exact same launch sequence can be
    re-issued later on the same buffers by :class:`Program` with no Python marshalling, no allocation
    and no autograd — the host-side analogue of a captured graph, but it keeps real HIP streams (the
    side stream of GradSink runs concurrently with the main one on replay)."""

    def __init__(self):
        self.active = False
        self.prog = []
        self.keep = []
        self.work = {}

    def begin(self):
        if self.active:
            raise RuntimeError("recorder already active")
        self.active, self.prog, self.keep, self.work = True, [], [], {}

    def end(self) -> "Program":
        p = Program(self.prog, self.keep, self.work)
        self.active, self.prog, self.keep, self.work = False, [], [], {}
        return p


class Program:
    """A recorded launch list.  ``run()`` re-issues it through ``dosx_replay`` (one ctypes call; the loop over the
    entries runs in C, csrc/replay.cpp).  Entries are libdosx calls and the stream fork / join operations of
    :class:`GradSink`, which are lowered to hipEventRecord / hipStreamWaitEvent on the raw handles."""

    def __init__(self, prog, keep, work=None):
        self.prog, self.keep = prog, keep
        self.work = work or {}            # index in prog -> (site, kernel, bound, work) of that launch
        self._calls = None
        self._entry_of = []               # lowered call index -> index in prog
        self._n = 0
        self._events = []

    # ---- lowering ------------------------------------------------------------------------------------------
    def _compile(self):
        lib = _lib.load()
        ops_by_name = {}

        def op_of(name):
            if name not in ops_by_name:
                ni, nf = C.c_int(0), C.c_int(0)
                op = lib.dosx_replay_op(name.encode(), C.byref(ni), C.byref(nf))
                if op < 0:
                    raise RuntimeError(f"{name} is not a replayable entry point")
                ops_by_name[name] = (op, ni.value, nf.value)
            return ops_by_name[name]

        out = []
        entry_of = self._entry_of = []
        cur = [0]

        def emit(name, ints, flts=()):
            entry_of.append(cur[0])
            op, ni, nf = op_of(name)
            if (ni, nf) != (len(ints), len(flts)):
                raise RuntimeError(f"{name}: recorded {len(ints)}+{len(flts)} arguments, the entry point takes {ni}+{nf}")
            c = _lib.Call()
            c.op, c.nint, c.nflt = op, len(ints), len(flts)
            for i, v in enumerate(ints):
                c.iarg[i] = int(v) if v is not None else 0
            for i, v in enumerate(flts):
                c.farg[i] = float(v)
            out.append(c)

        for pi, (fn, args) in enumerate(self.prog):
            cur[0] = pi
            owner = getattr(fn, "__self__", None)
            if isinstance(owner, torch.cuda.Event) and fn.__name__ == "record":          # ev.record(stream)
                emit("hipEventRecord", [owner.cuda_event, args[0].cuda_stream])
            elif isinstance(owner, torch.cuda.Stream) and fn.__name__ == "wait_event":    # stream.wait_event(ev)
                emit("hipStreamWaitEvent", [owner.cuda_stream, args[0].cuda_event, 0])
            elif isinstance(owner, torch.cuda.Stream) and fn.__name__ == "wait_stream":   # main.wait_stream(side)
                ev = torch.cuda.Event()
                ev.record(args[0])                                                       # creates the hip event
                self._events.append(ev)
                emit("hipEventRecord", [ev.cuda_event, args[0].cuda_stream])
                emit("hipStreamWaitEvent", [owner.cuda_stream, ev.cuda_event, 0])
            else:                                                                         # a libdosx entry point
                ints, flts = [], []
                for a, t in zip(args, fn.argtypes):
                    if t is C.c_float or t is C.c_double:
                        flts.append(a.value if hasattr(a, "value") else a)
                    elif hasattr(a, "_obj"):                                              # byref(descriptor)
                        ints.append(C.addressof(a._obj))
                    elif isinstance(a, C.Array) or isinstance(a, C.Structure):
                        ints.append(C.addressof(a))
                    else:
                        ints.append(a.value if hasattr(a, "value") else a)
                emit(fn.__name__, ints, flts)
        self._n = len(out)
        self._calls = (_lib.Call * self._n)(*out)

    def run(self) -> None:
        if self._calls is None:
            self._compile()
        failed = C.c_int(-1)
        rc = _lib.load().dosx_replay(self._calls, self._n, C.byref(failed))
        if rc:
            _lib.check(rc, f"replayed call #{failed.value}")

    def run_timed(self, timer: "_KernelTimer") -> None:
        """run() with a HIP event pair around every entry (dosx_replay_timed): the per-launch durations of the REPLAYED
        step, streams and all, appended to ``timer`` under the work records captured while recording."""
        if self._calls is None:
            self._compile()
        ms = (C.c_float * self._n)()
        failed = C.c_int(-1)
        rc = _lib.load().dosx_replay_timed(self._calls, self._n, ms, C.byref(failed))
        if rc:
            _lib.check(rc, f"replayed call #{failed.value}")
        for ci in range(self._n):
            w = self.work.get(self._entry_of[ci])
            if w is not None:
                timer.add_ms(w[0], w[1], w[2], w[3], float(ms[ci]), w[4] if len(w) > 4 else 1)

    def run_python(self) -> None:
        """Reference implementation of run(): the same list issued entry by entry from Python."""
        for fn, args in self.prog:
            rc = fn(*args)
            if rc:
                _lib.check(rc, getattr(fn, "__name__", "dosx call"))

    def __len__(self):
        return len(self.prog)


RECORDER = _Recorder()


@contextlib.contextmanager
def recording_scope(side_stream: Optional[bool] = None):
    """Around the first step of a bucket (recorded between ``RECORDER.begin()`` / ``end()`` by the caller, or captured into a
    HIP graph): the kernel timer is off - its events are not part of a replayed step - and, when given, ``side_stream`` is
    ``GradSink.use_side_stream`` for the duration.  However the scope is left, a recorder that is still active is ended and
    both switches get their values back."""
    timer_on, side_before = KERNEL_TIMER.enabled, GradSink.use_side_stream
    KERNEL_TIMER.enabled = False
    if side_stream is not None:
        GradSink.use_side_stream = side_stream
    try:
        yield
    finally:
        if RECORDER.active:
            RECORDER.end()
        GradSink.use_side_stream = side_before
        KERNEL_TIMER.enabled = timer_on


def _call(name: str, *args, w=None) -> None:
    """Issue one libdosx entry point.  ``w``: callable returning the work record ``(site, kernel, bound, work)`` of this
    launch, evaluated only when the kernel timer is on (bench.py's instrumented pass)."""
    fn = getattr(_lib.load(), name)
    ev = KERNEL_TIMER.start() if KERNEL_TIMER.enabled else None
    rc = fn(*args)
    if rc:
        COUNTERS.poison()
        _lib.check(rc, name)
    if ev is not None:
        rec = w() if w is not None else (name[5:], name[5:] + "_kernel", "hbm", 0.0)
        KERNEL_TIMER.stop(ev, rec[0], rec[1], rec[2], rec[3], rec[4] if len(rec) > 4 else 1)
    if RECORDER.active:
        if w is not None:
            RECORDER.work[len(RECORDER.prog)] = w()
        RECORDER.prog.append((fn, args))
    if CALL_LOG is not None:
        CALL_LOG.append(name)


CALL_LOG: Optional[list] = None       # a list: receives the name of every libdosx entry point issued (call_log)


@contextlib.contextmanager
def call_log():
    """Scope whose libdosx calls are listed by name, in issue order: ``with call_log() as names: ...`` (what an eagerly issued
    or graph-captured step launched: train.Trainer.program_stats; a recorded one has its Program)."""
    global CALL_LOG
    before, CALL_LOG = CALL_LOG, []
    try:
        yield CALL_LOG
    finally:
        CALL_LOG = before


def alloc(device, *shape) -> torch.Tensor:
    """Uninitialised fp32 device buffer (kept alive for the recorded program while recording)."""
    t = torch.empty(shape, device=device, dtype=torch.float32)
    if RECORDER.active:
        RECORDER.keep.append(t)
    return t


def zeros(device, *shape) -> torch.Tensor:
    t = alloc(device, *shape)
    fill(t, 0.0)
    return t


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk_f32(*ts):
    for t in ts:
        if t is not None:
            if t.dtype != torch.float32 or not t.is_cuda:
                raise TypeError(f"dosx ops need float32 CUDA tensors, got {t.dtype} on {t.device}")


def ident() -> RowMap:
    return RowMap(BIG, 0, 1, 0, None)


def rowmap(d: int = BIG, m: int = 0, c: int = 1, off: int = 0, idx: Optional[torch.Tensor] = None) -> RowMap:
    """row(r) = idx[t] if idx else t,  t = (r // d) * m + (r % d) * c + off."""
    return RowMap(int(d), int(m), int(c), int(off), _p(idx))


def seg(t: torch.Tensor, width: Optional[int] = None, col: int = 0, rmap: Optional[RowMap] = None) -> Seg:
    """A K-segment: columns [col, col+width) of the 2-D row-major tensor ``t`` (rows via rmap)."""
    assert t.dim() == 2 and t.stride(1) == 1, "segment must be 2-D with unit inner stride"
    w = t.shape[1] - col if width is None else width
    return Seg(t.data_ptr() + 4 * col, int(t.stride(0)), int(w), rmap if rmap is not None else ident())


def _set_segs(dst, segs: Sequence[Seg]):
    assert 1 <= len(segs) <= 3
    for i, s in enumerate(segs):
        dst[i] = s


def gemm(M: int, N: int, segs: Sequence[Seg], w: torch.Tensor, out: torch.Tensor, **kw) -> None:
    """out[M,N] = epilogue(prologue(A) @ B); the keywords are :func:`_gemm_desc`'s."""
    g = _gemm_desc(M, N, segs, w, out, **kw)
    _call("dosx_gemm", C.byref(g), _stream(), w=lambda: _gemm_work(g))


def gemm_pair(first: dict, second: dict) -> None:
    """Two independent GEMMs (keyword dictionaries of :func:`gemm`: M, N, segs, w, out, ...) as ONE launch when they share a
    tile configuration - same N, W[N,K], plain epilogue, aligned operands - else one after the other (include/dosx.h:
    dosx_gemm_pair)."""
    g1, g2 = _gemm_desc(**first), _gemm_desc(**second)

    def work():
        t1, t2 = _gemm_work(g1), _gemm_work(g2)
        return (f"gemm_pair[N{g1.N},K{g1.K}+{g2.K}]", "gemm_pair_kernel", "mfma", t1[3] + t2[3])
    _call("dosx_gemm_pair", C.byref(g1), C.byref(g2), _stream(), w=work)


def _gemm_desc(M: int, N: int, segs: Sequence[Seg], w: torch.Tensor, out: torch.Tensor, *, w_layout: int = 0,
               pro: int = PRO_NONE, pro_gamma=None, pro_beta=None, pro_alpha=None, pro_stats=None,
               epi: int = EPI_BIAS_ACT, act: int = ACT_NONE, act_slope: float = 0.01, bias=None,
               out_map: Optional[RowMap] = None, res=None, res_map: Optional[RowMap] = None,
               stats_out=None, aux_out=None, aux=None, aux_stats=None, epi_gamma=None, epi_beta=None,
               epi_alpha=None, partials=None, partial_ld: int = 0, res_col0: int = 0, seg_tile=None, seg_rowptr=None,
               seg_scale=None, seg_agg=None, norm_out=None, norm_rstd=None, res_pre: bool = False,
               add_p=None, add_ip=None, add_q=None, add_iq=None, w_seg_off: int = 0) -> "Gemm":
    """The descriptor of out[M,N] = epilogue(prologue(A) @ B); see include/dosx.h:DosxGemm."""
    g = Gemm()
    g.M, g.N = int(M), int(N)
    g.K = int(sum(s.width for s in segs))
    g.nseg = len(segs)
    _set_segs(g.a, segs)
    g.pro = pro
    g.pro_gamma, g.pro_beta, g.pro_alpha, g.pro_stats = _p(pro_gamma), _p(pro_beta), _p(pro_alpha), _p(pro_stats)
    assert w.dim() == 2 and w.stride(1) == 1
    g.w, g.ldw, g.w_layout = w.data_ptr(), int(w.stride(0)), int(w_layout)
    g.epi, g.act, g.act_slope = epi, act, float(act_slope)
    g.bias = _p(bias)
    g.out, g.ldo = (out.data_ptr(), int(out.stride(0))) if out is not None else (None, int(N))
    g.out_map = out_map if out_map is not None else ident()
    g.res = _p(res)
    g.ldr = int(res.stride(0)) if res is not None else 0
    g.res_map = res_map if res_map is not None else ident()
    g.stats_out, g.aux_out = _p(stats_out), _p(aux_out)
    if norm_out is not None:
        assert norm_rstd is not None and out is not None and norm_out.stride(0) == out.stride(0)
        g.norm_out, g.norm_rstd = norm_out.data_ptr(), norm_rstd.data_ptr()
    g.aux = _p(aux)
    g.ldaux = int(aux.stride(0)) if aux is not None else 0
    g.aux_stats = _p(aux_stats)
    g.epi_gamma, g.epi_beta, g.epi_alpha = _p(epi_gamma), _p(epi_beta), _p(epi_alpha)
    g.partials, g.partial_ld = _p(partials), int(partial_ld)
    g.res_col0 = int(res_col0)
    g.res_pre = 1 if res_pre else 0
    g.w_seg_off = int(w_seg_off)
    if add_p is not None:               # EPI_LN: gathered row addends (the factored EdgeModel Linear)
        assert add_q is not None and add_ip is not None and add_iq is not None and add_p.stride(0) == add_q.stride(0)
        assert add_ip.dtype == torch.int32 and add_iq.dtype == torch.int32
        g.add_p, g.add_ip, g.add_q, g.add_iq = add_p.data_ptr(), add_ip.data_ptr(), add_q.data_ptr(), add_iq.data_ptr()
        g.ld_add = int(add_p.stride(0))
    if seg_tile is not None:            # EPI_SEGSUM / EPI_PRELU_LN_BWD_SEG: [3, T+1] node-aligned tile table
        assert seg_tile.dim() == 2 and seg_tile.shape[0] == 3 and seg_tile.is_contiguous()
        g.seg_tile, g.seg_ntiles = seg_tile.data_ptr(), int(seg_tile.shape[1]) - 1
        g.seg_rowptr, g.seg_scale, g.seg_agg = _p(seg_rowptr), _p(seg_scale), _p(seg_agg)
        # chunk sums of over-full nodes (in-degree > 48) + their arrival counters: always there, a table may hold such tiles
        part = alloc(w.device, g.seg_ntiles, g.N)
        g.seg_part, g.seg_cnt = part.data_ptr(), COUNTERS.take(w.device, g.seg_ntiles)
    return g


def _gemm_work(g: Gemm):
    buf = C.create_string_buffer(96)
    _lib.load().dosx_gemm_kernel_name(C.byref(g), buf, 96)
    sym = buf.value.decode()
    # keyed by kernel symbol + (N, K): the batches of a run differ in M only and belong to one site
    return (f"gemm[N{g.N},K{g.K},{sym[11:]}]", sym, "mfma", 2.0 * _real(g.M) * g.N * g.K)


def ffn_supported(H: int) -> bool:
    return bool(_lib.load().dosx_ffn_supported(int(H)))


def ffn_att_supported(H: int, Nk: int) -> bool:
    return bool(_lib.load().dosx_ffn_att_supported(int(H), int(Nk)))


def ffn_att_aligned_supported(H: int, Nk: int) -> bool:
    return bool(_lib.load().dosx_ffn_att_aligned_supported(int(H), int(Nk)))


class Head(NamedTuple):
    """An encoder's final LayerNorm inside the feed-forward launches of its last layer (DosxFfn.fin_* / DosxFfnBwd.fin_*) and,
    with ``w`` set, the model's H -> 1 output layer behind it.  Forward (ffn_fwd): reads gamma, beta (, w, b), writes xhat
    [rows, H], rstd [rows] (, dos [Bq, S]).  Backward (ffn_bwd): reads gamma, xhat, rstd (, w, beta, ddos [Bq, S]) and writes
    dy [rows, H], the gradient in front of the LayerNorm.  S, Bq: the row layout behind dos / ddos (row = s * Bq + bq).
    keys: the names of the gradients (LayerNorm weight, bias (, output weight, bias)) - functional.encoder_bwd's, not read here."""
    gamma: torch.Tensor
    beta: torch.Tensor
    xhat: torch.Tensor
    rstd: torch.Tensor
    w: Optional[torch.Tensor] = None
    b: Optional[torch.Tensor] = None
    dos: Optional[torch.Tensor] = None
    ddos: Optional[torch.Tensor] = None
    dy: Optional[torch.Tensor] = None
    S: int = 0
    Bq: int = 0
    keys: Tuple[str, ...] = ()


class AttFwd(NamedTuple):
    """The attention half of an encoder layer inside dosx_ffn_fwd (include/dosx.h: DosxFfn.att_*): ffn_fwd's ``x`` is then the
    layer input (query rows at s * qs + b * qb); probs, qstats, x1, st1 are written.  aligned: crystal-aligned tiles."""
    kvhat: torch.Tensor
    gamma0: torch.Tensor
    beta0: torch.Tensor
    Nk: int
    Bk: int
    Bq: int
    Sq: int
    qs: int
    qb: int
    probs: torch.Tensor
    qstats: torch.Tensor
    x1: torch.Tensor
    st1: torch.Tensor
    mask: Optional[torch.Tensor] = None
    aligned: bool = False
    key_ptr: Optional[torch.Tensor] = None


class AttBwd(NamedTuple):
    """The attention half's backward inside dosx_ffn_bwd (include/dosx.h: DosxFfnBwd.att_*).  partials_q / partials_kv / dkv_cnt
    are device addresses (the two halves of one partial-row buffer; ops.COUNTERS.take).  ``dkvhat`` None: the query-only form -
    no key gradient; ``partials_kv`` / ``dkv_part`` / ``dkv_cnt`` may then be None too (nothing touches them)."""
    x: torch.Tensor
    kvhat: torch.Tensor
    gamma0: torch.Tensor
    beta0: torch.Tensor
    probs: torch.Tensor
    qstats: torch.Tensor
    dxin: torch.Tensor
    partials_q: int
    partials_kv: Optional[int]
    dkv_part: Optional[torch.Tensor]
    dkv_cnt: Optional[int]
    dkvhat: Optional[torch.Tensor]
    accumulate: int
    Nk: int
    Bk: int
    Bq: int
    Sq: int
    qs: int
    qb: int
    mask: Optional[torch.Tensor] = None
    key_ptr: Optional[torch.Tensor] = None


def ffn_fwd(M: int, H: int, x: torch.Tensor, stats: Optional[torch.Tensor], gamma, beta, w1, b1, w2, b2, h: torch.Tensor,
            out: torch.Tensor, fin: Optional[Head] = None, att: Optional[AttFwd] = None, defer: Optional[list] = None) -> None:
    """out = x + fc2(relu(fc1(LN1(x)))), h = relu(fc1(LN1(x))) in one launch (include/dosx.h: DosxFfn).
    ``fin``: also apply the encoder's final LayerNorm (out = LN(...), xhat / rstd saved) and, with ``fin.w`` set, the H -> 1
    output layer behind it (``out`` may be None then).  A bare ``(gamma, beta, xhat, rstd)`` is read as Head(gamma, beta, xhat, rstd)."""
    a = _ffn_desc(M, H, x, stats, gamma, beta, w1, b1, w2, b2, h, out, fin, att)
    nk_att = a.att_Nk if att is not None else 0
    if defer is not None:            # (encoder_fwd: the layers of a stack go out together, ffn_fwd_multi)
        defer.append((a, 16.0 * M * H * H + 4.0 * M * nk_att * H))
        return
    _call("dosx_ffn_fwd", C.byref(a), _stream(),
          w=lambda: (f"ffn_fwd[H{H}{',att' if nk_att else ''}]", "ffn_fwd_kernel", "mfma", 16.0 * M * H * H + 4.0 * M * nk_att * H))


def _ffn_desc(M: int, H: int, x, stats, gamma, beta, w1, b1, w2, b2, h, out, fin: Optional[Head], att: Optional[AttFwd]) -> "Ffn":
    a = Ffn()
    a.M, a.H = int(M), int(H)
    a.x, a.ldx = x.data_ptr(), int(x.stride(0))
    a.stats = _p(stats)
    a.gamma, a.beta = gamma.data_ptr(), beta.data_ptr()
    a.w1, a.b1, a.w2, a.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    a.h, a.ldh = h.data_ptr(), int(h.stride(0))
    if out is not None:
        a.out, a.ldo = out.data_ptr(), int(out.stride(0))
    if att is not None:             # the attention half of the layer in the same launch: ``x`` is then the layer input
        a.att_kvhat, a.att_gamma0, a.att_beta0 = att.kvhat.data_ptr(), att.gamma0.data_ptr(), att.beta0.data_ptr()
        a.att_mask = _p(att.mask)
        a.att_probs, a.att_qstats = att.probs.data_ptr(), att.qstats.data_ptr()
        a.att_x1, a.att_ldx1, a.att_st1 = att.x1.data_ptr(), int(att.x1.stride(0)), att.st1.data_ptr()
        a.att_Nk, a.att_Bk, a.att_Bq, a.att_Sq = int(att.Nk), int(att.Bk), int(att.Bq), int(att.Sq)
        a.att_qs, a.att_qb = int(att.qs), int(att.qb)
        a.att_aligned = int(bool(att.aligned))
        if att.key_ptr is not None:
            a.att_key_ptr = att.key_ptr.data_ptr()
    if fin is not None:
        if not isinstance(fin, Head):      # a bare (gamma, beta, xhat, rstd) - Head's four required fields, in their order - is
            gamma_f, beta_f, xhat_f, rstd_f = fin          # still taken (the final LayerNorm alone); any other length raises
            fin = Head(gamma_f, beta_f, xhat_f, rstd_f)
        a.fin_gamma, a.fin_beta, a.fin_xhat, a.fin_rstd = fin.gamma.data_ptr(), fin.beta.data_ptr(), fin.xhat.data_ptr(), fin.rstd.data_ptr()
        if fin.w is not None:      # the model head's H -> 1 output layer on the normalised rows
            a.fin_w, a.fin_b, a.fin_dos, a.fin_S, a.fin_Bq = fin.w.data_ptr(), fin.b.data_ptr(), fin.dos.data_ptr(), int(fin.S), int(fin.Bq)
    return a


FFN_MULTI_MAX = 2          # layers per dosx_ffn_fwd_multi launch (csrc/ffn.hip)


def ffn_fwd_multi(deferred: list) -> None:
    """The deferred layers of ONE encoder stack (ffn_fwd(..., defer=list)), FFN_MULTI_MAX per launch (include/dosx.h:
    dosx_ffn_fwd_multi): every layer carries its attention half and reads the previous one's output rows."""
    for i in range(0, len(deferred), FFN_MULTI_MAX):
        grp = deferred[i:i + FFN_MULTI_MAX]
        arr = (Ffn * len(grp))(*[d for d, _ in grp])
        work = sum(w for _, w in grp)
        H = grp[0][0].H
        if len(grp) == 1:
            _call("dosx_ffn_fwd", C.byref(arr[0]), _stream(), w=lambda H=H, work=work: (f"ffn_fwd[H{H},att]", "ffn_fwd_kernel", "mfma", work))
        else:
            _call("dosx_ffn_fwd_multi", arr, len(grp), _stream(),
                  w=lambda H=H, work=work, n=len(grp): (f"ffn_fwd[H{H},att,x{n}]", "ffn_fwd_multi_kernel", "mfma", work))


def ffn_bwd_partial_rows(M: int) -> int:
    return _lib.load().dosx_ffn_bwd_partial_rows(int(M))


def ffn_att_bwd_supported(H: int, Nk: int, Sq: int, Bq: int) -> bool:
    return bool(_lib.load().dosx_ffn_att_bwd_supported(int(H), int(Nk), int(Sq), int(Bq)))


def attention_pkv_supported(Nk: int, H: int) -> bool:
    """Whether dosx_attention_bwd keeps every query tile's share of dK + dV in ``dkv_part`` (small key sets) instead of
    streaming the scores' gradient through ``dscores``."""
    return bool(_lib.load().dosx_attention_pkv_supported(int(Nk), int(H)))


def ffn_att_bwd_partial_rows(Sq: int, Bq: int) -> int:
    return _lib.load().dosx_ffn_att_bwd_partial_rows(int(Sq), int(Bq))


def ffn_bwd(M: int, H: int, dy: torch.Tensor, h: torch.Tensor, x: torch.Tensor, stats: torch.Tensor, gamma, w1, w2,
            dh: torch.Tensor, dx: Optional[torch.Tensor], partials: torch.Tensor, fin: Optional[Head] = None,
            att: Optional[AttBwd] = None) -> None:
    """dh = (dy W2) o [h>0], dx = dy + LN1_bwd(dh W1), LN1 dgamma|dbeta partial rows — one launch
    (include/dosx.h: DosxFfnBwd).  ``fin``: ``dy`` is the gradient behind the encoder's final LayerNorm, whose backward runs
    first in the same launch (fin.dy receives the result, the partial rows two more column groups); with ``fin.w`` set the
    H -> 1 output layer's backward in front of it (``dy`` None: fin.ddos is the incoming gradient)."""
    a = _ffn_bwd_desc(M, H, dy, h, x, stats, gamma, w1, w2, dh, dx, partials, fin, att)
    nk_att = a.att_Nk if att is not None else 0
    _call("dosx_ffn_bwd", C.byref(a), _stream(),
          w=lambda: (f"ffn_bwd[H{H}{',att' if nk_att else ''}{',q' if att is not None and att.dkvhat is None else ''}]", "ffn_bwd_kernel",
                     "mfma", 16.0 * M * H * H + (6.0 if att is not None and att.dkvhat is None else 10.0) * M * nk_att * H))


def _ffn_bwd_desc(M: int, H: int, dy, h, x, stats, gamma, w1, w2, dh, dx, partials, fin: Optional[Head], att: Optional[AttBwd]):
    a = _lib.FfnBwd()
    if fin is not None:
        a.fin_gamma, a.fin_xhat, a.fin_rstd, a.fin_dy = fin.gamma.data_ptr(), fin.xhat.data_ptr(), fin.rstd.data_ptr(), fin.dy.data_ptr()
        if fin.w is not None:      # the H -> 1 output layer in front of that LayerNorm
            a.fin_ddos, a.fin_w, a.fin_beta, a.fin_S, a.fin_Bq = fin.ddos.data_ptr(), fin.w.data_ptr(), fin.beta.data_ptr(), int(fin.S), int(fin.Bq)
    a.M, a.H = int(M), int(H)
    if dy is not None:
        a.dy, a.lddy = dy.data_ptr(), int(dy.stride(0))
    else:
        a.lddy = int(fin.dy.stride(0))
    a.h, a.ldh = h.data_ptr(), int(h.stride(0))
    a.x, a.ldx = x.data_ptr(), int(x.stride(0))
    a.stats, a.gamma = stats.data_ptr(), gamma.data_ptr()
    a.w1, a.w2 = w1.data_ptr(), w2.data_ptr()
    a.dh, a.lddh = dh.data_ptr(), int(dh.stride(0))
    if dx is not None:
        a.dx, a.lddx = dx.data_ptr(), int(dx.stride(0))
    a.partials, a.partial_ld = partials.data_ptr(), int(partials.stride(0))
    if att is not None:             # the attention half's backward in the same launch
        a.att_x, a.att_ldxin = att.x.data_ptr(), int(att.x.stride(0))
        a.att_kvhat, a.att_gamma0, a.att_beta0 = att.kvhat.data_ptr(), att.gamma0.data_ptr(), att.beta0.data_ptr()
        a.att_probs, a.att_qstats, a.att_mask = att.probs.data_ptr(), att.qstats.data_ptr(), _p(att.mask)
        a.att_dxin, a.att_lddxin = att.dxin.data_ptr(), int(att.dxin.stride(0))
        a.att_partials_q = att.partials_q
        if att.dkvhat is not None:
            a.att_partials_kv, a.att_dkv_part, a.att_dkv_cnt = att.partials_kv, att.dkv_part.data_ptr(), att.dkv_cnt
            a.att_dkvhat, a.att_dkv_accumulate = att.dkvhat.data_ptr(), int(att.accumulate)
        a.att_Nk, a.att_Bk, a.att_Bq, a.att_Sq = int(att.Nk), int(att.Bk), int(att.Bq), int(att.Sq)
        a.att_qs, a.att_qb = int(att.qs), int(att.qb)
        if att.key_ptr is not None:
            a.att_key_ptr = att.key_ptr.data_ptr()
    return a


MLP_LN_MAX_ROWS = 4096
MLP_LN_MAX_KN = 256 * 256           # (tests lower / raise it to force the other form at a given shape)
# the FORWARD kernel alone also at hidden 256 (round 5: weight chunks four deep - 37.4 us against 30 + 13.5 + a launch gap for the
# two GEMMs at 1554 rows; the backward stays on its two GEMMs there: 39.7 against 35.0)
MLP_LN_MAX_KN_FWD = 512 * 512


def mlp_ln_supported(M: int, K: int, NH: int, NO: int) -> bool:
    """Whether the one-launch Linear-LN-PReLU-Linear kernel (include/dosx.h: DosxMlpLn) takes this block: its 16-row
    workgroups are the better cut while they are at most one round of the 256 CUs (M <= 4096 rows) and one workgroup's
    serial share of the weights is small (hidden <= 128: 13.7 + 14.5 us fwd + bwd against 2 x 2 launches of ~9.7 us at
    450 rows; at hidden 256 / 1554 rows the backward measured 42.9 against 33.9 us - tools/bench_kernels.py --what nmlp)."""
    return 0 < M <= MLP_LN_MAX_ROWS and K * NH <= MLP_LN_MAX_KN and bool(_lib.load().dosx_mlp_ln_supported(int(K), int(NH), int(NO)))


def mlp_ln_fwd_supported(M: int, K: int, NH: int, NO: int) -> bool:
    """... for the forward launch alone (the backward of the same block may run as two GEMMs: same saved tensors)."""
    return 0 < M <= MLP_LN_MAX_ROWS and K * NH <= MLP_LN_MAX_KN_FWD and bool(_lib.load().dosx_mlp_ln_supported(int(K), int(NH), int(NO)))


# Column-split form of the one-launch NodeModel kernels (round 6, include/dosx.h: DosxMlpLn.cs_buf): hidden / 16 workgroups per
# 16-row tile instead of one, while that grid stays a single round of small workgroups (profiles/r06_ab_cs.log)
MLP_LN_CS_MAX_WGS = 512


def mlp_ln_cs(M: int, K: int, NH: int, NO: int) -> bool:
    """Whether mlp_ln_fwd / mlp_ln_bwd run the column-split form for this block."""
    return bool(M > 0 and _lib.load().dosx_mlp_ln_cs_supported(int(K), int(NH), int(NO))
                and ((int(M) + 15) // 16) * (int(NO) // 16) <= MLP_LN_CS_MAX_WGS)


def _mlp_ln_cs_scratch(d, dev, M: int, NH: int) -> None:
    lib = _lib.load()
    buf = alloc(dev, int(lib.dosx_mlp_ln_cs_scratch_floats(int(M), int(NH))))
    d._cs_keep = buf
    d.cs_buf, d.cs_cnt = buf.data_ptr(), COUNTERS.take(dev, lib.dosx_mlp_ln_cs_tiles(int(M)))


def mlp_ln_fwd(M: int, a0: torch.Tensor, a1: Optional[torch.Tensor], w1, b1, gamma, beta, alpha, w2, b2,
               res: Optional[torch.Tensor], xhat: torch.Tensor, rstd: torch.Tensor, out: torch.Tensor,
               w3: Optional[torch.Tensor] = None, nb3: int = 0, pq: Optional[torch.Tensor] = None, cs: Optional[bool] = None) -> None:
    """out = prelu(LN([a0|a1] W1^T + b1)) W2^T + b2 (+ res); xhat / rstd saved (include/dosx.h: DosxMlpLn).
    w3 [n3, >= nb3 * NO] + pq [M, nb3 * n3]: the third product pq[:, b n3 + n] = out . w3[n, b NO:(b + 1) NO].
    cs: column-split form (None: the policy of :func:`mlp_ln_cs`)."""
    d = _lib.MlpLn()
    k0 = int(a0.shape[1])
    d.M, d.K, d.NH, d.NO, d.k0 = int(M), k0 + (int(a1.shape[1]) if a1 is not None else 0), int(w1.shape[0]), int(w2.shape[0]), k0
    d.a0, d.lda0 = a0.data_ptr(), int(a0.stride(0))
    if a1 is not None:
        d.a1, d.lda1 = a1.data_ptr(), int(a1.stride(0))
    d.w1, d.b1, d.gamma, d.beta, d.alpha = w1.data_ptr(), b1.data_ptr(), gamma.data_ptr(), beta.data_ptr(), alpha.data_ptr()
    d.w2, d.b2 = w2.data_ptr(), b2.data_ptr()
    if res is not None:
        d.res, d.ldres = res.data_ptr(), int(res.stride(0))
    d.xhat, d.rstd = xhat.data_ptr(), rstd.data_ptr()
    d.out, d.ldo = out.data_ptr(), int(out.stride(0))
    if w3 is not None:
        assert pq is not None and w3.stride(1) == 1 and pq.stride(1) == 1 and pq.shape[1] == nb3 * w3.shape[0]
        d.w3, d.ldw3, d.n3, d.nb3 = w3.data_ptr(), int(w3.stride(0)), int(w3.shape[0]), int(nb3)
        d.pq, d.ldpq = pq.data_ptr(), int(pq.stride(0))
    if cs is None:
        cs = mlp_ln_cs(d.M, d.K, d.NH, d.NO) and d.k0 % (d.K // 4) == 0
    if cs:
        _mlp_ln_cs_scratch(d, out.device, d.M, d.NH)
    _call("dosx_mlp_ln_fwd", C.byref(d), _stream(),
          w=lambda: (f"mlp_ln_fwd[K{d.K},NH{d.NH},NO{d.NO}" + (",pq" if d.w3 else "") + (",cs" if cs else "") + "]",
                     "mlp_ln_cs_fwd_kernel" if cs else "mlp_ln_fwd_kernel", "mfma",
                     2.0 * _real(d.M) * (d.NH * (d.K + d.NO) + d.nb3 * d.n3 * d.NO)))


def mlp_ln_bwd_partial_rows(M: int) -> int:
    return _lib.load().dosx_mlp_ln_bwd_partial_rows(int(M))


def mlp_ln_bwd_cs(M: int, K: int, NH: int, NO: int, dcat: torch.Tensor, with_pre: bool = False) -> bool:
    """Whether mlp_ln_bwd runs the column-split form for this block and this dcat layout: only where it is asked to absorb the
    launch in front of it (``with_pre``, DosxMlpLnBwd.pre).  Inside the step the backward N-row launches share the GPU with a
    weight-gradient group: 232 small workgroups that wait for each other then cost MORE than 29 large ones (1.0940 vs 1.0855 ms per
    cfg2 step, three interleaved rounds) - unlike in the forward pass, where the chip is otherwise idle (1.1018 -> 1.0940 with the
    forward launches alone) - but absorbing the dense-key backward launch in front of the last layer's NodeModel backward pays well
    beyond that (1.0726; profiles/r06_ab_run3.log)."""
    return with_pre and mlp_ln_cs(M, K, NH, NO) and int(dcat.stride(0)) % 2 == 0 and dcat.data_ptr() % 8 == 0


def mlp_ln_bwd(M: int, dy: torch.Tensor, xhat: torch.Tensor, rstd: torch.Tensor, w1, w2, gamma, beta, alpha, dz: torch.Tensor,
               dcat: torch.Tensor, partials: torch.Tensor, add_dy: bool = False, cs: Optional[bool] = None, pre: Optional[dict] = None) -> None:
    """dz = LN/PReLU backward of (dy W2), dcat = dz W1, [dgamma | dbeta | .. | dalpha] partial rows - one launch
    (include/dosx.h: DosxMlpLnBwd).
    pre (column-split form only): what produces ``dy`` in the same launch - dict(kind="node_grad", dz, rowptr_src, perm_src, aggd, w,
    res, res2, aggs) = :func:`node_grad` with dx = dy, or dict(kind="dense", dkv, kvhat, rstd_nodes, dense_row, dpool_ptr, ld_dpool,
    node_graph, num_graphs, ghost_row) = :func:`dense_normalize_pool_bwd` with dx = dy."""
    d = _lib.MlpLnBwd()
    d.M, d.K, d.NH, d.NO = int(M), int(w1.shape[1]), int(w1.shape[0]), int(w2.shape[0])
    d.dy, d.lddy = dy.data_ptr(), int(dy.stride(0))
    d.xhat, d.rstd = xhat.data_ptr(), rstd.data_ptr()
    d.w1, d.w2 = w1.data_ptr(), w2.data_ptr()
    d.gamma, d.beta, d.alpha = gamma.data_ptr(), beta.data_ptr(), alpha.data_ptr()
    d.dz = dz.data_ptr()
    d.dcat, d.lddcat = dcat.data_ptr(), int(dcat.stride(0))
    d.partials, d.partial_ld = partials.data_ptr(), int(partials.stride(0))
    d.add_dy = 1 if add_dy else 0
    if cs is None:
        cs = mlp_ln_bwd_cs(d.M, d.K, d.NH, d.NO, dcat, with_pre=pre is not None)
    extra = 0.0
    if pre is not None:
        assert cs, "mlp_ln_bwd: pre needs the column-split form"
        assert dy.stride(1) == 1
        d.pre_dy = dy.data_ptr()
        if pre["kind"] == "node_grad":
            d.pre = 1
            w = pre["w"]
            assert pre["dz"].is_contiguous() and pre["aggd"].is_contiguous() and pre["aggs"].is_contiguous() and w.stride(1) == 1
            d.pre_dz, d.pre_rowptr_src, d.pre_perm_src = pre["dz"].data_ptr(), pre["rowptr_src"].data_ptr(), pre["perm_src"].data_ptr()
            d.pre_aggd, d.pre_aggs = pre["aggd"].data_ptr(), pre["aggs"].data_ptr()
            d.pre_w, d.pre_ldw = w.data_ptr(), int(w.stride(0))
            if pre.get("res") is not None:
                d.pre_res, d.pre_ldres = pre["res"].data_ptr(), int(pre["res"].stride(0))
            if pre.get("res2") is not None:
                d.pre_res2, d.pre_ldres2 = pre["res2"].data_ptr(), int(pre["res2"].stride(0))
            extra = 2.0 * _real(d.M) * d.NO * 4 * d.NO
        else:
            assert pre["kind"] == "dense"
            d.pre = 2
            d.pre_dkv, d.pre_kvhat, d.pre_rstd_nodes = pre["dkv"].data_ptr(), pre["kvhat"].data_ptr(), pre["rstd_nodes"].data_ptr()
            d.pre_dense_row, d.pre_node_graph = pre["dense_row"].data_ptr(), pre["node_graph"].data_ptr()
            d.pre_dpool, d.pre_ld_dpool = int(pre["dpool_ptr"]), int(pre["ld_dpool"])
            d.pre_num_graphs, d.pre_ghost_row = int(pre["num_graphs"]), int(pre["ghost_row"])
    if cs:
        _mlp_ln_cs_scratch(d, dz.device, d.M, d.NH)
    tag = "" if pre is None else ("," + pre["kind"])
    _call("dosx_mlp_ln_bwd", C.byref(d), _stream(),
          w=lambda: (f"mlp_ln_bwd[K{d.K},NH{d.NH},NO{d.NO}" + (",cs" if cs else "") + tag + "]",
                     "mlp_ln_cs_bwd_kernel" if cs else "mlp_ln_bwd_kernel", "mfma", 2.0 * _real(d.M) * d.NH * (d.K + d.NO) + extra))


def edge_mlp_supported(H: int) -> bool:
    return bool(_lib.load().dosx_edge_mlp_supported(int(H)))


def edge_mlp_fwd(E: int, H: int, e: torch.Tensor, pq: torch.Tensor, src, dst, w1c: torch.Tensor, b1, gamma, beta, alpha, w3, b3,
                 xhat: torch.Tensor, rstd: torch.Tensor, e_out: Optional[torch.Tensor], seg_tile, seg_rowptr, seg_scale, seg_agg) -> None:
    """The EdgeModel (first Linear factored: ``pq`` = the two node products, ``w1c`` = its edge block [2H, H] as a view of the
    [2H, 3H] weight) + scatter_mean / scatter_sum + the edge residual in one launch (include/dosx.h: DosxEdgeMlp)."""
    d = _lib.EdgeMlp()
    d.E, d.H = int(E), int(H)
    d.e, d.lde = e.data_ptr(), int(e.stride(0))
    d.pq, d.ldpq = pq.data_ptr(), int(pq.stride(0))
    d.src, d.dst = src.data_ptr(), dst.data_ptr()
    assert w1c.stride(1) == 1 and w3.is_contiguous()
    d.w1, d.ldw1, d.b1 = w1c.data_ptr(), int(w1c.stride(0)), b1.data_ptr()
    d.gamma, d.beta, d.alpha = gamma.data_ptr(), beta.data_ptr(), alpha.data_ptr()
    d.w3, d.b3 = w3.data_ptr(), b3.data_ptr()
    d.xhat, d.rstd = xhat.data_ptr(), rstd.data_ptr()
    if e_out is not None:
        d.e_out, d.ldeo = e_out.data_ptr(), int(e_out.stride(0))
    assert seg_tile.dim() == 2 and seg_tile.shape[0] == 3 and seg_tile.is_contiguous()
    d.seg_tile, d.seg_ntiles = seg_tile.data_ptr(), int(seg_tile.shape[1]) - 1
    d.seg_rowptr, d.seg_scale, d.seg_agg = seg_rowptr.data_ptr(), _p(seg_scale), seg_agg.data_ptr()
    part = alloc(e.device, d.seg_ntiles, H)
    d.seg_part, d.seg_cnt = part.data_ptr(), COUNTERS.take(e.device, d.seg_ntiles)
    _call("dosx_edge_mlp_fwd", C.byref(d), _stream(),
          w=lambda: (f"edge_mlp_fwd[H{d.H}]", f"edge_fwd_kernel<{2 * d.H}>", "mfma", 2.0 * _real(d.E) * (2 * d.H) * (2 * d.H)))


def edge_mlp_bwd(E: int, H: int, dagg: torch.Tensor, de_next: Optional[torch.Tensor], dst, xhat, rstd, w3, w1c, gamma, beta, alpha,
                 dmsg: torch.Tensor, dz: torch.Tensor, de: torch.Tensor, partials: torch.Tensor, seg_tile, seg_rowptr, seg_scale,
                 seg_agg: torch.Tensor) -> None:
    """Backward of :func:`edge_mlp_fwd` in one launch (include/dosx.h: DosxEdgeMlpBwd): dagg [nodes, H] (any row stride) and
    de_next [E, H] (None: last layer) -> dmsg, dz, de = dz Wc + de_next, the destination-node sums of dz, the LayerNorm / PReLU
    parameter-gradient partial rows (one per tile)."""
    d = _lib.EdgeMlpBwd()
    d.E, d.H = int(E), int(H)
    d.dagg, d.lddagg = dagg.data_ptr(), int(dagg.stride(0))
    if de_next is not None:
        d.de_next, d.ldden = de_next.data_ptr(), int(de_next.stride(0))
    d.dst = dst.data_ptr()
    d.xhat, d.rstd = xhat.data_ptr(), rstd.data_ptr()
    assert w1c.stride(1) == 1 and w3.is_contiguous() and dmsg.is_contiguous() and dz.is_contiguous()
    d.w3, d.w1, d.ldw1 = w3.data_ptr(), w1c.data_ptr(), int(w1c.stride(0))
    d.gamma, d.beta, d.alpha = gamma.data_ptr(), beta.data_ptr(), alpha.data_ptr()
    d.dmsg, d.dz = dmsg.data_ptr(), dz.data_ptr()
    d.de, d.ldde = de.data_ptr(), int(de.stride(0))
    d.partials, d.partial_ld = partials.data_ptr(), int(partials.stride(0))
    assert seg_tile.dim() == 2 and seg_tile.shape[0] == 3 and seg_tile.is_contiguous()
    d.seg_tile, d.seg_ntiles = seg_tile.data_ptr(), int(seg_tile.shape[1]) - 1
    assert partials.shape[0] >= d.seg_ntiles
    d.seg_rowptr, d.seg_scale, d.seg_agg = seg_rowptr.data_ptr(), _p(seg_scale), seg_agg.data_ptr()
    part = alloc(dz.device, d.seg_ntiles, 2 * H)
    d.seg_part, d.seg_cnt = part.data_ptr(), COUNTERS.take(dz.device, d.seg_ntiles)
    _call("dosx_edge_mlp_bwd", C.byref(d), _stream(),
          w=lambda: (f"edge_mlp_bwd[H{d.H}]", f"edge_bwd_kernel<{2 * d.H}>", "mfma", 2.0 * _real(d.E) * (2 * d.H) * (2 * d.H)))


def node_grad(N: int, H: int, dz: torch.Tensor, rowptr_src, perm_src, aggd: torch.Tensor, w: torch.Tensor, res, res2,
              aggs: torch.Tensor, dx: torch.Tensor) -> None:
    """aggs = source-node sums of dz; dx = res + res2 + aggs W[:, :H] + aggd W[:, H:2H] - one launch (include/dosx.h: DosxNodeGrad)."""
    d = _lib.NodeGrad()
    d.N, d.H = int(N), int(H)
    assert dz.is_contiguous() and aggd.is_contiguous() and aggs.is_contiguous() and w.stride(1) == 1
    d.dz, d.rowptr_src, d.perm_src, d.aggd = dz.data_ptr(), rowptr_src.data_ptr(), perm_src.data_ptr(), aggd.data_ptr()
    d.w, d.ldw = w.data_ptr(), int(w.stride(0))
    if res is not None:
        d.res, d.ldres = res.data_ptr(), int(res.stride(0))
    if res2 is not None:
        d.res2, d.ldres2 = res2.data_ptr(), int(res2.stride(0))
    d.aggs = aggs.data_ptr()
    d.dx, d.lddx = dx.data_ptr(), int(dx.stride(0))
    _call("dosx_node_grad", C.byref(d), _stream(),
          w=lambda: (f"node_grad[H{d.H}]", f"node_grad_kernel<{d.H}>", "mfma", 2.0 * _real(d.N) * d.H * 4 * d.H))


def gemm_partial_rows(M: int, N: int, epi: int) -> int:
    return _lib.load().dosx_gemm_partial_rows(int(M), int(N), int(epi))


def wgrad_splits(M: int, N: int, K: int) -> int:
    return _lib.load().dosx_wgrad_splits(int(M), int(N), int(K))


def wgrad_tiles(N: int, K: int) -> int:
    return _lib.load().dosx_wgrad_tiles(int(N), int(K))


def wgrad_scratch_floats(N: int, K: int, nsplit: int) -> int:
    return int(_lib.load().dosx_wgrad_scratch_floats(int(N), int(K), int(nsplit)))


class _CounterPool:
    """Zeroed int32 arrival counters of the in-launch reductions (include/dosx.h: DosxWgrad.counters, DosxGemm.seg_cnt,
    DosxAttn.dkv_cnt).  A kernel leaves its counters at zero, so they are re-usable - but two launches that can be in
    flight at the same time (different streams) must never share an entry:

    * while a step is RECORDED every request gets memory of its own, kept alive with the program: a replayed program's
      counters are its own for as long as it exists, whatever else runs;
    * eagerly issued launches draw from a per-device ring.  Before the ring hands out an entry a second time the device
      is synchronised (every earlier user has finished and left zeros), and a request larger than the ring replaces it
      with a larger one - a wrap can therefore never alias a launch in flight, and no request is too large;
    * ``poison()`` (a libdosx call failed: an aborted launch may have left tickets behind) drops the ring."""
    SIZE = 1 << 16

    def __init__(self):
        self._bufs = {}
        self._graph_owned = []
        self._recorded = []          # weak references to the counters of recorded programs / captured graphs (zero_fill)

    def take(self, device, n: int) -> int:
        n = int(n)
        if RECORDER.active:
            t = torch.zeros(max(n, 1), dtype=torch.int32, device=device)
            RECORDER.keep.append(t)
            self._recorded.append(weakref.ref(t))
            return t.data_ptr()
        if torch.cuda.is_current_stream_capturing():
            # a captured HIP graph replays for as long as it lives, like a recorded program: counters of its own (the
            # allocation belongs to the graph's memory pool; the zero fill becomes a memset node of the graph)
            t = torch.zeros(max(n, 1), dtype=torch.int32, device=device)
            self._graph_owned.append(t)
            self._recorded.append(weakref.ref(t))
            return t.data_ptr()
        key = str(device)
        ent = self._bufs.get(key)
        if ent is None or n > ent[0].numel():
            if ent is not None:
                torch.cuda.synchronize(device)
            size = self.SIZE
            while size < n:
                size *= 2
            ent = self._bufs[key] = [torch.zeros(size, dtype=torch.int32, device=device), 0]
        if ent[1] + n > ent[0].numel():
            torch.cuda.synchronize(device)        # every earlier user of the ring is done: its entries are zero again
            ent[1] = 0
        off = ent[1]
        ent[1] += n
        return ent[0].data_ptr() + 4 * off

    def poison(self) -> None:
        self._bufs = {}

    def zero_fill(self, device=None) -> None:
        """A stalled column-split exchange was reported (check_exchanges): its launch left tickets behind.  Synchronise and zero every
        counter the pool knows - the eager rings and, through weak references, the counters recorded programs and captured graphs
        own for as long as they live."""
        torch.cuda.synchronize(device)
        for ent in self._bufs.values():
            ent[0].zero_()
            ent[1] = 0
        live = []
        for r in self._recorded:
            t = r()
            if t is not None:
                t.zero_()
                live.append(r)
        self._recorded = live
        torch.cuda.synchronize(device)


COUNTERS = _CounterPool()

EXCHANGE_KERNELS = {_abi.DOSX_EXCHANGE_KERNEL_MLP_LN_CS_FWD: "mlp_ln_cs_fwd", _abi.DOSX_EXCHANGE_KERNEL_ENC_CS_FWD: "enc_cs_fwd",
                    _abi.DOSX_EXCHANGE_KERNEL_MLP_LN_CS_BWD: "mlp_ln_cs_bwd"}


def exchange_status(device, clear: bool = False):
    """The sticky stall status of the column-split exchanges (csrc/mlp2.hip) as four ints ``(code, kernel id, tile, stalls)``:
    one one-thread launch on the current stream and one 16-byte read-back (which waits for that stream)."""
    out = torch.empty(4, dtype=torch.int32, device=device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().dosx_exchange_status(out.data_ptr(), int(bool(clear)), _stream()), "dosx_exchange_status")
    return tuple(int(v) for v in out.cpu().tolist())


def exchange_selftest(device, kernel_id: int, tile: int) -> None:
    """TEST ONLY: file one stall report for (kernel id, tile) without any exchange stalling (dosx_exchange_selftest)."""
    with torch.cuda.device(torch.device(device)):
        _lib.check(_lib.load().dosx_exchange_selftest(int(kernel_id), int(tile), _stream()), "dosx_exchange_selftest")


def check_exchanges(device) -> None:
    """Raise :class:`DosxError` if a column-split exchange reported a stall since the last clean check.  The status is cleared and
    the counter pool zero-filled first (the stalled launch left tickets behind), so the process can go on - but every number the
    device produced since the last clean check is untrustworthy: outputs are not poisoned in between."""
    code, kid, tile, stalls = exchange_status(device)
    if code == 0:
        return
    COUNTERS.zero_fill(device)
    exchange_status(device, clear=True)
    raise _lib.DosxError(
        f"column-split exchange stalled: kernel {EXCHANGE_KERNELS.get(kid, f'#{kid}')}, tile {tile} gave up waiting for its siblings "
        f"({stalls} stall{'s' if stalls != 1 else ''} reported since the last clean check) and went on with a partly published "
        f"tile.  Every number produced since the last clean check is untrustworthy: parameters, optimizer state and predictions "
        f"included.  The status is cleared and the arrival counters are zeroed.")


def wgrad_desc(M: int, N: int, dy: Seg, segs: Sequence[Seg], slab: Optional[torch.Tensor], slab_bias: Optional[torch.Tensor],
               nsplit: int, *, pro: int = PRO_NONE, pro_gamma=None, pro_beta=None, pro_alpha=None, pro_stats=None,
               dst: Optional[torch.Tensor] = None, dst_bias: Optional[torch.Tensor] = None, accumulate: bool = False) -> Wgrad:
    """``dst`` given: finished mode (the kernel reduces the M-splits itself and writes dW / db; ``slab`` / ``slab_bias`` are
    scratch from :func:`wgrad_scratch_floats`); else slab mode (partial sums left for reduce_partials)."""
    g = Wgrad()
    g.M, g.N = int(M), int(N)
    g.K = int(sum(s.width for s in segs))
    g.dy = dy
    g.nseg = len(segs)
    _set_segs(g.a, segs)
    g.pro = pro
    g.pro_gamma, g.pro_beta, g.pro_alpha, g.pro_stats = _p(pro_gamma), _p(pro_beta), _p(pro_alpha), _p(pro_stats)
    g.slab, g.slab_bias, g.nsplit = _p(slab), _p(slab_bias), int(nsplit)
    g._real_M = _real(g.M)            # (the job is launched later, at a flush point outside the scope it was described in)
    if dst is not None:
        # [N, K] contiguous, or a column block of a wider gradient (unit inner stride): DosxWgrad.ldd
        assert dst.dtype == torch.float32 and dst.numel() == g.N * g.K and (dst.is_contiguous() or (dst.dim() == 2 and dst.stride(1) == 1))
        g.dst, g.dst_bias, g.accumulate = dst.data_ptr(), _p(dst_bias), int(bool(accumulate))
        if not dst.is_contiguous():
            g.ldd = int(dst.stride(0))
        if nsplit > 1:
            g.counters = COUNTERS.take(dst.device, wgrad_tiles(g.N, g.K))
    return g


def wgrad(M: int, N: int, dy: Seg, segs: Sequence[Seg], slab: Optional[torch.Tensor], slab_bias: Optional[torch.Tensor],
          nsplit: int, **kw) -> None:
    g = wgrad_desc(M, N, dy, segs, slab, slab_bias, nsplit, **kw)
    _call("dosx_wgrad", C.byref(g), _stream(),
          w=lambda: (f"wgrad[N{g.N},K{g.K}]", "wgrad_kernel", "mfma", 2.0 * g._real_M * g.N * g.K))


def _reduce_job_array(jobs):
    arr = (ReduceJob * max(len(jobs), 1))()
    for i, j in enumerate(jobs):
        arr[i].src, arr[i].dst, arr[i].nsplit, arr[i].stride, arr[i].count, arr[i].accumulate = j
    return arr


def grad_flush(descs: Sequence[Wgrad], rjobs: Sequence[tuple] = ()) -> None:
    """The weight-gradient jobs and the row-partial reductions of one flush point in as few launches as possible - one,
    normally (include/dosx.h: dosx_grad_flush).  ``rjobs``: (src, dst, nsplit, stride, count, accumulate) tuples with
    distinct destinations."""
    if not descs and not rjobs:
        return
    arr = (Wgrad * max(len(descs), 1))(*descs)
    rarr = _reduce_job_array(rjobs)
    # (device kernels of this call: one per table of 8 weight-gradient jobs / 40 reductions, csrc/gemm.hip: dosx_grad_flush)
    nk = max(-(-len(descs) // 8), -(-len(rjobs) // 40), 1)
    _call("dosx_grad_flush", arr, len(descs), rarr, len(rjobs), _stream(),
          w=lambda: ("wgrad_grouped", "wgrad_grouped_kernel", "mfma", sum(2.0 * getattr(d, "_real_M", d.M) * d.N * d.K for d in descs), nk))


def wgrad_grouped(descs: Sequence[Wgrad]) -> None:
    """All the jobs in as few launches as possible (include/dosx.h: dosx_wgrad_grouped)."""
    grad_flush(descs, ())


def concurrent(device, side_fn, main_fn) -> None:
    """``side_fn`` (kernel launches) on the side stream NEXT TO ``main_fn`` on the current one: both ordered after
    everything issued so far on the current stream, which waits for the side work at the end.  Recorded like every stream
    fork / join (replayed programs, HIP-graph capture); eagerly issued steps run the two one after the other."""
    if not GradSink.use_side_stream:
        side_fn()
        main_fn()
        return
    main = torch.cuda.current_stream()
    # the SIDE stream of the recorded programs, not a stream of its own: a process has a handful of hardware queues (main,
    # side, weight-gradient, RCCL's), and a fifth software stream shares one of them - measured: the data-parallel step of a
    # process that had merely CREATED one more stream went from 1.31 to 1.38 ms
    key = (str(device), torch.cuda.is_current_stream_capturing())
    if key not in GradSink._side_streams:
        GradSink._side_streams[key] = torch.cuda.Stream(device=device)
    st = GradSink._side_streams[key]
    ev = torch.cuda.Event()
    ev.record(main)
    st.wait_event(ev)
    if RECORDER.active:
        RECORDER.prog.append((ev.record, (main,)))
        RECORDER.prog.append((st.wait_event, (ev,)))
    with torch.cuda.stream(st):
        side_fn()
    main_fn()
    main.wait_stream(st)
    if RECORDER.active:
        RECORDER.prog.append((main.wait_stream, (st,)))


class GradSink:
    """Collects the partial-sum slabs produced during a backward pass and reduces all of them
    into the parameter-gradient buffers with ONE deterministic kernel launch per 'wave'
    (jobs that share a destination are serialised into successive waves)."""

    # Weight-gradient (wgrad) and key/value-gradient kernels feed nothing but the final slab reduction,
    # so they are launched on a SIDE stream and run concurrently with the dgrad chain on the main stream:
    # at BASELINE sizes every kernel is one partial wave of workgroups, two streams simply fill more CUs.
    # Off for eagerly issued steps (the host cannot feed two streams from Python: no gain), switched on by
    # train.Trainer while it records a replayed step (1.80 vs 1.88 ms serialised).
    use_side_stream = False
    # ... with the grouped weight-gradient launches + slab reductions on a THIRD stream of their own (`wside`), flushed after every
    # encoder stack / GNN layer pair: queued on the side stream they sat in front of the key-gradient reductions the main
    # stream joins on, on their own stream they fill the CUs the latency-bound dgrad chain leaves idle (cfg2: 1.443 ->
    # 1.412 ms; round 1 had measured a third stream for the dk/dv CHAIN as a loss: that chain is on the critical path)
    _side_streams: dict = {}

    def __init__(self, device):
        self.device = device
        self.jobs: List[Tuple[int, int, int, int, int, int]] = []
        self._keep: List[torch.Tensor] = []
        self.main = torch.cuda.current_stream()
        self.side = None
        self.wside = None
        if GradSink.use_side_stream:
            key = (str(device), torch.cuda.is_current_stream_capturing())
            if key not in GradSink._side_streams:
                GradSink._side_streams[key] = torch.cuda.Stream(device=device)
            self.side = GradSink._side_streams[key]
            k2 = key + ("w",)                      # a third stream for the grouped weight gradients + slab reductions
            if k2 not in GradSink._side_streams:
                GradSink._side_streams[k2] = torch.cuda.Stream(device=device)
            self.wside = GradSink._side_streams[k2]
        self._forked = False
        self._wforked = False
        self.wgrad_keys: List[Optional[str]] = []      # one entry per weight-gradient job deferred to this sink

    @staticmethod
    def side_stream(device):
        """The (process-wide) side stream used by recorded programs on ``device`` (None before the first recording)."""
        return GradSink._side_streams.get((str(device), False))

    @staticmethod
    def grad_stream(device):
        """The stream the gradient reductions of recorded programs run on: the weight-gradient stream (None before the first recording)."""
        return GradSink._side_streams.get((str(device), False, "w"))

    # Weight-gradient jobs are collected and issued as ONE grouped launch at the next flush instead of one kernel each on
    # the side stream (interleaved they cost the dgrad chain ~0.45 ms per step of interference: round 1).

    def defer_wgrad(self, desc, keep=(), key: Optional[str] = None) -> None:
        """``key``: the name of the weight the job serves; ``wgrad_keys`` lists them in the order the jobs were described
        (what a pruned backward program is counted by: train.Trainer.program_stats)."""
        self._keep.extend(keep)
        if not hasattr(self, "_wjobs"):
            self._wjobs = []
        self._wjobs.append(desc)
        self.wgrad_keys.append(key)

    def _take_wjobs(self):
        jobs = getattr(self, "_wjobs", [])
        self._wjobs = []
        # biggest jobs first: the tail of the grid is then made of the small ones
        return sorted(jobs, key=lambda g: -(g.M * g.N * g.K))

    def _flush_launch(self, rjobs) -> None:
        """ONE launch for a flush point: the pending weight-gradient jobs (finished mode: they write the gradients
        themselves) + the first wave of row-partial reductions; reductions that share a destination with an earlier one
        follow in launches of their own (they accumulate)."""
        wjobs = self._take_wjobs()
        # finished-mode jobs that target the same gradient: the later ones accumulate, each in a later launch
        waves_w: List[list] = []
        occ = {}
        for g in wjobs:
            k = occ.get(g.dst, 0) if g.dst else 0
            if g.dst:
                occ[g.dst] = k + 1
            while k >= len(waves_w):
                waves_w.append([])
            if k > 0:
                g.accumulate = 1
            waves_w[k].append(g)
        waves_r = self._reduce_waves(rjobs)
        for i in range(max(len(waves_w), len(waves_r), 0)):
            grad_flush(waves_w[i] if i < len(waves_w) else [], waves_r[i] if i < len(waves_r) else [])

    def on_side(self, fn, keep=()) -> None:
        """Run ``fn`` (kernel launches) on the side stream, ordered after everything launched so far on
        the main stream.  ``keep``: tensors the side work reads that the caller is about to drop."""
        self._keep.extend(keep)
        if self.side is None:
            fn()
            return
        ev = torch.cuda.Event()
        ev.record(self.main)
        self.side.wait_event(ev)
        if RECORDER.active:
            RECORDER.prog.append((ev.record, (self.main,)))
            RECORDER.prog.append((self.side.wait_event, (ev,)))
        with torch.cuda.stream(self.side):
            fn()
        self._forked = True

    def join(self) -> None:
        """Main stream waits for all side work issued so far."""
        if self.side is not None and self._forked:
            self.main.wait_stream(self.side)
            if RECORDER.active:
                RECORDER.prog.append((self.main.wait_stream, (self.side,)))
            self._forked = False

    def keep(self, *tensors) -> None:
        """Keep ``tensors`` (None entries are skipped) alive until release(): work queued on a side stream still reads them."""
        self._keep.extend(t for t in tensors if t is not None)

    def scratch(self, *shape) -> torch.Tensor:
        t = alloc(self.device, *shape)
        self._keep.append(t)
        return t

    def add(self, src: torch.Tensor, src_off: int, dst: torch.Tensor, nsplit: int, stride: int, count: int,
            dst_off: int = 0, accumulate: bool = False):
        if count <= 0 or nsplit <= 0:
            return
        assert dst.is_contiguous() or dst.numel() == count
        self.jobs.append((src.data_ptr() + 4 * src_off, dst.data_ptr() + 4 * dst_off, int(nsplit), int(stride),
                          int(count), 1 if accumulate else 0))

    def flush_on_side(self):
        """Launch the weight-gradient jobs described so far and reduce the partials collected so far WITHOUT joining: on the
        weight-gradient stream, behind everything the main and the side stream have issued up to here, so the main stream
        runs on.  Also used for the early gradient bucket of data-parallel training."""
        jobs, self.jobs = self.jobs, []
        if self.wside is None:               # (one stream: eagerly issued steps)
            self._flush_launch(jobs)
            return
        # own stream: ordered after everything issued so far on the main AND the side stream (the slabs of the
        # attention key gradients are produced there), never in front of the kernels the main stream joins on
        for src in ([self.main, self.side] if self._forked else [self.main]):
            ev = torch.cuda.Event()
            ev.record(src)
            self.wside.wait_event(ev)
            if RECORDER.active:
                RECORDER.prog.append((ev.record, (src,)))
                RECORDER.prog.append((self.wside.wait_event, (ev,)))
        with torch.cuda.stream(self.wside):
            self._flush_launch(jobs)
        self._wforked = True

    def flush(self):
        self.join()              # (first: deferred weight-gradient jobs may read tensors produced on the side stream)
        jobs, self.jobs = self.jobs, []
        self._flush_launch(jobs)             # (nothing in it depends on the weight-gradient stream's earlier launches)
        if self.wside is not None and self._wforked:
            self.main.wait_stream(self.wside)
            if RECORDER.active:
                RECORDER.prog.append((self.main.wait_stream, (self.wside,)))
            self._wforked = False

    @staticmethod
    def _reduce_waves(jobs):
        # jobs that share a destination go to successive launches (later ones accumulate)
        occ = {}
        waves: List[List[tuple]] = []
        for j in jobs:
            k = occ.get(j[1], 0)
            occ[j[1]] = k + 1
            if k >= len(waves):
                waves.append([])
            waves[k].append(j if k == 0 else j[:5] + (1,))
        return waves

    def _reduce(self, jobs):
        for wv in self._reduce_waves(jobs):
            arr = _reduce_job_array(wv)
            _call("dosx_reduce_partials", arr, len(wv), _stream(),
                  w=lambda wv=wv: ("reduce_partials", "reduce_partials_kernel", "hbm",
                                   sum(4.0 * (j[2] + 1 + j[5]) * j[4] for j in wv)))

    def release(self):
        self._keep = []


def edge_feat_sh1(edge_vec: torch.Tensor, r_max: float = 4.0) -> torch.Tensor:
    _chk_f32(edge_vec)
    e = edge_vec.shape[0]
    out = alloc(edge_vec.device, e, 4)
    _call("dosx_edge_feat_sh1", edge_vec.data_ptr(), out.data_ptr(), e, float(r_max), _stream(),
          w=lambda: ("edge_feat_sh1", "edge_feat_kernel", "hbm", 28.0 * e))
    return out


def edge_embed_sh1(edge_vec: torch.Tensor, w0: torch.Tensor, b0: torch.Tensor, r_max: float = 4.0):
    """(edge_attr [E,4], z [E,H]) = SH(l<=1)*cutoff features and the first (K = 4) Linear of the edge encoder on them."""
    _chk_f32(edge_vec, w0, b0)
    e, H = edge_vec.shape[0], w0.shape[0]
    assert w0.shape[1] == 4 and w0.is_contiguous()
    attr, z = alloc(edge_vec.device, e, 4), alloc(edge_vec.device, e, H)
    _call("dosx_edge_embed_sh1", edge_vec.data_ptr(), w0.data_ptr(), b0.data_ptr(), attr.data_ptr(), z.data_ptr(), e, H,
          float(r_max), _stream(), w=lambda: ("edge_embed_sh1", "edge_embed_kernel", "hbm", 4.0 * e * (3 + 4 + H)))
    return attr, z


def edge_enc_supported(H: int) -> bool:
    return bool(_lib.load().dosx_edge_enc_supported(int(H)))


def edge_enc_fwd(edge_vec: torch.Tensor, w0, b0, alpha, w2, b2, r_max: float = 4.0):
    """(attr [E,4], z [E,H], out [E,H]): SH * cutoff features, the K = 4 Linear, PReLU, the second Linear of the phonon edge
    encoder in one launch (include/dosx.h: DosxEdgeEnc)."""
    _chk_f32(edge_vec, w0, b0, w2, b2)
    e, H = int(edge_vec.shape[0]), int(w2.shape[0])
    assert w0.shape == (H, 4) and w0.is_contiguous() and w2.is_contiguous() and edge_vec.is_contiguous()
    dev = edge_vec.device
    attr, z, out = alloc(dev, e, 4), alloc(dev, e, H), alloc(dev, e, H)
    d = _lib.EdgeEnc()
    d.E, d.H = e, H
    d.vec, d.inv_rmax = edge_vec.data_ptr(), 1.0 / float(r_max)
    d.w0, d.b0, d.alpha, d.w2, d.b2 = w0.data_ptr(), b0.data_ptr(), alpha.data_ptr(), w2.data_ptr(), b2.data_ptr()
    d.attr, d.z, d.out, d.ldo = attr.data_ptr(), z.data_ptr(), out.data_ptr(), H
    _call("dosx_edge_enc_fwd", C.byref(d), _stream(),
          w=lambda: (f"edge_enc_fwd[H{H}]", f"edge_enc_fwd_kernel<{H}>", "mfma", 2.0 * _real(e) * H * (H + 4)))
    return attr, z, out


def segment_reduce(msg, rowptr, scale, agg, e_in, e_out, N, E, H):
    # algorithmic bytes: messages + CSR row pointers + aggregated output (+ the fused edge residual e_out = e_in + msg:
    # one more read and one write of [E,H])
    _call("dosx_segment_reduce", _p(msg), _p(rowptr), _p(scale), _p(agg), _p(e_in), _p(e_out), N, E, H, _stream(),
          w=lambda: (f"scatter_add_fwd[H{H}{',res' if e_out is not None else ''}]", "segment_reduce_kernel", "hbm",
                     4.0 * (_real(E) * H + (_real(N) + 1) + _real(N) * H + (2 * _real(E) * H if e_out is not None else 0))))


def segment_reduce_perm(msg, rowptr, perm, agg, N, E, H):
    """agg[n] = sum of msg[perm[j]] over j in [rowptr[n], rowptr[n+1])   (include/dosx.h: dosx_segment_reduce_perm)"""
    _call("dosx_segment_reduce_perm", _p(msg), _p(rowptr), _p(perm), _p(agg), N, E, H, _stream(),
          w=lambda: (f"segment_sum_perm[H{H}]", "segment_reduce_perm_kernel", "hbm", 4.0 * (_real(E) * H + _real(E) + (_real(N) + 1) + _real(N) * H)))


def edge_grad_combine(de_new, dagg, ld_dagg, dst, scale, dmsg, E, H):
    """de_new: None or a 2-D tensor / view with unit inner stride ([E,H] or the e-block of an [E,3H] gradient)."""
    ld_de = int(de_new.stride(0)) if de_new is not None else 0
    _call("dosx_edge_grad_combine", _p(de_new), ld_de, dagg, ld_dagg, _p(dst), _p(scale), _p(dmsg), E, H, _stream(),
          w=lambda: (f"edge_grad_combine[H{H}]", "edge_grad_combine_kernel", "hbm",
                     4.0 * (_real(E) * H * (3 if de_new is not None else 2) + _real(E))))


def gather_bwd(dcat, dnode_ptr, ld_dnode, dx_res, rowptr_dst, rowptr_src, perm_src, de_new, dx, de_out, N, E, H):
    # algorithmic bytes: dcat [E,3H] read once (+ de_new read, de_out written), 3 index arrays, 3 node-row streams
    _call("dosx_gather_bwd", _p(dcat), dnode_ptr, ld_dnode, _p(dx_res), _p(rowptr_dst), _p(rowptr_src),
          _p(perm_src), _p(de_new), _p(dx), _p(de_out), N, E, H, _stream(),
          w=lambda: (f"gather_bwd[H{H}]", "gather_bwd_kernel", "hbm",
                     4.0 * (_real(E) * H * ((3 if de_out is not None else 2) + (1 if de_new is not None else 0)
                                            + (1 if de_out is not None else 0)) + _real(E) + 2 * (_real(N) + 1) + 3 * _real(N) * H)))


def graph_pool(x, graph_ptr, out_ptr, ld_out, B, H):
    _call("dosx_graph_pool", _p(x), _p(graph_ptr), out_ptr, ld_out, B, H, _stream(),
          w=lambda: ("graph_pool", "graph_pool_kernel", "hbm", 4.0 * (x.shape[0] * H + B * H)))


def graph_pool_bwd(dpool_ptr, ld, node_graph, dx, N, H, accumulate, num_graphs=0):
    _call("dosx_graph_pool_bwd", dpool_ptr, ld, _p(node_graph), _p(dx), N, H, int(accumulate), int(num_graphs), _stream(),
          w=lambda: ("graph_pool_bwd", "graph_pool_bwd_kernel", "hbm", 4.0 * N * H * (3 if accumulate else 2)))


def dense_normalize(x, dense_row, kvhat, rstd_nodes, N, H, dense_rows):
    _call("dosx_dense_normalize", _p(x), _p(dense_row), _p(kvhat), _p(rstd_nodes), N, H, dense_rows, _stream(),
          w=lambda: ("dense_normalize", "dense_normalize_kernel", "hbm", 4.0 * (N * H + dense_rows * H + N * H)))


def dense_normalize_slots(x, graph_ptr, kvhat, rstd_nodes, B, n_max, H):
    _call("dosx_dense_normalize_slots", _p(x), _p(graph_ptr), _p(kvhat), _p(rstd_nodes), B, n_max, H, _stream(),
          w=lambda: ("dense_normalize", "dense_normalize_slots_kernel", "hbm", 4.0 * H * (x.shape[0] + n_max * B + 1)))


def dense_normalize_bwd(dkvhat, kvhat, rstd_nodes, dense_row, dx, N, H, accumulate, ghost_row=-1):
    _call("dosx_dense_normalize_bwd", _p(dkvhat), _p(kvhat), _p(rstd_nodes), _p(dense_row), _p(dx), N, H,
          int(accumulate), int(ghost_row), _stream(),
          w=lambda: ("dense_normalize_bwd", "dense_normalize_bwd_kernel", "hbm", 4.0 * N * H * 3))


def dense_normalize_pool_bwd(dkvhat, kvhat, rstd_nodes, dense_row, dpool_ptr, ld_dpool, node_graph, num_graphs, dx, N, H,
                             accumulate, ghost_row=-1):
    """dense_normalize_bwd + graph_pool_bwd in one launch (include/dosx.h: dosx_dense_normalize_pool_bwd)."""
    _call("dosx_dense_normalize_pool_bwd", _p(dkvhat), _p(kvhat), _p(rstd_nodes), _p(dense_row), dpool_ptr, int(ld_dpool),
          _p(node_graph), int(num_graphs), _p(dx), N, H, int(accumulate), int(ghost_row), _stream(),
          w=lambda: ("dense_normalize_pool_bwd", "dense_normalize_bwd_kernel", "hbm", 4.0 * N * H * 4))


def dense_slots(x, graph_ptr, dense, B, n_max, H):
    """dense [n_max*B, H] = to_dense_batch(x) (zero rows for padded slots), no normalisation (include/dosx.h)."""
    _call("dosx_dense_slots", _p(x), _p(graph_ptr), _p(dense), B, n_max, H, _stream(),
          w=lambda: ("dense_slots", "dense_slots_kernel", "hbm", 4.0 * H * (x.shape[0] + n_max * B)))


def dense_slots_bwd(ddense, dense_row, dx, N, H, accumulate, ghost_row=-1):
    _call("dosx_dense_slots_bwd", _p(ddense), _p(dense_row), _p(dx), N, H, int(accumulate), int(ghost_row), _stream(),
          w=lambda: ("dense_slots_bwd", "dense_slots_bwd_kernel", "hbm", 4.0 * N * H * (3 if accumulate else 2)))


def ln_prelu_bwd_partial_rows(M: int) -> int:
    return (int(M) + 31) // 32


def ln_prelu_bwd(dy, xhat, rstd, gamma, beta, alpha, dz, partials, M, W):
    """dz = LayerNorm-PReLU backward of dy on rows of W <= 1024 floats + [dgamma | dbeta | pad | dalpha] partial rows
    (include/dosx.h: dosx_ln_prelu_bwd)."""
    _call("dosx_ln_prelu_bwd", _p(dy), _p(xhat), _p(rstd), _p(gamma), _p(beta), _p(alpha), _p(dz), _p(partials), M, W, _stream(),
          w=lambda: ("ln_prelu_bwd", "ln_bwd_wide_kernel", "hbm", 12.0 * M * W))


def ln_prelu_bwd_gather(dy, idx, scale, xhat, rstd, gamma, beta, alpha, dz, partials, M, W):
    """The same with dy rows gathered: row r reads dy[idx[r]] * scale[idx[r]] (include/dosx.h: dosx_ln_prelu_bwd_gather)."""
    _call("dosx_ln_prelu_bwd_gather", _p(dy), _p(idx), _p(scale), _p(xhat), _p(rstd), _p(gamma), _p(beta), _p(alpha), _p(dz),
          _p(partials), M, W, _stream(), w=lambda: ("ln_prelu_bwd_gather", "ln_bwd_wide_kernel", "hbm", 8.0 * _real(M) * W))


def act_segment_sum(xhat, rowptr, scale, gamma, beta, alpha, bias, S, R, N, E, W, Hout):
    """S[n] = scale[n] * sum over the segment of PReLU(xhat*gamma+beta), R[n] = c_n * bias (include/dosx.h: dosx_act_segment_sum)."""
    _call("dosx_act_segment_sum", _p(xhat), _p(rowptr), _p(scale), _p(gamma), _p(beta), _p(alpha), _p(bias), _p(S), _p(R), N, W, Hout,
          _stream(), w=lambda: (f"act_segment_sum[W{W}]", "act_segment_sum_kernel", "hbm", 4.0 * (_real(E) * W + _real(N) * (W + Hout))))


def seg_count_scale(src, ld_src, rowptr, mean, out, N, H):
    """out[n] = c_n * src[n], c_n = segment length (mean False) or [segment not empty]; src: tensor or raw pointer with row stride ld_src."""
    _call("dosx_seg_count_scale", src if isinstance(src, int) else _p(src), int(ld_src), _p(rowptr), int(bool(mean)), _p(out), N, H,
          _stream(), w=lambda: ("seg_count_scale", "seg_count_scale_kernel", "hbm", 8.0 * _real(N) * H))


def gather_add_rownorm(z, p, q, src, dst, xhat, rstd, E, W):
    """xhat = rownorm(z + p[src] + q[dst]) (include/dosx.h: dosx_gather_add_rownorm); p / q: 2-D views with unit inner stride."""
    _call("dosx_gather_add_rownorm", _p(z), _p(p), int(p.stride(0)), _p(q), int(q.stride(0)), _p(src), _p(dst), _p(xhat), _p(rstd),
          E, W, _stream(), w=lambda: ("gather_add_rownorm", "gather_add_rownorm_kernel", "hbm", 4.0 * _real(E) * W * 4))


def rownorm(x, xhat, rstd, M, H):
    _call("dosx_rownorm", _p(x), _p(xhat), _p(rstd), M, H, _stream(),
          w=lambda: ("rownorm", "rownorm_kernel", "hbm", 8.0 * M * H))


def rownorm_bwd(dxhat, xhat, rstd, dx, M, H, accumulate):
    _call("dosx_rownorm_bwd", _p(dxhat), _p(xhat), _p(rstd), _p(dx), M, H, int(accumulate), _stream(),
          w=lambda: ("rownorm_bwd", "rownorm_bwd_kernel", "hbm", 12.0 * M * H))


def rownorm_bwd_act(dxhat, xhat, rstd, dx_in, y, slope, out, M, H):
    """out = (dx_in + rownorm_bwd(dxhat, xhat, rstd)) * (y > 0 ? 1 : slope)   (include/dosx.h: dosx_rownorm_bwd_act)."""
    _call("dosx_rownorm_bwd_act", _p(dxhat), _p(xhat), _p(rstd), _p(dx_in), _p(y), float(slope), _p(out), M, H, _stream(),
          w=lambda: ("rownorm_bwd_act", "rownorm_bwd_act_kernel", "hbm", 20.0 * M * H))


def enc_cs_supported(M: int, Fa: int, H: int) -> bool:
    """Whether the node encoder + first node products run as ONE column-split launch (include/dosx.h: DosxEncCs)."""
    return bool(M > 0 and _lib.load().dosx_enc_cs_supported(int(Fa), int(H))
                and ((int(M) + 15) // 16) * (int(H) // 16) <= MLP_LN_CS_MAX_WGS)


def enc_cs_fwd(M: int, x, w0, b0, alpha, w2, b2, z, out, w3, pq) -> None:
    """z = x w0^T + b0; out = prelu(z) w2^T + b2; pq = out [w3[:, :H] | w3[:, H:2H]]^T - one launch (DosxEncCs)."""
    d = _lib.EncCs()
    H, Fa = int(w2.shape[0]), int(x.shape[1])
    assert x.stride(1) == 1 and w0.stride(1) == 1 and w2.is_contiguous() and z.is_contiguous() and out.stride(1) == 1 and w3.stride(1) == 1
    d.M, d.Fa, d.H = int(M), Fa, H
    d.x, d.ldx = x.data_ptr(), int(x.stride(0))
    d.w0, d.ldw0, d.b0, d.alpha = w0.data_ptr(), int(w0.stride(0)), b0.data_ptr(), alpha.data_ptr()
    d.w2, d.b2 = w2.data_ptr(), b2.data_ptr()
    d.z, d.out, d.ldo = z.data_ptr(), out.data_ptr(), int(out.stride(0))
    d.w3, d.ldw3, d.n3, d.nb3 = w3.data_ptr(), int(w3.stride(0)), int(w3.shape[0]), 2
    d.pq, d.ldpq = pq.data_ptr(), int(pq.stride(0))
    d.cs_cnt = COUNTERS.take(out.device, _lib.load().dosx_mlp_ln_cs_tiles(int(M)))
    _call("dosx_enc_cs_fwd", C.byref(d), _stream(),
          w=lambda: (f"enc_cs_fwd[Fa{Fa},H{H}]", "enc_cs_fwd_kernel", "mfma", 2.0 * _real(M) * H * (Fa + H + 4 * H)))


def heads_bwd_supported(H: int) -> bool:
    return bool(_lib.load().dosx_heads_bwd_supported(int(H)))


def heads_bwd(S: int, B: int, H: int, dkvs, kvs, rstd, ddosin, dosin, slope: float, dpre, wg, ws, de1) -> None:
    """dpre = (ddosin + rownorm_bwd(dkvs, kvs, rstd)) * leaky'(dosin) [S*2B, H]; de1 = dpre[global rows] wg[:, :H] + dpre[system rows]
    ws[:, :H] [S*B, H] - one launch (include/dosx.h: DosxHeadsBwd).  wg / ws: the heads' weights (or views of their first columns)."""
    d = _lib.HeadsBwd()
    d.S, d.B, d.H = int(S), int(B), int(H)
    for t in (dkvs, kvs, ddosin, dosin, dpre):
        assert t.is_contiguous() and t.shape == (S * 2 * B, H)
    assert wg.stride(1) == 1 and ws.stride(1) == 1 and de1.stride(1) == 1
    d.dkvs, d.kvs, d.rstd, d.ddosin, d.dosin = dkvs.data_ptr(), kvs.data_ptr(), rstd.data_ptr(), ddosin.data_ptr(), dosin.data_ptr()
    d.slope = float(slope)
    d.dpre = dpre.data_ptr()
    d.wg, d.ldwg, d.ws, d.ldws = wg.data_ptr(), int(wg.stride(0)), ws.data_ptr(), int(ws.stride(0))
    d.de1, d.ldde1 = de1.data_ptr(), int(de1.stride(0))
    _call("dosx_heads_bwd", C.byref(d), _stream(),
          w=lambda: (f"heads_bwd[H{H}]", f"heads_bwd_kernel<{H}>", "mfma", 2.0 * S * B * H * 2 * H))


def _pair_head_desc(who: str, e1, c, w2, slope: float):
    """The operands both pair-head launches read: e1 [S,H], c [B,H], w2 [H] (or [1,H], nn.Linear(H, 1).weight)."""
    _chk_f32(e1, c, w2)
    if e1.dim() != 2 or c.dim() != 2 or e1.shape[1] != c.shape[1] or w2.numel() != e1.shape[1]:
        raise ValueError(f"{who}: e1 [S,H], c [B,H], w2 [H], got {tuple(e1.shape)}, {tuple(c.shape)}, {tuple(w2.shape)}")
    if not (e1.is_contiguous() and c.is_contiguous() and w2.is_contiguous()):
        raise ValueError(f"{who}: e1, c and w2 must be contiguous")
    d = _lib.PairHead()
    d.S, d.B, d.H, d.slope = int(e1.shape[0]), int(c.shape[0]), int(e1.shape[1]), float(slope)
    d.e1, d.c, d.w2 = e1.data_ptr(), c.data_ptr(), w2.data_ptr()
    return d


def pair_head_partial_rows(S: int, B: int) -> int:
    return int(_lib.load().dosx_pair_head_partial_rows(int(S), int(B)))


def pair_head_fwd(e1, c, w2, b2, dos, slope: float = 0.01) -> None:
    """dos[b, s] = b2 + sum_h w2[h] * leaky(e1[s, h] + c[b, h]) in one launch (include/dosx.h: DosxPairHead); dos: [B,S]."""
    d = _pair_head_desc("pair_head_fwd", e1, c, w2, slope)
    _chk_f32(b2, dos)
    if tuple(dos.shape) != (d.B, d.S) or not dos.is_contiguous() or b2.numel() != 1:
        raise ValueError(f"pair_head_fwd: dos must be a contiguous [B,S] = [{d.B},{d.S}] and b2 one element, got "
                         f"{tuple(dos.shape)}, {tuple(b2.shape)}")
    d.b2, d.dos = b2.data_ptr(), dos.data_ptr()
    S, B, H = d.S, d.B, d.H
    _call("dosx_pair_head_fwd", C.byref(d), _stream(),
          w=lambda: (f"pair_head_fwd[H{H}]", "pair_head_fwd_kernel", "hbm", 4.0 * (S * H + B * H + S * B)))


def pair_head_bwd(ddos, e1, c, w2, de1, dc, partials, slope: float = 0.01) -> None:
    """The backward of pair_head_fwd from ddos [B,S] in one launch: de1 [S,H], dc [B,H] and ``partials``
    [pair_head_partial_rows(S, B), H + 1] whose column sums are dw2 (H) and db2 (GradSink.add)."""
    d = _pair_head_desc("pair_head_bwd", e1, c, w2, slope)
    _chk_f32(ddos, de1, dc, partials)
    rows = pair_head_partial_rows(d.S, d.B)
    ok = (tuple(ddos.shape) == (d.B, d.S) and de1.shape == e1.shape and dc.shape == c.shape
          and tuple(partials.shape) == (rows, d.H + 1))
    if not ok or not all(t.is_contiguous() for t in (ddos, de1, dc, partials)):
        raise ValueError(f"pair_head_bwd: contiguous ddos [B,S], de1 [S,H], dc [B,H], partials [{rows},H+1] wanted, got "
                         f"{tuple(ddos.shape)}, {tuple(de1.shape)}, {tuple(dc.shape)}, {tuple(partials.shape)}")
    d.ddos, d.de1, d.dc, d.partials = ddos.data_ptr(), de1.data_ptr(), dc.data_ptr(), partials.data_ptr()
    S, B, H = d.S, d.B, d.H
    _call("dosx_pair_head_bwd", C.byref(d), _stream(),
          w=lambda: (f"pair_head_bwd[H{H}]", "pair_head_bwd_kernel", "hbm", 4.0 * (3 * S * H + 2 * B * H + S * B)))


def gemm_bf16x3_supported(M: int, N: int, K: int) -> bool:
    return bool(_lib.load().dosx_gemm_bf16x3_supported(int(M), int(N), int(K)))


def gemm_bf16x3(a, w, out, bias=None, w_layout: int = 0, act: int = 0, res=None, mask=None) -> None:
    """out[M,N] = epi(a[M,K] . op(w) + bias) with the split-bf16 kernel (include/dosx.h: dosx_gemm_bf16x3).  w: [N,K] (w_layout 0) or
    [K,N] (1); fp32, unit inner strides.  epi: relu (act = ACT_RELU), + res, zero where mask <= 0."""
    M, K = a.shape
    N = out.shape[1]
    assert a.stride(1) == 1 and w.stride(1) == 1 and out.stride(1) == 1 and out.shape[0] == M
    assert tuple(w.shape) == ((N, K) if w_layout == 0 else (K, N)) and act in (0, ACT_RELU)
    for t in (res, mask):
        assert t is None or (t.stride(1) == 1 and tuple(t.shape) == (M, N))
    _call("dosx_gemm_bf16x3", _p(a), int(a.stride(0)), _p(w), int(w.stride(0)), int(w_layout), _p(bias), _p(out), int(out.stride(0)),
          int(M), int(N), int(K), 1 if act == ACT_RELU else 0, _p(res), int(res.stride(0)) if res is not None else 0,
          _p(mask), int(mask.stride(0)) if mask is not None else 0, _stream(),
          w=lambda: (f"gemm_bf16x3[N{N},K{K},wl{w_layout}]", "gemm_bf16x3_kernel", "mfma", 2.0 * M * N * K))


def mask_residual(a, mask, res, out, stats, M, H):
    """out = (res or 0) + a o (mask or 1), optionally with the LayerNorm statistics [M,2] of out (include/dosx.h)."""
    _call("dosx_mask_residual", _p(a), int(a.stride(0)), _p(mask), _p(res), int(res.stride(0)) if res is not None else 0,
          _p(out), int(out.stride(0)), _p(stats), M, H, _stream(),
          w=lambda: ("mask_residual", "mask_residual_kernel", "hbm", 4.0 * M * H * (2 + (mask is not None) + (res is not None))))


def layernorm(x, gamma, beta, y, xhat, rstd, M, H):
    _call("dosx_layernorm", _p(x), _p(gamma), _p(beta), _p(y), _p(xhat), _p(rstd), M, H, _stream(),
          w=lambda: ("layernorm", "ln_fwd_kernel", "hbm", 12.0 * M * H))


def layernorm_bwd(dy, xhat, rstd, gamma, dx, partials, M, H):
    _call("dosx_layernorm_bwd", _p(dy), _p(xhat), _p(rstd), _p(gamma), _p(dx), _p(partials), M, H, _stream(),
          w=lambda: ("layernorm_bwd", "ln_bwd_kernel", "hbm", 12.0 * M * H))


def _attn_shape(a: Attn) -> str:
    # (key-count CLASS, not Nk: the batches of a run differ in n_max and belong to one site per kernel path)
    return f"Sq{a.Sq},Bq{a.Bq},Nk<={16 if a.Nk <= 16 else (64 if a.Nk <= 64 else 320)},Bk{a.Bk},H{a.H}"


def attention_fwd(a: Attn):
    # algorithmic flops: Q.K^T and P.V, 2*Sq*Nk*H each per query batch entry
    _call("dosx_attention_fwd", C.byref(a), _stream(),
          w=lambda: (f"attention_fwd[{_attn_shape(a)}]", "attn_fwd", "mfma", 4.0 * a.Bq * a.Sq * a.Nk * a.H))


def attention_bwd(a: Attn):
    # dP = dO.K^T and dQ = dS.K (dq half), dK = dS^T.Q and dV = P^T.dO (dkv half): 4*Bq*Sq*Nk*H flops each half
    halves = (0 if a.flags & ATTN_BWD_DKV_HALF else 1) + (0 if a.flags & ATTN_BWD_DQ_HALF else 1)
    name = "attention_bwd" + ("_dkv" if (a.flags & ATTN_BWD_DKV_HALF) else ("_dq" if (a.flags & ATTN_BWD_DQ_HALF) else ""))
    _call("dosx_attention_bwd", C.byref(a), _stream(),
          w=lambda: (f"{name}[{_attn_shape(a)}]", "attn_bwd", "mfma", 4.0 * halves * a.Bq * a.Sq * a.Nk * a.H))


def attn_pv(A, mask, V, out, Sq, Bq, Nk, Bk, H):
    """out[(s,bq)] = sum_j (A o mask)[bq,s,j] V[(j, bq % Bk)]   (K != V attention, include/dosx.h)"""
    _call("dosx_attn_pv", _p(A), _p(mask), _p(V), _p(out), Sq, Bq, Nk, Bk, H, _stream())


def attn_tv(A, mask, X, out, Sq, Bq, Nk, Bk, H, accumulate=False):
    """out[(j,bk)] (+)= sum_bq sum_s (A o mask)[bq,s,j] X[(s,bq)]"""
    _call("dosx_attn_tv", _p(A), _p(mask), _p(X), _p(out), Sq, Bq, Nk, Bk, H, int(accumulate), _stream())


def attn_dp(X, V, dP, Sq, Bq, Nk, Bk, H):
    _call("dosx_attn_dp", _p(X), _p(V), _p(dP), Sq, Bq, Nk, Bk, H, _stream())


def softmax_bwd(P, mask, dPd, dS, rows, Nk, scale):
    _call("dosx_softmax_bwd", _p(P), _p(mask), _p(dPd), _p(dS), int(rows), int(Nk), float(scale), _stream())


# widest row of dosx_attention_* (any number of keys: <= 320 the MFMA kernels, more the general kernels of
# csrc/attention_general.hip); wider rows go through the K != V building blocks (any Nk, any H % 4 == 0)
ATTN_MAX_H = 256


def attention_weights(q, k, probs, Sq, Bq, Nk, Bk, H):
    """probs[bq, s, :] = softmax_fp32(H**-0.5 * q[(s,bq)] . k[(j, bq % Bk)]) for rows that are ALREADY normalised / projected
    (multihead_attention.py:68-70): the MFMA kernel where it fits, ``attn_dp`` + ``softmax_fwd`` for any shape."""
    if H <= ATTN_MAX_H:
        dev = q.device
        ones, zeros = torch.ones(H, device=dev), torch.zeros(H, device=dev)
        scratch = torch.empty(Sq * Bq, H, device=dev)
        a = _lib.Attn()
        a.Sq, a.Bq, a.Nk, a.Bk, a.H = Sq, Bq, Nk, Bk, H
        a.q_stride_s, a.q_stride_b, a.flags = Bq, 1, ATTN_RAW_Q | ATTN_NO_RESIDUAL
        a.x, a.kvhat, a.gamma0, a.beta0 = q.data_ptr(), k.data_ptr(), ones.data_ptr(), zeros.data_ptr()
        a.out, a.probs = scratch.data_ptr(), probs.data_ptr()
        attention_fwd(a)                                               # (its P.K output is discarded)
        return (ones, zeros, scratch)                                  # keep-alive for recorded programs
    scores = torch.empty(Bq, Sq, Nk, device=q.device)
    attn_dp(q, k, scores, Sq, Bq, Nk, Bk, H)
    softmax_fwd(scores, probs, Bq * Sq, Nk, H ** -0.5)
    return (scores,)


def softmax_fwd(S, P, rows, Nk, scale):
    """P = softmax_fp32(scale * S) row by row (any Nk); with ``attn_dp(Q, K, S)`` the general attention weights."""
    _call("dosx_softmax_fwd", _p(S), _p(P), int(rows), int(Nk), float(scale), _stream())


def ln_rowdot(x, gamma, beta, w, b, xhat, rstd, dos, S, Bq, H):
    _call("dosx_ln_rowdot", _p(x), _p(gamma), _p(beta), _p(w), _p(b), _p(xhat), _p(rstd), _p(dos), S, Bq, H, _stream(),
          w=lambda: ("ln_rowdot", "ln_rowdot_kernel", "hbm", 8.0 * S * Bq * H))


def ln_rowdot_bwd(ddos, xhat, rstd, gamma, beta, w, dx, partials, S, Bq, H):
    _call("dosx_ln_rowdot_bwd", _p(ddos), _p(xhat), _p(rstd), _p(gamma), _p(beta), _p(w), _p(dx), _p(partials), S, Bq,
          H, _stream(), w=lambda: ("ln_rowdot_bwd", "ln_bwd_kernel", "hbm", 8.0 * S * Bq * H))


def rowdot(x, w, b, dos, S, Bq, H):
    _call("dosx_rowdot", _p(x), _p(w), _p(b), _p(dos), S, Bq, H, _stream())


def rowdot_bwd(ddos, x, w, dx, partials, S, Bq, H):
    _call("dosx_rowdot_bwd", _p(ddos), _p(x), _p(w), _p(dx), _p(partials), S, Bq, H, _stream())


def sse2(pg, ps, y, sse, count):
    _call("dosx_sse2", _p(pg), _p(ps), _p(y), _p(sse), count, _stream())


def loss_phonon_bwd(pg, ps, y, sse, beta, count_global, dpg, dps, loss, count):
    _call("dosx_loss_phonon_bwd", _p(pg), _p(ps), _p(y), _p(sse), float(beta), float(count_global), _p(dpg), _p(dps),
                                        _p(loss), count, _stream())


def loss_phonon(pg, ps, y, sse, beta, dpg, dps, loss, count):
    """single-process phonon loss + gradient in one launch (include/dosx.h: dosx_loss_phonon)"""
    _call("dosx_loss_phonon", _p(pg), _p(ps), _p(y), _p(sse), float(beta), _p(dpg), _p(dps), _p(loss), count, _stream())


def loss_edos(pg, ps, y_ft, beta, B, S, B_global, dpg, dps, loss_partial):
    _call("dosx_loss_edos", _p(pg), _p(ps), _p(y_ft), float(beta), B, S, B_global, _p(dpg), _p(dps), _p(loss_partial),
                                  _stream())


def eval_metrics(pred: torch.Tensor, y: torch.Tensor, metrics: torch.Tensor, clamp0: bool = False,
                 pred_out: Optional[torch.Tensor] = None, y_out: Optional[torch.Tensor] = None) -> None:
    """metrics[b] = (rmse, mse, mae, r2) of row b of pred against row b of y, in float64 - the reference's metrics of a batch of
    one crystal (include/dosx.h: dosx_eval_metrics / dosx_eval_metrics_f64).  pred, y: [B,S], both float32 or both float64;
    metrics: [B,4] float64; ``clamp0``: clamp both at 0 first (eDOS); pred_out / y_out ([B,S], the inputs' dtype) receive the
    clamped values.  The outputs may be row slices of larger tables."""
    dt = pred.dtype
    if dt not in (torch.float32, torch.float64):
        raise TypeError(f"eval_metrics: float32 or float64 predictions, got {dt}")
    ins = {"pred": pred, "y": y, "pred_out": pred_out, "y_out": y_out}
    for k, t in ins.items():
        if t is not None and (t.dtype != dt or not t.is_cuda):
            raise TypeError(f"eval_metrics: {k} must be a {dt} CUDA tensor like pred, got {t.dtype} on {t.device}")
    if metrics.dtype != torch.float64 or not metrics.is_cuda:
        raise TypeError(f"eval_metrics: metrics must be a float64 CUDA tensor, got {metrics.dtype} on {metrics.device}")
    if pred.dim() != 2 or pred.shape[1] < 1 or any(t is not None and t.shape != pred.shape for t in ins.values()) \
            or tuple(metrics.shape) != (pred.shape[0], 4):
        raise ValueError("eval_metrics: " + ", ".join(f"{k} {tuple(t.shape)}" for k, t in ins.items() if t is not None)
                         + f", metrics {tuple(metrics.shape)}: want [B,S] (S >= 1) everywhere and metrics [B,4]")
    for k, t in list(ins.items()) + [("metrics", metrics)]:
        if t is not None and not t.is_contiguous():
            raise ValueError(f"eval_metrics: {k} must be contiguous (rows of a table are), got strides {t.stride()}")
    B, S = int(pred.shape[0]), int(pred.shape[1])
    _call("dosx_eval_metrics" if dt == torch.float32 else "dosx_eval_metrics_f64", pred.data_ptr(), y.data_ptr(), B, S,
          int(bool(clamp0)), metrics.data_ptr(), _p(pred_out), _p(y_out), _stream(),
          w=lambda: ("eval_metrics", "eval_metrics_kernel", "hbm", 3.0 * pred.element_size() * B * S))


def eval_functionals(pred: torch.Tensor, y: torch.Tensor, table: torch.Tensor, out: torch.Tensor,
                     scale: Optional[torch.Tensor] = None) -> None:
    """out[b,0,k] = F_k(pred_b) scale_b and out[b,1,k] = F_k(y_b) scale_b, ``F_k(p) = sum_s table[k,s] p_s``, in float64
    (include/dosx.h: dosx_eval_functionals / dosx_eval_functionals_f64).  pred, y: [B,S] and table: [K,S], all float32 or all
    float64; out: [B,2,K] float64; scale: None or [B] float64 (e.g. the eDOS ``y_max``).  Any S, K >= 1; B = 0 launches nothing."""
    dt = pred.dtype
    if dt not in (torch.float32, torch.float64):
        raise TypeError(f"eval_functionals: float32 or float64 predictions, got {dt}")
    for k, t in (("pred", pred), ("y", y), ("table", table)):
        if t.dtype != dt or not t.is_cuda:
            raise TypeError(f"eval_functionals: {k} must be a {dt} CUDA tensor like pred, got {t.dtype} on {t.device}")
    for k, t in (("out", out), ("scale", scale)):
        if t is not None and (t.dtype != torch.float64 or not t.is_cuda):
            raise TypeError(f"eval_functionals: {k} must be a float64 CUDA tensor, got {t.dtype} on {t.device}")
    if pred.dim() != 2 or pred.shape[1] < 1 or y.shape != pred.shape or table.dim() != 2 or table.shape[0] < 1 or \
            table.shape[1] != pred.shape[1] or tuple(out.shape) != (pred.shape[0], 2, table.shape[0]) or \
            (scale is not None and tuple(scale.shape) != (pred.shape[0],)):
        raise ValueError(f"eval_functionals: pred {tuple(pred.shape)}, y {tuple(y.shape)}, table {tuple(table.shape)}, out "
                         f"{tuple(out.shape)}" + ("" if scale is None else f", scale {tuple(scale.shape)}")
                         + ": want [B,S], [B,S], [K,S] (S, K >= 1), [B,2,K] and [B]")
    for k, t in (("pred", pred), ("y", y), ("table", table), ("out", out), ("scale", scale)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"eval_functionals: {k} must be contiguous, got strides {t.stride()}")
    B, S, K = int(pred.shape[0]), int(pred.shape[1]), int(table.shape[0])
    _call("dosx_eval_functionals" if dt == torch.float32 else "dosx_eval_functionals_f64", pred.data_ptr(), y.data_ptr(), B, S,
          _p(scale), table.data_ptr(), K, out.data_ptr(), _stream(),
          w=lambda: ("eval_functionals", "eval_functionals_kernel", "hbm", pred.element_size() * (2.0 * B * S + K * S) + 16.0 * B * K))


def sum_to(src, n, dst):
    _call("dosx_sum", _p(src), int(n), _p(dst), _stream())


# per-crystal losses (csrc/loss_rows.hip; include/dosx.h: dosx_loss_rows / dosx_loss_rows_f64): the trainers' names -> enumerators
LOSS_KINDS = {"crystal_rmse": _abi.DOSX_LOSS_RMSE, "mse": _abi.DOSX_LOSS_MSE, "mae": _abi.DOSX_LOSS_MAE, "huber": _abi.DOSX_LOSS_HUBER}
# linear functionals next to them (csrc/loss_functional.hip; include/dosx.h: dosx_loss_rows_fn / dosx_loss_rows_fn_f64)
FUNCTIONAL_KINDS = {"sq": _abi.DOSX_FN_SQ, "abs": _abi.DOSX_FN_ABS}
FUNCTIONAL_MAX = 512               # K and S of a table in the loss


def _loss_rows(who: str, dt: torch.dtype, pg, ps, y, kind, clamp_target, beta, delta, dpg, dps, per_crystal, loss, B_global,
               weights=None, weight_index=None, bin_weights=None, functionals=None, functional_kind="sq",
               functional_weight=1.0, functional_denominator=None, functional_norm_rows=0, functional_floor=None) -> None:
    if isinstance(kind, str):
        if kind not in LOSS_KINDS:
            raise ValueError(f"{who}: kind {kind!r} is not one of {sorted(LOSS_KINDS)}")
        kind = LOSS_KINDS[kind]
    if int(kind) == _abi.DOSX_LOSS_HUBER and (delta is None or not 0.0 < float(delta) < float("inf")):
        raise ValueError(f"{who}: the Huber kind needs a finite delta > 0, got {delta}")
    ts = {"pg": pg, "ps": ps, "y": y, "dpg": dpg, "dps": dps, "per_crystal": per_crystal, "loss": loss}
    for k, t in ts.items():
        if k in ("pg", "y", "dpg", "loss") and t is None:
            raise TypeError(f"{who}: {k} is required (only ps with dps, and per_crystal, may be None)")
        if t is not None and (t.dtype != dt or not t.is_cuda):
            raise TypeError(f"{who}: {k} must be a {dt} CUDA tensor, got {t.dtype} on {t.device}")
    if (ps is None) != (dps is None):
        raise ValueError(f"{who}: ps and dps are both given (two outputs) or both None (one output)")
    if pg.dim() != 2 or pg.shape[0] < 1 or pg.shape[1] < 1:
        raise ValueError(f"{who}: pg {tuple(pg.shape)}: want [B,S] with B, S >= 1")
    B, S = int(pg.shape[0]), int(pg.shape[1])
    if any(t is not None and t.numel() != B * S for t in (ps, y, dpg, dps)) or loss.numel() < 1 or \
            (per_crystal is not None and per_crystal.numel() != B):
        raise ValueError(f"{who}: " + ", ".join(f"{k} {tuple(t.shape)}" for k, t in ts.items() if t is not None)
                         + ": want B*S elements in ps, y, dpg, dps, B in per_crystal and at least 1 in loss")
    for k, t in ts.items():
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{who}: {k} must be contiguous (row slices of a table are), got strides {t.stride()}")
    args = (pg.data_ptr(), _p(ps), y.data_ptr(), B, S, B if B_global is None else int(B_global), int(kind),
            int(bool(clamp_target)), float(beta), 0.0 if delta is None else float(delta), dpg.data_ptr(), _p(dps), _p(per_crystal),
            loss.data_ptr())
    work = lambda: ("loss_rows", "loss_rows_kernel", "hbm", (2.0 if ps is None else 3.0) * pg.element_size() * 2 * B * S,
                    1 if per_crystal is None else 2)
    norm_rows = int(functional_norm_rows)
    if norm_rows < 0:
        raise ValueError(f"{who}: functional_norm_rows must be >= 0, got {functional_norm_rows}")
    if norm_rows == 0 and (functional_denominator is not None or functional_floor is not None):
        raise ValueError(f"{who}: functional_denominator / functional_floor belong to functional_norm_rows > 0 normalised rows")
    if norm_rows > 0 and functionals is None:
        raise ValueError(f"{who}: functional_norm_rows={norm_rows} without functionals: there is no table whose rows they could be")
    if weights is None and weight_index is None and bin_weights is None and functionals is None:   # today's callers issue today's launch
        _call("dosx_loss_rows" if dt == torch.float32 else "dosx_loss_rows_f64", *args, _stream(), w=work)
        return
    if weights is None:
        if weight_index is not None:
            raise ValueError(f"{who}: weight_index selects out of weights, which is None")
    else:
        if weights.dtype != dt or not weights.is_cuda:
            raise TypeError(f"{who}: weights must be a {dt} CUDA tensor, got {weights.dtype} on {weights.device}")
        if weights.dim() != 1 or not weights.is_contiguous():
            raise ValueError(f"{who}: weights must be a contiguous 1-D tensor, got shape {tuple(weights.shape)} strides "
                             f"{weights.stride()}")
        if weight_index is None and weights.numel() != B:
            raise ValueError(f"{who}: weights has {weights.numel()} entries for {B} crystals (a longer table needs weight_index)")
        if weight_index is not None and weights.numel() < 1:
            raise ValueError(f"{who}: weight_index selects out of an empty weights table")
    if weight_index is not None:
        if weight_index.dtype != torch.int32 or not weight_index.is_cuda:
            raise TypeError(f"{who}: weight_index must be an int32 CUDA tensor, got {weight_index.dtype} on {weight_index.device}")
        if weight_index.dim() != 1 or weight_index.numel() != B or not weight_index.is_contiguous():
            raise ValueError(f"{who}: weight_index must be a contiguous [B] = [{B}] tensor, got shape {tuple(weight_index.shape)} "
                             f"strides {weight_index.stride()}")
    if bin_weights is not None:
        if bin_weights.dtype != dt or not bin_weights.is_cuda:
            raise TypeError(f"{who}: bin_weights must be a {dt} CUDA tensor, got {bin_weights.dtype} on {bin_weights.device}")
        if bin_weights.dim() != 1 or bin_weights.numel() != S or not bin_weights.is_contiguous():
            raise ValueError(f"{who}: bin_weights must be a contiguous [S] = [{S}] tensor, got shape {tuple(bin_weights.shape)} "
                             f"strides {bin_weights.stride()}")
    if functionals is None:
        _call("dosx_loss_rows_w" if dt == torch.float32 else "dosx_loss_rows_w_f64", *args, _p(weights), _p(weight_index),
              _p(bin_weights), _stream(), w=work)
        return
    if isinstance(functional_kind, str):
        if functional_kind not in FUNCTIONAL_KINDS:
            raise ValueError(f"{who}: functional_kind {functional_kind!r} is not one of {sorted(FUNCTIONAL_KINDS)}")
        functional_kind = FUNCTIONAL_KINDS[functional_kind]
    lam = float(functional_weight)
    if not 0.0 <= lam < float("inf"):
        raise ValueError(f"{who}: functional_weight must be finite and >= 0, got {functional_weight}")
    if functionals.dtype != dt or not functionals.is_cuda:
        raise TypeError(f"{who}: functionals must be a {dt} CUDA tensor, got {functionals.dtype} on {functionals.device}")
    if functionals.dim() != 2 or functionals.shape[1] != S or not functionals.is_contiguous() or \
            not 1 <= functionals.shape[0] <= FUNCTIONAL_MAX or S > FUNCTIONAL_MAX:
        raise ValueError(f"{who}: functionals must be a contiguous [K,S] = [K,{S}] table with K, S <= {FUNCTIONAL_MAX}, got shape "
                         f"{tuple(functionals.shape)} strides {functionals.stride()}")
    K = int(functionals.shape[0])
    fwork = lambda: ("loss_rows_fn", "loss_fn_kernel", "hbm", (2.0 if ps is None else 3.0) * pg.element_size() * 2 * B * S
                     + pg.element_size() * K * S, 1 if per_crystal is None else 2)
    if norm_rows > 0:                  # the last norm_rows rows over the floored denominator functional: the normalised entry
        den = functional_denominator
        if norm_rows > K:
            raise ValueError(f"{who}: functional_norm_rows={norm_rows} of a table of K = {K} rows")
        if den is None or den.dtype != dt or not den.is_cuda:
            raise TypeError(f"{who}: functional_denominator must be a {dt} CUDA tensor, got "
                            f"{'None' if den is None else f'{den.dtype} on {den.device}'}")
        if den.dim() != 1 or den.numel() != S or not den.is_contiguous():
            raise ValueError(f"{who}: functional_denominator must be a contiguous [S] = [{S}] tensor, got shape {tuple(den.shape)} "
                             f"strides {den.stride()}")
        if functional_floor is None or not 0.0 < float(functional_floor) < float("inf"):
            raise ValueError(f"{who}: functional_floor must be finite and > 0, got {functional_floor}")
        d = _abi.FnNorm()
        d.fn_w, d.fn_den, d.K, d.K_norm, d.fn_kind = functionals.data_ptr(), den.data_ptr(), K, norm_rows, int(functional_kind)
        d.lam, d.den_floor = lam, float(functional_floor)
        nwork = lambda: ("loss_rows_fn_norm", "loss_fnn_kernel", "hbm", (2.0 if ps is None else 3.0) * pg.element_size() * 2 * B * S
                         + pg.element_size() * (K + 1) * S, 1 if per_crystal is None else 2)
        # the descriptor form: a recorded call carries at most 19 integer-class arguments (include/dosx.h: DosxFnNorm)
        _call("dosx_loss_rows_fn_norm_desc" if dt == torch.float32 else "dosx_loss_rows_fn_norm_desc_f64", *args, _p(weights),
              _p(weight_index), _p(bin_weights), C.byref(d), _stream(), w=nwork)
        return
    _call("dosx_loss_rows_fn" if dt == torch.float32 else "dosx_loss_rows_fn_f64", *args, _p(weights), _p(weight_index),
          _p(bin_weights), functionals.data_ptr(), K, int(functional_kind), lam, _stream(), w=fwork)


def loss_rows(pg: torch.Tensor, ps: Optional[torch.Tensor], y: torch.Tensor, kind, *, clamp_target: bool = False,
              beta: float = 1.0, delta: Optional[float] = None, dpg: torch.Tensor, dps: Optional[torch.Tensor] = None,
              per_crystal: Optional[torch.Tensor] = None, loss: torch.Tensor, B_global: Optional[int] = None,
              weights: Optional[torch.Tensor] = None, weight_index: Optional[torch.Tensor] = None,
              bin_weights: Optional[torch.Tensor] = None, functionals: Optional[torch.Tensor] = None,
              functional_kind="sq", functional_weight: float = 1.0, functional_denominator: Optional[torch.Tensor] = None,
              functional_norm_rows: int = 0, functional_floor: Optional[float] = None) -> None:
    """Per-crystal loss of the [B,S] predictions pg (and ps) against y with its gradient (include/dosx.h: dosx_loss_rows):
    ``l_b = f(pg_b) + beta f(ps_b)`` with f the crystal's RMSE, MSE, MAE or Huber(``delta``) term - ``kind`` a key of
    :data:`LOSS_KINDS` or its enumerator -, ``per_crystal[b] = l_b`` (optional), ``loss[0] = sum_b l_b / B_global`` (default B) and
    dpg / dps the gradient of loss[0].  ``clamp_target``: the eDOS target ``max(y, 0)``.  ``ps = dps = None``: a model with one
    output.  All float32, contiguous (row slices of larger tables are); a crystal whose RMSE is 0 gets a zero gradient.

    ``weights`` / ``weight_index`` / ``bin_weights`` (include/dosx.h: dosx_loss_rows_w): sample weights ``w_b`` - ``weights[b]``, or
    ``weights[weight_index[b]]`` out of a whole dataset's table with ``weight_index`` the batch's [B] int32 selection (its entries
    must lie inside the table: nothing here reads them) - and [S] energy-bin weights ``v_s`` (sum > 0): ``loss[0] = sum_b w_b l_b /
    B_global`` with f the ``v``-weighted means, ``per_crystal[b]`` still the crystal's own ``l_b``; ``w_b == 0`` writes zero
    gradient rows and a zero share whatever the crystal holds.  All three None: the unweighted entry, the launch it always was.

    ``functionals`` / ``functional_kind`` / ``functional_weight`` (include/dosx.h: dosx_loss_rows_fn): a [K,S] table of linear
    functionals ``F_k(p) = sum_s table[k,s] p_s`` (K, S <= 512) whose differences ``u_k = F_k(p_b) - F_k(t_b)`` add
    ``functional_weight / K * sum_k e(u_k)`` to each output's term, ``e(u) = u^2`` (``"sq"``) or ``|u|`` (``"abs"``) - the same
    launch, the rows written once.  ``per_crystal[b]`` includes the term.  Without a table the call is the one it was; with a
    table and ``functional_weight == 0`` the library runs the weighted kernels, bit for bit.

    ``functional_denominator`` / ``functional_norm_rows`` / ``functional_floor`` (include/dosx.h: dosx_loss_rows_fn_norm): the LAST
    ``functional_norm_rows`` rows of the table are divided by ``D+ = max(sum_s functional_denominator[s] x_s, functional_floor)`` on
    both sides, ``u_k = F_k(p_b) / D+(p_b) - F_k(t_b) / D+(t_b)`` - a band centre, a mean frequency, the cumulative curve of the
    shape; a floored denominator is a constant in the gradient.  The denominator is a [S] tensor like the table, the floor finite
    and > 0.  Such rows alone leave the scale of the prediction free: the pointwise term or a plain row carries it.  With
    ``functional_norm_rows == 0`` the call is the one above and the other two must be None."""
    _loss_rows("loss_rows", torch.float32, pg, ps, y, kind, clamp_target, beta, delta, dpg, dps, per_crystal, loss, B_global,
               weights, weight_index, bin_weights, functionals, functional_kind, functional_weight, functional_denominator,
               functional_norm_rows, functional_floor)


# ---- guarded optimizer step (csrc/step_guard.hip; include/dosx.h: DosxStepGuard) -----------------------------------------------
_GUARD_WORDS = C.sizeof(_abi.StepGuard) // 8
_STATUS_ADDRESS: dict = {}


def guard_buffers(device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(record, workspace) of one guarded trainer, both zeroed: the record as 12 float64 words (a DosxStepGuard; word 1 is
    ``norm``), the workspace of DOSX_GUARD_WORKSPACE_BYTES.  torch's allocations are 16-byte aligned."""
    rec = torch.zeros(_GUARD_WORDS, dtype=torch.float64, device=device)
    ws = torch.zeros(_abi.DOSX_GUARD_WORKSPACE_BYTES // 8, dtype=torch.int64, device=device)
    return rec, ws


def guard_read(rec: torch.Tensor) -> "_abi.StepGuard":
    """The record on the host: one 96-byte read-back (which waits for the current stream)."""
    return _abi.StepGuard.from_buffer_copy(rec.cpu().numpy().tobytes())


def exchange_status_address(device) -> int:
    """Device address of the exchanges' sticky stall status on ``device`` (dosx_exchange_status_address), asked for once."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _STATUS_ADDRESS:
        out = C.c_ulonglong(0)
        with torch.cuda.device(idx):
            _lib.check(_lib.load().dosx_exchange_status_address(C.byref(out)), "dosx_exchange_status_address")
        _STATUS_ADDRESS[idx] = int(out.value)
    return _STATUS_ADDRESS[idx]


def grad_guard(g: torch.Tensor, n: int, rec: torch.Tensor, ws: torch.Tensor, max_norm: Optional[float], lr: float, beta1: float,
               beta2: float, step: int, status_address: Optional[int] = None) -> None:
    """Statistics of the first n elements of the flat gradient ``g`` (fp32 or float64) into the record: norm, clip coefficient,
    non-finite count and first index, the skip verdict and the bias-correction scalars of the guarded AdamW behind it.
    ``max_norm`` None: no clipping; ``status_address``: :func:`exchange_status_address`, a stalled step is then skipped too."""
    if g.dtype not in (torch.float32, torch.float64) or not g.is_cuda or not g.is_contiguous():
        raise TypeError(f"grad_guard: a contiguous float32 / float64 CUDA gradient, got {g.dtype} on {g.device}")
    if not 0 <= n <= g.numel():
        raise ValueError(f"grad_guard: n = {n} of a gradient with {g.numel()} elements")
    if rec.dtype != torch.float64 or rec.numel() < _GUARD_WORDS or ws.numel() * ws.element_size() < _abi.DOSX_GUARD_WORKSPACE_BYTES:
        raise ValueError("grad_guard: record / workspace are not those of guard_buffers")
    f32 = g.dtype == torch.float32
    _call("dosx_grad_guard_f32" if f32 else "dosx_grad_guard_f64", g.data_ptr(), int(n), -1.0 if max_norm is None else float(max_norm),
          status_address, float(lr), float(beta1), float(beta2), int(step), rec.data_ptr(), ws.data_ptr(), _stream(),
          w=lambda: ("grad_guard", "grad_guard_kernel", "hbm", float(g.element_size()) * n))


# ---- AdamW on the flat buffers (csrc/adamw.hip): plain, guarded, with parameter groups, fp32 and float64 ---------------------------
def adamw_groups(groups, into: "Optional[_abi.AdamWGroups]" = None) -> "_abi.AdamWGroups":
    """The host struct of the grouped launches from ``(lr, weight_decay)`` pairs, one per group (a struct is passed through)."""
    if isinstance(groups, _abi.AdamWGroups):
        return groups
    groups = list(groups)
    if not 1 <= len(groups) <= _abi.DOSX_ADAMW_MAX_GROUPS:
        raise ValueError(f"adamw_groups: 1 to {_abi.DOSX_ADAMW_MAX_GROUPS} groups, got {len(groups)}")
    st = into if into is not None else _abi.AdamWGroups()
    st.n_groups = len(groups)
    for k, (lr, wd) in enumerate(groups):
        st.lr[k], st.weight_decay[k] = float(lr), float(wd)
    return st


def ema_decay_at(decay: float, warmup: bool, t: int, dtype=torch.float32) -> float:
    """The decay the EMA launches apply after ``t`` steps of averaging, rounded to ``dtype`` (dosx_adamw_ema_decay: the
    kernel's own expression, evaluated on the host)."""
    return float(_lib.load().dosx_adamw_ema_decay(float(decay), int(bool(warmup)), int(t), 4 if dtype == torch.float32 else 8))


def _adamw(who: str, dtype, p, g, m, v, n, beta1, beta2, eps, lr=None, weight_decay=None, step=None, grad_scale=None,
           chunk_group=None, groups=None, rec=None, ema=None) -> None:
    """All AdamW launches: the entry follows from ``dtype``, ``rec`` (the record of :func:`grad_guard`: the guarded
    entries), ``groups`` (the grouped ones) and ``ema`` (``(buffer, decay, warmup, t0)``: the same launch also keeps the
    exponential moving average of ``p`` in ``buffer`` - dosx_adamw_ema / _f64, which take every form's operands and ``step``
    always).  The operands are checked here because the C entry cannot: contiguous CUDA buffers of ``dtype`` with at least n
    elements and, grouped, n a multiple of 64 and a uint8 chunk map of at least n / 64 entries on their device - what the
    kernel indexes."""
    f32, grouped, n = dtype == torch.float32, groups is not None, int(n)
    bufs = (p, g, m, v) + ((ema[0],) if ema is not None else ())
    for t in bufs:
        if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.device != p.device:
            raise TypeError(f"{who}: contiguous {dtype} CUDA buffers on one device, got {t.dtype} on {t.device}")
    if not 0 <= n <= min(t.numel() for t in bufs):
        raise ValueError(f"{who}: n = {n} of buffers with {', '.join(str(t.numel()) for t in bufs)} elements")
    if ema is not None:
        return _adamw_ema(who, f32, bufs, n, beta1, beta2, eps, lr, weight_decay, step, grad_scale, chunk_group, groups, rec, ema)
    args = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n]
    if grouped:
        _chunk_map_ok(who, chunk_group, n, p.device)
        st = adamw_groups(groups)
        args += [chunk_group.data_ptr(), C.byref(st), float(beta1), float(beta2), float(eps), int(step)]
    else:
        args += [float(lr), float(beta1), float(beta2), float(eps), float(weight_decay)] + ([int(step)] if rec is None else [])
    if rec is not None:
        args.append(rec.data_ptr())
    elif f32:
        args.append(float(grad_scale))
    site = "adamw" + ("_grouped" if grouped else "") + ("_guarded" if rec is not None else "") + ("" if f32 else "_f64")
    _call("dosx_" + site, *args, _stream(),
          w=lambda: (site, "adamw_kernel", "hbm", (28.0 if f32 else 56.0) * n + (n / 64.0 if grouped else 0.0)))


def _chunk_map_ok(who: str, chunk_group, n: int, device) -> None:
    chunks = n // _abi.DOSX_ADAMW_GROUP_CHUNK
    if n % _abi.DOSX_ADAMW_GROUP_CHUNK:
        raise ValueError(f"{who}: n = {n} is not a multiple of {_abi.DOSX_ADAMW_GROUP_CHUNK}")
    if chunk_group.dtype != torch.uint8 or chunk_group.device != device or not chunk_group.is_contiguous() or \
            chunk_group.numel() < chunks:
        raise ValueError(f"{who}: the chunk map must be a contiguous uint8 tensor of at least {chunks} entries on {device}, "
                         f"got {chunk_group.dtype} x {chunk_group.numel()} on {chunk_group.device}")


def _adamw_ema(who, f32, bufs, n, beta1, beta2, eps, lr, weight_decay, step, grad_scale, chunk_group, groups, rec, ema) -> None:
    """:func:`_adamw` with an average: the one entry per type, the absent operands of the form as NULL / 0."""
    p, g, m, v, e = bufs
    _, decay, warmup, t0 = ema
    if step is None:
        raise ValueError(f"{who}: an EMA launch needs step (AdamW's time, guarded: the attempt count the guard was given)")
    st = None
    if groups is not None:
        _chunk_map_ok(who, chunk_group, n, p.device)
        st = adamw_groups(groups)
    desc = _abi.AdamWEma(e.data_ptr(), float(decay), int(bool(warmup)), int(t0))
    args = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 0.0 if lr is None else float(lr), float(beta1), float(beta2),
            float(eps), 0.0 if weight_decay is None else float(weight_decay), int(step)]
    if f32:
        args.append(1.0 if grad_scale is None else float(grad_scale))
    args += [_p(chunk_group) if st is not None else None, C.byref(st) if st is not None else None, _p(rec), C.byref(desc)]
    site = "adamw_ema" + ("" if f32 else "_f64")
    _call("dosx_" + site, *args, _stream(),
          w=lambda: (site, "adamw_kernel", "hbm", (36.0 if f32 else 72.0) * n + (n / 64.0 if st is not None else 0.0)))


def swap_buffers(a: torch.Tensor, b: torch.Tensor, n: Optional[int] = None) -> None:
    """Exchange the first ``n`` elements (default: all) of two contiguous CUDA buffers of one dtype in one launch
    (dosx_swap_buffers); ``n`` elements must be a multiple of 16 bytes."""
    if a.dtype != b.dtype or not a.is_cuda or a.device != b.device or not (a.is_contiguous() and b.is_contiguous()):
        raise TypeError(f"swap_buffers: two contiguous CUDA buffers of one dtype on one device, got {a.dtype} on {a.device} and "
                        f"{b.dtype} on {b.device}")
    n = min(a.numel(), b.numel()) if n is None else int(n)
    if not 0 <= n <= min(a.numel(), b.numel()):
        raise ValueError(f"swap_buffers: n = {n} of buffers with {a.numel()} and {b.numel()} elements")
    nbytes = n * a.element_size()
    _call("dosx_swap_buffers", a.data_ptr(), b.data_ptr(), nbytes, _stream(),
          w=lambda: ("swap_buffers", "swap_kernel", "hbm", 4.0 * nbytes))


def _grad_accumulate(who: str, dt: torch.dtype, dst, a, b, n, sdst, sa, sb) -> None:
    ts = {"dst": dst, "a": a, "b": b, "sdst": sdst, "sa": sa, "sb": sb}
    for k, t in ts.items():
        if t is None:
            if k in ("dst", "a"):
                raise TypeError(f"{who}: {k} is required")
            continue
        if t.dtype != dt or not t.is_cuda or t.device != dst.device or not t.is_contiguous():
            raise TypeError(f"{who}: {k} must be a contiguous {dt} CUDA tensor on dst's device, got {t.dtype} on {t.device}, "
                            f"strides {t.stride()}")
    vecs = [t for t in (dst, a, b) if t is not None]
    n = min(t.numel() for t in vecs) if n is None else int(n)
    if not 0 <= n <= min(t.numel() for t in vecs):
        raise ValueError(f"{who}: n = {n} of buffers with {', '.join(str(t.numel()) for t in vecs)} elements")
    if (sdst is None) != (sa is None) or (sb is not None and sdst is None):
        raise ValueError(f"{who}: sdst and sa go together, sb only with them (all three None: no scalar)")
    if any(t is not None and t.numel() < 1 for t in (sdst, sa, sb)):
        raise ValueError(f"{who}: a scalar operand without an element")
    _call("dosx_grad_accumulate" if dt == torch.float32 else "dosx_grad_accumulate_f64", dst.data_ptr(), a.data_ptr(), _p(b), n,
          _p(sdst), _p(sa), _p(sb), _stream(),
          w=lambda: ("grad_accumulate", "grad_accumulate_kernel", "hbm", (2.0 if b is None else 3.0) * dst.element_size() * n))


def grad_accumulate(dst: torch.Tensor, a: torch.Tensor, b: Optional[torch.Tensor] = None, n: Optional[int] = None, *,
                    sdst: Optional[torch.Tensor] = None, sa: Optional[torch.Tensor] = None,
                    sb: Optional[torch.Tensor] = None) -> None:
    """``dst[:n] = a[:n] + b[:n]`` in one launch, ``dst[:n] = a[:n]`` when ``b`` is None (dosx_grad_accumulate): how the fused
    trainers sum the flat gradients of the batches of one optimizer step.  ``dst`` may be ``a`` or ``b`` itself, no other
    overlap; ``n`` defaults to the shortest buffer.  ``sdst`` / ``sa`` / ``sb``: the same for element 0 of three scalars
    (``sdst[0] = sa[0] + sb[0]``, a copy when ``sb`` is None).  fp32, contiguous, 16-byte aligned; every element is one IEEE add -
    bit for bit ``torch.add(a, b)``."""
    _grad_accumulate("grad_accumulate", torch.float32, dst, a, b, n, sdst, sa, sb)


def adamw(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, ema=None):
    """torch.optim.AdamW's update of the first n elements of the flat fp32 buffers, on ``g * grad_scale`` (dosx_adamw).
    ``ema=(buffer, decay, warmup, t0)``, here and on the seven functions below: the launch also keeps the exponential moving
    average of the parameters (dosx_adamw_ema / _f64); p, m, v are bitwise those without it."""
    _adamw("adamw", torch.float32, p, g, m, v, n, beta1, beta2, eps, lr, weight_decay, step, grad_scale, ema=ema)


def adamw_guarded(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, rec, step=None, ema=None):
    """:func:`adamw` behind :func:`grad_guard`: skip, clip coefficient and bias correction come from the record.  ``step``
    (the attempt count the guard was given) is read with ``ema`` only."""
    _adamw("adamw_guarded", torch.float32, p, g, m, v, n, beta1, beta2, eps, lr, weight_decay, step=step if ema is not None else None,
           rec=rec, ema=ema)


def adamw_grouped(p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step, grad_scale=1.0, ema=None):
    """:func:`adamw` with parameter groups: ``chunk_group[c]`` names the group of the elements [64c, 64c + 64), ``groups`` is
    ``(lr, weight_decay)`` per group (or the struct of :func:`adamw_groups`).  Bit for bit :func:`adamw` on every run of chunks
    of one group with that group's values."""
    _adamw("adamw_grouped", torch.float32, p, g, m, v, n, beta1, beta2, eps, step=step, grad_scale=grad_scale,
           chunk_group=chunk_group, groups=groups, ema=ema)


def adamw_grouped_guarded(p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step, rec, ema=None):
    """:func:`adamw_grouped` behind :func:`grad_guard`: skip, clip and bc2_scale come from the record, the step size of group k
    is what the record would hold had the guard been called with ``lr_k``.  ``step``: the attempt count the guard was given."""
    _adamw("adamw_grouped_guarded", torch.float32, p, g, m, v, n, beta1, beta2, eps, step=step, chunk_group=chunk_group,
           groups=groups, rec=rec, ema=ema)


def dropout_mask(mask: torch.Tensor, p: float, seed_dev: torch.Tensor, stream_id: int) -> None:
    """mask <- {0, 1/(1-p)} multipliers (include/dosx.h: dosx_dropout_mask); seed_dev: 1-element int64 device tensor."""
    assert mask.dtype == torch.float32 and mask.is_contiguous() and seed_dev.dtype == torch.int64 and seed_dev.is_cuda
    _call("dosx_dropout_mask", mask.data_ptr(), mask.numel(), float(p), seed_dev.data_ptr(), int(stream_id), _stream(),
          w=lambda: ("dropout_mask", "dropout_mask_kernel", "hbm", 4.0 * mask.numel()))


def copy_many(pairs) -> None:
    """dst.copy_(src) for every (dst, src) pair of same-sized 4-byte-element contiguous device tensors, in one launch."""
    jobs = []
    for dst, src in pairs:
        assert dst.is_contiguous() and src.is_contiguous() and dst.element_size() == 4 and src.dtype == dst.dtype \
            and dst.numel() == src.numel() and src.device == dst.device, "copy_many: mismatched pair"
        if dst.numel():
            jobs.append((src.data_ptr(), dst.data_ptr(), dst.numel()))
    if not jobs:
        return
    arr = (_lib.CopyJob * len(jobs))(*jobs)
    _call("dosx_copy_many", arr, len(jobs), _stream(),
          w=lambda: ("copy_many", "copy_many_kernel", "hbm", 8.0 * sum(j[2] for j in jobs)))


def fill(t: torch.Tensor, value: float):
    _call("dosx_fill", t.data_ptr(), float(value), t.numel(), _stream(),
          w=lambda: ("fill", "fill_kernel", "hbm", 4.0 * t.numel()))


def embed_rows(table, idx, out, rows, width):
    _call("dosx_embed_rows", _p(table), _p(idx), _p(out), rows, width, _stream())


def embed_rows_bwd(dout_ptr, ld, idx, dtable, rows, table_rows, width):
    _call("dosx_embed_rows_bwd", dout_ptr, ld, _p(idx), _p(dtable), rows, table_rows, width, _stream())


def reduce_rows(src_ptr, ld_src, dst_ptr, ld_dst, n_out, n_red, stride_out, stride_red, width, accumulate=False):
    _call("dosx_reduce_rows", src_ptr, ld_src, dst_ptr, ld_dst, n_out, n_red, stride_out, stride_red, width,
          int(accumulate), _stream(),
          w=lambda: ("reduce_rows", "reduce_rows_kernel", "hbm", 4.0 * width * n_out * (n_red + 1)))


def act_bwd(dy, y, slope, out):
    _call("dosx_act_bwd", _p(dy), _p(y), float(slope), _p(out), dy.numel(), _stream(),
          w=lambda: ("act_bwd", "act_bwd_kernel", "hbm", 12.0 * dy.numel()))


def csr_build(edge_index: torch.Tensor, batch: torch.Tensor, num_graphs: int, want_perm: bool = True):
    """Graph metadata from PyG-style index tensors ON THE DEVICE (include/dosx.h: dosx_csr_build); returns a dict of
    int32 device tensors (+ ``inv_deg`` fp32, ``edge_perm`` int64 or None, ``n_max`` 1-element device tensor)."""
    assert edge_index.is_cuda and batch.is_cuda and edge_index.dtype == torch.int64 and batch.dtype == torch.int64
    ei = edge_index.contiguous()
    bv = batch.contiguous()
    dev, E, N, B = ei.device, int(ei.shape[1]), int(bv.shape[0]), int(num_graphs)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    out = {"src": i32(E), "dst": i32(E), "rowptr_dst": i32(N + 1), "perm_src": i32(E), "rowptr_src": i32(N + 1),
           "graph_ptr": i32(B + 1), "node_graph": i32(N), "dense_row": i32(N),
           "inv_deg": torch.empty(N, dtype=torch.float32, device=dev), "n_max": i32(1),
           "edge_perm": torch.empty(E, dtype=torch.int64, device=dev) if want_perm else None}
    nbytes = C.c_size_t(0)
    _lib.check(_lib.load().dosx_csr_workspace_bytes(E, C.byref(nbytes)), "dosx_csr_workspace_bytes")
    ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    _call("dosx_csr_build", ei.data_ptr(), bv.data_ptr(), N, E, B, out["src"].data_ptr(), out["dst"].data_ptr(),
          _p(out["edge_perm"]), out["rowptr_dst"].data_ptr(), out["perm_src"].data_ptr(), out["rowptr_src"].data_ptr(),
          out["graph_ptr"].data_ptr(), out["node_graph"].data_ptr(), out["dense_row"].data_ptr(), out["inv_deg"].data_ptr(),
          out["n_max"].data_ptr(), ws.data_ptr(), C.c_size_t(ws.numel()), _stream())
    return out


def neighbor_list(pos: torch.Tensor, cell: torch.Tensor, atom_ptr: torch.Tensor, cutoff: float,
                  self_interaction: bool = True, pbc=(True, True, True)):
    """Periodic neighbour list of C crystals in one go (include/dosx.h: dosx_neighbor_count / _fill; the job ASE's
    ``neighbor_list("ijS", ...)`` does in `utils.py:267`).  ``pos [N,3]`` fp64, ``cell [C,3,3]`` fp64 (rows = lattice
    vectors), ``atom_ptr [C+1]`` int32, all on the GPU.  Returns a dict of device tensors: ``crystal``, ``src``,
    ``dst`` (crystal-local atom indices), ``shift [E,3]`` int32, ``edge_vec [E,3]`` fp64, ``edge_ptr [C+1]`` int64."""
    assert pos.is_cuda and pos.dtype == torch.float64 and cell.dtype == torch.float64 and atom_ptr.dtype == torch.int32
    pos, cell, atom_ptr = pos.contiguous(), cell.contiguous(), atom_ptr.contiguous()
    dev, Cn = pos.device, int(cell.shape[0])
    assert cell.shape == (Cn, 3, 3) and atom_ptr.shape == (Cn + 1,)
    n = (atom_ptr[1:] - atom_ptr[:-1]).to(torch.int64)
    pair_ptr = torch.zeros(Cn + 1, dtype=torch.int64, device=dev)
    pair_ptr[1:] = torch.cumsum(n * n, 0)
    n_pairs = int(pair_ptr[-1])                      # featurisation runs once per dataset: a host read is fine here
    mask = sum(1 << k for k in range(3) if pbc[k])
    count = torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev)
    _call("dosx_neighbor_count", pos.data_ptr(), cell.data_ptr(), atom_ptr.data_ptr(), pair_ptr.data_ptr(), Cn,
          n_pairs, C.c_double(cutoff), int(self_interaction), mask, count.data_ptr(), _stream())
    incl = torch.cumsum(count[:n_pairs].to(torch.int64), 0)
    off = incl - count[:n_pairs]
    E = int(incl[-1]) if n_pairs else 0
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    out = {"crystal": i32(E), "src": i32(E), "dst": i32(E), "shift": i32(E, 3),
           "edge_vec": torch.empty(E, 3, dtype=torch.float64, device=dev)}
    if E:
        _call("dosx_neighbor_fill", pos.data_ptr(), cell.data_ptr(), atom_ptr.data_ptr(), pair_ptr.data_ptr(), Cn,
              n_pairs, C.c_double(cutoff), int(self_interaction), mask, off.data_ptr(), out["crystal"].data_ptr(),
              out["src"].data_ptr(), out["dst"].data_ptr(), out["shift"].data_ptr(), out["edge_vec"].data_ptr(), _stream())
    edge_ptr = torch.zeros(Cn + 1, dtype=torch.int64, device=dev)
    if n_pairs:
        ends = pair_ptr[1:] - 1                      # last pair of every crystal (crystals have >= 1 atom)
        edge_ptr[1:] = incl[ends]
    out["edge_ptr"] = edge_ptr
    return out


def knn_graph(pos: torch.Tensor, cell: torch.Tensor, atom_ptr: torch.Tensor, radius: float = 8.0, k: int = 12,
              centers: Optional[torch.Tensor] = None, var: float = 0.2, tol: float = 1e-8, pbc=(True, True, True)):
    """The ``k`` nearest periodic neighbours inside ``radius`` of every atom of C crystals, in one launch (include/dosx.h:
    dosx_knn_graph; the job pymatgen's ``get_all_neighbors`` + sort + cut does in `data/mat2graph.py:193,216-232`).
    ``pos [N,3]`` fp64, ``cell [C,3,3]`` fp64 (rows = lattice vectors), ``atom_ptr [C+1]`` int32, all on the GPU.  Returns a
    dict of device tensors: ``nbr_idx [N,k]`` int32 (crystal-local), ``nbr_shift [N,k,3]`` int32, ``nbr_dist [N,k]`` fp64,
    ``nbr_count [N]`` int32 (ranks from there on are the reference's padding: index 0 at ``radius + 1``), and with
    ``centers [G]`` fp64 also ``edge_attr [N*k,G]`` fp32 = exp(-(dist - centers)^2 / var^2) (`:162-179`)."""
    assert pos.is_cuda and pos.dtype == torch.float64 and cell.dtype == torch.float64 and atom_ptr.dtype == torch.int32
    pos, cell, atom_ptr = pos.contiguous(), cell.contiguous(), atom_ptr.contiguous()
    dev, Cn, N, k = pos.device, int(cell.shape[0]), int(pos.shape[0]), int(k)
    assert pos.shape == (N, 3) and cell.shape == (Cn, 3, 3) and atom_ptr.shape == (Cn + 1,)
    out = {"nbr_idx": torch.empty(N, k, dtype=torch.int32, device=dev),
           "nbr_shift": torch.empty(N, k, 3, dtype=torch.int32, device=dev),
           "nbr_dist": torch.empty(N, k, dtype=torch.float64, device=dev),
           "nbr_count": torch.empty(N, dtype=torch.int32, device=dev)}
    d = _lib.Knn()
    d.C, d.N, d.K, d.pbc_mask = Cn, N, k, sum(1 << a for a in range(3) if pbc[a])
    d.radius, d.tol, d.pad_dist, d.var = float(radius), float(tol), float(radius) + 1.0, float(var)
    d.pos, d.cell, d.atom_ptr = pos.data_ptr(), cell.data_ptr(), atom_ptr.data_ptr()
    if centers is not None:
        assert centers.is_cuda and centers.dtype == torch.float64 and centers.dim() == 1
        centers = centers.contiguous()
        d.G, d.centers = int(centers.shape[0]), centers.data_ptr()
        out["edge_attr"] = torch.empty(N * k, d.G, dtype=torch.float32, device=dev)
        d.edge_attr = out["edge_attr"].data_ptr()
    for key in ("nbr_idx", "nbr_shift", "nbr_dist", "nbr_count"):
        setattr(d, key, out[key].data_ptr())
    if N:                                            # (an empty tensor has a null address, which the entry point refuses)
        _call("dosx_knn_graph", C.byref(d), _stream())
    return out


def _sym_descriptor(d, cell, frac, species, atom_ptr, symprec, n_min, n_max):
    assert frac.is_cuda and frac.dtype == torch.float64 and cell.dtype == torch.float64
    assert species.dtype == torch.int32 and atom_ptr.dtype == torch.int32
    cell, frac, species, atom_ptr = cell.contiguous(), frac.contiguous(), species.contiguous(), atom_ptr.contiguous()
    Cn, N = int(cell.shape[0]), int(frac.shape[0])
    assert frac.shape == (N, 3) and cell.shape == (Cn, 3, 3) and atom_ptr.shape == (Cn + 1,) and species.shape == (N,)
    d.C, d.N, d.n_min, d.n_max, d.symprec = Cn, N, int(n_min), int(n_max), float(symprec)
    d.cell, d.frac, d.species, d.atom_ptr = cell.data_ptr(), frac.data_ptr(), species.data_ptr(), atom_ptr.data_ptr()
    return (cell, frac, species, atom_ptr), Cn, N


def sym_translations(cell: torch.Tensor, frac: torch.Tensor, species: torch.Tensor, atom_ptr: torch.Tensor,
                     symprec: float, n_min: int, n_max: int) -> torch.Tensor:
    """Pure translations of C crystals in one launch (include/dosx.h: dosx_sym_translations).  ``cell [C,3,3]`` fp64
    Delaunay-reduced (rows = lattice vectors), ``frac [N,3]`` fp64 fractional rows, ``species [N]`` and ``atom_ptr [C+1]`` int32,
    all on the GPU; ``n_min`` / ``n_max``: atoms of the smallest / largest crystal (the caller built ``atom_ptr``).  Returns
    ``flag [N]`` uint8: 1 where ``frac[j] - frac[ref]`` is a pure translation of j's crystal."""
    d = _lib.SymTranslations()
    keep, Cn, N = _sym_descriptor(d, cell, frac, species, atom_ptr, symprec, n_min, n_max)
    flag = torch.zeros(N, dtype=torch.uint8, device=frac.device)
    d.flag = flag.data_ptr()
    _call("dosx_sym_translations", C.byref(d), _stream())
    return flag


def sym_point_group(cell: torch.Tensor, frac: torch.Tensor, species: torch.Tensor, atom_ptr: torch.Tensor,
                    symprec: float, n_min: int, n_max: int):
    """Point groups of C reduced primitive cells in one launch (include/dosx.h: dosx_sym_point_group); arguments as
    ``sym_translations``.  Returns a dict of device tensors: ``n_lattice_ops [C]``, ``n_ops [C]`` int32, ``ops [C,48,9]`` int8
    (the kept matrices in lexicographic order, zeros after them), ``hist [C,5]`` int32 (distinct proper parts by trace -1..3),
    ``code [C]`` int32 (0..6 the reference's crystal-system codes, 7 = INCONSISTENT)."""
    d = _lib.SymPointGroup()
    keep, Cn, N = _sym_descriptor(d, cell, frac, species, atom_ptr, symprec, n_min, n_max)
    dev = frac.device
    out = {"n_lattice_ops": torch.zeros(Cn, dtype=torch.int32, device=dev), "n_ops": torch.zeros(Cn, dtype=torch.int32, device=dev),
           "ops": torch.zeros(Cn, 48, 9, dtype=torch.int8, device=dev), "hist": torch.zeros(Cn, 5, dtype=torch.int32, device=dev),
           "code": torch.full((Cn,), 7, dtype=torch.int32, device=dev)}
    for key, t in out.items():
        setattr(d, key, t.data_ptr())
    _call("dosx_sym_point_group", C.byref(d), _stream())
    return out


def _spectra_descriptor(d, ptr, e, v, shift, e0, de, bins, n_min, n_max, normalize):
    """Fills the fields DosxSpectra and DosxSpectraInterp share; returns (tensors to keep alive, outputs)."""
    assert ptr.is_cuda and ptr.dtype == torch.int32 and e.dtype == v.dtype == shift.dtype == torch.float64
    ptr, e, v, shift = ptr.contiguous(), e.contiguous(), v.contiguous(), shift.contiguous()
    Cn, T, S = int(shift.shape[0]), int(e.shape[0]), int(bins)
    assert ptr.shape == (Cn + 1,) and e.shape == v.shape == (T,) and shift.shape == (Cn,)
    dev, rows = ptr.device, max(S, 0)
    out = {"y": torch.empty(Cn, rows, dtype=torch.float64, device=dev), "y_max": torch.empty(Cn, dtype=torch.float64, device=dev),
           "area": torch.empty(Cn, dtype=torch.float64, device=dev), "report": torch.empty(Cn, 4, dtype=torch.int32, device=dev)}
    if normalize:
        out["y_norm"] = torch.empty(Cn, rows, dtype=torch.float64, device=dev)
    d.C, d.T, d.S, d.n_min, d.n_max, d.e0, d.de = Cn, T, S, int(n_min), int(n_max), float(e0), float(de)
    d.ptr, d.shift = ptr.data_ptr(), shift.data_ptr()
    if T:                                            # (an empty tensor has a null address)
        d.e, d.v = e.data_ptr(), v.data_ptr()
    for key, t in out.items():
        setattr(d, key, t.data_ptr())
    return (ptr, e, v, shift), out


def spectra_broaden(ptr: torch.Tensor, e: torch.Tensor, v: torch.Tensor, shift: torch.Tensor, sigma: torch.Tensor, e0: float,
                    de: float, bins: int, n_min: int, n_max: int, kind: int = _abi.DOSX_SPECTRA_CURVE, cutoff: float = 6.0,
                    normalize: bool = False):
    """Gaussian broadening of the raw spectra of C crystals onto the grid ``e0 + de * s``, ``s < bins``, in one launch
    (include/dosx.h: dosx_spectra_broaden).  ``ptr [C+1]`` int32, ``e [T]`` / ``v [T]`` fp64 (crystal c owns
    ``[ptr[c], ptr[c+1])``), ``shift [C]`` / ``sigma [C]`` fp64, all on the GPU; ``kind``: ``_abi.DOSX_SPECTRA_CURVE`` (a tabulated
    density, trapezoid weights) or ``DOSX_SPECTRA_POINTS`` (delta peaks); ``n_min`` / ``n_max``: samples of the smallest / largest
    crystal (the caller built ``ptr``).  Returns a dict of device tensors: ``y [C,bins]``, ``y_max [C]``, ``area [C]`` fp64,
    ``report [C,4]`` int32 (n_inside, covered, bad, unsorted), and with ``normalize`` also ``y_norm [C,bins]``."""
    d = _lib.Spectra()
    assert sigma.dtype == torch.float64 and sigma.shape == shift.shape
    sigma = sigma.contiguous()
    keep, out = _spectra_descriptor(d, ptr, e, v, shift, e0, de, bins, n_min, n_max, normalize)
    d.kind, d.cutoff, d.sigma = int(kind), float(cutoff), sigma.data_ptr()
    _call("dosx_spectra_broaden", C.byref(d), _stream())
    return out


def spectra_interp(ptr: torch.Tensor, e: torch.Tensor, v: torch.Tensor, shift: torch.Tensor, e0: float, de: float, bins: int,
                   n_min: int, n_max: int, normalize: bool = False):
    """Linear interpolation of C tabulated curves at the grid ``e0 + de * s``, zero outside each curve, in one launch
    (include/dosx.h: dosx_spectra_interp); arguments and result as ``spectra_broaden``."""
    d = _lib.SpectraInterp()
    keep, out = _spectra_descriptor(d, ptr, e, v, shift, e0, de, bins, n_min, n_max, normalize)
    _call("dosx_spectra_interp", C.byref(d), _stream())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# float64 program (csrc/f64.hip, include/dosx.h "float64 program"): thin wrappers, used by functional64.py
# ---------------------------------------------------------------------------------------------------------------------
ACT64_NONE, ACT64_RELU, ACT64_LEAKY, ACT64_PRELU = _abi.DOSX_ACT64_NONE, _abi.DOSX_ACT64_RELU, _abi.DOSX_ACT64_LEAKY, _abi.DOSX_ACT64_PRELU
COLSUM64_ROWS = _abi.DOSX_COLSUM64_ROWS
_WGRAD64_ROWS = 512                    # rows of M per split of dosx_wgrad_f64


def _chk_f64(*ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float64 or not t.is_cuda or t.stride(-1) != 1):
            raise TypeError(f"dosx fp64 ops need float64 CUDA tensors with unit inner stride, got {t.dtype} on {t.device}")


def _chk_c64(*ts):
    """fp64 operands the kernels index with their logical row width (no row stride argument): must be contiguous."""
    _chk_f64(*ts)
    for t in ts:
        if t is not None and not t.is_contiguous():
            raise ValueError(f"dosx fp64 op needs a contiguous operand here, got shape {tuple(t.shape)} strides {t.stride()}")


def keep_alive(t: torch.Tensor) -> torch.Tensor:
    """A tensor created inside a program by anything but alloc / alloc64 (a torch.empty dropout mask, an arange index): kept
    alive for the recorded program while recording - the descriptors hold raw pointers, and the caching allocator would hand
    a freed buffer to someone else."""
    if RECORDER.active:
        RECORDER.keep.append(t)
    return t


def alloc64(device, *shape) -> torch.Tensor:
    """Uninitialised fp64 device buffer (kept alive for the recorded program while recording, like alloc)."""
    return keep_alive(torch.empty(shape, device=device, dtype=torch.float64))


def seg64(t: torch.Tensor, rmap: Optional[RowMap] = None) -> _lib.Seg64:
    """A K-segment: all columns of the 2-D fp64 tensor (or column slice) ``t``, rows through ``rmap``."""
    _chk_f64(t)
    assert t.dim() == 2
    return _lib.Seg64(t.data_ptr(), t.stride(0), t.shape[1], rmap if rmap is not None else ident())


def gemm64(M: int, N: int, segs: Sequence[_lib.Seg64], w: torch.Tensor, out: torch.Tensor, *, w_layout: int = 0,
           bias=None, act: int = ACT64_NONE, alpha=None, pre=None, res=None) -> torch.Tensor:
    """out[M,N] = act(cat(segs) @ op(w) + bias) + res; ``pre`` (optional) receives acc + bias.  w_layout 0: w[N,K], 1: w[K,N]."""
    _chk_f64(w, out, bias, alpha, pre, res)
    assert pre is None or pre.stride(0) == out.stride(0), "pre shares the row stride of out (DosxGemm64.ldo)"
    d = _lib.Gemm64()
    d.M, d.N, d.K, d.nseg = M, N, sum(s.width for s in segs), len(segs)
    for i, s in enumerate(segs):
        d.a[i] = s
    d.w, d.ldw, d.w_layout = w.data_ptr(), w.stride(0), w_layout
    d.act, d.alpha, d.bias = act, _p(alpha), _p(bias)
    d.out, d.ldo, d.pre = out.data_ptr(), out.stride(0), _p(pre)
    d.res, d.ldr = _p(res), (res.stride(0) if res is not None else 0)
    _call("dosx_gemm_f64", C.byref(d), _stream())
    return out


def wgrad64(M: int, dy: torch.Tensor, segs: Sequence[_lib.Seg64], dw: torch.Tensor, accumulate: bool = False) -> None:
    """dw[N,K] (+)= dy[M,N]^T @ cat(segs)[M,K], split over M with a fixed-order reduction of the splits."""
    _chk_f64(dy, dw)
    N, K = dw.shape
    d = _lib.Wgrad64()
    d.M, d.N, d.K = M, N, K
    d.dy, d.lddy = dy.data_ptr(), dy.stride(0)
    d.nseg = len(segs)
    for i, s in enumerate(segs):
        d.x[i] = s
    d.dw, d.ldd, d.accumulate = dw.data_ptr(), dw.stride(0), int(accumulate)
    d.nsplit = max(1, min(64, M // _WGRAD64_ROWS))
    part = alloc64(dw.device, d.nsplit, N, K) if d.nsplit > 1 else None
    d.partials = _p(part)
    _call("dosx_wgrad_f64", C.byref(d), _stream())


def colsum64(src: torch.Tensor, out: torch.Tensor, accumulate: bool = False) -> None:
    """out[N] (+)= src[M,N].sum(0), rows added in order."""
    _chk_f64(src)
    _chk_c64(out)
    M, N = src.shape
    part = alloc64(src.device, (M + COLSUM64_ROWS - 1) // COLSUM64_ROWS, N) if M > COLSUM64_ROWS else None
    _call("dosx_colsum_f64", src.data_ptr(), M, N, src.stride(0), _p(part), out.data_ptr(), int(accumulate), _stream())


def layernorm64(z: torch.Tensor, gamma, beta, alpha=None):
    """(xhat, rstd, prelu(LN(z)) or LN(z)) of z [M,W], eps 1e-5."""
    _chk_c64(z, gamma, beta, alpha)
    M, W = z.shape
    xhat, rstd, out = alloc64(z.device, M, W), alloc64(z.device, M), alloc64(z.device, M, W)
    _call("dosx_layernorm_f64", z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _p(alpha), xhat.data_ptr(), rstd.data_ptr(),
          out.data_ptr(), M, W, _stream())
    return xhat, rstd, out


def layernorm_bwd64(dout: torch.Tensor, xhat, rstd, gamma, beta, alpha=None):
    """(dz [M,W], part [M, 2W+1]): column sums of part are dgamma | dbeta | dalpha."""
    _chk_c64(dout, xhat, rstd, gamma, beta, alpha)
    M, W = xhat.shape
    dz, part = alloc64(xhat.device, M, W), alloc64(xhat.device, M, 2 * W + 1)
    _call("dosx_layernorm_bwd_f64", dout.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
          _p(alpha), dz.data_ptr(), part.data_ptr(), M, W, _stream())
    return dz, part


def act_bwd64(dy: torch.Tensor, z: torch.Tensor, act: int, alpha=None):
    """(dz, part): dz = dy * act'(z); part [M,1] the per-row dalpha terms for ACT64_PRELU (else None)."""
    _chk_c64(dy, alpha)                  # dy: row stride W; z: its own row stride
    _chk_f64(z)
    M, W = dy.shape
    dz = alloc64(dy.device, M, W)
    part = alloc64(dy.device, M, 1) if act == ACT64_PRELU else None
    _call("dosx_act_bwd_f64", dy.data_ptr(), z.data_ptr(), z.stride(0), act, _p(alpha), dz.data_ptr(), _p(part), M, W,
          _stream())
    return dz, part


def edge_feat_sh1_64(edge_vec: torch.Tensor, r_max: float = 4.0) -> torch.Tensor:
    _chk_c64(edge_vec)
    assert edge_vec.dim() == 2 and edge_vec.shape[1] == 3, tuple(edge_vec.shape)
    E = edge_vec.shape[0]
    out = alloc64(edge_vec.device, E, 4)
    _call("dosx_edge_feat_sh1_f64", edge_vec.data_ptr(), out.data_ptr(), E, C.c_double(r_max), _stream())
    return out


def segment_mean64(src: torch.Tensor, rowptr: torch.Tensor, N: int) -> torch.Tensor:
    _chk_c64(src)
    out = alloc64(src.device, N, src.shape[1])
    _call("dosx_segment_mean_f64", src.data_ptr(), rowptr.data_ptr(), out.data_ptr(), N, src.shape[1], _stream())
    return out


def segment_mean_bwd64(dagg: torch.Tensor, dst, rowptr, res: Optional[torch.Tensor], E: int) -> torch.Tensor:
    _chk_f64(dagg)
    _chk_c64(res)
    H = dagg.shape[1]
    out = alloc64(dagg.device, E, H)
    _call("dosx_segment_mean_bwd_f64", dagg.data_ptr(), dagg.stride(0), dst.data_ptr(), rowptr.data_ptr(), _p(res),
          out.data_ptr(), E, H, _stream())
    return out


def gather_bwd64(dcat: torch.Tensor, m, base0: Optional[torch.Tensor], base1: Optional[torch.Tensor], N: int, H: int):
    _chk_f64(dcat, base0, base1)
    dx = alloc64(dcat.device, N, H)
    _call("dosx_gather_bwd_f64", dcat.data_ptr(), dcat.stride(0), m.rowptr_src.data_ptr(), m.perm_src.data_ptr(),
          m.rowptr_dst.data_ptr(), _p(base0), base0.stride(0) if base0 is not None else 0, _p(base1),
          base1.stride(0) if base1 is not None else 0, dx.data_ptr(), N, H, _stream())
    return dx


def graph_pool64(x: torch.Tensor, graph_ptr: torch.Tensor, B: int) -> torch.Tensor:
    _chk_c64(x)
    out = alloc64(x.device, B, x.shape[1])
    _call("dosx_graph_pool_f64", x.data_ptr(), graph_ptr.data_ptr(), out.data_ptr(), B, x.shape[1], _stream())
    return out


def rows_add64(M: int, a: torch.Tensor, b: Optional[torch.Tensor] = None, ia=None, ib=None) -> torch.Tensor:
    """out[r] = a[ia[r] or r] + b[ib[r] or r], [M, width of a]."""
    _chk_f64(a, b)
    W = a.shape[1]
    out = alloc64(a.device, M, W)
    _call("dosx_rows_add_f64", a.data_ptr(), a.stride(0), _p(ia), _p(b), b.stride(0) if b is not None else 0, _p(ib),
          out.data_ptr(), W, M, W, _stream())
    return out


def reduce_rows64(src: torch.Tensor, n_out: int, n_red: int, stride_out: int, stride_red: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = sum_{j < n_red} src[i * stride_out + j * stride_red] (rows added in order of j); ``out`` [n_out, width]
    optional (a gradient slot, say)."""
    _chk_f64(src, out)
    W = src.shape[1]
    if out is None:
        out = alloc64(src.device, n_out, W)
    assert out.shape[0] == n_out and out.shape[1] == W
    _call("dosx_reduce_rows_f64", src.data_ptr(), src.stride(0), out.data_ptr(), out.stride(0), n_out, n_red, stride_out,
          stride_red, W, 0, _stream())
    return out


# float64 attention of DOSTransformer_phonon (csrc/f64_attention.hip)
ATTN64_MAX_H = _abi.DOSX_ATTN64_MAX_H
ATTN64_SOFTMAX_F64 = _abi.DOSX_ATTN64_SOFTMAX_F64


def _attn64_desc(q, kvhat, gamma0, beta0, Sq: int, Bq: int, Nk: int, Bk: int, mask, softmax64: bool,
                 key_ptr=None) -> _lib.Attn64:
    _chk_c64(q, kvhat, gamma0, beta0)
    H = q.shape[1]
    if not (1 <= H <= ATTN64_MAX_H) or Sq < 1 or Nk < 1 or Bk < 1 or Bq % Bk:
        raise ValueError(f"attention64: Sq={Sq} Bq={Bq} Nk={Nk} Bk={Bk} H={H}")
    if q.shape[0] != Bq * Sq or tuple(kvhat.shape) != (Bk * Nk, H) or gamma0.numel() != H or beta0.numel() != H:
        raise ValueError(f"attention64: q {tuple(q.shape)}, kvhat {tuple(kvhat.shape)} for Sq={Sq} Bq={Bq} Nk={Nk} Bk={Bk}")
    if mask is not None and (mask.dtype != torch.float32 or not mask.is_contiguous() or tuple(mask.shape) != (Bq, Sq, Nk)):
        raise ValueError(f"attention64: the dropout mask must be a contiguous float32 [Bq, Sq, Nk] tensor")
    if key_ptr is not None and (not isinstance(key_ptr, torch.Tensor) or key_ptr.dtype != torch.int32 or
                                key_ptr.device != q.device or not key_ptr.is_contiguous() or key_ptr.numel() != Bk + 1):
        raise ValueError(f"attention64: key_ptr must be a contiguous int32 tensor of Bk + 1 = {Bk + 1} entries on {q.device}")
    d = _lib.Attn64()
    d.Sq, d.Bq, d.Nk, d.Bk, d.H = Sq, Bq, Nk, Bk, H
    d.flags = ATTN64_SOFTMAX_F64 if softmax64 else 0
    d.q, d.kvhat, d.gamma0, d.beta0, d.drop_mask = q.data_ptr(), kvhat.data_ptr(), gamma0.data_ptr(), beta0.data_ptr(), _p(mask)
    d.key_ptr = _p(key_ptr)
    return d


def attention64(q: torch.Tensor, x: torch.Tensor, kvhat: torch.Tensor, gamma0, beta0, Sq: int, Bq: int, Nk: int, Bk: int,
                mask: Optional[torch.Tensor] = None, softmax64: bool = False, key_ptr: Optional[torch.Tensor] = None):
    """(out, probs): out = x + (softmax(q k^T / sqrt(H)) o mask) v with k = v = kvhat * gamma0 + beta0 (include/dosx.h:
    DosxAttn64 for the row layouts); probs [Bq, Sq, Nk] the un-dropped probabilities the backward reads.  key_ptr (int32
    [Bk + 1] on the device): key crystal bk has key_ptr[bk+1] - key_ptr[bk] keys, the rows past them take no part and get
    probability exactly 0."""
    d = _attn64_desc(q, kvhat, gamma0, beta0, Sq, Bq, Nk, Bk, mask, softmax64, key_ptr)
    _chk_c64(x)
    assert x.shape == q.shape
    out, probs = alloc64(q.device, *q.shape), alloc64(q.device, Bq, Sq, Nk)
    d.x, d.out, d.probs = x.data_ptr(), out.data_ptr(), probs.data_ptr()
    _call("dosx_attention_f64", C.byref(d), _stream())
    return out, probs


def attention_bwd64(dout: torch.Tensor, q: torch.Tensor, kvhat: torch.Tensor, gamma0, beta0, probs: torch.Tensor, Sq: int, Bq: int,
                    Nk: int, Bk: int, dkvhat: torch.Tensor, mask: Optional[torch.Tensor] = None, softmax64: bool = False,
                    accumulate: bool = False, key_ptr: Optional[torch.Tensor] = None):
    """(dq [Bq*Sq, H], part [Bk*Nk, 2H], ds [Bq, Sq, Nk]); dkvhat (+)= the key + value gradient times gamma0.  Column sums
    of part are the key side's dgamma0 | dbeta0; ds is the gradient of the scaled scores.  key_ptr as in attention64: ds and
    part are zero past a crystal's keys, dkvhat too unless accumulate (then those rows are left alone)."""
    d = _attn64_desc(q, kvhat, gamma0, beta0, Sq, Bq, Nk, Bk, mask, softmax64, key_ptr)
    _chk_c64(dout, probs, dkvhat)
    assert dout.shape == q.shape and dkvhat.shape == kvhat.shape and tuple(probs.shape) == (Bq, Sq, Nk)
    H = q.shape[1]
    dq, ds, part = alloc64(q.device, *q.shape), alloc64(q.device, Bq, Sq, Nk), alloc64(q.device, Bk * Nk, 2 * H)
    d.probs, d.dout, d.dq, d.ds = probs.data_ptr(), dout.data_ptr(), dq.data_ptr(), ds.data_ptr()
    d.dkvhat, d.part, d.accumulate = dkvhat.data_ptr(), part.data_ptr(), int(accumulate)
    _call("dosx_attention_bwd_f64", C.byref(d), _stream())
    return dq, part, ds


def dense_rows64(x: torch.Tensor, graph_ptr: torch.Tensor, B: int, nmax: int):
    """(rows [B*nmax, H], rstd [N]): the normalised (no affine) rows of to_dense_batch(x), zero rows for the padding."""
    _chk_c64(x)
    assert graph_ptr.dtype == torch.int32 and graph_ptr.numel() >= B + 1
    N, H = x.shape
    out, rstd = alloc64(x.device, B * nmax, H), alloc64(x.device, N)
    _call("dosx_dense_rows_f64", x.data_ptr(), graph_ptr.data_ptr(), out.data_ptr(), rstd.data_ptr(), B, nmax, H, _stream())
    return out, rstd


def dense_rows_bwd64(dout: torch.Tensor, xhat: torch.Tensor, rstd: torch.Tensor, graph_ptr: torch.Tensor, dx: torch.Tensor,
                     B: int, nmax: int, accumulate: bool = True) -> torch.Tensor:
    """dx[n] (+)= the LayerNorm (no affine) backward of node n's dense row; padding rows reach nothing."""
    _chk_c64(dout, xhat, rstd, dx)
    assert graph_ptr.dtype == torch.int32 and dout.shape == xhat.shape and dout.shape[0] == B * nmax
    _call("dosx_dense_rows_bwd_f64", dout.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), graph_ptr.data_ptr(), dx.data_ptr(), B,
          nmax, dx.shape[1], int(accumulate), _stream())
    return dx


def index_sum64(src: torch.Tensor, idx: torch.Tensor, out: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    """out[i] (+)= sum of the rows r of src with idx[r] == i, in order of r (fixed order: no atomics)."""
    _chk_f64(src, out)
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == src.shape[0] and out.shape[1] == src.shape[1]
    _call("dosx_index_sum_f64", src.data_ptr(), src.stride(0), idx.data_ptr(), src.shape[0], out.data_ptr(), out.stride(0),
          out.shape[0], src.shape[1], int(accumulate), _stream())
    return out


# float64 training step (csrc/f64_train.hip, csrc/adamw.hip), used by train64.Trainer64
def loss_phonon64(pg: torch.Tensor, ps: torch.Tensor, y: torch.Tensor, beta: float, dpg: torch.Tensor, dps: torch.Tensor,
                  loss: torch.Tensor, sse: Optional[torch.Tensor] = None) -> None:
    """loss[0] = rmse(pg, y) + beta rmse(ps, y) over all elements, dpg / dps its gradient, sse (optional, 2 elements) the two sums
    of squares (include/dosx.h: dosx_loss_phonon_f64).  An RMSE of exactly 0 gives a zero gradient."""
    _chk_c64(pg, ps, y, dpg, dps, loss, sse)
    count = pg.numel()
    if not (ps.numel() == y.numel() == dpg.numel() == dps.numel() == count) or loss.numel() < 1 or \
            (sse is not None and sse.numel() < 2):
        raise ValueError(f"loss_phonon64: pg {tuple(pg.shape)}, ps {tuple(ps.shape)}, y {tuple(y.shape)}, dpg {tuple(dpg.shape)}, "
                         f"dps {tuple(dps.shape)}, loss {tuple(loss.shape)}" + ("" if sse is None else f", sse {tuple(sse.shape)}"))
    _call("dosx_loss_phonon_f64", pg.data_ptr(), ps.data_ptr(), y.data_ptr(), float(beta), dpg.data_ptr(), dps.data_ptr(),
          loss.data_ptr(), _p(sse), count, _stream())


def loss_rows64(pg: torch.Tensor, ps: Optional[torch.Tensor], y: torch.Tensor, kind, *, clamp_target: bool = False,
                beta: float = 1.0, delta: Optional[float] = None, dpg: torch.Tensor, dps: Optional[torch.Tensor] = None,
                per_crystal: Optional[torch.Tensor] = None, loss: torch.Tensor, B_global: Optional[int] = None,
                weights: Optional[torch.Tensor] = None, weight_index: Optional[torch.Tensor] = None,
                bin_weights: Optional[torch.Tensor] = None, functionals: Optional[torch.Tensor] = None,
                functional_kind="sq", functional_weight: float = 1.0, functional_denominator: Optional[torch.Tensor] = None,
                functional_norm_rows: int = 0, functional_floor: Optional[float] = None) -> None:
    """:func:`loss_rows` on float64 operands (include/dosx.h: dosx_loss_rows_f64 / dosx_loss_rows_w_f64 / dosx_loss_rows_fn_f64 /
    dosx_loss_rows_fn_norm_f64)."""
    _loss_rows("loss_rows64", torch.float64, pg, ps, y, kind, clamp_target, beta, delta, dpg, dps, per_crystal, loss, B_global,
               weights, weight_index, bin_weights, functionals, functional_kind, functional_weight, functional_denominator,
               functional_norm_rows, functional_floor)


def grad_accumulate64(dst: torch.Tensor, a: torch.Tensor, b: Optional[torch.Tensor] = None, n: Optional[int] = None, *,
                      sdst: Optional[torch.Tensor] = None, sa: Optional[torch.Tensor] = None,
                      sb: Optional[torch.Tensor] = None) -> None:
    """:func:`grad_accumulate` on float64 operands (include/dosx.h: dosx_grad_accumulate_f64)."""
    _grad_accumulate("grad_accumulate64", torch.float64, dst, a, b, n, sdst, sa, sb)


def adamw64(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, n: int, lr: float, beta1: float, beta2: float,
            eps: float, weight_decay: float, step: int, ema=None) -> None:
    """torch.optim.AdamW's update of the first n elements of the flat fp64 buffers (include/dosx.h: dosx_adamw_f64).
    ``ema``: as on :func:`adamw`, here and on the three functions below."""
    _adamw("adamw64", torch.float64, p, g, m, v, n, beta1, beta2, eps, lr, weight_decay, step, ema=ema)


def adamw64_guarded(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, n: int, lr: float, beta1: float,
                    beta2: float, eps: float, weight_decay: float, rec: torch.Tensor, step=None, ema=None) -> None:
    """:func:`adamw64` behind :func:`grad_guard`: skip, clip coefficient and bias correction come from the record.  ``step``
    (the attempt count the guard was given) is read with ``ema`` only."""
    _adamw("adamw64_guarded", torch.float64, p, g, m, v, n, beta1, beta2, eps, lr, weight_decay, step=step if ema is not None else None,
           rec=rec, ema=ema)


def adamw64_grouped(p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step, ema=None) -> None:
    """:func:`adamw64` with parameter groups (see :func:`adamw_grouped`): bit for bit :func:`adamw64` on every run of chunks of
    one group with that group's ``(lr, weight_decay)``."""
    _adamw("adamw64_grouped", torch.float64, p, g, m, v, n, beta1, beta2, eps, step=step, chunk_group=chunk_group, groups=groups,
           ema=ema)


def adamw64_grouped_guarded(p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step, rec, ema=None) -> None:
    """:func:`adamw64_grouped` behind :func:`grad_guard` (see :func:`adamw_grouped_guarded`)."""
    _adamw("adamw64_grouped_guarded", torch.float64, p, g, m, v, n, beta1, beta2, eps, step=step, chunk_group=chunk_group,
           groups=groups, rec=rec, ema=ema)


# float64 pair head of Graphnetwork_phonon (csrc/pair_head_f64.hip), used by functional64's factored program
def _pair_head_desc64(who: str, e1, c, w2, slope: float):
    """The operands both float64 pair-head launches read: e1 [S,H], c [B,H], w2 [H] (or [1,H], nn.Linear(H, 1).weight)."""
    _chk_c64(e1, c, w2)
    if e1.dim() != 2 or c.dim() != 2 or e1.shape[1] != c.shape[1] or w2.numel() != e1.shape[1]:
        raise ValueError(f"{who}: e1 [S,H], c [B,H], w2 [H], got {tuple(e1.shape)}, {tuple(c.shape)}, {tuple(w2.shape)}")
    d = _lib.PairHead64()
    d.S, d.B, d.H, d.slope = int(e1.shape[0]), int(c.shape[0]), int(e1.shape[1]), float(slope)
    d.e1, d.c, d.w2 = e1.data_ptr(), c.data_ptr(), w2.data_ptr()
    return d


def pair_head_fwd64(e1, c, w2, b2, dos, slope: float = 0.01) -> None:
    """dos[b, s] = b2 + sum_h w2[h] * leaky(e1[s, h] + c[b, h]) in float64, one launch (include/dosx.h: DosxPairHead64); dos: [B,S]."""
    d = _pair_head_desc64("pair_head_fwd64", e1, c, w2, slope)
    _chk_c64(b2, dos)
    if tuple(dos.shape) != (d.B, d.S) or b2.numel() != 1:
        raise ValueError(f"pair_head_fwd64: dos must be a contiguous [B,S] = [{d.B},{d.S}] and b2 one element, got "
                         f"{tuple(dos.shape)}, {tuple(b2.shape)}")
    d.b2, d.dos = b2.data_ptr(), dos.data_ptr()
    _call("dosx_pair_head_fwd_f64", C.byref(d), _stream())


def pair_head_bwd64(ddos, e1, c, w2, de1, dc, partials, slope: float = 0.01) -> None:
    """The backward of pair_head_fwd64 from ddos [B,S] in one launch: de1 [S,H], dc [B,H] and ``partials``
    [pair_head_partial_rows(S, B), H + 1] whose column sums (colsum64) are dw2 (H) and db2."""
    d = _pair_head_desc64("pair_head_bwd64", e1, c, w2, slope)
    _chk_c64(ddos, de1, dc, partials)
    rows = pair_head_partial_rows(d.S, d.B)
    if not (tuple(ddos.shape) == (d.B, d.S) and de1.shape == e1.shape and dc.shape == c.shape
            and tuple(partials.shape) == (rows, d.H + 1)):
        raise ValueError(f"pair_head_bwd64: contiguous ddos [B,S], de1 [S,H], dc [B,H], partials [{rows},H+1] wanted, got "
                         f"{tuple(ddos.shape)}, {tuple(de1.shape)}, {tuple(dc.shape)}, {tuple(partials.shape)}")
    d.ddos, d.de1, d.dc, d.partials = ddos.data_ptr(), de1.data_ptr(), dc.data_ptr(), partials.data_ptr()
    _call("dosx_pair_head_bwd_f64", C.byref(d), _stream())
