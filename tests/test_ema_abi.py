"""CPU-only checks of the C boundary of the weight average (include/dosx.h: DosxAdamWEma, dosx_adamw_ema / _f64,
dosx_adamw_ema_decay, dosx_swap_buffers): the descriptor's layout against a gcc probe of the real header, the generated argument
types, the refusals that stand in front of every launch, and the decay schedule against a Python twin.  No compute calls."""
import ctypes as C
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dosx_adamw_ema", "dosx_adamw_ema_f64")
SYMBOLS = ENTRIES + ("dosx_swap_buffers", "dosx_adamw_ema_decay")


def test_symbols_are_declared_exported_and_generated():
    from dostransformer_amd import _abi, _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    P, I64, I, D, F, G, E = C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_float, C.POINTER(_abi.AdamWGroups), C.POINTER(_abi.AdamWEma)
    want = {"dosx_adamw_ema": [P, P, P, P, I64, F, F, F, F, F, I, F, P, G, P, E, P],
            "dosx_adamw_ema_f64": [P, P, P, P, I64, D, D, D, D, D, I, P, G, P, E, P],
            "dosx_swap_buffers": [P, P, I64, P],
            "dosx_adamw_ema_decay": [D, I, I, I]}
    for name in SYMBOLS:
        assert f"{name}(" in header and name in _lib.EXPORTS and name in _abi.SIGS, name
        fn = getattr(lib, name)                                     # (AttributeError: not exported)
        assert fn.argtypes == _abi.SIGS[name] == want[name], name
    assert lib.dosx_adamw_ema_decay.restype is C.c_double and _abi.RESTYPES["dosx_adamw_ema_decay"] is C.c_double
    for name in ENTRIES + ("dosx_swap_buffers",):
        assert getattr(lib, name).restype is C.c_int
    # the eight entries without an average keep their signatures
    assert lib.dosx_adamw.argtypes == [P, P, P, P, I64, F, F, F, F, F, I, F, P]
    assert lib.dosx_adamw_grouped_guarded_f64.argtypes == [P, P, P, P, I64, P, G, D, D, D, I, P, P]
    assert (_abi.DOSX_SWAP_THREADS, _abi.DOSX_SWAP_MAX_BLOCKS) == (256, 2048)


def test_descriptor_matches_the_c_layout(tmp_path):
    from dostransformer_amd import _abi
    fields = ["ema", "decay", "warmup", "t0"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dosx.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(DosxAdamWEma));']
    lines += [f'  printf("%zu %zu\\n", offsetof(DosxAdamWEma, {f}), sizeof(((DosxAdamWEma*)0)->{f}));' for f in fields]
    probe, exe = tmp_path / "probe.c", tmp_path / "probe"
    probe.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    cls = _abi.AdamWEma
    assert [f for f, _ in cls._fields_] == fields and C.sizeof(cls) == int(out[0]) == 24
    for f, line in zip(fields, out[1:]):
        d = getattr(cls, f)
        assert [d.offset, d.size] == [int(v) for v in line.split()], f
    types = dict(cls._fields_)
    assert types["ema"] is C.c_void_p and types["decay"] is C.c_double and types["warmup"]._type_ == "i" and types["t0"]._type_ == "i"


A, B, D, E, M, R, X = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000     # 16-byte aligned fake device addresses


@pytest.mark.parametrize("form", ["plain", "guarded", "grouped", "grouped_guarded"])
@pytest.mark.parametrize("name", ENTRIES)
def test_ema_entries_validate_before_any_launch(name, form):
    """Everything the form without an average refuses, and the average's own refusals, through DOSX_CHECK_ARG: rc -22 and a
    message naming the entry point.  n = 0 returns 0 behind the checks.  The addresses here are never dereferenced."""
    from dostransformer_amd import _abi, _lib
    lib = _lib.load()
    fn, who, f64 = getattr(lib, name), name.encode(), name.endswith("f64")
    grouped, guarded = "grouped" in form, "guarded" in form

    def groups(n=2, lr=(1e-3, 1e-4), wd=(1e-2, 0.0)):
        st = _abi.AdamWGroups()
        st.n_groups = n
        for k, (a, b) in enumerate(zip(lr, wd)):
            st.lr[k], st.weight_decay[k] = a, b
        return st

    def desc(ema=X, decay=0.999, warmup=1, t0=0):
        return _abi.AdamWEma(ema, decay, warmup, t0)

    def call(p=A, g=B, m=D, v=E, n=128, chunk="default", st="default", step=3, rec="default", e="default"):
        chunk = (M if grouped else None) if chunk == "default" else chunk
        st = (groups() if grouped else None) if st == "default" else st
        rec = (R if guarded else None) if rec == "default" else rec
        e = desc() if e == "default" else e
        head = [p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step] + ([] if f64 else [1.0])
        return fn(*head, chunk, None if st is None else C.byref(st), rec, None if e is None else C.byref(e), None)

    def refused(rc, *msgs):
        assert rc == -22, rc
        for msg in (who,) + msgs:
            assert msg in lib.dosx_last_error(), lib.dosx_last_error()

    assert call(n=0) == 0                                                             # nothing to do
    # ---- what the form without an average refuses
    for k in "pgmv":
        refused(call(**{k: None}), b"NULL")
    refused(call(n=-64), b"n must not be negative", b"-64")
    refused(call(step=0), b"step is the 1-based", b"got 0")
    refused(call(step=-3), b"step is the 1-based", b"got -3")
    for k, base in zip("pgmv", (A, B, D, E)):
        refused(call(**{k: base + 8}), b"buffers must be 16-byte aligned")
    if guarded:
        refused(call(rec=R + 8), b"16-byte aligned")
    if grouped:
        refused(call(chunk=None), b"chunk map and groups go together")
        refused(call(st=None), b"chunk map and groups go together")
        for n in (1, 63, 130):
            refused(call(n=n), b"multiple of 64", str(n).encode())
        for n in (0, 17):
            refused(call(st=groups(n=n)), b"n_groups must be in [1, 16]", f"got {n}".encode())
        nan = float("nan")
        refused(call(st=groups(lr=(1e-3, nan))), b"lr[1]", b"nan")
        refused(call(st=groups(lr=(-1e-3, 1e-3))), b"lr[0]", b"-0.001")
        refused(call(st=groups(wd=(1e-2, nan))), b"weight_decay[1]", b"nan")
        refused(call(st=groups(wd=(1e-2, -0.5))), b"weight_decay[1]", b"-0.5")
    else:
        refused(call(chunk=M), b"chunk map and groups go together")
        refused(call(st=groups()), b"chunk map and groups go together")
        assert call(n=0, step=1) == 0 and call(n=0, chunk=None, st=None) == 0
    # ---- the average's own
    refused(call(e=None), b"NULL ema")
    refused(call(e=desc(ema=None)), b"NULL ema")
    refused(call(e=desc(ema=X + 8)), b"ema must be 16-byte aligned")
    refused(call(e=desc(ema=X + 4)), b"ema must be 16-byte aligned")
    refused(call(e=desc(ema=A)), b"ema must not alias p")
    refused(call(e=desc(ema=A), n=0), b"ema must not alias p")
    refused(call(e=desc(ema=A + 64)), b"ema must not alias p")                         # inside p[0, n)
    refused(call(e=desc(ema=A - 16)), b"ema must not alias p")                         # p inside ema[0, n)
    esize = 8 if f64 else 4
    assert call(e=desc(ema=A + 128 * esize), n=0) == 0                                 # right behind p[0, 128): no overlap ...
    refused(call(e=desc(ema=A + 128 * esize - 16)), b"ema must not alias p")           # ... one vector earlier: overlap
    for bad in (float("nan"), -0.1, 1.0, 1.5, float("inf")):
        refused(call(e=desc(decay=bad)), b"ema decay must be in [0, 1)")
    assert call(n=0, e=desc(decay=0.0)) == 0
    refused(call(e=desc(t0=-1)), b"ema t0", b"got -1")
    refused(call(e=desc(t0=3)), b"ema t0", b"got 3")                                   # t0 >= step
    refused(call(e=desc(t0=7)), b"ema t0", b"got 7")
    assert call(n=0, e=desc(t0=2)) == 0


def test_swap_buffers_validates_before_any_launch():
    from dostransformer_amd import _lib
    lib = _lib.load()
    fn = lib.dosx_swap_buffers

    def refused(rc, *msgs):
        assert rc == -22, rc
        for msg in (b"dosx_swap_buffers",) + msgs:
            assert msg in lib.dosx_last_error(), lib.dosx_last_error()

    assert fn(A, B, 0, None) == 0                                                     # nothing to do
    refused(fn(None, B, 16, None), b"NULL")
    refused(fn(A, None, 16, None), b"NULL")
    refused(fn(A, B, -16, None), b"multiple of 16", b"-16")
    for n in (1, 8, 24):
        refused(fn(A, B, n, None), b"multiple of 16", str(n).encode())
    refused(fn(A + 8, B, 16, None), b"16-byte aligned")
    refused(fn(A, B + 4, 16, None), b"16-byte aligned")
    refused(fn(A, A, 16, None), b"overlap")
    refused(fn(A, A + 16, 32, None), b"overlap")
    refused(fn(A + 16, A, 32, None), b"overlap")
    refused(fn(A, A, 0, None), b"overlap")


def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


@pytest.mark.parametrize("warmup", [False, True], ids=["fixed", "warmup"])
def test_decay_schedule_agrees_with_its_python_twin(warmup):
    """d_t = min(decay, (1 + t) / (10 + t)) under warm-up, else decay: evaluated in double, rounded once to the buffer's type.
    At decay = 0.999 the min switches between t = 8989 ((1 + t) / (10 + t) = 8990 / 8999 < 0.999) and 8990 (8991 / 9000 = 0.999)."""
    from dostransformer_amd import ema, ops
    import torch
    decay = 0.999
    assert (1 + 8989) / (10 + 8989) < decay <= (1 + 8990) / (10 + 8990)
    for t in (1, 9, 8989, 8990, 8991):
        twin = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
        assert ema.schedule(decay, warmup, t) == twin
        assert ops.ema_decay_at(decay, warmup, t, torch.float64) == twin, t
        assert ops.ema_decay_at(decay, warmup, t, torch.float32) == _f32(twin), t
        if warmup:
            assert (twin < decay) == (t <= 8989), t
    if warmup:
        assert ops.ema_decay_at(decay, True, 1, torch.float64) == 2.0 / 11.0
