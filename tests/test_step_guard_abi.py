"""CPU-only checks of the guarded optimizer step's C boundary (include/dosx.h: DosxStepGuard, dosx_grad_guard_f32 / _f64,
dosx_adamw_guarded / _f64, dosx_grad_guard_blocks, dosx_exchange_status_address): the record's layout against a gcc probe of the
real header, the argument types, and the refusals that stand in front of every launch.  No compute calls."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the record as the header declares it: (C type, field), in order
FIELDS = [("double", "sumsq"), ("double", "norm"), ("double", "clip"), ("double", "step_size"), ("double", "bc2_scale"),
          ("int64_t", "n_bad"), ("int64_t", "first_bad"), ("int64_t", "first_skip_bad"), ("int32_t", "skip"), ("int32_t", "reason"),
          ("int32_t", "t"), ("int32_t", "applied"), ("int32_t", "skipped"), ("int32_t", "first_skip_step"),
          ("int32_t", "first_skip_reason"), ("int32_t", "reserved")]


def test_step_guard_record_matches_the_c_layout(tmp_path):
    """Size and every offset of DosxStepGuard from a gcc probe of include/dosx.h; 96 bytes = six 16-byte rows, the doubles first
    (word 1 is `norm`: Trainer.grad_norm is a view of it), and the workspace constant is what the slab needs."""
    from dostransformer_amd import _abi, ops
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dosx.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(DosxStepGuard));']
    lines += [f'  printf("%zu %zu\\n", offsetof(DosxStepGuard, {f}), sizeof(((DosxStepGuard*)0)->{f}));' for _, f in FIELDS]
    probe, exe = tmp_path / "probe.c", tmp_path / "probe"
    probe.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    cls = _abi.StepGuard
    assert [f for f, _ in cls._fields_] == [f for _, f in FIELDS]
    assert C.sizeof(cls) == int(out[0]) == 96 and C.sizeof(cls) % 16 == 0
    sizes = {"double": 8, "int64_t": 8, "int32_t": 4}
    codes = {"double": "d", "int64_t": "lq", "int32_t": "i"}
    for (c_type, f), line, (_, ct) in zip(FIELDS, out[1:], cls._fields_):
        d = getattr(cls, f)
        assert [d.offset, d.size] == [int(v) for v in line.split()], f
        assert d.size == sizes[c_type] and ct._type_ in codes[c_type], (f, ct)
    assert cls.norm.offset == 8 and ops._GUARD_WORDS == 12
    assert _abi.DOSX_GUARD_WORKSPACE_BYTES == 64 + _abi.DOSX_GUARD_MAX_BLOCKS * 24 and _abi.DOSX_GUARD_WORKSPACE_BYTES % 16 == 0
    assert (_abi.DOSX_GUARD_NONFINITE, _abi.DOSX_GUARD_OVERFLOW, _abi.DOSX_GUARD_STALLED) == (1, 2, 4)
    assert _abi.DOSX_GUARD_THREADS == 256


def test_step_guard_argument_types():
    from dostransformer_amd import _lib
    lib = _lib.load()
    P, I64, I, D, F = C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_float
    assert lib.dosx_grad_guard_f32.argtypes == [P, I64, D, P, F, F, F, I, P, P, P]
    assert lib.dosx_grad_guard_f64.argtypes == [P, I64, D, P, D, D, D, I, P, P, P]
    assert lib.dosx_adamw_guarded.argtypes == [P, P, P, P, I64, F, F, F, F, F, P, P]
    assert lib.dosx_adamw_guarded_f64.argtypes == [P, P, P, P, I64, D, D, D, D, D, P, P]
    assert lib.dosx_grad_guard_blocks.argtypes == [I64, I] and lib.dosx_exchange_status_address.argtypes == [P]
    for name in ("dosx_grad_guard_f32", "dosx_grad_guard_f64", "dosx_adamw_guarded", "dosx_adamw_guarded_f64", "dosx_grad_guard_blocks",
                 "dosx_exchange_status_address"):
        assert getattr(lib, name).restype is C.c_int and name in _lib.EXPORTS
    # the four launches are replayable ops with their prototype's argument classes
    for name, ni, nf in (("dosx_grad_guard_f32", 7, 4), ("dosx_grad_guard_f64", 7, 4), ("dosx_adamw_guarded", 7, 5),
                         ("dosx_adamw_guarded_f64", 7, 5)):
        a, b = C.c_int(-1), C.c_int(-1)
        assert lib.dosx_replay_op(name.encode(), C.byref(a), C.byref(b)) >= 0 and (a.value, b.value) == (ni, nf), name


def test_grad_guard_grid_is_a_function_of_n_alone():
    """ceil(n / elements per 16 bytes / 256) workgroups, at least 1, at most DOSX_GUARD_MAX_BLOCKS."""
    from dostransformer_amd import _abi, _lib
    lib = _lib.load()
    cap, thr = _abi.DOSX_GUARD_MAX_BLOCKS, _abi.DOSX_GUARD_THREADS
    for size, per in ((4, 4), (8, 2)):
        for n in (0, 1, per - 1, per, per * thr, per * thr + per - 1, per * thr + per, 1000003, cap * thr * per - 1, cap * thr * per,
                  cap * thr * per + per, 3 * cap * thr * per, 2 ** 33):
            want = min(max(-(-(n // per) // thr), 1), cap)
            assert lib.dosx_grad_guard_blocks(n, size) == want, (n, size)
    assert lib.dosx_grad_guard_blocks(-1, 4) == -22 and lib.dosx_grad_guard_blocks(8, 2) == -22
    assert b"dosx_grad_guard_blocks" in lib.dosx_last_error()


def test_step_guard_entry_points_validate_before_any_launch():
    """NULL operands, a negative n, step < 1, a NaN max_norm and buffers off a 16-byte boundary are refused through
    DOSX_CHECK_ARG (rc -22 and a message naming the entry point); the addresses here are never dereferenced."""
    from dostransformer_amd import _lib
    lib = _lib.load()
    A, B, D, E, R, W = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000          # 16-byte aligned fake device addresses

    def refused(rc, msg):
        assert rc == -22, rc
        assert msg in lib.dosx_last_error(), lib.dosx_last_error()

    for name in ("dosx_grad_guard_f32", "dosx_grad_guard_f64"):
        fn, who = getattr(lib, name), name.encode()
        call = lambda g=A, n=8, mx=1.0, st=None, step=1, rec=R, ws=W: fn(g, n, mx, st, 1e-3, 0.9, 0.999, step, rec, ws, None)
        refused(call(g=None), who + b": NULL")
        refused(call(rec=None), who + b": NULL")
        refused(call(ws=None), who + b": NULL")
        refused(call(n=-1), who + b": n must not be negative")
        refused(call(step=0), who + b": step is the 1-based attempt count")
        refused(call(step=-7), who + b": step is the 1-based attempt count")
        refused(call(mx=float("nan")), who + b": max_norm is NaN")
        refused(call(g=A + 4 if "f32" in name else A + 8), who + b": buffers must be 16-byte aligned")
        refused(call(rec=R + 8), who + b": buffers must be 16-byte aligned")
        refused(call(ws=W + 8), who + b": buffers must be 16-byte aligned")
        refused(call(st=B + 2), who + b": exchange_status must be 4-byte aligned")
    for name in ("dosx_adamw_guarded", "dosx_adamw_guarded_f64"):
        fn, who = getattr(lib, name), name.encode()
        call = lambda p=A, g=B, m=D, v=E, n=8, rec=R: fn(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, rec, None)
        assert call(n=0) == 0                                                            # nothing to do
        for k in "pgmv":
            refused(call(**{k: None}), who + b": NULL buffer or record")
        refused(call(rec=None), who + b": NULL buffer or record")
        refused(call(n=-2), who + b": n must not be negative")
        for k, base in zip("pgmv", (A, B, D, E)):
            refused(call(**{k: base + 8}), who + b": buffers must be 16-byte aligned")
        refused(call(rec=R + 8), who + b": buffers must be 16-byte aligned")
    refused(lib.dosx_exchange_status_address(None), b"dosx_exchange_status_address: null output")


def test_trainers_refuse_bad_guard_arguments_without_a_gpu():
    """A negative or NaN max_grad_norm is a ValueError at construction, on every trainer; the default is no guard."""
    import pytest
    import torch
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.guard import StepGuard, locate, reason_names
    from dostransformer_amd.train import Trainer
    model = DOSTransformer_phonon(2, 2, 118, 4, 32, "cpu", 0.0)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            Trainer(model, max_grad_norm=bad)
    tr = Trainer(model)
    assert not tr.guarded and tr.max_grad_norm is None and tr.skip_nonfinite is False and isinstance(tr, StepGuard)
    assert Trainer(model, max_grad_norm=0.5).guarded and Trainer(model, skip_nonfinite=True).guarded
    assert reason_names(5) == ("non-finite gradient", "exchange stalled") and reason_names(0) == ()

    class FP:
        names, offsets = ["a", "b"], [0, 8]
        P = {"a": torch.zeros(2, 3), "b": torch.zeros(5)}
    assert locate(FP, -1) is None and locate(FP, 5) == ("a", 5) and locate(FP, 6) == (None, 6) and locate(FP, 12) == ("b", 4)
