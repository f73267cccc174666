"""CPU-only checks of the entries of csrc/loss_functional.hip (dosx_loss_rows_fn / _fn_f64, dosx_eval_functionals / _f64):
declared, exported, replayable, prototyped from the header - the weighted loss entry's arguments, then fn_w, K, fn_kind, lam in
the operands' type, then the stream -; every refusal of include/dosx.h comes back as -22 with a message that starts with the
entry's name, before any launch: what dosx_loss_rows_w refuses (tests/test_loss_weighted_abi.py), K outside 1 .. 512 and S > 512
with a table, fn_kind outside the enumerators, lam negative or not finite, and fn_w lying inside one of the [B,S] operands."""
import ctypes as C
import math
import os

import pytest

from tests.util import dosx_lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS = {"dosx_loss_rows_fn": (C.c_float, "dosx_loss_rows_w", 4), "dosx_loss_rows_fn_f64": (C.c_double, "dosx_loss_rows_w_f64", 8)}
EVAL = {"dosx_eval_functionals": 4, "dosx_eval_functionals_f64": 8}
B, S, K = 5, 51, 7
# never dereferenced: every call below is refused before any launch.  The operands 1 MiB apart.
PG, PS, Y, DPG, DPS, PER, LOSSP, W, WI, BW, FN = ((1 << 20) * i for i in range(1, 12))


def test_functional_symbols_declared_exported_replayable_and_prototyped():
    _l = _lib()
    lib = _l.load()
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    assert "enum { DOSX_FN_SQ = 0, DOSX_FN_ABS = 1 };" in header
    from dostransformer_amd import _abi
    assert (_abi.DOSX_FN_SQ, _abi.DOSX_FN_ABS) == (0, 1)
    for n, (scalar, weighted, _) in LOSS.items():
        assert f"int {n}(" in header, n
        assert hasattr(lib, n), n
        ni, nf = C.c_int(0), C.c_int(0)
        assert lib.dosx_replay_op(n.encode(), C.byref(ni), C.byref(nf)) >= 0, n
        args = getattr(lib, n).argtypes
        assert len(args) == 22 and len(args) == ni.value + nf.value, n
        other = C.c_double if scalar is C.c_float else C.c_float
        sig = _l._SIGS[n]
        assert sig.count(scalar) == 3 == nf.value and sig.count(other) == 0, n                    # beta, delta, lam
        assert sig.count(C.c_int) == 7, n                                          # B, S, B_global, kind, clamp_target, K, fn_kind
        # every argument of the weighted entry up to bin_w, then fn_w, K, fn_kind, lam, then the stream
        assert list(sig[:17]) == list(_l._SIGS[weighted][:17]), n
        assert list(sig[17:]) == [C.c_void_p, C.c_int, C.c_int, scalar, C.c_void_p], n
    for n in EVAL:
        assert f"int {n}(" in header, n
        assert hasattr(lib, n), n
        ni, nf = C.c_int(0), C.c_int(0)
        assert lib.dosx_replay_op(n.encode(), C.byref(ni), C.byref(nf)) >= 0, n
        sig = _l._SIGS[n]
        assert len(sig) == 9 == ni.value and nf.value == 0, n
        assert list(sig) == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p], n


@pytest.mark.parametrize("name", list(LOSS))
def test_functional_loss_argument_validation_needs_no_gpu(name):
    lib = _lib().load()
    err = lambda: lib.dosx_last_error().decode()
    fn = getattr(lib, name)
    esize = LOSS[name][2]
    # 0 pg, 1 ps, 2 y, 3 B, 4 S, 5 B_global, 6 kind, 7 clamp_target, 8 beta, 9 delta, 10 dpg, 11 dps, 12 per_crystal, 13 loss,
    # 14 w, 15 w_index, 16 bin_w, 17 fn_w, 18 K, 19 fn_kind, 20 lam
    ok = [PG, PS, Y, B, S, B, 0, 0, 1.0, 0.0, DPG, DPS, PER, LOSSP, W, WI, BW, FN, K, 0, 0.5]
    call = lambda a: fn(*a, None)

    def refused(a, *words):
        assert call(a) == -22, a
        e = err()
        assert e.startswith(name + ":") and all(w in e for w in words), e

    # ---- everything dosx_loss_rows_w refuses: with a table, without one, and with lam == 0 --------------------------------------
    for tail in ((FN, K, 0, 0.5), (FN, K, 1, 0.5), (None, 0, 0, 0.5), (FN, K, 0, 0.0)):
        for extra in ((W, WI, BW), (W, None, None), (None, None, BW), (None, None, None)):
            base = ok[:14] + list(extra) + list(tail)
            for i in (0, 2, 10, 13):                      # pg, y, dpg, loss
                a = list(base)
                a[i] = None
                refused(a, "NULL")
            for i in (1, 11):                             # ps without dps, dps without ps
                a = list(base)
                a[i] = None
                refused(a, "ps", "dps")
            for i, word in ((3, "B="), (4, "S="), (5, "B_global=")):
                for v in (0, -3):
                    a = list(base)
                    a[i] = v
                    refused(a, word + str(v))
            for kind in (-1, 4, 17):
                a = list(base)
                a[6] = kind
                refused(a, "kind=" + str(kind))
            for delta in (0.0, -0.25, math.inf, math.nan):
                a = list(base)
                a[6], a[9] = 3, delta
                refused(a, "HUBER", "delta")
            a = list(base)
            a[3], a[4], a[5] = 1 << 16, 1 << 15, 1 << 16  # B * S = 2^31
            refused(a, "2^31", str(1 << 31))
        for bw in (BW, None):                             # w_index without w
            a = ok[:17] + list(tail)
            a[14], a[16] = None, bw
            refused(a, "w_index", "NULL")
        n = B * S
        for op in (PG, PS, Y, DPG, DPS):                  # w or bin_w inside a [B,S] operand
            for i, word in ((14, "w"), (16, "bin_w")):
                for off in (0, (n // 2) * esize, (n - 1) * esize):
                    a = ok[:17] + list(tail)
                    a[i] = op + off
                    refused(a, word, "inside")
                a = ok[:17] + list(tail)
                a[i], a[15] = op - esize, None
                refused(a, word, "inside")
    # ---- K outside 1 .. 512 and S > 512, with a table ---------------------------------------------------------------------------
    for k in (0, -1, 513, 1 << 20):
        a = list(ok)
        a[18] = k
        refused(a, "K=" + str(k))
    for s in (513, 1024):
        a = list(ok)
        a[4] = s
        refused(a, "S=" + str(s))
    # ---- fn_kind outside the enumerators (with and without a table) ----------------------------------------------------------
    for kind in (-1, 2, 9):
        for table in (FN, None):
            a = list(ok)
            a[17], a[19] = table, kind
            refused(a, "fn_kind=" + str(kind))
    # ---- lam negative or not finite ---------------------------------------------------------------------------------------------
    for lam in (-1e-3, -math.inf, math.inf, math.nan):
        for table in (FN, None):
            a = list(ok)
            a[17], a[20] = table, lam
            refused(a, "lam")
    # ---- fn_w inside a [B,S] operand: at its first, a middle and its last element, and a table that ENDS inside it ---------------
    n = B * S
    for op in (PG, PS, Y, DPG, DPS):
        for off in (0, (n // 2) * esize, (n - 1) * esize, -(K * S - 1) * esize):
            a = list(ok)
            a[17] = op + off
            refused(a, "fn_w", "inside")
    # (one output: ps and dps both NULL - their addresses are then not operands)
    a = list(ok)
    a[1] = a[11] = None
    a[17] = PG + esize
    refused(a, "fn_w", "inside")


@pytest.mark.parametrize("name", list(EVAL))
def test_eval_functionals_argument_validation_needs_no_gpu(name):
    lib = _lib().load()
    err = lambda: lib.dosx_last_error().decode()
    fn = getattr(lib, name)
    # pred, y, B, S, scale, fn_w, K, out
    ok = [PG, Y, B, S, W, FN, K, DPG]

    def refused(a, *words):
        assert fn(*a, None) == -22, a
        e = err()
        assert e.startswith(name + ":") and all(w in e for w in words), e

    for i, word in ((2, "B=-1"), (3, "S=0"), (6, "K=0")):
        a = list(ok)
        a[i] = int(word.split("=")[1])
        refused(a, word)
    for i in (0, 1, 5, 7):
        a = list(ok)
        a[i] = None
        refused(a, "NULL")
    a = list(ok)
    a[2] = 0                                  # B = 0: a no-op, whatever the pointers are
    a[0] = a[1] = a[5] = a[7] = None
    assert fn(*a, None) == 0
