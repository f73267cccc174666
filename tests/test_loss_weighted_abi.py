"""CPU-only checks of the weighted per-crystal loss entries (csrc/loss_rows.hip: dosx_loss_rows_w / dosx_loss_rows_w_f64):
declared, exported, replayable, prototyped from the header with their scalars in the operands' type and the three further
pointers (w, w_index, bin_w) behind ``loss``; every refusal of include/dosx.h comes back as -22 with a message that names the
entry, before any launch - what dosx_loss_rows refuses (tests/test_loss_rows_abi.py), w_index without w, and w or bin_w lying
inside one of the [B,S] operands."""
import ctypes as C
import math
import os

import pytest

from tests.util import dosx_lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"dosx_loss_rows_w": (C.c_float, "dosx_loss_rows", 4), "dosx_loss_rows_w_f64": (C.c_double, "dosx_loss_rows_f64", 8)}
B, S = 5, 51
# never dereferenced: every call below is refused before any launch.  The five [B,S] operands one page apart, w / w_index /
# bin_w far from them and from each other.
PG, PS, Y, DPG, DPS, PER, LOSS = (1 << 20) * 1, (1 << 20) * 2, (1 << 20) * 3, (1 << 20) * 4, (1 << 20) * 5, (1 << 20) * 6, (1 << 20) * 7
W, WI, BW = (1 << 20) * 8, (1 << 20) * 9, (1 << 20) * 10


def test_weighted_symbols_declared_exported_replayable_and_prototyped():
    _l = _lib()
    lib = _l.load()
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    for n, (scalar, plain, _) in SYMBOLS.items():
        assert f"int {n}(" in header, n
        assert hasattr(lib, n), n
        ni, nf = C.c_int(0), C.c_int(0)
        assert lib.dosx_replay_op(n.encode(), C.byref(ni), C.byref(nf)) >= 0, n
        args = getattr(lib, n).argtypes
        assert len(args) == 18 and len(args) == ni.value + nf.value, n
        other = C.c_double if scalar is C.c_float else C.c_float
        sig = _l._SIGS[n]
        assert sig.count(scalar) == 2 == nf.value and sig.count(other) == 0, n                    # beta, delta
        assert sig.count(C.c_int) == 5, n                                                         # B, S, B_global, kind, clamp_target
        # the unweighted entry's arguments, then w, w_index, bin_w, then the stream
        assert list(sig[:14]) == list(_l._SIGS[plain][:14]), n
        assert list(sig[14:]) == [C.c_void_p] * 4, n


@pytest.mark.parametrize("name", list(SYMBOLS))
def test_weighted_argument_validation_needs_no_gpu(name):
    lib = _lib().load()
    err = lambda: lib.dosx_last_error().decode()
    fn = getattr(lib, name)
    esize = SYMBOLS[name][2]
    # pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps, per_crystal, loss, w, w_index, bin_w
    ok = [PG, PS, Y, B, S, B, 0, 0, 1.0, 0.0, DPG, DPS, PER, LOSS, W, WI, BW]
    call = lambda a: fn(*a, None)

    def refused(a, *words):
        assert call(a) == -22, a
        e = err()
        assert e.startswith(name + ":") and all(w in e for w in words), e

    # ---- everything dosx_loss_rows refuses, with every combination of the three pointers ------------------------------------
    for extra in ((W, WI, BW), (W, None, None), (None, None, BW), (None, None, None)):
        base = ok[:14] + list(extra)
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
    # ---- w_index without w ---------------------------------------------------------------------------------------------------
    for bw in (BW, None):
        a = list(ok)
        a[14], a[16] = None, bw
        refused(a, "w_index", "NULL")
    # ---- w or bin_w inside a [B,S] operand: at its first, a middle and its last element ----------------------------------------
    n = B * S
    for op in (PG, PS, Y, DPG, DPS):
        for i, word in ((14, "w"), (16, "bin_w")):
            for off in (0, (n // 2) * esize, (n - 1) * esize):
                a = list(ok)
                a[i] = op + off
                refused(a, word, "inside")
            # a vector that starts in front of the operand and ENDS inside it (w ungathered: B entries; bin_w: S entries)
            a = list(ok)
            a[i], a[15] = op - esize, None
            refused(a, word, "inside")
