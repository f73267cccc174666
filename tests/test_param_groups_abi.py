"""CPU-only checks of the grouped AdamW's C boundary (include/dosx.h: DosxAdamWGroups, dosx_adamw_grouped / _f64 /
_guarded / _guarded_f64): the host struct's layout against a gcc probe of the real header, the generated argument types, and the
refusals that stand in front of every launch.  No compute calls."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dosx_adamw_grouped", "dosx_adamw_grouped_f64", "dosx_adamw_grouped_guarded", "dosx_adamw_grouped_guarded_f64")


def test_groups_struct_matches_the_c_layout(tmp_path):
    """Size and every offset of DosxAdamWGroups from a gcc probe of include/dosx.h; both arrays hold DOSX_ADAMW_MAX_GROUPS doubles."""
    from dostransformer_amd import _abi
    fields = ["n_groups", "reserved", "lr", "weight_decay"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dosx.h"', "int main(void) {",
             '  printf("%zu %d %d\\n", sizeof(DosxAdamWGroups), DOSX_ADAMW_MAX_GROUPS, DOSX_ADAMW_GROUP_CHUNK);']
    lines += [f'  printf("%zu %zu\\n", offsetof(DosxAdamWGroups, {f}), sizeof(((DosxAdamWGroups*)0)->{f}));' for f in fields]
    probe, exe = tmp_path / "probe.c", tmp_path / "probe"
    probe.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    cls = _abi.AdamWGroups
    size, max_groups, chunk = (int(v) for v in out[0].split())
    assert (max_groups, chunk) == (_abi.DOSX_ADAMW_MAX_GROUPS, _abi.DOSX_ADAMW_GROUP_CHUNK) == (16, 64)
    assert [f for f, _ in cls._fields_] == fields and C.sizeof(cls) == size == 8 + 2 * 8 * max_groups
    for f, line in zip(fields, out[1:]):
        d = getattr(cls, f)
        assert [d.offset, d.size] == [int(v) for v in line.split()], f
    types = dict(cls._fields_)
    assert types["n_groups"]._type_ == "i" and types["reserved"]._type_ == "i"
    for f in ("lr", "weight_decay"):
        assert issubclass(types[f], C.Array) and types[f]._length_ == max_groups and types[f]._type_ is C.c_double


def test_grouped_argument_types():
    from dostransformer_amd import _abi, _lib
    lib = _lib.load()
    P, I64, I, D, F, G = C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_float, C.POINTER(_abi.AdamWGroups)
    assert lib.dosx_adamw_grouped.argtypes == [P, P, P, P, I64, P, G, F, F, F, I, F, P]
    assert lib.dosx_adamw_grouped_f64.argtypes == [P, P, P, P, I64, P, G, D, D, D, I, P]
    assert lib.dosx_adamw_grouped_guarded.argtypes == [P, P, P, P, I64, P, G, F, F, F, I, P, P]
    assert lib.dosx_adamw_grouped_guarded_f64.argtypes == [P, P, P, P, I64, P, G, D, D, D, I, P, P]
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _abi.SIGS[name]
        assert getattr(lib, name).restype is C.c_int and name in _lib.EXPORTS
    for name, ni, nf in (("dosx_adamw_grouped", 9, 4), ("dosx_adamw_grouped_f64", 9, 3), ("dosx_adamw_grouped_guarded", 10, 3),
                         ("dosx_adamw_grouped_guarded_f64", 10, 3)):
        a, b = C.c_int(-1), C.c_int(-1)
        assert lib.dosx_replay_op(name.encode(), C.byref(a), C.byref(b)) >= 0 and (a.value, b.value) == (ni, nf), name


@pytest.mark.parametrize("name", ENTRIES)
def test_grouped_entry_points_validate_before_any_launch(name):
    """NULL operands, n < 0, step < 1, n % 64 != 0, n_groups outside [1, 16], a NaN or negative lr / weight_decay of a USED group
    and buffers (or the record) off a 16-byte boundary are refused through DOSX_CHECK_ARG: rc -22 and a message naming the entry
    point and the offending value.  n = 0 returns 0.  The addresses here are never dereferenced."""
    from dostransformer_amd import _abi, _lib
    lib = _lib.load()
    fn, who = getattr(lib, name), name.encode()
    guarded, f64 = "guarded" in name, name.endswith("f64")
    A, B, D, E, M, R = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000        # 16-byte aligned fake device addresses

    def groups(n=2, lr=(1e-3, 1e-4), wd=(1e-2, 0.0)):
        st = _abi.AdamWGroups()
        st.n_groups = n
        for k, (a, b) in enumerate(zip(lr, wd)):
            st.lr[k], st.weight_decay[k] = a, b
        return st

    def call(p=A, g=B, m=D, v=E, n=128, chunk=M, st="default", step=1, rec=R):
        st = groups() if st == "default" else st
        tail = [rec, None] if guarded else [None]
        if not f64 and not guarded:
            tail = [1.0] + tail
        return fn(p, g, m, v, n, chunk, None if st is None else C.byref(st), 0.9, 0.999, 1e-8, step, *tail)

    def refused(rc, *msgs):
        assert rc == -22, rc
        for msg in (who,) + msgs:
            assert msg in lib.dosx_last_error(), lib.dosx_last_error()

    assert call(n=0) == 0                                                             # nothing to do
    for k in "pgmv":
        refused(call(**{k: None}), b"NULL")
    refused(call(chunk=None), b"NULL")
    refused(call(st=None), b"NULL")
    if guarded:
        refused(call(rec=None), b"NULL", b"record")
        refused(call(rec=R + 8), b"16-byte aligned")
    refused(call(n=-64), b"n must not be negative", b"-64")
    refused(call(step=0), b"step is the 1-based", b"got 0")
    refused(call(step=-3), b"step is the 1-based", b"got -3")
    for n in (1, 63, 100, 130):
        refused(call(n=n), b"multiple of 64", str(n).encode())
    for n in (0, -1, 17):
        refused(call(st=groups(n=n)), b"n_groups must be in [1, 16]", f"got {n}".encode())
    nan = float("nan")
    refused(call(st=groups(lr=(1e-3, nan))), b"lr[1]", b"nan")
    refused(call(st=groups(lr=(-1e-3, 1e-3))), b"lr[0]", b"-0.001")
    refused(call(st=groups(wd=(1e-2, nan))), b"weight_decay[1]", b"nan")
    refused(call(st=groups(wd=(1e-2, -0.5))), b"weight_decay[1]", b"-0.5")
    assert call(n=0, st=groups(n=1, lr=(1e-3, nan), wd=(0.0, -1.0))) == 0             # an unused group's values are not read
    full = groups(n=16, lr=[1e-3] * 16, wd=[1e-2] * 16)
    assert call(n=0, st=full) == 0
    full.lr[15] = -1.0
    refused(call(st=full), b"lr[15]")
    for k, base in zip("pgmv", (A, B, D, E)):
        refused(call(**{k: base + 8}), b"buffers must be 16-byte aligned")
