"""ctypes binding of ``csrc/libdosx.so`` (C ABI declared in ``include/dosx.h``).

There is NO fallback: if the HIP library is missing or fails to load, every op raises
:class:`DosxUnavailable` — the product path never routes through a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

# The ABI itself - struct mirrors, argtypes, restypes, DOSX_* constants - is _abi.py, GENERATED from include/dosx.h by
# tools/gen_ctypes.py (csrc/Makefile runs it): an entry point or a field is added by editing dosx.h and running make.  The
# struct classes are re-exported from here (`from ._lib import Gemm`, `_lib.Call`).
from . import _abi
from ._abi import *  # noqa: F401,F403

_HERE = os.path.dirname(os.path.abspath(__file__))


def from_environ(name: str, default: str = "") -> str:
    """The ONE place where the package reads a process variable: DOSX_LIB, DOSX_FFN_BF16X3, DOSX_DP_MID_BUCKET, DOSX_DP_CHECK
    (tests/test_host_logic.py holds that list).  Every other form choice is a plain module attribute."""
    return os.environ.get(name, default)


LIB_PATH = from_environ("DOSX_LIB") or os.path.join(_HERE, "csrc", "libdosx.so")   # DOSX_LIB: diagnostic builds only

BIG = 1 << 30


class DosxUnavailable(RuntimeError):
    pass


class DosxError(RuntimeError):
    pass


_SIGS = _abi.SIGS
EXPORTS = tuple(_SIGS)

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libdosx.so once; raise DosxUnavailable (never fall back) if that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DosxUnavailable(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C dostransformer_amd/csrc` (needs hipcc, --offload-arch=gfx950). "
            f"dostransformer_amd has no CPU fallback.")
    try:
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so); it must be the one already in the
        # process when libdosx.so is resolved, otherwise two runtimes coexist and ours sees no device.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise DosxUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    for name, args in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = _abi.RESTYPES.get(name, C.c_int)
    _lib = lib
    return lib


def source_hash() -> str:
    """sha256 (first 16 hex digits) over the sources that decide which kernels a step launches and what they do: csrc/,
    include/dosx.h and the launch-sequencing Python.  profiles/r*_pmc_traffic.json carries the hash it was measured on;
    bench.py refuses the file when it differs (the box has no .git, so a content hash stands in for the commit)."""
    import glob
    import hashlib
    root = os.path.dirname(_HERE)
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h")) +
                   glob.glob(os.path.join(_HERE, "csrc", "*.cpp")))
    files += [os.path.join(root, "include", "dosx.h")] + [os.path.join(_HERE, f) for f in ("functional.py", "ops.py", "train.py", "trainer_base.py")]
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.relpath(f, root).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().dosx_last_error()
        raise DosxError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")
