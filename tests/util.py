"""Shared helpers for the tests: golden-fixture loading, and the binding module with its library in place."""
import os

import numpy as np
import torch

from dostransformer_amd.batch import CrystalBatch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dosx_lib():
    """dostransformer_amd._lib with libdosx.so in place (built first when it is missing)."""
    from dostransformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def in_all_three_builds(src):
    """True when csrc/Makefile compiles ``src`` into libdosx.so and into both diagnostic builds: it stands in SRCS, and the
    `stamps` and `acqrel` recipes take every .hip file of SRCS."""
    import re
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "dostransformer_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()
    recipes = re.findall(r"^\t\$\(HIPCC\) .* -shared -o build/libdosx_(stamps|acqrel)\.so (.*)$", text, re.M)
    return src in srcs and sorted(k for k, _ in recipes) == ["acqrel", "stamps"] and \
        all(r.startswith("$(filter %.hip,$(SRCS)) ") for _, r in recipes)


def load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def sub(z, prefix):
    """All entries of an npz under ``prefix`` as torch tensors (prefix stripped)."""
    out = {}
    for k in z.files:
        if k.startswith(prefix):
            v = z[k]
            if v.dtype.kind in "fiub":
                out[k[len(prefix):]] = torch.from_numpy(np.array(v))
    return out


def batch_from(z, prefix="b/"):
    f = sub(z, prefix)
    nb = int(f.pop("num_graphs"))
    g = CrystalBatch(f, nb)
    if prefix + "mp_id" in z.files:
        g.mp_id = [str(s) for s in z[prefix + "mp_id"]]
    return g


def rmse(a, b):
    a = torch.as_tensor(a).detach().to(torch.float64)
    b = torch.as_tensor(b).detach().to(torch.float64)
    return float(torch.sqrt(torch.mean((a - b) ** 2)))


def maxabs(a, b):
    a = torch.as_tensor(a).detach().to(torch.float64)
    b = torch.as_tensor(b).detach().to(torch.float64)
    return float((a - b).abs().max()) if a.numel() else 0.0
