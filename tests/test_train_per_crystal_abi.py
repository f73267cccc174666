"""Per-crystal keys of the fp32 trainer, the parts a machine without a GPU can check: the ctypes mirror of DosxFfnBwd against the
C layout (att_key_ptr last), Trainer(per_crystal_keys=...) as an interface, and that model.set_per_crystal_keys stays the float64
program's switch."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dosx.h")


def test_ffn_bwd_mirror_has_the_c_layout_with_att_key_ptr_last(tmp_path):
    from dostransformer_amd import _lib
    names = [n for n, _ in _lib.FfnBwd._fields_]
    assert names[-1] == "att_key_ptr"
    # the C struct's own field order, from the header text
    body = re.search(r"typedef struct DosxFfnBwd \{(.*?)\} DosxFfnBwd;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            c_names.append(re.search(r"(\w+)\s*$", part.strip()).group(1))
    assert c_names == names
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dosx.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(DosxFfnBwd));']
    lines += [f'  printf("%zu\\n", offsetof(DosxFfnBwd, {n}));' for n in names]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)   # (as tests/test_lib_abi.py)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.FfnBwd)
    assert out[1:] == [getattr(_lib.FfnBwd, n).offset for n in names]


def _cpu_model():
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    return DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.0)


def test_trainer_flag_is_a_read_only_attribute():
    from dostransformer_amd.train import Trainer
    model = _cpu_model()
    assert Trainer(model).per_crystal_keys is False
    tr = Trainer(model, per_crystal_keys=True)
    assert tr.per_crystal_keys is True
    with pytest.raises(AttributeError):
        tr.per_crystal_keys = False
    assert tr.per_crystal_keys is True


def test_trainer_refuses_the_flag_under_data_parallelism():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer

    class _Dist:
        world, rank = 2, 0

    with pytest.raises(DosxError, match="per_crystal_keys"):
        Trainer(_cpu_model(), dist=_Dist(), per_crystal_keys=True)
    assert Trainer(_cpu_model(), dist=_Dist()).per_crystal_keys is False       # (the flag off: as before)


def test_set_per_crystal_keys_still_belongs_to_the_float64_program():
    from dostransformer_amd._lib import DosxError
    model = _cpu_model()
    with pytest.raises(DosxError):
        model.set_per_crystal_keys(True)
    assert model.per_crystal_keys is False
