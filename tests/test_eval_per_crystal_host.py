"""evaluate.per_crystal_metrics_host - the written-down definition of what dosx_eval_metrics computes - against the reference's
own arithmetic on one-crystal batches (`utils.py:76-89`, `:127-139`: ``((y-p)**2).mean()``, its square root, ``L1Loss`` and
sklearn's ``r2_score``), against the pinned oracle's ``_batch_metrics``, and what the new entry points do without a GPU."""
import functools

import numpy as np
import pytest
import torch

from dostransformer_amd import evaluate, synth

TOL = 1e-12                      # x max(1, |v|): sums of at most 201 float64 terms


def _close(a: float, b: float) -> bool:
    return abs(a - b) <= TOL * max(1.0, abs(b))


@functools.lru_cache(maxsize=None)
def _rows(kind: str):
    """(targets, noisy predictions) in float64: the phdos of 37 phonon crystals (S = 51) / the y_ft of 21 eDOS crystals (S = 201)."""
    if kind == "phonon":
        y = torch.stack([c["phdos"].reshape(-1) for c in synth.phonon_crystals(37, 401)]).double()
    else:
        y = torch.stack([c["y_ft"].reshape(-1) for c in synth.edos_crystals(21, 402)]).double()
    gen = torch.Generator().manual_seed(7)
    scale = y.std(dim=1, keepdim=True) * (0.5 + torch.rand(y.shape[0], 1, generator=gen, dtype=torch.float64))
    p = y + scale * torch.randn(y.shape, generator=gen, dtype=torch.float64)
    return y, p


@pytest.mark.parametrize("clamp0", [False, True])
@pytest.mark.parametrize("kind", ["phonon", "edos"])
def test_twin_equals_the_reference_loop_at_batch_size_1(kind, clamp0):
    sk = pytest.importorskip("sklearn.metrics")
    y, p = _rows(kind)
    assert tuple(y.shape) == ((37, 51) if kind == "phonon" else (21, 201))
    got = evaluate.per_crystal_metrics_host(p, y, clamp0)
    assert got.dtype == torch.float64 and tuple(got.shape) == (y.shape[0], 4)
    l1 = torch.nn.L1Loss()
    for c in range(y.shape[0]):
        yc, pc = y[c:c + 1], p[c:c + 1]                      # the batch of one crystal
        if clamp0:
            yc, pc = torch.clamp(yc, min=0.0), torch.clamp(pc, min=0.0)
        assert float(((yc - yc.mean()) ** 2).sum()) > 1.0   # far from sklearn's special case for a constant target
        mse = ((yc - pc) ** 2).mean(dim=1)
        want = (float(torch.sqrt(mse).mean()), float(mse.mean()), float(l1(pc, yc)),
                float(sk.r2_score(yc.flatten().numpy(), pc.flatten().numpy(), multioutput="variance_weighted")))
        for k in range(4):
            assert _close(float(got[c, k]), want[k]), (c, k, float(got[c, k]), want[k])


@pytest.mark.parametrize("clamp0", [False, True])
@pytest.mark.parametrize("kind", ["phonon", "edos"])
def test_twin_mean_equals_the_oracle_over_single_row_batches(kind, clamp0):
    from oracle import dos_oracle as O
    y, p = _rows(kind)
    yc, pc = (torch.clamp(y, min=0.0), torch.clamp(p, min=0.0)) if clamp0 else (y, p)
    acc = np.zeros(4)
    for c in range(y.shape[0]):
        acc += np.array(O._batch_metrics(yc[c:c + 1], pc[c:c + 1]))
    acc /= y.shape[0]
    got = evaluate.per_crystal_metrics_host(p, y, clamp0).mean(0)
    for k in range(4):
        assert _close(float(got[k]), float(acc[k])), (k, float(got[k]), float(acc[k]))


def test_twin_on_a_constant_target_is_evaluate_r2_of_that_row():
    y = torch.full((3, 51), 0.5, dtype=torch.float64)
    y[2] = torch.linspace(0.0, 1.0, 51, dtype=torch.float64)
    p = y.clone()
    p[0] += 0.25                                             # constant target, error > 0: -inf; row 1: error 0 too: NaN
    got = evaluate.per_crystal_metrics_host(p, y)
    for c in range(3):
        want = evaluate.r2(y[c:c + 1], p[c:c + 1])
        assert np.isclose(float(got[c, 3]), want, rtol=0.0, atol=0.0, equal_nan=True), (c, float(got[c, 3]), want)
    assert float(got[0, 3]) == -np.inf and np.isnan(float(got[1, 3])) and float(got[2, 3]) == 1.0
    assert _close(float(got[0, 0]), 0.25) and _close(float(got[0, 1]), 0.0625) and _close(float(got[0, 2]), 0.25)
    # the eDOS clamp: a negative constant target is the constant 0
    got = evaluate.per_crystal_metrics_host(torch.full((1, 7), -2.0), torch.full((1, 7), -1.0), clamp0=True)
    assert np.isnan(float(got[0, 3])) and float(got[0, 0]) == 0.0


def test_mean_of_per_crystal_r2_is_not_the_r2_of_the_flattened_batch():
    """What test_per_crystal returns is a different quantity from evaluate.test_phonon on one big batch."""
    y, p = _rows("phonon")
    per = float(evaluate.per_crystal_metrics_host(p, y)[:, 3].mean())
    flat = evaluate.r2(y, p)
    assert abs(per - flat) > 1e-3, (per, flat)
    # ... while the batch's mse is the mean of the rows' (equal row lengths), and its rmse - a mean of roots - is too
    rows = evaluate.per_crystal_metrics_host(p, y)
    assert _close(float(rows[:, 1].mean()), float(((y - p) ** 2).mean()))


def test_entry_points_are_bound_and_refuse_without_a_gpu():
    import ctypes as C
    from dostransformer_amd import _abi, _lib, ops
    for name in ("dosx_eval_metrics", "dosx_eval_metrics_f64"):
        assert name in _abi.SIGS and name in _lib.EXPORTS
        assert _abi.SIGS[name] == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib = _lib.load()
    A, B, D = 0x10000, 0x20000, 0x30000                      # fake device addresses: refused before they are dereferenced
    for fn in (lib.dosx_eval_metrics, lib.dosx_eval_metrics_f64):
        assert fn(A, B, 0, 51, 0, D, None, None, None) == 0  # no rows: nothing to do
        for args in ((A, B, 4, 0, 0, D, None, None), (A, B, -1, 51, 0, D, None, None), (None, B, 4, 51, 0, D, None, None),
                     (A, None, 4, 51, 1, D, None, None), (A, B, 4, 51, 1, None, None, None), (A, B, 4, 51, 1, D, B, None),
                     (A, B, 4, 51, 1, D, None, A)):
            assert fn(*args, None) == -22, args
            assert b"dosx_eval_metrics" in lib.dosx_last_error()
    # the wrapper: no CPU path, and shapes / dtypes are checked before anything is launched
    p, y, m = torch.zeros(4, 51), torch.zeros(4, 51), torch.zeros(4, 4, dtype=torch.float64)
    with pytest.raises((TypeError, RuntimeError), match="CUDA"):
        ops.eval_metrics(p, y, m)
    with pytest.raises(ValueError, match="per-crystal keys"):
        class _NoKeys:
            per_crystal_keys = False
        evaluate.test_per_crystal(_NoKeys(), None)
