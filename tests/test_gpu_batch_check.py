"""Batch validation on the GPU (csrc/validate.hip behind dostransformer_amd/validate.py): dosx_batch_check's report against the
numpy twin word for word - on the hand-worked small batch (tests/batch_check_cases.py), on synthetic batches with random
corruptions, at the launch's workgroup and grid strides, inside sentinel-filled allocations with extreme values - the finite
checks at the edges of their 16-byte loads, and the process-wide switch in front of a model call."""
import numpy as np
import pytest
import torch

from tests import batch_check_cases as cases
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

INT64_MIN = -2 ** 63
EXTREMES = [-1, None, 2 ** 40, INT64_MIN]          # None: the array's own bound (N for an endpoint, B for batch, 7 for system)


def _twin(b, **kw):
    from dostransformer_amd import validate
    return validate.check_batch_host(b["edge_index"], b["batch"], b["system"], b["num_graphs"], **kw)


def _device(b, tensors=None, **kw):
    """dosx_batch_check on device copies of the batch dict (or on the given device tensors): the report's words."""
    from dostransformer_amd import validate
    t = tensors or {k: (None if b[k] is None else torch.from_numpy(np.ascontiguousarray(b[k])).to(DEV))
                    for k in ("edge_index", "batch", "system")}
    rep = torch.from_numpy(validate.empty_report()).to(DEV)
    validate.batch_check_device(t["edge_index"], t["batch"], t["system"], b["num_graphs"], kw.get("n_max"),
                                kw.get("require_sorted", False), rep)
    return rep.cpu().numpy()


@pytest.mark.parametrize("name", [c[0] for c in cases.CASES])
def test_report_on_the_small_batch_is_the_twins(name):
    b, kw, want = cases.corrupted(name)
    got = _device(b, **kw)
    assert got.tolist() == _twin(b, **kw).tolist() == cases.expected_words(want).tolist(), (name, got.tolist())


def test_report_r6_first_no_edges_and_one_crystal():
    sizes, kw, want = cases.CASE_R6_FIRST
    assert _device(cases.small_batch(sizes), **kw).tolist() == cases.expected_words(want).tolist()
    b = cases.small_batch()
    b["edge_index"] = np.zeros((2, 0), np.int64)
    assert _device(b, require_sorted=True).tolist() == cases.expected_words({}).tolist()
    one = {"edge_index": np.zeros((2, 1), np.int64), "batch": np.zeros(1, np.int64), "system": np.asarray([7]), "num_graphs": 1}
    assert _device(one, require_sorted=True, n_max=1).tolist() == cases.expected_words({5: (1, 0)}).tolist()


def _synth(seed):
    from dostransformer_amd import synth
    g = synth.phonon_batch(6, seed, dtype=torch.float32)
    return {"edge_index": g.edge_index.numpy().copy(), "batch": g.batch.numpy().copy(), "system": g.system.numpy().copy(),
            "num_graphs": 6}


def _corrupt(b, k, rng):
    """k random corruptions of mixed rules, extreme values included."""
    N, E, B = b["batch"].shape[0], b["edge_index"].shape[1], b["num_graphs"]
    for _ in range(k):
        kind = int(rng.integers(0, 5))
        ext = EXTREMES[int(rng.integers(0, 4))]
        if kind == 0:                                                           # R1: an endpoint out of range
            b["edge_index"][int(rng.integers(0, 2)), int(rng.integers(0, E))] = N if ext is None else ext
        elif kind == 1:                                                         # R2 / R7: an endpoint somewhere else in range
            b["edge_index"][int(rng.integers(0, 2)), int(rng.integers(0, E))] = int(rng.integers(0, N))
        elif kind == 2:                                                         # R3 (and what follows from it: R2, R4, R6)
            b["batch"][int(rng.integers(0, N))] = B if ext is None else ext
        elif kind == 3:
            b["batch"][int(rng.integers(0, N))] = int(rng.integers(0, B))
        else:                                                                   # R5
            b["system"][int(rng.integers(0, B))] = 7 if ext is None else ext


@pytest.mark.parametrize("k", [1, 2, 50])
@pytest.mark.parametrize("seed", [0, 1])
def test_report_on_a_synthetic_batch_with_random_corruptions_is_the_twins(seed, k):
    b = _synth(seed)
    n_max = int(np.bincount(b["batch"]).max()) - 1 if k == 50 else int(np.bincount(b["batch"]).max())
    clean = _device(b, require_sorted=True, n_max=int(np.bincount(b["batch"]).max()))
    assert clean.tolist() == cases.expected_words({}).tolist()
    _corrupt(b, k, np.random.default_rng(100 * seed + k))
    got, want = _device(b, require_sorted=True, n_max=n_max), _twin(b, require_sorted=True, n_max=n_max)
    assert got.tolist() == want.tolist(), (got.tolist(), want.tolist())
    assert want[0::2].sum() >= 1                                                # the corruption did corrupt


def _strided_batch(E, seed=0):
    """4 crystals of 8 atoms, E destination-sorted edges inside their crystals."""
    rng = np.random.default_rng(seed)
    B, n = 4, 8
    dst = np.sort(rng.integers(0, B * n, E)).astype(np.int64)
    src = (dst // n) * n + rng.integers(0, n, E)
    return {"edge_index": np.stack([src, dst]).astype(np.int64), "batch": np.repeat(np.arange(B), n).astype(np.int64),
            "system": np.asarray([0, 1, 5, 6], np.int64), "num_graphs": B}


def _stride_sizes():
    from dostransformer_amd import _abi
    wg, sweep = _abi.DOSX_CHECK_THREADS, _abi.DOSX_CHECK_THREADS * _abi.DOSX_CHECK_MAX_BLOCKS
    return [wg - 1, wg, wg + 1, 2 * sweep + 17]


@pytest.mark.parametrize("which", range(4))
def test_report_at_the_workgroup_and_grid_strides_with_the_offender_at_the_last_edge(which):
    E = _stride_sizes()[which]
    b = _strided_batch(E, seed=which)
    assert _device(b, require_sorted=True, n_max=8).tolist() == cases.expected_words({}).tolist()
    N = b["batch"].shape[0]
    b["edge_index"][0, E - 1] = N                                               # R1 at the very last edge
    got = _device(b, require_sorted=True)
    assert got.tolist() == _twin(b, require_sorted=True).tolist() == cases.expected_words({1: (1, E - 1)}).tolist()
    b["edge_index"][:, E - 1] = (0, 8)                                          # in range again: joins crystals 0 and 1, steps down
    got = _device(b, require_sorted=True)
    assert got.tolist() == _twin(b, require_sorted=True).tolist() == cases.expected_words({2: (1, E - 1), 7: (1, E - 1)}).tolist()
    b["edge_index"][0, ::3] = -1                                                # many offenders: the sum and the minimum hold
    got = _device(b, require_sorted=True)
    assert got.tolist() == _twin(b, require_sorted=True).tolist() and got[0] == (E + 2) // 3 and got[1] == 0


SENT = 2 ** 62 + 12345          # as an index it would be far outside anything; as a value it violates R1, R3 and R5


def _inside_sentinels(a, pad):
    """``a`` (int64 numpy) as a contiguous view into a larger device allocation filled with SENT, ``pad`` words on either side."""
    buf = torch.full((a.size + 2 * pad,), SENT, dtype=torch.int64, device=DEV)
    view = buf[pad:pad + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, view


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_extreme_values_are_classified_from_the_value_alone_inside_sentinel_filled_allocations(seed):
    """edge_index, batch and system sit in the middle of sentinel-filled allocations and hold -1, their own bound, 2**40 and
    INT64_MIN: the report is the twin's on the inner arrays - a sentinel read as an element would be counted as a violation, an
    extreme value used as an index would leave the allocation.  Nothing else runs on these batches."""
    rng = np.random.default_rng(seed)
    b = cases.small_batch() if seed == 0 else _synth(seed)
    N, E, B = b["batch"].shape[0], b["edge_index"].shape[1], b["num_graphs"]
    for i, ext in enumerate(EXTREMES):
        b["edge_index"][i % 2, int(rng.integers(0, E))] = N if ext is None else ext
        b["batch"][int(rng.integers(0, N))] = B if ext is None else ext
    b["edge_index"][:, E - 1] = (INT64_MIN, 2 ** 40)                            # both endpoints of the last edge
    b["edge_index"][:, 0] = (-1, N)
    b["batch"][N - 1] = INT64_MIN
    b["system"][:3] = (-1, 7, 2 ** 40)
    keep, tensors = [], {}
    for k in ("edge_index", "batch", "system"):
        buf, view = _inside_sentinels(b[k], pad=64)
        keep.append(buf)
        tensors[k] = view
        assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 8 * 64
    got, want = _device(b, tensors, require_sorted=True, n_max=2), _twin(b, require_sorted=True, n_max=2)
    assert got.tolist() == want.tolist(), (got.tolist(), want.tolist())
    assert want[0] >= 2 and want[4] >= 2 and want[8] >= 3
    for buf, k in zip(keep, ("edge_index", "batch", "system")):                 # (the checker writes nothing but its report)
        assert bool((buf[:64] == SENT).all()) and bool((buf[-64:] == SENT).all())
        assert torch.equal(tensors[k].cpu(), torch.from_numpy(b[k]))


def _finite(t):
    from dostransformer_amd import validate
    slot = torch.from_numpy(validate.empty_report(1)).to(DEV)
    validate.finite_check_device(t, slot)
    return tuple(slot.cpu().tolist())


BAD = [float("nan"), float("inf"), float("-inf")]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_finite_check_counts_and_finds_the_first_at_the_edges_of_the_vector_loads(dtype, n, offset):
    """NaN, +inf and -inf at index 0, at n - 1 and at the first element of the scalar tail: count and first are exact; a clean tensor
    gives {0, INT32_MAX}.  offset1: the tensor starts one element behind a 16-byte boundary (a scalar head in front of the loads)."""
    per = 16 // torch.empty(0, dtype=dtype).element_size()
    g = torch.Generator().manual_seed(n)
    base = torch.randn(n + offset + 8, generator=g, dtype=torch.float64).to(dtype)
    base[0:offset] = float("nan")                                               # in front of the tensor: must not be seen
    base[n + offset:] = float("inf")                                            # behind it: must not be seen
    dev = base.to(DEV)
    t = dev[offset:offset + n]
    assert t.data_ptr() % 16 == (offset * t.element_size()) % 16
    assert _finite(t) == (0, cases.INT32_MAX)
    head = (per - offset) % per if offset else 0
    tail0 = head + ((n - head) // per) * per if n >= head else 0                # first element of the scalar tail (n: none)
    spots = sorted({0, n - 1, min(tail0, n - 1), min(head, n - 1)})
    for i in spots:                                                             # one at a time: `first` is that index
        for v in BAD:
            u = t.clone()
            u[i] = v
            assert _finite(u if offset == 0 else _rehome(u, offset)) == (1, i), (i, v)
    u = t.clone()
    for j, i in enumerate(spots):
        u[i] = BAD[j % 3]
    assert _finite(u if offset == 0 else _rehome(u, offset)) == (len(spots), 0)
    if n >= 5:
        u = t.clone()
        u[2:n - 1] = float("nan")
        assert _finite(u if offset == 0 else _rehome(u, offset)) == (n - 3, 2)


def _rehome(u, offset):
    """A copy of ``u`` that starts ``offset`` elements behind a 16-byte boundary again (clone() re-aligns)."""
    buf = torch.zeros(u.numel() + offset + 4, dtype=u.dtype, device=u.device)
    out = buf[offset:offset + u.numel()]
    out.copy_(u)
    assert out.data_ptr() % 16 == (offset * u.element_size()) % 16
    return out


def test_finite_check_beyond_one_grid_sweep():
    """More 16-byte loads than one sweep of the capped grid (2048 workgroups of 256 threads): the stride loop's later rounds."""
    n = 2 * 2048 * 256 * 4 + 4 * 300 + 3
    t = torch.zeros(n, dtype=torch.float32, device=DEV)
    assert _finite(t) == (0, cases.INT32_MAX)
    t[n - 1] = float("nan")
    assert _finite(t) == (1, n - 1)
    t[2048 * 256 * 4 + 5] = float("-inf")                                       # the first load of the second sweep's second thread
    assert _finite(t) == (2, 2048 * 256 * 4 + 5)
    t[::2] = float("inf")
    assert _finite(t) == ((n + 1) // 2 + 1, 0)
    assert _finite(torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)) == (n, 0)


def _foreign(seed=3, system7=False):
    from dostransformer_amd import synth
    from dostransformer_amd.batch import CrystalBatch
    g = synth.phonon_batch(4, seed=seed, dtype=torch.float32, sort_edges=False)
    perm = torch.randperm(g.edge_index.shape[1], generator=torch.Generator().manual_seed(5))
    system = g.system.clone()
    if system7:
        system[2] = 7
    return CrystalBatch({"x": g.x.to(DEV), "edge_index": g.edge_index[:, perm].to(DEV), "edge_vec": g.edge_vec[perm].to(DEV),
                         "batch": g.batch.to(DEV), "system": system.to(DEV), "phdos": g.phdos.to(DEV)}, 4, meta=None)


def test_switch_stops_a_bad_foreign_batch_before_any_other_launch_and_changes_nothing_for_a_valid_one(monkeypatch):
    from dostransformer_amd import ops, validate
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(0)
    model = DOSTransformer_phonon(2, 1, 118, 4, 64, DEV, 0.0).to(DEV).eval()
    with torch.no_grad():
        off = [t.clone() for t in model(_foreign())]
    issued, real_call = [], ops._call

    def counting(name, *a, **k):
        issued.append(name)
        return real_call(name, *a, **k)
    monkeypatch.setattr(ops, "_call", counting)
    try:
        validate.enable(True, finite=True)
        bad = _foreign(system7=True)
        with torch.no_grad(), pytest.raises(DosxError, match=r"R5 .*crystal 2: system 7 outside \[0, 7\)"):
            model(bad)
        assert issued and set(issued) <= {"dosx_batch_check", "dosx_finite_check_f32"} and issued[0] == "dosx_batch_check", issued
        assert bad.meta is None                                                 # nothing was derived from it
        del issued[:]
        with torch.no_grad():
            on = model(_foreign())
        assert issued[:4] == ["dosx_batch_check"] + ["dosx_finite_check_f32"] * 3 and "dosx_csr_build" in issued
    finally:
        validate.enable(False)
    for a, b in zip(on, off):
        assert torch.equal(a, b)                                                # bitwise: the check reads, it changes nothing
