"""The bits of the eight AdamW entries (csrc/adamw.hip; include/dosx.h: dosx_adamw, _f64, _guarded*, _grouped*) on a real MI355X.

The other optimizer tests hold the ungrouped kernels to error bounds and the guarded / grouped ones to the ungrouped kernels of
the SAME build.  This one pins every form to tests/golden/adamw_bits.json: the SHA-256 of the bytes of p, m and v after one launch
on seeded inputs, recorded by tools/record_adamw_bits.py from the library of the commit the fixture names.  A changed contraction
(an fma where a mul + add stood), a changed rounding of a host scalar or a changed tail shows here as another digest.

Inputs come from a seeded CPU generator in the style of test_gpu_tail._adam_state: |p| over 1e-4 .. 10, |g| over 1e-8 .. 100 with
some exact zeros, moments of the gradients' own magnitude (zero at step 1).  The record of a guarded case is written by
ops.grad_guard on the case's own gradient."""
import functools
import hashlib
import json
import os

import pytest
import torch

from tests.gpu_util import DEV, ops

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw_bits.json")
B1, B2, EPS, LR, WD = 0.9, 0.999, 1e-8, 1e-3, 1e-2
SENT = -7.25
PAD = 64                                    # sentinel elements behind n (one chunk for the grouped forms)
F32, F64 = torch.float32, torch.float64
# one sweep of the capped grid: fp32 4096 workgroups x 256 threads x 4 floats, float64 2048 x 256 x 2
CAP = {F32: 4096 * 256 * 4, F64: 2048 * 256 * 2}
NAME = {F32: "f32", F64: "f64"}


def _groups(G):
    """G (lr, weight_decay) pairs, every pair distinct; from 3 groups on, group 2 stands at lr = 0"""
    return [(0.0 if k == 2 else LR * (k + 1) / G, WD * (k % 4) / 4) for k in range(G)]


def _chunk_ids(n, G):
    """Neighbouring chunks differ wherever there is more than one group; with more than two chunks the second byte is 200
    (>= n_groups: stepped as group 0)"""
    ids = [(c + c // 4099) % G for c in range(n // 64)]
    if len(ids) > 2:
        ids[1] = 200
    return ids


def _cases():
    out = []
    for dt in (F32, F64):
        sizes = (1, 5, 1003, CAP[dt] + 7) if dt == F32 else (1, 2, 1003, CAP[dt] + 3)
        for n in sizes:                     # scalar tail only, vectors + tail, beyond the grid cap
            for step in ((1000,) if n > CAP[dt] else (1, 1000)):
                out.append(dict(form="plain", dtype=dt, n=n, step=step))
        for n, G in ((64, 1), (17 * 64, 16), (CAP[dt] + 64, 3)):
            for step in ((1000,) if n > CAP[dt] else (1, 1000)):
                out.append(dict(form="grouped", dtype=dt, n=n, step=step, G=G))
        for state in ("notrip", "clip", "skipped"):
            out.append(dict(form="guarded", dtype=dt, n=1003, step=7, state=state))
            out.append(dict(form="grouped_guarded", dtype=dt, n=17 * 64, step=7, G=16, state=state))
    for c in out:
        c["id"] = "-".join([c["form"], NAME[c["dtype"]], f"n{c['n']}"] + ([f"G{c['G']}"] if "G" in c else []) +
                           [c["state"] if "state" in c else f"step{c['step']}"])
    return out


CASES = _cases()


def _state(dtype, n, step, seed):
    """p, g, m, v of n (rounded up to 4) + PAD elements, sentinel-filled behind n"""
    gen = torch.Generator().manual_seed(seed)
    npad = (n + 3) // 4 * 4 + PAD
    u = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    r = lambda: torch.randn(n, generator=gen, dtype=torch.float64)
    gmag = 10.0 ** (u() * 10 - 8)
    g = r() * gmag
    g[torch.randperm(n, generator=gen)[:min(100, n // 2)]] = 0.0
    vals = [r() * 10.0 ** (u() * 5 - 4), g]
    if step == 1:
        vals += [torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)]
    else:
        vals += [0.5 * r() * gmag, (r() * gmag) ** 2 * u()]
    out = []
    for t in vals:
        b = torch.full((npad,), SENT, dtype=dtype, device=DEV)
        b[:n] = t.to(dtype).to(DEV)
        out.append(b)
    return out


def _launch(case, p, g, m, v, rec=None, step=None):
    o, n, f32 = ops(), case["n"], case["dtype"] == F32
    step = case["step"] if step is None else step
    if "G" in case:
        chunk = torch.tensor(_chunk_ids(n, case["G"]), dtype=torch.uint8).to(DEV)
        a = (p, g, m, v, n, chunk, _groups(case["G"]), B1, B2, EPS, step)
        if rec is not None:
            (o.adamw_grouped_guarded if f32 else o.adamw64_grouped_guarded)(*a, rec)
        elif f32:
            o.adamw_grouped(*a, 1.0 / 3.0)
        else:
            o.adamw64_grouped(*a)
    elif rec is not None:
        (o.adamw_guarded if f32 else o.adamw64_guarded)(p, g, m, v, n, LR, B1, B2, EPS, WD, rec)
    elif f32:
        o.adamw(p, g, m, v, n, LR, B1, B2, EPS, WD, step, 1.0 / 3.0)
    else:
        o.adamw64(p, g, m, v, n, LR, B1, B2, EPS, WD, step)


def run_case(case):
    """One launch of ``case`` -> {"p", "m", "v"}: the SHA-256 of the first n elements' bytes.  Asserts what no fixture is needed
    for: g and everything behind n untouched, a skipped step without a store."""
    o, n, step = ops(), case["n"], case["step"]
    p, g, m, v = _state(case["dtype"], n, step, 4100 + CASES.index(case))
    start = [t.clone() for t in (p, g, m, v)]
    rec = None
    if "state" in case:
        rec, ws = o.guard_buffers(DEV)
        guard = lambda grad, max_norm, at: o.grad_guard(grad, n, rec, ws, max_norm, LR, B1, B2, at)
        if case["state"] == "notrip":
            guard(g, None, step)
            r = o.guard_read(rec)
            assert r.skip == 0 and r.clip == 1.0 and r.t == step
        elif case["state"] == "clip":
            guard(g, 1e-2, step)
            r = o.guard_read(rec)
            assert r.skip == 0 and 0.0 < r.clip < 1.0 and r.t == step
        else:                               # one skipped attempt first: AdamW's time falls behind the attempt count
            bad = g.clone()
            bad[n // 2] = float("nan")
            guard(bad, None, 1)
            assert o.guard_read(rec).skip == 1
            _launch(case, p, bad, m, v, rec, step=1)
            torch.cuda.synchronize()
            for t, t0 in zip((p, m, v), (start[0], start[2], start[3])):
                assert torch.equal(t, t0), (case["id"], "a skipped step stored something")
            guard(g, None, 2)
            r = o.guard_read(rec)
            assert r.skip == 0 and r.skipped == 1 and r.t == 1
            step = 2
    _launch(case, p, g, m, v, rec, step=step)
    torch.cuda.synchronize()
    assert torch.equal(g, start[1]), (case["id"], "gradient changed")
    for t in (p, m, v):
        assert bool((t[n:] == SENT).all()), (case["id"], "written behind n")
    assert not torch.equal(m[:n], start[2][:n]) and not torch.equal(v[:n], start[3][:n]), (case["id"], "nothing stepped")
    return {k: hashlib.sha256(t[:n].cpu().numpy().tobytes()).hexdigest() for k, t in (("p", p), ("m", m), ("v", v))}


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_names_every_case_and_its_commit():
    fx = _fixture()
    assert len(fx["commit"]) == 40 and sorted(fx["cases"]) == sorted(c["id"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_adamw_bits(case):
    want = _fixture()["cases"][case["id"]]
    got = run_case(case)
    assert got == want, (case["id"], [k for k in "pmv" if got[k] != want[k]], "recorded from", _fixture()["commit"])
