"""Every compiled dosx_gemm kernel (csrc/gemm.hip: gemm_kernel, gemm_mixed_kernel, gemm_pair_kernel - tests/gemm_census.py lists
the instantiations and the smallest shapes that select each) at its tile edges: the last row tile holding one row and all but
one, a column tile filled exactly and ragged, K = 4 / not a multiple of the k-chunk / a multiple of it / two segments meeting
inside a chunk.  Each case asserts
  - the kernel: dosx_gemm_kernel_name names the instantiation of the census row (a tail split: dosx_gemm_partial_rows);
  - no stray store: every output is a view into a sentinel-filled allocation (a guard row above, 64 below, guard columns
    left and right, ldo > N) whose margins keep the sentinel's bits;
  - no stray read: every operand is a view into NaN (rows behind M, columns behind K, table rows behind the last index), and
    no NaN reaches an output or a partial row;
  - the values: float64 torch on the same fp32 operands, PER ROW against that row's own largest magnitude."""
import pytest
import torch

from tests import gemm_census as cen
from tests.gpu_util import DEV, ops

pytestmark = pytest.mark.gpu


def _lib():
    from dostransformer_amd import _lib
    return _lib.load()


def _kid(kernel):
    return kernel.replace("gemm_", "").replace("_kernel<", "").replace(", ", "").rstrip(">")


def _judge(spec, got, ref, intact, what, t):
    if "dalpha" in ref:                       # the figure the dalpha bounds of the census are 4 x of, on these very operands
        base = cen.errors(spec, cen.reference(spec, t, torch.float32), ref)
        print(f"fp32 torch [{spec['epi']}]: dalpha {base['dalpha']:.2e}")
    assert all(intact.values()), f"{what}: store outside the output view: {intact}"
    assert set(got) == cen.outputs(ref), (what, sorted(got), sorted(ref))
    e = cen.errors(spec, got, ref)
    print(f"{what}: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v < cen.bound(spec["epi"], k), (what, k, v, cen.bound(spec["epi"], k))


def _what(spec):
    keys = ("M", "N", "K", "k1", "bias", "act", "res", "res_col0", "res_pre", "stats", "norm", "partials", "add", "mean")
    return spec["kernel"] + " " + " ".join(f"{k}={spec[k]}" for k in keys if spec.get(k))


def _run_cases(specs, split):
    o, lib = ops(), _lib()
    for spec in specs:
        t = cen.make_inputs(spec, DEV)
        ref = cen.reference(spec, t)
        got, named, intact, prow = cen.run(o, lib, spec, t)
        assert named == spec["kernel"], (named, _what(spec))
        if "graph" not in spec and not (spec.get("stats") or spec.get("norm")):      # (stats_out / norm_out never split)
            assert cen.is_split(lib, spec["M"], spec["N"], spec["epi"], named) == split, _what(spec)
        if split:                   # what dosx_gemm needs besides the policy to take the mixed-height grid, on the real descriptor
            assert named.split(", ")[4] == "1" and not (spec.get("stats") or spec.get("norm")), _what(spec)
        _judge(spec, got, ref, intact, _what(spec), t)


@pytest.mark.parametrize("row", cen.ROWS, ids=[_kid(r[4]) + ("_" + r[3] if r[3] else "") for r in cen.ROWS])
def test_gemm_kernel_instantiation(row):
    _run_cases(cen.cases(row), split=False)


@pytest.mark.parametrize("row", cen.MIXED_ROWS, ids=[_kid(r[3]) for r in cen.MIXED_ROWS])
def test_gemm_tail_split_instantiation(row):
    """Full rounds of the head tile and the remaining rows as lower tiles in one grid; the partial rows of the LayerNorm-backward
    epilogues are numbered through both parts (a NaN partial row - one nobody wrote - fails the sum)."""
    fam, pro, epi, mixed, head, (nf, mf1, mf2, pf1, pf2), (nr, mr1, mr2, pr1, pr2) = row
    _run_cases(cen.cases((fam, pro, epi, "", head, (nf, mf1, mf2), (nr, mr1, mr2))), split=True)


@pytest.mark.parametrize("row", cen.SEG_ROWS, ids=[_kid(r[3]) for r in cen.SEG_ROWS])
def test_gemm_node_aligned_instantiation(row):
    """One workgroup per node-aligned tile: a 60- and a 96-in-degree node (chunk tiles, their sums combined in the launch),
    isolated nodes, a tile slot without rows that owns two ghost nodes (their aggregate: zeros) and an empty slot."""
    fam, pro, epi, kernel, nf, nr = row
    gr = cen.seg_graph(DEV, 11)
    E = gr["E"]
    specs = cen.cases((fam, pro, epi, "", kernel, (nf, E, E), (nr, E, E)))
    for s in specs:
        s["graph"] = gr
    _run_cases(specs, split=False)


@pytest.mark.parametrize("row", cen.PAIR_ROWS, ids=[_kid(r[0]) for r in cen.PAIR_ROWS])
def test_gemm_pair_instantiation(row):
    """dosx_gemm_pair: two plain W[N,K] problems in one grid at the tile height of their rows together."""
    kernel, head, extra, nf, nr, m1, m2 = row
    o, lib = ops(), _lib()
    for N, (k_a, k_b), k1 in ((nf, (100, 160), 0), (nr, (4, 64), 20)):
        specs = []
        for i, (M, K) in enumerate(((m1, k_a), (m2, k_b))):
            s = dict(M=M, N=N, K=K, wl=0, vec=1, pro="NONE", epi="BIAS_ACT", kernel=head, family="plain_nk", a_left=4,
                     bias=i == 0, act=1 + i, res=i == 1, seed=i)
            if i == 1 and k1:
                s["k1"] = k1
            if extra:
                s["norm"], s["stats"] = True, N == nf and i == 0
            elif N <= 128:
                s["stats"] = i == 1
            specs.append(s)
        ts = [cen.make_inputs(s, DEV) for s in specs]
        both = cen.fake_desc(m1 + m2, N, 64, "plain_nk", "NONE", "BIAS_ACT", extra)
        assert cen.kernel_name(lib, both) == head
        gots, intacts = cen.run_pair(o, lib, specs, ts)
        for s, t, got, intact in zip(specs, ts, gots, intacts):
            _judge(s, got, cen.reference(s, t), intact, kernel + " / " + _what(s), t)


def test_gemm_pair_of_two_tile_heights():
    """dosx_gemm_pair on two PRELU_BWD problems: 16-row tiles for the first, 48-row tiles for the second, one grid
    (gemm_mixed_kernel<0, 3, 1, 1, 0, 1, 5>), partial rows numbered per problem."""
    kernel, head_a, head_b, N, m1, m2 = cen.PAIR_MIXED
    o, lib = ops(), _lib()
    for k_a, k_b in ((100, 160), (4, 64)):
        specs = [dict(M=M, N=N, K=K, wl=1, vec=1, pro="NONE", epi="PRELU_BWD", kernel=h, family="bwd", a_left=4, partials=True, seed=i)
                 for i, (M, K, h) in enumerate(((m1, k_a, head_a), (m2, k_b, head_b)))]
        ts = [cen.make_inputs(s, DEV) for s in specs]
        for s in specs:
            assert cen.kernel_name(lib, cen.fake_desc(s["M"], N, 64, "bwd", "NONE", "PRELU_BWD")) == s["kernel"]
        gots, intacts = cen.run_pair(o, lib, specs, ts)
        for s, t, got, intact in zip(specs, ts, gots, intacts):
            _judge(s, got, cen.reference(s, t), intact, kernel + " / " + _what(s), t)
