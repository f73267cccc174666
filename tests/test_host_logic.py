"""CPU tests of the host-side logic: batch container / CSR metadata, drop-in module structure,
flat-parameter storage, data-parallel sharding."""
import numpy as np
import pytest
import torch

from dostransformer_amd import synth
from dostransformer_amd.batch import CrystalBatch, collate, graph_meta, split_crystals
from dostransformer_amd.dist import shard_batch, shard_bounds


def test_batch_mapping_and_attribute_protocol():
    g = synth.phonon_batch(4, seed=1, dtype=torch.float64)
    assert "batch" in g and "edge_index" in g and "pos" not in g          # DOSTransformer_phonon.py:48-56
    assert g["edge_vec"] is g.edge_vec and g.x.shape[1] == 118 and g.phdos.shape == (4, 51)
    assert g.system.shape == (4,) and g.system.dtype == torch.int64
    e = synth.edos_batch(3, seed=2)
    assert e.glob.shape == (6,) and e.y_ft.shape == (3 * 201,) and len(e.mp_id) == 3 and e.x.shape[1] == 200
    counts = torch.bincount(e.batch)
    ptr = torch.cumsum(counts, 0)
    assert torch.all(e.x[ptr - 1] == 0)                                    # phantom all-zero node per crystal
    assert not torch.isin(ptr - 1, e.edge_index.flatten()).any()           # ... and it is isolated
    g.to("cpu")


@pytest.mark.parametrize("sort_edges", [True, False])
def test_csr_metadata(sort_edges):
    g = synth.phonon_batch(5, seed=3, dtype=torch.float32, sort_edges=sort_edges)
    m = graph_meta(g)
    N, E, B = m.num_nodes, m.num_edges, m.num_graphs
    src, dst = m.src.long(), m.dst.long()
    assert torch.all(dst[1:] >= dst[:-1])
    ei = g.edge_index if m.edge_perm is None else g.edge_index[:, m.edge_perm]
    assert torch.equal(ei[0], src) and torch.equal(ei[1], dst)
    rp = m.rowptr_dst.long()
    for n in range(N):
        assert torch.all(dst[rp[n]:rp[n + 1]] == n)
    assert rp[-1] == E
    rs = m.rowptr_src.long()
    ps = m.perm_src.long()
    for n in range(N):
        assert torch.all(src[ps[rs[n]:rs[n + 1]]] == n)
    assert sorted(ps.tolist()) == list(range(E))
    gp = m.graph_ptr.long()
    assert gp[-1] == N and m.n_max == int((gp[1:] - gp[:-1]).max())
    pos = torch.arange(N) - gp[m.node_graph.long()]
    assert torch.equal(m.dense_row.long(), pos * B + m.node_graph.long())
    deg = torch.bincount(dst, minlength=N).clamp(min=1).float()
    assert torch.allclose(m.inv_deg, 1.0 / deg)
    with pytest.raises(ValueError):
        collate(split_crystals(g), n_max=1)


def test_foreign_batch_object_gets_metadata():
    g = synth.edos_batch(3, seed=4, sort_edges=False)

    class Foreign:            # e.g. a PyG Batch: attributes only
        pass
    f = Foreign()
    for k in g.keys():
        setattr(f, k, g[k])
    m = graph_meta(f)
    assert m.num_graphs == 3 and m.edge_perm is not None and m.num_edges == g.edge_index.shape[1]


def test_split_collate_roundtrip():
    g = synth.edos_batch(4, seed=5)
    g2 = collate(split_crystals(g))
    for k in ("x", "edge_index", "edge_attr", "glob", "y_ft", "system", "batch"):
        assert torch.equal(g[k], g2[k]), k


def test_shard_bounds_cover_and_balance():
    for n, w in [(64, 8), (8, 8), (512, 8), (10, 3), (5, 2)]:
        ne = np.random.RandomState(n).randint(40, 240, size=n).tolist()
        b = shard_bounds(ne, w)
        assert b[0][0] == 0 and b[-1][1] == n and all(b[i][1] == b[i + 1][0] for i in range(w - 1))
        assert all(hi > lo for lo, hi in b)
        loads = [sum(ne[lo:hi]) for lo, hi in b]
        if n >= 8 * w:
            assert max(loads) < 1.35 * sum(ne) / w
    cs = synth.phonon_crystals(16, seed=6, dtype=torch.float32)
    n_max = max(c["x"].shape[0] for c in cs)
    shards = [shard_batch(cs, 4, r) for r in range(4)]
    assert sum(s.num_graphs for s in shards) == 16 and all(s.meta.n_max == n_max for s in shards)


def test_flat_params_layout_and_dead_parameters():
    from dostransformer_amd._fused import FlatParams, is_dead_param
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(0)
    model = DOSTransformer_phonon(3, 2, 118, 4, 16, "cpu", 0.0)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    fp = FlatParams(model, torch.device("cpu"))
    after = model.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    dead = [n for n, _ in model.named_parameters() if is_dead_param(n)]
    n_dead = sum(p.numel() for n, p in model.named_parameters() if is_dead_param(n))
    assert "alpha" in dead and any("node_mlp_1" in d for d in dead) and any("in_proj_weight" in d for d in dead)
    assert all(n not in fp.P for n in dead) and n_dead > 0
    for n, p in model.named_parameters():
        if n in fp.P:
            assert p.data_ptr() == fp.P[n].data_ptr() and fp.G[n].shape == p.shape
            assert (p.data_ptr() - fp.flat.data_ptr()) % 256 == 0
    # in-place updates of the flat buffer are what the module sees (fused AdamW writes there)
    fp.flat.add_(1.0)
    assert torch.allclose(model.fc.weight, before["fc.weight"] + 1.0)
    assert fp.intact(torch.device("cpu"))
    model.double()
    assert not fp.intact(torch.device("cpu"))            # .to()/.double() re-homes parameters -> re-flatten


def test_drop_in_aliases():
    import sys
    import dostransformer_amd
    dostransformer_amd.install_dropin()
    from layers import TransformerEncoder                                   # reference: DOSTransformer.py:6
    from embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon  # reference: main_phDOS.py:67
    from embedder_eDOS.DOSTransformer import DOSTransformer                 # reference: main_eDOS.py:68
    from embedder_eDOS.graphnetwork import Graphnetwork
    from embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    assert TransformerEncoder.__module__.startswith("dostransformer_amd")
    for k in ("layers", "embedder_phDOS", "embedder_eDOS"):
        sys.modules.pop(k, None)


def test_flat_params_bucket_layout():
    """[last = encoders + layer 0 | mid = rest of the GNN trunk | early = the rest], all aligned, every live parameter exactly once."""
    import torch
    from dostransformer_amd._fused import FlatParams, is_dead_param, is_last_param, is_late_param
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    model = DOSTransformer_phonon(3, 1, 118, 4, 16, "cpu", 0.0)
    fp = FlatParams(model, torch.device("cpu"))
    live = [n for n, _ in model.named_parameters() if not is_dead_param(n)]
    assert sorted(fp.names) == sorted(live)
    flags = [is_late_param(n) for n in fp.names]
    assert flags == sorted(flags, reverse=True) and any(flags) and not all(flags)      # late block first
    for n, o in zip(fp.names, fp.offsets):
        assert (o < fp.n_late) == is_late_param(n) and o % 64 == 0
    assert fp.n_late % 64 == 0 and 0 < fp.n_late < fp.total
    # the GNN trunk's slice again in two: what is final only at the end of the backward pass (encoders, layer 0) comes first
    for n, o in zip(fp.names, fp.offsets):
        assert (o < fp.n_last) == is_last_param(n)
    assert fp.n_last % 64 == 0 and 0 < fp.n_last < fp.n_late
    mid = [n for n, o in zip(fp.names, fp.offsets) if fp.n_last <= o < fp.n_late]
    assert any(n.startswith("GN_decoder.") for n in mid) and any(n.startswith("stacked_processor.2.") for n in mid)
    assert not any(n.startswith(("GN_encoder.", "stacked_processor.0.")) for n in mid)
    # at the headline shape (hidden 128, 3 layers) the exposed bucket is 1.12 MB of the trunk's 3.04 MB
    fp2 = FlatParams(DOSTransformer_phonon(3, 2, 118, 4, 128, "cpu", 0.0), torch.device("cpu"))
    assert 4 * fp2.n_last == 1121280 and 4 * (fp2.n_late - fp2.n_last) == 1916416 and 4 * (fp2.total - fp2.n_late) == 3501056


def test_checkpoint_is_read_without_unpickling_objects(tmp_path):
    """checkpoint.load uses weights_only=True: a file carrying an arbitrary pickled object is refused unless
    the caller opts in; our own format (tensors / str / int / float / tuple / dict) round-trips."""
    from dostransformer_amd import checkpoint
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(0)
    m = DOSTransformer_phonon(3, 1, 118, 4, 16, "cpu", 0.0)
    p = str(tmp_path / "a.pt")
    checkpoint.save(p, m, extra={"epoch": 3, "note": "x"})
    m2 = DOSTransformer_phonon(3, 1, 118, 4, 16, "cpu", 0.0)
    assert checkpoint.load(p, m2) == {"epoch": 3, "note": "x"}
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k

    class Evil:
        def __reduce__(self):
            return (print, ("pwned",))
    bad = str(tmp_path / "bad.pt")
    torch.save({"model": m.state_dict(), "extra": {"x": Evil()}}, bad)
    with pytest.raises(Exception):
        checkpoint.load(bad, m2)


def test_padded_copy_cache_is_invalidated_by_assignment():
    g = synth.phonon_batch(2, seed=5, dtype=torch.float32)
    object.__setattr__(g, "_dosx_padded", ("bucket", "copy"))
    g.to("cpu")
    assert g._dosx_padded is not None                      # nothing moved
    g.x = g.x * 2
    assert g._dosx_padded is None
    object.__setattr__(g, "_dosx_padded", ("bucket", "copy"))
    g["edge_vec"] = g.edge_vec + 1
    assert g._dosx_padded is None
    object.__setattr__(g, "_dosx_padded", ("bucket", "copy"))
    g.to("cpu", torch.float64)
    assert g._dosx_padded is None and g.x.dtype == torch.float64


def test_shard_batch_records_the_global_batch_size():
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    cs = synth.phonon_crystals(7, seed=4, dtype=torch.float32)
    g = shard_batch(cs, 2, 1)
    assert g.n_global == 7
    gp = pad_batch(g, *bucket_sizes(g.meta.num_nodes, g.meta.num_edges))
    assert gp.n_global == 7 and gp.clone().n_global == 7
    assert collate(cs).n_global is None


def test_optimizer_moments_follow_rehomed_parameters():
    """Trainer._state carries m / v BY NAME when the flat parameter buffer is rebuilt (CPU-only: pure bookkeeping)."""
    from dostransformer_amd._fused import FlatParams
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.train import Trainer
    torch.manual_seed(0)
    m = DOSTransformer_phonon(3, 1, 118, 4, 16, "cpu", 0.0)
    tr = Trainer(m)
    fp = m.flat_params()
    mm, vv = tr._state(fp)
    mm.copy_(torch.arange(mm.numel(), dtype=torch.float32))
    vv.fill_(2.0)
    tr.step_count = 5
    want = {n: mm[o:o + fp.P[n].numel()].clone() for n, o in zip(fp.names, fp.offsets)}
    fp2 = FlatParams(m, torch.device("cpu"), extra_dead=("fc.bias",))       # a different layout (one parameter less)
    m2, v2 = tr._state(fp2)
    assert tr.step_count == 5 and m2.numel() == fp2.total
    for n, o in zip(fp2.names, fp2.offsets):
        assert torch.equal(m2[o:o + fp2.P[n].numel()], want[n]), n
        assert float(v2[o:o + fp2.P[n].numel()].min()) == 2.0


def test_seg_tiles_host_properties():
    """Node-aligned row tiles of the message GEMM (batch.seg_tiles_host), incl. over-full nodes (> 48 incoming edges) cut into
    chunk tiles and isolated nodes: monotone boundaries, <= 48 rows per tile, every node owned exactly once, every edge covered
    exactly once, chunk k of a node starts 48*k rows into its segment whatever surrounds it, consecutive tiles hold more than
    48 rows together (what seg_tile_bound relies on)."""
    from dostransformer_amd.batch import SEG_TILE_ROWS, seg_tile_bound, seg_tiles_host
    R = SEG_TILE_ROWS
    rng = np.random.default_rng(0)
    for trial in range(400):
        n = int(rng.integers(1, 30))
        deg = rng.integers(0, 30, size=n)
        deg[rng.random(n) < 0.3] = 0
        for _ in range(int(rng.integers(0, 5))):
            deg[int(rng.integers(0, n))] = int(rng.choice([48, 49, 60, 96, 97, 144, 145, 200]))
        rp = np.concatenate([[0], np.cumsum(deg)])
        t = seg_tiles_host(rp)
        assert t.shape[0] == 3 and t.dtype == np.int32
        eb, nb, pi = t
        T = t.shape[1] - 1
        assert eb[0] == 0 and nb[0] == 0 and eb[-1] == rp[-1] and nb[-1] == n and pi[-1] == 0
        assert (np.diff(eb) >= 0).all() and (np.diff(nb) >= 0).all() and np.diff(eb).max(initial=0) <= R
        cover, owned = np.zeros(n, int), np.zeros(n, int)
        for i in range(T):
            lo, hi = nb[i], nb[i + 1]
            whole = range(lo, hi)
            if pi[i]:
                ci, nc = pi[i] >> 16, pi[i] & 0xffff
                assert deg[lo] > R and nc == -(-deg[lo] // R) and 0 <= ci < nc
                assert eb[i] == rp[lo] + ci * R                        # the chunk is cut from the START of the node's segment
                rows = min(rp[lo + 1], eb[i + 1]) - eb[i]
                assert rows == (R if ci < nc - 1 else deg[lo] - ci * R)
                assert (hi == lo) if ci < nc - 1 else (hi >= lo + 1)
                cover[lo] += rows
                owned[lo] += ci == nc - 1
                whole = range(lo + 1, hi)
            for k in whole:
                assert deg[k] <= R and rp[k] >= eb[i] and rp[k + 1] <= eb[i + 1]
                cover[k] += deg[k]
                owned[k] += 1
        assert (cover == deg).all() and (owned == 1).all()
        rows = np.diff(eb)
        assert all(i == 0 and rows[0] == 0 for i in range(T - 1) if rows[i] + rows[i + 1] <= R)
        assert T <= seg_tile_bound(n, int(rp[-1]), 1)


def test_size_policies_of_the_factored_forms():
    """The size limits that switch the EdgeModel between its fused and its factored forms, and the tail split of the unfused
    feed-forward layers (functional._factor_edge / _factor_last / _ffn_tail_start): the BASELINE shapes land where DESIGN.md
    says they do."""
    from dostransformer_amd import functional as Fn
    # Phonon-DOS benchmark shape (H 128, ~9000 edges): factored first Linear since round 5 (gathers / node sums inside the GEMM
    # epilogues), per-edge last layer; the CPU-reference shape (H 64, ~1100 edges: 0.05 GF) keeps the gathered-concat GEMM;
    # Electron-DOS (H 256, 17880 edges; the 32-crystal shard has about half of them): factored first Linear and aggregate-first
    # last layer
    assert Fn._factor_edge(9000, 128) and not Fn._factor_last(9000, 128)
    assert not Fn._factor_edge(1100, 64) and not Fn._factor_last(1100, 64)

    class _M:                                                  # a batch with node-aligned row tiles: the one-launch kernels of
        seg_tile = object()                                    # csrc/edge_mlp.hip take hidden 64 / 128 at EVERY size
    assert Fn._factor_edge(1100, 64, _M()) and Fn._factor_edge(140, 128, _M())
    assert not Fn._factor_edge(300, 256, _M()) and Fn._factor_edge(1100, 256, _M())    # hidden 256: the epilogue forms, by size (0.5 GF)
    assert Fn._factor_edge(17880, 256) and Fn._factor_last(17880, 256)
    assert Fn._factor_edge(8900, 256) and Fn._factor_last(8900, 256)
    assert not Fn._factor_last(17880, 384)                    # 2 * hidden > 512: the unfused wide-row path keeps the per-edge form
    # output heads: factored at the Electron-DOS shapes (B * S = 64 * 201 and 32 * 201 rows, H 256), not at 64 * 51 rows / H 128
    assert Fn._factor_heads(64 * 201, 256) and Fn._factor_heads(32 * 201, 256)
    assert not Fn._factor_heads(64 * 51, 128) and not Fn._factor_heads(51, 128)
    # feed-forward tail: 25728 = 3 full rounds of 8192 rows + 1152; 12864 = 1 round + 4672 (too large a tail); small problems never
    assert Fn._ffn_tail_start(25728, 256) == 24576
    assert Fn._ffn_tail_start(12864, 256) == 0
    assert Fn._ffn_tail_start(8192, 256) == 0 and Fn._ffn_tail_start(6528, 256) == 0
    assert Fn._ffn_tail_start(25728, 384) == 0                # 3 column tiles do not divide the 256 CUs: no split
    assert Fn._ffn_tail_start(16384 + 100, 512) == 16384      # 4 column tiles: rounds of 4096 rows
    # round 5: the NodeModel FORWARD runs as one launch up to hidden 256 (1554 nodes of the Electron-DOS batch), its backward only up
    # to hidden 128; unfused encoder layers (hidden 256) take LN1 from the attention kernel; the measured-neutral forms are off
    from dostransformer_amd import ops
    assert ops.mlp_ln_fwd_supported(1554, 512, 512, 256) and not ops.mlp_ln_supported(1554, 512, 512, 256)
    assert ops.mlp_ln_supported(450, 256, 256, 128) and not ops.mlp_ln_fwd_supported(5000, 256, 256, 128)
    _assert_switch_surface()           # ... and are no switches any more


def test_attention_forms_at_the_baseline_encoder_shapes():
    """functional.attention_form_fwd / attention_bwd_in_ffn (host-only: switches + the library's support functions) at the
    BASELINE encoder shapes (Sq, Bq, Nk, Bk, H): the Phonon-DOS step (cfg2) has no stand-alone attention launch left, forward
    or backward; hidden 256 (Electron-DOS) keeps the attention kernels; relu / res dropout runs every layer unfused."""
    from dostransformer_amd import functional as Fn
    A = Fn.AttForm
    phonon = {"cross": ((51, 64, 12, 64, 128), A.ROWS_IN_FFN), "self": ((51, 128, 51, 128, 128), A.ALIGNED_IN_FFN),
              "source": ((51, 128, 12, 64, 128), A.ALIGNED_IN_FFN)}
    edos = {"cross": (201, 64, 30, 64, 256), "self": (201, 128, 201, 128, 256), "source": (201, 128, 30, 64, 256)}   # (201 bins; any atom count)
    fdrop = (0.1, 0.1, None, 0)
    for name, ((Sq, Bq, Nk, Bk, H), want) in phonon.items():
        assert Fn.attention_form_fwd(Sq * Bq, Sq, Bq, Nk, H, None) is want, name
        assert Fn.attention_form_fwd(Sq * Bq, Sq, Bq, Nk, H, fdrop) is A.STANDALONE, name
        assert Fn.attention_bwd_in_ffn(Sq, Bq, Nk, H, fdrop=False), name
        assert not Fn.attention_bwd_in_ffn(Sq, Bq, Nk, H, fdrop=True), name
    for name, (Sq, Bq, Nk, Bk, H) in edos.items():
        assert Fn.attention_form_fwd(Sq * Bq, Sq, Bq, Nk, H, None) is A.STANDALONE, name
        assert Fn.attention_form_fwd(Sq * Bq, Sq, Bq, Nk, H, fdrop) is A.STANDALONE, name
        assert not Fn.attention_bwd_in_ffn(Sq, Bq, Nk, H, fdrop=False), name
    for Sq, Bq, Nk, H in ((51, 64, 12, 256), (7, 3, 1, 256), (51, 128, 51, 256)):          # hidden 256 at any shape
        assert Fn.attention_form_fwd(Sq * Bq, Sq, Bq, Nk, H, None) is A.STANDALONE
        assert not Fn.attention_bwd_in_ffn(Sq, Bq, Nk, H, fdrop=False)


def test_backward_forms_at_the_baseline_encoder_shapes():
    """functional.attention_form_bwd / ffn_form name what encoder_bwd dispatches on.  Expected values: the booleans the unnamed
    code computed (attention_bwd_in_ffn, dosx_attention_pkv_supported), evaluated on the CPU build.  The Phonon-DOS step runs
    every attention backward inside its layer's dosx_ffn_bwd; hidden 256 splits the 201-key self attention and runs the 30-key
    cross attentions as one launch; relu / res dropout never rides in the feed-forward launch."""
    from dostransformer_amd import functional as Fn, ops
    A, F = Fn.AttBwdForm, Fn.FfnForm
    shapes = {"phonon cross": ((51, 64, 12, 128), A.IN_FFN, A.ONE_LAUNCH), "phonon self": ((51, 128, 51, 128), A.IN_FFN, A.ONE_LAUNCH),
              "phonon source": ((51, 128, 12, 128), A.IN_FFN, A.ONE_LAUNCH), "edos cross": ((201, 64, 30, 256), A.ONE_LAUNCH, A.ONE_LAUNCH),
              "edos self": ((201, 128, 201, 256), A.SPLIT, A.SPLIT), "edos source": ((201, 128, 30, 256), A.ONE_LAUNCH, A.ONE_LAUNCH)}
    for name, ((Sq, Bq, Nk, H), want, want_fdrop) in shapes.items():
        assert Fn.attention_form_bwd(Sq, Bq, Nk, H, False) is want, name
        assert Fn.attention_form_bwd(Sq, Bq, Nk, H, True) is want_fdrop, name
    assert ops.attention_pkv_supported(30, 256) and not ops.attention_pkv_supported(201, 256)
    assert [Fn.ffn_form(H, False) for H in (32, 64, 128, 256, 512)] == [F.ONE_LAUNCH] * 3 + [F.GEMMS] * 2
    assert all(Fn.ffn_form(H, True) is F.DROPOUT for H in (32, 128, 256))
    # (Sq, Bq) on either side of the 256-workgroup bound of the in-ffn form; key counts around the 16- and 64-key limits
    assert ops.ffn_att_bwd_partial_rows(51, 64) == Fn._ATT_ALIGNED_MAX_WGS < ops.ffn_att_bwd_partial_rows(51, 400)
    for H in (32, 64, 128, 256):
        for Nk in (1, 16, 17, 64, 65, 201):
            for Sq, Bq in ((51, 64), (51, 400)):
                for fdrop in (False, True):
                    form = Fn.attention_form_bwd(Sq, Bq, Nk, H, fdrop)
                    assert Fn.attention_bwd_in_ffn(Sq, Bq, Nk, H, fdrop) == (form is A.IN_FFN), (H, Nk, Sq, Bq, fdrop)
                    assert (form is A.IN_FFN) == (H in (64, 128) and Nk <= 64 and Bq == 64 and not fdrop), (H, Nk, Sq, Bq, fdrop)
                    assert (form is A.SPLIT) == (Nk > 64), (H, Nk, Sq, Bq, fdrop)
    with Fn.forms(_FUSED_ATT_BWD=False):                      # (derived when asked, from the switches as they are then)
        assert Fn.attention_form_bwd(51, 64, 12, 128, False) is A.ONE_LAUNCH
    # one query-only rule: the layer condition is shared, the trunk condition is each caller's
    names = [f"{p}.layers.{t}.layer_norms.0.{w}" for p in ("transformer", "transformer_self", "transformer_source") for t in range(2)
             for w in ("weight", "bias")] + ["GN_encoder.node_encoder.0.weight", "stacked_processor.0.x", "GN_decoder.0.weight"]
    trunk = frozenset(n for n in names if n.startswith(Fn._TRUNK))
    for pre in ("transformer", "transformer_self", "transformer_source"):
        ln0 = frozenset(f"{pre}.layers.1.layer_norms.0.{w}" for w in ("weight", "bias"))
        for frozen in (trunk | ln0, ln0, trunk, trunk | {sorted(ln0)[0]}):
            for t in range(2):
                layer = Fn._keys_unread_by(frozen, pre, t)
                assert layer == (pre != "transformer_self" and t == 1 and ln0 <= frozen), (pre, t, sorted(frozen))
                assert Fn.attention_query_only(names, frozen, pre, t) == (Fn.trunk_cut(names, frozen) and layer), (pre, t, sorted(frozen))


def test_forms_scope_sets_and_restores_the_policy_globals():
    """functional.forms: the override scope of the tests - restores on normal exit and on an exception, a nested scope hands back
    the OUTER scope's value, and a name that is not one of the module's policy globals is refused (nothing set)."""
    from dostransformer_amd import functional as Fn
    before = (Fn._FFN_MULTI, Fn._ATT_FFN_MAX_ROWS, Fn._FACTOR_MIN_GF)
    assert before == (True, 4096, 0.5)
    with Fn.forms(_FFN_MULTI=False, _ATT_FFN_MAX_ROWS=0):
        assert (Fn._FFN_MULTI, Fn._ATT_FFN_MAX_ROWS, Fn._FACTOR_MIN_GF) == (False, 0, 0.5)
        assert Fn.attention_form_fwd(51 * 64, 51, 64, 12, 128, None) is Fn.AttForm.ALIGNED_IN_FFN        # (the functions read them)
        with Fn.forms(_ATT_FFN_MAX_ROWS=7, _FACTOR_MIN_GF=0.0):
            assert (Fn._FFN_MULTI, Fn._ATT_FFN_MAX_ROWS, Fn._FACTOR_MIN_GF) == (False, 7, 0.0)
        assert (Fn._FFN_MULTI, Fn._ATT_FFN_MAX_ROWS, Fn._FACTOR_MIN_GF) == (False, 0, 0.5)
    assert (Fn._FFN_MULTI, Fn._ATT_FFN_MAX_ROWS, Fn._FACTOR_MIN_GF) == before
    with pytest.raises(ZeroDivisionError):
        with Fn.forms(_FFN_MULTI=False, _FUSED_ATT_BWD=False):
            assert not Fn._FUSED_ATT_BWD
            1 / 0
    assert Fn._FFN_MULTI is True and Fn._FUSED_ATT_BWD is True
    for bad in ("_NO_SUCH_FORM", "DROP_MASK_LOG", "forms", "_rows32", "ops"):
        with pytest.raises(AttributeError):
            with Fn.forms(_FFN_MULTI=False, **{bad: 1}):
                pass
        assert Fn._FFN_MULTI is True
    assert not hasattr(Fn, "_NO_SUCH_FORM") and Fn.DROP_MASK_LOG is None


def test_ffn_descriptors_take_the_head_fields_by_name():
    """ops._ffn_desc / _ffn_bwd_desc (descriptor construction without a launch): every DosxFfn / DosxFfnBwd ``fin_*`` field holds
    the address of the ops.Head field of that name, with and without the output layer; the attention records likewise."""
    from dostransformer_amd import ops
    H, S, Bq, Nk, Bk = 8, 5, 3, 4, 3
    M = S * Bq
    t = lambda *shape: torch.zeros(*shape)              # distinct CPU allocations: only their addresses are read
    x, stats, g, b, w1, b1, w2, b2, h, out = t(M, H), t(M, 2), t(H), t(H), t(4 * H, H), t(4 * H), t(H, 4 * H), t(H), t(M, 4 * H), t(M, H)
    fwd = ops.Head(gamma=t(H), beta=t(H), xhat=t(M, H), rstd=t(M), w=t(H), b=t(1), dos=t(Bq, S), S=S, Bq=Bq)
    a = ops._ffn_desc(M, H, x, stats, g, b, w1, b1, w2, b2, h, None, fwd, None)
    for name in ("gamma", "beta", "xhat", "rstd", "w", "b", "dos"):
        assert getattr(a, "fin_" + name) == getattr(fwd, name).data_ptr(), name
    assert (a.fin_S, a.fin_Bq, a.out) == (S, Bq, None)
    assert len({getattr(a, "fin_" + n) for n in ("gamma", "beta", "xhat", "rstd", "w", "b", "dos")}) == 7
    ln = ops.Head(t(H), t(H), t(M, H), t(M))            # the final LayerNorm alone: no output-layer field is set
    a = ops._ffn_desc(M, H, x, stats, g, b, w1, b1, w2, b2, h, out, ln, None)
    assert [getattr(a, "fin_" + n) for n in ("gamma", "beta", "xhat", "rstd")] == [v.data_ptr() for v in ln[:4]]
    assert (a.fin_w, a.fin_b, a.fin_dos, a.fin_S, a.fin_Bq) == (None, None, None, 0, 0) and a.out == out.data_ptr()
    bare = ops._ffn_desc(M, H, x, stats, g, b, w1, b1, w2, b2, h, out, tuple(ln[:4]), None)      # Head's required fields, unnamed
    assert all(getattr(bare, "fin_" + n) == getattr(a, "fin_" + n) for n in ("gamma", "beta", "xhat", "rstd", "w", "dos", "S"))
    with pytest.raises(ValueError):                     # ... and nothing longer: the output layer goes in by name only
        ops._ffn_desc(M, H, x, stats, g, b, w1, b1, w2, b2, h, None, tuple(fwd[:4]) + (fwd.w, fwd.b, fwd.dos, S, Bq), None)
    a = ops._ffn_desc(M, H, x, stats, g, b, w1, b1, w2, b2, h, out, None, None)
    assert (a.fin_gamma, a.fin_xhat, a.att_kvhat, a.att_Nk) == (None, None, None, 0)

    dy, dh, dx, part = t(M, H), t(M, 4 * H), t(M, H), t(1, 5 * H + 4)
    bwd = ops.Head(gamma=t(H), beta=t(H), xhat=t(M, H), rstd=t(M), w=t(H), ddos=t(Bq, S), dy=t(M, H), S=S, Bq=Bq,
                   keys=("ln.weight", "ln.bias", "out.weight", "out.bias"))
    d = ops._ffn_bwd_desc(M, H, None, h, x, stats, g, w1, w2, dh, dx, part, bwd, None)
    for name in ("gamma", "xhat", "rstd", "dy", "ddos", "w", "beta"):
        assert getattr(d, "fin_" + name) == getattr(bwd, name).data_ptr(), name
    assert (d.fin_S, d.fin_Bq, d.dy, d.lddy) == (S, Bq, None, H)
    lnb = ops.Head(t(H), t(H), t(M, H), t(M), dy=t(M, H))
    d = ops._ffn_bwd_desc(M, H, dy, h, x, stats, g, w1, w2, dh, dx, part, lnb, None)
    for name in ("gamma", "xhat", "rstd", "dy"):
        assert getattr(d, "fin_" + name) == getattr(lnb, name).data_ptr(), name
    assert (d.fin_ddos, d.fin_w, d.fin_beta, d.fin_S, d.fin_Bq) == (None, None, None, 0, 0) and d.dy == dy.data_ptr()

    kp = torch.zeros(Bk + 1, dtype=torch.int32)
    af = ops.AttFwd(kvhat=t(Nk * Bk, H), gamma0=t(H), beta0=t(H), Nk=Nk, Bk=Bk, Bq=Bq, Sq=S, qs=Bq, qb=1, probs=t(Bq, S, Nk),
                    qstats=t(M, 2), x1=t(M, H), st1=t(M, 2), mask=t(Bq, S, Nk), aligned=True, key_ptr=kp)
    a = ops._ffn_desc(M, H, x, None, g, b, w1, b1, w2, b2, h, out, None, af)
    for name in ("kvhat", "gamma0", "beta0", "probs", "qstats", "x1", "st1", "mask", "key_ptr"):
        assert getattr(a, "att_" + name) == getattr(af, name).data_ptr(), name
    assert (a.att_Nk, a.att_Bk, a.att_Bq, a.att_Sq, a.att_qs, a.att_qb, a.att_aligned) == (Nk, Bk, Bq, S, Bq, 1, 1)
    ab = ops.AttBwd(x=t(M, H), kvhat=t(Nk * Bk, H), gamma0=t(H), beta0=t(H), probs=t(Bq, S, Nk), qstats=t(M, 2), dxin=t(M, H),
                    partials_q=4096, partials_kv=8192, dkv_part=t(Bq * Nk, H), dkv_cnt=12288, dkvhat=t(Nk * Bk, H), accumulate=1,
                    Nk=Nk, Bk=Bk, Bq=Bq, Sq=S, qs=Bq, qb=1)
    d = ops._ffn_bwd_desc(M, H, dy, h, x, stats, g, w1, w2, dh, None, part, None, ab)
    for name in ("x", "kvhat", "gamma0", "beta0", "probs", "qstats", "dxin", "dkv_part", "dkvhat"):
        assert getattr(d, "att_" + name) == getattr(ab, name).data_ptr(), name
    assert (d.att_partials_q, d.att_partials_kv, d.att_dkv_cnt, d.att_dkv_accumulate) == (4096, 8192, 12288, 1)
    assert (d.att_mask, d.att_key_ptr, d.dx) == (None, None, None) and (d.att_Nk, d.att_Bk, d.att_Bq, d.att_Sq) == (Nk, Bk, Bq, S)
    with pytest.raises(TypeError):
        ops.AttFwd(kvhat=af.kvhat, gamma0=af.gamma0, beta0=af.beta0, Nk=Nk, Bk=Bk, Bq=Bq, Sq=S, qs=Bq, qb=1, probs=af.probs,
                   qstats=af.qstats, x1=af.x1, st1=af.st1, msk=None)                     # a misspelt optional field is an error
    with pytest.raises(TypeError):                                                       # ... and so is an unknown gemm keyword
        ops.gemm(2, 2, [ops.seg(t(2, 2))], t(2, 2), t(2, 2), biass=None)


_ENV_SWITCHES ={"DOSX_LIB", "DOSX_FFN_BF16X3", "DOSX_DP_MID_BUCKET", "DOSX_DP_CHECK"}
_REMOVED_SWITCHES = {
    "functional": ("_NODE_CHAIN", "_FLUSH_AFTER_CHAIN", "_DENSE_CHAIN", "_SPLIT_LATE_FLUSH", "_LATE_SELF_FLUSH", "_MID_HOOK_LATE",
                   "_GNN_FLUSH_BEFORE_NODE", "_NODE_GRAD_ONE_LAUNCH", "_FACTOR_DGRAD", "_FACTOR_ONE_LAUNCH_ALWAYS", "_ENC_CS",
                   "_EDGE_ENC_ONE_LAUNCH", "_ENC_BWD_PAIR", "_PQ_IN_NODE_MLP", "_PQ_IN_NODE_MLP_CS", "_HEADS_BWD_ONE_LAUNCH",
                   "_HEADS_BWD_MAX_H", "_FUSED_FFN_BWD", "_FUSED_DKV", "_FUSED_HEAD_NORM", "_LN1_IN_ATTN", "_LN1_WGRAD", "_FFN_TAIL"),
    "ops": ("MLP_LN_CS", "MLP_LN_CS_BWD", "_LPT"),
    "train": ("_EARLY_REDUCE",),
}


def _assert_switch_surface():
    """The package reads exactly four process variables (a form choice left to a user-set variable is what bench.py has to refuse),
    and the switches whose other side was measured and rejected are gone: a new one cannot appear without this list being edited."""
    import importlib
    import pathlib
    import re
    root = pathlib.Path(__file__).resolve().parent.parent / "dostransformer_amd"
    files = sorted(root.rglob("*.py"))
    assert len(files) > 10
    names = set()
    for f in files:
        for line in f.read_text().splitlines():
            if re.search(r"environ|getenv", line):
                names |= set(re.findall(r"DOSX_[A-Z0-9_]+", line))
    assert names == _ENV_SWITCHES, sorted(names ^ _ENV_SWITCHES)
    for mod, gone in _REMOVED_SWITCHES.items():
        m = importlib.import_module("dostransformer_amd." + mod)
        assert not [n for n in gone if hasattr(m, n)], (mod, [n for n in gone if hasattr(m, n)])
    from dostransformer_amd.ops import GradSink
    assert not hasattr(GradSink, "use_wgrad_stream") and GradSink.use_side_stream is False


def _assert_library_switch_surface():
    """The C library reads no process variable outside the diagnostic stamps build: every getenv of csrc/ lies inside an
    `#ifdef DOSX_STAMPS ... #endif` region (the guard logic of test_no_work_skipping_switch_ships_in_the_package).  Its runtime
    selectors are the two setters of include/dosx.h, dosx_attention_aligned_mode and dosx_set_sliver_max_gf."""
    import pathlib
    import re
    root = pathlib.Path(__file__).resolve().parent.parent / "dostransformer_amd" / "csrc"
    files = sorted(f for ext in ("*.hip", "*.cpp", "*.h") for f in root.glob(ext))
    assert len(files) > 20
    seen = 0
    for f in files:
        src = f.read_text()
        for m in re.finditer(r"getenv", src):
            guard = src.rfind("#ifdef DOSX_STAMPS", 0, m.start())
            assert guard >= 0 and src.find("#endif", guard) > m.start(), f"{f.name}: getenv outside the stamps build"
            seen += 1
    assert seen == 1                       # (DOSX_DEBUG_SKIP_WGRAD of the stamps build: the scan does see what it looks for)


def test_only_the_documented_switches_read_the_environment():
    _assert_switch_surface()
    _assert_library_switch_surface()


def test_bucket_promotion_picks_the_smallest_live_bucket_that_fits():
    """slots.promote_key: a first-time bucket runs in a live one of the same batch size / key-slot count / tiling with at
    least as many rows and at most `tol` more of either, the smallest by (edges, nodes); never in a smaller or a foreign one."""
    from dostransformer_amd.slots import promote_key
    rest = (64, 12, 64, True)
    live = [(448, 8960) + rest, (464, 9280) + rest, (480, 9600) + rest, (464, 9280, 32, 12, 32, True), (432, 8640) + rest]
    assert promote_key(live, (448, 9280) + rest, 0.08) == (464, 9280) + rest          # exact edges, one node step up
    assert promote_key(live, (448, 9000) + rest, 0.08) == (464, 9280) + rest          # (448, 8960) has too few edges
    assert promote_key(live, (432, 8640) + rest, 0.08) == (432, 8640) + rest          # itself, if it were live
    assert promote_key(live, (480, 9920) + rest, 0.08) is None                        # nothing large enough
    assert promote_key(live, (400, 8000) + rest, 0.08) == (432, 8640) + rest          # exactly 8 % more of both
    assert promote_key(live, (400, 7900) + rest, 0.08) is None                        # ... and just beyond
    assert promote_key(live, (464, 9280, 16, 12, 16, True), 0.5) is None              # other batch size: never
    assert promote_key([], (448, 8960) + rest, 0.08) is None


def test_bound_ratio_judges_each_row_on_its_own_scale():
    """tests/gpu_util.bound_ratio (the element-wise measure of the GPU kernel tests): a 1e-4 relative error in one element of a
    small row next to large rows fails it, where the global err() - max error / max of the tensor - would pass."""
    from tests.gpu_util import EPS32, bound_ratio, err
    g = torch.Generator().manual_seed(0)
    mags = torch.tensor([1e3, 1e3, 1e-2, 1e3], dtype=torch.float64)[:, None]
    ref = (torch.randn(4, 64, generator=g, dtype=torch.float64) * mags).float()           # an fp32 result ...
    scale = ref.double().abs().mean(1, keepdim=True)                                     # ... and each row's own scale
    assert bound_ratio(ref, ref.double(), scale, 8) == 0.0
    bad = ref.clone()
    bad[2, 5] *= 1 + 1e-4
    assert err(bad, ref) < 2e-5                                                          # the global measure accepts it
    assert bound_ratio(bad, ref.double(), scale, 8) > 1.0                                # the row's own scale does not
    ok = ref.clone()
    ok[2, 5] += 4 * EPS32 * float(scale[2])                                              # half the bound of c = 8
    assert 0.4 < bound_ratio(ok, ref.double(), scale, 8) <= 0.5 + 1e-6
    nan = ref.clone()
    nan[0, 0] = float("nan")
    assert bound_ratio(nan, ref.double(), scale, 8) == float("inf")
    zero = torch.zeros(3)                                                                # a zero bound demands exact zeros
    assert bound_ratio(zero, torch.zeros(3, dtype=torch.float64), 0.0, 8) == 0.0
    assert bound_ratio(zero + 1e-30, torch.zeros(3, dtype=torch.float64), 0.0, 8) == float("inf")


@pytest.mark.parametrize("kind,dtype,tiled", [("phonon", torch.float32, True), ("edos", torch.float32, False),
                                              ("phonon", torch.float64, False)])
def test_empty_slot_has_the_buffers_the_collate_kernel_fills(kind, dtype, tiled):
    """slots.Slot.empty on the CPU (no libdosx call): every field and index array DeviceDataset.collate_into writes, in the
    slot's dtype and the bucket's padded shape, and the lazily made collate scratch."""
    from dostransformer_amd.batch import seg_tile_bound
    from dostransformer_amd.slots import META_TENSORS, Slot
    B, n_pad, e_pad, n_max, Fa, Fe, S = 4, 48, 896, 19, 118, 3, 51
    slot = Slot.empty(kind, "cpu", dtype, B, n_pad, e_pad, n_max, Fa, Fe, S, tiled=tiled)
    g, m = slot.g, slot.g.meta
    want = {"x": (n_pad, Fa), "system": (B,)}
    want.update({"edge_vec": (e_pad, Fe), "phdos": (B, S)} if kind == "phonon" else
                {"edge_attr": (e_pad, Fe), "glob": (2 * B,), "y_ft": (B * S,)})
    assert list(slot.fields) == list(want)
    for k, shape in want.items():
        assert tuple(g[k].shape) == shape and g[k].dtype == (torch.int32 if k == "system" else dtype) and g[k].is_contiguous(), k
    assert (m.num_nodes, m.num_edges, m.num_graphs, m.n_max, m.edge_perm) == (n_pad, e_pad, B, n_max, None)
    shapes = {"src": e_pad, "dst": e_pad, "perm_src": e_pad, "rowptr_dst": n_pad + 1, "rowptr_src": n_pad + 1, "graph_ptr": B + 1,
              "node_graph": n_pad, "dense_row": n_pad, "inv_deg": n_pad}
    assert set(shapes) == set(META_TENSORS)
    for k, n in shapes.items():
        t = getattr(m, k)
        assert tuple(t.shape) == (n,) and t.dtype == (torch.float32 if k == "inv_deg" else torch.int32), k
    if tiled:
        assert tuple(m.seg_tile.shape) == (3, seg_tile_bound(48, 896, 4) + 1) and m.seg_tile.dtype == torch.int32
    else:
        assert m.seg_tile is None
    assert slot.real_nodes == 48
    assert (slot.prog, slot.plan, slot.graph_a, slot.graph_b, slot.keep, slot.loss, slot.out, slot.sse) == \
        (None, [], None, None, None, None, None, None)
    sc = slot.collate_scratch()
    assert {k: (tuple(v.shape), v.dtype) for k, v in sc.items()} == \
        {"small": ((4 * B + 3,), torch.int32), "node_row": ((48,), torch.int32), "edge_row": ((896,), torch.int32)}
    assert slot.collate_scratch() is sc


def _lookup_walk(cache):
    """A fixed key sequence through ``cache._lookup`` the way the trainers use it (a fresh slot is registered after its first
    step); after every call (slot_hits, slot_misses, slot_promoted, live keys, least recently used first) against the rule worked
    out by hand for max_slots = 2, promote = 0.08."""
    rest = (8, 12, 8, True)
    A, a, B, C = (400, 8000) + rest, (416, 8320) + rest, (432, 8640) + rest, (600, 12000) + rest
    walk = [
        (B, True, (0, 1, 0, [B]), None),        # nothing live to run in: recorded
        (B, True, (1, 1, 0, [B]), B),           # hit
        (a, True, (2, 1, 1, [B]), B),           # first visit, B holds it with <= 8 % more rows: promoted, not recorded
        (a, True, (2, 2, 1, [B, a]), None),     # second visit: recorded
        (B, True, (3, 2, 1, [a, B]), B),        # hit: B is the most recently used now
        (C, True, (3, 3, 1, [B, C]), None),     # no live bucket is large enough: recorded, the oldest (a) evicted
        (a, True, (3, 4, 1, [C, a]), None),     # a is gone and was seen before: recorded again, B evicted
        (C, True, (4, 4, 1, [a, C]), C),        # hit
        (A, True, (5, 4, 2, [C, a]), a),        # first visit: promoted into a (C is 50 % larger), which moves to the end
        (A, False, (5, 5, 2, [a, A]), None),    # step(batch) never promotes: recorded, C evicted
    ]
    for k, (key, allow, want, host) in enumerate(walk):
        slot = cache._lookup(key, allow_promote=allow)
        if slot is None:
            assert host is None, k
            cache._slots[key] = ("slot of", key)
        else:
            assert slot == ("slot of", host), k
        assert (cache.slot_hits, cache.slot_misses, cache.slot_promoted, list(cache._slots)) == want, k


def test_shared_lookup_counts_hits_misses_promotions_and_evicts_the_oldest():
    from collections import OrderedDict
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.slots import SlotCache
    from dostransformer_amd.train import Trainer
    from dostransformer_amd.train64 import Trainer64

    class Bare(SlotCache):
        def __init__(self):
            self._slots, self._seen, self.max_slots, self.promote = OrderedDict(), {}, 2, 0.08
            self.slot_hits = self.slot_misses = self.slot_promoted = 0
    _lookup_walk(Bare())
    torch.manual_seed(0)
    m32 = DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.0)
    m64 = DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.0).double().set_program_dtype(torch.float64)
    assert Trainer._lookup is SlotCache._lookup and Trainer64._lookup is SlotCache._lookup
    _lookup_walk(Trainer(m32, replay=True, max_slots=2, promote=0.08))
    _lookup_walk(Trainer64(m64, replay=True, bucket=(8, 128), max_slots=2, promote=0.08))


def test_the_three_trainers_share_one_step_driver():
    """step, step_accumulate, step_dataset, step_dataset_accumulate and _flat_for are written once, in trainer_base.TrainerBase:
    train.Trainer, train64.Trainer64 and train64.GraphnetworkTrainer64 resolve them to the same function objects."""
    from dostransformer_amd import train
    from dostransformer_amd.train64 import GraphnetworkTrainer64, Trainer64
    from dostransformer_amd.trainer_base import TrainerBase
    for name in ("step", "step_accumulate", "step_dataset", "step_dataset_accumulate", "_flat_for"):
        for cls in (train.Trainer, Trainer64, GraphnetworkTrainer64):
            assert getattr(cls, name) is getattr(TrainerBase, name), (cls.__name__, name)
    assert not hasattr(train, "_AdamWState")


def test_a_refused_dataset_step_leaves_the_dropout_seed_alone():
    """Every refusal that can be known before a launch comes before the seed bump: a slotted step_dataset with a foreign
    n_global raises and the seed is what it was (fp32 and float64 driver)."""
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.train import Trainer
    from dostransformer_amd.train64 import Trainer64

    class Dataset:                                          # what the refused step reads of a loader.DeviceDataset
        def bucket_dims(self, indices, n_max):
            return torch.as_tensor(indices), 9, 40, 5

        def _f32_tables(self):
            return {"x": torch.empty(0, 118)}
        _f64_tables = _f32_tables
    torch.manual_seed(0)
    m64 = DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.25).double().set_program_dtype(torch.float64)
    for tr in (Trainer(DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.25), replay=True, loss="crystal_rmse"),
               Trainer64(m64, replay=True, bucket=(8, 128), loss="crystal_rmse")):
        tr.model.train()
        object.__setattr__(tr.model, "_drop_seed", torch.tensor([7], dtype=torch.int64))
        with pytest.raises(ValueError, match="n_global=4"):
            tr.step_dataset(Dataset(), [0, 1, 2], n_global=4)
        assert int(tr.model._drop_seed) == 7 and tr.step_count == 0 and len(tr._slots) == 0
