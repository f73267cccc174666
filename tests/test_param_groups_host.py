"""CPU-only checks of the host side of the optimizer parameter groups (dostransformer_amd/param_groups.py and the
``param_groups=`` argument of the trainers): resolving the user's list, the chunk map of a flat layout, the two helpers that
produce lists, and the checkpoint.  Modules on the CPU; nothing is launched."""
import io

import pytest
import torch

LR, WD = 1e-3, 1e-2


def _phonon(L=2, T=1, H=16):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(0)
    return DOSTransformer_phonon(L, T, 118, 4, H, "cpu", 0.0)


def _graphnetwork(L=2, H=16):
    from dostransformer_amd.embedder_eDOS.graphnetwork import Graphnetwork
    torch.manual_seed(0)
    return Graphnetwork(L, 200, 41, 2, H, 201, "cpu")


def _live(model):
    return [n for n, _ in model._live_named()]


# ---- resolve -----------------------------------------------------------------------------------------------------------
def test_resolve_inherits_missing_values_and_collects_the_rest_in_group_zero():
    from dostransformer_amd import param_groups as pg
    model = _phonon()
    got = pg.resolve(model, [{"params": "GN_encoder.", "lr": 1e-5},
                             {"params": ["transformer.", "fc."], "weight_decay": 0.0},
                             {"params": "out_layer.", "lr": LR, "weight_decay": WD}], LR, WD)
    assert [sorted(g) for g in got] == [["lr", "names", "weight_decay"]] * 4
    assert [(g["lr"], g["weight_decay"]) for g in got] == [(LR, WD), (1e-5, WD), (LR, 0.0), (LR, WD)]     # equal values: not merged
    live = _live(model)
    assert got[1]["names"] == [n for n in live if n.startswith("GN_encoder.")]
    assert got[2]["names"] == [n for n in live if n.startswith(("transformer.", "fc."))]
    assert "transformer_self.layer_norm.weight" not in got[2]["names"] and "fc_prompt.weight" not in got[2]["names"]
    assert got[3]["names"] == ["out_layer.weight", "out_layer.bias"]
    named = set(got[1]["names"] + got[2]["names"] + got[3]["names"])
    assert got[0]["names"] == [n for n in live if n not in named] and got[0]["names"]
    assert sorted(n for g in got for n in g["names"]) == sorted(live)                                    # a partition of the live names
    assert not any("self_attn" in n or "node_mlp_1" in n or n == "alpha" for n in live)                  # dead parameters: no group
    assert pg.assignment(got)["out_layer.bias"] == 3 and pg.assignment(got)["embeddings.weight"] == 0
    # frozen parameters are live: a group of frozen parameters resolves
    model.freeze("out_layer.")
    assert pg.resolve(model, [{"params": "out_layer."}], LR, WD)[1]["names"] == ["out_layer.weight", "out_layer.bias"]
    # everything matched: the implicit group stays, empty
    every = pg.resolve(model, [{"params": sorted({n.split(".")[0] for n in live})}], LR, WD)
    assert every[0]["names"] == [] and every[1]["names"] == live


def test_resolve_names_what_is_wrong():
    from dostransformer_amd import param_groups as pg
    model = _phonon()
    with pytest.raises(ValueError, match=r"prefix 'no_such\.' of group 1 matches no live parameter"):
        pg.resolve(model, [{"params": "fc."}, {"params": ["GN_decoder.", "no_such."]}], LR, WD)
    with pytest.raises(ValueError, match=r"matches no live parameter"):                                  # a dead parameter is not live
        pg.resolve(model, [{"params": "transformer.layers.0.self_attn."}], LR, WD)
    with pytest.raises(ValueError, match=r"parameter 'GN_encoder\.node_encoder\.0\.weight' is matched by group 0 and by group 2"):
        pg.resolve(model, [{"params": "GN_encoder."}, {"params": "fc."}, {"params": "GN_encoder.node_encoder."}], LR, WD)
    names = _live(model)
    assert len(names) >= 16
    assert len(pg.resolve(model, [{"params": n} for n in names[:15]], LR, WD)) == 16                    # 15 + the implicit one
    with pytest.raises(ValueError, match=r"16 groups and the implicit one are more than the 16"):
        pg.resolve(model, [{"params": n} for n in names[:16]], LR, WD)
    with pytest.raises(ValueError, match="betas"):
        pg.resolve(model, [{"params": "fc.", "betas": (0.9, 0.99)}], LR, WD)
    for bad in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="lr of group 0"):
            pg.resolve(model, [{"params": "fc.", "lr": bad}], LR, WD)
        with pytest.raises(ValueError, match="weight_decay of group 0"):
            pg.resolve(model, [{"params": "fc.", "weight_decay": bad}], LR, WD)


# ---- chunk_map ---------------------------------------------------------------------------------------------------------
def _check_map(fp, assign, cmap):
    assert cmap.dtype == torch.uint8 and cmap.device.type == "cpu" and cmap.numel() == fp.n_train // 64 and fp.n_train % 64 == 0
    covered = torch.zeros(cmap.numel(), dtype=torch.bool)
    for n, o in zip(fp.names, fp.offsets):
        k = fp.P[n].numel()
        a, b = o // 64, (o + k + 63) // 64                  # every chunk of the parameter, its padded last one included
        if n in fp.frozen:
            assert o >= fp.n_train                           # behind n_train: no entry
            continue
        assert o % 64 == 0 and b <= cmap.numel()
        assert bool((cmap[a:b] == assign.get(n, 0)).all()), n
        covered[a:b] = True
    assert bool(covered.all())                               # no chunk belongs to nobody


@pytest.mark.parametrize("kind", ["phonon", "graphnetwork"])
def test_chunk_map_follows_the_flat_layout(kind):
    from dostransformer_amd import param_groups as pg
    model = _phonon() if kind == "phonon" else _graphnetwork()
    groups = pg.resolve(model, [{"params": "GN_encoder.", "lr": 1e-5}, {"params": pg.no_decay(model)[-3:], "weight_decay": 0.0},
                                {"params": "stacked_processor.1."}], LR, WD)
    assign = pg.assignment(groups)
    fp = model.flat_params()
    assert fp.n_train == fp.total and not fp.frozen
    cmap = pg.chunk_map(fp, assign)
    _check_map(fp, assign, cmap)
    assert sorted(set(cmap.tolist())) == [0, 1, 2, 3]
    assert torch.equal(cmap, pg.chunk_map(fp, assign))                                                   # a pure function
    odd = [n for n in fp.names if fp.P[n].numel() % 64 not in (0,) and fp.P[n].numel() > 64]
    assert odd, "no parameter with a padded last chunk"
    # frozen parameters get no entry; the map is that of the new layout
    model.freeze("stacked_processor.1.")
    fp2 = model.flat_params()
    assert fp2 is not fp and fp2.frozen and fp2.n_train < fp2.total
    cmap2 = pg.chunk_map(fp2, assign)
    _check_map(fp2, assign, cmap2)
    assert cmap2.numel() < cmap.numel() and 3 not in cmap2.tolist()
    with pytest.raises(ValueError, match="outside"):
        pg.chunk_map(fp2, {fp2.names[0]: 16})


def test_trainer_rebuilds_the_chunk_map_with_the_layout():
    """TrainerBase._state is where the moments are re-homed - and the chunk map with them: after freeze() / update_trainable() the
    trainer's map is the new layout's.  Without groups no map is built."""
    from dostransformer_amd import param_groups as pg
    from dostransformer_amd.train import Trainer
    model = _phonon()
    tr = Trainer(model, lr=LR, weight_decay=WD, param_groups=[{"params": "GN_encoder.", "lr": 1e-5}, {"params": "fc", "weight_decay": 0.0}])
    assert tr._chunk_group is None and tr.lr == LR and tr.wd == WD
    fp = model.flat_params()
    tr._state(fp)
    assign = pg.assignment(tr.param_groups)
    first = tr._chunk_group
    assert torch.equal(first, pg.chunk_map(fp, assign)) and set(first.tolist()) == {0, 1, 2}
    tr._state(fp)
    assert tr._chunk_group is first                                                                      # same layout: not rebuilt
    model.freeze("GN_encoder.")                                                                          # (calls update_trainable())
    fp2 = model.flat_params()
    tr._state(fp2)
    assert tr._chunk_group is not first and torch.equal(tr._chunk_group, pg.chunk_map(fp2, assign))
    assert 1 not in tr._chunk_group.tolist() and tr._chunk_group.numel() == fp2.n_train // 64            # an all-frozen group: legal
    for p in model.parameters():
        p.requires_grad_(True)
    assert model.update_trainable()
    tr._state(model.flat_params())
    assert torch.equal(tr._chunk_group, first)
    plain = Trainer(_phonon(), lr=LR)
    plain._state(plain.model.flat_params())
    assert plain.param_groups is None and plain._chunk_group is None and plain._groups_host is None


# ---- helpers -----------------------------------------------------------------------------------------------------------
def test_no_decay_lists_biases_norms_slopes_embeddings_and_prompt_tokens():
    from dostransformer_amd import param_groups as pg
    model = _phonon()
    nd = pg.no_decay(model)
    live = _live(model)
    assert nd == [n for n in live if n in set(nd)] and len(set(nd)) == len(nd)                           # live names, module order
    for n in ("embeddings.weight", "prompt_token.weight", "GN_encoder.node_encoder.1.weight", "GN_encoder.node_encoder.0.bias",
              "stacked_processor.0.edge_model.edge_mlp.1.weight", "stacked_processor.0.edge_model.edge_mlp.1.bias",
              "stacked_processor.1.node_model.node_mlp_2.2.weight", "transformer.layers.0.layer_norms.1.weight",
              "transformer.layer_norm.weight", "transformer_source.layer_norm.bias", "out_layer.bias", "fc_prompt.bias"):
        assert n in nd, n
    rest = [n for n in live if n not in nd]
    assert rest and all(n.endswith(".weight") and model.get_parameter(n).dim() == 2 for n in rest)       # what decays: the matrices
    for n in ("GN_encoder.node_encoder.0.weight", "transformer.layers.0.fc1.weight", "fc.weight", "out_layer.weight"):
        assert n in rest, n
    # the names are a legal group
    groups = pg.resolve(model, [{"params": nd, "weight_decay": 0.0}], LR, WD)
    assert groups[1]["names"] == nd and groups[0]["names"] == rest
    gn = _graphnetwork()
    assert all(n.endswith(".bias") or gn.get_parameter(n).dim() == 1 or "embed" in n or "prom" in n for n in pg.no_decay(gn))


def test_layerwise_ladder():
    from dostransformer_amd import param_groups as pg
    L = 3
    model = _phonon(L=L)
    lr, d = 1e-3, 0.5
    groups = pg.layerwise(model, lr, d)
    assert len(groups) == L + 3 and all(sorted(g) == ["lr", "params"] for g in groups)
    assert [g["lr"] for g in groups] == [lr * d ** k for k in range(L + 3)]
    assert [g["params"] for g in groups[1:]] == [["GN_decoder."], ["stacked_processor.2."], ["stacked_processor.1."],
                                                 ["stacked_processor.0."], ["GN_encoder."]]
    assert groups[-1]["lr"] == lr * d ** (L + 2) and groups[1]["lr"] == lr * d and groups[2]["lr"] == lr * d ** 2
    top = groups[0]["params"]
    assert set(top) == {"embeddings.", "prompt_token.", "transformer.", "transformer_self.", "transformer_source.", "out_layer.", "fc.",
                        "fc_prompt."}
    res = pg.resolve(model, groups, 7.0, WD)
    assert res[0]["names"] == [] and all(g["weight_decay"] == WD for g in res)                           # every live name has a rung
    by = pg.assignment(res)
    assert by["fc.weight"] == 1 and by["GN_decoder.mlp.0.weight"] == 2 and by["stacked_processor.2.edge_model.edge_mlp.0.weight"] == 3
    assert by["stacked_processor.0.edge_model.edge_mlp.0.weight"] == 5 and by["GN_encoder.edge_encoder.0.weight"] == 6
    # together with no_decay: every rung split in two, no parameter twice, the rates kept
    both = pg.resolve(model, pg.with_no_decay(model, groups), 7.0, WD)
    assert len(both) == 1 + 2 * (L + 3) and both[0]["names"] == []
    nd = set(pg.no_decay(model))
    for g in both[1:]:
        assert g["names"] and (g["weight_decay"] == 0.0) == (g["names"][0] in nd)
        assert all((n in nd) == (g["weight_decay"] == 0.0) for n in g["names"])
    rate = {n: g["lr"] for g in both for n in g["names"]}
    assert all(rate[n] == res[by[n]]["lr"] for n in by)
    gn = _graphnetwork(L=2)
    assert [g["lr"] for g in pg.layerwise(gn, 1.0, 0.5)][-1] == 0.5 ** 4


# ---- trainers: construction and checkpoint ---------------------------------------------------------------------------------
def test_trainers_take_param_groups_and_refuse_them_with_dist():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    from tests.gpu_util import _FakeDist
    model = _phonon()
    groups = [{"params": "GN_encoder.", "lr": 1e-5}]
    with pytest.raises(DosxError, match=r"Trainer\(param_groups=\.\.\.\) is a single-GPU mode: not with dist"):
        Trainer(model, dist=_FakeDist(None), param_groups=groups)
    with pytest.raises(ValueError, match="matches no live parameter"):
        Trainer(model, param_groups=[{"params": "nothing."}])
    tr = Trainer(model, lr=LR, weight_decay=WD, param_groups=groups)
    assert [(g["lr"], g["weight_decay"]) for g in tr.param_groups] == [(LR, WD), (1e-5, WD)]
    tr.param_groups[1]["lr"] = 5e-6                                                                      # a schedule writes here
    assert tr._groups[1]["lr"] == 5e-6 and tr.lr == LR


def _save_load(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False), buf.getvalue()


def test_state_dict_carries_the_groups_only_when_there_are_groups():
    from dostransformer_amd.train import Trainer
    groups = [{"params": "GN_encoder.", "lr": 1e-5}, {"params": "fc.", "weight_decay": 0.0}]
    plain = Trainer(_phonon(), lr=LR, weight_decay=WD)
    sd_plain = plain.state_dict()
    assert "param_groups" not in sd_plain
    assert sorted(sd_plain) == ["drop_seed_base", "exp_avg", "exp_avg_sq", "hyper", "step"]              # the file it always wrote
    tr = Trainer(_phonon(), lr=LR, weight_decay=WD, param_groups=groups)
    tr.param_groups[2]["lr"] = 2e-4
    with torch.no_grad():
        tr._state(tr.model.flat_params())
        tr._m.fill_(0.25)
        tr._v.fill_(0.5)
    tr.step_count = 5
    sd, _ = _save_load(tr.state_dict())
    assert [(g["lr"], g["weight_decay"]) for g in sd["param_groups"]] == [(LR, WD), (1e-5, WD), (2e-4, 0.0)]
    assert [g["names"] for g in sd["param_groups"]] == [g["names"] for g in tr.param_groups]
    assert sorted(set(sd) - set(sd_plain)) == ["param_groups"]
    # round trip: values by group index, moments by name
    tr2 = Trainer(_phonon(), lr=LR, weight_decay=WD, param_groups=groups)
    tr2.load_state_dict(sd)
    assert [(g["lr"], g["weight_decay"]) for g in tr2.param_groups] == [(LR, WD), (1e-5, WD), (2e-4, 0.0)]
    assert tr2.step_count == 5 and bool((tr2._m[:8] == 0.25).all()) and bool((tr2._v[:8] == 0.5).all())
    # another number of groups: the trainer keeps its own values
    tr3 = Trainer(_phonon(), lr=LR, weight_decay=WD, param_groups=groups[:1])
    tr3.load_state_dict(sd)
    assert [(g["lr"], g["weight_decay"]) for g in tr3.param_groups] == [(LR, WD), (1e-5, WD)] and tr3.step_count == 5
    # a grouped file into an ungrouped trainer, and back
    plain.load_state_dict(sd)
    assert plain.param_groups is None and plain.step_count == 5 and bool((plain._m[:8] == 0.25).all())
    back = plain.state_dict()
    assert "param_groups" not in back
    tr4 = Trainer(_phonon(), lr=LR, weight_decay=WD, param_groups=groups)
    tr4.load_state_dict(back)
    assert [(g["lr"], g["weight_decay"]) for g in tr4.param_groups] == [(LR, WD), (1e-5, WD), (LR, 0.0)]
    assert tr4.step_count == 5 and bool((tr4._v[:8] == 0.5).all())
