"""CPU tests of fine-tuning's host side: the [trainable | frozen] layout of the flat parameters, the prefix methods of the
models, the optimizer checkpoint and the policy functions that prune the backward programs (functional.wgrad_needed /
trunk_cut / first_encoder_cut)."""
import pytest
import torch

from dostransformer_amd import functional as Fn
from dostransformer_amd._fused import FlatParams, GradViews, is_dead_param, is_last_param, is_late_param
from dostransformer_amd._lib import DosxError

CPU = torch.device("cpu")
TRUNK = ("GN_encoder", "stacked_processor", "GN_decoder")


def _phonon(H=16, T=2):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(0)
    return DOSTransformer_phonon(2, T, 118, 4, H, "cpu", 0.0)


def _edos(H=16, T=2):
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    torch.manual_seed(0)
    return DOSTransformer(2, T, 200, 41, 2, H, "cpu", 0.0)


def _recipe(model, which):
    if which == "A":
        return model.freeze(*TRUNK)
    if which == "B":
        # (the prompt table under its own name: the Electron-DOS reference spells it `promt_token`)
        return model.train_only(model._cfg.prompt_key.rsplit(".", 1)[0], "fc_prompt")
    if which == "C":
        for n, p in model.named_parameters():
            if n == "transformer.layers.0.fc1.weight" or n == "embeddings.weight" or n.startswith("stacked_processor.1"):
                p.requires_grad_(False)
        model.update_trainable()
        return model
    if which == "D":
        return model.train_only("GN_encoder.node_encoder")
    raise ValueError(which)


def _todays_layout(model):
    """names, offsets, total, n_late, n_last by the formula the flat buffer had before parameters could be frozen."""
    live = [(n, p) for n, p in model.named_parameters() if not is_dead_param(n)]
    ordered = [x for x in live if is_last_param(x[0])] + [x for x in live if is_late_param(x[0]) and not is_last_param(x[0])] + \
              [x for x in live if not is_late_param(x[0])]
    offs, tot, n_late, n_last = [], 0, 0, 0
    for n, p in ordered:
        offs.append(tot)
        tot += (p.numel() + 63) // 64 * 64
        if is_late_param(n):
            n_late = tot
        if is_last_param(n):
            n_last = tot
    return [n for n, _ in ordered], offs, tot, n_late, n_last


@pytest.mark.parametrize("make", [_phonon, _edos])
def test_all_trainable_layout_is_todays(make):
    model = make()
    names, offs, tot, n_late, n_last = _todays_layout(model)
    fp = FlatParams(model, CPU)
    assert fp.names == names and fp.offsets == offs and fp.total == tot
    assert (fp.n_late, fp.n_last, fp.n_train) == (n_late, n_last, tot)
    assert fp.frozen == frozenset() and fp.G.frozen == frozenset() and not fp.G.cut_trunk and not fp.G.cut_first
    assert fp.trainable_names() == names and sorted(model.trainable_names()) == sorted(names)


@pytest.mark.parametrize("which", ["A", "B", "C", "D"])
def test_frozen_parameters_lie_behind_the_trainable_ones(which):
    model = _recipe(_phonon(), which)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    fp = FlatParams(model, CPU)
    live = [n for n, _ in model.named_parameters() if not is_dead_param(n)]
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad and not is_dead_param(n)}
    assert frozen and fp.frozen == frozen and sorted(fp.names) == sorted(live)
    assert 0 < fp.n_train < fp.total and fp.n_train % 64 == 0
    for n, o in zip(fp.names, fp.offsets):                       # [trainable | frozen], everything aligned
        assert (o >= fp.n_train) == (n in frozen), n
        assert o % 64 == 0 and fp.P[n].data_ptr() == fp.params[n].data_ptr() and fp.G[n].shape == fp.P[n].shape
    train = [n for n in fp.names if n not in frozen]
    # the trainable part keeps [last | mid | early], each in module order, and its two marks
    assert train == [n for n in live if is_last_param(n) and n not in frozen] + \
        [n for n in live if is_late_param(n) and not is_last_param(n) and n not in frozen] + \
        [n for n in live if not is_late_param(n) and n not in frozen]
    for n, o in zip(fp.names, fp.offsets):
        if n not in frozen:
            assert (o < fp.n_late) == is_late_param(n) and (o < fp.n_last) == is_last_param(n)
    assert fp.n_last <= fp.n_late <= fp.n_train
    assert fp.names[len(train):] == [n for n in live if n in frozen]          # the frozen tail in module order
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)              # values are carried over
    assert fp.trainable_names() == train


def test_prefix_methods():
    model = _phonon()
    with pytest.raises(ValueError, match="GN_encodr"):
        model.freeze("GN_encoder", "GN_encodr")
    with pytest.raises(ValueError, match="promt"):
        model.train_only("promt_token")
    with pytest.raises(ValueError, match="self_attn"):             # dead parameters are not live: nothing to match
        model.freeze("transformer.layers.0.self_attn")
    with pytest.raises(ValueError):
        model.freeze()
    assert all(p.requires_grad for p in model.parameters())         # a refused call changed nothing
    assert model.freeze(*TRUNK) is model
    names = model.trainable_names()
    assert names and not any(n.startswith(TRUNK) for n in names) and "fc.weight" in names
    model.train_only("prompt_token", "fc_prompt")
    assert sorted(model.trainable_names()) == ["fc_prompt.bias", "fc_prompt.weight", "prompt_token.weight"]


def test_update_trainable_rebuilds_only_on_a_change_and_check_reports_a_stale_snapshot():
    from dostransformer_amd.train import Trainer
    model = _phonon()
    assert model.update_trainable() is False                       # no flat buffer yet: it is laid out from the flags
    fp = model.flat_params()
    assert model.update_trainable() is False and model.flat_params() is fp
    tr = Trainer(model)
    tr._state(fp)
    tr._m.fill_(3.0)
    tr.check()                                                     # (module on the CPU: nothing launched, nothing stale)
    w = model.fc.weight.detach().clone()
    model.fc.weight.requires_grad_(False)                          # a bare flag change: the snapshot is stale ...
    assert model.flat_params() is fp and model.trainable_stale()
    with pytest.raises(DosxError, match=r"update_trainable\(\)"):  # ... and check() says which call is missing
        tr.check()
    assert model.update_trainable() is True
    fp2 = model.flat_params()
    assert fp2 is not fp and fp2.frozen == {"fc.weight"} and fp2.names[-1] == "fc.weight" and not model.trainable_stale()
    assert torch.equal(model.fc.weight, w) and model.fc.weight.data_ptr() == fp2.P["fc.weight"].data_ptr()
    tr.check()
    m2, _ = tr._state(fp2)                                         # the moments follow by name
    assert m2.numel() == fp2.total
    for n, o in zip(fp2.names, fp2.offsets):
        assert float(m2[o:o + fp2.P[n].numel()].min()) == 3.0, n
    model.fc.weight.requires_grad_(True)
    assert model.update_trainable() is True and model.flat_params().frozen == frozenset()


def test_state_dict_carries_trainable_and_loads_across_frozen_sets():
    from dostransformer_amd.train import Trainer
    full = Trainer(_phonon())
    sd_full = full.state_dict()
    assert "trainable" not in sd_full                              # all-trainable: the file of always
    model = _recipe(_phonon(), "B")
    tr = Trainer(model)
    sd = tr.state_dict()
    fp = model.flat_params()
    assert sd["trainable"] == fp.trainable_names() == ["prompt_token.weight", "fc_prompt.weight", "fc_prompt.bias"]
    assert set(sd["exp_avg"]) == set(fp.names) == set(sd_full["exp_avg"])     # an entry for every live parameter
    sd_full["exp_avg"] = {k: torch.full_like(v, 0.5) for k, v in sd_full["exp_avg"].items()}
    sd_full["step"] = 4
    tr.load_state_dict(sd_full)                                    # all-trainable file -> partly frozen trainer
    assert tr.step_count == 4
    assert all(float(tr._m[o:o + fp.P[n].numel()].min()) == 0.5 for n, o in zip(fp.names, fp.offsets))
    sd["step"] = 9
    full.load_state_dict(sd)                                       # ... and the reverse
    assert full.step_count == 9


def test_dist_is_refused_with_frozen_parameters():
    from dostransformer_amd.train import Trainer

    class _Dist:
        world, rank = 1, 0
    with pytest.raises(DosxError, match="single-GPU mode"):
        Trainer(_recipe(_phonon(), "A"), dist=_Dist())
    model = _phonon()
    tr = Trainer(model, dist=_Dist())                              # frozen after construction: refused when the layout is taken
    model.freeze(*TRUNK)
    with pytest.raises(DosxError, match="single-GPU mode"):
        tr._state(model.flat_params())


@pytest.mark.parametrize("make", [_phonon, _edos])
def test_pruning_policies_for_the_recipes(make):
    want = {"A": (True, False), "B": (True, True), "C": (False, False), "D": (False, False)}
    for which, (cut, cut_first) in want.items():
        model = _recipe(make(), which)
        G = model.flat_params().G
        assert isinstance(G, GradViews)
        assert (Fn.trunk_cut(G.keys(), G.frozen), Fn.first_encoder_cut(G.keys(), G.frozen)) == (cut, cut_first), which
        assert (G.cut_trunk, G.cut_first) == (cut, cut_first)
        # P4: a layer's attention backward needs no key gradient under a frozen trunk AND a frozen layer_norms.0 of its own -
        # recipe B alone (A keeps the LayerNorms training, D the node encoder); never for the self attention
        for pre in ("transformer", "transformer_self", "transformer_source"):
            for t in range(2):
                want_q = which == "B" and pre != "transformer_self"
                assert Fn.attention_query_only(G.keys(), G.frozen, pre, t) == want_q, (which, pre, t)
    names = list(make().flat_params().G)
    trunk = {n for n in names if n.startswith(tuple(p + "." for p in TRUNK))}
    one = next(iter(sorted(trunk)))
    assert not Fn.trunk_cut(names, trunk - {one})                   # one trainable trunk parameter keeps the whole trunk backward
    first = {n for n in names if n.startswith("transformer.") or n == "embeddings.weight"}
    assert Fn.first_encoder_cut(names, trunk | first)
    assert not Fn.first_encoder_cut(names, trunk | first - {"embeddings.weight"})
    assert not Fn.first_encoder_cut(names, first)                   # (the key gradient still feeds a trainable trunk)
    assert not Fn.trunk_cut(names, frozenset()) and not Fn.trunk_cut([], frozenset())
    ln0 = {"transformer_source.layers.1.layer_norms.0.weight", "transformer_source.layers.1.layer_norms.0.bias"}
    assert Fn.attention_query_only(names, trunk | ln0, "transformer_source", 1)                 # both conditions ...
    assert not Fn.attention_query_only(names, trunk | ln0, "transformer_source", 0)             # (another layer's LayerNorm)
    assert not Fn.attention_query_only(names, ln0, "transformer_source", 1)                     # ... a trainable trunk wants its key gradient
    assert not Fn.attention_query_only(names, trunk | {sorted(ln0)[0]}, "transformer_source", 1)   # ... the LayerNorm's weight still trains


def test_weight_gradient_job_policy():
    fz = frozenset({"a.weight", "a.bias", "b.weight", "t.weight"})
    assert not Fn.wgrad_needed(fz, "a.weight", "a.bias")            # weight and bias frozen: no job
    assert not Fn.wgrad_needed(fz, "a.weight", None)                # a column block of a frozen weight
    assert Fn.wgrad_needed(fz, "b.weight", "b.bias")                # trainable bias next to a frozen weight: the job runs whole
    assert not Fn.wgrad_needed(fz, "b.weight", None)
    assert Fn.wgrad_needed(fz, "c.weight", "a.bias") and Fn.wgrad_needed(frozenset(), "a.weight", "a.bias")
    assert not Fn.table_needed(fz, "t.weight") and Fn.table_needed(fz, "u.weight")
    assert Fn.frozen_of({}) == frozenset() and Fn.frozen_of(GradViews({}, fz)) == fz
