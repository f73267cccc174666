"""CPU-only checks of the GNN-only baselines' fused path: the g10 fixtures (the reference's own Graphnetwork_phonon, Graphnetwork
and mlp through its drivers' train step) against the pinned oracle in float64; the mlp module's parameters; the pair-head
entries' boundary (declared, replayable, prototyped, every bad descriptor refused before any launch); and the refusals of
train.Trainer / predict.Predictor for these modules."""
import ctypes as C
import os

import pytest
import torch

from tests.util import batch_from, dosx_lib as _lib, in_all_three_builds, load, maxabs, sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTIONS = ("ph", "gn", "mlp")


# ---- the fixtures ----------------------------------------------------------------------------------------------------
def _oracle(name, z):
    """Outputs, one-output loss and autograd gradients of the oracle in float64 on the stored parameters and batch."""
    from oracle import dos_oracle as O
    p = {k: v.double().requires_grad_(True) for k, v in sub(z, "p0/").items()}
    g = batch_from(z).to("cpu", dtype=torch.float64)
    if name == "ph":
        dos, x = O.graphnetwork_phonon_forward(p, g, 3), None
        loss = torch.sqrt(((dos - g.phdos.reshape(dos.shape)) ** 2).mean())
    else:
        dos, x = O.graphnetwork_forward(p, g, 3 if name == "gn" else 0)        # mlp: Graphnetwork without processors
        y = torch.clamp(g.y_ft, min=0.0).reshape(dos.shape)
        loss = torch.sqrt(((y - dos) ** 2).mean(1)).mean()
    loss.backward()
    return dos.detach(), x, loss.detach(), p


@pytest.mark.parametrize("name", SECTIONS)
def test_g10_sections_agree_with_the_oracle(name):
    """float64 section: outputs, loss and gradients to 1e-10; the fp32 sections at the fixture's own fp32 level, the bounds of
    tests/test_oracle_golden.py for G8 (outputs 2e-5, gradients 5e-4)."""
    z = load(f"g10_baselines_{name}.npz")
    tol_out, tol_grad = (1e-10, 1e-10) if name == "ph" else (2e-5, 5e-4)
    assert (z["dos"].dtype, z["p0/embeddings.weight"].dtype) == (("float64",) * 2 if name == "ph" else ("float32",) * 2)
    dos, x, loss, p = _oracle(name, z)
    assert maxabs(dos, z["dos"]) < tol_out and abs(float(loss) - float(z["loss"])) < tol_out
    if name == "gn":
        assert maxabs(x, z["x_nodes"]) < tol_out
    dead = set(str(s) for s in z["dead_params"])
    for k, v in p.items():
        if k in dead:
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, k
        else:
            assert maxabs(v.grad, z["g/" + k]) < tol_grad, k
    # sizes the issue fixes: three crystals of 1 / 4 / 9 atoms (eDOS: + one phantom node each), hidden 16
    counts = torch.bincount(torch.from_numpy(z["b/batch"])).tolist()
    assert counts == ([1, 4, 9] if name == "ph" else [2, 5, 10]) and z["p0/embeddings.weight"].shape[1] == 16
    assert float(z["min_abs_pre"]) >= 1e-5                                    # no LeakyReLU gate can flip at fp32 rounding
    # p1 / p3 moved every live parameter and no dead one
    for k, v in sub(z, "p0/").items():
        assert (maxabs(v, z["p3/" + k]) == 0.0) == (k in dead), k


def test_mlp_module_has_the_reference_parameters_and_dead_set():
    from dostransformer_amd.embedder_eDOS.mlp import mlp
    z = load("g10_baselines_mlp.npz")
    model = mlp(3, 200, 41, 2, 16, 201, "cpu")
    ref = sub(z, "p0/")
    sd = model.state_dict()
    assert list(sd) == list(ref) and all(tuple(sd[k].shape) == tuple(ref[k].shape) for k in sd)
    assert not any(k.startswith("stacked_processor") for k in sd)
    g = batch_from(z)
    assert set(model._extra_dead(g)) == set(str(s) for s in z["dead_params"])
    assert all(k.startswith(("GN_encoder.node_encoder_prompt.", "GN_encoder.edge_encoder.")) for k in model._extra_dead(g))
    model.load_state_dict(ref)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(g)


# ---- the library boundary (style of tests/test_knn_abi.py) -----------------------------------------------------------------
POINTERS = ("e1", "c", "w2", "b2", "dos", "ddos", "de1", "dc", "partials")


def test_pair_head_declared_exported_replayable_and_prototyped():
    _l = _lib()
    lib = _l.load()
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    thunks = open(os.path.join(ROOT, "dostransformer_amd", "csrc", "replay_thunks.inc")).read()
    for name in ("dosx_pair_head_fwd", "dosx_pair_head_bwd"):
        assert f"int {name}(const DosxPairHead* a, dosx_stream_t stream);" in header
        assert f'{{"{name}", thunk_{name}, 2, 0}}' in thunks
        ni, nf = C.c_int(0), C.c_int(0)
        assert lib.dosx_replay_op(name.encode(), C.byref(ni), C.byref(nf)) >= 0 and (ni.value, nf.value) == (2, 0)
        assert getattr(lib, name).argtypes == [C.POINTER(_l.PairHead), C.c_void_p]
    assert in_all_three_builds("pair_head.hip")              # libdosx.so and the two diagnostic builds
    assert [k for k, _ in _l.PairHead._fields_] == ["S", "B", "H", "slope"] + list(POINTERS)
    assert C.sizeof(_l.PairHead) == 4 * 4 + 9 * 8
    assert lib.dosx_pair_head_partial_rows(201, 64) == 201 and lib.dosx_pair_head_partial_rows(0, 64) == 0


def _descriptor(_l):
    """A descriptor both entries accept; the addresses are never dereferenced (each call below is refused before a launch)."""
    d = _l.PairHead()
    d.S, d.B, d.H, d.slope = 201, 64, 256, 0.01
    for i, k in enumerate(POINTERS):
        setattr(d, k, 0x10000 * (i + 1))
    return d


def test_pair_head_argument_validation_needs_no_gpu():
    _l = _lib()
    lib = _l.load()
    err = lambda: lib.dosx_last_error().decode()
    for name, outs in (("dosx_pair_head_fwd", ("b2", "dos")), ("dosx_pair_head_bwd", ("ddos", "de1", "dc", "partials"))):
        fn = getattr(lib, name)

        def refused(d, word=""):
            assert fn(C.byref(d), None) == -22
            assert name in err() and word in err(), err()

        assert fn(None, None) == -22 and name in err() and "null descriptor" in err()
        for field, bad, word in (("S", 0, "S=0"), ("S", -3, "S=-3"), ("B", 0, "B=0"), ("B", -1, "B=-1"), ("H", 0, "H=0"),
                                 ("H", 12, "hidden 12"), ("H", 520, "hidden 520"), ("H", 1024, "hidden 1024")):
            d = _descriptor(_l)
            setattr(d, field, bad)
            refused(d, word)
        for k in ("e1", "c", "w2") + outs:
            d = _descriptor(_l)
            setattr(d, k, None)
            refused(d, "null operand")
        d = _descriptor(_l)
        d.e1 = 0x10004
        refused(d, "16-byte aligned")
        d = _descriptor(_l)
        d.S, d.B, d.H = 1 << 11, 1 << 11, 512                       # S*B*H = 2^31
        refused(d, "S*B*H")


# ---- the drivers' refusals -----------------------------------------------------------------------------------------------
def _modules():
    from dostransformer_amd.embedder_eDOS.graphnetwork import Graphnetwork
    from dostransformer_amd.embedder_eDOS.mlp import mlp
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    return [Graphnetwork_phonon(1, 118, 4, 16, 51, "cpu"), Graphnetwork(1, 200, 41, 2, 16, 201, "cpu"), mlp(1, 200, 41, 2, 16, 201, "cpu")]


def test_trainer_and_predictor_accept_the_baselines_and_refuse_what_they_cannot_do():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.predict import Predictor
    from dostransformer_amd.train import Trainer
    for model in _modules():
        name = type(model).__name__
        tr = Trainer(model)
        assert tr.kind == ("phonon" if name == "Graphnetwork_phonon" else "edos") and not tr.per_crystal_keys
        assert Trainer(model, replay=True).replay and Trainer(model, graph=True).graph
        with pytest.raises(ValueError, match="beta"):
            Trainer(model, beta=0.5)
        with pytest.raises(DosxError, match="per_crystal_keys"):
            Trainer(model, per_crystal_keys=True)
        with pytest.raises(DosxError, match="data parallelism"):
            Trainer(model, dist=object())
        pred = Predictor(model)
        assert pred.batch_independent and not pred.per_crystal_keys
        with pytest.raises(DosxError, match="per_crystal_keys"):
            Predictor(model, per_crystal_keys=True)
    with pytest.raises(TypeError):
        Trainer(torch.nn.Linear(2, 2))
    with pytest.raises(TypeError):
        Predictor(torch.nn.Linear(2, 2))
    # a float64 Graphnetwork_phonon runs the float64 program: not these drivers'
    m64 = _modules()[0].double()
    with pytest.raises(DosxError, match="float64"):
        Trainer(m64)
    with pytest.raises(DosxError, match="float64"):
        Predictor(m64)


def test_trainer_fixes_the_dead_set_with_the_first_batch_and_checks_n_global():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    from dostransformer_amd.trainer_base import _Width
    for model in _modules():
        expected = 118 if model._cfg.kind == "phonon" else 200
        tr = Trainer(model)
        cpu = torch.device("cpu")
        fp = tr._flat_for(cpu, _Width(expected))
        assert not any("node_encoder_prompt" in n for n in fp.names) and any("node_encoder." in n for n in fp.names)
        assert tr._flat_for(cpu, None, expected) is fp
        with pytest.raises(DosxError, match="first batch"):
            tr._flat_for(cpu, _Width(expected + 8))
        with pytest.raises(DosxError, match="first batch"):
            tr._flat_for(cpu, None, expected + 8)
        st = {"B": 4, "S": model._cfg.S, "dos": None}
        with pytest.raises(ValueError, match="n_global=8"):
            tr._part_b(fp, None, st, 8)


def test_a_transformer_predictor_without_the_flag_is_still_refused_by_the_evaluator():
    from dostransformer_amd import evaluate
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.predict import Predictor
    pred = Predictor(DOSTransformer_phonon(1, 1, 118, 4, 16, "cpu", 0.0))
    assert not pred.batch_independent
    with pytest.raises(ValueError, match="per-crystal keys"):
        evaluate.test_per_crystal(pred, None)
