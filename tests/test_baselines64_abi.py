"""CPU-only checks of the float64 baseline path: the float64 pair-head entry points (csrc/pair_head_f64.hip) are declared,
exported, replayable and refuse bad arguments before any launch; which modules train64.GraphnetworkTrainer64 and
predict.Predictor64 take; the trainer's checkpoint vocabulary and its dead-parameter rule."""
import ctypes as C
import os

import pytest
import torch

from tests.util import dosx_lib as _lib, in_all_three_builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dosx_pair_head_fwd_f64", "dosx_pair_head_bwd_f64")
POINTERS = ("e1", "c", "w2", "b2", "dos", "ddos", "de1", "dc", "partials")


def test_pair_head64_declared_exported_replayable_and_prototyped():
    _l = _lib()
    lib = _l.load()
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    abi = open(os.path.join(ROOT, "dostransformer_amd", "_abi.py")).read()
    thunks = open(os.path.join(ROOT, "dostransformer_amd", "csrc", "replay_thunks.inc")).read()
    assert "typedef struct DosxPairHead64 {" in header and "class PairHead64(C.Structure):" in abi
    for name in NAMES:
        assert f"int {name}(const DosxPairHead64* a, dosx_stream_t stream);" in header
        assert f'"{name}": [C.POINTER(PairHead64), C.c_void_p]' in abi
        assert f'{{"{name}", thunk_{name}, 2, 0}}' in thunks
        ni, nf = C.c_int(0), C.c_int(0)
        assert lib.dosx_replay_op(name.encode(), C.byref(ni), C.byref(nf)) >= 0 and (ni.value, nf.value) == (2, 0)
        assert getattr(lib, name).argtypes == [C.POINTER(_l.PairHead64), C.c_void_p]
    assert in_all_three_builds("pair_head_f64.hip")           # libdosx.so and the two diagnostic builds
    assert [k for k, _ in _l.PairHead64._fields_] == ["S", "B", "H", "slope"] + list(POINTERS)
    assert dict(_l.PairHead64._fields_)["slope"] is C.c_double
    assert C.sizeof(_l.PairHead64) == 16 + 8 + 9 * 8               # three ints padded to the double, the slope, nine pointers


def _descriptor(_l):
    """A descriptor both entries accept; the addresses are never dereferenced (each call below is refused before a launch)."""
    d = _l.PairHead64()
    d.S, d.B, d.H, d.slope = 51, 64, 128, 0.01
    for i, k in enumerate(POINTERS):
        setattr(d, k, 0x10000 * (i + 1))
    return d


def test_pair_head64_argument_validation_needs_no_gpu():
    _l = _lib()
    lib = _l.load()
    err = lambda: lib.dosx_last_error().decode()
    for name, outs in ((NAMES[0], ("b2", "dos")), (NAMES[1], ("ddos", "de1", "dc", "partials"))):
        fn = getattr(lib, name)

        def refused(d, word=""):
            assert fn(C.byref(d), None) == -22
            assert name in err() and word in err(), err()

        assert fn(None, None) == -22 and name in err() and "null descriptor" in err()
        for field, bad, word in (("S", 0, "S=0"), ("S", -3, "S=-3"), ("B", 0, "B=0"), ("H", 0, "H=0"), ("H", 12, "hidden 12"),
                                 ("H", 520, "hidden 520"), ("H", 1024, "hidden 1024")):
            d = _descriptor(_l)
            setattr(d, field, bad)
            refused(d, word)
        for k in ("e1", "c", "w2") + outs:
            d = _descriptor(_l)
            setattr(d, k, None)
            refused(d, "null operand")
        d = _descriptor(_l)
        d.e1 = 0x10008                                              # double-aligned, not 16-byte aligned
        refused(d, "16-byte aligned")
        d = _descriptor(_l)
        d.S, d.B, d.H = 1 << 11, 1 << 11, 512                       # S*B*H = 2^31
        refused(d, "S*B*H")
    d = _descriptor(_l)
    d.dc = 0x70008
    assert lib.dosx_pair_head_bwd_f64(C.byref(d), None) == -22 and "de1 / dc" in err()


# ---- the drivers ---------------------------------------------------------------------------------------------------------
def _gn64(H=16):
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    torch.manual_seed(0)
    return Graphnetwork_phonon(2, 118, 4, H, 51, "cpu").double()


def _others():
    from dostransformer_amd.embedder_eDOS.graphnetwork import Graphnetwork
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    ph = lambda: DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.0).double()
    return [Graphnetwork_phonon(2, 118, 4, 16, 51, "cpu"),                      # fp32 parameters: train.Trainer's
            ph(), ph().set_program_dtype(torch.float64),                         # the transformer: Trainer64's
            Graphnetwork(1, 200, 41, 2, 16, 201, "cpu").double(),                # eDOS: its program is fp32 whatever the dtype
            torch.nn.Linear(2, 2)]


def test_graphnetwork_trainer64_takes_only_a_float64_graphnetwork_phonon():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train64 import GraphnetworkTrainer64, Trainer64
    assert issubclass(GraphnetworkTrainer64, Trainer64)
    m64 = _gn64()
    tr = GraphnetworkTrainer64(m64, lr=1e-3, replay=True, max_slots=3, bucket=(8, 128), promote=0.1)
    assert (tr.lr, tr.replay, tr.max_slots, tr.bucket, tr.promote, tr.step_count) == (1e-3, True, 3, (8, 128), 0.1, 0)
    assert (tr.slot_hits, tr.slot_misses, tr.slot_promoted) == (0, 0, 0) and callable(tr.step_dataset)
    for bad in _others():
        with pytest.raises(DosxError, match="GraphnetworkTrainer64"):
            GraphnetworkTrainer64(bad)
    with pytest.raises(ValueError, match="beta"):
        GraphnetworkTrainer64(m64, beta=0.5)
    with pytest.raises(TypeError):
        GraphnetworkTrainer64(m64, dist=None)
    with pytest.raises(TypeError):
        GraphnetworkTrainer64(m64, graph=True)
    with pytest.raises(ValueError, match="bucket"):
        GraphnetworkTrainer64(m64, bucket=(8,))
    # the other drivers point at this one
    from dostransformer_amd.predict import Predictor
    from dostransformer_amd.train import Trainer
    for drv in (Trainer, Predictor, Trainer64):
        with pytest.raises(DosxError, match="float64") as e:
            drv(m64)
        assert "GraphnetworkTrainer64" in str(e.value) and "Predictor64" in str(e.value) and "loss.backward" not in str(e.value)
    wide = _gn64(520)
    with pytest.raises(DosxError, match="hidden <= 512"):
        GraphnetworkTrainer64(wide)
    # parameters cast back under a live driver: refused at the step, before anything runs
    m64.float()
    with pytest.raises(DosxError, match="GraphnetworkTrainer64"):
        tr.forward_backward(object())


def test_predictor64_accepts_the_float64_baseline():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.predict import Predictor64
    m64 = _gn64()
    p = Predictor64(m64)
    assert p.batch_independent and p.kind == "phonon" and p.bucket == (8, 128) and (p.slot_hits, p.slot_misses) == (0, 0)
    assert p.eval() is p and not m64.training and p._key_tail() == ()
    for bad in _others():
        if getattr(bad, "program_dtype", None) == torch.float64:
            assert not Predictor64(bad).batch_independent                 # the switched transformer stays its own case
            continue
        with pytest.raises(DosxError, match="Predictor64"):
            Predictor64(bad)


def test_graphnetwork_trainer64_state_dict_is_trainer64s():
    from dostransformer_amd.train64 import GraphnetworkTrainer64
    m64 = _gn64()
    tr = GraphnetworkTrainer64(m64, lr=3e-4)
    sd = tr.state_dict()
    assert set(sd) == {"step", "exp_avg", "exp_avg_sq", "drop_seed_base", "hyper"} and sd["step"] == 0
    assert set(sd["hyper"]) == {"lr", "betas", "eps", "weight_decay", "beta"} and sd["drop_seed_base"] is None
    fp = m64.flat_params()
    assert set(sd["exp_avg"]) == set(fp.names) == set(sd["exp_avg_sq"])
    assert not any("node_encoder_prompt" in k or "node_mlp_1" in k for k in sd["exp_avg"])
    assert all(v.dtype == torch.float64 and v.shape == fp.P[k].shape for k, v in sd["exp_avg"].items())
    sd["step"] = 7
    sd["exp_avg"] = {k: torch.full_like(v, 0.25) for k, v in sd["exp_avg"].items()}
    sd["hyper"]["lr"] = 5e-4
    tr2 = GraphnetworkTrainer64(_gn64())
    tr2.load_state_dict(sd)
    assert tr2.step_count == 7 and tr2.lr == 5e-4 and tr2._m.dtype == torch.float64
    assert all(bool((v == 0.25).all()) for v in tr2.state_dict()["exp_avg"].values())


def test_the_first_width_fixes_the_dead_node_encoder():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.trainer_base import _Width
    from dostransformer_amd.train64 import GraphnetworkTrainer64
    H, cpu = 16, torch.device("cpu")
    for first, other, dead, live in ((118, 118 + H // 2, "node_encoder_prompt.", "node_encoder."),
                                     (118 + H // 2, 118, "node_encoder.", "node_encoder_prompt.")):
        tr = GraphnetworkTrainer64(_gn64(H))
        fp = tr._flat_for(cpu, _Width(first))
        assert fp.dtype == torch.float64
        assert not any(dead in n for n in fp.names) and any(live in n for n in fp.names)
        assert tr._flat_for(cpu, None, first) is fp
        for args in ((_Width(other),), (None, other)):
            with pytest.raises(DosxError, match="first batch"):
                tr._flat_for(cpu, *args)


def test_functional64_factored_flag_must_match_the_context():
    from dostransformer_amd import functional64 as F64
    with pytest.raises(ValueError, match="factored_head"):
        F64.graphnetwork_phonon_bwd({}, {}, None, None, (None,) * 5, None, factored_head=True)
    ctx = F64._FactoredCtx64(None, None, None, None, None, None, False)
    with pytest.raises(ValueError, match="factored_head"):
        F64.graphnetwork_phonon_bwd({}, {}, None, None, ctx, None)
