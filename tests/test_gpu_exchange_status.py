"""The stall report of the column-split exchanges (csrc/mlp2.hip: cs_report_stall behind cs_publish_done_and_wait) on the GPU:
the sticky status through dosx_exchange_status, the report path through the test-only dosx_exchange_selftest, ops.check_exchanges
and the places that call it (the drivers' check(), checkpoint.save, evaluate.test_per_crystal), and that real training steps on
the column-split path leave the status clear.  No test here - or anywhere - makes a real exchange stall: the three-line timeout
branch itself is verified by review."""
import math
import os

import pytest
import torch

from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu


def _dev():
    return torch.zeros(1, device=DEV).device


@pytest.fixture(autouse=True)
def _status_is_clear_around_every_test():
    from dostransformer_amd import ops
    assert ops.exchange_status(_dev()) == (0, 0, 0, 0)          # before the first test: what a fresh process reads
    yield
    ops.exchange_status(_dev(), clear=True)


def test_selftest_files_a_report_and_the_first_one_keeps_its_kernel_and_tile():
    from dostransformer_amd import _abi, ops
    dev = _dev()
    assert ops.exchange_status(dev) == (_abi.DOSX_EXCHANGE_OK, 0, 0, 0)
    k = _abi.DOSX_EXCHANGE_KERNEL_ENC_CS_FWD
    ops.exchange_selftest(dev, k, 17)
    assert ops.exchange_status(dev) == (_abi.DOSX_EXCHANGE_STALLED, k, 17, 1)
    assert ops.exchange_status(dev) == (_abi.DOSX_EXCHANGE_STALLED, k, 17, 1)           # sticky: reading does not clear
    ops.exchange_selftest(dev, _abi.DOSX_EXCHANGE_KERNEL_MLP_LN_CS_BWD, 3)
    assert ops.exchange_status(dev) == (_abi.DOSX_EXCHANGE_STALLED, k, 17, 2)           # first kernel and tile, two stalls
    assert ops.exchange_status(dev, clear=True) == (_abi.DOSX_EXCHANGE_STALLED, k, 17, 2)
    assert ops.exchange_status(dev) == (0, 0, 0, 0)
    ops.exchange_selftest(dev, _abi.DOSX_EXCHANGE_KERNEL_MLP_LN_CS_FWD, 0)              # tile 0 is a tile, not "none"
    assert ops.exchange_status(dev) == (_abi.DOSX_EXCHANGE_STALLED, _abi.DOSX_EXCHANGE_KERNEL_MLP_LN_CS_FWD, 0, 1)


def _model(H):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(0)
    return DOSTransformer_phonon(2, 1, 118, 4, H, DEV, 0.0).to(DEV)


def test_check_exchanges_raises_names_kernel_and_tile_clears_the_status_and_zeroes_the_counters():
    from dostransformer_amd import _abi, ops, synth
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    dev = _dev()
    ops.check_exchanges(dev)                                                            # clean: returns
    tr = Trainer(_model(64), lr=1e-3, replay=True)                                      # a recorded program owns counters too
    tr.step(synth.phonon_batch(6, seed=2, dtype=torch.float32).to(DEV))
    ops.COUNTERS.take(dev, 8)                                                           # (the eager ring exists)
    torch.cuda.synchronize()
    ring = ops.COUNTERS._bufs[str(dev)][0]
    owned = [r() for r in ops.COUNTERS._recorded if r() is not None]
    assert owned and not bool(ring.any()) and not any(bool(t.any()) for t in owned)     # every launch left its counters at zero
    ring[:8] = 3                                                                        # tickets a stalled launch would leave behind
    owned[0][:1] = 2
    ops.exchange_selftest(dev, _abi.DOSX_EXCHANGE_KERNEL_MLP_LN_CS_BWD, 28)
    ops.exchange_selftest(dev, _abi.DOSX_EXCHANGE_KERNEL_MLP_LN_CS_BWD, 5)
    with pytest.raises(DosxError) as e:
        ops.check_exchanges(dev)
    msg = str(e.value)
    assert "mlp_ln_cs_bwd" in msg and "tile 28" in msg and "2 stalls" in msg and "untrustworthy" in msg, msg
    assert ops.exchange_status(dev) == (0, 0, 0, 0)
    assert not bool(ring.any()) and not any(bool(t.any()) for t in owned) and ops.COUNTERS._bufs[str(dev)][1] == 0
    ops.check_exchanges(dev)                                                            # reported once: clean again
    tr.check()


@pytest.mark.parametrize("H", [64, 128])
def test_replayed_training_steps_on_the_column_split_path_leave_the_status_clear(H):
    from dostransformer_amd import ops, synth
    from dostransformer_amd.train import Trainer
    issued, real_call = [], ops._call

    def counting(name, *a, **k):
        issued.append(name)
        return real_call(name, *a, **k)
    tr = Trainer(_model(H), lr=1e-3, replay=True)
    g = synth.phonon_batch(6, seed=1, dtype=torch.float32).to(DEV)
    ops._call = counting
    try:
        first = float(tr.step(g))                                                       # recorded
    finally:
        ops._call = real_call
    assert "dosx_enc_cs_fwd" in issued and "dosx_mlp_ln_fwd" in issued and "dosx_mlp_ln_bwd" in issued   # the exchanging launches
    assert ops.mlp_ln_cs(int(g.x.shape[0]), 2 * H, 2 * H, H) and ops.enc_cs_supported(int(g.x.shape[0]), 118, H)
    second = float(tr.step(g))                                                          # replayed
    assert math.isfinite(first) and math.isfinite(second) and second != first
    assert ops.exchange_status(_dev()) == (0, 0, 0, 0)
    assert tr.check() is None


def test_checkpoint_save_refuses_to_write_on_top_of_a_reported_stall(tmp_path):
    from dostransformer_amd import _abi, checkpoint, ops, synth
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    model = _model(64)
    tr = Trainer(model, lr=1e-3)
    tr.step(synth.phonon_batch(4, seed=1, dtype=torch.float32).to(DEV))
    path = str(tmp_path / "ckpt.pt")
    ops.exchange_selftest(_dev(), _abi.DOSX_EXCHANGE_KERNEL_MLP_LN_CS_FWD, 9)
    with pytest.raises(DosxError, match=r"mlp_ln_cs_fwd, tile 9 .*1 stall reported"):
        checkpoint.save(path, model, trainer=tr)
    assert not os.path.exists(path) and os.listdir(str(tmp_path)) == []
    checkpoint.save(path, model, trainer=tr)                                            # reported and cleared: the next save writes
    assert os.path.exists(path)


def test_per_crystal_evaluation_raises_on_a_reported_stall():
    from dostransformer_amd import _abi, evaluate, ops, synth
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.loader import DeviceDataset
    from dostransformer_amd.predict import Predictor
    ds = DeviceDataset(synth.phonon_crystals(6, 4, dtype=torch.float32), DEV)
    pred = Predictor(_model(64).eval(), per_crystal_keys=True)
    res = evaluate.test_per_crystal(pred, ds, batch_size=4)
    ops.exchange_selftest(_dev(), _abi.DOSX_EXCHANGE_KERNEL_ENC_CS_FWD, 1)
    with pytest.raises(DosxError, match=r"enc_cs_fwd, tile 1 "):
        evaluate.test_per_crystal(pred, ds, batch_size=4)
    with pytest.raises(DosxError, match=r"enc_cs_fwd, tile 2 "):
        ops.exchange_selftest(_dev(), _abi.DOSX_EXCHANGE_KERNEL_ENC_CS_FWD, 2)
        pred.check()
    again = evaluate.test_per_crystal(pred, ds, batch_size=4)                           # clean again: the same metrics
    assert (again.rmse, again.mse, again.mae) == (res.rmse, res.mse, res.mae)
