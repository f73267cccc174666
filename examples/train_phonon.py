#!/usr/bin/env python3
"""End-to-end Phonon-DOS run on the MI355X path: structures -> graphs (GPU neighbour list) -> device-resident
dataset -> fused training steps -> evaluation -> checkpoint.  The build's own counterpart of the reference driver
`main_phDOS.py` (whose model constructor call and `test_phonon` unpacking do not match its own modules, SURVEY.md
§3.1 — this driver uses the signatures the modules actually have).  No dataset ships with the reference, so by
default it trains on synthetic structures; pass --pickle with a list of
{symbols, positions, cell, phdos, crystal_system, mp_id} dicts to use real ones.

    python examples/train_phonon.py --epochs 5 --crystals 512

--float64 trains as the reference does (main_phDOS.py:15-16,52-55,92): the float64 program, eager, torch.optim.AdamW, and
every crystal attending over its own atoms only (set_per_crystal_keys), so a batch of B crystals is B of the reference's
batch-size-1 samples in one pass - the loss is the sum of their per-crystal terms (main_phDOS.py:109-114 crystal by crystal).

    python examples/train_phonon.py --float64 --epochs 2 --crystals 128 --hidden 64

--float64 --fused runs that training through train64.Trainer64 instead (float64 loss and AdamW kernels, no autograd): per-crystal
keys as above, with the reference's loss of the batch as a whole - ONE rmse over all of its B*51 elements per branch
(main_phDOS.py:109-114).  --replay: recorded launch lists, one per ghost-padded shape bucket; every shuffled batch is collated on
the GPU straight into its bucket's static buffers (Trainer64.step_dataset) and evaluation replays too (predict.Predictor64).

    python examples/train_phonon.py --float64 --fused --replay --epochs 2 --crystals 128 --hidden 64

--embedder graphnetwork trains the reference's GNN-only baseline (main_phDOS.py:74-76) through the fp32 Trainer and Predictor: its
output head runs on its rank structure, the loss is the driver's on its one output, and evaluation goes through
evaluate.test_per_crystal (no attention: batched passes ARE the batch-size-1 numbers).

    python examples/train_phonon.py --embedder graphnetwork --epochs 5

--embedder graphnetwork --float64 trains the baseline as the reference does (main_phDOS.py:15-16,70-72): model(batch), the driver's
loss on its one output, loss.backward(), torch.optim.AdamW.  With --fused the same step runs through train64.GraphnetworkTrainer64
(the float64 head on its rank structure, float64 loss and AdamW kernels), with --replay from recorded launch lists per shape
bucket and evaluation through predict.Predictor64.

    python examples/train_phonon.py --embedder graphnetwork --float64 --fused --replay --epochs 2 --crystals 128 --hidden 64

Fine-tuning: --init CKPT loads a trained model (the optimizer starts fresh), --train-only / --freeze take parameter-name
prefixes (FusedModel.train_only / freeze).  Frozen parameters are bitwise untouched - no weight decay either - and the backward
program drops what only they needed: with the GNN trunk frozen it ends behind the first encoder.  Every mode above takes them.

    python examples/train_phonon.py --init phonon_best.pt --train-only prompt_token fc_prompt --epochs 2 --out phonon_ft.pt
    python examples/train_phonon.py --init phonon_best.pt --freeze GN_encoder stacked_processor GN_decoder --epochs 2

Optimizer parameter groups (fused trainers; next to --init / --freeze / --train-only): --group PREFIX[,PREFIX...]:lr=X[:wd=Y]
(repeatable) trains the named parameters at their own rate / weight decay, --no-decay-norms keeps biases, norms, slopes,
embeddings and prompt tokens out of the weight decay, --layerwise-lr-decay D lowers the rate layer by layer towards the input.

    python examples/train_phonon.py --init phonon_best.pt --group GN_encoder.,stacked_processor.,GN_decoder.:lr=1e-5 --no-decay-norms
    python examples/train_phonon.py --float64 --fused --layerwise-lr-decay 0.8 --epochs 2 --crystals 128 --hidden 64

Averaged weights (fused trainers): --ema DECAY keeps an exponential moving average of the weights inside the AdamW launch
(--no-ema-warmup: the decay from the first step on).  Every evaluation also prints the metrics under the averaged weights
(trainer.ema_weights()), the checkpoint carries both weight sets, --save-ema PATH writes the averaged model alone.

    python examples/train_phonon.py --ema 0.999 --eval-per-crystal 64 --save-ema phonon_ema.pt

Gradient accumulation (fused trainers): --accumulate K groups K consecutive batches of the epoch into one optimizer step on the
objective of their concatenation (trainer.step_accumulate / step_dataset_accumulate; the last window of an epoch may be shorter).
The reference's pooled RMSE does not accumulate, so K > 1 needs one of the per-crystal --loss kinds.

    python examples/train_phonon.py --accumulate 4 --batch-size 16 --loss crystal_rmse --per-crystal-keys

Class-balanced training (fused trainers, with a per-crystal --loss): --balance-systems [POWER] weighs every training crystal by
count[its crystal system] ** -POWER (default 1), normalised to mean 1 (weights.balanced -> DeviceDataset.set_weights ->
Trainer(sample_weights=True): the loss becomes sum_b w_b l_b / B, the weights ride on the batch or are gathered by the loss launch).

    python examples/train_phonon.py --loss crystal_rmse --per-crystal-keys --balance-systems 0.5

A cumulative-DOS term (fused trainers, with a per-crystal --loss): --cdf-loss LAM[,sq|abs] adds LAM times the Cramer (sq) or the
Wasserstein-1 (abs) distance between predicted and target cumulative DOS to every crystal's loss (functionals.cumulative ->
Trainer(functionals=...): the same loss launch).  --report-heat-capacity T[,T...] prints, at every evaluation, the mean absolute
error of the harmonic C_V(T) of the predicted DOS, computed on the device from the per-crystal evaluator's outputs.

    python examples/train_phonon.py --loss crystal_rmse --cdf-loss 0.5 --eval-per-crystal 64 --report-heat-capacity 100,300,1000

Normalised functionals (rows over one floored denominator, functionals.centre / functionals.normalised_cumulative): --mean-frequency-loss
LAM[,sq|abs] penalises the error of the mean frequency m1 / m0 (on a grid of unit length), --cdf-loss LAM,sq|abs,norm compares the
cumulative curves of the DOS as SHAPES, each over its own total.  One functional term per run.  Such a term leaves the scale of the
prediction free; the per-crystal --loss next to it carries the scale.  --functional-floor X is the floor of the denominator m0 (below
it the denominator is the constant X); without it the driver takes 1e-3 times the median m0 of the training targets and prints it.

    python examples/train_phonon.py --loss crystal_rmse --mean-frequency-loss 0.5
    python examples/train_phonon.py --loss crystal_rmse --cdf-loss 0.5,abs,norm --functional-floor 1e-4
"""
import argparse
import os
import pickle
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dostransformer_amd import checkpoint, evaluate, featurize, functionals, ops, param_groups, spectra, synth, validate, weights  # noqa: E402
from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon  # noqa: E402
from dostransformer_amd.loader import DeviceDataset  # noqa: E402
from dostransformer_amd.predict import Predictor  # noqa: E402
from dostransformer_amd.train import Trainer  # noqa: E402


def main(argv=None):
    """_main() with batch validation on (--no-validate: off); the process-wide switch gets its earlier setting back on the way out,
    so a caller that imports this module and runs main() is left as it was."""
    state = validate.ENABLED, validate.FINITE
    try:
        return _main(argv)
    finally:
        validate.enable(*state)


def _main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=3)          # utils.py:29-42 defaults
    ap.add_argument("--transformer", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--embedder", default="DOSTransformer_phonon", choices=["DOSTransformer_phonon", "graphnetwork"])   # utils.py:38
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--r-max", type=float, default=4.0)       # main_phDOS.py:21
    ap.add_argument("--crystals", type=int, default=512)
    ap.add_argument("--pickle", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--crystal-system", default="given", choices=["given", "derive", "check"],
                    help="prompt labels: as the entries give them; derived from the structure where an entry has none; or every "
                         "label derived and compared with the given one (symmetry.crystal_systems; a mismatch stops the run)")
    ap.add_argument("--symprec", type=float, default=0.1, metavar="X", help="with --crystal-system derive / check: distance tolerance in angstrom")
    ap.add_argument("--raw-dos", type=float, default=None, metavar="SIGMA",
                    help="build phdos on the GPU from raw spectra broadened by SIGMA: mode frequencies with q-point weights, or a tabulated "
                         "DOS (featurize.build_data_all(targets=spectra.PhononTargets(...))); synthetic structures get synthetic spectra "
                         "(synth.raw_phonon), a --pickle's entries bring their own `frequencies` / `dos`")
    ap.add_argument("--out", default="phonon_best.pt")
    ap.add_argument("--no-validate", action="store_true",
                    help="skip batch validation (validate.enable: every crystal and every first-seen batch is checked for out-of-range "
                         "indices, cross-crystal edges, bad crystal-system labels and NaN / inf before a kernel reads it)")
    ap.add_argument("--float64", action="store_true", help="the reference's float64 training with per-crystal keys")
    ap.add_argument("--fused", action="store_true", help="with --float64: train64.Trainer64 instead of autograd + torch.optim.AdamW")
    ap.add_argument("--replay", action="store_true", help="with --float64 --fused: replay recorded launch lists, one per shape bucket (step_dataset + Predictor64)")
    ap.add_argument("--per-crystal-keys", action="store_true",
                    help="fp32 trainer: attend over each crystal's own atoms - what the reference's batch_size = 1 training computes")
    ap.add_argument("--eval-per-crystal", type=int, default=0, metavar="N",
                    help="N > 0: validate and test with the reference's batch-size-1 metrics, from batched passes of N crystals "
                         "(evaluate.test_per_crystal; fp32 run, or --float64 --fused --replay)")
    ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="X",
                    help="fused trainers: clip the gradient norm to X on the device (what clip_grad_norm_ does in a torch loop); "
                         "steps with a non-finite gradient are skipped")
    ap.add_argument("--skip-nonfinite", action="store_true",
                    help="fused trainers: skip a step whose gradient holds a NaN / inf instead of writing it into the parameters")
    ap.add_argument("--init", default=None, metavar="CKPT",
                    help="fine-tuning: load the model from this checkpoint (checkpoint.save's file or a bare state_dict); the optimizer starts fresh")
    ap.add_argument("--train-only", nargs="+", default=None, metavar="PREFIX",
                    help="fine-tuning: train exactly the parameters whose names start with one of these prefixes, freeze the rest")
    ap.add_argument("--freeze", nargs="+", default=None, metavar="PREFIX",
                    help="fine-tuning: freeze the parameters whose names start with one of these prefixes")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY",
                    help="fused trainers: keep an exponential moving average of the weights inside the AdamW launch (decay in [0, 1), "
                         "e.g. 0.999); every evaluation also reports the metrics under the averaged weights, and the checkpoint "
                         "carries both weight sets")
    ap.add_argument("--no-ema-warmup", action="store_true", help="with --ema: the decay from the first step on, no min(decay, (1 + t) / (10 + t))")
    ap.add_argument("--save-ema", default=None, metavar="PATH", help="with --ema: write the averaged model alone to PATH at the end of the run")
    ap.add_argument("--loss", default="reference", choices=["reference", "crystal_rmse", "mse", "mae", "huber"],
                    help="fused trainers: the training objective - the reference driver's (ONE RMSE pooled over the batch, "
                         "main_phDOS.py:109-114) or the mean over crystals of each crystal's own RMSE / MSE / MAE / Huber term; "
                         "crystal_rmse is what the reference optimises at its batch_size = 1 (with --per-crystal-keys, or --float64 "
                         "--fused, a step follows the mean of the batch-1 gradients)")
    ap.add_argument("--huber-delta", type=float, default=None, metavar="X", help="with --loss huber: torch.nn.HuberLoss's delta")
    ap.add_argument("--accumulate", type=int, default=1, metavar="K",
                    help="fused trainers: one optimizer step per K consecutive batches, on the objective of their concatenation "
                         "(gradient accumulation; K > 1 needs a per-crystal --loss)")
    ap.add_argument("--balance-systems", type=float, nargs="?", const=1.0, default=None, metavar="POWER",
                    help="fused trainers: class-balanced sample weights over the 7 crystal systems, w ~ count[system] ** -POWER "
                         "(default 1), mean 1 over the training set (weights.balanced; sample_weights=True); needs a per-crystal --loss")
    ap.add_argument("--mean-frequency-loss", default=None, metavar="LAM[,sq|abs]",
                    help="LAM times the (squared: sq, default; absolute: abs) error of the mean frequency m1 / m0 next to the per-crystal "
                         "loss, on a grid of unit length (functionals.centre; functionals=...); needs a per-crystal --loss")
    ap.add_argument("--functional-floor", type=float, default=None, metavar="X",
                    help="floor of the denominator m0 of --mean-frequency-loss / --cdf-loss ...,norm (default: 1e-3 times the median m0 "
                         "of the training targets, printed)")
    ap.add_argument("--cdf-loss", default=None, metavar="LAM[,sq|abs[,norm]]",
                    help="fused trainers: LAM times the distance between the cumulative DOS curves next to the per-crystal loss - sq "
                         "(default): Cramer, abs: Wasserstein-1 (functionals.cumulative; functionals=...); needs a per-crystal --loss")
    ap.add_argument("--report-heat-capacity", default=None, metavar="T[,T...]",
                    help="with --eval-per-crystal: the mean absolute error of the harmonic C_V(T) (k_B per mode, on the 51-point grid "
                         "over 0 .. 1000 cm^-1) of predicted against target DOS at the temperatures T in K, computed on the device "
                         "(functionals.heat_capacity; evaluate.functionals_per_crystal)")
    param_groups.add_arguments(ap)
    args = ap.parse_args(argv)
    args.cdf_loss = _parse_cdf(ap, "--cdf-loss", args.cdf_loss, norm=True)
    args.mean_frequency_loss = _parse_cdf(ap, "--mean-frequency-loss", args.mean_frequency_loss)
    if args.cdf_loss is not None and args.mean_frequency_loss is not None:
        ap.error("--cdf-loss and --mean-frequency-loss: one functional term per run (a trainer takes one table with one weight and one "
                 "kind: functionals.stack(...) in code)")
    if args.mean_frequency_loss is not None and args.loss == "reference":
        ap.error("--mean-frequency-loss adds a term to the per-crystal losses: pick --loss crystal_rmse or another per-crystal --loss")
    if args.functional_floor is not None and not (args.mean_frequency_loss is not None or (args.cdf_loss or (0, 0, False))[2]):
        ap.error("--functional-floor belongs to --mean-frequency-loss or --cdf-loss LAM,KIND,norm")
    if args.functional_floor is not None and not 0.0 < args.functional_floor < float("inf"):
        ap.error("--functional-floor X: finite and > 0")
    if args.cdf_loss is not None and args.loss == "reference":
        ap.error("--cdf-loss adds a term to the per-crystal losses: pick --loss crystal_rmse (the reference's own batch-1 objective), "
                 "mse, mae or huber")
    if args.report_heat_capacity is not None:
        try:
            args.report_heat_capacity = [float(t) for t in args.report_heat_capacity.split(",")]
            assert args.report_heat_capacity and min(args.report_heat_capacity) > 0
        except (ValueError, AssertionError):
            ap.error("--report-heat-capacity T[,T...]: positive temperatures in K")
        if args.eval_per_crystal <= 0 and args.embedder != "graphnetwork":
            ap.error("--report-heat-capacity reads the per-crystal evaluator's outputs: pass --eval-per-crystal N")
    if args.balance_systems is not None and args.loss == "reference":
        ap.error("--balance-systems weighs the per-crystal losses: pick --loss crystal_rmse (the reference's own batch-1 objective), "
                 "mse, mae or huber")
    if args.accumulate < 1:
        ap.error("--accumulate K: K is at least 1")
    if args.accumulate > 1 and args.float64 and not args.fused:
        ap.error("--accumulate belongs to the fused trainers: the fp32 run, or --float64 --fused")
    if args.accumulate > 1 and args.loss == "reference":
        ap.error("--accumulate K > 1: the reference's pooled RMSE does not accumulate over batches - pick --loss crystal_rmse "
                 "(its own batch-1 objective), mse, mae or huber")
    if (args.loss == "huber") != (args.huber_delta is not None):
        ap.error("--huber-delta X belongs to --loss huber, and --loss huber needs it")
    if args.loss != "reference" and args.float64 and not args.fused:
        ap.error("--loss belongs to the fused trainers: the fp32 run, or --float64 --fused")
    if args.ema is not None and args.float64 and not args.fused:
        ap.error("--ema belongs to the fused trainers: the fp32 run, or --float64 --fused")
    if (args.no_ema_warmup or args.save_ema) and args.ema is None:
        ap.error("--no-ema-warmup / --save-ema need --ema DECAY")
    if (args.clip_grad_norm is not None or args.skip_nonfinite) and args.float64 and not args.fused:
        ap.error("--clip-grad-norm / --skip-nonfinite belong to the fused trainers: the fp32 run, or --float64 --fused")
    if param_groups.wanted(args) and args.float64 and not args.fused:
        ap.error("--group / --no-decay-norms / --layerwise-lr-decay belong to the fused trainers: the fp32 run, or --float64 --fused")
    if args.eval_per_crystal > 0 and args.float64 and not args.replay:
        ap.error("--eval-per-crystal needs a replayed predictor: the fp32 run, or --float64 --fused --replay")
    if args.fused and not args.float64:
        ap.error("--fused selects the float64 trainer: use it with --float64 (the fp32 run is fused already)")
    baseline = args.embedder == "graphnetwork"
    if baseline and (args.per_crystal_keys or args.beta != 1.0):
        ap.error("--embedder graphnetwork: one output, no attention: no --per-crystal-keys, --beta")
    if args.replay and not args.fused:
        ap.error("--replay belongs to --float64 --fused (the fp32 run always replays)")
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    validate.enable(not args.no_validate, finite=True)

    entries = pickle.load(open(args.pickle, "rb")) if args.pickle else synth.phonon_structures(args.crystals, args.seed)
    targets = None
    if args.raw_dos is not None:
        # raw spectra -> phdos on the GPU; the window (0 .. 7.5 in the synthetic spectra's unit) is this example's, not the paper's
        if not args.pickle:
            entries = synth.raw_phonon(entries, args.seed)
        targets = spectra.PhononTargets(spectra.Grid.linspace(0.0, 7.5, synth.PH_BINS, unit="THz"), args.raw_dos)
    t0 = time.perf_counter()
    crystals = featurize.build_data_all(entries, r_max=args.r_max, device=dev,
                                        dtype=torch.float64 if args.float64 else torch.float32,
                                        crystal_system=args.crystal_system, symprec=args.symprec, targets=targets)
    print(f"{len(crystals)} crystals -> graphs in {time.perf_counter() - t0:.2f} s "
          f"({sum(c['edge_index'].shape[1] for c in crystals)} edges)")
    perm = np.random.default_rng(args.seed).permutation(len(crystals))
    n_val = max(1, len(perm) // 10)
    split = {"valid": perm[:n_val], "test": perm[n_val:2 * n_val], "train": perm[2 * n_val:]}
    ds = {k: DeviceDataset([crystals[i] for i in idx], dev, dtype=torch.float64 if args.float64 else None)
          for k, idx in split.items()}
    if args.balance_systems is not None:                           # resident table: set once, read by every loss launch
        sysw = weights.balanced(ds["train"]._graph["system"].cpu(), power=args.balance_systems)
        ds["train"].set_weights(sysw)
        print(f"--balance-systems {args.balance_systems:g}: sample weights {float(sysw.min()):.3g} .. {float(sysw.max()):.3g}, mean 1")

    args.functional_term = _functional_term(args, ds["train"])
    if args.float64:
        return train_float64_fused(args, ds, dev) if args.fused else train_float64(args, ds, dev)
    if baseline:
        from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
        model = Graphnetwork_phonon(args.layers, 118, 4, args.hidden, 51, dev).to(dev)
        if args.eval_per_crystal <= 0:
            args.eval_per_crystal = args.batch_size      # (its predictor returns one DOS: the per-crystal evaluator reads it)
    else:
        model = DOSTransformer_phonon(args.layers, args.transformer, 118, 4, args.hidden, dev, 0.0).to(dev)
    _fine_tune(args, model)
    # coarse shape buckets: reshuffled batches then fall into a few dozen (N, E, n_max) buckets that are all recorded
    # within the first epoch (ghost padding is exact; it costs a few per cent of extra rows)
    trainer = Trainer(model, lr=args.lr, beta=args.beta, replay=True, bucket=(32, 1024), promote=0.08,
                      per_crystal_keys=args.per_crystal_keys, param_groups=_groups(args, model), **_guard_args(args),
                      **_ema_args(args), **_loss_args(args))
    predictor = Predictor(model, bucket=(32, 1024), per_crystal_keys=args.eval_per_crystal > 0 and not baseline)
    run_test = _tester(args, predictor, ds)
    best, history = float("inf"), []
    for epoch in range(args.epochs):
        model.train()
        t0, losses, seen = time.perf_counter(), [], 0
        for window in _windows(ds["train"].batches(args.batch_size, shuffle=True, seed=args.seed + epoch), args.accumulate):
            # (a window's loss lives in a scalar the trainer owns: cloned)
            losses.append(trainer.step(window[0]) if args.accumulate == 1 else trainer.step_accumulate(window).clone())
            seen += sum(batch.num_graphs for batch in window)
        loss = float(torch.stack(losses).mean())                  # one host read per epoch
        dt = time.perf_counter() - t0
        history.append(loss)
        rmse, mse, mae, r2v = run_test("valid")
        _check(trainer)                                           # once per evaluation: a stalled exchange voids the epoch
        print(f"[epoch {epoch + 1}/{args.epochs}] loss {loss:.4f} | {seen / dt:8.0f} crystals/s | "
              f"valid rmse {rmse:.4f} mse {mse:.4f} mae {mae:.4f} r2 {r2v:.4f}")
        _ema_report(args, trainer, run_test, "valid")
        if rmse < best:
            best = rmse
            checkpoint.save(args.out, model, trainer)
            t = run_test("test")
            print(f"            test rmse {t[0]:.4f} mse {t[1]:.4f} mae {t[2]:.4f} r2 {t[3]:.4f}   (saved {args.out})")
            _ema_report(args, trainer, run_test, "test")
    _save_ema(args, model, trainer)
    return {"best_valid_rmse": best, "train_loss": history}


def _windows(items, k):
    """--accumulate K: the items of an epoch in lists of K consecutive ones; the last list may be shorter."""
    window = []
    for item in items:
        window.append(item)
        if len(window) == k:
            yield window
            window = []
    if window:
        yield window


def _ema_args(args):
    return dict(ema_decay=args.ema, ema_warmup=not args.no_ema_warmup)


def _parse_cdf(ap, flag, text, norm=False):
    """FLAG LAM[,sq|abs[,norm]] -> None or (lam, kind, normalised); the third part only where `norm` allows it"""
    if text is None:
        return None
    parts = text.split(",")
    try:
        lam, kind = float(parts[0]), (parts[1] if len(parts) > 1 else "sq")
        assert len(parts) <= (3 if norm else 2) and kind in ("sq", "abs") and 0.0 <= lam < float("inf")
        assert len(parts) < 3 or parts[2] == "norm"
    except (ValueError, AssertionError):
        ap.error(f"{flag} LAM[,sq|abs{'[,norm]' if norm else ''}]: a finite weight >= 0 and, optionally, the kind"
                 + (" and `norm`" if norm else ""))
    return lam, kind, len(parts) == 3


def _functional_term(args, train, S=51):
    """--cdf-loss / --mean-frequency-loss -> None or (Functionals, lam, kind), on a grid of unit length: bin width 1 / S.  The floor
    of a normalised term: --functional-floor, or 1e-3 times the median m0 of the training targets, computed once."""
    flag = args.mean_frequency_loss or args.cdf_loss
    if flag is None:
        return None
    lam, kind, norm = flag
    if args.mean_frequency_loss is None and not norm:
        return functionals.cumulative(S, 1.0 / S), lam, kind
    floor = args.functional_floor
    if floor is None:
        floor = 1e-3 * float((train._graph["phdos"].double().sum(1) / S).median())
        print(f"--functional-floor {floor:.6g}   (1e-3 x the median m0 of the {len(train)} training targets)")
    if args.mean_frequency_loss is not None:
        return functionals.centre((torch.arange(S, dtype=torch.float64) + 0.5) / S, floor, de=1.0 / S), lam, kind
    return functionals.normalised_cumulative(S, floor, 1.0 / S), lam, kind


def _loss_args(args):
    kw = dict(loss=None if args.loss == "reference" else args.loss, huber_delta=args.huber_delta,
              sample_weights=args.balance_systems is not None)
    if args.functional_term is not None:
        fn, lam, kind = args.functional_term
        kw.update(functionals=fn, functional_weight=lam, functional_kind=kind)
    return kw


def _ema_report(args, trainer, run_test, name):
    """--ema: the split's metrics under the averaged weights - one swap launch in, the same evaluator (nothing re-recorded), one out."""
    if args.ema is None:
        return
    with trainer.ema_weights():
        t = run_test(name)
    print(f"            ema {name} rmse {t[0]:.4f} mse {t[1]:.4f} mae {t[2]:.4f} r2 {t[3]:.4f}")


def _save_ema(args, model, trainer):
    """--save-ema PATH: the averaged model alone, as a checkpoint any plain module loads (checkpoint.load(PATH, model))."""
    if args.save_ema:
        with trainer.ema_weights():
            checkpoint.save(args.save_ema, model, extra={"ema_decay": trainer.ema_decay})
        print(f"averaged weights saved to {args.save_ema}")


def _fine_tune(args, model):
    """--init / --train-only / --freeze: the model from a checkpoint (no optimizer state: a fresh one), then the frozen set.
    ``requires_grad`` is what every driver reads - the fused trainers through the flat layout, torch.optim.AdamW through
    ``grad is None``."""
    if args.init:
        checkpoint.load(args.init, model)
    if args.train_only:
        model.train_only(*args.train_only)
    if args.freeze:
        model.freeze(*args.freeze)
    if args.train_only or args.freeze:
        names = model.trainable_names()
        n = sum(p.numel() for k, p in model.named_parameters() if k in set(names))
        print(f"fine-tuning: {len(names)} parameter tensors ({n} elements) train, the rest is frozen")
    return model


def _groups(args, model):
    """--group / --no-decay-norms / --layerwise-lr-decay -> the trainer's ``param_groups=`` (None: none given), after the frozen set:
    a group may name frozen parameters, they stay untouched."""
    groups = param_groups.from_args(model, args, args.lr)
    if groups is not None:
        for k, grp in enumerate(param_groups.resolve(model, groups, args.lr, 1e-2)):
            print(f"param group {k}: lr {grp['lr']:.3g} weight_decay {grp['weight_decay']:.3g}, {len(grp['names'])} tensors")
    return groups


def _tester(args, evaluator, ds):
    """name of a split -> (rmse, mse, mae, r2).  --eval-per-crystal N: the reference's numbers (main_phDOS.py:52-55 evaluates at
    batch size 1) from passes of N crystals through a predictor with per-crystal keys; otherwise test_phonon over batches of
    --batch-size, whose R2 and means are those of the batches."""
    if args.eval_per_crystal > 0:
        def run(name):
            res = evaluate.test_per_crystal(evaluator, ds[name], batch_size=args.eval_per_crystal)
            if args.report_heat_capacity is not None:        # --report-heat-capacity: from the outputs still on the device
                nu = torch.linspace(0.0, 1000.0, int(res.preds.shape[1]), dtype=torch.float64)
                cv = evaluate.functionals_per_crystal(res, functionals.heat_capacity(nu, args.report_heat_capacity))
                print(f"            {name} C_V mae " + "  ".join(f"{n} {e:.4g}" for n, e in zip(cv.names, cv.mae)))
            return res.as_reference()
        return run
    return lambda name: evaluate.test_phonon(evaluator, ds[name].batches(args.batch_size))


def _baseline64(args, dev):
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    return Graphnetwork_phonon(args.layers, 118, 4, args.hidden, 51, dev).double().to(dev)


def train_float64(args, ds, dev):
    """Eager float64 training: model(batch), loss.backward(), torch.optim.AdamW (the fp32 drivers Trainer / Predictor refuse
    a float64 module).  evaluate.test_phonon takes the module itself.  --embedder graphnetwork: the baseline's one output under
    the reference's loss of the batch, ONE rmse over all of its elements (main_phDOS.py:109-111)."""
    baseline = args.embedder == "graphnetwork"
    if baseline:
        model = _baseline64(args, dev)
    else:
        model = DOSTransformer_phonon(args.layers, args.transformer, 118, 4, args.hidden, dev, 0.0).double()
        model = model.set_program_dtype(torch.float64).set_per_crystal_keys(True).to(dev)
    _fine_tune(args, model)
    opt = torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=1e-2)       # main_phDOS.py:92
    best, history = float("inf"), []
    for epoch in range(args.epochs):
        model.train()
        t0, total, seen = time.perf_counter(), torch.zeros((), dtype=torch.float64, device=dev), 0
        for batch in ds["train"].batches(args.batch_size, shuffle=True, seed=args.seed + epoch):
            if baseline:
                dos = model(batch)
                rmse_all = torch.sqrt(((dos - batch.phdos.reshape(dos.shape).to(torch.float64)) ** 2).mean())
                opt.zero_grad()
                rmse_all.backward()
                opt.step()
                total += rmse_all.detach() * batch.num_graphs
                seen += batch.num_graphs
                continue
            dos_global, _, dos_system = model(batch)
            y = batch.phdos.reshape(dos_global.shape[0], -1).to(torch.float64)
            # the reference's loss of one batch-size-1 sample, for every crystal of the batch; summed, so the gradient is
            # the sum of the per-sample gradients
            per_crystal = (torch.sqrt(((dos_global - y) ** 2).mean(dim=1)) +
                           args.beta * torch.sqrt(((dos_system - y) ** 2).mean(dim=1)))
            opt.zero_grad()
            per_crystal.sum().backward()
            opt.step()
            total += per_crystal.detach().sum()
            seen += batch.num_graphs
        loss = float(total) / max(seen, 1)                          # one host read per epoch
        dt = time.perf_counter() - t0
        history.append(loss)
        rmse, mse, mae, r2v = evaluate.test_phonon(model, ds["valid"].batches(args.batch_size))
        ops.check_exchanges(dev)                                    # (no trainer object here: the same check, once per evaluation)
        print(f"[epoch {epoch + 1}/{args.epochs}] loss per crystal {loss:.4f} | {seen / dt:8.0f} crystals/s | "
              f"valid rmse {rmse:.4f} mse {mse:.4f} mae {mae:.4f} r2 {r2v:.4f}")
        if rmse < best:
            best = rmse
            checkpoint.save(args.out, model)
            t = evaluate.test_phonon(model, ds["test"].batches(args.batch_size))
            print(f"            test rmse {t[0]:.4f} mse {t[1]:.4f} mae {t[2]:.4f} r2 {t[3]:.4f}   (saved {args.out})")
    return {"best_valid_rmse": best, "train_loss": history}


def _guard_args(args):
    return dict(max_grad_norm=args.clip_grad_norm, skip_nonfinite=args.skip_nonfinite)


def _check(trainer):
    """trainer.check(); behind the gradient guard skipped steps left parameters and moments untouched, so the run reports them and
    goes on - without it a reported stall ends the run, as before."""
    from dostransformer_amd._lib import DosxError
    try:
        trainer.check()
    except DosxError as e:
        if not trainer.guarded:
            raise
        print(f"            warning: {e}")


def train_float64_fused(args, ds, dev):
    """float64 training through train64.Trainer64: forward program, loss kernel, backward program, flat AdamW - the loss stays
    on the device, one host read per epoch.  --replay: shape buckets as in the fp32 run, every shuffled selection collated on
    the device straight into its bucket (step_dataset, one n_max for the whole dataset - with per-crystal keys the numbers do
    not depend on it) and evaluation through Predictor64.  The checkpoint carries the optimizer state (Trainer64.state_dict).
    --embedder graphnetwork: the same through train64.GraphnetworkTrainer64 (one output, no keys to switch)."""
    from dostransformer_amd.predict import Predictor64
    from dostransformer_amd.train64 import GraphnetworkTrainer64, Trainer64
    bucket = (32, 1024)
    slots = dict(replay=args.replay, bucket=bucket if args.replay else None, promote=0.08 if args.replay else 0.0)
    if args.embedder == "graphnetwork":
        model = _fine_tune(args, _baseline64(args, dev))
        trainer = GraphnetworkTrainer64(model, lr=args.lr, param_groups=_groups(args, model), **slots, **_guard_args(args),
                                        **_ema_args(args), **_loss_args(args))
    else:
        model = DOSTransformer_phonon(args.layers, args.transformer, 118, 4, args.hidden, dev, 0.0).double()
        model = model.set_program_dtype(torch.float64).set_per_crystal_keys(True).to(dev)
        _fine_tune(args, model)
        trainer = Trainer64(model, lr=args.lr, beta=args.beta, param_groups=_groups(args, model), **slots, **_guard_args(args),
                            **_ema_args(args), **_loss_args(args))
    evaluator = Predictor64(model, bucket=bucket) if args.replay else model       # (the module's per-crystal keys are on)
    run_test = _tester(args, evaluator, ds)
    train = ds["train"]
    n_max = int(train.n_nodes.max())
    best, history = float("inf"), []
    for epoch in range(args.epochs):
        model.train()
        t0, losses, seen = time.perf_counter(), [], 0
        order = np.random.default_rng(args.seed + epoch).permutation(len(train))
        for sels in _windows((order[i:i + args.batch_size] for i in range(0, len(order), args.batch_size)), args.accumulate):
            if args.accumulate == 1:
                losses.append(trainer.step_dataset(train, sels[0], n_max=n_max).clone())     # (replay: the loss lives in the slot's buffer)
            else:
                losses.append(trainer.step_dataset_accumulate(train, sels, n_max=n_max).clone())
            seen += sum(len(sel) for sel in sels)
        loss = float(torch.stack(losses).mean())                  # one host read per epoch
        dt = time.perf_counter() - t0
        history.append(loss)
        rmse, mse, mae, r2v = run_test("valid")
        _check(trainer)
        print(f"[epoch {epoch + 1}/{args.epochs}] loss {loss:.4f} | {seen / dt:8.0f} crystals/s | "
              f"valid rmse {rmse:.4f} mse {mse:.4f} mae {mae:.4f} r2 {r2v:.4f}"
              + (f" | slots {trainer.slot_misses} recorded, {trainer.slot_hits} replayed ({trainer.slot_promoted} promoted)"
                 if args.replay else ""))
        _ema_report(args, trainer, run_test, "valid")
        if rmse < best:
            best = rmse
            checkpoint.save(args.out, model, trainer)
            t = run_test("test")
            print(f"            test rmse {t[0]:.4f} mse {t[1]:.4f} mae {t[2]:.4f} r2 {t[3]:.4f}   (saved {args.out})")
            _ema_report(args, trainer, run_test, "test")
    _save_ema(args, model, trainer)
    return {"best_valid_rmse": best, "train_loss": history}


if __name__ == "__main__":
    main()
