#!/usr/bin/env python3
"""End-to-end Electron-DOS run on the MI355X path: crystal graphs -> device-resident dataset -> fused training steps
(collated on the GPU straight into the shape bucket) -> batch-1 evaluation -> checkpoint.  The build's counterpart of the
reference driver `main_eDOS.py` (loop `:101-127`, evaluation / model selection / early stopping `:132-175`); flags and
defaults are those of `utils.py:25-43`.  The Materials-Project graphs (`data/processed/dos_dataset_random.pt`, built by
`data/mat2graph.py` from downloads) do not ship with the reference, so by default it trains on synthetic graphs of the same
layout; pass --pickle with a list of {x [n+1,200] (phantom zero node last, `mat2graph.py:155-158`),
edge_index [2,E], edge_attr [E,41], glob [2], system, y_ft [201], mp_id} dicts (tensors) to use real ones, or --structures N
to start from N synthetic *structures* (atomic numbers, positions, cell) and build their graphs on the GPU with
featurize.build_edos_all - the route a list of real structures takes (`data/mat2graph.py:120-243` without pymatgen).

    python examples/train_edos.py --epochs 10 --crystals 512 --batch_size 64
    python examples/train_edos.py --structures 256 --epochs 1

--embedder graphnetwork / mlp trains the reference's GNN-only baselines (`main_eDOS.py:71-81`) through the same Trainer and
Predictor: their output head runs on its rank structure, the loss is the driver's on their one output, and evaluation always goes
through evaluate.test_per_crystal (these models have no attention: batched passes ARE the batch-size-1 numbers).

    python examples/train_edos.py --embedder graphnetwork --epochs 10

Fine-tuning: --init CKPT loads a trained model (the optimizer starts fresh), --train-only / --freeze take parameter-name
prefixes (FusedModel.train_only / freeze; the prompt table of this model is spelt `promt_token`, as upstream).  Frozen
parameters are bitwise untouched - no weight decay either - and the backward program drops what only they needed.

    python examples/train_edos.py --init edos_best.pt --train-only promt_token fc_prompt --epochs 20 --out edos_ft.pt

Optimizer parameter groups (next to --init / --freeze / --train-only): --group PREFIX[,PREFIX...]:lr=X[:wd=Y] (repeatable) trains
the named parameters at their own rate / weight decay, --no-decay-norms keeps biases, norms, slopes, embeddings and prompt tokens
out of the weight decay, --layerwise-lr-decay D lowers the rate layer by layer towards the input (param_groups.py).

    python examples/train_edos.py --init edos_best.pt --group GN_encoder.,stacked_processor.,GN_decoder.:lr=1e-5 --no-decay-norms

Gradient accumulation: --accumulate K groups K consecutive batches of the epoch into one optimizer step on the objective of their
concatenation (every loss, the reference's included: each is a mean over crystals).

    python examples/train_edos.py --accumulate 4 --batch_size 16

Weighted losses (with a per-crystal --loss; on this model --loss crystal_rmse is the reference's objective): --balance-systems
[POWER] weighs every training crystal by count[its crystal system] ** -POWER, normalised to mean 1 (weights.balanced; the loss
launch gathers the weights out of the dataset's table); --fermi-weight CENTER,WIDTH[,FLOOR] weighs the 201 energy bins by a
Gaussian bump around bin CENTER on a floor (weights.fermi_window).

    python examples/train_edos.py --loss crystal_rmse --balance-systems 0.5 --fermi-weight 100,20,0.25
"""
import argparse
import os
import pickle
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dostransformer_amd import checkpoint, evaluate, featurize, functionals, param_groups, spectra, synth, validate, weights  # noqa: E402
from dostransformer_amd._lib import DosxError  # noqa: E402
from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer  # noqa: E402
from dostransformer_amd.loader import DeviceDataset  # noqa: E402
from dostransformer_amd.predict import Predictor  # noqa: E402
from dostransformer_amd.train import Trainer  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()                                  # `utils.py:25-43`, same names and defaults
    ap.add_argument("--device", "-d", type=int, default=0)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--epochs", type=int, default=1000)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--layers", "-l", type=int, default=3)
    ap.add_argument("--transformer", "-t", type=int, default=2)
    ap.add_argument("--eval", type=int, default=5)
    ap.add_argument("--es", type=int, default=50)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--random_state", type=int, default=0)
    ap.add_argument("--attn_drop", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--embedder", default="DOSTransformer", choices=["DOSTransformer", "graphnetwork", "mlp"])   # `utils.py:38`
    # (not upstream: the data source and the output file)
    ap.add_argument("--crystals", type=int, default=512, help="synthetic graphs to generate when no --pickle is given")
    ap.add_argument("--pickle", default=None)
    ap.add_argument("--structures", type=int, default=0,
                    help="build the graphs of this many synthetic structures with featurize.build_edos_all (0: off)")
    ap.add_argument("--crystal-system", default="given", choices=["given", "derive", "check"],
                    help="with --structures: prompt labels as the entries give them; derived from the structure where an entry has "
                         "none; or every label derived and compared with the given one (a mismatch stops the run)")
    ap.add_argument("--symprec", type=float, default=0.1, metavar="X", help="with --crystal-system derive / check: distance tolerance in angstrom")
    ap.add_argument("--raw-dos", type=float, default=None, metavar="SIGMA",
                    help="with --structures: give the structures synthetic raw spectra (synth.raw_edos) and build y_ft / y from them on "
                         "the GPU, broadened by SIGMA eV (featurize.build_edos_all(targets=spectra.EdosTargets(...)))")
    ap.add_argument("--eval_batch_size", type=int, default=1, help="main_eDOS.py:55-56 evaluates at batch size 1")
    ap.add_argument("--eval-per-crystal", type=int, default=0, metavar="N",
                    help="N > 0: the batch-size-1 metrics from batched passes of N crystals (evaluate.test_per_crystal, "
                         "per-crystal keys) instead of --eval_batch_size forwards")
    ap.add_argument("--out", default="edos_best.pt")
    ap.add_argument("--no-validate", action="store_true",
                    help="skip batch validation (validate.enable: every crystal and every first-seen batch is checked for out-of-range "
                         "indices, cross-crystal edges, bad crystal-system labels and NaN / inf before a kernel reads it)")
    ap.add_argument("--per-crystal-keys", action="store_true",
                    help="train over each crystal's own atoms (and its phantom node) - what the batch-size-1 evaluation computes")
    ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="X",
                    help="clip the gradient norm to X on the device (what clip_grad_norm_ does in a torch loop); steps with a "
                         "non-finite gradient are skipped")
    ap.add_argument("--skip-nonfinite", action="store_true",
                    help="skip a step whose gradient holds a NaN / inf instead of writing it into the parameters")
    ap.add_argument("--init", default=None, metavar="CKPT",
                    help="fine-tuning: load the model from this checkpoint (checkpoint.save's file or a bare state_dict); the optimizer starts fresh")
    ap.add_argument("--train-only", nargs="+", default=None, metavar="PREFIX",
                    help="fine-tuning: train exactly the parameters whose names start with one of these prefixes, freeze the rest")
    ap.add_argument("--freeze", nargs="+", default=None, metavar="PREFIX",
                    help="fine-tuning: freeze the parameters whose names start with one of these prefixes")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY",
                    help="keep an exponential moving average of the weights inside the AdamW launch (decay in [0, 1), e.g. 0.999); every "
                         "evaluation also reports the metrics under the averaged weights, and the checkpoint carries both weight sets")
    ap.add_argument("--no-ema-warmup", action="store_true", help="with --ema: the decay from the first step on, no min(decay, (1 + t) / (10 + t))")
    ap.add_argument("--save-ema", default=None, metavar="PATH", help="with --ema: write the averaged model alone to PATH at the end of the run")
    ap.add_argument("--loss", default="reference", choices=["reference", "crystal_rmse", "mse", "mae", "huber"],
                    help="the training objective: the reference's (mean of the per-crystal RMSEs, main_eDOS.py:111-123) or the mean over "
                         "crystals of each crystal's own RMSE / MSE / MAE / Huber term (target clamped at 0 as there); on this model "
                         "crystal_rmse is the reference's objective through the per-crystal entry")
    ap.add_argument("--huber-delta", type=float, default=None, metavar="X", help="with --loss huber: torch.nn.HuberLoss's delta")
    ap.add_argument("--accumulate", type=int, default=1, metavar="K",
                    help="one optimizer step per K consecutive batches of the epoch, on the objective of their concatenation "
                         "(gradient accumulation: trainer.step_dataset_accumulate; the last window of an epoch may be shorter)")
    ap.add_argument("--balance-systems", type=float, nargs="?", const=1.0, default=None, metavar="POWER",
                    help="class-balanced sample weights over the 7 crystal systems: w ~ count[system] ** -POWER (default 1), mean 1 "
                         "over the training set (weights.balanced; Trainer(sample_weights=True)); needs a per-crystal --loss")
    ap.add_argument("--fermi-weight", default=None, metavar="CENTER,WIDTH[,FLOOR]",
                    help="energy-bin weights: a Gaussian bump of WIDTH bins around bin CENTER on a floor in [0, 1] (default 0) "
                         "(weights.fermi_window; Trainer(bin_weights=...)); needs a per-crystal --loss")
    ap.add_argument("--cdf-loss", default=None, metavar="LAM[,sq|abs[,norm]]",
                    help="LAM times the distance between the cumulative DOS curves next to the per-crystal loss - sq (default): "
                         "Cramer, abs: Wasserstein-1 (functionals.cumulative; Trainer(functionals=...)); a third part `norm` compares "
                         "the curves as shapes, each over its own total (functionals.normalised_cumulative); needs a per-crystal --loss")
    ap.add_argument("--band-centre-loss", default=None, metavar="LAM[,sq|abs]",
                    help="LAM times the (squared: sq, default; absolute: abs) error of the band centre m1 / m0 next to the per-crystal "
                         "loss, on a grid of unit length (functionals.centre); needs a per-crystal --loss.  One functional term per "
                         "run; a normalised term leaves the scale of the prediction free, the per-crystal loss carries it")
    ap.add_argument("--functional-floor", type=float, default=None, metavar="X",
                    help="floor of the denominator m0 of --band-centre-loss / --cdf-loss ...,norm (default: 1e-3 times the median m0 "
                         "of the clamped training targets, printed)")
    ap.add_argument("--report-moments", action="store_true",
                    help="with --eval-per-crystal: the mean absolute errors of the zeroth, first and second moment of the DOS and of "
                         "the band centre m1 / m0 (energies in bins from the middle of the grid), computed on the device "
                         "(functionals.moments; evaluate.functionals_per_crystal)")
    param_groups.add_arguments(ap)
    args = ap.parse_args(argv)
    for flag, norm in (("cdf_loss", True), ("band_centre_loss", False)):
        text, name = getattr(args, flag), "--" + flag.replace("_", "-")
        if text is None:
            continue
        parts = text.split(",")
        try:
            lam, kind = float(parts[0]), (parts[1] if len(parts) > 1 else "sq")
            assert len(parts) <= (3 if norm else 2) and kind in ("sq", "abs") and 0.0 <= lam < float("inf")
            assert len(parts) < 3 or parts[2] == "norm"
        except (ValueError, AssertionError):
            ap.error(f"{name} LAM[,sq|abs{'[,norm]' if norm else ''}]: a finite weight >= 0 and, optionally, the kind"
                     + (" and `norm`" if norm else ""))
        setattr(args, flag, (lam, kind, len(parts) == 3))
        if args.loss == "reference":
            ap.error(f"{name} adds a term to the per-crystal losses: pass --loss crystal_rmse (this model's reference objective "
                     "through the per-crystal entry) or another per-crystal --loss")
    if args.cdf_loss is not None and args.band_centre_loss is not None:
        ap.error("--cdf-loss and --band-centre-loss: one functional term per run (a trainer takes one table with one weight and one "
                 "kind: functionals.stack(...) in code)")
    if args.functional_floor is not None:
        if args.band_centre_loss is None and not (args.cdf_loss is not None and args.cdf_loss[2]):
            ap.error("--functional-floor belongs to --band-centre-loss or --cdf-loss LAM,KIND,norm")
        if not 0.0 < args.functional_floor < float("inf"):
            ap.error("--functional-floor X: finite and > 0")
    if args.report_moments and args.eval_per_crystal <= 0 and args.embedder == "DOSTransformer":
        ap.error("--report-moments reads the per-crystal evaluator's outputs: pass --eval-per-crystal N")
    if (args.balance_systems is not None or args.fermi_weight is not None) and args.loss == "reference":
        ap.error("--balance-systems / --fermi-weight weigh the per-crystal losses: pass --loss crystal_rmse (this model's reference "
                 "objective through the per-crystal entry) or another per-crystal --loss")
    if args.fermi_weight is not None:
        try:
            fw = [float(x) for x in args.fermi_weight.split(",")]
            assert len(fw) in (2, 3)
        except (ValueError, AssertionError):
            ap.error("--fermi-weight CENTER,WIDTH[,FLOOR]: two or three numbers")
        args.fermi_weight = fw
    if args.accumulate < 1:
        ap.error("--accumulate K: K is at least 1")
    if (args.no_ema_warmup or args.save_ema) and args.ema is None:
        ap.error("--no-ema-warmup / --save-ema need --ema DECAY")
    if (args.loss == "huber") != (args.huber_delta is not None):
        ap.error("--huber-delta X belongs to --loss huber, and --loss huber needs it")
    return args


def _functional_args(args, train, S=201):
    """--cdf-loss / --band-centre-loss -> the trainer's functionals= arguments, on a grid of unit length: bin width 1 / S.  The floor
    of a normalised term: --functional-floor, or 1e-3 times the median m0 of the clamped training targets, computed once."""
    flag = args.band_centre_loss or args.cdf_loss
    if flag is None:
        return {}
    lam, kind, norm = flag
    if args.band_centre_loss is None and not norm:
        return dict(functionals=functionals.cumulative(S, 1.0 / S), functional_weight=lam, functional_kind=kind)
    floor = args.functional_floor
    if floor is None:
        floor = 1e-3 * float((train._graph["y_ft"].double().clamp(min=0.0).sum(1) / S).median())
        print(f"--functional-floor {floor:.6g}   (1e-3 x the median m0 of the {len(train)} training targets)")
    if args.band_centre_loss is not None:
        fn = functionals.centre((torch.arange(S, dtype=torch.float64) + 0.5) / S, floor, de=1.0 / S)
    else:
        fn = functionals.normalised_cumulative(S, floor, 1.0 / S)
    return dict(functionals=fn, functional_weight=lam, functional_kind=kind)


def main(argv=None):
    """_main() with batch validation on (--no-validate: off); the process-wide switch gets its earlier setting back on the way out,
    so a caller that imports this module and runs main() is left as it was."""
    state = validate.ENABLED, validate.FINITE
    try:
        return _main(argv)
    finally:
        validate.enable(*state)


def _main(argv=None):
    args = parse_args(argv)
    dev = torch.device(f"cuda:{args.device}")
    torch.cuda.set_device(dev)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)                                    # `main_eDOS.py:20-23`
    validate.enable(not args.no_validate, finite=True)

    if args.structures:
        # structures -> graphs on the GPU; the element table stands in for the matscholar embedding (`mat2graph.py:33-47`)
        table = featurize.load_elem_feats({s: v for s, v in zip(featurize.SYMBOLS[:100],
                                                                np.random.default_rng(args.seed).normal(size=(100, 200)))})
        entries, targets = synth.edos_structures(args.structures, args.seed), None
        if args.raw_dos is not None:
            # raw spectra -> targets on the GPU; the window (-8 .. 6 eV around the Fermi level) is this example's, not the paper's
            entries = synth.raw_edos(entries, args.seed)
            targets = spectra.EdosTargets(spectra.Grid.linspace(-8.0, 6.0, synth.E_BINS), args.raw_dos)
        t0 = time.perf_counter()
        crystals = featurize.build_edos_all(entries, table, device=dev, crystal_system=args.crystal_system, symprec=args.symprec,
                                            targets=targets)
        print(f"built {len(crystals)} crystal graphs from structures in {time.perf_counter() - t0:.2f} s")
    elif args.pickle:
        crystals = pickle.load(open(args.pickle, "rb"))
    else:
        crystals = synth.edos_crystals(args.crystals, args.seed, torch.float32)
    # 8 : 1 : 1 random split (`main_eDOS.py:42-49`, sklearn's train_test_split with random_state)
    perm = np.random.default_rng(args.random_state).permutation(len(crystals))
    n_hold = max(1, len(perm) // 10)
    split = {"valid": perm[:n_hold], "test": perm[n_hold:2 * n_hold], "train": perm[2 * n_hold:]}
    ds = {k: DeviceDataset([crystals[i] for i in idx], dev) for k, idx in split.items()}
    print(f"train_dataset_len:{len(ds['train'])}\nvalid_dataset_len:{len(ds['valid'])}\ntest_dataset_len:{len(ds['test'])}")

    n_atom, n_bond = int(crystals[0]["x"].shape[1]), int(crystals[0]["edge_attr"].shape[1])
    baseline = args.embedder != "DOSTransformer"
    if args.embedder == "graphnetwork":                             # `main_eDOS.py:71-81`
        from dostransformer_amd.embedder_eDOS.graphnetwork import Graphnetwork
        model = Graphnetwork(args.layers, n_atom, n_bond, 2, args.hidden, 201, dev).to(dev)
    elif args.embedder == "mlp":
        from dostransformer_amd.embedder_eDOS.mlp import mlp
        model = mlp(args.layers, n_atom, n_bond, 2, args.hidden, 201, dev).to(dev)
    else:
        model = DOSTransformer(args.layers, args.transformer, n_atom, n_bond, 2, args.hidden, dev, args.attn_drop).to(dev)
    # fine-tuning: the model from a checkpoint (a fresh optimizer), then the frozen set - the trainer reads requires_grad
    if args.init:
        checkpoint.load(args.init, model)
    if args.train_only:
        model.train_only(*args.train_only)
    if args.freeze:
        model.freeze(*args.freeze)
    if args.train_only or args.freeze:
        names = set(model.trainable_names())
        print(f"fine-tuning: {len(names)} parameter tensors ({sum(p.numel() for k, p in model.named_parameters() if k in names)} "
              f"elements) train, the rest is frozen")
    if baseline and (args.per_crystal_keys or args.beta != 1.0):
        raise SystemExit(f"--embedder {args.embedder} has one output and no attention: --beta and --per-crystal-keys do not apply")
    # coarse shape buckets: reshuffled batches fall into a few dozen (N, E) buckets, each recorded once (ghost padding is
    # exact); every batch pads its keys to the training set's largest crystal so that n_max is not a bucket dimension
    bucket = (32, 512)
    groups = param_groups.from_args(model, args, args.lr)          # --group / --no-decay-norms / --layerwise-lr-decay (None: none)
    if groups is not None:
        for k, grp in enumerate(param_groups.resolve(model, groups, args.lr, 1e-2)):
            print(f"param group {k}: lr {grp['lr']:.3g} weight_decay {grp['weight_decay']:.3g}, {len(grp['names'])} tensors")
    if args.balance_systems is not None:                           # resident table: set once, gathered by every loss launch
        sysw = weights.balanced(ds["train"]._graph["system"].cpu(), power=args.balance_systems)
        ds["train"].set_weights(sysw)
        print(f"--balance-systems {args.balance_systems:g}: sample weights {float(sysw.min()):.3g} .. {float(sysw.max()):.3g}, mean 1")
    bin_w = None if args.fermi_weight is None else weights.fermi_window(201, *args.fermi_weight)
    trainer = Trainer(model, lr=args.lr, beta=args.beta, replay=True, bucket=bucket, promote=0.08,
                      sample_weights=args.balance_systems is not None, bin_weights=bin_w,
                      per_crystal_keys=args.per_crystal_keys,      # AdamW(lr, weight_decay=1e-2), `:91`
                      max_grad_norm=args.clip_grad_norm, skip_nonfinite=args.skip_nonfinite, param_groups=groups,
                      ema_decay=args.ema, ema_warmup=not args.no_ema_warmup,
                      loss=None if args.loss == "reference" else args.loss, huber_delta=args.huber_delta,
                      **_functional_args(args, ds["train"]))
    predictor = Predictor(model, bucket=bucket, per_crystal_keys=args.eval_per_crystal > 0 and not baseline)
    criterion_2 = torch.nn.L1Loss()                                                       # `main_eDOS.py:93`

    def run_test(name):
        """`utils.test` on a split -> (rmse, mse, mae, r2, ...): the reference's batch-size-1 numbers either way."""
        if args.eval_per_crystal > 0 or baseline:
            res = evaluate.test_per_crystal(predictor, ds[name], batch_size=args.eval_per_crystal or 64)
            if args.report_moments:                                  # from the outputs still on the device
                e = torch.arange(201, dtype=torch.float64) - 100.0
                mo = evaluate.functionals_per_crystal(res, functionals.moments(e, orders=(0, 1, 2), de=1.0))
                print(f"            {name} moments mae " + "  ".join(f"{n} {v:.4g}" for n, v in zip(mo.names + mo.ratio_names,
                                                                                                 mo.mae + mo.ratio_mae)))
            return res.as_reference()
        return evaluate.test(predictor, ds[name].batches(args.eval_batch_size), criterion_2, evaluate.r2)

    nmax_train = int(ds["train"].n_nodes.max())

    best_rmse = best_mae = 1000.0
    best_epoch, best_losses, history = 0, [], []
    test_m = (float("nan"),) * 4
    rng = np.random.default_rng(args.seed)
    for epoch in range(args.epochs):
        model.train()
        t0, losses, seen = time.perf_counter(), [], 0
        order = rng.permutation(len(ds["train"]))                                         # DataLoader(shuffle=True), `:54`
        cuts = [order[i:i + args.batch_size] for i in range(0, len(order), args.batch_size)]
        for w in range(0, len(cuts), args.accumulate):
            sels = cuts[w:w + args.accumulate]                                            # --accumulate K: the last window may be shorter
            if args.accumulate == 1:
                losses.append(trainer.step_dataset(ds["train"], sels[0], n_max=nmax_train))   # the loop body `:104-127`
            else:                                                                         # (the window's loss: a scalar the trainer owns)
                losses.append(trainer.step_dataset_accumulate(ds["train"], sels, n_max=nmax_train).clone())
            seen += sum(len(idx) for idx in sels)
        loss = float(torch.stack(losses).mean())                                          # one host read per epoch
        history.append(loss)
        print(f"[ epoch {epoch + 1}/{args.epochs} ]  Total Loss: {loss:.4f}   ({seen / (time.perf_counter() - t0):.0f} crystals/s)")
        if (epoch + 1) % min(args.eval, args.epochs):              # (a run shorter than --eval evaluates at its last epoch)
            continue
        # `main_eDOS.py:132-152`: validate; a new best in RMSE or MAE re-evaluates the test split (and, here, saves)
        v_rmse, v_mse, v_mae, v_r2, _ = run_test("valid")
        try:
            trainer.check()                                        # once per evaluation: a stalled exchange voids the epoch
        except DosxError as e:                                     # behind the gradient guard skipped steps changed nothing:
            if not trainer.guarded:                                # report them and go on
                raise
            print(f"warning: {e}")
        print(f"[ {epoch + 1} epochs ]valid_rmse:{v_rmse:.4f}|valid_mse:{v_mse:.4f}|valid_mae:{v_mae:.4f}|valid_r2:{v_r2:.4f}")
        if args.ema is not None:                                   # the same evaluator under the averaged weights: a swap launch in, one out
            with trainer.ema_weights():
                e = run_test("valid")[:4]
            print("[ {} epochs ]ema_valid_rmse:{:.4f}|ema_valid_mse:{:.4f}|ema_valid_mae:{:.4f}|ema_valid_r2:{:.4f}".format(epoch + 1, *e))
        improved = v_rmse < best_rmse or v_mae < best_mae
        if v_rmse < best_rmse:
            best_rmse = v_rmse
        if v_mae < best_mae:
            best_mae = v_mae
        if improved:
            best_epoch = epoch + 1
            test_m = run_test("test")[:4]
            print("[ {} epochs ]System:test_rmse:{:.4f}|test_mse:{:.4f}|test_mae:{:.4f}|test_r2:{:.4f}".format(epoch + 1, *test_m))
            checkpoint.save(args.out, model, trainer, extra={"epoch": epoch + 1, "valid_rmse": v_rmse, "test": list(test_m)})
            if args.ema is not None:
                with trainer.ema_weights():
                    e = run_test("test")[:4]
                print("[ {} epochs ]System:ema_test_rmse:{:.4f}|ema_test_mse:{:.4f}|ema_test_mae:{:.4f}|ema_test_r2:{:.4f}".format(epoch + 1, *e))
        best_losses.append(best_rmse)
        print("**System [Best epoch: {}] Best RMSE: {:.4f}|Best MSE: {:.4f} |Best MAE: {:.4f}|Best R2: {:.4f}**".format(best_epoch, *test_m))
        if len(best_losses) > int(args.es / args.eval) and best_losses[-1] == best_losses[-int(args.es / 5)]:   # `:166-167`
            print("Early stop!!")
            break
    if args.save_ema:                                              # the averaged model alone: checkpoint.load(PATH, plain_model) reads it
        with trainer.ema_weights():
            checkpoint.save(args.save_ema, model, extra={"ema_decay": trainer.ema_decay})
        print(f"averaged weights saved to {args.save_ema}")
    return {"best_epoch": best_epoch, "best_valid_rmse": best_rmse, "test": test_m, "train_loss": history}


if __name__ == "__main__":
    main()
