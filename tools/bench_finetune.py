#!/usr/bin/env python3
"""What freezing parameters buys back of the training step, at the cfg2 / cfg3 shapes of BASELINE.json (Phonon-DOS hidden 128
batch 64, Electron-DOS hidden 256 batch 64; 3 message-passing layers, 2 encoder layers), in ONE process:

  all  - every parameter trains: the step as it always was;
  A    - the GNN trunk frozen (model.freeze("GN_encoder", "stacked_processor", "GN_decoder")): the backward ends behind the first
         encoder (functional.trunk_cut);
  B    - only the prompt path trains (model.train_only(<prompt table>, "fc_prompt")): no backward of the first encoder either
         (functional.first_encoder_cut), and the source encoder's attention backward in its query-only form where it runs inside
         dosx_ffn_bwd (functional.attention_query_only).

All three are train.Trainer(replay=True) on the same pre-collated device-resident batches from the same initial parameters.
After a warm-up of each, rounds of `--steps` steps alternate between the three, each round timed by one device event pair; the
reported time is the median round, the spread its min .. max.  Then the dosx_ffn_bwd launch alone at the Phonon-DOS source
encoder's shape, full form against query-only.  Prints one JSON line per configuration and one for the launch.

    python tools/bench_finetune.py
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dostransformer_amd import functional as Fn, ops, synth  # noqa: E402
from dostransformer_amd.batch import collate  # noqa: E402
from dostransformer_amd.train import Trainer  # noqa: E402

CONFIGS = {"cfg2": dict(kind="phonon", hidden=128, batch=64), "cfg3": dict(kind="edos", hidden=256, batch=64)}
TRUNK = ("GN_encoder", "stacked_processor", "GN_decoder")
DEV = "cuda"


def make_model(kind, hidden):
    if kind == "phonon":
        from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
        return DOSTransformer_phonon(3, 2, 118, 4, hidden, DEV, 0.0)
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    return DOSTransformer(3, 2, 200, 41, 2, hidden, DEV, 0.0)


def recipe(model, which):
    if which == "A":
        model.freeze(*TRUNK)
    elif which == "B":
        model.train_only(model._cfg.prompt_key.rsplit(".", 1)[0], "fc_prompt")
    return model


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def run(name, steps, warmup, rounds):
    c = CONFIGS[name]
    kind, H, B = c["kind"], c["hidden"], c["batch"]
    crystals = synth.phonon_crystals(4 * B, 7, torch.float32) if kind == "phonon" else synth.edos_crystals(4 * B, 7, torch.float32)
    batches = [collate(crystals[i * B:(i + 1) * B]).to(DEV) for i in range(4)]
    torch.manual_seed(0)
    base = make_model(kind, H)
    trainers = {}
    for which in ("all", "A", "B"):
        m = make_model(kind, H)
        m.load_state_dict(base.state_dict())
        trainers[which] = Trainer(recipe(m.to(DEV), which), lr=1e-4, replay=True)
    step = {w: (lambda i, t=t: t.step(batches[i % 4])) for w, t in trainers.items()}
    for w in step:
        timed(step[w], max(warmup, 8))             # (every bucket recorded, then replayed at least once)
    ms = {w: [] for w in step}
    for _ in range(rounds):                        # alternating rounds: all see the same clocks and the same neighbours
        for w in step:
            ms[w].append(timed(step[w], steps))
    res = {"config": name, "kind": kind, "hidden": H, "batch": B}
    for w, t in trainers.items():
        st = t.program_stats()
        res[w] = {"ms_per_step": round(statistics.median(ms[w]), 4), "min_ms": round(min(ms[w]), 4), "max_ms": round(max(ms[w]), 4),
                  "launches": st["launches"], "wgrad_jobs": st["wgrad_jobs"],
                  "trainable_floats": t._fp.n_train, "floats": t._fp.total}
    for w in ("A", "B"):
        res[w]["vs_all"] = round(res[w]["ms_per_step"] / res["all"]["ms_per_step"], 4)
    print(json.dumps(res), flush=True)
    return res


def ffn_bwd_alone(steps, warmup, H=128, Sq=51, Bq=128, Bk=64, Nk=12):
    """The dosx_ffn_bwd launch of one source-encoder layer (cfg2: 51 energies x 2 x 64 rows, <= Nk atoms per crystal), recorded
    and replayed alone: full form (key gradient, ticket, last-arriver reduction) against query-only."""
    out = {"launch": "ffn_bwd", "H": H, "Sq": Sq, "Bq": Bq, "Bk": Bk, "Nk": Nk,
           "in_ffn": bool(Fn.attention_bwd_in_ffn(Sq, Bq, Nk, H, False))}
    if not ops.ffn_att_bwd_supported(H, Nk, Sq, Bq):
        print(json.dumps(out), flush=True)
        return out
    dev = torch.device(DEV, torch.cuda.current_device())
    gen = torch.Generator().manual_seed(1)
    lp = "e.layers.0"
    P = {}
    for k, shp, sc in ((".layer_norms.0.weight", (H,), 0.2), (".layer_norms.0.bias", (H,), 0.3), (".layer_norms.1.weight", (H,), 0.2),
                       (".layer_norms.1.bias", (H,), 0.3), (".fc1.weight", (4 * H, H), H ** -0.5), (".fc1.bias", (4 * H,), 0.1),
                       (".fc2.weight", (H, 4 * H), (4 * H) ** -0.5), (".fc2.bias", (H,), 0.1)):
        P[lp + k] = (torch.randn(*shp, generator=gen) * sc + (1.0 if "norms" in k and k.endswith("weight") else 0.0)).to(dev)
    P = Fn.pack_params(P)
    rows = Sq * Bq
    x, kvhat = torch.randn(rows, H, generator=gen).to(dev), torch.randn(Nk * Bk, H, generator=gen).to(dev)
    with torch.no_grad():
        _, ctx = Fn.encoder_fwd(P, "e", x, Sq, Bq, Bq, 1, kvhat, Nk, Bk, H, 1, final_ln=False)
    lay = ctx.layers[0]
    nq = ops.ffn_att_bwd_partial_rows(Sq, Bq)
    part_a = torch.zeros(nq + Bk * ((Nk + 15) // 16), 2 * H, device=dev)
    dxin, dh, dy = torch.zeros(rows, H, device=dev), torch.zeros(rows, 4 * H, device=dev), torch.randn(rows, H, generator=gen).to(dev)
    part, kvp, dkv = torch.zeros(nq, 2 * H, device=dev), torch.zeros(nq * Nk, H, device=dev), torch.zeros(Nk * Bk, H, device=dev)
    common = dict(x=lay.x, kvhat=kvhat, gamma0=P[lp + ".layer_norms.0.weight"], beta0=P[lp + ".layer_norms.0.bias"], probs=lay.probs,
                  qstats=lay.qstats, mask=None, dxin=dxin, partials_q=part_a.data_ptr(), Nk=Nk, Bk=Bk, Bq=Bq, Sq=Sq, qs=lay.qs, qb=lay.qb)
    forms = {"full": ops.AttBwd(partials_kv=part_a.data_ptr() + 4 * nq * 2 * H, dkv_part=kvp, dkv_cnt=ops.COUNTERS.take(dev, Bk),
                                dkvhat=dkv, accumulate=0, **common),
             "query_only": ops.AttBwd(partials_kv=None, dkv_part=None, dkv_cnt=None, dkvhat=None, accumulate=0, **common)}
    progs = {}
    for name, att in forms.items():
        with ops.recording_scope(), torch.no_grad():
            ops.RECORDER.begin()
            ops.ffn_bwd(rows, H, dy, lay.h, lay.x1, lay.st1, P[lp + ".layer_norms.1.weight"], P[lp + ".fc1.weight"],
                        P[lp + ".fc2.weight"], dh, None, part, att=att)
            progs[name] = ops.RECORDER.end()
        timed(lambda _: progs[name].run(), warmup)
    us = {name: [] for name in progs}
    for _ in range(5):
        for name, prog in progs.items():
            us[name].append(1e3 * timed(lambda _: prog.run(), steps))
    for name in progs:
        out[name + "_us"] = round(statistics.median(us[name]), 2)
        out[name + "_us_min_max"] = [round(min(us[name]), 2), round(max(us[name]), 2)]
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cfg2", "cfg3"], choices=list(CONFIGS))
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    res = [run(n, args.steps, args.warmup, args.rounds) for n in args.configs]
    res.append(ffn_bwd_alone(max(args.steps, 100), args.warmup))
    return res


if __name__ == "__main__":
    main()
