#!/usr/bin/env python3
"""Training-step time of the GNN-only baselines at the cfg2 / cfg3 shapes of BASELINE.json (Phonon-DOS hidden 128 batch 64,
Electron-DOS hidden 256 batch 64; 3 message-passing layers), two ways in ONE process:

  (a) the autograd step: model(batch), the driver's loss in torch ops, loss.backward(), torch.optim.AdamW - how a baseline was
      trained before train.Trainer took these modules;
  (b) train.Trainer(replay=True): forward program, loss kernel, backward program with the output head on its rank structure
      (csrc/pair_head.hip), flat AdamW kernel - a recorded launch list per shape bucket.

Both run on the same pre-collated device-resident batches from the same initial parameters.  After a warm-up of each, rounds of
`--steps` steps alternate between the two, each round timed by one device event pair; the reported time is the median round.
Then the output head's launches alone (forward + backward + gradient flush on a stand-alone [B, H] decoder output), un-factored
and factored.  Prints one JSON line per configuration.

    python tools/bench_baselines.py --embedder graphnetwork
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
DEV = "cuda"


def make_model(kind, embedder, hidden):
    if kind == "phonon":
        from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
        return Graphnetwork_phonon(3, 118, 4, hidden, 51, DEV)
    if embedder == "mlp":
        from dostransformer_amd.embedder_eDOS.mlp import mlp
        return mlp(3, 200, 41, 2, hidden, 201, DEV)
    from dostransformer_amd.embedder_eDOS.graphnetwork import Graphnetwork
    return Graphnetwork(3, 200, 41, 2, hidden, 201, DEV)


def autograd_step(model, opt, g, kind):
    """`main_phDOS.py:104-118` / `main_eDOS.py:104-127` with the one output of these models."""
    out = model(g)
    dos = out[0] if isinstance(out, tuple) else out
    if kind == "phonon":
        loss = torch.sqrt(torch.nn.functional.mse_loss(dos, g.phdos.reshape(dos.shape)))
    else:
        y = torch.clamp(g.y_ft, min=0.0).reshape(dos.shape)
        loss = torch.sqrt(((y - dos) ** 2).mean(dim=1)).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def head_alone(model, B, factored, steps, warmup):
    """(ms, launches) per forward + backward + gradient flush of the output head alone on a random decoder output [B, H]."""
    fp, cfg = model.flat_params(), model._cfg
    graph = torch.randn(B, cfg.H, device=DEV)
    ddos = torch.randn(B, cfg.S, device=DEV)

    def once(_):
        with torch.no_grad():
            dos, a, hid = Fn._pair_head_fwd(fp.P, cfg, B, graph, factored)
            sink = ops.GradSink(torch.device(DEV))
            Fn._pair_head_bwd(fp.P, fp.G, cfg, B, a, hid, ddos, sink)
            sink.flush()
            sink.release()

    # recorded once and replayed (one C loop over the launch list): device time, not the host's cost of issuing from Python
    with ops.recording_scope(), torch.no_grad():
        ops.RECORDER.begin()
        once(0)
        prog = ops.RECORDER.end()
    timed(lambda _: prog.run(), warmup)
    return statistics.median(timed(lambda _: prog.run(), steps) for _ in range(5)), len(prog)


def run(name, embedder, steps, warmup, rounds):
    c = CONFIGS[name]
    kind, H, B = c["kind"], c["hidden"], c["batch"]
    crystals = synth.phonon_crystals(4 * B, 7, torch.float32) if kind == "phonon" else synth.edos_crystals(4 * B, 7, torch.float32)
    batches = [collate(crystals[i * B:(i + 1) * B]).to(DEV) for i in range(4)]
    torch.manual_seed(0)
    m_a = make_model(kind, embedder, H)
    m_b = make_model(kind, embedder, H)
    m_b.load_state_dict(m_a.state_dict())
    m_a, m_b = m_a.to(DEV), m_b.to(DEV)
    opt = torch.optim.AdamW(m_a.parameters(), lr=1e-4, weight_decay=1e-2)
    tr = Trainer(m_b, lr=1e-4, replay=True)
    step_a = lambda i: autograd_step(m_a, opt, batches[i % 4], kind)
    step_b = lambda i: tr.step(batches[i % 4])
    timed(step_a, warmup)
    timed(step_b, max(warmup, 8))                  # (every bucket recorded, then replayed at least once)
    ta, tb = [], []
    for _ in range(rounds):                        # alternating rounds: both see the same clocks and the same neighbours
        ta.append(timed(step_a, steps))
        tb.append(timed(step_b, steps))
    a, b = statistics.median(ta), statistics.median(tb)
    res = {"config": name, "embedder": embedder if kind == "edos" else "graphnetwork", "kind": kind, "hidden": H, "batch": B,
           "autograd_ms_per_step": round(a, 4), "autograd_crystals_per_s": round(B / a * 1e3, 1),
           "trainer_replay_ms_per_step": round(b, 4), "trainer_replay_crystals_per_s": round(B / b * 1e3, 1),
           "rounds_ms": {"autograd": [round(t, 4) for t in ta], "trainer_replay": [round(t, 4) for t in tb]},
           }
    for key, factored in (("head_unfactored", False), ("head_factored", True)):
        ms, launches = head_alone(m_b, B, factored, steps, warmup)
        res[key + "_ms"], res[key + "_launches"] = round(ms, 4), launches
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--embedder", default="graphnetwork", choices=["graphnetwork", "mlp"])
    ap.add_argument("--configs", nargs="+", default=["cfg2", "cfg3"], choices=list(CONFIGS))
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    return [run(n, args.embedder, args.steps, args.warmup, args.rounds) for n in args.configs]


if __name__ == "__main__":
    main()
