#!/usr/bin/env python3
"""Generate tests/golden/g10_baselines_{ph,gn,mlp}.npz by running the REFERENCE's GNN-only baselines through its drivers' train step.

Like make_golden.py (whose stand-ins and pack helpers it imports) this runs only where the reference is checked out
(make_golden.REF, from DOSX_REFERENCE); the reference's model files are imported unmodified by path, nothing is copied.

Three sections, one file each (together they are 1.4 MiB of incompressible parameters and gradients - more than one
committed file may hold), at the G8 sizes (3 layers, hidden 16, three crystals of 1 / 4 / 9 atoms; Electron-DOS with phantom nodes):

    ph    embedder_phDOS.graphnetwork_phonon.Graphnetwork_phonon   float64   loss sqrt(mean_all (dos - y)^2)
    gn    embedder_eDOS.graphnetwork.Graphnetwork                  float32   loss mean_b sqrt(mean_s (dos - max(y, 0))^2)
    mlp   embedder_eDOS.mlp.mlp                                    float32   (same loss)

the drivers' loss (main_phDOS.py:109-114, main_eDOS.py:111-123) on the ONE output these models have.  Each section holds the
batch (b/), the initial parameters (p0/), the output(s) (dos, and x_nodes for Graphnetwork), the loss, every gradient (g/),
dead_params (grad is None), and the parameters after 1 and 3 AdamW(lr 1e-4, weight_decay 1e-2) steps (p1/, p3/).

min_abs_pre: the smallest |E1[s] + C[b]| over the pre-activations of out_layer.0 at p0, in float64.  A LeakyReLU gate at
pre == 0 has no fp32-stable gradient, so a seed where this is below 1e-5 is refused: no gate of the fixture can flip at fp32
rounding.

    python tests/golden/make_golden_baselines.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, install_standins, np_, pack_batch, pack_sd, synth        # noqa: E402

MIN_ABS_PRE = 1e-5
N_ATOMS = [1, 4, 9]


def min_abs_pre(model, graph):
    """Smallest |E1[s] + C[b]| of out_layer.0 (float64), from the module's parameters and its decoder output ``graph`` [B,H]."""
    sd = {k: v.detach().double() for k, v in model.state_dict().items()}
    W0, H = sd["out_layer.0.weight"], graph.shape[1]
    e1 = sd["embeddings.weight"] @ W0[:, :H].T + sd["out_layer.0.bias"]
    c = graph.detach().double() @ W0[:, H:].T
    return float((e1[:, None, :] + c[None, :, :]).abs().min())


def run_section(out, pre, model, g, kind, returns_x):
    """Reference train-step body (main_phDOS.py:104-118 / main_eDOS.py:104-127) with the one-output loss, three steps."""
    grabbed = []
    hook = model.GN_decoder.register_forward_hook(lambda mod, args, res: grabbed.append(res))
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-2)
    pack_batch(out, g, pre + "b/")
    if kind == "edos":
        out[pre + "b/mp_id"] = np.array(g.mp_id)
    pack_sd(out, model.state_dict(), pre + "p0/")
    for step in (1, 2, 3):
        model.train()
        res = model(g)
        dos, xn = res if returns_x else (res, None)
        if kind == "phonon":
            loss = torch.sqrt(torch.nn.MSELoss()(dos, g.phdos).cpu()).mean()
        else:
            y_ft = torch.where(g.y_ft < 0, torch.tensor(0, dtype=torch.float), g.y_ft)
            loss = torch.sqrt(((y_ft.reshape(len(g.mp_id), -1) - dos) ** 2).mean(dim=1)).mean()
        opt.zero_grad()
        loss.backward()
        if step == 1:
            m = min_abs_pre(model, grabbed[0])
            if m < MIN_ABS_PRE:
                raise SystemExit(f"{pre}: min |pre| = {m:.3g} < {MIN_ABS_PRE}: a LeakyReLU gate could flip at fp32 rounding - "
                                 f"pick another seed")
            out[pre + "min_abs_pre"] = np.float64(m)
            out[pre + "dos"], out[pre + "loss"] = np_(dos), np_(loss)
            if xn is not None:
                out[pre + "x_nodes"] = np_(xn)
            dead = []
            for k, p in model.named_parameters():
                if p.grad is None:
                    dead.append(k)
                else:
                    out[pre + "g/" + k] = np_(p.grad)
            out[pre + "dead_params"] = np.array(dead)
        opt.step()
        if step in (1, 3):
            pack_sd(out, model.state_dict(), f"{pre}p{step}/")
    hook.remove()


def main():
    install_standins()
    sys.path.insert(0, REF)
    from embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    from embedder_eDOS.graphnetwork import Graphnetwork
    from embedder_eDOS.mlp import mlp

    dev = torch.device("cpu")
    out = {}
    torch.set_default_dtype(torch.float64)
    g = synth.phonon_batch(3, seed=10, dtype=torch.float64, sort_edges=False, n_atoms=N_ATOMS)
    torch.manual_seed(0)
    run_section(out, "ph/", Graphnetwork_phonon(3, 118, 4, 16, 51, dev), g, "phonon", False)
    torch.set_default_dtype(torch.float32)

    g = synth.edos_batch(3, seed=11, dtype=torch.float32, sort_edges=False, n_atoms=N_ATOMS)
    torch.manual_seed(0)
    run_section(out, "gn/", Graphnetwork(3, 200, 41, 2, 16, 201, dev), g, "edos", True)

    g = synth.edos_batch(3, seed=12, dtype=torch.float32, sort_edges=False, n_atoms=N_ATOMS)
    torch.manual_seed(0)
    run_section(out, "mlp/", mlp(3, 200, 41, 2, 16, 201, dev), g, "edos", False)

    for sec in ("ph", "gn", "mlp"):
        path = os.path.join(HERE, f"g10_baselines_{sec}.npz")
        np.savez_compressed(path, **{k[len(sec) + 1:]: v for k, v in out.items() if k.startswith(sec + "/")})
        print(os.path.basename(path), os.path.getsize(path) // 1024, "KiB", "min |pre|", float(out[sec + "/min_abs_pre"]))


if __name__ == "__main__":
    main()
