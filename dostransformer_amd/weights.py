"""Weights for the weighted per-crystal losses (include/dosx.h: dosx_loss_rows_w; the trainers' ``sample_weights=True`` and
``bin_weights=...``): class-balanced sample weights over the crystal systems the models are prompted with, and an energy-bin
window for the Electron-DOS model.  Pure torch on the CPU: they run once, in front of training."""
from __future__ import annotations

import torch


def balanced(systems, n_classes: int = 7, power: float = 1.0) -> torch.Tensor:
    """[C] float64 sample weights ``w_c ~ count[system_c] ** -power``, normalised to mean 1 over the given crystals - the loss
    ``sum_b w_b l_b / B`` of the weighted trainers then keeps its scale.  ``systems``: the crystals' class indices in
    ``[0, n_classes)`` (the models' ``prompt_token``: 7 crystal systems).  ``power = 1``: every class that occurs carries the same
    total weight; ``power = 0``: all ones; in between (0.5 is common) a softer balance.  Classes that do not occur are ignored."""
    s = torch.as_tensor(systems).detach().to("cpu").reshape(-1)
    if s.numel() == 0:
        raise ValueError("weights.balanced: no crystals")
    if s.is_floating_point():
        if not bool((s == s.round()).all()):
            raise ValueError("weights.balanced: systems must be integer class indices")
    s = s.to(torch.int64)
    if int(s.min()) < 0 or int(s.max()) >= int(n_classes):
        raise ValueError(f"weights.balanced: class indices must lie in [0, {int(n_classes)}), got {int(s.min())} .. {int(s.max())}")
    if not float("-inf") < float(power) < float("inf"):
        raise ValueError(f"weights.balanced: power must be finite, got {power}")
    count = torch.bincount(s, minlength=int(n_classes)).to(torch.float64)
    w = count[s] ** -float(power)               # (count[s] >= 1: only classes that occur are looked up)
    return w / w.mean()


def fermi_window(S: int, center: float, width: float, floor: float = 0.0) -> torch.Tensor:
    """[S] float64 energy-bin weights ``v_s = floor + (1 - floor) exp(-(s - center)^2 / (2 width^2))``: a Gaussian bump of height 1
    around bin ``center`` (fractional bins allowed; for the eDOS grid the Fermi level's bin) on a floor in [0, 1] - the bins that
    carry band gap and conductivity count fully, the far ones ``floor`` times as much (0: not at all).  ``width`` in bins, > 0."""
    S = int(S)
    if S < 1:
        raise ValueError(f"weights.fermi_window: S must be positive, got {S}")
    if not 0.0 < float(width) < float("inf"):
        raise ValueError(f"weights.fermi_window: width must be finite and > 0, got {width}")
    if not 0.0 <= float(floor) <= 1.0:
        raise ValueError(f"weights.fermi_window: floor must lie in [0, 1], got {floor}")
    if not float("-inf") < float(center) < float("inf"):
        raise ValueError(f"weights.fermi_window: center must be finite, got {center}")
    s = torch.arange(S, dtype=torch.float64)
    bump = torch.exp(-((s - float(center)) ** 2) / (2.0 * float(width) ** 2))
    return float(floor) + (1.0 - float(floor)) * bump
