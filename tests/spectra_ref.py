"""Case builders for the spectra tests (tests/test_spectra_host.py, tests/test_gpu_spectra.py).  The definition the kernels are
held to is the numpy twin inside the package (dostransformer_amd/spectra.py); nothing here computes a target."""
import numpy as np

from dostransformer_amd import spectra

# crystal sizes and bin counts at the edges of a wave (64), a staged tile / the lanes of a workgroup (256) and lane ownership
SIZES = (2, 63, 64, 65, 255, 256, 257, 1025)
POINT_SIZES = (0, 1) + SIZES
BINS = (1, 51, 63, 64, 65, 201, 256, 257, 1024)
FULL_BINS = (1, 201, 257)                    # the bin counts every crystal size meets; the others meet n in {2, 257}
WINDOW = (-4.0, 4.0)


def grid_of(bins: int) -> spectra.Grid:
    return spectra.Grid(WINDOW[0], 0.125, 1) if bins == 1 else spectra.Grid.linspace(WINDOW[0], WINDOW[1], bins)


def mixed_case(kind: str, bins: int, seed: int = 0):
    """One launch of mixed crystals: every size this bin count has to meet, in a shuffled order, sigma and shift different per
    crystal, some values negative, spectra that overhang the window, end inside it or (the last but one, 65 samples) lie wholly
    outside it.  Returns the keyword arguments of ``spectra.broaden`` (flat arrays plus ``ptr``) and the index of the crystal
    outside the window."""
    rng = np.random.default_rng(1000 * bins + seed + (7 if kind == "points" else 0))
    sizes = list((POINT_SIZES if kind == "points" else SIZES) if bins in FULL_BINS else ((0, 1, 2, 257) if kind == "points" else (2, 257)))
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    outside = len(sizes) - 1
    sizes.insert(outside, 65)
    es, vs, shift, sigma = [], [], [], []
    for c, n in enumerate(sizes):
        sh = float(rng.uniform(-1.0, 1.0))
        lo, hi = WINDOW[0] - rng.uniform(-1.5, 3.0), WINDOW[1] + rng.uniform(-1.5, 3.0)     # overhangs, or ends inside
        sg = float(rng.uniform(0.05, 0.6))
        if c == outside:
            lo, hi = WINDOW[1] + 6.0 * sg + 0.5, WINDOW[1] + 6.0 * sg + 3.0
        e = rng.uniform(lo, hi, n) + sh
        if kind == "curve":
            e = np.sort(e)
            assert (np.diff(e) > 0).all()
        es.append(e)
        vs.append(rng.normal(0.6, 1.0, n))
        shift.append(sh)
        sigma.append(sg)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    args = dict(energies=np.concatenate(es), values=np.concatenate(vs), ptr=ptr, grid=grid_of(bins), sigma=np.array(sigma),
                shift=np.array(shift), kind=kind, cutoff=6.0)
    return args, outside


def twin_rows(args, details: bool = True):
    """The twin on the flat arrays of ``mixed_case``: (y, y_max, area, y_norm, report, A, n_kept)."""
    ptr, e, v = spectra._flatten(args["energies"], args["values"], args["ptr"], args["kind"])
    return spectra.broaden_rows_host(ptr, e, v, np.asarray(args["shift"], np.float64), np.asarray(args["sigma"], np.float64),
                                     args["grid"], args["cutoff"], args["kind"], normalize=True, details=details)


def interp_case(bins: int, seed: int = 0):
    """Curves for ``spectra.resample``: the sizes of ``mixed_case``, plus one curve whose shifted ends sit exactly on grid points
    (the first and the last sample are hit by a bin, and bins lie outside it on both sides; bins >= 9 only)."""
    rng = np.random.default_rng(2000 * bins + seed)
    grid = grid_of(bins)
    E = grid.energies()
    sizes = list(SIZES if bins in FULL_BINS else (2, 257))
    es, vs, shift = [], [], []
    for n in sizes:
        sh = float(rng.uniform(-1.0, 1.0))
        lo, hi = WINDOW[0] - rng.uniform(-1.5, 3.0), WINDOW[1] + rng.uniform(-1.5, 3.0)
        es.append(np.sort(rng.uniform(lo, hi, n)) + sh)
        vs.append(rng.normal(0.6, 1.0, n))
        shift.append(sh)
    if bins >= 9:
        a, b = bins // 8, bins - 1 - bins // 8
        inner = np.sort(rng.uniform(E[a], E[b], 30))
        es.append(np.concatenate([[E[a]], inner, [E[b]]]))            # (shift 0: the ends are the grid's own bits)
        vs.append(rng.normal(0.6, 1.0, 32))
        shift.append(0.0)
    ptr = np.concatenate([[0], np.cumsum([e.shape[0] for e in es])])
    return dict(energies=np.concatenate(es), values=np.concatenate(vs), ptr=ptr, grid=grid, shift=np.array(shift))
