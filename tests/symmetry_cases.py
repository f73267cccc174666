"""Known answers for the crystal-system derivation (dostransformer_amd/symmetry.py, csrc/symmetry.hip) - a helper, not a test.

CASES: name -> (entry, expected system code, expected number of structure operations), every crystal built in code from its
textbook description.  The transforms below must not change the answer: a rigid rotation, a unimodular change of basis, an origin
shift, a permutation of the atoms (``disguise`` applies all four) and a supercell."""
import numpy as np

CUBIC, HEXAGONAL, TETRAGONAL, TRIGONAL, ORTHORHOMBIC, MONOCLINIC, TRICLINIC, INCONSISTENT = range(8)


def entry(cell, frac, numbers, name):
    cell = np.asarray(cell, np.float64)
    return {"cell": cell, "positions": np.asarray(frac, np.float64).reshape(-1, 3) @ cell, "numbers": np.asarray(numbers, np.int64),
            "mp_id": name}


def cell_from_parameters(a, b, c, alpha, beta, gamma):
    al, be, ga = np.radians([alpha, beta, gamma])
    cx = c * np.cos(be)
    cy = c * (np.cos(al) - np.cos(be) * np.cos(ga)) / np.sin(ga)
    return np.array([[a, 0, 0], [b * np.cos(ga), b * np.sin(ga), 0], [cx, cy, np.sqrt(c * c - cx * cx - cy * cy)]])


def _hex(a, c):
    return np.array([[a, 0, 0], [-a / 2, a * np.sqrt(3) / 2, 0], [0, 0, c]])


def _rhombohedral(a, alpha):
    co = np.cos(np.radians(alpha))
    s, d = np.sqrt(1 + 2 * co), np.sqrt(1 - co)
    q = (s - d) / 3
    p = q + d
    return a * np.array([[p, q, q], [q, p, q], [q, q, p]])


def _quartz():
    """alpha-quartz from the six operations of P3_2 21 on Si (0.4697, 0, 2/3) and O (0.4135, 0.2669, 0.1191)."""
    ops = (lambda x, y, z: (x, y, z), lambda x, y, z: (-y, x - y, z + 2 / 3), lambda x, y, z: (-x + y, -x, z + 1 / 3),
           lambda x, y, z: (y, x, -z), lambda x, y, z: (x - y, -y, -z + 1 / 3), lambda x, y, z: (-x, -x + y, -z + 2 / 3))
    frac, numbers = [], []
    for z_at, site in ((14, (0.4697, 0.0, 2 / 3)), (8, (0.4135, 0.2669, 0.1191))):
        orbit = []
        for op in ops:
            p = np.mod(np.array(op(*site)), 1.0)
            if not any(np.abs((p - q) - np.rint(p - q)).max() < 1e-6 for q in orbit):
                orbit.append(p)
        frac += orbit
        numbers += [z_at] * len(orbit)
    assert numbers.count(14) == 3 and numbers.count(8) == 6
    return entry(_hex(4.916, 5.4054), frac, numbers, "alpha-quartz")


def _cases():
    fcc = lambda a: a / 2 * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0.0]])
    bcc = lambda a: a / 2 * np.array([[-1, 1, 1], [1, -1, 1], [1, 1, -1.0]])
    cub = lambda a: a * np.eye(3)
    u = 0.305
    return {
        "sc": (entry(cub(3.0), [[0, 0, 0]], [84], "sc"), CUBIC, 48),
        "fcc primitive": (entry(fcc(4.05), [[0, 0, 0]], [13], "fcc primitive"), CUBIC, 48),
        "bcc primitive": (entry(bcc(2.87), [[0, 0, 0]], [26], "bcc primitive"), CUBIC, 48),
        "conventional fcc": (entry(cub(4.05), [[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]], [13] * 4, "conventional fcc"), CUBIC, 48),
        "conventional bcc": (entry(cub(2.87), [[0, 0, 0], [.5, .5, .5]], [26] * 2, "conventional bcc"), CUBIC, 48),
        "diamond": (entry(fcc(5.43), [[0, 0, 0], [.25, .25, .25]], [14, 14], "diamond"), CUBIC, 48),
        "zincblende": (entry(fcc(5.41), [[0, 0, 0], [.25, .25, .25]], [30, 16], "zincblende"), CUBIC, 24),
        "CsCl": (entry(cub(4.12), [[0, 0, 0], [.5, .5, .5]], [55, 17], "CsCl"), CUBIC, 48),
        "hcp": (entry(_hex(3.21, 5.21), [[1 / 3, 2 / 3, .25], [2 / 3, 1 / 3, .75]], [12, 12], "hcp"), HEXAGONAL, 24),
        "wurtzite": (entry(_hex(3.82, 6.26), [[1 / 3, 2 / 3, 0], [2 / 3, 1 / 3, .5], [1 / 3, 2 / 3, .375], [2 / 3, 1 / 3, .875]],
                           [30, 30, 16, 16], "wurtzite"), HEXAGONAL, 12),
        "rutile": (entry(np.diag([4.59, 4.59, 2.96]), [[0, 0, 0], [.5, .5, .5], [u, u, 0], [-u, -u, 0], [.5 + u, .5 - u, .5],
                                                      [.5 - u, .5 + u, .5]], [22, 22, 8, 8, 8, 8], "rutile"), TETRAGONAL, 16),
        "alpha-quartz": (_quartz(), TRIGONAL, 6),
        "rhombohedral": (entry(_rhombohedral(4.0, 75.0), [[0, 0, 0]], [83], "rhombohedral"), TRIGONAL, 12),
        "orthorhombic": (entry(np.diag([3.0, 4.0, 5.0]), [[0, 0, 0], [.5, .5, .3]], [11, 17], "orthorhombic"), ORTHORHOMBIC, 4),
        "monoclinic": (entry(cell_from_parameters(5.0, 6.0, 7.0, 90, 100, 90), [[0, 0, 0], [.2, .3, .15], [-.2, .3, -.15]],
                             [20, 8, 8], "monoclinic"), MONOCLINIC, 2),
        "triclinic, inversion": (entry(cell_from_parameters(4.0, 5.0, 6.0, 80, 85, 95), [[0, 0, 0], [.2, .3, .15], [-.2, -.3, -.15]],
                                       [20, 8, 8], "triclinic, inversion"), TRICLINIC, 2),
        "triclinic": (entry(cell_from_parameters(4.0, 5.0, 6.0, 80, 85, 95), [[0, 0, 0], [.2, .3, .15], [.6, .1, .7]],
                            [20, 8, 9], "triclinic"), TRICLINIC, 1),
        "cubic metric, tetragonal decoration": (entry(cub(4.0), [[0, 0, 0], [.5, .5, .5], [0, 0, .3], [0, 0, .7]], [11, 12, 9, 9],
                                                      "cubic metric, tetragonal decoration"), TETRAGONAL, 16),
    }


CASES = _cases()
SUPERCELLS = ((2, 1, 1), (1, 3, 1), (2, 2, 1))
CENTRED = {"conventional fcc": 4, "conventional bcc": 2}


def rotate(e, rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return dict(e, cell=e["cell"] @ q, positions=e["positions"] @ q)


def rebase(e, rng):
    """A random unimodular change of basis with entries in -2..2 (same lattice, same Cartesian atoms)."""
    while True:
        m = rng.integers(-2, 3, size=(3, 3))
        if abs(round(np.linalg.det(m))) == 1:
            return dict(e, cell=m.astype(np.float64) @ e["cell"])


def shift(e, rng):
    return dict(e, positions=e["positions"] + rng.uniform(-3, 3, 3))


def permute(e, rng):
    p = rng.permutation(len(e["numbers"]))
    return dict(e, positions=e["positions"][p], numbers=e["numbers"][p])


def disguise(e, seed):
    rng = np.random.default_rng(seed)
    return permute(shift(rebase(rotate(e, rng), rng), rng), rng)


def supercell(e, reps):
    reps = np.asarray(reps)
    grid = np.stack(np.meshgrid(*[np.arange(r) for r in reps], indexing="ij"), -1).reshape(-1, 3)
    pos = (e["positions"][None, :, :] + (grid.astype(np.float64) @ e["cell"])[:, None, :]).reshape(-1, 3)
    return dict(e, cell=e["cell"] * reps[:, None], positions=pos, numbers=np.tile(e["numbers"], len(grid)))


def displaced(e, atom, vector):
    pos = e["positions"].copy()
    pos[atom] += np.asarray(vector, np.float64)
    return dict(e, positions=pos)


def all_forms(seed=0):
    """[(label, entry, code, n_ops, n_translations)]: every case as listed, disguised, and as each supercell, disguised."""
    out = []
    for k, (name, (e, code, n_ops)) in enumerate(CASES.items()):
        cells = CENTRED.get(name, 1)                       # primitive cells in the case as listed
        out.append((name, e, code, n_ops, cells - 1))
        out.append((name + " / disguised", disguise(e, seed + 100 * k), code, n_ops, cells - 1))
        for r, reps in enumerate(SUPERCELLS):
            out.append((f"{name} / {reps} disguised", disguise(supercell(e, reps), seed + 100 * k + r + 1), code, n_ops,
                        cells * int(np.prod(reps)) - 1))
    return out
