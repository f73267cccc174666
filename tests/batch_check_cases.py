"""The small batch and its single-rule corruptions shared by tests/test_batch_check_host.py (the numpy twin against expectations
worked out by hand) and tests/test_gpu_batch_check.py (dosx_batch_check against the twin, word for word).

The batch: 3 crystals of 2, 1 and 3 atoms, 7 edges sorted by destination - a self edge on every atom plus 4 -> 3 inside the last
crystal (self edges stay inside their crystal whatever `batch` says, so a corrupted batch vector does not light up R2 by itself):

    node    0 1 | 2 | 3 4 5          edge   e0    e1    e2    e3    e4    e5    e6
    batch   0 0 | 1 | 2 2 2          s->d   0->0  1->1  2->2  3->3  4->3  4->4  5->5          system 0 3 6
"""
import numpy as np

INT32_MAX = 2 ** 31 - 1
N_RULES = 7


def small_batch(sizes=(2, 1, 3)):
    """dict(edge_index [2,E] int64, batch [N] int64, system [B] int64, num_graphs) - every atom a self edge, plus second -> first
    atom of the largest crystal."""
    sizes = list(sizes)
    start = np.concatenate([[0], np.cumsum(sizes)])
    batch = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    big = int(np.argmax(sizes))
    edges = [(n, n) for n in range(int(start[-1]))] + [(int(start[big]) + 1, int(start[big]))]
    edges.sort(key=lambda e: (e[1], e[0]))
    return {"edge_index": np.asarray(edges, np.int64).T.copy(), "batch": batch,
            "system": np.asarray([0, 3, 6][:len(sizes)], np.int64), "num_graphs": len(sizes)}


def _set(key, *assignments):
    def f(b):
        for idx, val in assignments:
            b[key][idx] = val
    return f


def _swap_edges(*pairs):
    def f(b):
        for i, j in pairs:
            b["edge_index"][:, [i, j]] = b["edge_index"][:, [j, i]]
    return f


def _whole_batch(values):
    def f(b):
        b["batch"][:] = values
    return f


def _five_crystals(b):
    b["num_graphs"], b["system"] = 5, None


# (name, mutation of a small_batch() copy, keyword arguments of the check, {rule: (count, first)} expected - by hand, see the table
#  in the module docstring; every rule once at the first element it can apply to, once at the last, once twice)
CASES = [
    ("clean", lambda b: None, {}, {}),
    ("clean-sorted-nmax", lambda b: None, {"require_sorted": True, "n_max": 3}, {}),
    ("unsorted-but-not-required", _swap_edges((0, 1)), {}, {}),
    ("R1-first", _set("edge_index", ((0, 0), -1)), {}, {1: (1, 0)}),
    ("R1-last", _set("edge_index", ((1, 6), 6)), {}, {1: (1, 6)}),
    ("R1-twice", _set("edge_index", ((0, 2), 6), ((0, 5), 2 ** 40)), {}, {1: (2, 2)}),
    # e4 = 0 -> 6: its source sits in another crystal than node 3 did, but the destination fails R1 first: no R2 for this edge
    ("R1-shadows-R2", _set("edge_index", ((0, 4), 0), ((1, 4), 6)), {}, {1: (1, 4)}),
    ("R2-first", _set("edge_index", ((0, 0), 2)), {}, {2: (1, 0)}),
    ("R2-last", _set("edge_index", ((0, 6), 0)), {}, {2: (1, 6)}),
    ("R2-twice", _set("edge_index", ((0, 1), 3), ((0, 5), 1)), {}, {2: (2, 1)}),
    ("R3-first", _set("batch", (0, -1)), {}, {3: (1, 0)}),                         # (node 1 still gives crystal 0 an atom)
    ("R3-last", _set("batch", (5, 3)), {}, {3: (1, 5)}),
    # batch 0 0 1 0 2 1: nodes 3 and 5 step down; edge e4 = 4 -> 3 now joins crystals 2 and 0
    ("R3-twice", _set("batch", (3, 0), (5, 1)), {}, {3: (2, 3), 2: (1, 4)}),
    ("R4-first", _whole_batch([1, 1, 1, 2, 2, 2]), {}, {3: (1, 0), 4: (1, 0)}),    # (batch[0] != 0 is R3 as well)
    ("R4-last", _whole_batch([0, 0, 1, 1, 1, 1]), {}, {4: (1, 2)}),
    ("R4-twice", _five_crystals, {}, {4: (2, 3)}),
    ("R5-first", _set("system", (0, 7)), {}, {5: (1, 0)}),
    ("R5-last", _set("system", (2, -1)), {}, {5: (1, 2)}),
    ("R5-twice", _set("system", (1, 7), (2, 2 ** 40)), {}, {5: (2, 1)}),
    ("R6-last", lambda b: None, {"n_max": 2}, {6: (1, 2)}),
    ("R6-twice", lambda b: None, {"n_max": 1}, {6: (2, 0)}),
    ("R7-first", _swap_edges((0, 1)), {"require_sorted": True}, {7: (1, 1)}),
    ("R7-last", _swap_edges((5, 6)), {"require_sorted": True}, {7: (1, 6)}),
    ("R7-twice", _swap_edges((0, 1), (5, 6)), {"require_sorted": True}, {7: (2, 1)}),
]
# R6 at the first crystal alone needs other sizes: 3, 1, 2 atoms with n_max = 2
CASE_R6_FIRST = ((3, 1, 2), {"n_max": 2}, {6: (1, 0)})


def corrupted(name):
    """(batch dict, check kwargs, expected) of one case."""
    for n, mutate, kw, want in CASES:
        if n == name:
            b = small_batch()
            mutate(b)
            return b, kw, want
    raise KeyError(name)


def expected_words(want):
    w = np.zeros(2 * N_RULES, np.int32)
    w[1::2] = INT32_MAX
    for rule, (count, first) in want.items():
        w[2 * (rule - 1):2 * rule] = (count, first)
    return w
