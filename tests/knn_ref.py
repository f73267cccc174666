"""Brute-force numpy restatement of dosx_knn_graph (include/dosx.h: DosxKnn), one crystal at a time - a helper, not a test.

The reference is `data/mat2graph.py:120-243`: pymatgen's ``get_all_neighbors(radius)`` sorted by distance, cut at
``max_num_nbr``, padded with (index 0, radius + 1) and Gaussian-expanded.  pymatgen is neither in the reference tree nor pinned,
so this file restates its documented behaviour (PARITY UNPINNED at that boundary) and fixes what the reference leaves open:
the order inside a distance tie is (r2, j, S0, S1, S2) ascending.  Candidates come from the oracle's brute-force neighbour
list, so the difference vectors carry the reference's summation order."""
import numpy as np

from oracle.dos_oracle import neighbor_list_bruteforce


def knn_reference(pos, cell, radius=8.0, k=12, tol=1e-8, step=0.2, pbc=(True, True, True)):
    """Returns a dict: nbr_idx [n,k] int32, nbr_shift [n,k,3] int32, nbr_dist [n,k] float64, nbr_count [n] int32 (kept before
    padding), n_cand [n] (images inside the radius before the cut), edge_attr [n*k, G] float32."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    n = pos.shape[0]
    i, j, S, D = neighbor_list_bruteforce(pos, cell, radius * (1 + 1e-9) + 1e-9, False)
    r2 = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
    keep = (r2 > tol * tol) & (r2 <= radius * radius)
    for a in range(3):
        if not pbc[a]:
            keep &= S[:, a] == 0
    i, j, S, r2 = i[keep], j[keep], S[keep], r2[keep]
    idx = np.zeros((n, k), np.int32)
    shift = np.zeros((n, k, 3), np.int32)
    dist = np.full((n, k), radius + 1.0)
    count = np.zeros(n, np.int32)
    n_cand = np.zeros(n, np.int64)
    for a in range(n):
        m = np.nonzero(i == a)[0]
        n_cand[a] = m.size
        order = m[np.lexsort((S[m, 2], S[m, 1], S[m, 0], j[m], r2[m]))][:k]
        c = order.size
        count[a] = c
        idx[a, :c], shift[a, :c], dist[a, :c] = j[order], S[order], np.sqrt(r2[order])
    centers = np.arange(0.0, radius + step, step)
    attr = np.exp(-(dist.reshape(-1)[:, None] - centers) ** 2 / step ** 2).astype(np.float32)
    return {"nbr_idx": idx, "nbr_shift": shift, "nbr_dist": dist, "nbr_count": count, "n_cand": n_cand, "edge_attr": attr}
