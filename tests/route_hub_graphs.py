"""Edge lists shared by test_route_hub_plan_cpu.py and test_gpu_route_hub.py (numpy int64 src / dst, symmetrised by
Graph.from_edge_rows), and the independent recount of what a routing hub plan gathers."""
import numpy as np


def hub_clique_70():
    """70 nodes: four hubs (0..3) joined to most of 4..59, a clique on 10..17, self-loops, 60..69 isolated."""
    src, dst = [], []
    for h in range(4):
        for v in range(4, 60):
            if (v + h) % (h + 1) == 0 or v % 4 == h:
                src.append(h), dst.append(v)
    for a in range(10, 18):
        for b in range(a + 1, 18):
            src.append(a), dst.append(b)
    for v in (0, 5, 12, 20, 59):
        src.append(v), dst.append(v)
    src += [0, 1, 2]
    dst += [1, 2, 3]
    return np.array(src), np.array(dst), 70


def power_law_300():
    """300 nodes, three edges per new node towards low ids (a skewed degree sequence), a few self-loops."""
    rng = np.random.default_rng(300)
    v = np.repeat(np.arange(1, 300), 3)
    u = np.floor(v * rng.random(v.size) ** 2.5).astype(np.int64)
    loops = np.array([0, 7, 150, 299])
    return np.concatenate([v, loops]), np.concatenate([u, loops]), 300


def n17():
    """17 nodes that all own an entry (a self-loop each): the second block of 16 rows holds one row."""
    i = np.arange(17)
    return np.concatenate([i, i, i]), np.concatenate([i, (i + 1) % 17, (i * 5 + 3) % 17]), 17


def lattice_4096():
    """Degree-4 ring lattice on 4,096 nodes, strides 1 and 64: no two of 16 consecutive rows share a neighbour they own.
    (With strides 1 and 2 the rows i and i + 1 both own an edge to i + 2: the first block shares 1.84 entries per
    gathered row and the automatic rule gives it a plan.)"""
    i = np.arange(4096)
    return np.concatenate([i, i]), np.concatenate([(i + 1) % 4096, (i + 64) % 4096]), 4096


SMALL = {"hub_clique_70": hub_clique_70, "power_law_300": power_law_300, "n17": n17}


def engineered(nA, nB, nC):
    """16 hub rows (0..15) and partners from node 16 up: nA partners joined to one hub each (slots of A steps), nB to the
    hubs (2i, 2i + 1) mod 16 (halves of B steps), nC to the hubs 4i .. 4i + 3 mod 16 (C steps) — the lists of
    test_gpu_score_hub_tail.py as a graph.  Every hub has a larger degree than any partner (<= 4), so the hubs own every
    edge: one block, and with one work item the step lists are (ceil(nA / 4), ceil(nB / 2), nC) long.  A path over the
    hubs keeps their degrees apart from the partners' where a list is short."""
    src, dst, v = [], [], 16
    for i in range(nA):
        src.append(i % 16), dst.append(v)
        v += 1
    for i in range(nB):
        src += [(2 * i) % 16, (2 * i + 1) % 16]
        dst += [v, v]
        v += 1
    for i in range(nC):
        src += [(4 * i + j) % 16 for j in range(4)]
        dst += [v] * 4
        v += 1
    return np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64), v


def csr_arrays(g):
    """(row, col, rev) of every directed entry of a Graph, as numpy int64."""
    ptr = g.rowptr.cpu().numpy().astype(np.int64)
    row = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    return row, g.col.cpu().numpy().astype(np.int64), g.rev.cpu().numpy().astype(np.int64)


def recount_gathered(g):
    """Partner rows a routing hub plan over every owner row gathers, recounted with numpy alone: owners ranked by the
    entries they own (ties by id), blocks of 16, and per (block, partner) with c entries c // 4 rows for C steps, one for a
    rest of 2 or 3 (half a B step), one for a rest of 1 or 3 (a slot of an A step)."""
    row, col, _ = csr_arrays(g)
    n = g.n_nodes
    deg = np.bincount(row, minlength=n)
    up = col >= row
    r, c = row[up], col[up]
    swap = deg[c] > deg[r]
    owner, partner = np.where(swap, c, r), np.where(swap, r, c)
    owned = np.bincount(owner, minlength=n)
    order = np.argsort(-owned, kind="stable")
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    _, cnt = np.unique((rank[owner] // 16) * n + partner, return_counts=True)
    return int((cnt // 4 + (cnt % 4 >= 2) + (cnt % 2 == 1)).sum())
