"""Inputs and the brute force of the cloud-search edge tests (tests/test_cloud_edges_host.py: the host twins,
tests/test_cloud_edges_gpu.py: the device path).  The searches of csrc/cloud_knn.hip and csrc/cloud_dist.hip branch on the size of
a work item: its queries take P lanes (the next power of two) and the lanes split into S = LANES / P slices, a sweep steps by
slices, the candidates pass in tiles of LANES, an item of more than LANES queries takes two passes.  The sweep here puts a
cluster at every such edge.

Every coordinate is a multiple of 1/16, the search runs at c = R = D = 1 with the lattice origin (0, 0, 0): every cell centre is a
multiple of 1/2, every centre-relative coordinate a multiple of 1/16 below 2, and every fp32 operation of the pair arithmetic is
exact.  So there is no tolerance and no query is set aside: d2, index and count equal the fp64 brute force bit for bit under the
total order (d2, then the lower number), and the exact ties such a grid is full of go through the merges.

A cluster is c points of one cell (drawn without replacement from its 4096 grid positions) and max(t - c, 0) points dealt round
robin over the neighbour cells that exist, so that a query of the cell has t candidates (itself included); for the nearest-target
search c queries of the cell and t targets dealt over all 27 cells.  Clusters stand 4 cells apart, so none sees another, and the
brute force works cluster by cluster: all pairs in fp64, no lattice, nothing of the project's search code."""
import numpy as np

from ada_mvs_amd import _lib
import accuracy_inputs as I

KS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32)        # 7 | 8, 15 | 16 | 17 and 31 | 32: the last slot of a class of k and the first of the next
K_REF = 33                                      # the brute force keeps one place more than the largest k: a tie at the 32nd place shows
# queries per cluster: around every power of two (P full, and the first count of the next P), two items, three items
COUNTS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
ORIGIN = (0.0, 0.0, 0.0)
R = 1.0
GRID = 16                                       # positions per axis of a cell
SPACING = 4                                     # cells between two clusters along x
# (cell, c, t) at the lattice's borders: the first cell of all axes, the last of all axes, first on x and last on y
BORDERS = (((0.0, 0.0, 0.0), 9, 300), ((I.LAST, I.LAST, I.LAST), 65, 257), ((0.0, I.LAST, 10.0), 3, 513))
CHUNK_CASES = ((1, 1), (1, 300), (3, 300), (257, 600), (513, 800))      # the small cloud of the chunk tests: about 2 k points, one alone
CHUNKS = (1, 255, 256, 257, 512)


def lanes_of(k):
    """Lanes of the workgroup that searches with k (launch_knn_search: the tile's width, half of it for k > 16)."""
    return _lib.CLOUD_TILE if k <= 16 else _lib.CLOUD_TILE // 2


LANES = (lanes_of(1), lanes_of(_lib.KNN_MAX_K))


def slices(count, L):
    """-> (P, S): the lanes `count` queries take and the slices the L lanes split into."""
    P = 1
    while P < count:
        P <<= 1
    return P, L // P


def totals(c, L):
    """Candidate totals at the edges of the sweep (S - 1 .. 4 S + 1) and of the tile loop (L - 1 .. 2 L + 1) for c queries."""
    _, S = slices(min(c, L), L)
    return {S - 1, S, S + 1, 4 * S - 1, 4 * S, 4 * S + 1, L - 1, L, L + 1, 2 * L + 1}


def knn_cases():
    """(c, t) of the k-NN sweep: per query count the totals of both lane counts that hold the c queries themselves."""
    return [(c, t) for c in COUNTS for t in sorted(set().union(*(totals(c, L) for L in LANES))) if t >= max(c, 1)]


def nearest_cases():
    """(c, t) of the nearest-target sweep: 256 lanes only, every total and t = 0 (a query cell with nothing around it)."""
    return [(c, t) for c in COUNTS for t in sorted(totals(c, LANES[0]) | {0}) if t >= 0]


def _draw(rng, cell, m):
    """m distinct grid positions of the cell -> [m, 3]."""
    pos = rng.choice(GRID ** 3, m, replace=False)
    return np.asarray(cell, np.float64) + np.stack([pos // (GRID * GRID), pos // GRID % GRID, pos % GRID], 1) / float(GRID)


def _around(cell, own):
    """The cells around `cell` that lie in the lattice, the cell itself first if `own`."""
    out = [np.asarray(cell, np.float64)] if own else []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                n = np.asarray(cell, np.float64) + (dx, dy, dz)
                if (dx, dy, dz) != (0, 0, 0) and (n >= 0).all() and (n <= I.LAST).all():
                    out.append(n)
    return out


def _deal(rng, cells, m):
    """m points dealt round robin over the cells, each cell drawing from its own positions -> [m, 3]."""
    parts = [_draw(rng, cell, m // len(cells) + (j < m % len(cells))) for j, cell in enumerate(cells)]
    return np.concatenate(parts) if parts else np.zeros((0, 3))


def _placed(cases, borders):
    """-> [(cell, c, t)]: the cases along x at y = z = 10, then the border clusters."""
    return [((SPACING * j + 2.0, 10.0, 10.0), c, t) for j, (c, t) in enumerate(cases)] + [tuple(b) for b in borders]


def cell_keys(points):
    """One int64 per point: its cell (21 bits per axis, x lowest)."""
    cell = np.floor(np.asarray(points, np.float64)).astype(np.int64)
    return cell[:, 0] | (cell[:, 1] << 21) | (cell[:, 2] << 42)


def assert_apart(points, cluster):
    """No two clusters within reach of each other: between the cells of any two there is a gap of at least 2 on some axis, so no
    query's 27 cells hold a point of another cluster."""
    cell = np.floor(points)
    ids = np.unique(cluster)
    lo = np.stack([cell[cluster == j].min(0) for j in ids])
    hi = np.stack([cell[cluster == j].max(0) for j in ids])
    gap = np.maximum(lo[:, None, :] - hi[None, :, :], lo[None, :, :] - hi[:, None, :]).max(-1)
    gap[np.arange(len(ids)), np.arange(len(ids))] = 2
    assert (gap >= 2).all(), "clusters %s see each other" % (np.argwhere(gap < 2)[:3].tolist(),)


def knn_cloud(cases=None, borders=BORDERS, seed=31):
    """-> dict(P [n, 3] in a seeded order, cluster [n]: the cluster of each point, own [n]: in its cluster's first cell,
    cases [(cell, c, t)] by cluster)."""
    rng = np.random.default_rng(seed)
    placed = _placed(knn_cases() if cases is None else cases, borders)
    pts, cluster, own = [], [], []
    for j, (cell, c, t) in enumerate(placed):
        assert t >= c >= 1
        inner, outer = _draw(rng, cell, c), _deal(rng, _around(cell, False), t - c)
        pts += [inner, outer]
        cluster += [np.full(t, j)]
        own += [np.arange(t) < c]
    P, cluster, own = np.concatenate(pts), np.concatenate(cluster), np.concatenate(own)
    assert_apart(P, cluster)
    perm = rng.permutation(len(P))
    return dict(P=P[perm], cluster=cluster[perm], own=own[perm], cases=placed)


def nearest_clouds(cases=None, borders=BORDERS, seed=32):
    """-> dict(T [nt, 3], Q [nq, 3] in seeded orders, tcluster [nt], qcluster [nq], cases [(cell, c, t)] by cluster)."""
    rng = np.random.default_rng(seed)
    placed = _placed(nearest_cases() if cases is None else cases, borders)
    T, Q, tc, qc = [], [], [], []
    for j, (cell, c, t) in enumerate(placed):
        Q.append(_draw(rng, cell, c)), qc.append(np.full(c, j))
        T.append(_deal(rng, _around(cell, True), t)), tc.append(np.full(t, j))
    T, Q, tc, qc = np.concatenate(T), np.concatenate(Q), np.concatenate(tc), np.concatenate(qc)
    assert_apart(np.concatenate([T, Q]), np.concatenate([tc, qc]))
    pt, pq = rng.permutation(len(T)), rng.permutation(len(Q))
    return dict(T=T[pt], Q=Q[pq], tcluster=tc[pt], qcluster=qc[pq], cases=placed)


# ---- the brute force -------------------------------------------------------------------------------------------------------------
def _ranked(d2, number, width):
    """d2 [m, n] (inf: dropped), number [n] -> the first `width` of every row under (d2, number): (d2 [m, width], number [m, width],
    kept [m]), inf and -1 where a row holds fewer."""
    order = np.lexsort((np.broadcast_to(number, d2.shape), d2))[:, :width]
    rd2 = np.take_along_axis(d2, order, 1)
    rnum = np.where(np.isfinite(rd2), number[order], -1)
    pad = width - rd2.shape[1]
    if pad > 0:
        rd2 = np.concatenate([rd2, np.full((len(rd2), pad), np.inf)], 1)
        rnum = np.concatenate([rnum, np.full((len(rnum), pad), -1, np.int64)], 1)
    return rd2, rnum, np.isfinite(d2).sum(1)


def _groups(cluster):
    order = np.argsort(cluster, kind="stable")                  # within a cluster the numbers ascend
    return np.split(order, np.cumsum(np.bincount(cluster))[:-1])


def knn_brute(P, cluster, width=K_REF):
    """All pairs of every cluster in fp64, self dropped, d2 > R R dropped, np.lexsort((number, d2)) -> (d2 [n, width] fp64, index
    [n, width] int64, within [n]: the others within R, uncut)."""
    n = len(P)
    d2 = np.full((n, width), np.inf)
    index = np.full((n, width), -1, np.int64)
    within = np.zeros(n, np.int64)
    for ids in _groups(cluster):
        if len(ids) == 0:
            continue
        X = P[ids]
        d = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
        d[np.arange(len(ids)), np.arange(len(ids))] = np.inf
        d[d > R * R] = np.inf
        d2[ids], index[ids], within[ids] = _ranked(d, ids, width)
    return d2, index, within


def knn_cut(ref, k):
    """The first k of knn_brute's places (under a total order the first k of the first 33 are the first k) -> (d2, index, count)."""
    return ref[0][:, :k], ref[1][:, :k], np.minimum(ref[2], k)


def tie_at_last_place(ref, k):
    """[n] bool: the k-th and the (k + 1)-th of the reference lie at the same d2, so which of them is kept goes by number."""
    return np.isfinite(ref[0][:, k]) & (ref[0][:, k - 1] == ref[0][:, k])


def nearest_brute(T, Q, tcluster, qcluster):
    """-> (d2 [nq] fp64, inf where no target lies within D; index [nq] int64: the lowest number among the nearest, or -1)."""
    d2 = np.full(len(Q), np.inf)
    index = np.full(len(Q), -1, np.int64)
    nclusters = int(max(tcluster.max(initial=-1), qcluster.max(initial=-1))) + 1
    tg = _groups(np.concatenate([tcluster, np.arange(nclusters)]))      # a cluster without targets still has its (empty) group
    qg = _groups(np.concatenate([qcluster, np.arange(nclusters)]))
    for tid, qid in zip(tg, qg):
        tid, qid = tid[tid < len(T)], qid[qid < len(Q)]
        if len(tid) == 0 or len(qid) == 0:
            continue
        d = ((Q[qid][:, None, :] - T[tid][None, :, :]) ** 2).sum(-1)
        d[d > R * R] = np.inf
        rd2, rnum, _ = _ranked(d, tid, 1)
        d2[qid], index[qid] = rd2[:, 0], rnum[:, 0]
    return d2, index


# ---- what a row went through, for the properties and the messages ----------------------------------------------------------------------
def passes(points, L):
    """The pass of the L-lane kernel that serves each point as a query -> (cnt [n]: the queries of the pass, P [n], S [n],
    items: the work items of the cloud).  The sort by cell is stable, a cell's run is cut into items of CLOUD_TILE queries and an
    item into passes of L."""
    key = cell_keys(points)
    _, inv, count = np.unique(key, return_inverse=True, return_counts=True)
    order = np.argsort(inv, kind="stable")
    rank = np.empty(len(key), np.int64)
    rank[order] = np.arange(len(key)) - (np.cumsum(count) - count)[inv[order]]
    T = _lib.CLOUD_TILE
    item_count = np.minimum(count[inv] - rank // T * T, T)
    cnt = np.minimum(item_count - rank % T // L * L, L)
    P = np.array([slices(int(v), L)[0] for v in cnt])
    return cnt, P, L // P, int(((count + T - 1) // T).sum())


def candidates(points, targets=None):
    """[n]: the points of `targets` (default: the points themselves) in the 27 cells around each point."""
    cell = np.floor(points).astype(np.int64)
    tkeys, tcount = np.unique(cell_keys(points if targets is None else targets), return_counts=True)
    total = np.zeros(len(points), np.int64)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                n = cell + (dx, dy, dz)
                ok = ((n >= 0) & (n <= int(I.LAST))).all(1)
                key = n[:, 0] | (n[:, 1] << 21) | (n[:, 2] << 42)
                at = np.minimum(np.searchsorted(tkeys, key), len(tkeys) - 1)
                total += np.where(ok & (tkeys[at] == key), tcount[at], 0)
    return total


def describe(cloud, rows, k):
    """The (c, t, P, S) of the first few of `rows` of knn_cloud(): which edge a wrong row sits at."""
    cnt, P, S, _ = passes(cloud["P"], lanes_of(k))
    total = candidates(cloud["P"])
    out = []
    for r in np.asarray(rows)[:6]:
        _, c, t = cloud["cases"][cloud["cluster"][r]]
        out.append("row %d: cluster (c %d, t %d)%s, pass of %d queries, P %d, S %d, %d candidates"
                   % (r, c, t, "" if cloud["own"][r] else " neighbour cell", cnt[r], P[r], S[r], total[r]))
    return "k = %d, %d lanes, %d wrong rows; " % (k, lanes_of(k), len(rows)) + "; ".join(out)
