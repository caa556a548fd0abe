"""The drainage stage restated on the host (include/adamvs_hip.h "Drainage", steps 1 - 7) by other algorithms, in numpy and the
standard library: the fill by priority-flood plus one unit with heapq, the directions by the definition, the accumulation by
one pass over the cells in descending F, the roots by walking, the links by walking down from the heads, the Strahler order by
recursion, and the bound on the rounds of the tiled fill.  It shares no code with ada-mvs_amd/drainage.py or with the kernels: no
relaxation, no pointer doubling, no scans."""
import heapq
import sys

import numpy as np

from contours_ref import surface

NONE = -2 ** 31
UNITS = 65536
# E, SE, S, SW, W, NW, N, NE: (row step, column step), code 1 << k
STEPS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))


def routing_surface(z, z_ref, passes):
    """-> (s, r) int64 [H, W]: r = s 2^(8 - 4 passes), NONE outside V"""
    s, _ = surface(z, z_ref, passes)
    return s, np.where(s == NONE, NONE, s * 2 ** (8 - 4 * passes))


def edge_cells(r):
    """-> bool [H, W]: in V and on the border or next to a cell outside V"""
    V = r != NONE
    H, W = r.shape
    vp = np.pad(V, 1)
    whole = np.ones((H, W), bool)
    for di, dj in STEPS:
        whole &= vp[1 + di:1 + di + H, 1 + dj:1 + dj + W]
    return V & ~whole


def fill(r):
    """Priority-flood from the edge cells, raising every cell to at least its parent's level + 1 -> F int64 [H, W]"""
    H, W = r.shape
    F = np.full((H, W), NONE, np.int64)
    done = r == NONE
    heap = []
    for i, j in np.argwhere(edge_cells(r)).tolist():
        F[i, j] = r[i, j]
        done[i, j] = True
        heap.append((int(r[i, j]), i, j))
    heapq.heapify(heap)
    while heap:
        f, i, j = heapq.heappop(heap)
        for di, dj in STEPS:
            a, b = i + di, j + dj
            if 0 <= a < H and 0 <= b < W and not done[a, b]:
                done[a, b] = True
                F[a, b] = max(int(r[a, b]), f + 1)
                heapq.heappush(heap, (int(F[a, b]), a, b))
    return F


def directions(F, edge):
    """-> (dir uint8 [H, W], recv int64 [H W]: the receiver's index, -1 for none)"""
    H, W = F.shape
    d = np.full((H, W), 255, np.uint8)
    recv = np.full(H * W, -1, np.int64)
    for i in range(H):
        for j in range(W):
            if F[i, j] == NONE:
                continue
            d[i, j] = 0
            if edge[i, j]:
                continue
            best, code, to = 0, 0, -1
            for k, (di, dj) in enumerate(STEPS):
                drop = int(F[i, j]) - int(F[i + di, j + dj])
                if drop <= 0:
                    continue
                key = drop * drop * (1 if k % 2 else 2)            # squared slopes times two: exact in Python integers
                if key > best:
                    best, code, to = key, 1 << k, (i + di) * W + j + dj
            d[i, j], recv[i * W + j] = code, to
    return d, recv


def accumulate(F, recv, value):
    """value int [H W] -> acc int64 [H W]: one pass in descending F, so that every donor comes before its receiver"""
    acc = np.asarray(value, np.int64).copy()
    flat = F.reshape(-1)
    for c in np.argsort(-flat, kind="stable").tolist():
        if flat[c] != NONE and recv[c] >= 0:
            acc[recv[c]] += acc[c]
    return acc


def roots(F, recv):
    root = np.full(recv.size, -1, np.int64)
    for c in np.flatnonzero(F.reshape(-1) != NONE).tolist():
        at = c
        while recv[at] >= 0:
            at = recv[at]
        root[c] = at
    return root


def basins(root, acc, min_cells):
    """-> (int64 [H W]: 1 .. K for the cells of the outlets with acc >= min_cells in ascending index, 0 elsewhere; K)"""
    outlets = [c for c in np.flatnonzero(root == np.arange(root.size)).tolist() if acc[c] >= min_cells]
    number = {c: k + 1 for k, c in enumerate(outlets)}
    return np.array([number.get(int(c), 0) for c in root], np.int64), len(outlets)


def streams(F, recv, acc, min_cells):
    """-> dict(nd uint8, link, pos int64 [H W], link_first, link_head, link_end, link_to, vertex, L, P) by walking from the heads"""
    n = recv.size
    stream = (F.reshape(-1) != NONE) & (acc >= min_cells)
    nd = np.zeros(n, np.int64)
    for c in np.flatnonzero(stream).tolist():
        if recv[c] >= 0:
            nd[recv[c]] += 1
    heads = [c for c in np.flatnonzero(stream).tolist() if nd[c] != 1 and recv[c] >= 0]
    number = {c: l for l, c in enumerate(heads)}
    link, pos = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    first, end, to, vertex = [0], [], [], []
    for l, h in enumerate(heads):
        at, k = h, 0
        while True:
            vertex.append(at)
            link[at], pos[at] = l, k
            nxt = int(recv[at])
            if nxt < 0:                                             # an outlet the link owns
                end.append(at)
                to.append(-1)
                break
            if nd[nxt] != 1:                                        # a head: the last vertex, not owned
                vertex.append(nxt)
                end.append(nxt)
                to.append(number.get(nxt, -1))
                break
            at, k = nxt, k + 1
        first.append(len(vertex))
    return dict(nd=np.where(stream, nd, 255).astype(np.uint8), link=link, pos=pos, link_first=np.array(first, np.int64),
                link_head=np.array(heads, np.int64), link_end=np.array(end, np.int64), link_to=np.array(to, np.int64),
                vertex=np.array(vertex, np.int64), L=len(heads), P=len(vertex))


def strahler(link_to):
    """-> int64 [L] by recursion over the links that flow into a link"""
    L = len(link_to)
    into = [[] for _ in range(L)]
    for l, t in enumerate(np.asarray(link_to).tolist()):
        if t >= 0:
            into[t].append(l)
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * L + 1000))
    memo = {}

    def order(l):
        if l not in memo:
            ups = sorted((order(u) for u in into[l]), reverse=True)
            memo[l] = 1 if not ups else ups[0] + 1 if len(ups) >= 2 and ups[1] == ups[0] else ups[0]
        return memo[l]
    return np.array([order(l) for l in range(L)], np.int64)


def rounds_bound(F, edge, T):
    """The header's bound on the rounds of the tiled fill that change a word: t = 0 at an edge cell, elsewhere max(1, min over the
    neighbours n with F(n) < F(c) of t(n) + [n in another tile]); -> max t (0 if no cell moves)."""
    H, W = F.shape
    t = np.zeros((H, W), np.int64)
    flat = F.reshape(-1)
    worst = 0
    for c in np.argsort(flat, kind="stable").tolist():
        i, j = divmod(c, W)
        if flat[c] == NONE or edge[i, j]:
            continue
        best = None
        for di, dj in STEPS:
            a, b = i + di, j + dj
            if F[a, b] < F[i, j]:
                v = int(t[a, b]) + (0 if (a // T, b // T) == (i // T, j // T) else 1)
                best = v if best is None or v < best else best
        t[i, j] = max(1, best)
        worst = max(worst, int(t[i, j]))
    return worst


def route(z, z_ref=0.0, passes=0, min_cells=1, tile=32):
    """-> the dict of every array of the stage, flat arrays reshaped to [H, W] where the header says so"""
    z = np.asarray(z, np.float32)
    H, W = z.shape
    s, r = routing_surface(z, z_ref, passes)
    edge = edge_cells(r)
    F = fill(r)
    d, recv = directions(F, edge)
    valid = (F != NONE).reshape(-1)
    acc = accumulate(F, recv, valid.astype(np.int64))
    root = roots(F, recv)
    bas, K = basins(root, acc, min_cells)
    st = streams(F, recv, acc, min_cells)
    source = ((st["nd"] == 0)).astype(np.int64)
    mag = accumulate(F, recv, source)
    res = dict(s=s, r=r, F=F, edge=edge, dir=d, recv=recv, acc=acc.reshape(H, W), root=root.reshape(H, W), basins=bas.reshape(H, W), K=K,
               magnitude=mag.reshape(H, W), bound=rounds_bound(F, edge, tile))
    res.update(st)
    for k in ("nd", "link", "pos"):
        res[k] = res[k].reshape(H, W)
    res["strahler"] = strahler(st["link_to"])
    return res
