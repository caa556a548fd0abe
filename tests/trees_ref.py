"""numpy restatement of include/adamvs_hip.h "Trees", steps 1-10, written literally: the canopy and the integer surface, the
windows by explicit shifts over the disc, the parents, the roots by following the parents cell by cell, the crowns and the
table; detect_ref mirrors ada_mvs_amd/trees.py detect() without a GPU; and the scenes the tests run on."""
import numpy as np

from ada_mvs_amd import trees
from buildings_ref import serpentine_mask

COLUMNS = ("cells", "q_sum", "q_max", "row_min", "row_max", "col_min", "col_max", "r2_max", "top", "s_top")


# ---- steps 1 and 2 ------------------------------------------------------------------------------------------------------------
def surface_ref(ndsm, building, min_height, smooth_passes):
    """-> (mask uint8, q int32, s int32 (-1 outside the canopy), s_max)."""
    nd = np.asarray(ndsm, np.float32)
    H, W = nd.shape
    with np.errstate(invalid="ignore"):
        C = np.isfinite(nd) & (nd.astype(np.float64) >= float(min_height))
    if building is not None:
        C &= np.asarray(building) == 0
    q = np.zeros((H, W), np.int64)
    q[C] = np.rint(np.minimum(nd[C].astype(np.float64), 2047.0) * 256.0).astype(np.int64)
    s = q.copy()
    for _ in range(int(smooth_passes)):
        nxt = np.zeros((H, W), np.int64)
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                w = (2 - abs(di)) * (2 - abs(dj))
                nb, ok = s.copy(), np.zeros((H, W), bool)              # the neighbour's value where it exists in C, else the centre's
                dst = (slice(max(0, -di), H - max(0, di)), slice(max(0, -dj), W - max(0, dj)))
                src = (slice(max(0, di), H - max(0, -di)), slice(max(0, dj), W - max(0, -dj)))
                ok[dst] = C[src]
                shifted = np.zeros((H, W), np.int64)
                shifted[dst] = s[src]
                nb[ok] = shifted[ok]
                nxt += w * nb
        s = nxt
    s = np.where(C, s, -1)
    return C.astype(np.uint8), q.astype(np.int32), s.astype(np.int32), (int(s.max()) if C.any() else -1)


# ---- steps 3 to 6 -------------------------------------------------------------------------------------------------------------
def keys_ref(s):
    """The order of step 3 as one integer per cell: the larger key beats; 0 outside the canopy."""
    s = np.asarray(s, np.int64)
    idx = np.arange(s.size, dtype=np.int64).reshape(s.shape)
    return np.where(s >= 0, (s << 32) | (0xFFFFFFFF - idx), 0)


def _shifted(a, di, dj, fill=0):
    """b(i, j) = a(i + di, j + dj), `fill` outside the grid."""
    H, W = a.shape
    b = np.full((H, W), fill, a.dtype)
    if abs(di) >= H or abs(dj) >= W:
        return b
    dst = (slice(max(0, -di), H - max(0, di)), slice(max(0, -dj), W - max(0, dj)))
    src = (slice(max(0, di), H - max(0, -di)), slice(max(0, dj), W - max(0, -dj)))
    b[dst] = a[src]
    return b


def parents_ref(s, thr):
    """-> (parent int32, top bool, radius int64): steps 4 to 6 with the windows by explicit shifts over the disc."""
    s = np.asarray(s, np.int64)
    H, W = s.shape
    C = s >= 0
    key = keys_ref(s)
    radius = np.where(C, trees.window_cells(np.maximum(s, 0), thr), 0)
    r2 = radius * radius
    rmax = int(radius.max()) if C.any() else 0
    best_w = key.copy()                                              # the best key of the window: the cell itself to begin with
    for di in range(-rmax, rmax + 1):
        for dj in range(-rmax, rmax + 1):
            d2 = di * di + dj * dj
            if d2 == 0 or d2 > rmax * rmax:
                continue
            k = _shifted(key, di, dj)
            take = (r2 >= d2) & (k > best_w)
            best_w[take] = k[take]
    best_n = np.zeros((H, W), np.int64)                              # b(c)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            if di or dj:
                best_n = np.maximum(best_n, _shifted(key, di, dj))
    top = C & (best_w == key) & (best_n <= key)                      # the disc of r = 1 lacks the diagonal neighbours
    own = np.arange(H * W, dtype=np.int64).reshape(H, W)
    cell_of = lambda k: 0xFFFFFFFF - (k & 0xFFFFFFFF)
    parent = np.where(best_n > key, cell_of(best_n), np.where(top, own, cell_of(best_w)))
    parent = np.where(C, parent, -1)
    return parent.astype(np.int32), top, radius


def roots_ref(parent):
    """root(c) by following the parents cell by cell (what a walk has found is remembered) -> int32, -1 outside the canopy."""
    par = np.asarray(parent).reshape(-1).tolist()
    root = [-2] * len(par)
    for c0 in range(len(par)):
        if par[c0] < 0:
            root[c0] = -1
            continue
        path, c = [], c0
        while root[c] == -2 and par[c] != c:
            path.append(c)
            c = par[c]
        r = c if root[c] == -2 else root[c]
        root[c] = r
        for v in path:
            root[v] = r
    return np.array(root, np.int32).reshape(np.asarray(parent).shape)


def jump_rounds_ref(parent, hops=8):
    """The rounds of double-buffered pointer jumping, `hops` parents per cell and round (ADAMVS_TREE_JUMP_HOPS), that move a
    pointer."""
    cur = np.asarray(parent, np.int64).reshape(-1)
    rounds = 0
    while True:
        nxt = cur
        for _ in range(hops - 1):                                    # a root is its own parent: the walk stays there
            nxt = np.where(nxt >= 0, cur[np.maximum(nxt, 0)], -1)
        if np.array_equal(nxt, cur):
            return rounds
        cur, rounds = nxt, rounds + 1


# ---- steps 8 and 9 ------------------------------------------------------------------------------------------------------------
def crowns_ref(s, root, ratio_pm, rc2):
    """-> (label int32: tops numbered 1 .. T in ascending cell index, T, unassigned)."""
    s, root = np.asarray(s, np.int64), np.asarray(root, np.int64)
    H, W = s.shape
    own = np.arange(H * W, dtype=np.int64).reshape(H, W)
    is_top = root == own
    number = np.cumsum(is_top.reshape(-1)).reshape(H, W)
    T = int(is_top.sum())
    C = root >= 0
    t = np.maximum(root, 0)
    i, j = np.divmod(own, W)
    it, jt = np.divmod(t, W)
    ok = C & (s * 1000 >= int(ratio_pm) * s.reshape(-1)[t]) & ((i - it) ** 2 + (j - jt) ** 2 <= int(rc2))
    label = np.where(ok, number.reshape(-1)[t], 0).astype(np.int32)
    return label, T, int((C & ~ok).sum())


def table_ref(label, T, q, s, root):
    """dict of int64 [T] per column."""
    label, q, s, root = (np.asarray(a) for a in (label, q, s, root))
    W = label.shape[1]
    idx = np.flatnonzero(label)
    k = label.reshape(-1)[idx].astype(np.int64) - 1
    rows, cols = idx // W, idx % W
    t = root.reshape(-1)[idx].astype(np.int64)
    qq = q.reshape(-1)[idx].astype(np.int64)
    tab = {name: np.full(T, -1, np.int64) for name in COLUMNS}
    tab["cells"][:] = tab["q_sum"][:] = 0
    tab["row_min"][:] = tab["col_min"][:] = 0x7FFFFFFF
    np.add.at(tab["cells"], k, 1)
    np.add.at(tab["q_sum"], k, qq)
    np.maximum.at(tab["q_max"], k, qq)
    np.minimum.at(tab["row_min"], k, rows)
    np.maximum.at(tab["row_max"], k, rows)
    np.minimum.at(tab["col_min"], k, cols)
    np.maximum.at(tab["col_max"], k, cols)
    np.maximum.at(tab["r2_max"], k, (rows - t // W) ** 2 + (cols - t % W) ** 2)
    np.maximum.at(tab["top"], k, t)
    np.maximum.at(tab["s_top"], k, s.reshape(-1)[t].astype(np.int64))
    return tab


def stage_ref(ndsm, building, min_height, smooth_passes, thr, ratio_pm, rc2):
    """Steps 1 to 9 with a given window table -> dict(mask, q, s, s_max, parent, top, root, crowns, T, unassigned, table)."""
    mask, q, s, s_max = surface_ref(ndsm, building, min_height, smooth_passes)
    parent, top, radius = parents_ref(s, thr)
    root = roots_ref(parent)
    crowns, T, unassigned = crowns_ref(s, root, ratio_pm, rc2)
    assert T == int(top.sum()) and np.array_equal(root.reshape(-1)[np.flatnonzero(top)], np.flatnonzero(top))    # the roots are the tops
    return dict(mask=mask, q=q, s=s, s_max=s_max, parent=parent, top=top, root=root, crowns=crowns, T=T, unassigned=unassigned,
                table=table_ref(crowns, T, q, s, root), radius=radius)


def detect_ref(ndsm, gsd, building=None, grid=None, **kw):
    """trees.detect() without a GPU: the same keys, the device's share from the restatement above."""
    from ada_mvs_amd.dsm import Grid
    ndsm = np.ascontiguousarray(ndsm, np.float32)
    H, W = ndsm.shape
    p = trees.parameters(gsd, **kw)
    mask, q, s, s_max = surface_ref(ndsm, building, p["min_height"], p["smooth_passes"])
    p = trees.parameters(gsd, s_max=s_max, **kw)
    thr = trees.window_table(gsd, p["radius_min"], p["radius_slope"], p["smooth_passes"], s_max)
    r = stage_ref(ndsm, building, p["min_height"], p["smooth_passes"], thr, p["ratio_pm"], p["rc2"])
    table = dict(r["table"])
    table["q_top"] = r["q"].reshape(-1)[table["top"]].astype(np.int64) if r["T"] else np.zeros(0, np.int64)
    keep, counts = trees.select(table, gsd, p["min_crown_area"])
    lut = np.zeros(r["T"] + 1, np.int32)
    lut[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    label = lut[r["crowns"]]
    counts = dict(canopy=int(mask.sum()), labelled=int((r["crowns"] > 0).sum()), unassigned=r["unassigned"], **counts)
    if grid is None:
        grid = Grid(0.0, H * float(gsd), float(gsd), 0.0, W, H)
    polys, props = trees.finish(label, table, keep, counts, grid, thr)
    return dict(label=label, crowns=r["crowns"], mask=mask, q=r["q"], s=r["s"], parent=r["parent"], root=r["root"], T=r["T"], thr=thr,
                s_max=s_max, table=table, keep=keep, properties=props, polygons=polys, counts=counts, params=p, gsd=float(gsd), grid=grid,
                top=r["top"], jump_rounds=jump_rounds_ref(r["parent"]))


# ---- scenes -------------------------------------------------------------------------------------------------------------------
CROWN_GSD = 0.5
CROWN_TREES = ((30, 30, 14, 12.0), (30, 90, 10, 8.0), (80, 50, 16, 20.0), (120, 120, 12, 15.0), (125, 30, 8, 6.0),
               (60, 130, 9, 9.0))                                    # row, column, radius in cells, height of the top in metres
CROWN_BOXES = ((90, 85, 20, 24, 6.0), (5, 120, 14, 30, 9.0))         # row, column, rows, columns, metres: roof_scene-style boxes


def crown_scene(H=150, W=160):
    """Paraboloid crowns h (1 - 0.6 d^2 / R^2) with integer tops at known cells, farther apart than their windows, on flat
    ground, and two flat boxes that carry building labels, at gsd 0.5 m -> (ndsm float32, building int32, truth) with
    truth = dict(tops=[cell index, ...] ascending, heights=[metres, ...] in that order, discs=[mask, ...] in that order)."""
    i, j = np.mgrid[0:H, 0:W]
    nd = np.zeros((H, W), np.float64)
    items = []
    for ci, cj, rad, h in CROWN_TREES:
        d2 = (i - ci) ** 2 + (j - cj) ** 2
        disc = d2 <= rad * rad
        nd[disc] = (h * (1.0 - 0.6 * d2 / float(rad * rad)))[disc]
        items.append((ci * W + cj, h, disc))
    building = np.zeros((H, W), np.int32)
    for k, (i0, j0, h, w, dz) in enumerate(CROWN_BOXES, start=1):
        nd[i0:i0 + h, j0:j0 + w] = dz
        building[i0:i0 + h, j0:j0 + w] = k
    items.sort(key=lambda t: t[0])
    return nd.astype(np.float32), building, dict(tops=[t[0] for t in items], heights=[t[1] for t in items], discs=[t[2] for t in items])


def plateau(H, W, height=5.0):
    return np.full((H, W), height, np.float32)


def serpentine_ramp(H, W, base=2.0):
    """A one-cell-wide canopy path through the whole raster (buildings_ref.serpentine_mask) that rises by 1/256 m per cell along
    its whole length; 0 elsewhere."""
    m = serpentine_mask(H, W)
    nd = np.zeros((H, W), np.float64)
    k = 0
    for n, i in enumerate(range(0, H, 2)):
        cols = range(W) if n % 2 == 0 else range(W - 1, -1, -1)
        for j in cols:
            nd[i, j] = base + k / 256.0
            k += 1
        if i + 1 < H and m[i + 1].any():
            nd[i + 1, W - 1 if n % 2 == 0 else 0] = base + k / 256.0
            k += 1
    assert np.array_equal(nd > 0, m) and base + k / 256.0 < 2047.0
    return nd.astype(np.float32)


def random_canopy(H, W, density, seed, lo=2.0, hi=12.0):
    """Seeded heights in lo .. hi m on `density` of the cells, 0 elsewhere."""
    rng = np.random.default_rng(seed)
    nd = rng.uniform(lo, hi, (H, W))
    nd[rng.random((H, W)) >= density] = 0.0
    return nd.astype(np.float32)
