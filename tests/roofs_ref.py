"""numpy / Python-integer restatement of include/adamvs_hip.h "Roof planes", steps 1-7, written from the header's text and sharing
no code with ada_mvs_amd/roofs.py: the link bits, the segments (scipy's connected components of the edge list), the integer
moments, the exact rational plane fits, the growth rounds, the merge on the region graph and the residuals; and the scenes and
link patterns the tests run on."""
import math
from fractions import Fraction

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

COLUMNS = ("n", "su", "sv", "sq", "suu", "suv", "svv", "suq", "svq", "sqq_lo", "sqq_hi", "row_min", "row_max", "col_min", "col_max", "q_min",
           "q_max", "building")
SUMS, MINS, MAXS = COLUMNS[:11], ("row_min", "col_min", "q_min"), ("row_max", "col_max", "q_max", "building")
DEFAULTS = dict(smooth_span=1.0, smooth_tol=0.2, slope_tol=0.15, step_tol=0.1, assign_tol=0.2, min_plane_area=2.0, grow_rounds=None,
                merge_rms=0.1, flat_deg=5.0)
MAX_GROW = 256


def derived(gsd, dsm, smooth_span=1.0, slope_tol=0.15, grow_rounds=None):
    """-> (s, g_tol, z_ref, rounds)."""
    s = max(1, int(round(smooth_span / gsd)))
    z = np.asarray(dsm, np.float32)
    fin = z[np.isfinite(z)]
    z_ref = float(math.floor(float(fin.min()))) if fin.size else 0.0
    rounds = min(4 * s, MAX_GROW) if grow_rounds is None else int(grow_rounds)
    return s, slope_tol * (2 * s * gsd), z_ref, rounds


# ---- 1. links -----------------------------------------------------------------------------------------------------------
def core_ref(dsm, bld, s, smooth_tol):
    """-> (core bool, gx, gy fp64 (0 off core))."""
    z = np.asarray(dsm, np.float32).astype(np.float64)
    b = np.asarray(bld, np.int32)
    H, W = z.shape
    core = np.zeros((H, W), bool)
    gx, gy = np.zeros((H, W)), np.zeros((H, W))
    if H <= 2 * s or W <= 2 * s:
        return core, gx, gy
    c = (slice(s, H - s), slice(s, W - s))
    e, w = (slice(s, H - s), slice(2 * s, W)), (slice(s, H - s), slice(0, W - 2 * s))
    so, no = (slice(2 * s, H), slice(s, W - s)), (slice(0, H - 2 * s), slice(s, W - s))
    fin = np.isfinite(z)
    ok = (b[c] > 0) & fin[c]
    for nb in (e, w, so, no):
        ok &= (b[nb] == b[c]) & fin[nb]
    with np.errstate(invalid="ignore", over="ignore"):
        ok &= np.abs((z[e] + z[w]) - 2.0 * z[c]) <= smooth_tol
        ok &= np.abs((z[so] + z[no]) - 2.0 * z[c]) <= smooth_tol
        core[c] = ok
        gx[c] = np.where(ok, z[e] - z[w], 0.0)
        gy[c] = np.where(ok, z[so] - z[no], 0.0)
    return core, gx, gy


def links_ref(dsm, bld, s, smooth_tol, g_tol, step_tol):
    z = np.asarray(dsm, np.float32).astype(np.float64)
    b = np.asarray(bld, np.int32)
    core, gx, gy = core_ref(dsm, bld, s, smooth_tol)
    link = core.astype(np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for bit, A, B, g in ((2, (slice(None), slice(0, -1)), (slice(None), slice(1, None)), gx),
                             (4, (slice(0, -1), slice(None)), (slice(1, None), slice(None)), gy)):
            ok = core[A] & core[B] & (b[A] == b[B])
            ok &= np.abs(gx[A] - gx[B]) <= g_tol
            ok &= np.abs(gy[A] - gy[B]) <= g_tol
            ok &= np.abs((z[B] - z[A]) - (g[A] + g[B]) / (4.0 * s)) <= step_tol
            link[A] |= np.where(ok, bit, 0).astype(np.uint8)
    return link


# ---- 2. segments --------------------------------------------------------------------------------------------------------
def segments_ref(link):
    """-> (parent int32 (-1 off core, else the segment's smallest cell index), segment int32 (0 / 1 .. S), S)."""
    link = np.asarray(link, np.uint8)
    H, W = link.shape
    core = (link & 1) > 0
    idx = np.arange(H * W).reshape(H, W)
    east = np.zeros((H, W), bool)
    south = np.zeros((H, W), bool)
    east[:, :-1] = ((link[:, :-1] & 2) > 0) & core[:, :-1] & core[:, 1:]
    south[:-1, :] = ((link[:-1, :] & 4) > 0) & core[:-1, :] & core[1:, :]
    a = np.r_[idx[east], idx[south]]
    b = np.r_[idx[east] + 1, idx[south] + W]
    g = sp.coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(H * W, H * W))
    _, comp = connected_components(g, directed=False)
    smallest = np.full(comp.max() + 1, H * W, np.int64)
    np.minimum.at(smallest, comp, np.arange(H * W))
    parent = np.where(core.reshape(-1), smallest[comp], -1).astype(np.int32)
    roots = np.flatnonzero(parent == np.arange(H * W))
    number = np.zeros(H * W + 1, np.int32)
    number[roots] = np.arange(1, roots.size + 1)
    seg = np.where(parent >= 0, number[np.maximum(parent, 0)], 0).astype(np.int32)
    return parent.reshape(H, W), seg.reshape(H, W), int(roots.size)


# ---- 3. moments ---------------------------------------------------------------------------------------------------------
def quantise(dsm, z_ref):
    z = np.asarray(dsm, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.minimum(np.maximum((z - z_ref) * 256.0, 0.0), 524287.0)
    return np.where(np.isfinite(z), np.rint(x), 0).astype(np.int64)


def moments_ref(dsm, label, bld, z_ref, N):
    """-> int64 [18, N]."""
    z = np.asarray(dsm, np.float32)
    label = np.asarray(label, np.int32)
    H, W = z.shape
    use = (label >= 1) & (label <= N) & np.isfinite(z)
    k = label[use].astype(np.int64) - 1
    v, u = (a[use].astype(np.int64) for a in np.mgrid[0:H, 0:W])
    q = quantise(z, z_ref)[use]
    b = np.asarray(bld, np.int32)[use].astype(np.int64)
    t = {name: np.zeros(N, np.int64) for name in COLUMNS}
    for name in MINS:
        t[name][:] = 0x7FFFFFFF
    for name in MAXS:
        t[name][:] = -1
    for name, val in (("n", np.ones_like(u)), ("su", u), ("sv", v), ("sq", q), ("suu", u * u), ("suv", u * v), ("svv", v * v), ("suq", u * q),
                      ("svq", v * q), ("sqq_lo", (q * q) & 0xFFFFF), ("sqq_hi", (q * q) >> 20)):
        np.add.at(t[name], k, val)
    for name, val in (("row_min", v), ("col_min", u), ("q_min", q)):
        np.minimum.at(t[name], k, val)
    for name, val in (("row_max", v), ("col_max", u), ("q_max", q), ("building", b)):
        np.maximum.at(t[name], k, val)
    return np.stack([t[name] for name in COLUMNS])


# ---- 4. planes ----------------------------------------------------------------------------------------------------------
def fit_ref(row):
    """row: the 18 Python integers of a label -> None if the determinant is zero, else (a, b, c, sse) as Fractions in q units."""
    n, su, sv, sq, suu, suv, svv, suq, svq, lo, hi = (int(x) for x in row[:11])
    if n == 0:
        return None
    Suu, Svv, Suv = n * suu - su * su, n * svv - sv * sv, n * suv - su * sv
    Suq, Svq = n * suq - su * sq, n * svq - sv * sq
    D = Suu * Svv - Suv * Suv
    if D == 0:
        return None
    a, b = Fraction(Suq * Svv - Svq * Suv, D), Fraction(Svq * Suu - Suq * Suv, D)
    c = (sq - a * su - b * sv) / n
    sse = (lo + (hi << 20)) - a * suq - b * svq - c * sq
    return a, b, c, sse


def to_metres(fit):
    return [float(x / 256) for x in fit[:3]]


def planes_ref(table, gsd, min_plane_area):
    """-> (keep bool [S], planes fp64 [P, 3])."""
    rows = np.asarray(table).T.tolist()
    keep, planes = [], []
    for row in rows:
        f = fit_ref(row) if row[0] * (gsd * gsd) >= min_plane_area else None
        keep.append(f is not None)
        if f is not None:
            planes.append(to_metres(f))
    return np.array(keep, bool), np.array(planes, np.float64).reshape(-1, 3)


# ---- 5. growth ----------------------------------------------------------------------------------------------------------
def errors_ref(dsm, z_ref, planes, lab):
    """e of every cell against the plane lab (>= 1 where used)."""
    z = np.asarray(dsm, np.float32).astype(np.float64)
    H, W = z.shape
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    pl = np.asarray(planes, np.float64).reshape(-1, 3)
    p = np.clip(lab, 1, max(1, pl.shape[0])) - 1
    if pl.shape[0] == 0:
        return np.full((H, W), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs((z - z_ref) - ((pl[p, 0] * j + pl[p, 1] * i) + pl[p, 2]))


def grow_ref(dsm, bld, z_ref, planes, assign_tol, label, rounds):
    """-> (label after the rounds, counts int64 [rounds])."""
    z = np.asarray(dsm, np.float32)
    b = np.asarray(bld, np.int32)
    H, W = z.shape
    P = np.asarray(planes).reshape(-1, 3).shape[0]
    cur = np.asarray(label, np.int32).copy()
    counts = np.zeros(rounds, np.int64)
    for k in range(rounds):
        free = (cur == 0) & (b > 0) & np.isfinite(z)
        best_e = np.full((H, W), np.inf)
        best_p = np.zeros((H, W), np.int32)
        for di, dj in ((-1, 0), (0, -1), (0, 1), (1, 0)):
            nl = np.zeros((H, W), np.int32)
            nb = np.zeros((H, W), np.int32)
            dst = (slice(max(0, -di), H - max(0, di)), slice(max(0, -dj), W - max(0, dj)))
            src = (slice(max(0, di), H - max(0, -di)), slice(max(0, dj), W - max(0, -dj)))
            nl[dst], nb[dst] = cur[src], b[src]
            cand = free & (nl >= 1) & (nl <= P) & (nb == b)
            e = errors_ref(z, z_ref, planes, nl)
            with np.errstate(invalid="ignore"):
                better = cand & ((e < best_e) | ((e == best_e) & (nl < best_p)))
            best_e = np.where(better, e, best_e)
            best_p = np.where(better, nl, best_p)
        take = (best_p > 0) & (best_e <= assign_tol)
        nxt = np.where(take, best_p, cur).astype(np.int32)
        counts[k] = int(take.sum())
        cur = nxt
    return cur, counts


# ---- 6. merge -----------------------------------------------------------------------------------------------------------
def adjacency_ref(label, bld):
    """-> {(p, q): shared edges} with p < q, over 4-adjacent cells of different plane labels > 0 and the same building."""
    label, b = np.asarray(label), np.asarray(bld)
    adj = {}
    for A, B in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))), ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
        ok = (label[A] > 0) & (label[B] > 0) & (label[A] != label[B]) & (b[A] == b[B])
        for p, q in zip(label[A][ok].tolist(), label[B][ok].tolist()):
            key = (min(p, q), max(p, q))
            adj[key] = adj.get(key, 0) + 1
    return adj


def add_rows(r0, r1):
    out = [int(x) + int(y) for x, y in zip(r0[:11], r1[:11])]
    for k in range(11, 18):
        out.append(min(int(r0[k]), int(r1[k])) if COLUMNS[k] in MINS else max(int(r0[k]), int(r1[k])))
    return out


def merge_ref(rows, adj, merge_rms):
    """rows: list of P rows of Python integers; adj: {(p, q): edges}, 1-based -> (groups: list of sorted member lists ordered by
    their smallest member, rows of the groups).  Greedy: among the adjacent pairs whose summed moments fit with
    sse / 65536 <= merge_rms^2 n, the least sse / n (ties: the smaller (p, q)), until none qualifies."""
    rows = {p + 1: [int(x) for x in r] for p, r in enumerate(rows)}
    members = {p: [p] for p in rows}
    edges = {tuple(k): int(v) for k, v in adj.items()}
    if merge_rms > 0:
        bar = Fraction(merge_rms) ** 2 * 65536
        while True:
            best = None
            for (p, q) in sorted(edges):
                row = add_rows(rows[p], rows[q])
                f = fit_ref(row)
                if f is None or f[3] > bar * row[0]:
                    continue
                score = f[3] / row[0]
                if best is None or score < best[0]:
                    best = (score, p, q, row)
            if best is None:
                break
            _, p, q, row = best
            rows[p] = row
            members[p] = sorted(members[p] + members.pop(q))
            del rows[q]
            new = {}
            for (x, y), cnt in edges.items():
                x, y = (p if x == q else x), (p if y == q else y)
                if x != y:
                    key = (min(x, y), max(x, y))
                    new[key] = new.get(key, 0) + cnt
            edges = new
    order = sorted(members)
    return [members[p] for p in order], [rows[p] for p in order]


# ---- 7. residuals -------------------------------------------------------------------------------------------------------
def residuals_ref(dsm, label, z_ref, planes, assign_tol):
    """-> int64 [2, R]."""
    z = np.asarray(dsm, np.float32)
    label = np.asarray(label, np.int32)
    R = np.asarray(planes).reshape(-1, 3).shape[0]
    out = np.zeros((2, R), np.int64)
    use = (label >= 1) & (label <= R) & np.isfinite(z)
    e = errors_ref(z, z_ref, planes, label)[use]
    k = label[use].astype(np.int64) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(out[0], k, e <= assign_tol)
        m = np.where(np.isnan(e), 1048576.0, np.rint(np.minimum(e * 1024.0, 1048576.0)))
    np.maximum.at(out[1], k, m.astype(np.int64))
    return out


# ---- all of it ----------------------------------------------------------------------------------------------------------
def run_ref(dsm, bld, gsd, **kw):
    p = dict(DEFAULTS, **kw)
    dsm, bld = np.asarray(dsm, np.float32), np.asarray(bld, np.int32)
    s, g_tol, z_ref, rounds = derived(gsd, dsm, p["smooth_span"], p["slope_tol"], p["grow_rounds"])
    link = links_ref(dsm, bld, s, p["smooth_tol"], g_tol, p["step_tol"])
    parent, seg, S = segments_ref(link)
    seg_table = moments_ref(dsm, seg, bld, z_ref, S)
    keep, planes = planes_ref(seg_table, gsd, p["min_plane_area"])
    P = int(keep.sum())
    lut = np.zeros(S + 1, np.int32)
    lut[1:][keep] = np.arange(1, P + 1)
    seed = lut[seg]
    grown, counts = grow_ref(dsm, bld, z_ref, planes, p["assign_tol"], seed, rounds)
    grown_table = moments_ref(dsm, grown, bld, z_ref, P)
    adj = adjacency_ref(grown, bld)
    groups, rows = merge_ref(grown_table.T.tolist(), adj, p["merge_rms"])
    R = len(groups)
    lut2 = np.zeros(P + 1, np.int32)
    for r, g in enumerate(groups, start=1):
        lut2[g] = r
    label = lut2[grown]
    fits = [fit_ref(r) for r in rows]
    final_planes = np.array([to_metres(f) for f in fits], np.float64).reshape(-1, 3)
    resid = residuals_ref(dsm, label, z_ref, final_planes, p["assign_tol"])
    return dict(s=s, g_tol=g_tol, z_ref=z_ref, rounds=rounds, link=link, parent=parent, segments=seg, S=S, seg_table=seg_table, keep=keep,
                planes=planes, P=P, seed=seed, grown=grown, counts=counts, grown_table=grown_table, adjacency=adj, groups=groups,
                table=np.array(rows, np.int64).reshape(-1, 18).T, R=R, label=label, final_planes=final_planes, fits=fits, residuals=resid)


# ---- scenes -------------------------------------------------------------------------------------------------------------
def _noise(shape, amplitude, seed):
    """uniform in multiples of a quarter of the amplitude: -4 .. 4 quarters"""
    rng = np.random.default_rng(seed)
    return rng.integers(-4, 5, shape).astype(np.float64) * (amplitude / 4.0)


def four_roofs(noise=0.0, seed=0, gsd=0.5):
    """A gable (2 planes), a pyramid roof (4), a flat roof with a step (2) and a shed roof (1) on flat ground at 10 m ->
    (dsm fp32, building int32, truth: per building a list of (a, b) slopes in metres per cell)."""
    H, W = 150, 170
    z = np.full((H, W), 10.0)
    bld = np.zeros((H, W), np.int32)
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    truth = {}
    # 1: gable, ridge along the rows' direction (east-west) at the middle row; slope 0.25 per cell (pitch 0.5)
    r0, r1, c0, c1 = 10, 70, 10, 80
    m = (i >= r0) & (i < r1) & (j >= c0) & (j < c1)
    mid = (r0 + r1 - 1) / 2.0
    z[m] = (30.0 - 0.25 * np.abs(i - mid))[m]
    bld[m] = 1
    truth[1] = [(0.0, 0.25), (0.0, -0.25)]
    # 2: pyramid roof on a square, slope 0.2 per cell
    r0, r1, c0, c1 = 10, 70, 95, 155
    m = (i >= r0) & (i < r1) & (j >= c0) & (j < c1)
    ci, cj = (r0 + r1 - 1) / 2.0, (c0 + c1 - 1) / 2.0
    z[m] = (28.0 - 0.2 * np.maximum(np.abs(i - ci), np.abs(j - cj)))[m]
    bld[m] = 2
    truth[2] = [(0.0, 0.2), (0.0, -0.2), (0.2, 0.0), (-0.2, 0.0)]
    # 3: flat roof with a step of 1.5 m
    r0, r1, c0, c1 = 85, 140, 10, 80
    m = (i >= r0) & (i < r1) & (j >= c0) & (j < c1)
    z[m] = np.where(j < 45, 22.0, 23.5)[m]
    bld[m] = 3
    truth[3] = [(0.0, 0.0), (0.0, 0.0)]
    # 4: shed roof, slope 0.1 per cell along the columns
    r0, r1, c0, c1 = 85, 140, 95, 155
    m = (i >= r0) & (i < r1) & (j >= c0) & (j < c1)
    z[m] = (20.0 + 0.1 * (j - c0))[m]
    bld[m] = 4
    truth[4] = [(0.1, 0.0)]
    if noise:
        z = z + _noise(z.shape, noise, seed)
    return z.astype(np.float32), bld, truth


EXPECTED_PLANES = {1: 2, 2: 4, 3: 2, 4: 1}


def dome(noise=0.0, seed=1):
    H = W = 70
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    r2 = (i - 34.5) ** 2 + (j - 34.5) ** 2
    bld = (r2 <= 30.0 ** 2).astype(np.int32)
    z = np.where(bld > 0, 15.0 + np.sqrt(np.maximum(45.0 ** 2 - r2, 0.0)), 10.0)
    if noise:
        z = z + _noise(z.shape, noise, seed)
    return z.astype(np.float32), bld


def with_holes(dsm, fraction=0.02, seed=2):
    rng = np.random.default_rng(seed)
    z = np.array(dsm, np.float32)
    z[rng.random(z.shape) < fraction] = np.nan
    z[20:24, 30:37] = np.nan
    return z


def on_the_edge():
    """a shed roof whose building reaches the grid's north and west edges, and a gable that reaches the south-east corner"""
    H, W = 66, 75
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    z = np.full((H, W), 5.0)
    bld = np.zeros((H, W), np.int32)
    m = (i < 30) & (j < 33)
    z[m] = (12.0 + 0.125 * j + 0.0625 * i)[m]
    bld[m] = 1
    m = (i >= 40) & (j >= 40)
    z[m] = (16.0 - 0.25 * np.abs(j - 57.0))[m]
    bld[m] = 2
    return z.astype(np.float32), bld


def touching():
    """two buildings that share a wall line: the same roof plane runs across both labels"""
    H, W = 50, 90
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    z = np.full((H, W), 3.0)
    bld = np.zeros((H, W), np.int32)
    m = (i >= 5) & (i < 45) & (j >= 5) & (j < 85)
    z[m] = (9.0 + 0.125 * (i - 5))[m]
    bld[m & (j < 44)] = 1
    bld[m & (j >= 44)] = 2
    return z.astype(np.float32), bld


# ---- link patterns given directly -----------------------------------------------------------------------------------------
def random_links(H, W, density, seed):
    """every bit of the low three drawn independently with the given probability, plus noise in the ignored high bits"""
    rng = np.random.default_rng(seed)
    link = np.zeros((H, W), np.uint8)
    for bit in (1, 2, 4):
        link |= np.where(rng.random((H, W)) < density, bit, 0).astype(np.uint8)
    link |= (rng.integers(0, 2, (H, W)) << 3).astype(np.uint8)
    return link


def serpentine_links(H, W):
    """every cell core; rows linked along their whole length, consecutive rows linked only at alternating ends: one segment that
    winds through every row, adjacent rows otherwise separated by unlinked walls"""
    link = np.full((H, W), 1, np.uint8)
    link[:, :-1] |= 2
    for i in range(H - 1):
        link[i, (W - 1) if i % 2 == 0 else 0] |= 4
    return link


def comb_links(H, W):
    """every cell core; the top row linked along its length and every column linked downwards: one segment whose teeth are
    adjacent core columns without a link between them"""
    link = np.full((H, W), 1, np.uint8)
    link[0, :-1] |= 2
    link[:-1, :] |= 4
    return link


def checkerboard_links(H, W):
    """2 x 2 blocks aligned to even cells, fully linked inside, no link between blocks: no segment crosses a tile border"""
    link = np.full((H, W), 1, np.uint8)
    link[:, 0:W - 1:2] |= 2
    link[0:H - 1:2, :] |= 4
    return link
