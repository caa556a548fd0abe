"""numpy restatement of include/adamvs_hip.h "Building extraction", steps 1-6: the candidate mask, the opening (tests/dtm_ref.py),
the flatness flags, the 4-connected components by a plain flood fill, the per-component table and the selection; and the
scenes the tests run on."""
import math

import numpy as np

from dtm_ref import open_brute, open_sep

COLUMNS = ("cells", "smooth", "rough", "undetermined", "row_min", "row_max", "col_min", "col_max", "height_sum", "height_max_bits")
DIRECTIONS = ((0, 1), (1, 0), (1, 1), (1, -1))
DEFAULTS = dict(min_height=2.5, min_width=2.0, smooth_span=1.0, smooth_tol=0.2, min_smooth=0.5, min_area=10.0)


def cell_parameters(gsd, min_width=2.0, smooth_span=1.0):
    """-> (r_open, s): floor(min_width / (2 gsd)) and max(1, round(smooth_span / gsd)), half to even."""
    return int(math.floor(min_width / (2.0 * gsd))), max(1, int(round(smooth_span / gsd)))


def mask_ref(ndsm, min_height, r_open, opening=open_sep):
    """-> (M0, M)."""
    ndsm = np.asarray(ndsm, np.float32)
    with np.errstate(invalid="ignore"):
        m0 = np.isfinite(ndsm) & (ndsm.astype(np.float64) >= float(min_height))
    if r_open == 0:
        return m0, m0.copy()
    return m0, opening(m0.astype(np.float32), int(r_open)) == np.float32(1.0)


def flags_ref(dsm, ndsm, min_height, r_open, s, smooth_tol, opening=open_sep):
    """uint8 [H, W]: 0 not a candidate, 1 removed by the opening, 2 undetermined, 3 smooth, 4 rough."""
    z = np.asarray(dsm, np.float32)
    H, W = z.shape
    m0, m = mask_ref(ndsm, min_height, r_open, opening)
    z64, fin = z.astype(np.float64), np.isfinite(z)
    counting = np.zeros((H, W), np.int64)
    rough = np.zeros((H, W), bool)
    for di, dj in DIRECTIONS:
        oi, oj = s * di, s * dj
        i0, i1 = max(0, oi, -oi), H - max(0, oi, -oi)              # rows c with both neighbours inside
        j0, j1 = max(0, oj, -oj), W - max(0, oj, -oj)
        if i0 >= i1 or j0 >= j1:
            continue
        c = (slice(i0, i1), slice(j0, j1))
        a = (slice(i0 - oi, i1 - oi), slice(j0 - oj, j1 - oj))
        b = (slice(i0 + oi, i1 + oi), slice(j0 + oj, j1 + oj))
        counts = m[a] & m[b] & fin[a] & fin[b]
        with np.errstate(invalid="ignore", over="ignore"):
            D = np.abs((z64[a] + z64[b]) - 2.0 * z64[c])
            bad = counts & ~(D <= float(smooth_tol))
        counting[c] += counts
        rough[c] |= bad
    flags = np.zeros((H, W), np.uint8)
    flags[m0] = 1
    flags[m] = np.where(counting[m] == 0, 2, np.where(rough[m], 4, 3))
    return flags


def components_ref(m):
    """4-connected components of the mask by flood fill, scanned in cell order: label int32 (0 outside), numbered 1 .. N in
    ascending order of the smallest cell index -> (label, N)."""
    m = np.asarray(m, bool)
    H, W = m.shape
    todo = m.reshape(-1).tolist()
    label = [0] * (H * W)
    N = 0
    for c0 in np.flatnonzero(m).tolist():
        if not todo[c0]:
            continue
        N += 1
        todo[c0] = False
        stack = [c0]
        while stack:
            c = stack.pop()
            label[c] = N
            j = c % W
            if j > 0 and todo[c - 1]:
                todo[c - 1] = False
                stack.append(c - 1)
            if j + 1 < W and todo[c + 1]:
                todo[c + 1] = False
                stack.append(c + 1)
            if c >= W and todo[c - W]:
                todo[c - W] = False
                stack.append(c - W)
            if c + W < H * W and todo[c + W]:
                todo[c + W] = False
                stack.append(c + W)
    return np.array(label, np.int32).reshape(H, W), N


def table_ref(label, N, flags, ndsm):
    """dict of int64 [N] per column."""
    label, flags = np.asarray(label), np.asarray(flags)
    nd = np.asarray(ndsm, np.float32)
    idx = np.flatnonzero(label)
    k = label.reshape(-1)[idx].astype(np.int64) - 1
    f = flags.reshape(-1)[idx]
    rows, cols = idx // label.shape[1], idx % label.shape[1]
    v = nd.reshape(-1)[idx]
    t = {name: np.zeros(N, np.int64) for name in COLUMNS}
    t["row_min"][:] = t["col_min"][:] = 0x7FFFFFFF
    t["row_max"][:] = t["col_max"][:] = -1
    np.add.at(t["cells"], k, 1)
    np.add.at(t["smooth"], k, f == 3)
    np.add.at(t["rough"], k, f == 4)
    np.add.at(t["undetermined"], k, f == 2)
    np.minimum.at(t["row_min"], k, rows)
    np.maximum.at(t["row_max"], k, rows)
    np.minimum.at(t["col_min"], k, cols)
    np.maximum.at(t["col_max"], k, cols)
    np.add.at(t["height_sum"], k, np.rint(np.minimum(v.astype(np.float64), 65535.0) * 1024.0).astype(np.int64))
    np.maximum.at(t["height_max_bits"], k, v.view(np.uint32).astype(np.int64))
    return t


def select_ref(table, gsd, min_area, min_smooth):
    """-> (keep, counts), component by component as stated."""
    keep, small, rough = [], 0, 0
    for cells, s, r in zip(table["cells"].tolist(), table["smooth"].tolist(), table["rough"].tolist()):
        big = cells * (gsd * gsd) >= min_area
        flat = (s >= min_smooth * (s + r)) if s + r > 0 else (min_smooth == 0)
        keep.append(bool(big and flat))
        small += not big
        rough += bool(big and not flat)
    keep = np.array(keep, bool)
    return keep, dict(components=len(keep), buildings=int(keep.sum()), rejected_small=small, rejected_rough=rough)


def extract_ref(dsm, ndsm, gsd, min_height=2.5, min_width=2.0, smooth_span=1.0, smooth_tol=0.2, min_smooth=0.5, min_area=10.0,
                opening=open_sep):
    """Steps 1-6 -> dict(flags, components, N, table, keep, label, counts)."""
    r_open, s = cell_parameters(gsd, min_width, smooth_span)
    flags = flags_ref(dsm, ndsm, min_height, r_open, s, smooth_tol, opening)
    comp, N = components_ref(flags >= 2)
    table = table_ref(comp, N, flags, ndsm)
    keep, counts = select_ref(table, gsd, min_area, min_smooth)
    lut = np.zeros(N + 1, np.int32)
    lut[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    hist = np.bincount(flags.reshape(-1), minlength=5)
    counts = dict(candidate=int(hist[1:].sum()), opened_away=int(hist[1]), undetermined=int(hist[2]), smooth=int(hist[3]), rough=int(hist[4]),
                  **counts)
    return dict(flags=flags, components=comp, N=N, table=table, keep=keep, label=lut[comp], counts=counts, r_open=r_open, stride=s)


# ---- scenes: every builder returns (dsm, ndsm) float32 with heights in multiples of 1/8 m, so that every D is exact -----------
def rasters_of_mask(mask, seed=0, height=5.0):
    """ndsm = `height` on the mask and 0 elsewhere; dsm = seeded multiples of 1/8 m in 50 .. 54 m."""
    mask = np.asarray(mask, bool)
    rng = np.random.default_rng(seed)
    dsm = 50.0 + rng.integers(0, 33, mask.shape) / 8.0
    return dsm.astype(np.float32), np.where(mask, height, 0.0).astype(np.float32)


def random_mask_raster(H, W, density, seed):
    return rasters_of_mask(np.random.default_rng(seed).random((H, W)) < density, seed + 1)


def serpentine_mask(H, W):
    """One cell wide, winding through the whole raster: every even row, joined alternately at the right and the left end."""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    for k, i in enumerate(range(1, H, 2)):
        if i + 1 < H:
            m[i, W - 1 if k % 2 == 0 else 0] = True
    return m


def comb_mask(H, W):
    """A spine along the bottom row with a tooth on every even column, reaching up to the top row."""
    m = np.zeros((H, W), bool)
    m[H - 1] = True
    m[:, 0::2] = True
    return m


def checkerboard_mask(H, W):
    i, j = np.mgrid[0:H, 0:W]
    return (i + j) % 2 == 0


def rings_mask(H, W):
    """Nested square rings two cells thick and two cells apart around a 2 x 2 block: every ring has a hole that holds the next."""
    i, j = np.mgrid[0:H, 0:W]
    d = np.minimum(np.minimum(i, H - 1 - i), np.minimum(j, W - 1 - j))
    return (d // 2) % 2 == 0


ROOF_GSD = 0.5
ROOF_BOXES = ((20, 30, 30, 40, 6.0), (90, 20, 24, 50, 9.5), (150, 120, 16, 16, 3.0))       # row, column, rows, columns, metres
ROOF_GABLES = ((30, 110, 40, 32, 4.0), (100, 100, 30, 21, 5.0))                            # ..., eaves height; the ridge runs along rows
ROOF_CROWNS = ((70, 170, 9), (140, 40, 11), (170, 90, 8))                                  # row, column, radius in cells
ROOF_SMALL = ((10, 100, 5, 5, 4.0), (80, 100, 5, 6, 4.0), (180, 20, 6, 6, 7.0))            # below min_area = 40 cells, 5 wide or more
ROOF_NARROW = ((60, 60, 3, 30, 5.0), (185, 150, 12, 4, 5.0))                               # narrower than 2 r_open + 1 = 5 cells


def roof_scene(H=200, W=200, seed=4):
    """Boxes (flat roofs), gabled roofs (pitch 0.25 m per cell, the ridge along rows), noise "crowns" (discs whose heights
    are seeded multiples of 1/8 m in 6 .. 10 m), small boxes and narrow strips on a sloping plane, at gsd 0.5 m ->
    (dsm, ndsm, truth) with truth = dict(buildings=[(cells, height_mean, height_max), ...] in cell order, crowns, small,
    narrow as masks)."""
    i, j = np.mgrid[0:H, 0:W]
    plane = 40.0 + 0.125 * j + 0.25 * i
    nd = np.zeros((H, W), np.float64)
    truth = dict(buildings=[], crowns=np.zeros((H, W), bool), small=np.zeros((H, W), bool), narrow=np.zeros((H, W), bool))
    for i0, j0, h, w, dz in ROOF_BOXES:
        nd[i0:i0 + h, j0:j0 + w] = dz
        truth["buildings"].append((i0 * W + j0, h * w, dz, dz))
    for i0, j0, h, w, eaves in ROOF_GABLES:
        jj = np.arange(w)
        prof = eaves + 0.25 * np.minimum(jj, w - 1 - jj)
        nd[i0:i0 + h, j0:j0 + w] = prof[None, :]
        total = int(np.rint(prof * 1024.0).astype(np.int64).sum()) * h
        truth["buildings"].append((i0 * W + j0, h * w, total / 1024.0 / (h * w), float(prof.max())))
    rng = np.random.default_rng(seed)
    for ci, cj, rad in ROOF_CROWNS:
        disc = (i - ci) ** 2 + (j - cj) ** 2 <= rad * rad
        nd[disc] = (6.0 + rng.integers(0, 33, (H, W)) / 8.0)[disc]
        truth["crowns"] |= disc
    for key, items in (("small", ROOF_SMALL), ("narrow", ROOF_NARROW)):
        for i0, j0, h, w, dz in items:
            nd[i0:i0 + h, j0:j0 + w] = dz
            truth[key][i0:i0 + h, j0:j0 + w] = True
    truth["buildings"] = [b[1:] for b in sorted(truth["buildings"])]
    return (plane + nd).astype(np.float32), nd.astype(np.float32), truth
