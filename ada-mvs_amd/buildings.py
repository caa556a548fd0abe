"""Building footprints from the nDSM: labelled components of the tall, wide and flat cells, and their outlines as polygons.

    python buildings_whu.py --dsm /out/predict/dsm [--filled] [--min_height 2.5] [--min_width 2.0] [--smooth_span 1.0]
                            [--smooth_tol 0.2] [--min_smooth 0.5] [--min_area 10] [--simplify_tol METRES] [--out PREFIX]

The step after dtm_whu.py.  Read: the DSM (`<PREFIX>_dsm.tif`, or `<PREFIX>_dsm_filled.tif` with --filled), the nDSM
(`<PREFIX>_ndsm.tif`) and the grid (`<PREFIX>_dsm.json`).  On the GPU (csrc/dsm_buildings.hip; include/adamvs_hip.h "Building
extraction" states the result operation by operation): the cells at least min_height above ground, opened with a square of
min_width, flagged smooth / rough by the second difference of the DSM across smooth_span, grouped into 4-connected components
and summarised per component.  On the host: a component is a building iff it covers min_area and at least min_smooth of its
flagged cells are smooth (roofs are planar, crowns are not); the outlines of the buildings run along cell edges.  Written:
`<out>_buildings.geojson` (one Polygon per building: the exterior ring counter-clockwise, then the holes clockwise, RFC 7946
order, in the world coordinates of the grid; properties id, cells, area_m2, height_mean, height_max, smooth_fraction, bbox),
`<out>_buildings.tif` (int32 labels, 0 = no building), `<out>_buildings.tfw` and `<out>_buildings.json`.  --out defaults to
--dsm; none of the names collides with a file of dsm_whu.py, its gap fill or dtm_whu.py.

With --simplify_tol > 0 every ring is reduced by Douglas-Peucker (start vertex fixed, a subset of the vertices, never below
three distinct ones, every dropped vertex within the tolerance of the result); rings simplified that way may cross themselves
or each other.  The default 0 keeps the exact outlines.

The defaults (min_height 2.5 m, min_width 2.0 m, smooth_span 1.0 m, smooth_tol 0.2 m, min_smooth 0.5, min_area 10 m^2) are
conventions from the building-extraction literature.  They are not values measured on WHU scenes, and no real-scene tuning has
been done.
"""
import argparse
import json
import math
import time

import numpy as np

from . import raster_stage
from .dsm import _check_gsd

MAX_RADIUS = 1024                                   # ADAMVS_DTM_MAX_RADIUS: the opening, cells
MAX_STRIDE = 64                                     # ADAMVS_BLD_MAX_STRIDE, cells
DEFAULTS = dict(min_height=2.5, min_width=2.0, smooth_span=1.0, smooth_tol=0.2, min_smooth=0.5, min_area=10.0)
COLUMNS = ("cells", "smooth", "rough", "undetermined", "row_min", "row_max", "col_min", "col_max", "height_sum", "height_max_bits")


def parameters(gsd, min_height=DEFAULTS["min_height"], min_width=DEFAULTS["min_width"], smooth_span=DEFAULTS["smooth_span"],
               smooth_tol=DEFAULTS["smooth_tol"], min_smooth=DEFAULTS["min_smooth"], min_area=DEFAULTS["min_area"]):
    """The checked parameters with the two cell counts derived from them: r_open = floor(min_width / (2 gsd)) and
    stride = max(1, round(smooth_span / gsd)) (round half to even).  Raises ValueError."""
    gsd = _check_gsd(gsd)
    p = dict(min_height=float(min_height), min_width=float(min_width), smooth_span=float(smooth_span), smooth_tol=float(smooth_tol),
             min_smooth=float(min_smooth), min_area=float(min_area))
    for name, positive in (("min_height", True), ("min_width", False), ("smooth_span", True), ("smooth_tol", False), ("min_smooth", False),
                           ("min_area", False)):
        v = p[name]
        if not math.isfinite(v) or v < 0.0 or (positive and v == 0.0):
            raise ValueError("%s=%r must be finite and %s 0" % (name, v, ">" if positive else ">="))
    if p["min_smooth"] > 1.0:
        raise ValueError("min_smooth=%r is a fraction: 0 .. 1" % p["min_smooth"])
    r_open = math.floor(p["min_width"] / (2.0 * gsd))
    if r_open > MAX_RADIUS:
        raise ValueError("min_width=%g m at gsd %g opens with %d cells: at most %d" % (p["min_width"], gsd, r_open, MAX_RADIUS))
    stride = max(1, int(round(p["smooth_span"] / gsd)))
    if stride > MAX_STRIDE:
        raise ValueError("smooth_span=%g m at gsd %g is %d cells: at most %d" % (p["smooth_span"], gsd, stride, MAX_STRIDE))
    p.update(r_open=int(r_open), stride=int(stride))
    return p


# ---- selection ----------------------------------------------------------------------------------------------------------
def select(table, gsd, min_area=DEFAULTS["min_area"], min_smooth=DEFAULTS["min_smooth"]):
    """table: dict of integer arrays [N] (COLUMNS) -> (keep bool [N], counts).  A component is a building iff
    cells gsd^2 >= min_area and smooth >= min_smooth (smooth + rough); one with smooth + rough == 0 passes the second test
    only if min_smooth == 0.  counts: components, buildings, rejected_small (the area test fails), rejected_rough (the area
    test passes, the smoothness test fails)."""
    cells = np.asarray(table["cells"], np.int64)
    smooth, rough = np.asarray(table["smooth"], np.int64), np.asarray(table["rough"], np.int64)
    big = cells.astype(np.float64) * (float(gsd) * float(gsd)) >= float(min_area)
    flagged = smooth + rough
    flat = np.where(flagged > 0, smooth.astype(np.float64) >= float(min_smooth) * flagged.astype(np.float64), float(min_smooth) == 0.0)
    keep = big & flat
    counts = dict(components=int(cells.size), buildings=int(keep.sum()), rejected_small=int((~big).sum()), rejected_rough=int((big & ~flat).sum()))
    return keep, counts


def relabel(label, keep):
    """label int32 [H, W] (0 .. N), keep bool [N] -> the final labels: kept components renumbered 1 .. B in the same order."""
    keep = np.asarray(keep, bool)
    lut = np.zeros(keep.size + 1, np.int32)
    lut[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    return lut[np.asarray(label)]


# ---- vectorising --------------------------------------------------------------------------------------------------------
# Corners are (row, column) of the cell grid: cell (i, j) has the corners (i, j) .. (i + 1, j + 1).  Rows run south, so a ring
# that is counter-clockwise in world coordinates (x east, y north) keeps its interior on the left when walked with the
# directions below: E along a bottom edge, N along a right edge, W along a top edge, S along a left edge.
_DIRS = ((0, 1), (-1, 0), (0, -1), (1, 0))          # E, N, W, S as (d row, d column); (d + 1) % 4 is the left turn


def trace_rings(mask):
    """mask bool [h, w] -> the boundary rings of its cells as lists of (row, column) corners: vertices only where the direction
    changes, the first vertex not repeated at the end, each ring starting at its smallest (row, column) corner; interior on
    the left (see above), so outer boundaries have a positive world area and holes a negative one.  At a corner where four
    boundary edges meet the ring turns left: it stays with its own cell and does not join the two diagonal cells, so a ring
    may touch itself at a vertex and never crosses.  Rings are ordered by their first vertex."""
    m = np.pad(np.asarray(mask, bool), 1)
    core = m[1:-1, 1:-1]
    h, w = core.shape
    out = np.zeros((4, h + 1, w + 1), bool)           # out[d, r, c]: a boundary edge leaves corner (r, c) in direction d
    out[0, 1:, :-1] = core & ~m[2:, 1:-1]             # bottom edge, eastwards from (i + 1, j)
    out[1, 1:, 1:] = core & ~m[1:-1, 2:]              # right edge, northwards from (i + 1, j + 1)
    out[2, :-1, 1:] = core & ~m[:-2, 1:-1]            # top edge, westwards from (i, j + 1)
    out[3, :-1, :-1] = core & ~m[1:-1, :-2]           # left edge, southwards from (i, j)
    edges = {(int(r), int(c), int(d)) for d, r, c in zip(*np.nonzero(out))}
    rings = []
    for start in sorted(edges):
        if start not in edges:
            continue
        ring = []
        r, c, d = start
        prev = None
        while (r, c, d) in edges:
            edges.remove((r, c, d))
            if d != prev:
                ring.append((r, c))
            prev = d
            r, c = r + _DIRS[d][0], c + _DIRS[d][1]
            for nd in ((d + 1) % 4, d, (d + 3) % 4):                 # left, straight, right
                if (r, c, nd) in edges:
                    d = nd
                    break
        # the walk began at the ring's smallest corner, which is a vertex: the edge that closes the ring arrives there
        # in another direction than the first one leaves it
        assert (r, c) == ring[0] and len(ring) >= 4 and prev != start[2]
        rings.append(ring)
    return rings


def ring_area2(ring):
    """Twice the signed area of a ring of (row, column) corners in world orientation (x = column, y = -row), an integer."""
    a = 0
    for (r0, c0), (r1, c1) in zip(ring, ring[1:] + ring[:1]):
        a += c0 * (-r1) - c1 * (-r0)
    return a


def _point_segment(p, a, b):
    (px, py), (ax, ay), (bx, by) = p, a, b
    dx, dy = bx - ax, by - ay
    L = dx * dx + dy * dy
    t = 0.0 if L == 0.0 else min(1.0, max(0.0, ((px - ax) * dx + (py - ay) * dy) / L))
    return math.hypot(px - (ax + t * dx), py - (ay + t * dy))


def simplify_ring(ring, tol):
    """Douglas-Peucker on a closed ring of (x, y) vertices (the first not repeated at the end).  The start vertex stays; the
    ring is split at the vertex farthest from it, and both halves are reduced with the distance to the chord as a segment.
    The result is a subset of the vertices in their order; every dropped vertex lies within tol of it; a ring is never
    reduced below three distinct vertices (the vertex farthest from the remaining chord comes back).  tol <= 0: the ring."""
    ring = [tuple(p) for p in ring]
    n = len(ring)
    if not tol > 0.0 or n <= 3:
        return list(ring)
    far = max(range(1, n), key=lambda k: (math.hypot(ring[k][0] - ring[0][0], ring[k][1] - ring[0][1]), -k))
    pts = ring + [ring[0]]
    keep = {0, far, n}
    stack = [(0, far), (far, n)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        k = max(range(a + 1, b), key=lambda q: (_point_segment(pts[q], pts[a], pts[b]), -q))
        if _point_segment(pts[k], pts[a], pts[b]) > tol:
            keep.add(k)
            stack += [(a, k), (k, b)]
    keep.discard(n)
    if len({ring[k] for k in keep}) < 3:
        rest = [k for k in range(n) if ring[k] not in {ring[q] for q in keep}]
        keep.add(max(rest, key=lambda q: (_point_segment(ring[q], ring[0], ring[far]), -q)))
    return [ring[k] for k in sorted(keep)]


def _groups(label):
    """-> (ids ascending, per id (row_min, row_max, col_min, col_max)) of the non-zero labels."""
    label = np.asarray(label)
    idx = np.flatnonzero(label)
    if idx.size == 0:
        return np.zeros(0, np.int64), np.zeros((0, 4), np.int64)
    lab = label.reshape(-1)[idx]
    order = np.argsort(lab, kind="stable")              # within an id the cells stay in row-major order
    lab, idx = lab[order], idx[order]
    first = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
    last = np.r_[first[1:], lab.size] - 1
    rows, cols = idx // label.shape[1], idx % label.shape[1]
    box = np.stack([rows[first], rows[last], np.minimum.reduceat(cols, first), np.maximum.reduceat(cols, first)], 1)
    return lab[first].astype(np.int64), box.astype(np.int64)


def polygons(label, grid, simplify_tol=0.0):
    """label int32 [H, W] (0 = none; every id one 4-connected component), grid (x0, y_top, gsd as attributes) -> a list of
    dict(id, rings), ascending id.  rings: the exterior ring first (counter-clockwise in world coordinates), then the holes
    (clockwise) in the order of their smallest (row, column) corner; each a list of (x, y) with the corner (i, j) at
    (x0 + j gsd, y_top - i gsd), the first vertex not repeated."""
    label = np.asarray(label)
    ids, boxes = _groups(label)
    res = []
    for k, (r0, r1, c0, c1) in zip(ids.tolist(), boxes.tolist()):
        rings = trace_rings(label[r0:r1 + 1, c0:c1 + 1] == k)
        outer = [r for r in rings if ring_area2(r) > 0]
        if len(outer) != 1:
            raise ValueError("label %d is not one 4-connected component: %d outer boundaries" % (k, len(outer)))
        world = []
        for ring in outer + [r for r in rings if ring_area2(r) < 0]:
            pts = [(grid.x0 + (c0 + c) * grid.gsd, grid.y_top - (r0 + r) * grid.gsd) for r, c in ring]
            world.append(simplify_ring(pts, simplify_tol))
        res.append(dict(id=k, rings=world))
    return res


def feature_properties(table, keep, grid):
    """The properties of the kept components, in order: id 1 .. B."""
    gsd = float(grid.gsd)
    props = []
    for b, k in enumerate(np.flatnonzero(keep).tolist(), start=1):
        cells, smooth, rough = int(table["cells"][k]), int(table["smooth"][k]), int(table["rough"][k])
        r0, r1, c0, c1 = (int(table[n][k]) for n in ("row_min", "row_max", "col_min", "col_max"))
        top = np.array([int(table["height_max_bits"][k])], np.uint32).view(np.float32)[0]
        props.append(dict(id=b, cells=cells, area_m2=cells * (gsd * gsd), height_mean=int(table["height_sum"][k]) / 1024.0 / cells,
                          height_max=float(top), smooth_fraction=(smooth / (smooth + rough) if smooth + rough else None),
                          bbox=[grid.x0 + c0 * gsd, grid.y_top - (r1 + 1) * gsd, grid.x0 + (c1 + 1) * gsd, grid.y_top - r0 * gsd]))
    return props


def geojson_text(polys, props):
    """The FeatureCollection as text: one Polygon per building, every ring closed (the first vertex repeated), fixed key order
    and number formatting, so that equal inputs give equal bytes."""
    feats = []
    for poly, prop in zip(polys, props):
        assert poly["id"] == prop["id"]
        coords = [[[float(x), float(y)] for x, y in ring + ring[:1]] for ring in poly["rings"]]
        feats.append(dict(type="Feature", properties=prop, geometry=dict(type="Polygon", coordinates=coords)))
    return json.dumps(dict(type="FeatureCollection", features=feats), separators=(",", ":")) + "\n"


# ---- the stage ----------------------------------------------------------------------------------------------------------
def _no_gpu():
    return raster_stage.no_gpu("buildings", "building-extraction")


def extract(dsm, ndsm, gsd, min_height=DEFAULTS["min_height"], min_width=DEFAULTS["min_width"], smooth_span=DEFAULTS["smooth_span"],
            smooth_tol=DEFAULTS["smooth_tol"], min_smooth=DEFAULTS["min_smooth"], min_area=DEFAULTS["min_area"], simplify_tol=0.0,
            grid=None, device=None):
    """dsm, ndsm [H, W] float32 (host; NaN where there is no value) -> dict(label int32 (0 none, buildings 1 .. B), components
    int32 (every component of the mask, 1 .. N), flags uint8, table (dict of int64 arrays [N], COLUMNS), keep bool [N],
    properties, polygons, counts (candidate, opened_away, undetermined, smooth, rough cells; components, buildings,
    rejected_small, rejected_rough), label_stats (rounds, tiles, pairs), params, seconds).  grid: the dsm.Grid the polygons'
    coordinates refer to (default: x0 = 0, y_top = H gsd).  Raises without a GPU: there is no CPU fallback."""
    import torch
    from . import hip_ops
    p = parameters(gsd, min_height, min_width, smooth_span, smooth_tol, min_smooth, min_area)
    simplify_tol = float(simplify_tol)
    if not (math.isfinite(simplify_tol) and simplify_tol >= 0.0):
        raise ValueError("simplify_tol=%r must be finite and >= 0" % simplify_tol)
    dsm, ndsm = np.ascontiguousarray(dsm, np.float32), np.ascontiguousarray(ndsm, np.float32)
    if dsm.ndim != 2 or dsm.shape != ndsm.shape:
        raise ValueError("dsm %s and ndsm %s must be one [H, W]" % (dsm.shape, ndsm.shape))
    if not torch.cuda.is_available():
        raise _no_gpu()
    H, W = dsm.shape
    gsd = float(gsd)
    if grid is None:
        grid = raster_stage.default_grid(H, W, gsd)
    dev = torch.device(device if device is not None else "cuda")
    d, nd = torch.from_numpy(dsm).to(dev), torch.from_numpy(ndsm).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.time()
    flags = hip_ops.bld_flags(d, nd, p["min_height"], p["r_open"], p["stride"], p["smooth_tol"])
    torch.cuda.synchronize(dev)
    t1 = time.time()
    comp, N, st = hip_ops.bld_label(flags)
    t2 = time.time()
    tab = hip_ops.bld_table(flags, nd, comp, N).cpu().numpy()
    t3 = time.time()
    table = {name: tab[k] for k, name in enumerate(COLUMNS)}
    keep, counts = select(table, gsd, p["min_area"], p["min_smooth"])
    label = raster_stage.relabel_kept(comp, keep).cpu().numpy()
    flags = flags.cpu().numpy()
    hist = np.bincount(flags.reshape(-1), minlength=5)
    counts = dict(candidate=int(hist[1:].sum()), opened_away=int(hist[1]), undetermined=int(hist[2]), smooth=int(hist[3]), rough=int(hist[4]),
                  **counts)
    t4 = time.time()
    polys = polygons(label, grid, simplify_tol)
    props = feature_properties(table, keep, grid)
    t5 = time.time()
    p["simplify_tol"] = simplify_tol
    return dict(label=label, components=comp.cpu().numpy(), flags=flags, table=table, keep=keep, properties=props, polygons=polys,
                counts=counts, label_stats=dict(rounds=int(st.rounds), tiles=int(st.tiles), pairs=int(st.pairs)), params=p, gsd=gsd, grid=grid,
                seconds=dict(flags=t1 - t0, label=t2 - t1, table=t3 - t2, select=t4 - t3, vectorise=t5 - t4))


def from_dsm(prefix, filled=False, min_height=DEFAULTS["min_height"], min_width=DEFAULTS["min_width"], smooth_span=DEFAULTS["smooth_span"],
             smooth_tol=DEFAULTS["smooth_tol"], min_smooth=DEFAULTS["min_smooth"], min_area=DEFAULTS["min_area"], simplify_tol=0.0,
             device=None, out=None):
    """The DSM of dsm_whu.py at the path prefix (its gap-filled raster if `filled`) and the nDSM of dtm_whu.py next to it ->
    extract()'s dict with `source` added; written to `out` (a path prefix) if given."""
    import torch
    from .ortho import read_dsm
    if not torch.cuda.is_available():
        raise _no_gpu()
    dsm, grid = read_dsm(prefix, filled)
    ndsm = raster_stage.read_raster(prefix + "_ndsm.tif", np.float32, dsm.shape, "no nDSM (run dtm_whu.py --dsm %s first)" % prefix,
                                    "the DSM %s" % (dsm.shape,))
    res = extract(dsm, ndsm, grid.gsd, min_height, min_width, smooth_span, smooth_tol, min_smooth, min_area, simplify_tol, grid, device)
    res["source"] = dict(prefix=prefix, filled=bool(filled))
    if out is not None:
        write_outputs(out, res)
    return res


# ---- files --------------------------------------------------------------------------------------------------------------
def output_paths(out):
    """The files of this stage, disjoint from dsm.output_paths(out), dsm.fill_output_paths(out) and dtm.output_paths(out)."""
    return dict(geojson=out + "_buildings.geojson", label=out + "_buildings.tif", label_world=out + "_buildings.tfw",
                json=out + "_buildings.json")


def summary(res):
    return dict(grid=raster_stage.grid_summary(res["grid"]), source=res.get("source"), params=res["params"],
                counts=res["counts"], label_stats=res["label_stats"], seconds=res["seconds"])


def write_outputs(out, res):
    """The GeoJSON, the label raster, its world file and the JSON summary at the path prefix `out` -> output_paths(out)."""
    return raster_stage.write_outputs(output_paths(out), out, dict(geojson=geojson_text(res["polygons"], res["properties"])), summary(res),
                                      res["label"], res["grid"])


def read_outputs(out):
    """-> (label int32, the GeoJSON as a dict, the summary as a dict) read back from the files of write_outputs."""
    return raster_stage.read_outputs(output_paths(out), ("geojson",))


def build_parser():
    ap = argparse.ArgumentParser(description="Extract building footprints from the nDSM as polygons")
    ap.add_argument("--dsm", required=True, metavar="PREFIX", help="path prefix of dsm_whu.py's and dtm_whu.py's output "
                    "(<PREFIX>_dsm.tif, <PREFIX>_ndsm.tif, <PREFIX>_dsm.json)")
    ap.add_argument("--filled", action="store_true", help="use <PREFIX>_dsm_filled.tif (dsm_whu.py --fill_max_dist), as dtm_whu.py --filled did")
    ap.add_argument("--min_height", type=float, default=DEFAULTS["min_height"], help="least height above ground in metres")
    ap.add_argument("--min_width", type=float, default=DEFAULTS["min_width"], help="objects narrower than this many metres are opened away")
    ap.add_argument("--smooth_span", type=float, default=DEFAULTS["smooth_span"], help="half length in metres of the second difference of the DSM")
    ap.add_argument("--smooth_tol", type=float, default=DEFAULTS["smooth_tol"], help="largest second difference in metres of a smooth cell")
    ap.add_argument("--min_smooth", type=float, default=DEFAULTS["min_smooth"], help="least fraction of smooth cells among the smooth and rough ones")
    ap.add_argument("--min_area", type=float, default=DEFAULTS["min_area"], help="least area of a building in square metres")
    ap.add_argument("--simplify_tol", type=float, default=0.0, metavar="METRES",
                    help="Douglas-Peucker tolerance per ring (default 0: exact outlines; simplified rings may cross)")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="output path prefix (default: --dsm): <out>_buildings.geojson, ...")
    return ap


def main(argv=None):
    args, out, t0 = raster_stage.open_main(build_parser, argv)
    res = from_dsm(args.dsm, args.filled, args.min_height, args.min_width, args.smooth_span, args.smooth_tol, args.min_smooth, args.min_area,
                   args.simplify_tol, out=out)
    g, c, p, s = res["grid"], res["counts"], res["params"], res["seconds"]
    print("buildings %d x %d cells at gsd %g: opening %d cells, stride %d cells; %d candidate cells, %d opened away, %d smooth, %d rough, "
          "%d undetermined" % (g.W, g.H, g.gsd, p["r_open"], p["stride"], c["candidate"], c["opened_away"], c["smooth"], c["rough"], c["undetermined"]))
    print("%d components (%d border rounds): %d buildings, %d rejected as small, %d as rough; flags %.3f s, labels %.3f s, table %.3f s, "
          "outlines %.3f s; total_time = %.3f s" % (c["components"], res["label_stats"]["rounds"], c["buildings"], c["rejected_small"],
                                                    c["rejected_rough"], s["flags"], s["label"], s["table"], s["vectorise"], time.time() - t0))
    return res


if __name__ == "__main__":
    main()
