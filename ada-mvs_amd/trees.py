"""Trees from the nDSM: tree tops by a height-dependent local-maximum filter, and the crown of every top as a labelled region with
its outline.

    python trees_whu.py --dsm /out/predict/dsm [--no_buildings] [--min_height 2.0] [--smooth_passes 1] [--radius_min 1.5]
                        [--radius_slope 0.05] [--crown_ratio 0.55] [--max_crown_radius 10.0] [--min_crown_area 1.0] [--out PREFIX]

The step after buildings_whu.py, independent of roofs_whu.py.  Read: the nDSM (`<PREFIX>_ndsm.tif`), the grid
(`<PREFIX>_dsm.json`) and the building labels (`<PREFIX>_buildings.tif`; --no_buildings does without them and excludes nothing).
Outside the buildings the nDSM is a canopy height model.  On the GPU (csrc/dsm_trees.hip; include/adamvs_hip.h "Trees" states the
result operation by operation): the canopy cells at least min_height above ground and off every building, their heights in
1/256 m smoothed by smooth_passes binomial passes, a window per cell whose radius radius_min + radius_slope * height grows with
the height, the tops (cells that nothing in their window beats), a parent for every canopy cell (its best neighbour if that is
higher, else the best cell of its window), the top every cell climbs to, and the crown of a top: the cells that climb to it, are
at least crown_ratio of its height and lie within max_crown_radius.  On the host: a tree is kept iff its crown covers
min_crown_area; the outlines run along cell edges.  Written: `<out>_trees.geojson` (one Point per tree at the centre of its top
cell; properties id, x, y, height_m, height_mean_m, crown_area_m2, crown_diameter_m, crown_radius_max_m, volume_m3, cells, parts,
window_cells), `<out>_crowns.geojson` (one MultiPolygon per tree, same order, same ids, same properties: one Polygon per
4-connected part of the crown, exterior ring counter-clockwise, holes clockwise), `<out>_trees.tif` (int32 crown labels, 0 = none),
`<out>_trees.tfw` and `<out>_trees.json`.  --out defaults to --dsm; no name collides with a file of an earlier stage.

The method is the classic pair restated so that nothing depends on a visiting order: the variable-window local-maximum filter
(Popescu & Wynne 2004) and marker-controlled crown growth limited by a height ratio and a radius (Dalponte & Coomes 2016).  The
defaults (min_height 2 m, one smoothing pass, radius 1.5 m + 0.05 height, crown_ratio 0.55, max_crown_radius 10 m, min_crown_area
1 m^2) are conventions of that literature.  They are not values measured on WHU scenes, and no real-scene tuning has been done.

Limits.  Any object of min_height that is not a building counts as canopy: a lorry, a wall, a building rejected as small.  A
window may reach across a gap in the canopy.  A crown may consist of several parts (`parts`); crowns are not regularised.
Nothing is classified by species.
"""
import argparse
import json
import math
import time
from fractions import Fraction

import numpy as np

from . import raster_stage
from .buildings import _groups, ring_area2, trace_rings
from .dsm import _check_gsd

MAX_RADIUS = 64                                     # ADAMVS_TREE_MAX_RADIUS, cells
Q_SCALE = 256                                       # ADAMVS_TREE_Q_SCALE
DEFAULTS = dict(min_height=2.0, smooth_passes=1, radius_min=1.5, radius_slope=0.05, crown_ratio=0.55, max_crown_radius=10.0,
                min_crown_area=1.0)
COLUMNS = ("cells", "q_sum", "q_max", "row_min", "row_max", "col_min", "col_max", "r2_max", "top", "s_top")


def _radius(s, gsd, radius_min, radius_slope, scale):
    """floor((radius_min + radius_slope s / scale) / gsd) in exact rationals, clamped below at 1."""
    return max(1, math.floor((Fraction(radius_min) + Fraction(radius_slope) * s / scale) / Fraction(gsd)))


def window_table(gsd, radius_min, radius_slope, smooth_passes, s_max):
    """-> [thr[1], ..., thr[r_cap]]: thr[r] is the smallest integer s >= 0 whose window radius (in cells, see _radius) is at least
    r; r_cap is the radius at s_max (1 for s_max < 0: no canopy).  Built with fractions.Fraction: no rounding anywhere."""
    scale = Q_SCALE * 16 ** int(smooth_passes)
    r_cap = _radius(max(int(s_max), 0), gsd, radius_min, radius_slope, scale)
    g, r0, slope = Fraction(gsd), Fraction(radius_min), Fraction(radius_slope)
    thr = []
    for r in range(1, r_cap + 1):
        need = r * g - r0                                            # radius_slope s / scale >= need
        # r = 1 is the clamp; beyond it need > 0 and r <= r_cap imply slope > 0
        thr.append(0 if r == 1 or need <= 0 else math.ceil(need * scale / slope))
    return thr


def parameters(gsd, min_height=DEFAULTS["min_height"], smooth_passes=DEFAULTS["smooth_passes"], radius_min=DEFAULTS["radius_min"],
               radius_slope=DEFAULTS["radius_slope"], crown_ratio=DEFAULTS["crown_ratio"], max_crown_radius=DEFAULTS["max_crown_radius"],
               min_crown_area=DEFAULTS["min_crown_area"], s_max=None):
    """The checked parameters with the integers derived from them: ratio_pm = round-half-even(crown_ratio 1000) and
    rc2 = floor((max_crown_radius / gsd)^2), both exact; with s_max (the largest smoothed height present, from the device) also
    r_cap, the window radius there in cells.  Raises ValueError."""
    gsd = _check_gsd(gsd)
    p = dict(min_height=float(min_height), radius_min=float(radius_min), radius_slope=float(radius_slope), crown_ratio=float(crown_ratio),
             max_crown_radius=float(max_crown_radius), min_crown_area=float(min_crown_area))
    for name, positive in (("min_height", True), ("radius_min", False), ("radius_slope", False), ("crown_ratio", False),
                           ("max_crown_radius", False), ("min_crown_area", False)):
        v = p[name]
        if not math.isfinite(v) or v < 0.0 or (positive and v == 0.0):
            raise ValueError("%s=%r must be finite and %s 0" % (name, v, ">" if positive else ">="))
    if p["crown_ratio"] > 1.0:
        raise ValueError("crown_ratio=%r is a fraction: 0 .. 1" % p["crown_ratio"])
    if isinstance(smooth_passes, bool) or int(smooth_passes) != smooth_passes or not 0 <= int(smooth_passes) <= 2:
        raise ValueError("smooth_passes=%r must be 0, 1 or 2" % (smooth_passes,))
    p["smooth_passes"] = int(smooth_passes)
    p["ratio_pm"] = int(round(Fraction(p["crown_ratio"]) * 1000))                # Fraction rounds half to even
    p["rc2"] = int(math.floor((Fraction(p["max_crown_radius"]) / Fraction(gsd)) ** 2))
    if p["rc2"] >= 2 ** 62:
        raise ValueError("max_crown_radius=%g m at gsd %g is out of range" % (p["max_crown_radius"], gsd))
    if s_max is not None:
        r_cap = _radius(max(int(s_max), 0), gsd, p["radius_min"], p["radius_slope"], Q_SCALE * 16 ** p["smooth_passes"])
        if r_cap > MAX_RADIUS:
            raise ValueError("radius_min=%g m + radius_slope=%g x %.2f m at gsd %g is a window of %d cells radius: at most %d"
                             % (p["radius_min"], p["radius_slope"], max(int(s_max), 0) / (Q_SCALE * 16 ** p["smooth_passes"]), gsd, r_cap,
                                MAX_RADIUS))
        p["r_cap"] = int(r_cap)
    return p


def window_cells(s, thr):
    """r(c) of step 4 for the integer heights s: the largest r with s >= thr[r]."""
    return np.searchsorted(np.asarray(thr, np.int64), np.asarray(s, np.int64), side="right").astype(np.int64)


# ---- selection ----------------------------------------------------------------------------------------------------------
def select(table, gsd, min_crown_area=DEFAULTS["min_crown_area"]):
    """table: dict of integer arrays [T] (COLUMNS) -> (keep bool [T], counts).  A top is a tree iff cells gsd^2 >=
    min_crown_area.  counts: tops, trees, rejected_small."""
    cells = np.asarray(table["cells"], np.int64)
    keep = cells.astype(np.float64) * (float(gsd) * float(gsd)) >= float(min_crown_area)
    return keep, dict(tops=int(cells.size), trees=int(keep.sum()), rejected_small=int((~keep).sum()))


# ---- vectorising --------------------------------------------------------------------------------------------------------
def _inside(ring, y, x):
    """Even-odd test of the point (y, x), which lies on no edge, against a ring of (row, column) corners."""
    n = 0
    for (r0, c0), (r1, c1) in zip(ring, ring[1:] + ring[:1]):
        if c0 == c1 and c0 < x and min(r0, r1) < y < max(r0, r1):
            n += 1
    return n % 2 == 1


def crown_polygons(label, grid):
    """label int32 [H, W] (0 = none; an id may have several 4-connected parts, and parts that touch at a corner stay apart) ->
    a list of dict(id, polygons), ascending id.  polygons: one list of rings per 4-connected part, ordered by the first vertex
    of the exterior ring; each the exterior ring (counter-clockwise in world coordinates), then its holes (clockwise) in the
    order of their smallest (row, column) corner.  A hole belongs to the exterior ring that contains its first vertex (the
    innermost such ring where parts are nested: the cell above that vertex is a cell of the part).  Rings are lists of (x, y)
    with the corner (i, j) at (x0 + j gsd, y_top - i gsd), the first vertex not repeated."""
    label = np.asarray(label)
    ids, boxes = _groups(label)
    res = []
    for k, (r0, r1, c0, c1) in zip(ids.tolist(), boxes.tolist()):
        rings = trace_rings(label[r0:r1 + 1, c0:c1 + 1] == k)       # ordered by first vertex
        outer = [r for r in rings if ring_area2(r) > 0]
        parts = [[r] for r in outer]
        for hole in (r for r in rings if ring_area2(r) < 0):
            y, x = hole[0][0] - 0.5, hole[0][1] + 0.5                 # the centre of the cell above the hole's first vertex
            owners = [n for n, r in enumerate(outer) if _inside(r, y, x)]
            if not owners:
                raise ValueError("label %d: a hole at corner %r lies in no exterior ring" % (k, (r0 + hole[0][0], c0 + hole[0][1])))
            parts[min(owners, key=lambda n: ring_area2(outer[n]))].append(hole)
        world = [[[(grid.x0 + (c0 + c) * grid.gsd, grid.y_top - (r0 + r) * grid.gsd) for r, c in ring] for ring in part] for part in parts]
        res.append(dict(id=k, polygons=world))
    return res


def feature_properties(table, keep, grid, thr, parts):
    """The properties of the kept trees, in order: id 1 .. K.  table: COLUMNS and q_top (q at the top cell); parts: the number
    of 4-connected parts per kept tree."""
    gsd = float(grid.gsd)
    radius = window_cells(table["s_top"], thr)
    props = []
    for b, k in enumerate(np.flatnonzero(keep).tolist(), start=1):
        cells, q_sum, top = int(table["cells"][k]), int(table["q_sum"][k]), int(table["top"][k])
        i, j = divmod(top, int(grid.W))
        area = cells * (gsd * gsd)
        props.append(dict(id=b, x=grid.x0 + (j + 0.5) * gsd, y=grid.y_top - (i + 0.5) * gsd, height_m=int(table["q_top"][k]) / Q_SCALE,
                          height_mean_m=q_sum / Q_SCALE / cells, crown_area_m2=area, crown_diameter_m=2.0 * math.sqrt(area / math.pi),
                          crown_radius_max_m=math.sqrt(int(table["r2_max"][k])) * gsd, volume_m3=q_sum / Q_SCALE * (gsd * gsd), cells=cells,
                          parts=int(parts[b - 1]), window_cells=int(radius[k])))
    return props


def points_geojson_text(props):
    """The tree tops as a FeatureCollection of Points: fixed key order and number formatting, equal inputs give equal bytes."""
    feats = [dict(type="Feature", properties=p, geometry=dict(type="Point", coordinates=[float(p["x"]), float(p["y"])])) for p in props]
    return json.dumps(dict(type="FeatureCollection", features=feats), separators=(",", ":")) + "\n"


def crowns_geojson_text(polys, props):
    """The crowns as a FeatureCollection of MultiPolygons, same order and ids as the points; every ring closed."""
    feats = []
    for poly, prop in zip(polys, props):
        assert poly["id"] == prop["id"]
        coords = [[[[float(x), float(y)] for x, y in ring + ring[:1]] for ring in part] for part in poly["polygons"]]
        feats.append(dict(type="Feature", properties=prop, geometry=dict(type="MultiPolygon", coordinates=coords)))
    return json.dumps(dict(type="FeatureCollection", features=feats), separators=(",", ":")) + "\n"


# ---- the stage ----------------------------------------------------------------------------------------------------------
def _no_gpu():
    return raster_stage.no_gpu("trees", "tree-detection")


def finish(label, table, keep, counts, grid, thr):
    """The host's share after the selection, common to detect() and to the restatement of the tests: label (final, 1 .. K) and
    the table -> (polygons, properties)."""
    polys = crown_polygons(label, grid)
    assert [p["id"] for p in polys] == list(range(1, counts["trees"] + 1))       # every kept tree owns at least its top
    props = feature_properties(table, keep, grid, thr, [len(p["polygons"]) for p in polys])
    return polys, props


def detect(ndsm, gsd, building=None, min_height=DEFAULTS["min_height"], smooth_passes=DEFAULTS["smooth_passes"],
           radius_min=DEFAULTS["radius_min"], radius_slope=DEFAULTS["radius_slope"], crown_ratio=DEFAULTS["crown_ratio"],
           max_crown_radius=DEFAULTS["max_crown_radius"], min_crown_area=DEFAULTS["min_crown_area"], grid=None, device=None):
    """ndsm [H, W] float32 (host; NaN where there is no value), building [H, W] int32 or None -> dict(label int32 (0 none, trees
    1 .. K), crowns int32 (every top's crown, 1 .. T), mask, q, s, parent, root, T, thr, table (dict of int64 arrays [T]: COLUMNS
    and q_top), keep bool [T], properties, polygons, counts (canopy, labelled, unassigned cells; tops, trees, rejected_small),
    stats (rounds, tops, candidates, window_cells), params, seconds).  grid: the dsm.Grid the coordinates refer to (default:
    x0 = 0, y_top = H gsd).  Raises without a GPU: there is no CPU fallback."""
    import torch
    from . import hip_ops
    p = parameters(gsd, min_height, smooth_passes, radius_min, radius_slope, crown_ratio, max_crown_radius, min_crown_area)
    ndsm = np.ascontiguousarray(ndsm, np.float32)
    if ndsm.ndim != 2:
        raise ValueError("ndsm %s must be [H, W]" % (ndsm.shape,))
    if building is not None:
        building = np.ascontiguousarray(building, np.int32)
        if building.shape != ndsm.shape:
            raise ValueError("ndsm %s and building %s must be one [H, W]" % (ndsm.shape, building.shape))
    if not torch.cuda.is_available():
        raise _no_gpu()
    H, W = ndsm.shape
    gsd = float(gsd)
    if grid is None:
        grid = raster_stage.default_grid(H, W, gsd)
    dev = torch.device(device if device is not None else "cuda")
    nd = torch.from_numpy(ndsm).to(dev)
    bd = None if building is None else torch.from_numpy(building).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.time()
    mask, q, s, s_max = hip_ops.tree_surface(nd, bd, p["min_height"], p["smooth_passes"])
    s_max = int(s_max.item())
    p = parameters(gsd, min_height, smooth_passes, radius_min, radius_slope, crown_ratio, max_crown_radius, min_crown_area, s_max=s_max)
    thr = window_table(gsd, p["radius_min"], p["radius_slope"], p["smooth_passes"], s_max)
    t1 = time.time()
    parent, st = hip_ops.tree_parents(s, thr)
    t2 = time.time()
    root, number, T, st = hip_ops.tree_roots(parent, stats=st)
    t3 = time.time()
    crowns, unassigned = hip_ops.tree_crowns(s, root, number, p["ratio_pm"], p["rc2"])
    tab = hip_ops.tree_table(crowns, q, s, root, T)
    q_top = q.view(-1)[tab[COLUMNS.index("top")]] if T else torch.zeros(0, device=dev, dtype=torch.int32)
    tab, q_top = tab.cpu().numpy(), q_top.cpu().numpy().astype(np.int64)
    t4 = time.time()
    table = {name: tab[k] for k, name in enumerate(COLUMNS)}
    table["q_top"] = q_top
    keep, counts = select(table, gsd, p["min_crown_area"])
    label = raster_stage.relabel_kept(crowns, keep).cpu().numpy()
    counts = dict(canopy=int(mask.sum()), labelled=int((crowns > 0).sum()), unassigned=int(unassigned.item()), **counts)
    t5 = time.time()
    polys, props = finish(label, table, keep, counts, grid, thr)
    t6 = time.time()
    return dict(label=label, crowns=crowns.cpu().numpy(), mask=mask.cpu().numpy(), q=q.cpu().numpy(), s=s.cpu().numpy(),
                parent=parent.cpu().numpy(), root=root.cpu().numpy(), T=T, thr=thr, s_max=s_max, table=table, keep=keep, properties=props,
                polygons=polys, counts=counts,
                stats=dict(rounds=int(st.rounds), tops=int(st.tops), candidates=int(st.candidates), window_cells=int(st.window_cells)),
                params=p, gsd=gsd, grid=grid,
                seconds=dict(surface=t1 - t0, parents=t2 - t1, roots=t3 - t2, crowns_table=t4 - t3, select=t5 - t4, vectorise=t6 - t5))


def from_dsm(prefix, no_buildings=False, min_height=DEFAULTS["min_height"], smooth_passes=DEFAULTS["smooth_passes"],
             radius_min=DEFAULTS["radius_min"], radius_slope=DEFAULTS["radius_slope"], crown_ratio=DEFAULTS["crown_ratio"],
             max_crown_radius=DEFAULTS["max_crown_radius"], min_crown_area=DEFAULTS["min_crown_area"], device=None, out=None):
    """The nDSM of dtm_whu.py at the path prefix and the building labels of buildings_whu.py next to it (none with
    `no_buildings`) -> detect()'s dict with `source` added; written to `out` (a path prefix) if given."""
    import torch
    grid = raster_stage.read_grid(prefix)
    npath, bpath = prefix + "_ndsm.tif", prefix + "_buildings.tif"
    raster_stage.require(npath, "no nDSM (run dtm_whu.py --dsm %s first)" % prefix)
    if not no_buildings:
        raster_stage.require(bpath, "no building labels (run buildings_whu.py --dsm %s first, or pass --no_buildings to exclude nothing)" % prefix)
    if not torch.cuda.is_available():
        raise _no_gpu()
    ndsm = raster_stage.read_raster(npath, np.float32, (grid.H, grid.W), says="the grid %d x %d" % (grid.H, grid.W))
    building = None
    if not no_buildings:
        building = raster_stage.read_raster(bpath, np.int32, ndsm.shape, says="the nDSM %s" % (ndsm.shape,))
    res = detect(ndsm, grid.gsd, building, min_height, smooth_passes, radius_min, radius_slope, crown_ratio, max_crown_radius, min_crown_area,
                 grid, device)
    res["source"] = dict(prefix=prefix, buildings=not no_buildings)
    if out is not None:
        write_outputs(out, res)
    return res


# ---- files --------------------------------------------------------------------------------------------------------------
def output_paths(out):
    """The files of this stage, disjoint from those of dsm_whu.py, its gap fill, dtm_whu.py, buildings_whu.py and roofs_whu.py."""
    return dict(points=out + "_trees.geojson", crowns=out + "_crowns.geojson", label=out + "_trees.tif", label_world=out + "_trees.tfw",
                json=out + "_trees.json")


def summary(res):
    params = dict(res["params"], thr=[int(v) for v in res["thr"]])
    return dict(grid=raster_stage.grid_summary(res["grid"]), source=res.get("source"), params=params, counts=res["counts"],
                jump_rounds=res["stats"]["rounds"], stats=res["stats"], seconds=res["seconds"])


def write_outputs(out, res):
    """The two GeoJSON files, the label raster, its world file and the JSON summary at the path prefix `out` -> output_paths(out)."""
    texts = dict(points=points_geojson_text(res["properties"]), crowns=crowns_geojson_text(res["polygons"], res["properties"]))
    return raster_stage.write_outputs(output_paths(out), out, texts, summary(res), res["label"], res["grid"])


def read_outputs(out):
    """-> (label int32, the points as a dict, the crowns as a dict, the summary as a dict) read back from write_outputs' files."""
    return raster_stage.read_outputs(output_paths(out), ("points", "crowns"))


def build_parser():
    ap = argparse.ArgumentParser(description="Detect trees on the nDSM and delineate their crowns")
    ap.add_argument("--dsm", required=True, metavar="PREFIX", help="path prefix of the earlier stages' output "
                    "(<PREFIX>_ndsm.tif, <PREFIX>_dsm.json, <PREFIX>_buildings.tif)")
    ap.add_argument("--no_buildings", action="store_true", help="do not read <PREFIX>_buildings.tif: no cell is excluded as a building")
    ap.add_argument("--min_height", type=float, default=DEFAULTS["min_height"], help="least canopy height above ground in metres")
    ap.add_argument("--smooth_passes", type=int, default=DEFAULTS["smooth_passes"], help="3 x 3 binomial smoothing passes: 0, 1 or 2")
    ap.add_argument("--radius_min", type=float, default=DEFAULTS["radius_min"], help="window radius in metres at height 0")
    ap.add_argument("--radius_slope", type=float, default=DEFAULTS["radius_slope"], help="growth of the window radius per metre of height")
    ap.add_argument("--crown_ratio", type=float, default=DEFAULTS["crown_ratio"], help="least height of a crown cell as a fraction of its top's")
    ap.add_argument("--max_crown_radius", type=float, default=DEFAULTS["max_crown_radius"], help="largest distance in metres of a crown cell from its top")
    ap.add_argument("--min_crown_area", type=float, default=DEFAULTS["min_crown_area"], help="least crown area of a tree in square metres")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="output path prefix (default: --dsm): <out>_trees.geojson, ...")
    return ap


def main(argv=None):
    args, out, t0 = raster_stage.open_main(build_parser, argv)
    res = from_dsm(args.dsm, args.no_buildings, args.min_height, args.smooth_passes, args.radius_min, args.radius_slope, args.crown_ratio,
                   args.max_crown_radius, args.min_crown_area, out=out)
    g, c, p, s, st = res["grid"], res["counts"], res["params"], res["seconds"], res["stats"]
    print("trees %d x %d cells at gsd %g: %d canopy cells, windows of 1 .. %d cells radius, %d window searches over %d cells"
          % (g.W, g.H, g.gsd, c["canopy"], p["r_cap"], st["candidates"], st["window_cells"]))
    print("%d tops (%d jump rounds): %d trees, %d rejected as small; %d crown cells, %d unassigned; surface %.3f s, parents %.3f s, "
          "roots %.3f s, crowns and table %.3f s, outlines %.3f s; total_time = %.3f s"
          % (c["tops"], st["rounds"], c["trees"], c["rejected_small"], c["labelled"], c["unassigned"], s["surface"], s["parents"], s["roots"],
             s["crowns_table"], s["vectorise"], time.time() - t0))
    return res


if __name__ == "__main__":
    main()
