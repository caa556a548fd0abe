"""The drainage network of the DTM (or of another height raster of the grid): fill, D8 directions, accumulation, basins, streams.

    python drainage_whu.py --dsm /out/predict/dsm [--source dtm|dsm|dsm_filled] [--min_area 1000.0] [--smooth_passes 1]
                           [--min_length 0.0] [--out PREFIX]

The second vector product of the terrain, next to the contour lines, after dtm_whu.py.  Read: `<PREFIX>_<source>.tif` and the grid
(`<PREFIX>_dsm.json`).  On the GPU (csrc/dsm_drainage.hip; include/adamvs_hip.h "Drainage" states the result operation by
operation): the contours' integer surface brought to 65536 units per metre, the depression-free surface F as the unique solution
of F = max(r, lowest neighbour + 1) with the cells at the edge of the data held at their height (one unit per step: no flat
survives), the D8 direction of every cell (steepest drop of F, diagonal against orthogonal compared exactly), the number of
cells that drain through every cell and the outlet each cell drains to by pointer doubling, the cells of the streams (at least
min_area upstream), their donors in closed form, every cell's link and position in it by list ranking, the link table and the
ordered cell lists.  On the host: the cell centres in float64, length, drop, upstream cells, Strahler order and Shreve magnitude
of every link, the catchments of the outlets that carry a stream numbered by cell index, the links shorter than min_length
dropped.  Written: `<out>_flowdir.tif` (uint8: the ESRI codes 1 E, 2 SE, 4 S, 8 SW, 16 W, 32 NW, 64 N, 128 NE, 0 at an outlet, 255
at no data), `<out>_flowacc.tif` (int32 cell counts), `<out>_sinkdepth.tif` (float32 metres, (F - r) / 65536 with the one-unit
steps left in, NaN at no data), `<out>_basins.tif` with its world file (int32, 0 outside the numbered catchments),
`<out>_streams.geojson` (one LineString per link, running downstream; properties id, strahler, magnitude, upstream_cells,
upstream_area_m2, length_m, drop_m, vertices, to_id (0 at an outlet), basin) and `<out>_drainage.json` (grid, source, parameters
with min_cells, counts, stats, seconds).  --out defaults to --dsm; no name collides with a file of an earlier stage.

Priority-flood, the topological walk of the accumulation and "follow the stream" are serial walks whose bookkeeping depends on
the visiting order; here every step is a definition that needs none, so the stage is exact in integers and bit-identical from
run to run.  The defaults (streams from 1000 m^2 upstream, one smoothing pass, no minimum length) are conventions.  They are not
values measured on WHU scenes, and no real-scene tuning has been done.

Limits.  D8 only: a cell drains to one neighbour, there are no multiple flow directions.  Outlets lie only at the edge of the
data (the border of the raster and the rim of every hole), so a true closed basin is filled up to its spill point.  The lines
run from cell centre to cell centre and are not smoothed, and the files carry no CRS.  |z - z_ref| of a cell must not exceed
8191 m.  min_area and min_length given as floats are taken as the decimal number they print as (0.1 is one tenth).
"""
import argparse
import json
import math
import time

import numpy as np

from . import raster_stage
from .contours import MAX_ABS_M, _exact, line_lengths
from .dsm import _check_gsd

UNITS = 65536                                       # ADAMVS_DRAIN_UNITS
TILE = 32                                           # ADAMVS_DRAIN_TILE
NO_DATA = -2 ** 31
SOURCES = ("dtm", "dsm", "dsm_filled")
DEFAULTS = dict(source="dtm", min_area=1000.0, smooth_passes=1, min_length=0.0)
PROPERTIES = ("id", "strahler", "magnitude", "upstream_cells", "upstream_area_m2", "length_m", "drop_m", "vertices", "to_id", "basin")
INT32_MAX = 2 ** 31 - 1


def parameters(gsd, min_area=DEFAULTS["min_area"], smooth_passes=DEFAULTS["smooth_passes"], min_length=DEFAULTS["min_length"], max_rounds=None):
    """The checked parameters; min_cells = ceil(min_area / gsd^2) in exact rationals, at least 1 and at most 2^31 - 1 (which no
    raster reaches).  Raises ValueError."""
    ma, ml = _exact(min_area, "min_area"), _exact(min_length, "min_length")
    g = _exact(_check_gsd(gsd), "gsd")
    if ma < 0:
        raise ValueError("min_area=%r must be >= 0" % (min_area,))
    if ml < 0:
        raise ValueError("min_length=%r must be >= 0" % (min_length,))
    if isinstance(smooth_passes, bool) or int(smooth_passes) != smooth_passes or not 0 <= int(smooth_passes) <= 2:
        raise ValueError("smooth_passes=%r must be 0, 1 or 2" % (smooth_passes,))
    if max_rounds is not None and (isinstance(max_rounds, bool) or int(max_rounds) != max_rounds or not 1 <= int(max_rounds) <= INT32_MAX):
        raise ValueError("max_rounds=%r must be an integer >= 1" % (max_rounds,))
    min_cells = min(max(1, math.ceil(ma / (g * g))), INT32_MAX)
    return dict(min_area=float(ma), smooth_passes=int(smooth_passes), min_length=float(ml), min_cells=int(min_cells),
                max_rounds=None if max_rounds is None else int(max_rounds))


# ---- the host's share ---------------------------------------------------------------------------------------------------
def cell_centres(cells, grid):
    """cells int [P] (indices i W + j) -> xy float64 [P, 2]: the centres."""
    cells = np.asarray(cells, np.int64).reshape(-1)
    i, j = cells // int(grid.W), cells % int(grid.W)
    return np.stack([grid.x0 + (j + 0.5) * grid.gsd, grid.y_top - (i + 0.5) * grid.gsd], axis=1)


def strahler(link_to, acc_head):
    """link_to int [L] (the link a link flows into, -1 for none), acc_head int [L] (acc of the links' heads) -> int64 [L]: 1 for a
    link nothing flows into; where links meet, the largest order, one more if two or more carry it.  One pass in ascending
    acc_head: what flows into a link has fewer cells upstream of its head."""
    link_to, acc_head = np.asarray(link_to, np.int64), np.asarray(acc_head, np.int64)
    L = link_to.size
    top, times = np.zeros(L, np.int64), np.zeros(L, np.int64)
    order = np.zeros(L, np.int64)
    for l in np.argsort(acc_head, kind="stable").tolist():
        o = 1 if times[l] == 0 else int(top[l]) + (1 if times[l] >= 2 else 0)
        order[l] = o
        t = int(link_to[l])
        if t >= 0:
            if o > top[t]:
                top[t], times[t] = o, 1
            elif o == top[t]:
                times[t] += 1
    return order


def link_properties(res, grid):
    """The per-link columns of the host: own_last (the last cell a link owns alone), length, drop, upstream_cells, magnitude,
    strahler, basin."""
    first, head, end, to, vertex = (np.asarray(res[k], np.int64) for k in ("link_first", "link_head", "link_end", "link_to", "vertex"))
    L = head.size
    flat = lambda k: np.asarray(res[k]).reshape(-1)
    owned = flat("link")[end] == np.arange(L) if L else np.zeros(0, bool)
    own_last = np.where(owned, end, vertex[np.maximum(first[1:] - 2, 0)]) if L else np.zeros(0, np.int64)
    xy = cell_centres(vertex, grid)
    F = flat("F").astype(np.int64)
    return dict(xy=xy, own_last=own_last, length=line_lengths(xy, first), drop=(F[head] - F[end]) / float(UNITS),
                upstream_cells=flat("acc")[own_last].astype(np.int64), magnitude=flat("magnitude")[own_last].astype(np.int64),
                strahler=strahler(to, flat("acc")[head]), basin=flat("basins")[head].astype(np.int64))


def features(res, cols, grid, min_length=DEFAULTS["min_length"]):
    """The links at least min_length long as a list of dict(properties, xy); a link's id is its number + 1 whether or not its
    neighbours were kept."""
    first, to = np.asarray(res["link_first"], np.int64), np.asarray(res["link_to"], np.int64)
    feats = []
    for l in np.flatnonzero(cols["length"] >= float(min_length)).tolist():
        p0, p1 = int(first[l]), int(first[l + 1])
        up = int(cols["upstream_cells"][l])
        props = dict(id=l + 1, strahler=int(cols["strahler"][l]), magnitude=int(cols["magnitude"][l]), upstream_cells=up,
                     upstream_area_m2=float(up * grid.gsd * grid.gsd), length_m=float(cols["length"][l]), drop_m=float(cols["drop"][l]),
                     vertices=p1 - p0, to_id=int(to[l]) + 1, basin=int(cols["basin"][l]))
        feats.append(dict(properties=props, xy=cols["xy"][p0:p1]))
    return feats


def geojson_text(feats):
    """A FeatureCollection of LineStrings: fixed key order and number formatting, equal inputs give equal bytes."""
    out = []
    for f in feats:
        props = {k: f["properties"][k] for k in PROPERTIES}
        coords = [[float(x), float(y)] for x, y in np.asarray(f["xy"], np.float64).tolist()]
        out.append(dict(type="Feature", properties=props, geometry=dict(type="LineString", coordinates=coords)))
    return json.dumps(dict(type="FeatureCollection", features=out), separators=(",", ":")) + "\n"


def sink_depth(r, F):
    """-> float32 [H, W]: (F - r) / 65536 metres, NaN at no data."""
    r, F = np.asarray(r, np.int64), np.asarray(F, np.int64)
    return np.where(r == NO_DATA, np.nan, (F - r) / float(UNITS)).astype(np.float32)


# ---- the stage ----------------------------------------------------------------------------------------------------------
def _no_gpu():
    return raster_stage.no_gpu("drainage", "drainage")


def route(z, gsd, z_ref=0.0, min_area=DEFAULTS["min_area"], smooth_passes=DEFAULTS["smooth_passes"], min_length=DEFAULTS["min_length"],
          max_rounds=None, grid=None, device=None):
    """z [H, W] float32 (host; NaN where there is no value) -> dict(s, r, F, dir, acc, root, nd, link, pos, link_first, link_head,
    link_end, link_to, vertex (all as the header names them, numpy), magnitude int32 [H, W] (the stream sources upstream), basins
    int32 [H, W], sinkdepth float32 [H, W], L, P, K (the numbered basins), xy float64 [P, 2], the per-link columns own_last,
    length, drop, upstream_cells, link_magnitude, strahler, basin, features, counts, stats, params, grid, seconds).  max_rounds caps
    the rounds of the fill (default: the number of cells, which no raster needs).  grid: the dsm.Grid the coordinates refer to
    (default: x0 = 0, y_top = H gsd).  Raises ValueError for bad parameters and for a finite height further than 8191 m from
    z_ref, RuntimeError if the fill hits the cap and without a GPU: there is no CPU fallback."""
    import torch
    from . import hip_ops
    p = parameters(gsd, min_area, smooth_passes, min_length, max_rounds)
    gsd = _check_gsd(gsd)
    z = np.ascontiguousarray(z, np.float32)
    if z.ndim != 2:
        raise ValueError("z %s must be [H, W]" % (z.shape,))
    if z.size >= 2 ** 30:
        raise ValueError("z %s: fewer than 2^30 cells can be routed" % (z.shape,))
    if not math.isfinite(float(z_ref)):
        raise ValueError("z_ref=%r must be finite" % (z_ref,))
    if not torch.cuda.is_available():
        raise _no_gpu()
    H, W = z.shape
    if grid is None:
        grid = raster_stage.default_grid(H, W, gsd, float(z_ref))
    cap = p["max_rounds"] if p["max_rounds"] is not None else min(H * W, INT32_MAX - 1) + 1
    dev = torch.device(device if device is not None else "cuda")
    zd = torch.from_numpy(z).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.time()
    s, info = hip_ops.contour_surface(zd, float(z_ref), p["smooth_passes"])
    out_of_range = int(info.cpu()[2])
    if out_of_range:
        raise ValueError("drainage: %d cells lie further than %d m from z_ref=%g" % (out_of_range, MAX_ABS_M, float(z_ref)))
    t1 = time.time()
    r, F, st_fill, ws = hip_ops.drain_fill(s, p["smooth_passes"], cap)
    if not st_fill["converged"]:
        raise RuntimeError("drainage: the fill was still moving after max_rounds=%d rounds" % cap)
    t2 = time.time()
    direction = hip_ops.drain_direction(F)
    torch.cuda.synchronize(dev)
    t3 = time.time()
    acc, root, st_acc, ws = hip_ops.drain_accumulate(direction, None, ws)
    t4 = time.time()
    number, n_outlets = hip_ops._number_roots(root)
    outlet = torch.nonzero(root.view(-1) == torch.arange(H * W, device=dev, dtype=torch.int32)).view(-1)
    keep = (acc.view(-1)[outlet] >= p["min_cells"]).cpu().numpy()
    basins = raster_stage.relabel_kept(number, keep)
    torch.cuda.synchronize(dev)
    t5 = time.time()
    nd, link, pos, L, P, st_str, ws = hip_ops.drain_streams(direction, acc, p["min_cells"], ws)
    table = hip_ops.drain_links(direction, nd, link, pos, L, P, ws)
    magnitude = hip_ops.drain_accumulate(direction, (nd == 0).to(torch.int32), ws)[0]
    res = dict(s=s, r=r, F=F, dir=direction, acc=acc, root=root, nd=nd, link=link, pos=pos, link_first=table[0], link_head=table[1],
               link_end=table[2], link_to=table[3], vertex=table[4], magnitude=magnitude, basins=basins)
    res = {k: v.cpu().numpy() for k, v in res.items()}
    t6 = time.time()
    cols = link_properties(res, grid)
    feats = features(res, cols, grid, p["min_length"])
    res["sinkdepth"] = sink_depth(res["r"], res["F"])
    t7 = time.time()
    valid = int((res["dir"] != 255).sum())
    counts = dict(valid=valid, outlets=int(n_outlets), basins=int(keep.sum()), filled=int((res["F"] > res["r"]).sum()),
                  stream_cells=int((res["nd"] != 255).sum()), links=L, vertices=P, kept=len(feats), rejected_short=L - len(feats),
                  max_strahler=int(cols["strahler"].max()) if L else 0, max_acc=int(res["acc"].max()) if valid else 0)
    stats = dict(fill=st_fill, accumulate=st_acc, streams=st_str)
    res.update(cols, link_magnitude=cols["magnitude"], magnitude=res["magnitude"], L=L, P=P, K=int(keep.sum()), features=feats, counts=counts,
               stats=stats, params=p, grid=grid, gsd=float(gsd), z_ref=float(z_ref),
               seconds=dict(surface=t1 - t0, fill=t2 - t1, direction=t3 - t2, accumulation=t4 - t3, basins=t5 - t4, streams=t6 - t5,
                            host=t7 - t6))
    return res


def from_dsm(prefix, source=DEFAULTS["source"], min_area=DEFAULTS["min_area"], smooth_passes=DEFAULTS["smooth_passes"],
             min_length=DEFAULTS["min_length"], max_rounds=None, device=None, out=None):
    """The raster `<prefix>_<source>.tif` of an earlier stage -> route()'s dict with `source` added; written to `out` (a path
    prefix) if given.  The heights are quantised about the grid's z_ref."""
    import torch
    if source not in SOURCES:
        raise ValueError("source=%r must be one of %s" % (source, ", ".join(SOURCES)))
    parameters(1.0, min_area, smooth_passes, min_length, max_rounds)            # what does not depend on the grid, before any file
    grid = raster_stage.read_grid(prefix)
    path = "%s_%s.tif" % (prefix, source)
    hint = {"dtm": "dtm_whu.py --dsm", "dsm": "dsm_whu.py --out", "dsm_filled": "dsm_whu.py --fill_max_dist .. --out"}
    raster_stage.require(path, "no such raster (run %s %s first)" % (hint[source], prefix))
    if not torch.cuda.is_available():
        raise _no_gpu()
    z = raster_stage.read_raster(path, np.float32, (grid.H, grid.W), says="the grid %d x %d" % (grid.H, grid.W))
    res = route(z, grid.gsd, grid.z_ref, min_area, smooth_passes, min_length, max_rounds, grid, device)
    res["source"] = dict(prefix=prefix, raster=source)
    if out is not None:
        write_outputs(out, res)
    return res


# ---- files --------------------------------------------------------------------------------------------------------------
def output_paths(out):
    """The files of this stage, disjoint from those of every earlier stage."""
    return dict(flowdir=out + "_flowdir.tif", flowacc=out + "_flowacc.tif", sinkdepth=out + "_sinkdepth.tif", label=out + "_basins.tif",
                label_world=out + "_basins.tfw", geojson=out + "_streams.geojson", json=out + "_drainage.json")


def summary(res):
    return dict(grid=raster_stage.grid_summary(res["grid"]), source=res.get("source"), params=dict(res["params"], z_ref=res["z_ref"]),
                counts=res["counts"], stats=res["stats"], seconds=res["seconds"])


def write_outputs(out, res):
    """The rasters, the GeoJSON file and the JSON summary at the path prefix `out` -> output_paths(out)."""
    from PIL import Image
    paths = raster_stage.write_outputs(output_paths(out), out, dict(geojson=geojson_text(res["features"])), summary(res), res["basins"],
                                       res["grid"])
    Image.fromarray(np.ascontiguousarray(res["dir"], np.uint8)).save(paths["flowdir"], format="TIFF")
    Image.fromarray(np.ascontiguousarray(res["acc"], np.int32)).save(paths["flowacc"], format="TIFF")
    Image.fromarray(np.ascontiguousarray(res["sinkdepth"], np.float32)).save(paths["sinkdepth"], format="TIFF")
    return paths


def read_outputs(out):
    """-> (basins int32, flowdir uint8, flowacc int32, sinkdepth float32, the streams as a dict, the summary as a dict) read back
    from write_outputs' files."""
    from PIL import Image
    paths = output_paths(out)
    basins, streams, js = raster_stage.read_outputs(paths, ("geojson",))
    return (basins, np.array(Image.open(paths["flowdir"]), np.uint8), np.array(Image.open(paths["flowacc"]), np.int32),
            np.array(Image.open(paths["sinkdepth"]), np.float32), streams, js)


def build_parser():
    ap = argparse.ArgumentParser(description="Derive the drainage network of the DTM: fill, D8 directions, accumulation, basins, streams")
    ap.add_argument("--dsm", required=True, metavar="PREFIX", help="path prefix of the earlier stages' output "
                    "(<PREFIX>_<source>.tif, <PREFIX>_dsm.json)")
    ap.add_argument("--source", choices=SOURCES, default=DEFAULTS["source"], help="the raster that is routed")
    ap.add_argument("--min_area", type=float, default=DEFAULTS["min_area"], help="least upstream area of a stream cell in square metres")
    ap.add_argument("--smooth_passes", type=int, default=DEFAULTS["smooth_passes"], help="3 x 3 binomial smoothing passes of the surface: 0, 1 or 2")
    ap.add_argument("--min_length", type=float, default=DEFAULTS["min_length"], help="least length of a written link in metres")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="output path prefix (default: --dsm): <out>_flowdir.tif, <out>_flowacc.tif, "
                    "<out>_sinkdepth.tif, <out>_basins.tif, <out>_streams.geojson, <out>_drainage.json")
    return ap


def main(argv=None):
    args, out, t0 = raster_stage.open_main(build_parser, argv)
    res = from_dsm(args.dsm, args.source, args.min_area, args.smooth_passes, args.min_length, out=out)
    g, c, s, st = res["grid"], res["counts"], res["seconds"], res["stats"]
    print("drainage %d x %d cells at gsd %g: %d valid cells, %d outlets, %d cells filled in %d rounds, %d stream cells (min_cells %d) in %d "
          "links up to order %d, %d basins" % (g.W, g.H, g.gsd, c["valid"], c["outlets"], c["filled"], st["fill"]["rounds"], c["stream_cells"],
                                                res["params"]["min_cells"], c["links"], c["max_strahler"], c["basins"]))
    print("%d links written, %d rejected as short; surface %.3f s, fill %.3f s, direction %.3f s, accumulation %.3f s, basins %.3f s, "
          "streams %.3f s, host %.3f s; total_time = %.3f s" % (c["kept"], c["rejected_short"], s["surface"], s["fill"], s["direction"],
                                                                 s["accumulation"], s["basins"], s["streams"], s["host"], time.time() - t0))
    return res


if __name__ == "__main__":
    main()
