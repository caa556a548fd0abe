"""Contour lines of the DTM (or of another height raster of the grid) as ordered polylines.

    python contours_whu.py --dsm /out/predict/dsm [--source dtm|dsm|dsm_filled|ndsm] [--interval 1.0] [--base 0.0] [--major_every 5]
                           [--smooth_passes 1] [--min_length 0.0] [--out PREFIX]

The vector product of the terrain, after dtm_whu.py and independent of the object stages.  Read: `<PREFIX>_<source>.tif` and the
grid (`<PREFIX>_dsm.json`).  On the GPU (csrc/dsm_contours.hip; include/adamvs_hip.h "Contours" states the result operation by
operation): the heights above z_ref in 1/256 m smoothed by smooth_passes binomial passes, the segments of marching squares at
every level base + n interval that the surface reaches (a saddle is decided by the mean of its four corners), the successor and
predecessor of every segment in closed form, the position of every segment in its line by list ranking (open lines start where
they enter the data, rings at their smallest segment), the line table and one exact rational vertex per crossing.  On the host:
the coordinates in float64, the length of every line, the lines shorter than min_length dropped.  Written:
`<out>_contours.geojson` (one LineString per line, ordered by level and then by line number; properties id, elevation_m, level,
major, closed, vertices, length_m; a closed line repeats its first vertex; the higher ground is on the left of a line) and
`<out>_contours.json` (grid, source, parameters with the level table, counts, stats, seconds).  --out defaults to --dsm; no name
collides with a file of an earlier stage.

The usual "follow the line from cell to cell" is a serial walk whose output depends on the visiting order; here every step is a
definition that needs none.  The defaults (interval 1 m from base 0, every fifth line major, one smoothing pass, no minimum
length) are conventions of topographic mapping.  They are not values measured on WHU scenes, and no real-scene tuning has been
done.

Limits.  The lines are not simplified or smoothed (the smoothing belongs to the surface), carry no labels or depression marks,
are not clipped at buildings, and the files carry no CRS.  |z - z_ref| of a cell must not exceed 8191 m.  interval, base and
min_length given as floats are taken as the decimal number they print as (0.1 is one tenth).
"""
import argparse
import json
import math
import time
from fractions import Fraction

import numpy as np

from . import raster_stage
from .dsm import _check_gsd

Q_SCALE = 256                                       # ADAMVS_CONTOUR_Q_SCALE
MAX_LEVELS = 4096                                   # ADAMVS_CONTOUR_MAX_LEVELS
MAX_ABS_M = 8191                                    # ADAMVS_CONTOUR_MAX_ABS_M
SOURCES = ("dtm", "dsm", "dsm_filled", "ndsm")
DEFAULTS = dict(source="dtm", interval=1.0, base=0.0, major_every=5, smooth_passes=1, min_length=0.0)
PROPERTIES = ("id", "elevation_m", "level", "major", "closed", "vertices", "length_m")


def _exact(v, name):
    """v as a Fraction: a float stands for the decimal number it prints as, so that 0.1 is one tenth."""
    if isinstance(v, bool):
        raise ValueError("%s=%r must be a number" % (name, v))
    if isinstance(v, (int, Fraction)):
        return Fraction(v)
    f = float(v)
    if not math.isfinite(f):
        raise ValueError("%s=%r must be finite" % (name, v))
    return Fraction(repr(f))


def parameters(interval=DEFAULTS["interval"], base=DEFAULTS["base"], major_every=DEFAULTS["major_every"], smooth_passes=DEFAULTS["smooth_passes"],
               min_length=DEFAULTS["min_length"]):
    """The checked parameters; `scale` = 256 16^smooth_passes, the units of the integer surface per metre.  Raises ValueError."""
    iv, b, ml = _exact(interval, "interval"), _exact(base, "base"), _exact(min_length, "min_length")
    if iv <= 0:
        raise ValueError("interval=%r must be > 0" % (interval,))
    if ml < 0:
        raise ValueError("min_length=%r must be >= 0" % (min_length,))
    if isinstance(major_every, bool) or int(major_every) != major_every or int(major_every) < 1:
        raise ValueError("major_every=%r must be an integer >= 1" % (major_every,))
    if isinstance(smooth_passes, bool) or int(smooth_passes) != smooth_passes or not 0 <= int(smooth_passes) <= 2:
        raise ValueError("smooth_passes=%r must be 0, 1 or 2" % (smooth_passes,))
    return dict(interval=float(iv), base=float(b), major_every=int(major_every), smooth_passes=int(smooth_passes), min_length=float(ml),
                scale=Q_SCALE * 16 ** int(smooth_passes))


def level_table(s_min, s_max, z_ref, interval=DEFAULTS["interval"], base=DEFAULTS["base"], smooth_passes=DEFAULTS["smooth_passes"]):
    """-> (lev, n): for every integer n whose level base + n interval lies inside [z_ref + s_min / S, z_ref + s_max / S],
    S = 256 16^smooth_passes, lev holds round-half-even((base + n interval - z_ref) S); both ascending, empty for s_min > s_max
    (no valid cell) or a surface between two levels.  Built with fractions.Fraction: no rounding but the stated one.  Raises
    ValueError if two levels round to one integer or if there are more than MAX_LEVELS."""
    S = Q_SCALE * 16 ** int(smooth_passes)
    iv, b, zr = _exact(interval, "interval"), _exact(base, "base"), Fraction(float(z_ref))
    if iv <= 0:
        raise ValueError("interval=%r must be > 0" % (interval,))
    s_min, s_max = int(s_min), int(s_max)
    if s_min > s_max:
        return [], []
    lo, hi = zr + Fraction(s_min, S), zr + Fraction(s_max, S)
    n0, n1 = math.ceil((lo - b) / iv), math.floor((hi - b) / iv)
    if n1 - n0 + 1 > MAX_LEVELS:
        raise ValueError("interval=%s between %.3f m and %.3f m gives %d levels: at most %d" % (iv, float(lo), float(hi), n1 - n0 + 1, MAX_LEVELS))
    ns = list(range(n0, n1 + 1))
    lev = [int(round((b + n * iv - zr) * S)) for n in ns]                       # Fraction rounds half to even
    for k in range(1, len(lev)):
        if lev[k] <= lev[k - 1]:
            raise ValueError("interval=%s is below the resolution 1/%d m of the surface: levels %d and %d both round to %d"
                             % (iv, S, ns[k - 1], ns[k], lev[k]))
    return lev, ns


# ---- the host's share ---------------------------------------------------------------------------------------------------
def vertex_coordinates(vertex, grid):
    """vertex int64 [P, 3] (edge code, num, den) -> xy float64 [P, 2]: step 8 of the definition."""
    vertex = np.asarray(vertex, np.int64).reshape(-1, 3)
    cell, d = vertex[:, 0] >> 1, vertex[:, 0] & 1
    i, j = cell // int(grid.W), cell % int(grid.W)
    t = vertex[:, 1].astype(np.float64) / vertex[:, 2].astype(np.float64)
    x = grid.x0 + (j + 0.5 + np.where(d == 0, t, 0.0)) * grid.gsd
    y = grid.y_top - (i + 0.5 + np.where(d == 1, t, 0.0)) * grid.gsd
    return np.stack([x, y], axis=1)


def line_lengths(xy, line_first):
    """-> float64 [M]: the length of every polyline, by np.add.reduceat over the vertex order."""
    line_first = np.asarray(line_first, np.int64)
    M = line_first.size - 1
    if M == 0:
        return np.zeros(0, np.float64)
    step = np.zeros(xy.shape[0], np.float64)
    step[:-1] = np.hypot(xy[1:, 0] - xy[:-1, 0], xy[1:, 1] - xy[:-1, 1])
    step[line_first[1:] - 1] = 0.0                                   # from a line's last vertex to the next line's first
    return np.add.reduceat(step, line_first[:-1])


def select(length, line_level, min_length=DEFAULTS["min_length"]):
    """-> the kept lines' numbers ordered by (level, line number): those at least min_length long."""
    keep = np.flatnonzero(np.asarray(length, np.float64) >= float(min_length))
    return keep[np.argsort(np.asarray(line_level, np.int64)[keep], kind="stable")]


def features(xy, line_first, line_level, line_closed, length, order, ns, params):
    """The kept lines as a list of dict(properties, xy): id 1 .. kept in `order`."""
    iv, b = _exact(params["interval"], "interval"), _exact(params["base"], "base")
    feats = []
    for fid, m in enumerate(np.asarray(order).tolist(), start=1):
        p0, p1 = int(line_first[m]), int(line_first[m + 1])
        n = int(ns[int(line_level[m])])
        props = dict(id=fid, elevation_m=float(b + n * iv), level=n, major=n % params["major_every"] == 0, closed=bool(line_closed[m]),
                     vertices=p1 - p0, length_m=float(length[m]))
        feats.append(dict(properties=props, xy=xy[p0:p1]))
    return feats


def geojson_text(feats):
    """A FeatureCollection of LineStrings: fixed key order and number formatting, equal inputs give equal bytes."""
    out = []
    for f in feats:
        props = {k: f["properties"][k] for k in PROPERTIES}
        coords = [[float(x), float(y)] for x, y in np.asarray(f["xy"], np.float64).tolist()]
        out.append(dict(type="Feature", properties=props, geometry=dict(type="LineString", coordinates=coords)))
    return json.dumps(dict(type="FeatureCollection", features=out), separators=(",", ":")) + "\n"


# ---- the stage ----------------------------------------------------------------------------------------------------------
def _no_gpu():
    return raster_stage.no_gpu("contours", "contour")


def trace(z, gsd, z_ref=0.0, interval=DEFAULTS["interval"], base=DEFAULTS["base"], major_every=DEFAULTS["major_every"],
          smooth_passes=DEFAULTS["smooth_passes"], min_length=DEFAULTS["min_length"], grid=None, device=None):
    """z [H, W] float32 (host; NaN where there is no value) -> dict(s, info, lev, ns, count, N, M, entry, exit, level, succ, pred,
    start, rank, closed, line_first, line_start, line_level, line_closed, vertex (all as the header names them, numpy), xy float64
    [N + M, 2], length float64 [M], order (the kept lines by level and number), features, counts, stats, params, grid, seconds).
    grid: the dsm.Grid the coordinates refer to (default: x0 = 0, y_top = H gsd).  Raises ValueError for a finite height further
    than 8191 m from z_ref, and RuntimeError without a GPU: there is no CPU fallback."""
    import torch
    from . import hip_ops
    p = parameters(interval, base, major_every, smooth_passes, min_length)
    gsd = _check_gsd(gsd)
    z = np.ascontiguousarray(z, np.float32)
    if z.ndim != 2:
        raise ValueError("z %s must be [H, W]" % (z.shape,))
    if not math.isfinite(float(z_ref)):
        raise ValueError("z_ref=%r must be finite" % (z_ref,))
    if not torch.cuda.is_available():
        raise _no_gpu()
    H, W = z.shape
    if grid is None:
        grid = raster_stage.default_grid(H, W, gsd, float(z_ref))
    dev = torch.device(device if device is not None else "cuda")
    zd = torch.from_numpy(z).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.time()
    s, info = hip_ops.contour_surface(zd, float(z_ref), p["smooth_passes"])
    s_min, s_max, out_of_range = (int(v) for v in info.cpu().tolist())
    if out_of_range:
        raise ValueError("contours: %d cells lie further than %d m from z_ref=%g" % (out_of_range, MAX_ABS_M, float(z_ref)))
    lev, ns = level_table(s_min, s_max, z_ref, interval, base, p["smooth_passes"])
    t1 = time.time()
    count, N, ws, st = hip_ops.contour_count(s, lev)
    t2 = time.time()
    seg = hip_ops.contour_segments(s, lev, N, ws)
    torch.cuda.synchronize(dev)
    t3 = time.time()
    start, rank, closed, M, ws2, st = hip_ops.contour_rank(seg[4], stats=st)
    t4 = time.time()
    line_first, line_start, line_level, line_closed, vertex = hip_ops.contour_lines(s, lev, seg, start, rank, closed, M, ws2)
    res = dict(s=s, count=count, entry=seg[0], exit=seg[1], level=seg[2], succ=seg[3], pred=seg[4], start=start, rank=rank, closed=closed,
               line_first=line_first, line_start=line_start, line_level=line_level, line_closed=line_closed, vertex=vertex)
    res = {k: v.cpu().numpy() for k, v in res.items()}
    valid = int((res["s"] != -2 ** 31).sum())
    t5 = time.time()
    xy = vertex_coordinates(res["vertex"], grid)
    length = line_lengths(xy, res["line_first"])
    order = select(length, res["line_level"], p["min_length"])
    feats = features(xy, res["line_first"], res["line_level"], res["line_closed"], length, order, ns, p)
    t6 = time.time()
    counts = dict(valid=valid, levels=len(lev), segments=N, lines=M, closed=int(res["line_closed"].sum()), kept=int(order.size),
                  rejected_short=int(M - order.size), vertices=int(sum(f["properties"]["vertices"] for f in feats)),
                  longest=int((res["line_first"][1:] - res["line_first"][:-1]).max()) if M else 0)
    stats = dict(rounds=int(st.rounds), rounds_min=int(st.rounds_min), rounds_dist=int(st.rounds_dist), launched=int(st.launched),
                 converged=int(st.converged), ms_count=float(st.ms_count), ms_rank=float(st.ms_rank))
    res.update(info=(s_min, s_max, out_of_range), lev=lev, ns=ns, N=N, M=M, xy=xy, length=length, order=order, features=feats,
               counts=counts, stats=stats, params=p, grid=grid, gsd=float(gsd), z_ref=float(z_ref),
               seconds=dict(surface=t1 - t0, count=t2 - t1, segments=t3 - t2, rank=t4 - t3, lines=t5 - t4, host=t6 - t5))
    return res


def from_dsm(prefix, source=DEFAULTS["source"], interval=DEFAULTS["interval"], base=DEFAULTS["base"], major_every=DEFAULTS["major_every"],
             smooth_passes=DEFAULTS["smooth_passes"], min_length=DEFAULTS["min_length"], device=None, out=None):
    """The raster `<prefix>_<source>.tif` of an earlier stage -> trace()'s dict with `source` added; written to `out` (a path
    prefix) if given.  The heights are quantised about the grid's z_ref (about 0 for the nDSM, which is a height above ground)."""
    import torch
    if source not in SOURCES:
        raise ValueError("source=%r must be one of %s" % (source, ", ".join(SOURCES)))
    parameters(interval, base, major_every, smooth_passes, min_length)
    grid = raster_stage.read_grid(prefix)
    path = "%s_%s.tif" % (prefix, source)
    hint = {"dtm": "dtm_whu.py --dsm", "ndsm": "dtm_whu.py --dsm", "dsm": "dsm_whu.py --out", "dsm_filled": "dsm_whu.py --fill_max_dist .. --out"}
    raster_stage.require(path, "no such raster (run %s %s first)" % (hint[source], prefix))
    if not torch.cuda.is_available():
        raise _no_gpu()
    z = raster_stage.read_raster(path, np.float32, (grid.H, grid.W), says="the grid %d x %d" % (grid.H, grid.W))
    z_ref = 0.0 if source == "ndsm" else grid.z_ref
    res = trace(z, grid.gsd, z_ref, interval, base, major_every, smooth_passes, min_length, grid, device)
    res["source"] = dict(prefix=prefix, raster=source)
    if out is not None:
        write_outputs(out, res)
    return res


# ---- files --------------------------------------------------------------------------------------------------------------
def output_paths(out):
    """The files of this stage, disjoint from those of every earlier stage."""
    return dict(geojson=out + "_contours.geojson", json=out + "_contours.json")


def summary(res):
    params = dict(res["params"], z_ref=res["z_ref"], lev=[int(v) for v in res["lev"]], n=[int(v) for v in res["ns"]])
    return dict(grid=raster_stage.grid_summary(res["grid"]), source=res.get("source"), params=params, counts=res["counts"],
                stats=res["stats"], seconds=res["seconds"])


def write_outputs(out, res):
    """The GeoJSON file and the JSON summary at the path prefix `out` -> output_paths(out)."""
    return raster_stage.write_outputs(output_paths(out), out, dict(geojson=geojson_text(res["features"])), summary(res))


def read_outputs(out):
    """-> (the lines as a dict, the summary as a dict) read back from write_outputs' files."""
    return raster_stage.read_outputs(output_paths(out), ("geojson",))


def build_parser():
    ap = argparse.ArgumentParser(description="Draw the contour lines of the DTM as ordered polylines")
    ap.add_argument("--dsm", required=True, metavar="PREFIX", help="path prefix of the earlier stages' output "
                    "(<PREFIX>_<source>.tif, <PREFIX>_dsm.json)")
    ap.add_argument("--source", choices=SOURCES, default=DEFAULTS["source"], help="the raster whose lines are drawn")
    ap.add_argument("--interval", type=float, default=DEFAULTS["interval"], help="height between two lines in metres")
    ap.add_argument("--base", type=float, default=DEFAULTS["base"], help="the lines lie at base + n interval metres")
    ap.add_argument("--major_every", type=int, default=DEFAULTS["major_every"], help="every n-th line (n divisible by this) is marked major")
    ap.add_argument("--smooth_passes", type=int, default=DEFAULTS["smooth_passes"], help="3 x 3 binomial smoothing passes of the surface: 0, 1 or 2")
    ap.add_argument("--min_length", type=float, default=DEFAULTS["min_length"], help="least length of a written line in metres")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="output path prefix (default: --dsm): <out>_contours.geojson, <out>_contours.json")
    return ap


def main(argv=None):
    args, out, t0 = raster_stage.open_main(build_parser, argv)
    res = from_dsm(args.dsm, args.source, args.interval, args.base, args.major_every, args.smooth_passes, args.min_length, out=out)
    g, c, s, st = res["grid"], res["counts"], res["seconds"], res["stats"]
    print("contours %d x %d cells at gsd %g: %d valid cells, %d levels, %d segments in %d lines (%d closed, longest %d vertices), %d ranking "
          "rounds" % (g.W, g.H, g.gsd, c["valid"], c["levels"], c["segments"], c["lines"], c["closed"], c["longest"], st["rounds"]))
    print("%d lines written, %d rejected as short; surface %.3f s, count %.3f s, segments %.3f s, rank %.3f s, lines %.3f s, host %.3f s; "
          "total_time = %.3f s" % (c["kept"], c["rejected_short"], s["surface"], s["count"], s["segments"], s["rank"], s["lines"], s["host"],
                                   time.time() - t0))
    return res


if __name__ == "__main__":
    main()
