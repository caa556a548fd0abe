"""Roof planes of the buildings: every building's roof cut into planar faces with their pitch, aspect and true area (LoD2).

    python roofs_whu.py --dsm /out/predict/dsm [--filled] [--smooth_span 1.0] [--smooth_tol 0.2] [--slope_tol 0.15] [--step_tol 0.1]
                        [--assign_tol 0.2] [--min_plane_area 2] [--grow_rounds N] [--merge_rms 0.1] [--flat_deg 5] [--out PREFIX]

The step after buildings_whu.py.  Read: the DSM (`<PREFIX>_dsm.tif`, or `<PREFIX>_dsm_filled.tif` with --filled), the building
labels (`<PREFIX>_buildings.tif`) and the grid (`<PREFIX>_dsm.json`).  The method is smoothness-constraint region growing
(Rabbani et al. 2006) restated so that nothing depends on a visiting order; include/adamvs_hip.h "Roof planes" states the result
operation by operation.  On the GPU (csrc/dsm_roofs.hip): a symmetric link test between adjacent cells (equal gradient across
smooth_span within slope_tol, no step above step_tol), the connected components of the links, integer moments per component,
the growth of the fitted planes into the unassigned rims (a cell joins the neighbouring plane it fits best within assign_tol,
grow_rounds times), and the residuals.  On the host, in exact integer arithmetic: the least-squares plane of every component
that covers min_plane_area, and the merge of adjacent planes of one building whose joint fit stays within merge_rms.  Written:
`<out>_roofs.geojson` (one Polygon per plane in the conventions of buildings_whu.py; properties id, building, cells,
segments_merged, area_m2, area_3d_m2, slope_deg, aspect_deg (the azimuth of steepest descent, clockwise from north; null below
flat_deg), kind (flat / pitched), normal, plane (z = z0 + sx (x - xc) + sy (y - yc)), rms_m, max_residual_m, inlier_fraction,
height_min, height_max), `<out>_roofs.tif` (int32 plane labels, 0 = none), `<out>_roofs.tfw` and `<out>_roofs.json`.  --out
defaults to --dsm; none of the names collides with a file of an earlier stage.

The defaults are conventions, not values measured on WHU scenes.  A curved roof (a dome) comes out as few planes with a large
rms_m, which is reported and not hidden.  Not here: ridge and eave lines, roof-type names, right-angle regularisation (the solids
and their CityJSON are the next stage's: lod2.py).
"""
import argparse
import math
import time
from fractions import Fraction

import numpy as np

from . import raster_stage
from .buildings import geojson_text, polygons
from .dsm import _check_gsd

MAX_STRIDE = 64                                     # ADAMVS_BLD_MAX_STRIDE, cells
MAX_GROW = 256                                      # ADAMVS_ROOF_MAX_GROW, rounds
MAX_SIDE = 32768                                    # ADAMVS_ROOF_MAX_SIDE, cells
Q_SCALE = 256                                       # ADAMVS_ROOF_Q_SCALE: q is the height above z_ref in 1/256 m
GROW_CHUNK = 4                                      # growth rounds between two looks at the counts
DEFAULTS = dict(smooth_span=1.0, smooth_tol=0.2, slope_tol=0.15, step_tol=0.1, assign_tol=0.2, min_plane_area=2.0, grow_rounds=None,
                merge_rms=0.1, flat_deg=5.0)
COLUMNS = ("n", "su", "sv", "sq", "suu", "suv", "svv", "suq", "svq", "sqq_lo", "sqq_hi", "row_min", "row_max", "col_min", "col_max", "q_min",
           "q_max", "building")
_N_SUMS = 11                                        # n .. sqq_hi add; then minima and maxima
_IS_MIN = (True, False, True, False, True, False, False)   # row_min, row_max, col_min, col_max, q_min, q_max, building


def parameters(gsd, smooth_span=DEFAULTS["smooth_span"], smooth_tol=DEFAULTS["smooth_tol"], slope_tol=DEFAULTS["slope_tol"],
               step_tol=DEFAULTS["step_tol"], assign_tol=DEFAULTS["assign_tol"], min_plane_area=DEFAULTS["min_plane_area"],
               grow_rounds=DEFAULTS["grow_rounds"], merge_rms=DEFAULTS["merge_rms"], flat_deg=DEFAULTS["flat_deg"]):
    """The checked parameters with what is derived from them: stride = max(1, round(smooth_span / gsd)) (round half to even),
    g_tol = slope_tol (2 stride gsd) and grow_rounds = min(4 stride, MAX_GROW) unless given.  Raises ValueError."""
    gsd = _check_gsd(gsd)
    p = dict(smooth_span=float(smooth_span), smooth_tol=float(smooth_tol), slope_tol=float(slope_tol), step_tol=float(step_tol),
             assign_tol=float(assign_tol), min_plane_area=float(min_plane_area), merge_rms=float(merge_rms), flat_deg=float(flat_deg))
    for name, v in p.items():
        positive = name == "smooth_span"
        if not math.isfinite(v) or v < 0.0 or (positive and v == 0.0):
            raise ValueError("%s=%r must be finite and %s 0" % (name, v, ">" if positive else ">="))
    if p["flat_deg"] > 90.0:
        raise ValueError("flat_deg=%r is an angle: 0 .. 90" % p["flat_deg"])
    stride = max(1, int(round(p["smooth_span"] / gsd)))
    if stride > MAX_STRIDE:
        raise ValueError("smooth_span=%g m at gsd %g is %d cells: at most %d" % (p["smooth_span"], gsd, stride, MAX_STRIDE))
    if grow_rounds is None:
        grow_rounds = min(4 * stride, MAX_GROW)
    if isinstance(grow_rounds, bool) or int(grow_rounds) != grow_rounds or not 0 <= int(grow_rounds) <= MAX_GROW:
        raise ValueError("grow_rounds=%r must be an integer 0 .. %d" % (grow_rounds, MAX_GROW))
    p.update(stride=int(stride), g_tol=p["slope_tol"] * (2 * stride * gsd), grow_rounds=int(grow_rounds))
    return p


# ---- planes from moments, exactly ---------------------------------------------------------------------------------------
def fit_moments(row):
    """row: the integers of one label in the order of COLUMNS (at least n .. sqq_hi) -> None if the label is empty or its cells
    lie on one line (the centred determinant is zero), otherwise dict(a, b, c, sse: Fractions in units of 1/256 m per cell,
    1/256 m and (1/256 m)^2; n).  The exact least-squares solution of the integer normal equations."""
    n, su, sv, sq, suu, suv, svv, suq, svq, lo, hi = (int(v) for v in row[:_N_SUMS])
    if n <= 0:
        return None
    cuu, cvv, cuv = n * suu - su * su, n * svv - sv * sv, n * suv - su * sv
    det = cuu * cvv - cuv * cuv
    if det == 0:
        return None
    cuq, cvq = n * suq - su * sq, n * svq - sv * sq
    a = Fraction(cuq * cvv - cvq * cuv, det)
    b = Fraction(cvq * cuu - cuq * cuv, det)
    c = (Fraction(sq) - a * su - b * sv) / n
    sqq = lo + (hi << 20)
    return dict(a=a, b=b, c=c, sse=sqq - a * suq - b * svq - c * sq, n=n)


def plane_metres(fit):
    """-> [a, b, c] in fp64 metres (per cell, per cell, above z_ref): each rational divided by 256, rounded once."""
    return [float(fit[k] / Q_SCALE) for k in "abc"]


def select_planes(table, gsd, min_plane_area=DEFAULTS["min_plane_area"]):
    """table: int64 [18, S] -> (keep bool [S], planes fp64 [P, 3]).  A segment is kept iff n gsd^2 >= min_plane_area and its
    determinant is not zero."""
    table = np.asarray(table, np.int64)
    keep = np.zeros(table.shape[1], bool)
    planes = []
    big = table[0].astype(np.float64) * (float(gsd) * float(gsd)) >= float(min_plane_area)
    for k in np.flatnonzero(big).tolist():
        fit = fit_moments(table[:, k].tolist())
        if fit is not None:
            keep[k] = True
            planes.append(plane_metres(fit))
    return keep, np.array(planes, np.float64).reshape(-1, 3)


def sum_rows(r0, r1):
    """The moments of the union of two disjoint labels."""
    out = [int(x) + int(y) for x, y in zip(r0[:_N_SUMS], r1[:_N_SUMS])]
    out += [(min if is_min else max)(int(x), int(y)) for is_min, x, y in zip(_IS_MIN, r0[_N_SUMS:], r1[_N_SUMS:])]
    return out


def merge_planes(rows, adjacency, merge_rms=DEFAULTS["merge_rms"]):
    """rows: P lists of integers (COLUMNS), plane p = rows[p - 1]; adjacency: {(p, q): shared cell edges}, p < q, 1-based.
    Greedy merge on the region graph: among the adjacent pairs whose summed moments have a fit with
    sse / 256^2 <= merge_rms^2 n (compared as exact rationals), the pair of least sse / n is merged, ties to the smaller
    (p, q); the merged plane keeps the smaller id and inherits both sets of neighbours.  Repeated until no pair qualifies;
    merge_rms = 0 switches the merge off.  -> (groups: the member lists in ascending order of their smallest member, the
    summed rows of the groups, the shared edges between the groups {(r, s): edges}, 1-based group numbers)."""
    rows = {p: [int(v) for v in r] for p, r in enumerate(rows, start=1)}
    members = {p: [p] for p in rows}
    nbrs = {p: {} for p in rows}
    for (p, q), cnt in adjacency.items():
        p, q = int(p), int(q)
        if not (1 <= p < q <= len(rows)):
            raise ValueError("adjacency pair (%d, %d) outside 1 <= p < q <= %d" % (p, q, len(rows)))
        nbrs[p][q] = nbrs[q][p] = int(cnt)
    if merge_rms > 0.0:
        bar = Fraction(float(merge_rms)) ** 2 * (Q_SCALE * Q_SCALE)
        score = {}                                                   # (p, q) -> (sse / n, summed row) or None: not a candidate

        def rate(p, q):
            row = sum_rows(rows[p], rows[q])
            fit = fit_moments(row)
            score[(p, q)] = None if fit is None or fit["sse"] > bar * fit["n"] else (fit["sse"] / fit["n"], row)

        for p in nbrs:
            for q in nbrs[p]:
                if p < q:
                    rate(p, q)
        while True:
            live = [(v[0], k) for k, v in score.items() if v is not None]
            if not live:
                break
            _, (p, q) = min(live)
            rows[p] = score[(p, q)][1]
            members[p] = sorted(members[p] + members.pop(q))
            del rows[q]
            for k in [k for k in score if p in k or q in k]:
                del score[k]
            for x, cnt in nbrs.pop(q).items():
                del nbrs[x][q]
                if x != p:
                    nbrs[p][x] = nbrs[x][p] = nbrs[p].get(x, 0) + cnt
            for x in nbrs[p]:
                rate(min(p, x), max(p, x))
    order = sorted(members)
    number = {p: r for r, p in enumerate(order, start=1)}
    edges = {(number[p], number[q]): cnt for p in order for q, cnt in sorted(nbrs[p].items()) if p < q}
    return [members[p] for p in order], [rows[p] for p in order], edges


# ---- what a plane means --------------------------------------------------------------------------------------------------
def plane_properties(a, b, gsd, flat_deg=DEFAULTS["flat_deg"]):
    """a, b: metres per cell along the columns (east) and the rows (south) -> dict(sx, sy: metres per metre east and north,
    slope_deg, aspect_deg: the azimuth of steepest descent clockwise from north in [0, 360), None below flat_deg, kind,
    normal: the upward unit normal (east, north, up), stretch = sqrt(1 + sx^2 + sy^2): true area over plan area)."""
    sx, sy = float(a) / gsd, -float(b) / gsd
    stretch = math.sqrt(1.0 + sx * sx + sy * sy)
    slope = math.degrees(math.atan(math.hypot(sx, sy)))
    flat = slope < flat_deg
    aspect = None if flat else math.degrees(math.atan2(-sx, -sy)) % 360.0
    if aspect is not None and aspect >= 360.0:                       # -1e-17 % 360 rounds to 360
        aspect = 0.0
    return dict(sx=sx, sy=sy, slope_deg=slope, aspect_deg=aspect, kind="flat" if flat else "pitched",
                normal=[-sx / stretch, -sy / stretch, 1.0 / stretch], stretch=stretch)


def feature_properties(rows, groups, fits, residuals, grid, z_ref, flat_deg=DEFAULTS["flat_deg"]):
    """The properties of the final planes, in order: id 1 .. R."""
    gsd = float(grid.gsd)
    props = []
    for r, (row, group, fit) in enumerate(zip(rows, groups, fits), start=1):
        n = int(row[0])
        a, b, c = plane_metres(fit)
        pp = plane_properties(a, b, gsd, flat_deg)
        uc, vc = int(row[1]) / n, int(row[2]) / n
        area = n * (gsd * gsd)
        props.append(dict(id=r, building=int(row[17]), cells=n, segments_merged=len(group), area_m2=area, area_3d_m2=area * pp["stretch"],
                          slope_deg=pp["slope_deg"], aspect_deg=pp["aspect_deg"], kind=pp["kind"], normal=pp["normal"],
                          plane=dict(z0=float(z_ref) + ((a * uc + b * vc) + c), sx=pp["sx"], sy=pp["sy"], xc=grid.x0 + (uc + 0.5) * gsd,
                                     yc=grid.y_top - (vc + 0.5) * gsd),
                          rms_m=math.sqrt(max(0.0, float(fit["sse"] / n))) / Q_SCALE, max_residual_m=int(residuals[1][r - 1]) / 1024.0,
                          inlier_fraction=int(residuals[0][r - 1]) / n, height_min=float(z_ref) + int(row[15]) / Q_SCALE,
                          height_max=float(z_ref) + int(row[16]) / Q_SCALE))
    return props


# ---- the stage ----------------------------------------------------------------------------------------------------------
def _no_gpu():
    return raster_stage.no_gpu("roofs", "roof-plane")


def reference_height(dsm):
    """z_ref = floor(min finite Z); 0 for a raster without a finite cell."""
    fin = dsm[np.isfinite(dsm)]
    return float(math.floor(float(fin.min()))) if fin.size else 0.0


def grow(d, b, z_ref, planes, assign_tol, seed, rounds, stop_early=True):
    """The growth rounds on the device: seed int32 [H, W] (device) -> (label, counts int64 [rounds] (numpy), rounds run).  With
    stop_early the counts are read every GROW_CHUNK rounds and the loop ends after a round that labelled nothing: a fixed
    point, so the labels and the counts (zero from there on) are those of all the rounds."""
    import torch
    from . import hip_ops
    bufs = [seed.clone(), torch.empty_like(seed)]                 # the seed itself stays as it is
    counts = torch.zeros(MAX_GROW, device=seed.device, dtype=torch.int32)
    host = np.zeros(rounds, np.int64)
    done = 0
    while done < rounds:
        m = min(GROW_CHUNK, rounds - done)
        hip_ops.roof_grow(d, b, z_ref, planes, assign_tol, bufs[0], bufs[1], counts, done, m)
        host[done:done + m] = counts[done:done + m].cpu().numpy()
        done += m
        if stop_early and (host[done - m:done] == 0).any():
            break
    return bufs[done & 1], host, done


def region_adjacency(label, b, P):
    """label, b int32 [H, W] (device) -> {(p, q): shared cell edges}, p < q: the 4-adjacent cells with different plane labels > 0
    and the same building."""
    import torch
    keys = []
    for x, y, bx, by in ((label[:, :-1], label[:, 1:], b[:, :-1], b[:, 1:]), (label[:-1, :], label[1:, :], b[:-1, :], b[1:, :])):
        ok = (x > 0) & (y > 0) & (x != y) & (bx == by)
        x, y = x[ok].long(), y[ok].long()
        keys.append(torch.minimum(x, y) * (P + 1) + torch.maximum(x, y))
    key, cnt = torch.unique(torch.cat(keys), return_counts=True)
    return {(int(k) // (P + 1), int(k) % (P + 1)): int(c) for k, c in zip(key.tolist(), cnt.tolist())}


def extract(dsm, building, gsd, smooth_span=DEFAULTS["smooth_span"], smooth_tol=DEFAULTS["smooth_tol"], slope_tol=DEFAULTS["slope_tol"],
            step_tol=DEFAULTS["step_tol"], assign_tol=DEFAULTS["assign_tol"], min_plane_area=DEFAULTS["min_plane_area"],
            grow_rounds=DEFAULTS["grow_rounds"], merge_rms=DEFAULTS["merge_rms"], flat_deg=DEFAULTS["flat_deg"], grid=None, device=None,
            stop_early=True):
    """dsm [H, W] float32 (host; NaN where there is no value), building [H, W] int32 (0 none, 1 .. B) -> dict(label int32 (0 none,
    planes 1 .. R), properties, polygons, table (int64 [18, R], COLUMNS), groups, edges, residuals int64 [2, R]; the
    intermediate results link uint8, parent, segments int32 (1 .. S), segment_table, keep, planes fp64 [P, 3], seed, grown int32
    (1 .. P), grow_counts, grown_table, adjacency, final_planes fp64 [R, 3]; counts, per_building, label_stats, grow_stats,
    params, z_ref, seconds).  grid: the dsm.Grid the polygons' coordinates refer to (default: x0 = 0, y_top = H gsd).  Raises
    without a GPU: there is no CPU fallback."""
    import torch
    from . import hip_ops
    p = parameters(gsd, smooth_span, smooth_tol, slope_tol, step_tol, assign_tol, min_plane_area, grow_rounds, merge_rms, flat_deg)
    dsm = np.ascontiguousarray(dsm, np.float32)
    building = np.ascontiguousarray(building)
    if dsm.ndim != 2 or dsm.shape != building.shape:
        raise ValueError("dsm %s and building %s must be one [H, W]" % (dsm.shape, building.shape))
    if building.dtype.kind not in "iu":
        raise ValueError("building must hold integer labels, got %s" % building.dtype)
    building = building.astype(np.int32)
    H, W = dsm.shape
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError("the grid is %d x %d cells: at most %d on a side" % (W, H, MAX_SIDE))
    if not torch.cuda.is_available():
        raise _no_gpu()
    gsd = float(gsd)
    if grid is None:
        grid = raster_stage.default_grid(H, W, gsd)
    z_ref = reference_height(dsm)
    dev = torch.device(device if device is not None else "cuda")
    d, b = torch.from_numpy(dsm).to(dev), torch.from_numpy(building).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.time()
    link = hip_ops.roof_links(d, b, p["stride"], p["smooth_tol"], p["g_tol"], p["step_tol"])
    torch.cuda.synchronize(dev)
    t1 = time.time()
    seg, S, parent, st = hip_ops.roof_label(link)
    t2 = time.time()
    seg_table = hip_ops.roof_moments(d, seg, b, z_ref, S).cpu().numpy()
    t3 = time.time()
    keep, planes = select_planes(seg_table, gsd, p["min_plane_area"])
    P = int(keep.sum())
    t4 = time.time()
    seed = raster_stage.relabel_kept(seg, keep)
    planes_dev = torch.from_numpy(planes).to(dev)
    grown, grow_counts, rounds_run = grow(d, b, z_ref, planes_dev, p["assign_tol"], seed, p["grow_rounds"], stop_early)
    torch.cuda.synchronize(dev)
    t5 = time.time()
    grown_table = hip_ops.roof_moments(d, grown, b, z_ref, P).cpu().numpy()
    adjacency = region_adjacency(grown, b, P)
    t6 = time.time()
    groups, rows, edges = merge_planes(grown_table.T.tolist(), adjacency, p["merge_rms"])
    R = len(groups)
    fits = [fit_moments(r) for r in rows]
    final_planes = np.array([plane_metres(f) for f in fits], np.float64).reshape(-1, 3)
    t7 = time.time()
    lut2 = np.zeros(P + 1, np.int32)
    for r, g in enumerate(groups, start=1):
        lut2[g] = r
    label_dev = torch.from_numpy(lut2).to(dev)[grown.long()]          # the look-up of the plane numbers
    resid = hip_ops.roof_residuals(d, label_dev, z_ref, torch.from_numpy(final_planes).to(dev), p["assign_tol"]).cpu().numpy()
    label = label_dev.cpu().numpy()
    t8 = time.time()
    polys = polygons(label, grid)                                     # raises if a plane is not one 4-connected component
    props = feature_properties(rows, groups, fits, resid, grid, z_ref, p["flat_deg"])
    t9 = time.time()
    link_h = link.cpu().numpy()
    cells_building = int((building > 0).sum())
    counts = dict(building_cells=cells_building, core_cells=int((link_h & 1).sum()), segments=S, segments_kept=P,
                  cells_seeded=int(seg_table[0][keep].sum()) if S else 0, cells_grown=int(grow_counts.sum()), planes=R,
                  cells_assigned=int((label > 0).sum()), cells_unassigned=int(((building > 0) & (label == 0)).sum()))
    per_building = {}
    for row in rows:
        per_building[str(int(row[17]))] = per_building.get(str(int(row[17])), 0) + 1
    table = np.array(rows, np.int64).reshape(-1, len(COLUMNS)).T
    return dict(label=label, properties=props, polygons=polys, table=table, groups=groups, edges=edges, residuals=resid, link=link_h,
                parent=parent.cpu().numpy(), segments=seg.cpu().numpy(), S=S, segment_table=seg_table, keep=keep, planes=planes, P=P,
                seed=seed.cpu().numpy(), grown=grown.cpu().numpy(), grow_counts=grow_counts, grown_table=grown_table, adjacency=adjacency,
                final_planes=final_planes, fits=fits, R=R, counts=counts, per_building=per_building,
                label_stats=dict(rounds=int(st.rounds), tiles=int(st.tiles), pairs=int(st.pairs)),
                grow_stats=dict(rounds=p["grow_rounds"], rounds_run=int(rounds_run), per_round=[int(v) for v in grow_counts]),
                params=p, gsd=gsd, grid=grid, z_ref=z_ref,
                seconds=dict(links=t1 - t0, label=t2 - t1, moments=t3 - t2, planes=t4 - t3, grow=t5 - t4, adjacency=t6 - t5, merge=t7 - t6,
                             residuals=t8 - t7, vectorise=t9 - t8))


def from_dsm(prefix, filled=False, smooth_span=DEFAULTS["smooth_span"], smooth_tol=DEFAULTS["smooth_tol"], slope_tol=DEFAULTS["slope_tol"],
             step_tol=DEFAULTS["step_tol"], assign_tol=DEFAULTS["assign_tol"], min_plane_area=DEFAULTS["min_plane_area"],
             grow_rounds=DEFAULTS["grow_rounds"], merge_rms=DEFAULTS["merge_rms"], flat_deg=DEFAULTS["flat_deg"], device=None, out=None):
    """The DSM of dsm_whu.py at the path prefix (its gap-filled raster if `filled`) and the building labels of buildings_whu.py
    next to it -> extract()'s dict with `source` added; written to `out` (a path prefix) if given."""
    import torch
    from .ortho import read_dsm
    dsm, grid = read_dsm(prefix, filled)
    bpath = prefix + "_buildings.tif"
    raster_stage.require(bpath, "no building labels (run buildings_whu.py --dsm %s first)" % prefix)
    if not torch.cuda.is_available():
        raise _no_gpu()
    building = raster_stage.read_raster(bpath, np.int32, dsm.shape, says="the DSM %s" % (dsm.shape,))
    res = extract(dsm, building, grid.gsd, smooth_span, smooth_tol, slope_tol, step_tol, assign_tol, min_plane_area, grow_rounds, merge_rms,
                  flat_deg, grid, device)
    res["source"] = dict(prefix=prefix, filled=bool(filled))
    if out is not None:
        write_outputs(out, res)
    return res


# ---- files --------------------------------------------------------------------------------------------------------------
def output_paths(out):
    """The files of this stage, disjoint from those of dsm_whu.py, its gap fill, dtm_whu.py and buildings_whu.py."""
    return dict(geojson=out + "_roofs.geojson", label=out + "_roofs.tif", label_world=out + "_roofs.tfw", json=out + "_roofs.json")


def summary(res):
    return dict(grid=raster_stage.grid_summary(res["grid"]), source=res.get("source"), params=res["params"], z_ref=res["z_ref"],
                counts=res["counts"], planes_per_building=res["per_building"], label_stats=res["label_stats"], grow_stats=res["grow_stats"],
                seconds=res["seconds"])


def write_outputs(out, res):
    """The GeoJSON, the label raster, its world file and the JSON summary at the path prefix `out` -> output_paths(out)."""
    return raster_stage.write_outputs(output_paths(out), out, dict(geojson=geojson_text(res["polygons"], res["properties"])), summary(res),
                                      res["label"], res["grid"])


def read_outputs(out):
    """-> (label int32, the GeoJSON as a dict, the summary as a dict) read back from the files of write_outputs."""
    return raster_stage.read_outputs(output_paths(out), ("geojson",))


def build_parser():
    ap = argparse.ArgumentParser(description="Segment the roofs of the extracted buildings into planes")
    ap.add_argument("--dsm", required=True, metavar="PREFIX", help="path prefix of dsm_whu.py's and buildings_whu.py's output "
                    "(<PREFIX>_dsm.tif, <PREFIX>_buildings.tif, <PREFIX>_dsm.json)")
    ap.add_argument("--filled", action="store_true", help="use <PREFIX>_dsm_filled.tif (dsm_whu.py --fill_max_dist), as buildings_whu.py --filled did")
    ap.add_argument("--smooth_span", type=float, default=DEFAULTS["smooth_span"], help="half length in metres of the differences of the DSM")
    ap.add_argument("--smooth_tol", type=float, default=DEFAULTS["smooth_tol"], help="largest second difference in metres of a core cell")
    ap.add_argument("--slope_tol", type=float, default=DEFAULTS["slope_tol"], help="largest difference of slope (metres per metre) across a link")
    ap.add_argument("--step_tol", type=float, default=DEFAULTS["step_tol"], help="largest step in metres across a link beyond the slope's rise")
    ap.add_argument("--assign_tol", type=float, default=DEFAULTS["assign_tol"], help="largest distance in metres of a grown cell from its plane")
    ap.add_argument("--min_plane_area", type=float, default=DEFAULTS["min_plane_area"], help="least area in square metres of a segment that seeds a plane")
    ap.add_argument("--grow_rounds", type=int, default=None, help="growth rounds (default: four strides, at most %d)" % MAX_GROW)
    ap.add_argument("--merge_rms", type=float, default=DEFAULTS["merge_rms"], help="largest rms in metres of a merged plane (0: no merge)")
    ap.add_argument("--flat_deg", type=float, default=DEFAULTS["flat_deg"], help="a plane below this slope in degrees is flat and has no aspect")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="output path prefix (default: --dsm): <out>_roofs.geojson, ...")
    return ap


def main(argv=None):
    args, out, t0 = raster_stage.open_main(build_parser, argv)
    res = from_dsm(args.dsm, args.filled, args.smooth_span, args.smooth_tol, args.slope_tol, args.step_tol, args.assign_tol, args.min_plane_area,
                   args.grow_rounds, args.merge_rms, args.flat_deg, out=out)
    g, c, p, s = res["grid"], res["counts"], res["params"], res["seconds"]
    print("roofs %d x %d cells at gsd %g: stride %d cells; %d building cells, %d core, %d segments (%d border rounds), %d kept"
          % (g.W, g.H, g.gsd, p["stride"], c["building_cells"], c["core_cells"], c["segments"], res["label_stats"]["rounds"], c["segments_kept"]))
    print("%d cells grown in %d of %d rounds; %d planes after the merge, %d building cells unassigned; links %.3f s, labels %.3f s, "
          "growth %.3f s, merge %.3f s, outlines %.3f s; total_time = %.3f s"
          % (c["cells_grown"], res["grow_stats"]["rounds_run"], p["grow_rounds"], c["planes"], c["cells_unassigned"], s["links"], s["label"],
             s["grow"], s["merge"], s["vectorise"], time.time() - t0))
    return res


if __name__ == "__main__":
    main()
