"""LoD2 building solids: footprints, roof planes and terrain joined into one watertight solid per building (CityJSON, OBJ).

    python lod2_whu.py --dsm /out/predict/dsm [--fill_rounds N] [--out PREFIX]

The step after roofs_whu.py.  Read: the grid (`<PREFIX>_dsm.json`), the terrain (`<PREFIX>_dtm.tif`), the building labels
(`<PREFIX>_buildings.tif`), the plane labels (`<PREFIX>_roofs.tif`) and every plane's `building` and `plane` from
`<PREFIX>_roofs.geojson`.  include/adamvs_hip.h "LoD2 solids" states the result operation by operation.  Everything is integer:
heights in 1/1024 m above z_ref = floor(min finite DTM), horizontal positions in 1/1024 of a cell.  On the host: the planes as
integers (integer_planes).  On the GPU (csrc/dsm_lod2.hip): the model labels (the roof labels spread over the building cells the
roof stage left unassigned, the smallest neighbouring plane first, fill_rounds times), the per-building table (cells, filled
cells, base = the lowest terrain under the building, the lowest roof corner) and the boundary runs of the model labels: one
record per maximal stretch of a lattice line with the same pair of labels on its two sides, with the heights of both sides at
both ends, in a fixed order.  On the host again, in exact integers over the runs only (faces): the walls (a vertical polygon
per run whose sides differ in height, two triangles where the sides cross), one roof polygon with holes per plane, one ground
polygon per building.  A building without any plane, without terrain, or whose base is not below its lowest roof corner gets no
solid and is counted with its reason.  Written: `<out>_lod2.city.json` (CityJSON 1.1, one Building with one Solid of lod "2" per
building, RoofSurface / WallSurface / GroundSurface semantics, integer vertices under the transform), `<out>_lod2.obj` (the same
faces as triangles, one `o` per building) and `<out>_lod2.json`.  --out defaults to --dsm; none of the names collides with a file
of an earlier stage.

Not here: ridge and eave lines as plane intersections, right-angle regularisation, roof-type names, textures.  A crossing of two
roof planes along a run that falls within 1/2048 of a cell of the run's end is rounded onto that end: the two triangles are then
slivers of no area, kept so that the shell stays closed.
"""
import argparse
import json
import math
import time
from collections import Counter
from fractions import Fraction

import numpy as np

from . import raster_stage
from .dsm import _check_gsd
from .roofs import reference_height

MAX_SIDE = 32768                                    # ADAMVS_LOD2_MAX_SIDE, cells
MAX_FILL = 1024                                     # ADAMVS_LOD2_MAX_FILL, rounds
Z_SCALE = 1024                                      # ADAMVS_LOD2_Z_SCALE: heights in 1/1024 m above z_ref
XY_SCALE = 1024                                     # ADAMVS_LOD2_XY_SCALE: positions in 1/1024 of a cell
PLANE_BITS = 20                                     # ADAMVS_LOD2_PLANE_BITS
Z_MAX = 1 << 30                                     # ADAMVS_LOD2_Z_MAX
FILL_CHUNK = 8                                      # fill rounds between two looks at the counts
MIN_START = (1 << 31) - 1                           # the start of a minimum of the building table
COLUMNS = ("cells", "filled", "base", "roof_min")
FIELDS = ("orientation", "line", "start", "end", "L", "R", "zL_s", "zL_e", "zR_s", "zR_e")
REASONS = ("no_plane", "no_terrain", "base_not_below_roof")
DEFAULTS = dict(fill_rounds=MAX_FILL)


def parameters(gsd, fill_rounds=DEFAULTS["fill_rounds"]):
    gsd = _check_gsd(gsd)
    if isinstance(fill_rounds, bool) or int(fill_rounds) != fill_rounds or not 0 <= int(fill_rounds) <= MAX_FILL:
        raise ValueError("fill_rounds=%r must be an integer 0 .. %d" % (fill_rounds, MAX_FILL))
    return dict(fill_rounds=int(fill_rounds))


# ---- step 1: the planes as integers -------------------------------------------------------------------------------------------
def integer_planes(properties, grid, z_ref):
    """properties: the roof stage's, one dict per plane with id 1 .. P in order, `building` and `plane` (z0, sx, sy, xc, yc) ->
    (planes int64 [P, 3] = A, B, C in 2^-20 m, building int32 [P]).  The one path from the properties to the integers: extract()
    and the file route both come through here.  Raises ValueError."""
    gsd, x0, y_top, z_ref = float(grid.gsd), float(grid.x0), float(grid.y_top), float(z_ref)
    planes, bld = [], []
    for k, prop in enumerate(properties, start=1):
        if int(prop["id"]) != k:
            raise ValueError("roof plane %d has id %r: the planes must come in the order of their ids 1 .. P" % (k, prop["id"]))
        pl = prop["plane"]
        z0, sx, sy, xc, yc = (float(pl[n]) for n in ("z0", "sx", "sy", "xc", "yc"))
        a = sx * gsd
        b = -(sy * gsd)
        c = ((z0 + sx * ((x0 + 0.5 * gsd) - xc)) + sy * ((y_top - 0.5 * gsd) - yc)) - z_ref
        if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
            raise ValueError("roof plane %d is not finite: %r" % (k, pl))
        A, B, C = (int(round(v * float(1 << PLANE_BITS))) for v in (a, b, c))     # round(): ties to even, as rint
        if abs(A) >= 1 << 40 or abs(B) >= 1 << 40 or abs(C) >= 1 << 50:
            raise ValueError("roof plane %d is out of range: %g, %g m per cell, %g m above z_ref" % (k, a, b, c))
        for r, cc in ((0, 0), (0, grid.W), (grid.H, 0), (grid.H, grid.W)):
            if abs(corner_height((A, B, C), r, cc)) >= Z_MAX:
                raise ValueError("roof plane %d leaves +-%d m above z_ref inside the grid" % (k, Z_MAX // Z_SCALE))
        if int(prop["building"]) < 1:
            raise ValueError("roof plane %d belongs to building %r" % (k, prop["building"]))
        planes.append((A, B, C))
        bld.append(int(prop["building"]))
    return np.array(planes, np.int64).reshape(-1, 3), np.array(bld, np.int32)


def corner_height(plane, r, c):
    """The height of the integer plane (A, B, C) at lattice corner (r, c) in 1/1024 m, rounded half up: csrc/lod2_plane.h in
    Python integers."""
    A, B, C = (int(v) for v in plane)
    return (A * (2 * c - 1) + B * (2 * r - 1) + 2 * C + 1024) >> 11


# ---- step 3: which buildings get a solid --------------------------------------------------------------------------------------
def refusals(table):
    """table int64 [4, B] (COLUMNS) -> {building: reason} of the buildings that get no solid."""
    out = {}
    for k in range(table.shape[1]):
        cells, filled, base, roof_min = (int(v) for v in table[:, k])
        if cells == 0:
            continue                                                     # a number without cells is no building
        if filled == 0:
            out[k + 1] = "no_plane"
        elif base == MIN_START:
            out[k + 1] = "no_terrain"
        elif base >= roof_min:
            out[k + 1] = "base_not_below_roof"
    return out


# ---- step 5: faces from the runs ----------------------------------------------------------------------------------------------
_LEFT = {(1, 0): (0, 1), (0, 1): (-1, 0), (-1, 0): (0, -1), (0, -1): (1, 0)}     # a quarter turn to the left; x east, y north


def _round_half_up(fr):
    return math.floor(fr + Fraction(1, 2))


def _dedupe(ring):
    out = []
    for v in ring:
        if not out or out[-1] != v:
            out.append(v)
    while len(out) > 1 and out[0] == out[-1]:
        out.pop()
    return out


def _area2(ring):
    """Twice the signed area of the ring's projection (x east, y north): positive = counter-clockwise from above."""
    return sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(ring, ring[1:] + ring[:1]))


def _inside(pt2, ring):
    """Whether the point (in doubled coordinates) lies inside the ring: crossings of the ray towards +x, half-open in y."""
    x, y = pt2
    inside = False
    for a, b in zip(ring, ring[1:] + ring[:1]):
        ax, ay, bx, by = 2 * a[0], 2 * a[1], 2 * b[0], 2 * b[1]
        if (ay > y) != (by > y) and Fraction(x - ax) < Fraction((bx - ax) * (y - ay), by - ay):
            inside = not inside
    return inside


def _rings(segments):
    """segments: [(node_from, node_to, heading, path)] of one region with the region on the left, path = the vertices from one
    node to the other, both included -> the closed rings.  At a node with two ways on, the left turn is taken: two parts of a
    region that touch in a corner only stay two rings."""
    out_at = {}
    for k, s in enumerate(segments):
        out_at.setdefault(s[0], []).append(k)
    nxt = []
    for s in segments:
        cand = out_at.get(s[1], [])
        if not cand:
            raise ValueError("the runs do not close around a region at corner %r" % (s[1],))
        want = [_LEFT[s[2]], s[2], _LEFT[_LEFT[_LEFT[s[2]]]]]
        nxt.append(min(cand, key=lambda k: want.index(segments[k][2]) if segments[k][2] in want else 3))
    if sorted(nxt) != list(range(len(segments))):
        raise ValueError("the runs around a region do not pair up")
    seen, rings = [False] * len(segments), []
    for k0 in range(len(segments)):
        if seen[k0]:
            continue
        ring, k = [], k0
        while not seen[k]:
            seen[k] = True
            ring.extend(segments[k][3][:-1])
            k = nxt[k]
        rings.append(_dedupe(ring))
    return rings


def _polygons(rings):
    """Closed rings of one region (outer rings counter-clockwise, holes clockwise) -> [[outer, hole, ...]]: every hole with the
    smallest outer ring around the midpoint of its first edge."""
    outers = [r for r in rings if _area2(r) > 0]
    holes = [r for r in rings if _area2(r) < 0]
    polys = [[o] for o in outers]
    for h in holes:
        if len(outers) == 1:
            polys[0].append(h)
            continue
        mid = (h[0][0] + h[1][0], h[0][1] + h[1][1])
        around = [k for k, o in enumerate(outers) if _inside(mid, o)]
        if not around:
            raise ValueError("a hole lies in no outer ring")
        polys[min(around, key=lambda k: _area2(outers[k]))].append(h)
    return polys


def faces(records, base, plane_building, H):
    """records: the runs, [10, N] (FIELDS) or N rows of 10 integers; base: the base of building b at base[b - 1] (1/1024 m);
    plane_building: the building of plane p at [p - 1]; H: the rows of the grid -> {building: [face]} in ascending order of the
    buildings, face = dict(kind "roof" / "wall" / "ground", plane (roofs) or None, rings [[(x, y, z)]]: the outer ring first,
    counter-clockwise seen from outside, then the holes).  Vertices are integers: x = 1024 c, y = 1024 (H - r), z in 1/1024 m
    above z_ref.  O(runs); Python integers and Fractions only."""
    if isinstance(records, np.ndarray):
        if records.ndim != 2 or records.shape[0] != len(FIELDS):
            raise ValueError("records as an array must be [%d, N], got %s" % (len(FIELDS), records.shape))
        records = records.T.tolist()
    runs = [tuple(int(v) for v in row) for row in records]
    if any(len(row) != len(FIELDS) for row in runs):
        raise ValueError("a run record has %d fields" % len(FIELDS))
    H = int(H)

    def corner(o, line, pos):                                           # the lattice corner (r, c) at position pos of a line
        return (line, pos) if o == 0 else (pos, line)

    def vertex(o, line, u, z):                                          # u: the position along the line in 1/1024 cell
        return (u, XY_SCALE * (H - line), z) if o == 0 else (XY_SCALE * line, XY_SCALE * H - u, z)

    heights = {}
    for o, line, s, e, L, R, zls, zle, zrs, zre in runs:
        heights.setdefault(corner(o, line, s), set()).update((zls, zrs))
        heights.setdefault(corner(o, line, e), set()).update((zle, zre))

    def vertical(o, line, pos, z_from, z_to):                           # the vertices of a vertical edge, z_to left out
        node = corner(o, line, pos)
        mids = sorted((z for z in heights[node] if min(z_from, z_to) < z < max(z_from, z_to)), reverse=z_from > z_to)
        return [vertex(o, line, XY_SCALE * pos, z) for z in [z_from] + mids]

    solids, roof_segs, ground_segs = {}, {}, {}
    for o, line, s, e, L, R, zls, zle, zrs, zre in runs:
        b = int(plane_building[(L if L else R) - 1])
        if L and R and int(plane_building[R - 1]) != b:
            raise ValueError("buildings %d and %d share a cell edge on %s line %d at %d: two buildings must not be 4-adjacent"
                             % (b, int(plane_building[R - 1]), "horizontal" if o == 0 else "vertical", line, s))
        out = solids.setdefault(b, [])
        S_L, S_R = vertex(o, line, XY_SCALE * s, zls), vertex(o, line, XY_SCALE * s, zrs)
        E_L, E_R = vertex(o, line, XY_SCALE * e, zle), vertex(o, line, XY_SCALE * e, zre)
        d_s, d_e = zls - zrs, zle - zre
        X = None
        if d_s * d_e < 0:
            if not (L and R):
                raise ValueError("building %d: its base crosses a roof plane along a run" % b)
            t = Fraction(d_s, d_s - d_e)
            X = vertex(o, line, _round_half_up(XY_SCALE * (s + t * (e - s))), _round_half_up(zls + t * (zle - zls)))
            walls = [[X] + vertical(o, line, s, zls, zrs) + [S_R], [X] + vertical(o, line, e, zre, zle) + [E_L]]
        elif d_s or d_e:
            walls = [vertical(o, line, e, zre, zle) + [E_L] + vertical(o, line, s, zls, zrs) + [S_R]]
        else:
            walls = []
        for ring in walls:
            ring = _dedupe(ring)
            if len(ring) >= 3:
                out.append(dict(kind="wall", plane=None, rings=[ring]))
        ahead = (1, 0) if o == 0 else (0, -1)                            # a horizontal line runs east, a vertical one south
        back = (-ahead[0], -ahead[1])
        ns, ne = corner(o, line, s), corner(o, line, e)
        mid = [X] if X is not None else []
        if L:
            roof_segs.setdefault(L, []).append((ns, ne, ahead, [S_L] + mid + [E_L]))
        else:
            ground_segs.setdefault(b, []).append((ne, ns, back, [E_L, S_L]))           # backwards: the building on the left
        if R:
            roof_segs.setdefault(R, []).append((ne, ns, back, [E_R] + mid + [S_R]))
        else:
            ground_segs.setdefault(b, []).append((ns, ne, ahead, [S_R, E_R]))
    result = {}
    for b in sorted(solids):
        fs = []
        for p in sorted(p for p in roof_segs if int(plane_building[p - 1]) == b):
            fs += [dict(kind="roof", plane=p, rings=poly) for poly in _polygons(_rings(roof_segs[p]))]
        fs += solids[b]
        for poly in _polygons(_rings(ground_segs.get(b, []))):
            fs.append(dict(kind="ground", plane=None, rings=[r[::-1] for r in poly]))
        result[b] = fs
    return result


def triangulate(rings):
    """One face's rings -> triangles [(v0, v1, v2)]: every hole bridged to the nearest vertex of the ring so far (ties to the
    first), then a fan from the ring's first vertex; triangles with a repeated vertex are left out."""
    ring = list(rings[0])
    for hole in rings[1:]:
        h0 = hole[0]
        k = min(range(len(ring)), key=lambda i: (sum((a - c) ** 2 for a, c in zip(ring[i], h0)), i))
        ring = ring[:k + 1] + list(hole) + [h0] + ring[k:]
    tris = []
    for i in range(1, len(ring) - 1):
        t = (ring[0], ring[i], ring[i + 1])
        if t[0] != t[1] and t[1] != t[2] and t[0] != t[2]:
            tris.append(t)
    return tris


def volume6(tris):
    """Six times the signed volume enclosed by the triangles, an integer."""
    return sum(a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]) for a, b, c in tris)


def edge_census(fs):
    """The directed edges of the faces' rings -> (unmatched: the directed edges that do not occur as often as their reverse,
    over_used: the undirected edges used by more than two faces)."""
    cnt = Counter()
    for f in fs:
        for ring in f["rings"]:
            cnt.update(zip(ring, ring[1:] + ring[:1]))
    unmatched = sum(1 for (a, b), n in cnt.items() if cnt.get((b, a), 0) != n)
    uses = Counter()
    for (a, b), n in cnt.items():
        uses[(min(a, b), max(a, b))] += n
    return unmatched, sum(1 for n in uses.values() if n > 2)


# ---- the stage ----------------------------------------------------------------------------------------------------------------
def _no_gpu():
    return raster_stage.no_gpu("lod2", "LoD2 solid")


def fill(building, start, P, rounds, stop_early=True):
    """The fill rounds on the device: building, start int32 [H, W] (device) -> (label, counts int64 [rounds] (numpy), rounds
    run).  With stop_early the counts are read every FILL_CHUNK rounds and the loop ends after a round that labelled nothing: a
    fixed point, so the labels and the counts (zero from there on) are those of all the rounds."""
    import torch
    from . import hip_ops
    bufs = [start.clone(), torch.empty_like(start)]
    counts = torch.zeros(MAX_FILL, device=start.device, dtype=torch.int32)
    host = np.zeros(rounds, np.int64)
    done = 0
    while done < rounds:
        m = min(FILL_CHUNK, rounds - done)
        hip_ops.lod2_fill(building, P, bufs[0], bufs[1], counts, done, m)
        host[done:done + m] = counts[done:done + m].cpu().numpy()
        done += m
        if stop_early and (host[done - m:done] == 0).any():
            break
    return bufs[done & 1], host, done


def _checked(dtm, building, roof_label, roof_properties, gsd, grid, fill_rounds):
    p = parameters(gsd, fill_rounds)
    dtm = np.ascontiguousarray(dtm, np.float32)
    building, roof_label = np.ascontiguousarray(building), np.ascontiguousarray(roof_label)
    if dtm.ndim != 2 or dtm.shape != building.shape or dtm.shape != roof_label.shape:
        raise ValueError("dtm %s, building %s and roof_label %s must be one [H, W]" % (dtm.shape, building.shape, roof_label.shape))
    for name, a in (("building", building), ("roof_label", roof_label)):
        if a.dtype.kind not in "iu":
            raise ValueError("%s must hold integer labels, got %s" % (name, a.dtype))
    H, W = dtm.shape
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError("the grid is %d x %d cells: at most %d on a side" % (W, H, MAX_SIDE))
    building, roof_label = building.astype(np.int32), roof_label.astype(np.int32)
    gsd = float(gsd)
    if grid is None:
        grid = raster_stage.default_grid(H, W, gsd)
    if (grid.W, grid.H) != (W, H) or float(grid.gsd) != gsd:
        raise ValueError("the grid is %d x %d at gsd %g, the rasters %d x %d at gsd %g" % (grid.W, grid.H, grid.gsd, W, H, gsd))
    z_ref = reference_height(dtm)
    planes, plane_building = integer_planes(roof_properties, grid, z_ref)
    P, B = len(planes), int(building.max()) if building.size else 0
    if building.size and (int(building.min()) < 0 or int(roof_label.min()) < 0 or int(roof_label.max()) > P):
        raise ValueError("labels must be 0 .. N: building %d .. %d, roof_label %d .. %d with %d planes"
                         % (building.min(), building.max(), roof_label.min(), roof_label.max(), P))
    if P and int(plane_building.max()) > B:
        raise ValueError("a roof plane belongs to building %d of %d" % (plane_building.max(), B))
    return p, dtm, building, roof_label, grid, z_ref, planes, plane_building, P, B


def extract(dtm, building, roof_label, roof_properties, gsd, grid=None, fill_rounds=DEFAULTS["fill_rounds"], device=None, stop_early=True):
    """dtm [H, W] float32 (host; NaN where there is no value), building [H, W] int (0 none, 1 .. B), roof_label [H, W] int (0 none,
    planes 1 .. P), roof_properties: the roof stage's properties of the planes 1 .. P -> dict(solids {building: [face]} (faces()),
    buildings (the attributes per solid), refused {building: reason}, label int32 (the model labels, refused buildings zeroed),
    filled int32 (before that), fill_counts, table int64 [4, B] (COLUMNS), records int32 [10, N] (FIELDS), planes int64 [P, 3],
    plane_building, counts, fill_stats, params, z_ref, grid, seconds).  Raises without a GPU: there is no CPU fallback."""
    import torch
    from . import hip_ops
    p, dtm, building, roof_label, grid, z_ref, planes, plane_building, P, B = _checked(dtm, building, roof_label, roof_properties, gsd, grid,
                                                                                       fill_rounds)
    if not torch.cuda.is_available():
        raise _no_gpu()
    H, W = dtm.shape
    dev = torch.device(device if device is not None else "cuda")
    d, b, r = torch.from_numpy(dtm).to(dev), torch.from_numpy(building).to(dev), torch.from_numpy(roof_label).to(dev)
    planes_dev, pb_dev = torch.from_numpy(planes).to(dev), torch.from_numpy(plane_building).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.time()
    owner = torch.cat([torch.zeros(1, device=dev, dtype=torch.int32), pb_dev])[r.long()]       # the building of the cell's plane
    start = torch.where((b > 0) & (owner == b), r, torch.zeros((), device=dev, dtype=torch.int32))
    filled, fill_counts, rounds_run = fill(b, start, P, p["fill_rounds"], stop_early)
    torch.cuda.synchronize(dev)
    t1 = time.time()
    table = hip_ops.lod2_table(d, b, filled, z_ref, B, planes_dev).cpu().numpy()
    refused = refusals(table)
    t2 = time.time()
    ok = np.ones(B + 1, bool)
    ok[0] = False
    for k in refused:
        ok[k] = False
    label_dev = torch.where(torch.from_numpy(ok).to(dev)[b.long()], filled, torch.zeros((), device=dev, dtype=torch.int32))
    base = np.where(table[2] == MIN_START, 0, table[2]) if B else np.zeros(0, np.int64)
    plane_base = base[plane_building - 1].astype(np.int32) if P else np.zeros(0, np.int32)
    records_dev, N = hip_ops.lod2_runs(label_dev, planes_dev, torch.from_numpy(plane_base).to(dev))
    records = records_dev.cpu().numpy()
    t3 = time.time()
    model = solids_from_runs(records, table, refused, plane_building, roof_properties, grid, z_ref)
    t4 = time.time()
    label = label_dev.cpu().numpy()
    counts = dict(model["counts"], planes=P, building_cells=int((building > 0).sum()), cells_with_plane=int((start > 0).sum()),
                  cells_filled=int(fill_counts.sum()), cells_unfilled=int(((label == 0) & ok[building]).sum()))
    model.update(label=label, filled=filled.cpu().numpy(), start=start.cpu().numpy(), fill_counts=fill_counts, table=table, records=records,
                 N=int(N), planes=planes, plane_building=plane_building, counts=counts,
                 fill_stats=dict(rounds=p["fill_rounds"], rounds_run=int(rounds_run), per_round=[int(v) for v in fill_counts[:rounds_run]]),
                 params=p, gsd=float(gsd), seconds=dict(fill=t1 - t0, table=t2 - t1, runs=t3 - t2, faces=t4 - t3))
    return model


def solids_from_runs(records, table, refused, plane_building, roof_properties, grid, z_ref):
    """Step 5 and what the files need, from the runs alone (no GPU): records [10, N], table int64 [4, B], refused {building:
    reason} -> dict(solids, buildings, refused, roof_properties {id: properties}, counts, grid, z_ref)."""
    table = np.asarray(table, np.int64).reshape(len(COLUMNS), -1)
    base = np.where(table[2] == MIN_START, 0, table[2])
    solids = faces(records, base.tolist(), [int(v) for v in plane_building], grid.H)
    buildings, n_faces, over_used, unmatched = {}, Counter(), 0, 0
    for k, fs in solids.items():
        buildings[k] = building_attributes(k, fs, int(base[k - 1]), z_ref, grid.gsd)
        n_faces.update(f["kind"] for f in fs)
        u, o = edge_census(fs)
        unmatched, over_used = unmatched + u, over_used + o
    by_reason = {reason: sum(1 for v in refused.values() if v == reason) for reason in REASONS}
    n_runs = records.shape[1] if isinstance(records, np.ndarray) else len(records)
    counts = dict(buildings=int((table[0] > 0).sum()), solids=len(solids), refused=len(refused), refused_by_reason=by_reason, runs=int(n_runs),
                  faces=dict(roof=n_faces["roof"], wall=n_faces["wall"], ground=n_faces["ground"]), edges_unmatched=unmatched,
                  edges_used_by_more_than_two_faces=over_used)
    return dict(solids=solids, buildings=buildings, refused=dict(refused), roof_properties={int(q["id"]): q for q in roof_properties},
                counts=counts, grid=grid, z_ref=float(z_ref))


def building_attributes(k, fs, base, z_ref, gsd):
    """The attributes of solid k: heights in metres (absolute), the volume from the triangulated faces, the footprint from the
    ground polygon."""
    roof_z = [v[2] for f in fs if f["kind"] == "roof" for ring in f["rings"] for v in ring]
    tris = [t for f in fs for t in triangulate(f["rings"])]
    foot2 = sum(-_area2(ring) for f in fs if f["kind"] == "ground" for ring in f["rings"])
    unit = float(gsd) / XY_SCALE
    return dict(id=int(k), base_m=z_ref + base / Z_SCALE, eave_m=z_ref + min(roof_z) / Z_SCALE, ridge_m=z_ref + max(roof_z) / Z_SCALE,
                roof_planes=sorted({f["plane"] for f in fs if f["kind"] == "roof"}), volume6=int(volume6(tris)),
                volume_m3=volume6(tris) / 6.0 * unit * unit / Z_SCALE, footprint_m2=foot2 / 2.0 * unit * unit)


def from_dsm(prefix, fill_rounds=DEFAULTS["fill_rounds"], device=None, out=None):
    """The grid of dsm_whu.py at the path prefix, the terrain of dtm_whu.py, the labels of buildings_whu.py and the planes of
    roofs_whu.py next to it -> extract()'s dict with `source` added; written to `out` (a path prefix) if given."""
    import torch
    grid = raster_stage.read_grid(prefix)
    hints = (("_dtm.tif", "no terrain (run dtm_whu.py --dsm %s first)"), ("_buildings.tif", "no building labels (run buildings_whu.py --dsm %s first)"),
             ("_roofs.tif", "no roof labels (run roofs_whu.py --dsm %s first)"), ("_roofs.geojson", "no roof planes (run roofs_whu.py --dsm %s first)"))
    for suffix, hint in hints:
        raster_stage.require(prefix + suffix, hint % prefix)
    if not torch.cuda.is_available():
        raise _no_gpu()
    shape = (grid.H, grid.W)
    says = "the grid %s" % (shape,)
    dtm = raster_stage.read_raster(prefix + "_dtm.tif", np.float32, shape, says=says)
    building = raster_stage.read_raster(prefix + "_buildings.tif", np.int32, shape, says=says)
    roof_label = raster_stage.read_raster(prefix + "_roofs.tif", np.int32, shape, says=says)
    with open(prefix + "_roofs.geojson") as f:
        props = [feat["properties"] for feat in json.load(f)["features"]]
    res = extract(dtm, building, roof_label, props, grid.gsd, grid, fill_rounds, device)
    res["source"] = dict(prefix=prefix)
    if out is not None:
        write_outputs(out, res)
    return res


# ---- files --------------------------------------------------------------------------------------------------------------------
def output_paths(out):
    """The files of this stage, disjoint from those of every earlier stage."""
    return dict(cityjson=out + "_lod2.city.json", obj=out + "_lod2.obj", json=out + "_lod2.json")


_SEMANTICS = dict(roof="RoofSurface", wall="WallSurface", ground="GroundSurface")


def transform(grid, z_ref):
    unit = float(grid.gsd) / XY_SCALE
    return dict(scale=[unit, unit, 1.0 / Z_SCALE], translate=[float(grid.x0), float(grid.y_top) - grid.H * float(grid.gsd), float(z_ref)])


def cityjson(res):
    """CityJSON 1.1 as a dict: one Building per solid, one Solid of lod "2" with one outer shell, semantics per surface, integer
    vertices (each once, in the order of their first use) under the transform."""
    index, vertices, objects = {}, [], {}

    def vid(v):
        if v not in index:
            index[v] = len(vertices)
            vertices.append(list(v))
        return index[v]

    for k, fs in res["solids"].items():
        surfaces, values, shell = [], [], []
        for f in fs:
            sem = dict(type=_SEMANTICS[f["kind"]])
            if f["kind"] == "roof":
                q = res["roof_properties"][f["plane"]]
                sem.update(plane=int(f["plane"]), slope_deg=q.get("slope_deg"), aspect_deg=q.get("aspect_deg"))
            values.append(len(surfaces))
            surfaces.append(sem)
            shell.append([[vid(v) for v in ring] for ring in f["rings"]])
        a = res["buildings"][k]
        attributes = dict(id=a["id"], base_m=a["base_m"], eave_m=a["eave_m"], ridge_m=a["ridge_m"], roof_planes=a["roof_planes"],
                          volume_m3=a["volume_m3"], footprint_m2=a["footprint_m2"])
        objects["building_%d" % k] = dict(type="Building", attributes=attributes,
                                          geometry=[dict(type="Solid", lod="2", boundaries=[shell],
                                                         semantics=dict(surfaces=surfaces, values=[values]))])
    return dict(type="CityJSON", version="1.1", transform=transform(res["grid"], res["z_ref"]), CityObjects=objects, vertices=vertices)


def obj_text(res):
    """The faces as triangles (triangulate()), one `o` per building, the vertices of the whole file numbered once in the order of
    their first use, in world coordinates through the transform."""
    tf = transform(res["grid"], res["z_ref"])
    index, lines_v, lines_f = {}, [], []
    for k, fs in res["solids"].items():
        lines_f.append("o building_%d" % k)
        for f in fs:
            for tri in triangulate(f["rings"]):
                ids = []
                for v in tri:
                    if v not in index:
                        index[v] = len(index) + 1
                        lines_v.append("v %r %r %r" % tuple(tf["translate"][i] + v[i] * tf["scale"][i] for i in range(3)))
                    ids.append(index[v])
                lines_f.append("f %d %d %d" % tuple(ids))
    return "\n".join(["# LoD2 building solids: %d buildings" % len(res["solids"])] + lines_v + lines_f) + "\n"


def summary(res, seconds=True):
    s = dict(grid=raster_stage.grid_summary(res["grid"]), source=res.get("source"), params=res["params"], z_ref=res["z_ref"],
             transform=transform(res["grid"], res["z_ref"]), counts=res["counts"],
             refused={str(k): v for k, v in sorted(res["refused"].items())}, fill_stats=res["fill_stats"])
    if seconds:
        s["seconds"] = res["seconds"]
    return s


def write_outputs(out, res, seconds=True):
    """The CityJSON, the OBJ and the JSON summary at the path prefix `out` -> output_paths(out).  seconds=False leaves the
    timings out of the summary: every byte of the three files is then the same from run to run."""
    texts = dict(cityjson=json.dumps(cityjson(res), separators=(",", ":")) + "\n", obj=obj_text(res))
    return raster_stage.write_outputs(output_paths(out), out, texts, summary(res, seconds))


def read_outputs(out):
    """-> (the CityJSON as a dict, the OBJ as (vertices [(x, y, z)], {object: [(i, j, k)]} with 0-based indices), the summary)."""
    paths = output_paths(out)
    city, js = raster_stage.read_outputs(paths, ("cityjson",))
    verts, objects, cur = [], {}, None
    with open(paths["obj"]) as f:
        for line in f:
            w = line.split()
            if not w or w[0] == "#":
                continue
            if w[0] == "v":
                verts.append(tuple(float(x) for x in w[1:4]))
            elif w[0] == "o":
                cur = objects.setdefault(w[1], [])
            elif w[0] == "f":
                cur.append(tuple(int(x) - 1 for x in w[1:4]))
    return city, (verts, objects), js


def build_parser():
    ap = argparse.ArgumentParser(description="Join footprints, roof planes and terrain into LoD2 building solids")
    ap.add_argument("--dsm", required=True, metavar="PREFIX", help="path prefix of the earlier stages' output (<PREFIX>_dsm.json, "
                    "<PREFIX>_dtm.tif, <PREFIX>_buildings.tif, <PREFIX>_roofs.tif, <PREFIX>_roofs.geojson)")
    ap.add_argument("--fill_rounds", type=int, default=DEFAULTS["fill_rounds"],
                    help="rounds in which a building cell without a plane takes a neighbour's (at most %d)" % MAX_FILL)
    ap.add_argument("--out", default=None, metavar="PREFIX", help="output path prefix (default: --dsm): <out>_lod2.city.json, ...")
    return ap


def main(argv=None):
    args, out, t0 = raster_stage.open_main(build_parser, argv)
    res = from_dsm(args.dsm, args.fill_rounds, out=out)
    g, c, s = res["grid"], res["counts"], res["seconds"]
    print("lod2 %d x %d cells at gsd %g: %d buildings, %d planes, %d cells filled in %d rounds; %d solids, %d refused %s"
          % (g.W, g.H, g.gsd, c["buildings"], c["planes"], c["cells_filled"], res["fill_stats"]["rounds_run"], c["solids"], c["refused"],
             c["refused_by_reason"]))
    print("%d runs; %d roof, %d wall, %d ground faces, %d edges used by more than two faces; fill %.3f s, table %.3f s, runs %.3f s, "
          "faces %.3f s; total_time = %.3f s"
          % (c["runs"], c["faces"]["roof"], c["faces"]["wall"], c["faces"]["ground"], c["edges_used_by_more_than_two_faces"], s["fill"],
             s["table"], s["runs"], s["faces"], time.time() - t0))
    return res


if __name__ == "__main__":
    main()
