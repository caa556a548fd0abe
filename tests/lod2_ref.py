"""numpy / Python-integer restatement of include/adamvs_hip.h "LoD2 solids", written from the header's text and sharing nothing
with the kernels: steps 1 - 4 literally (integer planes, corner heights, the fill rounds with their counts, the building table,
the run records) and step 5 as what the header promises of the faces (check_solid: closed, outward, planar) with the volume the
cells themselves give (volume_ref).  The scenes of the host and the GPU tests are here too, so both run the same ones."""
import json
from collections import Counter
from fractions import Fraction

import numpy as np

from ada_mvs_amd import dsm

MAX_FILL = 1024
MIN_START = 2 ** 31 - 1
FIELDS = ("orientation", "line", "start", "end", "L", "R", "zL_s", "zL_e", "zR_s", "zR_e")


# ---- step 1 -------------------------------------------------------------------------------------------------------------------
def integer_planes_ref(properties, grid, z_ref):
    out = []
    for q in properties:
        pl = q["plane"]
        z0, sx, sy, xc, yc = (np.float64(pl[k]) for k in ("z0", "sx", "sy", "xc", "yc"))
        gsd, x0, y_top = np.float64(grid.gsd), np.float64(grid.x0), np.float64(grid.y_top)
        a = sx * gsd
        b = -(sy * gsd)
        c = ((z0 + sx * ((x0 + np.float64(0.5) * gsd) - xc)) + sy * ((y_top - np.float64(0.5) * gsd) - yc)) - np.float64(z_ref)
        out.append([int(np.rint(v * np.float64(2 ** 20))) for v in (a, b, c)])
    return np.array(out, np.int64).reshape(-1, 3), np.array([int(q["building"]) for q in properties], np.int32)


def corner_height_ref(plane, r, c):
    A, B, C = (int(v) for v in plane)
    return (A * (2 * c - 1) + B * (2 * r - 1) + 2 * C + 2 ** 10) // 2 ** 11          # // floors: round half up


def corner_grid(plane, H, W):
    """zq at every corner, int64 [H + 1, W + 1]."""
    A, B, C = (int(v) for v in plane)
    r, c = np.mgrid[0:H + 1, 0:W + 1].astype(np.int64)
    return (A * (2 * c - 1) + B * (2 * r - 1) + 2 * C + 2 ** 10) // 2 ** 11


# ---- step 2 -------------------------------------------------------------------------------------------------------------------
def start_labels(building, roof, plane_building):
    P = len(plane_building)
    owner = np.concatenate([[0], np.asarray(plane_building, np.int64)])[np.clip(roof, 0, P)]
    ok = (roof >= 1) & (roof <= P) & (building > 0) & (owner == building)
    return np.where(ok, roof, 0).astype(np.int32)


def fill_ref(building, start, P, rounds):
    """-> (labels after `rounds` rounds, counts int64 [rounds])."""
    H, W = building.shape
    lab = np.where((start >= 1) & (start <= P), start, 0).astype(np.int64)
    counts = np.zeros(rounds, np.int64)
    big = np.int64(2 ** 40)
    for k in range(rounds):
        best = np.full((H, W), big)
        for di, dj in ((-1, 0), (0, -1), (0, 1), (1, 0)):
            nl = np.zeros((H, W), np.int64)
            nb = np.zeros((H, W), np.int64)
            dst = (slice(max(0, -di), H - max(0, di)), slice(max(0, -dj), W - max(0, dj)))
            src = (slice(max(0, di), H - max(0, -di)), slice(max(0, dj), W - max(0, -dj)))
            nl[dst], nb[dst] = lab[src], building[src]
            cand = (nl > 0) & (nb == building)
            best = np.where(cand & (nl < best), nl, best)
        take = (building > 0) & (lab == 0) & (best < big)
        new = np.where(take, best, lab)
        new[building <= 0] = 0
        counts[k] = int(take.sum())
        lab = new
        if counts[k] == 0:
            break                                                            # a fixed point: the rest of the counts are 0
    return lab.astype(np.int32), counts


# ---- step 3 -------------------------------------------------------------------------------------------------------------------
def table_ref(dtm, building, label, z_ref, B, planes):
    H, W = building.shape
    table = np.zeros((4, B), np.int64)
    table[2:] = MIN_START
    P = len(planes)
    grids = {}
    for i in range(H):
        for j in range(W):
            b = int(building[i, j])
            if b < 1 or b > B:
                continue
            table[0, b - 1] += 1
            z = np.float64(dtm[i, j])
            if np.isfinite(z):
                v = int(min(max(np.floor((z - np.float64(z_ref)) * np.float64(1024.0)), -2.0 ** 30), 2.0 ** 30))
                table[2, b - 1] = min(table[2, b - 1], v)
            p = int(label[i, j])
            if 1 <= p <= P:
                table[1, b - 1] += 1
                g = grids.setdefault(p, corner_grid(planes[p - 1], H, W))
                table[3, b - 1] = min(table[3, b - 1], int(g[i:i + 2, j:j + 2].min()))
    return table


def refused_ref(table):
    out = {}
    for k in range(table.shape[1]):
        cells, filled, base, roof_min = (int(v) for v in table[:, k])
        if cells and filled == 0:
            out[k + 1] = "no_plane"
        elif cells and base == MIN_START:
            out[k + 1] = "no_terrain"
        elif cells and base >= roof_min:
            out[k + 1] = "base_not_below_roof"
    return out


def zero_refused(label, building, refused):
    out = label.copy()
    for k in refused:
        out[building == k] = 0
    return out


# ---- step 4 -------------------------------------------------------------------------------------------------------------------
def runs_ref(label, planes, plane_base):
    """-> the records as a list of 10-tuples in ascending (orientation, line, start)."""
    H, W = label.shape
    P = len(planes)
    m = np.where((label >= 1) & (label <= P), label, 0).astype(np.int64)
    pad = np.zeros((H + 2, W + 2), np.int64)
    pad[1:-1, 1:-1] = m

    def side(q, other, r, c):
        return corner_height_ref(planes[q - 1], r, c) if q else int(plane_base[other - 1])

    out = []
    for o in (0, 1):
        n_lines, n_pos = (H + 1, W) if o == 0 else (W + 1, H)
        for k in range(n_lines):
            if o == 0:
                Ls, Rs = pad[k, 1:-1], pad[k + 1, 1:-1]                      # north of the line, south of it
            else:
                Ls, Rs = pad[1:-1, k + 1], pad[1:-1, k]                      # east of the line, west of it
            pos = 0
            while pos < n_pos:
                L, R = int(Ls[pos]), int(Rs[pos])
                if L == R:
                    pos += 1
                    continue
                end = pos + 1
                while end < n_pos and int(Ls[end]) == L and int(Rs[end]) == R:
                    end += 1
                cs, ce = ((k, pos), (k, end)) if o == 0 else ((pos, k), (end, k))
                out.append((o, k, pos, end, L, R, side(L, R, *cs), side(L, R, *ce), side(R, L, *cs), side(R, L, *ce)))
                pos = end
    return out


def records_array(runs):
    return np.array(runs, np.int64).reshape(-1, 10).T.astype(np.int32)


def run_ref(dtm, building, roof, properties, grid, rounds=MAX_FILL):
    """Steps 1 - 4 -> dict(planes, plane_building, z_ref, start, filled, counts, table, refused, label, plane_base, runs)."""
    fin = dtm[np.isfinite(dtm)]
    z_ref = float(np.floor(fin.min())) if fin.size else 0.0
    planes, pb = integer_planes_ref(properties, grid, z_ref)
    B = int(building.max())
    start = start_labels(building, roof, pb)
    filled, counts = fill_ref(building, start, len(planes), rounds)
    table = table_ref(dtm, building, filled, z_ref, B, planes)
    refused = refused_ref(table)
    label = zero_refused(filled, building, refused)
    base = np.where(table[2] == MIN_START, 0, table[2])
    plane_base = base[pb - 1].astype(np.int32) if len(pb) else np.zeros(0, np.int32)
    return dict(planes=planes, plane_building=pb, z_ref=z_ref, start=start, filled=filled, counts=counts, table=table, refused=refused,
                label=label, plane_base=plane_base, base=base, runs=runs_ref(label, planes, plane_base))


# ---- step 5: what the header promises of the faces ---------------------------------------------------------------------------
def _normal2(ring):
    """Newell's sum: twice the area vector of the ring."""
    n = [0, 0, 0]
    for a, b in zip(ring, ring[1:] + ring[:1]):
        n[0] += (a[1] - b[1]) * (a[2] + b[2])
        n[1] += (a[2] - b[2]) * (a[0] + b[0])
        n[2] += (a[0] - b[0]) * (a[1] + b[1])
    return n


def directed_edges(rings_of_faces):
    cnt = Counter()
    for rings in rings_of_faces:
        for ring in rings:
            cnt.update(zip(ring, ring[1:] + ring[:1]))
    return cnt


def volume6_of_triangles(tris):
    return sum(a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]) for a, b, c in tris)


def fan(rings):
    """A fan per ring from its first vertex: the signed volume under a face with holes is the sum over its rings."""
    return [(r[0], r[i], r[i + 1]) for r in rings for i in range(1, len(r) - 1)]


def check_solid(fs, planes, H, base):
    """The faces of one solid against the header: every directed edge as often as its reverse; roofs up, ground down, walls
    vertical; every face within one unit (1/1024 m) of a plane (roofs: the plane's own equation, exactly evaluated); 6 V > 0.
    -> 6 V as an integer."""
    cnt = directed_edges(f["rings"] for f in fs)
    bad = [(e, n, cnt.get((e[1], e[0]), 0)) for e, n in cnt.items() if cnt.get((e[1], e[0]), 0) != n]
    assert not bad, bad[:5]
    kinds = Counter(f["kind"] for f in fs)
    assert kinds["roof"] >= 1 and kinds["ground"] >= 1 and kinds["wall"] >= 3
    for f in fs:
        n = _normal2(f["rings"][0])
        for ring in f["rings"]:
            assert len(ring) >= 3 and len(set(ring)) == len(ring), ring
        if f["kind"] == "roof":
            assert n[2] > 0
            A, B, C = (int(v) for v in planes[f["plane"] - 1])
            for ring in f["rings"]:
                for x, y, z in ring:
                    # the plane at column x / 1024 - 1/2 and row H - y / 1024 - 1/2 of the cell-centre frame, in 1/1024 m
                    want = (Fraction(A) * (Fraction(x, 1024) - Fraction(1, 2)) + Fraction(B) * (H - Fraction(y, 1024) - Fraction(1, 2)) + C) / 1024
                    assert abs(want - z) <= 1, (f["plane"], (x, y, z), float(want))
        elif f["kind"] == "ground":
            assert n[2] < 0 and n[0] == 0 and n[1] == 0
            assert {v[2] for ring in f["rings"] for v in ring} == {base}
        else:
            assert n[2] == 0 and (n[0] == 0) != (n[1] == 0), n
            (ring,) = f["rings"]
            assert len({v[0] for v in ring}) == 1 or len({v[1] for v in ring}) == 1       # in one vertical lattice plane
    v6 = volume6_of_triangles([t for f in fs for t in fan(f["rings"])])
    assert v6 > 0
    return v6


def volume_ref(label, building, k, planes, base, gsd):
    """Sum over the cells of building k of (plane height at the cell centre - base) gsd^2 in m^3, as a Fraction, and the footprint."""
    vol, cells = Fraction(0), 0
    for i, j in zip(*np.nonzero((building == k) & (label > 0))):
        A, B, C = (int(v) for v in planes[int(label[i, j]) - 1])
        vol += Fraction(A * int(j) + B * int(i) + C, 2 ** 20) - Fraction(int(base), 1024)
        cells += 1
    g2 = Fraction(gsd) ** 2
    return vol * g2, cells * g2


def check_model(model, label, building, planes, base, gsd):
    """Every solid of lod2.solids_from_runs() / lod2.extract(): check_solid, and its volume in m^3 within footprint x 2 / 1024 m of
    the cells' own (half a unit per corner, at most one at a crossing).  -> {building: (6 V, the difference in m^3, the bound)}."""
    from ada_mvs_amd import lod2
    out = {}
    H = label.shape[0]
    for k, fs in model["solids"].items():
        v6 = check_solid(fs, planes, H, int(base[k - 1]))
        tris = [t for f in fs for t in lod2.triangulate(f["rings"])]
        assert lod2.volume6(tris) == model["buildings"][k]["volume6"] > 0             # what the OBJ's triangles enclose
        want, foot = volume_ref(label, building, k, planes, base[k - 1], gsd)
        bound = foot * 2 / 1024
        for v in (model["buildings"][k]["volume6"], v6):                             # the bridged fans, and a fan per ring
            got = Fraction(v, 6) * Fraction(gsd) ** 2 / 1024 ** 3
            print("building %d: volume %.6f m3, the cells' %.6f, difference %.6f (bound %.6f)" % (k, got, want, abs(got - want), bound))
            assert abs(got - want) <= bound
        a = model["buildings"][k]
        got = Fraction(a["volume6"], 6) * Fraction(gsd) ** 2 / 1024 ** 3
        assert abs(a["volume_m3"] - float(got)) <= 1e-9 * float(got) and a["footprint_m2"] == float(foot)
        assert a["eave_m"] <= a["ridge_m"] and a["base_m"] < a["eave_m"]
        out[k] = (v6, abs(got - want), bound)
    assert model["counts"]["edges_unmatched"] == 0 and model["counts"]["solids"] == len(model["solids"])
    return out


def check_files(out, model, label):
    """lod2.write_outputs(out, model) read back: the CityJSON parses, its boundaries index into its vertices, the semantics cover
    every surface, the transform gives the footprint corners' world coordinates exactly, and the OBJ holds the same vertices
    and a closed triangle shell per building."""
    from ada_mvs_amd import lod2
    lod2.write_outputs(out, model)
    city, (verts, objects), js = lod2.read_outputs(out)
    grid = model["grid"]
    assert city["type"] == "CityJSON" and city["version"] == "1.1"
    tf = city["transform"]
    assert tf["scale"] == [grid.gsd / 1024, grid.gsd / 1024, 1 / 1024]
    assert tf["translate"] == [grid.x0, grid.y_top - grid.H * grid.gsd, model["z_ref"]]
    V = city["vertices"]
    assert all(len(v) == 3 and all(isinstance(x, int) for x in v) for v in V) and len({tuple(v) for v in V}) == len(V)
    assert sorted(city["CityObjects"]) == sorted("building_%d" % k for k in model["solids"])
    used = set()
    for k, fs in model["solids"].items():
        obj = city["CityObjects"]["building_%d" % k]
        (geom,) = obj["geometry"]
        assert obj["type"] == "Building" and geom["type"] == "Solid" and geom["lod"] == "2" and len(geom["boundaries"]) == 1
        (shell,) = geom["boundaries"]
        (values,) = geom["semantics"]["values"]
        surfaces = geom["semantics"]["surfaces"]
        assert len(values) == len(shell) == len(fs) and all(0 <= v < len(surfaces) for v in values)
        assert {surfaces[v]["type"] for v in values} == {"RoofSurface", "WallSurface", "GroundSurface"}
        for f, surface, v in zip(fs, shell, values):
            assert surfaces[v]["type"] == dict(roof="RoofSurface", wall="WallSurface", ground="GroundSurface")[f["kind"]]
            if f["kind"] == "roof":
                q = model["roof_properties"][f["plane"]]
                assert (surfaces[v]["plane"], surfaces[v]["slope_deg"], surfaces[v]["aspect_deg"]) == (f["plane"], q["slope_deg"], q["aspect_deg"])
            assert [[tuple(V[i]) for i in ring] for ring in surface] == [[tuple(p) for p in ring] for ring in f["rings"]]
            used.update(i for ring in surface for i in ring)
        for key in ("id", "base_m", "eave_m", "ridge_m", "roof_planes", "volume_m3", "footprint_m2"):
            assert obj["attributes"][key] == model["buildings"][k][key]
        # the footprint corners: the ground face's vertices are lattice corners, and the transform puts them where the grid does
        for f in fs:
            if f["kind"] == "ground":
                for x, y, z in (p for ring in f["rings"] for p in ring):
                    assert x % 1024 == 0 and y % 1024 == 0
                    c, r = x // 1024, grid.H - y // 1024
                    wx = Fraction(tf["translate"][0]) + x * Fraction(tf["scale"][0])
                    wy = Fraction(tf["translate"][1]) + y * Fraction(tf["scale"][1])
                    assert wx == Fraction(grid.x0) + c * Fraction(grid.gsd) and wy == Fraction(grid.y_top) - r * Fraction(grid.gsd)
                    assert (label[max(r - 1, 0):r + 1, max(c - 1, 0):c + 1] > 0).any()       # a corner of a model cell
        # the OBJ: the same vertices, a closed shell of triangles
        tris = objects["building_%d" % k]
        cnt = Counter(e for t in tris for e in zip(t, t[1:] + t[:1]))
        assert tris and all(cnt.get((b, a), 0) == n for (a, b), n in cnt.items())
    assert used == set(range(len(V)))
    world = {tuple(tf["translate"][i] + v[i] * tf["scale"][i] for i in range(3)) for v in V}
    assert set(verts) == world and len(verts) == len(V)
    assert js["counts"] == json.loads(json.dumps(model["counts"])) and js["transform"] == tf
    return city, js


# ---- scenes -------------------------------------------------------------------------------------------------------------------
GSD = 0.5


def _grid(H, W, x0=1000.0, y0=2000.0):
    return dsm.Grid(x0, y0 + H * GSD, GSD, 0.0, W, H)


def _prop(k, b, a, bb, c, grid):
    """The roof stage's properties of plane k of building b: z = a j + bb i + c (metres per cell; c at the centre of cell (0, 0))."""
    import math
    sx, sy = a / grid.gsd, -bb / grid.gsd
    uc, vc = 3.0, 2.0                                                        # any cell: the equation is the same plane
    slope = math.degrees(math.atan(math.hypot(sx, sy)))
    return dict(id=k, building=b, slope_deg=slope, aspect_deg=None if slope < 5.0 else math.degrees(math.atan2(-sx, -sy)) % 360.0,
                plane=dict(z0=a * uc + bb * vc + c, sx=sx, sy=sy, xc=grid.x0 + (uc + 0.5) * grid.gsd,
                           yc=grid.y_top - (vc + 0.5) * grid.gsd))


def _terrain(H, W):
    i, j = np.mgrid[0:H, 0:W]
    return (3.0 + j / 64.0 + i / 128.0).astype(np.float32)


def _lowest(planes_abc, H, W):
    """The label raster of a roof that is the lower envelope of the planes at the cell centres (ties to the smaller id)."""
    i, j = np.mgrid[0:H, 0:W]
    z = np.stack([a * j + b * i + c for a, b, c in planes_abc])
    return (np.argmin(z, axis=0) + 1).astype(np.int32)


def scene(name, shift=(0, 0)):
    """-> dict(dtm, building, roof, properties, grid): the scene moved by `shift` = (rows, columns) whole cells inside a larger
    grid, planes and terrain with it."""
    di, dj = shift
    H, W = 22 + di, 26 + dj
    grid = _grid(H, W)
    building = np.zeros((H, W), np.int32)
    roof = np.zeros((H, W), np.int32)
    abc = []                                                                 # (building, a, b, c) in the unshifted frame

    def box(i0, i1, j0, j1):
        return (slice(i0 + di, i1 + di), slice(j0 + dj, j1 + dj))

    if name in ("gable", "gable_rough"):                                     # the ridge runs obliquely to the lattice: crossings
        building[box(3, 19, 4, 22)] = 1
        abc = [(1, 0.25, 0.0625, 6.0), (1, -0.25, 0.03125, 12.5)]
        if name == "gable_rough":                                            # slopes that are no dyadic numbers: every corner rounds
            abc = [(1, 0.3, 0.07, 6.01), (1, -0.23, 0.031, 12.47)]
        lab = _lowest([p[1:] for p in abc], 22, 26)
        roof[box(3, 19, 4, 22)] = lab[3:19, 4:22]
        roof[box(8, 11, 9, 12)] = 0                                          # a patch the roof stage left open: the fill closes it
    elif name == "hip":
        building[box(4, 18, 3, 23)] = 1
        abc = [(1, 0.25, 0.0, 7.0 - 0.25 * 3), (1, -0.25, 0.0, 7.0 + 0.25 * 22), (1, 0.0, 0.25, 7.0 - 0.25 * 4), (1, 0.0, -0.25, 7.0 + 0.25 * 17)]
        lab = _lowest([p[1:] for p in abc], 22, 26)
        roof[box(4, 18, 3, 23)] = lab[4:18, 3:23]
    elif name == "penthouse":                                                # steps, and a corner where three heights meet
        building[box(3, 19, 3, 23)] = 1
        roof[box(3, 19, 3, 23)] = 1
        roof[box(6, 12, 8, 16)] = 2
        roof[box(12, 19, 8, 23)] = 3
        abc = [(1, 0.0, 0.0, 10.0), (1, 0.0, 0.0, 13.0), (1, 0.0, 0.0, 11.5)]
    elif name == "courtyard":                                                # an L with a hole: holes in roof and ground
        building[box(2, 20, 2, 12)] = 1
        building[box(12, 20, 12, 24)] = 1
        building[box(5, 9, 5, 9)] = 0
        roof[building > 0] = 1
        abc = [(1, 0.125, 0.0625, 9.0)]
    elif name == "corner":                                                   # 2 x 2 blocks of four planes around one corner
        building[box(4, 16, 4, 16)] = 1
        roof[box(4, 10, 4, 10)], roof[box(4, 10, 10, 16)], roof[box(10, 16, 4, 10)], roof[box(10, 16, 10, 16)] = 1, 2, 3, 4
        abc = [(1, 0.0, 0.0, 9.0), (1, 0.125, 0.0, 10.0), (1, 0.0, -0.125, 12.0), (1, 0.0625, 0.0625, 8.0)]
    elif name == "pinch":                                                    # two planes, each in two blocks that touch in a corner
        building[box(4, 16, 4, 16)] = 1
        roof[box(4, 10, 4, 10)], roof[box(4, 10, 10, 16)], roof[box(10, 16, 4, 10)], roof[box(10, 16, 10, 16)] = 1, 2, 2, 1
        abc = [(1, 0.0, 0.0, 9.0), (1, 0.125, 0.0, 10.0)]
    elif name == "two":                                                      # building 2 has no plane at all: refused and counted
        building[box(3, 12, 3, 12)] = 1
        building[box(14, 20, 15, 24)] = 2
        roof[box(3, 12, 3, 12)] = 1
        roof[box(5, 7, 5, 7)] = 0
        abc = [(1, -0.125, 0.25, 8.0)]
    else:
        raise KeyError(name)
    # the plane through the shifted cells: z = a (j - dj) + b (i - di) + c
    props = [_prop(k, b, a, bb, c - a * dj - bb * di, grid) for k, (b, a, bb, c) in enumerate(abc, start=1)]
    terrain = np.full((H, W), np.nan, np.float32)
    terrain[di:, dj:] = _terrain(22, 26)
    terrain[:di, :] = 3.0
    terrain[:, :dj] = 3.0
    return dict(dtm=terrain, building=building, roof=roof, properties=props, grid=grid)


def write_inputs(folder, sc, upto=5):
    """The files the stage reads, each written by the writer of the stage it comes from (dsm.write_outputs, dtm.write_outputs,
    and raster_stage.write_outputs with the building and the roof stage's paths), as far as `upto` says (1 the DSM stage's, 2 the
    ground filter's, 3 the building labels, 4 the plane labels, 5 the planes) -> the path prefix.  The surface is the terrain
    itself where there is no building: only the grid of the DSM stage's files is read."""
    import os
    from ada_mvs_amd import buildings, dsm as dsm_stage, dtm as dtm_stage, raster_stage, roofs
    prefix = os.path.join(str(folder), "dsm")
    g = sc["grid"]
    H, W = sc["dtm"].shape
    if upto >= 1:
        dsm_stage.write_outputs(prefix, dict(dsm=sc["dtm"], count=np.ones((H, W), np.uint16), rgba=np.zeros((H, W, 4), np.uint8), grid=g, mode="max",
                                             min_count=1, points_read=H * W, points_used=H * W, cells_filled=H * W))
    if upto >= 2:
        dtm_stage.write_outputs(prefix, dict(dtm=sc["dtm"], ndsm=np.zeros((H, W), np.float32), level=np.zeros((H, W), np.uint8), grid=g,
                                             params=dict(), radius=[], dh=[], counts=dict(), fill=None, seconds=dict()))
    if upto >= 3:
        raster_stage.write_outputs(buildings.output_paths(prefix), prefix, dict(geojson=buildings.geojson_text([], [])), dict(), sc["building"], g)
    if upto >= 4:
        polys = [dict(id=q["id"], rings=[[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0)]]) for q in sc["properties"]] if upto >= 5 else []
        raster_stage.write_outputs(roofs.output_paths(prefix), prefix, dict(geojson=buildings.geojson_text(polys, sc["properties"][:len(polys)])),
                                   dict(), sc["roof"], g)
        if upto < 5:
            os.remove(prefix + "_roofs.geojson")
    return prefix


SCENES = ("gable", "gable_rough", "hip", "penthouse", "courtyard", "corner", "pinch", "two")
DYADIC = ("gable", "hip", "penthouse", "courtyard", "corner", "pinch", "two")     # a whole-cell shift moves these exactly
