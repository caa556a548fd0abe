"""Building extraction, host side: the vectoriser, the simplifier and the selection of ada_mvs_amd/buildings.py on hand-made label
rasters and tables, the numpy restatement (tests/buildings_ref.py) against hand-computed cases and on the roof scene, the
parameter checks, the file names, the ABI and the CLI."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, buildings, dsm, dtm
from buildings_ref import (COLUMNS, cell_parameters, checkerboard_mask, comb_mask, components_ref, extract_ref, flags_ref, mask_ref,
                           random_mask_raster, rasters_of_mask, rings_mask, roof_scene, select_ref, serpentine_mask, table_ref)
from conftest import ROOT
from dtm_ref import open_brute

GRID = dsm.Grid(1000.0, 5000.0, 0.5, 0.0, 64, 48)                      # gsd a power of two: every coordinate and area is exact


def shoelace(ring):
    return 0.5 * sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1]))


def inside_even_odd(rings, x, y):
    """Even-odd rule over all rings, for points that lie on no edge: crossings of the ray towards +x."""
    n = 0
    for ring in rings:
        for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1]):
            if (y0 > y) != (y1 > y) and x < x0 + (y - y0) * (x1 - x0) / (y1 - y0):
                n += 1
    return n % 2 == 1


def check_polygons(label, grid=GRID):
    """Every property the outlines must have on any label raster -> the polygons."""
    polys = buildings.polygons(label, grid)
    ids = sorted(set(np.unique(label).tolist()) - {0})
    assert [p["id"] for p in polys] == ids
    H, W = label.shape
    for p in polys:
        rings = p["rings"]
        areas = [shoelace(r) for r in rings]
        assert areas[0] > 0 and all(a < 0 for a in areas[1:])           # one exterior ring, counter-clockwise; holes clockwise
        assert sum(areas) == (label == p["id"]).sum() * grid.gsd ** 2   # exactly
        for r in rings:
            corners = [((grid.y_top - y) / grid.gsd, (x - grid.x0) / grid.gsd) for x, y in r]
            assert all(float(a).is_integer() and float(b).is_integer() for a, b in corners)
            assert min(corners) == corners[0]                            # starts at its smallest (row, column) corner
            for a, b, c in zip(r, r[1:] + r[:1], r[2:] + r[:2]):         # axis-parallel edges, a turn at every vertex
                assert (a[0] == b[0]) != (a[1] == b[1]) and (a[0] == b[0]) != (b[0] == c[0])
        starts = [((grid.y_top - r[0][1]) / grid.gsd, (r[0][0] - grid.x0) / grid.gsd) for r in rings[1:]]
        assert starts == sorted(starts)                                  # holes in the order of that corner
        i0, i1 = max(0, int(min((grid.y_top - y) / grid.gsd for x, y in rings[0])) - 1), min(H, int(max((grid.y_top - y) / grid.gsd for x, y in rings[0])) + 1)
        j0, j1 = max(0, int(min((x - grid.x0) / grid.gsd for x, y in rings[0])) - 1), min(W, int(max((x - grid.x0) / grid.gsd for x, y in rings[0])) + 1)
        for i in range(i0, i1):
            for j in range(j0, j1):
                centre = (grid.x0 + (j + 0.5) * grid.gsd, grid.y_top - (i + 0.5) * grid.gsd)
                assert inside_even_odd(rings, *centre) == (label[i, j] == p["id"]), (p["id"], i, j)
    return polys


def corners_of(ring, grid=GRID):
    return [(int((grid.y_top - y) / grid.gsd), int((x - grid.x0) / grid.gsd)) for x, y in ring]


# ---- the vectoriser -----------------------------------------------------------------------------------------------------------
def test_a_rectangle_is_four_vertices_counter_clockwise_from_its_top_left_corner():
    label = np.zeros((48, 64), np.int32)
    label[3:7, 10:15] = 1
    (p,) = check_polygons(label)
    assert corners_of(p["rings"][0]) == [(3, 10), (7, 10), (7, 15), (3, 15)]          # down the left side first: the interior lies east
    assert p["rings"][0][0] == (1000.0 + 10 * 0.5, 5000.0 - 3 * 0.5)


def test_a_hole_is_clockwise_and_holes_are_ordered_by_their_corner():
    label = np.zeros((48, 64), np.int32)
    label[2:12, 2:20] = 1
    label[8:10, 4:6] = 0                                               # listed second: row 8
    label[4:6, 12:15] = 0                                              # listed first: row 4
    label[4:6, 4:6] = 2                                                # a second building inside a third hole (row 4, column 4)
    label[3:7, 3:7][label[3:7, 3:7] == 1] = 0
    p1, p2 = check_polygons(label)
    assert [corners_of(r)[0] for r in p1["rings"]] == [(2, 2), (3, 3), (4, 12), (8, 4)]
    assert corners_of(p1["rings"][2]) == [(4, 12), (4, 15), (6, 15), (6, 12)]          # along the top edge first: clockwise
    assert len(p2["rings"]) == 1 and corners_of(p2["rings"][0]) == [(4, 4), (6, 4), (6, 6), (4, 6)]


def test_a_hole_that_touches_the_exterior_at_a_corner_becomes_a_notch_of_the_exterior_ring():
    """Cells (1, 1) and (2, 2) are empty and touch at the corner (2, 2); four boundary edges of label 1 meet there.  The ring
    stays with its own cell at that corner, so the empty cell (1, 1) is not a hole ring: the exterior ring passes the corner
    twice and does not cross itself."""
    label = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 0]], np.int32)
    (p,) = check_polygons(label, dsm.Grid(0.0, 3.0, 1.0, 0.0, 3, 3))
    assert len(p["rings"]) == 1
    ring = corners_of(p["rings"][0], dsm.Grid(0.0, 3.0, 1.0, 0.0, 3, 3))
    assert ring == [(0, 0), (3, 0), (3, 2), (2, 2), (2, 1), (1, 1), (1, 2), (2, 2), (2, 3), (0, 3)]
    assert ring.count((2, 2)) == 2


def test_two_buildings_touching_at_a_corner_stay_two_simple_rings():
    label = np.zeros((6, 6), np.int32)
    label[1:3, 1:3] = 1
    label[3:5, 3:5] = 2
    g = dsm.Grid(0.0, 6.0, 1.0, 0.0, 6, 6)
    p1, p2 = check_polygons(label, g)
    assert corners_of(p1["rings"][0], g) == [(1, 1), (3, 1), (3, 3), (1, 3)] and corners_of(p2["rings"][0], g) == [(3, 3), (5, 3), (5, 5), (3, 5)]


def test_the_pinch_rule_on_one_label():
    """Two empty cells, (1, 1) and (2, 2), inside one label touch at the corner (2, 2), where the label's cells (1, 2) and (2, 1)
    touch too.  The ring turns so that those two cells are not joined through the corner: one hole ring, clockwise, that
    passes the corner twice (it touches itself and does not cross), not two holes."""
    label = np.ones((4, 4), np.int32)
    label[1, 1] = label[2, 2] = 0
    g = dsm.Grid(0.0, 4.0, 1.0, 0.0, 4, 4)
    (p,) = check_polygons(label, g)
    assert len(p["rings"]) == 2 and corners_of(p["rings"][0], g) == [(0, 0), (4, 0), (4, 4), (0, 4)]
    assert corners_of(p["rings"][1], g) == [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 2), (2, 2), (2, 1)]
    assert shoelace(p["rings"][1]) == -2.0


@pytest.mark.parametrize("name", ["random", "rings", "serpentine", "comb", "checkerboard"])
def test_outlines_on_the_component_scenes(name):
    mask = dict(random=np.random.default_rng(2).random((30, 41)) < 0.59, rings=rings_mask(29, 37), serpentine=serpentine_mask(21, 17),
                comb=comb_mask(15, 22), checkerboard=checkerboard_mask(9, 11))[name]
    label, N = components_ref(mask)
    polys = check_polygons(label, dsm.Grid(-8.0, 16.0, 0.25, 0.0, mask.shape[1], mask.shape[0]))
    assert len(polys) == N
    if name == "rings":
        assert [len(p["rings"]) for p in polys] == [2] * N


def test_polygons_refuse_a_label_that_is_not_one_component():
    label = np.zeros((5, 5), np.int32)
    label[0, 0] = label[4, 4] = 1
    with pytest.raises(ValueError, match="not one 4-connected component"):
        buildings.polygons(label, GRID)
    assert buildings.polygons(np.zeros((5, 5), np.int32), GRID) == []


def test_output_is_byte_identical_across_two_calls():
    d, nd = random_mask_raster(40, 50, 0.62, seed=8)
    ref = extract_ref(d, nd, 0.5, min_width=0.0, min_area=1.0, min_smooth=0.0)
    g = dsm.Grid(12.5, 99.0, 0.5, 0.0, 50, 40)
    texts = []
    for _ in range(2):
        polys = buildings.polygons(ref["label"].copy(), g)
        props = buildings.feature_properties(ref["table"], ref["keep"], g)
        texts.append(buildings.geojson_text(polys, props))
    assert texts[0] == texts[1] and texts[0].endswith("\n")
    gj = json.loads(texts[0])
    assert gj["type"] == "FeatureCollection" and len(gj["features"]) == ref["counts"]["buildings"] > 3
    for f in gj["features"]:
        assert f["geometry"]["type"] == "Polygon" and all(r[0] == r[-1] for r in f["geometry"]["coordinates"])
        assert set(f["properties"]) == {"id", "cells", "area_m2", "height_mean", "height_max", "smooth_fraction", "bbox"}
        assert f["properties"]["area_m2"] == f["properties"]["cells"] * 0.25


# ---- the simplifier -----------------------------------------------------------------------------------------------------------
def staircase(n):
    """A right triangle whose hypotenuse is n unit steps: (0, 0), down to (0, -n), right to (n, -n), then the steps back up to
    the start; 2 n + 2 vertices as (x, y), counter-clockwise."""
    ring = [(0.0, 0.0), (0.0, float(-n)), (float(n), float(-n))]
    for k in range(n, 0, -1):
        ring += [(float(k), float(-(k - 1))), (float(k - 1), float(-(k - 1)))]
    return ring[:-1]


def distance_to_ring(p, ring):
    return min(buildings._point_segment(p, a, b) for a, b in zip(ring, ring[1:] + ring[:1]))


@pytest.mark.parametrize("tol", [0.0, 0.3, 0.75, 2.0, 100.0])
def test_simplifier_guarantees_on_a_staircase(tol):
    ring = staircase(8)
    assert len(ring) == len(set(ring)) == 18 and shoelace(ring) > 0
    out = buildings.simplify_ring(ring, tol)
    assert out[0] == ring[0]                                            # the start vertex stays
    it = iter(ring)
    assert all(p in it for p in out)                                    # a subset, in order
    assert len(set(out)) >= 3
    assert all(distance_to_ring(p, out) <= tol for p in ring)           # every dropped vertex within tol of the result
    if tol == 0.0:
        assert out == ring                                              # the identity
    if tol == 0.3:
        assert out == ring                                              # every step is 0.707 from its chord
    if tol == 0.75:
        assert len(out) == 3                                            # the steps go, the triangle stays
    if tol >= 2.0:
        assert len(out) == 3                                            # the floor of three distinct vertices


def test_simplifier_on_short_rings_and_through_polygons():
    tri = [(0.0, 0.0), (4.0, 0.0), (0.0, 3.0)]
    assert buildings.simplify_ring(tri, 50.0) == tri
    square = [(0.0, 0.0), (0.0, -1.0), (1.0, -1.0), (1.0, 0.0)]
    out = buildings.simplify_ring(square, 50.0)
    assert len(out) == 3 and out[0] == square[0] and set(out) <= set(square)
    label = np.zeros((48, 64), np.int32)
    for k in range(10):
        label[10 + k, 5:6 + k] = 1
    exact = buildings.polygons(label, GRID)[0]["rings"][0]
    assert buildings.polygons(label, GRID, simplify_tol=0.0)[0]["rings"][0] == exact and len(exact) == 22
    simple = buildings.polygons(label, GRID, simplify_tol=0.4)[0]["rings"][0]
    assert simple[0] == exact[0] and 3 <= len(simple) < len(exact) and set(simple) <= set(exact)
    assert all(distance_to_ring(p, simple) <= 0.4 for p in exact)


# ---- the selection ------------------------------------------------------------------------------------------------------------
def test_selection_rule_on_a_hand_made_table():
    #                 big+flat  small  rough  exactly at both limits  no flagged cell  just below the area  just below the fraction
    cells = np.array([100,      39,    100,   40,                     50,              39,                  40])
    smooth = np.array([80,      39,    10,    20,                     0,               30,                  19])
    rough = np.array([10,       0,     90,    20,                     0,               0,                   20])
    table = dict(cells=cells, smooth=smooth, rough=rough)
    keep, counts = buildings.select(table, 0.5, min_area=10.0, min_smooth=0.5)       # 40 cells of 0.25 m^2 are 10 m^2
    assert keep.tolist() == [True, False, False, True, False, False, False]
    assert counts == dict(components=7, buildings=2, rejected_small=2, rejected_rough=3)
    keep0, counts0 = buildings.select(table, 0.5, min_area=10.0, min_smooth=0.0)     # smooth + rough == 0 passes only now
    assert keep0.tolist() == [True, False, True, True, True, False, True] and counts0["rejected_rough"] == 0
    for args in ((10.0, 0.5), (10.0, 0.0), (0.0, 1.0), (12.5, 0.25)):
        a, b = buildings.select(table, 0.5, *args), select_ref(table, 0.5, *args)
        assert a[0].tolist() == b[0].tolist() and a[1] == b[1]
    assert buildings.relabel(np.array([[0, 1, 2], [3, 4, 7]]), keep).tolist() == [[0, 1, 0], [0, 2, 0]]
    keep, counts = buildings.select(dict(cells=np.zeros(0, np.int64), smooth=np.zeros(0, np.int64), rough=np.zeros(0, np.int64)), 0.5)
    assert keep.size == 0 and counts == dict(components=0, buildings=0, rejected_small=0, rejected_rough=0)


def test_feature_properties():
    table = {n: np.zeros(2, np.int64) for n in COLUMNS}
    table.update(cells=np.array([8, 5]), smooth=np.array([3, 0]), rough=np.array([1, 0]), row_min=np.array([2, 0]), row_max=np.array([3, 0]),
                 col_min=np.array([4, 0]), col_max=np.array([7, 4]), height_sum=np.array([8 * 6 * 1024 + 512, 5 * 3 * 1024]),
                 height_max_bits=np.array([0x40E00000, 0x40400000]))
    a, b = buildings.feature_properties(table, np.array([True, True]), GRID)
    assert a == dict(id=1, cells=8, area_m2=2.0, height_mean=6.0625, height_max=7.0, smooth_fraction=0.75,
                     bbox=[1002.0, 5000.0 - 2.0, 1004.0, 5000.0 - 1.0])
    assert b["smooth_fraction"] is None and b["height_mean"] == 3.0 and b["height_max"] == 3.0
    (only,) = buildings.feature_properties(table, np.array([False, True]), GRID)
    assert only["id"] == 1 and only["cells"] == 5


# ---- the restatement against hand-computed cases --------------------------------------------------------------------------------
def test_restatement_mask_and_opening_by_hand():
    nd = np.zeros((7, 9), np.float32)
    nd[1:6, 1:6] = 3.0                                                 # 5 x 5: survives r = 2
    nd[1:4, 7] = 3.0                                                   # 1 wide: removed by r = 1
    nd[0, 0], nd[6, 8], nd[6, 0] = np.nan, np.inf, 2.5
    m0, m = mask_ref(nd, 2.5, 0)
    assert m0.sum() == 25 + 3 + 1 and np.array_equal(m, m0) and m0[6, 0] and not m0[0, 0] and not m0[6, 8]
    for r in (1, 2):
        m0, m = mask_ref(nd, 2.5, r)
        assert m.sum() == 25 and m[1:6, 1:6].all()
        assert np.array_equal(m, mask_ref(nd, 2.5, r, opening=open_brute)[1])
    assert mask_ref(nd, 2.5, 3)[1].sum() == 0
    assert mask_ref(nd, np.nextafter(np.float32(2.5), np.float32(3)), 0)[0].sum() == 28


def test_restatement_flags_by_hand():
    """A 3 x 5 slab, s = 1, tol 0.25.  Row 1 is 0, 1, 2, 3.5, 5: the second differences along it are 0, 0.5, 0."""
    nd = np.full((3, 5), 4.0, np.float32)
    d = np.zeros((3, 5), np.float32)
    d[:] = np.array([0.0, 1.0, 2.0, 3.5, 5.0], np.float32)
    f = flags_ref(d, nd, 2.5, 0, 1, 0.25)
    # the corners have no direction; rows 0 and 2 only the horizontal one; the middle row all of them (columns are constant)
    assert f.tolist() == [[2, 3, 4, 3, 2], [3, 3, 4, 3, 3], [2, 3, 4, 3, 2]]
    d[1, 2] = np.nan                                                   # a direction through an empty neighbour does not count
    f = flags_ref(d, nd, 2.5, 0, 1, 0.25)
    assert f[1, 1] == 3 and f[1, 3] == 3 and f[0, 2] == 4 and f[1, 2] == 4    # (1, 1): only the vertical counts; (1, 2): D is NaN
    assert flags_ref(d, nd, 2.5, 0, 2, 0.25).tolist() == [[2, 2, 4, 2, 2]] * 3  # s = 2: the horizontal of column 2 alone: 0 + 5 - 4
    nd[0, 0] = 1.0
    nd[2, 4] = np.nan
    f = flags_ref(d, nd, 2.5, 0, 1, 0.25)
    assert f[0, 0] == 0 and f[2, 4] == 0 and f[1, 1] == 3 and f[0, 1] == 2   # (0, 1) lost its horizontal neighbour


def test_restatement_components_and_table_by_hand():
    m = np.array([[1, 1, 0, 1], [0, 1, 0, 0], [1, 0, 1, 1], [1, 0, 0, 1]], bool)
    label, N = components_ref(m)
    assert N == 4 and label.tolist() == [[1, 1, 0, 2], [0, 1, 0, 0], [3, 0, 4, 4], [3, 0, 0, 4]]     # corners do not join
    flags = np.where(m, 3, 0).astype(np.uint8)
    flags[0, 0], flags[2, 2] = 4, 2
    nd = np.where(m, 2.5, 0.0).astype(np.float32)
    nd[2, 3], nd[3, 3] = 70000.0, 3.0 + 2.0 ** -11                     # capped at 65535; 3072.5 rounds to the even 3072
    t = table_ref(label, N, flags, nd)
    assert t["cells"].tolist() == [3, 1, 2, 3] and t["smooth"].tolist() == [2, 1, 2, 2] and t["rough"].tolist() == [1, 0, 0, 0]
    assert t["undetermined"].tolist() == [0, 0, 0, 1]
    assert (t["row_min"].tolist(), t["row_max"].tolist(), t["col_min"].tolist(), t["col_max"].tolist()) == ([0, 0, 2, 2], [1, 0, 3, 3], [0, 3, 0, 2], [1, 3, 0, 3])
    assert t["height_sum"].tolist() == [3 * 2560, 2560, 2 * 2560, 2560 + 65535 * 1024 + 3072]
    assert t["height_max_bits"].tolist()[:3] == [0x40200000] * 3 and t["height_max_bits"][3] == int(np.array([70000.0], np.float32).view(np.uint32)[0])
    for mask in (serpentine_mask(9, 7), comb_mask(6, 9)):
        assert components_ref(mask)[1] == 1 and mask.sum() > mask.size // 2
    assert components_ref(checkerboard_mask(5, 6))[1] == 15 and components_ref(rings_mask(21, 21))[1] == 3
    assert cell_parameters(0.5) == (2, 2) and cell_parameters(0.4, 0.8, 0.8) == (1, 2) and cell_parameters(3.0, 2.0, 1.0) == (0, 1)
    assert cell_parameters(0.4, 2.0, 1.0) == (2, 2) and cell_parameters(1.0, 2.0, 2.5) == (1, 2)          # 2.5 rounds to the even 2


def test_roof_scene_on_the_restatement():
    """What the GPU test expects of the scene holds for the restatement: the boxes and gabled roofs come out whole, every
    crown is rejected as rough, every small box as small, the narrow strips are opened away."""
    d, nd, truth = roof_scene()
    assert (np.abs(d * 8) % 1 == 0).all() and (np.abs(nd * 8) % 1 == 0).all()
    ref = extract_ref(d, nd, 0.5)
    assert (ref["r_open"], ref["stride"]) == (2, 2)
    t, keep = ref["table"], ref["keep"]
    found = [(int(t["cells"][k]), t["height_sum"][k] / 1024.0 / t["cells"][k], float(np.array([t["height_max_bits"][k]], np.uint32).view(np.float32)[0]))
             for k in np.flatnonzero(keep)]
    assert found == truth["buildings"] and len(found) == 5
    assert ref["counts"]["rejected_rough"] == 3 and ref["counts"]["rejected_small"] == 3 and ref["counts"]["components"] == 11
    assert not ref["label"][truth["crowns"]].any() and not ref["label"][truth["small"]].any()
    assert (ref["flags"][truth["narrow"]] == 1).all() and ref["counts"]["opened_away"] >= truth["narrow"].sum()
    small = np.unique(ref["components"][truth["small"]])
    assert len(small) == 3 and all(t["cells"][k - 1] * 0.25 < 10.0 for k in small)


# ---- parameters, files, ABI, CLI ------------------------------------------------------------------------------------------------
def test_parameters_and_their_errors():
    p = buildings.parameters(0.5)
    assert p == dict(min_height=2.5, min_width=2.0, smooth_span=1.0, smooth_tol=0.2, min_smooth=0.5, min_area=10.0, r_open=2, stride=2)
    assert buildings.DEFAULTS == dict(min_height=2.5, min_width=2.0, smooth_span=1.0, smooth_tol=0.2, min_smooth=0.5, min_area=10.0)
    p = buildings.parameters(3.0, min_width=0.0, smooth_tol=0.0, min_smooth=0.0, min_area=0.0)
    assert (p["r_open"], p["stride"]) == (0, 1)
    assert buildings.parameters(0.01, min_width=20.48, smooth_span=0.64)["r_open"] == 1024
    bad = [dict(gsd=0.0), dict(gsd=float("nan")), dict(min_height=0.0), dict(min_height=-1.0), dict(min_height=float("inf")), dict(min_width=-1.0),
           dict(min_width=float("nan")), dict(smooth_span=0.0), dict(smooth_span=float("inf")), dict(smooth_tol=-0.1), dict(smooth_tol=float("nan")),
           dict(min_smooth=-0.1), dict(min_smooth=1.5), dict(min_area=-1.0), dict(min_area=float("inf")),
           dict(gsd=0.01, min_width=20.6), dict(gsd=0.01, smooth_span=0.66)]                   # 1030 cells; 66 cells
    for kw in bad:
        args = dict(gsd=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            buildings.parameters(**args)
    z = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError):
        buildings.extract(z, z, 0.5, simplify_tol=-1.0)
    with pytest.raises(ValueError):
        buildings.extract(z, z[:3], 0.5)
    with pytest.raises(ValueError):
        buildings.extract(z, z, 0.5, min_height=0.0)


def test_extract_raises_without_a_gpu(monkeypatch, tmp_path):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    z = np.zeros((4, 4), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        buildings.extract(z, z, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        buildings.from_dsm(str(tmp_path / "dsm"))


def test_parser_defaults_and_help():
    a = buildings.build_parser().parse_args(["--dsm", "/x/dsm"])
    assert (a.dsm, a.filled, a.min_height, a.min_width, a.smooth_span, a.smooth_tol, a.min_smooth, a.min_area, a.simplify_tol, a.out) == \
        ("/x/dsm", False, 2.5, 2.0, 1.0, 0.2, 0.5, 10.0, 0.0, None)
    a = buildings.build_parser().parse_args(["--dsm", "p", "--filled", "--min_area", "25", "--simplify_tol", "0.5", "--out", "q"])
    assert (a.filled, a.min_area, a.simplify_tol, a.out) == (True, 25.0, 0.5, "q")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "buildings_whu.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "--min_height" in r.stdout and "--simplify_tol" in r.stdout
    assert "not values measured on WHU scenes" in " ".join(buildings.__doc__.split())


def test_output_paths_are_disjoint_from_every_earlier_stage():
    mine = set(buildings.output_paths("/o/p").values())
    assert mine == {"/o/p_buildings.geojson", "/o/p_buildings.tif", "/o/p_buildings.tfw", "/o/p_buildings.json"}
    assert len(mine) == len(buildings.output_paths("/o/p"))
    for other in (dsm.output_paths("/o/p"), dsm.fill_output_paths("/o/p"), dtm.output_paths("/o/p")):
        assert not mine & set(other.values())


def test_files_round_trip(tmp_path):
    d, nd = random_mask_raster(30, 36, 0.62, seed=3)
    ref = extract_ref(d, nd, 0.5, min_width=0.0, min_area=1.0, min_smooth=0.0)
    g = dsm.Grid(5e5 + 0.25, 3.4e6 - 0.75, 0.5, 12.0, 36, 30)
    res = dict(label=ref["label"], polygons=buildings.polygons(ref["label"], g), properties=buildings.feature_properties(ref["table"], ref["keep"], g),
               grid=g, params=buildings.parameters(0.5, min_width=0.0, min_area=1.0, min_smooth=0.0), counts=ref["counts"],
               label_stats=dict(rounds=0, tiles=1, pairs=0), seconds=dict(flags=0.0), source=dict(prefix="x", filled=False))
    out = str(tmp_path / "sub" / "scene")
    paths = buildings.write_outputs(out, res)
    assert paths == buildings.output_paths(out) and all(os.path.exists(p) for p in paths.values())
    label, gj, js = buildings.read_outputs(out)
    assert label.dtype == np.int32 and np.array_equal(label, ref["label"])
    assert open(paths["geojson"]).read() == buildings.geojson_text(res["polygons"], res["properties"])
    assert len(gj["features"]) == ref["counts"]["buildings"] == label.max()
    for f, poly, prop in zip(gj["features"], res["polygons"], res["properties"]):
        assert f["properties"] == prop
        assert f["geometry"]["coordinates"] == [[list(p) for p in ring + ring[:1]] for ring in poly["rings"]]
    assert js["grid"] == dict(x0=g.x0, y_top=g.y_top, gsd=0.5, W=36, H=30) and js["counts"] == ref["counts"] and js["params"] == res["params"]
    assert open(paths["label_world"]).read() == dsm.world_file_text(g)


def test_abi_and_the_new_signatures():
    assert _lib.ABI_VERSION == 22                                      # grown by four entry points; nothing existing changed
    for name in ("adamvs_bld_workspace_bytes", "adamvs_bld_flags", "adamvs_bld_label", "adamvs_bld_table"):
        assert name in _lib.SIGNATURES
    assert (_lib.BLD_TILE_W, _lib.BLD_TILE_H, _lib.BLD_MAX_STRIDE, _lib.BLD_MAX_ROUNDS, _lib.BLD_NOT_CONVERGED) == (64, 64, 64, 64, -2)
    assert _lib.BLD_COLUMNS == buildings.COLUMNS == COLUMNS and buildings.MAX_STRIDE == _lib.BLD_MAX_STRIDE
    assert buildings.MAX_RADIUS == _lib.DTM_MAX_RADIUS
    assert ctypes.sizeof(_lib.BldStats) == 2 * 4 + 2 * 8 + 3 * 4 + 4     # three floats, padded to the long's alignment
    header = open(os.path.join(ROOT, "include", "adamvs_hip.h")).read()
    for k, v in (("TILE_W", 64), ("TILE_H", 64), ("MAX_STRIDE", 64), ("MAX_ROUNDS", 64), ("COLUMNS", 10)):
        assert "#define ADAMVS_BLD_%s %d" % (k, v) in header
    assert "Building extraction" in header
    lib = _lib.load()
    assert lib.adamvs_bld_workspace_bytes(0, 5) < 0 and lib.adamvs_bld_workspace_bytes(1 << 15, 1 << 14) < 0
    assert lib.adamvs_bld_workspace_bytes(7, 5) == 256 + 2 * 256 + lib.adamvs_dtm_workspace_bytes(7, 5)
    st = _lib.BldStats()
    assert lib.adamvs_bld_flags(4, 4, None, None, 2.5, 1, 1, 0.2, None, 0, None, None) < 0              # before any launch
    assert lib.adamvs_bld_label(4, 4, None, None, 0, None, ctypes.byref(st), None) < 0
    assert lib.adamvs_bld_table(4, 4, None, None, None, 1, None, None) < 0
    assert math.isfinite(buildings.DEFAULTS["min_height"])
