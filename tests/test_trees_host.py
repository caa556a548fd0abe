"""Tree detection, host side: the window table and the parameter checks of ada_mvs_amd/trees.py, the numpy restatement
(tests/trees_ref.py) on the crown scene, a plateau and the roof scene, the selection, the crown outlines, the GeoJSON text, the
file names, the ABI and the CLI."""
import ctypes
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, buildings, dsm, dtm, roofs, trees
from buildings_ref import extract_ref, roof_scene
from conftest import ROOT
from trees_ref import (COLUMNS, CROWN_GSD, crown_scene, crowns_ref, detect_ref, jump_rounds_ref, parents_ref, plateau, roots_ref,
                       serpentine_ramp, stage_ref, surface_ref)

GRID = dsm.Grid(1000.0, 5000.0, 0.5, 0.0, 64, 48)                      # gsd a power of two: every coordinate and area is exact


# ---- parameters and the window table ------------------------------------------------------------------------------------------
def brute_radius(s, gsd, radius_min, radius_slope, passes):
    metres = Fraction(radius_min) + Fraction(radius_slope) * Fraction(s, 256 * 16 ** passes)
    return max(1, math.floor(metres / Fraction(gsd)))


@pytest.mark.parametrize("gsd,radius_min,radius_slope,passes,s_max", [
    (0.5, 1.5, 0.05, 0, 30 * 256), (0.5, 1.5, 0.05, 1, 3000), (0.3, 0.7, 0.11, 0, 5000), (0.25, 0.0, 0.4, 0, 2500), (0.5, 1.5, 0.0, 0, 4000),
    (1.0, 0.2, 0.01, 0, 6000), (0.1, 1.5, 0.05, 2, 70000)])
def test_window_table_against_brute_force_for_every_s(gsd, radius_min, radius_slope, passes, s_max):
    thr = trees.window_table(gsd, radius_min, radius_slope, passes, s_max)
    assert thr[0] == 0 and thr == sorted(thr) and len(thr) == brute_radius(s_max, gsd, radius_min, radius_slope, passes)
    step = 1 if s_max <= 8000 else 7
    ss = np.arange(0, s_max + 1, step)
    want = [brute_radius(int(s), gsd, radius_min, radius_slope, passes) for s in ss]
    assert trees.window_cells(ss, thr).tolist() == want
    for r, t in enumerate(thr, start=1):                                # the threshold at which r changes: r at thr[r], below r just before it
        assert brute_radius(t, gsd, radius_min, radius_slope, passes) >= r
        assert t == 0 or brute_radius(t - 1, gsd, radius_min, radius_slope, passes) < r


def test_window_table_of_the_defaults_at_gsd_half_a_metre():
    """radius = 1.5 m + 0.05 x height: 3 cells up to 10 m, 4 cells from 10 m, 5 from 20 m; 10 m is 2560 in 1/256 m."""
    assert trees.window_table(0.5, 1.5, 0.05, 0, 25 * 256) == [0, 0, 0, 10 * 256, 20 * 256]
    assert trees.window_table(0.5, 1.5, 0.05, 1, 25 * 256 * 16) == [0, 0, 0, 10 * 256 * 16, 20 * 256 * 16]
    assert trees.window_table(0.5, 1.5, 0.05, 0, -1) == [0, 0, 0] and trees.window_table(2.0, 1.5, 0.05, 0, -1) == [0]
    assert trees.window_cells([0, 2559, 2560, 5119, 5120], [0, 0, 0, 2560, 5120]).tolist() == [3, 3, 4, 4, 5]


def test_parameters_and_their_errors():
    p = trees.parameters(0.5)
    assert p == dict(min_height=2.0, smooth_passes=1, radius_min=1.5, radius_slope=0.05, crown_ratio=0.55, max_crown_radius=10.0,
                     min_crown_area=1.0, ratio_pm=550, rc2=400)
    assert trees.parameters(0.5, s_max=12 * 256 * 16)["r_cap"] == 4 and trees.parameters(0.5, s_max=-1)["r_cap"] == 3
    assert trees.parameters(0.3, max_crown_radius=1.0)["rc2"] == 11                         # (1 / 0.3)^2 = 11.1
    assert trees.parameters(0.5, crown_ratio=0.0625)["ratio_pm"] == 62                      # 62.5 rounds half to even
    assert trees.parameters(0.5, crown_ratio=0.1875)["ratio_pm"] == 188                     # 187.5 too
    assert trees.parameters(0.5, crown_ratio=1.0, max_crown_radius=0.0, min_crown_area=0.0, radius_min=0.0, radius_slope=0.0)["rc2"] == 0
    for kw in (dict(min_height=0.0), dict(min_height=-1.0), dict(min_height=float("nan")), dict(radius_min=-0.1), dict(radius_slope=-1.0),
               dict(radius_slope=float("inf")), dict(crown_ratio=1.5), dict(crown_ratio=-0.1), dict(max_crown_radius=-1.0),
               dict(min_crown_area=float("nan")), dict(smooth_passes=3), dict(smooth_passes=-1), dict(smooth_passes=1.5), dict(smooth_passes=True)):
        with pytest.raises(ValueError):
            trees.parameters(0.5, **kw)
    with pytest.raises(ValueError):
        trees.parameters(0.0)
    # 1.5 m + 0.05 x 60 m = 4.5 m at 6.25 cm: 72 cells; at 50 m it is 4 m: 64 cells
    with pytest.raises(ValueError, match=r"window of 72 cells radius: at most 64"):
        trees.parameters(0.0625, s_max=60 * 256 * 16)
    assert trees.parameters(0.0625, s_max=50 * 256 * 16)["r_cap"] == 64
    z = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError):
        trees.detect(z[0], 0.5)
    with pytest.raises(ValueError):
        trees.detect(z, 0.5, building=np.zeros((3, 4), np.int32))
    with pytest.raises(ValueError):
        trees.detect(z, 0.5, min_height=0.0)


# ---- the restatement by hand ----------------------------------------------------------------------------------------------------
def test_restatement_surface_by_hand():
    nd = np.array([[2.0, 4.0, np.nan], [1.99, 3.0, 2047.5], [np.inf, 2.0, 8.0]], np.float32)
    bld = np.zeros((3, 3), np.int32)
    bld[2, 2] = 7
    mask, q, s, s_max = surface_ref(nd, bld, 2.0, 0)
    assert mask.tolist() == [[1, 1, 0], [0, 1, 1], [0, 1, 0]]
    assert q.tolist() == [[512, 1024, 0], [0, 768, 2047 * 256], [0, 512, 0]] and s_max == 2047 * 256
    assert s.tolist() == [[512, 1024, -1], [-1, 768, 2047 * 256], [-1, 512, -1]]
    assert surface_ref(nd, None, 2.0, 0)[0][2, 2] == 1 and surface_ref(np.zeros_like(nd), None, 2.0, 1)[3] == -1
    # one pass at the corner (0, 0): neighbours (0, 1) and (1, 1) count, the other six positions give the centre's 512
    _, _, s1, _ = surface_ref(nd, bld, 2.0, 1)
    assert s1[0, 0] == 2 * 1024 + 1 * 768 + (16 - 3) * 512 and s1[0, 2] == -1
    # a constant canopy stays constant, scaled by 16 per pass
    for passes in (0, 1, 2):
        assert (surface_ref(plateau(5, 6), None, 2.0, passes)[2] == 5 * 256 * 16 ** passes).all()


def test_restatement_parents_tops_and_roots_by_hand():
    """One row: heights 3 5 4 . 6 2 at r = 1.  5 and 6 are tops; with r = 3 the 5 sees the 6 across the gap and hangs on it."""
    nd = np.array([[3.0, 5.0, 4.0, 0.0, 6.0, 2.0]], np.float32)
    _, _, s, _ = surface_ref(nd, None, 2.0, 0)
    parent, top, radius = parents_ref(s, [0])
    assert parent.tolist() == [[1, 1, 1, -1, 4, 4]] and top.tolist() == [[False, True, False, False, True, False]]
    assert radius.tolist() == [[1, 1, 1, 0, 1, 1]] and roots_ref(parent).tolist() == [[1, 1, 1, -1, 4, 4]]
    parent, top, _ = parents_ref(s, [0, 0, 0])
    assert parent.tolist() == [[1, 4, 1, -1, 4, 4]] and top.sum() == 1 and roots_ref(parent).tolist() == [[4, 4, 4, -1, 4, 4]]
    assert jump_rounds_ref(parent) == 1
    label, T, unassigned = crowns_ref(s, roots_ref(parent), 550, 9)
    # 0.55 x 6 = 3.3: the 3 m and the 2 m cell fail the ratio; cell 0 also lies 4 cells from the top
    assert label.tolist() == [[0, 1, 1, 0, 1, 0]] and T == 1 and unassigned == 2
    assert crowns_ref(s, roots_ref(parent), 0, 9)[0].tolist() == [[0, 1, 1, 0, 1, 1]]       # the radius test alone: 4^2 > 9
    assert crowns_ref(s, roots_ref(parent), 500, 16)[0].tolist() == [[1, 1, 1, 0, 1, 0]]     # both inclusive: 3 = 0.5 x 6, 4^2 = 16


def test_restatement_on_a_plateau_has_one_top():
    for passes in (0, 1):
        r = stage_ref(plateau(9, 13), None, 2.0, passes, [0, 0, 0, 0], 550, 10 ** 6)
        assert r["T"] == 1 and np.flatnonzero(r["top"]).tolist() == [0] and (r["root"] == 0).all() and (r["crowns"] == 1).all()
        assert {n: int(r["table"][n][0]) for n in COLUMNS} == dict(cells=117, q_sum=117 * 1280, q_max=1280, row_min=0, row_max=8, col_min=0,
                                                                    col_max=12, r2_max=64 + 144, top=0, s_top=1280 * 16 ** passes)


def test_restatement_on_the_serpentine_ramp_is_one_chain():
    nd = serpentine_ramp(9, 7)
    r = stage_ref(nd, None, 2.0, 0, [0], 0, 10 ** 6)
    end = int(np.argmax(nd))
    assert r["T"] == 1 and (r["root"][nd > 0] == end).all() and int(r["table"]["cells"][0]) == int((nd > 0).sum()) == 5 * 7 + 4
    # a chain of the order of the path (39 cells, a few skipped at the turns): 5 rounds of two hops, 2 rounds of eight
    assert jump_rounds_ref(r["parent"], hops=2) == 5 and jump_rounds_ref(r["parent"]) == 2


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crown_result():
    nd, building, truth = crown_scene()
    return nd, building, truth, detect_ref(nd, CROWN_GSD, building)


def test_crown_scene_tops_are_the_planted_cells(crown_result):
    nd, building, truth, res = crown_result
    assert np.flatnonzero(res["top"]).tolist() == truth["tops"] and res["T"] == len(truth["tops"]) == res["counts"]["trees"]
    assert res["table"]["top"].tolist() == truth["tops"] and res["keep"].all()
    assert [p["height_m"] for p in res["properties"]] == truth["heights"]
    assert [p["id"] for p in res["properties"]] == list(range(1, len(truth["tops"]) + 1))
    W = nd.shape[1]
    for p, t in zip(res["properties"], truth["tops"]):
        assert (p["x"], p["y"]) == ((t % W + 0.5) * 0.5, nd.shape[0] * 0.5 - (t // W + 0.5) * 0.5)


def test_crown_scene_crowns_lie_in_their_discs_and_off_the_buildings(crown_result):
    nd, building, truth, res = crown_result
    assert not res["label"][building > 0].any() and not res["mask"][building > 0].any()
    for k, disc in enumerate(truth["discs"], start=1):
        crown = res["label"] == k
        assert crown.any() and not (crown & ~disc).any()
        assert crown.sum() == res["properties"][k - 1]["cells"] and res["properties"][k - 1]["parts"] == 1
    # the paraboloids fall to 0.4 of their top at the rim: the ratio 0.55 leaves the rim unassigned
    assert res["counts"]["unassigned"] > 0 and res["counts"]["labelled"] + res["counts"]["unassigned"] == res["counts"]["canopy"]
    # without the labels the boxes are canopy and grow tops of their own
    free = detect_ref(nd, CROWN_GSD, None)
    assert free["label"][building > 0].any() and free["T"] > res["T"]


def test_roof_scene_trees_stand_off_the_buildings_and_in_every_crown():
    d, nd, truth = roof_scene()
    building = extract_ref(d, nd, 0.5)["label"]
    res = detect_ref(nd, 0.5, building)
    assert not res["label"][building > 0].any()
    i, j = np.mgrid[0:nd.shape[0], 0:nd.shape[1]]
    from buildings_ref import ROOF_CROWNS
    tops = np.flatnonzero(res["keep"])
    top_cells = res["table"]["top"][tops]
    for ci, cj, rad in ROOF_CROWNS:                                     # every crown of the scene is 6 .. 10 m: it survives min_height = 2 m
        inside = ((top_cells // nd.shape[1] - ci) ** 2 + (top_cells % nd.shape[1] - cj) ** 2) <= rad * rad
        assert inside.sum() >= 1
    assert res["counts"]["trees"] >= len(ROOF_CROWNS)


# ---- selection, outlines, text --------------------------------------------------------------------------------------------------
def test_selection_rule_on_a_hand_made_table():
    table = {n: np.zeros(4, np.int64) for n in COLUMNS}
    table["cells"] = np.array([4, 3, 40, 1])
    keep, counts = trees.select(table, 0.5, 1.0)                        # 4 cells of 0.25 m^2 are exactly 1 m^2
    assert keep.tolist() == [True, False, True, False] and counts == dict(tops=4, trees=2, rejected_small=2)
    assert trees.select(table, 0.5, 0.0)[0].all()


def test_crown_polygons_two_parts_a_hole_and_a_corner_touch():
    label = np.zeros((48, 64), np.int32)
    label[2:7, 2:7] = 1
    label[4, 4] = 0                                                    # a hole in the first part
    label[10:12, 20:23] = 1                                            # a second part far away
    label[7, 7] = 1                                                    # a third that touches the first at the corner (7, 7)
    label[20:22, 5:8] = 2
    polys = trees.crown_polygons(label, GRID)
    assert [p["id"] for p in polys] == [1, 2] and [len(p["polygons"]) for p in polys] == [3, 1]
    first, corner, second = polys[0]["polygons"]                        # ordered by the exterior ring's first vertex
    xy = lambda r, c: (1000.0 + c * 0.5, 5000.0 - r * 0.5)
    assert first[0] == [xy(2, 2), xy(7, 2), xy(7, 7), xy(2, 7)] and len(first) == 2
    assert first[1] == [xy(4, 4), xy(4, 5), xy(5, 5), xy(5, 4)]         # the hole, clockwise
    assert corner == [[xy(7, 7), xy(8, 7), xy(8, 8), xy(7, 8)]]
    assert second == [[xy(10, 20), xy(12, 20), xy(12, 23), xy(10, 23)]]
    assert polys[1]["polygons"] == [[[xy(20, 5), xy(22, 5), xy(22, 8), xy(20, 8)]]]
    with pytest.raises(ValueError, match="not one 4-connected component"):
        buildings.polygons(label, GRID)                                 # the building stage's vectoriser is untouched


def test_crown_polygons_nested_parts_keep_their_own_holes():
    """A ring-shaped part with a second part in its hole, which has a hole itself: each hole goes to the innermost exterior."""
    label = np.zeros((48, 64), np.int32)
    label[1:12, 1:12] = 1
    label[2:11, 2:11] = 0
    label[4:9, 4:9] = 1
    label[6, 6] = 0
    (poly,) = trees.crown_polygons(label, GRID)
    outer, inner = poly["polygons"]
    assert len(outer) == 2 and len(inner) == 2
    assert outer[1][0] == (1000.0 + 2 * 0.5, 5000.0 - 2 * 0.5) and inner[1][0] == (1000.0 + 6 * 0.5, 5000.0 - 6 * 0.5)


def test_geojson_text_is_stable(crown_result):
    nd, building, truth, res = crown_result
    again = detect_ref(nd, CROWN_GSD, building)
    pts, crowns = trees.points_geojson_text(res["properties"]), trees.crowns_geojson_text(res["polygons"], res["properties"])
    assert pts == trees.points_geojson_text(again["properties"]) and crowns == trees.crowns_geojson_text(again["polygons"], again["properties"])
    a, b = json.loads(pts), json.loads(crowns)
    assert len(a["features"]) == len(b["features"]) == res["counts"]["trees"]
    keys = ["id", "x", "y", "height_m", "height_mean_m", "crown_area_m2", "crown_diameter_m", "crown_radius_max_m", "volume_m3", "cells", "parts",
            "window_cells"]
    for fa, fb, prop in zip(a["features"], b["features"], res["properties"]):
        assert list(fa["properties"]) == keys and fa["properties"] == fb["properties"] == prop
        assert fa["geometry"] == dict(type="Point", coordinates=[prop["x"], prop["y"]]) and fb["geometry"]["type"] == "MultiPolygon"
        assert all(ring[0] == ring[-1] for part in fb["geometry"]["coordinates"] for ring in part)
    p = res["properties"][0]                                            # the 12 m tree: window 1.5 + 0.6 = 2.1 m = 4 cells
    assert p["window_cells"] == 4 and p["crown_area_m2"] == p["cells"] * 0.25 and p["volume_m3"] == p["height_mean_m"] * p["crown_area_m2"]
    assert p["crown_diameter_m"] == 2.0 * math.sqrt(p["crown_area_m2"] / math.pi) and p["crown_radius_max_m"] <= 14 * 0.5


def test_files_round_trip(tmp_path, crown_result):
    nd, building, truth, ref = crown_result
    g = dsm.Grid(5e5 + 0.25, 3.4e6 - 0.75, 0.5, 12.0, nd.shape[1], nd.shape[0])
    res = detect_ref(nd, CROWN_GSD, building, grid=g)
    res.update(stats=dict(rounds=res["jump_rounds"], tops=res["T"], candidates=0, window_cells=0), seconds=dict(surface=0.0),
               source=dict(prefix="x", buildings=True))
    out = str(tmp_path / "sub" / "scene")
    paths = trees.write_outputs(out, res)
    assert paths == trees.output_paths(out) and all(os.path.exists(p) for p in paths.values())
    label, pts, crowns, js = trees.read_outputs(out)
    assert label.dtype == np.int32 and np.array_equal(label, res["label"])
    assert open(paths["points"]).read() == trees.points_geojson_text(res["properties"])
    assert open(paths["crowns"]).read() == trees.crowns_geojson_text(res["polygons"], res["properties"])
    assert len(pts["features"]) == len(crowns["features"]) == res["counts"]["trees"] == label.max()
    assert js["grid"] == dict(x0=g.x0, y_top=g.y_top, gsd=0.5, W=g.W, H=g.H) and js["counts"] == res["counts"]
    assert js["params"] == dict(res["params"], thr=res["thr"]) and js["jump_rounds"] == res["jump_rounds"] and "seconds" in js
    assert open(paths["label_world"]).read() == dsm.world_file_text(g)


def test_output_paths_are_disjoint_from_every_earlier_stage():
    mine = set(trees.output_paths("/o/p").values())
    assert mine == {"/o/p_trees.geojson", "/o/p_crowns.geojson", "/o/p_trees.tif", "/o/p_trees.tfw", "/o/p_trees.json"}
    assert len(mine) == len(trees.output_paths("/o/p"))
    for other in (dsm.output_paths("/o/p"), dsm.fill_output_paths("/o/p"), dtm.output_paths("/o/p"), buildings.output_paths("/o/p"),
                  roofs.output_paths("/o/p")):
        assert not mine & set(other.values())


# ---- the stage without a GPU, the CLI, the ABI ------------------------------------------------------------------------------------
def test_detect_raises_without_a_gpu(monkeypatch, tmp_path):
    import torch
    from PIL import Image
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    z = np.zeros((4, 4), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        trees.detect(z, 0.5)
    P = str(tmp_path / "dsm")
    with pytest.raises(FileNotFoundError, match="dsm_whu.py"):
        trees.from_dsm(P)
    with open(P + "_dsm.json", "w") as f:
        json.dump(dict(grid=dict(x0=0.0, y_top=2.0, gsd=0.5, W=4, H=4), z_ref=0.0), f)
    with pytest.raises(FileNotFoundError, match="dtm_whu.py"):
        trees.from_dsm(P)
    Image.fromarray(z).save(P + "_ndsm.tif", format="TIFF")
    with pytest.raises(FileNotFoundError, match=r"buildings_whu\.py.*--no_buildings"):
        trees.from_dsm(P)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        trees.from_dsm(P, no_buildings=True)


def test_parser_defaults_and_help():
    a = trees.build_parser().parse_args(["--dsm", "/x/dsm"])
    assert (a.dsm, a.no_buildings, a.min_height, a.smooth_passes, a.radius_min, a.radius_slope, a.crown_ratio, a.max_crown_radius,
            a.min_crown_area, a.out) == ("/x/dsm", False, 2.0, 1, 1.5, 0.05, 0.55, 10.0, 1.0, None)
    a = trees.build_parser().parse_args(["--dsm", "p", "--no_buildings", "--smooth_passes", "2", "--crown_ratio", "0.7", "--out", "q"])
    assert (a.no_buildings, a.smooth_passes, a.crown_ratio, a.out) == (True, 2, 0.7, "q")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "trees_whu.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "--min_height" in r.stdout and "--no_buildings" in r.stdout and "--max_crown_radius" in r.stdout
    doc = " ".join(trees.__doc__.split())
    assert "not values measured on WHU scenes" in doc and "Popescu & Wynne" in doc and "Dalponte & Coomes" in doc


def test_abi_and_the_new_signatures():
    assert _lib.ABI_VERSION == 22                                      # grown by six entry points; nothing existing changed
    for name in ("adamvs_tree_workspace_bytes", "adamvs_tree_surface", "adamvs_tree_parents", "adamvs_tree_roots", "adamvs_tree_crowns",
                 "adamvs_tree_table"):
        assert name in _lib.SIGNATURES
    assert (_lib.TREE_TILE, _lib.TREE_MAX_RADIUS, _lib.TREE_MAX_ROUNDS, _lib.TREE_NOT_CONVERGED, _lib.TREE_Q_SCALE) == (64, 64, 32, -2, 256)
    assert _lib.TREE_JUMP_HOPS == 8
    assert _lib.TREE_COLUMNS == trees.COLUMNS == COLUMNS and trees.MAX_RADIUS == _lib.TREE_MAX_RADIUS and trees.Q_SCALE == _lib.TREE_Q_SCALE
    assert _lib.TREE_Q_SCALE == _lib.ROOF_Q_SCALE
    assert ctypes.sizeof(_lib.TreeStats) == 2 * 4 + 3 * 8 + 2 * 4
    header = open(os.path.join(ROOT, "include", "adamvs_hip.h")).read()
    for k, v in (("TILE", 64), ("MAX_RADIUS", 64), ("MAX_ROUNDS", 32), ("JUMP_HOPS", 8), ("Q_SCALE", 256), ("COLUMNS", 10)):
        assert "#define ADAMVS_TREE_%s %d" % (k, v) in header
    assert "#define ADAMVS_TREE_NOT_CONVERGED (-2)" in header and "#define ADAMVS_ABI_VERSION 22" in header
    for k, name in enumerate(COLUMNS):
        assert "ADAMVS_TREE_%s = %d" % (name.upper(), k) in header
    assert "---- Trees" in header
    lib = _lib.load()
    assert lib.adamvs_tree_workspace_bytes(0, 5) < 0 and lib.adamvs_tree_workspace_bytes(1 << 15, 1 << 14) < 0
    assert lib.adamvs_tree_workspace_bytes(7, 5) == 256 + 2 * 256
    st = _lib.TreeStats()
    thr = (ctypes.c_int * 1)(0)
    assert lib.adamvs_tree_surface(4, 4, None, None, 2.0, 1, None, 0, None, None, None, None, None) < 0         # before any launch
    assert lib.adamvs_tree_parents(4, 4, None, 1, thr, None, 0, None, ctypes.byref(st), None) < 0
    assert lib.adamvs_tree_roots(4, 4, None, None, 0, None, ctypes.byref(st), None) < 0
    assert lib.adamvs_tree_crowns(4, 4, None, None, None, 550, 400, None, None, None) < 0
    assert lib.adamvs_tree_table(4, 4, None, None, None, None, 1, None, None) < 0
