"""Contour lines, host side: the level table and the parameter checks of ada_mvs_amd/contours.py, invariants of the numpy
restatement (tests/contours_ref.py) on random rasters and on a cone, the host's share (coordinates, lengths, selection, GeoJSON
text), the file names, the ABI and the CLI."""
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
import contours_ref
from ada_mvs_amd import _lib, buildings, contours, dsm, dtm, roofs, trees
from conftest import ROOT

GRID = dsm.Grid(1000.0, 5000.0, 0.5, 0.0, 41, 41)                      # gsd a power of two


# ---- the level table ------------------------------------------------------------------------------------------------------------
def test_level_table_of_a_tenth_of_a_metre():
    lev, ns = contours.level_table(0, 3 * 256, 0.0, 0.1, 0.0, 0)
    assert ns == list(range(31))
    for n, v in zip(ns, lev):
        q, r = divmod(n * 256, 10)                                      # n / 10 m in 1/256 m: never a half, so plain rounding
        assert v == q + (1 if 2 * r > 10 else 0) and 2 * r != 10
    assert lev[1] == 26 and lev[5] == 128 and lev[30] == 768
    # 0.1 is the decimal tenth, not the double next to it: level 10 is exactly 1 m
    assert contours.level_table(256, 256, 0.0, 0.1, 0.0, 0) == ([256], [10])


def test_level_table_rounds_half_to_even():
    # (1/512 + n/128) 256 = 2 n + 1/2 -> the even 2 n; (3/512 + n/128) 256 = 2 n + 3/2 -> the even 2 n + 2
    lev, ns = contours.level_table(0, 9, 0.0, Fraction(1, 128), Fraction(1, 512), 0)
    assert (lev, ns) == ([0, 2, 4, 6, 8], [0, 1, 2, 3, 4])
    lev, ns = contours.level_table(0, 9, 0.0, Fraction(1, 128), Fraction(3, 512), 0)
    assert (lev, ns) == ([2, 4, 6, 8], [0, 1, 2, 3])                    # n = 4 lies at 9.5 / 256 m, above the surface
    # the same through z_ref: levels at n metres seen from z_ref = 1/512 m lie at 256 n - 1/2
    lev, ns = contours.level_table(0, 600, 1.0 / 512, 1.0, 0.0, 0)
    assert (lev, ns) == ([256, 512], [1, 2])                            # 255.5 -> 256 and 511.5 -> 512, both even


def test_level_table_collisions_bases_and_empty_tables():
    with pytest.raises(ValueError, match="both round to"):
        contours.level_table(0, 10, 0.0, Fraction(1, 512), 0.0, 0)      # 0.5 -> 0 and 0 -> 0
    assert contours.level_table(0, 16 * 10, 0.0, Fraction(1, 512), 0.0, 1)[0] == list(range(0, 161, 8))      # fine at S = 4096
    assert contours.level_table(60, 700, 0.0, 1.0, 0.25, 0) == ([64, 320, 576], [0, 1, 2])
    assert contours.level_table(-700, -100, 0.0, 1.0, 0.25, 0) == ([-448, -192], [-2, -1])
    assert contours.level_table(100, 700, 100.0, 1.0, 0.5, 0) == ([128, 384, 640], [100, 101, 102])
    assert contours.level_table(300, 500, 0.0, 1.0, 0.0, 0) == ([], [])                # the surface lies between two levels
    assert contours.level_table(256, 256, 0.0, 1.0, 0.0, 0) == ([256], [1])            # the ends of the range are inside
    assert contours.level_table(2 ** 31 - 1, -2 ** 31, 0.0) == ([], [])                 # no valid cell
    assert contours.level_table(0, 4096 * 2, 0.0, 1.0, 0.0, 1) == ([0, 4096, 8192], [0, 1, 2])
    with pytest.raises(ValueError, match="at most 4096"):
        contours.level_table(0, 256 * 5000, 0.0, 1.0, 0.0, 0)
    assert len(contours.level_table(0, 256 * 4095, 0.0, 1.0, 0.0, 0)[0]) == 4096
    with pytest.raises(ValueError, match="interval"):
        contours.level_table(0, 10, 0.0, 0.0)


def test_parameters_and_their_errors():
    p = contours.parameters()
    assert p == dict(interval=1.0, base=0.0, major_every=5, smooth_passes=1, min_length=0.0, scale=4096)
    assert contours.parameters(0.5, -3.0, 2, 0, 12.5) == dict(interval=0.5, base=-3.0, major_every=2, smooth_passes=0, min_length=12.5, scale=256)
    assert contours.parameters(smooth_passes=2)["scale"] == 65536
    for kw in (dict(interval=0.0), dict(interval=-1.0), dict(interval=float("nan")), dict(interval=float("inf")), dict(base=float("nan")),
               dict(major_every=0), dict(major_every=2.5), dict(major_every=True), dict(smooth_passes=3), dict(smooth_passes=-1),
               dict(smooth_passes=1.5), dict(smooth_passes=True), dict(min_length=-0.1), dict(min_length=float("inf")), dict(interval=True)):
        with pytest.raises(ValueError):
            contours.parameters(**kw)


# ---- invariants of the restatement ------------------------------------------------------------------------------------------------
def random_raster(seed, H, W, density):
    rng = np.random.default_rng(seed)
    z = rng.integers(-2, 5, (H, W)).astype(np.float32) + rng.integers(0, 2, (H, W)).astype(np.float32) * 0.5
    z[rng.random((H, W)) < density] = np.nan
    return z


@pytest.mark.parametrize("seed,H,W,density,passes", [(1, 23, 31, 0.0, 0), (2, 40, 17, 0.05, 1), (3, 33, 35, 0.3, 0), (4, 30, 30, 0.1, 2)])
def test_restatement_invariants_on_random_rasters(seed, H, W, density, passes):
    z = random_raster(seed, H, W, density)
    r = contours_ref.trace(z, -1.0, passes, None, lambda lo, hi: contours.level_table(lo, hi, -1.0, 0.5, 0.0, passes)[0])
    N, M = r["N"], r["M"]
    assert N > 50 and M > 5 and int(r["count"].sum()) == N and not r["count"][-1].any() and not r["count"][:, -1].any()
    as_entry, as_exit = list(zip(r["entry"].tolist(), r["level"].tolist())), list(zip(r["exit"].tolist(), r["level"].tolist()))
    assert len(set(as_entry)) == N and len(set(as_exit)) == N              # a crossing is the entry of at most one segment, the exit of at most one
    has = np.flatnonzero(r["succ"] >= 0)
    assert np.array_equal(r["pred"][r["succ"][has]], has)                   # pred is the inverse of succ
    has = np.flatnonzero(r["pred"] >= 0)
    assert np.array_equal(r["succ"][r["pred"][has]], has)
    assert (r["vertex"][:, 1] > 0).all() and (r["vertex"][:, 1] < r["vertex"][:, 2]).all()
    # the numbering: by (block, level, entry edge); the block of a segment is where its count says
    block = np.repeat(np.arange(H * W), r["count"].reshape(-1))
    assert (np.diff(block * 8192 + r["level"]) >= 0).all()
    # per level: the distinct crossings are the grid edges of a fully valid block whose ends differ in "up"
    s = r["s"]
    valid = s != contours_ref.NONE
    full = valid[:-1, :-1] & valid[:-1, 1:] & valid[1:, 1:] & valid[1:, :-1]
    east = np.zeros((H, W), bool)                                           # the edge from (i, j) to (i, j + 1) lies in a fully valid block
    east[:-1, :-1] |= full
    east[1:, :-1] |= full
    south = np.zeros((H, W), bool)
    south[:-1, :-1] |= full
    south[:-1, 1:] |= full
    for k, level in enumerate(r["lev"]):
        up = s >= level
        want = int((east[:, :-1] & (up[:, :-1] != up[:, 1:])).sum() + (south[:-1] & (up[:-1] != up[1:])).sum())
        here = r["level"] == k
        assert len(set(r["entry"][here].tolist()) | set(r["exit"][here].tolist())) == want
    # the lines: every segment in exactly one, ranks 0 .. len - 1, rings start at their smallest segment
    assert r["line_first"][-1] == N + M and np.array_equal(np.sort(r["line_start"]), r["line_start"])
    for m in range(M):
        members = np.flatnonzero(r["start"] == r["line_start"][m])
        assert members.size + 1 == r["line_first"][m + 1] - r["line_first"][m]
        assert members.min() == r["line_start"][m] or not r["line_closed"][m]
        first, last = r["vertex"][r["line_first"][m]], r["vertex"][r["line_first"][m + 1] - 1]
        assert bool(r["line_closed"][m]) == (first.tolist() == last.tolist())


def test_cone_rings_lie_on_the_circles_and_run_counter_clockwise():
    i, j = np.meshgrid(np.arange(41), np.arange(41), indexing="ij")
    z = (10.0 - 0.5 * np.hypot(i - 20, j - 20)).astype(np.float32)
    r = contours_ref.trace(z, 0.0, 0, [256 * n for n in range(1, 10)])
    assert r["M"] == 9 and r["line_closed"].all()
    xy = contours.vertex_coordinates(r["vertex"], GRID)
    cx, cy = GRID.x0 + 20.5 * GRID.gsd, GRID.y_top - 20.5 * GRID.gsd
    length = contours.line_lengths(xy, r["line_first"])
    for m in range(9):
        p = xy[r["line_first"][m]:r["line_first"][m + 1]]
        radius = (10.0 - (int(r["line_level"][m]) + 1)) / 0.5 * GRID.gsd                 # metres
        assert np.abs(np.hypot(p[:, 0] - cx, p[:, 1] - cy) - radius).max() < GRID.gsd
        area2 = float(np.sum(p[:-1, 0] * p[1:, 1] - p[1:, 0] * p[:-1, 1]))
        assert area2 > 0 and abs(area2 / 2 - math.pi * radius ** 2) < 0.1 * math.pi * radius ** 2
        assert abs(length[m] - 2 * math.pi * radius) < 0.1 * 2 * math.pi * radius
    pit = contours_ref.trace(-z, 0.0, 0, [256 * n for n in range(-9, 0)])
    xy = contours.vertex_coordinates(pit["vertex"], GRID)
    for m in range(9):
        p = xy[pit["line_first"][m]:pit["line_first"][m + 1]]
        assert float(np.sum(p[:-1, 0] * p[1:, 1] - p[1:, 0] * p[:-1, 1])) < 0


def test_the_comb_is_one_ring_of_820_segments():
    i, j = np.meshgrid(np.arange(41), np.arange(40), indexing="ij")
    high = (np.isin(i % 4, (1, 2)) & (j >= 1) & (j <= 38) & (i <= 39)) | ((j == 1) & (i >= 1) & (i <= 39))
    r = contours_ref.trace(high.astype(np.float32), 0.0, 0, [128])
    assert (r["N"], r["M"]) == (820, 1) and r["line_closed"].tolist() == [1] and r["line_start"].tolist() == [0]


# ---- the host's share --------------------------------------------------------------------------------------------------------------
def hand_made():
    """Two lines on a 4 x 5 grid at gsd 0.5: an open one of three vertices and a closed one of five."""
    W = 5
    code = lambda i, j, d: 2 * (i * W + j) + d
    vertex = np.array([(code(0, 1, 1), 1, 2), (code(1, 1, 0), 1, 4), (code(1, 2, 1), 3, 4),
                       (code(2, 2, 0), 1, 2), (code(2, 3, 1), 1, 2), (code(3, 2, 0), 1, 2), (code(2, 2, 1), 1, 2), (code(2, 2, 0), 1, 2)], np.int64)
    return vertex, np.array([0, 3, 8], np.int64), dsm.Grid(100.0, 50.0, 0.5, 0.0, W, 4)


def test_coordinates_lengths_and_selection():
    vertex, line_first, grid = hand_made()
    xy = contours.vertex_coordinates(vertex, grid)
    assert xy[0].tolist() == [100.0 + 1.5 * 0.5, 50.0 - (0.5 + 0.5) * 0.5] and xy[1].tolist() == [100.0 + (1.5 + 0.25) * 0.5, 50.0 - 1.5 * 0.5]
    assert xy[2].tolist() == [100.0 + 2.5 * 0.5, 50.0 - (1.5 + 0.75) * 0.5]
    length = contours.line_lengths(xy, line_first)
    want0 = math.hypot(*(xy[1] - xy[0])) + math.hypot(*(xy[2] - xy[1]))
    assert length.shape == (2,) and abs(length[0] - want0) < 1e-12 and abs(length[1] - 4 * math.hypot(0.25, 0.25)) < 1e-12
    assert contours.line_lengths(np.zeros((0, 2)), np.array([0])).shape == (0,)
    assert contours.select(length, [3, 1]).tolist() == [1, 0]              # by level, then by line number
    assert contours.select(length, [1, 1]).tolist() == [0, 1]
    assert contours.select(length, [3, 1], min_length=1.0).tolist() == [1] and length[0] < 1.0 <= length[1]
    assert contours.select(length, [3, 1], min_length=float(length[1])).tolist() == [1]           # inclusive


def test_geojson_text_is_stable_and_rings_repeat_their_first_vertex():
    vertex, line_first, grid = hand_made()
    xy = contours.vertex_coordinates(vertex, grid)
    length = contours.line_lengths(xy, line_first)
    p = contours.parameters(interval=0.5, base=100.0, major_every=5)
    ns = [7, 8, 9, 10]
    order = contours.select(length, [3, 1])
    feats = contours.features(xy, line_first, [3, 1], [0, 1], length, order, ns, p)
    text = contours.geojson_text(feats)
    assert text == contours.geojson_text(contours.features(xy.copy(), line_first, [3, 1], [0, 1], length, order, ns, p)) and text.endswith("}\n")
    fc = json.loads(text)
    assert fc["type"] == "FeatureCollection" and len(fc["features"]) == 2
    a, b = fc["features"]
    assert list(a["properties"]) == list(contours.PROPERTIES) == ["id", "elevation_m", "level", "major", "closed", "vertices", "length_m"]
    assert a["properties"] == dict(id=1, elevation_m=104.0, level=8, major=False, closed=True, vertices=5, length_m=float(length[1]))
    assert b["properties"] == dict(id=2, elevation_m=105.0, level=10, major=True, closed=False, vertices=3, length_m=float(length[0]))
    assert a["geometry"]["type"] == "LineString" and a["geometry"]["coordinates"][0] == a["geometry"]["coordinates"][-1]
    assert b["geometry"]["coordinates"] == xy[:3].tolist() and b["geometry"]["coordinates"][0] != b["geometry"]["coordinates"][-1]
    assert text.index('"id"') < text.index('"elevation_m"') < text.index('"level"') < text.index('"major"') < text.index('"closed"') \
        < text.index('"vertices"') < text.index('"length_m"') and " " not in text
    assert contours.geojson_text([]) == '{"type":"FeatureCollection","features":[]}\n'


def test_output_paths_are_disjoint_from_every_earlier_stage():
    mine = set(contours.output_paths("/o/p").values())
    assert mine == {"/o/p_contours.geojson", "/o/p_contours.json"}
    for other in (dsm.output_paths("/o/p"), dsm.fill_output_paths("/o/p"), dtm.output_paths("/o/p"), buildings.output_paths("/o/p"),
                  roofs.output_paths("/o/p"), trees.output_paths("/o/p")):
        assert not mine & set(other.values())


# ---- the stage without a GPU, the CLI, the ABI ------------------------------------------------------------------------------------
def test_trace_raises_without_a_gpu(monkeypatch, tmp_path):
    import torch
    from PIL import Image
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    z = np.zeros((4, 4), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        contours.trace(z, 0.5)
    with pytest.raises(ValueError, match="interval"):
        contours.trace(z, 0.5, interval=0.0)
    P = str(tmp_path / "dsm")
    with pytest.raises(FileNotFoundError, match="dsm_whu.py"):
        contours.from_dsm(P)
    with open(P + "_dsm.json", "w") as f:
        json.dump(dict(grid=dict(x0=0.0, y_top=2.0, gsd=0.5, W=4, H=4), z_ref=0.0), f)
    with pytest.raises(FileNotFoundError, match="dtm_whu.py"):
        contours.from_dsm(P)
    with pytest.raises(ValueError, match="source"):
        contours.from_dsm(P, source="ortho")
    Image.fromarray(z).save(P + "_dtm.tif", format="TIFF")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        contours.from_dsm(P)


def test_parser_defaults_and_help():
    a = contours.build_parser().parse_args(["--dsm", "/x/dsm"])
    assert (a.dsm, a.source, a.interval, a.base, a.major_every, a.smooth_passes, a.min_length, a.out) == ("/x/dsm", "dtm", 1.0, 0.0, 5, 1, 0.0, None)
    a = contours.build_parser().parse_args(["--dsm", "p", "--source", "ndsm", "--interval", "0.25", "--base", "-1", "--major_every", "4",
                                            "--smooth_passes", "2", "--min_length", "7.5", "--out", "q"])
    assert (a.source, a.interval, a.base, a.major_every, a.smooth_passes, a.min_length, a.out) == ("ndsm", 0.25, -1.0, 4, 2, 7.5, "q")
    with pytest.raises(SystemExit):
        contours.build_parser().parse_args(["--dsm", "p", "--source", "ortho"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "contours_whu.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "--interval" in r.stdout and "--major_every" in r.stdout and "--min_length" in r.stdout and "dsm_filled" in r.stdout
    doc = " ".join(contours.__doc__.split())
    assert "conventions of topographic mapping" in doc and "not values measured on WHU scenes" in doc


def test_abi_and_the_new_signatures():
    assert _lib.ABI_VERSION == 22                                      # grown by seven entry points; nothing existing changed
    names = ("adamvs_contour_workspace_bytes", "adamvs_contour_rank_workspace_bytes", "adamvs_contour_surface", "adamvs_contour_count",
             "adamvs_contour_segments", "adamvs_contour_rank", "adamvs_contour_lines")
    header = open(os.path.join(ROOT, "include", "adamvs_hip.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES and name + "(" in header
    assert (_lib.CONTOUR_TILE, _lib.CONTOUR_MAX_LEVELS, _lib.CONTOUR_MAX_ROUNDS, _lib.CONTOUR_Q_SCALE, _lib.CONTOUR_MAX_ABS_M,
            _lib.CONTOUR_NOT_CONVERGED, _lib.CONTOUR_TOO_MANY) == (64, 4096, 64, 256, 8191, -2, -3)
    assert (contours.Q_SCALE, contours.MAX_LEVELS, contours.MAX_ABS_M) == (_lib.CONTOUR_Q_SCALE, _lib.CONTOUR_MAX_LEVELS, _lib.CONTOUR_MAX_ABS_M)
    assert _lib.CONTOUR_Q_SCALE == _lib.TREE_Q_SCALE
    for k, v in (("TILE", 64), ("MAX_LEVELS", 4096), ("MAX_ROUNDS", 64), ("Q_SCALE", 256), ("MAX_ABS_M", 8191)):
        assert "#define ADAMVS_CONTOUR_%s %d" % (k, v) in header
    assert "#define ADAMVS_CONTOUR_NOT_CONVERGED (-2)" in header and "#define ADAMVS_CONTOUR_TOO_MANY (-3)" in header
    assert "#define ADAMVS_ABI_VERSION 22" in header and "---- Contours" in header
    assert ctypes.sizeof(_lib.ContourStats) == 6 * 4 + 2 * 8 + 2 * 4
    lib = _lib.load()
    assert lib.adamvs_contour_workspace_bytes(0, 5) < 0 and lib.adamvs_contour_workspace_bytes(5, -1) < 0
    assert lib.adamvs_contour_workspace_bytes(1 << 15, 1 << 14) < 0
    assert lib.adamvs_contour_workspace_bytes(7, 5) == 512 + 16384 + 2 * 256 + 256 + 2 * 256
    assert lib.adamvs_contour_workspace_bytes(1, 1) > 0
    assert lib.adamvs_contour_rank_workspace_bytes(-1) < 0 and lib.adamvs_contour_rank_workspace_bytes(1 << 31) < 0
    assert lib.adamvs_contour_rank_workspace_bytes(0) == 512 + 16384 + 5 * 256
    assert lib.adamvs_contour_rank_workspace_bytes(1000) == 512 + 16384 + 2 * 8192 + 4096 + 2 * 256
    st = _lib.ContourStats()
    lev = (ctypes.c_int * 2)(0, 256)
    assert lib.adamvs_contour_surface(4, 4, None, 0.0, 1, None, 0, None, None, None) < 0                      # before any launch
    assert lib.adamvs_contour_count(4, 4, None, 2, lev, None, 0, None, ctypes.byref(st), None) < 0
    assert lib.adamvs_contour_segments(4, 4, None, 2, lev, 3, None, 0, None, None, None, None, None, None) < 0
    assert lib.adamvs_contour_rank(3, None, None, 0, None, None, None, ctypes.byref(st), None) < 0
    assert lib.adamvs_contour_lines(4, 4, None, 2, lev, 3, 1, None, None, None, None, None, None, None, None, 0, None, None, None, None, None,
                                    None) < 0
    assert b"null pointer" in lib.adamvs_last_error_string()
