"""The host side of the drainage stage (ada_mvs_amd/drainage.py) and its restatement (tests/drainage_ref.py) without a GPU: the
restatement against cases worked out by hand (a pit, a plane, a Y of three links), the parameter checks with min_cells in exact
rationals, the Strahler pass against the recursion, the GeoJSON bytes, the file names, the refusals and the new entry points."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
import drainage_ref as R
from ada_mvs_amd import _lib, buildings, contours, drainage, dsm, dtm, roofs, trees
from conftest import ROOT

GRID = dsm.Grid(100.0, 50.0, 0.5, 0.0, 5, 5)


# ---- the restatement against hand-computed cases -----------------------------------------------------------------------------
def test_ref_pit_5x5():
    """Heights 1 m with a pit of 0 m in the middle: the ring round the pit is one unit above the border, the pit two; the pit drains
    east (the first of eight equal drops, the orthogonal ones steeper than the diagonal ones)."""
    z = np.ones((5, 5), np.float32)
    z[2, 2] = 0.0
    ref = R.route(z, 0.0, 0, min_cells=2)
    assert np.array_equal(ref["r"], np.where(z == 0, 0, 65536))
    F = np.full((5, 5), 65536)
    F[1:4, 1:4] = 65537
    F[2, 2] = 65538
    assert np.array_equal(ref["F"], F)
    assert np.array_equal(ref["edge"], F == 65536)
    assert ref["dir"].tolist() == [[0, 0, 0, 0, 0], [0, 16, 64, 1, 0], [0, 16, 1, 1, 0], [0, 4, 4, 1, 0], [0, 0, 0, 0, 0]]
    acc = np.ones((5, 5), int)
    acc[1, 0] = acc[0, 2] = acc[1, 4] = acc[2, 0] = acc[3, 4] = acc[4, 1] = acc[4, 2] = 2
    acc[2, 3], acc[2, 4] = 2, 3
    assert np.array_equal(ref["acc"], acc)
    assert ref["root"][2, 2] == 14 and ref["root"][1, 1] == 5 and ref["root"][0, 0] == 0
    # streams at two cells: (2, 3) is a source and heads the one link that ends at the outlet (2, 4), which it owns (nd = 1)
    assert ref["L"] == 1 and ref["vertex"].tolist() == [13, 14] and ref["link_to"].tolist() == [-1] and ref["link_end"].tolist() == [14]
    assert ref["nd"][2, 3] == 0 and ref["nd"][2, 4] == 1 and ref["nd"][2, 2] == 255 and ref["nd"][1, 0] == 0
    assert ref["link"][2, 4] == 0 and ref["pos"][2, 4] == 1 and ref["link"][1, 0] == -1          # a head that is an outlet heads no link
    assert ref["K"] == 8 and ref["basins"][2, 2] == ref["basins"][2, 4] == 5 and ref["basins"][0, 0] == 0
    assert ref["bound"] == 1


def test_ref_plane():
    """A plane that falls one metre per cell to the east: nothing is filled, every inner cell drains east."""
    z = np.tile(np.arange(5, -1, -1, dtype=np.float32), (4, 1))
    ref = R.route(z, 0.0, 0, min_cells=3)
    assert np.array_equal(ref["F"], ref["r"]) and np.array_equal(ref["r"], z.astype(np.int64) * 65536)
    assert (ref["dir"][1:3, 1:5] == 1).all() and (ref["dir"][0] == 0).all() and (ref["dir"][:, 0] == 0).all()
    assert ref["acc"][1].tolist() == [1, 1, 2, 3, 4, 5] and ref["acc"][0].tolist() == [1] * 6
    assert ref["L"] == 2 and ref["vertex"].tolist() == [9, 10, 11, 15, 16, 17] and ref["strahler"].tolist() == [1, 1]
    assert ref["bound"] == 1
    assert R.route(z, 0.0, 0, min_cells=3, tile=2)["bound"] == 1      # every inner cell has a lower edge cell next to it
    # a flat pit of 5 x 5 cells in a 7 x 7 raster fills ring by ring; in tiles of 2 the second ring waits for the first of another tile
    z = np.ones((7, 7), np.float32)
    z[1:6, 1:6] = 0.0
    ref = R.route(z, 0.0, 0, tile=2)
    assert ref["F"][3].tolist() == [65536, 65537, 65538, 65539, 65538, 65537, 65536] and ref["bound"] == 2
    assert R.rounds_bound(ref["F"], ref["edge"], 32) == 1


def y_valley():
    """Two arms (0, 0) -> (1, 1) -> (2, 2) and (0, 4) -> (1, 3) -> (2, 2) and the trunk (2, 2) -> (3, 2) -> (4, 2) on a 5 x 5 grid."""
    F = np.full((5, 5), R.NONE, np.int64)
    recv = np.full(25, -1, np.int64)
    acc = np.zeros(25, np.int64)
    for c, to, a, f in ((0, 6, 1, 9), (6, 12, 2, 8), (4, 8, 1, 9), (8, 12, 2, 8), (12, 17, 5, 7), (17, 22, 6, 6), (22, -1, 7, 5)):
        recv[c], acc[c] = to, a
        F[c // 5, c % 5] = f
    return F, recv, acc


def test_ref_y_valley_orders_1_1_2():
    F, recv, acc = y_valley()
    st = R.streams(F, recv, acc, 1)
    assert st["L"] == 3 and st["P"] == 9
    assert st["link_head"].tolist() == [0, 4, 12] and st["link_end"].tolist() == [12, 12, 22] and st["link_to"].tolist() == [2, 2, -1]
    assert st["link_first"].tolist() == [0, 3, 6, 9] and st["vertex"].tolist() == [0, 6, 12, 4, 8, 12, 12, 17, 22]
    assert st["nd"].reshape(5, 5)[2, 2] == 2 and st["pos"].tolist()[22] == 2 and st["link"].tolist()[12] == 2
    assert R.strahler(st["link_to"]).tolist() == [1, 1, 2]
    assert drainage.strahler(st["link_to"], acc[st["link_head"]]).tolist() == [1, 1, 2]
    st = R.streams(F, recv, acc, 2)                                  # the arms start one cell lower: links of two vertices
    assert st["vertex"].tolist() == [6, 12, 8, 12, 12, 17, 22] and R.strahler(st["link_to"]).tolist() == [1, 1, 2]
    assert R.streams(F, recv, acc, 8)["L"] == 0


def test_ref_fill_is_the_fixed_point_and_drains():
    rng = np.random.default_rng(5)
    for hole in (0.0, 0.2):
        z = rng.integers(0, 4, (17, 23)).astype(np.float32) / 256
        z[rng.random(z.shape) < hole] = np.nan
        ref = R.route(z, 0.0, 0, min_cells=4, tile=8)
        F, edge, V = ref["F"], ref["edge"], ref["F"] != R.NONE
        Fp = np.pad(np.where(V, F, 2 ** 40), 1, constant_values=2 ** 40)
        low = np.min([Fp[1 + di:18 + di, 1 + dj:24 + dj] for di, dj in R.STEPS], axis=0)
        inner = V & ~edge
        assert np.array_equal(F[inner], np.maximum(ref["r"], low + 1)[inner]) and np.array_equal(F[edge], ref["r"][edge])
        assert (low[inner] < F[inner]).all() and (((ref["dir"] != 0) & (ref["dir"] != 255)) == inner).all()
        assert ref["acc"].reshape(-1)[ref["root"].reshape(-1) == np.arange(F.size)].sum() == V.sum()


# ---- parameters ---------------------------------------------------------------------------------------------------------------
def test_parameters_and_min_cells_in_exact_rationals():
    p = drainage.parameters(0.5)
    assert p == dict(min_area=1000.0, smooth_passes=1, min_length=0.0, min_cells=4000, max_rounds=None)
    for gsd, area, cells in ((0.1, 1000.0, 100000), (0.3, 0.63, 7), (0.1, 0.07, 7), (0.2, 0.12, 3), (0.16, 1000, 39063), (0.1, 0.0701, 8),
                             (1.0, 0.0, 1), (0.7, 0.49, 1), (0.7, 0.4901, 2), (0.001, 1e6, 2 ** 31 - 1)):
        assert drainage.parameters(gsd, area)["min_cells"] == cells, (gsd, area)
    for bad in (dict(min_area=-1.0), dict(min_area=float("nan")), dict(min_area=True), dict(smooth_passes=3), dict(smooth_passes=0.5),
                dict(min_length=-0.1), dict(max_rounds=0), dict(max_rounds=1.5)):
        with pytest.raises(ValueError):
            drainage.parameters(0.5, **bad)
    with pytest.raises(ValueError):
        drainage.parameters(0.0)
    assert (drainage.UNITS, drainage.TILE) == (_lib.DRAIN_UNITS, _lib.DRAIN_TILE) == (65536, 32)


# ---- Strahler orders from a link table ------------------------------------------------------------------------------------------
def test_strahler_pass_equals_the_recursion():
    assert drainage.strahler([], []).tolist() == []
    # 0, 1 -> 4; 2, 3 -> 5; 4, 5 -> 6 (order 3); 7 -> 6 (a first-order link into a third-order one changes nothing)
    to = [4, 4, 5, 5, 6, 6, -1, 6]
    acc_head = [1, 1, 1, 1, 5, 6, 20, 2]
    assert drainage.strahler(to, acc_head).tolist() == [1, 1, 1, 1, 2, 2, 3, 1] == R.strahler(to).tolist()
    assert drainage.strahler([1, 2, -1], [1, 2, 3]).tolist() == [1, 1, 1]             # a chain through junctions with outlets beside it
    rng = np.random.default_rng(11)
    for L in (1, 2, 9, 200):
        to = np.array([-1 if l == L - 1 or rng.random() < 0.05 else rng.integers(l + 1, L) for l in range(L)])
        acc_head = np.arange(L) * 3 + 1                              # a link flows into a later one: ascending acc
        perm = rng.permutation(L)                                    # numbered in any order
        inv = np.argsort(perm)
        to_p = np.where(to[perm] >= 0, inv[np.maximum(to[perm], 0)], -1)
        assert np.array_equal(drainage.strahler(to_p, acc_head[perm]), R.strahler(to_p))
        assert np.array_equal(R.strahler(to_p), R.strahler(to)[perm])


# ---- the host's columns and the GeoJSON text --------------------------------------------------------------------------------------
def y_result():
    F, recv, acc = y_valley()
    st = R.streams(F, recv, acc, 1)
    res = dict(st, F=F, acc=acc.reshape(5, 5), magnitude=R.accumulate(F, recv, (st["nd"] == 0).astype(np.int64)).reshape(5, 5),
               basins=np.where(F != R.NONE, 1, 0))
    return res


def test_link_properties_and_features():
    res = y_result()
    cols = drainage.link_properties(res, GRID)
    assert cols["own_last"].tolist() == [6, 8, 22] and cols["upstream_cells"].tolist() == [2, 2, 7] and cols["magnitude"].tolist() == [1, 1, 2]
    assert cols["strahler"].tolist() == [1, 1, 2] and cols["basin"].tolist() == [1, 1, 1]
    assert cols["drop"].tolist() == [2 / 65536, 2 / 65536, 2 / 65536]
    assert np.allclose(cols["length"], [2 * 0.5 * 2 ** 0.5, 2 * 0.5 * 2 ** 0.5, 1.0], rtol=0, atol=1e-12)
    assert cols["xy"][0].tolist() == [100.25, 49.75] and cols["xy"][8].tolist() == [101.25, 47.75]
    feats = drainage.features(res, cols, GRID)
    assert [f["properties"]["id"] for f in feats] == [1, 2, 3] and [f["properties"]["to_id"] for f in feats] == [3, 3, 0]
    assert feats[2]["properties"] == dict(id=3, strahler=2, magnitude=2, upstream_cells=7, upstream_area_m2=1.75, length_m=1.0, drop_m=2 / 65536,
                                          vertices=3, to_id=0, basin=1)
    short = drainage.features(res, cols, GRID, min_length=1.2)
    assert [f["properties"]["id"] for f in short] == [1, 2] and short[0]["properties"]["to_id"] == 3
    empty = dict(res, link_first=np.zeros(1, int), link_head=np.zeros(0, int), link_end=np.zeros(0, int), link_to=np.zeros(0, int),
                 vertex=np.zeros(0, int))
    assert drainage.features(empty, drainage.link_properties(empty, GRID), GRID) == []


def test_geojson_bytes_are_equal_for_equal_inputs():
    res = y_result()
    a = drainage.geojson_text(drainage.features(res, drainage.link_properties(res, GRID), GRID))
    b = drainage.geojson_text(drainage.features(y_result(), drainage.link_properties(y_result(), GRID), GRID))
    assert a == b and a.endswith("\n") and " " not in a
    js = json.loads(a)
    assert [tuple(f["properties"]) for f in js["features"]] == [drainage.PROPERTIES] * 3
    assert js["features"][0]["geometry"] == dict(type="LineString", coordinates=[[100.25, 49.75], [100.75, 49.25], [101.25, 48.75]])
    assert drainage.geojson_text([]) == '{"type":"FeatureCollection","features":[]}\n'
    d = drainage.sink_depth(np.array([[0, R.NONE, 65536]]), np.array([[32768, R.NONE, 65536]]))
    assert d.dtype == np.float32 and d[0, 0] == 0.5 and np.isnan(d[0, 1]) and d[0, 2] == 0.0


def test_output_paths_are_disjoint_from_every_earlier_stage():
    mine = set(drainage.output_paths("/o/p").values())
    assert mine == {"/o/p_flowdir.tif", "/o/p_flowacc.tif", "/o/p_sinkdepth.tif", "/o/p_basins.tif", "/o/p_basins.tfw", "/o/p_streams.geojson",
                    "/o/p_drainage.json"}
    for other in (dsm.output_paths("/o/p"), dsm.fill_output_paths("/o/p"), dtm.output_paths("/o/p"), buildings.output_paths("/o/p"),
                  roofs.output_paths("/o/p"), trees.output_paths("/o/p"), contours.output_paths("/o/p")):
        assert not mine & set(other.values())


# ---- the stage without a GPU, the CLI, the entry points -------------------------------------------------------------------------
def test_route_raises_without_a_gpu(monkeypatch, tmp_path):
    import torch
    from PIL import Image
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    z = np.zeros((4, 4), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        drainage.route(z, 0.5)
    with pytest.raises(ValueError, match="min_area"):
        drainage.route(z, 0.5, min_area=-1.0)
    with pytest.raises(ValueError, match="smooth_passes"):
        drainage.route(z, 0.5, smooth_passes=3)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        drainage.route(z[0], 0.5)
    P = str(tmp_path / "dsm")
    with pytest.raises(FileNotFoundError, match="dsm_whu.py"):
        drainage.from_dsm(P)
    with pytest.raises(ValueError, match="min_length"):
        drainage.from_dsm(P, min_length=-1.0)
    with open(P + "_dsm.json", "w") as f:
        json.dump(dict(grid=dict(x0=0.0, y_top=2.0, gsd=0.5, W=4, H=4), z_ref=0.0), f)
    with pytest.raises(FileNotFoundError, match="dtm_whu.py"):
        drainage.from_dsm(P)
    with pytest.raises(ValueError, match="source"):
        drainage.from_dsm(P, source="ndsm")
    Image.fromarray(z).save(P + "_dtm.tif", format="TIFF")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        drainage.from_dsm(P)
    Image.fromarray(np.zeros((3, 4), np.float32)).save(P + "_dsm.tif", format="TIFF")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(ValueError, match="the grid 4 x 4"):
        drainage.from_dsm(P, source="dsm")


def test_parser_defaults_help_and_the_stated_limits():
    a = drainage.build_parser().parse_args(["--dsm", "/x/dsm"])
    assert (a.dsm, a.source, a.min_area, a.smooth_passes, a.min_length, a.out) == ("/x/dsm", "dtm", 1000.0, 1, 0.0, None)
    a = drainage.build_parser().parse_args(["--dsm", "p", "--source", "dsm_filled", "--min_area", "250", "--smooth_passes", "2", "--min_length",
                                            "7.5", "--out", "q"])
    assert (a.source, a.min_area, a.smooth_passes, a.min_length, a.out) == ("dsm_filled", 250.0, 2, 7.5, "q")
    with pytest.raises(SystemExit):
        drainage.build_parser().parse_args(["--dsm", "p", "--source", "ndsm"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "drainage_whu.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "--min_area" in r.stdout and "--min_length" in r.stdout and "dsm_filled" in r.stdout
    doc = " ".join(drainage.__doc__.split())
    for words in ("D8 only", "no multiple flow directions", "closed basin is filled", "not smoothed", "no CRS", "are conventions",
                  "not values measured on WHU scenes"):
        assert words in doc, words


def test_the_new_entry_points_refuse_before_any_launch():
    names = ("adamvs_drain_workspace_bytes", "adamvs_drain_fill", "adamvs_drain_direction", "adamvs_drain_accumulate", "adamvs_drain_streams",
             "adamvs_drain_links")
    header = open(os.path.join(ROOT, "include", "adamvs_hip.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES and name + "(" in header
    assert "#define ADAMVS_DRAIN_TILE 32" in header and "#define ADAMVS_DRAIN_UNITS 65536" in header and "---- Drainage" in header
    assert "#define ADAMVS_DRAIN_NOT_A_FOREST (-2)" in header and _lib.DRAIN_NOT_A_FOREST == -2
    assert ctypes.sizeof(_lib.DrainStats) == 4 * 4 + 2 * 8 + 2 * 4
    lib = _lib.load()
    assert lib.adamvs_drain_workspace_bytes(0, 5) < 0 and lib.adamvs_drain_workspace_bytes(1 << 15, 1 << 14) < 0
    assert lib.adamvs_drain_workspace_bytes(7, 5) == 512 + 2 * 512 + 256 + 2 * 256
    st = _lib.DrainStats()
    assert lib.adamvs_drain_fill(4, 4, None, 0, 8, None, 0, None, None, ctypes.byref(st), None) < 0
    assert lib.adamvs_drain_direction(4, 4, None, None, None) < 0
    assert lib.adamvs_drain_accumulate(4, 4, None, None, None, 0, None, None, ctypes.byref(st), None) < 0
    assert lib.adamvs_drain_streams(4, 4, None, None, 1, None, 0, None, None, None, ctypes.byref(st), None) < 0
    assert lib.adamvs_drain_links(4, 4, None, None, None, None, 1, 2, None, 0, None, None, None, None, None, None) < 0
