"""Host side of the LoD2 stage (ada_mvs_amd/lod2.py) without a GPU: the planes as integers and the one corner-height function
(Python, the restatement and the library's own host entry), the face assembly on hand-written run records and on the records of
the restatement (tests/lod2_ref.py) for every scene, the three files, the refusals, the file names and the header's constants
against _lib."""
import json
import os

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, buildings, contours, dsm, dtm, hip_ops, lod2, roofs, trees
from conftest import ROOT
import lod2_ref as R


def host_model(sc, rounds=R.MAX_FILL):
    """The scene through the restatement's steps 1 - 4 and lod2's step 5 -> (the restatement's dict, the model with what the
    writers need of extract()'s dict)."""
    r = R.run_ref(sc["dtm"], sc["building"], sc["roof"], sc["properties"], sc["grid"], rounds)
    m = lod2.solids_from_runs(R.records_array(r["runs"]), r["table"], r["refused"], r["plane_building"], sc["properties"], sc["grid"], r["z_ref"])
    m.update(params=dict(fill_rounds=rounds), fill_stats=dict(rounds=rounds), seconds=dict(faces=0.0))
    return r, m


# ---- step 1 -------------------------------------------------------------------------------------------------------------------
def test_integer_planes_are_the_restatements_and_one_function_gives_the_corner_heights():
    sc = R.scene("gable_rough")
    planes, pb = lod2.integer_planes(sc["properties"], sc["grid"], 3.0)
    want, wpb = R.integer_planes_ref(sc["properties"], sc["grid"], 3.0)
    assert planes.dtype == np.int64 and planes.tolist() == want.tolist() and pb.tolist() == wpb.tolist() == [1, 1]
    # the plane of the scene: 0.3 m per cell east, 0.07 south, 6.01 - 3 m at the centre of cell (0, 0), to 2^-20 m
    assert abs(planes[0, 0] - 0.3 * 2 ** 20) <= 1 and abs(planes[0, 1] - 0.07 * 2 ** 20) <= 1 and abs(planes[0, 2] - 3.01 * 2 ** 20) <= 2
    # through JSON text and back: the file route reads the same integers
    again = json.loads(json.dumps(sc["properties"]))
    assert lod2.integer_planes(again, sc["grid"], 3.0)[0].tolist() == planes.tolist()
    rng = np.random.default_rng(0)
    P = 40
    rand = np.concatenate([rng.integers(-2 ** 39, 2 ** 39, (P, 2)), rng.integers(-2 ** 49, 2 ** 49, (P, 1))], axis=1).astype(np.int64)
    rand[:4] = [[0, 0, 0], [1, 1, 511], [-1, -1, -513], [2 ** 40 - 1, -(2 ** 40 - 1), 2 ** 50 - 1]]
    plane = rng.integers(1, P + 1, 500).astype(np.int32)
    row, col = rng.integers(0, 32769, 500).astype(np.int32), rng.integers(0, 32769, 500).astype(np.int32)
    row[:4], col[:4] = [0, 0, 32768, 32768], [0, 32768, 0, 32768]
    got = hip_ops.lod2_corner_heights_host(rand, plane, row, col)            # csrc/lod2_plane.h, compiled for the host
    for k in range(500):
        want_z = R.corner_height_ref(rand[plane[k] - 1], int(row[k]), int(col[k]))
        assert int(got[k]) == want_z == lod2.corner_height(rand[plane[k] - 1], int(row[k]), int(col[k]))
    # round half up, also below zero: (n + 1024) / 2048 floored
    assert [lod2.corner_height((0, 0, c), 0, 0) for c in (511, 512, 1535, 1536, -512, -513, -1536, -1537)] == [0, 1, 1, 2, 0, -1, -1, -2]
    assert R.corner_grid(planes[0], 22, 26)[5, 7] == lod2.corner_height(planes[0], 5, 7)
    with pytest.raises(_lib.AdaMVSHipError, match="plane 3"):
        hip_ops.lod2_corner_heights_host(rand[:2], [3], [0], [0])


def test_planes_out_of_range_are_refused():
    g = dsm.Grid(0.0, 8.0, 0.5, 0.0, 16, 16)

    def prop(**kw):
        pl = dict(z0=10.0, sx=0.1, sy=0.0, xc=1.0, yc=1.0)
        pl.update(kw)
        return [dict(id=1, building=1, plane=pl)]
    lod2.integer_planes(prop(), g, 0.0)
    for kw in (dict(z0=float("nan")), dict(sx=float("inf")), dict(sx=1e13), dict(z0=2e6), dict(z0=-2e6)):
        with pytest.raises(ValueError):
            lod2.integer_planes(prop(**kw), g, 0.0)
    with pytest.raises(ValueError, match="order of their ids"):
        lod2.integer_planes([dict(id=2, building=1, plane=prop()[0]["plane"])], g, 0.0)
    with pytest.raises(ValueError, match="building"):
        lod2.integer_planes([dict(id=1, building=0, plane=prop()[0]["plane"])], g, 0.0)


# ---- step 5 on hand-written records -------------------------------------------------------------------------------------------
def test_faces_of_one_cell_by_hand():
    """One cell under a flat plane 2 m above its base: four runs; a cube of 1024 x 1024 x 2048 units."""
    runs = [(0, 0, 0, 1, 0, 1, 0, 0, 2048, 2048), (0, 1, 0, 1, 1, 0, 2048, 2048, 0, 0),
            (1, 0, 0, 1, 1, 0, 2048, 2048, 0, 0), (1, 1, 0, 1, 0, 1, 0, 0, 2048, 2048)]
    (fs,) = lod2.faces(runs, [0], [1], 1).values()
    assert [f["kind"] for f in fs] == ["roof", "wall", "wall", "wall", "wall", "ground"]
    assert fs[0]["plane"] == 1 and len(fs[0]["rings"]) == 1 and sorted(fs[0]["rings"][0]) == [(0, 0, 2048), (0, 1024, 2048), (1024, 0, 2048), (1024, 1024, 2048)]
    assert sorted(fs[-1]["rings"][0]) == [(0, 0, 0), (0, 1024, 0), (1024, 0, 0), (1024, 1024, 0)]
    assert R.check_solid(fs, np.array([[0, 0, 2 * 2 ** 20]]), 1, 0) == 6 * 1024 * 1024 * 2048
    assert lod2.edge_census(fs) == (0, 0)
    # the north wall (line 0: outside on the left = north) faces north, the west wall west
    north = fs[1]
    assert {v[1] for v in north["rings"][0]} == {1024} and R._normal2(north["rings"][0])[1] > 0
    west = fs[3]
    assert {v[0] for v in west["rings"][0]} == {0} and R._normal2(west["rings"][0])[0] < 0
    assert lod2.faces(np.array(runs, np.int32).T, [0], [1], 1) == lod2.faces(runs, [0], [1], 1)
    assert lod2.faces([], [], [], 4) == {} and lod2.faces(np.zeros((10, 0), np.int32), [], [], 4) == {}
    with pytest.raises(ValueError):
        lod2.faces(np.zeros((4, 10), np.int32), [], [], 4)


def test_a_crossing_by_hand():
    """Two cells side by side: plane 1 flat at 2048, plane 2 falls south from 2148 to 1948.  Along their common edge the higher
    side changes: two triangles that meet in X = the middle of the edge at 2048, and X is a vertex of both roofs."""
    runs = [(0, 0, 0, 1, 0, 1, 0, 0, 2048, 2048), (0, 0, 1, 2, 0, 2, 0, 0, 2148, 2148),
            (0, 1, 0, 1, 1, 0, 2048, 2048, 0, 0), (0, 1, 1, 2, 2, 0, 1948, 1948, 0, 0),
            (1, 0, 0, 1, 1, 0, 2048, 2048, 0, 0), (1, 1, 0, 1, 2, 1, 2148, 1948, 2048, 2048), (1, 2, 0, 1, 0, 2, 0, 0, 2148, 1948)]
    (fs,) = lod2.faces(runs, [0], [1, 1], 1).values()
    X = (1024, 512, 2048)
    walls = [f["rings"][0] for f in fs if f["kind"] == "wall"]
    tri = [w for w in walls if X in w]
    assert len(tri) == 2 and all(len(w) == 3 for w in tri)
    assert {v for w in tri for v in w} == {X, (1024, 1024, 2048), (1024, 1024, 2148), (1024, 0, 2048), (1024, 0, 1948)}
    # each triangle faces its lower side: north of X plane 2 (east) is higher, so the wall faces west; south of X it faces east
    for w in tri:
        upper_half = any(v[1] == 1024 for v in w)
        assert (R._normal2(w)[0] < 0) == upper_half
    roofs_ = {f["plane"]: f["rings"][0] for f in fs if f["kind"] == "roof"}
    assert X in roofs_[1] and X in roofs_[2] and len(roofs_[1]) == len(roofs_[2]) == 5
    assert lod2.edge_census(fs)[0] == 0
    # the node (0, 1) holds the heights 0, 2048 and 2148: the outer wall of plane 2 above it starts there at 0 and passes 2048 ... only
    # on the edge that the two walls share
    north2 = next(w for w in walls if {v[1] for v in w} == {1024} and max(v[0] for v in w) == 2048)
    assert (1024, 1024, 2048) in north2 and (1024, 1024, 2148) in north2 and len(north2) == 5
    with pytest.raises(ValueError, match="buildings 2 and 1 share a cell edge on vertical line 1 at 0"):      # the same runs, two buildings
        lod2.faces(runs, [0, 0], [1, 2], 1)
    with pytest.raises(ValueError, match="base crosses"):
        lod2.faces([(0, 0, 0, 1, 0, 1, 100, 100, 50, 150)], [100], [1], 1)


# ---- step 5 on the restatement's records --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.SCENES)
def test_every_scene_gives_closed_solids_of_the_cells_volume(name, tmp_path):
    sc = R.scene(name)
    r, m = host_model(sc)
    got = R.check_model(m, r["label"], sc["building"], r["planes"], r["base"], R.GSD)
    fs = m["solids"][1]
    roofs_ = [f for f in fs if f["kind"] == "roof"]
    ground = [f for f in fs if f["kind"] == "ground"]
    lattice = lambda v: v[0] % 1024 == 0 and v[1] % 1024 == 0                # noqa: E731
    off = {v for f in fs for ring in f["rings"] for v in ring if not lattice(v)}
    if name in ("gable", "gable_rough"):
        assert len(roofs_) == 2 and len(off) >= 2                           # crossings: vertices between the lattice corners
        assert all(sum(v in ring for f in roofs_ for ring in f["rings"]) == 2 for v in off)     # each X in both roofs
        assert r["counts"][:3].tolist() == [8, 1, 0] and (r["label"][sc["building"] > 0] > 0).all()
    else:
        assert not off
    if name == "hip":
        assert len(roofs_) == 4 and sorted(m["buildings"][1]["roof_planes"]) == [1, 2, 3, 4]
    if name == "penthouse":
        # the corner (12, 8): planes 1, 2 and 3 at 7, 10 and 8.5 m above z_ref = 3 meet there
        x, y = 1024 * 8, 1024 * (22 - 12)
        assert {v[2] for f in fs for ring in f["rings"] for v in ring if v[:2] == (x, y)} >= {7 * 1024, 10 * 1024, 8704}
    if name == "courtyard":
        assert [len(f["rings"]) for f in roofs_] == [2] and [len(f["rings"]) for f in ground] == [2]
        assert m["buildings"][1]["footprint_m2"] == (18 * 10 + 8 * 12 - 16) * 0.25
    if name == "corner":
        assert len(roofs_) == 4 and m["counts"]["edges_used_by_more_than_two_faces"] == 1      # the vertical edge in the middle
    if name == "pinch":
        assert len(roofs_) == 4 and sorted(f["plane"] for f in roofs_) == [1, 1, 2, 2]          # the left turn keeps the blocks apart
    if name == "two":
        assert sorted(m["solids"]) == [1] and m["refused"] == {2: "no_plane"}
        assert m["counts"]["refused_by_reason"] == dict(no_plane=1, no_terrain=0, base_not_below_roof=0)
        assert m["counts"]["buildings"] == 2 and (r["label"][sc["building"] == 2] == 0).all()
    assert len(got) == 1
    city, js = R.check_files(str(tmp_path / name), m, r["label"])
    assert js["refused"] == {str(k): v for k, v in m["refused"].items()}


def test_refusal_reasons():
    table = np.array([[4, 4, 4, 4, 0], [4, 0, 2, 4, 0], [100, 100, R.MIN_START, 5000, R.MIN_START], [5000, R.MIN_START, 5000, 5000, R.MIN_START]], np.int64)
    assert lod2.refusals(table) == R.refused_ref(table) == {2: "no_plane", 3: "no_terrain", 4: "base_not_below_roof"}
    # a terrain above the roof: the scene's terrain raised by 20 m under the building
    sc = R.scene("penthouse")
    sc["dtm"] = sc["dtm"].copy()
    sc["dtm"][sc["building"] > 0] += 20.0
    r, m = host_model(sc)
    assert m["refused"] == {1: "base_not_below_roof"} and m["solids"] == {} and r["runs"] == []
    sc["dtm"][sc["building"] > 0] = np.nan
    assert host_model(sc)[1]["refused"] == {1: "no_terrain"}


def test_a_shift_by_whole_cells_moves_the_solids_and_nothing_else():
    for name in ("gable", "courtyard"):
        base_faces = host_model(R.scene(name))[1]["solids"]
        moved = host_model(R.scene(name, shift=(3, 5)))[1]["solids"]
        assert sorted(moved) == sorted(base_faces)
        for k in base_faces:
            shifted = [dict(f, rings=[[(x + 5 * 1024, y, z) for x, y, z in ring] for ring in f["rings"]]) for f in base_faces[k]]
            assert moved[k] == shifted


def test_the_files_are_the_same_bytes_from_the_same_model(tmp_path):
    sc = R.scene("hip")
    for k in (0, 1):
        _, m = host_model(sc)
        m["seconds"] = dict(faces=float(k))
        lod2.write_outputs(str(tmp_path / ("run%d" % k)), m, seconds=False)
    for key in ("cityjson", "obj", "json"):
        a, b = (open(lod2.output_paths(str(tmp_path / ("run%d" % k)))[key], "rb").read() for k in (0, 1))
        assert a == b and len(a) > 100
    assert "seconds" in lod2.summary(m) and "seconds" not in lod2.summary(m, seconds=False)


def test_triangulation_bridges_holes_and_keeps_the_shell_closed():
    outer = [(0, 0, 0), (4, 0, 0), (4, 4, 0), (0, 4, 0)]
    hole = [(1, 1, 0), (1, 2, 0), (2, 2, 0), (2, 1, 0)]
    tris = lod2.triangulate([outer, hole])
    assert all(len(set(t)) == 3 for t in tris) and all(t[0] == outer[0] for t in tris)
    # signed area of the fans = the outer ring less the hole
    area2 = sum((b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1]) for a, b, c in tris)
    assert area2 == 2 * (16 - 1)
    assert lod2.triangulate([outer]) == [(outer[0], outer[1], outer[2]), (outer[0], outer[2], outer[3])]


# ---- refusals, names, constants -----------------------------------------------------------------------------------------------
def test_parameters_and_shapes_are_checked_before_the_device(monkeypatch):
    sc = R.scene("hip")
    args = (sc["dtm"], sc["building"], sc["roof"], sc["properties"], R.GSD)
    assert lod2.parameters(0.5) == dict(fill_rounds=1024) and lod2.parameters(0.5, 0)["fill_rounds"] == 0
    for bad in (-1, 1025, 1.5, True):
        with pytest.raises(ValueError, match="fill_rounds"):
            lod2.parameters(0.5, bad)
    for gsd in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            lod2.parameters(gsd)
    with pytest.raises(ValueError, match="one \\[H, W\\]"):
        lod2.extract(sc["dtm"][:, :-1], sc["building"], sc["roof"], sc["properties"], R.GSD)
    with pytest.raises(ValueError, match="one \\[H, W\\]"):
        lod2.extract(sc["dtm"], sc["building"], sc["roof"][:-1], sc["properties"], R.GSD)
    with pytest.raises(ValueError, match="integer labels"):
        lod2.extract(sc["dtm"], sc["building"].astype(np.float32), sc["roof"], sc["properties"], R.GSD)
    with pytest.raises(ValueError, match="integer labels"):
        lod2.extract(sc["dtm"], sc["building"], sc["roof"].astype(np.float64), sc["properties"], R.GSD)
    with pytest.raises(ValueError, match="at most 32768 on a side"):
        lod2.extract(np.zeros((1, 32769), np.float32), np.zeros((1, 32769), np.int32), np.zeros((1, 32769), np.int32), [], R.GSD)
    with pytest.raises(ValueError, match="roof_label"):
        lod2.extract(sc["dtm"], sc["building"], sc["roof"] + 4, sc["properties"], R.GSD)       # labels above the number of planes
    with pytest.raises(ValueError, match="the grid is"):
        lod2.extract(*args, grid=dsm.Grid(0.0, 1.0, 0.5, 0.0, 5, 4))
    with pytest.raises(ValueError, match="fill_rounds"):
        lod2.extract(*args, fill_rounds=2000)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="lod2: needs an MI355X \\(there is no CPU fallback"):
        lod2.extract(*args)


def test_missing_files_name_the_stage_to_run(tmp_path, monkeypatch):
    _write_inputs = R.write_inputs
    sc = R.scene("hip")
    hints = ["dsm_whu.py --out", r"_dtm\.tif: no terrain \(run dtm_whu\.py --dsm", r"_buildings\.tif: no building labels \(run buildings_whu\.py --dsm",
             r"_roofs\.tif: no roof labels \(run roofs_whu\.py --dsm", r"_roofs\.geojson: no roof planes \(run roofs_whu\.py --dsm"]
    for upto, hint in enumerate(hints):
        with pytest.raises(FileNotFoundError, match=hint):
            lod2.from_dsm(_write_inputs(tmp_path, sc, upto))
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # every file there: the device is asked for next
        lod2.from_dsm(_write_inputs(tmp_path, sc, 5))


def test_output_paths_are_disjoint_from_every_earlier_stage():
    mine = set(lod2.output_paths("/x/dsm").values())
    assert mine == {"/x/dsm_lod2.city.json", "/x/dsm_lod2.obj", "/x/dsm_lod2.json"}
    others = set()
    for paths in (dsm.output_paths, dsm.fill_output_paths, dtm.output_paths, buildings.output_paths, roofs.output_paths, trees.output_paths,
                  contours.output_paths):
        others |= set(paths("/x/dsm").values())
    assert not mine & others
    ap = lod2.build_parser()
    assert ap.parse_args(["--dsm", "p"]).fill_rounds == 1024 and ap.parse_args(["--dsm", "p", "--out", "q"]).out == "q"
    shim = open(os.path.join(ROOT, "lod2_whu.py")).read()
    assert "from ada_mvs_amd.lod2 import main" in shim


def test_abi_constants_and_argument_errors_before_any_launch():
    assert _lib.ABI_VERSION == 22                                      # grown by seven entry points; nothing existing changed
    names = ("adamvs_lod2_workspace_bytes", "adamvs_lod2_corner_heights_host", "adamvs_lod2_fill", "adamvs_lod2_table", "adamvs_lod2_transpose",
             "adamvs_lod2_count", "adamvs_lod2_runs")
    header = open(os.path.join(ROOT, "include", "adamvs_hip.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES and name + "(" in header
        decl = header[header.index(name + "("):]
        decl = decl[:decl.index(");")]
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("adamvs_lod2_")) == sorted(names)
    assert (_lib.LOD2_MAX_SIDE, _lib.LOD2_MAX_FILL, _lib.LOD2_Z_SCALE, _lib.LOD2_XY_SCALE, _lib.LOD2_PLANE_BITS, _lib.LOD2_Z_MAX, _lib.LOD2_BLOCK) \
        == (32768, 1024, 1024, 1024, 20, 2 ** 30, 256)
    assert (lod2.MAX_SIDE, lod2.MAX_FILL, lod2.Z_SCALE, lod2.XY_SCALE, lod2.PLANE_BITS, lod2.Z_MAX) \
        == (_lib.LOD2_MAX_SIDE, _lib.LOD2_MAX_FILL, _lib.LOD2_Z_SCALE, _lib.LOD2_XY_SCALE, _lib.LOD2_PLANE_BITS, _lib.LOD2_Z_MAX)
    assert _lib.LOD2_COLUMNS == lod2.COLUMNS and _lib.LOD2_FIELDS == lod2.FIELDS == R.FIELDS and R.MAX_FILL == _lib.LOD2_MAX_FILL
    assert lod2.MIN_START == R.MIN_START == 2 ** 31 - 1 and lod2.FILL_CHUNK < 20
    for k, v in (("MAX_SIDE", 32768), ("MAX_FILL", 1024), ("Z_SCALE", 1024), ("XY_SCALE", 1024), ("PLANE_BITS", 20), ("Z_MAX", 2 ** 30), ("BLOCK", 256),
                 ("COLUMNS", 4), ("FIELDS", 10)):
        assert "#define ADAMVS_LOD2_%s %d" % (k, v) in header
    for k, name in enumerate(_lib.LOD2_COLUMNS):
        assert "ADAMVS_LOD2_%s = %d" % (name.upper(), k) in header
    for k, name in enumerate(_lib.LOD2_FIELDS):
        assert "ADAMVS_LOD2_F_%s = %d" % (name.upper(), k) in header
    assert "---- LoD2 solids" in header and header.index("LoD2 solids") > header.index("Roof planes")
    # the bound the header states for the corner height's sum
    assert (2 ** 40) * (2 ** 16) * 2 + 2 * 2 ** 50 + 2 ** 10 < 2 ** 58
    lib = _lib.load()
    assert lib.adamvs_lod2_workspace_bytes(0, 5) < 0 and lib.adamvs_lod2_workspace_bytes((1 << 15) + 1, 2) < 0
    assert lib.adamvs_lod2_workspace_bytes(1 << 15, (1 << 13) + 1) < 0 and lib.adamvs_lod2_workspace_bytes(1 << 15, 1 << 13) > 0
    # 7 x 5: 6 * 7 = 42 horizontal and 8 * 5 = 40 vertical edges: one workgroup each; two words, then three
    assert lib.adamvs_lod2_workspace_bytes(7, 5) == 512
    nb = (130 * 129 + 255) // 256 + (130 * 129 + 255) // 256
    assert lib.adamvs_lod2_workspace_bytes(129, 129) == ((4 * nb + 255) & ~255) + ((4 * (nb + 1) + 255) & ~255)
    assert lib.adamvs_lod2_fill(4, 4, None, 1, 0, 1, None, None, None, None) < 0                     # before any launch
    assert lib.adamvs_lod2_table(4, 4, None, None, None, 0.0, 1, 1, None, None, None) < 0
    assert lib.adamvs_lod2_transpose(4, 4, None, None, None) < 0
    assert lib.adamvs_lod2_count(4, 4, None, None, 1, None, 0, None, None) < 0
    assert lib.adamvs_lod2_runs(4, 4, None, None, 1, None, None, 1, None, 0, None, None) < 0
    assert b"null pointer" in lib.adamvs_last_error_string()
    assert lib.adamvs_lod2_corner_heights_host(1, None, 1, None, None, None, None) < 0
