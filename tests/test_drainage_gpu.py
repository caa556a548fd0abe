"""The drainage stage on the GPU (csrc/dsm_drainage.hip through hip_ops and ada_mvs_amd/drainage.py) against the host restatement
(tests/drainage_ref.py): s, r, F, dir, acc, root, the magnitude raster, basins, nd, link, pos, the link table and every vertex for
exact equality, at every edge of the tiles, on flats, pits, nested depressions, holes, an island, the diagonal ties, a serpentine
channel through nine tiles and a comb of tributaries; the rounds of the fill against the header's bound, the round cap, run-to-run
identity, the refusals and drainage_whu.py end to end.  There is no tolerance and nothing is left out."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
import drainage_ref as R
from ada_mvs_amd import _lib, drainage, dsm, dtm
from conftest import ROOT

pytestmark = pytest.mark.gpu

T = _lib.DRAIN_TILE
RASTERS = (("s", np.int32), ("r", np.int32), ("F", np.int32), ("dir", np.uint8), ("acc", np.int32), ("root", np.int32), ("magnitude", np.int32),
           ("basins", np.int32), ("nd", np.uint8), ("link", np.int32), ("pos", np.int32))
TABLES = ("link_first", "link_head", "link_end", "link_to", "vertex")


def check_stage(z, z_ref=0.0, passes=0, min_cells=1, max_rounds=None):
    """The GPU result equals the restatement in every word.  gsd = 1: min_area is min_cells.  -> (got, ref)."""
    z = np.asarray(z, np.float32)
    ref = R.route(z, z_ref, passes, min_cells, T)
    got = drainage.route(z, 1.0, z_ref, float(min_cells), passes, 0.0, max_rounds)
    assert got["params"]["min_cells"] == min_cells
    for name, dtype in RASTERS:
        assert got[name].dtype == dtype and got[name].shape == z.shape, name
        assert np.array_equal(got[name], ref[name]), (name, np.argwhere(got[name] != ref[name])[:10])
    assert (got["L"], got["P"], got["K"]) == (ref["L"], ref["P"], ref["K"])
    for name in TABLES:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], ref[name]), (name, np.flatnonzero(got[name] != ref[name])[:10])
    assert np.array_equal(got["strahler"], ref["strahler"])
    assert np.array_equal(got["link_magnitude"], ref["magnitude"].reshape(-1)[got["own_last"]])
    st = got["stats"]["fill"]
    print("fill rounds %d (bound %d), launched %d" % (st["rounds"], ref["bound"], st["launched"]))
    assert st["converged"] == 1 and st["rounds"] <= ref["bound"] and st["rounds"] < st["launched"] <= st["rounds"] + 4
    valid = int((ref["F"] != R.NONE).sum())
    assert int(got["acc"].reshape(-1)[got["root"].reshape(-1) == np.arange(z.size)].sum()) == valid == got["counts"]["valid"]
    assert got["stats"]["accumulate"]["converged"] == 1 and got["stats"]["streams"]["converged"] == 1
    return got, ref


def heights(rng, shape, top, hole=0.0):
    """integers 0 .. top in units of 1/256 m, a fraction `hole` of the cells without a value"""
    z = rng.integers(0, top + 1, shape).astype(np.float32) / 256
    z[rng.random(shape) < hole] = np.nan
    return z


# ---- the edges of the tiles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, T + 2), (T + 2, 1), (2, 2), (3, 3)])
def test_rasters_of_edge_cells_only(shape):
    got, ref = check_stage(heights(np.random.default_rng(1), shape, 50), min_cells=1)
    if shape != (3, 3):
        assert (got["dir"] == 0).all() and got["L"] == 0 and got["stats"]["fill"]["rounds"] == 0
        assert got["K"] == shape[0] * shape[1] and got["features"] == []


@pytest.mark.parametrize("H", [T, T + 1, 2 * T + 2])
@pytest.mark.parametrize("W", [T, T + 1, 2 * T + 2])
def test_shapes_at_the_tile_edges(H, W):
    rng = np.random.default_rng(H * 100 + W)
    got, ref = check_stage(heights(rng, (H, W), 3, 0.03), min_cells=6)
    assert got["L"] > 0 and got["counts"]["filled"] > 0


def test_all_equal_raster_routes_by_the_steps_and_the_tie_order():
    got, ref = check_stage(np.full((T + 9, 2 * T + 5), 7.25, np.float32), passes=1, min_cells=4)
    H, W = got["F"].shape
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ring = np.minimum(np.minimum(i, H - 1 - i), np.minimum(j, W - 1 - j))
    assert np.array_equal(got["F"] - got["r"], ring)                 # one unit per step from the border
    assert got["dir"][1, 1] == 16 and got["dir"][H // 2, 1] == 16 and got["dir"][1, W // 2] == 64       # W before N; orthogonal before diagonal


# ---- depressions --------------------------------------------------------------------------------------------------------------------
def test_pits():
    z = np.full((20, 21), 3.0, np.float32)
    z[9, 11] = 1.0
    got, _ = check_stage(z, min_cells=2)
    assert got["sinkdepth"][9, 11] > 2.0 and got["counts"]["filled"] == 18 * 19
    i, j = np.meshgrid(np.arange(2 * T + 3), np.arange(2 * T + 6), indexing="ij")
    z = (5.0 + 0.01 * j + 0.02 * i).astype(np.float32)
    z[T - 3:T + 3, T - 4:T + 4] = 2.0                                # a pit over the corner of four tiles
    z[T - 1:T + 1, T - 1:T + 1] = 1.5
    got, _ = check_stage(z, min_cells=30)
    assert got["F"][T, T] > got["r"][T, T] and got["L"] > 0


def test_nested_depressions():
    i, j = np.meshgrid(np.arange(T + 20), np.arange(2 * T + 10), indexing="ij")
    bowl = 0.002 * ((i - 25) ** 2 + (j - 37) ** 2)                   # the outer depression: its rim is the raster's edge
    z = 20.0 - 6.0 * np.exp(-bowl) + 0.03 * j
    for ci, cj, depth, size in ((20, 30, 3.0, 4), (30, 45, 2.0, 3), (25, 37, 4.0, 6), (24, 36, 1.0, 2), (40, 10, 1.0, 2)):
        z[ci - size:ci + size, cj - size:cj + size] -= depth         # pits inside it, one inside another
    for passes in (0, 1):
        got, _ = check_stage(z.astype(np.float32), z_ref=15.0, passes=passes, min_cells=25)
        assert got["counts"]["filled"] > 200


# ---- random heights: flats, ties and plain descent -------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 1, 2])
@pytest.mark.parametrize("hole", [0.0, 0.1, 0.3])
@pytest.mark.parametrize("top", [3, 50, 4000])
def test_random_heights(top, hole, passes):
    rng = np.random.default_rng(top * 1000 + int(hole * 100) + passes)
    check_stage(heights(rng, (T + 13, 2 * T + 7), top, hole), z_ref=0.0, passes=passes, min_cells=5)


def test_island_surrounded_by_no_data():
    i, j = np.meshgrid(np.arange(T + 12), np.arange(T + 16), indexing="ij")
    d2 = (i - 22) ** 2 + (j - 25) ** 2
    z = np.where(d2 < 18 ** 2, 30.0 - 0.05 * d2 + 0.5 * np.sin(i * 0.7) * np.cos(j * 0.9), np.nan).astype(np.float32)
    z[20:23, 24:27] -= 3.0
    got, _ = check_stage(z, z_ref=20.0, passes=1, min_cells=12)
    assert (got["dir"][0] == 255).all() and got["K"] > 0 and got["L"] > 0


def test_diagonal_ties_at_the_margin_of_2a2_and_b2():
    """2 a^2 against b^2 at the nearest integers on either side: (a, b) = (5, 7), (29, 41): 50 > 49, 1682 > 1681, the orthogonal
    neighbour wins; (12, 17), (70, 99): 288 < 289, 9800 < 9801, the diagonal one.  In every orientation."""
    for (a, b), code in (((5, 7), 1), ((29, 41), 1), ((12, 17), 2), ((70, 99), 2)):
        z = np.full((3, 3), 200.0, np.float32)
        z[1, 1], z[1, 2], z[2, 2] = 100.0, 100.0 - a, 100.0 - b
        z /= 256
        for k in range(4):
            for flip in (False, True):
                zz = np.rot90(z, k)
                zz = zz[:, ::-1] if flip else zz
                got, ref = check_stage(np.ascontiguousarray(zz))
                centre = int(got["dir"][1, 1])
                assert centre in ((1, 4, 16, 64) if code == 1 else (2, 8, 32, 128)), (a, b, k, flip, centre)
    got, _ = check_stage(np.ascontiguousarray(z))
    assert got["dir"][1, 1] == 2


# ---- the rounds of the fill -------------------------------------------------------------------------------------------------------------
def serpentine():
    """A flat channel between walls of 100 m that winds through 3 x 3 tiles and leaves at (1, 0): its fill is the distance along it."""
    H = W = 3 * T + 2
    z = np.full((H, W), 100.0, np.float32)
    lanes = list(range(1, H - 1, 4))
    for k, i in enumerate(lanes):
        z[i, 1:W - 1] = 0.0
        if k + 1 < len(lanes):
            j = W - 2 if k % 2 == 0 else 1
            z[i:lanes[k + 1] + 1, j] = 0.0
    z[1, 0] = 0.0
    return z


def test_serpentine_channel_rounds_and_cap():
    z = serpentine()
    got, ref = check_stage(z, min_cells=50)
    st = got["stats"]["fill"]
    assert ref["bound"] >= 60 and st["rounds"] > 20                  # many global rounds, within the header's bound (check_stage)
    assert got["F"][z == 0].max() < 65536 and got["L"] == 1          # the channel fills by its length, far below the walls
    import torch
    from ada_mvs_amd import hip_ops
    s, _ = hip_ops.contour_surface(torch.from_numpy(z).cuda(), 0.0, 0)
    # every second lane runs against the order in which the tiles start, so each of its three tile crossings costs a round whatever
    # the tiles of one round see of each other: 20 rounds are too few.  (The count itself may differ from run to run; F may not.)
    for cap in (1, 3, 20):
        _, F, capped, _ = hip_ops.drain_fill(s, 0, cap)
        assert capped["converged"] == 0 and capped["launched"] == cap and capped["rounds"] == cap
        assert not np.array_equal(F.cpu().numpy(), ref["F"])
    _, F, enough, _ = hip_ops.drain_fill(s, 0, ref["bound"] + 1)
    assert enough["converged"] == 1 and 20 < enough["rounds"] <= ref["bound"] and np.array_equal(F.cpu().numpy(), ref["F"])
    with pytest.raises(RuntimeError, match="max_rounds=3"):
        drainage.route(z, 1.0, min_area=50.0, smooth_passes=0, max_rounds=3)


# ---- links ----------------------------------------------------------------------------------------------------------------------------
def test_comb_of_tributaries():
    """A valley along row 40 that falls to the east across the tile borders; every column is a tributary from the north (39 cells) and
    from the south (8 cells: with min_cells = 8 a single stream cell, a source next to its junction)."""
    H, W = 50, 2 * T + 6
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = (50.0 + np.abs(i - 40) - 0.1 * j).astype(np.float32)
    got, ref = check_stage(z, z_ref=40.0, min_cells=8)
    trunk = got["link"][40, 1:W - 2]
    assert (got["nd"][40, 1] == 2) and (got["nd"][40, 2:W - 1] == 3).all() and (got["pos"][40, 1:W - 1] == 0).all()
    first, to, end, head = got["link_first"], got["link_to"], got["link_end"], got["link_head"]
    two = np.flatnonzero(first[1:] - first[:-1] == 2)
    south = [l for l in two.tolist() if head[l] // W == 41]
    assert len(south) == W - 2 and all(got["nd"].reshape(-1)[head[l]] == 0 and end[l] == head[l] - W for l in south)
    j5 = 40 * W + 5
    assert sorted(np.flatnonzero(end == j5).tolist()) == sorted([got["link"][39, 5], got["link"][41, 5], got["link"][40, 4]])
    assert (to[np.flatnonzero(end == j5)] == got["link"][40, 5]).all() and to[got["link"][40, W - 2]] == -1
    assert got["strahler"][trunk].tolist() == [2] * trunk.size and got["strahler"][got["link"][39, 7]] == 1
    assert got["link_magnitude"][got["link"][40, 1:W - 1]].tolist() == [2 * k for k in range(1, W - 1)]
    ids = {f["properties"]["id"]: f for f in got["features"]}
    f = ids[int(got["link"][39, 5]) + 1]
    assert f["properties"]["to_id"] == int(got["link"][40, 5]) + 1 and f["properties"]["upstream_cells"] == 39 and f["properties"]["vertices"] == 33


def test_min_cells_extremes():
    z = heights(np.random.default_rng(8), (T + 3, T + 5), 50, 0.1)
    got, ref = check_stage(z, min_cells=1)
    assert (got["nd"] != 255).sum() == got["counts"]["valid"] and ((got["link"] >= 0) | (got["dir"] == 0) | (got["dir"] == 255)).all()
    res = drainage.route(z, 1.0, min_area=float(z.size + 1), smooth_passes=0)
    assert res["L"] == 0 and res["P"] == 0 and res["K"] == 0 and res["features"] == [] and (res["nd"] == 255).all() and (res["basins"] == 0).all()
    assert res["link_first"].tolist() == [0] and (res["link"] == -1).all()
    assert drainage.geojson_text(res["features"]) == '{"type":"FeatureCollection","features":[]}\n'
    assert np.array_equal(res["acc"], ref["acc"])


def test_two_runs_are_byte_identical():
    z = heights(np.random.default_rng(21), (2 * T + 5, 2 * T + 9), 3, 0.1)
    a = drainage.route(z, 0.5, min_area=2.0)
    b = drainage.route(z, 0.5, min_area=2.0)
    for name, _ in RASTERS:
        assert a[name].tobytes() == b[name].tobytes(), name
    for name in TABLES:
        assert a[name].tobytes() == b[name].tobytes(), name
    assert drainage.geojson_text(a["features"]) == drainage.geojson_text(b["features"]) and a["L"] > 3


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def synthetic_dtm(H=90, W=120):
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = 103.0 + 4.0 * np.exp(-((i - 40) ** 2 + (j - 50) ** 2) / 300.0) + 0.02 * j - 2.5 * np.exp(-((i - 60) ** 2 + (j - 95) ** 2) / 60.0)
    z += 0.3 * np.sin(i * 0.35) * np.cos(j * 0.27)
    z = z.astype(np.float32)
    z[5:12, 100:110] = np.nan
    return z


def write_stage_inputs(prefix, z, grid):
    res = dict(dtm=z, ndsm=np.zeros_like(z), level=np.where(np.isfinite(z), 255, 0).astype(np.uint8), grid=grid, params={}, radius=[], dh=[],
               counts={}, fill={}, seconds={})
    dtm.write_outputs(prefix, res)
    with open(prefix + "_dsm.json", "w") as f:
        json.dump(dict(grid=dict(x0=grid.x0, y_top=grid.y_top, gsd=grid.gsd, W=grid.W, H=grid.H), z_ref=grid.z_ref), f)


def check_collection(fc, F, acc, grid, min_length=0.0):
    feats = {f["properties"]["id"]: f for f in fc["features"]}
    cell = lambda xy: int(round((grid.y_top - xy[1]) / grid.gsd - 0.5)) * grid.W + int(round((xy[0] - grid.x0) / grid.gsd - 0.5))
    for f in fc["features"]:
        p, xy = f["properties"], f["geometry"]["coordinates"]
        assert list(p) == list(drainage.PROPERTIES) and f["geometry"]["type"] == "LineString"
        assert p["vertices"] == len(xy) >= 2 and p["strahler"] >= 1 and p["magnitude"] >= 1 and p["basin"] >= 1
        cells = [cell(v) for v in xy]
        level = [int(F.reshape(-1)[c]) for c in cells]
        assert all(a > b for a, b in zip(level, level[1:]))            # downhill in F
        assert abs(p["drop_m"] - (level[0] - level[-1]) / 65536) < 1e-12 and p["upstream_area_m2"] == p["upstream_cells"] * grid.gsd ** 2
        length = sum(math.hypot(b[0] - a[0], b[1] - a[1]) for a, b in zip(xy, xy[1:]))
        assert abs(length - p["length_m"]) <= 1e-9 * max(1.0, length) and p["length_m"] >= min_length
        if p["to_id"]:
            if p["to_id"] in feats:
                assert feats[p["to_id"]]["geometry"]["coordinates"][0] == xy[-1]
            assert p["upstream_cells"] == acc.reshape(-1)[cells[-2]]
        else:
            assert p["upstream_cells"] == acc.reshape(-1)[cells[-1]] or p["upstream_cells"] == acc.reshape(-1)[cells[-2]]


def test_route_from_dsm_and_cli_end_to_end(tmp_path):
    z = synthetic_dtm()
    H, W = z.shape
    grid = dsm.Grid(5e5, 3.4e6, 0.5, 100.0, W, H)
    res = drainage.route(z, grid.gsd, grid.z_ref, min_area=10.0, grid=grid)
    ref = R.route(z, grid.z_ref, 1, 40, T)
    assert res["params"]["min_cells"] == 40
    for name in ("F", "dir", "acc", "basins", "link", "pos"):
        assert np.array_equal(res[name], ref[name]), name
    assert np.array_equal(res["vertex"], ref["vertex"]) and np.array_equal(res["link_to"], ref["link_to"]) and res["L"] == ref["L"] > 5
    assert res["counts"]["max_strahler"] >= 2 and np.array_equal(res["strahler"], ref["strahler"])
    P = str(tmp_path / "cli" / "dsm")
    write_stage_inputs(P, z, grid)
    paths = drainage.write_outputs(str(tmp_path / "direct"), res)
    via = drainage.from_dsm(P, min_area=10.0, out=str(tmp_path / "via" / "x"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "drainage_whu.py"), "--dsm", P, "--min_area", "10"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "total_time" in r.stdout
    assert sorted(os.listdir(os.path.dirname(P))) == sorted(os.path.basename(p) for p in
                                                            list(dtm.output_paths(P).values()) + [P + "_dsm.json"] + list(drainage.output_paths(P).values()))
    for key in ("geojson", "flowdir", "flowacc", "sinkdepth", "label"):
        with open(paths[key], "rb") as f, open(drainage.output_paths(P)[key], "rb") as g, open(drainage.output_paths(str(tmp_path / "via" / "x"))[key], "rb") as h:
            direct, cli, lib = f.read(), g.read(), h.read()
        assert direct == cli == lib, key                                 # three runs, byte-identical files
    assert via["source"] == dict(prefix=P, raster="dtm")
    basins, flowdir, flowacc, sinkdepth, fc, js = drainage.read_outputs(P)
    assert np.array_equal(basins, ref["basins"]) and np.array_equal(flowdir, ref["dir"]) and np.array_equal(flowacc, ref["acc"])
    assert np.array_equal(np.isnan(sinkdepth), ref["F"] == R.NONE)
    assert np.array_equal(sinkdepth[ref["F"] != R.NONE], ((ref["F"] - ref["r"]) / 65536).astype(np.float32)[ref["F"] != R.NONE])
    check_collection(fc, ref["F"], ref["acc"], grid)
    assert len(fc["features"]) == ref["L"] and js["counts"]["links"] == ref["L"] and js["params"]["min_cells"] == 40
    assert js["source"] == dict(prefix=P, raster="dtm") and js["stats"]["fill"]["converged"] == 1 and js["counts"]["basins"] == ref["K"]
    outlets = ref["root"].reshape(-1) == np.arange(z.size)
    assert int(flowacc.reshape(-1)[outlets].sum()) == int(np.isfinite(z).sum()) == js["counts"]["valid"]
    lengths = sorted(f["properties"]["length_m"] for f in fc["features"])
    cut = (lengths[len(lengths) // 2 - 1] + lengths[len(lengths) // 2]) / 2 if lengths[len(lengths) // 2 - 1] < lengths[len(lengths) // 2] else lengths[-1]
    out2 = str(tmp_path / "cli" / "long")
    drainage.main(["--dsm", P, "--min_area", "10", "--min_length", repr(cut), "--out", out2])          # the CLI's main, in this process
    fc2, js2 = drainage.read_outputs(out2)[4:]
    check_collection(fc2, ref["F"], ref["acc"], grid, cut)
    kept = [f for f in fc["features"] if f["properties"]["length_m"] >= cut]
    assert fc2["features"] == kept and 0 < len(kept) < len(fc["features"]) and js2["counts"]["rejected_short"] == len(fc["features"]) - len(kept)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_out_of_range_heights_raise():
    z = np.zeros((4, 5), np.float32)
    z[2, 3] = 9000.0
    with pytest.raises(ValueError, match="8191"):
        drainage.route(z, 1.0)
    with pytest.raises(ValueError, match="min_area"):
        drainage.route(z, 1.0, min_area=-2.0)


def test_argument_errors_return_before_any_launch():
    import torch
    lib = _lib.load()
    H, W = 6, 7
    n = H * W
    SENT = 77
    i32 = lambda *shape: torch.full(shape, SENT, device="cuda", dtype=torch.int32)
    u8 = lambda *shape: torch.full(shape, SENT, device="cuda", dtype=torch.uint8)
    s, r, F, acc, root, link, pos = (i32(H, W) for _ in range(7))
    d, nd = u8(H, W), u8(H, W)
    need = lib.adamvs_drain_workspace_bytes(W, H)
    ws = torch.zeros(need, device="cuda", dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = _lib.DrainStats()
    fill = lambda W_=W, H_=H, s_=p(s), ps=1, cap=8, w=p(ws), wb=need, r_=p(r), F_=p(F), st_=ctypes.byref(st): \
        lib.adamvs_drain_fill(W_, H_, s_, ps, cap, w, wb, r_, F_, st_, None)
    assert fill(s_=None) < 0 and fill(w=None) < 0 and fill(r_=None) < 0 and fill(F_=None) < 0 and fill(st_=None) < 0
    assert fill(W_=0) < 0 and fill(H_=-1) < 0 and fill(W_=1 << 15, H_=1 << 15) < 0 and fill(ps=-1) < 0 and fill(ps=3) < 0 and fill(cap=0) < 0
    assert fill(wb=need - 1) < 0 and fill(r_=p(s)) < 0 and fill(F_=p(r)) < 0 and fill(F_=ctypes.c_void_p(ws.data_ptr() + 256)) < 0
    direction = lambda W_=W, F_=p(F), d_=p(d): lib.adamvs_drain_direction(W_, H, F_, d_, None)
    assert direction(W_=0) < 0 and direction(F_=None) < 0 and direction(d_=None) < 0 and direction(d_=p(F)) < 0
    accum = lambda W_=W, d_=p(d), v=None, w=p(ws), wb=need, a=p(acc), ro=p(root), st_=ctypes.byref(st): \
        lib.adamvs_drain_accumulate(W_, H, d_, v, w, wb, a, ro, st_, None)
    assert accum(W_=-3) < 0 and accum(d_=None) < 0 and accum(w=None) < 0 and accum(a=None) < 0 and accum(ro=None) < 0 and accum(st_=None) < 0
    assert accum(wb=need - 1) < 0 and accum(ro=p(acc)) < 0 and accum(v=p(acc)) < 0
    streams = lambda W_=W, d_=p(d), a=p(acc), mc=3, w=p(ws), wb=need, nd_=p(nd), l=p(link), po=p(pos), st_=ctypes.byref(st): \
        lib.adamvs_drain_streams(W_, H, d_, a, mc, w, wb, nd_, l, po, st_, None)
    assert streams(W_=0) < 0 and streams(d_=None) < 0 and streams(a=None) < 0 and streams(mc=0) < 0 and streams(w=None) < 0
    assert streams(wb=need - 1) < 0 and streams(nd_=None) < 0 and streams(l=None) < 0 and streams(po=None) < 0 and streams(st_=None) < 0
    assert streams(po=p(link)) < 0 and streams(nd_=p(d)) < 0
    first, head, end, to, vertex = i32(3), i32(2), i32(2), i32(2), i32(5)
    links = lambda L=2, P=5, d_=p(d), w=p(ws), wb=need, f=p(first), h=p(head), v=p(vertex): \
        lib.adamvs_drain_links(W, H, d_, p(nd), p(link), p(pos), L, P, w, wb, f, h, p(end), p(to), v, None)
    assert links(L=-1) < 0 and links(L=n + 1, P=3 * n) < 0 and links(P=3) < 0 and links(L=0, P=1) < 0 and links(P=1 << 31) < 0
    assert links(d_=None) < 0 and links(w=None) < 0 and links(wb=need - 1) < 0 and links(f=None) < 0 and links(h=None) < 0 and links(v=None) < 0
    assert links(v=p(first)) < 0
    torch.cuda.synchronize()
    for t in (s, r, F, acc, root, link, pos, d, nd, first, head, end, to, vertex):
        assert bool((t == SENT).all())                                   # nothing was written: every call returned before a launch
    assert not bool(ws.any())
