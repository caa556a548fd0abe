"""Building extraction on the GPU (csrc/dsm_buildings.hip through hip_ops and ada_mvs_amd/buildings.py) against the numpy
restatement (tests/buildings_ref.py): flags, component labels, every column of the table and the counts for exact equality at
every edge of the tiles and of the border rounds, the thresholds, the roof scene, run-to-run identity, argument errors and
buildings_whu.py end to end.  There is no tolerance and no cell is left out."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, buildings, dsm, dtm, fusion, fusion_synth
from buildings_ref import (COLUMNS, checkerboard_mask, comb_mask, components_ref, extract_ref, flags_ref, random_mask_raster, rasters_of_mask,
                           rings_mask, roof_scene, serpentine_mask, table_ref)
from conftest import ROOT
from dtm_ref import open_brute

pytestmark = pytest.mark.gpu

TW, TH = _lib.BLD_TILE_W, _lib.BLD_TILE_H
OFFSET = np.array([5e5, 3.4e6, 0.0])


def gpu_stage(d, nd, min_height=2.5, r_open=0, s=1, tol=1.0):
    """-> dict(flags, components, N, table, stats) through the three entry points."""
    import torch
    from ada_mvs_amd import hip_ops
    dd, nn = torch.from_numpy(np.ascontiguousarray(d, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(nd, np.float32)).cuda()
    flags = hip_ops.bld_flags(dd, nn, min_height, r_open, s, tol)
    comp, N, st = hip_ops.bld_label(flags)
    tab = hip_ops.bld_table(flags, nn, comp, N).cpu().numpy()
    assert st.converged == 1 and st.tiles == -(-d.shape[0] // TH) * -(-d.shape[1] // TW)
    return dict(flags=flags.cpu().numpy(), components=comp.cpu().numpy(), N=N, table={n: tab[k] for k, n in enumerate(COLUMNS)}, stats=st)


def check_stage(d, nd, min_height=2.5, r_open=0, s=1, tol=1.0, opening=None):
    """The GPU result equals the restatement: flags, labels, N and every column of the table.  -> (got, N)."""
    kw = {} if opening is None else dict(opening=opening)
    flags = flags_ref(d, nd, min_height, r_open, s, tol, **kw)
    comp, N = components_ref(flags >= 2)
    table = table_ref(comp, N, flags, nd)
    got = gpu_stage(d, nd, min_height, r_open, s, tol)
    assert got["flags"].dtype == np.uint8 and np.array_equal(got["flags"], flags), np.argwhere(got["flags"] != flags)[:10]
    assert got["N"] == N
    assert got["components"].dtype == np.int32 and np.array_equal(got["components"], comp), np.argwhere(got["components"] != comp)[:10]
    for name in COLUMNS:
        assert got["table"][name].dtype == np.int64 and np.array_equal(got["table"][name], table[name]), name
    assert 0 <= got["stats"].rounds < _lib.BLD_MAX_ROUNDS
    return got, N


# ---- the smallest shapes ----------------------------------------------------------------------------------------------------
SMALL = [
    pytest.param(1, 1, 1.0, id="1x1-foreground"), pytest.param(1, 1, 0.0, id="1x1-empty"), pytest.param(TH + 1, 1, 0.7, id="W1"),
    pytest.param(1, TW + 1, 0.7, id="H1"), pytest.param(TH + 6, TW + 9, 1.0, id="all-foreground"), pytest.param(TH + 6, TW + 9, 0.0, id="no-foreground"),
]


@pytest.mark.parametrize("H,W,density", SMALL)
def test_small_shapes(H, W, density):
    d, nd = random_mask_raster(H, W, density, seed=H * 7 + W)
    got, N = check_stage(d, nd)
    assert N == (0 if density == 0.0 else 1 if density == 1.0 else N)
    if density == 1.0:
        assert got["table"]["cells"].tolist() == [H * W] and (got["components"] == 1).all()


# ---- every edge of a tile, at three densities (0.59 is near the percolation threshold: long ragged components) ----------------
@pytest.mark.parametrize("density", [0.3, 0.59, 0.9])
@pytest.mark.parametrize("edge", [-1, 0, 1, "2T+1"])
def test_random_masks_at_every_tile_edge(edge, density):
    w = 2 * TW + 1 if edge == "2T+1" else TW + edge
    h = 2 * TH + 1 if edge == "2T+1" else TH + edge
    for k, (H, W) in enumerate(((TH + 7, w), (h, TW + 7), (h, w))):
        d, nd = random_mask_raster(H, W, density, seed=1000 * k + 10 * w + int(density * 100))
        _, N = check_stage(d, nd)
        assert N > 0


def test_checkerboard_every_cell_its_own_root():
    H, W = 2 * TH + 1, 2 * TW + 1
    d, nd = rasters_of_mask(checkerboard_mask(H, W), seed=3)
    got, N = check_stage(d, nd)
    assert N == (H * W + 1) // 2 and (got["table"]["cells"] == 1).all() and got["stats"].rounds == 0


@pytest.mark.parametrize("name", ["serpentine", "comb"])
def test_long_components_across_every_tile_border(name, capsys):
    """One component whose diameter is of the order of the cell count and which crosses every tile border many times."""
    H, W = 5 * TH + 3, 5 * TW + 3
    mask = serpentine_mask(H, W) if name == "serpentine" else comb_mask(H, W)
    d, nd = rasters_of_mask(mask, seed=5)
    got, N = check_stage(d, nd)
    assert N == 1 and got["table"]["cells"].tolist() == [int(mask.sum())]
    assert 0 < got["stats"].rounds < _lib.BLD_MAX_ROUNDS and got["stats"].pairs == 5 * H + 5 * W
    with capsys.disabled():
        print("\n%s %d x %d: %d border rounds over %d pairs (cap %d)" % (name, H, W, got["stats"].rounds, got["stats"].pairs, _lib.BLD_MAX_ROUNDS))


def test_rings_with_holes_around_other_components():
    H, W = TH + 21, 2 * TW + 5
    mask = rings_mask(H, W)
    d, nd = rasters_of_mask(mask, seed=6)
    got, N = check_stage(d, nd)
    assert N == (min(H, W) - 1) // 2 // 4 + 1                        # one ring per four cells of depth
    t = got["table"]
    assert (t["row_min"][0], t["row_max"][0], t["col_min"][0], t["col_max"][0]) == (0, H - 1, 0, W - 1)
    assert (t["row_min"][1], t["row_max"][1], t["col_min"][1], t["col_max"][1]) == (4, H - 5, 4, W - 5)


@pytest.mark.parametrize("shape", [(70000, 2), (2, 70000)], ids=["70000x2", "2x70000"])
def test_more_rows_than_a_grid_dimension(shape):
    d, nd = random_mask_raster(shape[0], shape[1], 0.59, seed=9)
    _, N = check_stage(d, nd)
    assert N > 1000


# ---- the flags ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 64])
def test_flags_on_a_raster_narrower_than_the_stride(s):
    """On 2s x 2s cells no cell has both neighbours of any direction inside the grid: all undetermined.  On (2s + 1)^2 the
    middle row has them along the row, the middle column along the column, and the centre alone in all four directions."""
    d, nd = rasters_of_mask(np.ones((2 * s, 2 * s), bool), seed=s)
    got, _ = check_stage(d, nd, s=s)
    assert (got["flags"] == 2).all() and got["table"]["undetermined"].tolist() == [4 * s * s]
    d, nd = rasters_of_mask(np.ones((2 * s + 1, 2 * s + 1), bool), seed=s)
    d[s, s] = np.float32(1e6)                                        # seen from the centre only: its neighbours lie s cells away
    got, _ = check_stage(d, nd, s=s)
    determined = np.zeros(d.shape, bool)
    determined[s, :] = determined[:, s] = True
    assert got["flags"][s, s] == 4 and np.array_equal(got["flags"] != 2, determined)


@pytest.mark.parametrize("s", [1, 3, 64])
def test_flags_with_empty_dsm_cells_next_to_candidates(s):
    H, W = 2 * TH + 9, 3 * TW - 5
    d, nd = random_mask_raster(H, W, 0.9, seed=20 + s)
    rng = np.random.default_rng(s)
    d[rng.random((H, W)) < 0.1] = np.nan
    d[rng.random((H, W)) < 0.02] = np.inf
    got, _ = check_stage(d, nd, s=s, tol=1.5)
    assert all((got["flags"] == v).any() for v in (0, 2, 3, 4))


@pytest.mark.parametrize("r_open", [0, 1, 3])
def test_the_opening(r_open):
    rng = np.random.default_rng(r_open)
    H, W = TH + 30, 2 * TW + 11
    i, j = np.mgrid[0:H, 0:W]
    mask = np.zeros((H, W), bool)
    for _ in range(40):
        h, w = rng.integers(1, 16, 2)
        i0, j0 = rng.integers(-3, H - 3), rng.integers(-3, W - 3)
        mask |= (i >= i0) & (i < i0 + h) & (j >= j0) & (j < j0 + w)
    d, nd = rasters_of_mask(mask, seed=7)
    got, N = check_stage(d, nd, r_open=r_open)
    assert N > 0 and ((got["flags"] == 1).any() == (r_open > 0))
    d, nd = d[:40, :50], nd[:40, :50]                                # and against the literal 2-D window
    check_stage(d, nd, r_open=r_open, opening=open_brute)


def test_the_height_threshold_is_inclusive():
    below = np.nextafter(np.float32(2.5), np.float32(0))
    nd = np.array([[2.5, below, 3.0, np.nan, np.inf, 0.0, -1.0, 2.5]], np.float32)
    d = np.full(nd.shape, 10.0, np.float32)
    got, N = check_stage(d, nd)
    assert got["flags"].tolist() == [[2, 0, 2, 0, 0, 0, 0, 2]] and N == 3
    # the comparison is made in fp64: float32(0.1) is above 0.1 and float32(0.7) is below 0.7
    nd = np.array([[0.1, 0.7]], np.float32)
    assert float(nd[0, 0]) > 0.1 and float(nd[0, 1]) < 0.7
    assert gpu_stage(d[:, :2], nd, min_height=0.1)["flags"].tolist() == [[2, 2]]
    assert gpu_stage(d[:, :2], nd, min_height=0.7)["flags"].tolist() == [[0, 0]]


def test_the_smoothness_threshold_is_inclusive():
    """(1 + 1) - 2 x 0.875 = 0.25 = smooth_tol is smooth; with the centre one fp32 step lower D exceeds it: rough."""
    nd = np.full((1, 7), 5.0, np.float32)
    d = np.ones((1, 7), np.float32)
    d[0, 1] = 0.875
    d[0, 5] = np.nextafter(np.float32(0.875), np.float32(0))
    got, _ = check_stage(d, nd, tol=0.25)
    f = got["flags"][0]
    assert f.tolist() == [2, 3, 3, 3, 3, 4, 2]
    assert got["table"]["smooth"].tolist() == [4] and got["table"]["rough"].tolist() == [1] and got["table"]["undetermined"].tolist() == [2]


# ---- the product --------------------------------------------------------------------------------------------------------------
def same_result(got, ref):
    assert np.array_equal(got["flags"], ref["flags"]) and np.array_equal(got["components"], ref["components"])
    assert got["label"].dtype == np.int32 and np.array_equal(got["label"], ref["label"])
    for name in COLUMNS:
        assert np.array_equal(got["table"][name], ref["table"][name]), name
    assert np.array_equal(got["keep"], ref["keep"]) and got["counts"] == ref["counts"]


def test_roof_scene_with_the_defaults():
    d, nd, truth = roof_scene()
    got = buildings.extract(d, nd, 0.5)
    same_result(got, extract_ref(d, nd, 0.5))
    assert (got["params"]["r_open"], got["params"]["stride"]) == (2, 2)
    c = got["counts"]
    assert c["buildings"] == len(truth["buildings"]) == 5 and c["rejected_rough"] == 3 and c["rejected_small"] == 3
    found = [(p["cells"], p["height_mean"], p["height_max"]) for p in got["properties"]]
    assert found == truth["buildings"]
    assert [p["area_m2"] for p in got["properties"]] == [b[0] * 0.25 for b in truth["buildings"]]
    assert not got["label"][truth["crowns"]].any() and not got["label"][truth["small"]].any()
    assert (got["flags"][truth["narrow"]] == 1).all()
    comp_of_crowns = np.unique(got["components"][truth["crowns"] & (got["flags"] >= 2)])
    rejected_rough = [k for k in comp_of_crowns.tolist() if got["table"]["cells"][k - 1] * 0.25 >= 10.0 and not got["keep"][k - 1]]
    assert len(rejected_rough) == 3 and all(got["table"]["rough"][k - 1] > got["table"]["smooth"][k - 1] for k in rejected_rough)
    assert [len(p["rings"]) for p in got["polygons"]] == [1] * 5 and [len(p["rings"][0]) for p in got["polygons"]] == [4] * 5


def test_bit_identical_runs():
    d, nd = random_mask_raster(3 * TH + 5, 4 * TW + 3, 0.62, seed=31)
    nd = (nd * (1.0 + np.random.default_rng(1).integers(0, 9, nd.shape) / 8.0)).astype(np.float32)
    kw = dict(min_width=0.0, smooth_tol=1.0, min_area=3.0, min_smooth=0.2)
    a, b = buildings.extract(d, nd, 1.0, **kw), buildings.extract(d, nd, 1.0, **kw)
    same_result(a, extract_ref(d, nd, 1.0, **kw))
    assert a["counts"]["buildings"] > 5 and a["counts"]["rejected_small"] > 0
    for k in ("label", "components", "flags"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for name in COLUMNS:
        assert a["table"][name].tobytes() == b["table"][name].tobytes(), name
    assert a["counts"] == b["counts"] and a["label_stats"] == b["label_stats"]
    ga, gb = (buildings.geojson_text(r["polygons"], r["properties"]).encode() for r in (a, b))
    assert ga == gb and len(json.loads(ga)["features"]) == a["counts"]["buildings"]


def test_argument_errors():
    import torch
    from ada_mvs_amd import hip_ops
    d = torch.zeros(20, 30, device="cuda")
    nd = torch.full((20, 30), 5.0, device="cuda")
    bad = [dict(min_height=0.0), dict(min_height=-1.0), dict(min_height=float("nan")), dict(min_height=float("inf")), dict(r_open=-1),
           dict(r_open=1025), dict(s=0), dict(s=65), dict(smooth_tol=-0.1), dict(smooth_tol=float("nan")), dict(smooth_tol=float("inf"))]
    for kw in bad:
        args = dict(min_height=2.5, r_open=1, s=1, smooth_tol=0.2)
        args.update(kw)
        with pytest.raises(_lib.AdaMVSHipError, match="bld_flags"):
            hip_ops.bld_flags(d, nd, **args)
    for a, b in ((d.cpu(), nd), (d, nd.double()), (d, nd[:10]), (d[0], nd[0])):
        with pytest.raises(_lib.AdaMVSHipError):
            hip_ops.bld_flags(a, b, 2.5, 1, 1, 0.2)
    with pytest.raises(_lib.AdaMVSHipError):
        hip_ops.bld_label(d)
    # through the C ABI: a short workspace, aliased buffers, null pointers; nothing is launched
    lib = _lib.load()
    need = lib.adamvs_bld_workspace_bytes(30, 20)
    assert need >= 256 + 2 * 2560 + lib.adamvs_dtm_workspace_bytes(30, 20)
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    flags = torch.empty(20, 30, device="cuda", dtype=torch.uint8)
    parent = torch.empty(20, 30, device="cuda", dtype=torch.int32)
    table = torch.empty(10, 1, device="cuda", dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    fl = lambda **kw: [kw.get("W", 30), 20, kw.get("dsm", p(d)), kw.get("ndsm", p(nd)), 2.5, 1, 1, 0.2, kw.get("ws", p(ws)),
                       kw.get("bytes", need), kw.get("flags", p(flags)), None]
    assert lib.adamvs_bld_flags(*fl()) == 0
    for kw in (dict(bytes=need - 1), dict(ndsm=p(d)), dict(flags=p(d)), dict(ws=p(nd)), dict(flags=p(ws)), dict(dsm=None), dict(ndsm=None),
               dict(ws=None), dict(flags=None), dict(W=0)):
        assert lib.adamvs_bld_flags(*fl(**kw)) < 0, kw
    st = _lib.BldStats()
    lb = lambda **kw: [kw.get("W", 30), 20, kw.get("flags", p(flags)), kw.get("ws", p(ws)), kw.get("bytes", need), kw.get("parent", p(parent)),
                       kw.get("stats", ctypes.byref(st)), None]
    assert lib.adamvs_bld_label(*lb()) == 0 and st.converged == 1 and st.tiles == 1 and st.pairs == 0 and st.rounds == 0
    for kw in (dict(bytes=need - 1), dict(parent=p(ws)), dict(ws=p(flags)), dict(flags=p(parent)), dict(flags=None), dict(ws=None),
               dict(parent=None), dict(stats=None), dict(W=-1)):
        assert lib.adamvs_bld_label(*lb(**kw)) < 0, kw
    label = torch.ones(20, 30, device="cuda", dtype=torch.int32)
    tb = lambda **kw: [30, kw.get("H", 20), kw.get("flags", p(flags)), kw.get("ndsm", p(nd)), kw.get("label", p(label)), kw.get("N", 1),
                       kw.get("table", p(table)), None]
    assert lib.adamvs_bld_table(*tb()) == 0
    torch.cuda.synchronize()
    # level ground under a 5 m slab: only the four corner cells have no counting direction at s = 1
    assert table[:, 0].tolist() == [600, 596, 0, 4, 0, 19, 0, 29, 600 * 5 * 1024, 0x40A00000]
    assert lib.adamvs_bld_table(*tb(N=0, table=None)) == 0
    for kw in (dict(N=-1), dict(N=601), dict(table=None), dict(table=p(label)), dict(label=p(nd)), dict(flags=None), dict(ndsm=None),
               dict(label=None), dict(H=0)):
        assert lib.adamvs_bld_table(*tb(**kw)) < 0, kw
    torch.cuda.synchronize()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_buildings_whu_end_to_end(tmp_path):
    sc = fusion_synth.scene(192, 256, 4, offset=OFFSET, seed=13)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    fusion_synth.write_predict_layout(sc, data, out)
    ply = fusion.fuse_folder(data, out, log=lambda *a: None)["ply"]
    P = str(tmp_path / "cli" / "dsm")
    run = lambda script, *args: subprocess.run([sys.executable, os.path.join(ROOT, script)] + list(args), capture_output=True, text=True,
                                               timeout=300, cwd=ROOT)
    r = run("dsm_whu.py", "--ply", ply, "--gsd", "0.4", "--chunk", "40000", "--fill_max_dist", "3.0", "--out", P)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = run("dtm_whu.py", "--dsm", P, "--filled", "--max_radius", "6.1")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    folder = os.path.dirname(P)
    before = {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}
    assert len(before) == len(dsm.output_paths(P)) + len(dsm.fill_output_paths(P)) + len(dtm.output_paths(P))
    params = dict(min_height=0.5, min_width=0.8, smooth_span=0.8, smooth_tol=0.3, min_smooth=0.25, min_area=2.0)
    r = run("buildings_whu.py", "--dsm", P, "--filled", *[v for k in params for v in ("--" + k, repr(params[k]))])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "components" in r.stdout and "buildings" in r.stdout
    after = {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}
    paths = buildings.output_paths(P)
    assert set(after) == set(before) | {os.path.basename(v) for v in paths.values()}
    for f in before:
        assert after[f] == before[f], f
    mine = buildings.from_dsm(P, filled=True, **params)
    label, gj, js = buildings.read_outputs(P)
    assert label.dtype == np.int32 and np.array_equal(label, mine["label"])
    assert after[os.path.basename(paths["geojson"])] == buildings.geojson_text(mine["polygons"], mine["properties"]).encode()
    assert len(gj["features"]) == mine["counts"]["buildings"] == int(label.max())
    g = mine["grid"]
    assert js["counts"] == mine["counts"] and js["grid"] == dict(x0=g.x0, y_top=g.y_top, gsd=g.gsd, W=g.W, H=g.H)
    assert js["params"] == dict(params, r_open=1, stride=2, simplify_tol=0.0) and js["source"] == dict(prefix=P, filled=True)
    assert js["label_stats"] == mine["label_stats"] and mine["counts"]["candidate"] > 0
    assert open(paths["label_world"]).read() == open(dsm.output_paths(P)["dsm_world"]).read()
    print("end to end: %s" % (mine["counts"],))
