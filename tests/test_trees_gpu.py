"""Tree detection on the GPU (csrc/dsm_trees.hip through hip_ops and ada_mvs_amd/trees.py) against the numpy restatement
(tests/trees_ref.py): mask, q, s, parents, roots, crown labels, every column of the table and the counts for exact equality at
every edge of the tiles, every window size and both sweep forms, plateaus and long chains, the inclusive thresholds, the crown
scene, run-to-run identity, argument errors and trees_whu.py end to end.  There is no tolerance and no cell is left out."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, buildings, dsm, dtm, fusion, fusion_synth, trees
from conftest import ROOT
from trees_ref import COLUMNS, CROWN_GSD, crown_scene, detect_ref, jump_rounds_ref, plateau, random_canopy, serpentine_ramp, stage_ref

pytestmark = pytest.mark.gpu

T = _lib.TREE_TILE
OFFSET = np.array([5e5, 3.4e6, 0.0])
THR = [0, 0, 0, 10 * 256, 20 * 256]                                     # the defaults at gsd 0.5 m without smoothing: 3, 4, 5 cells


def gpu_stage(nd, building, min_height, passes, thr, ratio_pm, rc2):
    """-> the dict of stage_ref through the five entry points."""
    import torch
    from ada_mvs_amd import hip_ops
    nn = torch.from_numpy(np.ascontiguousarray(nd, np.float32)).cuda()
    bb = None if building is None else torch.from_numpy(np.ascontiguousarray(building, np.int32)).cuda()
    mask, q, s, s_max = hip_ops.tree_surface(nn, bb, min_height, passes)
    parent, st = hip_ops.tree_parents(s, thr)
    root, number, n_tops, st = hip_ops.tree_roots(parent, stats=st)
    crowns, unassigned = hip_ops.tree_crowns(s, root, number, ratio_pm, rc2)
    tab = hip_ops.tree_table(crowns, q, s, root, n_tops).cpu().numpy()
    return dict(mask=mask.cpu().numpy(), q=q.cpu().numpy(), s=s.cpu().numpy(), s_max=int(s_max.item()), parent=parent.cpu().numpy(),
                root=root.cpu().numpy(), crowns=crowns.cpu().numpy(), T=n_tops, unassigned=int(unassigned.item()),
                table={n: tab[k] for k, n in enumerate(COLUMNS)}, stats=st)


def check_stage(nd, building=None, min_height=2.0, passes=0, thr=THR, ratio_pm=550, rc2=400):
    """The GPU result equals the restatement: every raster, T, the counts and every column of the table.  -> (got, ref)."""
    if callable(thr):
        thr = thr(stage_ref(nd, building, min_height, passes, [0], ratio_pm, rc2)["s_max"])
    ref = stage_ref(nd, building, min_height, passes, thr, ratio_pm, rc2)
    got = gpu_stage(nd, building, min_height, passes, thr, ratio_pm, rc2)
    for name, dtype in (("mask", np.uint8), ("q", np.int32), ("s", np.int32), ("parent", np.int32), ("root", np.int32), ("crowns", np.int32)):
        assert got[name].dtype == dtype and np.array_equal(got[name], ref[name]), (name, np.argwhere(got[name] != ref[name])[:10])
    assert (got["s_max"], got["T"], got["unassigned"]) == (ref["s_max"], ref["T"], ref["unassigned"])
    for name in COLUMNS:
        assert got["table"][name].dtype == np.int64 and np.array_equal(got["table"][name], ref["table"][name]), name
    st = got["stats"]
    assert st.converged == 1 and st.tops == ref["T"] and st.rounds == jump_rounds_ref(ref["parent"], _lib.TREE_JUMP_HOPS) < _lib.TREE_MAX_ROUNDS
    assert st.candidates >= ref["T"] and st.window_cells >= st.candidates
    return got, ref


def table_for(passes, gsd=0.5):
    return lambda s_max: trees.window_table(gsd, 1.5, 0.05, passes, s_max)


# ---- the smallest shapes ------------------------------------------------------------------------------------------------------
SMALL = [
    pytest.param(1, 1, 1.0, id="1x1-canopy"), pytest.param(1, 1, 0.0, id="1x1-empty"), pytest.param(T + 1, 1, 0.7, id="W1"),
    pytest.param(1, T + 1, 0.7, id="H1"), pytest.param(T + 6, T + 9, 1.0, id="all-canopy"), pytest.param(T + 6, T + 9, 0.0, id="no-canopy"),
]


@pytest.mark.parametrize("H,W,density", SMALL)
def test_small_shapes(H, W, density):
    nd = random_canopy(H, W, density, seed=H * 7 + W)
    got, ref = check_stage(nd, passes=1, thr=table_for(1))
    assert (got["T"] == 0) == (density == 0.0) and got["mask"].sum() == (H * W if density == 1.0 else got["mask"].sum())
    if density == 0.0:
        assert got["s_max"] == -1 and (got["parent"] == -1).all() and got["stats"].candidates == 0


# ---- every edge of a tile, at three canopy densities ----------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.3, 0.6, 0.9])
@pytest.mark.parametrize("edge", [-1, 0, 1, "2T+1"])
def test_random_heights_at_every_tile_edge(edge, density):
    w = 2 * T + 1 if edge == "2T+1" else T + edge
    h = 2 * T + 1 if edge == "2T+1" else T + edge
    for k, (H, W) in enumerate(((T + 7, w), (h, T + 7), (h, w))):
        nd = random_canopy(H, W, density, seed=1000 * k + 10 * w + int(density * 100), hi=30.0)
        got, _ = check_stage(nd, passes=1, thr=table_for(1))
        assert got["T"] > 0 and got["unassigned"] > 0


# ---- the windows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 5, 64])
def test_windows_at_exactly_r_and_r_plus_one(r):
    """Two pairs of equal peaks on a low canopy with holes.  Pair A, 10 m, exactly r cells apart along a row, its first peak
    within r of the grid's corner: the second is beaten by the first (equal height, larger index) and hangs on it.  Pair B, 12 m,
    r + 1 cells apart along a column, its first peak astride a tile corner: each is outside the other's window, both are tops.
    r = 5 adds a peak at the offset (3, 4), on the rim of the disc, and one at (4, 4), outside it.  At r = 1 and 5 every cell has
    the window r (the candidates that are no tops take the best cell of their window as parent); at r = 64 only cells of 9 m
    and more have it (a row of the bounding box no longer fits into a wave) and the low canopy has r = 1."""
    H, W = 2 * T + 8, 3 * T + 8
    rng = np.random.default_rng(r)
    nd = rng.uniform(2.0, 4.0, (H, W)).astype(np.float32)
    nd[rng.random((H, W)) < 0.1] = np.nan
    a1, a2, b1, b2 = (2, 3), (2, 3 + r), (T - 1, 2 * T), (T + r, 2 * T)
    nd[a1] = nd[a2] = 10.0
    nd[b1] = nd[b2] = 12.0
    extra = {}
    if r == 5:
        extra = dict(rim=(100 + 3, 20 + 4), out=(100 + 4, 40 + 4))
        nd[100, 20] = nd[extra["rim"]] = nd[100, 40] = nd[extra["out"]] = 11.0
    thr = [0] * r if r < 64 else [0] + [9 * 256] * 63
    got, ref = check_stage(nd, thr=thr, ratio_pm=0, rc2=10 ** 6)
    cell = lambda p: p[0] * W + p[1]
    par = got["parent"]
    assert par[a1] == cell(a1) and par[b1] == cell(b1) and par[b2] == cell(b2)
    assert par[a2] == cell(a1)
    if r == 5:
        assert par[100, 20] == cell((100, 20)) and par[extra["rim"]] == cell((100, 20))
        assert par[100, 40] == cell((100, 40)) and par[extra["out"]] == cell(extra["out"])
    assert int(ref["radius"].max()) == r and got["stats"].window_cells > got["stats"].candidates


def test_neighbouring_equal_peaks_at_r_one():
    """r = 1 is the 4-neighbourhood: of two equal peaks side by side the second hangs on the first; diagonal ones are both
    local maxima of their discs, but b(c) looks at all eight neighbours, so the second still hangs on the first."""
    nd = np.full((6, 9), 3.0, np.float32)
    nd[1, 1] = nd[1, 2] = nd[4, 5] = nd[3, 4] = 8.0
    got, _ = check_stage(nd, thr=[0], ratio_pm=0, rc2=10 ** 6)
    assert got["parent"][1, 2] == 1 * 9 + 1 and got["parent"][4, 5] == 3 * 9 + 4 and got["T"] == 2


# ---- plateaus and chains --------------------------------------------------------------------------------------------------------
def test_plateau_ties_go_to_the_smaller_index(capsys):
    H = W = 2 * T + 1
    got, _ = check_stage(plateau(H, W), thr=[0, 0, 0], rc2=10 ** 9)
    assert got["T"] == 1 and (got["root"] == 0).all() and (got["crowns"] == 1).all() and got["table"]["cells"].tolist() == [H * W]
    assert got["stats"].candidates == 1                                 # every other cell has a neighbour of a smaller index
    with capsys.disabled():
        print("\nplateau %d x %d: chains of %d cells, %d jump rounds" % (H, W, H - 1, got["stats"].rounds))


def test_serpentine_ramp_is_one_chain(capsys):
    H = W = 3 * T + 3
    nd = serpentine_ramp(H, W)
    got, ref = check_stage(nd, thr=[0], ratio_pm=0, rc2=10 ** 9)
    assert got["T"] == 1 and got["table"]["cells"].tolist() == [int((nd > 0).sum())]
    rounds = got["stats"].rounds
    assert rounds <= math.ceil(math.log2(W * H)) + 1 and rounds < _lib.TREE_MAX_ROUNDS
    assert jump_rounds_ref(ref["parent"], hops=2) >= math.floor(math.log2((nd > 0).sum() // 2))     # the chain is of the order of the cell count
    assert rounds >= math.floor(math.log((nd > 0).sum() // 2, _lib.TREE_JUMP_HOPS))
    with capsys.disabled():
        print("\nserpentine ramp %d x %d: one chain over %d cells, %d jump rounds (cap %d)" % (H, W, int((nd > 0).sum()), rounds, _lib.TREE_MAX_ROUNDS))


# ---- the surface ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 1, 2])
def test_smoothing_with_holes_and_buildings(passes):
    H, W = T + 30, 2 * T + 11
    rng = np.random.default_rng(40 + passes)
    nd = rng.uniform(0.0, 40.0, (H, W)).astype(np.float32)
    nd[rng.random((H, W)) < 0.04] = np.nan
    nd[rng.random((H, W)) < 0.03] = np.inf
    nd[rng.random((H, W)) < 0.03] = -np.inf
    nd[rng.random((H, W)) < 0.01] = 5000.0                              # clamped to 2047 m
    building = np.where(rng.random((H, W)) < 0.1, rng.integers(1, 9, (H, W)), 0).astype(np.int32)
    got, ref = check_stage(nd, building, passes=passes, thr=table_for(passes, gsd=2.0))
    assert got["s_max"] >= 2047 * 256 and not got["mask"][building > 0].any()
    free, _ = check_stage(nd, None, passes=passes, thr=table_for(passes, gsd=2.0))
    assert free["mask"].sum() > got["mask"].sum()


def test_the_thresholds_are_inclusive():
    below = np.nextafter(np.float32(2.0), np.float32(0))
    nd = np.array([[2.0, below, 3.0, np.nan, np.inf, 0.0, -1.0, 2.0]], np.float32)
    got, _ = check_stage(nd, thr=[0])
    assert got["mask"].tolist() == [[1, 0, 1, 0, 0, 0, 0, 1]]
    # the comparison is made in fp64: float32(0.1) is above 0.1 and float32(0.7) is below 0.7
    nd = np.array([[0.1, 0.7]], np.float32)
    assert float(nd[0, 0]) > 0.1 and float(nd[0, 1]) < 0.7
    assert gpu_stage(nd, None, 0.1, 0, [0], 550, 400)["mask"].tolist() == [[1, 1]]
    assert gpu_stage(nd, None, 0.7, 0, [0], 550, 400)["mask"].tolist() == [[0, 0]]
    # the ratio: 3 m is exactly half of 6 m, 767 / 256 m is one step below
    nd = np.array([[3.0, 6.0, 767.0 / 256.0]], np.float32)
    got, _ = check_stage(nd, thr=[0], ratio_pm=500, rc2=400)
    assert got["crowns"].tolist() == [[1, 1, 0]] and got["unassigned"] == 1
    # the radius: a ramp up to the top in column 5; 3^2 = 9 is inside rc2 = 9 and outside rc2 = 8
    nd = np.array([[5.0, 6.0, 7.0, 8.0, 9.0, 10.0]], np.float32)
    assert check_stage(nd, thr=[0], ratio_pm=0, rc2=9)[0]["crowns"].tolist() == [[0, 0, 1, 1, 1, 1]]
    assert check_stage(nd, thr=[0], ratio_pm=0, rc2=8)[0]["crowns"].tolist() == [[0, 0, 0, 1, 1, 1]]
    assert check_stage(nd, thr=[0], ratio_pm=1000, rc2=0)[0]["crowns"].tolist() == [[0, 0, 0, 0, 0, 1]]


@pytest.mark.parametrize("shape", [(70000, 2), (2, 70000)], ids=["70000x2", "2x70000"])
def test_more_rows_than_a_grid_dimension(shape):
    nd = random_canopy(shape[0], shape[1], 0.8, seed=9, hi=30.0)
    got, _ = check_stage(nd, passes=1, thr=table_for(1))
    assert got["T"] > 1000


# ---- the product ----------------------------------------------------------------------------------------------------------------
def same_result(got, ref):
    for name in ("mask", "q", "s", "parent", "root", "crowns", "label"):
        assert got[name].dtype == ref[name].dtype and np.array_equal(got[name], ref[name]), name
    for name in COLUMNS + ("q_top",):
        assert np.array_equal(got["table"][name], ref["table"][name]), name
    assert np.array_equal(got["keep"], ref["keep"]) and got["counts"] == ref["counts"] and got["thr"] == ref["thr"]
    assert got["params"] == ref["params"] and got["T"] == ref["T"] and got["s_max"] == ref["s_max"]
    assert got["properties"] == ref["properties"] and got["polygons"] == ref["polygons"]
    assert got["stats"]["rounds"] == ref["jump_rounds"] and got["stats"]["tops"] == ref["T"]


def test_crown_scene_with_the_defaults():
    nd, building, truth = crown_scene()
    got = trees.detect(nd, CROWN_GSD, building)
    same_result(got, detect_ref(nd, CROWN_GSD, building))
    assert got["table"]["top"].tolist() == truth["tops"] and [p["height_m"] for p in got["properties"]] == truth["heights"]
    assert not got["label"][building > 0].any() and got["counts"]["trees"] == len(truth["tops"])
    same_result(trees.detect(nd, CROWN_GSD, None, smooth_passes=2, min_crown_area=30.0), detect_ref(nd, CROWN_GSD, None, smooth_passes=2, min_crown_area=30.0))


def test_bit_identical_runs():
    rng = np.random.default_rng(31)
    nd = random_canopy(3 * T + 5, 4 * T + 3, 0.8, seed=31, hi=25.0)
    building = np.where(rng.random(nd.shape) < 0.05, 1, 0).astype(np.int32)
    kw = dict(min_crown_area=3.0, crown_ratio=0.3)
    a, b = trees.detect(nd, 1.0, building, **kw), trees.detect(nd, 1.0, building, **kw)
    same_result(a, detect_ref(nd, 1.0, building, **kw))
    assert a["counts"]["trees"] > 5 and a["counts"]["rejected_small"] > 0 and max(p["parts"] for p in a["properties"]) > 1
    for k in ("label", "crowns", "mask", "q", "s", "parent", "root"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for name in COLUMNS + ("q_top",):
        assert a["table"][name].tobytes() == b["table"][name].tobytes(), name
    assert a["counts"] == b["counts"] and a["stats"] == b["stats"]
    assert trees.points_geojson_text(a["properties"]).encode() == trees.points_geojson_text(b["properties"]).encode()
    ca, cb = (trees.crowns_geojson_text(r["polygons"], r["properties"]).encode() for r in (a, b))
    assert ca == cb and len(json.loads(ca)["features"]) == a["counts"]["trees"]


def test_argument_errors():
    import torch
    from ada_mvs_amd import hip_ops
    H, W, n = 20, 30, 600
    nd = torch.full((H, W), 5.0, device="cuda")
    bld = torch.zeros(H, W, device="cuda", dtype=torch.int32)
    for kw in (dict(min_height=0.0), dict(min_height=-1.0), dict(min_height=float("nan")), dict(min_height=float("inf")), dict(smooth_passes=-1),
               dict(smooth_passes=3)):
        args = dict(min_height=2.0, smooth_passes=1)
        args.update(kw)
        with pytest.raises(_lib.AdaMVSHipError, match="tree_surface"):
            hip_ops.tree_surface(nd, bld, **args)
    for a, b in ((nd.cpu(), bld), (nd.double(), bld), (nd, bld[:10]), (nd, bld.float()), (nd[0], None)):
        with pytest.raises(_lib.AdaMVSHipError):
            hip_ops.tree_surface(a, b, 2.0, 1)
    mask, q, s, s_max = hip_ops.tree_surface(nd, bld, 2.0, 1)
    for thr in ([], [1], [0, 5, 4], [0] * 65, [0, 2 ** 31]):
        with pytest.raises(_lib.AdaMVSHipError, match="tree_parents"):
            hip_ops.tree_parents(s, thr)
    with pytest.raises(_lib.AdaMVSHipError):
        hip_ops.tree_parents(nd, [0])
    with pytest.raises(_lib.AdaMVSHipError):
        hip_ops.tree_roots(nd)
    parent, st = hip_ops.tree_parents(s, [0] * 64)
    root, number, n_tops, st = hip_ops.tree_roots(parent, stats=st)
    assert n_tops == 1 and st.tops == 1 and st.converged == 1 and st.candidates == 1 and st.window_cells == n
    for kw in (dict(ratio_pm=-1), dict(ratio_pm=1001), dict(rc2=-1)):
        args = dict(ratio_pm=550, rc2=400)
        args.update(kw)
        with pytest.raises(_lib.AdaMVSHipError, match="tree_crowns"):
            hip_ops.tree_crowns(s, root, number, **args)
    label, unassigned = hip_ops.tree_crowns(s, root, number, 550, 400)
    for bad_T in (-1, n + 1):
        with pytest.raises((_lib.AdaMVSHipError, RuntimeError)):
            hip_ops.tree_table(label, q, s, root, bad_T)
    # through the C ABI: a short workspace, aliased buffers, null pointers; nothing is launched
    lib = _lib.load()
    need = lib.adamvs_tree_workspace_bytes(W, H)
    assert need == 256 + 2 * 2560
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    table = torch.empty(10, 1, device="cuda", dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    sf = lambda **kw: [kw.get("W", W), H, kw.get("ndsm", p(nd)), kw.get("building", p(bld)), 2.0, 1, kw.get("ws", p(ws)), kw.get("bytes", need),
                       kw.get("mask", p(mask)), kw.get("q", p(q)), kw.get("s", p(s)), kw.get("s_max", p(s_max)), None]
    assert lib.adamvs_tree_surface(*sf()) == 0 and lib.adamvs_tree_surface(*sf(building=None)) == 0
    for kw in (dict(bytes=need - 1), dict(q=p(s)), dict(s=p(nd)), dict(mask=p(ws)), dict(building=p(q)), dict(s_max=p(q)), dict(ndsm=None),
               dict(ws=None), dict(mask=None), dict(q=None), dict(s=None), dict(s_max=None), dict(W=0)):
        assert lib.adamvs_tree_surface(*sf(**kw)) < 0, kw
    st = _lib.TreeStats()
    thr1 = (ctypes.c_int * 2)(0, 7)
    pa = lambda **kw: [kw.get("W", W), H, kw.get("s", p(s)), kw.get("r_cap", 2), kw.get("thr", thr1), kw.get("ws", p(ws)), kw.get("bytes", need),
                       kw.get("parent", p(parent)), kw.get("stats", ctypes.byref(st)), None]
    assert lib.adamvs_tree_parents(*pa()) == 0 and st.candidates == 1
    for kw in (dict(bytes=need - 1), dict(parent=p(s)), dict(parent=p(ws)), dict(ws=p(s)), dict(s=None), dict(thr=None), dict(ws=None),
               dict(parent=None), dict(stats=None), dict(r_cap=0), dict(r_cap=65), dict(thr=(ctypes.c_int * 2)(1, 7)),
               dict(thr=(ctypes.c_int * 2)(0, -1)), dict(W=-1)):
        assert lib.adamvs_tree_parents(*pa(**kw)) < 0, kw
    ro = lambda **kw: [kw.get("W", W), H, kw.get("parent", p(parent)), kw.get("ws", p(ws)), kw.get("bytes", need), kw.get("root", p(root)),
                       kw.get("stats", ctypes.byref(st)), None]
    assert lib.adamvs_tree_roots(*ro()) == 0 and st.converged == 1 and st.tops == 1
    for kw in (dict(bytes=need - 1), dict(root=p(parent)), dict(root=p(ws)), dict(ws=p(parent)), dict(parent=None), dict(ws=None), dict(root=None),
               dict(stats=None), dict(W=0)):
        assert lib.adamvs_tree_roots(*ro(**kw)) < 0, kw
    cr = lambda **kw: [W, kw.get("H", H), kw.get("s", p(s)), kw.get("root", p(root)), kw.get("number", p(number)), kw.get("ratio_pm", 550),
                       kw.get("rc2", 400), kw.get("label", p(label)), kw.get("unassigned", p(unassigned)), None]
    assert lib.adamvs_tree_crowns(*cr()) == 0
    for kw in (dict(ratio_pm=-1), dict(ratio_pm=1001), dict(rc2=-1), dict(label=p(s)), dict(label=p(root)), dict(number=p(root)),
               dict(unassigned=p(label)), dict(s=None), dict(root=None), dict(number=None), dict(label=None), dict(unassigned=None), dict(H=0)):
        assert lib.adamvs_tree_crowns(*cr(**kw)) < 0, kw
    tb = lambda **kw: [W, kw.get("H", H), kw.get("label", p(label)), kw.get("q", p(q)), kw.get("s", p(s)), kw.get("root", p(root)), kw.get("T", 1),
                       kw.get("table", p(table)), None]
    assert lib.adamvs_tree_table(*tb()) == 0
    torch.cuda.synchronize()
    # a 5 m slab: one top at cell 0; the cells within 20 cells of it carry its label (rc2 = 400)
    i, j = np.mgrid[0:H, 0:W]
    inside = i * i + j * j <= 400
    assert table[:, 0].tolist() == [int(inside.sum()), int(inside.sum()) * 1280, 1280, 0, 19, 0, 20, 400, 0, 1280 * 16]
    assert int(unassigned.item()) == n - int(inside.sum())
    assert lib.adamvs_tree_table(*tb(T=0, table=None)) == 0
    for kw in (dict(T=-1), dict(T=n + 1), dict(table=None), dict(table=p(label)), dict(q=p(s)), dict(label=None), dict(q=None),
               dict(s=None), dict(root=None), dict(H=0)):
        assert lib.adamvs_tree_table(*tb(**kw)) < 0, kw
    torch.cuda.synchronize()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_trees_whu_end_to_end(tmp_path):
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
    listing = lambda: {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}
    params = dict(min_height=0.5, radius_min=0.8, radius_slope=0.1, crown_ratio=0.4, max_crown_radius=4.0, min_crown_area=0.5)
    flags = [v for k in params for v in ("--" + k, repr(params[k]))]
    r = run("trees_whu.py", "--dsm", P, *flags)                          # the labels are not there yet
    assert r.returncode != 0 and "buildings_whu.py" in r.stderr and "--no_buildings" in r.stderr
    bparams = dict(min_height=0.5, min_width=0.8, smooth_span=0.8, smooth_tol=0.3, min_smooth=0.25, min_area=2.0)
    r = run("buildings_whu.py", "--dsm", P, "--filled", *[v for k in bparams for v in ("--" + k, repr(bparams[k]))])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    before = listing()
    assert len(before) == len(dsm.output_paths(P)) + len(dsm.fill_output_paths(P)) + len(dtm.output_paths(P)) + len(buildings.output_paths(P))
    r = run("trees_whu.py", "--dsm", P, "--smooth_passes", "1", *flags)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "tops" in r.stdout and "trees" in r.stdout and "jump rounds" in r.stdout
    after = listing()
    paths = trees.output_paths(P)
    assert set(after) == set(before) | {os.path.basename(v) for v in paths.values()}
    for f in before:
        assert after[f] == before[f], f
    mine = trees.from_dsm(P, smooth_passes=1, **params)
    label, pts, crowns, js = trees.read_outputs(P)
    assert label.dtype == np.int32 and np.array_equal(label, mine["label"])
    assert after[os.path.basename(paths["points"])] == trees.points_geojson_text(mine["properties"]).encode()
    assert after[os.path.basename(paths["crowns"])] == trees.crowns_geojson_text(mine["polygons"], mine["properties"]).encode()
    assert len(pts["features"]) == len(crowns["features"]) == mine["counts"]["trees"] == int(label.max())
    g = mine["grid"]
    assert js["counts"] == mine["counts"] and js["grid"] == dict(x0=g.x0, y_top=g.y_top, gsd=g.gsd, W=g.W, H=g.H)
    assert js["params"] == dict(mine["params"], thr=mine["thr"]) and js["source"] == dict(prefix=P, buildings=True)
    assert js["jump_rounds"] == mine["stats"]["rounds"] and js["stats"] == mine["stats"]
    assert open(paths["label_world"]).read() == open(dsm.output_paths(P)["dsm_world"]).read()
    building = buildings.read_outputs(P)[0]
    assert not label[building > 0].any()
    # --no_buildings: nothing is excluded, written next to the first run under another prefix
    Q = str(tmp_path / "free" / "dsm")
    r = run("trees_whu.py", "--dsm", P, "--no_buildings", "--out", Q, *flags)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    free = trees.from_dsm(P, no_buildings=True, **params)
    assert np.array_equal(trees.read_outputs(Q)[0], free["label"]) and free["counts"]["canopy"] >= mine["counts"]["canopy"]
    assert trees.read_outputs(Q)[3]["source"] == dict(prefix=P, buildings=False) and listing() == after
    print("end to end: with the building labels %s, without %s" % (mine["counts"], free["counts"]))
