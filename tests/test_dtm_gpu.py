"""Ground filter on the GPU (csrc/dsm_dtm.hip through hip_ops and ada_mvs_amd/dtm.py) against the numpy restatement
(tests/dtm_ref.py): the opening value for value at every edge of the kernels, the filter's labels, opened raster and counts
exactly, the analytic scenes, degenerate inputs, run-to-run identity, argument errors and dtm_whu.py end to end."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, dsm, dtm, fusion, fusion_synth
from conftest import ROOT
from dtm_ref import NAN_BITS, WIDE_BOX, open_brute, open_sep, plane_scene, pmf, random_raster, same_opening

pytestmark = pytest.mark.gpu

TILE = _lib.DTM_TILE            # cells of a row per workgroup; the transposes work on 64 x 64 tiles
OFFSET = np.array([5e5, 3.4e6, 0.0])


def gpu_open(z, r):
    import torch
    from ada_mvs_amd import hip_ops
    return hip_ops.dsm_open(torch.from_numpy(np.ascontiguousarray(z, np.float32)).cuda(), r).cpu().numpy()


def gpu_classify(z, radius, dh):
    import torch
    from ada_mvs_amd import hip_ops
    level, opened, st = hip_ops.dtm_classify(torch.from_numpy(np.ascontiguousarray(z, np.float32)).cuda(), radius, dh)
    K = len(radius)
    counts = dict(valid=st.cells_valid, ground=st.cells_ground, object=st.cells_object, empty=st.cells_empty,
                  per_level=[st.cells_level[k] for k in range(1, K + 1)])
    assert st.levels == K and st.cells_level[0] == st.cells_ground and not any(st.cells_level[k] for k in range(K + 1, 17))
    return dict(level=level.cpu().numpy(), opened=opened.cpu().numpy(), counts=counts)


def check_classify(got, ref, z):
    assert np.array_equal(got["level"], ref["level"]), np.argwhere(got["level"] != ref["level"])[:10]
    assert same_opening(got["opened"], ref["opened"], z)
    assert got["counts"] == ref["counts"]


# ---- the opening against the literal 2-D window ---------------------------------------------------------------------------
SMALL = [
    pytest.param(1, 1, 1.0, id="1x1-valid"), pytest.param(1, 1, 0.0, id="1x1-empty"), pytest.param(37, 1, 0.6, id="W1"),
    pytest.param(1, 53, 0.6, id="H1"), pytest.param(23, 31, 0.0, id="no-valid"), pytest.param(23, 31, 1.0, id="all-valid"),
    pytest.param(41, 47, 0.05, id="sparse"),
]


@pytest.mark.parametrize("H,W,p", SMALL)
def test_opening_small_shapes_against_the_brute_force_window(H, W, p):
    z = random_raster(H, W, seed=H * 100 + W, p_valid=p)
    for r in (1, 3, 40, 1024):
        want = open_brute(z, r)
        assert same_opening(gpu_open(z, r), want, z), r


@pytest.mark.parametrize("r", [1, 2, 3, 5, 40, 100])
def test_opening_64x70_against_the_brute_force_window(r):
    z = random_raster(64, 70, seed=7, p_valid=0.7, blobs=2)
    z[5, 9], z[40, 41], z[63, 69] = np.inf, -np.inf, -0.0            # infinities are empty cells; a negative zero is a value
    got = gpu_open(z, r)
    assert same_opening(got, open_brute(z, r), z)
    v = np.isfinite(z)
    assert (got[v] <= z[v]).all()


# ---- the opening against the separable restatement: every edge of the kernels -----------------------------------------------
# One form serves every radius, so there is no switch-over radius.  The edges: r = 1; the window 2r + 1 either side of a power
# of two (the number of doubling steps changes at r = 2^k, the overlap of the two last windows is largest at r = 2^k - 1); the
# segment length TILE minus one and TILE itself (TILE + 1 exceeds the largest radius, 1024, so the cap takes its place: 1023
# and 1024); widths and heights of TILE - 1, TILE, TILE + 1 and of the transpose tile (63, 64, 65).
EDGE_RADII = sorted({1, 2, 3, 4, 7, 8, 63, 64, 65, 255, 256, 511, 512, 513, TILE - 1, TILE, 1023, 1024})


@pytest.mark.parametrize("shape", [(3, 2300), (2300, 3)], ids=["3x2300", "2300x3"])
def test_opening_at_every_radius_edge(shape):
    H, W = shape
    rng = np.random.default_rng(H)
    z = rng.normal(100.0, 30.0, (H, W)).astype(np.float32)
    z[rng.random((H, W)) < 0.3] = np.nan
    for r in EDGE_RADII:
        assert same_opening(gpu_open(z, r), open_sep(z, r), z), r


@pytest.mark.parametrize("n", [63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_opening_at_every_tile_edge(n):
    rng = np.random.default_rng(n)
    for H, W in ((5, n), (n, 5), (66, n)):
        z = rng.normal(0.0, 10.0, (H, W)).astype(np.float32)
        z[rng.random((H, W)) < 0.3] = np.nan
        for r in (2, 37, 600):
            assert same_opening(gpu_open(z, r), open_sep(z, r), z), (H, W, r)


@pytest.mark.parametrize("shape", [(70000, 2), (2, 70000)], ids=["70000x2", "2x70000"])
def test_opening_with_more_rows_than_a_grid_dimension(shape):
    """Past 65535 rows (of the raster, or of its transpose) a workgroup strides over several rows."""
    rng = np.random.default_rng(9)
    z = rng.normal(0.0, 10.0, shape).astype(np.float32)
    z[rng.random(shape) < 0.3] = np.nan
    assert same_opening(gpu_open(z, 5), open_sep(z, 5), z)
    radius, dh = dtm.schedule(1.0, max_radius=3.0)
    check_classify(gpu_classify(z, radius, dh), pmf(z, radius, dh), z)


@pytest.mark.parametrize("r", [16, 64])
def test_opening_with_empty_bands(r):
    """Whole rows and columns empty: windows that hold no valid cell at all (E is none there)."""
    z = random_raster(300, 500, seed=5, p_valid=0.9, blobs=10)
    z[100:181, :] = np.nan
    z[:, 200:261] = np.nan
    got = gpu_open(z, r)
    assert same_opening(got, open_sep(z, r), z)
    assert np.isfinite(got[np.isfinite(z)]).all()


# ---- the filter ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5, 32, 100])
@pytest.mark.parametrize("H,W", [(64, 70), (300, 500)])
def test_classify_equals_the_restatement(H, W, R):
    z = random_raster(H, W, seed=H + R, p_valid=0.8, blobs=12)
    radius, dh = dtm.schedule(1.0, max_radius=float(R))
    ref = pmf(z, radius, dh)
    assert ref["counts"]["ground"] > 0 and ref["counts"]["empty"] > 0 and (ref["counts"]["object"] > 0 or (H, R) == (64, 1))
    check_classify(gpu_classify(z, radius, dh), ref, z)


def test_classify_on_a_larger_raster():
    z = random_raster(700, 1000, seed=3, p_valid=0.85, blobs=40)
    z[100:400, 200:260] = np.nan
    radius, dh = dtm.schedule(1.0, max_radius=64.0)
    check_classify(gpu_classify(z, radius, dh), pmf(z, radius, dh), z)


def test_classify_threshold_is_strict():
    """Z - O == dh exactly keeps the cell as ground (3.5 - 2 = 1.5, all exact); one fp32 step above is flagged.  The difference
    is taken in fp64: 2^24 + 2 over 1 is 16777217 there, above a dh of 16777216.5 that an fp32 difference would round onto."""
    z = np.full((9, 40), 2.0, np.float32)
    z[4, 4] = 3.5
    z[4, 20] = np.nextafter(np.float32(3.5), np.float32(4))
    got = gpu_classify(z, [1], [1.5])
    assert got["level"][4, 4] == 0 and got["level"][4, 20] == 1 and got["counts"]["object"] == 1
    check_classify(got, pmf(z, [1], [1.5]), z)
    z = np.full((9, 9), 1.0, np.float32)
    z[4, 4] = 16777218.0
    for t, flagged in ((16777217.0, False), (16777216.5, True)):
        got = gpu_classify(z, [1], [t])
        assert (got["level"][4, 4] == 1) == flagged
        check_classify(got, pmf(z, [1], [t]), z)


# ---- the products on analytic scenes ------------------------------------------------------------------------------------------
def test_boxes_on_a_plane():
    z, plane, mask = plane_scene()
    res = dtm.ground_filter(z, 0.5)
    assert res["radius"].tolist() == [1, 2, 4, 8, 16, 32]
    assert np.array_equal(res["level"] != 0, mask)
    assert res["counts"]["object"] == mask.sum() and res["counts"]["ground"] == z.size - mask.sum() and res["counts"]["empty"] == 0
    # a plane is discrete-harmonic and the boxes are bounded by ground only: the exact solution under them is the plane
    bound = 1e-3 + np.spacing(np.abs(plane[mask]).astype(np.float32)).astype(np.float64)
    err = np.abs(res["dtm"][mask].astype(np.float64) - plane[mask])
    print("dtm - plane on the boxes: max %.3e m" % err.max())
    assert (err <= bound).all(), err.max()
    assert res["dtm"][~mask].tobytes() == z[~mask].tobytes()
    assert np.array_equal(res["ground"][~mask], z[~mask]) and np.isnan(res["ground"][mask]).all()
    height = np.rint(z.astype(np.float64) - plane)                     # 9 and 4 m on the boxes
    err = np.abs(res["ndsm"][mask].astype(np.float64) - height[mask])
    print("ndsm - box height on the boxes: max %.3e m" % err.max())
    assert (err <= bound).all(), err.max()
    assert set(np.round(res["ndsm"][mask]).tolist()) == {4.0, 9.0}
    assert (res["ndsm"][~mask] == 0).all()


def test_products_against_the_reference():
    """The whole chain on a raster with empty cells: labels exactly, the DTM's support exactly, its heights to the 1e-3 m the
    gap fill is held to (tests/test_dsm_fill_gpu.py), the nDSM exactly the stated difference of the DSM and the DTM."""
    from dtm_ref import dtm_ref
    z = random_raster(64, 70, seed=21, p_valid=0.8, blobs=6)
    ref = dtm_ref(z, 1.0, max_radius=5.0)
    got = dtm.ground_filter(z, 1.0, max_radius=5.0)
    assert ref["counts"]["object"] > 0 and np.array_equal(got["level"], ref["level"]) and got["counts"] == ref["counts"]
    assert got["fill"]["r_cells"] == ref["r_fill"] == 10.0
    assert got["ground"].tobytes() == ref["ground"].tobytes()
    fin = np.isfinite(ref["dtm"])
    assert np.array_equal(np.isfinite(got["dtm"]), fin) and (got["dtm"][~fin].view(np.uint32) == NAN_BITS).all()
    g = got["level"] == 0
    assert got["dtm"][g].tobytes() == z[g].tobytes()
    assert np.abs(got["dtm"][fin].astype(np.float64) - ref["dtm"][fin]).max() <= 1e-3
    both = np.isfinite(z) & fin
    assert np.array_equal(np.isfinite(got["ndsm"]), both)
    assert got["ndsm"][both].tobytes() == (z[both].astype(np.float64) - got["dtm"][both].astype(np.float64)).astype(np.float32).tobytes()
    assert (got["ndsm"][g] == 0).all()


def test_wide_box_is_kept_as_ground():
    z, _, mask = plane_scene(boxes=WIDE_BOX, gradients=(0.0, 0.0))
    res = dtm.ground_filter(z, 0.5)
    assert (res["level"] == 0).all() and res["counts"]["object"] == 0
    assert res["dtm"].tobytes() == z.tobytes() and (res["ndsm"] == 0).all()
    assert res["fill"]["cycles"] == 0 and res["fill"]["cells_filled"] == 0
    # on the sloping plane the dh_max cap takes part of the box's high side at the last level: exactly as the restatement
    z, _, mask = plane_scene(boxes=WIDE_BOX)
    radius, dh = dtm.schedule(0.5)
    check_classify(gpu_classify(z, radius, dh), pmf(z, radius, dh), z)


def test_degenerate_rasters():
    z = np.full((40, 50), np.nan, np.float32)
    res = dtm.ground_filter(z, 0.5)
    assert res["counts"] == dict(valid=0, ground=0, object=0, empty=2000, per_level=[0] * 6)
    assert (res["level"] == 255).all() and np.isnan(res["dtm"]).all() and np.isnan(res["ndsm"]).all()
    assert (res["opened"].view(np.uint32) == NAN_BITS).all()
    z = np.full((40, 50), 12.25, np.float32)
    res = dtm.ground_filter(z, 0.5)
    assert res["counts"] == dict(valid=2000, ground=2000, object=0, empty=0, per_level=[0] * 6)
    assert (res["level"] == 0).all() and res["fill"]["cycles"] == 0
    assert res["dtm"].tobytes() == z.tobytes() and res["opened"].tobytes() == z.tobytes() and (res["ndsm"] == 0).all()


def test_bit_identical_runs():
    z = random_raster(300, 500, seed=11, p_valid=0.8, blobs=30)
    a, b = dtm.ground_filter(z, 1.0, max_radius=20.0), dtm.ground_filter(z, 1.0, max_radius=20.0)
    assert a["counts"]["object"] > 0
    for k in ("level", "opened", "dtm"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["counts"] == b["counts"]


def test_argument_errors():
    import torch
    from ada_mvs_amd import hip_ops
    d = torch.zeros(20, 30, device="cuda")
    for r in (0, -1, 1025):
        with pytest.raises(_lib.AdaMVSHipError, match="dsm_open"):
            hip_ops.dsm_open(d, r)
    with pytest.raises(_lib.AdaMVSHipError):
        hip_ops.dsm_open(d.cpu(), 1)
    with pytest.raises(_lib.AdaMVSHipError):
        hip_ops.dsm_open(d[0], 1)
    bad = [([], []), ([1, 2], [0.5]), ([0], [0.5]), ([1025], [0.5]), ([2, 2], [0.5, 0.5]), ([4, 2], [0.5, 0.5]), ([1], [0.0]), ([1], [-1.0]),
           ([1], [float("nan")]), ([1], [float("inf")]), (list(range(1, 18)), [0.5] * 17)]
    for radius, dh in bad:
        with pytest.raises(_lib.AdaMVSHipError):
            hip_ops.dtm_classify(d, radius, dh)
    with pytest.raises(_lib.AdaMVSHipError):
        hip_ops.dtm_classify(d.double(), [1], [0.5])
    # through the C ABI: a short workspace, aliased buffers, null pointers; nothing is launched
    lib = _lib.load()
    need = lib.adamvs_dtm_workspace_bytes(30, 20)
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    out = torch.empty_like(d)
    level = torch.empty(20, 30, device="cuda", dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.adamvs_dsm_open(30, 20, p(d), 1, p(ws), need, p(out), None) == 0
    assert lib.adamvs_dsm_open(30, 20, p(d), 1, p(ws), need - 1, p(out), None) < 0
    assert lib.adamvs_dsm_open(30, 20, p(d), 1, p(ws), need, p(d), None) < 0
    assert lib.adamvs_dsm_open(30, 20, p(d), 1, p(d), need, p(out), None) < 0
    assert lib.adamvs_dsm_open(30, 20, None, 1, p(ws), need, p(out), None) < 0
    st = _lib.DtmStats()
    rad, dh = (ctypes.c_int * 1)(1), (ctypes.c_double * 1)(0.5)
    args = lambda **kw: [kw.get("W", 30), 20, kw.get("dsm", p(d)), 1, rad, dh, kw.get("ws", p(ws)), kw.get("bytes", need),
                         kw.get("level", p(level)), kw.get("opened", p(out)), ctypes.byref(st), None]
    assert lib.adamvs_dtm_classify(*args()) == 0 and st.cells_valid == 600 and st.cells_ground == 600
    for kw in (dict(bytes=need - 1), dict(opened=p(d)), dict(level=p(out)), dict(ws=p(out)), dict(dsm=None), dict(W=0)):
        assert lib.adamvs_dtm_classify(*args(**kw)) < 0, kw
    torch.cuda.synchronize()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_dtm_whu_end_to_end(tmp_path):
    sc = fusion_synth.scene(192, 256, 4, offset=OFFSET, seed=13)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    fusion_synth.write_predict_layout(sc, data, out)
    ply = fusion.fuse_folder(data, out, log=lambda *a: None)["ply"]
    P = str(tmp_path / "cli" / "dsm")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "dsm_whu.py"), "--ply", ply, "--gsd", "0.4", "--chunk", "40000", "--fill_max_dist", "3.0",
                        "--out", P], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    before = {f: open(os.path.join(os.path.dirname(P), f), "rb").read() for f in sorted(os.listdir(os.path.dirname(P)))}
    assert len(before) == len(dsm.output_paths(P)) + len(dsm.fill_output_paths(P))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "dtm_whu.py"), "--dsm", P, "--filled", "--max_radius", "6.1"], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ground" in r.stdout and "V-cycles" in r.stdout
    after = {f: open(os.path.join(os.path.dirname(P), f), "rb").read() for f in sorted(os.listdir(os.path.dirname(P)))}
    paths = dtm.output_paths(P)
    assert set(after) == set(before) | {os.path.basename(v) for v in paths.values()}
    for f in before:
        assert after[f] == before[f], f
    mine = dtm.from_dsm(P, filled=True, max_radius=6.1)
    assert mine["radius"].tolist() == [1, 2, 4, 8, 15] and mine["counts"]["valid"] > 0
    d, n, level = dtm.read_outputs(P)
    assert d.tobytes() == mine["dtm"].tobytes() and n.tobytes() == mine["ndsm"].tobytes() and np.array_equal(level, mine["level"])
    js = json.load(open(paths["json"]))
    assert js["counts"] == mine["counts"] and js["schedule"] == dict(radius=[1, 2, 4, 8, 15], dh=mine["dh"].tolist())
    assert js["params"] == dict(max_radius=6.1, slope=1.0, dh0=0.15, dh_max=2.5) and js["source"] == dict(prefix=P, filled=True)
    assert js["fill"]["r_cells"] == 2.0 * 6.1 / 0.4 and js["fill"]["cells_filled"] == mine["fill"]["cells_filled"]
    assert open(paths["dtm_world"]).read() == open(dsm.output_paths(P)["dsm_world"]).read()
