"""DSM rasterisation on the GPU (csrc/dsm.hip through the C ABI) against the fp64 restatement (tests/dsm_ref.py), bit for bit;
the analytic scene fused through fusion.fuse_view; dsm_whu.py end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import dsm, fusion, fusion_synth
from conftest import ROOT
from dsm_ref import cells, restate

pytestmark = pytest.mark.gpu

OFFSET = np.array([5e5, 3.4e6, 0.0])


def run_kernel(grid, xyz, rgb, mode="max", min_count=1, chunks=None):
    """DsmBuilder over the points, split at the sizes `chunks` (default one chunk) -> finish()'s dict."""
    import torch
    b = dsm.DsmBuilder(grid, mode, "cuda")
    sizes = [len(xyz)] if chunks is None else list(chunks) + [len(xyz) - sum(chunks)]
    s = 0
    for n in sizes:
        b.add(torch.from_numpy(np.ascontiguousarray(xyz[s:s + n])).cuda(), torch.from_numpy(np.ascontiguousarray(rgb[s:s + n])).cuda())
        s += n
    assert s == len(xyz)
    return b.finish(min_count)


def assert_same(ker, ref):
    assert ker["dsm"].dtype == np.float32 and ker["dsm"].tobytes() == ref["dsm"].tobytes(), \
        np.argwhere(ker["dsm"].view(np.uint32) != ref["dsm"].view(np.uint32))[:10]
    assert np.array_equal(ker["count"], ref["count"])
    assert np.array_equal(ker["rgba"], ref["rgba"]), np.argwhere((ker["rgba"] != ref["rgba"]).any(-1))[:10]
    assert ker["points_used"] == int(ref["count32"].sum())


def random_points(grid, n, seed):
    """Points over and around the grid with fp32-height ties, duplicates in other colours, NaN / inf coordinates, points
    outside the grid and outside +-65536 m, in runs of neighbouring points as a view's pixels give them."""
    rng = np.random.default_rng(seed)
    w, h = grid.W * grid.gsd, grid.H * grid.gsd
    xyz = np.empty((n, 3))
    xyz[:, 0] = grid.x0 + rng.uniform(-0.1, 1.1, n) * w
    xyz[:, 1] = grid.y_top - rng.uniform(-0.1, 1.1, n) * h
    run = rng.random(n) < 0.6                        # most points continue near the previous one (same cell)
    for k in np.flatnonzero(run)[np.flatnonzero(run) > 0]:
        xyz[k, :2] = xyz[k - 1, :2] + rng.normal(0, 0.05 * grid.gsd, 2)
    xyz[:, 2] = grid.z_ref + rng.choice([12.25, 13.5, 40.0, 0.0, -3.75], n)       # exact fp32 ties
    xyz[:, 2] += np.where(rng.random(n) < 0.3, rng.uniform(-1e-7, 1e-7, n), rng.uniform(-30, 60, n) * (rng.random(n) < 0.3))
    dup = rng.choice(n, n // 10, replace=False)
    xyz[dup[1:]] = xyz[dup[:-1]]                      # duplicate points, other colours
    k = rng.choice(n, n // 50, replace=False)
    bad = np.array([np.nan, np.inf, -np.inf])
    xyz[k, rng.integers(0, 3, len(k))] = bad[rng.integers(0, 3, len(k))]
    k = rng.choice(n, n // 50, replace=False)
    xyz[k, 2] = grid.z_ref + rng.choice([65536.0, -65536.0, 65535.999, -65535.999, 7e4, -1e6, 65536.0 - 1e-9], len(k))
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    return xyz, rgb


GRIDS = [
    pytest.param(dsm.Grid(-13.5, 7.25, 0.25, -2.0, 37, 23), 20000, id="37x23"),
    pytest.param(dsm.Grid(512345.25, 3401434.25, 0.5, 812.0, 1, 17), 3000, id="W1-far"),
    pytest.param(dsm.Grid(-3.0, 4.0, 1.0, 0.0, 29, 1), 3000, id="H1"),
    pytest.param(dsm.Grid(0.0, 1.0, 1.0, 5.0, 1, 1), 2000, id="1x1"),
    pytest.param(dsm.Grid(100.0, 300.0, 0.1, 50.0, 1000, 700), 500000, id="1000x700"),
]


@pytest.mark.parametrize("mode", ["max", "mean"])
@pytest.mark.parametrize("grid,n", GRIDS)
def test_kernel_matches_restatement(grid, n, mode):
    xyz, rgb = random_points(grid, n, seed=n + grid.W)
    ref = restate(grid, xyz, rgb, mode)
    assert ref["used"].mean() > 0.3 and (~ref["used"]).sum() > 0
    ker = run_kernel(grid, xyz, rgb, mode)
    assert_same(ker, ref)
    assert ker["points_read"] == n and ker["cells_filled"] == int((ref["count32"] >= 1).sum())
    ker3 = run_kernel(grid, xyz, rgb, mode, min_count=3)
    assert_same(ker3, restate(grid, xyz, rgb, mode, min_count=3))


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_chunking_and_sequence_numbers(mode):
    grid = dsm.Grid(-13.5, 7.25, 0.25, -2.0, 37, 23)
    xyz, rgb = random_points(grid, 30000, seed=4)
    whole = run_kernel(grid, xyz, rgb, mode)
    assert_same(whole, restate(grid, xyz, rgb, mode))
    for chunks in ([0, 1, 17, 0, 1000, 1], [64, 63, 65, 1, 1, 12000], [29999]):
        part = run_kernel(grid, xyz, rgb, mode, chunks=chunks)
        for k in ("dsm", "count", "rgba"):
            assert part[k].tobytes() == whole[k].tobytes(), (chunks, k)


def test_mean_mode_is_independent_of_the_point_order():
    grid = dsm.Grid(-13.5, 7.25, 0.25, -2.0, 37, 23)
    xyz, rgb = random_points(grid, 30000, seed=5)
    a = run_kernel(grid, xyz, rgb, "mean")
    p = np.random.default_rng(6).permutation(len(xyz))
    b = run_kernel(grid, xyz[p], rgb[p], "mean", chunks=[777, 5000])
    assert a["dsm"].tobytes() == b["dsm"].tobytes() and np.array_equal(a["count"], b["count"])
    assert_same(b, restate(grid, xyz[p], rgb[p], "mean"))


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_a_million_points_in_one_cell(mode):
    """Every lane of every wave in one run: the combined atomics under full contention."""
    grid = dsm.Grid(0.0, 3.0, 1.0, 0.0, 3, 3)
    rng = np.random.default_rng(7)
    n = 1 << 20
    xyz = np.stack([rng.uniform(1.0, 2.0, n), rng.uniform(1.0, 2.0, n), rng.uniform(0.0, 100.0, n)], 1)
    xyz[rng.choice(n, 50, replace=False), 2] = 100.5               # a tie at the top: the first of them wins
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    ref = restate(grid, xyz, rgb, mode)
    ker = run_kernel(grid, xyz, rgb, mode)
    assert_same(ker, ref)
    assert ker["count"][1, 1] == 65535 and ker["points_used"] == n
    if mode == "max":
        assert ker["dsm"][1, 1] == 100.5


def view_points(H, W, seed, gsd_px=0.16):
    """Row-major pixels of a nadir view over a height field: the point order a fused view gives."""
    rng = np.random.default_rng(seed)
    j, i = np.mgrid[0:H, 0:W]
    x = (i + rng.uniform(-0.3, 0.3, (H, W))) * gsd_px
    y = -(j + rng.uniform(-0.3, 0.3, (H, W))) * gsd_px
    z = 20.0 * np.sin(x / 37.0) * np.cos(y / 23.0) + np.where((x % 60 < 25) & (y % 50 > -20), 18.0, 0.0)
    xyz = np.stack([x, y, z], -1).reshape(-1, 3)
    return xyz, rng.integers(0, 256, (H * W, 3)).astype(np.uint8)


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_ten_million_points_at_the_bench_shape(mode):
    xyz, rgb = view_points(2752, 3712, seed=8)
    assert len(xyz) > 1e7
    for gsd in (0.8, 4.0):
        grid = dsm.grid_for_bounds(xyz[:, :2].min(0), xyz[:, :2].max(0), gsd, np.floor(xyz[:, 2].min()))
        assert_same(run_kernel(grid, xyz, rgb, mode, chunks=[len(xyz) // 2]), restate(grid, xyz, rgb, mode))


# ---- the analytic scene, fused on the GPU ---------------------------------------------------------------------------------
def fused_points(offset=(0.0, 0.0, 0.0), H=768, W=1024):
    import torch
    sc = fusion_synth.scene(H, W, 4, offset=offset, seed=21)
    dev = torch.device("cuda")
    views = [dict(depth=torch.from_numpy(d).to(dev), K=c["K"], R=c["R"], C=c["C"]) for c, d in zip(sc["cams"], sc["depths"])]
    conf = torch.ones(H, W, device=dev)
    _, _, xyz, rgb = fusion.fuse_view(views[0], views[1:], conf, torch.from_numpy(sc["rgba"]).to(dev))
    return xyz, rgb


def cell_edges(grid):
    x0 = grid.x0 + np.arange(grid.W) * grid.gsd
    y1 = grid.y_top - np.arange(grid.H) * grid.gsd
    X0, Y1 = np.meshgrid(x0, y1)
    return X0, X0 + grid.gsd, Y1 - grid.gsd, Y1


def test_dsm_of_the_analytic_scene():
    import torch
    xyz, rgb = fused_points()
    lo, hi = torch.aminmax(xyz, dim=0)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    gsd = 0.5
    grid = dsm.grid_for_bounds(lo, hi, gsd, np.floor(lo[2]))
    b = dsm.DsmBuilder(grid, "max")
    b.add(xyz, rgb)
    res = b.finish()
    assert_same(res, restate(grid, xyz.cpu().numpy(), rgb.cpu().numpy(), "max"))
    d = res["dsm"]
    X0, X1, Y0, Y1 = cell_edges(grid)
    for bx0, bx1, by0, by1, top in fusion_synth.BOXES:
        inner = (X0 >= bx0 + gsd) & (X1 <= bx1 - gsd) & (Y0 >= by0 + gsd) & (Y1 <= by1 - gsd)
        assert inner.sum() > 1000
        ok = np.isfinite(d[inner]) & (np.abs(d[inner] - top) <= 0.05)
        assert ok.mean() >= 0.95, (top, ok.mean())
    # open terrain (2 m clear of every building): z = 0.  The fused depth averages bilinear taps of oblique sources, whose
    # interpolation error on the ground plane reaches ~0.1 m near the far edges of the view (0.12 m max, 3e-4 of the cells
    # beyond 0.05 m in the fp64 restatement of the fusion)
    open_ = np.ones_like(d, bool)
    for bx0, bx1, by0, by1, _ in fusion_synth.BOXES:
        open_ &= ~((X1 > bx0 - 2) & (X0 < bx1 + 2) & (Y1 > by0 - 2) & (Y0 < by1 + 2))
    f = open_ & np.isfinite(d)
    assert f.sum() > 0.95 * open_.sum()
    assert (np.abs(d[f]) <= 0.05).mean() >= 0.999 and np.abs(d[f]).max() <= 0.25


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_world_coordinates_far_from_the_origin(mode):
    """The scene shifted by (5e5, 3.4e6, 0) m and fused again: the grid shifts by exactly the offset, the heights agree."""
    gsd = 0.5
    runs = []
    for off in (np.zeros(3), OFFSET):
        xyz, rgb = fused_points(off)
        grid = dsm.grid_for_bounds((off[0] - 140.0, off[1] - 100.0), (off[0] + 140.0, off[1] + 100.0), gsd, 0.0)
        b = dsm.DsmBuilder(grid, mode)
        b.add(xyz, rgb)
        xyz_h = xyz.cpu().numpy()
        res = b.finish()
        assert_same(res, restate(grid, xyz_h, rgb.cpu().numpy(), mode))
        runs.append((grid, res, xyz_h - off))
    (ga, a, pa), (gb, b_, pb) = runs
    assert gb.x0 - ga.x0 == OFFSET[0] and gb.y_top - ga.y_top == OFFSET[1] and (ga.W, ga.H) == (gb.W, gb.H)
    # cells a point may leave between the runs (fused coordinates agree to ~1e-6 m, not bit for bit) are set aside: those
    # holding a point within 2e-3 m of a cell edge
    unstable = np.zeros(ga.W * ga.H, bool)
    for p in (pa, pb):
        u = (p[:, :2] - [ga.x0, ga.y_top]) / [gsd, -gsd]
        frac = u - np.floor(u)
        near = ((frac < 4e-3) | (frac > 1 - 4e-3)).any(1)
        used, cell, _ = cells(ga, p)
        unstable[cell[used & near]] = True
    both = np.isfinite(a["dsm"]) & np.isfinite(b_["dsm"]) & ~unstable.reshape(ga.H, ga.W)
    assert both.sum() > 0.8 * np.isfinite(a["dsm"]).sum()
    diff = np.abs(a["dsm"][both].astype(np.float64) - b_["dsm"][both])
    assert (diff <= 1e-3).mean() >= 0.998, (diff <= 1e-3).mean()    # the fusion keeps or drops ~1e-3 of the pixels differently
    assert np.median(diff) <= 1e-4


def test_bit_identical_runs():
    grid = dsm.Grid(-13.5, 7.25, 0.05, -2.0, 185, 115)
    xyz, rgb = random_points(grid, 400000, seed=9)
    for mode in ("max", "mean"):
        a = run_kernel(grid, xyz, rgb, mode)
        b = run_kernel(grid, xyz, rgb, mode)
        for k in ("dsm", "count", "rgba"):
            assert a[k].tobytes() == b[k].tobytes()


# ---- end to end: fuse_whu.py's PLY -> dsm_whu.py ---------------------------------------------------------------------------
def test_dsm_whu_end_to_end(tmp_path):
    sc = fusion_synth.scene(192, 256, 4, offset=OFFSET, seed=13)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    fusion_synth.write_predict_layout(sc, data, out)
    res = fusion.fuse_folder(data, out, log=lambda *a: None)
    ply = res["ply"]
    cli, api = str(tmp_path / "cli" / "dsm"), str(tmp_path / "api" / "dsm")
    args = ["--ply", ply, "--gsd", "0.75", "--out", cli, "--mode", "mean", "--min_count", "2", "--chunk", "40000"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "dsm_whu.py")] + args, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "total_time" in r.stdout
    mine = dsm.from_ply(ply, 0.75, "mean", 2, chunk=40000, out=api)
    for k, p in dsm.output_paths(cli).items():
        assert open(p, "rb").read() == open(dsm.output_paths(api)[k], "rb").read(), k
    import json
    meta = json.load(open(dsm.output_paths(cli)["json"]))
    assert meta["points_read"] == res["points"] and meta["points_used"] == res["points"] and meta["mode"] == "mean"
    assert meta["cells_filled"] == mine["cells_filled"] > 0
    d, c, rgba = dsm.read_outputs(cli)
    assert np.array_equal(np.isfinite(d), c >= 2) and np.array_equal(rgba[..., 3] == 255, c >= 2)
    # the whole stream in one chunk, and the raster against the restatement of the PLY's points
    pts = fusion.read_ply(ply)
    xyz = np.stack([pts["x"], pts["y"], pts["z"]], 1)
    rgb = np.stack([pts["red"], pts["green"], pts["blue"]], 1)
    ref = restate(mine["grid"], xyz, rgb, "mean", 2)
    assert d.tobytes() == ref["dsm"].tobytes() and np.array_equal(c, ref["count"]) and np.array_equal(rgba, ref["rgba"])
    # --bounds crops to the area asked for
    g = mine["grid"]
    bounds = (g.x0 + 30.0, g.y_top - 60.0, g.x0 + 60.0, g.y_top - 30.0)
    crop = dsm.from_ply(ply, 0.75, "max", 1, bounds=bounds)
    cg = crop["grid"]
    assert cg == dsm.grid_for_bounds(bounds[:2], bounds[2:], 0.75, g.z_ref) and (cg.W, cg.H) in ((41, 41), (41, 42), (42, 41), (42, 42))
    ref = restate(cg, xyz, rgb, "max")
    assert crop["dsm"].tobytes() == ref["dsm"].tobytes() and np.array_equal(crop["rgba"], ref["rgba"])
    assert crop["points_read"] == len(xyz) and 0 < crop["points_used"] < len(xyz)
