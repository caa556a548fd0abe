"""DSM gap fill on the GPU (csrc/dsm_fill.hip through dsm.fill_gaps) against the fp64 reference (tests/dsm_fill_ref.py): the
distance, the classes and the counts exactly; heights and colours to the bound the stopping rule gives; analytic harmonic
fields; run-to-run identity; the analytic scene far from the origin; the bench shape; dsm_whu.py --fill_max_dist end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import dsm, fusion, fusion_synth
from conftest import ROOT
from dsm_fill_ref import INT32_MAX, components, dist2_brute, dist2_separable, fill_ref, residual

pytestmark = pytest.mark.gpu

OFFSET = np.array([5e5, 3.4e6, 0.0])
TOL_H, TOL_C = 1e-6, 1e-3


def random_raster(H, W, seed, p_valid=0.5, blobs=0):
    """A smooth height field (+ boxes) with random empty cells and, optionally, empty discs; random colours."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:H, 0:W]
    z = 80.0 + 20.0 * np.sin(j / 17.0) * np.cos(i / 11.0) + np.where(((i // 23) + (j // 29)) % 3 == 0, 12.5, 0.0)
    valid = rng.random((H, W)) < p_valid
    for _ in range(blobs):
        ci, cj, rad = rng.integers(0, H), rng.integers(0, W), rng.uniform(2, 12)
        valid &= (i - ci) ** 2 + (j - cj) ** 2 > rad * rad
    d = np.where(valid, z, np.nan).astype(np.float32)
    rgba = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    rgba[..., 3] = 255
    rgba[~valid] = 0
    return d, rgba


def check_exact_parts(got, ref):
    assert np.array_equal(got["dist2"], ref["dist2"]), np.argwhere(got["dist2"] != ref["dist2"])[:10]
    assert np.array_equal(got["filled"], ref["filled"])
    for k in ("cells_valid", "cells_filled", "cells_empty"):
        assert got[k] == ref[k], k


def check_inputs_kept(got, d, rgba):
    valid = np.isfinite(d)
    assert got["dsm"][valid].tobytes() == d[valid].tobytes()
    assert np.array_equal(got["rgba"][valid], rgba[valid])
    empty = ~valid & (got["filled"] == 0)
    assert (got["dsm"][empty].view(np.uint32) == 0x7FC00000).all() and (got["rgba"][empty] == 0).all()
    f = got["filled"] == 1
    assert np.isfinite(got["dsm"][f]).all() and (got["rgba"][f][:, 3] == 255).all()


SHAPES = [
    pytest.param(1, 1, 0.0, 3.0, id="1x1-empty"), pytest.param(1, 1, 1.0, 3.0, id="1x1-valid"),
    pytest.param(37, 1, 0.3, 2.5, id="W1"), pytest.param(1, 53, 0.2, 4.0, id="H1"),
    pytest.param(23, 31, 0.0, 5.0, id="no-valid"), pytest.param(23, 31, 1.0, 5.0, id="all-valid"),
    pytest.param(40, 50, 0.4, 0.7, id="r-below-1"), pytest.param(41, 47, 0.05, 3.0, id="sparse"),
    pytest.param(64, 70, 0.3, 6.5, id="64x70"),
]


@pytest.mark.parametrize("H,W,p,r", SHAPES)
def test_small_shapes_against_the_brute_force_reference(H, W, p, r):
    d, rgba = random_raster(H, W, seed=H * 1000 + W, p_valid=p, blobs=2)
    ref = fill_ref(d, rgba, r, dist=dist2_brute(np.isfinite(d), r))
    assert np.array_equal(ref["dist2"], dist2_separable(np.isfinite(d), r))
    got = dsm.fill_gaps(d, rgba, r)
    check_exact_parts(got, ref)
    check_inputs_kept(got, d, rgba)
    f = ref["filled"] == 1
    assert np.abs(got["dsm"][f].astype(np.float64) - ref["u"][f]).max(initial=0) <= 1e-3
    assert np.abs(got["rgba"][f].astype(int) - ref["rgba"][f].astype(int)).max(initial=0) <= 1
    if ref["cells_filled"] == 0:
        assert got["cycles"] == 0 and got["dsm"].tobytes() == d.tobytes() and np.array_equal(got["rgba"], rgba)
    if p == 0.0:
        assert (got["dist2"] == INT32_MAX).all()


@pytest.mark.parametrize("r", [1.0, 2.5, 9.0, 31.7, 64.0])
def test_distance_on_a_large_grid(r):
    d, rgba = random_raster(700, 1000, seed=int(r * 10), p_valid=0.7, blobs=40)
    d[100:400, 200:260] = np.nan                     # a wide void: rows far from any valid cell
    rgba[100:400, 200:260] = 0
    valid = np.isfinite(d)
    want = dist2_separable(valid, r)
    got = dsm.fill_gaps(d, rgba, r)
    assert np.array_equal(got["dist2"], want), np.argwhere(got["dist2"] != want)[:10]
    assert np.array_equal(got["filled"], (~valid & (want.astype(np.float64) <= r * r)).astype(np.uint8))
    assert got["cells_valid"] == valid.sum() and got["cells_filled"] + got["cells_valid"] + got["cells_empty"] == d.size
    check_inputs_kept(got, d, rgba)


def test_radius_at_the_cap():
    H, W = 30, 2600                                   # wider than the cap on both sides of a cell
    d = np.full((H, W), np.nan, np.float32)
    rgba = np.zeros((H, W, 4), np.uint8)
    for i, j in ((3, 5), (20, 1300), (29, 2599)):
        d[i, j] = 10.0 + j * 1e-3
        rgba[i, j] = (10, 200, 30, 255)
    valid = np.isfinite(d)
    got = dsm.fill_gaps(d, rgba, 1024.0)
    want = dist2_separable(valid, 1024.0)
    assert np.array_equal(got["dist2"], want)
    assert got["cells_filled"] == int(((~valid) & (want != INT32_MAX)).sum())


def test_heights_and_colours_against_the_fp64_solution():
    """Error bound from the stopping rule: for a hole of radius rho the discrete Green's function is about rho^2 / 4, so a
    residual of at most tol_height leaves an error of about rho^2 / 4 * tol_height: 2.6e-4 m at rho = 32 (tol 1e-6)."""
    for seed, (H, W, r) in enumerate([(120, 160, 8.0), (200, 180, 32.0)]):
        d, rgba = random_raster(H, W, seed=seed, p_valid=0.85, blobs=25)
        d[50:90, 60:100] = np.nan
        rgba[50:90, 60:100] = 0
        ref = fill_ref(d, rgba, r)
        got = dsm.fill_gaps(d, rgba, r)
        check_exact_parts(got, ref)
        check_inputs_kept(got, d, rgba)
        assert got["residual_height"] <= TOL_H and got["residual_colour"] <= TOL_C
        f = ref["filled"] == 1
        assert f.sum() > 1000
        err = np.abs(got["dsm"][f].astype(np.float64) - ref["u"][f])
        assert err.max() <= 1e-3, err.max()
        assert np.abs(got["rgba"][f][:, :3].astype(int) - np.clip(np.rint(ref["c"][f]), 0, 255).astype(int)).max() <= 1


@pytest.mark.parametrize("field", ["linear", "i2-j2", "ij"])
def test_analytic_harmonic_fields(field):
    """Discrete-harmonic fields are reproduced in holes surrounded by V.  |u| <= 100 m, holes at most 20 cells across:
    rho^2 / 4 * tol = 1e-4 m at worst, plus fp32 rounding (6e-6 at 100 m)."""
    H, W = 150, 170
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    u = {"linear": 0.3 * i - 0.2 * j + 7.0, "i2-j2": (i * i - j * j) / 300.0, "ij": i * j / 260.0}[field]
    assert np.abs(u).max() <= 100.0
    d = u.astype(np.float32)
    rng = np.random.default_rng(3)
    holes = np.zeros((H, W), bool)
    for _ in range(30):
        ci, cj, rad = rng.integers(15, H - 15), rng.integers(15, W - 15), rng.uniform(1.5, 10.0)
        holes |= (i - ci) ** 2 + (j - cj) ** 2 <= rad * rad
    d[holes] = np.nan
    rgba = np.zeros((H, W, 4), np.uint8)
    rgba[~holes] = (40, 120, 250, 255)
    got = dsm.fill_gaps(d, rgba, 12.0)
    assert (got["filled"] == holes).all()
    assert np.abs(got["dsm"][holes].astype(np.float64) - u[holes]).max() <= 1e-4
    assert (got["rgba"][holes] == (40, 120, 250, 255)).all()


def test_bit_identical_runs():
    d, rgba = random_raster(300, 400, seed=11, p_valid=0.6, blobs=60)
    a = dsm.fill_gaps(d, rgba, 20.0)
    b = dsm.fill_gaps(d, rgba, 20.0)
    for k in ("dsm", "rgba", "filled", "dist2"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["cycles"], a["residual_height"], a["residual_colour"]) == (b["cycles"], b["residual_height"], b["residual_colour"])


def test_not_converging_raises_with_the_residuals():
    d, rgba = random_raster(200, 200, seed=12, p_valid=0.9, blobs=30)
    with pytest.raises(dsm.FillNotConverged, match=r"residual .* m .* colour"):
        dsm.fill_gaps(d, rgba, 16.0, tol_height=1e-12, max_cycles=1)


# ---- the analytic scene, fused on the GPU, far from the origin --------------------------------------------------------------
def scene_raster(offset, gsd=0.5):
    import torch
    H, W = 768, 1024
    sc = fusion_synth.scene(H, W, 4, offset=offset, seed=21)
    dev = torch.device("cuda")
    views = [dict(depth=torch.from_numpy(x).to(dev), K=c["K"], R=c["R"], C=c["C"]) for c, x in zip(sc["cams"], sc["depths"])]
    _, _, xyz, rgb = fusion.fuse_view(views[0], views[1:], torch.ones(H, W, device=dev), torch.from_numpy(sc["rgba"]).to(dev))
    grid = dsm.grid_for_bounds((offset[0] - 140.0, offset[1] - 100.0), (offset[0] + 140.0, offset[1] + 100.0), gsd, 0.0)
    b = dsm.DsmBuilder(grid, "max")
    b.add(xyz, rgb)
    return b.finish()


def test_scene_far_from_the_origin():
    runs = []
    for off in (np.zeros(3), OFFSET):
        res = scene_raster(off)
        runs.append(dsm.fill_gaps(res["dsm"], res["rgba"], 6.0))
    a, b = runs
    both = (a["filled"] == 1) & (b["filled"] == 1)
    assert both.sum() > 1000
    diff = np.abs(a["dsm"][both].astype(np.float64) - b["dsm"][both])
    assert (diff <= 1e-3).mean() >= 0.99, (diff <= 1e-3).mean()
    assert np.median(diff) <= 1e-4
    assert abs(int(a["filled"].sum()) - int(b["filled"].sum())) <= 0.01 * a["filled"].sum()


# ---- the bench shape: no direct solve, the maximum principle instead --------------------------------------------------------
def bench_shape_raster(seed=0):
    """2562 x 2751 cells: a smooth surface with buildings, an empty margin outside the footprint, speckle and disc holes of
    radius 4-60 (the shape tools/dsm_fill_bench.py fills)."""
    H, W = 2751, 2562
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:H, 0:W].astype(np.float32)
    z = 20.0 * np.sin(j / 300.0) * np.cos(i / 230.0) + np.where(((i // 150) + (j // 190)) % 4 == 0, 18.0, 0.0)
    valid = (i - H / 2) ** 2 / (0.47 * H) ** 2 + (j - W / 2) ** 2 / (0.47 * W) ** 2 <= 1.0
    valid &= rng.random((H, W)) > 0.03
    for _ in range(600):
        ci, cj, rad = rng.integers(0, H), rng.integers(0, W), rng.uniform(4, 60)
        y0, y1, x0, x1 = max(0, int(ci - rad)), min(H, int(ci + rad) + 1), max(0, int(cj - rad)), min(W, int(cj + rad) + 1)
        valid[y0:y1, x0:x1] &= (i[y0:y1, x0:x1] - ci) ** 2 + (j[y0:y1, x0:x1] - cj) ** 2 > rad * rad
    d = np.where(valid, z, np.nan).astype(np.float32)
    rgba = np.zeros((H, W, 4), np.uint8)
    rgba[valid] = np.stack([(z[valid] * 5) % 256, (i[valid] / 11) % 256, (j[valid] / 13) % 256, np.full(valid.sum(), 255)], -1).astype(np.uint8)
    return d, rgba


def test_bench_shape_residual_and_maximum_principle():
    d, rgba = bench_shape_raster()
    got = dsm.fill_gaps(d, rgba, 64.0)
    valid = np.isfinite(d)
    f = got["filled"] == 1
    assert got["cells_filled"] > 0.05 * valid.sum()
    assert got["residual_height"] <= TOL_H and got["residual_colour"] <= TOL_C
    check_inputs_kept(got, d, rgba)
    u = np.where(valid, d, np.where(f, got["dsm"], 0)).astype(np.float64)
    res = residual(u, valid, f)
    # the output is (float)u: its residual is the solver's plus fp32 rounding of up to 5 values near 40 m
    assert np.abs(res).max() <= TOL_H + 5 * 40.0 * 2.0 ** -24
    lab = components(f)
    lo = np.full(d.size, np.inf)
    hi = np.full(d.size, -np.inf)
    from dsm_fill_ref import shift
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        nv = shift(valid, dy, dx, False) & f
        vals = shift(d.astype(np.float64), dy, dx, np.nan)
        np.minimum.at(lo, lab[nv], vals[nv])
        np.maximum.at(hi, lab[nv], vals[nv])
    eps = 1e-4
    assert (got["dsm"][f] >= lo[lab[f]] - eps).all() and (got["dsm"][f] <= hi[lab[f]] + eps).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_dsm_whu_fill_end_to_end(tmp_path):
    sc = fusion_synth.scene(192, 256, 4, offset=OFFSET, seed=13)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    fusion_synth.write_predict_layout(sc, data, out)
    ply = fusion.fuse_folder(data, out, log=lambda *a: None)["ply"]
    cli, api, plain = str(tmp_path / "cli" / "dsm"), str(tmp_path / "api" / "dsm"), str(tmp_path / "plain" / "dsm")
    args = ["--ply", ply, "--gsd", "0.4", "--mode", "max", "--chunk", "40000", "--fill_max_dist", "3.0"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "dsm_whu.py")] + args + ["--out", cli], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "cells filled" in r.stdout and "V-cycles" in r.stdout
    mine = dsm.from_ply(ply, 0.4, "max", 1, chunk=40000, out=api, fill_max_dist=3.0)
    fp_cli, fp_api = dsm.fill_output_paths(cli), dsm.fill_output_paths(api)
    for k in list(dsm.output_paths(cli)):
        assert open(dsm.output_paths(cli)[k], "rb").read() == open(dsm.output_paths(api)[k], "rb").read(), k
    for k in fp_cli:
        if k != "json":
            assert open(fp_cli[k], "rb").read() == open(fp_api[k], "rb").read(), k
    a, b = json.load(open(fp_cli["json"])), json.load(open(fp_api["json"]))
    a.pop("seconds")
    b.pop("seconds")
    assert a == b and a["r_cells"] == 3.0 / 0.4 and a["cells_filled"] == mine["fill"]["cells_filled"] > 0
    fd, frgba, ffilled = dsm.read_fill_outputs(cli)
    assert fd.tobytes() == mine["fill"]["dsm"].tobytes() and np.array_equal(frgba, mine["fill"]["rgba"])
    assert np.array_equal(ffilled, mine["fill"]["filled"])
    # without the flag: the files of the plain run only
    r = subprocess.run([sys.executable, os.path.join(ROOT, "dsm_whu.py"), "--ply", ply, "--gsd", "0.4", "--chunk", "40000", "--out", plain],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "V-cycles" not in r.stdout
    assert not any(os.path.exists(p) for p in dsm.fill_output_paths(plain).values())
    for k, p in dsm.output_paths(plain).items():
        assert open(p, "rb").read() == open(dsm.output_paths(cli)[k], "rb").read(), k
