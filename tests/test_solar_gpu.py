"""The solar stage on the GPU (csrc/dsm_solar.hip through hip_ops and ada_mvs_amd/solar.py) against the host restatement
(tests/solar_ref.py): hz_n, hz_h, svf as fp64 bits, minutes, direct and the plane table for exact equality, at the wave edges of
the line grid and with directions whose step exceeds a side, for K = 8, 16 and 32, on equal heights, ties everywhere, holes, a
tower on a plane, a bowl and a concave ramp that outgrows the stack window; the exposure with a table that hits every sector with
rows at, just above and just below a cell's threshold; run-to-run identity, the refusals and solar_whu.py end to end.  There is
no tolerance and nothing is left out."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
import solar_ref as R
from ada_mvs_amd import _lib, solar
from conftest import ROOT

pytestmark = pytest.mark.gpu

WIN = _lib.SOLAR_STACK_WINDOW
GSD = 0.5
Q = (256.0 * GSD) ** 2
SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (3, 3)] + [(H, W) for H in (63, 64, 65) for W in (63, 64, 65)] + [(5, 131)]


def device_surface(s):
    import torch
    return torch.from_numpy(np.asarray(s, np.int64).astype(np.int32)).cuda()


def random_surface(rng, shape, top, holes=0.0):
    s = rng.integers(0, top + 1, shape).astype(np.int64)
    s[rng.random(shape) < holes] = R.NONE
    return s


def synthetic_table(K, hz_n, hz_h, rng):
    """Rows for every sector: where a cell of the sector has an occluder with (h / n) n == h in fp64, a row exactly at its
    threshold (lit: equality), one an ulp above (lit) and one an ulp below (shadow); a row that shadows every occluded cell, one that
    lights every cell, one with zero weights.  Sorted by sector."""
    rows = []
    az = R.azimuths(K)
    for k in range(K):
        thrs = [0.0, 1e9, 3.25]
        cells = np.argwhere(hz_h[k] > 0)
        for i, j in cells[:: max(1, len(cells) // 3)][:3]:
            n, h = int(hz_n[k, i, j]), int(hz_h[k, i, j])
            t = float(h) / n
            if t * n == float(h):
                thrs += [t, np.nextafter(t, np.inf), np.nextafter(t, 0.0)]
        for t in thrs:
            el = float(rng.uniform(0.05, 1.5))
            v = (math.sin(az[k]) * math.cos(el), math.cos(az[k]) * math.cos(el), math.sin(el))
            rows.append((k, float(t), int(rng.integers(0, 50)), int(rng.integers(0, 2 ** 20)), [round(32768 * c) for c in v]))
        rows.append((k, 1.5, 0, 0, [0, 0, 32768]))
    return dict(sector=np.array([r[0] for r in rows]), thr=np.array([r[1] for r in rows]), minutes=np.array([r[2] for r in rows]),
                energy=np.array([r[3] for r in rows]), sun=np.array([r[4] for r in rows]))


def labels_for(shape, rng):
    """Label 1 fills the upper half (a run across many waves and rows), 2 and 3 are scattered, 0 elsewhere; plane 2 faces north and
    steeply away from a southern sun, plane 3 is level."""
    H, W = shape
    lab = np.where(rng.random(shape) < 0.3, rng.integers(2, 4, shape), 0).astype(np.int32)
    lab[: max(1, H // 2)] = 1
    normal = solar.quantise_normals([[0.0, -0.6, 0.8], [0.0, 0.8, 0.6], [0.0, 0.0, 1.0]])
    return lab, normal


def check_stage(s, K, rng, spills=None):
    """Every output word of the four kernels equals the restatement.  -> (hz_n, hz_h, stats)"""
    import torch
    from ada_mvs_amd import hip_ops
    s = np.asarray(s, np.int64)
    sd = device_surface(s)
    rn, rh = R.horizon_brute(s, K)
    hz_n, hz_h, st, ws = hip_ops.solar_horizon(sd, K)
    gn, gh = hz_n.cpu().numpy(), hz_h.cpu().numpy()
    assert gn.dtype == np.int32 and gn.shape == (K,) + s.shape
    assert np.array_equal(gn, rn), ("hz_n", np.argwhere(gn != rn)[:10])
    assert np.array_equal(gh, rh), ("hz_h", np.argwhere(gh != rh)[:10])
    assert st["lines"] == sum(R.line_count(s.shape[0], s.shape[1], di, dj) for di, dj in R.directions(K))
    if spills is not None:
        hn, hh, ref_st = R.horizon_hull(s, K)
        assert np.array_equal(hn, rn) and np.array_equal(hh, rh)
        print("stats", st, "restated", ref_st)
        assert (st["deepest"], st["spills"]) == (ref_st["deepest"], ref_st["spills"])
        assert (st["spills"] > 0) == spills
    w = solar.direction_weights(K)
    svf = hip_ops.solar_svf(sd, hz_n, hz_h, w, Q).cpu().numpy()
    ref_svf = R.svf(s, rn, rh, w, Q)
    assert svf.dtype == np.float64 and np.array_equal(svf.view(np.int64), ref_svf.view(np.int64)), np.argwhere(svf != ref_svf)[:10]
    table = synthetic_table(K, rn, rh, rng)
    lab, normal = labels_for(s.shape, rng)
    for with_labels in (False, True):
        ld = torch.from_numpy(lab).cuda() if with_labels else None
        nd = torch.from_numpy(normal.astype(np.int32)).cuda() if with_labels else None
        minutes, direct, ws = hip_ops.solar_expose(sd, hz_n, hz_h, table, ld, nd, ws)
        rm, rd = R.expose(s, rn, rh, table, lab if with_labels else None, normal if with_labels else None)
        assert minutes.dtype == torch.int32 and np.array_equal(minutes.cpu().numpy(), rm), "minutes"
        assert np.array_equal(direct.cpu().numpy(), rd), ("direct", with_labels)
        P = 3 if with_labels else 0
        sums = hip_ops.solar_plane_sums(sd, minutes, direct, ld, P).cpu().numpy()
        assert sums.dtype == np.int64 and np.array_equal(sums, R.plane_sums(s, rm, rd, lab if with_labels else None, P)), sums
        assert sums[0].sum() == (s != R.NONE).sum()
    return gn, gh, st


# ---- the shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 16, 32])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_word_at_the_wave_edges_of_the_line_grid(shape, K):
    """Equal heights (every horizon 0, svf exactly 1), heights 0 .. 1 (ties everywhere), 0 .. 50 with 30 % holes."""
    rng = np.random.default_rng(7 * K + shape[0] * 131 + shape[1])
    n, h, _ = check_stage(np.full(shape, 5, np.int64), K, rng, spills=False if K == 8 or shape[0] * shape[1] < 400 else None)
    assert (n == 0).all() and (h == 0).all()
    check_stage(random_surface(rng, shape, 1), K, rng)
    check_stage(random_surface(rng, shape, 50, 0.3), K, rng)
    if K == 16:
        steps = random_surface(rng, shape, 3, 0.1)                  # whole metres about a negative height, holes kept
        check_stage(np.where(steps == R.NONE, R.NONE, steps * 256 - 300), K, rng)


def test_equal_heights_have_an_open_sky():
    import torch
    from ada_mvs_amd import hip_ops
    s = np.full((64, 65), -7, np.int64)
    s[3, 4] = R.NONE
    sd = device_surface(s)
    for K in (8, 16, 32):
        hz_n, hz_h, st, _ = hip_ops.solar_horizon(sd, K)
        assert int(hz_n.abs().max()) == 0 and int(hz_h.abs().max()) == 0 and st["spills"] == 0 and st["deepest"] == 2
        svf = hip_ops.solar_svf(sd, hz_n, hz_h, solar.direction_weights(K), Q).cpu().numpy()
        assert svf[3, 4] == 0.0 and (np.delete(svf.reshape(-1), 3 * 65 + 4) == 1.0).all()
    assert torch.cuda.is_available()


@pytest.mark.parametrize("K", [8, 16, 32])
def test_one_tower_on_a_plane(K):
    """Every cell on a ray through the tower sees it at its distance with its height; the shadow of a one-row table has the closed-form
    length: with h = 10 units and 2.5 units per step the cells 1, 2 and 3 steps north of the tower are in shadow, the fourth
    (10 > 2.5 * 4 fails: equality) is lit."""
    from ada_mvs_amd import hip_ops
    H = W = 33
    s = np.zeros((H, W), np.int64)
    s[16, 16] = 10
    n, h, st = check_stage(s, K, np.random.default_rng(K), spills=False)
    for k, (di, dj) in enumerate(R.directions(K)):
        expect = np.zeros((H, W), np.int64)
        t = 1
        while 0 <= 16 - t * di < H and 0 <= 16 - t * dj < W:
            expect[16 - t * di, 16 - t * dj] = t
            t += 1
        assert np.array_equal(n[k], expect) and np.array_equal(h[k], np.where(expect > 0, 10, 0)), k
    sd = device_surface(s)
    hz_n, hz_h, _, ws = hip_ops.solar_horizon(sd, K)
    south = K // 2
    assert R.directions(K)[south] == (1, 0)
    one = dict(sector=[south], thr=[2.5], minutes=[1], energy=[16], sun=[[0, -23170, 23170]])
    lit = hip_ops.solar_expose(sd, hz_n, hz_h, one)[0].cpu().numpy()
    expect = np.ones((H, W), np.int64)
    expect[13:16, 16] = 0
    assert np.array_equal(lit, expect)


def test_a_bowl_and_a_concave_ramp_outgrow_the_stack_window():
    """Side 2 WINDOW + 3.  On the concave ramp every cell stays on the hull: the stack passes the window and entries spill; with a
    tower behind it they all come back, popped one by one.  The convex bowl pops down to two entries at every cell, a plane's
    collinear cells replace one another: neither spills."""
    side = 2 * WIN + 3
    x = np.arange(side, dtype=np.int64)
    rng = np.random.default_rng(3)
    ramp = -(x[:, None] ** 2) - x[None, :] ** 2
    for K in (8, 32):
        _, _, st = check_stage(ramp + 5000, K, rng, spills=True)
        assert st["deepest"] == side
    tower = ramp + 5000
    tower[side - 1, side - 1] = 6000
    tower[0, side // 2] = 7000
    check_stage(tower, 16, rng, spills=True)
    bowl = (x[:, None] - side // 2) ** 2 + (x[None, :] - side // 2) ** 2
    check_stage(bowl, 16, rng, spills=False)
    plane = 3 * x[:, None] + 2 * x[None, :]
    _, _, st = check_stage(plane, 32, rng, spills=False)
    assert st["spills"] == 0 and st["deepest"] == 2
    check_stage(np.minimum(ramp + 5000, 4000) + random_surface(rng, ramp.shape, 1), 8, rng, spills=True)


def test_a_plane_facing_away_contributes_nothing():
    import torch
    from ada_mvs_amd import hip_ops
    s = np.zeros((4, 70), np.int64)
    sd = device_surface(s)
    hz_n, hz_h, _, _ = hip_ops.solar_horizon(sd, 8)
    lab = np.zeros((4, 70), np.int32)
    lab[1], lab[2] = 1, 2
    normal = solar.quantise_normals([[0.0, 0.8, 0.6], [0.0, -0.8, 0.6]])             # facing north, facing south
    table = dict(sector=[4], thr=[100.0], minutes=[30], energy=[16000], sun=[[0, -26214, 19661]])     # the sun in the south at 36.9 degrees
    minutes, direct, _ = hip_ops.solar_expose(sd, hz_n, hz_h, table, torch.from_numpy(lab).cuda(), torch.from_numpy(normal.astype(np.int32)).cuda())
    minutes, direct = minutes.cpu().numpy(), direct.cpu().numpy()
    assert (minutes == 30).all() and (direct[1] == 0).all()
    assert (direct[0] == (16000 * 19661 * 32768 >> 30)).all() and (direct[3] == direct[0]).all()
    assert (direct[2] == (16000 * (26214 * 26214 + 19661 * 19661) >> 30)).all() and direct[2, 0] in (15999, 16000)
    sums = hip_ops.solar_plane_sums(sd, torch.from_numpy(minutes).cuda(), torch.from_numpy(direct).cuda(), torch.from_numpy(lab).cuda(), 2).cpu().numpy()
    assert sums.tolist() == [[140, 70, 70], [4200, 2100, 2100], [140 * int(direct[0, 0]), 0, 70 * int(direct[2, 0])]]


def test_run_to_run_identity():
    import torch
    from ada_mvs_amd import hip_ops
    rng = np.random.default_rng(11)
    s = random_surface(rng, (65, 63), 40, 0.1)
    table = synthetic_table(32, *R.horizon_brute(s, 32), rng)
    lab, normal = labels_for(s.shape, rng)
    runs = []
    for _ in range(2):
        sd = device_surface(s)
        hz_n, hz_h, st, ws = hip_ops.solar_horizon(sd, 32)
        svf = hip_ops.solar_svf(sd, hz_n, hz_h, solar.direction_weights(32), Q)
        ld, nd = torch.from_numpy(lab).cuda(), torch.from_numpy(normal.astype(np.int32)).cuda()
        minutes, direct, ws = hip_ops.solar_expose(sd, hz_n, hz_h, table, ld, nd, ws)
        sums = hip_ops.solar_plane_sums(sd, minutes, direct, ld, 3)
        runs.append([t.cpu().numpy().tobytes() for t in (hz_n, hz_h, svf, minutes, direct, sums)] + [(st["lines"], st["deepest"], st["spills"])])
    assert runs[0] == runs[1]


def test_the_refusals_through_the_c_abi():
    import torch
    from ada_mvs_amd import hip_ops
    s = np.zeros((4, 6), np.int64)
    sd = device_surface(s)
    with pytest.raises(_lib.AdaMVSHipError, match="K=12"):
        hip_ops.solar_horizon(sd, 12)
    hz_n, hz_h, _, ws = hip_ops.solar_horizon(sd, 8)
    with pytest.raises(_lib.AdaMVSHipError, match="workspace"):
        _raw_horizon(sd, hz_n, hz_h, ws[:1024])
    row = dict(sector=[0], thr=[1.0], minutes=[1], energy=[1], sun=[[0, 0, 32768]])
    many = {k: list(v) * 8193 for k, v in row.items()}
    for bad, words in ((many, "T=8193"), (dict(row, sector=[8]), "sector"), (dict(row, thr=[float("nan")]), "thr"), (dict(row, minutes=[-1]), "weights"),
                       (dict(row, sun=[[0, 0, 40000]]), "sun"),
                       (dict(sector=[1, 0], thr=[1.0, 1.0], minutes=[1, 1], energy=[1, 1], sun=[[0, 0, 32768]] * 2), "ascending"),
                       ({k: list(v) * 3 for k, v in dict(row, energy=[2 ** 30]).items()}, "2\\^31 - 1")):
        with pytest.raises(_lib.AdaMVSHipError, match=words):
            hip_ops.solar_expose(sd, hz_n, hz_h, bad)
    lab = torch.zeros(4, 6, dtype=torch.int32, device="cuda")
    lab[2, 3] = 2
    normal = torch.tensor([[0, 0, 32768], [0, 0, 32768]], dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.AdaMVSHipError, match="label outside 0 .. P=1"):
        hip_ops.solar_expose(sd, hz_n, hz_h, row, lab, normal)
    with pytest.raises(_lib.AdaMVSHipError, match="go together"):
        hip_ops.solar_expose(sd, hz_n, hz_h, row, lab, None)
    with pytest.raises(_lib.AdaMVSHipError, match="weight"):
        hip_ops.solar_svf(sd, hz_n, hz_h, [0.125] * 7 + [0.0], Q)
    with pytest.raises(_lib.AdaMVSHipError, match="q="):
        hip_ops.solar_svf(sd, hz_n, hz_h, [0.125] * 8, 0.0)
    with pytest.raises(_lib.AdaMVSHipError, match="overlap"):
        _raw_horizon(sd, hz_n, hz_n, ws)
    with pytest.raises(ValueError, match="8191 m"):
        solar.expose(np.full((3, 3), 9000.0, np.float32), 0.5, latitude=30.5)


def _raw_horizon(sd, hz_n, hz_h, ws):
    import ctypes
    from ada_mvs_amd import hip_ops
    st = _lib.SolarStats()
    H, W = sd.shape
    hip_ops.check(_lib.load().adamvs_solar_horizon(W, H, 8, hip_ops._p(sd), hip_ops._p(ws), ws.numel(), hip_ops._p(hz_n), hip_ops._p(hz_h),
                                                   ctypes.byref(st), None), "solar_horizon")


# ---- the stage and the CLI ----------------------------------------------------------------------------------------------------------
def scene():
    """96 x 80 cells at gsd 0.5: ground falling gently to the east, a box building of 8 m and a gable building whose two roof faces
    are the planes 1 and 2, one cell without a value."""
    H, W = 96, 80
    z = np.tile(20.0 - 0.01 * np.arange(W, dtype=np.float64), (H, 1))
    z[10:30, 50:70] = 28.0
    label = np.zeros((H, W), np.int32)
    rows = np.arange(40, 60)
    for i in rows:                                                   # a ridge along row 50: the north face rises southwards, the south face falls
        z[i, 20:50] = 24.0 + 0.4 * (10 - abs(i - 50 + 0.5) + 0.5)
    label[40:50, 20:50], label[50:60, 20:50] = 1, 2
    z[70, 5] = np.nan
    slope = 0.4 / 0.5                                                # metres per metre
    nlen = math.sqrt(1 + slope * slope)
    normals = [[0.0, slope / nlen, 1 / nlen], [0.0, -slope / nlen, 1 / nlen]]       # the north face looks north, the south face south
    return z.astype(np.float32), label, normals


def write_scene(prefix):
    from PIL import Image
    z, label, normals = scene()
    H, W = z.shape
    with open(prefix + "_dsm.json", "w") as f:
        json.dump(dict(grid=dict(x0=1000.0, y_top=2000.0, gsd=0.5, W=W, H=H), z_ref=20.0), f)
    Image.fromarray(z).save(prefix + "_dsm_filled.tif", format="TIFF")
    Image.fromarray(label).save(prefix + "_roofs.tif", format="TIFF")
    feats = [dict(type="Feature", properties=dict(id=r + 1, building=1, cells=300, area_3d_m2=75.0 * math.sqrt(1.64), normal=normals[r]),
                  geometry=dict(type="Polygon", coordinates=[[[1010.0, 1980.0 - 5 * r], [1025.0, 1980.0 - 5 * r], [1025.0, 1975.0 - 5 * r],
                                                              [1010.0, 1980.0 - 5 * r]]])) for r in (1, 0)]
    with open(prefix + "_roofs.geojson", "w") as f:
        json.dump(dict(type="FeatureCollection", features=feats), f)
    return z, label, normals


def test_the_stage_equals_the_restatement_on_a_scene():
    z, label, normals = scene()
    got = solar.expose(z, 0.5, 20.0, label, normals, directions=16, latitude=30.5, shadow_at=(172, 9.5))
    s = R.surface(z, 20.0)
    assert np.array_equal(got["s"], s) and got["s"][70, 5] == R.NONE
    rn, rh = R.horizon_brute(s, 16)
    assert np.array_equal(got["hz_n"], rn) and np.array_equal(got["hz_h"], rh)
    ref_svf = R.svf(s, rn, rh, solar.direction_weights(16), (256.0 * 0.5) ** 2)
    assert np.array_equal(got["svf"].view(np.int64), ref_svf.view(np.int64))
    table, nq = got["samples"], solar.quantise_normals(normals)
    rm, rd = R.expose(s, rn, rh, table, label, nq)
    assert np.array_equal(got["minutes"], rm) and np.array_equal(got["direct"], rd)
    assert np.array_equal(got["table"], R.plane_sums(s, rm, rd, label, 2))
    assert got["counts"]["valid"] == 96 * 80 - 1 and got["counts"]["planes"] == 2 and got["counts"]["samples"] == table["sector"].size
    # at 30.5 degrees north the south face of the gable receives more than the north face, and a cell in the open more hours than
    # one at the foot of the box building's north wall
    p = got["planes"]
    assert p["direct_kwh_m2"][2] > p["direct_kwh_m2"][1] > 0 and p["global_kwh_m2"][2] > p["direct_kwh_m2"][2]
    assert got["sun_hours"][80, 40] > got["sun_hours"][9, 60] and np.isnan(got["sun_hours"][70, 5]) and got["shadow"][70, 5] == 255
    assert abs(p["sun_hours"][2] - got["sun_hours"][label == 2].mean()) < 1e-9
    D, per = got["diffuse"], 1 / 16000.0
    assert np.allclose(got["global_kwh"][label == 0][:50], ((rd + D * ref_svf) * per)[label == 0][:50], rtol=1e-12, atol=0)
    assert set(np.unique(got["shadow"]).tolist()) == {0, 1, 255}


def test_solar_whu_end_to_end(tmp_path):
    from PIL import Image
    P, O = str(tmp_path / "dsm"), str(tmp_path / "out" / "sun")
    z, label, normals = write_scene(P)
    args = ["--dsm", P, "--latitude", "30.5", "--directions", "16", "--shadow_at", "172,9.5", "--out", O]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "solar_whu.py")] + args, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "total_time" in r.stdout and "16 directions" in r.stdout
    got = solar.expose(z, 0.5, 20.0, label, normals, directions=16, latitude=30.5, shadow_at=(172, 9.5))
    paths = solar.output_paths(O)
    hole = np.isnan(z)
    for key, name, dtype in (("svf", "svf", np.float32), ("sunhours", "sun_hours", np.float32), ("direct", "direct_kwh", np.float32),
                             ("global_", "global_kwh", np.float32), ("shadow", "shadow", np.uint8)):
        a = np.array(Image.open(paths[key]))
        assert a.dtype == dtype and a.shape == z.shape, key
        want = np.where(hole, np.nan, got[name]).astype(np.float32) if dtype == np.float32 else got[name]
        assert np.array_equal(a, want, equal_nan=dtype == np.float32), key
        assert (np.isnan(a) == hole).all() if dtype == np.float32 else ((a == 255) == hole).all()
    with open(paths["geojson"]) as f:
        gj = json.load(f)
    assert [f["properties"]["id"] for f in gj["features"]] == [2, 1]
    for f in gj["features"]:
        pr, r_ = f["properties"], f["properties"]["id"]
        assert tuple(pr)[-4:] == solar.ADDED and tuple(pr)[:5] == ("id", "building", "cells", "area_3d_m2", "normal")
        for key in ("sun_hours", "direct_kwh_m2", "global_kwh_m2"):
            assert pr[key] == float("%.6g" % got["planes"][key][r_]), key
        assert pr["global_kwh"] == float("%.6g" % (got["planes"]["global_kwh_m2"][r_] * pr["area_3d_m2"]))
        assert f["geometry"]["type"] == "Polygon"
    with open(paths["json"]) as f:
        js = json.load(f)
    assert js["grid"] == dict(x0=1000.0, y_top=2000.0, gsd=0.5, W=80, H=96) and js["source"] == dict(prefix=P, raster="dsm_filled")
    assert js["params"]["directions"] == 16 and js["params"]["latitude"] == 30.5 and js["params"]["surface"] == "roofs"
    assert js["samples"] == got["counts"]["samples"] and js["counts"] == got["counts"] and js["stats"]["horizon"]["lines"] == got["stats"]["horizon"]["lines"]
    assert set(js["seconds"]) == {"horizon", "svf", "expose", "planes", "host"}
