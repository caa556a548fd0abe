"""The host side of the solar stage (ada_mvs_amd/solar.py) and its restatement (tests/solar_ref.py) without a GPU: the hull walk
against the brute force over every distance, the direction table against the header's literal, weights and sectors, the closed-form
numbering of the lattice lines against an enumeration, the sample table, the sun's positions against identities of the spherical
triangle, the parameter checks, the refusals and the new entry points."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
import solar_ref as R
from ada_mvs_amd import _lib, buildings, contours, drainage, dsm, dtm, roofs, solar, trees
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "adamvs_hip.h")).read()


def random_surface(rng, H, W, top, holes):
    s = rng.integers(0, top + 1, (H, W)).astype(np.int64)
    s[rng.random((H, W)) < holes] = R.NONE
    return s


# ---- the hull walk against the brute force ----------------------------------------------------------------------------------------
def test_hull_walk_equals_the_brute_force_in_all_32_directions():
    """K = 32 holds the directions of K = 8 and 16.  Heights 0 .. 1 tie everywhere, 0 .. 50 rarely; with holes the step counter runs
    on while the stack does not."""
    rng = np.random.default_rng(1981)
    shapes = [(1, 1), (1, 7), (6, 1), (2, 2), (3, 5), (7, 4), (9, 9), (13, 13), (13, 5)]
    compared = 0
    for top in (1, 3, 50):
        for holes in (0.0, 0.1, 0.3):
            for H, W in shapes:
                s = random_surface(rng, H, W, top, holes)
                bn, bh = R.horizon_brute(s, 32)
                hn, hh, st = R.horizon_hull(s, 32)
                assert np.array_equal(bn, hn) and np.array_equal(bh, hh), (top, holes, H, W)
                pn, ph, plain = R.horizon_hull(s, 32, collapse=False)                         # the plain loop that pushes every cell
                assert np.array_equal(bn, pn) and np.array_equal(bh, ph) and plain["deepest"] >= st["deepest"]
                assert st["lines"] == sum(R.line_count(H, W, di, dj) for di, dj in R.directions(32))
                assert ((bn > 0) == (bh > 0)).all() and (bn[:, s == R.NONE] == 0).all()
                compared += 32
    assert compared == 32 * 81


def test_hull_walk_on_hand_cases():
    # a tower of 5 units at column 4 of a flat row: looking east (k = 2 of 8) every cell west of it sees it at its distance
    s = np.zeros((1, 8), np.int64)
    s[0, 4] = 5
    n, h, _ = R.horizon_hull(s, 8)
    assert n[2, 0].tolist() == [4, 3, 2, 1, 0, 0, 0, 0] and h[2, 0].tolist() == [5, 5, 5, 5, 0, 0, 0, 0]
    assert n[6, 0].tolist() == [0, 0, 0, 0, 0, 1, 2, 3] and (n[0] == 0).all() and (n[4] == 0).all()
    # collinear occluders: heights 0 1 2 3 seen from the first cell looking east all have h / n = 1: the nearest wins
    s = np.array([[0, 1, 2, 3]], np.int64)
    n, h, _ = R.horizon_hull(s, 8)
    assert (n[2, 0, 0], h[2, 0, 0]) == (1, 1) and (R.horizon_brute(s, 8)[0][2, 0, 0]) == 1
    # a hole is transparent: it neither occludes nor gets a result
    s = np.array([[0, R.NONE, 4, 0]], np.int64)
    n, h, _ = R.horizon_hull(s, 8)
    assert (n[2, 0].tolist(), h[2, 0].tolist()) == ([2, 0, 0, 0], [4, 0, 0, 0]) and n[6, 0].tolist() == [0, 0, 0, 1]
    # a concave ramp keeps every cell on the hull: the stack outgrows the window and spills; a plane's never holds more than two
    side = 2 * R.WINDOW + 3
    x = np.arange(side, dtype=np.int64)
    ramp = np.tile(-(x * x), (1, 1))
    assert R.horizon_hull(ramp, 8)[2] == dict(lines=6 * side + 2, deepest=side, spills=2 * (side - R.WINDOW))
    plane = np.tile(3 * x, (1, 1))
    st = R.horizon_hull(plane, 8)[2]
    assert st["spills"] == 0 and st["deepest"] == 2                                          # collinear cells replace one another
    assert R.horizon_hull(plane, 8, collapse=False)[2]["deepest"] == side


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def test_direction_table_equals_the_header_literal_and_its_definition():
    for K in (8, 16, 32):
        m = re.search(r"#define ADAMVS_SOLAR_DIRS_%d (\{.*\})\n" % K, HEADER)
        literal = [tuple(int(v) for v in p) for p in re.findall(r"\{(-?\d+), (-?\d+)\}", m.group(1))]
        assert literal == list(solar.DIRECTIONS[K]) == R.directions(K) and len(literal) == K
        assert literal[0] == (-1, 0) and literal[K // 4] == (0, 1) and literal[K // 2] == (1, 0)
        az = solar.direction_azimuths(K)
        assert (np.diff(az) > 0).all() and az[0] == 0.0 and np.allclose(az, R.azimuths(K), rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="8, 16 or 32"):
        solar.direction_weights(12)


def test_weights_sum_to_one_and_sectors_split_at_the_bisectors():
    for K in (8, 16, 32):
        w = solar.direction_weights(K)
        assert abs(w.sum() - 1.0) < 1e-15 and (w > 0).all() and np.allclose(w, R.weights(K), rtol=0, atol=1e-16)
        assert np.allclose(w, w[::-1][np.arange(K) - 1], rtol=0, atol=1e-16)                # symmetric about north
        az = solar.direction_azimuths(K)
        assert solar.sector(0.0, K) == 0 and solar.sector(2 * math.pi, K) == 0 and solar.sector(-1e-9, K) == 0
        for k in range(K):
            nxt = (k + 1) % K
            mid = az[k] + ((az[nxt] - az[k]) % (2 * math.pi)) / 2
            assert solar.sector(az[k], K) == k == R.sector(az[k], K)
            assert solar.sector(mid, K) == min(k, nxt) == R.sector(mid, K), (K, k)         # the tie goes to the smaller k
            assert solar.sector(mid - 1e-9, K) == k and solar.sector(mid + 1e-9, K) == nxt
    assert np.allclose(solar.direction_weights(8), 0.125, rtol=0, atol=1e-16)


def test_line_starts_in_closed_form_against_an_enumeration():
    """Every shape has directions whose step exceeds a side (|di| >= H or |dj| >= W)."""
    for H, W in ((1, 1), (1, 5), (2, 7), (3, 3), (5, 2), (4, 6), (3, 1)):
        for di, dj in R.directions(32):
            starts = [(i, j) for i in range(H) for j in range(W) if not (0 <= i + di < H and 0 <= j + dj < W)]
            count = R.line_count(H, W, di, dj)
            assert count == len(starts) == H * W - max(H - abs(di), 0) * max(W - abs(dj), 0)
            numbered = [R.line_start(l, H, W, di, dj) for l in range(count)]
            assert sorted(numbered) == sorted(starts) and len(set(numbered)) == count
            a = min(abs(di), H)
            assert all(numbered[l] == ((l // W if di < 0 else H - a + l // W), l % W) for l in range(a * W))     # the full rows first
            cells = [c for l in range(count) for c in R.line_cells(l, H, W, di, dj)]
            assert sorted(cells) == [(i, j) for i in range(H) for j in range(W)]                                  # the lines partition the raster


# ---- the sun ----------------------------------------------------------------------------------------------------------------------
def test_sun_positions_identities():
    for lat in (30.5, 52.0, -35.0, 66.0):
        for day in (21, 80, 172, 264, 355):
            dec = math.degrees(float(solar.declination(day)))
            az, el = solar.sun_at(lat, day, 12.0)
            assert abs(math.degrees(float(el)) - (90.0 - abs(lat - dec))) < 1e-9
            if lat > dec:
                assert abs(float(az) - math.pi) < 1e-9                                       # due south at noon
            else:
                assert min(float(az), 2 * math.pi - float(az)) < 1e-9
            for hour in (0.25, 3.0, 6.5, 11.75):
                (a1, e1), (a2, e2) = solar.sun_at(lat, day, 12.0 - hour), solar.sun_at(lat, day, 12.0 + hour)
                assert abs(float(e1) - float(e2)) < 1e-9 and abs(float(a1) - (2 * math.pi - float(a2))) < 1e-9
    assert abs(math.degrees(float(solar.declination(172))) - 23.44) < 0.1
    pos = solar.sun_positions(30.5)
    assert pos["hour"].size == 12 * 48 and pos["hour"][0] == 0.25 and pos["weight"].reshape(12, 48)[:, 0].tolist() == [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    assert pos["day"].reshape(12, 48)[:, 0].tolist() == [21, 52, 80, 111, 141, 172, 202, 233, 264, 294, 325, 355]
    el = pos["elevation"].reshape(12, 48)
    assert np.allclose(el, el[:, ::-1], rtol=0, atol=1e-9)                                   # morning and afternoon mirror
    assert abs(float(solar.clear_sky_dni(math.pi / 2)) - 1353.0 * 0.7 ** (1.0 / (1.0 + 0.50572 * 96.07995 ** -1.6364)) ** 0.678) < 1e-9


def test_sample_table_quantisation_sort_and_refusals():
    t = solar.sample_table(0.2, 32, 30.5)
    T = t["sector"].size
    assert 250 < T < 350 and (np.diff(t["sector"]) >= 0).all() and t["sector"].min() >= 0 and t["sector"].max() < 32
    assert t["minutes"].sum() == 30 * sum(w * int((solar.sun_positions(30.5, [d])["elevation"] > 0).sum()) for d, w in solar.MONTH_DAYS)
    for i in range(T):
        az, el, k = float(t["azimuth"][i]), float(t["elevation"][i]), int(t["sector"][i])
        di, dj = solar.DIRECTIONS[32][k]
        assert k == R.sector(az, 32) and el > 0
        assert t["thr"][i] == math.tan(el) * math.sqrt(di * di + dj * dj) * 0.2 * 256.0
        v = (math.sin(az) * math.cos(el), math.cos(az) * math.cos(el), math.sin(el))
        assert t["sun"][i].tolist() == [round(32768 * c) for c in v] and abs(np.linalg.norm(t["sun"][i]) - 32768) < 1.0
    weight = t["minutes"] // 30
    dni = solar.clear_sky_dni(t["elevation"])
    assert np.array_equal(t["energy"], np.rint(16 * 1.0 * dni * 0.5 * weight).astype(np.int64))
    assert abs(t["diffuse"] - float(np.sum(0.1 * dni * np.sin(t["elevation"]) * 8.0 * weight))) < 1e-6 * t["diffuse"]
    half = solar.sample_table(0.2, 32, 30.5, clearness=0.5)
    assert np.abs(2 * half["energy"] - t["energy"]).max() <= 1 and half["diffuse"] == t["diffuse"]
    # a table of one's own: sorted by sector, the rows below the horizon only add to D
    own = solar.sample_table(0.5, 8, sun=[[270.0, 30.0, 10, 500.0, 50.0], [90.0, 45.0, 20, 800.0, 80.0], [0.0, -5.0, 30, 0.0, 7.0]])
    assert own["sector"].tolist() == [2, 6] and own["minutes"].tolist() == [20, 10] and own["energy"].tolist() == [12800, 8000]
    assert own["diffuse"] == 16 * 137.0 and own["sun"][0].tolist() == [round(32768 * math.cos(math.pi / 4)), 0, round(32768 * math.sin(math.pi / 4))]
    assert own["thr"][0] == math.tan(math.radians(45.0)) * 1.0 * 0.5 * 256.0
    with pytest.raises(ValueError, match="at most 8192"):
        solar.sample_table(0.2, 32, 30.5, days=list(range(1, 366)), step_min=15)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        solar.sample_table(0.2, 8, sun=[[90.0, 45.0, 2 ** 30, 1.0, 0.0]] * 3)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        solar.sample_table(0.2, 8, sun=[[90.0, 45.0, 1, 2.0 ** 27, 0.0]] * 2)
    with pytest.raises(ValueError, match=r"\[T, 5\]"):
        solar.sample_table(0.2, 8, sun=[[90.0, 45.0, 1.0]])
    with pytest.raises(ValueError, match="minutes must be integers"):
        solar.sample_table(0.2, 8, sun=[[90.0, 45.0, 1.5, 1.0, 0.0]])


# ---- parameters, files, refusals ------------------------------------------------------------------------------------------------
def test_parameters_and_their_refusals():
    p = solar.parameters(0.5, latitude=30.5)
    assert p == dict(directions=32, latitude=30.5, days=[list(d) for d in solar.MONTH_DAYS], step_min=30, clearness=1.0, surface="roofs",
                     source="dsm_filled", own_sun=False)
    assert sum(w for _, w in solar.MONTH_DAYS) == 365
    assert solar.parameters(0.5, sun=[[0, 0, 0, 0, 0]])["latitude"] is None
    with pytest.raises(ValueError, match="latitude is required"):
        solar.parameters(0.5)
    for bad in (dict(directions=12), dict(directions=True), dict(latitude=91.0), dict(latitude=float("nan")), dict(step_min=0), dict(step_min=7),
                dict(step_min=240), dict(clearness=1.5), dict(clearness=-0.1), dict(surface="walls"), dict(source="ndsm"), dict(days=[0]),
                dict(days=[400]), dict(days=[]), dict(days=[(21, 0)]), dict(days=[1.5])):
        with pytest.raises(ValueError):
            solar.parameters(0.5, **dict(dict(latitude=30.5), **bad))
    with pytest.raises(ValueError):
        solar.parameters(0.0, latitude=30.5)
    assert (solar.STACK_WINDOW, solar.MAX_SAMPLES, solar.MAX_SIDE) == (_lib.SOLAR_STACK_WINDOW, _lib.SOLAR_MAX_SAMPLES, _lib.SOLAR_MAX_SIDE)
    assert R.WINDOW == solar.STACK_WINDOW == 16
    q = solar.quantise_normals([[0.0, 0.6, 0.8]])
    assert q.tolist() == [[0, 0, 32768], [0, 19661, 26214]]
    with pytest.raises(ValueError, match="unit vectors"):
        solar.quantise_normals([[0.0, 0.0, 1.5]])


def test_output_paths_are_disjoint_from_every_earlier_stage():
    mine = set(solar.output_paths("/o/p").values())
    assert mine == {"/o/p_svf.tif", "/o/p_sunhours.tif", "/o/p_direct.tif", "/o/p_global.tif", "/o/p_shadow.tif", "/o/p_solar_roofs.geojson",
                    "/o/p_solar.json"}
    for other in (dsm.output_paths("/o/p"), dsm.fill_output_paths("/o/p"), dtm.output_paths("/o/p"), buildings.output_paths("/o/p"),
                  roofs.output_paths("/o/p"), trees.output_paths("/o/p"), contours.output_paths("/o/p"), drainage.output_paths("/o/p")):
        assert not mine & set(other.values())


def test_geojson_text_appends_the_columns_in_a_fixed_order():
    roofs_gj = dict(type="FeatureCollection", features=[
        dict(type="Feature", properties=dict(id=2, area_3d_m2=10.0, normal=[0.0, 0.6, 0.8]), geometry=dict(type="Polygon", coordinates=[])),
        dict(type="Feature", properties=dict(id=1, area_3d_m2=4.0, normal=[0.0, 0.0, 1.0]), geometry=dict(type="Polygon", coordinates=[]))])
    planes = dict(sun_hours=np.array([0.0, 1234.5678, 2000.0]), direct_kwh_m2=np.array([0.0, 1.5, 2.5]), global_kwh_m2=np.array([0.0, 1.75, float("nan")]))
    a = solar.geojson_text(roofs_gj, planes)
    assert a == solar.geojson_text(json.loads(json.dumps(roofs_gj)), planes) and a.endswith("\n") and " " not in a
    f = json.loads(a)["features"]
    assert tuple(f[0]["properties"])[-4:] == solar.ADDED and tuple(f[0]["properties"])[:3] == ("id", "area_3d_m2", "normal")
    assert f[1]["properties"]["sun_hours"] == 1234.57 and f[1]["properties"]["global_kwh"] == 7.0 and f[0]["properties"]["global_kwh_m2"] is None
    assert solar.geojson_text(None, planes) == '{"type":"FeatureCollection","features":[]}\n'


def test_expose_raises_without_a_gpu_and_for_absent_files(monkeypatch, tmp_path):
    import torch
    from PIL import Image
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    z = np.zeros((4, 4), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        solar.expose(z, 0.5, latitude=30.5)
    with pytest.raises(ValueError, match="latitude is required"):
        solar.expose(z, 0.5)
    with pytest.raises(ValueError, match="directions"):
        solar.expose(z, 0.5, latitude=30.5, directions=24)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        solar.expose(z[0], 0.5, latitude=30.5)
    with pytest.raises(ValueError, match="go together"):
        solar.expose(z, 0.5, latitude=30.5, label=np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="values 0 .. 1"):
        solar.expose(z, 0.5, latitude=30.5, label=np.full((4, 4), 2, np.int32), normals=[[0.0, 0.0, 1.0]])
    P = str(tmp_path / "dsm")
    with pytest.raises(FileNotFoundError, match="dsm_whu.py"):
        solar.from_dsm(P, latitude=30.5)
    with pytest.raises(ValueError, match="latitude is required"):
        solar.from_dsm(P)
    with open(P + "_dsm.json", "w") as f:
        json.dump(dict(grid=dict(x0=0.0, y_top=2.0, gsd=0.5, W=4, H=4), z_ref=0.0), f)
    with pytest.raises(FileNotFoundError, match=r"--fill_max_dist.*--source dsm"):
        solar.from_dsm(P, latitude=30.5)
    with pytest.raises(FileNotFoundError, match="dtm_whu.py"):
        solar.from_dsm(P, source="dtm", latitude=30.5)
    Image.fromarray(z).save(P + "_dsm.tif", format="TIFF")
    with pytest.raises(FileNotFoundError, match="roofs_whu.py"):
        solar.from_dsm(P, source="dsm", latitude=30.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        solar.from_dsm(P, source="dsm", surface="horizontal", latitude=30.5)
    with pytest.raises(FileNotFoundError, match="sun table"):
        solar.read_sun_table(str(tmp_path / "none.txt"))
    (tmp_path / "sun.txt").write_text("# az el min dn dh\n90 45 20 800 80\n")
    assert solar.read_sun_table(str(tmp_path / "sun.txt")).tolist() == [[90.0, 45.0, 20.0, 800.0, 80.0]]


def test_parser_defaults_help_and_the_stated_limits():
    a = solar.build_parser().parse_args(["--dsm", "/x/dsm", "--latitude", "30.5"])
    assert (a.dsm, a.source, a.surface, a.directions, a.latitude, a.days, a.step_min, a.clearness, a.sun_table, a.shadow_at, a.out) == \
        ("/x/dsm", "dsm_filled", "roofs", 32, 30.5, None, 30, 1.0, None, None, None)
    a = solar.build_parser().parse_args(["--dsm", "p", "--source", "dtm", "--surface", "horizontal", "--directions", "16", "--shadow_at", "172,9.5",
                                         "--out", "q"])
    assert (a.source, a.surface, a.directions, a.shadow_at, a.out) == ("dtm", "horizontal", 16, (172, 9.5), "q")
    for bad in (["--directions", "12"], ["--source", "ndsm"], ["--shadow_at", "400,9"], ["--shadow_at", "noon"]):
        with pytest.raises(SystemExit):
            solar.build_parser().parse_args(["--dsm", "p"] + bad)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "solar_whu.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "--latitude" in r.stdout and "--sun_table" in r.stdout and "dsm_filled" in r.stdout
    doc = " ".join(solar.__doc__.split())
    for words in ("snapped to the nearest of the K directions", "Clear sky only", "Nothing outside the raster casts a shadow", "No reflected light",
                  "Tree canopy occludes as a solid", "are conventions", "not values measured on WHU scenes", "isotropic-sky convention"):
        assert words in doc, words


def test_the_new_entry_points_refuse_before_any_launch():
    names = ("adamvs_solar_workspace_bytes", "adamvs_solar_horizon", "adamvs_solar_svf", "adamvs_solar_expose", "adamvs_solar_plane_sums")
    for name in names:
        assert name in _lib.SIGNATURES and name + "(" in HEADER
    assert "#define ADAMVS_ABI_VERSION 22" in HEADER and _lib.ABI_VERSION == 22
    assert "---- Solar" in HEADER and HEADER.index("---- Drainage") < HEADER.index("---- Solar") < HEADER.index("---- TSDF mesh")
    for text in ("#define ADAMVS_SOLAR_STACK_WINDOW 16", "#define ADAMVS_SOLAR_MAX_SAMPLES 8192", "#define ADAMVS_SOLAR_MAX_SIDE 32768",
                 "#define ADAMVS_SOLAR_HEAD_BYTES 262656", "#define ADAMVS_SOLAR_BAD_LABEL (-2)"):
        assert text in HEADER
    assert _lib.SOLAR_HEAD_BYTES == 512 + 32 * 8192 and _lib.SOLAR_BAD_LABEL == -2
    assert ctypes.sizeof(_lib.SolarStats) == 2 * 8 + 2 * 4 + 2 * 4
    lib = _lib.load()
    ws = lib.adamvs_solar_workspace_bytes
    assert ws(7, 5, 8) == 262656 + 8 * 8 * 35 + (-(8 * 8 * 35) % 256) and ws(7, 5, 32) == 262656 + 8 * 32 * 35
    assert ws(7, 5, 12) < 0 and ws(0, 5, 8) < 0 and ws(32769, 1, 8) < 0 and ws(1, 32769, 8) < 0 and ws(1 << 15, 1 << 14, 8) < 0
    assert ws(32768, 1, 8) > 0
    st = _lib.SolarStats()
    assert lib.adamvs_solar_horizon(4, 4, 8, None, None, 0, None, None, ctypes.byref(st), None) < 0
    assert lib.adamvs_solar_horizon(4, 4, 9, None, None, 0, None, None, ctypes.byref(st), None) < 0
    w = (ctypes.c_double * 8)(*[0.125] * 8)
    assert lib.adamvs_solar_svf(4, 4, 8, None, None, None, w, 1.0, None, None) < 0
    one_i, one_d, sun = (ctypes.c_int * 1)(0), (ctypes.c_double * 1)(1.0), (ctypes.c_int * 3)(0, 0, 32768)
    assert lib.adamvs_solar_expose(4, 4, 8, None, None, None, 1, one_i, one_d, one_i, one_i, sun, None, 0, None, None, 0, None, None, None) < 0
    assert lib.adamvs_solar_expose(4, 4, 8, None, None, None, 8193, one_i, one_d, one_i, one_i, sun, None, 0, None, None, 0, None, None, None) < 0
    assert "T=8193" in lib.adamvs_last_error_string().decode()
    assert lib.adamvs_solar_plane_sums(4, 4, None, None, 0, None, None, None, None) < 0
