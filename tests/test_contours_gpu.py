"""Contour lines on the GPU (csrc/dsm_contours.hip through hip_ops and ada_mvs_amd/contours.py) against the numpy restatement
(tests/contours_ref.py): s, its range, the per-block counts, N, every segment field, succ, pred, start, rank, closed, the line
table and every vertex triple for exact equality, at every edge of the tiles, on cliffs, saddles, rings through every tile and
open lines between holes; run-to-run identity, argument errors and contours_whu.py end to end.  There is no tolerance and nothing
is left out."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
import contours_ref
from ada_mvs_amd import _lib, contours, dsm, dtm
from conftest import ROOT

pytestmark = pytest.mark.gpu

T = _lib.CONTOUR_TILE
NAMES = ("entry", "exit", "level", "succ", "pred", "start", "rank")
LINE_NAMES = ("line_start", "line_level")


def gpu_stage(z, z_ref, passes, lev):
    """-> the dict of contours_ref.trace through the five entry points; lev may be a function of (s_min, s_max)."""
    import torch
    from ada_mvs_amd import hip_ops
    zz = torch.from_numpy(np.ascontiguousarray(z, np.float32)).cuda()
    s, info = hip_ops.contour_surface(zz, z_ref, passes)
    info = tuple(int(v) for v in info.cpu().tolist())
    if callable(lev):
        lev = lev(info[0], info[1])
    count, N, ws, st = hip_ops.contour_count(s, lev)
    seg = hip_ops.contour_segments(s, lev, N, ws)
    start, rank, closed, M, ws2, st = hip_ops.contour_rank(seg[4], stats=st)
    line_first, line_start, line_level, line_closed, vertex = hip_ops.contour_lines(s, lev, seg, start, rank, closed, M, ws2)
    res = dict(s=s, count=count, entry=seg[0], exit=seg[1], level=seg[2], succ=seg[3], pred=seg[4], start=start, rank=rank, closed=closed,
               line_first=line_first, line_start=line_start, line_level=line_level, line_closed=line_closed, vertex=vertex)
    res = {k: v.cpu().numpy() for k, v in res.items()}
    res.update(info=info, N=N, M=M, stats=st, lev=list(lev))
    return res


def rounds_bound(N):
    return 2 * (math.ceil(math.log2(max(N, 2))) + 1)


def check_stage(z, z_ref=0.0, passes=0, lev=None, interval=1.0, base=0.0):
    """The GPU result equals the restatement in every word.  -> (got, ref)."""
    if lev is None:
        lev = lambda s_min, s_max: contours.level_table(s_min, s_max, z_ref, interval, base, passes)[0]
    ref = contours_ref.trace(z, z_ref, passes, None if callable(lev) else lev, lev if callable(lev) else None)
    got = gpu_stage(z, z_ref, passes, lev)
    assert got["lev"] == ref["lev"]
    assert got["s"].dtype == np.int32 and np.array_equal(got["s"], ref["s"]), np.argwhere(got["s"] != ref["s"])[:10]
    assert got["info"] == ref["info"]
    assert got["count"].dtype == np.int32 and np.array_equal(got["count"], ref["count"]), np.argwhere(got["count"] != ref["count"])[:10]
    assert (got["N"], got["M"]) == (ref["N"], ref["M"])
    for name in NAMES + LINE_NAMES:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], ref[name]), (name, np.flatnonzero(got[name] != ref[name])[:10])
    for name in ("closed", "line_closed"):
        assert got[name].dtype == np.uint8 and np.array_equal(got[name], ref[name]), name
    assert got["line_first"].dtype == np.int64 and np.array_equal(got["line_first"], ref["line_first"])
    assert got["vertex"].dtype == np.int64 and got["vertex"].shape == (ref["N"] + ref["M"], 3)
    assert np.array_equal(got["vertex"], ref["vertex"]), np.argwhere(got["vertex"] != ref["vertex"])[:10]
    if ref["N"]:
        assert (got["vertex"][:, 1] > 0).all() and (got["vertex"][:, 1] < got["vertex"][:, 2]).all()
    st = got["stats"]
    print("N %d, M %d, rounds %d + %d (bound %d), launched %d" % (ref["N"], ref["M"], st.rounds_min, st.rounds_dist, rounds_bound(ref["N"]),
                                                                  st.launched))
    assert st.converged == 1 and st.rounds == st.rounds_min + st.rounds_dist <= rounds_bound(ref["N"])
    assert (st.segments, st.lines) == (ref["N"], ref["M"])
    return got, ref


def world_area2(got, m, W):
    """Twice the signed area of line m in world orientation (x east, y north)."""
    grid = dsm.Grid(0.0, 0.0, 1.0, 0.0, W, 0)
    xy = contours.vertex_coordinates(got["vertex"][got["line_first"][m]:got["line_first"][m + 1]], grid)
    return float(np.sum(xy[:-1, 0] * xy[1:, 1] - xy[1:, 0] * xy[:-1, 1]))


# ---- the smallest shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, T + 2), (T + 2, 1)])
def test_no_block(H, W):
    rng = np.random.default_rng(H + W)
    got, _ = check_stage(rng.integers(0, 5, (H, W)).astype(np.float32) + 0.5)
    assert got["N"] == 0 and got["M"] == 0 and got["line_first"].tolist() == [0]


@pytest.mark.parametrize("pattern", range(16))
def test_two_by_two_patterns(pattern):
    z = np.array([[pattern & 1, (pattern >> 1) & 1], [(pattern >> 3) & 1, (pattern >> 2) & 1]], np.float32)      # A B / D C
    got, _ = check_stage(z, lev=[128])
    assert got["N"] == (0 if pattern in (0, 15) else 2 if pattern in (5, 10) else 1)
    assert got["M"] == got["N"] and not got["closed"].any()


@pytest.mark.parametrize("a,b,c,d,centre_up", [(300, 299, 300, 299, True), (300, 299, 300, 298, False), (299, 300, 299, 300, True),
                                               (299, 300, 298, 300, False), (900, 0, 900, 0, True), (301, 0, 300, 0, False),
                                               (0, 900, 0, 900, True), (0, 300, 0, 301, False)])
def test_saddle_centre(a, b, c, d, centre_up):
    """Both saddles on either side of the centre test; the first and third make it an equality: 2 (a + b + c + d) == 4 (2 lev - 1)."""
    lev = 300
    assert (2 * (a + b + c + d) >= 4 * (2 * lev - 1)) == centre_up
    if (a, b, c, d) in ((300, 299, 300, 299), (299, 300, 299, 300)):
        assert 2 * (a + b + c + d) == 4 * (2 * lev - 1)
    z = np.array([[a, b], [d, c]], np.float32) / 256.0
    got, _ = check_stage(z, lev=[lev])
    assert got["N"] == 2
    pairs = set(zip(got["entry"].tolist(), got["exit"].tolist()))
    code = lambda e: 2 * ((e == 2) * 2 + (e == 1)) + (e & 1)             # W = 2
    first = 1 if a >= lev else 0
    want = {(code(e), code((e - 1) % 4 if centre_up else (e + 1) % 4)) for e in (first, first + 2)}
    assert pairs == want


def test_degenerate_rasters():
    H, W = T + 3, T + 5
    for z in (np.full((H, W), np.nan, np.float32), np.full((H, W), 1.0, np.float32), np.full((H, W), 2.0, np.float32),
              np.full((H, W), 0.0, np.float32)):                        # all NaN, a plateau exactly at the level, all up, all down
        got, _ = check_stage(z, lev=[256])
        assert got["N"] == 0 and got["M"] == 0
    got, _ = check_stage(np.full((H, W), 1.0, np.float32))             # the table of level_table: the level 1 m is in it
    assert got["lev"] == [256] and got["N"] == 0
    got, _ = check_stage(np.full((H, W), 1.25, np.float32))            # between two levels: K = 0
    assert got["lev"] == [] and got["N"] == 0


# ---- the tile edges -------------------------------------------------------------------------------------------------------------
SIDES = [T - 1, T, T + 1, 2 * T + 1]                                     # blocks per side
SHAPES = [(n + 1, 10) for n in SIDES] + [(10, n + 1) for n in SIDES] + [(n + 1, n + 1) for n in SIDES]


@pytest.mark.parametrize("passes", [0, 1, 2])
@pytest.mark.parametrize("H,W", SHAPES)
def test_random_heights(H, W, passes):
    for density in (0.0, 0.05, 0.3):
        rng = np.random.default_rng(1000 * H + 10 * W + passes + int(100 * density))
        z = rng.integers(-2, 5, (H, W)).astype(np.float32)
        z[rng.random((H, W)) < density] = np.nan
        got, _ = check_stage(z, z_ref=-1.0, passes=passes)
        assert got["N"] > 0


def test_cliff():
    """310 levels in every block of one column across a tile edge, next to flat ground: more segments in one block than a
    workgroup has lanes, and offsets that jump by hundreds."""
    H, W = 20, T + 6
    z = np.zeros((H, W), np.float32)
    z[:, T:] = 310.25
    z[5:9, 3:9] = 1.5                                                    # a little relief on the flat side
    got, ref = check_stage(z)
    assert ref["count"][:, T - 1].max() >= 300 and ref["count"][:, T - 1].max() > 256 and len(ref["lev"]) >= 300
    got, ref = check_stage(z, passes=1)                                  # the pass spreads the step over two columns of blocks
    assert ref["count"].max() > 128


@pytest.mark.parametrize("level,centre_up", [(128, True), (200, False)])
def test_checkerboard_saddles(level, centre_up):
    H = W = T + 3
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = ((i + j) % 2).astype(np.float32)
    assert (2 * 2 * 256 >= 4 * (2 * level - 1)) == centre_up
    got, ref = check_stage(z, lev=[level])
    assert (ref["count"][:-1, :-1] == 2).all() and ref["N"] == 2 * (H - 1) * (W - 1)
    # centre up: the down samples are cut off one by one (rings of four round the inner ones); centre down: the up samples
    inner = ((i + j) % 2 == (0 if centre_up else 1))[1:-1, 1:-1].sum()
    assert int(got["line_closed"].sum()) == inner
    areas = [world_area2(got, m, W) for m in np.flatnonzero(got["line_closed"])]
    assert all(a < 0 for a in areas) if centre_up else all(a > 0 for a in areas)


@pytest.mark.parametrize("sign", [1, -1])
def test_cone(sign):
    H = W = 41
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = (sign * (10.0 - 0.5 * np.hypot(i - 20, j - 20))).astype(np.float32)
    lev = [256 * n for n in (range(1, 10) if sign > 0 else range(-9, 0))]
    got, ref = check_stage(z, lev=lev)
    assert got["M"] == 9 and got["line_closed"].all() and sorted(got["line_level"].tolist()) == list(range(9))
    area = {int(got["line_level"][m]): world_area2(got, m, W) for m in range(9)}
    assert all(a * sign > 0 for a in area.values())                    # summit: counter-clockwise; pit: clockwise
    sizes = [abs(area[k]) for k in range(9)]
    assert sizes == sorted(sizes, reverse=sign > 0)                     # nested, one per level


def comb(H, W, phase=1):
    """Teeth two rows high every four rows, from row `phase` on, joined by a spine in column 1; nothing high on the border."""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    high = (np.isin((i - phase) % 4, (0, 1)) & (j >= 1) & (j <= W - 2)) | (j == 1)
    return (high & (i >= 1) & (i <= H - 2)).astype(np.float32)


@pytest.mark.parametrize("H,W,phase", [(41, 40, 1), (2 * T + 2, 2 * T + 2, 0)])       # phase 0: the last tooth lies in the last row of blocks
def test_comb_is_one_ring(H, W, phase):
    got, ref = check_stage(comb(H, W, phase), lev=[128])
    assert (H, W) != (41, 40) or got["N"] == 820
    assert got["M"] == 1 and got["line_closed"].tolist() == [1] and got["line_start"].tolist() == [0]
    assert int(got["rank"].max()) == got["N"] - 1 and (got["start"] == 0).all()
    assert got["vertex"][0].tolist() == got["vertex"][-1].tolist()
    if (H, W) == (2 * T + 2, 2 * T + 2):
        tiles = {(int(c) // 2 // W // T, int(c) // 2 % W // T) for c in got["entry"].tolist()}
        assert len(tiles) == 9                                           # through every tile of the count kernel


def test_tilted_plane_with_holes():
    H, W = T + 8, 2 * T + 5
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = (0.31 * i + 0.17 * j).astype(np.float32)
    for r, c in ((10, 10), (30, T - 2), (50, T + 40), (T - 1, 100)):
        z[r:r + 6, c:c + 7] = np.nan
    got, ref = check_stage(z, passes=1)
    assert got["M"] > 20 and not got["line_closed"].any() and not got["closed"].any()
    ends = got["vertex"][np.concatenate([got["line_first"][:-1], got["line_first"][1:] - 1]), 0] >> 1
    ei, ej = ends // W, ends % W
    hole = np.pad(~np.isfinite(z), 2, constant_values=True)
    near = np.array([hole[a:a + 5, b:b + 5].any() for a, b in zip(ei.tolist(), ej.tolist())])      # the border or a hole within two cells
    assert near.all()


def test_two_runs_are_identical():
    rng = np.random.default_rng(7)
    z = rng.normal(0.0, 2.0, (T + 9, 2 * T + 3)).astype(np.float32)
    z[rng.random(z.shape) < 0.05] = np.nan
    lev = lambda lo, hi: contours.level_table(lo, hi, 0.0, 0.5, 0.0, 1)[0]
    a, b = gpu_stage(z, 0.0, 1, lev), gpu_stage(z, 0.0, 1, lev)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == b[k].tobytes(), k
    assert (a["N"], a["M"], a["info"]) == (b["N"], b["M"], b["info"])


# ---- the stage and the CLI ------------------------------------------------------------------------------------------------------
def synthetic_dtm(H=90, W=120):
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = 103.0 + 4.0 * np.exp(-((i - 40) ** 2 + (j - 50) ** 2) / 300.0) + 0.02 * j - 2.5 * np.exp(-((i - 60) ** 2 + (j - 95) ** 2) / 60.0)
    z = z.astype(np.float32)
    z[5:12, 100:110] = np.nan
    return z


def write_stage_inputs(prefix, z, grid):
    res = dict(dtm=z, ndsm=np.zeros_like(z), level=np.where(np.isfinite(z), 255, 0).astype(np.uint8), grid=grid, params={}, radius=[], dh=[],
               counts={}, fill={}, seconds={})
    dtm.write_outputs(prefix, res)
    with open(prefix + "_dsm.json", "w") as f:
        json.dump(dict(grid=dict(x0=grid.x0, y_top=grid.y_top, gsd=grid.gsd, W=grid.W, H=grid.H), z_ref=grid.z_ref), f)


def check_collection(fc, min_length=0.0):
    feats = fc["features"]
    assert [f["properties"]["id"] for f in feats] == list(range(1, len(feats) + 1))
    levels = [f["properties"]["level"] for f in feats]
    assert levels == sorted(levels)                                      # by level; the order inside a level is held through trace()'s `order`
    for f in feats:
        p, xy = f["properties"], f["geometry"]["coordinates"]
        assert list(p) == list(contours.PROPERTIES) and f["geometry"]["type"] == "LineString"
        assert p["closed"] == (xy[0] == xy[-1]) and p["vertices"] == len(xy) >= 2
        assert p["major"] == (p["level"] % 5 == 0) and p["elevation_m"] == p["level"] * 0.5
        length = sum(math.hypot(b[0] - a[0], b[1] - a[1]) for a, b in zip(xy, xy[1:]))
        assert abs(length - p["length_m"]) <= 1e-9 * max(1.0, length) and p["length_m"] >= min_length


def test_trace_and_cli_end_to_end(tmp_path):
    z = synthetic_dtm()
    H, W = z.shape
    grid = dsm.Grid(5e5, 3.4e6, 0.5, 100.0, W, H)
    res = contours.trace(z, grid.gsd, grid.z_ref, interval=0.5, grid=grid)
    ref = contours_ref.trace(z, grid.z_ref, 1, res["lev"])
    assert np.array_equal(res["vertex"], ref["vertex"]) and np.array_equal(res["line_first"], ref["line_first"])
    assert res["counts"]["lines"] == ref["M"] > 5 and res["counts"]["closed"] > 0 and res["counts"]["closed"] < ref["M"]
    # the order of the features: by level, then by line number
    order = res["order"].tolist()
    assert order == sorted(range(ref["M"]), key=lambda m: (int(ref["line_level"][m]), m))
    P = str(tmp_path / "cli" / "dsm")
    write_stage_inputs(P, z, grid)
    paths = contours.write_outputs(str(tmp_path / "direct"), res)
    run = lambda *args: subprocess.run([sys.executable, os.path.join(ROOT, "contours_whu.py")] + list(args), capture_output=True, text=True,
                                       timeout=300, cwd=ROOT)
    r = run("--dsm", P, "--interval", "0.5")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "total_time" in r.stdout
    assert sorted(os.listdir(os.path.dirname(P))) == sorted(os.path.basename(p) for p in
                                                            list(dtm.output_paths(P).values()) + [P + "_dsm.json"] + list(contours.output_paths(P).values()))
    with open(paths["geojson"], "rb") as f, open(contours.output_paths(P)["geojson"], "rb") as g:
        direct, cli = f.read(), g.read()
    assert direct == cli                                                 # two runs, byte-identical text
    fc, js = contours.read_outputs(P)
    check_collection(fc)
    assert len(fc["features"]) == ref["M"] and js["counts"]["segments"] == ref["N"] and js["params"]["lev"] == res["lev"]
    assert js["source"] == dict(prefix=P, raster="dtm") and js["stats"]["converged"] == 1
    lengths = sorted(f["properties"]["length_m"] for f in fc["features"])
    cut = (lengths[len(lengths) // 2 - 1] + lengths[len(lengths) // 2]) / 2
    assert lengths[len(lengths) // 2 - 1] < cut < lengths[len(lengths) // 2]
    out2 = str(tmp_path / "cli" / "long")
    contours.main(["--dsm", P, "--interval", "0.5", "--min_length", repr(cut), "--out", out2])      # the CLI's main, in this process
    fc2, js2 = contours.read_outputs(out2)
    check_collection(fc2, cut)
    kept = [f for f in fc["features"] if f["properties"]["length_m"] >= cut]
    assert [f["geometry"] for f in fc2["features"]] == [f["geometry"] for f in kept] and 0 < len(kept) < len(fc["features"])
    assert js2["counts"]["rejected_short"] == len(fc["features"]) - len(kept)
    contours.main(["--dsm", P, "--source", "ndsm"])                      # a flat nDSM: no line, still the files
    assert contours.read_outputs(P)[0]["features"] == []


def test_out_of_range_heights_raise():
    z = np.zeros((4, 5), np.float32)
    z[2, 3] = 9000.0
    with pytest.raises(ValueError, match="8191"):
        contours.trace(z, 1.0)
    # the count itself, over several waves and workgroups, with the edge of the range on either side
    import torch
    from ada_mvs_amd import hip_ops
    rng = np.random.default_rng(3)
    z = rng.choice(np.array([0.0, 8191.0, -8191.0, 8191.5, -8192.0, 1e30, np.nan, np.inf], np.float32), (37, 61))
    for passes in (0, 1):
        s, info = hip_ops.contour_surface(torch.from_numpy(z).cuda(), 0.0, passes)
        ref_s, ref_info = contours_ref.surface(z, 0.0, passes)
        assert tuple(info.cpu().tolist()) == ref_info and ref_info[2] > 500 and np.array_equal(s.cpu().numpy(), ref_s)


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_any_launch():
    import torch
    lib = _lib.load()
    H, W = 6, 7
    n = H * W
    SENT = 77
    z = torch.zeros(H, W, device="cuda")
    s = torch.full((H, W), SENT, device="cuda", dtype=torch.int32)
    info = torch.full((3,), SENT, device="cuda", dtype=torch.int32)
    count = torch.full((H, W), SENT, device="cuda", dtype=torch.int32)
    need = lib.adamvs_contour_workspace_bytes(W, H)
    ws = torch.zeros(need, device="cuda", dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = _lib.ContourStats()
    lev = (ctypes.c_int * 3)(10, 20, 30)
    flat = (ctypes.c_int * 3)(10, 20, 20)
    big = (ctypes.c_int * (_lib.CONTOUR_MAX_LEVELS + 1))(*range(_lib.CONTOUR_MAX_LEVELS + 1))
    surface = lambda W_=W, H_=H, z_=p(z), zr=0.0, ps=1, w=p(ws), wb=need, s_=p(s), i_=p(info): \
        lib.adamvs_contour_surface(W_, H_, z_, zr, ps, w, wb, s_, i_, None)
    assert surface(z_=None) < 0 and surface(w=None) < 0 and surface(s_=None) < 0 and surface(i_=None) < 0
    assert surface(W_=0) < 0 and surface(H_=-1) < 0 and surface(W_=1 << 15, H_=1 << 15) < 0
    assert surface(ps=-1) < 0 and surface(ps=3) < 0 and surface(zr=float("nan")) < 0
    assert surface(wb=need - 1) < 0 and surface(s_=p(z)) < 0 and surface(s_=ctypes.c_void_p(ws.data_ptr() + 256)) < 0
    cnt = lambda W_=W, H_=H, s_=p(s), K=3, l=lev, w=p(ws), wb=need, c=p(count), st_=ctypes.byref(st): \
        lib.adamvs_contour_count(W_, H_, s_, K, l, w, wb, c, st_, None)
    assert cnt(s_=None) < 0 and cnt(l=None) < 0 and cnt(w=None) < 0 and cnt(c=None) < 0 and cnt(st_=None) < 0
    assert cnt(W_=0) < 0 and cnt(K=-1) < 0 and cnt(K=_lib.CONTOUR_MAX_LEVELS + 1, l=big) < 0 and cnt(l=flat) < 0
    assert cnt(wb=need - 1) < 0 and cnt(c=p(s)) < 0
    seg5 = [torch.full((4,), SENT, device="cuda", dtype=torch.int32) for _ in range(5)]
    segs = lambda N=4, K=3, l=lev, w=p(ws), wb=need, a=None: \
        lib.adamvs_contour_segments(W, H, p(s), K, l, N, w, wb, *(a if a is not None else [p(t) for t in seg5]), None)
    assert segs(N=-1) < 0 and segs(N=1 << 31) < 0 and segs(l=flat) < 0 and segs(wb=need - 1) < 0 and segs(w=None) < 0
    assert segs(a=[None] + [p(t) for t in seg5[1:]]) < 0 and segs(a=[p(seg5[0])] * 2 + [p(t) for t in seg5[2:]]) < 0
    need2 = lib.adamvs_contour_rank_workspace_bytes(4)
    assert lib.adamvs_contour_rank_workspace_bytes(-1) < 0 and lib.adamvs_contour_rank_workspace_bytes(1 << 31) < 0
    assert lib.adamvs_contour_workspace_bytes(0, 5) < 0 and lib.adamvs_contour_workspace_bytes(1 << 15, 1 << 15) < 0
    ws2 = torch.zeros(need2, device="cuda", dtype=torch.uint8)
    closed = torch.full((4,), SENT, device="cuda", dtype=torch.uint8)
    rank = lambda N=4, pr=p(seg5[4]), w=p(ws2), wb=need2, a=p(seg5[0]), b=p(seg5[1]), c=p(closed), st_=ctypes.byref(st): \
        lib.adamvs_contour_rank(N, pr, w, wb, a, b, c, st_, None)
    assert rank(N=-1) < 0 and rank(pr=None) < 0 and rank(w=None) < 0 and rank(a=None) < 0 and rank(c=None) < 0 and rank(st_=None) < 0
    assert rank(wb=need2 - 1) < 0 and rank(a=p(seg5[4])) < 0
    out = dict(first=torch.full((3,), SENT, device="cuda", dtype=torch.int64), lstart=torch.full((2,), SENT, device="cuda", dtype=torch.int32),
               llevel=torch.full((2,), SENT, device="cuda", dtype=torch.int32), lclosed=torch.full((2,), SENT, device="cuda", dtype=torch.uint8),
               vertex=torch.full((6, 3), SENT, device="cuda", dtype=torch.int64))
    more = [torch.full((4,), SENT, device="cuda", dtype=torch.int32) for _ in range(2)]
    def lines(N=4, M=2, K=3, l=lev, w=p(ws2), wb=need2, first=p(out["first"]), vertex=p(out["vertex"]), entry=p(seg5[0])):
        return lib.adamvs_contour_lines(W, H, p(s), K, l, N, M, entry, p(seg5[1]), p(seg5[2]), p(seg5[3]), p(more[0]), p(more[1]), p(closed),
                                        w, wb, first, p(out["lstart"]), p(out["llevel"]), p(out["lclosed"]), vertex, None)
    assert lines(M=-1) < 0 and lines(M=5) < 0 and lines(M=0) < 0 and lines(N=-1) < 0 and lines(l=flat) < 0 and lines(K=-1) < 0
    assert lines(w=None) < 0 and lines(wb=need2 - 1) < 0 and lines(first=None) < 0 and lines(vertex=None) < 0 and lines(entry=None) < 0
    assert lines(vertex=p(out["first"])) < 0
    torch.cuda.synchronize()
    for t in [s, info, count, closed] + seg5 + more + list(out.values()):
        assert bool((t == SENT).all())                                   # nothing was written: every call returned before a launch
    assert not bool(ws.any()) and not bool(ws2.any())
