"""DSM rasterisation, host side (no GPU): the grid, world files, raster files, the streamed PLY, the key order of the fp64
restatement (tests/dsm_ref.py) and argument errors of the C ABI."""
import ctypes
import math

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, dsm, fusion
from conftest import ROOT  # noqa: F401
from dsm_ref import cells, order, restate, unorder


def _inside(grid, pts):
    used, _, _ = cells(grid, np.array([[x, y, grid.z_ref] for x, y in pts]))
    return used


# ---- grid ----------------------------------------------------------------------------------------------------------------
def test_grid_from_bounds():
    g = dsm.grid_for_bounds((2.3, 7.6), (10.1, 11.9), 0.5, 3.0)
    assert g == dsm.Grid(2.0, 12.0, 0.5, 3.0, 17, 9)
    # negative coordinates: floor, not truncation
    g = dsm.grid_for_bounds((-3.3, -2.1), (-0.2, -0.6), 0.25, -4.0)
    assert g == dsm.Grid(-3.5, -0.5, 0.25, -4.0, 14, 7)
    assert _inside(g, [(-3.3, -2.1), (-0.2, -0.6), (-3.3, -0.6), (-0.2, -2.1)]).all()
    # far from the origin, as WHU-OMVS coordinates are
    g = dsm.grid_for_bounds((512345.37, 3401234.11), (512545.0, 3401434.0), 0.25, 812.0)
    assert (g.x0, g.y_top, g.W, g.H) == (512345.25, 3401434.25, 800, 801)
    # bounds on exact cell edges: lo.x starts column 0; hi.y on an edge falls in row 1 (row j holds y_top - (j+1) gsd < y <=
    # y_top - j gsd), so the top row stays empty; hi.x on an edge opens a last column of its own
    g = dsm.grid_for_bounds((-1.0, -2.0), (1.0, 2.0), 0.25, 0.0)
    assert g == dsm.Grid(-1.0, 2.25, 0.25, 0.0, 9, 18)
    used, cell, _ = cells(g, np.array([[-1.0, 2.0, 0.0], [1.0, -2.0, 0.0]]))
    assert used.all() and list(cell) == [1 * 9 + 0, 17 * 9 + 8]


def test_grid_bound_points_stay_inside_where_the_division_rounds_up():
    # -127.70000000000002 / 0.1 rounds to -1277.0, but x0 = -1277 * 0.1 = -127.7 lies right of the point: the grid widens
    lx = -127.70000000000002
    assert math.floor(lx / 0.1) * 0.1 > lx
    g = dsm.grid_for_bounds((lx, 0.0), (-120.0, 5.0), 0.1, 0.0)
    assert g.x0 == math.floor(lx / 0.1) * 0.1 - 0.1
    assert _inside(g, [(lx, 0.0), (-120.0, 5.0)]).all()
    rng = np.random.default_rng(0)
    for gsd in (0.1, 0.16, 0.25, 0.3, 0.7):
        k = rng.integers(-5000, 5000, 200)
        for kx in k:
            for lo in (math.nextafter(kx * gsd, -math.inf), kx * gsd, math.nextafter(kx * gsd, math.inf)):
                g = dsm.grid_for_bounds((lo, lo), (lo + 3.0, lo + 3.0), gsd, 0.0)
                assert _inside(g, [(lo, lo), (lo + 3.0, lo + 3.0), (lo, lo + 3.0), (lo + 3.0, lo)]).all(), (gsd, lo, g)


def test_grid_refusals():
    with pytest.raises(ValueError, match="cap"):
        dsm.grid_for_bounds((0.0, 0.0), (1e5, 1e5), 1.0, 0.0)
    g = dsm.grid_for_bounds((0.0, 0.0), (16383.0, 16382.5), 1.0, 0.0)
    assert (g.W, g.H) == (16384, 16384)                                                      # 2^28 cells: the cap itself
    for gsd in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gsd"):
            dsm.grid_for_bounds((0.0, 0.0), (1.0, 1.0), gsd, 0.0)
    with pytest.raises(ValueError, match="exceed"):
        dsm.grid_for_bounds((2.0, 0.0), (1.0, 1.0), 0.5, 0.0)
    with pytest.raises(ValueError, match="finite"):
        dsm.grid_for_bounds((0.0, float("nan")), (1.0, 1.0), 0.5, 0.0)


def test_world_file_text():
    g = dsm.Grid(512345.25, 3401434.25, 0.25, 812.0, 800, 801)
    assert dsm.world_file_text(g) == "0.25\n0.0\n0.0\n-0.25\n512345.375\n3401434.125\n"
    g = dsm.Grid(-3.5, -0.5, 0.1, 0.0, 3, 3)
    lines = dsm.world_file_text(g).splitlines()
    assert len(lines) == 6 and [float(v) for v in lines] == [0.1, 0.0, 0.0, -0.1, -3.5 + 0.05, -0.5 - 0.05]


def test_raster_files_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    H, W = 13, 21
    d = rng.normal(100.0, 30.0, (H, W)).astype(np.float32)
    d[rng.random((H, W)) < 0.2] = np.nan
    cnt = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    cnt[0, :3] = (0, 65535, 1)
    rgba = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    g = dsm.Grid(-3.5, 7.0, 0.5, 90.0, W, H)
    res = dict(dsm=d, count=cnt, rgba=rgba, grid=g, mode="mean", min_count=2, points_read=11, points_used=7, cells_filled=5)
    out = str(tmp_path / "sub" / "area")
    paths = dsm.write_outputs(out, res)
    a, b, c = dsm.read_outputs(out)
    assert a.dtype == np.float32 and a.tobytes() == d.tobytes()          # NaN payloads included
    assert b.dtype == np.uint16 and np.array_equal(b, cnt)
    assert np.array_equal(c, rgba)
    for k in ("dsm_world", "count_world", "ortho_world"):
        assert open(paths[k]).read() == dsm.world_file_text(g)
    import json
    meta = json.load(open(paths["json"]))
    assert meta == dict(grid=dict(x0=-3.5, y_top=7.0, gsd=0.5, W=W, H=H), z_ref=90.0, mode="mean", min_count=2, points_read=11,
                        points_used=7, cells_filled=5)
    first = {k: open(p, "rb").read() for k, p in paths.items()}
    dsm.write_outputs(out, res)
    assert all(open(p, "rb").read() == first[k] for k, p in paths.items())


# ---- the streamed PLY ----------------------------------------------------------------------------------------------------
def test_ply_chunks_equal_read_ply(tmp_path):
    rng = np.random.default_rng(2)
    path = str(tmp_path / "c.ply")
    n = 1000
    with fusion.PlyWriter(path) as w:
        w.write(rng.normal(size=(n, 3)) * 1e6, rng.integers(0, 256, (n, 3)).astype(np.uint8))
    whole = fusion.read_ply(path)
    for chunk in (1, 7, 999, 1000, 4096):
        parts = list(dsm.ply_chunks(path, chunk))
        assert [len(p[0]) for p in parts] == [min(chunk, n - s) for s in range(0, n, chunk)]
        xyz = np.concatenate([p[0] for p in parts])
        rgb = np.concatenate([p[1] for p in parts])
        assert xyz.dtype == np.float64 and rgb.dtype == np.uint8
        assert np.array_equal(xyz, np.stack([whole["x"], whole["y"], whole["z"]], 1))
        assert np.array_equal(rgb, np.stack([whole["red"], whole["green"], whole["blue"]], 1))
    empty = str(tmp_path / "e.ply")
    fusion.PlyWriter(empty).close()
    assert list(dsm.ply_chunks(empty, 10)) == []
    bad = str(tmp_path / "b.ply")
    open(bad, "wb").write(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="binary_little_endian"):
        list(dsm.ply_chunks(bad, 10))


# ---- the restatement -----------------------------------------------------------------------------------------------------
def test_key_order_is_monotone():
    big = np.float32(65536.0)
    v = np.array([-big, np.nextafter(-big, np.float32(0)), -65535.5, -1.0, -1e-30, -1e-45, -0.0, 0.0, 1e-45, 1e-30, 0.5, 1.0,
                  65535.99, np.nextafter(big, np.float32(0)), big], np.float32)
    o = order(v)
    assert (np.diff(o.astype(np.int64)) >= 0).all()
    # strictly increasing except at -0 / +0, which are one height
    assert o[6] == o[7] and (np.diff(o.astype(np.int64))[np.arange(len(v) - 1) != 6] > 0).all()
    assert (o >= 0x00800000).all()                            # a used point's key is never 0
    assert np.array_equal(unorder(o), np.where(v == 0, np.float32(0), v))
    rng = np.random.default_rng(3)
    h = np.sort(rng.uniform(-65536, 65536, 100000).astype(np.float32))
    assert (np.diff(order(h).astype(np.int64)) >= 0).all()
    assert np.array_equal(np.diff(order(h).astype(np.int64)) > 0, np.diff(h) > 0)


def test_restatement_by_hand():
    g = dsm.Grid(0.0, 2.0, 1.0, 100.0, 2, 2)
    xyz = np.array([[0.5, 1.5, 101.0], [0.7, 1.2, 103.0], [0.2, 1.9, 103.0],      # cell (0, 0): a tie at 103, the first wins
                    [1.5, 0.5, 99.0], [1.5, 0.5, 100.5],                          # cell (1, 1)
                    [1.5, 1.5, 100.0 + 65536.0], [np.nan, 1.5, 100.0], [2.0, 0.5, 100.0],   # refused: height, NaN, x = x0 + W gsd
                    [0.5, 0.5, 100.0 - 65535.0]], np.float64)                     # cell (0, 1): just inside the height range
    rgb = np.arange(27, dtype=np.uint8).reshape(9, 3)
    r = restate(g, xyz, rgb, "max")
    assert list(r["used"]) == [True] * 5 + [False] * 3 + [True]
    assert np.array_equal(r["count"], [[3, 0], [1, 2]])
    assert r["dsm"][0, 0] == 103.0 and r["dsm"][1, 1] == np.float32(100.5) and r["dsm"][1, 0] == 100.0 - 65535.0
    assert np.isnan(r["dsm"][0, 1])
    assert list(r["rgba"][0, 0]) == [3, 4, 5, 255] and list(r["rgba"][1, 1]) == [12, 13, 14, 255] and list(r["rgba"][0, 1]) == [0] * 4
    m = restate(g, xyz, rgb, "mean", min_count=2)
    assert m["dsm"][0, 0] == np.float32((101.0 + 103.0 + 103.0) / 3) and m["dsm"][1, 1] == np.float32(99.75)
    assert np.isnan(m["dsm"][1, 0]) and list(m["rgba"][1, 0]) == [0] * 4 and m["count"][1, 0] == 1
    assert list(m["rgba"][0, 0]) == [3, 4, 5, 255]


# ---- C ABI argument errors -----------------------------------------------------------------------------------------------
def test_dsm_argument_errors_without_a_gpu():
    lib = _lib.load()
    dummy = ctypes.c_void_p(16)            # never dereferenced: every call below is refused before a launch
    null = ctypes.c_void_p(0)

    def grid(**kw):
        g = _lib.DsmGrid()
        g.x0, g.y_top, g.gsd, g.z_ref, g.W, g.H = 0.0, 10.0, 0.5, 0.0, 20, 20
        for k, v in kw.items():
            setattr(g, k, v)
        return ctypes.byref(g)

    def acc(g=None, xyz=dummy, n=10, seq0=0, mode=0, key=dummy, count=dummy, sum_=dummy):
        return lib.adamvs_dsm_accumulate(grid() if g is None else g, xyz, n, seq0, mode, key, count, sum_, null)

    def claim(g=None, xyz=dummy, rgb=dummy, n=10, seq0=0, color=dummy):
        return lib.adamvs_dsm_claim(grid() if g is None else g, xyz, rgb, n, seq0, dummy, color, null)

    def fin(g=None, mode=0, min_count=1, dsm_=dummy, sum_=dummy):
        return lib.adamvs_dsm_finalize(grid() if g is None else g, dummy, dummy, sum_, dummy, mode, min_count, dsm_, dummy, dummy, null)

    nan, inf = float("nan"), float("inf")
    cases = {
        "null grid": acc(g=ctypes.POINTER(_lib.DsmGrid)()), "null xyz": acc(xyz=null), "null key": acc(key=null),
        "null count": acc(count=null), "null sum in mean mode": acc(mode=1, sum_=null), "n < 0": acc(n=-1),
        "seq0 < 0": acc(seq0=-1), "seq0 + n > 2^32": acc(seq0=(1 << 32) - 9), "n > 2^32": acc(n=(1 << 32) + 1),
        "gsd 0": acc(g=grid(gsd=0.0)), "gsd < 0": acc(g=grid(gsd=-0.5)), "gsd NaN": acc(g=grid(gsd=nan)), "gsd inf": acc(g=grid(gsd=inf)),
        "x0 NaN": acc(g=grid(x0=nan)), "z_ref inf": acc(g=grid(z_ref=-inf)), "W 0": acc(g=grid(W=0)), "H < 0": acc(g=grid(H=-2)),
        "cells over the cap": acc(g=grid(W=1 << 14, H=(1 << 14) + 1)), "mode 2": acc(mode=2), "mode -1": acc(mode=-1),
        "claim null rgb": claim(rgb=null), "claim null color": claim(color=null), "claim n < 0": claim(n=-5),
        "claim seq0 + n > 2^32": claim(seq0=1 << 32, n=1), "claim gsd NaN": claim(g=grid(gsd=nan)), "claim W 0": claim(g=grid(W=0)),
        "finalize min_count 0": fin(min_count=0), "finalize min_count < 0": fin(min_count=-3), "finalize mode 7": fin(mode=7),
        "finalize null dsm": fin(dsm_=null), "finalize null sum in mean mode": fin(mode=1, sum_=null),
        "finalize H 0": fin(g=grid(H=0)), "finalize gsd inf": fin(g=grid(gsd=inf)),
    }
    for what, rc in cases.items():
        assert rc < 0, what
        with pytest.raises(_lib.AdaMVSHipError, match="invalid argument"):
            _lib.check(rc, what)


def test_wrappers_refuse_host_tensors():
    import torch
    from ada_mvs_amd import hip_ops
    g = dsm.Grid(0.0, 4.0, 1.0, 0.0, 4, 4)
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        hip_ops.dsm_accumulate(g, torch.zeros(5, 3, dtype=torch.float64), 0, 0, torch.zeros(16, dtype=torch.int64),
                               torch.zeros(16, dtype=torch.int32))
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        hip_ops.dsm_finalize(g, torch.zeros(16, dtype=torch.int64), torch.zeros(16, dtype=torch.int32), None,
                             torch.zeros(16, dtype=torch.int32), 0, 1)
