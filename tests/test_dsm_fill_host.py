"""DSM gap fill, host side (no GPU): the fp64 reference (tests/dsm_fill_ref.py) on cases solved by hand, argument errors of the
C ABI, the wrapper's refusal of host tensors, and the fill files."""
import ctypes
import json

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, dsm
from dsm_fill_ref import INT32_MAX, dist2_brute, dist2_separable, fill_ref


def blank(H, W):
    return np.full((H, W), np.nan, np.float32), np.zeros((H, W, 4), np.uint8)


# ---- the reference on cases solved by hand ----------------------------------------------------------------------------------
def test_a_one_dimensional_gap_is_filled_linearly():
    d, rgba = blank(1, 9)
    d[0, 0], d[0, 8] = 2.0, 10.0
    rgba[0, 0], rgba[0, 8] = (0, 80, 255, 255), (160, 0, 255, 255)
    ref = fill_ref(d, rgba, 4.0)
    assert np.allclose(ref["u"][0], np.arange(2.0, 11.0), atol=1e-12)
    assert ref["rgba"][0, 4].tolist() == [80, 40, 255, 255]
    assert ref["filled"][0].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 0] and ref["cells_filled"] == 7


def test_a_gap_at_the_grid_edge_takes_the_last_valid_value():
    d, rgba = blank(1, 7)
    d[0, :3] = (1.0, 2.0, 4.5)                   # zero flux across the edge: the slope of the valid cells is not continued
    assert np.allclose(fill_ref(d, rgba, 10.0)["u"][0, 3:], 4.5, atol=1e-12)
    d, rgba = blank(5, 8)
    d[:, 2] = 6.25
    d[1:4, 0] = 6.25
    ref = fill_ref(d, rgba, 10.0)
    assert ref["cells_filled"] == 5 * 8 - 5 - 3 and np.allclose(ref["u"][ref["filled"] == 1], 6.25, atol=1e-12)


@pytest.mark.parametrize("field", ["linear", "i2-j2", "ij"])
def test_discrete_harmonic_fields_are_reproduced(field):
    H, W = 30, 34
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    u = {"linear": 0.7 * i - 1.3 * j + 4.0, "i2-j2": (i * i - j * j) / 10.0, "ij": i * j / 9.0}[field]
    d = u.astype(np.float32)
    holes = ((i - 12) ** 2 + (j - 15) ** 2 <= 36) | ((i > 22) & (i < 27) & (j > 3) & (j < 30))
    d[holes] = np.nan
    ref = fill_ref(d, np.zeros((H, W, 4), np.uint8), 8.0)
    # the boundary values are fp32 roundings of u: the harmonic fill of the rounded values differs by at most their error
    bound = np.abs(d[~holes].astype(np.float64) - u[~holes]).max()
    assert (ref["filled"] == holes).all()
    assert np.abs(ref["u"][holes] - u[holes]).max() <= bound + 1e-9


def test_the_3_4_5_boundary():
    d, rgba = blank(9, 9)
    d[0, 0] = 1.0
    assert fill_ref(d, rgba, 5.0)["filled"][3, 4] == 1
    r = fill_ref(d, rgba, 4.999)
    assert r["filled"][3, 4] == 0 and r["dist2"][3, 4] == INT32_MAX
    assert fill_ref(d, rgba, 5.0)["dist2"][3, 4] == 25


def test_the_two_distance_forms_agree():
    rng = np.random.default_rng(0)
    for H, W in ((1, 1), (1, 17), (19, 1), (21, 26), (33, 40)):
        for p in (0.0, 0.03, 0.3, 1.0):
            valid = rng.random((H, W)) < p
            for r in (0.5, 1.0, 1.5, 3.0, 7.3):
                assert np.array_equal(dist2_brute(valid, r), dist2_separable(valid, r)), (H, W, p, r)


def test_the_cg_path_matches_the_direct_solve():
    import dsm_fill_ref as R
    rng = np.random.default_rng(1)
    d = (50.0 + rng.normal(size=(40, 45))).astype(np.float32)
    d[10:30, 8:38] = np.nan
    rgba = rng.integers(0, 256, (40, 45, 4)).astype(np.uint8)
    direct = fill_ref(d, rgba, 12.0)
    old = R.DIRECT_MAX
    try:
        R.DIRECT_MAX = 10
        cg = fill_ref(d, rgba, 12.0)
    finally:
        R.DIRECT_MAX = old
    assert np.abs(direct["u"] - cg["u"]).max() <= 1e-8


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_dsm_fill_argument_errors_without_a_gpu():
    lib = _lib.load()
    dummy = ctypes.c_void_p(256)               # never dereferenced: every call below is refused before a launch
    null = ctypes.c_void_p(0)
    W, H = 20, 10
    need = lib.adamvs_dsm_fill_workspace_bytes(W, H)
    assert need > 0 and need % 256 == 0
    stats = _lib.DsmFillStats()

    def fill(W=W, H=H, dsm_=dummy, rgba=dummy, r=3.0, th=1e-6, tc=1e-3, cycles=10, ws=dummy, wsb=need, out=dummy, rgba_out=dummy,
             dist2=dummy, filled=dummy, st=True):
        return lib.adamvs_dsm_fill(W, H, dsm_, rgba, r, th, tc, cycles, ws, wsb, out, rgba_out, dist2, filled,
                                   ctypes.byref(stats) if st else ctypes.POINTER(_lib.DsmFillStats)(), null)

    nan, inf = float("nan"), float("inf")
    cases = {
        "null dsm": fill(dsm_=null), "null rgba": fill(rgba=null), "null workspace": fill(ws=null), "null dsm_out": fill(out=null),
        "null rgba_out": fill(rgba_out=null), "null dist2": fill(dist2=null), "null filled": fill(filled=null), "null stats": fill(st=False),
        "W 0": fill(W=0), "H < 0": fill(H=-1), "cells over the cap": fill(W=1 << 14, H=(1 << 14) + 1),
        "r NaN": fill(r=nan), "r inf": fill(r=inf), "r 0": fill(r=0.0), "r < 0": fill(r=-2.0), "r over the cap": fill(r=1024.5),
        "tol_height 0": fill(th=0.0), "tol_height NaN": fill(th=nan), "tol_colour < 0": fill(tc=-1e-3), "tol_colour inf": fill(tc=inf),
        "max_cycles 0": fill(cycles=0), "max_cycles < 0": fill(cycles=-4), "workspace too small": fill(wsb=need - 1),
        "workspace query W 0": lib.adamvs_dsm_fill_workspace_bytes(0, 5),
        "workspace query over the cap": lib.adamvs_dsm_fill_workspace_bytes(1 << 15, 1 << 14),
    }
    for what, rc in cases.items():
        assert rc < 0, what
        with pytest.raises(_lib.AdaMVSHipError, match="invalid argument"):
            _lib.check(int(rc), what)
    assert lib.adamvs_dsm_fill_workspace_bytes(1 << 14, 1 << 14) > 60 * (1 << 28)


def test_wrapper_refuses_host_tensors():
    import torch
    from ada_mvs_amd import hip_ops
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        hip_ops.dsm_fill(torch.zeros(4, 5), torch.zeros(4, 5, 4, dtype=torch.uint8), 2.0)


def test_fill_radius_refusals():
    assert dsm.fill_radius_cells(3.0, 0.25) == 12.0
    for m, gsd in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (1025.0, 1.0), (300.0, 0.25)):
        with pytest.raises(ValueError, match="fill_max_dist"):
            dsm.fill_radius_cells(m, gsd)
    for r in (0.0, -1.0, float("nan"), 1024.5):
        with pytest.raises(ValueError, match="fill radius"):
            dsm.fill_gaps(np.zeros((2, 2), np.float32), np.zeros((2, 2, 4), np.uint8), r)


# ---- files ------------------------------------------------------------------------------------------------------------------
def test_fill_output_paths_are_disjoint_from_the_dsm_files():
    a, b = dsm.output_paths("/x/area"), dsm.fill_output_paths("/x/area")
    assert not set(a.values()) & set(b.values())
    assert set(b) == {"dsm", "dsm_world", "ortho", "ortho_world", "filled", "filled_world", "json"}
    assert b["dsm"] == "/x/area_dsm_filled.tif" and b["ortho"] == "/x/area_ortho_filled.png" and b["filled"] == "/x/area_filled.png"
    assert b["json"] == "/x/area_fill.json"


def test_fill_files_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    H, W = 11, 17
    d = rng.normal(100.0, 30.0, (H, W)).astype(np.float32)
    d[rng.random((H, W)) < 0.2] = np.nan
    rgba = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    filled = (rng.random((H, W)) < 0.3).astype(np.uint8)
    g = dsm.Grid(-3.5, 7.0, 0.5, 90.0, W, H)
    fill = dict(dsm=d, rgba=rgba, filled=filled, dist2=np.zeros((H, W), np.int32), cycles=7, residual_height=3.5e-7,
                residual_colour=2e-4, cells_valid=100, cells_filled=40, cells_empty=47, seconds=0.25, max_dist=2.0, gsd=0.5, r_cells=4.0)
    out = str(tmp_path / "sub" / "area")
    paths = dsm.write_fill_outputs(out, g, fill)
    a, b, c = dsm.read_fill_outputs(out)
    assert a.dtype == np.float32 and a.tobytes() == d.tobytes()
    assert np.array_equal(b, rgba) and np.array_equal(c, filled)
    for k in ("dsm_world", "ortho_world", "filled_world"):
        assert open(paths[k]).read() == dsm.world_file_text(g)
    meta = json.load(open(paths["json"]))
    assert meta == dict(max_dist=2.0, gsd=0.5, r_cells=4.0, cells_valid=100, cells_filled=40, cells_empty=47, cycles=7,
                        residual_height=3.5e-7, residual_colour=2e-4, seconds=0.25)
    assert set(paths.values()) == set(dsm.fill_output_paths(out).values())
