"""Roof planes on the GPU (csrc/dsm_roofs.hip through hip_ops and ada_mvs_amd/roofs.py) against the numpy / Python-integer
restatement (tests/roofs_ref.py): the link bytes, parent, segments and S, every column of the moments, the grown labels and the
per-round counts, the merged labels and the residual table for exact equality, at every edge of the tiles, of the stride and of
the border rounds; the scenes, a shifted scene, run-to-run identity, growth stopped early against all rounds, argument errors
and roofs_whu.py end to end.  There is no tolerance and no cell is left out."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, dsm, roofs
from conftest import ROOT
import roofs_ref as R

pytestmark = pytest.mark.gpu

T = _lib.BLD_TILE_W
assert T == _lib.BLD_TILE_H == 64


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True), (what, np.argwhere(got != want)[:10])


def gpu_segments(link):
    """-> (parent, segments, S, stats) through adamvs_roof_label."""
    import torch
    from ada_mvs_amd import hip_ops
    seg, S, parent, st = hip_ops.roof_label(torch.from_numpy(np.ascontiguousarray(link, np.uint8)).cuda())
    assert st.converged == 1 and st.tiles == -(-link.shape[0] // T) * -(-link.shape[1] // T)
    assert st.pairs == link.shape[0] * (-(-link.shape[1] // T) - 1) + link.shape[1] * (-(-link.shape[0] // T) - 1)
    assert 0 <= st.rounds < _lib.BLD_MAX_ROUNDS
    return parent.cpu().numpy(), seg.cpu().numpy(), S, st


def check_segments(link):
    parent, seg, S = R.segments_ref(link)
    gp, gs, gS, st = gpu_segments(link)
    same(gp, parent, "parent")
    same(gs, seg, "segments")
    assert gS == S
    return seg, S, st


def check_stage(z, b, gsd, **kw):
    """extract() equals the restatement at every step.  -> (got, ref)"""
    ref = R.run_ref(z, b, gsd, **kw)
    got = roofs.extract(z, b, gsd, **kw)
    assert (got["params"]["stride"], got["params"]["g_tol"], got["z_ref"], got["params"]["grow_rounds"]) == (ref["s"], ref["g_tol"], ref["z_ref"],
                                                                                                       ref["rounds"])
    same(got["link"], ref["link"], "link")
    same(got["parent"], ref["parent"], "parent")
    same(got["segments"], ref["segments"], "segments")
    assert got["S"] == ref["S"]
    for k, name in enumerate(R.COLUMNS):
        same(got["segment_table"][k], ref["seg_table"][k], "segment moments " + name)
    same(got["keep"], ref["keep"], "keep")
    same(got["planes"], ref["planes"], "planes")
    same(got["seed"], ref["seed"], "seed")
    same(got["grown"], ref["grown"], "grown")
    same(got["grow_counts"], ref["counts"], "growth counts")
    for k, name in enumerate(R.COLUMNS):
        same(got["grown_table"][k], ref["grown_table"][k], "grown moments " + name)
    assert got["adjacency"] == ref["adjacency"]
    assert got["groups"] == ref["groups"] and got["R"] == ref["R"]
    same(got["label"], ref["label"], "label")
    for k, name in enumerate(R.COLUMNS):
        same(got["table"][k], ref["table"][k], "final moments " + name)
    same(got["final_planes"], ref["final_planes"], "final planes")
    same(got["residuals"], ref["residuals"], "residuals")
    assert [p["id"] for p in got["properties"]] == list(range(1, ref["R"] + 1)) == [p["id"] for p in got["polygons"]]
    assert [p["cells"] for p in got["properties"]] == ref["table"][0].tolist()
    return got, ref


# ---- the smallest shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (T + 1, 1), (1, T + 1), (3, 3)], ids=["1x1", "W1", "H1", "3x3"])
def test_smallest_shapes(H, W):
    rng = np.random.default_rng(H * 5 + W)
    z = (20.0 + rng.integers(0, 3, (H, W)) / 16.0).astype(np.float32)
    got, ref = check_stage(z, np.ones((H, W), np.int32), 1.0, smooth_tol=1.0)
    assert got["S"] == (1 if (H, W) == (3, 3) else 0)                   # a cell needs its four neighbours at the stride
    for bits in (0, 1, 7, 255):
        seg, S, st = check_segments(np.full((H, W), bits, np.uint8))
        assert S == (0 if bits == 0 else H * W if bits == 1 else 1) and st.rounds == (1 if S == 1 and max(H, W) > T else 0)
    check_segments(R.random_links(H, W, 0.6, seed=H + W))


@pytest.mark.parametrize("density", [0.3, 0.6, 0.9])
@pytest.mark.parametrize("edge", [-1, 0, 1, "2T+1"])
def test_random_link_bits_at_every_tile_edge(edge, density):
    n = 2 * T + 1 if edge == "2T+1" else T + edge
    for k, (H, W) in enumerate(((T + 7, n), (n, T + 7), (n, n))):
        _, S, _ = check_segments(R.random_links(H, W, density, seed=1000 * k + 10 * n + int(density * 100)))
        assert S > 0


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1])
def test_whole_stage_at_every_tile_edge(n):
    """One noisy gable over the whole grid, n rows of n and of n + 3 cells: the planes reach every edge of the grid, a run of
    equal labels ends with its row even where the next row goes on with the same label in the same wave, and rows start at
    every lane."""
    for W in (n, n + 3):
        i, j = np.mgrid[0:n, 0:W]
        z = (20.0 + 0.25 * np.abs(i - n // 2) + R._noise((n, W), 0.05, seed=n + W)).astype(np.float32)
        got, _ = check_stage(z, np.ones((n, W), np.int32), 0.5)
        assert got["R"] == 2 and got["counts"]["cells_unassigned"] == 0
        assert got["table"][13].tolist() == [0, 0] and got["table"][14].tolist() == [W - 1, W - 1] and got["table"][12, 1] == n - 1


# ---- the given patterns at 5T + 3 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.3, 0.6, 0.9])
def test_random_link_bits_over_many_tiles(density):
    n = 5 * T + 3
    _, S, st = check_segments(R.random_links(n, n, density, seed=int(density * 10)))
    assert S > 1 and st.pairs == 10 * n
    print("random links %.1f at %d^2: S = %d, %d border rounds" % (density, n, S, st.rounds))


# ---- a mask is a link raster with every edge present ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["T+1", "2T+1", "serpentine"])
def test_a_mask_as_link_bits_gives_the_building_labels(case):
    """The one labelling serves both stages: over a mask written as link bits (every bit set on the mask's cells, or exactly
    the bits of the edges that exist) adamvs_roof_label returns the label raster and the count of adamvs_bld_label over the
    mask as flags, and both are the flood fill of the mask."""
    import torch
    from ada_mvs_amd import hip_ops
    import buildings_ref as B
    if case == "serpentine":
        mask = B.serpentine_mask(2 * T + 3, 2 * T + 3)
    else:
        n = T + 1 if case == "T+1" else 2 * T + 1
        mask = B.random_mask_raster(n, n, 0.59, seed=n)[1] > 0
    want, N = B.components_ref(mask)
    label, got_N, _ = hip_ops.bld_label(torch.from_numpy(np.where(mask, 3, 0).astype(np.uint8)).cuda())
    same(label.cpu().numpy(), want, "building labels")
    assert got_N == N and N > 0
    exact = mask.astype(np.uint8)
    exact[:, :-1] |= (mask[:, :-1] & mask[:, 1:]).astype(np.uint8) * 2
    exact[:-1, :] |= (mask[:-1, :] & mask[1:, :]).astype(np.uint8) * 4
    for what, link in (("every bit", np.where(mask, 7, 0).astype(np.uint8)), ("the edges' bits", exact)):
        _, seg, S, _ = gpu_segments(link)
        same(seg, want, "segments of " + what)
        same(seg, label.cpu().numpy(), "segments against the building labels, " + what)
        assert S == got_N


@pytest.mark.parametrize("name", ["serpentine", "comb"])
def test_one_segment_across_every_tile_border(name, capsys):
    """Every cell is core and adjacent rows (columns) are separated by unlinked walls: a labelling that joined adjacent core cells
    would need no rounds at all; the links make one segment whose diameter is of the order of the cell count."""
    n = 5 * T + 3
    link = R.serpentine_links(n, n) if name == "serpentine" else R.comb_links(n, n)
    seg, S, st = check_segments(link)
    assert S == 1 and (seg == 1).all() and 0 < st.rounds < _lib.BLD_MAX_ROUNDS
    with capsys.disabled():
        print("\n%s links %d x %d: %d border rounds over %d pairs (cap %d)" % (name, n, n, st.rounds, st.pairs, _lib.BLD_MAX_ROUNDS))
    # the same cells without the bits that cross a wall: as many segments as rows (columns)
    walls = link.copy()
    if name == "serpentine":
        walls &= ~np.uint8(4)
    else:
        walls[0] &= ~np.uint8(2)
    _, S, _ = check_segments(walls)
    assert S == n


def test_checkerboard_of_links_needs_no_round():
    n = 2 * T + 1
    seg, S, st = check_segments(R.checkerboard_links(n, n))
    assert S == ((n + 1) // 2) ** 2 and st.rounds == 0 and st.pairs == 4 * n
    assert np.bincount(seg.reshape(-1))[1:].max() == 4


@pytest.mark.parametrize("shape", [(_lib.ROOF_MAX_SIDE, 2), (3, _lib.ROOF_MAX_SIDE)], ids=["32768x2", "3x32768"])
def test_the_longest_side(shape):
    _, S, st = check_segments(R.random_links(shape[0], shape[1], 0.7, seed=9))
    assert S > 1000 and st.tiles == 512


# ---- the stride -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 64])
def test_links_on_a_grid_just_larger_than_the_stride(s):
    """On (2 s + 1)^2 cells the centre alone can be core; on (2 s + 2) x (2 s + 3) a 2 x 3 block, with links inside it."""
    import torch
    from ada_mvs_amd import hip_ops
    for H, W in ((2 * s, 2 * s + 5), (2 * s + 1, 2 * s + 1), (2 * s + 2, 2 * s + 3)):
        i, j = np.mgrid[0:H, 0:W]
        z = (30.0 + (j + 2 * i) / (8.0 * s)).astype(np.float32)
        b = np.ones((H, W), np.int32)
        want = R.links_ref(z, b, s, 0.2, 0.3, 0.1)
        got = hip_ops.roof_links(torch.from_numpy(z).cuda(), torch.from_numpy(b).cuda(), s, 0.2, 0.3, 0.1).cpu().numpy()
        same(got, want, "link")
        core = np.zeros((H, W), bool)
        core[s:H - s, s:W - s] = True
        assert np.array_equal(got & 1 > 0, core)
        if (H, W) == (2 * s + 2, 2 * s + 3):
            assert got[s:s + 2, s:s + 3].tolist() == [[7, 7, 5], [3, 3, 1]]
    check_stage(z, b, 1.0 / s if s > 1 else 1.0, smooth_span=1.0, min_plane_area=0.0)


def test_link_thresholds_are_inclusive_and_in_fp64():
    """One row band of 3 x 9 cells, s = 1: the middle row is core where the second difference is <= smooth_tol."""
    import torch
    from ada_mvs_amd import hip_ops
    z = np.zeros((3, 9), np.float32)
    z[1] = [0.0, 0.0, 0.125, 0.0, 0.0, 0.0, 0.5, 0.5 + 0.25, 1.0]
    b = np.ones((3, 9), np.int32)
    for tol in (0.25, np.nextafter(0.25, 0.0), 0.5, 0.1):
        for g_tol, step_tol in ((0.3, 0.1), (0.125, 0.0625), (0.0, 0.0), (10.0, 10.0)):
            want = R.links_ref(z, b, 1, tol, g_tol, step_tol)
            got = hip_ops.roof_links(torch.from_numpy(z).cuda(), torch.from_numpy(b).cuda(), 1, tol, g_tol, step_tol).cpu().numpy()
            same(got, want, "link")
    # float32(0.1) lies above 0.1: the comparison is made on the widened value
    z = np.zeros((3, 3), np.float32)
    z[1, 1] = np.float32(-0.05)
    got = hip_ops.roof_links(torch.from_numpy(z).cuda(), torch.from_numpy(b[:, :3].copy()).cuda(), 1, 0.1, 0.3, 0.1).cpu().numpy()
    assert float(np.float32(0.05)) * 2 > 0.1 and got[1, 1] == 0 == R.links_ref(z, b[:, :3], 1, 0.1, 0.3, 0.1)[1, 1]


# ---- the scenes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [0.0, 0.05, 0.1])
def test_four_roofs(noise, capsys):
    z, b, truth = R.four_roofs(noise, seed=0)
    got, ref = check_stage(z, b, 0.5, grow_rounds=12)
    assert got["R"] == 9 and got["per_building"] == {"1": 2, "2": 4, "3": 2, "4": 1}
    assert got["counts"]["cells_unassigned"] <= 0.01 * got["counts"]["building_cells"]
    with capsys.disabled():
        print("\nfour roofs +-%g m: %s, %d border rounds, growth %s" % (noise, got["counts"], got["label_stats"]["rounds"], got["grow_stats"]))
    for p in got["properties"]:
        assert 0.0 <= p["rms_m"] <= 0.1 and p["inlier_fraction"] > 0.9 and p["height_min"] <= p["plane"]["z0"] <= p["height_max"]
        assert (p["kind"] == "flat") == (p["building"] == 3) and (p["aspect_deg"] is None) == (p["building"] == 3)
    if noise == 0.0:
        assert sorted(round(p["aspect_deg"]) for p in got["properties"] if p["building"] == 2) == [0, 90, 180, 270]
        assert [round(p["aspect_deg"]) for p in got["properties"] if p["building"] == 4] == [270]


def test_defaults_and_the_merge_switched_off():
    z, b, _ = R.four_roofs(0.1, seed=3)
    got, _ = check_stage(z, b, 0.5)
    assert got["params"]["grow_rounds"] == 8 and got["R"] == 9
    off, _ = check_stage(z, b, 0.5, merge_rms=0.0)
    assert off["R"] == off["P"] > 9 and np.array_equal(off["label"], off["grown"]) and all(len(g) == 1 for g in off["groups"])


def test_dome():
    z, b = R.dome(0.02)
    got, _ = check_stage(z, b, 0.5)
    assert got["R"] >= 1 and max(p["rms_m"] for p in got["properties"]) > 0.05


def test_nan_holes():
    z, b, _ = R.four_roofs(0.05, seed=4)
    z = R.with_holes(z)
    got, _ = check_stage(z, b, 0.5)
    assert (got["label"][~np.isfinite(z)] == 0).all() and got["R"] >= 9
    z[:] = np.nan                                                       # nothing finite at all: z_ref 0, no plane
    got, _ = check_stage(z, b, 0.5)
    assert got["R"] == 0 and got["z_ref"] == 0.0 and got["properties"] == []


def test_building_on_the_grid_edge():
    z, b = R.on_the_edge()
    got, _ = check_stage(z, b, 0.5)
    assert got["per_building"] == {"1": 1, "2": 2}
    assert got["label"][0, 0] == 1 and got["label"][-1, -1] > 0          # grown out to the corner cells


def test_two_buildings_that_touch():
    z, b = R.touching()
    got, _ = check_stage(z, b, 0.5)
    assert got["per_building"] == {"1": 1, "2": 1}                        # one plane in the air, never linked, grown or merged across
    assert (got["label"][b == 1] == 1).all() and (got["label"][b == 2] == 2).all()
    one, _ = check_stage(z, (b > 0).astype(np.int32), 0.5)
    assert one["R"] == 1


def test_shifted_scene_gives_the_shifted_labels():
    z, b, _ = R.four_roofs(0.05, seed=5)
    H, W = z.shape
    canvas = lambda a, fill, di, dj: np.pad(a, ((di, 3 - di), (dj, 5 - dj)), constant_values=fill)
    a = roofs.extract(canvas(z, 10.0, 0, 0), canvas(b, 0, 0, 0), 0.5)
    c = roofs.extract(canvas(z, 10.0, 3, 5), canvas(b, 0, 3, 5), 0.5)
    assert a["R"] == c["R"] == 9
    for name in ("link", "segments", "seed", "grown", "label"):
        same(c[name][3:, 5:], a[name][:H, :W], name)
        assert not c[name][:3].any() and not c[name][:, :5].any()
    same(c["grow_counts"], a["grow_counts"], "growth counts")
    same(c["residuals"], a["residuals"], "residuals")
    for k in (0, 3, 9, 10, 15, 16, 17):                                   # n, sq, sqq, q_min, q_max, building do not move
        same(c["table"][k], a["table"][k], R.COLUMNS[k])
    same(c["table"][11] - 3, a["table"][11], "row_min")
    same(c["table"][13] - 5, a["table"][13], "col_min")


def test_run_to_run_identity():
    z, b, _ = R.four_roofs(0.1, seed=6)
    runs = [roofs.extract(z, b, 0.5) for _ in range(3)]
    for r in runs[1:]:
        for name in ("link", "parent", "segments", "segment_table", "planes", "seed", "grown", "grow_counts", "grown_table", "label", "table",
                     "final_planes", "residuals"):
            same(r[name], runs[0][name], name)
        assert r["adjacency"] == runs[0]["adjacency"] and r["properties"] == runs[0]["properties"] and r["polygons"] == runs[0]["polygons"]


def test_growth_stopped_early_equals_all_rounds():
    z, b, _ = R.four_roofs(0.0)
    ref = R.run_ref(z, b, 0.5, grow_rounds=40)
    early = roofs.extract(z, b, 0.5, grow_rounds=40)
    full = roofs.extract(z, b, 0.5, grow_rounds=40, stop_early=False)
    assert full["grow_stats"]["rounds_run"] == 40 and early["grow_stats"]["rounds_run"] == 8
    assert np.flatnonzero(ref["counts"] == 0)[0] == 6                     # the first round that labels nothing
    for r in (early, full):
        same(r["grown"], ref["grown"], "grown")
        same(r["grow_counts"], ref["counts"], "growth counts")
        same(r["label"], ref["label"], "label")
    # an odd and an even number of rounds end in different buffers
    for rounds in (0, 1, 2, 3, 5):
        got, _ = check_stage(z, b, 0.5, grow_rounds=rounds)
        assert got["grow_stats"]["rounds_run"] == rounds


# ---- argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_any_launch():
    import torch
    lib = _lib.load()
    H, W = 20, 30
    z = torch.full((H, W), 7.0, device="cuda")
    z2 = torch.full((H, W), 7.0, device="cuda")
    b = torch.ones(H, W, device="cuda", dtype=torch.int32)
    link = torch.zeros(H, W, device="cuda", dtype=torch.uint8)
    need = lib.adamvs_roof_workspace_bytes(W, H)
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    parent = torch.full((H, W), -7, device="cuda", dtype=torch.int32)
    l0 = torch.ones(H, W, device="cuda", dtype=torch.int32)
    l1 = torch.full((H, W), -7, device="cuda", dtype=torch.int32)
    counts = torch.full((_lib.ROOF_MAX_GROW,), -7, device="cuda", dtype=torch.int32)
    planes = torch.zeros(1, 3, device="cuda", dtype=torch.float64)
    table = torch.full((18, 1), -7, device="cuda", dtype=torch.int64)
    rtab = torch.full((2, 1), -7, device="cuda", dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nan, inf = float("nan"), float("inf")

    lk = lambda **kw: [kw.get("W", W), kw.get("H", H), kw.get("dsm", p(z)), kw.get("bld", p(b)), kw.get("s", 1), kw.get("t0", 0.2), kw.get("t1", 0.3),
                       kw.get("t2", 0.1), kw.get("link", p(link)), None]
    for kw in (dict(W=0), dict(H=-1), dict(W=32769, H=1), dict(dsm=None), dict(bld=None), dict(link=None), dict(s=0), dict(s=65), dict(t0=nan),
               dict(t1=-0.1), dict(t2=inf), dict(bld=p(z)), dict(link=p(z)), dict(link=p(b))):
        assert lib.adamvs_roof_links(*lk(**kw)) < 0, kw
    st = _lib.BldStats()
    lb = lambda **kw: [kw.get("W", W), H, kw.get("link", p(link)), kw.get("ws", p(ws)), kw.get("bytes", need), kw.get("parent", p(parent)),
                       kw.get("stats", ctypes.byref(st)), None]
    for kw in (dict(bytes=need - 1), dict(parent=p(ws)), dict(ws=p(link)), dict(link=p(parent)), dict(link=None), dict(ws=None), dict(parent=None),
               dict(stats=None), dict(W=-1)):
        assert lib.adamvs_roof_label(*lb(**kw)) < 0, kw
    mo = lambda **kw: [W, kw.get("H", H), kw.get("dsm", p(z)), kw.get("label", p(l0)), kw.get("bld", p(b)), kw.get("z_ref", 0.0), kw.get("N", 1),
                       kw.get("table", p(table)), None]
    for kw in (dict(N=-1), dict(N=H * W + 1), dict(table=None), dict(table=p(l0)), dict(label=p(b)), dict(dsm=None), dict(label=None), dict(bld=None),
               dict(z_ref=nan), dict(z_ref=inf), dict(H=0)):
        assert lib.adamvs_roof_moments(*mo(**kw)) < 0, kw
    gr = lambda **kw: [W, kw.get("H", H), kw.get("dsm", p(z)), kw.get("bld", p(b)), kw.get("z_ref", 0.0), kw.get("P", 1), kw.get("planes", p(planes)),
                       kw.get("tol", 0.2), kw.get("round0", 0), kw.get("rounds", 2), kw.get("l0", p(l0)), kw.get("l1", p(l1)),
                       kw.get("counts", p(counts)), None]
    for kw in (dict(P=-1), dict(P=H * W + 1), dict(planes=None), dict(l0=None), dict(l1=None), dict(counts=None), dict(dsm=None), dict(bld=None),
               dict(z_ref=nan), dict(tol=nan), dict(tol=-1.0), dict(round0=-1), dict(rounds=-1), dict(round0=255, rounds=2), dict(round0=257, rounds=0),
               dict(rounds=2 ** 31 - 1, round0=2), dict(l1=p(l0)), dict(l0=p(b)), dict(counts=p(l1)), dict(planes=p(z)), dict(H=0)):
        assert lib.adamvs_roof_grow(*gr(**kw)) < 0, kw
    rs = lambda **kw: [W, kw.get("H", H), kw.get("dsm", p(z)), kw.get("label", p(l0)), kw.get("z_ref", 0.0), kw.get("R", 1), kw.get("planes", p(planes)),
                       kw.get("tol", 0.2), kw.get("table", p(rtab)), None]
    for kw in (dict(R=-1), dict(R=H * W + 1), dict(planes=None), dict(table=None), dict(dsm=None), dict(label=None), dict(z_ref=nan), dict(tol=inf),
               dict(tol=-0.5), dict(table=p(l0)), dict(planes=p(z)), dict(H=0)):
        assert lib.adamvs_roof_residuals(*rs(**kw)) < 0, kw
    torch.cuda.synchronize()
    # nothing was launched: no output buffer has been written
    assert (parent == -7).all() and (l1 == -7).all() and (counts == -7).all() and (table == -7).all() and (rtab == -7).all() and not link.any()
    # and the calls as they stand succeed: flat ground at 7 m, all one building, z_ref 0
    assert lib.adamvs_roof_links(*lk()) == 0
    assert lib.adamvs_roof_label(*lb()) == 0 and st.converged == 1 and st.tiles == 1 and st.pairs == 0 and st.rounds == 0
    assert lib.adamvs_roof_moments(*mo()) == 0
    assert lib.adamvs_roof_moments(*mo(N=0, table=None)) == 0
    assert lib.adamvs_roof_grow(*gr()) == 0 and lib.adamvs_roof_grow(*gr(rounds=0)) == 0 and lib.adamvs_roof_grow(*gr(P=0, planes=None)) == 0
    assert lib.adamvs_roof_residuals(*rs()) == 0 and lib.adamvs_roof_residuals(*rs(R=0, planes=None, table=None)) == 0
    torch.cuda.synchronize()
    q = 7 * 256
    su, sv = H * sum(range(W)), W * sum(range(H))
    assert table[:, 0].tolist() == [H * W, su, sv, H * W * q, H * sum(u * u for u in range(W)), sum(range(W)) * sum(range(H)),
                                    W * sum(v * v for v in range(H)), su * q, sv * q, H * W * ((q * q) & 0xFFFFF), H * W * ((q * q) >> 20),
                                    0, H - 1, 0, W - 1, q, q, 1]
    assert link[1:-2, 1:-2].min() == 7 and link[-2, -2] == 1 and int((link & 1).sum()) == (H - 2) * (W - 2)      # no link out of the core block
    assert rtab[:, 0].tolist() == [0, 7 * 1024] and (l1 == 1).all() and counts[:2].tolist() == [0, 0] and (counts[2:] == -7).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_roofs_whu_end_to_end(tmp_path):
    from PIL import Image
    z, b, _ = R.four_roofs(0.05, seed=7)
    H, W = z.shape
    P = str(tmp_path / "cli" / "dsm")
    os.makedirs(os.path.dirname(P))
    g = dsm.Grid(500000.0, 3400000.0 + H * 0.5, 0.5, 0.0, W, H)
    Image.fromarray(z).save(P + "_dsm.tif", format="TIFF")
    Image.fromarray(b).save(P + "_buildings.tif", format="TIFF")
    with open(P + "_dsm.tfw", "w") as f:
        f.write(dsm.world_file_text(g))
    with open(P + "_dsm.json", "w") as f:
        json.dump(dict(grid=dict(x0=g.x0, y_top=g.y_top, gsd=g.gsd, W=g.W, H=g.H), z_ref=0.0), f)
    folder = os.path.dirname(P)
    before = {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}
    params = dict(smooth_tol=0.25, slope_tol=0.2, assign_tol=0.15, grow_rounds=10, merge_rms=0.08, flat_deg=3.0)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "roofs_whu.py"), "--dsm", P] + [v for k in params for v in ("--" + k, repr(params[k]))],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planes after the merge" in r.stdout and "total_time" in r.stdout
    after = {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}
    paths = roofs.output_paths(P)
    assert set(after) == set(before) | {os.path.basename(v) for v in paths.values()}
    for f in before:
        assert after[f] == before[f], f
    mine = roofs.from_dsm(P, **params)
    ref = R.run_ref(z, b, 0.5, **params)
    label, gj, js = roofs.read_outputs(P)
    assert label.dtype == np.int32 and np.array_equal(label, mine["label"]) and np.array_equal(label, ref["label"])
    assert after[os.path.basename(paths["geojson"])] == roofs.geojson_text(mine["polygons"], mine["properties"]).encode()
    assert len(gj["features"]) == mine["R"] == int(label.max()) == 9
    assert [f["properties"] for f in gj["features"]] == mine["properties"]
    assert js["counts"] == mine["counts"] and js["grid"] == dict(x0=g.x0, y_top=g.y_top, gsd=g.gsd, W=g.W, H=g.H)
    assert js["params"] == mine["params"] and js["params"]["grow_rounds"] == 10 and js["source"] == dict(prefix=P, filled=False)
    assert js["planes_per_building"] == {"1": 2, "2": 4, "3": 2, "4": 1} and js["label_stats"] == mine["label_stats"]
    assert js["grow_stats"] == mine["grow_stats"] and js["z_ref"] == mine["z_ref"] == 9.0      # the noisy ground dips below 10 m
    assert open(paths["label_world"]).read() == open(P + "_dsm.tfw").read()
    x0, y0 = gj["features"][0]["geometry"]["coordinates"][0][0]
    assert g.x0 <= x0 <= g.x0 + W * 0.5 and g.y_top - H * 0.5 <= y0 <= g.y_top
    with pytest.raises(FileNotFoundError, match="buildings_whu.py"):
        os.remove(P + "_buildings.tif")
        roofs.from_dsm(P)
