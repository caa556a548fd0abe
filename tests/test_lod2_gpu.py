"""LoD2 solids on the GPU (csrc/dsm_lod2.hip through hip_ops and ada_mvs_amd/lod2.py) against the numpy / Python-integer
restatement (tests/lod2_ref.py): the filled labels and the per-round counts, every column of the building table, the run count
and every field of every record in order, for exact equality, at every edge of the raster tile (64), of the scan's block (256
edges) and of the grid; then the scenes of the host test through extract(), run-to-run identity of the files, a shifted scene and
lod2_whu.py end to end.  There is no tolerance and no cell is left out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, lod2
from conftest import ROOT
import lod2_ref as R

pytestmark = pytest.mark.gpu

T = _lib.BLD_TILE_W
assert T == 64 and _lib.LOD2_BLOCK == 256


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:10])


def rand_planes(P, seed):
    """Integer planes of up to 4 mm per cell (a metre over the largest grid here), 4 .. 20 m above z_ref at cell (0, 0): above
    every base of these tests, and no two corners round alike."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(-2 ** 12, 2 ** 12, (P, 2)), rng.integers(2 ** 22, 20 * 2 ** 20, (P, 1))], axis=1).astype(np.int64)


def gpu_runs(label, planes, plane_base):
    import torch
    from ada_mvs_amd import hip_ops
    rec, N = hip_ops.lod2_runs(torch.from_numpy(np.ascontiguousarray(label, np.int32)).cuda(), torch.from_numpy(planes).cuda(),
                               torch.from_numpy(np.ascontiguousarray(plane_base, np.int32)).cuda())
    torch.cuda.synchronize()
    return rec.cpu().numpy(), N


def check_runs(label, planes, plane_base):
    """The run records of any label raster (0 = outside) -> the restatement's runs."""
    want = R.runs_ref(label, planes, plane_base)
    got, N = gpu_runs(label, planes, plane_base)
    assert N == len(want)
    same(got, R.records_array(want), "records")
    return want


def check_kernels(dtm, building, roof, planes, plane_building, rounds=R.MAX_FILL, stop_early=True):
    """Steps 2 - 4 on the device equal the restatement.  -> (the restatement's runs, the rounds run)"""
    import torch
    from ada_mvs_amd import hip_ops
    P, B = len(planes), int(building.max())
    z_ref = float(np.floor(dtm[np.isfinite(dtm)].min())) if np.isfinite(dtm).any() else 0.0
    start = R.start_labels(building, roof, plane_building)
    want_filled, want_counts = R.fill_ref(building, start, P, rounds)
    b = torch.from_numpy(building).cuda()
    filled, counts, run = lod2.fill(b, torch.from_numpy(start).cuda(), P, rounds, stop_early)
    same(filled.cpu().numpy(), want_filled, "filled")
    same(counts, want_counts, "counts")
    planes_dev = torch.from_numpy(planes).cuda()
    table = hip_ops.lod2_table(torch.from_numpy(dtm).cuda(), b, filled, z_ref, B, planes_dev).cpu().numpy()
    want_table = R.table_ref(dtm, building, want_filled, z_ref, B, planes)
    same(table, want_table, "table")
    refused = R.refused_ref(want_table)
    assert lod2.refusals(table) == refused
    label = R.zero_refused(want_filled, building, refused)
    base = np.where(want_table[2] == R.MIN_START, 0, want_table[2])
    plane_base = base[plane_building - 1].astype(np.int32)
    return check_runs(label, planes, plane_base), run


def whole_grid_case(H, W, P, seed, density):
    """One building over the whole grid (it touches all four grid edges), random plane labels at `density`, a sloping terrain."""
    rng = np.random.default_rng(seed)
    roof = np.where(rng.random((H, W)) < density, rng.integers(1, P + 1, (H, W)), 0).astype(np.int32)
    i, j = np.mgrid[0:H, 0:W]
    dtm = (1.25 + j / 128.0 + i / 256.0).astype(np.float32)
    return dtm, np.ones((H, W), np.int32), roof, rand_planes(P, seed), np.ones(P, np.int32)


# ---- steps 2 - 4 against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, T + 1), (T + 1, 1), (3, 3)])
def test_smallest_grids(H, W):
    dtm, building, roof, planes, pb = whole_grid_case(H, W, 3, H * 100 + W, 0.6)
    roof[0, 0] = 2                                                        # at least one plane: the fill reaches every cell
    runs, _ = check_kernels(dtm, building, roof, planes, pb)
    assert len(runs) >= 4                                                 # the four grid edges at the least
    check_runs(roof, planes, np.full(3, -5, np.int32))                    # and the raster as it is, holes and all


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("extra", [0, 3])
def test_a_gable_over_the_whole_grid(n, extra):
    """Two planes whose ridge runs obliquely from edge to edge: runs cross every tile and scan-block edge, reach every grid edge,
    and the sides change their order along the ridge's runs."""
    H, W = n, n + extra
    i, j = np.mgrid[0:H, 0:W]
    planes = np.array([[2 ** 17, 2 ** 15, 6 * 2 ** 20], [-2 ** 17, 2 ** 14, 6 * 2 ** 20 + 2 ** 17 * (W - 1) + 2 ** 15 * (H // 3)]], np.int64)
    z = np.stack([A * j + B * i + C for A, B, C in planes.tolist()])
    roof = (np.argmin(z, axis=0) + 1).astype(np.int32)
    roof[H // 2, W // 3:W // 3 + 2] = 0
    dtm = (2.0 + (i + j) / 512.0).astype(np.float32)
    runs, _ = check_kernels(dtm, np.ones((H, W), np.int32), roof, planes, np.ones(2, np.int32))
    ridge = [r for r in runs if r[4] and r[5]]
    assert ridge and any((r[6] - r[8]) * (r[7] - r[9]) < 0 for r in ridge)             # a crossing
    edges = {(r[0], r[1]) for r in runs}
    assert {(0, 0), (0, H), (1, 0), (1, W)} <= edges


def test_a_run_over_the_full_width():
    n = 2 * T + 1
    roof = np.ones((n, n), np.int32)
    roof[n // 2:] = 2
    planes = np.array([[0, 0, 9 * 2 ** 20], [0, 0, 11 * 2 ** 20]], np.int64)
    runs, _ = check_kernels(np.full((n, n), 2.5, np.float32), np.ones((n, n), np.int32), roof, planes, np.ones(2, np.int32))
    assert (0, n // 2, 0, n, 1, 2, 9216, 9216, 11264, 11264) in runs and (0, 0, 0, n, 0, 1, 512, 512, 9216, 9216) in runs
    assert len(runs) == 3 + 4                                             # three horizontal, two on either side


@pytest.mark.parametrize("density", [0.3, 0.6, 0.9])
def test_random_labels(density):
    """Every 2 x 2 pattern of labels at the tile corners and the block edges; as a raster of its own (zeros are outside), and
    through the fill as the roof of one building."""
    n = 2 * T + 1
    dtm, building, roof, planes, pb = whole_grid_case(n, n, 5, int(density * 10), density)
    runs = check_runs(roof, planes, np.arange(5, dtype=np.int32) * 7 - 3)
    assert len(runs) > n                                                  # the 16 patterns at a tile corner have a test of their own
    building[5:9, 100:120] = 0                                            # a yard, so that the building has a hole
    runs, _ = check_kernels(dtm, building, roof, planes, pb)
    assert len(runs) > n                                                  # the building was not refused


def test_every_two_by_two_pattern_at_a_tile_corner():
    n = 2 * T + 1
    planes = rand_planes(2, 3)
    for code in range(16):
        lab = np.zeros((n, n), np.int32)
        for k, (a, b) in enumerate(((T - 1, T - 1), (T - 1, T), (T, T - 1), (T, T))):
            lab[a, b] = 1 + (k & 1) if code >> k & 1 else 0
        lab[2 * T - 1:2 * T + 1, 2 * T - 1:2 * T + 1] = lab[T - 1:T + 1, T - 1:T + 1]      # the same pattern at the next tile corner
        check_runs(lab, planes, np.array([40, 50], np.int32))


def test_fill_fronts_longer_than_a_chunk():
    """A corridor one cell wide that the fill walks down, and a second building it must not enter: more rounds than one
    read-back chunk, stopped early and not, and capped before the end."""
    H, W = 9, 3 * lod2.FILL_CHUNK + 5
    building = np.zeros((H, W), np.int32)
    building[1, :] = 1
    building[1:8, W - 1] = 1
    building[7, 2:] = 1
    building[3:6, 2:8] = 2
    roof = np.zeros((H, W), np.int32)
    roof[1, 0], roof[1, 1], roof[4, 4] = 2, 1, 3
    planes = rand_planes(3, 9)
    pb = np.array([1, 1, 2], np.int32)
    dtm = np.full((H, W), 0.5, np.float32)
    runs, run = check_kernels(dtm, building, roof, planes, pb)
    need = (W - 2) + 6 + (W - 3)                                          # along the top, down the side, back along the bottom
    assert lod2.FILL_CHUNK < need < run <= need + lod2.FILL_CHUNK
    _, run_all = check_kernels(dtm, building, roof, planes, pb, rounds=need + 3, stop_early=False)
    assert run_all == need + 3
    check_kernels(dtm, building, roof, planes, pb, rounds=lod2.FILL_CHUNK + 1)             # capped: the rest stays outside
    check_kernels(dtm, building, roof, planes, pb, rounds=0)


def test_nothing_to_do():
    """No label at all: zero runs and no launch failure; buildings without planes; a raster without terrain."""
    import torch
    from ada_mvs_amd import hip_ops
    n = 2 * T + 1
    zeros = np.zeros((n, n + 3), np.int32)
    planes = rand_planes(2, 1)
    got, N = gpu_runs(zeros, planes, np.zeros(2, np.int32))
    assert N == 0 and got.shape == (10, 0)
    got, N = gpu_runs(zeros, np.zeros((0, 3), np.int64), np.zeros(0, np.int32))
    assert N == 0
    building = zeros.copy()
    building[3:9, 3:9], building[20:30, 20:30] = 1, 2
    runs, _ = check_kernels(np.full(zeros.shape, np.nan, np.float32), building, zeros, planes, np.array([1, 2], np.int32))
    assert runs == []
    same(hip_ops.lod2_transpose(torch.from_numpy(building).cuda()).cpu().numpy(), np.ascontiguousarray(building.T), "transpose")
    odd = np.arange(33 * 65, dtype=np.int32).reshape(33, 65)
    same(hip_ops.lod2_transpose(torch.from_numpy(odd).cuda()).cpu().numpy(), np.ascontiguousarray(odd.T), "transpose")


# ---- the stage ----------------------------------------------------------------------------------------------------------------
def check_stage(sc, **kw):
    """extract() equals the restatement at every step, and its solids pass the host test's checks.  -> (got, ref)"""
    ref = R.run_ref(sc["dtm"], sc["building"], sc["roof"], sc["properties"], sc["grid"])
    got = lod2.extract(sc["dtm"], sc["building"], sc["roof"], sc["properties"], R.GSD, grid=sc["grid"], **kw)
    assert got["z_ref"] == ref["z_ref"]
    same(got["planes"], ref["planes"], "planes")
    same(got["start"], ref["start"], "start")
    same(got["filled"], ref["filled"], "filled")
    same(got["fill_counts"], ref["counts"], "counts")
    same(got["table"], ref["table"], "table")
    assert got["refused"] == ref["refused"]
    same(got["label"], ref["label"], "label")
    assert got["N"] == len(ref["runs"])
    same(got["records"], R.records_array(ref["runs"]), "records")
    R.check_model(got, ref["label"], sc["building"], ref["planes"], ref["base"], R.GSD)
    return got, ref


@pytest.mark.parametrize("name", R.SCENES)
def test_scenes_through_extract(name, tmp_path):
    sc = R.scene(name)
    got, ref = check_stage(sc)
    assert got["counts"]["runs"] == len(ref["runs"]) and got["counts"]["cells_unfilled"] == 0
    if name == "two":
        assert got["counts"]["refused_by_reason"]["no_plane"] == 1 and sorted(got["solids"]) == [1]
    R.check_files(str(tmp_path / name), got, ref["label"])


def test_files_are_bit_identical_from_run_to_run(tmp_path):
    sc = R.scene("gable_rough")
    blobs = []
    for k in range(2):
        res = lod2.extract(sc["dtm"], sc["building"], sc["roof"], sc["properties"], R.GSD, grid=sc["grid"])
        paths = lod2.write_outputs(str(tmp_path / ("run%d" % k)), res, seconds=False)     # the timings are the one thing that differs
        blobs.append({key: open(p, "rb").read() for key, p in paths.items()})
    assert sorted(blobs[0]) == ["cityjson", "json", "obj"]
    for key in blobs[0]:
        assert blobs[0][key] == blobs[1][key] and len(blobs[0][key]) > 200, key


def test_a_shifted_scene_gives_the_same_solids():
    for name in ("gable", "courtyard"):
        got = lod2.extract(**_args(R.scene(name)))["solids"]
        moved = lod2.extract(**_args(R.scene(name, shift=(3, 5))))["solids"]
        assert sorted(got) == sorted(moved)
        for k in got:
            assert moved[k] == [dict(f, rings=[[(x + 5 * 1024, y, z) for x, y, z in ring] for ring in f["rings"]]) for f in got[k]]


def _args(sc):
    return dict(dtm=sc["dtm"], building=sc["building"], roof_label=sc["roof"], roof_properties=sc["properties"], gsd=R.GSD, grid=sc["grid"])


def test_lod2_whu_end_to_end(tmp_path):
    sc = R.scene("two")
    P = R.write_inputs(tmp_path, sc)
    folder = os.path.dirname(P)
    before = {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "lod2_whu.py"), "--dsm", P], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "1 solids, 1 refused" in r.stdout and "total_time" in r.stdout
    after = {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}
    paths = lod2.output_paths(P)
    assert set(after) == set(before) | {os.path.basename(v) for v in paths.values()}
    for f in before:
        assert after[f] == before[f], f
    mine, ref = check_stage(sc)                                           # extract() on the arrays: the same integers as the files' route
    city, (verts, objects), js = lod2.read_outputs(P)
    assert city == json.loads(json.dumps(lod2.cityjson(mine))) and sorted(objects) == ["building_1"]
    assert js["counts"] == json.loads(json.dumps(mine["counts"])) and js["refused"] == {"2": "no_plane"}
    assert js["source"] == dict(prefix=P) and set(js["seconds"]) == {"fill", "table", "runs", "faces"}
    assert open(paths["obj"]).read() == lod2.obj_text(mine)
