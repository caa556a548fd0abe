"""Cloud neighbourhoods on the GPU (csrc/cloud_knn.hip through ada_mvs_amd/cloud_filter.py) against the fp64 restatement
(tests/filter_ref.py): the inputs and the bars of tests/test_filter_host.py through the device path (tests/filter_checks.py holds
both).  Where every fp32 operation is exact (the hand-made cloud on a dyadic lattice) d2, index and count equal the brute force
bit for bit; on the random clouds the header's bound |d - d_fp64| <= 1e-6 c holds, with at most 1e-3 of the queries set aside
at R or as ties; everywhere the device's bytes equal the host twin's.
tests/test_cloud_edges_gpu.py holds the search at every slice, tile, pass and chunk edge.

Measured on an MI355X (and, the bytes being equal, through the host twins): cloud T at k = 8: largest |d - d_fp64| = 0.135 of the
bound, 0 queries at R and 9 ties set aside of 30 000; cloud Q at k = 16: 0.129 of the bound, 0 at R, 3 ties.  Normals against
eigh on the kernel's own lists: the largest angle is 4.4e-4 of its bar 1e-12 lambda2 / (lambda1 - lambda0) on T at k = 8 (host
twin: 4.4e-4, the same bytes) and 4.9e-4 on Q at k = 16; no point is set aside.  The scene with strays: mu = 0.3173,
sigma = 0.0635, thresholds 0.3808 / 0.4443 / 0.5078 at ratios 1 / 2 / 3, 16 934 / 19 660 / 20 200 points kept, no point near a
threshold."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, cloud_filter, dsm, fusion, hip_ops
from conftest import ROOT
import accuracy_inputs as I
import filter_checks as C
import filter_ref as F

pytestmark = pytest.mark.gpu


def dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def search(P, R, k, **kw):
    """cloud_filter.knn on a numpy cloud -> (d2 float32, index int32, count int32, info)."""
    info = {}
    d2, index, count = cloud_filter.knn(dev(P), R, k, info=info, **kw)
    return d2.cpu().numpy(), index.cpu().numpy(), count.cpu().numpy(), info


@pytest.fixture(scope="module")
def cloud_t():
    T, _, R = I.random_clouds()
    return dict(P=T, R=R, k=8, ref=F.knn(T, R, 8), got=search(T, R, 8))


# ---- 1. the hand-made cloud ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", C.HAND_KS)
def test_hand_made_cloud_bit_for_bit(k):
    P = C.hand_cloud()
    d2, index, count, info = search(P, 1.0, k, origin=I.HAND_ORIGIN)
    C.check_hand_cloud(P, k, d2, index, count)
    h_d2, h_index, h_count, h_pairs = hip_ops.knn_search_host(P, 1.0, k, I.HAND_ORIGIN)
    assert h_d2.tobytes() == d2.tobytes() and h_index.tobytes() == index.tobytes() and h_count.tobytes() == count.tobytes()
    assert info["pairs"] == h_pairs and info["points"] == len(P)
    cells = np.unique(np.floor(P), axis=0, return_counts=True)[1]
    assert info["cells"] == len(cells) and info["items"] == int(((cells + 255) // 256).sum()) > len(cells)      # the cell of 300 is two items


def test_one_point_two_points_and_an_empty_cloud():
    import torch
    d2, index, count, info = search([[5.0, 5.0, 5.0]], 1.0, 4)
    assert count[0] == 0 and np.isinf(d2).all() and (index == -1).all() and info["pairs"] == 1
    d2, index, count, _ = search([[5.0, 5.0, 5.0], [5.5, 5.0, 5.0]], 1.0, 4, origin=(0.0, 0.0, 0.0))
    assert d2[:, 0].tolist() == [0.25, 0.25] and index[:, 0].tolist() == [1, 0] and count.tolist() == [1, 1] and np.isinf(d2[:, 1:]).all()
    d2, index, count = cloud_filter.knn(torch.empty(0, 3, dtype=torch.float64).cuda(), 1.0, 4)
    assert d2.shape == (0, 4) and index.shape == (0, 4) and count.shape == (0,) and d2.dtype == torch.float32 and index.dtype == torch.int32
    with pytest.raises(_lib.AdaMVSHipError, match="not finite"):
        cloud_filter.knn(dev([[np.nan, 0.0, 0.0], [0.0, 0.0, 0.0]]), 1.0, 4)
    with pytest.raises(_lib.AdaMVSHipError, match="outside the lattice"):
        cloud_filter.knn(dev([[0.0, 0.0, 0.0], [3e6, 0.0, 0.0]]), 1.0, 4)
    for bad in (0.0, float("nan")):
        with pytest.raises(ValueError, match="radius"):
            cloud_filter.knn(dev(np.zeros((2, 3))), bad, 4)
    with pytest.raises(ValueError, match="k="):
        cloud_filter.knn(dev(np.zeros((2, 3))), 1.0, 33)


# ---- 2. random clouds ------------------------------------------------------------------------------------------------------------
def test_cloud_t_holds_the_bound(cloud_t):
    d2, index, count, info = cloud_t["got"]
    ratio, at_R, ties, full = C.hold(d2, index, count, cloud_t["ref"], cloud_t["R"], cloud_t["k"])
    assert 0.9 <= full <= 1.0 and info["pairs"] > 8 * len(d2)
    P, R = cloud_t["P"], cloud_t["R"]
    h = hip_ops.knn_search_host(P, R, 8, P.min(0) - R / 3.0 - R)
    assert h[0].tobytes() == d2.tobytes() and h[1].tobytes() == index.tobytes() and h[2].tobytes() == count.tobytes() and h[3] == info["pairs"]


def test_cloud_q_holds_the_bound():
    _, Q, R = I.random_clouds()
    d2, index, count, _ = search(Q, R, 16)
    ratio, at_R, ties, full = C.hold(d2, index, count, F.knn(Q, R, 16), R, 16)
    assert full <= 0.05 and 0.05 <= (count < 3).mean() <= 0.12
    normal, curvature, flag, ncount = (t.cpu().numpy() for t in cloud_filter.normals(dev(Q), R, 16))
    assert np.array_equal(ncount, count) and np.array_equal(flag == F.TOO_FEW, count < 3)
    C.check_normals(Q, index, count, normal, curvature, flag)


# ---- 3. permutation and chunking -------------------------------------------------------------------------------------------------
def test_bit_identical_permuted_and_chunked(cloud_t):
    P, R, k = cloud_t["P"], cloud_t["R"], cloud_t["k"]
    d2, index, count, info = cloud_t["got"]
    again = search(P, R, k)
    assert again[0].tobytes() == d2.tobytes() and again[1].tobytes() == index.tobytes() and again[2].tobytes() == count.tobytes()
    perm = np.random.default_rng(21).permutation(len(P))
    C.check_permuted(P, perm, (d2, index, count), search(P[perm], R, k)[:3])
    chunked = search(P, R, k, chunk_queries=1000)
    assert chunked[0].tobytes() == d2.tobytes() and chunked[1].tobytes() == index.tobytes() and chunked[2].tobytes() == count.tobytes()
    assert chunked[3]["pairs"] == info["pairs"]
    s = cloud_filter.Search(dev(P), R, k, chunk_queries=1000)
    ranges = s.ranges()
    assert len(ranges) >= 30 and max(r[3] for r in ranges) <= 1000 and sum(r[3] for r in ranges) == len(P)
    assert [r[0] for r in ranges[1:]] == [r[1] for r in ranges[:-1]] and ranges[-1][1] == s.items


# ---- 4. the filter on a scene with known strays --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    P, stray = F.stray_scene()
    R, k = 0.5, 8
    ref = F.knn(P, R, k)
    want_d2, _, want_count = F.cut(ref[0], ref[1], R, k)
    return dict(P=P, stray=stray, R=R, k=k, m=F.mean_distance(want_d2, R), count=want_count)


@pytest.mark.parametrize("s,removed", [(1.0, 200), (2.0, 200), (3.0, 0)])
def test_statistical_rule_equals_the_reference_mask(scene, s, removed):
    P, stray, R, k = scene["P"], scene["stray"], scene["R"], scene["k"]
    keep_ref, mu, sigma, t = F.statistical_keep(scene["m"], s)
    assert int((~keep_ref[stray]).sum()) == removed                             # a property of the input
    keep, res = cloud_filter.filter_points(dev(P), R, k, std_ratio=s)
    near = np.abs(scene["m"] - t) <= (2.0 + s) * 1e-6 * R
    print("std_ratio %g: mu %.4f sigma %.4f threshold %.4f; %d near the threshold; kept %d" % (s, res["mu"], res["sigma"], res["threshold"],
                                                                                             near.sum(), res["kept"]))
    assert near.mean() <= 1e-3 and np.array_equal(keep.cpu().numpy()[~near], keep_ref[~near])
    assert abs(res["mu"] - mu) <= 1e-6 * R and abs(res["sigma"] - sigma) <= 1e-6 * R and abs(res["threshold"] - t) <= (1.0 + s) * 1e-6 * R
    assert res["points"] == len(P) and res["kept"] + res["removed"] == len(P) and res["removed_radius"] == 0
    assert res["removed"] == res["removed_statistical"] == int((~keep).sum()) and res["isolated"] == int((scene["count"] == 0).sum())
    chunked, res_c = cloud_filter.filter_points(dev(P), R, k, std_ratio=s, chunk_queries=1000)
    assert bool((chunked == keep).all()) and (res_c["mu"], res_c["sigma"], res_c["threshold"]) == (res["mu"], res["sigma"], res["threshold"])


def test_radius_rule_and_both_rules(scene):
    P, stray, R, k = scene["P"], scene["stray"], scene["R"], scene["k"]
    keep, res = cloud_filter.filter_points(dev(P), R, k, std_ratio=None, min_neighbours=1)
    keep = keep.cpu().numpy()
    assert np.array_equal(~keep, scene["count"] == 0) and (~keep[stray]).all() and res["mu"] is None and res["removed_statistical"] == 0
    assert res["removed"] == res["removed_radius"] == res["isolated"] == int((scene["count"] == 0).sum())
    both, res_b = cloud_filter.filter_points(dev(P), R, k, std_ratio=2.0, min_neighbours=4)
    stat, _ = cloud_filter.filter_points(dev(P), R, k, std_ratio=2.0)
    assert np.array_equal(both.cpu().numpy(), stat.cpu().numpy() & (scene["count"] >= 4))
    assert res_b["removed"] <= res_b["removed_statistical"] + res_b["removed_radius"]


def cloud_of(rec):
    return np.stack([rec["x"], rec["y"], rec["z"]], 1), np.stack([rec["red"], rec["green"], rec["blue"]], 1)


def test_written_files_and_the_command_line(scene, tmp_path):
    import torch
    P, stray, R, k = scene["P"], scene["stray"], scene["R"], scene["k"]
    rgb = np.random.default_rng(6).integers(0, 256, (len(P), 3)).astype(np.uint8)
    ply, out = str(tmp_path / "fused.ply"), str(tmp_path / "filtered" / "run")
    with fusion.PlyWriter(ply) as w:
        w.write(P, rgb)
    res = cloud_filter.main(["--ply", ply, "--radius", str(R), "--k", str(k), "--normals", "--out", out])
    keep, want = cloud_filter.filter_points(dev(P), R, k)
    keep = keep.cpu().numpy()
    assert (res["kept"], res["removed"], res["mu"], res["sigma"], res["threshold"], res["pairs"]) == \
        (want["kept"], want["removed"], want["mu"], want["sigma"], want["threshold"], want["pairs"])
    assert res["removed"] >= 200 and not keep[stray].any()
    assert dsm.ply_layout(out + ".ply")[1] == res["kept"] and dsm.ply_layout(out + "_removed.ply")[1] == res["removed"]
    kept_xyz, kept_rgb = cloud_of(fusion.read_ply(out + ".ply"))
    rem_xyz, rem_rgb = cloud_of(fusion.read_ply(out + "_removed.ply"))
    assert np.array_equal(kept_xyz, P[keep]) and np.array_equal(kept_rgb, rgb[keep])                 # the kept points, in input order
    assert np.array_equal(rem_xyz, P[~keep]) and np.array_equal(rem_rgb, rgb[~keep])                 # together: a partition of the input
    assert next(dsm.ply_chunks(out + ".ply", 10))[0].shape == (10, 3)
    js = json.load(open(out + ".json"))
    for key in ("points", "kept", "removed", "removed_statistical", "removed_radius", "isolated", "mu", "sigma", "threshold", "pairs", "cells", "items"):
        assert js[key] == json.loads(json.dumps(res[key])), key
    assert js["options"] == dict(radius=R, k=k, std_ratio=2.0, min_neighbours=None, normals=True, chunk_queries=cloud_filter.DEFAULT_CHUNK)
    assert {"filter", "normals"} <= set(js["stage_ms"]) and js["device_seconds"] > 0 and js["seconds"] > 0
    # the normals are those of the kept cloud searched afresh, bit for bit: removed points tilt nothing
    normal, curvature, flag, _ = (t.cpu().numpy() for t in cloud_filter.normals(dev(P[keep]), R, k))
    rec = cloud_filter.read_normals_ply(out + "_normals.ply")
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), P[keep]) and np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), rgb[keep])
    assert np.stack([rec["nx"], rec["ny"], rec["nz"]], 1).tobytes() == normal.astype(np.float32).tobytes()
    assert rec["curvature"].tobytes() == curvature.tobytes()
    assert js["normals"]["valid"] == int((flag == F.VALID).sum()) and js["normals"]["too_few"] == int((flag == F.TOO_FEW).sum())
    assert (normal[flag == F.VALID][:, 2] > 0.9).mean() > 0.99                  # a noisy horizontal plane: the normals point up
    # the root CLI in a fresh process, the radius rule alone
    out2 = str(tmp_path / "radius")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "filter_whu.py"), "--ply", ply, "--radius", str(R), "--k", str(k), "--std_ratio", "off",
                        "--min_neighbours", "1", "--chunk_queries", "5000", "--out", out2], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "argv:" in r.stdout and "total_time" in r.stdout
    js2 = json.load(open(out2 + ".json"))
    assert js2["removed"] == js2["removed_radius"] == int((scene["count"] == 0).sum()) and js2["mu"] is None and js2["normals_ply"] is None
    assert np.array_equal(cloud_of(fusion.read_ply(out2 + "_removed.ply"))[0], P[scene["count"] == 0]) and not os.path.exists(out2 + "_normals.ply")
    torch.cuda.synchronize()


# ---- 5. normals --------------------------------------------------------------------------------------------------------------------
def test_normals_against_eigh_on_the_kernel_s_own_lists(cloud_t):
    P, R, k = cloud_t["P"], cloud_t["R"], cloud_t["k"]
    d2, index, count, _ = cloud_t["got"]
    normal, curvature, flag, ncount = (t.cpu().numpy() for t in cloud_filter.normals(dev(P), R, k))
    assert normal.dtype == np.float64 and np.array_equal(ncount, count)
    worst, aside = C.check_normals(P, index, count, normal, curvature, flag)
    h = hip_ops.knn_normals_host(P, index, count)
    assert h[0].tobytes() == normal.tobytes() and h[1].tobytes() == curvature.tobytes() and h[2].tobytes() == flag.tobytes()
    chunked = [t.cpu().numpy() for t in cloud_filter.normals(dev(P), R, k, chunk_queries=1000)]
    assert chunked[0].tobytes() == normal.tobytes() and chunked[1].tobytes() == curvature.tobytes() and chunked[2].tobytes() == flag.tobytes()


def test_normals_of_hand_made_neighbourhoods():
    for name, (P, want) in C.normals_cases().items():
        normal, curvature, flag, count = (t.cpu().numpy() for t in cloud_filter.normals(dev(P), 1.0, 32, origin=(0.0, 0.0, 0.0)))
        assert (count == 15).all() and (flag == F.VALID).all() and (curvature == 0.0).all(), name
        assert np.abs(normal - np.array(want)).max() <= 2e-16 and (normal[:, 2] == want[2]).all(), name
        if name in ("plane", "wall_x", "wall_y"):
            assert np.array_equal(normal, np.tile(want, (16, 1))), name
        d2, index, cnt, _ = hip_ops.knn_search_host(P, 1.0, 32, (0.0, 0.0, 0.0))
        assert hip_ops.knn_normals_host(P, index, cnt)[0].tobytes() == normal.tobytes(), name
    line = np.array([[5.0, 5.0, 5.0], [5.125, 5.25, 5.375], [5.25, 5.5, 5.75], [5.375, 5.75, 6.125]])
    normal, curvature, flag, count = (t.cpu().numpy() for t in cloud_filter.normals(dev(line), 2.0, 8, origin=(0.0, 0.0, 0.0)))
    assert (count == 3).all() and (flag == F.COLLINEAR).all() and (normal == 0.0).all() and (curvature == 0.0).all()
    normal, curvature, flag, count = (t.cpu().numpy() for t in cloud_filter.normals(dev(line[:3]), 2.0, 8, origin=(0.0, 0.0, 0.0)))
    assert (count == 2).all() and (flag == F.TOO_FEW).all() and (normal == 0.0).all()
