"""Cloud neighbourhoods without a device: the search and the normals through the host twins (adamvs_knn_search_host,
adamvs_knn_normals_host: the inline functions the kernels run) against the fp64 restatement (tests/filter_ref.py), the filter's
statistics, the options, and the header / binding match.  tests/filter_checks.py holds the inputs and the bars, shared with the
device tests.

Measured here through the host twins: cloud T (30 000 points, R = 0.5) at k = 8: largest |d - d_fp64| = 0.135 of the bound 1e-6 c,
0 queries at R and 9 ties set aside (3.0e-4), 96.8 % of rows full; cloud Q at k = 16: 0.129 of the bound, 0 at R, 3 ties (1.0e-4),
1.1 % of rows full, 8.1 % of points with count < 3.  Normals of T at k = 8 against eigh: the largest angle is 4.4e-4 of its bar
1e-12 lambda2 / (lambda1 - lambda0) (6.1e-14 rad at most; the least lambda1 - lambda0 is 1.8e-3 lambda2, so no point is set aside),
the curvature differs by 7.4e-9 at most; on cloud Q at k = 16 the largest angle is 4.9e-4 of its bar."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, cloud_filter, hip_ops

import accuracy_inputs as I
import filter_checks as C
import filter_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNN_SYMBOLS = ("search", "search_host", "normals", "normals_host")


@pytest.fixture(scope="module")
def cloud_t():
    T, _, R = I.random_clouds()
    return dict(P=T, R=R, k=8, ref=F.knn(T, R, 8), got=hip_ops.knn_search_host(T, R, 8, T.min(0) - R / 3.0 - R))


# ---- 1. the hand-made cloud ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", C.HAND_KS)
def test_host_search_equals_the_brute_force_exactly_on_the_hand_made_cloud(k):
    P = C.hand_cloud()
    d2, index, count, pairs = hip_ops.knn_search_host(P, 1.0, k, I.HAND_ORIGIN)
    C.check_hand_cloud(P, k, d2, index, count)
    cell = np.floor(P)
    assert pairs == int((np.abs(cell[:, None, :] - cell[None, :, :]) <= 1).all(-1).sum())      # every point of the 27 cells, once, itself too


# ---- 2. random clouds ------------------------------------------------------------------------------------------------------------
def test_host_search_holds_the_bound_on_cloud_t(cloud_t):
    d2, index, count, _ = cloud_t["got"]
    ratio, at_R, ties, full = C.hold(d2, index, count, cloud_t["ref"], cloud_t["R"], cloud_t["k"])
    assert 0.9 <= full <= 1.0


def test_host_search_holds_the_bound_on_cloud_q():
    _, Q, R = I.random_clouds()
    d2, index, count, _ = hip_ops.knn_search_host(Q, R, 16, Q.min(0) - R / 3.0 - R)
    ratio, at_R, ties, full = C.hold(d2, index, count, F.knn(Q, R, 16), R, 16)
    assert full <= 0.05 and 0.05 <= (count < 3).mean() <= 0.12              # the padding and the invalid normals are exercised


# ---- 3. permutation --------------------------------------------------------------------------------------------------------------
def test_host_search_is_equivariant_under_a_permutation(cloud_t):
    P, R, k = cloud_t["P"], cloud_t["R"], cloud_t["k"]
    perm = np.random.default_rng(21).permutation(len(P))
    got = hip_ops.knn_search_host(P[perm], R, k, P.min(0) - R / 3.0 - R)
    C.check_permuted(P, perm, cloud_t["got"][:3], got[:3])


# ---- 4. the filter's rules ---------------------------------------------------------------------------------------------------------
def test_statistics_on_the_scene_with_known_strays():
    P, stray = F.stray_scene()
    R, k = 0.5, 8
    ref = F.knn(P, R, k)
    want_d2, _, want_count = F.cut(ref[0], ref[1], R, k)
    m_ref = F.mean_distance(want_d2, R)
    d2, _, count, _ = hip_ops.knn_search_host(P, R, k, P.min(0) - R / 3.0 - R)
    m = cloud_filter.mean_distance(torch.from_numpy(d2), R)
    assert m.dtype == torch.float64 and np.abs(m.numpy() - m_ref).max() <= 1e-6 * R
    assert (m_ref[stray] == R).all()                                          # every stray is alone: all k slots count as R
    for s, removed, inliers in ((1.0, 200, 0.847), (2.0, 200, 0.983), (3.0, 0, 1.0)):
        keep_ref, mu, sigma, t = F.statistical_keep(m_ref, s)
        assert int((~keep_ref[stray]).sum()) == removed and abs(keep_ref[~stray].mean() - inliers) <= 5e-4      # a property of the input
        keep, g_mu, g_sigma, g_t = cloud_filter.statistical_keep(m, s)
        near = np.abs(m_ref - t) <= (2.0 + s) * 1e-6 * R
        assert near.mean() <= 1e-3 and np.array_equal(keep.numpy()[~near], keep_ref[~near])
        assert abs(g_mu - mu) <= 1e-6 * R and abs(g_sigma - sigma) <= 1e-6 * R and abs(g_t - t) <= (1.0 + s) * 1e-6 * R
        if s == 2.0:
            assert round(mu, 4) == 0.3173 and round(sigma, 4) == 0.0635 and round(t, 4) == 0.4443
        if s == 3.0:
            assert t > R
    assert np.array_equal(count == 0, want_count == 0) and (count[stray] == 0).all()
    # order independence: the decision is reduced from the sorted values
    perm = np.random.default_rng(4).permutation(len(P))
    keep, mu, sigma, t = cloud_filter.statistical_keep(m, 2.0)
    keep_p, mu_p, sigma_p, t_p = cloud_filter.statistical_keep(m[torch.from_numpy(perm)], 2.0)
    assert (mu_p, sigma_p, t_p) == (mu, sigma, t) and np.array_equal(keep_p.numpy(), keep.numpy()[perm])


def test_mean_distance_counts_missing_slots_as_the_radius():
    inf = float("inf")
    d2 = torch.tensor([[0.25, 1.0, inf, inf], [inf, inf, inf, inf], [0.0, 0.0, 0.0625, 4.0]], dtype=torch.float32)
    assert cloud_filter.mean_distance(d2, 2.0).tolist() == [(0.5 + 1.0 + 2.0 + 2.0) / 4, 2.0, (0.25 + 2.0) / 4]
    keep, mu, sigma, t = cloud_filter.statistical_keep(torch.tensor([1.0, 1.0, 1.0, 5.0], dtype=torch.float64), 1.0)
    assert mu == 2.0 and sigma == pytest.approx(np.sqrt(3.0), rel=1e-15) and keep.tolist() == [True, True, True, False]
    assert cloud_filter.statistical_keep(torch.zeros(0, dtype=torch.float64), 1.0)[1] is None


# ---- 5. normals --------------------------------------------------------------------------------------------------------------------
def test_host_normals_against_eigh_on_the_search_s_own_lists(cloud_t):
    d2, index, count, _ = cloud_t["got"]
    normal, curvature, flag = hip_ops.knn_normals_host(cloud_t["P"], index, count)
    worst, aside = C.check_normals(cloud_t["P"], index, count, normal, curvature, flag)


def test_host_normals_flags_on_cloud_q():
    _, Q, R = I.random_clouds()
    d2, index, count, _ = hip_ops.knn_search_host(Q, R, 16, Q.min(0) - R / 3.0 - R)
    normal, curvature, flag = hip_ops.knn_normals_host(Q, index, count)
    assert np.array_equal(flag == F.TOO_FEW, count < 3) and (flag == F.TOO_FEW).mean() >= 0.05
    C.check_normals(Q, index, count, normal, curvature, flag)


def test_host_normals_of_hand_made_neighbourhoods():
    for name, (P, want) in C.normals_cases().items():
        d2, index, count, _ = hip_ops.knn_search_host(P, 1.0, 32, (0.0, 0.0, 0.0))
        assert (count == 15).all(), name
        normal, curvature, flag = hip_ops.knn_normals_host(P, index, count)
        assert (flag == F.VALID).all() and (curvature == 0.0).all(), name
        assert np.abs(normal - np.array(want)).max() <= 2e-16 and (normal[:, 2] == want[2]).all(), name
        if name in ("plane", "wall_x", "wall_y"):
            assert np.array_equal(normal, np.tile(want, (16, 1))), name
    line = np.array([[5.0, 5.0, 5.0], [5.125, 5.25, 5.375], [5.25, 5.5, 5.75], [5.375, 5.75, 6.125]])
    d2, index, count, _ = hip_ops.knn_search_host(line, 2.0, 8, (0.0, 0.0, 0.0))
    normal, curvature, flag = hip_ops.knn_normals_host(line, index, count)
    assert (count == 3).all() and (flag == F.COLLINEAR).all() and (normal == 0.0).all() and (curvature == 0.0).all()
    d2, index, count, _ = hip_ops.knn_search_host(line[:3] + [[0, 0, 0], [0.125, 0, 0], [0, 0, 0]], 2.0, 8, (0.0, 0.0, 0.0))
    normal, curvature, flag = hip_ops.knn_normals_host(line[:3], index, count)
    assert (count == 2).all() and (flag == F.TOO_FEW).all() and (normal == 0.0).all()
    # row_point: rows in another order than the points
    P = C.normals_cases()["wall_xy"][0]
    d2, index, count, _ = hip_ops.knn_search_host(P, 1.0, 32, (0.0, 0.0, 0.0))
    rows = np.array([7, 0, 12], np.int32)
    got = hip_ops.knn_normals_host(P, index[rows], count[rows], rows)
    full = hip_ops.knn_normals_host(P, index, count)
    assert all(np.array_equal(g, f[rows]) for g, f in zip(got, full))


# ---- 6. bindings and refusals ------------------------------------------------------------------------------------------------------
def test_header_and_bindings_match_both_ways():
    hdr = open(os.path.join(ROOT, "include", "adamvs_hip.h")).read()
    declared = {n for n in re.findall(r"\b(adamvs_[a-z0-9_]+)\s*\(", hdr) if n.startswith("adamvs_knn_")}
    bound = {n for n in _lib.SIGNATURES if n.startswith("adamvs_knn_")}
    assert declared == bound == {"adamvs_knn_" + n for n in KNN_SYMBOLS}
    lib = _lib.load()
    for name in bound:
        assert hasattr(lib, name)
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 22 and lib.adamvs_version() == 22
    assert "#define ADAMVS_KNN_MAX_K %d" % _lib.KNN_MAX_K in hdr and _lib.KNN_MAX_K == 32
    assert "#define ADAMVS_KNN_RANK_EPS 1e-12" in hdr and _lib.KNN_RANK_EPS == 1e-12 == F.RANK_EPS
    for name, v in (("VALID", _lib.KNN_VALID), ("TOO_FEW", _lib.KNN_TOO_FEW), ("COLLINEAR", _lib.KNN_COLLINEAR)):
        assert "#define ADAMVS_KNN_%s %d" % (name, v) in hdr
    assert (F.VALID, F.TOO_FEW, F.COLLINEAR) == (_lib.KNN_VALID, _lib.KNN_TOO_FEW, _lib.KNN_COLLINEAR)
    assert "Cloud neighbourhoods" in hdr and '"cloud_knn.hip"' in open(os.path.join(ROOT, "ada-mvs_amd", "build.py")).read()


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    o = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    bad_o = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data                                       # never dereferenced: every call below is refused first

    def search(origin=o, R=1.0, k=8, n=4, ni=1, base=0, rows=4, nc=1, null=None):
        a = [p] * 11
        if null is not None:
            a[null] = None
        return lib.adamvs_knn_search(origin, R, k, a[0], a[1], nc, a[2], a[3], n, a[4], a[5], a[6], ni, base, rows, a[7], a[8], a[9], a[10], None)

    for kw in (dict(k=0), dict(k=33), dict(R=0.0), dict(R=-1.0), dict(R=float("nan")), dict(R=float("inf")), dict(n=0), dict(n=1 << 31),
               dict(ni=0), dict(ni=5), dict(rows=0), dict(rows=5), dict(base=1), dict(base=-1), dict(nc=0), dict(nc=5), dict(origin=None),
               dict(origin=bad_o)) + tuple(dict(null=i) for i in range(11)):
        assert search(**kw) < 0, kw
    assert "knn_search" in lib.adamvs_last_error_string().decode()
    for args in ((o, 1.0, 0, p, 4, p, p, p, None), (o, 1.0, 33, p, 4, p, p, p, None), (o, 0.0, 8, p, 4, p, p, p, None),
                 (o, float("inf"), 8, p, 4, p, p, p, None), (o, 1.0, 8, p, 0, p, p, p, None), (o, 1.0, 8, None, 4, p, p, p, None),
                 (o, 1.0, 8, p, 4, None, p, p, None), (o, 1.0, 8, p, 4, p, None, p, None), (o, 1.0, 8, p, 4, p, p, None, None),
                 (None, 1.0, 8, p, 4, p, p, p, None)):
        assert lib.adamvs_knn_search_host(*args) < 0, args
    for fn, tail in ((lib.adamvs_knn_normals, (None,)), (lib.adamvs_knn_normals_host, ())):
        for args in ((p, 4, p, p, 0, 4, None, p, p, p), (p, 4, p, p, 33, 4, None, p, p, p), (p, 0, p, p, 8, 4, None, p, p, p),
                     (p, 4, p, p, 8, 0, None, p, p, p), (p, 1 << 31, p, p, 8, 4, None, p, p, p), (None, 4, p, p, 8, 4, None, p, p, p),
                     (p, 4, None, p, 8, 4, None, p, p, p), (p, 4, p, None, 8, 4, None, p, p, p), (p, 4, p, p, 8, 4, None, None, p, p),
                     (p, 4, p, p, 8, 4, None, p, None, p), (p, 4, p, p, 8, 4, None, p, p, None)):
            assert fn(*(args + tail)) < 0, args


def test_host_search_rejects_bad_points_and_options():
    with pytest.raises(_lib.AdaMVSHipError, match="not finite"):
        hip_ops.knn_search_host([[np.nan, 0.0, 0.0]], 1.0, 8, (0.0, 0.0, 0.0))
    with pytest.raises(_lib.AdaMVSHipError, match="outside the lattice"):
        hip_ops.knn_search_host([[-0.5, 0.0, 0.0]], 1.0, 8, (0.0, 0.0, 0.0))
    with pytest.raises(_lib.AdaMVSHipError, match="finite and > 0"):
        hip_ops.knn_search_host([[0.5, 0.0, 0.0]], 0.0, 8, (0.0, 0.0, 0.0))
    for k in (0, 33, 8.0, True):
        with pytest.raises(_lib.AdaMVSHipError, match="k="):
            hip_ops.knn_search_host([[0.5, 0.0, 0.0]], 1.0, k, (0.0, 0.0, 0.0))
    d2, index, count, pairs = hip_ops.knn_search_host([[0.5, 0.5, 0.5]], 1.0, 4, (0.0, 0.0, 0.0))      # one point: itself is no neighbour
    assert count[0] == 0 and np.isinf(d2).all() and (index == -1).all() and pairs == 1


def test_cpu_tensors_raise():
    t = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        cloud_filter.knn(t, 1.0, 8)
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        cloud_filter.normals(t, 1.0, 8)
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        cloud_filter.filter_points(t, 1.0)
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        hip_ops.knn_normals(t, torch.zeros(4, 8, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))


def test_options_and_parser():
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="radius"):
            cloud_filter.check_options(bad)
    for bad in (0, 33, 8.0, True):
        with pytest.raises(ValueError, match="k="):
            cloud_filter.check_options(1.0, bad)
    with pytest.raises(ValueError, match="std_ratio"):
        cloud_filter.check_options(1.0, 8, -1.0)
    with pytest.raises(ValueError, match="min_neighbours"):
        cloud_filter.check_options(1.0, 8, None, 9)
    with pytest.raises(ValueError, match="chunk_queries"):
        cloud_filter.check_options(1.0, 8, None, None, 0)
    ap = cloud_filter.build_parser()
    a = ap.parse_args(["--ply", "fused.ply", "--radius", "0.5"])
    assert (a.ply, a.radius, a.k, a.std_ratio, a.min_neighbours, a.normals, a.out) == ("fused.ply", 0.5, 16, 2.0, None, False, None)
    assert a.chunk_queries == cloud_filter.DEFAULT_CHUNK
    a = ap.parse_args(["--ply", "f", "--radius", "1", "--k", "8", "--std_ratio", "off", "--min_neighbours", "2", "--normals", "--out", "x"])
    assert (a.k, a.std_ratio, a.min_neighbours, a.normals, a.out) == (8, None, 2, True, "x")
    with pytest.raises(SystemExit):
        ap.parse_args(["--ply", "fused.ply"])
    assert cloud_filter.output_paths("a/b") == ("a/b.json", "a/b.ply", "a/b_removed.ply", "a/b_normals.ply")


def test_normals_ply_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    xyz, nrm = rng.uniform(-5e5, 5e5, (7, 3)), rng.normal(size=(7, 3))
    curv, rgb = rng.uniform(0, 1 / 3, 7).astype(np.float32), rng.integers(0, 256, (7, 3)).astype(np.uint8)
    path = str(tmp_path / "n.ply")
    cloud_filter.write_normals_ply(path, xyz, nrm, curv, rgb)
    head = open(path, "rb").read(400).split(b"end_header\n")[0].decode().splitlines()
    assert [ln.split()[1:] for ln in head if ln.startswith("property")] == [["double", "x"], ["double", "y"], ["double", "z"], ["float", "nx"],
                                                                          ["float", "ny"], ["float", "nz"], ["float", "curvature"],
                                                                          ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    rec = cloud_filter.read_normals_ply(path)
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), xyz) and np.array_equal(rec["curvature"], curv)
    assert np.array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], 1), nrm.astype(np.float32))
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), rgb)
