"""The cloud searches on the GPU (k_knn_search of csrc/cloud_knn.hip through ada_mvs_amd/cloud_filter.py, k_cloud_nearest of
csrc/cloud_dist.hip through ada_mvs_amd/accuracy.py) at every edge of the walk they share (csrc/cloud_lattice.h): every split of
the lanes into P queries times S slices, candidate totals of S - 1 .. 4 S + 1 (the sweep's step and its last batch) and of
LANES - 1 .. 2 LANES + 1 (the tile loop) for both lane counts, items of two passes, lists that are not full, exact ties at the
last place across slices, the first and the last slot of every class of k, the lattice's borders, and chunk boundaries between
the items of one cell.  tests/cloud_edges.py builds the clouds on a 1/16 grid where every fp32 operation is exact and holds the
fp64 brute force, so d2, index and count are compared bit for bit, with no tolerance, no mask and no query set aside;
tests/test_cloud_edges_host.py asserts that the sweep reaches those edges and holds the host twins to the same reference.

Measured on an MI355X: the k-NN sweep cloud is 193 clusters, 39 985 points in 4 440 cells and 4 444 work items, 8 308 715 pair
evaluations at every k; the nearest-target sweep is 219 clusters, 34 859 targets, 20 498 queries in 249 work items, 2 631 991
pairs, 17 575 queries within D; the small cloud of the chunk tests is 2 001 points.  Everything equals the brute force and the
host twins.  Times: the fixture (cloud and brute force) 0.6 s once, the first search 0.9 s (it loads the library), every other
case of test 1 0.12 to 0.13 s, test 2 0.33 s, test 3 0.41 / 0.46 s, test 4 0.11 s per k, test 5 0.19 s at most; the file 6.6 s.

Each of these one-line changes to the kernels (none can leave an array: tried once each, never committed) fails the file:
the sweep's step KNN_BATCH S + S: every case of tests 1, 3 and 4, test 5 at m = 8 and 32; the k-NN merge tree from S / 4: the same
cases; the nearest-target merge tree from S / 4: test 2; no reset of the list at the second pass: test 1 at k = 17, 31 and 32,
tests 3 and 4 at k = 32; the nearest-target sweep to n - 1: test 2; cloud_walk_fill one short of every row: all 18 cases."""
import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, accuracy, cloud_filter, hip_ops
import cloud_edges as E
import filter_checks as C

pytestmark = pytest.mark.gpu


def dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def search(P, k, **kw):
    """cloud_filter.knn on a numpy cloud of the 1/16 grid -> (d2 float32, index int32, count int32, info)."""
    info = {}
    d2, index, count = cloud_filter.knn(dev(P), E.R, k, origin=E.ORIGIN, info=info, **kw)
    return d2.cpu().numpy(), index.cpu().numpy(), count.cpu().numpy(), info


def same_bytes(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def knn():
    cloud = E.knn_cloud()
    return dict(cloud, ref=E.knn_brute(cloud["P"], cloud["cluster"]), got={})


@pytest.fixture(scope="module")
def small():
    cloud = E.knn_cloud(cases=E.CHUNK_CASES, borders=(), seed=33)
    return dict(cloud, ref=E.knn_brute(cloud["P"], cloud["cluster"]))


def searched(knn, k):
    """The search of the sweep cloud at k, once per module."""
    if k not in knn["got"]:
        knn["got"][k] = search(knn["P"], k)
    return knn["got"][k]


def assert_equals_brute(cloud, k, d2, index, count):
    want_d2, want_index, want_count = E.knn_cut(cloud["ref"], k)
    assert d2.dtype == np.float32 and index.dtype == np.int32 and count.dtype == np.int32 and d2.shape == index.shape == want_d2.shape
    wrong = np.nonzero((d2.astype(np.float64) != want_d2).any(1) | (index != want_index).any(1) | (count != want_count))[0]
    assert len(wrong) == 0, E.describe(cloud, wrong, k)


# ---- 1. the k nearest on the sweep cloud -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", E.KS)
def test_knn_equals_the_brute_force_at_every_edge(knn, k):
    d2, index, count, info = searched(knn, k)
    assert_equals_brute(knn, k, d2, index, count)
    h_d2, h_index, h_count, h_pairs = hip_ops.knn_search_host(knn["P"], E.R, k, E.ORIGIN)
    assert same_bytes((d2, index, count), (h_d2, h_index, h_count))
    cells = np.unique(E.cell_keys(knn["P"]), return_counts=True)[1]
    T = _lib.CLOUD_TILE
    assert info["pairs"] == h_pairs and info["points"] == len(knn["P"]) and info["cells"] == len(cells)
    assert info["items"] == int(((cells + T - 1) // T).sum()) > len(cells)
    print("k = %d: %d points, %d cells, %d items, %d pairs" % (k, info["points"], info["cells"], info["items"], info["pairs"]))


# ---- 2. the nearest target on its sweep --------------------------------------------------------------------------------------------
def test_nearest_equals_the_brute_force_at_every_edge():
    clouds = E.nearest_clouds()
    T, Q = clouds["T"], clouds["Q"]
    want_d2, want_index = E.nearest_brute(T, Q, clouds["tcluster"], clouds["qcluster"])
    detail = {}
    dist, index, info = accuracy.nearest(dev(T), dev(Q), E.R, detail=detail, origin=E.ORIGIN)
    d2, index = detail["d2"].cpu().numpy(), index.cpu().numpy()
    assert d2.dtype == np.float32 and index.dtype == np.int32
    wrong = np.nonzero((d2.astype(np.float64) != want_d2) | (index != want_index))[0]
    cnt, P, S, items = E.passes(Q, E.LANES[0])
    total = E.candidates(Q, T)
    assert len(wrong) == 0, "%d wrong queries; " % len(wrong) + "; ".join(
        "query %d: cluster (c %d, t %d), item of %d queries, P %d, S %d, %d candidates"
        % ((r,) + tuple(clouds["cases"][clouds["qcluster"][r]][1:]) + (cnt[r], P[r], S[r], total[r])) for r in wrong[:6])
    h_d2, h_index, h_pairs = hip_ops.cloud_nearest_host(T, Q, E.R, E.ORIGIN)
    assert same_bytes((d2, index), (h_d2, h_index))
    assert info["pairs"] == h_pairs == int(total.sum()) and info["items"] == items and info["within"] == int((want_index >= 0).sum())
    assert info["targets"] == len(T) and info["queries"] == len(Q) and info["outside"] == 0
    empty = np.array([clouds["cases"][j][2] == 0 for j in clouds["qcluster"]])      # the clusters of t = 0: nothing around the query cell
    assert empty.sum() >= sum(E.COUNTS) and np.isposinf(d2[empty]).all() and (index[empty] == -1).all()
    assert np.isposinf(dist.cpu().numpy()[empty]).all() and (total[empty] == 0).all()
    print("%d targets, %d queries, %d items, %d pairs, %d within D" % (len(T), len(Q), info["items"], info["pairs"], info["within"]))


# ---- 3. equivariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (8, 32))
def test_knn_of_the_permuted_sweep_cloud(knn, k):
    """On this grid the k-th and the (k + 1)-th place lie at the same d2 in 13 % of the rows at k = 8 and 14 % at k = 32 (measured
    on the brute force alone), and there the numbers decide which of the two stays, so the set changes with the permutation: the
    reference cannot keep 90 % of the rows for a comparison of sets.  So d2 and count of the permuted run are compared on every
    row, bit for bit, and the permuted run is held to the brute force of the permuted cloud, index included.  Beyond that the
    indices go through filter_checks.check_permuted on the rows without such a tie (the tied rows are handed over as the mapping
    of the base run, so they pass by construction)."""
    P = knn["P"]
    d2, index, count, _ = searched(knn, k)
    perm = np.random.default_rng(41).permutation(len(P))
    pd2, pindex, pcount, _ = search(P[perm], k)
    assert pd2.tobytes() == d2[perm].tobytes() and np.array_equal(pcount, count[perm])
    permuted = dict(P=P[perm], cluster=knn["cluster"][perm], own=knn["own"][perm], cases=knn["cases"])
    permuted["ref"] = E.knn_brute(permuted["P"], permuted["cluster"])
    assert_equals_brute(permuted, k, pd2, pindex, pcount)
    tied = E.tie_at_last_place(knn["ref"], k)[perm]
    inverse = np.empty(len(P), np.int64)
    inverse[perm] = np.arange(len(P))
    base = index[perm]
    handed = pindex.copy()
    handed[tied] = np.where(base[tied] >= 0, inverse[np.maximum(base[tied], 0)], -1)
    print("k = %d: %d of %d rows without a tie at the last place (%.1f %%)" % (k, (~tied).sum(), len(tied), 100.0 * (~tied).mean()))
    assert 0.5 <= (~tied).mean() < 0.9
    C.check_permuted(P, perm, (d2, index, count), (pd2, handed, pcount))


# ---- 4. chunk edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (8, 32))
def test_chunks_cut_between_the_items_of_a_cell(small, k):
    P = small["P"]
    d2, index, count, info = search(P, k)
    assert_equals_brute(small, k, d2, index, count)
    normal, curvature, flag, ncount = (t.cpu().numpy() for t in cloud_filter.normals(dev(P), E.R, k, origin=E.ORIGIN))
    assert np.array_equal(ncount, count) and same_bytes((normal, curvature, flag), hip_ops.knn_normals_host(P, index, count))
    assert {_lib.KNN_VALID, _lib.KNN_TOO_FEW} <= set(flag.tolist())
    for chunk in E.CHUNKS:
        c_d2, c_index, c_count, c_info = search(P, k, chunk_queries=chunk)
        assert same_bytes((c_d2, c_index, c_count), (d2, index, count)), chunk
        assert c_info["pairs"] == info["pairs"] and c_info["items"] == info["items"], chunk
        s = cloud_filter.Search(dev(P), E.R, k, origin=E.ORIGIN, chunk_queries=chunk)
        ranges = s.ranges()
        end = s.item_end
        assert ranges[0][0] == 0 and ranges[-1][1] == s.items and [r[0] for r in ranges[1:]] == [r[1] for r in ranges[:-1]], chunk
        assert all(i1 > i0 and base == (int(end[i0 - 1]) if i0 else 0) and base + rows == int(end[i1 - 1]) for i0, i1, base, rows in ranges)
        assert sum(r[3] for r in ranges) == len(P) and all(r[3] <= chunk or r[1] == r[0] + 1 for r in ranges), chunk
        if chunk == _lib.CLOUD_TILE:                            # a chunk ends after the first item of the cell of 257 and of the cell of 513
            key, cnt = s.item_key.cpu().numpy(), s.item_count.cpu().numpy()
            inside = [i0 for i0, _, _, _ in ranges[1:] if key[i0 - 1] == key[i0]]
            assert len(inside) >= 3 and any(cnt[i0 - 1] == 256 and cnt[i0] == 1 for i0 in inside)
        chunked = [t.cpu().numpy() for t in cloud_filter.normals(dev(P), E.R, k, origin=E.ORIGIN, chunk_queries=chunk)]
        assert same_bytes(chunked, (normal, curvature, flag, ncount)), chunk


# ---- 5. the radius rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 8, 32))
def test_radius_rule_equals_the_count_of_the_brute_force(small, m):
    keep, res = cloud_filter.filter_points(dev(small["P"]), E.R, 32, std_ratio=None, min_neighbours=m, origin=E.ORIGIN)
    want = small["ref"][2] >= m
    assert np.array_equal(keep.cpu().numpy(), want) and 0 < want.sum() < len(want)
    assert res["kept"] == int(want.sum()) and res["removed"] == res["removed_radius"] == int((~want).sum()) and res["removed_statistical"] == 0
    assert res["isolated"] == int((small["ref"][2] == 0).sum()) >= 1
