"""The cloud searches at every slice and tile edge, without a device: the host twins (adamvs_knn_search_host,
adamvs_cloud_nearest_host: the inline functions of csrc/cloud_lattice.h that the kernels run) against the fp64 brute force of
tests/cloud_edges.py on its sweep clouds, bit for bit, no tolerance and no query set aside; and the properties of the sweep that
tests/test_cloud_edges_gpu.py relies on, asserted so that a later edit cannot hollow it out.

Measured here: the k-NN sweep is 193 clusters and 39 985 points in 4 440 cells, knn_search_host evaluates 8 308 715 pairs; at k = 8
18 812 rows hold an exact tie among their places and 5 159 one at the last place, at k = 32 16 925 rows are not full.  The
nearest-target sweep is 219 clusters, 34 859 targets and 20 498 queries, cloud_nearest_host evaluates 2 631 991 pairs, 17 575 queries
find a target.  The brute force of both takes about two seconds, the file ten."""
import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, hip_ops

import accuracy_ref
import cloud_edges as E
import filter_ref


@pytest.fixture(scope="module")
def knn():
    cloud = E.knn_cloud()
    return dict(cloud, ref=E.knn_brute(cloud["P"], cloud["cluster"]))


@pytest.fixture(scope="module")
def near():
    clouds = E.nearest_clouds()
    return dict(clouds, ref=E.nearest_brute(clouds["T"], clouds["Q"], clouds["tcluster"], clouds["qcluster"]))


# ---- 1. the host twins against the brute force ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", E.KS)
def test_host_knn_equals_the_brute_force_on_the_sweep(knn, k):
    d2, index, count, pairs = hip_ops.knn_search_host(knn["P"], E.R, k, E.ORIGIN)
    want_d2, want_index, want_count = E.knn_cut(knn["ref"], k)
    wrong = np.nonzero((d2.astype(np.float64) != want_d2).any(1) | (index != want_index).any(1) | (count != want_count))[0]
    assert len(wrong) == 0, E.describe(knn, wrong, k)
    assert pairs == int(E.candidates(knn["P"]).sum())
    print("k = %d: %d points, %d pairs, %d rows with a tie among their places, %d with one at the last place, %d rows not full"
          % (k, len(d2), pairs, (np.isfinite(want_d2[:, 1:]) & (want_d2[:, 1:] == want_d2[:, :-1])).any(1).sum(),
             E.tie_at_last_place(knn["ref"], k).sum(), (want_count < k).sum()))


def test_host_nearest_equals_the_brute_force_on_the_sweep(near):
    d2, index, pairs = hip_ops.cloud_nearest_host(near["T"], near["Q"], E.R, E.ORIGIN)
    want_d2, want_index = near["ref"]
    wrong = np.nonzero((d2.astype(np.float64) != want_d2) | (index != want_index))[0]
    assert len(wrong) == 0, [(int(r),) + tuple(near["cases"][near["qcluster"][r]][1:]) for r in wrong[:6]]
    assert pairs == int(E.candidates(near["Q"], near["T"]).sum())
    print("%d targets, %d queries, %d pairs, %d within D" % (len(near["T"]), len(near["Q"]), pairs, (want_index >= 0).sum()))


def test_the_brute_force_has_a_second_opinion():
    """The restatements the other cloud tests use (another brute force, written apart from this one) on a small cloud of three
    clusters: they agree with cloud_edges' bit for bit.  A second opinion, not the reference."""
    cloud = E.knn_cloud(cases=((5, 40), (64, 65)), borders=E.BORDERS[:1], seed=3)
    ref = E.knn_brute(cloud["P"], cloud["cluster"])
    other = filter_ref.knn(cloud["P"], E.R, 8)
    got = filter_ref.cut(other[0], other[1], E.R, 8)
    for a, b in zip(got, E.knn_cut(ref, 8)):
        assert np.array_equal(a, b)
    clouds = E.nearest_clouds(cases=((5, 40), (3, 0), (64, 65)), borders=E.BORDERS[:1], seed=4)
    want = E.nearest_brute(clouds["T"], clouds["Q"], clouds["tcluster"], clouds["qcluster"])
    other = accuracy_ref.nearest(clouds["T"], clouds["Q"], E.R)
    assert np.array_equal(other[0], want[0]) and np.array_equal(other[1], want[1]) and (want[1] == -1).sum() >= 3


# ---- 2. the sweep reaches what it is meant to reach -----------------------------------------------------------------------------------
def test_the_sweep_is_derived_from_the_kernels_sizes():
    assert E.LANES == (_lib.CLOUD_TILE, _lib.CLOUD_TILE // 2) and E.lanes_of(16) == E.LANES[0] and E.lanes_of(17) == E.LANES[1]
    assert E.slices(1, 256) == (1, 256) and E.slices(3, 256) == (4, 64) and E.slices(128, 256) == (128, 2) and E.slices(129, 256) == (256, 1)
    assert E.totals(64, 256) == {3, 4, 5, 15, 16, 17, 255, 256, 257, 513} and max(E.KS) == _lib.KNN_MAX_K == E.K_REF - 1


@pytest.mark.parametrize("L", E.LANES)
def test_every_split_into_slices_occurs(knn, near, L):
    cnt, P, S, _ = E.passes(knn["P"], L)
    powers = {1 << b for b in range(L.bit_length())}
    assert set(zip(P.tolist(), S.tolist())) == {(p, L // p) for p in powers}
    for p in powers - {1}:                                      # both ends of every class of counts: P / 2 + 1 and P queries
        assert (cnt[P == p] == p).any() and (cnt[P == p] == p // 2 + 1).any(), p
    if L == E.LANES[0]:
        cnt, P, S, _ = E.passes(near["Q"], L)
        assert set(zip(P.tolist(), S.tolist())) == {(p, L // p) for p in powers}
    else:                                                       # the second pass of a two-pass item: 1, 127 and 128 queries
        own = knn["own"]
        assert {1, 127, 128} <= set(cnt[own].tolist())
        assert set(c for _, c, _ in knn["cases"]) >= {129, 255, 256, 257, 513}


def test_every_total_occurs(knn, near):
    total, own = E.candidates(knn["P"]), knn["own"]
    have = set(zip((np.array([knn["cases"][j][1] for j in knn["cluster"]])[own]).tolist(), total[own].tolist()))
    for c in E.COUNTS:
        for L in E.LANES:
            for t in E.totals(c, L):
                assert t < max(c, 1) or (c, t) in have, (c, t, L)
    assert {(c, t) for _, c, t in E.BORDERS} <= have and min(t for _, _, t in E.BORDERS) >= _lib.CLOUD_TILE + 1
    total = E.candidates(near["Q"], near["T"])
    have = set(zip(np.array([near["cases"][j][1] for j in near["qcluster"]]).tolist(), total.tolist()))
    for c in E.COUNTS:
        for t in E.totals(c, E.LANES[0]) | {0}:
            assert (c, t) in have, (c, t)
    assert {(c, t) for _, c, t in E.BORDERS} <= have
    # a row boundary of the packed candidates falls inside a tile: the candidates of a cluster's cell come from several rows
    for j, (_, c, t) in enumerate(near["cases"][:-len(E.BORDERS)]):
        assert t < 27 or len(np.unique(np.floor(near["T"][near["tcluster"] == j][:, 1:]), axis=0)) == 9


def test_rows_that_are_not_full_and_ties_at_the_last_place(knn):
    ref = knn["ref"]
    for k in E.KS:
        if k > 1:
            assert (ref[2] < k).any(), k
        if k <= 16:
            assert E.tie_at_last_place(ref, k).any(), k
    assert ((ref[2] > 0) & (ref[2] < 32)).sum() > 1000 and (ref[2] == 0).any() and (ref[2] >= E.K_REF).any()


def test_the_clusters_do_not_see_each_other(knn, near):
    E.assert_apart(knn["P"], knn["cluster"])
    E.assert_apart(np.concatenate([near["T"], near["Q"]]), np.concatenate([near["tcluster"], near["qcluster"]]))
    apart = knn["P"].copy()
    apart[knn["cluster"] == 1, 0] -= 1.0                        # one cluster moved a cell towards its neighbour: the check sees it
    with pytest.raises(AssertionError, match="see each other"):
        E.assert_apart(apart, knn["cluster"])
    for pts in (knn["P"], near["T"], near["Q"]):
        assert np.array_equal(pts * 16.0, np.round(pts * 16.0)) and (pts >= 0).all()


def test_the_small_cloud_of_the_chunk_tests():
    cloud = E.knn_cloud(cases=E.CHUNK_CASES, borders=(), seed=33)
    assert 1500 <= len(cloud["P"]) <= 2500 and [c for _, c, _ in cloud["cases"]] == [1, 1, 3, 257, 513]
    count = np.unique(E.cell_keys(cloud["P"]), return_counts=True)[1]
    assert {257, 513} <= set(count.tolist())                    # cells of two and of three work items
    ref = E.knn_brute(cloud["P"], cloud["cluster"])
    d2, index, count, _ = hip_ops.knn_search_host(cloud["P"], E.R, 32, E.ORIGIN)
    for a, b in zip((d2.astype(np.float64), index, count), E.knn_cut(ref, 32)):
        assert np.array_equal(a, b)
    for m in (1, 8, 32):                                        # the radius rule has both answers at every m
        assert 0 < (ref[2] >= m).sum() < len(count)
