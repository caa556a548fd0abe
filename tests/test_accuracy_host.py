"""Cloud distance without a device: the search rule through adamvs_cloud_nearest_host (the inline functions the kernel runs) against
the fp64 brute force, the statistics, the down-sampling, the colour ramp, options, and the header / binding match."""
import os
import re

import numpy as np
import pytest
import torch

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, accuracy, hip_ops

import accuracy_inputs as I
import accuracy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUD_SYMBOLS = ("nearest", "nearest_host", "sample_count", "sample_emit")


def test_host_search_equals_the_brute_force_exactly_on_the_hand_made_input():
    T, Q, names = I.hand_made()
    d2, index, pairs = hip_ops.cloud_nearest_host(T, Q, I.HAND_D, I.HAND_ORIGIN)
    want_d2, want_index, _, _ = R.nearest(T, Q, I.HAND_D)
    assert d2.dtype == np.float32 and index.dtype == np.int32
    assert np.array_equal(d2.astype(np.float64), want_d2)
    assert np.array_equal(index.astype(np.int64), want_index)
    ok = np.isfinite(Q).all(1) & (Q >= 0).all(1) & (Q < I.LAST + 1).all(1)
    ct, cq = np.floor(T), np.floor(Q[ok])
    assert pairs == int((np.abs(cq[:, None, :] - ct[None, :, :]) <= 1).all(-1).sum())       # every target of the 27 cells, once
    # the rules by name, so that a wrong restatement cannot hide a wrong search
    assert (index[names["neighbour"]] >= 0).all() and len(names["neighbour"]) == 26
    assert sorted(set(np.round(d2[names["neighbour"]] * 16).astype(int))) == [1, 2, 3]        # 0.25^2 |d|^2, |d|^2 = 1, 2, 3
    assert d2[names["at_D"]] == 1.0 and index[names["at_D"]] >= 0
    for name in ("past_D", "two_cells", "outside"):
        assert np.isinf(d2[names[name]]).all() and (index[names[name]] == -1).all(), name
    assert list(d2[names["on_face"]]) == [0.25, 0.5625]
    assert (index[names["first_cell"]] >= 0).all() and (index[names["last_cell"]] >= 0).all()
    assert d2[names["first_cell"]][3] == 0.0625
    assert list(np.isinf(d2[names["empty_cell"]])) == [False, True]
    dup = np.nonzero((T == (90.75, 30.5, 10.5)).all(1))[0]
    assert len(dup) == 3 and index[names["duplicate"]] == dup.min()
    tie = [int(np.nonzero((T == p).all(1))[0][0]) for p in ((96.25, 30.5, 10.5), (94.75, 30.5, 10.5))]
    assert index[names["tie"]] == min(tie) and d2[names["tie"]] == 0.5625
    assert d2[names["full_cell"]][0] == 0.0 and (index[names["full_query_cell"]] >= 0).all()


def test_host_search_is_a_function_of_the_targets_as_a_set():
    T, Q, _ = I.hand_made()
    d2, index, _ = hip_ops.cloud_nearest_host(T, Q, I.HAND_D, I.HAND_ORIGIN)
    perm = np.random.default_rng(3).permutation(len(T))
    d2p, indexp, _ = hip_ops.cloud_nearest_host(T[perm], Q, I.HAND_D, I.HAND_ORIGIN)
    assert d2p.tobytes() == d2.tobytes()
    hit = index >= 0
    assert np.array_equal(indexp >= 0, hit)
    # the winner is the same point; among exact duplicates and exact ties its number may be any of theirs, the lowest new one
    assert np.array_equal(T[perm][indexp[hit]][:, 1:], T[index[hit]][:, 1:])
    dup = np.nonzero((T[perm] == (90.75, 30.5, 10.5)).all(1))[0]
    assert indexp[I.hand_made()[2]["duplicate"]] == dup.min()


def test_host_search_with_the_default_origin_holds_the_bound():
    T, Q, names = I.hand_made(last_cell=False)
    c = I.HAND_D
    o = accuracy.default_lattice_origin(c, T.min(0))
    assert np.array_equal(o, T.min(0) - c / 3.0 - c)
    d2, index, _ = hip_ops.cloud_nearest_host(T, Q, c, o)
    want_d2, want_index, second, _ = R.nearest(T, Q, c)
    d, want = np.sqrt(d2.astype(np.float64)), np.sqrt(want_d2)
    both = np.isfinite(d) & np.isfinite(want)
    assert np.abs(d[both] - want[both]).max() <= 1e-6 * c
    edge = names["at_D"]                                             # exactly D: may fall either way off the dyadic lattice
    clear = np.ones(len(Q), bool)
    clear[edge] = False
    assert np.array_equal(np.isfinite(d)[clear], np.isfinite(want)[clear])
    with np.errstate(invalid="ignore"):
        untied = both & (second - want > 2e-6 * c)
    assert np.array_equal(index[untied], want_index[untied]) and untied.sum() > 300


def test_one_target_one_query_on_the_host():
    d2, index, pairs = hip_ops.cloud_nearest_host([[5.0, 5.0, 5.0]], [[5.5, 5.0, 5.0]], 1.0, (0.0, 0.0, 0.0))
    assert d2[0] == 0.25 and index[0] == 0 and pairs == 1
    d2, index, _ = hip_ops.cloud_nearest_host([[5.0, 5.0, 5.0]], [[6.5, 5.0, 5.0]], 1.0, (0.0, 0.0, 0.0))
    assert np.isinf(d2[0]) and index[0] == -1


def test_host_search_rejects_bad_targets_and_arguments():
    with pytest.raises(_lib.AdaMVSHipError, match="not finite"):
        hip_ops.cloud_nearest_host([[np.nan, 0.0, 0.0]], [[0.0, 0.0, 0.0]], 1.0, (0.0, 0.0, 0.0))
    with pytest.raises(_lib.AdaMVSHipError, match="outside the lattice"):
        hip_ops.cloud_nearest_host([[-0.5, 0.0, 0.0]], [[0.0, 0.0, 0.0]], 1.0, (0.0, 0.0, 0.0))
    with pytest.raises(_lib.AdaMVSHipError, match="finite and > 0"):
        hip_ops.cloud_nearest_host([[0.5, 0.0, 0.0]], [[0.0, 0.0, 0.0]], 0.0, (0.0, 0.0, 0.0))
    with pytest.raises(_lib.AdaMVSHipError, match="nq"):
        hip_ops.cloud_nearest_host([[0.5, 0.0, 0.0]], np.zeros((0, 3)), 1.0, (0.0, 0.0, 0.0))


def test_summarise_on_given_distances():
    inf = float("inf")
    dist = torch.tensor([0.0, 0.125, 0.25, 0.3125, 0.375, 0.5, inf, inf], dtype=torch.float32)
    s = accuracy.summarise(dist, 0.5, [0.125, 0.25, 0.5])
    d = dist.double().numpy()
    w = d[np.isfinite(d)]
    tr = np.where(np.isfinite(d), d, 0.5)
    assert s["n"] == 8 and s["within"] == 6
    assert s["mean_trunc"] == pytest.approx(tr.mean(), rel=1e-14) and s["rmse_trunc"] == pytest.approx(np.sqrt((tr * tr).mean()), rel=1e-14)
    assert s["mean_within"] == pytest.approx(w.mean(), rel=1e-14)
    assert s["median_within"] == pytest.approx(np.median(w), rel=1e-14) and s["p90_within"] == pytest.approx(np.quantile(w, 0.9), rel=1e-14)
    assert [e["tau"] for e in s["share"]] == [0.125, 0.25, 0.5]
    assert [e["share"] for e in s["share"]] == [2 / 8, 3 / 8, 6 / 8]      # a distance equal to tau counts
    # tau = D counts exactly the points within D; the default thresholds are D/4, D/2, D
    assert accuracy.summarise(dist, 0.5)["share"][-1] == dict(tau=0.5, share=6 / 8)
    assert [e["tau"] for e in accuracy.summarise(dist, 0.5)["share"]] == [0.125, 0.25, 0.5]
    # nothing within D, and nothing at all
    s = accuracy.summarise(torch.full((3,), inf), 2.0, [1.0])
    assert s["within"] == 0 and s["mean_trunc"] == 2.0 and s["rmse_trunc"] == 2.0 and s["mean_within"] is None and s["share"][0]["share"] == 0.0
    s = accuracy.summarise(torch.empty(0), 2.0, [1.0])
    assert s["n"] == 0 and s["mean_trunc"] is None and s["share"][0]["share"] == 0.0
    with pytest.raises(ValueError, match="tau"):
        accuracy.summarise(dist, 0.5, [0.6])


def test_precision_recall_and_f():
    inf = float("inf")
    acc = accuracy.summarise(torch.tensor([0.1, 0.1, 0.3, inf], dtype=torch.float64), 0.4, [0.05, 0.2, 0.4])
    com = accuracy.summarise(torch.tensor([0.3, 0.3, inf, inf, inf], dtype=torch.float64), 0.4, [0.05, 0.2, 0.4])
    rows = accuracy.combine(acc, com)
    assert [r["tau"] for r in rows] == [0.05, 0.2, 0.4]
    assert rows[0] == dict(tau=0.05, precision=0.0, recall=0.0, fscore=0.0)             # P + R = 0
    assert rows[1] == dict(tau=0.2, precision=0.5, recall=0.0, fscore=0.0)
    assert rows[2]["precision"] == 0.75 and rows[2]["recall"] == 0.4
    assert rows[2]["fscore"] == pytest.approx(2 * 0.75 * 0.4 / 1.15, rel=1e-15)
    assert accuracy.fscore(0.0, 0.0) == 0.0 and accuracy.fscore(1.0, 1.0) == 1.0


def test_voxel_first_keeps_the_lowest_index_of_every_cell():
    rng = np.random.default_rng(2)
    p = rng.uniform(-3.0, 4.0, (500, 3))
    p[100:120] = p[5] + 1e-3                                       # a crowded cell: its first member is 5 or earlier
    kept = accuracy.voxel_first(torch.from_numpy(p), 0.7)
    cell = np.floor((p - p.min(0)) / 0.7).astype(np.int64)
    first = {}
    for i, c in enumerate(map(tuple, cell)):
        first.setdefault(c, i)
    assert kept.dtype == torch.int64 and kept.tolist() == sorted(first.values())
    assert accuracy.voxel_first(torch.from_numpy(p), 0.7).tolist() == kept.tolist()
    assert accuracy.voxel_first(torch.from_numpy(p), 100.0).tolist() == [0]
    assert accuracy.voxel_first(torch.zeros(0, 3, dtype=torch.float64), 1.0).numel() == 0
    with pytest.raises(ValueError):
        accuracy.voxel_first(torch.from_numpy(p), 0.0)
    with pytest.raises(ValueError, match="2\\^21"):
        accuracy.voxel_first(torch.from_numpy(p), 1e-7)


def test_the_colour_ramp():
    D = 2.0
    rgb = accuracy.ramp(np.array([0.0, 0.5, 1.0, 1.5, 2.0, 2.0 + 1e-9, np.inf, np.nan]), D)
    assert rgb.dtype == np.uint8 and rgb.shape == (8, 3)
    assert rgb[:5].tolist() == [[0, 0, 255], [0, 128, 128], [0, 255, 0], [128, 128, 0], [255, 0, 0]]
    assert rgb[5:].tolist() == [list(accuracy.BEYOND_RGB)] * 3
    t = np.linspace(0.0, D, 1001)
    ramp = accuracy.ramp(t, D).astype(int)
    assert not (ramp == accuracy.BEYOND_RGB).all(1).any()            # "beyond D" is a colour of its own
    assert (np.diff(ramp[:, 0]) >= 0).all() and (np.diff(ramp[:, 2]) <= 0).all()
    assert (np.abs(ramp.sum(1) - 255) <= 1).all()


def test_options_and_parser_defaults():
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError):
            accuracy.check_options(bad)
    with pytest.raises(ValueError, match="tau"):
        accuracy.check_options(1.0, [0.5, 1.5])
    with pytest.raises(ValueError, match="tau"):
        accuracy.check_options(1.0, [0.0])
    with pytest.raises(ValueError, match="spacing"):
        accuracy.check_options(1.0, spacing=0.0)
    with pytest.raises(ValueError, match="voxel_down"):
        accuracy.check_options(1.0, voxel=-1.0)
    assert accuracy.default_thresholds(2.0) == [0.5, 1.0, 2.0]
    assert accuracy.resolve_spacing(None, None, 2.0, None) == 0.5
    assert accuracy.resolve_spacing(0.3, None, 2.0, None) == 0.3
    assert accuracy.resolve_spacing(None, 2.0, 2.0, dict(voxel=0.25)) == 0.5
    with pytest.raises(ValueError, match="not both"):
        accuracy.resolve_spacing(0.3, 2.0, 2.0, dict(voxel=0.25))
    with pytest.raises(ValueError, match="json"):
        accuracy.resolve_spacing(None, 2.0, 2.0, None)
    ap = accuracy.build_parser()
    a = ap.parse_args(["--recon", "r.ply", "--truth", "t.ply", "--max_dist", "0.5"])
    assert (a.recon, a.truth, a.max_dist) == ("r.ply", "t.ply", 0.5)
    assert a.tau is None and a.spacing is None and a.spacing_voxels is None and a.voxel_down is None and a.out is None
    a = ap.parse_args(["--recon", "r", "--truth", "t", "--max_dist", "1", "--tau", "0.1", "0.2", "--voxel_down", "0.05", "--out", "x"])
    assert a.tau == [0.1, 0.2] and a.voxel_down == 0.05 and a.out == "x"
    with pytest.raises(SystemExit):
        ap.parse_args(["--recon", "r.ply", "--truth", "t.ply"])
    assert accuracy.output_paths("a/b") == ("a/b.json", "a/b_accuracy.ply", "a/b_completeness.ply")
    with pytest.raises(SystemExit, match="not both"):
        accuracy.main(["--recon", "r", "--truth", "t", "--max_dist", "1", "--spacing", "1", "--spacing_voxels", "1"])


def test_header_and_bindings_match_both_ways():
    hdr = open(os.path.join(ROOT, "include", "adamvs_hip.h")).read()
    declared = {n for n in re.findall(r"\b(adamvs_[a-z0-9_]+)\s*\(", hdr) if n.startswith("adamvs_cloud_")}
    bound = {n for n in _lib.SIGNATURES if n.startswith("adamvs_cloud_")}
    assert declared == bound == {"adamvs_cloud_" + n for n in CLOUD_SYMBOLS}
    lib = _lib.load()
    for name in bound:
        assert hasattr(lib, name)
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 22 and lib.adamvs_version() == 22
    assert "#define ADAMVS_CLOUD_TILE %d" % _lib.CLOUD_TILE in hdr and "#define ADAMVS_CLOUD_MAX_SUBDIV %d" % _lib.CLOUD_MAX_SUBDIV in hdr
    assert "Cloud distance" in hdr and "1e-6 c" in hdr and "s / sqrt(3)" in hdr


def test_cpu_tensors_raise():
    t = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        accuracy.nearest(t, t, 1.0)
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        accuracy.compare(t, t, 1.0)
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        accuracy.sample_mesh(t, torch.zeros(1, 3, dtype=torch.int64), 1.0)
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        hip_ops.cloud_sample_count(t, torch.zeros(1, 3, dtype=torch.int32), 1.0)


def test_sampler_restatement_counts_and_covers():
    """The restatement itself: (n + 1)(n + 2) / 2 samples per face, the corners among them, and the covering property of the header
    (every point of a face within s / sqrt(3) of a sample) on seeded random triangles."""
    rng = np.random.default_rng(4)
    xyz = rng.uniform(-2.0, 2.0, (30, 3))
    faces = rng.integers(0, 30, (12, 3))
    s = 0.37
    pts = R.sample_mesh(xyz, faces, s)
    ns = [R.subdivisions(xyz[f[0]], xyz[f[1]], xyz[f[2]], s) for f in faces]
    assert len(pts) == sum((n + 1) * (n + 2) // 2 for n in ns)
    at = 0
    for f, n in zip(faces, ns):
        m = (n + 1) * (n + 2) // 2
        blk = pts[at:at + m]
        assert np.array_equal(blk[0], xyz[f[0]]) and np.allclose(blk[n], xyz[f[2]], atol=1e-14) and np.allclose(blk[-1], xyz[f[1]], atol=1e-14)
        w = rng.dirichlet((1.0, 1.0, 1.0), 200)
        x = w @ xyz[f]
        d = np.sqrt(((x[:, None, :] - blk[None]) ** 2).sum(-1)).min(1)
        assert d.max() <= s / np.sqrt(3.0) * (1 + 1e-12)
        at += m
