"""Cloud distance on the GPU (csrc/cloud_dist.hip through ada_mvs_amd/accuracy.py) against the fp64 restatement
(tests/accuracy_ref.py).  The bar is the header's derived bound |d - d_fp64| <= 1e-6 c: the kept flags must agree outside
|d - D| <= 1e-6 c, the indices unless the second-nearest target lies within 2e-6 c of the nearest, and each set-aside share is at
most 1e-3.  Where every fp32 operation is exact (the hand-made input on a dyadic lattice) d2 and index are equal bit for bit.
tests/test_cloud_edges_gpu.py holds the search at every slice and tile edge of its walk.

Measured with the same inline functions on the host (adamvs_cloud_nearest_host, random clouds of test 2): largest |d - d_fp64| =
0.126 of the bound, no query of 30 000 set aside at D or as a tie, 85.4 % within D, the fullest cell holds 14 targets."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, accuracy, fusion, fusion_synth, mesh
from conftest import ROOT
import accuracy_inputs as I
import accuracy_ref as R

pytestmark = pytest.mark.gpu


def dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def run(T, Q, D, **kw):
    """nearest() on numpy clouds -> (dist fp64 view of the fp32 result, index int64, d2 fp32, info)."""
    detail = {}
    dist, index, info = accuracy.nearest(dev(T), dev(Q), D, detail=detail, **kw)
    assert dist.dtype.is_floating_point and dist.element_size() == 4 and index.element_size() == 4
    d2 = detail["d2"].cpu().numpy() if "d2" in detail else np.full(len(Q), np.inf, np.float32)
    return dist.cpu().numpy().astype(np.float64), index.cpu().numpy().astype(np.int64), d2, info


def hold(dist, index, ref, c, D, extra=0.0, shares=True):
    """The GPU result against the restatement ref = (d2, index, second, first) as the module docstring says -> (largest error over
    the bound, queries set aside at D, queries set aside as ties, share within D).  shares=False: the input is made of edge cases,
    the two set-aside shares are not held to 1e-3."""
    want = np.sqrt(ref[0])
    bound = 1e-6 * c + extra
    both = np.isfinite(dist) & np.isfinite(want)
    err = float(np.abs(dist[both] - want[both]).max())
    print("largest |d - d_fp64| = %.3e = %.3f of the bound %.3e" % (err, err / bound, bound))
    assert err <= bound
    at_edge = np.abs(ref[3] - D) <= bound                        # the nearest target lies within the bound of D: either way
    assert np.array_equal(np.isfinite(dist)[~at_edge], np.isfinite(want)[~at_edge])
    with np.errstate(invalid="ignore"):
        tied = both & ~(ref[2] - want > 2.0 * bound)
    ok = both & ~tied
    assert np.array_equal(index[ok], ref[1][ok])
    assert (index[~np.isfinite(dist)] == -1).all() and (index[np.isfinite(dist)] >= 0).all()
    print("set aside: %d at D, %d ties of %d; %.1f %% within D" % (at_edge.sum(), tied.sum(), len(dist), 100.0 * np.isfinite(dist).mean()))
    assert not shares or (at_edge.mean() <= 1e-3 and tied.mean() <= 1e-3)
    return err / bound, int(at_edge.sum()), int(tied.sum()), float(np.isfinite(dist).mean())


@pytest.fixture(scope="module")
def clouds():
    T, Q, D = I.random_clouds()
    return dict(T=T, Q=Q, D=D, ref=R.nearest(T, Q, D))


@pytest.fixture(scope="module")
def base(clouds):
    return run(clouds["T"], clouds["Q"], clouds["D"])


# ---- 1. the hand-made input ---------------------------------------------------------------------------------------------------
def test_hand_made_input_bit_for_bit():
    T, Q, names = I.hand_made()
    dist, index, d2, info = run(T, Q, I.HAND_D, origin=I.HAND_ORIGIN)
    want_d2, want_index, _, _ = R.nearest(T, Q, I.HAND_D)
    assert np.array_equal(d2.astype(np.float64), want_d2)
    assert np.array_equal(index, want_index)
    hit = want_index >= 0
    assert np.array_equal(np.isinf(dist), ~hit) and np.abs(dist[hit] - np.sqrt(want_d2[hit])).max() <= 1e-6 * I.HAND_D      # dist is an fp32 root
    from ada_mvs_amd import hip_ops
    h_d2, h_index, h_pairs = hip_ops.cloud_nearest_host(T, Q, I.HAND_D, I.HAND_ORIGIN)
    assert h_d2.tobytes() == d2.tobytes() and np.array_equal(h_index, index) and info["pairs"] == h_pairs
    assert info["outside"] == len(names["outside"]) and info["within"] == int((want_index >= 0).sum())
    inside = np.isfinite(Q).all(1) & (Q >= 0).all(1) & (Q < I.LAST + 1).all(1)
    assert info["items"] == len(np.unique(np.floor(Q[inside]), axis=0)) + 1            # the cell with 300 queries is two work items
    assert d2[names["at_D"]] == 1.0 and np.isinf(d2[names["past_D"]]) and np.isinf(d2[names["two_cells"]]).all()


def test_hand_made_input_on_the_default_lattice():
    T, Q, _ = I.hand_made(last_cell=False)
    dist, index, _, _ = run(T, Q, I.HAND_D)
    hold(dist, index, R.nearest(T, Q, I.HAND_D), I.HAND_D, I.HAND_D, shares=False)


def test_one_target_one_query_and_empty_clouds():
    import torch
    dist, index, d2, info = run([[5.0, 5.0, 5.0]], [[5.5, 5.0, 5.0]], 1.0, origin=(0.0, 0.0, 0.0))
    assert d2[0] == 0.25 and dist[0] == 0.5 and index[0] == 0 and info["pairs"] == 1 and info["items"] == 1
    dist, index, _, info = run([[5.0, 5.0, 5.0]], [[5.5, 5.0, 5.0]], 0.25)
    assert np.isinf(dist[0]) and index[0] == -1 and info["within"] == 0
    none = torch.empty(0, 3, dtype=torch.float64).cuda()
    some = dev(np.zeros((3, 3)))
    dist, index, info = accuracy.nearest(none, some, 1.0)
    assert dist.shape == (3,) and bool(torch.isinf(dist).all()) and index.tolist() == [-1, -1, -1] and info["pairs"] == 0
    dist, index, info = accuracy.nearest(some, none, 1.0)
    assert dist.shape == (0,) and index.shape == (0,) and dist.dtype == torch.float32 and index.dtype == torch.int32
    with pytest.raises(_lib.AdaMVSHipError, match="not finite"):
        accuracy.nearest(dev([[np.nan, 0.0, 0.0], [0.0, 0.0, 0.0]]), some, 1.0)
    with pytest.raises(_lib.AdaMVSHipError, match="outside the lattice"):
        accuracy.nearest(dev([[0.0, 0.0, 0.0], [3e6, 0.0, 0.0]]), some, 1.0)


# ---- 2. random clouds ------------------------------------------------------------------------------------------------------------
def test_random_clouds(clouds, base):
    dist, index, _, info = base
    ratio, at_edge, tied, within = hold(dist, index, clouds["ref"], clouds["D"], clouds["D"])
    assert 0.8 <= within <= 0.9 and info["within"] == int(np.isfinite(dist).sum())
    assert info["pairs"] > info["within"] and info["cells"] > 5000


# ---- 3. determinism --------------------------------------------------------------------------------------------------------------
def test_bit_identical_and_independent_of_either_order(clouds, base):
    T, Q, D = clouds["T"], clouds["Q"], clouds["D"]
    dist, index, d2, _ = base
    again = run(T, Q, D)
    assert again[2].tobytes() == d2.tobytes() and np.array_equal(again[1], index)
    rng = np.random.default_rng(21)
    perm = rng.permutation(len(T))
    p = run(T[perm], Q, D)
    assert p[2].tobytes() == d2.tobytes()
    hit = index >= 0
    assert np.array_equal(p[1] >= 0, hit) and np.array_equal(perm[p[1][hit]], index[hit])
    qperm = rng.permutation(len(Q))
    p = run(T, Q[qperm], D)
    assert p[2].tobytes() == d2[qperm].tobytes() and np.array_equal(p[1], index[qperm])


# ---- 4. far from the origin -----------------------------------------------------------------------------------------------------
def test_far_from_the_origin(clouds, base):
    off = np.array([5e5, 3.4e6, 0.0])
    T, Q, D = clouds["T"] + off, clouds["Q"] + off, clouds["D"]
    dist, index, _, _ = run(T, Q, D)
    hold(dist, index, clouds["ref"], D, D, extra=4.0 * float(np.spacing(np.abs(T).max())))


# ---- 5. the sampler --------------------------------------------------------------------------------------------------------------
def sample(xyz, faces, s):
    return accuracy.sample_mesh(dev(xyz), dev(faces, np.int64), s).cpu().numpy()


def test_sampler_hand_made_faces_bit_for_bit():
    s = 0.25
    xyz = np.array([[0.0, 0.0, 0.0], [0.125, 0.0, 0.0], [0.0, 0.1875, 0.0625],            # n = 1
                    [10.0, 0.0, 0.0], [12.0, 0.0, 0.0], [11.0, 1.3, 0.7],                # the longest edge is exactly 8 s
                    [5.0, 5.0, 5.0], [6.0, 6.0, 6.0], [7.0, 7.0, 7.0],                    # zero area: collinear
                    [3.0, 3.0, 3.0],                                                        # zero area: one point thrice
                    [100.1, 200.2, 0.3], [100.1 + 153.6, 200.2 + 204.8, 0.3], [90.7, 260.9, 33.3]])      # the longest edge is 1024 s
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 9, 9], [10, 11, 12], [2, 1, 0]])
    ns = [R.subdivisions(xyz[f[0]], xyz[f[1]], xyz[f[2]], s) for f in faces]
    assert ns == [1, 8, 14, 1, 1024, 1]
    got, want = sample(xyz, faces, s), R.sample_mesh(xyz, faces, s)
    assert got.shape == want.shape == (sum((n + 1) * (n + 2) // 2 for n in ns), 3)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(got[:3], xyz[[0, 2, 1]]) and np.array_equal(got[-3:], xyz[[2, 0, 1]])      # (0,0) (0,1) (1,0): v0, v2, v1
    xyz[11, 1] += 0.5                                                                                 # more than 1024 subdivisions
    with pytest.raises(_lib.AdaMVSHipError, match="face 4 "):
        sample(xyz, faces, s)
    with pytest.raises(_lib.AdaMVSHipError, match="refers to vertex"):
        sample(xyz, np.array([[0, 1, 13]]), s)
    assert sample(xyz, np.zeros((0, 3), np.int64), s).shape == (0, 3)


def test_sampler_covers_random_triangles():
    rng = np.random.default_rng(8)
    xyz = rng.uniform(-3.0, 3.0, (60, 3)) + np.array([5e5, 3.4e6, 20.0])
    faces = np.stack([rng.permutation(60)[:3] for _ in range(40)])
    s = 0.45
    got = sample(xyz, faces, s)
    assert got.tobytes() == R.sample_mesh(xyz, faces, s).tobytes()
    at = 0
    for f in faces:
        n = R.subdivisions(xyz[f[0]], xyz[f[1]], xyz[f[2]], s)
        m = (n + 1) * (n + 2) // 2
        x = rng.dirichlet((1.0, 1.0, 1.0), 300) @ xyz[f]
        d = np.sqrt(((x[:, None, :] - got[None, at:at + m]) ** 2).sum(-1)).min(1)
        assert d.max() <= s / np.sqrt(3.0) * (1 + 1e-12)
        at += m
    assert at == len(got)


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
def quad(x0, x1, y0, y1, z):
    return np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], np.float64), np.array([[0, 1, 2], [0, 2, 3]])


def write_points(path, pts):
    with fusion.PlyWriter(path) as w:
        w.write(pts, np.zeros((len(pts), 3), np.uint8))


def test_end_to_end(tmp_path):
    """The analytic scene of fusion_synth as horizontal faces (the terrain and the top of every box of BOXES), sampled at 1 m: the
    truth.  The reconstruction: the same samples lifted by 0.1 m, once with every box and once with box 2 left out."""
    D, taus, s, lift, missing = 0.4, [0.05, 0.2, 0.4], 1.0, 0.1, 2
    parts = [quad(-100.0, 100.0, -100.0, 100.0, 0.0)] + [quad(x0, x1, y0, y1, h) for x0, x1, y0, y1, h in fusion_synth.BOXES]
    pts = [sample(v, f, s) for v, f in parts]
    truth = np.concatenate(pts)
    up = np.array([0.0, 0.0, lift])
    full = truth + up
    recon = np.concatenate([p for k, p in enumerate(pts) if k != 1 + missing]) + up
    share_missing = len(pts[1 + missing]) / len(truth)
    res_full = accuracy.compare(dev(full), dev(truth), D, taus)
    res = accuracy.compare(dev(recon), dev(truth), D, taus)
    acc = res["accuracy"]
    assert acc["n"] == len(recon) and acc["within"] == len(recon)
    assert lift - 1e-6 * D <= acc["mean_within"] <= np.sqrt(lift * lift + s * s / 3.0) + 1e-6 * D
    assert lift - 1e-6 * D <= acc["median_within"] <= acc["p90_within"] <= np.sqrt(lift * lift + s * s / 3.0) + 1e-6 * D
    assert [r["tau"] for r in res["scores"]] == taus
    assert res["scores"][0]["precision"] == 0.0 and res["scores"][0]["recall"] == 0.0 and res["scores"][0]["fscore"] == 0.0
    assert res["scores"][1]["precision"] == 1.0 and res_full["scores"][1]["recall"] == 1.0
    for k in (1, 2):
        assert res_full["scores"][k]["recall"] - res["scores"][k]["recall"] == pytest.approx(share_missing, abs=1e-15)
        assert res["scores"][k]["recall"] == (len(truth) - len(pts[1 + missing])) / len(truth)
        p, r = res["scores"][k]["precision"], res["scores"][k]["recall"]
        assert res["scores"][k]["fscore"] == pytest.approx(2 * p * r / (p + r), rel=1e-15)
    com = res["completeness"]
    assert com["n"] == len(truth) and com["within"] == len(truth) - len(pts[1 + missing])
    assert com["mean_trunc"] == pytest.approx((com["within"] * com["mean_within"] + (com["n"] - com["within"]) * D) / com["n"], rel=1e-12)
    assert res["pairs"] == res["accuracy_search"]["pairs"] + res["completeness_search"]["pairs"] > 0
    # the CLI on PLYs of the same data, in a fresh process
    recon_ply, truth_ply, out = str(tmp_path / "recon.ply"), str(tmp_path / "truth.ply"), str(tmp_path / "scored" / "run")
    write_points(recon_ply, recon), write_points(truth_ply, truth)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "accuracy_whu.py"), "--recon", recon_ply, "--truth", truth_ply, "--max_dist", str(D),
                        "--tau"] + [str(t) for t in taus] + ["--out", out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "argv:" in r.stdout and "total_time" in r.stdout
    js = json.load(open(out + ".json"))
    for k in ("accuracy", "completeness", "scores", "pairs", "max_dist"):
        assert js[k] == json.loads(json.dumps(res[k])), k
    assert js["thresholds"] == taus and js["options"]["max_dist"] == D and js["inputs"]["recon"] == dict(path=recon_ply, kind="points", points=len(recon))
    assert js["inputs"]["truth"]["points"] == len(truth) and js["device_seconds"] > 0
    assert {"accuracy_nearest", "completeness_nearest", "accuracy_sorts", "accuracy_keys", "accuracy_items", "statistics"} <= set(js["stage_ms"])
    a, c = fusion.read_ply(js["accuracy_ply"]), fusion.read_ply(js["completeness_ply"])
    assert len(a) == len(recon) and len(c) == len(truth)
    assert np.array_equal(np.stack([a["x"], a["y"], a["z"]], 1), recon) and np.array_equal(np.stack([c["x"], c["y"], c["z"]], 1), truth)
    rgb_a, rgb_c = np.stack([a["red"], a["green"], a["blue"]], 1), np.stack([c["red"], c["green"], c["blue"]], 1)
    want = accuracy.ramp([lift], D)[0].astype(int)                  # t = 1/4: a channel sits on a rounding boundary, so +- 1
    assert (np.abs(rgb_a.astype(int) - want) <= 1).all()
    beyond = (rgb_c == accuracy.BEYOND_RGB).all(1)
    assert beyond.sum() == len(pts[1 + missing]) and (np.abs(rgb_c[~beyond].astype(int) - want) <= 1).all()


def test_mesh_given_as_recon_is_scored_through_its_samples(tmp_path):
    D = 0.4
    v, f = quad(0.0, 4.0, 0.0, 3.0, 1.0)
    mesh_ply, truth_ply, out = str(tmp_path / "quad.ply"), str(tmp_path / "plane.ply"), str(tmp_path / "quad_scored")
    with mesh.MeshPlyWriter(mesh_ply) as w:
        w.write(v, np.zeros((4, 3), np.uint8), f.astype(np.uint32))
    gx, gy = np.meshgrid(np.arange(0.0, 4.01, 0.5), np.arange(0.0, 3.01, 0.5), indexing="ij")
    plane = np.stack([gx.reshape(-1), gy.reshape(-1), np.ones(gx.size)], 1)
    write_points(truth_ply, plane)
    res = accuracy.main(["--recon", mesh_ply, "--truth", truth_ply, "--max_dist", str(D), "--out", out])
    n = 50                                                      # ceil(5 / (D / 4))
    assert res["inputs"]["recon"] == dict(path=mesh_ply, kind="mesh", vertices=4, faces=2, spacing=D / 4, points=(n + 1) * (n + 2))
    assert res["thresholds"] == [D / 4, D / 2, D]
    acc, com = res["accuracy"], res["completeness"]
    assert acc["n"] == acc["within"] == (n + 1) * (n + 2) and com["n"] == com["within"] == len(plane)
    assert acc["p90_within"] <= 0.25 * np.sqrt(2.0) + 1e-6 * D          # no sample is farther from the 0.5 m grid than half its diagonal
    assert com["mean_within"] <= com["p90_within"] <= (D / 4) / np.sqrt(3.0) + 1e-6 * D      # the covering bound
    assert res["scores"][0]["recall"] == 1.0 and res["scores"][2]["precision"] == 1.0
    js = json.load(open(out + ".json"))
    assert js["scores"] == json.loads(json.dumps(res["scores"]))
    assert len(fusion.read_ply(out + "_accuracy.ply")) == (n + 1) * (n + 2) and len(fusion.read_ply(out + "_completeness.ply")) == len(plane)
    with open(mesh_ply + ".json", "w") as fj:
        json.dump(dict(voxel=0.25), fj)
    res = accuracy.from_files(mesh_ply, truth_ply, D, spacing_voxels=2.0, out=out, log=lambda *a: None)
    assert res["inputs"]["recon"]["spacing"] == 0.5 and res["inputs"]["recon"]["points"] == 11 * 12
