"""Cloud registration on the GPU (csrc/cloud_register.hip through ada_mvs_amd/register.py): the three kernels against their host
twins bit for bit on the inputs of tests/test_register_host.py, the device loop against the host loop bit for bit (the host loop is
held to the restatement and to the known motion there), permutations, the georeferenced offset, the "lost" error, and the files:
register_whu.py followed by accuracy_whu.py, and a mesh whose faces and colours must come through byte for byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, accuracy, dsm, fusion, hip_ops, mesh, register
from conftest import ROOT
import register_inputs as I
import register_ref as R
from register_inputs import same_bits, same_values

pytestmark = pytest.mark.gpu


def dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@pytest.fixture(scope="module")
def terrain():
    return I.terrain()


@pytest.fixture(scope="module")
def runs(terrain):
    """The device loop on both sources, once."""
    return {name: register.icp(dev(terrain[name]), dev(terrain["truth"]), I.D, tol=1e-9 if name == "copy" else None)
            for name in ("copy", "independent")}


def same_result(a, b):
    return (same_bits(a["R"], b["R"]) and same_bits(a["t"], b["t"]) and same_bits(a["pivot"], b["pivot"]) and a["history"] == b["history"]
            and a["iterations"] == b["iterations"] and a["converged"] == b["converged"] and a["pairs"] == b["pairs"]
            and all(a[k] == b[k] for k in ("fitness_before", "fitness_after", "rms_plane_before", "rms_plane_after", "rms_point_after")))


def test_rigid_apply_equals_its_host_twin_bit_for_bit():
    for n in (0, 1, 257):
        x, rot, c, t = I.apply_cases(n)
        y = hip_ops.rigid_apply(dev(x).reshape(n, 3), rot, c, t).cpu().numpy()
        assert same_values(y, hip_ops.rigid_apply_host(x, rot, c, t)), n
        fine = np.isfinite(x).all(1)
        assert same_bits(hip_ops.rigid_apply(dev(x).reshape(n, 3), np.eye(3), c, np.zeros(3)).cpu().numpy()[fine], x[fine])


@pytest.mark.parametrize("delta", [0.0, 0.2])
def test_accumulate_and_reduce_equal_their_host_twins_bit_for_bit(delta):
    for nq in I.SIZES:
        k = I.accumulate_cases(nq)
        partial = hip_ops.icp_accumulate(dev(k["y"]).reshape(nq, 3), dev(k["index"], np.int32), dev(k["targets"]), dev(k["normals"]),
                                         dev(k["flag"], np.uint8), k["c"], k["L"], delta)
        sums = hip_ops.icp_reduce(partial)
        want = hip_ops.icp_accumulate_host(k["y"], k["index"], k["targets"], k["normals"], k["flag"], k["c"], k["L"], delta)
        assert same_bits(partial.cpu().numpy(), want), nq
        assert same_bits(sums.cpu().numpy(), hip_ops.icp_reduce_host(want)), nq


@pytest.mark.parametrize("name", ["copy", "independent"])
def test_icp_equals_icp_host_bit_for_bit_and_from_run_to_run(terrain, runs, name):
    tol = 1e-9 if name == "copy" else None
    want = register.icp_host(terrain[name], terrain["truth"], I.D, tol=tol)
    assert same_result(runs[name], want)
    assert same_result(register.icp(dev(terrain[name]), dev(terrain["truth"]), I.D, tol=tol), runs[name])
    assert runs[name]["converged"] and runs[name]["constrained_dof"] == 6


def test_a_permuted_target_gives_the_same_bits_and_a_permuted_source_the_same_motion(terrain, runs):
    rng = np.random.default_rng(9)
    src, tgt = terrain["independent"], terrain["truth"]
    a = register.icp(dev(src), dev(tgt[rng.permutation(len(tgt))]), I.D)
    assert same_bits(a["R"], runs["independent"]["R"]) and same_bits(a["t"], runs["independent"]["t"])
    assert a["history"] == runs["independent"]["history"]
    b = register.icp(dev(src[rng.permutation(len(src))]), dev(tgt), I.D)
    apart = np.sqrt(((R.apply(src, b["R"], b["pivot"], b["t"]) - R.apply(src, a["R"], a["pivot"], a["t"])) ** 2).sum(1)).max()
    print("permuted source: %.3e m apart" % apart)
    assert apart <= 1e-9


def test_the_offset_does_not_change_the_estimated_motion(terrain, runs):
    zero = I.terrain(offset=(0.0, 0.0, 0.0))
    res = register.icp(dev(zero["independent"]), dev(zero["truth"]), I.D)
    here = R.apply(zero["independent"], res["R"], res["pivot"], res["t"])
    there = R.apply(terrain["independent"], runs["independent"]["R"], runs["independent"]["pivot"], runs["independent"]["t"])
    apart = np.sqrt(((there - np.asarray(I.OFFSET) - here) ** 2).sum(1)).max()
    print("offset 0 against the stated offset: %.3e m apart" % apart)
    assert apart <= 1e-6


def test_lost(terrain):
    import torch
    src, tgt = dev(terrain["independent"]), dev(terrain["truth"])
    empty = torch.empty(0, 3, device="cuda", dtype=torch.float64)
    for s, t in ((empty, tgt), (src, empty), (src + torch.tensor([0.0, 0.0, 30.0], device="cuda", dtype=torch.float64), tgt)):
        with pytest.raises(_lib.AdaMVSHipError, match="lost: 0 pairs within D"):
            register.icp(s, t, I.D)


def write_points(path, pts, rgb=None):
    with fusion.PlyWriter(path) as w:
        w.write(pts, rgb if rgb is not None else np.zeros((len(pts), 3), np.uint8))


def cli(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + [str(a) for a in args], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "argv:" in r.stdout and "total_time" in r.stdout
    return r


def test_register_then_score_through_the_files(terrain, tmp_path):
    """register_whu.py, then accuracy_whu.py on <out>.ply.  The nearest distance, truncated or not, is 1-Lipschitz in a point's
    displacement, so the mean of the registered cloud differs from that of the never-moved source by at most the error of the
    transform: at most twice what the restatement's loop reaches (tests/test_register_host.py: 3.08e-3 m)."""
    ref = R.icp(terrain["independent"], terrain["truth"], I.D)
    bound = 2.0 * I.estimate_error(ref, terrain["independent"], terrain["still_independent"])
    recon, truth, out = str(tmp_path / "recon.ply"), str(tmp_path / "truth.ply"), str(tmp_path / "reg" / "run")
    rgb = np.random.default_rng(4).integers(0, 256, (len(terrain["independent"]), 3)).astype(np.uint8)
    write_points(recon, terrain["independent"], rgb), write_points(truth, terrain["truth"])
    cli("register_whu.py", "--recon", recon, "--truth", truth, "--max_dist", I.D, "--out", out)
    res = json.load(open(out + ".json"))
    assert res["converged"] and res["fitness_after"] >= res["fitness_before"] and res["constrained_dof"] == 6
    assert set(register.STAGES) <= set(res["stage_ms"]) and res["written"] == len(rgb)
    M = np.loadtxt(out + ".txt")
    assert same_bits(M, np.asarray(res["matrix"]))
    assert I.estimate_error(res, terrain["independent"], terrain["still_independent"]) <= bound
    moved = [np.concatenate(p) for p in zip(*dsm.ply_chunks(out + ".ply", 1 << 20))]
    assert np.array_equal(moved[1], rgb)
    assert same_bits(moved[0], hip_ops.rigid_apply(dev(terrain["independent"]), res["R"], res["pivot"], res["t"]).cpu().numpy())
    cli("accuracy_whu.py", "--recon", out + ".ply", "--truth", truth, "--max_dist", I.D, "--out", str(tmp_path / "scored"))
    scored = json.load(open(str(tmp_path / "scored") + ".json"))
    still = accuracy.summarise(accuracy.nearest(dev(terrain["truth"]), dev(terrain["still_independent"]), I.D)[0], I.D)
    raw = accuracy.summarise(accuracy.nearest(dev(terrain["truth"]), dev(terrain["independent"]), I.D)[0], I.D)
    print("mean_trunc: registered %.4e m, never moved %.4e m, not registered %.4e m; bound %.3e m"
          % (scored["accuracy"]["mean_trunc"], still["mean_trunc"], raw["mean_trunc"], bound))
    assert abs(scored["accuracy"]["mean_trunc"] - still["mean_trunc"]) <= bound
    # --init from the written matrix: already there
    register.from_files(recon, truth, I.D, init=out + ".txt", voxel_down=0.5, out=str(tmp_path / "again"), log=lambda *a: None)
    again = json.load(open(str(tmp_path / "again") + ".json"))
    assert again["iterations"] <= 2 and again["inputs"]["recon"]["points_kept"] < len(rgb) and again["written"] == len(rgb)


def test_a_mesh_keeps_its_faces_and_colours_byte_for_byte(terrain, tmp_path):
    xyz, rgb, faces = I.grid_mesh()
    xyz = I.moved(xyz, terrain["centre"], terrain["R"], terrain["shift"])
    mesh_ply, truth, out = str(tmp_path / "grid.ply"), str(tmp_path / "truth.ply"), str(tmp_path / "grid_reg")
    with mesh.MeshPlyWriter(mesh_ply) as w:
        w.write(xyz, rgb, faces)
    write_points(truth, terrain["truth"])
    res = register.from_files(mesh_ply, truth, I.D, out=out, log=lambda *a: None)
    assert res["inputs"]["recon"]["kind"] == "mesh" and res["converged"] and res["written"] == len(xyz)
    v0, f0 = mesh.read_mesh_ply(mesh_ply)
    v1, f1 = mesh.read_mesh_ply(out + ".ply")
    assert np.array_equal(f0, f1) and all(np.array_equal(v0[c], v1[c]) for c in ("red", "green", "blue"))
    a, b = open(mesh_ply, "rb").read(), open(out + ".ply", "rb").read()
    end = a.index(b"end_header\n") + 11
    tail = end + len(v0) * fusion.PLY_DTYPE.itemsize
    assert a[:end] == b[:end] and a[tail:] == b[tail:] and len(a) == len(b)
    want = hip_ops.rigid_apply(dev(xyz), res["R"], res["pivot"], res["t"]).cpu().numpy()
    assert same_bits(np.stack([v1["x"], v1["y"], v1["z"]], 1), want)
    back = np.sqrt(((want - I.grid_mesh()[0]) ** 2).sum(1)).max()
    print("mesh: vertices back within %.3e m of where they came from" % back)
