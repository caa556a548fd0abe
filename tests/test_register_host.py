"""Cloud registration without a device: the host twins of the three kernels (the inline functions the kernels run) against the numpy
restatement tests/register_ref.py bit for bit, the whole loop (register.icp_host, assembled from the host twins of every kernel it
launches) against the known motion and against the restatement's loop, the flat scene, options and errors, and the header /
binding match."""
import math
import os
import re

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, hip_ops, register

import register_inputs as I
import register_ref as R
from register_inputs import same_bits, same_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("adamvs_rigid_apply", "adamvs_icp_accumulate", "adamvs_icp_reduce")


@pytest.fixture(scope="module")
def terrain():
    return I.terrain()


@pytest.fixture(scope="module")
def ref_normals(terrain):
    return R.target_normals(terrain["truth"], I.D, 16)


@pytest.mark.parametrize("n", [0, 1, 257])
def test_rigid_apply_host_equals_the_restatement_bit_for_bit(n):
    x, rot, c, t = I.apply_cases(n)
    y = hip_ops.rigid_apply_host(x, rot, c, t)
    assert y.shape == (n, 3) and same_values(y, R.apply(x, rot, c, t))
    assert np.array_equal(np.isfinite(y).all(1), np.isfinite(x).all(1)) and not np.isfinite(y[~np.isfinite(x).all(1)]).any()
    # the identity about the scene's own centre with t = 0: x - c is exact (c / 2 <= x <= 2 c), so the input's bits come back
    fine = np.isfinite(x).all(1)
    assert same_bits(hip_ops.rigid_apply_host(x, np.eye(3), c, np.zeros(3))[fine], x[fine])


@pytest.mark.parametrize("delta", [0.0, 0.2])
@pytest.mark.parametrize("nq", I.SIZES)
def test_accumulate_and_reduce_twins_equal_the_restatement_bit_for_bit(nq, delta):
    """The twins run the kernels' inline functions and the kernels' order of additions; the restatement is numpy from the header."""
    k = I.accumulate_cases(nq)
    partial = hip_ops.icp_accumulate_host(k["y"], k["index"], k["targets"], k["normals"], k["flag"], k["c"], k["L"], delta)
    sums = hip_ops.icp_reduce_host(partial)
    term, pair = R.rows(k["y"], k["index"], k["targets"], k["normals"], k["flag"], k["c"], k["L"], delta)
    want_partial, want_sums = R.block_sums(term)
    assert partial.shape == (hip_ops.icp_blocks(nq), 32) and same_bits(partial, want_partial)
    assert sums.shape == (32,) and same_bits(sums, want_sums)
    assert sums[30] == pair.sum() and (nq < 100 or 0.3 * nq < pair.sum() < nq)           # the non-pairs are there, and so are pairs
    if delta <= 0:
        assert sums[31] == sums[30] and sums[27] == sums[28]
    elif nq > 60:
        assert sums[31] < sums[30] and sums[27] < sums[28]                                  # Huber weighs some pair down
    # against the exact sum of the restatement's terms: a term passes at most 3 + 6 + 2 + 2 + 8 roundings at these sizes
    for col in range(32):
        exact, scale = math.fsum(term[:, col]), math.fsum(np.abs(term[:, col]))
        assert abs(sums[col] - exact) <= 32 * 2.0 ** -53 * scale, (col, sums[col], exact)


def test_the_sums_do_not_depend_on_the_order_of_the_targets():
    k = I.accumulate_cases(1000)
    perm = np.random.default_rng(2).permutation(len(k["targets"]))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    idx = k["index"].copy()
    ok = (idx >= 0) & (idx < len(perm))
    idx[ok] = inv[idx[ok]]
    a = hip_ops.icp_accumulate_host(k["y"], k["index"], k["targets"], k["normals"], k["flag"], k["c"], k["L"], 0.2)
    b = hip_ops.icp_accumulate_host(k["y"], idx, k["targets"][perm], k["normals"][perm], k["flag"][perm], k["c"], k["L"], 0.2)
    assert same_bits(a, b)


def test_icp_host_recovers_the_motion_of_the_copy_source(terrain):
    """Every source point is a target, so the fixed point is exact.  Measured: icp_host ends at 4.69e-10 m (one ulp of the
    northing) after 4 iterations; the restatement's loop (fp64 brute-force search, eigh normals) ends at 4.69e-10 m after 4.  A
    few targets at the rim of the scene have too few neighbours for a normal and pair with nothing: fitness 0.9995."""
    res = register.icp_host(terrain["copy"], terrain["truth"], I.D, tol=1e-9)
    err = I.estimate_error(res, terrain["copy"], terrain["still_copy"])
    print("icp_host, copy source: %.3e m after %d iterations" % (err, res["iterations"]))
    assert res["converged"] and res["constrained_dof"] == 6 and err <= 1e-7
    assert res["fitness_after"] >= 0.999 and res["rms_point_after"] <= 1e-7
    assert np.abs(res["R"].T @ res["R"] - np.eye(3)).max() <= 1e-12
    M = res["matrix"]
    assert np.abs((terrain["copy"] @ M[:3, :3].T + M[:3, 3]) - terrain["still_copy"]).max() <= 1e-6    # about the origin: 3e6 m times eps


def test_the_restatement_recovers_the_motion_of_the_copy_source(terrain, ref_normals):
    ref = R.icp(terrain["copy"], terrain["truth"], I.D, tol=1e-9, prepared=ref_normals)
    err = I.estimate_error(ref, terrain["copy"], terrain["still_copy"])
    print("restatement, copy source: %.3e m after %d iterations" % (err, ref["iterations"]))
    assert ref["converged"] and err <= 1e-7


def test_icp_host_against_the_restatement_on_the_independent_source(terrain, ref_normals):
    """Measured at tol = 1e-3 D: the restatement reaches 3.08e-3 m against the known motion after 3 iterations, icp_host 3.08e-3 m
    after 3 (the bar: twice the restatement's); no correspondence of 4000 differs at any of the 4 evaluations (seeds 1 and 2), and
    the two transforms agree within 1.5e-14 m over the source."""
    detail = {}
    res = register.icp_host(terrain["independent"], terrain["truth"], I.D, detail=detail)
    ref = R.icp(terrain["independent"], terrain["truth"], I.D, prepared=ref_normals)
    err = I.estimate_error(res, terrain["independent"], terrain["still_independent"])
    ref_err = I.estimate_error(ref, terrain["independent"], terrain["still_independent"])
    differ = [float((np.asarray(a, np.int64) != b).mean()) for a, b in zip(detail["index"], ref["index"])]
    apart = float(np.sqrt(((R.apply(terrain["independent"], res["R"], res["pivot"], res["t"])
                            - R.apply(terrain["independent"], ref["R"], ref["pivot"], ref["t"])) ** 2).sum(1)).max())
    print("independent source: icp_host %.3e m after %d iterations, restatement %.3e m after %d; differing shares %s; apart %.3e m"
          % (err, res["iterations"], ref_err, ref["iterations"], differ, apart))
    assert res["converged"] and ref["converged"] and res["iterations"] == ref["iterations"]
    assert len(differ) == res["iterations"] + 1 and max(differ) <= 1e-3
    if max(differ) == 0.0:
        assert apart <= 1e-9
    assert err <= 2.0 * ref_err
    assert res["fitness_after"] >= res["fitness_before"] and res["rms_plane_after"] < res["rms_plane_before"]


def test_huber_and_init_on_the_independent_source(terrain):
    plain = register.icp_host(terrain["independent"], terrain["truth"], I.D)
    rob = register.icp_host(terrain["independent"], terrain["truth"], I.D, huber=0.05)
    assert rob["converged"] and I.estimate_error(rob, terrain["independent"], terrain["still_independent"]) <= 1e-2
    again = register.icp_host(terrain["independent"], terrain["truth"], I.D, init=plain["matrix"])
    assert again["converged"] and again["iterations"] <= 2
    assert I.estimate_error(again, terrain["independent"], terrain["still_independent"]) <= 1e-2
    none = register.icp_host(terrain["independent"], terrain["truth"], I.D, max_iter=0)
    assert none["iterations"] == 0 and not none["converged"] and np.array_equal(none["R"], np.eye(3)) and not none["t"].any()
    assert none["fitness_before"] == none["fitness_after"] == plain["fitness_before"]


def test_the_flat_scene_constrains_three_freedoms_and_the_others_stay():
    f = I.flat()
    res = register.icp_host(f["source"], f["truth"], I.D)
    print("flat scene: %d iterations, rms_plane %.3e m, t = %s" % (res["iterations"], res["rms_plane_after"], res["t"]))
    assert res["constrained_dof"] == 3 and all(h["kept"] == 3 for h in res["history"]) and res["converged"]
    assert res["rms_plane_after"] <= 1e-9
    assert abs(res["t"][0]) <= 1e-9                      # the 0.3 m slide along the plane is not "corrected"
    assert np.abs(res["R"].T @ res["R"] - np.eye(3)).max() <= 1e-12


def test_the_solve_on_a_hand_made_system():
    # A = diag(4, 1, 1e-9, 2, 2, 2), g = (4, 1, 1, 2, -2, 0): the third freedom falls below 1e-6 lambda_max and stays put
    sums = np.zeros(32)
    at = 0
    diag = (4.0, 1.0, 1e-9, 2.0, 2.0, 2.0)
    for u in range(6):
        for v in range(u, 6):
            sums[at] = diag[u] if u == v else 0.0
            at += 1
    sums[21:27] = (4.0, 1.0, 1.0, 2.0, -2.0, 0.0)
    omega, dt, kept = register.solve(sums, 10.0, 1e-6)
    assert kept == 5 and np.allclose(omega, (-0.1, -0.1, 0.0), atol=1e-15) and np.allclose(dt, (-1.0, 1.0, 0.0), atol=1e-15)
    omega, dt, kept = register.solve(sums, 10.0, 0.0)
    assert kept == 6 and omega[2] == pytest.approx(-1e8, rel=1e-12)
    assert register.solve(np.zeros(32), 1.0)[2] == 0
    assert np.array_equal(register.rodrigues(np.zeros(3)), np.eye(3))
    dR = register.rodrigues(np.deg2rad(I.ANGLE_DEG) * np.asarray(I.AXIS) / np.linalg.norm(I.AXIS))
    assert np.abs(dR - I.rotation(I.AXIS, I.ANGLE_DEG)).max() <= 1e-15
    M = register.matrix_of(dR, np.array([1.0, 2.0, 3.0]), np.array([10.0, 20.0, 30.0]))
    p = np.array([11.0, 19.0, 33.0])
    assert np.allclose(M[:3, :3] @ p + M[:3, 3], dR @ (p - (10.0, 20.0, 30.0)) + (11.0, 22.0, 33.0), atol=1e-13)


def test_options_and_errors(terrain):
    src, tgt = terrain["independent"][:200], terrain["truth"]
    bad = np.eye(4)
    bad[0, 0] = 1.001
    mirror = np.diag([1.0, 1.0, -1.0, 1.0])
    for init in (bad, mirror, np.eye(3), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError, match="init"):
            register.icp_host(src, tgt, I.D, init=init)
    for D in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_dist"):
            register.icp_host(src, tgt, D)
    with pytest.raises(ValueError, match="tol"):
        register.icp_host(src, tgt, I.D, tol=-1e-3)
    for k in (2, 33, 16.0):
        with pytest.raises(ValueError, match="k="):
            register.icp_host(src, tgt, I.D, k=k)
    with pytest.raises(ValueError, match="huber"):
        register.icp_host(src, tgt, I.D, huber=0.0)
    with pytest.raises(ValueError, match="max_iter"):
        register.icp_host(src, tgt, I.D, max_iter=-1)
    with pytest.raises(ValueError, match="min_eig_ratio"):
        register.icp_host(src, tgt, I.D, min_eig_ratio=1.0)
    # fewer than six pairs: five source points, an empty cloud on either side, a source wholly farther than D
    with pytest.raises(_lib.AdaMVSHipError, match="lost: 5 pairs within D"):
        register.icp_host(terrain["truth"][:5], tgt, I.D)
    with pytest.raises(_lib.AdaMVSHipError, match="lost: 0 pairs within D"):
        register.icp_host(np.zeros((0, 3)), tgt, I.D)
    with pytest.raises(_lib.AdaMVSHipError, match="lost: 0 pairs within D"):
        register.icp_host(src, np.zeros((0, 3)), I.D)
    with pytest.raises(_lib.AdaMVSHipError, match="lost: 0 pairs within D"):
        register.icp_host(src + (0.0, 0.0, 30.0), tgt, I.D)
    with pytest.raises(SystemExit, match="not both"):
        register.main(["--recon", "r", "--truth", "t", "--max_dist", "1", "--spacing", "1", "--spacing_voxels", "1"])
    with pytest.raises(ValueError, match="not both"):
        register.from_files("r", "t", 1.0, spacing=1.0, spacing_voxels=1.0)
    a = register.build_parser().parse_args(["--recon", "r.ply", "--truth", "t.ply", "--max_dist", "0.5"])
    assert (a.max_iter, a.tol, a.huber, a.normal_radius, a.k, a.min_eig_ratio) == (50, None, None, None, 16, 1e-6)
    assert a.init is None and a.voxel_down is None and a.spacing is None and a.spacing_voxels is None and a.out is None
    assert register.output_paths("a/b") == ("a/b.json", "a/b.txt", "a/b.ply")


def test_cpu_tensors_raise():
    import torch
    t = torch.zeros(8, 3, dtype=torch.float64)
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        register.icp(t, t, 1.0)
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        hip_ops.rigid_apply(t, np.eye(3), np.zeros(3), np.zeros(3))
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        hip_ops.icp_reduce(torch.zeros(1, 32, dtype=torch.float64))


def test_header_and_bindings_match_both_ways():
    hdr = open(os.path.join(ROOT, "include", "adamvs_hip.h")).read()
    want = {s + e for s in SYMBOLS for e in ("", "_host")}
    declared = {n for n in re.findall(r"\b(adamvs_[a-z0-9_]+)\s*\(", hdr) if n.startswith(("adamvs_rigid_", "adamvs_icp_"))}
    bound = {n for n in _lib.SIGNATURES if n.startswith(("adamvs_rigid_", "adamvs_icp_"))}
    assert declared == bound == want
    lib = _lib.load()
    for name in bound:
        assert hasattr(lib, name)
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "#define ADAMVS_ICP_TERMS %d" % _lib.ICP_TERMS in hdr and "Cloud registration" in hdr
    # argument errors before anything runs
    with pytest.raises(_lib.AdaMVSHipError, match="L="):
        hip_ops.icp_accumulate_host(np.zeros((1, 3)), [0], np.zeros((1, 3)), np.zeros((1, 3)), [0], np.zeros(3), 0.0, 0.0)
    with pytest.raises(_lib.AdaMVSHipError, match="not finite"):
        hip_ops.rigid_apply_host(np.zeros((1, 3)), np.full((3, 3), np.nan), np.zeros(3), np.zeros(3))
