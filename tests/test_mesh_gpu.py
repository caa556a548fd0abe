"""TSDF mesh on the GPU (csrc/mesh.hip through ada_mvs_amd/mesh.py) against the restatement (tests/mesh_ref.py): integration
(weights and colours exactly, the tsdf within the header's bound, outside the tie margin), extraction bit for bit on the
GPU-produced volume, bit-identical brick seams, a closed sphere, the geometry and facades of the analytic scene, the scene far
from the origin, run-to-run identity and mesh_whu.py end to end."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import fusion_synth, mesh
from conftest import ROOT
import mesh_ref as M

pytestmark = pytest.mark.gpu

OFFSET = np.array([5e5, 3.4e6, 0.0])
ORIGIN = np.array([-112.0, -112.0, -8.0])
VOXEL, MU, B = 1.0, 4.0, 32
NB = (7, 7, 3)
# bricks with terrain, walls and roofs in them
PROBE = [(3, 3, 0), (1, 2, 1), (4, 2, 0)]


def scene_views(offset=(0.0, 0.0, 0.0), seed=5):
    import torch
    sc = fusion_synth.scene(192, 256, 4, offset=offset, seed=seed)
    views = []
    for c, d in zip(sc["cams"], sc["depths"]):
        rgba = fusion_synth.texture(c, d.astype(np.float64))
        views.append(dict(K=c["K"], R=c["R"], C=c["C"], depth=torch.from_numpy(d).cuda(), rgba=torch.from_numpy(rgba).cuda(),
                          depth_h=d, rgba_h=rgba))
    return views


def records(views, origin):
    return [M.view_record(v["K"], v["R"], v["C"], origin, v["depth_h"], v["rgba_h"]) for v in views]


def host(vol):
    t, w, c = vol
    return t.cpu().numpy(), w.cpu().numpy().view(np.uint16), c.cpu().numpy().view(np.uint32)


def whole_mesh(mesher, nb=NB):
    xs, cs, fs, base = [], [], [], 0
    for b in itertools.product(range(nb[0]), range(nb[1]), range(nb[2])):
        if not mesher.view_list(b):
            continue
        xyz, rgb, f = mesher.brick(b, base)
        xs.append(xyz.cpu().numpy())
        cs.append(rgb.cpu().numpy())
        fs.append(f.cpu().numpy().view(np.uint32))
        base += len(xs[-1])
    return np.concatenate(xs), np.concatenate(cs), np.concatenate(fs).astype(np.int64)


def surface_distance(P):
    """Distance to the analytic scene: the terrain z = 0 or a box's boundary, whichever is nearer (local coordinates)."""
    d = np.abs(P[:, 2])
    for x0, x1, y0, y1, h in fusion_synth.BOXES:
        lo, hi = np.array([x0, y0, 0.0]), np.array([x1, y1, h])
        q = np.maximum(np.maximum(lo - P, P - hi), 0)
        inside = (q == 0).all(1)
        d = np.minimum(d, np.where(inside, np.minimum(P - lo, hi - P).min(1), np.linalg.norm(q, axis=1)))
    return d


@pytest.fixture(scope="module")
def scene():
    views = scene_views()
    return views, mesh.TsdfMesher(ORIGIN, VOXEL, MU, B, views)


# ---- integration and extraction against the restatement --------------------------------------------------------------------
@pytest.mark.parametrize("b", PROBE)
def test_integration_matches_restatement(scene, b):
    views, mesher = scene
    vl = mesher.view_list(b)
    assert len(vl) >= 3
    t, w, c = host(mesher.integrate(b, vl))
    ref = M.integrate(VOXEL, MU, B, b, records(views, ORIGIN), vl)
    ok = ~ref["tie"]
    # the margin is the header's whole error bound for every view of the list: it flags 13-15 % of these bricks' samples
    assert ok.mean() > 0.8, ok.mean()
    assert np.array_equal(w[ok], ref["weight"][ok]), np.argwhere(w[ok] != ref["weight"][ok])[:5]
    assert np.array_equal(c[ok], ref["rgba"][ok])
    bound = M.tsdf_bound(VOXEL, MU, B, b, records(views, ORIGIN), vl, ref["weight"])
    err = np.abs(t.astype(np.float64) - ref["tsdf64"])
    assert (err[ok] <= bound[ok]).all(), (err[ok] - bound[ok]).max()
    assert (w > 0).mean() > 0.2 and (c != 0).any()


@pytest.mark.parametrize("b", PROBE)
@pytest.mark.parametrize("min_weight", [1, 3])
def test_extraction_matches_restatement_on_the_gpu_volume(scene, b, min_weight):
    import torch
    views, mesher = scene
    vol = mesher.integrate(b)
    t, w, c = host(vol)
    m2 = mesh.TsdfMesher(ORIGIN, VOXEL, MU, B, views, min_weight=min_weight)
    xyz, rgb, faces = m2.extract(b, vol, vertex_base=1234)
    ref = M.extract(ORIGIN, VOXEL, B, b, t, w, c, min_weight, 1234)
    assert len(ref["faces"]) > 100
    assert xyz.cpu().numpy().tobytes() == ref["xyz"].tobytes()
    assert np.array_equal(rgb.cpu().numpy(), ref["rgb"])
    assert np.array_equal(faces.cpu().numpy().view(np.uint32), ref["faces"])
    torch.cuda.synchronize()


# ---- seams --------------------------------------------------------------------------------------------------------------------
def test_shared_layers_of_adjacent_bricks_are_bit_identical(scene):
    _, mesher = scene
    B1 = B + 1
    a = [x.reshape(B1, B1, B1) for x in host(mesher.integrate((3, 3, 0)))]
    for b, sl_a, sl_b in (((4, 3, 0), np.s_[:, :, B], np.s_[:, :, 0]), ((3, 4, 0), np.s_[:, B, :], np.s_[:, 0, :]),
                          ((3, 3, 1), np.s_[B, :, :], np.s_[0, :, :])):
        o = [x.reshape(B1, B1, B1) for x in host(mesher.integrate(b))]
        for u, v in zip(a, o):
            assert u[sl_a].tobytes() == v[sl_b].tobytes(), b
    assert (a[1] > 0).any()


def test_uploaded_sphere_over_eight_bricks_is_closed():
    import torch
    centre = (32.37, 31.81, 32.23)
    vol = M.sphere_volume(B, centre, 10.0, 4.0)
    views = scene_views()[:1]
    mesher = mesh.TsdfMesher((0.0, 0.0, 0.0), 1.0, 4.0, B, views)
    xs, cs, fs, base = [], [], [], 0
    for b in sorted(vol):
        t, w, c = vol[b]
        dev = (torch.from_numpy(t).cuda(), torch.from_numpy(w.view(np.int16)).cuda(), torch.from_numpy(c.view(np.int32)).cuda())
        xyz, rgb, f = mesher.extract(b, dev, base)
        ref = M.extract((0.0, 0.0, 0.0), 1.0, B, b, t, w, c, 1, base)
        assert xyz.cpu().numpy().tobytes() == ref["xyz"].tobytes() and np.array_equal(f.cpu().numpy().view(np.uint32), ref["faces"])
        xs.append(xyz), cs.append(rgb), fs.append(f.to(torch.int64))
        base += xyz.shape[0]
    u, f, rgb = mesh.weld(torch.cat(xs), torch.cat(fs), torch.cat(cs))
    u, f = u.cpu().numpy(), f.cpu().numpy()
    assert len(u) < base
    closed, chi = M.closed_and_oriented(f)
    assert closed and chi == 2
    assert abs(M.signed_volume(u - np.asarray(centre), f) / (4.0 / 3.0 * np.pi * 1000.0) - 1.0) < 0.01


# ---- the analytic scene -------------------------------------------------------------------------------------------------------
def test_geometry_and_facades_of_the_analytic_scene(scene):
    _, mesher = scene
    xyz, _, f = whole_mesh(mesher)
    # the restatement on CPU gave median 0.069 voxel, 99th percentile 0.73 voxel, walls covered 0.49 at this scene
    d = surface_distance(xyz) / VOXEL
    assert np.median(d) <= 0.25 and np.percentile(d, 99) <= 1.0, (np.median(d), np.percentile(d, 99))
    p = xyz[f]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    area = np.linalg.norm(n, axis=1) / 2
    nz = np.abs(n[:, 2]) / np.maximum(2 * area, 1e-30)
    cen = p.mean(1)
    near = np.zeros(len(f), bool)
    wall_area = 0.0
    for x0, x1, y0, y1, h in fusion_synth.BOXES:
        wall_area += 2 * (x1 - x0) * h + 2 * (y1 - y0) * h
        inz = (cen[:, 2] > 0.5) & (cen[:, 2] < h - 0.5)
        for ax, val, lo, hi in ((0, x0, y0, y1), (0, x1, y0, y1), (1, y0, x0, x1), (1, y1, x0, x1)):
            near |= inz & (np.abs(cen[:, ax] - val) < 1.5) & (cen[:, 1 - ax] > lo) & (cen[:, 1 - ax] < hi)
    frac = area[(nz < 0.3) & near].sum() / wall_area
    assert frac >= 0.4, frac


def test_far_from_the_origin():
    views = scene_views(OFFSET)
    far = mesh.TsdfMesher(ORIGIN + OFFSET, VOXEL, MU, B, views)
    near = mesh.TsdfMesher(ORIGIN, VOXEL, MU, B, scene_views())
    for b in PROBE:
        xa, ca, fa = (x.cpu().numpy() for x in far.brick(b))
        xb, cb, fb = (x.cpu().numpy() for x in near.brick(b))
        assert np.array_equal(fa, fb) and np.array_equal(ca, cb)
        assert np.abs(xa - OFFSET - xb).max() <= 1e-3


def test_bit_identical_runs(scene):
    _, mesher = scene
    for b in PROBE[:2]:
        r1 = [x.cpu().numpy() for x in mesher.integrate(b) + mesher.brick(b)]
        r2 = [x.cpu().numpy() for x in mesher.integrate(b) + mesher.brick(b)]
        for u, v in zip(r1, r2):
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()


# ---- end to end: predict's output layout -> fuse_whu.py -> mesh_whu.py ------------------------------------------------------
def test_mesh_whu_end_to_end(tmp_path):
    sc = fusion_synth.scene(192, 256, 4, offset=OFFSET, seed=13)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    fusion_synth.write_predict_layout(sc, data, out)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fuse_whu.py"), "--data_folder", data, "--output_folder", out],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    cli = str(tmp_path / "cli" / "mesh.ply")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mesh_whu.py"), "--data_folder", data, "--output_folder", out, "--voxel", "1.0",
                        "--brick", "32", "--out", cli], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "total_time" in r.stdout
    api = str(tmp_path / "api" / "mesh.ply")
    res = mesh.from_folder(data, out, voxel=1.0, brick=32, out=api, log=lambda *a: None)
    assert open(cli, "rb").read() == open(api, "rb").read()
    meta = json.load(open(cli + ".json"))
    for k in ("voxel", "mu", "min_weight", "origin", "grid", "brick", "bricks_total", "bricks_active", "views", "vertices", "faces",
              "seconds", "device_seconds", "device_bytes"):
        assert k in meta, k
    assert meta["vertices"] == res["vertices"] > 1000 and meta["faces"] == res["faces"] and meta["views"] == 5
    assert 0 < meta["bricks_active"] < meta["bricks_total"]
    verts, faces = mesh.read_mesh_ply(cli)
    assert len(verts) == meta["vertices"] and len(faces) == meta["faces"] and faces.max() < len(verts)
    xyz = np.stack([verts["x"], verts["y"], verts["z"]], 1) - OFFSET
    p = xyz[faces.astype(np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    nz = np.abs(n[:, 2]) / np.maximum(np.linalg.norm(n, axis=1), 1e-30)
    assert (nz < 0.3).mean() > 0.02                            # walls on the boxes' sides (3.0 % of the faces measured)
    # --weld merges the seams: fewer vertices, the same number of faces
    welded = mesh.from_folder(data, out, voxel=1.0, brick=32, out=str(tmp_path / "w" / "mesh.ply"), weld_mesh=True, log=lambda *a: None)
    assert welded["faces"] == res["faces"] and welded["vertices"] < res["vertices"]
