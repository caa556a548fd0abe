"""Mesh simplification on the GPU (csrc/mesh_simplify.hip through ada_mvs_amd/simplify.py) against the restatement
(tests/simplify_ref.py).  Cells, the faces' cells, the survive / duplicate / used decisions, the face list, the vertex order, the
colours and every count are compared exactly; ranks and fallback flags exactly outside tied cells; positions outside tied cells
to 1e-9 c + 2 spacing(|coordinate|) (the sums differ only in order, ~n 2^-53 relative with n <= 1e4 entries, times the kept
part's condition <= 1 / rank_eps = 1e3: <= ~1e-11 c, two decades of margin; the second term is the final fp64 add).  Tied cells
(a rank or an in-cell decision within the restatement's tie window) may be at most 0.1 % of the cells."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, fusion_synth, hip_ops, mesh, simplify, texture
from conftest import ROOT
import simplify_inputs as I
import simplify_ref as S
from test_mesh_gpu import B, MU, OFFSET, ORIGIN, VOXEL, scene_views, surface_distance

pytestmark = pytest.mark.gpu

BRICKS = [(x, y, z) for x in (2, 3, 4) for y in (2, 3, 4) for z in (0, 1)]
SCENE_SHIFT = np.array([0.37, 0.21, 0.53])         # lattice origin = ORIGIN - SCENE_SHIFT c


def run_gpu(xyz, rgb, faces, cell, origin, **kw):
    """simplify() on numpy inputs -> dict of numpy arrays: the result, the intermediates and info."""
    import torch
    detail = {}
    x, c, f, info = simplify.simplify(torch.from_numpy(np.ascontiguousarray(xyz, np.float64)).cuda(),
                                      torch.from_numpy(np.ascontiguousarray(rgb, np.uint8)).cuda(),
                                      torch.from_numpy(np.ascontiguousarray(faces).astype(np.int64)).cuda(), cell, origin, detail=detail, **kw)
    out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in detail.items()}
    out.update(out_xyz=x.cpu().numpy(), out_rgb=c.cpu().numpy(), out_faces=f.cpu().numpy().view(np.uint32).astype(np.int64), info=info)
    return out


def hold(g, r, cell, bitwise=False):
    """The GPU run g against the restatement r as the module docstring says -> the largest position error over its bound."""
    assert np.array_equal(g["keys"], r["keys"])
    assert np.array_equal(g["vcell"], r["vcell"])
    assert np.array_equal(g["fcell"], r["fcell"])
    assert np.array_equal(g["survive"].astype(bool), r["survive"])
    assert np.array_equal(g["keep"].astype(bool), r["keep"])
    assert np.array_equal(g["used"].astype(bool), r["used"])
    assert np.array_equal(g["col"], r["col"])
    assert np.array_equal(g["out_faces"], r["faces"])
    assert np.array_equal(g["out_rgb"], r["rgb"])
    for k in ("cells", "cells_used", "vertices_in", "faces_in", "faces_collapsed", "faces_duplicate", "faces_out"):
        assert g["info"][k] == r["info"][k], (k, g["info"][k], r["info"][k])
    tied = r["rank_tie"] | r["box_tie"]
    assert tied.mean() <= 1e-3, (int(tied.sum()), len(tied))
    ok = ~tied
    assert np.array_equal(g["rank"][ok], r["rank"][ok])
    assert np.array_equal(g["fallback"][ok].astype(bool), r["fallback"][ok])
    if not tied.any():
        assert g["info"]["rank_hist"] == r["info"]["rank_hist"] and g["info"]["fallbacks"] == r["info"]["fallbacks"]
    assert g["out_xyz"].tobytes() == g["pos"][g["used"].astype(bool)].tobytes()
    # the reported error p.A p + 2 b.p + sum d^2 cancels: held to 1e-9 of the sum of its terms' magnitudes
    pr = r["pos"] - r["centre"]
    scale = np.abs(np.einsum("ni,nij,nj->n", pr, r["A"], pr)) + 2 * np.abs(np.einsum("ni,ni->n", r["b"], pr)) + r["dd"]
    assert (np.abs(g["error"] - r["error"])[ok] <= 1e-9 * scale[ok] + 1e-300).all()
    if bitwise:
        assert g["pos"].tobytes() == r["pos"].tobytes(), np.abs(g["pos"] - r["pos"]).max()
        return 0.0
    bound = 1e-9 * cell + 2 * np.spacing(np.abs(r["pos"]))
    ratio = (np.abs(g["pos"] - r["pos"]) / bound)[ok]
    worst = float(ratio.max())
    print("simplify: %d cells, %d tied, largest position error / bound = %.3g" % (len(tied), int(tied.sum()), worst))
    assert worst <= 1.0, worst
    return worst


def inside_cells(pos, centre, cell):
    """Every representative in its cell's closed box, up to the rounding of centre + p (p itself is held to |p_k| <= c / 2)."""
    return bool((np.abs(pos - centre) <= cell / 2 + 2 * np.spacing(np.abs(pos))).all())


# ---- 1. the hand-made mesh, the empty mesh, the refusals ---------------------------------------------------------------------
def test_hand_made_mesh_bit_for_bit():
    xyz, rgb, faces, cell, origin = I.hand_mesh()
    r = S.simplify(xyz, rgb, faces, cell, origin)
    # the mesh has what it is meant to have (read off the restatement)
    assert set(r["rank"]) == {1, 2, 3} and r["fallback"].sum() == 1 and r["rank"][r["fallback"]].tolist() == [2]
    assert r["info"]["faces_collapsed"] == 3 and r["info"]["faces_duplicate"] == 1 and r["info"]["faces_out"] == 8
    assert r["keep"][3] and r["survive"][4] and not r["keep"][4]                     # of the folded pair the first survives
    assert (~r["used"]).sum() == 1 and len(xyz) == r["info"]["vertices_in"] == 26
    assert not (r["rank_tie"] | r["box_tie"]).any()
    referenced = np.zeros(len(xyz), bool)
    referenced[faces.ravel()] = True
    assert (~referenced).sum() == 1 and (xyz[:, 0] == 1.0).any()
    g = run_gpu(xyz, rgb, faces, cell, origin)
    hold(g, r, cell, bitwise=True)
    assert g["out_xyz"].tobytes() == r["xyz"].tobytes()
    # the quadrics themselves: every sum of this mesh is exact
    A = r["A"][:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    assert np.array_equal(g["quadric"], np.concatenate([A, r["b"], r["dd"][:, None]], 1))
    assert np.array_equal(g["member"] / r["count"][:, None], r["mean"])


def test_empty_mesh():
    import torch
    x, c, f, info = simplify.simplify(torch.empty(0, 3, dtype=torch.float64).cuda(), torch.empty(0, 3, dtype=torch.uint8).cuda(),
                                      torch.empty(0, 3, dtype=torch.int64).cuda(), 1.0, (0.0, 0.0, 0.0))
    assert tuple(x.shape) == (0, 3) and tuple(c.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    assert info["cells"] == info["cells_used"] == info["faces_in"] == info["faces_out"] == 0
    # vertices without faces: every cell goes unused
    xyz, rgb, _, cell, origin = I.hand_mesh()
    g = run_gpu(xyz, rgb, np.zeros((0, 3), np.int64), cell, origin)
    assert g["out_xyz"].shape == (0, 3) and g["out_faces"].shape == (0, 3) and g["info"]["cells"] == 13


@pytest.mark.parametrize("case", ["nan", "inf", "beyond", "below"])
def test_bad_coordinates_are_errors_not_clamps(case, tmp_path):
    import torch
    xyz, rgb, faces, cell, origin = I.hand_mesh()
    xyz = xyz.copy()
    xyz[7, 1] = {"nan": np.nan, "inf": np.inf, "beyond": float(1 << 21) + 0.5, "below": -0.25}[case]
    keys, bad = hip_ops.simplify_keys(torch.from_numpy(xyz).cuda(), cell, origin)
    keys, bad = keys.cpu().numpy(), bad.cpu().numpy()
    assert bad[7] == (1 if case in ("nan", "inf") else 2) and keys[7] == -1 and (bad[np.arange(len(xyz)) != 7] == 0).all()
    with pytest.raises(_lib.AdaMVSHipError):
        run_gpu(xyz, rgb, faces, cell, origin)
    # through the file interface nothing is written
    src, out = str(tmp_path / "m.ply"), str(tmp_path / "s.ply")
    with mesh.MeshPlyWriter(src) as w:
        w.write(xyz, rgb, faces.astype(np.uint32))
    with pytest.raises(_lib.AdaMVSHipError):
        simplify.from_file(src, out=out, cell=cell, origin=origin, log=lambda *a: None)
    assert not os.path.exists(out) and not os.path.exists(out + ".json")


# ---- 2. and 3. the sphere and the box ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    return I.sphere_mesh()


@pytest.fixture(scope="module")
def box():
    return I.box_mesh()


@pytest.mark.parametrize("cell", I.CELLS)
def test_sphere(sphere, cell):
    xyz, rgb, faces = sphere
    r = S.simplify(xyz, rgb, faces, cell, I.LATTICE_ORIGIN)
    assert (r["info"]["vertices_in"], r["info"]["faces_in"]) == (5628, 11252)
    g = run_gpu(xyz, rgb, faces, cell, I.LATTICE_ORIGIN)
    hold(g, r, cell)
    e = I.SPHERE_EXPECT[cell]
    i = g["info"]
    assert (i["cells"], i["faces_out"], i["faces_duplicate"], i["fallbacks"]) == (e["cells"], e["faces_out"], e["faces_duplicate"], e["fallbacks"])
    assert inside_cells(g["pos"], r["centre"], cell)
    dist = np.abs(np.linalg.norm(g["out_xyz"] - np.asarray(I.SPHERE_CENTRE), axis=1) - I.SPHERE_RADIUS)
    assert dist.max() <= e["dist"], dist.max()


@pytest.mark.parametrize("cell", I.CELLS)
def test_box(box, cell):
    from mesh_ref import closed_and_oriented
    xyz, rgb, faces = box
    r = S.simplify(xyz, rgb, faces, cell, I.LATTICE_ORIGIN)
    assert (r["info"]["vertices_in"], r["info"]["faces_in"]) == (7938, 15872)
    g = run_gpu(xyz, rgb, faces, cell, I.LATTICE_ORIGIN)
    hold(g, r, cell)
    closed, chi = closed_and_oriented(g["out_faces"])
    assert closed and chi == 2
    assert g["info"]["faces_out"] == I.BOX_EXPECT[cell]["faces_out"]
    assert tuple(g["info"]["rank_hist"][1:]) == I.BOX_EXPECT[cell]["rank_hist"] and g["info"]["rank_hist"][0] == 0
    assert inside_cells(g["pos"], r["centre"], cell)


# ---- 4. - 7. the analytic scene ------------------------------------------------------------------------------------------------
def brick_meshes(mesher):
    """The unwelded concatenation of BRICKS' meshes, device tensors (faces int64)."""
    import torch
    xs, cs, fs, base = [], [], [], 0
    for b in BRICKS:
        xyz, rgb, f = mesher.brick(b, base)
        xs.append(xyz), cs.append(rgb), fs.append(f.to(torch.int64) & 0xFFFFFFFF)
        base += xyz.shape[0]
    return torch.cat(xs), torch.cat(cs), torch.cat(fs)


@pytest.fixture(scope="module")
def scene():
    """The welded mesh of BRICKS of test_mesh_gpu.py's scene (numpy), the unwelded one, and the restatement per cell size."""
    ux, uc, uf = brick_meshes(mesh.TsdfMesher(ORIGIN, VOXEL, MU, B, scene_views()))
    wx, wf, wc = mesh.weld(ux, uf, uc)
    sc = dict(xyz=wx.cpu().numpy(), rgb=wc.cpu().numpy(), faces=wf.cpu().numpy(), unwelded=(ux.cpu().numpy(), uc.cpu().numpy(), uf.cpu().numpy()),
              ref={}, gpu={})
    assert 80000 < len(sc["xyz"]) < len(ux) and len(sc["faces"]) > 150000
    return sc


def scene_ref(sc, cell):
    if cell not in sc["ref"]:
        sc["ref"][cell] = S.simplify(sc["xyz"], sc["rgb"], sc["faces"], cell, ORIGIN - SCENE_SHIFT * cell)
    return sc["ref"][cell]


def scene_gpu(sc, cell):
    if cell not in sc["gpu"]:
        sc["gpu"][cell] = run_gpu(sc["xyz"], sc["rgb"], sc["faces"], cell, ORIGIN - SCENE_SHIFT * cell)
    return sc["gpu"][cell]


@pytest.mark.parametrize("cell", [2.0, 4.0])
def test_analytic_scene(scene, cell):
    # the restatement on the CPU-integrated volume: 5 608 / 1 559 cells, 10 760 / 3 033 faces, 239 / 381 duplicates, 203 / 98 fallbacks
    r, g = scene_ref(scene, cell), scene_gpu(scene, cell)
    hold(g, r, cell)
    assert g["info"]["cells"] > 1000 and g["info"]["faces_duplicate"] > 0 and g["info"]["fallbacks"] > 0
    assert g["info"]["faces_out"] < g["info"]["faces_in"] / 8
    assert inside_cells(g["pos"], r["centre"], cell)
    d = surface_distance(g["out_xyz"]) / VOXEL
    print("simplify: scene c = %g: median %.3f, 99th percentile %.3f voxel" % (cell, np.median(d), np.percentile(d, 99)))
    assert np.median(d) <= 0.25 and np.percentile(d, 99) <= 1.0, (np.median(d), np.percentile(d, 99))


@pytest.mark.parametrize("cell", [4.0])
def test_far_from_the_origin(scene, cell):
    near = scene_gpu(scene, cell)
    ux, uc, uf = brick_meshes(mesh.TsdfMesher(ORIGIN + OFFSET, VOXEL, MU, B, scene_views(OFFSET)))
    x, c, f, info = simplify.simplify(ux, uc, uf, cell, ORIGIN + OFFSET - SCENE_SHIFT * cell)
    assert np.array_equal(f.cpu().numpy().view(np.uint32).astype(np.int64), near["out_faces"])
    assert np.array_equal(c.cpu().numpy(), near["out_rgb"])
    assert {k: v for k, v in info.items() if k != "quadric_error"} == {k: v for k, v in near["info"].items() if k != "quadric_error"}
    assert np.abs(x.cpu().numpy() - OFFSET - near["out_xyz"]).max() <= 1e-3


def test_bit_identical_runs(scene):
    a = run_gpu(scene["xyz"], scene["rgb"], scene["faces"], 4.0, ORIGIN - SCENE_SHIFT * 4.0)
    b = run_gpu(scene["xyz"], scene["rgb"], scene["faces"], 4.0, ORIGIN - SCENE_SHIFT * 4.0)
    for k in ("out_xyz", "out_rgb", "out_faces", "quadric", "member", "colour", "pos", "rank", "fallback", "error", "keep", "used"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert a["info"] == b["info"]


def test_independent_of_welding_and_of_the_order_of_the_faces(scene):
    cell = 4.0
    g = scene_gpu(scene, cell)
    u = run_gpu(*scene["unwelded"], cell, ORIGIN - SCENE_SHIFT * cell)
    for k in ("out_xyz", "out_rgb", "out_faces"):
        assert u[k].tobytes() == g[k].tobytes(), k
    perm = np.random.default_rng(7).permutation(len(scene["faces"]))
    p = run_gpu(scene["xyz"], scene["rgb"], scene["faces"][perm], cell, ORIGIN - SCENE_SHIFT * cell)
    assert p["out_xyz"].tobytes() == g["out_xyz"].tobytes() and p["out_rgb"].tobytes() == g["out_rgb"].tobytes()
    sets = lambda f: set(map(tuple, np.sort(f, 1).tolist()))  # noqa: E731
    assert len(p["out_faces"]) == len(g["out_faces"]) and sets(p["out_faces"]) == sets(g["out_faces"])
    assert not np.array_equal(p["out_faces"], g["out_faces"])


# ---- 8. end to end: predict's output layout -> fuse_whu.py -> mesh_whu.py -> simplify_whu.py -> texture_whu.py --------------
def _run(args, timeout=300):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_simplify_whu_end_to_end(tmp_path):
    sc = fusion_synth.scene(192, 256, 4, offset=OFFSET, seed=13)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    fusion_synth.write_predict_layout(sc, data, out)
    _run([os.path.join(ROOT, "fuse_whu.py"), "--data_folder", data, "--output_folder", out])
    _run([os.path.join(ROOT, "mesh_whu.py"), "--data_folder", data, "--output_folder", out, "--voxel", "1.0", "--brick", "32"])
    r = _run([os.path.join(ROOT, "simplify_whu.py"), "--output_folder", out, "--cell_voxels", "3"])
    assert "argv:" in r.stdout and "total_time" in r.stdout
    cli = os.path.join(out, "mesh_simplified.ply")
    api = str(tmp_path / "api" / "mesh_simplified.ply")
    res = simplify.from_file(os.path.join(out, "mesh.ply"), out=api, cell_voxels=3, log=lambda *a: None)
    assert open(cli, "rb").read() == open(api, "rb").read()
    src, meta = json.load(open(os.path.join(out, "mesh.ply.json"))), json.load(open(cli + ".json"))
    for k in ("voxel", "mu", "origin", "views"):
        assert meta[k] == src[k], k
    for k in ("cell", "lattice_origin", "source", "cells", "cells_used", "vertices_in", "faces_in", "faces_collapsed", "faces_duplicate", "faces_out",
              "rank_hist", "fallbacks", "vertices", "faces", "seconds", "device_seconds"):
        assert k in meta, k
    assert meta["cell"] == 3.0 and meta["lattice_origin"] == [v - 1.0 for v in src["origin"]]
    assert meta["faces_in"] == src["faces"] and meta["faces"] == res["faces"] == meta["faces_out"] and 0 < meta["faces"] < src["faces"] / 4
    verts, faces = mesh.read_mesh_ply(cli)
    assert len(verts) == meta["vertices"] and len(faces) == meta["faces"] and faces.max() < len(verts)
    _run([os.path.join(ROOT, "texture_whu.py"), "--data_folder", data, "--output_folder", out, "--mesh", cli, "--page", "1024"])
    ply = texture.read_textured_ply(os.path.join(out, "mesh_textured.ply"))
    assert len(ply["faces"]) == len(faces)
