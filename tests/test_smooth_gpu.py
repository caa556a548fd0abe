"""Mesh smoothing on the GPU (csrc/mesh_smooth.hip through ada_mvs_amd/smooth.py) against the restatement (tests/smooth_ref.py).
On the hand-made mesh (coordinates in eighths) the face records, the boundary marks and the incidence are compared exactly and
the normals to 1e-12 after 0, 1 and 3 passes.  On the strips, the fan, the box and the sphere the fixed marks and the clamp
counts are compared exactly and the positions to 1e-9 voxel + 2 spacing(|coordinate|), the bound simplify's positions are held
to: the two sides run the same operations in the same order and differ only in exp (a few 2^-53 per weight), which ten passes
of a contraction (normalised means, projections) do not amplify, so the first term has decades of margin; the second term is
the final fp64 add of the origin.  Measured on an MI355X: at most 1.4e-5 of the bound (one unit in the last place of a
coordinate)."""
import json

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, hip_ops, mesh, simplify, smooth
import clean_ref as CR
import simplify_inputs as I
import smooth_inputs as SI
import smooth_ref as R

pytestmark = pytest.mark.gpu

OFFSET = np.array([5e5, 3.4e6, 0.0])          # dyadic: exact to add to coordinates that are multiples of 2^-16 below 2^7


def run_gpu(xyz, rgb, faces, **kw):
    """smooth() on numpy inputs -> dict of numpy arrays: the result, the intermediates and info."""
    import torch
    detail = {}
    x, c, f, info = smooth.smooth(torch.from_numpy(np.ascontiguousarray(xyz, np.float64)).cuda(),
                                  torch.from_numpy(np.ascontiguousarray(rgb, np.uint8)).cuda(),
                                  torch.from_numpy(np.ascontiguousarray(faces).astype(np.int64)).cuda(), detail=detail, **kw)
    out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in detail.items()}
    out.update(out_xyz=x.cpu().numpy(), out_rgb=c.cpu().numpy(), out_faces=f.cpu().numpy().view(np.uint32).astype(np.int64), info=info)
    return out


def runs_of(g):
    """The vertex -> face runs of a GPU run as lists."""
    return [g["vface"][a:b].tolist() for a, b in zip(g["vstart"][:-1], g["vstart"][1:])]


def hold(g, r, voxel=1.0, what=""):
    """The GPU run g against the restatement r as the module docstring says -> the largest position error over its bound."""
    assert np.array_equal(g["out_faces"], r["faces"]) and np.array_equal(g["out_rgb"], r["rgb"])
    assert np.array_equal(g["fixed"].astype(bool), r["fixed"])
    assert np.array_equal(g["clamped"].astype(bool), r["clamped"])
    assert np.array_equal(g["moved"].astype(bool), r["moved"])
    for k in ("vertices", "faces", "fixed", "degenerate_faces", "clamped"):
        assert g["info"][k] == r["info"][k], (k, g["info"][k], r["info"][k])
    assert np.abs(g["normals"] - r["normals"]).max() <= 1e-12
    bound = 1e-9 * voxel + 2 * np.spacing(np.abs(r["xyz"]))
    worst = float((np.abs(g["out_xyz"] - r["xyz"]) / bound).max())
    print("smooth: %s %d vertices, %d faces, %d fixed, %d clamped, largest position error / bound = %.3g"
          % (what, len(r["xyz"]), len(r["faces"]), r["info"]["fixed"], r["info"]["clamped"], worst))
    assert worst <= 1.0, worst
    assert g["out_xyz"][~r["moved"]].tobytes() == r["xyz"][~r["moved"]].tobytes()
    assert abs(g["info"]["largest_move"] - r["info"]["largest_move"]) <= 1e-9 * voxel
    assert abs(g["info"]["rms_move"] - r["info"]["rms_move"]) <= 1e-9 * voxel
    return worst


# ---- the hand-made mesh ---------------------------------------------------------------------------------------------------------
HAND = dict(sigma_s=1.0, sigma_r=0.35, max_move=1.0)


def test_hand_made_mesh_records_marks_and_incidence_exactly():
    xyz, rgb, faces = SI.hand_mesh()
    r = R.smooth(xyz, rgb, faces, normal_iters=0, vertex_iters=0, **HAND)
    g = run_gpu(xyz, rgb, faces, normal_iters=0, vertex_iters=0, **HAND)
    assert g["xyz"].tobytes() == R.weld(xyz, rgb, faces)[0].tobytes() and np.array_equal(g["faces"], r["faces"])
    assert g["rec"][:, 0:3].tobytes() == np.ascontiguousarray(r["centroid"]).tobytes()
    assert g["rec"][:, 3].tobytes() == np.ascontiguousarray(r["area"]).tobytes()
    assert g["rec"][:, 4:7].tobytes() == np.ascontiguousarray(r["n0"]).tobytes() and (g["rec"][:, 7] == 0).all()
    assert np.array_equal(g["fixed"].astype(bool), r["fixed"]) and 0 < r["fixed"].sum() < len(r["fixed"])
    assert runs_of(g) == r["F"] and g["vstart"][-1] == 3 * len(faces)
    assert g["info"]["degenerate_faces"] == 2 and g["info"]["fixed"] == int(r["fixed"].sum())
    free = run_gpu(xyz, rgb, faces, normal_iters=0, vertex_iters=0, fix_boundary=False, **HAND)
    assert not free["fixed"].any()


@pytest.mark.parametrize("iters", [0, 1, 3])
def test_hand_made_mesh_normals(iters):
    xyz, rgb, faces = SI.hand_mesh()
    r = R.smooth(xyz, rgb, faces, normal_iters=iters, vertex_iters=2, fix_boundary=False, **HAND)
    g = run_gpu(xyz, rgb, faces, normal_iters=iters, vertex_iters=2, fix_boundary=False, **HAND)
    assert np.abs(g["normals"] - r["normals"]).max() <= 1e-12
    # the cancelling face keeps the zero vector exactly; its two neighbours stay opposite
    f = int(np.nonzero((r["area"] == 0) & (np.array([len(n) for n in r["N"]]) == 3))[0][0])
    assert (g["normals"][f] == 0).all()
    hold(g, r, what="hand-made, %d passes:" % iters)


# ---- kernel edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", list(SI.EDGE_TILE_FACES) + [255, 256, 257])
def test_strips_across_a_workgroup_boundary(nf):
    import torch
    xyz, rgb, faces = SI.strip(nf)
    # the edge keys alone (one lane per edge), with vertex numbers that have bit 31 set: both entry points against the half-edges of
    # the cleaning restatement; then the marks of the vertices below nf against the restatement on the strip before the renaming
    big, bits = SI.renamed_strip_faces(nf)
    f32 = torch.from_numpy(bits).cuda()
    tail, head = CR.half_edges(big)
    want = (np.minimum(tail, head) << 32) | np.maximum(tail, head)
    keys = hip_ops._edge_keys("smooth_edge_keys", f32).cpu().numpy()
    assert keys.tobytes() == want.tobytes() and (want < 0).sum() == 1 and (want & 0x80000000 != 0).sum() >= 3
    assert hip_ops.texture_edge_keys(f32).cpu().numpy().tobytes() == keys.tobytes()
    fixed = hip_ops.smooth_boundary(f32, nf).cpu().numpy()
    assert np.array_equal(fixed.astype(bool), R.boundary_vertices(faces, nf + 2)[:nf]) and fixed.all()
    for fix in (True, False):
        kw = dict(sigma_s=1.0, sigma_r=0.5, normal_iters=3, vertex_iters=3, max_move=0.125, fix_boundary=fix)
        r = R.smooth(xyz, rgb, faces, **kw)
        g = run_gpu(xyz, rgb, faces, **kw)
        assert len(r["faces"]) == nf and runs_of(g) == r["F"]
        hold(g, r, what="strip %d fix %d:" % (nf, fix))
    assert r["info"]["fixed"] == 0 and r["info"]["largest_move"] > 0


def test_fan_with_runs_longer_than_a_wave():
    xyz, rgb, faces = SI.fan(200)
    for fix in (True, False):
        kw = dict(sigma_s=1.0, sigma_r=0.5, normal_iters=3, vertex_iters=3, max_move=0.05, fix_boundary=fix)
        r = R.smooth(xyz, rgb, faces, **kw)
        g = run_gpu(xyz, rgb, faces, **kw)
        assert max(len(f) for f in r["F"]) == 200 and all(len(n) == 200 for n in r["N"]) and runs_of(g) == r["F"]
        hold(g, r, what="fan fix %d:" % fix)
    assert r["info"]["clamped"] > 0


def test_zero_passes_return_the_input_bits():
    xyz, rgb, faces = SI.meshes()["sphere_noisy"]
    g = run_gpu(xyz, rgb, faces, normal_iters=0, vertex_iters=0, **HAND)
    assert g["out_xyz"].tobytes() == xyz.tobytes() and g["info"]["largest_move"] == 0.0 and g["info"]["clamped"] == 0
    g = run_gpu(xyz, rgb, faces, normal_iters=4, vertex_iters=0, **HAND)
    assert g["out_xyz"].tobytes() == xyz.tobytes()
    # no normal pass: the vertices move towards the planes of the input normals
    r = R.smooth(xyz, rgb, faces, normal_iters=0, vertex_iters=2, **HAND)
    g = run_gpu(xyz, rgb, faces, normal_iters=0, vertex_iters=2, **HAND)
    assert g["normals"].tobytes() == np.ascontiguousarray(r["n0"]).tobytes()
    hold(g, r, what="no normal pass:")


def test_empty_meshes():
    import torch
    x, c, f, info = smooth.smooth(torch.empty(0, 3, dtype=torch.float64).cuda(), torch.empty(0, 3, dtype=torch.uint8).cuda(),
                                  torch.empty(0, 3, dtype=torch.int64).cuda(), 1.0, max_move=1.0)
    assert tuple(x.shape) == (0, 3) and tuple(c.shape) == (0, 3) and tuple(f.shape) == (0, 3) and info["vertices"] == info["faces"] == 0
    xyz, rgb, _ = SI.hand_mesh()
    g = run_gpu(xyz, rgb, np.zeros((0, 3), np.int64), **HAND)                      # nf = 0: the welded vertices, unmoved
    w = R.weld(xyz, rgb, np.zeros((0, 3), np.int64))
    assert g["out_xyz"].tobytes() == w[0].tobytes() and np.array_equal(g["out_rgb"], w[1]) and g["out_faces"].shape == (0, 3)
    assert g["info"]["faces"] == 0 and g["info"]["largest_move"] == 0.0


def test_refusals():
    import torch
    xyz, rgb, faces = SI.hand_mesh()
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    with pytest.raises(_lib.AdaMVSHipError, match="no CPU fallback"):
        smooth.smooth(torch.from_numpy(xyz), t(rgb), t(faces), 1.0, max_move=1.0)
    with pytest.raises(_lib.AdaMVSHipError, match="no CPU fallback"):
        smooth.smooth(t(xyz), t(rgb), torch.from_numpy(faces), 1.0, max_move=1.0)
    with pytest.raises(_lib.AdaMVSHipError, match="float64"):
        smooth.smooth(t(xyz.astype(np.float32)), t(rgb), t(faces), 1.0, max_move=1.0)
    with pytest.raises(_lib.AdaMVSHipError, match="refers to vertex"):
        smooth.smooth(t(xyz), t(rgb), t(faces + 20), 1.0, max_move=1.0)
    bad = xyz.copy()
    bad[3, 1] = np.nan
    with pytest.raises(_lib.AdaMVSHipError, match="not finite"):
        smooth.smooth(t(bad), t(rgb), t(faces), 1.0, max_move=1.0)
    with pytest.raises(ValueError, match="sigma_s"):
        smooth.smooth(t(xyz), t(rgb), t(faces), 0.0, max_move=1.0)


# ---- the box and the sphere -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", ["defaults", "other"])
@pytest.mark.parametrize("name", ["box", "box_noisy", "sphere", "sphere_noisy"])
def test_box_and_sphere(name, options):
    xyz, rgb, faces = SI.meshes()[name]
    kw = SI.DEFAULTS if options == "defaults" else SI.OTHER
    r = R.smooth(xyz, rgb, faces, weld_first=False, **kw)
    g = run_gpu(xyz, rgb, faces, **kw)
    hold(g, r, what="%s, %s:" % (name, options))
    assert r["info"]["fixed"] == 0
    if options == "other" and name.endswith("noisy"):
        assert r["info"]["clamped"] > 0                                              # the clamp binds
    move = np.linalg.norm(g["p"] - g["p0"], axis=1)
    assert move.max() <= kw["max_move"] * (1 + 1e-12)
    if name == "box_noisy" and options == "defaults":
        flat = SI.box_edge_distance(SI.clean_of("box_noisy")) > 2.0
        assert SI.rms(SI.box_distance(g["out_xyz"])[flat]) <= SI.rms(SI.box_distance(xyz)[flat]) / 2.0


def test_cut_open_box_keeps_its_boundary_bits():
    xyz, rgb, faces = SI.cut_open(*SI.meshes()["box_noisy"])
    r = R.smooth(xyz, rgb, faces, weld_first=False, **SI.DEFAULTS)
    g = run_gpu(xyz, rgb, faces, **SI.DEFAULTS)
    hold(g, r, what="cut open:")
    fixed = g["fixed"].astype(bool)
    assert fixed.sum() > 50 and g["out_xyz"][fixed].tobytes() == xyz[fixed].tobytes()


# ---- determinism and precision ----------------------------------------------------------------------------------------------------
def write_mesh(path, xyz, rgb, faces, meta=None):
    with mesh.MeshPlyWriter(path) as w:
        w.write(xyz, rgb, faces.astype(np.uint32))
    if meta is not None:
        with open(path + ".json", "w") as f:
            json.dump(meta, f)


META = dict(voxel=1.0, mu=4.0, origin=[0.0, 0.0, 0.0], views=3, brick=32)


def test_two_runs_write_the_same_bytes_and_the_json_carries_over(tmp_path):
    xyz, rgb, faces = SI.meshes()["box_noisy"]
    src = str(tmp_path / "mesh.ply")
    write_mesh(src, xyz, rgb, faces, META)
    a = smooth.from_file(src, log=lambda *a: None)
    b = smooth.from_file(src, out=str(tmp_path / "again.ply"), log=lambda *a: None)
    out = str(tmp_path / "mesh_smoothed.ply")
    assert a["ply"] == out and open(out, "rb").read() == open(b["ply"], "rb").read()
    verts, f = mesh.read_mesh_ply(out)
    assert np.array_equal(f.astype(np.int64), faces)
    assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), rgb)
    got = np.stack([verts["x"], verts["y"], verts["z"]], 1)
    r = R.smooth(xyz, rgb, faces, weld_first=False, origin=META["origin"], **SI.DEFAULTS)
    assert (np.abs(got - r["xyz"]) <= 1e-9 + 2 * np.spacing(np.abs(r["xyz"]))).all()
    res = json.load(open(out + ".json"))
    for k in smooth.CARRIED:
        assert res[k] == META[k], k
    assert "brick" not in res and res["source"] == src and res["ply"] == out
    assert (res["sigma_s"], res["sigma_r"], res["normal_iters"], res["vertex_iters"], res["max_move"], res["fix_boundary"]) == (1.0, 0.35, 10, 10, 1.0, True)
    assert (res["vertices"], res["faces"], res["fixed"], res["degenerate_faces"], res["clamped"]) == (7938, 15872, 0, 0, 0)
    assert 0 < res["rms_move"] < res["largest_move"] <= 1.0 and res["device_seconds"] > 0 and "filter" in res["stage_seconds"]
    # simplify_whu.py --cell_voxels runs on the result without --cell
    s = simplify.from_file(out, cell_voxels=2, log=lambda *a: None)
    assert s["cell"] == 2.0 and 0 < s["faces"] < len(faces) / 4


def test_a_permutation_of_the_faces_changes_only_the_order_of_the_sums():
    xyz, rgb, faces = SI.meshes()["box_noisy"]
    a = run_gpu(xyz, rgb, faces, **SI.DEFAULTS)
    perm = np.random.default_rng(7).permutation(len(faces))
    b = run_gpu(xyz, rgb, faces[perm], **SI.DEFAULTS)
    assert np.array_equal(b["out_faces"], faces[perm]) and np.array_equal(b["out_rgb"], a["out_rgb"])
    bound = 1e-9 + 2 * np.spacing(np.abs(a["out_xyz"]))
    assert (np.abs(b["out_xyz"] - a["out_xyz"]) <= bound).all()


def test_the_unwelded_bricks_give_the_bytes_of_the_welded_mesh():
    raw = I.box_mesh()
    assert len(raw[0]) > 7938
    wx, wc, wf = SI.meshes()["box"]
    a = run_gpu(wx, wc, wf, **SI.DEFAULTS)
    b = run_gpu(*raw, **SI.DEFAULTS)
    for k in ("out_xyz", "out_rgb", "out_faces", "normals", "p"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_far_from_the_origin():
    """Coordinates in multiples of 2^-16 below 128 m: the shift by OFFSET is exact, so p = xyz - O has the near scene's bits and
    so has every value computed from it; only the final O + p rounds differently, by at most one spacing of the coordinate."""
    xyz, rgb, faces = SI.meshes()["sphere_noisy"]
    xyz = np.round(xyz * 65536.0) / 65536.0
    far = xyz + OFFSET
    assert ((far - OFFSET) == xyz).all()
    near = run_gpu(xyz, rgb, faces, origin=(0.0, 0.0, 0.0), **SI.DEFAULTS)
    g = run_gpu(far, rgb, faces, origin=tuple(OFFSET), **SI.DEFAULTS)
    assert g["p0"].tobytes() == near["p0"].tobytes() and g["p"].tobytes() == near["p"].tobytes()
    assert g["normals"].tobytes() == near["normals"].tobytes() and g["info"] == near["info"]
    assert (np.abs((g["out_xyz"] - OFFSET) - near["out_xyz"]) <= np.spacing(np.abs(g["out_xyz"]))).all()
