"""Mesh simplification without a GPU: the restatement's own properties on the sphere and the box (tests/simplify_ref.py: the
numbers the numpy prototype of the rule gave), the solve of csrc/mesh_simplify.hip run on the host against np.linalg.eigh, the
parser and its defaults, the default lattice origin, what <out>.json carries over, and the refusals."""
import json

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, hip_ops, mesh, simplify
import simplify_inputs as I
import simplify_ref as S
from mesh_ref import closed_and_oriented


@pytest.fixture(scope="module")
def sphere():
    return I.sphere_mesh()


@pytest.fixture(scope="module")
def box():
    return I.box_mesh()


def in_cells(r, cell):
    return bool((np.abs(r["pos"] - r["centre"]) <= cell / 2 + 2 * np.spacing(np.abs(r["pos"]))).all())


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", I.CELLS)
def test_restatement_on_the_sphere(sphere, cell):
    xyz, rgb, faces = sphere
    r = S.simplify(xyz, rgb, faces, cell, I.LATTICE_ORIGIN)
    i, e = r["info"], I.SPHERE_EXPECT[cell]
    assert (i["vertices_in"], i["faces_in"]) == (5628, 11252)
    assert (i["cells"], i["faces_out"], i["faces_duplicate"], i["fallbacks"]) == (e["cells"], e["faces_out"], e["faces_duplicate"], e["fallbacks"])
    assert i["faces_in"] == i["faces_collapsed"] + i["faces_duplicate"] + i["faces_out"] and sum(i["rank_hist"]) == i["cells"]
    assert not (r["rank_tie"] | r["box_tie"]).any()
    assert in_cells(r, cell) and np.array_equal(S.cell_keys(r["pos"], cell, I.LATTICE_ORIGIN)[0], r["keys"])
    dist = np.abs(np.linalg.norm(r["xyz"] - np.asarray(I.SPHERE_CENTRE), axis=1) - I.SPHERE_RADIUS)
    assert dist.max() <= e["dist"], dist.max()                       # 0.056 / 0.123 / 0.218
    assert r["faces"].max() == len(r["xyz"]) - 1 == i["cells_used"] - 1


@pytest.mark.parametrize("cell", I.CELLS)
def test_restatement_on_the_box(box, cell):
    xyz, rgb, faces = box
    r = S.simplify(xyz, rgb, faces, cell, I.LATTICE_ORIGIN)
    i, e = r["info"], I.BOX_EXPECT[cell]
    assert (i["vertices_in"], i["faces_in"]) == (7938, 15872)
    assert i["faces_out"] == e["faces_out"] and tuple(i["rank_hist"]) == (0,) + e["rank_hist"]       # planar / edge / corner cells
    assert not (r["rank_tie"] | r["box_tie"]).any() and in_cells(r, cell)
    closed, chi = closed_and_oriented(r["faces"])
    assert closed and chi == 2


def test_restatement_under_an_offset_and_without_the_weld(box):
    """The faces, the colours and the counts do not feel a shift of the mesh and the lattice by whole metres (the shift is exact
    in fp64 for these coordinates); welded or not, the input gives the same result."""
    xyz, rgb, faces = box
    off = np.array([5e5, 3.4e6, 0.0])
    a = S.simplify(xyz, rgb, faces, 3.0, I.LATTICE_ORIGIN)
    b = S.simplify(xyz + off, rgb, faces, 3.0, np.asarray(I.LATTICE_ORIGIN) + off)
    assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(a["rgb"], b["rgb"]) and a["info"] == b["info"]
    assert np.abs(b["xyz"] - off - a["xyz"]).max() <= 1e-3
    w = S.weld(xyz, rgb, faces)
    c = S.simplify(*w, 3.0, I.LATTICE_ORIGIN, weld_first=False)
    assert c["xyz"].tobytes() == a["xyz"].tobytes() and np.array_equal(c["faces"], a["faces"])


def test_restatement_on_the_hand_made_mesh_and_its_refusals():
    xyz, rgb, faces, cell, origin = I.hand_mesh()
    r = S.simplify(xyz, rgb, faces, cell, origin)
    assert r["info"] == dict(cells=13, cells_used=12, vertices_in=26, faces_in=12, faces_collapsed=3, faces_duplicate=1, faces_out=8,
                             rank_hist=[0, 8, 4, 1], fallbacks=1)
    for bad in (np.nan, np.inf, float(1 << 21) + 0.5, -0.25):
        x = xyz.copy()
        x[7, 1] = bad
        with pytest.raises(S.SimplifyError):
            S.simplify(x, rgb, faces, cell, origin)
    e = S.simplify(np.zeros((0, 3)), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int64), 1.0, (0.0, 0.0, 0.0))
    assert e["xyz"].shape == (0, 3) and e["faces"].shape == (0, 3) and e["info"]["cells"] == 0


# ---- the kernel's solve, run on the host ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", I.CELLS)
def test_jacobi_solve_on_the_host_matches_eigh(sphere, box, cell):
    """adamvs_simplify_solve_host runs the inline function k_simplify_solve runs: ranks and fallbacks as np.linalg.eigh decides
    them, positions within the GPU tests' bound (the quadrics are the restatement's here, so only the solve differs)."""
    for xyz, rgb, faces in (sphere, box):
        r = S.simplify(xyz, rgb, faces, cell, I.LATTICE_ORIGIN)
        q = np.concatenate([r["A"][:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]], r["b"], r["dd"][:, None]], 1)
        p, rank, fb, err = hip_ops.simplify_solve_host(q, r["mean"], cell)
        assert np.array_equal(rank, r["rank"]) and np.array_equal(fb.astype(bool), r["fallback"])
        bound = 1e-9 * cell + 2 * np.spacing(np.abs(r["pos"]))
        assert (np.abs(r["centre"] + p - r["pos"]) <= bound).all()
        assert (np.abs(p) <= cell / 2).all()
        assert np.abs(err - r["error"]).max() <= 1e-9 * r["dd"].max()
    with pytest.raises(_lib.AdaMVSHipError, match="rank_eps"):
        hip_ops.simplify_solve_host(np.zeros((1, 10)), np.zeros((1, 3)), 1.0, rank_eps=1.0)
    # nothing to keep: the zero quadric falls back to the mean
    p, rank, fb, _ = hip_ops.simplify_solve_host(np.zeros((1, 10)), np.array([[0.25, -0.125, 0.0]]), 1.0)
    assert rank[0] == 0 and fb[0] == 1 and p.tolist() == [[0.25, -0.125, 0.0]]


def test_binding_constants_and_symbols():
    assert (_lib.SIMPLIFY_TILE, _lib.SIMPLIFY_KEY_BITS) == (256, 21) and S.KEY_BITS == 21
    for name in ("keys", "corners", "accumulate", "solve", "solve_host", "triples", "first", "mark", "count", "emit"):
        assert "adamvs_simplify_" + name in _lib.SIGNATURES
        assert hasattr(_lib.load(), "adamvs_simplify_" + name)


# ---- the parser, the defaults, the JSON, the refusals ----------------------------------------------------------------------------
def test_parser_and_defaults():
    ap = simplify.build_parser()
    a = ap.parse_args(["--output_folder", "o"])
    assert (a.mesh, a.cell, a.cell_voxels, a.origin, a.rank_eps, a.out) == (None, None, None, None, 1e-3, None)
    assert simplify.mesh_path_of(a) == "o/mesh.ply" and simplify.default_out("o/mesh.ply") == "o/mesh_simplified.ply"
    assert simplify.default_out("a/b.PLY") == "a/b_simplified.ply" and simplify.default_out("a/b") == "a/b_simplified.ply"
    a = ap.parse_args(["--mesh", "m.ply", "--cell", "0.75", "--origin", "1", "2", "3", "--rank_eps", "0.01", "--out", "x.ply"])
    assert (simplify.mesh_path_of(a), a.cell, a.origin, a.rank_eps, a.out) == ("m.ply", 0.75, [1.0, 2.0, 3.0], 0.01, "x.ply")
    assert simplify.resolve_cell(None, None, {"voxel": 0.25}) == 1.0             # four voxels by default
    assert simplify.resolve_cell(None, 2, {"voxel": 0.25}) == 0.5 and simplify.resolve_cell(0.3, None, None) == 0.3
    with pytest.raises(ValueError, match="--mesh or --output_folder"):
        simplify.mesh_path_of(ap.parse_args([]))


def test_default_lattice_origin():
    o = simplify.default_lattice_origin(3.0, [10.0, 20.0, 30.0], [11.0, 21.0, 30.0])
    assert o.tolist() == [9.0, 19.0, 29.0]                                        # the volume origin of <mesh>.json - c / 3
    o = simplify.default_lattice_origin(3.0, None, [11.0, 21.0, 30.0])
    assert o.tolist() == [10.0, 20.0, 29.0]                                       # else the vertex minimum - c / 3
    # a plane a whole number of cells above the volume origin does not sit on a cell boundary
    assert (((30.0 + 3.0 * np.arange(4)) - 29.0) / 3.0 % 1.0 != 0).all()
    o = simplify.default_lattice_origin(0.75, [0.0, 0.0, 0.0], [5.0, 5.0, -1.0])
    assert o.tolist() == [-0.25, -0.25, -1.0] and (o <= [5.0, 5.0, -1.0]).all()   # never above a vertex: lowered by whole cells


def test_summary_carries_the_mesh_json_over():
    meta = dict(voxel=0.25, mu=1.0, origin=[1.0, 2.0, 3.0], views=5, brick=128, vertices=10, faces=20, seconds=3.0)
    info = dict(cells=7, cells_used=5, vertices_in=10, faces_in=20, faces_collapsed=12, faces_duplicate=1, faces_out=7, rank_hist=[0, 4, 2, 1],
                fallbacks=1)
    res = simplify.summary(meta, info, 1.0, np.array([0.5, 1.5, 2.5]), "m.ply", "s.ply", 2.0, 0.5)
    assert [res[k] for k in simplify.CARRIED] == [0.25, 1.0, [1.0, 2.0, 3.0], 5] and "brick" not in res
    assert (res["cell"], res["lattice_origin"], res["source"], res["ply"]) == (1.0, [0.5, 1.5, 2.5], "m.ply", "s.ply")
    assert (res["vertices"], res["faces"], res["seconds"], res["device_seconds"]) == (5, 7, 2.0, 0.5)
    assert all(res[k] == v for k, v in info.items())
    json.dumps(res)
    assert "voxel" not in simplify.summary(None, info, 1.0, np.zeros(3), "m.ply", "s.ply", 0.0, 0.0)


def test_refusals(tmp_path):
    import torch
    xyz, rgb, faces, _, _ = I.hand_mesh()
    src = str(tmp_path / "m.ply")
    with mesh.MeshPlyWriter(src) as w:
        w.write(xyz, rgb, faces.astype(np.uint32))
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell"):
            simplify.from_file(src, cell=cell)
    with pytest.raises(ValueError, match="<mesh>.json"):
        simplify.from_file(src)                                                   # no JSON and no --cell
    with pytest.raises(ValueError, match="<mesh>.json"):
        simplify.from_file(src, cell_voxels=2)
    with pytest.raises(ValueError, match="not both"):
        simplify.from_file(src, cell=1.0, cell_voxels=2)
    with pytest.raises(SystemExit, match="not both"):
        simplify.main(["--mesh", src, "--cell", "1", "--cell_voxels", "2"])
    with pytest.raises(ValueError, match="rank_eps"):
        simplify.from_file(src, cell=1.0, rank_eps=1.5)
    with open(src + ".json", "w") as f:
        json.dump(dict(voxel=0.25), f)
    with pytest.raises(ValueError, match="cell_voxels"):
        simplify.from_file(src, cell_voxels=0)
    assert not (tmp_path / "m_simplified.ply").exists()
    # there is no CPU path
    with pytest.raises(_lib.AdaMVSHipError, match="no CPU fallback"):
        simplify.simplify(torch.from_numpy(xyz), torch.from_numpy(rgb), torch.from_numpy(faces), 1.0, (0.0, 0.0, 0.0))
