"""Mesh cleaning without a GPU: the options, the parser and its defaults, how the area threshold resolves, what <out>.json carries
over, the binding's symbols, and the rule itself: the numpy restatement (tests/clean_ref.py) on the box and the sphere of
tests/smooth_inputs.py with 16 holes punched into each (the faces around 8 random vertices and 8 random single faces), and on a
scene of floaters.

The bars:
  the box (7938 vertices, 15872 faces) and the sphere (5628, 11252) are closed, Euler characteristic 2, no edge twice one way;
  punched, each has 16 loops and no pinched vertex; closing them by the rule leaves no open edge and no edge twice in one
    direction and restores Euler characteristic 2;
  holes only where the box is flat: the fans are planar, the signed volume equals the uncut box's to 1e-12 relative;
  holes anywhere: the volume changes by less than 1e-4 relative (the prototype of the rule measured 8.9e-6 on the box and
    7.3e-6 on the sphere with holes of its own choosing; tenfold margin)."""
import json

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, clean, mesh, simplify, smooth
import clean_inputs as CI
import clean_ref as R
import smooth_inputs as SI

NAMES = ("components", "area", "boundary", "successor", "double", "validate", "accumulate", "emit")


@pytest.fixture(scope="module")
def closed_again():
    """The restatement at the defaults on the punched box, the punched sphere and the box punched where it is flat, once."""
    out = {}
    for key, (name, flat) in dict(box=("box", False), sphere=("sphere", False), box_flat=("box", True)).items():
        xyz, rgb, faces, holes = CI.punched(name, flat)
        out[key] = (xyz, rgb, faces, holes, R.clean(xyz, rgb, faces))
    return out


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def test_the_box_and_the_sphere_are_closed_oriented_manifolds():
    m = SI.meshes()
    for name, nv, nf in (("box", 7938, 15872), ("sphere", 5628, 11252)):
        xyz, _, faces = m[name]
        assert (len(xyz), len(faces)) == (nv, nf)
        assert R.edge_facts(faces) == (0, 0, 2), name


@pytest.mark.parametrize("key", ["box", "sphere", "box_flat"])
def test_closing_the_punched_holes_restores_the_closed_manifold(closed_again, key):
    xyz, rgb, faces, holes, r = closed_again[key]
    once, twice, euler = R.edge_facts(faces)
    info = r["info"]
    print("clean: %s punched: %d faces left, %d boundary half-edges, %d loops of %d .. %d, %d pinched vertices"
          % (key, len(faces), once, info["loops"], min(r["lengths"].values()), max(r["lengths"].values()), info["nonsimple_vertices"]))
    assert holes == 16 and once == info["boundary_edges_in"] > 0 and twice == 0 and euler == 2 - 16
    assert (info["loops"], info["loops_closed"], info["loops_too_long"], info["nonsimple_vertices"]) == (16, 16, 0, 0)
    assert info["fill_faces"] == once and info["edges_left_open"] == 0 and info["components_kept"] == info["components"] == 1
    assert R.edge_facts(r["faces"]) == (0, 0, 2)
    # nothing moved: every input vertex still in use is in the output with its colour
    order = np.lexsort(r["xyz"].T[::-1])
    assert (np.diff(order) == 1).all()                                         # the output is in welded order
    pos = {tuple(v): i for i, v in enumerate(r["xyz"])}
    used = np.unique(faces)
    assert all(tuple(xyz[v]) in pos for v in used) and all((r["rgb"][pos[tuple(xyz[v])]] == rgb[v]).all() for v in used[::97])


@pytest.mark.parametrize("key,bar", [("box_flat", 1e-12), ("box", 1e-4), ("sphere", 1e-4)])
def test_the_enclosed_volume_stays(closed_again, key, bar):
    _, _, _, _, r = closed_again[key]
    full = SI.meshes()["sphere" if key == "sphere" else "box"]
    v0, v1 = R.signed_volume(full[0], full[2]), R.signed_volume(r["xyz"], r["faces"])
    print("clean: %s volume %.6f -> %.6f, relative change %.3g" % (key, v0, v1, abs(v1 - v0) / abs(v0)))
    assert abs(v1 - v0) <= bar * abs(v0), (v0, v1)


def test_floaters_go_by_their_size_and_the_sphere_only_by_its_area():
    xyz, rgb, faces, nbox = CI.floaters()
    box_triangles = xyz[faces[:nbox]]
    nsphere = len(SI.meshes()["sphere"][2])
    assert nsphere < 12000 < nbox
    r = R.clean(xyz, rgb, faces, min_faces=12000, max_hole_edges=0)
    assert r["xyz"][r["faces"]].tobytes() == box_triangles.tobytes()          # exactly the box's faces, in input order
    assert (r["info"]["components"], r["info"]["components_kept"], r["info"]["faces_removed"]) == (5, 1, nsphere + 12)
    assert r["info"]["largest_removed_faces"] == nsphere and r["info"]["fill_faces"] == 0
    r = R.clean(xyz, rgb, faces, min_faces=100, max_hole_edges=0)             # the tetrahedra go, the sphere stays
    assert (r["info"]["components_kept"], r["info"]["faces_removed"], len(r["faces"])) == (2, 12, nbox + nsphere)
    areas = np.sort(r["component_area"])
    assert areas[2] < 1.0 and 70.0 < areas[3] < 90.0 and areas[4] > 2000.0   # far from the threshold on either side
    r = R.clean(xyz, rgb, faces, min_faces=100, min_area=CI.BOX_AREA_THRESHOLD, max_hole_edges=0)
    assert r["xyz"][r["faces"]].tobytes() == box_triangles.tobytes()
    assert (r["info"]["components_kept"], r["info"]["faces_removed"]) == (1, nsphere + 12)
    assert abs(r["info"]["area_removed"] - areas[:4].sum()) <= 1e-9
    r = R.clean(xyz, rgb, faces, min_faces=0, max_hole_edges=0)               # nothing goes
    assert r["info"]["components_kept"] == 5 and len(r["faces"]) == len(faces)


def test_the_hand_made_mesh_and_the_grid_hold_what_they_are_meant_to_hold():
    xyz, rgb, faces = CI.hand_mesh()
    assert (xyz * 8 == np.round(xyz * 8)).all()
    r = R.clean(xyz, rgb, faces, min_faces=2, max_hole_edges=4)
    i = r["info"]
    assert (i["vertices_in"], i["faces_degenerate"], i["components"], i["components_kept"], i["faces_removed"]) == (len(xyz) - 1, 1, 3, 2, 1)
    assert sorted(r["lengths"].values()) == [3, 4, 24] and (i["loops_closed"], i["loops_too_long"]) == (2, 1)
    # not simple: the pinch (two in, two out), the fin's foot on the hole's rim (two in) and its other foot (one out, none in)
    assert i["nonsimple_vertices"] == 3 and i["edges_left_open"] == i["boundary_edges_in"] - 7
    assert len(r["xyz"]) == len(xyz) - 1 - 3 - 1 + 2                           # the copy, the lone triangle and the unused vertex go
    tail, head = R.half_edges(r["surviving"])
    key, cnt = np.unique(np.stack([np.minimum(tail, head), np.maximum(tail, head)], 1), axis=0, return_counts=True)
    assert (cnt == 3).sum() == 1
    r = R.clean(xyz, rgb, faces, min_faces=0, max_hole_edges=32)
    assert sorted(r["lengths"].values()) == [3, 3, 4, 24] and r["info"]["loops_closed"] == 4 and r["info"]["components_kept"] == 3
    gx, gc, gf = CI.grid_holes()
    g = R.clean(gx, gc, gf, min_faces=0, max_hole_edges=32)
    assert sorted(g["lengths"].values()) == sorted(CI.RIMS + (CI.OUTER_RIM,)) and g["info"]["nonsimple_vertices"] == 0
    assert (g["info"]["loops_closed"], g["info"]["loops_too_long"], g["info"]["fill_faces"]) == (4, 5, 3 + 4 + 31 + 32)


def test_cleaning_a_cleaned_mesh_changes_nothing(closed_again):
    xyz, rgb, faces, _, r = closed_again["sphere"]
    again = R.clean(r["xyz"], r["rgb"], r["faces"])
    for k in ("xyz", "rgb", "faces"):
        assert again[k].tobytes() == r[k].tobytes(), k
    hx, hc, hf = CI.hand_mesh()
    r = R.clean(hx, hc, hf, min_faces=2, max_hole_edges=4)
    again = R.clean(r["xyz"], r["rgb"], r["faces"], min_faces=2, max_hole_edges=4)
    for k in ("xyz", "rgb", "faces"):
        assert again[k].tobytes() == r[k].tobytes(), k
    # nothing to drop, nothing to close: the welded input minus its degenerate faces and unused vertices
    r = R.clean(hx, hc, hf, min_faces=0, max_hole_edges=0)
    wx, wc, wf = r["welded"]
    used = np.unique(wf)
    assert r["xyz"].tobytes() == wx[used].tobytes() and r["rgb"].tobytes() == wc[used].tobytes()
    assert np.array_equal(used[r["faces"]], wf) and len(wf) == len(hf) - 1


# ---- the options, the parser, the JSON, the binding --------------------------------------------------------------------------
def test_check_options():
    clean.check_options()
    clean.check_options(0, None, 0)
    clean.check_options(5, 0.25, 4096)
    for bad in (-1, 2.5, float("nan"), None, True, "3"):
        with pytest.raises(ValueError, match="min_faces"):
            clean.check_options(min_faces=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="min_area"):
            clean.check_options(min_area=bad)
    for bad in (-1, 4097, 2.5, None, True):
        with pytest.raises(ValueError, match="max_hole_edges"):
            clean.check_options(max_hole_edges=bad)


def test_parser_and_defaults():
    ap = clean.build_parser()
    a = ap.parse_args(["--output_folder", "o"])
    assert (a.mesh, a.min_faces, a.min_area, a.min_area_voxels, a.max_hole_edges, a.origin, a.out) == (None, 100, None, None, 32, None, None)
    assert clean.mesh_path_of(a) == "o/mesh.ply" and clean.default_out("o/mesh.ply") == "o/mesh_cleaned.ply"
    assert clean.default_out("a/b.PLY") == "a/b_cleaned.ply" and clean.default_out("a/b") == "a/b_cleaned.ply"
    a = ap.parse_args(["--mesh", "m.ply", "--min_faces", "0", "--min_area_voxels", "50", "--max_hole_edges", "8", "--origin", "1", "2", "3",
                       "--out", "x.ply"])
    assert (clean.mesh_path_of(a), a.min_faces, a.min_area, a.min_area_voxels, a.max_hole_edges, a.origin, a.out) == \
        ("m.ply", 0, None, 50.0, 8, [1.0, 2.0, 3.0], "x.ply")
    with pytest.raises(ValueError, match="--mesh or --output_folder"):
        clean.mesh_path_of(ap.parse_args([]))


def test_the_area_threshold_resolves():
    meta = {"voxel": 0.25}
    assert clean.resolve_min_area(None, None, meta) is None and clean.resolve_min_area(None, None, None) is None       # off by default
    assert clean.resolve_min_area(None, 8, meta) == 0.5 and clean.resolve_min_area(0.3, None, None) == 0.3
    with pytest.raises(ValueError, match="not both"):
        clean.resolve_min_area(0.3, 2, meta)
    with pytest.raises(ValueError, match="--min_area"):
        clean.resolve_min_area(None, 2, None)                                   # K voxels without the JSON
    with pytest.raises(ValueError, match="--min_area"):
        clean.resolve_min_area(None, 2, {"mu": 1.0})
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_area"):
            clean.resolve_min_area(bad, None, meta)
        with pytest.raises(ValueError, match="min_area_voxels"):
            clean.resolve_min_area(None, bad, meta)


def test_summary_carries_the_mesh_json_over():
    meta = dict(voxel=0.25, mu=1.0, origin=[1.0, 2.0, 3.0], views=5, brick=128, vertices=10, faces=20, seconds=3.0)
    info = dict.fromkeys(clean.COUNTS, 3)
    info.update(area_removed=0.5, vertices=9, faces=17)
    options = dict(min_faces=100, min_area=None, max_hole_edges=32)
    res = clean.summary(meta, info, options, np.array([1.0, 2.0, 3.0]), "m.ply", "c.ply", 2.0, 0.5, {"loops": 0.1})
    assert clean.CARRIED is simplify.CARRIED and list(res)[:4] == list(clean.CARRIED)
    assert [res[k] for k in clean.CARRIED] == [0.25, 1.0, [1.0, 2.0, 3.0], 5] and "brick" not in res
    assert (res["clean_origin"], res["source"], res["ply"]) == ([1.0, 2.0, 3.0], "m.ply", "c.ply")
    assert all(res[k] == v for k, v in info.items()) and all(res[k] == v for k, v in options.items())
    assert (res["vertices"], res["faces"]) == (9, 17)                           # the cleaned mesh's, not <mesh>.json's
    assert (res["seconds"], res["device_seconds"], res["stage_seconds"]) == (2.0, 0.5, {"loops": 0.1})
    json.dumps(res)
    assert "voxel" not in clean.summary(None, info, options, np.zeros(3), "m.ply", "c.ply", 0.0, 0.0)
    # the next steps' defaults keep working on the cleaned mesh
    assert simplify.resolve_cell(None, 2, res) == 0.5 and smooth.resolve_sigma_s(None, None, res) == 0.25


def test_binding_constants_and_symbols():
    assert _lib.ABI_VERSION == 22 and _lib.CLEAN_TILE == 256 and _lib.CLEAN_CHUNK == R.CHUNK == 1024
    assert _lib.CLEAN_MAX_HOLE_EDGES == clean.MAX_HOLE_EDGES == 4096 and _lib.CLEAN_MAX_ROUNDS == clean.MAX_ROUNDS == 64
    assert sorted(k for k in _lib.SIGNATURES if k.startswith("adamvs_clean_")) == sorted("adamvs_clean_" + n for n in NAMES)
    for name in NAMES:
        assert hasattr(_lib.load(), "adamvs_clean_" + name)


def test_doubling_rounds_cover_every_cycle():
    assert [clean.doubling_rounds(n) for n in (0, 1, 2, 3, 32, 33, 64, 65)] == [0, 1, 2, 3, 6, 7, 7, 8]
    for n in (2, 3, 31, 32, 33, 160, 4096, 4097):
        assert 2 ** clean.doubling_rounds(n) >= 2 * n


def test_refusals(tmp_path):
    import torch
    xyz, rgb, faces = CI.hand_mesh()
    src = str(tmp_path / "m.ply")
    with mesh.MeshPlyWriter(src) as w:
        w.write(xyz, rgb, faces.astype(np.uint32))
    with pytest.raises(ValueError, match="<mesh>.json"):
        clean.from_file(src, min_area_voxels=4)                                 # K voxels and no JSON
    with pytest.raises(ValueError, match="not both"):
        clean.from_file(src, min_area=1.0, min_area_voxels=2)
    with pytest.raises(SystemExit, match="not both"):
        clean.main(["--mesh", src, "--min_area", "1", "--min_area_voxels", "2"])
    with pytest.raises(ValueError, match="max_hole_edges"):
        clean.from_file(src, max_hole_edges=4097)
    with pytest.raises(ValueError, match="min_faces"):
        clean.from_file(src, min_faces=-1)
    with pytest.raises(ValueError, match="min_area"):
        clean.from_file(src, min_area=0.0)
    assert not (tmp_path / "m_cleaned.ply").exists() and not (tmp_path / "m_cleaned.ply.json").exists()
    # there is no CPU path
    with pytest.raises(_lib.AdaMVSHipError, match="no CPU fallback"):
        clean.clean(torch.from_numpy(xyz), torch.from_numpy(rgb), torch.from_numpy(faces))
