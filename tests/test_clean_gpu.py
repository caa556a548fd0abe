"""Mesh cleaning on the GPU (csrc/mesh_clean.hip through ada_mvs_amd/clean.py) against the restatement (tests/clean_ref.py), never
against itself.  Everything that is an integer (labels, masks, successors, loop labels, faces, counts) must be equal; the fill
vertices and their colours must be bit-equal (a fixed order of additions and one division); the areas of the components agree
to 1e-12 relative (the pieces are summed in the same order on both sides; the face areas are smooth's, which its own tests
hold), and no threshold used here lies within 1e-6 relative of an area."""
import json

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, clean, hip_ops, mesh, simplify, smooth
import clean_inputs as CI
import clean_ref as R
import simplify_inputs as I
import smooth_inputs as SI

pytestmark = pytest.mark.gpu

OFFSET = np.array([5e6, 3.4e6, 0.0])          # dyadic: exact to add to coordinates that are multiples of 2^-16 below 2^7
EXACT_INFO = [k for k in clean.COUNTS if k not in ("area_removed", "component_rounds")]


def dev(xyz, rgb, faces):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(xyz, np.float64)).cuda(), torch.from_numpy(np.ascontiguousarray(rgb, np.uint8)).cuda(),
            torch.from_numpy(np.ascontiguousarray(faces).astype(np.int64)).cuda())


def run_gpu(xyz, rgb, faces, **kw):
    """clean() on numpy inputs -> dict of numpy arrays: the result, the intermediates and info."""
    detail = {}
    x, c, f, info = clean.clean(*dev(xyz, rgb, faces), detail=detail, **kw)
    out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in detail.items()}
    out.update(out_xyz=x.cpu().numpy(), out_rgb=c.cpu().numpy(), out_faces=f.cpu().numpy().astype(np.int64), info=info)
    return out


def hold(g, r, what=""):
    """The GPU run g against the restatement r as the module docstring says."""
    gi, ri = g["info"], r["info"]
    for k in EXACT_INFO:
        assert gi[k] == ri[k], (what, k, gi[k], ri[k])
    assert abs(gi["area_removed"] - ri["area_removed"]) <= 1e-12 * abs(ri["area_removed"])
    assert g["out_xyz"].tobytes() == np.ascontiguousarray(r["xyz"]).tobytes(), what
    assert np.array_equal(g["out_rgb"], r["rgb"]) and np.array_equal(g["out_faces"], r["faces"]), what
    if "labels" in r:
        assert g["xyz"].tobytes() == r["welded"][0].tobytes() and np.array_equal(g["faces"], r["welded"][2])
        assert np.array_equal(g["degenerate"], r["degenerate"])
        assert np.array_equal(g["labels"], r["labels"]) and np.array_equal(g["face_labels"], r["face_labels"])
        assert np.array_equal(g["kept"], r["kept"]) and np.array_equal(g["component_faces"], r["component_faces"])
        assert (np.abs(g["component_area"] - r["component_area"]) <= 1e-12 * r["component_area"]).all()
        assert np.array_equal(g["surviving"], r["surviving"])
    if "loop" in r:
        assert np.array_equal(g["boundary"].astype(bool), r["boundary"]) and np.array_equal(g["successor"], r["successor"])
        assert np.array_equal(g["loop"], r["loop"]) and np.array_equal(g["closed"].astype(bool), r["closed"])
        if len(r["centres"]):
            assert g["centre"].tobytes() == r["centres"].tobytes() and np.array_equal(g["colour"], r["colours"])
    print("clean: %s %d -> %d vertices, %d -> %d faces, %d / %d components kept in %d rounds, %d / %d loops closed, %d fill faces"
          % (what, gi["vertices_in"], gi["vertices"], gi["faces_in"], gi["faces"], gi["components_kept"], gi["components"],
             gi["component_rounds"], gi["loops_closed"], gi["loops"], gi["fill_faces"]))


def both(xyz, rgb, faces, what="", **kw):
    g, r = run_gpu(xyz, rgb, faces, **kw), R.clean(xyz, rgb, faces, **kw)
    hold(g, r, what)
    return g, r


# ---- the hand-made mesh ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_faces,M", [(2, 4), (0, 32), (0, 0), (9, 3)])
def test_hand_made_mesh_every_intermediate(min_faces, M):
    xyz, rgb, faces = CI.hand_mesh()
    g, r = both(xyz, rgb, faces, "hand-made %d %d:" % (min_faces, M), min_faces=min_faces, max_hole_edges=M)
    assert g["info"]["faces_degenerate"] == 1 and g["info"]["nonsimple_vertices"] == 3
    if (min_faces, M) == (2, 4):
        assert (g["info"]["components"], g["info"]["components_kept"], g["info"]["loops"], g["info"]["loops_closed"]) == (3, 2, 3, 2)
    if M == 0:
        assert g["info"]["fill_faces"] == 0 and g["info"]["edges_left_open"] == g["info"]["boundary_edges_in"]


# ---- components -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", list(SI.EDGE_TILE_FACES) + [255, 256, 257])
def test_strips_across_a_workgroup_boundary(nf):
    import torch
    # the open edges alone, with vertex numbers that have bit 31 set: the restatement on the strip before the renaming (the same
    # half-edges), and smoothing's marks are the ends of cleaning's open half-edges
    big, bits = SI.renamed_strip_faces(nf)
    f32 = torch.from_numpy(bits).cuda()
    bnd = hip_ops.clean_boundary(f32).cpu().numpy().astype(bool)
    assert np.array_equal(bnd, R.boundary(SI.strip(nf)[2], nf + 2)[0]) and bnd.sum() == nf + 2
    ends = np.concatenate([a[bnd] for a in R.half_edges(big)])
    marks = np.zeros(nf, bool)
    marks[ends[ends < nf]] = True
    assert np.array_equal(hip_ops.smooth_boundary(f32, nf).cpu().numpy().astype(bool), marks)
    g, _ = both(*SI.strip(nf), "strip %d:" % nf, min_faces=nf, max_hole_edges=0)
    assert g["info"]["components"] == g["info"]["components_kept"] == 1 and len(g["out_faces"]) == nf
    g, _ = both(*SI.strip(nf), "strip %d, dropped:" % nf, min_faces=nf + 1, max_hole_edges=0)
    assert g["info"]["components_kept"] == 0 and g["out_xyz"].shape == (0, 3) and g["info"]["faces_removed"] == nf


@pytest.mark.parametrize("which", ["renumbered", "scrambled"])
def test_the_smallest_label_travels_a_strip_of_5000_faces(which):
    """The weld numbers the vertices by position, so renumbering alone changes nothing after it; the scrambled strip puts the
    vertices at permuted places, and the welded numbers are then random along the strip."""
    xyz, rgb, faces = CI.renumbered_strip(5000) if which == "renumbered" else CI.scrambled_strip(5000)
    g, r = both(xyz, rgb, faces, "strip of 5000, %s:" % which, min_faces=5000, max_hole_edges=0)
    print("clean: %s strip of 5000 faces: component_rounds = %d" % (which, g["info"]["component_rounds"]))
    assert g["info"]["components"] == 1 and (g["labels"] == 0).all() and g["info"]["component_rounds"] <= clean.MAX_ROUNDS


def test_fan_with_a_run_longer_than_a_wave():
    g, _ = both(*SI.fan(200), "fan:", min_faces=200, max_hole_edges=0)
    assert g["info"]["components"] == 1 and len(g["out_faces"]) == 200


def test_many_roots_at_once():
    xyz, rgb, faces = CI.disjoint_triangles(300)
    g, _ = both(xyz, rgb, faces, "300 triangles:", min_faces=1, max_hole_edges=0)
    assert g["info"]["components"] == g["info"]["components_kept"] == 300 and g["info"]["loops"] == 300
    g, _ = both(xyz, rgb, faces, "300 triangles, closed:", min_faces=1, max_hole_edges=3)
    assert g["info"]["loops_closed"] == 300 and g["info"]["fill_faces"] == 900
    g, _ = both(xyz, rgb, faces, "300 triangles, dropped:", min_faces=2, max_hole_edges=3)
    assert g["info"]["components_kept"] == 0 and g["info"]["faces_removed"] == 300


def test_a_component_longer_than_a_chunk_and_floaters():
    xyz, rgb, faces, nbox = CI.floaters()
    g, r = both(xyz, rgb, faces, "floaters by faces:", min_faces=12000, max_hole_edges=0)
    assert g["out_xyz"][g["out_faces"]].tobytes() == xyz[faces[:nbox]].tobytes()
    assert (r["component_faces"] > 10 * R.CHUNK).sum() == 2                     # both are sums of many pieces
    g, _ = both(xyz, rgb, faces, "floaters by area:", min_faces=100, min_area=CI.BOX_AREA_THRESHOLD, max_hole_edges=0)
    assert g["out_xyz"][g["out_faces"]].tobytes() == xyz[faces[:nbox]].tobytes() and g["info"]["components_kept"] == 1
    assert (np.abs(g["component_area"] / CI.BOX_AREA_THRESHOLD - 1) > 1e-6).all()
    g, _ = both(xyz, rgb, faces, "floaters, tetrahedra only:", min_faces=100, max_hole_edges=0)
    assert g["info"]["components_kept"] == 2 and g["info"]["faces_removed"] == 12


# ---- loop lengths ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    return CI.grid_holes()


def lengths_closed(g):
    """The lengths of the loops the run g closed, from its closed mask and loop labels."""
    return sorted(np.unique(g["loop"][g["closed"].astype(bool)], return_counts=True)[1].tolist())


def test_rims_up_to_the_bound_are_closed_and_longer_ones_left_wholly_open(grid):
    g, r = both(*grid, "grid, M = 32:", min_faces=0, max_hole_edges=32)
    assert lengths_closed(g) == [3, 4, 31, 32] and g["info"]["loops_too_long"] == 5 and g["info"]["loops"] == 9
    assert g["info"]["fill_faces"] == 70 and g["info"]["edges_left_open"] == 33 + 64 + 65 + 200 + 160
    # not one fill face on a longer rim: every fill face's rim edge belongs to a closed loop
    ns = len(g["surviving"])
    assert len(g["out_faces"]) == ns + 70 and R.edge_facts(g["out_faces"])[0] == g["info"]["edges_left_open"]


def test_a_large_bound_closes_the_outer_rim_and_zero_closes_nothing(grid):
    g, _ = both(*grid, "grid, M = 4096:", min_faces=0, max_hole_edges=4096)
    assert lengths_closed(g) == sorted(CI.RIMS + (CI.OUTER_RIM,)) and g["info"]["edges_left_open"] == 0
    assert R.edge_facts(g["out_faces"])[:2] == (0, 0)
    g, _ = both(*grid, "grid, M = 0:", min_faces=0, max_hole_edges=0)
    assert g["info"]["fill_faces"] == 0 and g["info"]["loops"] == 9 and g["info"]["loops_too_long"] == 9
    for M in (2, 3, 33, 64, 199, 200):
        both(*grid, "grid, M = %d:" % M, min_faces=0, max_hole_edges=M)


def test_the_doubling_trap_too_few_rounds_still_close_no_part_of_a_longer_rim(grid):
    """ceil(log2(32)) + 1 = 6 rounds label every loop of up to 32 edges whole; on the rims of 33, 64 and 65 the labels are then
    minima over 64 half-edges and on the longer ones window minima.  The validation must still find exactly the four short loops."""
    import torch
    _, r = both(*grid, "grid:", min_faces=0, max_hole_edges=32)
    sf = torch.from_numpy(r["surviving"].astype(np.int32)).cuda()
    bnd = hip_ops.clean_boundary(sf)
    st = hip_ops.clean_successor(sf, len(r["welded"][0]), bnd)
    state, other = (st["lab"], st["nxt"], st["broken"]), (st["lab"].clone(), st["nxt"].clone(), st["broken"].clone())
    for _ in range(6):
        other = hip_ops.clean_double(bnd, state, other)
        state, other = other, state
    _, _, loop, closed = hip_ops.clean_validate(bnd, st["succ"], state[0], state[2], 32)
    assert np.array_equal(closed.cpu().numpy().astype(bool), r["closed"])
    loop = loop.cpu().numpy()
    short = np.isin(r["loop"], [l for l, n in r["lengths"].items() if n <= 64])
    assert np.array_equal(loop[short], r["loop"][short])                        # whole where the window covers the cycle
    assert ((loop == -1) | (loop == r["loop"]))[r["boundary"]].all()


# ---- the box and the sphere -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["box", "sphere", "box_flat"])
def test_punched_box_and_sphere(key):
    name, flat = ("box", True) if key == "box_flat" else (key, False)
    xyz, rgb, faces, holes = CI.punched(name, flat)
    g, r = both(xyz, rgb, faces, "punched %s:" % key)
    assert (g["info"]["loops"], g["info"]["loops_closed"], g["info"]["nonsimple_vertices"], g["info"]["edges_left_open"]) == (16, 16, 0, 0)
    assert R.edge_facts(g["out_faces"]) == (0, 0, 2)
    full = SI.meshes()[name]
    v0, v1 = R.signed_volume(full[0], full[2]), R.signed_volume(g["out_xyz"], g["out_faces"])
    assert abs(v1 - v0) <= (1e-12 if flat else 1e-4) * abs(v0), (v0, v1)


def test_cut_open_box_gets_no_fill_and_keeps_its_bits():
    xyz, rgb, faces = SI.cut_open(*SI.meshes()["box"])
    g, r = both(xyz, rgb, faces, "cut open:")
    assert min(r["lengths"].values()) > 32 and g["info"]["loops_too_long"] == g["info"]["loops"] >= 1
    assert g["info"]["fill_faces"] == 0 and g["info"]["fill_vertices"] == 0 and np.array_equal(g["out_faces"], g["new_index"][faces])
    used = np.unique(faces)
    assert g["out_xyz"].tobytes() == xyz[used].tobytes() and np.array_equal(g["out_rgb"], rgb[used])


# ---- invariances ------------------------------------------------------------------------------------------------------------------
def test_the_unwelded_bricks_give_the_bytes_of_the_welded_mesh():
    raw = I.box_mesh()
    assert len(raw[0]) > 7938
    a = run_gpu(*SI.meshes()["box"])
    b = run_gpu(*raw)
    for k in ("out_xyz", "out_rgb", "out_faces", "labels", "loop"):
        assert a[k].tobytes() == b[k].tobytes(), k


def write_mesh(path, xyz, rgb, faces, meta=None):
    with mesh.MeshPlyWriter(path) as w:
        w.write(xyz, rgb, faces.astype(np.uint32))
    if meta is not None:
        with open(path + ".json", "w") as f:
            json.dump(meta, f)


META = dict(voxel=1.0, mu=4.0, origin=[0.0, 0.0, 0.0], views=3, brick=32)
TIMINGS = ("seconds", "device_seconds", "stage_seconds")


def test_two_runs_write_the_same_bytes_and_the_json_carries_every_key(tmp_path):
    xyz, rgb, faces, _ = CI.punched("sphere")
    src = str(tmp_path / "mesh.ply")
    write_mesh(src, xyz, rgb, faces, META)
    a = clean.from_file(src, log=lambda *a: None)
    b = clean.from_file(src, out=str(tmp_path / "mesh_cleaned.ply"), min_area_voxels=2, log=lambda *a: None)
    out = str(tmp_path / "mesh_cleaned.ply")
    first = open(out, "rb").read(), {k: v for k, v in json.load(open(out + ".json")).items() if k not in TIMINGS}
    c = clean.from_file(src, out=str(tmp_path / "again.ply"), min_area_voxels=2, log=lambda *a: None)
    assert open(c["ply"], "rb").read() == first[0]
    again = {k: v for k, v in json.load(open(c["ply"] + ".json")).items() if k not in TIMINGS + ("ply",)}
    assert again == {k: v for k, v in first[1].items() if k != "ply"}
    assert a["ply"] == out and a["min_area"] is None and b["min_area"] == 2.0
    res = json.load(open(out + ".json"))
    for k in clean.CARRIED:
        assert res[k] == META[k], k
    for k in clean.COUNTS + TIMINGS + ("min_faces", "min_area", "max_hole_edges", "source", "ply", "clean_origin"):
        assert k in res, k
    assert "brick" not in res and res["source"] == src and set(res["stage_seconds"]) == set(clean.STAGES) and res["device_seconds"] > 0
    r = R.clean(xyz, rgb, faces, origin=META["origin"])
    verts, f = mesh.read_mesh_ply(out)
    assert np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float64).tobytes() == r["xyz"].tobytes()
    assert np.array_equal(f.astype(np.int64), r["faces"]) and all(res[k] == r["info"][k] for k in EXACT_INFO)
    # the next steps run on the result with their defaults
    assert simplify.resolve_cell(None, 2, res) == 2.0 and smooth.resolve_sigma_s(None, None, res) == 1.0
    # cleaning the output again returns the same bytes
    d = clean.from_file(out, out=str(tmp_path / "twice.ply"), log=lambda *a: None)
    assert open(d["ply"], "rb").read() == open(out, "rb").read() and d["fill_faces"] == 0 and d["faces_removed"] == 0


def test_cleaning_the_output_again_returns_the_same_arrays():
    for args, kw in ((CI.hand_mesh(), dict(min_faces=2, max_hole_edges=4)), (CI.grid_holes(), dict(min_faces=0, max_hole_edges=32)),
                     (CI.punched("box")[:3], {})):
        a = run_gpu(*args, **kw)
        b = run_gpu(a["out_xyz"], a["out_rgb"], a["out_faces"], **kw)
        for k in ("out_xyz", "out_rgb", "out_faces"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert b["info"]["fill_faces"] == 0 and b["info"]["faces_removed"] == 0 and b["info"]["faces_degenerate"] == 0


def test_nothing_to_drop_and_nothing_to_close_returns_the_welded_input():
    xyz, rgb, faces = CI.hand_mesh()
    g, r = both(xyz, rgb, faces, "hand-made, nothing asked:", min_faces=0, max_hole_edges=0)
    wx, wc, wf = r["welded"]
    used = np.unique(wf)
    assert g["out_xyz"].tobytes() == wx[used].tobytes() and np.array_equal(g["out_rgb"], wc[used]) and np.array_equal(used[g["out_faces"]], wf)


def test_a_permutation_of_the_faces_keeps_the_faces_and_the_loops():
    xyz, rgb, faces, _ = CI.punched("sphere")
    big = np.concatenate([faces, CI.disjoint_triangles(5)[2] + len(xyz)])
    bx, bc = np.concatenate([xyz, CI.disjoint_triangles(5)[0] + 100.0]), np.concatenate([rgb, CI.disjoint_triangles(5)[1]])
    perm = np.random.default_rng(7).permutation(len(big))
    a, b = run_gpu(bx, bc, big, min_faces=2), run_gpu(bx, bc, big[perm], min_faces=2)
    assert a["info"]["faces_removed"] == 5 and {k: v for k, v in a["info"].items() if k != "component_rounds"} == \
        {k: v for k, v in b["info"].items() if k != "component_rounds"}
    rows = lambda f: sorted(map(tuple, f.tolist()))  # noqa: E731
    assert rows(a["surviving"]) == rows(b["surviving"]) and np.array_equal(a["labels"], b["labels"])
    # the same loops up to relabelling: the same sets of rim edges
    def rims(g):
        tail, head = R.half_edges(g["surviving"].astype(np.int64))
        return sorted(tuple(sorted(zip(tail[g["loop"] == l].tolist(), head[g["loop"] == l].tolist()))) for l in np.unique(g["loop"]) if l >= 0)
    assert rims(a) == rims(b) and len(rims(a)) == 16
    # the centres sum the same rim vertices in another order: equal to a unit in the last place of the relative position
    ca, cb = np.sort(a["centre"], 0), np.sort(b["centre"], 0)
    assert (np.abs(ca - cb) <= 2 * np.spacing(np.abs(ca).max())).all() and np.array_equal(np.sort(a["colour"], 0), np.sort(b["colour"], 0))


def test_far_from_the_origin():
    """Coordinates in multiples of 2^-16 below 128 m: the shift by OFFSET is exact, so p = xyz - O has the near scene's bits and
    so has every value computed from it; every integer comes out the same."""
    xyz, rgb, faces, _ = CI.punched("sphere")
    xyz = np.round(xyz * 65536.0) / 65536.0
    far = xyz + OFFSET
    assert ((far - OFFSET) == xyz).all()
    near = run_gpu(xyz, rgb, faces, origin=(0.0, 0.0, 0.0), min_area=1.0)
    g = run_gpu(far, rgb, faces, origin=tuple(OFFSET), min_area=1.0)
    for k in ("labels", "kept", "boundary", "successor", "loop", "closed", "colour"):
        assert np.array_equal(g[k], near[k]), k
    assert g["p0"].tobytes() == near["p0"].tobytes() and g["component_area"].tobytes() == near["component_area"].tobytes()
    assert g["info"] == near["info"] and g["info"]["fill_vertices"] == 16
    assert (np.abs((g["centre"] - OFFSET) - near["centre"]) <= np.spacing(np.abs(g["centre"]))).all()
    hold(g, R.clean(far, rgb, faces, origin=tuple(OFFSET), min_area=1.0), "far:")


# ---- edge cases -------------------------------------------------------------------------------------------------------------------
def test_empty_meshes():
    import torch
    x, c, f, info = clean.clean(torch.empty(0, 3, dtype=torch.float64).cuda(), torch.empty(0, 3, dtype=torch.uint8).cuda(),
                                torch.empty(0, 3, dtype=torch.int64).cuda())
    assert tuple(x.shape) == (0, 3) and tuple(c.shape) == (0, 3) and tuple(f.shape) == (0, 3) and f.dtype == torch.int32
    assert info["vertices"] == info["faces"] == info["vertices_in"] == 0 and set(info) == set(clean.COUNTS)
    xyz, rgb, faces = CI.hand_mesh()
    g = run_gpu(xyz, rgb, np.zeros((0, 3), np.int64))                               # vertices without faces: none is used
    assert g["out_xyz"].shape == (0, 3) and g["out_faces"].shape == (0, 3) and g["info"]["vertices_in"] == len(xyz) - 1
    g, _ = both(xyz, rgb, faces, "everything removed:", min_faces=1000)
    assert g["out_xyz"].shape == (0, 3) and g["out_rgb"].shape == (0, 3) and g["out_faces"].shape == (0, 3)
    assert g["info"]["components_kept"] == 0 and g["info"]["faces_removed"] == len(faces) - 1 and g["info"]["vertices"] == 0
    g = run_gpu(xyz[:3], rgb[:3], np.array([[0, 0, 1], [2, 2, 2]]))                 # only degenerate faces
    assert g["out_faces"].shape == (0, 3) and g["info"]["faces_degenerate"] == 2


def test_refusals():
    import torch
    xyz, rgb, faces = CI.hand_mesh()
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    with pytest.raises(_lib.AdaMVSHipError, match="no CPU fallback"):
        clean.clean(torch.from_numpy(xyz), t(rgb), t(faces))
    with pytest.raises(_lib.AdaMVSHipError, match="no CPU fallback"):
        clean.clean(t(xyz), t(rgb), torch.from_numpy(faces))
    with pytest.raises(_lib.AdaMVSHipError, match="float64"):
        clean.clean(t(xyz.astype(np.float32)), t(rgb), t(faces))
    with pytest.raises(_lib.AdaMVSHipError, match=r"\[nf, 3\]"):
        clean.clean(t(xyz), t(rgb), t(faces[:, :2].copy()))
    with pytest.raises(_lib.AdaMVSHipError, match="refers to vertex"):
        clean.clean(t(xyz), t(rgb), t(faces + 20))
    bad = xyz.copy()
    bad[3, 1] = np.nan
    with pytest.raises(_lib.AdaMVSHipError, match="not finite"):
        clean.clean(t(bad), t(rgb), t(faces))
    with pytest.raises(ValueError, match="max_hole_edges"):
        clean.clean(t(xyz), t(rgb), t(faces), max_hole_edges=4097)
    # the entry points refuse before any launch
    sf = t(faces[:40].astype(np.int32))
    bnd = hip_ops.clean_boundary(sf)
    st = hip_ops.clean_successor(sf, len(xyz), bnd)
    with pytest.raises(_lib.AdaMVSHipError, match="max_hole_edges"):
        hip_ops.clean_validate(bnd, st["succ"], st["lab"], st["broken"], 4097)
    with pytest.raises(_lib.AdaMVSHipError, match="double-buffered"):
        hip_ops.clean_double(bnd, (st["lab"], st["nxt"], st["broken"]), (st["lab"], st["nxt"], st["broken"]))
    parent = torch.arange(len(xyz), dtype=torch.int32).cuda()
    with pytest.raises(_lib.AdaMVSHipError, match="double-buffered"):
        hip_ops.clean_components_round(sf, parent, parent, torch.zeros(1, dtype=torch.int32).cuda())
    with pytest.raises(_lib.AdaMVSHipError, match="int32"):
        hip_ops.clean_components_round(sf, parent.to(torch.int64), parent, torch.zeros(1, dtype=torch.int32).cuda())


def test_the_cli_writes_the_mesh_and_its_json(tmp_path):
    xyz, rgb, faces = CI.hand_mesh()
    src = str(tmp_path / "mesh.ply")
    write_mesh(src, xyz, rgb, faces, META)
    res = clean.main(["--output_folder", str(tmp_path), "--min_faces", "2", "--max_hole_edges", "4"])
    out = str(tmp_path / "mesh_cleaned.ply")
    assert res["ply"] == out and (tmp_path / "mesh_cleaned.ply.json").exists()
    on_disk = json.load(open(out + ".json"))
    for k in clean.COUNTS + TIMINGS + clean.CARRIED + ("min_faces", "min_area", "max_hole_edges", "source", "ply", "clean_origin"):
        assert k in on_disk, k
    r = R.clean(xyz, rgb, faces, min_faces=2, max_hole_edges=4, origin=META["origin"])
    verts, f = mesh.read_mesh_ply(out)
    assert np.array_equal(f.astype(np.int64), r["faces"]) and all(on_disk[k] == r["info"][k] for k in EXACT_INFO)
    assert np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float64).tobytes() == r["xyz"].tobytes()
