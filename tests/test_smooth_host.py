"""Mesh smoothing without a GPU: the options, the parser and its defaults, how sigma_s and the cap resolve, what <out>.json
carries over, the binding's symbols, and the quality of the rule itself: the numpy restatement (tests/smooth_ref.py) at the
default options on the box and the sphere of tests/simplify_inputs.py, clean and with noise of 0.1 voxel.

The bars, with what the restatement measures next to them (smooth_inputs.EXPECT):
  noisy box, flat vertices (farther than 2 voxels from every box edge):   RMS distance falls at least 2x     0.0998 -> 0.0313
  noisy box, edge vertices (within 1 voxel of a box edge):                RMS grows by no more than 10 %     0.1294 -> 0.1273
  noisy sphere:                                                           RMS falls at least 2x              0.1024 -> 0.0334
  clean box, smoothed: 99th percentile <= 1.0 voxel, median <= 0.25 voxel                                    0.234, 0.004
  no vertex moves farther than cap (1 + 1e-12)                                                               largest move 0.53
  a mesh cut open: every boundary vertex keeps its input bits"""
import json

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, mesh, smooth
import smooth_inputs as SI
import smooth_ref as R


@pytest.fixture(scope="module")
def results():
    """The restatement at the defaults on the four meshes, once."""
    m = SI.meshes()
    return {k: R.smooth(*m[k], weld_first=False, **SI.DEFAULTS) for k in ("box", "box_noisy", "sphere_noisy")}


# ---- quality of the rule ---------------------------------------------------------------------------------------------------------
def test_inputs_are_the_welded_box_and_sphere():
    m = SI.meshes()
    assert (len(m["box"][0]), len(m["box"][2])) == (7938, 15872) and (len(m["sphere"][0]), len(m["sphere"][2])) == (5628, 11252)
    assert abs(SI.rms(SI.box_distance(m["box_noisy"][0])) - 0.1) < 0.02


def test_noisy_box_flattens_and_keeps_its_edges(results):
    clean, noisy, out = SI.clean_of("box_noisy"), SI.meshes()["box_noisy"][0], results["box_noisy"]["xyz"]
    flat, edge = SI.box_edge_distance(clean) > 2.0, SI.box_edge_distance(clean) <= 1.0
    assert flat.sum() > 3000 and edge.sum() > 500
    d0, d1 = SI.box_distance(noisy), SI.box_distance(out)
    f0, f1, e0, e1 = SI.rms(d0[flat]), SI.rms(d1[flat]), SI.rms(d0[edge]), SI.rms(d1[edge])
    print("smooth: noisy box flat %.4f -> %.4f, edge %.4f -> %.4f" % (f0, f1, e0, e1))
    assert f1 <= f0 / 2.0, (f0, f1)
    assert e1 <= 1.1 * e0, (e0, e1)
    for got, want in zip((f0, f1, e0, e1), SI.EXPECT["box_flat"] + SI.EXPECT["box_edge"]):
        assert abs(got - want) < 5e-4, (got, want)


def test_noisy_sphere_smooths(results):
    d0, d1 = SI.sphere_distance(SI.meshes()["sphere_noisy"][0]), SI.sphere_distance(results["sphere_noisy"]["xyz"])
    print("smooth: noisy sphere %.4f -> %.4f" % (SI.rms(d0), SI.rms(d1)))
    assert SI.rms(d1) <= SI.rms(d0) / 2.0, (SI.rms(d0), SI.rms(d1))
    assert abs(SI.rms(d0) - SI.EXPECT["sphere"][0]) < 5e-4 and abs(SI.rms(d1) - SI.EXPECT["sphere"][1]) < 5e-4


def test_clean_box_stays_on_the_surface(results):
    d = SI.box_distance(results["box"]["xyz"])
    print("smooth: clean box median %.4f, 99th percentile %.4f" % (np.median(d), np.percentile(d, 99)))
    assert np.percentile(d, 99) <= 1.0 and np.median(d) <= 0.25
    assert abs(np.percentile(d, 99) - SI.EXPECT["clean_p99"]) < 5e-3


def test_no_vertex_moves_farther_than_the_cap(results):
    for k, r in results.items():
        move = np.linalg.norm(r["p"] - r["p0"], axis=1)
        assert move.max() <= SI.DEFAULTS["max_move"] * (1 + 1e-12), (k, move.max())
        assert r["info"]["clamped"] == 0
    assert abs(results["box_noisy"]["info"]["largest_move"] - SI.EXPECT["max_move"]) < 5e-3
    # where the clamp binds it holds too
    m = SI.meshes()["box_noisy"]
    r = R.smooth(*m, weld_first=False, **SI.OTHER)
    move = np.linalg.norm(r["p"] - r["p0"], axis=1)
    assert r["info"]["clamped"] > 0 and move.max() <= SI.OTHER["max_move"] * (1 + 1e-12), (r["info"], move.max())


def test_boundary_vertices_keep_their_bits():
    xyz, rgb, faces = SI.cut_open(*SI.meshes()["box"])
    assert len(faces) < 15872
    r = R.smooth(xyz, rgb, faces, weld_first=False, **SI.DEFAULTS)
    assert 50 < r["info"]["fixed"] < 500 and r["fixed"].sum() == r["info"]["fixed"]
    assert r["xyz"][r["fixed"]].tobytes() == xyz[r["fixed"]].tobytes()
    assert (r["xyz"][~r["fixed"]] != xyz[~r["fixed"]]).any()
    free = R.smooth(xyz, rgb, faces, weld_first=False, fix_boundary=False, **SI.DEFAULTS)
    assert free["info"]["fixed"] == 0 and (free["xyz"][r["fixed"]] != xyz[r["fixed"]]).any()
    assert np.array_equal(r["faces"], faces) and np.array_equal(r["rgb"], rgb)


def test_hand_made_mesh_holds_what_it_is_meant_to_hold():
    xyz, rgb, faces = SI.hand_mesh()
    assert len(xyz) == 23 and (xyz * 8 == np.round(xyz * 8)).all()
    r = R.smooth(xyz, rgb, faces, sigma_s=1.0, normal_iters=3, vertex_iters=2, max_move=1.0)
    w = r["faces"]
    assert r["info"]["degenerate_faces"] == 2 and (r["area"] == 0).sum() == 2
    assert (np.array([len(f) for f in r["F"]]) == 0).sum() == 1                     # a vertex without a face
    edges = np.sort(np.concatenate([w[:, [0, 1]], w[:, [1, 2]], w[:, [2, 0]]]), 1)
    _, cnt = np.unique(edges, axis=0, return_counts=True)
    assert (cnt == 3).sum() == 1 and (cnt == 1).sum() > 4 and 0 < (~r["fixed"]).sum()
    # the crease: the two sides of the roof keep distinct normals
    assert np.abs(r["normals"][0] - r["normals"][2]).max() > 0.5
    # the cancelling face: zero area, two opposite neighbours, its normal stays the zero vector
    f = int(np.nonzero((r["area"] == 0) & (np.array([len(n) for n in r["N"]]) == 3))[0][0])
    assert (r["normals"][f] == 0).all() and (r["normals"][r["N"][f][1]] == -r["normals"][r["N"][f][2]]).all()


# ---- the options, the parser, the JSON, the binding --------------------------------------------------------------------------
def test_check_options():
    smooth.check_options(0.25)
    smooth.check_options(0.25, 0.35, 0, 1000, 0.1)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="sigma_s"):
            smooth.check_options(bad)
        with pytest.raises(ValueError, match="sigma_r"):
            smooth.check_options(1.0, sigma_r=bad)
        with pytest.raises(ValueError, match="max_move"):
            smooth.check_options(1.0, max_move=bad)
    for bad in (-1, 1001, 2.5, float("nan"), None, True):
        with pytest.raises(ValueError, match="normal_iters"):
            smooth.check_options(1.0, normal_iters=bad)
        with pytest.raises(ValueError, match="vertex_iters"):
            smooth.check_options(1.0, vertex_iters=bad)


def test_parser_and_defaults():
    ap = smooth.build_parser()
    a = ap.parse_args(["--output_folder", "o"])
    assert (a.mesh, a.sigma_s, a.sigma_s_voxels, a.sigma_r, a.normal_iters, a.vertex_iters, a.max_move, a.max_move_voxels, a.no_fix_boundary,
            a.origin, a.out) == (None, None, None, 0.35, 10, 10, None, None, False, None, None)
    assert smooth.mesh_path_of(a) == "o/mesh.ply" and smooth.default_out("o/mesh.ply") == "o/mesh_smoothed.ply"
    assert smooth.default_out("a/b.PLY") == "a/b_smoothed.ply" and smooth.default_out("a/b") == "a/b_smoothed.ply"
    a = ap.parse_args(["--mesh", "m.ply", "--sigma_s", "0.5", "--sigma_r", "0.2", "--normal_iters", "3", "--vertex_iters", "0", "--max_move_voxels",
                       "2", "--no_fix_boundary", "--origin", "1", "2", "3", "--out", "x.ply"])
    assert (smooth.mesh_path_of(a), a.sigma_s, a.sigma_r, a.normal_iters, a.vertex_iters, a.max_move_voxels, a.no_fix_boundary, a.origin,
            a.out) == ("m.ply", 0.5, 0.2, 3, 0, 2.0, True, [1.0, 2.0, 3.0], "x.ply")
    with pytest.raises(ValueError, match="--mesh or --output_folder"):
        smooth.mesh_path_of(ap.parse_args([]))


def test_sigma_s_and_the_cap_resolve():
    meta = {"voxel": 0.25}
    assert smooth.resolve_sigma_s(None, None, meta) == 0.25 and smooth.resolve_max_move(None, None, meta) == 0.25      # one voxel by default
    assert smooth.resolve_sigma_s(None, 2, meta) == 0.5 and smooth.resolve_sigma_s(0.3, None, None) == 0.3
    assert smooth.resolve_max_move(None, 0.5, meta) == 0.125 and smooth.resolve_max_move(0.7, None, meta) == 0.7
    with pytest.raises(ValueError, match="not both"):
        smooth.resolve_sigma_s(0.3, 2, meta)
    with pytest.raises(ValueError, match="not both"):
        smooth.resolve_max_move(0.3, 2, meta)
    with pytest.raises(ValueError, match="--sigma_s"):
        smooth.resolve_sigma_s(None, None, None)                                   # without the JSON --sigma_s is required
    with pytest.raises(ValueError, match="--sigma_s"):
        smooth.resolve_sigma_s(None, 2, {"mu": 1.0})
    with pytest.raises(ValueError, match="--max_move"):
        smooth.resolve_max_move(None, None, None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma_s"):
            smooth.resolve_sigma_s(bad, None, meta)
        with pytest.raises(ValueError, match="sigma_s_voxels"):
            smooth.resolve_sigma_s(None, bad, meta)
        with pytest.raises(ValueError, match="max_move_voxels"):
            smooth.resolve_max_move(None, bad, meta)


def test_summary_carries_the_mesh_json_over():
    from ada_mvs_amd import simplify
    meta = dict(voxel=0.25, mu=1.0, origin=[1.0, 2.0, 3.0], views=5, brick=128, vertices=10, faces=20, seconds=3.0)
    info = dict(vertices=9, faces=20, fixed=2, degenerate_faces=1, clamped=3, largest_move=0.2, rms_move=0.05)
    options = dict(sigma_s=0.25, sigma_r=0.35, normal_iters=10, vertex_iters=10, max_move=0.25, fix_boundary=True)
    res = smooth.summary(meta, info, options, np.array([1.0, 2.0, 3.0]), "m.ply", "s.ply", 2.0, 0.5, {"filter": 0.1})
    assert smooth.CARRIED is simplify.CARRIED
    assert [res[k] for k in smooth.CARRIED] == [0.25, 1.0, [1.0, 2.0, 3.0], 5] and "brick" not in res
    assert (res["smooth_origin"], res["source"], res["ply"]) == ([1.0, 2.0, 3.0], "m.ply", "s.ply")
    assert all(res[k] == v for k, v in info.items()) and all(res[k] == v for k, v in options.items())
    assert (res["seconds"], res["device_seconds"], res["stage_seconds"]) == (2.0, 0.5, {"filter": 0.1})
    json.dumps(res)
    assert "voxel" not in smooth.summary(None, info, options, np.zeros(3), "m.ply", "s.ply", 0.0, 0.0)
    assert simplify.resolve_cell(None, 2, res) == 0.5                                # simplify_whu.py --cell_voxels keeps working


def test_binding_constants_and_symbols():
    assert _lib.ABI_VERSION == 22 and _lib.SMOOTH_TILE == 256
    for name in ("faces", "edge_keys", "boundary", "filter", "centroids", "update"):
        assert "adamvs_smooth_" + name in _lib.SIGNATURES
        assert hasattr(_lib.load(), "adamvs_smooth_" + name)


def test_refusals(tmp_path):
    import torch
    xyz, rgb, faces = SI.hand_mesh()
    src = str(tmp_path / "m.ply")
    with mesh.MeshPlyWriter(src) as w:
        w.write(xyz, rgb, faces.astype(np.uint32))
    with pytest.raises(ValueError, match="<mesh>.json"):
        smooth.from_file(src)                                                      # no JSON and no --sigma_s
    with pytest.raises(ValueError, match="--max_move"):
        smooth.from_file(src, sigma_s=1.0)
    with pytest.raises(ValueError, match="not both"):
        smooth.from_file(src, sigma_s=1.0, sigma_s_voxels=2, max_move=1.0)
    with pytest.raises(SystemExit, match="not both"):
        smooth.main(["--mesh", src, "--sigma_s", "1", "--sigma_s_voxels", "2"])
    with pytest.raises(SystemExit, match="not both"):
        smooth.main(["--mesh", src, "--sigma_s", "1", "--max_move", "1", "--max_move_voxels", "2"])
    with pytest.raises(ValueError, match="normal_iters"):
        smooth.from_file(src, sigma_s=1.0, max_move=1.0, normal_iters=1001)
    with pytest.raises(ValueError, match="sigma_r"):
        smooth.from_file(src, sigma_s=1.0, max_move=1.0, sigma_r=0.0)
    assert not (tmp_path / "m_smoothed.ply").exists()
    # there is no CPU path
    with pytest.raises(_lib.AdaMVSHipError, match="no CPU fallback"):
        smooth.smooth(torch.from_numpy(xyz), torch.from_numpy(rgb), torch.from_numpy(faces), 1.0, max_move=1.0)
