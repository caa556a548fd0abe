"""TSDF mesh, host side (no GPU): the restatement (tests/mesh_ref.py) on cases known in closed form, conservative view culling,
the mesh PLY writer, argument errors of the C ABI, the wrapper's refusal of host tensors, and the crafted inputs of
tests/mesh_inputs.py against the restatement: every precondition that tests/test_mesh_edges_gpu.py relies on."""
import ctypes
import itertools
from fractions import Fraction

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, fusion_synth, mesh
import mesh_inputs as I
import mesh_ref as M

SPHERE_CENTRE = (32.37, 31.81, 32.23)


# ---- one tetrahedron ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", range(6))
def test_the_sixteen_cases_of_a_tet(t):
    v = M.tet_vertices(t).astype(np.float64)
    rng = np.random.default_rng(t)
    for case in range(16):
        tris = M.case_triangles(t, case)
        nin = bin(case).count("1")
        assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[nin]
        # a tsdf with these signs, linear along the edges: vertices on the sign-changing edges, normals along the gradient
        tv = np.where([(case >> k) & 1 for k in range(4)], -rng.uniform(0.1, 1.0, 4), rng.uniform(0.1, 1.0, 4)).astype(np.float32)
        for tri in tris:
            P = []
            for i, j in tri:
                assert ((case >> i) & 1) != ((case >> j) & 1)
                lam = np.float32(tv[i] / (tv[i] - tv[j]))
                P.append(v[i] + float(lam) * (v[j] - v[i]))
            n = np.cross(P[1] - P[0], P[2] - P[0])
            # the affine tsdf through the 4 vertex values has a gradient pointing to increasing tsdf
            A = np.c_[v, np.ones(4)]
            grad = np.linalg.solve(A, tv.astype(np.float64))[:3]
            assert n @ grad > 0, (t, case, tri)


def test_every_kuhn_edge_runs_in_one_of_the_seven_positive_directions():
    seen = set()
    for t in range(6):
        for (i, j), (start, e) in M.tet_edges(t).items():
            assert (M.tet_vertices(t)[j] - M.tet_vertices(t)[i] == M.DIRS[e]).all()
            seen.add(e)
    assert seen == set(range(7))


# ---- the analytic sphere ------------------------------------------------------------------------------------------------------
def sphere_mesh(B=32, radius=10.0):
    vol = M.sphere_volume(B, SPHERE_CENTRE, radius, 4.0)
    xs, fs, base = [], [], 0
    for b in sorted(vol):
        r = M.extract((0.0, 0.0, 0.0), 1.0, B, b, *vol[b], min_weight=1, vertex_base=base)
        xs.append(r["xyz"])
        fs.append(r["faces"])
        base += len(r["xyz"])
    return np.concatenate(xs), np.concatenate(fs)


def test_sphere_over_eight_bricks_is_closed_after_welding():
    xyz, faces = sphere_mesh()
    u, f = M.weld(xyz, faces)
    assert len(u) < len(xyz)                                  # the seams were written twice
    closed, chi = M.closed_and_oriented(f)
    assert closed and chi == 2
    vol = M.signed_volume(u - np.asarray(SPHERE_CENTRE), f)
    assert abs(vol / (4.0 / 3.0 * np.pi * 1000.0) - 1.0) < 0.01, vol
    d = np.linalg.norm(u - np.asarray(SPHERE_CENTRE), axis=1)
    assert np.abs(d - 10.0).max() < 0.2


def test_min_weight_leaves_unprocessed_cubes_out():
    B = 32
    vol = M.sphere_volume(B, (16.3, 16.2, 16.1), 6.0, 4.0, nb=1)[(0, 0, 0)]
    t, w, c = vol
    w = w.copy()
    w[M.sample_grid(B, (0, 0, 0))[:, 0] > 16] = 0
    full = M.extract((0, 0, 0), 1.0, B, (0, 0, 0), t, np.ones_like(w), c)
    half = M.extract((0, 0, 0), 1.0, B, (0, 0, 0), t, w, c, min_weight=1)
    assert 0 < len(half["faces"]) < len(full["faces"])
    assert (half["xyz"][:, 0] <= 16.0).all()


# ---- integration ------------------------------------------------------------------------------------------------------------
def test_a_plane_seen_by_one_camera_gives_a_linear_tsdf():
    H, W = 64, 80
    K = fusion_synth.intrinsics(H, W)
    C = np.array([3.0, -2.0, 120.0])
    R_wc = fusion_synth.look_at(C, C - np.array([0.0, 0.0, 1.0]))
    depth = np.full((H, W), np.float32(120.0))                 # the plane z = 0 straight below
    rgba = np.full((H, W, 4), 77, np.uint8)
    origin = np.array([-10.0, -10.0, -6.0])
    voxel, mu = 0.5, 2.0
    view = M.view_record(K, R_wc, C, origin, depth, rgba)
    r = M.integrate(voxel, mu, 32, (0, 0, 0), [view], [0])
    g = M.sample_grid(32, (0, 0, 0))
    h = origin[2] + g[:, 2] * np.float32(voxel)                 # height of the sample above the plane
    seen = r["weight"] > 0
    assert seen.any() and not seen[h < -mu - 1e-3].any()
    assert np.abs(r["tsdf"][seen] - np.minimum(1.0, h[seen] / mu)).max() < 1e-4
    col = seen & (np.abs(h) <= mu - 1e-3)
    assert (r["rgba"][col] == (77 | 77 << 8 | 77 << 16 | 255 << 24)).all()
    assert (r["rgba"][seen & (h > mu + 1e-3)] == 0).all()


def test_depth_zero_is_unknown_not_free_space():
    H, W = 32, 32
    K = fusion_synth.intrinsics(H, W)
    C = np.array([0.0, 0.0, 50.0])
    R_wc = fusion_synth.look_at(C, (0.0, 0.0, 0.0))
    view = M.view_record(K, R_wc, C, (-4.0, -4.0, -4.0), np.zeros((H, W), np.float32), np.zeros((H, W, 4), np.uint8))
    r = M.integrate(0.25, 1.0, 32, (0, 0, 0), [view], [0])
    assert (r["weight"] == 0).all() and (r["tsdf"] == 0).all()


def test_culling_is_conservative():
    sc = fusion_synth.make_cameras(96, 128, 8)
    cams = [(c["K"], c["R"], c["C"], c["H"], c["W"]) for c in sc]
    rng = np.random.default_rng(3)
    origin, voxel, B, mu = np.array([-150.0, -150.0, -10.0]), 1.0, 32, 4.0
    culled = 0
    for b in itertools.product(range(10), range(10), range(3)):
        lo, hi = mesh.brick_box(origin, voxel, B, b, mu)
        keep = set(mesh.cull_views(lo, hi, cams))
        culled += len(cams) - len(keep)
        X = lo + rng.random((400, 3)) * (hi - lo)
        for i, (K, R, C, H, W) in enumerate(cams):
            p = (X - C) @ R
            front = p[:, 2] > 0
            u = (p @ K[0])[front] / p[front, 2]
            v = (p @ K[1])[front] / p[front, 2]
            sees = ((np.floor(u + 0.5) >= 0) & (np.floor(u + 0.5) < W) & (np.floor(v + 0.5) >= 0) & (np.floor(v + 0.5) < H)).any()
            assert not sees or i in keep, (b, i)
    assert culled > 0                                          # and it does cull


# ---- the PLY writer -------------------------------------------------------------------------------------------------------------
def test_mesh_ply_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    path = str(tmp_path / "m.ply")
    parts = [(rng.normal(size=(n, 3)) * 1e5, rng.integers(0, 256, (n, 3)).astype(np.uint8), rng.integers(0, 1000, (m, 3)).astype(np.uint32))
             for n, m in ((10, 7), (0, 0), (33, 50), (1, 0))]
    with mesh.MeshPlyWriter(path) as w:
        for xyz, rgb, f in parts:
            w.write(xyz, rgb, f)
        assert w.vertices == 44 and w.faces == 57
    assert not (tmp_path / "m.ply.faces.tmp").exists()
    verts, faces = mesh.read_mesh_ply(path)
    assert len(verts) == 44 and len(faces) == 57
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), np.concatenate([p[0] for p in parts]))
    assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), np.concatenate([p[1] for p in parts]))
    assert np.array_equal(faces, np.concatenate([p[2] for p in parts]))
    head = open(path, "rb").read(400).decode("ascii", "replace")
    assert "element vertex 0000000044\n" in head and "element face 0000000057\n" in head
    assert "property list uchar uint vertex_indices\n" in head
    assert mesh.mesh_ply_header(0, 0).__len__() == mesh.mesh_ply_header(44, 57).__len__()


def test_grid_refuses_volumes_past_the_extent():
    o, nb = mesh.grid_for_bounds((0, 0, 0), (100.0, 50.0, 10.0), 0.25, 128)
    assert list(nb) == [4, 2, 1]
    with pytest.raises(ValueError, match="exceeds"):
        mesh.grid_for_bounds((0, 0, 0), (20000.0, 10.0, 10.0), 1.0, 32)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------
def test_mesh_argument_errors_without_a_gpu():
    lib = _lib.load()
    dummy = ctypes.c_void_p(256)               # never dereferenced: every call below is refused before a launch
    null = ctypes.c_void_p(0)

    def brick(**kw):
        d = dict(origin=(0.0, 0.0, 0.0), voxel=0.5, mu=2.0, B=32, bx=0, by=0, bz=0, min_weight=1)
        d.update(kw)
        b = _lib.MeshBrick()
        b.origin[:] = d.pop("origin")
        for k, v in d.items():
            setattr(b, k, v)
        return ctypes.byref(b)

    def integ(b=None, views=dummy, nv=4, lst=dummy, nl=2, t=dummy, w=dummy, c=dummy):
        return lib.adamvs_tsdf_integrate(b or brick(), views, nv, lst, nl, t, w, c, null)

    nan, inf = float("nan"), float("inf")
    cases = {
        "null brick": lib.adamvs_tsdf_integrate(ctypes.POINTER(_lib.MeshBrick)(), dummy, 4, dummy, 2, dummy, dummy, dummy, null),
        "null views": integ(views=null), "null list": integ(lst=null), "null tsdf": integ(t=null), "null weight": integ(w=null),
        "null rgba": integ(c=null), "B 16": integ(brick(B=16)), "B 256": integ(brick(B=256)), "voxel 0": integ(brick(voxel=0.0)),
        "voxel NaN": integ(brick(voxel=nan)), "mu < 0": integ(brick(mu=-1.0)), "mu inf": integ(brick(mu=inf)),
        "origin NaN": integ(brick(origin=(0.0, nan, 0.0))), "brick < 0": integ(brick(by=-1)),
        "brick past the extent": integ(brick(B=128, voxel=1.0, bz=128)), "min_weight 0": integ(brick(min_weight=0)),
        "nviews 0": integ(nv=0), "too many views": integ(nv=65536), "nlist > nviews": integ(nl=5), "nlist < 0": integ(nl=-1),
        "classify null": lib.adamvs_mesh_classify(brick(), dummy, null, dummy, dummy, null),
        "classify min_weight": lib.adamvs_mesh_classify(brick(min_weight=70000), dummy, dummy, dummy, dummy, null),
        "count null": lib.adamvs_mesh_count_vertices(brick(), dummy, dummy, null, dummy, null),
        "count B": lib.adamvs_mesh_count_vertices(brick(B=48), dummy, dummy, dummy, dummy, null),
        "emit null": lib.adamvs_mesh_emit(brick(), dummy, dummy, dummy, dummy, null, dummy, 0, dummy, dummy, dummy, 1, dummy, 1, null),
        "emit capacity < 0": lib.adamvs_mesh_emit(brick(), dummy, dummy, dummy, dummy, dummy, dummy, 0, dummy, dummy, dummy, -1, dummy, 1, null),
        "emit null faces": lib.adamvs_mesh_emit(brick(), dummy, dummy, dummy, dummy, dummy, dummy, 0, dummy, dummy, dummy, 1, null, 1, null),
    }
    # the brick at the extent itself is accepted by the checks: (b + 1) B s = 16384
    assert lib.adamvs_mesh_count_vertices(brick(B=128, voxel=1.0, bx=127), dummy, dummy, null, dummy, null) < 0   # (null mask)

    def view(**kw):
        arr = (_lib.MeshView * 2)()
        for v in arr:
            v.K[:] = [100.0, 0, 50.0, 0, 100.0, 40.0, 0, 0, 1.0]
            v.R[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
            v.c[:] = [10.0, 20.0, 30.0]
            v.H, v.W, v.depth, v.rgba = 80, 100, 256, 512
        for k, val in kw.items():
            if k in ("K", "R", "c"):
                getattr(arr[1], k)[:] = val
            else:
                setattr(arr[1], k, val)
        return lib.adamvs_mesh_check_views(arr, 2)

    assert view() == 0
    cases.update({
        "view null depth": view(depth=None), "view W 0": view(W=0), "view K NaN": view(K=[nan] * 9),
        "view K last row": view(K=[100.0, 0, 50.0, 0, 100.0, 40.0, 0, 0, 2.0]), "view R inf": view(R=[inf] * 9),
        "camera past the extent": view(c=[0.0, 16500.0, 0.0]), "views null": lib.adamvs_mesh_check_views(None, 1),
    })
    for what, rc in cases.items():
        assert rc < 0, what
        with pytest.raises(_lib.AdaMVSHipError, match="invalid argument"):
            _lib.check(int(rc), what)


def test_wrapper_refuses_host_tensors():
    import torch
    from ada_mvs_amd import hip_ops
    b = hip_ops.mesh_brick((0, 0, 0), 1.0, 4.0, 32, (0, 0, 0))
    S = 33 ** 3
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        hip_ops.mesh_extract(b, torch.zeros(S), torch.zeros(S, dtype=torch.int16), torch.zeros(S, dtype=torch.int32))
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        hip_ops.tsdf_integrate(b, torch.zeros(112, dtype=torch.uint8), 1, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.AdaMVSHipError, match="GPU tensor"):
        hip_ops.mesh_views([(np.eye(3), np.eye(3), np.zeros(3), torch.zeros(4, 5), torch.zeros(4, 5, 4, dtype=torch.uint8))], "cpu")


# ---- the crafted inputs of tests/mesh_inputs.py: every precondition of the GPU tests, from the restatement alone -------------
@pytest.mark.parametrize("B,voxel,mu,b,min_weights", I.SCENE_CASES)
def test_scene_bricks_at_64_and_128_have_views_surface_and_few_ties(B, voxel, mu, b, min_weights):
    case = I.scene_reference(B, voxel, mu, b)
    ref = case["ref"]
    assert len(case["vl"]) >= 3
    assert (~ref["tie"]).mean() > 0.8, ref["tie"].mean()
    assert (B + 1) ** 3 > 1 << 16 and I.SCENE_ORIGIN[0] + b[0] * B * voxel != 0
    # a cube processed at the largest min_weight is processed at every smaller one, and a cube's triangles depend on signs alone:
    # the face count at the largest min_weight bounds the others from below
    faces = M.extract(I.SCENE_ORIGIN, voxel, B, b, ref["tsdf"], ref["weight"], ref["rgba"], max(min_weights))["faces"]
    assert len(faces) > 100


def test_threshold_scene_is_exact_and_meets_every_threshold():
    recs = I.threshold_records()
    for vl in ([0, 1], [0, 1, 2]):
        exact = I.exact_samples(recs, vl)
        ref = I.threshold_reference(vl)
        assert exact.sum() >= 3000
        assert (exact & (ref["weight"] >= 1)).sum() > 250 and (exact & (ref["rgba"] != 0)).sum() > 100
        assert ref["tie"][exact].mean() > 0.2                  # samples the tie mask would have left out
        for name, hit in I.threshold_events(recs, vl).items():
            assert (hit & exact).sum() > 0, (vl, name)
    # with the wide nadir view most EXACT samples carry weight
    assert (ref["weight"][exact] >= 1).mean() > 0.5
    # the planted and the bad pixels do what they were placed for (sample (x, y, z) -> entry (z 33 + y) 33 + x)
    at = lambda x, y, z: (z * 33 + y) * 33 + x  # noqa: E731
    one = I.threshold_reference([1])
    assert exact[at(14, 16, 17)] and one["weight"][at(14, 16, 17)] == 1 and one["tsdf"][at(14, 16, 17)] == -1.0     # depth 1e-45 at z = 4
    assert one["rgba"][at(14, 16, 17)] != 0
    assert one["weight"][at(26, 8, 17)] == 1 and one["tsdf"][at(26, 8, 17)] == -1.0 and one["rgba"][at(26, 8, 17)] != 0   # sdf = -mu
    assert one["weight"][at(26, 10, 17)] == 0                                                                          # sdf = -mu - 1/4
    assert one["weight"][at(18, 12, 17)] == 1 and one["tsdf"][at(18, 12, 17)] == 1.0 and one["rgba"][at(18, 12, 17)] != 0  # sdf = +mu
    assert one["weight"][at(18, 13, 17)] == 1 and one["rgba"][at(18, 13, 17)] == 0                                     # sdf = +mu + 1/4
    assert one["weight"][at(18, 20, 17)] == 1 and one["tsdf"][at(18, 20, 17)] == 1.0 and one["rgba"][at(18, 20, 17)] == 0   # FLT_MAX
    assert (one["weight"][[at(18, y, 17) for y in range(15, 20)]] == 0).all()                     # NaN, +inf, -inf, 0, -3 are unknown
    assert (one["weight"][M.sample_grid(32, (0, 0, 0))[:, 0] <= 10] == 0).all()                   # at or behind the side camera


def test_threshold_scene_view_lists():
    recs = I.threshold_records()
    exact = I.exact_samples(recs, [0, 1])
    a, b = I.threshold_reference([0, 1]), I.threshold_reference([1, 0])
    assert np.array_equal(a["weight"], b["weight"]) and np.array_equal(a["rgba"], b["rgba"])
    assert np.array_equal(a["tsdf"][exact], b["tsdf"][exact])                                      # exact sums do not feel the order
    many = I.records(I.many_views(), I.TH["origin"])
    ref = M.integrate(I.TH["voxel"], I.TH["mu"], I.TH["B"], I.TH["b"], many, list(range(len(many))))
    assert len(many) == 300 and (ref["weight"][exact] == 300).sum() > 0 and ref["weight"].max() == 300
    both = ref["weight"] == 300
    assert np.array_equal(ref["rgba"][both], a["rgba"][both])                                     # 150 times the same two pixels


@pytest.mark.parametrize("B,tiny", [(32, False), (32, True), (64, False), (128, False)])
def test_crafted_volume_holds_every_case_and_scattered_unprocessed_cubes(B, tiny):
    vol = I.crafted_volume(B, tiny=tiny)
    ref = I.extraction_reference(I.FAR_ORIGIN, 0.1, B, (0, 0, 0), vol, key=(B, tiny, "far"))
    assert 0.15 < ref["processed"].mean() < 0.3
    cases = M.cube_cases(B, vol[0])[ref["processed"]]
    assert all(set(np.unique(cases[:, t])) == set(range(16)) for t in range(6))                   # all 96 (tet, case) pairs
    unused = I.used_by_none(B, ref)
    for e in range(7):
        assert ((ref["edge_mask"] >> e) & 1).sum() > 0 and ((unused >> e) & 1).sum() > 0, e
    assert np.isfinite(ref["xyz"]).all() and len(ref["faces"]) > 1000 and len(ref["xyz"]) > 1000
    t = vol[0]
    assert (np.signbit(t) & (t == 0)).any() and ((t == 0) & ~np.signbit(t)).any()                 # -0 and +0
    if B == 32 and not tiny:
        # voxel 0.1 shows a contracted multiply-add along z, where the origin is small: O + g s rounded once (exact rationals)
        # differs from the two roundings
        bits = (ref["edge_mask"][:, None] >> np.arange(7)) & 1
        n_idx, e_idx = (a[::20] for a in np.nonzero(bits))
        lam = (t[n_idx] / (t[n_idx] - t[n_idx + M.DIRS[e_idx] @ [1, B + 1, (B + 1) ** 2]])).astype(np.float32)
        g = M.sample_grid(B, (0, 0, 0))[n_idx, 2] + np.where(M.DIRS[e_idx, 2] == 1, lam.astype(np.float64), 0.0)
        once = np.array([float(Fraction(I.FAR_ORIGIN[2]) + Fraction(float(x)) * Fraction(0.1)) for x in g])
        assert 50 < (once != ref["xyz"][::20, 2]).sum() < len(once) // 2
    tiny_values = (t != 0) & (np.abs(t) < 2.0 ** -126)
    assert tiny_values.any() == tiny
    if tiny:
        # a subnormal value decides a sign: its edge to a zero or a positive neighbour carries a vertex
        B1 = B + 1
        n = np.nonzero(tiny_values & (t < 0))[0]
        n = n[(n % B1 < B)]
        assert ((t[n + 1] >= 0) & ((ref["edge_mask"][n] & 1) == 1)).sum() > 0


def test_crafted_special_volumes():
    B = 32
    t, w, c = I.crafted_volume(B)
    assert len(I.extraction_reference(I.FAR_ORIGIN, 0.1, B, (0, 0, 0), (t, w, c), 2)["faces"]) > 0
    for vol in ((np.abs(t) + np.float32(0.0), w, c), (t, np.zeros_like(w), c)):
        ref = M.extract(I.FAR_ORIGIN, 0.1, B, (0, 0, 0), *vol)
        assert len(ref["xyz"]) == 0 and len(ref["faces"]) == 0
    assert not np.signbit(np.abs(t) + np.float32(0.0)).any()
    for cube in ((0, 0, 0), (B - 1, B - 1, B - 1)):
        ref = M.extract(I.FAR_ORIGIN, 0.1, B, (0, 0, 0), *I.single_cube_volume(B, cube))
        assert ref["processed"].sum() == 1 and len(ref["faces"]) >= 6 and len(ref["xyz"]) >= 7
    last = I.single_cube_volume(B, (B - 1, B - 1, B - 1))
    assert np.nonzero(last[1])[0].min() // 256 >= 131 and np.nonzero(last[1])[0].max() == 33 ** 3 - 1 == 140 * 256 + 96
    # the last brick inside the extent, and a vertex_base at the top of uint32
    ref = I.extraction_reference(I.FAR_ORIGIN, 1.0, B, (511, 0, 3), (t, w, c), key=(B, "extent"))
    assert (511 + 1) * B * 1.0 == mesh.MAX_EXTENT and ref["xyz"][:, 0].max() > I.FAR_ORIGIN[0] + 16383
    nv = len(ref["xyz"])
    top = M.extract(I.FAR_ORIGIN, 1.0, B, (511, 0, 3), t, w, c, 1, 0xFFFFFFFF - nv)["faces"]
    assert top.dtype == np.uint32 and top.max() == 0xFFFFFFFE and np.array_equal(top - np.uint32(0xFFFFFFFF - nv), ref["faces"])
