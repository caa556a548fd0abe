"""The TSDF mesh kernels (csrc/mesh.hip) against the restatement (tests/mesh_ref.py) where tests/test_mesh_gpu.py does not reach:
the brick sizes 64 and 128 with a voxel that is not 1, integration at its thresholds on samples whose arithmetic is exact in
fp32 (bitwise, no tie mask), extraction on crafted volumes (every tet case, scattered unprocessed cubes, signed zeros,
subnormal values, the last brick of the extent, a vertex_base at the top of uint32), and the raw calls: every intermediate array
and the capacities.  tests/test_mesh_host.py asserts the preconditions of every input used here (tests/mesh_inputs.py)."""
import ctypes
import itertools

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, mesh
import mesh_inputs as I
import mesh_ref as M

pytestmark = pytest.mark.gpu


def device_views(views):
    import torch
    cache = {}

    def up(a):
        if id(a) not in cache:
            cache[id(a)] = torch.from_numpy(a).cuda()
        return cache[id(a)]
    return [dict(K=v["K"], R=v["R"], C=v["C"], depth=up(v["depth_h"]), rgba=up(v["rgba_h"])) for v in views]


def host(vol):
    t, w, c = vol
    return t.cpu().numpy(), w.cpu().numpy().view(np.uint16), c.cpu().numpy().view(np.uint32)


def upload(vol):
    import torch
    t, w, c = vol
    return (torch.from_numpy(np.ascontiguousarray(t)).cuda(), torch.from_numpy(np.ascontiguousarray(w).view(np.int16)).cuda(),
            torch.from_numpy(np.ascontiguousarray(c).view(np.int32)).cuda())


def assert_mesh_equals(got, ref):
    xyz, rgb, faces = got
    assert xyz.shape[0] == len(ref["xyz"]) and faces.shape[0] == len(ref["faces"]), (xyz.shape, faces.shape, len(ref["xyz"]), len(ref["faces"]))
    assert xyz.cpu().numpy().tobytes() == ref["xyz"].tobytes()
    assert np.array_equal(rgb.cpu().numpy(), ref["rgb"])
    assert np.array_equal(faces.cpu().numpy().view(np.uint32), ref["faces"])


# ---- A. brick sizes 64 and 128, voxel not 1 ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_dev():
    return device_views(I.scene_host())


@pytest.mark.parametrize("B,voxel,mu,b,min_weights", I.SCENE_CASES)
def test_scene_brick_matches_restatement(scene_dev, B, voxel, mu, b, min_weights):
    case = I.scene_reference(B, voxel, mu, b)
    ref, vl = case["ref"], case["vl"]
    mesher = mesh.TsdfMesher(I.SCENE_ORIGIN, voxel, mu, B, scene_dev)
    assert mesher.view_list(b) == vl and len(vl) >= 3
    vol = mesher.integrate(b, vl)
    t, w, c = host(vol)
    ok = ~ref["tie"]
    assert ok.mean() > 0.8, ok.mean()
    assert np.array_equal(w[ok], ref["weight"][ok]), np.argwhere(w[ok] != ref["weight"][ok])[:5]
    assert np.array_equal(c[ok], ref["rgba"][ok])
    err = np.abs(t.astype(np.float64) - ref["tsdf64"])
    assert (err[ok] <= case["bound"][ok]).all(), (err[ok] - case["bound"][ok]).max()
    assert (w > 0).mean() > 0.2 and (c != 0).any()
    for min_weight in min_weights:
        m2 = mesh.TsdfMesher(I.SCENE_ORIGIN, voxel, mu, B, scene_dev, min_weight=min_weight)
        want = M.extract(I.SCENE_ORIGIN, voxel, B, b, t, w, c, min_weight, 1234)
        assert len(want["faces"]) > 100
        assert_mesh_equals(m2.extract(b, vol, vertex_base=1234), want)


def test_shared_layers_of_adjacent_bricks_are_bit_identical_at_64(scene_dev):
    B, voxel, mu = 64, 0.5, 2.0
    B1 = B + 1
    mesher = mesh.TsdfMesher(I.SCENE_ORIGIN, voxel, mu, B, scene_dev)
    b0, neighbours = I.SEAM_B64
    a = [x.reshape(B1, B1, B1) for x in host(mesher.integrate(b0))]
    for b, axis in neighbours:
        o = [x.reshape(B1, B1, B1) for x in host(mesher.integrate(b))]
        top, bottom = [np.s_[:]] * 3, [np.s_[:]] * 3
        top[2 - axis], bottom[2 - axis] = B, 0                       # arrays are [z][y][x]
        for u, v in zip(a, o):
            assert u[tuple(top)].tobytes() == v[tuple(bottom)].tobytes(), b
    assert (a[1] > 0).any() and (a[2] != 0).any()


# ---- B. integration at its thresholds -----------------------------------------------------------------------------------------
def threshold_mesher(views):
    return mesh.TsdfMesher(I.TH["origin"], I.TH["voxel"], I.TH["mu"], I.TH["B"], device_views(views))


def assert_integration_equals(got, recs, view_list, ref):
    """Bitwise on the EXACT samples of the list; elsewhere the rule of test_mesh_gpu.py (outside the tie margin: equal weights
    and colours, the tsdf within the header's bound)."""
    t, w, c = host(got)
    valid = [i for i in view_list if 0 <= i < len(recs)]
    exact = I.exact_samples(recs, valid)
    assert exact.sum() >= 3000
    bad = np.nonzero(exact & (w != ref["weight"]))[0]
    assert len(bad) == 0, (bad[:5], w[bad[:5]], ref["weight"][bad[:5]])
    bad = np.nonzero(exact & (c != ref["rgba"]))[0]
    assert len(bad) == 0, (bad[:5], c[bad[:5]], ref["rgba"][bad[:5]])
    bad = np.nonzero(exact & (t.view(np.uint32) != ref["tsdf"].view(np.uint32)))[0]
    assert len(bad) == 0, (bad[:5], t[bad[:5]], ref["tsdf"][bad[:5]])
    ok = ~ref["tie"] & ~exact
    assert np.array_equal(w[ok], ref["weight"][ok]) and np.array_equal(c[ok], ref["rgba"][ok])
    bound = M.tsdf_bound(I.TH["voxel"], I.TH["mu"], I.TH["B"], I.TH["b"], recs, valid, ref["weight"])
    err = np.abs(t.astype(np.float64) - ref["tsdf64"])
    assert (err[ok] <= bound[ok]).all(), (err[ok] - bound[ok]).max()
    return t, w, c


@pytest.fixture(scope="module")
def th_mesher():
    return threshold_mesher(I.threshold_views())


@pytest.mark.parametrize("view_list", [[0, 1], [0, 1, 2], [0], [1], [2]])
def test_thresholds_are_decided_as_the_restatement_decides_them(th_mesher, view_list):
    recs = I.threshold_records()
    ref = I.threshold_reference(view_list)
    t, w, c = assert_integration_equals(th_mesher.integrate(I.TH["b"], view_list), recs, view_list, ref)
    assert (w > 0).any() and (c != 0).any()


def test_view_list_order_and_empty_list(th_mesher):
    recs = I.threshold_records()
    fwd = assert_integration_equals(th_mesher.integrate(I.TH["b"], [0, 1]), recs, [0, 1], I.threshold_reference([0, 1]))
    rev = assert_integration_equals(th_mesher.integrate(I.TH["b"], [1, 0]), recs, [1, 0], I.threshold_reference([1, 0]))
    assert np.array_equal(fwd[1], rev[1]) and np.array_equal(fwd[2], rev[2])
    t, w, c = host(th_mesher.integrate(I.TH["b"], []))
    assert not t.view(np.uint32).any() and not w.any() and not c.any()


def test_three_hundred_views_and_indices_outside_the_view_set():
    views = I.many_views()
    n = len(views)
    mesher = threshold_mesher(views)
    recs = I.records(views, I.TH["origin"])
    every = list(range(n))
    ref = M.integrate(I.TH["voxel"], I.TH["mu"], I.TH["B"], I.TH["b"], recs, every)
    t, w, c = assert_integration_equals(mesher.integrate(I.TH["b"], every), recs, every, ref)
    assert w.max() == 300 == n
    # -1 and nviews among valid indices are skipped
    lst = [-1, 0, n, 1, -1, 2, n]
    want = M.integrate(I.TH["voxel"], I.TH["mu"], I.TH["B"], I.TH["b"], recs, [0, 1, 2])
    assert_integration_equals(mesher.integrate(I.TH["b"], lst), recs, lst, want)


# ---- C. extraction on crafted volumes -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def any_views():
    return device_views(I.threshold_views()[:1])


def extract_on_device(any_views, origin, voxel, B, b, vol, min_weight=1, vertex_base=0):
    # the mesher wants a view, which extraction never reads: the camera moves with the origin to stay within the extent
    views = [dict(v, C=np.asarray(origin) + v["C"]) for v in any_views]
    mesher = mesh.TsdfMesher(origin, voxel, 4.0 * voxel, B, views, min_weight=min_weight)
    return mesher.extract(b, upload(vol), vertex_base)


@pytest.mark.parametrize("B,tiny,min_weight", [(32, False, 1), (32, False, 2), (32, True, 1), (64, False, 1), (128, False, 1)])
def test_crafted_volume_far_from_the_origin(any_views, B, tiny, min_weight):
    vol = I.crafted_volume(B, tiny=tiny)
    key = (B, tiny, "far") if min_weight == 1 else None
    ref = I.extraction_reference(I.FAR_ORIGIN, 0.1, B, (0, 0, 0), vol, min_weight, key=key)
    assert len(ref["faces"]) > 0
    assert_mesh_equals(extract_on_device(any_views, I.FAR_ORIGIN, 0.1, B, (0, 0, 0), vol, min_weight), ref)


def test_last_brick_of_the_extent_and_the_top_of_uint32(any_views):
    B, b = 32, (511, 0, 3)
    vol = I.crafted_volume(B)
    ref = I.extraction_reference(I.FAR_ORIGIN, 1.0, B, b, vol, key=(B, "extent"))
    assert_mesh_equals(extract_on_device(any_views, I.FAR_ORIGIN, 1.0, B, b, vol), ref)
    nv = len(ref["xyz"])
    base = 0xFFFFFFFF - nv
    top = M.extract(I.FAR_ORIGIN, 1.0, B, b, *vol, 1, base)
    got = extract_on_device(any_views, I.FAR_ORIGIN, 1.0, B, b, vol, vertex_base=base)
    assert_mesh_equals(got, top)
    assert int(got[2].cpu().numpy().view(np.uint32).max()) == 0xFFFFFFFE
    with pytest.raises(_lib.AdaMVSHipError, match="vertices"):
        extract_on_device(any_views, I.FAR_ORIGIN, 1.0, B, b, vol, vertex_base=base + 1)


def test_empty_and_single_cube_volumes(any_views):
    B = 32
    t, w, c = I.crafted_volume(B)
    for vol in ((np.abs(t) + np.float32(0.0), w, c), (t, np.zeros_like(w), c)):
        xyz, rgb, faces = extract_on_device(any_views, I.FAR_ORIGIN, 0.1, B, (0, 0, 0), vol)
        assert xyz.shape == (0, 3) and rgb.shape == (0, 3) and faces.shape == (0, 3)
    for cube in ((0, 0, 0), (B - 1, B - 1, B - 1)):
        vol = I.single_cube_volume(B, cube)
        ref = M.extract(I.FAR_ORIGIN, 0.1, B, (0, 0, 0), *vol)
        assert len(ref["faces"]) >= 6
        assert_mesh_equals(extract_on_device(any_views, I.FAR_ORIGIN, 0.1, B, (0, 0, 0), vol), ref)


# ---- D. the raw calls: intermediates and capacities ---------------------------------------------------------------------------
PATTERN = 0xA5


def test_intermediate_arrays_and_capacities():
    import torch
    from ada_mvs_amd import hip_ops
    B, TILE = 32, _lib.MESH_TILE
    S, nbs, nbc = (B + 1) ** 3, ((B + 1) ** 3 + TILE - 1) // TILE, B ** 3 // TILE
    vol = I.crafted_volume(B)
    ref = I.extraction_reference(I.FAR_ORIGIN, 0.1, B, (0, 0, 0), vol, key=(B, False, "far"))
    tsdf, weight, rgba = upload(vol)
    brick = hip_ops.mesh_brick(I.FAR_ORIGIN, 0.1, 0.4, B, (0, 0, 0), 1)
    lib = _lib.load()
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = dict(device="cuda", dtype=torch.int32)
    code, mask = torch.full((B ** 3,), -1, **i32), torch.full((S,), PATTERN, device="cuda", dtype=torch.uint8)
    block_tris, block_verts = torch.full((nbc,), -1, **i32), torch.full((nbs,), -1, **i32)
    tri_off, vert_off = torch.full((nbc + 1,), -1, **i32), torch.full((nbs + 1,), -1, **i32)
    _lib.check(lib.adamvs_mesh_classify(ctypes.byref(brick), p(tsdf), p(weight), p(code), p(block_tris), st), "mesh_classify")
    _lib.check(lib.adamvs_mesh_count_vertices(ctypes.byref(brick), p(tsdf), p(code), p(mask), p(block_verts), st), "mesh_count_vertices")
    _lib.check(lib.adamvs_fusion_scan(p(block_tris), p(tri_off), nbc, st), "fusion_scan")
    _lib.check(lib.adamvs_fusion_scan(p(block_verts), p(vert_off), nbs, st), "fusion_scan")
    u32 = lambda x: x.cpu().numpy().view(np.uint32)  # noqa: E731

    # cube_code: the processed bit, the six cases (0 for a cube not processed), the triangle count
    cases = M.cube_cases(B, vol[0]) * ref["processed"][:, None]
    ntri = M.case_triangle_count(cases).sum(1) * ref["processed"]
    want = ref["processed"].astype(np.int64) | (ntri << 25)
    for t in range(6):
        want |= cases[:, t] << (1 + 4 * t)
    got = u32(code)
    assert np.array_equal(got & 1, ref["processed"])
    assert np.array_equal((got >> 25) & 15, ntri) and (got >> 29 == 0).all()
    assert np.array_equal(got, want.astype(np.uint32))
    assert np.array_equal(mask.cpu().numpy(), ref["edge_mask"])
    counts = M._popcount(ref["edge_mask"])
    per_tile = lambda v, nb: np.concatenate([v, np.zeros(nb * TILE - len(v), np.int64)]).reshape(nb, TILE).sum(1)  # noqa: E731
    bt, bv = per_tile(ntri, nbc), per_tile(counts, nbs)
    assert np.array_equal(u32(block_tris), bt) and np.array_equal(u32(block_verts), bv)
    assert np.array_equal(u32(tri_off), np.concatenate([[0], np.cumsum(bt)])) and np.array_equal(u32(vert_off), np.concatenate([[0], np.cumsum(bv)]))
    nv, nt = int(bv.sum()), int(bt.sum())
    assert nv == len(ref["xyz"]) and nt == len(ref["faces"])

    # emit: buffers with a tail, filled with a pattern; whatever the capacity, every store lands in allocated memory
    TAIL = 64

    def emit(vcap, tcap):
        xyz = torch.full(((nv + TAIL) * 24,), PATTERN, device="cuda", dtype=torch.uint8)
        rgb = torch.full(((nv + TAIL) * 3,), PATTERN, device="cuda", dtype=torch.uint8)
        faces = torch.full(((nt + TAIL) * 12,), PATTERN, device="cuda", dtype=torch.uint8)
        first = torch.full((S,), -1, **i32)
        _lib.check(lib.adamvs_mesh_emit(ctypes.byref(brick), p(tsdf), p(rgba), p(code), p(mask), p(vert_off), p(tri_off), 7, p(xyz), p(rgb),
                                        p(first), vcap, p(faces), tcap, st), "mesh_emit")
        return xyz, rgb, faces, first

    full = emit(nv, nt)
    want_first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    assert np.array_equal(u32(full[3]), want_first)
    assert full[0][:nv * 24].cpu().numpy().tobytes() == ref["xyz"].tobytes()
    assert np.array_equal(full[1][:nv * 3].cpu().numpy().reshape(-1, 3), ref["rgb"])
    assert np.array_equal(full[2][:nt * 12].cpu().numpy().view(np.uint32).reshape(-1, 3), ref["faces"] + np.uint32(7))
    for vcap, tcap in itertools.product((nv, nv // 2, 1, 0), (nt, nt // 3, 1, 0)):
        got = full if (vcap, tcap) == (nv, nt) else emit(vcap, tcap)
        for buf, whole, rows, cap in ((got[0], full[0], 24, vcap), (got[1], full[1], 3, vcap), (got[2], full[2], 12, tcap)):
            assert torch.equal(buf[:cap * rows], whole[:cap * rows]), (vcap, tcap, rows)
            assert bool((buf[cap * rows:] == PATTERN).all()), (vcap, tcap, rows)
        assert torch.equal(got[3], full[3])
    torch.cuda.synchronize()
