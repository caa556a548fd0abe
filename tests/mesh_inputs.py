"""Inputs of the TSDF-mesh tests, numpy only: the analytic scene at the brick sizes 64 and 128 with its restatement, a scene whose
integration is exact in fp32 (every threshold of the header is hit exactly, on samples where the kernel and the restatement must
agree bit for bit), and crafted volumes for the extraction (every tet case, scattered unprocessed cubes, signed zeros, subnormal
values, single cubes in the brick's first and last corner)."""
import numpy as np

from ada_mvs_amd import fusion_synth, mesh
import mesh_ref as M

# ---- A. the analytic scene at B = 64 and 128, voxel not 1 -------------------------------------------------------------------
SCENE_ORIGIN = np.array([-112.0, -112.0, -8.0])
# (B, voxel, mu, brick, the min_weights extracted)
SCENE_CASES = [(64, 0.5, 2.0, (2, 4, 0), (1,)), (64, 0.5, 2.0, (4, 2, 0), (1,)), (128, 0.3, 1.2, (2, 2, 0), (1, 3))]
SEAM_B64 = ((2, 4, 0), (((3, 4, 0), 0), ((2, 5, 0), 1), ((2, 4, 1), 2)))            # a brick and its upper neighbour along each axis

_cache = {}


def scene_host():
    """The views of fusion_synth.scene(192, 256, 4, seed=5) on the host -> [dict(K, R, C, depth_h, rgba_h)]."""
    if "scene" not in _cache:
        sc = fusion_synth.scene(192, 256, 4, seed=5)
        _cache["scene"] = [dict(K=c["K"], R=c["R"], C=c["C"], depth_h=d, rgba_h=fusion_synth.texture(c, d.astype(np.float64)))
                           for c, d in zip(sc["cams"], sc["depths"])]
    return _cache["scene"]


def records(views, origin):
    return [M.view_record(v["K"], v["R"], v["C"], origin, v["depth_h"], v["rgba_h"]) for v in views]


def host_view_list(views, origin, voxel, mu, B, b):
    """mesh.TsdfMesher.view_list without a device."""
    cams = [(np.asarray(v["K"], np.float64), np.asarray(v["R"], np.float64), np.asarray(v["C"], np.float64)) + tuple(v["depth_h"].shape)
            for v in views]
    return mesh.cull_views(*mesh.brick_box(np.asarray(origin, np.float64), voxel, B, b, mu), cams)


def scene_reference(B, voxel, mu, b):
    """-> dict(vl, recs, ref, bound) of one brick of the analytic scene, computed once per process."""
    key = ("ref", B, voxel, mu, b)
    if key not in _cache:
        views = scene_host()
        vl = host_view_list(views, SCENE_ORIGIN, voxel, mu, B, b)
        recs = records(views, SCENE_ORIGIN)
        ref = M.integrate(voxel, mu, B, b, recs, vl)
        _cache[key] = dict(vl=vl, recs=recs, ref=ref, bound=M.tsdf_bound(voxel, mu, B, b, recs, vl, ref["weight"]))
    return _cache[key]


# ---- B. integration at its thresholds ---------------------------------------------------------------------------------------
# B = 32, O = 0, voxel 1, mu 4, brick (0, 0, 0).  Every camera is axis-aligned at integer coordinates, K holds small integers and
# the depths are multiples of 1/4: wherever z is a power of two (or <= 0) in every view, K p, the division by z, d - z, sdf / mu
# and the running sum are exact in fp32 and in fp64 alike, and T / w is one correctly rounded division.
TH = dict(B=32, origin=(0.0, 0.0, 0.0), voxel=1.0, mu=4.0, b=(0, 0, 0))
NADIR_R_CW = np.diag([1.0, -1.0, -1.0])                                   # z = 33 - g.z
SIDE_R_CW = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])  # z = g.x - 10
BAD_DEPTHS = (("nan", np.float32(np.nan)), ("+inf", np.float32(np.inf)), ("-inf", np.float32(-np.inf)), ("zero", np.float32(0.0)),
              ("negative", np.float32(-3.0)), ("flt_max", np.finfo(np.float32).max), ("subnormal", np.float32(1e-45)))
# pixels (row, column) that EXACT samples look at: the bad depths in BAD_DEPTHS' order, and planted offsets k (depth = base + k / 4)
# that put sdf at -mu, just below it, at +mu and just above it
NADIR_BAD = ((7, 0), (7, 2), (7, 3), (7, 4), (7, 6), (7, 10), (6, 1))
SIDE_BAD = ((3, 4), (3, 5), (3, 6), (3, 7), (3, 8), (3, 9), (2, 5))
NADIR_PLANTED = {(5, 2): 0, (5, 3): 1}                                     # z = 16: sdf = +mu, +mu + 1/4
SIDE_PLANTED = {(4, 1): 0, (4, 2): -1, (3, 1): 0, (3, 2): 1}               # z = 16: -mu, -mu - 1/4;  z = 8: +mu, +mu + 1/4
WIDE_PLANTED = {(10, 12): 0, (10, 13): 1}                                  # z = 16: +mu, +mu + 1/4


def _depth_map(rng, H, W, base, bad, planted):
    k = rng.integers(-24, 25, (H, W))
    for (r, c), kk in planted.items():
        k[r, c] = kk
    d = (base + k / 4.0).astype(np.float32)
    for (r, c), (_, val) in zip(bad, BAD_DEPTHS):
        d[r, c] = val
    return d


def threshold_views():
    """-> [nadir, side, wide nadir] as dict(K, R (R_wc), C, depth_h, rgba_h).  The wide nadir view (f = 2 on 20 x 24) sees most
    of the brick, so that most EXACT samples carry weight."""
    if "th" not in _cache:
        rng = np.random.default_rng(11)
        K8 = np.array([[8.0, 0.0, 5.0], [0.0, 8.0, 4.0], [0.0, 0.0, 1.0]])
        K2 = np.array([[2.0, 0.0, 12.0], [0.0, 2.0, 10.0], [0.0, 0.0, 1.0]])
        specs = ((K8, NADIR_R_CW, (16.0, 16.0, 33.0), 10, 12, 20.0, NADIR_BAD, NADIR_PLANTED),
                 (K8, SIDE_R_CW, (10.0, 16.0, 16.0), 10, 12, 12.0, SIDE_BAD, SIDE_PLANTED),
                 (K2, NADIR_R_CW, (16.0, 16.0, 33.0), 20, 24, 20.0, (), WIDE_PLANTED))
        views = []
        for K, R_cw, C, H, W, base, bad, planted in specs:
            views.append(dict(K=K, R=R_cw.T.copy(), C=np.array(C), depth_h=_depth_map(rng, H, W, base, bad, planted),
                              rgba_h=rng.integers(0, 256, (H, W, 4)).astype(np.uint8)))
        _cache["th"] = views
    return _cache["th"]


def threshold_records(views=None):
    return records(threshold_views() if views is None else views, TH["origin"])


def threshold_reference(view_list, views=None):
    return M.integrate(TH["voxel"], TH["mu"], TH["B"], TH["b"], threshold_records(views), list(view_list))


def exact_samples(recs, view_list):
    """EXACT: in every listed view z <= 0 or z is a power of two."""
    ok = np.ones((TH["B"] + 1) ** 3, bool)
    for vi in view_list:
        z, _, _ = M.project(TH["voxel"], TH["B"], TH["b"], recs[vi])
        m, _ = np.frexp(np.where(z > 0, z, 1.0))
        ok &= (z <= 0) | (m == 0.5)
    return ok


def threshold_events(recs, view_list):
    """-> {event: bool [(B+1)^3]}: the samples at which some listed view meets the event, from the restatement's own terms."""
    n = (TH["B"] + 1) ** 3
    mu = TH["mu"]
    names = ["z == 0", "u + 0.5 an integer", "u == -0.5", "u == size - 0.5", "sdf == -mu", "sdf == +mu", "sdf == -mu - 1/4",
             "sdf == +mu + 1/4"] + ["depth " + name for name, _ in BAD_DEPTHS]
    ev = {k: np.zeros(n, bool) for k in names}
    for vi in view_list:
        V = recs[vi]
        H, W = V["depth"].shape
        z, u, v = M.project(TH["voxel"], TH["B"], TH["b"], V)
        front = z > 0
        ev["z == 0"] |= z == 0
        fu, fv = np.floor(u + 0.5), np.floor(v + 0.5)
        ev["u + 0.5 an integer"] |= front & ((u + 0.5 == fu) | (v + 0.5 == fv))
        ev["u == -0.5"] |= front & ((u == -0.5) | (v == -0.5))
        ev["u == size - 0.5"] |= front & ((u == W - 0.5) | (v == H - 0.5))
        inside = front & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        iu, iv = np.where(inside, fu, 0).astype(np.int64), np.where(inside, fv, 0).astype(np.int64)
        d = V["depth"][iv, iu]
        for name, val in BAD_DEPTHS:
            ev["depth " + name] |= inside & ((d == val) | (np.isnan(val) & np.isnan(d)))
        with np.errstate(invalid="ignore"):
            good = inside & np.isfinite(d) & (d > 0)
            sdf = d.astype(np.float64) - z
        ev["sdf == -mu"] |= good & (sdf == -mu)
        ev["sdf == +mu"] |= good & (sdf == mu)
        ev["sdf == -mu - 1/4"] |= good & (sdf == -mu - 0.25)
        ev["sdf == +mu + 1/4"] |= good & (sdf == mu + 0.25)
    return ev


def many_views(n=300):
    """n views that share the nadir and the side view's maps, alternating."""
    v = threshold_views()
    return [v[i % 2] for i in range(n)]


# ---- C. crafted volumes for the extraction ----------------------------------------------------------------------------------
CONSTANTS = (-1.0, -0.5, -0.0, 0.0, 0.25, 1.0)
TINY = (1e-45, -1e-45, 1e-40, -1e-40)                                      # subnormal in fp32: below 2^-126
FAR_ORIGIN = (500000.3, 3399999.3, 12.1)


def crafted_volume(B, seed=0, tiny=False):
    """-> (tsdf fp32, weight uint16, rgba uint32) [(B+1)^3]: half the samples one of CONSTANTS (and of TINY), half uniform in
    [-1, 1]; weights from {0, 1, 1, 1, 2, 2}, so that (5/6)^8 = 23 % of the cubes are processed at min_weight 1 and the others lie
    scattered among them; random colours."""
    key = ("vol", B, seed, tiny)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        n = (B + 1) ** 3
        consts = np.array(CONSTANTS + (TINY if tiny else ()), np.float32)
        t = np.where(rng.random(n) < 0.5, consts[rng.integers(0, len(consts), n)], rng.uniform(-1.0, 1.0, n).astype(np.float32))
        w = np.array([0, 1, 1, 1, 2, 2], np.uint16)[rng.integers(0, 6, n)]
        c = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        _cache[key] = (t.astype(np.float32), w, c)
    return _cache[key]


def single_cube_volume(B, cube, seed=0):
    """crafted_volume with weight 1 on the 8 corners of `cube` and 0 elsewhere; the cube's main diagonal changes sign, so that all
    six of its tets give triangles."""
    t, w, c = crafted_volume(B, seed)
    t, w = t.copy(), np.zeros_like(w)
    B1 = B + 1
    n0 = (cube[2] * B1 + cube[1]) * B1 + cube[0]
    for k in range(8):
        w[n0 + (k & 1) + ((k >> 1) & 1) * B1 + ((k >> 2) & 1) * B1 * B1] = 1
    t[n0], t[n0 + 1 + B1 + B1 * B1] = -0.5, 0.25
    return t, w, c


def extraction_reference(origin, voxel, B, b, vol, min_weight=1, vertex_base=0, key=None):
    """M.extract, computed once per process where a key is given."""
    if key is None:
        return M.extract(origin, voxel, B, b, *vol, min_weight, vertex_base)
    key = ("ext",) + tuple(key)
    if key not in _cache:
        _cache[key] = M.extract(origin, voxel, B, b, *vol, min_weight, vertex_base)
    return _cache[key]


def used_by_none(B, ref):
    """Per direction e: the sample edges with a sign change that no processed cube uses (bit e of sign_change set, of edge_mask not)."""
    return ref["sign_change"] & ~ref["edge_mask"]
