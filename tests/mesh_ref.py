"""numpy restatement of include/adamvs_hip.h "TSDF mesh": integration in fp64 of the fp32 inputs (K, R_cw, c = C - O, the voxel
and mu rounded to fp32), extraction op for op (lambda and the colours in fp32, positions in fp64).  The tet table is derived
here geometrically from the header's rule, not copied from csrc/mesh.hip."""
import itertools

import numpy as np

PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
DIRS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)])
EPS32 = 2.0 ** -24


def tet_vertices(t):
    a, b, _ = PERMS[t]
    v = np.zeros((4, 3), np.int64)
    v[1, a] = 1
    v[2, a] = v[2, b] = 1
    v[3] = 1
    return v


def dir_index(d):
    return int(np.nonzero((DIRS == np.asarray(d)).all(1))[0][0])


def case_triangles(t, case):
    """Triangles of tet t in sign case `case` (bit k: vertex k inside) as lists of three tet-vertex pairs (i, j), i < j, oriented
    so that the normal at the edge midpoints points along centroid(outside) - centroid(inside)."""
    v = tet_vertices(t).astype(np.float64)
    inside = [k for k in range(4) if (case >> k) & 1]
    outside = [k for k in range(4) if not (case >> k) & 1]
    e = lambda i, j: (min(i, j), max(i, j))  # noqa: E731
    if len(inside) in (1, 3):
        lone = inside[0] if len(inside) == 1 else outside[0]
        tris = [[e(lone, k) for k in range(4) if k != lone]]
    elif len(inside) == 2:
        (i, j), (k, l) = inside, outside
        q = [e(i, k), e(i, l), e(j, l), e(j, k)]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    else:
        return []
    D = v[outside].mean(0) - v[inside].mean(0)
    out = []
    for tri in tris:
        P = [(v[i] + v[j]) / 2 for i, j in tri]
        n = np.cross(P[1] - P[0], P[2] - P[0])
        out.append(tri if n @ D > 0 else [tri[0], tri[2], tri[1]])
    return out


def tet_edges(t):
    """-> {(i, j): (start corner offset (3,), direction index)} of the six edges of tet t."""
    v = tet_vertices(t)
    return {(i, j): (v[i], dir_index(v[j] - v[i])) for i, j in itertools.combinations(range(4), 2)}


# ---- integration ------------------------------------------------------------------------------------------------------------
def view_record(K, R_wc, C, origin, depth, rgba):
    """The fp32 inputs of one view as adamvs_mesh_view holds them (c = C - O formed in fp64, rounded)."""
    return dict(K=np.asarray(K, np.float32), R=np.asarray(R_wc, np.float64).T.astype(np.float32),
                c=(np.asarray(C, np.float64) - np.asarray(origin, np.float64)).astype(np.float32), depth=np.asarray(depth, np.float32),
                rgba=np.asarray(rgba, np.uint8))


def sample_grid(B, b):
    """-> g [(B+1)^3, 3] int64 in sample row-major order (x fastest) of brick b."""
    r = np.arange(B + 1)
    z, y, x = np.meshgrid(r, r, r, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1) + np.asarray(b, np.int64) * B


def pixel_margin(H, W, floor=1e-4):
    return max(floor, 8.0 * float(np.spacing(np.float32(max(H, W)))))


def project(voxel, B, b, V):
    """-> (z, u, v) fp64 [(B+1)^3] of brick b's samples in view record V: x = g sf - c, p = R_cw x, z = p.z, (u, v) = (K p).xy / z
    (inf or NaN where z = 0)."""
    K, R, c = V["K"].astype(np.float64), V["R"].astype(np.float64), V["c"].astype(np.float64)
    p = (sample_grid(B, b).astype(np.float64) * float(np.float32(voxel)) - c) @ R.T
    z = p[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (K[0, 0] * p[:, 0] + K[0, 1] * p[:, 1] + K[0, 2] * z) / z
        v = (K[1, 0] * p[:, 0] + K[1, 1] * p[:, 1] + K[1, 2] * z) / z
    return z, u, v


def integrate(voxel, mu, B, b, views, view_list):
    """-> dict(tsdf fp32, weight uint16, rgba uint32, tie bool): the samples of brick b, views[i] for i in view_list, in order.
    tie: some view's decision lies within the header's error bound of a threshold (the fp32 kernel may decide it either way)."""
    sf, muf = float(np.float32(voxel)), float(np.float32(mu))
    g = sample_grid(B, b)
    gs = g.astype(np.float64) * sf
    n = len(g)
    T = np.zeros(n)
    w = np.zeros(n, np.int64)
    csum = np.zeros((n, 3), np.int64)
    nc = np.zeros(n, np.int64)
    tie = np.zeros(n, bool)
    for vi in view_list:
        V = views[vi]
        K, R, c = V["K"].astype(np.float64), V["R"].astype(np.float64), V["c"].astype(np.float64)
        H, W = V["depth"].shape
        z, u, v = project(voxel, B, b, V)
        L = np.linalg.norm(gs, axis=1) + np.linalg.norm(c)
        dz = 16 * EPS32 * L
        front = z > 0
        tie |= np.abs(z) <= dz
        zz = np.where(front, z, 1.0)
        mpx = pixel_margin(H, W) + 4.0 * (abs(K[0, 0]) + abs(K[1, 1]) + abs(K[0, 1])) * dz / zz + 8 * EPS32 * (np.abs(u) + np.abs(v) + 1)
        fu, fv = np.floor(u + 0.5), np.floor(v + 0.5)
        for q, fq in ((u, fu), (v, fv)):
            with np.errstate(invalid="ignore"):                            # z = 0: inf - inf, behind `front`
                frac = (q + 0.5) - fq
            tie |= front & ((frac < mpx) | (1.0 - frac < mpx))
        ok = front & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        iu, iv = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
        d = V["depth"][iv, iu].astype(np.float64)
        ok &= np.isfinite(d) & (d > 0)
        sdf = d - z
        tie |= ok & ((np.abs(sdf + muf) <= 2 * dz) | (np.abs(np.abs(sdf) - muf) <= 2 * dz))
        ok &= sdf >= -muf
        T += np.where(ok, np.minimum(1.0, sdf / muf), 0.0)
        w += ok
        col = ok & (np.abs(sdf) <= muf)
        rgb = V["rgba"][iv, iu, :3].astype(np.int64)
        csum += np.where(col[:, None], rgb, 0)
        nc += col
    with np.errstate(divide="ignore", invalid="ignore"):
        tsdf = np.where(w > 0, T / np.maximum(w, 1), 0.0).astype(np.float32)
    h = nc // 2
    ch = [(csum[:, k] + h) // np.maximum(nc, 1) for k in range(3)]
    rgba = np.where(nc > 0, ch[0] | (ch[1] << 8) | (ch[2] << 16) | (255 << 24), 0).astype(np.uint32)
    return dict(tsdf=tsdf, weight=np.minimum(w, 65535).astype(np.uint16), rgba=rgba, tie=tie, tsdf64=np.where(w > 0, T / np.maximum(w, 1), 0.0))


def tsdf_bound(voxel, mu, B, b, views, view_list, weight):
    """The header's bound on |tsdf - tsdf_fp64| per sample."""
    gs = sample_grid(B, b).astype(np.float64) * float(np.float32(voxel))
    cmax = max([np.linalg.norm(views[i]["c"].astype(np.float64)) for i in view_list] + [0.0])
    L = np.linalg.norm(gs, axis=1) + cmax
    return 16 * EPS32 * L / float(np.float32(mu)) + EPS32 * (weight.astype(np.float64) + 2)


# ---- extraction ---------------------------------------------------------------------------------------------------------------
def extract(origin, voxel, B, b, tsdf, weight, rgba, min_weight=1, vertex_base=0):
    """-> dict(xyz [nv, 3] fp64, rgb [nv, 3] uint8, faces [nt, 3] uint32, edge_mask [(B+1)^3] uint8, processed [B^3] bool)."""
    B1 = B + 1
    t3 = np.asarray(tsdf, np.float32).reshape(B1, B1, B1)           # [z][y][x]
    w3 = np.asarray(weight).astype(np.int64).reshape(B1, B1, B1)
    inside = t3 < 0

    def corner(arr, off):
        ox, oy, oz = off
        return arr[oz:oz + B, oy:oy + B, ox:ox + B]

    offs = [(k & 1, (k >> 1) & 1, (k >> 2) & 1) for k in range(8)]
    processed = np.ones((B, B, B), bool)
    for o in offs:
        processed &= corner(w3, o) >= min_weight
    # edge masks: sign change and a processed cube of the brick using the edge
    users = {e: set() for e in range(7)}
    for t in range(6):
        for start, e in tet_edges(t).values():
            users[e].add(tuple(start))
    mask = np.zeros((B1, B1, B1), np.uint8)
    cmask = np.zeros((B1, B1, B1), np.uint8)                             # sign changes alone, used or not
    pp = np.zeros((B + 2, B + 2, B + 2), bool)                           # processed, padded by one on both sides
    pp[1:B + 1, 1:B + 1, 1:B + 1] = processed
    for e in range(7):
        dx, dy, dz = DIRS[e]
        other = np.full((B1, B1, B1), False)
        valid = np.zeros((B1, B1, B1), bool)
        valid[:B1 - dz, :B1 - dy, :B1 - dx] = True
        other[:B1 - dz, :B1 - dy, :B1 - dx] = inside[dz:, dy:, dx:]
        change = valid & (other != inside)
        used = np.zeros((B1, B1, B1), bool)
        for sx, sy, sz in users[e]:
            # cube of sample l is l - s: padded index l - s + 1
            used |= pp[1 - sz:1 - sz + B1, 1 - sy:1 - sy + B1, 1 - sx:1 - sx + B1]
        mask |= ((change & used).astype(np.uint8) << e)
        cmask |= (change.astype(np.uint8) << e)
    flat_mask = mask.ravel()
    bits = (flat_mask[:, None] >> np.arange(7)) & 1
    counts = bits.sum(1)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    n_idx, e_idx = np.nonzero(bits)                                      # sample row-major, then direction
    g = sample_grid(B, b)
    tf = t3.ravel()
    m_idx = n_idx + DIRS[e_idx, 0] + DIRS[e_idx, 1] * B1 + DIRS[e_idx, 2] * B1 * B1
    ta, tb = tf[n_idx], tf[m_idx]
    lam = (ta / (ta - tb)).astype(np.float32)
    xyz = np.empty((len(n_idx), 3))
    O = np.asarray(origin, np.float64)
    for ax in range(3):
        gg = g[n_idx, ax].astype(np.float64)
        gg = np.where(DIRS[e_idx, ax] == 1, gg + lam.astype(np.float64), gg)
        xyz[:, ax] = O[ax] + gg * float(voxel)
    ca, cb = np.asarray(rgba, np.uint32)[n_idx], np.asarray(rgba, np.uint32)[m_idx]
    rgb = np.empty((len(n_idx), 3), np.uint8)
    for ch in range(3):
        fa = ((ca >> (8 * ch)) & 255).astype(np.float32)
        fb = ((cb >> (8 * ch)) & 255).astype(np.float32)
        c = np.rint(fa + lam * (fb - fa)).astype(np.float32)
        rgb[:, ch] = np.clip(c, 0, 255).astype(np.uint8)
    # triangles: cube row-major, then tet, then table order
    cubes = np.nonzero(processed.ravel())[0]
    cz, cy, cx = cubes // (B * B), (cubes // B) % B, cubes % B
    cases = cube_cases(B, tsdf)[cubes]
    per_tet = []
    for t in range(6):
        case = cases[:, t]
        edges = tet_edges(t)
        idx = {}
        for (i, j), (s, e) in edges.items():
            sn = ((cz + s[2]) * B1 + cy + s[1]) * B1 + cx + s[0]
            idx[(i, j)] = first[sn] + _popcount(flat_mask[sn].astype(np.int64) & ((1 << e) - 1))
        tris = np.full((len(cubes), 2, 3), -1, np.int64)
        for c in range(16):
            sel = case == c
            for r, tri in enumerate(case_triangles(t, c)):
                for m, pair in enumerate(tri):
                    tris[sel, r, m] = idx[pair][sel]
        per_tet.append(tris)
    allt = np.stack(per_tet, 1).reshape(-1, 3)                          # [cube][tet][r]
    faces = (allt[allt[:, 0] >= 0] + vertex_base).astype(np.uint32)
    return dict(xyz=xyz, rgb=rgb, faces=faces, edge_mask=flat_mask, processed=processed.ravel(), sign_change=cmask.ravel())


def cube_cases(B, tsdf):
    """-> [B^3, 6] int64: the sign case of tet t of every cube, cube row-major (sum over k of inside(v_k) << k, inside iff tsdf < 0)."""
    B1 = B + 1
    ins = (np.asarray(tsdf, np.float32) < 0).reshape(B1, B1, B1)
    out = np.zeros((B, B, B, 6), np.int64)
    for t in range(6):
        v = tet_vertices(t)
        for k in range(4):
            out[..., t] |= ins[v[k, 2]:v[k, 2] + B, v[k, 1]:v[k, 1] + B, v[k, 0]:v[k, 0] + B].astype(np.int64) << k
    return out.reshape(-1, 6)


def case_triangle_count(case):
    """Triangles of a sign case (the same for every tet), elementwise."""
    nin = _popcount(case)
    return np.where((nin == 0) | (nin == 4), 0, np.where(nin == 2, 2, 1))


def _popcount(x):
    x = np.asarray(x, np.int64)
    return sum(((x >> k) & 1) for k in range(8))


# ---- mesh checks --------------------------------------------------------------------------------------------------------------
def weld(xyz, faces):
    """Exact-position weld: -> (xyz unique rows, faces remapped)."""
    u, inv = np.unique(np.asarray(xyz), axis=0, return_inverse=True)
    return u, inv.reshape(-1)[np.asarray(faces, np.int64)]


def closed_and_oriented(faces):
    """-> (every undirected edge in exactly two faces and every directed edge in one, Euler characteristic V - E + F)."""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = np.sort(d, 1)
    _, cu = np.unique(und, axis=0, return_counts=True)
    _, cd = np.unique(d, axis=0, return_counts=True)
    V = len(np.unique(f))
    return bool((cu == 2).all() and (cd == 1).all()), V - len(cu) + len(f)


def signed_volume(xyz, faces):
    p = np.asarray(xyz)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def sphere_volume(B, centre, radius, mu, nb=2):
    """An analytic tsdf clip((|g - centre| - r) / mu, -1, 1) (voxel units, fp32) over nb^3 bricks: {brick: (tsdf, weight, rgba)}."""
    out = {}
    for b in itertools.product(range(nb), repeat=3):
        g = sample_grid(B, b).astype(np.float64)
        dist = np.linalg.norm(g - np.asarray(centre), axis=1)
        t = np.clip((dist - radius) / mu, -1.0, 1.0).astype(np.float32)
        col = (np.clip(g[:, 0] * 3, 0, 255).astype(np.uint32) | (np.clip(g[:, 1] * 3, 0, 255).astype(np.uint32) << 8)
               | (np.uint32(200) << 16) | (np.uint32(255) << 24))
        out[b] = (t, np.ones(len(g), np.uint16), col.astype(np.uint32))
    return out
