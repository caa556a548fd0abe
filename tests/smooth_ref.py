"""numpy restatement of include/adamvs_hip.h "Mesh smoothing": the five steps in fp64, written from the header's rule and sharing no
code with csrc/mesh_smooth.hip.  N(f) and F(v) are built face by face in Python and then padded to matrices, so that every sum
runs column by column in the header's order.  Besides the result it returns every intermediate the GPU tests compare."""
import numpy as np


def weld(xyz, rgb, faces):
    """Exact-position weld as ada_mvs_amd.mesh.weld does it (coincident vertices carry the same colour)."""
    u, inv = np.unique(np.asarray(xyz, np.float64), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    col = np.empty((len(u), 3), np.uint8)
    col[inv] = np.asarray(rgb, np.uint8)
    return u, col, inv[np.asarray(faces).astype(np.int64)]


def face_records(p, faces):
    """Step 1 -> (n [nf, 3], A [nf], c [nf, 3])."""
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    u, w = b - a, c - a
    m = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    ln = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where(ln[:, None] > 0, m / ln[:, None], 0.0)
    return n, ln / 2.0, centroids(p, faces)


def centroids(p, faces):
    return ((p[faces[:, 0]] + p[faces[:, 1]]) + p[faces[:, 2]]) / 3.0


def incidence(faces, nv):
    """Step 2 -> (F: list per vertex of its faces ascending, each once; N: list per face, f first, then corner by corner)."""
    F = [[] for _ in range(nv)]
    for f, tri in enumerate(faces.tolist()):
        for k, v in enumerate(tri):
            if v not in tri[:k]:
                F[v].append(f)
    N = []
    for f, tri in enumerate(faces.tolist()):
        row, seen = [f], {f}
        for k, v in enumerate(tri):
            if v in tri[:k]:
                continue
            for g in F[v]:
                if g not in seen:
                    seen.add(g)
                    row.append(g)
        N.append(row)
    return F, N


def padded(rows):
    """Lists of unequal length -> (index matrix [n, width] with 0 where absent, mask)."""
    width = max([len(r) for r in rows] + [1])
    idx = np.zeros((len(rows), width), np.int64)
    mask = np.zeros((len(rows), width), bool)
    for i, r in enumerate(rows):
        idx[i, :len(r)] = r
        mask[i, :len(r)] = True
    return idx, mask


def filter_normals(n, A, c, Nidx, Nmask, sigma_s, sigma_r, iters):
    """Step 3: `iters` double-buffered passes -> n [nf, 3]."""
    ds, dr = 2.0 * sigma_s * sigma_s, 2.0 * sigma_r * sigma_r
    for _ in range(iters):
        s = np.zeros_like(n)
        for j in range(Nidx.shape[1]):
            g, on = Nidx[:, j], Nmask[:, j]
            dc, dn = c - c[g], n - n[g]
            dc2 = (dc[:, 0] * dc[:, 0] + dc[:, 1] * dc[:, 1]) + dc[:, 2] * dc[:, 2]
            dn2 = (dn[:, 0] * dn[:, 0] + dn[:, 1] * dn[:, 1]) + dn[:, 2] * dn[:, 2]
            w = A[g] * np.exp(-(dc2 / ds + dn2 / dr))
            s = np.where(on[:, None], s + w[:, None] * n[g], s)
        ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.where(ln[:, None] > 1e-12, s / ln[:, None], n)
    return n


def boundary_vertices(faces, nv):
    """Step 4 -> fixed [nv] bool: the ends of every edge that exactly one face corner pair uses."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = np.sort(e, 1)
    fixed = np.zeros(nv, bool)
    if len(e):
        u, cnt = np.unique(e, axis=0, return_counts=True)
        fixed[u[cnt == 1].ravel()] = True
    return fixed


def update_vertices(p0, faces, n, Fidx, Fmask, fixed, cap, iters):
    """Step 5: `iters` Jacobi passes -> (p [nv, 3], clamped [nv] bool of the last pass)."""
    count = Fmask.sum(1)
    still = fixed | (count == 0)
    p = p0.copy()
    clamped = np.zeros(len(p0), bool)
    for _ in range(iters):
        c = centroids(p, faces)
        s = np.zeros_like(p)
        for j in range(Fidx.shape[1]):
            f, on = Fidx[:, j], Fmask[:, j]
            e = c[f] - p
            t = (n[f, 0] * e[:, 0] + n[f, 1] * e[:, 1]) + n[f, 2] * e[:, 2]
            s = np.where(on[:, None], s + n[f] * t[:, None], s)
        x = p + s / np.maximum(count, 1)[:, None]
        d = x - p0
        ld = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        clamped = (ld > cap) & ~still
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(ld > cap, cap / ld, 1.0)
        p = np.where(still[:, None], p0, p0 + d * t[:, None])
    return p, clamped


def smooth(xyz, rgb, faces, sigma_s, sigma_r=0.35, normal_iters=10, vertex_iters=10, max_move=None, fix_boundary=True, origin=None,
           weld_first=True):
    """-> dict: xyz [nv, 3] fp64, rgb, faces (the welded mesh, positions moved); p0, p (relative to the origin), n0 / area / centroid
    (step 1), normals (after step 3), F, N (the incidence lists), fixed, clamped, moved, info."""
    xyz, rgb, faces = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(rgb, np.uint8).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    if weld_first and len(xyz):
        xyz, rgb, faces = weld(xyz, rgb, faces)
    faces = faces.astype(np.int64)
    nv, nf = len(xyz), len(faces)
    O = np.asarray(origin, np.float64) if origin is not None else (xyz.min(0) if nv else np.zeros(3))
    cap = float(max_move)
    p0 = xyz - O
    n0, A, c0 = face_records(p0, faces)
    F, N = incidence(faces, nv)
    Nidx, Nmask = padded(N)
    Fidx, Fmask = padded(F)
    n = filter_normals(n0, A, c0, Nidx, Nmask, float(sigma_s), float(sigma_r), normal_iters)
    fixed = boundary_vertices(faces, nv) if fix_boundary else np.zeros(nv, bool)
    p, clamped = update_vertices(p0, faces, n, Fidx, Fmask, fixed, cap, vertex_iters)
    moved = ~(fixed | (Fmask.sum(1) == 0)) if vertex_iters else np.zeros(nv, bool)
    out = np.where(moved[:, None], O + p, xyz)
    move = np.sqrt(((p - p0) ** 2).sum(1))
    info = dict(vertices=int(nv), faces=int(nf), fixed=int(fixed.sum()), degenerate_faces=int((A == 0).sum()), clamped=int(clamped.sum()),
                largest_move=float(move.max()) if nv else 0.0, rms_move=float(np.sqrt((move ** 2).mean())) if nv else 0.0)
    return dict(xyz=out, rgb=rgb, faces=faces, origin=O, p0=p0, p=p, n0=n0, area=A, centroid=c0, normals=n, F=F, N=N, fixed=fixed,
                clamped=clamped, moved=moved, info=info)
