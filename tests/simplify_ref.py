"""numpy restatement of include/adamvs_hip.h "Mesh simplification": the six steps in fp64 (np.linalg.eigh, np.add.at, np.unique),
written from the header's rule and sharing no code with csrc/mesh_simplify.hip.  Besides the result it returns every
intermediate the GPU tests compare (cells, the faces' cells, the survive / duplicate / used decisions, ranks, fallbacks) and, per
cell, the two tie flags inside which the GPU's Jacobi solve may decide the other way."""
import numpy as np

KEY_BITS = 21
RANK_TIE = 1e-6            # |lambda_k / lambda_max - rank_eps| <= RANK_TIE * rank_eps
BOX_TIE = 1e-9             # ||p_k| - c / 2| <= BOX_TIE * c


class SimplifyError(ValueError):
    pass


def weld(xyz, rgb, faces):
    """Exact-position weld as ada_mvs_amd.mesh.weld does it (coincident vertices carry the same colour)."""
    u, inv = np.unique(np.asarray(xyz, np.float64), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    col = np.empty((len(u), 3), np.uint8)
    col[inv] = np.asarray(rgb, np.uint8)
    return u, col, inv[np.asarray(faces).astype(np.int64)]


def cell_keys(xyz, cell, origin):
    """Step 1 -> (key [nv] int64, index [nv, 3] int64); raises for a non-finite coordinate or an index outside 0 .. 2^21 - 1."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (xyz - np.asarray(origin, np.float64)) / float(cell)
        ok = np.isfinite(xyz) & (t >= 0) & (t < float(1 << KEY_BITS))
    if not ok.all():
        raise SimplifyError("a coordinate is not finite or its cell index lies outside 0 .. 2^21 - 1")
    i = np.floor(t).astype(np.int64)
    return (i[:, 2] << (2 * KEY_BITS)) | (i[:, 1] << KEY_BITS) | i[:, 0], i


def simplify(xyz, rgb, faces, cell, origin, rank_eps=1e-3, weld_first=True):
    """-> dict: xyz [n, 3] fp64, rgb [n, 3] uint8, faces [m, 3] int64 (the result); keys [nc] int64, vcell [nv], fcell [nf, 3],
    survive / keep [nf] bool, used [nc] bool, pos [nc, 3], col [nc, 3], rank [nc], fallback [nc], rank_tie / box_tie [nc], the quadrics A
    [nc, 3, 3], b [nc, 3], dd [nc], the members' mean [nc, 3] and count [nc], info."""
    c = float(cell)
    O = np.asarray(origin, np.float64)
    xyz, rgb, faces = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(rgb, np.uint8).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    if weld_first and len(xyz):
        xyz, rgb, faces = weld(xyz, rgb, faces)
    faces = faces.astype(np.int64)
    nv, nf = len(xyz), len(faces)
    key, _ = cell_keys(xyz, c, O)
    keys, vcell = np.unique(key, return_inverse=True)
    vcell = vcell.reshape(-1)
    nc = len(keys)
    mask = (1 << KEY_BITS) - 1
    idx = np.stack([keys & mask, (keys >> KEY_BITS) & mask, keys >> (2 * KEY_BITS)], 1).astype(np.float64)
    centre = O + (idx + 0.5) * c
    # step 2: quadrics, once per face and cell
    fcell = vcell[faces] if nf else np.zeros((0, 3), np.int64)
    A = np.zeros((nc, 3, 3))
    b = np.zeros((nc, 3))
    dd = np.zeros(nc)
    for k in range(3):
        new = np.ones(nf, bool)
        for j in range(k):
            new &= fcell[:, k] != fcell[:, j]
        f = np.nonzero(new)[0]
        cc = fcell[f, k]
        p = xyz[faces[f]] - centre[cc][:, None, :]
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        d = -np.einsum("ij,ij->i", n, p[:, 0])
        np.add.at(A, cc, n[:, :, None] * n[:, None, :])
        np.add.at(b, cc, d[:, None] * n)
        np.add.at(dd, cc, d * d)
    # step 3: members
    count = np.bincount(vcell, minlength=nc).astype(np.int64)
    msum = np.zeros((nc, 3))
    np.add.at(msum, vcell, xyz - centre[vcell])
    m = msum / np.maximum(count, 1)[:, None]
    csum = np.zeros((nc, 3), np.int64)
    np.add.at(csum, vcell, rgb.astype(np.int64))
    col = ((csum + (count // 2)[:, None]) // np.maximum(count, 1)[:, None]).astype(np.uint8)
    # step 4: representative
    lam, V = np.linalg.eigh(A) if nc else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    lmax = lam.max(1) if nc else np.zeros(0)
    kept = lam > rank_eps * lmax[:, None]
    g = -(b + np.einsum("nij,nj->ni", A, m))
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(kept, np.einsum("njk,nj->nk", V, g) / lam, 0.0)       # (v_k . g) / lambda_k for the kept k
        ratio = lam / lmax[:, None]
    p = m + np.einsum("nik,nk->ni", V, w)
    rank = kept.sum(1)
    with np.errstate(invalid="ignore"):
        fallback = (rank == 0) | ~np.isfinite(p).all(1) | (np.abs(p) > c / 2).any(1)
        rank_tie = (np.abs(ratio - rank_eps) <= RANK_TIE * rank_eps).any(1)
        box_tie = (rank > 0) & (np.abs(np.abs(p) - c / 2) <= BOX_TIE * c).any(1)
    p = np.where(fallback[:, None], m, p)
    pos = centre + p
    err = np.einsum("ni,nij,nj->n", p, A, p) + 2 * np.einsum("ni,ni->n", b, p) + dd
    # step 5: faces
    survive = (fcell[:, 0] != fcell[:, 1]) & (fcell[:, 1] != fcell[:, 2]) & (fcell[:, 0] != fcell[:, 2])
    keep = np.zeros(nf, bool)
    s = np.nonzero(survive)[0]
    if len(s):
        _, first = np.unique(np.sort(fcell[s], 1), axis=0, return_index=True)       # the first occurrence of each set
        keep[s[first]] = True
    # step 6: vertices out
    used = np.zeros(nc, bool)
    used[fcell[keep].ravel()] = True
    new = np.cumsum(used) - 1
    info = dict(cells=int(nc), cells_used=int(used.sum()), vertices_in=int(nv), faces_in=int(nf), faces_collapsed=int((~survive).sum()),
                faces_duplicate=int(survive.sum() - keep.sum()), faces_out=int(keep.sum()),
                rank_hist=[int((rank == r).sum()) for r in range(4)], fallbacks=int(fallback.sum()))
    return dict(xyz=pos[used], rgb=col[used], faces=new[fcell[keep]], keys=keys, vcell=vcell, fcell=fcell, survive=survive, keep=keep,
                used=used, centre=centre, pos=pos, col=col, rank=rank, fallback=fallback, rank_tie=rank_tie, box_tie=box_tie, error=err,
                A=A, b=b, dd=dd, mean=m, count=count, info=info)
