"""fp64 numpy restatement of the mesh texture (include/adamvs_hip.h "Mesh texturing"): projection, the per-view z-buffer (the
orthophoto's inclusive rule on arbitrary triangles), visibility and the label, connected charts (root = the smallest face),
boxes, an independent shelf packer, the atlas and the texture coordinates.

As in tests/ortho_ref.py, the z-buffer can be evaluated with every edge moved by `grow` pixels; two such buffers bracket every
fp32 rasterisation whose edge decisions may go either way, and labels() uses them to set aside faces whose visibility or
choice is marginal."""
import numpy as np

NEAR = 0.1


def project(cam, xyz):
    """xyz [n, 3] fp64 -> (u, v, z) fp64 [n].  cam: dict(K, R (R_wc), C)."""
    d = np.asarray(xyz, np.float64) - np.asarray(cam["C"], np.float64)
    p = d @ np.asarray(cam["R"], np.float64)
    K = np.asarray(cam["K"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (K[0, 0] * p[:, 0] + K[0, 1] * p[:, 1] + K[0, 2] * p[:, 2]) / p[:, 2]
        v = (K[1, 0] * p[:, 0] + K[1, 1] * p[:, 1] + K[1, 2] * p[:, 2]) / p[:, 2]
    return u, v, p[:, 2]


def corners(u, v, z, faces):
    f = np.asarray(faces, np.int64)
    return u[f], v[f], z[f]


def zbuf(u, v, z, faces, H, W, grow=0.0):
    """Depth buffer [H, W] fp64 (+inf where uncovered) of the faces whose three vertices have z > NEAR and finite (u, v)."""
    U, V, Z = corners(u, v, z, faces)
    ok = (Z > NEAR).all(1) & np.isfinite(U).all(1) & np.isfinite(V).all(1)
    U, V, Z = U[ok].copy(), V[ok].copy(), Z[ok].copy()
    area = (U[:, 1] - U[:, 0]) * (V[:, 2] - V[:, 0]) - (V[:, 1] - V[:, 0]) * (U[:, 2] - U[:, 0])
    keep = (area != 0) & np.isfinite(area)
    U, V, Z, area = U[keep], V[keep], Z[keep], area[keep]
    flip = area < 0
    for A in (U, V, Z):
        A[flip, 1], A[flip, 2] = A[flip, 2].copy(), A[flip, 1].copy()
    area = np.abs(area)
    out = np.full(H * W, np.inf)
    pad = max(grow, 0.0)
    u0 = np.maximum(np.ceil(U.min(1) - pad), 0).astype(np.int64)
    u1 = np.minimum(np.floor(U.max(1) + pad), W - 1).astype(np.int64)
    v0 = np.maximum(np.ceil(V.min(1) - pad), 0).astype(np.int64)
    v1 = np.minimum(np.floor(V.max(1) + pad), H - 1).astype(np.int64)
    bw, bh = u1 - u0 + 1, v1 - v0 + 1
    live = (bw > 0) & (bh > 0)
    U, V, Z, area, u0, v0, bw, bh = (A[live] for A in (U, V, Z, area, u0, v0, bw, bh))
    iz = 1.0 / Z
    l0 = np.hypot(U[:, 2] - U[:, 1], V[:, 2] - V[:, 1])
    l1 = np.hypot(U[:, 0] - U[:, 2], V[:, 0] - V[:, 2])
    l2 = np.hypot(U[:, 1] - U[:, 0], V[:, 1] - V[:, 0])

    def splat(sel, du, dv):
        x = (u0[sel] + du).astype(np.float64)
        y = (v0[sel] + dv).astype(np.float64)
        inside = (du < bw[sel]) & (dv < bh[sel])
        Us, Vs = U[sel], V[sel]
        e0 = (Us[:, 2] - Us[:, 1]) * (y - Vs[:, 1]) - (Vs[:, 2] - Vs[:, 1]) * (x - Us[:, 1])
        e1 = (Us[:, 0] - Us[:, 2]) * (y - Vs[:, 2]) - (Vs[:, 0] - Vs[:, 2]) * (x - Us[:, 2])
        e2 = (Us[:, 1] - Us[:, 0]) * (y - Vs[:, 0]) - (Vs[:, 1] - Vs[:, 0]) * (x - Us[:, 0])
        cov = inside & (e0 >= -grow * l0[sel]) & (e1 >= -grow * l1[sel]) & (e2 >= -grow * l2[sel])
        with np.errstate(divide="ignore", invalid="ignore"):
            d = area[sel] / (e0 * iz[sel, 0] + e1 * iz[sel, 1] + e2 * iz[sel, 2])
        cov &= np.isfinite(d) & (d > 0)
        np.minimum.at(out, y[cov].astype(np.int64) * W + x[cov].astype(np.int64), d[cov])

    small = (bw <= 4) & (bh <= 4)
    sel = np.nonzero(small)[0]
    for dv in range(4):
        for du in range(4):
            splat(sel, np.full(sel.size, du), np.full(sel.size, dv))
    for t in np.nonzero(~small)[0]:
        dv, du = np.mgrid[0:bh[t], 0:bw[t]]
        splat(np.full(du.size, t), du.reshape(-1), dv.reshape(-1))
    return out.reshape(H, W)


def labels(xyz, faces, views, tol, border, zbufs, margin=None):
    """The label of every face over the views (ascending image id; the label is the index in `views`).  zbufs: image id ->
    the view's depth buffer (the GPU's, so that the decisions are taken against the same buffer).  With margin = (grow_px,
    eps_z, eps_score, eps_area) also -> `marginal`: faces any of whose visibility decisions, or whose choice, could go the other
    way within those margins.  -> dict(label, nvis, uv [nf, 6], score, marginal)."""
    nf = len(faces)
    label = np.full(nf, -1, np.int64)
    nvis = np.zeros(nf, np.int64)
    best = np.full(nf, -np.inf)
    second = np.full(nf, -np.inf)
    uv = np.zeros((nf, 6))
    marginal = np.zeros(nf, bool)
    err = np.zeros(nf)          # a bound of the fp32 score's rounding: u and v carry about 2^-22 of the image size
    for vi, vw in enumerate(views):
        if vw["iid"] not in zbufs:
            continue
        zb = zbufs[vw["iid"]]
        H, W = zb.shape
        u, v, z = project(vw, xyz)
        U, V, Z = corners(u, v, z, faces)
        with np.errstate(invalid="ignore"):
            inb = ((Z > NEAR) & (U >= border) & (U <= W - 1 - border) & (V >= border) & (V <= H - 1 - border)).all(1)
        t1 = (U[:, 1] - U[:, 0]) * (V[:, 2] - V[:, 0])
        t2 = (V[:, 1] - V[:, 0]) * (U[:, 2] - U[:, 0])
        area = t1 - t2
        Us, Vs = np.where(inb[:, None], U, 0.0), np.where(inb[:, None], V, 0.0)
        uc, vc = Us.mean(1), Vs.mean(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            zc = 3.0 / (1.0 / Z).sum(1)
        pts = [(Us[:, k], Vs[:, k], Z[:, k]) for k in range(3)] + [(uc, vc, zc)]

        def look(buf, pu, pv):
            return buf[np.clip(np.floor(pv + 0.5).astype(np.int64), 0, H - 1), np.clip(np.floor(pu + 0.5).astype(np.int64), 0, W - 1)]

        vis = inb & (area < 0)
        for pu, pv, pz in pts:
            vis &= pz <= look(zb, pu, pv) + tol
        if margin is not None:
            g, eps_z, _, eps_a = margin
            zlo, zhi = zbuf(u, v, z, faces, H, W, g), zbuf(u, v, z, faces, H, W, -g)
            m = np.zeros(nf, bool)
            with np.errstate(invalid="ignore"):
                for k in range(3):
                    m |= (np.abs(U[:, k] - border) < g) | (np.abs(U[:, k] - (W - 1 - border)) < g)
                    m |= (np.abs(V[:, k] - border) < g) | (np.abs(V[:, k] - (H - 1 - border)) < g)
            m &= np.isfinite(U).all(1)
            m |= inb & (np.abs(area) <= eps_a * np.maximum(np.abs(t1), np.abs(t2)))
            cand = inb & (area < 0)
            for pu, pv, pz in pts:
                lo = np.full(nf, np.inf)
                hi = np.full(nf, -np.inf)
                for su in (-g, g):
                    for sv in (-g, g):
                        lo = np.minimum(lo, look(zlo, pu + su, pv + sv))
                        hi = np.maximum(hi, look(zhi, pu + su, pv + sv))
                sure_vis = pz <= lo + tol - eps_z
                sure_hid = pz > hi + tol + eps_z
                m |= cand & ~sure_vis & ~sure_hid
            marginal |= m
        score = np.where(vis, -area / 2.0, -np.inf)
        with np.errstate(invalid="ignore"):
            ext = np.maximum(np.abs(U - np.roll(U, 1, 1)).max(1), np.abs(V - np.roll(V, 1, 1)).max(1))
            err = np.maximum(err, np.where(vis, 2.0 ** -20 * max(W, H) * ext, 0.0))
        nvis += vis
        take = vis & (score > best)
        second = np.where(take, best, np.maximum(second, score))
        best = np.where(take, score, best)
        label = np.where(take, vi, label)
        uv[take] = np.stack([U[take, 0], V[take, 0], U[take, 1], V[take, 1], U[take, 2], V[take, 2]], 1)
    if margin is not None:
        eps_s = margin[2]
        with np.errstate(invalid="ignore"):
            marginal |= np.isfinite(second) & (np.abs(best - second) <= eps_s * np.abs(best) + 2.0 * err)
    return dict(label=label, nvis=nvis, uv=uv, score=best, marginal=marginal)


def components(label, faces):
    """parent [nf]: the smallest face of each face's chart (faces with the same label >= 0 joined through shared edges); an
    untextured face is its own parent."""
    f = np.asarray(faces, np.int64)
    nf = len(f)
    a, b = np.minimum(f, np.roll(f, -1, 1)), np.maximum(f, np.roll(f, -1, 1))
    ent_face = np.repeat(np.arange(nf), 3)
    key = a.reshape(-1) * (int(f.max()) + 1 if nf else 1) + b.reshape(-1)
    lab = np.repeat(np.asarray(label, np.int64), 3)
    good = lab >= 0
    key, lab, ent_face = key[good], lab[good], ent_face[good]
    # every face of a (key, label) group joins the group's first face
    order = np.lexsort((ent_face, lab, key))
    key, lab, ent_face = key[order], lab[order], ent_face[order]
    start = np.ones(len(key), bool)
    start[1:] = (key[1:] != key[:-1]) | (lab[1:] != lab[:-1])
    head = ent_face[np.maximum.accumulate(np.where(start, np.arange(len(key)), 0))]
    parent = np.arange(nf)
    while True:
        old = parent.copy()
        m = np.minimum(parent[head], parent[ent_face])
        np.minimum.at(parent, head, m)
        np.minimum.at(parent, ent_face, m)
        parent = parent[parent]
        while not np.array_equal(parent, parent[parent]):
            parent = parent[parent]
        if np.array_equal(parent, old):
            return parent


def charts(label, parent, uv, Ws, Hs, pad):
    """-> (chart [nf] (-1 untextured), table [nc, 6] = x0, y0, w, h, view, root) with charts numbered in ascending root order."""
    label = np.asarray(label, np.int64)
    roots = np.nonzero((label >= 0) & (parent == np.arange(len(label))))[0]
    cid = np.full(len(label), -1, np.int64)
    cid[roots] = np.arange(len(roots))
    chart = np.where(label >= 0, cid[parent], -1)
    nc = len(roots)
    uv = np.asarray(uv, np.float64).reshape(-1, 6)
    U, V = uv[:, 0::2], uv[:, 1::2]
    tex = label >= 0
    mnu, mnv = np.full(nc, np.inf), np.full(nc, np.inf)
    mxu, mxv = np.full(nc, -np.inf), np.full(nc, -np.inf)
    np.minimum.at(mnu, chart[tex], np.floor(U[tex].min(1)))
    np.minimum.at(mnv, chart[tex], np.floor(V[tex].min(1)))
    np.maximum.at(mxu, chart[tex], np.floor(U[tex].max(1)))
    np.maximum.at(mxv, chart[tex], np.floor(V[tex].max(1)))
    view = label[roots]
    W, H = np.asarray(Ws)[view], np.asarray(Hs)[view]
    x0, y0 = np.maximum(mnu - pad, 0), np.maximum(mnv - pad, 0)
    x1, y1 = np.minimum(mxu + 1 + pad, W - 1), np.minimum(mxv + 1 + pad, H - 1)
    table = np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1, view, roots], 1).astype(np.int64)
    return chart, table


def shelf_pack(sizes, P):
    """An independent statement of the packing rule, item by item: sizes [(w, h)] -> [(ox, oy, page)], pages."""
    order = sorted(range(len(sizes)), key=lambda i: (-sizes[i][1], -sizes[i][0], i))
    out = [None] * len(sizes)
    x = y = page = 0
    shelf_h = None
    for i in order:
        w, h = sizes[i]
        if shelf_h is None:
            shelf_h = h
        elif x + w > P:
            x, y = 0, y + shelf_h
            shelf_h = h
            if y + h > P:
                page, y = page + 1, 0
        out[i] = (x, y, page)
        x += w
    return out, (page + 1 if sizes else 0)


def atlas(table, place, views, P, pages, pal=None, pal_faces=None, rgb=None, faces=None):
    """Atlas [pages, P, P, 3] uint8: each chart's box copied from its view's image; the palette texels (pal = (ox, oy, page),
    pal_faces: the untextured faces in face order) with the rounded mean of their vertex colours."""
    out = np.zeros((pages, P, P, 3), np.uint8)
    for (x0, y0, w, h, view, _), (ox, oy, pg) in zip(table, place):
        img = np.asarray(views[view]["rgba"])
        out[pg, oy:oy + h, ox:ox + w] = img[y0:y0 + h, x0:x0 + w, :3]
    if pal is not None and len(pal_faces):
        ox, oy, pg = pal
        k = np.arange(len(pal_faces))
        s = np.asarray(rgb, np.int64)[np.asarray(faces, np.int64)[pal_faces]].sum(1)
        out[pg, oy + k // P, ox + k % P] = np.floor(s / 3.0 + 0.5).astype(np.uint8)
    return out


def bilinear(img, x, y):
    """Bilinear sample [.., 3] fp64 of img [H, W, >=3] at pixel coordinates (x, y), the taps clamped to the image."""
    H, W = img.shape[:2]
    xa = np.clip(np.floor(x).astype(np.int64), 0, W - 1)
    ya = np.clip(np.floor(y).astype(np.int64), 0, H - 1)
    fx, fy = (x - np.floor(x))[..., None], (y - np.floor(y))[..., None]
    xb, yb = np.minimum(xa + 1, W - 1), np.minimum(ya + 1, H - 1)
    c = img[..., :3].astype(np.float64)
    return (1 - fy) * ((1 - fx) * c[ya, xa] + fx * c[ya, xb]) + fy * ((1 - fx) * c[yb, xa] + fx * c[yb, xb])


def sample_atlas(atl, page, s, t):
    """Bilinear sample of atlas page `page` at texture coordinates (s, t) (origin bottom-left, texel centres at (i + 1/2) / P)."""
    P = atl.shape[1]
    return bilinear(atl[page], np.asarray(s, np.float64) * P - 0.5, (1.0 - np.asarray(t, np.float64)) * P - 0.5)
