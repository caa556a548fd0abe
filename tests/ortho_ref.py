"""fp64 numpy restatement of the image orthophoto (include/adamvs_hip.h "Image orthophoto"): the surface, the per-view z-buffer
(the same inclusive rule), visibility, both modes and the finalize step.

The z-buffer can be evaluated with the edge test moved by `grow` pixels (distance from each edge): grow > 0 takes in pixels
just outside a triangle, grow < 0 leaves out those just inside.  Two such buffers bracket every fp32 rasterisation whose
edge decisions may go either way within |grow|, and the visibility helpers use them to set aside marginal decisions.
"""
import numpy as np

MODES = ("best", "feather")
NEAR = 0.1


def surface(dsm, K):
    """height [H K, W K] fp64 (NaN: no surface) of the triangulated DSM at the orthophoto cell centres."""
    dsm = np.asarray(dsm, np.float32)
    H, W = dsm.shape
    i = np.arange(W * K, dtype=np.float64)
    j = np.arange(H * K, dtype=np.float64)
    s = np.clip((i + 0.5) / K - 0.5, 0.0, W - 1)[None, :].repeat(H * K, 0)
    t = np.clip((j + 0.5) / K - 0.5, 0.0, H - 1)[:, None].repeat(W * K, 1)
    a, b = np.floor(s).astype(np.int64), np.floor(t).astype(np.int64)
    fs, ft = s - a, t - b
    first = fs >= ft
    va = [a, np.where(first, a + 1, a), a + 1]
    vb = [b, np.where(first, b, b + 1), b + 1]
    w = [np.where(first, 1 - fs, 1 - ft), np.where(first, fs - ft, ft - fs), np.where(first, ft, fs)]
    h = np.zeros(s.shape)
    ok = np.ones(s.shape, bool)
    for k in range(3):
        use = w[k] > 0
        z = dsm[np.minimum(vb[k], H - 1), np.minimum(va[k], W - 1)].astype(np.float64)
        ok &= ~use | np.isfinite(z)
        h = h + np.where(use, w[k] * np.where(np.isfinite(z), z, 0.0), 0.0)
    return np.where(ok, h, np.nan)


def cell_centres(grid, K):
    """(x, y) fp64 [H K, W K] of the orthophoto cell centres; grid: dsm.Grid of the DSM."""
    g = grid.gsd / K
    x = grid.x0 + (np.arange(grid.W * K) + 0.5) * g
    y = grid.y_top - (np.arange(grid.H * K) + 0.5) * g
    return np.broadcast_to(x[None, :], (grid.H * K, grid.W * K)), np.broadcast_to(y[:, None], (grid.H * K, grid.W * K))


def project(cam, X, Y, Z):
    """World points (fp64) -> (d [.., 3] = X - C, u, v, z), all fp64.  cam: dict(K, R (R_wc), C)."""
    d = np.stack([X - cam["C"][0], Y - cam["C"][1], Z - cam["C"][2]], -1)
    p = d @ np.asarray(cam["R"], np.float64)          # R_cw d
    K = np.asarray(cam["K"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (K[0, 0] * p[..., 0] + K[0, 1] * p[..., 1] + K[0, 2] * p[..., 2]) / p[..., 2]
        v = (K[1, 0] * p[..., 0] + K[1, 1] * p[..., 1] + K[1, 2] * p[..., 2]) / p[..., 2]
    return d, u, v, p[..., 2]


def triangles(grid, dsm, cam):
    """Screen-space triangles of the split that pass the vertex tests -> (u [n, 3], v [n, 3], z [n, 3]), oriented (area > 0)."""
    dsm = np.asarray(dsm, np.float32)
    H, W = dsm.shape
    a, b = np.meshgrid(np.arange(W), np.arange(H))
    X = grid.x0 + (a + 0.5) * grid.gsd
    Y = grid.y_top - (b + 0.5) * grid.gsd
    _, U, V, Z = project(cam, X, Y, dsm.astype(np.float64))
    good = np.isfinite(dsm) & (Z > NEAR) & np.isfinite(U) & np.isfinite(V)
    tris = []
    for da, db in (((0, 1, 1), (0, 0, 1)), ((0, 0, 1), (0, 1, 1))):
        idx = [(slice(db[k], H - 1 + db[k]), slice(da[k], W - 1 + da[k])) for k in range(3)]
        ok = good[idx[0]] & good[idx[1]] & good[idx[2]]
        tris.append(np.stack([np.stack([A[ix][ok] for ix in idx], -1) for A in (U, V, Z)], 0))
    t = np.concatenate(tris, 1) if tris else np.zeros((3, 0, 3))
    u, v, z = t[0], t[1], t[2]
    area = (u[:, 1] - u[:, 0]) * (v[:, 2] - v[:, 0]) - (v[:, 1] - v[:, 0]) * (u[:, 2] - u[:, 0])
    keep = (area != 0) & np.isfinite(area)
    u, v, z, area = u[keep], v[keep], z[keep], area[keep]
    flip = area < 0
    for A in (u, v, z):
        A[flip, 1], A[flip, 2] = A[flip, 2].copy(), A[flip, 1].copy()
    return u, v, z


def _edges(u, v, x, y):
    """Edge functions e0, e1, e2 and edge lengths for pixel centres (x, y) (broadcast against the triangles)."""
    e0 = (u[..., 2] - u[..., 1]) * (y - v[..., 1]) - (v[..., 2] - v[..., 1]) * (x - u[..., 1])
    e1 = (u[..., 0] - u[..., 2]) * (y - v[..., 2]) - (v[..., 0] - v[..., 2]) * (x - u[..., 2])
    e2 = (u[..., 1] - u[..., 0]) * (y - v[..., 0]) - (v[..., 1] - v[..., 0]) * (x - u[..., 0])
    l0 = np.hypot(u[..., 2] - u[..., 1], v[..., 2] - v[..., 1])
    l1 = np.hypot(u[..., 0] - u[..., 2], v[..., 0] - v[..., 2])
    l2 = np.hypot(u[..., 1] - u[..., 0], v[..., 1] - v[..., 0])
    return (e0, e1, e2), (l0, l1, l2)


def zbuf(grid, dsm, cam, H, W, grow=0.0):
    """Depth buffer [H, W] fp64 (+inf where uncovered) of the view: min over covering triangles of the perspective-correct
    depth.  grow moves every edge outward by that many pixels (0: the rule of the header)."""
    u, v, z = triangles(grid, dsm, cam)
    out = np.full(H * W, np.inf)
    pad = max(grow, 0.0)
    u0 = np.maximum(np.ceil(u.min(1) - pad), 0).astype(np.int64)
    u1 = np.minimum(np.floor(u.max(1) + pad), W - 1).astype(np.int64)
    v0 = np.maximum(np.ceil(v.min(1) - pad), 0).astype(np.int64)
    v1 = np.minimum(np.floor(v.max(1) + pad), H - 1).astype(np.int64)
    bw, bh = u1 - u0 + 1, v1 - v0 + 1
    live = (bw > 0) & (bh > 0)
    u, v, z, u0, v0, bw, bh = (A[live] for A in (u, v, z, u0, v0, bw, bh))
    area = (u[:, 1] - u[:, 0]) * (v[:, 2] - v[:, 0]) - (v[:, 1] - v[:, 0]) * (u[:, 2] - u[:, 0])
    iz = 1.0 / z

    def splat(sel, du, dv):
        x = (u0[sel] + du).astype(np.float64)
        y = (v0[sel] + dv).astype(np.float64)
        inside = (du < bw[sel]) & (dv < bh[sel])
        (e0, e1, e2), (l0, l1, l2) = _edges(u[sel], v[sel], x, y)
        cov = inside & (e0 >= -grow * l0) & (e1 >= -grow * l1) & (e2 >= -grow * l2)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = area[sel] / (e0 * iz[sel, 0] + e1 * iz[sel, 1] + e2 * iz[sel, 2])
        cov &= np.isfinite(d) & (d > 0)
        np.minimum.at(out, (y[cov].astype(np.int64) * W + x[cov].astype(np.int64)), d[cov])

    small = (bw <= 4) & (bh <= 4)
    sel = np.nonzero(small)[0]
    for dv in range(4):
        for du in range(4):
            splat(sel, du, dv)
    for t in np.nonzero(~small)[0]:
        dv, du = np.mgrid[0:bh[t], 0:bw[t]]
        splat(np.full(du.size, t), du.reshape(-1), dv.reshape(-1))
    return out.reshape(H, W)


def view_terms(grid, K, height, cam, H, W, border):
    """Per cell, fp64: dict(z, u, v, score, inb (surface, in front and inside the border), border) of the sample P in one
    view."""
    x, y = cell_centres(grid, K)
    d, u, v, z = project(cam, x, y, np.where(np.isnan(height), 0.0, height))
    with np.errstate(invalid="ignore"):
        score = -d[..., 2] / np.sqrt((d * d).sum(-1))
        inb = ~np.isnan(height) & (z > 0) & (u >= border) & (u <= W - 1 - border) & (v >= border) & (v <= H - 1 - border)
    return dict(z=z, u=u, v=v, score=score, inb=inb, border=border)


def bilinear(img, u, v):
    """Bilinear sample [.., 3] fp64 of img [H, W, >=3] at (u, v) (inside the image)."""
    H, W = img.shape[:2]
    xa = np.floor(u).astype(np.int64)
    ya = np.floor(v).astype(np.int64)
    fx, fy = (u - xa)[..., None], (v - ya)[..., None]
    xb, yb = np.minimum(xa + 1, W - 1), np.minimum(ya + 1, H - 1)
    c = img[..., :3].astype(np.float64)
    return (1 - fy) * ((1 - fx) * c[ya, xa] + fx * c[ya, xb]) + fy * ((1 - fx) * c[yb, xa] + fx * c[yb, xb])


def visibility(t, zb, tol, margin=None):
    """Visible mask of one view from view_terms t and the z-buffer zb (header rule).  With margin = (zb_lo, zb_hi, eps_px,
    eps_z) -> (visible, marginal): a decision is marginal if the border test, the pixel rounding or the depth test could go the
    other way within eps_px pixels / eps_z metres, or between the bracketing buffers zb_lo <= zb <= zb_hi."""
    H, W = zb.shape
    inb = t["inb"]
    u = np.where(inb, t["u"], 0.0)
    v = np.where(inb, t["v"], 0.0)
    pu = np.clip(np.floor(u + 0.5).astype(np.int64), 0, W - 1)
    pv = np.clip(np.floor(v + 0.5).astype(np.int64), 0, H - 1)
    vis = inb & (t["z"] <= zb[pv, pu] + tol)
    if margin is None:
        return vis
    zb_lo, zb_hi, eps, eps_z = margin
    lo = np.full(u.shape, np.inf)
    hi = np.full(u.shape, -np.inf)
    for su in (-eps, eps):
        for sv in (-eps, eps):
            qu = np.clip(np.floor(u + su + 0.5).astype(np.int64), 0, W - 1)
            qv = np.clip(np.floor(v + sv + 0.5).astype(np.int64), 0, H - 1)
            lo = np.minimum(lo, zb_lo[qv, qu])
            hi = np.maximum(hi, zb_hi[qv, qu])
    sure_vis = t["z"] <= lo + tol - eps_z
    sure_hid = t["z"] > hi + tol + eps_z
    b = t["border"]
    with np.errstate(invalid="ignore"):
        near_border = ~np.isnan(t["u"]) & ((np.abs(t["u"] - b) < eps) | (np.abs(t["u"] - (W - 1 - b)) < eps) |
                                           (np.abs(t["v"] - b) < eps) | (np.abs(t["v"] - (H - 1 - b)) < eps))
    marginal = (inb & ~sure_vis & ~sure_hid) | near_border
    return vis, marginal


def compose(grid, dsm, K, views, mode="best", tol=None, border=2.0, feather_px=64.0, zbufs=None, margin=None):
    """The whole mosaic in fp64.  views: [dict(iid, K, R, C, rgba [H, W, 4] uint8 host)] in ascending iid.
    -> dict(rgba, view, nvis, height, marginal (cells whose visibility or choice may go either way; with margin = (grow_px,
    eps_z, eps_score), eps_score relative to the leading score or weight))."""
    assert mode in MODES
    tol = 2.0 * grid.gsd if tol is None else tol
    height = surface(dsm, K)
    shape = height.shape
    nvis = np.zeros(shape, np.int64)
    best_s = np.full(shape, -np.inf)
    view = np.full(shape, -1, np.int64)
    col = np.zeros(shape + (3,))
    sw = np.zeros(shape)
    swc = np.zeros(shape + (3,))
    wmax = np.zeros(shape)
    marginal = np.zeros(shape, bool)
    scores = []
    for vw in views:
        img = np.asarray(vw["rgba"])
        H, W = img.shape[:2]
        zb = zbufs[vw["iid"]] if zbufs is not None else zbuf(grid, dsm, vw, H, W)
        t = view_terms(grid, K, height, vw, H, W, border)
        if margin is not None:
            g, eps_z, _ = margin
            vis, marg = visibility(t, zb, tol, (zbuf(grid, dsm, vw, H, W, g), zbuf(grid, dsm, vw, H, W, -g), g, eps_z))
            marginal |= marg
        else:
            vis = visibility(t, zb, tol)
        nvis += vis
        c = np.zeros(shape + (3,))
        if vis.any():
            c[vis] = bilinear(img, t["u"][vis], t["v"][vis])
        s = np.where(vis, t["score"], -np.inf)
        if mode == "best":
            scores.append(s)
            take = vis & (s > best_s)
            best_s = np.where(take, s, best_s)
            view = np.where(take, vw["iid"], view)
            col = np.where(take[..., None], c, col)
        else:
            e = np.minimum(np.minimum(t["u"], W - 1 - t["u"]), np.minimum(t["v"], H - 1 - t["v"]))
            w = np.where(vis, s ** 4 * np.minimum(1.0, (e - border) / feather_px), 0.0)
            scores.append(np.where(vis, w, -np.inf))
            sw += w
            swc += w[..., None] * c
            take = vis & (w > wmax)
            wmax = np.where(take, w, wmax)
            view = np.where(take, vw["iid"], view)
    if margin is not None and len(scores) > 1:
        # the choice between the two leading views (scores in best mode, weights in feather mode) is a tie within eps_score,
        # relative to the leader
        S = np.sort(np.stack(scores), 0)
        with np.errstate(invalid="ignore"):
            marginal |= np.isfinite(S[-2]) & (S[-1] - S[-2] <= margin[2] * np.abs(S[-1]))
    if mode == "best":
        ok = view >= 0
        c = col
    else:
        ok = (view >= 0) & (sw > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            c = swc / sw[..., None]
    rgba = np.zeros(shape + (4,), np.uint8)
    rgba[ok, :3] = np.clip(np.floor(c[ok] + 0.5), 0, 255).astype(np.uint8)
    rgba[ok, 3] = 255
    return dict(rgba=rgba, view=np.where(ok, view, -1).astype(np.int32), nvis=np.minimum(nvis, 65535).astype(np.uint16), height=height,
                marginal=marginal)


def plane_zbuf(cam, H, W, n, c):
    """Closed form: the depth [H, W] at every pixel centre of the plane n . X = c seen by cam (inf where the ray misses it or
    meets it behind the camera)."""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ray_c = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(np.asarray(cam["K"], np.float64)).T     # camera z = 1
    r = ray_c @ np.asarray(cam["R"], np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (c - np.dot(n, cam["C"])) / (r @ np.asarray(n, np.float64))
    return np.where(z > 0, z, np.inf)

