"""float64 numpy restatement of the seam levelling (include/adamvs_hip.h "Mesh texturing", seam levelling), written from the
definition: nodes, smoothness / data / seam edges, the observed colour f, the graph Laplacian and its minimum-norm solution
(a dense solve; plain conjugate gradients too), the owner map with its dilation and the levelled texels.

The owner map can be evaluated with every edge moved by `grow` pixels, as tests/texture_ref.py's z-buffer can: two such maps
bracket every fp32 rasterisation whose edge decisions may go either way."""
import numpy as np

import texture_ref as R

UNOWNED = 2 ** 31 - 1
BAND = 2


# ---- graph ------------------------------------------------------------------------------------------------------------------
def nodes(faces, chart):
    """-> (node_vertex [n], node_chart [n], corner_node [nf, 3] (-1 on untextured faces)): one node per distinct (vertex, chart)
    over the corners of textured faces, in ascending (vertex, chart)."""
    faces = np.asarray(faces, np.int64)
    chart = np.asarray(chart, np.int64)
    tex = chart >= 0
    pairs = np.stack([faces[tex].reshape(-1), np.repeat(chart[tex], 3)], 1)
    uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
    corner = np.full((len(faces), 3), -1, np.int64)
    corner[tex] = np.asarray(inv).reshape(-1, 3)
    return uniq[:, 0], uniq[:, 1], corner


def edges(faces, chart, corner):
    """-> (smooth [ms, 2], seam [ms] bool, data [md, 2]): undirected edges as ascending node pairs, each once, sorted."""
    faces = np.asarray(faces, np.int64)
    chart = np.asarray(chart, np.int64)
    tex = np.nonzero(chart >= 0)[0]
    smooth, mesh_edge_charts = set(), {}
    for f in tex:
        for k in range(3):
            v, w = int(faces[f, k]), int(faces[f, (k + 1) % 3])
            if v == w:
                continue
            a, b = int(corner[f, k]), int(corner[f, (k + 1) % 3])
            smooth.add((min(a, b), max(a, b), min(v, w), max(v, w)))
            mesh_edge_charts.setdefault((min(v, w), max(v, w)), set()).add(int(chart[f]))
    smooth = sorted(smooth)
    seam = np.array([len(mesh_edge_charts[(v, w)]) > 1 for _, _, v, w in smooth], bool)
    smooth = np.array([(a, b) for a, b, _, _ in smooth], np.int64).reshape(-1, 2)
    return smooth, seam, data_edges(faces, chart, corner)


def data_edges(faces, chart, corner):
    at = {}
    tex = np.nonzero(np.asarray(chart) >= 0)[0]
    for f in tex:
        for k in range(3):
            at.setdefault(int(faces[f, k]), set()).add(int(corner[f, k]))
    out = []
    for v in at:
        ns = sorted(at[v])               # ascending node = ascending chart at one vertex
        out += [(ns[i], ns[j]) for i in range(len(ns)) for j in range(i + 1, len(ns))]
    return np.array(sorted(out), np.int64).reshape(-1, 2)


def edges_fast(faces, chart, corner):
    """edges() by sorting instead of Python sets (the full scene): the same definition, the same output."""
    faces = np.asarray(faces, np.int64)
    chart = np.asarray(chart, np.int64)
    tex = chart >= 0
    fv, fc, cn = faces[tex], chart[tex], corner[tex]
    v, w = fv.reshape(-1), np.roll(fv, -1, 1).reshape(-1)
    a, b = cn.reshape(-1), np.roll(cn, -1, 1).reshape(-1)
    c = np.repeat(fc, 3)
    keep = v != w
    v, w, a, b, c = v[keep], w[keep], a[keep], b[keep], c[keep]
    me = np.stack([np.minimum(v, w), np.maximum(v, w)], 1)
    _, inv = np.unique(me, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    cmin = np.full(inv.max() + 1 if len(inv) else 0, np.iinfo(np.int64).max)
    cmax = np.full(len(cmin), -1)
    np.minimum.at(cmin, inv, c)
    np.maximum.at(cmax, inv, c)
    rows = np.stack([np.minimum(a, b), np.maximum(a, b), (cmin[inv] != cmax[inv]).astype(np.int64)], 1)
    rows = np.unique(rows, axis=0)
    nv, cnode = faces[tex].reshape(-1), corner[tex].reshape(-1)
    pairs = np.unique(np.stack([nv, cnode], 1), axis=0)          # (vertex, node), ascending
    out = []
    d = 1
    while d < len(pairs):
        i = np.nonzero(pairs[:-d, 0] == pairs[d:, 0])[0]
        if len(i) == 0:
            break
        out.append(np.stack([pairs[i, 1], pairs[i + d, 1]], 1))
        d += 1
    data = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    data = data[np.lexsort((data[:, 1], data[:, 0]))]
    return rows[:, :2], rows[:, 2].astype(bool), data


def positions(corner, uv, n):
    """pos [n, 2]: the (u, v) the faces stored at each node."""
    pos = np.zeros((n, 2))
    tex = corner[:, 0] >= 0
    pos[corner[tex].reshape(-1)] = np.asarray(uv, np.float64)[tex].reshape(-1, 2)
    return pos


# ---- observed colour --------------------------------------------------------------------------------------------------------
def observe(pos, node_view, smooth, seam, images):
    """f [n, 3] float64: the weighted mean of bilinear samples at p_v + t (p_w - p_v), t = 0, 1/4, 1/2, weights 1, 3/4, 1/2, over
    the node's seam edges; the single sample at p_v for a node without one.  images: per view index an [H, W, >= 3] array."""
    n = len(pos)
    s = smooth[seam]
    i = np.concatenate([s[:, 0], s[:, 1]])
    j = np.concatenate([s[:, 1], s[:, 0]])
    acc, wsum = np.zeros((n, 3)), np.zeros(n)
    f = np.zeros((n, 3))
    for vi in np.unique(node_view):
        img = np.asarray(images[vi])
        m = node_view[i] == vi
        ii, jj = i[m], j[m]
        for t, w in ((0.0, 1.0), (0.25, 0.75), (0.5, 0.5)):
            p = pos[ii] + t * (pos[jj] - pos[ii])
            np.add.at(acc, ii, w * R.bilinear(img, p[:, 0], p[:, 1]))
            np.add.at(wsum, ii, w)
        own = np.nonzero(node_view == vi)[0]
        f[own] = R.bilinear(img, pos[own, 0], pos[own, 1])
    has = wsum > 0
    f[has] = acc[has] / wsum[has, None]
    return f


# ---- the system -------------------------------------------------------------------------------------------------------------
def laplacian(n, smooth, data, lam):
    """Dense L = D - W [n, n] with weight 1 / lam on smoothness edges and 1 on data edges."""
    L = np.zeros((n, n))
    for e, w in ((smooth, 1.0 / lam), (data, 1.0)):
        np.add.at(L, (e[:, 0], e[:, 1]), -w)
        np.add.at(L, (e[:, 1], e[:, 0]), -w)
        np.add.at(L, (e[:, 0], e[:, 0]), w)
        np.add.at(L, (e[:, 1], e[:, 1]), w)
    return L


def rhs(f, data, n):
    """b_i = sum over data neighbours j of (f_j - f_i)."""
    b = np.zeros((n, f.shape[1]))
    d = f[data[:, 1]] - f[data[:, 0]]
    np.add.at(b, data[:, 0], d)
    np.add.at(b, data[:, 1], -d)
    return b


def components(n, edge_lists):
    """Connected-component label [n] (the smallest node of the component) of the graph with the given edges."""
    e = np.concatenate([np.asarray(x, np.int64).reshape(-1, 2) for x in edge_lists])
    lab = np.arange(n)
    while True:
        old = lab.copy()
        m = np.minimum(lab[e[:, 0]], lab[e[:, 1]])
        np.minimum.at(lab, e[:, 0], m)
        np.minimum.at(lab, e[:, 1], m)
        lab = lab[lab]
        while not np.array_equal(lab, lab[lab]):
            lab = lab[lab]
        if np.array_equal(lab, old):
            return lab


def min_norm(L, b, comp):
    """The minimum-norm solution of L g = b: solve (L + sum_c 1_c 1_c^T / n_c) g = b over the connected components c (b sums
    to zero on each, so the added term only fixes each component's mean at zero)."""
    A = L.copy()
    for c in np.unique(comp):
        idx = np.nonzero(comp == c)[0]
        A[np.ix_(idx, idx)] += 1.0 / len(idx)
    return np.linalg.solve(A, b)


def cg(L, b, tol, iters):
    """Plain conjugate gradients from 0, every column of b with its own scalars, all stopping together -> (g, iterations)."""
    g = np.zeros_like(b)
    r, p = b.copy(), b.copy()
    rr = (r * r).sum(0)
    bb = rr.copy()
    it = 0
    while it < iters and not (rr <= tol * tol * bb).all():
        Ap = L @ p
        pAp = (p * Ap).sum(0)
        alpha = np.where(pAp > 0, rr / np.where(pAp > 0, pAp, 1.0), 0.0)
        g += alpha * p
        r -= alpha * Ap
        new = (r * r).sum(0)
        beta = np.where((rr > 0) & (alpha != 0), new / np.where(rr > 0, rr, 1.0), 0.0)
        rr = new
        p = r + beta * p
        it += 1
    return g, it


def level(faces, chart, uv, chart_view, images, lam):
    """The whole chain on small cases -> dict(node_vertex, node_chart, corner, smooth, seam, data, pos, f, g)."""
    nv_, nc_, corner = nodes(faces, chart)
    smooth, seam, data = edges(faces, chart, corner)
    n = len(nv_)
    pos = positions(corner, uv, n)
    f = observe(pos, np.asarray(chart_view)[nc_], smooth, seam, images)
    g = min_norm(laplacian(n, smooth, data, lam), rhs(f, data, n), components(n, [smooth, data]))
    return dict(node_vertex=nv_, node_chart=nc_, corner=corner, smooth=smooth, seam=seam, data=data, pos=pos, f=f, g=g)


# ---- owner, dilation, apply -----------------------------------------------------------------------------------------------------
def owner_map(uv, chart, charts, prefix, grow=0.0):
    """owner [texels]: for every texel of every chart box (concatenated in chart order, row-major) the smallest face of the
    chart whose image triangle holds the texel centre (inclusive edge functions), UNOWNED if none.  grow: every edge moved
    outwards by that many pixels."""
    uv = np.asarray(uv, np.float64)
    chart = np.asarray(chart, np.int64)
    owner = np.full(int(prefix[-1]), UNOWNED, np.int64)
    tex = np.nonzero(chart >= 0)[0]
    U, V = uv[tex][:, 0::2].copy(), uv[tex][:, 1::2].copy()
    area = (U[:, 1] - U[:, 0]) * (V[:, 2] - V[:, 0]) - (V[:, 1] - V[:, 0]) * (U[:, 2] - U[:, 0])
    ok = (area != 0) & np.isfinite(area)
    tex, U, V, area = tex[ok], U[ok], V[ok], area[ok]
    flip = area < 0
    for A in (U, V):
        A[flip, 1], A[flip, 2] = A[flip, 2].copy(), A[flip, 1].copy()
    c = np.asarray(charts, np.int64)[chart[tex]]
    pad = max(grow, 0.0)
    u0 = np.maximum(np.ceil(U.min(1) - pad), c[:, 0]).astype(np.int64)
    u1 = np.minimum(np.floor(U.max(1) + pad), c[:, 0] + c[:, 2] - 1).astype(np.int64)
    v0 = np.maximum(np.ceil(V.min(1) - pad), c[:, 1]).astype(np.int64)
    v1 = np.minimum(np.floor(V.max(1) + pad), c[:, 1] + c[:, 3] - 1).astype(np.int64)
    bw, bh = u1 - u0 + 1, v1 - v0 + 1
    l0 = np.hypot(U[:, 2] - U[:, 1], V[:, 2] - V[:, 1])
    l1 = np.hypot(U[:, 0] - U[:, 2], V[:, 0] - V[:, 2])
    l2 = np.hypot(U[:, 1] - U[:, 0], V[:, 1] - V[:, 0])
    base = np.asarray(prefix, np.int64)[chart[tex]]
    for dv in range(int(bh.max()) if len(bh) else 0):
        for du in range(int(bw.max()) if len(bw) else 0):
            sel = np.nonzero((du < bw) & (dv < bh))[0]
            if len(sel) == 0:
                continue
            x, y = (u0[sel] + du).astype(np.float64), (v0[sel] + dv).astype(np.float64)
            Us, Vs = U[sel], V[sel]
            e0 = (Us[:, 2] - Us[:, 1]) * (y - Vs[:, 1]) - (Vs[:, 2] - Vs[:, 1]) * (x - Us[:, 1])
            e1 = (Us[:, 0] - Us[:, 2]) * (y - Vs[:, 2]) - (Vs[:, 0] - Vs[:, 2]) * (x - Us[:, 2])
            e2 = (Us[:, 1] - Us[:, 0]) * (y - Vs[:, 0]) - (Vs[:, 1] - Vs[:, 0]) * (x - Us[:, 0])
            cov = (e0 >= -grow * l0[sel]) & (e1 >= -grow * l1[sel]) & (e2 >= -grow * l2[sel])
            s = sel[cov]
            k = base[s] + (v0[s] + dv - c[s, 1]) * c[s, 2] + (u0[s] + du - c[s, 0])
            np.minimum.at(owner, k, tex[s])
    return owner


def dilate(owner, charts, prefix, rounds=BAND):
    """`rounds` double-buffered rounds: an unowned texel takes the owner of the first owned texel of its 3 x 3 neighbourhood
    inside the chart's box, in row-major order, of the previous round."""
    out = np.asarray(owner, np.int64).copy()
    for ci, c in enumerate(np.asarray(charts, np.int64)):
        w, h = int(c[2]), int(c[3])
        cur = out[prefix[ci]:prefix[ci + 1]].reshape(h, w)
        for _ in range(rounds):
            pad = np.full((h + 2, w + 2), UNOWNED, np.int64)
            pad[1:-1, 1:-1] = cur
            nxt = cur.copy()
            todo = cur == UNOWNED
            for dy in (0, 1, 2):
                for dx in (0, 1, 2):
                    nb = pad[dy:dy + h, dx:dx + w]
                    take = todo & (nb != UNOWNED)
                    nxt[take] = nb[take]
                    todo &= ~take
            cur = nxt
        out[prefix[ci]:prefix[ci + 1]] = cur.reshape(-1)
    return out


def texel_index(charts, prefix):
    """For every texel of the concatenated boxes: (chart, image x, image y, page, atlas x, atlas y)."""
    ci = np.repeat(np.arange(len(charts)), np.diff(prefix))
    c = np.asarray(charts, np.int64)[ci]
    local = np.arange(int(prefix[-1])) - np.asarray(prefix, np.int64)[ci]
    dx, dy = local % c[:, 2], local // c[:, 2]
    return ci, c[:, 0] + dx, c[:, 1] + dy, c[:, 6], c[:, 4] + dx, c[:, 5] + dy


def levelled_values(atlas, owner, uv, corner, g, charts, prefix):
    """-> (owned [texels] bool, value [owned texels, 3] float64 = texel + g interpolated in the owner's image triangle at the
    texel centre, clamped to the corners' [min, max], page, ax, ay of the owned texels) before rounding."""
    owned = owner != UNOWNED
    _, x, y, pg, ax, ay = (a[owned] for a in texel_index(charts, prefix))
    o = owner[owned]
    q = np.asarray(uv, np.float64)[o]
    area = (q[:, 2] - q[:, 0]) * (q[:, 5] - q[:, 1]) - (q[:, 3] - q[:, 1]) * (q[:, 4] - q[:, 0])
    e1 = (q[:, 0] - q[:, 4]) * (y - q[:, 5]) - (q[:, 1] - q[:, 5]) * (x - q[:, 4])
    e2 = (q[:, 2] - q[:, 0]) * (y - q[:, 1]) - (q[:, 3] - q[:, 1]) * (x - q[:, 0])
    b1, b2 = (e1 / area)[:, None], (e2 / area)[:, None]
    gk = np.asarray(g, np.float64)[corner[o]]                # [m, 3 corners, 3 channels]
    gi = gk[:, 0] + b1 * (gk[:, 1] - gk[:, 0]) + b2 * (gk[:, 2] - gk[:, 0])
    gi = np.clip(gi, gk.min(1), gk.max(1))
    return owned, atlas[pg, ay, ax].astype(np.float64) + gi, pg, ax, ay
