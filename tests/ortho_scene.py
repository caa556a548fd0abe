"""The analytic scene of ada_mvs_amd/fusion_synth.py prepared for the orthophoto tests: a DSM cast analytically at the cell
centres and images textured by world position (R, G) and face class (B)."""
import numpy as np

from ada_mvs_amd import dsm as dsm_mod, fusion_synth

TERRAIN, ROOF, WALL = 40, 130, 220


def tex_rg(x, y):
    """The smooth texture of world position: R of x and y, G of y and x (levels, fp64)."""
    return 128.0 + 90.0 * np.sin(x / 23.0 + 0.3 + 0.2 * np.sin(y / 41.0)), 128.0 + 90.0 * np.sin(y / 19.0 - 0.2 + 0.2 * np.sin(x / 37.0))


def cameras(H, W, n_src=4, offset=(0.0, 0.0, 0.0), src_sizes=None):
    """fusion_synth cameras with centres rounded to 2^-12 m, so that the scene shifted by an offset of whole metres has
    bit-identical differences X - C."""
    cams = fusion_synth.make_cameras(H, W, n_src, src_sizes, (0.0, 0.0, 0.0))
    off = np.asarray(offset, np.float64)
    for c in cams:
        c["C"] = np.round(c["C"] * 4096.0) / 4096.0 + off
        c["offset"] = off
    return cams


def box_heights(x, y):
    h = np.zeros(np.broadcast(x, y).shape)
    for x0, x1, y0, y1, bh in fusion_synth.BOXES:
        h = np.where((x >= x0) & (x <= x1) & (y >= y0) & (y <= y1), np.maximum(h, bh), h)
    return h


def dsm_grid(gsd=1.0, x0=-160.0, y_top=130.0, W=320, H=260, offset=(0.0, 0.0, 0.0)):
    """-> (dsm [H, W] float32 cast at the cell centres, dsm.Grid) of the scene (local coordinates shifted by offset)."""
    a, b = np.meshgrid(np.arange(W), np.arange(H))
    x, y = x0 + (a + 0.5) * gsd, y_top - (b + 0.5) * gsd
    g = dsm_mod.Grid(x0 + offset[0], y_top + offset[1], gsd, 0.0, W, H)
    return (box_heights(x, y) + offset[2]).astype(np.float32), g


def face_class(face):
    """fusion_synth face ids -> TERRAIN / ROOF / WALL codes (0 where nothing is hit)."""
    return np.where(face < 0, 0, np.where(face == 0, TERRAIN, np.where((face - 1) % 5 == 0, ROOF, WALL)))


def image(cam):
    """RGBA [H, W, 4] uint8: R, G = tex_rg of the surface point each pixel centre sees, B = its face class."""
    d, f = fusion_synth.render(cam)
    v, u = np.mgrid[0:cam["H"], 0:cam["W"]].astype(np.float64)
    dd = np.where(np.isfinite(d), d, 0.0)
    X = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(cam["K"]).T * dd[..., None]
    P = X @ cam["R"].T + (cam["C"] - cam["offset"])
    r, g = tex_rg(P[..., 0], P[..., 1])
    rgba = np.zeros(d.shape + (4,), np.uint8)
    hit = np.isfinite(d)
    rgba[..., 0] = np.where(hit, np.clip(np.floor(r + 0.5), 0, 255), 0)
    rgba[..., 1] = np.where(hit, np.clip(np.floor(g + 0.5), 0, 255), 0)
    rgba[..., 2] = face_class(f)
    rgba[..., 3] = 255
    return rgba


def views(cams, device=None):
    """[dict(iid, K, R, C, rgba)] (rgba on `device` if given, else host) with iid = index."""
    out = []
    for i, c in enumerate(cams):
        img = image(c)
        v = dict(iid=i, K=c["K"], R=c["R"], C=c["C"], rgba=img, cam=c)
        if device is not None:
            import torch
            v["rgba"] = torch.from_numpy(img).to(device)
            v["rgba_h"] = img
        out.append(v)
    return out


def terrain_check_cells(grid, K, margin_cells=2.0):
    """Cells whose centre is terrain more than margin_cells DSM cells from every box edge (local coordinates)."""
    g = grid.gsd / K
    xs = (grid.x0 + (np.arange(grid.W * K) + 0.5) * g)
    ys = (grid.y_top - (np.arange(grid.H * K) + 0.5) * g)
    X, Y = np.meshgrid(xs, ys)
    m = margin_cells * grid.gsd
    ok = np.ones(X.shape, bool)
    for x0, x1, y0, y1, _ in fusion_synth.BOXES:
        ok &= ~((X >= x0 - m) & (X <= x1 + m) & (Y >= y0 - m) & (Y <= y1 + m))
    return ok, X, Y


def neighbour_classes(cam, u, v):
    """Face classes of the four pixels a bilinear sample at (u, v) reads -> [.., 4]."""
    H, W = cam["H"], cam["W"]
    xa = np.floor(u).astype(np.int64)
    ya = np.floor(v).astype(np.int64)
    xb, yb = np.minimum(xa + 1, W - 1), np.minimum(ya + 1, H - 1)
    out = []
    for px, py in ((xa, ya), (xb, ya), (xa, yb), (xb, yb)):
        _, f = fusion_synth.cast(cam, px.astype(np.float64), py.astype(np.float64))
        out.append(face_class(f))
    return np.stack(out, -1)


def hidden_from(cam, X, Y, Z):
    """Terrain points (local coordinates) the camera does not see: the surface its ray meets first is elsewhere."""
    Cl = cam["C"] - cam["offset"]
    d = np.stack([X - Cl[0], Y - Cl[1], Z - Cl[2]], -1)
    p = d @ cam["R"]
    u = (cam["K"][0, 0] * p[..., 0] + cam["K"][0, 1] * p[..., 1] + cam["K"][0, 2] * p[..., 2]) / p[..., 2]
    v = (cam["K"][1, 1] * p[..., 1] + cam["K"][1, 2] * p[..., 2]) / p[..., 2]
    inside = (u >= 0) & (u <= cam["W"] - 1) & (v >= 0) & (v <= cam["H"] - 1)
    depth, f = fusion_synth.cast(cam, u, v)
    return inside & ((f != 0) | (np.abs(depth - p[..., 2]) > 1e-6 * p[..., 2]))



def segment_hits_boxes(P, C, grow):
    """Whether the open segment from points P [.., 3] to C [3] (local coordinates) meets a box of the scene with its footprint
    grown by `grow` metres (negative: shrunk).  The DSM at gsd g is a solid between the boxes shrunk by g and grown by g, so a
    segment that misses every box grown by g is clear in the scene and in the DSM, and one that meets a box shrunk by g is
    blocked in both."""
    P = np.asarray(P, np.float64)
    D = np.asarray(C, np.float64) - P
    hit = np.zeros(P.shape[:-1], bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for x0, x1, y0, y1, h in fusion_synth.BOXES:
            lo = np.array([x0 - grow, y0 - grow, 0.0])
            hi = np.array([x1 + grow, y1 + grow, h])
            t0 = np.full(P.shape[:-1], 1e-9)
            t1 = np.ones(P.shape[:-1])
            for a in range(3):
                ta, tb = (lo[a] - P[..., a]) / D[..., a], (hi[a] - P[..., a]) / D[..., a]
                par = D[..., a] == 0
                inside_slab = (P[..., a] >= lo[a]) & (P[..., a] <= hi[a])
                tn, tf = np.minimum(ta, tb), np.maximum(ta, tb)
                t0 = np.where(par, np.where(inside_slab, t0, np.inf), np.maximum(t0, tn))
                t1 = np.where(par, np.where(inside_slab, t1, -np.inf), np.minimum(t1, tf))
            hit |= t0 <= t1
    return hit
