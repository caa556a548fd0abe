"""fp64 numpy restatement of the depth-map fusion contract (ada_mvs_amd/fusion.py, csrc/fusion.hip): the CPU yardstick of
tests/test_fusion_*.py and of tools/fusion_bench.py's CPU baseline.

It follows the steps literally (back-project with K_r^-1, R_sr / t_sr from the poses, project with K_s, bilinear tap,
back-project in the source, R_rs / t_rs, project with K_r) and shares no code with the host layer.  Besides the decisions it
returns, per pixel, the smallest distance of any decision to its threshold, so that comparisons against the fp32 kernel
can leave ties out.
"""
import numpy as np


def restate(ref_depth, ref_conf, ref_cam, srcs, prob_threshold=0.5, pix_threshold=1.0, rel_depth_threshold=0.01,
            min_consistent=2, rgba=None, keep_uv=False):
    """ref_cam / srcs[i]["cam"]: {K, R (R_wc, x right / y down / z forward), C}; srcs[i]["depth"]: [Hs, Ws].
    -> dict: count [H, W] int, fused [H, W] fp64 (0 where rejected), kept [H, W] bool, pix_tie [H, W] (smallest
    |reprojection error - pix_threshold| over the sources whose taps were valid, px; +inf if none), depth_tie (smallest
    |depth error - rel d| / d), bound_tie (smallest distance of u, v to the bounds of the footprint test, px), and, when
    `rgba` is given, the points xyz [M, 3] fp64 / rgb [M, 3] uint8 in row-major order; keep_uv: u, v [N, H, W]."""
    d = np.asarray(ref_depth, np.float64)
    H, W = d.shape
    conf = np.asarray(ref_conf, np.float64)
    with np.errstate(invalid="ignore"):
        cand = np.isfinite(d) & (d > 0) & (conf >= prob_threshold)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    Kr, Rr, Cr = (np.asarray(ref_cam[k], np.float64) for k in ("K", "R", "C"))
    dd = np.where(cand, d, 0.0)
    ray = np.stack([x, y, np.ones_like(x)], -1) @ np.linalg.inv(Kr).T
    Xr = ray * dd[..., None]
    n = np.zeros((H, W), np.int64)
    acc = dd.copy()
    pix_tie = np.full((H, W), np.inf)
    depth_tie = np.full((H, W), np.inf)
    bound_tie = np.full((H, W), np.inf)
    uv = []
    for s in srcs:
        Ks, Rs, Cs = (np.asarray(s["cam"][k], np.float64) for k in ("K", "R", "C"))
        Ds = np.asarray(s["depth"], np.float64)
        Hs, Ws = Ds.shape
        R_sr = Rs.T @ Rr
        t_sr = Rs.T @ (Cr - Cs)
        Xs = Xr @ R_sr.T + t_sr
        zs = Xs[..., 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            ps = Xs @ Ks.T
            u, v = ps[..., 0] / ps[..., 2], ps[..., 1] / ps[..., 2]
            ok = cand & (zs > 0)
            bt = np.minimum(np.minimum(np.abs(u), np.abs(u - (Ws - 1))), np.minimum(np.abs(v), np.abs(v - (Hs - 1))))
            bound_tie = np.where(ok, np.minimum(bound_tie, bt), bound_tie)
            ok &= (u >= 0) & (u < Ws - 1) & (v >= 0) & (v < Hs - 1)
        if keep_uv:
            uv.append((u, v))
        ui, vi = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
        x0, y0 = np.floor(ui).astype(np.int64), np.floor(vi).astype(np.int64)
        ax, ay = ui - x0, vi - y0
        t00, t01 = Ds[y0, x0], Ds[y0, x0 + 1]
        t10, t11 = Ds[y0 + 1, x0], Ds[y0 + 1, x0 + 1]
        with np.errstate(invalid="ignore"):
            for t in (t00, t01, t10, t11):
                ok &= np.isfinite(t) & (t > 0)
        taps = [np.where(ok, t, 1.0) for t in (t00, t01, t10, t11)]
        ds = (1 - ay) * ((1 - ax) * taps[0] + ax * taps[1]) + ay * ((1 - ax) * taps[2] + ax * taps[3])
        Xs2 = np.stack([ui, vi, np.ones_like(ui)], -1) @ np.linalg.inv(Ks).T * ds[..., None]
        Xr2 = Xs2 @ R_sr + (Rr.T @ (Cs - Cr))           # R_rs = R_sr^T, t_rs = R_r^T (C_s - C_r)
        d2 = Xr2[..., 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            pr = Xr2 @ Kr.T
            ok &= d2 > 0
            err = np.hypot(pr[..., 0] / pr[..., 2] - x, pr[..., 1] / pr[..., 2] - y)
            derr = np.abs(d2 - dd)
            good = ok & (err < pix_threshold) & (derr < rel_depth_threshold * dd)
            pix_tie = np.where(ok, np.minimum(pix_tie, np.abs(err - pix_threshold)), pix_tie)
            depth_tie = np.where(ok, np.minimum(depth_tie, np.abs(derr - rel_depth_threshold * dd) / np.where(cand, dd, 1.0)), depth_tie)
        n += good
        acc += np.where(good, d2, 0.0)
    kept = cand & (n >= min_consistent)
    fused = np.where(kept, acc / (1 + n), 0.0)
    out = dict(count=n, fused=fused, kept=kept, pix_tie=pix_tie, depth_tie=depth_tie, bound_tie=bound_tie)
    if keep_uv:
        out["u"] = np.stack([a for a, _ in uv])
        out["v"] = np.stack([b for _, b in uv])
    if rgba is not None:
        idx = np.flatnonzero(kept.reshape(-1))
        P = ray.reshape(-1, 3)[idx] * fused.reshape(-1)[idx, None]
        out["xyz"] = P @ Rr.T + Cr
        out["rgb"] = np.asarray(rgba).reshape(-1, 4)[idx, :3].copy()
    return out


def pixel_margin(H, W, floor=1e-4):
    """Tie margin in px: 1e-4 px, or 8 fp32 spacings of the largest pixel coordinate where that is coarser (2.4e-4 px
    between 2048 and 4096: the fp32 kernel cannot place a reprojected pixel closer than that at the predict size)."""
    return max(floor, 8.0 * float(np.spacing(np.float32(max(H, W)))))


def ties(ref, pix_margin=None, rel_margin=1e-6):
    """Pixels whose decisions lie within the margins of a threshold (the fp32 kernel may decide them either way)."""
    if pix_margin is None:
        pix_margin = pixel_margin(*ref["count"].shape)
    return (ref["pix_tie"] < pix_margin) | (ref["depth_tie"] < rel_margin) | (ref["bound_tie"] < pix_margin)


# ---- analytic-scene helpers (ada_mvs_amd/fusion_synth.py) -------------------------------------------------------------
def visible_sources(sc):
    """Per reference pixel: how many sources see its surface point (inside the footprint test, not occluded)."""
    from ada_mvs_amd import fusion_synth
    ref_cam = sc["cams"][0]
    H, W = sc["depths"][0].shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d, _ = fusion_synth.render(ref_cam)
    d = np.where(np.isfinite(d), d, 0.0)
    X = (np.stack([x, y, np.ones_like(x)], -1) @ np.linalg.inv(ref_cam["K"]).T) * d[..., None] @ ref_cam["R"].T + ref_cam["C"]
    n = np.zeros((H, W), np.int64)
    for c in sc["cams"][1:]:
        p = (X - c["C"]) @ c["R"] @ c["K"].T
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v, z = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2], p[..., 2]
            inside = (z > 0) & (u >= 0) & (u < c["W"] - 1) & (v >= 0) & (v < c["H"] - 1)
        zt, _ = fusion_synth.cast(c, np.where(inside, u, 0.0), np.where(inside, v, 0.0))
        n += inside & (np.abs(zt - z) < 1e-6 * z)
    return n


def interior(sc, ref_out):
    """Pixels whose 3x3 neighbourhood lies on one planar face of the reference and whose 2x2 bilinear taps lie on that same
    face in every source whose footprint test they pass (ref_out: restate(..., keep_uv=True)).  Elsewhere a tap mixes two
    depths, or the source sees another face next to the point (an occluder within the thresholds)."""
    face = sc["faces"][0]
    H, W = face.shape
    flat = np.zeros((H, W), bool)
    flat[1:-1, 1:-1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            flat[1:-1, 1:-1] &= face[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] == face[1:-1, 1:-1]
    for s, fs in enumerate(sc["faces"][1:]):
        u, v = ref_out["u"][s], ref_out["v"][s]
        Hs, Ws = fs.shape
        with np.errstate(invalid="ignore"):
            inside = (u >= 0) & (u < Ws - 1) & (v >= 0) & (v < Hs - 1)
        x0 = np.floor(np.where(inside, u, 0.0)).astype(np.int64)
        y0 = np.floor(np.where(inside, v, 0.0)).astype(np.int64)
        same = ((fs[y0, x0] == face) & (fs[y0, x0 + 1] == face) & (fs[y0 + 1, x0] == face) & (fs[y0 + 1, x0 + 1] == face))
        flat &= ~inside | same
    return flat


def patch(H, W):
    """A block of terrain in a corner of the nadir reference, clear of the buildings (for the corrupted-depth tests)."""
    return slice(int(0.03 * H), int(0.19 * H)), slice(int(0.8 * W), int(0.975 * W))
