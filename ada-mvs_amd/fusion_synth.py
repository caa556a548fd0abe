"""Analytic synthetic scenes for the depth-map fusion (tests, tools/fusion_bench.py): a terrain plane with box buildings
seen by one nadir reference camera and oblique / near-nadir source cameras, laid out like a WHU-OMVS oblique rig.

Every depth is ray-cast in fp64, so the exact surface depth of any (sub-)pixel is known; each pixel also gets the id of
the planar face it sees (0 terrain, 1 + 5 k + j face j of box k: top, x0, x1, y0, y1).  Cameras use the axes of the
predict output folder (x right, y down, z forward): world point X = R_wc X_cam + C.  Coordinates are local; `offset`
shifts the whole scene (cameras and buildings) in world space, as real WHU-OMVS coordinates do (1e5 .. 1e6 m).
"""
import numpy as np

# (x0, x1, y0, y1, height) in metres around the scene centre; the terrain is z = 0
BOXES = ((-70.0, -25.0, -45.0, 5.0, 42.0), (18.0, 66.0, -72.0, -28.0, 27.0), (8.0, 52.0, 26.0, 81.0, 55.0),
         (-95.0, -52.0, 38.0, 92.0, 16.0), (-20.0, 4.0, 30.0, 48.0, 33.0))


def look_at(C, target):
    """R_wc (columns: camera x right, y down, z forward in world coordinates) of a camera at C looking at `target`."""
    f = np.asarray(target, np.float64) - np.asarray(C, np.float64)
    f /= np.linalg.norm(f)
    hint = np.array([0.0, 1.0, 0.0]) if abs(f[2]) > 0.99 else np.array([0.0, 0.0, 1.0])
    x = np.cross(hint, f) if abs(f[2]) > 0.99 else np.cross(f, hint)
    x /= np.linalg.norm(x)
    y = np.cross(f, x)
    return np.stack([x, y, f], 1)


def intrinsics(H, W, fov_scale=1.0):
    f = 1.85 * W * fov_scale
    return np.array([[f, 0.0, (W - 1) / 2.0 + 0.37], [0.0, f * 1.0003, (H - 1) / 2.0 - 0.21], [0.0, 0.0, 1.0]])


def make_cameras(H, W, n_src, src_sizes=None, offset=(0.0, 0.0, 0.0)):
    """Reference (index 0, nadir, 550 m above the terrain) + n_src sources: the first four oblique (N, E, S, W, 40 deg
    off nadir), further ones near-nadir around the reference.  src_sizes: optional [(Hs, Ws)] per source.
    -> list of dicts {K, R (R_wc), C (world), H, W}."""
    off = np.asarray(offset, np.float64)
    cams = [dict(K=intrinsics(H, W), R=look_at((0.0, 0.0, 550.0), (0.0, 0.0, 0.0)), C=np.array([0.0, 0.0, 550.0]), H=H, W=W)]
    for k in range(n_src):
        Hs, Ws = src_sizes[k] if src_sizes else (H, W)
        a = 0.5 * np.pi * k + 0.3 * (k // 4)
        if k < 4:
            C = np.array([380.0 * np.cos(a), 380.0 * np.sin(a), 460.0])
            tgt = np.array([20.0 * np.cos(a), 20.0 * np.sin(a), 0.0])
        else:
            r = 45.0 + 12.0 * (k % 3)
            C = np.array([r * np.cos(a + 0.7), r * np.sin(a + 0.7), 530.0 + 7.0 * (k % 5)])
            tgt = np.array([0.3 * C[0], 0.3 * C[1], 0.0])
        cams.append(dict(K=intrinsics(Hs, Ws, 0.9 if k < 4 else 1.0), R=look_at(C, tgt), C=C, H=Hs, W=Ws))
    for c in cams:
        c["C"] = c["C"] + off
        c["offset"] = off
    return cams


def cast(cam, u, v):
    """Exact depth (camera z) and face id of the surface seen through pixel coordinates (u, v) (arrays, any shape);
    inf / -1 where the ray misses everything."""
    u = np.asarray(u, np.float64)
    v = np.asarray(v, np.float64)
    Kinv = np.linalg.inv(cam["K"])
    ray_c = np.stack([Kinv[0, 0] * u + Kinv[0, 1] * v + Kinv[0, 2], Kinv[1, 0] * u + Kinv[1, 1] * v + Kinv[1, 2],
                      Kinv[2, 0] * u + Kinv[2, 1] * v + Kinv[2, 2]], -1)
    r = ray_c @ cam["R"].T                 # world direction per unit of camera depth
    C = cam["C"] - cam.get("offset", 0.0)
    best = np.full(u.shape, np.inf)
    face = np.full(u.shape, -1, np.int32)
    eps = 1e-9

    def consider(t, ok, fid):
        nonlocal best, face
        take = ok & (t > 0) & (t < best)
        best = np.where(take, t, best)
        face = np.where(take, fid, face)

    with np.errstate(divide="ignore", invalid="ignore"):
        t = -C[2] / r[..., 2]
        consider(t, np.isfinite(t), 0)
        for k, (x0, x1, y0, y1, h) in enumerate(BOXES):
            t = (h - C[2]) / r[..., 2]
            px, py = C[0] + t * r[..., 0], C[1] + t * r[..., 1]
            consider(t, (px >= x0 - eps) & (px <= x1 + eps) & (py >= y0 - eps) & (py <= y1 + eps), 1 + 5 * k)
            for j, (axis, val) in enumerate(((0, x0), (0, x1), (1, y0), (1, y1))):
                t = (val - C[axis]) / r[..., axis]
                pz = C[2] + t * r[..., 2]
                other = C[1 - axis] + t * r[..., 1 - axis]
                lo, hi = (y0, y1) if axis == 0 else (x0, x1)
                consider(t, (pz >= -eps) & (pz <= h + eps) & (other >= lo - eps) & (other <= hi + eps), 2 + 5 * k + j)
    return best, face


def render(cam):
    """-> (depth [H, W] fp64, face id [H, W] int32) at the pixel centres (integer coordinates)."""
    v, u = np.mgrid[0:cam["H"], 0:cam["W"]].astype(np.float64)
    return cast(cam, u, v)


def texture(cam, depth):
    """RGBA [H, W, 4] uint8 of the reference image: a pattern of the world position (local coordinates)."""
    v, u = np.mgrid[0:cam["H"], 0:cam["W"]].astype(np.float64)
    d = np.where(np.isfinite(depth), depth, 0.0)
    X = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(cam["K"]).T * d[..., None]
    P = X @ cam["R"].T + (cam["C"] - cam.get("offset", 0.0))
    rgba = np.empty(depth.shape + (4,), np.uint8)
    rgba[..., 0] = (np.floor(P[..., 0] * 3.1) % 256).astype(np.uint8)
    rgba[..., 1] = (np.floor(P[..., 1] * 2.3) % 256).astype(np.uint8)
    rgba[..., 2] = (np.floor(P[..., 2] * 5.7 + 40.0) % 256).astype(np.uint8)
    rgba[..., 3] = 255
    return rgba


def scene(H, W, n_src, src_sizes=None, offset=(0.0, 0.0, 0.0), seed=0):
    """A whole view set: cameras, fp32 depth maps (exact depths rounded to fp32; 0 where nothing is hit), confidences
    (seeded, ~90 % above 0.5), face ids and the reference RGBA image."""
    cams = make_cameras(H, W, n_src, src_sizes, offset)
    rng = np.random.default_rng(seed)
    depths, faces, confs = [], [], []
    for c in cams:
        d, f = render(c)
        depths.append(np.where(np.isfinite(d), d, 0.0).astype(np.float32))
        faces.append(f)
        confs.append(np.clip(rng.uniform(0.45, 1.0, d.shape), 0.0, 1.0).astype(np.float32))
    rgba = texture(cams[0], depths[0].astype(np.float64))
    return dict(cams=cams, depths=depths, confs=confs, faces=faces, rgba=rgba)


def write_predict_layout(sc, data, out):
    """The data-folder text files (poses in fp64, camera axes x right / y up as image_info.txt holds them) and predict's
    output folder (<vid>/<name>_init.pfm, _prob.pfm, <name>.txt through write_red_cam, RGBA <name>.jpg)."""
    import os

    from PIL import Image

    from .datasets.data_io import save_pfm, write_red_cam
    os.makedirs(data, exist_ok=True)
    flip = np.diag([1.0, -1.0, -1.0])
    n = len(sc["cams"])
    with open(os.path.join(data, "camera_info.txt"), "w") as f:
        for i, c in enumerate(sc["cams"]):
            f.write("%d %d %d 0.0046 %.17g %.17g %.17g %.17g 0 0 0 0 0\n" % (i, c["W"], c["H"], c["K"][0, 0], c["K"][1, 1], c["K"][0, 2], c["K"][1, 2]))
    with open(os.path.join(data, "image_info.txt"), "w") as f:
        for i, c in enumerate(sc["cams"]):
            R = c["R"] @ flip
            f.write("%d %d %s %s 300 800 %d/IMG_%04d.jpg\n" % (i, i, " ".join("%.17g" % v for v in R.reshape(-1)),
                                                            " ".join("%.17g" % v for v in c["C"]), i % 2, i))
    with open(os.path.join(data, "image_path.txt"), "w") as f:
        f.write("%d\n" % n + "".join("%d IMG_%04d /images/IMG_%04d.jpg\n" % (i, i, i) for i in range(n)))
    with open(os.path.join(data, "viewpair.txt"), "w") as f:
        f.write("%d\n" % n)
        for i in range(n):
            srcs = [j for j in range(n) if j != i]
            f.write("%d\n%d %s\n" % (i, len(srcs), " ".join("%d %.2f" % (j, 1.0 / (1 + j)) for j in srcs)))
    for i, c in enumerate(sc["cams"]):
        folder = os.path.join(out, str(i % 2))
        os.makedirs(folder, exist_ok=True)
        name = "IMG_%04d" % i
        save_pfm(os.path.join(folder, name + "_init.pfm"), sc["depths"][i])
        save_pfm(os.path.join(folder, name + "_prob.pfm"), sc["confs"][i])
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0, :3, :3] = c["R"].T
        cam[0, :3, 3] = -c["R"].T @ c["C"]
        cam[0, 3, 3] = 1
        cam[1, :3, :3] = c["K"]
        cam[1, 3] = (300, 2.6, 192, 800)
        write_red_cam(os.path.join(folder, name + ".txt"), cam, "/images/%s.jpg" % name)
        d = sc["depths"][i].astype(np.float64)
        with open(os.path.join(folder, name + ".jpg"), "wb") as f:
            Image.fromarray(texture(c, d)).save(f, format="png")
