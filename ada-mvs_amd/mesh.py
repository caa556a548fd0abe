"""TSDF meshing: the fused depth maps of all views integrated into a truncated signed-distance field on a voxel grid, brick by
brick on the GPU, and its zero level set extracted as a coloured triangle mesh (marching tetrahedra, also on the GPU).

    python mesh_whu.py --data_folder <whu-omvs data> --output_folder <predict output> [--ply fused.ply] [--voxel 0.25] [--trunc 4]
                       [--min_weight 1] [--depth fused|init] [--bounds XMIN YMIN ZMIN XMAX YMAX ZMAX] [--brick 128]
                       [--out <output_folder>/mesh.ply] [--weld]

The step after fuse_whu.py.  The volume spans the fused PLY's points padded by mu = trunc * voxel (or --bounds); it is cut into
bricks of B^3 voxels, and a brick is ACTIVE iff a fused point lies in its box grown by mu (found on the GPU, chunk by chunk).
Per active brick: the views are culled by a conservative fp64 frustum test against the grown box, then csrc/mesh.hip
integrates the depth maps (`<vid>/<name>_fused.pfm`, or `_init.pfm` with --depth init) and extracts the mesh
(include/adamvs_hip.h "TSDF mesh" states every operation).  The mesh is streamed to a binary little-endian PLY (vertices
double x y z, uchar red green blue as fuse_whu.py writes them; faces list uchar uint vertex_indices): vertices are written in
place, faces spooled to a temporary file next to the output and appended at the end, and both counts are patched in.
`<out>.json` records the volume, the counts and the timings.  clean_whu.py (ada_mvs_amd/clean.py) is the step after this one.

Seam vertices between bricks are written by each brick that uses them, at bit-identical coordinates; --weld merges them by
exact position on the GPU (it holds the whole mesh on the device).  Precision: camera-frame arithmetic is fp32 relative to the
volume origin O, so cameras and bricks must lie within 16384 m of it (MAX_EXTENT); positions are fp64.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

from . import fusion
from .dsm import ply_chunks, ply_layout, point_bounds

BRICKS = (32, 64, 128)
MAX_EXTENT = 16384.0               # ADAMVS_MESH_MAX_EXTENT, metres
MAX_VIEWS = 65535                  # ADAMVS_MESH_MAX_VIEWS
MAX_VERTICES = (1 << 32) - 1
DEPTHS = {"fused": "_fused.pfm", "init": "_init.pfm"}
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<u4", (3,))])
_COUNT_DIGITS = 10


# ---- the mesh PLY, streamed ---------------------------------------------------------------------------------------------------
def mesh_ply_header(nv, nf):
    """Header of the binary mesh PLY; both counts zero-padded to a fixed width so that they can be patched in place."""
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %0*d\nproperty double x\nproperty double y\nproperty double z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %0*d\nproperty list uchar uint vertex_indices\n"
            "end_header\n" % (_COUNT_DIGITS, nv, _COUNT_DIGITS, nf)).encode("ascii")


class MeshPlyWriter:
    """Vertices go straight into the PLY, faces into a spool file next to it; close() appends the faces and patches the counts."""

    def __init__(self, path):
        self.path = path
        self.spool_path = path + ".faces.tmp"
        self.vertices = self.faces = 0
        self.f = open(path, "wb")
        self.f.write(mesh_ply_header(0, 0))
        self.spool = open(self.spool_path, "wb")

    def write(self, xyz, rgb, faces):
        """xyz [n, 3] float64, rgb [n, 3] uint8, faces [m, 3] uint32 (global indices), numpy."""
        n, m = len(xyz), len(faces)
        if self.vertices + n > MAX_VERTICES:
            raise ValueError("mesh: more than %d vertices" % MAX_VERTICES)
        if self.faces + m >= 10 ** _COUNT_DIGITS:
            raise ValueError("mesh: more than %d faces" % (10 ** _COUNT_DIGITS - 1))
        if n:
            rec = np.empty(n, fusion.PLY_DTYPE)
            rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
            rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
            self.f.write(rec.tobytes())
        if m:
            rec = np.empty(m, FACE_DTYPE)
            rec["n"] = 3
            rec["v"] = faces
            self.spool.write(rec.tobytes())
        self.vertices += n
        self.faces += m

    def close(self):
        if self.f is None:
            return
        self.spool.close()
        with open(self.spool_path, "rb") as s:
            while True:
                buf = s.read(1 << 24)
                if not buf:
                    break
                self.f.write(buf)
        os.remove(self.spool_path)
        self.f.seek(0)
        self.f.write(mesh_ply_header(self.vertices, self.faces))
        self.f.close()
        self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def read_mesh_ply(path):
    """-> (vertices: structured array of fusion.PLY_DTYPE, faces [m, 3] uint32) of a file MeshPlyWriter wrote."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[2])
    verts = np.frombuffer(data, fusion.PLY_DTYPE, count=nv, offset=end)
    faces = np.frombuffer(data, FACE_DTYPE, count=nf, offset=end + nv * fusion.PLY_DTYPE.itemsize)
    if nf and not (faces["n"] == 3).all():
        raise ValueError("%s: a face is not a triangle" % path)
    return verts, faces["v"].copy()


# ---- volume ---------------------------------------------------------------------------------------------------------------------
def brick_box(origin, voxel, B, b, grow=0.0):
    """(lo, hi) fp64 of brick b's closed box, grown by `grow` on every side."""
    lo = np.asarray(origin, np.float64) + np.asarray(b, np.float64) * (B * voxel) - grow
    return lo, lo + B * voxel + 2.0 * grow


def cull_views(lo, hi, cams, margin_px=2.0):
    """Conservative view list of the box [lo, hi] in fp64: cams = [(K, R_wc, C, H, W)].  A view is left out only if the box lies
    wholly behind it (every corner at z < -tol) or wholly in front of it with every corner projecting outside the image grown by
    margin_px (the perspective image of a box in front of the camera is the convex hull of its corners' images)."""
    corners = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
    keep = []
    for i, (K, R_wc, C, H, W) in enumerate(cams):
        rel = corners - np.asarray(C, np.float64)
        p = rel @ np.asarray(R_wc, np.float64)          # rows: R_cw (X - C)
        z = p[:, 2]
        tol = 1e-5 * (np.abs(rel).max() + 1.0)
        if z.max() < -tol:
            continue
        if z.min() > tol:
            K = np.asarray(K, np.float64)
            u = (p @ K[0]) / z
            v = (p @ K[1]) / z
            if u.max() < -0.5 - margin_px or u.min() > W - 0.5 + margin_px or v.max() < -0.5 - margin_px or v.min() > H - 0.5 + margin_px:
                continue
        keep.append(i)
    return keep


class TsdfMesher:
    """One volume (origin O, voxel s, truncation mu, brick size B) over a fixed list of views on the device.
    views: [dict(K [3, 3], R (R_wc, camera x right / y down / z forward -> world), C (world), depth [H, W] fp32, rgba [H, W, 4]
    uint8)]; depth and rgba device tensors."""

    def __init__(self, origin, voxel, mu, brick, views, min_weight=1, device=None):
        import torch
        from . import hip_ops
        if brick not in BRICKS:
            raise ValueError("brick %r: one of %s" % (brick, BRICKS))
        for name, v in (("voxel", voxel), ("mu", mu)):
            if not (math.isfinite(float(v)) and float(v) > 0):
                raise ValueError("%s=%r must be finite and > 0" % (name, v))
        if not 1 <= int(min_weight) <= 65535:
            raise ValueError("min_weight=%r (1 .. 65535)" % min_weight)
        if not 1 <= len(views) <= MAX_VIEWS:
            raise ValueError("%d views (1 .. %d)" % (len(views), MAX_VIEWS))
        self.origin = np.asarray(origin, np.float64)
        self.voxel, self.mu, self.B, self.min_weight = float(voxel), float(mu), int(brick), int(min_weight)
        self.device = torch.device(device if device is not None else views[0]["depth"].device)
        self.views = views
        recs = []
        for v in views:
            c = np.asarray(v["C"], np.float64) - self.origin
            if not (np.abs(c) <= MAX_EXTENT).all():
                raise ValueError("a camera lies %.1f m from the volume origin (at most %g m)" % (np.abs(c).max(), MAX_EXTENT))
            recs.append((np.asarray(v["K"], np.float64), np.asarray(v["R"], np.float64).T, c, v["depth"], v["rgba"]))
        self.views_dev = hip_ops.mesh_views(recs, self.device)
        self.cams = [(np.asarray(v["K"], np.float64), np.asarray(v["R"], np.float64), np.asarray(v["C"], np.float64)) + tuple(v["depth"].shape)
                     for v in views]

    def brick_desc(self, b):
        from . import hip_ops
        return hip_ops.mesh_brick(self.origin, self.voxel, self.mu, self.B, b, self.min_weight)

    def view_list(self, b):
        lo, hi = brick_box(self.origin, self.voxel, self.B, b, self.mu)
        return cull_views(lo, hi, self.cams)

    def integrate(self, b, view_list=None):
        """-> (tsdf, weight, rgba) of brick b (device, [(B+1)^3]; hip_ops.tsdf_integrate)."""
        import torch
        from . import hip_ops
        vl = self.view_list(b) if view_list is None else list(view_list)
        lst = torch.tensor(vl if vl else [0], dtype=torch.int32)[:len(vl)].to(self.device)
        return hip_ops.tsdf_integrate(self.brick_desc(b), self.views_dev, len(self.views), lst)

    def extract(self, b, vol, vertex_base=0):
        """vol = (tsdf, weight, rgba) of brick b -> (xyz, rgb, faces) on the device (hip_ops.mesh_extract)."""
        from . import hip_ops
        return hip_ops.mesh_extract(self.brick_desc(b), *vol, vertex_base=vertex_base)

    def brick(self, b, vertex_base=0):
        """Integrate and extract brick b -> (xyz [nv, 3] float64, rgb [nv, 3] uint8, faces [nt, 3] int32 (uint32)), device tensors."""
        return self.extract(b, self.integrate(b), vertex_base)


def weld(xyz, faces, rgb=None):
    """Exact-position weld on the device: -> (xyz unique rows in lexicographic order, faces remapped[, rgb]).  Seam vertices
    that neighbouring bricks both wrote carry the same bits (and colour), so they merge."""
    import torch
    u, inv = torch.unique(xyz, dim=0, return_inverse=True)
    f = inv.to(torch.int64)[faces.to(torch.int64) & 0xFFFFFFFF]
    if rgb is None:
        return u, f
    out = torch.empty(u.shape[0], 3, device=rgb.device, dtype=rgb.dtype)
    out[inv] = rgb
    return u, f, out


# ---- a predict output folder ------------------------------------------------------------------------------------------------
def grid_for_bounds(lo, hi, voxel, B):
    """-> (origin = lo, bricks per axis (3,)) covering [lo, hi]; refuses a volume reaching past MAX_EXTENT from its origin."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError("bounds lo %r, hi %r" % (lo, hi))
    cubes = np.maximum(np.ceil((hi - lo) / voxel), 1).astype(np.int64)
    nb = (cubes + B - 1) // B
    if (nb * B * voxel > MAX_EXTENT).any():
        raise ValueError("a volume of %s m at voxel %g exceeds %g m along an axis: crop with --bounds or raise --voxel"
                         % (tuple(np.round(hi - lo, 1)), voxel, MAX_EXTENT))
    return lo, nb


def active_bricks(chunks, origin, voxel, mu, B, nb, device):
    """Bricks whose box grown by mu holds a point (x - O in [b L - mu, (b + 1) L + mu] per axis, L = B s), on the device;
    chunks: iterable of point tensors [n, 3] float64 -> [(bx, by, bz)] in brick row-major order (x fastest)."""
    import torch
    L = B * voxel
    nbt = torch.as_tensor(nb, device=device)
    hit = torch.zeros(int(nb[2]), int(nb[1]), int(nb[0]), dtype=torch.bool, device=device)
    O = torch.as_tensor(origin, dtype=torch.float64, device=device)
    for xyz in chunks:
        t = torch.as_tensor(xyz).to(device) - O
        t = t[torch.isfinite(t).all(1)]
        lo = torch.ceil((t - mu) / L).to(torch.int64) - 1
        hi = torch.floor((t + mu) / L).to(torch.int64)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    b = lo + torch.tensor([dx, dy, dz], device=device)
                    ok = (b <= hi).all(1) & (b >= 0).all(1) & (b < nbt).all(1)
                    b = b[ok]
                    hit[b[:, 2], b[:, 1], b[:, 0]] = True
    idx = torch.nonzero(hit).cpu().numpy()            # row-major (z, y, x)
    return [(int(x), int(y), int(z)) for z, y, x in idx]


def load_views(folder, depth, device):
    """Every view of the folder with its depth map, camera and image -> [dict(iid, K, R, C, depth, rgba)] in image-id order."""
    import torch
    from PIL import Image
    from .datasets.data_io import read_pfm
    views = []
    for iid in sorted(folder.images):
        base = folder.base(iid)
        if not all(os.path.exists(base + ext) for ext in (DEPTHS[depth], ".txt", ".jpg")):
            continue
        d = np.ascontiguousarray(read_pfm(base + DEPTHS[depth])[0], dtype=np.float32)
        _, K = fusion.read_cam_txt(base + ".txt")
        rgba = np.ascontiguousarray(np.array(Image.open(base + ".jpg").convert("RGBA")))
        if rgba.shape[:2] != d.shape:
            raise ValueError("view %d: depth %s and image %s differ in size" % (iid, d.shape, rgba.shape[:2]))
        R, C = fusion.pose(folder.images[iid])
        views.append(dict(iid=iid, K=K, R=R, C=C, depth=torch.from_numpy(d).to(device), rgba=torch.from_numpy(rgba).to(device)))
    return views


def from_folder(data_folder, output_folder, ply=None, voxel=0.25, trunc=4.0, min_weight=1, depth="fused", bounds=None, brick=128,
                out=None, weld_mesh=False, chunk=1 << 22, device=None, log=print):
    """The whole chain step: -> the summary dict also written to <out>.json."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("mesh: needs an MI355X (there is no CPU fallback for the mesh kernels)")
    if depth not in DEPTHS:
        raise ValueError("depth %r: one of %s" % (depth, sorted(DEPTHS)))
    if brick not in BRICKS:
        raise ValueError("brick %r: one of %s" % (brick, BRICKS))
    voxel, trunc = float(voxel), float(trunc)
    if not (math.isfinite(voxel) and voxel > 0 and math.isfinite(trunc) and trunc > 0):
        raise ValueError("voxel %r and trunc %r must be finite and > 0" % (voxel, trunc))
    mu = trunc * voxel
    device = torch.device(device if device is not None else "cuda")
    t_start = time.time()
    ply = ply or os.path.join(output_folder, "fused.ply")
    out = out or os.path.join(output_folder, "mesh.ply")
    ply_layout(ply)
    if bounds is not None:
        lo, hi = np.asarray(bounds[:3], np.float64), np.asarray(bounds[3:], np.float64)
    else:
        lo, hi = point_bounds(ply, chunk, device)
        if not np.isfinite(lo).all():
            raise ValueError("%s: no point with finite coordinates" % ply)
        lo, hi = lo - mu, hi + mu
    origin, nb = grid_for_bounds(lo, hi, voxel, brick)
    folder = fusion.Folder(data_folder, output_folder)
    views = load_views(folder, depth, device)
    if not views:
        raise ValueError("%s: no view has %s maps" % (output_folder, DEPTHS[depth]))
    mesher = TsdfMesher(origin, voxel, mu, brick, views, min_weight, device)
    active = active_bricks((xyz for xyz, _ in ply_chunks(ply, chunk)), origin, voxel, mu, brick, nb, device)
    log("mesh: volume %d x %d x %d bricks of %d^3 voxels at %g m (mu %g m), %d active, %d views"
        % (nb[0], nb[1], nb[2], brick, voxel, mu, len(active), len(views)))
    events = []
    parts = []
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    nv = nf = 0
    with MeshPlyWriter(out) as w:
        for b in active:
            vl = mesher.view_list(b)
            if not vl:
                continue
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            vol = mesher.integrate(b, vl)
            e1.record()
            xyz, rgb, faces = mesher.extract(b, vol, 0 if weld_mesh else nv)
            e2.record()
            events.append((e0, e1, e2))
            if weld_mesh:
                parts.append((xyz, rgb, faces.to(torch.int64) + nv))
            else:
                w.write(xyz.cpu().numpy(), rgb.cpu().numpy(), faces.cpu().numpy().view(np.uint32))
            nv += xyz.shape[0]
            nf += faces.shape[0]
            if nv > MAX_VERTICES:
                raise ValueError("mesh: more than %d vertices" % MAX_VERTICES)
        if weld_mesh and parts:
            xyz, f, rgb = weld(torch.cat([p[0] for p in parts]), torch.cat([p[2] for p in parts]), torch.cat([p[1] for p in parts]))
            w.write(xyz.cpu().numpy(), rgb.cpu().numpy(), f.cpu().numpy().astype(np.uint32))
        nv, nf = w.vertices, w.faces
    torch.cuda.synchronize(device)
    t_int = sum(a.elapsed_time(b) for a, b, _ in events) / 1e3
    t_ext = sum(b.elapsed_time(c) for _, b, c in events) / 1e3
    S = (brick + 1) ** 3
    res = dict(voxel=voxel, mu=mu, min_weight=int(min_weight), depth=depth, origin=[float(v) for v in origin],
               grid=[int(v) * brick for v in nb], brick=brick, bricks_total=int(np.prod(nb)), bricks_active=len(active),
               bricks_meshed=len(events), views=len(views), vertices=int(nv), faces=int(nf), welded=bool(weld_mesh),
               seconds=time.time() - t_start, device_seconds=t_int + t_ext, integrate_seconds=t_int, extract_seconds=t_ext,
               device_bytes=int(sum(v["depth"].numel() * 8 for v in views) + S * 11 + brick ** 3 * 4), ply=out)
    with open(out + ".json", "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    log("mesh: %d vertices, %d faces from %d bricks into %s, device %.3f s, total_time = %.3f s"
        % (nv, nf, len(events), out, res["device_seconds"], res["seconds"]))
    return res


def build_parser():
    ap = argparse.ArgumentParser(description="Integrate the fused depth maps into a TSDF volume and extract a coloured triangle mesh")
    ap.add_argument("--data_folder", required=True, help="the whu-omvs data folder predict_whu.py read")
    ap.add_argument("--output_folder", required=True, help="predict_whu.py's output folder, after fuse_whu.py")
    ap.add_argument("--ply", default=None, help="fused point cloud (default <output_folder>/fused.ply): the volume's bounds and active bricks")
    ap.add_argument("--voxel", type=float, default=0.25, help="voxel size in metres")
    ap.add_argument("--trunc", type=float, default=4.0, help="truncation mu in voxels")
    ap.add_argument("--min_weight", type=int, default=1, help="a cube is meshed iff its 8 corners have at least this many views")
    ap.add_argument("--depth", choices=sorted(DEPTHS), default="fused", help="fused: <name>_fused.pfm (fuse_whu.py); init: <name>_init.pfm")
    ap.add_argument("--bounds", type=float, nargs=6, metavar=("XMIN", "YMIN", "ZMIN", "XMAX", "YMAX", "ZMAX"), default=None,
                    help="volume to mesh (default: the fused points padded by mu)")
    ap.add_argument("--brick", type=int, choices=BRICKS, default=128, help="brick size in voxels")
    ap.add_argument("--out", default=None, help="mesh PLY to write (default <output_folder>/mesh.ply); the summary goes to <out>.json")
    ap.add_argument("--weld", action="store_true", help="merge the seam vertices of neighbouring bricks (holds the whole mesh on the GPU)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    return from_folder(args.data_folder, args.output_folder, args.ply, args.voxel, args.trunc, args.min_weight, args.depth, args.bounds,
                       args.brick, args.out, args.weld)


if __name__ == "__main__":
    main()
