"""Depth-map fusion: geometric-consistency filtering of a predict output folder and one fused point cloud.

    python fuse_whu.py --data_folder <whu-omvs predict data> --output_folder <predict_whu.py's output folder> [--ply out.ply]

The step after predict_whu.py (the reference stops at writing the maps, predict_whu.py "step1").  Per reference view of
`viewpair.txt` (at most `num_src` of its listed sources, duplicates removed, no padding): the view's `<vid>/<name>_init.pfm`
and `_prob.pfm` are checked against the sources' depth maps on the GPU (csrc/fusion.hip; include/adamvs_hip.h "depth-map
fusion" states the test), and every kept pixel becomes a world point coloured from `<vid>/<name>.jpg`.  Written:
`<vid>/<name>_fused.pfm` (fused depth, 0 where rejected), `<vid>/mask/<name>_final.png` (0 / 255) and one binary
little-endian PLY (double x y z, uchar red green blue), streamed view by view.

Precision: WHU-OMVS camera centres are world coordinates of 1e5 .. 1e6 m and the `<name>.txt` cameras are fp32.  The poses
therefore come from image_info.txt in fp64; the relative transforms between cameras are formed here in fp64 (camera-frame
magnitudes are depths and baselines, so the kernel takes them in fp32), and the camera -> world step runs in fp64 in the
emit kernel.  Intrinsics come from each view's `<name>.txt` (predict's scale and crop included).
"""
import argparse
import os
import sys
import time
from collections import OrderedDict

import numpy as np

from .datasets.data_io import read_cameras_text, read_images_path_text, read_images_text, read_pfm, read_view_pair_text, save_pfm

# camera axes of image_info.txt (x right, y up, z back) -> those of the predict output folder (x right, y down, z forward)
_FLIP_YZ = np.diag([1.0, -1.0, -1.0])

PLY_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_PLY_COUNT_DIGITS = 10


def ply_header(count):
    """Header of the binary PLY; the vertex count is zero-padded to a fixed width so that it can be patched in place."""
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %0*d\nproperty double x\nproperty double y\nproperty double z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % (_PLY_COUNT_DIGITS, count)).encode("ascii")


class PlyWriter:
    """Streams points into a binary little-endian PLY chunk by chunk; the vertex count is written on close()."""

    def __init__(self, path):
        self.path = path
        self.count = 0
        self.f = open(path, "wb")
        self.f.write(ply_header(0))

    def write(self, xyz, rgb):
        """xyz [n, 3] float64, rgb [n, 3] uint8 (numpy)."""
        n = len(xyz)
        if n == 0:
            return
        if self.count + n >= 10 ** _PLY_COUNT_DIGITS:
            raise ValueError("PLY: more than %d points" % (10 ** _PLY_COUNT_DIGITS - 1))
        rec = np.empty(n, PLY_DTYPE)
        rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
        self.f.write(rec.tobytes())
        self.count += n

    def close(self):
        if self.f is None:
            return
        self.f.seek(0)
        self.f.write(ply_header(self.count))
        self.f.close()
        self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def read_ply(path):
    """-> structured array of PLY_DTYPE (files written by PlyWriter)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    count = int([ln for ln in data[:end].decode("ascii").splitlines() if ln.startswith("element vertex")][0].split()[2])
    return np.frombuffer(data[end:], PLY_DTYPE, count=count)


def read_cam_txt(path):
    """<name>.txt of the predict output folder (datasets/data_io.py::write_red_cam) -> (extrinsic [4, 4], K [3, 3]) fp64."""
    with open(path) as f:
        lines = [ln.split() for ln in f.read().splitlines()]
    ext = np.array([[float(v) for v in lines[1 + i]] for i in range(4)])
    K = np.array([[float(v) for v in lines[7 + i]] for i in range(3)])
    return ext, K


def pose(photo):
    """image_info.txt record (datasets/data_io.py::Photo) -> (R_wc, C) fp64 in the output folder's camera axes."""
    return np.asarray(photo.rotation_matrix, np.float64) @ _FLIP_YZ, np.asarray(photo.project_center, np.float64)


def relative_transforms(K_r, R_r, C_r, K_s, R_s, C_s):
    """fp64 -> (fwd [12], back [12]) as include/adamvs_hip.h's adamvs_fusion_source takes them.
    R_sr = R_s^T R_r, t_sr = R_s^T (C_r - C_s); R_rs = R_sr^T, t_rs = R_r^T (C_s - C_r): only differences of camera centres
    enter, so the result keeps fp64 accuracy however large the world coordinates are."""
    K_r, R_r, C_r, K_s, R_s, C_s = (np.asarray(a, np.float64) for a in (K_r, R_r, C_r, K_s, R_s, C_s))
    R_sr = R_s.T @ R_r
    t_sr = R_s.T @ (C_r - C_s)
    R_rs = R_sr.T
    t_rs = R_r.T @ (C_s - C_r)
    fwd = np.concatenate([(K_s @ R_sr @ np.linalg.inv(K_r)).reshape(-1), K_s @ t_sr])
    back = np.concatenate([(K_r @ R_rs @ np.linalg.inv(K_s)).reshape(-1), K_r @ t_rs])
    return fwd, back


def emit_camera(K, R_wc, C):
    """21 doubles {K^-1, R_wc, C} of adamvs_fusion_emit."""
    return np.concatenate([np.linalg.inv(np.asarray(K, np.float64)).reshape(-1), np.asarray(R_wc, np.float64).reshape(-1),
                           np.asarray(C, np.float64)])


def view_pairs(pair_path, num_src):
    """viewpair.txt -> [(ref, [src, ...])]: at most num_src listed sources per reference, first occurrence of each kept,
    the reference itself left out, no padding (read_view_pair_text pads only for inference; view_num = 0 turns that off)."""
    out = []
    for row in read_view_pair_text(pair_path, 0):
        ref, seen = row[0], []
        for s in row[1:]:
            if s != ref and s not in seen:
                seen.append(s)
        out.append((ref, seen[:num_src]))
    return out


def view_key(photo):
    """image id -> predict's `<vid>`, `<name>` (the NAME field, as datasets/predict_oblique.py forms out_view / out_name)."""
    return os.path.dirname(photo.name).split("/")[-1], os.path.splitext(os.path.basename(photo.name))[0]


class Folder:
    """The data folder's text files and predict's output folder."""

    def __init__(self, data_folder, output_folder):
        self.images = read_images_text(os.path.join(data_folder, "image_info.txt"))
        self.cameras = read_cameras_text(os.path.join(data_folder, "camera_info.txt"))
        self.paths, _ = read_images_path_text(os.path.join(data_folder, "image_path.txt"))
        self.pair_path = os.path.join(data_folder, "viewpair.txt")
        self.output_folder = output_folder

    def base(self, iid):
        vid, name = view_key(self.images[iid])
        return os.path.join(self.output_folder, vid, name)

    def has_maps(self, iid):
        return iid in self.images and all(os.path.exists(self.base(iid) + ext) for ext in ("_init.pfm", ".txt"))

    def plan(self, num_src):
        """-> [(ref, [src, ...]) with the maps present], [skipped refs]"""
        views, skipped = [], []
        for ref, srcs in view_pairs(self.pair_path, num_src):
            if ref not in self.images or not (self.has_maps(ref) and os.path.exists(self.base(ref) + "_prob.pfm")
                                              and os.path.exists(self.base(ref) + ".jpg")):
                skipped.append(ref)
                continue
            views.append((ref, [s for s in srcs if s in self.images and self.has_maps(s)]))
        return views, skipped


class _MapCache:
    """Bounded LRU cache of device depth maps and their cameras (neighbouring views share most sources)."""

    def __init__(self, folder, device, capacity):
        self.folder, self.device, self.capacity = folder, device, capacity
        self.entries = OrderedDict()
        self.io_seconds = 0.0

    def get(self, iid):
        import torch
        if iid in self.entries:
            self.entries.move_to_end(iid)
            return self.entries[iid]
        t0 = time.time()
        b = self.folder.base(iid)
        depth = np.ascontiguousarray(read_pfm(b + "_init.pfm")[0], dtype=np.float32)
        _, K = read_cam_txt(b + ".txt")
        self.io_seconds += time.time() - t0
        R, C = pose(self.folder.images[iid])
        entry = dict(depth=torch.from_numpy(depth).to(self.device), K=K, R=R, C=C)
        self.entries[iid] = entry
        while len(self.entries) > self.capacity:
            self.entries.popitem(last=False)
        return entry


def fuse_view(ref, srcs, conf, rgba, prob_threshold=0.5, pix_threshold=1.0, rel_depth_threshold=0.01, min_consistent=2, buffers=None):
    """One reference view on the GPU.  ref / srcs[i]: {depth (device [H, W] fp32), K, R (R_wc), C}; conf: device [H, W] fp32;
    rgba: device [H, W, 4] uint8.  -> (count, fused (device maps), xyz [M, 3] float64, rgb [M, 3] uint8 (device, row-major))."""
    from . import hip_ops
    sources = []
    for s in srcs:
        fwd, back = relative_transforms(ref["K"], ref["R"], ref["C"], s["K"], s["R"], s["C"])
        sources.append((s["depth"], fwd, back))
    count, fused, block_kept = hip_ops.geo_consistency(ref["depth"], conf, sources, prob_threshold, pix_threshold, rel_depth_threshold,
                                                       min_consistent)
    xyz, rgb = (None, None) if buffers is None else buffers
    xyz, rgb, offsets = hip_ops.emit_points(fused, block_kept, rgba, emit_camera(ref["K"], ref["R"], ref["C"]), xyz, rgb)
    total = int(offsets[-1].item())
    return count, fused, xyz[:total], rgb[:total]


def fuse_folder(data_folder, output_folder, ply_path=None, prob_threshold=0.5, pix_threshold=1.0, rel_depth_threshold=0.01,
                min_consistent=2, num_src=4, device=None, log=print):
    """The whole folder, view by view in viewpair.txt order.  -> dict(points, views, skipped, seconds, io_seconds, per_view)."""
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        raise RuntimeError("fuse: needs an MI355X (there is no CPU fallback for the fusion kernels)")
    device = torch.device(device if device is not None else "cuda")
    max_src = _max_sources()
    if not 1 <= num_src <= max_src:
        raise ValueError("num_src=%d: 1 .. %d" % (num_src, max_src))
    t_start = time.time()
    folder = Folder(data_folder, output_folder)
    views, skipped = folder.plan(num_src)
    for ref in skipped:
        log("skip view %d: no depth maps in %s" % (ref, output_folder))
    ply_path = ply_path or os.path.join(output_folder, "fused.ply")
    cache = _MapCache(folder, device, capacity=2 * num_src + 2)
    io = 0.0
    per_view = []
    buffers = None
    with PlyWriter(ply_path) as ply:
        for ref_id, src_ids in views:
            if not src_ids:
                log("skip view %d: none of its sources has depth maps" % ref_id)
                skipped.append(ref_id)
                continue
            ref = cache.get(ref_id)
            srcs = [cache.get(s) for s in src_ids]
            t0 = time.time()
            b = folder.base(ref_id)
            conf = np.ascontiguousarray(read_pfm(b + "_prob.pfm")[0], dtype=np.float32)
            rgba = np.ascontiguousarray(np.array(Image.open(b + ".jpg").convert("RGBA")))
            io += time.time() - t0
            H, W = ref["depth"].shape
            if conf.shape != (H, W) or rgba.shape[:2] != (H, W):
                raise ValueError("view %d: depth %s, confidence %s, image %s differ in size" % (ref_id, (H, W), conf.shape, rgba.shape[:2]))
            if buffers is None or buffers[0].shape[0] < H * W:
                buffers = (torch.empty(H * W, 3, device=device, dtype=torch.float64), torch.empty(H * W, 3, device=device, dtype=torch.uint8))
            _, fused, xyz, rgb = fuse_view(ref, srcs, torch.from_numpy(conf).to(device), torch.from_numpy(rgba).to(device), prob_threshold,
                                           pix_threshold, rel_depth_threshold, min_consistent, buffers)
            fused_h, xyz_h, rgb_h = fused.cpu().numpy(), xyz.cpu().numpy(), rgb.cpu().numpy()
            t0 = time.time()
            vid_dir = os.path.dirname(b)
            os.makedirs(os.path.join(vid_dir, "mask"), exist_ok=True)
            save_pfm(b + "_fused.pfm", fused_h)
            Image.fromarray(np.where(fused_h > 0, 255, 0).astype(np.uint8)).save(os.path.join(vid_dir, "mask", os.path.basename(b) + "_final.png"))
            ply.write(xyz_h, rgb_h)
            io += time.time() - t0
            per_view.append((ref_id, len(xyz_h)))
            log("fuse view %d (%s, %d sources): %d points" % (ref_id, "/".join(view_key(folder.images[ref_id])), len(srcs), len(xyz_h)))
        points = ply.count
    seconds = time.time() - t_start
    io += cache.io_seconds
    log("fused %d points from %d views into %s, total_time = %.3f s (file I/O %.3f s)" % (points, len(per_view), ply_path, seconds, io))
    return dict(points=points, views=len(per_view), skipped=skipped, seconds=seconds, io_seconds=io, per_view=per_view, ply=ply_path)


def _max_sources():
    from . import _lib
    return _lib.load().adamvs_fusion_max_sources()


def build_parser():
    ap = argparse.ArgumentParser(description="Fuse the depth maps of a predict output folder into one point cloud")
    ap.add_argument("--data_folder", required=True, help="the whu-omvs data folder predict_whu.py read")
    ap.add_argument("--output_folder", required=True, help="predict_whu.py's output folder (maps in, fused maps and masks out)")
    ap.add_argument("--ply", default=None, help="point cloud to write (default <output_folder>/fused.ply)")
    ap.add_argument("--prob_threshold", type=float, default=0.5, help="reference pixels need a confidence >= this")
    ap.add_argument("--pix_threshold", type=float, default=1.0, help="largest reprojection error of a consistent source (px)")
    ap.add_argument("--rel_depth_threshold", type=float, default=0.01, help="largest relative depth error of a consistent source")
    ap.add_argument("--min_consistent", type=int, default=2, help="consistent sources a pixel needs to be kept")
    ap.add_argument("--num_src", type=int, default=4, help="listed sources checked per reference view (default view_num - 1)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    return fuse_folder(args.data_folder, args.output_folder, args.ply, args.prob_threshold, args.pix_threshold, args.rel_depth_threshold,
                       args.min_consistent, args.num_src)


if __name__ == "__main__":
    main()
