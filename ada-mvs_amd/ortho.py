"""Image orthophoto: the source images mosaicked over a DSM into a true orthophoto on the GPU.

    python ortho_whu.py --data_folder D --output_folder O --dsm PREFIX [--filled] [--upsample K] [--mode best|feather]
                        [--occlusion_tol M] [--border_px 2] [--feather_px 64] [--out PREFIX]

The step after dsm_whu.py.  PREFIX is the prefix dsm_whu.py --out was given: the grid comes from `<PREFIX>_dsm.json`, the
heights from `<PREFIX>_dsm.tif` (or `<PREFIX>_dsm_filled.tif` with --filled; NaN: no surface).  The views are predict's
images `<vid>/<name>.jpg` with the `<name>.txt` intrinsics and the fp64 poses of image_info.txt, every view with both files,
in ascending image id.  Per view, csrc/ortho.hip renders the DSM's triangulated height field into a depth buffer at the
image's size, then every orthophoto cell's surface point is projected, tested against that buffer and coloured by a
bilinear sample; `best` keeps the most nadir view that sees the cell, `feather` blends every such view
(include/adamvs_hip.h "Image orthophoto" states every operation).  Written (--out defaults to PREFIX):
`<out>_ortho_img.png` (RGBA, alpha 0 where no surface or no view), `<out>_ortho_img.pgw`, `<out>_ortho_img_view.tif`
(int32 image id of the chosen view, -1 where none), `<out>_ortho_img_nvis.tif` (uint16 views that see the cell) and
`<out>_ortho_img.json`.  The orthophoto grid is the DSM's refined K times: cells of gsd / K from the same corner.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

from . import fusion
from .dsm import Grid, world_file_text
from .mesh import cull_views

MODES = {"best": 0, "feather": 1}                   # ADAMVS_ORTHO_BEST / ADAMVS_ORTHO_FEATHER
MAX_CELLS = 1 << 28                                 # ADAMVS_ORTHO_MAX_CELLS
MAX_UPSAMPLE = 8                                    # ADAMVS_ORTHO_MAX_UPSAMPLE
CULL_MARGIN_PX = 2.0


def check_upsample(upsample):
    """K: an integer 1 .. 8 (an integral float is accepted)."""
    if isinstance(upsample, bool):
        raise ValueError("upsample %r: an integer 1 .. %d" % (upsample, MAX_UPSAMPLE))
    try:
        k = float(upsample)
    except (TypeError, ValueError):
        raise ValueError("upsample %r: an integer 1 .. %d" % (upsample, MAX_UPSAMPLE)) from None
    if not (math.isfinite(k) and k.is_integer() and 1 <= k <= MAX_UPSAMPLE):
        raise ValueError("upsample %r: an integer 1 .. %d" % (upsample, MAX_UPSAMPLE))
    return int(k)


def ortho_grid(grid, upsample):
    """The orthophoto grid of a DSM grid at upsample K, as a dsm.Grid: cells of gsd / K, W K x H K, the same x0 and y_top."""
    K = check_upsample(upsample)
    W, H = int(grid.W) * K, int(grid.H) * K
    if W * H > MAX_CELLS:
        raise ValueError("orthophoto of %d x %d cells (DSM %d x %d at upsample %d) exceeds the cap of %d cells"
                         % (W, H, grid.W, grid.H, K, MAX_CELLS))
    return Grid(float(grid.x0), float(grid.y_top), float(grid.gsd) / K, grid.z_ref, W, H)


def check_options(mode, occlusion_tol, border_px, feather_px):
    if mode not in MODES:
        raise ValueError("mode %r: one of %s" % (mode, sorted(MODES)))
    for name, v, lo_ok in (("occlusion_tol", occlusion_tol, True), ("border_px", border_px, True), ("feather_px", feather_px, False)):
        f = float(v)
        if not (math.isfinite(f) and (f >= 0.0 if lo_ok else f > 0.0)):
            raise ValueError("%s=%r must be finite and %s" % (name, v, ">= 0" if lo_ok else "> 0"))


def dsm_box(grid, dsm):
    """(lo, hi) fp64 of the DSM's bounding box: the grid's extent, z from the finite min and max; None if no cell is finite."""
    z = np.asarray(dsm, np.float32)
    fin = z[np.isfinite(z)]
    if fin.size == 0:
        return None
    lo = np.array([grid.x0, grid.y_top - grid.H * grid.gsd, float(fin.min())], np.float64)
    hi = np.array([grid.x0 + grid.W * grid.gsd, grid.y_top, float(fin.max())], np.float64)
    return lo, hi


def view_camera(view):
    """(K, R_wc, C, H, W) of a view dict for mesh.cull_views."""
    H, W = int(view["rgba"].shape[0]), int(view["rgba"].shape[1])
    return (np.asarray(view["K"], np.float64), np.asarray(view["R"], np.float64), np.asarray(view["C"], np.float64), H, W)


# ---- the GPU mosaic ---------------------------------------------------------------------------------------------------
class OrthoBuilder:
    """Cell state of one orthophoto on the device.  dsm: [H, W] float32 (host or device) on `grid` (a dsm.Grid);
    add_view() the views in ascending image id, finish() once.  A view is dict(iid, K [3, 3], R (R_wc), C (fp64),
    rgba device [H, W, 4] uint8).  keep_zbufs: keep each view's depth buffer in .zbufs (image id -> device tensor)."""

    def __init__(self, grid, upsample, mode, dsm, occlusion_tol=None, border_px=2.0, feather_px=64.0, device=None, keep_zbufs=False):
        import torch
        from . import hip_ops
        occlusion_tol = 2.0 * float(grid.gsd) if occlusion_tol is None else float(occlusion_tol)
        check_options(mode, occlusion_tol, border_px, feather_px)
        self.grid, self.K, self.mode = grid, check_upsample(upsample), mode
        self.ogrid = ortho_grid(grid, self.K)
        self.occlusion_tol, self.border_px, self.feather_px = occlusion_tol, float(border_px), float(feather_px)
        self.device = torch.device(device if device is not None else "cuda")
        d = dsm if isinstance(dsm, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dsm, np.float32))
        if tuple(d.shape) != (grid.H, grid.W):
            raise ValueError("dsm %s does not match the grid's %d x %d cells" % (tuple(d.shape), grid.H, grid.W))
        self.dsm = d.to(self.device, torch.float32).contiguous()
        self.box = dsm_box(grid, self.dsm.cpu().numpy())
        self.cgrid = hip_ops.ortho_grid(grid.x0, grid.y_top, grid.gsd, grid.W, grid.H, self.K)
        self.height = hip_ops.ortho_surface(self.cgrid, self.dsm)
        n = self.ogrid.W * self.ogrid.H
        self.acc = torch.zeros(n, 4, device=self.device, dtype=torch.float32)
        self.wmax = torch.full((n,), -math.inf if mode == "best" else 0.0, device=self.device, dtype=torch.float32)
        self.vstate = torch.full((n,), -1, device=self.device, dtype=torch.int32)
        self.nvis = torch.zeros(n, device=self.device, dtype=torch.int32)
        self.big = torch.empty(1 + 2 * max(grid.W - 1, 0) * max(grid.H - 1, 0), device=self.device, dtype=torch.int32)
        self.used, self.culled, self.events = [], [], []
        self.last_iid = None
        self.zbufs = {} if keep_zbufs else None          # image id -> the view's depth buffer (device int32, float bits)

    def add_view(self, view):
        """Mosaic one view in -> True, or False if it is culled (the DSM's box projects wholly outside its image)."""
        import torch
        from . import hip_ops
        iid = int(view["iid"])
        if self.last_iid is not None and iid <= self.last_iid:
            raise ValueError("views must come in ascending image id: %d after %d" % (iid, self.last_iid))
        self.last_iid = iid
        cam = view_camera(view)
        if self.box is None or not cull_views(self.box[0], self.box[1], [cam], CULL_MARGIN_PX):
            self.culled.append(iid)
            return False
        v = hip_ops.ortho_view(cam[0], cam[1].T, cam[2], view["rgba"])
        zbuf = torch.empty(cam[3], cam[4], device=self.device, dtype=torch.int32)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        hip_ops.ortho_zbuf(self.cgrid, self.dsm, v, zbuf, self.big)
        e1.record()
        hip_ops.ortho_compose(self.cgrid, v, iid, self.height, zbuf, MODES[self.mode], self.border_px, self.feather_px, self.occlusion_tol,
                              self.acc, self.wmax, self.vstate, self.nvis)
        e2.record()
        self.events.append((e0, e1, e2))
        self.used.append(iid)
        if self.zbufs is not None:
            self.zbufs[iid] = zbuf
        return True

    def finish(self):
        """-> dict(rgba [H_o, W_o, 4] uint8, view int32, nvis uint16 (host arrays), grid (the orthophoto's dsm.Grid), summary
        counts and device seconds)."""
        import torch
        from . import hip_ops
        rgba, view, nvis = hip_ops.ortho_finalize(self.cgrid, self.acc, self.vstate, self.nvis)
        rgba, view, nvis = rgba.cpu().numpy(), view.cpu().numpy(), nvis.cpu().numpy().view(np.uint16)
        torch.cuda.synchronize(self.device)
        t_z = sum(a.elapsed_time(b) for a, b, _ in self.events) / 1e3
        t_c = sum(b.elapsed_time(c) for _, b, c in self.events) / 1e3
        surface = ~torch.isnan(self.height).cpu().numpy()
        return dict(rgba=rgba, view=view, nvis=nvis, grid=self.ogrid, dsm_grid=self.grid, upsample=self.K, mode=self.mode,
                    occlusion_tol=self.occlusion_tol, border_px=self.border_px, feather_px=self.feather_px, views_used=list(self.used),
                    views_culled=list(self.culled), cells_surface=int(surface.sum()), cells_coloured=int((rgba[..., 3] > 0).sum()),
                    cells_unseen=int((surface & (nvis == 0)).sum()), zbuf_seconds=t_z, compose_seconds=t_c, device_seconds=t_z + t_c)


def from_dsm(dsm, grid, views, upsample=1, mode="best", occlusion_tol=None, border_px=2.0, feather_px=64.0, device=None):
    """A host DSM array [H, W] float32 on `grid` (dsm.Grid) and views as load_views gives them -> OrthoBuilder.finish()'s dict
    plus `seconds`."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("ortho: needs an MI355X (there is no CPU fallback for the orthophoto kernels)")
    t0 = time.time()
    b = OrthoBuilder(grid, upsample, mode, dsm, occlusion_tol, border_px, feather_px, device)
    for v in sorted(views, key=lambda v: int(v["iid"])):
        b.add_view(v)
    res = b.finish()
    res["seconds"] = time.time() - t0
    return res


# ---- a predict output folder ------------------------------------------------------------------------------------------
def load_views(folder, device):
    """Every view of the folder with an image and a camera -> [dict(iid, K, R, C, rgba)] in ascending image id (depth maps are
    not read)."""
    import torch
    from PIL import Image
    views = []
    for iid in sorted(folder.images):
        base = folder.base(iid)
        if not all(os.path.exists(base + ext) for ext in (".txt", ".jpg")):
            continue
        _, K = fusion.read_cam_txt(base + ".txt")
        rgba = np.ascontiguousarray(np.array(Image.open(base + ".jpg").convert("RGBA")))
        R, C = fusion.pose(folder.images[iid])
        views.append(dict(iid=iid, K=K, R=R, C=C, rgba=torch.from_numpy(rgba).to(device)))
    return views


def read_dsm(prefix, filled=False):
    """-> (dsm [H, W] float32, dsm.Grid) from `<prefix>_dsm.json` and `<prefix>_dsm.tif` (`_dsm_filled.tif` if filled)."""
    from . import raster_stage
    grid = raster_stage.read_grid(prefix)
    tif = prefix + ("_dsm_filled.tif" if filled else "_dsm.tif")
    return raster_stage.read_raster(tif, np.float32, (grid.H, grid.W), says="%s_dsm.json says %d x %d" % (prefix, grid.H, grid.W)), grid


def output_paths(out):
    return dict(ortho=out + "_ortho_img.png", ortho_world=out + "_ortho_img.pgw", view=out + "_ortho_img_view.tif",
                nvis=out + "_ortho_img_nvis.tif", json=out + "_ortho_img.json")


def summary(res):
    g, dg = res["grid"], res["dsm_grid"]
    return dict(grid=dict(x0=g.x0, y_top=g.y_top, gsd=g.gsd, W=g.W, H=g.H), dsm_grid=dict(gsd=dg.gsd, W=dg.W, H=dg.H),
                upsample=res["upsample"], mode=res["mode"], occlusion_tol=res["occlusion_tol"], border_px=res["border_px"],
                feather_px=res["feather_px"], views_used=res["views_used"], views_culled=res["views_culled"],
                cells_surface=res["cells_surface"], cells_coloured=res["cells_coloured"], cells_unseen=res["cells_unseen"],
                seconds=res.get("seconds", 0.0), device_seconds=res["device_seconds"])


def write_outputs(out, res):
    """The orthophoto, its world file, the view and count rasters and the JSON summary at the prefix `out` -> output_paths(out)."""
    from PIL import Image
    paths = output_paths(out)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(res["rgba"], np.uint8)).save(paths["ortho"], format="PNG")
    Image.fromarray(np.ascontiguousarray(res["view"], np.int32)).save(paths["view"], format="TIFF")
    Image.fromarray(np.ascontiguousarray(res["nvis"], np.uint16)).save(paths["nvis"], format="TIFF")
    with open(paths["ortho_world"], "w") as f:
        f.write(world_file_text(res["grid"]))
    with open(paths["json"], "w") as f:
        json.dump(summary(res), f, indent=1)
        f.write("\n")
    return paths


def read_outputs(out):
    """-> (rgba uint8, view int32, nvis uint16) read back from the files of write_outputs."""
    from PIL import Image
    paths = output_paths(out)
    return (np.array(Image.open(paths["ortho"]).convert("RGBA")), np.array(Image.open(paths["view"])).astype(np.int32),
            np.array(Image.open(paths["nvis"])).astype(np.uint16))


def from_folder(data_folder, output_folder, dsm_prefix, filled=False, upsample=1, mode="best", occlusion_tol=None, border_px=2.0,
                feather_px=64.0, out=None, device=None, log=print):
    """The whole chain step: read the DSM and the views, mosaic, write output_paths(out) -> from_dsm()'s dict."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("ortho: needs an MI355X (there is no CPU fallback for the orthophoto kernels)")
    check_upsample(upsample)
    check_options(mode, 0.0 if occlusion_tol is None else occlusion_tol, border_px, feather_px)
    t0 = time.time()
    dsm, grid = read_dsm(dsm_prefix, filled)
    ortho_grid(grid, upsample)
    device = torch.device(device if device is not None else "cuda")
    views = load_views(fusion.Folder(data_folder, output_folder), device)
    if not views:
        raise ValueError("%s: no view has both <name>.jpg and <name>.txt" % output_folder)
    res = from_dsm(dsm, grid, views, upsample, mode, occlusion_tol, border_px, feather_px, device)
    res["seconds"] = time.time() - t0
    write_outputs(dsm_prefix if out is None else out, res)
    g = res["grid"]
    log("ortho %d x %d cells at gsd %g (%s, upsample %d): %d views used, %d culled; %d of %d surface cells coloured, %d seen by no "
        "view; device %.3f s, total_time = %.3f s" % (g.W, g.H, g.gsd, mode, res["upsample"], len(res["views_used"]), len(res["views_culled"]),
                                                      res["cells_coloured"], res["cells_surface"], res["cells_unseen"], res["device_seconds"],
                                                      res["seconds"]))
    return res


def build_parser():
    ap = argparse.ArgumentParser(description="Mosaic the source images over a DSM into a true orthophoto")
    ap.add_argument("--data_folder", required=True, help="the whu-omvs data folder predict_whu.py read")
    ap.add_argument("--output_folder", required=True, help="predict_whu.py's output folder (its <vid>/<name>.jpg and .txt)")
    ap.add_argument("--dsm", required=True, metavar="PREFIX", help="the prefix dsm_whu.py --out was given")
    ap.add_argument("--filled", action="store_true", help="use <PREFIX>_dsm_filled.tif (dsm_whu.py --fill_max_dist)")
    ap.add_argument("--upsample", type=int, default=1, help="orthophoto cells per DSM cell along each axis (1 .. 8)")
    ap.add_argument("--mode", choices=sorted(MODES), default="best", help="best: the most nadir view that sees a cell; feather: a blend")
    ap.add_argument("--occlusion_tol", type=float, default=None, metavar="M", help="depth tolerance of the visibility test (default 2 gsd)")
    ap.add_argument("--border_px", type=float, default=2.0, help="samples closer than this to an image edge are not used")
    ap.add_argument("--feather_px", type=float, default=64.0, help="feather mode: the weight ramps up over this many pixels")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="output prefix (default: --dsm): <out>_ortho_img.png, ...")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    return from_folder(args.data_folder, args.output_folder, args.dsm, args.filled, args.upsample, args.mode, args.occlusion_tol,
                       args.border_px, args.feather_px, args.out)


if __name__ == "__main__":
    main()
