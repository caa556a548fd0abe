"""Rasterisation of a fused point cloud into a digital surface model (DSM) and a true orthophoto.

    python dsm_whu.py --ply /out/predict/fused.ply --gsd 0.25 --out /out/predict/dsm [--mode max|mean] [--min_count 1]
                      [--bounds XMIN YMIN XMAX YMAX] [--chunk N] [--fill_max_dist METRES]

The step after fuse_whu.py.  The PLY is streamed twice in chunks through a memory map (the cloud is never held in host
memory): the first pass finds the bounds of the finite points on the GPU (torch aminmax; min and max are exact), the second
scatters every chunk into the cell state on the GPU (csrc/dsm.hip; include/adamvs_hip.h "DSM" states the semantics).
Written: `<out>_dsm.tif` (float32 heights, NaN where empty), `<out>_count.tif` (uint16 points per cell, saturating),
`<out>_ortho.png` (RGBA, alpha 0 where empty), ESRI world files next to each image (`.tfw` / `.pgw`) and `<out>_dsm.json`.

With --fill_max_dist, the empty cells within that distance of a filled one are filled on the GPU by bounded harmonic
interpolation (fill_gaps; csrc/dsm_fill.hip, include/adamvs_hip.h "DSM gap fill"), and fill_output_paths(out) are written too.

World axes are x east, y north, z up.  Row 0 of every raster is the northern edge (y_top); column 0 the western (x0).
"""
import argparse
import json
import math
import os
import sys
import time
from collections import namedtuple

import numpy as np

from .fusion import PLY_DTYPE

MODES = {"max": 0, "mean": 1}                       # ADAMVS_DSM_MAX / ADAMVS_DSM_MEAN
MAX_CELLS = 1 << 28                                 # ADAMVS_DSM_MAX_CELLS
MAX_POINTS = (1 << 32) - 1                          # sequence numbers are uint32
FILL_MAX_RADIUS = 1024                              # ADAMVS_DSM_FILL_MAX_RADIUS, cells
FILL_MAX_CYCLES = 200
# device bytes per cell: key 8 + count 4 + colour 4 (+ sum 8 in mean mode) of state, dsm 4 + count 2 + rgba 4 of output
STATE_BYTES = {"max": 16, "mean": 24}
OUTPUT_BYTES = 10

Grid = namedtuple("Grid", "x0 y_top gsd z_ref W H")


def _check_gsd(gsd):
    gsd = float(gsd)
    if not (math.isfinite(gsd) and gsd > 0.0):
        raise ValueError("gsd=%r must be finite and > 0" % gsd)
    return gsd


def grid_for_bounds(lo, hi, gsd, z_ref):
    """The grid covering every point with lo <= (x, y) <= hi, in fp64:
        x0 = floor(lo.x / gsd) gsd,  y_top = (floor(hi.y / gsd) + 1) gsd,  W = floor((hi.x - x0) / gsd) + 1,
        H = floor((y_top - lo.y) / gsd) + 1.
    Should rounding put lo.x left of x0 or hi.y above y_top (the division lands on an integer the exact quotient lies just
    below), the grid is widened by that one cell, so the bound points always fall inside it."""
    gsd = _check_gsd(gsd)
    lx, ly, hx, hy, z_ref = (float(v) for v in (lo[0], lo[1], hi[0], hi[1], z_ref))
    if not all(math.isfinite(v) for v in (lx, ly, hx, hy, z_ref)):
        raise ValueError("bounds / z_ref must be finite: lo %r, hi %r, z_ref %r" % (lo, hi, z_ref))
    if not (lx <= hx and ly <= hy):
        raise ValueError("bounds: lo %r must not exceed hi %r" % ((lx, ly), (hx, hy)))
    x0 = math.floor(lx / gsd) * gsd
    if math.floor((lx - x0) / gsd) < 0:
        x0 -= gsd
    y_top = (math.floor(hy / gsd) + 1) * gsd
    if math.floor((y_top - hy) / gsd) < 0:
        y_top += gsd
    W = math.floor((hx - x0) / gsd) + 1
    H = math.floor((y_top - ly) / gsd) + 1
    if W * H > MAX_CELLS:
        raise ValueError("grid of %d x %d cells at gsd %g exceeds the cap of %d cells (%d device bytes per cell in mean mode, "
                         "%d in max mode): raise --gsd or crop with --bounds" % (W, H, gsd, MAX_CELLS, STATE_BYTES["mean"] + OUTPUT_BYTES,
                                                                                 STATE_BYTES["max"] + OUTPUT_BYTES))
    return Grid(x0, y_top, gsd, z_ref, int(W), int(H))


def world_file_text(grid):
    """ESRI world file: pixel size in x, two rotation terms, pixel size in y (negative: rows run south), then the x and y of
    the first cell's centre."""
    vals = (grid.gsd, 0.0, 0.0, -grid.gsd, grid.x0 + grid.gsd / 2.0, grid.y_top - grid.gsd / 2.0)
    return "".join(repr(float(v)) + "\n" for v in vals)


# ---- the PLY, streamed ------------------------------------------------------------------------------------------------
def ply_layout(path):
    """-> (byte offset of the vertex data, vertex count) of a binary little-endian PLY with fusion.PLY_DTYPE's vertices."""
    with open(path, "rb") as f:
        head = f.read(4096)
    end = head.find(b"end_header\n")
    if not head.startswith(b"ply\n") or end < 0:
        raise ValueError("%s: not a PLY file with a header under 4 KB" % path)
    lines = head[:end].decode("ascii").splitlines()
    props = [tuple(ln.split()[1:]) for ln in lines if ln.startswith("property")]
    want = [("double", "x"), ("double", "y"), ("double", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    if "format binary_little_endian 1.0" not in lines or props != want:
        raise ValueError("%s: expected binary_little_endian vertices (double x y z, uchar red green blue) as fuse_whu.py writes them"
                         % path)
    count = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    offset = end + len(b"end_header\n")
    if os.path.getsize(path) < offset + count * PLY_DTYPE.itemsize:
        raise ValueError("%s: %d vertices announced, the file is shorter" % (path, count))
    return offset, count


def ply_chunks(path, n):
    """Yields (xyz [m, 3] float64, rgb [m, 3] uint8) of at most n points each, in file order, through a memory map."""
    if n < 1:
        raise ValueError("chunk size %d (>= 1)" % n)
    offset, count = ply_layout(path)
    if count == 0:
        return
    mm = np.memmap(path, dtype=PLY_DTYPE, mode="r", offset=offset, shape=(count,))
    for s in range(0, count, n):
        rec = mm[s:s + n]
        xyz = np.empty((len(rec), 3), np.float64)
        rgb = np.empty((len(rec), 3), np.uint8)
        for c, name in enumerate(("x", "y", "z")):
            xyz[:, c] = rec[name]
        for c, name in enumerate(("red", "green", "blue")):
            rgb[:, c] = rec[name]
        yield xyz, rgb
    del mm


# ---- the GPU raster -----------------------------------------------------------------------------------------------------
class DsmBuilder:
    """Cell state of one grid on the device; add() chunks of points in stream order, finish() once."""

    def __init__(self, grid, mode="max", device=None):
        import torch
        if mode not in MODES:
            raise ValueError("mode %r: one of %s" % (mode, sorted(MODES)))
        if grid.W * grid.H > MAX_CELLS:
            raise ValueError("grid of %d x %d cells exceeds the cap of %d" % (grid.W, grid.H, MAX_CELLS))
        self.grid, self.mode = grid, mode
        self.device = torch.device(device if device is not None else "cuda")
        n = grid.W * grid.H
        self.key = torch.zeros(n, device=self.device, dtype=torch.int64)
        self.count = torch.zeros(n, device=self.device, dtype=torch.int32)
        self.color = torch.zeros(n, device=self.device, dtype=torch.int32)
        self.sum = torch.zeros(n, device=self.device, dtype=torch.int64) if mode == "mean" else None
        self.points = 0

    def add(self, xyz, rgb):
        """xyz [n, 3] float64, rgb [n, 3] uint8: device tensors (a CPU tensor raises AdaMVSHipError)."""
        from . import hip_ops
        n = int(xyz.shape[0])
        if self.points + n > MAX_POINTS:
            raise ValueError("more than %d points in one DSM (sequence numbers are uint32)" % MAX_POINTS)
        hip_ops.dsm_accumulate(self.grid, xyz, self.points, MODES[self.mode], self.key, self.count, self.sum)
        hip_ops.dsm_claim(self.grid, xyz, rgb, self.points, self.key, self.color)
        self.points += n

    def finish(self, min_count=1):
        """-> dict(dsm [H, W] float32, count [H, W] uint16, rgba [H, W, 4] uint8 (host arrays), points_read, points_used,
        cells_filled)."""
        from . import hip_ops
        if int(min_count) < 1:
            raise ValueError("min_count=%r (>= 1)" % min_count)
        dsm, count16, rgba = hip_ops.dsm_finalize(self.grid, self.key, self.count, self.sum, self.color, MODES[self.mode], int(min_count))
        count = self.count.to("cpu").numpy().view(np.uint32)
        return dict(dsm=dsm.cpu().numpy(), count=count16.cpu().numpy().view(np.uint16), rgba=rgba.cpu().numpy(), grid=self.grid,
                    mode=self.mode, min_count=int(min_count), points_read=self.points, points_used=int(count.sum(dtype=np.uint64)),
                    cells_filled=int((count >= int(min_count)).sum()))


def point_bounds(path, chunk, device):
    """First pass: (lo, hi) (x, y, z) of the points with three finite coordinates, and the number of points."""
    import torch
    lo = np.full(3, np.inf)
    hi = np.full(3, -np.inf)
    for xyz, _ in ply_chunks(path, chunk):
        t = torch.from_numpy(xyz).to(device)
        t = t[torch.isfinite(t).all(1)]
        if t.shape[0]:
            mn, mx = torch.aminmax(t, dim=0)
            lo = np.minimum(lo, mn.cpu().numpy())
            hi = np.maximum(hi, mx.cpu().numpy())
    return lo, hi


# ---- gap fill -----------------------------------------------------------------------------------------------------------
class FillNotConverged(RuntimeError):
    pass


def fill_gaps(dsm, rgba, r_cells, tol_height=1e-6, tol_colour=1e-3, max_cycles=FILL_MAX_CYCLES, device=None):
    """Bounded harmonic fill of the empty cells of finish()'s rasters (host arrays dsm [H, W] float32, rgba [H, W, 4] uint8)
    within r_cells of a valid cell -> dict(dsm, rgba, filled (uint8, 1 where filled), dist2 (int32), cycles, residual_height,
    residual_colour, cells_valid, cells_filled, cells_empty, seconds).  Raises FillNotConverged if max_cycles V-cycles do not
    bring the largest residual under the tolerances."""
    import torch
    from . import hip_ops
    r = float(r_cells)
    if not (math.isfinite(r) and 0.0 < r <= FILL_MAX_RADIUS):
        raise ValueError("fill radius %r cells: must be finite, > 0 and <= %d" % (r_cells, FILL_MAX_RADIUS))
    dev = torch.device(device if device is not None else "cuda")
    d = torch.from_numpy(np.ascontiguousarray(dsm, np.float32)).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(rgba, np.uint8)).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.time()
    d2, c2, dist2, filled, st = hip_ops.dsm_fill(d, c, r, tol_height, tol_colour, max_cycles)
    seconds = time.time() - t0
    if not st.converged:
        raise FillNotConverged("gap fill did not converge in %d V-cycles: largest residual %.3e m (tolerance %.3e) and %.3e colour "
                               "levels (tolerance %.3e)" % (st.cycles, st.residual_height, tol_height, st.residual_colour, tol_colour))
    return dict(dsm=d2.cpu().numpy(), rgba=c2.cpu().numpy(), filled=filled.cpu().numpy(), dist2=dist2.cpu().numpy(), cycles=st.cycles,
                residual_height=st.residual_height, residual_colour=st.residual_colour, cells_valid=st.cells_valid,
                cells_filled=st.cells_filled, cells_empty=st.cells_empty, seconds=seconds)


def from_ply(ply, gsd, mode="max", min_count=1, bounds=None, chunk=1 << 23, device=None, out=None, fill_max_dist=None):
    """Two passes over the PLY (bounds, raster) -> DsmBuilder.finish()'s dict; written to `out` (a path prefix) if given.
    bounds: (xmin, ymin, xmax, ymax) crops the grid; z_ref = floor of the lowest finite z either way.
    fill_max_dist (metres): also fill_gaps() at r = fill_max_dist / gsd cells, as res["fill"] (with max_dist, gsd, r_cells),
    written to fill_output_paths(out)."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("dsm: needs an MI355X (there is no CPU fallback for the DSM kernels)")
    device = torch.device(device if device is not None else "cuda")
    gsd = _check_gsd(gsd)
    if fill_max_dist is not None:
        fill_r = fill_radius_cells(fill_max_dist, gsd)
    if mode not in MODES:
        raise ValueError("mode %r: one of %s" % (mode, sorted(MODES)))
    if int(min_count) < 1:
        raise ValueError("min_count=%r (>= 1)" % min_count)
    _, count = ply_layout(ply)
    if count > MAX_POINTS:
        raise ValueError("%s holds %d points: at most %d go into one DSM" % (ply, count, MAX_POINTS))
    lo, hi = point_bounds(ply, chunk, device)
    if not np.isfinite(lo).all():
        raise ValueError("%s: no point with finite coordinates" % ply)
    z_ref = math.floor(lo[2])
    if bounds is not None:
        xmin, ymin, xmax, ymax = (float(v) for v in bounds)
        grid = grid_for_bounds((xmin, ymin), (xmax, ymax), gsd, z_ref)
    else:
        grid = grid_for_bounds(lo, hi, gsd, z_ref)
    b = DsmBuilder(grid, mode, device)
    for xyz, rgb in ply_chunks(ply, chunk):
        b.add(torch.from_numpy(xyz).to(device), torch.from_numpy(rgb).to(device))
    res = b.finish(min_count)
    if out is not None:
        write_outputs(out, res)
    if fill_max_dist is not None:
        res["fill"] = fill_gaps(res["dsm"], res["rgba"], fill_r, device=device)
        res["fill"].update(max_dist=float(fill_max_dist), gsd=gsd, r_cells=fill_r)
        if out is not None:
            write_fill_outputs(out, res["grid"], res["fill"])
    return res


def fill_radius_cells(max_dist, gsd):
    """--fill_max_dist (metres) -> r in cells (max_dist / gsd), checked against the cap."""
    m = float(max_dist)
    r = m / gsd
    if not (math.isfinite(m) and m > 0.0 and r <= FILL_MAX_RADIUS):
        raise ValueError("fill_max_dist=%r m at gsd %g is %g cells: must be > 0 and at most %d cells" % (max_dist, gsd, r, FILL_MAX_RADIUS))
    return r


# ---- files --------------------------------------------------------------------------------------------------------------
def output_paths(out):
    return dict(dsm=out + "_dsm.tif", dsm_world=out + "_dsm.tfw", count=out + "_count.tif", count_world=out + "_count.tfw",
                ortho=out + "_ortho.png", ortho_world=out + "_ortho.pgw", json=out + "_dsm.json")


def fill_output_paths(out):
    """The files of the gap fill (--fill_max_dist), next to output_paths(out) and disjoint from them."""
    return dict(dsm=out + "_dsm_filled.tif", dsm_world=out + "_dsm_filled.tfw", ortho=out + "_ortho_filled.png",
                ortho_world=out + "_ortho_filled.pgw", filled=out + "_filled.png", filled_world=out + "_filled.pgw", json=out + "_fill.json")


def fill_summary(fill):
    return {k: fill[k] for k in ("max_dist", "gsd", "r_cells", "cells_valid", "cells_filled", "cells_empty", "cycles", "residual_height",
                                 "residual_colour", "seconds")}


def write_fill_outputs(out, grid, fill):
    """fill_gaps()'s rasters (with max_dist, gsd, r_cells added), their world files and the JSON -> fill_output_paths(out)."""
    from PIL import Image
    paths = fill_output_paths(out)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(fill["dsm"], np.float32)).save(paths["dsm"], format="TIFF")
    Image.fromarray(np.ascontiguousarray(fill["rgba"], np.uint8)).save(paths["ortho"], format="PNG")
    Image.fromarray(np.where(np.asarray(fill["filled"]) != 0, 255, 0).astype(np.uint8)).save(paths["filled"], format="PNG")
    wf = world_file_text(grid)
    for k in ("dsm_world", "ortho_world", "filled_world"):
        with open(paths[k], "w") as f:
            f.write(wf)
    with open(paths["json"], "w") as f:
        json.dump(fill_summary(fill), f, indent=1)
        f.write("\n")
    return paths


def read_fill_outputs(out):
    """-> (dsm float32, rgba uint8, filled uint8 (1 where filled)) read back from the files of write_fill_outputs."""
    from PIL import Image
    paths = fill_output_paths(out)
    return (np.array(Image.open(paths["dsm"]), np.float32), np.array(Image.open(paths["ortho"]).convert("RGBA")),
            (np.array(Image.open(paths["filled"])) == 255).astype(np.uint8))


def summary(res):
    g = res["grid"]
    return dict(grid=dict(x0=g.x0, y_top=g.y_top, gsd=g.gsd, W=g.W, H=g.H), z_ref=g.z_ref, mode=res["mode"], min_count=res["min_count"],
                points_read=res["points_read"], points_used=res["points_used"], cells_filled=res["cells_filled"])


def write_outputs(out, res):
    """The rasters, their world files and the JSON summary at the path prefix `out` -> output_paths(out)."""
    from PIL import Image
    paths = output_paths(out)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    # float32 -> mode "F", uint16 -> "I;16", [H, W, 4] uint8 -> "RGBA"
    Image.fromarray(np.ascontiguousarray(res["dsm"], np.float32)).save(paths["dsm"], format="TIFF")
    Image.fromarray(np.ascontiguousarray(res["count"], np.uint16)).save(paths["count"], format="TIFF")
    Image.fromarray(np.ascontiguousarray(res["rgba"], np.uint8)).save(paths["ortho"], format="PNG")
    wf = world_file_text(res["grid"])
    for k in ("dsm_world", "count_world", "ortho_world"):
        with open(paths[k], "w") as f:
            f.write(wf)
    with open(paths["json"], "w") as f:
        json.dump(summary(res), f, indent=1)
        f.write("\n")
    return paths


def read_outputs(out):
    """-> (dsm float32, count uint16, rgba uint8) read back from the files of write_outputs."""
    from PIL import Image
    paths = output_paths(out)
    return (np.array(Image.open(paths["dsm"]), np.float32), np.array(Image.open(paths["count"])).astype(np.uint16),
            np.array(Image.open(paths["ortho"]).convert("RGBA")))


def build_parser():
    ap = argparse.ArgumentParser(description="Rasterise a fused point cloud into a DSM and a true orthophoto")
    ap.add_argument("--ply", required=True, help="point cloud written by fuse_whu.py")
    ap.add_argument("--gsd", type=float, required=True, help="ground sample distance: cell size in metres")
    ap.add_argument("--out", required=True, help="output path prefix: <out>_dsm.tif, <out>_count.tif, <out>_ortho.png, ...")
    ap.add_argument("--mode", choices=sorted(MODES), default="max", help="max: the highest point per cell; mean: the mean height")
    ap.add_argument("--min_count", type=int, default=1, help="cells with fewer points are left empty (NaN, alpha 0)")
    ap.add_argument("--bounds", type=float, nargs=4, metavar=("XMIN", "YMIN", "XMAX", "YMAX"), default=None, help="crop to this area")
    ap.add_argument("--chunk", type=int, default=1 << 23, help="points per chunk streamed to the GPU")
    ap.add_argument("--fill_max_dist", type=float, default=None, metavar="METRES",
                    help="also fill empty cells within this distance of a filled cell by harmonic interpolation (<out>_dsm_filled.tif, ...)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    t0 = time.time()
    res = from_ply(args.ply, args.gsd, args.mode, args.min_count, args.bounds, args.chunk, out=args.out, fill_max_dist=args.fill_max_dist)
    g = res["grid"]
    print("dsm %d x %d cells at gsd %g (x0 %.3f, y_top %.3f, z_ref %g, %s): %d of %d points used, %d cells filled, total_time = %.3f s"
          % (g.W, g.H, g.gsd, g.x0, g.y_top, g.z_ref, res["mode"], res["points_used"], res["points_read"], res["cells_filled"], time.time() - t0))
    if "fill" in res:
        f = res["fill"]
        print("fill within %g m (%g cells): %d cells filled, %d left empty, %d valid; %d V-cycles, residual %.2e m / %.2e levels, %.3f s"
              % (f["max_dist"], f["r_cells"], f["cells_filled"], f["cells_empty"], f["cells_valid"], f["cycles"], f["residual_height"],
                 f["residual_colour"], f["seconds"]))
    return res


if __name__ == "__main__":
    main()
