"""Ground filter of a DSM: the bare-earth terrain model (DTM) and the normalised DSM (nDSM = DSM - DTM, heights above ground).

    python dtm_whu.py --dsm /out/predict/dsm [--filled] [--max_radius 16] [--slope 1.0] [--dh0 0.15] [--dh_max 2.5]
                      [--fill_max_dist METRES] [--out PREFIX]

The step after dsm_whu.py.  The DSM (`<PREFIX>_dsm.tif`, or `<PREFIX>_dsm_filled.tif` with --filled) is classified on the GPU
by a progressive morphological filter with square windows (csrc/dsm_dtm.hip; include/adamvs_hip.h "DSM ground filter" states
the result operation by operation); the cells flagged as objects are removed and the terrain under them is interpolated by
the bounded harmonic gap fill the DSM already has (csrc/dsm_fill.hip, unchanged).  Written: `<out>_dtm.tif` and
`<out>_ndsm.tif` (float32, NaN where there is no value), `<out>_ground.png` (L: 0 empty, 255 ground, otherwise 16 x the level
at which the cell was flagged), ESRI world files next to each and `<out>_dtm.json`.  --out defaults to --dsm; none of the
names collides with a file of dsm_whu.py.

The defaults (max_radius 16 m, slope 1.0, dh0 0.15 m, dh_max 2.5 m) are the defaults of PCL's and PDAL's `pmf` at their
cell size 1: conventions, not measurements on this data.
"""
import argparse
import json
import math
import os
import time

import numpy as np

from . import raster_stage
from .dsm import FILL_MAX_CYCLES, FILL_MAX_RADIUS, FillNotConverged, _check_gsd, world_file_text

MAX_RADIUS = 1024                                   # ADAMVS_DTM_MAX_RADIUS, cells
MAX_LEVELS = 16                                     # ADAMVS_DTM_MAX_LEVELS
DEFAULTS = dict(max_radius=16.0, slope=1.0, dh0=0.15, dh_max=2.5)


def schedule(gsd, max_radius=DEFAULTS["max_radius"], slope=DEFAULTS["slope"], dh0=DEFAULTS["dh0"], dh_max=DEFAULTS["dh_max"]):
    """-> (radius int32 [K], dh float64 [K]): R = floor(max_radius / gsd) cells, radii 1, 2, 4, ... while below R, then R;
    w_k = 2 r_k + 1, w_0 = 1; dh_k = min(dh_max, dh0 + slope gsd (w_k - w_{k-1}))."""
    gsd = _check_gsd(gsd)
    max_radius, slope, dh0, dh_max = float(max_radius), float(slope), float(dh0), float(dh_max)
    for name, v, positive in (("max_radius", max_radius, True), ("slope", slope, False), ("dh0", dh0, True), ("dh_max", dh_max, True)):
        if not math.isfinite(v) or v < 0.0 or (positive and v == 0.0):
            raise ValueError("%s=%r must be finite and %s 0" % (name, v, ">" if positive else ">="))
    R = math.floor(max_radius / gsd)
    if not 1 <= R <= MAX_RADIUS:
        raise ValueError("max_radius=%g m at gsd %g is %d cells: must be 1 .. %d cells" % (max_radius, gsd, R, MAX_RADIUS))
    radius = []
    r = 1
    while r < R:
        radius.append(r)
        r *= 2
    radius.append(R)
    assert len(radius) <= MAX_LEVELS
    dh, w_prev = [], 1
    for r in radius:
        w = 2 * r + 1
        dh.append(min(dh_max, dh0 + slope * gsd * (w - w_prev)))
        w_prev = w
    return np.array(radius, np.int32), np.array(dh, np.float64)


def fill_radius_cells(fill_max_dist, max_radius, gsd):
    """The fill radius in cells: fill_max_dist / gsd, fill_max_dist defaulting to 2 max_radius (the centre of a removed object
    lies within R + 1 cells of ground), capped at the fill's largest radius."""
    m = 2.0 * float(max_radius) if fill_max_dist is None else float(fill_max_dist)
    if not (math.isfinite(m) and m > 0.0):
        raise ValueError("fill_max_dist=%r m must be finite and > 0" % fill_max_dist)
    return m, min(m / gsd, float(FILL_MAX_RADIUS))


def ground_filter(dsm, gsd, max_radius=DEFAULTS["max_radius"], slope=DEFAULTS["slope"], dh0=DEFAULTS["dh0"], dh_max=DEFAULTS["dh_max"],
                  fill_max_dist=None, device=None):
    """dsm [H, W] float32 (host; NaN / inf where empty) -> dict(level uint8 (0 ground, k flagged at level k, 255 empty), opened,
    ground, dtm, ndsm (float32), radius, dh, counts (valid, ground, object, empty, per_level), fill (the fill's statistics),
    seconds (classify, fill)).  Raises without a GPU: there is no CPU fallback."""
    import torch
    from . import hip_ops
    radius, dh = schedule(gsd, max_radius, slope, dh0, dh_max)
    fill_m, r_fill = fill_radius_cells(fill_max_dist, max_radius, float(gsd))
    if not torch.cuda.is_available():
        raise raster_stage.no_gpu("dtm", "ground-filter")
    dev = torch.device(device if device is not None else "cuda")
    dsm = np.ascontiguousarray(dsm, np.float32)
    d = torch.from_numpy(dsm).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.time()
    level, opened, st = hip_ops.dtm_classify(d, radius, dh)
    t1 = time.time()
    nan = torch.full_like(d, float("nan"))
    ground = torch.where(level == 0, d, nan)
    rgba = torch.zeros(d.shape + (4,), device=dev, dtype=torch.uint8)        # heights only: the colour output is dropped
    dtm, _, _, filled, fs = hip_ops.dsm_fill(ground, rgba, r_fill, max_cycles=FILL_MAX_CYCLES)
    t2 = time.time()
    if not fs.converged:
        raise FillNotConverged("dtm: the fill under the removed objects did not converge in %d V-cycles: largest residual %.3e m"
                               % (fs.cycles, fs.residual_height))
    dtm = dtm.cpu().numpy()
    ndsm = np.full(dsm.shape, np.nan, np.float32)
    both = np.isfinite(dsm) & np.isfinite(dtm)
    ndsm[both] = (dsm[both].astype(np.float64) - dtm[both].astype(np.float64)).astype(np.float32)
    K = len(radius)
    counts = dict(valid=int(st.cells_valid), ground=int(st.cells_ground), object=int(st.cells_object), empty=int(st.cells_empty),
                  per_level=[int(st.cells_level[k]) for k in range(1, K + 1)])
    fill = dict(max_dist=fill_m, r_cells=r_fill, cells_valid=int(fs.cells_valid), cells_filled=int(fs.cells_filled),
                cells_empty=int(fs.cells_empty), cycles=int(fs.cycles), residual_height=float(fs.residual_height))
    return dict(level=level.cpu().numpy(), opened=opened.cpu().numpy(), ground=ground.cpu().numpy(), dtm=dtm, ndsm=ndsm, radius=radius, dh=dh,
                counts=counts, fill=fill, seconds=dict(classify=t1 - t0, fill=t2 - t1), gsd=float(gsd),
                params=dict(max_radius=float(max_radius), slope=float(slope), dh0=float(dh0), dh_max=float(dh_max)))


def from_dsm(prefix, filled=False, max_radius=DEFAULTS["max_radius"], slope=DEFAULTS["slope"], dh0=DEFAULTS["dh0"],
             dh_max=DEFAULTS["dh_max"], fill_max_dist=None, device=None, out=None):
    """The DSM of dsm_whu.py at the path prefix (its gap-filled raster if `filled`) -> ground_filter()'s dict with `grid` and
    `source` added; written to `out` (a path prefix) if given."""
    import torch
    from .ortho import read_dsm
    if not torch.cuda.is_available():
        raise raster_stage.no_gpu("dtm", "ground-filter")
    dsm, grid = read_dsm(prefix, filled)
    res = ground_filter(dsm, grid.gsd, max_radius, slope, dh0, dh_max, fill_max_dist, device)
    res["grid"] = grid
    res["source"] = dict(prefix=prefix, filled=bool(filled))
    if out is not None:
        write_outputs(out, res)
    return res


# ---- files --------------------------------------------------------------------------------------------------------------
def output_paths(out):
    """The files of the ground filter, disjoint from dsm.output_paths(out) and dsm.fill_output_paths(out)."""
    return dict(dtm=out + "_dtm.tif", dtm_world=out + "_dtm.tfw", ndsm=out + "_ndsm.tif", ndsm_world=out + "_ndsm.tfw",
                ground=out + "_ground.png", ground_world=out + "_ground.pgw", json=out + "_dtm.json")


def ground_image(level):
    """level -> the L image: 0 empty, 255 ground, otherwise 16 x level (schedule() yields at most 11 levels: R <= 1024)."""
    level = np.asarray(level, np.uint8)
    if ((level > 15) & (level != 255)).any():
        raise ValueError("ground image: a level above 15 has no grey value")
    img = (level * 16).astype(np.uint8)
    img[level == 0] = 255
    img[level == 255] = 0
    return img


def level_from_image(img):
    img = np.asarray(img, np.uint8)
    level = (img // 16).astype(np.uint8)
    level[img == 255] = 0
    level[img == 0] = 255
    return level


def summary(res):
    return dict(grid=raster_stage.grid_summary(res["grid"]), z_ref=res["grid"].z_ref, source=res.get("source"), params=res["params"],
                schedule=dict(radius=[int(v) for v in res["radius"]], dh=[float(v) for v in res["dh"]]), counts=res["counts"],
                fill=res["fill"], seconds=res["seconds"])


def write_outputs(out, res):
    """The rasters, their world files and the JSON summary at the path prefix `out` -> output_paths(out)."""
    from PIL import Image
    paths = output_paths(out)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(res["dtm"], np.float32)).save(paths["dtm"], format="TIFF")
    Image.fromarray(np.ascontiguousarray(res["ndsm"], np.float32)).save(paths["ndsm"], format="TIFF")
    Image.fromarray(ground_image(res["level"])).save(paths["ground"], format="PNG")
    wf = world_file_text(res["grid"])
    for k in ("dtm_world", "ndsm_world", "ground_world"):
        with open(paths[k], "w") as f:
            f.write(wf)
    with open(paths["json"], "w") as f:
        json.dump(summary(res), f, indent=1)
        f.write("\n")
    return paths


def read_outputs(out):
    """-> (dtm float32, ndsm float32, level uint8) read back from the files of write_outputs."""
    from PIL import Image
    paths = output_paths(out)
    return (np.array(Image.open(paths["dtm"]), np.float32), np.array(Image.open(paths["ndsm"]), np.float32),
            level_from_image(np.array(Image.open(paths["ground"]))))


def build_parser():
    ap = argparse.ArgumentParser(description="Ground-filter a DSM into a bare-earth DTM and an nDSM")
    ap.add_argument("--dsm", required=True, metavar="PREFIX", help="path prefix of dsm_whu.py's output (<PREFIX>_dsm.tif, <PREFIX>_dsm.json)")
    ap.add_argument("--filled", action="store_true", help="use <PREFIX>_dsm_filled.tif (dsm_whu.py --fill_max_dist)")
    ap.add_argument("--max_radius", type=float, default=DEFAULTS["max_radius"], help="largest window radius in metres (objects wider than "
                    "twice this in both axes are kept as ground)")
    ap.add_argument("--slope", type=float, default=DEFAULTS["slope"], help="terrain slope the height threshold grows with")
    ap.add_argument("--dh0", type=float, default=DEFAULTS["dh0"], help="initial height threshold in metres")
    ap.add_argument("--dh_max", type=float, default=DEFAULTS["dh_max"], help="cap on the height threshold in metres")
    ap.add_argument("--fill_max_dist", type=float, default=None, metavar="METRES",
                    help="interpolate the terrain within this distance of ground (default: 2 x max_radius)")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="output path prefix (default: --dsm): <out>_dtm.tif, <out>_ndsm.tif, ...")
    return ap


def main(argv=None):
    args, out, t0 = raster_stage.open_main(build_parser, argv)
    res = from_dsm(args.dsm, args.filled, args.max_radius, args.slope, args.dh0, args.dh_max, args.fill_max_dist, out=out)
    g, c, f = res["grid"], res["counts"], res["fill"]
    print("dtm %d x %d cells at gsd %g: radii %s cells; %d valid cells, %d ground, %d object (per level %s), %d empty; classify %.3f s"
          % (g.W, g.H, g.gsd, [int(v) for v in res["radius"]], c["valid"], c["ground"], c["object"], c["per_level"], c["empty"],
             res["seconds"]["classify"]))
    print("fill within %g m (%g cells): %d cells interpolated, %d left empty; %d V-cycles, residual %.2e m, %.3f s; total_time = %.3f s"
          % (f["max_dist"], f["r_cells"], f["cells_filled"], f["cells_empty"], f["cycles"], f["residual_height"], res["seconds"]["fill"],
             time.time() - t0))
    return res


if __name__ == "__main__":
    main()
