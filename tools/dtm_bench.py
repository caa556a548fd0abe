"""Ground-filter timing (csrc/dsm_dtm.hip): the progressive morphological filter at the bench shape, and the fill under it.

    python tools/dtm_bench.py [--H 2752 --W 1856] [--steps 10 --warmup 2] [--hole-fraction 0.1] [--boxes 400]

Input: the raster of tools/dsm_fill_bench.py (the fused 5-view scene rasterised in max mode at the pixel footprint of the
nadir view, about 2562 x 2751 cells, with its seeded disc holes) plus --boxes seeded boxes of 10-120 cells a side and
+3-30 m as "buildings".  One adamvs_dtm_classify call (all levels, the flag step and the read-back of the counts) is timed
with device events after warm-up at R = 16, 64, 256 and 1024 cells; median and p10-p90 over --steps runs, and the median per
level; one opening alone (adamvs_dsm_open) at r = 1, 4, 16, 64, 256 and 1024 shows how the time of a level depends on r.
Then the fill of the ground cells of the R = 64 run (adamvs_dsm_fill at r = 2 R, heights only), timed the same way.
Byte model per level and cell: the four min / max passes read and write fp32 (4 x 8 B) and the flag step folded into the last
one reads Z_{k-1} (4 B) and reads and writes the level byte (2 B): 38 B; the two transposes this implementation adds move
another 16 B (54 B moved, halo re-reads not counted); against 6.3 TB/s (measured HBM copy rate).
CPU baseline: the numpy restatement (tests/dtm_ref.py pmf) at R = 64 on the 1024 x 1024 crop at the centre of the raster.
One JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import ada_mvs_amd  # noqa: E402,F401

HBM_BPS = 6.3e12
MODEL_BYTES, MOVED_BYTES = 4 * 8 + 6, 6 * 8 + 6
RADII = (16, 64, 256, 1024)


def add_boxes(d, count, seed=1):
    """Seeded boxes of 10-120 cells a side, +3-30 m, added to the valid cells they cover."""
    H, W = d.shape
    rng = np.random.default_rng(seed)
    for _ in range(count):
        h, w = rng.integers(10, 121, 2)
        i0, j0, dz = rng.integers(0, H - h), rng.integers(0, W - w), rng.uniform(3.0, 30.0)
        d[i0:i0 + h, j0:j0 + w] += np.float32(dz)          # NaN stays NaN


def timed(fn, steps, warmup):
    import torch
    out = None
    ms = []
    for it in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    return out, float(np.median(ms)), [round(float(np.percentile(ms, 10)), 3), round(float(np.percentile(ms, 90)), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--hole-fraction", type=float, default=0.1)
    ap.add_argument("--boxes", type=int, default=400)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dtm_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from ada_mvs_amd import _lib, dsm, dtm, hip_ops
    from dsm_bench import fused_scene
    from dsm_fill_bench import punch_holes
    t0 = time.time()
    xyz, rgb, _, footprint = fused_scene(args.H, args.W)
    lo, hi = torch.aminmax(xyz, dim=0)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    grid = dsm.grid_for_bounds(lo, hi, round(footprint, 4), np.floor(lo[2]))
    b = dsm.DsmBuilder(grid, "max")
    b.add(xyz, rgb)
    res = b.finish()
    d, rgba = res["dsm"].copy(), res["rgba"].copy()
    punch_holes(d, rgba, args.hole_fraction)
    add_boxes(d, args.boxes)
    scene_s = time.time() - t0
    del xyz, rgb, b, res
    dev = torch.device("cuda")
    dd = torch.from_numpy(d).to(dev)
    n = grid.W * grid.H
    ws = torch.empty(int(_lib.load().adamvs_dtm_workspace_bytes(grid.W, grid.H)), device=dev, dtype=torch.uint8)
    out = {"workload": "dtm", "W": grid.W, "H": grid.H, "cells": n, "gsd": grid.gsd, "boxes": args.boxes, "steps": args.steps,
           "warmup": args.warmup, "model_bytes_per_cell_level": MODEL_BYTES, "moved_bytes_per_cell_level": MOVED_BYTES, "classify": []}
    ground = None
    for R in RADII:
        radius, dh = dtm.schedule(grid.gsd, max_radius=(R + 0.5) * grid.gsd)
        assert int(radius[-1]) == R
        (level, _, st), med, band = timed(lambda: hip_ops.dtm_classify(dd, radius, dh, workspace=ws), args.steps, args.warmup)
        K = len(radius)
        out["classify"].append({"R": R, "levels": K, "ms_median": round(med, 3), "ms_p10_p90": band, "ms_per_level": round(med / K, 3),
                                "hbm_roof_fraction_model": round(n * MODEL_BYTES * K / (med * 1e-3) / HBM_BPS, 3),
                                "hbm_roof_fraction_moved": round(n * MOVED_BYTES * K / (med * 1e-3) / HBM_BPS, 3),
                                "cells_valid": st.cells_valid, "cells_ground": st.cells_ground, "cells_object": st.cells_object})
        if R == 64:
            ground = torch.where(level == 0, dd, torch.full_like(dd, float("nan")))
    # one opening (six passes, no flag step) per radius: is the time of a level flat in r?
    out["open"] = []
    for r in (1, 4, 16, 64, 256, 1024):
        _, med, band = timed(lambda: hip_ops.dsm_open(dd, r, workspace=ws), args.steps, args.warmup)
        out["open"].append({"r": r, "ms_median": round(med, 3), "ms_p10_p90": band})
    zero = torch.zeros(grid.H, grid.W, 4, device=dev, dtype=torch.uint8)
    fws = torch.empty(int(_lib.load().adamvs_dsm_fill_workspace_bytes(grid.W, grid.H)), device=dev, dtype=torch.uint8)
    fill, med, band = timed(lambda: hip_ops.dsm_fill(ground, zero, 128.0, workspace=fws), max(args.steps // 2, 1), 1)
    fs = fill[4]
    out["fill"] = {"r_cells": 128.0, "ms_median": round(med, 3), "ms_p10_p90": band, "cycles": fs.cycles, "converged": bool(fs.converged),
                   "cells_filled": fs.cells_filled, "cells_empty": fs.cells_empty, "residual_height": fs.residual_height}
    # CPU baseline: the numpy restatement at R = 64 on the central 1024 x 1024 crop
    from dtm_ref import pmf
    i0, j0 = max(0, grid.H // 2 - 512), max(0, grid.W // 2 - 512)
    radius, dh = dtm.schedule(grid.gsd, max_radius=64.5 * grid.gsd)
    t1 = time.time()
    ref = pmf(d[i0:i0 + 1024, j0:j0 + 1024], radius, dh)
    out["cpu_numpy_crop"] = {"crop": [i0, j0, 1024, 1024], "R": 64, "cells_object": ref["counts"]["object"], "seconds": round(time.time() - t1, 2)}
    out["scene_s"] = round(scene_s, 1)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
