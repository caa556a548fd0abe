"""DSM gap fill timing (csrc/dsm_fill.hip): distance transform + multigrid solve at the bench shape.

    python tools/dsm_fill_bench.py [--H 2752 --W 1856] [--r 64] [--steps 10 --warmup 2] [--hole-fraction 0.1]

Input: the fused 5-view scene of tools/dsm_bench.py rasterised (max mode) at the pixel footprint of the nadir view (about
2562 x 2751 cells), with seeded disc holes of radius 4-60 cells punched in until they cover about --hole-fraction of the
valid cells.  The whole fill (one adamvs_dsm_fill call: distance, V-cycles with their per-cycle residual read-back, output)
is timed with device events after warm-up; median and p10-p90 over --steps runs.  Byte model of the fine-level passes per
V-cycle (class byte 1 B, height 8 B, colours 16 B per cell): residual 49 B (reads 25, writes the scaled residual 24),
restriction 24 B, prolongation 49 B, 4 red-black half-sweeps 37 B each (read every cell, write half): 270 B per cell and
cycle, plus 38 B per cell for the distance passes and 33 B for the output; against 6.3 TB/s (measured HBM copy rate).
CPU baseline: the fp64 numpy reference (tests/dsm_fill_ref.py) on the 1024 x 1024 crop at the centre of the raster.
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

TARGET_MS = 30.0
HBM_BPS = 6.3e12
FINE_BYTES_PER_CYCLE = 270
EDT_BYTES, OUTPUT_BYTES = 38, 33


def punch_holes(d, rgba, fraction, seed=0):
    """Seeded discs of radius 4-60 cells cleared until they cover `fraction` of the valid cells."""
    H, W = d.shape
    rng = np.random.default_rng(seed)
    valid0 = np.isfinite(d)
    target = fraction * valid0.sum()
    ii, jj = np.nonzero(valid0)
    removed = 0
    while removed < target:
        k = rng.integers(0, len(ii))
        ci, cj, rad = ii[k], jj[k], rng.uniform(4, 60)
        y0, y1, x0, x1 = max(0, int(ci - rad)), min(H, int(ci + rad) + 1), max(0, int(cj - rad)), min(W, int(cj + rad) + 1)
        y, x = np.mgrid[y0:y1, x0:x1]
        m = ((y - ci) ** 2 + (x - cj) ** 2 <= rad * rad) & np.isfinite(d[y0:y1, x0:x1])
        removed += int(m.sum())
        d[y0:y1, x0:x1][m] = np.nan
        rgba[y0:y1, x0:x1][m] = 0
    return removed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--r", type=float, default=64.0)
    ap.add_argument("--hole-fraction", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dsm_fill_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from ada_mvs_amd import dsm, hip_ops
    from dsm_bench import fused_scene
    t0 = time.time()
    xyz, rgb, per_view, footprint = fused_scene(args.H, args.W)
    lo, hi = torch.aminmax(xyz, dim=0)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    grid = dsm.grid_for_bounds(lo, hi, round(footprint, 4), np.floor(lo[2]))
    b = dsm.DsmBuilder(grid, "max")
    b.add(xyz, rgb)
    res = b.finish()
    d, rgba = res["dsm"].copy(), res["rgba"].copy()
    valid_before = int(np.isfinite(d).sum())
    punched = punch_holes(d, rgba, args.hole_fraction)
    scene_s = time.time() - t0
    dev = torch.device("cuda")
    dd, cc = torch.from_numpy(d).to(dev), torch.from_numpy(rgba).to(dev)
    ws = torch.empty(_ws_bytes(grid), device=dev, dtype=torch.uint8)

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = hip_ops.dsm_fill(dd, cc, args.r, workspace=ws)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for _ in range(args.warmup):
        once()
    runs = [once() for _ in range(args.steps)]
    ms = np.array([r[0] for r in runs])
    st = runs[-1][1][4]
    n = grid.W * grid.H
    med = float(np.median(ms))
    model = n * (EDT_BYTES + OUTPUT_BYTES + FINE_BYTES_PER_CYCLE * st.cycles)
    out = {"workload": "dsm_fill", "W": grid.W, "H": grid.H, "cells": n, "gsd": grid.gsd, "r_cells": args.r,
           "valid_before_holes": valid_before, "hole_cells": punched, "cells_valid": st.cells_valid, "cells_filled": st.cells_filled,
           "cells_empty": st.cells_empty, "cycles": st.cycles, "converged": bool(st.converged), "residual_height": st.residual_height,
           "residual_colour": st.residual_colour, "steps": args.steps, "warmup": args.warmup, "ms_median": round(med, 3),
           "ms_p10_p90": [round(float(np.percentile(ms, 10)), 3), round(float(np.percentile(ms, 90)), 3)],
           "fine_pass_bytes_model": int(model), "hbm_roof_fraction": round(model / (med * 1e-3) / HBM_BPS, 3),
           "target_ms": TARGET_MS, "meets_target": med <= TARGET_MS}
    # CPU baseline: the numpy reference on the central 1024 x 1024 crop
    from dsm_fill_ref import fill_ref
    i0, j0 = max(0, grid.H // 2 - 512), max(0, grid.W // 2 - 512)
    crop = (slice(i0, i0 + 1024), slice(j0, j0 + 1024))
    t1 = time.time()
    ref = fill_ref(d[crop], rgba[crop], args.r)
    out["cpu_numpy_crop"] = {"crop": [i0, j0, 1024, 1024], "cells_filled": ref["cells_filled"], "seconds": round(time.time() - t1, 2)}
    out["scene_s"] = round(scene_s, 1)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


def _ws_bytes(grid):
    from ada_mvs_amd import _lib
    return int(_lib.load().adamvs_dsm_fill_workspace_bytes(grid.W, grid.H))


if __name__ == "__main__":
    main()
