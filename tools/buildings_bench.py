"""Building-extraction timing (csrc/dsm_buildings.hip): flags, tile labelling, border rounds and the table at the bench shape.

    python tools/buildings_bench.py [--H 2752 --W 1856] [--steps 10 --warmup 2] [--hole-fraction 0.1] [--boxes 400] [--blobs 150]

Input: the raster of tools/dsm_fill_bench.py (the fused 5-view scene rasterised in max mode at the pixel footprint of the
nadir view, about 2562 x 2751 cells, with its seeded disc holes), tools/dtm_bench.py's --boxes seeded boxes as "buildings" and
--blobs seeded discs of 8-40 cells radius with uniform noise of 4-9 m as "crowns"; the nDSM is dtm.ground_filter's at R = 64
cells with the fill at 128 cells (the run of tools/dtm_bench.py).  Parameters: the defaults of buildings.py at the raster's gsd.
Each group is timed with device events after warm-up, median and p10-p90 over --steps runs:
  flags     adamvs_bld_flags: the mask (8 B per cell), the opening's six passes (48 B) and the flag pass (the two masks, the DSM,
            the flag byte: 13 B; the neighbours at the stride are re-reads served by L2 and not counted): 69 B per cell
  tile      the tile phase of adamvs_bld_label (its own device events): the flag byte in, the parent word out: 5 B per cell
  rounds    the border rounds (device events, the one-word read-back of every round included): 40 B per pair and round
            (two parents in, the pair out and in again, two parents re-read and re-written); the number of rounds is reported
  compress  the final walk of every cell to its root: the parent word in, its root's word in: 8 B per cell (written only
            where it changes)
  number    the scan over the roots and the look-up of the labels in torch: no model
  table     adamvs_bld_table: label, flag byte and nDSM in: 9 B per cell
against 6.3 TB/s (measured HBM copy rate).  N (components) and B (buildings) are reported, and the host time of the selection
and of the outlines once.  CPU baseline on the 1024 x 1024 crop at the centre: the numpy restatement (tests/buildings_ref.py,
steps 1-6) and, where scipy imports, scipy.ndimage.label on the same mask (the labelling alone).  One JSON line.
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
BYTES = dict(flags=8 + 48 + 13, tile=5, compress=8, table=9)
PAIR_BYTES = 40


def add_blobs(d, count, seed=2):
    """Seeded discs of 8-40 cells radius whose valid cells rise by uniform noise of 4-9 m."""
    H, W = d.shape
    rng = np.random.default_rng(seed)
    for _ in range(count):
        ci, cj, rad = rng.integers(0, H), rng.integers(0, W), rng.uniform(8.0, 40.0)
        y0, y1, x0, x1 = max(0, int(ci - rad)), min(H, int(ci + rad) + 1), max(0, int(cj - rad)), min(W, int(cj + rad) + 1)
        y, x = np.mgrid[y0:y1, x0:x1]
        disc = (y - ci) ** 2 + (x - cj) ** 2 <= rad * rad
        d[y0:y1, x0:x1][disc] += rng.uniform(4.0, 9.0, disc.shape).astype(np.float32)[disc]       # NaN stays NaN


def stat(ms):
    ms = np.array(ms)
    return round(float(np.median(ms)), 3), [round(float(np.percentile(ms, 10)), 3), round(float(np.percentile(ms, 90)), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--hole-fraction", type=float, default=0.1)
    ap.add_argument("--boxes", type=int, default=400)
    ap.add_argument("--blobs", type=int, default=150)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("buildings_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from ada_mvs_amd import _lib, buildings, dsm, dtm, hip_ops
    from dsm_bench import fused_scene
    from dsm_fill_bench import punch_holes
    from dtm_bench import add_boxes, timed
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
    add_blobs(d, args.blobs)
    del xyz, rgb, b, res, rgba
    gf = dtm.ground_filter(d, grid.gsd, max_radius=64.5 * grid.gsd, fill_max_dist=128.0 * grid.gsd)
    nd = gf["ndsm"]
    scene_s = time.time() - t0
    del gf
    p = buildings.parameters(grid.gsd)
    dev = torch.device("cuda")
    dd, nn = torch.from_numpy(d).to(dev), torch.from_numpy(nd).to(dev)
    n = grid.W * grid.H
    ws = torch.empty(int(_lib.load().adamvs_bld_workspace_bytes(grid.W, grid.H)), device=dev, dtype=torch.uint8)
    out = {"workload": "buildings", "W": grid.W, "H": grid.H, "cells": n, "gsd": grid.gsd, "boxes": args.boxes, "blobs": args.blobs,
           "r_open": p["r_open"], "stride": p["stride"], "steps": args.steps, "warmup": args.warmup, "bytes_per_cell": BYTES,
           "bytes_per_pair_round": PAIR_BYTES}

    def roof(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / HBM_BPS, 3) if ms > 0 else None

    flags, med, band = timed(lambda: hip_ops.bld_flags(dd, nn, p["min_height"], p["r_open"], p["stride"], p["smooth_tol"], workspace=ws),
                             args.steps, args.warmup)
    out["flags"] = {"ms_median": round(med, 3), "ms_p10_p90": band, "hbm_roof_fraction": roof(n * BYTES["flags"], med)}
    # the labelling: the C call reports its three groups from device events; the numbering in torch is the rest of the call
    tile, rounds, compress, whole = [], [], [], []
    for it in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        comp, N, st = hip_ops.bld_label(flags, workspace=ws)
        e1.record()
        e1.synchronize()
        if it >= args.warmup:
            tile.append(st.ms_tile)
            rounds.append(st.ms_rounds)
            compress.append(st.ms_compress)
            whole.append(e0.elapsed_time(e1))
    pairs, nr = int(st.pairs), int(st.rounds)
    med, band = stat(tile)
    out["tile"] = {"ms_median": med, "ms_p10_p90": band, "tiles": int(st.tiles), "hbm_roof_fraction": roof(n * BYTES["tile"], med)}
    med, band = stat(rounds)
    out["rounds"] = {"ms_median": med, "ms_p10_p90": band, "rounds": nr, "pairs": pairs,
                     "hbm_roof_fraction": roof((nr + 1) * pairs * PAIR_BYTES, med)}
    med, band = stat(compress)
    out["compress"] = {"ms_median": med, "ms_p10_p90": band, "hbm_roof_fraction": roof(n * BYTES["compress"], med)}
    med_whole, band = stat(whole)
    out["label_call"] = {"ms_median": med_whole, "ms_p10_p90": band,
                         "number_ms": round(med_whole - out["tile"]["ms_median"] - out["rounds"]["ms_median"] - out["compress"]["ms_median"], 3)}
    table, med, band = timed(lambda: hip_ops.bld_table(flags, nn, comp, N), args.steps, args.warmup)
    out["table"] = {"ms_median": round(med, 3), "ms_p10_p90": band, "hbm_roof_fraction": roof(n * BYTES["table"], med)}
    tab = table.cpu().numpy()
    tdict = {name: tab[k] for k, name in enumerate(buildings.COLUMNS)}
    t1 = time.time()
    keep, counts = buildings.select(tdict, grid.gsd, p["min_area"], p["min_smooth"])
    label = buildings.relabel(comp.cpu().numpy(), keep)
    t2 = time.time()
    polys = buildings.polygons(label, grid)
    t3 = time.time()
    out.update(N=int(N), B=counts["buildings"], rejected_small=counts["rejected_small"], rejected_rough=counts["rejected_rough"],
               largest_component_cells=int(tdict["cells"].max()) if N else 0,
               host={"select_relabel_s": round(t2 - t1, 3), "outlines_s": round(t3 - t2, 3), "rings": sum(len(q["rings"]) for q in polys),
                     "vertices": sum(len(r) for q in polys for r in q["rings"])})
    # CPU baseline on the central 1024 x 1024 crop
    from buildings_ref import components_ref, extract_ref
    i0, j0 = max(0, grid.H // 2 - 512), max(0, grid.W // 2 - 512)
    crop = (slice(i0, i0 + 1024), slice(j0, j0 + 1024))
    t1 = time.time()
    ref = extract_ref(d[crop], nd[crop], grid.gsd)
    cpu = {"crop": [i0, j0, 1024, 1024], "numpy_restatement_s": round(time.time() - t1, 2), "components": ref["N"], "buildings": ref["counts"]["buildings"]}
    mask = ref["flags"] >= 2
    t1 = time.time()
    components_ref(mask)
    cpu["flood_fill_alone_s"] = round(time.time() - t1, 2)
    try:
        from scipy import ndimage
        t1 = time.time()
        _, n_scipy = ndimage.label(mask)
        cpu["scipy_ndimage_label_s"] = round(time.time() - t1, 4)
        cpu["scipy_components"] = int(n_scipy)
    except ImportError:
        cpu["scipy_ndimage_label_s"] = None
    out["cpu_crop"] = cpu
    out["scene_s"] = round(scene_s, 1)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
