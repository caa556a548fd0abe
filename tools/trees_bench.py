"""Tree-detection timing (csrc/dsm_trees.hip): surface, parents, jump rounds, crowns and the table at the bench shape.

    python tools/trees_bench.py [--H 2752 --W 1856] [--steps 10 --warmup 2] [--hole-fraction 0.1] [--boxes 400] [--blobs 150]

Input: the raster and the building labels of tools/buildings_bench.py (the fused 5-view scene rasterised at the pixel footprint of
the nadir view, about 2562 x 2751 cells, with seeded holes, boxes as "buildings" and noise discs as "crowns"; the nDSM of
dtm.ground_filter at R = 64 cells; buildings.extract with its defaults).  Parameters: the defaults of trees.py at the raster's gsd.
Each group is timed with device events after warm-up, median and p10-p90 over --steps runs:
  surface   adamvs_tree_surface: the mask pass (nDSM and building label in, mask byte, q and s out: 17 B per cell) and 8 B per
            cell and smoothing pass (the eight neighbours are re-reads served by the caches and not counted)
  parents   adamvs_tree_parents (its own device events).  No honest byte model: the tile is read once (4 B) and written once (4 B),
            the rest is the window searches, whose reads come from L2.  Reported instead: the candidates (8-neighbour local
            maxima) and the window cells read, per second
  jump      the rounds of adamvs_tree_roots (device events, the read-back of every fourth round included): 12 B per cell and
            launched round (the pointer in, one gathered ancestor in, the new pointer out; the further hops of the cells that
            have not arrived are gathers a few cells away and not counted); the rounds that moved a pointer and the rounds
            launched are reported
  number    the scan over the tops in torch: the rest of the tree_roots call, no model
  crowns    adamvs_tree_crowns: s and root in, label out: 12 B per cell (s and the number at the top are gathers over few cells)
  table     adamvs_tree_table: label in; q and root in where a label is: at most 12 B per cell
against 6.3 TB/s (measured HBM copy rate).  T (tops) and K (trees) are reported, and the host time of the selection and of the
outlines once.  CPU baseline on the 512 x 512 crop at the centre: the numpy restatement (tests/trees_ref.py).  One JSON line.
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
BYTES = dict(surface_mask=17, surface_pass=8, jump_round=12, crowns=12, table=12)
JUMP_CHUNK = 4                                      # TREE_JUMP_CHUNK of csrc/dsm_trees.hip: rounds launched per read-back


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
        raise SystemExit("trees_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from ada_mvs_amd import _lib, buildings, dsm, dtm, hip_ops, trees
    from buildings_bench import add_blobs
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
    nd = dtm.ground_filter(d, grid.gsd, max_radius=64.5 * grid.gsd, fill_max_dist=128.0 * grid.gsd)["ndsm"]
    building = buildings.extract(d, nd, grid.gsd, grid=grid)["label"]
    scene_s = time.time() - t0
    p = trees.parameters(grid.gsd)
    dev = torch.device("cuda")
    nn, bb = torch.from_numpy(nd).to(dev), torch.from_numpy(building).to(dev)
    n = grid.W * grid.H
    ws = torch.empty(int(_lib.load().adamvs_tree_workspace_bytes(grid.W, grid.H)), device=dev, dtype=torch.uint8)
    out = {"workload": "trees", "W": grid.W, "H": grid.H, "cells": n, "gsd": grid.gsd, "boxes": args.boxes, "blobs": args.blobs,
           "building_cells": int((building > 0).sum()), "steps": args.steps, "warmup": args.warmup, "bytes": BYTES,
           "roots_design": "plain double-buffered jumping, %d parents per round" % _lib.TREE_JUMP_HOPS}

    def roof(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / HBM_BPS, 3) if ms > 0 else None

    (mask, q, s, s_max), med, band = timed(lambda: hip_ops.tree_surface(nn, bb, p["min_height"], p["smooth_passes"], workspace=ws),
                                           args.steps, args.warmup)
    nbytes = n * (BYTES["surface_mask"] + p["smooth_passes"] * BYTES["surface_pass"])
    out["surface"] = {"ms_median": round(med, 3), "ms_p10_p90": band, "bytes_per_cell": nbytes // n, "hbm_roof_fraction": roof(nbytes, med)}
    s_max = int(s_max.item())
    p = trees.parameters(grid.gsd, s_max=s_max)     # raises if the tallest cell's window exceeds ADAMVS_TREE_MAX_RADIUS
    thr = trees.window_table(grid.gsd, p["radius_min"], p["radius_slope"], p["smooth_passes"], s_max)
    out.update(canopy_cells=int(mask.sum()), s_max=s_max, r_cap=p["r_cap"])
    parents_ms, jump_ms, roots_call = [], [], []
    for it in range(args.warmup + args.steps):
        parent, st = hip_ops.tree_parents(s, thr, workspace=ws)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        root, number, T, st = hip_ops.tree_roots(parent, workspace=ws, stats=st)
        e1.record()
        e1.synchronize()
        if it >= args.warmup:
            parents_ms.append(st.ms_parents)
            jump_ms.append(st.ms_jump)
            roots_call.append(e0.elapsed_time(e1))
    med, band = stat(parents_ms)
    cand, swept = int(st.candidates), int(st.window_cells)
    out["parents"] = {"ms_median": med, "ms_p10_p90": band, "candidates": cand, "window_cells": swept,
                      "candidates_per_s": round(cand / (med * 1e-3)) if med > 0 else None,
                      "window_cells_per_s": round(swept / (med * 1e-3)) if med > 0 else None,
                      "window_cells_per_candidate": round(swept / cand, 1) if cand else None}
    med, band = stat(jump_ms)
    launched = -(-(int(st.rounds) + 1) // JUMP_CHUNK) * JUMP_CHUNK
    out["jump"] = {"ms_median": med, "ms_p10_p90": band, "rounds": int(st.rounds), "rounds_launched": launched,
                   "hbm_roof_fraction": roof(n * BYTES["jump_round"] * launched, med)}
    med_call, band = stat(roots_call)
    out["roots_call"] = {"ms_median": med_call, "ms_p10_p90": band, "number_ms": round(med_call - med, 3)}
    (crowns, unassigned), med, band = timed(lambda: hip_ops.tree_crowns(s, root, number, p["ratio_pm"], p["rc2"]), args.steps, args.warmup)
    out["crowns"] = {"ms_median": round(med, 3), "ms_p10_p90": band, "hbm_roof_fraction": roof(n * BYTES["crowns"], med)}
    table, med, band = timed(lambda: hip_ops.tree_table(crowns, q, s, root, T), args.steps, args.warmup)
    out["table"] = {"ms_median": round(med, 3), "ms_p10_p90": band, "hbm_roof_fraction": roof(n * BYTES["table"], med)}
    tab = table.cpu().numpy()
    tdict = {name: tab[k] for k, name in enumerate(trees.COLUMNS)}
    t1 = time.time()
    keep, counts = trees.select(tdict, grid.gsd, p["min_crown_area"])
    lut = np.zeros(T + 1, np.int32)
    lut[1:][keep] = np.arange(1, counts["trees"] + 1, dtype=np.int32)
    label = lut[crowns.cpu().numpy()]
    t2 = time.time()
    polys = trees.crown_polygons(label, grid)
    t3 = time.time()
    out.update(T=int(T), K=counts["trees"], rejected_small=counts["rejected_small"], labelled_cells=int((label > 0).sum()),
               unassigned_cells=int(unassigned.item()), largest_crown_cells=int(tdict["cells"].max()) if T else 0,
               host={"select_relabel_s": round(t2 - t1, 3), "outlines_s": round(t3 - t2, 3), "parts": sum(len(q_["polygons"]) for q_ in polys)})
    # CPU baseline on the central 512 x 512 crop
    from trees_ref import detect_ref
    i0, j0 = max(0, grid.H // 2 - 256), max(0, grid.W // 2 - 256)
    crop = (slice(i0, i0 + 512), slice(j0, j0 + 512))
    t1 = time.time()
    ref = detect_ref(nd[crop], grid.gsd, building[crop])
    out["cpu_crop"] = {"crop": [i0, j0, 512, 512], "numpy_restatement_s": round(time.time() - t1, 2), "tops": ref["T"], "trees": ref["counts"]["trees"]}
    out["scene_s"] = round(scene_s, 1)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
