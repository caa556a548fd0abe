"""Contour timing (csrc/dsm_contours.hip): surface, count and scan, segments, the ranking rounds and the lines at the bench shape.

    python tools/contours_bench.py [--H 2752 --W 1856] [--steps 10 --warmup 2] [--hole-fraction 0.1] [--boxes 400] [--interval 1.0]

Input: the DTM of the bench scene: the raster of tools/dtm_bench.py (the fused 5-view scene rasterised at the pixel footprint of
the nadir view, about 2562 x 2751 cells, with seeded holes and boxes) through dtm.ground_filter at R = 64 cells.  Parameters:
interval 1 m from base 0, one smoothing pass.  Each group is timed with device events after warm-up, median and p10-p90 over
--steps runs:
  surface   adamvs_contour_surface: the quantise pass (z in, s out: 8 B per cell) and 8 B per cell and smoothing pass (the eight
            neighbours are re-reads served by the caches and not counted)
  count     adamvs_contour_count (its own device events): the tile pass (s in, count out: 8 B per cell), the workgroup scans (count
            in, offsets out: 8 B) and the add pass (offsets in and out: 8 B): 24 B per cell
  segments  adamvs_contour_segments: 20 B written per segment; the reads are a binary search in the offsets and twelve samples
            gathered from L2: no honest byte model, segments per second instead
  rank      adamvs_contour_rank (its own device events, the read-back of every fourth round included): every round is one gather
            of 8 B per segment at an address that halves its distance to the head: no byte model, segments x launched rounds per
            second instead; the rounds that moved something and the rounds launched are reported
  lines     adamvs_contour_lines (three read-backs of a word included): 24 B written per vertex; the reads are gathers through
            start: vertices per second
against 6.3 TB/s (measured HBM copy rate) where a model is stated.  N, M, the longest line and the rounds are reported, and the
host time of the coordinates, lengths and GeoJSON text once.  CPU baseline on the 512 x 512 crop at the centre: the numpy
restatement (tests/contours_ref.py).  One JSON line.
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
BYTES = dict(surface_quant=8, surface_pass=8, count=24, segment_out=20, vertex_out=24)


def stat(ms):
    ms = np.array(ms)
    return round(float(np.median(ms)), 3), [round(float(np.percentile(ms, 10)), 3), round(float(np.percentile(ms, 90)), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--hole-fraction", type=float, default=0.1)
    ap.add_argument("--boxes", type=int, default=400)
    ap.add_argument("--interval", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("contours_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from ada_mvs_amd import contours, dsm, dtm, hip_ops
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
    del xyz, rgb, b, res, rgba
    z = dtm.ground_filter(d, grid.gsd, max_radius=64.5 * grid.gsd, fill_max_dist=128.0 * grid.gsd)["dtm"]
    scene_s = time.time() - t0
    p = contours.parameters(interval=args.interval)
    dev = torch.device("cuda")
    zz = torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(dev)
    n = grid.W * grid.H
    out = {"workload": "contours", "W": grid.W, "H": grid.H, "cells": n, "gsd": grid.gsd, "boxes": args.boxes, "interval": p["interval"],
           "smooth_passes": p["smooth_passes"], "steps": args.steps, "warmup": args.warmup, "bytes": BYTES}

    def roof(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / HBM_BPS, 3) if ms > 0 else None

    def rate(items, ms):
        return round(items / (ms * 1e-3)) if ms > 0 else None

    (s, info), med, band = timed(lambda: hip_ops.contour_surface(zz, grid.z_ref, p["smooth_passes"]), args.steps, args.warmup)
    nbytes = n * (BYTES["surface_quant"] + p["smooth_passes"] * BYTES["surface_pass"])
    out["surface"] = {"ms_median": round(med, 3), "ms_p10_p90": band, "bytes_per_cell": nbytes // n, "hbm_roof_fraction": roof(nbytes, med)}
    s_min, s_max, bad = (int(v) for v in info.cpu().tolist())
    valid = int((s != -2 ** 31).sum())
    if bad:
        raise SystemExit("contours_bench: %d cells out of range" % bad)
    lev, ns = contours.level_table(s_min, s_max, grid.z_ref, p["interval"], p["base"], p["smooth_passes"])
    out.update(valid_cells=valid, levels=len(lev), z_min=round(grid.z_ref + s_min / p["scale"], 3), z_max=round(grid.z_ref + s_max / p["scale"], 3))
    count_ms, rank_ms, seg_ms, lines_ms = [], [], [], []
    for it in range(args.warmup + args.steps):
        count, N, ws, st = hip_ops.contour_count(s, lev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        seg = hip_ops.contour_segments(s, lev, N, ws)
        ev[1].record()
        start, rank, closed, M, ws2, st = hip_ops.contour_rank(seg[4], stats=st)
        ev[2].record()
        tables = hip_ops.contour_lines(s, lev, seg, start, rank, closed, M, ws2)
        ev[3].record()
        ev[3].synchronize()
        if it >= args.warmup:
            count_ms.append(st.ms_count)
            rank_ms.append(st.ms_rank)
            seg_ms.append(ev[0].elapsed_time(ev[1]))
            lines_ms.append(ev[2].elapsed_time(ev[3]))
    med, band = stat(count_ms)
    out["count"] = {"ms_median": med, "ms_p10_p90": band, "bytes_per_cell": BYTES["count"], "hbm_roof_fraction": roof(n * BYTES["count"], med)}
    med, band = stat(seg_ms)
    out["segments"] = {"ms_median": med, "ms_p10_p90": band, "segments_per_s": rate(N, med), "out_roof_fraction": roof(N * BYTES["segment_out"], med)}
    med, band = stat(rank_ms)
    out["rank"] = {"ms_median": med, "ms_p10_p90": band, "rounds": int(st.rounds), "rounds_min": int(st.rounds_min), "rounds_dist": int(st.rounds_dist),
                   "rounds_launched": int(st.launched), "segment_rounds_launched_per_s": rate(N * int(st.launched), med)}
    med, band = stat(lines_ms)
    out["lines"] = {"ms_median": med, "ms_p10_p90": band, "vertices_per_s": rate(N + M, med), "out_roof_fraction": roof((N + M) * BYTES["vertex_out"], med)}
    line_first, _, line_level, line_closed, vertex = (t.cpu().numpy() for t in tables)
    t1 = time.time()
    xy = contours.vertex_coordinates(vertex, grid)
    length = contours.line_lengths(xy, line_first)
    order = contours.select(length, line_level, p["min_length"])
    t2 = time.time()
    text = contours.geojson_text(contours.features(xy, line_first, line_level, line_closed, length, order, ns, p))
    t3 = time.time()
    out.update(N=int(N), M=int(M), closed_lines=int(line_closed.sum()), longest_line_vertices=int(np.diff(line_first).max()) if M else 0,
               total_length_m=round(float(length.sum()), 1),
               host={"coordinates_lengths_s": round(t2 - t1, 3), "geojson_text_s": round(t3 - t2, 3), "geojson_bytes": len(text)})
    # CPU baseline on the central 512 x 512 crop
    import contours_ref
    i0, j0 = max(0, grid.H // 2 - 256), max(0, grid.W // 2 - 256)
    t1 = time.time()
    ref = contours_ref.trace(z[i0:i0 + 512, j0:j0 + 512], grid.z_ref, p["smooth_passes"], lev)
    out["cpu_crop"] = {"crop": [i0, j0, 512, 512], "numpy_restatement_s": round(time.time() - t1, 2), "segments": ref["N"], "lines": ref["M"]}
    out["scene_s"] = round(scene_s, 1)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
