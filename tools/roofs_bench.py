"""Roof-plane timing (csrc/dsm_roofs.hip): links, tile labelling, border rounds, moments, growth and residuals at the bench shape.

    python tools/roofs_bench.py [--H 2752 --W 1856] [--steps 10 --warmup 2] [--hole-fraction 0.1] [--boxes 400] [--blobs 150]

Input: the raster of tools/buildings_bench.py (the fused 5-view scene rasterised at the nadir footprint, about 2562 x 2751
cells, with seeded holes, tools/dtm_bench.py's --boxes seeded boxes and --blobs seeded noise discs) with pitched roofs added:
every box gets, in the order of its seed, a gable (ridge along its longer side), a hip-less pyramid, a shed or stays flat, at a
pitch of 0.3 - 0.7.  The nDSM is dtm.ground_filter's as in buildings_bench.py, the building labels are buildings.extract's at
its defaults, the roof parameters are the defaults of roofs.py at the raster's gsd.  Each group is timed with device events
after warm-up, median and p10-p90 over --steps runs:
  links      adamvs_roof_links: Z and the building label in, the link byte out: 9 B per cell (the neighbours at the stride of
             the cell, of its east and of its south neighbour are re-reads served by L2 and not counted)
  tile       the tile phase of adamvs_roof_label (its own device events): the link byte in, the parent word out: 5 B per cell
  rounds     the border rounds (device events, the one-word read-back of every look included): 41 B per pair and look (the
             link byte and two parents in, the pair out and in again, two parents re-read and re-written)
  compress   the final walk of every cell to its root: 8 B per cell
  number     the scan over the roots and the look-up of the segment numbers in torch: no model
  moments    adamvs_roof_moments on the segments, and again on the grown labels: label, Z and building in: 12 B per cell
  grow       adamvs_roof_grow, all grow_rounds rounds in one call (no early stop): per round the label in and out, the building
             label and Z in: 16 B per cell and round (the four neighbours' labels are re-reads served by L2)
  residuals  adamvs_roof_residuals: label and Z in: 8 B per cell
against 6.3 TB/s (measured HBM copy rate).  The counts (S segments, P kept, R planes), the border rounds, the growth rounds
that labelled something, and the host times of one roofs.extract (plane fits, merge, outlines) are reported.  One JSON line.
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
BYTES = dict(links=9, tile=5, compress=8, moments=12, grow_round=16, residuals=8)
PAIR_BYTES = 41


def add_pitched_boxes(d, count, seed=1):
    """tools/dtm_bench.py's add_boxes (the same seeded footprints and heights) with a roof shape on every box: by turns a gable
    along the longer side, a pyramid, a shed, none; pitch 0.3 - 0.7 (a second generator, so the boxes stay those of the seed)."""
    H, W = d.shape
    rng, shape_rng = np.random.default_rng(seed), np.random.default_rng(seed + 1000)
    for k in range(count):
        h, w = rng.integers(10, 121, 2)
        i0, j0, dz = rng.integers(0, H - h), rng.integers(0, W - w), rng.uniform(3.0, 30.0)
        pitch = shape_rng.uniform(0.3, 0.7)
        i, j = np.mgrid[0:h, 0:w].astype(np.float64)
        di, dj = np.minimum(i, h - 1 - i), np.minimum(j, w - 1 - j)      # cells from the nearer eave
        rise = (di if w >= h else dj, np.minimum(di, dj), j, np.zeros((h, w)))[k % 4]
        d[i0:i0 + h, j0:j0 + w] += (dz + pitch * rise).astype(np.float32)          # NaN stays NaN


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
        raise SystemExit("roofs_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from ada_mvs_amd import _lib, buildings, dsm, dtm, hip_ops, roofs
    from buildings_bench import add_blobs
    from dsm_bench import fused_scene
    from dsm_fill_bench import punch_holes
    from dtm_bench import timed
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
    add_pitched_boxes(d, args.boxes)
    add_blobs(d, args.blobs)
    del xyz, rgb, b, res, rgba
    gf = dtm.ground_filter(d, grid.gsd, max_radius=64.5 * grid.gsd, fill_max_dist=128.0 * grid.gsd)
    bl = buildings.extract(d, gf["ndsm"], grid.gsd, grid=grid)
    building = bl["label"]
    del gf
    scene_s = time.time() - t0
    p = roofs.parameters(grid.gsd)
    z_ref = roofs.reference_height(d)
    dev = torch.device("cuda")
    dd, bb = torch.from_numpy(d).to(dev), torch.from_numpy(building).to(dev)
    n = grid.W * grid.H
    ws = torch.empty(int(_lib.load().adamvs_roof_workspace_bytes(grid.W, grid.H)), device=dev, dtype=torch.uint8)
    out = {"workload": "roofs", "W": grid.W, "H": grid.H, "cells": n, "gsd": grid.gsd, "boxes": args.boxes, "blobs": args.blobs,
           "buildings": bl["counts"]["buildings"], "building_cells": int((building > 0).sum()), "stride": p["stride"],
           "grow_rounds": p["grow_rounds"], "steps": args.steps, "warmup": args.warmup, "bytes_per_cell": BYTES, "bytes_per_pair_look": PAIR_BYTES}

    def roof(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / HBM_BPS, 3) if ms > 0 else None

    def group(name, med, band, nbytes, **more):
        out[name] = dict({"ms_median": round(med, 3), "ms_p10_p90": band, "hbm_roof_fraction": roof(nbytes, med)}, **more)

    link, med, band = timed(lambda: hip_ops.roof_links(dd, bb, p["stride"], p["smooth_tol"], p["g_tol"], p["step_tol"]), args.steps, args.warmup)
    group("links", med, band, n * BYTES["links"])
    tile, rounds, compress, whole = [], [], [], []
    for it in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        seg, S, parent, st = hip_ops.roof_label(link, workspace=ws)
        e1.record()
        e1.synchronize()
        if it >= args.warmup:
            tile.append(st.ms_tile)
            rounds.append(st.ms_rounds)
            compress.append(st.ms_compress)
            whole.append(e0.elapsed_time(e1))
    pairs, nr = int(st.pairs), int(st.rounds)
    group("tile", *stat(tile), n * BYTES["tile"], tiles=int(st.tiles))
    group("rounds", *stat(rounds), (nr + 1) * pairs * PAIR_BYTES, rounds=nr, looks=nr + 1, pairs=pairs)
    group("compress", *stat(compress), n * BYTES["compress"])
    med_whole, band = stat(whole)
    out["label_call"] = {"ms_median": med_whole, "ms_p10_p90": band,
                         "number_ms": round(med_whole - out["tile"]["ms_median"] - out["rounds"]["ms_median"] - out["compress"]["ms_median"], 3)}
    seg_table, med, band = timed(lambda: hip_ops.roof_moments(dd, seg, bb, z_ref, S), args.steps, args.warmup)
    group("moments_segments", med, band, n * BYTES["moments"], labels=int(S))
    t1 = time.time()
    keep, planes = roofs.select_planes(seg_table.cpu().numpy(), grid.gsd, p["min_plane_area"])
    fit_s = time.time() - t1
    P = int(keep.sum())
    lut = torch.zeros(S + 1, device=dev, dtype=torch.int32)
    lut[1:][torch.from_numpy(keep).to(dev)] = torch.arange(1, P + 1, device=dev, dtype=torch.int32)
    seed = lut[seg.long()]
    planes_dev = torch.from_numpy(planes).to(dev)
    l0, l1 = torch.empty_like(seed), torch.empty_like(seed)
    counts = torch.zeros(_lib.ROOF_MAX_GROW, device=dev, dtype=torch.int32)
    ms = []
    for it in range(args.warmup + args.steps):
        l0.copy_(seed)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip_ops.roof_grow(dd, bb, z_ref, planes_dev, p["assign_tol"], l0, l1, counts, 0, p["grow_rounds"])
        e1.record()
        e1.synchronize()
        if it >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    med, band = stat(ms)
    per_round = counts[:p["grow_rounds"]].cpu().numpy().astype(np.int64)
    grown = (l0, l1)[p["grow_rounds"] & 1]
    group("grow", med, band, n * BYTES["grow_round"] * p["grow_rounds"], rounds=p["grow_rounds"],
          ms_per_round=round(med / max(1, p["grow_rounds"]), 4), rounds_that_labelled=int((per_round > 0).sum()), cells_grown=int(per_round.sum()))
    grown_table, med, band = timed(lambda: hip_ops.roof_moments(dd, grown, bb, z_ref, P), args.steps, args.warmup)
    group("moments_grown", med, band, n * BYTES["moments"], labels=P)
    _, med, band = timed(lambda: hip_ops.roof_residuals(dd, grown, z_ref, planes_dev, p["assign_tol"]), args.steps, args.warmup)
    group("residuals", med, band, n * BYTES["residuals"], labels=P)
    out["total_ms"] = round(sum(out[k]["ms_median"] for k in ("links", "label_call", "moments_segments", "grow", "moments_grown", "residuals")), 3)
    # the whole stage once: the counts and the host's share
    full = roofs.extract(d, building, grid.gsd, grid=grid)
    assert np.array_equal(full["grown"], grown.cpu().numpy()) and full["S"] == S and full["P"] == P
    out.update(S=int(S), P=P, R=full["R"], counts=full["counts"], grow_stats=dict(rounds_run=full["grow_stats"]["rounds_run"]),
               host={"segment_fits_s": round(fit_s, 3), **{k: round(v, 3) for k, v in full["seconds"].items()}},
               largest_plane_cells=int(full["table"][0].max()) if full["R"] else 0, scene_s=round(scene_s, 1), device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
