"""LoD2 timing (csrc/dsm_lod2.hip): fill rounds, building table, transpose, run count and run emission at the bench shape.

    python tools/lod2_bench.py [--H 2752 --W 1856] [--steps 10 --warmup 2] [--boxes 400] [--open-fraction 0.05]

Input: a seeded raster of the bench shape of the other raster stages with --boxes rectangular buildings that keep a cell of
distance (10 - 120 cells on a side, a box that would touch an earlier one is left out), each by turns with a gable, a hip, a
shed or a flat roof given as planes (the labels are the lower envelope of the planes at the cell centres), a sloping terrain, and
--open-fraction of the roof cells without a plane in seeded patches of 3 x 3 cells, which the fill closes.  No earlier stage
runs: the planes are the scene's own.  Each group is timed with device events after warm-up, median and p10-p90 over --steps:
  fill       adamvs_lod2_fill, the rounds to the fixed point in one call: per round the building label in, the label in and
             out: 12 B per cell and round (the four neighbours are re-reads served by L2)
  table      adamvs_lod2_table: terrain, building and label in: 12 B per cell
  transpose  adamvs_lod2_transpose: 8 B per cell
  count      adamvs_lod2_count, both orientations and the scan: the label raster once per orientation: 8 B per cell (the row
             above a line is a re-read served by L2)
  runs       adamvs_lod2_runs: the same reads and 40 B per run written
against 6.3 TB/s (measured HBM copy rate).  The counts and the host time of the faces of one lod2.extract are reported.  One
JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import ada_mvs_amd  # noqa: E402,F401

HBM_BPS = 6.3e12
BYTES = dict(fill_round=12, table=12, transpose=8, count=8, runs=8)
RUN_BYTES = 40


def scene(H, W, boxes, open_fraction, gsd=0.25, seed=1):
    """-> (dtm, building, roof, properties, grid): see the module's text."""
    from ada_mvs_amd import dsm
    rng = np.random.default_rng(seed)
    grid = dsm.Grid(0.0, H * gsd, gsd, 0.0, W, H)
    i, j = np.mgrid[0:H, 0:W]
    terrain = (20.0 + j / 256.0 + i / 512.0).astype(np.float32)
    building, roof, props = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32), []
    taken = np.zeros((H, W), bool)
    B = 0
    for k in range(boxes):
        h, w = rng.integers(10, 121, 2)
        i0, j0, eave, pitch = rng.integers(1, H - h - 1), rng.integers(1, W - w - 1), rng.uniform(3.0, 30.0), rng.uniform(0.3, 0.7) * gsd
        if taken[i0 - 1:i0 + h + 1, j0 - 1:j0 + w + 1].any():
            continue
        B += 1
        taken[i0:i0 + h, j0:j0 + w] = True
        building[i0:i0 + h, j0:j0 + w] = B
        z0 = float(terrain[i0:i0 + h, j0:j0 + w].max()) + eave
        east, west = (pitch, 0.0, z0 - pitch * j0), (-pitch, 0.0, z0 + pitch * (j0 + w - 1))
        south, north = (0.0, pitch, z0 - pitch * i0), (0.0, -pitch, z0 + pitch * (i0 + h - 1))
        planes = ([east, west] if w <= h else [south, north], [east, west, south, north], [east], [(0.0, 0.0, z0)])[k % 4]
        ii, jj = np.mgrid[i0:i0 + h, j0:j0 + w]
        low = np.argmin(np.stack([a * jj + b * ii + c for a, b, c in planes]), axis=0)
        roof[i0:i0 + h, j0:j0 + w] = len(props) + 1 + low
        for a, b, c in planes:
            props.append(dict(id=len(props) + 1, building=B, slope_deg=0.0, aspect_deg=None,
                              plane=dict(z0=c, sx=a / gsd, sy=-b / gsd, xc=grid.x0 + 0.5 * gsd, yc=grid.y_top - 0.5 * gsd)))
    cells = np.argwhere(building > 0)
    for c in cells[rng.choice(len(cells), int(open_fraction * len(cells) / 9), replace=False)]:
        roof[max(c[0] - 1, 0):c[0] + 2, max(c[1] - 1, 0):c[1] + 2] = 0
    used = np.unique(roof[roof > 0])                                        # a plane that lost every cell would leave its id unused: fine
    return terrain, building, roof, props, grid, len(used)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--boxes", type=int, default=400)
    ap.add_argument("--open-fraction", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lod2_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from ada_mvs_amd import _lib, hip_ops, lod2
    from dtm_bench import timed
    t0 = time.time()
    terrain, building, roof, props, grid, planes_used = scene(args.H, args.W, args.boxes, args.open_fraction)
    scene_s = time.time() - t0
    z_ref = lod2.reference_height(terrain)
    planes, pb = lod2.integer_planes(props, grid, z_ref)
    P, B, n = len(planes), int(building.max()), grid.W * grid.H
    dev = torch.device("cuda")
    d, b, r = torch.from_numpy(terrain).to(dev), torch.from_numpy(building).to(dev), torch.from_numpy(roof).to(dev)
    planes_dev = torch.from_numpy(planes).to(dev)
    out = {"workload": "lod2", "W": grid.W, "H": grid.H, "cells": n, "gsd": grid.gsd, "boxes": args.boxes, "buildings": B, "planes": P,
           "planes_with_cells": planes_used, "building_cells": int((building > 0).sum()), "open_cells": int(((building > 0) & (roof == 0)).sum()),
           "steps": args.steps, "warmup": args.warmup, "bytes_per_cell": BYTES, "bytes_per_run": RUN_BYTES}

    def group(name, med, band, nbytes, **more):
        out[name] = dict({"ms_median": round(med, 3), "ms_p10_p90": band,
                          "hbm_roof_fraction": round(nbytes / (med * 1e-3) / HBM_BPS, 3) if med > 0 else None}, **more)

    filled, counts, rounds_run = lod2.fill(b, r, P, lod2.MAX_FILL)         # the rounds the early stop runs: whole chunks
    l0, l1 = torch.empty_like(r), torch.empty_like(r)
    cnt = torch.zeros(_lib.LOD2_MAX_FILL, device=dev, dtype=torch.int32)

    def fill_all():
        l0.copy_(r)
        hip_ops.lod2_fill(b, P, l0, l1, cnt, 0, rounds_run)
        return (l0, l1)[rounds_run & 1]
    again, med, band = timed(fill_all, args.steps, args.warmup)
    assert torch.equal(again, filled)
    group("fill", med, band, n * (BYTES["fill_round"] * rounds_run + 8), rounds=int(rounds_run), rounds_that_labelled=int((counts > 0).sum()),
          cells_filled=int(counts.sum()), ms_per_round=round(med / max(1, rounds_run), 4), includes="the copy of the start labels")
    table, med, band = timed(lambda: hip_ops.lod2_table(d, b, filled, z_ref, B, planes_dev), args.steps, args.warmup)
    group("table", med, band, n * BYTES["table"])
    table = table.cpu().numpy()
    refused = lod2.refusals(table)
    base = np.where(table[2] == lod2.MIN_START, 0, table[2])
    plane_base = torch.from_numpy(base[pb - 1].astype(np.int32)).to(dev)
    label_t, med, band = timed(lambda: hip_ops.lod2_transpose(filled), args.steps, args.warmup)
    group("transpose", med, band, n * BYTES["transpose"])
    lib = _lib.load()
    ws = torch.empty(int(lib.adamvs_lod2_workspace_bytes(grid.W, grid.H)), device=dev, dtype=torch.uint8)
    total = torch.zeros(1, device=dev, dtype=torch.int32)
    ptr = hip_ops._p

    def count():
        hip_ops.check(lib.adamvs_lod2_count(grid.W, grid.H, ptr(filled), ptr(label_t), P, ptr(ws), ws.numel(), ptr(total), hip_ops._stream()),
                      "lod2_count")
    _, med, band = timed(count, args.steps, args.warmup)
    N = int(total.item())
    blk = _lib.LOD2_BLOCK                                                   # as the launcher: the edges of either orientation, 256 per workgroup
    workgroups = -(-((grid.H + 1) * grid.W) // blk) + -(-((grid.W + 1) * grid.H) // blk)
    group("count", med, band, n * BYTES["count"], runs=N, workgroups=workgroups)
    records = torch.empty(len(_lib.LOD2_FIELDS), N, device=dev, dtype=torch.int32)

    def emit():
        hip_ops.check(lib.adamvs_lod2_runs(grid.W, grid.H, ptr(filled), ptr(label_t), P, ptr(planes_dev), ptr(plane_base), N, ptr(ws), ws.numel(),
                                           ptr(records), hip_ops._stream()), "lod2_runs")
    _, med, band = timed(emit, args.steps, args.warmup)
    group("runs", med, band, n * BYTES["runs"] + N * RUN_BYTES)
    out["total_ms"] = round(sum(out[k]["ms_median"] for k in ("fill", "table", "transpose", "count", "runs")), 3)
    full = lod2.extract(terrain, building, roof, props, grid.gsd, grid=grid)
    assert not refused and np.array_equal(full["records"], records.cpu().numpy()) and full["N"] == N
    out.update(counts=full["counts"], host={k: round(v, 3) for k, v in full["seconds"].items()}, scene_s=round(scene_s, 1),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
