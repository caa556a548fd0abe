"""Solar timing (csrc/dsm_solar.hip): horizon, sky-view factor, exposure and plane sums at the raster benches' size.

    python tools/solar_bench.py [--H 2656 --W 2656] [--gsd 0.16] [--buildings 900] [--latitude 30.5] [--steps 3 --warmup 1] [--seed 7]

Input: a synthetic city (a plane that falls to the east, seeded box and gable buildings of 3 .. 25 m on it, every roof face a
labelled plane with its normal) of the drainage bench's 7.05 M cells.  For K = 8, 16 and 32 each kernel is timed with device events
around the call after warm-up, median and p10-p90 over --steps runs; the calls that block (horizon, exposure) include their
read-backs:
  horizon       adamvs_solar_horizon: the lines, the deepest stack and the entries spilled are reported.  Bytes moved: the output
                (8 K B per cell, the unavoidable traffic: the floor), the heights read once per direction (4 K B per cell) and
                16 B per spilled entry if every one comes back; the time is set against the floor and against all bytes at
                6.3 TB/s (measured HBM copy rate), and given per cell and direction
  svf           adamvs_solar_svf (8 K B per cell in, 8 B out)
  expose        adamvs_solar_expose with the built-in clear-sky year at --latitude (T rows) and the roof planes' normals
  planes        adamvs_solar_plane_sums
The surface (adamvs_contour_surface) and the host's share (the sample table, the per-plane columns) are timed once.  CPU baseline on
a 128 x 128 crop at the centre, K = 8: the brute force of the host restatement (tests/solar_ref.py).  One JSON line.
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


def city(H, W, gsd, buildings, seed):
    """-> (z float32 [H, W], label int32 [H, W], normals float [P, 3]): ground falling 2 % to the east; boxes (one level plane) and
    gables (two planes, the ridge along the rows or the columns) where they fit without touching an earlier building."""
    rng = np.random.default_rng(seed)
    z = np.tile(50.0 - 0.02 * gsd * np.arange(W, dtype=np.float64), (H, 1))
    label = np.zeros((H, W), np.int32)
    normals = []
    for _ in range(buildings):
        h, w = (int(v) for v in rng.integers(int(6 / gsd), int(30 / gsd), 2))
        if h + 2 >= H or w + 2 >= W:
            continue
        i, j = int(rng.integers(1, H - h - 1)), int(rng.integers(1, W - w - 1))
        if label[i - 1:i + h + 1, j - 1:j + w + 1].any():
            continue
        eave = float(z[i, j]) + float(rng.uniform(3.0, 25.0))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            z[i:i + h, j:j + w] = eave
            normals.append([0.0, 0.0, 1.0])
            label[i:i + h, j:j + w] = len(normals)
            continue
        slope = float(rng.uniform(0.3, 1.0))
        c = 1.0 / np.sqrt(1.0 + slope * slope)
        if kind == 1:                                                # the ridge along the columns: a north and a south face
            d = (np.minimum(np.arange(h), h - 1 - np.arange(h)) + 0.5) * gsd
            z[i:i + h, j:j + w] = eave + slope * d[:, None]
            normals += [[0.0, slope * c, c], [0.0, -slope * c, c]]
            label[i:i + h // 2, j:j + w], label[i + h // 2:i + h, j:j + w] = len(normals) - 1, len(normals)
        else:                                                        # the ridge along the rows: a west and an east face
            d = (np.minimum(np.arange(w), w - 1 - np.arange(w)) + 0.5) * gsd
            z[i:i + h, j:j + w] = eave + slope * d[None, :]
            normals += [[-slope * c, 0.0, c], [slope * c, 0.0, c]]
            label[i:i + h, j:j + w // 2], label[i:i + h, j + w // 2:j + w] = len(normals) - 1, len(normals)
    return z.astype(np.float32), label, np.array(normals, np.float64).reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2656)
    ap.add_argument("--W", type=int, default=2656)
    ap.add_argument("--gsd", type=float, default=0.16)
    ap.add_argument("--buildings", type=int, default=900)
    ap.add_argument("--latitude", type=float, default=30.5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("solar_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from ada_mvs_amd import hip_ops, solar
    from dtm_bench import timed
    t0 = time.time()
    z, label, normals = city(args.H, args.W, args.gsd, args.buildings, args.seed)
    scene_s = time.time() - t0
    H, W = z.shape
    n = H * W
    P = normals.shape[0]
    dev = torch.device("cuda")
    out = {"workload": "solar", "W": W, "H": H, "cells": n, "gsd": args.gsd, "planes": P, "cells_on_planes": int((label > 0).sum()),
           "latitude": args.latitude, "steps": args.steps, "warmup": args.warmup, "seed": args.seed, "stack_window": solar.STACK_WINDOW}

    def entry(med, band, **more):
        return dict({"ms_median": round(med, 3), "ms_p10_p90": band}, **more)

    def roof(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / HBM_BPS, 3) if ms > 0 else None

    zz = torch.from_numpy(z).to(dev)
    (s, info), med, band = timed(lambda: hip_ops.contour_surface(zz, 50.0, 0), args.steps, args.warmup)
    out["surface"] = entry(med, band)
    if int(info.cpu()[2]):
        raise SystemExit("solar_bench: cells out of range")
    lab_d = torch.from_numpy(label).to(dev)
    nrm_d = torch.from_numpy(solar.quantise_normals(normals).astype(np.int32)).to(dev)
    for K in (8, 16, 32):
        ws = None
        t1 = time.time()
        table = solar.sample_table(args.gsd, K, args.latitude)
        table_s = time.time() - t1

        def horizon():
            return hip_ops.solar_horizon(s, K, ws)
        (hz_n, hz_h, st, ws), med, band = timed(horizon, args.steps, args.warmup)
        floor, moved = 8 * K * n, 12 * K * n + 16 * st["spills"]
        res = {"horizon": entry(med, band, ms_device=round(st["ms"], 3), lines=st["lines"], deepest=st["deepest"], spills=st["spills"],
                                floor_bytes=floor, floor_ms=round(floor / HBM_BPS * 1e3, 3), times_the_floor=round(med / (floor / HBM_BPS * 1e3), 1),
                                moved_bytes=moved, hbm_roof_fraction=roof(moved, med), ns_per_cell_direction=round(med * 1e6 / (K * n), 4))}
        svf, med, band = timed(lambda: hip_ops.solar_svf(s, hz_n, hz_h, solar.direction_weights(K), (256.0 * args.gsd) ** 2), args.steps, args.warmup)
        res["svf"] = entry(med, band, hbm_roof_fraction=roof((8 * K + 12) * n, med))
        (minutes, direct, ws), med, band = timed(lambda: hip_ops.solar_expose(s, hz_n, hz_h, table, lab_d, nrm_d, ws), args.steps, args.warmup)
        res["expose"] = entry(med, band, samples=int(table["sector"].size), hbm_roof_fraction=roof((8 * K + 16) * n, med))
        sums, med, band = timed(lambda: hip_ops.solar_plane_sums(s, minutes, direct, lab_d, P), args.steps, args.warmup)
        res["planes"] = entry(med, band, hbm_roof_fraction=roof(16 * n, med))
        res["total_ms"] = round(sum(res[k]["ms_median"] for k in ("horizon", "svf", "expose", "planes")), 3)
        res["sample_table_s"] = round(table_s, 3)
        sv = svf.cpu().numpy()
        res["svf_mean"] = round(float(sv.mean()), 4)
        res["sun_hours_mean"] = round(float(minutes.double().mean()) / 60.0, 1)
        res["occluded_fraction"] = round(float((hz_h > 0).double().mean()), 4)
        out["K%d" % K] = res
        del hz_n, hz_h, ws
        torch.cuda.empty_cache()
    import solar_ref
    i0, j0 = max(0, H // 2 - 64), max(0, W // 2 - 64)
    crop = solar_ref.surface(z[i0:i0 + 128, j0:j0 + 128], 50.0)
    t1 = time.time()
    solar_ref.horizon_brute(crop, 8)
    out["cpu_crop"] = {"crop": [i0, j0, 128, 128], "K": 8, "brute_force_s": round(time.time() - t1, 2)}
    out["scene_s"] = round(scene_s, 1)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
