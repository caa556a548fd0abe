"""Mesh smoothing timing (csrc/mesh_smooth.hip through ada_mvs_amd/smooth.py) on the TSDF mesh of the fused analytic scene.
    python tools/smooth_bench.py [--H 2752 --W 1856] [--voxel 0.25] [--brick 128] [--runs 10] [--normal_iters 10] [--vertex_iters 10]
The 5-view scene of tools/mesh_bench.py meshed at --voxel and welded, held on the device (tools/simplify_bench.py builds it).
2 warm-ups and then --runs calls of smooth() at the default options (sigma_s and the cap one voxel): device events around the
whole call and around every stage, the median over the runs.  `sort_ms` is what torch does (the weld and the stable sort of
the (vertex, face) entries with its searchsorted); `boundary` holds torch's sort of the edge keys between its two kernels;
`kernel_ms` is the rest.  The byte model below is priced against 6.3 TB/s over the filter and the update stages.  One JSON
line; there is no pass bar, nothing of this had a number before.
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

HBM_GBS = 6300.0
SORT_STAGES = ("weld", "sort_incidence")


def filter_bytes(nf, neighbours, entries):
    """Algorithmic bytes of one pass of the normal filter.  Per face: 12 B of indices, its record's first half (32 B), its normal
    (24 B), three run bounds (48 B), 24 B written.  Per run entry visited (entries = the sum over faces of the runs of their
    corners): 4 B of face number and, at corners 1 and 2 (two thirds), 12 B of indices for the skip test.  Per neighbour summed:
    32 B of record and 24 B of normal."""
    return nf * (12 + 32 + 24 + 48 + 24) + entries * (4 + 8) + neighbours * 56


def update_bytes(nv, nf):
    """Algorithmic bytes of one pass of the vertex update with its centroids.  Centroids: 12 B of indices and three 24 B positions
    read, 24 B written per face.  Update: per vertex 48 B of positions, 16 B of run bounds, 1 B of flag read, 25 B written; per
    (vertex, face) entry (3 nf) 4 B of face number, 24 B of normal, 24 B of centroid."""
    return nf * (12 + 72 + 24) + nv * (48 + 16 + 1 + 25) + 3 * nf * 52


def neighbour_counts(detail):
    """-> (the sum over faces of |N(f)|, the sum over faces of the lengths of their corners' runs)."""
    import torch
    count = (detail["vstart"][1:] - detail["vstart"][:-1])
    f = detail["faces"].to(torch.int64) & 0xFFFFFFFF
    entries = int(count[f].sum())
    # |N(f)| where the mesh is a closed manifold: f is in all three runs (counted once: - 2) and each of the three faces across
    # an edge of f is in two of them (- 3); at a boundary this undercounts slightly
    return entries - 5 * int(f.shape[0]), entries


def run(xyz, rgb, faces, voxel, origin, runs, normal_iters, vertex_iters, warmup=2):
    import torch
    from ada_mvs_amd import smooth
    per_stage, totals, info, detail = {}, [], None, {}
    for i in range(warmup + runs):
        timing = []
        d = detail if i == 0 else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, _, _, info = smooth.smooth(xyz, rgb, faces, voxel, smooth.DEFAULT_SIGMA_R, normal_iters, vertex_iters, voxel, True, origin, detail=d,
                                      timing=timing)
        e1.record()
        torch.cuda.synchronize()
        if i < warmup:
            continue
        totals.append(e0.elapsed_time(e1))
        for name, a, b in timing:
            per_stage.setdefault(name, []).append(a.elapsed_time(b))
    stages = {k: float(np.median(v)) for k, v in per_stage.items()}
    total = float(np.median(totals))
    sort_ms = sum(v for k, v in stages.items() if k in SORT_STAGES)
    kernel_ms = sum(v for k, v in stages.items() if k not in SORT_STAGES)
    nv, nf = info["vertices"], info["faces"]
    neighbours, entries = neighbour_counts(detail)
    fb, ub = filter_bytes(nf, neighbours, entries) * normal_iters, update_bytes(nv, nf) * vertex_iters
    gbs = lambda b, ms: round(b / (ms * 1e-3) / 1e9, 1) if ms > 0 else None  # noqa: E731
    return dict(device_ms=round(total, 3), sort_ms=round(sort_ms, 3), kernel_ms=round(kernel_ms, 3),
                stage_ms={k: round(v, 3) for k, v in stages.items()}, vertices=nv, faces=nf, fixed=info["fixed"],
                degenerate_faces=info["degenerate_faces"], clamped=info["clamped"], largest_move=info["largest_move"], rms_move=info["rms_move"],
                neighbours_per_face=round(neighbours / max(nf, 1), 2), filter_ms_per_pass=round(stages.get("filter", 0.0) / max(normal_iters, 1), 3),
                update_ms_per_pass=round(stages.get("update", 0.0) / max(vertex_iters, 1), 3), filter_bytes=int(fb), update_bytes=int(ub),
                filter_gb_per_s=gbs(fb, stages.get("filter", 0.0)), update_gb_per_s=gbs(ub, stages.get("update", 0.0)),
                frac_of_6_3_tbs=round((fb + ub) / ((stages.get("filter", 0.0) + stages.get("update", 0.0)) * 1e-3) / 1e9 / HBM_GBS, 4),
                ns_per_face=round(total * 1e6 / max(nf, 1), 3), neighbour_form="recomputed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--voxel", type=float, default=0.25)
    ap.add_argument("--trunc", type=float, default=4.0)
    ap.add_argument("--brick", type=int, default=128)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--normal_iters", type=int, default=10)
    ap.add_argument("--vertex_iters", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("smooth_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from simplify_bench import build_mesh
    dev = torch.device("cuda")
    t0 = time.time()
    xyz, rgb, faces, origin = build_mesh(args.H, args.W, args.voxel, args.trunc, args.brick, dev)
    res = {"workload": "smooth", "H": args.H, "W": args.W, "voxel": args.voxel, "normal_iters": args.normal_iters,
           "vertex_iters": args.vertex_iters, "runs": args.runs, "setup_s": round(time.time() - t0, 2)}
    res.update(run(xyz, rgb, faces, args.voxel, origin, args.runs, args.normal_iters, args.vertex_iters))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
