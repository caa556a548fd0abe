"""Mesh cleaning timing (csrc/mesh_clean.hip through ada_mvs_amd/clean.py) on the TSDF mesh of the fused analytic scene.
    python tools/clean_bench.py [--H 2752 --W 1856] [--voxel 0.25] [--brick 128] [--runs 10] [--holes 2000] [--floaters 2000]
                                [--min_faces 100] [--max_hole_edges 32]
The 5-view scene of tools/mesh_bench.py meshed at --voxel and welded, held on the device (tools/simplify_bench.py builds it), the
scene tools/smooth_bench.py uses.  That mesh is clean, so the defects are made here: the faces around --holes random vertices
are taken out, and --floaters tetrahedra of four faces are put beside the scene.  2 warm-ups and then --runs calls of clean():
device events around the whole call and around every stage, the median over the runs.  `sort_ms` is the weld; the stages
`areas`, `boundary` and `fill` each hold one stable sort of torch's next to their kernels, `components` holds one read-back of
the `changed` word per round.  One JSON line; there is no pass bar, nothing of this had a number before.
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

SORT_STAGES = ("weld",)


def add_defects(xyz, rgb, faces, holes, floaters, seed=0):
    """-> (xyz, rgb, faces) without the faces around `holes` random vertices and with `floaters` tetrahedra beside the scene."""
    import torch
    dev = xyz.device
    g = torch.Generator(device="cpu").manual_seed(seed)
    if holes:
        centres = torch.randperm(xyz.shape[0], generator=g)[:holes].to(dev)
        hit = torch.zeros(xyz.shape[0], device=dev, dtype=torch.bool)
        hit[centres] = True
        faces = faces[~hit[faces].any(1)]
    if floaters:
        corner = torch.tensor([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], device=dev, dtype=torch.float64) * 0.5
        k = torch.arange(floaters, device=dev, dtype=torch.float64)
        at = torch.stack([xyz[:, 0].max() + 4.0 + 2.0 * (k % 64), xyz[:, 1].min() + 2.0 * torch.div(k, 64, rounding_mode="floor"),
                          xyz[:, 2].max().expand(floaters)], 1)
        tx = (at[:, None, :] + corner[None]).reshape(-1, 3)
        tf = torch.tensor([(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)], device=dev, dtype=torch.int64)
        tf = (tf[None] + 4 * torch.arange(floaters, device=dev, dtype=torch.int64)[:, None, None]).reshape(-1, 3) + xyz.shape[0]
        xyz = torch.cat([xyz, tx])
        rgb = torch.cat([rgb, torch.full((tx.shape[0], 3), 128, device=dev, dtype=torch.uint8)])
        faces = torch.cat([faces, tf])
    return xyz, rgb, faces


def run(xyz, rgb, faces, origin, runs, min_faces, max_hole_edges, warmup=2):
    import torch
    from ada_mvs_amd import clean
    per_stage, totals, info = {}, [], None
    for i in range(warmup + runs):
        timing = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, _, _, info = clean.clean(xyz, rgb, faces, min_faces, None, max_hole_edges, origin, timing=timing)
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
    res = dict(device_ms=round(total, 3), sort_ms=round(sort_ms, 3), rest_ms=round(sum(stages.values()) - sort_ms, 3),
               stage_ms={k: round(v, 3) for k, v in stages.items()}, ns_per_face=round(total * 1e6 / max(info["faces_in"], 1), 3),
               doubling_rounds=clean.doubling_rounds(info["boundary_edges_in"]))
    res.update(info)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--voxel", type=float, default=0.25)
    ap.add_argument("--trunc", type=float, default=4.0)
    ap.add_argument("--brick", type=int, default=128)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--holes", type=int, default=2000)
    ap.add_argument("--floaters", type=int, default=2000)
    ap.add_argument("--min_faces", type=int, default=100)
    ap.add_argument("--max_hole_edges", type=int, default=32)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("clean_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from simplify_bench import build_mesh
    dev = torch.device("cuda")
    t0 = time.time()
    xyz, rgb, faces, origin = build_mesh(args.H, args.W, args.voxel, args.trunc, args.brick, dev)
    xyz, rgb, faces = add_defects(xyz, rgb, faces, args.holes, args.floaters)
    res = {"workload": "clean", "H": args.H, "W": args.W, "voxel": args.voxel, "holes": args.holes, "floaters": args.floaters,
           "min_faces": args.min_faces, "max_hole_edges": args.max_hole_edges, "runs": args.runs, "setup_s": round(time.time() - t0, 2)}
    res.update(run(xyz, rgb, faces, origin, args.runs, args.min_faces, args.max_hole_edges))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
