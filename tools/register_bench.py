"""Cloud registration timing (csrc/cloud_register.hip through ada_mvs_amd/register.py) on a seeded synthetic terrain.
    python tools/register_bench.py [--targets 2000000] [--sources 1000000] [--spacing 0.1] [--ratio 4] [--noise 0.03] [--runs 5]
The truth: --targets points of a smooth height field (tests/register_inputs.py's, stretched to the scene) uniform over a square
sized for a mean point spacing of --spacing metres; the source: --sources points of the same field drawn independently, with
Gaussian noise in z, rolled 0.2 degrees about an oblique axis through the centre and shifted by 0.4 D.  D = --ratio times the
spacing.  One warm-up and then --runs calls of register.icp; reported per EVALUATION (an iteration's move, keys, sort, items,
nearest, accumulate, reduce: device events, the median over every evaluation of every run), the host solve per iteration (wall
clock around register.solve), the preparation (normals, keys and sort of the truth, once per call) as the rest of the device
time, iterations and the error against the known motion.  One JSON line; it sets no bar.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import ada_mvs_amd  # noqa: E402,F401


def terrain(n, side, noise, seed, device):
    """n points of the height field over [0, side]^2 (one period of its longest wave per 40 m, as in the tests) on the device."""
    import torch
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    xy = torch.rand(n, 2, device=device, dtype=torch.float64, generator=gen) * side
    x, y = xy[:, 0], xy[:, 1]
    z = 2.0 * torch.sin(x / 5.0) * torch.cos(y / 7.0) + 1.5 * torch.sin((x + y) / 4.0) + 0.8 * torch.cos(x / 3.0 - y / 2.5)
    if noise:
        z = z + torch.randn(n, device=device, dtype=torch.float64, generator=gen) * noise
    offset = torch.tensor([512345.0, 3376543.0, 120.0], device=device, dtype=torch.float64)
    return torch.stack([x, y, z], 1) + offset


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=2000000)
    ap.add_argument("--sources", type=int, default=1000000)
    ap.add_argument("--spacing", type=float, default=0.1, help="mean point spacing of the truth in metres")
    ap.add_argument("--ratio", type=float, default=4.0, help="D / point spacing")
    ap.add_argument("--noise", type=float, default=0.03, help="sigma of the source's noise in z, metres")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("register_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from ada_mvs_amd import hip_ops, register
    dev = torch.device("cuda")
    side = math.sqrt(args.targets) * args.spacing
    D = args.ratio * args.spacing
    truth = terrain(args.targets, side, 0.0, 1, dev)
    still = terrain(args.sources, side, args.noise, 2, dev)
    c = ((truth.min(0).values + truth.max(0).values) / 2.0).cpu().numpy()
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    rot = register.rodrigues(np.deg2rad(0.2) * axis)
    source = hip_ops.rigid_apply(still, rot, c, np.array([0.4, -0.3, 0.25]) * 0.8 * D)

    solve_s, plain_solve = [], register.solve

    def timed_solve(*a, **kw):
        t0 = time.perf_counter()
        r = plain_solve(*a, **kw)
        solve_s.append(time.perf_counter() - t0)
        return r

    register.solve = timed_solve
    per_stage, device_ms, wall_s, evaluations, res = {}, [], [], [], None
    try:
        for i in range(1 + args.runs):
            timing, solve_s[:] = [], []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            res = register.icp(source, truth, D, timing=timing)
            e1.record()
            torch.cuda.synchronize()
            if i == 0:
                continue
            wall_s.append(time.perf_counter() - t0)
            device_ms.append(e0.elapsed_time(e1))
            evaluations.append(res["iterations"] + 1)
            for name, a, b in timing:
                per_stage.setdefault(name, []).append(a.elapsed_time(b))
    finally:
        register.solve = plain_solve
    stage_ms = {k: round(float(np.median(per_stage[k])), 4) for k in register.STAGES}
    per_eval = sum(stage_ms.values())
    moved = hip_ops.rigid_apply(source, res["R"], res["pivot"], res["t"])
    err = float(torch.sqrt(((moved - still) ** 2).sum(1)).max())
    out = {"workload": "register", "targets": args.targets, "sources": args.sources, "point_spacing": args.spacing, "max_dist": D,
           "noise": args.noise, "runs": args.runs, "iterations": res["iterations"], "converged": res["converged"],
           "evaluations": int(np.median(evaluations)), "stage_ms_per_evaluation": stage_ms, "evaluation_ms": round(per_eval, 4),
           "host_solve_ms_per_iteration": round(1e3 * float(np.median(solve_s)), 4), "device_ms": round(float(np.median(device_ms)), 3),
           "preparation_ms": round(float(np.median(device_ms)) - per_eval * float(np.median(evaluations)), 3),
           "wall_s": round(float(np.median(wall_s)), 4), "fitness_after": res["fitness_after"], "rms_plane_after": res["rms_plane_after"],
           "search_pairs": res["pairs"], "error_against_the_known_motion_m": err, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
