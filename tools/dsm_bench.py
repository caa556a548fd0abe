"""DSM rasterisation timing (csrc/dsm.hip): accumulate + claim + finalize over the fused points of the seeded 5-view scene.

    python tools/dsm_bench.py [--H 2752 --W 1856] [--gsd-factors 1,5,25] [--steps 20 --warmup 3] [--uncombined 1]

The scene of tools/fusion_bench.py (ada_mvs_amd/fusion_synth.py, 4 sources) is fused with every one of its 5 views as the
reference (fusion.fuse_view: 15.6 M points, 4.6 M of them from the nadir view, each view's in row-major pixel order).  At
the pixel footprint of the nadir view (~0.16 m) and at 5x and 25x that GSD, the launches of all 5 views (one chunk per view)
plus the finalize pass are timed with device events after warm-up, in max and in mean mode; the state is zeroed outside the
timed window.  --uncombined times the same with the library built with -DADAMVS_DSM_NO_COMBINE (tools/build_variant.py
dsm_nocombine; built here if missing or older than the shipped library) in a child process.  Atomic requests per point: wave
lanes that issue atomics (one per run of equal cells inside a wave when combined, one per used point when not) times the
atomics each issues (2 in max mode, 3 in mean), over the points.  CPU baseline: the fp64 numpy restatement
(tests/dsm_ref.py) on one view.  One JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import ada_mvs_amd  # noqa: E402,F401

VARIANT = "dsm_nocombine"
TARGET_MS = 1.0                # per 4.6 M-point view, at every GSD


def fused_scene(H, W, seed=0):
    """-> (xyz [N, 3] float64, rgb [N, 3] uint8) on the device, [points per view], nadir pixel footprint (m)."""
    import torch
    from ada_mvs_amd import fusion, fusion_synth
    sc = fusion_synth.scene(H, W, 4, seed=seed)
    dev = torch.device("cuda")
    views = [dict(depth=torch.from_numpy(d).to(dev), K=c["K"], R=c["R"], C=c["C"]) for c, d in zip(sc["cams"], sc["depths"])]
    xyzs, rgbs, per_view = [], [], []
    for r in range(len(views)):
        conf = torch.from_numpy(sc["confs"][r]).to(dev)
        rgba = torch.from_numpy(fusion_synth.texture(sc["cams"][r], sc["depths"][r].astype(np.float64))).to(dev)
        _, _, xyz, rgb = fusion.fuse_view(views[r], [v for i, v in enumerate(views) if i != r], conf, rgba)
        xyzs.append(xyz.clone())
        rgbs.append(rgb.clone())
        per_view.append(int(xyz.shape[0]))
    cam = sc["cams"][0]
    footprint = float(cam["C"][2] / cam["K"][0, 0])          # nadir view over the z = 0 terrain
    return torch.cat(xyzs), torch.cat(rgbs), per_view, footprint


def time_raster(xyz, rgb, per_view, gsd, mode, steps, warmup):
    import torch
    from ada_mvs_amd import dsm, hip_ops
    lo, hi = torch.aminmax(xyz, dim=0)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    grid = dsm.grid_for_bounds(lo, hi, gsd, np.floor(lo[2]))
    bounds = np.cumsum([0] + per_view)
    chunks = [(xyz[a:b], rgb[a:b], int(a)) for a, b in zip(bounds[:-1], bounds[1:])]
    b = dsm.DsmBuilder(grid, mode, xyz.device)

    def once():
        for t in (b.key, b.count, b.color) + ((b.sum,) if b.sum is not None else ()):
            t.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for x, c, s in chunks:
            hip_ops.dsm_accumulate(grid, x, s, dsm.MODES[mode], b.key, b.count, b.sum)
            hip_ops.dsm_claim(grid, x, c, s, b.key, b.color)
        out = hip_ops.dsm_finalize(grid, b.key, b.count, b.sum, b.color, dsm.MODES[mode], 1)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for _ in range(warmup):
        once()
    ms = np.array([once()[0] for _ in range(steps)])
    return grid, ms


def measure(xyz, rgb, per_view, gsds, steps, warmup):
    res = {}
    n = sum(per_view)
    for gsd in gsds:
        for mode in ("max", "mean"):
            grid, ms = time_raster(xyz, rgb, per_view, gsd, mode, steps, warmup)
            med = float(np.median(ms))
            res["%g/%s" % (gsd, mode)] = {
                "gsd": gsd, "mode": mode, "W": grid.W, "H": grid.H, "ms_total": round(med, 4),
                "ms_p10_p90": [round(float(np.percentile(ms, 10)), 4), round(float(np.percentile(ms, 90)), 4)],
                "ms_per_4.6M_view": round(med * 4.6e6 / n, 4), "points_per_s": round(n / (med * 1e-3), -6)}
    return res


def requests_per_point(xyz_h, per_view, gsd):
    from ada_mvs_amd import dsm
    from dsm_ref import cells, combined_requests
    grid = dsm.grid_for_bounds(xyz_h[:, :2].min(0), xyz_h[:, :2].max(0), gsd, np.floor(xyz_h[:, 2].min()))
    runs = used = 0
    s = 0
    for n in per_view:                    # waves restart at every chunk
        u, c, _ = cells(grid, xyz_h[s:s + n])
        runs += combined_requests(c, u)
        used += int(u.sum())
        s += n
    return runs / len(xyz_h), used / len(xyz_h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--gsd-factors", default="1,5,25", help="GSDs as multiples of the nadir pixel footprint")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--uncombined", type=int, default=1, help="also time the -DADAMVS_DSM_NO_COMBINE build (child process)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)       # points file: time them with this process's library
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dsm_bench: needs an MI355X (no CPU timing is reported)")
    if args.child:
        z = np.load(args.child)
        xyz, rgb = torch.from_numpy(z["xyz"]).cuda(), torch.from_numpy(z["rgb"]).cuda()
        print(json.dumps(measure(xyz, rgb, [int(v) for v in z["per_view"]], [float(g) for g in z["gsds"]], args.steps, args.warmup)))
        return
    t0 = time.time()
    xyz, rgb, per_view, footprint = fused_scene(args.H, args.W)
    scene_s = time.time() - t0
    gsds = [round(footprint * float(f), 4) for f in args.gsd_factors.split(",")]
    n = sum(per_view)
    res = {"workload": "dsm", "H": args.H, "W": args.W, "views": len(per_view), "points": n, "points_per_view": per_view,
           "pixel_footprint_m": round(footprint, 4), "steps": args.steps, "warmup": args.warmup,
           "combined": measure(xyz, rgb, per_view, gsds, args.steps, args.warmup)}
    xyz_h = xyz.cpu().numpy()
    rgb_h = rgb.cpu().numpy()
    res["atomic_requests_per_point"] = {}
    for gsd in gsds:
        runs, used = requests_per_point(xyz_h, per_view, gsd)
        res["atomic_requests_per_point"]["%g" % gsd] = {"combined_max": round(2 * runs, 4), "combined_mean": round(3 * runs, 4),
                                                        "uncombined_max": round(2 * used, 4), "uncombined_mean": round(3 * used, 4)}
    if args.uncombined:
        lib = os.path.join(ROOT, "ada-mvs_amd", "libadamvs_hip.%s.so" % VARIANT)
        shipped = os.path.join(ROOT, "ada-mvs_amd", "libadamvs_hip.so")
        if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(shipped):
            subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_variant.py"), VARIANT, "-DADAMVS_DSM_NO_COMBINE"], check=True,
                           stdout=subprocess.DEVNULL)
        with tempfile.TemporaryDirectory(prefix="dsm_bench_") as tmp:
            pts = os.path.join(tmp, "points.npz")
            np.savez(pts, xyz=xyz_h, rgb=rgb_h, per_view=np.array(per_view), gsds=np.array(gsds))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pts, "--steps", str(args.steps), "--warmup",
                                str(args.warmup)], capture_output=True, text=True, timeout=1800, cwd=ROOT,
                               env=dict(os.environ, ADAMVS_LIB_PATH=lib))
            if r.returncode != 0:
                raise SystemExit("uncombined child failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
            res["uncombined"] = json.loads(r.stdout.strip().splitlines()[-1])
    from ada_mvs_amd import dsm
    from dsm_ref import restate
    v0 = xyz_h[:per_view[0]]
    grid = dsm.grid_for_bounds(v0[:, :2].min(0), v0[:, :2].max(0), gsds[0], np.floor(v0[:, 2].min()))
    t0 = time.time()
    restate(grid, v0, rgb_h[:per_view[0]], "max")
    res["cpu_numpy_s_per_view"] = {"gsd": gsds[0], "mode": "max", "points": per_view[0], "seconds": round(time.time() - t0, 3)}
    worst = max(v["ms_per_4.6M_view"] for v in res["combined"].values())
    res["ms_per_view_worst"] = worst
    res["target_ms"] = TARGET_MS
    res["meets_target"] = worst <= TARGET_MS
    res["scene_s"] = round(scene_s, 1)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
