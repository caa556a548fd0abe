"""Depth-map fusion timing (csrc/fusion.hip): consistency + scan + emit per reference view at the reference predict size.

    python tools/fusion_bench.py [--H 2752 --W 1856] [--sources 4,10] [--steps 50 --warmup 5] [--e2e 1]

A seeded analytic scene (ada_mvs_amd/fusion_synth.py) with 4 and with 10 sources; each view's three launches are timed with
device events after warm-up (median and spread over the repetitions).  Bytes per view come from the shape-based model
below; the CPU baseline is the fp64 numpy restatement (tests/fusion_ref.py) on one view; --e2e times fuse_whu.py on the
scene written in predict's output layout (a fresh child process), with its file I/O reported separately.  One JSON line.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import ada_mvs_amd  # noqa: E402,F401

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s
POINT_BYTES = 27               # double x y z + uchar r g b


def bytes_per_view(H, W, src_shapes, kept):
    """Algorithmic bytes of one view: reference depth + confidence (fp32) + RGBA image, every source depth map once (the
    bilinear taps of neighbouring pixels overlap: each map is counted once), count (uint8) + fused depth (fp32) written, the
    fused depth read again by the emit pass, 27 B per kept point."""
    px = H * W
    return px * (4 + 4 + 4) + sum(4 * h * w for h, w in src_shapes) + px * (1 + 4) + px * 4 + POINT_BYTES * kept


def time_view(views, conf, rgba, steps, warmup):
    import torch
    from ada_mvs_amd import fusion, hip_ops
    ref, srcs = views[0], views[1:]
    sources = []
    for s in srcs:
        fwd, back = fusion.relative_transforms(ref["K"], ref["R"], ref["C"], s["K"], s["R"], s["C"])
        sources.append((s["depth"], fwd, back))
    cam = fusion.emit_camera(ref["K"], ref["R"], ref["C"])
    H, W = ref["depth"].shape
    xyz = torch.empty(H * W, 3, device="cuda", dtype=torch.float64)
    rgb = torch.empty(H * W, 3, device="cuda", dtype=torch.uint8)

    def once():
        _, fused, block_kept = hip_ops.geo_consistency(ref["depth"], conf, sources)
        return hip_ops.emit_points(fused, block_kept, rgba, cam, xyz, rgb)[2]

    for _ in range(warmup):
        once()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        offsets = once()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return np.array(ms), int(offsets[-1].item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--sources", default="4,10")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--e2e", type=int, default=1, help="also time fuse_whu.py end to end on the 4-source scene")
    args = ap.parse_args()
    import torch
    from ada_mvs_amd import fusion_synth
    from fusion_ref import restate
    if not torch.cuda.is_available():
        raise SystemExit("fusion_bench: needs an MI355X (no CPU timing is reported)")
    counts = [int(n) for n in args.sources.split(",")]
    t0 = time.time()
    sc = fusion_synth.scene(args.H, args.W, max(counts), seed=0)
    render_s = time.time() - t0
    dev = torch.device("cuda")
    views = [dict(depth=torch.from_numpy(d).to(dev), K=c["K"], R=c["R"], C=c["C"]) for c, d in zip(sc["cams"], sc["depths"])]
    conf = torch.from_numpy(sc["confs"][0]).to(dev)
    rgba = torch.from_numpy(sc["rgba"]).to(dev)
    res = {"workload": "fusion", "H": args.H, "W": args.W, "steps": args.steps, "warmup": args.warmup, "per_sources": {}}
    for n in counts:
        ms, kept = time_view(views[:1 + n], conf, rgba, args.steps, args.warmup)
        nbytes = bytes_per_view(args.H, args.W, [tuple(v["depth"].shape) for v in views[1:1 + n]], kept)
        med = float(np.median(ms))
        gbs = nbytes / (med * 1e-3) / 1e9
        res["per_sources"][str(n)] = {
            "ms_per_view": round(med, 4), "ms_min": round(float(ms.min()), 4), "ms_max": round(float(ms.max()), 4),
            "ms_p10_p90": [round(float(np.percentile(ms, 10)), 4), round(float(np.percentile(ms, 90)), 4)],
            "kept_points": kept, "bytes_per_view": int(nbytes), "gb_per_s": round(gbs, 1),
            "frac_hbm_roof": round(gbs / HBM_PEAK_GBS, 3), "target_ms": 0.5, "meets_target": med <= 0.5}
    n0 = counts[0]
    t0 = time.time()
    restate(sc["depths"][0], sc["confs"][0], sc["cams"][0], [dict(cam=c, depth=d) for c, d in zip(sc["cams"][1:1 + n0], sc["depths"][1:1 + n0])],
            rgba=sc["rgba"])
    res["cpu_numpy_s_per_view"] = {"sources": n0, "seconds": round(time.time() - t0, 3)}
    res["scene_render_s"] = round(render_s, 1)
    if args.e2e:
        sub = dict(sc, cams=sc["cams"][:1 + n0], depths=sc["depths"][:1 + n0], confs=sc["confs"][:1 + n0])
        tmp = tempfile.mkdtemp(prefix="fusion_bench_")
        try:
            fusion_synth.write_predict_layout(sub, os.path.join(tmp, "data"), os.path.join(tmp, "out"))
            t0 = time.time()
            r = subprocess.run([sys.executable, os.path.join(ROOT, "fuse_whu.py"), "--data_folder", os.path.join(tmp, "data"),
                                "--output_folder", os.path.join(tmp, "out"), "--num_src", str(n0)], capture_output=True, text=True,
                               timeout=900, cwd=ROOT)
            wall = time.time() - t0
            if r.returncode != 0:
                raise SystemExit("fuse_whu.py failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
            m = re.search(r"fused (\d+) points from (\d+) views .* total_time = ([0-9.]+) s \(file I/O ([0-9.]+) s\)", r.stdout)
            res["fuse_whu"] = {"views": int(m.group(2)), "points": int(m.group(1)), "seconds": float(m.group(3)),
                               "file_io_seconds": float(m.group(4)), "process_wall_s": round(wall, 2)}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    first = res["per_sources"][str(n0)]
    res["ms_per_view"] = first["ms_per_view"]
    res["gb_per_s"] = first["gb_per_s"]
    res["frac_hbm_roof"] = first["frac_hbm_roof"]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
