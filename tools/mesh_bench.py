"""TSDF mesh timing (csrc/mesh.hip): integrate + extract over the active bricks of the fused analytic scene.
    python tools/mesh_bench.py [--H 2752 --W 1856] [--voxels 0.25,0.5] [--brick 128] [--trunc 4] [--cpu 1]
The 5-view scene of tools/fusion_bench.py (ada_mvs_amd/fusion_synth.py: one nadir and four 40-degree obliques), each view
fused against the other four on the GPU (fusion.fuse_view); the fused points give the volume and the active bricks, the fused
depth maps are integrated.  Per voxel size, one warm-up pass over a few bricks, then one timed pass over every active brick:
device events around integrate and around extract (extract includes the read-back of the two totals), the wall time of the
pass, and the per-brick host round trip (wall minus device, per brick).  The byte model below is priced against 6.3 TB/s.
The CPU baseline is the numpy restatement (tests/mesh_ref.py) on one brick.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import ada_mvs_amd  # noqa: E402,F401

HBM_GBS = 6300.0               # the bandwidth the estimate was priced against
TARGET_MS = 50.0               # device-side, the scene at 0.25 m


def brick_bytes(B, nlist, nv, nt):
    """Algorithmic bytes of one brick: integrate reads one depth tap (4 B) and at most one colour (4 B) per sample and listed
    view and writes tsdf + weight + rgba (10 B); classify reads tsdf + weight (6 B per sample) and writes a code (4 B per
    cube); count reads tsdf and the codes (8 B) and writes the mask (1 B); emit reads tsdf, rgba, mask (9 B), writes the first
    vertex (4 B) and reads the codes and masks again (5 B); 27 B per vertex and 12 B per face written."""
    S, C = (B + 1) ** 3, B ** 3
    return S * (8 * nlist + 10) + S * 6 + C * 4 + S * 9 + S * 9 + 4 * S + 5 * C + 27 * nv + 12 * nt


def fused_scene(H, W, device):
    import torch
    from ada_mvs_amd import fusion, fusion_synth
    sc = fusion_synth.scene(H, W, 4, seed=0)
    views = [dict(depth=torch.from_numpy(d).to(device), K=c["K"], R=c["R"], C=c["C"]) for c, d in zip(sc["cams"], sc["depths"])]
    out, pts = [], []
    for i, v in enumerate(views):
        rgba = torch.from_numpy(fusion_synth.texture(sc["cams"][i], sc["depths"][i].astype(np.float64))).to(device)
        conf = torch.from_numpy(sc["confs"][i]).to(device)
        _, fused, xyz, _ = fusion.fuse_view(v, [u for j, u in enumerate(views) if j != i], conf, rgba)
        out.append(dict(K=v["K"], R=v["R"], C=v["C"], depth=fused.clone(), rgba=rgba))
        pts.append(xyz.clone())
    return out, pts


def run(views, pts, voxel, trunc, B, device):
    import torch
    from ada_mvs_amd import mesh
    mu = trunc * voxel
    allp = torch.cat(pts)
    lo = allp.min(0).values.cpu().numpy() - mu
    hi = allp.max(0).values.cpu().numpy() + mu
    origin, nb = mesh.grid_for_bounds(lo, hi, voxel, B)
    m = mesh.TsdfMesher(origin, voxel, mu, B, views)
    active = mesh.active_bricks(pts, origin, voxel, mu, B, nb, device)
    lists = [(b, m.view_list(b)) for b in active]
    lists = [(b, vl) for b, vl in lists if vl]
    for b, vl in lists[:3]:                                        # warm-up
        m.extract(b, m.integrate(b, vl))
    torch.cuda.synchronize()
    ev, counts = [], []
    t0 = time.time()
    for b, vl in lists:
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        vol = m.integrate(b, vl)
        e[1].record()
        xyz, _, f = m.extract(b, vol)
        e[2].record()
        ev.append(e)
        counts.append((len(vl), xyz.shape[0], f.shape[0]))
    torch.cuda.synchronize()
    wall = time.time() - t0
    t_int = sum(e[0].elapsed_time(e[1]) for e in ev)
    t_ext = sum(e[1].elapsed_time(e[2]) for e in ev)
    dev_ms = t_int + t_ext
    nbytes = sum(brick_bytes(B, *c) for c in counts)
    S = (B + 1) ** 3 * len(lists)
    return dict(voxel=voxel, mu=mu, brick=B, bricks_total=int(np.prod(nb)), bricks_active=len(lists), samples=S,
                vertices=int(sum(c[1] for c in counts)), faces=int(sum(c[2] for c in counts)), integrate_ms=round(t_int, 3),
                extract_ms=round(t_ext, 3), device_ms=round(dev_ms, 3), wall_ms=round(wall * 1e3, 3),
                host_round_trip_ms_per_brick=round((wall * 1e3 - dev_ms) / max(len(lists), 1), 4),
                samples_per_s=float("%.4g" % (S / (t_int * 1e-3))) if t_int > 0 else None, bytes=int(nbytes),
                gb_per_s=round(nbytes / (dev_ms * 1e-3) / 1e9, 1), frac_of_6_3_tbs=round(nbytes / (dev_ms * 1e-3) / 1e9 / HBM_GBS, 3),
                first_brick=lists[0][0] if lists else None), (m, lists)


def cpu_baseline(m, views_h, b, vl):
    import mesh_ref as M
    recs = [M.view_record(v["K"], v["R"], v["C"], m.origin, v["depth_h"], v["rgba_h"]) for v in views_h]
    t0 = time.time()
    r = M.integrate(m.voxel, m.mu, m.B, b, recs, vl)
    M.extract(m.origin, m.voxel, m.B, b, r["tsdf"], r["weight"], r["rgba"])
    return time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--voxels", default="0.25,0.5")
    ap.add_argument("--brick", type=int, default=128)
    ap.add_argument("--trunc", type=float, default=4.0)
    ap.add_argument("--cpu", type=int, default=1, help="also time the numpy restatement on one brick")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    dev = torch.device("cuda")
    t0 = time.time()
    views, pts = fused_scene(args.H, args.W, dev)
    setup_s = time.time() - t0
    res = {"workload": "mesh", "H": args.H, "W": args.W, "views": len(views), "fused_points": int(sum(p.shape[0] for p in pts)),
           "per_voxel": {}, "target_device_ms_at_0.25": TARGET_MS}
    keep = None
    for vx in (float(v) for v in args.voxels.split(",")):
        r, ctx = run(views, pts, vx, args.trunc, args.brick, dev)
        res["per_voxel"][repr(vx)] = r
        if keep is None:
            keep = ctx
    r25 = res["per_voxel"].get("0.25")
    if r25 is not None:
        res["meets_target"] = r25["device_ms"] <= TARGET_MS
    if args.cpu and keep is not None and keep[1]:
        m, lists = keep
        views_h = [dict(K=v["K"], R=v["R"], C=v["C"], depth_h=v["depth"].cpu().numpy(), rgba_h=v["rgba"].cpu().numpy()) for v in views]
        b, vl = lists[len(lists) // 2]
        s = cpu_baseline(m, views_h, b, vl)
        first = next(iter(res["per_voxel"].values()))
        gpu_per_brick = first["device_ms"] / max(first["bricks_active"], 1)
        res["cpu_restatement_s_per_brick"] = round(s, 3)
        res["gpu_ms_per_brick"] = round(gpu_per_brick, 4)
        res["speedup_vs_cpu_per_brick"] = round(s * 1e3 / gpu_per_brick, 1)
    res["setup_s"] = round(setup_s, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
