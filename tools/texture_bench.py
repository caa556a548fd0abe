"""Mesh texture timing (csrc/texture.hip): the TSDF mesh of tools/fusion_bench.py's 5-view scene textured from its 5 images.
    python tools/texture_bench.py [--H 2752 --W 1856] [--voxel 0.25] [--page 8192] [--write 1]
                                  [--seam_level 1 [--seam_tol 1e-4] [--seam_iters 1000]]
The scene of tools/mesh_bench.py (one nadir and four 40-degree obliques, each view fused against the other four on the GPU),
meshed over every active brick of 128^3 at --voxel and welded on the GPU.  One warm-up texturing of a small part of the mesh,
then one timed run of texture.texture_mesh over the whole mesh: device events per phase (project + z-buffer, score, edge sort +
components, rank + boxes, fill + texture coordinates), host seconds for packing and (--write 1) for writing the PLY and the
pages to a temporary folder.  One JSON line.  With --seam_level 1 the same run also levels the seams (csrc/texture_level.hip): the
line then holds the three level_* phases, `device_ms_base` (the five phases every run has: the yardstick), the node graph's
sizes, the iterations, and the solve's traffic per iteration counted from the array sizes (the CSR once, the fp64 vectors
as the three passes read and write them: 11 vector passes of 24 bytes per node) over the level_solve time.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import ada_mvs_amd  # noqa: E402,F401

TARGET_MS = 100.0              # device-side, all five views, edge sort included (an estimate, not a measurement)


def whole_mesh(views, pts, voxel, trunc, B, device):
    """-> (xyz float64, rgb uint8, faces int32) of the welded mesh on the device."""
    import torch
    from ada_mvs_amd import mesh
    mu = trunc * voxel
    allp = torch.cat(pts)
    lo = allp.min(0).values.cpu().numpy() - mu
    hi = allp.max(0).values.cpu().numpy() + mu
    origin, nb = mesh.grid_for_bounds(lo, hi, voxel, B)
    m = mesh.TsdfMesher(origin, voxel, mu, B, views)
    parts, nv = [], 0
    for b in mesh.active_bricks(pts, origin, voxel, mu, B, nb, device):
        vl = m.view_list(b)
        if not vl:
            continue
        xyz, rgb, f = m.extract(b, m.integrate(b, vl))
        parts.append((xyz, rgb, f.to(torch.int64) + nv))
        nv += xyz.shape[0]
    xyz, f, rgb = mesh.weld(torch.cat([p[0] for p in parts]), torch.cat([p[2] for p in parts]), torch.cat([p[1] for p in parts]))
    return xyz, rgb, f.to(torch.int32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--voxel", type=float, default=0.25)
    ap.add_argument("--page", type=int, default=8192)
    ap.add_argument("--write", type=int, default=1, help="also time writing the PLY and the pages (to a temporary folder)")
    ap.add_argument("--seam_level", type=int, default=0, help="1: level the seams too and report the level_* phases")
    ap.add_argument("--seam_tol", type=float, default=1e-4)
    ap.add_argument("--seam_iters", type=int, default=1000)
    args = ap.parse_args()
    import torch
    from ada_mvs_amd import fusion, texture
    from mesh_bench import fused_scene
    if not torch.cuda.is_available():
        raise SystemExit("texture_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    dev = torch.device("cuda")
    t0 = time.time()
    views, pts = fused_scene(args.H, args.W, dev)
    xyz, rgb, faces = whole_mesh(views, pts, args.voxel, 4.0, 128, dev)
    tviews = [dict(iid=i, K=v["K"], R=v["R"], C=v["C"], rgba=v["rgba"]) for i, v in enumerate(views)]
    setup_s = time.time() - t0
    tol = 2.0 * args.voxel
    level = dict(seam_level=True, seam_tol=args.seam_tol, seam_iters=args.seam_iters) if args.seam_level else {}
    texture.texture_mesh(xyz, rgb, faces[:100000], tviews, tol, page=args.page, device=dev, **level)         # warm-up
    torch.cuda.synchronize()
    t1 = time.time()
    res = texture.texture_mesh(xyz, rgb, faces, tviews, tol, page=args.page, device=dev, **level)
    run_s = time.time() - t1
    out = {"workload": "texture", "H": args.H, "W": args.W, "views": len(views), "voxel": args.voxel, "vertices": int(xyz.shape[0]),
           "faces": res["faces"], "faces_textured": res["faces_textured"], "faces_untextured": res["faces_untextured"],
           "charts": res["charts_count"], "component_rounds": res["component_rounds"], "pages": res["pages"], "P": res["P"],
           "box_fraction": round(res["box_fraction"], 4), "device_ms": {k: round(v, 3) for k, v in res["device_ms"].items()},
           "device_ms_total": round(res["device_ms_total"], 3), "target_device_ms": TARGET_MS,
           "meets_target": res["device_ms_total"] <= TARGET_MS, "pack_s": round(res["pack_seconds"], 3), "texture_mesh_s": round(run_s, 3)}
    if args.seam_level:
        n, nnz, it = res["nodes"], res["graph_entries"], res["seam_iterations"]
        bytes_per_iter = 4 * (n + 1) + 4 * nnz + 11 * 24 * n
        solve_ms = res["device_ms"]["level_solve"]
        base = sum(res["device_ms"][k] for k in texture.PHASES)
        out.update({"device_ms_base": round(base, 3), "nodes": n, "graph_entries": nnz, "data_edges": res["data_edges"],
                    "seam_edges": res["seam_edges"], "seam_tol": args.seam_tol, "seam_iters": args.seam_iters, "seam_iterations": it,
                    "seam_cap_hit": res["seam_cap_hit"], "seam_residual": [float("%.3g" % r) for r in res["seam_residual"]],
                    "seam_rms_before": round(res["seam_rms_before"], 4), "seam_rms_after": round(res["seam_rms_after"], 4),
                    "solve_bytes_per_iteration": bytes_per_iter, "solve_ms_per_iteration": round(solve_ms / max(it, 1), 4),
                    "solve_tb_per_s": round(bytes_per_iter * it / (solve_ms * 1e-3) / 1e12, 3) if solve_ms > 0 else None,
                    "copy_rate_tb_per_s": 6.3, "level_over_base": round((res["device_ms_total"] - base) / base, 3)})
        out["meets_target"] = base <= TARGET_MS
    if args.write:
        verts = np.zeros(int(xyz.shape[0]), fusion.PLY_DTYPE)
        x = xyz.cpu().numpy()
        c = rgb.cpu().numpy()
        verts["x"], verts["y"], verts["z"] = x[:, 0], x[:, 1], x[:, 2]
        verts["red"], verts["green"], verts["blue"] = c[:, 0], c[:, 1], c[:, 2]
        with tempfile.TemporaryDirectory() as d:
            texture.write_outputs(os.path.join(d, "mesh_textured"), verts, faces.cpu().numpy().view(np.uint32), res)
        out["write_s"] = round(res["write_seconds"], 3)
    out["setup_s"] = round(setup_s, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
