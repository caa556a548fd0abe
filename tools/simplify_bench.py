"""Mesh simplification timing (csrc/mesh_simplify.hip through ada_mvs_amd/simplify.py) on the TSDF mesh of the fused analytic scene.
    python tools/simplify_bench.py [--H 2752 --W 1856] [--voxel 0.25] [--cell_voxels 2,4,8] [--brick 128] [--runs 10] [--cpu_faces 200000]
The 5-view scene of tools/mesh_bench.py meshed at --voxel and welded, held on the device.  Per cell size, 2 warm-ups and then
--runs calls of simplify(): device events around the whole call and around every stage, the median over the runs.  `sort_ms` is
what torch does (the weld, the unique of the keys, the stable sorts that bring a cell's faces and vertices into runs, the
canonical face order, the sort of the surviving faces' triples); `kernel_ms` is the rest: the kernels of mesh_simplify.hip with
their launches and the two read-backs.  The byte model below is priced against 6.3 TB/s over kernel_ms.  The CPU baseline is
the numpy restatement (tests/simplify_ref.py) on the first --cpu_faces faces of the welded mesh (a slab: the weld orders the
vertices by x).  One JSON line; there is no pass bar, nothing of this had a number before.
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
SORT_STAGES = ("weld", "sort_cells", "sort_canonical", "sort_entries", "sort_faces")


def kernel_bytes(nv, nf, ne, nc, ns, nu, nk):
    """Algorithmic bytes of the kernels of one call.  keys: 24 B read, 9 B written per vertex.  corners, twice (the faces as given
    and the canonical list): 12 B of indices and three 4 B cell taps read, 25 B written per face.  accumulate: per (cell, face)
    entry 8 B of order, 12 B of indices and three 24 B vertices; per vertex 8 B of order, 24 B of position, 3 B of colour; 128 B
    written per cell.  solve: 152 B read and 45 B written per cell.  triples and first: 20 + 12 B and 16 + 24 + 1 B per surviving
    face.  mark, the two counts, emit: 1 B of flag per face three times, 12 B of cells and 3 stores per kept face twice, 2 B per
    cell, 28 B read and 31 B written per used cell, 12 B written per kept face."""
    return (33 * nv + 2 * 49 * nf + 92 * ne + 35 * nv + 128 * nc + 197 * nc + 73 * ns + 3 * nf + 2 * 15 * nk + 2 * nc + 59 * nu + 12 * nk)


def build_mesh(H, W, voxel, trunc, B, device):
    """-> (xyz, rgb, faces int64) of the welded mesh on the device, the volume origin."""
    import torch
    from ada_mvs_amd import mesh
    from mesh_bench import fused_scene
    views, pts = fused_scene(H, W, device)
    mu = trunc * voxel
    allp = torch.cat(pts)
    lo = allp.min(0).values.cpu().numpy() - mu
    hi = allp.max(0).values.cpu().numpy() + mu
    origin, nb = mesh.grid_for_bounds(lo, hi, voxel, B)
    m = mesh.TsdfMesher(origin, voxel, mu, B, views)
    xs, cs, fs, base = [], [], [], 0
    for b in mesh.active_bricks(pts, origin, voxel, mu, B, nb, device):
        vl = m.view_list(b)
        if not vl:
            continue
        xyz, rgb, f = m.extract(b, m.integrate(b, vl), 0)
        xs.append(xyz), cs.append(rgb), fs.append((f.to(torch.int64) & 0xFFFFFFFF) + base)
        base += xyz.shape[0]
    xyz, faces, rgb = mesh.weld(torch.cat(xs), torch.cat(fs), torch.cat(cs))
    return xyz, rgb, faces, origin


def run(xyz, rgb, faces, cell, origin, runs, warmup=2):
    import torch
    from ada_mvs_amd import simplify
    o = simplify.default_lattice_origin(cell, origin, None)
    per_stage, totals, info, detail = {}, [], None, {}
    for i in range(warmup + runs):
        timing = []
        d = detail if i == 0 else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, _, _, info = simplify.simplify(xyz, rgb, faces, cell, o, detail=d, timing=timing)
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
    fc = detail["fcell"]
    ne = int((1 + (fc[:, 1] != fc[:, 0]).long() + ((fc[:, 2] != fc[:, 0]) & (fc[:, 2] != fc[:, 1])).long()).sum())
    ns = info["faces_in"] - info["faces_collapsed"]
    nbytes = kernel_bytes(info["vertices_in"], info["faces_in"], ne, info["cells"], ns, info["cells_used"], info["faces_out"])
    return dict(cell=cell, device_ms=round(total, 3), sort_ms=round(sort_ms, 3), kernel_ms=round(kernel_ms, 3),
                stage_ms={k: round(v, 3) for k, v in stages.items()}, vertices_in=info["vertices_in"], faces_in=info["faces_in"],
                cells=info["cells"], vertices_out=info["cells_used"], faces_out=info["faces_out"], faces_duplicate=info["faces_duplicate"],
                fallbacks=info["fallbacks"], rank_hist=info["rank_hist"], entries=ne, entries_per_cell=round(ne / max(info["cells"], 1), 1),
                ns_per_face_in=round(total * 1e6 / max(info["faces_in"], 1), 3), bytes=int(nbytes),
                gb_per_s=round(nbytes / (kernel_ms * 1e-3) / 1e9, 1), frac_of_6_3_tbs=round(nbytes / (kernel_ms * 1e-3) / 1e9 / HBM_GBS, 4))


def cpu_baseline(xyz, rgb, faces, n, cell, origin):
    import simplify_ref as S
    from ada_mvs_amd import simplify
    f = faces[:n].cpu().numpy()
    used, inv = np.unique(f, return_inverse=True)
    x, c = xyz.cpu().numpy()[used], rgb.cpu().numpy()[used]
    t0 = time.time()
    r = S.simplify(x, c, inv.reshape(-1, 3), cell, simplify.default_lattice_origin(cell, origin, None), weld_first=False)
    return time.time() - t0, len(f), r["info"]["faces_out"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--voxel", type=float, default=0.25)
    ap.add_argument("--trunc", type=float, default=4.0)
    ap.add_argument("--brick", type=int, default=128)
    ap.add_argument("--cell_voxels", default="2,4,8")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--cpu_faces", type=int, default=200000, help="faces of the crop the numpy restatement is timed on (0: skip)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("simplify_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    dev = torch.device("cuda")
    t0 = time.time()
    xyz, rgb, faces, origin = build_mesh(args.H, args.W, args.voxel, args.trunc, args.brick, dev)
    res = {"workload": "simplify", "H": args.H, "W": args.W, "voxel": args.voxel, "vertices": int(xyz.shape[0]), "faces": int(faces.shape[0]),
           "runs": args.runs, "setup_s": round(time.time() - t0, 2), "per_cell_voxels": {}}
    for k in (float(v) for v in args.cell_voxels.split(",")):
        res["per_cell_voxels"]["%g" % k] = run(xyz, rgb, faces, k * args.voxel, origin, args.runs)
    if args.cpu_faces:
        s, n, nout = cpu_baseline(xyz, rgb, faces, args.cpu_faces, 4.0 * args.voxel, origin)
        res["cpu_restatement"] = dict(faces_in=n, faces_out=nout, seconds=round(s, 3), ns_per_face_in=round(s * 1e9 / max(n, 1), 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
