"""Mesh smoothing: the TSDF mesh denoised by bilateral normal filtering (Zheng, Fu, Au, Tai: the local iterative scheme), on the GPU.

    python smooth_whu.py --output_folder <predict output> [--mesh <output_folder>/mesh.ply] [--sigma_s M | --sigma_s_voxels 1]
                         [--sigma_r 0.35] [--normal_iters 10] [--vertex_iters 10] [--max_move M | --max_move_voxels 1]
                         [--no_fix_boundary] [--origin X Y Z] [--out <mesh minus .ply>_smoothed.ply]

The step after mesh_whu.py and before simplify_whu.py (clean_whu.py, ada_mvs_amd/clean.py, goes in front of it: it drops
floaters and closes the pinholes whose rims this step would pin).  The zero level set of a TSDF built from predicted depth carries the
voxel lattice's staircase and the depth noise the truncation band did not average out.  Here every face normal becomes the
weighted mean of the normals of the faces around it, weighted by area, by the distance between the centroids (sigma_s) and by
the difference between the normals (sigma_r): across a crease the last weight vanishes, so flat ground and roofs flatten and
roof edges and facade corners stay.  The vertices then move, a few Jacobi passes, towards the planes of their faces' new
normals, never farther than the cap from where they were; with the boundary fixed, the vertices of open edges do not move at
all.  Faces, their order and the colours leave unchanged.  include/adamvs_hip.h "Mesh smoothing" states every operation,
csrc/mesh_smooth.hip holds the kernels; the sorts that bring a vertex's faces into runs and equal edges together are torch's.

The mesh is welded by exact position first (mesh.weld), always, so the result does not depend on mesh_whu.py's --brick or
--weld.  `<out>.json` carries the input JSON's voxel, mu, origin and views unchanged (simplify_whu.py --cell_voxels and
texture_whu.py's default occlusion tolerance keep working on the smoothed mesh) and adds the options, the source, the counts,
the largest and the RMS move and the timings.
"""
import argparse
import sys

import numpy as np

from . import mesh_stage
from .mesh_stage import CARRIED, MAX_COUNT, mesh_path_of, positive as _positive  # noqa: F401  (shared with simplify.py and clean.py)

DEFAULT_SIGMA_S_VOXELS = 1.0
DEFAULT_SIGMA_R = 0.35
DEFAULT_ITERS = 10
DEFAULT_MAX_MOVE_VOXELS = 1.0
MAX_ITERS = 1000
MAX_FACES = MAX_COUNT // 3                    # the 3 nf (vertex, face) entries are counted in 31 bits


def _iters(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= MAX_ITERS:
        raise ValueError("%s=%r must be an integer in 0 .. %d" % (name, v, MAX_ITERS))


def check_options(sigma_s, sigma_r=DEFAULT_SIGMA_R, normal_iters=DEFAULT_ITERS, vertex_iters=DEFAULT_ITERS, max_move=1.0):
    _positive("sigma_s", sigma_s)
    _positive("sigma_r", sigma_r)
    _iters("normal_iters", normal_iters)
    _iters("vertex_iters", vertex_iters)
    _positive("max_move", max_move)


def default_out(mesh_path):
    return mesh_stage.default_out(mesh_path, "_smoothed")


def resolve_sigma_s(sigma_s, sigma_s_voxels, meta):
    """--sigma_s M, or --sigma_s_voxels K (default 1) times the voxel of <mesh>.json."""
    return mesh_stage.resolve_metres("sigma_s", sigma_s, sigma_s_voxels, DEFAULT_SIGMA_S_VOXELS, meta)


def resolve_max_move(max_move, max_move_voxels, meta):
    """--max_move M, or --max_move_voxels K (default 1) times the voxel of <mesh>.json."""
    return mesh_stage.resolve_metres("max_move", max_move, max_move_voxels, DEFAULT_MAX_MOVE_VOXELS, meta)


def summary(meta, info, options, origin, source, out, seconds, device_seconds, stage_seconds=None):
    """The dict written to <out>.json: the carried keys of <mesh>.json first, unchanged."""
    return mesh_stage.summary(meta, dict(options, smooth_origin=[float(v) for v in origin], source=source, ply=out), info,
                              seconds=float(seconds), device_seconds=float(device_seconds), stage_seconds=dict(stage_seconds or {}))


def smooth(xyz, rgb, faces, sigma_s, sigma_r=DEFAULT_SIGMA_R, normal_iters=DEFAULT_ITERS, vertex_iters=DEFAULT_ITERS, max_move=None,
           fix_boundary=True, origin=None, detail=None, timing=None):
    """xyz [nv, 3] float64, rgb [nv, 3] uint8, faces [nf, 3] int32 (uint32) or int64: device tensors -> (xyz, rgb, faces int32
    (uint32), info) of the welded mesh with its positions smoothed; info: vertices (after the weld), faces, fixed,
    degenerate_faces, clamped (in the last pass), largest_move, rms_move.  sigma_s, max_move: metres (max_move is required).
    origin: O (default: the per-axis vertex minimum).  detail: a dict that receives the intermediates (device tensors);
    timing: a list that receives (name, start event, end event) of the stages."""
    import torch
    from . import _lib, hip_ops
    if max_move is None:
        raise ValueError("max_move (metres) is required")
    check_options(sigma_s, sigma_r, normal_iters, vertex_iters, max_move)
    clock = mesh_stage.StageClock(timing)
    stage = clock.stage
    welded = mesh_stage.enter("mesh smoothing", xyz, rgb, faces, MAX_FACES, clock)
    dev = xyz.device
    normal_iters, vertex_iters = int(normal_iters), int(vertex_iters)
    info = dict(vertices=int(xyz.shape[0]), faces=int(faces.shape[0]), fixed=0, degenerate_faces=0, clamped=0, largest_move=0.0, rms_move=0.0)
    if welded is None:
        return mesh_stage.empty_mesh(dev) + (info,)
    xyz, f64, rgb = welded
    nv, nf = int(xyz.shape[0]), int(f64.shape[0])
    info["vertices"] = nv
    o = np.asarray(origin, np.float64).reshape(3) if origin is not None else xyz.min(0).values.cpu().numpy()
    if not np.isfinite(o).all() or not bool(torch.isfinite(xyz).all()):
        raise _lib.AdaMVSHipError("smooth: a vertex or the origin %r is not finite" % (o,))
    faces32 = f64.to(torch.int32).contiguous()
    if nf == 0:
        if detail is not None:
            detail.update(xyz=xyz, rgb=rgb, faces=faces32, origin=o, p0=xyz - torch.from_numpy(o).to(dev), p=xyz - torch.from_numpy(o).to(dev),
                          fixed=torch.zeros(nv, device=dev, dtype=torch.uint8), clamped=torch.zeros(nv, device=dev, dtype=torch.uint8))
        return xyz, rgb, faces32, info
    o_dev = torch.from_numpy(o).to(dev)
    p0 = (xyz - o_dev).contiguous()
    # step 2: the (vertex, face) entries in runs by vertex; a corner that repeats an earlier corner of its face sorts to the end
    stage("sort_incidence")
    ent = f64.clone()
    ent[:, 1][f64[:, 1] == f64[:, 0]] = nv
    ent[:, 2][(f64[:, 2] == f64[:, 0]) | (f64[:, 2] == f64[:, 1])] = nv
    es = torch.sort(ent.reshape(-1), stable=True)
    vface = (es.indices // 3).to(torch.int32).contiguous()
    vstart = torch.searchsorted(es.values, torch.arange(nv + 1, device=dev, dtype=torch.int64)).to(torch.int64).contiguous()
    stage("faces")
    rec = hip_ops.smooth_faces(p0, faces32)
    stage("boundary")                                   # two kernels around torch's sort of the edge keys
    fixed = hip_ops.smooth_boundary(faces32, nv) if fix_boundary else torch.zeros(nv, device=dev, dtype=torch.uint8)
    stage("filter")
    n0 = rec[:, 4:7].contiguous()
    normals, spare = n0, None
    for _ in range(normal_iters):
        out = hip_ops.smooth_filter(rec, normals, faces32, nv, vface, vstart, sigma_s, sigma_r, out=spare)
        spare = normals if normals is not n0 else None
        normals = out
    stage("update")
    p, spare = p0, None
    cen = torch.empty(nf, 3, device=dev, dtype=torch.float64)
    clamped = torch.zeros(nv, device=dev, dtype=torch.uint8)
    for _ in range(vertex_iters):
        hip_ops.smooth_centroids(p, faces32, out=cen)
        out, _ = hip_ops.smooth_update(p0, p, normals, cen, vface, vstart, fixed, max_move, out=spare, clamped=clamped)
        spare = p if p is not p0 else None
        p = out
    stage("finish")
    count = vstart[1:] - vstart[:-1]
    moved = (fixed == 0) & (count > 0) if vertex_iters else torch.zeros(nv, device=dev, dtype=torch.bool)
    out_xyz = torch.where(moved[:, None], o_dev + p, xyz)
    move2 = ((p - p0) ** 2).sum(1)
    stats = torch.stack([move2.max().sqrt(), move2.mean().sqrt(), fixed.sum().to(torch.float64), clamped.sum().to(torch.float64),
                         (rec[:, 3] == 0).sum().to(torch.float64)]).cpu().tolist()
    clock.end()
    info.update(largest_move=float(stats[0]), rms_move=float(stats[1]), fixed=int(stats[2]), clamped=int(stats[3]), degenerate_faces=int(stats[4]))
    if detail is not None:
        detail.update(xyz=xyz, rgb=rgb, faces=faces32, origin=o, p0=p0, p=p, rec=rec, normals=normals, vface=vface, vstart=vstart, fixed=fixed,
                      clamped=clamped, moved=moved)
    return out_xyz, rgb, faces32, info


def from_file(mesh_path, out=None, sigma_s=None, sigma_s_voxels=None, sigma_r=DEFAULT_SIGMA_R, normal_iters=DEFAULT_ITERS,
              vertex_iters=DEFAULT_ITERS, max_move=None, max_move_voxels=None, fix_boundary=True, origin=None, device=None, log=print):
    """Smooth the mesh PLY mesh_whu.py wrote -> the summary dict also written to <out>.json."""
    def resolve(meta):
        ss = resolve_sigma_s(sigma_s, sigma_s_voxels, meta)
        cap = resolve_max_move(max_move, max_move_voxels, meta)
        check_options(ss, sigma_r, normal_iters, vertex_iters, cap)
        return dict(sigma_s=ss, sigma_r=float(sigma_r), normal_iters=int(normal_iters), vertex_iters=int(vertex_iters), max_move=cap,
                    fix_boundary=bool(fix_boundary))

    def run(opt, xyz, rgb, f, o, timing):
        return smooth(xyz, rgb, f, opt["sigma_s"], sigma_r, normal_iters, vertex_iters, opt["max_move"], fix_boundary, o, timing=timing)

    out = out or default_out(mesh_path)
    res, info, _ = mesh_stage.run_file("smooth", "smoothing", mesh_path, out, origin, device, resolve, mesh_stage.volume_origin, run, summary)
    log("smooth: %d vertices, %d faces (%d fixed, %d degenerate faces, %d clamped), largest move %.4g m, rms %.4g m into %s, "
        "device %.3f s, total_time = %.3f s" % (info["vertices"], info["faces"], info["fixed"], info["degenerate_faces"], info["clamped"],
                                                info["largest_move"], info["rms_move"], out, res["device_seconds"], res["seconds"]))
    return res


def build_parser():
    ap = argparse.ArgumentParser(description="Smooth the TSDF mesh by bilateral normal filtering")
    ap.add_argument("--mesh", default=None, help="mesh PLY of mesh_whu.py (default <output_folder>/mesh.ply)")
    ap.add_argument("--output_folder", default=None, help="predict_whu.py's output folder, after mesh_whu.py")
    ap.add_argument("--sigma_s", type=float, default=None, metavar="M", help="spatial sigma in metres")
    ap.add_argument("--sigma_s_voxels", type=float, default=None, metavar="K",
                    help="spatial sigma in voxels of <mesh>.json (default %g; needs <mesh>.json)" % DEFAULT_SIGMA_S_VOXELS)
    ap.add_argument("--sigma_r", type=float, default=DEFAULT_SIGMA_R, help="range sigma, on the difference of unit normals")
    ap.add_argument("--normal_iters", type=int, default=DEFAULT_ITERS, help="passes of the normal filter (0 .. %d)" % MAX_ITERS)
    ap.add_argument("--vertex_iters", type=int, default=DEFAULT_ITERS, help="passes of the vertex update (0 .. %d)" % MAX_ITERS)
    ap.add_argument("--max_move", type=float, default=None, metavar="M", help="cap on a vertex's move from its input position, metres")
    ap.add_argument("--max_move_voxels", type=float, default=None, metavar="K",
                    help="the cap in voxels of <mesh>.json (default %g; needs <mesh>.json)" % DEFAULT_MAX_MOVE_VOXELS)
    ap.add_argument("--no_fix_boundary", action="store_true", help="let the vertices of open edges move too")
    ap.add_argument("--origin", type=float, nargs=3, metavar=("X", "Y", "Z"), default=None,
                    help="origin the arithmetic is relative to (default: the volume origin of <mesh>.json, else the vertex minimum)")
    ap.add_argument("--out", default=None, help="PLY to write (default <mesh minus .ply>_smoothed.ply); the summary goes to <out>.json")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    for name in ("sigma_s", "max_move"):
        if getattr(args, name) is not None and getattr(args, name + "_voxels") is not None:
            raise SystemExit("smooth: give --%s or --%s_voxels, not both" % (name, name))
    return from_file(mesh_path_of(args), args.out, args.sigma_s, args.sigma_s_voxels, args.sigma_r, args.normal_iters, args.vertex_iters,
                     args.max_move, args.max_move_voxels, not args.no_fix_boundary, args.origin)


if __name__ == "__main__":
    main()
