"""Mesh simplification: the TSDF mesh reduced by vertex clustering on a lattice, one Garland-Heckbert quadric per cell (Lindstrom's
out-of-core simplification), on the GPU.

    python simplify_whu.py --output_folder <predict output> [--mesh <output_folder>/mesh.ply] [--cell M | --cell_voxels 4]
                           [--origin X Y Z] [--rank_eps 1e-3] [--out <mesh minus .ply>_simplified.ply]

The step after mesh_whu.py and before texture_whu.py.  Every vertex falls into a cubic cell of side c (--cell in metres, or
--cell_voxels times the voxel recorded in `<mesh>.json`); all vertices of a cell become one, placed at the minimiser of the
cell's quadric (the sum of squared, area-weighted distances to the planes of every face that touches the cell) nearest to the
members' mean and kept inside the cell; faces whose corners no longer lie in three distinct cells disappear, and of the faces
that fold onto the same three cells the first stays.  Flat ground and flat roofs collapse to a few faces per cell; edges and
corners keep their place, because the minimiser lands on them.  include/adamvs_hip.h "Mesh simplification" states every
operation, csrc/mesh_simplify.hip holds the kernels; the sorts that bring a cell's faces and vertices into runs are torch's.
The result is a function of the mesh as a set: it does not depend on the order of the vertices, and on the order of the faces
only in which of several faces with the same three cells survives.

The mesh is welded by exact position first (mesh.weld), always, so the result does not depend on mesh_whu.py's --brick or
--weld.  `<out>.json` carries the input JSON's voxel, mu, origin and views unchanged (texture_whu.py's default occlusion
tolerance keeps working) and adds the cell, the lattice origin, the source, the counts and the timings.  The default lattice
origin is (the volume origin of `<mesh>.json`, else the per-axis vertex minimum) - c / 3: unshifted, a ground plane at a round
height sits exactly on a cell boundary and splits into two sheets of cells.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

CARRIED = ("voxel", "mu", "origin", "views")      # of <mesh>.json, unchanged into <out>.json
DEFAULT_CELL_VOXELS = 4.0
MAX_COUNT = (1 << 31) - 1


def check_options(cell, rank_eps=1e-3):
    if not (isinstance(cell, (int, float)) and math.isfinite(float(cell)) and float(cell) > 0):
        raise ValueError("cell=%r must be finite and > 0" % (cell,))
    if not (math.isfinite(float(rank_eps)) and 0 <= float(rank_eps) < 1):
        raise ValueError("rank_eps=%r (0 <= rank_eps < 1)" % (rank_eps,))


def default_out(mesh_path):
    return (mesh_path[:-4] if mesh_path.lower().endswith(".ply") else mesh_path) + "_simplified.ply"


def default_lattice_origin(cell, meta_origin, vertex_min):
    """(the volume origin of <mesh>.json, else the per-axis vertex minimum) - c / 3 per axis, lowered by whole cells where a
    vertex lies below it (the lattice origin must not exceed any vertex)."""
    base = np.asarray(meta_origin if meta_origin is not None else vertex_min, np.float64).reshape(3)
    o = base - float(cell) / 3.0
    if vertex_min is not None:
        vmin = np.asarray(vertex_min, np.float64).reshape(3)
        o = o - np.ceil(np.maximum(o - vmin, 0.0) / float(cell)) * float(cell)
    return o


def resolve_cell(cell, cell_voxels, meta):
    """--cell M, or --cell_voxels K (default 4) times the voxel of <mesh>.json."""
    if cell is not None and cell_voxels is not None:
        raise ValueError("give --cell or --cell_voxels, not both")
    if cell is not None:
        check_options(cell)
        return float(cell)
    k = DEFAULT_CELL_VOXELS if cell_voxels is None else float(cell_voxels)
    if not (math.isfinite(k) and k > 0):
        raise ValueError("cell_voxels=%r must be finite and > 0" % (cell_voxels,))
    if meta is None or "voxel" not in meta:
        raise ValueError("<mesh>.json with the voxel size is absent: give --cell")
    return k * float(meta["voxel"])


def summary(meta, info, cell, lattice_origin, source, out, seconds, device_seconds):
    """The dict written to <out>.json: the carried keys of <mesh>.json first, unchanged."""
    res = {k: meta[k] for k in CARRIED if meta is not None and k in meta}
    res.update(cell=float(cell), lattice_origin=[float(v) for v in lattice_origin], source=source, ply=out)
    res.update(info)
    res.update(vertices=int(info["cells_used"]), faces=int(info["faces_out"]), seconds=float(seconds), device_seconds=float(device_seconds))
    return res


def _empty(device):
    import torch
    return (torch.empty(0, 3, device=device, dtype=torch.float64), torch.empty(0, 3, device=device, dtype=torch.uint8),
            torch.empty(0, 3, device=device, dtype=torch.int32))


def simplify(xyz, rgb, faces, cell, origin=None, rank_eps=1e-3, detail=None, timing=None):
    """xyz [nv, 3] float64, rgb [nv, 3] uint8, faces [nf, 3] int32 (uint32) or int64: device tensors -> (xyz, rgb, faces int32
    (uint32), info) of the simplified mesh; info: cells, cells_used, vertices_in (after the weld), faces_in, faces_collapsed,
    faces_duplicate, faces_out, rank_hist (cells of rank 0 .. 3), fallbacks.  origin: the lattice origin (default: the vertex
    minimum - cell / 3).  detail: a dict that receives the intermediates (device tensors); timing: a list that receives
    (name, start event, end event) of the stages."""
    import torch
    from . import _lib, hip_ops, mesh
    check_options(cell, rank_eps)
    for name, t in (("xyz", xyz), ("rgb", rgb), ("faces", faces)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.AdaMVSHipError("%s must be a GPU tensor: mesh simplification has no CPU fallback" % name)
    if xyz.dtype != torch.float64 or rgb.dtype != torch.uint8 or faces.dtype not in (torch.int32, torch.int64):
        raise _lib.AdaMVSHipError("xyz float64, rgb uint8, faces int32 / int64: got %s, %s, %s" % (xyz.dtype, rgb.dtype, faces.dtype))
    if xyz.dim() != 2 or xyz.shape[1] != 3 or tuple(rgb.shape) != tuple(xyz.shape) or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.AdaMVSHipError("xyz [nv, 3], rgb [nv, 3], faces [nf, 3]: got %s, %s, %s" % (tuple(xyz.shape), tuple(rgb.shape), tuple(faces.shape)))
    dev, c = xyz.device, float(cell)
    marks = []

    def stage(name):
        if timing is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

    info = dict(cells=0, cells_used=0, vertices_in=int(xyz.shape[0]), faces_in=int(faces.shape[0]), faces_collapsed=int(faces.shape[0]),
                faces_duplicate=0, faces_out=0, rank_hist=[0, 0, 0, 0], fallbacks=0)
    if xyz.shape[0] == 0:
        if faces.shape[0]:
            raise _lib.AdaMVSHipError("%d faces without vertices" % faces.shape[0])
        return _empty(dev) + (info,)
    if faces.shape[0] > MAX_COUNT or xyz.shape[0] > MAX_COUNT:
        raise _lib.AdaMVSHipError("more than 2^31 - 1 vertices or faces")
    f64 = faces.to(torch.int64) & 0xFFFFFFFF
    if faces.shape[0] and int(f64.max()) >= xyz.shape[0]:
        raise _lib.AdaMVSHipError("a face refers to vertex %d of %d" % (int(f64.max()), xyz.shape[0]))
    stage("weld")
    xyz, f64, rgb = mesh.weld(xyz.contiguous(), f64, rgb.contiguous())
    nv, nf = int(xyz.shape[0]), int(f64.shape[0])
    info["vertices_in"] = nv
    o = np.asarray(origin, np.float64).reshape(3) if origin is not None else default_lattice_origin(c, None, xyz.min(0).values.cpu().numpy())
    if not np.isfinite(o).all():
        raise _lib.AdaMVSHipError("the lattice origin %r is not finite (a vertex is not?)" % (o,))
    stage("keys")
    keys, bad = hip_ops.simplify_keys(xyz, c, o)
    if int(bad.max()):
        raise _lib.AdaMVSHipError("simplify: %d vertices are not finite, %d lie outside the lattice of 2^21 cells per axis (cell %g, lattice "
                                  "origin %s)" % (int((bad == 1).sum()), int((bad == 2).sum()), c, o.tolist()))
    stage("sort_cells")
    ukeys, vcell64 = torch.unique(keys, return_inverse=True)
    nc = int(ukeys.numel())
    info["cells"] = nc
    vcell = vcell64.to(torch.int32)
    vorder = torch.sort(vcell, stable=True).indices
    bounds = torch.arange(nc + 1, device=dev, dtype=torch.int32)
    vstart = torch.searchsorted(vcell[vorder].contiguous(), bounds).to(torch.int64)
    if nf == 0:
        return _empty(dev) + (info,)
    faces32 = f64.to(torch.int32).contiguous()
    # the canonical face list of step 2: corners ascending by (welded) vertex number, faces ascending by those triples
    stage("sort_canonical")
    fs = torch.sort(f64, dim=1).values
    corder = torch.sort(fs[:, 2], stable=True).indices
    corder = corder[torch.sort(((fs[:, 0] << 31) | fs[:, 1])[corder], stable=True).indices]
    faces_c = fs[corder].to(torch.int32).contiguous()
    stage("corners")
    fcell, _, survive = hip_ops.simplify_corners(faces32, vcell, nc)
    _, entry_cell, _ = hip_ops.simplify_corners(faces_c, vcell, nc)
    stage("sort_entries")
    es = torch.sort(entry_cell.reshape(-1), stable=True)
    fstart = torch.searchsorted(es.values, bounds).to(torch.int64)
    stage("accumulate")
    quadric, member, colour = hip_ops.simplify_accumulate(ukeys, c, o, xyz, rgb, faces_c, es.indices, fstart, vorder, vstart)
    stage("solve")
    pos, col, rank, fallback, error = hip_ops.simplify_solve(ukeys, c, o, rank_eps, quadric, member, colour, vstart)
    stage("sort_faces")
    surv = torch.nonzero(survive).reshape(-1)
    ns = int(surv.numel())
    if ns:
        tri = hip_ops.simplify_triples(fcell, surv)
        order = torch.sort(tri[2], stable=True).indices                     # least significant first: lexicographic, stable
        order = order[torch.sort(tri[1][order], stable=True).indices]
        order = order[torch.sort(tri[0][order], stable=True).indices]
        stage("first")
        keep = hip_ops.simplify_first(tri, surv, order.contiguous(), nf)
    else:
        keep = torch.zeros(nf, device=dev, dtype=torch.uint8)
    stage("emit")
    out_xyz, out_rgb, out_faces, used = hip_ops.simplify_emit(pos, col, fcell, keep)
    stage("end")
    if timing is not None:
        timing.extend((a[0], a[1], b[1]) for a, b in zip(marks[:-1], marks[1:]))
    nk = int(out_faces.shape[0])
    info.update(cells_used=int(out_xyz.shape[0]), faces_collapsed=nf - ns, faces_duplicate=ns - nk, faces_out=nk,
                rank_hist=[int(v) for v in torch.bincount(rank.to(torch.int64), minlength=4).cpu().tolist()[:4]],
                fallbacks=int(fallback.sum()), quadric_error=float(error[used.bool()].sum()))
    if detail is not None:
        detail.update(xyz=xyz, rgb=rgb, faces=faces32, lattice_origin=o, keys=ukeys, vcell=vcell, fcell=fcell, survive=survive, keep=keep,
                      used=used, quadric=quadric, member=member, colour=colour, pos=pos, col=col, rank=rank, fallback=fallback, error=error)
    return out_xyz, out_rgb, out_faces, info


def from_file(mesh_path, out=None, cell=None, cell_voxels=None, origin=None, rank_eps=1e-3, device=None, log=print):
    """Simplify the mesh PLY mesh_whu.py wrote -> the summary dict also written to <out>.json."""
    import torch
    from . import mesh
    t_start = time.time()
    meta = None
    if os.path.exists(mesh_path + ".json"):
        with open(mesh_path + ".json") as f:
            meta = json.load(f)
    c = resolve_cell(cell, cell_voxels, meta)
    check_options(c, rank_eps)
    if not torch.cuda.is_available():
        raise RuntimeError("simplify: needs an MI355X (there is no CPU fallback for the simplification kernels)")
    out = out or default_out(mesh_path)
    device = torch.device(device if device is not None else "cuda")
    verts, faces = mesh.read_mesh_ply(mesh_path)
    xyz_h = np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float64)
    rgb_h = np.stack([verts["red"], verts["green"], verts["blue"]], 1)
    if origin is not None:
        o = np.asarray(origin, np.float64).reshape(3)
    elif len(xyz_h):
        o = default_lattice_origin(c, meta.get("origin") if meta else None, xyz_h.min(0))
    else:
        o = default_lattice_origin(c, meta.get("origin") if meta else np.zeros(3), None)
    xyz = torch.from_numpy(np.ascontiguousarray(xyz_h)).to(device)
    rgb = torch.from_numpy(np.ascontiguousarray(rgb_h)).to(device)
    f = torch.from_numpy(faces.astype(np.int64)).to(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sx, sc, sf, info = simplify(xyz, rgb, f, c, o, rank_eps)
    e1.record()
    torch.cuda.synchronize(device)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with mesh.MeshPlyWriter(out) as w:
        w.write(sx.cpu().numpy(), sc.cpu().numpy(), sf.cpu().numpy().view(np.uint32))
    res = summary(meta, info, c, o, mesh_path, out, time.time() - t_start, e0.elapsed_time(e1) / 1e3)
    with open(out + ".json", "w") as fj:
        json.dump(res, fj, indent=1)
        fj.write("\n")
    log("simplify: %d -> %d vertices, %d -> %d faces (%d collapsed, %d duplicate) over %d cells of %g m (%d fallbacks) into %s, "
        "device %.3f s, total_time = %.3f s" % (info["vertices_in"], res["vertices"], info["faces_in"], res["faces"], info["faces_collapsed"],
                                                info["faces_duplicate"], info["cells"], c, info["fallbacks"], out, res["device_seconds"],
                                                res["seconds"]))
    return res


def build_parser():
    ap = argparse.ArgumentParser(description="Simplify the TSDF mesh by quadric vertex clustering on a lattice")
    ap.add_argument("--mesh", default=None, help="mesh PLY of mesh_whu.py (default <output_folder>/mesh.ply)")
    ap.add_argument("--output_folder", default=None, help="predict_whu.py's output folder, after mesh_whu.py")
    ap.add_argument("--cell", type=float, default=None, metavar="M", help="cell size in metres")
    ap.add_argument("--cell_voxels", type=float, default=None, metavar="K",
                    help="cell size in voxels of <mesh>.json (default %g; needs <mesh>.json)" % DEFAULT_CELL_VOXELS)
    ap.add_argument("--origin", type=float, nargs=3, metavar=("X", "Y", "Z"), default=None,
                    help="lattice origin (default: the volume origin of <mesh>.json, else the vertex minimum, minus a third of a cell)")
    ap.add_argument("--rank_eps", type=float, default=1e-3, help="an eigenvalue of a cell's quadric counts iff it exceeds this share of the largest")
    ap.add_argument("--out", default=None, help="PLY to write (default <mesh minus .ply>_simplified.ply); the summary goes to <out>.json")
    return ap


def mesh_path_of(args):
    if args.mesh:
        return args.mesh
    if not args.output_folder:
        raise ValueError("give --mesh or --output_folder")
    return os.path.join(args.output_folder, "mesh.ply")


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    if args.cell is not None and args.cell_voxels is not None:
        raise SystemExit("simplify: give --cell or --cell_voxels, not both")
    return from_file(mesh_path_of(args), args.out, args.cell, args.cell_voxels, args.origin, args.rank_eps)


if __name__ == "__main__":
    main()
