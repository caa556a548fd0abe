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
import math
import sys

import numpy as np

from . import mesh_stage
from .mesh_stage import CARRIED, MAX_COUNT, mesh_path_of  # noqa: F401  (shared with smooth.py and clean.py)

DEFAULT_CELL_VOXELS = 4.0


def check_options(cell, rank_eps=1e-3):
    if not (isinstance(cell, (int, float)) and math.isfinite(float(cell)) and float(cell) > 0):
        raise ValueError("cell=%r must be finite and > 0" % (cell,))
    if not (math.isfinite(float(rank_eps)) and 0 <= float(rank_eps) < 1):
        raise ValueError("rank_eps=%r (0 <= rank_eps < 1)" % (rank_eps,))


def default_out(mesh_path):
    return mesh_stage.default_out(mesh_path, "_simplified")


def default_lattice_origin(cell, meta_origin, vertex_min):
    """(the volume origin of <mesh>.json, else the per-axis vertex minimum) - c / 3 per axis, lowered by whole cells where a
    vertex lies below it (the lattice origin must not exceed any vertex)."""
    base = np.asarray(meta_origin if meta_origin is not None else vertex_min, np.float64).reshape(3)
    o = base - float(cell) / 3.0
    if vertex_min is not None:
        vmin = np.asarray(vertex_min, np.float64).reshape(3)
        o = o - np.ceil(np.maximum(o - vmin, 0.0) / float(cell)) * float(cell)
    return o


def _check_size(name, v):
    """cell as check_options has it; cell_voxels is whatever float() takes."""
    if name == "cell":
        check_options(v)
    elif not (math.isfinite(float(v)) and float(v) > 0):
        raise ValueError("%s=%r must be finite and > 0" % (name, v))


def resolve_cell(cell, cell_voxels, meta):
    """--cell M, or --cell_voxels K (default 4) times the voxel of <mesh>.json."""
    return mesh_stage.resolve_metres("cell", cell, cell_voxels, DEFAULT_CELL_VOXELS, meta, check=_check_size)


def summary(meta, info, cell, lattice_origin, source, out, seconds, device_seconds):
    """The dict written to <out>.json: the carried keys of <mesh>.json first, unchanged."""
    return mesh_stage.summary(meta, dict(cell=float(cell), lattice_origin=[float(v) for v in lattice_origin], source=source, ply=out), info,
                              vertices=int(info["cells_used"]), faces=int(info["faces_out"]), seconds=float(seconds),
                              device_seconds=float(device_seconds))


def simplify(xyz, rgb, faces, cell, origin=None, rank_eps=1e-3, detail=None, timing=None):
    """xyz [nv, 3] float64, rgb [nv, 3] uint8, faces [nf, 3] int32 (uint32) or int64: device tensors -> (xyz, rgb, faces int32
    (uint32), info) of the simplified mesh; info: cells, cells_used, vertices_in (after the weld), faces_in, faces_collapsed,
    faces_duplicate, faces_out, rank_hist (cells of rank 0 .. 3), fallbacks.  origin: the lattice origin (default: the vertex
    minimum - cell / 3).  detail: a dict that receives the intermediates (device tensors); timing: a list that receives
    (name, start event, end event) of the stages."""
    import torch
    from . import _lib, hip_ops
    check_options(cell, rank_eps)
    clock = mesh_stage.StageClock(timing)
    stage = clock.stage
    welded = mesh_stage.enter("mesh simplification", xyz, rgb, faces, MAX_COUNT, clock)
    dev, c = xyz.device, float(cell)
    info = dict(cells=0, cells_used=0, vertices_in=int(xyz.shape[0]), faces_in=int(faces.shape[0]), faces_collapsed=int(faces.shape[0]),
                faces_duplicate=0, faces_out=0, rank_hist=[0, 0, 0, 0], fallbacks=0)
    if welded is None:
        return mesh_stage.empty_mesh(dev) + (info,)
    xyz, f64, rgb = welded
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
        return mesh_stage.empty_mesh(dev) + (info,)
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
    clock.end()
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
    def resolve(meta):
        c = resolve_cell(cell, cell_voxels, meta)
        check_options(c, rank_eps)
        return c

    def lattice_origin(c, meta, xyz_h):
        if len(xyz_h):
            return default_lattice_origin(c, meta.get("origin") if meta else None, xyz_h.min(0))
        return default_lattice_origin(c, meta.get("origin") if meta else np.zeros(3), None)

    out = out or default_out(mesh_path)
    res, info, c = mesh_stage.run_file("simplify", "simplification", mesh_path, out, origin, device, resolve, lattice_origin,
                                       lambda c, xyz, rgb, f, o, timing: simplify(xyz, rgb, f, c, o, rank_eps),
                                       lambda meta, info, c, o, src, out, s, ds, stages: summary(meta, info, c, o, src, out, s, ds))
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


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    if args.cell is not None and args.cell_voxels is not None:
        raise SystemExit("simplify: give --cell or --cell_voxels, not both")
    return from_file(mesh_path_of(args), args.out, args.cell, args.cell_voxels, args.origin, args.rank_eps)


if __name__ == "__main__":
    main()
