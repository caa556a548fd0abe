"""Mesh cleaning: small components of the TSDF mesh dropped and its small holes closed, on the GPU.

    python clean_whu.py --output_folder <predict output> [--mesh <output_folder>/mesh.ply] [--min_faces 100]
                        [--min_area A | --min_area_voxels K] [--max_hole_edges 32] [--origin X Y Z]
                        [--out <mesh minus .ply>_cleaned.ply]

The step after mesh_whu.py and before smooth_whu.py.  The zero level set of a TSDF built from predicted depth has two defects
that every later mesh step otherwise takes as it comes: floaters (small blobs where a few consistent but wrong depths passed
fuse_whu.py) and pinholes (small loops of open edges where a few voxels missed --min_weight; smooth_whu.py pins their rims,
texture_whu.py starts a chart boundary there, accuracy_whu.py samples nothing there).  Here the connected components (faces
that share a vertex) with fewer than --min_faces faces, or less than --min_area of surface, are dropped, and every loop of
open edges of at most --max_hole_edges edges whose rim is an ordinary closed curve is closed by a fan around the mean of its
rim.  Nothing moves: a surviving vertex keeps the bits of its position and its colour.  include/adamvs_hip.h "Mesh cleaning"
states every operation, csrc/mesh_clean.hip holds the kernels; the sorts, scans and compactions are torch's.

The defaults 100 and 32 are conventions: nobody has measured them on a real scene.  --min_faces 0 keeps every component,
--max_hole_edges 0 closes nothing; with both (and no area threshold) the output is the welded input without its degenerate
faces and unused vertices.

The mesh is welded by exact position first (mesh.weld), always, so the result does not depend on mesh_whu.py's --brick or
--weld; two runs are bit-identical; cleaning a cleaned mesh with the same options returns the same bytes.  `<out>.json`
carries the input JSON's voxel, mu, origin and views unchanged (smooth_whu.py --sigma_s_voxels, simplify_whu.py --cell_voxels
and texture_whu.py's default occlusion tolerance keep working on the cleaned mesh) and adds the options, the source, the
counts and the timings.
"""
import argparse
import math
import sys

import numpy as np

from . import mesh_stage
from .mesh_stage import CARRIED, MAX_COUNT, mesh_path_of  # noqa: F401  (shared with simplify.py and smooth.py)

DEFAULT_MIN_FACES = 100                       # a convention, not a measurement
DEFAULT_MAX_HOLE_EDGES = 32                   # likewise
MAX_HOLE_EDGES = 4096
MAX_ROUNDS = 64
MAX_FACES = MAX_COUNT // 3
STAGES = ("weld", "faces", "components", "areas", "select", "boundary", "loops", "fill", "emit")
COUNTS = ("vertices_in", "faces_in", "faces_degenerate", "components", "components_kept", "component_rounds", "faces_removed",
          "area_removed", "largest_removed_faces", "boundary_edges_in", "loops", "loops_closed", "loops_too_long", "edges_left_open",
          "nonsimple_vertices", "fill_vertices", "fill_faces", "vertices", "faces")


def check_options(min_faces=DEFAULT_MIN_FACES, min_area=None, max_hole_edges=DEFAULT_MAX_HOLE_EDGES):
    if isinstance(min_faces, bool) or not isinstance(min_faces, (int, np.integer)) or not 0 <= int(min_faces) <= MAX_COUNT:
        raise ValueError("min_faces=%r must be an integer in 0 .. 2^31 - 1" % (min_faces,))
    if min_area is not None:
        mesh_stage.positive("min_area", min_area)
    if isinstance(max_hole_edges, bool) or not isinstance(max_hole_edges, (int, np.integer)) or not 0 <= int(max_hole_edges) <= MAX_HOLE_EDGES:
        raise ValueError("max_hole_edges=%r must be an integer in 0 .. %d" % (max_hole_edges, MAX_HOLE_EDGES))


def default_out(mesh_path):
    return mesh_stage.default_out(mesh_path, "_cleaned")


def resolve_min_area(min_area, min_area_voxels, meta):
    """--min_area A (square metres), or --min_area_voxels K times the squared voxel of <mesh>.json, or neither: no area threshold."""
    return mesh_stage.resolve_metres("min_area", min_area, min_area_voxels, None, meta, power=2)


def summary(meta, info, options, origin, source, out, seconds, device_seconds, stage_seconds=None):
    """The dict written to <out>.json: the carried keys of <mesh>.json first, unchanged."""
    return mesh_stage.summary(meta, dict(options, clean_origin=[float(v) for v in origin], source=source, ply=out), info,
                              seconds=float(seconds), device_seconds=float(device_seconds), stage_seconds=dict(stage_seconds or {}))


def doubling_rounds(n):
    """Rounds after which a label is the minimum over at least 2 n half-edges: every cycle among n half-edges is labelled whole."""
    return 0 if n < 1 else int(math.ceil(math.log2(n))) + 1 if n > 1 else 1


def _weld_output(xyz, rgb, faces):
    """The weld of the output: unique rows in lexicographic order; of coincident vertices the earliest gives the colour."""
    import torch
    u, inv = torch.unique(xyz, dim=0, return_inverse=True)
    inv = inv.reshape(-1)
    first = torch.full((u.shape[0],), xyz.shape[0], device=xyz.device, dtype=torch.int64)
    first.scatter_reduce_(0, inv, torch.arange(xyz.shape[0], device=xyz.device, dtype=torch.int64), "amin")
    return u, rgb[first], inv[faces.to(torch.int64)].to(torch.int32)


def clean(xyz, rgb, faces, min_faces=DEFAULT_MIN_FACES, min_area=None, max_hole_edges=DEFAULT_MAX_HOLE_EDGES, origin=None, detail=None,
          timing=None):
    """xyz [nv, 3] float64, rgb [nv, 3] uint8, faces [nf, 3] int32 (uint32) or int64: device tensors -> (xyz, rgb, faces int32, info)
    of the cleaned mesh; info: the keys of COUNTS.  min_area: square metres, or None.  origin: O (default: the per-axis vertex
    minimum).  detail: a dict that receives the intermediates (device tensors): the welded mesh, `labels` [vertices] and
    `face_labels`, `kept` [faces after the degenerate ones left], `surviving` [ns, 3], `boundary`, `successor`, `loop`, `closed`
    [3 ns]; timing: a list that receives (name, start event, end event) of the stages."""
    import torch
    from . import _lib, hip_ops
    check_options(min_faces, min_area, max_hole_edges)
    clock = mesh_stage.StageClock(timing)
    stage = clock.stage
    welded = mesh_stage.enter("mesh cleaning", xyz, rgb, faces, MAX_FACES, clock)
    dev = xyz.device
    min_faces, M = int(min_faces), int(max_hole_edges)

    def done(out):
        clock.end()
        info.update(vertices=int(out[0].shape[0]), faces=int(out[2].shape[0]))
        return out + (info,)

    info = dict.fromkeys(COUNTS, 0)
    info.update(area_removed=0.0, faces_in=int(faces.shape[0]))
    if welded is None:
        return done(mesh_stage.empty_mesh(dev))
    xyz, f64, rgb = welded
    nv = int(xyz.shape[0])
    info["vertices_in"] = nv
    o = np.asarray(origin, np.float64).reshape(3) if origin is not None else xyz.min(0).values.cpu().numpy()
    if not np.isfinite(o).all() or not bool(torch.isfinite(xyz).all()):
        raise _lib.AdaMVSHipError("clean: a vertex or the origin %r is not finite" % (o,))
    degenerate = (f64[:, 0] == f64[:, 1]) | (f64[:, 1] == f64[:, 2]) | (f64[:, 2] == f64[:, 0])
    f64 = f64[~degenerate]
    nf = int(f64.shape[0])
    info["faces_degenerate"] = info["faces_in"] - nf
    if detail is not None:
        detail.update(xyz=xyz, rgb=rgb, faces=f64.to(torch.int32), degenerate=degenerate, origin=o)
    if nf == 0:
        return done(mesh_stage.empty_mesh(dev))
    faces32 = f64.to(torch.int32).contiguous()
    p0 = (xyz - torch.from_numpy(o).to(dev)).contiguous()
    stage("faces")
    area = hip_ops.smooth_faces(p0, faces32)[:, 3].contiguous()
    # step 3: the labels, round by round until one changes nothing
    stage("components")
    parent, spare = torch.arange(nv, device=dev, dtype=torch.int32), torch.empty(nv, device=dev, dtype=torch.int32)
    changed = torch.zeros(1, device=dev, dtype=torch.int32)
    rounds = 0
    while True:
        if rounds == MAX_ROUNDS:
            raise RuntimeError("clean: the connected components did not converge in %d rounds" % MAX_ROUNDS)
        hip_ops.clean_components_round(faces32, parent, spare, changed)
        parent, spare = spare, parent
        rounds += 1
        if int(changed.item()) == 0:
            break
    stage("areas")
    face_label = parent[f64[:, 0]]
    by_label = torch.sort(face_label, stable=True)
    _, seg_of, count = torch.unique_consecutive(by_label.values, return_inverse=True, return_counts=True)
    seg_start = torch.cat([torch.zeros(1, device=dev, dtype=torch.int64), torch.cumsum(count, 0)])
    comp_area = hip_ops.clean_area(area, by_label.indices, seg_of, seg_start)
    stage("select")
    comp_kept = count >= min_faces
    if min_area is not None:
        comp_kept &= comp_area >= float(min_area)
    kept = torch.empty(nf, device=dev, dtype=torch.bool)
    kept[by_label.indices] = comp_kept[seg_of]
    count_h, area_h, kept_h = count.cpu().numpy(), comp_area.cpu().numpy(), comp_kept.cpu().numpy()
    info.update(components=int(len(count_h)), components_kept=int(kept_h.sum()), component_rounds=rounds,
                faces_removed=int(count_h[~kept_h].sum()), area_removed=float(np.sum(area_h[~kept_h])),
                largest_removed_faces=int(count_h[~kept_h].max()) if (~kept_h).any() else 0)
    sf = faces32[kept].contiguous()
    ns = int(sf.shape[0])
    if detail is not None:
        detail.update(labels=parent, face_labels=face_label, kept=kept, component_area=comp_area, component_faces=count, surviving=sf)
    if ns == 0:
        return done(mesh_stage.empty_mesh(dev))
    # steps 5 and 6
    stage("boundary")
    bnd = hip_ops.clean_boundary(sf)
    st = hip_ops.clean_successor(sf, nv, bnd)
    nb = int(bnd.sum())
    stage("loops")
    state = (st["lab"], st["nxt"], st["broken"])
    if nb:
        other = tuple(t.clone() for t in state)
        for _ in range(doubling_rounds(nb)):
            other = hip_ops.clean_double(bnd, state, other)
            state, other = other, state
    group, bad, loop, closed = hip_ops.clean_validate(bnd, st["succ"], state[0], state[2], M)
    leader = loop == torch.arange(3 * ns, device=dev, dtype=torch.int32)
    on = (st["out_count"] + st["in_count"]) > 0
    simple = (st["out_count"] == 1) & (st["in_count"] == 1)
    fill_edge = torch.nonzero(closed).reshape(-1)
    stats = torch.stack([leader.sum(), (leader & (closed != 0)).sum(), (leader & (group > M)).sum(), (on & ~simple).sum()]).cpu().tolist()
    nfill = int(fill_edge.shape[0])
    info.update(boundary_edges_in=nb, loops=int(stats[0]), loops_closed=int(stats[1]), loops_too_long=int(stats[2]),
                edges_left_open=nb - nfill, nonsimple_vertices=int(stats[3]), fill_vertices=int(stats[1]), fill_faces=nfill)
    # step 7
    stage("fill")
    centre = colour = loop_of = None
    if nfill:
        labs = loop[fill_edge]
        by_loop = torch.sort(labs, stable=True)
        members = fill_edge[by_loop.indices].to(torch.int32)
        loops, length = torch.unique_consecutive(by_loop.values, return_counts=True)
        start = torch.cat([torch.zeros(1, device=dev, dtype=torch.int64), torch.cumsum(length, 0)])
        loop_of = torch.searchsorted(loops, labs).to(torch.int32)
        centre, colour = hip_ops.clean_accumulate(p0, rgb, sf, members, start, o)
    # step 8
    stage("emit")
    used = torch.zeros(nv, device=dev, dtype=torch.bool)
    used[sf.reshape(-1).to(torch.int64)] = True
    rank = torch.cumsum(used, 0)
    new_index = torch.where(used, rank - 1, torch.full_like(rank, -1)).to(torch.int32)
    out = hip_ops.clean_emit(xyz, rgb, new_index, int(rank[-1]), sf, fill_edge.to(torch.int32) if nfill else None, loop_of, centre, colour)
    if nfill:
        out = _weld_output(*out)
    if detail is not None:
        detail.update(boundary=bnd, successor=st["succ"], out_count=st["out_count"], in_count=st["in_count"], lab=state[0], broken=state[2],
                      group=group, bad=bad, loop=loop, closed=closed, centre=centre, colour=colour, new_index=new_index, p0=p0, area=area)
    return done(out)


def from_file(mesh_path, out=None, min_faces=DEFAULT_MIN_FACES, min_area=None, min_area_voxels=None, max_hole_edges=DEFAULT_MAX_HOLE_EDGES,
              origin=None, device=None, log=print):
    """Clean the mesh PLY mesh_whu.py wrote -> the summary dict also written to <out>.json."""
    def resolve(meta):
        area = resolve_min_area(min_area, min_area_voxels, meta)
        check_options(min_faces, area, max_hole_edges)
        return dict(min_faces=int(min_faces), min_area=area, max_hole_edges=int(max_hole_edges))

    def run(opt, xyz, rgb, f, o, timing):
        return clean(xyz, rgb, f, min_faces, opt["min_area"], max_hole_edges, o, timing=timing)

    out = out or default_out(mesh_path)
    res, info, _ = mesh_stage.run_file("clean", "cleaning", mesh_path, out, origin, device, resolve, mesh_stage.volume_origin, run, summary)
    log("clean: %d vertices, %d faces in; %d of %d components kept (%d faces removed), %d of %d loops closed (%d too long, %d edges left "
        "open) -> %d vertices, %d faces into %s, device %.3f s, total_time = %.3f s"
        % (info["vertices_in"], info["faces_in"], info["components_kept"], info["components"], info["faces_removed"], info["loops_closed"],
           info["loops"], info["loops_too_long"], info["edges_left_open"], info["vertices"], info["faces"], out, res["device_seconds"],
           res["seconds"]))
    return res


def build_parser():
    ap = argparse.ArgumentParser(description="Clean the TSDF mesh: drop small components, close small holes")
    ap.add_argument("--mesh", default=None, help="mesh PLY of mesh_whu.py (default <output_folder>/mesh.ply)")
    ap.add_argument("--output_folder", default=None, help="predict_whu.py's output folder, after mesh_whu.py")
    ap.add_argument("--min_faces", type=int, default=DEFAULT_MIN_FACES,
                    help="drop the components of fewer faces (default %d, a convention; 0 keeps every component)" % DEFAULT_MIN_FACES)
    ap.add_argument("--min_area", type=float, default=None, metavar="A", help="also drop the components of less surface, square metres (default off)")
    ap.add_argument("--min_area_voxels", type=float, default=None, metavar="K",
                    help="the area threshold as K squared voxels of <mesh>.json (needs <mesh>.json)")
    ap.add_argument("--max_hole_edges", type=int, default=DEFAULT_MAX_HOLE_EDGES,
                    help="close the loops of open edges of at most this many edges (default %d, a convention; 0 closes nothing; at most %d)"
                    % (DEFAULT_MAX_HOLE_EDGES, MAX_HOLE_EDGES))
    ap.add_argument("--origin", type=float, nargs=3, metavar=("X", "Y", "Z"), default=None,
                    help="origin the arithmetic is relative to (default: the volume origin of <mesh>.json, else the vertex minimum)")
    ap.add_argument("--out", default=None, help="PLY to write (default <mesh minus .ply>_cleaned.ply); the summary goes to <out>.json")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    if args.min_area is not None and args.min_area_voxels is not None:
        raise SystemExit("clean: give --min_area or --min_area_voxels, not both")
    return from_file(mesh_path_of(args), args.out, args.min_faces, args.min_area, args.min_area_voxels, args.max_hole_edges, args.origin)


if __name__ == "__main__":
    main()
