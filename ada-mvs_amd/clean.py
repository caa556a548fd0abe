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
import json
import math
import os
import sys
import time

import numpy as np

from .simplify import CARRIED, MAX_COUNT, mesh_path_of  # noqa: F401  (the same carried keys and path rule)

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
    if min_area is not None and (isinstance(min_area, bool) or not isinstance(min_area, (int, float)) or not math.isfinite(float(min_area))
                                 or float(min_area) <= 0):
        raise ValueError("min_area=%r must be finite and > 0" % (min_area,))
    if isinstance(max_hole_edges, bool) or not isinstance(max_hole_edges, (int, np.integer)) or not 0 <= int(max_hole_edges) <= MAX_HOLE_EDGES:
        raise ValueError("max_hole_edges=%r must be an integer in 0 .. %d" % (max_hole_edges, MAX_HOLE_EDGES))


def default_out(mesh_path):
    return (mesh_path[:-4] if mesh_path.lower().endswith(".ply") else mesh_path) + "_cleaned.ply"


def resolve_min_area(min_area, min_area_voxels, meta):
    """--min_area A (square metres), or --min_area_voxels K times the squared voxel of <mesh>.json, or neither: no area threshold."""
    if min_area is not None and min_area_voxels is not None:
        raise ValueError("give --min_area or --min_area_voxels, not both")
    if min_area is not None:
        check_options(min_area=min_area)
        return float(min_area)
    if min_area_voxels is None:
        return None
    k = min_area_voxels
    if isinstance(k, bool) or not isinstance(k, (int, float)) or not math.isfinite(float(k)) or float(k) <= 0:
        raise ValueError("min_area_voxels=%r must be finite and > 0" % (k,))
    if meta is None or "voxel" not in meta:
        raise ValueError("<mesh>.json with the voxel size is absent: give --min_area")
    return float(k) * float(meta["voxel"]) * float(meta["voxel"])


def summary(meta, info, options, origin, source, out, seconds, device_seconds, stage_seconds=None):
    """The dict written to <out>.json: the carried keys of <mesh>.json first, unchanged."""
    res = {k: meta[k] for k in CARRIED if meta is not None and k in meta}
    res.update(options)
    res.update(clean_origin=[float(v) for v in origin], source=source, ply=out)
    res.update(info)
    res.update(seconds=float(seconds), device_seconds=float(device_seconds), stage_seconds=dict(stage_seconds or {}))
    return res


def doubling_rounds(n):
    """Rounds after which a label is the minimum over at least 2 n half-edges: every cycle among n half-edges is labelled whole."""
    return 0 if n < 1 else int(math.ceil(math.log2(n))) + 1 if n > 1 else 1


def _empty(dev):
    import torch
    return (torch.empty(0, 3, device=dev, dtype=torch.float64), torch.empty(0, 3, device=dev, dtype=torch.uint8),
            torch.empty(0, 3, device=dev, dtype=torch.int32))


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
    from . import _lib, hip_ops, mesh
    check_options(min_faces, min_area, max_hole_edges)
    for name, t in (("xyz", xyz), ("rgb", rgb), ("faces", faces)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.AdaMVSHipError("%s must be a GPU tensor: mesh cleaning has no CPU fallback" % name)
    if xyz.dtype != torch.float64 or rgb.dtype != torch.uint8 or faces.dtype not in (torch.int32, torch.int64):
        raise _lib.AdaMVSHipError("xyz float64, rgb uint8, faces int32 / int64: got %s, %s, %s" % (xyz.dtype, rgb.dtype, faces.dtype))
    if xyz.dim() != 2 or xyz.shape[1] != 3 or tuple(rgb.shape) != tuple(xyz.shape) or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.AdaMVSHipError("xyz [nv, 3], rgb [nv, 3], faces [nf, 3]: got %s, %s, %s" % (tuple(xyz.shape), tuple(rgb.shape), tuple(faces.shape)))
    dev = xyz.device
    min_faces, M = int(min_faces), int(max_hole_edges)
    marks = []

    def stage(name):
        if timing is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

    def done(out):
        stage("end")
        if timing is not None:
            timing.extend((a[0], a[1], b[1]) for a, b in zip(marks[:-1], marks[1:]))
        info.update(vertices=int(out[0].shape[0]), faces=int(out[2].shape[0]))
        return out + (info,)

    info = dict.fromkeys(COUNTS, 0)
    info.update(area_removed=0.0, faces_in=int(faces.shape[0]))
    if xyz.shape[0] == 0:
        if faces.shape[0]:
            raise _lib.AdaMVSHipError("%d faces without vertices" % faces.shape[0])
        return done(_empty(dev))
    if faces.shape[0] > MAX_FACES or xyz.shape[0] > MAX_COUNT:
        raise _lib.AdaMVSHipError("more than 2^31 - 1 vertices or (2^31 - 1) / 3 faces")
    f64 = faces.to(torch.int64) & 0xFFFFFFFF
    if faces.shape[0] and int(f64.max()) >= xyz.shape[0]:
        raise _lib.AdaMVSHipError("a face refers to vertex %d of %d" % (int(f64.max()), xyz.shape[0]))
    stage("weld")
    xyz, f64, rgb = mesh.weld(xyz.contiguous(), f64, rgb.contiguous())
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
        return done(_empty(dev))
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
        return done(_empty(dev))
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
    import torch
    from . import mesh
    t_start = time.time()
    meta = None
    if os.path.exists(mesh_path + ".json"):
        with open(mesh_path + ".json") as f:
            meta = json.load(f)
    area = resolve_min_area(min_area, min_area_voxels, meta)
    check_options(min_faces, area, max_hole_edges)
    if not torch.cuda.is_available():
        raise RuntimeError("clean: needs an MI355X (there is no CPU fallback for the cleaning kernels)")
    out = out or default_out(mesh_path)
    device = torch.device(device if device is not None else "cuda")
    verts, faces = mesh.read_mesh_ply(mesh_path)
    xyz_h = np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float64)
    rgb_h = np.stack([verts["red"], verts["green"], verts["blue"]], 1)
    if origin is not None:
        o = np.asarray(origin, np.float64).reshape(3)
    elif meta is not None and "origin" in meta:
        o = np.asarray(meta["origin"], np.float64).reshape(3)
    else:
        o = xyz_h.min(0) if len(xyz_h) else np.zeros(3)
    xyz = torch.from_numpy(np.ascontiguousarray(xyz_h)).to(device)
    rgb = torch.from_numpy(np.ascontiguousarray(rgb_h)).to(device)
    f = torch.from_numpy(faces.astype(np.int64)).to(device)
    timing = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    cx, cc, cf, info = clean(xyz, rgb, f, min_faces, area, max_hole_edges, o, timing=timing)
    e1.record()
    torch.cuda.synchronize(device)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with mesh.MeshPlyWriter(out) as w:
        w.write(cx.cpu().numpy(), cc.cpu().numpy(), cf.cpu().numpy().view(np.uint32))
    options = dict(min_faces=int(min_faces), min_area=area, max_hole_edges=int(max_hole_edges))
    res = summary(meta, info, options, o, mesh_path, out, time.time() - t_start, e0.elapsed_time(e1) / 1e3,
                  {name: a.elapsed_time(b) / 1e3 for name, a, b in timing})
    with open(out + ".json", "w") as fj:
        json.dump(res, fj, indent=1)
        fj.write("\n")
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
