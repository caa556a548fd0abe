"""Accuracy and completeness of a cloud or a mesh against a truth, on the GPU: the DTU and Tanks-and-Temples measures.

    python accuracy_whu.py --recon <cloud or mesh PLY> --truth <cloud or mesh PLY> --max_dist D [--tau T [T ...]]
                           [--spacing S | --spacing_voxels K] [--voxel_down V] [--out PREFIX]

Accuracy is the distance from every point of the reconstruction to the nearest point of the truth, completeness the distance from
every point of the truth to the nearest point of the reconstruction; precision and recall at a threshold tau are the shares of
those distances <= tau, and F = 2 P R / (P + R).  Both directions are one bounded nearest-neighbour search (include/adamvs_hip.h
"Cloud distance" states every operation, csrc/cloud_dist.hip holds the kernels): distances beyond --max_dist D are not looked
for.  The mean and the RMSE count them as D (the DTU convention); the other figures are over the points within D.  Both inputs
are taken to share a frame, as every product of this pipeline does: nothing is registered here.  A truth georeferenced on its
own is aligned first by register_whu.py (ada_mvs_amd/register.py: point-to-plane ICP), whose `<out>.ply` is scored here.

Each input is a point PLY (fuse_whu.py's layout) or a mesh PLY (mesh_whu.py's); a mesh is scored through points sampled on its
faces at --spacing (default D / 4; or --spacing_voxels times the voxel of `<mesh>.json`): every point of the surface lies within
spacing / sqrt(3) of a sample, so a distance to the samples exceeds the distance to the surface by at most that.  --voxel_down V
keeps one point per cubic cell of side V of either input first (the Tanks-and-Temples down-sampling: the member with the lowest
index).

Written: `<out>.json` (every figure, the counts, the options, the pair evaluations, the timings) and two clouds,
`<out>_accuracy.ply` (the reconstruction coloured by its distance to the truth) and `<out>_completeness.ply` (the truth coloured
by its distance to the reconstruction).  The colour RAMP over t = dist / D in [0, 1] is piecewise linear, channels rounded to
the nearest integer: blue (0, 0, 255) at t = 0, green (0, 255, 0) at t = 1/2, red (255, 0, 0) at t = 1; a point with nothing
within D is magenta (255, 0, 255), a colour the ramp never takes.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

from .cloud_lattice import MAX_COUNT

KEY_BITS = 21
BEYOND_RGB = (255, 0, 255)
QUANTILES = (("median_within", 0.5), ("p90_within", 0.9))


def check_options(D, thresholds=(), spacing=None, voxel=None):
    if not (isinstance(D, (int, float)) and math.isfinite(float(D)) and float(D) > 0):
        raise ValueError("max_dist=%r must be finite and > 0" % (D,))
    for t in thresholds:
        if not (math.isfinite(float(t)) and 0 < float(t) <= float(D)):
            raise ValueError("tau=%r: 0 < tau <= max_dist = %g (distances beyond max_dist are not measured)" % (t, D))
    for name, v in (("spacing", spacing), ("voxel_down", voxel)):
        if v is not None and not (math.isfinite(float(v)) and float(v) > 0):
            raise ValueError("%s=%r must be finite and > 0" % (name, v))


def default_thresholds(D):
    return [float(D) / 4.0, float(D) / 2.0, float(D)]


def default_lattice_origin(cell, target_min):
    """cloud_lattice.default_origin, under the name tests and tools call."""
    from . import cloud_lattice
    return cloud_lattice.default_origin(cell, target_min)


def resolve_spacing(spacing, spacing_voxels, D, meta):
    """--spacing S, or --spacing_voxels K times the voxel of <mesh>.json, or D / 4."""
    if spacing is not None and spacing_voxels is not None:
        raise ValueError("give --spacing or --spacing_voxels, not both")
    if spacing is not None:
        check_options(D, spacing=spacing)
        return float(spacing)
    if spacing_voxels is None:
        return float(D) / 4.0
    k = float(spacing_voxels)
    if not (math.isfinite(k) and k > 0):
        raise ValueError("spacing_voxels=%r must be finite and > 0" % (spacing_voxels,))
    if meta is None or "voxel" not in meta:
        raise ValueError("<mesh>.json with the voxel size is absent: give --spacing")
    return k * float(meta["voxel"])


def ramp(dist, D):
    """dist [n] (numpy; inf or anything > D: nothing within D) -> rgb [n, 3] uint8 by the RAMP of the module docstring."""
    d = np.asarray(dist, np.float64).reshape(-1)
    within = d <= float(D)
    t = np.where(within, d, 0.0) / float(D)
    lo = t <= 0.5
    r = np.where(lo, 0.0, 2.0 * t - 1.0)
    g = np.where(lo, 2.0 * t, 2.0 - 2.0 * t)
    b = np.where(lo, 1.0 - 2.0 * t, 0.0)
    rgb = np.floor(np.stack([r, g, b], 1) * 255.0 + 0.5).astype(np.uint8)
    rgb[~within] = BEYOND_RGB
    return rgb


def nearest(targets, queries, D, detail=None, timing=None, origin=None):
    """targets [nt, 3], queries [nq, 3] float64 device tensors -> (dist [nq] float32: the distance to the nearest target, +inf where
    none lies within D; index [nq] int32: that target's number, or -1; info: targets, queries, cells, items, within, pairs).
    origin: the lattice origin (default: default_lattice_origin).  detail: a dict that receives d2 and the intermediates (device
    tensors); timing: a list that receives (name, start event, end event) of the stages keys, sorts, items, nearest."""
    import torch
    from . import cloud_lattice, hip_ops, mesh_stage
    check_options(D)
    targets, queries = cloud_lattice.cloud(targets, "targets"), cloud_lattice.cloud(queries, "queries")
    dev, c = queries.device, float(D)
    nt, nq = int(targets.shape[0]), int(queries.shape[0])
    info = dict(targets=nt, queries=nq, cells=0, items=0, within=0, pairs=0)
    dist = torch.full((nq,), float("inf"), device=dev, dtype=torch.float32)
    index = torch.full((nq,), -1, device=dev, dtype=torch.int32)
    if nt == 0 or nq == 0:
        return dist, index, info
    clock = mesh_stage.StageClock(timing)
    clock.stage("keys")
    o = cloud_lattice.origin_of(origin, c, targets, "target")
    tkeys = cloud_lattice.keyed(targets, c, o, "nearest", "targets")
    qkeys, _ = hip_ops.simplify_keys(queries, c, o)
    clock.stage("sorts")
    cells = cloud_lattice.Cells(targets, tkeys)
    ukeys, tstart, tindex = cells.ukeys, cells.tstart, cells.index
    qs = torch.sort(qkeys, stable=True)
    clock.stage("items")
    outside, qorder, items = cloud_lattice.work_items(qs.values, qs.indices)
    info.update(cells=int(ukeys.numel()), outside=outside)
    if items is None:
        return dist, index, info
    item_key, item_first, item_count = items
    clock.stage("nearest")
    d2, index, pairs = hip_ops.cloud_nearest(o, c, ukeys, tstart, cells.sorted, tindex, queries, qorder, item_key, item_first, item_count)
    dist = torch.sqrt(d2)
    clock.end()
    info.update(items=int(item_key.numel()), within=int((index >= 0).sum()), pairs=int(pairs.sum()))
    if detail is not None:
        detail.update(d2=d2, lattice_origin=o, tkeys=tkeys, qkeys=qkeys, ukeys=ukeys, tstart=tstart, tindex=tindex, qorder=qorder,
                      item_key=item_key, item_first=item_first, item_count=item_count, pairs=pairs)
    return dist, index, info


def sample_mesh(xyz, faces, spacing):
    """xyz [nv, 3] float64, faces [nf, 3] int32 (uint32) or int64: device tensors -> points [m, 3] float64 on the faces, every point
    of the surface within spacing / sqrt(3) of one (include/adamvs_hip.h "Cloud distance", surface sampler)."""
    import torch
    from . import _lib, cloud_lattice, hip_ops
    check_options(1.0, spacing=spacing)
    xyz = cloud_lattice.cloud(xyz, "xyz")
    if not isinstance(faces, torch.Tensor) or not faces.is_cuda:
        raise _lib.AdaMVSHipError("faces must be a GPU tensor: the surface sampler has no CPU fallback")
    if faces.dtype not in (torch.int32, torch.int64) or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.AdaMVSHipError("faces: [nf, 3] int32 / int64, got %s %s" % (tuple(faces.shape), faces.dtype))
    nv, nf = int(xyz.shape[0]), int(faces.shape[0])
    if nf == 0:
        return torch.empty(0, 3, device=xyz.device, dtype=torch.float64)
    f64 = faces.to(torch.int64) & 0xFFFFFFFF
    if nv == 0 or int(f64.max()) >= nv:
        raise _lib.AdaMVSHipError("a face refers to vertex %d of %d" % (int(f64.max()), nv))
    f32 = f64.to(torch.int32).contiguous()
    subdiv = hip_ops.cloud_sample_count(xyz, f32, spacing)
    if int(subdiv.max()) > _lib.CLOUD_MAX_SUBDIV:
        f = int(torch.nonzero(subdiv > _lib.CLOUD_MAX_SUBDIV)[0])
        raise _lib.AdaMVSHipError("sample_mesh: face %d needs more than %d subdivisions at spacing %g (or is not finite)"
                                  % (f, _lib.CLOUD_MAX_SUBDIV, float(spacing)))
    n = subdiv.to(torch.int64)
    offsets = torch.zeros(nf + 1, device=xyz.device, dtype=torch.int64)
    offsets[1:] = torch.cumsum((n + 1) * (n + 2) // 2, 0)
    total = int(offsets[-1])
    if total > MAX_COUNT:
        raise _lib.AdaMVSHipError("sample_mesh: %d samples at spacing %g (at most 2^31 - 1)" % (total, float(spacing)))
    return hip_ops.cloud_sample_emit(xyz, f32, subdiv, offsets, total)


def voxel_first(points, voxel):
    """points [n, 3] float64 (any device) -> the indices [m] int64, ascending, of one point per cubic cell of side `voxel` (cells
    counted from the per-axis minimum): the member with the lowest index.  Integers only, so the choice is deterministic."""
    import torch
    check_options(1.0, voxel=voxel)
    n = int(points.shape[0])
    if n == 0:
        return torch.empty(0, device=points.device, dtype=torch.int64)
    p = points.to(torch.float64)
    if not bool(torch.isfinite(p).all()):
        raise ValueError("voxel_first: a point is not finite")
    cell = torch.floor((p - p.min(0).values) / float(voxel)).to(torch.int64)
    if int(cell.max()) >= 1 << KEY_BITS:
        raise ValueError("voxel_first: more than 2^21 cells of %g along an axis" % float(voxel))
    key = cell[:, 0] | (cell[:, 1] << KEY_BITS) | (cell[:, 2] << (2 * KEY_BITS))
    uniq, inverse = torch.unique(key, return_inverse=True)
    first = torch.full((uniq.numel(),), n, device=points.device, dtype=torch.int64)
    first = first.scatter_reduce(0, inverse, torch.arange(n, device=points.device), reduce="amin")
    return torch.sort(first).values


def _quantile(sorted_values, q):
    """Linear interpolation between the closest ranks (numpy's default), on an ascending fp64 tensor."""
    m = int(sorted_values.numel())
    pos = q * (m - 1)
    lo = int(math.floor(pos))
    hi = min(lo + 1, m - 1)
    a, b = float(sorted_values[lo]), float(sorted_values[hi])
    return a + (b - a) * (pos - lo)


def summarise(dist, D, thresholds=None):
    """dist [n] (torch, any device; inf or > D: nothing within D) -> dict: n, within (count), mean_trunc and rmse_trunc (distances
    beyond D counted as D), mean_within, median_within, p90_within (None without a point within D) and share: [{tau, share}] of the
    points <= tau, of all n, for every tau <= D.  fp64 throughout."""
    import torch
    thresholds = default_thresholds(D) if thresholds is None else [float(t) for t in thresholds]
    check_options(D, thresholds)
    d = dist.reshape(-1).to(torch.float64)
    n = int(d.numel())
    inside = d <= float(D)
    w = int(inside.sum())
    res = dict(n=n, within=w, mean_trunc=None, rmse_trunc=None, mean_within=None, median_within=None, p90_within=None, share=[])
    if n:
        tr = torch.where(inside, d, torch.full_like(d, float(D)))
        res.update(mean_trunc=float(tr.mean()), rmse_trunc=float(torch.sqrt((tr * tr).mean())))
    if w:
        s = torch.sort(d[inside]).values
        res.update(mean_within=float(s.mean()), **{name: _quantile(s, q) for name, q in QUANTILES})
    for t in thresholds:
        res["share"].append(dict(tau=t, share=(int((d <= t).sum()) / n) if n else 0.0))
    return res


def fscore(precision, recall):
    return 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0


def combine(accuracy, completeness):
    """The two summaries -> [{tau, precision, recall, fscore}]."""
    return [dict(tau=a["tau"], precision=a["share"], recall=c["share"], fscore=fscore(a["share"], c["share"]))
            for a, c in zip(accuracy["share"], completeness["share"])]


def compare(recon, truth, D, thresholds=None, detail=None, timing=None):
    """recon [n, 3], truth [m, 3] float64 device tensors -> dict: accuracy (summarise of the distances recon -> truth), completeness
    (truth -> recon), scores [{tau, precision, recall, fscore}], pairs (pair evaluations of both searches).  detail receives
    accuracy_dist and completeness_dist (device, float32)."""
    from . import mesh_stage
    thresholds = default_thresholds(D) if thresholds is None else [float(t) for t in thresholds]
    check_options(D, thresholds)
    t_acc, t_com = [], []
    acc_d, _, acc_i = nearest(truth, recon, D, timing=t_acc if timing is not None else None)
    com_d, _, com_i = nearest(recon, truth, D, timing=t_com if timing is not None else None)
    clock = mesh_stage.StageClock(timing)
    clock.stage("statistics")
    acc, com = summarise(acc_d, D, thresholds), summarise(com_d, D, thresholds)
    if timing is not None:
        timing.extend(("accuracy_" + n, a, b) for n, a, b in t_acc)
        timing.extend(("completeness_" + n, a, b) for n, a, b in t_com)
    clock.end()
    if detail is not None:
        detail.update(accuracy_dist=acc_d, completeness_dist=com_d)
    return dict(max_dist=float(D), accuracy=acc, completeness=com, scores=combine(acc, com), pairs=acc_i["pairs"] + com_i["pairs"],
                accuracy_search=acc_i, completeness_search=com_i)


def is_mesh_ply(path):
    """Whether the PLY's header declares faces (mesh_whu.py's layout) or vertices only (fuse_whu.py's)."""
    with open(path, "rb") as f:
        head = f.read(4096)
    end = head.find(b"end_header\n")
    if not head.startswith(b"ply\n") or end < 0:
        raise ValueError("%s: not a PLY file with a header under 4 KB" % path)
    return any(ln.startswith("element face") for ln in head[:end].decode("ascii").splitlines())


def load_points(path, D, spacing, spacing_voxels, device, chunk=1 << 23):
    """A point PLY, or a mesh PLY through its samples -> (points [n, 3] float64 on the device, description dict)."""
    import torch
    from . import dsm, mesh
    if is_mesh_ply(path):
        meta = None
        if os.path.exists(path + ".json"):
            with open(path + ".json") as f:
                meta = json.load(f)
        s = resolve_spacing(spacing, spacing_voxels, D, meta)
        verts, faces = mesh.read_mesh_ply(path)
        xyz = torch.from_numpy(np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float64)).to(device)
        pts = sample_mesh(xyz, torch.from_numpy(faces.astype(np.int64)).to(device), s)
        return pts, dict(path=path, kind="mesh", vertices=int(len(verts)), faces=int(len(faces)), spacing=s, points=int(pts.shape[0]))
    parts = [torch.from_numpy(xyz).to(device) for xyz, _ in dsm.ply_chunks(path, chunk)]
    pts = torch.cat(parts) if parts else torch.empty(0, 3, device=device, dtype=torch.float64)
    return pts, dict(path=path, kind="points", points=int(pts.shape[0]))


def output_paths(out):
    return out + ".json", out + "_accuracy.ply", out + "_completeness.ply"


def from_files(recon, truth, max_dist, tau=None, spacing=None, spacing_voxels=None, voxel_down=None, out=None, device=None, log=print):
    """Score the PLY `recon` against the PLY `truth` -> the dict also written to <out>.json."""
    import torch
    from . import fusion
    t_start = time.time()
    thresholds = default_thresholds(max_dist) if not tau else [float(t) for t in tau]
    check_options(max_dist, thresholds, spacing, voxel_down)
    if spacing is not None and spacing_voxels is not None:
        raise ValueError("give --spacing or --spacing_voxels, not both")
    if not torch.cuda.is_available():
        raise RuntimeError("accuracy: needs an MI355X (there is no CPU fallback for the cloud distance kernels)")
    device = torch.device(device if device is not None else "cuda")
    out = out or (recon[:-4] if recon.lower().endswith(".ply") else recon) + "_scored"
    clouds, inputs = {}, {}
    for name, path in (("recon", recon), ("truth", truth)):
        pts, desc = load_points(path, max_dist, spacing, spacing_voxels, device)
        if voxel_down is not None:
            pts = pts[voxel_first(pts, voxel_down)].contiguous()
            desc.update(voxel_down=float(voxel_down), points_kept=int(pts.shape[0]))
        clouds[name], inputs[name] = pts, desc
    timing, detail = [], {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = compare(clouds["recon"], clouds["truth"], max_dist, thresholds, detail=detail, timing=timing)
    e1.record()
    torch.cuda.synchronize(device)
    json_path, acc_ply, com_ply = output_paths(out)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    for path, pts, d in ((acc_ply, clouds["recon"], detail["accuracy_dist"]), (com_ply, clouds["truth"], detail["completeness_dist"])):
        with fusion.PlyWriter(path) as w:
            w.write(pts.cpu().numpy(), ramp(d.cpu().numpy(), max_dist))
    res.update(inputs=inputs, thresholds=thresholds, options=dict(max_dist=float(max_dist), spacing=spacing, spacing_voxels=spacing_voxels,
                                                                  voxel_down=voxel_down),
               accuracy_ply=acc_ply, completeness_ply=com_ply, stage_ms={n: a.elapsed_time(b) for n, a, b in timing},
               device_seconds=e0.elapsed_time(e1) / 1e3, seconds=time.time() - t_start)
    with open(json_path, "w") as fj:
        json.dump(res, fj, indent=1)
        fj.write("\n")
    best = res["scores"][-1]
    log("accuracy: %d points against %d: accuracy mean %.4g m, completeness mean %.4g m (truncated at %g m); at tau = %g m precision %.4f, "
        "recall %.4f, F %.4f; %d pair evaluations, device %.3f s, total_time = %.3f s, into %s"
        % (res["accuracy"]["n"], res["completeness"]["n"], res["accuracy"]["mean_trunc"] or 0.0, res["completeness"]["mean_trunc"] or 0.0,
           max_dist, best["tau"], best["precision"], best["recall"], best["fscore"], res["pairs"], res["device_seconds"], res["seconds"],
           json_path))
    return res


def build_parser():
    ap = argparse.ArgumentParser(description="Accuracy, completeness and F-score of a cloud or mesh against a truth")
    ap.add_argument("--recon", required=True, help="the reconstruction: a point PLY (fuse_whu.py) or a mesh PLY (mesh_whu.py)")
    ap.add_argument("--truth", required=True, help="the truth: a point PLY or a mesh PLY, in the same frame")
    ap.add_argument("--max_dist", type=float, required=True, metavar="D", help="truncation distance in metres: nothing farther is looked for")
    ap.add_argument("--tau", type=float, nargs="+", default=None, metavar="T", help="thresholds of precision / recall / F (default D/4 D/2 D)")
    ap.add_argument("--spacing", type=float, default=None, metavar="S", help="sample spacing on a mesh in metres (default D / 4)")
    ap.add_argument("--spacing_voxels", type=float, default=None, metavar="K", help="sample spacing in voxels of <mesh>.json")
    ap.add_argument("--voxel_down", type=float, default=None, metavar="V", help="keep one point per cubic cell of side V of both inputs first")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="prefix of <out>.json and the two coloured PLYs (default <recon minus .ply>_scored)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    if args.spacing is not None and args.spacing_voxels is not None:
        raise SystemExit("accuracy: give --spacing or --spacing_voxels, not both")
    return from_files(args.recon, args.truth, args.max_dist, args.tau, args.spacing, args.spacing_voxels, args.voxel_down, args.out)


if __name__ == "__main__":
    main()
