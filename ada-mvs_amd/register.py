"""Align a reconstruction to the truth before it is scored: point-to-plane ICP on the GPU.

    python register_whu.py --recon <cloud or mesh PLY> --truth <cloud or mesh PLY> --max_dist D [--init FILE] [--max_iter 50] [--tol M]
                           [--huber M] [--normal_radius M] [--k 16] [--min_eig_ratio 1e-6] [--voxel_down V]
                           [--spacing S | --spacing_voxels K] [--out PREFIX]

A reconstruction and an independently georeferenced truth never share a frame exactly: a residual shift of a few decimetres or
a tilt of a fraction of a degree lands in every figure accuracy_whu.py prints.  DTU and Tanks and Temples register by ICP before
they score; this stage does the same (include/adamvs_hip.h "Cloud registration" states every operation, csrc/cloud_register.hip
holds the kernels).  The SOURCE (the reconstruction) is moved onto the TARGET (the truth) by y = R (x - c) + c + t about the
pivot c, the centre of the truth's bounding box.

Once: the truth's normals (cloud_filter.normals within --normal_radius, default D, from --k neighbours; a target without a
valid normal pairs with nothing) and the truth keyed and sorted on the lattice of cell D as accuracy.nearest does.  Per
iteration: the source is moved (rigid_apply), keyed, sorted and cut into work items, every moved point finds its nearest target
within D (cloud_nearest), the 32 sums of the normal equations are accumulated and reduced on the device, and the 6 x 6 system
is solved on the host in numpy fp64 through its eigenpairs: those with lambda_i > --min_eig_ratio lambda_max are kept, so a
flat scene (three constrained freedoms) leaves the others where --init put them instead of drifting on noise.  The 32 doubles
are all the host reads of an iteration's arithmetic (the sorts' dynamic shapes synchronise as they do in accuracy.nearest).
--huber M weights a pair by min(1, M / |r|).  The loop stops once no source point moved by more than --tol (default 1e-3 D: a
convention, like --min_eig_ratio 1e-6 and --k 16, not a measurement) or after --max_iter iterations; fewer than six pairs is an
error ("lost").  A start farther than D from the truth needs --init (a 4 x 4 matrix as `<out>.txt` holds it).

Each input is a point PLY or a mesh PLY; a mesh is estimated through points sampled on its faces (--spacing, --spacing_voxels:
as accuracy_whu.py).  --voxel_down V thins the source used for the ESTIMATE (accuracy.voxel_first); what is written is whole.

Written: `<out>.json` (R, t, pivot, the 4 x 4 matrix about the origin, iterations, converged, constrained_dof, the history,
fitness and rms before and after, the inputs, options and timings), `<out>.txt` (the matrix, %.17g) and `<out>.ply`: the whole
reconstruction moved, in the layout it came in (a point PLY with its colours; of a mesh PLY the vertices move, the faces and
colours stay byte for byte).  accuracy_whu.py --recon <out>.ply scores it.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

DEFAULT_MAX_ITER = 50
DEFAULT_K = 16
DEFAULT_MIN_EIG_RATIO = 1e-6
DEFAULT_TOL_RATIO = 1e-3
MIN_PAIRS = 6
MIN_K = 3                          # a normal needs three neighbours
STAGES = ("move", "keys", "sort", "items", "nearest", "accumulate", "reduce")


def check_options(D, max_iter=DEFAULT_MAX_ITER, tol=None, huber=None, normal_radius=None, k=DEFAULT_K, min_eig_ratio=DEFAULT_MIN_EIG_RATIO):
    from . import _lib, accuracy
    accuracy.check_options(D)
    if not (isinstance(max_iter, int) and not isinstance(max_iter, bool) and max_iter >= 0):
        raise ValueError("max_iter=%r: an integer >= 0" % (max_iter,))
    if tol is not None and not (math.isfinite(float(tol)) and float(tol) >= 0):
        raise ValueError("tol=%r must be finite and >= 0" % (tol,))
    for name, v in (("huber", huber), ("normal_radius", normal_radius)):
        if v is not None and not (math.isfinite(float(v)) and float(v) > 0):
            raise ValueError("%s=%r must be finite and > 0 (None: %s)" % (name, v, "off" if name == "huber" else "max_dist"))
    if not (isinstance(k, int) and not isinstance(k, bool) and MIN_K <= k <= _lib.KNN_MAX_K):
        raise ValueError("k=%r: an integer %d .. %d" % (k, MIN_K, _lib.KNN_MAX_K))
    if not (math.isfinite(float(min_eig_ratio)) and 0 <= float(min_eig_ratio) < 1):
        raise ValueError("min_eig_ratio=%r: 0 <= ratio < 1" % (min_eig_ratio,))


def check_init(init):
    """init: None or a 4 x 4 rigid matrix about the origin -> (R [3, 3], T [3]) with y = R x + T."""
    if init is None:
        return np.eye(3), np.zeros(3)
    M = np.asarray(init, np.float64)
    if M.shape != (4, 4) or not np.isfinite(M).all() or not np.array_equal(M[3], (0.0, 0.0, 0.0, 1.0)):
        raise ValueError("init: a finite 4 x 4 matrix with the last row 0 0 0 1")
    R = M[:3, :3].copy()
    if not (np.abs(R.T @ R - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0):
        raise ValueError("init: its 3 x 3 block is no rotation (|R^T R - I|_max = %.3g, det = %.3g)"
                         % (np.abs(R.T @ R - np.eye(3)).max(), np.linalg.det(R)))
    return R, M[:3, 3].copy()


def matrix_of(R, t, c):
    """(R, t) about the pivot c -> the 4 x 4 matrix about the origin, [R | c + t - R c]."""
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = (c + t) - R @ c
    return M


def rodrigues(omega):
    """The rotation by the vector omega (radians about its direction); the identity for omega = 0."""
    o = np.asarray(omega, np.float64).reshape(3)
    theta = math.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
    if theta == 0.0:
        return np.eye(3)
    k = o / theta
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    h = math.sin(0.5 * theta)
    return np.eye(3) + math.sin(theta) * K + (2.0 * h * h) * (K @ K)


def solve(sums, L, min_eig_ratio=DEFAULT_MIN_EIG_RATIO):
    """sums [32] of one accumulation -> (omega [3], dt [3], kept): x = - sum over the kept eigenpairs of v (v . g) / lambda, the
    eigenpairs of A (numpy.linalg.eigh) with lambda > min_eig_ratio lambda_max; omega = x[:3] / L, dt = x[3:]."""
    s = np.asarray(sums, np.float64).reshape(-1)
    A = np.zeros((6, 6))
    at = 0
    for u in range(6):
        for v in range(u, 6):
            A[u, v] = A[v, u] = s[at]
            at += 1
    g = s[21:27]
    lam, vec = np.linalg.eigh(A)
    x = np.zeros(6)
    kept = 0
    for i in range(6):
        if lam[-1] > 0 and lam[i] > float(min_eig_ratio) * lam[-1]:
            x = x - vec[:, i] * (float(vec[:, i] @ g) / lam[i])
            kept += 1
    return x[:3] / float(L), x[3:].copy(), kept


def figures(sums, nq, D, where):
    """sums [32] -> dict(pairs, fitness, rms_plane, rms_point); fewer than six pairs is the "lost" error."""
    from . import _lib
    pairs = int(round(float(sums[30])))
    if pairs < MIN_PAIRS:
        raise _lib.AdaMVSHipError("lost: %d pairs within D = %g m %s (at least %d; a start farther than D from the truth needs `init`)"
                                  % (pairs, float(D), where, MIN_PAIRS))
    return dict(pairs=pairs, fitness=pairs / nq, rms_plane=math.sqrt(float(sums[28]) / pairs), rms_point=math.sqrt(float(sums[29]) / pairs))


def frame_of(tmin, tmax, D):
    """The targets' box -> (the pivot c = (min + max) / 2, L = max(half the box diagonal, D))."""
    tmin, tmax = np.asarray(tmin, np.float64).reshape(3), np.asarray(tmax, np.float64).reshape(3)
    e = tmax - tmin
    return (tmin + tmax) / 2.0, max(0.5 * math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]), float(D))


class _Device:
    """The evaluation of one transform on the device: move, search, accumulate, reduce."""

    def __init__(self, source, target, D, huber, normal_radius, k, timing):
        import torch
        from . import _lib, cloud_filter, cloud_lattice
        self.source, self.target = cloud_lattice.cloud(source, "source"), cloud_lattice.cloud(target, "target")
        self.nq, self.nt, self.D, self.delta, self.timing = int(self.source.shape[0]), int(self.target.shape[0]), float(D), float(huber or 0.0), timing
        self.search_pairs = torch.zeros((), device=self.target.device, dtype=torch.int64)
        if self.nq == 0 or self.nt == 0:
            return
        tmin, tmax = self.target.min(0).values.cpu().numpy(), self.target.max(0).values.cpu().numpy()
        if not (np.isfinite(tmin).all() and np.isfinite(tmax).all()):
            raise _lib.AdaMVSHipError("register: a target is not finite")
        self.c, self.L = frame_of(tmin, tmax, D)
        d = self.source - torch.from_numpy(self.c).to(self.source.device)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        self.rho = math.sqrt(float(torch.where(torch.isfinite(d2), d2, torch.zeros_like(d2)).max()))
        self.normal, _, self.flag, _ = cloud_filter.normals(self.target, float(normal_radius or D), k)
        self.origin = cloud_lattice.default_origin(self.D, tmin)
        self.cells = cloud_lattice.Cells(self.target, cloud_lattice.keyed(self.target, self.D, self.origin, "register", "targets"))

    def move(self, x, R, t):
        from . import hip_ops
        return hip_ops.rigid_apply(x, R, self.c, t)

    def evaluate(self, R, t, detail):
        import torch
        from . import cloud_lattice, hip_ops, mesh_stage
        clock = mesh_stage.StageClock(self.timing)
        clock.stage("move")
        Y = self.move(self.source, R, t)
        clock.stage("keys")
        qkeys, _ = hip_ops.simplify_keys(Y, self.D, self.origin)
        clock.stage("sort")
        qs = torch.sort(qkeys, stable=True)
        clock.stage("items")
        _, qorder, items = cloud_lattice.work_items(qs.values, qs.indices)
        clock.stage("nearest")
        index = torch.full((self.nq,), -1, device=Y.device, dtype=torch.int32)
        if items is not None:
            t = self.cells
            _, index, pairs = hip_ops.cloud_nearest(self.origin, self.D, t.ukeys, t.tstart, t.sorted, t.index, Y, qorder, *items)
            self.search_pairs = self.search_pairs + pairs.sum()
        clock.stage("accumulate")
        partial = hip_ops.icp_accumulate(Y, index, self.target, self.normal, self.flag, self.c, self.L, self.delta)
        clock.stage("reduce")
        sums = hip_ops.icp_reduce(partial)
        clock.end()
        if detail is not None:
            detail.setdefault("index", []).append(index)
            detail.setdefault("partial", []).append(partial)
        return sums.cpu().numpy()                       # the iteration's one read of its arithmetic

    def pairs_evaluated(self):
        return int(self.search_pairs)


class _Host:
    """The same evaluation from the host twins of the kernels, on numpy arrays: for checks of the whole loop without a device."""

    def __init__(self, source, target, D, huber, normal_radius, k):
        from . import _lib, accuracy, hip_ops
        self.source = np.ascontiguousarray(np.asarray(source, np.float64).reshape(-1, 3))
        self.target = np.ascontiguousarray(np.asarray(target, np.float64).reshape(-1, 3))
        self.nq, self.nt, self.D, self.delta, self.search_pairs = len(self.source), len(self.target), float(D), float(huber or 0.0), 0
        if self.nq == 0 or self.nt == 0:
            return
        tmin, tmax = self.target.min(0), self.target.max(0)
        if not (np.isfinite(tmin).all() and np.isfinite(tmax).all()):
            raise _lib.AdaMVSHipError("register: a target is not finite")
        self.c, self.L = frame_of(tmin, tmax, D)
        d = self.source - self.c
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        self.rho = math.sqrt(float(np.where(np.isfinite(d2), d2, 0.0).max()))
        Rn = float(normal_radius or D)
        _, nindex, ncount, _ = hip_ops.knn_search_host(self.target, Rn, k, accuracy.default_lattice_origin(Rn, tmin))
        self.normal, _, self.flag = hip_ops.knn_normals_host(self.target, nindex, ncount)
        self.origin = accuracy.default_lattice_origin(self.D, tmin)

    def move(self, x, R, t):
        from . import hip_ops
        return hip_ops.rigid_apply_host(x, R, self.c, t)

    def evaluate(self, R, t, detail):
        from . import hip_ops
        Y = self.move(self.source, R, t)
        _, index, pairs = hip_ops.cloud_nearest_host(self.target, Y, self.D, self.origin)
        self.search_pairs += pairs
        partial = hip_ops.icp_accumulate_host(Y, index, self.target, self.normal, self.flag, self.c, self.L, self.delta)
        if detail is not None:
            detail.setdefault("index", []).append(index)
            detail.setdefault("partial", []).append(partial)
        return hip_ops.icp_reduce_host(partial)

    def pairs_evaluated(self):
        return int(self.search_pairs)


def _loop(be, D, init, max_iter, tol, min_eig_ratio, detail):
    """The iteration both icp and icp_host run: `be` evaluates a transform (the 32 sums), everything else is numpy fp64 here."""
    from . import _lib
    if be.nq == 0 or be.nt == 0:
        raise _lib.AdaMVSHipError("lost: 0 pairs within D = %g m (%d source points, %d targets)" % (float(D), be.nq, be.nt))
    tol = DEFAULT_TOL_RATIO * float(D) if tol is None else float(tol)
    Ri, Ti = init
    c = be.c
    R, t = Ri.copy(), (Ri @ c + Ti) - c
    history, before, converged, constrained = [], None, False, None
    for it in range(max_iter):
        sums = be.evaluate(R, t, detail)
        fig = figures(sums, be.nq, D, "at iteration %d" % it)
        before = before or fig
        omega, dt, kept = solve(sums, be.L, min_eig_ratio)
        dR = rodrigues(omega)
        R, t = dR @ R, dR @ t + dt
        step = math.sqrt((omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2]) * be.rho + \
            math.sqrt((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2])
        history.append(dict(pairs=fig["pairs"], rms_plane=fig["rms_plane"], rms_point=fig["rms_point"], step=step, kept=kept))
        constrained = kept if constrained is None else min(constrained, kept)
        if step <= tol:
            converged = True
            break
    after = figures(be.evaluate(R, t, detail), be.nq, D, "at the final transform")
    before = before or after
    if detail is not None:
        detail.update(backend=be)
    return dict(R=R, t=t, pivot=c.copy(), matrix=matrix_of(R, t, c), iterations=len(history), converged=converged, constrained_dof=constrained,
                history=history, fitness_before=before["fitness"], fitness_after=after["fitness"],
                rms_plane_before=before["rms_plane"], rms_plane_after=after["rms_plane"],
                rms_point_before=before["rms_point"], rms_point_after=after["rms_point"], pairs_before=before["pairs"],
                pairs_after=after["pairs"], pairs=be.pairs_evaluated(), scale=be.L, rho=be.rho, tol=tol)


def icp(source, target, D, init=None, max_iter=DEFAULT_MAX_ITER, tol=None, huber=None, normal_radius=None, k=DEFAULT_K,
        min_eig_ratio=DEFAULT_MIN_EIG_RATIO, detail=None, timing=None):
    """source [nq, 3], target [nt, 3] float64 device tensors -> dict: R [3, 3], t [3] and pivot [3] (numpy; y = R (x - pivot) + pivot
    + t moves the source onto the target), matrix (4 x 4 about the origin), iterations, converged, constrained_dof (the fewest
    eigenpairs kept over the iterations), history (per iteration: pairs, rms_plane, rms_point, step, kept), fitness_before /
    _after (pairs / nq), rms_plane_ and rms_point_before / _after, pairs (the pair evaluations of the searches).  init: a 4 x 4
    rigid matrix about the origin.  detail: a dict that receives the index and partial sums of every evaluation (device tensors)
    and the backend; timing: a list that receives (name, start event, end event) of the stages of every evaluation (STAGES)."""
    check_options(D, max_iter, tol, huber, normal_radius, k, min_eig_ratio)
    start = check_init(init)
    return _loop(_Device(source, target, D, huber, normal_radius, k, timing), D, start, max_iter, tol, min_eig_ratio, detail)


def icp_host(source, target, D, init=None, max_iter=DEFAULT_MAX_ITER, tol=None, huber=None, normal_radius=None, k=DEFAULT_K,
             min_eig_ratio=DEFAULT_MIN_EIG_RATIO, detail=None):
    """icp on numpy arrays through the host twins of every kernel (cloud_nearest_host, knn_search_host, knn_normals_host,
    rigid_apply_host, icp_accumulate_host, icp_reduce_host) and the same loop and solve: small clouds, no device."""
    check_options(D, max_iter, tol, huber, normal_radius, k, min_eig_ratio)
    start = check_init(init)
    return _loop(_Host(source, target, D, huber, normal_radius, k), D, start, max_iter, tol, min_eig_ratio, detail)


def transform(points, R, t, pivot):
    """points [n, 3] float64 device tensor -> R (points - pivot) + pivot + t (adamvs_rigid_apply)."""
    from . import cloud_lattice, hip_ops
    return hip_ops.rigid_apply(cloud_lattice.cloud(points, "points"), R, pivot, t)


def output_paths(out):
    return out + ".json", out + ".txt", out + ".ply"


def _move_point_ply(src, dst, R, t, pivot, device, chunk):
    import torch
    from . import dsm, fusion
    with fusion.PlyWriter(dst) as w:
        for xyz, rgb in dsm.ply_chunks(src, chunk):
            w.write(transform(torch.from_numpy(xyz).to(device), R, t, pivot).cpu().numpy(), rgb)
        return w.count


def _move_mesh_ply(src, dst, R, t, pivot, device):
    """The vertices' x, y, z are rewritten in place in a copy of the file's bytes: header, colours and faces stay as they were."""
    import torch
    from . import fusion
    with open(src, "rb") as f:
        data = bytearray(f.read())
    end = data.index(b"end_header\n") + len(b"end_header\n")
    nv = int([ln for ln in data[:end].decode("ascii").splitlines() if ln.startswith("element vertex")][0].split()[2])
    verts = np.frombuffer(data, fusion.PLY_DTYPE, count=nv, offset=end)
    if nv:
        xyz = np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float64)
        moved = transform(torch.from_numpy(np.ascontiguousarray(xyz)).to(device), R, t, pivot).cpu().numpy()
        verts["x"], verts["y"], verts["z"] = moved[:, 0], moved[:, 1], moved[:, 2]
    with open(dst, "wb") as f:
        f.write(data)
    return nv


def from_files(recon, truth, max_dist, init=None, max_iter=DEFAULT_MAX_ITER, tol=None, huber=None, normal_radius=None, k=DEFAULT_K,
               min_eig_ratio=DEFAULT_MIN_EIG_RATIO, voxel_down=None, spacing=None, spacing_voxels=None, out=None, device=None,
               chunk=1 << 22, log=print):
    """Register the PLY `recon` to the PLY `truth` -> the dict also written to <out>.json."""
    import torch
    from . import accuracy
    t_start = time.time()
    check_options(max_dist, max_iter, tol, huber, normal_radius, k, min_eig_ratio)
    accuracy.check_options(max_dist, (), spacing, voxel_down)
    if spacing is not None and spacing_voxels is not None:
        raise ValueError("give --spacing or --spacing_voxels, not both")
    if isinstance(init, str):
        init = np.loadtxt(init, dtype=np.float64)
    check_init(init)
    if not torch.cuda.is_available():
        raise RuntimeError("register: needs an MI355X (there is no CPU fallback for the cloud registration kernels)")
    device = torch.device(device if device is not None else "cuda")
    out = out or (recon[:-4] if recon.lower().endswith(".ply") else recon) + "_registered"
    clouds, inputs = {}, {}
    for name, path in (("recon", recon), ("truth", truth)):
        clouds[name], inputs[name] = accuracy.load_points(path, max_dist, spacing, spacing_voxels, device)
    if voxel_down is not None:
        clouds["recon"] = clouds["recon"][accuracy.voxel_first(clouds["recon"], voxel_down)].contiguous()
        inputs["recon"].update(voxel_down=float(voxel_down), points_kept=int(clouds["recon"].shape[0]))
    timing = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = icp(clouds["recon"], clouds["truth"], max_dist, init, max_iter, tol, huber, normal_radius, k, min_eig_ratio, timing=timing)
    e1.record()
    torch.cuda.synchronize(device)
    R, t, pivot = res["R"], res["t"], res["pivot"]
    json_path, txt_path, ply_path = output_paths(out)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    if inputs["recon"]["kind"] == "mesh":
        written = _move_mesh_ply(recon, ply_path, R, t, pivot, device)
    else:
        written = _move_point_ply(recon, ply_path, R, t, pivot, device, chunk)
    with open(txt_path, "w") as f:
        for row in res["matrix"]:
            f.write(" ".join("%.17g" % v for v in row) + "\n")
    stage_ms = {}
    for name, a, b in timing:
        stage_ms[name] = stage_ms.get(name, 0.0) + a.elapsed_time(b)
    res = dict(res, R=R.tolist(), t=t.tolist(), pivot=pivot.tolist(), matrix=res["matrix"].tolist())
    res.update(inputs=inputs, options=dict(max_dist=float(max_dist), max_iter=max_iter, tol=res["tol"], huber=huber, normal_radius=normal_radius,
                                           k=k, min_eig_ratio=min_eig_ratio, voxel_down=voxel_down, spacing=spacing,
                                           spacing_voxels=spacing_voxels, init=None if init is None else np.asarray(init).tolist()),
               ply=ply_path, matrix_txt=txt_path, written=written, stage_ms=stage_ms, device_seconds=e0.elapsed_time(e1) / 1e3,
               seconds=time.time() - t_start)
    with open(json_path, "w") as fj:
        json.dump(res, fj, indent=1)
        fj.write("\n")
    log("register: %d points against %d: %d iterations (%s, %d freedoms constrained), fitness %.4f -> %.4f, point-to-plane rms %.4g -> "
        "%.4g m; %d pair evaluations, device %.3f s, total_time = %.3f s, into %s"
        % (clouds["recon"].shape[0], clouds["truth"].shape[0], res["iterations"], "converged" if res["converged"] else "not converged",
           res["constrained_dof"] if res["constrained_dof"] is not None else 0, res["fitness_before"], res["fitness_after"],
           res["rms_plane_before"], res["rms_plane_after"], res["pairs"], res["device_seconds"], res["seconds"], json_path))
    return res


def build_parser():
    ap = argparse.ArgumentParser(description="Align a cloud or mesh to a truth by point-to-plane ICP before it is scored")
    ap.add_argument("--recon", required=True, help="the reconstruction (moved): a point PLY (fuse_whu.py) or a mesh PLY (mesh_whu.py)")
    ap.add_argument("--truth", required=True, help="the truth (fixed): a point PLY or a mesh PLY")
    ap.add_argument("--max_dist", type=float, required=True, metavar="D", help="pairing distance in metres: no correspondence farther is looked for")
    ap.add_argument("--init", default=None, metavar="FILE", help="a 4 x 4 rigid matrix (text, as <out>.txt) to start from (default: the identity)")
    ap.add_argument("--max_iter", type=int, default=DEFAULT_MAX_ITER, help="most iterations (default 50)")
    ap.add_argument("--tol", type=float, default=None, metavar="M", help="stop once no source point moved farther than M metres (default 1e-3 D, a convention)")
    ap.add_argument("--huber", type=float, default=None, metavar="M", help="Huber width in metres: a pair with |r| > M weighs M / |r| (default off)")
    ap.add_argument("--normal_radius", type=float, default=None, metavar="M", help="radius of the truth's normals in metres (default D)")
    ap.add_argument("--k", type=int, default=DEFAULT_K, help="neighbours of a normal, 3 .. 32 (default 16, PCL's and Open3D's convention)")
    ap.add_argument("--min_eig_ratio", type=float, default=DEFAULT_MIN_EIG_RATIO, metavar="E",
                    help="keep the eigenpairs of the normal matrix above E lambda_max (default 1e-6, a convention)")
    ap.add_argument("--voxel_down", type=float, default=None, metavar="V", help="estimate from one source point per cubic cell of side V")
    ap.add_argument("--spacing", type=float, default=None, metavar="S", help="sample spacing on a mesh in metres (default D / 4)")
    ap.add_argument("--spacing_voxels", type=float, default=None, metavar="K", help="sample spacing in voxels of <mesh>.json")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="prefix of <out>.json, <out>.txt and <out>.ply (default <recon minus .ply>_registered)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    if args.spacing is not None and args.spacing_voxels is not None:
        raise SystemExit("register: give --spacing or --spacing_voxels, not both")
    return from_files(args.recon, args.truth, args.max_dist, args.init, args.max_iter, args.tol, args.huber, args.normal_radius, args.k,
                      args.min_eig_ratio, args.voxel_down, args.spacing, args.spacing_voxels, args.out)


if __name__ == "__main__":
    main()
