"""Filter the fused cloud on the GPU before anything reads it: k-nearest-neighbour outlier removal and normals.

    python filter_whu.py --ply /out/predict/fused.ply --radius R [--k 16] [--std_ratio 2.0] [--min_neighbours M]
                         [--normals] [--chunk_queries N] [--out PREFIX]

fuse_whu.py judges a depth against its neighbour views; nothing judges a fused point against the fused points around it.  One
stray above a roof is a spike in the DSM (and gap filling spreads it), a dent or a bump in the TSDF mesh, a miss in the scores.
Both rules here rest on one search (include/adamvs_hip.h "Cloud neighbourhoods" states every operation, csrc/cloud_knn.hip holds
the kernels): for every point the k nearest other points within --radius R.

STATISTICAL rule (--std_ratio s; `off` disables it).  d_ij = sqrt(d2_ij) in fp32, widened to fp64; a missing slot counts as R (the
convention of accuracy.py's mean_trunc); m_i is the fp64 mean over the k slots, summed in slot order.  The m_i are sorted
ascending, mu and sigma (population) are reduced from the sorted values in fp64, so the decision does not depend on the order of
the input, and point i is kept iff m_i <= mu + s sigma.  k = 16 and s = 2.0 are the defaults of PCL's StatisticalOutlierRemoval
and Open3D's remove_statistical_outlier: conventions, not measurements on this pipeline's clouds.
RADIUS rule (--min_neighbours M, default off): kept iff count_i >= M, count_i the neighbours within R (at most k).
With both given, both must hold.

--normals: a normal per KEPT point from its k nearest KEPT points (a second search on the kept cloud: removed points must not
tilt them): the unit eigenvector of the least eigenvalue of the neighbourhood's covariance, and PCL's surface variation
lambda0 / (lambda0 + lambda1 + lambda2) as `curvature`.  Normals point UPWARD (the first non-zero of n_z, n_y, n_x is positive):
the fused PLY does not record which view a point came from, so orientation towards the cameras is out of scope.  A point with
fewer than three neighbours, or with collinear ones, has the normal (0, 0, 0).

The queries run in chunks of work items of at most --chunk_queries points, so the [n][k] arrays never exist for a whole large
cloud; the result equals the unchunked one bit for bit.

Written: `<out>.ply` (the kept points, fuse_whu.py's layout, input order: dsm_whu.py, mesh_whu.py and accuracy_whu.py read it
unchanged), `<out>_removed.ply` (the removed points, same layout), `<out>.json` (counts, mu, sigma, threshold, options, pair
evaluations, timings) and with --normals `<out>_normals.ply` (double x y z, float nx ny nz, float curvature, uchar red green blue).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

DEFAULT_K = 16
DEFAULT_STD_RATIO = 2.0
DEFAULT_CHUNK = 1 << 20
NORMALS_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("curvature", "<f4"),
                          ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def check_options(radius, k=DEFAULT_K, std_ratio=None, min_neighbours=None, chunk_queries=DEFAULT_CHUNK):
    from . import _lib
    if not (isinstance(radius, (int, float)) and not isinstance(radius, bool) and math.isfinite(float(radius)) and float(radius) > 0):
        raise ValueError("radius=%r must be finite and > 0" % (radius,))
    if not (isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= _lib.KNN_MAX_K):
        raise ValueError("k=%r: an integer 1 .. %d" % (k, _lib.KNN_MAX_K))
    if std_ratio is not None and not (math.isfinite(float(std_ratio)) and float(std_ratio) >= 0):
        raise ValueError("std_ratio=%r must be finite and >= 0 (None: the statistical rule is off)" % (std_ratio,))
    if min_neighbours is not None and not (isinstance(min_neighbours, int) and 0 <= min_neighbours <= k):
        raise ValueError("min_neighbours=%r: an integer 0 .. k = %d (no point has more than k neighbours counted)" % (min_neighbours, k))
    if not (isinstance(chunk_queries, int) and chunk_queries >= 1):
        raise ValueError("chunk_queries=%r (>= 1)" % (chunk_queries,))


class Search:
    """The cloud keyed, sorted and cut into the work items of accuracy.nearest (one cell, at most 256 queries), the cloud being both
    the targets and the queries; chunks() runs _knn_search over contiguous ranges of the items."""

    def __init__(self, points, R, k, origin=None, chunk_queries=DEFAULT_CHUNK):
        from . import cloud_lattice
        check_options(R, k, chunk_queries=chunk_queries)
        self.points = points = cloud_lattice.cloud(points, "points", "the neighbour search")
        self.R, self.k, self.chunk_queries = float(R), k, chunk_queries
        self.n = n = int(points.shape[0])
        self.pairs, self.items, self.cells = 0, 0, 0
        if n == 0:
            return
        self.origin = cloud_lattice.origin_of(origin, self.R, points, "point")
        cells = cloud_lattice.Cells(points, cloud_lattice.keyed(points, self.R, self.origin, "knn", "points"))
        self.ukeys, self.tstart, self.order, self.sorted, self.pindex = cells.ukeys, cells.tstart, cells.order, cells.sorted, cells.index
        self.item_key, self.item_first, self.item_count = cells.items()
        self.cells, self.items = int(self.ukeys.numel()), int(self.item_key.numel())
        self.item_end = (self.item_first + self.item_count).cpu().numpy()            # ascending: the items tile the sorted order

    def ranges(self):
        """-> [(first item, past the last item, row_base, rows)]: the most items whose queries number at most chunk_queries, at least
        one item each."""
        out, i0, base = [], 0, 0
        while i0 < self.items:
            i1 = max(int(np.searchsorted(self.item_end, base + self.chunk_queries, "right")), i0 + 1)
            end = int(self.item_end[i1 - 1])
            out.append((i0, i1, base, end - base))
            i0, base = i1, end
        return out

    def chunks(self):
        """Yields (order [rows] int64: the points of the rows in the caller's numbering; d2 [rows, k]; index [rows, k]; count [rows];
        row_base) per chunk."""
        from . import hip_ops
        for i0, i1, base, rows in self.ranges():
            d2, index, count, pairs = hip_ops.knn_search(self.origin, self.R, self.k, self.ukeys, self.tstart, self.sorted, self.pindex,
                                                         self.item_key[i0:i1], self.item_first[i0:i1], self.item_count[i0:i1], base, rows)
            self.pairs += int(pairs.sum())
            yield self.order[base:base + rows], d2, index, count, base


def knn(points, R, k, origin=None, chunk_queries=DEFAULT_CHUNK, info=None):
    """points [n, 3] float64 device tensor -> (d2 [n, k] float32 ascending, +inf padded; index [n, k] int32, -1 padded; count [n]
    int32): the k nearest other points within R of every point, at the point's own position.  info: a dict that receives
    points, cells, items, pairs."""
    import torch
    s = Search(points, R, k, origin, chunk_queries)
    dev = s.points.device
    d2 = torch.full((s.n, k), float("inf"), device=dev, dtype=torch.float32)
    index = torch.full((s.n, k), -1, device=dev, dtype=torch.int32)
    count = torch.zeros(s.n, device=dev, dtype=torch.int32)
    if s.n:
        for order, cd2, cindex, ccount, _ in s.chunks():
            d2[order], index[order], count[order] = cd2, cindex, ccount
    if info is not None:
        info.update(points=s.n, cells=s.cells, items=s.items, pairs=s.pairs)
    return d2, index, count


def mean_distance(d2, R):
    """d2 [rows, k] float32 (+inf: a missing slot) -> m [rows] float64: the mean over the k slots of sqrt(d2) (fp32, widened), a
    missing slot counted as R; summed in slot order, so the bits do not depend on how the rows were chunked."""
    import torch
    d = torch.sqrt(d2).to(torch.float64)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float(R)))
    acc = torch.zeros(d.shape[0], device=d.device, dtype=torch.float64)
    for j in range(d.shape[1]):
        acc = acc + d[:, j]
    return acc / float(d.shape[1])


def neighbourhood(points, R, k, origin=None, chunk_queries=DEFAULT_CHUNK, info=None):
    """-> (m [n] float64, count [n] int32) at the points' own positions, chunk by chunk: the [n][k] arrays never exist whole."""
    import torch
    s = Search(points, R, k, origin, chunk_queries)
    m = torch.full((s.n,), float(R), device=s.points.device, dtype=torch.float64)
    count = torch.zeros(s.n, device=s.points.device, dtype=torch.int32)
    if s.n:
        for order, cd2, _, ccount, _ in s.chunks():
            m[order], count[order] = mean_distance(cd2, R), ccount
    if info is not None:
        info.update(points=s.n, cells=s.cells, items=s.items, pairs=s.pairs)
    return m, count


def statistical_keep(m, std_ratio):
    """m [n] float64 (any device) -> (keep [n] bool, mu, sigma, threshold): keep iff m <= mu + std_ratio sigma, mu and sigma
    (population) reduced from the sorted m in fp64."""
    import torch
    m = m.reshape(-1).to(torch.float64)
    if m.numel() == 0:
        return torch.zeros(0, device=m.device, dtype=torch.bool), None, None, None
    s = torch.sort(m).values
    mu = float(s.mean())
    sigma = math.sqrt(float(((s - mu) * (s - mu)).mean()))
    t = mu + float(std_ratio) * sigma
    return m <= t, mu, sigma, t


def normals(points, R, k, origin=None, chunk_queries=DEFAULT_CHUNK, info=None):
    """points [n, 3] float64 device tensor -> (normal [n, 3] float64, unit and upward, (0, 0, 0) where not valid; curvature [n]
    float32; flag [n] uint8: _lib.KNN_VALID / KNN_TOO_FEW / KNN_COLLINEAR; count [n] int32), from a search of `points` itself."""
    import torch
    from . import _lib, hip_ops
    s = Search(points, R, k, origin, chunk_queries)
    dev = s.points.device
    normal = torch.zeros(s.n, 3, device=dev, dtype=torch.float64)
    curvature = torch.zeros(s.n, device=dev, dtype=torch.float32)
    flag = torch.full((s.n,), _lib.KNN_TOO_FEW, device=dev, dtype=torch.uint8)
    count = torch.zeros(s.n, device=dev, dtype=torch.int32)
    if s.n:
        for order, _, cindex, ccount, base in s.chunks():
            nrm, curv, fl = hip_ops.knn_normals(s.points, cindex, ccount, s.pindex[base:base + cindex.shape[0]])
            normal[order], curvature[order], flag[order], count[order] = nrm, curv, fl, ccount
    if info is not None:
        info.update(points=s.n, cells=s.cells, items=s.items, pairs=s.pairs)
    return normal, curvature, flag, count


def filter_points(points, R, k=DEFAULT_K, std_ratio=DEFAULT_STD_RATIO, min_neighbours=None, origin=None, chunk_queries=DEFAULT_CHUNK):
    """points [n, 3] float64 device tensor -> (keep [n] bool, dict: points, kept, removed, removed_statistical, removed_radius, mu,
    sigma, threshold, isolated (count 0), cells, items, pairs)."""
    import torch
    check_options(R, k, std_ratio, min_neighbours, chunk_queries)
    info = {}
    m, count = neighbourhood(points, R, k, origin, chunk_queries, info)
    keep = torch.ones(m.numel(), device=m.device, dtype=torch.bool)
    res = dict(info, mu=None, sigma=None, threshold=None, removed_statistical=0, removed_radius=0, isolated=int((count == 0).sum()))
    if std_ratio is not None:
        ks, mu, sigma, t = statistical_keep(m, std_ratio)
        keep &= ks
        res.update(mu=mu, sigma=sigma, threshold=t, removed_statistical=int((~ks).sum()))
    if min_neighbours is not None:
        kr = count >= int(min_neighbours)
        keep &= kr
        res.update(removed_radius=int((~kr).sum()))
    res.update(kept=int(keep.sum()), removed=int((~keep).sum()))
    return keep, res


def output_paths(out):
    return out + ".json", out + ".ply", out + "_removed.ply", out + "_normals.ply"


def normals_ply_header(count):
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty float curvature\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % count).encode("ascii")


def write_normals_ply(path, xyz, normal, curvature, rgb):
    rec = np.empty(len(xyz), NORMALS_DTYPE)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rec["nx"], rec["ny"], rec["nz"] = normal[:, 0], normal[:, 1], normal[:, 2]
    rec["curvature"] = curvature
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    with open(path, "wb") as f:
        f.write(normals_ply_header(len(rec)))
        f.write(rec.tobytes())


def read_normals_ply(path):
    """-> structured array of NORMALS_DTYPE (files written by write_normals_ply)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    count = int([ln for ln in data[:end].decode("ascii").splitlines() if ln.startswith("element vertex")][0].split()[2])
    return np.frombuffer(data[end:], NORMALS_DTYPE, count=count)


def from_file(ply, radius, k=DEFAULT_K, std_ratio=DEFAULT_STD_RATIO, min_neighbours=None, with_normals=False, out=None,
              chunk_queries=DEFAULT_CHUNK, device=None, log=print):
    """Filter the point PLY `ply` (fuse_whu.py's layout) -> the dict also written to <out>.json."""
    import torch
    from . import _lib, dsm, fusion, mesh_stage
    t_start = time.time()
    check_options(radius, k, std_ratio, min_neighbours, chunk_queries)
    if not torch.cuda.is_available():
        raise RuntimeError("cloud_filter: needs an MI355X (there is no CPU fallback for the neighbour search)")
    device = torch.device(device if device is not None else "cuda")
    out = out or (ply[:-4] if ply.lower().endswith(".ply") else ply) + "_filtered"
    parts = list(dsm.ply_chunks(ply, 1 << 23))
    xyz = np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, 3), np.float64)
    rgb = np.concatenate([p[1] for p in parts]) if parts else np.zeros((0, 3), np.uint8)
    pts = torch.from_numpy(xyz).to(device)
    timing = []
    clock = mesh_stage.StageClock(timing)
    clock.stage("filter")
    keep, res = filter_points(pts, radius, k, std_ratio, min_neighbours, chunk_queries=chunk_queries)
    kept = keep.cpu().numpy()
    json_path, kept_ply, removed_ply, normals_ply = output_paths(out)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    nres = None
    if with_normals:
        clock.stage("normals")
        info = {}
        nrm, curv, flag, _ = normals(pts[keep].contiguous(), radius, k, chunk_queries=chunk_queries, info=info)
        nres = dict(valid=int((flag == _lib.KNN_VALID).sum()), too_few=int((flag == _lib.KNN_TOO_FEW).sum()),
                    collinear=int((flag == _lib.KNN_COLLINEAR).sum()), pairs=info.get("pairs", 0))
    clock.end()
    torch.cuda.synchronize(device)
    for path, sel in ((kept_ply, kept), (removed_ply, ~kept)):
        with fusion.PlyWriter(path) as w:
            w.write(xyz[sel], rgb[sel])
    if with_normals:
        write_normals_ply(normals_ply, xyz[kept], nrm.cpu().numpy(), curv.cpu().numpy(), rgb[kept])
    res.update(input=ply, options=dict(radius=float(radius), k=k, std_ratio=std_ratio, min_neighbours=min_neighbours, normals=bool(with_normals),
                                       chunk_queries=chunk_queries),
               ply=kept_ply, removed_ply=removed_ply, normals_ply=normals_ply if with_normals else None, normals=nres,
               stage_ms={name: a.elapsed_time(b) for name, a, b in timing},
               device_seconds=timing[0][1].elapsed_time(timing[-1][2]) / 1e3, seconds=time.time() - t_start)
    with open(json_path, "w") as fj:
        json.dump(res, fj, indent=1)
        fj.write("\n")
    log("filter: %d points, %d kept, %d removed (%d by the statistical rule at threshold %s, %d by the radius rule); %d pair evaluations, "
        "device %.3f s, total_time = %.3f s, into %s"
        % (res["points"], res["kept"], res["removed"], res["removed_statistical"], "%.4g m" % res["threshold"] if res["threshold"] is not None
           else "off", res["removed_radius"], res["pairs"], res["device_seconds"], res["seconds"], json_path))
    return res


def _ratio(text):
    return None if text.lower() in ("off", "none") else float(text)


def build_parser():
    ap = argparse.ArgumentParser(description="Filter a fused cloud: k-NN statistical / radius outlier removal and normals")
    ap.add_argument("--ply", required=True, help="the fused cloud: a point PLY as fuse_whu.py writes it")
    ap.add_argument("--radius", type=float, required=True, metavar="R", help="search radius in metres: no neighbour farther is looked for")
    ap.add_argument("--k", type=int, default=DEFAULT_K, help="neighbours per point, 1 .. 32 (default 16, PCL's and Open3D's convention)")
    ap.add_argument("--std_ratio", type=_ratio, default=DEFAULT_STD_RATIO, metavar="S",
                    help="keep a point iff its mean neighbour distance <= mu + S sigma (default 2.0, the same convention; `off`: no statistical rule)")
    ap.add_argument("--min_neighbours", type=int, default=None, metavar="M", help="keep a point iff it has at least M neighbours within R (default off)")
    ap.add_argument("--normals", action="store_true", help="also write <out>_normals.ply: upward normals and curvature of the kept points")
    ap.add_argument("--chunk_queries", type=int, default=DEFAULT_CHUNK, metavar="N", help="queries per launch of the search (default 2^20)")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="prefix of the outputs (default <ply minus .ply>_filtered)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    return from_file(args.ply, args.radius, args.k, args.std_ratio, args.min_neighbours, args.normals, args.out, args.chunk_queries)


if __name__ == "__main__":
    main()
