"""Cloud neighbourhood timing (csrc/cloud_knn.hip through ada_mvs_amd/cloud_filter.py) on the fused cloud of the analytic scene.
    python tools/filter_bench.py [--H 2752 --W 1856] [--ratios 2,4] [--ks 8,16,32] [--runs 10]
The cloud of tools/accuracy_bench.py: the reference view of tools/fusion_bench.py's scene fused against its 4 sources, held on
the device.  Its point spacing is the ground sampling distance of the reference camera; per R / spacing in --ratios and per k in
--ks, 2 warm-ups and then --runs calls, device events, the median over the runs:
  search    one _knn_search launch over every work item (the [n][k] outputs included), in pair evaluations per second;
  nearest   the yardstick: the `nearest` stage of accuracy.nearest on the same cloud against itself at D = R (the 1-NN kernel on
            the same work items and candidates: every point finds itself at distance 0), in the same unit;
  ratio     search time per pair over nearest time per pair (k / 4 is where the cost of keeping k instead of one would be called
            unremarkable);
  filter    filter_points (keys, sorts, work items, search in chunks, mean distances, the statistical rule) and normals (the same
            and the normals kernel), whole calls.
One JSON line; there is no pass bar, nothing of this had a number before.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import ada_mvs_amd  # noqa: E402,F401


def timed(fn, runs, warmup=2):
    import torch
    ms, out = [], None
    for i in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def nearest_stage(cloud, R, runs, warmup=2):
    """-> (median ms of the `nearest` stage of accuracy.nearest(cloud, cloud, R), pairs)."""
    import torch
    from ada_mvs_amd import accuracy
    ms, info = [], None
    for i in range(warmup + runs):
        timing = []
        _, _, info = accuracy.nearest(cloud, cloud, R, timing=timing)
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(dict((n, a.elapsed_time(b)) for n, a, b in timing)["nearest"])
    return float(np.median(ms)), info["pairs"]


def run(cloud, R, ks, runs):
    from ada_mvs_amd import cloud_filter, hip_ops
    n = int(cloud.shape[0])
    near_ms, near_pairs = nearest_stage(cloud, R, runs)
    near_rate = near_pairs / (near_ms * 1e-3)
    res = dict(radius=R, points=n, nearest_ms=round(near_ms, 3), nearest_pairs=near_pairs, nearest_pairs_per_s=round(near_rate, 1), per_k={})
    for k in ks:
        s = cloud_filter.Search(cloud, R, k, chunk_queries=n)
        ms, out = timed(lambda: hip_ops.knn_search(s.origin, R, k, s.ukeys, s.tstart, s.sorted, s.pindex, s.item_key, s.item_first,
                                                   s.item_count, 0, n), runs)
        pairs = int(out[3].sum())
        rate = pairs / (ms * 1e-3)
        f_ms, (keep, fres) = timed(lambda: cloud_filter.filter_points(cloud, R, k), max(runs // 3, 1), 1)
        n_ms, _ = timed(lambda: cloud_filter.normals(cloud, R, k), max(runs // 3, 1), 1)
        res["per_k"]["%d" % k] = dict(search_ms=round(ms, 3), pairs=pairs, pairs_per_query=round(pairs / n, 1), pairs_per_s=round(rate, 1),
                                       per_pair_over_nearest=round(near_rate / rate, 2), k_over_4=k / 4.0, cells=s.cells, items=s.items,
                                       queries_per_item=round(n / max(s.items, 1), 2), full_rows=round(float((out[2] == k).double().mean()), 4),
                                       mean_count=round(float(out[2].double().mean()), 2), filter_ms=round(f_ms, 3),
                                       normals_ms=round(n_ms, 3), removed=fres["removed"], threshold=fres["threshold"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--ratios", default="2,4", help="R / point spacing")
    ap.add_argument("--ks", default="8,16,32")
    ap.add_argument("--runs", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("filter_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from accuracy_bench import fused_reference_view
    dev = torch.device("cuda")
    t0 = time.time()
    cloud, spacing = fused_reference_view(args.H, args.W, dev)
    res = {"workload": "filter", "H": args.H, "W": args.W, "points": int(cloud.shape[0]), "point_spacing": round(spacing, 4), "runs": args.runs,
           "setup_s": round(time.time() - t0, 2), "per_ratio": {}}
    ks = [int(v) for v in args.ks.split(",")]
    for r in (float(v) for v in args.ratios.split(",")):
        res["per_ratio"]["%g" % r] = run(cloud, r * spacing, ks, args.runs)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
