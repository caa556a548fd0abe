"""Cloud distance timing (csrc/cloud_dist.hip through ada_mvs_amd/accuracy.py) on the fused cloud of the analytic scene.
    python tools/accuracy_bench.py [--H 2752 --W 1856] [--ratios 2,4] [--jitter 0.25] [--runs 10] [--crop 20000]
The reference view of tools/fusion_bench.py's scene fused against its 4 sources, held on the device: the truth.  The
reconstruction is a copy jittered by a seeded uniform +-jitter D per axis.  The point spacing is the ground sampling distance of
the reference camera; per D / spacing in --ratios, 2 warm-ups and then --runs calls of nearest() (truth as targets, the copy as
queries) and of summarise(): device events around the whole call and around every stage (keys, sorts, items = the work list,
nearest = the kernel, statistics), the median over the runs.  Reported next to it: pair evaluations per second of the kernel,
their share of the fp32 VALU rate (VALU_PER_PAIR vector instructions per pair in the sweep's ISA, against 256 CUs x 4 SIMDs x 32
lanes per clock at 2.4 GHz), ns per query.  Two baselines on a crop of --crop queries and their targets' neighbourhood (both hold
the full distance matrix): chunked torch.cdist(...).min on the same GPU, and the numpy restatement (tests/accuracy_ref.py) on the
CPU.  One JSON line; there is no pass bar, nothing of this had a number before.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import ada_mvs_amd  # noqa: E402,F401

# the sweep of k_cloud_nearest per (query, candidate) pair and lane: v_pk_add_f32, v_sub_f32, v_pk_mul_f32, v_mul_f32, 2 v_add_f32,
# 3 v_cmp, 2 v_cndmask (and 1/64 of a ds_read_b128, 2 scalar mask operations)
VALU_PER_PAIR = 11
VALU_LANE_RATE = 256 * 4 * 32 * 2.4e9
STAGES = ("keys", "sorts", "items", "nearest")


def fused_reference_view(H, W, device):
    """-> (points [n, 3] float64 on the device, the ground sampling distance in metres)."""
    import torch
    from ada_mvs_amd import fusion, fusion_synth
    sc = fusion_synth.scene(H, W, 4, seed=0)
    views = [dict(depth=torch.from_numpy(d).to(device), K=c["K"], R=c["R"], C=c["C"]) for c, d in zip(sc["cams"], sc["depths"])]
    _, _, xyz, _ = fusion.fuse_view(views[0], views[1:], torch.from_numpy(sc["confs"][0]).to(device), torch.from_numpy(sc["rgba"]).to(device))
    return xyz.clone(), float(sc["cams"][0]["C"][2] / sc["cams"][0]["K"][0, 0])


def run(truth, recon, D, runs, warmup=2):
    import torch
    from ada_mvs_amd import accuracy
    per_stage, totals, stats_ms, info = {}, [], [], None
    for i in range(warmup + runs):
        timing = []
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        dist, _, info = accuracy.nearest(truth, recon, D, timing=timing)
        e1.record()
        summary = accuracy.summarise(dist, D)
        e2.record()
        torch.cuda.synchronize()
        if i < warmup:
            continue
        totals.append(e0.elapsed_time(e1))
        stats_ms.append(e1.elapsed_time(e2))
        for name, a, b in timing:
            per_stage.setdefault(name, []).append(a.elapsed_time(b))
    stages = {k: float(np.median(v)) for k, v in per_stage.items()}
    stages["statistics"] = float(np.median(stats_ms))
    total, kernel = float(np.median(totals)), stages["nearest"]
    rate = info["pairs"] / (kernel * 1e-3)
    return dict(max_dist=D, device_ms=round(total, 3), stage_ms={k: round(v, 3) for k, v in stages.items()}, targets=info["targets"],
                queries=info["queries"], cells=info["cells"], items=info["items"], within=info["within"], pairs=info["pairs"],
                pairs_per_query=round(info["pairs"] / max(info["queries"], 1), 1), pairs_per_s=round(rate, 1),
                valu_per_pair=VALU_PER_PAIR, frac_of_fp32_valu=round(rate * VALU_PER_PAIR / VALU_LANE_RATE, 4),
                ns_per_query=round(total * 1e6 / max(info["queries"], 1), 3),
                kernel_ns_per_query=round(kernel * 1e6 / max(info["queries"], 1), 3), mean_within=summary["mean_within"])


def baselines(truth, recon, D, crop, runs):
    """A crop of queries (a square patch around the cloud's centre) and the targets within D of its box: torch.cdist in chunks on the
    GPU, the numpy restatement on the CPU, and the kernel on the same crop."""
    import torch
    import accuracy_ref as R
    from ada_mvs_amd import accuracy
    c = truth.mean(0)
    order = torch.sort(((recon[:, :2] - c[:2]).abs().max(1).values)).indices[:crop]
    q = recon[order].contiguous()
    lo, hi = q.min(0).values - D, q.max(0).values + D
    t = truth[((truth >= lo) & (truth <= hi)).all(1)].contiguous()

    def cdist_min():
        out = []
        for s in range(0, q.shape[0], 4096):
            d, j = torch.cdist(q[s:s + 4096], t).min(1)
            out.append(torch.where(d <= D, d, torch.full_like(d, float("inf"))))
        return torch.cat(out)

    def timed(fn):
        ms = []
        for i in range(2 + runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(a.elapsed_time(b))
        return float(np.median(ms)), r

    cd_ms, cd = timed(cdist_min)
    k_ms, (kd, _, info) = timed(lambda: accuracy.nearest(t, q, D))
    t0 = time.time()
    ref = R.nearest(t.cpu().numpy(), q.cpu().numpy(), D)
    cpu_s = time.time() - t0
    both = torch.isfinite(cd) & torch.isfinite(kd)
    return dict(queries=int(q.shape[0]), targets=int(t.shape[0]), max_dist=D, kernel_ms=round(k_ms, 3), kernel_pairs=info["pairs"],
                torch_cdist_min_ms=round(cd_ms, 3), torch_cdist_pairs=int(q.shape[0]) * int(t.shape[0]),
                numpy_restatement_s=round(cpu_s, 3), within=int(torch.isfinite(kd).sum()), within_cdist=int(torch.isfinite(cd).sum()),
                within_numpy=int(np.isfinite(ref[0]).sum()),
                max_abs_diff_to_cdist=float((cd[both] - kd[both].double()).abs().max()) if bool(both.any()) else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2752)
    ap.add_argument("--W", type=int, default=1856)
    ap.add_argument("--ratios", default="2,4", help="D / point spacing")
    ap.add_argument("--jitter", type=float, default=0.25, help="the copy's uniform jitter per axis, as a share of D")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--crop", type=int, default=20000, help="queries of the crop the baselines are timed on (0: skip)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("accuracy_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    dev = torch.device("cuda")
    t0 = time.time()
    truth, spacing = fused_reference_view(args.H, args.W, dev)
    res = {"workload": "accuracy", "H": args.H, "W": args.W, "points": int(truth.shape[0]), "point_spacing": round(spacing, 4), "jitter": args.jitter,
           "runs": args.runs, "setup_s": round(time.time() - t0, 2), "per_ratio": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    unit = torch.rand(truth.shape, device=dev, dtype=torch.float64, generator=gen) * 2.0 - 1.0
    ratios = [float(v) for v in args.ratios.split(",")]
    for k in ratios:
        D = k * spacing
        res["per_ratio"]["%g" % k] = run(truth, truth + unit * (args.jitter * D), D, args.runs)
    if args.crop:
        D = ratios[0] * spacing
        res["baselines"] = baselines(truth, truth + unit * (args.jitter * D), D, args.crop, args.runs)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
