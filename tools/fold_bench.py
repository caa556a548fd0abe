#!/usr/bin/env python3
"""conv2 / conv4 of CostRegNet2D at the grid sizes of cfg2, cfg3, one GPU's share of cfg4 and cfg5 (GPU box): F(2x2, 3x3), which the
network ran there, against F(2x4, 3x3) on 64-pixel blocks and on the folded blocks that tile these maps (the *_blocks entry points); with
--s2 conv3 / conv5 on the direct stride-2 kernel, the pair form and the folded pair form.

    python tools/fold_bench.py [--s2] [--reps 20] [--only cfg2]   -> one line per (shape, form): mean, standard deviation, min of the launches
                                                                     (--only: one row of SHAPES, for counter passes)

Each form runs `reps` timed launches after two warm-up launches, every launch between its own pair of events.
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ada_mvs_amd  # noqa: E402,F401
from ada_mvs_amd import _lib, hip_ops, packing  # noqa: E402

dev = "cuda"
# (what, N maps, D, h, w of the layer's input)
SHAPES = [("cfg2", 1024, 192), ("cfg3", 128, 192), ("cfg4 share", 16, 192), ("one tile", 4, 192), ("cfg5", 64, 256)]


def launches(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.mean(ms), statistics.pstdev(ms), min(ms)


def report(what, N, D, h, w, name, stats):
    print("%-10s N=%-4d D=%d %3dx%-3d %-28s %8.4f ms  sd %.4f  min %8.4f" % ((what, N, D, h, w, name) + stats), flush=True)


def stride1(what, N, D, h, w, reps):
    x_cl = torch.randn(N, h * w, D, device=dev)
    wt = torch.randn(D, D, 3, 3) / (3 * D ** 0.5)
    bias = (torch.randn(D) * 0.1).to(dev)
    pw, pw4 = packing.pack_reg_layer_wino(wt, torch.ones(D)).to(dev), packing.pack_reg_layer_wino24(wt, torch.ones(D)).to(dev)
    out = torch.empty(N, h * w, D, device=dev)
    report(what, N, D, h, w, "F(2x2,3x3)", launches(lambda: hip_ops.conv3x3_dd_wino(x_cl, pw, bias, None, N, D, h, w, 1, out=out), reps))
    for blocks in (1, -1):
        fold = _lib.load().adamvs_conv_wino24_fold(h, w, blocks)
        report(what, N, D, h, w, "F(2x4,3x3) fold %d" % fold, launches(lambda: hip_ops.conv3x3_dd_wino24(x_cl, pw4, bias, None, N, D, h, w, 1, out=out, blocks=blocks), reps))


def stride2(what, N, D, h, w, reps):
    x_cl = torch.randn(N, h * w, D, device=dev)
    wt = torch.randn(D, D, 3, 3) / (3 * D ** 0.5)
    pk = packing.pack_reg_layer(wt, torch.ones(D), torch.randn(D) * 0.1, False).to(dev)
    out = torch.empty(N, (h // 2) * (w // 2), D, device=dev)
    for name, opts, blocks in (("direct", dict(s2_pairs=0), 0), ("pairs, no folded blocks", {}, 0), ("pairs, folded blocks", {}, -1)):
        with _lib.options(conv_rows2=0, **opts):
            report(what, N, D, h, w, "stride 2 " + name,
                   launches(lambda: hip_ops.conv3x3_dd_s2_blocks(x_cl, pk[:9 * D * D], pk[9 * D * D:], N, D, h, w, 1, blocks, out=out), reps))


if __name__ == "__main__":
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    for what, N, D in SHAPES:
        if only and what != only:
            continue
        for h, w in ((48, 96), (24, 48)) if D == 192 else ((96, 192), (48, 96), (24, 48)):
            (stride2 if "--s2" in sys.argv else stride1)(what, N, D, h, w, reps)
