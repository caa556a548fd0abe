"""Drainage timing (csrc/dsm_drainage.hip): surface, fill, directions, accumulation, basins and streams at the raster benches' size.

    python tools/drainage_bench.py [--H 2751 --W 2562] [--gsd 0.16] [--relief 40.0] [--hole-fraction 0.02] [--min_area 1000.0]
                                   [--steps 5 --warmup 1] [--seed 7]

Input: a synthetic fractal DTM (spectral synthesis, power-law spectrum of exponent --beta, seeded; a tilt across the raster so that
it drains; square holes over --hole-fraction of the cells) of the size the other raster benches reach with the bench scene (about
2562 x 2751 cells at 0.16 m).  Parameters: the defaults of drainage_whu.py (1000 m^2, one smoothing pass).  Each phase is timed with
device events around the call after warm-up, median and p10-p90 over --steps runs; the calls that block (fill, accumulation,
streams) include their read-backs:
  surface       adamvs_contour_surface
  fill          adamvs_drain_fill: the rounds that changed a word and the rounds launched are reported, and the time per round
                launched (a round reads and writes F once: 8 B per cell, 4 B of r where a cell can move); fill_one_tile is the
                same call on one flat tile: the init kernel, four rounds of one workgroup and one read-back of the changed words,
                that is what a chunk of four rounds costs beside its kernels
  direction     adamvs_drain_direction (F in, dir out: 5 B per cell; the eight neighbours are re-reads served by the caches)
  accumulation  adamvs_drain_accumulate with value = 1: two kernels per round, rounds reported
  basins        the numbering of the outlets and the look-up through root (torch: a scan, a gather)
  streams       adamvs_drain_streams, adamvs_drain_links and the second accumulation for the magnitude
against 6.3 TB/s (measured HBM copy rate) where a model is stated.  The host's share (coordinates, lengths, Strahler pass, GeoJSON
text) is timed once.  CPU baseline on the 256 x 256 crop at the centre: the host restatement (tests/drainage_ref.py).  One JSON
line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import ada_mvs_amd  # noqa: E402,F401

HBM_BPS = 6.3e12
BYTES = dict(fill_round=12, direction=5)


def fractal_dtm(H, W, relief, beta, hole_fraction, seed):
    """-> z float32 [H, W]: a power-law surface of about `relief` metres with a tilt of relief / 2 from west to east, NaN in holes"""
    rng = np.random.default_rng(seed)
    fy, fx = np.meshgrid(np.fft.fftfreq(H), np.fft.rfftfreq(W), indexing="ij")
    f = np.hypot(fy, fx)
    f[0, 0] = 1.0
    spec = (rng.standard_normal(f.shape) + 1j * rng.standard_normal(f.shape)) * f ** (-beta / 2.0)
    spec[0, 0] = 0.0
    z = np.fft.irfft2(spec, s=(H, W))
    z = (z - z.min()) / (z.max() - z.min()) * relief - 0.5 * relief * np.arange(W)[None, :] / W
    z = z.astype(np.float32)
    side = 24
    for _ in range(int(hole_fraction * H * W / side ** 2)):
        i, j = int(rng.integers(0, H - side)), int(rng.integers(0, W - side))
        z[i:i + side, j:j + side] = np.nan
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2751)
    ap.add_argument("--W", type=int, default=2562)
    ap.add_argument("--gsd", type=float, default=0.16)
    ap.add_argument("--relief", type=float, default=40.0)
    ap.add_argument("--beta", type=float, default=4.0)
    ap.add_argument("--hole-fraction", type=float, default=0.02)
    ap.add_argument("--min_area", type=float, default=1000.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("drainage_bench: needs an MI355X (no CPU timing of the kernels is reported)")
    from ada_mvs_amd import drainage, dsm, hip_ops, raster_stage
    from dtm_bench import timed
    t0 = time.time()
    z = fractal_dtm(args.H, args.W, args.relief, args.beta, args.hole_fraction, args.seed)
    scene_s = time.time() - t0
    H, W = z.shape
    n = H * W
    grid = dsm.Grid(0.0, H * args.gsd, args.gsd, 0.0, W, H)
    p = drainage.parameters(args.gsd, args.min_area)
    dev = torch.device("cuda")
    zz = torch.from_numpy(z).to(dev)
    out = {"workload": "drainage", "W": W, "H": H, "cells": n, "gsd": args.gsd, "relief_m": args.relief, "beta": args.beta,
           "hole_fraction": args.hole_fraction, "min_area": p["min_area"], "min_cells": p["min_cells"], "smooth_passes": p["smooth_passes"],
           "steps": args.steps, "warmup": args.warmup, "seed": args.seed, "bytes": BYTES, "tile": drainage.TILE}

    def entry(med, band, **more):
        return dict({"ms_median": round(med, 3), "ms_p10_p90": band}, **more)

    def roof(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / HBM_BPS, 3) if ms > 0 else None

    (s, info), med, band = timed(lambda: hip_ops.contour_surface(zz, 0.0, p["smooth_passes"]), args.steps, args.warmup)
    out["surface"] = entry(med, band)
    if int(info.cpu()[2]):
        raise SystemExit("drainage_bench: cells out of range")
    (r, F, st, ws), med, band = timed(lambda: hip_ops.drain_fill(s, p["smooth_passes"], n + 1), args.steps, args.warmup)
    if not st["converged"]:
        raise SystemExit("drainage_bench: the fill did not converge")
    out["fill"] = entry(med, band, rounds=st["rounds"], rounds_launched=st["launched"], ms_per_round_launched=round(med / st["launched"], 4),
                        round_hbm_roof_fraction=roof(n * BYTES["fill_round"], med / st["launched"]))
    # what a chunk costs beside its kernels: a flat raster of one tile settles in one round, so the call is the init kernel, four
    # rounds of one workgroup and one read-back of the changed words
    flat = torch.zeros(drainage.TILE, drainage.TILE, device=dev, dtype=torch.int32)
    (_, _, st1, _), med1, band1 = timed(lambda: hip_ops.drain_fill(flat, 0, n + 1), 5 * args.steps, args.warmup)
    out["fill_one_tile"] = entry(med1, band1, rounds=st1["rounds"], rounds_launched=st1["launched"])
    direction, med, band = timed(lambda: hip_ops.drain_direction(F), args.steps, args.warmup)
    out["direction"] = entry(med, band, hbm_roof_fraction=roof(n * BYTES["direction"], med))
    (acc, root, st_acc, ws), med, band = timed(lambda: hip_ops.drain_accumulate(direction, None, ws), args.steps, args.warmup)
    out["accumulation"] = entry(med, band, rounds=st_acc["rounds"], rounds_launched=st_acc["launched"])

    def basins():
        number, n_out = hip_ops._number_roots(root)
        outlet = torch.nonzero(root.view(-1) == torch.arange(n, device=dev, dtype=torch.int32)).view(-1)
        keep = (acc.view(-1)[outlet] >= p["min_cells"]).cpu().numpy()
        return raster_stage.relabel_kept(number, keep), n_out, int(keep.sum())
    (label, n_out, K), med, band = timed(basins, args.steps, args.warmup)
    out["basins"] = entry(med, band, outlets=int(n_out), basins=K)

    def streams():
        nd, link, pos, L, P, st_s, w = hip_ops.drain_streams(direction, acc, p["min_cells"], ws)
        table = hip_ops.drain_links(direction, nd, link, pos, L, P, w)
        mag = hip_ops.drain_accumulate(direction, (nd == 0).to(torch.int32), w)[0]
        return nd, link, pos, L, P, st_s, table, mag
    (nd, link, pos, L, P, st_s, table, mag), med, band = timed(streams, args.steps, args.warmup)
    out["streams"] = entry(med, band, rank_rounds=st_s["rounds"], rank_rounds_launched=st_s["launched"], links=L, vertices=P)
    phases = ("surface", "fill", "direction", "accumulation", "basins", "streams")
    total = sum(out[k]["ms_median"] for k in phases)
    out["total_ms"] = round(total, 3)
    out["dominant"] = max(phases, key=lambda k: out[k]["ms_median"])
    res = dict(F=F, acc=acc, link=link, magnitude=mag, basins=label, link_first=table[0], link_head=table[1], link_end=table[2], link_to=table[3],
               vertex=table[4])
    res = {k: v.cpu().numpy() for k, v in res.items()}
    t1 = time.time()
    cols = drainage.link_properties(res, grid)
    feats = drainage.features(res, cols, grid)
    t2 = time.time()
    text = drainage.geojson_text(feats)
    t3 = time.time()
    Fh, rh = res["F"], r.cpu().numpy()
    out.update(valid_cells=int((Fh != drainage.NO_DATA).sum()), filled_cells=int((Fh > rh).sum()),
               max_sink_depth_m=round(float((Fh.astype(np.int64) - rh).max()) / drainage.UNITS, 3), max_acc=int(res["acc"].max()),
               max_strahler=int(cols["strahler"].max()) if L else 0, longest_link_vertices=int(np.diff(res["link_first"]).max()) if L else 0,
               host={"columns_features_s": round(t2 - t1, 3), "geojson_text_s": round(t3 - t2, 3), "geojson_bytes": len(text)})
    # CPU baseline on the central 256 x 256 crop
    import drainage_ref
    i0, j0 = max(0, H // 2 - 128), max(0, W // 2 - 128)
    t1 = time.time()
    ref = drainage_ref.route(z[i0:i0 + 256, j0:j0 + 256], 0.0, p["smooth_passes"], p["min_cells"], drainage.TILE)
    out["cpu_crop"] = {"crop": [i0, j0, 256, 256], "host_restatement_s": round(time.time() - t1, 2), "links": ref["L"], "rounds_bound": ref["bound"]}
    out["scene_s"] = round(scene_s, 1)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
