"""Depth-map fusion on the GPU (csrc/fusion.hip through the C ABI) against the fp64 restatement (tests/fusion_ref.py) and the
analytic scenes of ada_mvs_amd/fusion_synth.py; fuse_whu.py end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import fusion, fusion_synth
from conftest import ROOT
from fusion_ref import interior, patch, pixel_margin, restate, ties, visible_sources

pytestmark = pytest.mark.gpu

OFFSET = np.array([5e5, 3.4e6, 0.0])


def _views(sc):
    return [dict(cam=c, depth=d) for c, d in zip(sc["cams"][1:], sc["depths"][1:])]


def run_kernel(sc, ref_depth=None, ref_conf=None, src_depths=None, **thr):
    """fusion.fuse_view on the scene -> numpy (count, fused, xyz, rgb)."""
    import torch
    dev = torch.device("cuda")
    cams = sc["cams"]
    depths = [sc["depths"][0] if ref_depth is None else ref_depth] + list(sc["depths"][1:] if src_depths is None else src_depths)
    views = [dict(depth=torch.from_numpy(np.ascontiguousarray(d)).to(dev), K=c["K"], R=c["R"], C=c["C"]) for c, d in zip(cams, depths)]
    conf = torch.from_numpy(np.ascontiguousarray(sc["confs"][0] if ref_conf is None else ref_conf)).to(dev)
    rgba = torch.from_numpy(sc["rgba"]).to(dev)
    count, fused, xyz, rgb = fusion.fuse_view(views[0], views[1:], conf, rgba, **thr)
    torch.cuda.synchronize()
    return count.cpu().numpy(), fused.cpu().numpy(), xyz.cpu().numpy(), rgb.cpu().numpy()


def run_ref(sc, ref_depth=None, ref_conf=None, src_depths=None, **thr):
    srcs = _views(sc)
    if src_depths is not None:
        srcs = [dict(cam=s["cam"], depth=d) for s, d in zip(srcs, src_depths)]
    return restate(sc["depths"][0] if ref_depth is None else ref_depth, sc["confs"][0] if ref_conf is None else ref_conf, sc["cams"][0],
                   srcs, rgba=sc["rgba"], keep_uv=True, **thr)


def compare(sc, ker, ref):
    """The kernel against the restatement: decisions outside the tie margins identical, fused depths and points.
    Where a pixel's bilinear taps lie on its own face in every source (fusion_ref.interior) the fused depth is held to 1e-6
    and the point to 2e-6 of the depth.  Where a tap straddles a depth edge the sample's slope (up to the building's height
    per pixel) multiplies the fp32 rounding of the tap position (up to ~5e-4 px at 2752 px): those pixels are held to 2e-4
    (8.7e-5 measured at 2752 x 1856), and their decisions are compared outside wider margins."""
    count, fused, xyz, rgb = ker
    tie = ties(ref)
    assert tie.mean() <= 1e-4, tie.mean()
    smooth = interior(sc, ref)
    # at a tap across a depth edge the same fp32 position error moves d' by up to ~1e-2 m and the reprojected pixel by a few
    # 1e-2 px (the full-size scene flipped 4 of 5.1 M pixels, all such, with pixel margins of 3e-3 .. 2e-2 px)
    # (margins in proportion to the fp32 spacing of the largest pixel coordinate: 0.05 px / 1e-4 at 2048 .. 4096 px)
    scale = pixel_margin(*fused.shape, floor=0.0) / pixel_margin(2752, 1856, floor=0.0)
    edge_tie = ~smooth & ((ref["pix_tie"] < 0.05 * scale) | (ref["depth_tie"] < 1e-4 * scale))
    assert edge_tie.mean() <= 2e-3, edge_tie.mean()
    sure = ~(tie | edge_tie)
    assert np.array_equal(count[sure], ref["count"][sure]), np.argwhere(sure & (count != ref["count"]))[:10]
    kept = fused > 0
    assert np.array_equal(kept[sure], ref["kept"][sure])
    both = kept & ref["kept"]
    assert both.sum() > 0
    rel = np.abs(fused - ref["fused"]) / np.where(both, ref["fused"], 1.0)
    assert rel[both & smooth].max() <= 1e-6, rel[both & smooth].max()
    assert rel[both].max() <= 2e-4, rel[both].max()
    # points: one per kept pixel, in row-major pixel order
    assert len(xyz) == kept.sum() and len(rgb) == kept.sum()
    common, pk, pr = np.intersect1d(np.flatnonzero(kept), np.flatnonzero(ref["kept"]), return_indices=True)
    err = np.abs(xyz[pk] - ref["xyz"][pr]).max(1) / ref["fused"].reshape(-1)[common]
    on_face = smooth.reshape(-1)[common]
    assert (err[on_face] <= 2e-6).all(), err[on_face].max()
    assert (err <= 2e-4).all(), err.max()
    assert np.array_equal(rgb[pk], ref["rgb"][pr])


PARITY = [
    pytest.param(256, 320, 4, None, id="320x256-N4"),
    pytest.param(256, 320, 1, None, id="320x256-N1"),
    pytest.param(203, 317, 16, [(190 + 7 * k, 300 + 5 * (k % 6)) for k in range(16)], id="odd-N16-mixed-sizes"),
    pytest.param(131, 263, 4, [(140, 250), (120, 270), (131, 263), (99, 201)], id="odd-N4-mixed-sizes"),
    pytest.param(2752, 1856, 4, None, id="2752x1856-N4"),
]


@pytest.mark.parametrize("H,W,N,sizes", PARITY)
def test_kernel_matches_restatement(H, W, N, sizes):
    sc = fusion_synth.scene(H, W, N, sizes, seed=H + N)
    mc = min(2, N)
    ker = run_kernel(sc, min_consistent=mc)
    ref = run_ref(sc, min_consistent=mc)
    compare(sc, ker, ref)
    assert ref["kept"].mean() > 0.2


def test_kernel_matches_restatement_on_corrupted_maps():
    """NaN / inf / 0 in every map, NaN confidences: the taps' validity tests, pixel for pixel."""
    sc = fusion_synth.scene(256, 320, 4, seed=5)
    rng = np.random.default_rng(5)
    bad_vals = np.array([np.nan, np.inf, -np.inf, 0.0, -3.0], np.float32)
    depths = []
    for d in sc["depths"]:
        d = d.copy()
        m = rng.random(d.shape) < 0.02
        d[m] = bad_vals[rng.integers(0, len(bad_vals), m.sum())]
        depths.append(d)
    conf = sc["confs"][0].copy()
    conf[rng.random(conf.shape) < 0.02] = np.nan
    ker = run_kernel(sc, depths[0], conf, depths[1:])
    ref = run_ref(sc, depths[0], conf, depths[1:])
    compare(sc, ker, ref)
    fused = ker[1]
    assert not (fused > 0)[~np.isfinite(depths[0]) | (depths[0] <= 0) | np.isnan(conf)].any()
    assert np.isfinite(ker[2]).all() and np.isfinite(fused).all()


def test_geometry_on_the_analytic_scene():
    sc = fusion_synth.scene(256, 320, 4, seed=7)
    sc["confs"][0][:] = 1.0
    count, fused, xyz, rgb = run_kernel(sc)
    ref = run_ref(sc)
    kept = fused > 0
    inner = interior(sc, ref)
    true_d, _ = fusion_synth.render(sc["cams"][0])
    cam = sc["cams"][0]
    H, W = true_d.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    Xtrue = ((np.stack([x, y, np.ones_like(x)], -1) @ np.linalg.inv(cam["K"]).T) * true_d[..., None] @ cam["R"].T + cam["C"]).reshape(-1, 3)
    idx = np.flatnonzero(kept)
    dist = np.linalg.norm(xyz - Xtrue[idx], axis=1)
    depth = true_d.reshape(-1)[idx]
    is_inner = inner.reshape(-1)[idx]
    assert is_inner.sum() > 0.3 * H * W
    assert (dist[is_inner] <= 1e-5 * depth[is_inner]).all(), (dist[is_inner] / depth[is_inner]).max()
    assert (dist[~is_inner] <= 0.01 * depth[~is_inner]).all(), (dist[~is_inner] / depth[~is_inner]).max()
    want = inner & (visible_sources(sc) >= 2)
    assert kept[want].mean() >= 0.99, kept[want].mean()
    assert np.isfinite(xyz).all()
    # +3 % depth on a patch of the reference: rejected
    rows, cols = patch(H, W)
    assert kept[rows, cols].mean() > 0.9
    bad = sc["depths"][0].copy()
    bad[rows, cols] *= 1.03
    _, fused2, _, _ = run_kernel(sc, ref_depth=bad)
    assert not (fused2[rows, cols] > 0).any()
    # NaN / inf / 0 depths and NaN confidences never give a point
    bad = sc["depths"][0].copy()
    conf = sc["confs"][0].copy()
    bad[100:110, 100:200] = np.nan
    bad[120:130, 100:200] = np.inf
    bad[140:150, 100:200] = 0.0
    conf[160:170, 100:200] = np.nan
    _, fused3, xyz3, _ = run_kernel(sc, ref_depth=bad, ref_conf=conf)
    for r in (slice(100, 110), slice(120, 130), slice(140, 150), slice(160, 170)):
        assert not (fused3[r, 100:200] > 0).any()
    assert np.isfinite(xyz3).all() and (fused3 > 0).sum() == len(xyz3)


def test_world_coordinates_far_from_the_origin():
    """The same scene shifted by (5e5, 3.4e6, 0): the unshifted points plus the offset, within 1e-3 m."""
    near = fusion_synth.scene(256, 320, 4, seed=9)
    far = fusion_synth.scene(256, 320, 4, offset=OFFSET, seed=9)
    _, fa, xa, _ = run_kernel(near)
    _, fb, xb, _ = run_kernel(far)
    ka, kb = fa > 0, fb > 0
    assert (ka != kb).mean() < 1e-3
    both = np.flatnonzero(ka & kb)
    ia = np.searchsorted(np.flatnonzero(ka), both)
    ib = np.searchsorted(np.flatnonzero(kb), both)
    err = np.abs(xb[ib] - OFFSET - xa[ia]).max()
    assert err < 1e-3, err
    # the yardstick is sharp: the camera -> world step in fp32 misses it by two orders of magnitude
    cam = far["cams"][0]
    X64 = xb[ib] - cam["C"]
    X32 = (X64.astype(np.float32) + cam["C"].astype(np.float32)).astype(np.float64)
    assert np.abs(X32 - OFFSET - xa[ia]).max() > 0.05


def test_bit_identical_runs():
    sc = fusion_synth.scene(203, 317, 16, [(190 + 7 * k, 300 + 5 * (k % 6)) for k in range(16)], seed=11)
    a = run_kernel(sc)
    b = run_kernel(sc)
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()


# ---- end to end: predict's output layout -> fuse_whu.py ------------------------------------------------------------------
def test_fuse_whu_end_to_end(tmp_path):
    import shutil
    sc = fusion_synth.scene(192, 256, 4, offset=OFFSET, seed=13)
    data, out_cli = str(tmp_path / "data"), str(tmp_path / "out_cli")
    fusion_synth.write_predict_layout(sc, data, out_cli)
    out_api = str(tmp_path / "out_api")
    shutil.copytree(out_cli, out_api)
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fuse_whu.py"), "--data_folder", data, "--output_folder", out_cli],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "total_time" in r.stdout
    res = fusion.fuse_folder(data, out_api, log=lambda *a: None)
    assert res["views"] == 5 and res["points"] > 0.3 * 5 * 192 * 256
    a = open(os.path.join(out_cli, "fused.ply"), "rb").read()
    b = open(os.path.join(out_api, "fused.ply"), "rb").read()
    assert a == b
    pts = fusion.read_ply(os.path.join(out_cli, "fused.ply"))
    assert len(pts) == res["points"]
    for i in range(5):
        for rel in ("%d/IMG_%04d_fused.pfm" % (i % 2, i), "%d/mask/IMG_%04d_final.png" % (i % 2, i)):
            assert open(os.path.join(out_cli, rel), "rb").read() == open(os.path.join(out_api, rel), "rb").read(), rel
    # the points of the reference view (0, nadir) lie on the analytic surface: world coordinates through image_info.txt's poses
    z = pts["z"] - OFFSET[2]
    heights = np.array([0.0] + [b[4] for b in fusion_synth.BOXES])
    assert np.mean(np.min(np.abs(z[:, None] - heights[None, :]), 1) < 0.05) > 0.5
