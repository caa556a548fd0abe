"""Depth-map fusion, host side (no GPU): PLY writer, folder discovery, fp64 transform assembly, the fp64 restatement
(tests/fusion_ref.py) against an analytic scene, and argument errors of the C ABI."""
import ctypes
import os

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, fusion, fusion_synth
from conftest import ROOT  # noqa: F401
from fusion_ref import interior, patch, restate, ties, visible_sources


# ---- PLY -------------------------------------------------------------------------------------------------------------
def test_ply_header_bytes_and_streamed_count(tmp_path):
    assert fusion.ply_header(7) == (b"ply\nformat binary_little_endian 1.0\nelement vertex 0000000007\nproperty double x\n"
                                    b"property double y\nproperty double z\nproperty uchar red\nproperty uchar green\n"
                                    b"property uchar blue\nend_header\n")
    assert fusion.PLY_DTYPE.itemsize == 27
    rng = np.random.default_rng(0)
    chunks = [(rng.normal(size=(n, 3)) * 1e6, rng.integers(0, 256, (n, 3)).astype(np.uint8)) for n in (5, 0, 11, 3)]
    path = str(tmp_path / "c.ply")
    with fusion.PlyWriter(path) as w:
        for xyz, rgb in chunks:
            w.write(xyz, rgb)
    data = open(path, "rb").read()
    assert data.startswith(fusion.ply_header(19))
    rec = np.frombuffer(data[len(fusion.ply_header(19)):], fusion.PLY_DTYPE)
    assert len(rec) == 19
    xyz = np.concatenate([c[0] for c in chunks])
    rgb = np.concatenate([c[1] for c in chunks])
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), xyz)
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), rgb)
    assert np.array_equal(fusion.read_ply(path), rec)


# ---- folder discovery ------------------------------------------------------------------------------------------------
def _write_data_folder(root, ids, pairs):
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "camera_info.txt"), "w") as f:
        f.write("# cameras\n0 320 256 0.01 590 590 160 128 0 0 0 0 0\n")
    with open(os.path.join(root, "image_info.txt"), "w") as f:
        for i in ids:
            f.write("%d 0 1 0 0 0 -1 0 0 0 -1 %.3f 3400000.5 800 300 800 %d/%d_img.jpg\n" % (i, 500000.0 + i, i % 2, i))
    with open(os.path.join(root, "image_path.txt"), "w") as f:
        f.write("%d\n" % len(ids) + "".join("%d %d_img /imgs/%d.jpg\n" % (i, i, i) for i in ids))
    with open(os.path.join(root, "viewpair.txt"), "w") as f:
        f.write("%d\n" % len(pairs))
        for ref, srcs in pairs:
            f.write("%d\n%d %s\n" % (ref, len(srcs), " ".join("%d 0.5" % s for s in srcs)))


def test_folder_discovery(tmp_path):
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    ids = [0, 1, 2, 3, 4, 5]
    pairs = [(0, [1, 2, 1, 3, 4, 5]), (1, [0]), (2, [3, 3, 2, 0, 1]), (3, []), (4, [5, 0]), (5, [4])]
    _write_data_folder(data, ids, pairs)
    # view_pairs: truncated to num_src after de-duplication, the reference left out, no padding, empty lists dropped
    assert fusion.view_pairs(os.path.join(data, "viewpair.txt"), 4) == [(0, [1, 2, 3, 4]), (1, [0]), (2, [3, 0, 1]), (4, [5, 0]), (5, [4])]
    assert fusion.view_pairs(os.path.join(data, "viewpair.txt"), 2) == [(0, [1, 2]), (1, [0]), (2, [3, 0]), (4, [5, 0]), (5, [4])]
    folder = fusion.Folder(data, out)
    assert fusion.view_key(folder.images[3]) == ("1", "3_img")
    assert folder.base(4) == os.path.join(out, "0", "4_img")
    # maps of every view but 4 (its reference is skipped, and it is dropped from 0's and 5's sources)
    for i in ids:
        if i == 4:
            continue
        b = folder.base(i)
        os.makedirs(os.path.dirname(b), exist_ok=True)
        for ext in ("_init.pfm", "_prob.pfm", ".txt", ".jpg"):
            open(b + ext, "wb").close()
    views, skipped = folder.plan(4)
    assert skipped == [4]
    assert views == [(0, [1, 2, 3]), (1, [0]), (2, [3, 0, 1]), (5, [])]


def test_cam_txt_round_trip(tmp_path):
    from ada_mvs_amd.datasets.data_io import write_red_cam
    cam = np.zeros((2, 4, 4), np.float32)
    cam[0] = np.eye(4)
    cam[0, :3, 3] = (-512345.6, 3401234.5, 812.25)
    cam[1, :3, :3] = [[2351.5, 0, 927.3], [0, 2351.75, 1375.1], [0, 0, 1]]
    cam[1, 3] = (300, 2.5, 192, 780)
    p = str(tmp_path / "v.txt")
    write_red_cam(p, cam, "/x/y.jpg")
    ext, K = fusion.read_cam_txt(p)
    # str() of an fp32 value is its shortest round-trip form: the fp64 parse rounds back to the same fp32
    assert np.array_equal(ext.astype(np.float32), cam[0]) and np.array_equal(K.astype(np.float32), cam[1, :3, :3])


# ---- fp64 transform assembly -----------------------------------------------------------------------------------------
def test_relative_transforms_match_direct_projection_far_from_the_origin():
    off = np.array([5e5, 3.4e6, 800.0])
    cams = fusion_synth.make_cameras(256, 320, 4, offset=off - np.array([0.0, 0.0, 550.0]))
    ref = cams[0]
    assert np.allclose(ref["C"], off)
    rng = np.random.default_rng(1)
    Xw = np.array([off[0], off[1], 0.0]) + rng.uniform(-80, 80, (50, 3)) * [1, 1, 0.3]
    for s in cams[1:]:
        fwd, back = fusion.relative_transforms(ref["K"], ref["R"], ref["C"], s["K"], s["R"], s["C"])
        A, b = fwd[:9].reshape(3, 3), fwd[9:]
        B, c = back[:9].reshape(3, 3), back[9:]
        for X in Xw:
            xr = ref["K"] @ (ref["R"].T @ (X - ref["C"]))
            xs = s["K"] @ (s["R"].T @ (X - s["C"]))
            x, y, d = xr[0] / xr[2], xr[1] / xr[2], xr[2]
            h = d * (A @ [x, y, 1.0]) + b
            assert abs(h[2] - xs[2]) < 1e-6 * xs[2]
            assert np.hypot(h[0] / h[2] - xs[0] / xs[2], h[1] / h[2] - xs[1] / xs[2]) < 1e-6
            u, v = h[0] / h[2], h[1] / h[2]
            q = h[2] * (B @ [u, v, 1.0]) + c
            assert np.hypot(q[0] / q[2] - x, q[1] / q[2] - y) < 1e-6 and abs(q[2] - d) < 1e-6 * d
    # the emit camera: K^-1, R_wc, C -> the world point of a reference pixel
    cam = fusion.emit_camera(ref["K"], ref["R"], ref["C"])
    X = Xw[0]
    xr = ref["K"] @ (ref["R"].T @ (X - ref["C"]))
    Xc = xr[2] * (cam[:9].reshape(3, 3) @ [xr[0] / xr[2], xr[1] / xr[2], 1.0])
    assert np.abs(cam[9:18].reshape(3, 3) @ Xc + cam[18:] - X).max() < 1e-6


# ---- the restatement against the analytic scene ----------------------------------------------------------------------
def _restate_scene(sc, **kw):
    ref_cam = sc["cams"][0]
    srcs = [dict(cam=c, depth=d) for c, d in zip(sc["cams"][1:], sc["depths"][1:])]
    return restate(sc["depths"][0], sc["confs"][0], ref_cam, srcs, rgba=sc["rgba"], keep_uv=True, **kw)


def test_restatement_keeps_the_clean_scene_and_rejects_a_corrupted_patch():
    sc = fusion_synth.scene(128, 160, 4, seed=3)
    sc["confs"][0][:] = 1.0
    out = _restate_scene(sc)
    vis = visible_sources(sc)
    flat = interior(sc, out)
    want = flat & (vis >= 2)
    assert want.sum() > 0.5 * want.size
    assert out["kept"][want].mean() > 0.99
    true_d, _ = fusion_synth.render(sc["cams"][0])
    k = out["kept"] & flat
    assert np.abs(out["fused"][k] - true_d[k]).max() < 1e-5 * true_d[k].max()
    assert np.all(np.isfinite(out["xyz"])) and len(out["xyz"]) == out["kept"].sum()
    # +3 % depth on a patch of the reference: rejected
    bad = sc["depths"][0].copy()
    rows, cols = patch(*bad.shape)
    assert out["kept"][rows, cols].mean() > 0.9
    bad[rows, cols] *= 1.03
    sc2 = dict(sc, depths=[bad] + sc["depths"][1:])
    out2 = _restate_scene(sc2)
    assert not out2["kept"][rows, cols].any()
    assert not ties(out).all()


# ---- C ABI argument errors -------------------------------------------------------------------------------------------
def test_fusion_argument_errors_without_a_gpu():
    lib = _lib.load()
    assert lib.adamvs_fusion_max_sources() == 16
    dummy = ctypes.c_void_p(16)            # never dereferenced: every call below is refused before a launch
    null = ctypes.c_void_p(0)

    def srcs(n, H=8, W=8, depth=dummy, bad=False):
        arr = (_lib.FusionSource * max(n, 1))()
        for i in range(n):
            arr[i].depth, arr[i].H, arr[i].W = depth.value, H, W
            arr[i].fwd[:] = [float("nan") if bad else 0.0] * 12
            arr[i].back[:] = [0.0] * 12
        return arr

    def geo(ref=dummy, H=8, W=8, s=None, N=1, prob=0.5, pix=1.0, rel=0.01, mc=2, count=dummy):
        return lib.adamvs_geo_consistency(ref, dummy, H, W, srcs(N) if s is None else s, N, prob, pix, rel, mc, count, dummy, dummy, null)

    cases = {
        "null reference": geo(ref=null), "null output": geo(count=null), "N = 0": geo(N=0), "N = 17": geo(s=srcs(17), N=17),
        "H = 0": geo(H=0), "W < 0": geo(W=-3), "NaN prob": geo(prob=float("nan")), "inf pix": geo(pix=float("inf")),
        "pix = 0": geo(pix=0.0), "NaN rel": geo(rel=float("nan")), "min_consistent < 0": geo(mc=-1),
        "null source depth": geo(s=srcs(2, depth=null), N=2), "source size 0": geo(s=srcs(1, H=0)),
        "source transform NaN": geo(s=srcs(1, bad=True)),
        "scan null": lib.adamvs_fusion_scan(null, dummy, 4, null), "scan nblocks 0": lib.adamvs_fusion_scan(dummy, dummy, 0, null),
    }
    cam = (ctypes.c_double * 21)(*([1.0] * 21))
    cam_nan = (ctypes.c_double * 21)(*([1.0] * 20 + [float("nan")]))
    cases["emit null"] = lib.adamvs_fusion_emit(null, dummy, 8, 8, cam, dummy, dummy, dummy, 64, null)
    cases["emit capacity"] = lib.adamvs_fusion_emit(dummy, dummy, 8, 8, cam, dummy, dummy, dummy, 63, null)
    cases["emit camera NaN"] = lib.adamvs_fusion_emit(dummy, dummy, 8, 8, cam_nan, dummy, dummy, dummy, 64, null)
    cases["emit H = 0"] = lib.adamvs_fusion_emit(dummy, dummy, 0, 8, cam, dummy, dummy, dummy, 64, null)
    for what, rc in cases.items():
        assert rc < 0, what
        with pytest.raises(_lib.AdaMVSHipError, match="invalid argument"):
            _lib.check(rc, what)
