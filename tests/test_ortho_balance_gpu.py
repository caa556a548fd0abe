"""The orthophoto's radiometric balance on the GPU (csrc/ortho_balance.hip through ada_mvs_amd/ortho.py) against the restatement
(tests/ortho_balance_ref.py): the pair statistics and the seam statistics exactly, the observations outside the visibility
margin, the image adjustment exactly, and end to end the property a user sees: scaled exposures are recovered and the colour
step across the seams falls back to that of the unscaled images.  The scene is the one of tests/test_ortho_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, fusion, fusion_synth, hip_ops, ortho
from conftest import ROOT
import ortho_balance_ref as B
import ortho_ref as R
import ortho_scene as S

pytestmark = pytest.mark.gpu

OFFSET = (5e5, 3.4e6, 0.0)
GROW_PX, EPS_Z = 2e-3, 2e-3                                          # the visibility margins of tests/test_ortho_gpu.py
MAX_ASIDE = 0.06
CHUNK = _lib.ORTHO_BAL_CHUNK
GAMMA = np.array([0.85, 1.10, 1.00, 0.92, 1.18])


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def build(z, g, views, K=1, mode="best"):
    b = ortho.OrthoBuilder(g, K, mode, z, keep_zbufs=True)
    for v in views:
        b.add_view(v)
    return b, b.finish()


@pytest.fixture(scope="module")
def scene():
    cams = S.cameras(192, 256)
    z, g = S.dsm_grid()
    return cams, S.views(cams, device="cuda"), z, g


@pytest.fixture(scope="module")
def mosaics(scene):
    """The builder and the best mosaic of the unscaled scene at K = 1 and K = 2."""
    _, views, z, g = scene
    return {K: build(z, g, views, K) for K in (1, 2)}


def scaled_views(views, gamma=GAMMA):
    out = []
    for v, gam in zip(views, gamma):
        img = v["rgba_h"].copy()
        img[..., :3] = np.clip(np.floor(gam * img[..., :3].astype(np.float64) + 0.5), 0, 255).astype(np.uint8)
        out.append(dict(v, rgba=dev(img), rgba_h=img))
    return out


# ---- 1. pair statistics ---------------------------------------------------------------------------------------------------
def synthetic_obs(Ns, maxd, seed):
    """obs [4, N_s, 4] uint16: view 1 is view 0 moved by 0, +-maxd or +-(maxd + 1) per channel, view 2 is independent, and
    view 3 is visible only where view 0 is not."""
    rng = np.random.default_rng(seed)
    obs = np.zeros((4, Ns, 4), np.int64)
    obs[..., :3] = rng.integers(0, B.MAX_Q + 1, (4, Ns, 3))
    if maxd == B.MAX_Q:
        obs[0, ::3, :3] = 0                                          # differences of exactly 16320 need the two ends
        obs[1, ::3, :3] = np.where(rng.random((len(obs[1, ::3]), 3)) < 0.5, B.MAX_Q, obs[1, ::3, :3])
    else:
        step = rng.choice([0, maxd, -maxd, maxd + 1, -maxd - 1], (Ns, 3))
        moved = obs[0, :, :3] + step
        inside = (moved >= 0) & (moved <= B.MAX_Q)
        obs[1, :, :3] = np.where(inside, moved, obs[0, :, :3])
    obs[..., 3] = rng.random((4, Ns)) < 0.8
    obs[3, :, 3] &= 1 - obs[0, :, 3]
    obs[..., :3] *= obs[..., 3:]                                     # an unseen cell is (0, 0, 0, 0), as observe writes it
    return obs.astype(np.uint16)


ALL_PAIRS = [(a, b) for a in range(4) for b in range(a + 1, 4)]


@pytest.mark.parametrize("maxd", [0, 64 * 8, B.MAX_Q])
@pytest.mark.parametrize("Ns", [1, 63, 64, 65, 255, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK - 101])
def test_pair_stats_equal_numpy_exactly(Ns, maxd):
    obs = synthetic_obs(Ns, maxd, Ns + maxd)
    ref = B.pair_stats(obs, ALL_PAIRS, maxd)
    d = np.abs(obs[0, :, :3].astype(int) - obs[1, :, :3].astype(int))[(obs[0, :, 3] == 1) & (obs[1, :, 3] == 1)]
    if Ns >= 255:                                                    # the data hold both sides of the bound
        assert (d == maxd).any() and ((d == maxd + 1).any() or maxd == B.MAX_Q) and 0 < ref[0, 0] < Ns
    assert ref[2, 0] == 0 and (ref[2] == 0).all()                    # views 0 and 3 share no cell
    d_obs = dev(obs.view(np.int16))
    got = hip_ops.ortho_pair_stats(d_obs, ALL_PAIRS, maxd).cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(hip_ops.ortho_pair_stats(d_obs, ALL_PAIRS, maxd).cpu().numpy(), got)       # run to run
    # a subset in another order gives the same rows
    sub = [ALL_PAIRS[4], ALL_PAIRS[1]]
    np.testing.assert_array_equal(hip_ops.ortho_pair_stats(d_obs, np.array(sub), maxd).cpu().numpy(), ref[[4, 1]])


def test_pair_stats_without_pairs_and_with_bad_pairs():
    obs = dev(synthetic_obs(300, 512, 0).view(np.int16))
    assert tuple(hip_ops.ortho_pair_stats(obs, np.zeros((0, 2), np.int32), 512).shape) == (0, 7)
    assert tuple(hip_ops.ortho_pair_stats(obs, [], 512).shape) == (0, 7)
    for bad in ([(1, 1)], [(2, 1)], [(0, 4)], [(-1, 2)], [(0, 1), (3, 3)]):
        with pytest.raises(_lib.AdaMVSHipError, match="a < b"):
            hip_ops.ortho_pair_stats(obs, bad, 512)
    with pytest.raises(_lib.AdaMVSHipError, match="max_diff_q"):
        hip_ops.ortho_pair_stats(obs, [(0, 1)], B.MAX_Q + 1)


def test_candidate_pairs_lose_no_pair_with_a_common_cell():
    obs = synthetic_obs(3 * CHUNK - 101, 512, 5)
    obs[2, :, :] = 0
    obs[2, 70:75] = (1, 2, 3, 1)                                     # view 2 is seen in run 1 only
    obs[1, 64:128] = 0                                               # and view 1 not in that run
    got = ortho.candidate_pairs(dev(obs.view(np.int16)))
    assert got.dtype == np.int32 and [tuple(p) for p in got] == sorted(tuple(p) for p in got)
    ref = B.pair_stats(obs, ALL_PAIRS, B.MAX_Q)
    have = {tuple(p) for p in got}
    assert all(p in have for p, s in zip(ALL_PAIRS, ref) if s[0] > 0)
    assert (1, 2) not in have and ((0, 2) in have or (2, 3) in have)


# ---- 2. observations ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def margins(scene):
    """Per view: the bracketing fp64 depth buffers of the visibility margin."""
    _, views, z, g = scene
    return {v["iid"]: (R.zbuf(g, z, v, 192, 256, GROW_PX), R.zbuf(g, z, v, 192, 256, -GROW_PX)) for v in views}


def gpu_observe(b, view, S_):
    import torch
    Ws, Hs = B.lattice_shape(b.grid, S_)
    obs = torch.full((Ws * Hs, 4), -1, device="cuda", dtype=torch.int16)        # the call writes every entry
    cam = ortho.view_camera(view)
    hip_ops.ortho_observe(b.cgrid, b.dsm, hip_ops.ortho_view(cam[0], cam[1].T, cam[2], view["rgba"]), b.zbufs[view["iid"]], S_,
                          b.border_px, b.occlusion_tol, obs)
    return obs.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("S_,shape", [(1, (320, 260)), (3, (107, 87)), (400, (1, 1))])
def test_observe_against_the_restatement(scene, mosaics, margins, S_, shape):
    _, views, z, g = scene
    b = mosaics[1][0]
    assert B.lattice_shape(g, S_) == shape == ortho.lattice_shape(g, S_)
    aside, cells, seen = 0, 0, 0
    for v in views:
        got = gpu_observe(b, v, S_).astype(np.int64)
        zb = b.zbufs[v["iid"]].cpu().numpy().view(np.float32).astype(np.float64)
        hv = dict(iid=v["iid"], K=v["K"], R=v["R"], C=v["C"], rgba=v["rgba_h"])
        ref, marginal = B.observe(g, z, hv, zb, S_, margin=margins[v["iid"]] + (GROW_PX, EPS_Z))
        keep = ~marginal
        aside, cells, seen = aside + int(marginal.sum()), cells + marginal.size, seen + int(ref[keep, 3].sum())
        assert marginal.mean() <= MAX_ASIDE, "view %d: %.2f %% of the cells set aside" % (v["iid"], 100.0 * marginal.mean())
        assert set(np.unique(got[:, 3])) <= {0, 1}
        assert (got[got[:, 3] == 0] == 0).all()
        np.testing.assert_array_equal(got[keep, 3], ref[keep, 3])
        assert np.abs(got[keep, :3] - ref[keep, :3]).max(initial=0) <= 1, "view %d" % v["iid"]
    if S_ < 400:
        assert seen > 0.5 * cells
    print("S=%d: %d of %d cells set aside, %d seen" % (S_, aside, cells, seen))


def test_observe_far_offset_is_bit_identical(scene, mosaics):
    _, views, z, g = scene
    cams_o = S.cameras(192, 256, offset=OFFSET)
    z_o, g_o = S.dsm_grid(offset=OFFSET)
    views_o = [dict(v, C=c["C"]) for v, c in zip(views, cams_o)]
    b_o, _ = build(z_o, g_o, views_o)
    for v, vo in zip(views, views_o):
        for S_ in (1, 3):
            np.testing.assert_array_equal(gpu_observe(mosaics[1][0], v, S_), gpu_observe(b_o, vo, S_))


# ---- 3. adjust ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 37), (192, 256)])
@pytest.mark.parametrize("gain", [(1.0, 1.0, 1.0), (0.5, 1.37, 2.0)])
def test_adjust_image_equals_the_float32_formula(shape, gain):
    rng = np.random.default_rng(shape[0])
    img = rng.integers(0, 256, shape + (4,)).astype(np.uint8)
    img.reshape(-1, 4)[:256, :3] = np.arange(256, dtype=np.uint8)[:, None][:min(256, img.shape[0] * img.shape[1])]     # every level
    got = hip_ops.ortho_adjust_image(dev(img), gain).cpu().numpy()
    ref = B.adjust(img, gain)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got[..., 3], img[..., 3])
    if gain == (1.0, 1.0, 1.0):
        np.testing.assert_array_equal(got, img)
    else:
        assert (got[..., 2] == 255).sum() > (img[..., 2] == 255).sum() and got[..., 0].max() <= 128
    with pytest.raises(_lib.AdaMVSHipError):
        hip_ops.ortho_adjust_image(dev(img), (1.0, 0.0, 1.0))


# ---- 4. seam statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 300), (7, 13), (300, 1), (67, 259)])
def test_seam_stats_equal_numpy_on_small_mosaics(H, W):
    rng = np.random.default_rng(H * W)
    view = rng.integers(-1, 4, (H, W)).astype(np.int32)             # -1: holes
    rgba = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    got = hip_ops.ortho_seam_stats(hip_ops.ortho_grid(0.0, 0.0, 1.0, W, H, 1), dev(view), dev(rgba)).cpu().numpy()
    ref = B.seam_stats(view, rgba)
    np.testing.assert_array_equal(got, ref)
    assert (H * W == 1) == (ref[0] == 0)


@pytest.mark.parametrize("K", [1, 2])
def test_seam_stats_equal_numpy_on_the_scene(scene, mosaics, K):
    _, _, _, g = scene
    b, res = mosaics[K]
    ref = B.seam_stats(res["view"], res["rgba"])
    got = hip_ops.ortho_seam_stats(b.cgrid, b.mosaic[1], b.mosaic[0]).cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    assert ref[0] > 100
    rms, pairs = ortho.seam_rms(res)
    assert pairs == ref[0] and rms == np.sqrt(ref[1:].sum() / (3.0 * ref[0])) == B.seam_rms(res["view"], res["rgba"])[0]


# ---- 5. end to end --------------------------------------------------------------------------------------------------------
def terrain_seam(res, g):
    """The rms colour step across the seams on R and G between terrain cells at least 3 DSM cells from every box."""
    ok, _, _ = S.terrain_check_cells(g, 1, 3.0)
    return B.seam_rms(res["view"], res["rgba"], ok, (0, 1))[0]


def test_scaled_exposures_are_recovered_and_the_seams_close(scene, mosaics):
    """gamma = (0.85, 1.10, 1.00, 0.92, 1.18) on the images.  With a weak prior (gain_sigma = 10) g gamma is constant over the
    views to 0.005 (R, G) and 0.02 (B, whose 220 x 1.18 clips) and the seam step is that of the unscaled images within 10 %;
    with the default prior (0.1) the seam step is below half that of the unbalanced mosaic."""
    _, views, z, g = scene
    sv = scaled_views(views)
    gains, rep = ortho.balance_views(z, g, sv, stride=1, gain_sigma=10.0)
    gg = np.stack([gains[v["iid"]] for v in sv]) * GAMMA[:, None]
    dev_ = np.abs(gg / gg.mean(0) - 1.0).max(0)
    print("g gamma / mean - 1: max |.| per channel", dev_, "overlap rms", rep["overlap_rms_before"], "->", rep["overlap_rms_after"])
    assert rep["stride"] == 1 and rep["samples"] == 320 * 260 and rep["pairs_used"] == rep["pairs_candidate"] == 10
    assert dev_[0] <= 0.005 and dev_[1] <= 0.005 and dev_[2] <= 0.02, dev_
    unscaled = terrain_seam(mosaics[1][1], g)
    plain = terrain_seam(ortho.from_dsm(z, g, sv), g)
    weak = ortho.from_dsm(z, g, sv, balance="gain", gain_sigma=10.0)
    stiff = ortho.from_dsm(z, g, sv, balance="gain")
    s_weak, s_stiff = terrain_seam(weak, g), terrain_seam(stiff, g)
    print("seam rms (R, G; terrain): unscaled %.3f, scaled %.3f, balanced sigma 10: %.3f, sigma 0.1: %.3f"
          % (unscaled, plain, s_weak, s_stiff))
    assert plain > 3.0 * unscaled                                    # the scaling is what the balance has to undo
    assert s_weak <= 1.1 * unscaled, (s_weak, unscaled)
    assert s_stiff < 0.5 * plain, (s_stiff, plain)
    # the report of from_dsm: the same gains as balance_views, and the seam statistics of its own mosaic
    assert weak["balance"]["gains"] == rep["gains"] and weak["balance"]["stride"] == 1
    for res in (weak, stiff):
        ref = B.seam_stats(res["view"], res["rgba"])
        assert res["balance"]["seam_pairs"] == ref[0] and res["balance"]["seam_rms"] == np.sqrt(ref[1:].sum() / (3.0 * ref[0]))
        assert res["views_used"] == [0, 1, 2, 3, 4] and res["balance"]["model"] == "gain"
    json.dumps(ortho.summary(weak))


def test_views_with_equal_images_get_gains_of_one(scene):
    """Every view carries the same image, of one colour: whatever the cameras, two views observe the same colour in every common
    cell, the means of every pair are equal and the solve has nothing to correct.  (The scene's own unscaled images are not equal
    in this sense: each view samples the texture at its own pixel positions and sees walls the others do not, and the fp64
    restatement gives them max |g - 1| = 1.6e-3 at gain_sigma = 0.1; the figure of the GPU is printed.)"""
    _, views, z, g = scene
    img = np.empty((192, 256, 4), np.uint8)
    img[...] = (100, 150, 200, 255)
    same = dev(img)
    for sigma in (0.1, 10.0):
        gains, rep = ortho.balance_views(z, g, [dict(v, rgba=same) for v in views], gain_sigma=sigma)
        dev_ = max(np.abs(np.asarray(x) - 1.0).max() for x in gains.values())
        assert sorted(gains) == [0, 1, 2, 3, 4] and rep["pairs_used"] == 10 and dev_ <= 1e-3, dev_
        assert max(rep["overlap_rms_before"]) == 0.0
    gains, _ = ortho.balance_views(z, g, views)
    print("the scene's unscaled images: max |g - 1| = %.2e" % max(np.abs(np.asarray(x) - 1.0).max() for x in gains.values()))


def test_a_culled_view_gets_gain_one_and_is_reported(scene):
    cams, views, z, g = scene
    away = dict(cams[1])
    away["C"] = cams[1]["C"] + np.array([5000.0, 0.0, 0.0])
    away["R"] = fusion_synth.look_at(away["C"], away["C"] + np.array([1.0, 0.0, 0.2]))
    extra = S.views([away], device="cuda")[0]
    extra["iid"] = 9
    sv = scaled_views(views)
    a = ortho.from_dsm(z, g, sv, balance="gain")
    b = ortho.from_dsm(z, g, sv + [extra], balance="gain", zbuf_cache_bytes=0)             # and every depth buffer rebuilt
    assert b["views_culled"] == [9] and b["balance"]["gains"]["9"] == [1.0, 1.0, 1.0]
    assert {k: v for k, v in b["balance"]["gains"].items() if k != "9"} == a["balance"]["gains"]
    for k in ("rgba", "view", "nvis"):
        np.testing.assert_array_equal(a[k], b[k])


# ---- 6. nothing changes without the option; the CLI -----------------------------------------------------------------------
@pytest.mark.parametrize("K,mode", [(1, "best"), (2, "feather")])
def test_from_dsm_without_balance_is_unchanged(scene, K, mode):
    _, views, z, g = scene
    _, direct = build(z, g, views, K, mode)
    res = ortho.from_dsm(z, g, views, K, mode)
    assert "balance" not in res and "balance" not in ortho.summary(res)
    assert sorted(set(res) - {"seconds"}) == sorted(direct)
    for k in ("rgba", "view", "nvis"):
        np.testing.assert_array_equal(res[k], direct[k])


def _run(args, timeout=600):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_cli_writes_the_balance_block(tmp_path):
    import torch
    sc = fusion_synth.scene(96, 128, 4, seed=2)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    fusion_synth.write_predict_layout(sc, data, out)
    _run([os.path.join(ROOT, "fuse_whu.py"), "--data_folder", data, "--output_folder", out])
    _run([os.path.join(ROOT, "dsm_whu.py"), "--ply", os.path.join(out, "fused.ply"), "--gsd", "1.0", "--fill_max_dist", "8", "--out",
          str(tmp_path / "d")])
    common = [os.path.join(ROOT, "ortho_whu.py"), "--data_folder", data, "--output_folder", out, "--dsm", str(tmp_path / "d"), "--filled"]
    _run(common + ["--out", str(tmp_path / "bal"), "--balance", "gain", "--gain_sigma", "0.5", "--balance_stride", "2"])
    ortho.from_folder(data, out, str(tmp_path / "d"), filled=True, out=str(tmp_path / "plain"), device=torch.device("cuda"), log=lambda *a: None)
    plain = json.load(open(ortho.output_paths(str(tmp_path / "plain"))["json"]))
    js = json.load(open(ortho.output_paths(str(tmp_path / "bal"))["json"]))
    assert "balance" not in plain and {k: v for k, v in js.items() if k not in ("balance", "seconds", "device_seconds")} == \
        {k: v for k, v in plain.items() if k not in ("seconds", "device_seconds")}
    bal = js["balance"]
    assert bal["model"] == "gain" and bal["gain_sigma"] == 0.5 and bal["noise_sigma"] == 10.0 and bal["stride"] == 2
    assert sorted(bal["gains"]) == [str(i) for i in js["views_used"]] and bal["pairs_used"] >= 1 and bal["seam_pairs"] > 0
    dsm, grid = ortho.read_dsm(str(tmp_path / "d"), filled=True)
    assert bal["samples"] == int(np.prod(ortho.lattice_shape(grid, 2)))
    views = ortho.load_views(fusion.Folder(data, out), torch.device("cuda"))
    gains, rep = ortho.balance_views(dsm, grid, views, stride=2, gain_sigma=0.5)
    assert rep["gains"] == bal["gains"] and {str(k): list(v) for k, v in gains.items()} == bal["gains"]
    rgba, view, _ = ortho.read_outputs(str(tmp_path / "bal"))
    ref = B.seam_stats(view, rgba)
    assert bal["seam_pairs"] == ref[0] and bal["seam_rms"] == np.sqrt(ref[1:].sum() / (3.0 * ref[0]))
