"""Image orthophoto on the GPU (csrc/ortho.hip through ada_mvs_amd/ortho.py) against the fp64 restatement (tests/ortho_ref.py):
z-buffer depths, visibility, chosen views, colours and counts outside a tie margin; the true-orthophoto property on the analytic
scene (terrain hidden behind buildings is not painted with roofs or walls); the scene far from the origin; run-to-run identity;
holes, a view that sees nothing, odd image sizes, K = 8; and ortho_whu.py at the end of the CLI chain."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import dsm as dsm_mod, fusion_synth, ortho
from conftest import ROOT
import ortho_ref as R
import ortho_scene as S

pytestmark = pytest.mark.gpu

OFFSET = (5e5, 3.4e6, 0.0)
# tie margin: edge decisions within GROW_PX pixels, depth tests within EPS_Z metres, scores within EPS_SCORE
GROW_PX, EPS_Z, EPS_SCORE = 2e-3, 2e-3, 2e-5
# The fp32 rasteriser's barycentrics carry the rounding of u, v (about 2^-24 of the image size) divided by the triangle's size
# in pixels; on the steep wall triangles of the oblique views that is about 1e-6 of the depth (4.4e-6 measured at worst).
ZBUF_RTOL = 2.0 ** -16


def gpu_views(cams):
    return S.views(cams, device="cuda")


def run(z, g, views, K=1, mode="best", keep_zbufs=False, **kw):
    b = ortho.OrthoBuilder(g, K, mode, z, keep_zbufs=keep_zbufs, **kw)
    for v in views:
        b.add_view(v)
    res = b.finish()
    if keep_zbufs:
        res["zbufs"] = {k: v.cpu().numpy().view(np.float32).astype(np.float64) for k, v in b.zbufs.items()}
    return res


def host_views(views):
    return [dict(iid=v["iid"], K=v["K"], R=v["R"], C=v["C"], rgba=v["rgba_h"], cam=v["cam"]) for v in views]


def check_parity(z, g, views, K, mode, max_aside=0.06):
    res = run(z, g, views, K, mode, keep_zbufs=True)
    hv = host_views(views)
    # z-buffers: where the bracketing buffers agree, the GPU's fp32 depth is the fp64 depth within ZBUF_RTOL
    for v in hv:
        if v["iid"] not in res["zbufs"]:
            continue
        H, W = v["rgba"].shape[:2]
        got = res["zbufs"][v["iid"]]
        lo, hi = R.zbuf(g, z, v, H, W, GROW_PX), R.zbuf(g, z, v, H, W, -GROW_PX)
        firm = (lo == hi)
        ref = R.zbuf(g, z, v, H, W)
        assert firm.mean() > 0.9, firm.mean()
        inf = firm & np.isinf(ref)
        assert np.isinf(got[inf]).all()
        fin = firm & np.isfinite(ref)
        err = np.abs(got[fin] - ref[fin]) / ref[fin]
        assert err.max() <= ZBUF_RTOL, "view %d: zbuf relative error %.3g" % (v["iid"], err.max())
    ref = R.compose(g, z, K, [dict(v, rgba=v["rgba"]) for v in hv], mode, zbufs=res["zbufs"], margin=(GROW_PX, EPS_Z, EPS_SCORE))
    keep = ~ref["marginal"]
    aside = 1.0 - keep.mean()
    assert aside <= max_aside, "%.2f %% of the cells set aside" % (100 * aside)
    np.testing.assert_array_equal(res["nvis"][keep], ref["nvis"][keep])
    np.testing.assert_array_equal(res["view"][keep], ref["view"][keep])
    np.testing.assert_array_equal(res["rgba"][keep][:, 3], ref["rgba"][keep][:, 3])
    d = np.abs(res["rgba"][keep][:, :3].astype(int) - ref["rgba"][keep][:, :3].astype(int))
    assert d.max() <= 1
    assert res["cells_surface"] == int((~np.isnan(ref["height"])).sum())
    return res, ref, aside


@pytest.fixture(scope="module")
def scene():
    cams = S.cameras(192, 256)
    z, g = S.dsm_grid()
    return cams, gpu_views(cams), z, g


# ---- 1. parity with the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,mode", [(1, "best"), (1, "feather"), (2, "best"), (2, "feather")])
def test_parity_with_the_restatement(scene, K, mode):
    _, views, z, g = scene
    res, ref, aside = check_parity(z, g, views, K, mode)
    assert (res["rgba"][..., 3] > 0).mean() > 0.9
    print("K=%d %s: %.3f %% of cells set aside by the tie margin" % (K, mode, 100 * aside))


# ---- 2. the true-orthophoto property --------------------------------------------------------------------------------------
def true_ortho_check(res, z, g, views, tol):
    """-> (failures: cells where a view the mosaic used is blocked by a building, clean cells, cells set aside, max R/G error on
    clean cells, B mismatches on clean cells)."""
    ok, X, Y = S.terrain_check_cells(g, 1)
    P = np.stack([X, Y, np.zeros_like(X)], -1)
    rgba = res["rgba"]
    a = ok & (rgba[..., 3] > 0)
    h = R.surface(z, 1)
    fail = np.zeros(ok.shape, bool)
    aside = np.zeros(ok.shape, bool)
    for v in views:
        H, W = v["rgba_h"].shape[:2]
        t = R.view_terms(g, 1, h, v, H, W, 2.0)
        vis = R.visibility(t, res["zbufs"][v["iid"]], tol) & a
        if res["mode"] == "best":
            vis &= res["view"] == v["iid"]
        # the DSM at gsd g lies between the boxes shrunk and grown by g; a z-buffer decides at pixel resolution
        pix = np.sqrt(((P - v["C"]) ** 2).sum(-1)).max() / v["K"][0, 0]
        clear = ~S.segment_hits_boxes(P, v["C"], g.gsd + pix)
        blocked = S.segment_hits_boxes(P, v["C"], -g.gsd - pix)
        nc = np.zeros(ok.shape + (4,), int)
        nc[vis] = S.neighbour_classes(v["cam"], t["u"][vis], t["v"][vis])
        fail |= vis & blocked
        aside |= vis & ((~clear & ~blocked) | ~(nc == S.TERRAIN).all(-1))
    clean = a & ~aside
    r, gg = S.tex_rg(X, Y)
    err = max(np.abs(rgba[..., 0] - r)[clean].max(), np.abs(rgba[..., 1] - gg)[clean].max())
    return fail, clean, a & aside, err, int((clean & (rgba[..., 2] != S.TERRAIN)).sum())


@pytest.mark.parametrize("mode", ["best", "feather"])
def test_true_orthophoto_keeps_roofs_off_hidden_terrain(scene, mode):
    cams, views, z, g = scene
    ok, X, Y = S.terrain_check_cells(g, 1)
    hidden = ok & S.segment_hits_boxes(np.stack([X, Y, np.zeros_like(X)], -1), cams[0]["C"], -g.gsd)
    assert hidden.sum() > 300                       # terrain the nadir camera cannot see: what makes the test meaningful
    res = run(z, g, views, 1, mode, keep_zbufs=True)
    fail, clean, aside, err, bmis = true_ortho_check(res, z, g, views, 2.0 * g.gsd)
    assert fail.sum() == 0, "%d terrain cells coloured from a view a building blocks" % fail.sum()
    assert bmis == 0
    assert err <= 2.0, err
    assert clean.sum() > 0.85 * ok.sum() and aside.sum() < 0.15 * ok.sum()
    # the hidden terrain is coloured from the views that see it
    assert (res["rgba"][hidden, 3] > 0).mean() > 0.95
    # without the occlusion test (an unbounded tolerance) the same check catches roofs and walls painted on the terrain
    res2 = run(z, g, views, 1, mode, keep_zbufs=True, occlusion_tol=1e6)
    fail2 = true_ortho_check(res2, z, g, views, 1e6)[0]
    assert fail2.sum() > 100


# ---- 3. far offset --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["best", "feather"])
def test_far_offset_gives_the_same_rasters(scene, mode):
    _, views, z, g = scene
    cams_o = S.cameras(192, 256, offset=OFFSET)
    z_o, g_o = S.dsm_grid(offset=OFFSET)
    views_o = [dict(v, C=c["C"]) for v, c in zip(views, cams_o)]
    a = run(z, g, views, 2, mode)
    b = run(z_o, g_o, views_o, 2, mode)
    for k in ("rgba", "view", "nvis"):
        np.testing.assert_array_equal(a[k], b[k])


# ---- 4. determinism -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["best", "feather"])
def test_two_runs_are_bit_identical(scene, mode):
    _, views, z, g = scene
    a = run(z, g, views, 2, mode, keep_zbufs=True)
    b = run(z, g, views, 2, mode, keep_zbufs=True)
    for k in ("rgba", "view", "nvis"):
        np.testing.assert_array_equal(a[k], b[k])
    for i in a["zbufs"]:
        np.testing.assert_array_equal(a["zbufs"][i], b["zbufs"][i])


# ---- 5. edge cases --------------------------------------------------------------------------------------------------------
def test_dsm_with_holes_and_filled(scene):
    _, views, z, g = scene
    rng = np.random.default_rng(3)
    zh = z.copy()
    zh[rng.random(z.shape) < 0.03] = np.nan
    zh[100:130, 40:90] = np.nan
    res, ref, _ = check_parity(zh, g, views, 2, "best")
    void = np.isnan(ref["height"])
    assert void.sum() > 0 and (res["rgba"][void] == 0).all() and (res["view"][void] == -1).all() and (res["nvis"][void] == 0).all()
    full = run(z, g, views, 2, "best")
    assert full["cells_surface"] == full["grid"].W * full["grid"].H > res["cells_surface"]


def test_a_view_that_sees_nothing_is_culled_and_reported(scene):
    cams, views, z, g = scene
    away = dict(cams[1])
    away["C"] = cams[1]["C"] + np.array([5000.0, 0.0, 0.0])
    away["R"] = fusion_synth.look_at(away["C"], away["C"] + np.array([1.0, 0.0, 0.2]))      # looks away from the scene
    extra = S.views([away], device="cuda")[0]
    extra["iid"] = 9
    a = run(z, g, views, 1, "best")
    b = run(z, g, views + [extra], 1, "best")
    assert b["views_culled"] == [9] and b["views_used"] == a["views_used"] == [0, 1, 2, 3, 4]
    for k in ("rgba", "view", "nvis"):
        np.testing.assert_array_equal(a[k], b[k])


def test_odd_image_sizes():
    cams = S.cameras(97, 131, 4, src_sizes=[(101, 77), (63, 149), (97, 131), (55, 55)])
    views = gpu_views(cams)
    z, g = S.dsm_grid()
    check_parity(z, g, views, 1, "feather", max_aside=0.12)


def test_upsample_8():
    cams = S.cameras(192, 256)
    views = gpu_views(cams)
    z, g = S.dsm_grid(x0=5.0, y_top=-20.0, W=40, H=32)                 # a crop over the corner of the box at x 18 .. 66, y -72 .. -28
    res, ref, _ = check_parity(z, g, views, 8, "best")
    assert res["grid"].W == 320 and res["grid"].gsd == 0.125


# ---- 6. the CLI chain -----------------------------------------------------------------------------------------------------
def _run(args, timeout=600):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_cli_chain_end_to_end(tmp_path):
    import torch
    sc = fusion_synth.scene(96, 128, 4, seed=2)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    fusion_synth.write_predict_layout(sc, data, out)
    _run([os.path.join(ROOT, "fuse_whu.py"), "--data_folder", data, "--output_folder", out])
    ply = os.path.join(out, "fused.ply")
    args = [os.path.join(ROOT, "dsm_whu.py"), "--ply", ply, "--gsd", "1.0", "--fill_max_dist", "8"]
    _run(args + ["--out", str(tmp_path / "ref" / "d")])
    _run(args + ["--out", str(tmp_path / "d")])
    before = {k: open(p, "rb").read() for k, p in dsm_mod.output_paths(str(tmp_path / "d")).items()}
    _run([os.path.join(ROOT, "ortho_whu.py"), "--data_folder", data, "--output_folder", out, "--dsm", str(tmp_path / "d"), "--filled",
          "--upsample", "2", "--mode", "feather"])
    # the DSM step's files are untouched and equal to a run without the new step
    for k, p in dsm_mod.output_paths(str(tmp_path / "d")).items():
        assert open(p, "rb").read() == before[k]
        if k != "json":
            assert open(p, "rb").read() == open(dsm_mod.output_paths(str(tmp_path / "ref" / "d"))[k], "rb").read()
    for k in ("dsm", "ortho"):
        p = dsm_mod.fill_output_paths(str(tmp_path / "d"))[k]
        assert open(p, "rb").read() == open(dsm_mod.fill_output_paths(str(tmp_path / "ref" / "d"))[k], "rb").read()
    # the CLI's files equal the in-process API's
    got = ortho.read_outputs(str(tmp_path / "d"))
    api = ortho.from_folder(data, out, str(tmp_path / "d"), filled=True, upsample=2, mode="feather", out=str(tmp_path / "api"),
                            device=torch.device("cuda"))
    for a, b in zip(got, ortho.read_outputs(str(tmp_path / "api"))):
        np.testing.assert_array_equal(a, b)
    for a, k in zip(got, ("rgba", "view", "nvis")):
        np.testing.assert_array_equal(a, api[k])
    js = json.load(open(ortho.output_paths(str(tmp_path / "d"))["json"]))
    assert js["mode"] == "feather" and js["upsample"] == 2 and js["views_used"] == [0, 1, 2, 3, 4]
    assert js["cells_coloured"] > 0.8 * js["cells_surface"] > 0
    wf = open(ortho.output_paths(str(tmp_path / "d"))["ortho_world"]).read().split()
    assert float(wf[0]) == 0.5 and float(wf[3]) == -0.5
