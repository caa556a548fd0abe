"""Mesh texturing on the GPU (csrc/texture.hip through ada_mvs_amd/texture.py) against the fp64 restatement
(tests/texture_ref.py): z-buffers, labels and visible-view counts outside a tie margin, charts, boxes and placements, every
atlas texel and the texture coordinates; the true-texture property on the analytic mesh (tests/texture_scene.py); the scene
far from the origin; run-to-run identity of the written files; edge cases; and texture_whu.py at the end of the CLI chain."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import fusion_synth, mesh as mesh_mod, texture
from conftest import ROOT
import ortho_scene as OS
import texture_ref as R
import texture_scene as S

pytestmark = pytest.mark.gpu

OFFSET = (5e5, 3.4e6, 0.0)
# the images hold 1.2 .. 1.6 m of ground per pixel: the depth test needs a tolerance of about one pixel's depth change
TOL, BORDER, PAD, PAGE = 1.0, 2.0, 2, 1024
# tie margin: edge decisions within GROW_PX pixels, depth tests within EPS_Z metres, scores within EPS_SCORE (relative) and the
# front-facing sign within EPS_AREA of the area's scale
GROW_PX, EPS_Z, EPS_SCORE, EPS_AREA = 2e-3, 2e-3, 2e-5, 1e-6
ZBUF_RTOL = 2.0 ** -16


def run(xyz, rgb, faces, views, **kw):
    args = dict(occlusion_tol=TOL, border_px=BORDER, pad=PAD, page=PAGE)
    args.update(kw)
    return texture.texture_mesh(xyz, rgb, faces, views, **args)


def host_views(views):
    return [dict(iid=v["iid"], K=v["K"], R=v["R"], C=v["C"], rgba=v["rgba_h"], cam=v["cam"]) for v in views]


@pytest.fixture(scope="module")
def scene():
    cams = OS.cameras(192, 256)
    views = OS.views(cams, device="cuda")
    xyz, rgb, faces, cls, box = S.mesh()
    res = run(xyz, rgb, faces, views, keep_zbufs=True)
    return dict(cams=cams, views=views, hv=host_views(views), xyz=xyz, rgb=rgb, faces=faces, cls=cls, box=box, res=res)


def sizes(hv):
    return [v["rgba"].shape[1] for v in hv], [v["rgba"].shape[0] for v in hv]


# ---- 1. z-buffers ---------------------------------------------------------------------------------------------------------
def test_zbuf_matches_the_restatement(scene):
    res = scene["res"]
    assert sorted(res["zbufs"]) == [0, 1, 2, 3, 4]
    for v in scene["hv"]:
        H, W = v["rgba"].shape[:2]
        u, vv, z = R.project(v, scene["xyz"])
        got = res["zbufs"][v["iid"]]
        lo, hi = R.zbuf(u, vv, z, scene["faces"], H, W, GROW_PX), R.zbuf(u, vv, z, scene["faces"], H, W, -GROW_PX)
        firm = lo == hi
        ref = R.zbuf(u, vv, z, scene["faces"], H, W)
        assert firm.mean() > 0.9, firm.mean()
        assert np.isinf(got[firm & np.isinf(ref)]).all()
        fin = firm & np.isfinite(ref)
        err = np.abs(got[fin] - ref[fin]) / ref[fin]
        assert err.max() <= ZBUF_RTOL, "view %d: zbuf relative error %.3g" % (v["iid"], err.max())


# ---- 2. labels and visible-view counts ---------------------------------------------------------------------------------------
def test_labels_and_nvis_match_outside_the_tie_margin(scene):
    res = scene["res"]
    ref = R.labels(scene["xyz"], scene["faces"], scene["hv"], TOL, BORDER, res["zbufs"], (GROW_PX, EPS_Z, EPS_SCORE, EPS_AREA))
    keep = ~ref["marginal"]
    assert 1.0 - keep.mean() <= 0.06, "%.2f %% of the faces set aside" % (100 * (1 - keep.mean()))
    np.testing.assert_array_equal(res["label"][keep], ref["label"][keep])
    np.testing.assert_array_equal(res["nvis"][keep], ref["nvis"][keep])
    tex = keep & (ref["label"] >= 0)
    assert np.abs(res["uv"][tex] - ref["uv"][tex]).max() < 1e-2
    assert (res["label"] >= 0).mean() > 0.5


# ---- 3. charts, boxes, placements ------------------------------------------------------------------------------------------
def test_charts_boxes_and_placements_equal_the_restatement(scene):
    res = scene["res"]
    parent = R.components(res["label"], scene["faces"])
    np.testing.assert_array_equal(res["parent"], parent)
    Ws, Hs = sizes(scene["hv"])
    chart, table = R.charts(res["label"], parent, res["uv"], Ws, Hs, PAD)
    np.testing.assert_array_equal(res["chart"], chart)
    assert res["charts_count"] == len(table)
    np.testing.assert_array_equal(res["charts"][:, [0, 1, 2, 3, 7]], table[:, :5])
    items = [(int(w), int(h)) for w, h in table[:, 2:4]]
    n_u = res["faces_untextured"]
    if n_u:
        items.append((min(n_u, PAGE), -(-n_u // PAGE)))
    place, pages = R.shelf_pack(items, PAGE)
    assert res["pages"] == pages
    np.testing.assert_array_equal(res["charts"][:, 4:7], np.array(place[:len(table)]).reshape(-1, 3))
    if n_u:
        assert tuple(res["palette"][:3]) == place[-1]
    # every corner of every textured face lies inside its chart's box, so every bilinear tap does
    tex = res["label"] >= 0
    c = res["charts"][res["chart"][tex]]
    U, V = res["uv"][tex][:, 0::2], res["uv"][tex][:, 1::2]
    assert (U.min(1) >= c[:, 0]).all() and (U.max(1) <= c[:, 0] + c[:, 2] - 1).all()
    assert (V.min(1) >= c[:, 1]).all() and (V.max(1) <= c[:, 1] + c[:, 3] - 1).all()


# ---- 4. atlas texels and texture coordinates ---------------------------------------------------------------------------
def atlas_property(res, hv, faces, rgb, points=16, seed=0):
    """The atlas sampled at interpolated (s, t) equals the chosen image's bilinear sample at the interpolated (u, v)."""
    tex = np.nonzero(res["label"] >= 0)[0]
    rng = np.random.default_rng(seed)
    w = rng.dirichlet((1.0, 1.0, 1.0), size=(len(tex), points))          # [n, points, 3]
    tc, uv = res["tc"][tex].astype(np.float64), res["uv"][tex].astype(np.float64)
    s = (w * tc[:, None, 0::2]).sum(-1)
    t = (w * tc[:, None, 1::2]).sum(-1)
    u = (w * uv[:, None, 0::2]).sum(-1)
    v = (w * uv[:, None, 1::2]).sum(-1)
    worst = 0.0
    for vi in np.unique(res["label"][tex]):
        sel = res["label"][tex] == vi
        img = np.asarray(hv[vi]["rgba"])
        want = R.bilinear(img, u[sel], v[sel])
        got = np.zeros_like(want)
        pages = res["texnum"][tex][sel]
        for pg in np.unique(pages):
            m = pages == pg
            got[m] = R.sample_atlas(res["atlas"], pg, s[sel][m], t[sel][m])
        worst = max(worst, float(np.abs(got - want).max()))
    return worst


def test_atlas_texels_and_texture_coordinates(scene):
    res = scene["res"]
    pal = np.nonzero(res["label"] < 0)[0]
    table = np.concatenate([res["charts"][:, :4], res["charts"][:, 7:8], np.zeros((len(res["charts"]), 1), np.int64)], 1)
    want = R.atlas(table, [tuple(p) for p in res["charts"][:, 4:7]], scene["hv"], PAGE, res["pages"],
                   tuple(res["palette"][:3]) if len(pal) else None, pal, scene["rgb"], scene["faces"])
    # chart texels are their image texels, the palette texels the rounded vertex means, every other texel 0
    np.testing.assert_array_equal(res["atlas"], want)
    # texture coordinates: the fp32 rule
    tex = res["label"] >= 0
    c = res["charts"][res["chart"][tex]]
    for k in range(3):
        s, t = texture.tex_coords(res["uv"][tex][:, 2 * k], res["uv"][tex][:, 2 * k + 1], c[:, 0], c[:, 1], c[:, 4], c[:, 5], PAGE)
        np.testing.assert_array_equal(res["tc"][tex][:, 2 * k], s)
        np.testing.assert_array_equal(res["tc"][tex][:, 2 * k + 1], t)
    np.testing.assert_array_equal(res["texnum"][tex], c[:, 6])
    if len(pal):
        ox, oy, pg = res["palette"][:3]
        k = np.arange(len(pal))
        np.testing.assert_array_equal(res["tc"][pal][:, 0], ((ox + k % PAGE + 0.5) / PAGE).astype(np.float32))
        np.testing.assert_array_equal(res["texnum"][pal], pg)
    assert atlas_property(res, scene["hv"], scene["faces"], scene["rgb"]) <= 1.0


# ---- 5. the true-texture property ------------------------------------------------------------------------------------------
def tap_faces(cam, u, v):
    """fusion_synth face ids of the four pixels a bilinear sample at (u, v) reads -> [n, 4]."""
    xa, ya = np.floor(u), np.floor(v)
    xb, yb = np.minimum(xa + 1, cam["W"] - 1), np.minimum(ya + 1, cam["H"] - 1)
    return np.stack([fusion_synth.cast(cam, px, py)[1] for px, py in ((xa, ya), (xb, ya), (xa, yb), (xb, yb))], -1)


def test_true_texture_on_the_analytic_scene(scene):
    res, hv, xyz, faces = scene["res"], scene["hv"], scene["xyz"], scene["faces"]
    tex = np.nonzero(res["label"] >= 0)[0]
    # every chosen view sees the face's front side (fp64)
    n = S.normals(xyz, faces)[tex]
    C = np.stack([hv[l]["C"] for l in res["label"][tex]])
    assert ((n * (C - xyz[faces[tex, 0].astype(np.int64)])).sum(1) > 0).all()
    # terrain wholly under a box is untextured
    hidden = S.under_a_box(xyz, faces)
    assert hidden.sum() > 1000
    assert (res["label"][hidden] == -1).all()
    # at the screen centroid, where the four taps see one planar face of the face's class: B is that class, R and G follow the
    # world position
    ok = tot = 0
    rg_err = 0.0
    for vi in np.unique(res["label"][tex]):
        f = tex[res["label"][tex] == vi]
        cam = hv[vi]["cam"]
        uc, vc = res["uv"][f][:, 0::2].mean(1).astype(np.float64), res["uv"][f][:, 1::2].mean(1).astype(np.float64)
        taps = tap_faces(cam, uc, vc)
        clean = (OS.face_class(taps) == scene["cls"][f][:, None]).all(1) & (taps == taps[:, :1]).all(1)
        sc, tcc = res["tc"][f][:, 0::2].mean(1), res["tc"][f][:, 1::2].mean(1)
        got = np.zeros((len(f), 3))
        for pg in np.unique(res["texnum"][f]):
            m = res["texnum"][f] == pg
            got[m] = R.sample_atlas(res["atlas"], pg, sc[m], tcc[m])
        tot += int(clean.sum())
        ok += int((np.abs(got[clean, 2] - scene["cls"][f][clean]) < 0.5).sum())
        depth, _ = fusion_synth.cast(cam, uc[clean], vc[clean])
        ray = np.stack([uc[clean], vc[clean], np.ones(clean.sum())], 1) @ np.linalg.inv(cam["K"]).T
        P = (ray * depth[:, None]) @ cam["R"].T + (cam["C"] - cam["offset"])
        r, g = OS.tex_rg(P[:, 0], P[:, 1])
        # the image stores rounded levels and the atlas sample blends up to four of them
        rg_err = max(rg_err, float(np.abs(got[clean, 0] - r).max()), float(np.abs(got[clean, 1] - g).max()))
    assert tot > 0.5 * len(tex)
    assert ok >= 0.99 * tot, "%d of %d clean faces sample their own class" % (ok, tot)
    assert rg_err <= 3.0, rg_err


# ---- 6. far from the origin ------------------------------------------------------------------------------------------------
def test_far_offset_gives_bit_identical_results(scene):
    cams = OS.cameras(192, 256, offset=OFFSET)
    xyz, rgb, faces, _, _ = S.mesh(offset=OFFSET)
    res = run(xyz, rgb, faces, OS.views(cams, device="cuda"))
    for k in ("label", "nvis", "parent", "chart", "charts", "atlas", "tc", "texnum"):
        np.testing.assert_array_equal(res[k], scene["res"][k], err_msg=k)


# ---- 7. run to run ------------------------------------------------------------------------------------------------------
def test_two_runs_write_identical_bytes(scene, tmp_path):
    verts = np.zeros(len(scene["xyz"]), mesh_mod.fusion.PLY_DTYPE)
    verts["x"], verts["y"], verts["z"] = scene["xyz"].T
    verts["red"], verts["green"], verts["blue"] = scene["rgb"].T
    out = []
    for k in range(2):
        res = run(scene["xyz"], scene["rgb"], scene["faces"], scene["views"])
        paths = texture.write_outputs(str(tmp_path / ("r%d" % k) / "m"), verts, scene["faces"], res)
        out.append([open(p, "rb").read() for p in [paths["ply"]] + paths["pages"]])
    assert len(out[0]) == len(out[1]) >= 2
    for a, b in zip(*out):
        assert a == b
    back = texture.read_textured_ply(str(tmp_path / "r0" / "m.ply"))
    np.testing.assert_array_equal(back["tc"], scene["res"]["tc"])
    assert back["tex_files"] == ["m_tex_%04d.png" % k for k in range(scene["res"]["pages"])]


# ---- 8. edge cases --------------------------------------------------------------------------------------------------------
def test_a_view_that_sees_nothing_is_culled(scene):
    cams = OS.cameras(192, 256)
    away = dict(cams[0])
    away["R"] = fusion_synth.look_at((0.0, 0.0, 550.0), (0.0, 0.0, 2000.0))
    views = OS.views(cams[:1] + [away] + cams[1:], device="cuda")
    res = run(scene["xyz"], scene["rgb"], scene["faces"], views)
    assert res["views_culled"] == [1] and res["views_used"] == [0, 2, 3, 4, 5]
    lab = np.where(scene["res"]["label"] >= 1, scene["res"]["label"] + 1, scene["res"]["label"])
    np.testing.assert_array_equal(res["label"], lab)
    np.testing.assert_array_equal(res["atlas"], scene["res"]["atlas"])


def test_one_face_mesh(scene):
    xyz = np.array([[-10.0, -10.0, 0.0], [10.0, -10.0, 0.0], [0.0, 10.0, 0.0]])
    rgb = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 91]], np.uint8)
    res = run(xyz, rgb, np.array([[0, 1, 2]], np.uint32), scene["views"])
    assert res["faces_textured"] == 1 and res["charts_count"] == 1 and res["pages"] == 1
    assert res["nvis"][0] >= 1
    assert atlas_property(res, scene["hv"], None, rgb) <= 1.0


def test_face_behind_the_camera_and_untextured_palette(scene):
    xyz = np.array([[-10.0, -10.0, 0.0], [10.0, -10.0, 0.0], [0.0, 10.0, 0.0],
                    [-10.0, -10.0, 600.0], [0.0, 10.0, 600.0], [10.0, -10.0, 600.0]])
    rgb = np.array([[0, 0, 0], [3, 3, 3], [6, 6, 7], [10, 20, 30], [40, 50, 60], [70, 80, 91]], np.uint8)
    res = run(xyz, rgb, np.array([[0, 1, 2], [3, 4, 5]], np.uint32), scene["views"][:1], keep_zbufs=True)
    assert list(res["label"]) == [0, -1] and list(res["nvis"]) == [1, 0]
    u, v, z = R.project(scene["hv"][0], xyz[:3])
    np.testing.assert_allclose(res["zbufs"][0][np.isfinite(res["zbufs"][0])].max(), 550.0, rtol=1e-4)
    ox, oy, pg = res["palette"][:3]
    np.testing.assert_array_equal(res["atlas"][pg, oy, ox], [40, 50, 60])      # (10+40+70+1)//3, (20+50+80+1)//3, (30+60+91+1)//3
    assert res["tc"][1, 0] == res["tc"][1, 2] == res["tc"][1, 4]


def test_non_manifold_edge_connects_equal_labels():
    import torch
    from ada_mvs_amd import hip_ops
    # three faces on the edge (0, 1) labelled 1, 2, 1, and a fourth face of label 1 on the edge (1, 2) of face 2 only
    faces = torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4], [4, 1, 5]], dtype=torch.int32, device="cuda")
    want = {(1, 2, 1, 1): [0, 1, 0, 0], (2, 1, 1, 2): [0, 1, 1, 3], (1, 1, 2, 1): [0, 0, 2, 3]}
    for lab in want:
        label = torch.tensor(lab, dtype=torch.int32, device="cuda")
        keys = hip_ops.texture_edge_keys(faces)
        p1 = torch.sort(label.repeat_interleave(3), stable=True).indices
        ks, p2 = torch.sort(keys[p1], stable=True)
        parent = torch.arange(4, dtype=torch.int32, device="cuda")
        changed = torch.zeros(1, dtype=torch.int32, device="cuda")
        for _ in range(8):
            hip_ops.texture_components_round(ks, p1[p2].contiguous(), label, parent, changed)
            if int(changed.item()) == 0:
                break
        np.testing.assert_array_equal(parent.cpu().numpy(), R.components(np.array(lab), faces.cpu().numpy()))
        assert list(parent.cpu().numpy()) == want[lab]
    # strips whose 3 nf edges end inside the first tile of 256 lanes, in the second and in the third, two vertex numbers with bit 31
    # set: one chart, charts of seven faces with untextured faces between them, and the roots after the guarded walk
    import smooth_inputs as SI
    for nf in SI.EDGE_TILE_FACES:
        big, bits = SI.renamed_strip_faces(nf)
        faces = torch.from_numpy(bits).cuda()
        keys = hip_ops.texture_edge_keys(faces)
        for lab in (np.zeros(nf, np.int64), np.where(np.arange(nf) % 8 == 7, -1, (np.arange(nf) // 8) % 2)):
            label = torch.from_numpy(lab.astype(np.int32)).cuda()
            p1 = torch.sort(label.repeat_interleave(3), stable=True).indices
            ks, p2 = torch.sort(keys[p1], stable=True)
            parent = torch.arange(nf, dtype=torch.int32, device="cuda")
            changed = torch.ones(1, dtype=torch.int32, device="cuda")
            for _ in range(64):
                if int(changed.item()) == 0:
                    break
                hip_ops.texture_components_round(ks, p1[p2].contiguous(), label, parent, changed)
            assert int(changed.item()) == 0
            np.testing.assert_array_equal(parent.cpu().numpy(), R.components(lab, big))
            assert len(np.unique(parent.cpu().numpy())) == (1 if lab.max() == 0 else len(np.unique(np.arange(nf) // 8)) + (lab < 0).sum())


def test_odd_image_sizes():
    cams = OS.cameras(97, 131)
    views = OS.views(cams, device="cuda")
    xyz, rgb, faces, _, _ = S.mesh(terrain_step=2.0)
    # about 2.6 m of ground per pixel: a tolerance of about one pixel's depth change
    res = run(xyz, rgb, faces, views, keep_zbufs=True, occlusion_tol=3.0)
    hv = host_views(views)
    ref = R.labels(xyz, faces, hv, 3.0, BORDER, res["zbufs"], (GROW_PX, EPS_Z, EPS_SCORE, EPS_AREA))
    keep = ~ref["marginal"]
    assert keep.mean() >= 0.92
    np.testing.assert_array_equal(res["label"][keep], ref["label"][keep])
    assert atlas_property(res, hv, faces, rgb) <= 1.0


def test_a_page_smaller_than_an_image_is_refused(scene):
    import torch
    views = [dict(iid=0, K=scene["hv"][0]["K"], R=scene["hv"][0]["R"], C=scene["hv"][0]["C"],
                  rgba=torch.zeros(600, 1030, 4, dtype=torch.uint8, device="cuda"))]
    with pytest.raises(ValueError, match="smaller than the largest image side 1030"):
        run(scene["xyz"], scene["rgb"], scene["faces"], views)
    with pytest.raises(ValueError, match="out of range"):
        run(scene["xyz"][:10], scene["rgb"][:10], scene["faces"], scene["views"])


def test_unwelded_mesh_splits_charts_and_stays_exact(scene):
    xyz, rgb, faces = scene["xyz"], scene["rgb"], scene["faces"].astype(np.int64)
    nv = len(xyz)
    # a seam at x = 0: faces whose first vertex lies east of it use a copy of every vertex, as two bricks would write them
    east = xyz[faces[:, 0], 0] >= 0.0
    f2 = np.where(east[:, None], faces + nv, faces).astype(np.uint32)
    res = run(np.concatenate([xyz, xyz]), np.concatenate([rgb, rgb]), f2, scene["views"])
    np.testing.assert_array_equal(res["label"], scene["res"]["label"])
    np.testing.assert_array_equal(res["uv"], scene["res"]["uv"])
    assert res["charts_count"] > scene["res"]["charts_count"]
    assert atlas_property(res, scene["hv"], f2, None) <= 1.0


# ---- 9. the CLI chain -------------------------------------------------------------------------------------------------------
def _run(args, timeout=600):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_cli_chain_end_to_end(tmp_path):
    sc = fusion_synth.scene(96, 128, 4, seed=2)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    fusion_synth.write_predict_layout(sc, data, out)
    _run([os.path.join(ROOT, "fuse_whu.py"), "--data_folder", data, "--output_folder", out])
    _run([os.path.join(ROOT, "mesh_whu.py"), "--data_folder", data, "--output_folder", out, "--voxel", "0.5", "--weld"])
    _run([os.path.join(ROOT, "texture_whu.py"), "--data_folder", data, "--output_folder", out, "--page", "1024"])
    _, mfaces = mesh_mod.read_mesh_ply(os.path.join(out, "mesh.ply"))
    ply = texture.read_textured_ply(os.path.join(out, "mesh_textured.ply"))
    assert len(ply["faces"]) == len(mfaces) > 0
    np.testing.assert_array_equal(ply["faces"], mfaces)
    js = json.load(open(os.path.join(out, "mesh_textured.json")))
    assert js["occlusion_tol"] == 1.0 and js["P"] == 1024
    assert js["faces"] == len(mfaces) == js["faces_textured"] + js["faces_untextured"]
    assert sorted(js["views_used"] + js["views_culled"]) == [0, 1, 2, 3, 4]
    assert js["faces_textured"] > 0.5 * js["faces"] and js["charts"] >= 1 and 0 < js["box_fraction"] <= 1
    assert set(js["device_ms"]) == set(texture.PHASES)
    assert ply["tex_files"] == ["mesh_textured_tex_%04d.png" % k for k in range(js["pages"])]
    for name in ply["tex_files"]:
        assert os.path.exists(os.path.join(out, name))
    assert (ply["texnum"] >= 0).all() and (ply["texnum"] < js["pages"]).all()
