"""Seam levelling on the GPU (csrc/texture_level.hip through ada_mvs_amd/texture.py, seam_level=True) against the float64
restatement (tests/texture_level_ref.py): the node graph, the observed colour, the solve against the restatement's
minimum-norm solution, the property users see (per-view exposure offsets are removed up to one constant per connected
component), the owner map and the levelled texels, no change without seams or with the option off, determinism, the CLI.

A view's radiometry is changed by adding an integer offset to the R and G channels of its uint8 image: ortho_scene.tex_rg
spans 38 .. 218, so offsets within +-12 never clip (asserted).  B holds the face-class code and stays as it is."""
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
import texture_level_ref as L
import texture_scene as S

pytestmark = pytest.mark.gpu

OFFSET = (5e5, 3.4e6, 0.0)
TOL, BORDER, PAD, PAGE = 1.0, 2.0, 2, 1024
GROW_PX = 2e-3                      # owner decisions within this many pixels of an edge are set aside (tests/test_texture_gpu.py)
U = 2.0 ** -24                      # fp32 unit roundoff
TIGHT = dict(seam_level=True, seam_tol=1e-10, seam_iters=20000, keep_level=True)


def run(xyz, rgb, faces, views, **kw):
    args = dict(occlusion_tol=TOL, border_px=BORDER, pad=PAD, page=PAGE)
    args.update(kw)
    return texture.texture_mesh(xyz, rgb, faces, views, **args)


def shifted(views, offsets, hit_only=False):
    """The views with offsets[k] added to R and G of view k (every pixel, or only those that see the scene) -> (device views,
    host images)."""
    import torch
    out, imgs = [], []
    for v, b in zip(views, offsets):
        img = v["rgba_h"].copy()
        hit = img[..., 2] != 0
        rg = img[..., :2].astype(np.int64)
        assert rg[hit].min() >= 12 and rg[hit].max() <= 243, "tex_rg left its range"
        new = rg + (b * hit[..., None] if hit_only else b)
        assert new.min() >= 0 and new.max() <= 255, "an offset clips"
        img[..., :2] = new
        out.append(dict(iid=v["iid"], K=v["K"], R=v["R"], C=v["C"], rgba=torch.from_numpy(img).to("cuda"), rgba_h=img))
        imgs.append(img)
    return out, imgs


B_OFFSETS = (0, 3, 6, 9, 12)        # >= 0: the pixels that see nothing hold 0 and must not clip either


@pytest.fixture(scope="module")
def scene():
    cams = OS.cameras(192, 256)
    views = OS.views(cams, device="cuda")
    xyz, rgb, faces, cls, box = S.mesh()
    vb, imgs_b = shifted(views, B_OFFSETS)
    plain = run(xyz, rgb, faces, views)
    a = run(xyz, rgb, faces, views, **TIGHT)
    b = run(xyz, rgb, faces, vb, **TIGHT)
    return dict(views=views, vb=vb, imgs_a=[v["rgba_h"] for v in views], imgs_b=imgs_b, xyz=xyz, rgb=rgb, faces=faces, plain=plain, a=a, b=b)


def graph_of(res, faces):
    nv_, nc_, corner = L.nodes(faces, res["chart"])
    smooth, seam, data = L.edges_fast(faces, res["chart"], corner)
    return dict(node_vertex=nv_, node_chart=nc_, corner=corner, smooth=smooth, seam=seam, data=data, n=len(nv_))


def assert_graph(res, faces):
    g = graph_of(res, faces)
    np.testing.assert_array_equal(res["node_vertex"], g["node_vertex"])
    np.testing.assert_array_equal(res["node_chart"], g["node_chart"])
    tex = res["chart"] >= 0
    np.testing.assert_array_equal(res["corner_node"][tex], g["corner"][tex])
    np.testing.assert_array_equal(res["edges_smooth"], g["smooth"])
    np.testing.assert_array_equal(res["edges_seam"], g["seam"])
    np.testing.assert_array_equal(res["edges_data"], g["data"])
    assert res["nodes"] == g["n"] and res["data_edges"] == len(g["data"]) and res["smooth_edges"] == len(g["smooth"])
    assert res["graph_entries"] == 2 * (len(g["data"]) + len(g["smooth"]))
    return g


# ---- 1. structure -----------------------------------------------------------------------------------------------------------
def test_graph_equals_the_restatement_welded_and_unwelded(scene):
    xyz, rgb, faces = scene["xyz"], scene["rgb"], scene["faces"]
    g = assert_graph(scene["a"], faces)
    assert len(g["data"]) > 1000 and g["seam"].sum() > 1000 and g["n"] > len(np.unique(faces[scene["a"]["chart"] >= 0]))
    quick = dict(seam_level=True, seam_iters=0, keep_level=True)
    # welded: the scene's parts (terrain, roofs, walls) share their border vertices
    uniq, first, inv = np.unique(xyz, axis=0, return_index=True, return_inverse=True)
    fw = np.asarray(inv).reshape(-1)[faces.astype(np.int64)].astype(np.uint32)
    assert len(uniq) < len(xyz)
    rw = run(uniq, rgb[first], fw, scene["views"], **quick)
    gw = assert_graph(rw, fw)
    assert rw["seam_cap_hit"] and rw["seam_iterations"] == 0
    # unwelded: a cut at x = 0, as two bricks would write it
    f64 = faces.astype(np.int64)
    east = xyz[f64[:, 0], 0] >= 0.0
    f2 = np.where(east[:, None], f64 + len(xyz), f64).astype(np.uint32)
    r2 = run(np.concatenate([xyz, xyz]), np.concatenate([rgb, rgb]), f2, scene["views"], **quick)
    g2 = assert_graph(r2, f2)
    # the cut splits charts but joins nothing across it: its two sides share no vertex, so no data edge crosses it
    assert g2["n"] > g["n"]
    assert ((g2["node_vertex"][g2["data"][:, 0]] >= len(xyz)) == (g2["node_vertex"][g2["data"][:, 1]] >= len(xyz))).all()
    assert gw["n"] > 0


# ---- 2. the observed colour ---------------------------------------------------------------------------------------------------
def f_bound(res, W, H):
    """fp32 against float64 on the same fp32 positions.  Per sample position and axis two roundings (d = p_w - p_v, p_v + t d;
    t d is exact) of at most U max(W, H) each, seen through a bilinear surface of slope at most 255 per pixel and axis:
    255 U 4 max(W, H).  The bilinear formula is 11 operations on values <= 255; the accumulation adds two roundings per sample
    (3 per seam edge) relative to a partial sum whose share of the result is <= 255, and the division one."""
    deg = np.bincount(res["edges_smooth"][res["edges_seam"]].reshape(-1), minlength=res["nodes"]).max()
    return 255.0 * U * (4 * max(W, H) + 11 + 2 * 3 * deg + 1)


def test_observed_colour_matches_the_restatement(scene):
    for key, imgs in (("a", scene["imgs_a"]), ("b", scene["imgs_b"])):
        res = scene[key]
        np.testing.assert_array_equal(res["pos"], L.positions(res["corner_node"].astype(np.int64), res["uv"], res["nodes"]).astype(np.float32))
        view = res["charts"][:, 7][res["node_chart"]]
        want = L.observe(res["pos"].astype(np.float64), view, res["edges_smooth"], res["edges_seam"], imgs)
        err = np.abs(res["f"] - want).max()
        bound = f_bound(res, 256, 192)
        print("f: max error %.3g, bound %.3g" % (err, bound))
        assert err <= bound
    # the offsets show in f exactly as added (R, G) and not at all in B
    view = scene["a"]["charts"][:, 7][scene["a"]["node_chart"]]
    d = scene["b"]["f"].astype(np.float64) - scene["a"]["f"]
    assert np.abs(d[:, :2] - np.asarray(B_OFFSETS, np.float64)[view][:, None]).max() <= 2 * f_bound(scene["a"], 256, 192)
    assert (d[:, 2] == 0).all()


# ---- 3. the solve ----------------------------------------------------------------------------------------------------------------
def small_mesh():
    """mesh(terrain_step=4) cut down to the window x in [-56, 6], y in [10, 70]: the box (-20 .. 4, 30 .. 48, 33 m) whole, the
    terrain around it and the strip of the next box that reaches into the window, welded."""
    xyz, rgb, faces, _, _ = S.mesh(terrain_step=4.0)
    P = xyz[faces.astype(np.int64)]
    keep = ((P[..., 0] >= -56.0) & (P[..., 0] <= 6.0) & (P[..., 1] >= 10.0) & (P[..., 1] <= 70.0)).all(1)
    used, inv = np.unique(faces[keep].astype(np.int64), return_inverse=True)
    xyz, rgb, faces = xyz[used], rgb[used], np.asarray(inv).reshape(-1, 3)
    # welded: the roof, the walls and the terrain share their border vertices, so their charts meet in seams
    uniq, first, inv = np.unique(xyz, axis=0, return_index=True, return_inverse=True)
    return uniq, rgb[first], np.asarray(inv).reshape(-1)[faces].astype(np.uint32)


def test_solve_reaches_the_minimum_norm_solution(scene):
    xyz, rgb, faces = small_mesh()
    views, _ = shifted(scene["views"], (-12, -6, 0, 6, 12), hit_only=True)
    res = run(xyz, rgb, faces, views, **TIGHT)
    g = assert_graph(res, faces)
    n = g["n"]
    assert 1000 <= n <= 4500, n
    assert len(g["data"]) > 50 and len(np.unique(res["charts"][:, 7])) >= 3
    Lm = L.laplacian(n, g["smooth"], g["data"], 0.1)
    comp = L.components(n, [g["smooth"], g["data"]])
    b = L.rhs(res["f"].astype(np.float64), g["data"], n)
    ref = L.min_norm(Lm, b, comp)
    err = np.abs(res["g"] - ref).max()
    print("solve: %d nodes, %d iterations, residual %s, max |g - g_ref| = %.3g, max |g| = %.3g"
          % (n, res["seam_iterations"], res["seam_residual"], err, np.abs(ref).max()))
    assert not res["seam_cap_hit"] and max(res["seam_residual"]) <= 1e-10
    assert np.abs(ref).max() > 3.0                 # the offsets are there to be removed
    assert err <= 0.25
    # the residual the solver reports is the true one
    # the residual the solver reports is the true one, up to what the recursion r -= alpha Ap loses in fp64: one rounding of
    # |L| |g| per iteration (|L| <= twice the largest diagonal entry), with a factor 10 for the vector norms
    true = np.linalg.norm(b - Lm @ res["g"], axis=0) / np.linalg.norm(b, axis=0)
    drift = 10 * res["seam_iterations"] * 2.0 ** -52 * 2 * Lm.diagonal().max() * np.linalg.norm(res["g"], axis=0) / np.linalg.norm(b, axis=0)
    assert (true <= 1e-10 + drift).all(), (true, drift)
    # and the default tolerance stops earlier, at its own exact iteration
    res4 = run(xyz, rgb, faces, views, seam_level=True)
    assert 0 < res4["seam_iterations"] < res["seam_iterations"] and max(res4["seam_residual"]) <= 1e-4 and not res4["seam_cap_hit"]
    print("default tolerance: %d iterations on the GPU, %d by the restatement's conjugate gradients" % (res4["seam_iterations"], L.cg(Lm, b, 1e-4, 1000)[1]))
    assert np.abs(res4["g"] - ref).max() <= 0.25
    # the cap is reported
    res5 = run(xyz, rgb, faces, views, seam_level=True, seam_iters=5)
    assert res5["seam_cap_hit"] and res5["seam_iterations"] == 5


# ---- 4. the property users see ------------------------------------------------------------------------------------------------
def rms_rg(res, with_g):
    v = res["f"][:, :2].astype(np.float64) + (res["g"][:, :2] if with_g else 0.0)
    e = res["edges_data"]
    return float(np.sqrt(((v[e[:, 0]] - v[e[:, 1]]) ** 2).mean()))


def test_per_view_offsets_are_levelled_out(scene):
    a, b = scene["a"], scene["b"]
    for k in ("label", "chart", "charts", "node_vertex", "node_chart", "corner_node", "edges_smooth", "edges_data", "owner", "tc", "texnum"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for r in (a, b):
        assert not r["seam_cap_hit"] and max(r["seam_residual"]) <= 1e-10, (r["seam_iterations"], r["seam_residual"])
    n = a["nodes"]
    comp = L.components(n, [a["edges_smooth"], a["edges_data"]])
    view = a["charts"][:, 7][a["node_chart"]]
    d = b["g"][:, :2] - a["g"][:, :2] + np.asarray(B_OFFSETS, np.float64)[view][:, None]
    _, ci = np.unique(comp, return_inverse=True)
    ci = np.asarray(ci).reshape(-1)
    cnt = np.bincount(ci)
    c = np.stack([np.bincount(ci, d[:, k]) / cnt for k in range(2)], 1)           # one constant per component and channel
    dev = np.abs(d - c[ci]).max()
    print("g_B - g_A + b_view - c: max %.3g over %d nodes in %d components; iterations %d / %d"
          % (dev, n, len(cnt), a["seam_iterations"], b["seam_iterations"]))
    assert dev <= 1e-3
    assert (b["g"][:, 2] == a["g"][:, 2]).all() or np.abs(b["g"][:, 2] - a["g"][:, 2]).max() <= 1e-3
    before_a, before_b, after_a, after_b = rms_rg(a, False), rms_rg(b, False), rms_rg(a, True), rms_rg(b, True)
    print("rms across seams (R, G): A %.3f -> %.3f, B %.3f -> %.3f; reported A %.3f -> %.3f, B %.3f -> %.3f"
          % (before_a, after_a, before_b, after_b, a["seam_rms_before"], a["seam_rms_after"], b["seam_rms_before"], b["seam_rms_after"]))
    assert abs(after_b - after_a) <= 1e-3 and abs(b["seam_rms_after"] - a["seam_rms_after"]) <= 1e-3
    assert before_b > before_a + 1.0 and b["seam_rms_before"] > a["seam_rms_before"]
    assert after_a <= before_a and after_b < before_b
    # the reported figures are the stated rms over all three channels
    for r in (a, b):
        v = r["f"].astype(np.float64)
        e = r["edges_data"]
        np.testing.assert_allclose(r["seam_rms_before"], np.sqrt(((v[e[:, 0]] - v[e[:, 1]]) ** 2).mean()), rtol=1e-12)
        v = v + r["g"]
        np.testing.assert_allclose(r["seam_rms_after"], np.sqrt(((v[e[:, 0]] - v[e[:, 1]]) ** 2).mean()), rtol=1e-12)
    # the atlases: B levelled = A levelled + round(c) within one level on the owned texels that are not clamped
    owned = a["owner"] != L.UNOWNED
    _, _, _, pg, ax, ay = (t[owned] for t in L.texel_index(a["charts"], a["owner_prefix"]))
    tc = ci[a["corner_node"][a["owner"][owned], 0]]
    ta, tb = a["atlas"][pg, ay, ax, :2].astype(np.int64), b["atlas"][pg, ay, ax, :2].astype(np.int64)
    free = (ta > 0) & (ta < 255) & (tb > 0) & (tb < 255)
    diff = np.abs(tb - ta - np.round(c[tc]).astype(np.int64))
    assert free.mean() > 0.99
    assert diff[free].max() <= 1, diff[free].max()
    # while before levelling they differ by the offsets
    ua, ub = a["atlas_unlevelled"][pg, ay, ax, :2].astype(np.int64), b["atlas_unlevelled"][pg, ay, ax, :2].astype(np.int64)
    np.testing.assert_array_equal(ub - ua, np.broadcast_to(np.asarray(B_OFFSETS)[a["charts"][:, 7]][a["chart"][a["owner"][owned]]][:, None], ua.shape))


# ---- 5. apply -----------------------------------------------------------------------------------------------------------------
def test_owner_map_and_levelled_texels(scene):
    """Owned texels whose float64 value texel + g lies within 1e-3 of a rounding boundary are held to one level only; uniform
    fractions would make them 0.2 %, the condition is at most 1 %.  On this scene (the full analytic mesh, offsets 0 .. 12)
    they are 0.80 % of 86 243 owned texels, evaluated with the restatement's float64 arithmetic on the solved g (the share
    is above the uniform figure because most of the terrain carries an almost constant g and integer texels)."""
    res, plain = scene["b"], scene["plain"]
    charts, prefix = res["charts"], res["owner_prefix"]
    np.testing.assert_array_equal(prefix, np.concatenate([[0], np.cumsum(charts[:, 2].astype(np.int64) * charts[:, 3])]))
    lo = L.owner_map(res["uv"], res["chart"], charts, prefix, GROW_PX)
    hi = L.owner_map(res["uv"], res["chart"], charts, prefix, -GROW_PX)
    firm = lo == hi
    assert firm.mean() > 0.9, firm.mean()
    np.testing.assert_array_equal(res["owner_raster"][firm], lo[firm])
    ref = L.owner_map(res["uv"], res["chart"], charts, prefix)
    assert (res["owner_raster"] != ref).mean() <= 1.0 - firm.mean()
    # the owner is a face of the texel's chart
    ci = L.texel_index(charts, prefix)[0]
    own = res["owner_raster"] != L.UNOWNED
    np.testing.assert_array_equal(res["chart"][res["owner_raster"][own]], ci[own])
    # the dilation, exactly, from the GPU's own raster
    np.testing.assert_array_equal(res["owner"], L.dilate(res["owner_raster"], charts, prefix))
    assert (res["owner"] != L.UNOWNED).sum() > own.sum()
    # the levelled texels
    owned, val, pg, ax, ay = L.levelled_values(res["atlas_unlevelled"], res["owner"].astype(np.int64), res["uv"],
                                               res["corner_node"].astype(np.int64), res["g"].astype(np.float32), charts, prefix)
    want = np.clip(np.floor(val + 0.5), 0, 255)
    got = res["atlas"][pg, ay, ax].astype(np.float64)
    frac = val + 0.5 - np.floor(val + 0.5)
    near = (np.minimum(frac, 1.0 - frac) <= 1e-3).any(1)
    print("apply: %d owned texels, %.3f %% within 1e-3 of a rounding boundary, max |g| %.2f" % (owned.sum(), 100 * near.mean(), np.abs(res["g"]).max()))
    assert near.mean() <= 0.01
    np.testing.assert_array_equal(got[~near], want[~near])
    assert np.abs(got - want).max() <= 1
    assert (got != res["atlas_unlevelled"][pg, ay, ax]).any()
    # everything else is untouched: unowned texels, the palette, the rest of the pages
    mask = np.zeros(res["atlas"].shape[:3], bool)
    mask[pg, ay, ax] = True
    np.testing.assert_array_equal(res["atlas"][~mask], res["atlas_unlevelled"][~mask])
    assert res["palette"] is not None
    ox, oy, ppg, pw, ph = res["palette"]
    assert not mask[ppg, oy:oy + ph, ox:ox + pw].any()
    np.testing.assert_array_equal(scene["a"]["atlas_unlevelled"], plain["atlas"])


# ---- 6. no seams, no change ------------------------------------------------------------------------------------------------------
def write(tmp_path, name, scene, res):
    verts = np.zeros(len(scene["xyz"]), mesh_mod.fusion.PLY_DTYPE)
    verts["x"], verts["y"], verts["z"] = scene["xyz"].T
    verts["red"], verts["green"], verts["blue"] = scene["rgb"].T
    paths = texture.write_outputs(str(tmp_path / name / "m"), verts, scene["faces"], res)
    return [open(p, "rb").read() for p in [paths["ply"]] + paths["pages"]]


def test_one_view_has_no_seams_and_changes_nothing(scene, tmp_path):
    one = scene["views"][:1]
    off = run(scene["xyz"], scene["rgb"], scene["faces"], one)
    on = run(scene["xyz"], scene["rgb"], scene["faces"], one, seam_level=True, keep_level=True)
    assert on["seam_iterations"] == 0 and not on["seam_cap_hit"] and on["seam_residual"] == [0.0, 0.0, 0.0]
    assert on["nodes"] > 0 and on["data_edges"] == 0 and (on["g"] == 0.0).all() and on["seam_rms_before"] == on["seam_rms_after"] == 0.0
    np.testing.assert_array_equal(on["atlas"], off["atlas"])
    for x, y in zip(write(tmp_path, "on", scene, on), write(tmp_path, "off", scene, off)):
        assert x == y
    assert set(on["device_ms"]) == set(texture.PHASES + texture.LEVEL_PHASES) and set(off["device_ms"]) == set(texture.PHASES)


def test_the_option_off_is_the_call_without_it(scene):
    off = run(scene["xyz"], scene["rgb"], scene["faces"], scene["views"], seam_level=False)
    for k in ("label", "nvis", "best", "uv", "parent", "chart", "charts", "pal", "atlas", "tc", "texnum"):
        np.testing.assert_array_equal(off[k], scene["plain"][k], err_msg=k)
    assert "g" not in off and "seam_iterations" not in off and set(off["device_ms"]) == set(texture.PHASES)
    assert set(texture.summary(off)) == set(texture.summary(scene["plain"]))


# ---- 7. determinism -----------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_far_offset_give_identical_bytes(scene, tmp_path):
    again = run(scene["xyz"], scene["rgb"], scene["faces"], scene["vb"], **TIGHT)
    assert again["seam_iterations"] == scene["b"]["seam_iterations"]
    assert again["g"].tobytes() == scene["b"]["g"].tobytes() and again["f"].tobytes() == scene["b"]["f"].tobytes()
    for x, y in zip(write(tmp_path, "r0", scene, scene["b"]), write(tmp_path, "r1", scene, again)):
        assert x == y
    cams = OS.cameras(192, 256, offset=OFFSET)
    far_views, _ = shifted(OS.views(cams, device="cuda"), B_OFFSETS)
    xyz, rgb, faces, _, _ = S.mesh(offset=OFFSET)
    far = run(xyz, rgb, faces, far_views, **TIGHT)
    assert far["g"].tobytes() == scene["b"]["g"].tobytes()
    np.testing.assert_array_equal(far["atlas"], scene["b"]["atlas"])
    np.testing.assert_array_equal(far["owner"], scene["b"]["owner"])


# ---- 8. the CLI ---------------------------------------------------------------------------------------------------------------
def _run(args, timeout=600):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_cli_chain_with_seam_level(tmp_path):
    sc = fusion_synth.scene(96, 128, 4, seed=2)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    fusion_synth.write_predict_layout(sc, data, out)
    _run([os.path.join(ROOT, "fuse_whu.py"), "--data_folder", data, "--output_folder", out])
    _run([os.path.join(ROOT, "mesh_whu.py"), "--data_folder", data, "--output_folder", out, "--voxel", "0.5", "--weld"])
    base = [os.path.join(ROOT, "texture_whu.py"), "--data_folder", data, "--output_folder", out, "--page", "1024"]
    _run(base)
    r = _run(base + ["--seam_level", "--seam_iters", "3000", "--out", os.path.join(out, "levelled")])
    assert "seams levelled" in r.stdout
    js, js0 = json.load(open(os.path.join(out, "levelled.json"))), json.load(open(os.path.join(out, "mesh_textured.json")))
    for k in ("nodes", "seam_lambda", "seam_tol", "seam_iters", "seam_iterations", "seam_residual", "seam_cap_hit", "seam_rms_before",
              "seam_rms_after"):
        assert k in js and k not in js0, k
    assert (js["seam_lambda"], js["seam_tol"], js["seam_iters"]) == (0.1, 1e-4, 3000)
    assert set(js["device_ms"]) == set(texture.PHASES + texture.LEVEL_PHASES) and set(js0["device_ms"]) == set(texture.PHASES)
    assert js["nodes"] > 0 and len(js["seam_residual"]) == 3
    assert js["seam_cap_hit"] or max(js["seam_residual"]) <= 1e-4
    assert js["seam_rms_after"] <= js["seam_rms_before"]
    a, b = texture.read_textured_ply(os.path.join(out, "mesh_textured.ply")), texture.read_textured_ply(os.path.join(out, "levelled.ply"))
    for k in ("faces", "tc", "texnum"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["verts"].tobytes() == b["verts"].tobytes()
    assert b["tex_files"] == ["levelled_tex_%04d.png" % k for k in range(js["pages"])]
    for name in b["tex_files"]:
        assert os.path.exists(os.path.join(out, name))
