"""Host side of the mesh texture (ada_mvs_amd/texture.py), on CPU: the packing rule on hand cases and against the restatement's
independent packer, the texture-coordinate formula, the textured PLY round trip, option and mesh checks, and the parser."""
import json

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, fusion, texture
import texture_ref as R


def test_packing_hand_cases():
    # sorted by h, then w (both descending), then index; a shelf is as tall as its first item
    ox, oy, pg, n = texture.pack([3, 5, 2, 4], [2, 2, 7, 1], 1024)
    assert (list(ox), list(oy), list(pg), n) == ([7, 2, 0, 10], [0, 0, 0, 0], [0, 0, 0, 0], 1)
    # x + w > P starts a shelf, y + h > P a page
    ox, oy, pg, n = texture.pack([600, 600, 600, 300], [500, 500, 400, 100], 1024)
    assert list(ox) == [0, 0, 0, 600] and list(oy) == [0, 500, 0, 0] and list(pg) == [0, 0, 1, 1] and n == 2
    # an exact fit stays on the shelf
    ox, oy, pg, n = texture.pack([512, 512, 1], [3, 3, 3], 1024)
    assert list(ox) == [0, 512, 0] and list(oy) == [0, 0, 3] and n == 1
    assert texture.pack([], [], 1024)[3] == 0
    with pytest.raises(ValueError):
        texture.pack([1025], [1], 1024)


def test_packing_equals_the_independent_packer():
    rng = np.random.default_rng(3)
    for P, n in ((1024, 2000), (2048, 500), (1024, 1)):
        w = rng.integers(1, 300, n)
        h = rng.integers(1, 300, n)
        h[::7] = h[0]                      # ties on h, then on w
        w[::11] = w[0]
        ox, oy, pg, pages = texture.pack(w, h, P)
        place, ref_pages = R.shelf_pack(list(zip(w.tolist(), h.tolist())), P)
        assert pages == ref_pages
        np.testing.assert_array_equal(np.stack([ox, oy, pg], 1), np.array(place))
        # no two items overlap and every item lies inside its page
        assert ((ox + w <= P) & (oy + h <= P)).all()
        for p in range(pages):
            cov = np.zeros((P, P), np.int32)
            for i in np.nonzero(pg == p)[0]:
                cov[oy[i]:oy[i] + h[i], ox[i]:ox[i] + w[i]] += 1
            assert cov.max() <= 1


def test_palette_block_and_boxes():
    assert texture.palette_block(0, 1024) is None
    assert texture.palette_block(5, 1024) == (5, 1)
    assert texture.palette_block(1024 * 3 + 1, 1024) == (1024, 4)
    x0, y0, x1, y1 = texture.chart_boxes([[1, 0, 98, 40], [10, 20, 30, 40]], np.array([0, 1]), [100, 200], [50, 60], 2)
    assert list(x0) == [0, 8] and list(y0) == [0, 18] and list(x1) == [99, 33] and list(y1) == [43, 43]


def test_texture_coordinate_formula():
    s, t = texture.tex_coords([10.25], [20.5], [8], [19], [100], [200], 1024)
    assert s.dtype == np.float32 and t.dtype == np.float32
    assert s[0] == np.float32((100 + 2.25 + 0.5) / 1024)
    assert t[0] == np.float32(1.0 - (200 + 1.5 + 0.5) / 1024)
    # a texel centre maps back to its pixel: s P - 1/2 = ox + u - x0
    s, t = texture.tex_coords(np.array([3.0]), np.array([4.0]), 3, 4, 7, 9, 2048)
    assert s[0] * 2048 - 0.5 == 7 and (1 - t[0]) * 2048 - 0.5 == 9


def test_textured_ply_round_trip(tmp_path):
    verts = np.zeros(4, fusion.PLY_DTYPE)
    verts["x"], verts["y"], verts["z"] = [0.0, 1.0, 0.0, 5e5 + 0.125], [0.0, 0.0, 1.0, 3.4e6], [0.0, 0.0, 0.0, 2.0]
    verts["red"] = [1, 2, 3, 4]
    faces = np.array([[0, 1, 2], [1, 3, 2]], np.uint32)
    tc = np.arange(12, dtype=np.float32).reshape(2, 6) / 16
    texnum = np.array([0, 1], np.int32)
    p = str(tmp_path / "m.ply")
    texture.write_textured_ply(p, verts, faces, tc, texnum, texture.texture_names(str(tmp_path / "m"), 2))
    back = texture.read_textured_ply(p)
    assert back["tex_files"] == ["m_tex_0000.png", "m_tex_0001.png"]
    assert back["verts"].tobytes() == verts.tobytes()
    np.testing.assert_array_equal(back["faces"], faces)
    np.testing.assert_array_equal(back["tc"], tc)
    np.testing.assert_array_equal(back["texnum"], texnum)
    head = open(p, "rb").read().split(b"end_header\n")[0].decode()
    assert "property list uchar float texcoord\nproperty int texnumber" in head
    assert head.count("comment TextureFile") == 2
    assert len(open(p, "rb").read()) == len(head) + 11 + 4 * 27 + 2 * (1 + 12 + 1 + 24 + 4)


def test_option_and_mesh_checks(tmp_path):
    for bad in (512, 1000, 32768, 8192.0, True, None):
        with pytest.raises(ValueError):
            texture.check_page(bad)
    assert texture.check_page(1024) == 1024 and texture.check_page(16384) == 16384
    for tol, border, pad in ((-1.0, 2.0, 2), (float("nan"), 2.0, 2), (0.5, -1.0, 2), (0.5, 2.0, -1), (0.5, 2.0, 1.5)):
        with pytest.raises(ValueError):
            texture.check_options(tol, border, pad)
    texture.check_options(0.0, 0.0, 0)
    with pytest.raises(ValueError, match="out of range"):
        texture.check_mesh(3, np.array([[0, 1, 3]], np.uint32))
    texture.check_mesh(3, np.array([[0, 1, 2]], np.uint32))

    class Huge:
        shape = (texture.MAX_FACES + 1, 3)
    with pytest.raises(ValueError, match="faces"):
        texture.check_mesh(3, Huge())
    mesh = str(tmp_path / "mesh.ply")
    assert texture.default_tol(mesh) is None
    json.dump({"voxel": 0.25}, open(mesh + ".json", "w"))
    assert texture.default_tol(mesh) == 0.5


def test_parser_and_abi():
    a = texture.build_parser().parse_args(["--data_folder", "d", "--output_folder", "o"])
    assert (a.mesh, a.out, a.occlusion_tol, a.border_px, a.pad, a.page) == (None, None, None, 2.0, 2, 8192)
    a = texture.build_parser().parse_args(["--data_folder", "d", "--output_folder", "o", "--mesh", "m.ply", "--out", "x", "--page", "1024",
                                           "--occlusion_tol", "0.3", "--pad", "0", "--border_px", "1"])
    assert (a.mesh, a.out, a.page, a.occlusion_tol, a.pad, a.border_px) == ("m.ply", "x", 1024, 0.3, 0, 1.0)
    with pytest.raises(SystemExit):
        texture.build_parser().parse_args(["--data_folder", "d"])
    assert _lib.ABI_VERSION == 22 and (texture.MIN_PAGE, texture.MAX_PAGE) == _lib.TEXTURE_PAGES
    for name in ("adamvs_texture_project", "adamvs_texture_zbuf", "adamvs_texture_score", "adamvs_texture_components",
                 "adamvs_texture_fill", "adamvs_texture_coords"):
        assert name in _lib.SIGNATURES
