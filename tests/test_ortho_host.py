"""Image orthophoto, host side (no GPU): the orthophoto grid, argument refusals, the surface rule of the restatement
(tests/ortho_ref.py), world-file text and output paths, the restatement's z-buffer of a plane against the closed form, and the
C ABI's argument errors."""
import ctypes
import json

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, dsm, fusion_synth, ortho
import ortho_ref as R

GRID = dsm.Grid(1000.0, 2000.0, 0.5, 0.0, 40, 30)


@pytest.mark.parametrize("K", range(1, 9))
def test_orthophoto_grid(K):
    g = ortho.ortho_grid(GRID, K)
    assert (g.W, g.H) == (40 * K, 30 * K)
    assert g.x0 == GRID.x0 and g.y_top == GRID.y_top and g.gsd == GRID.gsd / K
    x, y = R.cell_centres(GRID, K)
    assert x[0, 0] == GRID.x0 + 0.5 * GRID.gsd / K and y[0, 0] == GRID.y_top - 0.5 * GRID.gsd / K
    # the orthophoto covers exactly the DSM's extent
    assert abs(x[0, -1] + 0.5 * g.gsd - (GRID.x0 + GRID.W * GRID.gsd)) < 1e-9
    assert abs(y[-1, 0] - 0.5 * g.gsd - (GRID.y_top - GRID.H * GRID.gsd)) < 1e-9


@pytest.mark.parametrize("K", [0, 9, 1.5, -1, "x", None, True, float("nan")])
def test_refuses_bad_upsample(K):
    with pytest.raises(ValueError):
        ortho.ortho_grid(GRID, K)


def test_integral_float_upsample_is_accepted():
    assert ortho.check_upsample(2.0) == 2


def test_refuses_more_than_2_28_cells():
    big = dsm.Grid(0.0, 0.0, 1.0, 0.0, 1 << 13, 1 << 13)          # 2^26 cells
    assert ortho.ortho_grid(big, 2).W == 1 << 14                   # 2^28: the cap itself is allowed
    with pytest.raises(ValueError, match="cap"):
        ortho.ortho_grid(big, 3)


@pytest.mark.parametrize("kw", [dict(mode="median"), dict(occlusion_tol=-0.1), dict(occlusion_tol=float("inf")), dict(border_px=-1),
                                dict(feather_px=0.0)])
def test_refuses_bad_options(kw):
    args = dict(mode="best", occlusion_tol=1.0, border_px=2.0, feather_px=64.0)
    args.update(kw)
    with pytest.raises(ValueError):
        ortho.check_options(**args)


def test_refuses_missing_dsm_json(tmp_path):
    with pytest.raises(FileNotFoundError, match="_dsm.json"):
        ortho.read_dsm(str(tmp_path / "nothing"))


def test_read_dsm_round_trip(tmp_path):
    from PIL import Image
    prefix = str(tmp_path / "d")
    z = np.arange(12, dtype=np.float32).reshape(3, 4)
    z[1, 2] = np.nan
    with open(prefix + "_dsm.json", "w") as f:
        json.dump(dict(grid=dict(x0=10.0, y_top=20.0, gsd=0.25, W=4, H=3), z_ref=-3), f)
    Image.fromarray(z).save(prefix + "_dsm.tif", format="TIFF")
    Image.fromarray(z + 1).save(prefix + "_dsm_filled.tif", format="TIFF")
    d, g = ortho.read_dsm(prefix)
    assert g == dsm.Grid(10.0, 20.0, 0.25, -3, 4, 3)
    np.testing.assert_array_equal(d, z)
    np.testing.assert_array_equal(ortho.read_dsm(prefix, filled=True)[0], z + 1)


# ---- the surface rule -----------------------------------------------------------------------------------------------------
def test_upsample_1_is_the_dsm_cell_for_cell():
    rng = np.random.default_rng(0)
    z = rng.uniform(-5, 50, (17, 23)).astype(np.float32)
    z[rng.random(z.shape) < 0.2] = np.nan
    h = R.surface(z, 1)
    np.testing.assert_array_equal(np.isnan(h), np.isnan(z))
    np.testing.assert_array_equal(h[~np.isnan(h)], z[~np.isnan(z)].astype(np.float64))


@pytest.mark.parametrize("K", [2, 3, 8])
def test_surface_reproduces_a_plane_and_clamps_at_the_edges(K):
    a, b = np.meshgrid(np.arange(9), np.arange(7))
    z = (0.5 * a - 0.25 * b + 3.0).astype(np.float32)
    h = R.surface(z, K)
    s = np.clip((np.arange(9 * K) + 0.5) / K - 0.5, 0, 8)[None, :]
    t = np.clip((np.arange(7 * K) + 0.5) / K - 0.5, 0, 6)[:, None]
    np.testing.assert_allclose(h, 0.5 * s - 0.25 * t + 3.0, atol=1e-12)
    # the outer half cell is clamped: the first K/2 columns all repeat column 0's height
    assert (h[:, 0] == h[:, (K - 1) // 2]).all()


def test_surface_triangles_follow_the_diagonal_split():
    # one quad, a single raised corner (1, 0): only the triangle (a,b) (a+1,b) (a+1,b+1) (fs >= ft) sees it
    z = np.zeros((2, 2), np.float32)
    z[0, 1] = 1.0
    h = R.surface(z, 8)
    s = np.clip((np.arange(16) + 0.5) / 8 - 0.5, 0, 1)
    S, T = np.meshgrid(s, s)
    np.testing.assert_allclose(h, np.where(S >= T, S - T, 0.0), atol=1e-12)


def test_nan_vertex_of_weight_zero_does_not_void_a_cell():
    z = np.ones((3, 3), np.float32)
    z[0, 1] = np.nan                         # vertex (a=1, b=0)
    h = R.surface(z, 2)
    # K = 2 puts cell centres at s, t in {-1/4 (clamped to 0), 1/4, 3/4, ...}; the cell at s = t = 1/4 lies on the diagonal
    # (fs = ft) of quad (0, 0): its triangle is (0,0) (1,0) (1,1) with weights (3/4, 0, 1/4): the NaN vertex is not used
    assert h[1, 1] == 1.0
    # the cell at s = 3/4, t = 1/4 uses (1, 0) with weight 1/2: void
    assert np.isnan(h[1, 2])
    # the cell exactly on the NaN vertex at K = 1 is void, its neighbours are not
    h1 = R.surface(z, 1)
    assert np.isnan(h1[0, 1]) and np.isfinite(h1[0, 0]) and np.isfinite(h1[1, 1])


# ---- files ----------------------------------------------------------------------------------------------------------------
def test_world_file_and_output_paths():
    g = ortho.ortho_grid(GRID, 4)
    vals = [float(v) for v in dsm.world_file_text(g).split()]
    assert vals == [0.125, 0.0, 0.0, -0.125, 1000.0625, 1999.9375]
    p = ortho.output_paths("/x/run")
    assert p == dict(ortho="/x/run_ortho_img.png", ortho_world="/x/run_ortho_img.pgw", view="/x/run_ortho_img_view.tif",
                     nvis="/x/run_ortho_img_nvis.tif", json="/x/run_ortho_img.json")
    # none of them is a file dsm_whu.py writes
    existing = set(dsm.output_paths("/x/run").values()) | set(dsm.fill_output_paths("/x/run").values())
    assert not existing & set(p.values())


def test_cli_parser_defaults():
    a = ortho.build_parser().parse_args(["--data_folder", "d", "--output_folder", "o", "--dsm", "p"])
    assert (a.upsample, a.mode, a.occlusion_tol, a.border_px, a.feather_px, a.filled, a.out) == (1, "best", None, 2.0, 64.0, False, None)


# ---- the restatement's z-buffer -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam_index", [0, 1, 3])
def test_zbuf_of_a_plane_matches_the_closed_form(cam_index):
    cam = fusion_synth.make_cameras(48, 64, 4)[cam_index]
    g = dsm.Grid(-300.0, 300.0, 4.0, 0.0, 150, 150)
    a, b = np.meshgrid(np.arange(150), np.arange(150))
    x, y = g.x0 + (a + 0.5) * g.gsd, g.y_top - (b + 0.5) * g.gsd
    z = 0.0625 * x - 0.03125 * y + 7.0                          # slopes of a power of two: heights exact in fp32
    zf = z.astype(np.float32)
    assert (zf == z).all()
    zb = R.zbuf(g, zf, cam, 48, 64)
    ref = R.plane_zbuf(cam, 48, 64, np.array([-0.0625, 0.03125, 1.0]), 7.0)
    cov = np.isfinite(zb)
    assert cov.mean() > 0.6
    np.testing.assert_allclose(zb[cov], ref[cov], rtol=1e-12)


def test_zbuf_takes_the_nearer_surface():
    cam = fusion_synth.make_cameras(48, 64, 1)[0]               # nadir at 550 m
    g = dsm.Grid(-40.0, 40.0, 1.0, 0.0, 80, 80)
    z = np.zeros((80, 80), np.float32)
    z[30:50, 30:50] = 100.0
    zb = R.zbuf(g, z, cam, 48, 64)
    assert np.nanmin(zb) == pytest.approx(450.0, rel=1e-9)
    fin = zb[np.isfinite(zb)]
    assert fin.max() <= 550.0 + 1e-9 and zb[24, 32] == pytest.approx(450.0 / np.cos(np.arctan(0.37 / (1.85 * 64))), rel=1e-3)


# ---- the C ABI refuses bad arguments before any launch ---------------------------------------------------------------------
def test_abi_refuses_bad_grid_and_view():
    lib = _lib.load()
    g = _lib.OrthoGrid(0.0, 0.0, 1.0, 10, 10, 9)
    p = ctypes.c_void_p(16)
    assert lib.adamvs_ortho_surface(ctypes.byref(g), p, p, None) < 0
    g.K = 1
    g.gsd = 0.0
    assert lib.adamvs_ortho_surface(ctypes.byref(g), p, p, None) < 0
    g.gsd = 1.0
    v = _lib.OrthoView()
    v.K[8] = 1.0
    v.H, v.W, v.rgba = 8, 8, 16
    assert lib.adamvs_ortho_zbuf(ctypes.byref(g), p, ctypes.byref(v), p, p, p, 161, None) < 0        # capacity 2 * 9 * 9 = 162
    v.K[8] = 2.0
    assert lib.adamvs_ortho_zbuf(ctypes.byref(g), p, ctypes.byref(v), p, p, p, 162, None) < 0
    v.K[8] = 1.0
    for mode, border, feather, tol in ((2, 2.0, 64.0, 1.0), (0, -1.0, 64.0, 1.0), (0, 2.0, 0.0, 1.0), (1, 2.0, 64.0, -1.0)):
        assert lib.adamvs_ortho_compose(ctypes.byref(g), ctypes.byref(v), 0, p, p, mode, border, feather, tol, p, p, p, p, None) < 0
    assert lib.adamvs_ortho_finalize(ctypes.byref(g), p, p, p, p, p, None, None) < 0
    assert b"ortho_finalize" in lib.adamvs_last_error_string()
