"""Ground filter, host side: the numpy restatement (tests/dtm_ref.py) against itself and against hand-computed values, the
schedule, the argument checks of ada_mvs_amd/dtm.py, the file names, the ABI, and the two analytic scenes the GPU tests
build on, on the reference alone."""
import ctypes

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, dsm, dtm
from dtm_ref import NAN_BITS, WIDE_BOX, open_brute, open_sep, plane_scene, pmf, random_raster, same_opening, schedule

SMALL = [
    pytest.param(1, 1, 1.0, id="1x1-valid"), pytest.param(1, 1, 0.0, id="1x1-empty"), pytest.param(37, 1, 0.6, id="W1"),
    pytest.param(1, 53, 0.6, id="H1"), pytest.param(23, 31, 0.0, id="no-valid"), pytest.param(23, 31, 1.0, id="all-valid"),
    pytest.param(41, 47, 0.05, id="sparse"), pytest.param(30, 26, 0.7, id="30x26"),
]


@pytest.mark.parametrize("H,W,p", SMALL)
def test_separable_opening_equals_the_brute_force_window(H, W, p):
    z = random_raster(H, W, seed=H * 100 + W, p_valid=p)
    valid = np.isfinite(z)
    for r in (1, 2, 3, 5, 40):                      # 40 exceeds every side here
        a, b = open_brute(z, r), open_sep(z, r)
        assert same_opening(a, b, z), r
        assert (a[valid] <= z[valid]).all() and np.isfinite(a[valid]).all()


def test_opening_treats_infinities_as_empty_and_keeps_zero_signs_equal():
    z = np.array([[1.0, np.inf, -0.0, 3.0], [-np.inf, 0.0, np.nan, 2.0], [5.0, 4.0, 4.0, 6.0]], np.float32)
    o = open_brute(z, 1)
    assert same_opening(o, open_sep(z, 1), z)
    assert (o[~np.isfinite(z)].view(np.uint32) == NAN_BITS).all()
    assert o[0, 0] == 0.0 and o[2, 3] == 2.0          # E is 0 (of either sign) wherever a window holds a zero; E(2, 3) = min(2, 4, 6)


def test_opening_removes_a_narrow_peak_and_keeps_a_wide_one():
    z = np.zeros((20, 30), np.float32)
    z[5:8, 5:8] = 7.0                                  # 3 wide: removed by r = 2, kept by r = 1
    z[10:19, 12:25] = 4.0                              # 9 x 13: kept by both
    assert (open_sep(z, 1) == z).all()
    o = open_sep(z, 2)
    assert (o[5:8, 5:8] == 0).all() and (o[10:19, 12:25] == 4.0).all()


def test_schedule_against_hand_computed_values():
    radius, dh = dtm.schedule(0.5)
    assert radius.dtype == np.int32 and dh.dtype == np.float64
    assert radius.tolist() == [1, 2, 4, 8, 16, 32]
    # w = 3, 5, 9, 17, 33, 65; differences 2, 2, 4, 8, 16, 32; dh = 0.15 + 0.5 * diff, capped at 2.5
    assert dh.tolist() == [0.15 + 1.0, 0.15 + 1.0, 0.15 + 2.0, 2.5, 2.5, 2.5]
    radius, dh = dtm.schedule(0.5, max_radius=5.0, slope=0.1, dh0=0.2, dh_max=10.0)     # R = 10: 1, 2, 4, 8, 10
    assert radius.tolist() == [1, 2, 4, 8, 10]
    assert dh.tolist() == [0.2 + 0.1 * 0.5 * d for d in (2, 2, 4, 8, 4)]
    radius, dh = dtm.schedule(1.0, max_radius=1.5)                                       # R = 1
    assert radius.tolist() == [1] and dh.tolist() == [2.15]
    radius, dh = dtm.schedule(1.0, max_radius=1024.0)                                    # the cap: 11 levels
    assert radius.tolist() == [1 << k for k in range(11)] and len(radius) <= _lib.DTM_MAX_LEVELS
    for args in ((0.5,), (0.3, 7.0, 0.4, 0.1, 1.7), (1.0, 1.5)):
        a, b = dtm.schedule(*args), schedule(*args)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()


@pytest.mark.parametrize("kw", [dict(gsd=0.0), dict(gsd=float("nan")), dict(gsd=-1.0), dict(max_radius=0.0), dict(max_radius=float("inf")),
                                dict(max_radius=0.4), dict(gsd=0.25, max_radius=256.25), dict(slope=-0.1), dict(slope=float("nan")),
                                dict(dh0=0.0), dict(dh0=-1.0), dict(dh_max=0.0), dict(dh_max=float("inf"))])
def test_schedule_refuses_bad_arguments(kw):
    args = dict(gsd=0.5)
    args.update(kw)
    with pytest.raises(ValueError):
        dtm.schedule(**args)                            # max_radius 0.4 at gsd 0.5: R = 0; 256.25 at 0.25: R = 1025


def test_fill_radius_default_and_cap():
    assert dtm.fill_radius_cells(None, 16.0, 0.5) == (32.0, 64.0)
    assert dtm.fill_radius_cells(10.0, 16.0, 0.5) == (10.0, 20.0)
    assert dtm.fill_radius_cells(None, 400.0, 0.5)[1] == 1024.0
    with pytest.raises(ValueError):
        dtm.fill_radius_cells(0.0, 16.0, 0.5)


def test_parser_defaults():
    a = dtm.build_parser().parse_args(["--dsm", "/x/dsm"])
    assert (a.dsm, a.filled, a.max_radius, a.slope, a.dh0, a.dh_max, a.fill_max_dist, a.out) == ("/x/dsm", False, 16.0, 1.0, 0.15, 2.5, None, None)
    a = dtm.build_parser().parse_args(["--dsm", "p", "--filled", "--max_radius", "8", "--fill_max_dist", "20", "--out", "q"])
    assert (a.filled, a.max_radius, a.fill_max_dist, a.out) == (True, 8.0, 20.0, "q")


def test_output_paths_are_disjoint_from_the_dsm_and_the_fill():
    mine = set(dtm.output_paths("/o/p").values())
    assert mine == {"/o/p_dtm.tif", "/o/p_dtm.tfw", "/o/p_ndsm.tif", "/o/p_ndsm.tfw", "/o/p_ground.png", "/o/p_ground.pgw", "/o/p_dtm.json"}
    assert len(mine) == len(dtm.output_paths("/o/p"))
    assert not mine & set(dsm.output_paths("/o/p").values()) and not mine & set(dsm.fill_output_paths("/o/p").values())


def test_ground_image_round_trip():
    level = np.array([[0, 1, 2, 255], [11, 15, 0, 255]], np.uint8)
    img = dtm.ground_image(level)
    assert img.tolist() == [[255, 16, 32, 0], [176, 240, 255, 0]]
    assert np.array_equal(dtm.level_from_image(img), level)
    with pytest.raises(ValueError):
        dtm.ground_image(np.array([[16]], np.uint8))


def test_abi_version_and_the_new_signatures():
    assert _lib.ABI_VERSION == 22
    for name in ("adamvs_dtm_workspace_bytes", "adamvs_dsm_open", "adamvs_dtm_classify"):
        assert name in _lib.SIGNATURES
    assert (_lib.DTM_MAX_RADIUS, _lib.DTM_MAX_LEVELS, _lib.DTM_TILE) == (1024, 16, 1024)
    assert dtm.MAX_RADIUS == _lib.DTM_MAX_RADIUS and dtm.MAX_LEVELS == _lib.DTM_MAX_LEVELS
    assert ctypes.sizeof(_lib.DtmStats) == 8 + 4 * 8 + 17 * 8      # int levels padded to 8, four longs, 17 per-level longs
    lib = _lib.load()
    assert lib.adamvs_dtm_workspace_bytes(0, 5) < 0 and lib.adamvs_dtm_workspace_bytes(1 << 15, 1 << 14) < 0
    assert lib.adamvs_dtm_workspace_bytes(7, 5) == 256 + 2 * 256
    st = _lib.DtmStats()
    assert lib.adamvs_dtm_classify(4, 4, None, 1, None, None, None, 0, None, None, ctypes.byref(st), None) < 0     # before any launch
    assert lib.adamvs_dsm_open(4, 4, None, 1, None, 0, None, None) < 0


# ---- the analytic scenes of the GPU tests, on the reference alone ---------------------------------------------------------
def test_plane_flags_nothing_and_boxes_are_flagged_completely():
    radius, dh = schedule(0.5)
    z, _, _ = plane_scene(boxes=())
    res = pmf(z, radius, dh)
    assert res["counts"]["object"] == 0 and (res["level"] == 0).all()
    z, _, mask = plane_scene()
    res = pmf(z, radius, dh)
    assert np.array_equal(res["level"] != 0, mask)
    assert res["counts"] == dict(valid=z.size, ground=int(z.size - mask.sum()), object=int(mask.sum()), empty=0,
                                 per_level=res["counts"]["per_level"])
    assert sum(res["counts"]["per_level"]) == mask.sum() == 25 * 30 + 4 * 3


def test_a_box_wider_than_the_largest_window_is_kept_as_ground():
    """On level ground the 80 x 80 box survives every opening.  On the sloping plane of the other scene it does not count as
    a premise: there the openings of the last level take more than dh_max off the high side of the box's sloping roof (the
    documented limit of the dh_max cap), and the restatement flags part of the box at that level and nothing else."""
    radius, dh = schedule(0.5)
    z, _, mask = plane_scene(boxes=WIDE_BOX, gradients=(0.0, 0.0))
    assert mask.sum() == 6400
    res = pmf(z, radius, dh)
    assert (res["level"] == 0).all() and res["opened"].tobytes() == z.tobytes()
    z, _, mask = plane_scene(boxes=WIDE_BOX)
    res = pmf(z, radius, dh)
    assert res["counts"]["per_level"][:-1] == [0] * 5 and 0 < res["counts"]["per_level"][-1] < mask.sum()
    assert not (res["level"] != 0)[~mask].any()


def test_the_threshold_is_strict():
    """Z - O == dh exactly keeps the cell as ground; one fp32 step more flags it."""
    for top, flagged in ((np.float32(3.5), False), (np.nextafter(np.float32(3.5), np.float32(4)), True)):
        z = np.full((9, 9), 2.0, np.float32)
        z[4, 4] = top
        res = pmf(z, [1], [1.5])
        assert (res["level"][4, 4] == 1) == flagged and res["counts"]["object"] == int(flagged)
