"""CPU-only checks of the orthophoto's radiometric balance (ada_mvs_amd/ortho.py): solve_gains against the restatement
(tests/ortho_balance_ref.py) and on cases with a known answer, the option and range checks, default_stride at the cap, the
CLI's defaults, and the new entry points' argument checks (no launch)."""
import ctypes

import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, dsm as dsm_mod, ortho
import ortho_balance_ref as B


def random_stats(rng, V, P, lo=1, hi=5000):
    """P distinct pairs of V views in lexicographic order with plausible sums: n cells of means 20 .. 235 levels."""
    every = np.array([(a, b) for a in range(V) for b in range(a + 1, V)])
    pairs = every[np.sort(rng.choice(len(every), P, replace=False))]
    n = rng.integers(lo, hi, P)
    stats = np.zeros((P, 7), np.int64)
    stats[:, 0] = n
    for k in range(6):
        stats[:, 1 + k] = np.floor(n * 64 * rng.uniform(20.0, 235.0, P)).astype(np.int64)
    return pairs, stats


@pytest.mark.parametrize("V,P,sig", [(2, 1, (10.0, 0.1)), (5, 10, (10.0, 0.1)), (12, 30, (10.0, 10.0)), (40, 200, (3.0, 0.5))])
def test_solve_gains_agrees_with_the_restatement(V, P, sig):
    rng = np.random.default_rng(V)
    pairs, stats = random_stats(rng, V, P, lo=64)
    stats[3::4, 0] = 63                                              # one short of min_samples: those pairs are left out
    got = ortho.solve_gains(pairs, stats, V, sig[0], sig[1], 64)
    ref = B.solve_gains(pairs, stats, V, sig[0], sig[1], 64)
    for g, r in zip(got, ref):
        np.testing.assert_allclose(g, r, rtol=1e-12, atol=0.0)


def test_equal_means_give_gain_one():
    rng = np.random.default_rng(1)
    pairs, stats = random_stats(rng, 6, 12, lo=64)
    stats[:, 4:7] = stats[:, 1:4]
    g, before, after = ortho.solve_gains(pairs, stats, 6)
    np.testing.assert_allclose(g, 1.0, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(before, 0.0, atol=1e-12)
    np.testing.assert_allclose(after, 0.0, atol=1e-9)


def test_a_view_without_a_pair_of_enough_samples_gets_exactly_one():
    pairs = np.array([(0, 1), (0, 3), (1, 2), (2, 3)])
    stats = np.array([[500, 6400000, 6400000, 6400000, 7000000, 7000000, 7000000],
                      [63, 403200, 403200, 403200, 500000, 500000, 500000],
                      [900, 9000000, 9000000, 9000000, 8000000, 8000000, 8000000],
                      [10, 64000, 64000, 64000, 99000, 99000, 99000]])
    g, _, _ = ortho.solve_gains(pairs, stats, 5)
    assert (g[3] == 1.0).all() and (g[4] == 1.0).all()              # view 3 has pairs of 63 and 10 cells only, view 4 none
    assert (g[:3] != 1.0).all()
    g64, _, _ = ortho.solve_gains(pairs, stats, 5, min_samples=63)
    assert (g64[3] != 1.0).all() and (g64[4] == 1.0).all()


def test_disconnected_groups_solve_as_they_do_alone():
    rng = np.random.default_rng(2)
    p1, s1 = random_stats(rng, 4, 5, lo=64)
    p2, s2 = random_stats(rng, 3, 3, lo=64)
    g1 = ortho.solve_gains(p1, s1, 4)[0]
    g2 = ortho.solve_gains(p2, s2, 3)[0]
    both = ortho.solve_gains(np.concatenate([p1, p2 + 4]), np.concatenate([s1, s2]), 7)[0]
    np.testing.assert_allclose(both[:4], g1, rtol=1e-12)
    np.testing.assert_allclose(both[4:], g2, rtol=1e-12)


@pytest.mark.parametrize("gain_sigma", [0.1, 10.0])
def test_a_scaled_view_is_pulled_towards_the_others(gain_sigma):
    """Three views of equal means; view 0's sums scaled by gamma: g_0 gamma moves towards the others' g (and all the way for a
    weak prior)."""
    gamma = 1.25
    pairs = np.array([(0, 1), (0, 2), (1, 2)])
    n, mean_q = 2000, 64 * 120
    stats = np.array([[n] + [n * mean_q] * 6] * 3, np.int64)
    stats[:2, 1:4] = np.round(stats[:2, 1:4] * gamma).astype(np.int64)
    g, before, after = ortho.solve_gains(pairs, stats, 3, gain_sigma=gain_sigma)
    spread_before = gamma - 1.0
    spread_after = np.abs(g[0] * gamma - g[1:].mean(0))
    assert (spread_after < 0.5 * spread_before).all(), spread_after
    assert (g[0] < 1.0).all() and (g[1:] > 1.0).all()
    assert (after < before).all()
    if gain_sigma == 10.0:
        assert (spread_after < 1e-3).all(), spread_after


@pytest.mark.parametrize("kw", [dict(V=0), dict(V=4097), dict(noise_sigma=0.0), dict(noise_sigma=float("nan")), dict(gain_sigma=0.0),
                                dict(gain_sigma=100.5), dict(gain_sigma=float("inf")), dict(min_samples=0), dict(min_samples=1.5)])
def test_solve_gains_refuses_bad_options(kw):
    args = dict(V=2, noise_sigma=10.0, gain_sigma=0.1, min_samples=64)
    args.update(kw)
    with pytest.raises(ValueError):
        ortho.solve_gains(np.array([(0, 1)]), np.array([[100] + [640000] * 6]), **args)


def test_solve_gains_refuses_bad_pairs():
    s = np.array([[100] + [640000] * 6])
    for pair in ((1, 1), (1, 0), (0, 2), (-1, 1)):
        with pytest.raises(ValueError):
            ortho.solve_gains(np.array([pair]), s, 2)
    with pytest.raises(ValueError):
        ortho.solve_gains(np.array([(0, 1), (0, 1)]), s, 2)          # two pairs, one row


@pytest.mark.parametrize("kw", [dict(balance="offset"), dict(balance=True), dict(stride=0), dict(stride=1.5), dict(stride=1),
                                dict(max_diff=-1.0), dict(max_diff=255.5), dict(max_diff=float("nan")), dict(gain_sigma=-0.1)])
def test_balance_options_are_checked(kw):
    grid = dsm_mod.Grid(0.0, 0.0, 1.0, 0.0, 2048, 1024)              # 2^21 cells: stride 1 is over the cap
    args = dict(balance="gain", stride=None, max_diff=255.0, gain_sigma=0.1)
    args.update(kw)
    with pytest.raises(ValueError):
        ortho.check_balance_options(args["balance"], 10.0, args["gain_sigma"], args["stride"], args["max_diff"], 64, grid)
    assert ortho.check_balance_options("gain", 10.0, 0.1, 2, 8.0, 64, grid) == (2, 512)
    assert ortho.check_balance_options("gain", grid=grid) == (None, 16320)


def test_default_stride_at_the_cap():
    def g(W, H):
        return dsm_mod.Grid(0.0, 0.0, 1.0, 0.0, W, H)
    assert ortho.default_stride(g(1 << 20, 1)) == 1                  # N_s = 2^20
    assert ortho.default_stride(g((1 << 20) + 1, 1)) == 2            # 2^20 + 1 cells
    assert ortho.default_stride(g(1024, 1024)) == 1
    assert ortho.default_stride(g(1025, 1024)) == 2
    assert ortho.default_stride(g(320, 260)) == 1
    assert ortho.default_stride(g(1, 1)) == 1
    for W, H in ((2125, 3000), (16384, 16384), (5000, 333), (3, 1 << 22)):
        S = ortho.default_stride(g(W, H))
        ws, hs = ortho.lattice_shape(g(W, H), S)
        assert ws * hs <= 1 << 20 and (ws, hs) == B.lattice_shape(g(W, H), S)
        ws, hs = ortho.lattice_shape(g(W, H), S - 1)
        assert ws * hs > 1 << 20


def test_cli_parser_leaves_the_balance_off():
    a = ortho.build_parser().parse_args(["--data_folder", "d", "--output_folder", "o", "--dsm", "p"])
    assert a.balance is None
    assert (a.gain_sigma, a.noise_sigma, a.balance_stride, a.balance_max_diff, a.balance_min_samples) == (0.1, 10.0, None, 255.0, 64)
    b = ortho.build_parser().parse_args(["--data_folder", "d", "--output_folder", "o", "--dsm", "p", "--balance", "gain", "--gain_sigma",
                                         "10", "--balance_stride", "3"])
    assert b.balance == "gain" and b.gain_sigma == 10.0 and b.balance_stride == 3
    with pytest.raises(SystemExit):
        ortho.build_parser().parse_args(["--data_folder", "d", "--output_folder", "o", "--dsm", "p", "--balance", "offset"])


def test_summary_has_a_balance_block_only_when_balancing():
    g = dsm_mod.Grid(0.0, 0.0, 1.0, 0.0, 2, 2)
    res = dict(grid=g, dsm_grid=g, upsample=1, mode="best", occlusion_tol=2.0, border_px=2.0, feather_px=64.0, views_used=[0],
               views_culled=[], cells_surface=4, cells_coloured=4, cells_unseen=0, device_seconds=0.0)
    assert "balance" not in ortho.summary(res)
    assert ortho.summary(dict(res, balance=dict(model="gain")))["balance"] == dict(model="gain")


def test_abi_refuses_bad_balance_arguments():
    """Every argument is checked before any launch, so the checks run without a GPU (the pointers are never followed)."""
    lib = _lib.load()
    assert (_lib.ORTHO_BAL_MAX_SAMPLES, _lib.ORTHO_BAL_CHUNK, _lib.ORTHO_BAL_MAX_Q) == (1 << 20, 8192, B.MAX_Q)
    assert ortho.BAL_MAX_SAMPLES == _lib.ORTHO_BAL_MAX_SAMPLES and ortho.BAL_Q == B.Q
    p = ctypes.c_void_p(256)                                         # a non-null address that is never read
    ps = lib.adamvs_ortho_pair_stats
    assert ps(p, 0, 10, p, 1, 0, p, None) < 0                        # V < 1
    assert ps(p, 2, 10, p, -1, 0, p, None) < 0                       # P < 0
    assert ps(p, 2, 0, p, 1, 0, p, None) < 0                         # N_s < 1
    assert ps(p, 2, (1 << 20) + 1, p, 1, 0, p, None) < 0             # N_s over the cap
    assert ps(p, 2, 10, p, 1, -1, p, None) < 0 and ps(p, 2, 10, p, 1, 16321, p, None) < 0
    assert ps(None, 2, 10, p, 1, 0, p, None) < 0 and ps(p, 2, 10, None, 1, 0, p, None) < 0 and ps(p, 2, 10, p, 1, 0, None, None) < 0
    assert ps(p, 2, 10, p, 0, 16320, p, None) == 0                   # P = 0: nothing to do, no launch
    adj = lib.adamvs_ortho_adjust_image
    ok = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    q = ctypes.c_void_p(512)
    assert adj(p, 0, 4, ok, q, None) < 0 and adj(p, 4, 0, ok, q, None) < 0
    assert adj(None, 4, 4, ok, q, None) < 0 and adj(p, 4, 4, None, q, None) < 0 and adj(p, 4, 4, ok, None, None) < 0
    assert adj(p, 4, 4, ok, p, None) < 0                             # aliased
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert adj(p, 4, 4, (ctypes.c_float * 3)(1.0, bad, 1.0), q, None) < 0
    grid = _lib.OrthoGrid()
    grid.x0, grid.y_top, grid.gsd, grid.W, grid.H, grid.K = 0.0, 0.0, 1.0, 2048, 1024, 1
    view = _lib.OrthoView()
    view.C[:], view.R[:], view.K[:] = [0.0] * 3, [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], [100.0, 0, 50.0, 0, 100.0, 50.0, 0, 0, 1.0]
    view.H, view.W, view.rgba = 100, 100, 256
    obs = lib.adamvs_ortho_observe
    assert obs(ctypes.byref(grid), p, ctypes.byref(view), p, 0, 2.0, 2.0, p, None) < 0          # S < 1
    assert obs(ctypes.byref(grid), p, ctypes.byref(view), p, 1, 2.0, 2.0, p, None) < 0          # 2^21 lattice cells
    assert obs(ctypes.byref(grid), None, ctypes.byref(view), p, 2, 2.0, 2.0, p, None) < 0
    assert obs(ctypes.byref(grid), p, ctypes.byref(view), None, 2, 2.0, 2.0, p, None) < 0
    assert obs(ctypes.byref(grid), p, ctypes.byref(view), p, 2, 2.0, 2.0, None, None) < 0
    assert obs(ctypes.byref(grid), p, ctypes.byref(view), p, 2, -1.0, 2.0, p, None) < 0
    assert obs(ctypes.byref(grid), p, ctypes.byref(view), p, 2, 2.0, float("nan"), p, None) < 0
    assert obs(None, p, ctypes.byref(view), p, 2, 2.0, 2.0, p, None) < 0
    seam = lib.adamvs_ortho_seam_stats
    assert seam(ctypes.byref(grid), None, p, p, None) < 0 and seam(ctypes.byref(grid), p, None, p, None) < 0
    assert seam(ctypes.byref(grid), p, p, None, None) < 0 and seam(None, p, p, p, None) < 0
    grid.K = 9
    assert seam(ctypes.byref(grid), p, p, p, None) < 0
