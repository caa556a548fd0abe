"""Seam levelling on the CPU: the float64 restatement (tests/texture_level_ref.py) on hand cases with closed-form answers, its
minimum-norm solve against a dense least-squares solve and against plain conjugate gradients, its owner map and dilation
on a hand case, and the host side of ada_mvs_amd/texture.py: option checks, parser defaults, the new symbols, the ABI."""
import numpy as np
import pytest

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, texture
import texture_level_ref as L


def strip(cols_a, cols_b, extra=False):
    """Two rows of vertices, quads split into two triangles; the first cols_a quads are chart 0 (view 0), the next cols_b
    chart 1 (view 1); with extra, a detached quad of chart 2 (view 0).  -> faces, chart, uv, chart_view."""
    m = cols_a + cols_b
    faces, chart = [], []
    for i in range(m):
        a, b, c, d = 2 * i, 2 * i + 2, 2 * i + 3, 2 * i + 1
        faces += [(a, b, c), (a, c, d)]
        chart += [0 if i < cols_a else 1] * 2
    nv = 2 * (m + 1)
    xy = [(1.0 + (k // 2), 1.0 + (k % 2)) for k in range(nv)]
    view = [0, 1]
    if extra:
        faces += [(nv, nv + 1, nv + 2), (nv, nv + 2, nv + 3)]
        chart += [2, 2]
        xy += [(3.0, 5.0), (4.0, 5.0), (4.0, 6.0), (3.0, 6.0)]
        view.append(0)
    faces = np.array(faces, np.int64)
    uv = np.array([[c for k in f for c in xy[k]] for f in faces])
    return faces, np.array(chart), uv, np.array(view)


def flat(colour, size=24):
    img = np.zeros((size, size, 3))
    img[:] = colour
    return img


def test_two_charts_in_a_strip_have_the_closed_form_answer():
    faces, chart, uv, view = strip(3, 5, extra=True)
    fa, d = np.array([100.0, 50.0, 20.0]), np.array([8.0, -6.0, 0.0])
    r = L.level(faces, chart, uv, view, [flat(fa), flat(fa + d)], 0.1)
    na, nb = (r["node_chart"] == 0).sum(), (r["node_chart"] == 1).sum()
    assert (na, nb) == (8, 12) and len(r["data"]) == 2 and r["seam"].sum() == 2     # the shared column: one edge per chart
    for c, want in ((0, d * nb / (na + nb)), (1, -d * na / (na + nb)), (2, 0.0 * d)):
        np.testing.assert_allclose(r["g"][r["node_chart"] == c], np.broadcast_to(want, ((r["node_chart"] == c).sum(), 3)), atol=1e-10)
    v = r["f"] + r["g"]
    assert np.abs(v[r["data"][:, 0]] - v[r["data"][:, 1]]).max() < 1e-10            # every seam difference is gone
    assert (r["g"][r["node_chart"] == 2] == 0.0).all() or np.abs(r["g"][r["node_chart"] == 2]).max() < 1e-12


def test_graph_definition_on_the_strip():
    faces, chart, uv, view = strip(1, 1)
    nv_, nc_, corner = L.nodes(faces, chart)
    # vertices 0..5; the middle column (2, 3) belongs to both charts
    assert list(zip(nv_, nc_)) == [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (4, 1), (5, 1)]
    smooth, seam, data = L.edges(faces, chart, corner)
    assert [tuple(e) for e in data] == [(2, 3), (4, 5)]
    assert len(smooth) == 10 and [tuple(e) for e in smooth[seam]] == [(2, 4), (3, 5)]
    s2, m2, d2 = L.edges_fast(faces, chart, corner)
    np.testing.assert_array_equal(s2, smooth)
    np.testing.assert_array_equal(m2, seam)
    np.testing.assert_array_equal(d2, data)
    # an untextured face contributes nothing
    chart2 = chart.copy()
    chart2[:2] = -1
    assert len(L.nodes(faces, chart2)[0]) == 4 and len(L.edges(faces, chart2, L.nodes(faces, chart2)[2])[2]) == 0


def test_observed_colour_averages_along_the_seam():
    faces, chart, uv, view = strip(1, 1)
    img = np.zeros((8, 8, 3))
    img[..., 0] = np.arange(8)[None, :] * 10.0           # R = 10 x
    img[..., 1] = np.arange(8)[:, None] * 4.0            # G = 4 y
    r = L.level(faces, chart, uv, view, [img, img], 0.1)
    # node (2, 0) at (2, 1) has the seam edge to (3, 0) at (2, 2): samples at y = 1, 1.25, 1.5 with weights 1, 3/4, 1/2
    i = 2
    assert tuple(r["pos"][i]) == (2.0, 1.0)
    np.testing.assert_allclose(r["f"][i], [20.0, 4.0 * (1.0 + 0.75 * 1.25 + 0.5 * 1.5) / 2.25, 0.0], atol=1e-12)
    # node (0, 0) has no seam edge: the single sample
    np.testing.assert_allclose(r["f"][0], [10.0, 4.0, 0.0], atol=1e-12)


def test_minimum_norm_solve_is_linear_and_equals_lstsq_and_cg():
    faces, chart, uv, view = strip(4, 3, extra=True)
    rng = np.random.default_rng(5)
    nv_, nc_, corner = L.nodes(faces, chart)
    smooth, seam, data = L.edges(faces, chart, corner)
    n = len(nv_)
    Lm = L.laplacian(n, smooth, data, 0.1)
    comp = L.components(n, [smooth, data])
    assert len(np.unique(comp)) == 2
    np.testing.assert_allclose(Lm.sum(1), 0.0, atol=1e-12)
    f1, f2 = rng.uniform(0, 255, (n, 3)), rng.uniform(0, 255, (n, 3))
    g1, g2 = (L.min_norm(Lm, L.rhs(f, data, n), comp) for f in (f1, f2))
    g12 = L.min_norm(Lm, L.rhs(f1 + 2.0 * f2, data, n), comp)
    np.testing.assert_allclose(g12, g1 + 2.0 * g2, atol=1e-9)
    np.testing.assert_allclose(g1, np.linalg.lstsq(Lm, L.rhs(f1, data, n), rcond=None)[0], atol=1e-9)
    for c in np.unique(comp):
        assert np.abs(g1[comp == c].sum(0)).max() < 1e-9                          # minimum norm: zero mean per component
    gc, it = L.cg(Lm, L.rhs(f1, data, n), 1e-12, 10 * n)
    assert it < 10 * n
    np.testing.assert_allclose(gc, g1, atol=1e-8)
    assert L.cg(Lm, np.zeros((n, 3)), 1e-4, 10)[1] == 0                            # b = 0: no iteration


def test_owner_dilation_and_levelled_values_on_a_hand_case():
    # one chart of two faces in a 9 x 9 box at (10, 20) of its view, placed at (3, 4) of page 0
    uv = np.array([[12.0, 22.0, 12.0, 26.0, 16.0, 22.0], [16.0, 22.0, 12.0, 26.0, 16.0, 26.0]])
    chart = np.array([0, 0])
    charts = np.array([[10, 20, 9, 9, 3, 4, 0, 0]])
    prefix = np.array([0, 81])
    own = L.owner_map(uv, chart, charts, prefix).reshape(9, 9)
    assert own[2, 2] == 0 and own[6, 6] == 1 and own[4, 4] == 0        # the diagonal belongs to both: the smaller face
    assert (own[2:7, 2:7] != L.UNOWNED).all() and (own != L.UNOWNED).sum() == 25
    dil = L.dilate(own.reshape(-1), charts, prefix).reshape(9, 9)
    assert (dil != L.UNOWNED).all() and dil[0, 0] == 0 and dil[8, 8] == 1
    np.testing.assert_array_equal(dil[2:7, 2:7], own[2:7, 2:7])
    corner = np.array([[0, 1, 2], [2, 1, 3]])
    g = np.array([[0.0] * 3, [4.0] * 3, [8.0] * 3, [12.0] * 3])
    atlas = np.full((1, 16, 16, 3), 100, np.uint8)
    owned, val, pg, ax, ay = L.levelled_values(atlas, dil.reshape(-1), uv, corner, g, charts, prefix)
    val = val.reshape(9, 9, 3)
    assert val[2, 2, 0] == 100.0 and val[2, 6, 0] == 108.0 and val[6, 2, 0] == 104.0 and val[6, 6, 0] == 112.0
    assert val[4, 4, 0] == 106.0 and val[0, 0, 0] == 100.0 and val[8, 8, 0] == 112.0       # the band is clamped to the corners' range
    assert (ax.reshape(9, 9)[0] == np.arange(3, 12)).all() and (ay.reshape(9, 9)[:, 0] == np.arange(4, 13)).all()


def test_seam_options_parser_symbols_and_abi():
    for lam, tol, iters in ((0.0, 1e-4, 10), (-1.0, 1e-4, 10), (float("inf"), 1e-4, 10), (float("nan"), 1e-4, 10), (0.1, -1e-4, 10),
                            (0.1, float("nan"), 10), (0.1, 1e-4, -1), (0.1, 1e-4, 2.5), (0.1, 1e-4, True)):
        with pytest.raises(ValueError):
            texture.check_seam_options(lam, tol, iters)
    texture.check_seam_options(0.1, 0.0, 0)
    a = texture.build_parser().parse_args(["--data_folder", "d", "--output_folder", "o"])
    assert (a.seam_level, a.seam_lambda, a.seam_tol, a.seam_iters) == (False, 0.1, 1e-4, 1000)
    a = texture.build_parser().parse_args(["--data_folder", "d", "--output_folder", "o", "--seam_level", "--seam_lambda", "0.5",
                                           "--seam_tol", "1e-6", "--seam_iters", "50"])
    assert (a.seam_level, a.seam_lambda, a.seam_tol, a.seam_iters) == (True, 0.5, 1e-6, 50)
    assert _lib.ABI_VERSION == 22
    for name in ("observe", "rhs", "cg_init", "cg", "owner", "dilate", "apply"):
        assert "adamvs_texture_level_" + name in _lib.SIGNATURES
    assert texture.PHASES == ("project_zbuf", "score", "components", "boxes", "fill_coords")       # unchanged when the step is off
    assert texture.LEVEL_PHASES == ("level_graph", "level_solve", "level_apply")
    assert texture.LEVEL_BAND == _lib.TEXTURE_LEVEL_BAND == L.BAND == 2
    assert texture.LEVEL_MAX_NODES == _lib.TEXTURE_LEVEL_MAX_NODES
    import inspect
    for fn in (texture.texture_mesh, texture.from_folder):
        p = inspect.signature(fn).parameters
        assert p["seam_level"].default is False and p["seam_lambda"].default == 0.1 and p["seam_tol"].default == 1e-4
        assert p["seam_iters"].default == 1000


# ---- the restatements of the single kernels (tests/level_kernels_ref.py) ------------------------------------------------------------
import level_kernels_ref as K


def edge_lists(g):
    """The CSR's undirected edges among the nodes -> (smooth [ms, 2], seam [ms] bool, data [md, 2]) as texture_level_ref takes them."""
    word = g["col"].astype(np.int64)
    j = word & K.INDEX
    up = (g["row"] < j) & (j < g["n"])
    e = np.stack([g["row"][up], j[up]], 1)
    is_data = (word[up] & K.DATA) != 0
    return e[~is_data], (word[up][~is_data] & K.SEAM) != 0, e[is_data]


def test_graph_generator_places_what_it_states():
    for n in (1, 2, 3, 255, 400, 5000):
        g = K.random_graph(n, seed=n)
        rp, word = g["rowptr"].astype(np.int64), g["col"].astype(np.int64)
        j = word & K.INDEX
        assert rp[0] == 0 and rp[-1] == len(word) and len(rp) == n + 1 and (np.diff(rp) >= 0).all()
        same = g["row"][1:] == g["row"][:-1]
        assert (j[1:][same] > j[:-1][same]).all()                                   # sorted by neighbour, no duplicates
        assert (j != g["row"]).all()
        inside = j < n
        assert 1 <= (~inside).sum() <= 5 and j.max() == (K.INDEX if n >= 2 else n)   # stray words, one of them the largest index
        A = K.laplacian_sparse(g, 10.0)
        assert abs(A - A.T).max() == 0 and abs(A.sum(1)).max() < 1e-9
        if n >= 400:
            assert tuple(K.degrees(g)[g["special"]]) == K.SPECIAL_DEGREES and g["special"][0] == 0 and g["special"][1] == n - 1
            kinds = word[inside] >> 30
            assert all((kinds == k).mean() > 0.2 for k in (0, 1, 2))
    up = K.random_graph(500, seed=1, upper_only=True)
    assert ((up["col"].astype(np.int64) & K.INDEX) > up["row"]).all()
    eq = K.equitable_graph(7 * 40 + 3, seed=2)
    assert (K.degrees(eq)[:280] == 6).all() and (K.degrees(eq)[280:] == 0).all()
    # equitable: L maps a vector that is constant on the blocks to one that is constant on the blocks
    x = np.random.default_rng(0).normal(size=8)[eq["block"]]
    y = K.laplacian_sparse(eq, 2.0) @ x
    assert all(np.ptp(y[eq["block"] == c]) < 1e-12 for c in range(8))


def test_ordered_spmv_and_rhs_equal_the_dense_definition():
    """Per row the ordered sums make deg - 1 additions of d (exact here: the weights are 1 and 10), deg products and deg - 1
    additions for s, one product d p_i and one subtraction: at most (deg + 2) roundings, each relative to a partial sum that
    the row's sum of |terms| bounds.  The yardstick is the dense Laplacian applied in longdouble."""
    n = 600
    g = K.random_graph(n, seed=11)
    smooth, seam, data = edge_lists(g)
    p = np.random.default_rng(3).normal(size=(n, 3))
    Lm = L.laplacian(n, smooth, data, 0.1)
    want = Lm.astype(np.longdouble) @ p.astype(np.longdouble)
    terms = np.abs(Lm) @ np.abs(p)
    got = K.spmv_ordered(g, p, 1.0 / 0.1)
    bound = (K.degrees(g)[:, None] + 2) * K.U64 * terms
    assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / np.maximum(bound, 1e-300)).max()
    assert np.abs(got - Lm @ p).max() <= 2 * bound.max()
    np.testing.assert_allclose(K.laplacian_sparse(g, 10.0).toarray(), Lm, atol=0, rtol=0)
    assert (got[K.degrees(g) == 0] == 0).all()
    # b: the data entries alone, (double)f_j - (double)f_i summed in order; every term is exact, the sum makes deg - 1 roundings
    f = np.random.default_rng(4).uniform(0, 255, (n, 3)).astype(np.float32)
    b = K.rhs_ordered(g, f)
    ref = L.rhs(f.astype(np.float64), data, n)
    dd = np.bincount(data.reshape(-1), minlength=n)
    assert (np.abs(b - ref) <= (2 * dd[:, None]) * K.U64 * 2 * 255.0 * np.maximum(dd[:, None], 1)).all()
    assert (b[dd == 0] == 0).all()


def test_sparse_cg_equals_the_dense_cg():
    """Two fp64 runs of conjugate gradients that differ only in the order of their sums drift apart by about (iterations x
    condition number x 2^-53) |g|.  With lambda = 1 every weight is 1 and the condition number of a random graph of six neighbours
    is some tens, so some tens of iterations leave the difference well below the 1e-12 max |g| asked for."""
    n = 300
    g = K.random_graph(n, seed=12, special=False)
    smooth, seam, data = edge_lists(g)
    f = np.random.default_rng(5).uniform(0, 255, (n, 3))
    b = L.rhs(f, data, n)
    Lm = L.laplacian(n, smooth, data, 1.0)
    gd, itd = L.cg(Lm, b, 1e-8, 5000)
    gs, its, hist = K.cg_sparse(K.laplacian_sparse(g, 1.0), b, 1e-8, 5000)
    assert its == itd and 10 < its < 200 and len(hist) == its + 1 and hist[-1] <= 1e-8 < hist[-2]
    print("sparse against dense cg: %d iterations, max |dg| = %.3g of max |g| = %.3g" % (its, np.abs(gs - gd).max(), np.abs(gd).max()))
    assert np.abs(gs - gd).max() <= 1e-12 * np.abs(gd).max()


def test_a_refused_step_restarts_from_the_residual():
    """alpha = 0 with r.r unchanged gave beta = 1 and p = r + p: p doubled every iteration, overflowed after about 1024 and
    0 * inf = NaN reached g.  The definition now takes beta = 0 there."""
    b = np.array([[3.0, -2.0, 0.0], [1.0, 0.5, 0.0]])
    with np.errstate(all="raise"):
        gd, it = L.cg(np.zeros((2, 2)), b, 1e-4, 1100)
        gs, its, _ = K.cg_sparse(K.laplacian_sparse(K.csr(2, [], [], []), 10.0), b, 1e-4, 1100)
    assert it == its == 1100 and (gd == 0).all() and (gs == 0).all()


def test_fp32_observed_colour_restatement_agrees_with_the_definition():
    n, W, H = 500, 31, 24
    rng = np.random.default_rng(6)
    g = K.random_graph(n, seed=13)
    smooth, seam, data = edge_lists(g)
    images = [rng.integers(0, 256, (H, W, 4), dtype=np.uint8) for _ in range(2)]
    view = rng.integers(0, 2, n)
    pos = (rng.uniform(0, 1, (n, 2)) * [W - 1, H - 1]).astype(np.float32)
    got = K.observe32(g, pos, view, images)
    want = L.observe(pos.astype(np.float64), view, smooth, seam, images)
    deg = np.bincount(smooth[seam].reshape(-1), minlength=n).max()
    bound = 255.0 * 2.0 ** -24 * (4 * max(W, H) + 11 + 2 * 3 * deg + 1)                # f_bound of tests/test_texture_level_gpu.py
    err = np.abs(got - want).max()
    assert deg >= 10 and 0 < err <= bound, (err, bound)
    # a view out of range gives 0; a node without a seam entry takes the single sample
    view2 = view.copy()
    view2[:7] = [-1, 2, -5, 2, 7, -1, 2]
    got2 = K.observe32(g, pos, view2, images)
    assert (got2[:7] == 0).all()
    none = np.bincount(smooth[seam].reshape(-1), minlength=n) == 0
    assert none.any()
    np.testing.assert_array_equal(got[none], K.sample_views32(images, view[none], pos[none, 0], pos[none, 1]))
