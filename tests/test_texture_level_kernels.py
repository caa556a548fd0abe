"""The seam-levelling kernels (csrc/texture_level.hip) one call at a time, on synthetic CSR graphs and hand-built charts, against
the restatements of tests/level_kernels_ref.py (the kernels' own order of operations) and tests/texture_level_ref.py (the
definition).  No mesh, no cameras, no texture_mesh.  The file is compiled without contraction and the header states every
operation, so vectors are compared bit for bit; the dot products, whose summation tree numpy cannot restate cheaply, are held
to the bound of that tree (level_kernels_ref.dot_path) against longdouble sums.

Graph sizes n (SIZES) and what they turn.  The workgroups are nb = min(ceil(n / 256), 2048), each owning chunk = ceil(n / nb)
rows and pchunk = ceil(ceil(3 n / 2) / nb) 16-byte pairs.

kernel               held by                                     loops: zero times / once / more than once
k_lvl_observe        test_observe                                row entries: degree 0 / 1 / 7 .. 40 (SPECIAL_DEGREES); seam entries none
                                                                 / one / several; images 1 x 1, 2 x 3, 257 x 3
k_lvl_rhs            test_rhs                                    row entries as above; n = 1 .. 1 050 631, more than one block from 257
k_lvl_init           test_stop_protocol, test_whole_solve,       row loop (i += 256): lanes past the chunk and blocks past n / n <= 524 288
                     test_degenerate_solves                      / twice at n = 524 289 (chunk 257), three times at 1 050 631 (chunk 513)
k_lvl_spmv           test_cg_step (Ap bit for bit)               row loop as k_lvl_init; batches of 8: degree 0 / 1, 7, 8 / 9, 16 (two),
                                                                 17 (three), 40 (five); words with index >= n skipped
k_lvl_reduce_*       test_cg_step (alpha, beta, r.r), test_stop_ partials loop (k += 256): lanes past nb / nb <= 256 / twice at
(total3, block_sum3) protocol, test_degenerate_solves            n = 65 797 (nb 258), eight times at nb = 2048; guards p.Ap <= 0, r.r = 0
k_lvl_update_xr      test_cg_step (g, r bit for bit; r.r bound)  pair loop (e += 256): lanes past pchunk / n <= 349 525 / twice at 524 289
                                                                 (pchunk 385), four times at 1 050 631 (pchunk 770); 3 n odd and even
k_lvl_update_p       test_cg_step (p bit for bit)                as k_lvl_update_xr
stop flag            test_stop_protocol                          every kernel after the flag returns without a write
k_lvl_owner_clear,   test_owner_and_dilation                     pixel loops: boxes of 1 .. 16 centres; list split at 16 / 17 centres
k_lvl_owner_small
k_lvl_owner_large    test_owner_and_dilation                     wave-stride loop: > 40 000 listed faces against at most 256 CUs x 8
                                                                 workgroups x 4 waves resident; lane loop: boxes of 17 .. 64 centres once,
                                                                 of more than 64 twice and more
lvl_chart_of         test_owner_and_dilation, test_apply         3000 charts (12 halvings), empty boxes first, in the middle and last
k_lvl_dilate         test_owner_and_dilation                     1 x 1, 1 x h, w x 1 boxes (neighbourhood cut on every side)
k_lvl_apply          test_apply                                  skips: texel outside its page, page out of range, corner_node out of range

The derived bounds are the bars.  Every test prints the share of its bound that it measured; no run on an MI355X has been
recorded here yet, so the shares are still to be written into the tests' docstrings after the first one."""
import functools

import numpy as np
import pytest
import torch

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, hip_ops
from ada_mvs_amd._lib import check
import level_kernels_ref as K
import texture_level_ref as L

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 255, 256, 257, 256 * 257 + 5, 2048 * 256 + 1, 2048 * 513 + 7)
LAM = 0.1                            # 1 / LAM = 10 exactly: smoothness entries weigh 10, data entries 1
GROW_PX = 2e-3                       # owner decisions within this many pixels of an edge are set aside (tests/test_texture_gpu.py)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d entries differ, the first at %s: %r against %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


@functools.lru_cache(maxsize=None)
def graph(n, upper_only=False):
    return K.random_graph(n, seed=1000 + n, upper_only=upper_only)


def graph_dev(g):
    return dev(g["rowptr"]), dev(g["col"].view(np.int32))


def ptr(t):
    return hip_ops._p(t)


# ---- 1. graph kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_rhs(n):
    """b against the float64 sum of (double)f_j - (double)f_i over the data entries in ascending order: bit for bit."""
    g = graph(n)
    f = np.random.default_rng(n).uniform(0, 255, (n, 3)).astype(np.float32)
    rowptr, col = graph_dev(g)
    got = hip_ops.texture_level_rhs(rowptr, col, dev(f)).cpu().numpy()
    assert_bits(got, K.rhs_ordered(g, f), "b")
    assert n < 400 or np.abs(got).max() > 0


@pytest.mark.parametrize("n", (1, 2, 3, 255, 257, 256 * 257 + 5))
def test_observe(n):
    """f against the fp32 restatement of lvl_sample and the weighted mean: bit for bit (fp32 division is correctly rounded).
    Views of 1 x 1, 2 x 3 and 257 x 3 pixels; positions outside the image on every side, exactly on its corners and on
    W - 1, H - 1; node_view -1 and nviews; nodes without a usable seam entry; seam words with an index >= n."""
    rng = np.random.default_rng(7 * n)
    g = graph(n)
    dims = [(1, 1), (3, 2), (3, 257)]                               # (H, W)
    images = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for h, w in dims]
    view = rng.integers(-1, len(dims) + 1, n)
    hw = np.array(dims + [(3, 257)])[np.where((view >= 0) & (view < len(dims)), view, len(dims))]
    pos = rng.uniform(-2.0, 1.0, (n, 2)) + rng.uniform(0, 1, (n, 2)) * (hw[:, ::-1] + 2.0)
    on = rng.integers(0, 4, (n, 2))                                 # a quarter each: on 0, on W - 1 / H - 1, anywhere (twice)
    pos = np.where(on == 0, 0.0, np.where(on == 1, hw[:, ::-1] - 1.0, pos)).astype(np.float32)
    imgs_d = [dev(i) for i in images]
    tab = torch.tensor([[t.data_ptr(), w, h] for t, (h, w) in zip(imgs_d, dims)], dtype=torch.int64).cuda()
    rowptr, col = graph_dev(g)
    got = hip_ops.texture_level_observe(tab, rowptr, col, dev(view.astype(np.int32)), dev(pos)).cpu().numpy()
    want = K.observe32(g, pos, view, images)
    assert_bits(got, want, "f")
    valid = (view >= 0) & (view < len(dims))
    assert (got[~valid] == 0).all()
    if n >= 255:
        word = g["col"].astype(np.int64)
        seam = ((word & K.DATA) == 0) & ((word & K.SEAM) != 0)
        usable = np.bincount(g["row"][seam & ((word & K.INDEX) < n)], minlength=n)
        outside = ((pos < 0) | (pos > hw[:, ::-1] - 1)).any(1)
        assert (usable == 0).any() and (usable > 1).any() and (seam & ((word & K.INDEX) >= n)).any() or n < 400
        assert outside.any() and (~outside).any() and (~valid).any()


def cg_call(g, gd, lam, iters, G, R, P, AP, partials, state):
    check(_lib.load().adamvs_texture_level_cg(ptr(gd[0]), ptr(gd[1]), gd[1].numel(), g["n"], lam, iters, ptr(G), ptr(R), ptr(P), ptr(AP),
                                              ptr(partials), ptr(state), hip_ops._stream()), "texture_level_cg")


def spare(v):
    """[n, 3] -> device [n + 1, 3] whose spare row is NaN."""
    return dev(np.concatenate([v, np.full((1, 3), np.nan)]))


def one_step(g, lam, G, R, P, rr):
    """One iteration from (G, R, P) and a state holding r.r = rr, b.b = 1, tol^2 = 0, stop = 0; Ap, the partials and the spare
    rows start as NaN -> host copies of g, r, p, Ap [n + 1, 3] and state [16]."""
    n = g["n"]
    gd = graph_dev(g)
    state = np.zeros(16)
    state[K.ST_RR:K.ST_RR + 3], state[K.ST_BB:K.ST_BB + 3] = rr, 1.0
    Gd, Rd, Pd, APd = spare(G), spare(R), spare(P), dev(np.full((n + 1, 3), np.nan))
    partials, sd = dev(np.full(3 * K.BLOCKS, np.nan)), dev(state)
    cg_call(g, gd, lam, 1, Gd, Rd, Pd, APd, partials, sd)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (Gd, Rd, Pd, APd, sd)]


def check_step(n, upper_only, label):
    """-> the shares of their bounds that alpha, the new r.r and beta took."""
    g = graph(n, upper_only)
    rng = np.random.default_rng(31 * n + upper_only)
    G, R, P = (rng.normal(size=(n, 3)) for _ in range(3))
    rr = rng.uniform(0.5, 2.0, 3) * n
    if upper_only:
        # only the entries j > i are left: p.Ap = sum w (p_i^2 - p_i p_j), negative when p grows with the index
        P[:, 0] = 1.0 + np.arange(n) / n + 0.01 * rng.uniform(size=n)
        rr[1] = 0.0
    w = 1.0 / LAM
    nb, chunk, pairs, pchunk = K.grid(n)
    Ap = K.spmv_ordered(g, P, w)
    T, S = K.dot_ld(P, Ap)
    # p.Ap: chunk rows per workgroup, one term per row and channel -> dot_path(chunk, nb) additions on the longest path
    B = K.dot_path(chunk, nb) * K.U64 * S
    refused = T <= -B                                  # the GPU's sum is then certainly <= 0: alpha = 0
    assert (refused | (T >= 2 * B)).all(), "choose another seed: p.Ap = %s lies within its bound %s of 0" % (T, B)
    assert not upper_only or tuple(refused) == (True, False, False)
    G1, R1, P1, AP1, st = one_step(g, LAM, G, R, P, rr)
    # the spare row's NaN reaches nothing else
    for name, v in (("g", G1), ("r", R1), ("p", P1), ("Ap", AP1)):
        assert not np.isnan(v[:n]).any(), name
    assert not np.isnan(st).any() and st[K.ST_ITERS] == 1.0 and st[K.ST_DONE] == 0.0 and st[K.ST_TOL2] == 0.0
    assert_bits(AP1[:n], Ap, "Ap")
    alpha, beta, new = st[K.ST_ALPHA:K.ST_ALPHA + 3], st[K.ST_BETA:K.ST_BETA + 3], st[K.ST_RR:K.ST_RR + 3]
    assert_bits(G1[:n], G + alpha * P, "g + alpha p")
    r1 = R - alpha * Ap
    assert_bits(R1[:n], r1, "r - alpha Ap")
    assert_bits(P1[:n], r1 + beta * P, "r + beta p")
    assert (st[K.ST_BB:K.ST_BB + 3] == 1.0).all()
    # alpha = fl(rr / tot) with tot = T (1 + theta), |theta| <= eps = B / |T| < 1 / 2:  alpha / (rr / T) - 1 = (delta - theta) / (1 + theta)
    live = ~refused
    assert (alpha[refused] == 0.0).all() and (beta[refused] == 0.0).all()
    eps = np.where(live, B / np.where(live, np.abs(T), 1), 0)
    alpha_ld = np.where(live, rr / np.where(live, T, 1), 0)
    alpha_bound = np.abs(alpha_ld) * (eps + K.U64) / (1 - eps)
    alpha_err = np.abs(alpha - alpha_ld)
    # r'.r' over 16-byte pairs: pchunk pairs per workgroup, at most one term per pair and channel -> dot_path(pchunk, nb)
    N, _ = K.dot_ld(r1, r1)
    new_bound = K.dot_path(pchunk, nb) * K.U64 * N
    new_err = np.abs(new - N)
    # beta = fl(new / rr): the error of new divided by rr, and the division's own rounding
    has_beta = live & (rr > 0) & (alpha != 0)
    beta_ld = np.where(has_beta, N / np.where(rr > 0, rr, 1), 0)
    beta_bound = np.where(has_beta, new_bound / np.where(rr > 0, rr, 1) * (1 + K.U64) + K.U64 * np.abs(beta_ld), 0)
    beta_err = np.abs(beta - beta_ld)
    share = lambda e, b: float(np.max(np.where(b > 0, e / np.where(b > 0, b, 1), np.where(e > 0, np.inf, 0)).astype(np.float64)))
    shares = share(alpha_err, alpha_bound), share(new_err, new_bound), share(beta_err, beta_bound)
    print("cg step %s n = %d (nb %d, chunk %d, pchunk %d; path %d / %d): alpha %.3f, r.r %.3f, beta %.3f of the bound"
          % (label, n, nb, chunk, pchunk, K.dot_path(chunk, nb), K.dot_path(pchunk, nb), *shares))
    assert (alpha_err <= alpha_bound).all(), (alpha, alpha_ld, alpha_bound)
    assert (new_err <= new_bound).all(), (new, N, new_bound)
    assert (beta_err <= beta_bound).all(), (beta, beta_ld, beta_bound)
    assert (beta[~has_beta] == 0.0).all()
    return dict(g=g, P=P, rr=rr, alpha=alpha, alpha_ld=alpha_ld, alpha_bound=alpha_bound, live=live, w=w)


@pytest.mark.parametrize("n", SIZES)
def test_cg_step(n):
    """One iteration from an arbitrary state: Ap, g', r', p' bit for bit; alpha, beta and r'.r' within the bound of the fixed
    summation order against longdouble sums."""
    s = check_step(n, False, "symmetric")
    if n != 256 * 257 + 5:
        return
    # the yardstick is sharp: alpha with its channels rotated by one misses the bound, and so does alpha from p rounded to fp32
    assert s["live"].all()
    assert (np.abs(s["alpha"] - np.roll(s["alpha_ld"], 1)) > s["alpha_bound"]).all()
    P32 = s["P"].astype(np.float32).astype(np.float64)
    T32, _ = K.dot_ld(P32, K.spmv_ordered(s["g"], P32, s["w"]))
    assert (np.abs(s["alpha"] - s["rr"] / T32) > s["alpha_bound"]).all()


@pytest.mark.parametrize("n", (257, 256 * 257 + 5))
def test_cg_step_guards(n):
    """A matrix that is neither symmetric nor definite (only the entries j > i): channel 0 has p.Ap < 0 (alpha 0), channel 1 has
    r.r = 0 (alpha 0, beta 0), channel 2 steps as usual.  A refused step takes beta = 0."""
    check_step(n, True, "guards")


def solve_raw(g, b, lam, tol, iters, groups=1):
    """cg_init, then `groups` calls of `iters` iterations, on buffers of the test's own -> device (g, r, p, state) and a call
    that queues more."""
    n = g["n"]
    gd = graph_dev(g)
    G, R, P, AP = (torch.zeros(n + 1, 3, device="cuda", dtype=torch.float64) for _ in range(4))
    partials, state = torch.zeros(3 * K.BLOCKS, device="cuda", dtype=torch.float64), torch.zeros(16, device="cuda", dtype=torch.float64)
    bd = dev(b)
    check(_lib.load().adamvs_texture_level_cg_init(ptr(bd), n, tol, ptr(G), ptr(R), ptr(P), ptr(partials), ptr(state), hip_ops._stream()),
          "texture_level_cg_init")
    more = lambda k: cg_call(g, gd, lam, k, G, R, P, AP, partials, state)
    for _ in range(groups):
        more(iters)
    torch.cuda.synchronize()
    return G, R, P, state, more


@pytest.mark.parametrize("n", (256, 257))
def test_channel_symmetry(n):
    """The same system with the channels of b permuted.  Ap, alpha, g and r of the first iteration are the permuted ones bit for
    bit: the SpMV and its dot product treat a row's three channels alike.  r'.r' is not: k_lvl_update_xr sums it over 16-byte
    pairs of the flat vector, and entry (i, c) lies in pair floor((3 i + c) / 2), so another channel spreads the same squares
    over other lanes and the fixed tree adds them in another order.  beta and everything after it therefore agree only within
    the bound of that sum (twice: both runs carry it), which replaces the bit-for-bit claim over a fixed number of iterations."""
    g = graph(n)
    rng = np.random.default_rng(n)
    b = K.laplacian_sparse(g, 1.0 / LAM) @ rng.normal(size=(n, 3))
    perm = [2, 0, 1]
    (G1, R1, P1, s1, _), (G2, R2, P2, s2, _) = (solve_raw(g, x, LAM, 0.0, 1) for x in (b, np.ascontiguousarray(b[:, perm])))
    G1, R1, P1, G2, R2, P2 = (t.cpu().numpy()[:n] for t in (G1, R1, P1, G2, R2, P2))
    s1, s2 = s1.cpu().numpy(), s2.cpu().numpy()
    assert_bits(G2, np.ascontiguousarray(G1[:, perm]), "g")
    assert_bits(R2, np.ascontiguousarray(R1[:, perm]), "r")
    for k in (K.ST_BB, K.ST_ALPHA):
        assert_bits(s2[k:k + 3], s1[k:k + 3][perm], "state[%d..]" % k)
    nb, chunk, pairs, pchunk = K.grid(n)
    N, _ = K.dot_ld(R1, R1)
    bound = 2 * K.dot_path(pchunk, nb) * K.U64 * N
    d_rr = np.abs(s2[K.ST_RR:K.ST_RR + 3] - s1[K.ST_RR:K.ST_RR + 3][perm])
    assert (d_rr <= bound[perm]).all(), (d_rr, bound)
    bb = s1[K.ST_BB:K.ST_BB + 3]
    d_beta = np.abs(s2[K.ST_BETA:K.ST_BETA + 3] - s1[K.ST_BETA:K.ST_BETA + 3][perm])
    beta_bound = (bound / bb * (1 + K.U64) + 2 * K.U64 * s1[K.ST_BETA:K.ST_BETA + 3])[perm]
    assert (d_beta <= beta_bound).all(), (d_beta, beta_bound)
    # p' = r' + beta p with p = b: the two differ by at most |d beta| |b| and one rounding of each product and sum
    slack = beta_bound * np.abs(b[:, perm]) + 4 * K.U64 * (np.abs(R2) + np.abs(s2[K.ST_BETA:K.ST_BETA + 3] * b[:, perm]))
    assert (np.abs(P2 - P1[:, perm]) <= slack).all()
    print("channel symmetry n = %d: |d r.r| %.3g, |d beta| %.3g of their bounds" % (n, (d_rr / bound[perm]).max(), (d_beta / beta_bound).max()))


def test_stop_protocol():
    """A graph of about 120 neighbours per node with equal weights is well conditioned (eigenvalues within 120 +- 2 sqrt 120), so
    every iteration divides the residual by about ten and a tol can sit a factor 2 away from the residuals on both sides."""
    n = 3000
    g = K.random_graph(n, seed=77, mean_deg=120, special=False)
    Lm = K.laplacian_sparse(g, 1.0)
    b = Lm @ np.random.default_rng(8).normal(size=(n, 3))
    _, _, hist = K.cg_sparse(Lm, b, 0.0, 14)
    ks = [k for k in range(2, 15) if hist[k - 1] >= 4 * hist[k] and hist[k] > 1e-9]
    assert ks, hist
    k = ks[len(ks) // 2]
    tol = float(np.sqrt(hist[k] * hist[k - 1]))
    _, k_ref, h2 = K.cg_sparse(Lm, b, tol, 100)
    assert k_ref == k and 2 <= k <= 14 and h2[k] <= tol / 2 and h2[k - 1] >= 2 * tol and min(h2[:k]) >= 2 * tol, (k, tol, h2)
    G, R, P, state, more = solve_raw(g, b, 1.0, tol, 16)
    st = state.cpu().numpy()
    assert st[K.ST_ITERS] == k and st[K.ST_DONE] == 1.0
    assert (st[K.ST_RR:K.ST_RR + 3] <= tol * tol * st[K.ST_BB:K.ST_BB + 3]).all()
    G0, _, _, st0, _ = solve_raw(g, b, 1.0, 0.0, k)
    assert st0.cpu().numpy()[K.ST_ITERS] == k and st0.cpu().numpy()[K.ST_DONE] == 0.0
    assert_bits(G.cpu().numpy()[:n], G0.cpu().numpy()[:n], "g at the stopping iteration")
    before = [t.cpu().numpy().tobytes() for t in (G, R, P, state)]
    more(16)
    torch.cuda.synchronize()
    assert [t.cpu().numpy().tobytes() for t in (G, R, P, state)] == before
    print("stop protocol: stops at %d, tol %.3g between %.3g and %.3g" % (k, tol, h2[k], h2[k - 1]))


def solve(g, b, lam, tol, iters):
    gd = graph_dev(g)
    out, it, res, cap = hip_ops.texture_level_solve(gd[0], gd[1], dev(b).reshape(-1, 3), lam, tol, iters)
    return out.cpu().numpy(), it, res, cap


def test_degenerate_solves():
    g = graph(257)
    n = g["n"]
    Lm = K.laplacian_sparse(g, 1.0 / LAM)
    b = Lm @ np.random.default_rng(9).normal(size=(n, 3))
    # b = 0: done at init
    out, it, res, cap = solve(g, np.zeros((n, 3)), LAM, 1e-6, 50)
    assert it == 0 and not cap and res == [0.0, 0.0, 0.0] and (out == 0).all() and out.shape == (n, 3)
    # one channel of b zero: that channel of g stays exactly 0 while the others converge
    b1 = b.copy()
    b1[:, 1] = 0.0
    out, it, res, cap = solve(g, b1, LAM, 1e-8, 2000)
    assert not cap and 0 < it < 2000 and max(res) <= 1e-8 and res[1] == 0.0
    assert (bits(np.ascontiguousarray(out[:, 1])) == 0).all() and np.abs(out[:, [0, 2]]).max() > 0
    nb_ = np.linalg.norm(b1, axis=0)[[0, 2]]
    true = np.linalg.norm(b1 - Lm @ out, axis=0)[[0, 2]] / nb_
    drift = 10 * it * 2.0 ** -52 * 2 * Lm.diagonal().max() * np.linalg.norm(out, axis=0)[[0, 2]] / nb_     # as in test_whole_solve
    assert (true <= np.asarray(res)[[0, 2]] + drift).all(), (true, res, drift)
    # a NaN in b never converges: the cap is reported
    b2 = b.copy()
    b2[n // 2, 2] = np.nan
    out, it, res, cap = solve(g, b2, LAM, 1e-4, 40)
    assert cap and it == 40
    # isolated nodes with b != 0: p.Ap = 0, every step is refused; g stays 0 and finite however long it runs (p must not grow:
    # doubling it every iteration overflows after about 1024 of them and 0 * inf would reach g)
    iso = K.csr(n, [], [], [])
    out, it, res, cap = solve(iso, b, LAM, 1e-4, 1100)
    assert cap and it == 1100 and (out == 0).all() and max(abs(x - 1.0) for x in res) < 1e-12
    # n = 0 and n = 1
    out, it, res, cap = solve(K.csr(0, [], [], []), np.zeros((0, 3)), LAM, 1e-4, 10)
    assert out.shape == (0, 3) and it == 0 and not cap and res == [0.0, 0.0, 0.0]
    one = graph(1)
    out, it, res, cap = solve(one, np.zeros((1, 3)), LAM, 1e-4, 10)
    assert it == 0 and not cap and (out == 0).all()
    out, it, res, cap = solve(one, np.array([[1.0, -2.0, 3.0]]), LAM, 1e-4, 5)
    assert it == 5 and cap and (out == 0).all()


@pytest.mark.parametrize("n", SIZES[-2:])
def test_whole_solve(n):
    """tol = 1e-8 through hip_ops.texture_level_solve.  On the random graph (special rows and all): the reported residual, the true
    one within the drift of the recursion, identical bytes from two runs.  The iteration count is compared where the margins
    around tol can hold: consecutive residuals of a graph of six neighbours lie a factor of about 2 apart, never 4, unless the
    iteration is the last of a finite termination.  equitable_graph gives that: b constant on the seven blocks lies in an
    invariant subspace of dimension 7, so conjugate gradients end after at most six iterations with a drop of many orders."""
    lam, tol = 0.5, 1e-8
    # the iteration count
    ge = K.equitable_graph(n, seed=n)
    Le = K.laplacian_sparse(ge, 1.0 / lam)
    be = Le @ np.random.default_rng(n).normal(size=(8, 3))[ge["block"]]
    _, k, hist = K.cg_sparse(Le, be, tol, 50)
    assert 2 <= k <= 7 and hist[k] <= tol / 2 and min(hist[:k]) >= 2 * tol, hist
    out, it, res, cap = solve(ge, be, lam, tol, 1000)
    print("whole solve n = %d, equitable: %d iterations, restatement %d (%.3g after %.3g), reported %s" % (n, it, k, hist[k], hist[k - 1], res))
    assert it == k and not cap and max(res) <= tol
    # the residuals, on the random graph
    g = graph(n)
    Lm = K.laplacian_sparse(g, 1.0 / lam)
    b = Lm @ np.random.default_rng(n + 1).normal(size=(n, 3))
    out, it, res, cap = solve(g, b, lam, tol, 5000)
    assert not cap and 10 <= it < 5000 and max(res) <= tol, (it, res, cap)
    nb_ = np.linalg.norm(b, axis=0)
    true = np.linalg.norm(b - Lm @ out, axis=0) / nb_
    # one rounding of |L| |g| per iteration (|L| <= twice the largest diagonal entry), with a factor 10 for the vector norms
    drift = 10 * it * 2.0 ** -52 * 2 * Lm.diagonal().max() * np.linalg.norm(out, axis=0) / nb_
    print("whole solve n = %d, random: %d iterations, reported %s, true %s, drift term %s" % (n, it, res, true, drift))
    assert (true <= np.asarray(res) + drift).all(), (true, res, drift)
    out2, it2, res2, cap2 = solve(g, b, lam, tol, 5000)
    assert it2 == it and res2 == res and out2.tobytes() == out.tobytes()


# ---- 2. owner, dilation, apply ----------------------------------------------------------------------------------------------
P_PAGE, PAGES, NC, SLOT = 1024, 3, 3000, 32


@functools.lru_cache(maxsize=None)
def chart_scene():
    """3000 charts, one per 32 x 32 slot of three pages: empty boxes (w = 0 or h = 0) first, in the middle and last, boxes of
    1 x 1, 1 x h, w x 1, wide ones (20 x 3, for faces whose box holds exactly 16 and 17 centres in one row) and ordinary ones of
    8 .. 14 texels a side carrying 26 faces of about 5 x 5 texels each (overlapping, reaching over the box, of either
    orientation) and some larger ones.  Degenerate, NaN and inf faces and faces of chart -1 or >= nc are mixed in; the faces
    are shuffled, so a face that must own nothing has a fair chance of holding the smallest index."""
    rng = np.random.default_rng(2024)
    kind = rng.choice(5, NC, p=[0.05, 0.05, 0.05, 0.05, 0.8])      # 0: 1 x 1, 1: 1 x h, 2: w x 1, 3: wide, 4: ordinary
    w = np.choose(kind, [1, 1, rng.integers(2, 10, NC), 20, rng.integers(8, 15, NC)])
    h = np.choose(kind, [1, rng.integers(2, 10, NC), 1, 3, rng.integers(8, 15, NC)])
    empty = np.array([0, 1, NC // 2, NC // 2 + 1, NC // 2 + 2, NC - 2, NC - 1])
    w[empty] = [0, 4, 0, 0, 5, 3, 0]
    h[empty] = [5, 0, 0, 7, 0, 0, 2]
    kind[empty] = -1
    i = np.arange(NC)
    charts = np.stack([rng.integers(0, 500, NC), rng.integers(0, 500, NC), w, h, (i % 32) * SLOT, ((i // 32) % 32) * SLOT, i // 1024,
                       rng.integers(0, 4, NC)], 1).astype(np.int32)
    ordinary = np.nonzero(kind == 4)[0]
    charts[ordinary[5:8], 6] = [-1, PAGES, PAGES + 3]               # a page out of range
    edge = ordinary[[8, 48, 88, 128]]                               # four slot rows: moved to the page's edge they do not meet
    assert len(set(edge // 32)) == 4
    charts[edge[:3], 4] = P_PAGE - 3                                # texels with dx >= 3 lie outside the page
    charts[edge[3], 5] = P_PAGE - 2
    prefix = np.concatenate([[0], np.cumsum(charts[:, 2].astype(np.int64) * charts[:, 3])])
    x0, y0 = charts[:, 0].astype(np.float64), charts[:, 1].astype(np.float64)

    def blobs(c, radius):
        """One face per entry of c: corners at `radius` from a centre inside the box, 120 degrees apart within +- 25."""
        m = len(c)
        cx, cy = x0[c] + rng.uniform(0, 1, m) * charts[c, 2], y0[c] + rng.uniform(0, 1, m) * charts[c, 3]
        ang = rng.uniform(0, 2 * np.pi, m)[:, None] + np.arange(3) * 2 * np.pi / 3 + rng.uniform(-0.43, 0.43, (m, 3))
        r = radius * rng.uniform(0.8, 1.15, (m, 3))
        q = np.stack([cx[:, None] + r * np.cos(ang), cy[:, None] + r * np.sin(ang)], 2)          # [m, 3, 2]
        flip = rng.integers(0, 2, m).astype(bool)
        q[flip] = q[flip][:, [0, 2, 1]]
        return q.reshape(m, 6)

    uv, ch = [], []
    uv.append(blobs(np.repeat(ordinary, 26), 3.5)), ch.append(np.repeat(ordinary, 26))
    uv.append(blobs(ordinary[::20], 6.5)), ch.append(ordinary[::20])                         # boxes of more than 64 centres
    thin = np.nonzero((kind >= 0) & (kind <= 2))[0]
    uv.append(blobs(np.repeat(thin, 2), 3.0)), ch.append(np.repeat(thin, 2))
    wide = np.nonzero(kind == 3)[0]
    for span in (15.3, 16.3):                                       # u from a - 0.3 to a + span: 16 and 17 centres in the one row v = b
        a, b = x0[wide] + 1, y0[wide] + 1
        uv.append(np.stack([a - 0.3, b - 0.3, a + span, b - 0.3, a + 8.0, b + 0.6], 1)), ch.append(wide)
    a, b = x0[ordinary[:200]] + 1, y0[ordinary[:200]] + 1          # a box of 4 x 4 centres exactly
    uv.append(np.stack([a - 0.3, b - 0.3, a + 3.3, b - 0.35, a + 1.4, b + 3.3], 1)), ch.append(ordinary[:200])
    # faces that own nothing: zero area (a point, a repeated corner, three collinear corners), NaN and inf corners
    bad = blobs(ordinary[:60], 3.5)
    bad[:10, 2:4] = bad[:10, 4:6] = bad[:10, 0:2]
    bad[10:20, 4:6] = bad[10:20, 2:4]
    bad[20:30] = np.stack([x0[ordinary[:10]] + 1.0, y0[ordinary[:10]] + 1.0, x0[ordinary[:10]] + 3.0, y0[ordinary[:10]] + 3.0,
                           x0[ordinary[:10]] + 7.0, y0[ordinary[:10]] + 7.0], 1)
    bad[30:40, 1] = np.nan
    bad[40:50, 4] = np.inf
    bad[50:60, 3] = -np.inf
    uv.append(bad), ch.append(ordinary[:60])
    stray = blobs(ordinary[60:120], 3.5)
    uv.append(stray), ch.append(np.resize([-1, NC, NC + 5, -7], 60))
    uv, ch = np.concatenate(uv).astype(np.float32), np.concatenate(ch)
    order = rng.permutation(len(ch))
    uv, ch = uv[order], ch[order].astype(np.int32)
    n_bad = 60
    nf = len(ch)
    nodes = 5000
    corner = rng.integers(0, nodes, (nf, 3)).astype(np.int32)
    corner[::97, 1] = -1
    corner[5::101, 2] = nodes
    corner[7::103, 0] = nodes + 9
    return dict(charts=charts, prefix=prefix, uv=uv, chart=ch, kind=kind, corner=corner, nodes=nodes, n_bad=n_bad,
                chart_ref=np.where((ch >= 0) & (ch < NC), ch, -1))


def box_centres(s):
    """Per face the pixel centres of its clamped box, by the set-up's own rule (ceil / floor of the fp32 corners, the chart's box)."""
    uv, c = s["uv"].astype(np.float64), s["charts"][np.maximum(s["chart_ref"], 0)].astype(np.int64)
    U, V = uv[:, 0::2], uv[:, 1::2]
    with np.errstate(invalid="ignore"):
        bw = np.minimum(np.floor(U.max(1)), c[:, 0] + c[:, 2] - 1) - np.maximum(np.ceil(U.min(1)), c[:, 0]) + 1
        bh = np.minimum(np.floor(V.max(1)), c[:, 1] + c[:, 3] - 1) - np.maximum(np.ceil(V.min(1)), c[:, 1]) + 1
        area = (U[:, 1] - U[:, 0]) * (V[:, 2] - V[:, 0]) - (V[:, 1] - V[:, 0]) * (U[:, 2] - U[:, 0])
    ok = (s["chart_ref"] >= 0) & np.isfinite(area) & (area != 0) & (bw >= 1) & (bh >= 1)
    return np.where(ok, bw * bh, 0), area


@functools.lru_cache(maxsize=None)
def gpu_owner():
    s = chart_scene()
    charts_d, prefix_d, uv_d, chart_d = dev(s["charts"]), dev(s["prefix"]), dev(s["uv"]), dev(s["chart"])
    big = torch.zeros(1 + len(s["chart"]), device="cuda", dtype=torch.int32)
    raster = hip_ops.texture_level_owner(uv_d, chart_d, charts_d, prefix_d, big)
    d1 = hip_ops.texture_level_dilate(charts_d, prefix_d, raster)
    d2 = hip_ops.texture_level_dilate(charts_d, prefix_d, d1)
    torch.cuda.synchronize()
    return dict(raster=raster.cpu().numpy(), d1=d1.cpu().numpy(), d2=d2.cpu().numpy(), listed=int(big[0].item()),
                charts_d=charts_d, prefix_d=prefix_d, uv_d=uv_d)


def test_owner_and_dilation():
    s = chart_scene()
    charts, prefix, uv64 = s["charts"], s["prefix"], s["uv"].astype(np.float64)
    assert L.BAND == _lib.TEXTURE_LEVEL_BAND == 2
    # what the scene holds, on the CPU
    px, area = box_centres(s)
    assert (px > 16).sum() >= 40000 and (px == 16).sum() >= 100 and (px == 17).sum() >= 50 and (px > 64).sum() >= 20
    assert ((px >= 1) & (px < 16)).sum() >= 100
    with np.errstate(invalid="ignore"):
        assert (area < 0).sum() > 10000 and (area > 0).sum() > 10000 and (area == 0).sum() >= 30 and (~np.isfinite(area)).sum() >= 30
    assert ((s["chart"] < 0) | (s["chart"] >= NC)).sum() == 60
    wh = charts[:, 2].astype(np.int64) * charts[:, 3]
    assert wh[0] == wh[1] == wh[NC // 2] == wh[NC - 1] == 0 and prefix[-1] > 200000
    for kw, kh in ((1, 1), (1, 5), (5, 1)):
        assert ((charts[:, 2] == kw) & (charts[:, 3] == kh)).any()
    with np.errstate(invalid="ignore"):
        lo = L.owner_map(uv64, s["chart_ref"], charts, prefix, GROW_PX)
        hi = L.owner_map(uv64, s["chart_ref"], charts, prefix, -GROW_PX)
    firm = lo == hi
    assert firm.mean() > 0.9, firm.mean()
    o = gpu_owner()
    assert o["listed"] == (px > 16).sum()
    raster = o["raster"].astype(np.int64)
    np.testing.assert_array_equal(raster[firm], lo[firm])
    print("owner: %d texels, %.2f %% firm, %d faces listed of %d" % (len(firm), 100 * firm.mean(), o["listed"], len(px)))
    ci = L.texel_index(charts, prefix)[0]
    own = raster != L.UNOWNED
    assert own.sum() > 100000 and (~own).sum() > 1000
    np.testing.assert_array_equal(s["chart"][raster[own]], ci[own])
    assert (px[raster[own]] > 0).all()                                  # no degenerate, NaN or stray face owns a texel
    np.testing.assert_array_equal(o["d1"], L.dilate(raster, charts, prefix, rounds=1))
    np.testing.assert_array_equal(o["d2"], L.dilate(raster, charts, prefix, rounds=L.BAND))
    assert own.sum() < (o["d1"] != L.UNOWNED).sum() < (o["d2"] != L.UNOWNED).sum()


def test_apply():
    """Owned texels whose float64 value texel + g lies within 1e-3 of a rounding boundary are held to one level only; the
    condition on their share is at most 1 % (uniform fractions make it 0.2 %), asserted on the restatement."""
    s = chart_scene()
    o = gpu_owner()
    charts, prefix, nodes = s["charts"], s["prefix"], s["nodes"]
    rng = np.random.default_rng(5)
    g = rng.uniform(-40.0, 40.0, (nodes, 3))
    atlas = rng.integers(0, 256, (PAGES, P_PAGE, P_PAGE, 4), dtype=np.uint8)
    owner = o["d2"].astype(np.int64)
    _, _, _, pg, ax, ay = L.texel_index(charts, prefix)
    owned = owner != L.UNOWNED
    cn = s["corner"].astype(np.int64)[np.where(owned, owner, 0)]
    off_page = (ax >= P_PAGE) | (ay >= P_PAGE) | (pg < 0) | (pg >= PAGES)
    bad_node = ((cn < 0) | (cn >= nodes)).any(1)
    skipped = owned & (off_page | bad_node)
    assert (owned & off_page).sum() > 50 and (owned & bad_node & ~off_page).sum() > 50
    kept = np.where(skipped, L.UNOWNED, owner)
    m, val, pg, ax, ay = L.levelled_values(atlas[..., :3], kept, s["uv"].astype(np.float64), s["corner"].astype(np.int64),
                                           g.astype(np.float32), charts, prefix)
    want = np.clip(np.floor(val + 0.5), 0, 255)
    frac = val + 0.5 - np.floor(val + 0.5)
    near = (np.minimum(frac, 1.0 - frac) <= 1e-3).any(1)
    assert near.mean() <= 0.01, near.mean()
    assert (val < -0.5).any() and (val > 255.5).any()                  # both clamps bind
    runs = []
    for _ in range(2):
        a = dev(atlas)
        hip_ops.texture_level_apply(o["uv_d"], dev(s["corner"]), dev(g), o["charts_d"], o["prefix_d"], dev(o["d2"]), P_PAGE, a)
        runs.append(a.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes()
    out = runs[0]
    got = out[pg, ay, ax, :3].astype(np.float64)
    print("apply: %d texels levelled, %d skipped, %.3f %% within 1e-3 of a rounding boundary, %d of them one level off"
          % (m.sum(), skipped.sum(), 100 * near.mean(), (got != want).any(1).sum()))
    np.testing.assert_array_equal(got[~near], want[~near])
    assert np.abs(got - want).max() <= 1
    assert (got != atlas[pg, ay, ax, :3]).any(1).mean() > 0.9
    np.testing.assert_array_equal(out[..., 3], atlas[..., 3])
    mask = np.zeros(atlas.shape[:3], bool)
    mask[pg, ay, ax] = True
    assert mask.sum() == m.sum()                                        # every levelled texel has a place of its own
    np.testing.assert_array_equal(out[~mask], atlas[~mask])            # unowned and skipped texels, everything outside the boxes
