"""fp64 / exact-integer numpy restatement of the orthophoto's radiometric balance (include/adamvs_hip.h "Image orthophoto:
radiometric balance") on top of tests/ortho_ref.py: the observations of a view on the lattice, the pair statistics, the gain
solve, the image adjustment and the seam statistics."""
import numpy as np

import ortho_ref as R

Q = 64
MAX_Q = 64 * 255


def lattice_shape(grid, S):
    return -(-grid.W // S), -(-grid.H // S)


def observe(grid, dsm, view, zb, S, border=2.0, tol=None, margin=None):
    """One view's observations on the lattice of stride S -> obs [N_s, 4] int64 = (q_r, q_g, q_b, flag).  view: dict(K, R, C,
    rgba host [H, W, 4] uint8); zb: its depth buffer [H, W] fp64.  With margin = (zb_lo, zb_hi, eps_px, eps_z) (the bracketing
    buffers of ortho_ref.zbuf) -> (obs, marginal [N_s]): the cells whose visibility may go either way within the margin."""
    tol = 2.0 * grid.gsd if tol is None else tol
    img = np.asarray(view["rgba"])
    H, W = img.shape[:2]
    z = np.asarray(dsm, np.float32).astype(np.float64)
    height = np.where(np.isfinite(z), z, np.nan)                   # the K = 1 sample of a DSM cell is the cell
    t = R.view_terms(grid, 1, height, view, H, W, border)
    t = {k: (v[::S, ::S] if isinstance(v, np.ndarray) else v) for k, v in t.items()}
    if margin is None:
        vis, marg = R.visibility(t, zb, tol), None
    else:
        vis, marg = R.visibility(t, zb, tol, margin)
    obs = np.zeros(vis.shape + (4,), np.int64)
    if vis.any():
        c = R.bilinear(img, t["u"][vis], t["v"][vis])
        obs[vis, :3] = np.floor(Q * c + 0.5).astype(np.int64)
        obs[vis, 3] = 1
    obs = obs.reshape(-1, 4)
    return obs if margin is None else (obs, marg.reshape(-1))


def pair_stats(obs, pairs, max_diff_q):
    """obs [V, N_s, 4] integers, pairs [P, 2] -> stats [P, 7] int64 = (n, Sa_0..2, Sb_0..2)."""
    obs = np.asarray(obs).astype(np.int64)
    out = np.zeros((len(pairs), 7), np.int64)
    for p, (a, b) in enumerate(pairs):
        A, B = obs[a], obs[b]
        ok = (A[:, 3] == 1) & (B[:, 3] == 1) & (np.abs(A[:, :3] - B[:, :3]) <= max_diff_q).all(1)
        out[p, 0] = ok.sum()
        out[p, 1:4] = A[ok, :3].sum(0)
        out[p, 4:7] = B[ok, :3].sum(0)
    return out


def solve_gains(pairs, stats, V, noise_sigma=10.0, gain_sigma=0.1, min_samples=64):
    """The normal equations of  sum n ((g_a I_ab - g_b I_ba)^2 / sN^2 + (1 - g_a)^2 / sg^2 + (1 - g_b)^2 / sg^2), pair by pair
    and channel by channel, with a dense solve over the views with a non-zero diagonal -> (gains [V, 3], rms before [3], rms
    after [3])."""
    gains = np.ones((V, 3))
    before, after = np.zeros(3), np.zeros(3)
    for k in range(3):
        A = np.zeros((V, V))
        r = np.zeros(V)
        rows = []
        for (a, b), s in zip(pairs, stats):
            n = float(s[0])
            if s[0] < min_samples:
                continue
            Iab, Iba = float(s[1 + k]) / (Q * n), float(s[4 + k]) / (Q * n)
            A[a, a] += n * (Iab ** 2 / noise_sigma ** 2 + 1.0 / gain_sigma ** 2)
            A[b, b] += n * (Iba ** 2 / noise_sigma ** 2 + 1.0 / gain_sigma ** 2)
            A[a, b] += -n * Iab * Iba / noise_sigma ** 2
            A[b, a] += -n * Iab * Iba / noise_sigma ** 2
            r[a] += n / gain_sigma ** 2
            r[b] += n / gain_sigma ** 2
            rows.append((a, b, n, Iab, Iba))
        act = [v for v in range(V) if A[v, v] != 0.0]
        if act:
            gains[act, k] = np.linalg.solve(A[np.ix_(act, act)], r[act])
        if rows:
            tot = sum(n for _, _, n, _, _ in rows)
            before[k] = np.sqrt(sum(n * (Iab - Iba) ** 2 for _, _, n, Iab, Iba in rows) / tot)
            after[k] = np.sqrt(sum(n * (gains[a, k] * Iab - gains[b, k] * Iba) ** 2 for a, b, n, Iab, Iba in rows) / tot)
    return gains, before, after


def adjust(rgba, gain):
    """out_k = min(255, floor(gain_k * (float)in_k + 0.5f)) in float32, alpha copied."""
    rgba = np.asarray(rgba, np.uint8)
    out = rgba.copy()
    for k in range(3):
        prod = np.float32(gain[k]) * rgba[..., k].astype(np.float32)            # one fp32 product
        out[..., k] = np.minimum(np.float32(255.0), np.floor(prod + np.float32(0.5))).astype(np.uint8)
    return out


def seam_pairs(view, ok=None):
    """The adjacent cell pairs (horizontal, then vertical) of a mosaic with both views >= 0 and different (and, with ok, both
    cells in the mask) -> [(mask over the first cells, slices of the first and second cells)]."""
    view = np.asarray(view)
    out = []
    for first, second in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))),
                          ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
        m = (view[first] >= 0) & (view[second] >= 0) & (view[first] != view[second])
        if ok is not None:
            m &= ok[first] & ok[second]
        out.append((m, first, second))
    return out


def seam_stats(view, rgba):
    """-> [4] int64: the seam pairs and the sums of the squared differences of R, G and B over them."""
    rgba = np.asarray(rgba).astype(np.int64)
    out = np.zeros(4, np.int64)
    for m, first, second in seam_pairs(view):
        d = rgba[first][m][:, :3] - rgba[second][m][:, :3]
        out[0] += m.sum()
        out[1:] += (d * d).sum(0)
    return out


def seam_rms(view, rgba, ok=None, channels=(0, 1, 2)):
    """The rms colour step across the seams over the given channels (with ok: between cells of the mask only) -> (rms, pairs)."""
    rgba = np.asarray(rgba).astype(np.float64)
    ss, n = 0.0, 0
    for m, first, second in seam_pairs(view, ok):
        d = rgba[first][m][:, list(channels)] - rgba[second][m][:, list(channels)]
        ss += float((d * d).sum())
        n += int(m.sum())
    return (np.sqrt(ss / (len(channels) * n)) if n else 0.0), n
