"""fp64 numpy reference of the DSM gap fill (include/adamvs_hip.h "DSM gap fill"): the exact bounded distance in two forms,
and the harmonic system assembled explicitly and solved directly (small) or by fp64 conjugate gradients (large).  numpy only."""
import math

import numpy as np

INT32_MAX = np.iinfo(np.int32).max
NAN32 = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.float32)[0]
DIRECT_MAX = 3000            # unknowns solved by np.linalg.solve; more go to CG


def dist2_brute(valid, r):
    """min over every valid cell within ceil(r) of dy^2 + dx^2 (INT32_MAX where that exceeds r^2): small grids only."""
    H, W = valid.shape
    R = int(math.ceil(r))
    best = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sh = np.zeros((H, W), bool)          # sh[i, j] = valid[i + dy, j + dx]
            ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
            xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
            sh[yd, xd] = valid[ys, xs]
            best = np.where(sh, np.minimum(best, dy * dy + dx * dx), best)
    return np.where(best.astype(np.float64) <= r * r, best, INT32_MAX).astype(np.int32)


def column_distance(valid):
    """Rows to the nearest valid cell of the same column (a large value where the column has none)."""
    H, W = valid.shape
    big = 1 << 30
    g = np.full((H, W), big, np.int64)
    run = np.full(W, big, np.int64)
    for i in range(H):
        run = np.where(valid[i], 0, np.minimum(run + 1, big))
        g[i] = run
    run = np.full(W, big, np.int64)
    for i in range(H - 1, -1, -1):
        run = np.where(valid[i], 0, np.minimum(run + 1, big))
        g[i] = np.minimum(g[i], run)
    return g


def dist2_separable(valid, r):
    """The same, restated separably: per-column distances g, then min over |dx| <= ceil(r) of dx^2 + g(j + dx)^2 per row."""
    H, W = valid.shape
    R = int(math.ceil(r))
    g = np.minimum(column_distance(valid), R + 1)
    best = g * g
    for dx in range(1, R + 1):
        if dx >= W:
            break
        for s in (dx, -dx):
            sh = np.full((H, W), R + 1, np.int64)          # sh[:, j] = g[:, j + s]
            if s > 0:
                sh[:, :W - s] = g[:, s:]
            else:
                sh[:, -s:] = g[:, :W + s]
            best = np.minimum(best, dx * dx + sh * sh)
    return np.where(best.astype(np.float64) <= r * r, best, INT32_MAX).astype(np.int32)


def neighbours(H, W):
    """(dy, dx, inside-mask) of the 4 edge neighbours."""
    i, j = np.mgrid[0:H, 0:W]
    return [(dy, dx, (i + dy >= 0) & (i + dy < H) & (j + dx >= 0) & (j + dx < W)) for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1))]


def shift(a, dy, dx, fill=0):
    """out[i, j] = a[i + dy, j + dx] (fill outside)."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[yd, xd] = a[ys, xs]
    return out


def residual(u, valid, fill):
    """sum over N4 & (V | F) of (u_n - u_c) on F (0 elsewhere); u [H, W] or [H, W, k] float64 holding V's values."""
    H, W = valid.shape
    keep = valid | fill
    res = np.zeros_like(u)
    for dy, dx, inside in neighbours(H, W):
        m = inside & shift(keep, dy, dx, False)
        if u.ndim == 3:
            m = m[..., None]
        res += np.where(m, shift(u, dy, dx) - u, 0.0)
    return np.where(fill[..., None] if u.ndim == 3 else fill, res, 0.0)


def solve_harmonic(values, valid, fill, tol=1e-11, max_iter=200000):
    """values [H, W, k] float64 (on V) -> u with the harmonic fill on F, in fp64: a dense direct solve for at most DIRECT_MAX
    unknowns, else conjugate gradients to max |residual| <= tol."""
    H, W = valid.shape
    u = np.where(valid[..., None], values, 0.0).astype(np.float64)
    nf = int(fill.sum())
    if nf == 0:
        return u
    keep = valid | fill
    if nf <= DIRECT_MAX:
        idx = -np.ones((H, W), np.int64)
        idx[fill] = np.arange(nf)
        A = np.zeros((nf, nf))
        b = np.zeros((nf, u.shape[2]))
        ii, jj = np.nonzero(fill)
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            y, x = ii + dy, jj + dx
            ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            r, y, x = idx[ii[ok], jj[ok]], y[ok], x[ok]
            k = keep[y, x]
            A[r[k], r[k]] += 1.0
            f = fill[y, x]
            np.add.at(A, (r[f], idx[y[f], x[f]]), -1.0)
            v = valid[y, x]
            np.add.at(b, r[v], u[y[v], x[v]])
        u[fill] = np.linalg.solve(A, b)
        return u
    # CG on A x = b, A = -(residual operator restricted to F): x on F, V fixed
    def apply(x):                               # A x for x zero outside F
        return -residual_masked(x, keep, fill)
    b = residual_masked(u, keep, fill)          # r0 with x = 0 on F: A x = b
    x = np.zeros_like(u)
    r = b.copy()
    p = r.copy()
    rr = (r * r).sum(axis=(0, 1))
    for _ in range(max_iter):
        if np.abs(r).max() <= tol:
            break
        Ap = apply(p)
        alpha = rr / np.maximum((p * Ap).sum(axis=(0, 1)), 1e-300)
        x += alpha * p
        r -= alpha * Ap
        rr_new = (r * r).sum(axis=(0, 1))
        p = r + (rr_new / np.maximum(rr, 1e-300)) * p
        rr = rr_new
    u = u + x
    res = residual(u, valid, fill)
    assert np.abs(res).max() <= 10 * tol, np.abs(res).max()
    return u


def residual_masked(u, keep, fill):
    """sum over N4 & keep of (u_n - u_c), on F only; u [H, W, k]."""
    H, W = keep.shape
    res = np.zeros_like(u)
    for dy, dx, inside in neighbours(H, W):
        m = (inside & shift(keep, dy, dx, False))[..., None]
        res += np.where(m, shift(u, dy, dx) - u, 0.0)
    return np.where(fill[..., None], res, 0.0)


def fill_ref(dsm, rgba, r, dist=None):
    """The whole fill in fp64 -> dict(dsm float32, rgba uint8, filled uint8, dist2 int32, u [H, W] float64 heights, c [H, W, 3]
    float64 colours, cells_valid, cells_filled, cells_empty)."""
    dsm = np.asarray(dsm, np.float32)
    valid = np.isfinite(dsm)
    dist2 = dist2_separable(valid, r) if dist is None else dist
    fill = ~valid & (dist2.astype(np.float64) <= r * r)
    vals = np.concatenate([np.where(valid, dsm, 0).astype(np.float64)[..., None], rgba[..., :3].astype(np.float64)], -1)
    u = solve_harmonic(vals, valid, fill)
    out = np.where(valid, dsm, np.where(fill, u[..., 0].astype(np.float32), NAN32)).astype(np.float32)
    q = np.clip(np.rint(u[..., 1:]), 0, 255).astype(np.uint8)
    col = np.where(valid[..., None], rgba, np.where(fill[..., None], np.concatenate([q, np.full(q.shape[:2] + (1,), 255, np.uint8)], -1), 0))
    return dict(dsm=out, rgba=col.astype(np.uint8), filled=fill.astype(np.uint8), dist2=dist2, u=u[..., 0], c=u[..., 1:],
                cells_valid=int(valid.sum()), cells_filled=int(fill.sum()), cells_empty=int((~valid & ~fill).sum()))


def components(mask):
    """4-connected labels of mask (-1 outside): min-label propagation with pointer jumping, numpy only."""
    H, W = mask.shape
    lab = np.where(mask, np.arange(H * W).reshape(H, W), H * W)
    flat_mask = mask.ravel()
    while True:
        new = lab.copy()
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            new = np.minimum(new, np.where(mask, shift(lab, dy, dx, H * W), H * W))
        new = np.where(mask, new, H * W)
        f = new.ravel()
        for _ in range(4):                      # pointer jumping: a label is a cell index of the same component
            f = np.where(flat_mask, f[np.minimum(f, H * W - 1)], H * W)
        new = f.reshape(H, W)
        if np.array_equal(new, lab):
            return np.where(mask, lab, -1)
        lab = new
