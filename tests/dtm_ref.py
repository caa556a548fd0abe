"""numpy restatement of include/adamvs_hip.h "DSM ground filter": the opening with square windows (literally, and in the
separable doubling form), the schedule, the progressive morphological filter and the DTM / nDSM built on the gap fill's
reference (tests/dsm_fill_ref.py)."""
import math

import numpy as np

from dsm_fill_ref import fill_ref

NAN_BITS = 0x7FC00000
NAN32 = np.array([NAN_BITS], np.uint32).view(np.float32)[0]


def open_brute(z, r):
    """open(Z, r) as stated: E(c) = min of Z over the valid cells of the (2r+1)^2 window of c, O(c) = max of E over the cells
    of the window that have an E; O on valid cells, NaN on empty ones."""
    z = np.asarray(z, np.float32)
    H, W = z.shape
    valid = np.isfinite(z)
    E = np.full((H, W), np.nan, np.float32)
    for i in range(H):
        for j in range(W):
            win = (slice(max(0, i - r), i + r + 1), slice(max(0, j - r), j + r + 1))
            v = z[win][valid[win]]
            if v.size:
                E[i, j] = v.min()
    has = ~np.isnan(E)
    out = np.full((H, W), NAN32, np.float32)
    for i in range(H):
        for j in range(W):
            if valid[i, j]:
                win = (slice(max(0, i - r), i + r + 1), slice(max(0, j - r), j + r + 1))
                out[i, j] = E[win][has[win]].max()
    return out


def _running(a, r, op, neutral):
    """op over the window [x - r, x + r] along the last axis (entries outside the array are `neutral`), by doubling."""
    n = a.shape[-1]
    w = 2 * r + 1
    p = w.bit_length() - 1
    m = np.concatenate([np.full(a.shape[:-1] + (r,), neutral, a.dtype), a, np.full(a.shape[:-1] + (r,), neutral, a.dtype)], -1)
    for j in range(p):                                  # m[x] = op over [x, x + 2^(j+1))
        m = op(m[..., :m.shape[-1] - (1 << j)], m[..., (1 << j):])
    tail = w - (1 << p)
    return op(m[..., :n], m[..., tail:tail + n])


def open_sep(z, r):
    """The same, restated separably (rows, then columns) with windows formed by doubling: seconds on large grids."""
    z = np.asarray(z, np.float32)
    valid = np.isfinite(z)
    e = np.where(valid, z, np.float32(np.inf))
    e = _running(e, r, np.minimum, np.float32(np.inf))
    e = _running(e.T, r, np.minimum, np.float32(np.inf)).T
    o = np.where(np.isfinite(e), e, np.float32(-np.inf))
    o = _running(o, r, np.maximum, np.float32(-np.inf))
    o = _running(o.T, r, np.maximum, np.float32(-np.inf)).T
    return np.where(valid, o, NAN32).astype(np.float32)


def same_opening(a, b, z):
    """== on the valid cells of z (so -0.0 and 0.0 agree), the NaN bit pattern on the empty ones."""
    valid = np.isfinite(z)
    return bool(a.shape == b.shape == z.shape and (a[valid] == b[valid]).all()
                and (a[~valid].view(np.uint32) == NAN_BITS).all() and (b[~valid].view(np.uint32) == NAN_BITS).all())


def schedule(gsd, max_radius=16.0, slope=1.0, dh0=0.15, dh_max=2.5):
    R = math.floor(max_radius / gsd)
    radius = []
    r = 1
    while r < R:
        radius.append(r)
        r *= 2
    radius.append(R)
    dh, w_prev = [], 1
    for r in radius:
        w = 2 * r + 1
        dh.append(min(dh_max, dh0 + slope * gsd * (w - w_prev)))
        w_prev = w
    return np.array(radius, np.int32), np.array(dh, np.float64)


def pmf(dsm, radius, dh, opening=open_sep):
    """-> dict(level uint8, opened float32, counts): Z_0 = dsm; O_k = open(Z_{k-1}, r_k); a valid, not yet flagged cell gets
    level k iff (double)Z_{k-1} - (double)O_k > dh_k; Z_k = O_k."""
    z = np.asarray(dsm, np.float32)
    valid = np.isfinite(z)
    z = np.where(valid, z, NAN32).astype(np.float32)
    level = np.where(valid, 0, 255).astype(np.uint8)
    per_level = []
    for k, (r, t) in enumerate(zip(radius, dh), start=1):
        o = opening(z, int(r))
        with np.errstate(invalid="ignore"):
            flag = valid & (level == 0) & (z.astype(np.float64) - o.astype(np.float64) > float(t))
        level[flag] = k
        per_level.append(int(flag.sum()))
        z = o
    nv = int(valid.sum())
    counts = dict(valid=nv, ground=nv - sum(per_level), object=sum(per_level), empty=int(z.size - nv), per_level=per_level)
    return dict(level=level, opened=z, counts=counts)


def dtm_ref(dsm, gsd, max_radius=16.0, slope=1.0, dh0=0.15, dh_max=2.5, fill_max_dist=None):
    """The products: ground = dsm where level == 0, dtm = fill_ref(ground, r_fill) with r_fill = fill_max_dist / gsd (default
    2 max_radius, capped at 1024 cells), ndsm = (float)((double)dsm - (double)dtm) where both are finite."""
    dsm = np.asarray(dsm, np.float32)
    radius, dh = schedule(gsd, max_radius, slope, dh0, dh_max)
    res = pmf(dsm, radius, dh)
    ground = np.where(res["level"] == 0, dsm, NAN32).astype(np.float32)
    r_fill = min((2.0 * max_radius if fill_max_dist is None else fill_max_dist) / gsd, 1024.0)
    dtm = fill_ref(ground, np.zeros(dsm.shape + (4,), np.uint8), r_fill)["dsm"]
    both = np.isfinite(dsm) & np.isfinite(dtm)
    ndsm = np.full(dsm.shape, NAN32, np.float32)
    ndsm[both] = (dsm[both].astype(np.float64) - dtm[both].astype(np.float64)).astype(np.float32)
    res.update(ground=ground, dtm=dtm, ndsm=ndsm, radius=radius, dh=dh, r_fill=r_fill)
    return res


# ---- scenes -----------------------------------------------------------------------------------------------------------------
WIDE_BOX = ((40, 60, 80, 80, 12.0),)               # wider than 2 R + 1 = 65 cells in both axes at gsd 0.5


def plane_scene(H=160, W=200, gsd=0.5, boxes=((60, 70, 25, 30, 9.0), (110, 150, 4, 3, 4.0)), gradients=(0.2, -0.1)):
    """A plane with the gradients (per metre, along x and y) plus boxes (row, column, rows, columns, metres), every box at least
    R + 2 = 34 cells from the grid's edges -> (dsm, plane, box mask)."""
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    plane = 50.0 + gradients[0] * gsd * j + gradients[1] * gsd * i
    z = plane.copy()
    mask = np.zeros((H, W), bool)
    for i0, j0, h, w, dz in boxes:
        z[i0:i0 + h, j0:j0 + w] += dz
        mask[i0:i0 + h, j0:j0 + w] = True
    return z.astype(np.float32), plane, mask


def random_raster(H, W, seed, p_valid=0.5, blobs=0):
    """test_dsm_fill_gpu.random_raster's heights: a smooth field (+ 12.5 m boxes) with random empty cells and empty discs."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:H, 0:W]
    z = 80.0 + 20.0 * np.sin(j / 17.0) * np.cos(i / 11.0) + np.where(((i // 23) + (j // 29)) % 3 == 0, 12.5, 0.0)
    valid = rng.random((H, W)) < p_valid
    for _ in range(blobs):
        ci, cj, rad = rng.integers(0, H), rng.integers(0, W), rng.uniform(2, 12)
        valid &= (i - ci) ** 2 + (j - cj) ** 2 > rad * rad
    return np.where(valid, z, np.nan).astype(np.float32)
