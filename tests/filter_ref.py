"""fp64 numpy restatement of include/adamvs_hip.h "Cloud neighbourhoods" and of ada_mvs_amd/cloud_filter.py's rules, written from
their text and sharing nothing with the library: the k nearest other points by brute force (no lattice: the cloud is cut into
slabs along x only, and a slab holds every point within reach of its queries), the mean distances and the statistical rule, and
normals through numpy.linalg.eigh.  Needs no scipy."""
import numpy as np

RANK_EPS = 1e-12
VALID, TOO_FEW, COLLINEAR = 0, 1, 2


def knn(points, R, k, chunk=512):
    """-> (d2 [n, k + 1] fp64, index [n, k + 1] int64): of every point the k + 1 other points that are least in the order (d2,
    number), whether or not they lie within R (the caller cuts at R R); +inf and -1 where the slab holds fewer.  Entries beyond
    the slab's reach (> R by a margin) may be missing; none within it is."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(P)
    d2 = np.full((n, k + 1), np.inf)
    index = np.full((n, k + 1), -1, np.int64)
    reach = float(R) * (1.0 + 1e-3) + 1e-3
    torder = np.argsort(P[:, 0], kind="stable")
    tx = P[torder, 0]
    for s in range(0, n, chunk):
        qi = torder[s:s + chunk]
        q = P[qi]
        a = np.searchsorted(tx, q[:, 0].min() - reach, "left")
        b = np.searchsorted(tx, q[:, 0].max() + reach, "right")
        cand = np.sort(torder[a:b])                           # ascending numbers: a stable sort then puts the lowest among equals first
        e = q[:, None, :] - P[cand][None, :, :]
        dd = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        dd[cand[None, :] == qi[:, None]] = np.inf             # the point itself, by number: a duplicate at another number stays
        o = np.argsort(dd, 1, kind="stable")[:, :k + 1]
        m = o.shape[1]
        got = np.take_along_axis(dd, o, 1)
        d2[qi, :m] = got
        index[qi, :m] = np.where(np.isfinite(got), cand[o], -1)
    return d2, index


def cut(d2, index, R, k):
    """The first k slots of knn() cut at R R -> (d2 [n, k], index [n, k], count [n])."""
    keep = d2[:, :k] <= float(R) * float(R)
    return np.where(keep, d2[:, :k], np.inf), np.where(keep, index[:, :k], -1), keep.sum(1)


def mean_distance(d2, R):
    """d2 [n, k] (+inf: missing) -> the mean over the k slots of sqrt(d2), a missing slot counted as R."""
    d = np.sqrt(d2)
    return np.where(np.isfinite(d), d, float(R)).mean(1)


def statistical_keep(m, std_ratio):
    """-> (keep [n] bool, mu, sigma (population), threshold)."""
    s = np.sort(np.asarray(m, np.float64))
    mu = float(s.mean())
    sigma = float(np.sqrt(((s - mu) ** 2).mean()))
    t = mu + float(std_ratio) * sigma
    return np.asarray(m) <= t, mu, sigma, t


def normals(points, index, count):
    """points [n, 3], index [rows, k] (row r is point r), count [rows] -> (normal [rows, 3], curvature [rows], flag [rows] uint8,
    lam [rows, 3] ascending): eigh of the covariance of the neighbours' differences and the point itself as 0."""
    P = np.asarray(points, np.float64)
    rows = len(index)
    normal, curvature = np.zeros((rows, 3)), np.zeros(rows)
    flag, lam = np.full(rows, TOO_FEW, np.uint8), np.zeros((rows, 3))
    for r in range(rows):
        m = int(count[r])
        d = np.concatenate([P[index[r, :m]] - P[r], np.zeros((1, 3))])
        e = d - d.mean(0)
        w, v = np.linalg.eigh(e.T @ e / len(d))
        lam[r] = w
        if m < 3:
            continue
        if not w[1] > RANK_EPS * w[2]:
            flag[r] = COLLINEAR
            continue
        flag[r] = VALID
        normal[r] = orient(v[:, 0] / np.linalg.norm(v[:, 0]))
        l0 = max(w[0], 0.0)
        curvature[r] = l0 / (l0 + w[1] + w[2])
    return normal, curvature, flag, lam


def orient(nrm):
    """Upward: the first non-zero of (n_z, n_y, n_x) is positive."""
    for c in (2, 1, 0):
        if nrm[c] != 0.0:
            return -nrm if nrm[c] < 0.0 else nrm
    return nrm


def stray_scene():
    """The scene of the filter test: 20 000 points on a plane with sigma_z = 0.02 over [0, 40]^2 and 200 strays 1 to 10 m above
    it, appended after them -> (points [20 200, 3], stray [20 200] bool)."""
    rng = np.random.default_rng(3)
    n = 20000
    xy = rng.uniform(0, 40, (n, 2))
    z = rng.normal(0, 0.02, (n, 1))
    sxy = rng.uniform(0, 40, (200, 2))
    sz = rng.uniform(1, 10, (200, 1))
    pts = np.concatenate([np.concatenate([xy, z], 1), np.concatenate([sxy, sz], 1)])
    stray = np.zeros(len(pts), bool)
    stray[n:] = True
    return pts, stray
