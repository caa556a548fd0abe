"""fp64 numpy restatement of include/adamvs_hip.h "Cloud distance", written from the header's text and sharing nothing with the
library: the truncated nearest neighbour by brute force (no lattice: the targets are cut into slabs along x only so that the
30 000 x 30 000 case stays quick, and a slab holds every target within D of its queries), and the surface sampler in the
header's operation order.  Needs no scipy."""
import numpy as np


def nearest(targets, queries, D, chunk=512):
    """-> (d2 [nq] fp64: the squared distance to the nearest target, inf where none lies within D; index [nq] int64: the lowest
    number among the targets at exactly that distance, -1 where none; second [nq] fp64: the distance (not squared) to the nearest
    target with another number, inf where there is none within reach of the slab; first [nq] fp64: the distance to the nearest
    target whether or not it lies within D, inf where the slab holds none)."""
    T = np.asarray(targets, np.float64).reshape(-1, 3)
    Q = np.asarray(queries, np.float64).reshape(-1, 3)
    nq = len(Q)
    d2 = np.full(nq, np.inf)
    index = np.full(nq, -1, np.int64)
    second = np.full(nq, np.inf)
    first = np.full(nq, np.inf)
    if len(T) == 0 or nq == 0:
        return d2, index, second, first
    reach = float(D) * (1.0 + 1e-3) + 1e-3              # the slab's margin: past D, so that `second` sees every near tie
    torder = np.argsort(T[:, 0], kind="stable")
    tx = T[torder, 0]
    finite = np.isfinite(Q).all(1)
    qorder = np.argsort(np.where(finite, Q[:, 0], np.inf), kind="stable")
    qorder = qorder[finite[qorder]]
    for s in range(0, len(qorder), chunk):
        qi = qorder[s:s + chunk]
        q = Q[qi]
        a = np.searchsorted(tx, q[:, 0].min() - reach, "left")
        b = np.searchsorted(tx, q[:, 0].max() + reach, "right")
        if b <= a:
            continue
        cand = np.sort(torder[a:b])                        # ascending numbers: argmin then returns the lowest among equals
        p = T[cand]
        e = q[:, None, :] - p[None, :, :]
        dd = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        j = dd.argmin(1)
        m = dd[np.arange(len(q)), j]
        first[qi] = np.sqrt(m)
        if dd.shape[1] > 1:
            dd[np.arange(len(q)), j] = np.inf
            second[qi] = np.sqrt(dd.min(1))
        keep = m <= float(D) * float(D)
        d2[qi] = np.where(keep, m, np.inf)
        index[qi] = np.where(keep, cand[j], -1)
    return d2, index, second, first


def subdivisions(v0, v1, v2, s):
    """n of one face: max(1, ceil(L / s)), L the longest edge."""
    def edge2(a, b):
        d = b - a
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    L = np.sqrt(max(edge2(v0, v1), edge2(v1, v2), edge2(v2, v0)))
    return max(1, int(np.ceil(L / np.float64(s))))


def sample_mesh(xyz, faces, s):
    """-> points [m, 3] fp64: per face, ascending, the samples (v0 + (i / n)(v1 - v0)) + (j / n)(v2 - v0), i ascending, then j,
    i + j <= n."""
    xyz = np.asarray(xyz, np.float64)
    out = []
    for f in np.asarray(faces, np.int64).reshape(-1, 3):
        v0, v1, v2 = xyz[f[0]], xyz[f[1]], xyz[f[2]]
        n = subdivisions(v0, v1, v2, s)
        u, w = v1 - v0, v2 - v0
        i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
        ok = (i + j) <= n
        a = (i[ok].astype(np.float64) / np.float64(n))[:, None]
        b = (j[ok].astype(np.float64) / np.float64(n))[:, None]
        out.append((v0[None, :] + a * u[None, :]) + b * w[None, :])
    return np.concatenate(out) if out else np.zeros((0, 3))
