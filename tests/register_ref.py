"""fp64 numpy restatement of include/adamvs_hip.h "Cloud registration", written from the header's text and sharing nothing with the
library or the driver: the rigid motion, the 32 terms of every query, the sums in the stated butterfly and wave order, the solve
through numpy.linalg.eigh, and the whole loop on accuracy_ref.nearest (fp64 brute force) and filter_ref's normals.  Needs no
scipy."""
import numpy as np

import accuracy_ref
import filter_ref

TERMS = 32
TILE = 256


def apply(x, R, c, t):
    """y_k = ((R_k0 d_0 + R_k1 d_1) + R_k2 d_2) + u_k,  d = x - c,  u = c + t."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    R, c, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(c, np.float64).reshape(3), np.asarray(t, np.float64).reshape(3)
    u = c + t
    with np.errstate(invalid="ignore"):
        d = x - c
        return np.stack([((R[k, 0] * d[:, 0] + R[k, 1] * d[:, 1]) + R[k, 2] * d[:, 2]) + u[k] for k in range(3)], 1)


def rows(y, index, targets, normals, flag, c, L, delta):
    """-> (term [nq, 32] fp64: the terms of every query, zeros where it is no pair; pair [nq] bool)."""
    y = np.asarray(y, np.float64).reshape(-1, 3)
    index = np.asarray(index, np.int64).reshape(-1)
    nt = len(targets)
    inside = (index >= 0) & (index < nt)
    j = np.where(inside, index, 0)
    pair = inside & np.isfinite(y).all(1)
    if nt:
        pair &= np.asarray(flag)[j] == 0
    term = np.zeros((len(y), TERMS))
    if not pair.any():
        return term, pair
    p, n = np.asarray(targets, np.float64)[j], np.asarray(normals, np.float64)[j]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e = y - p
        r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
        q = (y - np.asarray(c, np.float64)) / np.float64(L)
        a = [q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1], q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2], q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0],
             n[:, 0], n[:, 1], n[:, 2]]
        ar = np.abs(r)
        w = np.ones(len(y)) if not delta > 0 else np.where(ar <= delta, 1.0, np.float64(delta) / ar)
        cols = [(w * a[u]) * a[v] for u in range(6) for v in range(u, 6)]
        cols += [(w * a[u]) * r for u in range(6)]
        cols += [(w * r) * r, r * r, (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2], np.ones(len(y)), w]
    return np.where(pair[:, None], np.stack(cols, 1), 0.0), pair


def _workgroup(v):
    """v [.., 256, 32] -> [.., 32]: per wave the butterfly over lane distances 32, 16, .. 1, then (W0 + W1) + (W2 + W3)."""
    v = v.reshape(v.shape[:-2] + (4, 64, TERMS))
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off, :] + v[..., off:2 * off, :]
    w = v[..., 0, :]
    return (w[..., 0, :] + w[..., 1, :]) + (w[..., 2, :] + w[..., 3, :])


def block_sums(term):
    """term [nq, 32] -> (partial [ceil(nq / 256), 32], sums [32]) in the header's order of additions."""
    term = np.asarray(term, np.float64).reshape(-1, TERMS)
    nb = (len(term) + TILE - 1) // TILE
    padded = np.zeros((nb * TILE, TERMS))
    padded[:len(term)] = term
    partial = _workgroup(padded.reshape(nb, TILE, TERMS)) if nb else np.zeros((0, TERMS))
    lanes = np.zeros((TILE, TERMS))
    for s in range(0, nb, TILE):                               # lane l: b = l, l + 256, .. ascending
        blk = partial[s:s + TILE]
        lanes[:len(blk)] = lanes[:len(blk)] + blk
    return partial, _workgroup(lanes)


def solve(sums, L, min_eig_ratio=1e-6):
    """-> (omega [3], dt [3], kept)."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[:21]
    A = A + np.triu(A, 1).T
    g = np.asarray(sums[21:27], np.float64)
    lam, vec = np.linalg.eigh(A)
    keep = lam > min_eig_ratio * lam.max()
    x = -sum((vec[:, i] * (vec[:, i] @ g) / lam[i] for i in np.nonzero(keep)[0]), np.zeros(6))
    return x[:3] / L, x[3:], int(keep.sum())


def rodrigues(omega):
    theta = np.linalg.norm(omega)
    if theta == 0:
        return np.eye(3)
    k = omega / theta
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def target_normals(target, radius, k):
    d2, index = filter_ref.knn(target, radius, k)
    _, index, count = filter_ref.cut(d2, index, radius, k)
    normal, _, flag, _ = filter_ref.normals(target, index, count)
    return normal, flag


def icp(source, target, D, max_iter=50, tol=None, huber=None, k=16, min_eig_ratio=1e-6, prepared=None):
    """The loop of the issue in fp64 -> dict(R, t, pivot, iterations, converged, constrained_dof, history, index: the
    correspondences of every evaluation).  prepared: (normal, flag) of the target, computed once by target_normals."""
    source, target = np.asarray(source, np.float64), np.asarray(target, np.float64)
    c = (target.min(0) + target.max(0)) / 2.0
    L = max(0.5 * np.linalg.norm(target.max(0) - target.min(0)), D)
    rho = np.linalg.norm(source - c, axis=1).max()
    normal, flag = prepared if prepared is not None else target_normals(target, D, k)
    tol = 1e-3 * D if tol is None else tol
    R, t = np.eye(3), np.zeros(3)
    history, indices, converged, constrained = [], [], False, 6

    def evaluate():
        y = apply(source, R, c, t)
        _, index, _, _ = accuracy_ref.nearest(target, y, D)
        indices.append(index)
        term, pair = rows(y, index, target, normal, flag, c, L, huber or 0.0)
        return block_sums(term)[1]

    for _ in range(max_iter):
        s = evaluate()
        omega, dt, kept = solve(s, L, min_eig_ratio)
        dR = rodrigues(omega)
        R, t = dR @ R, dR @ t + dt
        step = np.linalg.norm(omega) * rho + np.linalg.norm(dt)
        history.append(dict(pairs=int(s[30]), rms_plane=float(np.sqrt(s[28] / s[30])), rms_point=float(np.sqrt(s[29] / s[30])),
                            step=float(step), kept=kept))
        constrained = min(constrained, kept)
        if step <= tol:
            converged = True
            break
    s = evaluate()
    return dict(R=R, t=t, pivot=c, iterations=len(history), converged=converged, constrained_dof=constrained, history=history,
                index=indices, rms_plane_after=float(np.sqrt(s[28] / s[30])), pairs_after=int(s[30]))
