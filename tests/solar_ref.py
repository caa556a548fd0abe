"""The solar stage restated in numpy (include/adamvs_hip.h "Solar"): the direction table, the weights and the sector function
from their definitions, the horizon by brute force over every distance and again as the hull walk along the lattice lines, the
sky-view factor as the explicit k loop, the exposure and the plane sums in int64.  Nothing here is shared with
ada_mvs_amd/solar.py; the tests hold the two and the kernels to one another by equality."""
import math

import numpy as np

NONE = -2 ** 31
WINDOW = 16                                         # ADAMVS_SOLAR_STACK_WINDOW
TWO_PI = 2.0 * math.pi


# ---- directions ---------------------------------------------------------------------------------------------------------------
def directions(K):
    """-> [(di, dj)] * K sorted by the azimuth atan2(dj, -di) mod 2 pi: north first, clockwise."""
    reach = {8: 1, 16: 2, 32: 3}[K]
    d = [(di, dj) for di in range(-reach, reach + 1) for dj in range(-reach, reach + 1) if math.gcd(abs(di), abs(dj)) == 1]
    d.sort(key=lambda p: math.atan2(p[1], -p[0]) % TWO_PI)
    assert len(d) == K
    return d


def azimuths(K):
    return np.array([math.atan2(dj, -di) % TWO_PI for di, dj in directions(K)])


def weights(K):
    """Half the angular gap to each cyclic neighbour, over 2 pi."""
    az = azimuths(K)
    w = np.zeros(K)
    for k in range(K):
        nxt, prv = (az[(k + 1) % K] - az[k]) % TWO_PI, (az[k] - az[k - 1]) % TWO_PI
        w[k] = (nxt + prv) / 2.0 / TWO_PI
    return w


def sector(az, K):
    """The k at the smallest angular distance from az; a tie (within 1e-12 rad) goes to the smaller k."""
    a = azimuths(K)
    d = np.abs(a - float(az) % TWO_PI)
    d = np.minimum(d, TWO_PI - d)
    return int(np.flatnonzero(d <= d.min() + 1e-12)[0])


# ---- the lattice lines --------------------------------------------------------------------------------------------------------
def line_count(H, W, di, dj):
    a, b = min(abs(di), H), min(abs(dj), W)
    return a * W + (H - a) * b


def line_start(l, H, W, di, dj):
    """Line l of the look direction (di, dj) -> its first cell (i, j): the lines are walked along w = -d; first the min(|di|, H) full
    rows on the side they enter from, then the first (wj > 0) or last min(|dj|, W) columns of the remaining rows."""
    wi, wj = -di, -dj
    a, b = min(abs(di), H), min(abs(dj), W)
    if l < a * W:
        r, j = divmod(l, W)
        return (r if wi > 0 else H - a + r), j
    r, c = divmod(l - a * W, b)
    return (a + r if wi > 0 else r), (c if wj > 0 else W - b + c)


def line_cells(l, H, W, di, dj):
    i, j = line_start(l, H, W, di, dj)
    cells = []
    while 0 <= i < H and 0 <= j < W:
        cells.append((i, j))
        i, j = i - di, j - dj
    return cells


# ---- the horizon --------------------------------------------------------------------------------------------------------------
def horizon_brute(s, K):
    """s int [H, W] (NONE outside V) -> (hz_n, hz_h) int64 [K, H, W]: every distance n = 1 .. max(H, W), kept on a strict
    improvement of h / n, so the nearest of equals stays."""
    s = np.asarray(s, np.int64)
    H, W = s.shape
    V = s != NONE
    hz_n, hz_h = np.zeros((K, H, W), np.int64), np.zeros((K, H, W), np.int64)
    for k, (di, dj) in enumerate(directions(K)):
        bn, bh = hz_n[k], hz_h[k]
        for n in range(1, max(H, W) + 1):
            a, b = n * di, n * dj
            i0, i1, j0, j1 = max(0, -a), min(H, H - a), max(0, -b), min(W, W - b)
            if i0 >= i1 or j0 >= j1:
                break
            here, there = (slice(i0, i1), slice(j0, j1)), (slice(i0 + a, i1 + a), slice(j0 + b, j1 + b))
            h = s[there] - s[here]
            better = V[here] & V[there] & (h > 0) & ((bh[here] == 0) | (h * bn[here] > bh[here] * n))
            bn[here] = np.where(better, n, bn[here])
            bh[here] = np.where(better, h, bh[here])
    return hz_n, hz_h


def horizon_hull(s, K, collapse=True):
    """The same by the hull walk of the header, line by line -> (hz_n, hz_h, dict(lines, deepest, spills)): spills counts the
    pushes into a full window of WINDOW entries.  collapse=False is the plain loop that pushes every cell: the same horizon from
    a deeper stack."""
    s = np.asarray(s, np.int64)
    H, W = s.shape
    hz_n, hz_h = np.zeros((K, H, W), np.int64), np.zeros((K, H, W), np.int64)
    lines = deepest = spills = 0
    for k, (di, dj) in enumerate(directions(K)):
        for l in range(line_count(H, W, di, dj)):
            lines += 1
            stack, inwin = [], 0
            for m, (i, j) in enumerate(line_cells(l, H, W, di, dj)):
                v = int(s[i, j])
                if v == NONE:
                    continue
                collinear = False
                while len(stack) >= 2:
                    inwin = max(inwin, 2)
                    (m2, v2), (m1, v1) = stack[-2], stack[-1]
                    far, near = (v2 - v) * (m - m1), (v1 - v) * (m - m2)
                    if far > near:
                        stack.pop()
                        inwin -= 1
                    else:
                        collinear = far == near
                        break
                if stack and stack[-1][1] > v:
                    hz_n[k, i, j], hz_h[k, i, j] = m - stack[-1][0], stack[-1][1] - v
                if collinear and collapse:          # the top lies between its neighbours on the hull: the cell takes its place
                    stack[-1] = (m, v)
                    continue
                if inwin == WINDOW:
                    spills += 1
                    inwin -= 1
                stack.append((m, v))
                inwin += 1
                deepest = max(deepest, len(stack))
    return hz_n, hz_h, dict(lines=lines, deepest=deepest, spills=spills)


# ---- the sky-view factor --------------------------------------------------------------------------------------------------------
def svf(s, hz_n, hz_h, w, q):
    """The k loop of step 4 -> float64 [H, W]: every numpy operation is one correctly rounded fp64 operation."""
    s = np.asarray(s, np.int64)
    K = hz_n.shape[0]
    acc = np.zeros(s.shape, np.float64)
    for k, (di, dj) in enumerate(directions(K)):
        n, h = hz_n[k].astype(np.float64), hz_h[k].astype(np.float64)
        L2 = (n * n) * (float(di * di + dj * dj) * float(q))
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(hz_h[k] == 0, 1.0, L2 / (L2 + h * h))
        acc = acc + float(w[k]) * t
    return np.where(s == NONE, 0.0, acc)


# ---- the exposure and the plane sums ----------------------------------------------------------------------------------------------
def expose(s, hz_n, hz_h, table, label=None, normal=None):
    """table: dict(sector, thr, minutes, energy, sun [T, 3]) -> (minutes, direct) int64 [H, W]."""
    s = np.asarray(s, np.int64)
    V = s != NONE
    nrm = np.zeros(s.shape + (3,), np.int64)
    nrm[..., 2] = 32768
    if label is not None:
        lab = np.asarray(label, np.int64)
        nrm = np.where((lab > 0)[..., None], np.asarray(normal, np.int64)[lab], nrm)
    minutes, direct = np.zeros(s.shape, np.int64), np.zeros(s.shape, np.int64)
    for t in range(len(table["sector"])):
        k, thr = int(table["sector"][t]), float(table["thr"][t])
        n, h = hz_n[k], hz_h[k]
        lit = V & ~((h > 0) & (h.astype(np.float64) > thr * n.astype(np.float64)))
        sun = np.asarray(table["sun"], np.int64)[t]
        dot = np.clip(nrm[..., 0] * sun[0] + nrm[..., 1] * sun[1] + nrm[..., 2] * sun[2], 0, 2 ** 30)
        minutes += np.where(lit, int(table["minutes"][t]), 0)
        direct += np.where(lit, (int(table["energy"][t]) * dot) >> 30, 0)
    return minutes, direct


def plane_sums(s, minutes, direct, label=None, P=0):
    """-> int64 [3, P + 1]: cells, minutes, direct per label over V."""
    V = np.asarray(s, np.int64) != NONE
    lab = np.zeros(V.shape, np.int64) if label is None else np.asarray(label, np.int64)
    table = np.zeros((3, P + 1), np.int64)
    np.add.at(table[0], lab[V], 1)
    np.add.at(table[1], lab[V], np.asarray(minutes, np.int64)[V])
    np.add.at(table[2], lab[V], np.asarray(direct, np.int64)[V])
    return table


def surface(z, z_ref=0.0):
    """z float [H, W] (NaN: no value) -> s int64: llrint((z - z_ref) 256), NONE outside V."""
    z = np.asarray(z, np.float32).astype(np.float64)
    ok = np.isfinite(z) & (np.abs(z - z_ref) <= 8191.0)
    return np.where(ok, np.rint(np.where(ok, z - z_ref, 0.0) * 256.0), NONE).astype(np.int64)
