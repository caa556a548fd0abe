"""Inputs and bars that tests/test_filter_host.py (the host twins) and tests/test_filter_gpu.py (the device path) share, so that
both hold the same cases to the same numbers.  The bars are those of include/adamvs_hip.h "Cloud neighbourhoods": where every
fp32 operation is exact the result equals the fp64 brute force bit for bit; elsewhere |d - d_fp64| <= 1e-6 c, a count may differ
only where a candidate lies within 1e-6 c of R, an index only where two of the reference's slots lie within 2e-6 c of each other,
and at most 1e-3 of the queries may be set aside for either reason."""
import numpy as np

import accuracy_inputs as I
import filter_ref as F

HAND_KS = (1, 8, 9, 16, 32)      # 9 and 16 take the kernel's form for k <= 16, 9 with a list that is not full width
TIE_CENTRES = {1: (200.5, 30.5, 10.5), 8: (220.5, 30.5, 10.5), 32: (240.5, 30.5, 10.5), 9: (260.5, 30.5, 10.5), 16: (280.5, 30.5, 10.5)}
TIE_PAIR = ((0.75, 0.0, 0.0), (-0.75, 0.0, 0.0))            # the k-th and the (k + 1)-th candidate: both at d2 = 0.5625


def hand_cloud(seed=9):
    """The targets of accuracy_inputs.hand_made() (the cell of 300 points, the three exact duplicates, the equal-distance pair,
    the first and last lattice cells, points on cell faces, isolated points) and, per k of HAND_KS, a cluster far from everything:
    a centre with exactly k + 1 candidates within R = 1, k - 1 of them nearer than the last two, which are equidistant.  All
    coordinates are multiples of 1/8, so with the origin (0, 0, 0) every fp32 operation is exact.  -> the cloud in a seeded order."""
    T, _, _ = I.hand_made()
    g = np.arange(-4, 5) / 8.0
    off = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    d2 = (off ** 2).sum(1)
    near = off[(d2 > 0) & (d2 < 0.5625)]
    near = near[np.argsort((near ** 2).sum(1), kind="stable")]
    extra = []
    for k in HAND_KS:
        c = np.array(TIE_CENTRES[k])
        extra += [c] + [c + o for o in near[:k - 1]] + [c + np.array(o) for o in TIE_PAIR]
    P = np.concatenate([T, np.array(extra)])
    return P[np.random.default_rng(seed).permutation(len(P))]


def find(P, p):
    hit = np.nonzero((P == np.asarray(p)).all(1))[0]
    assert len(hit) >= 1
    return hit


def check_hand_cloud(P, k, d2, index, count):
    """The result of the search on hand_cloud() at R = 1, origin (0, 0, 0): exact, and the rules by name."""
    ref = F.knn(P, 1.0, k)
    want_d2, want_index, want_count = F.cut(ref[0], ref[1], 1.0, k)
    assert d2.dtype == np.float32 and index.dtype == np.int32 and count.dtype == np.int32 and d2.shape == index.shape == (len(P), k)
    assert np.array_equal(d2.astype(np.float64), want_d2)
    assert np.array_equal(index.astype(np.int64), want_index)
    assert np.array_equal(count.astype(np.int64), want_count)
    # by name, so that a wrong restatement cannot hide a wrong search
    dup = find(P, (90.75, 30.5, 10.5))
    assert len(dup) == 3
    for i in dup:                                           # the other two duplicates are neighbours at d2 = 0, the lower number first
        others = sorted(set(dup) - {i})
        assert list(index[i, :min(k, 2)]) == others[:min(k, 2)] and (d2[i, :min(k, 2)] == 0.0).all()
    lone = find(P, (31.875, 30.5, 10.5))[0]                 # nothing within R (the nearest other point is 1.75 away)
    assert count[lone] == 0 and np.isinf(d2[lone]).all() and (index[lone] == -1).all()
    centre = find(P, TIE_CENTRES[k])[0]
    a, b = (find(P, np.array(TIE_CENTRES[k]) + np.array(o))[0] for o in TIE_PAIR)
    assert count[centre] == k and index[centre, k - 1] == min(a, b) and d2[centre, k - 1] == 0.5625
    assert max(a, b) not in index[centre]
    full = find(P, (100.5, 30.5, 10.5))[0]                  # inside the cell of 300 points: more than one candidate tile
    assert count[full] == k and d2[full, 0] == 0.015625
    first, last = find(P, (0.25, 0.5, 0.5))[0], find(P, (I.LAST + 0.25, I.LAST + 0.5, I.LAST + 0.5))[0]
    assert index[first, 0] == find(P, (1.125, 0.5, 0.5))[0] and count[first] == 1 and count[last] == 0
    return want_d2, want_index, want_count


def hold(d2, index, count, ref, R, k):
    """The search on a random cloud against ref = filter_ref.knn(..) as the module docstring says -> (largest error over the bound,
    queries set aside at R, queries set aside as ties, share of full rows)."""
    c = float(R)
    bound = 1e-6 * c
    rd = np.sqrt(ref[0])
    with np.errstate(invalid="ignore"):
        at_R = (np.abs(rd - R) <= bound).any(1)
        tie = ((rd[:, 1:] - rd[:, :-1] <= 2.0 * bound) & (rd[:, :-1] <= R + bound)).any(1)
    want_d2, want_index, want_count = F.cut(ref[0], ref[1], R, k)
    d, want = np.sqrt(d2.astype(np.float64)), np.sqrt(want_d2)
    assert np.array_equal(np.sort(d, 1), d)                 # ascending, the padding last
    assert np.array_equal(count, np.isfinite(d).sum(1)) and np.array_equal(index >= 0, np.isfinite(d))
    both = np.isfinite(d) & np.isfinite(want)
    err = float(np.abs(d[both] - want[both]).max())
    print("largest |d - d_fp64| = %.3e = %.3f of the bound %.3e" % (err, err / bound, bound))
    assert err <= bound
    assert np.array_equal(count[~at_R], want_count[~at_R])
    ok = ~at_R & ~tie
    assert np.array_equal(index[ok].astype(np.int64), want_index[ok])
    full = float((count == k).mean())
    print("set aside: %d at R, %d ties of %d; %.1f %% of rows full, %.1f %% with count < 3"
          % (at_R.sum(), tie.sum(), len(d), 100.0 * full, 100.0 * (count < 3).mean()))
    assert (at_R | tie).mean() <= 1e-3
    return err / bound, int(at_R.sum()), int(tie.sum()), full


def check_permuted(P, perm, base, permuted):
    """Search of P[perm] against the search of P: the rows permuted accordingly, the numbers mapped, bit for bit.  Within a run of
    equal fp32 d2 the order goes by number, which the permutation changes, so each row is brought back into the order (d2, number)
    after the mapping; a tie across the last place would change the set itself and is asserted absent from the input."""
    d2, index, count = base
    pd2, pindex, pcount = permuted
    assert pd2.tobytes() == d2[perm].tobytes() and np.array_equal(pcount, count[perm])
    mapped = np.where(pindex >= 0, perm[np.maximum(pindex, 0)], -1)
    key = np.where(mapped >= 0, mapped, np.iinfo(np.int64).max)
    order = np.lexsort((key, pd2), axis=1)
    assert np.array_equal(np.take_along_axis(mapped, order, 1), index[perm])


def normals_cases():
    """Hand-made clouds of 16 points on the 1/8 grid (means and covariances are then exact): -> {name: (points, want normal)}."""
    g = np.arange(4) / 8.0
    a, b = (v.reshape(-1) for v in np.meshgrid(g, g, indexing="ij"))
    zero = np.zeros(16)
    s = np.sqrt(0.5)
    return {"plane": (np.stack([a, b, zero + 0.25], 1) + 5.0, (0.0, 0.0, 1.0)),
            "wall_x": (np.stack([zero + 0.5, a, b], 1) + 5.0, (1.0, 0.0, 0.0)),          # n_z = n_y = 0: n_x must be positive
            "wall_xy": (np.stack([a, a, b], 1) + 5.0, (-s, s, 0.0)),                       # n_z = 0: n_y positive, the normal along -x
            "wall_y": (np.stack([a, zero + 0.5, b], 1) + 5.0, (0.0, 1.0, 0.0))}


def check_normals(points, index, count, normal, curvature, flag):
    """Normals on the kernel's own neighbour lists (row r is point r) against eigh -> (largest angle over its bar, share set aside).
    Bar: angle <= 1e-12 lambda2 / (lambda1 - lambda0) for valid points (sin theta <= |E| / gap with |E| a few hundred roundings of
    2^-53 on |C|; the bar leaves about 50x over that); points with lambda1 - lambda0 <= 1e-6 lambda2 are set aside, at most 1e-3."""
    want_n, want_c, want_f, lam = F.normals(points, index, count)
    assert np.array_equal(flag, want_f)
    valid = flag == F.VALID
    assert (normal[~valid] == 0.0).all() and (curvature[~valid] == 0.0).all()
    assert np.abs(np.linalg.norm(normal[valid], axis=1) - 1.0).max() <= 4e-16
    lead = np.where(normal[:, 2] != 0, normal[:, 2], np.where(normal[:, 1] != 0, normal[:, 1], normal[:, 0]))
    assert (lead[valid] > 0).all()                          # upward, exactly
    assert np.abs(curvature.astype(np.float64) - want_c).max() <= 1e-6 and curvature.dtype == np.float32
    gap = lam[:, 1] - lam[:, 0]
    aside = valid & ~(gap > 1e-6 * lam[:, 2])
    held = valid & ~aside
    angle = np.arcsin(np.minimum(np.linalg.norm(np.cross(normal[held], want_n[held]), axis=1), 1.0))
    bar = 1e-12 * lam[held, 2] / gap[held]
    worst = float((angle / bar).max())
    print("normals: largest angle = %.3e of its bar over %d valid points; %d set aside (%.2e), %d too few, %d collinear"
          % (worst, held.sum(), aside.sum(), aside.mean(), (flag == F.TOO_FEW).sum(), (flag == F.COLLINEAR).sum()))
    assert aside.mean() <= 1e-3
    assert worst <= 1.0
    return worst, float(aside.mean())
