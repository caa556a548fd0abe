"""Inputs of the cloud-distance tests (tests/test_accuracy_host.py, tests/test_accuracy_gpu.py): a hand-made pair of clouds that
meets every rule of include/adamvs_hip.h "Cloud distance" once, and the seeded random clouds.

The hand-made input has D = 1 and coordinates in multiples of 1/8.  With the lattice origin HAND_ORIGIN = (0, 0, 0) every cell
centre is a multiple of 1/2, every q - C and p - C a multiple of 1/8 below 2, and every fp32 operation of the search exact, so
d2 and index must equal the fp64 brute force bit for bit.  (With the driver's default origin, min - c / 3 - c, the centres are
not dyadic and the 1e-6 c bound applies instead; the cases at the lattice's last cell do not fit such a lattice and are
left out there: `last_cell=False`.)"""
import numpy as np

HAND_D = 1.0
HAND_ORIGIN = (0.0, 0.0, 0.0)
LAST = float((1 << 21) - 1)         # the last cell of an axis spans [LAST, LAST + 1)


def hand_made(last_cell=True, seed=5):
    """-> (targets [nt, 3], queries [nq, 3]) fp64, both in a seeded order, and a dict of named query numbers."""
    T, Q, names = [], [], {}

    def q(name, *p):
        names.setdefault(name, []).append(len(Q))
        Q.append(p)

    # the nearest target in each of the 26 neighbour cells: the query sits towards that cell, a farther target in its own cell
    k = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == dy == dz == 0:
                    continue
                b = np.array([10.5 + 5.0 * k, 10.5, 10.5])
                d = np.array([dx, dy, dz], np.float64)
                q("neighbour", *(b + 0.375 * d))
                T.append(b + 0.625 * d)          # in the neighbour cell, at 0.25 |d|
                T.append(b - 0.375 * d)          # in the query's cell, at 0.75 |d|
                k += 1
    # exactly D is kept, D + 1/8 is not
    q("at_D", 10.5, 30.5, 10.5), T.append((11.5, 30.5, 10.5))
    q("past_D", 20.5, 30.5, 10.5), T.append((21.625, 30.5, 10.5))
    # inside the 27 cells only a target at 1.75; a nearer one (1.25) two cells away must not be found: nothing within D
    q("two_cells", 30.125, 30.5, 10.5), T.append((31.875, 30.5, 10.5)), T.append((28.875, 30.5, 10.5))
    # points exactly on cell faces, edges and corners
    q("on_face", 40.0, 30.5, 10.5), T.append((39.5, 30.5, 10.5)), T.append((41.0, 30.5, 10.5))
    q("on_face", 45.0, 31.0, 11.0), T.append((44.25, 31.0, 11.0)), T.append((45.0, 32.0, 11.0))
    # the lattice's first cell on every axis, and on all three
    q("first_cell", 0.5, 50.5, 50.5), T.append((1.25, 50.5, 50.5))
    q("first_cell", 50.5, 0.5, 50.5), T.append((50.5, 1.25, 50.5))
    q("first_cell", 50.5, 50.5, 0.5), T.append((50.5, 50.5, 1.25))
    q("first_cell", 0.5, 0.5, 0.5), T.append((0.25, 0.5, 0.5)), T.append((1.125, 0.5, 0.5))
    if last_cell:
        q("last_cell", LAST + 0.5, 60.5, 60.5), T.append((LAST - 0.25, 60.5, 60.5))
        q("last_cell", 60.5, LAST + 0.5, 60.5), T.append((60.5, LAST - 0.25, 60.5))
        q("last_cell", 60.5, 60.5, LAST + 0.5), T.append((60.5, 60.5, LAST - 0.25))
        q("last_cell", LAST + 0.5, LAST + 0.5, LAST + 0.5), T.append((LAST + 0.25, LAST + 0.5, LAST + 0.5))
        q("last_cell", LAST + 0.875, LAST + 0.875, LAST + 0.125), T.append((LAST + 0.875, LAST + 0.125, LAST - 0.25))
    # a query in an unoccupied cell with a target next door, and one with nothing around
    q("empty_cell", 70.5, 30.5, 10.5), T.append((71.25, 30.5, 10.5))
    q("empty_cell", 80.5, 80.5, 80.5)
    # queries outside the lattice, by more than one cell, and queries that are not finite: no candidates, no error
    q("outside", -2.5, 10.5, 10.5)
    q("outside", 10.5, -1.5, 10.5)
    if last_cell:
        q("outside", LAST + 4.5, 60.5, 60.5)
    q("outside", np.nan, 30.5, 10.5)
    q("outside", 40.0, np.inf, 10.5)
    # exact duplicates, and two distinct targets at the same distance in different cells: the lowest number wins
    q("duplicate", 90.5, 30.5, 10.5)
    for _ in range(3):
        T.append((90.75, 30.5, 10.5))
    q("tie", 95.5, 30.5, 10.5), T.append((96.25, 30.5, 10.5)), T.append((94.75, 30.5, 10.5))
    # one target cell with 300 points (more than one tile of 256) on the 1/8 grid, queries in it and next to it
    grid = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3) / 8.0
    for g in grid[:300]:
        T.append(np.array([100.0, 30.0, 10.0]) + g)
    q("full_cell", 100.5, 30.5, 10.5), q("full_cell", 101.25, 30.0, 10.0), q("full_cell", 99.875, 30.875, 10.875)
    # one query cell with 300 queries (a split run), a few targets in and around it
    for g in grid[:300]:
        q("full_query_cell", *(np.array([110.0, 30.0, 10.0]) + g))
    T.extend([(110.5, 30.5, 10.5), (110.125, 30.125, 10.875), (111.0, 30.0, 10.0), (109.875, 29.875, 9.875), (110.25, 31.25, 10.5)])
    T, Q = np.array(T, np.float64), np.array(Q, np.float64)
    rng = np.random.default_rng(seed)
    pt, pq = rng.permutation(len(T)), rng.permutation(len(Q))
    inv = np.empty(len(Q), np.int64)
    inv[pq] = np.arange(len(Q))
    return T[pt], Q[pq], {name: inv[np.array(v)] for name, v in names.items()}


def random_clouds(seed=11, n=30000):
    """30 000 targets on [0, 40]^2 with sigma_z = 0.05 and 30 000 queries on [-1, 41]^2 with sigma_z = 0.3; D = 0.5."""
    rng = np.random.default_rng(seed)
    T = np.concatenate([rng.uniform(0.0, 40.0, (n, 2)), rng.normal(0.0, 0.05, (n, 1))], 1)
    Q = np.concatenate([rng.uniform(-1.0, 41.0, (n, 2)), rng.normal(0.0, 0.3, (n, 1))], 1)
    return T, Q, 0.5
