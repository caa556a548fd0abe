"""Inputs of the mesh-cleaning tests: the welded box and sphere of tests/smooth_inputs.py with holes punched into them, a scene
of floaters, a flat grid with holes of exact rim lengths, and a hand-made mesh that holds every case of the rule once."""
import numpy as np

import smooth_inputs as SI

BOX_AREA_THRESHOLD = 500.0        # between the shrunk sphere (4 pi 2.5^2 ~ 78.5) and the box (~ 2093), far from both


def punch(xyz, rgb, faces, seed, allowed=None, vertices=8, singles=8):
    """The mesh without the faces around `vertices` random vertices and without `singles` random single faces, chosen (from the
    faces whose corners are all `allowed`) so that no two holes share a vertex -> (xyz, rgb, faces left, holes made)."""
    rng = np.random.default_rng(seed)
    ok_vertex = np.ones(len(xyz), bool) if allowed is None else allowed.copy()
    # a vertex may be the centre of a hole only if all its faces have allowed corners
    face_ok = ok_vertex[faces].all(1)
    centre_ok = ok_vertex.copy()
    np.logical_and.at(centre_ok, faces.reshape(-1), np.repeat(face_ok, 3))
    taken = np.zeros(len(xyz), bool)                                  # vertices on or next to a hole made so far
    remove = np.zeros(len(faces), bool)

    def neighbourhood(vs):
        """The vertices of every face that touches one of vs: a hole is made only where none of them is on a hole already."""
        return np.unique(faces[np.isin(faces, vs).any(1)])

    holes = 0
    for v in rng.permutation(np.nonzero(centre_ok)[0]).tolist():
        if holes == vertices:
            break
        fan = (faces == v).any(1)
        rim = np.unique(faces[fan])
        if taken[neighbourhood(rim)].any():
            continue
        remove |= fan
        taken[rim] = True
        holes += 1
    for f in rng.permutation(np.nonzero(face_ok)[0]).tolist():
        if holes == vertices + singles:
            break
        if taken[neighbourhood(faces[f])].any():
            continue
        remove[f] = True
        taken[faces[f]] = True
        holes += 1
    assert holes == vertices + singles
    return xyz, rgb, faces[~remove], holes


def punched(name, flat=False):
    """The box or the sphere of smooth_inputs.meshes() with 16 holes; flat: only where the box is flat (farther than 2 from an edge)."""
    xyz, rgb, faces = SI.meshes()[name]
    allowed = SI.box_edge_distance(xyz) > 2.0 if flat else None
    return punch(xyz, rgb, faces, 11 if name == "box" else 12, allowed)


def tetrahedron(at, size=0.5):
    at = np.asarray(at, np.float64)
    v = at + size * np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float64)
    return v, np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)], np.int64)


def floaters():
    """The box, the sphere shrunk to a quarter and shifted clear of it, and three tiny tetrahedra -> (xyz, rgb, faces, the
    number of box faces).  The box's faces come first."""
    m = SI.meshes()
    bx, bc, bf = m["box"]
    sx, sc, sf = m["sphere"]
    centre = np.asarray([32.37, 31.81, 32.23])
    parts = [(bx, bc, bf), ((sx - centre) * 0.25 + centre + np.array([40.0, 0.0, 0.0]), sc, sf)]
    for at in ((80.0, 10.0, 10.0), (5.0, 70.0, 12.0), (33.0, 33.0, 90.0)):
        v, f = tetrahedron(at)
        parts.append((v, SI.colours(4), f))
    base, xs, cs, fs = 0, [], [], []
    for x, c, f in parts:
        xs.append(x), cs.append(c), fs.append(f + base)
        base += len(x)
    return np.concatenate(xs), np.concatenate(cs), np.concatenate(fs), len(bf)


# ---- the grid with holes of exact rim lengths -------------------------------------------------------------------------------------
GRID = 40
RIMS = (3, 4, 31, 32, 33, 64, 65, 200)
OUTER_RIM = 4 * GRID


def grid_holes():
    """A flat grid of 40 x 40 quads, each cut into T0 = (a, b, d) and T1 = (a, d, c) (a the quad's low corner, b right, c up,
    d opposite), without the faces of eight regions that lie a cell apart.  A region of w x h whole quads has a rim of
    2 (w + h) edges; a T1 attached to its right side adds one.
      row 1: T0 of quad (1, 1): 3;  quad (3, 1): 4
      row 3: quads x = 1 .. 14 and T1 of (15, 3): 31        row 5: quads x = 1 .. 15: 32
      row 7: quads x = 1 .. 15 and T1 of (16, 7): 33        rows 9, 10: quads x = 1 .. 30: 64
      rows 12, 13: quads x = 1 .. 30 and T1 of (31, 12): 65
      a comb: the spine, row 15, quads x = 1 .. 38 (78) with teeth on every other column x = 1, 3, .. 37, the first four 4 quads
      high and the other fifteen 3 (2 x 61 more): 200
    -> (xyz, rgb, faces)."""
    n = GRID + 1
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="xy"), -1).reshape(-1, 2)      # vertex y * n + x
    xyz = np.concatenate([ij.astype(np.float64), np.zeros((len(ij), 1))], 1)
    gone = set()

    def quads(x0, x1, y0, y1):
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                gone.update([(x, y, 0), (x, y, 1)])

    gone.add((1, 1, 0))
    quads(3, 3, 1, 1)
    quads(1, 14, 3, 3), gone.add((15, 3, 1))
    quads(1, 15, 5, 5)
    quads(1, 15, 7, 7), gone.add((16, 7, 1))
    quads(1, 30, 9, 10)
    quads(1, 30, 12, 13), gone.add((31, 12, 1))
    quads(1, 38, 15, 15)
    for t, x in enumerate(range(1, 38, 2)):
        quads(x, x, 16, 16 + (4 if t < 4 else 3) - 1)
    F = []
    for y in range(GRID):
        for x in range(GRID):
            a, b, c, d = y * n + x, y * n + x + 1, (y + 1) * n + x, (y + 1) * n + x + 1
            if (x, y, 0) not in gone:
                F.append((a, b, d))
            if (x, y, 1) not in gone:
                F.append((a, d, c))
    return xyz, SI.colours(len(xyz)), np.array(F, np.int64)


# ---- the hand-made mesh --------------------------------------------------------------------------------------------------------------
def hand_mesh():
    """Every coordinate a multiple of 1/8 -> (xyz, rgb, faces).
      a sheet of 8 x 4 quads (vertices 0 .. 44, vertex y * 9 + x; T0 and T1 as in grid_holes), gently folded, without
        T0 of quad (1, 1): a triangle hole;  quad (3, 2): a square hole;
        T0 of quad (4, 1) and T0 of quad (5, 2): two holes pinched at vertex (5, 2), both of which stay open;
        T0 of quad (6, 1): a triangle hole next to the edge (7, 2) - (7, 3), which a fin (to vertex 45) makes an edge of three faces:
        vertex (7, 2) is entered twice, so that hole stays open as well, and so does the fin's own chain;
      two tetrahedra joined at one vertex (46 .. 52): one component of 8 faces, closed;
      a lone triangle (53 .. 55);  vertex 56, which no face uses;
      vertex 57 at the position of 53, and the face (53, 57, 54): degenerate after the weld."""
    n = 9
    V = [(x * 1.0, y * 1.0, (x % 2) * 0.125 + (y % 3) * 0.25) for y in range(5) for x in range(n)]
    gone = {(1, 1, 0), (3, 2, 0), (3, 2, 1), (4, 1, 0), (5, 2, 0), (6, 1, 0)}
    F = []
    for y in range(4):
        for x in range(8):
            a, b, c, d = y * n + x, y * n + x + 1, (y + 1) * n + x, (y + 1) * n + x + 1
            if (x, y, 0) not in gone:
                F.append((a, b, d))
            if (x, y, 1) not in gone:
                F.append((a, d, c))
    V.append((7.5, 2.5, 1.5))                                            # 45: the fin's tip
    F.append((2 * n + 7, 3 * n + 7, 45))
    t = len(V)                                                            # 46
    V += [(12.0, 0.0, 0.0), (13.0, 0.0, 0.0), (12.0, 1.0, 0.0), (12.0, 0.0, 1.0),          # the first tetrahedron, 49 shared
          (12.0, 0.0, 2.0), (13.0, 0.0, 2.0), (12.0, 1.0, 2.0)]
    F += [(t, t + 2, t + 1), (t, t + 1, t + 3), (t + 1, t + 2, t + 3), (t + 2, t, t + 3),
          (t + 3, t + 5, t + 4), (t + 3, t + 4, t + 6), (t + 4, t + 5, t + 6), (t + 5, t + 3, t + 6)]
    V += [(20.0, 0.0, 0.0), (21.0, 0.0, 0.125), (20.0, 1.0, 0.25)]        # 53 .. 55: the lone triangle
    F.append((53, 54, 55))
    V.append((7.5, 7.5, 7.5))                                            # 56: no face
    V.append((20.0, 0.0, 0.0))                                           # 57 = 53
    F.append((53, 57, 54))
    xyz = np.array(V, np.float64)
    return xyz, SI.colours(len(V)), np.array(F, np.int64)


def scrambled_strip(nf, seed=3):
    """A strip of nf faces whose vertex k sits at x = perm(k): the weld numbers the vertices by position, so the welded numbers
    are a random permutation along the strip and the smallest label has to travel its whole length."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(nf + 2).astype(np.float64)
    xyz = np.stack([perm, np.arange(nf + 2) % 2 * 1.0, np.zeros(nf + 2)], 1)
    faces = np.array([(k, k + 1, k + 2) if k % 2 == 0 else (k + 1, k, k + 2) for k in range(nf)], np.int64)
    return xyz, SI.colours(nf + 2), faces


def renumbered_strip(nf, seed=5):
    """smooth_inputs.strip(nf) with its vertex numbers reversed and then randomly permuted (the positions go with the numbers)."""
    xyz, rgb, faces = SI.strip(nf)
    n = len(xyz)
    new = (n - 1 - np.arange(n))[np.random.default_rng(seed).permutation(n)]           # old number -> new number
    x2, c2 = np.empty_like(xyz), np.empty_like(rgb)
    x2[new], c2[new] = xyz, rgb
    return x2, c2, new[faces]


def disjoint_triangles(n):
    """n triangles apart from each other."""
    k = np.arange(n)
    base = np.stack([(k % 20) * 2.0, (k // 20) * 2.0, np.zeros(n)], 1)
    xyz = (base[:, None, :] + np.array([(0.0, 0, 0), (1.0, 0, 0.125), (0.0, 1.0, 0.25)])[None]).reshape(-1, 3)
    return xyz, SI.colours(3 * n), np.arange(3 * n).reshape(n, 3)
