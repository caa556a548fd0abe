"""Inputs of the mesh-smoothing tests: tests/simplify_inputs.py's box and sphere, welded, clean and with the noise of the quality
bars, the analytic distances those bars are judged by, and the small hand-made meshes of the kernel tests."""
import itertools

import numpy as np

import simplify_inputs as I
import smooth_ref as R

VOXEL = 1.0
NOISE_SIGMA = 0.1                                   # voxels
DEFAULTS = dict(sigma_s=1.0, sigma_r=0.35, normal_iters=10, vertex_iters=10, max_move=1.0)
OTHER = dict(sigma_s=2.0, sigma_r=0.5, normal_iters=3, vertex_iters=4, max_move=0.25)     # the clamp binds
# what the restatement gives at the defaults (next to the bars of tests/test_smooth_host.py)
EXPECT = dict(box_flat=(0.0998, 0.0313), box_edge=(0.1294, 0.1273), sphere=(0.1024, 0.0334), clean_p99=0.234, max_move=0.53)

_cache = {}


def meshes():
    """-> dict: box, sphere (welded: xyz, rgb, faces), box_noisy, sphere_noisy (welded too).  The noise is one generator's draws, the box first."""
    if not _cache:
        rng = np.random.default_rng(0)
        for name, raw in (("box", I.box_mesh()), ("sphere", I.sphere_mesh())):
            xyz, rgb, faces = R.weld(*raw)
            _cache[name] = (xyz, rgb, faces)
            # welded again: the noise changes the lexicographic order of the vertices, and smooth() returns the welded order
            noisy, inv = np.unique(xyz + rng.normal(0, NOISE_SIGMA, xyz.shape), axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            assert len(noisy) == len(xyz)
            col, clean = np.empty_like(rgb), np.empty_like(xyz)
            col[inv], clean[inv] = rgb, xyz
            _cache[name + "_noisy"] = (noisy, col, inv[faces])
            _cache[name + "_noisy_clean"] = clean
    return _cache


def clean_of(name):
    """The clean positions of a noisy mesh's vertices, in that mesh's vertex order."""
    return meshes()[name + "_clean"]


def box_distance(x):
    lo, hi = np.asarray(I.BOX[0]), np.asarray(I.BOX[1])
    q = np.maximum(lo - x, x - hi)
    return np.abs(np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0))


def sphere_distance(x):
    return np.abs(np.linalg.norm(x - np.asarray(I.SPHERE_CENTRE), axis=1) - I.SPHERE_RADIUS)


def box_edge_distance(x):
    """Distance to the nearest of the box's twelve edges."""
    lo, hi = np.asarray(I.BOX[0]), np.asarray(I.BOX[1])
    best = np.full(len(x), np.inf)
    for ax in range(3):
        o1, o2 = [a for a in range(3) if a != ax]
        along = np.maximum(np.maximum(lo[ax] - x[:, ax], x[:, ax] - hi[ax]), 0.0)
        for c1, c2 in itertools.product((lo, hi), repeat=2):
            best = np.minimum(best, np.sqrt(along ** 2 + (x[:, o1] - c1[o1]) ** 2 + (x[:, o2] - c2[o2]) ** 2))
    return best


def rms(d):
    return float(np.sqrt((d ** 2).mean()))


def cut_open(xyz, rgb, faces, lo=(32.0, 32.0, 32.0), hi=(64.0, 64.0, 64.0)):
    """The mesh without the faces of one brick (every corner inside the brick's box): it gains a boundary."""
    inside = ((xyz >= np.asarray(lo)) & (xyz <= np.asarray(hi))).all(1)
    keep = ~inside[faces].all(1)
    return xyz, rgb, faces[keep]


def colours(n):
    return np.stack([(np.arange(n) * 37 + 10) % 256, (np.arange(n) * 91 + 3) % 256, (np.arange(n) * 13 + 200) % 256], 1).astype(np.uint8)


def hand_mesh():
    """Every coordinate a multiple of 1/8 -> (xyz, rgb, faces).
      a 4 x 3 grid of vertices folded along its second column into a roof: a crease, and a boundary all round;
      a fin (face 12) on the crease edge 1 - 5, which three faces then use;
      a zero-area face (13: three collinear vertices, one of them the grid's corner);
      vertex 15, which no face uses;
      two faces (14, 15) with opposite normals and equal areas, mirror images in the plane z = 11, and a second zero-area face
      (16) that shares one vertex with each and has its centroid on that plane: its own term is zero, the two neighbours'
      terms are equal and opposite, the filtered sum cancels exactly and the normal stays (the fallback)."""
    V = []
    for j in range(3):
        for i in range(4):
            V.append((i * 1.0, j * 1.0, 1.0 - abs(i - 1) * 0.5))           # 0 .. 11: the roof, ridge at i = 1
    V += [(1.0, 0.5, 2.0),                                                 # 12: the fin's tip
          (4.0, 0.0, -0.5), (5.0, 0.0, -1.0),                              # 13, 14: on one line with vertex 3 = (3, 0, 0)
          (7.5, 7.5, 7.5)]                                                 # 15: no face
    F = []
    for j in range(2):
        for i in range(3):
            a, b, c, d = j * 4 + i, j * 4 + i + 1, (j + 1) * 4 + i, (j + 1) * 4 + i + 1
            F += [(a, b, d), (a, d, c)]                                    # 0 .. 11
    F += [(1, 5, 12),                                                      # 12: the fin
          (3, 13, 14)]                                                     # 13: zero area
    # the cancelling pair, away from the roof: faces 14 and 15 in the planes z = 10 (normal +z) and z = 12 (normal -z), mirror
    # images in z = 11; face 16 is collinear (zero area) and touches one vertex of each, its centroid on the mirror plane
    V += [(10.0, 10.0, 10.0), (11.0, 10.0, 10.0), (10.0, 11.0, 10.0),      # 16, 17, 18
          (10.0, 10.0, 12.0), (11.0, 10.0, 12.0), (10.0, 11.0, 12.0),      # 19, 20, 21
          (10.0, 10.0, 11.0)]                                              # 22: between 16 and 19
    F += [(16, 17, 18), (19, 21, 20),                                      # 14, 15
          (16, 22, 19)]                                                    # 16: zero area, a neighbour of both
    xyz = np.array(V, np.float64)
    return xyz, colours(len(V)), np.array(F, np.int64)


def strip(nf):
    """A wavy strip of nf faces along x (nf + 2 vertices)."""
    i = np.arange(nf + 2)
    xyz = np.stack([(i // 2) * 0.5, (i % 2) * 1.0, 0.125 * ((i // 2) % 3) + 0.0625 * (i % 2) * ((i // 4) % 2)], 1).astype(np.float64)
    faces = np.array([(k, k + 1, k + 2) if k % 2 == 0 else (k + 1, k, k + 2) for k in range(nf)], np.int64)
    return xyz, colours(len(xyz)), faces


EDGE_TILE_FACES = (85, 86, 171)               # 255, 258 and 513 edges: a partial tile of 256 lanes, a second tile, a third


def renamed_strip_faces(nf):
    """strip(nf)'s faces with its last two vertices, nf and nf + 1, renamed to numbers with bit 31 set -> (faces int64 [nf, 3], the
    same as the int32 bits a kernel reads).  The edge between the two has bit 31 in both halves of its key."""
    faces = strip(nf)[2]
    big = np.where(faces == nf, 0x80000005, np.where(faces == nf + 1, 0xFFFFFFF9, faces)).astype(np.int64)
    return big, big.astype(np.uint32).view(np.int32)


def fan(nf):
    """nf faces around one apex (vertex 0), closed, on a wavy rim: every face neighbours every other through the apex."""
    t = 2 * np.pi * np.arange(nf) / nf
    rim = np.stack([np.cos(t), np.sin(t), 0.1 * np.cos(5 * t) - 0.5], 1)
    xyz = np.concatenate([np.zeros((1, 3)), rim])
    faces = np.array([(0, 1 + k, 1 + (k + 1) % nf) for k in range(nf)], np.int64)
    return xyz, colours(len(xyz)), faces
