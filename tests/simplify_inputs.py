"""Inputs of the mesh-simplification tests, built on the CPU from tests/mesh_ref.py: the sphere and the box over eight bricks, and
a hand-made mesh that exercises every rule of include/adamvs_hip.h "Mesh simplification" once."""
import itertools

import numpy as np

import mesh_ref as M

B = 32
SPHERE_CENTRE = (32.37, 31.81, 32.23)          # the centre of test_mesh_gpu.py's sphere
SPHERE_RADIUS = 10.0
BOX = ((20.3, 22.6, 24.2), (44.1, 40.7, 38.9))
LATTICE_ORIGIN = (-0.5, -0.25, -0.125)
CELLS = (2.0, 3.0, 4.0)
# what the restatement gives (and the numpy prototype of the rule gave) per cell size
SPHERE_EXPECT = {2.0: dict(cells=413, faces_out=825, faces_duplicate=25, fallbacks=4, dist=0.1),
                 3.0: dict(cells=201, faces_out=399, faces_duplicate=13, fallbacks=4, dist=0.2),
                 4.0: dict(cells=121, faces_out=237, faces_duplicate=11, fallbacks=1, dist=0.3)}
BOX_EXPECT = {2.0: dict(faces_out=1020, rank_hist=(379, 120, 13)), 3.0: dict(faces_out=456, rank_hist=(120, 92, 18)),
              4.0: dict(faces_out=252, rank_hist=(65, 51, 12))}


def box_volume(lo, hi, mu=4.0, nb=2):
    """The analytic tsdf of the box [lo, hi] (voxel units, fp32) over nb^3 bricks, as mesh_ref.sphere_volume lays a volume out."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    out = {}
    for b in itertools.product(range(nb), repeat=3):
        g = M.sample_grid(B, b).astype(np.float64)
        q = np.maximum(lo - g, g - hi)
        sdf = np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)
        t = np.clip(sdf / mu, -1.0, 1.0).astype(np.float32)
        col = (np.clip(g[:, 0] * 3, 0, 255).astype(np.uint32) | (np.clip(g[:, 1] * 3, 0, 255).astype(np.uint32) << 8)
               | (np.uint32(200) << 16) | (np.uint32(255) << 24))
        out[b] = (t, np.ones(len(g), np.uint16), col.astype(np.uint32))
    return out


def mesh_of(vol):
    """The unwelded mesh of a volume {brick: (tsdf, weight, rgba)}: the bricks' meshes concatenated -> (xyz, rgb, faces int64)."""
    xs, cs, fs, base = [], [], [], 0
    for b in sorted(vol):
        t, w, c = vol[b]
        r = M.extract((0.0, 0.0, 0.0), 1.0, B, b, t, w, c, 1, base)
        xs.append(r["xyz"]), cs.append(r["rgb"]), fs.append(r["faces"].astype(np.int64))
        base += len(r["xyz"])
    return np.concatenate(xs), np.concatenate(cs), np.concatenate(fs)


def sphere_mesh():
    return mesh_of(M.sphere_volume(B, SPHERE_CENTRE, SPHERE_RADIUS, 4.0))


def box_mesh():
    return mesh_of(box_volume(*BOX))


def hand_mesh():
    """-> (xyz, rgb, faces, cell = 1, lattice origin 0).  Every coordinate is a multiple of 1/8, so every sum of the quadrics is exact
    in fp64 in any order; every face but one lies in an axis-aligned plane, so those cells' A is diagonal and needs no rotation;
    the cells of the one tilted face fall back or have a single member on the plane (g = 0).  The GPU therefore has to match the
    restatement bit for bit, positions included.
      a corner of the planes x = 1.5, y = 1.5, z = 1.5 in cell (1, 1, 1): rank 3; creases in (0, 1, 1), (1, 0, 1), (1, 1, 0): rank 2;
      flat cells, e.g. (0, 0, 1): rank 1; cell (5, 5, 5) between z = 5.25 and a plane that meets it at x = 1.5: fallback."""
    V = [(1.5, 1.5, 1.5),                                              # 0: the corner
         (0.5, 1.25, 1.5), (1.25, 0.5, 1.5),                           # 1, 2: plane z = 1.5
         (1.5, 0.5, 1.25), (1.5, 1.25, 0.5),                           # 3, 4: plane x = 1.5
         (1.25, 1.5, 0.5), (0.5, 1.5, 1.25),                           # 5, 6: plane y = 1.5
         (0.5, 0.5, 1.5),                                              # 7: flat cell (0, 0, 1)
         (0.375, 1.375, 1.5), (1.375, 0.375, 1.5), (0.375, 0.375, 1.5),  # 8, 9, 10: the folded sheet over 1, 2, 7
         (3.125, 0.125, 1.5), (3.25, 0.125, 1.5), (3.125, 0.25, 1.5),  # 11, 12, 13: a face inside cell (3, 0, 1), which goes unused
         (0.625, 0.625, 1.5), (0.75, 0.625, 1.5), (1.0, 0.25, 1.5),    # 14, 15 in (0, 0, 1); 16 exactly on the boundary x = 1
         (0.875, 0.875, 1.875),                                        # 17: no face refers to it
         (1.5, 0.5, 0.5), (0.5, 1.5, 0.5),                             # 18, 19: the planes x = 1.5 and y = 1.5 further down
         (5.5, 5.5, 5.25), (6.5, 5.5, 5.25), (5.5, 6.5, 5.25),         # 20, 21, 22: plane z = 5.25
         (5.5, 5.5, 5.75), (4.5, 5.5, 5.625), (5.5, 4.5, 5.75)]        # 23, 24, 25: z = 5.75 + (x - 5.5) / 8
    F = [(0, 1, 2), (0, 3, 4), (0, 5, 6),                              # the corner's three faces
         (1, 7, 2),                                                    # flat, three cells
         (8, 9, 10),                                                   # the same three cells, opposite orientation: a duplicate
         (11, 12, 13),                                                 # wholly inside one cell
         (14, 15, 16),                                                 # two corners in one cell
         (3, 18, 4), (5, 19, 6),                                       # more of the planes x = 1.5 and y = 1.5
         (20, 21, 22), (23, 24, 25),                                   # the fallback cell's two planes
         (16, 2, 9)]                                                   # 16 (on the boundary) and 2, 9 share cell (1, 0, 1): collapses
    xyz = np.array(V, np.float64)
    rgb = np.stack([(np.arange(len(V)) * 37 + 10) % 256, (np.arange(len(V)) * 91 + 3) % 256, (np.arange(len(V)) * 13 + 200) % 256], 1).astype(np.uint8)
    return xyz, rgb, np.array(F, np.int64), 1.0, (0.0, 0.0, 0.0)
