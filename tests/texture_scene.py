"""An analytic triangle mesh of ada_mvs_amd/fusion_synth.py's scene for the texture tests: the terrain triangulated at 1 m and
every box as its roof and four walls, each planar face a grid of its own vertices, counter-clockwise about the outward normal.
Every face is tagged TERRAIN, ROOF or WALL (tests/ortho_scene.py's codes, which its images carry in B).  Grid steps are
dyadic, so the scene shifted by whole metres has bit-identical differences X - C."""
import numpy as np

from ada_mvs_amd import fusion_synth
from ortho_scene import ROOF, TERRAIN, WALL

EXTENT = (-160.0, 160.0, -130.0, 130.0)       # terrain x0, x1, y0, y1


def _grid(origin, e1, e2, n1, n2):
    """Vertices [(n1+1)(n2+1), 3] and faces [2 n1 n2, 3] of the patch origin + s e1 + t e2 (s, t in [0, 1]); normal e1 x e2."""
    s = np.arange(n1 + 1) / n1
    t = np.arange(n2 + 1) / n2
    S, T = np.meshgrid(s, t)                           # [n2+1, n1+1]
    P = np.asarray(origin, np.float64) + S.reshape(-1, 1) * np.asarray(e1, np.float64) + T.reshape(-1, 1) * np.asarray(e2, np.float64)
    i, j = np.meshgrid(np.arange(n1), np.arange(n2))
    a = (j * (n1 + 1) + i).reshape(-1)
    b, c, d = a + 1, a + n1 + 2, a + n1 + 1
    return P, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])


def _steps(length, target=2.0):
    """A power of two of subdivisions giving steps of at most `target` metres."""
    n = 1
    while length / n > target:
        n *= 2
    return n


def mesh(offset=(0.0, 0.0, 0.0), terrain_step=1.0):
    """-> (xyz [nv, 3] float64, rgb [nv, 3] uint8, faces [nf, 3] uint32, cls [nf] (TERRAIN / ROOF / WALL), box [nf] (box index of
    a roof or wall face, -1 on the terrain))."""
    x0, x1, y0, y1 = EXTENT
    parts = [(_grid((x0, y0, 0.0), (x1 - x0, 0, 0), (0, y1 - y0, 0), int((x1 - x0) / terrain_step), int((y1 - y0) / terrain_step)),
              TERRAIN, -1)]
    for k, (bx0, bx1, by0, by1, h) in enumerate(fusion_synth.BOXES):
        lx, ly = bx1 - bx0, by1 - by0
        nx, ny, nh = _steps(lx), _steps(ly), _steps(h)
        parts.append((_grid((bx0, by0, h), (lx, 0, 0), (0, ly, 0), nx, ny), ROOF, k))
        parts.append((_grid((bx0, by1, 0.0), (0, -ly, 0), (0, 0, h), ny, nh), WALL, k))       # x0 wall, normal -x
        parts.append((_grid((bx1, by0, 0.0), (0, ly, 0), (0, 0, h), ny, nh), WALL, k))        # x1 wall, normal +x
        parts.append((_grid((bx0, by0, 0.0), (lx, 0, 0), (0, 0, h), nx, nh), WALL, k))        # y0 wall, normal -y
        parts.append((_grid((bx1, by1, 0.0), (-lx, 0, 0), (0, 0, h), nx, nh), WALL, k))       # y1 wall, normal +y
    xyz, faces, cls, box = [], [], [], []
    base = 0
    for (P, F), c, k in parts:
        xyz.append(P)
        faces.append(F + base)
        cls.append(np.full(len(F), c))
        box.append(np.full(len(F), k))
        base += len(P)
    xyz = np.concatenate(xyz) + np.asarray(offset, np.float64)
    rgb = np.stack([np.full(len(xyz), 50), np.full(len(xyz), 100), np.full(len(xyz), 150)], 1).astype(np.uint8)
    rgb[:, 0] = (np.arange(len(xyz)) * 7) % 256
    return xyz, rgb, np.concatenate(faces).astype(np.uint32), np.concatenate(cls), np.concatenate(box)


def normals(xyz, faces):
    """Unnormalised right-hand normals [nf, 3] (fp64)."""
    A, B, C = (xyz[faces[:, k].astype(np.int64)] for k in range(3))
    return np.cross(B - A, C - A)


def under_a_box(xyz, faces, offset=(0.0, 0.0, 0.0)):
    """Terrain faces wholly under a box (every vertex strictly inside a box's footprint)."""
    P = xyz[faces.astype(np.int64)] - np.asarray(offset, np.float64)
    out = np.zeros(len(faces), bool)
    for x0, x1, y0, y1, _ in fusion_synth.BOXES:
        inside = (P[..., 0] > x0) & (P[..., 0] < x1) & (P[..., 1] > y0) & (P[..., 1] < y1) & (P[..., 2] == 0.0)
        out |= inside.all(1)
    return out
