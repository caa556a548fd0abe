"""numpy restatement of include/adamvs_hip.h "Mesh cleaning": the eight steps, written from the header's rule and sharing no code
with csrc/mesh_clean.hip.  Where the GPU iterates (label rounds, pointer doubling) this walks: components by union-find over the
faces, loops by following the successor from every boundary half-edge until it returns or meets an undefined successor.
Besides the result it returns every intermediate the GPU tests compare."""
import numpy as np

import smooth_ref as SR

CHUNK = 1024                                   # ADAMVS_CLEAN_CHUNK


def components(faces, nv):
    """Step 3 -> labels [nv]: the smallest vertex of each vertex's component (itself where no face uses it)."""
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in faces.tolist():
        r = sorted((find(a), find(b), find(c)))
        parent[r[1]] = r[0]
        parent[r[2]] = r[0]
    return np.array([find(v) for v in range(nv)], np.int64)


def component_areas(area, face_label):
    """-> (labels ascending, face counts, areas by the header's pieces: chunks of CHUNK positions of the stably sorted faces)."""
    order = np.argsort(face_label, kind="stable")
    labs, start, count = np.unique(face_label[order], return_index=True, return_counts=True)
    out = np.zeros(len(labs))
    for c, (s, n) in enumerate(zip(start.tolist(), count.tolist())):
        cuts = [s] + list(range((s // CHUNK + 1) * CHUNK, s + n, CHUNK)) + [s + n]
        total = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            piece = float(np.cumsum(area[order[a:b]])[-1])          # cumsum adds one by one, in order
            total = piece if total is None else total + piece
        out[c] = total
    return labs, count, out


def half_edges(sf):
    """-> (tail [3 ns], head [3 ns]) of h = 3 s + k."""
    return sf.reshape(-1), sf[:, [1, 2, 0]].reshape(-1)


def boundary(sf, nv):
    """Step 5 -> (bnd [3 ns] bool, out_count, in_count [nv], succ [3 ns] (-1 undefined))."""
    tail, head = half_edges(sf)
    key = (np.minimum(tail, head).astype(np.int64) << 32) | np.maximum(tail, head).astype(np.int64)
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    bnd = cnt[inv.reshape(-1)] == 1
    out_count = np.bincount(tail[bnd], minlength=nv)
    in_count = np.bincount(head[bnd], minlength=nv)
    simple = (out_count == 1) & (in_count == 1)
    leaving = np.full(nv, -1, np.int64)
    hb = np.nonzero(bnd)[0]
    leaving[tail[hb][::-1]] = hb[::-1]                               # the smallest where several leave (unused then)
    succ = np.where(bnd & simple[head], leaving[head], -1)
    return bnd, out_count, in_count, succ


def loops(bnd, succ):
    """Step 6 -> loop [3 ns]: the label (smallest h) of the loop each half-edge is in, -1 where in none; and {label: length}."""
    loop = np.full(len(bnd), -1, np.int64)
    seen = np.zeros(len(bnd), bool)
    length = {}
    for h in np.nonzero(bnd)[0].tolist():
        if seen[h]:
            continue
        chain, g = [h], int(succ[h])
        seen[h] = True
        while g >= 0 and g != h and not seen[g]:                     # a chain walked before is open: so is one that runs into it
            seen[g] = True
            chain.append(g)
            g = int(succ[g])
        if g == h:
            loop[chain] = min(chain)
            length[min(chain)] = len(chain)
    return loop, length


def clean(xyz, rgb, faces, min_faces=100, min_area=None, max_hole_edges=32, origin=None):
    """-> dict: xyz, rgb, faces (the cleaned mesh); welded (xyz, rgb, faces after the degenerate ones left); labels, face_labels,
    component_labels / _faces / _area, kept, surviving, boundary, successor, loop, closed, lengths, info."""
    xyz, rgb = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(rgb, np.uint8).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    info = dict(vertices_in=0, faces_in=len(faces), faces_degenerate=0, components=0, components_kept=0, faces_removed=0, area_removed=0.0,
                largest_removed_faces=0, boundary_edges_in=0, loops=0, loops_closed=0, loops_too_long=0, edges_left_open=0,
                nonsimple_vertices=0, fill_vertices=0, fill_faces=0, vertices=0, faces=0)
    empty = dict(xyz=np.zeros((0, 3)), rgb=np.zeros((0, 3), np.uint8), faces=np.zeros((0, 3), np.int64), info=info)
    if len(xyz) == 0:
        return empty
    xyz, rgb, faces = SR.weld(xyz, rgb, faces)
    nv = len(xyz)
    O = np.asarray(origin, np.float64) if origin is not None else xyz.min(0)
    degenerate = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 2] == faces[:, 0])
    faces = faces[~degenerate]
    info.update(vertices_in=nv, faces_degenerate=int(degenerate.sum()))
    empty.update(welded=(xyz, rgb, faces), degenerate=degenerate)
    if len(faces) == 0:
        return empty
    p = xyz - O
    _, area, _ = SR.face_records(p, faces)
    labels = components(faces, nv)
    face_labels = labels[faces[:, 0]]
    comp_labels, comp_faces, comp_area = component_areas(area, face_labels)
    comp_kept = comp_faces >= min_faces
    if min_area is not None:
        comp_kept &= comp_area >= min_area
    kept = comp_kept[np.searchsorted(comp_labels, face_labels)]
    info.update(components=len(comp_labels), components_kept=int(comp_kept.sum()), faces_removed=int(comp_faces[~comp_kept].sum()),
                area_removed=float(np.sum(comp_area[~comp_kept])), largest_removed_faces=int(comp_faces[~comp_kept].max()) if (~comp_kept).any() else 0)
    sf = faces[kept]
    res = dict(welded=(xyz, rgb, faces), degenerate=degenerate, origin=O, labels=labels, face_labels=face_labels, component_labels=comp_labels,
               component_faces=comp_faces, component_area=comp_area, kept=kept, surviving=sf, area=area)
    if len(sf) == 0:
        empty.update(res)
        return empty
    bnd, out_count, in_count, succ = boundary(sf, nv)
    loop, length = loops(bnd, succ)
    M = int(max_hole_edges)
    closed_labels = sorted(l for l, n in length.items() if 3 <= n <= M)
    closed = np.isin(loop, closed_labels) & (loop >= 0)
    tail, head = half_edges(sf)
    # step 7: the centres, each axis summed one by one in ascending h
    centres, colours = [], []
    for l in closed_labels:
        hs = np.nonzero(loop == l)[0]
        s = np.zeros(3)
        c = np.zeros(3, np.int64)
        for h in hs.tolist():
            s = s + p[tail[h]]
            c = c + rgb[tail[h]].astype(np.int64)
        centres.append(O + s / float(len(hs)))
        colours.append(np.floor(c / float(len(hs)) + 0.5).astype(np.uint8))
    # step 8
    used = np.zeros(nv, bool)
    used[sf.reshape(-1)] = True
    new_index = np.cumsum(used) - 1
    nvs = int(used.sum())
    fill_h = np.nonzero(closed)[0]
    rank = {l: i for i, l in enumerate(closed_labels)}
    fans = np.array([(new_index[head[h]], new_index[tail[h]], nvs + rank[int(loop[h])]) for h in fill_h.tolist()], np.int64).reshape(-1, 3)
    out_xyz = np.concatenate([xyz[used], np.array(centres, np.float64).reshape(-1, 3)])
    out_rgb = np.concatenate([rgb[used], np.array(colours, np.uint8).reshape(-1, 3)])
    out_faces = np.concatenate([new_index[sf], fans])
    if len(fill_h):                                                  # the weld of the output: the earliest of equal rows gives the colour
        u, first, inv = np.unique(out_xyz, axis=0, return_index=True, return_inverse=True)
        out_xyz, out_rgb, out_faces = u, out_rgb[first], inv.reshape(-1)[out_faces]
    on = (out_count + in_count) > 0
    info.update(boundary_edges_in=int(bnd.sum()), loops=len(length), loops_closed=len(closed_labels),
                loops_too_long=sum(1 for n in length.values() if n > M), edges_left_open=int(bnd.sum()) - len(fill_h),
                nonsimple_vertices=int((on & ~((out_count == 1) & (in_count == 1))).sum()), fill_vertices=len(closed_labels),
                fill_faces=len(fill_h), vertices=len(out_xyz), faces=len(out_faces))
    res.update(xyz=out_xyz, rgb=out_rgb, faces=out_faces, boundary=bnd, successor=succ, loop=loop, closed=closed, lengths=length,
               centres=np.array(centres, np.float64).reshape(-1, 3), colours=np.array(colours, np.uint8).reshape(-1, 3), info=info)
    return res


# ---- facts about a mesh the tests hold ---------------------------------------------------------------------------------------------
def edge_facts(faces):
    """-> (edges used once, directed edges used more than once, Euler characteristic V - E + F over the vertices in use)."""
    tail, head = half_edges(np.asarray(faces, np.int64))
    und = np.unique(np.stack([np.minimum(tail, head), np.maximum(tail, head)], 1), axis=0, return_counts=True)
    _, dcnt = np.unique(np.stack([tail, head], 1), axis=0, return_counts=True)
    V = len(np.unique(faces))
    return int((und[1] == 1).sum()), int((dcnt > 1).sum()), V - len(und[0]) + len(faces)


def signed_volume(xyz, faces):
    a, b, c = xyz[faces[:, 0]], xyz[faces[:, 1]], xyz[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
