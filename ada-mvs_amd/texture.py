"""Mesh texturing: the TSDF mesh textured from the source images on the GPU.

    python texture_whu.py --data_folder D --output_folder O [--mesh O/mesh.ply] [--out O/mesh_textured]
                          [--occlusion_tol M] [--border_px 2] [--pad 2] [--page 8192]
                          [--seam_level [--seam_lambda 0.1] [--seam_tol 1e-4] [--seam_iters 1000]]

The step after mesh_whu.py.  The views are predict's images `<vid>/<name>.jpg` with the `<name>.txt` intrinsics and the fp64
poses of image_info.txt (ortho.load_views), every view with both files, in ascending image id; views whose image the mesh's
bounding box misses are culled (mesh.cull_views).  Per view, csrc/texture.hip projects the vertices, renders the mesh into a
depth buffer with the orthophoto's rasteriser and scores every face it sees front-on and unoccluded by its projected area; each
face keeps the best view (a tie keeps the earlier one).  Faces that share an edge and a view form a chart (connected
components on the GPU, root = the smallest face); each chart's pixel box in its view is shelf-packed into square pages of side
P here, copied texel for texel into the atlas on the GPU, and the faces get texture coordinates into it.  Faces no view sees
get one palette texel with the mean of their vertex colours (include/adamvs_hip.h "Mesh texturing" states every operation).

With --seam_level the chart boundaries are levelled radiometrically afterwards (csrc/texture_level.hip): one additive
correction per (vertex, chart) node and channel from one global least-squares solve (the views' colours at a vertex agree
after correction; the correction varies smoothly inside a chart; the minimum-norm solution, by unpreconditioned conjugate
gradients in fp64), interpolated over every chart's texels and added to the atlas.  Vertices are identified by index, so a
mesh written without mesh_whu.py --weld is levelled within each brick only.  Off by default: every output byte is then
what it is without the option.

Written: `<out>.ply` (binary little-endian: the mesh's vertices unchanged, faces with `texcoord` (6 floats, origin bottom-left)
and `texnumber` (the page), one `comment TextureFile` per page, the layout OpenMVS and MeshLab read), `<out>_tex_NNNN.png`
(RGB pages) and `<out>.json`.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

from . import fusion
from .mesh import cull_views, read_mesh_ply

MIN_PAGE, MAX_PAGE = 1024, 16384            # ADAMVS_TEXTURE_MIN_PAGE / ADAMVS_TEXTURE_MAX_PAGE
MAX_FACES = (1 << 31) - 1                   # ADAMVS_TEXTURE_MAX_FACES
CULL_MARGIN_PX = 2.0
TEX_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<u4", (3,)), ("nt", "u1"), ("tc", "<f4", (6,)), ("tex", "<i4")])
PHASES = ("project_zbuf", "score", "components", "boxes", "fill_coords")
LEVEL_PHASES = ("level_graph", "level_solve", "level_apply")         # added to device_ms by seam_level=True only
LEVEL_BAND = 2                              # ADAMVS_TEXTURE_LEVEL_BAND
LEVEL_MAX_NODES = 1 << 30                   # ADAMVS_TEXTURE_LEVEL_MAX_NODES
SEAM_LAMBDA, SEAM_TOL, SEAM_ITERS = 0.1, 1e-4, 1000


# ---- options --------------------------------------------------------------------------------------------------------------
def check_page(page):
    """P: a power of two 1024 .. 16384."""
    if isinstance(page, bool) or not isinstance(page, (int, np.integer)) or not MIN_PAGE <= page <= MAX_PAGE or page & (page - 1):
        raise ValueError("page %r: a power of two %d .. %d" % (page, MIN_PAGE, MAX_PAGE))
    return int(page)


def check_options(occlusion_tol, border_px, pad):
    for name, v in (("occlusion_tol", occlusion_tol), ("border_px", border_px)):
        f = float(v)
        if not (math.isfinite(f) and f >= 0.0):
            raise ValueError("%s=%r must be finite and >= 0" % (name, v))
    if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or pad < 0:
        raise ValueError("pad=%r: an integer >= 0" % (pad,))


def check_seam_options(seam_lambda, seam_tol, seam_iters):
    lam, tol = float(seam_lambda), float(seam_tol)
    if not (math.isfinite(lam) and lam > 0.0):
        raise ValueError("seam_lambda=%r must be finite and > 0" % (seam_lambda,))
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError("seam_tol=%r must be finite and >= 0" % (seam_tol,))
    if isinstance(seam_iters, bool) or not isinstance(seam_iters, (int, np.integer)) or seam_iters < 0:
        raise ValueError("seam_iters=%r: an integer >= 0" % (seam_iters,))


def default_tol(mesh_path):
    """Twice the voxel recorded in `<mesh>.json`; None if that file is absent."""
    jp = mesh_path + ".json"
    if not os.path.exists(jp):
        return None
    with open(jp) as f:
        return 2.0 * float(json.load(f)["voxel"])


def check_mesh(nv, faces):
    """Refuse more than 2^31 - 1 faces and a vertex index out of range (faces: numpy [m, 3] uint32 or a device tensor)."""
    nf = int(faces.shape[0])
    if nf > MAX_FACES:
        raise ValueError("mesh: %d faces (at most %d)" % (nf, MAX_FACES))
    if nf:
        top = int(faces.max()) if isinstance(faces, np.ndarray) else int((faces.to(dtype=faces.dtype).long() & 0xFFFFFFFF).max())
        if top >= nv:
            raise ValueError("mesh: vertex index %d out of range (%d vertices)" % (top, nv))


# ---- packing (host) -----------------------------------------------------------------------------------------------------------
def palette_block(n_untextured, P):
    """(w, h) of the palette block for n untextured faces: min(n, P) by ceil(n / P); None if n == 0."""
    if n_untextured == 0:
        return None
    return min(n_untextured, P), -(-n_untextured // P)


def pack(w, h, P):
    """Shelf-pack items of size w x h (int arrays, in item order) into pages of side P -> (ox, oy, page, npages).  Items are
    sorted by h descending, w descending, index; a new shelf starts where x + w > P, a new page where y + h > P; a shelf is
    as tall as its first item.  The loop runs over shelves."""
    w, h = np.asarray(w, np.int64), np.asarray(h, np.int64)
    n = w.size
    ox, oy, page = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    if n == 0:
        return ox, oy, page, 0
    if (w < 1).any() or (h < 1).any() or (w > P).any() or (h > P).any():
        raise ValueError("pack: an item of size outside 1 .. %d" % P)
    order = np.lexsort((np.arange(n), -w, -h))
    ws, hs = w[order], h[order]
    cw = np.concatenate([[0], np.cumsum(ws)])             # exclusive prefix of the widths in packing order
    i, y, pg = 0, 0, 0
    while i < n:
        j = int(np.searchsorted(cw, cw[i] + P, side="right")) - 1     # items i .. j-1 fit on a shelf that starts with item i
        if y + hs[i] > P:
            pg, y = pg + 1, 0
        sel = order[i:j]
        ox[sel] = cw[i:j] - cw[i]
        oy[sel] = y
        page[sel] = pg
        y += int(hs[i])
        i = j
    return ox, oy, page, pg + 1


def chart_boxes(box, view, Ws, Hs, pad):
    """Raw boxes (min floor u, min floor v, max floor u, max floor v) -> (x0, y0, x1, y1) padded by pad and clamped to the view."""
    box = np.asarray(box, np.int64).reshape(-1, 4)
    W, H = np.asarray(Ws, np.int64)[view], np.asarray(Hs, np.int64)[view]
    x0 = np.maximum(box[:, 0] - pad, 0)
    y0 = np.maximum(box[:, 1] - pad, 0)
    x1 = np.minimum(box[:, 2] + 1 + pad, W - 1)
    y1 = np.minimum(box[:, 3] + 1 + pad, H - 1)
    return x0, y0, x1, y1


def tex_coords(u, v, x0, y0, ox, oy, P):
    """The texture-coordinate rule in fp32, left to right: s = (ox + (u - x0) + 1/2) / P, t = 1 - (oy + (v - y0) + 1/2) / P."""
    f = np.float32
    u, v = np.asarray(u, f), np.asarray(v, f)
    s = (np.asarray(ox, f) + (u - np.asarray(x0, f)) + f(0.5)) / f(P)
    t = f(1.0) - (np.asarray(oy, f) + (v - np.asarray(y0, f)) + f(0.5)) / f(P)
    return s.astype(f), t.astype(f)


# ---- the textured PLY -------------------------------------------------------------------------------------------------------
def texture_names(out, npages):
    base = os.path.basename(out)
    return ["%s_tex_%04d.png" % (base, k) for k in range(npages)]


def textured_ply_header(nv, nf, tex_files):
    return ("ply\nformat binary_little_endian 1.0\n" + "".join("comment TextureFile %s\n" % t for t in tex_files) +
            "element vertex %d\nproperty double x\nproperty double y\nproperty double z\nproperty uchar red\nproperty uchar green\n"
            "property uchar blue\nelement face %d\nproperty list uchar uint vertex_indices\nproperty list uchar float texcoord\n"
            "property int texnumber\nend_header\n" % (nv, nf)).encode("ascii")


def write_textured_ply(path, verts, faces, tc, texnum, tex_files):
    """verts: structured array of fusion.PLY_DTYPE; faces [m, 3] uint32; tc [m, 6] float32; texnum [m] int32."""
    verts = np.ascontiguousarray(verts, fusion.PLY_DTYPE)
    rec = np.empty(len(faces), TEX_FACE_DTYPE)
    rec["n"], rec["v"], rec["nt"], rec["tc"], rec["tex"] = 3, faces, 6, tc, texnum
    with open(path, "wb") as f:
        f.write(textured_ply_header(len(verts), len(rec), tex_files))
        f.write(verts.tobytes())
        f.write(rec.tobytes())


def read_textured_ply(path):
    """-> dict(verts (fusion.PLY_DTYPE), faces [m, 3] uint32, tc [m, 6] float32, texnum [m] int32, tex_files) of write_textured_ply."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    if lines[1] != "format binary_little_endian 1.0":
        raise ValueError("%s: not a binary little-endian PLY" % path)
    tex = [ln.split(None, 2)[2] for ln in lines if ln.startswith("comment TextureFile ")]
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[2])
    verts = np.frombuffer(data, fusion.PLY_DTYPE, count=nv, offset=end)
    rec = np.frombuffer(data, TEX_FACE_DTYPE, count=nf, offset=end + nv * fusion.PLY_DTYPE.itemsize)
    if nf and not ((rec["n"] == 3).all() and (rec["nt"] == 6).all()):
        raise ValueError("%s: a face is not a triangle with six texture coordinates" % path)
    return dict(verts=verts, faces=rec["v"].copy(), tc=rec["tc"].copy(), texnum=rec["tex"].copy(), tex_files=tex)


# ---- seam levelling ---------------------------------------------------------------------------------------------------------
def level_graph(faces, chart, uv, chart_view, nc):
    """The node graph of include/adamvs_hip.h "Seam levelling" from device tensors (faces int32 [nf, 3] holding uint32, chart
    int32 [nf], uv float32 [nf, 6], chart_view int64 [nc]) by torch sorts: -> dict(n, node_vertex, node_chart (int64 [n]),
    corner_node int32 [nf, 3] (-1 on untextured faces), pos float32 [n, 2], node_view int32 [n], smooth int64 [ms, 2], seam bool
    [ms], data int64 [md, 2] (edges as ascending node pairs, sorted), rowptr int32 [n + 1], col int32 [nnz], and the same CSR
    renumbered for the solve: solve_order (solve position -> node), solve_rank (its inverse), solve_rowptr, solve_col)."""
    import torch
    dev = faces.device
    nf = int(faces.shape[0])
    tex = torch.nonzero(chart >= 0).squeeze(1)
    fv = faces[tex].long() & 0xFFFFFFFF
    fc = chart[tex].long()
    nodes, inv = torch.unique((fv * max(nc, 1) + fc[:, None]).reshape(-1), sorted=True, return_inverse=True)
    n = int(nodes.numel())
    if n > LEVEL_MAX_NODES:
        raise ValueError("seam_level: %d nodes (at most %d)" % (n, LEVEL_MAX_NODES))
    node_vertex, node_chart = nodes // max(nc, 1), nodes % max(nc, 1)
    cn = inv.reshape(-1, 3)
    corner_node = torch.full((nf, 3), -1, device=dev, dtype=torch.int32)
    corner_node[tex] = cn.to(torch.int32)
    pos = torch.zeros(n, 2, device=dev, dtype=torch.float32)
    pos[cn.reshape(-1)] = uv[tex].reshape(-1, 2)              # every face of a chart stored the same bits at a vertex
    node_view = chart_view[node_chart].to(torch.int32) if n else torch.zeros(0, device=dev, dtype=torch.int32)
    # smoothness edges, and which of them lie on a seam: the mesh edge carries textured faces of more than one chart
    a, b = cn.reshape(-1), cn.roll(-1, 1).reshape(-1)
    va, vb = fv.reshape(-1), fv.roll(-1, 1).reshape(-1)
    mesh_edge, einv = torch.unique((torch.minimum(va, vb) << 32) | torch.maximum(va, vb), return_inverse=True)
    c3 = fc.repeat_interleave(3)
    cmin = torch.full((mesh_edge.numel(),), 1 << 62, device=dev, dtype=torch.int64).scatter_reduce_(0, einv, c3, "amin")
    cmax = torch.full((mesh_edge.numel(),), -1, device=dev, dtype=torch.int64).scatter_reduce_(0, einv, c3, "amax")
    on_seam = (cmin[einv] != cmax[einv]).long()
    keep = a != b
    sk = torch.unique(((torch.minimum(a, b) * max(n, 1) + torch.maximum(a, b)) * 2 + on_seam)[keep])
    seam, sk = (sk & 1).bool(), sk >> 1
    slo, shi = sk // max(n, 1), sk % max(n, 1)
    # data edges: the nodes of a vertex are consecutive; pair every two of them
    dlo, dhi, d = [], [], 1
    while d < n:
        i = torch.nonzero(node_vertex[:-d] == node_vertex[d:]).squeeze(1)
        if i.numel() == 0:
            break
        dlo.append(i)
        dhi.append(i + d)
        d += 1
    dlo = torch.cat(dlo) if dlo else torch.zeros(0, device=dev, dtype=torch.int64)
    dhi = torch.cat(dhi) if dhi else torch.zeros(0, device=dev, dtype=torch.int64)
    order = torch.argsort(dlo * max(n, 1) + dhi)
    dlo, dhi = dlo[order], dhi[order]
    # CSR with both directions, rows sorted by neighbour; the edge kind rides in the two top bits of the column word
    rows = torch.cat([slo, shi, dlo, dhi])
    cols = torch.cat([shi, slo, dhi, dlo])
    kind = torch.cat([seam.long() << 30, seam.long() << 30, torch.full((2 * dlo.numel(),), 1 << 31, device=dev, dtype=torch.int64)])
    if rows.numel() > (1 << 31) - 1:
        raise ValueError("seam_level: %d graph entries (at most 2^31 - 1)" % rows.numel())
    order = torch.argsort(rows * max(n, 1) + cols)
    word = (cols | kind)[order]
    col = torch.where(word >= (1 << 31), word - (1 << 32), word).to(torch.int32).contiguous()
    rowptr = torch.zeros(n + 1, device=dev, dtype=torch.int64)
    if n:
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    # the same graph numbered for the solve: by chart, then along a Z-order curve of the node's position in the chart's image
    # (quarter pixels), so that a row's neighbours lie near it in memory; ties keep the node order
    q = (pos * 4.0).floor().clamp_(0, 65535).long()
    solve_order = torch.sort((node_chart << 32) | _interleave16(q[:, 0]) | (_interleave16(q[:, 1]) << 1), stable=True).indices
    rank = torch.empty_like(solve_order)
    rank[solve_order] = torch.arange(n, device=dev, dtype=torch.int64)
    srows, scols = rank[rows], rank[cols]
    order = torch.argsort(srows * max(n, 1) + scols)
    word = (scols | kind)[order]
    scol = torch.where(word >= (1 << 31), word - (1 << 32), word).to(torch.int32).contiguous()
    srowptr = torch.zeros(n + 1, device=dev, dtype=torch.int64)
    if n:
        srowptr[1:] = torch.cumsum(torch.bincount(srows, minlength=n), 0)
    return dict(n=n, node_vertex=node_vertex, node_chart=node_chart, corner_node=corner_node, pos=pos, node_view=node_view,
                smooth=torch.stack([slo, shi], 1), seam=seam, data=torch.stack([dlo, dhi], 1), rowptr=rowptr.to(torch.int32).contiguous(),
                col=col, solve_order=solve_order, solve_rank=rank, solve_rowptr=srowptr.to(torch.int32).contiguous(), solve_col=scol)


def _interleave16(x):
    """The 16 low bits of x (int64 tensor) spread to the even bit positions."""
    x = x & 0xFFFF
    x = (x | (x << 8)) & 0x00FF00FF
    x = (x | (x << 4)) & 0x0F0F0F0F
    x = (x | (x << 2)) & 0x33333333
    return (x | (x << 1)) & 0x55555555


def seam_rms(f, g, data):
    """rms over the data edges and the three channels of f_i + g_i - f_j - g_j (fp64 device tensors; 0 without data edges)."""
    if data.shape[0] == 0:
        return 0.0
    v = f.double() + g
    return float((v[data[:, 0]] - v[data[:, 1]]).pow(2).mean().sqrt())


# ---- the GPU texturer -------------------------------------------------------------------------------------------------------
def texture_mesh(xyz, rgb, faces, views, occlusion_tol, border_px=2.0, pad=2, page=8192, device=None, keep_zbufs=False,
                 seam_level=False, seam_lambda=SEAM_LAMBDA, seam_tol=SEAM_TOL, seam_iters=SEAM_ITERS, keep_level=False):
    """xyz [nv, 3] float64, rgb [nv, 3] uint8, faces [nf, 3] uint32 (numpy or device tensors), views as ortho.load_views gives
    them (ascending image id).  -> dict: label (view index or -1), nvis, uv [nf, 6], parent, chart, charts [nc, 8]
    (x0 y0 w h ox oy page view), atlas [pages, P, P, 3] uint8, tc [nf, 6], texnum (host arrays), counts, timings.
    seam_level=True levels the chart boundaries (see the module text) and adds g [nodes, 3] float64, node_vertex, node_chart,
    seam_iterations, seam_residual [3], seam_cap_hit, seam_rms_before, seam_rms_after, nodes and the three LEVEL_PHASES in
    device_ms; keep_level=True also keeps f, pos, corner_node, the edge lists, the owner map before and after the dilation
    (owner_raster, owner, with owner_prefix) and the atlas before levelling (atlas_unlevelled)."""
    import torch
    from . import hip_ops
    from .ortho import view_camera
    if not torch.cuda.is_available():
        raise RuntimeError("texture: needs an MI355X (there is no CPU fallback for the texture kernels)")
    P = check_page(page)
    check_options(occlusion_tol, border_px, pad)
    if seam_level:
        check_seam_options(seam_lambda, seam_tol, seam_iters)
    device = torch.device(device if device is not None else "cuda")
    views = sorted(views, key=lambda v: int(v["iid"]))
    cams = [view_camera(v) for v in views]
    Hs, Ws = [c[3] for c in cams], [c[4] for c in cams]
    side = max(max(Hs, default=0), max(Ws, default=0))
    if side > P:
        raise ValueError("page %d is smaller than the largest image side %d: raise --page" % (P, side))
    t0 = time.time()
    xyz = torch.as_tensor(xyz).to(device, torch.float64).contiguous()
    rgb = torch.as_tensor(rgb).to(device, torch.uint8).contiguous()
    f_np = faces if isinstance(faces, np.ndarray) else None
    faces = torch.from_numpy(np.ascontiguousarray(faces, np.uint32).view(np.int32)) if f_np is not None else faces
    faces = faces.to(device, torch.int32).contiguous().reshape(-1, 3)
    nv, nf = int(xyz.shape[0]), int(faces.shape[0])
    if nv < 1:
        raise ValueError("mesh: no vertex")
    check_mesh(nv, f_np if f_np is not None else faces)
    lo, hi = xyz.min(0).values.cpu().numpy(), xyz.max(0).values.cpu().numpy()
    best = torch.full((nf,), -math.inf, device=device, dtype=torch.float32)
    label = torch.full((nf,), -1, device=device, dtype=torch.int32)
    nvis = torch.zeros(nf, device=device, dtype=torch.int32)
    uv = torch.zeros(nf, 6, device=device, dtype=torch.float32)
    big = torch.empty(1 + nf, device=device, dtype=torch.int32)
    uvz = torch.empty(nv, 4, device=device, dtype=torch.float32)
    phases = PHASES + (LEVEL_PHASES if seam_level else ())
    ev = {k: [] for k in phases}
    used, culled, vdesc, zbufs = [], [], [], {}

    def mark(phase):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ev[phase].append((a, b))
        return b

    for vi, (v, cam) in enumerate(zip(views, cams)):
        vdesc.append(hip_ops.ortho_view(cam[0], cam[1].T, cam[2], v["rgba"]))
        if not cull_views(lo, hi, [cam], CULL_MARGIN_PX):
            culled.append(int(v["iid"]))
            continue
        used.append(int(v["iid"]))
        zbuf = torch.empty(cam[3], cam[4], device=device, dtype=torch.int32)
        e = mark("project_zbuf")
        hip_ops.texture_project(vdesc[vi], xyz, uvz)
        hip_ops.texture_zbuf(vdesc[vi], uvz, faces, zbuf, big)
        e.record()
        e = mark("score")
        hip_ops.texture_score(vdesc[vi], vi, uvz, faces, zbuf, border_px, occlusion_tol, best, label, nvis, uv)
        e.record()
        if keep_zbufs:
            zbufs[int(v["iid"])] = zbuf
    # charts
    e = mark("components")
    keys = hip_ops.texture_edge_keys(faces)
    p1 = torch.sort(label.repeat_interleave(3), stable=True).indices
    keys_sorted, p2 = torch.sort(keys[p1], stable=True)
    entry = p1[p2].contiguous()
    del keys, p1, p2
    parent = torch.arange(nf, device=device, dtype=torch.int32)
    changed = torch.zeros(1, device=device, dtype=torch.int32)
    rounds = 0
    while True:
        hip_ops.texture_components_round(keys_sorted, entry, label, parent, changed)
        rounds += 1
        if int(changed.item()) == 0:
            break
        if rounds > nf + 1:
            raise RuntimeError("texture: connected components did not converge in %d rounds" % rounds)
    e.record()
    del keys_sorted, entry
    e = mark("boxes")
    root_chart, pal, nc, n_untex = hip_ops.texture_rank(label, parent)
    chart, box = hip_ops.texture_boxes(label, parent, root_chart, uv, nc)
    roots = torch.nonzero(root_chart >= 0).squeeze(1)
    cview = label[roots]
    e.record()
    # packing (host)
    t_pack = time.time()
    cview_h = cview.cpu().numpy().astype(np.int64)
    x0, y0, x1, y1 = chart_boxes(box.cpu().numpy(), cview_h, Ws, Hs, pad)
    cw, ch = x1 - x0 + 1, y1 - y0 + 1
    pb = palette_block(n_untex, P)
    if pb is not None and pb[1] > P:
        raise ValueError("texture: %d untextured faces do not fit a palette block of one page %d" % (n_untex, P))
    iw = np.concatenate([cw, [pb[0]] if pb else []]).astype(np.int64)
    ih = np.concatenate([ch, [pb[1]] if pb else []]).astype(np.int64)
    ox, oy, pg, npages = pack(iw, ih, P)
    npages = max(npages, 1)
    charts = np.stack([x0, y0, cw, ch, ox[:nc], oy[:nc], pg[:nc], cview_h], 1).astype(np.int32) if nc else np.zeros((0, 8), np.int32)
    pal_place = (int(ox[nc]), int(oy[nc]), int(pg[nc])) if pb else (0, 0, 0)
    t_pack = time.time() - t_pack
    # atlas
    charts_d = torch.from_numpy(charts).to(device)
    atlas = torch.zeros(npages, P, P, 4, device=device, dtype=torch.uint8)
    e = mark("fill_coords")
    for vi in range(len(views)):
        sel = np.nonzero(cview_h == vi)[0]
        if sel.size == 0:
            continue
        area = cw[sel].astype(np.int64) * ch[sel]
        prefix = np.concatenate([[0], np.cumsum(area)]).astype(np.int64)
        hip_ops.texture_fill(vdesc[vi], charts_d[torch.from_numpy(sel).to(device)], torch.from_numpy(prefix).to(device), int(prefix[-1]), P,
                             atlas)
    tc, texnum = hip_ops.texture_coords(label, chart, pal, uv, charts_d if nc else torch.zeros(1, 8, device=device, dtype=torch.int32),
                                        pal_place, P, faces, rgb, atlas)
    e.record()
    lev = {}
    if seam_level:
        e = mark("level_graph")
        gr = level_graph(faces, chart, uv, torch.from_numpy(cview_h).to(device), nc)
        n = gr["n"]
        f_obs = hip_ops.texture_level_observe(hip_ops.texture_level_view_table(vdesc).to(device), gr["rowptr"], gr["col"], gr["node_view"],
                                              gr["pos"])
        rhs = hip_ops.texture_level_rhs(gr["rowptr"], gr["col"], f_obs)
        e.record()
        e = mark("level_solve")
        g, iters, resid, cap = hip_ops.texture_level_solve(gr["solve_rowptr"], gr["solve_col"], rhs[gr["solve_order"]].contiguous(), seam_lambda,
                                                           seam_tol, seam_iters)
        g = g[gr["solve_rank"]].contiguous()
        e.record()
        if keep_level:
            lev["atlas_unlevelled"] = atlas[..., :3].cpu().numpy()
        e = mark("level_apply")
        prefix = torch.from_numpy(np.concatenate([[0], np.cumsum(cw.astype(np.int64) * ch)]).astype(np.int64)).to(device)
        owner = torch.zeros(0, device=device, dtype=torch.int32)
        if nc:
            owner = hip_ops.texture_level_owner(uv, chart, charts_d, prefix, big)
            if keep_level:
                lev["owner_raster"] = owner.cpu().numpy()
            for _ in range(LEVEL_BAND):
                owner = hip_ops.texture_level_dilate(charts_d, prefix, owner)
            hip_ops.texture_level_apply(uv, gr["corner_node"], g, charts_d, prefix, owner, P, atlas)
        e.record()
        lev.update(g=g.cpu().numpy(), node_vertex=gr["node_vertex"].cpu().numpy(), node_chart=gr["node_chart"].cpu().numpy(), nodes=n,
                   seam_lambda=float(seam_lambda), seam_tol=float(seam_tol), seam_iters=int(seam_iters), seam_iterations=iters,
                   seam_residual=resid, seam_cap_hit=cap, seam_rms_before=seam_rms(f_obs, torch.zeros_like(g), gr["data"]),
                   seam_rms_after=seam_rms(f_obs, g, gr["data"]), seam_edges=int(gr["seam"].sum()), data_edges=int(gr["data"].shape[0]),
                   smooth_edges=int(gr["smooth"].shape[0]), graph_entries=int(gr["col"].numel()))
        if keep_level:
            lev.update(f=f_obs.cpu().numpy(), pos=gr["pos"].cpu().numpy(), corner_node=gr["corner_node"].cpu().numpy(),
                       edges_smooth=gr["smooth"].cpu().numpy(), edges_seam=gr["seam"].cpu().numpy(), edges_data=gr["data"].cpu().numpy(),
                       owner=owner.cpu().numpy(), owner_prefix=prefix.cpu().numpy())
    torch.cuda.synchronize(device)
    ms = {k: sum(a.elapsed_time(b) for a, b in ev[k]) for k in phases}
    res = dict(label=label.cpu().numpy(), nvis=nvis.cpu().numpy(), best=best.cpu().numpy(), uv=uv.cpu().numpy(), parent=parent.cpu().numpy(),
               chart=chart.cpu().numpy(), charts=charts, pal=pal.cpu().numpy(), palette=(pal_place + pb) if pb else None,
               atlas=atlas[..., :3].cpu().numpy(), tc=tc.cpu().numpy(), texnum=texnum.cpu().numpy(), P=P, pad=int(pad),
               border_px=float(border_px), occlusion_tol=float(occlusion_tol), views_used=used, views_culled=culled,
               view_ids=[int(v["iid"]) for v in views], faces=nf, faces_textured=nf - n_untex, faces_untextured=n_untex, charts_count=nc,
               component_rounds=rounds, pages=npages, box_fraction=float((cw.astype(np.int64) * ch).sum()) / (npages * P * P),
               device_ms=ms, device_ms_total=sum(ms.values()), pack_seconds=t_pack, seconds=time.time() - t0)
    res.update(lev)
    if keep_zbufs:
        res["zbufs"] = {k: z.cpu().numpy().view(np.float32).astype(np.float64) for k, z in zbufs.items()}
    return res


# ---- a predict output folder ------------------------------------------------------------------------------------------------
def output_paths(out, npages):
    d = os.path.dirname(out)
    return dict(ply=out + ".ply", json=out + ".json", pages=[os.path.join(d, n) for n in texture_names(out, npages)])


def summary(res):
    keys = ("P", "pad", "border_px", "occlusion_tol", "views_used", "views_culled", "faces", "faces_textured", "faces_untextured",
            "component_rounds", "pages", "box_fraction", "device_ms", "device_ms_total", "pack_seconds", "write_seconds", "seconds",
            "nodes", "seam_lambda", "seam_tol", "seam_iters", "seam_iterations", "seam_residual", "seam_cap_hit", "seam_rms_before",
            "seam_rms_after")
    js = {k: res[k] for k in keys if k in res}
    js["charts"] = res["charts_count"]
    return js


def write_outputs(out, verts, faces, res):
    """`<out>.ply`, the pages and `<out>.json` -> output_paths(out, pages)."""
    from PIL import Image
    t0 = time.time()
    paths = output_paths(out, res["pages"])
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    write_textured_ply(paths["ply"], verts, faces, res["tc"], res["texnum"], texture_names(out, res["pages"]))
    for k, p in enumerate(paths["pages"]):
        Image.fromarray(np.ascontiguousarray(res["atlas"][k])).save(p, format="PNG", compress_level=1)
    res["write_seconds"] = time.time() - t0
    with open(paths["json"], "w") as f:
        json.dump(summary(res), f, indent=1)
        f.write("\n")
    return paths


def from_folder(data_folder, output_folder, mesh=None, out=None, occlusion_tol=None, border_px=2.0, pad=2, page=8192, device=None,
                log=print, seam_level=False, seam_lambda=SEAM_LAMBDA, seam_tol=SEAM_TOL, seam_iters=SEAM_ITERS):
    """The whole chain step: read the mesh and the views, texture, write output_paths(out) -> texture_mesh()'s dict."""
    import torch
    from .ortho import load_views
    if not torch.cuda.is_available():
        raise RuntimeError("texture: needs an MI355X (there is no CPU fallback for the texture kernels)")
    mesh = mesh or os.path.join(output_folder, "mesh.ply")
    out = out or os.path.join(output_folder, "mesh_textured")
    if occlusion_tol is None:
        occlusion_tol = default_tol(mesh)
        if occlusion_tol is None:
            raise ValueError("%s.json is absent: give --occlusion_tol" % mesh)
    check_page(page)
    check_options(occlusion_tol, border_px, pad)
    if seam_level:
        check_seam_options(seam_lambda, seam_tol, seam_iters)
    t0 = time.time()
    verts, faces = read_mesh_ply(mesh)
    check_mesh(len(verts), faces)
    device = torch.device(device if device is not None else "cuda")
    views = load_views(fusion.Folder(data_folder, output_folder), device)
    if not views:
        raise ValueError("%s: no view has both <name>.jpg and <name>.txt" % output_folder)
    xyz = np.stack([verts["x"], verts["y"], verts["z"]], 1)
    rgb = np.stack([verts["red"], verts["green"], verts["blue"]], 1)
    res = texture_mesh(xyz, rgb, faces, views, occlusion_tol, border_px, pad, page, device, seam_level=seam_level, seam_lambda=seam_lambda,
                       seam_tol=seam_tol, seam_iters=seam_iters)
    write_outputs(out, verts, faces, res)
    res["seconds"] = time.time() - t0
    if seam_level:
        log("texture: seams levelled over %d nodes in %d iterations%s, residual %.2e; rms across seams %.2f -> %.2f levels"
            % (res["nodes"], res["seam_iterations"], " (the cap: raise --seam_iters)" if res["seam_cap_hit"] else "",
               max(res["seam_residual"]), res["seam_rms_before"], res["seam_rms_after"]))
    log("texture: %d faces, %d textured in %d charts on %d page(s) of %d, %d untextured; %d views used, %d culled; device %.1f ms, "
        "total_time = %.3f s" % (res["faces"], res["faces_textured"], res["charts_count"], res["pages"], res["P"], res["faces_untextured"],
                                 len(res["views_used"]), len(res["views_culled"]), res["device_ms_total"], res["seconds"]))
    return res


def build_parser():
    ap = argparse.ArgumentParser(description="Texture the TSDF mesh with the source images")
    ap.add_argument("--data_folder", required=True, help="the whu-omvs data folder predict_whu.py read")
    ap.add_argument("--output_folder", required=True, help="predict_whu.py's output folder (its <vid>/<name>.jpg and .txt)")
    ap.add_argument("--mesh", default=None, help="mesh PLY of mesh_whu.py (default <output_folder>/mesh.ply)")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="output prefix (default <output_folder>/mesh_textured): <out>.ply, ...")
    ap.add_argument("--occlusion_tol", type=float, default=None, metavar="M",
                    help="depth tolerance of the visibility test (default twice the voxel in <mesh>.json)")
    ap.add_argument("--border_px", type=float, default=2.0, help="faces closer than this to an image edge are not textured from it")
    ap.add_argument("--pad", type=int, default=2, help="pixels added around every chart's box")
    ap.add_argument("--page", type=int, default=8192, help="side of the square atlas pages (a power of two 1024 .. 16384)")
    ap.add_argument("--seam_level", action="store_true", help="level the colour steps between charts of different views (a global solve)")
    ap.add_argument("--seam_lambda", type=float, default=SEAM_LAMBDA, help="smoothness edges weigh 1 / lambda against the seams' 1")
    ap.add_argument("--seam_tol", type=float, default=SEAM_TOL, help="stop the solve at |r| <= seam_tol |b| in every channel")
    ap.add_argument("--seam_iters", type=int, default=SEAM_ITERS, help="at most this many conjugate-gradient iterations")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    return from_folder(args.data_folder, args.output_folder, args.mesh, args.out, args.occlusion_tol, args.border_px, args.pad, args.page,
                       seam_level=args.seam_level, seam_lambda=args.seam_lambda, seam_tol=args.seam_tol, seam_iters=args.seam_iters)


if __name__ == "__main__":
    main()
