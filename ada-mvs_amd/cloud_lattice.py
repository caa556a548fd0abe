"""The Python side of csrc/cloud_lattice.h: what accuracy.py, cloud_filter.py and register.py do to a cloud before a search walks
the lattice.  The cloud is checked, keyed on the lattice of cubic cells (adamvs_simplify_keys), sorted stably by key, its occupied
cells are numbered, and the sorted queries are cut into work items of one cell and at most CLOUD_TILE queries.  The sort, the
numbering and the cut are plain torch on whatever device the keys live on; the keys come from the kernel.
"""
import numpy as np

from .mesh_stage import MAX_COUNT


def cloud(t, name, stage="the cloud distance"):
    """t: [n, 3] float64 GPU tensor of at most MAX_COUNT points -> t, contiguous.  stage: what has no CPU fallback."""
    import torch
    from . import _lib
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.AdaMVSHipError("%s must be a GPU tensor: %s has no CPU fallback" % (name, stage))
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 3:
        raise _lib.AdaMVSHipError("%s: [n, 3] float64, got %s %s" % (name, tuple(t.shape), t.dtype))
    if t.shape[0] > MAX_COUNT:
        raise _lib.AdaMVSHipError("%s: more than 2^31 - 1 points" % name)
    return t.contiguous()


def default_origin(cell, lo):
    """Per axis the minimum `lo` of the targets - c / 3 - c (simplify.default_lattice_origin, lowered by one whole cell, so that
    the lower neighbour of every target's cell lies in the lattice)."""
    return np.asarray(lo, np.float64).reshape(3) - float(cell) / 3.0 - float(cell)


def origin_of(origin, cell, points, noun):
    """The caller's origin, or default_origin under the points (device tensor; noun: "target"); refused where not finite."""
    from . import _lib
    o = np.asarray(origin, np.float64).reshape(3) if origin is not None else default_origin(cell, points.min(0).values.cpu().numpy())
    if not np.isfinite(o).all():
        raise _lib.AdaMVSHipError("the lattice origin %r is not finite (a %s is not?)" % (o, noun))
    return o


def keyed(points, cell, origin, who, noun):
    """The keys [n] int64 of the points, all of which must lie in the lattice: "<who>: 3 <noun> are not finite, ..." otherwise."""
    from . import _lib, hip_ops
    keys, bad = hip_ops.simplify_keys(points, cell, origin)
    if int(bad.max()):
        raise _lib.AdaMVSHipError("%s: %d %s are not finite, %d lie outside the lattice of 2^21 cells per axis (cell %g, lattice "
                                  "origin %s)" % (who, int((bad == 1).sum()), noun, int((bad == 2).sum()), cell, origin.tolist()))
    return keys


def cut(cell_key, cell_count):
    """Runs of cell_count[j] sorted queries in the cell cell_key[j], end to end -> (item_key, item_first [ni] int64, item_count [ni]
    int32): every run cut into work items of at most CLOUD_TILE queries, first the position in the sorted order."""
    import torch
    from . import _lib
    dev, T = cell_key.device, _lib.CLOUD_TILE
    cell_first = torch.cumsum(cell_count, 0) - cell_count
    pieces = (cell_count + (T - 1)) // T
    owner = torch.repeat_interleave(torch.arange(cell_key.numel(), device=dev), pieces)
    rank = torch.arange(owner.numel(), device=dev) - (torch.cumsum(pieces, 0) - pieces)[owner]
    return (cell_key[owner].contiguous(), (cell_first[owner] + rank * T).contiguous(),
            torch.clamp(cell_count[owner] - rank * T, max=T).to(torch.int32))


def work_items(sorted_keys, order):
    """The stable sort of the query keys (values, indices) -> (outside: the queries with a key of -1; qorder [nqs] int64: the others
    in sorted order; the work items of cut(), or None where no query lies in the lattice)."""
    import torch
    outside = int(torch.searchsorted(sorted_keys, torch.zeros(1, device=sorted_keys.device, dtype=torch.int64)))     # keys of -1 sort first
    qorder = order[outside:].contiguous()
    if qorder.numel() == 0:
        return outside, qorder, None
    return outside, qorder, cut(*torch.unique_consecutive(sorted_keys[outside:], return_counts=True))


class Cells:
    """points [n, 3] under their keys [n] (all >= 0), sorted stably: ukeys [nc] int64, the occupied cells ascending; count [nc] and
    tstart [nc + 1] int64, the length and the start of each cell's run; sorted [n, 3], the points in that order; order [n] int64
    and index [n] int32, their numbers in the caller's order."""

    def __init__(self, points, keys):
        import torch
        ks = torch.sort(keys, stable=True)
        self.ukeys, self.count = torch.unique_consecutive(ks.values, return_counts=True)
        self.tstart = torch.zeros(int(self.ukeys.numel()) + 1, device=keys.device, dtype=torch.int64)
        self.tstart[1:] = torch.cumsum(self.count, 0)
        self.order = ks.indices
        self.sorted = points[ks.indices].contiguous()
        self.index = ks.indices.to(torch.int32)

    def items(self):
        """The work items of the cloud as its own queries."""
        return cut(self.ukeys, self.count)
