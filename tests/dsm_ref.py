"""fp64 numpy restatement of the DSM rasterisation (include/adamvs_hip.h "DSM"), operation for operation: the GPU kernels are
held to it bit for bit."""
import numpy as np

NAN32 = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.float32)[0]


def order(h):
    """fp32 heights -> order-preserving uint32 (-0 taken as +0)."""
    h = np.asarray(h, np.float32)
    b = np.where(h == 0, np.float32(0), h).astype(np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unorder(o):
    o = np.asarray(o, np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(np.float32)


def cells(grid, xyz):
    """-> (used [n] bool, cell [n] int64 (0 where unused), dz [n] float64)."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        fi = np.floor((xyz[:, 0] - grid.x0) / grid.gsd)
        fj = np.floor((grid.y_top - xyz[:, 1]) / grid.gsd)
        dz = xyz[:, 2] - grid.z_ref
        used = (fi >= 0) & (fi < grid.W) & (fj >= 0) & (fj < grid.H) & (np.abs(dz) < 65536.0)
    cell = np.where(used, np.where(used, fj, 0) * grid.W + np.where(used, fi, 0), 0).astype(np.int64)
    return used, cell, dz


def keys(dz, seq):
    with np.errstate(over="ignore", invalid="ignore"):
        h = dz.astype(np.float32)
    return (order(h).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - seq.astype(np.uint64))


def restate(grid, xyz, rgb, mode="max", min_count=1, seq0=0):
    """The whole stream at once -> dict(dsm [H, W] float32, count [H, W] uint16, rgba [H, W, 4] uint8, count32, key, used)."""
    n = len(xyz)
    ncell = grid.W * grid.H
    used, cell, dz = cells(grid, xyz)
    seq = np.uint64(seq0) + np.arange(n, dtype=np.uint64)
    key = keys(dz, seq)
    cu = cell[used]
    K = np.zeros(ncell, np.uint64)
    np.maximum.at(K, cu, key[used])
    cnt = np.zeros(ncell, np.uint32)
    np.add.at(cnt, cu, np.uint32(1))
    color = np.zeros((ncell, 4), np.uint8)
    win = used.copy()
    win[used] = key[used] == K[cu]
    color[cell[win], :3] = np.asarray(rgb, np.uint8).reshape(-1, 3)[win]
    color[cell[win], 3] = 255
    assert len(np.unique(cell[win])) == win.sum() == (cnt > 0).sum()
    filled = cnt >= min_count
    dsm = np.full(ncell, NAN32, np.float32)
    if mode == "max":
        h = unorder((K[filled] >> np.uint64(32)).astype(np.uint32))
        dsm[filled] = (grid.z_ref + h.astype(np.float64)).astype(np.float32)
    else:
        S = np.zeros(ncell, np.int64)
        np.add.at(S, cu, np.rint(dz[used] * 65536.0).astype(np.int64))
        dsm[filled] = (grid.z_ref + (S[filled].astype(np.float64) / cnt[filled].astype(np.float64)) / 65536.0).astype(np.float32)
    color[~filled] = 0
    return dict(dsm=dsm.reshape(grid.H, grid.W), count=np.minimum(cnt, 65535).astype(np.uint16).reshape(grid.H, grid.W),
                rgba=color.reshape(grid.H, grid.W, 4), count32=cnt.reshape(grid.H, grid.W), key=K.reshape(grid.H, grid.W), used=used)


def combined_requests(cell, used, wave=64):
    """Atomic wave-lanes the combined accumulate issues: runs of equal cells inside each aligned group of 64 points (one per run
    of used points), against used.sum() uncombined."""
    c = np.where(used, cell, -1)
    n = len(c)
    head = np.ones(n, bool)
    head[1:] = c[1:] != c[:-1]
    head[::wave] = True
    return int((head & used).sum())
