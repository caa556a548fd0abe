"""The contour stage restated in numpy (include/adamvs_hip.h "Contours", steps 1 - 7): vectorised over the blocks per level, a
dictionary of crossings for the links, and a plain serial walk for the lines.  It shares no code with ada-mvs_amd/contours.py
or with the kernels: no closed-form segment numbers, no binary searches, no pointer doubling."""
import numpy as np

NONE = -2 ** 31                                     # s outside V
# edge e of block (i, j) -> (row offset, column offset, d) of its grid edge: AB east of A, BC south of B, CD east of D, DA south of A
EDGE = ((0, 0, 0), (0, 1, 1), (1, 0, 0), (0, 0, 1))


def surface(z, z_ref, passes):
    """-> (s int64 [H, W], (s_min, s_max, out_of_range))"""
    z = np.asarray(z, np.float32)
    d = z.astype(np.float64) - float(z_ref)
    finite = np.isfinite(z)
    with np.errstate(invalid="ignore"):
        V = finite & (np.abs(d) <= 8191.0)
    s = np.where(V, np.rint(np.where(V, d, 0.0) * 256.0), 0).astype(np.int64)         # rint: ties to even
    H, W = z.shape
    for _ in range(passes):
        sp, vp = np.pad(s, 1), np.pad(V, 1)
        out = np.zeros_like(s)
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                nb, ok = sp[1 + di:1 + di + H, 1 + dj:1 + dj + W], vp[1 + di:1 + di + H, 1 + dj:1 + dj + W]
                out += (2 - abs(di)) * (2 - abs(dj)) * np.where(ok, nb, s)
        s = out
    info = (int(s[V].min()) if V.any() else 2 ** 31 - 1, int(s[V].max()) if V.any() else NONE, int((finite & ~V).sum()))
    return np.where(V, s, NONE), info


def segments(s, lev):
    """-> dict(count int64 [H, W], N, entry, exit, level, succ, pred (int64 [N]))"""
    s = np.asarray(s, np.int64)
    H, W = s.shape
    rows = []
    if H > 1 and W > 1:
        corner = [s[:-1, :-1], s[:-1, 1:], s[1:, 1:], s[1:, :-1]]                    # A, B, C, D
        valid = np.ones((H - 1, W - 1), bool)
        for c in corner:
            valid &= c != NONE
        bi, bj = np.meshgrid(np.arange(H - 1), np.arange(W - 1), indexing="ij")
        total = corner[0] + corner[1] + corner[2] + corner[3]
        for k, level in enumerate(lev):
            up = [c >= level for c in corner]
            entry = [valid & ~up[e] & up[(e + 1) % 4] for e in range(4)]
            leave = [valid & up[e] & ~up[(e + 1) % 4] for e in range(4)]
            n_entry = sum(e.astype(np.int64) for e in entry)
            the_exit = sum(e * x.astype(np.int64) for e, x in enumerate(leave))      # where there is one exit
            centre_up = 2 * total >= 4 * (2 * int(level) - 1)
            for e in range(4):
                i, j = bi[entry[e]], bj[entry[e]]
                saddle = n_entry[entry[e]] == 2
                x = np.where(saddle, np.where(centre_up[entry[e]], (e - 1) % 4, (e + 1) % 4), the_exit[entry[e]])
                code_in = 2 * ((i + EDGE[e][0]) * W + j + EDGE[e][1]) + EDGE[e][2]
                table = np.array(EDGE, np.int64)
                code_out = 2 * ((i + table[x, 0]) * W + j + table[x, 1]) + table[x, 2]
                rows.append(np.stack([i * W + j, np.full(i.size, k, np.int64), np.full(i.size, e, np.int64), code_in, code_out], axis=1))
    rows = np.concatenate(rows) if rows else np.zeros((0, 5), np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]                      # by (block, level, entry edge)
    N = rows.shape[0]
    count = np.bincount(rows[:, 0], minlength=H * W).reshape(H, W).astype(np.int64)
    entry, leave, level = rows[:, 3], rows[:, 4], rows[:, 1]
    by_entry = {(int(c), int(k)): n for n, (c, k) in enumerate(zip(entry.tolist(), level.tolist()))}
    by_exit = {(int(c), int(k)): n for n, (c, k) in enumerate(zip(leave.tolist(), level.tolist()))}
    assert len(by_entry) == N and len(by_exit) == N, "a crossing is the entry of two segments, or the exit of two"
    succ = np.array([by_entry.get((int(c), int(k)), -1) for c, k in zip(leave.tolist(), level.tolist())], np.int64).reshape(N)
    pred = np.array([by_exit.get((int(c), int(k)), -1) for c, k in zip(entry.tolist(), level.tolist())], np.int64).reshape(N)
    return dict(count=count, N=N, entry=entry, exit=leave, level=level, succ=succ, pred=pred)


def walk(succ, pred):
    """The serial walk: -> (start, rank, closed), int64 [N] each."""
    N = len(succ)
    start, rank, closed = np.full(N, -1, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    for ring in (0, 1):                             # first the open chains from their heads, then what is left, smallest first
        for n in range(N):
            if start[n] >= 0 or (not ring and pred[n] >= 0):
                continue
            m, r = n, 0
            while m >= 0 and start[m] < 0:
                start[m], rank[m], closed[m] = n, r, ring
                m, r = int(succ[m]), r + 1
            assert (m == n) if ring else (m < 0)
    return start, rank, closed


def lines(s, lev, seg, start, rank, closed):
    """-> dict(M, line_first int64 [M + 1], line_start, line_level, line_closed (int64 [M]), vertex int64 [N + M, 3])"""
    s = np.asarray(s, np.int64).reshape(-1)
    W = np.asarray(seg["count"]).shape[1]
    N = seg["N"]
    line_start = np.unique(start)
    M = line_start.size
    vertex, first = [], [0]
    order = np.lexsort((rank, start))              # line by line (ascending start), each in rank order
    cuts = np.flatnonzero(np.diff(start[order])) + 1 if N else np.zeros(0, np.int64)
    for members in (np.split(order, cuts) if N else []):
        assert rank[members].tolist() == list(range(members.size))
        crossings = [(int(seg["entry"][n]), int(seg["level"][n])) for n in members] + [(int(seg["exit"][members[-1]]), int(seg["level"][members[-1]]))]
        for code, k in crossings:
            c = code >> 1
            a, b2 = int(s[c]), int(s[c + (W if code & 1 else 1)])
            num, den = 2 * int(lev[k]) - 1 - 2 * a, 2 * b2 - 2 * a
            if den < 0:
                num, den = -num, -den
            vertex.append((code, num, den))
        first.append(len(vertex))
    assert len(vertex) == N + M
    return dict(M=M, line_first=np.array(first, np.int64), line_start=line_start.astype(np.int64),
                line_level=np.asarray(seg["level"], np.int64)[line_start] if M else np.zeros(0, np.int64),
                line_closed=closed[line_start] if M else np.zeros(0, np.int64), vertex=np.array(vertex, np.int64).reshape(-1, 3))


def trace(z, z_ref, passes, lev=None, table=None):
    """Steps 1 - 7.  lev: the level table; or table(s_min, s_max) -> lev, asked once the surface is known."""
    s, info = surface(z, z_ref, passes)
    if lev is None:
        lev = table(info[0], info[1])
    seg = segments(s, lev)
    start, rank, closed = walk(seg["succ"], seg["pred"])
    res = dict(s=s, info=info, lev=list(lev), start=start, rank=rank, closed=closed, **seg)
    res.update(lines(s, lev, seg, start, rank, closed))
    return res
