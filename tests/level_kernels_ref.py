"""Restatements of the seam-levelling kernels (csrc/texture_level.hip) one call at a time, on synthetic CSR graphs: the graph
generators, the sums of _level_rhs and of the SpMV in the kernel's own order (float64, entry by entry, no contraction), the
fp32 observed colour operation by operation, the longdouble dot products with the error bound of the fixed summation order,
a sparse Laplacian and plain conjugate gradients on it.  Everything is vectorised over the rows: the only Python loops run over
the entry rank k within a row (up to the largest degree) and over the views.

texture_level_ref.py holds the definition (dense, float64); this file restates the kernels' order of operations."""
import numpy as np
import scipy.sparse as sp

DATA, SEAM, INDEX = 0x80000000, 0x40000000, 0x3FFFFFFF
TILE, BLOCKS, BATCH = 256, 2048, 8             # ADAMVS_TEXTURE_TILE, ADAMVS_TEXTURE_LEVEL_BLOCKS, LVL_BATCH
SPECIAL_DEGREES = (0, 1, 7, 8, 9, 16, 17, 40)   # an empty row, the SpMV batch of 8 exactly full, one over, two batches, one over
ST_RR, ST_BB, ST_ALPHA, ST_BETA, ST_DONE, ST_ITERS, ST_TOL2 = 0, 3, 6, 9, 12, 13, 14
U64 = 2.0 ** -53                                # fp64 unit roundoff
KINDS = np.array([DATA, 0, SEAM], np.int64)     # kind code 0: data, 1: smoothness, 2: smoothness on a seam


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def csr(n, row, nbr, code):
    """Directed entries (row, neighbour, kind code) -> dict(n, rowptr int32 [n + 1], col uint32 [nnz], row int64 [nnz]), every
    row sorted by neighbour (one sort of a packed key)."""
    key = np.sort((np.asarray(row, np.int64) << 32) | (np.asarray(nbr, np.int64) << 2) | np.asarray(code, np.int64))
    row, nbr, code = key >> 32, (key >> 2) & INDEX, key & 3
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=rowptr[1:])
    return dict(n=n, rowptr=rowptr.astype(np.int32), col=(nbr | KINDS[code]).astype(np.uint32), row=row)


def random_graph(n, seed, mean_deg=6, special=True, stray=True, upper_only=False):
    """A seeded symmetric graph of about mean_deg neighbours per node with the three kinds of edge mixed.  From 400 nodes on,
    with special: eight nodes (the first, the last and six others) have exactly SPECIAL_DEGREES entries.  With stray: a few
    rows carry one more word whose index is >= n, of every kind (the kernels skip it; it sorts last).  upper_only keeps only the entries with
    neighbour > row: a matrix that is neither symmetric nor definite."""
    rng = np.random.default_rng(seed)
    m = min(mean_deg * n // 2, 4 * n * max(n - 1, 0))
    a, b = rng.integers(0, max(n, 1), m), rng.integers(0, max(n, 1), m)
    if n >= 2:
        a, b = np.append(a, 0), np.append(b, n - 1)
    spec = np.zeros(0, np.int64)
    if special and n >= 400:
        spec = np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), len(SPECIAL_DEGREES) - 2, replace=False)])
        is_spec = np.zeros(n, bool)
        is_spec[spec] = True
        keep = ~(is_spec[a] | is_spec[b])
        a, b = a[keep], b[keep]
        for s, d in zip(spec, SPECIAL_DEGREES):
            cand = rng.choice(n, d + 2 * len(spec), replace=False)
            cand = cand[~is_spec[cand]][:d]
            a, b = np.concatenate([a, np.full(d, s)]), np.concatenate([b, cand])
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    und = np.unique(lo * n + hi)
    lo, hi = und // max(n, 1), und % max(n, 1)
    code = rng.integers(0, 3, len(lo))
    row, nbr, code = (np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([code, code]))
    if upper_only:
        keep = nbr > row
        row, nbr, code = row[keep], nbr[keep], code[keep]
    if stray and n >= 1:
        k = min(5, n)
        srow = rng.choice(n, k, replace=False)
        if len(spec):
            srow = srow[~np.isin(srow, spec)]
        sidx = np.concatenate([[n, INDEX], rng.integers(n, INDEX, 3)])[:len(srow)]
        row, nbr, code = np.concatenate([row, srow]), np.concatenate([nbr, sidx]), np.concatenate([code, np.resize([2, 0, 1, 2, 0], len(srow))])
    g = csr(n, row, nbr, code)
    g["special"] = spec
    return g


def equitable_graph(n, seed, classes=7):
    """classes blocks of n // classes nodes; between every two blocks one random perfect matching, of one kind per pair of
    blocks: a random (classes - 1)-regular graph whose partition into the blocks is equitable, so the vectors that are constant on
    every block form an invariant subspace of its Laplacian.  The n mod classes last nodes are isolated."""
    rng = np.random.default_rng(seed)
    c = n // classes
    lo, hi, code = [], [], []
    for a in range(classes):
        for b in range(a + 1, classes):
            lo.append(a * c + np.arange(c))
            hi.append(b * c + rng.permutation(c))
            code.append(np.full(c, rng.integers(0, 3)))
    lo, hi, code = (np.concatenate(x) if c else np.zeros(0, np.int64) for x in (lo, hi, code))
    g = csr(n, np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([code, code]))
    g["block"] = np.minimum(np.arange(n) // max(c, 1), classes)       # classes: the isolated rest
    return g


def degrees(g):
    return np.diff(g["rowptr"].astype(np.int64))


def ranks(g):
    """For k = 0, 1, ...: (rows that hold a k-th entry, that entry's index): a row's entries in ascending order, one per step."""
    rp, deg = g["rowptr"].astype(np.int64), degrees(g)
    rows = np.nonzero(deg > 0)[0]
    k = 0
    while len(rows):
        yield rows, rp[rows] + k
        k += 1
        rows = rows[deg[rows] > k]


def laplacian_sparse(g, w_smooth):
    """L = D - W (scipy CSR, float64) over the entries whose index is < n: weight 1 on data entries, w_smooth on the others."""
    n = g["n"]
    word = g["col"].astype(np.int64)
    j = word & INDEX
    ok = j < n
    w = np.where(word & DATA, 1.0, w_smooth)[ok]
    W = sp.csr_matrix((w, (g["row"][ok], j[ok])), shape=(n, n))
    return (sp.diags(np.asarray(W.sum(1)).reshape(-1)) - W).tocsr()


# ---- the kernels' sums, in their order ----------------------------------------------------------------------------------------------
def rhs_ordered(g, f):
    """k_lvl_rhs: s = 0; for the row's data entries j < n in ascending order s += (double)f_j - (double)f_i."""
    n = g["n"]
    f = np.asarray(f, np.float32).astype(np.float64)
    s = np.zeros((n, 3))
    word = g["col"].astype(np.int64)
    for rows, e in ranks(g):
        j = word[e] & INDEX
        ok = ((word[e] & DATA) != 0) & (j < n)
        rows, j = rows[ok], j[ok]
        s[rows] += f[j] - f[rows]
    return s


def spmv_ordered(g, p, w_smooth):
    """k_lvl_spmv: d = 0, s = 0; for the row's entries j < n in ascending order d += w, s += w p_j; Ap_i = d p_i - s (every
    product rounded before it is added: numpy does not contract)."""
    n = g["n"]
    d, s = np.zeros(n), np.zeros((n, 3))
    word = g["col"].astype(np.int64)
    for rows, e in ranks(g):
        j = word[e] & INDEX
        ok = j < n
        rows, j = rows[ok], j[ok]
        w = np.where(word[e][ok] & DATA, 1.0, w_smooth)
        d[rows] += w
        s[rows] += w[:, None] * p[j]
    return d[:, None] * p - s


def grid(n):
    """-> (nb, chunk, pairs, pchunk) of launch_lvl_cg: workgroups, rows per workgroup, 16-byte pairs, pairs per workgroup."""
    nb = min(max((n + TILE - 1) // TILE, 1), BLOCKS)
    pairs = (3 * n + 1) // 2
    return nb, (n + nb - 1) // nb, pairs, (pairs + nb - 1) // nb


def dot_path(per_block, nb):
    """Additions on the longest path from one term of a dot product to its total: a lane adds ceil(per_block / 256) terms one
    after the other, the xor tree over the 64 lanes adds 6 times, the four waves 3 times; the reducing workgroup repeats that
    over the nb partials: ceil(nb / 256) + 6 + 3.  Two of these additions start from an exact 0, which leaves room for the
    rounding of the term's own product and for the second-order terms, so the count times 2^-53, relative to the sum of the
    absolute values of the terms, bounds the error of the whole."""
    return -(-per_block // TILE) + 6 + 3 + -(-nb // TILE) + 6 + 3


def dot_ld(a, b):
    """Per channel: (sum a b, sum |a b|) in longdouble (64-bit mantissa: the products of doubles round at 2^-64)."""
    t = np.asarray(a, np.longdouble) * np.asarray(b, np.longdouble)
    return t.sum(0), np.abs(t).sum(0)


def cg_sparse(Lm, b, tol, iters):
    """tests/texture_level_ref.py's cg on a sparse L -> (g, iterations, [max over channels of |r| / |b| after 0, 1, ...
    iterations])."""
    g = np.zeros_like(b)
    r, p = b.copy(), b.copy()
    rr = (r * r).sum(0)
    bb = rr.copy()
    rel = lambda: float(np.sqrt(np.where(bb > 0, rr / np.where(bb > 0, bb, 1.0), np.where(rr > 0, np.inf, 0.0))).max()) if len(b) else 0.0
    it, hist = 0, [rel()]
    while it < iters and not (rr <= tol * tol * bb).all():
        Ap = Lm @ p
        pAp = (p * Ap).sum(0)
        alpha = np.where(pAp > 0, rr / np.where(pAp > 0, pAp, 1.0), 0.0)
        g += alpha * p
        r -= alpha * Ap
        new = (r * r).sum(0)
        beta = np.where((rr > 0) & (alpha != 0), new / np.where(rr > 0, rr, 1.0), 0.0)
        rr = new
        p = r + beta * p
        it += 1
        hist.append(rel())
    return g, it, hist


# ---- the observed colour, fp32 operation by operation ---------------------------------------------------------------------------------
F = np.float32


def sample32(img, x, y):
    """lvl_sample on one image uint8 [H, W, 4] at fp32 positions (no NaN) -> [m, 3] fp32."""
    H, W = img.shape[:2]
    x = np.minimum(np.maximum(x, F(0)), F(W - 1))
    y = np.minimum(np.maximum(y, F(0)), F(H - 1))
    xa, ya = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = (x - xa.astype(F))[:, None], (y - ya.astype(F))[:, None]
    xb, yb = np.minimum(xa + 1, W - 1), np.minimum(ya + 1, H - 1)
    c = img[..., :3].astype(F)
    one = F(1)
    out = (one - fy) * ((one - fx) * c[ya, xa] + fx * c[ya, xb]) + fy * ((one - fx) * c[yb, xa] + fx * c[yb, xb])
    assert out.dtype == F
    return out


def sample_views32(images, view, x, y):
    out = np.zeros((len(x), 3), F)
    for v, img in enumerate(images):
        m = view == v
        if m.any():
            out[m] = sample32(img, x[m], y[m])
    return out


def observe32(g, pos, node_view, images):
    """k_lvl_observe: 0 for a node whose view is out of range; else over the row's seam entries j < n in ascending order and
    (t, w) = (0, 1), (1/4, 3/4), (1/2, 1/2): acc = acc + w sample(p + t (pos_j - p)), wsum = wsum + w; f = acc / wsum, or sample(p)
    when wsum is 0.  All fp32."""
    n = g["n"]
    pos = np.asarray(pos, F).reshape(n, 2)
    view = np.asarray(node_view, np.int64)
    valid = (view >= 0) & (view < len(images))
    acc, wsum = np.zeros((n, 3), F), np.zeros(n, F)
    word = g["col"].astype(np.int64)
    for rows, e in ranks(g):
        j = word[e] & INDEX
        ok = ((word[e] & DATA) == 0) & ((word[e] & SEAM) != 0) & (j < n) & valid[rows]
        rows, j = rows[ok], j[ok]
        du, dv = pos[j, 0] - pos[rows, 0], pos[j, 1] - pos[rows, 1]
        for t, w in ((F(0), F(1)), (F(0.25), F(0.75)), (F(0.5), F(0.5))):
            s = sample_views32(images, view[rows], pos[rows, 0] + t * du, pos[rows, 1] + t * dv)
            acc[rows] = acc[rows] + w * s
            wsum[rows] = wsum[rows] + w
    f = np.where(valid[:, None], sample_views32(images, np.where(valid, view, -1), pos[:, 0], pos[:, 1]), F(0))
    has = wsum != 0
    f[has] = acc[has] / wsum[has, None]
    assert f.dtype == F
    return f
