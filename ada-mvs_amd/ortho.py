"""Image orthophoto: the source images mosaicked over a DSM into a true orthophoto on the GPU.

    python ortho_whu.py --data_folder D --output_folder O --dsm PREFIX [--filled] [--upsample K] [--mode best|feather]
                        [--occlusion_tol M] [--border_px 2] [--feather_px 64] [--out PREFIX]
                        [--balance gain] [--gain_sigma 0.1] [--noise_sigma 10] [--balance_stride S] [--balance_max_diff LEVELS]
                        [--balance_min_samples 64]

The step after dsm_whu.py.  PREFIX is the prefix dsm_whu.py --out was given: the grid comes from `<PREFIX>_dsm.json`, the
heights from `<PREFIX>_dsm.tif` (or `<PREFIX>_dsm_filled.tif` with --filled; NaN: no surface).  The views are predict's
images `<vid>/<name>.jpg` with the `<name>.txt` intrinsics and the fp64 poses of image_info.txt, every view with both files,
in ascending image id.  Per view, csrc/ortho.hip renders the DSM's triangulated height field into a depth buffer at the
image's size, then every orthophoto cell's surface point is projected, tested against that buffer and coloured by a
bilinear sample; `best` keeps the most nadir view that sees the cell, `feather` blends every such view
(include/adamvs_hip.h "Image orthophoto" states every operation).  Written (--out defaults to PREFIX):
`<out>_ortho_img.png` (RGBA, alpha 0 where no surface or no view), `<out>_ortho_img.pgw`, `<out>_ortho_img_view.tif`
(int32 image id of the chosen view, -1 where none), `<out>_ortho_img_nvis.tif` (uint16 views that see the cell) and
`<out>_ortho_img.json`.  The orthophoto grid is the DSM's refined K times: cells of gsd / K from the same corner.

--balance gain levels the views' exposures before the mosaic (include/adamvs_hip.h "Image orthophoto: radiometric balance"):
every view is sampled on a lattice of every S-th DSM cell (csrc/ortho_balance.hip), the pairwise sums of the views over the
cells they both see are reduced on the GPU as exact integers, solve_gains() solves the V x V normal equations of Brown & Lowe's
gain compensation on the host, and the mosaic is made from the images scaled by their gains.  noise_sigma = 10 and
gain_sigma = 0.1 are the values Brown & Lowe published: conventions, not measurements on this data.  The JSON gains a
`balance` block (the gains, the overlap rms before and after, the rms colour step across the mosaic's seams).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

from . import fusion
from .dsm import Grid, world_file_text
from .mesh import cull_views

MODES = {"best": 0, "feather": 1}                   # ADAMVS_ORTHO_BEST / ADAMVS_ORTHO_FEATHER
MAX_CELLS = 1 << 28                                 # ADAMVS_ORTHO_MAX_CELLS
MAX_UPSAMPLE = 8                                    # ADAMVS_ORTHO_MAX_UPSAMPLE
CULL_MARGIN_PX = 2.0
BALANCE_MODELS = ("gain",)
BAL_MAX_SAMPLES = 1 << 20                           # ADAMVS_ORTHO_BAL_MAX_SAMPLES
BAL_MAX_VIEWS = 4096                                # the host solve is dense: V x V fp64
BAL_RUN = 64                                        # lattice cells per run of candidate_pairs
BAL_Q = 64                                          # quantisation of an observed colour: 1/64 level
NOISE_SIGMA, GAIN_SIGMA = 10.0, 0.1                 # Brown & Lowe 2007: published conventions, not measurements
ZBUF_CACHE_BYTES = 8 << 30                          # depth buffers kept from the balance pass for the mosaic (a convention)


def check_upsample(upsample):
    """K: an integer 1 .. 8 (an integral float is accepted)."""
    if isinstance(upsample, bool):
        raise ValueError("upsample %r: an integer 1 .. %d" % (upsample, MAX_UPSAMPLE))
    try:
        k = float(upsample)
    except (TypeError, ValueError):
        raise ValueError("upsample %r: an integer 1 .. %d" % (upsample, MAX_UPSAMPLE)) from None
    if not (math.isfinite(k) and k.is_integer() and 1 <= k <= MAX_UPSAMPLE):
        raise ValueError("upsample %r: an integer 1 .. %d" % (upsample, MAX_UPSAMPLE))
    return int(k)


def ortho_grid(grid, upsample):
    """The orthophoto grid of a DSM grid at upsample K, as a dsm.Grid: cells of gsd / K, W K x H K, the same x0 and y_top."""
    K = check_upsample(upsample)
    W, H = int(grid.W) * K, int(grid.H) * K
    if W * H > MAX_CELLS:
        raise ValueError("orthophoto of %d x %d cells (DSM %d x %d at upsample %d) exceeds the cap of %d cells"
                         % (W, H, grid.W, grid.H, K, MAX_CELLS))
    return Grid(float(grid.x0), float(grid.y_top), float(grid.gsd) / K, grid.z_ref, W, H)


def check_options(mode, occlusion_tol, border_px, feather_px):
    if mode not in MODES:
        raise ValueError("mode %r: one of %s" % (mode, sorted(MODES)))
    for name, v, lo_ok in (("occlusion_tol", occlusion_tol, True), ("border_px", border_px, True), ("feather_px", feather_px, False)):
        f = float(v)
        if not (math.isfinite(f) and (f >= 0.0 if lo_ok else f > 0.0)):
            raise ValueError("%s=%r must be finite and %s" % (name, v, ">= 0" if lo_ok else "> 0"))


def dsm_box(grid, dsm):
    """(lo, hi) fp64 of the DSM's bounding box: the grid's extent, z from the finite min and max; None if no cell is finite."""
    z = np.asarray(dsm, np.float32)
    fin = z[np.isfinite(z)]
    if fin.size == 0:
        return None
    lo = np.array([grid.x0, grid.y_top - grid.H * grid.gsd, float(fin.min())], np.float64)
    hi = np.array([grid.x0 + grid.W * grid.gsd, grid.y_top, float(fin.max())], np.float64)
    return lo, hi


def view_camera(view):
    """(K, R_wc, C, H, W) of a view dict for mesh.cull_views."""
    H, W = int(view["rgba"].shape[0]), int(view["rgba"].shape[1])
    return (np.asarray(view["K"], np.float64), np.asarray(view["R"], np.float64), np.asarray(view["C"], np.float64), H, W)


# ---- the GPU mosaic ---------------------------------------------------------------------------------------------------
class OrthoBuilder:
    """Cell state of one orthophoto on the device.  dsm: [H, W] float32 (host or device) on `grid` (a dsm.Grid);
    add_view() the views in ascending image id, finish() once.  A view is dict(iid, K [3, 3], R (R_wc), C (fp64),
    rgba device [H, W, 4] uint8).  keep_zbufs: keep each view's depth buffer in .zbufs (image id -> device tensor)."""

    def __init__(self, grid, upsample, mode, dsm, occlusion_tol=None, border_px=2.0, feather_px=64.0, device=None, keep_zbufs=False):
        import torch
        from . import hip_ops
        occlusion_tol = 2.0 * float(grid.gsd) if occlusion_tol is None else float(occlusion_tol)
        check_options(mode, occlusion_tol, border_px, feather_px)
        self.grid, self.K, self.mode = grid, check_upsample(upsample), mode
        self.ogrid = ortho_grid(grid, self.K)
        self.occlusion_tol, self.border_px, self.feather_px = occlusion_tol, float(border_px), float(feather_px)
        self.device = torch.device(device if device is not None else "cuda")
        d = dsm if isinstance(dsm, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dsm, np.float32))
        if tuple(d.shape) != (grid.H, grid.W):
            raise ValueError("dsm %s does not match the grid's %d x %d cells" % (tuple(d.shape), grid.H, grid.W))
        self.dsm = d.to(self.device, torch.float32).contiguous()
        self.box = dsm_box(grid, self.dsm.cpu().numpy())
        self.cgrid = hip_ops.ortho_grid(grid.x0, grid.y_top, grid.gsd, grid.W, grid.H, self.K)
        self.height = hip_ops.ortho_surface(self.cgrid, self.dsm)
        n = self.ogrid.W * self.ogrid.H
        self.acc = torch.zeros(n, 4, device=self.device, dtype=torch.float32)
        self.wmax = torch.full((n,), -math.inf if mode == "best" else 0.0, device=self.device, dtype=torch.float32)
        self.vstate = torch.full((n,), -1, device=self.device, dtype=torch.int32)
        self.nvis = torch.zeros(n, device=self.device, dtype=torch.int32)
        self.big = torch.empty(1 + 2 * max(grid.W - 1, 0) * max(grid.H - 1, 0), device=self.device, dtype=torch.int32)
        self.used, self.culled, self.events = [], [], []
        self.last_iid = None
        self.zbufs = {} if keep_zbufs else None          # image id -> the view's depth buffer (device int32, float bits)

    def sees(self, view):
        """Whether the view passes the cull (the DSM's box does not project wholly outside its image)."""
        return self.box is not None and bool(cull_views(self.box[0], self.box[1], [view_camera(view)], CULL_MARGIN_PX))

    def view_zbuf(self, view):
        """-> (the view as hip_ops.ortho_view, its depth buffer rendered now)."""
        import torch
        from . import hip_ops
        cam = view_camera(view)
        v = hip_ops.ortho_view(cam[0], cam[1].T, cam[2], view["rgba"])
        zbuf = torch.empty(cam[3], cam[4], device=self.device, dtype=torch.int32)
        hip_ops.ortho_zbuf(self.cgrid, self.dsm, v, zbuf, self.big)
        return v, zbuf

    def add_view(self, view, zbuf=None):
        """Mosaic one view in -> True, or False if it is culled (the DSM's box projects wholly outside its image).  zbuf: the
        view's depth buffer if the caller has it already (balance_views keeps them); by default it is rendered here."""
        import torch
        from . import hip_ops
        iid = int(view["iid"])
        if self.last_iid is not None and iid <= self.last_iid:
            raise ValueError("views must come in ascending image id: %d after %d" % (iid, self.last_iid))
        self.last_iid = iid
        cam = view_camera(view)
        if not self.sees(view):
            self.culled.append(iid)
            return False
        v = hip_ops.ortho_view(cam[0], cam[1].T, cam[2], view["rgba"])
        if zbuf is not None and tuple(zbuf.shape) != (cam[3], cam[4]):
            raise ValueError("zbuf %s does not match the image's %d x %d" % (tuple(zbuf.shape), cam[3], cam[4]))
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        if zbuf is None:
            zbuf = torch.empty(cam[3], cam[4], device=self.device, dtype=torch.int32)
            hip_ops.ortho_zbuf(self.cgrid, self.dsm, v, zbuf, self.big)
        e1.record()
        hip_ops.ortho_compose(self.cgrid, v, iid, self.height, zbuf, MODES[self.mode], self.border_px, self.feather_px, self.occlusion_tol,
                              self.acc, self.wmax, self.vstate, self.nvis)
        e2.record()
        self.events.append((e0, e1, e2))
        self.used.append(iid)
        if self.zbufs is not None:
            self.zbufs[iid] = zbuf
        return True

    def finish(self):
        """-> dict(rgba [H_o, W_o, 4] uint8, view int32, nvis uint16 (host arrays), grid (the orthophoto's dsm.Grid), summary
        counts and device seconds)."""
        import torch
        from . import hip_ops
        rgba, view, nvis = hip_ops.ortho_finalize(self.cgrid, self.acc, self.vstate, self.nvis)
        self.mosaic = (rgba, view)                       # on the device, for seam_stats
        rgba, view, nvis = rgba.cpu().numpy(), view.cpu().numpy(), nvis.cpu().numpy().view(np.uint16)
        torch.cuda.synchronize(self.device)
        t_z = sum(a.elapsed_time(b) for a, b, _ in self.events) / 1e3
        t_c = sum(b.elapsed_time(c) for _, b, c in self.events) / 1e3
        surface = ~torch.isnan(self.height).cpu().numpy()
        return dict(rgba=rgba, view=view, nvis=nvis, grid=self.ogrid, dsm_grid=self.grid, upsample=self.K, mode=self.mode,
                    occlusion_tol=self.occlusion_tol, border_px=self.border_px, feather_px=self.feather_px, views_used=list(self.used),
                    views_culled=list(self.culled), cells_surface=int(surface.sum()), cells_coloured=int((rgba[..., 3] > 0).sum()),
                    cells_unseen=int((surface & (nvis == 0)).sum()), zbuf_seconds=t_z, compose_seconds=t_c, device_seconds=t_z + t_c)


# ---- radiometric balance: one gain per view and channel ---------------------------------------------------------------
def lattice_shape(grid, stride):
    """(W_s, H_s) of the observation lattice: every stride-th DSM cell from cell (0, 0)."""
    S = int(stride)
    return -(-int(grid.W) // S), -(-int(grid.H) // S)


def default_stride(grid):
    """The smallest stride S whose lattice has at most 2^20 cells."""
    S = max(1, math.isqrt(int(grid.W) * int(grid.H) // BAL_MAX_SAMPLES))
    while lattice_shape(grid, S)[0] * lattice_shape(grid, S)[1] > BAL_MAX_SAMPLES:
        S += 1
    while S > 1 and lattice_shape(grid, S - 1)[0] * lattice_shape(grid, S - 1)[1] <= BAL_MAX_SAMPLES:
        S -= 1
    return S


def check_balance_options(balance, noise_sigma=NOISE_SIGMA, gain_sigma=GAIN_SIGMA, stride=None, max_diff=255.0, min_samples=64, grid=None):
    """Raises ValueError unless the options of the balance are in range -> (stride or None, max_diff_q)."""
    if balance not in BALANCE_MODELS:
        raise ValueError("balance %r: one of %s (or None)" % (balance, list(BALANCE_MODELS)))
    ns, gs, md = float(noise_sigma), float(gain_sigma), float(max_diff)
    if not (math.isfinite(ns) and ns > 0.0):
        raise ValueError("noise_sigma=%r must be finite and > 0" % (noise_sigma,))
    if not (math.isfinite(gs) and 0.0 < gs <= 100.0):
        raise ValueError("gain_sigma=%r must be in (0, 100]" % (gain_sigma,))
    if not (math.isfinite(md) and 0.0 <= md <= 255.0):
        raise ValueError("balance_max_diff=%r must be 0 .. 255 levels" % (max_diff,))
    if isinstance(min_samples, bool) or int(min_samples) != min_samples or int(min_samples) < 1:
        raise ValueError("balance_min_samples=%r must be an integer >= 1" % (min_samples,))
    if stride is not None:
        if isinstance(stride, bool) or int(stride) != stride or int(stride) < 1:
            raise ValueError("balance_stride=%r must be an integer >= 1" % (stride,))
        stride = int(stride)
        if grid is not None:
            Ws, Hs = lattice_shape(grid, stride)
            if Ws * Hs > BAL_MAX_SAMPLES:
                raise ValueError("balance_stride=%d: %d x %d lattice cells exceed the cap of %d (default_stride: %d)"
                                 % (stride, Ws, Hs, BAL_MAX_SAMPLES, default_stride(grid)))
    return stride, int(round(BAL_Q * md))


def candidate_pairs(obs):
    """obs device int16 [V, N_s, 4] -> the pairs (a, b), a < b, of views that are both visible somewhere in one run of 64
    consecutive lattice cells, as a host int32 [P, 2] in lexicographic order.  A pair whose views share no run shares no cell
    (its n is 0), so nothing is lost."""
    import torch
    V, Ns = int(obs.shape[0]), int(obs.shape[1])
    flags = obs[:, :, 3] != 0
    runs = -(-Ns // BAL_RUN)
    if runs * BAL_RUN != Ns:
        flags = torch.cat([flags, torch.zeros(V, runs * BAL_RUN - Ns, device=obs.device, dtype=torch.bool)], 1)
    seen = flags.view(V, runs, BAL_RUN).any(-1).to(torch.float32)
    common = seen @ seen.t()                            # counts of common runs: at most 2^14, exact in fp32
    idx = torch.triu(common > 0, diagonal=1).nonzero()  # row-major: lexicographic
    return idx.cpu().numpy().astype(np.int32).reshape(-1, 2)


def solve_gains(pairs, stats, V, noise_sigma=NOISE_SIGMA, gain_sigma=GAIN_SIGMA, min_samples=64):
    """The gains of Brown & Lowe's gain compensation from the pair statistics, fp64 on the host.  pairs [P, 2] (a < b), stats
    [P, 7] = (n, Sa_0..2, Sb_0..2) of adamvs_ortho_pair_stats.  Per channel k, over the pairs with n >= min_samples, with
    I_ab = Sa_k / (64 n) and I_ba = Sb_k / (64 n) (the mean of a, and of b, over their common cells), the minimum of
        sum n ((g_a I_ab - g_b I_ba)^2 / noise_sigma^2 + (1 - g_a)^2 / gain_sigma^2 + (1 - g_b)^2 / gain_sigma^2)
    over the views with such a pair; every other view gets exactly 1.  noise_sigma = 10 and gain_sigma = 0.1 are the published
    values (conventions, not measurements).  -> (gains [V, 3], rms_before [3], rms_after [3]): the rms over the used pairs of
    I_ab - I_ba and of g_a I_ab - g_b I_ba, weighted by n (0 where no pair is used)."""
    V = int(V)
    if not 1 <= V <= BAL_MAX_VIEWS:
        raise ValueError("V=%r: 1 .. %d views" % (V, BAL_MAX_VIEWS))
    check_balance_options("gain", noise_sigma, gain_sigma, None, 0.0, min_samples)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    stats = np.asarray(stats, np.int64).reshape(-1, 7)
    if pairs.shape[0] != stats.shape[0]:
        raise ValueError("%d pairs, %d rows of statistics" % (pairs.shape[0], stats.shape[0]))
    if pairs.size and not ((pairs[:, 0] >= 0) & (pairs[:, 0] < pairs[:, 1]) & (pairs[:, 1] < V)).all():
        raise ValueError("a pair is not 0 <= a < b < V = %d" % V)
    use = stats[:, 0] >= int(min_samples)
    a, b = pairs[use, 0], pairs[use, 1]
    n = stats[use, 0].astype(np.float64)
    iN, iG = 1.0 / float(noise_sigma) ** 2, 1.0 / float(gain_sigma) ** 2
    gains = np.ones((V, 3), np.float64)
    before, after = np.zeros(3), np.zeros(3)
    for k in range(3):
        if not n.size:
            break
        Iab = stats[use, 1 + k] / (BAL_Q * n)
        Iba = stats[use, 4 + k] / (BAL_Q * n)
        A = np.zeros((V, V), np.float64)
        r = np.zeros(V, np.float64)
        np.add.at(A, (a, a), n * (Iab * Iab * iN + iG))
        np.add.at(A, (b, b), n * (Iba * Iba * iN + iG))
        np.add.at(A, (a, b), -n * Iab * Iba * iN)
        np.add.at(A, (b, a), -n * Iab * Iba * iN)
        np.add.at(r, a, n * iG)
        np.add.at(r, b, n * iG)
        act = np.nonzero(np.diag(A) != 0.0)[0]
        gains[act, k] = np.linalg.solve(A[np.ix_(act, act)], r[act])
        before[k] = math.sqrt(float((n * (Iab - Iba) ** 2).sum() / n.sum()))
        after[k] = math.sqrt(float((n * (gains[a, k] * Iab - gains[b, k] * Iba) ** 2).sum() / n.sum()))
    return gains, before, after


def _balance(b, views, stride, max_diff_q, noise_sigma, gain_sigma, min_samples, zbuf_cache_bytes):
    """Pass 1 over the views (ascending image id) on the builder's DSM -> (gains {iid: [3] fp64}, report, depth buffers kept
    {iid: tensor})."""
    import torch
    from . import hip_ops
    S = default_stride(b.grid) if stride is None else int(stride)
    Ws, Hs = lattice_shape(b.grid, S)
    obs = torch.zeros(len(views), Ws * Hs, 4, device=b.device, dtype=torch.int16)
    kept, kept_bytes, ev_obs = {}, 0, []
    for k, view in enumerate(views):
        if not b.sees(view):                             # its plane stays 0: no pair, gain 1
            continue
        v, zbuf = b.view_zbuf(view)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip_ops.ortho_observe(b.cgrid, b.dsm, v, zbuf, S, b.border_px, b.occlusion_tol, obs[k])
        e1.record()
        ev_obs.append((e0, e1))
        nbytes = zbuf.numel() * 4
        if kept_bytes + nbytes <= zbuf_cache_bytes:
            kept[int(view["iid"])] = zbuf
            kept_bytes += nbytes
    pairs = candidate_pairs(obs)
    checked = hip_ops.OrthoPairs(pairs, len(views), b.device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    stats = hip_ops.ortho_pair_stats(obs, checked, max_diff_q)
    e1.record()
    stats = stats.cpu().numpy()
    torch.cuda.synchronize(b.device)
    g, before, after = solve_gains(pairs, stats, len(views), noise_sigma, gain_sigma, min_samples)
    gains = {int(view["iid"]): g[k] for k, view in enumerate(views)}
    report = dict(model="gain", noise_sigma=float(noise_sigma), gain_sigma=float(gain_sigma), stride=S, lattice=[Ws, Hs],
                  samples=Ws * Hs, max_diff_q=int(max_diff_q), min_samples=int(min_samples), pairs_candidate=int(pairs.shape[0]),
                  pairs_used=int((stats[:, 0] >= int(min_samples)).sum()), gains={str(i): [float(x) for x in gains[i]] for i in gains},
                  overlap_rms_before=[float(x) for x in before], overlap_rms_after=[float(x) for x in after],
                  observe_seconds=sum(x.elapsed_time(y) for x, y in ev_obs) / 1e3, pair_stats_seconds=e0.elapsed_time(e1) / 1e3)
    return gains, report, kept


def _sorted_views(views):
    views = sorted(views, key=lambda v: int(v["iid"]))
    ids = [int(v["iid"]) for v in views]
    if len(set(ids)) != len(ids):
        raise ValueError("two views share an image id")
    if len(views) > BAL_MAX_VIEWS:
        raise ValueError("%d views: the balance takes at most %d" % (len(views), BAL_MAX_VIEWS))
    return views


def balance_views(dsm, grid, views, occlusion_tol=None, border_px=2.0, stride=None, max_diff=255.0, noise_sigma=NOISE_SIGMA,
                  gain_sigma=GAIN_SIGMA, min_samples=64, zbuf_cache_bytes=ZBUF_CACHE_BYTES, device=None):
    """The gains that level the views' exposures over `dsm` on `grid` -> (gains {image id: [3] fp64}, report).  Per view, in
    ascending image id: the cull of add_view (a culled view gets gain 1), its depth buffer, its samples on the lattice of every
    stride-th DSM cell (default_stride by default); then the pairs of views that share a run of the lattice, their statistics
    (cells that differ by more than max_diff levels in a channel are left out; 255: none) and solve_gains."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("ortho: needs an MI355X (there is no CPU fallback for the orthophoto kernels)")
    stride, max_diff_q = check_balance_options("gain", noise_sigma, gain_sigma, stride, max_diff, min_samples, grid)
    b = OrthoBuilder(grid, 1, "best", dsm, occlusion_tol, border_px, device=device)
    gains, report, _ = _balance(b, _sorted_views(views), stride, max_diff_q, noise_sigma, gain_sigma, min_samples, zbuf_cache_bytes)
    return gains, report


def from_dsm(dsm, grid, views, upsample=1, mode="best", occlusion_tol=None, border_px=2.0, feather_px=64.0, device=None, balance=None,
             noise_sigma=NOISE_SIGMA, gain_sigma=GAIN_SIGMA, balance_stride=None, balance_max_diff=255.0, balance_min_samples=64,
             zbuf_cache_bytes=ZBUF_CACHE_BYTES):
    """A host DSM array [H, W] float32 on `grid` (dsm.Grid) and views as load_views gives them -> OrthoBuilder.finish()'s dict
    plus `seconds`.  balance="gain": the views' images are scaled by the gains of balance_views first, and the dict gains a
    `balance` block (its report, the rms colour step across the mosaic's seams and the seam pairs it is over)."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("ortho: needs an MI355X (there is no CPU fallback for the orthophoto kernels)")
    t0 = time.time()
    if balance is None:
        b = OrthoBuilder(grid, upsample, mode, dsm, occlusion_tol, border_px, feather_px, device)
        for v in sorted(views, key=lambda v: int(v["iid"])):
            b.add_view(v)
        res = b.finish()
        res["seconds"] = time.time() - t0
        return res
    from . import hip_ops
    stride, max_diff_q = check_balance_options(balance, noise_sigma, gain_sigma, balance_stride, balance_max_diff, balance_min_samples, grid)
    views = _sorted_views(views)
    b = OrthoBuilder(grid, upsample, mode, dsm, occlusion_tol, border_px, feather_px, device)
    gains, report, zbufs = _balance(b, views, stride, max_diff_q, noise_sigma, gain_sigma, balance_min_samples, zbuf_cache_bytes)
    ev_adj = []
    for v in views:
        iid = int(v["iid"])
        if not b.sees(v):
            b.add_view(v)                                # culled and reported as before
            continue
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        adjusted = hip_ops.ortho_adjust_image(v["rgba"], gains[iid])
        e1.record()
        ev_adj.append((e0, e1))
        b.add_view(dict(v, rgba=adjusted), zbuf=zbufs.get(iid))
    res = b.finish()
    seam = hip_ops.ortho_seam_stats(b.cgrid, b.mosaic[1], b.mosaic[0]).cpu().numpy()
    report["adjust_seconds"] = sum(x.elapsed_time(y) for x, y in ev_adj) / 1e3
    report["seam_pairs"] = int(seam[0])
    report["seam_rms"] = math.sqrt(float(seam[1:].sum()) / (3.0 * float(seam[0]))) if seam[0] > 0 else 0.0
    res["balance"] = report
    res["seconds"] = time.time() - t0
    return res


def seam_rms(res, device=None):
    """The rms colour step across the seams of a mosaic (finish()'s or from_dsm()'s dict) -> (rms, seam pairs)."""
    import torch
    from . import hip_ops
    dev = torch.device(device if device is not None else "cuda")
    g, K = res["dsm_grid"], res["upsample"]
    cgrid = hip_ops.ortho_grid(g.x0, g.y_top, g.gsd, g.W, g.H, K)
    s = hip_ops.ortho_seam_stats(cgrid, torch.from_numpy(np.ascontiguousarray(res["view"], np.int32)).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(res["rgba"], np.uint8)).to(dev)).cpu().numpy()
    return (math.sqrt(float(s[1:].sum()) / (3.0 * float(s[0]))) if s[0] > 0 else 0.0), int(s[0])


# ---- a predict output folder ------------------------------------------------------------------------------------------
def load_views(folder, device):
    """Every view of the folder with an image and a camera -> [dict(iid, K, R, C, rgba)] in ascending image id (depth maps are
    not read)."""
    import torch
    from PIL import Image
    views = []
    for iid in sorted(folder.images):
        base = folder.base(iid)
        if not all(os.path.exists(base + ext) for ext in (".txt", ".jpg")):
            continue
        _, K = fusion.read_cam_txt(base + ".txt")
        rgba = np.ascontiguousarray(np.array(Image.open(base + ".jpg").convert("RGBA")))
        R, C = fusion.pose(folder.images[iid])
        views.append(dict(iid=iid, K=K, R=R, C=C, rgba=torch.from_numpy(rgba).to(device)))
    return views


def read_dsm(prefix, filled=False):
    """-> (dsm [H, W] float32, dsm.Grid) from `<prefix>_dsm.json` and `<prefix>_dsm.tif` (`_dsm_filled.tif` if filled)."""
    from . import raster_stage
    grid = raster_stage.read_grid(prefix)
    tif = prefix + ("_dsm_filled.tif" if filled else "_dsm.tif")
    return raster_stage.read_raster(tif, np.float32, (grid.H, grid.W), says="%s_dsm.json says %d x %d" % (prefix, grid.H, grid.W)), grid


def output_paths(out):
    return dict(ortho=out + "_ortho_img.png", ortho_world=out + "_ortho_img.pgw", view=out + "_ortho_img_view.tif",
                nvis=out + "_ortho_img_nvis.tif", json=out + "_ortho_img.json")


def summary(res):
    g, dg = res["grid"], res["dsm_grid"]
    return dict(grid=dict(x0=g.x0, y_top=g.y_top, gsd=g.gsd, W=g.W, H=g.H), dsm_grid=dict(gsd=dg.gsd, W=dg.W, H=dg.H),
                upsample=res["upsample"], mode=res["mode"], occlusion_tol=res["occlusion_tol"], border_px=res["border_px"],
                feather_px=res["feather_px"], views_used=res["views_used"], views_culled=res["views_culled"],
                cells_surface=res["cells_surface"], cells_coloured=res["cells_coloured"], cells_unseen=res["cells_unseen"],
                seconds=res.get("seconds", 0.0), device_seconds=res["device_seconds"], **({"balance": res["balance"]} if "balance" in res else {}))


def write_outputs(out, res):
    """The orthophoto, its world file, the view and count rasters and the JSON summary at the prefix `out` -> output_paths(out)."""
    from PIL import Image
    paths = output_paths(out)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(res["rgba"], np.uint8)).save(paths["ortho"], format="PNG")
    Image.fromarray(np.ascontiguousarray(res["view"], np.int32)).save(paths["view"], format="TIFF")
    Image.fromarray(np.ascontiguousarray(res["nvis"], np.uint16)).save(paths["nvis"], format="TIFF")
    with open(paths["ortho_world"], "w") as f:
        f.write(world_file_text(res["grid"]))
    with open(paths["json"], "w") as f:
        json.dump(summary(res), f, indent=1)
        f.write("\n")
    return paths


def read_outputs(out):
    """-> (rgba uint8, view int32, nvis uint16) read back from the files of write_outputs."""
    from PIL import Image
    paths = output_paths(out)
    return (np.array(Image.open(paths["ortho"]).convert("RGBA")), np.array(Image.open(paths["view"])).astype(np.int32),
            np.array(Image.open(paths["nvis"])).astype(np.uint16))


def from_folder(data_folder, output_folder, dsm_prefix, filled=False, upsample=1, mode="best", occlusion_tol=None, border_px=2.0,
                feather_px=64.0, out=None, device=None, log=print, balance=None, noise_sigma=NOISE_SIGMA, gain_sigma=GAIN_SIGMA,
                balance_stride=None, balance_max_diff=255.0, balance_min_samples=64):
    """The whole chain step: read the DSM and the views, mosaic, write output_paths(out) -> from_dsm()'s dict.  balance and the
    options after it: see from_dsm."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("ortho: needs an MI355X (there is no CPU fallback for the orthophoto kernels)")
    check_upsample(upsample)
    check_options(mode, 0.0 if occlusion_tol is None else occlusion_tol, border_px, feather_px)
    t0 = time.time()
    dsm, grid = read_dsm(dsm_prefix, filled)
    ortho_grid(grid, upsample)
    if balance is not None:
        check_balance_options(balance, noise_sigma, gain_sigma, balance_stride, balance_max_diff, balance_min_samples, grid)
    device = torch.device(device if device is not None else "cuda")
    views = load_views(fusion.Folder(data_folder, output_folder), device)
    if not views:
        raise ValueError("%s: no view has both <name>.jpg and <name>.txt" % output_folder)
    res = from_dsm(dsm, grid, views, upsample, mode, occlusion_tol, border_px, feather_px, device, balance, noise_sigma, gain_sigma,
                   balance_stride, balance_max_diff, balance_min_samples)
    res["seconds"] = time.time() - t0
    write_outputs(dsm_prefix if out is None else out, res)
    g = res["grid"]
    log("ortho %d x %d cells at gsd %g (%s, upsample %d): %d views used, %d culled; %d of %d surface cells coloured, %d seen by no "
        "view; device %.3f s, total_time = %.3f s" % (g.W, g.H, g.gsd, mode, res["upsample"], len(res["views_used"]), len(res["views_culled"]),
                                                      res["cells_coloured"], res["cells_surface"], res["cells_unseen"], res["device_seconds"],
                                                      res["seconds"]))
    if "balance" in res:
        bal = res["balance"]
        log("balance (%s): stride %d, %d lattice cells, %d of %d candidate pairs used; overlap rms %s -> %s levels; seam rms %.2f levels "
            "over %d seam pairs" % (bal["model"], bal["stride"], bal["samples"], bal["pairs_used"], bal["pairs_candidate"],
                                    ["%.2f" % x for x in bal["overlap_rms_before"]], ["%.2f" % x for x in bal["overlap_rms_after"]],
                                    bal["seam_rms"], bal["seam_pairs"]))
    return res


def build_parser():
    ap = argparse.ArgumentParser(description="Mosaic the source images over a DSM into a true orthophoto")
    ap.add_argument("--data_folder", required=True, help="the whu-omvs data folder predict_whu.py read")
    ap.add_argument("--output_folder", required=True, help="predict_whu.py's output folder (its <vid>/<name>.jpg and .txt)")
    ap.add_argument("--dsm", required=True, metavar="PREFIX", help="the prefix dsm_whu.py --out was given")
    ap.add_argument("--filled", action="store_true", help="use <PREFIX>_dsm_filled.tif (dsm_whu.py --fill_max_dist)")
    ap.add_argument("--upsample", type=int, default=1, help="orthophoto cells per DSM cell along each axis (1 .. 8)")
    ap.add_argument("--mode", choices=sorted(MODES), default="best", help="best: the most nadir view that sees a cell; feather: a blend")
    ap.add_argument("--occlusion_tol", type=float, default=None, metavar="M", help="depth tolerance of the visibility test (default 2 gsd)")
    ap.add_argument("--border_px", type=float, default=2.0, help="samples closer than this to an image edge are not used")
    ap.add_argument("--feather_px", type=float, default=64.0, help="feather mode: the weight ramps up over this many pixels")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="output prefix (default: --dsm): <out>_ortho_img.png, ...")
    ap.add_argument("--balance", choices=list(BALANCE_MODELS), default=None,
                    help="level the views' exposures before the mosaic: gain = one gain per view and channel (default: off)")
    ap.add_argument("--gain_sigma", type=float, default=GAIN_SIGMA, help="balance: prior sigma of a gain about 1 (Brown & Lowe's 0.1)")
    ap.add_argument("--noise_sigma", type=float, default=NOISE_SIGMA, help="balance: sigma of a mean difference, levels (Brown & Lowe's 10)")
    ap.add_argument("--balance_stride", type=int, default=None, metavar="S",
                    help="balance: sample every S-th DSM cell (default: the smallest with at most 2^20 samples)")
    ap.add_argument("--balance_max_diff", type=float, default=255.0, metavar="LEVELS",
                    help="balance: leave out cells where two views differ by more than this in a channel (255: none)")
    ap.add_argument("--balance_min_samples", type=int, default=64, help="balance: common cells a pair of views needs to be used")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    return from_folder(args.data_folder, args.output_folder, args.dsm, args.filled, args.upsample, args.mode, args.occlusion_tol,
                       args.border_px, args.feather_px, args.out, balance=args.balance, noise_sigma=args.noise_sigma,
                       gain_sigma=args.gain_sigma, balance_stride=args.balance_stride, balance_max_diff=args.balance_max_diff,
                       balance_min_samples=args.balance_min_samples)


if __name__ == "__main__":
    main()
