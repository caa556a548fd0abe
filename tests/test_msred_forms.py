"""The MS-REDNet path per element against float64, in every form its launchers can take (csrc/msred.hip, the folded-prologue
variants of k_conv_dd_resident in csrc/costreg2d.hip and of k_conv_small in csrc/slice_red.hip).

tests/test_msrednet.py holds this model by means over whole maps against fp32; a wrong halo column of a recomputed window, a wrong
parity buffer on an odd plane count, a wrong last plane or a padding channel inside a GroupNorm population moves such a mean by far
less than its bar.  Here every op is compared with a float64 reference (oracle/msrednet_oracle.py, tests/msred_ref.py) through
fp64_bars.check, with the RED_ bars of tests/fp64_bars.py, and every path of the two recurrence entry points is chosen on purpose:
the case ids name the path the launcher's rule gives (`pair_path`, `split_path` below restate it).
"""
import math

import pytest
import torch

import ada_mvs_amd  # noqa: F401
import fp64_bars
import msred_ref
from ada_mvs_amd import synth
from oracle import msrednet_oracle as mo

pytestmark = pytest.mark.gpu

HC = msred_ref.HC
RW = (16, 32, 64, 64)          # width of the stored GRU outputs (slice_RED_Regularization.RW)
PAD = 7.0                      # what the pad channels of an output hold before a call, and must hold after it
PLANE_DIMS = ("plane", "n", "c", "y", "x")


def _cl(x):
    """[B,C,h,w] -> channel-last [B,h*w,C] on the GPU"""
    B, C, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(B, h * w, C).contiguous().cuda()


def _nchw(x_cl, h, w):
    B, _, C = x_cl.shape
    return x_cl.reshape(B, h, w, C).permute(0, 3, 1, 2).cpu()


def _held(got, ref, bars, what, scale=None, dims=None):
    """fp64_bars.check with the figures printed first (pytest -s shows them whether the case passes or not)."""
    e = (got.detach().cpu().double() - ref).abs()
    print("measured %s: max|err| / scale %.3e, mean|err| / mean|ref| %.3e"
          % (what, float(e.max()) / max(scale if scale is not None else float(ref.abs().max()), 1e-30),
             float(e.mean() / ref.abs().mean().clamp_min(1e-30))))
    mx, mean = bars if isinstance(bars, tuple) else (bars, None)
    return fp64_bars.check(got, ref, mx, mean, scale=scale, what=what, dims=dims)


# ---------------------------------------------------------------------------------------------------------------------------
# which path a recurrence takes: the launchers' rule restated (csrc/kernels.h::gn_epilogue_partials, ::gru_fold_enabled,
# csrc/slice_red.hip::launch_conv_pair, csrc/costreg2d.hip::resident_rows, ::can_fold_gru_applies)
# ---------------------------------------------------------------------------------------------------------------------------
def _epilogue_partials(parts, B):
    return 0 < parts <= 2048 and parts * B <= 4096


def _fold(fold, B):
    return fold != 0 if fold >= 0 else B <= 2


def pair_path(B, h, w, fold):
    parts = math.ceil(w / 16) * math.ceil(h / 4) * 4                 # 4 x 16 tiles, one partial per wave
    if not _epilogue_partials(parts, B):
        return "gn_partial"
    return "folded" if _fold(fold, B) else "epilogue"


def resident_rows(level, B, h, w, grid):
    """NTR of k_conv_dd_resident: the fewest rows per workgroup whose grid stays within conv_small_grid; 0: the generic k_conv_dd."""
    wn = 4 // (HC[level - 1] // 16)
    for ntr in (1, 2, 4):
        if math.ceil(w / 16) * B * math.ceil(h / (ntr * wn)) <= grid:
            return ntr
    return 0


def split_path(level, B, h, w, fold, grid):
    ntr = resident_rows(level, B, h, w, grid)
    wn = 4 // (HC[level - 1] // 16)
    parts = math.ceil(w / 16) * math.ceil(h / (ntr * wn)) * 4 if ntr else 0
    if not _epilogue_partials(parts, B):
        return "gn_partial-" + ("single_ntr%d" % ntr if ntr else "generic")
    return ("folded" if _fold(fold, B) else "epilogue") + "-dual_ntr%d" % ntr


def grid_for(level, B, h, w, ntr):
    """The conv_small_grid value at which exactly `ntr` rows are the fewest that fit."""
    wn = 4 // (HC[level - 1] // 16)
    grid = math.ceil(w / 16) * B * math.ceil(h / (ntr * wn))
    assert resident_rows(level, B, h, w, grid) == ntr, (level, B, h, w, ntr)
    return grid


# ---------------------------------------------------------------------------------------------------------------------------
# a. adamvs_red_recur_pair
# ---------------------------------------------------------------------------------------------------------------------------
def _packed(sd, C):
    from ada_mvs_amd import packing
    flat, off = packing.pack_red_regularization(sd, "", C)
    return flat.cuda(), off


def run_pair(level, C, sd, xs, B, h, w):
    """-> R [D*B, h*w, RW] on the CPU, every element PAD before the call."""
    from ada_mvs_amd import hip_ops
    flat, off = _packed(sd, C)
    hc, cx, D = HC[level - 1], xs[0].shape[1], len(xs)

    def wp(name):
        o, rows = off[name]
        n = rows * 9 * (cx + hc)
        return flat[o:o + n], flat[o + n:o + n + rows]
    wg, bg = wp("gp%d" % level)
    wc, bc = wp("cp%d" % level)
    o, n = off["gn%d" % level]
    assert n == hc
    R = torch.full((D * B, h * w, RW[level - 1]), PAD, device="cuda")
    hip_ops.red_recur_pair(torch.cat([_cl(x) for x in xs], 0), wg, bg, wc, bc, flat[o:o + 6 * hc], R, B, h, w, hc)
    torch.cuda.synchronize()
    return R.cpu()


def run_split(level, sd, xs, B, h, w):
    from ada_mvs_amd import hip_ops
    flat, off = _packed(sd, 32)
    hc, D = HC[level - 1], len(xs)
    blocks = []
    for name in ("ghr", "ghu", "ch"):
        o, W = off["%s%d" % (name, level)]
        assert W == hc
        blocks.append(flat[o:o + 9 * W * W + W])
    o, n = off["gn%d" % level]
    R = torch.full((D * B, h * w, RW[level - 1]), PAD, device="cuda")
    gxr, gxu, cx = (torch.cat([_cl(x[k]) for x in xs], 0) for k in range(3))
    hip_ops.red_recur_split(gxr, gxu, cx, blocks[0], blocks[1], blocks[2], flat[o:o + 6 * hc], R, B, h, w, hc)
    torch.cuda.synchronize()
    return R.cpu()


def _states(R, level, B, h, w):
    """R [D*B, npix, RW] -> [D, B, HC, h, w]"""
    hc = HC[level - 1]
    return R[:, :, :hc].reshape(-1, B, h, w, hc).permute(0, 1, 4, 2, 3)


def _reference(level, sd, xs):
    return torch.stack(msred_ref.recurrence(level, msred_ref.to_dtype(xs, torch.float64), fp64_bars.double_sd(sd)))


def _check_recurrence(R, level, sd, xs, B, h, w, bars, what):
    hc = HC[level - 1]
    _held(_states(R, level, B, h, w), _reference(level, sd, xs), bars, what, dims=PLANE_DIMS)
    assert bool((R[:, :, hc:] == PAD).all()), what + ": pad channels of R written"


def _pair_cases():
    c = []
    for level, C in ((1, 32), (1, 16), (1, 8), (2, 16)):            # (CA, CB, NT) = (C, 8, 1) x 3 and (16, 16, 2 | 1): five instantiations
        for fold in (1, 0):
            c.append((level, C, 2, 37, 53, 3, fold))                # ragged in both directions, both parities and the last plane
            c.append((level, C, 1, 2, 3, 2, fold))                  # less than one 4 x 16 tile
        c.append((level, C, 3, 37, 53, 2, -1))                      # three samples: unfolded by default
        c.append((level, C, 3, 21, 35, 3, 1))                       # ... and the fold forced
    for level in (1, 2):
        for fold in (1, 0):
            c.append((level, 32 if level == 1 else 16, 1, 1, 1, 1, fold))       # one pixel, one plane: no GRU_PRO_OUT launch at all
            c.append((level, 32 if level == 1 else 16, 2, 1, 18, 8, fold))      # one row, two tiles; eight planes
        c.append((level, 16, 1, 21, 35, 9, -1))
    # the partial buffer's boundaries: one case on each side (plane counts 2: both launches of the folded form, both parities)
    c += [(1, 32, 1, 128, 256, 2, -1), (1, 32, 1, 128, 256, 2, 0), (1, 32, 1, 132, 256, 2, -1), (1, 8, 2, 128, 256, 3, -1),
          (2, 16, 3, 84, 256, 2, -1), (2, 16, 3, 84, 256, 2, 1), (2, 16, 3, 88, 256, 2, 1)]
    # more 4 x 16 tiles (2112) than a persistent grid can hold (at most 8 workgroups on each of 256 CUs): the tile loop wraps
    c += [(1, 16, 3, 176, 256, 2, -1), (2, 16, 3, 176, 256, 1, -1)]
    return c


def _pair_id(c):
    level, C, B, h, w, D, fold = c
    return "L%d-C%d-B%d-%dx%d-D%d-fold%d-%s" % (level, C, B, h, w, D, fold, pair_path(B, h, w, fold))


@pytest.mark.parametrize("level,C,B,h,w,D,fold", _pair_cases(), ids=[_pair_id(c) for c in _pair_cases()])
def test_red_recur_pair(set_option, level, C, B, h, w, D, fold):
    """adamvs_red_recur_pair, every plane of R per element against msred_ref.recurrence in float64: every supported pairing, each of
    the three paths on both sides of the partial buffer's boundaries, folded and unfolded on the same inputs, one to nine planes,
    maps smaller than a tile, ragged ones and two whose tiles outnumber any persistent grid.  RW is wider than HC at both levels:
    the pad channels of R keep what they held.

    The tile loop of the persistent kernels wraps where a case has more 4 x 16 tiles than workgroups stay resident.  By the grid
    bound alone (8 workgroups on each of 256 CUs) only the k_gn_partial path can be that large: the two 176 x 256 cases have 2112
    tiles.  In fact the kernels' occupancy is lower, and the kernel trace shows the grids: k_conv_small runs 1024 (<16, 8, 1>),
    768 (<16, 16, 1>) and 512 (<16, 16, 2>, <32, 8, 1>) workgroups there, so the 132 x 256, 88 x 256 and 84 x 256 cases wrap as
    well.  The folded kernel wraps too, in two cases: a map with epilogue partials has at most 1024 tiles over its samples, and
    k_conv_small_pro<8, 8, 1> runs the two samples of 128 x 256 (1024 tiles) on 768 workgroups, k_conv_small_pro<16, 16, 2> /
    <16, 16, 1> the three samples of 84 x 256 (1008 tiles) on 256 / 512; the one sample of 128 x 256 (512 tiles on 512 workgroups
    of <32, 8, 1>) and every smaller folded case run one tile per workgroup.

    The path in each id is what `pair_path` gives.  A kernel trace (rocprofv3 --kernel-trace --stats, one run per path label over
    the cases whose id carries it) confirmed the labels: k_conv_small_pro in all five (CA, CB, NT) instantiations and
    k_gru2_last_apply only in the cases labelled folded, where no k_gru2_gates_apply / k_gru2_out_apply / k_gn_partial ran (the
    plain k_conv_small appears there once per case, for the gate convolution of the first plane, which has no prologue);
    k_conv_small with k_gru2_gates_apply / k_gru2_out_apply and no k_gn_partial in those labelled epilogue; k_gn_partial (two
    launches per plane) only in those labelled gn_partial."""
    set_option("red_fold_applies", fold)
    sd, xs = msred_ref.recur_inputs(level, C, B, h, w, D)
    R = run_pair(level, C, sd, xs, B, h, w)
    _check_recurrence(R, level, sd, xs, B, h, w, fp64_bars.RED_PAIR, "red_recur_pair " + _pair_id((level, C, B, h, w, D, fold)))


# ---------------------------------------------------------------------------------------------------------------------------
# b. adamvs_red_recur_split
# ---------------------------------------------------------------------------------------------------------------------------
def _split_cases():
    c = []
    for level in (3, 4):
        big = {3: ((80, 256), (160, 256)), 4: ((40, 256), (80, 256))}[level]
        # the default limit on the sizes that reach the larger NTR with epilogue partials (two samples, 1280 partials each)
        c += [(level, 2) + big[0] + (2, -1, 1024), (level, 2) + big[0] + (2, 0, 1024), (level, 2) + big[1] + (2, -1, 1024)]
        c.append((level, 1, {3: 100, 4: 50}[level], 256, 2, -1, 1024))      # 3200 partials: k_gn_partial, the resident kernel single
        for ntr in (1, 2, 4):                                               # a lowered limit on a ragged map
            for fold in (1, 0):
                c.append((level, 2, 37, 53, 3, fold, grid_for(level, 2, 37, 53, ntr)))
        c.append((level, 2, 37, 53, 3, -1, 0))                              # the generic k_conv_dd on the same inputs
        c += [(level, 3, 37, 53, 3, -1, 1024), (level, 3, 37, 53, 3, 1, 1024), (level, 1, 21, 35, 9, -1, 1024)]
        for h, w, D in ((1, 1, 1), (2, 3, 2), (1, 18, 3)):
            for fold in (1, 0):
                c.append((level, 1, h, w, D, fold, 1024))
        c.append((level, 1, 2, 3, 2, -1, 0))
    return c


def _split_id(c):
    level, B, h, w, D, fold, grid = c
    return "L%d-B%d-%dx%d-D%d-fold%d-grid%d-%s" % (level, B, h, w, D, fold, grid, split_path(level, B, h, w, fold, grid))


@pytest.mark.parametrize("level,B,h,w,D,fold,grid", _split_cases(), ids=[_split_id(c) for c in _split_cases()])
def test_red_recur_split(set_option, level, B, h, w, D, fold, grid):
    """adamvs_red_recur_split (W = HC = 32 and 64), every plane of R per element against msred_ref.recurrence in float64; the x
    halves are random maps that the reference adds as the Wx.x + b term.  k_conv_dd_resident<D, NTR, DUAL> at NTR = 1, 2 and 4,
    the gate pair (DUAL) and the candidate (single), with the GRU prologues (folded) and without: at the default conv_small_grid
    on the sizes that reach the larger NTR, and through a lowered limit on a ragged map; conv_small_grid = 0 is the generic
    k_conv_dd with every reduction a launch of its own.

    The path and NTR in each id are what `split_path` gives.  A kernel trace (rocprofv3 --kernel-trace --stats, one run per label
    over the cases whose id carries it) confirmed them: every "dual_ntrN" selection ran k_conv_dd_resident<32 | 64, N, true> and
    <32 | 64, N, false> and no other NTR; the folded ones ran k_gru2_last_apply and none of k_gru2_gates_apply / k_gru2_out_apply /
    k_gn_partial, the epilogue ones the two apply kernels without k_gn_partial; "gn_partial-single_ntr1" ran only the single
    <32 | 64, 1, false> kernel (three launches per plane) with k_gn_partial; "gn_partial-generic" ran k_conv_dd<2, 1> / <4, 1>
    with k_gn_partial and no resident kernel.  These kernels are not persistent (one workgroup per tile): nothing wraps."""
    set_option("red_fold_applies", fold)
    set_option("conv_small_grid", grid)
    sd, xs = msred_ref.recur_inputs(level, 32, B, h, w, D)
    R = run_split(level, sd, xs, B, h, w)
    _check_recurrence(R, level, sd, xs, B, h, w, fp64_bars.RED_SPLIT, "red_recur_split " + _split_id((level, B, h, w, D, fold, grid)))


@pytest.mark.parametrize("level", [1, 2, 3, 4])
def test_recurrence_paths_by_their_bits(set_option, level):
    """Which path ran is a property of the launcher, not of the output -- except in the last bits.  On one ragged map at two and at
    three samples: red_fold_applies = -1 equals the forced arm of its side bit for bit (folded up to two samples, unfolded from
    three).  The folded form is the same arithmetic in the same order as the unfolded one -- it recomputes sigmoid / tanh / GroupNorm
    in the next convolution's window fill from the same partial sums, finished in the same order, and blends with the same
    expression as the elementwise kernels -- and so is k_conv_dd_resident at NTR = 1, 2 and 4 (a pixel's chunks and taps in one
    order, the partial sums in double): all of these agree bit for bit, asserted here, and only the kernel trace tells them apart.
    The generic k_conv_dd (conv_small_grid = 0) sums a pixel's chunks in another order than the resident kernel: its bits differ, so
    a case that silently took the other of those two would fail here."""
    h, w, D = 37, 53, 3
    facts = {}
    for B in (2, 3):
        sd, xs = msred_ref.recur_inputs(level, 32 if level != 2 else 16, B, h, w, D)
        outs = {}
        for fold in (-1, 0, 1):
            set_option("red_fold_applies", fold)
            outs[fold] = run_pair(level, 32 if level == 1 else 16, sd, xs, B, h, w) if level < 3 else run_split(level, sd, xs, B, h, w)
        assert torch.equal(outs[-1], outs[1 if B <= 2 else 0]), "B=%d: the default is not the forced arm of its side" % B
        facts["B%d folded == unfolded" % B] = torch.equal(outs[0], outs[1])
        if level >= 3:
            set_option("conv_small_grid", 0)
            set_option("red_fold_applies", 0)
            generic = run_split(level, sd, xs, B, h, w)
            facts["B%d generic == resident" % B] = torch.equal(generic, outs[0])
            for ntr in (2, 4):
                set_option("conv_small_grid", grid_for(level, B, h, w, ntr))
                facts["B%d ntr%d == ntr1" % (B, ntr)] = torch.equal(run_split(level, sd, xs, B, h, w), outs[0])
            set_option("conv_small_grid", 1024)
    print("measured bits, level %d: %s" % (level, facts))
    for k, same in facts.items():
        assert same == ("generic" not in k), k


# ---------------------------------------------------------------------------------------------------------------------------
# c. the elementwise kernels and the GroupNorm statistics on their own
# ---------------------------------------------------------------------------------------------------------------------------
def _gn64(x, weight, bias, eps=1e-5):
    """GroupNorm(1 group) of [N, npix, HC] in float64"""
    mean = x.mean(dim=(1, 2), keepdim=True)
    var = x.var(dim=(1, 2), unbiased=False, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


@pytest.mark.parametrize("layout", ["halves_of_one_map", "two_maps"])
def test_gru2_applies_per_element(layout):
    """k_gru2_gates_apply and k_gru2_out_apply on their own, per element against float64, at Wf != W != HC and a thread count
    (npix * HC / 4) that is not a multiple of 256; fr / fu as views of the two halves of one map and as two separate maps.  The pad
    channels of rh, h and out keep what they held."""
    from ada_mvs_amd import hip_ops
    N, npix = 3, 37 * 11
    hc, W, Wf, Wo = (12, 16, 24, 32) if layout == "halves_of_one_map" else (8, 16, 32, 24)
    assert (npix * hc // 4) % 256 and len({hc, W, Wf}) == 3
    g = torch.Generator().manual_seed(hc)
    f = torch.randn(N, npix, 2 * Wf, generator=g) * 1.5 + 0.3
    gn = torch.randn(6, hc, generator=g) * 0.3 + torch.tensor([1.0, 0, 1, 0, 1, 0]).reshape(6, 1)
    h0 = torch.tanh(torch.randn(N, npix, hc, generator=g))
    if layout == "halves_of_one_map":
        fm = f[:, :, :Wf].contiguous().cuda()
        fr, fu = fm[:, :, :hc], fm[:, :, hc:2 * hc]
    else:
        fr, fu = f[:, :, :Wf].contiguous().cuda(), f[:, :, Wf:].contiguous().cuda()
    state = torch.full((N, npix, W), PAD)
    state[:, :, :hc] = h0
    state = state.cuda()
    rh, u = torch.full((N, npix, W), PAD, device="cuda"), torch.zeros(N, npix, hc, device="cuda")
    part = hip_ops.group_stats_workspace(N, 2, fr.device)
    hip_ops.group_stats_partial(fr, fu, hc, part)
    hip_ops.gru2_gates_apply(fr, fu, part, gn.reshape(-1).cuda(), state, rh, u, hc)
    fr64, fu64, g64, h64 = fr.cpu().double()[:, :, :hc], fu.cpu().double()[:, :, :hc], gn.double(), h0.double()
    r = torch.sigmoid(_gn64(fr64, g64[0], g64[1]))
    uu = torch.sigmoid(_gn64(fu64, g64[2], g64[3]))
    dims = ("n", "pixel", "c")
    _held(rh[:, :, :hc], r * h64, fp64_bars.RED_APPLY, "gates_apply r*h (%s)" % layout, dims=dims)
    _held(u, uu, fp64_bars.RED_APPLY, "gates_apply u (%s)" % layout, dims=dims)
    assert bool((rh[:, :, hc:] == PAD).all())
    o = torch.full((N, npix, W), PAD)
    o[:, :, :hc] = torch.randn(N, npix, hc, generator=g) * 2 - 0.5
    o = o.cuda()
    out = torch.full((N, npix, Wo), PAD, device="cuda")
    hip_ops.group_stats_partial(o, None, hc, part)
    hip_ops.gru2_out_apply(o, part, gn[4:].reshape(-1).cuda(), u, state, out, hc)
    u64 = u.cpu().double()                                             # the kernel's own u: this step on its own
    want = u64 * h64 + (1 - u64) * torch.tanh(_gn64(o.cpu().double()[:, :, :hc], g64[4], g64[5]))
    _held(state[:, :, :hc], want, fp64_bars.RED_APPLY, "out_apply h (%s)" % layout, dims=dims)
    assert torch.equal(out[:, :, :hc], state[:, :, :hc]) and bool((out[:, :, hc:] == PAD).all()) and bool((state[:, :, hc:] == PAD).all())


def _group_stats(x0, x1, n):
    from ada_mvs_amd import hip_ops
    N, npix = x0.shape[:2]
    part = hip_ops.group_stats_workspace(N, 2 if x1 is not None else 1, x0.device)
    hip_ops.group_stats_partial(x0, x1, n, part)
    return hip_ops.group_stats_finish(part, N, 2 if x1 is not None else 1, npix, n).cpu().double()


def _stats64(x, n):
    sel = x.cpu().double()[:, :, :n]
    return sel.mean(dim=(1, 2)), 1.0 / torch.sqrt(sel.var(dim=(1, 2), unbiased=False) + 1e-5)


@pytest.mark.parametrize("case", ["constant", "mean_1e3_std_1e-2", "pad_channels_nonzero"])
def test_group_stats_edges(case):
    """k_gn_partial / gn_finish where E[x^2] - E[x]^2 is delicate: a constant map (variance 0: the fmax(., 0) clamp, rstd =
    1 / sqrt(eps)); mean 1e3 with standard deviation 1e-2; n < D with large values in the channels [n, D), which must not enter
    the population.

    Bars: the sums are in double, so mean and rstd are the float32 roundings (2^-24 each way, 1.2e-7 allowed) of values whose own
    error is the cancellation in q / count - mean^2: a few 2^-53 relative on terms of size mean^2, i.e. (mean^2 / var) * 2^-52 on
    the variance and half of that on rstd.  For mean 1e3, std 1e-2 that is 1e10 * 2.2e-16 / 2 = 1.1e-6 per rounding; four roundings
    (two sums, a division, a product) give the 4.5e-6 asserted there.  The other two cases have mean^2 / (var + eps) < 1e7, under
    1e-9, and are held to the float32 rounding alone."""
    g = torch.Generator().manual_seed(11)
    N, npix, D, n = 3, 37 * 11, 16, 8
    if case == "constant":
        x = torch.full((N, npix, D), 3.25)
        rbar = 1.2e-7
    elif case == "mean_1e3_std_1e-2":
        x = 1e3 + 1e-2 * torch.randn(N, npix, D, generator=g)
        rbar = 1.2e-7 + 4 * 1.1e-6
    else:
        x = torch.randn(N, npix, D, generator=g) * 0.7 + 0.2
        x[:, :, n:] = 1e4 * (1 + torch.rand(N, npix, D - n, generator=g))
        rbar = 1.2e-7
    x1 = -2 * x
    stats = _group_stats(x.cuda(), x1.cuda(), n)
    for gi, xx in enumerate((x, x1)):
        mean, rstd = _stats64(xx, n)
        em = float(((stats[:, gi, 0] - mean).abs() / mean.abs()).max())
        er = float(((stats[:, gi, 1] - rstd).abs() / rstd).max())
        print("measured group_stats %s group %d: mean rel %.3e, rstd rel %.3e" % (case, gi, em, er))
        assert em < 1.2e-7 and er < rbar, (case, gi, em, er)
    if case == "constant":
        assert float(stats[0, 0, 1]) == pytest.approx(1e-5 ** -0.5, rel=1.2e-7)


@pytest.mark.parametrize("npix", [64 * 2048, 64 * 2048 + 1, 2048 * 2048, 2048 * 2048 + 1])
def test_group_stats_at_the_ends_of_gn_parts(npix):
    """gn_parts(npix) = ceil(npix / 2048) clamped to [64, 2048]: 131072 pixels are the last map on 64 ranges, 131073 the first on
    65; 2048 x 2048 pixels the last that is not clamped to 2048 ranges, one more the first that is.  Ragged last ranges; mean and
    rstd to float32 rounding (sums in double; mean^2 / var is about 0.1 here)."""
    g = torch.Generator().manual_seed(npix % 1000)
    x = (torch.randn(1, npix, 4, generator=g) * 2 + 0.7)
    x[0, -1] = 50.0                                                  # the last pixel is in the population
    stats = _group_stats(x.cuda(), None, 4)
    mean, rstd = _stats64(x, 4)
    em, er = float((stats[0, 0, 0] - mean[0]).abs() / mean[0].abs()), float((stats[0, 0, 1] - rstd[0]).abs() / rstd[0])
    print("measured group_stats npix %d: mean rel %.3e, rstd rel %.3e" % (npix, em, er))
    assert em < 1.2e-7 and er < 1.2e-7, (em, er)


# ---------------------------------------------------------------------------------------------------------------------------
# d. adamvs_red_variance_cost
# ---------------------------------------------------------------------------------------------------------------------------
def _variance_id(c):
    kind, C, S, B, h, w, negate, Da, with_b = c
    sweep = negate and S <= 8 and B * h * w >= 65536
    return "%s-C%d-S%d-B%d-%dx%d-%s-Da%d-%s-%s" % (kind, C, S, B, h, w, "neg" if negate else "pos", Da, "b" if with_b else "nob",
                                                 "sweep" if sweep else "plain")


VARIANCE_CASES = [
    # the plain kernel: every width, view counts on both sides of 8, both signs, wide and compact outputs, an odd width
    ("rig8", 8, 1, 2, 24, 41, True, 16, True), ("rig8", 16, 4, 2, 24, 41, True, 32, False), ("rig8", 32, 8, 1, 23, 40, False, 32, True),
    ("rig150", 16, 9, 2, 24, 41, True, 16, True), ("rig150", 32, 4, 2, 24, 40, False, 48, False),
    ("border", 8, 4, 2, 24, 41, True, 16, True), ("border", 16, 1, 1, 24, 40, False, 16, False), ("border", 32, 8, 2, 17, 33, True, 32, True),
    # B*h*w = 65536 exactly: the sweep form; one row less, positive sign or nine views: the plain kernel on the same size
    ("rig8", 16, 4, 2, 128, 256, True, 32, True), ("rig8", 16, 4, 2, 127, 256, True, 32, True), ("rig8", 16, 4, 2, 128, 256, False, 32, True),
    ("rig150", 8, 8, 2, 128, 256, True, 16, False), ("rig150", 32, 1, 1, 256, 256, True, 48, True), ("rig150", 16, 9, 2, 128, 256, True, 16, True),
    ("border", 32, 4, 2, 128, 256, True, 32, True), ("border", 8, 8, 1, 255, 257, True, 8, False), ("border", 16, 8, 2, 128, 256, True, 16, True),
]


@pytest.mark.parametrize("kind,C,S,B,h,w,negate,Da,with_b", VARIANCE_CASES, ids=[_variance_id(c) for c in VARIANCE_CASES])
def test_red_variance_cost_per_element(kind, C, S, B, h, w, negate, Da, with_b):
    """adamvs_red_variance_cost per element against oracle.variance_cost in float64: the plain kernel and the register-resident-tap
    sweep (negate, S <= 8, C in 8 / 16 / 32, B*h*w >= 65536) on either side of each of those conditions, Da > C with and without the
    compact second output (pad channels untouched), odd widths, taps inside the image, leaving it, exactly on the last row and
    column, and a view with every tap outside.  The two kernels sum in different orders: no bit equality, one bar per geometry."""
    from ada_mvs_amd import hip_ops
    feats, proj, planes = msred_ref.variance_inputs(kind, C, S + 1, B, h, w)
    D = planes.shape[1]
    a = torch.full((D * B, h * w, Da), PAD, device="cuda")
    b = torch.full((D * B, h * w, C), PAD, device="cuda") if with_b else None
    feat_cl = torch.cat([_cl(f) for f in feats], 0)
    hip_ops.red_variance_cost(feat_cl, hip_ops.relative_transforms(proj.cuda()), planes.reshape(B, D, h * w).cuda(), a, b, B, S, C, D, h, w,
                              negate=negate)
    p64 = proj.double()
    rel = [mo.ao.relative_transform(p64[:, v], p64[:, 0]) for v in range(1, S + 1)]
    f64 = [f.double() for f in feats]
    want = torch.stack([mo.variance_cost(f64[0], f64[1:], [r[0] for r in rel], [r[1] for r in rel], planes[:, d:d + 1].double())
                        for d in range(D)]) * (-1.0 if negate else 1.0)
    what = "variance " + _variance_id((kind, C, S, B, h, w, negate, Da, with_b))
    got = a[:, :, :C].reshape(D, B, h, w, C).permute(0, 1, 4, 2, 3)
    _held(got, want, fp64_bars.RED_VARIANCE[(kind, "large" if B * h * w >= 65024 else "small")], what, dims=PLANE_DIMS)
    assert bool((a[:, :, C:] == PAD).all()), what + ": pad channels written"
    if with_b:
        assert torch.equal(b, a[:, :, :C]), what + ": the compact output differs from the wide one"


# ---------------------------------------------------------------------------------------------------------------------------
# e. adamvs_soft_argmin
# ---------------------------------------------------------------------------------------------------------------------------
RANGES = [[400.0, 600.0], [380.0, 650.0]]


@pytest.mark.parametrize("D", [1, 8, 64, 192])
def test_soft_argmin_per_pixel(D):
    """k_soft_argmin per pixel against float64: two batch items with different depth ranges, h*w = 273 (not a multiple of 256),
    logits of a trained network's range (one dominant +60, rows at a -60 floor).  Depth in hypothesis intervals of sample 0,
    confidence absolute, as STAGE_DEPTH / STAGE_CONF."""
    from ada_mvs_amd import hip_ops
    B, h, w = 2, 13, 21
    vol = msred_ref.trained_range_logits(B, D, h, w, seed=D)
    planes, interval = msred_ref.uniform_planes(RANGES, D, h, w)
    depth, conf = hip_ops.soft_argmin(vol.reshape(B, D, h * w).cuda(), planes.cuda(), B, D, h, w)
    rd, rc = msred_ref.soft_argmin(vol.double(), planes.double())
    _held(depth, rd, fp64_bars.RED_SOFT_DEPTH[D], "soft_argmin depth D=%d" % D, scale=interval)
    _held(conf, rc, fp64_bars.RED_SOFT_CONF, "soft_argmin confidence D=%d" % D, scale=1.0)


def test_soft_argmin_overflow_pattern():
    """The reference has no max subtraction: logits above ln(FLT_MAX) = 88.72 overflow its exp, and the inf / NaN that follow are
    its output.  The kernel gives the same pattern pixel for pixel as the fp32 oracle: one logit of 95 (E, A, M infinite: depth and
    confidence NaN), two of 88.5 (each finite, their sum not: confidence 0, depth NaN), one of 87 (finite sum; the depth-weighted
    sum overflows: depth inf), and ordinary pixels, which stay under the finite bars."""
    from ada_mvs_amd import hip_ops
    B, D, h, w = 2, 8, 13, 21
    vol = torch.randn(B, D, h, w, generator=torch.Generator().manual_seed(3)) * 3
    vol[:, 2, ::4, ::3] = 95.0
    vol[:, 1, 1::4, ::3] = 88.5
    vol[:, 6, 1::4, ::3] = 88.5
    vol[:, 5, 2::4, 1::3] = 87.0
    planes, interval = msred_ref.uniform_planes(RANGES, D, h, w)
    depth, conf = hip_ops.soft_argmin(vol.reshape(B, D, h * w).cuda(), planes.cuda(), B, D, h, w)
    depth, conf = depth.cpu(), conf.cpu()
    od, oc = msred_ref.soft_argmin(vol, planes)                       # the fp32 oracle
    assert bool(od.isnan().any()) and bool(od.isinf().any()) and bool((oc == 0).any()) and bool(od.isfinite().any())
    for name, got, want in (("depth", depth, od), ("confidence", conf, oc)):
        assert torch.equal(got.isnan(), want.isnan()), name + ": NaN pattern"
        assert torch.equal(got.isinf(), want.isinf()) and torch.equal(got[want.isinf()], want[want.isinf()]), name + ": inf pattern"
    assert torch.equal(conf == 0, oc == 0)
    plain = vol.amax(1) < 80                                          # pixels without an overflowing logit: the finite bars hold there
    assert bool(od[plain].isfinite().all()) and int(plain.sum()) > 100
    rd, rc = msred_ref.soft_argmin(vol.double(), planes.double())
    _held(depth[plain], rd[plain], fp64_bars.RED_SOFT_DEPTH[8], "soft_argmin depth, ordinary pixels", scale=interval, dims=("i",))
    _held(conf[plain], rc[plain], fp64_bars.RED_SOFT_CONF, "soft_argmin confidence, ordinary pixels", scale=1.0, dims=("i",))


# ---------------------------------------------------------------------------------------------------------------------------
# f. adamvs_channel_copy, planes_to_volume
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("n,c0s,c0d,Ds,Dd,shift", [(8, 4, 8, 16, 32, 0),        # every count a multiple of 4, 16-byte base: f32x4
                                                   (16, 0, 0, 16, 16, 0),       # whole maps
                                                   (8, 4, 8, 16, 32, 1),        # the same from a 4-byte-aligned base: scalar
                                                   (3, 1, 2, 7, 9, 0),          # nothing a multiple of 4
                                                   (4, 2, 4, 16, 16, 0),        # one offset not a multiple of 4
                                                   (4, 4, 4, 18, 16, 0),        # one pixel stride not a multiple of 4
                                                   (6, 4, 8, 16, 16, 0)])       # the count not a multiple of 4
def test_channel_copy_exact(N, n, c0s, c0d, Ds, Dd, shift):
    """adamvs_channel_copy in its f32x4 and scalar forms: exactly torch's slicing, everything else in dst untouched."""
    from ada_mvs_amd import hip_ops
    npix = 37 * 11
    g = torch.Generator().manual_seed(n + Ds)
    src_h, dst_h = torch.randn(N * npix * Ds + shift, generator=g), torch.randn(N * npix * Dd + shift, generator=g)
    src_d, dst_d = src_h.cuda(), dst_h.cuda()
    src, dst = src_d[shift:].view(N, npix, Ds), dst_d[shift:].view(N, npix, Dd)
    assert src.data_ptr() % 16 == 4 * shift and dst.data_ptr() % 16 == 4 * shift
    hip_ops.channel_copy(src, c0s, dst, c0d, n)
    want = dst_h[shift:].view(N, npix, Dd).clone()
    want[:, :, c0d:c0d + n] = src_h[shift:].view(N, npix, Ds)[:, :, c0s:c0s + n]
    assert torch.equal(dst.cpu(), want)
    assert torch.equal(dst_d[:shift].cpu(), dst_h[:shift])


@pytest.mark.parametrize("B,D,Ws", [(1, 5, 16), (3, 4, 16), (3, 1, 5)])
def test_planes_to_volume_exact(B, D, Ws):
    """vol[b, d, p] = src[d * B + b, p, 0], exactly."""
    from ada_mvs_amd import hip_ops
    npix = 37 * 11
    src = torch.randn(D * B, npix, Ws, generator=torch.Generator().manual_seed(B + D))
    vol = torch.full((B, D, npix), PAD, device="cuda")
    hip_ops.planes_to_volume(src.cuda(), vol, B)
    assert torch.equal(vol.cpu(), src[:, :, 0].reshape(D, B, npix).permute(1, 0, 2))


# ---------------------------------------------------------------------------------------------------------------------------
# g. one slice step and one stage end to end
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("concurrent", [True, False])
@pytest.mark.parametrize("C", [32, 16, 8])
def test_regularize_maps_per_element(C, concurrent):
    """slice_RED_Regularization.regularize_maps on random costs at 40 x 72 (8-aligned, ragged for every tile size) over three planes,
    two samples: reg and all four states per element against oracle.slice_red_step in float64, the four levels on their own
    streams and one after the other."""
    from ada_mvs_amd.models.msrednet import slice_RED_Regularization
    B, D, h, w = 2, 3, 40, 72
    sd = msred_ref.red_state_dict(C, seed=20 + C)
    net = slice_RED_Regularization(C, 8)
    net.load_state_dict(sd)
    net = net.cuda()
    net.concurrent_levels = concurrent
    net.packed(torch.device("cuda:0"))
    g = torch.Generator().manual_seed(C)
    costs = [torch.rand(B, C, h, w, generator=g) * 0.8 for _ in range(D)]
    xw0 = net.x_widths()[0]
    xc = torch.cat([-_cl(c) for c in costs], 0)
    X0 = xc if xw0 == C else torch.zeros(D * B, h * w, xw0, device="cuda")
    if xw0 != C:
        X0[:, :, :C] = xc
    fin, R = net.regularize_maps(X0, B, h, w, None if xw0 == C else xc)
    torch.cuda.synchronize()
    sd64 = fp64_bars.double_sd(sd)
    states = [torch.zeros(B, 8 << k, h >> k, w >> k, dtype=torch.float64) for k in range(4)]
    for d in range(D):
        reg, states = mo.slice_red_step(costs[d].double(), states, sd64, "")
        what = "C=%d concurrent=%s plane %d" % (C, concurrent, d)
        _held(fin[d * B:(d + 1) * B, :, 0].reshape(B, 1, h, w), reg, fp64_bars.RED_STEP, "reg " + what)
        for k in range(4):
            got = _nchw(R[k][d * B:(d + 1) * B, :, :HC[k]].contiguous(), h >> k, w >> k)
            _held(got, states[k], fp64_bars.RED_STEP, "state %d %s" % (k + 1, what))


@pytest.mark.parametrize("views", [2, 6])
def test_stage_per_pixel(views):
    """InferDepthNet.run at the `tiny` shape's first stage (16 x 24, 16 planes) for one and five source views: depth in hypothesis
    intervals, confidence absolute, against oracle.infer_depth_stage_red in float64."""
    from ada_mvs_amd import hip_ops
    from ada_mvs_amd.models.msrednet import InferDepthNet, slice_RED_Regularization
    B, C, h, w, D = 2, 32, 16, 24, 16
    sd = msred_ref.red_state_dict(C, seed=30 + views)
    net = slice_RED_Regularization(C, 8)
    net.load_state_dict(sd)
    net = net.cuda()
    feats = [synth.smooth_features(B, C, h, w, seed=40 + v) for v in range(views)]
    proj = synth.rig_projections(views, 4 * h, 4 * w, batch=B)["stage1"]
    planes, interval = msred_ref.uniform_planes(RANGES, D, h, w)
    depth, conf = InferDepthNet().run(torch.cat([_cl(f) for f in feats], 0), B, C, h, w, hip_ops.relative_transforms(proj.cuda()),
                                      planes.cuda(), net)
    ref = mo.infer_depth_stage_red([f.double() for f in feats], proj.double(), planes.double(), fp64_bars.double_sd(sd), "")
    _held(depth, ref["depth"], fp64_bars.RED_STAGE_DEPTH, "stage depth, %d views" % views, scale=interval)
    _held(conf, ref["photometric_confidence"], fp64_bars.RED_STAGE_CONF, "stage confidence, %d views" % views, scale=1.0)
