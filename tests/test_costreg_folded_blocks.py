"""Folded blocks of the F(2x4, 3x3) form (csrc/costreg2d_wino24.hip, Wino24Geom<MT, NT, FOLD>) and of the stride-2 pair form
(csrc/costreg2d.hip, S2PGeom<FOLD>).

The 16 matrix columns of an instruction are 16 / F tiles of each of F tile rows, so a block is F times narrower and F times taller
than the unfolded one: 8 x 32 pixels (F = 2) or 8 x 16 (F = 4) where the unfolded block has 4 x 64.  Per pixel the sums and their
order are those of the unfolded kernel, so every block shape gives the same bits; the layer is held to the bars of
tests/test_costreg_wino24.py::test_conv3x3_dd_wino24 at block widths of one, two and three blocks and heights of a block, one row
more and one row less, and the network to the bar of tests/test_costreg_t2_pairs.py::test_cost_reg_net_2d_at_cfg2_shape_under_s2_pairs.
The selection goes by the maps alone (no option: in the network the forms round differently, and a tile must give the same bits alone
and in a batch); the rule is a host function and is tested without a GPU, and the entry points with an explicit `blocks` argument
(include/adamvs_hip.h) force each form for the comparisons here.
"""
import pytest
import torch

from conftest import rel_l1
from fp64_bars import check
import ada_mvs_amd  # noqa: F401

LAYER_REL, LAYER_MAX = 2e-6, 1.1e-5      # tests/test_costreg_wino24.py::test_conv3x3_dd_wino24 (rel-L1; max |err| / max |ref|)
BLOCK_ROWS = 8                           # both folded blocks: FOLD 2 x NT 2 x 2 rows, FOLD 4 x NT 1 x 2 rows


# ------------------------------------------------------------------------------------------------ the rule (no GPU)
# (N, D, h, w) at the level the layer runs on -> FOLD of conv2 / conv4 (0: the layer stays in F(2x2, 3x3))
NET_RULE = [
    ((1024, 192, 48, 96), 2), ((1024, 192, 24, 48), 4),      # cfg2, 256 tiles x 4 pairs: conv2, conv4
    ((1024, 192, 96, 192), 0), ((1024, 192, 12, 24), 0),     # its outer level (64-pixel blocks tile it) and conv6's (24 = a block and a half)
    ((128, 192, 48, 96), 2), ((128, 192, 24, 48), 4),        # cfg3, 32 tiles
    ((16, 192, 48, 96), 2), ((16, 192, 24, 48), 4),          # one GPU's share of cfg4, 4 tiles
    ((4, 192, 24, 48), 4), ((1, 192, 48, 96), 2),            # ... and one tile of it: by the shape alone, a tile's bits do not depend on the batch
    ((64, 256, 48, 96), 2),                                  # cfg5, 8 tiles x 8 pairs: conv4 (its conv6, on 24 x 48, is not asked: F(2x2, 3x3))
    ((64, 256, 24, 48), 4),                                  # ... the shape rule for a conv2 / conv4 on 24 x 48 at D = 256
    ((64, 256, 96, 192), 0),                                 # ... its conv2: 192 = three 64-pixel blocks
    ((1024, 128, 48, 96), 0), ((1024, 64, 48, 96), 0),       # the blob carries conv2 / conv4 in this form from D = 192
    ((1024, 192, 44, 96), 0), ((1024, 192, 48, 80), 4), ((1024, 192, 48, 72), 0),    # rows that no 8-row block tiles; 80 = 5 x 16; 72
    ((1024, 100, 48, 96), 0),                                # not a width of the network
]
# h x w -> FOLD of the layer op: by the map (adamvs_conv3x3_dd_wino24), and with blocks = 2, 4 (adamvs_conv3x3_dd_wino24_blocks)
LAYER_RULE = [
    ((48, 96), 2, 2, 4), ((24, 48), 4, 1, 4), ((96, 192), 1, 2, 4), ((8, 64), 1, 2, 4), ((8, 32), 2, 2, 4), ((8, 16), 4, 1, 4),
    ((9, 96), 1, 2, 4), ((7, 48), 1, 1, 4), ((8, 40), 1, 1, 1), ((8, 70), 1, 1, 1),
]


def test_fold_rule_on_a_table_of_shapes(set_option):
    from ada_mvs_amd import _lib
    lib = _lib.load()
    for (N, D, h, w), fold in NET_RULE:
        assert lib.adamvs_cost_reg_fold(N, D, h, w) == fold, (N, D, h, w)
    for (h, w), f1, f2, f4 in LAYER_RULE:
        assert lib.adamvs_conv_wino24_fold(h, w, -1) == f1, (h, w)
        assert lib.adamvs_conv_wino24_fold(h, w, 2) == f2 and lib.adamvs_conv_wino24_fold(h, w, 4) == f4, (h, w)
        assert lib.adamvs_conv_wino24_fold(h, w, 1) == 1, (h, w)
    assert lib.adamvs_cost_reg_fold(0, 192, 48, 96) == -1 and lib.adamvs_conv_wino24_fold(0, 96, -1) == -1
    set_option("winograd", 3)                                # F(2x2, 3x3) in every stride-1 layer
    assert lib.adamvs_cost_reg_fold(1024, 192, 48, 96) == 0
    set_option("winograd", 1)
    set_option("wino_wps", 2)                                # a forced tiling keeps the unfolded blocks
    assert lib.adamvs_conv_wino24_fold(48, 96, -1) == 1 and lib.adamvs_conv_wino24_fold(48, 96, 2) == 1


# (N, D, hi, wi) of a stride-2 layer -> its kernel by the map (blocks = -1) and without folded blocks (blocks = 0): 0 direct, 1 / 2 / 4 the pair form on 3 x 32, 6 x 16, 12 x 8
S2_RULE = [
    ((1024, 192, 96, 192), 1, 1), ((1024, 192, 48, 96), 2, 0), ((1024, 192, 24, 48), 4, 0),     # cfg2: conv1, conv3, conv5
    ((1024, 384, 48, 96), 2, 0),                                                                 # two launches of the 192-channel tiling
    ((128, 192, 96, 192), 1, 1), ((128, 192, 48, 96), 0, 0), ((128, 192, 24, 48), 0, 0),         # cfg3: 1152 and 512 blocks of 8 rows: 2-row blocks
    ((64, 256, 192, 384), 0, 0), ((64, 256, 96, 192), 0, 0),                                     # cfg5: D = 256 has no pair form
    ((1024, 192, 44, 96), 0, 0), ((1024, 192, 48, 80), 4, 0), ((1024, 192, 48, 100), 0, 0),      # 22 rows: no blocks of 6 or 12; 40 = 5 x 8 columns; 50: none
    ((1024, 192, 48, 520), 1, 1), ((1024, 100, 48, 96), -1, -1),
]


def test_stride_two_rule_on_a_table_of_shapes(set_option):
    from ada_mvs_amd import _lib
    lib = _lib.load()
    for (N, D, hi, wi), f1, f0 in S2_RULE:
        assert lib.adamvs_conv_s2_form(N, D, hi, wi, -1) == f1, (N, D, hi, wi)
        assert lib.adamvs_conv_s2_form(N, D, hi, wi, 0) == f0, (N, D, hi, wi)
    # forced wherever the width is a multiple of 8, at any height
    assert lib.adamvs_conv_s2_form(1024, 192, 46, 96, 4) == 4 and lib.adamvs_conv_s2_form(1024, 192, 46, 100, 4) == 0
    set_option("s2_pairs", 0)
    assert lib.adamvs_conv_s2_form(1024, 192, 48, 96, -1) == 0 and lib.adamvs_conv_s2_form(1024, 192, 96, 192, -1) == 0


def test_the_blob_grows_behind_the_blocks_of_before():
    """pack_cost_reg_net_2d from D = 192: conv2 and conv4 in the F(2x4, 3x3) form behind everything that was there, which stays where
    it was; the blobs at D = 64 and 128 are those of before; the library expects that length."""
    from ada_mvs_amd import _lib, packing, synth
    from ada_mvs_amd.models.adamvs import CostRegNet2D
    lib = _lib.load()
    for D in (128, 192):
        sd = synth.seeded_state_dict(CostRegNet2D(D), seed=3)
        blob = packing.pack_cost_reg_net_2d(sd, "")
        n_old = 11 * (9 * D * D + D) + 5 * 16 * D * D + 2 * 24 * D * D
        assert blob.numel() == lib.adamvs_cost_reg_net_2d_weight_floats(D, 0) == n_old + (2 * 24 * D * D if D >= 192 else 0)
        inner = packing.WINO24_INNER_BLOB_WIDTHS
        try:
            packing.WINO24_INNER_BLOB_WIDTHS = ()                # the packing of before
            assert torch.equal(packing.pack_cost_reg_net_2d(sd, ""), blob[:n_old])
        finally:
            packing.WINO24_INNER_BLOB_WIDTHS = inner
        if D >= 192:
            for k, name in enumerate(("conv2", "conv4")):
                bn = lambda s: sd["%s.bn.%s" % (name, s)].float()      # noqa: E731
                want = packing.pack_reg_layer_wino24(sd[name + ".conv.weight"], bn("weight") / torch.sqrt(bn("running_var") + packing.BN_EPS))
                assert torch.equal(blob[n_old + k * 24 * D * D:n_old + (k + 1) * 24 * D * D], want), name


# ------------------------------------------------------------------------------------------------ the layer, F(2x4, 3x3)
def dev(t):
    return t.cuda().contiguous()


def _layer_case(N, D, h, w, relu, skip):
    """Inputs drawn as in tests/test_costreg_wino24.py::layer_case, the float64 reference with them."""
    g = torch.Generator().manual_seed(N * 1000 + D + h + w)
    x = torch.randn(N, D, h, w, generator=g)
    wt = torch.randn(D, D, 3, 3, generator=g) / (3 * D ** 0.5)
    scale, shift = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.1
    sk = torch.randn(N, h * w, D, generator=g) if skip else None
    ref = torch.nn.functional.conv2d(x.double(), (wt * scale.reshape(-1, 1, 1, 1)).double(), shift.double(), padding=1)
    ref = torch.relu(ref) if relu else ref
    if skip:
        ref = ref + sk.double().reshape(N, h, w, D).permute(0, 3, 1, 2)
    return x, wt, scale, shift, sk, ref


# widths of one, two and three blocks of the fold by 2 (32 columns) and of one and three of the fold by 4 (16); 40: ragged for both
# folds, the layer must fall back to the 64-pixel blocks
FOLD_WIDTHS = [(2, 32), (2, 64), (2, 96), (4, 16), (4, 48), (2, 40), (4, 40)]
# one block, a row past it (the second block row has one row in the map), a row short of it; each with ReLU and no skip, and with
# a skip and no ReLU
HEIGHTS = [(hh, relu, skip) for hh in (BLOCK_ROWS, BLOCK_ROWS + 1, BLOCK_ROWS - 1) for relu, skip in ((1, False), (0, True))]


@pytest.mark.gpu
@pytest.mark.parametrize("h,relu,skip", HEIGHTS)
@pytest.mark.parametrize("fold,w", FOLD_WIDTHS)
@pytest.mark.parametrize("D", [128, 192])
def test_wino24_layer_on_folded_blocks(D, fold, w, h, relu, skip):
    """hip_ops.conv3x3_dd_wino24 with the fold forced (blocks = 2 / 4), into an output pre-filled with NaN (a pixel or channel that
    no lane stores fails the bars), against a float64 convolution and the direct kernel under the bars of test_conv3x3_dd_wino24;
    then the same inputs on the unfolded blocks (blocks = 1) and through the plain entry point: the same bits."""
    from ada_mvs_amd import _lib, hip_ops, packing
    N = 2
    took = _lib.load().adamvs_conv_wino24_fold(h, w, fold)
    assert took == (fold if w % (64 // fold) == 0 else 1), took
    x, wt, scale, shift, sk, ref = _layer_case(N, D, h, w, relu, skip)
    x_cl = dev(x.permute(0, 2, 3, 1).reshape(N, h * w, D).contiguous())
    wk, bias, skd = dev(packing.pack_reg_layer_wino24(wt, scale)), dev(shift), dev(sk) if skip else None

    def run(blocks):
        out = torch.full((N, h * w, D), float("nan"), device="cuda")
        hip_ops.conv3x3_dd_wino24(x_cl, wk, bias, skd, N, D, h, w, relu, out=out, blocks=blocks)
        torch.cuda.synchronize()
        return out.cpu()
    folded = run(fold)
    pk = dev(packing.pack_reg_layer(wt, scale, shift, False))
    direct = hip_ops.conv3x3_dd(x_cl, pk[:9 * D * D], pk[9 * D * D:], skd, N, D, h, w, 0, relu)
    back = lambda y: y.cpu().double().reshape(N, h, w, D).permute(0, 3, 1, 2)      # noqa: E731
    assert bool(torch.isfinite(folded).all())
    e64, edir = rel_l1(back(folded), ref), rel_l1(back(folded), back(direct))
    emax = float((back(folded) - ref).abs().max() / ref.abs().max())
    print("fold %d, %s: rel-L1 %.3e against float64, %.3e against the direct kernel, max|err|/max|ref| %.3e" % (took, (N, D, h, w, relu, skip), e64, edir, emax))
    assert e64 < LAYER_REL and edir < LAYER_REL
    check(back(folded), ref, LAYER_MAX, what="layer, per element")
    assert torch.equal(run(1), folded) and torch.equal(run(None), folded)


# ------------------------------------------------------------------------------------------------ the network
@pytest.mark.gpu
def test_cost_reg_net_2d_with_and_without_folded_blocks(set_option):
    """The whole network at cfg2's shape (D = 192, two maps of 96 x 192) with the large-grid kernels forced (t2_fused = 0, conv_rows2 = 0):
    conv2 on 8 x 32 blocks, conv4 on 8 x 16, conv3 and conv5 in the pair form on 6 x 16 and 12 x 8, against the oracle under the bar of
    test_cost_reg_net_2d_at_cfg2_shape_under_s2_pairs; adamvs_cost_reg_net_2d_blocks(blocks = 0): the selection of before (F(2x2, 3x3) and
    the direct stride-2 kernel there), within the same bar, other bits; blocks = -1 is the plain entry point.  Left to the grid rules,
    two maps give conv3 and conv5 the 2-row kernel either way: then only conv2 and conv4 differ."""
    from test_hip_parity import OP_TOL
    from ada_mvs_amd import _lib, hip_ops, packing, synth
    from ada_mvs_amd.models.adamvs import CostRegNet2D
    from oracle import adamvs_oracle as O
    lib = _lib.load()
    D, h, w = 192, 96, 192
    sd = synth.seeded_state_dict(CostRegNet2D(D), seed=1)
    x = torch.randn(2, D, h, w, generator=torch.Generator().manual_seed(D)) * 0.5
    ref = O.cost_reg_net_2d(x, sd, "")
    blob, x_cl = packing.pack_cost_reg_net_2d(sd, "").cuda(), x.permute(0, 2, 3, 1).reshape(2, h * w, D).contiguous().cuda()
    net = lambda blocks: hip_ops.cost_reg_net_2d(x_cl, blob, h, w, blocks=blocks).cpu().reshape(2, h, w, D).permute(0, 3, 1, 2)      # noqa: E731
    assert (lib.adamvs_cost_reg_fold(2, D, h // 2, w // 2), lib.adamvs_cost_reg_fold(2, D, h // 4, w // 4)) == (2, 4)
    s2 = lambda blocks: (lib.adamvs_conv_s2_form(2, D, h // 2, w // 2, blocks), lib.adamvs_conv_s2_form(2, D, h // 4, w // 4, blocks))      # noqa: E731
    outs = {}
    for rows2, want in ((0, (2, 4)), (-1, (0, 0))):
        set_option("t2_fused", rows2)
        set_option("conv_rows2", rows2)
        assert s2(-1) == want and s2(0) == (0, 0)
        for blocks in (None, -1, 0):
            outs[rows2, blocks] = net(blocks)
            err = rel_l1(outs[rows2, blocks], ref.reshape(outs[rows2, blocks].shape))
            print("conv_rows2 = %d, blocks = %s: rel_l1 %.3e" % (rows2, blocks, err))
            assert err < OP_TOL, (rows2, blocks, err)
        assert torch.equal(outs[rows2, None], outs[rows2, -1]) and not torch.equal(outs[rows2, -1], outs[rows2, 0])
    assert not torch.equal(outs[0, -1], outs[-1, -1])


@pytest.mark.gpu
@pytest.mark.parametrize("rows2", [0, -1])
def test_blocks_0_is_the_chain_of_before(set_option, rows2):
    """adamvs_cost_reg_net_2d_blocks(blocks = 0) against the network of before round 10 rebuilt from the one-layer ops that this change
    leaves untouched, bit for bit, on a shape where the default folds (D = 192, two maps of 96 x 192; large-grid kernels forced, and the
    grid rules left alone).  The chain: bench.timed_cost_reg_layers, as test_costreg_wino24.py::test_winograd_3_is_the_network_of_before
    uses it -- adamvs_conv3x3_dd_wino for every stride-1 layer and adamvs_conv3x3_dd for the others -- under winograd = 7 (F(2x2, 3x3)
    everywhere; + 4 keeps the plain stride-2 op off the folded blocks).  Under winograd = 3, blocks = 0 must equal it; so must the plain
    entry point under winograd = 7.  With conv0 and prob in F(2x4, 3x3) again (winograd = 1), blocks = 0 equals the plain entry point
    under winograd = 5, the run-time switch of bench.py's A/B, and the chain with those two layers through adamvs_conv3x3_dd_wino24."""
    import bench
    from ada_mvs_amd import hip_ops, packing, synth
    from ada_mvs_amd.models.adamvs import CostRegNet2D
    N, D, h, w = 2, 192, 96, 192
    sd = synth.seeded_state_dict(CostRegNet2D(D), seed=1)
    blob = packing.pack_cost_reg_net_2d(sd, "").cuda()
    x = (torch.randn(N, h * w, D, generator=torch.Generator().manual_seed(D)) * 0.5).cuda()
    set_option("t2_fused", rows2)
    set_option("conv_rows2", rows2)
    set_option("winograd", 7)
    chain = bench.timed_cost_reg_layers(lambda name, fn: fn(), 1, x, blob, N, D, h, w)
    plain7 = hip_ops.cost_reg_net_2d(x, blob, h, w)
    set_option("winograd", 3)
    before3 = hip_ops.cost_reg_net_2d(x, blob, h, w, blocks=0)
    default3 = hip_ops.cost_reg_net_2d(x, blob, h, w)
    torch.cuda.synchronize()
    assert float(chain.abs().max()) > 0 and torch.equal(before3, chain) and torch.equal(plain7, chain)
    # winograd = 3 alone leaves the stride-2 folds on: other bits with the large-grid kernels, none on this small grid's 2-row kernels
    assert torch.equal(default3, chain) == (rows2 == -1)
    set_option("winograd", 5)
    plain5 = hip_ops.cost_reg_net_2d(x, blob, h, w)
    # the chain of before with conv0 and prob in F(2x4, 3x3): the F(2x2, 3x3) chain's layers, those two swapped
    LW, n24 = 9 * D * D + D, 11 * (9 * D * D + D) + 5 * 16 * D * D
    real = hip_ops.conv3x3_dd_wino

    def swapped(xin, ww, bias, skip, N_, D_, hi, wi, relu, out=None):
        if (hi, wi) != (h, w):
            return real(xin, ww, bias, skip, N_, D_, hi, wi, relu, out=out)
        k = 0 if relu else 1                                 # conv0 has the ReLU, prob has none
        return hip_ops.conv3x3_dd_wino24(xin, blob[n24 + k * 24 * D * D:n24 + (k + 1) * 24 * D * D], bias, skip, N_, D_, hi, wi, relu, out=out, blocks=1)
    hip_ops.conv3x3_dd_wino = swapped
    try:
        chain24 = bench.timed_cost_reg_layers(lambda name, fn: fn(), 1, x, blob, N, D, h, w)
    finally:
        hip_ops.conv3x3_dd_wino = real
    set_option("winograd", 1)
    before1 = hip_ops.cost_reg_net_2d(x, blob, h, w, blocks=0)
    torch.cuda.synchronize()
    assert torch.equal(before1, plain5) and torch.equal(before1, chain24) and not torch.equal(before1, chain)


# ------------------------------------------------------------------------------------------------ the layer, stride 2 in the pair form
S2_REL, S2_MAX = 2e-6, 2e-5              # tests/test_hip_parity.py::test_stride_two_layer_in_the_pair_form
# (N, D, ho, wo, fold forced, relu).  Output widths of one and three blocks of 16 columns (fold 2) and of 8 (fold 4); output heights of
# one row, of a block and a row (7 = 6 + 1; 13 = 12 + 1), short of a block (5, 11) and whole blocks (6, 12, 24); D = 384 is two
# launches; 40 maps.  (adamvs_conv3x3_dd takes even input sizes only at stride 2: the odd sizes here are the outputs'.)
S2_CASES = [
    (2, 192, 1, 16, 2, 1), (2, 192, 7, 48, 2, 0), (2, 192, 5, 16, 2, 1), (2, 192, 24, 48, 2, 1), (2, 384, 7, 16, 2, 1), (2, 384, 6, 48, 2, 0),
    (2, 192, 1, 8, 4, 1), (2, 192, 7, 24, 4, 0), (2, 192, 13, 24, 4, 1), (2, 192, 12, 24, 4, 1), (2, 384, 11, 8, 4, 1), (2, 384, 7, 24, 4, 0),
    (40, 192, 7, 48, 2, 1), (40, 192, 13, 24, 4, 1),
]


def _s2_run(inputs, N, D, hi, wi, relu, blocks=None):
    """blocks None: hip_ops.conv3x3_dd(mode = 1), the plain entry point; else adamvs_conv3x3_dd_s2_blocks."""
    from ada_mvs_amd import hip_ops, packing
    x, _, wt, scale, shift, _ = inputs
    pk = packing.pack_reg_layer(wt, scale, shift, False).cuda()
    out = torch.full((N, (hi // 2) * (wi // 2), D), float("nan"), device="cuda")
    x_cl = x.permute(0, 2, 3, 1).reshape(N, hi * wi, D).contiguous().cuda()
    if blocks is None:
        hip_ops.conv3x3_dd(x_cl, pk[:9 * D * D], pk[9 * D * D:], None, N, D, hi, wi, 1, relu, out=out)
    else:
        hip_ops.conv3x3_dd_s2_blocks(x_cl, pk[:9 * D * D], pk[9 * D * D:], N, D, hi, wi, relu, blocks, out=out)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("N,D,ho,wo,fold,relu", S2_CASES)
def test_stride_two_pair_form_on_folded_blocks(set_option, N, D, ho, wo, fold, relu):
    """The stride-2 layer with conv_rows2 = 0 and the fold forced (adamvs_conv3x3_dd_s2_blocks), into an output pre-filled with NaN,
    against a float64 convolution under the bars of test_stride_two_layer_in_the_pair_form; blocks = 0 gives these widths to the
    direct kernel, as before: the bits of s2_pairs = 0.  hip_ops.conv3x3_dd(mode = 1) takes the fold exactly where the blocks tile
    the map."""
    from test_kernel_forms import _layer_inputs, _reference
    hi, wi = 2 * ho, 2 * wo
    set_option("conv_rows2", 0)
    inputs = _layer_inputs(1, D, N, hi, wi, False, False, seed=3000 + D + 7 * N + hi + wi)
    ref = _reference(1, inputs[0], None, inputs[2], inputs[3], inputs[4], relu, None)
    back = lambda y: y.double().reshape(N, ho, wo, D).permute(0, 3, 1, 2)      # noqa: E731
    folded = _s2_run(inputs, N, D, hi, wi, relu, fold)
    assert bool(torch.isfinite(folded).all())
    err, worst = rel_l1(back(folded), ref), float((back(folded) - ref).abs().max() / ref.abs().max())
    print("stride 2, fold %d, %s: rel_l1 %.3e, max|err| / max|ref| %.3e" % (fold, (N, D, ho, wo), err, worst))
    assert err < S2_REL and worst < S2_MAX
    before = _s2_run(inputs, N, D, hi, wi, relu, 0)
    plain = _s2_run(inputs, N, D, hi, wi, relu)
    assert torch.equal(_s2_run(inputs, N, D, hi, wi, relu, -1), plain)
    set_option("s2_pairs", 0)
    direct = _s2_run(inputs, N, D, hi, wi, relu)
    assert torch.equal(before, direct)                        # no 32-column block fits these widths: the direct kernel, as before
    assert not torch.equal(folded, direct)                    # ... and the pair form rounds differently
    tiles = ho % (3 * fold) == 0
    assert torch.equal(plain, folded if tiles else direct)


@pytest.mark.gpu
@pytest.mark.parametrize("D,ho,wo,relu", [(192, 7, 32, 1), (192, 12, 64, 0), (384, 5, 32, 1)])
def test_folded_and_unfolded_pair_kernels_give_the_same_bits(set_option, D, ho, wo, relu):
    """Widths that the 32-column block divides: the unfolded pair kernel (the plain entry point, blocks = -1, 0) and both folds forced,
    bit for bit."""
    from test_kernel_forms import _layer_inputs, _reference
    N, hi, wi = 2, 2 * ho, 2 * wo
    set_option("conv_rows2", 0)
    inputs = _layer_inputs(1, D, N, hi, wi, False, False, seed=4000 + D + hi + wi)
    ref = _reference(1, inputs[0], None, inputs[2], inputs[3], inputs[4], relu, None)
    outs = {blocks: _s2_run(inputs, N, D, hi, wi, relu, blocks) for blocks in (None, -1, 0, 2, 4)}
    got = outs[None].double().reshape(N, ho, wo, D).permute(0, 3, 1, 2)
    assert rel_l1(got, ref) < S2_REL and float((got - ref).abs().max()) < S2_MAX * float(ref.abs().max())
    for blocks in (-1, 0, 2, 4):
        assert torch.equal(outs[blocks], outs[None]), blocks
    set_option("s2_pairs", 0)
    assert not torch.equal(_s2_run(inputs, N, D, hi, wi, relu), outs[None])
