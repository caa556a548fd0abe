"""The transposed CostRegNet2D layers in the pair form along x (csrc/costreg2d.hip::k_conv_dd_t2p, option s2_pairs).

Two neighbouring odd output columns of a transposed 3 x 3 stride-2 layer share an input column; the kernel spends three products on
them instead of four (15 of 18 of the layer's products) by accumulating W2 (in[j] - in[j + 1]), (W0 + W2) in[j + 1] and
W0 (in[j + 2] - in[j + 1]).  The differences are rounded once more than the direct form's operands, so the form is held to the SAME
per-element float64 bars as the direct transposed kernel (tests/test_kernel_forms.py::test_conv3x3_dd_forms: relative L1 2e-6, largest
error 2e-5 of the largest value), at shapes that take the pair kernel and at shapes that must fall back, against the direct kernel on
the same inputs, and through the whole network.  The selection rule is a host function and is tested without a GPU.
"""
import pytest
import torch

from conftest import rel_l1
import ada_mvs_amd  # noqa: F401
from test_kernel_forms import _cl, _layer_inputs, _reference

REL_BAR, MAX_BAR = 2e-6, 2e-5          # test_kernel_forms.py::test_conv3x3_dd_forms, fp32
CLASS_BY_CLASS, FUSED, PAIRS = 0, 1, 2


# ------------------------------------------------------------------------------------------------ the rule (no GPU)
# (N, D, hi, wi) -> form under the default options.  The small-grid rule comes first (class-by-class blocks of 8 x 16 inputs,
# at most 2048 of them: the fused kernel); then the pair form for the 192-channel tiling where a row fills blocks of 32 columns.
RULE = [
    ((1024, 192, 48, 96), PAIRS),            # cfg2 conv11 at 256 tiles x 4 views
    ((1024, 192, 24, 48), CLASS_BY_CLASS),   # conv9: a block and a half per row
    ((1024, 192, 12, 24), CLASS_BY_CLASS),   # conv7: less than a block
    ((1024, 384, 48, 96), PAIRS),            # two launches of the 192-channel tiling
    ((32, 192, 96, 192), PAIRS),             # cfg5's width
    ((512, 192, 48, 32), PAIRS), ((512, 192, 48, 64), PAIRS), ((512, 192, 48, 100), PAIRS), ((512, 192, 47, 128), PAIRS),
    ((512, 192, 48, 80), CLASS_BY_CLASS),    # 3 pair blocks against 5 direct ones: 5 * 2 * 3 = 6 * 5, no fewer products
    ((512, 192, 48, 97), CLASS_BY_CLASS), ((512, 192, 48, 33), CLASS_BY_CLASS), ((2048, 192, 8, 30), CLASS_BY_CLASS),
    ((4, 192, 48, 96), FUSED),               # 72 blocks: the small-grid form keeps the layer
    ((1024, 64, 48, 96), CLASS_BY_CLASS), ((1024, 128, 48, 96), CLASS_BY_CLASS), ((1024, 256, 48, 96), CLASS_BY_CLASS),
    ((1024, 96, 48, 96), CLASS_BY_CLASS), ((1024, 512, 48, 96), CLASS_BY_CLASS),
    ((1024, 100, 48, 96), -1),               # not a width of the network
]


def test_transposed_form_rule_on_a_table_of_shapes(set_option):
    from ada_mvs_amd import _lib
    lib = _lib.load()
    for (N, D, hi, wi), form in RULE:
        assert lib.adamvs_conv_t2_form(N, D, hi, wi) == form, (N, D, hi, wi)
    assert lib.adamvs_conv_t2_form(0, 192, 48, 96) == -1
    set_option("s2_pairs", 0)
    for (N, D, hi, wi), form in RULE:
        assert lib.adamvs_conv_t2_form(N, D, hi, wi) == (CLASS_BY_CLASS if form == PAIRS else form), (N, D, hi, wi)
    set_option("s2_pairs", 1)
    set_option("t2_fused", 0)
    assert lib.adamvs_conv_t2_form(4, 192, 48, 96) == PAIRS and lib.adamvs_conv_t2_form(1, 192, 3, 32) == PAIRS
    assert lib.adamvs_conv_t2_form(4, 128, 48, 96) == CLASS_BY_CLASS
    set_option("t2_fused", 1)
    assert lib.adamvs_conv_t2_form(1024, 192, 48, 96) == FUSED


# ------------------------------------------------------------------------------------------------ the layer
def _run(mode_inputs, N, D, hi, wi, relu, skip, in2, nan_out=False):
    from ada_mvs_amd import hip_ops, packing
    x, x2, wt, scale, shift, sk = mode_inputs
    pk = packing.pack_reg_layer(wt, scale, shift, True).cuda()
    out = torch.full((N, 4 * hi * wi, D), float("nan"), device="cuda") if nan_out else None
    kw = {"out": out} if nan_out else {}
    got = hip_ops.conv3x3_dd(_cl(x), pk[:9 * D * D], pk[9 * D * D:], _cl(sk) if skip else None, N, D, hi, wi, 2, relu,
                             in2=_cl(x2) if in2 else None, **kw)
    torch.cuda.synchronize()
    return got.cpu().double().reshape(N, 2 * hi, 2 * wi, D).permute(0, 3, 1, 2)


def _errors(got, ref):
    return rel_l1(got, ref), float((got - ref).abs().max() / ref.abs().max())


# (N, D, hi, wi, relu, skip, in2, t2_fused, form the launcher must take)
LAYER_CASES = [
    # cfg2's three transposed layers (96 x 192 maps: inputs 48 x 96, 24 x 48, 12 x 24) on the large-grid path
    (2, 192, 48, 96, 1, True, True, 0, PAIRS),
    (2, 192, 24, 48, 1, False, True, 0, CLASS_BY_CLASS),
    (2, 192, 12, 24, 1, False, False, 0, CLASS_BY_CLASS),
    # widths of one, two, three blocks and a ragged fourth; rows no multiple of the block's two; with / without ReLU, skip, in2
    (2, 192, 5, 32, 0, False, False, 0, PAIRS),
    (1, 192, 7, 64, 1, True, False, 0, PAIRS),
    (3, 192, 3, 96, 0, False, True, 0, PAIRS),
    (2, 192, 9, 100, 1, True, True, 0, PAIRS),
    (1, 192, 1, 32, 0, True, True, 0, PAIRS),
    (2, 384, 5, 64, 1, True, True, 0, PAIRS),
    (1, 384, 6, 100, 0, False, False, 0, PAIRS),
    # must fall back: odd widths, widths that waste a block, a small grid, the other tilings
    (2, 192, 5, 33, 1, True, True, 0, CLASS_BY_CLASS),
    (2, 192, 5, 97, 1, True, True, 0, CLASS_BY_CLASS),
    (2, 192, 6, 48, 0, True, True, 0, CLASS_BY_CLASS),
    (2, 192, 6, 96, 1, True, True, -1, FUSED),
    (2, 64, 5, 64, 1, True, True, 0, CLASS_BY_CLASS),
    (2, 128, 5, 64, 1, True, True, 0, CLASS_BY_CLASS),
    (2, 256, 5, 64, 1, True, True, 0, CLASS_BY_CLASS),
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,D,hi,wi,relu,skip,in2,fused,form", LAYER_CASES)
def test_transposed_layer_in_the_pair_form(set_option, N, D, hi, wi, relu, skip, in2, fused, form):
    """hip_ops.conv3x3_dd(mode=2) against a float64 conv_transpose2d of the same weights, into an output buffer pre-filled with NaN
    (a pixel or channel no lane stores stays NaN and fails the bar); then the same inputs with s2_pairs = 0 (the direct kernels):
    both within the bars, and where the pair kernel runs the two differ in their last bits."""
    from ada_mvs_amd import _lib
    set_option("t2_fused", fused)
    assert _lib.load().adamvs_conv_t2_form(N, D, hi, wi) == form
    inputs = _layer_inputs(2, D, N, hi, wi, skip, in2, seed=2000 + D + 7 * N + hi + wi)
    ref = _reference(2, inputs[0], inputs[1], inputs[2], inputs[3], inputs[4], relu, inputs[5])
    got = _run(inputs, N, D, hi, wi, relu, skip, in2, nan_out=True)
    err, worst = _errors(got, ref)
    print("pair form: rel_l1 %.3e, max|err| / max|ref| %.3e" % (err, worst))
    set_option("s2_pairs", 0)
    direct = _run(inputs, N, D, hi, wi, relu, skip, in2, nan_out=True)
    derr, dworst = _errors(direct, ref)
    diff = float((got - direct).abs().max())
    print("direct:    rel_l1 %.3e, max|err| / max|ref| %.3e; max |pair - direct| %.3e" % (derr, dworst, diff))
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(direct).all())
    assert err < REL_BAR and worst < MAX_BAR, "rel_l1 %.3e, max|err| / max|ref| %.3e" % (err, worst)
    assert derr < REL_BAR and dworst < MAX_BAR, "direct: rel_l1 %.3e, max|err| / max|ref| %.3e" % (derr, dworst)
    assert (diff > 0) == (form == PAIRS), "max |pair - direct| %.3e" % diff
    assert diff < 2 * MAX_BAR * float(ref.abs().max()), "max |pair - direct| %.3e" % diff


@pytest.mark.gpu
@pytest.mark.parametrize("pairs", [1, 0])
def test_cost_reg_net_2d_at_cfg2_shape_under_s2_pairs(set_option, pairs):
    """The whole network at cfg2's shape (D = 192, 96 x 192 maps) with the large-grid kernels forced on two maps (t2_fused = 0,
    conv_rows2 = 0: conv11 takes the pair kernel under s2_pairs = 1), against the oracle and the bar the network tests use
    (tests/test_hip_parity.py::test_cost_reg_net_2d_widths: OP_TOL)."""
    from test_hip_parity import OP_TOL
    from ada_mvs_amd import _lib, synth
    from ada_mvs_amd.models.adamvs import CostRegNet2D
    from oracle import adamvs_oracle as O
    set_option("s2_pairs", pairs)
    set_option("t2_fused", 0)
    set_option("conv_rows2", 0)
    D, h, w = 192, 96, 192
    assert _lib.load().adamvs_conv_t2_form(2, D, h // 2, w // 2) == (PAIRS if pairs else CLASS_BY_CLASS)
    net = CostRegNet2D(D)
    sd = synth.seeded_state_dict(net, seed=1)
    net.load_state_dict(sd)
    x = torch.randn(2, D, h, w, generator=torch.Generator().manual_seed(D)) * 0.5
    ref = O.cost_reg_net_2d(x, sd, "")
    out = net.cuda()(x.cuda())
    err = rel_l1(out, ref)
    print("s2_pairs = %d: rel_l1 %.3e" % (pairs, err))
    assert err < OP_TOL, err
