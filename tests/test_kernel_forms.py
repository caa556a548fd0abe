"""Every kernel form behind the option table (include/adamvs_hip.h "OPTIONS") against a float64 reference of its layer.

The header says every option chooses between forms of the SAME layer, each held to the same oracle.  The network-level
tests measure eleven layers by one mean; here each form of adamvs_conv3x3_dd and of the unfused softmax / regression
(k_softmax_regress) is compared with torch in float64 at the shapes where tiled kernels go wrong -- maps smaller than one
block, ragged rows and columns, several images -- with a max-error bar as well as the mean, so that one wrong border
column or parity class fails.  FORMS lists every value of every option and the test that runs it; tests/test_host_logic.py
holds the table to csrc/options.h without a GPU.
"""
import math

import pytest
import torch

from conftest import rel_l1
import ada_mvs_amd  # noqa: F401

pytestmark = pytest.mark.gpu

# option -> {value: what it selects -- the test that runs it}.  Read by tests/test_host_logic.py with ast.literal_eval: keep it a
# literal, one entry per option of csrc/options.h, every value the launchers tell apart.
FORMS = {
    "winograd": {
        1: "stride-1 CostRegNet2D layers in F(2x2, 3x3) -- test_hip_parity.py::test_conv3x3_dd_winograd",
        0: "the direct kernels at those widths -- test_hip_parity.py::test_cost_reg_net_2d_direct_kernels_behind_their_options",
    },
    "wino_softmax": {
        1: "softmax partials in the F(2x2, 3x3) `prob` layer -- test_hip_parity.py::test_prob_softmax_regress_winograd",
        0: "score volume + k_softmax_regress -- test_hip_parity.py::test_cost_reg_net_2d_direct_kernels_behind_their_options",
    },
    "wino_wps": {
        0: "workgroups per CU by map size -- test_hip_parity.py::test_conv3x3_dd_winograd",
        1: "one workgroup per CU -- test_hip_parity.py::test_winograd_one_and_two_workgroups_per_cu_give_the_same_bits",
        2: "two workgroups per CU -- test_hip_parity.py::test_winograd_one_and_two_workgroups_per_cu_give_the_same_bits",
    },
    "fuse_softmax": {
        1: "softmax in the direct `prob` kernel's epilogue -- test_hip_parity.py::test_prob_softmax_regress_fused",
        0: "scores, then k_softmax_regress<NQ> -- test_kernel_forms.py::test_softmax_max_regress_unfused, "
           "test_hip_parity.py::test_cost_reg_net_2d_direct_kernels_behind_their_options",
    },
    "s2_pairs": {
        1: "k_conv_dd_s2p on large stride-2 layers -- test_kernel_forms.py::test_conv3x3_dd_forms, "
           "test_hip_parity.py::test_stride_two_layer_in_the_pair_form",
        0: "k_conv_dd<CONV_S2> there -- test_kernel_forms.py::test_conv3x3_dd_forms",
    },
    "conv_rows2": {
        -1: "by grid size (blocks8 <= 2048) -- test_kernel_forms.py::test_rows2_rule_boundary",
        0: "k_conv_dd (8-row blocks) -- test_kernel_forms.py::test_conv3x3_dd_forms",
        1: "k_conv_dd_rows2 -- test_kernel_forms.py::test_conv3x3_dd_forms",
    },
    "t2_fused": {
        -1: "by grid size (class-by-class blocks <= 2048) -- test_kernel_forms.py::test_t2_fused_rule_boundary",
        0: "k_conv_dd<CONV_T2> class by class -- test_kernel_forms.py::test_conv3x3_dd_forms",
        1: "k_conv_dd_t2_fused -- test_kernel_forms.py::test_conv3x3_dd_forms",
    },
    "t2_kb8": {
        1: "k_conv_dd<CONV_T2, KB = 8> at D = 192 / 384 -- test_kernel_forms.py::test_conv3x3_dd_forms",
        0: "k_conv_dd<CONV_T2, KB = 4> there -- test_kernel_forms.py::test_conv3x3_dd_forms",
    },
    "costreg_defer_skips": {
        1: "skips added by the consuming transposed layer (in2) -- test_hip_parity.py::test_cost_reg_net_2d_widths",
        0: "skips in the producer's epilogue -- test_hip_parity.py::test_cost_reg_net_2d_direct_kernels_behind_their_options",
    },
    "conv256_split": {
        1: "D = 256 as two launches of the <4, 2> tiling -- test_kernel_forms.py::test_conv3x3_dd_forms",
        0: "the wide <4, 4> tiling -- test_kernel_forms.py::test_conv3x3_dd_forms",
    },
    "conv_small_grid": {
        1024: "D = 32 / 64 stride-1 layers resident up to 1024 workgroups -- test_kernel_forms.py::test_conv3x3_dd_forms, "
              "test_msrednet.py::test_conv3x3_dd_small_grid_form_against_torch; per element, NTR = 1 / 2 / 4 at this limit and at "
              "lowered ones -- test_msred_forms.py::test_red_recur_split",
        0: "never resident: k_conv_dd<2, 1> / <4, 1> -- test_kernel_forms.py::test_conv3x3_dd_forms, "
           "test_msrednet.py::test_unfolded_recurrence_paths_in_a_child_process; per element -- "
           "test_msred_forms.py::test_red_recur_split, test_msred_forms.py::test_recurrence_paths_by_their_bits",
    },
    "red_fold_applies": {
        -1: "by batch -- test_msrednet.py::test_end_to_end_batch_of_two_against_oracle; bit-equal to the forced arm of its side -- "
            "test_msred_forms.py::test_recurrence_paths_by_their_bits",
        0: "unfolded GRU applies -- test_msrednet.py::test_unfolded_recurrence_paths_in_a_child_process; per element -- "
           "test_msred_forms.py::test_red_recur_pair, test_msred_forms.py::test_red_recur_split",
        1: "folded into the next layer (what -1 takes at one sample) -- test_msrednet.py::test_end_to_end_against_reference_golden_and_oracle; "
           "per element, three samples included -- test_msred_forms.py::test_red_recur_pair, test_msred_forms.py::test_red_recur_split",
    },
    "conv1_f23": {
        3: "F(2, 3) along x at C = 32 and C = 16 / 8, per element against float64 -- test_hip_parity.py::test_aggregate_conv1",
        2: "k_conv1_ksplit<32>, F(2, 3) at C = 16 / 8 -- test_hip_parity.py::test_conv1_and_feature_net0_behind_their_options "
           "(test_aggregate_conv1 per element)",
        1: "F(2, 3) at C = 32, k_conv1_two_row<16 / 8> -- test_hip_parity.py::test_conv1_and_feature_net0_behind_their_options "
           "(test_aggregate_conv1 per element)",
        0: "k_conv1_ksplit<32>, k_conv1_two_row<16 / 8> -- test_hip_parity.py::test_conv1_and_feature_net0_behind_their_options "
           "(test_aggregate_conv1 per element)",
    },
    "fconv_f23": {
        1: "k_fconv_f23 on FeatureNet0's stride-1 layers, per element against float64 -- test_hip_parity.py::test_feature_net0_against_oracle",
        0: "k_fconv there, class-by-class transposed layers -- test_hip_parity.py::test_conv1_and_feature_net0_behind_their_options "
           "(test_feature_net0_against_oracle per element)",
    },
    "gru_wino": {
        7: "gates1, gates2, cand2 in F(2x2, 3x3) -- test_hip_parity.py::test_gru_convolutions_in_the_minimal_filtering_form, "
           "per element against float64: test_hip_parity.py::test_slice_reg_step_every_form_against_float64",
        0: "direct GRU convolutions -- test_hip_parity.py::test_pipelined_recurrence_is_bit_identical_to_sequential, "
           "per element against float64: test_hip_parity.py::test_slice_reg_step_every_form_against_float64",
        1: "gates1 only -- test_hip_parity.py::test_gru_convolutions_in_the_minimal_filtering_form; the role in F(2x2, 3x3) per "
           "element (gru_wino = 15): test_hip_parity.py::test_slice_reg_step_every_form_against_float64",
        2: "gates2 only -- test_hip_parity.py::test_gru_convolutions_in_the_minimal_filtering_form; the role in F(2x2, 3x3) per "
           "element (gru_wino = 15): test_hip_parity.py::test_slice_reg_step_every_form_against_float64",
        4: "cand2 only -- test_hip_parity.py::test_gru_convolutions_in_the_minimal_filtering_form; the role in F(2x2, 3x3) per "
           "element (gru_wino = 15): test_hip_parity.py::test_slice_reg_step_every_form_against_float64",
        8: "cand1 only -- test_hip_parity.py::test_gru_convolutions_in_the_minimal_filtering_form; the role in F(2x2, 3x3) per "
           "element (gru_wino = 15): test_hip_parity.py::test_slice_reg_step_every_form_against_float64",
    },
    "recur_mode": {
        -1: "by stage size -- test_hip_parity.py::test_stage_on_random_shapes_against_oracle (per pixel against float64)",
        0: "one role per launch -- test_hip_parity.py::test_pipelined_recurrence_is_bit_identical_to_sequential, per pixel against "
           "float64: test_hip_parity.py::test_pipelined_recurrence_on_ragged_stage_sizes",
        1: "three launches per hypothesis -- test_hip_parity.py::test_pipelined_recurrence_is_bit_identical_to_sequential",
        3: "two launches per hypothesis -- test_hip_parity.py::test_pipelined_recurrence_is_bit_identical_to_sequential",
        5: "one launch per hypothesis -- test_hip_parity.py::test_pipelined_recurrence_is_bit_identical_to_sequential",
    },
}

WIDTHS = (16, 32, 48, 64, 96, 128, 192, 256, 384, 512)     # csrc/costreg2d.hip::costreg_depth_supported
WIDE = (96, 128, 192, 256, 384, 512)                       # tilings of two or four waves: the 2-row and fused-class forms exist
WIDTHS_BX3 = tuple(d for d in WIDTHS if d % 32 == 0)
# input maps per mode whose outputs are ragged for every block shape: 11 x 21 (8-row / 2-row blocks, 16 columns); stride 2:
# 7 x 19 outputs (S2P_ROWS = 3 too); transposed: 5 x 9 inputs (class-by-class blocks of 8 x 16 inputs, fused blocks of 2 rows)
RAGGED = {0: (11, 21), 1: (14, 38), 2: (5, 9)}
EDGES = {0: [(1, 1), (2, 2), (1, 18)], 1: [(2, 2), (4, 2)], 2: [(1, 1), (2, 2), (1, 2)]}
RULE_LIMIT = 2048          # costreg2d.hip::small_grid_rows2 and ::t2_fused: the small-grid forms up to 2048 blocks


def _case(precision, mode, D, N, hw, relu=1, skip=True, in2=None, **opts):
    if in2 is None:
        in2 = precision == 0 and mode != 1            # the entry point takes in2 for fp32, modes 0 and 2
    tag = "%s-m%d-D%d-N%d-%dx%d-relu%d%s%s" % ("fp32" if precision == 0 else "bx3", mode, D, N, hw[0], hw[1], relu,
                                             "-skip" if skip else "", "-in2" if in2 else "")
    tag += "".join("-%s=%d" % kv for kv in sorted(opts.items()))
    return pytest.param(precision, mode, D, N, hw[0], hw[1], relu, skip, in2, opts, id=tag)


def _cases():
    c = []
    for mode in (0, 1, 2):
        for D in WIDTHS:                                           # every width, default options
            c.append(_case(0, mode, D, 2, RAGGED[mode]))
        for relu in (0, 1):                                        # the epilogue's switches
            for skip in (False, True):
                for in2 in ((False, True) if mode != 1 else (False,)):
                    if (relu, skip, in2) != (1, True, mode != 1):      # (that one is the width case above)
                        c.append(_case(0, mode, 96, 2, RAGGED[mode], relu, skip, in2))
        c.append(_case(0, mode, 192, 5, RAGGED[mode], relu=0))
        for hw in EDGES[mode]:                                     # maps smaller than one block
            for D in (16, 64, 192, 512):
                c.append(_case(0, mode, D, 2, hw))
            c.append(_case(0, mode, 192, 2, hw, **({"t2_fused": 0} if mode == 2 else {"conv_rows2": 0})))
        for D in WIDE:                                             # the size-driven arms, forced
            for v in (0, 1):
                c.append(_case(0, mode, D, 2, RAGGED[mode], **({"t2_fused": v} if mode == 2 else {"conv_rows2": v})))
        for v in (0, 1):
            c.append(_case(0, mode, 256, 2, RAGGED[mode], conv256_split=v))
            c.append(_case(0, mode, 256, 2, RAGGED[mode], conv256_split=v, **({"t2_fused": 0} if mode == 2 else {"conv_rows2": 0})))
    for D in (192, 384):
        for v in (0, 1):
            c.append(_case(0, 2, D, 2, RAGGED[2], t2_kb8=v, t2_fused=0))
            c.append(_case(0, 2, D, 1, (2, 2), t2_kb8=v, t2_fused=0))
            # pair form: 32-column blocks (64 outputs: two), or from 256 columns (260: eight and a ragged one with an odd pair)
            c.append(_case(0, 1, D, 2, (14, 128), relu=v, skip=False, s2_pairs=v, conv_rows2=0))
            c.append(_case(0, 1, D, 1, (8, 520), relu=1 - v, skip=False, s2_pairs=v, conv_rows2=0))
    for D in (32, 64):                                             # the resident form off: the generic k_conv_dd<2 | 4, 1>
        c.append(_case(0, 0, D, 2, RAGGED[0], conv_small_grid=0))
        c.append(_case(0, 0, D, 3, (2, 2), relu=0, skip=False, in2=False, conv_small_grid=0))
    for mode in (0, 1, 2):                                         # split bf16 (bf16x3): no option reaches it
        for D in WIDTHS_BX3:
            c.append(_case(1, mode, D, 2, RAGGED[mode]))
        c.append(_case(1, mode, 96, 3, RAGGED[mode], relu=0, skip=False))
        for hw in EDGES[mode]:
            c.append(_case(1, mode, 64, 2, hw))
            c.append(_case(1, mode, 192, 1, hw, relu=0))
    return c


def _cl(t):
    """NCHW -> channel-last [N][h*w][C] on the GPU."""
    N, C, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(N, h * w, C).contiguous().cuda()


def _layer_inputs(mode, D, N, hi, wi, skip, in2, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, D, hi, wi, generator=g)
    x2 = torch.randn(N, D, hi, wi, generator=g) if in2 else None
    wt = torch.randn(D, D, 3, 3, generator=g) / (3 * D ** 0.5)      # [cout][cin] (transposed: [cin][cout])
    scale, shift = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.1
    ho, wo = (hi // 2, wi // 2) if mode == 1 else ((2 * hi, 2 * wi) if mode == 2 else (hi, wi))
    sk = torch.randn(N, D, ho, wo, generator=g) if skip else None
    return x, x2, wt, scale, shift, sk


def _reference(mode, x, x2, wt, scale, shift, relu, sk):
    """The layer in float64: conv2d / conv_transpose2d of x (+ in2) with BN folded, ReLU, + skip."""
    F = torch.nn.functional
    xx = x.double() + (x2.double() if x2 is not None else 0)
    if mode == 2:
        ref = F.conv_transpose2d(xx, wt.double() * scale.double().reshape(1, -1, 1, 1), shift.double(), stride=2, padding=1,
                                 output_padding=1)
    else:
        ref = F.conv2d(xx, wt.double() * scale.double().reshape(-1, 1, 1, 1), shift.double(), stride=1 + mode, padding=1)
    ref = torch.relu(ref) if relu else ref
    return ref + sk.double() if sk is not None else ref


@pytest.mark.parametrize("precision,mode,D,N,hi,wi,relu,skip,in2,opts", _cases())
def test_conv3x3_dd_forms(set_option, precision, mode, D, N, hi, wi, relu, skip, in2, opts):
    """adamvs_conv3x3_dd in every form the launcher can take (csrc/costreg2d.hip::launch_conv_dd_z, ::launch_conv_dd_cfg,
    csrc/costreg2d_bf16x3.hip::launch_conv_dd_bf16x3), each option forced through set_option, against float64 torch."""
    from ada_mvs_amd import hip_ops, packing
    for name, value in opts.items():
        set_option(name, value)
    x, x2, wt, scale, shift, sk = _layer_inputs(mode, D, N, hi, wi, skip, in2, seed=1000 * mode + D + 7 * N + hi + wi)
    ref = _reference(mode, x, x2, wt, scale, shift, relu, sk)
    ho, wo = ref.shape[-2:]
    pack = packing.pack_reg_layer if precision == 0 else packing.pack_reg_layer_bf16x3
    pk = pack(wt, scale, shift, mode == 2).cuda()
    out = hip_ops.conv3x3_dd(_cl(x), pk[:9 * D * D], pk[9 * D * D:], _cl(sk) if skip else None, N, D, hi, wi, mode, relu,
                             precision=precision, in2=_cl(x2) if in2 else None)
    got = out.cpu().double().reshape(N, ho, wo, D).permute(0, 3, 1, 2)
    err, worst = rel_l1(got, ref), float((got - ref).abs().max() / ref.abs().max())
    # fp32: the pair-form test's bars (test_hip_parity.py::test_stride_two_layer_in_the_pair_form); measured at most 9.0e-7 and
    # 2.8e-6 over these cases.  bf16x3 (16 significant bits per operand): measured at most 4.4e-6 and 4.8e-6
    rel_bar, max_bar = (2e-6, 2e-5) if precision == 0 else (1.5e-5, 1.5e-5)
    assert err < rel_bar and worst < max_bar, "rel_l1 %.3e, max|err| / max|ref| %.3e" % (err, worst)


def _layer(D, N, hi, wi, seed):
    from ada_mvs_amd import packing
    g = torch.Generator().manual_seed(seed)
    x = _cl(torch.randn(N, D, hi, wi, generator=g))
    pk = packing.pack_reg_layer(torch.randn(D, D, 3, 3, generator=g) / (3 * D ** 0.5), torch.rand(D, generator=g) + 0.5,
                                torch.randn(D, generator=g) * 0.1, False).cuda()
    return x, pk[:9 * D * D], pk[9 * D * D:]


def _outputs_by_option(set_option, name, D, N, hi, wi, mode, seed):
    from ada_mvs_amd import hip_ops
    x, w, b = _layer(D, N, hi, wi, seed)
    outs = {}
    for v in (-1, 0, 1):
        set_option(name, v)
        outs[v] = hip_ops.conv3x3_dd(x, w, b, None, N, D, hi, wi, mode, 1).cpu()
    return outs


@pytest.mark.parametrize("N", [RULE_LIMIT, RULE_LIMIT + 1])
def test_rows2_rule_boundary(set_option, N):
    """conv_rows2 = -1 takes the 2-row kernel while the 8-row grid has at most 2048 blocks.  A 5 x 13 map is one block of
    8 x 16, so N images are N blocks: 2048 falls on the 2-row side, 2049 on the other.  The default's output equals the
    forced arm of its side bit for bit.  The two arms are the same code (conv_dd_body with 2 or 8 rows per block: every pixel
    sums the same chunks and taps in the same order), so they agree bit for bit as well, and the output cannot tell which
    kernel ran; the kernel trace of this test shows k_conv_dd_rows2 at 2048 and k_conv_dd at 2049."""
    D, h, w = 96, 5, 13
    blocks8 = math.ceil(w / 16) * math.ceil(h / 8) * N           # the launcher's count (stride 1: output = input size)
    rows2 = blocks8 <= RULE_LIMIT
    assert rows2 == (N == RULE_LIMIT)
    outs = _outputs_by_option(set_option, "conv_rows2", D, N, h, w, 0, seed=N)
    assert torch.equal(outs[-1], outs[1 if rows2 else 0])
    assert torch.equal(outs[0], outs[1])
    assert float(outs[0].abs().max()) > 0


@pytest.mark.parametrize("N", [RULE_LIMIT, RULE_LIMIT + 1])
def test_t2_fused_rule_boundary(set_option, N):
    """t2_fused = -1 takes the fused-class transposed kernel while the class-by-class grid (8 x 16 input blocks) has at most
    2048 blocks; a 3 x 7 input is one block, so N images are N blocks.  The fused form sums a pixel's taps in another order
    than the class-by-class kernel: the two arms differ in their last bits, so the default's bits show which one ran."""
    D, h, w = 96, 3, 7
    blocks = math.ceil(w / 16) * math.ceil(h / 8) * N
    fused = blocks <= RULE_LIMIT
    assert fused == (N == RULE_LIMIT)
    outs = _outputs_by_option(set_option, "t2_fused", D, N, h, w, 2, seed=N + 1)
    assert torch.equal(outs[-1], outs[1 if fused else 0])
    assert not torch.equal(outs[0], outs[1])
    assert float(outs[0].abs().max()) > 0


# k_softmax_regress keeps NQ = ceil(D / 64) quads per lane in registers (NQ in 1, 2, 3, 4, 6, 8); other D take the two-pass
# NQ = 0 loop.  A workgroup walks 16-pixel groups over a grid of at most the resident capacity: at most 32 waves per CU, i.e.
# 8 workgroups of 256 threads on each of 256 CUs, 16 pixels each.
SOFTMAX_PIXELS_PER_TURN = 8 * 256 * 16


@pytest.mark.parametrize("D,h,w", [(20, 8, 10), (48, 7, 9), (64, 8, 10), (100, 7, 9), (128, 8, 10), (192, 7, 9), (256, 8, 10),
                                   (384, 7, 9), (512, 8, 10), (320, 8, 10), (448, 7, 9),      # 448, 320: NQ = 0
                                   (64, 130, 136), (320, 131, 137), (512, 131, 137)])          # the grid-stride loop turns
def test_softmax_max_regress_unfused(D, h, w):
    """adamvs_softmax_max_regress (k_softmax_regress<NQ>, what option fuse_softmax = 0 runs behind the scores) against the
    oracle in float64: every NQ instantiation and the generic loop, maps whose h*w is a multiple of 16 (every group of 16
    pixels staged through LDS) and not (groups across two maps read the planes directly), two batch items with different
    depth ranges, rows with one dominant logit (+60 over the rest, or one channel over -60 everywhere else)."""
    from ada_mvs_amd import hip_ops
    from oracle import adamvs_oracle as O
    S, B = 2, 2
    g = torch.Generator().manual_seed(D + h)
    score = torch.randn(S * B, D, h, w, generator=g) * 3
    score[:, (D * 5) // 7, ::7, ::5] = 60.0
    score[:, :, 3::11, :] = -60.0
    score[:, D // 3, 3::11, :] = 0.0
    planes = O.depth_range_samples(torch.tensor([[400.0, 600.0], [380.0, 650.0]]), D, 0.0, [B, h, w])
    if h * w > 1000:
        assert S * B * h * w > 2 * SOFTMAX_PIXELS_PER_TURN
    vw, pd = hip_ops.softmax_max_regress(_cl(score), planes.cuda(), S, B, D, h, w)
    vw, pd = vw.cpu().double().reshape(S, B, h, w), pd.cpu().double().reshape(S, B, h, w)
    for s in range(S):
        rvw, rpd = O.softmax_max_regress(score[s * B:(s + 1) * B].double(), planes.double())
        rvw = rvw[:, 0]
        assert rel_l1(vw[s], rvw) < 1e-5 and rel_l1(pd[s], rpd) < 1e-5
        # per pixel: measured at most 3.2e-7 (view weight) and 4.1e-7 (depth) of the largest reference value
        assert float((vw[s] - rvw).abs().max()) < 2e-6 * float(rvw.abs().max()), float((vw[s] - rvw).abs().max())
        assert float((pd[s] - rpd).abs().max()) < 2e-6 * float(rpd.abs().max()), float((pd[s] - rpd).abs().max())
