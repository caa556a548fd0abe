"""tests/fp64_bars.py without a GPU: the per-element bars catch what the mean bars of the GPU tests let through, the oracles
run a whole stage in float64, and the MS-REDNet recurrence bars can be met by a correct fp32 implementation that is not the code
under test."""
import pytest
import torch

import fp64_bars
from conftest import rel_l1

OP_TOL = 5e-5          # test_hip_parity.py: the mean relative L1 the fp32 kernels were held to before these bars
BX3_TOL = 2e-4         # and the split-bf16 ones
RED_TOL = 2e-5         # test_msrednet.py: OP_TOL, the mean the MS-REDNet ops are held to
BARS = {name: getattr(fp64_bars, name) for name in ("FEATNET", "PAIR_SIM", "SWEEP", "STEP", "SWEEP_BX3", "STEP_BX3",
                                                    "RED_PAIR", "RED_SPLIT", "RED_APPLY", "RED_CELL", "RED_CONV", "RED_STEP")}
# the variance bars of the small maps (the large maps' bars, up to 2.4e-4 for fp32 tap positions on 128 x 256, are beyond what the
# old mean passes on a whole plane)
BARS.update({"RED_VARIANCE_%s_small" % kind: fp64_bars.RED_VARIANCE[(kind, "small")] for kind in ("rig150", "border")})


def _reference():
    """A sweep-shaped float64 map [plane, n, c, y, x]: 19 planes of 2 x 8 x 14 x 42."""
    return torch.randn(19, 2, 8, 14, 42, generator=torch.Generator().manual_seed(0), dtype=torch.float64)


@pytest.mark.parametrize("name", sorted(BARS))
@pytest.mark.parametrize("where,index,at", [("one element", (7, 1, 3, 5, 9), "plane=7, n=1, c=3, y=5, x=9"),
                                            ("one border column", (Ellipsis, 41), "x=41"),
                                            ("one plane", (7,), "plane=7")])
def test_bars_catch_what_the_mean_let_through(name, where, index, at):
    """2x the max bar on one element, one border column or one plane: the old mean bar passes it, the comparator fails it and
    names the place."""
    max_bar, mean_bar = BARS[name]
    ref = _reference()
    got = ref.clone()
    got[index] += 2 * max_bar * float(ref.abs().max())
    assert rel_l1(got, ref) < (BX3_TOL if name.endswith("BX3") else RED_TOL if name.startswith("RED_") else OP_TOL), where
    with pytest.raises(AssertionError, match=at):
        fp64_bars.check(got, ref, max_bar, mean_bar, dims=("plane", "n", "c", "y", "x"))
    fp64_bars.check(ref.float(), ref, max_bar, mean_bar)            # fp32 rounding of the reference passes


def test_failure_names_the_fraction_over_the_bar_and_nan_fails():
    ref = _reference()[0]
    got = ref.clone()
    got[..., 0] += 1.0
    with pytest.raises(AssertionError, match=r"at \(n=\d+, c=\d+, y=\d+, x=0\).* 2\.38% of 9408 elements"):
        fp64_bars.check(got, ref, 1e-3)
    got = ref.clone()
    got[1, 2, 3, 4] = float("nan")
    with pytest.raises(AssertionError, match="n=1, c=2, y=3, x=4"):
        fp64_bars.check(got, ref, 1e-3)
    with pytest.raises(AssertionError, match="float64"):
        fp64_bars.check(ref, ref.float(), 1e-3)
    assert fp64_bars.check(ref + 0.5, ref + 0.5, 1e-12) == (0.0, 0.0)


def test_oracle_stage_in_float64():
    """oracle.infer_depth_stage in float64 (states and sums take the inputs' dtype) agrees with the fp32 run to fp32 rounding;
    the fp32 run itself is pinned by tests/test_oracle_golden.py."""
    from ada_mvs_amd import synth
    from ada_mvs_amd.models.adamvs import Infer_AdaMVSNet
    from oracle import adamvs_oracle as O
    B, V, D, h, w = 2, 3, 5, 6, 8
    m = Infer_AdaMVSNet(48, [48, 32, 8], synth.DEPTH_INTERVALS_RATIO, False, [8, 8, 8])
    sd = synth.seeded_state_dict(m, seed=0)
    feats = [synth.smooth_features(B, 16, h, w, seed=v) for v in range(V)]
    proj = synth.rig_projections(V, 4 * h, 4 * w, batch=B)["stage1"]
    planes = (430.0 + 4.0 * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)).expand(B, D, h, w).contiguous()
    prev = [torch.rand(B, 1, h // 2, w // 2, generator=torch.Generator().manual_seed(v)) for v in range(V - 1)]
    ref32 = O.infer_depth_stage(feats, proj, planes, sd, "DepthNet.1.", True, prev)
    ref64 = O.infer_depth_stage([f.double() for f in feats], proj.double(), planes.double(), fp64_bars.double_sd(sd), "DepthNet.1.", True,
                                [c.double() for c in prev])
    for key in ("depth", "photometric_confidence"):
        assert ref64[key].dtype == torch.float64 and ref32[key].dtype == torch.float32
        fp64_bars.check(ref32[key], ref64[key], 1e-5, 1e-6, what=key)


def _recurrence_cases(entry, limit=40000):
    """The (level, C, B, h, w, D) of the GPU cases of tests/test_msred_forms.py with at most `limit` pixels over the batch."""
    import test_msred_forms as forms
    if entry == "pair":
        cases = {c[:6] for c in forms._pair_cases()}
    else:
        cases = {(c[0], 32) + c[1:5] for c in forms._split_cases()}
    return sorted(c for c in cases if c[2] * c[3] * c[4] <= limit)


@pytest.mark.parametrize("entry,bar", [("pair", "RED_PAIR"), ("split", "RED_SPLIT")])
def test_recurrence_bars_hold_for_another_fp32_evaluation(entry, bar):
    """The recurrence bars are 4x the fp32 oracle's distance from float64.  A second fp32 evaluation in another summation order
    (tests/msred_ref.py::recurrence_unfold: convolutions as unfold + matmul, GroupNorm from sum and sum of squares) passes them on
    the inputs of the GPU cases, and so does the fp32 oracle itself, with the margin the rule promises (under half the bar)."""
    import msred_ref
    max_bar, mean_bar = getattr(fp64_bars, bar)
    cases = _recurrence_cases(entry)
    assert len(cases) >= 8 and {c[0] for c in cases} == ({1, 2} if entry == "pair" else {3, 4})
    for level, C, B, h, w, D in cases:
        sd, xs = msred_ref.recur_inputs(level, C, B, h, w, D)
        ref = torch.stack(msred_ref.recurrence(level, msred_ref.to_dtype(xs, torch.float64), fp64_bars.double_sd(sd)))
        what = "level %d C=%d B=%d %dx%d D=%d" % (level, C, B, h, w, D)
        fp64_bars.check(torch.stack(msred_ref.recurrence_unfold(level, xs, sd)), ref, max_bar, mean_bar, what="unfold + matmul, " + what,
                        dims=("plane", "n", "c", "y", "x"))
        fp64_bars.check(torch.stack(msred_ref.recurrence(level, xs, sd)), ref, max_bar / 2, mean_bar / 2, what="fp32 oracle, " + what,
                        dims=("plane", "n", "c", "y", "x"))


def test_unfold_evaluation_is_another_summation_order():
    """recurrence_unfold is not the oracle under another name: same values to fp32 rounding, other bits."""
    import msred_ref
    for level in (2, 3):
        sd, xs = msred_ref.recur_inputs(level, 32 if level == 3 else 16, 2, 13, 19, 3)
        a, b = torch.stack(msred_ref.recurrence(level, xs, sd)), torch.stack(msred_ref.recurrence_unfold(level, xs, sd))
        assert not torch.equal(a, b) and float((a - b).abs().max()) < 1e-5


def test_msred_soft_argmin_reference_is_the_oracle_loop():
    """msred_ref.soft_argmin on the volume a stage produces = oracle.infer_depth_stage_red's own depth and confidence, bit for bit
    (fp32): the reference of the soft-argmin test is lines of the oracle, not a second opinion."""
    import msred_ref
    from oracle import msrednet_oracle as mo
    feats, proj, planes, sd = _red_stage_inputs()
    want = mo.infer_depth_stage_red(feats, proj, planes, sd, "")
    rel = [mo.ao.relative_transform(proj[:, v], proj[:, 0]) for v in range(1, len(feats))]
    states = [torch.zeros(2, 8 << k, 8 >> k, 16 >> k) for k in range(4)]
    vol = []
    for d in range(planes.shape[1]):
        cost = mo.variance_cost(feats[0], feats[1:], [r[0] for r in rel], [r[1] for r in rel], planes[:, d:d + 1])
        reg, states = mo.slice_red_step(cost, states, sd, "")
        vol.append(reg)
    depth, conf = msred_ref.soft_argmin(torch.cat(vol, 1), planes)
    assert torch.equal(depth, want["depth"]) and torch.equal(conf, want["photometric_confidence"])


def _red_stage_inputs():
    import msred_ref
    from ada_mvs_amd import synth
    B, V, D, h, w = 2, 3, 5, 8, 16
    sd = msred_ref.red_state_dict(16, seed=0)
    feats = [synth.smooth_features(B, 16, h, w, seed=v) for v in range(V)]
    proj = synth.rig_projections(V, 4 * h, 4 * w, batch=B)["stage1"]
    planes = (430.0 + 4.0 * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)).expand(B, D, h, w).contiguous()
    return feats, proj, planes, sd


def test_msred_oracle_stage_in_float64():
    """oracle.infer_depth_stage_red in float64 (states and sums take the inputs' dtype) returns float64 and agrees with the fp32 run
    to fp32 rounding; the fp32 run itself is pinned by the golden tests of tests/test_msrednet.py."""
    from oracle import msrednet_oracle as mo
    feats, proj, planes, sd = _red_stage_inputs()
    ref32 = mo.infer_depth_stage_red(feats, proj, planes, sd, "")
    ref64 = mo.infer_depth_stage_red([f.double() for f in feats], proj.double(), planes.double(), fp64_bars.double_sd(sd), "")
    for key in ("depth", "photometric_confidence"):
        assert ref64[key].dtype == torch.float64 and ref32[key].dtype == torch.float32
        fp64_bars.check(ref32[key], ref64[key], 1e-5, 1e-6, what=key)


def test_msred_path_rule_at_the_documented_boundaries():
    """tests/test_msred_forms.py labels its cases by a restatement of the launchers' rule (pair_path, split_path).  Worked from the
    launchers as they stand: one sample, 128 x 256 is the last map with epilogue partials (2048) and 132 x 256 the
    first without; at three samples 84 x 256 has them and 88 x 256 does not.  D = 32 at the default conv_small_grid of 1024 and two
    samples: 80 x 256 runs NTR = 2 and 160 x 256 NTR = 4, both with 1280 partials; one sample of 100 x 256 runs NTR = 1 with 3200
    partials, more than the buffer holds."""
    from test_msred_forms import pair_path, split_path
    assert pair_path(1, 128, 256, -1) == "folded" and pair_path(1, 128, 256, 0) == "epilogue" and pair_path(1, 132, 256, -1) == "gn_partial"
    assert pair_path(3, 84, 256, -1) == "epilogue" and pair_path(3, 84, 256, 1) == "folded" and pair_path(3, 88, 256, 1) == "gn_partial"
    assert split_path(3, 2, 80, 256, -1, 1024) == "folded-dual_ntr2" and split_path(3, 2, 160, 256, 0, 1024) == "epilogue-dual_ntr4"
    assert split_path(4, 2, 40, 256, -1, 1024) == "folded-dual_ntr2" and split_path(4, 2, 80, 256, -1, 1024) == "folded-dual_ntr4"
    assert split_path(3, 1, 100, 256, -1, 1024) == "gn_partial-single_ntr1" and split_path(4, 1, 50, 256, -1, 1024) == "gn_partial-single_ntr1"
    assert split_path(3, 2, 37, 53, -1, 0) == "gn_partial-generic"
