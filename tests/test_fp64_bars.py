"""tests/fp64_bars.py without a GPU: the per-element bars catch what the mean bars of the GPU tests let through, and the oracle
runs a whole stage in float64."""
import pytest
import torch

import fp64_bars
from conftest import rel_l1

OP_TOL = 5e-5          # test_hip_parity.py: the mean relative L1 the fp32 kernels were held to before these bars
BX3_TOL = 2e-4         # and the split-bf16 ones
BARS = {name: getattr(fp64_bars, name) for name in ("FEATNET", "PAIR_SIM", "SWEEP", "STEP", "SWEEP_BX3", "STEP_BX3")}


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
    assert rel_l1(got, ref) < (BX3_TOL if name.endswith("BX3") else OP_TOL), where
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
