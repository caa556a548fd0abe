"""The two byte-saving forms of the fp32 recurrence (csrc/slice_roles_wino.h Gates1Conv2WinoRole, csrc/slice_roles.h
TwoRowPairRole<., 2>): conv2 of hypothesis t - 1 formed inside the level-1 gate launch of hypothesis t, out of the window that launch
holds anyway, and the level-1 candidate on 8 x 32 tiles.  Both reorder launches and tiles, not sums: every map must equal, bit for
bit, the one of the launches of before (option gru_wino with bits 16 and 32 set), which in turn is held to the float64 bars of
tests/test_hip_parity.py.

The switches are bits of option gru_wino (include/adamvs_hip.h, OPTIONS).  Two are set = the form of before:
    conv2 inside gates1 (schedule 0) <=> bit 16 clear,    cand1 on 8 x 32 tiles <=> bit 32 clear;
one is an opt-in: slot A of the three-launch schedule (recur_mode 1) is the gate role with conv2 inside <=> bit 64 set.
"""
import ctypes

import pytest
import torch

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, synth
from conftest import rel_l1

CONV2_APART, CAND1_TILE16, SLOT_A_FUSED = 16, 32, 64


def _gru_wino(conv2_in_gates1, cand1_tile32):
    """conv2 inside the level-1 gate tiles wherever a schedule can have it (0: its own launch / its own workgroups of slot A)"""
    return 7 | (SLOT_A_FUSED if conv2_in_gates1 else CONV2_APART) | (0 if cand1_tile32 else CAND1_TILE16)


def dev(t):
    return t.cuda().contiguous()


@pytest.fixture(scope="module")
def hip():
    from ada_mvs_amd import hip_ops
    _lib.load()
    assert torch.cuda.is_available()
    return hip_ops


@pytest.fixture(scope="module")
def O():
    from oracle import adamvs_oracle
    return adamvs_oracle


def _stage_case(stage, B, V, h, w, D, seed):
    from ada_mvs_amd.models.adamvs import Infer_AdaMVSNet
    m = Infer_AdaMVSNet(48, [48, 32, 8], synth.DEPTH_INTERVALS_RATIO, False, [8, 8, 8])
    sd = synth.seeded_state_dict(m, seed=0)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    net = m.DepthNet[stage]
    C = (32, 16, 8)[stage]
    feats = [synth.smooth_features(B, C, h, w, seed=seed + v) for v in range(V)]
    proj = synth.rig_projections(V, 4 * h, 4 * w, batch=B)["stage1"]
    g = torch.Generator().manual_seed(seed)
    near = 420.0 + 20.0 * torch.rand(B, 1, h, w, generator=g)
    planes = (near + 4.0 * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)).contiguous()
    prev = [torch.rand(B, 1, h // 2, w // 2, generator=g) for _ in range(V - 1)]
    return net, sd, feats, proj, planes, prev


def _run(net, feats, proj, planes, D, prev):
    with torch.no_grad():
        out = net([dev(f) for f in feats], dev(proj), dev(planes), D, [dev(c) for c in prev])
    torch.cuda.synchronize()
    return {k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v] if isinstance(v, (list, tuple)) else v) for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("D", [40, 2])
@pytest.mark.parametrize("stage,h,w", [(1, 22, 38), (2, 26, 50), (1, 4, 6), (1, 8, 32)])
def test_bit_identity_at_sizes_no_tile_divides(hip, O, set_option, stage, h, w, D):
    """One cascade stage (InferDepthNet0.forward, reference adamvs.py:433-533), B = 2, 3 views, fp32, on maps no tile divides (level-2
    maps of 11 x 19, 13 x 25, 2 x 3) and on 8 x 32, exactly one gate tile whose whole ring is padding.  D = 40 is a full chunk of 32
    hypotheses plus a ragged one: level 2 and the decoder, one hypothesis behind level 1, cross the chunk boundary and the soft-argmin
    of a chunk follows its last decoder; D = 2 is first step and drain and nothing else.  Under recur_mode 0 and 1, with each of the
    two forms on and off, depth and confidence equal those of the launches of before; those meet the oracle (per pixel in float64
    too, at the bars of tests/fp64_bars.py)."""
    from test_hip_parity import E2E_TOL, _check_stage64
    net, sd, feats, proj, planes, prev = _stage_case(stage, 2, 3, h, w, D, seed=70)
    outs = {}
    for mode in (0, 1):
        set_option("recur_mode", mode)
        for a in (0, 1):
            for b in (0, 1):
                set_option("gru_wino", _gru_wino(a, b))
                outs[mode, a, b] = _run(net, feats, proj, planes, D, prev)
    base = outs[0, 0, 0]
    for key, got in outs.items():
        for k in ("depth", "photometric_confidence"):
            assert torch.equal(got[k], base[k]), (key, k, float((got[k] - base[k]).abs().max()))
    with torch.no_grad():
        ref = O.infer_depth_stage(feats, proj, planes, sd, "DepthNet.%d." % stage, net.in_up, prev)
    for k in ("depth", "photometric_confidence"):
        assert base[k].shape == ref[k].shape
        assert rel_l1(base[k], ref[k]) < E2E_TOL, k
    _check_stage64(O, base, feats, proj, planes, sd, stage, net.in_up, prev, 4.0, "fp32")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [24, 48])
def test_many_tiles_per_workgroup(hip, set_option, B):
    """One stage (C = 16) on 64 x 96 maps, D = 3: at B = 24 the 8 x 16 tile loop of the candidate is past the resident capacity of a
    256-CU device (1152 tiles for at most 1024 workgroups), at B = 48 the 8 x 32 loops of the gate launch and of the new candidate
    too (1152 tiles), so a workgroup walks several tiles, interior and edge ones, with the next window in flight.  The same maps
    bit for bit with both forms on and off."""
    net, sd, feats, proj, planes, prev = _stage_case(1, B, 3, 64, 96, 3, seed=80)
    set_option("recur_mode", 0)
    set_option("gru_wino", _gru_wino(0, 0))
    base = _run(net, feats, proj, planes, 3, prev)
    for a, b in ((1, 1), (1, 0), (0, 1)):
        set_option("gru_wino", _gru_wino(a, b))
        got = _run(net, feats, proj, planes, 3, prev)
        for k in ("depth", "photometric_confidence"):
            assert torch.equal(got[k], base[k]), (a, b, k, float((got[k] - base[k]).abs().max()))
    assert bool(torch.isfinite(base["depth"]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("recur_mode", [-1, 0])
def test_captured_forward_replays_bit_identical(hip, set_option, recur_mode):
    """The end-to-end model at cfg `tiny`, batch 3, options at their defaults (and with recur_mode 0, which puts every stage on the
    five-launch schedule): a hipGraph captured on one sample and replayed on others equals the eager forward bit for bit -- the state
    rings and the lag of level 2 depend on nothing the previous replay left."""
    from ada_mvs_amd.graphed import GraphedForward
    from ada_mvs_amd.models.adamvs import Infer_AdaMVSNet
    if recur_mode != -1:
        set_option("recur_mode", recur_mode)
    c = synth.CONFIGS["tiny"]
    m = Infer_AdaMVSNet(c["num_depth"], c["ndepths"], synth.DEPTH_INTERVALS_RATIO, False, [8, 8, 8])
    m.load_state_dict(synth.seeded_state_dict(m, seed=0))
    m = m.cuda().eval()
    fwd = GraphedForward(m)
    for i, seed in enumerate((0, 1, 2)):
        imgs, proj, dv = synth.tile_inputs("tiny", batch=3, seed=seed, baseline=8.0 + seed)
        args = (dev(imgs), {k: dev(v) for k, v in proj.items()})
        with torch.no_grad():
            want = m(*args, dev(dv))
            want = {s: {k: want[s][k].clone() for k in ("depth", "photometric_confidence")} for s in ("stage1", "stage2", "stage3")}
            got = fwd(*args, dv)
        torch.cuda.synchronize()
        for s in ("stage1", "stage2", "stage3"):
            for k in ("depth", "photometric_confidence"):
                assert torch.equal(got[s][k], want[s][k]), (i, s, k)
    assert fwd.captures == 1


def test_schedule_report_and_switches_without_a_gpu():
    """adamvs_recurrence_schedule keeps reporting 0 (one role per launch) for the large stages although conv2 now rides in the gate
    launch (bench.py reads it); the two switches round-trip through adamvs_set_option / adamvs_get_option as bits of gru_wino and
    leave the F(2x2, 3x3) mask as it was."""
    lib = _lib.load()
    v = ctypes.c_int(0)
    assert lib.adamvs_option_default(b"gru_wino", ctypes.byref(v)) == 0 and v.value == 7        # schedule 0: both forms on by default
    assert lib.adamvs_recurrence_schedule(0, 256 * 96 * 192) == 0
    for a in (0, 1):
        for b in (0, 1):
            with _lib.options(gru_wino=_gru_wino(a, b)):
                assert _lib.get_option("gru_wino") == _gru_wino(a, b) and lib.adamvs_gru_wino_mask() & 15 == 7
                assert lib.adamvs_recurrence_schedule(0, 256 * 96 * 192) == 0
    assert _lib.get_option("gru_wino") == 7
