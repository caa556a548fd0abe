"""The F(2x4, 3x3) form of a stride-1 CostRegNet2D layer (csrc/costreg2d_wino24.hip) on the GPU: the layer against a float64
convolution and the direct kernel, `prob` with the softmax partials behind it, the three tilings bit for bit, and the network with
and without the form (option winograd 1 / 3)."""
import pytest
import torch

from conftest import rel_l1
from fp64_bars import STAGE_CONF, STAGE_DEPTH, check, double_sd
import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import packing, synth

pytestmark = pytest.mark.gpu

# max |err| / max |ref| of one layer against float64, over every case below (the three tilings give the same bits): measured at most
# 2.93e-6 on the MI355X (D = 512; F(2x2, 3x3): 5.8e-7 -- the column transform has the factors 4, 5, 8 and 1/24); the bar is just
# under 4x that, the convention of tests/fp64_bars.py
LAYER_MAX = 1.1e-5


@pytest.fixture(scope="module")
def hip():
    from ada_mvs_amd import hip_ops, _lib
    _lib.load()
    assert torch.cuda.is_available()
    return hip_ops


def dev(t):
    return t.cuda().contiguous()


def layer_case(N, D, h, w, relu, skip):
    """Inputs drawn as in test_hip_parity.py::test_conv3x3_dd_winograd, the float64 reference with them."""
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


# smaller than one 2 x 4 tile (and w < 4); exactly one 4 x 64 block; ragged in x by 2, 3, 1 columns of a tile and in y by a row;
# 1152 tiles for 512 resident workgroups (a workgroup walks several, the next tile's requests in flight); every width once
@pytest.mark.parametrize("N,D,h,w,relu,skip", [(1, 192, 3, 5, 1, False), (1, 192, 2, 3, 0, True), (1, 192, 4, 64, 1, False),
                                               (3, 192, 26, 70, 1, False), (2, 192, 7, 67, 0, True), (1, 192, 5, 129, 1, True),
                                               (12, 192, 32, 128, 1, False), (1, 64, 8, 40, 1, False), (1, 128, 13, 33, 0, True),
                                               (1, 256, 6, 32, 0, False), (1, 384, 5, 66, 1, False), (1, 512, 7, 34, 1, True)])
def test_conv3x3_dd_wino24(hip, N, D, h, w, relu, skip):
    """The layer against a float64 convolution (ConvBnReLU.forward, reference models/module.py:254-261, BN folded) and against the
    direct kernel.  rel-L1 2e-6 is the bar this layer has in every form (test_hip_parity.py::test_conv3x3_dd_winograd)."""
    x, wt, scale, shift, sk, ref = layer_case(N, D, h, w, relu, skip)
    x_cl = dev(x.permute(0, 2, 3, 1).reshape(N, h * w, D).contiguous())
    pk = dev(packing.pack_reg_layer(wt, scale, shift, False))
    out = hip.conv3x3_dd_wino24(x_cl, dev(packing.pack_reg_layer_wino24(wt, scale)), dev(shift), dev(sk) if skip else None, N, D, h, w, relu)
    direct = hip.conv3x3_dd(x_cl, pk[:9 * D * D], pk[9 * D * D:], dev(sk) if skip else None, N, D, h, w, 0, relu)
    back = lambda y: y.cpu().double().reshape(N, h, w, D).permute(0, 3, 1, 2)      # noqa: E731
    e64, edir = rel_l1(back(out), ref), rel_l1(back(out), back(direct))
    emax = float((back(out) - ref).abs().max() / ref.abs().max())
    print("wino24 %s: rel-L1 %.3e against float64, %.3e against the direct kernel, max|err|/max|ref| %.3e" % ((N, D, h, w, relu, skip), e64, edir, emax))
    assert e64 < 2e-6                                       # measured 3.5e-7 ... 9.6e-7 at D <= 192, 1.24e-6 at D = 384
    assert edir < 2e-6                                      # measured 4.4e-7 ... 1.59e-6
    check(back(out), ref, LAYER_MAX, what="layer, per element")


def test_the_three_tilings_give_the_same_bits(hip, set_option):
    """Two workgroups per CU with 2 channel tiles x 2 tile rows (the default) or 4 x 1, one workgroup with 4 x 2; `prob` with the
    softmax partials takes 4 x 1 or 4 x 2.  Option wino_wps forces one: the same layer through all, bit for bit."""
    g = torch.Generator().manual_seed(3)
    N, D, h, w = 3, 192, 26, 70
    x = dev(torch.randn(N, h * w, D, generator=g))
    wk = dev(packing.pack_reg_layer_wino24(torch.randn(D, D, 3, 3, generator=g) / 72, torch.ones(D)))
    bias, rng = dev(torch.randn(D, generator=g) * 0.1), dev(torch.tensor([[400.0, 580.0]]))
    outs, sms = [], []
    for wps in (0, 1, 2):
        set_option("wino_wps", wps)
        outs.append(hip.conv3x3_dd_wino24(x, wk, bias, None, N, D, h, w, 1).cpu())
        sms.append([t.cpu() for t in hip.prob_softmax_regress_wino24(x, wk, bias, rng, N, 1, D, h, w)])
    assert float(outs[0].abs().max()) > 0
    for k in (1, 2):
        assert torch.equal(outs[0], outs[k]), k
        assert torch.equal(sms[0][0], sms[k][0]) and torch.equal(sms[0][1], sms[k][1]), k


@pytest.mark.parametrize("D,h,w", [(192, 5, 70), (192, 8, 128), (384, 9, 33)])
def test_prob_softmax_regress_wino24(hip, D, h, w):
    """adamvs_prob_softmax_regress_wino24 -- `prob` in the F(2x4, 3x3) form, every lane's softmax partial in its epilogue, the merge
    kernel behind it (reference adamvs.py:238, 481-486) -- against float64 and against the layer + softmax / regression as two
    ops, with the bars of test_hip_parity.py::test_prob_softmax_regress_winograd: a ragged map and a map of whole blocks at D = 192;
    six channel groups per pixel (D = 384) against the two ops only, which is what that test holds there: against float64 the view
    weight is off by at most 1.07e-5 at D = 384 (rel-L1 1.9e-6) -- the error of a logit grows with the 9 D products behind it, and the
    1e-5 of that test was set for two fp32 evaluations of the same scores.  D = 192 against float64: rel-L1 1.3e-6 / 1.4e-7, max 8.2e-6 /
    2.6e-6; against the two ops, every case: 6.1e-8 / 8.6e-8, 3.6e-7 / 4.9e-7.  (Fewer planes than channels: the stage test below.)"""
    S, B = 2, 2
    g = torch.Generator().manual_seed(D + h)
    x = torch.randn(S * B, h * w, D, generator=g)
    wt = torch.randn(D, D, 3, 3, generator=g) * (2.0 / (9 * D)) ** 0.5 * 3.0                 # gain 3 on the logits layer, as in synth
    bias = torch.randn(D, generator=g) * 0.3
    wk = dev(packing.pack_reg_layer_wino24(wt, torch.ones(D)))
    rng = torch.tensor([[400.0, 580.0], [350.0, 610.0]])                                      # first and last plane of the two tiles
    step = (rng[:, 1] - rng[:, 0]) / (D - 1)
    planes = (rng[:, 0].view(B, 1, 1, 1) + torch.arange(D, dtype=torch.float32).view(1, D, 1, 1) * step.view(B, 1, 1, 1)).expand(B, D, h, w).contiguous()
    score64 = torch.nn.functional.conv2d(x.double().reshape(S * B, h, w, D).permute(0, 3, 1, 2), wt.double(), bias.double(), padding=1)
    p64 = torch.softmax(score64, 1).reshape(S, B, D, h, w)
    vw64, pd64 = p64.max(2)[0], (p64 * planes.double()[None]).sum(2)
    score = hip.conv3x3_dd_wino24(dev(x), wk, dev(bias), None, S * B, D, h, w, 0)
    vw0, pd0 = hip.softmax_max_regress(score, dev(planes), S, B, D, h, w)
    vw1, pd1 = hip.prob_softmax_regress_wino24(dev(x), wk, dev(bias), dev(rng), S, B, D, h, w)
    torch.cuda.synchronize()
    for name, vw_r, pd_r in (("float64", vw64, pd64), ("two ops", vw0, pd0)):
        if name == "float64" and D != 192:
            continue
        figs = (rel_l1(vw1, vw_r), rel_l1(pd1, pd_r), float((vw1.cpu().double() - vw_r.cpu().double()).abs().max()),
                float((pd1.cpu().double() - pd_r.cpu().double()).abs().max() / 500.0))
        print("wino24 softmax %s against %s: rel-L1 %.3e %.3e, max %.3e %.3e" % ((D, h, w), name, *figs))
        assert figs[0] < 2e-6 and figs[1] < 2e-6, name
        assert figs[2] < 1e-5 and figs[3] < 1e-5, name


def _stage(hip, net, feats, proj, rng, D):
    B, C, h, w = feats[0].shape
    feat_cl = hip.pack_features(dev(torch.stack(list(feats), 0).reshape(-1, C, h, w)))
    vw, pd, depth, conf = net.run(feat_cl, B, C, h, w, hip.relative_transforms(dev(proj)), None, None,
                                  planes=hip.plane_source(dev(rng), D, 0.0, [B, h, w]), num_depth=D)
    torch.cuda.synchronize()
    return net._as_dict(vw, pd, depth, conf, D)


def stage_both_ways(hip, set_option, D):
    """The first stage on an 8 x 128 map with D uniform planes under option winograd = 1 and 3 -> ({value: maps}, float64 oracle, interval)."""
    from oracle import adamvs_oracle as O
    from ada_mvs_amd.models.adamvs import Infer_AdaMVSNet
    B, V, C, h, w = 1, 2, 32, 8, 128
    m = Infer_AdaMVSNet(D, [D, 32, 8], synth.DEPTH_INTERVALS_RATIO, False, [8, 8, 8])
    sd = synth.seeded_state_dict(m, seed=5)
    m.load_state_dict(sd)
    net = m.cuda().eval().DepthNet[0]
    feats = [synth.smooth_features(B, C, h, w, seed=70 + v) for v in range(V)]
    proj = synth.rig_projections(V, 4 * h, 4 * w, batch=B)["stage1"]
    rng = torch.tensor([[420.0, 580.0]])
    interval = 160.0 / (D - 1)
    planes = (rng[:, :1, None, None] + interval * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)).expand(B, D, h, w).contiguous()
    got = {}
    with torch.no_grad():
        for value in (1, 3):
            set_option("winograd", value)
            got[value] = _stage(hip, net, feats, proj, rng, D)
        ref = O.infer_depth_stage([f.double() for f in feats], proj.double(), planes.double(), double_sd(sd), "DepthNet.0.", net.in_up, None)
    for value in (1, 3):
        worst = lambda key, i, scale: float((got[value][key][i].cpu().double().reshape(ref[key][i].shape) - ref[key][i]).abs().max() / scale)   # noqa: E731
        print("wino24 stage, %d planes, winograd=%d: depth %.3e intervals, pair depth %.3e intervals, confidence %.3e, pair confidence %.3e" % (
            D, value, float((got[value]["depth"].cpu().double() - ref["depth"]).abs().max() / interval), worst("pair_result", 0, interval),
            float((got[value]["photometric_confidence"].cpu().double() - ref["photometric_confidence"]).abs().max()), worst("pair_confidence", 0, 1.0)))
    return got, ref, interval


@pytest.fixture(scope="module")
def stage100(hip):
    """The stage at 100 planes both ways and its float64 oracle, once for the tests below."""
    from ada_mvs_amd import _lib
    saved = _lib.get_option("winograd")
    try:
        return stage_both_ways(hip, _lib.set_option, 100)
    finally:
        _lib.set_option("winograd", saved)


def test_stage_with_and_without_the_form(stage100):
    """The first stage (InferDepthNet0.forward, reference adamvs.py:433-533) on an 8 x 128 map with 100 uniform planes: CostRegNet2D
    runs at width 128 with 28 pad channels, conv0 and `prob` (softmax partials, fewer planes than channels) in the F(2x4, 3x3) form.
    Option winograd = 3 keeps F(2x2, 3x3) in every stride-1 layer; the two differ in rounding, and both hold the stage bars of
    tests/fp64_bars.py per pixel against the oracle in float64 in what CostRegNet2D produces -- the view weights and the pair depths
    -- and in the photometric confidence.  (The stage's depth: the two tests below.)"""
    got, ref, interval = stage100
    assert not torch.equal(got[1]["pair_confidence"][0], got[3]["pair_confidence"][0])        # the default takes the new form here
    for value in (1, 3):
        what = "winograd=%d: " % value
        check(got[value]["photometric_confidence"], ref["photometric_confidence"], STAGE_CONF, scale=1.0, what=what + "photometric confidence")
        for i, want in enumerate(ref["pair_confidence"]):
            check(got[value]["pair_confidence"][i].reshape(want.shape), want, STAGE_CONF, scale=1.0, what=what + "pair confidence %d" % i)
        for i, want in enumerate(ref["pair_result"]):
            check(got[value]["pair_result"][i], want, STAGE_DEPTH, scale=interval, what=what + "pair depth %d (hypothesis intervals)" % i)


# The reference's own fp32 evaluation of this stage (oracle in float32 against the oracle in float64, on the CPU) is 6.62e-4 hypothesis
# intervals off in depth at 100 planes on the 8 x 128 map (2.7e-4 of the pixels over STAGE_DEPTH; 64 planes on the same map: 3.2e-4; 64 planes on
# 24 x 32: 1.2e-4): STAGE_DEPTH, measured on stages of at most 64 planes and 50 columns, lies below what fp32 gives at any shape on which the
# network selects the new form.  The stage bars are therefore held where they were measured, with the form forced through the ops
# (test_stage_with_the_form_forced_through_the_ops), and the depth of the 100-plane stage is held to 4 x the reference's own distance, the
# convention of the reference-anchored bars of tests/fp64_bars.py.  Measured on the MI355X: 6.6e-4 with the form, 5.7e-4 without.
STAGE100_DEPTH = 2.6e-3


def test_stage_depth_with_and_without_the_form(stage100):
    """The 100-plane stage's depth map, both ways, against the bar derived above from the reference's own fp32 error at this shape."""
    got, ref, interval = stage100
    for value in (1, 3):
        check(got[value]["depth"], ref["depth"], STAGE100_DEPTH, scale=interval, what="winograd=%d: depth (hypothesis intervals)" % value)


def test_stage_with_the_form_forced_through_the_ops(hip, monkeypatch):
    """The first stage at the largest first-stage shape of test_hip_parity.py::test_stage_on_random_shapes_against_oracle (64 planes, 24 x 32,
    three views, two tiles) -- too narrow for the network to select the new form, so it is forced through the ops: pair similarity,
    CostRegNet2D layer by layer (bench.timed_cost_reg_layers, the chain adamvs_cost_reg_net_2d issues) with conv0 and `prob` + softmax
    partials on adamvs_conv3x3_dd_wino24 / adamvs_prob_softmax_regress_wino24, then the rest of the stage (aggregation, recurrence,
    soft-argmin) on those view weights.  The same chain on the F(2x2, 3x3) ops equals the whole stage call bit for bit (the path of
    before); with the new form the maps differ from it, and both hold STAGE_DEPTH / STAGE_CONF per pixel against the oracle in float64."""
    import bench
    from oracle import adamvs_oracle as O
    from ada_mvs_amd import _lib, hip_ops
    from ada_mvs_amd.models.adamvs import Infer_AdaMVSNet
    B, V, D, C, h, w = 2, 3, 64, 32, 24, 32
    S = V - 1
    m = Infer_AdaMVSNet(D, [D, 32, 8], synth.DEPTH_INTERVALS_RATIO, False, [8, 8, 8])
    sd = synth.seeded_state_dict(m, seed=6)
    m.load_state_dict(sd)
    net = m.cuda().eval().DepthNet[0]
    feats = [synth.smooth_features(B, C, h, w, seed=80 + v) for v in range(V)]
    proj = synth.rig_projections(V, 4 * h, 4 * w, batch=B)["stage1"]
    cur = dev(torch.tensor([[420.0, 580.0], [430.0, 590.0]]))
    interval = 160.0 / (D - 1)
    feat_cl = hip.pack_features(dev(torch.stack(feats, 0).reshape(-1, C, h, w)))
    rt = hip.relative_transforms(dev(proj))
    planes = hip.plane_source(cur, D, 0.0, [B, h, w])
    planes_t = hip.depth_range_samples(cur, D, 0.0, [B, h, w])            # the planes the kernels generate, bit for bit
    desc = hip.stage_desc(B, S, C, h, w, D, net.in_up, True, (0, 0), _lib.PRECISIONS[net.reg.effective_precision()],
                          _lib.PRECISIONS[net.reg_fuse.precision], plane_mode=planes[0], half_span=planes[1])
    ws = torch.empty(hip.depth_stage_workspace_bytes(desc) // 4, device="cuda")
    w_reg, fuse = net.reg.packed(cur.device), net.reg_fuse.packed(cur.device)
    # conv0 and prob in the new form, from the module's weights (the blob carries no such blocks at D = 64)
    bn = lambda s: sd["DepthNet.0.reg.conv0.bn." + s].float()            # noqa: E731
    w24 = {"conv0": dev(packing.pack_reg_layer_wino24(sd["DepthNet.0.reg.conv0.conv.weight"], bn("weight") / torch.sqrt(bn("running_var") + packing.BN_EPS))),
           "prob": dev(packing.pack_reg_layer_wino24(sd["DepthNet.0.reg.prob.weight"], torch.ones(D)))}
    plain, plain_sm = hip_ops.conv3x3_dd_wino, hip_ops.prob_softmax_regress_wino

    def layer24(x, ww, bias, skip, N, D_, hi, wi, relu, out=None):      # conv0 is the stride-1 layer with a ReLU on the full-size map
        return hip_ops.conv3x3_dd_wino24(x, w24["conv0"], bias, skip, N, D_, hi, wi, relu, out=out) if (hi, wi) == (h, w) \
            else plain(x, ww, bias, skip, N, D_, hi, wi, relu, out=out)

    def stage(forced):
        outs = (torch.empty(S, B, h, w, device="cuda"), torch.empty(S, B, h, w, device="cuda"), torch.empty(B, 2 * h, 2 * w, device="cuda"),
                torch.empty(B, 2 * h, 2 * w, device="cuda"))
        with monkeypatch.context() as mp:
            if forced:
                mp.setattr(hip_ops, "conv3x3_dd_wino", layer24)
                mp.setattr(hip_ops, "prob_softmax_regress_wino", lambda x, ww, *rest: hip_ops.prob_softmax_regress_wino24(x, w24["prob"], *rest))
            sim = hip.pair_similarity(feat_cl, rt, planes_t, B, S, C, D, h, w)
            vw, pd = bench.timed_cost_reg_layers(lambda name, fn: fn(), 1, sim, w_reg, S * B, D, h, w, 0, softmax=(planes_t, S, B, cur))
        outs[0].copy_(vw)
        outs[1].copy_(pd)
        hip.depth_stage_forward(desc, feat_cl, rt, planes[2], None, w_reg, fuse, ws,
                                phases=_lib.PHASE_AGGREGATE | _lib.PHASE_RECURRENCE | _lib.PHASE_SOFT_ARGMIN, outputs=outs)
        torch.cuda.synchronize()
        return net._as_dict(outs[0], outs[1], outs[2], outs[3], D)

    assert net.in_up
    with torch.no_grad():
        whole = net._as_dict(*net.run(feat_cl, B, C, h, w, rt, None, None, planes=planes, num_depth=D), D)
        got = {"F(2x2, 3x3)": stage(False), "F(2x4, 3x3)": stage(True)}
        ref = O.infer_depth_stage([f.double() for f in feats], proj.double(), planes_t.cpu().double(), double_sd(sd), "DepthNet.0.", net.in_up, None)
    for key in ("depth", "photometric_confidence"):
        assert torch.equal(got["F(2x2, 3x3)"][key], whole[key]), key                             # the path of before, op by op
    assert torch.equal(got["F(2x2, 3x3)"]["pair_confidence"][0], whole["pair_confidence"][0])
    assert not torch.equal(got["F(2x4, 3x3)"]["pair_confidence"][0], whole["pair_confidence"][0])
    for form, maps in got.items():
        figs = (check(maps["depth"], ref["depth"], STAGE_DEPTH, scale=interval, what=form + ": depth (hypothesis intervals)")[0],
                check(maps["photometric_confidence"], ref["photometric_confidence"], STAGE_CONF, scale=1.0, what=form + ": photometric confidence")[0])
        for i, want in enumerate(ref["pair_confidence"]):
            check(maps["pair_confidence"][i].reshape(want.shape), want, STAGE_CONF, scale=1.0, what=form + ": pair confidence %d" % i)
        for i, want in enumerate(ref["pair_result"]):
            check(maps["pair_result"][i], want, STAGE_DEPTH, scale=interval, what=form + ": pair depth %d (hypothesis intervals)" % i)
        print("wino24 stage forced through the ops, %s: depth %.3e intervals, confidence %.3e" % ((form,) + figs))


def test_winograd_3_is_the_network_of_before(hip, set_option):
    """Option winograd = 3: adamvs_cost_reg_net_2d on a map that selects the new form runs F(2x2, 3x3) in every stride-1 layer --
    bit for bit the chain of one-layer ops (adamvs_conv3x3_dd_wino / adamvs_conv3x3_dd, which this form leaves untouched) that the
    network was before; the default differs from it in conv0 and prob, within the layer's rounding."""
    import bench
    from ada_mvs_amd.models.adamvs import CostRegNet2D
    N, D, h, w = 2, 128, 8, 128
    net = CostRegNet2D(D)
    net.load_state_dict(synth.seeded_state_dict(net, seed=2))
    wpk = dev(packing.pack_cost_reg_net_2d(net.state_dict(), "", "fp32"))
    x = dev(torch.randn(N, h * w, D, generator=torch.Generator().manual_seed(4)) * 0.5)
    set_option("winograd", 3)
    whole = hip.cost_reg_net_2d(x, wpk, h, w)
    chain = bench.timed_cost_reg_layers(lambda name, fn: fn(), 1, x, wpk, N, D, h, w)
    set_option("winograd", 1)
    new = hip.cost_reg_net_2d(x, wpk, h, w)
    torch.cuda.synchronize()
    assert torch.equal(whole, chain)
    assert not torch.equal(new, whole) and rel_l1(new, whole) < 1e-5
