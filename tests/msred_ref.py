"""Float64 references for the MS-REDNet kernels that oracle/msrednet_oracle.py does not give at op level, and a second fp32
evaluation of the recurrent cell in another summation order.

`recurrence` is oracle.conv_gru_cell2 over the planes of a stage from a zero state; `soft_argmin` is the running exp-sum / max /
weighted-depth update of oracle.infer_depth_stage_red on a given volume.  Both are dtype-generic: the tests call them on
`.double()` inputs and `fp64_bars.double_sd(sd)`.  `recurrence_unfold` is NOT a reference: it is the stand-in for "some other
correct fp32 implementation" (convolution as unfold + matmul, GroupNorm from explicit sums) that tests/test_fp64_bars.py holds to
the RED_ bars on the CPU.  A plain module, imported by the test files.
"""
import torch
import torch.nn.functional as F

from oracle import msrednet_oracle as mo

HC = (8, 16, 32, 64)       # state channels of levels 1-4


def _cell_split(xterms, h, sd, pre, cx):
    """ConvGRUCell2 with the x halves of its two convolutions given: conv(cat(x, h)) = (Wx.x + b) + Wh.h, xterms = the three
    bracketed maps (reset rows, update rows of gate_conv; output_conv), cx = the number of x channels in the weights."""
    gxr, gxu, cxm = xterms
    hc = h.shape[1]
    wg, wc = sd[pre + "gate_conv.weight"][:, cx:], sd[pre + "output_conv.weight"][:, cx:]
    fr = gxr + F.conv2d(h, wg[:hc], None, padding=1)
    fu = gxu + F.conv2d(h, wg[hc:], None, padding=1)
    r = torch.sigmoid(F.group_norm(fr, 1, sd[pre + "reset_gate_norm.weight"], sd[pre + "reset_gate_norm.bias"], 1e-5))
    u = torch.sigmoid(F.group_norm(fu, 1, sd[pre + "update_gate_norm.weight"], sd[pre + "update_gate_norm.bias"], 1e-5))
    o = cxm + F.conv2d(r * h, wc, None, padding=1)
    y = torch.tanh(F.group_norm(o, 1, sd[pre + "output_norm.weight"], sd[pre + "output_norm.bias"], 1e-5))
    return u * h + (1 - u) * y


def recurrence(level, xs, sd, pre=""):
    """conv_gru<level> (1-4) of a slice_RED_Regularization state dict over the planes xs from a zero state -> every plane's state
    [D][B, HC, h, w].  xs: per plane x [B, Cx, h, w], or (gxr, gxu, cx) [B, HC, h, w] each -- the x halves (+ bias) of the three
    convolutions, as adamvs_red_recur_split takes them."""
    pre = pre + "conv_gru%d." % level
    hc = HC[level - 1]
    first = xs[0][0] if isinstance(xs[0], (tuple, list)) else xs[0]
    h = torch.zeros(first.shape[0], hc, first.shape[2], first.shape[3], dtype=first.dtype)
    out = []
    for x in xs:
        if isinstance(x, (tuple, list)):
            h = _cell_split(x, h, sd, pre, sd[pre + "gate_conv.weight"].shape[1] - hc)
        else:
            h = mo.conv_gru_cell2(x, h, sd, pre)
        out.append(h)
    return out


def soft_argmin(vol, planes):
    """vol [B, D, h, w] (the argument of exp), planes [B, D, h, w] -> depth, photometric_confidence [B, h, w]: the plane loop of
    oracle.infer_depth_stage_red, no max subtraction (inf / NaN where the reference gives them)."""
    B, D, h, w = vol.shape
    exp_sum = torch.zeros(B, 1, h, w, dtype=vol.dtype)
    depth_image, max_prob = torch.zeros_like(exp_sum), torch.zeros_like(exp_sum)
    for d in range(D):
        prob = vol[:, d:d + 1].exp()
        flag = (max_prob < prob).to(prob.dtype)
        max_prob = flag * prob + (1 - flag) * max_prob
        depth_image = planes[:, d:d + 1] * prob + depth_image
        exp_sum = exp_sum + prob
    denom = exp_sum + 1e-10
    return (depth_image / denom).squeeze(1), (max_prob / denom).squeeze(1)


# ---- the second fp32 evaluation: another summation order, not a reference ------------------------------------------------------
def _conv_unfold(x, w, b):
    B, _, h, ww = x.shape
    out = w.reshape(w.shape[0], -1) @ F.unfold(x, 3, padding=1)
    if b is not None:
        out = out + b.reshape(1, -1, 1)
    return out.reshape(B, -1, h, ww)


def _gn_sums(x, weight, bias, eps=1e-5):
    n = x[0].numel()
    mean = x.sum(dim=(1, 2, 3), keepdim=True) / n
    var = ((x * x).sum(dim=(1, 2, 3), keepdim=True) / n - mean * mean).clamp_min(0)
    return (x - mean) * torch.rsqrt(var + eps) * weight.reshape(1, -1, 1, 1) + bias.reshape(1, -1, 1, 1)


def recurrence_unfold(level, xs, sd, pre=""):
    """`recurrence` with every convolution as unfold + matmul and GroupNorm from sum and sum of squares."""
    pre = pre + "conv_gru%d." % level
    hc = HC[level - 1]
    split = isinstance(xs[0], (tuple, list))
    first = xs[0][0] if split else xs[0]
    h = torch.zeros(first.shape[0], hc, first.shape[2], first.shape[3], dtype=first.dtype)
    wg, bg, wc, bc = (sd[pre + k] for k in ("gate_conv.weight", "gate_conv.bias", "output_conv.weight", "output_conv.bias"))
    cx = wg.shape[1] - hc
    norm = lambda t, name: _gn_sums(t, sd[pre + name + ".weight"], sd[pre + name + ".bias"])       # noqa: E731
    out = []
    for x in xs:
        if split:
            f = torch.cat((x[0], x[1]), 1) + _conv_unfold(h, wg[:, cx:], None)
        else:
            f = _conv_unfold(torch.cat((x, h), 1), wg, bg)
        r, u = torch.sigmoid(norm(f[:, :hc], "reset_gate_norm")), torch.sigmoid(norm(f[:, hc:], "update_gate_norm"))
        o = x[2] + _conv_unfold(r * h, wc[:, cx:], None) if split else _conv_unfold(torch.cat((x, r * h), 1), wc, bc)
        h = u * h + (1 - u) * torch.tanh(norm(o, "output_norm"))
        out.append(h)
    return out


# ---- seeded inputs shared by the GPU cases (tests/test_msred_forms.py) and the CPU check of the bars (tests/test_fp64_bars.py) ---
def red_state_dict(C, seed):
    from ada_mvs_amd import synth
    from ada_mvs_amd.models.msrednet import slice_RED_Regularization
    return synth.seeded_state_dict(slice_RED_Regularization(C, 8), seed=seed)


def recur_inputs(level, C, B, h, w, D):
    """-> (state dict of slice_RED_Regularization(C, 8), the planes' x): levels 1, 2 one map per plane (level 1: C channels of
    cost-like values; level 2: 16 channels behind a ReLU, as conv1 leaves them); levels 3, 4 the three x halves per plane."""
    seed = 1000 * level + C + 7 * B + 3 * h + w + D
    sd = red_state_dict(C, seed)
    g = torch.Generator().manual_seed(seed)
    if level == 1:
        xs = [torch.randn(B, C, h, w, generator=g) * 0.5 for _ in range(D)]
    elif level == 2:
        xs = [torch.relu(torch.randn(B, 16, h, w, generator=g)) for _ in range(D)]
    else:
        xs = [tuple(torch.randn(B, HC[level - 1], h, w, generator=g) for _ in range(3)) for _ in range(D)]
    return sd, xs


def to_dtype(xs, dt):
    return [tuple(t.to(dt) for t in x) if isinstance(x, (tuple, list)) else x.to(dt) for x in xs]


def trained_range_logits(B, D, h, w, seed):
    """Logits of a trained network's range: N(0, 3) with one dominant +60 on a lattice of pixels and rows at a -60 floor under one
    channel at 0 (as tests/test_kernel_forms.py::test_softmax_max_regress_unfused builds them)."""
    g = torch.Generator().manual_seed(seed)
    vol = torch.randn(B, D, h, w, generator=g) * 3
    vol[:, (D * 5) // 7, ::7, ::5] = 60.0
    vol[:, :, 3::11, :] = -60.0
    vol[:, D // 3, 3::11, :] = 0.0
    return vol


def uniform_planes(ranges, D, h, w):
    """[B, D, h, w] planes, D uniform samples over each sample's [min, max] (D = 1: the minimum); -> planes, interval of sample 0."""
    r = torch.tensor(ranges, dtype=torch.float32)
    step = (r[:, 1] - r[:, 0]) / max(D - 1, 1)
    planes = r[:, :1] + torch.arange(D, dtype=torch.float32).reshape(1, -1) * step.unsqueeze(1)
    return planes.reshape(len(ranges), D, 1, 1).repeat(1, 1, h, w).contiguous(), float(step[0])


def variance_inputs(kind, C, V, B, h, w):
    """-> (V feature maps [B, C, h, w], projections [B, V, 4, 4], planes [B, 3, h, w]).
    kind "rig8" / "rig150": the synthetic rig at baseline 8 (taps inside the image) / 150 (taps leaving it), random planes.
    kind "border": focal length 64, pure translations; plane 0 (d = 512) shifts view v by exactly (v, 1 - v) pixels: every tap on
    the pixel grid, the last row and column included (and the first beyond them, weight 0); plane 1 (d = 16) sends every tap of
    every source view out of the image; plane 2 is random; the last source view is out of the image on all three."""
    from ada_mvs_amd import synth
    feats = [synth.smooth_features(B, C, h, w, seed=10 + v) for v in range(V)]
    g = torch.Generator().manual_seed(C + V + h)
    planes = 400 + 200 * torch.rand(B, 3, h, w, generator=g)
    if kind != "border":
        return feats, synth.rig_projections(V, 4 * h, 4 * w, batch=B, baseline={"rig8": 8.0, "rig150": 150.0}[kind])["stage1"], planes
    planes[:, 0], planes[:, 1] = 512.0, 16.0
    K = torch.tensor([[64.0, 0, w / 2.0, 0], [0, 64.0, h / 2.0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])
    proj = torch.zeros(B, V, 4, 4)
    for v in range(V):
        E = torch.eye(4)
        E[0, 3], E[1, 3] = 8.0 * v, 8.0 * (1 - v) if v else 0.0
        if v == V - 1 and V > 2:
            E[0, 3] = 16.0 * w
        proj[:, v] = K @ E
    return feats, proj, planes
