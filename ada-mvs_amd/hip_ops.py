"""Thin PyTorch-tensor wrappers over the C ABI (include/adamvs_hip.h).

PyTorch is used for device memory and the current stream only; every
computation below happens in libadamvs_hip.so.  All functions require CUDA
(ROCm) fp32 tensors and raise otherwise -- there is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import FuseWeights, StageDesc, check


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.AdaMVSHipError("%s must be a GPU tensor: the Ada-MVS hot path has no CPU fallback" % name)
    if t.dtype != torch.float32:
        raise _lib.AdaMVSHipError("%s must be float32, got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def relative_transforms(proj):
    """proj [B,V,4,4] -> rt [B,V-1,12]   (module.py:539-541)"""
    proj = _dev(proj, "proj")
    B, V = proj.shape[:2]
    rt = torch.empty(B, V - 1, 12, device=proj.device, dtype=torch.float32)
    check(_lib.load().adamvs_relative_transforms(_p(proj), _p(rt), B, V, _stream()), "relative_transforms")
    return rt


def pack_features(x, out=None):
    """[N,C,h,w] -> channel-last [N,h*w,C]"""
    x = _dev(x, "features")
    N, C, h, w = x.shape
    if out is None:
        out = torch.empty(N, h * w, C, device=x.device, dtype=torch.float32)
    check(_lib.load().adamvs_pack_features(_p(x), _p(out), N, C, h, w, _stream()), "pack_features")
    return out


def unpack_features(x, h, w):
    """channel-last [N,h*w,C] -> [N,C,h,w]"""
    x = _dev(x, "features")
    N, hw, C = x.shape
    out = torch.empty(N, C, h, w, device=x.device, dtype=torch.float32)
    check(_lib.load().adamvs_unpack_features(_p(x), _p(out), N, C, h, w, _stream()), "unpack_features")
    return out


def depth_range_samples(cur_depth, ndepth, depth_interval_pixel, shape):
    """get_depth_range_samples (module.py:646-663) -> [B,D,h,w]"""
    cur_depth = _dev(cur_depth, "cur_depth")
    B, h, w = shape
    out = torch.empty(B, ndepth, h, w, device=cur_depth.device, dtype=torch.float32)
    lib = _lib.load()
    if cur_depth.dim() == 2:
        if cur_depth.shape[1] != 2:        # the reference reads [:,0] and [:,-1] only
            cur_depth = torch.stack((cur_depth[:, 0], cur_depth[:, -1]), 1).contiguous()
        check(lib.adamvs_depth_range_samples_uniform(_p(cur_depth), _p(out), B, ndepth, h, w, _stream()),
              "depth_range_samples_uniform")
    else:
        if tuple(cur_depth.shape) != (B, h, w):
            raise _lib.AdaMVSHipError("cur_depth:%s, input shape:%s" % (tuple(cur_depth.shape), shape))
        check(lib.adamvs_depth_range_samples_window(_p(cur_depth), float(depth_interval_pixel), _p(out), B, ndepth, h, w,
                                                    _stream()), "depth_range_samples_window")
    return out


def resize_bilinear(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=False) for [N,1,h,w] / [N,h,w]"""
    x = _dev(x, "x")
    hi, wi = x.shape[-2:]
    ho, wo = size
    N = x.numel() // (hi * wi)
    out = torch.empty(x.shape[:-2] + (ho, wo), device=x.device, dtype=torch.float32)
    check(_lib.load().adamvs_resize_bilinear(_p(x), _p(out), N, hi, wi, ho, wo, _stream()), "resize_bilinear")
    return out


def depth_regression(p, depth_values):
    """module.py:617-625"""
    p = _dev(p, "p")
    depth_values = _dev(depth_values, "depth_values")
    B, D, h, w = p.shape
    out = torch.empty(B, h, w, device=p.device, dtype=torch.float32)
    hd, wd = (0, 0) if depth_values.dim() <= 2 else depth_values.shape[2:]
    check(_lib.load().adamvs_depth_regression(_p(p), _p(depth_values), _p(out), B, D, h, w, hd, wd, _stream()),
          "depth_regression")
    return out


def homo_warp(src_fea, rt, depth_values):
    """homo_warping_float body (module.py:543-566): src [B,C,h,w], rt [B,12], depth [B,Nd,h,w] -> [B,C,Nd,h,w]"""
    src_fea = _dev(src_fea, "src_fea")
    rt = _dev(rt, "rt")
    depth_values = _dev(depth_values, "depth_values")
    B, C, h, w = src_fea.shape
    Nd = depth_values.shape[1]
    out = torch.empty(B, C, Nd, h, w, device=src_fea.device, dtype=torch.float32)
    check(_lib.load().adamvs_homo_warp(_p(src_fea), _p(rt), _p(depth_values), _p(out), B, C, Nd, h, w, _stream()), "homo_warp")
    return out


def pair_similarity(feat, rt, planes, B, S, C, D, h, w):
    """feat [V*B,hw,C] (view-major), rt [B,S,12], planes [B,D,h,w] -> sim [S*B,hw,D]"""
    sim = torch.empty(S * B, h * w, D, device=feat.device, dtype=torch.float32)
    check(_lib.load().adamvs_pair_similarity(_p(_dev(feat, "feat")), _p(_dev(rt, "rt")), _p(_dev(planes, "planes")), _p(sim),
                                             B, S, C, D, h, w, _stream()), "pair_similarity")
    return sim


def cost_reg_net_2d(x_cl, wpk, h, w, precision=0, blocks=None):
    """x_cl [N,hw,D] channel-last -> score [N,hw,D]   (adamvs.py:229-238).  blocks (fp32; A/B, tests): -1 as None, 0 no folded
    blocks in any layer (adamvs_cost_reg_net_2d_blocks)."""
    x_cl = _dev(x_cl, "x")
    N, hw, D = x_cl.shape
    lib = _lib.load()
    nbytes = lib.adamvs_cost_reg_net_2d_workspace_bytes(N, D, h, w)
    ws = torch.empty(nbytes // 4, device=x_cl.device, dtype=torch.float32)
    score = torch.empty_like(x_cl)
    if blocks is not None:
        assert int(precision) == 0
        check(lib.adamvs_cost_reg_net_2d_blocks(_p(x_cl), _p(wpk), wpk.numel(), _p(score), N, D, h, w, int(blocks), _p(ws), nbytes, _stream()),
              "cost_reg_net_2d_blocks")
        return score
    check(lib.adamvs_cost_reg_net_2d(_p(x_cl), _p(wpk), wpk.numel(), _p(score), N, D, h, w, int(precision), _p(ws), nbytes, _stream()),
          "cost_reg_net_2d")
    return score


def softmax_max_regress(score, planes, S, B, D, h, w):
    vw = torch.empty(S, B, h, w, device=score.device, dtype=torch.float32)
    pd = torch.empty(S, B, h, w, device=score.device, dtype=torch.float32)
    check(_lib.load().adamvs_softmax_max_regress(_p(_dev(score, "score")), _p(_dev(planes, "planes")), _p(vw), _p(pd),
                                                 S, B, D, h, w, _stream()), "softmax_max_regress")
    return vw, pd


def prob_softmax_regress(x_cl, wpk_layer, bias, planes, S, B, D, h, w, precision=0):
    """The `prob` layer of CostRegNet2D with softmax / max / depth regression in its epilogue (what the stage runs):
    x_cl [S*B, h*w, D], planes [B, D, h, w] -> (view_weight, pair_depth) [S, B, h, w]."""
    vw = torch.empty(S, B, h, w, device=x_cl.device, dtype=torch.float32)
    pd = torch.empty(S, B, h, w, device=x_cl.device, dtype=torch.float32)
    check(_lib.load().adamvs_prob_softmax_regress(_p(_dev(x_cl, "x")), _p(wpk_layer), _p(bias), _p(_dev(planes, "planes")), _p(vw), _p(pd),
                                                  S, B, D, h, w, int(precision), _stream()), "prob_softmax_regress")
    return vw, pd


def prob_softmax_regress_wino(x_cl, wino_layer, bias, depth_range, S, B, D, h, w):
    """The same with `prob` in the F(2x2, 3x3) form (wino_layer from packing.pack_reg_layer_wino): per-lane softmax partials and a
    merge kernel instead of the score volume -- what the fp32 stage runs at D a multiple of 64.  depth_range [B, 2]: first and
    last hypothesis plane of every tile (stage 1's uniform planes)."""
    vw = torch.empty(S, B, h, w, device=x_cl.device, dtype=torch.float32)
    pd = torch.empty(S, B, h, w, device=x_cl.device, dtype=torch.float32)
    lib = _lib.load()
    nbytes = lib.adamvs_prob_softmax_regress_wino_workspace_bytes(S, B, D, h, w)
    ws = torch.empty(nbytes // 4, device=x_cl.device, dtype=torch.float32)
    check(lib.adamvs_prob_softmax_regress_wino(_p(_dev(x_cl, "x")), _p(wino_layer), _p(bias), _p(_dev(depth_range, "depth_range")), _p(vw), _p(pd),
                                               S, B, D, h, w, ctypes.c_void_p(ws.data_ptr()), nbytes, _stream()), "prob_softmax_regress_wino")
    return vw, pd


def prob_softmax_regress_wino24(x_cl, wino24_layer, bias, depth_range, S, B, D, h, w):
    """The same with `prob` in the F(2x4, 3x3) form (wino24_layer from packing.pack_reg_layer_wino24): what the fp32 stage runs on
    wide maps at D >= 128.  Same partials, merge kernel and workspace as prob_softmax_regress_wino."""
    vw = torch.empty(S, B, h, w, device=x_cl.device, dtype=torch.float32)
    pd = torch.empty(S, B, h, w, device=x_cl.device, dtype=torch.float32)
    lib = _lib.load()
    nbytes = lib.adamvs_prob_softmax_regress_wino_workspace_bytes(S, B, D, h, w)
    ws = torch.empty(nbytes // 4, device=x_cl.device, dtype=torch.float32)
    check(lib.adamvs_prob_softmax_regress_wino24(_p(_dev(x_cl, "x")), _p(wino24_layer), _p(bias), _p(_dev(depth_range, "depth_range")), _p(vw),
                                                 _p(pd), S, B, D, h, w, ctypes.c_void_p(ws.data_ptr()), nbytes, _stream()),
          "prob_softmax_regress_wino24")
    return vw, pd


def aggregate_conv1(feat, rt, planes, view_weight, w1pk, B, S, C, D, h, w, precision=0, return_similarity=False):
    """-> c1 [D,B,hw,8]; return_similarity (D <= 32, one chunk): also the aggregated similarity [D,B,hw,C] the call left in
    its workspace (include/adamvs_hip.h: the workspace holds the last chunk's similarity on return)."""
    c1 = torch.empty(D, B, h * w, 8, device=feat.device, dtype=torch.float32)
    lib = _lib.load()
    nbytes = lib.adamvs_aggregate_conv1_workspace_bytes(B, C, D, h, w)
    ws = torch.empty(max(nbytes // 4, 1), device=feat.device, dtype=torch.float32)
    check(_lib.load().adamvs_aggregate_conv1(_p(_dev(feat, "feat")), _p(_dev(rt, "rt")), _p(_dev(planes, "planes")),
                                             _p(_dev(view_weight, "view_weight")), _p(w1pk), _p(c1), B, S, C, D, h, w, int(precision),
                                             _p(ws), nbytes, _stream()), "aggregate_conv1")
    if return_similarity:
        if D > 32:
            raise _lib.AdaMVSHipError("aggregate_conv1: return_similarity needs D <= 32 (one chunk of planes in the workspace)")
        return c1, ws[:D * B * h * w * C].reshape(D, B, h * w, C)
    return c1


class PackedFuse:
    """Device copy of a packed SliceCostRegNetRED + its adamvs_fuse_weights struct."""

    def __init__(self, flat, offsets, device):
        self.buf = flat.to(device)
        base = self.buf.data_ptr()
        self.struct = FuseWeights(**{f: base + 4 * o for f, o in offsets.items()})

    def ptr(self):
        return ctypes.byref(self.struct)

    def field(self, name):
        return ctypes.c_void_p(getattr(self.struct, name))


class PackedFeature:
    """Device copy of a packed FeatureNet0 + its adamvs_feature_weights struct."""

    def __init__(self, flat, offsets, device):
        from ._lib import FeatureWeights, FConvWeights, ContextWeights
        self.buf = flat.to(device)
        base = self.buf.data_ptr()
        at = lambda f: base + 4 * offsets[f]
        kw = {n: FConvWeights(at(n + ".w"), at(n + ".b")) for n in packing_fields()[0]}
        kw.update({n: ContextWeights(at(n + ".w1"), at(n + ".b1"), at(n + ".w2")) for n in packing_fields()[1]})
        self.struct = FeatureWeights(**kw)

    def ptr(self):
        return ctypes.byref(self.struct)


def packing_fields():
    from . import packing
    return packing.FEATURE_CONVS, packing.FEATURE_BRANCHES


def feature_net0_workspace_bytes(N, H, W):
    return int(_lib.load().adamvs_feature_net0_workspace_bytes(int(N), int(H), int(W)))


def feature_net0(imgs, packed, workspace=None, out=None, views=None):
    """FeatureNet0.forward on [N,3,H,W] images -> channel-last (stage1 [N,hw/16,32], stage2 [N,hw/4,16], stage3 [N,hw,8]).
    out: the three (contiguous) result tensors, e.g. slices of the maps of a larger batch run in chunks.
    views = (n0, n): imgs is [B,V,3,H,W] as the reference's forward() receives it; images n0 .. n0+n-1 of the V*B images in
    view-major order (m = v*B + b) are computed, read in place (no transposed copy)."""
    lib = _lib.load()
    imgs = _dev(imgs, "imgs")
    if views is not None:
        Bv, Vv, c, H, W = imgs.shape
        n0, N = views
    else:
        N, c, H, W = imgs.shape
    if c != 3:
        check(-1, "feature_net0")
    dev = imgs.device
    if out is None:
        s1 = torch.empty(N, (H // 4) * (W // 4), 32, device=dev, dtype=torch.float32)
        s2 = torch.empty(N, (H // 2) * (W // 2), 16, device=dev, dtype=torch.float32)
        s3 = torch.empty(N, H * W, 8, device=dev, dtype=torch.float32)
    else:
        s1, s2, s3 = out
        want = ((N, (H // 4) * (W // 4), 32), (N, (H // 2) * (W // 2), 16), (N, H * W, 8))
        if any(tuple(t.shape) != w or not t.is_contiguous() or t.dtype != torch.float32 or t.device != dev for t, w in zip(out, want)):
            raise _lib.AdaMVSHipError("feature_net0: out tensors must be contiguous float32 %s on %s" % (want, dev))
    nbytes = lib.adamvs_feature_net0_workspace_bytes(N, H, W)
    if workspace is None or workspace.numel() * 4 < nbytes:
        workspace = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
    if views is not None:
        check(lib.adamvs_feature_net0_views(_p(imgs), packed.ptr(), _p(s1), _p(s2), _p(s3), Bv, Vv, n0, N, H, W, _p(workspace), nbytes,
                                            _stream()), "feature_net0_views")
    else:
        check(lib.adamvs_feature_net0(_p(imgs), packed.ptr(), _p(s1), _p(s2), _p(s3), N, H, W, _p(workspace), nbytes, _stream()),
              "feature_net0")
    return s1, s2, s3


class PackedFeatureFpn:
    """Device copy of a packed FPN FeatureNet + its adamvs_feature_fpn_weights struct."""

    def __init__(self, flat, offsets, device):
        from ._lib import FeatureFpnWeights, FConvWeights
        from . import packing
        self.buf = flat.to(device)
        base = self.buf.data_ptr()
        at = lambda f: base + 4 * offsets[f]
        self.struct = FeatureFpnWeights(**{n: FConvWeights(at(n + ".w"), at(n + ".b")) for n in packing.FEATURE_FPN_CONVS})

    def ptr(self):
        return ctypes.byref(self.struct)


def feature_net_fpn_workspace_bytes(N, H, W):
    return int(_lib.load().adamvs_feature_net_fpn_workspace_bytes(int(N), int(H), int(W)))


def feature_net_fpn(imgs, packed, workspace=None):
    """FeatureNet(arch_mode="fpn").forward (reference models/msrednet.py:115-125) on [N,3,H,W] images -> channel-last maps."""
    lib = _lib.load()
    imgs = _dev(imgs, "imgs")
    N, c, H, W = imgs.shape
    if c != 3:
        check(-1, "feature_net_fpn")
    dev = imgs.device
    s1 = torch.empty(N, (H // 4) * (W // 4), 32, device=dev, dtype=torch.float32)
    s2 = torch.empty(N, (H // 2) * (W // 2), 16, device=dev, dtype=torch.float32)
    s3 = torch.empty(N, H * W, 8, device=dev, dtype=torch.float32)
    nbytes = lib.adamvs_feature_net_fpn_workspace_bytes(N, H, W)
    if workspace is None or workspace.numel() * 4 < nbytes:
        workspace = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
    check(lib.adamvs_feature_net_fpn(_p(imgs), packed.ptr(), _p(s1), _p(s2), _p(s3), N, H, W, _p(workspace), nbytes, _stream()),
          "feature_net_fpn")
    return s1, s2, s3


def slice_reg_step(cost_cl, state1, state2, fuse, B, C, h, w, in_up, precision=0):
    """SliceCostRegNetRED.forward on channel-last maps; states updated in place. -> reg [B,1,Ho,Wo]"""
    lib = _lib.load()
    Ho, Wo = (2 * h, 2 * w) if in_up else (h, w)
    reg = torch.empty(B, 1, Ho, Wo, device=cost_cl.device, dtype=torch.float32)
    nbytes = lib.adamvs_slice_reg_step_scratch_bytes(B, h, w)
    scratch = torch.empty(nbytes // 4, device=cost_cl.device, dtype=torch.float32)
    check(lib.adamvs_slice_reg_step(_p(_dev(cost_cl, "cost")), _p(state1), _p(state2), fuse.ptr(), _p(reg), B, C, h, w,
                                    int(in_up), int(precision), _p(scratch), nbytes, _stream()), "slice_reg_step")
    return reg


def stage_desc(B, S, C, h, w, D, in_up, first_stage, prev_hw=(0, 0), precision=0, precision_fuse=0, eps_in_numerator=0,
               plane_mode=_lib.PLANES_EXPLICIT, half_span=0.0, half_span_dev=None):
    """half_span_dev: a one-element float32 device tensor holding the half span (window planes) -- read by the kernels when they run,
    so that a captured graph serves any depth range; the caller keeps it alive."""
    return StageDesc(B, S, C, h, w, D, int(in_up), int(first_stage), int(prev_hw[0]), int(prev_hw[1]), int(precision),
                     int(precision_fuse), int(eps_in_numerator), int(plane_mode), float(half_span),
                     ctypes.c_void_p(_dev(half_span_dev, "half_span_dev").data_ptr()) if half_span_dev is not None else None)


def half_span_of(ndepth, depth_interval_pixel):
    """ndepth / 2 * depth_inteval_pixel formed in Python floats, the product rounded to fp32 where it meets the map (module.py:632)."""
    return float(ndepth / 2.0 * float(depth_interval_pixel))


def plane_source(cur_depth, ndepth, depth_interval_pixel, shape, span_dev=None):
    """What get_depth_range_samples (module.py:646-663) would materialise, as (plane_mode, half_span, tensor[, span_dev]) for
    adamvs_depth_stage_forward: a 2-D cur_depth [B, >=2] gives uniform planes over [min, max] (the interval is ignored
    there, quirk Q3), a map [B,h,w] gives the per-pixel window cur -+ ndepth / 2 * depth_interval_pixel.  The planes are
    generated inside the kernels, bit-identical to depth_range_samples()."""
    cur_depth = _dev(cur_depth, "cur_depth")
    B, h, w = shape
    if cur_depth.dim() == 2:
        if cur_depth.shape[1] != 2:        # the reference reads [:,0] and [:,-1] only
            cur_depth = torch.stack((cur_depth[:, 0], cur_depth[:, -1]), 1).contiguous()
        return _lib.PLANES_UNIFORM, 0.0, cur_depth
    if tuple(cur_depth.shape) != (B, h, w):
        raise _lib.AdaMVSHipError("cur_depth:%s, input shape:%s" % (tuple(cur_depth.shape), shape))
    if span_dev is not None:           # the half span lives in device memory (graphed.py): nothing of the depth range is baked into the launch
        return _lib.PLANES_WINDOW, 0.0, cur_depth, span_dev
    return _lib.PLANES_WINDOW, half_span_of(ndepth, depth_interval_pixel), cur_depth


def depth_stage_workspace_bytes(desc):
    n = _lib.load().adamvs_depth_stage_workspace_bytes(ctypes.byref(desc))
    if n == 0:
        check(-1, "depth_stage_workspace_bytes")
    return n


def conv3x3_dd_wino(x_cl, wino_layer, bias, skip, N, D, h, w, relu, out=None):
    """A stride-1 CostRegNet2D layer in the F(2x2, 3x3) form; wino_layer from packing.pack_reg_layer_wino."""
    if out is None:
        out = torch.empty(N, h * w, D, device=x_cl.device, dtype=torch.float32)
    null = ctypes.c_void_p(0)
    check(_lib.load().adamvs_conv3x3_dd_wino(_p(_dev(x_cl, "x")), _p(wino_layer), _p(bias), _p(skip) if skip is not None else null,
                                             _p(out), N, D, h, w, int(relu), _stream()), "conv3x3_dd_wino")
    return out


def conv3x3_dd_wino24(x_cl, wino24_layer, bias, skip, N, D, h, w, relu, out=None, blocks=None):
    """A stride-1 CostRegNet2D layer in the F(2x4, 3x3) form; wino24_layer from packing.pack_reg_layer_wino24.  blocks (A/B, tests):
    1 the 64-pixel blocks, 2 / 4 the folded ones where the width allows, -1 as None (adamvs_conv3x3_dd_wino24_blocks)."""
    if out is None:
        out = torch.empty(N, h * w, D, device=x_cl.device, dtype=torch.float32)
    null = ctypes.c_void_p(0)
    if blocks is not None:
        check(_lib.load().adamvs_conv3x3_dd_wino24_blocks(_p(_dev(x_cl, "x")), _p(wino24_layer), _p(bias), _p(skip) if skip is not None else null,
                                                          _p(out), N, D, h, w, int(relu), int(blocks), _stream()), "conv3x3_dd_wino24_blocks")
        return out
    check(_lib.load().adamvs_conv3x3_dd_wino24(_p(_dev(x_cl, "x")), _p(wino24_layer), _p(bias), _p(skip) if skip is not None else null,
                                               _p(out), N, D, h, w, int(relu), _stream()), "conv3x3_dd_wino24")
    return out


def conv3x3_dd_s2_blocks(x_cl, wpk_layer, bias, N, D, hi, wi, relu, blocks, out=None):
    """A stride-2 CostRegNet2D layer (fp32, no skip) with the blocks of its pair form given (A/B, tests): -1 by the map, as
    conv3x3_dd(mode=1); 0 no folded blocks; 2 / 4 the folded ones where the width allows (adamvs_conv3x3_dd_s2_blocks)."""
    if out is None:
        out = torch.empty(N, (hi // 2) * (wi // 2), D, device=x_cl.device, dtype=torch.float32)
    check(_lib.load().adamvs_conv3x3_dd_s2_blocks(_p(_dev(x_cl, "x")), _p(wpk_layer), _p(bias), _p(out), N, D, hi, wi, int(relu), int(blocks),
                                                  _stream()), "conv3x3_dd_s2_blocks")
    return out


def conv3x3_dd(x_cl, wpk_layer, bias, skip, N, D, hi, wi, mode, relu, out=None, precision=0, in2=None):
    """One CostRegNet2D layer on channel-last maps (mode 0 stride 1, 1 stride 2, 2 transposed stride 2).
    skip: added to the output after the ReLU; in2: added to the input (the layer convolves x_cl + in2; fp32 only)."""
    ho, wo = (hi // 2, wi // 2) if mode == 1 else ((2 * hi, 2 * wi) if mode == 2 else (hi, wi))
    if out is None:
        out = torch.empty(N, ho * wo, D, device=x_cl.device, dtype=torch.float32)
    null = ctypes.c_void_p(0)
    check(_lib.load().adamvs_conv3x3_dd(_p(x_cl), _p(_dev(in2, "in2")) if in2 is not None else null, _p(wpk_layer), _p(bias),
                                        _p(skip) if skip is not None else null,
                                        _p(out), N, D, hi, wi, mode, int(relu), int(precision), _stream()), "conv3x3_dd")
    return out


def depth_stage_forward(desc, feat, rt, planes, prev_conf, w_reg, fuse, workspace=None, phases=_lib.PHASE_ALL, outputs=None,
                        timing_only=False):
    """InferDepthNet0.forward (adamvs.py:433-533).  Returns (view_weight [S,B,h,w], pair_depth or None,
    depth [B,Ho,Wo], confidence [B,Ho,Wo]).  timing_only: adamvs_bench_stage_phase -- the selected phases for their duration,
    no maps promised (bench.py's phase table)."""
    dev = feat.device
    B, S, h, w = desc.B, desc.S, desc.h, desc.w
    Ho, Wo = (2 * h, 2 * w) if desc.in_up else (h, w)
    nbytes = depth_stage_workspace_bytes(desc)
    if workspace is None or workspace.numel() * 4 < nbytes:
        workspace = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
    if outputs is not None:                 # piecewise (phase-by-phase) calls reuse one set of outputs
        vw, pd, depth, conf = outputs
    else:
        vw = torch.empty(S, B, h, w, device=dev, dtype=torch.float32)
        pd = torch.empty(S, B, h, w, device=dev, dtype=torch.float32) if desc.first_stage else None
        depth = torch.empty(B, Ho, Wo, device=dev, dtype=torch.float32)
        conf = torch.empty(B, Ho, Wo, device=dev, dtype=torch.float32)
    null = ctypes.c_void_p(0)
    entry = _lib.load().adamvs_bench_stage_phase if timing_only else _lib.load().adamvs_depth_stage_forward
    check(entry(
        ctypes.byref(desc), _p(_dev(feat, "feat")), _p(_dev(rt, "rt")), _p(_dev(planes, "planes")),
        _p(_dev(prev_conf, "prev_conf")) if prev_conf is not None else null,
        _p(w_reg) if w_reg is not None else null, w_reg.numel() if w_reg is not None else 0, fuse.ptr(),
        _p(vw), _p(pd) if pd is not None else null, _p(depth), _p(conf), int(phases), _p(workspace), nbytes, _stream()),
        "depth_stage_forward")
    return vw, pd, depth, conf


# ---- MS-REDNet pieces (csrc/msred.hip; reference models/msrednet.py:373-436, models/module.py:54-106) ---------------
def red_variance_cost(feat, rt, planes, out_a, out_b, B, S, C, D, h, w, negate=True):
    """-variance of (reference, warped sources) for the D planes [B,D,h*w] into channels [0,C) of out_a [D*B,h*w,Da]
    (plane-major) and out_b."""
    check(_lib.load().adamvs_red_variance_cost(_p(_dev(feat, "feat")), _p(rt), _p(_dev(planes, "planes")), _p(out_a), out_a.shape[-1],
                                               _p(out_b) if out_b is not None else ctypes.c_void_p(0),
                                               out_b.shape[-1] if out_b is not None else 0, B, S, C, D, h, w, int(negate),
                                               _stream()), "red_variance_cost")


def channel_copy(src, src_c0, dst, dst_c0, n):
    """dst[b, p, dst_c0:dst_c0+n] = src[b, p, src_c0:src_c0+n] for channel-last maps [N, npix, D]."""
    N, npix = src.shape[0], src.shape[1]
    check(_lib.load().adamvs_channel_copy(_p(src), _p(dst), N, npix, n, src.stride(0), src.stride(1), src_c0, dst.stride(0),
                                          dst.stride(1), dst_c0, _stream()), "channel_copy")


def planes_to_volume(src, vol, B):
    """vol[b, d, p] = src[d * B + b, p, 0]: the single real channel of the last decoder layer into the slice volume."""
    N, npix = src.shape[0], src.shape[1]
    D = N // B
    for b in range(B):
        check(_lib.load().adamvs_channel_copy(ctypes.c_void_p(src.data_ptr() + 4 * b * src.stride(0)),
                                              ctypes.c_void_p(vol.data_ptr() + 4 * b * vol.stride(0)), D, npix, 1,
                                              B * src.stride(0), src.stride(1), 0, vol.stride(1), 1, 0, _stream()), "channel_copy")


def group_stats_workspace(N, ngroups, device):
    return torch.empty(_lib.load().adamvs_group_stats_workspace_bytes(N, ngroups) // 8, device=device, dtype=torch.float64)


def group_stats_partial(x0, x1, n, partials):
    """Partial sums for GroupNorm(1 group) over channels [0, n) of x0 (and x1; views into a wider map are fine: the
    pixel stride is what counts): consumed by the gru2_* epilogues."""
    N, npix, D = x0.shape[0], x0.shape[1], x0.stride(1)
    check(_lib.load().adamvs_group_stats_partial(_p(x0), _p(x1) if x1 is not None else ctypes.c_void_p(0), N, npix, D, n,
                                                 _p(partials), partials.numel() * 8, _stream()), "group_stats_partial")


def group_stats_finish(partials, N, ngroups, npix, n, eps=1e-5):
    stats = torch.empty(N, ngroups, 2, device=partials.device, dtype=torch.float32)
    check(_lib.load().adamvs_group_stats_finish(_p(partials), _p(stats), N, ngroups, npix, n, eps, _stream()), "group_stats_finish")
    return stats


def gru2_gates_apply(fr, fu, partials, gn, h, rh, u, HC, eps=1e-5):
    """fr / fu: two maps of one width, or views of the two halves of one map (their last-but-one stride is the width)."""
    N, npix, W = h.shape
    check(_lib.load().adamvs_gru2_gates_apply(_p(fr), _p(fu), fr.stride(1), _p(partials), _p(gn), _p(h), _p(rh), _p(u), N, npix, W,
                                              HC, eps, _stream()), "gru2_gates_apply")


def conv3x3_pair(a, b, wpk, bias, cout, h, w, out=None):
    """conv3x3(cat(a, b)) + bias on compact channel-last maps [B, h*w, CA], [B, h*w, CB] -> [B, h*w, cout]."""
    B = a.shape[0]
    if out is None:
        out = torch.empty(B, h * w, cout, device=a.device, dtype=torch.float32)
    check(_lib.load().adamvs_conv3x3_pair(_p(_dev(a, "a")), a.shape[-1], _p(_dev(b, "b")), b.shape[-1], _p(wpk), _p(bias), _p(out),
                                          cout, B, h, w, _stream()), "conv3x3_pair")
    return out


def gru2_out_apply(o, partials, gn, u, h, out, HC, eps=1e-5):
    N, npix, W = o.shape
    check(_lib.load().adamvs_gru2_out_apply(_p(o), _p(partials), _p(gn), _p(u), _p(h),
                                            _p(out) if out is not None else ctypes.c_void_p(0),
                                            out.shape[-1] if out is not None else 0, N, npix, W, HC, eps, _stream()),
          "gru2_out_apply")


def red_recur_pair(x, wg, bg, wc, bc, gn, R, B, h, w, HC, eps=1e-5):
    """ConvGRUCell2 of a shallow level over all planes: x [D*B, h*w, Cx] compact -> R[:, :, :HC]."""
    D, Cx = x.shape[0] // B, x.shape[-1]
    lib = _lib.load()
    nbytes = lib.adamvs_red_recur_workspace_bytes(B, h, w, HC, 2 * HC, HC)
    ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
    check(lib.adamvs_red_recur_pair(_p(_dev(x, "x")), Cx, _p(wg), _p(bg), _p(wc), _p(bc), _p(gn), _p(R), R.shape[-1], B, D, h, w, HC,
                                    eps, _p(ws), nbytes, _stream()), "red_recur_pair")


def red_recur_split(gxr, gxu, cx, w_ghr, w_ghu, w_ch, gn, R, B, h, w, HC, eps=1e-5):
    """ConvGRUCell2 of a deep level over all planes from the precomputed x halves [D*B, h*w, W] -> R[:, :, :HC].
    w_*: the h halves as contiguous (9 W W + W)-float blocks."""
    D, W = gxr.shape[0] // B, gxr.shape[-1]
    lib = _lib.load()
    nbytes = lib.adamvs_red_recur_workspace_bytes(B, h, w, W, W, HC)
    ws = torch.empty(nbytes // 4, device=gxr.device, dtype=torch.float32)
    check(lib.adamvs_red_recur_split(_p(_dev(gxr, "gxr")), _p(gxu), _p(cx), _p(w_ghr), _p(w_ghu), _p(w_ch), _p(gn), _p(R),
                                     R.shape[-1], B, D, h, w, W, HC, eps, _p(ws), nbytes, _stream()), "red_recur_split")


def soft_argmin(vol, planes, B, D, h, w):
    depth = torch.empty(B, h, w, device=vol.device, dtype=torch.float32)
    conf = torch.empty(B, h, w, device=vol.device, dtype=torch.float32)
    check(_lib.load().adamvs_soft_argmin(_p(vol), _p(_dev(planes, "planes")), _p(depth), _p(conf), B, D, h, w, _stream()),
          "soft_argmin")
    return depth, conf


# ---- depth-map fusion (csrc/fusion.hip; driven per view by ada_mvs_amd/fusion.py) ----------------------------------------
def _dev_as(t, name, dtype):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.AdaMVSHipError("%s must be a GPU tensor: the fusion path has no CPU fallback" % name)
    if t.dtype != dtype:
        raise _lib.AdaMVSHipError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def fusion_blocks(H, W):
    """Workgroups of the fusion kernels for an [H, W] reference map (ADAMVS_FUSION_TILE consecutive pixels each)."""
    return (H * W + _lib.FUSION_TILE - 1) // _lib.FUSION_TILE


def geo_consistency(ref_depth, ref_conf, sources, prob_threshold=0.5, pix_threshold=1.0, rel_depth_threshold=0.01, min_consistent=2):
    """adamvs_geo_consistency.  ref_depth, ref_conf [H, W] fp32; sources: list of (depth [Hs, Ws] fp32, fwd (12,), back (12,))
    with fwd / back as include/adamvs_hip.h describes them (ada_mvs_amd/fusion.py::relative_transforms forms them in fp64).
    -> (count [H, W] uint8, fused [H, W] fp32, block_kept [nblocks] int32 (uint32 in the C ABI))."""
    ref_depth = _dev(ref_depth, "ref_depth")
    ref_conf = _dev(ref_conf, "ref_conf")
    H, W = ref_depth.shape
    if tuple(ref_conf.shape) != (H, W):
        raise _lib.AdaMVSHipError("ref_conf %s != ref_depth %s" % (tuple(ref_conf.shape), (H, W)))
    arr = (_lib.FusionSource * max(len(sources), 1))()
    keep = []
    for i, (dep, fwd, back) in enumerate(sources):
        dep = _dev(dep, "source depth %d" % i)
        keep.append(dep)
        arr[i].depth = dep.data_ptr()
        arr[i].H, arr[i].W = dep.shape
        arr[i].fwd[:] = [float(v) for v in fwd]
        arr[i].back[:] = [float(v) for v in back]
    count = torch.empty(H, W, device=ref_depth.device, dtype=torch.uint8)
    fused = torch.empty(H, W, device=ref_depth.device, dtype=torch.float32)
    block_kept = torch.empty(fusion_blocks(H, W), device=ref_depth.device, dtype=torch.int32)
    check(_lib.load().adamvs_geo_consistency(_p(ref_depth), _p(ref_conf), H, W, arr, len(sources), float(prob_threshold),
                                             float(pix_threshold), float(rel_depth_threshold), int(min_consistent), _p(count),
                                             _p(fused), _p(block_kept), _stream()), "geo_consistency")
    return count, fused, block_kept


def emit_points(fused, block_kept, rgba, camera, xyz=None, rgb=None):
    """adamvs_fusion_scan + adamvs_fusion_emit.  fused [H, W] fp32 and block_kept from geo_consistency, rgba [H, W, 4] uint8,
    camera: 21 float64 {K^-1 (9), R_wc (9), C (3)} (host).  -> (xyz [H W, 3] float64, rgb [H W, 3] uint8, offsets [nblocks + 1]
    int32): points 0 .. offsets[-1] are valid, in row-major pixel order.  xyz / rgb: reusable buffers of at least H W points."""
    import numpy as np
    fused = _dev(fused, "fused")
    block_kept = _dev_as(block_kept, "block_kept", torch.int32)
    rgba = _dev_as(rgba, "rgba", torch.uint8)
    H, W = fused.shape
    if tuple(rgba.shape) != (H, W, 4):
        raise _lib.AdaMVSHipError("rgba %s != (%d, %d, 4)" % (tuple(rgba.shape), H, W))
    nb = fusion_blocks(H, W)
    if block_kept.numel() != nb:
        raise _lib.AdaMVSHipError("block_kept holds %d counts, [%d, %d] needs %d" % (block_kept.numel(), H, W, nb))
    cam = np.ascontiguousarray(np.asarray(camera, dtype=np.float64).reshape(-1))
    if cam.size != 21:
        raise _lib.AdaMVSHipError("camera: 21 doubles {K^-1, R_wc, C}, got %d" % cam.size)
    if xyz is None:
        xyz = torch.empty(H * W, 3, device=fused.device, dtype=torch.float64)
    if rgb is None:
        rgb = torch.empty(H * W, 3, device=fused.device, dtype=torch.uint8)
    cap = min(xyz.shape[0], rgb.shape[0])
    if xyz.dtype != torch.float64 or rgb.dtype != torch.uint8 or not (xyz.is_contiguous() and rgb.is_contiguous()):
        raise _lib.AdaMVSHipError("xyz must be contiguous float64 [n, 3], rgb contiguous uint8 [n, 3]")
    offsets = torch.empty(nb + 1, device=fused.device, dtype=torch.int32)
    lib = _lib.load()
    check(lib.adamvs_fusion_scan(_p(block_kept), _p(offsets), nb, _stream()), "fusion_scan")
    check(lib.adamvs_fusion_emit(_p(fused), _p(rgba), H, W, cam.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _p(offsets),
                                 _p(xyz), _p(rgb), cap, _stream()), "fusion_emit")
    return xyz, rgb, offsets


# ---- DSM rasterisation (csrc/dsm.hip; driven chunk by chunk by ada_mvs_amd/dsm.py::DsmBuilder) ---------------------------
# Cell state as torch tensors of the signed type of each C type's width (key int64 = uint64, count / color int32 = uint32,
# sum int64); dsm.py reads them back through numpy views of the unsigned types.
def _dsm_grid(grid):
    g = _lib.DsmGrid()
    g.x0, g.y_top, g.gsd, g.z_ref = float(grid.x0), float(grid.y_top), float(grid.gsd), float(grid.z_ref)
    g.W, g.H = int(grid.W), int(grid.H)
    return g


def _dsm_points(xyz, rgb=None):
    xyz = _dev_as(xyz, "xyz", torch.float64)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise _lib.AdaMVSHipError("xyz must be [n, 3], got %s" % (tuple(xyz.shape),))
    if rgb is not None:
        rgb = _dev_as(rgb, "rgb", torch.uint8)
        if tuple(rgb.shape) != (xyz.shape[0], 3):
            raise _lib.AdaMVSHipError("rgb %s != (%d, 3)" % (tuple(rgb.shape), xyz.shape[0]))
    return xyz, rgb


def _dsm_cells(t, name, dtype, grid):
    if _dev_as(t, name, dtype) is not t:          # the kernels write the state in place: a contiguous copy would lose it
        raise _lib.AdaMVSHipError("%s must be contiguous" % name)
    if t.numel() != int(grid.W) * int(grid.H):
        raise _lib.AdaMVSHipError("%s holds %d cells, the grid has %d x %d" % (name, t.numel(), grid.H, grid.W))
    return t


def dsm_accumulate(grid, xyz, seq0, mode, key, count, sum_=None):
    """adamvs_dsm_accumulate: points xyz [n, 3] float64 (device) with sequence numbers seq0 .. seq0 + n - 1 into the cell state
    key [H W] int64, count [H W] int32 and, in mean mode, sum_ [H W] int64."""
    xyz, _ = _dsm_points(xyz)
    key = _dsm_cells(key, "key", torch.int64, grid)
    count = _dsm_cells(count, "count", torch.int32, grid)
    sp = None if sum_ is None else _p(_dsm_cells(sum_, "sum", torch.int64, grid))
    if xyz.shape[0] == 0:                         # nothing to launch (an empty tensor has no data pointer)
        return
    g = _dsm_grid(grid)
    check(_lib.load().adamvs_dsm_accumulate(ctypes.byref(g), _p(xyz), xyz.shape[0], int(seq0), int(mode), _p(key), _p(count), sp, _stream()),
          "dsm_accumulate")


def dsm_claim(grid, xyz, rgb, seq0, key, color):
    """adamvs_dsm_claim: after dsm_accumulate of the same points, the max-key point of each cell writes its colour into
    color [H W] int32 (RGBA bytes)."""
    xyz, rgb = _dsm_points(xyz, rgb)
    key = _dsm_cells(key, "key", torch.int64, grid)
    color = _dsm_cells(color, "color", torch.int32, grid)
    if xyz.shape[0] == 0:
        return
    g = _dsm_grid(grid)
    check(_lib.load().adamvs_dsm_claim(ctypes.byref(g), _p(xyz), _p(rgb), xyz.shape[0], int(seq0), _p(key), _p(color), _stream()), "dsm_claim")


def dsm_finalize(grid, key, count, sum_, color, mode, min_count):
    """adamvs_dsm_finalize -> (dsm [H, W] float32, count16 [H, W] int16 (uint16 in the C ABI), rgba [H, W, 4] uint8), device."""
    key = _dsm_cells(key, "key", torch.int64, grid)
    count = _dsm_cells(count, "count", torch.int32, grid)
    color = _dsm_cells(color, "color", torch.int32, grid)
    sp = None if sum_ is None else _p(_dsm_cells(sum_, "sum", torch.int64, grid))
    H, W = int(grid.H), int(grid.W)
    dev = key.device
    dsm = torch.empty(H, W, device=dev, dtype=torch.float32)
    count16 = torch.empty(H, W, device=dev, dtype=torch.int16)
    rgba = torch.empty(H, W, 4, device=dev, dtype=torch.uint8)
    g = _dsm_grid(grid)
    check(_lib.load().adamvs_dsm_finalize(ctypes.byref(g), _p(key), _p(count), sp, _p(color), int(mode), int(min_count), _p(dsm),
                                          _p(count16), _p(rgba), _stream()), "dsm_finalize")
    return dsm, count16, rgba


def dsm_fill(dsm, rgba, r_cells, tol_height=1e-6, tol_colour=1e-3, max_cycles=200, workspace=None):
    """adamvs_dsm_fill: bounded harmonic gap fill of a finalised DSM (dsm [H, W] float32, rgba [H, W, 4] uint8, device) ->
    (dsm_out float32, rgba_out uint8, dist2 [H, W] int32, filled [H, W] uint8, _lib.DsmFillStats).  Blocks until done."""
    dsm = _dev_as(dsm, "dsm", torch.float32)
    rgba = _dev_as(rgba, "rgba", torch.uint8)
    if dsm.dim() != 2:
        raise _lib.AdaMVSHipError("dsm must be [H, W], got %s" % (tuple(dsm.shape),))
    H, W = dsm.shape
    if tuple(rgba.shape) != (H, W, 4):
        raise _lib.AdaMVSHipError("rgba %s != (%d, %d, 4)" % (tuple(rgba.shape), H, W))
    lib = _lib.load()
    need = lib.adamvs_dsm_fill_workspace_bytes(W, H)
    check(0 if need >= 0 else int(need), "dsm_fill_workspace_bytes")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=dsm.device, dtype=torch.uint8)
    dsm_out = torch.empty_like(dsm)
    rgba_out = torch.empty_like(rgba)
    dist2 = torch.empty(H, W, device=dsm.device, dtype=torch.int32)
    filled = torch.empty(H, W, device=dsm.device, dtype=torch.uint8)
    stats = _lib.DsmFillStats()
    check(lib.adamvs_dsm_fill(W, H, _p(dsm), _p(rgba), float(r_cells), float(tol_height), float(tol_colour), int(max_cycles), _p(workspace),
                              workspace.numel(), _p(dsm_out), _p(rgba_out), _p(dist2), _p(filled), ctypes.byref(stats), _stream()),
          "dsm_fill")
    return dsm_out, rgba_out, dist2, filled, stats


def _workspace(entry_point, device, workspace, *args):
    """The caller's byte workspace where it holds the adamvs_<entry_point>(*args) bytes a call needs, otherwise a new one."""
    need = getattr(_lib.load(), "adamvs_" + entry_point)(*args)
    check(0 if need >= 0 else int(need), entry_point)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=device, dtype=torch.uint8)
    return workspace


def _dtm_raster(dsm, workspace):
    dsm = _dev_as(dsm, "dsm", torch.float32)
    if dsm.dim() != 2:
        raise _lib.AdaMVSHipError("dsm must be [H, W], got %s" % (tuple(dsm.shape),))
    H, W = dsm.shape
    return dsm, H, W, _workspace("dtm_workspace_bytes", dsm.device, workspace, W, H)


def dsm_open(dsm, r, workspace=None):
    """adamvs_dsm_open: one grey-scale opening with the square window of radius r cells (dsm [H, W] float32, device; empty
    cells NaN) -> opened [H, W] float32.  Enqueued on the current stream."""
    dsm, H, W, workspace = _dtm_raster(dsm, workspace)
    out = torch.empty_like(dsm)
    check(_lib.load().adamvs_dsm_open(W, H, _p(dsm), int(r), _p(workspace), workspace.numel(), _p(out), _stream()), "dsm_open")
    return out


def dtm_classify(dsm, radius, dh, workspace=None):
    """adamvs_dtm_classify: the progressive morphological ground filter (dsm [H, W] float32, device; radius: ascending integer
    radii in cells, dh: one height threshold per radius, host sequences) -> (level [H, W] uint8 (0 ground, k flagged at level
    k, 255 empty), opened [H, W] float32, _lib.DtmStats).  Blocks until done."""
    dsm, H, W, workspace = _dtm_raster(dsm, workspace)
    radius = [int(v) for v in radius]
    dh = [float(v) for v in dh]
    if len(radius) != len(dh):
        raise _lib.AdaMVSHipError("%d radii, %d thresholds" % (len(radius), len(dh)))
    K = len(radius)
    level = torch.empty(H, W, device=dsm.device, dtype=torch.uint8)
    opened = torch.empty_like(dsm)
    stats = _lib.DtmStats()
    check(_lib.load().adamvs_dtm_classify(W, H, _p(dsm), K, (ctypes.c_int * max(K, 1))(*radius), (ctypes.c_double * max(K, 1))(*dh),
                                          _p(workspace), workspace.numel(), _p(level), _p(opened), ctypes.byref(stats), _stream()),
          "dtm_classify")
    return level, opened, stats


def _raster(t, name, dtype, shape=None):
    """t as an [H, W] device raster of `dtype` (of the given shape, where one is given)"""
    t = _dev_as(t, name, dtype)
    if t.dim() != 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise _lib.AdaMVSHipError("%s must be [H, W]%s, got %s" % (name, "" if shape is None else " = %s" % (tuple(shape),), tuple(t.shape)))
    return t


def _number_roots(parent, spread=True):
    """parent [H, W] int32: a cell's root, itself at a root, negative outside -> (label [H, W] int32: 0 outside, otherwise the
    number 1 .. N of the cell's root in ascending cell index; N).  spread=False leaves out the look-up through parent: the
    label is then right at the roots only."""
    flat = parent.view(-1)
    root = flat == torch.arange(flat.numel(), device=parent.device, dtype=torch.int32)
    number = torch.cumsum(root, 0, dtype=torch.int32)               # the scan over the roots
    N = int(number[-1])
    if spread:
        number = torch.where(flat >= 0, number[flat.clamp(min=0).long()], torch.zeros((), device=parent.device, dtype=torch.int32))
    return number.view(parent.shape), N


def bld_flags(dsm, ndsm, min_height, r_open, s, smooth_tol, workspace=None):
    """adamvs_bld_flags: dsm, ndsm [H, W] float32 (device) -> flags [H, W] uint8 (0 not a candidate, 1 removed by the opening,
    2 undetermined, 3 smooth, 4 rough).  Enqueued on the current stream."""
    dsm = _raster(dsm, "dsm", torch.float32)
    ndsm = _raster(ndsm, "ndsm", torch.float32, dsm.shape)
    H, W = dsm.shape
    workspace = _workspace("bld_workspace_bytes", dsm.device, workspace, W, H)
    flags = torch.empty(H, W, device=dsm.device, dtype=torch.uint8)
    check(_lib.load().adamvs_bld_flags(W, H, _p(dsm), _p(ndsm), float(min_height), int(r_open), int(s), float(smooth_tol), _p(workspace),
                                       workspace.numel(), _p(flags), _stream()), "bld_flags")
    return flags


def bld_label(flags, workspace=None):
    """adamvs_bld_label and the numbering: flags [H, W] uint8 (device) -> (label [H, W] int32: 0 outside the mask flags >= 2,
    otherwise 1 .. N in ascending order of the component's smallest cell index; N; _lib.BldStats).  Blocks until done."""
    flags = _raster(flags, "flags", torch.uint8)
    H, W = flags.shape
    workspace = _workspace("bld_workspace_bytes", flags.device, workspace, W, H)
    parent = torch.empty(H, W, device=flags.device, dtype=torch.int32)
    stats = _lib.BldStats()
    check(_lib.load().adamvs_bld_label(W, H, _p(flags), _p(workspace), workspace.numel(), _p(parent), ctypes.byref(stats), _stream()),
          "bld_label")
    label, N = _number_roots(parent)
    return label, N, stats


def bld_table(flags, ndsm, label, N):
    """adamvs_bld_table: -> table [len(_lib.BLD_COLUMNS), N] int64 (device), row k - 1 of each column for component k.
    Enqueued on the current stream."""
    flags = _raster(flags, "flags", torch.uint8)
    ndsm = _raster(ndsm, "ndsm", torch.float32, flags.shape)
    label = _raster(label, "label", torch.int32, flags.shape)
    H, W = flags.shape
    table = torch.empty(len(_lib.BLD_COLUMNS), int(N), device=flags.device, dtype=torch.int64)
    check(_lib.load().adamvs_bld_table(W, H, _p(flags), _p(ndsm), _p(label), int(N), _p(table), _stream()), "bld_table")
    return table


# ---- Roof planes (csrc/dsm_roofs.hip; include/adamvs_hip.h "Roof planes") -----------------------------------------------------
def roof_links(dsm, building, s, smooth_tol, g_tol, step_tol):
    """adamvs_roof_links: dsm [H, W] float32, building [H, W] int32 (device) -> link [H, W] uint8 (bit 0 core, bit 1 east link,
    bit 2 south link).  Enqueued on the current stream."""
    dsm = _raster(dsm, "dsm", torch.float32)
    building = _raster(building, "building", torch.int32, dsm.shape)
    H, W = dsm.shape
    link = torch.empty(H, W, device=dsm.device, dtype=torch.uint8)
    check(_lib.load().adamvs_roof_links(W, H, _p(dsm), _p(building), int(s), float(smooth_tol), float(g_tol), float(step_tol), _p(link),
                                        _stream()), "roof_links")
    return link


def roof_label(link, workspace=None):
    """adamvs_roof_label and the numbering: link [H, W] uint8 (device; any bit pattern) -> (segment [H, W] int32: 0 where bit 0
    is clear, otherwise 1 .. S in ascending order of the segment's smallest cell index; S; parent [H, W] int32; _lib.BldStats).
    Blocks until done."""
    link = _raster(link, "link", torch.uint8)
    H, W = link.shape
    workspace = _workspace("roof_workspace_bytes", link.device, workspace, W, H)
    parent = torch.empty(H, W, device=link.device, dtype=torch.int32)
    stats = _lib.BldStats()
    check(_lib.load().adamvs_roof_label(W, H, _p(link), _p(workspace), workspace.numel(), _p(parent), ctypes.byref(stats), _stream()),
          "roof_label")
    seg, S = _number_roots(parent)
    return seg, S, parent, stats


def roof_moments(dsm, label, building, z_ref, N):
    """adamvs_roof_moments: -> table [len(_lib.ROOF_COLUMNS), N] int64 (device), row k - 1 of each column for label k.
    Enqueued on the current stream."""
    dsm = _raster(dsm, "dsm", torch.float32)
    label = _raster(label, "label", torch.int32, dsm.shape)
    building = _raster(building, "building", torch.int32, dsm.shape)
    H, W = dsm.shape
    table = torch.empty(len(_lib.ROOF_COLUMNS), int(N), device=dsm.device, dtype=torch.int64)
    check(_lib.load().adamvs_roof_moments(W, H, _p(dsm), _p(label), _p(building), float(z_ref), int(N), _p(table), _stream()), "roof_moments")
    return table


def _roof_planes(planes, device):
    planes = _dev_as(planes, "planes", torch.float64)
    if planes.dim() != 2 or planes.shape[1] != 3:
        raise _lib.AdaMVSHipError("planes must be [P, 3] float64, got %s" % (tuple(planes.shape),))
    return planes


def roof_grow(dsm, building, z_ref, planes, assign_tol, label0, label1, counts, round0, rounds):
    """adamvs_roof_grow: the rounds round0 .. round0 + rounds - 1, round k from label[k & 1] into label[(k + 1) & 1] (label0,
    label1 [H, W] int32, device), counts uint32-as-int32 [_lib.ROOF_MAX_GROW] (device).  Enqueued on the current stream."""
    dsm = _raster(dsm, "dsm", torch.float32)
    building = _raster(building, "building", torch.int32, dsm.shape)
    label0 = _raster(label0, "label0", torch.int32, dsm.shape)
    label1 = _raster(label1, "label1", torch.int32, dsm.shape)
    counts = _dev_as(counts, "counts", torch.int32)
    if counts.numel() != _lib.ROOF_MAX_GROW:
        raise _lib.AdaMVSHipError("counts must hold %d words, got %d" % (_lib.ROOF_MAX_GROW, counts.numel()))
    planes = _roof_planes(planes, dsm.device)
    H, W = dsm.shape
    check(_lib.load().adamvs_roof_grow(W, H, _p(dsm), _p(building), float(z_ref), planes.shape[0], _p(planes) if planes.shape[0] else None,
                                       float(assign_tol), int(round0), int(rounds), _p(label0), _p(label1), _p(counts), _stream()),
          "roof_grow")


def roof_residuals(dsm, label, z_ref, planes, assign_tol):
    """adamvs_roof_residuals: -> table [2, R] int64 (device): the inlier count and the largest llrint(e * 1024) per plane.
    Enqueued on the current stream."""
    dsm = _raster(dsm, "dsm", torch.float32)
    label = _raster(label, "label", torch.int32, dsm.shape)
    planes = _roof_planes(planes, dsm.device)
    H, W = dsm.shape
    R = planes.shape[0]
    table = torch.empty(2, R, device=dsm.device, dtype=torch.int64)
    check(_lib.load().adamvs_roof_residuals(W, H, _p(dsm), _p(label), float(z_ref), R, _p(planes) if R else None, float(assign_tol),
                                            _p(table) if R else None, _stream()), "roof_residuals")
    return table


# ---- LoD2 solids (csrc/dsm_lod2.hip; include/adamvs_hip.h "LoD2 solids") ------------------------------------------------------
def _lod2_planes(planes):
    planes = _dev_as(planes, "planes", torch.int64)
    if planes.dim() != 2 or planes.shape[1] != 3:
        raise _lib.AdaMVSHipError("planes must be [P, 3] int64, got %s" % (tuple(planes.shape),))
    return planes


def lod2_corner_heights_host(planes, plane, row, col):
    """adamvs_lod2_corner_heights_host: planes int64 [P, 3], plane (1 .. P), row, col: equal-length integer sequences (host) ->
    zq int64 (numpy): the device's own evaluation of a plane at a lattice corner, run on the host.  Needs no GPU."""
    import numpy as np
    planes = np.ascontiguousarray(planes, np.int64).reshape(-1, 3)
    plane, row, col = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (plane, row, col))
    if not plane.size == row.size == col.size:
        raise _lib.AdaMVSHipError("plane, row and col must have one length, got %d, %d, %d" % (plane.size, row.size, col.size))
    zq = np.empty(plane.size, np.int64)
    check(_lib.load().adamvs_lod2_corner_heights_host(planes.shape[0], planes.ctypes.data, plane.size, plane.ctypes.data, row.ctypes.data,
                                                      col.ctypes.data, zq.ctypes.data), "lod2_corner_heights_host")
    return zq


def lod2_fill(building, P, label0, label1, counts, round0, rounds):
    """adamvs_lod2_fill: the rounds round0 .. round0 + rounds - 1, round k from label[k & 1] into label[(k + 1) & 1] (label0,
    label1 [H, W] int32, device), counts uint32-as-int32 [_lib.LOD2_MAX_FILL] (device).  Enqueued on the current stream."""
    building = _raster(building, "building", torch.int32)
    label0 = _raster(label0, "label0", torch.int32, building.shape)
    label1 = _raster(label1, "label1", torch.int32, building.shape)
    counts = _dev_as(counts, "counts", torch.int32)
    if counts.numel() != _lib.LOD2_MAX_FILL:
        raise _lib.AdaMVSHipError("counts must hold %d words, got %d" % (_lib.LOD2_MAX_FILL, counts.numel()))
    H, W = building.shape
    check(_lib.load().adamvs_lod2_fill(W, H, _p(building), int(P), int(round0), int(rounds), _p(label0), _p(label1), _p(counts), _stream()),
          "lod2_fill")


def lod2_table(dtm, building, label, z_ref, B, planes):
    """adamvs_lod2_table: -> table [len(_lib.LOD2_COLUMNS), B] int64 (device), row k - 1 of each column for building k.
    Enqueued on the current stream."""
    dtm = _raster(dtm, "dtm", torch.float32)
    building = _raster(building, "building", torch.int32, dtm.shape)
    label = _raster(label, "label", torch.int32, dtm.shape)
    planes = _lod2_planes(planes)
    H, W = dtm.shape
    P = planes.shape[0]
    table = torch.empty(len(_lib.LOD2_COLUMNS), int(B), device=dtm.device, dtype=torch.int64)
    check(_lib.load().adamvs_lod2_table(W, H, _p(dtm), _p(building), _p(label), float(z_ref), int(B), P, _p(planes) if P else None,
                                        _p(table) if B else None, _stream()), "lod2_table")
    return table


def lod2_transpose(src):
    """adamvs_lod2_transpose: src [H, W] int32 (device) -> [W, H].  Enqueued on the current stream."""
    src = _raster(src, "src", torch.int32)
    H, W = src.shape
    dst = torch.empty(W, H, device=src.device, dtype=torch.int32)
    check(_lib.load().adamvs_lod2_transpose(W, H, _p(src), _p(dst), _stream()), "lod2_transpose")
    return dst


def lod2_runs(label, planes, plane_base, workspace=None):
    """adamvs_lod2_transpose, adamvs_lod2_count, the read-back of the run count and adamvs_lod2_runs: label [H, W] int32 (device;
    the model labels, refused buildings zeroed), planes int64 [P, 3], plane_base int32 [P] (device) -> (records
    [len(_lib.LOD2_FIELDS), N] int32 (device) in ascending (orientation, line, start), N).  Blocks for the one word."""
    label = _raster(label, "label", torch.int32)
    planes = _lod2_planes(planes)
    plane_base = _dev_as(plane_base, "plane_base", torch.int32)
    P = planes.shape[0]
    if plane_base.dim() != 1 or plane_base.numel() != P:
        raise _lib.AdaMVSHipError("plane_base must be [P = %d] int32, got %s" % (P, tuple(plane_base.shape)))
    H, W = label.shape
    workspace = _workspace("lod2_workspace_bytes", label.device, workspace, W, H)
    label_t = lod2_transpose(label)
    total = torch.zeros(1, device=label.device, dtype=torch.int32)
    lib = _lib.load()
    check(lib.adamvs_lod2_count(W, H, _p(label), _p(label_t), P, _p(workspace), workspace.numel(), _p(total), _stream()), "lod2_count")
    N = int(total.item())
    records = torch.empty(len(_lib.LOD2_FIELDS), N, device=label.device, dtype=torch.int32)
    check(lib.adamvs_lod2_runs(W, H, _p(label), _p(label_t), P, _p(planes) if P else None, _p(plane_base) if P else None, N, _p(workspace),
                               workspace.numel(), _p(records) if N else None, _stream()), "lod2_runs")
    return records, N


# ---- Trees (csrc/dsm_trees.hip; include/adamvs_hip.h "Trees") -----------------------------------------------------------------
def tree_surface(ndsm, building, min_height, smooth_passes, workspace=None):
    """adamvs_tree_surface: ndsm [H, W] float32, building [H, W] int32 or None (device) -> (mask uint8, q int32, s int32 (-1
    outside the canopy), s_max int32 [1]), all on the device.  Enqueued on the current stream."""
    ndsm = _raster(ndsm, "ndsm", torch.float32)
    if building is not None:
        building = _raster(building, "building", torch.int32, ndsm.shape)
    H, W = ndsm.shape
    workspace = _workspace("tree_workspace_bytes", ndsm.device, workspace, W, H)
    mask = torch.empty(H, W, device=ndsm.device, dtype=torch.uint8)
    q = torch.empty(H, W, device=ndsm.device, dtype=torch.int32)
    s = torch.empty(H, W, device=ndsm.device, dtype=torch.int32)
    s_max = torch.empty(1, device=ndsm.device, dtype=torch.int32)
    check(_lib.load().adamvs_tree_surface(W, H, _p(ndsm), None if building is None else _p(building), float(min_height), int(smooth_passes),
                                          _p(workspace), workspace.numel(), _p(mask), _p(q), _p(s), _p(s_max), _stream()), "tree_surface")
    return mask, q, s, s_max


def tree_parents(s, thr, workspace=None):
    """adamvs_tree_parents: s [H, W] int32 (device), thr: the ascending thresholds thr[1 .. r_cap] (host integers, thr[1] = 0) ->
    (parent [H, W] int32, _lib.TreeStats with candidates, window_cells and ms_parents set).  Blocks until done."""
    s = _raster(s, "s", torch.int32)
    H, W = s.shape
    thr = [int(v) for v in thr]
    if any(v < -2 ** 31 or v >= 2 ** 31 for v in thr):
        raise _lib.AdaMVSHipError("tree_parents: thr must hold int32 values")
    workspace = _workspace("tree_workspace_bytes", s.device, workspace, W, H)
    parent = torch.empty(H, W, device=s.device, dtype=torch.int32)
    stats = _lib.TreeStats()
    check(_lib.load().adamvs_tree_parents(W, H, _p(s), len(thr), (ctypes.c_int * max(len(thr), 1))(*thr), _p(workspace), workspace.numel(),
                                          _p(parent), ctypes.byref(stats), _stream()), "tree_parents")
    return parent, stats


def tree_roots(parent, workspace=None, stats=None):
    """adamvs_tree_roots and the numbering: parent [H, W] int32 (device) -> (root [H, W] int32, number [H, W] int32: at a top its
    number 1 .. T in ascending cell index, T, _lib.TreeStats with rounds, converged, tops and ms_jump set; pass tree_parents'
    stats to have both calls' fields in one).  Blocks until done."""
    parent = _raster(parent, "parent", torch.int32)
    H, W = parent.shape
    workspace = _workspace("tree_workspace_bytes", parent.device, workspace, W, H)
    root = torch.empty(H, W, device=parent.device, dtype=torch.int32)
    stats = _lib.TreeStats() if stats is None else stats
    check(_lib.load().adamvs_tree_roots(W, H, _p(parent), _p(workspace), workspace.numel(), _p(root), ctypes.byref(stats), _stream()),
          "tree_roots")
    number, T = _number_roots(root, spread=False)                    # crowns reads it at the tops only
    return root, number, T, stats


def tree_crowns(s, root, number, ratio_pm, rc2):
    """adamvs_tree_crowns: -> (label [H, W] int32: the number of the cell's top where both tests hold, else 0; unassigned int64
    [1]: the canopy cells that fail one), on the device.  Enqueued on the current stream."""
    s = _raster(s, "s", torch.int32)
    root = _raster(root, "root", torch.int32, s.shape)
    number = _raster(number, "number", torch.int32, s.shape)
    H, W = s.shape
    label = torch.empty(H, W, device=s.device, dtype=torch.int32)
    unassigned = torch.empty(1, device=s.device, dtype=torch.int64)
    check(_lib.load().adamvs_tree_crowns(W, H, _p(s), _p(root), _p(number), int(ratio_pm), int(rc2), _p(label), _p(unassigned), _stream()),
          "tree_crowns")
    return label, unassigned


def tree_table(label, q, s, root, T):
    """adamvs_tree_table: -> table [len(_lib.TREE_COLUMNS), T] int64 (device), row k - 1 of each column for tree k.  Enqueued
    on the current stream."""
    label = _raster(label, "label", torch.int32)
    q = _raster(q, "q", torch.int32, label.shape)
    s = _raster(s, "s", torch.int32, label.shape)
    root = _raster(root, "root", torch.int32, label.shape)
    H, W = label.shape
    table = torch.empty(len(_lib.TREE_COLUMNS), int(T), device=label.device, dtype=torch.int64)
    check(_lib.load().adamvs_tree_table(W, H, _p(label), _p(q), _p(s), _p(root), int(T), _p(table) if T else None, _stream()), "tree_table")
    return table


# ---- Contours (csrc/dsm_contours.hip; include/adamvs_hip.h "Contours") ------------------------------------------------------
def _contour_levels(lev, what):
    lev = [int(v) for v in lev]
    if any(v < -2 ** 31 or v >= 2 ** 31 for v in lev):
        raise _lib.AdaMVSHipError("%s: lev must hold int32 values" % what)
    return len(lev), (ctypes.c_int * max(len(lev), 1))(*lev)


def _contour_array(t, name, dtype, n):
    t = _dev_as(t, name, dtype)
    if t.dim() != 1 or t.numel() != n:
        raise _lib.AdaMVSHipError("%s must be [%d], got %s" % (name, n, tuple(t.shape)))
    return t


def _pn(t):
    """the pointer of an array that may be empty (a null pointer then: the library accepts it where N or M is 0)"""
    return _p(t) if t.numel() else None


def contour_surface(z, z_ref, smooth_passes, workspace=None):
    """adamvs_contour_surface: z [H, W] float32 (device) -> (s int32 [H, W], INT32_MIN outside V; info int32 [3]: s_min, s_max, the
    finite cells out of range), on the device.  Enqueued on the current stream."""
    z = _raster(z, "z", torch.float32)
    H, W = z.shape
    workspace = _workspace("contour_workspace_bytes", z.device, workspace, W, H)
    s = torch.empty(H, W, device=z.device, dtype=torch.int32)
    info = torch.empty(3, device=z.device, dtype=torch.int32)
    check(_lib.load().adamvs_contour_surface(W, H, _p(z), float(z_ref), int(smooth_passes), _p(workspace), workspace.numel(), _p(s), _p(info),
                                             _stream()), "contour_surface")
    return s, info


def contour_count(s, lev, workspace=None):
    """adamvs_contour_count: s [H, W] int32 (device), lev: the strictly ascending level table (host integers) -> (count int32
    [H, W]: the segments per block, N, the workspace that holds the scanned offsets for contour_segments, _lib.ContourStats with
    segments and ms_count set).  Blocks until done."""
    s = _raster(s, "s", torch.int32)
    H, W = s.shape
    K, table = _contour_levels(lev, "contour_count")
    workspace = _workspace("contour_workspace_bytes", s.device, workspace, W, H)
    count = torch.empty(H, W, device=s.device, dtype=torch.int32)
    stats = _lib.ContourStats()
    check(_lib.load().adamvs_contour_count(W, H, _p(s), K, table, _p(workspace), workspace.numel(), _p(count), ctypes.byref(stats), _stream()),
          "contour_count")
    return count, int(stats.segments), workspace, stats


def contour_segments(s, lev, N, workspace):
    """adamvs_contour_segments: `workspace` as contour_count returned it -> (entry, exit, level, succ, pred), int32 [N] each, on
    the device.  Enqueued on the current stream."""
    s = _raster(s, "s", torch.int32)
    H, W = s.shape
    K, table = _contour_levels(lev, "contour_segments")
    workspace = _dev_as(workspace, "workspace", torch.uint8)
    out = [torch.empty(int(N), device=s.device, dtype=torch.int32) for _ in range(5)]
    check(_lib.load().adamvs_contour_segments(W, H, _p(s), K, table, int(N), _p(workspace), workspace.numel(), *[_pn(t) for t in out], _stream()),
          "contour_segments")
    return tuple(out)


def contour_rank(pred, workspace=None, stats=None):
    """adamvs_contour_rank: pred int32 [N] (device) -> (start int32 [N], rank int32 [N], closed uint8 [N], M, the workspace,
    _lib.ContourStats with rounds, rounds_min, rounds_dist, launched, converged, lines and ms_rank set; pass contour_count's
    stats to have both calls' fields in one).  Blocks until done."""
    pred = _dev_as(pred, "pred", torch.int32)
    if pred.dim() != 1:
        raise _lib.AdaMVSHipError("pred must be [N], got %s" % (tuple(pred.shape),))
    N = pred.numel()
    workspace = _workspace("contour_rank_workspace_bytes", pred.device, workspace, int(N))
    start = torch.empty(N, device=pred.device, dtype=torch.int32)
    rank = torch.empty(N, device=pred.device, dtype=torch.int32)
    closed = torch.empty(N, device=pred.device, dtype=torch.uint8)
    stats = _lib.ContourStats() if stats is None else stats
    check(_lib.load().adamvs_contour_rank(N, _pn(pred), _p(workspace), workspace.numel(), _pn(start), _pn(rank), _pn(closed), ctypes.byref(stats),
                                          _stream()), "contour_rank")
    return start, rank, closed, int(stats.lines), workspace, stats


def contour_lines(s, lev, segments, start, rank, closed, M, workspace=None):
    """adamvs_contour_lines: segments = contour_segments' five arrays -> (line_first int64 [M + 1], line_start int32 [M],
    line_level int32 [M], line_closed uint8 [M], vertex int64 [N + M, 3]), on the device.  Blocks until done."""
    s = _raster(s, "s", torch.int32)
    H, W = s.shape
    K, table = _contour_levels(lev, "contour_lines")
    entry, exit_, level, succ, _ = segments
    N, M = int(entry.numel()), int(M)
    entry, exit_, level, succ = (_contour_array(t, name, torch.int32, N) for t, name in ((entry, "entry"), (exit_, "exit"), (level, "level"),
                                                                                        (succ, "succ")))
    start, rank = _contour_array(start, "start", torch.int32, N), _contour_array(rank, "rank", torch.int32, N)
    closed = _contour_array(closed, "closed", torch.uint8, N)
    workspace = _workspace("contour_rank_workspace_bytes", s.device, workspace, int(N))
    line_first = torch.empty(M + 1, device=s.device, dtype=torch.int64)
    line_start = torch.empty(M, device=s.device, dtype=torch.int32)
    line_level = torch.empty(M, device=s.device, dtype=torch.int32)
    line_closed = torch.empty(M, device=s.device, dtype=torch.uint8)
    vertex = torch.empty(N + M, 3, device=s.device, dtype=torch.int64)
    check(_lib.load().adamvs_contour_lines(W, H, _p(s), K, table, N, M, _pn(entry), _pn(exit_), _pn(level), _pn(succ), _pn(start), _pn(rank),
                                           _pn(closed), _p(workspace), workspace.numel(), _p(line_first), _pn(line_start), _pn(line_level),
                                           _pn(line_closed), _pn(vertex), _stream()), "contour_lines")
    return line_first, line_start, line_level, line_closed, vertex


# ---- Drainage (csrc/dsm_drainage.hip; include/adamvs_hip.h "Drainage") ------------------------------------------------------
def _drain_stats(st):
    return dict(rounds=int(st.rounds), launched=int(st.launched), converged=int(st.converged), ms=float(st.ms))


def drain_fill(s, smooth_passes, max_rounds, workspace=None):
    """adamvs_drain_fill: s [H, W] int32 (device; contour_surface's, of the same smooth_passes) -> (r int32 [H, W], F int32
    [H, W], stats dict(rounds, launched, converged, ms), the workspace).  Blocks until done.  F is the fill only if converged."""
    s = _raster(s, "s", torch.int32)
    H, W = s.shape
    workspace = _workspace("drain_workspace_bytes", s.device, workspace, W, H)
    r, F = torch.empty_like(s), torch.empty_like(s)
    st = _lib.DrainStats()
    check(_lib.load().adamvs_drain_fill(W, H, _p(s), int(smooth_passes), int(max_rounds), _p(workspace), workspace.numel(), _p(r), _p(F),
                                        ctypes.byref(st), _stream()), "drain_fill")
    return r, F, _drain_stats(st), workspace


def drain_direction(F):
    """adamvs_drain_direction: F [H, W] int32 (device) -> dir uint8 [H, W].  Enqueued on the current stream."""
    F = _raster(F, "F", torch.int32)
    H, W = F.shape
    d = torch.empty(H, W, device=F.device, dtype=torch.uint8)
    check(_lib.load().adamvs_drain_direction(W, H, _p(F), _p(d), _stream()), "drain_direction")
    return d


def drain_accumulate(direction, value=None, workspace=None):
    """adamvs_drain_accumulate: dir [H, W] uint8 (device), value [H, W] int32 or None (1 per valid cell) -> (acc int32 [H, W],
    root int32 [H, W], stats, the workspace).  Blocks until done."""
    direction = _raster(direction, "dir", torch.uint8)
    H, W = direction.shape
    if value is not None:
        value = _raster(value, "value", torch.int32, direction.shape)
    workspace = _workspace("drain_workspace_bytes", direction.device, workspace, W, H)
    acc = torch.empty(H, W, device=direction.device, dtype=torch.int32)
    root = torch.empty_like(acc)
    st = _lib.DrainStats()
    check(_lib.load().adamvs_drain_accumulate(W, H, _p(direction), None if value is None else _p(value), _p(workspace), workspace.numel(),
                                              _p(acc), _p(root), ctypes.byref(st), _stream()), "drain_accumulate")
    return acc, root, _drain_stats(st), workspace


def drain_streams(direction, acc, min_cells, workspace=None):
    """adamvs_drain_streams: -> (nd uint8 [H, W], link int32 [H, W], pos int32 [H, W], L, P, stats, the workspace that holds the
    vertex offsets for drain_links).  Blocks until done."""
    direction = _raster(direction, "dir", torch.uint8)
    acc = _raster(acc, "acc", torch.int32, direction.shape)
    H, W = direction.shape
    workspace = _workspace("drain_workspace_bytes", direction.device, workspace, W, H)
    nd = torch.empty_like(direction)
    link, pos = torch.empty_like(acc), torch.empty_like(acc)
    st = _lib.DrainStats()
    check(_lib.load().adamvs_drain_streams(W, H, _p(direction), _p(acc), int(min_cells), _p(workspace), workspace.numel(), _p(nd), _p(link),
                                           _p(pos), ctypes.byref(st), _stream()), "drain_streams")
    return nd, link, pos, int(st.links), int(st.vertices), _drain_stats(st), workspace


def drain_links(direction, nd, link, pos, L, P, workspace):
    """adamvs_drain_links: `workspace` as drain_streams returned it -> (link_first int32 [L + 1], link_head, link_end, link_to
    int32 [L], vertex int32 [P]), on the device.  Enqueued on the current stream after one read-back."""
    direction = _raster(direction, "dir", torch.uint8)
    nd = _raster(nd, "nd", torch.uint8, direction.shape)
    link = _raster(link, "link", torch.int32, direction.shape)
    pos = _raster(pos, "pos", torch.int32, direction.shape)
    workspace = _dev_as(workspace, "workspace", torch.uint8)
    H, W = direction.shape
    L, P = int(L), int(P)
    dev = direction.device
    link_first = torch.empty(L + 1, device=dev, dtype=torch.int32)
    link_head, link_end, link_to = (torch.empty(L, device=dev, dtype=torch.int32) for _ in range(3))
    vertex = torch.empty(P, device=dev, dtype=torch.int32)
    check(_lib.load().adamvs_drain_links(W, H, _p(direction), _p(nd), _p(link), _p(pos), L, P, _p(workspace), workspace.numel(), _p(link_first),
                                         _pn(link_head), _pn(link_end), _pn(link_to), _pn(vertex), _stream()), "drain_links")
    return link_first, link_head, link_end, link_to, vertex


# ---- Solar (csrc/dsm_solar.hip; include/adamvs_hip.h "Solar") ----------------------------------------------------------------
def _solar_horizons(s, hz_n, hz_h):
    s = _raster(s, "s", torch.int32)
    H, W = s.shape
    hz_n, hz_h = _dev_as(hz_n, "hz_n", torch.int32), _dev_as(hz_h, "hz_h", torch.int32)
    if hz_n.dim() != 3 or tuple(hz_n.shape[1:]) != (H, W) or hz_h.shape != hz_n.shape:
        raise _lib.AdaMVSHipError("hz_n and hz_h must be [K, %d, %d], got %s and %s" % (H, W, tuple(hz_n.shape), tuple(hz_h.shape)))
    return s, hz_n, hz_h, H, W, int(hz_n.shape[0])


def solar_horizon(s, K, workspace=None):
    """adamvs_solar_horizon: s [H, W] int32 (device; contour_surface's with 0 smoothing passes) -> (hz_n int32 [K, H, W], hz_h int32
    [K, H, W], stats dict(lines, deepest, spills, ms), the workspace).  Blocks until done."""
    s = _raster(s, "s", torch.int32)
    H, W = s.shape
    K = int(K)
    workspace = _workspace("solar_workspace_bytes", s.device, workspace, W, H, K)
    hz_n = torch.empty(K, H, W, device=s.device, dtype=torch.int32)
    hz_h = torch.empty_like(hz_n)
    st = _lib.SolarStats()
    check(_lib.load().adamvs_solar_horizon(W, H, K, _p(s), _p(workspace), workspace.numel(), _p(hz_n), _p(hz_h), ctypes.byref(st), _stream()),
          "solar_horizon")
    return hz_n, hz_h, dict(lines=int(st.lines), deepest=int(st.deepest), spills=int(st.spills), ms=float(st.ms)), workspace


def solar_svf(s, hz_n, hz_h, weight, q):
    """adamvs_solar_svf: weight: the K sector weights (host floats), q = (256 gsd)^2 -> svf float64 [H, W].  Enqueued on the
    current stream."""
    s, hz_n, hz_h, H, W, K = _solar_horizons(s, hz_n, hz_h)
    weight = [float(v) for v in weight]
    if len(weight) != K:
        raise _lib.AdaMVSHipError("solar_svf: %d weights for K=%d directions" % (len(weight), K))
    svf = torch.empty(H, W, device=s.device, dtype=torch.float64)
    check(_lib.load().adamvs_solar_svf(W, H, K, _p(s), _p(hz_n), _p(hz_h), (ctypes.c_double * max(K, 1))(*weight), float(q), _p(svf), _stream()),
          "solar_svf")
    return svf


def solar_expose(s, hz_n, hz_h, table, label=None, normal=None, workspace=None):
    """adamvs_solar_expose: table = dict(sector int [T], thr float64 [T], minutes int [T], energy int [T], sun int [T, 3]) on the
    host, sorted by sector; label int32 [H, W] and normal int32 [P + 1, 3] (device) or neither -> (minutes int32 [H, W], direct
    int32 [H, W], the workspace).  Blocks until done."""
    import numpy as np
    s, hz_n, hz_h, H, W, K = _solar_horizons(s, hz_n, hz_h)
    T = len(table["sector"])
    cols = [np.ascontiguousarray(table[k], dt).reshape(-1) for k, dt in (("sector", np.int64), ("thr", np.float64), ("minutes", np.int64),
                                                                          ("energy", np.int64), ("sun", np.int64))]
    if [c.size for c in cols] != [T, T, T, T, 3 * T]:
        raise _lib.AdaMVSHipError("solar_expose: the columns of the table must hold T=%d rows" % T)
    if any(c.size and (c.min() < -2 ** 31 or c.max() >= 2 ** 31) for c in (cols[0], cols[2], cols[3], cols[4])):
        raise _lib.AdaMVSHipError("solar_expose: the table must hold int32 values")
    ints = [(ctypes.c_int * max(c.size, 1))(*c.tolist()) for c in (cols[0], cols[2], cols[3], cols[4])]
    thr = (ctypes.c_double * max(T, 1))(*cols[1].tolist())
    P = 0
    if (label is None) != (normal is None):
        raise _lib.AdaMVSHipError("solar_expose: label and normal go together")
    if label is not None:
        label = _raster(label, "label", torch.int32, (H, W))
        normal = _dev_as(normal, "normal", torch.int32)
        if normal.dim() != 2 or normal.shape[1] != 3 or normal.shape[0] < 1:
            raise _lib.AdaMVSHipError("normal must be [P + 1, 3], got %s" % (tuple(normal.shape),))
        P = int(normal.shape[0]) - 1
    if workspace is None or workspace.numel() < _lib.SOLAR_HEAD_BYTES:
        workspace = torch.empty(_lib.SOLAR_HEAD_BYTES, device=s.device, dtype=torch.uint8)
    minutes = torch.empty(H, W, device=s.device, dtype=torch.int32)
    direct = torch.empty_like(minutes)
    check(_lib.load().adamvs_solar_expose(W, H, K, _p(s), _p(hz_n), _p(hz_h), T, ints[0], thr, ints[1], ints[2], ints[3],
                                          None if label is None else _p(label), P, None if normal is None else _p(normal), _p(workspace),
                                          workspace.numel(), _p(minutes), _p(direct), _stream()), "solar_expose")
    return minutes, direct, workspace


def solar_plane_sums(s, minutes, direct, label=None, P=0):
    """adamvs_solar_plane_sums: -> table int64 [3, P + 1] (cells, minutes, direct per label over V; a null label counts every cell
    under label 0), on the device.  Enqueued on the current stream."""
    s = _raster(s, "s", torch.int32)
    H, W = s.shape
    minutes, direct = _raster(minutes, "minutes", torch.int32, (H, W)), _raster(direct, "direct", torch.int32, (H, W))
    if label is not None:
        label = _raster(label, "label", torch.int32, (H, W))
    P = int(P)
    table = torch.empty(3, max(P, 0) + 1, device=s.device, dtype=torch.int64)
    check(_lib.load().adamvs_solar_plane_sums(W, H, _p(s), None if label is None else _p(label), P, _p(minutes), _p(direct), _p(table), _stream()),
          "solar_plane_sums")
    return table


# ---- TSDF mesh (csrc/mesh.hip; driven brick by brick by ada_mvs_amd/mesh.py) ------------------------------------------------
# Per-sample state as torch tensors of the signed type of each C type's width: weight int16 = uint16, rgba int32 = uint32
# (little-endian r g b a), cube_code int32 = uint32, faces int32 = uint32.
def mesh_brick(origin, voxel, mu, B, b, min_weight=1):
    """-> _lib.MeshBrick (adamvs_mesh_brick) of brick b = (bx, by, bz)."""
    mb = _lib.MeshBrick()
    mb.origin[:] = [float(v) for v in origin]
    mb.voxel, mb.mu, mb.B, mb.min_weight = float(voxel), float(mu), int(B), int(min_weight)
    mb.bx, mb.by, mb.bz = (int(v) for v in b)
    return mb


def mesh_views(views, device):
    """views: list of (K [3, 3], R_cw [3, 3], c = C - O [3] (fp64, rounded here to fp32), depth [H, W] fp32, rgba [H, W, 4] uint8
    (device tensors)) -> the device array of adamvs_mesh_view (a uint8 tensor), checked by adamvs_mesh_check_views.  The depth and
    image tensors must outlive it."""
    arr = (_lib.MeshView * max(len(views), 1))()
    for i, (K, R, c, depth, rgba) in enumerate(views):
        depth = _dev_as(depth, "view %d depth" % i, torch.float32)
        rgba = _dev_as(rgba, "view %d rgba" % i, torch.uint8)
        if depth.dim() != 2 or tuple(rgba.shape) != tuple(depth.shape) + (4,):
            raise _lib.AdaMVSHipError("view %d: depth %s, rgba %s" % (i, tuple(depth.shape), tuple(rgba.shape)))
        arr[i].K[:] = [float(v) for v in K.reshape(-1)]
        arr[i].R[:] = [float(v) for v in R.reshape(-1)]
        arr[i].c[:] = [float(v) for v in c]
        arr[i].H, arr[i].W = depth.shape
        arr[i].depth, arr[i].rgba = depth.data_ptr(), rgba.data_ptr()
    check(_lib.load().adamvs_mesh_check_views(arr, len(views)), "mesh_check_views")
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device)


def _mesh_sizes(B):
    S = (B + 1) ** 3
    return S, (S + _lib.MESH_TILE - 1) // _lib.MESH_TILE, B ** 3 // _lib.MESH_TILE


def tsdf_integrate(brick, views_dev, nviews, view_list):
    """adamvs_tsdf_integrate.  brick: _lib.MeshBrick; views_dev from mesh_views; view_list: device int32 [n] (sorted, conservative).
    -> (tsdf [(B+1)^3] float32, weight int16 (uint16), rgba int32 (uint32 r g b a))."""
    views_dev = _dev_as(views_dev, "views", torch.uint8)
    view_list = _dev_as(view_list, "view_list", torch.int32)
    S, _, _ = _mesh_sizes(brick.B)
    dev = views_dev.device
    tsdf = torch.empty(S, device=dev, dtype=torch.float32)
    weight = torch.empty(S, device=dev, dtype=torch.int16)
    rgba = torch.empty(S, device=dev, dtype=torch.int32)
    check(_lib.load().adamvs_tsdf_integrate(ctypes.byref(brick), _p(views_dev), int(nviews), _p(view_list), view_list.numel(), _p(tsdf),
                                            _p(weight), _p(rgba), _stream()), "tsdf_integrate")
    return tsdf, weight, rgba


def mesh_extract(brick, tsdf, weight, rgba, vertex_base=0):
    """adamvs_mesh_classify + _count_vertices + two adamvs_fusion_scan + adamvs_mesh_emit on one brick's volume.  Reads the two
    totals back (one synchronisation).  -> (xyz [nv, 3] float64, rgb [nv, 3] uint8, faces [nt, 3] int32 (uint32: vertex_base +
    brick-local index)), device tensors."""
    tsdf = _dev(tsdf, "tsdf")
    weight = _dev_as(weight, "weight", torch.int16)
    rgba = _dev_as(rgba, "rgba", torch.int32)
    B = brick.B
    S, nbs, nbc = _mesh_sizes(B)
    if tsdf.numel() != S or weight.numel() != S or rgba.numel() != S:
        raise _lib.AdaMVSHipError("B=%d needs %d samples: tsdf %d, weight %d, rgba %d" % (B, S, tsdf.numel(), weight.numel(), rgba.numel()))
    dev = tsdf.device
    lib = _lib.load()
    code = torch.empty(B ** 3, device=dev, dtype=torch.int32)
    mask = torch.empty(S, device=dev, dtype=torch.uint8)
    counts = torch.empty(nbc + nbs, device=dev, dtype=torch.int32)
    offs = torch.empty(nbc + 1 + nbs + 1, device=dev, dtype=torch.int32)
    block_tris, block_verts = counts[:nbc], counts[nbc:]
    tri_off, vert_off = offs[:nbc + 1], offs[nbc + 1:]
    st = _stream()
    check(lib.adamvs_mesh_classify(ctypes.byref(brick), _p(tsdf), _p(weight), _p(code), _p(block_tris), st), "mesh_classify")
    check(lib.adamvs_mesh_count_vertices(ctypes.byref(brick), _p(tsdf), _p(code), _p(mask), _p(block_verts), st), "mesh_count_vertices")
    check(lib.adamvs_fusion_scan(_p(block_tris), _p(tri_off), nbc, st), "fusion_scan")
    check(lib.adamvs_fusion_scan(_p(block_verts), _p(vert_off), nbs, st), "fusion_scan")
    nt, nv = (int(v) & 0xFFFFFFFF for v in torch.stack([tri_off[-1], vert_off[-1]]).cpu().tolist())
    if int(vertex_base) + nv > 0xFFFFFFFF:
        raise _lib.AdaMVSHipError("mesh: more than 2^32 - 1 vertices")
    xyz = torch.empty(max(nv, 1), 3, device=dev, dtype=torch.float64)
    rgb = torch.empty(max(nv, 1), 3, device=dev, dtype=torch.uint8)
    faces = torch.empty(max(nt, 1), 3, device=dev, dtype=torch.int32)
    first = torch.empty(S, device=dev, dtype=torch.int32)
    check(lib.adamvs_mesh_emit(ctypes.byref(brick), _p(tsdf), _p(rgba), _p(code), _p(mask), _p(vert_off), _p(tri_off), int(vertex_base),
                               _p(xyz), _p(rgb), _p(first), nv, _p(faces), nt, st), "mesh_emit")
    return xyz[:nv], rgb[:nv], faces[:nt]


# ---- mesh simplification (csrc/mesh_simplify.hip; driven by ada_mvs_amd/simplify.py) -------------------------------------------
# faces and new indices int32 = uint32, the colour sums int64 = uint64; flags uint8.
def _lattice(origin, cell):
    o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(-1))
    if o.size != 3:
        raise _lib.AdaMVSHipError("lattice origin: 3 doubles, got %d" % o.size)
    return o, o.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), float(cell)


def simplify_keys(xyz, cell, origin):
    """adamvs_simplify_keys.  xyz [nv, 3] float64 -> (keys [nv] int64, bad [nv] uint8: 0 fine, 1 not finite, 2 outside the lattice)."""
    xyz = _dev_as(xyz, "xyz", torch.float64)
    nv = xyz.shape[0]
    keep, o, c = _lattice(origin, cell)
    keys = torch.empty(nv, device=xyz.device, dtype=torch.int64)
    bad = torch.empty(nv, device=xyz.device, dtype=torch.uint8)
    check(_lib.load().adamvs_simplify_keys(o, c, _p(xyz), nv, _p(keys), _p(bad), _stream()), "simplify_keys")
    return keys, bad


def simplify_corners(faces, vcell, nc):
    """adamvs_simplify_corners.  faces [nf, 3] int32 (uint32), vcell [nv] int32 -> (fcell [nf, 3] int32, entry_cell [nf, 3] int32,
    survive [nf] uint8)."""
    faces = _dev_as(faces, "faces", torch.int32)
    vcell = _dev_as(vcell, "vcell", torch.int32)
    nf, dev = faces.shape[0], faces.device
    fcell = torch.empty(nf, 3, device=dev, dtype=torch.int32)
    entry_cell = torch.empty(nf, 3, device=dev, dtype=torch.int32)
    survive = torch.empty(nf, device=dev, dtype=torch.uint8)
    check(_lib.load().adamvs_simplify_corners(_p(faces), nf, _p(vcell), vcell.numel(), int(nc), _p(fcell), _p(entry_cell), _p(survive),
                                              _stream()), "simplify_corners")
    return fcell, entry_cell, survive


def simplify_accumulate(keys, cell, origin, xyz, rgb, faces, entry, fstart, vorder, vstart):
    """adamvs_simplify_accumulate.  keys [nc] int64 (the cells), entry [3 nf] / vorder [nv] int64 (stable sort orders), fstart / vstart
    [nc + 1] int64 -> (quadric [nc, 10] float64, member [nc, 3] float64, colour [nc, 3] int64)."""
    keys = _dev_as(keys, "keys", torch.int64)
    xyz = _dev_as(xyz, "xyz", torch.float64)
    rgb = _dev_as(rgb, "rgb", torch.uint8)
    faces = _dev_as(faces, "faces", torch.int32)
    entry, fstart = _dev_as(entry, "entry", torch.int64), _dev_as(fstart, "fstart", torch.int64)
    vorder, vstart = _dev_as(vorder, "vorder", torch.int64), _dev_as(vstart, "vstart", torch.int64)
    nc, nv, nf, dev = keys.numel(), xyz.shape[0], faces.shape[0], xyz.device
    if rgb.shape[0] != nv or entry.numel() != 3 * nf or vorder.numel() != nv or fstart.numel() != nc + 1 or vstart.numel() != nc + 1:
        raise _lib.AdaMVSHipError("simplify_accumulate: nv %d, nf %d, nc %d against rgb %d, entry %d, vorder %d, fstart %d, vstart %d"
                                  % (nv, nf, nc, rgb.shape[0], entry.numel(), vorder.numel(), fstart.numel(), vstart.numel()))
    keep, o, c = _lattice(origin, cell)
    quadric = torch.empty(nc, 10, device=dev, dtype=torch.float64)
    member = torch.empty(nc, 3, device=dev, dtype=torch.float64)
    colour = torch.empty(nc, 3, device=dev, dtype=torch.int64)
    check(_lib.load().adamvs_simplify_accumulate(o, c, _p(keys), nc, _p(xyz), _p(rgb), nv, _p(faces), nf, _p(entry), _p(fstart), _p(vorder),
                                                 _p(vstart), _p(quadric), _p(member), _p(colour), _stream()), "simplify_accumulate")
    return quadric, member, colour


def simplify_solve(keys, cell, origin, rank_eps, quadric, member, colour, vstart):
    """adamvs_simplify_solve -> (pos [nc, 3] float64, col [nc, 3] uint8, rank [nc] uint8, fallback [nc] uint8, error [nc] float64)."""
    keys = _dev_as(keys, "keys", torch.int64)
    quadric, member = _dev_as(quadric, "quadric", torch.float64), _dev_as(member, "member", torch.float64)
    colour, vstart = _dev_as(colour, "colour", torch.int64), _dev_as(vstart, "vstart", torch.int64)
    nc, dev = keys.numel(), keys.device
    if quadric.numel() != 10 * nc or member.numel() != 3 * nc or colour.numel() != 3 * nc or vstart.numel() != nc + 1:
        raise _lib.AdaMVSHipError("simplify_solve: nc %d against quadric %d, member %d, colour %d, vstart %d"
                                  % (nc, quadric.numel(), member.numel(), colour.numel(), vstart.numel()))
    keep, o, c = _lattice(origin, cell)
    pos = torch.empty(nc, 3, device=dev, dtype=torch.float64)
    col = torch.empty(nc, 3, device=dev, dtype=torch.uint8)
    rank = torch.empty(nc, device=dev, dtype=torch.uint8)
    fallback = torch.empty(nc, device=dev, dtype=torch.uint8)
    error = torch.empty(nc, device=dev, dtype=torch.float64)
    check(_lib.load().adamvs_simplify_solve(o, c, float(rank_eps), _p(keys), nc, _p(quadric), _p(member), _p(colour), _p(vstart), _p(pos),
                                            _p(col), _p(rank), _p(fallback), _p(error), _stream()), "simplify_solve")
    return pos, col, rank, fallback, error


def simplify_solve_host(quadric, mean, cell, rank_eps=1e-3):
    """adamvs_simplify_solve_host on numpy arrays: quadric [n, 10], mean [n, 3] -> (p [n, 3], rank [n], fallback [n], error [n])."""
    q = np.ascontiguousarray(np.asarray(quadric, np.float64).reshape(-1, 10))
    m = np.ascontiguousarray(np.asarray(mean, np.float64).reshape(-1, 3))
    n = len(q)
    if len(m) != n:
        raise _lib.AdaMVSHipError("simplify_solve_host: %d quadrics, %d means" % (n, len(m)))
    p, rank, fb, err = np.zeros((n, 3)), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n)
    check(_lib.load().adamvs_simplify_solve_host(q.ctypes.data, m.ctypes.data, n, float(cell), float(rank_eps), p.ctypes.data,
                                                 rank.ctypes.data, fb.ctypes.data, err.ctypes.data), "simplify_solve_host")
    return p, rank, fb, err


def simplify_triples(fcell, surv):
    """adamvs_simplify_triples.  surv [ns] int64 (surviving faces, ascending) -> tri [3, ns] int32."""
    fcell = _dev_as(fcell, "fcell", torch.int32)
    surv = _dev_as(surv, "surv", torch.int64)
    tri = torch.empty(3, surv.numel(), device=fcell.device, dtype=torch.int32)
    check(_lib.load().adamvs_simplify_triples(_p(fcell), fcell.shape[0], _p(surv), surv.numel(), _p(tri), _stream()), "simplify_triples")
    return tri


def simplify_first(tri, surv, order, nf):
    """adamvs_simplify_first -> keep [nf] uint8 (zero outside the surviving faces)."""
    tri = _dev_as(tri, "tri", torch.int32)
    surv, order = _dev_as(surv, "surv", torch.int64), _dev_as(order, "order", torch.int64)
    ns = surv.numel()
    if tri.numel() != 3 * ns or order.numel() != ns:
        raise _lib.AdaMVSHipError("simplify_first: ns %d against tri %d, order %d" % (ns, tri.numel(), order.numel()))
    keep = torch.zeros(int(nf), device=tri.device, dtype=torch.uint8)
    check(_lib.load().adamvs_simplify_first(_p(tri), _p(surv), _p(order), ns, int(nf), _p(keep), _stream()), "simplify_first")
    return keep


def simplify_emit(pos, col, fcell, keep):
    """adamvs_simplify_mark + two adamvs_simplify_count + two adamvs_fusion_scan + adamvs_simplify_emit.  Reads the two totals back
    (one synchronisation).  -> (xyz [nu, 3] float64, rgb [nu, 3] uint8, faces [nk, 3] int32 (uint32), used [nc] uint8)."""
    pos, col = _dev_as(pos, "pos", torch.float64), _dev_as(col, "col", torch.uint8)
    fcell, keep = _dev_as(fcell, "fcell", torch.int32), _dev_as(keep, "keep", torch.uint8)
    nc, nf, dev = pos.shape[0], fcell.shape[0], pos.device
    if col.shape[0] != nc or keep.numel() != nf:
        raise _lib.AdaMVSHipError("simplify_emit: nc %d, nf %d against col %d, keep %d" % (nc, nf, col.shape[0], keep.numel()))
    T = _lib.SIMPLIFY_TILE
    nbc, nbf = (nc + T - 1) // T, (nf + T - 1) // T
    lib, st = _lib.load(), _stream()
    used = torch.zeros(nc, device=dev, dtype=torch.uint8)
    counts = torch.empty(nbc + nbf, device=dev, dtype=torch.int32)
    offs = torch.empty(nbc + 1 + nbf + 1, device=dev, dtype=torch.int32)
    cell_off, face_off = offs[:nbc + 1], offs[nbc + 1:]
    check(lib.adamvs_simplify_mark(_p(fcell), _p(keep), nf, nc, _p(used), st), "simplify_mark")
    check(lib.adamvs_simplify_count(_p(used), nc, _p(counts[:nbc]), st), "simplify_count")
    check(lib.adamvs_simplify_count(_p(keep), nf, _p(counts[nbc:]), st), "simplify_count")
    check(lib.adamvs_fusion_scan(_p(counts[:nbc]), _p(cell_off), nbc, st), "fusion_scan")
    check(lib.adamvs_fusion_scan(_p(counts[nbc:]), _p(face_off), nbf, st), "fusion_scan")
    nu, nk = (int(v) & 0xFFFFFFFF for v in torch.stack([cell_off[-1], face_off[-1]]).cpu().tolist())
    xyz = torch.empty(max(nu, 1), 3, device=dev, dtype=torch.float64)
    rgb = torch.empty(max(nu, 1), 3, device=dev, dtype=torch.uint8)
    faces = torch.empty(max(nk, 1), 3, device=dev, dtype=torch.int32)
    new_index = torch.empty(nc, device=dev, dtype=torch.int32)
    check(lib.adamvs_simplify_emit(_p(pos), _p(col), _p(used), nc, _p(cell_off), _p(fcell), _p(keep), nf, _p(face_off), _p(xyz), _p(rgb),
                                   _p(new_index), nu, _p(faces), nk, st), "simplify_emit")
    return xyz[:nu], rgb[:nu], faces[:nk], used


# ---- cloud distance (csrc/cloud_dist.hip; driven by ada_mvs_amd/accuracy.py) -----------------------------------------------------
# keys and orders int64, target numbers int32, d2 float32, index int32, pair counts int64 = uint64.
def cloud_nearest(origin, D, ukeys, tstart, targets_sorted, tindex, queries, qorder, item_key, item_first, item_count):
    """adamvs_cloud_nearest.  ukeys [nc] / tstart [nc + 1] int64 (the occupied target cells and their runs), targets_sorted [nt, 3]
    float64 with tindex [nt] int32 (their numbers in the caller's order), queries [nq, 3] float64, qorder [nqs] int64, the work items
    (item_key, item_first int64, item_count int32) -> (d2 [nq] float32, index [nq] int32, pairs [ni] int64); +inf and -1 where no
    target lies within D."""
    ukeys, tstart = _dev_as(ukeys, "ukeys", torch.int64), _dev_as(tstart, "tstart", torch.int64)
    targets_sorted, tindex = _dev_as(targets_sorted, "targets_sorted", torch.float64), _dev_as(tindex, "tindex", torch.int32)
    queries, qorder = _dev_as(queries, "queries", torch.float64), _dev_as(qorder, "qorder", torch.int64)
    item_key, item_first = _dev_as(item_key, "item_key", torch.int64), _dev_as(item_first, "item_first", torch.int64)
    item_count = _dev_as(item_count, "item_count", torch.int32)
    nc, nt, nq, nqs, ni, dev = ukeys.numel(), targets_sorted.shape[0], queries.shape[0], qorder.numel(), item_key.numel(), queries.device
    if (targets_sorted.dim() != 2 or targets_sorted.shape[1] != 3 or queries.dim() != 2 or queries.shape[1] != 3 or tstart.numel() != nc + 1
            or tindex.numel() != nt or item_first.numel() != ni or item_count.numel() != ni):
        raise _lib.AdaMVSHipError("cloud_nearest: nc %d, nt %d, ni %d against targets %s, queries %s, tstart %d, tindex %d, item_first %d, "
                                  "item_count %d" % (nc, nt, ni, tuple(targets_sorted.shape), tuple(queries.shape), tstart.numel(),
                                                     tindex.numel(), item_first.numel(), item_count.numel()))
    keep, o, d = _lattice(origin, D)
    d2 = torch.full((nq,), float("inf"), device=dev, dtype=torch.float32)
    index = torch.full((nq,), -1, device=dev, dtype=torch.int32)
    pairs = torch.zeros(ni, device=dev, dtype=torch.int64)
    check(_lib.load().adamvs_cloud_nearest(o, d, _p(ukeys), _p(tstart), nc, _p(targets_sorted), _p(tindex), nt, _p(queries), nq, _p(qorder),
                                           nqs, _p(item_key), _p(item_first), _p(item_count), ni, _p(d2), _p(index), _p(pairs), _stream()),
          "cloud_nearest")
    return d2, index, pairs


def cloud_nearest_host(targets, queries, D, origin):
    """adamvs_cloud_nearest_host on numpy arrays: targets [nt, 3], queries [nq, 3] -> (d2 [nq] float32, index [nq] int32, pairs)."""
    t = np.ascontiguousarray(np.asarray(targets, np.float64).reshape(-1, 3))
    q = np.ascontiguousarray(np.asarray(queries, np.float64).reshape(-1, 3))
    keep, o, d = _lattice(origin, D)
    d2, index, pairs = np.zeros(len(q), np.float32), np.zeros(len(q), np.int32), ctypes.c_ulonglong(0)
    check(_lib.load().adamvs_cloud_nearest_host(o, d, t.ctypes.data, len(t), q.ctypes.data, len(q), d2.ctypes.data, index.ctypes.data,
                                                ctypes.addressof(pairs)), "cloud_nearest_host")
    return d2, index, int(pairs.value)


def cloud_sample_count(xyz, faces, spacing):
    """adamvs_cloud_sample_count.  xyz [nv, 3] float64, faces [nf, 3] int32 (uint32) -> subdiv [nf] int32 (n per face; 1025: too fine)."""
    xyz, faces = _dev_as(xyz, "xyz", torch.float64), _dev_as(faces, "faces", torch.int32)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.AdaMVSHipError("xyz [nv, 3], faces [nf, 3]: got %s, %s" % (tuple(xyz.shape), tuple(faces.shape)))
    subdiv = torch.empty(faces.shape[0], device=xyz.device, dtype=torch.int32)
    check(_lib.load().adamvs_cloud_sample_count(_p(xyz), xyz.shape[0], _p(faces), faces.shape[0], float(spacing), _p(subdiv), _stream()),
          "cloud_sample_count")
    return subdiv


def cloud_sample_emit(xyz, faces, subdiv, offsets, total):
    """adamvs_cloud_sample_emit.  offsets [nf + 1] int64 (exclusive sum of the samples per face), total = offsets[nf] -> points
    [total, 3] float64."""
    xyz, faces = _dev_as(xyz, "xyz", torch.float64), _dev_as(faces, "faces", torch.int32)
    subdiv, offsets = _dev_as(subdiv, "subdiv", torch.int32), _dev_as(offsets, "offsets", torch.int64)
    nf = faces.shape[0]
    if subdiv.numel() != nf or offsets.numel() != nf + 1:
        raise _lib.AdaMVSHipError("cloud_sample_emit: nf %d against subdiv %d, offsets %d" % (nf, subdiv.numel(), offsets.numel()))
    points = torch.empty(max(int(total), 1), 3, device=xyz.device, dtype=torch.float64)
    check(_lib.load().adamvs_cloud_sample_emit(_p(xyz), xyz.shape[0], _p(faces), nf, _p(subdiv), _p(offsets), _p(points), int(total),
                                               _stream()), "cloud_sample_emit")
    return points[:int(total)]


# ---- cloud neighbourhoods (csrc/cloud_knn.hip; driven by ada_mvs_amd/cloud_filter.py) ------------------------------------------
# keys int64, point numbers int32, d2 float32, index and count int32, pair counts int64 = uint64, normals float64, flags uint8.
def _knn_k(k):
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= _lib.KNN_MAX_K:
        raise _lib.AdaMVSHipError("k=%r: an integer 1 .. %d" % (k, _lib.KNN_MAX_K))
    return k


def knn_search(origin, R, k, ukeys, tstart, points_sorted, pindex, item_key, item_first, item_count, row_base, rows):
    """adamvs_knn_search on the work items given (a contiguous range of them).  ukeys [nc] / tstart [nc + 1] int64, points_sorted
    [n, 3] float64 with pindex [n] int32 (their numbers in the caller's order), the items (item_key, item_first int64, item_count
    int32) covering the sorted positions row_base .. row_base + rows -> (d2 [rows, k] float32, +inf padded; index [rows, k] int32,
    -1 padded; count [rows] int32; pairs [ni] int64), rows in sorted order."""
    k = _knn_k(k)
    ukeys, tstart = _dev_as(ukeys, "ukeys", torch.int64), _dev_as(tstart, "tstart", torch.int64)
    points_sorted, pindex = _dev_as(points_sorted, "points_sorted", torch.float64), _dev_as(pindex, "pindex", torch.int32)
    item_key, item_first = _dev_as(item_key, "item_key", torch.int64), _dev_as(item_first, "item_first", torch.int64)
    item_count = _dev_as(item_count, "item_count", torch.int32)
    nc, n, ni, dev = ukeys.numel(), points_sorted.shape[0], item_key.numel(), points_sorted.device
    row_base, rows = int(row_base), int(rows)
    if (points_sorted.dim() != 2 or points_sorted.shape[1] != 3 or tstart.numel() != nc + 1 or pindex.numel() != n or item_first.numel() != ni
            or item_count.numel() != ni or not (0 <= row_base and 1 <= rows and row_base + rows <= n)):
        raise _lib.AdaMVSHipError("knn_search: nc %d, n %d, ni %d, rows %d from %d against points %s, tstart %d, pindex %d, item_first %d, "
                                  "item_count %d" % (nc, n, ni, rows, row_base, tuple(points_sorted.shape), tstart.numel(), pindex.numel(),
                                                     item_first.numel(), item_count.numel()))
    keep, o, r = _lattice(origin, R)
    d2 = torch.full((rows, k), float("inf"), device=dev, dtype=torch.float32)
    index = torch.full((rows, k), -1, device=dev, dtype=torch.int32)
    count = torch.zeros(rows, device=dev, dtype=torch.int32)
    pairs = torch.zeros(ni, device=dev, dtype=torch.int64)
    check(_lib.load().adamvs_knn_search(o, r, k, _p(ukeys), _p(tstart), nc, _p(points_sorted), _p(pindex), n, _p(item_key), _p(item_first),
                                        _p(item_count), ni, row_base, rows, _p(d2), _p(index), _p(count), _p(pairs), _stream()),
          "knn_search")
    return d2, index, count, pairs


def knn_search_host(points, R, k, origin):
    """adamvs_knn_search_host on a numpy cloud [n, 3] -> (d2 [n, k] float32, index [n, k] int32, count [n] int32, pairs)."""
    k = _knn_k(k)
    pts = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    keep, o, r = _lattice(origin, R)
    n = len(pts)
    d2, index, count = np.zeros((n, k), np.float32), np.zeros((n, k), np.int32), np.zeros(n, np.int32)
    pairs = ctypes.c_ulonglong(0)
    check(_lib.load().adamvs_knn_search_host(o, r, k, pts.ctypes.data, n, d2.ctypes.data, index.ctypes.data, count.ctypes.data,
                                             ctypes.addressof(pairs)), "knn_search_host")
    return d2, index, count, int(pairs.value)


def knn_normals(points, index, count, row_point=None):
    """adamvs_knn_normals.  points [n, 3] float64, index [rows, k] int32, count [rows] int32 of knn_search, row_point [rows] int32 (the
    number of each row's point; None: row r is point r) -> (normal [rows, 3] float64, curvature [rows] float32, flag [rows] uint8)."""
    points, index, count = _dev_as(points, "points", torch.float64), _dev_as(index, "index", torch.int32), _dev_as(count, "count", torch.int32)
    if points.dim() != 2 or points.shape[1] != 3 or index.dim() != 2 or count.numel() != index.shape[0]:
        raise _lib.AdaMVSHipError("knn_normals: points %s, index %s, count %d" % (tuple(points.shape), tuple(index.shape), count.numel()))
    rows, k = int(index.shape[0]), _knn_k(int(index.shape[1]))
    if row_point is not None:
        row_point = _dev_as(row_point, "row_point", torch.int32)
        if row_point.numel() != rows:
            raise _lib.AdaMVSHipError("knn_normals: row_point %d against rows %d" % (row_point.numel(), rows))
    normal = torch.empty(rows, 3, device=points.device, dtype=torch.float64)
    curvature = torch.empty(rows, device=points.device, dtype=torch.float32)
    flag = torch.empty(rows, device=points.device, dtype=torch.uint8)
    check(_lib.load().adamvs_knn_normals(_p(points), points.shape[0], _p(index), _p(count), k, rows, _p(row_point) if row_point is not None else None,
                                         _p(normal), _p(curvature), _p(flag), _stream()), "knn_normals")
    return normal, curvature, flag


def knn_normals_host(points, index, count, row_point=None):
    """adamvs_knn_normals_host on numpy arrays -> (normal [rows, 3] float64, curvature [rows] float32, flag [rows] uint8)."""
    pts = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    index = np.ascontiguousarray(np.asarray(index, np.int32))
    count = np.ascontiguousarray(np.asarray(count, np.int32).reshape(-1))
    if index.ndim != 2 or len(count) != len(index):
        raise _lib.AdaMVSHipError("knn_normals_host: index %s, count %d" % (index.shape, len(count)))
    rows, k = len(index), _knn_k(int(index.shape[1]))
    rp = None if row_point is None else np.ascontiguousarray(np.asarray(row_point, np.int32).reshape(-1))
    if rp is not None and len(rp) != rows:
        raise _lib.AdaMVSHipError("knn_normals_host: row_point %d against rows %d" % (len(rp), rows))
    normal, curvature, flag = np.zeros((rows, 3), np.float64), np.zeros(rows, np.float32), np.zeros(rows, np.uint8)
    check(_lib.load().adamvs_knn_normals_host(pts.ctypes.data, len(pts), index.ctypes.data, count.ctypes.data, k, rows,
                                              rp.ctypes.data if rp is not None else None, normal.ctypes.data, curvature.ctypes.data,
                                              flag.ctypes.data), "knn_normals_host")
    return normal, curvature, flag


# ---- cloud registration (csrc/cloud_register.hip; driven by ada_mvs_amd/register.py) --------------------------------------------
# points, normals, partial sums float64, index int32, flags uint8; R [3, 3], the pivot c and u = c + t are host doubles.
def _vec(v, size, name):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    if a.size != size:
        raise _lib.AdaMVSHipError("%s: %d doubles, got %d" % (name, size, a.size))
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _motion(R, c, t):
    """-> the arrays (kept alive by the caller) and the pointers of R, c and u = c + t."""
    c0 = np.asarray(c, np.float64).reshape(-1)
    t0 = np.asarray(t, np.float64).reshape(-1)
    if c0.size != 3 or t0.size != 3:
        raise _lib.AdaMVSHipError("pivot and t: 3 doubles each, got %d and %d" % (c0.size, t0.size))
    (Ra, Rp), (ca, cp), (ua, up) = _vec(R, 9, "R"), _vec(c0, 3, "pivot"), _vec(c0 + t0, 3, "u")
    return (Ra, ca, ua), Rp, cp, up


def _xyz64(t, name):
    t = _dev_as(t, name, torch.float64)
    if t.dim() != 2 or t.shape[1] != 3:
        raise _lib.AdaMVSHipError("%s: [n, 3] float64, got %s" % (name, tuple(t.shape)))
    return t


def rigid_apply(x, R, c, t):
    """adamvs_rigid_apply.  x [n, 3] float64 -> y [n, 3] float64 = R (x - c) + (c + t)."""
    x = _xyz64(x, "x")
    keep, Rp, cp, up = _motion(R, c, t)
    y = torch.empty_like(x)
    check(_lib.load().adamvs_rigid_apply(Rp, cp, up, _p(x), x.shape[0], _p(y), _stream()), "rigid_apply")
    return y


def rigid_apply_host(x, R, c, t):
    """adamvs_rigid_apply_host on a numpy cloud [n, 3] -> y [n, 3] float64."""
    x = np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1, 3))
    keep, Rp, cp, up = _motion(R, c, t)
    y = np.zeros_like(x)
    check(_lib.load().adamvs_rigid_apply_host(Rp, cp, up, x.ctypes.data, len(x), y.ctypes.data), "rigid_apply_host")
    return y


def icp_blocks(nq):
    """Workgroups (and rows of the partial sums) of adamvs_icp_accumulate for nq queries."""
    return (int(nq) + _lib.CLOUD_TILE - 1) // _lib.CLOUD_TILE


def icp_accumulate(y, index, targets, normals, flag, c, L, delta):
    """adamvs_icp_accumulate.  y [nq, 3] float64 (the moved queries), index [nq] int32 of cloud_nearest, targets / normals [nt, 3]
    float64 and flag [nt] uint8 in the caller's order, the pivot c, the length scale L, the Huber width delta (<= 0: off)
    -> partial [ceil(nq / 256), 32] float64."""
    y, index = _xyz64(y, "y"), _dev_as(index, "index", torch.int32)
    targets, normals, flag = _xyz64(targets, "targets"), _xyz64(normals, "normals"), _dev_as(flag, "flag", torch.uint8)
    nq, nt = y.shape[0], targets.shape[0]
    if index.numel() != nq or normals.shape[0] != nt or flag.numel() != nt:
        raise _lib.AdaMVSHipError("icp_accumulate: nq %d, nt %d against index %d, normals %d, flag %d"
                                  % (nq, nt, index.numel(), normals.shape[0], flag.numel()))
    ca, cp = _vec(c, 3, "pivot")
    partial = torch.empty(icp_blocks(nq), _lib.ICP_TERMS, device=y.device, dtype=torch.float64)
    check(_lib.load().adamvs_icp_accumulate(_p(y), _p(index), nq, _p(targets), _p(normals), _p(flag), nt, cp, float(L), float(delta),
                                            _p(partial), _stream()), "icp_accumulate")
    return partial


def icp_accumulate_host(y, index, targets, normals, flag, c, L, delta):
    """adamvs_icp_accumulate_host on numpy arrays -> partial [ceil(nq / 256), 32] float64."""
    y = np.ascontiguousarray(np.asarray(y, np.float64).reshape(-1, 3))
    index = np.ascontiguousarray(np.asarray(index, np.int32).reshape(-1))
    targets = np.ascontiguousarray(np.asarray(targets, np.float64).reshape(-1, 3))
    normals = np.ascontiguousarray(np.asarray(normals, np.float64).reshape(-1, 3))
    flag = np.ascontiguousarray(np.asarray(flag, np.uint8).reshape(-1))
    nq, nt = len(y), len(targets)
    if len(index) != nq or len(normals) != nt or len(flag) != nt:
        raise _lib.AdaMVSHipError("icp_accumulate_host: nq %d, nt %d against index %d, normals %d, flag %d"
                                  % (nq, nt, len(index), len(normals), len(flag)))
    ca, cp = _vec(c, 3, "pivot")
    partial = np.zeros((icp_blocks(nq), _lib.ICP_TERMS), np.float64)
    check(_lib.load().adamvs_icp_accumulate_host(y.ctypes.data, index.ctypes.data, nq, targets.ctypes.data, normals.ctypes.data,
                                                 flag.ctypes.data, nt, cp, float(L), float(delta), partial.ctypes.data),
          "icp_accumulate_host")
    return partial


def icp_reduce(partial):
    """adamvs_icp_reduce.  partial [nb, 32] float64 -> sums [32] float64."""
    partial = _dev_as(partial, "partial", torch.float64)
    if partial.dim() != 2 or partial.shape[1] != _lib.ICP_TERMS:
        raise _lib.AdaMVSHipError("partial: [nb, %d] float64, got %s" % (_lib.ICP_TERMS, tuple(partial.shape)))
    sums = torch.empty(_lib.ICP_TERMS, device=partial.device, dtype=torch.float64)
    check(_lib.load().adamvs_icp_reduce(_p(partial), partial.shape[0], _p(sums), _stream()), "icp_reduce")
    return sums


def icp_reduce_host(partial):
    """adamvs_icp_reduce_host on a numpy array [nb, 32] -> sums [32] float64."""
    partial = np.ascontiguousarray(np.asarray(partial, np.float64).reshape(-1, _lib.ICP_TERMS))
    sums = np.zeros(_lib.ICP_TERMS, np.float64)
    check(_lib.load().adamvs_icp_reduce_host(partial.ctypes.data, len(partial), sums.ctypes.data), "icp_reduce_host")
    return sums


# ---- mesh smoothing (csrc/mesh_smooth.hip; driven by ada_mvs_amd/smooth.py) ---------------------------------------------------
# positions are relative to the origin (p = xyz - O); faces int32 = uint32; flags uint8.
def _smooth_mesh(p, faces):
    p = _dev_as(p, "p", torch.float64)
    faces = _dev_as(faces, "faces", torch.int32)
    if p.dim() != 2 or p.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.AdaMVSHipError("p [nv, 3], faces [nf, 3]: got %s, %s" % (tuple(p.shape), tuple(faces.shape)))
    return p, faces


def _smooth_runs(vface, vstart, nv, nf):
    vface, vstart = _dev_as(vface, "vface", torch.int32), _dev_as(vstart, "vstart", torch.int64)
    if vface.numel() != 3 * nf or vstart.numel() != nv + 1:
        raise _lib.AdaMVSHipError("nv %d, nf %d against vface %d, vstart %d" % (nv, nf, vface.numel(), vstart.numel()))
    return vface, vstart


def smooth_faces(p, faces):
    """adamvs_smooth_faces.  p [nv, 3] float64, faces [nf, 3] int32 (uint32) -> rec [nf, 8] float64: centroid, area, normal, 0."""
    p, faces = _smooth_mesh(p, faces)
    rec = torch.empty(faces.shape[0], 8, device=p.device, dtype=torch.float64)
    check(_lib.load().adamvs_smooth_faces(_p(p), p.shape[0], _p(faces), faces.shape[0], _p(rec), _stream()), "smooth_faces")
    return rec


def _edge_keys(what, faces):
    """adamvs_<what> (smooth_edge_keys or texture_edge_keys: one kernel behind both) -> keys int64 [3 nf], entry 3 f + k: edge k of
    face f as min << 32 | max."""
    keys = torch.empty(3 * faces.shape[0], device=faces.device, dtype=torch.int64)
    check(getattr(_lib.load(), "adamvs_" + what)(_p(faces), faces.shape[0], _p(keys), _stream()), what)
    return keys


def smooth_boundary(faces, nv):
    """adamvs_smooth_edge_keys, a sort of the keys, adamvs_smooth_boundary -> fixed [nv] uint8: the ends of every edge that occurs once."""
    faces = _dev_as(faces, "faces", torch.int32)
    fixed = torch.zeros(int(nv), device=faces.device, dtype=torch.uint8)
    keys = torch.sort(_edge_keys("smooth_edge_keys", faces), stable=True).values
    check(_lib.load().adamvs_smooth_boundary(_p(keys), keys.numel(), int(nv), _p(fixed), _stream()), "smooth_boundary")
    return fixed


def smooth_filter(rec, nin, faces, nv, vface, vstart, sigma_s, sigma_r, out=None):
    """adamvs_smooth_filter: one pass.  rec [nf, 8], nin [nf, 3] float64 -> nout [nf, 3] (`out`, a buffer other than nin, is reused)."""
    rec, nin = _dev_as(rec, "rec", torch.float64), _dev_as(nin, "nin", torch.float64)
    faces = _dev_as(faces, "faces", torch.int32)
    nf = faces.shape[0]
    vface, vstart = _smooth_runs(vface, vstart, int(nv), nf)
    if rec.numel() != 8 * nf or nin.numel() != 3 * nf:
        raise _lib.AdaMVSHipError("smooth_filter: nf %d against rec %d, nin %d" % (nf, rec.numel(), nin.numel()))
    nout = torch.empty_like(nin) if out is None else _dev_as(out, "out", torch.float64)
    if nout.numel() != 3 * nf or nout.data_ptr() == nin.data_ptr() or not nout.is_contiguous():
        raise _lib.AdaMVSHipError("smooth_filter: out must be a contiguous [nf, 3] buffer other than nin")
    check(_lib.load().adamvs_smooth_filter(_p(rec), _p(nin), _p(nout), _p(faces), nf, int(nv), _p(vface), _p(vstart), float(sigma_s),
                                           float(sigma_r), _stream()), "smooth_filter")
    return nout


def smooth_centroids(p, faces, out=None):
    """adamvs_smooth_centroids -> cen [nf, 3] float64 of the positions p."""
    p, faces = _smooth_mesh(p, faces)
    cen = torch.empty(faces.shape[0], 3, device=p.device, dtype=torch.float64) if out is None else _dev_as(out, "out", torch.float64)
    if cen.numel() != 3 * faces.shape[0]:
        raise _lib.AdaMVSHipError("smooth_centroids: out %d against nf %d" % (cen.numel(), faces.shape[0]))
    check(_lib.load().adamvs_smooth_centroids(_p(p), p.shape[0], _p(faces), faces.shape[0], _p(cen), _stream()), "smooth_centroids")
    return cen


def smooth_update(p0, p, normals, cen, vface, vstart, fixed, cap, out=None, clamped=None):
    """adamvs_smooth_update: one pass.  p0, p [nv, 3], normals, cen [nf, 3] float64, fixed [nv] uint8 -> (pout [nv, 3], clamped [nv] uint8)."""
    p0, p = _dev_as(p0, "p0", torch.float64), _dev_as(p, "p", torch.float64)
    normals, cen = _dev_as(normals, "normals", torch.float64), _dev_as(cen, "cen", torch.float64)
    fixed = _dev_as(fixed, "fixed", torch.uint8)
    nv, nf = p0.shape[0], normals.shape[0]
    vface, vstart = _smooth_runs(vface, vstart, nv, nf)
    if p.numel() != 3 * nv or p0.numel() != 3 * nv or cen.numel() != 3 * nf or normals.numel() != 3 * nf or fixed.numel() != nv:
        raise _lib.AdaMVSHipError("smooth_update: nv %d, nf %d against p %d, cen %d, fixed %d" % (nv, nf, p.numel(), cen.numel(), fixed.numel()))
    pout = torch.empty_like(p0) if out is None else _dev_as(out, "out", torch.float64)
    if pout.numel() != 3 * nv or pout.data_ptr() in (p.data_ptr(), p0.data_ptr()) or not pout.is_contiguous():
        raise _lib.AdaMVSHipError("smooth_update: out must be a contiguous [nv, 3] buffer other than p and p0")
    cl = torch.empty(nv, device=p0.device, dtype=torch.uint8) if clamped is None else _dev_as(clamped, "clamped", torch.uint8)
    if cl.numel() != nv:
        raise _lib.AdaMVSHipError("smooth_update: clamped %d against nv %d" % (cl.numel(), nv))
    check(_lib.load().adamvs_smooth_update(_p(p0), _p(p), _p(pout), nv, _p(normals), _p(cen), nf, _p(vface), _p(vstart), _p(fixed),
                                           float(cap), _p(cl), _stream()), "smooth_update")
    return pout, cl


# ---- mesh cleaning (csrc/mesh_clean.hip; driven by ada_mvs_amd/clean.py) -----------------------------------------------------
# faces int32 = uint32 [ns, 3]; half-edge arrays have 3 ns entries; labels and successors int32, flags uint8.
def _clean_faces(faces, name="faces"):
    faces = _dev_as(faces, name, torch.int32)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise _lib.AdaMVSHipError("%s [ns >= 1, 3]: got %s" % (name, tuple(faces.shape)))
    return faces


def _clean_len(what, n, *named):
    """Every (name, tensor, dtype) is a contiguous device tensor of n elements -> the tensors."""
    out = []
    for name, t, dtype in named:
        t = _dev_as(t, name, dtype)
        if t.numel() != n:
            raise _lib.AdaMVSHipError("%s: %s has %d elements, not %d" % (what, name, t.numel(), n))
        out.append(t)
    return out


def clean_components_round(faces, parent_in, parent_out, changed):
    """adamvs_clean_components: one hook + compress round.  parent_in [nv] int32 -> parent_out [nv] (another buffer); changed [1]
    int32 is set to whether a hook happened."""
    faces = _clean_faces(faces)
    parent_in, parent_out = _clean_len("clean_components", parent_in.numel(), ("parent_in", parent_in, torch.int32),
                                       ("parent_out", parent_out, torch.int32))
    changed, = _clean_len("clean_components", 1, ("changed", changed, torch.int32))
    check(_lib.load().adamvs_clean_components(_p(faces), faces.shape[0], parent_in.numel(), _p(parent_in), _p(parent_out), _p(changed),
                                              _stream()), "clean_components")
    return parent_out


def clean_area(area, order, seg_of, seg_start):
    """adamvs_clean_area.  area [nf] float64; order [nf] int64: the faces sorted stably by label; seg_of [nf] int64: the rank of the
    component at each sorted position; seg_start [ncomp + 1] int64 -> the components' areas [ncomp] float64."""
    nf = area.numel()
    area, order, seg_of = _clean_len("clean_area", nf, ("area", area, torch.float64), ("order", order, torch.int64),
                                     ("seg_of", seg_of, torch.int64))
    seg_start = _dev_as(seg_start, "seg_start", torch.int64)
    ncomp = seg_start.numel() - 1
    lead = torch.zeros((nf + _lib.CLEAN_CHUNK - 1) // _lib.CLEAN_CHUNK, device=area.device, dtype=torch.float64)
    first = torch.zeros(max(ncomp, 1), device=area.device, dtype=torch.float64)
    out = torch.empty(max(ncomp, 1), device=area.device, dtype=torch.float64)
    check(_lib.load().adamvs_clean_area(_p(area), nf, _p(order), _p(seg_of), _p(seg_start), ncomp, _p(lead), _p(first), _p(out), _stream()),
          "clean_area")
    return out[:ncomp]


def clean_boundary(faces):
    """adamvs_smooth_edge_keys, a stable sort of the keys, adamvs_clean_boundary -> bnd [3 ns] uint8: the half-edges whose key occurs once."""
    faces = _clean_faces(faces)
    ns = faces.shape[0]
    bnd = torch.empty(3 * ns, device=faces.device, dtype=torch.uint8)
    es = torch.sort(_edge_keys("smooth_edge_keys", faces), stable=True)
    ks, entry = es.values.contiguous(), es.indices.contiguous()
    check(_lib.load().adamvs_clean_boundary(_p(ks), _p(entry), ns, _p(bnd), _stream()), "clean_boundary")
    return bnd


def clean_successor(faces, nv, bnd):
    """adamvs_clean_successor -> dict: out_count, in_count, out_edge [nv] int32; succ, lab, nxt [3 ns] int32; broken [3 ns] uint8."""
    faces = _clean_faces(faces)
    ns, nv, dev = faces.shape[0], int(nv), faces.device
    bnd, = _clean_len("clean_successor", 3 * ns, ("bnd", bnd, torch.uint8))
    r = dict(out_count=torch.empty(nv, device=dev, dtype=torch.int32), in_count=torch.empty(nv, device=dev, dtype=torch.int32),
             out_edge=torch.empty(nv, device=dev, dtype=torch.int32), succ=torch.empty(3 * ns, device=dev, dtype=torch.int32),
             lab=torch.empty(3 * ns, device=dev, dtype=torch.int32), nxt=torch.empty(3 * ns, device=dev, dtype=torch.int32),
             broken=torch.empty(3 * ns, device=dev, dtype=torch.uint8))
    check(_lib.load().adamvs_clean_successor(_p(faces), ns, nv, _p(bnd), _p(r["out_count"]), _p(r["in_count"]), _p(r["out_edge"]), _p(r["succ"]),
                                             _p(r["lab"]), _p(r["nxt"]), _p(r["broken"]), _stream()), "clean_successor")
    return r


def clean_double(bnd, state_in, state_out):
    """adamvs_clean_double: one doubling round.  state_* = (lab int32, nxt int32, broken uint8), each [3 ns]; both states were
    initialised from clean_successor's output.  -> state_out."""
    n = bnd.numel()
    if n % 3 or n < 3:
        raise _lib.AdaMVSHipError("clean_double: %d half-edges is no multiple of 3" % n)
    bnd, = _clean_len("clean_double", n, ("bnd", bnd, torch.uint8))
    names = (("lab", torch.int32), ("nxt", torch.int32), ("broken", torch.uint8))
    a = _clean_len("clean_double", n, *[(k + "_in", t, d) for (k, d), t in zip(names, state_in)])
    b = _clean_len("clean_double", n, *[(k + "_out", t, d) for (k, d), t in zip(names, state_out)])
    check(_lib.load().adamvs_clean_double(_p(bnd), n // 3, _p(a[0]), _p(a[1]), _p(a[2]), _p(b[0]), _p(b[1]), _p(b[2]), _stream()), "clean_double")
    return tuple(b)


def clean_validate(bnd, succ, lab, broken, max_hole_edges):
    """adamvs_clean_validate -> (count [3 ns] int32: the size of each label group at its label, bad [3 ns] uint8, loop [3 ns] int32:
    the label of each half-edge's loop or -1, closed [3 ns] uint8)."""
    n = bnd.numel()
    if n % 3 or n < 3:
        raise _lib.AdaMVSHipError("clean_validate: %d half-edges is no multiple of 3" % n)
    bnd, succ, lab, broken = _clean_len("clean_validate", n, ("bnd", bnd, torch.uint8), ("succ", succ, torch.int32), ("lab", lab, torch.int32),
                                        ("broken", broken, torch.uint8))
    dev = bnd.device
    count, bad = torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.uint8)
    loop, closed = torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.uint8)
    check(_lib.load().adamvs_clean_validate(_p(bnd), _p(succ), _p(lab), _p(broken), n // 3, int(max_hole_edges), _p(count), _p(bad), _p(loop),
                                            _p(closed), _stream()), "clean_validate")
    return count, bad, loop, closed


def clean_accumulate(p, rgb, faces, members, start, origin):
    """adamvs_clean_accumulate.  p [nv, 3] float64 (relative to origin), rgb [nv, 3] uint8, members [nm] int32 (the closed half-edges
    by loop, ascending within a loop), start [nl + 1] int64 -> (centre [nl, 3] float64 world, colour [nl, 3] uint8)."""
    p, faces = _smooth_mesh(p, _clean_faces(faces))
    rgb = _dev_as(rgb, "rgb", torch.uint8)
    members, start = _dev_as(members, "members", torch.int32), _dev_as(start, "start", torch.int64)
    if tuple(rgb.shape) != tuple(p.shape) or start.numel() < 2:
        raise _lib.AdaMVSHipError("clean_accumulate: p %s, rgb %s, start %d" % (tuple(p.shape), tuple(rgb.shape), start.numel()))
    nl = start.numel() - 1
    keep, o, _ = _lattice(origin, 1.0)
    centre = torch.empty(nl, 3, device=p.device, dtype=torch.float64)
    colour = torch.empty(nl, 3, device=p.device, dtype=torch.uint8)
    check(_lib.load().adamvs_clean_accumulate(_p(p), _p(rgb), p.shape[0], _p(faces), faces.shape[0], _p(members), members.numel(), _p(start), nl,
                                              o, _p(centre), _p(colour), _stream()), "clean_accumulate")
    return centre, colour


def clean_emit(xyz, rgb, new_index, nvs, faces, fill_edge=None, loop_of=None, centre=None, colour=None):
    """adamvs_clean_emit.  xyz [nv, 3] float64, rgb [nv, 3] uint8, new_index [nv] int32 (-1: unused; nvs used), faces [ns, 3] and,
    where loops are closed, fill_edge, loop_of [nfill] int32, centre [nl, 3] float64, colour [nl, 3] uint8
    -> (xyz [nvs + nl, 3], rgb [nvs + nl, 3], faces [ns + nfill, 3] int32)."""
    xyz, faces = _smooth_mesh(xyz, _clean_faces(faces))
    rgb = _dev_as(rgb, "rgb", torch.uint8)
    nv, ns, dev = xyz.shape[0], faces.shape[0], xyz.device
    new_index, = _clean_len("clean_emit", nv, ("new_index", new_index, torch.int32))
    if tuple(rgb.shape) != tuple(xyz.shape):
        raise _lib.AdaMVSHipError("clean_emit: xyz %s, rgb %s" % (tuple(xyz.shape), tuple(rgb.shape)))
    nfill = 0 if fill_edge is None else fill_edge.numel()
    nl = 0 if centre is None else centre.shape[0]
    null = ctypes.c_void_p(0)
    fe = lo = ce = co = null
    if nfill or nl:
        fill_edge, loop_of = _clean_len("clean_emit", nfill, ("fill_edge", fill_edge, torch.int32), ("loop_of", loop_of, torch.int32))
        centre, = _clean_len("clean_emit", 3 * nl, ("centre", centre, torch.float64))
        colour, = _clean_len("clean_emit", 3 * nl, ("colour", colour, torch.uint8))
        fe, lo, ce, co = _p(fill_edge), _p(loop_of), _p(centre), _p(colour)
    nvs = int(nvs)
    xyz_out = torch.empty(max(nvs, 0) + nl, 3, device=dev, dtype=torch.float64)
    rgb_out = torch.empty(max(nvs, 0) + nl, 3, device=dev, dtype=torch.uint8)
    faces_out = torch.empty(ns + nfill, 3, device=dev, dtype=torch.int32)
    check(_lib.load().adamvs_clean_emit(_p(xyz), _p(rgb), nv, _p(new_index), _p(faces), ns, fe, lo, nfill, ce, co, nl, nvs, _p(xyz_out),
                                        _p(rgb_out), _p(faces_out), _stream()), "clean_emit")
    return xyz_out, rgb_out, faces_out


# ---- image orthophoto (csrc/ortho.hip; driven view by view by ada_mvs_amd/ortho.py) ------------------------------------------
# The depth buffer is int32 holding uint32 float bits; acc is float32 [N, 4]; view and nvis int32; nvis_out int16 (uint16).
def ortho_grid(x0, y_top, gsd, W, H, K):
    """-> _lib.OrthoGrid (adamvs_ortho_grid)."""
    g = _lib.OrthoGrid()
    g.x0, g.y_top, g.gsd, g.W, g.H, g.K = float(x0), float(y_top), float(gsd), int(W), int(H), int(K)
    return g


def ortho_view(K, R_cw, C, rgba):
    """K [3, 3], R_cw [3, 3] (rounded here to fp32), C [3] fp64, rgba device [H, W, 4] uint8 -> _lib.OrthoView.  The image
    tensor must outlive it."""
    rgba = _dev_as(rgba, "rgba", torch.uint8)
    if rgba.dim() != 3 or rgba.shape[2] != 4:
        raise _lib.AdaMVSHipError("rgba must be [H, W, 4], got %s" % (tuple(rgba.shape),))
    v = _lib.OrthoView()
    v.C[:] = [float(c) for c in np.asarray(C, np.float64).reshape(-1)]
    v.R[:] = [float(r) for r in np.asarray(R_cw, np.float64).reshape(-1)]
    v.K[:] = [float(k) for k in np.asarray(K, np.float64).reshape(-1)]
    v.H, v.W = int(rgba.shape[0]), int(rgba.shape[1])
    v.rgba = rgba.data_ptr()
    return v


def ortho_surface(grid, dsm):
    """adamvs_ortho_surface: dsm device [H, W] float32 -> height [H K, W K] float64 (NaN: no surface)."""
    dsm = _dev(dsm, "dsm")
    if tuple(dsm.shape) != (grid.H, grid.W):
        raise _lib.AdaMVSHipError("dsm %s, grid %d x %d" % (tuple(dsm.shape), grid.H, grid.W))
    height = torch.empty(grid.H * grid.K, grid.W * grid.K, device=dsm.device, dtype=torch.float64)
    check(_lib.load().adamvs_ortho_surface(ctypes.byref(grid), _p(dsm), _p(height), _stream()), "ortho_surface")
    return height


def ortho_zbuf(grid, dsm, view, zbuf, big):
    """adamvs_ortho_zbuf into zbuf (device int32 [H_img, W_img], uint32 float bits); big: device int32 [1 + 2 (W-1)(H-1)]
    (the large-triangle counter, then the list)."""
    dsm = _dev(dsm, "dsm")
    zbuf = _dev_as(zbuf, "zbuf", torch.int32)
    big = _dev_as(big, "big", torch.int32)
    if tuple(zbuf.shape) != (view.H, view.W):
        raise _lib.AdaMVSHipError("zbuf %s, image %d x %d" % (tuple(zbuf.shape), view.H, view.W))
    if tuple(dsm.shape) != (grid.H, grid.W) or big.numel() < 1:
        raise _lib.AdaMVSHipError("dsm %s, grid %d x %d, big %d" % (tuple(dsm.shape), grid.H, grid.W, big.numel()))
    check(_lib.load().adamvs_ortho_zbuf(ctypes.byref(grid), _p(dsm), ctypes.byref(view), _p(zbuf), _p(big),
                                        ctypes.c_void_p(big.data_ptr() + 4), big.numel() - 1, _stream()), "ortho_zbuf")


def ortho_compose(grid, view, view_id, height, zbuf, mode, border, feather_px, occlusion_tol, acc, wmax, vstate, nvis):
    """adamvs_ortho_compose: one view into the cell state (acc float32 [N, 4], wmax float32 [N], vstate int32 [N], nvis int32 [N])."""
    height = _dev_as(height, "height", torch.float64)
    zbuf = _dev_as(zbuf, "zbuf", torch.int32)
    n = grid.W * grid.K * grid.H * grid.K
    tensors = (_dev(acc, "acc"), _dev(wmax, "wmax"), _dev_as(vstate, "view", torch.int32), _dev_as(nvis, "nvis", torch.int32))
    if height.numel() != n or tensors[0].numel() != 4 * n or any(t.numel() != n for t in tensors[1:]) or zbuf.numel() != view.H * view.W:
        raise _lib.AdaMVSHipError("ortho_compose: state sizes do not match %d cells" % n)
    if any(not t.is_contiguous() for t in (acc, wmax, vstate, nvis)):
        raise _lib.AdaMVSHipError("ortho_compose: the state must be contiguous (it is updated in place)")
    check(_lib.load().adamvs_ortho_compose(ctypes.byref(grid), ctypes.byref(view), int(view_id), _p(height), _p(zbuf), int(mode),
                                           float(border), float(feather_px), float(occlusion_tol), *(_p(t) for t in tensors), _stream()),
          "ortho_compose")


def ortho_finalize(grid, acc, vstate, nvis):
    """adamvs_ortho_finalize -> (rgba [H_o, W_o, 4] uint8, view int32 [H_o, W_o], nvis int16 (uint16) [H_o, W_o])."""
    Ho, Wo = grid.H * grid.K, grid.W * grid.K
    acc, vstate, nvis = _dev(acc, "acc"), _dev_as(vstate, "view", torch.int32), _dev_as(nvis, "nvis", torch.int32)
    if acc.numel() != 4 * Ho * Wo or vstate.numel() != Ho * Wo or nvis.numel() != Ho * Wo:
        raise _lib.AdaMVSHipError("ortho_finalize: state sizes do not match %d cells" % (Ho * Wo))
    dev = acc.device
    rgba = torch.empty(Ho, Wo, 4, device=dev, dtype=torch.uint8)
    view_out = torch.empty(Ho, Wo, device=dev, dtype=torch.int32)
    nvis_out = torch.empty(Ho, Wo, device=dev, dtype=torch.int16)
    check(_lib.load().adamvs_ortho_finalize(ctypes.byref(grid), _p(acc), _p(vstate), _p(nvis), _p(rgba), _p(view_out), _p(nvis_out),
                                            _stream()), "ortho_finalize")
    return rgba, view_out, nvis_out


# ---- image orthophoto, radiometric balance (csrc/ortho_balance.hip; driven by ada_mvs_amd/ortho.py) --------------------------
# obs is int16 holding uint16 (q_r, q_g, q_b, flag) per lattice cell; the statistics are int64.
def ortho_lattice(grid, S):
    """(W_s, H_s) of the observation lattice of stride S over the DSM grid; raises unless S >= 1 and N_s is within the cap."""
    if isinstance(S, bool) or int(S) != S or int(S) < 1:
        raise _lib.AdaMVSHipError("balance stride %r: an integer >= 1" % (S,))
    S = int(S)
    Ws, Hs = -(-int(grid.W) // S), -(-int(grid.H) // S)
    if Ws * Hs > _lib.ORTHO_BAL_MAX_SAMPLES:
        raise _lib.AdaMVSHipError("balance stride %d: %d x %d lattice cells exceed the cap of %d" % (S, Ws, Hs, _lib.ORTHO_BAL_MAX_SAMPLES))
    return Ws, Hs


def ortho_observe(grid, dsm, view, zbuf, S, border, occlusion_tol, obs):
    """adamvs_ortho_observe: the view's samples on the lattice of stride S into obs (device int16 [N_s, 4], one plane)."""
    dsm = _dev(dsm, "dsm")
    zbuf = _dev_as(zbuf, "zbuf", torch.int32)
    Ws, Hs = ortho_lattice(grid, S)
    if tuple(dsm.shape) != (grid.H, grid.W) or zbuf.numel() != view.H * view.W:
        raise _lib.AdaMVSHipError("ortho_observe: dsm %s, grid %d x %d, zbuf %d, image %d x %d"
                                  % (tuple(dsm.shape), grid.H, grid.W, zbuf.numel(), view.H, view.W))
    if (not isinstance(obs, torch.Tensor) or not obs.is_cuda or obs.dtype != torch.int16 or not obs.is_contiguous()
            or tuple(obs.shape) != (Ws * Hs, 4)):
        raise _lib.AdaMVSHipError("ortho_observe: obs must be a contiguous GPU int16 [%d, 4] (it is written in place)" % (Ws * Hs))
    check(_lib.load().adamvs_ortho_observe(ctypes.byref(grid), _p(dsm), ctypes.byref(view), _p(zbuf), int(S), float(border),
                                           float(occlusion_tol), _p(obs), _stream()), "ortho_observe")


class OrthoPairs:
    """Pairs of views checked on the host (0 <= a < b < V) and uploaded: .host int32 [P, 2], .dev the same on the device."""

    def __init__(self, pairs, V, device):
        host = pairs.cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
        host = host.reshape(-1, 2) if host.size == 0 else host
        if host.ndim != 2 or host.shape[1] != 2 or (host.size and not np.issubdtype(host.dtype, np.integer)):
            raise _lib.AdaMVSHipError("ortho_pair_stats: pairs must be an integer [P, 2], got %s %s" % (host.dtype, host.shape))
        host = host.astype(np.int64)
        bad = (host[:, 0] < 0) | (host[:, 0] >= host[:, 1]) | (host[:, 1] >= V)
        if bad.any():
            raise _lib.AdaMVSHipError("ortho_pair_stats: pair %s is not 0 <= a < b < V = %d" % (tuple(host[np.nonzero(bad)[0][0]]), V))
        self.V, self.host = int(V), np.ascontiguousarray(host, np.int32)
        self.dev = torch.from_numpy(self.host).to(device)


def ortho_pair_stats(obs, pairs, max_diff_q):
    """adamvs_ortho_pair_stats: obs device int16 [V, N_s, 4]; pairs [P, 2] (any integer array, or an OrthoPairs made for V views:
    0 <= a < b < V is checked on the host, the kernel does not check it) -> stats device int64 [P, 7] = (n, Sa_0..2, Sb_0..2)."""
    obs = _dev_as(obs, "obs", torch.int16)
    if obs.dim() != 3 or obs.shape[2] != 4 or obs.shape[0] < 1 or obs.shape[1] < 1:
        raise _lib.AdaMVSHipError("ortho_pair_stats: obs must be [V, N_s, 4], got %s" % (tuple(obs.shape),))
    V, Ns = int(obs.shape[0]), int(obs.shape[1])
    if not isinstance(pairs, OrthoPairs):
        pairs = OrthoPairs(pairs, V, obs.device)
    if pairs.V != V or pairs.dev.device != obs.device:
        raise _lib.AdaMVSHipError("ortho_pair_stats: the pairs were checked for %d views on %s, obs has %d on %s"
                                  % (pairs.V, pairs.dev.device, V, obs.device))
    P = int(pairs.host.shape[0])
    stats = torch.empty(P, 7, device=obs.device, dtype=torch.int64)
    check(_lib.load().adamvs_ortho_pair_stats(_p(obs), V, Ns, _p(pairs.dev), P, int(max_diff_q), _p(stats), _stream()), "ortho_pair_stats")
    return stats


def ortho_adjust_image(rgba, gain, out=None):
    """adamvs_ortho_adjust_image: rgba device [H, W, 4] uint8, gain [3] (host) -> the adjusted image (into `out` if given)."""
    rgba = _dev_as(rgba, "rgba", torch.uint8)
    if rgba.dim() != 3 or rgba.shape[2] != 4:
        raise _lib.AdaMVSHipError("rgba must be [H, W, 4], got %s" % (tuple(rgba.shape),))
    if out is None:
        out = torch.empty_like(rgba)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous()
          or out.shape != rgba.shape or out.data_ptr() == rgba.data_ptr()):
        raise _lib.AdaMVSHipError("ortho_adjust_image: out must be another contiguous GPU uint8 tensor of the image's shape")
    g = (ctypes.c_float * 3)(*[float(x) for x in np.asarray(gain, np.float64).reshape(3)])
    check(_lib.load().adamvs_ortho_adjust_image(_p(rgba), int(rgba.shape[0]), int(rgba.shape[1]), g, _p(out), _stream()),
          "ortho_adjust_image")
    return out


def ortho_seam_stats(grid, view_out, rgba):
    """adamvs_ortho_seam_stats over the mosaic of ortho_finalize -> stats device int64 [4] = (pairs, sum d_r^2, d_g^2, d_b^2)."""
    view_out, rgba = _dev_as(view_out, "view", torch.int32), _dev_as(rgba, "rgba", torch.uint8)
    n = grid.H * grid.K * grid.W * grid.K
    if view_out.numel() != n or rgba.numel() != 4 * n:
        raise _lib.AdaMVSHipError("ortho_seam_stats: sizes do not match %d cells" % n)
    stats = torch.empty(4, device=rgba.device, dtype=torch.int64)
    check(_lib.load().adamvs_ortho_seam_stats(ctypes.byref(grid), _p(view_out), _p(rgba), _p(stats), _stream()), "ortho_seam_stats")
    return stats


# ---- mesh texturing (csrc/texture.hip; driven by ada_mvs_amd/texture.py) ------------------------------------------------------
# Views are _lib.OrthoView (ortho_view above).  faces: device int32 [nf, 3] holding uint32 indices; the depth buffer is int32
# holding uint32 float bits; every per-face state tensor is updated in place and must be contiguous.
def _tex_sizes(xyz_or_nv, faces):
    nv = xyz_or_nv if isinstance(xyz_or_nv, int) else xyz_or_nv.shape[0]
    return int(nv), int(faces.shape[0])


def texture_project(view, xyz, uvz=None):
    """adamvs_texture_project: xyz device float64 [nv, 3] -> uvz float32 [nv, 4] (u, v, z, 0)."""
    xyz = _dev_as(xyz, "xyz", torch.float64)
    if uvz is None:
        uvz = torch.empty(xyz.shape[0], 4, device=xyz.device, dtype=torch.float32)
    check(_lib.load().adamvs_texture_project(ctypes.byref(view), _p(xyz), xyz.shape[0], _p(uvz), _stream()), "texture_project")
    return uvz


def texture_zbuf(view, uvz, faces, zbuf, big):
    """adamvs_texture_zbuf into zbuf (int32 [H, W]); big: int32 [1 + nf] (the large-face counter, then the list)."""
    uvz, faces = _dev(uvz, "uvz"), _dev_as(faces, "faces", torch.int32)
    zbuf, big = _dev_as(zbuf, "zbuf", torch.int32), _dev_as(big, "big", torch.int32)
    if tuple(zbuf.shape) != (view.H, view.W) or big.numel() < 1:
        raise _lib.AdaMVSHipError("zbuf %s, image %d x %d, big %d" % (tuple(zbuf.shape), view.H, view.W, big.numel()))
    nv, nf = _tex_sizes(uvz, faces)
    check(_lib.load().adamvs_texture_zbuf(ctypes.byref(view), _p(uvz), nv, _p(faces), nf, _p(zbuf), _p(big),
                                          ctypes.c_void_p(big.data_ptr() + 4), big.numel() - 1, _stream()), "texture_zbuf")


def texture_score(view, view_index, uvz, faces, zbuf, border, tol, best, label, nvis, uv):
    """adamvs_texture_score: one view into the face state (best float32 [nf], label int32 [nf], nvis int32 [nf], uv float32 [nf, 6])."""
    uvz, faces, zbuf = _dev(uvz, "uvz"), _dev_as(faces, "faces", torch.int32), _dev_as(zbuf, "zbuf", torch.int32)
    nv, nf = _tex_sizes(uvz, faces)
    state = (best, label, nvis, uv)
    if any(not (t.is_cuda and t.is_contiguous()) for t in state) or uv.numel() != 6 * nf or any(t.numel() != nf for t in state[:3]):
        raise _lib.AdaMVSHipError("texture_score: the face state must be contiguous device tensors of %d faces" % nf)
    check(_lib.load().adamvs_texture_score(ctypes.byref(view), int(view_index), _p(uvz), nv, _p(faces), nf, _p(zbuf), float(border), float(tol),
                                           *(_p(t) for t in state), _stream()), "texture_score")


def texture_edge_keys(faces):
    """adamvs_texture_edge_keys -> keys int64 [3 nf] (entry 3 f + k: edge k of face f as min << 32 | max)."""
    return _edge_keys("texture_edge_keys", _dev_as(faces, "faces", torch.int32))


def texture_components_round(keys_sorted, entry, label, parent, changed):
    """adamvs_texture_components: one hook + compress round over the sorted edge entries (parent int32 [nf] in place; changed
    int32 [1], cleared and set by the call)."""
    keys_sorted, entry = _dev_as(keys_sorted, "keys", torch.int64), _dev_as(entry, "entry", torch.int64)
    label = _dev_as(label, "label", torch.int32)
    if not (parent.is_cuda and parent.is_contiguous() and parent.dtype == torch.int32) or keys_sorted.numel() != 3 * parent.numel():
        raise _lib.AdaMVSHipError("texture_components: parent must be contiguous int32 [nf] with 3 nf sorted entries")
    check(_lib.load().adamvs_texture_components(_p(keys_sorted), _p(entry), parent.numel(), _p(label), _p(parent), _p(changed), _stream()),
          "texture_components")


def texture_rank(label, parent):
    """adamvs_texture_rank -> (root_chart int32 [nf], pal int32 [nf], charts, untextured) (the two counts are read back)."""
    label, parent = _dev_as(label, "label", torch.int32), _dev_as(parent, "parent", torch.int32)
    nf = label.numel()
    nb = max(1, (nf + _lib.TEXTURE_TILE - 1) // _lib.TEXTURE_TILE)
    ws = torch.empty(4 * nb + 2, device=label.device, dtype=torch.int32)
    root_chart, pal = torch.empty_like(label), torch.empty_like(label)
    blk_r, blk_u, off_r, off_u = ws[:nb], ws[nb:2 * nb], ws[2 * nb:3 * nb + 1], ws[3 * nb + 1:]
    check(_lib.load().adamvs_texture_rank(_p(label), _p(parent), nf, _p(blk_r), _p(blk_u), _p(off_r), _p(off_u), _p(root_chart), _p(pal),
                                          _stream()), "texture_rank")
    if nf == 0:
        return root_chart, pal, 0, 0
    tot = torch.stack((off_r[nb], off_u[nb])).cpu()
    return root_chart, pal, int(tot[0]), int(tot[1])


def texture_boxes(label, parent, root_chart, uv, n_charts):
    """adamvs_texture_boxes -> (chart int32 [nf], box int32 [n_charts, 4] = min floor u, min floor v, max floor u, max floor v)."""
    label, parent, root_chart, uv = (_dev_as(label, "label", torch.int32), _dev_as(parent, "parent", torch.int32),
                                     _dev_as(root_chart, "root_chart", torch.int32), _dev(uv, "uv"))
    chart = torch.empty_like(label)
    box = torch.empty(max(n_charts, 1), 4, device=label.device, dtype=torch.int32)
    box[:, :2] = 2 ** 31 - 1
    box[:, 2:] = -2 ** 31
    check(_lib.load().adamvs_texture_boxes(_p(label), _p(parent), _p(root_chart), _p(uv), label.numel(), _p(chart), _p(box), _stream()),
          "texture_boxes")
    return chart, box[:n_charts]


def texture_fill(view, items, prefix, texels, P, atlas):
    """adamvs_texture_fill: items int32 [n, 8] (x0, y0, w, h, ox, oy, page, view), prefix int64 [n + 1], atlas uint8 [pages, P, P, 4]."""
    items, prefix = _dev_as(items, "items", torch.int32), _dev_as(prefix, "prefix", torch.int64)
    atlas = _dev_as(atlas, "atlas", torch.uint8)
    if tuple(atlas.shape[1:]) != (P, P, 4) or prefix.numel() != items.shape[0] + 1:
        raise _lib.AdaMVSHipError("texture_fill: atlas %s for page %d, %d items, %d prefix" % (tuple(atlas.shape), P, items.shape[0], prefix.numel()))
    check(_lib.load().adamvs_texture_fill(ctypes.byref(view), _p(items), _p(prefix), items.shape[0], int(texels), int(P), atlas.shape[0],
                                          _p(atlas), _stream()), "texture_fill")


def texture_coords(label, chart, pal, uv, charts, pal_place, P, faces, vrgb, atlas):
    """adamvs_texture_coords -> (tc float32 [nf, 6], texnum int32 [nf]); writes the palette texels into atlas.
    charts int32 [nc, 8]; pal_place = (ox, oy, page) of the palette block."""
    label, chart, pal = (_dev_as(t, n, torch.int32) for t, n in ((label, "label"), (chart, "chart"), (pal, "pal")))
    faces, vrgb, atlas = _dev_as(faces, "faces", torch.int32), _dev_as(vrgb, "rgb", torch.uint8), _dev_as(atlas, "atlas", torch.uint8)
    charts, uv = _dev_as(charts, "charts", torch.int32), _dev(uv, "uv")
    nf = label.numel()
    tc = torch.empty(nf, 6, device=label.device, dtype=torch.float32)
    texnum = torch.empty(nf, device=label.device, dtype=torch.int32)
    check(_lib.load().adamvs_texture_coords(_p(label), _p(chart), _p(pal), _p(uv), nf, _p(charts), *(int(v) for v in pal_place), int(P),
                                            atlas.shape[0], _p(faces), vrgb.shape[0], _p(vrgb), _p(atlas), _p(tc), _p(texnum), _stream()),
          "texture_coords")
    return tc, texnum


# ---- seam levelling (csrc/texture_level.hip; driven by ada_mvs_amd/texture.py) ------------------------------------------------
# The node graph is a CSR built by the caller: rowptr int32 [n + 1], col int32 [nnz] holding uint32 words (bits 0 .. 29 the
# neighbour, bit 30 a seam edge, bit 31 a data edge).
def _level_graph(rowptr, col):
    rowptr, col = _dev_as(rowptr, "rowptr", torch.int32), _dev_as(col, "col", torch.int32)
    n = rowptr.numel() - 1
    if n < 0:
        raise _lib.AdaMVSHipError("texture_level: rowptr must hold n + 1 entries")
    return rowptr, col, n


def texture_level_view_table(views):
    """[_lib.OrthoView] -> the device table int64 [nviews, 3] = (image address, W, H) _level_observe reads (the images must outlive it)."""
    return torch.tensor([[int(v.rgba), int(v.W), int(v.H)] for v in views], dtype=torch.int64).reshape(-1, 3)


def texture_level_observe(view_tab, rowptr, col, node_view, pos):
    """adamvs_texture_level_observe -> f float32 [n, 3]: the colour every node's view shows at it, averaged along its seam edges."""
    rowptr, col, n = _level_graph(rowptr, col)
    view_tab, node_view, pos = _dev_as(view_tab, "view_tab", torch.int64), _dev_as(node_view, "node_view", torch.int32), _dev(pos, "pos")
    if node_view.numel() != n or pos.numel() != 2 * n or view_tab.dim() != 2 or view_tab.shape[1] != 3:
        raise _lib.AdaMVSHipError("texture_level_observe: %d nodes, node_view %d, pos %d" % (n, node_view.numel(), pos.numel()))
    f = torch.empty(n, 3, device=rowptr.device, dtype=torch.float32)
    check(_lib.load().adamvs_texture_level_observe(_p(view_tab), view_tab.shape[0], _p(rowptr), _p(col), col.numel(), _p(node_view), _p(pos),
                                                   n, _p(f), _stream()), "texture_level_observe")
    return f


def texture_level_rhs(rowptr, col, f):
    """adamvs_texture_level_rhs -> b float64 [n, 3] = sum over data neighbours of (f_j - f_i)."""
    rowptr, col, n = _level_graph(rowptr, col)
    f = _dev(f, "f")
    if f.numel() != 3 * n:
        raise _lib.AdaMVSHipError("texture_level_rhs: f %s for %d nodes" % (tuple(f.shape), n))
    b = torch.empty(n, 3, device=rowptr.device, dtype=torch.float64)
    check(_lib.load().adamvs_texture_level_rhs(_p(rowptr), _p(col), col.numel(), _p(f), n, _p(b), _stream()), "texture_level_rhs")
    return b


LEVEL_POLL = 16          # iterations queued per read of the stop flag


def texture_level_solve(rowptr, col, b, lam, tol, iters):
    """Conjugate gradients on L g = b from g = 0 (adamvs_texture_level_cg_init, then adamvs_texture_level_cg in groups of LEVEL_POLL
    iterations with one read of the stop flag after each) -> (g float64 [n, 3], iterations, residual [3] = |r| / |b| per channel
    (0 where b = 0), cap_hit)."""
    rowptr, col, n = _level_graph(rowptr, col)
    b = _dev_as(b, "b", torch.float64)
    lam, tol, iters = float(lam), float(tol), int(iters)
    if b.numel() != 3 * n:
        raise _lib.AdaMVSHipError("texture_level_solve: b %s for %d nodes" % (tuple(b.shape), n))
    dev = rowptr.device
    g, r, p, ap = (torch.zeros(n + 1, 3, device=dev, dtype=torch.float64) for _ in range(4))      # one spare row (16-byte passes)
    partials = torch.zeros(3 * _lib.TEXTURE_LEVEL_BLOCKS, device=dev, dtype=torch.float64)
    state = torch.zeros(16, device=dev, dtype=torch.float64)
    lib = _lib.load()
    check(lib.adamvs_texture_level_cg_init(_p(b) if n else _p(g), n, tol, _p(g), _p(r), _p(p), _p(partials), _p(state), _stream()),
          "texture_level_cg_init")
    # the argument checks of _cg run even when nothing is queued
    check(lib.adamvs_texture_level_cg(_p(rowptr), _p(col), col.numel(), n, lam, 0, _p(g), _p(r), _p(p), _p(ap), _p(partials), _p(state),
                                      _stream()), "texture_level_cg")
    queued = 0
    while queued < iters and float(state[12].item()) == 0.0:
        k = min(LEVEL_POLL, iters - queued)
        check(lib.adamvs_texture_level_cg(_p(rowptr), _p(col), col.numel(), n, lam, k, _p(g), _p(r), _p(p), _p(ap), _p(partials), _p(state),
                                          _stream()), "texture_level_cg")
        queued += k
    st = state.cpu().numpy()
    res = [float(np.sqrt(st[c] / st[3 + c])) if st[3 + c] > 0 else 0.0 for c in range(3)]
    return g[:n], int(st[13]), res, bool(st[12] == 0.0)


def texture_level_owner(uv, chart, charts, prefix, big):
    """adamvs_texture_level_owner -> owner int32 [texels] (2^31 - 1: unowned) over the concatenated chart boxes; prefix int64
    [nc + 1] on the device, big int32 [1 + nf]."""
    uv, chart, charts = _dev(uv, "uv"), _dev_as(chart, "chart", torch.int32), _dev_as(charts, "charts", torch.int32)
    prefix, big = _dev_as(prefix, "prefix", torch.int64), _dev_as(big, "big", torch.int32)
    nf, nc = chart.numel(), prefix.numel() - 1
    if uv.numel() != 6 * nf or nc < 0 or (nc and tuple(charts.shape) != (nc, 8)) or big.numel() < 1:
        raise _lib.AdaMVSHipError("texture_level_owner: %d faces, uv %d, %d charts, charts %s" % (nf, uv.numel(), nc, tuple(charts.shape)))
    texels = int(prefix[-1].item())
    owner = torch.empty(texels, device=chart.device, dtype=torch.int32)
    check(_lib.load().adamvs_texture_level_owner(_p(uv), _p(chart), nf, _p(charts), _p(prefix), nc, texels, _p(owner), _p(big),
                                                 ctypes.c_void_p(big.data_ptr() + 4), big.numel() - 1, _stream()), "texture_level_owner")
    return owner


def texture_level_dilate(charts, prefix, owner):
    """adamvs_texture_level_dilate: one round -> a new owner tensor."""
    charts, prefix, owner = _dev_as(charts, "charts", torch.int32), _dev_as(prefix, "prefix", torch.int64), _dev_as(owner, "owner", torch.int32)
    out = torch.empty_like(owner)
    check(_lib.load().adamvs_texture_level_dilate(_p(charts), _p(prefix), prefix.numel() - 1, owner.numel(), _p(owner), _p(out), _stream()),
          "texture_level_dilate")
    return out


def texture_level_apply(uv, corner_node, g, charts, prefix, owner, P, atlas):
    """adamvs_texture_level_apply: g float64 [n, 3] interpolated in every owned texel's owner and added to atlas (uint8
    [pages, P, P, 4], in place)."""
    uv, corner_node, g = _dev(uv, "uv"), _dev_as(corner_node, "corner_node", torch.int32), _dev_as(g, "g", torch.float64)
    charts, prefix, owner = _dev_as(charts, "charts", torch.int32), _dev_as(prefix, "prefix", torch.int64), _dev_as(owner, "owner", torch.int32)
    if not (atlas.is_cuda and atlas.is_contiguous() and atlas.dtype == torch.uint8) or tuple(atlas.shape[1:]) != (P, P, 4):
        raise _lib.AdaMVSHipError("texture_level_apply: atlas %s for page %d (contiguous uint8 on the device)" % (tuple(atlas.shape), P))
    nf = corner_node.shape[0]
    if uv.numel() != 6 * nf or corner_node.numel() != 3 * nf:
        raise _lib.AdaMVSHipError("texture_level_apply: uv %d, corner_node %d for %d faces" % (uv.numel(), corner_node.numel(), nf))
    check(_lib.load().adamvs_texture_level_apply(_p(uv), _p(corner_node), nf, _p(g), g.shape[0], _p(charts), _p(prefix), prefix.numel() - 1,
                                                 owner.numel(), _p(owner), int(P), atlas.shape[0], _p(atlas), _stream()), "texture_level_apply")
