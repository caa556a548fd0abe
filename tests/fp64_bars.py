"""Per-element bars against the float64 oracle for the depth hot path: FeatureNet0, pass A, pass B + conv1, one recurrent step,
the stage.

A mean relative L1 against the fp32 oracle hides one wrong border column, channel or plane.  The float64 reference is the oracle
itself (oracle/adamvs_oracle.py is dtype-generic) called on `.double()` inputs and `double_sd(sd)`; `check` compares per
element.  A plain module, imported by the test files.
"""
import torch

# (max bar, mean bar): max |err| / max |ref| and mean |err| / mean |ref|, measured on the MI355X over every case of the tests that
# use them (the option reruns included); each bar is just under 4x the measured maximum.
FEATNET = (2.9e-6, 1.5e-6)       # FeatureNet0 stage maps, both fconv_f23 forms: measured at most 7.4e-7 and 4.0e-7
PAIR_SIM = (1.6e-5, 3.1e-6)      # pass A, every plane of every source view: measured at most 4.2e-6 and 7.9e-7
SWEEP = (1.6e-5, 4.8e-6)         # pass B: aggregated similarity, and c1 in fp32 (every conv1_f23 form): measured at most 4.2e-6, 1.2e-6
SWEEP_BX3 = (3.2e-5, 1.8e-5)     # c1 in split bf16 (bf16x3): measured at most 8.2e-6 and 4.7e-6
STEP = (3.4e-6, 1.5e-6)          # reg, state1, state2 of one recurrent step, fp32, gru_wino 0 / 7 / 15: measured at most 8.5e-7, 3.9e-7
STEP_BX3 = (6.5e-5, 4.0e-5)      # the same in bf16x3: measured at most 1.6e-5 and 1.0e-5
# the stage, per pixel: depth and pair depth in hypothesis intervals (measured at most 9.4e-5 fp32, 1.7e-3 bf16x3), confidences
# absolute (2.0e-6, 3.6e-5)
STAGE_DEPTH, STAGE_CONF = 3.7e-4, 8.0e-6
STAGE_DEPTH_BX3, STAGE_CONF_BX3 = 6.6e-3, 1.4e-4
# Pass B on a 4096 x 4112 map (the 2 GiB sweep): the projection R.[x, y, 1].d + t reaches ~2e6 there, so an fp32 tap position is off
# by ~1e-3 px and the similarity by that times the feature gradient -- most where taps leave the image.  The oracle's warp in fp32
# arithmetic errs as much at the same rows (4e-5 ... 4e-4 of max |ref|).  Measured at most 3.0e-4 and 4.7e-5.
SWEEP_4K = (1.2e-3, 1.8e-4)


def double_sd(sd):
    """The state dict with every floating tensor in float64."""
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}


def check(got, ref, max_bar, mean_bar=None, scale=None, what="", dims=None):
    """Fail unless max |got - ref| / scale < max_bar and, given mean_bar, mean |got - ref| / mean |ref| < mean_bar.

    got: a float tensor on any device; ref: float64 of the same shape.  scale defaults to max |ref|; the stage checks pass the
    hypothesis interval for depths and 1 for confidences.  dims names the axes in the message (default n, c, y, x for 4-D and
    n, y, x for 3-D).  A failure names the worst element's index and the fraction of elements over the bar, so that it points
    at a tile edge, a channel or a plane.  Returns (max |err| / scale, mean |err| / mean |ref|)."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu()
    assert ref.dtype == torch.float64, "%s: the reference must be float64, not %s" % (what, ref.dtype)
    assert got.shape == ref.shape, "%s: shape %s, reference %s" % (what, tuple(got.shape), tuple(ref.shape))
    err = torch.nan_to_num((got - ref).abs(), nan=float("inf"))
    if scale is None:
        scale = float(ref.abs().max())
    rel = err / max(float(scale), 1e-30)
    worst = float(rel.max())
    mean = float(err.mean() / ref.abs().mean().clamp_min(1e-30))
    if worst < max_bar and (mean_bar is None or mean < mean_bar):
        return worst, mean
    flat, at = int(torch.argmax(rel)), []
    for n in reversed(rel.shape):
        at.insert(0, flat % n)
        flat //= n
    at = tuple(at)
    names = dims or {4: "ncyx", 3: "nyx"}.get(rel.dim(), ["i%d" % k for k in range(rel.dim())])
    where = ", ".join("%s=%d" % (n, i) for n, i in zip(names, at))
    over = float((rel >= max_bar).double().mean())
    raise AssertionError("%s: max|err| / scale %.3e (bar %.1e) at (%s): got %.9g, ref %.9g; %.3g%% of %d elements over the bar; "
                         "mean |err| / mean |ref| %.3e (bar %s); scale %.6g"
                         % (what, worst, max_bar, where, float(got[at]), float(ref[at]), 100.0 * over, rel.numel(), mean,
                            "-" if mean_bar is None else "%.1e" % mean_bar, float(scale)))
