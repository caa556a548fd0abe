"""Per-element bars against the float64 oracle for the depth hot path: FeatureNet0, pass A, pass B + conv1, one recurrent step,
the stage.

A mean relative L1 against the fp32 oracle hides one wrong border column, channel or plane.  The float64 reference is the oracle
itself (oracle/adamvs_oracle.py is dtype-generic) called on `.double()` inputs and `double_sd(sd)`; `check` compares per
element.  A plain module, imported by the test files.
"""
import torch

# (max bar, mean bar): max |err| / max |ref| and mean |err| / mean |ref|, measured on the MI355X over every case of the tests that
# use them (the option reruns included); each bar is just under 4x the measured maximum.
FEATNET = (2.9e-6, 1.5e-6)       # FeatureNet0 stage maps, both fconv_f23 forms: measured at most 7.4e-7 and 4.0e-7 (MS-REDNet's U-Net,
                                 # the same kernels with zero context branches, at 64 x 96: 1.12e-6 and 6.7e-7; fp32 oracle 9.7e-7, 6.6e-7)
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


# ---- MS-REDNet (tests/test_msred_forms.py, tests/test_msrednet.py).  These bars are anchored on the REFERENCE, not on the kernels: over
# the cases of the tests that use a bar, the oracle is evaluated in fp32 and in float64 on the CPU; the bar is 4x the largest
# max |fp32 - float64| / max |float64| (and 4x the largest mean ratio) -- the margin of the bars above, since another correct fp32
# evaluation in another summation order lands within a small multiple of the first.  tests/test_fp64_bars.py holds a second fp32
# evaluation (tests/msred_ref.py::recurrence_unfold) to the recurrence bars.  Each comment: the oracle's distance; the MI355X maximum.
RED_PAIR = (5.2e-6, 8.6e-7)      # red_recur_pair, every plane: oracle 1.31e-6 and 2.17e-7 (unfold + matmul: 1.65e-6, 2.53e-7); measured at most 1.63e-6 and 2.50e-7
RED_SPLIT = (1.39e-6, 3.7e-7)    # red_recur_split, every plane: oracle 3.48e-7 and 9.37e-8 (unfold + matmul: 5.85e-7, 1.13e-7); measured at most 8.89e-7 and 1.23e-7
RED_APPLY = (8.4e-7, 2.6e-7)     # gru2_gates_apply / gru2_out_apply on their own: oracle 2.11e-7 and 6.66e-8; measured at most 1.22e-7 and 4.27e-8
RED_CELL = (2.2e-6, 5.8e-7)      # one cell from the golden state (test_gru_cell2_against_reference_golden): oracle 5.69e-7, 1.46e-7; measured 4.58e-7 and 1.46e-7
RED_CONV = (1.6e-6, 8.0e-7)      # conv3x3_pair and the small-grid conv3x3_dd on their own: oracle 4.17e-7 and 2.00e-7; measured at most 7.90e-7 and 3.06e-7
RED_STEP = (6.2e-6, 2.1e-6)      # reg and the four states of a slice step (40 x 72 random costs; the golden 16 x 24): oracle 1.56e-6, 5.30e-7; measured at most 2.18e-6 and 6.43e-7
# red_variance_cost by geometry and map size: an fp32 tap position is off by 2^-24 of the projected coordinate, which grows with the
# map (the rig's focal length is 1.2 x the width), times the feature gradient; most where taps leave the image.  Key: (kind of
# msred_ref.variance_inputs, "small" | "large": under / from 65024 pixels).
RED_VARIANCE = {
    ("rig8", "small"): (2.9e-5, 3.2e-6),      # oracle 7.36e-6 and 8.14e-7; measured at most 5.33e-6 and 5.86e-7
    ("rig8", "large"): (2.4e-4, 1.25e-5),     # oracle 6.05e-5 and 3.14e-6; measured at most 5.38e-5 and 3.00e-6
    ("rig150", "small"): (1.5e-5, 1.9e-6),    # oracle 3.75e-6 and 4.77e-7; measured at most 2.54e-6 and 3.87e-7
    ("rig150", "large"): (1.25e-4, 1.19e-5),  # oracle 3.14e-5 and 2.99e-6; measured at most 1.84e-5 and 3.64e-6
    ("border", "small"): (1.59e-5, 9.5e-7),   # oracle 3.98e-6 and 2.39e-7; measured at most 1.91e-6 and 1.53e-7
    ("border", "large"): (8.8e-5, 3.0e-6),    # oracle 2.20e-5 and 7.51e-7; measured at most 2.06e-5 and 6.68e-7
}
# soft_argmin on +60 / -60 logits, per pixel: depth in hypothesis intervals by plane count (the fp32 rounding of depths near 500 summed
# over D planes, not the exponential), confidence absolute.  Oracle: depth 1.92e-7 (D = 1), 4.22e-6 (8), 9.84e-5 (64), 5.00e-4 (192);
# confidence at most 8.17e-7 (D = 192).  Measured: depth 1.92e-7, 4.22e-6, 8.83e-5, 5.59e-4, confidence at most 8.17e-7
RED_SOFT_DEPTH = {1: 7.6e-7, 8: 1.68e-5, 64: 3.9e-4, 192: 2.0e-3}
RED_SOFT_CONF = 3.2e-6
# one stage (16 x 24, 16 planes, 2 and 6 views), per pixel: oracle depth 2.35e-5 intervals, confidence 1.52e-6; measured 2.51e-5 and 1.35e-6
RED_STAGE_DEPTH, RED_STAGE_CONF = 9.4e-5, 6.0e-6


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
