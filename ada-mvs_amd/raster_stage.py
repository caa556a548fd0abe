"""What the raster stages after dsm_whu.py (dtm.py, buildings.py, roofs.py, trees.py, contours.py, drainage.py, solar.py) share: the grid of
`<prefix>_dsm.json`, the rasters of the earlier stages with their refusals, the default grid of a bare array, the refusal without a
GPU, the look-up that renumbers the kept labels, the files a stage writes and reads back, and the opening of its main().  Nothing
here knows one stage from another: a stage passes its name, its hints and its own output_paths().
"""
import json
import os
import sys
import time

import numpy as np

from .dsm import Grid, world_file_text


def require(path, hint):
    """Refuse an absent file: `hint` says what is missing and which stage to run first."""
    if not os.path.exists(path):
        raise FileNotFoundError("%s: %s" % (path, hint))


def read_grid(prefix):
    """-> the dsm.Grid of `<prefix>_dsm.json`."""
    jpath = prefix + "_dsm.json"
    require(jpath, "no DSM summary (run dsm_whu.py --out %s first)" % prefix)
    with open(jpath) as f:
        js = json.load(f)
    g = js["grid"]
    return Grid(float(g["x0"]), float(g["y_top"]), float(g["gsd"]), float(js.get("z_ref", 0.0)), int(g["W"]), int(g["H"]))


def read_raster(path, dtype, shape, hint=None, says=None):
    """-> the image at `path` as an array of `dtype`.  hint: the refusal of an absent file (require(); None leaves it to the
    open).  A shape other than `shape` is refused as "<path> is <its shape>, <says>"."""
    from PIL import Image
    if hint is not None:
        require(path, hint)
    a = np.array(Image.open(path), dtype)
    if a.shape != tuple(shape):
        raise ValueError("%s is %s, %s" % (path, a.shape, says))
    return a


def default_grid(H, W, gsd, z_ref=0.0):
    """The grid of an array without one: x0 = 0, y_top = H gsd."""
    return Grid(0.0, H * float(gsd), float(gsd), z_ref, W, H)


def no_gpu(stage, kernels):
    return RuntimeError("%s: needs an MI355X (there is no CPU fallback for the %s kernels)" % (stage, kernels))


def grid_summary(grid):
    return dict(x0=grid.x0, y_top=grid.y_top, gsd=grid.gsd, W=grid.W, H=grid.H)


def relabel_kept(labels, keep):
    """labels int32 (device; 0 .. N), keep bool [N] (host) -> the kept labels renumbered 1 .. K in their order, 0 elsewhere
    (device): buildings.relabel as one look-up on the device."""
    import torch
    keep = np.asarray(keep, bool)
    lut = torch.zeros(keep.size + 1, device=labels.device, dtype=torch.int32)
    lut[1:][torch.from_numpy(keep).to(labels.device)] = torch.arange(1, int(keep.sum()) + 1, device=labels.device, dtype=torch.int32)
    return lut[labels.long()]


def write_outputs(paths, out, texts, summary, label=None, grid=None):
    """A stage's files at the path prefix `out`.  paths: its output_paths(out); texts: {key of paths: the file's text}; label: the
    int32 raster of paths["label"], with the world file of `grid` at paths["label_world"]; summary: the dict of paths["json"].
    -> paths"""
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    for key, text in texts.items():
        with open(paths[key], "w") as f:
            f.write(text)
    if label is not None:
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(label, np.int32)).save(paths["label"], format="TIFF")
        with open(paths["label_world"], "w") as f:
            f.write(world_file_text(grid))
    with open(paths["json"], "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    return paths


def read_outputs(paths, keys):
    """-> the files of write_outputs read back: the label raster first where paths has one, then the JSON texts at `keys`, then the
    summary."""
    res = []
    if "label" in paths:
        from PIL import Image
        res.append(np.array(Image.open(paths["label"]), np.int32))
    for key in tuple(keys) + ("json",):
        with open(paths[key]) as f:
            res.append(json.load(f))
    return tuple(res)


def open_main(build_parser, argv):
    """What every main() opens with -> (args, the output prefix, the start time)."""
    args = build_parser().parse_args(argv)
    print("argv:", sys.argv[1:] if argv is None else argv)
    return args, args.out if args.out is not None else args.dsm, time.time()
