"""What the mesh stages between mesh_whu.py and texture_whu.py (clean.py, smooth.py, simplify.py) share: the keys they carry from
`<mesh>.json` to `<out>.json`, the metres-or-voxels options, the checks and the weld every stage opens with, the event clock of
its stages, and the file driver (read the PLY, run, write the PLY and `<out>.json`).  Nothing here knows one stage from another:
a stage passes its noun, its limits and closures over its own options.
"""
import json
import math
import os
import time

import numpy as np

CARRIED = ("voxel", "mu", "origin", "views")      # of <mesh>.json, unchanged into <out>.json
MAX_COUNT = (1 << 31) - 1


def mesh_path_of(args):
    if args.mesh:
        return args.mesh
    if not args.output_folder:
        raise ValueError("give --mesh or --output_folder")
    return os.path.join(args.output_folder, "mesh.ply")


def default_out(mesh_path, suffix):
    return (mesh_path[:-4] if mesh_path.lower().endswith(".ply") else mesh_path) + suffix + ".ply"


def positive(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)) or float(v) <= 0:
        raise ValueError("%s=%r must be finite and > 0" % (name, v))


def resolve_metres(name, metres, voxels, default_voxels, meta, power=1, check=positive):
    """--<name> M, or --<name>_voxels K (default_voxels, or None: neither gives None) times the voxel of <mesh>.json to the
    `power` (1: a length, 2: an area).  check(name, value) refuses a value."""
    if metres is not None and voxels is not None:
        raise ValueError("give --%s or --%s_voxels, not both" % (name, name))
    if metres is not None:
        check(name, metres)
        return float(metres)
    k = default_voxels if voxels is None else voxels
    if k is None:
        return None
    check(name + "_voxels", k)
    if meta is None or "voxel" not in meta:
        raise ValueError("<mesh>.json with the voxel size is absent: give --%s" % name)
    res = float(k)
    for _ in range(power):
        res = res * float(meta["voxel"])
    return res


def empty_mesh(device):
    import torch
    return (torch.empty(0, 3, device=device, dtype=torch.float64), torch.empty(0, 3, device=device, dtype=torch.uint8),
            torch.empty(0, 3, device=device, dtype=torch.int32))


class StageClock:
    """The stages of one call as device events: stage(name) opens a stage and closes the one before, end() closes the last and
    hands (name, start event, end event) of every stage to `timing`.  Without a `timing` list nothing is recorded."""

    def __init__(self, timing):
        self.timing, self.marks = timing, []

    def stage(self, name):
        if self.timing is not None:
            import torch
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append((name, e))

    def end(self):
        self.stage("end")
        if self.timing is not None:
            self.timing.extend((a[0], a[1], b[1]) for a, b in zip(self.marks[:-1], self.marks[1:]))


def enter(noun, xyz, rgb, faces, max_faces, clock):
    """What every stage opens with.  xyz [nv, 3] float64, rgb [nv, 3] uint8, faces [nf, 3] int32 (uint32) or int64, device tensors
    of at most MAX_COUNT vertices and max_faces faces -> the welded (xyz, faces int64, rgb), or None for a mesh without vertices.
    noun: the stage in the refusal of a host tensor ("mesh smoothing").  The weld is the clock's stage "weld"."""
    import torch
    from . import _lib, mesh
    for name, t in (("xyz", xyz), ("rgb", rgb), ("faces", faces)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.AdaMVSHipError("%s must be a GPU tensor: %s has no CPU fallback" % (name, noun))
    if xyz.dtype != torch.float64 or rgb.dtype != torch.uint8 or faces.dtype not in (torch.int32, torch.int64):
        raise _lib.AdaMVSHipError("xyz float64, rgb uint8, faces int32 / int64: got %s, %s, %s" % (xyz.dtype, rgb.dtype, faces.dtype))
    if xyz.dim() != 2 or xyz.shape[1] != 3 or tuple(rgb.shape) != tuple(xyz.shape) or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.AdaMVSHipError("xyz [nv, 3], rgb [nv, 3], faces [nf, 3]: got %s, %s, %s" % (tuple(xyz.shape), tuple(rgb.shape), tuple(faces.shape)))
    if xyz.shape[0] == 0:
        if faces.shape[0]:
            raise _lib.AdaMVSHipError("%d faces without vertices" % faces.shape[0])
        return None
    if faces.shape[0] > max_faces or xyz.shape[0] > MAX_COUNT:
        raise _lib.AdaMVSHipError("more than 2^31 - 1 vertices or %sfaces" % ("(2^31 - 1) / 3 " if max_faces < MAX_COUNT else ""))
    f64 = faces.to(torch.int64) & 0xFFFFFFFF
    if faces.shape[0] and int(f64.max()) >= xyz.shape[0]:
        raise _lib.AdaMVSHipError("a face refers to vertex %d of %d" % (int(f64.max()), xyz.shape[0]))
    clock.stage("weld")
    return mesh.weld(xyz.contiguous(), f64, rgb.contiguous())


def summary(meta, head, info, **tail):
    """The dict written to <out>.json: the carried keys of <mesh>.json first, unchanged; then head, info and tail in that order."""
    res = {k: meta[k] for k in CARRIED if meta is not None and k in meta}
    res.update(head)
    res.update(info)
    res.update(tail)
    return res


def volume_origin(options, meta, xyz_h):
    """The default origin of smoothing and cleaning: the volume origin of <mesh>.json, else the per-axis vertex minimum."""
    if meta is not None and "origin" in meta:
        return np.asarray(meta["origin"], np.float64).reshape(3)
    return xyz_h.min(0) if len(xyz_h) else np.zeros(3)


def run_file(stage, kernels, mesh_path, out, origin, device, resolve, default_origin, run, summarise):
    """One stage from the mesh PLY mesh_whu.py (or an earlier stage) wrote to `out` and `<out>.json` -> (the summary, info, options).
    resolve(meta) -> the stage's options, every refusal raised before the device is asked for and before anything is written;
    default_origin(options, meta, xyz_h) -> the origin where `origin` is None;  run(options, xyz, rgb, faces, origin, timing) ->
    (xyz, rgb, faces, info) on the device, `timing` a list for the stage events;  summarise(meta, info, options, origin, source,
    out, seconds, device_seconds, stage_seconds) -> the dict of <out>.json.  stage, kernels: "smooth", "smoothing"."""
    import torch
    from . import mesh
    t_start = time.time()
    meta = None
    if os.path.exists(mesh_path + ".json"):
        with open(mesh_path + ".json") as f:
            meta = json.load(f)
    options = resolve(meta)
    if not torch.cuda.is_available():
        raise RuntimeError("%s: needs an MI355X (there is no CPU fallback for the %s kernels)" % (stage, kernels))
    device = torch.device(device if device is not None else "cuda")
    verts, faces = mesh.read_mesh_ply(mesh_path)
    xyz_h = np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float64)
    rgb_h = np.stack([verts["red"], verts["green"], verts["blue"]], 1)
    o = np.asarray(origin, np.float64).reshape(3) if origin is not None else default_origin(options, meta, xyz_h)
    xyz = torch.from_numpy(np.ascontiguousarray(xyz_h)).to(device)
    rgb = torch.from_numpy(np.ascontiguousarray(rgb_h)).to(device)
    f = torch.from_numpy(faces.astype(np.int64)).to(device)
    timing = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sx, sc, sf, info = run(options, xyz, rgb, f, o, timing)
    e1.record()
    torch.cuda.synchronize(device)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with mesh.MeshPlyWriter(out) as w:
        w.write(sx.cpu().numpy(), sc.cpu().numpy(), sf.cpu().numpy().view(np.uint32))
    res = summarise(meta, info, options, o, mesh_path, out, time.time() - t_start, e0.elapsed_time(e1) / 1e3,
                    {name: a.elapsed_time(b) / 1e3 for name, a, b in timing})
    with open(out + ".json", "w") as fj:
        json.dump(res, fj, indent=1)
        fj.write("\n")
    return res, info, options
