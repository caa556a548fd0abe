"""The sun exposure of the DSM and of the LoD2 roof planes: horizon, sky-view factor, hours of sun, direct and global energy.

    python solar_whu.py --dsm /out/predict/dsm --latitude 30.5 [--source dsm_filled|dsm|dtm] [--directions 32] [--step_min 30]
                        [--clearness 1.0] [--surface roofs|horizontal] [--days 21,52,..] [--sun_table FILE] [--shadow_at DAY,HOUR]
                        [--out PREFIX]

What GRASS does with r.horizon and r.sun and every solar cadastre with the same two steps, after dsm_whu.py and roofs_whu.py.
Read: `<PREFIX>_<source>.tif` and the grid (`<PREFIX>_dsm.json`); with --surface roofs also `<PREFIX>_roofs.tif` and
`<PREFIX>_roofs.geojson` (the planes' `normal` and `area_3d_m2`).  On the GPU (csrc/dsm_solar.hip; include/adamvs_hip.h "Solar"
states the result operation by operation): the contours' integer surface in 1/256 m; for every cell and each of K = 8, 16 or 32
lattice directions the steepest occluder along the ray to the edge of the raster, exactly (heights times distances compared in
int64, the nearest of equals), by a walk along the lattice lines that keeps the upper convex hull of the cells passed (Dozier,
Bruno and Downey 1981); the sky-view factor 1 - mean(sin^2 horizon) in fp64, operation by operation; for a table of sun positions
the minutes of sun and the direct-beam energy on the cell's plane in integers; their sums per roof plane.  On the host: the sun
positions (Spencer's 1971 series for the declination, the hour angle from local solar time, so no longitude, time zone or
equation of time), the clear-sky direct normal irradiance 1353 * 0.7^(AM^0.678) W/m^2 (Meinel 1976) with the air mass of Kasten
and Young (1989), the diffuse total D = sum of 0.1 DNI sin(elevation), and global = direct + D svf (1 + nz) / 2, the isotropic-sky
convention.  Written: `<out>_svf.tif` (float32, NaN at no data), `<out>_sunhours.tif` (float32, hours per year),
`<out>_direct.tif` and `<out>_global.tif` (float32, kWh/m^2 per year), with --shadow_at `<out>_shadow.tif` (uint8: 1 lit, 0 shadow,
255 no data, from a one-row table), `<out>_solar_roofs.geojson` (the roof polygons with sun_hours, direct_kwh_m2, global_kwh_m2,
the per-plane means, and global_kwh, times area_3d_m2, added) and `<out>_solar.json` (grid, source, parameters, the sample count,
counts, stats, seconds).  --out defaults to --dsm; no name collides with a file of an earlier stage.

The ray march of r.horizon is a serial walk per cell and direction; here the horizon is a definition on integers and the sums
are integer sums, so the stage is bit-identical from run to run.  The defaults (32 directions, day 21 of every month weighted by
the length of its month, a sample every 30 minutes, clearness 1, the clear-sky model above, a diffuse share of a tenth) are
conventions.  They are not values measured on WHU scenes.  Someone with an ephemeris or weather data of their own passes
sun=[T, 5] (azimuth and elevation in degrees, minutes, Wh/m^2 direct normal, Wh/m^2 diffuse horizontal per row) or --sun_table
FILE (the same five columns as text); the built-in model is then not used.

Limits.  The sun's azimuth is snapped to the nearest of the K directions, so the shadow edge of an instant is angularly coarse:
the annual sums are what the stage is for.  Clear sky only.  Nothing outside the raster casts a shadow.  No reflected light.  Tree
canopy occludes as a solid.  Shadows through holes of the surface are wrong, so the default source is the filled DSM.
|z - z_ref| of a cell must not exceed 8191 m and a side 32768 cells; latitude is required because the files carry no CRS.
"""
import argparse
import json
import math
import time

import numpy as np

from . import raster_stage
from .contours import MAX_ABS_M
from .dsm import _check_gsd

STACK_WINDOW = 16                                   # ADAMVS_SOLAR_STACK_WINDOW
MAX_SAMPLES = 8192                                  # ADAMVS_SOLAR_MAX_SAMPLES
MAX_SIDE = 32768                                    # ADAMVS_SOLAR_MAX_SIDE
NO_DATA = -2 ** 31
INT32_MAX = 2 ** 31 - 1
TWO_PI = 2.0 * math.pi
SOURCES = ("dsm_filled", "dsm", "dtm")
SURFACES = ("roofs", "horizontal")
MONTH_DAYS = ((21, 31), (52, 28), (80, 31), (111, 30), (141, 31), (172, 30), (202, 31), (233, 31), (264, 30), (294, 31), (325, 30), (355, 31))
DEFAULTS = dict(directions=32, source="dsm_filled", step_min=30, clearness=1.0, surface="roofs")
SOLAR_CONSTANT = 1353.0                             # W/m^2 (Meinel)
DIFFUSE_SHARE = 0.1
ENERGY_UNITS = 16                                   # units of the energy weights per Wh/m^2
ADDED = ("sun_hours", "direct_kwh_m2", "global_kwh_m2", "global_kwh")
# the header's ADAMVS_SOLAR_DIRS_8, _16, _32: (di, dj) by ascending azimuth, north first
DIRECTIONS = {
    8: ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1)),
    16: ((-1, 0), (-2, 1), (-1, 1), (-1, 2), (0, 1), (1, 2), (1, 1), (2, 1), (1, 0), (2, -1), (1, -1), (1, -2), (0, -1), (-1, -2), (-1, -1),
         (-2, -1)),
    32: ((-1, 0), (-3, 1), (-2, 1), (-3, 2), (-1, 1), (-2, 3), (-1, 2), (-1, 3), (0, 1), (1, 3), (1, 2), (2, 3), (1, 1), (3, 2), (2, 1), (3, 1),
         (1, 0), (3, -1), (2, -1), (3, -2), (1, -1), (2, -3), (1, -2), (1, -3), (0, -1), (-1, -3), (-1, -2), (-2, -3), (-1, -1), (-3, -2),
         (-2, -1), (-3, -1)),
}


# ---- directions ---------------------------------------------------------------------------------------------------------------
def _check_directions(K):
    if isinstance(K, bool) or K not in DIRECTIONS:
        raise ValueError("directions=%r must be 8, 16 or 32" % (K,))
    return int(K)


def direction_azimuths(K):
    """-> float64 [K]: atan2(dj, -di) mod 2 pi, clockwise from north (rows run south)."""
    d = np.array(DIRECTIONS[_check_directions(K)], np.float64)
    return np.mod(np.arctan2(d[:, 1], -d[:, 0]), TWO_PI)


def direction_weights(K):
    """-> float64 [K]: half the angular gap to each cyclic neighbour over 2 pi; they sum to 1."""
    az = direction_azimuths(K)
    nxt = np.mod(np.roll(az, -1) - az, TWO_PI)
    return (nxt + np.roll(nxt, 1)) / 2.0 / TWO_PI


def sector(az, K):
    """The direction at the smallest angular distance from the azimuth az (radians); a tie, to 1e-12 rad, goes to the smaller k."""
    d = np.abs(direction_azimuths(K) - math.fmod(math.fmod(float(az), TWO_PI) + TWO_PI, TWO_PI))
    d = np.minimum(d, TWO_PI - d)
    return int(np.flatnonzero(d <= d.min() + 1e-12)[0])


# ---- the sun ------------------------------------------------------------------------------------------------------------------
def declination(day):
    """Spencer (1971): the sun's declination in radians on day 1 .. 366 of the year."""
    g = TWO_PI * (np.asarray(day, np.float64) - 1.0) / 365.0
    return (0.006918 - 0.399912 * np.cos(g) + 0.070257 * np.sin(g) - 0.006758 * np.cos(2 * g) + 0.000907 * np.sin(2 * g)
            - 0.002697 * np.cos(3 * g) + 0.00148 * np.sin(3 * g))


def sun_at(latitude, day, hour):
    """Latitude in degrees, day of the year, local solar time in hours (arrays broadcast) -> (azimuth, elevation) in radians, the
    azimuth clockwise from north: the spherical triangle of latitude, declination and hour angle."""
    phi, dec = np.radians(np.asarray(latitude, np.float64)), declination(day)
    w = np.radians((np.asarray(hour, np.float64) - 12.0) * 15.0)
    east = -np.cos(dec) * np.sin(w)
    north = np.cos(phi) * np.sin(dec) - np.sin(phi) * np.cos(dec) * np.cos(w)
    up = np.sin(phi) * np.sin(dec) + np.cos(phi) * np.cos(dec) * np.cos(w)
    return np.mod(np.arctan2(east, north), TWO_PI), np.arcsin(np.clip(up, -1.0, 1.0))


def _check_days(days):
    days = MONTH_DAYS if days is None else days
    out = []
    for d in days:
        day, weight = (d if isinstance(d, (tuple, list)) else (d, 1))
        if isinstance(day, bool) or int(day) != day or not 1 <= int(day) <= 366:
            raise ValueError("days: %r is no day 1 .. 366 of the year" % (day,))
        if isinstance(weight, bool) or int(weight) != weight or not 1 <= int(weight) <= 366:
            raise ValueError("days: the weight %r of day %d must be an integer 1 .. 366" % (weight, day))
        out.append((int(day), int(weight)))
    if not out:
        raise ValueError("days must name at least one day")
    return tuple(out)


def sun_positions(latitude, days=None, step_min=DEFAULTS["step_min"]):
    """-> dict(day, weight, hour, azimuth, elevation), arrays [len(days) * 1440 / step_min]: the sun at the middle of every step
    of local solar time on every day (below the horizon included; azimuth and elevation in radians)."""
    days = _check_days(days)
    steps = 1440 // int(step_min)
    hour = (np.arange(steps) + 0.5) * (step_min / 60.0)
    day = np.repeat([d for d, _ in days], steps)
    weight = np.repeat([w for _, w in days], steps)
    hour = np.tile(hour, len(days))
    az, el = sun_at(latitude, day, hour)
    return dict(day=day, weight=weight, hour=hour, azimuth=az, elevation=el)


def clear_sky_dni(elevation):
    """Elevation in radians (> 0) -> the direct normal irradiance in W/m^2: 1353 * 0.7^(AM^0.678) with Kasten and Young's air mass."""
    el = np.asarray(elevation, np.float64)
    am = 1.0 / (np.sin(el) + 0.50572 * (np.degrees(el) + 6.07995) ** -1.6364)
    return SOLAR_CONSTANT * 0.7 ** (am ** 0.678)


def sample_table(gsd, directions=DEFAULTS["directions"], latitude=None, days=None, step_min=DEFAULTS["step_min"], clearness=DEFAULTS["clearness"],
                 sun=None):
    """The rows of the header's step 5, sorted by sector -> dict(sector int64 [T], thr float64 [T], minutes int64 [T], energy int64
    [T] (1/16 Wh/m^2 on a surface facing the sun), sun int64 [T, 3] (round(32768 v), x east, y north, z up), azimuth, elevation
    float64 [T] (radians), diffuse: D in the energy's units).  sun: None for the built-in clear-sky year, or [T, 5] rows (azimuth
    deg, elevation deg, minutes (an integer), Wh/m^2 direct normal, Wh/m^2 diffuse horizontal); rows at or below the horizon add to
    D only.  Raises ValueError for more than MAX_SAMPLES rows and for weights that sum above 2^31 - 1."""
    K = _check_directions(directions)
    gsd = _check_gsd(gsd)
    if sun is None:
        pos = sun_positions(latitude, days, step_min)
        up = pos["elevation"] > 0.0
        az, el, weight = pos["azimuth"][up], pos["elevation"][up], pos["weight"][up].astype(np.float64)
        dni = clear_sky_dni(el)
        hours = step_min / 60.0
        energy = np.rint(ENERGY_UNITS * float(clearness) * dni * hours * weight)
        minutes = np.rint(step_min * weight)
        diffuse = float(np.sum(DIFFUSE_SHARE * dni * np.sin(el) * (ENERGY_UNITS * hours) * weight))
    else:
        rows = np.asarray(sun, np.float64)
        if rows.ndim != 2 or rows.shape[1] != 5 or not np.isfinite(rows).all():
            raise ValueError("sun %s must be [T, 5] finite rows: azimuth deg, elevation deg, minutes, Wh/m2 direct normal, Wh/m2 diffuse" % (rows.shape,))
        if (rows[:, 2:] < 0).any() or (rows[:, 2] != np.rint(rows[:, 2])).any() or (np.abs(rows[:, 1]) > 90).any():
            raise ValueError("sun: minutes must be integers >= 0, the energies >= 0 and |elevation| <= 90")
        diffuse = float(ENERGY_UNITS * rows[:, 4].sum())
        rows = rows[rows[:, 1] > 0.0]
        az, el = np.mod(np.radians(rows[:, 0]), TWO_PI), np.radians(rows[:, 1])
        minutes, energy = rows[:, 2], np.rint(ENERGY_UNITS * rows[:, 3])
    if az.size > MAX_SAMPLES:
        raise ValueError("%d samples of the sun above the horizon: at most %d (fewer days or a longer step)" % (az.size, MAX_SAMPLES))
    if minutes.sum() > INT32_MAX or energy.sum() > INT32_MAX:
        raise ValueError("the weights sum to %.0f minutes and %.0f energy units: at most 2^31 - 1 each" % (minutes.sum(), energy.sum()))
    sec = np.array([sector(a, K) for a in az], np.int64)
    len2 = np.array([di * di + dj * dj for di, dj in DIRECTIONS[K]], np.float64)
    thr = np.tan(el) * np.sqrt(len2[sec]) * gsd * 256.0
    vec = np.stack([np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), np.sin(el)], axis=1)
    order = np.argsort(sec, kind="stable")
    pick = lambda a: a[order]
    return dict(sector=pick(sec), thr=pick(thr), minutes=pick(minutes.astype(np.int64)), energy=pick(energy.astype(np.int64)),
                sun=pick(np.rint(32768.0 * vec).astype(np.int64)), azimuth=pick(az), elevation=pick(el), diffuse=diffuse)


def parameters(gsd, directions=DEFAULTS["directions"], latitude=None, days=None, step_min=DEFAULTS["step_min"], clearness=DEFAULTS["clearness"],
               surface=DEFAULTS["surface"], source=DEFAULTS["source"], sun=None):
    """The checked parameters.  latitude (degrees, north positive) is required unless `sun` brings the positions: the files carry
    no CRS.  days: days of the year, or (day, the days it stands for) pairs; default day 21 of every month weighted by the length
    of its month.  Raises ValueError."""
    _check_gsd(gsd)
    K = _check_directions(directions)
    if source not in SOURCES:
        raise ValueError("source=%r must be one of %s" % (source, ", ".join(SOURCES)))
    if surface not in SURFACES:
        raise ValueError("surface=%r must be one of %s" % (surface, ", ".join(SURFACES)))
    if isinstance(step_min, bool) or int(step_min) != step_min or not 1 <= int(step_min) <= 120 or 1440 % int(step_min):
        raise ValueError("step_min=%r must be an integer 1 .. 120 that divides a day" % (step_min,))
    if isinstance(clearness, bool) or not math.isfinite(float(clearness)) or not 0.0 <= float(clearness) <= 1.0:
        raise ValueError("clearness=%r must lie in 0 .. 1" % (clearness,))
    if sun is None:
        if latitude is None:
            raise ValueError("latitude is required (degrees, north positive): the files carry no CRS")
        if isinstance(latitude, bool) or not math.isfinite(float(latitude)) or not -90.0 <= float(latitude) <= 90.0:
            raise ValueError("latitude=%r must lie in -90 .. 90" % (latitude,))
    days = _check_days(days)
    return dict(directions=K, latitude=None if latitude is None else float(latitude), days=[list(d) for d in days], step_min=int(step_min),
                clearness=float(clearness), surface=surface, source=source, own_sun=sun is not None)


# ---- the stage ----------------------------------------------------------------------------------------------------------------
def _no_gpu():
    return raster_stage.no_gpu("solar", "solar")


def quantise_normals(normals):
    """normals float [P, 3] (unit, east north up) for the labels 1 .. P -> int64 [P + 1, 3]: round(32768 n), row 0 horizontal."""
    n = np.asarray(normals, np.float64).reshape(-1, 3)
    if not np.isfinite(n).all() or (np.abs(n) > 1.0).any():
        raise ValueError("normals must be finite unit vectors")
    return np.concatenate([np.array([[0, 0, 32768]], np.int64), np.rint(32768.0 * n).astype(np.int64)])


def horizons(z, gsd, z_ref=0.0, directions=DEFAULTS["directions"], device=None):
    """z [H, W] float32 (host; NaN where there is no value) -> (s, hz_n, hz_h, stats, the workspace) on the device."""
    import torch
    from . import hip_ops
    dev = torch.device(device if device is not None else "cuda")
    s, info = hip_ops.contour_surface(torch.from_numpy(z).to(dev), float(z_ref), 0)
    out_of_range = int(info.cpu()[2])
    if out_of_range:
        raise ValueError("solar: %d cells lie further than %d m from z_ref=%g" % (out_of_range, MAX_ABS_M, float(z_ref)))
    hz_n, hz_h, stats, ws = hip_ops.solar_horizon(s, directions)
    return s, hz_n, hz_h, stats, ws


def expose(z, gsd, z_ref=0.0, label=None, normals=None, directions=DEFAULTS["directions"], latitude=None, days=None,
           step_min=DEFAULTS["step_min"], clearness=DEFAULTS["clearness"], sun=None, shadow_at=None, grid=None, device=None):
    """z [H, W] float32 (host; NaN where there is no value), label int [H, W] with 0 .. P and normals float [P, 3] (the planes' unit
    normals, east north up) or neither (every cell horizontal) -> dict(s, hz_n, hz_h, svf float64, minutes, direct int32, table
    int64 [3, P + 1] (all as the header names them, numpy), sun_hours, direct_kwh, global_kwh float64 [H, W] (hours, kWh/m^2; NaN
    at no data; global = direct + D svf (1 + nz) / 2, the isotropic-sky convention), planes: dict of float64 [P + 1] columns
    (cells, sun_hours, direct_kwh_m2, global_kwh_m2: the means over each label's cells), shadow uint8 [H, W] with shadow_at =
    (day, hour), samples, diffuse, params, counts, stats, seconds).  Raises ValueError for bad parameters and for a finite height
    further than 8191 m from z_ref, RuntimeError without a GPU: there is no CPU fallback."""
    import torch
    from . import hip_ops
    p = parameters(gsd, directions, latitude, days, step_min, clearness, "horizontal" if label is None else "roofs", sun=sun)
    gsd = _check_gsd(gsd)
    z = np.ascontiguousarray(z, np.float32)
    if z.ndim != 2:
        raise ValueError("z %s must be [H, W]" % (z.shape,))
    if max(z.shape) > MAX_SIDE or z.size > 2 ** 28:
        raise ValueError("z %s: at most %d cells a side and 2^28 cells" % (z.shape, MAX_SIDE))
    if not math.isfinite(float(z_ref)):
        raise ValueError("z_ref=%r must be finite" % (z_ref,))
    if (label is None) != (normals is None):
        raise ValueError("label and normals go together")
    H, W = z.shape
    K = p["directions"]
    nq = None
    if label is not None:
        label = np.ascontiguousarray(label, np.int32)
        nq = quantise_normals(normals)
        if label.shape != z.shape or label.min(initial=0) < 0 or label.max(initial=0) > nq.shape[0] - 1:
            raise ValueError("label %s must be [%d, %d] with values 0 .. %d" % (label.shape, H, W, nq.shape[0] - 1))
    P = 0 if nq is None else nq.shape[0] - 1
    table = sample_table(gsd, K, latitude, days, step_min, clearness, sun)
    if shadow_at is not None:
        if latitude is None:
            raise ValueError("shadow_at needs a latitude")
        az1, el1 = sun_at(latitude, shadow_at[0], shadow_at[1])
        one = sample_table(gsd, K, sun=[[math.degrees(float(az1)), math.degrees(float(el1)), 1, 0.0, 0.0]])
    if not torch.cuda.is_available():
        raise _no_gpu()
    if grid is None:
        grid = raster_stage.default_grid(H, W, gsd, float(z_ref))
    dev = torch.device(device if device is not None else "cuda")
    torch.cuda.synchronize(dev)
    t0 = time.time()
    s, hz_n, hz_h, st_hz, ws = horizons(z, gsd, z_ref, K, dev)
    t1 = time.time()
    svf = hip_ops.solar_svf(s, hz_n, hz_h, direction_weights(K), (256.0 * gsd) ** 2)
    torch.cuda.synchronize(dev)
    t2 = time.time()
    lab_d = None if label is None else torch.from_numpy(label).to(dev)
    nrm_d = None if nq is None else torch.from_numpy(nq.astype(np.int32)).to(dev)
    minutes, direct, ws = hip_ops.solar_expose(s, hz_n, hz_h, table, lab_d, nrm_d, ws)
    shadow = None
    if shadow_at is not None:
        shadow = hip_ops.solar_expose(s, hz_n, hz_h, one, None, None, ws)[0] if one["sector"].size else torch.zeros_like(minutes)
    t3 = time.time()
    sums = hip_ops.solar_plane_sums(s, minutes, direct, lab_d, P)
    res = dict(s=s, hz_n=hz_n, hz_h=hz_h, svf=svf, minutes=minutes, direct=direct, table=sums)
    res = {k: v.cpu().numpy() for k, v in res.items()}
    t4 = time.time()
    V = res["s"] != NO_DATA
    nz = np.ones((H, W)) if nq is None else (nq[:, 2] / 32768.0)[label]
    D = table["diffuse"]
    per = 1.0 / (ENERGY_UNITS * 1000.0)                             # energy units -> kWh/m^2
    nan = lambda a: np.where(V, a, np.nan)
    res["sun_hours"] = nan(res["minutes"] / 60.0)
    res["direct_kwh"] = nan(res["direct"] * per)
    res["global_kwh"] = nan((res["direct"] + D * res["svf"] * (1.0 + nz) / 2.0) * per)
    if shadow is not None:
        res["shadow"] = np.where(V, (shadow.cpu().numpy() > 0).astype(np.uint8), 255).astype(np.uint8)
    cells = res["table"][0].astype(np.float64)
    lab = np.zeros((H, W), np.int64) if label is None else label.astype(np.int64)
    svf_sum = np.bincount(lab[V], weights=res["svf"][V], minlength=P + 1)
    nzp = np.ones(1) if nq is None else nq[:, 2] / 32768.0
    with np.errstate(invalid="ignore", divide="ignore"):
        res["planes"] = dict(cells=res["table"][0], sun_hours=res["table"][1] / 60.0 / cells, direct_kwh_m2=res["table"][2] * per / cells,
                             global_kwh_m2=(res["table"][2] + D * svf_sum * (1.0 + nzp) / 2.0) * per / cells)
    t5 = time.time()
    counts = dict(valid=int(V.sum()), planes=P, on_planes=int((lab[V] > 0).sum()), samples=int(table["sector"].size),
                  never_lit=int((V & (res["minutes"] == 0)).sum()), open_sky=int((V & (res["hz_h"].max(axis=0) == 0)).sum()))
    res.update(samples=table, diffuse=D, params=p, counts=counts, stats=dict(horizon=st_hz), grid=grid, gsd=float(gsd), z_ref=float(z_ref),
               seconds=dict(horizon=t1 - t0, svf=t2 - t1, expose=t3 - t2, planes=t4 - t3, host=t5 - t4))
    return res


def read_roofs(prefix, grid):
    """-> (label int32 [H, W], normals float [P, 3], the GeoJSON dict) of roofs_whu.py: plane r of the raster is the feature with
    id r."""
    paths = dict(label=prefix + "_roofs.tif", geojson=prefix + "_roofs.geojson")
    for path in paths.values():
        raster_stage.require(path, "no roof planes (run roofs_whu.py --dsm %s first, or pass --surface horizontal)" % prefix)
    label = raster_stage.read_raster(paths["label"], np.int32, (grid.H, grid.W), says="the grid %d x %d" % (grid.H, grid.W))
    with open(paths["geojson"]) as f:
        gj = json.load(f)
    ids = [int(f["properties"]["id"]) for f in gj["features"]]
    if sorted(ids) != list(range(1, len(ids) + 1)) or label.min(initial=0) < 0 or label.max(initial=0) > len(ids):
        raise ValueError("%s: the ids of the planes must be 1 .. %d and cover the labels of %s" % (paths["geojson"], len(ids), paths["label"]))
    normals = np.zeros((len(ids), 3))
    for f in gj["features"]:
        normals[int(f["properties"]["id"]) - 1] = f["properties"]["normal"]
    return label, normals, gj


def read_sun_table(path):
    """A text file of rows `azimuth_deg elevation_deg minutes Wh/m2_direct_normal Wh/m2_diffuse_horizontal` (# starts a comment)."""
    raster_stage.require(path, "no such sun table")
    return np.loadtxt(path, dtype=np.float64, comments="#", ndmin=2)


def from_dsm(prefix, source=DEFAULTS["source"], surface=DEFAULTS["surface"], directions=DEFAULTS["directions"], latitude=None, days=None,
             step_min=DEFAULTS["step_min"], clearness=DEFAULTS["clearness"], sun=None, shadow_at=None, device=None, out=None):
    """The raster `<prefix>_<source>.tif` of an earlier stage -> expose()'s dict with `source`, `roofs` (the GeoJSON of the planes or
    None) added; written to `out` (a path prefix) if given.  The heights are quantised about the grid's z_ref."""
    import torch
    parameters(1.0, directions, latitude, days, step_min, clearness, surface, source, sun)     # what needs no file, before any file
    grid = raster_stage.read_grid(prefix)
    path = "%s_%s.tif" % (prefix, source)
    hint = {"dsm_filled": "no filled DSM: shadows through holes are wrong, so run dsm_whu.py --fill_max_dist .. --out %s first, or pass "
                          "--source dsm to take the DSM with its holes" % prefix,
            "dsm": "no such raster (run dsm_whu.py --out %s first)" % prefix, "dtm": "no such raster (run dtm_whu.py --dsm %s first)" % prefix}
    raster_stage.require(path, hint[source])
    label = normals = gj = None
    if surface == "roofs":
        label, normals, gj = read_roofs(prefix, grid)
    if not torch.cuda.is_available():
        raise _no_gpu()
    z = raster_stage.read_raster(path, np.float32, (grid.H, grid.W), says="the grid %d x %d" % (grid.H, grid.W))
    res = expose(z, grid.gsd, grid.z_ref, label, normals, directions, latitude, days, step_min, clearness, sun, shadow_at, grid, device)
    res["params"].update(source=source, surface=surface)
    res["source"] = dict(prefix=prefix, raster=source)
    res["roofs"] = gj
    if out is not None:
        write_outputs(out, res)
    return res


# ---- files --------------------------------------------------------------------------------------------------------------------
def output_paths(out):
    """The files of this stage, disjoint from those of every earlier stage."""
    return dict(svf=out + "_svf.tif", sunhours=out + "_sunhours.tif", direct=out + "_direct.tif", global_=out + "_global.tif",
                shadow=out + "_shadow.tif", geojson=out + "_solar_roofs.geojson", json=out + "_solar.json")


def _number(v):
    return float("%.6g" % v) if math.isfinite(v) else None


def geojson_text(roofs, planes):
    """The roof polygons with ADDED appended to their properties: fixed key order and number formatting (six significant digits),
    equal inputs give equal bytes.  roofs None: an empty collection."""
    out = []
    for f in ([] if roofs is None else roofs["features"]):
        r = int(f["properties"]["id"])
        props = dict(f["properties"])
        g = float(planes["global_kwh_m2"][r])
        props.update(sun_hours=_number(float(planes["sun_hours"][r])), direct_kwh_m2=_number(float(planes["direct_kwh_m2"][r])),
                     global_kwh_m2=_number(g), global_kwh=_number(g * float(f["properties"]["area_3d_m2"])))
        out.append(dict(type="Feature", properties=props, geometry=f["geometry"]))
    return json.dumps(dict(type="FeatureCollection", features=out), separators=(",", ":")) + "\n"


def summary(res):
    return dict(grid=raster_stage.grid_summary(res["grid"]), source=res.get("source"), params=dict(res["params"], z_ref=res["z_ref"]),
                samples=int(res["samples"]["sector"].size), diffuse_kwh_m2=res["diffuse"] / (ENERGY_UNITS * 1000.0), counts=res["counts"],
                stats=res["stats"], seconds=res["seconds"])


def write_outputs(out, res):
    """The rasters, the GeoJSON file and the JSON summary at the path prefix `out` -> the paths written."""
    from PIL import Image
    paths = output_paths(out)
    if "shadow" not in res:
        del paths["shadow"]
    raster_stage.write_outputs(paths, out, dict(geojson=geojson_text(res.get("roofs"), res["planes"])), summary(res))
    V = res["s"] != NO_DATA
    for key, a in (("svf", np.where(V, res["svf"], np.nan)), ("sunhours", res["sun_hours"]), ("direct", res["direct_kwh"]),
                   ("global_", res["global_kwh"])):
        Image.fromarray(np.ascontiguousarray(a, np.float32)).save(paths[key], format="TIFF")
    if "shadow" in res:
        Image.fromarray(np.ascontiguousarray(res["shadow"], np.uint8)).save(paths["shadow"], format="TIFF")
    return paths


def _shadow_at(text):
    try:
        day, hour = text.split(",")
        day, hour = int(day), float(hour)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not DAY,HOUR" % text)
    if not (1 <= day <= 366 and 0.0 <= hour <= 24.0):
        raise argparse.ArgumentTypeError("%r: DAY is 1 .. 366, HOUR 0 .. 24 of local solar time" % text)
    return day, hour


def build_parser():
    ap = argparse.ArgumentParser(description="Sun exposure of the DSM and the roof planes: horizon, sky-view factor, sun hours, direct and global energy")
    ap.add_argument("--dsm", required=True, metavar="PREFIX", help="path prefix of the earlier stages' output "
                    "(<PREFIX>_<source>.tif, <PREFIX>_dsm.json, <PREFIX>_roofs.tif, <PREFIX>_roofs.geojson)")
    ap.add_argument("--source", choices=SOURCES, default=DEFAULTS["source"], help="the height raster that casts and receives the shadows")
    ap.add_argument("--surface", choices=SURFACES, default=DEFAULTS["surface"], help="roofs: the cells of roofs_whu.py's planes take the planes' "
                    "normals; horizontal: every cell is level")
    ap.add_argument("--directions", type=int, choices=sorted(DIRECTIONS), default=DEFAULTS["directions"], help="azimuth directions of the horizon")
    ap.add_argument("--latitude", type=float, default=None, help="degrees, north positive; required unless --sun_table is given")
    ap.add_argument("--days", default=None, metavar="D,D,..", help="days of the year, equally weighted (default: day 21 of every month, "
                    "weighted by the length of its month)")
    ap.add_argument("--step_min", type=int, default=DEFAULTS["step_min"], help="minutes of local solar time between samples of the sun")
    ap.add_argument("--clearness", type=float, default=DEFAULTS["clearness"], help="factor 0 .. 1 on the clear-sky direct beam")
    ap.add_argument("--sun_table", default=None, metavar="FILE", help="rows of azimuth_deg elevation_deg minutes Wh/m2_direct_normal "
                    "Wh/m2_diffuse_horizontal in place of the built-in clear-sky year")
    ap.add_argument("--shadow_at", type=_shadow_at, default=None, metavar="DAY,HOUR", help="also write <out>_shadow.tif for this day of the year "
                    "and hour of local solar time (needs --latitude)")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="output path prefix (default: --dsm): <out>_svf.tif, <out>_sunhours.tif, "
                    "<out>_direct.tif, <out>_global.tif, <out>_shadow.tif, <out>_solar_roofs.geojson, <out>_solar.json")
    return ap


def main(argv=None):
    args, out, t0 = raster_stage.open_main(build_parser, argv)
    days = None if args.days is None else [int(d) for d in args.days.split(",")]
    sun = None if args.sun_table is None else read_sun_table(args.sun_table)
    if args.shadow_at is not None and args.latitude is None:
        raise SystemExit("--shadow_at needs --latitude")
    res = from_dsm(args.dsm, args.source, args.surface, args.directions, args.latitude, days, args.step_min, args.clearness, sun, args.shadow_at,
                   out=out)
    g, c, s, st = res["grid"], res["counts"], res["seconds"], res["stats"]["horizon"]
    print("solar %d x %d cells at gsd %g: %d valid cells, %d directions, %d lines (deepest stack %d, %d spills), %d samples of the sun, %d planes "
          "over %d cells, %d cells never lit" % (g.W, g.H, g.gsd, c["valid"], res["params"]["directions"], st["lines"], st["deepest"], st["spills"],
                                               c["samples"], c["planes"], c["on_planes"], c["never_lit"]))
    print("horizon %.3f s (%.3f ms on the device), svf %.3f s, exposure %.3f s, planes %.3f s, host %.3f s; total_time = %.3f s"
          % (s["horizon"], st["ms"], s["svf"], s["expose"], s["planes"], s["host"], time.time() - t0))
    return res


if __name__ == "__main__":
    main()
