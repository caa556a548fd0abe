"""Inputs of the cloud-registration tests (tests/test_register_host.py, tests/test_register_gpu.py): a seeded terrain at a
georeferenced offset, two sources of it under a known motion, a flat scene that constrains three freedoms only, and the inputs of
the kernel tests (moved queries, index arrays with every kind of non-pair)."""
import numpy as np

OFFSET = (512345.0, 3376543.0, 120.0)
D = 1.0
ANGLE_DEG, AXIS, SHIFT = 2.0, (0.3, -0.5, 0.8), (0.4, -0.3, 0.25)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 65537)       # 65 537: the smallest at which a lane of the reduce holds two partials


def height(x, y):
    return 2.0 * np.sin(x / 5.0) * np.cos(y / 7.0) + 1.5 * np.sin((x + y) / 4.0) + 0.8 * np.cos(x / 3.0 - y / 2.5)


def scene(seed, n, noise, offset=OFFSET):
    """n points of the height field over [0, 40]^2, z with Gaussian noise of sigma `noise`, plus the offset."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 40.0, (n, 2))
    z = height(xy[:, 0], xy[:, 1])
    if noise:
        z = z + rng.normal(0.0, noise, n)
    return np.concatenate([xy, z[:, None]], 1) + np.asarray(offset, np.float64)


def rotation(axis, angle_deg):
    """Rodrigues in numpy, written here and not taken from the driver."""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    a = np.deg2rad(angle_deg)
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def box_centre(points):
    return (points.min(0) + points.max(0)) / 2.0


def moved(points, centre, R, shift):
    return (points - centre) @ R.T + centre + np.asarray(shift, np.float64)


def terrain(offset=OFFSET):
    """-> dict: truth [8000, 3]; copy [4000, 3] = truth[::2] and independent [4000, 3] = scene(2, 4000, 0.03), both moved by 2
    degrees about AXIS through the truth's box centre plus SHIFT; still_copy / still_independent: the same before the motion (what
    a perfect registration gives back); R, shift, centre of the motion."""
    truth = scene(1, 8000, 0.0, offset)
    c = box_centre(truth)
    R = rotation(AXIS, ANGLE_DEG)
    still_copy, still_ind = truth[::2].copy(), scene(2, 4000, 0.03, offset)
    return dict(truth=truth, centre=c, R=R, shift=np.asarray(SHIFT), still_copy=still_copy, still_independent=still_ind,
                copy=moved(still_copy, c, R, SHIFT), independent=moved(still_ind, c, R, SHIFT))


def flat():
    """6000 points uniform on [0, 30]^2 at z = 0 plus the offset; the source: every second point, rolled 0.5 degrees about x through
    the box centre and shifted (0.3, 0, 0.2)."""
    rng = np.random.default_rng(7)
    truth = np.concatenate([rng.uniform(0.0, 30.0, (6000, 2)), np.zeros((6000, 1))], 1) + np.asarray(OFFSET)
    c = box_centre(truth)
    return dict(truth=truth, centre=c, source=moved(truth[::2], c, rotation((1.0, 0.0, 0.0), 0.5), (0.3, 0.0, 0.2)))


def estimate_error(res, source, still):
    """The largest distance over the source between where the estimate (R, t about pivot) puts a point and where it came from."""
    y = (source - res["pivot"]) @ np.asarray(res["R"]).T + res["pivot"] + np.asarray(res["t"])
    return float(np.sqrt(((y - still) ** 2).sum(1)).max())


def apply_cases(n, seed=11):
    """-> (x [n, 3] at the offset with NaN / inf rows where n allows, R, c, t)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 40.0, (n, 3)) + np.asarray(OFFSET)
    if n > 8:
        x[3, 1] = np.nan
        x[5, 0] = np.inf
        x[7] = (-np.inf, np.nan, 1.0)
    c = np.asarray(OFFSET) + (20.0, 20.0, 3.0)
    return x, rotation((0.2, 0.9, -0.4), 7.0), c, np.array([0.7, -1.1, 0.3])


def accumulate_cases(nq, seed=13, nt=500):
    """-> dict of the inputs of icp_accumulate: y [nq, 3], index [nq] int32 holding -1, numbers >= nt, flagged targets and rows of y
    that are not finite among real pairs; targets, normals (unit), flag [nt] uint8 (every seventh target 1 or 2); c, L."""
    rng = np.random.default_rng(seed + nq)
    targets = scene(3, nt, 0.0)
    normals = rng.normal(size=(nt, 3))
    normals /= np.linalg.norm(normals, axis=1)[:, None]
    flag = np.zeros(nt, np.uint8)
    flag[::7] = 1 + (np.arange(len(flag[::7])) % 2)
    index = rng.integers(0, nt, nq).astype(np.int32)
    y = targets[index] + rng.normal(0.0, 0.3, (nq, 3))
    kind = rng.integers(0, 12, nq)
    index[kind == 0] = -1
    index[kind == 1] = nt + rng.integers(0, 3, int((kind == 1).sum()))
    index[kind == 2] = -(2 ** 31)
    y[kind == 3, 0] = np.nan
    y[kind == 4, 2] = np.inf
    c = box_centre(targets)
    e = targets.max(0) - targets.min(0)
    return dict(y=y, index=index, targets=targets, normals=normals, flag=flag, c=c, L=max(0.5 * float(np.sqrt((e * e).sum())), D))


def grid_mesh(offset=OFFSET, n=40):
    """The height field triangulated on an n x n grid over [0, 40]^2 -> (xyz [n^2, 3], rgb [n^2, 3] uint8, faces [2 (n-1)^2, 3] uint32)."""
    g = np.linspace(0.0, 40.0, n)
    x, y = np.meshgrid(g, g, indexing="xy")
    xyz = np.stack([x.ravel(), y.ravel(), height(x.ravel(), y.ravel())], 1) + np.asarray(offset, np.float64)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="xy")
    a = (j * n + i).ravel()
    faces = np.concatenate([np.stack([a, a + 1, a + n + 1], 1), np.stack([a, a + n + 1, a + n], 1)]).astype(np.uint32)
    rgb = np.random.default_rng(5).integers(0, 256, (n * n, 3)).astype(np.uint8)
    return xyz, rgb, faces


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_values(a, b):
    """Equal bit for bit except that any NaN stands for any NaN (the payload of an invalid operation is the processor's)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and same_bits(np.where(nan, 0.0, a), np.where(nan, 0.0, b))
