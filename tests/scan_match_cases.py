"""Inputs shared by tests/test_scan_match_host.py and tests/test_gpu_scan_match.py: the recovery room, hand-made maps and
the small grids of the stand-alone GPU cases.  Everything is generated from seeds; nothing here touches a GPU."""
import math

import numpy as np

# ---- the recovery room: an L-shaped room with a box in it, 0.1 m cells on a 200 x 200 window ----
ROOM_OCC = dict(resolution=0.1, width=200, height=200, z_min=0.0, z_max=2.0, max_range=20.0)
ROOM_SCAN = dict(nx=4, ny=4, nt=4, xy_step=1024, theta_step=8, min_cells=50, min_mean=0)
ROOM_WALLS = [(-6.0, -4.0), (7.0, -4.0), (7.0, 2.0), (1.0, 2.0), (1.0, 6.0), (-6.0, 6.0)]      # closed
ROOM_BOX = (3.2, -1.9, 0.6)              # lower corner and side of the box
ROOM_RETURNS = 6000
ROOM_NOISE = 0.01
ROOM_SEEDS = tuple(range(12))
TICK = 2.0 * math.pi / 4096.0


def _segments():
    w = ROOM_WALLS
    seg = [(w[i], w[(i + 1) % len(w)]) for i in range(len(w))]
    x, y, s = ROOM_BOX
    b = [(x, y), (x + s, y), (x + s, y + s), (x, y + s)]
    return seg + [(b[i], b[(i + 1) % 4]) for i in range(4)]


def room_returns(rng, n=ROOM_RETURNS, scale=1.0):
    """n points on the walls and the box in the fixed frame, uniform along their length, z in the hit band (scale: the
    room's plan shrunk by it, for the small windows of the GPU tests)."""
    seg = np.array(_segments(), np.float64) * scale              # [S, 2, 2]
    length = np.linalg.norm(seg[:, 1] - seg[:, 0], axis=1)
    k = rng.choice(len(seg), size=n, p=length / length.sum())
    u = rng.uniform(0.0, 1.0, n)[:, None]
    xy = seg[k, 0] + u * (seg[k, 1] - seg[k, 0])
    return np.concatenate([xy, rng.uniform(0.2, 1.5, (n, 1))], axis=1)


def sensor_frame(world, pose, rng, noise=ROOM_NOISE):
    """The fixed-frame points as the sensor at `pose` [3, 4] returns them: R^T (p - t) plus noise, float32."""
    P = np.asarray(pose, np.float64)
    p = (world - P[:, 3]) @ P[:, :3]
    return (p + rng.normal(0.0, noise, p.shape)).astype(np.float32)


def yaw_pose(pp, x, y, yaw):
    return pp.sweeps.pose_from_xyyaw(x, y, yaw)


def room_case(pp, seed):
    """(map after five frames under true poses, the sixth frame, its prior, the displacement in steps (a, b, c) that
    leads from the prior to the truth): the prior is the truth moved back by whole steps, each axis -3 .. 3."""
    rng = np.random.default_rng(1000 + seed)
    m = pp.occupancy.OccupancyMap(ROOM_OCC)
    x0, y0, yaw0 = rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), rng.uniform(-math.pi, math.pi)
    for k in range(5):
        T = yaw_pose(pp, x0 + 0.05 * k, y0 - 0.03 * k, yaw0 + 0.02 * k)
        m.update(sensor_frame(room_returns(rng), T, rng), T)
    a, b, c = (int(v) for v in rng.integers(-3, 4, 3))
    x, y, yaw = x0 + 0.25, y0 - 0.15, yaw0 + 0.1
    T = yaw_pose(pp, x, y, yaw)
    pts = sensor_frame(room_returns(rng), T, rng)
    step = ROOM_SCAN["xy_step"] / 1024.0 * ROOM_OCC["resolution"]
    prior = yaw_pose(pp, x - a * step, y - b * step, yaw - c * ROOM_SCAN["theta_step"] * TICK)
    return m, pts, prior, (a, b, c)


# ---- hand-made maps ----
def blank(pp, w, h, **more):
    """(OccupancyConfig of a w x h window of 1 m cells that takes every z, L int16 zeros, known bool False)."""
    oc = pp.occupancy.OccupancyConfig(resolution=1.0, width=w, height=h, z_min=-10.0, z_max=10.0, max_range=1000.0, **more)
    return oc, np.zeros((h, w), np.int16), np.zeros((h, w), bool)


def rows_at(cells, res=1.0, z=0.0):
    """float32 rows whose x y are the centres of the sensor-frame cells (gx - W // 2, gy - H // 2) given."""
    c = np.asarray(cells, np.float64).reshape(-1, 2)
    return np.concatenate([(c + 0.5) * res, np.full((len(c), 1), z)], axis=1).astype(np.float32)


IDENTITY = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])


def at(x, y):
    P = IDENTITY.copy()
    P[0, 3], P[1, 3] = x, y
    return P


# ---- the stand-alone GPU cases: (name, occupancy fields, scan fields, per stream (origin cell or None, pose, rows)) ----
def random_map(rng, w, h, known_share=0.7):
    L = rng.integers(-200, 351, (h, w)).astype(np.int16)
    K = rng.uniform(0, 1, (h, w)) < known_share
    return L, K


def random_rows(rng, n, w, h, res):
    """n rows over and a little around a w x h window of `res` cells centred on the sensor, z around the hit band, with
    some NaN and infinite rows among them."""
    p = np.stack([rng.uniform(-0.6 * w * res, 0.6 * w * res, n), rng.uniform(-0.6 * h * res, 0.6 * h * res, n),
                  rng.uniform(-0.5, 1.5, n)], axis=1).astype(np.float32)
    if n >= 8:
        p[3, 0], p[5, 1], p[6, 2] = np.nan, np.inf, np.nan
    return p


def grid_cases(pp):
    """A list of dicts: name, occ (OccupancyConfig), scan (ScanMatchConfig fields), L [B, H, W], K [B, H, W], points (list),
    poses [B, 3, 4], origins (list of (ox, oy) or None)."""
    out = []

    def add(name, w, h, res, scan, streams, seed):
        rng = np.random.default_rng(seed)
        oc = pp.occupancy.OccupancyConfig(resolution=res, width=w, height=h, z_min=0.0, z_max=1.0, max_range=0.55 * max(w, h) * res)
        Ls, Ks, pts, poses, orgs = [], [], [], [], []
        for n, origin, (x, y, yaw) in streams:
            L, K = random_map(rng, w, h)
            Ls.append(L), Ks.append(K)
            pts.append(random_rows(rng, n, w, h, res))
            poses.append(yaw_pose(pp, x, y, yaw))
            orgs.append(origin)
        out.append(dict(name=name, occ=oc, scan=scan, L=np.stack(Ls), K=np.stack(Ks), points=pts, poses=np.stack(poses), origins=orgs))

    # the sensor in the window's middle cell: origin = floor(t / res) - (w // 2, h // 2)
    def mid(w, h, res, x, y):
        return (int(math.floor(x / res)) - w // 2, int(math.floor(y / res)) - h // 2)

    # 70 x 50: up to 3500 scan cells, more than three LDS chunks of 1024 and no multiple of one; 285 translations
    add("long-list-285-translations", 70, 50, 0.1, dict(nx=9, ny=7, nt=1, xy_step=1024, theta_step=8, min_cells=0, min_mean=-100000),
        [(30000, mid(70, 50, 0.1, 0.33, -0.21), (0.33, -0.21, 0.4))], 31)
    add("empty-and-one-row", 15, 11, 0.25, dict(nx=2, ny=1, nt=2, xy_step=512, theta_step=16, min_cells=1, min_mean=0),
        [(0, mid(15, 11, 0.25, 1.0, 2.0), (1.0, 2.0, -1.0)), (1, mid(15, 11, 0.25, -3.3, 0.7), (-3.3, 0.7, 2.5))], 32)
    add("one-translation-many-headings", 70, 11, 0.2, dict(nx=0, ny=0, nt=20, xy_step=1, theta_step=100, min_cells=0, min_mean=0),
        [(900, mid(70, 11, 0.2, 0.0, 0.0), (0.0, 0.0, 0.1))], 33)               # dh from -2000 to 2000: & 4095 through negatives
    add("one-heading", 15, 50, 0.2, dict(nx=6, ny=5, nt=0, xy_step=700, theta_step=1, min_cells=0, min_mean=0),
        [(700, mid(15, 50, 0.2, 5.0, 5.0), (5.0, 5.0, 3.0))], 34)
    # batch 3: a stream without a map, one whose prior lies outside its window, one matched; different scan counts
    add("no-map-outside-and-matched", 70, 50, 0.1, dict(nx=3, ny=3, nt=2, xy_step=1024, theta_step=8, min_cells=0, min_mean=0),
        [(400, None, (0.0, 0.0, 0.0)), (1300, mid(70, 50, 0.1, 9.0, 0.0), (0.5, 0.2, 0.3)), (2100, mid(70, 50, 0.1, -1.0, 1.0), (-1.0, 1.0, -0.7))], 35)
    # a prior near the window's edge: the origin puts the sensor 2 cells from the corner, so candidates leave the window
    add("near-the-edge", 15, 11, 0.5, dict(nx=5, ny=5, nt=3, xy_step=1024, theta_step=64, min_cells=0, min_mean=0),
        [(300, (int(math.floor(2.0 / 0.5)) - 2, int(math.floor(-1.0 / 0.5)) - 9), (2.0, -1.0, 0.2)),
         (300, (int(math.floor(2.0 / 0.5)) - 13, int(math.floor(-1.0 / 0.5)) - 1), (2.0, -1.0, 0.2))], 36)
    return out


def tie_case(pp):
    """Exact ties: a map of one constant value, all known, so every candidate that keeps the scan inside scores alike."""
    oc = pp.occupancy.OccupancyConfig(resolution=0.1, width=70, height=50, z_min=0.0, z_max=1.0, max_range=2.0)
    rng = np.random.default_rng(37)
    pts = np.stack([rng.uniform(-0.8, 0.8, 500), rng.uniform(-0.8, 0.8, 500), rng.uniform(0.1, 0.9, 500)], axis=1).astype(np.float32)
    L = np.full((1, 50, 70), 85, np.int16)
    K = np.ones((1, 50, 70), bool)
    scan = dict(nx=4, ny=3, nt=2, xy_step=1024, theta_step=4, min_cells=0, min_mean=0)
    return dict(name="ties", occ=oc, scan=scan, L=L, K=K, points=[pts], poses=yaw_pose(pp, 0.0, 0.0, 0.0)[None], origins=[(-35, -25)])
