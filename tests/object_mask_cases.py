"""Inputs shared by tests/test_object_mask_host.py and tests/test_gpu_object_mask.py: seeded rows and rectangles, the
yaw-0 boundary rows, a tracker with posed steps, and the room a square object crosses.  Everything is generated from
seeds; nothing here touches a GPU."""
import math

import numpy as np

MARGIN = 1e-9            # metres: object_mask.MARGIN
UNDECIDED_CAP = 0.001    # the share of rows a comparison behind a real pass may leave out (tests/nav_cycle_cases.py)
ROWS = (0, 1, 63, 64, 65, 257)
FOOTPRINTS = (0, 1, 63, 64, 65, 128)
SEEDS = tuple(range(6))


# ---- seeded rows against seeded rectangles ----
def seeded_rows(rng, n, F=4, span=4.0):
    """n float32 rows over [-span, span]^2; among them a NaN, an infinity and a huge value where there is room."""
    p = rng.uniform(-span, span, (n, F)).astype(np.float32)
    for k, v in enumerate((np.nan, np.inf, 1e30)):
        if n > 8 + k:
            p[5 + k, k % 2] = v
    return p


def seeded_rects(rng, k, span=4.0):
    """k rows x y w l yaw, float64; among them a non-finite field each where there is room (they cover nothing)."""
    r = np.stack([rng.uniform(-span, span, k), rng.uniform(-span, span, k), rng.uniform(0.2, 1.8, k), rng.uniform(0.2, 1.8, k),
                  rng.uniform(-math.pi, math.pi, k)], axis=1)
    if k > 4:
        r[1, 4] = np.nan
        r[2, 2] = np.inf
        r[3, 0] = -np.inf
    return r


def seeded_case(seed):
    """(frames: three unequal frames so that a frame's rows do not start on a 64-row boundary of the buffer, rects per
    frame, pad).  The sizes walk through ROWS and FOOTPRINTS with the seed."""
    rng = np.random.default_rng(4100 + seed)
    n = [ROWS[(seed + j * 2 + 3) % len(ROWS)] for j in range(3)]
    n[seed % 3] = 257
    k = [FOOTPRINTS[(seed + j * 2 + 1) % len(FOOTPRINTS)] for j in range(3)]
    k[(seed + 1) % 3] = 128 if seed % 2 else 65
    frames = [seeded_rows(rng, a) for a in n]
    rects = [seeded_rects(rng, b) for b in k]
    return frames, rects, (0.0, 0.07)[seed % 2]


def size_cases():
    """(rows, footprints) pairs that cover every value of ROWS and of FOOTPRINTS."""
    return [(r, FOOTPRINTS[(i + 2) % len(FOOTPRINTS)]) for i, r in enumerate(ROWS)] + [(257, 0), (257, 128), (64, 64), (0, 0)]


# ---- the boundary, yaw 0, float32-exact coordinates ----
BOUNDARY_RECT = np.array([[1.0, 2.0, 1.0, 0.5, 0.0]])       # centre (1, 2), hx = 0.5, hy = 0.25: all exact in float32


def boundary_rows():
    """(rows float32 [n, 3], inside bool [n]): a row at exactly hx (hy) from the centre is inside, the next float32
    beyond it is outside; on all four edges."""
    f = np.float32
    up, dn = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    rows = [(f(1.5), f(2.0), True), (up(1.5), f(2.0), False), (f(0.5), f(2.0), True), (dn(0.5), f(2.0), False),
            (f(1.0), f(2.25), True), (f(1.0), up(2.25), False), (f(1.0), f(1.75), True), (f(1.0), dn(1.75), False),
            (f(1.5), f(2.25), True), (up(1.5), f(2.25), False), (f(1.0), f(2.0), True), (f(3.0), f(2.0), False)]
    p = np.array([(x, y, 0.0) for x, y, _ in rows], np.float32)
    return p, np.array([r[2] for r in rows], bool)


# ---- a tracker whose streams have had posed steps ----
TRACK = dict(gate=1.25, birth_score=0.3, max_misses=50, min_hits=2, q_acc=4.0, r_pos=0.01)
TRACK_STREAMS = 2


def det_rows(pp, per_stream, rows=8):
    """per_stream: per stream a list of (x, y, w, l, yaw, score) -> (dets [streams, rows], n)."""
    d = np.zeros((len(per_stream), rows), pp.Engine.det_dtype())
    n = np.zeros(len(per_stream), np.int32)
    for s, rr in enumerate(per_stream):
        n[s] = len(rr)
        for i, r in enumerate(rr):
            d["box3d_lidar"][s, i] = (r[0], r[1], 0.3, r[2], r[3], 1.6, r[4])
            d["score"][s, i] = r[5]
    return d, n


def track_steps(pp):
    """[(dets, n, dt, poses or None)]: three steps of two streams.  Stream 0 has three objects -- one walking (over the
    speed boundary), one standing, one seen at the last step only (not confirmed) -- and stream 1 one walking object;
    the last two steps carry poses, so that both streams hold a previous pose."""
    P = pp.sweeps.pose_from_xyyaw
    steps = []
    for k in range(3):
        per = [[(0.6 + 0.1 * k, 0.2 - 0.05 * k, 0.5, 0.8, 0.3, 0.9), (-1.0, 1.0, 0.6, 0.6, -0.7, 0.9)],
               [(1.5 - 0.08 * k, -0.4 + 0.02 * k, 0.45, 0.7, 2.0, 0.8)]]
        if k == 2:
            per[0].append((2.5, -1.5, 0.4, 0.4, 1.1, 0.9))
        poses = None if k == 0 else np.stack([P(0.05 * k, 0.02 * k, 0.03 * k), P(-0.04 * k, 0.0, -0.02 * k)])
        steps.append(det_rows(pp, per) + ([0.1] * TRACK_STREAMS, poses))
    return steps


def peek_pose(pp):
    """The poses and dt a mask in front of the next frame's pass would be given."""
    P = pp.sweeps.pose_from_xyyaw
    return np.stack([P(0.17, 0.05, 0.11), P(-0.13, 0.02, -0.07)]), np.array([0.1, 0.05])


# ---- the room a square object crosses (the sketch of the issue, with the real functions) ----
ROOM_HALF = 5.0          # a 10 m square room around the sensor
ROOM_OCC = dict(resolution=0.1, width=120, height=120, z_min=-0.5, z_max=1.0, max_range=20.0)
ROOM_RAYS = 1440
ROOM_FRAMES = 40
ROOM_OBJECT = 0.6        # side of the square object, 3 m in front of the sensor
ROOM_PAD = 0.05          # the returns lie ON the object's faces: the pad takes them inside by more than any rounding
ROOM_INNER = 0.4         # an inner cell lies this far from every wall
ROOM_COST = 65


def room_object_centre(k):
    return 3.0, -2.0 + 4.0 * k / (ROOM_FRAMES - 1)


def room_frame(k):
    """(rows float32 [ROOM_RAYS, 3], rect [1, 5]) of frame k: every ray ends on the nearer of the walls and the object."""
    ox, oy = room_object_centre(k)
    h = ROOM_OBJECT / 2.0
    a = np.arange(ROOM_RAYS) * (2.0 * math.pi / ROOM_RAYS)
    dx, dy = np.cos(a), np.sin(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_wall = np.minimum(np.where(dx != 0, ROOM_HALF / np.abs(dx), np.inf), np.where(dy != 0, ROOM_HALF / np.abs(dy), np.inf))
        # the slab test against the object's square
        tx0, tx1 = (ox - h) / dx, (ox + h) / dx
        ty0, ty1 = (oy - h) / dy, (oy + h) / dy
        tmin = np.maximum(np.minimum(tx0, tx1), np.minimum(ty0, ty1))
        tmax = np.minimum(np.maximum(tx0, tx1), np.maximum(ty0, ty1))
    hit = (tmax >= tmin) & (tmin > 0)
    t = np.where(hit, np.minimum(tmin, t_wall), t_wall)
    rows = np.stack([t * dx, t * dy, np.zeros_like(t)], axis=1).astype(np.float32)
    return rows, np.array([[ox, oy, ROOM_OBJECT, ROOM_OBJECT, 0.0]])


def room_regions(pp):
    """(inner bool [H, W]: cells whose centre lies ROOM_INNER or more from every wall; wall = ~inner)."""
    c = pp.occupancy.OccupancyConfig(**ROOM_OCC)
    cx = (np.arange(c.width) - c.width // 2 + 0.5) * c.resolution
    cy = (np.arange(c.height) - c.height // 2 + 0.5) * c.resolution
    lim = ROOM_HALF - ROOM_INNER
    return (np.abs(cx)[None, :] <= lim) & (np.abs(cy)[:, None] <= lim)


# ---- cycles on a handle: hand-fed track rows at yaw 0, rows around them ----
CYCLE_STREAMS = 3
CYCLE_ROWS = (257, 300, 65)      # unequal, and no frame but the first starts on a 64-row boundary of the buffer
CYCLE_F = 4
CYCLE_TRACK = dict(gate=1.25, birth_score=0.3, max_misses=2, min_hits=2, q_acc=4.0, r_pos=0.01)
CYCLE_OCC = dict(resolution=0.1, z_min=0.0, z_max=1.0, max_range=2.5, width=37, height=29)
CYCLE_SCAN = dict(nx=2, ny=2, nt=2, xy_step=1024, theta_step=8, min_cells=5, min_mean=0)
CYCLE_COSTMAP = dict(x_min=-0.5, y_min=-1.0, resolution=0.05, width=51, height=43, z_min=-1.0, z_max=1.0, objects="tracks")
CYCLE_MASK = dict(objects="tracks", pad=0.03, consumers=("occupancy", "scan_match", "costmap"))


def cycle_frame(rng, n):
    """n rows over the tiny range, two thirds of them in the occupancy map's hit band."""
    p = np.stack([rng.uniform(0.05, 1.55, n), rng.uniform(-0.6, 0.6, n), rng.uniform(-0.5, 0.9, n), rng.random(n)], 1)
    return np.ascontiguousarray(p.astype(np.float32))


def cycles(pp, count=3, seed=23):
    """[dict(frames, poses, dt, dets, n)]: per stream two objects at yaw 0 that walk a few centimetres a cycle (the first
    of stream 2 stands still), a slow planar ego motion, 0.1 s between cycles."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        frames = [cycle_frame(rng, n) for n in CYCLE_ROWS]
        poses = np.stack([pp.sweeps.pose_from_xyyaw(0.03 * i, (-0.02, 0.0, 0.025)[b] * i, 0.02 * i * (b + 1)) for b in range(CYCLE_STREAMS)])
        per = [[(0.45 + 0.04 * i, -0.25 + 0.02 * i, 0.4, 0.5, 0.0, 0.9), (1.1 - 0.03 * i, 0.3, 0.35, 0.45, 0.0, 0.8)],
               [(0.8, 0.1 - 0.05 * i, 0.5, 0.4, 0.0, 0.9), (1.3, -0.4 + 0.03 * i, 0.3, 0.3, 0.0, 0.7)],
               [(0.6, 0.0, 0.45, 0.45, 0.0, 0.9), (1.2 - 0.05 * i, -0.3 + 0.04 * i, 0.4, 0.6, 0.0, 0.9)]]
        dets, n = det_rows(pp, per)
        out.append(dict(frames=frames, poses=poses, dt=np.full(CYCLE_STREAMS, 0.1), dets=dets, n=n))
    return out
