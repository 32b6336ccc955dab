"""Inputs shared by tests/test_ground_host.py and tests/test_gpu_ground.py: explicit triples that name given rows, the
dyadic boundary rows, seeded tilted floors with boxes, the scene under a sensor pitched 5 degrees, and small frames for a
handle.  Everything is generated from seeds; nothing here touches a GPU."""
import math

import numpy as np

ROWS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1025)      # 1025: one row past a tile of k_ground_score (1024)
HYPS = (1, 63, 64, 65, 512)                               # 512: PP_GROUND_MAX_HYP


def triple_for(rows, n):
    """uint32 [3]: entries u with (u * n) >> 32 == rows[q] -- the least such u, ceil(row * 2^32 / n)."""
    out = []
    for j in rows:
        u = -((-int(j) << 32) // int(n))
        assert 0 <= u < 2 ** 32 and (u * n) >> 32 == j
        out.append(u)
    return np.array(out, np.uint32)


def triples_for(rows_per_hyp, n):
    return np.stack([triple_for(r, n) for r in rows_per_hyp])


# ---- degenerate hypotheses, ties, fallback: a small hand-made frame ----
FIXED_CFG = dict(hypotheses=6, max_range=20.0, cand_z_max=1.0, max_slope=0.5, h_min=0.5, h_max=2.0, inlier_dist=0.125, min_inliers=4,
                 refine=0, ground_dist=0.125, overhead_max=2.0, fallback_c=-1.25)


def fixed_frame():
    """(rows float32 [n, 3], names): a floor z = 0.25 x - 1 on a 4 x 3 lattice (rows 0 .. 11), three collinear floor rows
    among them (0, 1, 2: y = 0, x = 0, 1, 2), a wall (12 .. 14: x = 3, z rising), a ceiling patch (15 .. 17: z = 0.75, a
    level plane 0.75 ABOVE the sensor, so -c < h_min), and a NaN row (18)."""
    rows = [(float(x), float(y), 0.25 * x - 1.0) for y in (0, 1, 2) for x in (0, 1, 2, 3)]
    rows += [(3.0, 0.0, -0.25), (3.0, 1.0, 0.5), (3.0625, 0.0, 0.75)]          # a wall: nearly vertical
    rows += [(0.0, 0.0, 0.75), (1.0, 0.0, 0.75), (0.0, 1.0, 0.75)]             # a ceiling
    rows += [(np.nan, 0.0, -1.0)]
    return np.array(rows, np.float32)


FIXED_TRIPLES = dict(floor=(0, 1, 4), collinear=(0, 1, 2), wall=(12, 13, 14), ceiling=(15, 16, 17), nan=(0, 4, 18), floor2=(5, 6, 9))


# ---- the boundary, dyadic numbers: plane z = 0.25 x - 1, inlier_dist = ground_dist = 0.125 ----
def boundary_frame():
    """(rows float32 [n, 3], ground bool [n], triples uint32 [1, 3]): three rows ON the plane carry the hypothesis; then
    rows whose residual is exactly +-0.125 (inliers / GROUND) and rows at the next float32 beyond it (neither; a float32
    row cannot lie one float64 step beyond -- BOUNDARY_CFG_BELOW moves the threshold by that step instead).  Every product
    and sum of the residual is exact in float64 for these values, so the boundary is the rule's own."""
    f = np.float32
    up, dn = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    rows = [(f(0), f(0), f(-1.0), True), (f(4), f(0), f(0.0), True), (f(0), f(2), f(-1.0), True)]
    for x, y in ((1.0, 0.5), (2.0, -1.0), (3.0, 1.5)):
        z = 0.25 * x - 1.0
        rows += [(f(x), f(y), f(z + 0.125), True), (f(x), f(y), up(z + 0.125), False),
                 (f(x), f(y), f(z - 0.125), True), (f(x), f(y), dn(z - 0.125), False)]
    p = np.array([r[:3] for r in rows], np.float32)
    return p, np.array([r[3] for r in rows], bool), triples_for([(0, 1, 2)], len(p))


BOUNDARY_CFG = dict(FIXED_CFG, hypotheses=1, min_inliers=3)
# Rows are float32, so the row next to a residual of exactly 0.125 lies a float32 step away, 2^29 doubles: that pair alone
# cannot tell a float64 comparison from a float32 one.  This configuration does: both thresholds are the next float64
# BELOW 0.125, so a row at a residual of exactly 0.125 is no inlier and not GROUND -- while a comparison in float32, or a
# threshold passed through float32, would round it back to 0.125 and take the row.
BOUNDARY_CFG_BELOW = dict(BOUNDARY_CFG, inlier_dist=float(np.nextafter(0.125, 0.0)), ground_dist=float(np.nextafter(0.125, 0.0)))


def boundary_on_plane(rows):
    """bool [n]: the rows of boundary_frame that lie ON z = 0.25 x - 1 (the three that carry the hypothesis): all that
    BOUNDARY_CFG_BELOW leaves as inliers and GROUND."""
    p = rows.astype(np.float64)
    return p[:, 2] == 0.25 * p[:, 0] - 1.0


# ---- seeded tilted floors with boxes (the recovery scenes) ----
RECOVERY_SEEDS = tuple(range(12))
RECOVERY_K = 64              # the K the recovery test was fixed at (tests/test_ground_host.py records how it was chosen)
RECOVERY_CFG = dict(hypotheses=RECOVERY_K, max_range=20.0, cand_z_max=1.5, max_slope=0.3, h_min=0.2, h_max=3.0, inlier_dist=0.03,
                    min_inliers=50, refine=1, ground_dist=0.05, overhead_max=2.5, fallback_c=-1.0)


def floor_scene(seed, n=600, F=4, max_pitch=8.0, max_roll=4.0):
    """(rows float32 [n, F], is_floor bool [n], plane (a, b, c)): 70 % of the rows on a floor patch pitched up to
    max_pitch and rolled up to max_roll degrees under a sensor 0.3 .. 1.2 m high, uniform noise of +-0.01 m on it; 30 % on
    boxes 0.15 .. 0.9 m above the floor.  The rows are shuffled."""
    rng = np.random.default_rng(9100 + seed)
    a = math.tan(math.radians(rng.uniform(-max_pitch, max_pitch)))
    b = math.tan(math.radians(rng.uniform(-max_roll, max_roll)))
    c = -rng.uniform(0.3, 1.2)
    nf = n - (n * 3) // 10
    x, y = rng.uniform(0.4, 6.0, n), rng.uniform(-2.5, 2.5, n)
    z = a * x + b * y + c
    is_floor = np.arange(n) < nf
    z = z + np.where(is_floor, rng.uniform(-0.01, 0.01, n), rng.uniform(0.16, 0.9, n))
    order = rng.permutation(n)
    p = np.zeros((n, F), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = x[order], y[order], z[order]
    if F > 3:
        p[:, 3:] = rng.random((n, F - 3))
    return p, is_floor[order], (a, b, c)


# ---- the point of the feature: a flat floor and one box, seen by a sensor pitched 5 degrees ----
PITCH = math.radians(5.0)
SENSOR_H = 0.5
PITCH_FRAMES = 10
PITCH_OCC = dict(resolution=0.1, width=200, height=100, z_min=-0.4, z_max=1.0, max_range=50.0)
PITCH_CFG = dict(hypotheses=32, seed=5, max_range=50.0, cand_z_max=1.5, max_slope=0.3, h_min=0.2, h_max=2.0, inlier_dist=0.03,
                 min_inliers=100, refine=1, ground_dist=0.05, overhead_max=2.0, fallback_c=-SENSOR_H)
PITCH_COSTMAP = dict(x_min=0.0, y_min=-3.0, resolution=0.1, width=100, height=60, z_min=-0.4, z_max=1.0, objects=0, min_points=1)


def pitch_scene():
    """(floor [n, 3], box [m, 3]) float64 in the FIXED frame, every point at the centre of a 0.1 m cell: a floor z = 0
    over x 0.55 .. 7.95, y -1.95 .. 1.95, and the face of a box at x = 5.05, y -0.25 .. 0.25, z 0.15 .. 0.8."""
    fx, fy = np.meshgrid(np.arange(75) * 0.1 + 0.55, np.arange(40) * 0.1 - 1.95)
    floor = np.stack([fx.ravel(), fy.ravel(), np.zeros(fx.size)], 1)
    by, bz = np.meshgrid(np.arange(6) * 0.1 - 0.25, np.arange(14) * 0.05 + 0.15)
    box = np.stack([np.full(by.size, 5.05), by.ravel(), bz.ravel()], 1)
    return floor, box


def pitch_pose(k, pitched):
    """float64 [3, 4]: the sensor-to-fixed transform of frame k -- SENSOR_H over the floor, 0.1 m further along x each
    frame, nose down by PITCH when `pitched`."""
    th = PITCH if pitched else 0.0
    c, s = math.cos(th), math.sin(th)
    return np.array([[c, 0.0, s, 0.1 * k], [0.0, 1.0, 0.0, 0.0], [-s, 0.0, c, SENSOR_H]])


def pitch_frame(k, pitched):
    """(rows float32 [n + m, 3] in the sensor frame, is_box bool, pose)."""
    floor, box = pitch_scene()
    P = pitch_pose(k, pitched)
    pts = np.concatenate([floor, box])
    rows = (pts - P[:, 3]) @ P[:, :3]                      # R^T (p - t)
    return rows.astype(np.float32), np.arange(len(pts)) >= len(floor), P


# ---- frames for a handle: a tilted floor with boxes in the tiny range of tests/object_mask_cases.py's cycles ----
CYCLE_GROUND = dict(hypotheses=48, seed=11, max_range=20.0, cand_z_max=1.0, max_slope=0.3, h_min=0.1, h_max=2.0, inlier_dist=0.03,
                    min_inliers=20, refine=1, ground_dist=0.05, overhead_max=1.0, fallback_c=-0.3,
                    consumers=("occupancy", "scan_match", "costmap"))


def cycle_frame(rng, n, F=4):
    """n rows over x 0.05 .. 1.55, y -0.6 .. 0.6: 60 % on a floor tilted by up to 5 degrees 0.3 m under the sensor, the rest
    up to 0.9 m above it -- hits for the occupancy map, scan cells, and counts of the costmap."""
    a, b = (math.tan(math.radians(v)) for v in rng.uniform(-5.0, 5.0, 2))
    x, y = rng.uniform(0.05, 1.55, n), rng.uniform(-0.6, 0.6, n)
    z = a * x + b * y - 0.3 + np.where(rng.random(n) < 0.6, rng.uniform(-0.01, 0.01, n), rng.uniform(0.07, 0.9, n))
    p = np.stack([x, y, z] + [rng.random(n)] * (F - 3), 1)
    return np.ascontiguousarray(p.astype(np.float32))


def cycle_frames(seed, rows, F=4):
    rng = np.random.default_rng(seed)
    return [cycle_frame(rng, n, F) for n in rows]
