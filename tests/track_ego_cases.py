"""Shared by tests/test_track_ego_host.py, tests/test_gpu_track_ego.py and tools/gen_golden_track_ego.py: the unposed
sequences of tests/test_tracking_host.py (whose outputs, recorded from the tracker as it stood before it took poses, lie in
tests/golden/track_ego_unposed.npz), and the moving-sensor scene."""
import hashlib
import math

import numpy as np

DT = 1.0 / 30.0


def rows_to_dets(det_dtype, rows_per_stream, rows=None):
    """rows_per_stream: per stream a list of (x, y, z, score, label) -> (dets [S, rows], n [S])."""
    R = rows or max(1, max(len(r) for r in rows_per_stream))
    d = np.zeros((len(rows_per_stream), R), det_dtype)
    n = np.zeros(len(rows_per_stream), np.int32)
    for s, rr in enumerate(rows_per_stream):
        n[s] = len(rr)
        for i, (x, y, z, sc, lb) in enumerate(rr):
            d["box3d_lidar"][s, i] = [x, y, z, 0.6, 0.8, 1.7, 0.25]
            d["score"][s, i] = sc
            d["label"][s, i] = lb
    return d, n


# ---- the unposed sequences: name -> (config fields, streams, [(rows per stream, dt or None, flagged streams)]) ----
def unposed_cases():
    base = dict(gate=1.25, birth_score=0.3, max_misses=2, min_hits=2)
    cases = {}

    def walk(seed, dropout=()):
        rng = np.random.default_rng(seed)
        v = np.array([0.9, -0.4, 0.0])
        steps = []
        for i in range(60):
            pos = np.array([2.0, 1.0, -0.6]) + v * (i / 30.0) + rng.uniform(-0.02, 0.02, 3)
            steps.append(([[] if i in dropout else [(pos[0], pos[1], pos[2], 0.8, 0)]], None, ()))
        return steps

    for seed in range(3):
        cases[f"walk{seed}"] = ({}, 1, walk(seed))
    cases["dropout5"] = (dict(max_misses=5), 1, walk(3, range(30, 35)))
    cases["dropout4"] = (dict(max_misses=4), 1, walk(3, range(30, 35)))
    rng = np.random.default_rng(11)
    steps = []
    for i in range(60):
        a = np.array([2.0 + 0.9 * i / 30.0, 0.0, -0.6]) + rng.uniform(-0.02, 0.02, 3)
        b = np.array([3.8 - 0.9 * i / 30.0, 1.0, -0.6]) + rng.uniform(-0.02, 0.02, 3)
        rows = [(a[0], a[1], a[2], 0.8, 0), (b[0], b[1], b[2], 0.7, 0)]
        if i % 2:
            rows.reverse()
        steps.append(([rows], None, ()))
    cases["crossing"] = ({}, 1, steps)
    many = [(2.0 * i, 0.0, 0.0, 0.9, 0) for i in range(65)]
    cases["overflow"] = (base, 1, [([many], None, ()), ([many], None, ())])
    cases["reuse"] = (dict(base, max_misses=0), 1, [
        ([[(0.0, 0.0, 0.0, 0.9, 0), (5.0, 0.0, 0.0, 0.9, 0), (10.0, 0.0, 0.0, 0.9, 0)]], None, ()),
        ([[(5.0, 0.0, 0.0, 0.9, 0), (20.0, 0.0, 0.0, 0.9, 0), (30.0, 0.0, 0.0, 0.9, 0)]], None, ())])
    beyond = float(np.nextafter(np.float32(2.0), np.float32(3.0)))
    cases["gate"] = (base, 2, [
        ([[(2.0, 1.0, 0.0, 0.9, 0)], [(2.0, 1.0, 0.0, 0.9, 0)]], [1e-3, 1e-3], ()),
        ([[(2.75, 2.0, 0.0, 0.9, 0)], [(2.75, beyond, 0.0, 0.9, 0)]], [1e-3, 1e-3], ())])
    one = [[(1.0, 0.0, 0.0, 0.9, 0)], [(2.0, 0.0, 0.0, 0.9, 0)]]
    cases["flagged"] = (base, 2, [(one, None, ()), (one, None, (1,)), (one, None, ())])
    # signed zeros: a track born at -0.0 is output with the row's bits (the digest covers every step's output)
    zero = [[(-0.0, -0.0, -0.0, 0.9, 0)]]
    cases["negzero"] = (base, 1, [(zero, None, ())] * 3)
    return cases


def run_unposed(tracking, det_dtype, name, make=None, step=None):
    """The case through `tracking.Tracker` (or make(cfg, streams) / step(tracker, dets, n, dt)): the sha256 of every
    step's tracks() bytes, and the last step's arrays."""
    fields, streams, steps = unposed_cases()[name]
    cfg = tracking.TrackConfig(**fields)
    t = make(cfg, streams) if make else tracking.Tracker(cfg, streams)
    h = hashlib.sha256()
    out = None
    for rows, dt, flagged in steps:
        d, n = rows_to_dets(det_dtype, rows)
        for s in flagged:
            n[s] |= 1 << 30
        out = step(t, d, n, dt) if step else t.step(d, n, dt)
        for a in out:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest(), out


# ---- the moving-sensor scene ----
def rot_zyx(yaw, pitch, roll):
    cz, sz, cy, sy, cx, sx = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    return Rz @ Ry @ Rx


def ego_poses(steps=40, planar=True):
    """The sensor drives at 1.5 m/s along its heading, sways sideways by +-0.1 m at 1 Hz and yaws at 1 rad/s, 30 Hz; not
    planar: it also rolls and pitches by a few hundredths of a radian and heaves by a few cm.  -> [steps, 3, 4]."""
    out = np.zeros((steps, 3, 4), np.float64)
    x = y = 0.0
    for i in range(steps):
        t = i * DT
        yaw = 0.3 + 1.0 * t
        sway = 0.1 * math.sin(2.0 * math.pi * t)
        px, py = x - math.sin(yaw) * sway, y + math.cos(yaw) * sway
        if planar:
            c, s = math.cos(yaw), math.sin(yaw)
            out[i] = [[c, -s, 0.0, px], [s, c, 0.0, py], [0.0, 0.0, 1.0, 0.0]]
        else:
            out[i, :, :3] = rot_zyx(yaw, 0.03 * math.sin(5.0 * t), 0.04 * math.cos(3.0 * t))
            out[i, :, 3] = [px, py, 0.05 * math.sin(4.0 * t)]
        x += 1.5 * math.cos(yaw) * DT
        y += 1.5 * math.sin(yaw) * DT
    return out


def ego_objects(seed=20240917):
    """8 objects 4 .. 20 m from the origin, at least 2.5 m apart, heights within +-0.5 m: 6 static, 2 at a constant ground
    velocity.  -> (positions at t = 0 [8, 3], velocities [8, 3]) in the fixed frame."""
    rng = np.random.default_rng(seed)
    pos = []
    while len(pos) < 8:
        r, a = rng.uniform(4.0, 20.0), rng.uniform(-math.pi, math.pi)
        p = np.array([r * math.cos(a), r * math.sin(a), rng.uniform(-0.5, 0.5)])
        if all(np.hypot(*(p - q)[:2]) >= 2.5 for q in pos):
            pos.append(p)
    vel = np.zeros((8, 3))
    vel[6] = [0.8, -0.5, 0.0]
    vel[7] = [-1.0, 0.3, 0.0]
    return np.array(pos), vel


def ego_scene(det_dtype, steps=40, planar=True, rows=16):
    """-> (poses [steps, 3, 4], [(dets [1, rows], n [1]) per step], positions, velocities): the detections are the
    float32 sensor-frame centres R^T (p - t) of the objects, in object order."""
    poses = ego_poses(steps, planar)
    pos, vel = ego_objects()
    frames = []
    for i in range(steps):
        R, t = poses[i, :, :3], poses[i, :, 3]
        local = (pos + vel * (i * DT) - t) @ R          # rows: R^T (p - t)
        frames.append(rows_to_dets(det_dtype, [[(p[0], p[1], p[2], 0.9, 0) for p in local]], rows))
    return poses, frames, pos, vel
