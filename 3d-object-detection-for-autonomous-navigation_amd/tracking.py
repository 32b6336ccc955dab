"""Tracking across frames: identities and velocities for the detections of a live feed.

The reference republishes its boxes every frame and keeps nothing (train.py:810-828); it has no tracker, so nothing here
is parity with it.  This module STATES the rule: `Tracker` is the numpy restatement that the GPU step (csrc/track.hip,
k_track_step, behind the detector's post-process: Engine.set_tracking) mirrors operation for operation and equals bit for
bit.  All arithmetic is float64 with + - * / and comparisons only -- no sqrt, nothing transcendental -- and the order of
every operation below is part of the rule.

One track table per STREAM (frame b of every pass is stream b), PP_TRACK_MAX slots each.  A step, per stream:

1. predict every live track by dt: x += vx * dt (y, z alike); P <- F P F' + Q with F = [[1, dt], [0, 1]] and the discrete
   white-acceleration Q = q_acc * [[dt^4 / 4, dt^3 / 2], [dt^3 / 2, dt^2]].  The three axes share q_acc, r_pos, p0 and dt,
   so their covariances are equal and one triple (p00, p01, p11) is kept;
2. associate: a (track, row) pair is admissible when its BEV squared distance d2 = dx * dx + dy * dy satisfies
   d2 <= gate * gate (inclusive) and, class_aware, the labels are equal; repeatedly the admissible pair of a still-free
   track and a still-free row with the smallest (d2, slot, row) is matched;
3. update each matched track per axis with the scalar-gain Kalman update (k0 = p00 / (p00 + r_pos), k1 = p01 / (p00 + r_pos));
   sizes are blended by size_alpha; yaw, score and label are the row's; hits += 1, misses = 0; confirmed at min_hits hits;
4. age the unmatched: misses += 1, freed when misses > max_misses;
5. births: each unmatched row with score >= birth_score, in row order, opens a track in the lowest free slot (slots freed
   in 4 included) with id = next_id++; no slot left: the row is dropped and `overflow` counts it;
6. output the live tracks in ascending slot order, `det_row` = the matched or birth row, else -1.

A frame whose count carries the post-process's non-finite flag leaves its stream untouched.

EGO MOTION.  The tracks of a stream stay in the sensor frame of its latest step, so `det_row`, the association and the
output keep their meaning while the sensor moves.  A step may be given a POSE per stream (sweeps.py's [3, 4] float64
sensor-to-fixed [R | t]); per stream the tracker keeps prev_pose, prev_psi and has_prev.  A step of stream b with pose P_c:

0. psi_c = math.atan2(P_c[1][0], P_c[0][0]) -- on the host (std::atan2 in the C library); the device only adds and
   subtracts it.  If has_prev: (M, u) = sweeps.relative_transform(P_c, prev_pose), and every live slot is CARRIED from the
   previous posed sensor frame into the current one before stage 1:
       x' = ((M00 * x + M01 * y) + M02 * z) + u0          (y', z' alike, all from the old x y z)
       vx' = (M00 * vx + M01 * vy) + M02 * vz             (vy', vz' alike)
       yaw' = yaw + (psi_c - prev_psi)                    (no wrap)
   The covariance triple is isotropic: a rotation leaves it as it is.
   Then stages 1 to 6, unchanged; at the end prev_pose = P_c, prev_psi = psi_c, has_prev = True.

A step WITHOUT a pose for the stream is stages 1 to 6 alone and leaves prev_* untouched: no carry runs, not even with an
identity (((1 * x + 0 * y) + 0 * z) + 0 would turn -0.0 into +0.0).  A flagged frame leaves table and prev_* untouched and
spends the pose, as it spends dt: the next posed step carries over the whole motion since the last step that ran.
reset(stream) forgets the previous pose; a stream's first posed step carries nothing.  After a carry a track's velocity is
the object's velocity over ground, in the current sensor axes.

The same step also gives the live tracks in the FIXED frame (tracks_fixed), for the streams it had a pose for: position
((R00 * x + R01 * y) + R02 * z) + t0 (y, z alike), velocity (R00 * vx + R01 * vy) + R02 * vz (alike), yaw + psi_c, every
other field copied; a stream whose step had no pose reports a count of -1 there.
"""
import dataclasses
import math

import numpy as np

from . import sweeps as _swp
from ._lib import PP_TRACK_MAX, PP_TRACK_MASK_ROWS as MAX_ROWS      # slots per stream; rows per frame the GPU step takes

_NONFINITE = 1 << 30            # PP_NDETS_NONFINITE

TRACK_DTYPE = np.dtype([("state", "<f8", (6,)), ("size", "<f8", (3,)), ("yaw", "<f8"), ("score", "<f4"), ("id", "<i4"),
                        ("label", "<i4"), ("hits", "<i4"), ("misses", "<i4"), ("confirmed", "<i4"), ("det_row", "<i4"),
                        ("reserved", "<i4")])       # pp_track (include/pp_hip.h), 112 bytes
assert TRACK_DTYPE.itemsize == 112


@dataclasses.dataclass
class TrackConfig:
    """The shipped pedestrian setup (a 30 Hz depth camera, 0.16 m pillars, people at walking pace):

    period       1/30 s  the camera's frame time: what a stream advances by when no time stamps are given
    gate         0.6 m   a pedestrian moves 5 cm per frame at 1.5 m/s and the detector's centres jitter by a few cm; 0.6 m
                         is the shoulder width that the stand-up NMS already treats as "the same object", so a detection
                         that survived NMS beside another is never inside the other's gate by much
    q_acc        4.0     (m/s^2)^2: people start and stop with about 2 m/s^2
    r_pos        0.01    m^2: a centre is good to about a tenth of a metre (under one pillar)
    p0_pos       0.01    m^2: a new track stands where its detection was, to r_pos
    p0_vel       4.0     (m/s)^2: a new track may already be walking (2 m/s), so the first updates learn the velocity fast
    size_alpha   0.3     sizes barely change; a slow blend takes the flicker out
    birth_score  0.3     the production score filter (anno.py / train.py:815): what is not published opens no track
    max_misses   5       a sixth of a second of missed detections is bridged by prediction, then the track is dropped
    min_hits     3       a track is `confirmed` at its third detection: one-frame false positives never are
    class_aware  True    a pedestrian never continues a cyclist's track
    """
    gate: float = 0.6
    q_acc: float = 4.0
    r_pos: float = 0.01
    p0_pos: float = 0.01
    p0_vel: float = 4.0
    size_alpha: float = 0.3
    birth_score: float = 0.3
    period: float = 1.0 / 30.0
    max_misses: int = 5
    min_hits: int = 3
    class_aware: bool = True

    def __post_init__(self):
        for f in ("gate", "q_acc", "r_pos", "p0_pos", "p0_vel", "size_alpha", "birth_score", "period"):
            try:
                v = float(getattr(self, f))
            except (TypeError, ValueError):
                raise ValueError(f"TrackConfig: {f} must be a number, got {getattr(self, f)!r}")
            if not math.isfinite(v):
                raise ValueError(f"TrackConfig: {f} is not finite")
            if f not in ("size_alpha", "birth_score") and not v > 0.0:
                raise ValueError(f"TrackConfig: {f} = {v} must be > 0")
            setattr(self, f, v)
        if not 0.0 <= self.size_alpha <= 1.0:
            raise ValueError(f"TrackConfig: size_alpha = {self.size_alpha} outside [0, 1]")
        for f, lo in (("max_misses", 0), ("min_hits", 1)):
            v = getattr(self, f)
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"TrackConfig: {f} must be an integer, got {v!r}")
            if int(v) < lo:
                raise ValueError(f"TrackConfig: {f} = {v} must be >= {lo}")
            setattr(self, f, int(v))
        self.class_aware = bool(self.class_aware)

    def to_dict(self):
        return dataclasses.asdict(self)

    @classmethod
    def from_any(cls, cfg):
        """A TrackConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"tracking: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"tracking: a TrackConfig, a dict of its fields or True, got {cfg!r}")


def stamps_to_dt(last, stamps, batch, period):
    """Per-stream dt from time stamps: stamps[b] - last[b], or `period` for a stream without an earlier stamp (NaN in
    `last`).  Raises ValueError, naming the stream, for a stamp that is not finite or does not increase.  Returns
    (dt, new_last); `last` itself is not changed."""
    s = np.asarray(stamps, np.float64).reshape(-1)
    if s.shape[0] != batch:
        raise ValueError(f"stamps: {s.shape[0]} values for {batch} frames")
    new = np.array(last, np.float64)
    dt = np.empty(batch, np.float64)
    for b in range(batch):
        if not math.isfinite(s[b]):
            raise ValueError(f"stamps: the stamp of stream {b} is not finite")
        if math.isnan(new[b]):
            dt[b] = period
        else:
            if not s[b] > new[b]:
                raise ValueError(f"stamps: the stamp of stream {b} does not increase ({s[b]!r} after {new[b]!r})")
            dt[b] = s[b] - new[b]
        new[b] = s[b]
    return dt, new


class Tracker:
    """The rule, on the host: `streams` track tables with the state of the GPU step.  step(dets, n, dt) advances streams
    0 .. len(n) - 1; tracks() returns what pp_get_tracks returns for them, tracks_fixed() what pp_get_tracks_fixed does."""

    def __init__(self, config=None, streams=1):
        self.cfg = TrackConfig.from_any(config if config is not None else True)
        S, M = int(streams), PP_TRACK_MAX
        self.streams = S
        self.x = np.zeros((S, M, 6), np.float64)
        self.p = np.zeros((S, M, 3), np.float64)
        self.size = np.zeros((S, M, 3), np.float64)
        self.yaw = np.zeros((S, M), np.float64)
        self.score = np.zeros((S, M), np.float32)
        self.id = np.zeros((S, M), np.int32)
        self.label = np.zeros((S, M), np.int32)
        self.hits = np.zeros((S, M), np.int32)
        self.misses = np.zeros((S, M), np.int32)
        self.confirmed = np.zeros((S, M), np.int32)
        self.live = np.zeros((S, M), bool)
        self.next_id = np.ones(S, np.int32)
        self.overflow = np.zeros(S, np.int32)
        self._out = np.zeros((S, M), TRACK_DTYPE)
        self._nout = np.zeros(S, np.int32)
        self._batch = 0
        self.prev_pose = np.zeros((S, 3, 4), np.float64)
        self.prev_psi = np.zeros(S, np.float64)
        self.has_prev = np.zeros(S, bool)
        self._outf = np.zeros((S, M), TRACK_DTYPE)
        self._noutf = np.full(S, -1, np.int32)

    def reset(self, stream=None):
        for s in (range(self.streams) if stream is None or stream < 0 else [int(stream)]):
            self.live[s] = False
            self.next_id[s] = 1
            self.overflow[s] = 0
            self.has_prev[s] = False

    # ---- the pieces of a step (float64 scalars; the order of the operations is the rule) ----
    @staticmethod
    def predict_axis(x, v, dt):
        return x + v * dt

    @staticmethod
    def predict_cov(p00, p01, p11, dt, q_acc):
        dt2 = dt * dt
        a = p01 + dt * p11
        n00 = (p00 + dt * p01) + dt * a
        return n00 + q_acc * (dt2 * dt2 * 0.25), a + q_acc * (dt2 * dt * 0.5), p11 + q_acc * dt2

    @staticmethod
    def gains(p00, p01, r_pos):
        s = p00 + r_pos
        return p00 / s, p01 / s

    @staticmethod
    def update_axis(x, v, z, k0, k1):
        y = z - x
        return x + k0 * y, v + k1 * y

    @staticmethod
    def update_cov(p00, p01, p11, k0, k1):
        omk = 1.0 - k0
        return omk * p00, omk * p01, p11 - k1 * p01

    @staticmethod
    def associate(tx, ty, tlabel, tlive, dx, dy, dlabel, gate, class_aware):
        """Greedy matching by the global minimum of (d2, slot, row).  tx, ty, tlabel, tlive: [M] predicted tracks; dx, dy,
        dlabel: [n] rows (float64 centres).  Returns match [M]: the row of each track, or -1."""
        M, n = len(tx), len(dx)
        match = np.full(M, -1, np.int64)
        if n == 0 or not np.any(tlive):
            return match
        ex = tx[:, None] - dx[None, :]
        ey = ty[:, None] - dy[None, :]
        d2 = ex * ex + ey * ey
        ok = (d2 <= gate * gate) & tlive[:, None]
        if class_aware:
            ok &= tlabel[:, None] == dlabel[None, :]
        d2 = np.where(ok, d2, np.inf)
        while True:
            k = int(np.argmin(d2))          # the first minimum in row-major order: the lowest slot, then the lowest row
            s, r = divmod(k, n)
            if not np.isfinite(d2[s, r]):
                return match
            match[s] = r
            d2[s, :] = np.inf
            d2[:, r] = np.inf

    def _carry(self, s, pose, psi):
        """Stage 0: the live slots of stream s from the previous posed sensor frame into the frame of `pose`."""
        M, u = _swp.relative_transform(pose, self.prev_pose[s])
        dpsi = np.float64(psi) - self.prev_psi[s]
        x = self.x[s]
        for k in np.nonzero(self.live[s])[0]:
            px, py, pz, vx, vy, vz = x[k]
            for i in range(3):
                x[k, i] = ((M[i, 0] * px + M[i, 1] * py) + M[i, 2] * pz) + u[i]
                x[k, 3 + i] = (M[i, 0] * vx + M[i, 1] * vy) + M[i, 2] * vz
            self.yaw[s, k] = self.yaw[s, k] + dpsi

    def _fixed_out(self, s, pose, psi):
        """The rows of _out[s] in the fixed frame of `pose`."""
        m = int(self._nout[s])
        o = self._outf[s]
        o[:] = self._out[s]
        st = self._out[s]["state"]
        for k in range(m):
            px, py, pz, vx, vy, vz = st[k]
            for i in range(3):
                o["state"][k, i] = ((pose[i, 0] * px + pose[i, 1] * py) + pose[i, 2] * pz) + pose[i, 3]
                o["state"][k, 3 + i] = (pose[i, 0] * vx + pose[i, 1] * vy) + pose[i, 2] * vz
            o["yaw"][k] = self._out[s]["yaw"][k] + np.float64(psi)
        self._noutf[s] = m

    def _step_stream(self, s, dets, n, dt, pose=None):
        c = self.cfg
        M = PP_TRACK_MAX
        x, p, live = self.x[s], self.p[s], self.live[s]
        dt = np.float64(dt)
        psi = None
        if pose is not None:
            psi = math.atan2(float(pose[1, 0]), float(pose[0, 0]))
            if self.has_prev[s]:
                self._carry(s, pose, psi)
        for k in np.nonzero(live)[0]:
            for q in range(3):
                x[k, q] = self.predict_axis(x[k, q], x[k, q + 3], dt)
            p[k] = self.predict_cov(p[k, 0], p[k, 1], p[k, 2], dt, np.float64(c.q_acc))
        box = dets["box3d_lidar"][:n].astype(np.float64)      # float32 -> float64, exact
        match = self.associate(x[:, 0], x[:, 1], self.label[s], live, box[:, 0], box[:, 1], dets["label"][:n],
                               np.float64(c.gate), c.class_aware)
        det_row = np.full(M, -1, np.int32)
        taken = np.zeros(n, bool)
        a = np.float64(c.size_alpha)
        oma = 1.0 - a
        for k in np.nonzero(live)[0]:
            r = int(match[k])
            if r >= 0:
                taken[r] = True
                k0, k1 = self.gains(p[k, 0], p[k, 1], np.float64(c.r_pos))
                for q in range(3):
                    x[k, q], x[k, q + 3] = self.update_axis(x[k, q], x[k, q + 3], box[r, q], k0, k1)
                p[k] = self.update_cov(p[k, 0], p[k, 1], p[k, 2], k0, k1)
                for q in range(3):
                    self.size[s, k, q] = oma * self.size[s, k, q] + a * box[r, 3 + q]
                self.yaw[s, k] = box[r, 6]
                self.score[s, k] = dets["score"][r]
                self.label[s, k] = dets["label"][r]
                self.hits[s, k] += 1
                self.misses[s, k] = 0
                if self.hits[s, k] >= c.min_hits:
                    self.confirmed[s, k] = 1
                det_row[k] = r
            else:
                self.misses[s, k] += 1
                if self.misses[s, k] > c.max_misses:
                    live[k] = False
        for r in range(n):
            if taken[r] or not np.float64(dets["score"][r]) >= c.birth_score:
                continue
            free = np.nonzero(~live)[0]
            if len(free) == 0:
                self.overflow[s] += 1
                continue
            k = int(free[0])
            x[k, :3] = box[r, :3]
            x[k, 3:] = 0.0
            p[k] = (c.p0_pos, 0.0, c.p0_vel)
            self.size[s, k] = box[r, 3:6]
            self.yaw[s, k] = box[r, 6]
            self.score[s, k] = dets["score"][r]
            self.id[s, k] = self.next_id[s]
            self.next_id[s] += 1
            self.label[s, k] = dets["label"][r]
            self.hits[s, k] = 1
            self.misses[s, k] = 0
            self.confirmed[s, k] = 1 if 1 >= c.min_hits else 0
            live[k] = True
            det_row[k] = r
        out = self._out[s]
        out[:] = np.zeros((), TRACK_DTYPE)
        idx = np.nonzero(live)[0]
        m = len(idx)
        out["state"][:m] = x[idx]
        out["size"][:m] = self.size[s, idx]
        out["yaw"][:m] = self.yaw[s, idx]
        out["score"][:m] = self.score[s, idx]
        for f in ("id", "label", "hits", "misses", "confirmed"):
            out[f][:m] = getattr(self, f)[s, idx]
        out["det_row"][:m] = det_row[idx]
        self._nout[s] = m
        if pose is None:
            self._noutf[s] = -1
        else:
            self._fixed_out(s, pose, psi)
            self.prev_pose[s] = pose
            self.prev_psi[s] = psi
            self.has_prev[s] = True

    def step(self, dets, n_dets, dt=None, poses=None):
        """dets [batch, rows] (engine.DET_DTYPE rows: box3d_lidar, score, label are read), n_dets [batch], dt [batch]
        seconds or None (the period), poses [k, 3, 4] sensor-to-fixed transforms for streams 0 .. k - 1 (1 <= k <= batch;
        the others step without one) or None.  A count with the non-finite flag leaves its stream untouched.  Returns
        tracks()."""
        n_dets = np.asarray(n_dets).reshape(-1)
        batch = int(n_dets.shape[0])
        if batch < 1 or batch > self.streams:
            raise ValueError(f"batch {batch} outside [1, streams={self.streams}]")
        dets = np.asarray(dets)
        if dets.ndim == 1:
            dets = dets[None]
        if dets.shape[0] < batch or dets.shape[1] > MAX_ROWS:
            raise ValueError(f"dets must be [batch, rows <= {MAX_ROWS}], got {dets.shape}")
        dts = np.full(batch, self.cfg.period, np.float64) if dt is None else np.asarray(dt, np.float64).reshape(-1)
        for b in range(batch):
            if not (math.isfinite(dts[b]) and dts[b] > 0.0):
                raise ValueError(f"dt of stream {b} is {dts[b]} (must be finite and > 0)")
        P = None
        if poses is not None:
            k = np.asarray(poses).shape[0] if np.asarray(poses).ndim == 3 else -1
            if k == 0 or k > batch:
                raise ValueError(f"poses: {k} poses for {batch} streams")
            P = _swp.check_poses(poses, k)
        for b in range(batch):
            raw = int(n_dets[b])
            if raw & _NONFINITE:
                continue
            self._step_stream(b, dets[b], min(max(raw, 0), dets.shape[1]), dts[b], P[b] if P is not None and b < len(P) else None)
        self._batch = batch
        return self.tracks()

    def tracks(self, batch=None):
        """(tracks [batch, PP_TRACK_MAX] TRACK_DTYPE -- the live tracks in ascending slot order, zeros behind them --,
        n_tracks [batch], overflow [batch]) of the last step."""
        b = self._batch if batch is None else int(batch)
        return self._out[:b].copy(), self._nout[:b].copy(), self.overflow[:b].copy()

    def tracks_fixed(self, batch=None):
        """(tracks [batch, PP_TRACK_MAX], n_tracks [batch]) of the last step in the FIXED frame of its poses: tracks()'s
        rows with position, velocity and yaw mapped by the stream's pose; n_tracks is -1 for a stream whose step had none."""
        b = self._batch if batch is None else int(batch)
        tr, n = self._outf[:b].copy(), self._noutf[:b].copy()
        for s in range(b):
            tr[s, max(int(n[s]), 0):] = np.zeros((), TRACK_DTYPE)
        return tr, n

    def info(self):
        return {"live": self.live.sum(axis=1).astype(np.int32), "next_id": self.next_id.copy(), "overflow": self.overflow.copy()}


def track_np(config, frames, dts=None, streams=None, poses=None):
    """Functional form: frames = [(dets, n_dets), ...] in time order, dts = per-step dt ([batch] each, or None: the period),
    poses = per-step poses (as Tracker.step takes them, or None).  Returns the list of tracks() after every step."""
    frames = list(frames)
    if streams is None:
        streams = max((len(np.asarray(n).reshape(-1)) for _, n in frames), default=1)
    t = Tracker(config, streams)
    return [t.step(d, n, None if dts is None else dts[i], None if poses is None else poses[i]) for i, (d, n) in enumerate(frames)]


def det_track_ids(tracks, n_tracks, rows):
    """For one stream: the track id of each of its `rows` detection rows (int32, -1 for a row no track was matched with or
    opened from), from the step's tracks [PP_TRACK_MAX] and their count."""
    ids = np.full(int(rows), -1, np.int32)
    t = tracks[:int(n_tracks)]
    ok = (t["det_row"] >= 0) & (t["det_row"] < int(rows))
    ids[t["det_row"][ok]] = t["id"][ok]
    return ids


def det_track_velocity(tracks, n_tracks, rows):
    """Beside det_track_ids: [rows, 3] float64, the matched track's velocity, zeros for a row without one."""
    v = np.zeros((int(rows), 3), np.float64)
    t = tracks[:int(n_tracks)]
    ok = (t["det_row"] >= 0) & (t["det_row"] < int(rows))
    v[t["det_row"][ok]] = t["state"][ok, 3:]
    return v
