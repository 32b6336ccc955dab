"""Multi-sweep accumulation: the last few sweeps of a stream carried into the current sensor frame under the ego poses.

The reference sees one sweep per pass and has no such path, so nothing here is parity with it.  This module STATES the
rule: `SweepAccumulator` is the numpy restatement that the GPU stage (csrc/sweeps.hip, between the feed and the pass:
Engine.set_sweeps / accumulate_sweeps) mirrors operation for operation and equals bit for bit.  All pose arithmetic is
float64 with + - * only, and the order of every operation below is part of the rule.

A POSE is a [3, 4] float64 matrix [R | t] that maps the sensor frame to a fixed frame (odometry, map): p_fixed = R p + t.

One history per STREAM (frame b of every call is stream b): a ring of `history + 1` slots, each holding up to `capacity`
point rows, its row count, its pose and its stamp.  A call accumulate(frames, poses, stamps), per stream b:

1. the USED sweeps: the stored sweeps, newest first, at most `history`, with 0 < stamp_c - stamp_s <= max_age (float64);
2. per used sweep the relative transform: M = R_c^T R_s, every entry ((a0 * b0 + a1 * b1) + a2 * b2); d = t_s - t_c;
   u = R_c^T d in the same order;
3. the output frame: the current rows first, bit-unchanged (column `time_feature`, when >= 0, set to 0.0f); then each
   used sweep's rows in stored order, x' = float32(((M00 * x + M01 * y) + M02 * z) + u0) on the widened float32
   coordinates (y', z' alike), column `time_feature` = float32(stamp_c - stamp_s), every other column copied bitwise;
4. the output is cut at max_points_per_frame rows (the cut may fall inside a sweep); `truncated` counts the rows dropped;
5. the ORIGINAL current frame (before 3, in its own sensor frame) is stored as rows 0, j, 2j ... (j = history_decimate),
   cut at `capacity` (`push_truncated` counts the rows cut), with its pose and stamp, in the slot that holds the oldest
   sweep -- never a slot this call has read.
"""
import dataclasses
import math

import numpy as np

from ._lib import PP_SWEEP_MAX

ORTHO_TOL = 1e-6          # largest |R R^T - I| entry of an accepted rotation


@dataclasses.dataclass
class SweepConfig:
    """history           past sweeps kept per stream, 1 .. PP_SWEEP_MAX
    capacity          rows per stored sweep (None: the engine's max_points_per_frame)
    history_decimate  j >= 1: a sweep is stored as rows 0, j, 2j ... of the frame it came from
    max_age           seconds, > 0: stored sweeps older than this are not used
    time_feature      -1, or the column 3 .. F - 1 that is overwritten with the time lag (0 for the current rows)"""
    history: int = 4
    capacity: int = None
    history_decimate: int = 1
    max_age: float = 0.5
    time_feature: int = -1

    def __post_init__(self):
        for f, lo, hi in (("history", 1, PP_SWEEP_MAX), ("capacity", 1, None), ("history_decimate", 1, None),
                          ("time_feature", -1, None)):
            v = getattr(self, f)
            if f == "capacity" and v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"SweepConfig: {f} must be an integer, got {v!r}")
            if int(v) < lo or (hi is not None and int(v) > hi):
                raise ValueError(f"SweepConfig: {f} = {v} outside [{lo}, {hi if hi is not None else '...'}]")
            setattr(self, f, int(v))
        if self.time_feature in (0, 1, 2):
            raise ValueError(f"SweepConfig: time_feature = {self.time_feature} would overwrite a coordinate (-1, or 3 .. F - 1)")
        try:
            a = float(self.max_age)
        except (TypeError, ValueError):
            raise ValueError(f"SweepConfig: max_age must be a number, got {self.max_age!r}")
        if not (math.isfinite(a) and a > 0.0):
            raise ValueError(f"SweepConfig: max_age = {a} must be finite and > 0")
        self.max_age = a

    def to_dict(self):
        return dataclasses.asdict(self)

    @classmethod
    def from_any(cls, cfg):
        """A SweepConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"sweeps: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"sweeps: a SweepConfig, a dict of its fields or True, got {cfg!r}")

    def resolved(self, num_point_features, max_points_per_frame):
        """The configuration an engine of that shape runs: capacity filled in, time_feature checked against F."""
        F = int(num_point_features)
        if self.time_feature >= F:
            raise ValueError(f"sweeps: time_feature = {self.time_feature} but the model has {F} point features "
                             f"(-1{', or 3 .. %d' % (F - 1) if F > 3 else ': a 3-feature model has no spare column'})")
        cap = int(max_points_per_frame) if self.capacity is None else self.capacity
        return dataclasses.replace(self, capacity=cap)


def pose_from_xyyaw(x, y, yaw):
    """[3, 4] pose of a planar ego motion: a rotation by `yaw` about z, then the translation (x, y, 0)."""
    c, s = math.cos(float(yaw)), math.sin(float(yaw))
    return np.array([[c, -s, 0.0, float(x)], [s, c, 0.0, float(y)], [0.0, 0.0, 1.0, 0.0]], np.float64)


def pose_from_matrix(T4x4):
    """[3, 4] pose from a homogeneous [4, 4] sensor-to-fixed transform (the last row must be 0 0 0 1)."""
    T = np.asarray(T4x4, np.float64)
    if T.shape != (4, 4):
        raise ValueError(f"pose_from_matrix: a [4, 4] matrix, got {T.shape}")
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f"pose_from_matrix: the last row is {T[3].tolist()}, not 0 0 0 1")
    return np.ascontiguousarray(T[:3, :4])


def _poses_array(poses, batch):
    P = np.ascontiguousarray(poses, np.float64)
    if P.ndim != 3 or P.shape[1:] != (3, 4):
        raise ValueError(f"poses: [batch, 3, 4] (sensor to fixed frame, [R | t]), got {P.shape}")
    if P.shape[0] != batch:
        raise ValueError(f"poses: {P.shape[0]} poses for {batch} frames")
    return P


def _pose_finite(P, b):
    if not np.isfinite(P[b]).all():
        raise ValueError(f"poses: the pose of stream {b} is not finite")


def _pose_orthonormal(P, b):
    R = P[b, :, :3]
    for i in range(3):
        for j in range(3):
            g = (R[i, 0] * R[j, 0] + R[i, 1] * R[j, 1]) + R[i, 2] * R[j, 2]
            if not abs(g - (1.0 if i == j else 0.0)) <= ORTHO_TOL:
                raise ValueError(f"poses: the rotation of stream {b} is not orthonormal (R R^T [{i}][{j}] = {g!r})")


def check_poses(poses, batch):
    """The pose half of check_call, for a caller without stamps (the tracker): poses -> [batch, 3, 4] float64, each
    finite and orthonormal to ORTHO_TOL.  Raises ValueError naming the stream."""
    P = _poses_array(poses, batch)
    for b in range(batch):
        _pose_finite(P, b)
        _pose_orthonormal(P, b)
    return P


def check_call(poses, stamps, batch, last):
    """What every accumulate refuses before anything is queued.  poses -> [batch, 3, 4] float64, stamps -> [batch]
    float64; `last`: the streams' previous stamps (NaN: none).  Raises ValueError naming the stream; returns
    (poses, stamps, new_last) -- `last` itself is not changed."""
    P = _poses_array(poses, batch)
    if stamps is None:
        raise ValueError("stamps: one time stamp per frame is required with poses")
    s = np.ascontiguousarray(stamps, np.float64).reshape(-1)
    if s.shape[0] != batch:
        raise ValueError(f"stamps: {s.shape[0]} values for {batch} frames")
    new = np.array(last, np.float64)
    for b in range(batch):
        _pose_finite(P, b)
        if not math.isfinite(s[b]):
            raise ValueError(f"stamps: the stamp of stream {b} is not finite")
        _pose_orthonormal(P, b)
        if not math.isnan(new[b]) and not s[b] > new[b]:
            raise ValueError(f"stamps: the stamp of stream {b} does not increase ({s[b]!r} after {new[b]!r})")
        new[b] = s[b]
    return P, s, new


def relative_transform(pose_c, pose_s):
    """(M [3, 3], u [3]) float64 with p_c = M p_s + u: M = R_c^T R_s, u = R_c^T (t_s - t_c), in the rule's order."""
    c, s = np.asarray(pose_c, np.float64), np.asarray(pose_s, np.float64)
    M, u = np.empty((3, 3), np.float64), np.empty(3, np.float64)
    d = [s[k, 3] - c[k, 3] for k in range(3)]
    for i in range(3):
        for j in range(3):
            M[i, j] = (c[0, i] * s[0, j] + c[1, i] * s[1, j]) + c[2, i] * s[2, j]
        u[i] = (c[0, i] * d[0] + c[1, i] * d[1]) + c[2, i] * d[2]
    return M, u


class SweepAccumulator:
    """The rule, on the host: `streams` rings with the state of the GPU stage.  accumulate(frames, poses, stamps) takes
    streams 0 .. len(frames) - 1 one call further and returns (output frames, info); info holds what pp_sweeps_info
    returns: `count`, `used`, `truncated`, `push_truncated`, int32 [batch] each."""

    def __init__(self, config=None, streams=1, num_point_features=4, max_points_per_frame=32768):
        self.F, self.nmax, self.streams = int(num_point_features), int(max_points_per_frame), int(streams)
        self.cfg = SweepConfig.from_any(config if config is not None else True).resolved(self.F, self.nmax)
        self.slots = self.cfg.history + 1
        self.reset()

    def reset(self, stream=None):
        """Forgets the history (and the last stamp) of `stream`, or of every stream."""
        if stream is None:
            self.ring = [[None] * self.slots for _ in range(self.streams)]
            self.head = [0] * self.streams
            self.last = np.full(self.streams, np.nan)
        else:
            self.ring[stream] = [None] * self.slots
            self.head[stream] = 0
            self.last[stream] = np.nan

    def accumulate(self, frames, poses, stamps):
        c, F, B = self.cfg, self.F, len(frames)
        if B < 1 or B > self.streams:
            raise ValueError(f"accumulate: {B} frames, the accumulator has {self.streams} streams")
        P, S, new_last = check_call(poses, stamps, B, self.last[:B])
        cur = []
        for b, f in enumerate(frames):
            a = np.ascontiguousarray(f, np.float32)
            if a.ndim != 2 or a.shape[1] != F:
                raise ValueError(f"frame {b} must be [N, {F}], got {a.shape}")
            if a.shape[0] > self.nmax:
                raise ValueError(f"frame {b} has {a.shape[0]} points > max_points_per_frame = {self.nmax}")
            cur.append(a)
        self.last[:B] = new_last
        out = []
        info = {k: np.zeros(B, np.int32) for k in ("count", "used", "truncated", "push_truncated")}
        for b in range(B):
            head, ring = self.head[b], self.ring[b]
            first = cur[b].copy()
            if c.time_feature >= 0:
                first[:, c.time_feature] = np.float32(0.0)
            parts, used = [first], 0
            for k in range(1, c.history + 1):                       # newest first
                slot = ring[(head - k) % self.slots]
                if slot is None:
                    continue
                dt = S[b] - slot["stamp"]
                if not (dt > 0.0 and dt <= c.max_age):
                    continue
                used += 1
                M, u = relative_transform(P[b], slot["pose"])
                rows = slot["points"].copy()
                x, y, z = (slot["points"][:, i].astype(np.float64) for i in range(3))
                for i in range(3):
                    rows[:, i] = (((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + u[i]).astype(np.float32)
                if c.time_feature >= 0:
                    rows[:, c.time_feature] = np.float32(dt)
                parts.append(rows)
            full = np.concatenate(parts, axis=0)
            info["count"][b] = min(full.shape[0], self.nmax)
            info["used"][b] = used
            info["truncated"][b] = full.shape[0] - info["count"][b]
            out.append(np.ascontiguousarray(full[:self.nmax]))
            stored = cur[b][::c.history_decimate]
            info["push_truncated"][b] = max(stored.shape[0] - c.capacity, 0)
            ring[head] = {"points": stored[:c.capacity].copy(), "pose": P[b].copy(), "stamp": float(S[b])}
            self.head[b] = (head + 1) % self.slots
        return out, info


def accumulate_np(config, calls, num_point_features=4, max_points_per_frame=32768, streams=None):
    """A sequence of calls through a fresh SweepAccumulator: calls = [(frames, poses, stamps), ...]; returns the list
    of (output frames, info) the calls give."""
    calls = list(calls)
    S = streams if streams is not None else max((len(c[0]) for c in calls), default=1)
    acc = SweepAccumulator(config, S, num_point_features, max_points_per_frame)
    return [acc.accumulate(*c) for c in calls]
