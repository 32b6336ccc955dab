"""Per-point object mask: for every row of a frame, "this return belongs to a detected or tracked object" -- so that the
maps are built from the static scene and not from the people walking through it.

The reference has no such path, so nothing here is parity with it.  This module STATES the rule: `object_mask_np` is the
numpy restatement that the GPU stage (csrc/object_mask.hip behind Engine.set_object_mask / object_mask_async /
object_mask) mirrors operation for operation.  All arithmetic is float64 with + - * and comparisons; the only
transcendental calls are the cos and sin of a footprint's yaw (and the atan2 of a pose, on the host in both), so the stage
equals the restatement bit for bit except in rows that lie within an ulp-sized margin of a footprint's edge
(`point_margins_np` names them).

FOOTPRINTS of frame b, in table order: exactly costmap.footprints_np's rectangles without the predicted steps -- centre
(ox, oy), c = cos(yaw), s = sin(yaw), hx = w * 0.5 + pad, hy = l * 0.5 + pad; a footprint with a non-finite field covers
nothing.  objects = "detections": the last pass's rows with score >= min_score, in row order (a frame flagged non-finite
has none).  objects = "tracks": the live slots (confirmed_only: the confirmed ones) in ascending slot order, as they stand
after the last tracking step -- in the sensor frame of that step.  The call may bring a COPY of every slot to now; the
tracker's own state is never written (a peek, not a step):

  pose P_c for the stream, and the tracker's has_prev set: the copy is carried exactly as tracking.Tracker._carry carries
      the slot: (M, u) = sweeps.relative_transform(P_c, prev_pose), x' = ((M00 * x + M01 * y) + M02 * z) + u0 (y' alike,
      from the old x y z), vx' = (M00 * vx + M01 * vy) + M02 * vz (vy' alike), yaw' = yaw + (psi_c - prev_psi) with
      psi_c = math.atan2(P_c[1][0], P_c[0][0]) on the host.  Without a previous pose the carry is skipped.
  dt (seconds, finite, >= 0): then x = Tracker.predict_axis(x, vx, dt), y alike.

A track masks only if (vx * vx + vy * vy) >= min_speed * min_speed, on the copy's velocity (after the carry), so a parked
object can stay in the map.

ROWS.  Per row, x and y widened from float32; per footprint: dx = x - ox, dy = y - oy, u = (dx * c) - (dy * s),
v = (dx * s) + (dy * c); the row is MASKED iff |u| <= hx and |v| <= hy for some footprint.  A NaN fails the test.  The test
is BEV only: z is left to the readers' own bands.  The device packs a frame's bits into 64-bit words, bit (i & 63) of word
i >> 6 for row i, zero past the frame's rows, with four info words per frame: footprints, masked rows, rows, flagged.

READERS, while their name is in `consumers` (each restatement takes mask=None and is unchanged without it):
  occupancy   OccupancyMap.update(points, pose, mask): a used row with z >= z_min whose bit is set is a MASKED end on its
              cell, not a hit; the cell still gets its one ray, and is itself neither hit nor passed by that ray.  A hit
              from an unmasked row in the same cell wins; ground rows are unaffected.
  scan_match  scan_cells_np(..., mask): a masked row takes no part and is counted with the ignored rows.
  costmap     point_layer_np / costmap_np(..., mask): an in-grid masked row marks its cell observed and adds no count.

Out of scope: a z test against the box, clearing cells under a track that were fused before it was confirmed, decay,
masking by predicted future positions (the costmap's horizon steps), rectangular movers in the local planner.
"""
import ctypes
import dataclasses
import math

import numpy as np

from . import _lib
from . import sweeps as _swp
from . import tracking as _trk
from ._lib import PP_OBJMASK_MAX_FOOTPRINTS as MAX_FOOTPRINTS, PP_OBJMASK_INFO

OBJECTS = ("detections", "tracks")          # pp_object_mask_config.objects: 1, 2
CONSUMERS = {"occupancy": _lib.PP_OBJMASK_OCCUPANCY, "scan_match": _lib.PP_OBJMASK_SCAN_MATCH, "costmap": _lib.PP_OBJMASK_COSTMAP}
INFO = ("footprints", "masked", "rows", "flagged")
MARGIN = 1e-9       # metres: rows nearer to a footprint's edge are those a last-place difference in cos / sin could flip

_FLOATS = ("min_score", "min_speed", "pad")


@dataclasses.dataclass
class ObjectMaskConfig:
    """objects           1 / "detections" (the last pass's rows), 2 / "tracks" (the streams' live slots)
    min_score         detections under it leave no footprint
    confirmed_only    tracks: only the confirmed ones
    min_speed         m/s, >= 0: a track masks only if (vx * vx + vy * vy) >= min_speed * min_speed
    pad               metres added to a footprint's half extents, >= 0
    consumers         the readers that use the mask: names out of "occupancy", "scan_match", "costmap" (or their
                      PP_OBJMASK_* bits as an int)"""
    objects: int = 2
    min_score: float = 0.0
    confirmed_only: int = 0
    min_speed: float = 0.0
    pad: float = 0.0
    consumers: object = ("occupancy", "scan_match", "costmap")

    def __post_init__(self):
        for f in _FLOATS:
            v = getattr(self, f)
            try:
                if isinstance(v, bool):
                    raise TypeError
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"ObjectMaskConfig: {f} must be a number, got {getattr(self, f)!r}")
            if not math.isfinite(v):
                raise ValueError(f"ObjectMaskConfig: {f} = {v} is not finite")
            setattr(self, f, v)
        if not self.min_speed >= 0.0:
            raise ValueError(f"ObjectMaskConfig: min_speed = {self.min_speed} must be >= 0")
        if not self.pad >= 0.0:
            raise ValueError(f"ObjectMaskConfig: pad = {self.pad} must be >= 0")
        if isinstance(self.objects, str):
            if self.objects not in OBJECTS:
                raise ValueError(f"ObjectMaskConfig: objects = {self.objects!r} is none of {OBJECTS}")
            self.objects = OBJECTS.index(self.objects) + 1
        if isinstance(self.objects, bool) or not isinstance(self.objects, (int, np.integer)) or int(self.objects) not in (1, 2):
            raise ValueError(f"ObjectMaskConfig: objects = {self.objects!r} (1 / 'detections', 2 / 'tracks')")
        self.objects = int(self.objects)
        if isinstance(self.confirmed_only, bool):
            self.confirmed_only = int(self.confirmed_only)
        if not isinstance(self.confirmed_only, (int, np.integer)) or int(self.confirmed_only) not in (0, 1):
            raise ValueError(f"ObjectMaskConfig: confirmed_only = {self.confirmed_only!r} outside [0, 1]")
        self.confirmed_only = int(self.confirmed_only)
        c = self.consumers
        if isinstance(c, bool):
            raise ValueError(f"ObjectMaskConfig: consumers = {c!r}")
        if isinstance(c, (int, np.integer)):
            bits = int(c)
            if bits < 0 or bits & ~sum(CONSUMERS.values()):
                raise ValueError(f"ObjectMaskConfig: consumers = {bits} holds bits outside {sum(CONSUMERS.values())}")
        else:
            names = [c] if isinstance(c, str) else list(c)
            unknown = [n for n in names if n not in CONSUMERS]
            if unknown:
                raise ValueError(f"ObjectMaskConfig: consumers {unknown!r} are none of {sorted(CONSUMERS)}")
            bits = 0
            for n in names:
                bits |= CONSUMERS[n]
        self.consumers = tuple(n for n, b in CONSUMERS.items() if bits & b)

    @property
    def consumer_bits(self):
        return sum(CONSUMERS[n] for n in self.consumers)

    def to_dict(self):
        """The fields as pp_object_mask_config holds them: consumers as its bits."""
        d = dataclasses.asdict(self)
        d["consumers"] = self.consumer_bits
        return d

    @classmethod
    def from_any(cls, cfg):
        """An ObjectMaskConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"object_mask: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"object_mask: an ObjectMaskConfig, a dict of its fields or True, got {cfg!r}")


def _cs(yaw):
    return (math.cos(yaw), math.sin(yaw)) if math.isfinite(yaw) else (math.nan, math.nan)


def _finite_rows(out):
    fp = np.array(out, np.float64).reshape(-1, 6)
    return fp[np.isfinite(fp).all(1)]


def rect_footprints_np(rects, pad=0.0):
    """float64 [K, 6] ox oy c s hx hy from rows x y w l yaw (what the stand-alone `object_mask` takes); rows with a
    non-finite field are left out."""
    r = np.asarray(rects, np.float64).reshape(-1, 5)
    return _finite_rows([(x, y) + _cs(yaw) + (w * 0.5 + pad, l * 0.5 + pad) for x, y, w, l, yaw in r.tolist()])


def peek_tracks_np(tracks, n_tracks, pose=None, prev=None, dt=None):
    """The copies the rule looks at: (state float64 [n, 6], yaw float64 [n]) of the first n_tracks rows of `tracks`
    (Tracker.tracks() / Engine.tracks() rows of one stream), carried by `pose` [3, 4] when prev = (prev_pose [3, 4],
    prev_psi) is given, then predicted by dt.  `tracks` is not changed."""
    t = np.asarray(tracks).reshape(-1)[:int(n_tracks)]
    st = np.array(t["state"], np.float64).reshape(-1, 6)
    yaw = np.array(t["yaw"], np.float64).reshape(-1)
    if pose is not None and prev is not None:
        P = np.asarray(pose, np.float64)
        psi = math.atan2(float(P[1, 0]), float(P[0, 0]))
        M, u = _swp.relative_transform(P, np.asarray(prev[0], np.float64))
        dpsi = np.float64(psi) - np.float64(prev[1])
        for k in range(len(st)):
            px, py, pz, vx, vy, vz = st[k]
            for i in range(3):
                st[k, i] = ((M[i, 0] * px + M[i, 1] * py) + M[i, 2] * pz) + u[i]
                st[k, 3 + i] = (M[i, 0] * vx + M[i, 1] * vy) + M[i, 2] * vz
            yaw[k] = yaw[k] + dpsi
    if dt is not None:
        d = np.float64(dt)
        for k in range(len(st)):
            for q in range(2):
                st[k, q] = _trk.Tracker.predict_axis(st[k, q], st[k, q + 3], d)
    return st, yaw


def footprints_np(cfg, dets=None, n_dets=None, tracks=None, n_tracks=None, pose=None, prev=None, dt=None):
    """The footprints of one frame, float64 [K, 6]: ox oy c s hx hy, in table order.  dets: rows of Engine.detections()
    (box3d_lidar, score), n_dets their count (a count with the non-finite flag: none); tracks: rows of tracks() of the
    frame's stream, with pose / prev / dt as `peek_tracks_np` takes them."""
    c = ObjectMaskConfig.from_any(cfg)
    out = []
    if c.objects == 1:
        if dets is None:
            raise ValueError("footprints_np: objects = detections needs dets")
        d = np.asarray(dets).reshape(-1)
        n = len(d) if n_dets is None else int(n_dets)
        if n & (1 << 30):
            n = 0
        d = d[:max(min(n, len(d)), 0)]
        box = d["box3d_lidar"].astype(np.float64).reshape(-1, 7)
        keep = d["score"].astype(np.float64) >= c.min_score
        for b in box[keep]:
            out.append((b[0], b[1]) + _cs(b[6]) + (b[3] * 0.5 + c.pad, b[4] * 0.5 + c.pad))
    else:
        if tracks is None:
            raise ValueError("footprints_np: objects = tracks needs tracks")
        t = np.asarray(tracks).reshape(-1)
        n = len(t) if n_tracks is None else int(n_tracks)
        st, yaw = peek_tracks_np(t, n, pose, prev, dt)
        for k in range(n):
            if c.confirmed_only and not t["confirmed"][k]:
                continue
            if not (st[k, 3] * st[k, 3] + st[k, 4] * st[k, 4]) >= c.min_speed * c.min_speed:
                continue
            size = t["size"][k].astype(np.float64)
            out.append((st[k, 0], st[k, 1]) + _cs(float(yaw[k])) + (size[0] * 0.5 + c.pad, size[1] * 0.5 + c.pad))
    return _finite_rows(out)


def _xy(points):
    p = np.asarray(points)
    if p.dtype != np.float32 or p.ndim != 2 or p.shape[1] < 3:
        raise ValueError(f"object_mask: points must be float32 [n, F >= 3], got {p.dtype} {p.shape}")
    return p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)


def _uv(x, y, f):
    dx, dy = x - f[0], y - f[1]
    return (dx * f[2]) - (dy * f[3]), (dx * f[3]) + (dy * f[2])


def object_mask_np(points, footprints):
    """bool [n]: the rows of one frame, float32 [n, F >= 3], that lie in one of `footprints` float64 [K, 6]."""
    x, y = _xy(points)
    mask = np.zeros(len(x), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in np.asarray(footprints, np.float64).reshape(-1, 6):
            u, v = _uv(x, y, f)
            mask |= (np.abs(u) <= f[4]) & (np.abs(v) <= f[5])
    return mask


def point_margins_np(points, footprints):
    """Per row [n] float64, metres: the smallest min(|hx - |u||, |hy - |v||) over the footprints (inf without any), as
    costmap.decision_margins gives it for cells.  Rows under MARGIN are those whose bit a last-place difference in
    cos / sin between libm and the device could flip; a row with a NaN has margin NaN and is masked by neither."""
    x, y = _xy(points)
    m = np.full(len(x), np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in np.asarray(footprints, np.float64).reshape(-1, 6):
            u, v = _uv(x, y, f)
            m = np.minimum(m, np.minimum(np.abs(f[4] - np.abs(u)), np.abs(f[5] - np.abs(v))))
    return m


def pack_words(mask, words=None):
    """uint64 [ceil(n / 64)] (or [words]) of bool [n]: bit (i & 63) of word i >> 6 is row i."""
    m = np.asarray(mask, bool).reshape(-1)
    w = (len(m) + 63) // 64 if words is None else int(words)
    bits = np.zeros(w * 64, np.uint64)
    bits[:len(m)] = m
    return (bits.reshape(w, 64) << np.arange(64, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def unpack_words(words, n):
    """bool [n] of uint64 words: the inverse of `pack_words`."""
    w = np.ascontiguousarray(words, np.uint64).reshape(-1)
    bits = (w[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    return bits.reshape(-1)[:int(n)].astype(bool)


def object_mask(points, rects, pad=0.0, device=0):
    """The GPU stage without an engine (pp_object_mask_points): points a list of B float32 [n, F >= 3] arrays (one F),
    rects a list of B float64 [k, 5] arrays x y w l yaw (k <= PP_OBJMASK_MAX_FOOTPRINTS) -> (masks, a list of B bool [n];
    words uint64 [B, ceil(max n / 64)]; info int32 [B, 4]: footprints, masked rows, rows, flagged)."""
    frames = [np.asarray(f) for f in points]
    B = len(frames)
    if B < 1 or any(f.dtype != np.float32 or f.ndim != 2 or f.shape[1] < 3 or f.shape[1] != frames[0].shape[1] for f in frames):
        raise ValueError("object_mask: points must be a list of float32 [n, F >= 3] arrays of one F")
    if len(rects) != B:
        raise ValueError(f"object_mask: {len(rects)} footprint tables for {B} frames")
    tables = [np.ascontiguousarray(r, np.float64).reshape(-1, 5) for r in rects]
    counts = np.array([len(t) for t in tables], np.int32)
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum([len(f) for f in frames])
    F = frames[0].shape[1]
    flat = np.ascontiguousarray(np.concatenate(frames, axis=0) if off[-1] else np.zeros((0, F), np.float32))
    fps = np.ascontiguousarray(np.concatenate(tables, axis=0) if counts.sum() else np.zeros((0, 5), np.float64))
    wpf = max((max(len(f) for f in frames) + 63) // 64, 1)
    words = np.zeros((B, wpf), np.uint64)
    info = np.zeros((B, PP_OBJMASK_INFO), np.int32)
    L_ = _lib.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    st = L_.pp_object_mask_points(int(device), vp(flat), vp(off), F, B, vp(fps), vp(counts), float(pad), vp(words), wpf, vp(info))
    if st != 0:
        msg = L_.pp_last_error(None)
        raise RuntimeError(f"pp_object_mask_points failed ({st}): {msg.decode() if msg else ''}")
    return [unpack_words(words[b], len(frames[b])) for b in range(B)], words, info
