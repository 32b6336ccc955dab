"""Obstacle costmap per frame: the resident points, the detections or the tracks of a pass as one int8 grid in the layout
of nav_msgs/OccupancyGrid (-1 unknown, 0 free, up to 100 lethal), in the sensor frame of that frame.

The reference has no such path, so nothing here is parity with it.  This module STATES the rule: `costmap_np` is the
numpy restatement that the GPU stage (csrc/costmap.hip behind Engine.set_costmap / costmaps) mirrors operation for
operation.  All arithmetic is float64 with + - * /, floor and comparisons; the only transcendental calls are the cos and
sin of a footprint's yaw, so the stage equals the restatement byte for byte except in cells whose centre lies within an
ulp-sized margin of a footprint's edge (`decision_margins` names them).

The grid is row-major, grid[iy, ix], cell (ix, iy) covering [x_min + ix * resolution, x_min + (ix + 1) * resolution) in x
and likewise in y.

POINT LAYER.  Per row of the frame, x y z widened from float32: fx = (x - x_min) / resolution, ix = floor(fx), the same
in y.  The point is in the grid iff fx >= 0 and ix < width (and likewise in y) -- a NaN fails every comparison.  An
in-grid point marks its cell OBSERVED; with z_min <= z <= z_max it also adds 1 to the cell's COUNT.  Further feature
columns are ignored.

OBJECT LAYER.  A footprint is a rectangle in the ground plane: centre (ox, oy), yaw r, half extents hx = w * 0.5 + pad
and hy = l * 0.5 + pad, in the convention of the lidar boxes x y z w l h r (rotation_3d_in_axis(axis=2): the offset of
local (lx, ly) is (lx cos r + ly sin r, -lx sin r + ly cos r)).  A cell belongs to a footprint iff its centre does:
cx = x_min + (ix + 0.5) * resolution, dx = cx - ox (the same in y), u = (dx * c) - (dy * s), v = (dx * s) + (dy * c),
inside iff |u| <= hx and |v| <= hy.  A footprint with a non-finite field covers nothing.  Sources: the detections with
score >= min_score at object_cost; or the live tracks (confirmed_only: the confirmed ones) at object_cost and, for
k = 1 .. horizon_steps, the same rectangle at (x + vx * t_k, y + vy * t_k), t_k = k * horizon_dt, at predict_cost[k - 1].

COMPOSE.  cell = max(point_cost if count >= min_points else -1, the costs of the footprints that cover it,
0 if observed else -1), stored as int8.

Inflation is a stage of its own behind this grid (inflation.py, Engine.set_inflation / inflated_costmaps).  Out of
scope: a map in the fixed frame accumulated over time (occupancy.py), ray-traced free space, any ROS import.

OBJECT MASK (object_mask.py; point_layer_np / costmap_np(..., mask=)): an in-grid row whose mask bit is set marks its cell
OBSERVED and adds no count, as a row outside the z band does -- an object is then painted once, as its footprint, and not
a second time as raw points.  Without a mask the rule is what it was.

GROUND CLASSES (ground.py; point_layer_np / costmap_np(..., ground=)): an in-grid row marks its cell observed, as now, and
adds to the count iff its class is OBSTACLE (and it is not object-masked), in the place of the z band.
"""
import dataclasses
import math

import numpy as np

from ._lib import PP_COSTMAP_MAX_STEPS, PP_COSTMAP_MAX_CELLS

OBJECTS = ("none", "detections", "tracks")      # pp_costmap_config.objects: 0, 1, 2

_FLOATS = ("x_min", "y_min", "resolution", "z_min", "z_max", "pad", "min_score", "horizon_dt")


@dataclasses.dataclass
class CostmapConfig:
    """x_min, y_min      the grid's origin in the sensor frame, metres
    resolution        metres per cell, > 0
    z_min, z_max      a point counts as an obstacle with z_min <= z <= z_max
    pad               metres added to a footprint's half extents, >= 0
    min_score         detections under it leave no footprint
    horizon_dt        seconds between two predicted footprints of a track, > 0
    width, height     cells, each >= 1, width * height <= PP_COSTMAP_MAX_CELLS
    min_points        counted points that make a cell an obstacle, >= 1
    objects           0 / "none", 1 / "detections", 2 / "tracks"
    confirmed_only    tracks: only the confirmed ones
    horizon_steps     0 .. PP_COSTMAP_MAX_STEPS predicted footprints per track
    point_cost, object_cost, predict_cost[k]   0 .. 100 (predict_cost past horizon_steps is ignored)"""
    x_min: float = 0.0
    y_min: float = -20.0
    resolution: float = 0.2
    z_min: float = -1.4
    z_max: float = 0.6
    pad: float = 0.0
    min_score: float = 0.0
    horizon_dt: float = 0.5
    width: int = 200
    height: int = 200
    min_points: int = 1
    objects: int = 0
    confirmed_only: int = 0
    horizon_steps: int = 0
    point_cost: int = 100
    object_cost: int = 100
    predict_cost: tuple = (90, 80, 70, 60, 50, 40, 30, 20)

    def __post_init__(self):
        for f in _FLOATS:
            v = getattr(self, f)
            try:
                if isinstance(v, bool):
                    raise TypeError
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"CostmapConfig: {f} must be a number, got {getattr(self, f)!r}")
            if math.isnan(v) or (f not in ("z_min", "z_max") and math.isinf(v)):
                raise ValueError(f"CostmapConfig: {f} = {v} is not finite")
            setattr(self, f, v)
        if not self.resolution > 0.0:
            raise ValueError(f"CostmapConfig: resolution = {self.resolution} must be > 0")
        if not self.pad >= 0.0:
            raise ValueError(f"CostmapConfig: pad = {self.pad} must be >= 0")
        if not self.horizon_dt > 0.0:
            raise ValueError(f"CostmapConfig: horizon_dt = {self.horizon_dt} must be > 0")
        if self.z_min > self.z_max:
            raise ValueError(f"CostmapConfig: z_min = {self.z_min} above z_max = {self.z_max}")
        if isinstance(self.objects, str):
            if self.objects not in OBJECTS:
                raise ValueError(f"CostmapConfig: objects = {self.objects!r} is none of {OBJECTS}")
            self.objects = OBJECTS.index(self.objects)
        if isinstance(self.confirmed_only, bool):
            self.confirmed_only = int(self.confirmed_only)
        for f, lo, hi in (("width", 1, PP_COSTMAP_MAX_CELLS), ("height", 1, PP_COSTMAP_MAX_CELLS), ("min_points", 1, None),
                          ("objects", 0, 2), ("confirmed_only", 0, 1), ("horizon_steps", 0, PP_COSTMAP_MAX_STEPS),
                          ("point_cost", 0, 100), ("object_cost", 0, 100)):
            v = getattr(self, f)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"CostmapConfig: {f} must be an integer, got {v!r}")
            if int(v) < lo or (hi is not None and int(v) > hi):
                raise ValueError(f"CostmapConfig: {f} = {v} outside [{lo}, {hi if hi is not None else '...'}]")
            setattr(self, f, int(v))
        if self.width * self.height > PP_COSTMAP_MAX_CELLS:
            raise ValueError(f"CostmapConfig: width * height = {self.width * self.height} cells, at most "
                             f"PP_COSTMAP_MAX_CELLS = {PP_COSTMAP_MAX_CELLS}")
        try:
            pc = list(self.predict_cost)
        except TypeError:
            raise ValueError(f"CostmapConfig: predict_cost must be a sequence of integers, got {self.predict_cost!r}")
        if len(pc) > PP_COSTMAP_MAX_STEPS or len(pc) < self.horizon_steps:
            raise ValueError(f"CostmapConfig: predict_cost has {len(pc)} entries for horizon_steps = {self.horizon_steps} "
                             f"(at most {PP_COSTMAP_MAX_STEPS})")
        for k, v in enumerate(pc):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"CostmapConfig: predict_cost[{k}] must be an integer, got {v!r}")
            if k < self.horizon_steps and not 0 <= int(v) <= 100:
                raise ValueError(f"CostmapConfig: predict_cost[{k}] = {v} outside [0, 100]")
        self.predict_cost = tuple(int(v) for v in pc) + (0,) * (PP_COSTMAP_MAX_STEPS - len(pc))

    def to_dict(self):
        d = dataclasses.asdict(self)
        d["predict_cost"] = list(self.predict_cost)
        return d

    @classmethod
    def from_any(cls, cfg):
        """A CostmapConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"costmap: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"costmap: a CostmapConfig, a dict of its fields or True, got {cfg!r}")


def _rows(rows, n, what):
    if rows is None:
        return None
    r = np.asarray(rows).reshape(-1)
    k = len(r) if n is None else int(n)
    if k < 0 or k > len(r):
        raise ValueError(f"{what}: count {k} outside [0, {len(r)}]")
    return r[:k]


def footprints_np(cfg, dets=None, n_dets=None, tracks=None, n_tracks=None):
    """The footprints of one frame, float64 [K, 7]: ox oy c s hx hy cost, in source order (a track's current rectangle,
    then its predicted ones).  dets: rows of Engine.detections() (any structured array with box3d_lidar and score);
    tracks: rows of Engine.tracks() (state, size, yaw, confirmed).  Rows that fail min_score / confirmed_only and
    footprints with a non-finite field are left out: they cover nothing."""
    c = CostmapConfig.from_any(cfg)
    out = []
    if c.objects == 1:
        d = _rows(dets, n_dets, "footprints_np: dets")
        if d is None:
            raise ValueError("footprints_np: objects = detections needs dets")
        box = d["box3d_lidar"].astype(np.float64).reshape(-1, 7)
        keep = d["score"].astype(np.float64) >= c.min_score
        for b in box[keep]:
            out.append((b[0], b[1], math.cos(b[6]) if math.isfinite(b[6]) else math.nan,
                        math.sin(b[6]) if math.isfinite(b[6]) else math.nan, b[3] * 0.5 + c.pad, b[4] * 0.5 + c.pad,
                        float(c.object_cost)))
    elif c.objects == 2:
        t = _rows(tracks, n_tracks, "footprints_np: tracks")
        if t is None:
            raise ValueError("footprints_np: objects = tracks needs tracks")
        for row in t:
            if c.confirmed_only and not row["confirmed"]:
                continue
            st, size, yaw = row["state"].astype(np.float64), row["size"].astype(np.float64), float(row["yaw"])
            cs = (math.cos(yaw), math.sin(yaw)) if math.isfinite(yaw) else (math.nan, math.nan)
            hx, hy = size[0] * 0.5 + c.pad, size[1] * 0.5 + c.pad
            out.append((st[0], st[1], cs[0], cs[1], hx, hy, float(c.object_cost)))
            for k in range(1, c.horizon_steps + 1):
                tk = float(k) * c.horizon_dt
                out.append((st[0] + st[3] * tk, st[1] + st[4] * tk, cs[0], cs[1], hx, hy, float(c.predict_cost[k - 1])))
    fp = np.array(out, np.float64).reshape(-1, 7)
    return fp[np.isfinite(fp[:, :6]).all(1)]


def _cell_centres(c):
    cx = c.x_min + (np.arange(c.width, dtype=np.float64) + 0.5) * c.resolution
    cy = c.y_min + (np.arange(c.height, dtype=np.float64) + 0.5) * c.resolution
    return cx[None, :], cy[:, None]


def _uv(c, f):
    cx, cy = _cell_centres(c)
    dx, dy = cx - f[0], cy - f[1]
    return (dx * f[2]) - (dy * f[3]), (dx * f[3]) + (dy * f[2])


def point_layer_np(points, cfg, mask=None, ground=None):
    """(counts int32 [H, W], observed bool [H, W]) of one frame's rows [n, F >= 3] float32; mask: bool [n], the rows'
    object mask, or None; ground: the pair (ground bool [n], obstacle bool [n]) of the rows' classes (ground.py), or None."""
    c = CostmapConfig.from_any(cfg)
    p = np.asarray(points)
    if p.dtype != np.float32 or p.ndim != 2 or p.shape[1] < 3:
        raise ValueError(f"costmap: points must be float32 [n, F >= 3], got {p.dtype} {p.shape}")
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = (x - c.x_min) / c.resolution, (y - c.y_min) / c.resolution
        inx = (fx >= 0) & (np.floor(fx) < c.width)
        iny = (fy >= 0) & (np.floor(fy) < c.height)
        ing = inx & iny
        if ground is None:
            zin = ing & (c.z_min <= z) & (z <= c.z_max)
        else:
            from . import ground as _gr
            zin = ing & _gr.check_classes(ground, len(p), "costmap")[1]
    if mask is not None:
        m = np.asarray(mask, bool).reshape(-1)
        if m.shape != (len(p),):
            raise ValueError(f"costmap: mask must be bool [{len(p)}], got {m.shape}")
        zin = zin & ~m
    cell = np.floor(fy[ing]).astype(np.int64) * c.width + np.floor(fx[ing]).astype(np.int64)
    n = c.width * c.height
    observed = np.bincount(cell, minlength=n) > 0
    czin = np.floor(fy[zin]).astype(np.int64) * c.width + np.floor(fx[zin]).astype(np.int64)
    counts = np.bincount(czin, minlength=n).astype(np.int32)
    return counts.reshape(c.height, c.width), observed.reshape(c.height, c.width)


def costmap_np(points, cfg, dets=None, n_dets=None, tracks=None, n_tracks=None, mask=None, ground=None):
    """One frame: (grid int8 [H, W], counts int32 [H, W]).  mask and ground as point_layer_np takes them."""
    c = CostmapConfig.from_any(cfg)
    counts, observed = point_layer_np(points, c, mask, ground)
    grid = np.where(observed, 0, -1).astype(np.int32)
    grid = np.maximum(grid, np.where(counts >= c.min_points, c.point_cost, -1))
    if c.objects:
        for f in footprints_np(c, dets, n_dets, tracks, n_tracks):
            u, v = _uv(c, f)
            inside = (np.abs(u) <= f[4]) & (np.abs(v) <= f[5])
            grid = np.where(inside, np.maximum(grid, int(f[6])), grid)
    return grid.astype(np.int8), counts


def decision_margins(cfg, footprints):
    """Per cell [H, W] float64, metres: the smallest min(|hx - |u||, |hy - |v||) over the footprints (inf without any).
    Cells under a bound are those whose membership a last-place difference in cos / sin could flip."""
    c = CostmapConfig.from_any(cfg)
    m = np.full((c.height, c.width), np.inf)
    for f in np.asarray(footprints, np.float64).reshape(-1, 7):
        u, v = _uv(c, f)
        m = np.minimum(m, np.minimum(np.abs(f[4] - np.abs(u)), np.abs(f[5] - np.abs(v))))
    return m


def to_occupancy_grid(grid, cfg, stamp=None, frame_id=""):
    """The plain-attribute dict of a nav_msgs/OccupancyGrid for one frame's grid: copy the entries into the message type
    of whatever ROS distribution publishes it (no ROS is imported here)."""
    c = CostmapConfig.from_any(cfg)
    g = np.ascontiguousarray(grid, np.int8)
    if g.shape != (c.height, c.width):
        raise ValueError(f"to_occupancy_grid: grid must be [{c.height}, {c.width}], got {g.shape}")
    return {"header": {"stamp": stamp, "frame_id": frame_id},
            "info": {"map_load_time": stamp, "resolution": np.float32(c.resolution), "width": c.width, "height": c.height,
                     "origin": {"position": {"x": c.x_min, "y": c.y_min, "z": 0.0},
                                "orientation": {"x": 0.0, "y": 0.0, "z": 0.0, "w": 1.0}}},
            "data": g.reshape(-1)}
