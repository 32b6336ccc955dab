"""Rolling occupancy map per stream in the fixed (odometry) frame: the resident points of a frame, under the sensor's pose,
update an int16 log-odds grid that stays centred on the sensor -- hits where returns end, free space along the rays that
reached them -- published as int8 in the layout of nav_msgs/OccupancyGrid (-1 unknown, 0 free .. 100 occupied) with its
origin in the fixed frame.

The reference has no such path, so nothing here is parity with it.  This module STATES the rule: `OccupancyMap` is the
numpy restatement that the GPU stage (csrc/occupancy.hip behind Engine.set_occupancy / occupancy_update_async /
occupancy_maps) mirrors operation for operation.  Apart from one float64 transform per row (+ * / and floor) the rule is
integer arithmetic, and the cost table is computed here on the host, so the stage equals the restatement byte for byte.

STATE.  An int16 log-odds L (units of 0.01 nat) and a `known` flag per cell of a W x H window, and the window's origin
cell (ox, oy) as global integer cell indices: window cell (ix, iy) is global cell (ox + ix, oy + iy), which covers
[(ox + ix) * resolution, (ox + ix + 1) * resolution) in the fixed frame's x, likewise y.  No window before the first update.

update(points float32 [n, F >= 3], pose [3, 4] sensor-to-fixed [R | t]):

1 WINDOW.  cx = floor(t_x / resolution), cy = floor(t_y / resolution) in float64; the new origin is (cx - W // 2,
  cy - H // 2), so the sensor's cell is always window cell (W // 2, H // 2).  Cells in both the old and the new window keep
  L and known; all others start as L = 0, unknown (a jump of W cells or more in x, or H or more in y, clears everything).
  |t_x| / resolution >= 2^30 (or t_y) is refused.

2 ENDPOINTS.  Per row, x y z widened from float32: px = ((R00 * x + R01 * y) + R02 * z) + t_x, py likewise with row 1;
  gx = floor(px / resolution) - ox, gy likewise (float64).  The row is USED iff gx >= 0, gx < W, gy >= 0, gy < H,
  (x * x + y * y) <= max_range * max_range and z <= z_max -- a NaN fails; the others are IGNORED.  A used row with
  z >= z_min is a HIT on its cell, with z < z_min a GROUND return on its cell.  z is the sensor-frame z, as in the costmap's
  point layer.

3 RAYS.  Every cell with a hit or ground endpoint gets exactly one ray, however many rows ended in it, from the sensor's
  cell (x0, y0) = (W // 2, H // 2) to that cell (x1, y1), walked FROM THE SENSOR OUTWARDS (`ray_cells`): dx = |x1 - x0|,
  dy = |y1 - y0|, sx = +1 if x1 > x0 else -1, sy likewise, err = dx - dy; while (x, y) != (x1, y1): mark (x, y) PASSED;
  e2 = 2 * err; if e2 > -dy: err -= dy, x += sx; if e2 < dx: err += dx, y += sy.  The endpoint itself is not marked by the
  walk; a ground endpoint marks its own cell passed.  The walk is not symmetric -- walked from the far end it visits other
  cells for 56 of the 225 targets (-7..7, -7..7) -- so its direction is part of the rule.

4 APPLY, once per cell and frame: delta = l_hit if hit, else -l_miss if passed, else 0; L = clamp(L + delta, l_min, l_max);
  known |= hit or passed.  A hit beats any number of passes.

5 PUBLISH.  cost = -1 if not known, else table[L - l_min], table[i] = floor(100 / (1 + exp(-(l_min + i) / 100)) + 0.5)
  (`cost_table`, float64 on the host; the device only looks it up).  grid[iy, ix], row-major;
  origin = (ox * resolution, oy * resolution) in the fixed frame.

The update reads whatever rows it is given.  On the engine that is the resident frame: after accumulate_sweeps it holds
the carried rows of past sweeps too, which would cast rays from the CURRENT sensor position -- so the update belongs
between the upload or ingest and the accumulation.

Inflation is a stage of its own behind the published grid (inflation.py, Engine.set_inflation / inflated_occupancy_maps);
it never feeds back into the log-odds.  OBJECT MASK (object_mask.py; update(..., mask=)): a used row with z >= z_min whose mask bit is set is a MASKED end on
its cell, not a hit.  Every cell with a hit, ground or masked end still gets its one ray; a cell whose only ends are
masked is neither hit nor passed by its own ray (another ray may pass it), and a hit from an unmasked row in the same
cell still wins.  The free space in front of an object is kept, the object itself leaves nothing.  Without a mask the
rule is what it was.  GROUND CLASSES (ground.py; update(..., ground=)): the z <= z_max test and the z >= z_min split are
dropped; an in-window, in-range row is a HIT iff OBSTACLE, a GROUND return iff GROUND and ignored otherwise, and an
object-mask bit still turns a hit into a masked end.  Without them the rule is what it was.

Out of scope: decay over time, 3D voxels, clipping rays that leave the window
(rows that end outside it are ignored, and counted), any ROS import.
"""
import dataclasses
import math

import numpy as np

from ._lib import PP_OCC_MAX_CELLS
from . import sweeps as _swp

_FLOATS = ("resolution", "z_min", "z_max", "max_range")
CELL_LIMIT = float(2 ** 30)      # |t| / resolution from which a pose is refused


@dataclasses.dataclass
class OccupancyConfig:
    """resolution        metres per cell, > 0
    z_min, z_max      a used row with z >= z_min is a hit, below z_min a ground return; rows above z_max are ignored
    max_range         metres in the sensor's x y plane, > 0: rows beyond it are ignored
    width, height     cells, each >= 1, width * height <= PP_OCC_MAX_CELLS
    l_hit, l_miss     log-odds steps in units of 0.01 nat, each 1 .. 1000
    l_min, l_max      clamps, -1000 <= l_min < 0 < l_max <= 1000
    The defaults are p = 0.7 / 0.4 per hit / miss, clamped at p = 0.1192 / 0.9707 (`from_probabilities`)."""
    resolution: float = 0.1
    z_min: float = -1.4
    z_max: float = 0.6
    max_range: float = 20.0
    width: int = 400
    height: int = 400
    l_hit: int = 85
    l_miss: int = 41
    l_min: int = -200
    l_max: int = 350

    def __post_init__(self):
        for f in _FLOATS:
            v = getattr(self, f)
            try:
                if isinstance(v, bool):
                    raise TypeError
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"OccupancyConfig: {f} must be a number, got {getattr(self, f)!r}")
            if math.isnan(v) or (f not in ("z_min", "z_max") and math.isinf(v)):
                raise ValueError(f"OccupancyConfig: {f} = {v} is not finite")
            setattr(self, f, v)
        if not self.resolution > 0.0:
            raise ValueError(f"OccupancyConfig: resolution = {self.resolution} must be > 0")
        if not self.max_range > 0.0:
            raise ValueError(f"OccupancyConfig: max_range = {self.max_range} must be > 0")
        if self.z_min > self.z_max:
            raise ValueError(f"OccupancyConfig: z_min = {self.z_min} above z_max = {self.z_max}")
        for f, lo, hi in (("width", 1, PP_OCC_MAX_CELLS), ("height", 1, PP_OCC_MAX_CELLS), ("l_hit", 1, 1000),
                          ("l_miss", 1, 1000), ("l_min", -1000, -1), ("l_max", 1, 1000)):
            v = getattr(self, f)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"OccupancyConfig: {f} must be an integer, got {v!r}")
            if int(v) < lo or int(v) > hi:
                raise ValueError(f"OccupancyConfig: {f} = {v} outside [{lo}, {hi}]")
            setattr(self, f, int(v))
        if self.width * self.height > PP_OCC_MAX_CELLS:
            raise ValueError(f"OccupancyConfig: width * height = {self.width * self.height} cells, at most "
                             f"PP_OCC_MAX_CELLS = {PP_OCC_MAX_CELLS}")

    def to_dict(self):
        return dataclasses.asdict(self)

    @classmethod
    def from_any(cls, cfg):
        """An OccupancyConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"occupancy: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"occupancy: an OccupancyConfig, a dict of its fields or True, got {cfg!r}")

    @classmethod
    def from_probabilities(cls, p_hit=0.7, p_miss=0.4, p_min=0.1192, p_max=0.9707, **fields):
        """The log-odds fields from probabilities: round(100 * ln(p / (1 - p))) each (p_miss < 0.5 gives the size of
        the step down).  The defaults give 85 / 41 / -200 / 350."""
        def lo(p, name):
            p = float(p)
            if not 0.0 < p < 1.0:
                raise ValueError(f"OccupancyConfig.from_probabilities: {name} = {p} outside (0, 1)")
            return int(round(100.0 * math.log(p / (1.0 - p))))
        return cls(l_hit=lo(p_hit, "p_hit"), l_miss=-lo(p_miss, "p_miss"), l_min=lo(p_min, "p_min"), l_max=lo(p_max, "p_max"),
                   **fields)


def cost_table(cfg):
    """int8 [l_max - l_min + 1]: table[i] = floor(100 / (1 + exp(-(l_min + i) / 100)) + 0.5), the cost of L = l_min + i."""
    c = OccupancyConfig.from_any(cfg)
    return np.array([math.floor(100.0 / (1.0 + math.exp(-(c.l_min + i) / 100.0)) + 0.5)
                     for i in range(c.l_max - c.l_min + 1)], np.int8)


def ray_cells(x0, y0, x1, y1):
    """The cells the walk from (x0, y0) to (x1, y1) marks passed, in order: (x0, y0) first, (x1, y1) never."""
    x, y = int(x0), int(y0)
    dx, dy = abs(x1 - x), abs(y1 - y)
    sx = 1 if x1 > x else -1
    sy = 1 if y1 > y else -1
    err = dx - dy
    out = []
    while (x, y) != (x1, y1):
        out.append((x, y))
        e2 = 2 * err
        if e2 > -dy:
            err -= dy
            x += sx
        if e2 < dx:
            err += dx
            y += sy
    return out


def window_origin(cfg, pose):
    """(ox, oy), the origin cell of the window a pose [3, 4] gives.  Raises ValueError from |t| / resolution = 2^30 on."""
    c = OccupancyConfig.from_any(cfg)
    P = np.asarray(pose, np.float64)
    out = []
    for k, (t, n) in enumerate(((P[0, 3], c.width), (P[1, 3], c.height))):
        if not abs(t / c.resolution) < CELL_LIMIT:
            raise ValueError(f"occupancy: the pose's t_{'xy'[k]} = {t!r} is 2^30 cells of {c.resolution} m or more from the origin")
        out.append(int(math.floor(t / c.resolution)) - n // 2)
    return tuple(out)


def end_cells(cfg, points, pose, origin_cell, mask=None, ground=None):
    """Step 2 for one frame: (hit bool [H, W], ground bool [H, W], (rows that hit, ground rows, ignored rows)) of rows
    float32 [n, F >= 3] under pose [3, 4] in the window whose origin cell is `origin_cell`.  With mask bool [n] (the
    object mask of the rows): (hit, ground, masked-end bool [H, W], (rows that hit, ground rows, ignored rows, masked
    rows)) -- a masked row of the hit band is a masked end and no hit.  With ground = (ground bool [n], obstacle bool [n])
    (the rows' classes, ground.py) the z tests are dropped: an in-window, in-range row is used iff it has one of the two
    bits, and lies in the hit band iff OBSTACLE."""
    c = OccupancyConfig.from_any(cfg)
    p, P = np.asarray(points), np.asarray(pose, np.float64)
    W, H = c.width, c.height
    ox, oy = origin_cell
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        px = ((P[0, 0] * x + P[0, 1] * y) + P[0, 2] * z) + P[0, 3]
        py = ((P[1, 0] * x + P[1, 1] * y) + P[1, 2] * z) + P[1, 3]
        gx = np.floor(px / c.resolution) - float(ox)
        gy = np.floor(py / c.resolution) - float(oy)
        inwin = (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H) & ((x * x + y * y) <= c.max_range * c.max_range)
        if ground is None:
            used = inwin & (z <= c.z_max)
            is_hit = used & (z >= c.z_min)
        else:
            from . import ground as _gr
            g_bit, o_bit = _gr.check_classes(ground, len(p), "occupancy")
            used = inwin & (g_bit | o_bit)
            is_hit = used & o_bit
    is_ground = used & ~is_hit
    if mask is not None:
        m = np.asarray(mask, bool).reshape(-1)
        if m.shape != (len(p),):
            raise ValueError(f"occupancy: mask must be bool [{len(p)}], got {m.shape}")
        is_masked = is_hit & m
        is_hit = is_hit & ~m
        masked = np.zeros((H, W), bool)
        masked[gy[is_masked].astype(np.int64), gx[is_masked].astype(np.int64)] = True
    hit = np.zeros((H, W), bool)
    ground = np.zeros((H, W), bool)
    hit[gy[is_hit].astype(np.int64), gx[is_hit].astype(np.int64)] = True
    ground[gy[is_ground].astype(np.int64), gx[is_ground].astype(np.int64)] = True
    if mask is not None:
        return hit, ground, masked, (int(is_hit.sum()), int(is_ground.sum()), int(len(p) - used.sum()), int(is_masked.sum()))
    return hit, ground, (int(is_hit.sum()), int(is_ground.sum()), int(len(p) - used.sum()))


def _passed_by_rays(ends_x, ends_y, x0, y0, shape):
    """bool [H, W]: the cells the walks from (x0, y0) to every (ends_x[k], ends_y[k]) mark, all walks stepped together
    (each exactly as `ray_cells` steps it)."""
    passed = np.zeros(shape, bool)
    x1, y1 = np.asarray(ends_x, np.int64), np.asarray(ends_y, np.int64)
    x, y = np.full_like(x1, x0), np.full_like(y1, y0)
    dx, dy = np.abs(x1 - x), np.abs(y1 - y)
    sx, sy = np.where(x1 > x, 1, -1), np.where(y1 > y, 1, -1)
    err = dx - dy
    while True:
        act = (x != x1) | (y != y1)
        if not act.any():
            return passed
        passed[y[act], x[act]] = True
        e2 = 2 * err
        mx, my = act & (e2 > -dy), act & (e2 < dx)
        err = err - np.where(mx, dy, 0) + np.where(my, dx, 0)
        x = x + np.where(mx, sx, 0)
        y = y + np.where(my, sy, 0)


class OccupancyMap:
    """One stream's map: the rule above, in numpy."""

    def __init__(self, cfg=True):
        self.cfg = OccupancyConfig.from_any(cfg)
        self.table = cost_table(self.cfg)
        self.reset()

    def reset(self):
        """Forgets the map: no window until the next update."""
        c = self.cfg
        self._L = np.zeros((c.height, c.width), np.int16)
        self._known = np.zeros((c.height, c.width), bool)
        self.origin_cell = None

    @property
    def origin(self):
        """(x, y) of window cell (0, 0)'s lower corner in the fixed frame, or None before the first update."""
        if self.origin_cell is None:
            return None
        return (self.origin_cell[0] * self.cfg.resolution, self.origin_cell[1] * self.cfg.resolution)

    def logodds(self):
        return self._L.copy()

    def known(self):
        return self._known.copy()

    def grid(self):
        """int8 [H, W]: -1 where not known, else table[L - l_min]."""
        cost = self.table[self._L.astype(np.int64) - self.cfg.l_min]
        return np.where(self._known, cost, -1).astype(np.int8)

    def _move_window(self, new):
        c = self.cfg
        W, H = c.width, c.height
        L, known = np.zeros((H, W), np.int16), np.zeros((H, W), bool)
        kept = 0
        if self.origin_cell is not None:
            sx, sy = new[0] - self.origin_cell[0], new[1] - self.origin_cell[1]      # new cell (ix, iy) was old (ix + sx, iy + sy)
            if abs(sx) < W and abs(sy) < H:
                nx0, nx1 = max(0, -sx), min(W, W - sx)
                ny0, ny1 = max(0, -sy), min(H, H - sy)
                L[ny0:ny1, nx0:nx1] = self._L[ny0 + sy:ny1 + sy, nx0 + sx:nx1 + sx]
                known[ny0:ny1, nx0:nx1] = self._known[ny0 + sy:ny1 + sy, nx0 + sx:nx1 + sx]
                kept = (nx1 - nx0) * (ny1 - ny0)
        self._L, self._known, self.origin_cell = L, known, new
        return W * H - kept

    def update(self, points, pose, mask=None, ground=None):
        """One frame.  Returns the info dict: rows `hits`, `ground`, `ignored`; `cells_hit`, `cells_free` (passed and not
        hit); `cleared`, the cells of the new window the old one did not hold (all of them at the first update).  mask:
        bool [n], the rows' object mask (object_mask.py) -- the dict then also counts the `masked` rows.  ground: the pair
        (ground bool [n], obstacle bool [n]) of the rows' classes (ground.py), in the place of the z band."""
        c = self.cfg
        p = np.asarray(points)
        if p.dtype != np.float32 or p.ndim != 2 or p.shape[1] < 3:
            raise ValueError(f"occupancy: points must be float32 [n, F >= 3], got {p.dtype} {p.shape}")
        P = _swp.check_poses(np.asarray(pose, np.float64)[None], 1)[0]
        W, H = c.width, c.height
        cleared = self._move_window(window_origin(c, P))
        if mask is None:
            hit, gnd, rows = end_cells(c, p, P, self.origin_cell, None, ground)
            ends = hit | gnd
        else:
            hit, gnd, masked, rows = end_cells(c, p, P, self.origin_cell, mask, ground)
            ends = hit | gnd | masked
        ey, ex = np.nonzero(ends)
        passed = _passed_by_rays(ex, ey, W // 2, H // 2, (H, W)) | gnd
        delta = np.where(hit, c.l_hit, np.where(passed, -c.l_miss, 0)).astype(np.int32)
        self._L = np.clip(self._L.astype(np.int32) + delta, c.l_min, c.l_max).astype(np.int16)
        self._known |= hit | passed
        info = {"hits": rows[0], "ground": rows[1], "ignored": rows[2],
                "cells_hit": int(hit.sum()), "cells_free": int((passed & ~hit).sum()), "cleared": int(cleared)}
        if mask is not None:
            info["masked"] = rows[3]
        return info


def to_occupancy_grid(grid, origin, cfg, stamp=None, frame_id=""):
    """The plain-attribute dict of a nav_msgs/OccupancyGrid for one stream's grid and its origin (x, y) in the fixed
    frame: copy the entries into the message type of whatever ROS distribution publishes it (no ROS is imported here)."""
    c = OccupancyConfig.from_any(cfg)
    g = np.ascontiguousarray(grid, np.int8)
    if g.shape != (c.height, c.width):
        raise ValueError(f"to_occupancy_grid: grid must be [{c.height}, {c.width}], got {g.shape}")
    o = np.asarray(origin, np.float64).reshape(-1)
    if o.shape != (2,):
        raise ValueError(f"to_occupancy_grid: origin must be (x, y), got {origin!r}")
    return {"header": {"stamp": stamp, "frame_id": frame_id},
            "info": {"map_load_time": stamp, "resolution": np.float32(c.resolution), "width": c.width, "height": c.height,
                     "origin": {"position": {"x": float(o[0]), "y": float(o[1]), "z": 0.0},
                                "orientation": {"x": 0.0, "y": 0.0, "z": 0.0, "w": 1.0}}},
            "data": g.reshape(-1)}
