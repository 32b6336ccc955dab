"""Obstacle inflation of an int8 grid in the layout of nav_msgs/OccupancyGrid (-1 unknown, 0 .. 100): every obstacle grown
by the robot's inscribed radius, and a cost beyond it that falls with the distance, so that a planner which treats the
robot as a point can read the grid as it is.  A third, opt-in stage behind the costmap (costmap.py) or the rolling
occupancy maps (occupancy.py), and a stand-alone call for any such grid.

The reference has no such path, so nothing here is parity with it.  This module STATES the rule: `inflate_np` is the
numpy restatement that the GPU (csrc/inflate.hip behind Engine.set_inflation / inflated_costmaps /
inflated_occupancy_maps, and `inflate`) equals byte for byte.  The device works in integers only; the cost table is
computed here on the host in float64 and only looked up there.

Input: one int8 grid g[H, W] and a configuration whose `resolution` is the grid's, metres per cell.

RADIUS.  R = ceil(inflation_radius / resolution) in float64 (`radius_cells`); R > PP_INFLATE_MAX_RADIUS = 64 is refused.

TABLE.  `cost_table` int8 [R * R + 1], indexed by the squared cell distance d2; with d = sqrt(float(d2)) * resolution:
100 if d2 == 0; 99 if d <= inscribed_radius; floor(98 * exp(-cost_scaling_factor * (d - inscribed_radius)) + 0.5) if
d <= inflation_radius; 0 otherwise.

DISTANCE.  A cell with g >= lethal_threshold is an OBSTACLE.  d2(cell) is the minimum of dx * dx + dy * dy over the
obstacle cells with |dx| <= R and |dy| <= R inside the grid; NONE = R * R + 1 if that minimum exceeds R * R or there is
no such cell (`distance2_np`).  Cells outside the grid are no obstacles.  The distance is the exact Euclidean one in
cells, not a chamfer or wavefront approximation.

COMPOSE.  t = 0 if d2 == NONE else table[d2].  A known cell (g >= 0) reads max(g, t); an unknown one reads t if
t >= unknown_min_cost, else -1.  Obstacle cells therefore read 100.  unknown_min_cost = 99 is the navigation stack's
"only the inscribed zone overwrites unknown".

Outputs: the grid int8 [H, W]; optionally the clearance map dist2 uint16 [H, W] (NONE where nothing is in reach); per
grid the counts `lethal` (obstacle cells) and `raised` (cells with out != g).

Out of scope: treating unknown cells as obstacles, non-circular footprints (the local planner's footprint, local_planner.py,
rolls the robot's outline itself and wants this stage at the footprint's inscribed radius), feeding inflated costs back into the
occupancy maps' log-odds, 3D, any ROS import.
"""
import ctypes
import dataclasses
import math

import numpy as np

from . import _lib
from ._lib import PP_INFLATE_MAX_RADIUS, PP_OCC_MAX_CELLS

SOURCES = ("costmap", "occupancy")      # `source` of the pp_*inflat* calls: PP_INFLATE_COSTMAP, PP_INFLATE_OCCUPANCY

_FLOATS = ("resolution", "inscribed_radius", "inflation_radius", "cost_scaling_factor")


@dataclasses.dataclass
class InflationConfig:
    """resolution            metres per cell, >= 0; 0.0: the source's (the engine fills it in; `inflate` needs > 0)
    inscribed_radius      metres, >= 0: the robot's centre keeps this far from every obstacle cell (cost 99 within)
    inflation_radius      metres, >= inscribed_radius: no cost beyond it
    cost_scaling_factor   1 / m, > 0: how fast the cost falls beyond the inscribed radius
    lethal_threshold      1 .. 100: a cell with g >= lethal_threshold is an obstacle
    unknown_min_cost      1 .. 100: the least cost that overwrites an unknown cell"""
    resolution: float = 0.0
    inscribed_radius: float = 0.3
    inflation_radius: float = 1.0
    cost_scaling_factor: float = 3.0
    lethal_threshold: int = 100
    unknown_min_cost: int = 1

    def __post_init__(self):
        for f in _FLOATS:
            v = getattr(self, f)
            try:
                if isinstance(v, bool):
                    raise TypeError
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"InflationConfig: {f} must be a number, got {getattr(self, f)!r}")
            if math.isnan(v) or math.isinf(v):
                raise ValueError(f"InflationConfig: {f} = {v} is not finite")
            setattr(self, f, v)
        if not self.resolution >= 0.0:
            raise ValueError(f"InflationConfig: resolution = {self.resolution} must be >= 0")
        if not self.inscribed_radius >= 0.0:
            raise ValueError(f"InflationConfig: inscribed_radius = {self.inscribed_radius} must be >= 0")
        if self.inflation_radius < self.inscribed_radius:
            raise ValueError(f"InflationConfig: inflation_radius = {self.inflation_radius} below inscribed_radius = "
                             f"{self.inscribed_radius}")
        if not self.cost_scaling_factor > 0.0:
            raise ValueError(f"InflationConfig: cost_scaling_factor = {self.cost_scaling_factor} must be > 0")
        for f, lo, hi in (("lethal_threshold", 1, 100), ("unknown_min_cost", 1, 100)):
            v = getattr(self, f)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"InflationConfig: {f} must be an integer, got {v!r}")
            if int(v) < lo or int(v) > hi:
                raise ValueError(f"InflationConfig: {f} = {v} outside [{lo}, {hi}]")
            setattr(self, f, int(v))
        if self.resolution > 0.0:
            radius_cells(self)

    def to_dict(self):
        return dataclasses.asdict(self)

    @classmethod
    def from_any(cls, cfg):
        """An InflationConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"inflation: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"inflation: an InflationConfig, a dict of its fields or True, got {cfg!r}")


def _with_resolution(cfg, who):
    c = InflationConfig.from_any(cfg)
    if not c.resolution > 0.0:
        raise ValueError(f"{who}: resolution = {c.resolution} must be > 0 (0.0 stands for a source's only on the engine)")
    return c


def radius_cells(cfg):
    """R = ceil(inflation_radius / resolution), float64.  Raises ValueError beyond PP_INFLATE_MAX_RADIUS."""
    c = cfg if isinstance(cfg, InflationConfig) else InflationConfig.from_any(cfg)
    if not c.resolution > 0.0:
        raise ValueError(f"inflation: resolution = {c.resolution} must be > 0")
    cells = math.ceil(c.inflation_radius / c.resolution)
    if cells > PP_INFLATE_MAX_RADIUS:
        raise ValueError(f"InflationConfig: inflation_radius = {c.inflation_radius} is {cells} cells of {c.resolution} m, at most "
                         f"PP_INFLATE_MAX_RADIUS = {PP_INFLATE_MAX_RADIUS}")
    return int(cells)


def cost_table(cfg):
    """int8 [R * R + 1]: the cost of a cell by its squared cell distance to the nearest obstacle (the rule's TABLE)."""
    c = _with_resolution(cfg, "cost_table")
    R = radius_cells(c)
    out = np.zeros(R * R + 1, np.int8)
    for d2 in range(R * R + 1):
        d = math.sqrt(float(d2)) * c.resolution
        if d2 == 0:
            out[d2] = 100
        elif d <= c.inscribed_radius:
            out[d2] = 99
        elif d <= c.inflation_radius:
            out[d2] = math.floor(98.0 * math.exp(-c.cost_scaling_factor * (d - c.inscribed_radius)) + 0.5)
    return out


def _grid(g, who):
    a = np.asarray(g)
    if a.dtype != np.int8 or a.ndim != 2 or a.size == 0:
        raise ValueError(f"{who}: a grid must be int8 [H, W] with H, W >= 1, got {a.dtype} {a.shape}")
    return a


def distance2_np(grid, cfg):
    """uint16 [H, W]: the rule's DISTANCE, as a row pass (the distance to the nearest obstacle of the cell's own row,
    R + 1 where none lies within R) and a column pass (the minimum over dy of h[y + dy][x]^2 + dy^2)."""
    c = _with_resolution(cfg, "distance2_np")
    g = _grid(grid, "distance2_np")
    R = radius_cells(c)
    H, W = g.shape
    obst = g >= c.lethal_threshold
    far = R + 1
    h = np.full((H, W), far, np.int64)
    for dx in range(max(-R, 1 - W), min(R, W - 1) + 1):     # cell x looks at x + dx, for x in [lo, hi)
        lo, hi = max(0, -dx), W - max(0, dx)
        dst = h[:, lo:hi]
        np.minimum(dst, np.where(obst[:, lo + dx:hi + dx], abs(dx), far), out=dst)
    best = np.full((H, W), R * R + 1, np.int64)
    for dy in range(max(-R, 1 - H), min(R, H - 1) + 1):
        lo, hi = max(0, -dy), H - max(0, dy)
        src = h[lo + dy:hi + dy, :]
        dst = best[lo:hi, :]
        np.minimum(dst, src * src + dy * dy, out=dst)
    return best.astype(np.uint16)


def inflate_np(grid, cfg, clearance=False, info=False):
    """The rule on one grid int8 [H, W]: out int8 [H, W]; clearance=True adds dist2 uint16 [H, W]; info=True adds
    {"lethal", "raised"}."""
    c = _with_resolution(cfg, "inflate_np")
    g = _grid(grid, "inflate_np")
    R = radius_cells(c)
    table = cost_table(c)
    d2 = distance2_np(g, c)
    t = np.where(d2 == R * R + 1, 0, table[np.minimum(d2, R * R)]).astype(np.int8)
    out = np.where(g >= 0, np.maximum(g, t), np.where(t >= c.unknown_min_cost, t, -1)).astype(np.int8)
    res = (out,)
    if clearance:
        res += (d2,)
    if info:
        res += ({"lethal": int((g >= c.lethal_threshold).sum()), "raised": int((out != g).sum())},)
    return res if len(res) > 1 else out


def inflate(grids, cfg, clearance=False, device=0, info=False):
    """The rule on the GPU, without an engine (pp_inflate_grids): grids int8 [H, W] or [B, H, W] (H * W <=
    PP_OCC_MAX_CELLS) -> out of the same shape; clearance=True adds dist2 uint16 of the same shape; info=True adds
    {"lethal", "raised"}, int32 [B] each (scalars for one grid)."""
    c = _with_resolution(cfg, "inflate")
    a = np.asarray(grids)
    one = a.ndim == 2
    if one:
        a = a[None]
    if a.dtype != np.int8 or a.ndim != 3 or a.size == 0:
        raise ValueError(f"inflate: grids must be int8 [H, W] or [B, H, W] with B, H, W >= 1, got {a.dtype} {np.asarray(grids).shape}")
    B, H, W = a.shape
    if H * W > PP_OCC_MAX_CELLS:
        raise ValueError(f"inflate: H * W = {H * W} cells, at most PP_OCC_MAX_CELLS = {PP_OCC_MAX_CELLS}")
    a = np.ascontiguousarray(a)
    table = np.ascontiguousarray(cost_table(c), np.int8)
    pc = _lib.PPInflationConfig(**c.to_dict())
    out = np.zeros((B, H, W), np.int8)
    d2 = np.zeros((B, H, W), np.uint16) if clearance else None
    counts = np.zeros((B, 2), np.int32)
    L = _lib.lib()
    st = L.pp_inflate_grids(int(device), a.ctypes.data, B, H, W, ctypes.byref(pc), table.ctypes.data, len(table),
                            out.ctypes.data, None if d2 is None else d2.ctypes.data, counts.ctypes.data)
    if st != 0:
        msg = L.pp_last_error(None)
        cls = ValueError if st == 1 else RuntimeError
        raise cls(f"inflate: {msg.decode() if msg else st}")
    res = (out[0] if one else out,)
    if clearance:
        res += (d2[0] if one else d2,)
    if info:
        res += ({"lethal": counts[0, 0] if one else counts[:, 0].copy(), "raised": counts[0, 1] if one else counts[:, 1].copy()},)
    return res if len(res) > 1 else res[0]


def to_occupancy_grid(grid, origin, resolution, stamp=None, frame_id=""):
    """The plain-attribute dict of a nav_msgs/OccupancyGrid for one inflated grid int8 [H, W], its origin (x, y) and its
    resolution: the entries of costmap.to_occupancy_grid / occupancy.to_occupancy_grid (no ROS is imported here)."""
    g = np.ascontiguousarray(_grid(grid, "to_occupancy_grid"), np.int8)
    o = np.asarray(origin, np.float64).reshape(-1)
    if o.shape != (2,):
        raise ValueError(f"to_occupancy_grid: origin must be (x, y), got {origin!r}")
    H, W = g.shape
    return {"header": {"stamp": stamp, "frame_id": frame_id},
            "info": {"map_load_time": stamp, "resolution": np.float32(resolution), "width": W, "height": H,
                     "origin": {"position": {"x": float(o[0]), "y": float(o[1]), "z": 0.0},
                                "orientation": {"x": 0.0, "y": 0.0, "z": 0.0, "w": 1.0}}},
            "data": g.reshape(-1)}
