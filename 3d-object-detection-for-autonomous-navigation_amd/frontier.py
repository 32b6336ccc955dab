"""Frontier clusters of an int8 grid in the layout of nav_msgs/OccupancyGrid (-1 unknown, 0 .. 100): where a robot that
explores should go next (Yamauchi 1997; explore_lite in ROS).  A fifth, opt-in stage behind the inflation of the costmap or
of the rolling occupancy maps, and a stand-alone call for any such grid.

The reference has no such path, so nothing here is parity with it.  This module STATES the rule: `frontier_np` is the numpy
restatement that the GPU (csrc/frontier.hip behind Engine.set_frontier / frontier_async / explore, and `frontier`) equals
byte for byte.  Everything is integer arithmetic; cells become metres on the host (`cells_to_metres`).  The operation order
below is part of the rule.

Input: one int8 grid g[H, W] (H * W <= PP_OCC_MAX_CELLS = 2^20), a FrontierConfig, one reference cell (rx, ry), and with
use_field a uint32 field pot[H, W] as navfn.py makes it.

1. FRONTIER CELL.  0 <= g <= free_max and at least one of the four edge neighbours INSIDE the grid is -1.  A neighbour
outside the grid is not unknown.  Four neighbours whatever `connectivity` says.  On an inflated grid the cells within the
robot's radius of an obstacle cost more than free_max, so they are never goals.

2. CLUSTERS.  The connected components of the frontier cells under `connectivity` (4: edges, 8: edges and corners).  A
cluster's label is the least linear index y * W + x of its cells (< 2^20).  labels uint32 [H, W], NONE = 0xFFFFFFFF where
there is no frontier cell.  The labelling is unique.

3. PER CLUSTER.  n = cells, sx = sum of x, sy = sum of y; the centroid cell cx = (2 sx + n) // (2 n), cy likewise; the
REPRESENTATIVE is the member that minimises the key (((x - cx)^2 + (y - cy)^2) << 20) | (y * W + x).  A centroid can lie
in unknown space or in a wall; the representative never does.

4. FILTER AND COST.  Clusters with n < min_size are dropped and counted in `small`.  D: with use_field = 0 the squared cell
distance from the reference cell to the representative (both reference coordinates within +-2^20, so D < 2^43); with
use_field = 1 the potential of the field at the representative, and a cluster whose D is UNREACHED is dropped and counted
in `unreached`.  The caller makes that field with the robot's own cell as the goal: D is then the travel cost over the
inflated grid, and a frontier behind a wall ranks by the way round it, not by air distance.

5. ORDER.  Ascending 64-bit key: rank 0 (nearest) (D << 20) | label, rank 1 (largest) ((2^20 - n) << 20) | label.  The
first max_frontiers are returned, eight int32 words each: x, y, cx, cy, n, label, D low, D high.  Per grid six info words:
frontier_cells, clusters, small, unreached, kept, returned.

Out of scope: information gain beyond size, blacklisting unreachable goals over time, frontiers of a map larger than the
window, multi-robot assignment, any ROS import.
"""
import ctypes
import dataclasses

import numpy as np

from . import _lib
from ._lib import PP_FRONTIER_INFO, PP_FRONTIER_MAX, PP_FRONTIER_NONE, PP_NAVFN_UNREACHED, PP_OCC_MAX_CELLS

SOURCES = ("costmap", "occupancy")      # `source` of the pp_*frontier* calls: the inflation's
NONE = PP_FRONTIER_NONE
UNREACHED = PP_NAVFN_UNREACHED
MAX_REF = 1 << 20                       # |reference coordinate| at most
INFO = ("frontier_cells", "clusters", "small", "unreached", "kept", "returned")
WORDS = ("x", "y", "cx", "cy", "n", "label", "d_lo", "d_hi")
assert len(INFO) == PP_FRONTIER_INFO and PP_OCC_MAX_CELLS == 1 << 20
assert (2 * (2 * MAX_REF) ** 2 << 20) < 2 ** 64         # the rank 0 key of the largest D fits 64 bits

_RANGES = (("free_max", 0, 99), ("connectivity", 4, 8), ("min_size", 1, PP_OCC_MAX_CELLS), ("max_frontiers", 1, PP_FRONTIER_MAX),
           ("rank", 0, 1), ("use_field", 0, 1))


@dataclasses.dataclass
class FrontierConfig:
    """free_max        0 .. 99: a known cell with g <= free_max is free
    connectivity    4 / 8: of the clusters
    min_size        >= 1 cells: smaller clusters are dropped
    max_frontiers   1 .. 64: frontiers returned per grid
    rank            0 nearest (least D), 1 largest (most cells)
    use_field       0 D is the squared cell distance from the reference cell; 1 D is a navigation-function potential"""
    free_max: int = 49
    connectivity: int = 8
    min_size: int = 3
    max_frontiers: int = 16
    rank: int = 0
    use_field: int = 0

    def __post_init__(self):
        for f, lo, hi in _RANGES:
            v = getattr(self, f)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"FrontierConfig: {f} must be an integer, got {v!r}")
            if int(v) < lo or int(v) > hi:
                raise ValueError(f"FrontierConfig: {f} = {v} outside [{lo}, {hi}]")
            setattr(self, f, int(v))
        if self.connectivity not in (4, 8):
            raise ValueError(f"FrontierConfig: connectivity = {self.connectivity} must be 4 or 8")

    def to_dict(self):
        return dataclasses.asdict(self)

    @classmethod
    def from_any(cls, cfg):
        """A FrontierConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"frontier: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"frontier: a FrontierConfig, a dict of its fields or True, got {cfg!r}")


def _ref(ref, who):
    a = np.asarray(ref)
    if a.shape != (2,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{who}: the reference must be an integer cell (x, y), got {ref!r}")
    x, y = int(a[0]), int(a[1])
    if abs(x) > MAX_REF or abs(y) > MAX_REF:
        raise ValueError(f"{who}: the reference cell ({x}, {y}) lies outside [-{MAX_REF}, {MAX_REF}]")
    return x, y


def frontier_cells_np(grid, cfg):
    """bool [H, W]: the rule's FRONTIER CELL."""
    c = FrontierConfig.from_any(cfg)
    g = np.asarray(grid)
    if g.dtype != np.int8 or g.ndim != 2 or g.size == 0:
        raise ValueError(f"frontier_cells_np: a grid must be int8 [H, W] with H, W >= 1, got {g.dtype} {g.shape}")
    unk = np.zeros((g.shape[0] + 2, g.shape[1] + 2), bool)          # one cell of "outside" around the grid: not unknown
    unk[1:-1, 1:-1] = g == -1
    near = unk[1:-1, 2:] | unk[1:-1, :-2] | unk[2:, 1:-1] | unk[:-2, 1:-1]
    return (g >= 0) & (g <= c.free_max) & near


def frontier_np(grid, cfg, ref=(0, 0), pot=None):
    """The rule on one grid -> (labels uint32 [H, W], words int32 [returned, 8], info int32 [6]); the words' columns are
    WORDS, the info's INFO.  pot uint32 [H, W] is read iff use_field."""
    c = FrontierConfig.from_any(cfg)
    front = frontier_cells_np(grid, c)
    H, W = front.shape
    if H * W > PP_OCC_MAX_CELLS:
        raise ValueError(f"frontier_np: H * W = {H * W} cells, at most PP_OCC_MAX_CELLS = {PP_OCC_MAX_CELLS}")
    rx, ry = _ref(ref, "frontier_np")
    if c.use_field:
        p = np.asarray(pot)
        if pot is None or p.dtype != np.uint32 or p.shape != (H, W):
            raise ValueError(f"frontier_np: use_field = 1 needs pot uint32 of the grid's shape {(H, W)}")
    moves = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))[:c.connectivity]
    labels = np.full((H, W), NONE, np.uint32)
    clusters = []                                       # (label, members) in the order of their labels
    ys, xs = np.nonzero(front)
    for y0, x0 in zip(ys.tolist(), xs.tolist()):        # raster order: the first cell met of a component is its least index
        if labels[y0, x0] != NONE:
            continue
        label = y0 * W + x0
        labels[y0, x0] = label
        members, stack = [], [(x0, y0)]
        while stack:
            x, y = stack.pop()
            members.append((x, y))
            for dx, dy in moves:
                qx, qy = x + dx, y + dy
                if 0 <= qx < W and 0 <= qy < H and front[qy, qx] and labels[qy, qx] == NONE:
                    labels[qy, qx] = label
                    stack.append((qx, qy))
        clusters.append((label, members))
    small = unreached = 0
    kept = []                                           # (sort key, words)
    for label, members in clusters:
        n = len(members)
        if n < c.min_size:
            small += 1
            continue
        sx, sy = sum(x for x, _ in members), sum(y for _, y in members)
        cx, cy = (2 * sx + n) // (2 * n), (2 * sy + n) // (2 * n)
        key = min((((x - cx) ** 2 + (y - cy) ** 2) << 20) | (y * W + x) for x, y in members)
        x, y = (key & 0xFFFFF) % W, (key & 0xFFFFF) // W
        if c.use_field:
            D = int(p[y, x])
            if D == UNREACHED:
                unreached += 1
                continue
        else:
            D = (x - rx) ** 2 + (y - ry) ** 2
        order = ((D if c.rank == 0 else (1 << 20) - n) << 20) | label
        assert order < 2 ** 64
        kept.append((order, (x, y, cx, cy, n, label, D & 0xFFFFFFFF, D >> 32)))
    kept.sort()
    words = np.array([w for _, w in kept[:c.max_frontiers]], np.int64).reshape(-1, 8)
    info = np.array([int(front.sum()), len(clusters), small, unreached, len(kept), len(words)], np.int32)
    return labels, words.astype(np.uint32).view(np.int32), info


def cost_of(words):
    """D of every row of `words` int32 [k, 8] as Python integers (the two halves joined)."""
    w = np.asarray(words).reshape(-1, 8)
    return [(int(np.uint32(r[7])) << 32) | int(np.uint32(r[6])) for r in w]


def cells_to_metres(cells, origin, resolution):
    """The centres of cells int32 [k, 2] in the grid's frame: float64 [k, 2] = origin + (cells + 0.5) * resolution."""
    c = np.asarray(cells, np.float64).reshape(-1, 2)
    return np.asarray(origin, np.float64).reshape(2) + (c + 0.5) * float(resolution)


def frontier(grids, cfg, refs=(0, 0), pot=None, device=0):
    """The rule on the GPU, without an engine (pp_frontier_grids): grids int8 [H, W] or [B, H, W] (H * W <=
    PP_OCC_MAX_CELLS), refs integer cells [B, 2] (or one (x, y)), pot uint32 of the grids' shape iff use_field ->
    (labels uint32 of the grids' shape, words, info): for one grid words int32 [returned, 8] and info int32 [6], for a batch
    a list of B such word arrays and info int32 [B, 6]."""
    c = FrontierConfig.from_any(cfg)
    a = np.asarray(grids)
    one = a.ndim == 2
    if one:
        a = a[None]
    if a.dtype != np.int8 or a.ndim != 3 or a.size == 0:
        raise ValueError(f"frontier: grids must be int8 [H, W] or [B, H, W] with B, H, W >= 1, got {a.dtype} {np.asarray(grids).shape}")
    B, H, W = a.shape
    if H * W > PP_OCC_MAX_CELLS:
        raise ValueError(f"frontier: H * W = {H * W} cells, at most PP_OCC_MAX_CELLS = {PP_OCC_MAX_CELLS}")
    a = np.ascontiguousarray(a)
    r = np.asarray(refs)
    if r.shape == (2,):
        r = np.broadcast_to(r, (B, 2))
    if r.shape != (B, 2) or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"frontier: refs must be integer cells [{B}, 2] as (x, y), got {r.dtype} {r.shape}")
    r = np.ascontiguousarray(np.clip(r, -(2 ** 31), 2 ** 31 - 1), np.int32)
    f = None
    if c.use_field:
        f = np.asarray(pot)
        if pot is None or f.dtype != np.uint32 or f.shape != np.asarray(grids).shape:
            raise ValueError(f"frontier: use_field = 1 needs pot uint32 of the grids' shape {np.asarray(grids).shape}")
        f = np.ascontiguousarray(f.reshape(B, H, W))
    pc = _lib.PPFrontierConfig(**c.to_dict())
    labels = np.zeros((B, H, W), np.uint32)
    words = np.zeros((B, PP_FRONTIER_MAX, 8), np.int32)
    info = np.zeros((B, PP_FRONTIER_INFO), np.int32)
    L = _lib.lib()
    st = L.pp_frontier_grids(int(device), a.ctypes.data, None if f is None else f.ctypes.data, B, H, W, ctypes.byref(pc),
                             r.ctypes.data, words.ctypes.data, info.ctypes.data, labels.ctypes.data)
    if st != 0:
        msg = L.pp_last_error(None)
        cls = ValueError if st == 1 else RuntimeError
        raise cls(f"frontier: {msg.decode() if msg else st}")
    wl = [words[b, :info[b, 5]].copy() for b in range(B)]
    return (labels[0], wl[0], info[0]) if one else (labels, wl, info)
