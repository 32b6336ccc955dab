"""Navigation function over an int8 grid in the layout of nav_msgs/OccupancyGrid (-1 unknown, 0 .. 100): the cost-to-go
field from one goal cell and the path that descends it from a start cell, for a robot read as a point -- the consumer the
inflated grids of inflation.py are made for.  A fourth, opt-in stage behind the inflation of the costmap or of the rolling
occupancy maps, and a stand-alone call for any such grid.

The reference has no such path, so nothing here is parity with it.  This module STATES the rule: `navfn_np` (a literal
heap Dijkstra from the goal), `relax_np` (whole-grid relaxation sweeps to the fixed point, an independent second statement)
and `descend_np` are the numpy restatement that the GPU (csrc/navfn.hip behind Engine.set_navfn / navfn_async / plan, and
`navfn`) equals byte for byte.  Everything is integer arithmetic; metres become cells here on the host (`goal_cells`).

Input: one int8 grid g[H, W], one goal cell (gx, gy), optionally one start cell (sx, sy), a NavfnConfig.

CELL COST.  c(p) uint16, 0 = BLOCKED.  A cell with g >= lethal_cost is blocked; an unknown cell (g < 0) is blocked unless
allow_unknown, then c = neutral_cost + cost_factor * unknown_cost; every other cell has c = neutral_cost + cost_factor * g.
The largest c is 50 + 5 * 100 = 550 (`cell_costs_np`).

MOVES.  Orthogonal neighbours weigh A = 5; with connectivity 8 diagonal neighbours weigh D = 7, and a diagonal move between
p and q is admissible only if both cells that share an edge with both are unblocked (no corner cutting).  Cells outside the
grid do not exist.  Neighbour order E, N, W, S, NE, NW, SW, SE = (dx, dy) (1,0) (0,1) (-1,0) (0,-1) (1,1) (-1,1) (-1,-1)
(1,-1); it decides ties in the path only.

FIELD.  pot uint32 [H, W], UNREACHED = 0xFFFFFFFF.  pot(goal) = 0 if the goal lies in the grid and is unblocked; every other
unblocked cell p has pot(p) = min over admissible reached neighbours q of pot(q) + w(p, q) * c(p): leaving p costs c(p).
Blocked cells and cells without such a chain read UNREACHED.  The largest step is 7 * 550 = 3850 and a grid has at most
PP_OCC_MAX_CELLS = 2^20 cells, so no potential reaches 2^32 - 1.  goal_state: 0 ok, 1 the goal is blocked, 2 the goal lies
outside the grid; 1 and 2 give an all-UNREACHED field and are no errors.  The field is the unique fixed point of the
relaxation, so any tiling, sweep order or number of rounds gives the same bytes.

PATH.  From the start, step to the admissible reached neighbour q that minimises pot(q) + w * c(p), the first in the order
above on a tie; stop at pot == 0.  int32 [n, 2] cells (x, y), start and goal included.  path_state: 0 the goal is reached;
1 the start is unreached or blocked (n = 0); 2 the start lies outside the grid (n = 0); 3 cut at max_path cells (the
first max_path are returned); 4 no start was given (n = 0).

Counts per grid: `reached`, the cells with pot != UNREACHED; `rounds`, the relaxation rounds the device ran
(implementation-defined, at least 1 where goal_state == 0).

Out of scope: several goals per grid, escaping from a blocked start, interpolated potentials and gradient paths, path
smoothing, non-circular footprints, 3D, a configuration key, any ROS import.  The local planner that reads this field
and gives velocity commands is local_planner.py.
"""
import ctypes
import dataclasses
import heapq

import numpy as np

from . import _lib
from ._lib import PP_NAVFN_MAX_PATH, PP_NAVFN_UNREACHED, PP_OCC_MAX_CELLS

SOURCES = ("costmap", "occupancy")      # `source` of the pp_*navfn* calls: the inflation's (PP_INFLATE_COSTMAP, PP_INFLATE_OCCUPANCY)
UNREACHED = PP_NAVFN_UNREACHED
A, D = 5, 7                             # the weight of an orthogonal and of a diagonal move
NEIGHBOURS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))     # (dx, dy): E N W S NE NW SW SE
MAX_COST = 50 + 5 * 100
assert D * MAX_COST * PP_OCC_MAX_CELLS < 2 ** 32 - 1        # a uint32 potential cannot overflow

_RANGES = (("lethal_cost", 1, 100), ("neutral_cost", 1, 50), ("cost_factor", 0, 5), ("allow_unknown", 0, 1),
           ("unknown_cost", 0, 100), ("connectivity", 4, 8), ("max_path", 1, PP_NAVFN_MAX_PATH), ("queued_rounds", 0, 4096))


@dataclasses.dataclass
class NavfnConfig:
    """lethal_cost     1 .. 100: a cell with g >= lethal_cost is blocked (99: the centre stays out of the inscribed zone)
    neutral_cost    1 .. 50: the cost of a free cell
    cost_factor     0 .. 5: c = neutral_cost + cost_factor * g for a known, unblocked cell
    allow_unknown   0 / 1: 0 unknown cells are blocked; 1 they cost neutral_cost + cost_factor * unknown_cost
    unknown_cost    0 .. 100
    connectivity    4 / 8
    max_path        1 .. 4096: the cells a returned path may hold
    queued_rounds   0 .. 4096: relaxation rounds an *_async call queues before it returns (0: a default from the grid's
                    shape); it affects timing only, never a result"""
    lethal_cost: int = 99
    neutral_cost: int = 10
    cost_factor: int = 1
    allow_unknown: int = 0
    unknown_cost: int = 50
    connectivity: int = 8
    max_path: int = 1024
    queued_rounds: int = 0

    def __post_init__(self):
        for f, lo, hi in _RANGES:
            v = getattr(self, f)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"NavfnConfig: {f} must be an integer, got {v!r}")
            if int(v) < lo or int(v) > hi:
                raise ValueError(f"NavfnConfig: {f} = {v} outside [{lo}, {hi}]")
            setattr(self, f, int(v))
        if self.connectivity not in (4, 8):
            raise ValueError(f"NavfnConfig: connectivity = {self.connectivity} must be 4 or 8")

    def to_dict(self):
        return dataclasses.asdict(self)

    @classmethod
    def from_any(cls, cfg):
        """A NavfnConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"navfn: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"navfn: a NavfnConfig, a dict of its fields or True, got {cfg!r}")


def _grid(g, who):
    a = np.asarray(g)
    if a.dtype != np.int8 or a.ndim != 2 or a.size == 0:
        raise ValueError(f"{who}: a grid must be int8 [H, W] with H, W >= 1, got {a.dtype} {a.shape}")
    return a


def _cell(xy, who, what):
    a = np.asarray(xy)
    if a.shape != (2,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{who}: {what} must be an integer cell (x, y), got {xy!r}")
    return int(a[0]), int(a[1])


def cell_costs_np(grid, cfg):
    """uint16 [H, W]: the rule's CELL COST, 0 where blocked."""
    c = NavfnConfig.from_any(cfg)
    g = _grid(grid, "cell_costs_np").astype(np.int64)
    cost = c.neutral_cost + c.cost_factor * g
    cost[g >= c.lethal_cost] = 0
    cost[g < 0] = c.neutral_cost + c.cost_factor * c.unknown_cost if c.allow_unknown else 0
    return cost.astype(np.uint16)


def _goal_state(cost, goal):
    H, W = cost.shape
    gx, gy = goal
    if not (0 <= gx < W and 0 <= gy < H):
        return 2
    return 0 if cost[gy, gx] else 1


def _admissible(cost, x, y, dx, dy):
    """The move from (x, y) to its neighbour (dx, dy), which lies in the grid: a diagonal one needs both cells beside it."""
    return not (dx and dy) or (cost[y, x + dx] != 0 and cost[y + dy, x] != 0)


def _result(pot, state, info):
    return (pot, {"goal_state": state, "reached": int((pot != UNREACHED).sum())}) if info else pot


def navfn_np(grid, goal, cfg, info=False):
    """The rule's FIELD on one grid, uint32 [H, W], by a heap Dijkstra from the goal, move by move as the rule states them.
    info=True adds {"goal_state", "reached"}."""
    c = NavfnConfig.from_any(cfg)
    cost = cell_costs_np(grid, c).astype(np.int64)
    goal = _cell(goal, "navfn_np", "goal")
    H, W = cost.shape
    pot = np.full((H, W), UNREACHED, np.uint32)
    state = _goal_state(cost, goal)
    if state:
        return _result(pot, state, info)
    moves = NEIGHBOURS[:c.connectivity]
    best = {goal: 0}
    done = set()
    heap = [(0, goal)]
    while heap:
        d, (x, y) = heapq.heappop(heap)
        if (x, y) in done:
            continue
        done.add((x, y))
        pot[y, x] = d
        for dx, dy in moves:                       # the cells p that may step to q = (x, y)
            px, py = x + dx, y + dy
            if not (0 <= px < W and 0 <= py < H) or cost[py, px] == 0 or (px, py) in done:
                continue
            if not _admissible(cost, x, y, dx, dy):
                continue
            nd = d + (D if dx and dy else A) * int(cost[py, px])
            if nd < best.get((px, py), 1 << 62):
                best[(px, py)] = nd
                heapq.heappush(heap, (nd, (px, py)))
    return _result(pot, state, info)


def relax_np(grid, goal, cfg, info=False):
    """The same field as the fixed point of whole-grid relaxation sweeps: every cell takes the minimum over its admissible
    reached neighbours at once, until a sweep moves nothing.  info=True adds {"goal_state", "reached", "sweeps"}."""
    c = NavfnConfig.from_any(cfg)
    cost = cell_costs_np(grid, c).astype(np.int64)
    goal = _cell(goal, "relax_np", "goal")
    H, W = cost.shape
    state = _goal_state(cost, goal)
    INF = np.int64(1) << 62
    P = np.full((H + 2, W + 2), INF, np.int64)          # one cell of "outside" around the grid
    C = np.zeros((H + 2, W + 2), np.int64)
    C[1:-1, 1:-1] = cost
    sweeps = 0
    if state == 0:
        P[goal[1] + 1, goal[0] + 1] = 0
        free = cost != 0
        ok = {}
        for dx, dy in NEIGHBOURS[:c.connectivity]:
            ok[dx, dy] = free.copy()
            if dx and dy:
                ok[dx, dy] &= (C[1:-1, 1 + dx:W + 1 + dx] != 0) & (C[1 + dy:H + 1 + dy, 1:-1] != 0)
        while True:
            sweeps += 1
            cur = P[1:-1, 1:-1]
            new = cur.copy()
            for (dx, dy), m in ok.items():
                q = P[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
                cand = np.where(m & (q < INF), q + (D if dx and dy else A) * cost, INF)
                np.minimum(new, cand, out=new)
            if np.array_equal(new, cur):
                break
            P[1:-1, 1:-1] = new
    pot = np.where(P[1:-1, 1:-1] >= INF, UNREACHED, P[1:-1, 1:-1]).astype(np.uint32)
    if not info:
        return pot
    return pot, {"goal_state": state, "reached": int((pot != UNREACHED).sum()), "sweeps": sweeps}


def descend_np(pot, grid, start, cfg):
    """The rule's PATH on one field: (cells int32 [n, 2] as (x, y), path_state).  start None: no path (state 4)."""
    c = NavfnConfig.from_any(cfg)
    cost = cell_costs_np(grid, c).astype(np.int64)
    p = np.asarray(pot)
    if p.dtype != np.uint32 or p.shape != cost.shape:
        raise ValueError(f"descend_np: pot must be uint32 of the grid's shape {cost.shape}, got {p.dtype} {p.shape}")
    none = np.zeros((0, 2), np.int32)
    if start is None:
        return none, 4
    x, y = _cell(start, "descend_np", "start")
    H, W = cost.shape
    if not (0 <= x < W and 0 <= y < H):
        return none, 2
    if p[y, x] == UNREACHED:
        return none, 1
    cells = []
    while True:
        cells.append((x, y))
        if p[y, x] == 0:
            state = 0
            break
        if len(cells) == c.max_path:
            state = 3
            break
        best = None
        for dx, dy in NEIGHBOURS[:c.connectivity]:
            qx, qy = x + dx, y + dy
            if not (0 <= qx < W and 0 <= qy < H) or p[qy, qx] == UNREACHED or not _admissible(cost, x, y, dx, dy):
                continue
            v = int(p[qy, qx]) + (D if dx and dy else A) * int(cost[y, x])
            if best is None or v < best[0]:
                best = (v, qx, qy)
        assert best is not None and best[0] == int(p[y, x]), "descend_np: pot is no field of this grid"
        x, y = best[1], best[2]
    return np.array(cells, np.int32).reshape(-1, 2), state


def goal_cells(xy, origins, resolution, shape):
    """Metres -> cells: int32 [B, 2] (x, y) = floor((xy - origin) / resolution) in float64, for points xy [B, 2] (or [2])
    in the frame of grids whose cell [0, 0] lies at origins [B, 2] (or [2]).  A NaN origin or coordinate gives (-1, -1),
    which reads as "outside"; a cell beyond the grid of `shape` = (H, W) is clipped to -1 / W / H, outside all the same."""
    p = np.atleast_2d(np.asarray(xy, np.float64))
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"goal_cells: xy must be [B, 2] metres, got {np.asarray(xy).shape}")
    o = np.broadcast_to(np.atleast_2d(np.asarray(origins, np.float64)), p.shape)
    if not float(resolution) > 0.0:
        raise ValueError(f"goal_cells: resolution = {resolution} must be > 0")
    H, W = int(shape[0]), int(shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((p - o) / float(resolution))
    bad = ~np.isfinite(f).all(axis=1)
    f = np.clip(np.where(bad[:, None], -1.0, f), -1.0, [float(W), float(H)])
    return f.astype(np.int32)


def path_to_metres(cells, origin, resolution):
    """The centres of a path's cells int32 [n, 2] in the grid's frame: float64 [n, 2] = origin + (cells + 0.5) * resolution."""
    c = np.asarray(cells, np.float64).reshape(-1, 2)
    o = np.asarray(origin, np.float64).reshape(2)
    return o + (c + 0.5) * float(resolution)


def _cells_arg(v, B, who, what):
    a = np.asarray(v)
    if a.shape == (2,):
        a = np.broadcast_to(a, (B, 2))
    if a.shape != (B, 2) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{who}: {what} must be integer cells [{B}, 2] as (x, y), got {a.dtype} {a.shape}")
    return np.ascontiguousarray(np.clip(a, -(2 ** 31), 2 ** 31 - 1), np.int32)


def navfn(grids, goals, cfg, starts=None, device=0, info=False):
    """The rule on the GPU, without an engine (pp_navfn_grids): grids int8 [H, W] or [B, H, W] (H * W <= PP_OCC_MAX_CELLS),
    goals integer cells [B, 2] (or one (x, y)), starts likewise or None (no paths: path_state 4) ->
    (pot uint32 of the grids' shape, paths, path_state): for one grid a path int32 [n, 2] and an int, for a batch a list of
    B paths and int32 [B].  info=True adds {"goal_state", "path_state", "path_len", "rounds", "reached"}, int32 [B] each
    (ints for one grid)."""
    c = NavfnConfig.from_any(cfg)
    a = np.asarray(grids)
    one = a.ndim == 2
    if one:
        a = a[None]
    if a.dtype != np.int8 or a.ndim != 3 or a.size == 0:
        raise ValueError(f"navfn: grids must be int8 [H, W] or [B, H, W] with B, H, W >= 1, got {a.dtype} {np.asarray(grids).shape}")
    B, H, W = a.shape
    if H * W > PP_OCC_MAX_CELLS:
        raise ValueError(f"navfn: H * W = {H * W} cells, at most PP_OCC_MAX_CELLS = {PP_OCC_MAX_CELLS}")
    a = np.ascontiguousarray(a)
    g = _cells_arg(goals, B, "navfn", "goals")
    s = None if starts is None else _cells_arg(starts, B, "navfn", "starts")
    pc = _lib.PPNavfnConfig(**c.to_dict())
    pot = np.zeros((B, H, W), np.uint32)
    paths = np.zeros((B, c.max_path, 2), np.int32)
    n = np.zeros(B, np.int32)
    st4 = np.zeros((4, B), np.int32)                    # goal_state, path_state, rounds, reached
    L = _lib.lib()
    st = L.pp_navfn_grids(int(device), a.ctypes.data, B, H, W, ctypes.byref(pc), g.ctypes.data,
                          None if s is None else s.ctypes.data, pot.ctypes.data, paths.ctypes.data, n.ctypes.data,
                          st4.ctypes.data)
    if st != 0:
        msg = L.pp_last_error(None)
        cls = ValueError if st == 1 else RuntimeError
        raise cls(f"navfn: {msg.decode() if msg else st}")
    plist = [paths[b, :n[b]].copy() for b in range(B)]
    res = (pot[0], plist[0], int(st4[1, 0])) if one else (pot, plist, st4[1].copy())
    if info:
        d = {"goal_state": st4[0], "path_state": st4[1], "path_len": n, "rounds": st4[2], "reached": st4[3]}
        res += ({k: int(v[0]) for k, v in d.items()} if one else {k: v.copy() for k, v in d.items()},)
    return res
