"""The shared cases of the local planner (local_planner.py): each a Case(name, grid int8 [H, W], pot uint32 [H, W], navfn
cfg dict, pose (X, Y, h), window (v0, dv, w0, dw), cfg dict, goal_state), the smallest shapes at which the kernels of
csrc/local_plan.hip can go wrong -- one sample, sample counts round a wave and a workgroup, the most samples and the most
steps; headings that wrap through tick 0, reverse windows, a floor shift below zero, a closed circle; pitches that are no
multiple of 4, every edge of the grid, a wall, unknown cells; lookaheads, one into the wall; ties inside a wave and across workgroups; every
state; the largest weights -- and a batch of three.  The fields come from navfn.navfn_np.  `reference(name)` computes the
restatement once per case and the tests share it; the property each case is named for is asserted here, at import, with
the restatement."""
import collections
import functools

import numpy as np

import pp_amd

N = pp_amd.navfn
LP = pp_amd.local_planner
SUB = LP.SUB

Case = collections.namedtuple("Case", "name grid pot ncfg pose window cfg goal_state")


def centre(cx, cy, h=0):
    """The pose at the centre of cell (cx, cy)."""
    return (cx * SUB + SUB // 2, cy * SUB + SUB // 2, h)


@functools.lru_cache(maxsize=None)
def _field_cached(key, goal, ncfg_items):
    pot, info = N.navfn_np(_GRIDS[key], goal, dict(ncfg_items), info=True)
    pot.setflags(write=False)
    return pot, info["goal_state"]


_GRIDS = {}


def field(key, grid, goal, ncfg):
    """(pot, goal_state) of navfn_np on `grid`, computed once per (key, goal, ncfg)."""
    _GRIDS.setdefault(key, grid)
    assert _GRIDS[key] is grid
    return _field_cached(key, tuple(goal), tuple(sorted(ncfg.items())))


def _open(H, W):
    return np.zeros((H, W), np.int8)


def _costs(seed, H, W):
    """Costs 0 .. 60 everywhere: nothing blocked, no two paths alike."""
    return np.random.default_rng(seed).integers(0, 61, (H, W)).astype(np.int8)


OPEN40 = _open(40, 40)
OPEN41 = _open(41, 40)                  # 41 rows: row 20 is the axis of a mirror symmetry
OPEN21 = _open(21, 21)
COSTS_37 = _costs(11, 29, 37)           # rows of 40 cells on the device behind an engine; 37 stand-alone
COSTS_33 = _costs(12, 31, 33)
COSTS_31 = _costs(13, 33, 31)

WALL = _open(40, 40)
WALL[5:35, 26] = 100

UNKNOWN_BAND = _costs(14, 40, 40)
UNKNOWN_BAND[:, 24:27] = -1             # a band of unknown cells across the way
UNKNOWN_BAND[18:22, 24:27] = 0          # ... with a known gap

POCKET = _open(40, 40)                  # a dead end that opens to -x: the robot faces its closed end
for _x, _y in ((21, 19), (21, 20), (21, 21), (20, 19), (20, 21), (19, 19), (19, 21)):
    POCKET[_y, _x] = 100

STEEP = np.full((40, 40), 98, np.int8)  # the dearest traversable cells: the largest potentials
STEEP_N = dict(cost_factor=5, neutral_cost=50, lethal_cost=99)

GOAL_BLOCKED = _open(40, 40)
GOAL_BLOCKED[20, 35] = 100

CASES = []


def add(name, key, grid, goal, pose, window, cfg, ncfg=None):
    ncfg = dict(ncfg or {})
    pot, gs = field(key, grid, goal, ncfg)
    CASES.append(Case(name, grid, pot, ncfg, tuple(pose), tuple(window), dict(cfg), gs))


W0 = dict(pot_weight=8, occ_weight=4, speed_weight=1, turn_weight=1)        # the weights of most cases
EAST = (35, 20)

# ---- the shape of the launch ----
add("one_sample_one_step", "open40", OPEN40, EAST, centre(20, 20), (512, 0, 0, 0), dict(W0, nv=1, nw=1, steps=1))
add("samples_63", "open40", OPEN40, EAST, centre(20, 20), (200, 100, -200, 50), dict(W0, nv=7, nw=9, steps=6))
add("samples_64", "open40", OPEN40, EAST, centre(20, 20), (200, 100, -210, 60), dict(W0, nv=8, nw=8, steps=6))
add("samples_65", "open40", OPEN40, EAST, centre(20, 20), (200, 150, -240, 40), dict(W0, nv=5, nw=13, steps=6))
add("samples_257", "open40", OPEN40, EAST, centre(20, 20), (800, 0, -512, 4), dict(W0, nv=1, nw=257, steps=5))
add("samples_16384", "open40", OPEN40, EAST, centre(20, 20), (-508, 8, -508, 8), dict(W0, nv=128, nw=128, steps=3))
add("steps_256", "open40", OPEN40, EAST, centre(20, 20), (16, 16, -8, 4), dict(W0, nv=3, nw=5, steps=256))
# ---- arithmetic ----
add("heading_wraps_up", "open40", OPEN40, (32, 34), centre(20, 20, 4090), (300, 200, -24, 6), dict(W0, nv=3, nw=9, steps=8))
add("heading_wraps_down", "open40", OPEN40, (32, 6), centre(20, 20, 6), (300, 200, -24, 6), dict(W0, nv=3, nw=9, steps=8))
add("reverse_window", "open40", OPEN40, (5, 20), centre(20, 20), (-900, 100, -80, 40), dict(W0, nv=8, nw=5, steps=8))
add("x_goes_negative", "open40", OPEN40, EAST, (300, 20 * SUB + 512, 0), (-600, 150, -40, 20), dict(W0, nv=9, nw=5, steps=1))
add("closed_circle", "open40", OPEN40, (20, 30), centre(20, 8), (824, 100, 56, 8), dict(W0, nv=3, nw=3, steps=64))
# ---- the grid ----
add("pitch_37", "costs37", COSTS_37, (33, 14), centre(6, 14, 100), (200, 100, -120, 30), dict(W0, nv=8, nw=9, steps=12))
add("pitch_33", "costs33", COSTS_33, (3, 28), centre(28, 4, 1500), (200, 100, -120, 30), dict(W0, nv=8, nw=9, steps=12))
add("pitch_31", "costs31", COSTS_31, (15, 30), centre(15, 3, 1024), (200, 100, -120, 30), dict(W0, nv=8, nw=9, steps=12))
for _name, _h, _goal in (("east", 0, (20, 10)), ("north", 1024, (10, 20)), ("west", 2048, (0, 10)), ("south", 3072, (10, 0))):
    add("leaves_" + _name, "open21", OPEN21, _goal, centre(10, 10, _h), (128, 128, -60, 30), dict(W0, nv=8, nw=5, steps=14))
add("wall_ahead", "wall", WALL, EAST, centre(20, 20), (524, 100, -96, 12), dict(W0, nv=6, nw=17, steps=10))
add("unknown_blocked", "band", UNKNOWN_BAND, EAST, centre(16, 14), (300, 100, -120, 30), dict(W0, nv=8, nw=9, steps=12),
    dict(allow_unknown=0))
add("unknown_allowed", "band", UNKNOWN_BAND, EAST, centre(16, 14), (300, 100, -120, 30), dict(W0, nv=8, nw=9, steps=12),
    dict(allow_unknown=1, unknown_cost=70))
# ---- lookahead: the goal behind the robot; the speed and turn terms off, so the field alone decides ----
_LOOK = dict(pot_weight=8, occ_weight=4, speed_weight=0, turn_weight=0, nv=5, nw=9, steps=4)
add("lookahead_0", "open40", OPEN40, (5, 20), centre(20, 20), (0, 128, -512, 128), dict(_LOOK, lookahead=0))
add("lookahead_3_cells", "open40", OPEN40, (5, 20), centre(20, 20), (0, 128, -512, 128), dict(_LOOK, lookahead=3 * SUB))
add("lookahead_unreached", "wall", WALL, EAST, centre(20, 20), (300, 100, -160, 40), dict(W0, nv=8, nw=9, steps=5, lookahead=3 * SUB))
# ---- ties ----
add("mirror_tie", "open41", OPEN41, (35, 20), centre(5, 20), (900, 0, -45, 6), dict(W0, nv=1, nw=16, steps=10))
add("tie_across_workgroups", "open41", OPEN41, (35, 20), centre(5, 20), (900, 0, -6, 2), dict(W0, nv=2, nw=256, steps=10))
# ---- each state ----
add("boxed_in", "pocket", POCKET, (2, 20), centre(20, 20), (600, 50, -100, 25), dict(W0, nv=9, nw=9, steps=4))
add("arrived", "open40", OPEN40, EAST, centre(35, 20, 77), (200, 100, -120, 30), dict(W0, nv=8, nw=9, steps=6))
add("pose_outside", "open40", OPEN40, EAST, (-1, 20 * SUB, 0), (200, 100, -120, 30), dict(W0, nv=8, nw=9, steps=6))
add("pose_blocked", "wall", WALL, EAST, centre(26, 20), (200, 100, -120, 30), dict(W0, nv=8, nw=9, steps=6))
add("goal_blocked", "goal_blocked", GOAL_BLOCKED, EAST, centre(20, 20), (200, 100, -120, 30), dict(W0, nv=8, nw=9, steps=6))
# ---- weights ----
add("largest_weights", "steep", STEEP, (39, 39), centre(1, 1, 512), (200, 100, -120, 30),
    dict(pot_weight=255, occ_weight=65535, speed_weight=65535, turn_weight=65535, nv=8, nw=9, steps=6, lookahead=2 * SUB), STEEP_N)

NAMES = [c.name for c in CASES]
assert len(set(NAMES)) == len(NAMES)


def case(name):
    return CASES[NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def reference(name):
    """best_np of the case (through scores_np); computed once, never written to."""
    c = case(name)
    out = LP.best_np(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg, c.goal_state)
    out["keys"].setflags(write=False)
    out["traj"].setflags(write=False)
    return out


def scores(name):
    """The distinct scores of the case's valid samples."""
    k = reference(name)["keys"]
    return np.unique(k[k != LP.INVALID] >> np.uint64(14))


# ---- the properties the cases are named for ----
# a reduction is only shown right by a real competition: every case in state 0 has at least 8 valid samples and at least 2
# distinct scores.  The one case that cannot is the launch of ONE sample, which is there for the launch's shape.
for _c in CASES:
    _r = reference(_c.name)
    if _r["cmd_state"] == 0 and _c.name != "one_sample_one_step":
        assert _r["n_ok"] >= 8 and len(scores(_c.name)) >= 2, (_c.name, _r["n_ok"], len(scores(_c.name)))
    assert _r["n_ok"] + _r["n_outside"] + _r["n_collision"] + _r["n_unreached"] == (_c.cfg["nv"] * _c.cfg["nw"] if _r["cmd_state"] < 2 else 0)
assert reference("one_sample_one_step")["cmd_state"] == 0 and reference("one_sample_one_step")["best"] == 0
for _n, _want in (("samples_63", 63), ("samples_64", 64), ("samples_65", 65), ("samples_257", 257), ("samples_16384", 16384)):
    assert case(_n).cfg["nv"] * case(_n).cfg["nw"] == _want and reference(_n)["cmd_state"] == 0
assert reference("samples_16384")["best"] >= 256 and reference("samples_257")["best"] >= 64        # not in the first workgroup / wave
assert case("steps_256").cfg["steps"] == LP.PP_LOCAL_MAX_STEPS and reference("steps_256")["n_ok"] == 15
for _n, _up in (("heading_wraps_up", True), ("heading_wraps_down", False)):
    _t = reference(_n)["traj"][:, 2].astype(np.int64)
    _d = np.diff(_t)
    assert ((_d < -2048) if _up else (_d > 2048)).any(), _n        # the winner itself passes tick 0
assert case("reverse_window").window[0] + 7 * case("reverse_window").window[1] < 0 and reference("reverse_window")["sv"] < 0
_r = reference("x_goes_negative")
assert _r["n_outside"] > 0 and _r["cmd_state"] == 0
_reason, _, _poses = LP.score_np(*case("x_goes_negative")[1:3], case("x_goes_negative").pose, -600, 0, {}, case("x_goes_negative").cfg)
assert _reason == LP.OUTSIDE and -SUB < _poses[-1][0] < 0          # X in (-1024, 0): cell -1 by the floor shift, cell 0 by a truncation
_c = case("closed_circle")
_reason, _, _poses = LP.score_np(_c.grid, _c.pot, _c.pose, 1024, 64, _c.ncfg, _c.cfg)
assert _reason == LP.OK and len(_poses) == 65 and _poses[-1] == _poses[0], (_poses[0], _poses[-1])
assert LP.sample(8, _c.window, _c.cfg) != (1024, 64) and LP.sample(7, _c.window, _c.cfg) == (1024, 64)
for _n in ("pitch_37", "pitch_33", "pitch_31"):
    assert case(_n).grid.shape[1] % 4 != 0 and reference(_n)["cmd_state"] == 0
for _n, _axis, _sign in (("leaves_east", 0, 1), ("leaves_north", 1, 1), ("leaves_west", 0, -1), ("leaves_south", 1, -1)):
    _r = reference(_n)
    assert _r["n_outside"] >= 5 and _r["n_collision"] == 0 and _r["cmd_state"] == 0, (_n, _r["n_outside"])
    _c = case(_n)
    _reason, _, _poses = LP.score_np(_c.grid, _c.pot, _c.pose, 1024, 0, _c.ncfg, _c.cfg)
    _cell = _poses[-1][_axis] >> 10
    assert _reason == LP.OUTSIDE and _cell == (21 if _sign > 0 else -1), (_n, _cell)       # ... through that edge
_r = reference("wall_ahead")
assert _r["n_collision"] > _r["n_ok"] + _r["n_outside"] + _r["n_unreached"] and _r["cmd_state"] == 0 and _r["sw"] != 0
_a, _b = reference("unknown_blocked"), reference("unknown_allowed")
assert _a["n_collision"] > 0 and _b["n_collision"] == 0 and not np.array_equal(_a["keys"], _b["keys"])
for _n in ("lookahead_0", "lookahead_3_cells"):
    _r = reference(_n)
    assert _r["cmd_state"] == 0 and _r["sv"] == 0 and abs(_r["sw"]) == 512, (_n, _r["sv"], _r["sw"])     # an in-place rotation
assert reference("lookahead_3_cells")["score"] < reference("lookahead_0")["score"]
_r = reference("lookahead_unreached")
assert _r["n_unreached"] >= 8 and _r["n_collision"] == 0 and _r["cmd_state"] == 0       # the scored point lies in the wall
_k = reference("mirror_tie")["keys"]
assert (_k[7] >> np.uint64(14)) == (_k[8] >> np.uint64(14)) == (_k >> np.uint64(14)).min() and reference("mirror_tie")["best"] == 7
_k = reference("tie_across_workgroups")["keys"]
assert (_k[3] >> np.uint64(14)) == (_k[259] >> np.uint64(14)) == (_k >> np.uint64(14)).min() and reference("tie_across_workgroups")["best"] == 3
_r = reference("boxed_in")
assert _r["cmd_state"] == 1 and _r["n_collision"] == 81 and _r["best"] == -1 and len(_r["traj"]) == 0
assert reference("arrived")["cmd_state"] == 2 and reference("pose_outside")["cmd_state"] == 3
assert reference("pose_blocked")["cmd_state"] == 3 and reference("goal_blocked")["cmd_state"] == 4 and case("goal_blocked").goal_state == 1
_c = case("largest_weights")
assert max(int(x.pot[x.pot != N.UNREACHED].max()) for x in CASES if (x.pot != N.UNREACHED).any()) == int(_c.pot[_c.pot != N.UNREACHED].max())
assert reference("largest_weights")["cmd_state"] == 0 and reference("largest_weights")["score"] > 2 ** 24     # (no float32 holds it)

# ---- the batch: three grids of one shape with different poses and windows; the second in state 1 (every sample leaves) ----
BATCH_CFG = dict(W0, nv=8, nw=9, steps=12)
BATCH_NCFG = {}
BATCH = np.stack([COSTS_37, _open(29, 37), _costs(15, 29, 37)])
BATCH_GOALS = [(33, 14), (3, 3), (20, 25)]
BATCH_POTS = np.stack([field(("batch", b), BATCH[b], BATCH_GOALS[b], BATCH_NCFG)[0] for b in range(3)])
BATCH_POSES = np.array([centre(6, 14, 100), centre(35, 14, 0), centre(30, 5, 1400)], np.int32)
BATCH_WINDOWS = np.array([(200, 100, -120, 30), (900, 15, -40, 10), (100, 120, -200, 50)], np.int32)


@functools.lru_cache(maxsize=None)
def batch_reference(b):
    return LP.best_np(BATCH[b], BATCH_POTS[b], BATCH_POSES[b], BATCH_WINDOWS[b], BATCH_NCFG, BATCH_CFG)


assert [batch_reference(b)["cmd_state"] for b in range(3)] == [0, 1, 0] and batch_reference(1)["n_outside"] == 72
