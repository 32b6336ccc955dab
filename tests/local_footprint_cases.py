"""The shared cases of the local planner's footprint (local_planner.py, FOOTPRINT): each an FCase(name, base, probes, fcfg,
movers, mcfg) on a Case of local_plan_cases.py's kind -- grid, field, pose, window, configuration -- with a table of probes
int [P, 2] (fx, fy), a FootprintConfig dict and, for some, a table of movers with its MoverConfig dict.  The smallest shapes
at which the kernels' footprint paths can go wrong: tables of 1, 7, 8, 9, 15, 16, 17, 63, 64, 65 and 256 probes whose LAST
probe decides (the boundaries of a lane group of 8, 16 or 64 and of the finish kernel's 64-probe trips); whole outlines of
56 and 256 probes; probes at +-32767; 1, 65, LOC_BLOCK - 1, LOC_BLOCK + 1 and two chunks plus one samples; 1 and 256
steps; headings that wrap through tick 4095; probes at negative coordinates; a blocked and an outside probe on one step
in both table orders; foot_lethal 99 against 100 on a ring cell; unknown cells allowed and not; movers beside the
footprint; every state; a batch in states 0, 5 and 2; the doorway.  `reference(name)` computes best_np once per case
(through scores_np) and the tests share it; the property each case is named for is asserted here, at import, with the
restatement."""
import collections
import functools

import numpy as np

import local_plan_cases as C
import pp_amd

LP = pp_amd.local_planner
INF = pp_amd.inflation
SUB = LP.SUB
LOC_BLOCK = 256         # csrc/pp_common.h

FCase = collections.namedtuple("FCase", "name base probes fcfg movers mcfg")
CASES = []


def base(name, key, grid, goal, pose, window, cfg, ncfg=None):
    ncfg = dict(ncfg or {})
    pot, gs = C.field(key, grid, goal, ncfg)
    return C.Case(name, grid, pot, ncfg, tuple(pose), tuple(window), dict(cfg), gs)


def add(name, b, probes, movers=None, mcfg=None, **fcfg):
    p = np.asarray(probes, np.int64).reshape(-1, 2)
    p.setflags(write=False)
    m = None if movers is None else np.asarray(movers, np.int64).reshape(-1, 6)
    CASES.append(FCase(name, b, p, dict(fcfg), m, None if movers is None else dict(dict(horizon=16, mover_weight=64), **(mcfg or {}))))


def run(c, samples=None, footprint=True):
    """best_np of case c (through scores_np unless `samples` says otherwise); footprint=False: the point robot."""
    b = c.base
    return LP.best_np(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, b.goal_state, samples, c.movers, c.mcfg,
                      c.probes if footprint else None, c.fcfg if footprint else None)


def ended(c, s, probes=None):
    """(reason, the step at which sample s of case c ended) under the case's footprint (or `probes`)."""
    b = c.base
    sv, sw = LP.sample(s, b.window, b.cfg)
    out = LP.score_np(b.grid, b.pot, b.pose, sv, sw, b.ncfg, b.cfg, c.movers, c.mcfg, c.probes if probes is None else probes, c.fcfg)
    return out[0], len(out[2]) - 1


def first_bad(c, pose):
    """(index, its cell) of the first probe of case c that is not free at `pose`, or None."""
    n = pp_amd.navfn.NavfnConfig.from_any(c.base.ncfg)
    fc = LP.FootprintConfig.from_any(c.fcfg or True)
    for q, (fx, fy) in enumerate(c.probes.tolist()):
        cell = LP._probe_cell(pose[0], pose[1], pose[2], fx, fy)
        if LP._probe_value(c.base.grid, n, fc, *cell) is not False:
            return q, cell
    return None


# ---- the robot: 0.9 m x 0.5 m at 0.1 m cells, 56 probes, and the same outline at the finest spacing that fits 256 ----
RES = 0.1
RECT = LP.Footprint.rectangle(0.9, 0.5, resolution=RES)
RECT_256 = LP.Footprint.rectangle(0.9, 0.5, resolution=RES, spacing=0.11)
assert len(RECT) == 56 and len(RECT_256) == 256
FRONT_LEFT = (4608, 2560)               # the corner that meets the pillar first on a left turn


def tail(P):
    """P probes of which the first P - 1 lie within 8 sub-cells of the centre (the centre's own cell, give or take) and the
    last is the front left corner: only the last can end a sample whose centre is free."""
    near = [(i % 16 - 8, i // 16 - 8) for i in range(P - 1)]
    return np.array(near + [FRONT_LEFT], np.int64)


# ---- the room: 40 rows x 48 columns of 0.1 m, a pillar and a wall stub left of the way east, inflated by the robot's
# inscribed radius; the robot starts at cell (10, 20) ----
_RAW = np.zeros((40, 48), np.int8)
_RAW[24:27, 20:23] = 100                # the pillar
_RAW[12:15, 30] = 100                   # the stub, right of the way
INFL = dict(resolution=RES, inscribed_radius=RECT.inscribed_radius(), inflation_radius=0.6, cost_scaling_factor=4.0)
ROOM = INF.inflate_np(_RAW, INFL)
ROOM.setflags(write=False)
W0 = C.W0
GOAL = (42, 22)
R = base("room", "foot_room", ROOM, GOAL, C.centre(10, 20), (600, 100, -96, 12), dict(W0, nv=5, nw=17, steps=14))

TAILS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 256)
for _p in TAILS:
    add("tail_%d" % _p, R, tail(_p))
add("outline_56", R, RECT.probes)
add("outline_256", R, RECT_256.probes)
# ---- foot_lethal on a ring cell; unknown cells ----
add("ring_lethal_100", R, RECT.probes, foot_lethal=100)
add("ring_lethal_99", R, RECT.probes, foot_lethal=99)
add("ring_lethal_60", R, RECT.probes, foot_lethal=60)
_BAND = np.array(ROOM)
_BAND[29:, 14:30] = -1                  # unknown to the left of the way: the centre stays clear of it, the left side does not
_BAND.setflags(write=False)
for _a in (0, 1):
    add("unknown_allowed_%d" % _a, base("band%d" % _a, "foot_band", _BAND, GOAL, C.centre(10, 24, 200), (600, 100, -96, 12),
                                         dict(W0, nv=5, nw=17, steps=14), dict(allow_unknown=_a, unknown_cost=30)), RECT.probes)
# ---- the shape of the launch ----
for _n, _nv, _nw, _w in ((1, 1, 1, (1000, 0, -12, 0)), (65, 5, 13, (600, 100, -96, 16)), (LOC_BLOCK - 1, 15, 17, (600, 30, -96, 12)),
                         (LOC_BLOCK + 1, 1, 257, (900, 0, -128, 1)), (2 * LOC_BLOCK + 1, 19, 27, (600, 23, -104, 8))):
    add("samples_%d" % _n, R._replace(window=_w, cfg=dict(W0, nv=_nv, nw=_nw, steps=14)), RECT.probes)
add("steps_1", R._replace(window=(1024, 0, -512, 64), cfg=dict(W0, nv=1, nw=17, steps=1), pose=C.centre(16, 20)), RECT.probes)
add("steps_256", R._replace(window=(16, 16, -8, 4), cfg=dict(W0, nv=3, nw=5, steps=256), pose=C.centre(12, 21)), RECT.probes)
add("heading_wraps_up", R._replace(pose=C.centre(10, 20, 4090), window=(600, 100, -16, 6)), RECT.probes)
add("heading_wraps_down", R._replace(pose=C.centre(10, 30, 6), window=(600, 100, -80, 6)), RECT.probes)
# ---- the extreme probes: 32767 sub-cells are 32 cells ----
FAR = base("far", "foot_room", ROOM, GOAL, C.centre(10, 4), (300, 150, -64, 8), dict(W0, nv=3, nw=17, steps=6))
add("probes_at_plus_32767", FAR, [(32767, 0), (0, 32767), (32767, 32767)])
add("probes_at_minus_32767", FAR, [(32767, 0), (-32767, -32767)])
# ---- probes at negative coordinates: a robot that backs towards x = 0 with its rear 1.2 cells behind the centre ----
BACK = base("back", "foot_open", C.OPEN40, (5, 20), (2 * SUB + 200, 20 * SUB + 512, 0), (-900, 100, -24, 12), dict(W0, nv=6, nw=5, steps=2))
REAR = [(-1224, 300), (-1224, -300), (1000, 0)]
add("negative_coordinates", BACK, REAR)
# ---- a blocked probe and an outside probe on one step: the straight sample east along row 12 of a 24 x 24 grid ----
_EDGE = np.zeros((24, 24), np.int8)
_EDGE[14, 21] = 100
_EDGE.setflags(write=False)
EDGE = base("edge", "foot_edge", _EDGE, (23, 12), C.centre(15, 12), (512, 512, -8, 4), dict(W0, nv=2, nw=5, steps=8))
AHEAD, LEFT = (3 * SUB, 0), (0, 2 * SUB)
add("outside_then_blocked", EDGE, [AHEAD, LEFT])
add("blocked_then_outside", EDGE, [LEFT, AHEAD])
# ---- movers beside the footprint ----
_PX, _PY = R.pose[:2]
WALKER = (_PX + 9 * SUB, _PY - 6 * SUB, 0, 600, 1200, 3000)     # crosses the way from the right
add("movers_and_footprint", R, RECT.probes, movers=[WALKER], mcfg=dict(horizon=14, mover_weight=80))
add("movers_empty_table", R, RECT.probes, movers=[], mcfg=dict(horizon=14))
_S6 = LP.score_np(R.grid, R.pot, R.pose, 1000, 0, R.ncfg, R.cfg)[2]
# the straight sample's front probe and a mover meet on one step: the probe comes first in the rule
_RAW2 = np.array(ROOM)
_RAW2[20, 22] = 100
_RAW2.setflags(write=False)
R2 = base("room2", "foot_room2", _RAW2, GOAL, R.pose, (1000, 0, 0, 0), dict(W0, nv=1, nw=1, steps=14))
_K = next(k for k, p in enumerate(_S6) if (p[0] + 4608) >> 10 == 22)
add("footprint_before_dynamic", R2, [(4608, 0)], movers=[(_S6[_K][0], _S6[_K][1], 0, 0, 50, 50)], mcfg=dict(horizon=14))
# ---- the states: 2, 3 and 4 before 5; 5 before 1 ----
for _n in ("arrived", "pose_outside", "pose_blocked", "goal_blocked"):
    add("state_" + _n, C.case(_n), RECT.probes)
add("state_5_start_blocked", R._replace(pose=C.centre(16, 21, 0)), RECT.probes)       # the front left corner in the pillar
add("state_5_start_outside", R._replace(pose=C.centre(3, 20, 0)), RECT.probes)        # the rear beyond x = 0
add("state_5_before_1", C.case("boxed_in"), [(0, 0), (SUB, 0)])                    # boxed in, and a probe in the closed end
add("state_1_every_sample_footprint", R._replace(pose=C.centre(16, 20, 0), window=(900, 30, 150, 20), cfg=dict(W0, nv=3, nw=5, steps=3)), RECT.probes)

# ---- the doorway: a wall with a door of 0.8 m in 64 x 64 cells; the 0.9 m x 0.5 m robot stands in it, facing through ----
_DOOR_RAW = np.zeros((64, 64), np.int8)
_DOOR_RAW[:, 31:33] = 100               # the wall, two cells thick, along x
_DOOR_RAW[28:36, 31:33] = 0             # the door: rows 28 .. 35, 0.8 m
DOOR_INFL = dict(resolution=RES, inscribed_radius=RECT.inscribed_radius(), inflation_radius=0.5, cost_scaling_factor=5.0)
DOOR_GRID = INF.inflate_np(_DOOR_RAW, DOOR_INFL)
DOOR_GRID.setflags(write=False)
DOOR = base("door", "foot_door", DOOR_GRID, (50, 32), (31 * SUB, 32 * SUB, 0), (400, 200, -120, 20), dict(W0, nv=4, nw=13, steps=10))
add("doorway", DOOR, RECT.probes)

NAMES = [c.name for c in CASES]
assert len(set(NAMES)) == len(NAMES)


def case(name):
    return CASES[NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def reference(name):
    """best_np of the case with its footprint (through scores_np); computed once, never written to."""
    out = run(case(name))
    out["keys"].setflags(write=False)
    out["traj"].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def point(name):
    """best_np of the case without its footprint: the point robot."""
    return run(case(name), footprint=False)


def reasons(name, footprint=True):
    c, b = case(name), case(name).base
    return LP.scores_np(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, c.movers, c.mcfg, c.probes if footprint else None,
                        c.fcfg if footprint else None)[1]


# ---- the properties the cases are named for ----
for _c in CASES:
    _r, _n = reference(_c.name), _c.base.cfg["nv"] * _c.base.cfg["nw"]
    _dyn = _r.get("n_dynamic", 0)
    assert _r["n_ok"] + _r["n_outside"] + _r["n_collision"] + _r["n_unreached"] + _dyn + _r["n_footprint"] == (_n if _r["cmd_state"] < 2 else 0), _c.name
    assert _r["n_probes"] == len(_c.probes) and (_r["start_probe"] >= 0) == (_r["cmd_state"] == 5), _c.name
for _p in TAILS:
    _r = reference("tail_%d" % _p)
    assert _r["cmd_state"] == 0 and _r["n_footprint"] > 0 and _r["n_ok"] >= 8, (_p, _r["n_footprint"], _r["n_ok"])
    assert _r["n_footprint"] == reference("tail_1")["n_footprint"]
    if _p > 1:                                              # the last probe of the table counts: without it nothing ends FOOTPRINT
        _short = FCase("short", R, tail(_p)[:-1], {}, None, None)
        assert run(_short)["n_footprint"] == 0 and np.array_equal(run(_short)["keys"], point("tail_%d" % _p)["keys"]), _p
for _n in ("outline_56", "outline_256"):
    _r = reference(_n)
    assert _r["cmd_state"] == 0 and _r["n_footprint"] > point(_n)["n_collision"] and not np.array_equal(_r["keys"], point(_n)["keys"]), _n
    _who = {first_bad(case(_n), LP.score_np(R.grid, R.pot, R.pose, *LP.sample(s, R.window, R.cfg), R.ncfg, R.cfg, None, None, case(_n).probes)[2][-1])[0]
            for s in np.flatnonzero(reasons(_n) == LP.FOOTPRINT)}
    assert len(_who) >= 3 and max(_who) >= len(case(_n).probes) // 4, (_n, sorted(_who))     # probes far along the table decide
assert reference("ring_lethal_60")["n_footprint"] > reference("ring_lethal_99")["n_footprint"] > reference("ring_lethal_100")["n_footprint"] > 0
assert reference("ring_lethal_99")["cmd_state"] == reference("ring_lethal_60")["cmd_state"] == 0
_a, _b = reference("unknown_allowed_0"), reference("unknown_allowed_1")
assert _a["cmd_state"] == _b["cmd_state"] == 0 and _a["n_footprint"] > _b["n_footprint"] > 0
for _n, _want in ((1, 1), (65, 65), (255, 255), (257, 257), (513, 513)):
    _c = case("samples_%d" % _n)
    assert _c.base.cfg["nv"] * _c.base.cfg["nw"] == _want and reference(_c.name)["cmd_state"] == 0, _n
    assert _n == 1 or (reference(_c.name)["n_footprint"] > 0 and reference(_c.name)["n_ok"] >= 8), (_n, reference(_c.name)["n_footprint"])
assert reference("samples_257")["best"] >= 64 and reference("samples_513")["best"] >= LOC_BLOCK
assert reference("steps_1")["n_footprint"] > 0 and reference("steps_1")["cmd_state"] == 0
assert case("steps_256").base.cfg["steps"] == LP.PP_LOCAL_MAX_STEPS and reference("steps_256")["cmd_state"] == 0
assert reference("steps_256")["n_footprint"] > 0 and len({ended(case("steps_256"), s)[1] for s in range(15)}) >= 3       # ... at different steps
for _n, _up in (("heading_wraps_up", True), ("heading_wraps_down", False)):     # a sample ends FOOTPRINT under a heading beyond the wrap
    _c, _hit = case(_n), False
    for _s in np.flatnonzero(reasons(_n) == LP.FOOTPRINT):
        _b = _c.base
        _d = np.diff([p[2] for p in LP.score_np(_b.grid, _b.pot, _b.pose, *LP.sample(_s, _b.window, _b.cfg), _b.ncfg, _b.cfg, None, None, _c.probes)[2]])
        _hit = _hit or bool(((_d < -2048) if _up else (_d > 2048)).any())
    assert _hit and reference(_n)["cmd_state"] == 0 and reference(_n)["n_ok"] >= 8, _n
_r = reference("probes_at_plus_32767")
assert _r["cmd_state"] == 0 and _r["n_outside"] > 0 and _r["n_ok"] >= 8 and point("probes_at_plus_32767")["n_outside"] == 0
_r = reference("probes_at_minus_32767")
assert _r["cmd_state"] == 5 and _r["start_probe"] == 1 and (_r["keys"] == LP.INVALID).all() and _r["n_outside"] == 0
_c = case("negative_coordinates")
_r = reference(_c.name)
assert _r["cmd_state"] == 0 and _r["n_outside"] > 0 and point(_c.name)["n_outside"] == 0
_s = int(np.flatnonzero(reasons(_c.name) == LP.OUTSIDE)[0])
_pose = LP.score_np(BACK.grid, BACK.pot, BACK.pose, *LP.sample(_s, BACK.window, BACK.cfg), BACK.ncfg, BACK.cfg, None, None, _c.probes)[2][-1]
_q, _cell = first_bad(_c, _pose)
_C, _S = (int(v) for v in LP.trig_table()[_pose[2]])
_x = _pose[0] + ((_c.probes[_q][0] * _C - _c.probes[_q][1] * _S + 8192) >> 14)
assert _cell[0] == -1 and -SUB < _x < 0 and _pose[0] >> 10 == 0        # X in (-1024, 0): cell -1 by the floor shift, cell 0 by a truncation
assert LP.sample(7, EDGE.window, EDGE.cfg) == (1024, 0)
assert ended(case("outside_then_blocked"), 7) == (LP.OUTSIDE, 6) and ended(case("blocked_then_outside"), 7) == (LP.FOOTPRINT, 6)
assert ended(case("outside_then_blocked"), 7, [AHEAD]) == (LP.OUTSIDE, 6) and ended(case("outside_then_blocked"), 7, [LEFT]) == (LP.FOOTPRINT, 6)
assert reference("outside_then_blocked")["cmd_state"] == reference("blocked_then_outside")["cmd_state"] == 0
_r = reference("movers_and_footprint")
assert _r["cmd_state"] == 0 and _r["n_dynamic"] > 0 and _r["n_footprint"] > 0 and _r["n_ok"] >= 8 and _r["near"] >= 0
assert np.array_equal(reference("movers_empty_table")["keys"], reference("outline_56")["keys"])
assert ended(case("footprint_before_dynamic"), 0) == (LP.FOOTPRINT, _K)
assert LP.score_np(R2.grid, R2.pot, R2.pose, 1000, 0, R2.ncfg, R2.cfg, case("footprint_before_dynamic").movers, case("footprint_before_dynamic").mcfg)[0] == LP.DYNAMIC
for _n, _s in (("arrived", 2), ("pose_outside", 3), ("pose_blocked", 3), ("goal_blocked", 4)):
    _r = reference("state_" + _n)
    assert _r["cmd_state"] == _s and _r["start_probe"] == -1 and _r["n_footprint"] == 0 and (_r["keys"] == LP.INVALID).all()
_r = reference("state_5_start_blocked")
assert _r["cmd_state"] == 5 and _r["best"] == -1 and len(_r["traj"]) == 0 and point("state_5_start_blocked")["cmd_state"] == 0
assert first_bad(case("state_5_start_blocked"), case("state_5_start_blocked").base.pose)[0] == _r["start_probe"] > 0
_r = reference("state_5_start_outside")
assert _r["cmd_state"] == 5 and first_bad(case("state_5_start_outside"), case("state_5_start_outside").base.pose)[1][0] < 0
assert reference("state_5_before_1")["cmd_state"] == 5 and reference("state_5_before_1")["start_probe"] == 1 and point("state_5_before_1")["cmd_state"] == 1
_r = reference("state_1_every_sample_footprint")
assert _r["cmd_state"] == 1 and _r["n_footprint"] > 0 and _r["n_ok"] == 0 and point("state_1_every_sample_footprint")["cmd_state"] == 0

# ---- the batch: three grids of the room's shape in states 0, 5 and 2, so that workgroups that return at once and workgroups
# that roll share a launch ----
BATCH_CFG = dict(W0, nv=5, nw=17, steps=14)
BATCH_NCFG = {}
BATCH = np.stack([ROOM, ROOM, ROOM])
BATCH_POTS = np.stack([R.pot, R.pot, R.pot])
BATCH_POSES = np.array([R.pose, C.centre(16, 21, 0), C.centre(*GOAL, 500)], np.int32)
BATCH_WINDOWS = np.array([R.window, (500, 100, -60, 10), R.window], np.int32)
BATCH_PROBES = RECT.probes


@functools.lru_cache(maxsize=None)
def batch_reference(b):
    return LP.best_np(BATCH[b], BATCH_POTS[b], BATCH_POSES[b], BATCH_WINDOWS[b], BATCH_NCFG, BATCH_CFG, footprint=BATCH_PROBES)


assert [batch_reference(b)["cmd_state"] for b in range(3)] == [0, 5, 2] and batch_reference(0)["n_footprint"] > 0
