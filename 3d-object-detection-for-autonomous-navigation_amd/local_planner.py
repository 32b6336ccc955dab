"""Local planner over an inflated int8 grid in the layout of nav_msgs/OccupancyGrid and the cost-to-go field of navfn.py:
a window of (v, w) samples rolled forward from the robot's pose, each scored on the field, and the best one as the velocity
command -- the stage that reads the field.  A fifth, opt-in stage behind the navigation function of the costmap or of the
rolling occupancy maps, and a stand-alone call for any such grid and field.

The reference has no such path, so nothing here is parity with it.  This module STATES the rule: `score_np` (one sample,
literally step by step in Python ints), `scores_np` (all samples of a window at once as numpy arrays, step-major with
masks, an independent second statement) and `best_np` are the restatement that the GPU (csrc/local_plan.hip behind
Engine.set_local_planner / local_plan_async / drive, and `local_plan`) equals with no tolerance.  Everything is integer
arithmetic; metres, radians and seconds become integers here on the host (`pose_ticks`, `LocalLimits.window`).

UNITS.  A position is int32 sub-cells, SUB = 1024 per cell; a heading is one of HEADINGS = 4096 ticks per revolution, tick
0 along +x, ticks growing towards +y.  C[h], S[h] = rint(cos / sin(2 pi h / 4096) * 2^14) as int32 (`trig_table`, computed
in float64 on the host and uploaded with the configuration; the device only looks it up).

INPUT per grid: the inflated grid g[H, W], the field pot uint32 [H, W], a pose (X, Y, h) (h is taken & 4095), a window
(v0, dv, w0, dw); the configuration fixes nv, nw and steps.  Sample s = i * nw + j has sv = v0 + i * dv sub-cells per
step (negative: reverse) and sw = w0 + j * dw ticks per step; every sample must satisfy |sv| <= 1024 and |sw| <= 512,
so a step never moves more than one cell along an axis.

ROLLOUT.  For k = 1 .. steps: X += (sv * C[h] + 8192) >> 14, Y += (sv * S[h] + 8192) >> 14, then h = (h + sw) & 4095 --
the move uses the old heading and the shift is arithmetic (floor).  The cell is (X >> 10, Y >> 10).  A cell outside the
grid ends the sample as OUTSIDE (reason 1); a blocked one -- g >= lethal_cost, or unknown while allow_unknown is 0, of the
NavfnConfig the field was made with -- as COLLISION (reason 2); otherwise occ = max(occ, g), unknown_cost standing in for
an unknown cell.  After the last step the scored point is the end pose pushed `lookahead` sub-cells along the final
heading, rounded like a step (0: the end cell itself); a scored cell that is outside, blocked or UNREACHED makes the
sample UNREACHED (reason 3).

SCORE.  score = pot_weight * pot(scored cell) + occ_weight * occ + speed_weight * (1024 - |sv|) + turn_weight * |sw|, below
2^41 by the configuration's ranges; key = (score << 14) | s, 2^64 - 1 for an invalid sample.  The command is the sample
with the least key: the lowest index wins a tie.

STATES.  cmd_state, the first that applies: 4 the field has no goal (navfn goal_state != 0); 3 the pose's cell is outside
the grid, blocked or UNREACHED; 2 arrived, pot at the pose's cell is 0; 1 no valid sample; 0 ok.  In states 1 .. 4 the
command is (0, 0), best = -1 and the trajectory is empty; in states 2 .. 4 no sample is rolled, every key is invalid and
the counts are 0.

Results per grid: cmd_state, best, sv, sw; the counts n_ok, n_outside, n_collision, n_unreached; score; the winning
trajectory int32 [steps + 1, 3] poses, the start included; all nv * nw keys uint64 on request.

MOVERS (opt-in: `movers=` / `mcfg=` here, Engine.set_local_movers behind an engine).  The grid has no time; a mover has.
A mover is six int32 (mx, my, mvx, mvy, r_hard, r_soft): its position at step 0 in sub-cells of the grid's frame (it may
lie outside the grid), its movement per rollout step, and two radii, all in sub-cells; |mx|, |my| <= 2^29, |mvx|, |mvy|
<= PP_LOCAL_MAX_MOVER_SPEED = 16384, 0 <= r_hard <= r_soft <= PP_LOCAL_MAX_MOVER_RADIUS = 32767, at most
PP_LOCAL_MAX_MOVERS = 64 per grid.  MoverConfig.horizon (0 .. 256) is the steps over which a prediction is trusted,
mover_weight (0 .. 65535) what a near miss costs.  The rollout is unchanged up to and including the static test of step
k (OUTSIDE, then COLLISION, then occ).  A sample still alive then, with k <= horizon, looks at every mover in table
order: dx = X - (mx + k * mvx), dy = Y - (my + k * mvy), d2 = dx * dx + dy * dy, exact integers (int64 holds them); d2 <=
r_hard^2 ends the sample as DYNAMIC (reason 4; later movers and steps are not looked at), otherwise d2 <= r_soft^2 sets
near = max(near, horizon + 1 - k): an earlier near miss weighs more.  Neither the start pose (k = 0) nor the lookahead
point is tested against movers.  The score gains mover_weight * near and stays below 2^41; key, tie rule and states are
unchanged, so where every sample ends invalid cmd_state is 1 and the robot stops for a pedestrian it cannot pass.
Further results per grid (MOVER_INFO): n_movers (-1: see below), n_skipped, n_dynamic and near, the winner's (0 unless
cmd_state is 0); n_ok + n_outside + n_collision + n_unreached + n_dynamic = nv * nw in states 0 and 1.

FROM TRACKS TO MOVERS (`movers_np`; k_local_movers on the GPU, where the track table lies).  Float64, operation by
operation in this order, floor, rint (half to even) and ceil the only roundings, no sqrt, no trig.  A track row gives x y
z vx vy vz w l in the grid's frame: the slot as it stands for the costmap source (`Engine.tracks()`), the slot carried into
the fixed frame by the pose of the stream's last posed tracking step for the occupancy source (`Engine.tracks_fixed()`; a
stream without one has n_movers = -1 and is rolled with no movers).  With the grid's origin (ox, oy) and resolution res
in metres and dt seconds per step: MX = floor(((x - ox) / res) * 1024.0), MY likewise; MVX = rint(((vx * dt) / res) *
1024.0), MVY likewise; RH = ceil(((fmax(w, l) * 0.5 + pad_hard) / res) * 1024.0) and RS with pad_soft, both clipped to [0,
32767] -- the planner's robot is a point, so its radius belongs in the pads.  A live row (a confirmed one where
confirmed_only is set) becomes a mover in ascending slot order; one with a non-finite input, |MX| or |MY| > 2^29 or |MVX|
or |MVY| > 16384 is skipped and counted in n_skipped.

FOOTPRINT (opt-in: `footprint=` / `fcfg=` here, Engine.set_local_footprint behind an engine).  Without one the robot is a
point on the inflated grid: its CENTRE keeps an inscribed radius from obstacles, which is exact only for a disc.  A
footprint is a table of P probe points (fx, fy) in the robot's frame, int32 sub-cells, x forward along heading tick h, y to
the left; 1 <= P <= PP_LOCAL_MAX_PROBES = 256, |fx|, |fy| <= PP_LOCAL_MAX_PROBE = 32767, so 32767 * 16384 * 2 + 8192 <
2^31 and the rotation fits int32.  PROBES: at a pose (X, Y, h) probe q lies at (X + ((fx * C[h] - fy * S[h] + 8192) >> 14),
Y + ((fx * S[h] + fy * C[h] + 8192) >> 14)); its cell is that >> 10, the shift arithmetic, so a negative coordinate is a
cell outside the grid.  TEST: a probe's cell is OUTSIDE the grid; BLOCKED if g >= foot_lethal (FootprintConfig, 1 .. 100,
default 100) or if it is unknown while the NavfnConfig's allow_unknown is 0; free otherwise.  Inflation leaves exactly 100
on obstacle cells and 99 on the inscribed ring, so with the default the corners may enter the ring -- which is the point:
inflate by `Footprint.inscribed_radius()` and let the probes keep the corners off the obstacles.  Probes never contribute
to occ, which stays the centre's alone (every close pass would cost 99 otherwise).  ROLLOUT: step k is unchanged up to
and including the centre's static test (OUTSIDE, COLLISION, occ); a sample still alive then looks at the probes in table
order under the heading AFTER the step's turn (the pose stored in the trajectory), and the first probe that is not free
ends it: as OUTSIDE (reason 1) if its cell is outside, as FOOTPRINT (reason 5) if blocked.  Then the movers' test runs,
unchanged, if movers are on.  The lookahead point is the centre's only.  STATE 5: the footprint at the start pose has a
probe that is not free; the order of the states is 4, 3, 2, 5, 1, 0, and in state 5 no sample is rolled, the command is
(0, 0), best = -1, the trajectory is empty, every key is invalid and the counts are 0.  Further results per grid
(FOOT_INFO): n_probes, n_footprint (samples ended with reason 5; a probe that is outside counts in n_outside) and
start_probe, the index of the first probe that is not free at the start pose, -1 if none or if the state is 2 .. 4; n_ok +
n_outside + n_collision + n_unreached + n_dynamic + n_footprint = nv * nw in states 0 and 1.  With footprint=None every
function returns exactly what it returned before.

FROM METRES TO PROBES (`Footprint`, host only, float64).  `Footprint.polygon(vertices_m, resolution, spacing=0.5)` takes the
vertices in order, closed implicitly; an edge of length L gives n = max(1, ceil(L / (spacing * resolution))) points at
the fractions i / n, i = 0 .. n - 1, each rint((p / resolution) * 1024.0); duplicates are dropped, the first kept.  It is
the OUTLINE only, no interior: a step moves the centre at most one cell and the outline is sampled every half cell, so
the outline cannot jump an obstacle cell that the start pose did not already contain -- as long as a step's turn moves
no probe by more than about a cell either (|sw| * circumscribed radius <= about 650 cells * ticks; a long robot that spins
fast can sweep a corner across a thin wall between two steps).

Out of scope: escaping from a blocked pose, footprints other than a point on the inflated grid for the robot unless a
footprint is set (against a
mover its radius rides in pad_hard / pad_soft), holonomic (vy) samples, oscillation suppression between cycles,
goal-orientation alignment, a diagonal step passing between two blocked cells that touch only at a corner (an inscribed
radius of one cell or more rules this out), a configuration key, any ROS import.  Of the movers: swept collision between
two steps (a fast mover can tunnel through a small radius), rectangular mover shapes, a lead time between the tracks' stamp
and now, movers that react to the robot.  Of the footprint: filled footprints (interior cells), the area swept between two
steps, a footprint-aware inflation or navigation function (both keep the inscribed radius), a skip of the probe test where
the centre's cost proves the circumscribed circle free (a natural follow-up), rectangular movers, escaping from state 5,
holonomic samples.
"""
import ctypes
import dataclasses
import math

import numpy as np

from . import _lib
from . import navfn as _nav
from ._lib import (PP_LOCAL_FOOT_INFO, PP_LOCAL_HEADINGS, PP_LOCAL_MAX_LOOKAHEAD, PP_LOCAL_MAX_MOVER_RADIUS,
                   PP_LOCAL_MAX_MOVER_SPEED, PP_LOCAL_MAX_MOVERS, PP_LOCAL_MAX_PROBE, PP_LOCAL_MAX_PROBES, PP_LOCAL_MAX_SAMPLES,
                   PP_LOCAL_MAX_STEPS, PP_LOCAL_MOVER_INFO, PP_LOCAL_SUB, PP_OCC_MAX_CELLS, PP_TRACK_MAX)

SUB = PP_LOCAL_SUB
HEADINGS = PP_LOCAL_HEADINGS
ONE = 1 << 14                           # the trig table's 1.0
MAX_SV, MAX_SW = 1024, 512              # |sv| sub-cells and |sw| ticks per step at most
INVALID = 2 ** 64 - 1                   # the key of a sample that did not end OK
OK, OUTSIDE, COLLISION, UNREACHED = 0, 1, 2, 3      # why a sample ended
DYNAMIC = 4                             # ... within r_hard of a mover (only with movers)
FOOTPRINT = 5                           # ... on a blocked probe of the footprint (only with a footprint)
MAX_MOVER_POS = 1 << 29                 # |mx|, |my| at most
MOVER_INFO = ("n_movers", "n_skipped", "n_dynamic", "near")      # pp_get_local_movers' words
STATE_OK, STATE_NO_SAMPLE, STATE_ARRIVED, STATE_POSE, STATE_NO_GOAL = 0, 1, 2, 3, 4
STATE_FOOTPRINT = 5                     # a probe of the footprint is not free at the start pose (behind 4, 3, 2; before 1, 0)
FOOT_INFO = ("n_probes", "n_footprint", "start_probe")      # pp_get_local_footprint's words (a fourth is reserved, 0)
RESULT = ("cmd_state", "best", "sv", "sw", "n_ok", "n_outside", "n_collision", "n_unreached")      # pp_get_local_plan's words

_RANGES = (("nv", 1, PP_LOCAL_MAX_SAMPLES), ("nw", 1, PP_LOCAL_MAX_SAMPLES), ("steps", 1, PP_LOCAL_MAX_STEPS),
           ("lookahead", 0, PP_LOCAL_MAX_LOOKAHEAD), ("pot_weight", 0, 255), ("occ_weight", 0, 65535),
           ("speed_weight", 0, 65535), ("turn_weight", 0, 65535))
MAX_SCORE = 255 * (_nav.UNREACHED - 1) + 65535 * 100 + 65535 * 1024 + 65535 * 512
MAX_SCORE_MOVERS = MAX_SCORE + 65535 * PP_LOCAL_MAX_STEPS   # mover_weight * near: near <= horizon + 1 - 1 <= 256
assert SUB == 1 << 10 and HEADINGS == 1 << 12 and MAX_SV == SUB and PP_LOCAL_MAX_SAMPLES == 1 << 14
assert MAX_SCORE < MAX_SCORE_MOVERS < 2 ** 41                             # so (score << 14) | s < 2^55 never reaches INVALID
# X and Y fit int32: a rolled pose lies in the grid, a step moves at most one cell and a sample ends at its first cell
# outside; the scored point adds the lookahead
assert (PP_OCC_MAX_CELLS + 1) * SUB + PP_LOCAL_MAX_LOOKAHEAD < 2 ** 31
assert MAX_SV * ONE + 8192 < 2 ** 31 and PP_LOCAL_MAX_LOOKAHEAD * ONE + 8192 < 2 ** 31       # the products do too
# a mover's position at step k <= 256 fits int32, and dx = X - position too: X is compared only behind the static test,
# which left it inside the grid (0 <= X < 2^20 cells); d2 = dx * dx + dy * dy then fits int64
_MAX_MPOS = MAX_MOVER_POS + PP_LOCAL_MAX_STEPS * PP_LOCAL_MAX_MOVER_SPEED
_MAX_DX = PP_OCC_MAX_CELLS * SUB + _MAX_MPOS
assert _MAX_MPOS < 2 ** 31 and _MAX_DX < 2 ** 31 and 2 * _MAX_DX * _MAX_DX < 2 ** 63
assert PP_LOCAL_MAX_MOVER_RADIUS ** 2 < 2 ** 31 and PP_LOCAL_MAX_MOVERS == PP_TRACK_MAX and len(MOVER_INFO) == PP_LOCAL_MOVER_INFO
# a probe: two int16; its rotation fits int32, and so does X + rx, because a pose whose probes are looked at lies in the grid
assert PP_LOCAL_MAX_PROBE == 32767 and PP_LOCAL_MAX_PROBES == 256 and len(FOOT_INFO) + 1 == PP_LOCAL_FOOT_INFO
assert PP_LOCAL_MAX_PROBE * ONE * 2 + 8192 < 2 ** 31
assert (PP_OCC_MAX_CELLS + 1) * SUB + 2 * PP_LOCAL_MAX_PROBE + 1 < 2 ** 31


@dataclasses.dataclass
class LocalPlanConfig:
    """nv, nw          >= 1, nv * nw <= 16384: velocity and turn-rate samples of a window
    steps           1 .. 256: steps of a rollout
    lookahead       0 .. 16384 sub-cells: how far beyond the end pose, along the final heading, the field is read
    pot_weight      0 .. 255
    occ_weight, speed_weight, turn_weight   0 .. 65535"""
    nv: int = 9
    nw: int = 21
    steps: int = 32
    lookahead: int = 0
    pot_weight: int = 32
    occ_weight: int = 16
    speed_weight: int = 1
    turn_weight: int = 1

    def __post_init__(self):
        for f, lo, hi in _RANGES:
            v = getattr(self, f)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"LocalPlanConfig: {f} must be an integer, got {v!r}")
            if int(v) < lo or int(v) > hi:
                raise ValueError(f"LocalPlanConfig: {f} = {v} outside [{lo}, {hi}]")
            setattr(self, f, int(v))
        if self.nv * self.nw > PP_LOCAL_MAX_SAMPLES:
            raise ValueError(f"LocalPlanConfig: nv * nw = {self.nv * self.nw} samples, at most PP_LOCAL_MAX_SAMPLES = {PP_LOCAL_MAX_SAMPLES}")

    def to_dict(self):
        return dataclasses.asdict(self)

    @classmethod
    def from_any(cls, cfg):
        """A LocalPlanConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"local_planner: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"local_planner: a LocalPlanConfig, a dict of its fields or True, got {cfg!r}")


@dataclasses.dataclass
class MoverConfig:
    """horizon         0 .. 256: rollout steps over which a mover's prediction is trusted (0: movers are never tested)
    mover_weight    0 .. 65535: what one unit of `near` adds to the score
    pad_hard        metres, finite, >= 0: added to max(w, l) / 2 for r_hard -- the robot's radius belongs here
    pad_soft        metres, finite, >= pad_hard: ... for r_soft
    confirmed_only  only confirmed tracks become movers"""
    horizon: int = 32
    mover_weight: int = 64
    pad_hard: float = 0.3
    pad_soft: float = 0.8
    confirmed_only: bool = True

    def __post_init__(self):
        for f, lo, hi in (("horizon", 0, PP_LOCAL_MAX_STEPS), ("mover_weight", 0, 65535)):
            v = getattr(self, f)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"MoverConfig: {f} must be an integer, got {v!r}")
            if int(v) < lo or int(v) > hi:
                raise ValueError(f"MoverConfig: {f} = {v} outside [{lo}, {hi}]")
            setattr(self, f, int(v))
        for f in ("pad_hard", "pad_soft"):
            v = getattr(self, f)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
                raise ValueError(f"MoverConfig: {f} must be a finite number of metres, got {v!r}")
            setattr(self, f, float(v))
        if not 0.0 <= self.pad_hard <= self.pad_soft:
            raise ValueError(f"MoverConfig: pad_hard = {self.pad_hard}, pad_soft = {self.pad_soft}: 0 <= pad_hard <= pad_soft")
        if not isinstance(self.confirmed_only, (bool, np.bool_)) and self.confirmed_only not in (0, 1):
            raise ValueError(f"MoverConfig: confirmed_only must be a bool, got {self.confirmed_only!r}")
        self.confirmed_only = bool(self.confirmed_only)

    def to_dict(self):
        return dataclasses.asdict(self)

    @classmethod
    def from_any(cls, cfg):
        """A MoverConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"local_planner: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"local_planner: a MoverConfig, a dict of its fields or True, got {cfg!r}")


def check_movers(movers, who="local_planner"):
    """int64 [n, 6] (mx, my, mvx, mvy, r_hard, r_soft) of at most PP_LOCAL_MAX_MOVERS movers; raises, naming the mover,
    unless each lies within the ranges the rule's integer widths rest on."""
    a = np.asarray(movers)
    if a.size == 0:
        return np.zeros((0, 6), np.int64)
    if a.ndim != 2 or a.shape[1] != 6 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{who}: movers must be integers [n, 6] (mx, my, mvx, mvy, r_hard, r_soft), got {a.dtype} {a.shape}")
    if a.shape[0] > PP_LOCAL_MAX_MOVERS:
        raise ValueError(f"{who}: {a.shape[0]} movers, at most PP_LOCAL_MAX_MOVERS = {PP_LOCAL_MAX_MOVERS}")
    a = a.astype(np.int64)
    for m, (mx, my, mvx, mvy, rh, rs) in enumerate(a.tolist()):
        if max(abs(mx), abs(my)) > MAX_MOVER_POS:
            raise ValueError(f"{who}: mover {m}: position ({mx}, {my}) outside [-2^29, 2^29]")
        if max(abs(mvx), abs(mvy)) > PP_LOCAL_MAX_MOVER_SPEED:
            raise ValueError(f"{who}: mover {m}: movement ({mvx}, {mvy}) per step outside [-{PP_LOCAL_MAX_MOVER_SPEED}, {PP_LOCAL_MAX_MOVER_SPEED}]")
        if not 0 <= rh <= rs <= PP_LOCAL_MAX_MOVER_RADIUS:
            raise ValueError(f"{who}: mover {m}: radii r_hard = {rh}, r_soft = {rs}, not 0 <= r_hard <= r_soft <= {PP_LOCAL_MAX_MOVER_RADIUS}")
    return a


def _mover_args(movers, mcfg, who):
    """(None, None) without movers; else (int64 [n, 6], MoverConfig)."""
    if movers is None:
        if mcfg is not None:
            raise ValueError(f"{who}: mcfg without movers (an empty table is movers=[])")
        return None, None
    if mcfg is None:
        raise ValueError(f"{who}: movers need mcfg (a MoverConfig, a dict of its fields or True)")
    return check_movers(movers, who), MoverConfig.from_any(mcfg)


@dataclasses.dataclass
class FootprintConfig:
    """foot_lethal     1 .. 100: a probe's cell with g >= foot_lethal is blocked (100: obstacle cells only, so the corners may
                    enter the inscribed ring that inflation marks 99)"""
    foot_lethal: int = 100

    def __post_init__(self):
        v = self.foot_lethal
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"FootprintConfig: foot_lethal must be an integer, got {v!r}")
        if int(v) < 1 or int(v) > 100:
            raise ValueError(f"FootprintConfig: foot_lethal = {v} outside [1, 100]")
        self.foot_lethal = int(v)

    def to_dict(self):
        return dataclasses.asdict(self)

    @classmethod
    def from_any(cls, cfg):
        """A FootprintConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"local_planner: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"local_planner: a FootprintConfig, a dict of its fields or True, got {cfg!r}")


def check_probes(probes, who="local_planner"):
    """int64 [P, 2] (fx, fy) of 1 .. PP_LOCAL_MAX_PROBES probes; raises, naming the probe, unless |fx|, |fy| <=
    PP_LOCAL_MAX_PROBE."""
    a = np.asarray(probes)
    if a.ndim != 2 or a.shape[1] != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{who}: probes must be integers [P, 2] (fx, fy), got {a.dtype} {a.shape}")
    if not 1 <= a.shape[0] <= PP_LOCAL_MAX_PROBES:
        raise ValueError(f"{who}: {a.shape[0]} probes, 1 to PP_LOCAL_MAX_PROBES = {PP_LOCAL_MAX_PROBES}")
    a = a.astype(np.int64)
    for q, (fx, fy) in enumerate(a.tolist()):
        if max(abs(fx), abs(fy)) > PP_LOCAL_MAX_PROBE:
            raise ValueError(f"{who}: probe {q}: ({fx}, {fy}) outside [-{PP_LOCAL_MAX_PROBE}, {PP_LOCAL_MAX_PROBE}]")
    return a


class Footprint:
    """The robot as a table of probes int64 [P, 2] (fx, fy) in sub-cells of its own frame, x forward, y to the left
    (`probes`), as the rule takes it.  `Footprint(probes)` takes the table itself; `Footprint.polygon` and
    `Footprint.rectangle` make it from metres (host only, float64) and remember the outline for the two radii."""

    def __init__(self, probes, vertices=None):
        self.probes = check_probes(probes, "Footprint")
        self.probes.setflags(write=False)
        self.vertices = None if vertices is None else np.array(vertices, np.float64)

    def __len__(self):
        return len(self.probes)

    def __eq__(self, other):
        return isinstance(other, Footprint) and np.array_equal(self.probes, other.probes)

    def __repr__(self):
        return f"Footprint({len(self.probes)} probes)"

    @classmethod
    def polygon(cls, vertices_m, resolution, spacing=0.5):
        """The outline of the polygon with the vertices float [n, 2] metres in the robot's frame, in order, closed
        implicitly, sampled every `spacing` cells of `resolution` metres: an edge of length L gives n = max(1, ceil(L /
        (spacing * resolution))) points at the fractions i / n, i = 0 .. n - 1, each rint((p / resolution) * 1024.0);
        duplicates are dropped, the first kept.  Refused, with the reason named: fewer than 3 vertices, the origin (the
        point the planner rolls) not strictly inside, a probe out of range, more than PP_LOCAL_MAX_PROBES probes."""
        v = np.asarray(vertices_m, np.float64)
        res, spacing = float(resolution), float(spacing)
        if v.ndim != 2 or v.shape[1] != 2 or not np.isfinite(v).all():
            raise ValueError(f"Footprint.polygon: vertices must be finite metres [n, 2], got {np.asarray(vertices_m).shape}")
        if len(v) < 3:
            raise ValueError(f"Footprint.polygon: {len(v)} vertices, fewer than 3")
        if not (math.isfinite(res) and res > 0.0):
            raise ValueError(f"Footprint.polygon: resolution = {res} must be finite and > 0")
        if not (math.isfinite(spacing) and spacing > 0.0):
            raise ValueError(f"Footprint.polygon: spacing = {spacing} must be finite and > 0")
        if not _origin_strictly_inside(v):
            raise ValueError("Footprint.polygon: the origin is not strictly inside the polygon")
        probes, seen = [], set()
        for a, b in zip(v, np.roll(v, -1, axis=0)):
            n = max(1, math.ceil(math.hypot(b[0] - a[0], b[1] - a[1]) / (spacing * res)))
            for i in range(n):
                pt = a + (b - a) * (i / n)
                q = (int(np.rint((pt[0] / res) * 1024.0)), int(np.rint((pt[1] / res) * 1024.0)))
                if max(abs(q[0]), abs(q[1])) > PP_LOCAL_MAX_PROBE:
                    raise ValueError(f"Footprint.polygon: the probe ({q[0]}, {q[1]}) at ({pt[0]:g}, {pt[1]:g}) m is out of range "
                                     f"[-{PP_LOCAL_MAX_PROBE}, {PP_LOCAL_MAX_PROBE}] sub-cells")
                if q not in seen:
                    seen.add(q)
                    probes.append(q)
        if len(probes) > PP_LOCAL_MAX_PROBES:
            raise ValueError(f"Footprint.polygon: {len(probes)} probes, more than PP_LOCAL_MAX_PROBES = {PP_LOCAL_MAX_PROBES} (a larger spacing)")
        return cls(np.array(probes, np.int64), v)

    @classmethod
    def rectangle(cls, length, width, offset_x=0.0, *, resolution, spacing=0.5):
        """The rectangle `length` metres along x and `width` metres along y whose centre lies offset_x metres in front of
        the origin, counter-clockwise from the rear right corner."""
        l, w, o = float(length), float(width), float(offset_x)
        if not (math.isfinite(l) and math.isfinite(w) and l > 0.0 and w > 0.0 and math.isfinite(o)):
            raise ValueError(f"Footprint.rectangle: length = {l}, width = {w}, offset_x = {o}: finite, length and width > 0")
        return cls.polygon([(o - l / 2, -w / 2), (o + l / 2, -w / 2), (o + l / 2, w / 2), (o - l / 2, w / 2)], resolution, spacing)

    def _outline(self, who):
        if self.vertices is None:
            raise ValueError(f"Footprint.{who}: a footprint given as probes has no outline in metres")
        return self.vertices

    def inscribed_radius(self):
        """Metres from the origin to the nearest point of the outline: what belongs in InflationConfig.inscribed_radius
        (the centre then keeps that far from obstacles, and the probes look after the rest of the robot)."""
        v = self._outline("inscribed_radius")
        return min(_segment_distance(a, b) for a, b in zip(v, np.roll(v, -1, axis=0)))

    def circumscribed_radius(self):
        """Metres from the origin to the farthest vertex: beyond it nothing can touch the robot."""
        return float(np.hypot(*self._outline("circumscribed_radius").T).max())


def _segment_distance(a, b):
    """Metres from the origin to the segment a - b."""
    d = b - a
    t = min(max(float(-(a @ d) / (d @ d)), 0.0), 1.0) if float(d @ d) > 0.0 else 0.0
    return float(np.hypot(*(a + t * d)))


def _origin_strictly_inside(v):
    """The crossing number of the ray from the origin along +x is odd, and the origin lies on no edge."""
    inside = False
    for a, b in zip(v, np.roll(v, -1, axis=0)):
        if _segment_distance(a, b) == 0.0:
            return False
        if (a[1] > 0.0) != (b[1] > 0.0) and a[0] + (0.0 - a[1]) * (b[0] - a[0]) / (b[1] - a[1]) > 0.0:
            inside = not inside
    return inside


def _foot_args(footprint, fcfg, who):
    """(None, None) without a footprint; else (probes int64 [P, 2], FootprintConfig): a Footprint or a table of probes, and
    fcfg a FootprintConfig, a dict of its fields, True or None (the defaults)."""
    if footprint is None:
        if fcfg is not None:
            raise ValueError(f"{who}: fcfg without a footprint")
        return None, None
    probes = footprint.probes if isinstance(footprint, Footprint) else check_probes(footprint, who)
    return probes, FootprintConfig.from_any(True if fcfg is None else fcfg)


def _probe_cell(X, Y, h, fx, fy):
    """The cell of probe (fx, fy) at the pose (X, Y, h), in Python ints."""
    C, S = int(_TRIG[h, 0]), int(_TRIG[h, 1])
    assert abs(fx * C - fy * S) + 8192 < 2 ** 31 and abs(fx * S + fy * C) + 8192 < 2 ** 31
    return (X + ((fx * C - fy * S + 8192) >> 14)) >> 10, (Y + ((fx * S + fy * C + 8192) >> 14)) >> 10


def _probe_value(g, n, fc, cx, cy):
    """The rule's reading of a probe's cell: None outside the grid, True blocked, False free."""
    H, W = g.shape
    if not (0 <= cx < W and 0 <= cy < H):
        return None
    v = int(g[cy, cx])
    return v >= fc.foot_lethal or (v < 0 and not n.allow_unknown)


def start_probe_np(grid, pose, navfn_cfg, footprint, fcfg=None):
    """The index of the first probe that is not free at the pose, -1 if none."""
    n = _nav.NavfnConfig.from_any(navfn_cfg)
    fp, fc = _foot_args(footprint, fcfg, "start_probe_np")
    g = np.asarray(grid)
    X, Y, h = _ints(pose, 3, "start_probe_np", "a pose (X, Y, h)")
    for q, (fx, fy) in enumerate(fp.tolist()):
        if _probe_value(g, n, fc, *_probe_cell(X, Y, h & (HEADINGS - 1), fx, fy)) is not False:
            return q
    return -1


def movers_np(rows, n, origin, res, dt, cfg):
    """The table of one stream from its track rows, as k_local_movers makes it: rows tracking.TRACK_DTYPE (from
    `Engine.tracks()` for the costmap source, `Engine.tracks_fixed()` for the occupancy source), of which the first n are
    live (n = -1: the stream has had no posed step); origin (ox, oy) and res in metres, dt seconds per step, cfg a
    MoverConfig -> (movers int32 [PP_LOCAL_MAX_MOVERS, 6] with zeros behind them, n_movers or -1, n_skipped)."""
    c = MoverConfig.from_any(cfg)
    ox, oy = (float(v) for v in origin)
    res, dt = float(res), float(dt)
    if not (math.isfinite(ox) and math.isfinite(oy)):
        raise ValueError(f"movers_np: origin = ({ox}, {oy}) must be finite")
    if not (math.isfinite(res) and res > 0.0):
        raise ValueError(f"movers_np: res = {res} must be finite and > 0")
    if not (math.isfinite(dt) and dt > 0.0):
        raise ValueError(f"movers_np: dt = {dt} must be finite and > 0")
    out = np.zeros((PP_LOCAL_MAX_MOVERS, 6), np.int32)
    n = int(n)
    if n < 0:
        return out, -1, 0
    r = np.asarray(rows)[:n]
    if n > PP_TRACK_MAX or len(r) != n:
        raise ValueError(f"movers_np: n = {n} rows of {len(np.asarray(rows))}, at most PP_TRACK_MAX = {PP_TRACK_MAX}")
    st = np.asarray(r["state"], np.float64).reshape(n, 6)
    size = np.asarray(r["size"], np.float64).reshape(n, 3)
    use = (r["confirmed"] != 0) if c.confirmed_only else np.ones(n, bool)
    x, y, vx, vy, w, l = st[:, 0], st[:, 1], st[:, 3], st[:, 4], size[:, 0], size[:, 1]
    finite = np.isfinite(st).all(axis=1) & np.isfinite(w) & np.isfinite(l)
    with np.errstate(all="ignore"):
        MX, MY = np.floor(((x - ox) / res) * 1024.0), np.floor(((y - oy) / res) * 1024.0)
        MVX, MVY = np.rint(((vx * dt) / res) * 1024.0), np.rint(((vy * dt) / res) * 1024.0)
        half = np.fmax(w, l) * 0.5
        RH, RS = np.ceil(((half + c.pad_hard) / res) * 1024.0), np.ceil(((half + c.pad_soft) / res) * 1024.0)
        ok = finite & (np.abs(MX) <= MAX_MOVER_POS) & (np.abs(MY) <= MAX_MOVER_POS)
        ok &= (np.abs(MVX) <= PP_LOCAL_MAX_MOVER_SPEED) & (np.abs(MVY) <= PP_LOCAL_MAX_MOVER_SPEED)
    take = use & ok
    k = int(take.sum())
    cols = (MX, MY, MVX, MVY, np.clip(RH, 0.0, PP_LOCAL_MAX_MOVER_RADIUS), np.clip(RS, 0.0, PP_LOCAL_MAX_MOVER_RADIUS))
    for q, v in enumerate(cols):
        out[:k, q] = v[take].astype(np.int64)
    return out, k, int((use & ~ok).sum())


def trig_table():
    """int32 [4096, 2]: (C[h], S[h]) = rint(cos / sin(2 pi h / 4096) * 2^14), in float64."""
    a = 2.0 * np.pi * np.arange(HEADINGS, dtype=np.float64) / HEADINGS
    return np.stack([np.rint(np.cos(a) * ONE), np.rint(np.sin(a) * ONE)], axis=1).astype(np.int32)


_TRIG = trig_table()
_TRIG.setflags(write=False)


def _inputs(grid, pot, who):
    g = np.asarray(grid)
    p = np.asarray(pot)
    if g.dtype != np.int8 or g.ndim != 2 or g.size == 0:
        raise ValueError(f"{who}: a grid must be int8 [H, W] with H, W >= 1, got {g.dtype} {g.shape}")
    if p.dtype != np.uint32 or p.shape != g.shape:
        raise ValueError(f"{who}: pot must be uint32 of the grid's shape {g.shape}, got {p.dtype} {p.shape}")
    return g, p


def _ints(v, n, who, what):
    a = np.asarray(v)
    if a.shape != (n,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{who}: {what} must be {n} integers, got {v!r}")
    return tuple(int(x) for x in a)


def check_window(window, cfg, who="local_planner"):
    """(v0, dv, w0, dw) as ints; raises unless every sample of the window has |sv| <= 1024 and |sw| <= 512."""
    c = LocalPlanConfig.from_any(cfg)
    v0, dv, w0, dw = _ints(window, 4, who, "a window (v0, dv, w0, dw)")
    v1, w1 = v0 + (c.nv - 1) * dv, w0 + (c.nw - 1) * dw
    if max(abs(v0), abs(v1)) > MAX_SV:
        raise ValueError(f"{who}: sv runs from {v0} to {v1}, outside [-{MAX_SV}, {MAX_SV}]")
    if max(abs(w0), abs(w1)) > MAX_SW:
        raise ValueError(f"{who}: sw runs from {w0} to {w1}, outside [-{MAX_SW}, {MAX_SW}]")
    return v0, dv, w0, dw


def sample(s, window, cfg):
    """(sv, sw) of sample s = i * nw + j."""
    c = LocalPlanConfig.from_any(cfg)
    v0, dv, w0, dw = window
    return int(v0) + (s // c.nw) * int(dv), int(w0) + (s % c.nw) * int(dw)


def _cell_value(g, x, y, n):
    """The rule's reading of cell (x, y): None outside the grid, -1 blocked, else the value occ takes."""
    H, W = g.shape
    if not (0 <= x < W and 0 <= y < H):
        return None
    v = int(g[y, x])
    if v >= n.lethal_cost:
        return -1
    if v < 0:
        return n.unknown_cost if n.allow_unknown else -1
    return v


def stream_state_np(grid, pot, pose, navfn_cfg, goal_state=0):
    """The part of cmd_state that needs no sample: 4, 3, 2 or 0."""
    n = _nav.NavfnConfig.from_any(navfn_cfg)
    g, p = _inputs(grid, pot, "stream_state_np")
    X, Y, _ = _ints(pose, 3, "stream_state_np", "a pose (X, Y, h)")
    if int(goal_state) != 0:
        return STATE_NO_GOAL
    cx, cy = X >> 10, Y >> 10
    v = _cell_value(g, cx, cy, n)
    if v is None or v < 0 or int(p[cy, cx]) == _nav.UNREACHED:
        return STATE_POSE
    return STATE_ARRIVED if int(p[cy, cx]) == 0 else STATE_OK


def score_np(grid, pot, pose, sv, sw, navfn_cfg, cfg, movers=None, mcfg=None, footprint=None, fcfg=None):
    """One sample, step by step in Python ints: (reason, score or None, poses) -- the poses [(X, Y, h)] the sample
    reached, the start included (steps + 1 of them when reason is OK or UNREACHED).  With movers (integers [n, 6] and a
    MoverConfig): (reason, score or None, poses, near).  With a footprint (a Footprint or probes [P, 2], and a
    FootprintConfig or None for the defaults) the tuple is the same; the start pose's own probes are not looked at (that
    is state 5, `start_probe_np`)."""
    mv, mc = _mover_args(movers, mcfg, "score_np")
    fp, fc = _foot_args(footprint, fcfg, "score_np")
    foot = None if fp is None else (fp.tolist(), fc)
    if mv is None:
        return _score(grid, pot, pose, sv, sw, navfn_cfg, cfg, (), None, foot)[:3]
    return _score(grid, pot, pose, sv, sw, navfn_cfg, cfg, mv.tolist(), mc, foot)


def _score(grid, pot, pose, sv, sw, navfn_cfg, cfg, mv, mc, foot=None):
    n = _nav.NavfnConfig.from_any(navfn_cfg)
    c = LocalPlanConfig.from_any(cfg)
    g, p = _inputs(grid, pot, "score_np")
    X, Y, h = _ints(pose, 3, "score_np", "a pose (X, Y, h)")
    sv, sw = int(sv), int(sw)
    h &= HEADINGS - 1
    C, S = _TRIG[:, 0], _TRIG[:, 1]
    poses = [(X, Y, h)]
    occ = near = 0
    for k in range(1, c.steps + 1):
        X += (sv * int(C[h]) + 8192) >> 14
        Y += (sv * int(S[h]) + 8192) >> 14
        h = (h + sw) & (HEADINGS - 1)
        poses.append((X, Y, h))
        v = _cell_value(g, X >> 10, Y >> 10, n)
        if v is None:
            return OUTSIDE, None, poses, near
        if v < 0:
            return COLLISION, None, poses, near
        occ = max(occ, v)
        if foot is not None:                                # the probes in table order, under the heading after the turn
            for fx, fy in foot[0]:
                blocked = _probe_value(g, n, foot[1], *_probe_cell(X, Y, h, fx, fy))
                if blocked is None:
                    return OUTSIDE, None, poses, near
                if blocked:
                    return FOOTPRINT, None, poses, near
        if mc is not None and k <= mc.horizon:
            for mx, my, mvx, mvy, rh, rs in mv:
                dx, dy = X - (mx + k * mvx), Y - (my + k * mvy)
                d2 = dx * dx + dy * dy
                assert d2 < 2 ** 63
                if d2 <= rh * rh:
                    return DYNAMIC, None, poses, near
                if d2 <= rs * rs:
                    near = max(near, mc.horizon + 1 - k)
    lx = X + ((c.lookahead * int(C[h]) + 8192) >> 14)
    ly = Y + ((c.lookahead * int(S[h]) + 8192) >> 14)
    cx, cy = lx >> 10, ly >> 10
    v = _cell_value(g, cx, cy, n)
    if v is None or v < 0 or int(p[cy, cx]) == _nav.UNREACHED:
        return UNREACHED, None, poses, near
    score = c.pot_weight * int(p[cy, cx]) + c.occ_weight * occ + c.speed_weight * (1024 - abs(sv)) + c.turn_weight * abs(sw)
    if mc is not None:
        score += mc.mover_weight * near
    return OK, score, poses, near


def keys_by_sample_np(grid, pot, pose, window, navfn_cfg, cfg, movers=None, mcfg=None, footprint=None, fcfg=None):
    """(keys uint64 [nv * nw], reasons int32 [nv * nw]) of a window through `score_np`, sample by sample."""
    c = LocalPlanConfig.from_any(cfg)
    window = check_window(window, c, "keys_by_sample_np")
    keys = np.full(c.nv * c.nw, INVALID, np.uint64)
    reasons = np.zeros(c.nv * c.nw, np.int32)
    for s in range(c.nv * c.nw):
        sv, sw = sample(s, window, c)
        reasons[s], score = score_np(grid, pot, pose, sv, sw, navfn_cfg, c, movers, mcfg, footprint, fcfg)[:2]
        if score is not None:
            keys[s] = (score << 14) | s
    return keys, reasons


def scores_np(grid, pot, pose, window, navfn_cfg, cfg, movers=None, mcfg=None, footprint=None, fcfg=None):
    """(keys uint64 [nv * nw], reasons int32 [nv * nw]) of a window, all samples at once: arrays over the samples, one
    masked update per step (and, with movers, per step and mover; with a footprint, one over samples x probes per step)."""
    mv, mc = _mover_args(movers, mcfg, "scores_np")
    fp, fc = _foot_args(footprint, fcfg, "scores_np")
    n = _nav.NavfnConfig.from_any(navfn_cfg)
    c = LocalPlanConfig.from_any(cfg)
    g, p = _inputs(grid, pot, "scores_np")
    v0, dv, w0, dw = check_window(window, c, "scores_np")
    X0, Y0, h0 = _ints(pose, 3, "scores_np", "a pose (X, Y, h)")
    H, W = g.shape
    # the value occ takes per cell, -1 where blocked
    val = g.astype(np.int64)
    val = np.where(val >= n.lethal_cost, -1, np.where(val < 0, n.unknown_cost if n.allow_unknown else -1, val))
    N = c.nv * c.nw
    s = np.arange(N, dtype=np.int64)
    sv, sw = v0 + (s // c.nw) * dv, w0 + (s % c.nw) * dw
    X, Y = np.full(N, X0, np.int64), np.full(N, Y0, np.int64)
    h = np.full(N, h0 & (HEADINGS - 1), np.int64)
    occ = np.zeros(N, np.int64)
    near = np.zeros(N, np.int64)
    reason = np.zeros(N, np.int32)
    alive = np.ones(N, bool)
    C, S = _TRIG[:, 0].astype(np.int64), _TRIG[:, 1].astype(np.int64)
    if fp is not None:                                      # a probe's reading by the cell's value + 1 (0: unknown)
        foot_raw = np.maximum(g.astype(np.int64), -1)
        foot_blocked = np.arange(-1, 128) >= fc.foot_lethal
        foot_blocked[0] = not n.allow_unknown

    def read(cx, cy, m):
        """(inside, index): which samples of mask m lie in the grid, and an index that is (0, 0) for the others"""
        inside = m & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        at = (np.where(inside, cy, 0), np.where(inside, cx, 0))
        return inside, at

    for k in range(1, c.steps + 1):
        X = np.where(alive, X + ((sv * C[h] + 8192) >> 14), X)
        Y = np.where(alive, Y + ((sv * S[h] + 8192) >> 14), Y)
        h = np.where(alive, (h + sw) & (HEADINGS - 1), h)
        inside, at = read(X >> 10, Y >> 10, alive)
        v = val[at]
        out = alive & ~inside
        hit = inside & (v < 0)
        reason[out] = OUTSIDE
        reason[hit] = COLLISION
        alive = alive & ~out & ~hit
        occ = np.where(alive, np.maximum(occ, v), occ)
        if fp is not None:                                  # [N, P]: 0 free, 1 outside, 2 blocked; the first that is not free
            Ch, Sh = C[h][:, None], S[h][:, None]
            px = (X[:, None] + ((fp[None, :, 0] * Ch - fp[None, :, 1] * Sh + 8192) >> 14)) >> 10
            py = (Y[:, None] + ((fp[None, :, 0] * Sh + fp[None, :, 1] * Ch + 8192) >> 14)) >> 10
            inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
            gq = foot_raw[np.where(inside, py, 0), np.where(inside, px, 0)]
            status = np.where(inside, np.where(foot_blocked[gq + 1], 2, 0), 1)
            first = np.argmax(status != 0, axis=1)
            verdict = status[np.arange(N), first]
            reason[alive & (verdict == 1)] = OUTSIDE
            reason[alive & (verdict == 2)] = FOOTPRINT
            alive = alive & (verdict == 0)
        if mc is None or k > mc.horizon:
            continue
        for mx, my, mvx, mvy, rh, rs in mv:                 # int64 arrays: |dx| < 2^31, so d2 < 2^63 (asserted above)
            dx, dy = X - (mx + k * mvx), Y - (my + k * mvy)
            d2 = dx * dx + dy * dy
            hard = alive & (d2 <= rh * rh)
            reason[hard] = DYNAMIC
            alive = alive & ~hard
            near = np.where(alive & (d2 <= rs * rs), np.maximum(near, mc.horizon + 1 - k), near)
    lx = X + ((c.lookahead * C[h] + 8192) >> 14)
    ly = Y + ((c.lookahead * S[h] + 8192) >> 14)
    inside, at = read(lx >> 10, ly >> 10, alive)
    reached = inside & (val[at] >= 0) & (p[at] != _nav.UNREACHED)
    reason[alive & ~reached] = UNREACHED
    score = c.pot_weight * p[at].astype(np.int64) + c.occ_weight * occ + c.speed_weight * (1024 - np.abs(sv)) + c.turn_weight * np.abs(sw)
    if mc is not None:
        score = score + mc.mover_weight * near
    keys = np.where(reached, (score.astype(np.uint64) << np.uint64(14)) | s.astype(np.uint64), np.uint64(INVALID))
    return keys.astype(np.uint64), reason


def best_np(grid, pot, pose, window, navfn_cfg, cfg, goal_state=0, samples=None, movers=None, mcfg=None, footprint=None, fcfg=None):
    """The results of one grid as a dict: the RESULT words, `score`, `traj` int32 [steps + 1, 3] (or [0, 3]) and `keys`
    uint64 [nv * nw].  samples: `scores_np` (the default) or `keys_by_sample_np`.  With movers (integers [n, 6] and a
    MoverConfig) also `n_movers`, `n_dynamic` and `near`.  With a footprint (a Footprint or probes [P, 2], and a
    FootprintConfig or None for the defaults) also the FOOT_INFO words `n_probes`, `n_footprint` and `start_probe`."""
    mv, mc = _mover_args(movers, mcfg, "best_np")
    fp, fc = _foot_args(footprint, fcfg, "best_np")
    extra = () if mv is None else (mv, mc)
    if fp is not None:
        extra = (mv, mc, fp, fc)
    c = LocalPlanConfig.from_any(cfg)
    window = check_window(window, c, "best_np")
    N = c.nv * c.nw
    out = {k: 0 for k in RESULT}
    out.update(best=-1, score=0, traj=np.zeros((0, 3), np.int32), keys=np.full(N, INVALID, np.uint64))
    if mv is not None:
        out.update(n_movers=len(mv), n_dynamic=0, near=0)
    if fp is not None:
        out.update(n_probes=len(fp), n_footprint=0, start_probe=-1)
    state = stream_state_np(grid, pot, pose, navfn_cfg, goal_state)
    if state == STATE_OK and fp is not None:
        out["start_probe"] = start_probe_np(grid, pose, navfn_cfg, fp, fc)
        if out["start_probe"] >= 0:
            state = STATE_FOOTPRINT
    if state == STATE_OK:
        keys, reasons = (samples or scores_np)(grid, pot, pose, window, navfn_cfg, c, *extra)
        out["keys"] = keys
        if mv is not None:
            out["n_dynamic"] = int((reasons == DYNAMIC).sum())
        if fp is not None:
            out["n_footprint"] = int((reasons == FOOTPRINT).sum())
        for r, name in ((OK, "n_ok"), (OUTSIDE, "n_outside"), (COLLISION, "n_collision"), (UNREACHED, "n_unreached")):
            out[name] = int((reasons == r).sum())
        k = int(keys.min())
        if k == INVALID:
            state = STATE_NO_SAMPLE
        else:
            s = k & (PP_LOCAL_MAX_SAMPLES - 1)
            sv, sw = sample(s, window, c)
            reason, score, poses, *near = score_np(grid, pot, pose, sv, sw, navfn_cfg, c, *extra)
            assert reason == OK and score == k >> 14
            out.update(best=s, sv=sv, sw=sw, score=score, traj=np.array(poses, np.int32).reshape(-1, 3))
            if mv is not None:
                out["near"] = near[0]
    out["cmd_state"] = state
    return out


# ---- host helpers: the only place where metres, radians and seconds appear (float64) ----
def pose_ticks(xy, yaw, origin, resolution):
    """Metres and radians -> int32 [B, 3] (X, Y, h): X = floor((x - origin_x) / resolution * 1024) sub-cells, likewise Y,
    h = rint(yaw / 2 pi * 4096) & 4095, for points xy [B, 2] (or [2]) and yaws [B] (or one) in the frame of grids whose
    cell [0, 0] lies at origins [B, 2] (or [2]).  A NaN gives (-1024, -1024, 0), a pose outside its grid; a point far beyond
    the grid is clipped to +-2^30 sub-cells, outside all the same."""
    p = np.atleast_2d(np.asarray(xy, np.float64))
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"pose_ticks: xy must be [B, 2] metres, got {np.asarray(xy).shape}")
    o = np.broadcast_to(np.atleast_2d(np.asarray(origin, np.float64)), p.shape)
    a = np.broadcast_to(np.asarray(yaw, np.float64).reshape(-1), (p.shape[0],))
    if not float(resolution) > 0.0:
        raise ValueError(f"pose_ticks: resolution = {resolution} must be > 0")
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((p - o) / float(resolution) * SUB)
        t = np.rint(a / (2.0 * np.pi) * HEADINGS)
    bad = ~(np.isfinite(f).all(axis=1) & np.isfinite(t))
    f = np.clip(np.where(bad[:, None], -float(SUB), f), -float(2 ** 30), float(2 ** 30))
    t = np.where(bad, 0.0, np.fmod(t, HEADINGS))
    out = np.empty((p.shape[0], 3), np.int32)
    out[:, :2] = f.astype(np.int64)
    out[:, 2] = t.astype(np.int64) & (HEADINGS - 1)
    return out


def command_metric(sv, sw, resolution, dt):
    """(v m/s, w rad/s) of a command in sub-cells and ticks per step of dt seconds."""
    return (np.asarray(sv, np.float64) / SUB * float(resolution) / float(dt),
            np.asarray(sw, np.float64) * (2.0 * np.pi / HEADINGS) / float(dt))


@dataclasses.dataclass
class LocalLimits:
    """v_min, v_max    m/s, v_min <= v_max (v_min < 0 allows reverse); not both 0
    w_max           rad/s, >= 0: |w| at most
    acc_v, acc_w    m/s^2 and rad/s^2, >= 0: what a control period may change
    sim_time        s, > 0: how far a rollout looks
    period          s, > 0: the control period"""
    v_min: float = 0.0
    v_max: float = 0.5
    w_max: float = 1.0
    acc_v: float = 0.5
    acc_w: float = 2.0
    sim_time: float = 2.0
    period: float = 0.1

    def __post_init__(self):
        for f in dataclasses.fields(self):
            v = float(getattr(self, f.name))
            if not math.isfinite(v):
                raise ValueError(f"LocalLimits: {f.name} = {v} must be finite")
            setattr(self, f.name, v)
        if self.v_min > self.v_max or max(abs(self.v_min), abs(self.v_max)) == 0.0:
            raise ValueError(f"LocalLimits: v_min = {self.v_min}, v_max = {self.v_max}: v_min <= v_max and not both 0")
        for f in ("w_max", "acc_v", "acc_w"):
            if getattr(self, f) < 0.0:
                raise ValueError(f"LocalLimits: {f} = {getattr(self, f)} must be >= 0")
        for f in ("sim_time", "period"):
            if not getattr(self, f) > 0.0:
                raise ValueError(f"LocalLimits: {f} = {getattr(self, f)} must be > 0")

    def step_dt(self, resolution):
        """Seconds per step: the fastest allowed sample moves one cell per step."""
        return float(resolution) / max(abs(self.v_min), abs(self.v_max))

    def steps(self, resolution):
        """The steps that cover sim_time, 1 .. 256."""
        return int(min(max(round(self.sim_time / self.step_dt(resolution)), 1), PP_LOCAL_MAX_STEPS))

    def window(self, v, w, nv, nw, resolution):
        """The dynamic window round the current velocity (v m/s, w rad/s), clipped to the limits, as integers
        (v0, dv, w0, dw): sample i, j has v0 + i * dv sub-cells and w0 + j * dw ticks per step.  The ends are rounded
        inwards, so no sample lies outside the limits (nor outside |sv| <= 1024, |sw| <= 512); a window narrower than
        one unit collapses onto the nearest admissible value."""
        dt = self.step_dt(resolution)
        ku, kw = SUB * dt / float(resolution), HEADINGS * dt / (2.0 * np.pi)       # units per m/s, per rad/s

        def axis(cur, lo, hi, acc, k, cap, n):
            lo_u, hi_u = max(math.ceil(lo * k - 1e-9), -cap), min(math.floor(hi * k + 1e-9), cap)
            a = max(math.ceil(max(lo, cur - acc * self.period) * k - 1e-9), lo_u)
            b = min(math.floor(min(hi, cur + acc * self.period) * k + 1e-9), hi_u)
            if a > b:
                a = b = min(max(int(round(cur * k)), lo_u), hi_u)
            d = (b - a) // (n - 1) if n > 1 else 0
            return int(a), int(d)

        v0, dv = axis(float(v), self.v_min, self.v_max, self.acc_v, ku, MAX_SV, int(nv))
        w0, dw = axis(float(w), -self.w_max, self.w_max, self.acc_w, kw, MAX_SW, int(nw))
        return v0, dv, w0, dw


def _batch_ints(v, B, n, who, what):
    a = np.asarray(v)
    if a.shape == (n,):
        a = np.broadcast_to(a, (B, n))
    if a.shape != (B, n) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{who}: {what} must be integers [{B}, {n}], got {a.dtype} {a.shape}")
    return np.ascontiguousarray(np.clip(a, -(2 ** 31), 2 ** 31 - 1), np.int32)


def unpack_results(c, B, res, score, traj, keys):
    """The buffers of pp_get_local_plan / pp_local_plan_grids -> a dict: the RESULT words int32 [B] each, `score` uint64
    [B], `traj` a list of B arrays int32 [steps + 1, 3] ([0, 3] unless cmd_state is 0), `keys` uint64 [B, nv * nw] if
    given."""
    out = {k: res[:, i].copy() for i, k in enumerate(RESULT)}
    out["score"] = score
    if traj is not None:
        out["traj"] = [traj[b].copy() if res[b, 0] == 0 else np.zeros((0, 3), np.int32) for b in range(B)]
    if keys is not None:
        out["keys"] = keys
    return out


def local_plan(grids, pots, poses, windows, navfn_cfg, cfg, goal_state=None, keys=False, device=0, movers=None, n_movers=None,
               mover_cfg=None, footprint=None, fcfg=None):
    """The rule on the GPU, without an engine (pp_local_plan_grids): grids int8 and pots uint32 [H, W] or [B, H, W]
    (H * W <= PP_OCC_MAX_CELLS), poses integers [B, 3] (or one), windows integers [B, 4] (or one), goal_state integers [B]
    or None (all 0) -> a dict: the RESULT words and `score` per grid, `traj`, and `keys` if asked (ints and arrays for one
    grid; int32 [B], uint64 [B], a list of B arrays and uint64 [B, nv * nw] for a batch).  With movers
    (pp_local_plan_grids_movers): movers integers [n, 6] for one grid, [B, PP_LOCAL_MAX_MOVERS, 6] with n_movers integers
    [B] for a batch, and mover_cfg a MoverConfig of which horizon and mover_weight are read; the dict then also holds the
    MOVER_INFO words.  With a footprint (pp_local_plan_grids_footprint, with or without movers): a Footprint or probes
    integers [P, 2], one table for every grid, and fcfg a FootprintConfig, a dict of its fields, True or None (the
    defaults); the dict then also holds the FOOT_INFO words."""
    n = _nav.NavfnConfig.from_any(navfn_cfg)
    c = LocalPlanConfig.from_any(cfg)
    a, p = np.asarray(grids), np.asarray(pots)
    one = a.ndim == 2
    if one:
        a, p = a[None], p[None] if p.ndim == 2 else p
    if a.dtype != np.int8 or a.ndim != 3 or a.size == 0:
        raise ValueError(f"local_plan: grids must be int8 [H, W] or [B, H, W] with B, H, W >= 1, got {a.dtype} {np.asarray(grids).shape}")
    if p.dtype != np.uint32 or p.shape != a.shape:
        raise ValueError(f"local_plan: pots must be uint32 of the grids' shape {a.shape}, got {p.dtype} {p.shape}")
    B, H, W = a.shape
    if H * W > PP_OCC_MAX_CELLS:
        raise ValueError(f"local_plan: H * W = {H * W} cells, at most PP_OCC_MAX_CELLS = {PP_OCC_MAX_CELLS}")
    a, p = np.ascontiguousarray(a), np.ascontiguousarray(p)
    P = _batch_ints(poses, B, 3, "local_plan", "poses")
    Wn = _batch_ints(windows, B, 4, "local_plan", "windows")
    for b in range(B):
        check_window(Wn[b], c, f"local_plan: grid {b}")
    gs = None if goal_state is None else np.ascontiguousarray(np.broadcast_to(np.asarray(goal_state), (B,)), np.int32)
    fp, fc = _foot_args(footprint, fcfg, "local_plan")
    if movers is None and (n_movers is not None or mover_cfg is not None):
        raise ValueError("local_plan: n_movers or mover_cfg without movers (an empty table is movers=[])")
    if movers is not None:
        if mover_cfg is None:
            raise ValueError("local_plan: movers need mover_cfg (a MoverConfig, a dict of its fields or True)")
        mc = MoverConfig.from_any(mover_cfg)
        M = np.zeros((B, PP_LOCAL_MAX_MOVERS, 6), np.int32)
        m = np.asarray(movers)
        if n_movers is None:                                # one table [n, 6], for every grid
            t = check_movers(m, "local_plan")
            NM = np.full(B, len(t), np.int32)
            M[:, :len(t)] = t
        else:
            NM = np.ascontiguousarray(np.broadcast_to(np.asarray(n_movers), (B,)), np.int32)
            if m.shape != (B, PP_LOCAL_MAX_MOVERS, 6) or not np.issubdtype(m.dtype, np.integer):
                raise ValueError(f"local_plan: movers with n_movers must be integers [{B}, {PP_LOCAL_MAX_MOVERS}, 6], got {m.dtype} {m.shape}")
            for b in range(B):
                if not 0 <= NM[b] <= PP_LOCAL_MAX_MOVERS:
                    raise ValueError(f"local_plan: grid {b}: n_movers = {NM[b]} outside [0, {PP_LOCAL_MAX_MOVERS}]")
                M[b, :NM[b]] = check_movers(m[b, :NM[b]], f"local_plan: grid {b}")
        info = np.zeros((B, PP_LOCAL_MOVER_INFO), np.int32)
    trig = np.ascontiguousarray(_TRIG)
    res = np.zeros((B, len(RESULT)), np.int32)
    score = np.zeros(B, np.uint64)
    traj = np.zeros((B, c.steps + 1, 3), np.int32)
    kk = np.zeros((B, c.nv * c.nw), np.uint64) if keys else None
    L = _lib.lib()
    head = (int(device), a.ctypes.data, p.ctypes.data, B, H, W, ctypes.byref(_lib.PPNavfnConfig(**n.to_dict())),
            ctypes.byref(_lib.PPLocalPlanConfig(**c.to_dict())), trig.ctypes.data, len(trig), P.ctypes.data, Wn.ctypes.data,
            None if gs is None else gs.ctypes.data)
    outs = (res.ctypes.data, score.ctypes.data, traj.ctypes.data, None if kk is None else kk.ctypes.data)
    if fp is not None:
        F = np.ascontiguousarray(fp, np.int32)
        finfo = np.zeros((B, PP_LOCAL_FOOT_INFO), np.int32)
        mover_args = (0, 0, None, None, None) if movers is None else (mc.horizon, mc.mover_weight, M.ctypes.data, NM.ctypes.data, info.ctypes.data)
        st = L.pp_local_plan_grids_footprint(*head, *mover_args[:4], F.ctypes.data, len(F), fc.foot_lethal, *outs, mover_args[4], finfo.ctypes.data)
    elif movers is None:
        st = L.pp_local_plan_grids(*head, *outs)
    else:
        st = L.pp_local_plan_grids_movers(*head, mc.horizon, mc.mover_weight, M.ctypes.data, NM.ctypes.data, *outs, info.ctypes.data)
    if st != 0:
        msg = L.pp_last_error(None)
        raise (ValueError if st == 1 else RuntimeError)(f"local_plan: {msg.decode() if msg else st}")
    out = unpack_results(c, B, res, score, traj, kk)
    if movers is not None:
        out.update({k: info[:, i].copy() for i, k in enumerate(MOVER_INFO)})
    if fp is not None:
        out.update({k: finfo[:, i].copy() for i, k in enumerate(FOOT_INFO)})
    if one:
        out = {k: (v[0] if isinstance(v, (list, np.ndarray)) else v) for k, v in out.items()}
        out = {k: (int(v) if np.ndim(v) == 0 else v) for k, v in out.items()}
    return out
