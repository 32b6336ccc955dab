"""The navigation chain (source, inflation, navigation function, local plan) on one handle ACROSS RECONFIGURATION: the shapes,
configurations and call sequences of tests/test_gpu_nav_reconfig.py, and `Model`, a host model of the chain that
tests/test_nav_reconfig_host.py holds to nav_cycle_cases.plan_np and shows to discriminate.  Pure numpy up to `Driver`,
which applies the same operations to an Engine.

THE RULE.  Every call of the chain either returns, byte for byte, what the package's numpy restatements give for the inputs
and configurations of the RUNS it rests on -- the source run, the inflation run, the navfn run, the local-plan run --
whatever set_*, reset or other run came between, or it is refused with the message the code has.  The model therefore
keeps, per source, one record per run with everything that run was queued with, and every expected value is computed from
records alone; the configurations in force only decide what the NEXT run gets and what is refused.

An operation is a tuple (name, *args); Model.apply(op) gives ("ok", expected), ("refused", regex) or ("either", expected,
regex) -- the last for a local-plan getter behind a re-made inflation, which is refused only if it has to roll the samples
again, and whether it has to depends on relaxation rounds the model does not predict.  Driver.apply(op) gives ("ok", got)
or ("refused", message).  `hold` compares the two."""
import re

import numpy as np

import nav_cycle_cases as K
from nav_cycle_cases import LIMITS, MARGIN, STREAMS, inflate_all

NMAX = K.NMAX
SOURCES = ("costmap", "occupancy")
SIZES = (257, 64, 65)                 # rows per stream: two chunks, a wave, a wave and one
PLAN_DT = K.PLAN_DT

# ---- shapes ----
CM_A = dict(K.GRID, objects="none")                           # 51 x 43: device rows of 52 cells, 2 x 2 navfn tiles
CM_B = dict(CM_A, width=37, height=29)                        # 37 x 29: rows of 40, 2 x 1 tiles
CM_C = dict(CM_A, width=70, height=33)                        # 70 x 33: rows of 72, 3 x 2 tiles, two inflation tiles wide
CM_A_MOVED = dict(CM_A, x_min=-0.43, y_min=-0.92)             # A's shape, another origin (no whole number of cells away)
CM_A_COARSE = dict(CM_A, resolution=0.1)                      # A's shape, another resolution
CM_WALK = (CM_A, CM_B, CM_C, CM_A)                            # a shrink, a growth and a return
OCC_A = dict(K.OCC)                                           # 37 x 29 cells of 0.1 m
OCC_B = dict(K.OCC, width=45, height=31)
OCC_WALK = (OCC_A, OCC_B, OCC_A)
OCC_SAME_MAP = dict(OCC_A, z_max=0.6, max_range=1.2)          # the maps are kept (api_occupancy.hip: same_map)
OCC_COARSE = dict(OCC_A, resolution=0.2)                      # the maps are forgotten


# ---- configurations that change what the kernels index ----
def infl_cfg(cells, res=0.05):
    """The inflation of `cells` cells radius at resolution res; the inscribed radius is one cell."""
    return dict(resolution=res, inscribed_radius=res, inflation_radius=cells * res, cost_scaling_factor=0.4 / res)


INFL_RADII = (4, 7, 2)
NAV_CM = dict(lethal_cost=100, allow_unknown=1, unknown_cost=30, max_path=64, queued_rounds=1)    # one round: every getter settles
NAV_OCC = dict(lethal_cost=100, allow_unknown=1, unknown_cost=20, max_path=64)
MAX_PATHS = (64, 256, 32)
LOC_1 = dict(nv=5, nw=13, steps=8, lookahead=1024, pot_weight=8, occ_weight=4, speed_weight=1, turn_weight=1)
LOC_2 = dict(LOC_1, nw=52, steps=12)                          # 260 samples: two rollout workgroups
LOC_3 = dict(LOC_1, nv=3, nw=7, steps=4)                      # buffers kept, strides of the run
LOCS = (LOC_1, LOC_2, LOC_3)
MOV = dict(horizon=4, mover_weight=64, pad_hard=0.0, pad_soft=0.15, confirmed_only=False)

# what the planner is asked, per stream: goals and poses in metres (the sensor frame for the costmap; offsets from the
# update's pose for the occupancy maps), velocities for the windows.  Chosen on the CPU (tests/test_nav_reconfig_host.py
# asserts what they discriminate): inside every shape of the walks, free, and apart by stream.
GOALS_CM = np.array([[1.1, 0.2], [0.9, -0.65], [0.3, 0.3]])
POSES_CM = np.array([[0.12, 0.13, 0.4], [0.33, -0.21, -0.7], [0.71, 0.14, 2.2]])
GOALS_OCC = np.array([[1.0, 0.5], [0.6, -0.9], [-1.1, -0.6]])
VEL = np.array([[0.11, 0.25], [0.2, -0.5], [0.05, 0.0]])


def frames(seed):
    """STREAMS frames of SIZES rows in the tiny range, seeded (nav_cycle_cases._frame)."""
    rng = np.random.default_rng(seed)
    return [K._frame(rng, n) for n in SIZES]


FRAME_SEEDS = (101, 102, 103)


def poses(i, pp):
    """The sensor-to-fixed poses of update i: stream b drifts 0.035 m per call sideways and turns slowly."""
    return np.stack([pp.sweeps.pose_from_xyyaw(0.02 * i, 0.035 * i * (b - 1), 0.05 * i * (b + 1)) for b in range(STREAMS)])


def windows(pp, lcfg, res, vel=VEL):
    """LIMITS' dynamic windows round the velocities under the local-plan configuration a call will run with."""
    L = pp.local_planner
    c, lim = L.LocalPlanConfig.from_any(lcfg), L.LocalLimits(**LIMITS)
    return np.array([lim.window(v, w, c.nv, c.nw, res) for v, w in np.asarray(vel)], np.int32)


def undecided_points(pp, frs, cfg):
    """Rows of the frames whose cell in the costmap of cfg lies within MARGIN metres of a cell border."""
    c = pp.costmap.CostmapConfig.from_any(cfg)
    n = 0
    for f in frs:
        for col, lo in ((0, c.x_min), (1, c.y_min)):
            t = (f[:, col].astype(np.float64) - lo) / c.resolution
            n += int((np.abs(t - np.rint(t)) * c.resolution < MARGIN).sum())
    return n


# ---- the restatements, cached per (grid bytes, configuration) ----
_FIELDS, _LOCAL = {}, {}


def field_np(pp, grid, goal, start, ncfg):
    """navfn_np and descend_np of one grid -> (pot, path, info with path_state)."""
    N = pp.navfn
    key = (grid.shape, grid.tobytes(), goal.tobytes(), start.tobytes(), repr(ncfg))
    if key not in _FIELDS:
        pot, info = N.navfn_np(grid, goal, ncfg, info=True)
        path, pstate = N.descend_np(pot, grid, start, ncfg)
        _FIELDS[key] = (pot, path, dict(info, path_state=pstate))
    return _FIELDS[key]


def best_np(pp, grid, pot, ticks, window, ncfg, lcfg, goal_state, movers, mcfg):
    L = pp.local_planner
    key = (grid.shape, grid.tobytes(), pot.tobytes(), ticks.tobytes(), window.tobytes(), repr(ncfg), repr(lcfg), int(goal_state),
           None if movers is None else movers.tobytes(), repr(mcfg))
    if key not in _LOCAL:
        _LOCAL[key] = L.best_np(grid, pot, ticks, window, ncfg, lcfg, goal_state) if movers is None else \
            L.best_np(grid, pot, ticks, window, ncfg, lcfg, goal_state, movers=movers, mcfg=mcfg)
    return _LOCAL[key]


# ---- the refusals, as the code words them ----
R_INFL_OFF = "PP_ERR_STATE.*: the inflation of the {} source is not configured"
R_SRC_OFF = "PP_ERR_STATE.*pp_inflate_async: the {} stage is not configured"
R_RES = "PP_ERR_STATE.*pp_inflate_async: the {} stage has resolution = .*, the inflation table was built for"
R_NO_SRC_RUN = ("PP_ERR_STATE.*pp_inflate_async: no costmap stage has run", "PP_ERR_STATE.*pp_inflate_async: no update has run")
R_CM_OFF = "PP_ERR_STATE.*pp_costmap_async: the costmap stage is not configured"
R_OCC_OFF = "occupancy_update_async: the occupancy stage is not configured"
R_NO_FRAMES = "PP_ERR_STATE.*upload or ingest frames first"
R_NO_INFL_RUN = "no inflation has run on th"                  # (engine.py: "on the costmap source"; the library: "on this source")
R_NAV_OFF = "PP_ERR_STATE.*: the navigation function of the {} source is not configured"
R_NO_NAV_RUN = "no navigation function has run on th"
R_LOC_OFF = "local_plan_async: the local planner of the {} source is not configured"
R_REMADE = "PP_ERR_STATE.*: the inflated grids of the {} source were re-made since its navigation function ran"
R_NO_LOC_RUN = "no local plan has run on the {} source"
R_NAV_AFTER = "PP_ERR_STATE.*: a pp_navfn_async of the {} source came after the last pp_local_plan_async"
R_NO_MOVERS = "local_movers: the last local plan of the {} source had no movers"

GETTERS = ("inflated", "navfn_fields", "navfn_paths", "navfn_paths_m", "navfn_info", "local_info", "local_traj", "local_keys",
           "local_commands", "local_commands_metric")
NAV_GETTERS, LOCAL_GETTERS = GETTERS[1:5], GETTERS[5:]


def _same_occ_map(a, b):
    return a is not None and all(getattr(a, f) == getattr(b, f) for f in ("width", "height", "resolution", "l_hit", "l_miss", "l_min", "l_max"))


class Model:
    """The chain on the host.  Configurations in force: cm, occ, infl[k], nav[k], loc[k], mov[k] (None: off).  Records:
    cm_run / occ_run, infl_run[k], nav_run[k], loc_run[k]; a record holds what its run was queued with and a reference to
    the record it rests on, and is never written afterwards (an occupancy_reset makes a NEW occ_run record)."""

    def __init__(self, pp, streams=STREAMS):
        self.pp, self.B = pp, streams
        self.frames = None
        self.cm, self.cm_buffers, self.cm_run = None, None, None
        self.occ, self.occ_given, self.maps, self.occ_run = None, None, [None] * streams, None
        self.infl, self.nav, self.loc, self.mov = [None, None], [None, None], [None, None], [None, None]
        self.infl_run, self.nav_run, self.loc_run = [None, None], [None, None], [None, None]
        self.runs = 0

    def _id(self):
        self.runs += 1
        return self.runs

    def apply(self, op):
        return getattr(self, op[0])(*op[1:])

    # -- the feed and the sources --
    def upload(self, seed):
        self.frames = frames(seed)
        return ("ok", None)

    def set_costmap(self, cfg):
        if cfg is None:
            self.cm = None                                      # (buffers and the last run are kept)
            return ("ok", None)
        c = self.pp.costmap.CostmapConfig.from_any(cfg)
        buffers = ((c.width + 3) & ~3, c.height)
        if buffers != self.cm_buffers:
            self.cm_buffers, self.cm_run = buffers, None
        self.cm = c
        return ("ok", None)

    def costmap_async(self):
        if self.cm is None:
            return ("refused", R_CM_OFF)
        if self.frames is None:
            return ("refused", R_NO_FRAMES)
        c = self.cm
        grids = np.stack([self.pp.costmap.costmap_np(f, c)[0] for f in self.frames])
        org = np.tile(np.array([[c.x_min, c.y_min]], np.float64), (self.B, 1))
        self.cm_run = dict(grids=grids, org=org, res=c.resolution, shape=(c.height, c.width), poses=None)
        return ("ok", None)

    def set_occupancy(self, cfg):
        if cfg is None:
            self.occ = None
            return ("ok", None)
        O = self.pp.occupancy
        c = O.OccupancyConfig.from_any(cfg)
        if _same_occ_map(self.occ_given, c):
            for m in self.maps:
                if m is not None:
                    m.cfg, m.table = c, O.cost_table(c)
        else:
            self.maps, self.occ_run = [None] * self.B, None
        self.occ = self.occ_given = c
        return ("ok", None)

    def occupancy_update_async(self, i):
        if self.occ is None:
            return ("refused", R_OCC_OFF)
        if self.frames is None:
            return ("refused", R_NO_FRAMES)
        P = poses(i, self.pp)
        for b in range(self.B):
            if self.maps[b] is None:
                self.maps[b] = self.pp.occupancy.OccupancyMap(self.occ)
            self.maps[b].update(self.frames[b], P[b])
        c = self.occ
        self.occ_run = dict(grids=np.stack([m.grid() for m in self.maps]), org=np.array([m.origin for m in self.maps], np.float64),
                            res=c.resolution, shape=(c.height, c.width), poses=P.copy())
        return ("ok", None)

    def occupancy_reset(self, stream):
        self.maps[stream] = None
        if self.occ_run is not None:                            # the stream reads all unknown, with no origin
            r = dict(self.occ_run, grids=self.occ_run["grids"].copy(), org=self.occ_run["org"].copy())
            r["grids"][stream], r["org"][stream] = -1, np.nan
            self.occ_run = r
        return ("ok", None)

    # -- the stages' configurations --
    def set_inflation(self, cfg, k):
        self.infl[k] = None if cfg is None else self.pp.inflation.InflationConfig.from_any(cfg)
        return ("ok", None)

    def set_navfn(self, cfg, k):
        self.nav[k] = None if cfg is None else self.pp.navfn.NavfnConfig.from_any(cfg)
        return ("ok", None)

    def set_local_planner(self, cfg, k):
        self.loc[k] = None if cfg is None else self.pp.local_planner.LocalPlanConfig.from_any(cfg)
        return ("ok", None)

    def set_local_movers(self, cfg, k):
        self.mov[k] = None if cfg is None else self.pp.local_planner.MoverConfig.from_any(cfg)
        return ("ok", None)

    # -- the runs --
    def inflate_async(self, k):
        name = SOURCES[k]
        if self.infl[k] is None:
            return ("refused", R_INFL_OFF.format(name))
        src, run = (self.cm, self.cm_run) if k == 0 else (self.occ, self.occ_run)
        if src is None:
            return ("refused", R_SRC_OFF.format(name))
        if (run["res"] if run is not None else src.resolution) != self.infl[k].resolution:
            return ("refused", R_RES.format(name))
        if run is None:
            return ("refused", R_NO_SRC_RUN[k])
        grids, d2, info = inflate_all(self.pp, run["grids"], self.infl[k])
        self.infl_run[k] = dict(id=self._id(), grids=grids, d2=d2, info=info, org=run["org"].copy(), res=run["res"], shape=run["shape"],
                                poses=run["poses"])
        return ("ok", None)

    def navfn_async(self, goals, k):
        """goals: metres [B, 2] in the grids' frame; for the occupancy maps OFFSETS from the recorded poses."""
        name = SOURCES[k]
        if self.infl_run[k] is None:
            return ("refused", R_NO_INFL_RUN)
        if self.nav[k] is None:
            return ("refused", R_NAV_OFF.format(name))
        if self.infl[k] is None:
            return ("refused", R_INFL_OFF.format(name))
        self.nav_run[k] = dict(id=self._id(), infl=self.infl_run[k], cfg=self.nav[k], goals=self.goals_for(goals, k))
        return ("ok", None)

    def goals_for(self, goals, k):
        """What navfn_async is given: the costmap's goals as they are, the occupancy maps' from the inflation run's poses."""
        G = np.asarray(goals, np.float64)
        if k == 1 and self.infl_run[k] is not None:
            G = self.infl_run[k]["poses"][:, :2, 3] + G
        return G.copy()

    def local_plan_async(self, P, lcfg_for_windows, k, tracks=None):
        """P: poses [B, 3] or None (the default); the windows are LIMITS' under lcfg_for_windows (the configuration in force
        where the call is accepted) at the navfn run's resolution.  tracks: (rows, n) the movers are made from."""
        name = SOURCES[k]
        nav = self.nav_run[k]
        if nav is None:
            return ("refused", R_NO_NAV_RUN)
        if self.loc[k] is None:
            return ("refused", R_LOC_OFF.format(name))
        if self.nav[k] is None:
            return ("refused", R_NAV_OFF.format(name))
        if self.infl_run[k]["id"] != nav["infl"]["id"]:
            return ("refused", R_REMADE.format(name))
        infl = nav["infl"]
        if P is None:
            T = infl["poses"]
            P = np.zeros((self.B, 3)) if k == 0 else np.stack([T[:, 0, 3], T[:, 1, 3], np.arctan2(T[:, 1, 0], T[:, 0, 0])], axis=1)
        self.loc_run[k] = dict(id=self._id(), nav=nav, cfg=self.loc[k], poses=np.array(P, np.float64), windows=windows(self.pp, self.loc[k], infl["res"]),
                               dt=PLAN_DT, mov=self.mov[k], tracks=tracks if self.mov[k] is not None else None)
        return ("ok", None)

    # -- what a record gives --
    def nav_results(self, run):
        if "out" not in run:
            N, infl, c = self.pp.navfn, run["infl"], run["cfg"]
            H, W = infl["shape"]
            k = 0 if infl["poses"] is None else 1
            goals = N.goal_cells(run["goals"], infl["org"], infl["res"], infl["shape"])
            starts = N.goal_cells(np.zeros((self.B, 2)), infl["org"], infl["res"], infl["shape"]) if k == 0 else \
                np.tile(np.array([[W // 2, H // 2]], np.int32), (self.B, 1))
            res = [field_np(self.pp, infl["grids"][b], goals[b], starts[b], c) for b in range(self.B)]
            run["out"] = dict(
                goal_cells=goals, fields=np.stack([r[0] for r in res]), paths=[r[1] for r in res],
                paths_m=[N.path_to_metres(r[1], infl["org"][b], infl["res"]) for b, r in enumerate(res)],
                info={key: np.array([r[2][key] for r in res], np.int32) for key in ("goal_state", "path_state", "reached")})
        return run["out"]

    def local_results(self, run):
        if "out" not in run:
            L, nav = self.pp.local_planner, run["nav"]
            infl, field = nav["infl"], self.nav_results(nav)
            ticks = L.pose_ticks(run["poses"][:, :2], run["poses"][:, 2], infl["org"], infl["res"])
            tables = [None] * self.B
            if run["mov"] is not None:
                rows, n = run["tracks"]
                tables = [L.movers_np(rows[b], n[b], infl["org"][b], infl["res"], run["dt"], run["mov"]) for b in range(self.B)]
            res = [best_np(self.pp, infl["grids"][b], field["fields"][b], ticks[b], run["windows"][b], nav["cfg"], run["cfg"],
                           field["info"]["goal_state"][b], None if tables[b] is None else tables[b][0][:max(tables[b][1], 0)], run["mov"])
                   for b in range(self.B)]
            info = {key: np.array([r[key] for r in res], np.int32) for key in L.RESULT}
            info["score"] = np.array([r["score"] for r in res], np.uint64)
            out = dict(ticks=ticks, traj=[r["traj"] for r in res], keys=np.stack([r["keys"] for r in res]))
            if run["mov"] is not None:
                minfo = dict(n_movers=np.array([t[1] for t in tables], np.int32), n_skipped=np.array([t[2] for t in tables], np.int32),
                             n_dynamic=np.array([r["n_dynamic"] for r in res], np.int32), near=np.array([r["near"] for r in res], np.int32))
                info.update(minfo)
                out["movers"] = (np.stack([t[0] for t in tables]), minfo)
            out["info"] = info
            v, w = L.command_metric(info["sv"], info["sw"], infl["res"], run["dt"])
            out["commands"] = (info["sv"], info["sw"], info["cmd_state"])
            out["commands_metric"] = (v, w, info["cmd_state"])
            run["out"] = out
        return run["out"]

    # -- the getters --
    def inflated(self, k):
        r = self.infl_run[k]
        return ("refused", R_NO_INFL_RUN) if r is None else ("ok", (r["grids"], r["d2"], r["info"]))

    def _nav_get(self, k, key):
        r = self.nav_run[k]
        return ("refused", R_NO_NAV_RUN) if r is None else ("ok", self.nav_results(r)[key])

    def navfn_fields(self, k):
        return self._nav_get(k, "fields")

    def navfn_paths(self, k):
        got = self._nav_get(k, "paths")
        return got if got[0] != "ok" else ("ok", (got[1], self.nav_results(self.nav_run[k])["info"]["path_state"]))

    def navfn_paths_m(self, k):
        return self._nav_get(k, "paths_m")

    def navfn_info(self, k):
        return self._nav_get(k, "info")

    def _local_get(self, k, key):
        name, r = SOURCES[k], self.loc_run[k]
        if r is None:
            return ("refused", R_NO_LOC_RUN.format(name))
        if r["nav"]["id"] != self.nav_run[k]["id"]:
            return ("refused", R_NAV_AFTER.format(name))
        if key == "movers" and r["mov"] is None:
            return ("refused", R_NO_MOVERS.format(name))
        want = self.local_results(r)[key]
        if self.infl_run[k]["id"] != r["nav"]["infl"]["id"]:
            return ("either", want, R_REMADE.format(name))
        return ("ok", want)

    def local_info(self, k):
        return self._local_get(k, "info")

    def local_traj(self, k):
        return self._local_get(k, "traj")

    def local_keys(self, k):
        return self._local_get(k, "keys")

    def local_commands(self, k):
        return self._local_get(k, "commands")

    def local_commands_metric(self, k):
        return self._local_get(k, "commands_metric")

    def local_movers(self, k):
        return self._local_get(k, "movers")

    def fetch_all(self, k, getters=GETTERS):
        """Every getter of source k -> {getter: its answer}."""
        return {g: getattr(self, g)(k) for g in getters}


# ---- comparing ----
def same(got, want, what):
    """got == want, exactly: arrays by dtype, shape and value, containers by element."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(want) <= set(got), (what, sorted(got), sorted(want))
        for key in want:
            same(got[key], want[key], (what, key))
    elif isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), (what, len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, (what, i))
    elif want is None:
        assert got is None, what
    else:
        g, w = np.asarray(got), np.asarray(want)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, "differs in", int((g != w).sum()), "of", w.size)


def differs(a, b):
    """True where two expected values are not the same bytes."""
    try:
        same(a, b, "")
    except AssertionError:
        return True
    return False


def hold(got, want, what):
    """A Driver's answer against the Model's."""
    if want[0] == "ok":
        assert got[0] == "ok", (what, "refused, the model expects a result:", got[1])
        same(got[1], want[1], what)
    elif want[0] == "refused":
        assert got[0] == "refused", (what, "accepted, the model expects", want[1])
        assert re.search(want[1], got[1]), (what, got[1], want[1])
    else:
        if got[0] == "ok":
            same(got[1], want[1], what)
        else:
            assert re.search(want[2], got[1]), (what, got[1], want[2])


# ---- the seeded walk ----
WALK_SEEDS = (891, 3583, 5732, 7383, 8576, 10526)         # chosen on the CPU: tests/test_nav_reconfig_host.py asserts what each reaches
WALK_OPS = 40
WALK_INFL = (infl_cfg(4), infl_cfg(2), None)
WALK_INFL_OCC = (infl_cfg(4, 0.1), infl_cfg(2, 0.1), None)
WALK_NAV = (NAV_CM, dict(NAV_CM, max_path=256, connectivity=4), None)
WALK_NAV_OCC = (NAV_OCC, dict(NAV_OCC, max_path=32, connectivity=4), None)
WALK_LOC = (LOC_1, LOC_3, None)
WALK_CM = (CM_A, CM_B, CM_A_MOVED)
WALK_KINDS = ("upload", "costmap_async", "occupancy_update_async", "occupancy_reset", "set_costmap", "set_inflation", "set_navfn",
              "set_local_planner", "inflate_async", "navfn_async", "local_plan_async") + GETTERS


def walk_items():
    """Everything a walk draws from, uniformly: an operation with its choice of argument and source."""
    items = [("upload", s) for s in FRAME_SEEDS] + [("costmap_async",), ("occupancy_update_async", None)]
    items += [("occupancy_reset", b) for b in range(STREAMS)] + [("set_costmap", c) for c in WALK_CM]
    for k in (0, 1):
        items += [("set_inflation", c, k) for c in (WALK_INFL, WALK_INFL_OCC)[k]] + [("set_navfn", c, k) for c in (WALK_NAV, WALK_NAV_OCC)[k]]
        items += [("set_local_planner", c, k) for c in WALK_LOC]
        items += [("inflate_async", k), ("navfn_async", (GOALS_CM, GOALS_OCC)[k], k), ("local_plan_async", None, None, k)]
        items += [(g, k) for g in GETTERS]
    items.append(("local_plan_async", POSES_CM, None, 0))
    return items


def walk_start():
    """What every walk begins behind: every stage on and a complete chain on both sources."""
    ops = [("set_costmap", CM_A), ("set_occupancy", OCC_A)]
    for k in (0, 1):
        ops += [("set_inflation", (WALK_INFL, WALK_INFL_OCC)[k][0], k), ("set_navfn", (WALK_NAV, WALK_NAV_OCC)[k][0], k),
                ("set_local_planner", LOC_1, k)]
    ops += [("upload", FRAME_SEEDS[0]), ("costmap_async",), ("occupancy_update_async", 0)]
    for k in (0, 1):
        ops += [("inflate_async", k), ("navfn_async", (GOALS_CM, GOALS_OCC)[k], k), ("local_plan_async", None, None, k)]
    return ops


def walk_ops(seed, n=WALK_OPS):
    """n operations drawn uniformly from walk_items, whatever the chain answers; the occupancy pose drifts with every update."""
    rng = np.random.default_rng(1000 + seed)
    items, ops, updates = walk_items(), [], 0
    for _ in range(n):
        op = items[rng.integers(len(items))]
        if op[0] == "occupancy_update_async":
            updates += 1
            op = (op[0], updates)
        ops.append(op)
    return ops


# ---- driving an Engine (GPU) ----
class Driver:
    """The same operations on an Engine: apply(op) -> ("ok", what the call gave, in the model's layout) or ("refused", text)."""

    def __init__(self, pp, eng):
        self.pp, self.eng = pp, eng

    def apply(self, op):
        try:
            return ("ok", getattr(self, op[0])(*op[1:]))
        except (RuntimeError, ValueError) as err:
            return ("refused", str(err))

    def upload(self, seed):
        self.eng.upload(frames(seed))

    def set_costmap(self, cfg):
        self.eng.set_costmap(cfg)

    def costmap_async(self):
        self.eng.costmap_async()

    def set_occupancy(self, cfg):
        self.eng.set_occupancy(cfg)

    def occupancy_update_async(self, i):
        self.eng.occupancy_update_async(poses(i, self.pp))

    def occupancy_reset(self, stream):
        self.eng.occupancy_reset(stream)

    def set_inflation(self, cfg, k):
        self.eng.set_inflation(cfg, SOURCES[k])

    def set_navfn(self, cfg, k):
        self.eng.set_navfn(cfg, SOURCES[k])

    def set_local_planner(self, cfg, k):
        self.eng.set_local_planner(cfg, SOURCES[k])

    def set_local_movers(self, cfg, k):
        self.eng.set_local_movers(cfg, SOURCES[k])

    def inflate_async(self, k):
        self.eng.inflate_async(SOURCES[k])

    def navfn_async(self, goals, k):
        G = np.asarray(goals, np.float64)
        if k == 1 and 1 in self.eng._infl_run:
            G = self.eng._infl_run[1][3][:, :2, 3] + G
        self.eng.navfn_async(G, SOURCES[k])

    def local_plan_async(self, P, lcfg, k, tracks=None):
        c = self.eng.local_planner_config(SOURCES[k])
        Wn = None
        if c is not None and k in self.eng._navfn_run:
            Wn = windows(self.pp, c, self.eng._navfn_run[k][4])
        self.eng.local_plan_async(P, Wn, SOURCES[k], dt=PLAN_DT)

    def inflated(self, k):
        return self.eng._inflated(k, None, True) + (self.eng.inflation_info(SOURCES[k]),)

    def navfn_fields(self, k):
        return self.eng.navfn_fields(SOURCES[k])

    def navfn_paths(self, k):
        return self.eng.navfn_paths(SOURCES[k])

    def navfn_paths_m(self, k):
        return self.eng.navfn_paths(SOURCES[k], metres=True)[0]

    def navfn_info(self, k):
        return self.eng.navfn_info(SOURCES[k])

    def local_info(self, k):
        return self.eng.local_plan_info(SOURCES[k])

    def local_traj(self, k):
        return self.eng.local_trajectories(SOURCES[k])

    def local_keys(self, k):
        return self.eng.local_keys(SOURCES[k])

    def local_commands(self, k):
        return self.eng.local_commands(SOURCES[k])

    def local_commands_metric(self, k):
        return self.eng.local_commands(SOURCES[k], metric=True)

    def local_movers(self, k):
        return self.eng.local_movers(SOURCES[k])


def engine(pp):
    """An engine of STREAMS streams with no stage on."""
    return pp.Engine(K.config(pp), max_batch=STREAMS, max_points_per_frame=NMAX)


TRACK = dict(max_misses=1, min_hits=2, gate=0.6)
TRACK_STEPS = 4


def walkers(pp, step):
    """(dets, n) of tracking step `step` of TRACK_STEPS: per stream a walker who crosses 0.14 m in front of the robot's pose
    (POSES_CM) at the last step, at 0.4 m/s, and one who stands 0.3 m in front of it."""
    d = np.zeros((STREAMS, 8), pp.engine.DET_DTYPE)
    for b in range(STREAMS):
        x, y, yaw = POSES_CM[b]
        ahead = lambda r: (x + r * np.cos(yaw), y + r * np.sin(yaw))
        for i, (x, y) in enumerate(((ahead(0.14)[0], ahead(0.14)[1] + 0.04 * (TRACK_STEPS - 1 - step)), ahead(0.3))):
            d["box3d_lidar"][b, i] = (x, y, 0.1, 0.12, 0.16, 1.7, 0.0)
            d["score"][b, i] = 0.9
    return d, np.full(STREAMS, 2, np.int32)


class Pair:
    """A Model and, on the GPU, a Driver fed the same operations with every answer held; without an engine the model alone
    (tests/test_nav_reconfig_host.py runs the same scripts that way)."""

    def __init__(self, pp, eng=None):
        self.pp, self.model, self.log = pp, Model(pp), []
        self.driver = None if eng is None else Driver(pp, eng)
        self.tracker = None

    def do(self, *op, tracks=None):
        want = self.model.apply(op + ((tracks,) if tracks is not None else ()))
        got = None
        if self.driver is not None:
            got = self.driver.apply(op)
            hold(got, want, (len(self.log), op[0], op[-1]))
        self.log.append((op[0], want[0], None if got is None else got[0]))
        return want

    def fetch(self, k, getters=GETTERS):
        """Every getter of source k, held; -> the model's answers."""
        return {g: self.do(g, k) for g in getters}

    def chain(self, k, goals, P=None, getters=GETTERS, tracks=None):
        """inflate, navfn, local plan of source k with the configurations in force, then every getter."""
        self.do("inflate_async", k)
        self.do("navfn_async", goals, k)
        self.do("local_plan_async", P, None, k, tracks=tracks)
        return self.fetch(k, getters)

    def track(self, steps):
        """set_tracking and `steps` tracking steps of 0.1 s -> (rows, n) of the streams' tracks in the sensor frame."""
        T = self.pp.tracking
        self.tracker = T.Tracker(T.TrackConfig(**TRACK), STREAMS)
        if self.driver is not None:
            self.driver.eng.set_tracking(TRACK)
        for i in range(steps):
            d, n = walkers(self.pp, i)
            rows, nt, _ = self.tracker.step(d, n, np.full(STREAMS, 0.1))
            if self.driver is not None:
                self.driver.eng.track_update(d, n, np.full(STREAMS, 0.1))
        if self.driver is not None:
            got = self.driver.eng.tracks(STREAMS)
            assert np.array_equal(got[1], nt) and got[0].tobytes() == rows.tobytes(), "the tracks the movers are made from"
        return rows, nt


def setup(pair, k, cm=CM_A, occ=OCC_A, radius=4, nav=None, loc=LOC_1, seed=FRAME_SEEDS[0]):
    """Source k and its three stages on, frames resident."""
    if k == 0:
        pair.do("set_costmap", cm)
        res = cm["resolution"]
    else:
        pair.do("set_occupancy", occ)
        res = occ["resolution"]
    pair.do("set_inflation", infl_cfg(radius, res), k)
    pair.do("set_navfn", (NAV_CM, NAV_OCC)[k] if nav is None else nav, k)
    pair.do("set_local_planner", loc, k)
    pair.do("upload", seed)


def source_run(pair, k, i=0):
    return pair.do(*((("costmap_async",), ("occupancy_update_async", i))[k]))


GOALS = (GOALS_CM, GOALS_OCC)
POSES = (POSES_CM, None)


# ---- part A: reallocation and strides ----
def part_a_shapes(pair, k):
    """The source's window through its shapes; at each change the previous shape's getters behind the source's new run."""
    shapes = (CM_WALK, OCC_WALK)[k]
    setup(pair, k)
    out = []
    for i, shape in enumerate(shapes):
        res = shape["resolution"]
        pair.do(("set_costmap", "set_occupancy")[k], shape)
        pair.do("set_inflation", infl_cfg(INFL_RADII[i % 3], res), k)
        pair.do("upload", FRAME_SEEDS[i % 3])
        source_run(pair, k, i)
        if i:
            out.append(pair.fetch(k))                           # still the old shape's, every one
        out.append(pair.chain(k, GOALS[k], POSES[k]))
    return out


def part_a_strides(pair, k):
    """max_path 64 -> 256 -> 32 and the three local-plan configurations at a fixed shape: the buffers grow once and are kept."""
    setup(pair, k)
    source_run(pair, k)
    pair.do("inflate_async", k)
    out = []
    for i, (mp, loc) in enumerate(zip(MAX_PATHS, LOCS)):       # (another goal per stream each time: what a kept buffer holds is stale)
        pair.do("set_navfn", dict((NAV_CM, NAV_OCC)[k], max_path=mp), k)
        pair.do("set_local_planner", loc, k)
        pair.do("navfn_async", np.roll(GOALS[k], i, axis=0), k)
        pair.do("local_plan_async", POSES[k], None, k)
        out.append(pair.fetch(k))
    return out


def part_a_movers(pair):
    """The costmap source with movers: horizon 4 -> 0 -> 4 between calls, and the movers off between a run and its getters."""
    k, getters = 0, GETTERS + ("local_movers",)
    setup(pair, k)
    tracks = pair.track(TRACK_STEPS)
    source_run(pair, k)
    out = []
    for h in (4, 0, 4):
        pair.do("set_local_movers", dict(MOV, horizon=h), k)
        out.append(pair.chain(k, GOALS[k], POSES[k], getters, tracks=tracks))
    pair.do("local_plan_async", POSES[k], None, k, tracks=tracks)
    pair.do("set_local_movers", None, k)
    out.append(pair.fetch(k, getters))                          # the run had movers: its result keeps them
    pair.do("local_plan_async", POSES[k], None, k)
    out.append(pair.fetch(k, GETTERS))
    assert pair.do("local_movers", k)[0] == "refused"
    return out


# ---- part B: set_* between a run and what rests on it ----
# a row: (name, source, change, place, getters).  The chain's calls are source run, inflate, navfn, local plan; `change`
# (a list of operations) comes behind the first `place` of them and the rest follow; then every getter.  The STALE order,
# which tests/test_nav_reconfig_host.py shows to give other bytes, has `change` in front of the source run.
CHAIN = ("source", "inflate_async", "navfn_async", "local_plan_async")
OTHER_NAV = (dict(NAV_CM, max_path=32, connectivity=4), dict(NAV_OCC, max_path=32, connectivity=4))
ROWS = []
for _k in (0, 1):
    _s = SOURCES[_k]
    _res = (0.05, 0.1)[_k]
    ROWS += [(f"{_s}-set_navfn-behind-navfn", _k, [("set_navfn", OTHER_NAV[_k], _k)], 3, LOC_1),
             (f"{_s}-set_navfn-behind-local_plan", _k, [("set_navfn", OTHER_NAV[_k], _k)], 4, LOC_1),
             (f"{_s}-larger-planner-behind-local_plan", _k, [("set_local_planner", LOC_2, _k)], 4, LOC_1),
             (f"{_s}-smaller-planner-behind-local_plan", _k, [("set_local_planner", LOC_3, _k)], 4, LOC_2),
             (f"{_s}-set_inflation-behind-inflate", _k, [("set_inflation", infl_cfg(7, _res), _k)], 2, LOC_1),
             (f"{_s}-set_inflation-behind-navfn", _k, [("set_inflation", infl_cfg(7, _res), _k)], 3, LOC_1)]
for _place in (1, 2, 3, 4):
    ROWS += [(f"costmap-moved-behind-{CHAIN[_place - 1]}", 0, [("set_costmap", CM_A_MOVED)], _place, LOC_1),
             (f"costmap-coarse-behind-{CHAIN[_place - 1]}", 0, [("set_costmap", CM_A_COARSE), ("set_inflation", infl_cfg(4, 0.1), 0)], _place, LOC_1),
             (f"occupancy-same-map-behind-{CHAIN[_place - 1]}", 1, [("set_occupancy", OCC_SAME_MAP)], _place, LOC_1)]
ROW_NAMES = [r[0] for r in ROWS]


def part_b_row(pair, name, stale=False):
    """Runs row `name` (stale: its change in front of the source run) -> the model's answers of every getter at the end."""
    _, k, change, place, loc = ROWS[ROW_NAMES.index(name)]
    setup(pair, k, loc=loc)
    calls = [lambda: source_run(pair, k), lambda: pair.do("inflate_async", k), lambda: pair.do("navfn_async", GOALS[k], k),
             lambda: pair.do("local_plan_async", POSES[k], None, k)]
    refused = False
    for i, call in enumerate(calls):
        if i == (0 if stale else place):
            for op in change:
                pair.do(*op)
        want = call()
        refused = refused or (want is not None and want[0] == "refused")
    if place == 4 and not stale:
        for op in change:
            pair.do(*op)
    out = pair.fetch(k)
    if refused:
        out = pair.fetch(k)                                     # unchanged(): a refusal moved nothing
    return out


# ... and the rows that end in a refusal or in a source switched off, behind a complete chain
def part_b_forgotten(pair, cfg, infl):
    """set_occupancy with another resolution or shape: the maps are forgotten, inflate_async is refused, everything made
    before stays fetchable and unchanged."""
    k = 1
    setup(pair, k)
    source_run(pair, k)
    before = pair.chain(k, GOALS[k])
    pair.do("set_occupancy", cfg)
    if infl is not None:
        pair.do("set_inflation", infl, k)
    want = pair.do("inflate_async", k)
    assert want == ("refused", R_NO_SRC_RUN[1]), want
    after = pair.fetch(k)                                       # unchanged()
    assert not any(differs(before[g], after[g]) for g in GETTERS)
    return after


def part_b_source_off(pair, k):
    """set_costmap(None) / set_occupancy(None) behind a complete chain: every getter answers from the runs' records, and so
    does a further navfn_async and local_plan_async -- the inflated grids and their frame are recorded; only inflate_async,
    which would read the source, is refused."""
    setup(pair, k)
    source_run(pair, k)
    before = pair.chain(k, GOALS[k], POSES[k])
    pair.do(("set_costmap", "set_occupancy")[k], None)
    after = pair.fetch(k)
    assert not any(differs(before[g], after[g]) for g in GETTERS)
    assert pair.do("inflate_async", k) == ("refused", R_SRC_OFF.format(SOURCES[k]))
    assert not any(differs(before[g], pair.fetch(k)[g]) for g in GETTERS)          # unchanged()
    assert pair.do("navfn_async", np.roll(GOALS[k], 1, axis=0), k)[0] == "ok"
    assert pair.do("local_plan_async", POSES[k], None, k)[0] == "ok"
    return before, pair.fetch(k)


def run_walk(pair, seed, n=WALK_OPS):
    for op in walk_start() + walk_ops(seed, n):
        pair.do(*op)
    return pair.log[len(walk_start()):]
