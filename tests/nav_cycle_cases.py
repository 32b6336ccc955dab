"""One navigation cycle with every resident-frame stage on: the scenario, the chain of the package's own numpy restatements
(HostChain / host_chain) and the comparison both tests/test_nav_cycle_host.py and tests/test_gpu_nav_cycle.py hold a run to.
Pure numpy up to `configure`; the functions below it drive an Engine and are shared by the GPU tests and by the child process
one of them starts (python tests/nav_cycle_cases.py).

A cycle is a dict: frames [B x [n, 4] float32], poses [B, 3, 4], stamps [B], planes [B, 6, 4]; the tracker's dt comes from
the stamps (tracking.stamps_to_dt).  What a cycle gives is a dict as well: HostChain.step fills every key, a GPU run the
keys it fetched (fetch_all), and same_as_chain / same_bytes compare the keys they find."""
import copy
import hashlib
import os
import re

import numpy as np

STREAMS = 3
NMAX = 512
F = 4
MARGIN = 1e-9        # metres: under it a costmap cell's membership is undecided (tests/test_gpu_costmap.py)
UNDECIDED_CAP = 0.001

# ---- stage configurations, each the one its own test file uses ----
SWEEPS = {"history": 2, "capacity": 200, "history_decimate": 1, "max_age": 0.25, "time_feature": 3}
TRACK = dict(gate=1.25, birth_score=0.3, max_misses=2, min_hits=2, q_acc=4.0, r_pos=0.01)
GRID = dict(x_min=-0.5, y_min=-1.0, resolution=0.05, width=51, height=43, z_min=-1.0, z_max=1.0)
COSTMAP = dict(GRID, objects="tracks", horizon_steps=2)
OCC = dict(resolution=0.1, z_min=0.0, z_max=1.0, max_range=2.5, width=37, height=29)
INFL_COSTMAP = dict(resolution=0.05, inscribed_radius=0.05, inflation_radius=0.2, cost_scaling_factor=8.0)          # 4 cells
INFL_OCC = dict(resolution=0.1, inscribed_radius=0.1, inflation_radius=0.5, cost_scaling_factor=4.0, lethal_threshold=65)   # 5 cells
# the planner behind both inflations: 5 x 13 = 65 samples (a wave and one lane).  The costmap's navigation function queues
# ONE round: on 51 x 43 cells (2 x 2 tiles) the field is never settled at the call, so every fetch goes through the
# getter's settle and its second rollout.  Both grids are unknown where nothing was seen and the scene is dense (the
# sensor's own cell often lies in an inscribed band): unknown cells pass and only the obstacles themselves block.  The
# movers' horizons are short for the same reason: the tracks of this scene are many, close and fast.
NAV_CM = dict(lethal_cost=100, allow_unknown=1, unknown_cost=30, max_path=256, queued_rounds=1)
NAV_OCC = dict(lethal_cost=100, allow_unknown=1, unknown_cost=20, max_path=256)
LOC_CM = dict(nv=5, nw=13, steps=8, lookahead=1024, pot_weight=8, occ_weight=4, speed_weight=1, turn_weight=1)
LOC_OCC = dict(nv=5, nw=13, steps=6, lookahead=512, pot_weight=16, occ_weight=8, speed_weight=2, turn_weight=1)
MOV_CM = dict(horizon=4, mover_weight=64, pad_hard=0.0, pad_soft=0.15, confirmed_only=False)
MOV_OCC = dict(horizon=3, mover_weight=100, pad_hard=0.0, pad_soft=0.25, confirmed_only=True)
LIMITS = dict(v_min=-0.1, v_max=0.4, w_max=1.5, acc_v=1.0, acc_w=4.0, sim_time=1.0, period=0.2)
PLAN_DT = 0.125      # seconds per rollout step, for both sources
# What the costmap's planner is asked per cycle (row i % 9) and stream: a goal (x, y) and the robot's pose (x, y, yaw),
# metres and radians in the sensor frame.  The scene is dense -- nine points in ten have y < 0, the sweeps carry old points
# back over the sensor's own cell, eight to eleven tracks stand in it --, so the rows were chosen on the host chain
# (tests/test_nav_cycle_host.py asserts what they reach): every goal is free, every pose lies on a free, reached cell
# and sees collisions, cells the field does not reach and, from cycle 1 on, movers among its 65 samples.
PLAN_CM = [
    [(-0.3, 0.5, 0.03, 0.12, -1.1), (1.9, 0.9, 0.78, 0.12, -1.9), (1.5, 1.0, 0.78, 0.12, -1.9)],
    [(0.6, 1.0, 0.78, 0.12, -1.9), (-0.2, 1.05, 0.03, 0.12, -1.9), (-0.3, 0.5, -0.27, 0.92, -0.4)],
    [(-0.2, 1.05, 1.68, 1.07, -0.4), (0.2, 0.95, 0.33, 0.92, 0.5), (-0.4, 0.8, -0.12, 0.92, -1.1)],
    [(1.9, 0.9, -0.12, 0.12, -1.1), (1.5, 1.0, 1.68, 1.07, 0.5), (1.3, 0.8, 0.03, 0.42, -1.1)],
    [(1.95, 0.3, -0.12, 0.12, -1.1), (0.2, 0.95, 0.03, 0.92, -1.9), (1.0, 1.0, 0.33, 0.72, -1.9)],
    [(0.2, 0.95, 0.33, 0.12, -1.9), (-0.4, 0.8, -0.12, 0.72, 0.5), (-0.4, 0.1, 1.23, 0.92, -1.9)],
    [(1.5, 1.0, 0.03, 0.12, -1.1), (-0.2, 1.05, 0.03, 0.92, -0.4), (-0.3, 0.5, 0.33, 0.42, -0.4)],
    [(-0.3, 0.5, 0.33, 0.12, -1.9), (1.0, 1.0, 0.78, 0.12, -1.1), (0.6, 1.0, 0.33, 0.12, -1.9)],
    [(-0.4, 0.8, 0.33, 0.12, -1.9), (1.95, 0.3, 0.33, 0.12, -0.4), (-0.2, 1.05, 0.33, 0.12, -1.9)],
]
# ... and the occupancy maps' goals per cycle (row i % 9) and stream, offsets in metres from the stream's pose: two lie
# outside every window (goal_state 2, cmd_state 4) and two at the pose itself (arrived, cmd_state 2), each between two
# cycles of its stream that give a command
GOALS_OCC = [
    [(1.0, 0.5), (0.6, -0.9), (-1.1, -0.6)],
    [(-0.8, 0.7), (1.3, -0.2), (0.0, 0.0)],
    [(0.6, -0.9), (-1.1, -0.6), (-0.8, 0.7)],
    [(1.3, -0.2), (1.0, 0.5), (0.6, -0.9)],
    [(-1.1, -0.6), (-0.8, 0.7), (1.3, -0.2)],
    [(1.0, 0.5), (0.6, -0.9), (-1.1, -0.6)],
    [(-0.8, 0.7), (1.3, -0.2), (9.0, 0.0)],
    [(0.0, 0.0), (-1.1, -0.6), (-0.8, 0.7)],
    [(1.3, -0.2), (9.0, 0.0), (0.6, -0.9)],
]
NAV_TILE = 32        # csrc/navfn.hip: a workgroup relaxes a tile of 32 x 32 cells per round
SRC = (("cm", "costmap"), ("occ", "occupancy"))
IMAGE_SHAPES = [(8, 4), (6, 5), (10, 3)]      # (height, width) per stream under default_calib's identity camera matrix

# rows of stream 0, 1, 2 per cycle, from {0, 1, 63, 64, 65, 257}: empty, a single row, a wave and one row either side of
# it, two chunks of 256 rows (tests/test_gpu_sweeps.py); every stream sees all six, cycle 0 has no empty frame, and
# stream 0's three 257s in a row overflow both the sweeps' capacity (200) and the frame (512)
SIZES = [[257, 64, 65], [257, 65, 1], [257, 63, 257], [0, 257, 64], [65, 1, 257], [63, 0, 65], [257, 257, 0], [64, 257, 257],
         [1, 65, 63]]
# metres per cycle sideways, per stream.  Stream 2's carries its window over a cell border between cycles 5 and 6, where
# its frame is empty: an empty frame under a window that stands would leave the occupancy map, and so its inflated grid,
# what it was, and a stale grid would pass for this cycle's
DRIFT_Y = (-0.03, 0.0, 0.035)
GAP_AFTER = 4        # the stamps jump by more than max_age between cycles 4 and 5

OCC_INFO = ("hits", "ground", "ignored", "cells_hit", "cells_free", "cleared")
SWEEP_INFO = ("count", "used", "truncated", "push_truncated")
TRACK_FIELDS = ("state", "size", "yaw", "score", "id", "label", "hits", "misses", "confirmed", "det_row", "reserved")


def ring_turn(pp):
    """2 * OFF_RING + 1 calls: one more than two turns of a call ring, with the depth read from csrc/pp_ring.h."""
    with open(os.path.join(os.path.dirname(pp._lib.__file__), "csrc", "pp_ring.h")) as f:
        depth = int(re.search(r"constexpr\s+int\s+OFF_RING\s*=\s*(\d+)\s*;", f.read()).group(1))
    return 2 * depth + 1


def config(pp):
    cfg = copy.deepcopy(pp.config.tiny_config(STREAMS))
    cfg["model"]["second"]["num_point_features"] = F
    for reader in ("eval_input_reader", "train_input_reader"):
        if reader in cfg:
            cfg[reader]["num_point_features"] = F
    return cfg


def weights(pp, d):
    w = dict(pp.weights.init_weights(d, seed=7))
    w["rpn/conv_cls/bias"] = np.array(w["rpn/conv_cls/bias"], np.float32) + np.float32(0.6)     # the passes keep rows
    return w


def calib(pp, B=STREAMS):
    rect, trv, p2 = pp.synth.default_calib()
    return np.stack([rect] * B), np.stack([trv] * B), np.asarray(p2, np.float64)


def planes(pp):
    rect, trv, p2 = pp.synth.default_calib()
    return np.stack([pp.frustum.frustum_planes(rect, trv, p2, shp) for shp in IMAGE_SHAPES])


def _frame(rng, n):
    """n rows inside the tiny range (x 0 .. 1.6, y -0.64 .. 0.64).  The camera of default_calib looks along +x and its
    image holds y < 0, z < 0 only, so nine rows in ten are drawn there (the crop keeps most of them, and drops those too
    close to the sensor for the image); the others, 0 < z < 1, are what the crop drops and the occupancy map counts as hits."""
    seen = rng.random(n) < 0.9
    x = rng.uniform(0.05, 1.55, n)
    y = np.where(seen, rng.uniform(-0.6, -0.01, n), rng.uniform(-0.6, 0.6, n))
    z = np.where(seen, rng.uniform(-1.0, -0.01, n), rng.uniform(0.05, 1.0, n))
    return np.ascontiguousarray(np.stack([x, y, z, rng.random(n)], 1).astype(np.float32))


def sequence(pp, cycles=None, seed=11):
    """`cycles` (default: ring_turn) cycles of STREAMS frames: a slow planar ego motion per stream that carries the
    occupancy window over cell borders, stamps 0.1 s apart (stream b offset by b seconds) with one gap of 0.5 s."""
    cycles = ring_turn(pp) if cycles is None else cycles
    rng = np.random.default_rng(seed)
    pl = planes(pp)
    out = []
    for i in range(cycles):
        row = SIZES[i % len(SIZES)]
        frames = [_frame(rng, n) for n in row]
        poses = np.stack([pp.sweeps.pose_from_xyyaw(0.04 * i + rng.normal() * 0.004, DRIFT_Y[b] * i + rng.normal() * 0.004,
                                                    0.03 * i * (b + 1)) for b in range(STREAMS)])
        t = 0.1 * i + (0.4 if i > GAP_AFTER else 0.0)
        out.append(dict(frames=frames, poses=poses, stamps=np.array([t + b for b in range(STREAMS)]), planes=pl,
                        **plan_inputs(i, poses)))
    return out


def plan_inputs(i, poses):
    """What the planner is asked in cycle i (no random draw: the frames above stay what they were): a goal per stream and
    source in metres -- the sensor frame for the costmap, the fixed frame (the stream's pose plus an offset) for the
    occupancy maps -- that moves with the cycle, the current velocity (v m/s, w rad/s) of LIMITS' window, and the robot's
    pose (x, y, yaw) in the costmap (the default, the sensor's own cell, lies in an obstacle in most cycles: the sweeps
    carry old points back over it; the occupancy source keeps the default, the pose of its update)."""
    xy = poses[:, :2, 3]
    asked = np.array(PLAN_CM[i % len(PLAN_CM)], np.float64)
    goals_cm, pose_cm = asked[:, :2], asked[:, 2:]
    goals_occ = xy + np.array(GOALS_OCC[i % len(GOALS_OCC)], np.float64)
    vel = np.array([[0.05 + 0.03 * ((i + b) % 5), 0.25 * ((i + 2 * b) % 5 - 2)] for b in range(STREAMS)], np.float64)
    return dict(goals_cm=goals_cm, goals_occ=goals_occ, velocities=vel, poses_cm=pose_cm)


def short_at(cycles):
    """The cycle that runs with 2 of the 3 streams in the stream-independence cases: two thirds through, behind the stamp
    gap, where stream 1 holds two young sweeps again (a reset that did nothing would show) and the next cycles' frames
    of streams 1 and 2 are not empty."""
    return (2 * cycles) // 3


def short(cycle, B):
    """The cycle for streams 0 .. B - 1 only."""
    return {k: v[:B] for k, v in cycle.items()}


# ---- the host chain ----
class HostChain:
    """The restatements in the order the engine documents; `detect(frames) -> (dets [B, rows], n [B], bboxes or None)`."""

    def __init__(self, pp, detect):
        self.pp, self.detect = pp, detect
        self.maps = [pp.occupancy.OccupancyMap(OCC) for _ in range(STREAMS)]
        self.acc = pp.sweeps.SweepAccumulator(SWEEPS, STREAMS, F, NMAX)
        self.tracker = pp.tracking.Tracker(pp.tracking.TrackConfig(**TRACK), STREAMS)
        self.last = np.full(STREAMS, np.nan)
        self.cm = pp.costmap.CostmapConfig.from_any(COSTMAP)
        self.ic = pp.inflation.InflationConfig(**INFL_COSTMAP)
        self.io = pp.inflation.InflationConfig(**INFL_OCC)

    def reset(self, stream):
        """What sweeps_reset, occupancy_reset and track_reset of one stream do together."""
        self.maps[stream].reset()
        self.acc.reset(stream)
        self.tracker.reset(stream)
        self.last[stream] = np.nan

    def step(self, cycle):
        pp, B = self.pp, len(cycle["frames"])
        out = {}
        # 1. the occupancy maps, from the frames as they arrive
        info = [self.maps[b].update(cycle["frames"][b], cycle["poses"][b]) for b in range(B)]
        out["occ_grid"] = np.stack([self.maps[b].grid() for b in range(B)])
        out["occ_logodds"] = np.stack([self.maps[b].logodds() for b in range(B)])
        out["occ_origin"] = np.array([self.maps[b].origin for b in range(B)], np.float64)
        out["occ_info"] = {k: np.array([w[k] for w in info], np.int32) for k in OCC_INFO}
        # 2. the crop, 3. the sweeps
        out["cropped"] = [pp.frustum.crop_np(cycle["frames"][b], cycle["planes"][b]) for b in range(B)]
        out["kept"] = np.array([len(c) for c in out["cropped"]], np.int32)
        out["accumulated"], out["sweeps_info"] = self.acc.accumulate(out["cropped"], cycle["poses"], cycle["stamps"])
        # 4. the pass, 5. its tracking step
        dets, n, bboxes = self.detect(out["accumulated"])
        out["dets"], out["n"], out["bboxes"] = dets[:B].copy(), np.asarray(n[:B], np.int32).copy(), bboxes
        dt, new_last = pp.tracking.stamps_to_dt(self.last[:B], cycle["stamps"], B, self.tracker.cfg.period)
        self.last[:B] = new_last
        out["dt"] = dt
        out["tracks"] = self.tracker.step(out["dets"], out["n"], dt, poses=cycle["poses"])
        out["tracks_fixed"] = self.tracker.tracks_fixed(B)
        out["track_info"] = self.tracker.info()
        # 6. the costmap of the accumulated frames and the tracks
        tr, nt, _ = out["tracks"]
        C = pp.costmap
        grids, counts, und, fps = [], [], [], []
        for b in range(B):
            g, k = C.costmap_np(out["accumulated"][b], self.cm, tracks=tr[b], n_tracks=int(nt[b]))
            fp = C.footprints_np(self.cm, tracks=tr[b], n_tracks=int(nt[b]))
            grids.append(g)
            counts.append(k)
            fps.append(len(fp))
            und.append(C.decision_margins(self.cm, fp) < MARGIN)
        out["cm_grid"], out["cm_counts"], out["cm_undecided"] = np.stack(grids), np.stack(counts), np.stack(und)
        a = out["accumulated"]
        with np.errstate(invalid="ignore"):
            ing = [int((((f[:, 0].astype(np.float64) - GRID["x_min"]) / GRID["resolution"] >= 0)
                        & (np.floor((f[:, 0].astype(np.float64) - GRID["x_min"]) / GRID["resolution"]) < GRID["width"])
                        & ((f[:, 1].astype(np.float64) - GRID["y_min"]) / GRID["resolution"] >= 0)
                        & (np.floor((f[:, 1].astype(np.float64) - GRID["y_min"]) / GRID["resolution"]) < GRID["height"])).sum())
                   for f in a]
        out["cm_info"] = {"points_in_grid": np.array(ing, np.int32), "footprints": np.array(fps, np.int32)}
        # 7. both inflations
        out["infl_cm"] = inflate_all(pp, out["cm_grid"], self.ic)
        out["infl_occ"] = inflate_all(pp, out["occ_grid"], self.io)
        # 8. per source: the field and the path, the movers from the tracks, the command
        out["plan_in"] = plan_in(cycle)
        out["plan_origin_occ"] = out["occ_origin"].copy()
        out.update(plan_np(pp, "cm", out["infl_cm"][0], out["plan_in"], cm_origins(B), out["tracks"][0], out["tracks"][1]))
        out.update(plan_np(pp, "occ", out["infl_occ"][0], out["plan_in"], out["occ_origin"], *out["tracks_fixed"]))
        return out


def inflate_all(pp, grids, cfg):
    """inflate_np per grid -> (grids, dist2, {"lethal", "raised"} int32 [B])."""
    res = [pp.inflation.inflate_np(g, cfg, clearance=True, info=True) for g in grids]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]),
            {k: np.array([r[2][k] for r in res], np.int32) for k in ("lethal", "raised")})


# ---- the planner's restatements on one source's inflated grids (HostChain.step on the chain's, same_plan on a run's own) ----
PLAN_KEYS = ("field", "paths", "paths_m", "nav_info", "plan_info", "traj", "keys", "movers")
_PLANNED = {}        # one grid's results by everything they depend on: most runs repeat the chain's grids


def plan_in(cycle):
    """What the planner was asked in this cycle, kept with the results: same_plan needs nothing else."""
    return {k: np.array(cycle[k], np.float64) for k in ("goals_cm", "goals_occ", "velocities", "poses", "poses_cm")}


def cm_origins(B):
    return np.tile(np.array([[GRID["x_min"], GRID["y_min"]]], np.float64), (B, 1))


def plan_configs(pp, s):
    """(NavfnConfig, LocalPlanConfig, MoverConfig, resolution) of source s."""
    N, L = pp.navfn, pp.local_planner
    if s == "cm":
        return N.NavfnConfig(**NAV_CM), L.LocalPlanConfig(**LOC_CM), L.MoverConfig(**MOV_CM), GRID["resolution"]
    return N.NavfnConfig(**NAV_OCC), L.LocalPlanConfig(**LOC_OCC), L.MoverConfig(**MOV_OCC), OCC["resolution"]


def plan_windows(pp, s, velocities):
    """LIMITS' dynamic window round each stream's current velocity, int32 [B, 4]."""
    _, lcfg, _, res = plan_configs(pp, s)
    lim = pp.local_planner.LocalLimits(**LIMITS)
    return np.array([lim.window(v, w, lcfg.nv, lcfg.nw, res) for v, w in np.asarray(velocities)], np.int32)


def plan_cells(pp, s, asked, origins, shape):
    """(goal cells [B, 2], start cells [B, 2], pose ticks [B, 3]) as navfn_async and local_plan_async make them: the paths
    start at the sensor's cell; the robot stands at the scenario's pose in the costmap and, by default, at the update's
    pose in the occupancy maps."""
    N, L = pp.navfn, pp.local_planner
    res = plan_configs(pp, s)[3]
    B = len(origins)
    if s == "cm":
        goals = N.goal_cells(asked["goals_cm"][:B], origins, res, shape)
        starts = N.goal_cells(np.zeros((B, 2)), origins, res, shape)
        ticks = L.pose_ticks(asked["poses_cm"][:B, :2], asked["poses_cm"][:B, 2], origins, res)
    else:
        T = asked["poses"][:B]
        goals = N.goal_cells(asked["goals_occ"][:B], origins, res, shape)
        starts = np.tile(np.array([[shape[1] // 2, shape[0] // 2]], np.int32), (B, 1))
        ticks = L.pose_ticks(T[:, :2, 3], np.arctan2(T[:, 1, 0], T[:, 0, 0]), origins, res)
    return goals, starts, ticks


def _plan_one(pp, s, grid, goal, start, ticks, window, origin, rows, n):
    N, L = pp.navfn, pp.local_planner
    ncfg, lcfg, mcfg, res = plan_configs(pp, s)
    key = (s, grid.tobytes(), goal.tobytes(), start.tobytes(), ticks.tobytes(), window.tobytes(), np.asarray(origin, np.float64).tobytes(),
           int(n), rows[:max(int(n), 0)].tobytes())
    if key not in _PLANNED:
        pot, info = N.navfn_np(grid, goal, ncfg, info=True)
        path, pstate = N.descend_np(pot, grid, start, ncfg)
        movers, nm, skipped = L.movers_np(rows, n, origin, res, PLAN_DT, mcfg)
        best = L.best_np(grid, pot, ticks, window, ncfg, lcfg, info["goal_state"], movers=movers[:max(nm, 0)], mcfg=mcfg)
        best["n_movers"], best["n_skipped"] = nm, skipped
        _PLANNED[key] = (pot, path, N.path_to_metres(path, origin, res), dict(info, path_state=pstate), best, movers)
    return _PLANNED[key]


def plan_np(pp, s, grids, asked, origins, tracks, n_tracks):
    """navfn_np, descend_np, movers_np and best_np per grid of source s ("cm" / "occ") -> the planner's keys of a cycle's dict,
    in the shapes fetch_plan gives them."""
    L = pp.local_planner
    B, shape = len(grids), grids.shape[1:]
    goals, starts, ticks = plan_cells(pp, s, asked, origins, shape)
    wins = plan_windows(pp, s, asked["velocities"][:B])
    res = [_plan_one(pp, s, grids[b], goals[b], starts[b], ticks[b], wins[b], origins[b], tracks[b], n_tracks[b]) for b in range(B)]
    words = L.RESULT + ("n_movers", "n_skipped", "n_dynamic", "near")
    info = {k: np.array([r[4][k] for r in res], np.int32) for k in words}
    info["score"] = np.array([r[4]["score"] for r in res], np.uint64)
    return {f"field_{s}": np.stack([r[0] for r in res]), f"paths_{s}": [r[1] for r in res], f"paths_m_{s}": [r[2] for r in res],
            f"nav_info_{s}": {k: np.array([r[3][k] for r in res], np.int32) for k in ("goal_state", "path_state", "reached")},
            f"plan_info_{s}": info, f"traj_{s}": [r[4]["traj"] for r in res], f"keys_{s}": np.stack([r[4]["keys"] for r in res]),
            f"movers_{s}": np.stack([r[5] for r in res])}


def host_chain(seq, detect, pp=None):
    """Per cycle, everything the GPU is to produce."""
    if pp is None:
        import pp_amd as pp
    chain = HostChain(pp, detect)
    return [chain.step(c) for c in seq]


def oracle_detector(pp):
    """detect() for the host test: the CPU oracle's pass (tests/util_ref.oracle_detect) as Engine.detections() rows."""
    import util_ref
    from pp_amd.engine import DET_DTYPE
    d = pp.config.Derived(config(pp))
    w = weights(pp, d)
    rect, trv, p2 = pp.synth.default_calib()
    rows = d.nms_dict()["nms_post_max_size"]

    def detect(frames):
        ref = util_ref.oracle_detect(d, w, [np.ascontiguousarray(f) for f in frames], rect, trv, p2)
        dets, n = np.zeros((len(frames), rows), DET_DTYPE), np.zeros(len(frames), np.int32)
        for b, r in enumerate(ref["dets"]):
            k = 0 if r["scores"] is None else len(r["scores"])
            n[b] = k
            if k:
                dets["box3d_lidar"][b, :k] = r["box3d_lidar"]
                dets["box3d_camera"][b, :k] = r["box3d_camera"]
                dets["score"][b, :k] = r["scores"]
                dets["label"][b, :k] = r["label_preds"]
        return dets, n, None
    return detect


# ---- the comparison ----
def dets_bytes(dets, n):
    return [dets[b, :n[b]].tobytes() for b in range(len(n))]


def same_tracks(got, want, what):
    (gt, gn, go), (wt, wn, wo) = got, want
    assert np.array_equal(gn, wn), (what, gn, wn)
    assert np.array_equal(go, wo), (what, go, wo)
    for f in TRACK_FIELDS:
        assert np.array_equal(gt[f], wt[f]), (what, f)
    assert gt.tobytes() == wt.tobytes(), what


def same_as_chain(got, want, what, streams=None):
    """Everything a run fetched (the keys of `got`) against the chain's cycle `want`.  streams: the streams to hold (all)."""
    ss = list(range(len(want["n"]))) if streams is None else list(streams)
    if "kept" in got:
        assert np.array_equal(got["kept"][ss], want["kept"][ss]), (what, "kept", got["kept"], want["kept"])
    if "sweeps_info" in got:
        for k in SWEEP_INFO:
            assert np.array_equal(got["sweeps_info"][k][ss], want["sweeps_info"][k][ss]), (what, "sweeps_info", k)
    for key in ("cropped", "accumulated"):
        if key in got:
            for b in ss:
                assert got[key][b].shape == want[key][b].shape and got[key][b].tobytes() == want[key][b].tobytes(), (what, key, b)
    if "dets" in got:
        assert np.array_equal(got["n"][ss], want["n"][ss]), (what, "n", got["n"], want["n"])
        g, w = dets_bytes(got["dets"], got["n"]), dets_bytes(want["dets"], want["n"])
        assert [g[b] for b in ss] == [w[b] for b in ss], (what, "detections")
    if "bboxes" in got and want["bboxes"] is not None:
        assert np.array_equal(got["bboxes"][ss], want["bboxes"][ss]), (what, "bboxes")
    if "tracks" in got:
        pick = lambda t: tuple(a[ss] for a in t)
        same_tracks(pick(got["tracks"]), pick(want["tracks"]), (what, "tracks"))
        (ft, fn), (rt, rn) = pick(got["tracks_fixed"]), pick(want["tracks_fixed"])
        same_tracks((ft, fn, fn), (rt, rn, rn), (what, "fixed tracks"))
        for k in ("live", "next_id", "overflow"):
            assert np.array_equal(got["track_info"][k][ss], want["track_info"][k][ss]), (what, "track_info", k)
    und = want["cm_undecided"]
    if "cm_grid" in got:
        assert int(und.sum()) <= UNDECIDED_CAP * und.size, (what, "undecided cells", int(und.sum()))
        assert np.array_equal(got["cm_counts"][ss], want["cm_counts"][ss]), (what, "costmap counts")
        for b in ss:
            assert np.array_equal(got["cm_grid"][b][~und[b]], want["cm_grid"][b][~und[b]]), (what, "costmap", b)
        for k in ("points_in_grid", "footprints"):
            assert np.array_equal(got["cm_info"][k][ss], want["cm_info"][k][ss]), (what, "costmap_info", k)
    if "occ_grid" in got:
        for k in ("occ_logodds", "occ_grid", "occ_origin"):
            assert np.array_equal(got[k][ss], want[k][ss]), (what, k)
        for k in OCC_INFO:
            assert np.array_equal(got["occ_info"][k][ss], want["occ_info"][k][ss]), (what, "occupancy_info", k)
    for key in ("infl_cm", "infl_occ"):
        if key in got:
            for b in ss:
                if key == "infl_cm" and und[b].any():
                    continue                          # (held to inflate_np of the run's own grid instead: same_inflation)
                assert np.array_equal(got[key][1][b], want[key][1][b]), (what, key, "dist2", b)
                assert np.array_equal(got[key][0][b], want[key][0][b]), (what, key, b)
                for k in ("lethal", "raised"):
                    assert got[key][2][k][b] == want[key][2][k][b], (what, key, k, b)
    # the planner: the occupancy source always; the costmap source where the chain's grid is the run's (same_plan holds the rest)
    if "plan_in" in got:
        for k, v in want["plan_in"].items():
            assert np.array_equal(got["plan_in"][k][ss], v[ss]), (what, "asked", k)
    if "plan_origin_occ" in got:
        assert np.array_equal(got["plan_origin_occ"][ss], want["plan_origin_occ"][ss]), (what, "the occupancy frame of the plan")
    _same_planned(got, want, "occ", ss, what)
    _same_planned(got, want, "cm", [b for b in ss if not und[b].any()], what)


def _same_planned(got, want, s, ss, what):
    """The planner's keys of source s that `got` holds against `want`'s, streams ss; exact."""
    for name in PLAN_KEYS:
        key = f"{name}_{s}"
        if key not in got:
            continue
        g, w = got[key], want[key]
        if isinstance(w, dict):
            for k in w:                                 # (a run also has the rounds the GPU took: implementation-defined)
                assert g[k].dtype == w[k].dtype and np.array_equal(g[k][ss], w[k][ss]), (what, key, k, g[k], w[k])
        else:
            for b in ss:
                assert g[b].dtype == w[b].dtype and g[b].shape == w[b].shape and np.array_equal(g[b], w[b]), (what, key, b)


def same_plan(pp, got, what):
    """Every planner output of a run against the restatements on that run's OWN fetched inflated grids, tracks and origins
    (whether or not the cycle's costmap has undecided cells), under what the run was asked (got["plan_in"])."""
    for s, infl, rows in (("cm", "infl_cm", "tracks"), ("occ", "infl_occ", "tracks_fixed")):
        if not any(f"{name}_{s}" in got for name in PLAN_KEYS):
            continue
        grids = got[infl][0]
        origins = cm_origins(len(grids)) if s == "cm" else got["plan_origin_occ"]
        want = plan_np(pp, s, grids, got["plan_in"], origins, got[rows][0], got[rows][1])
        _same_planned(got, want, s, range(len(grids)), (what, "on the run's own grids"))


def same_inflation(pp, got, what):
    """Both inflated grids of a run against inflate_np of that run's own source grids."""
    for key, src, cfg in (("infl_cm", "cm_grid", INFL_COSTMAP), ("infl_occ", "occ_grid", INFL_OCC)):
        if key not in got:
            continue
        grid, d2, info = got[key]
        assert grid.dtype == np.int8 and d2.dtype == np.uint16
        wg, wd2, winfo = inflate_all(pp, got[src], pp.inflation.InflationConfig(**cfg))
        assert np.array_equal(d2, wd2), (what, key, "dist2")
        assert np.array_equal(grid, wg), (what, key)
        for k in ("lethal", "raised"):
            assert np.array_equal(info[k], winfo[k]), (what, key, k)


def _blobs(out):
    """The bytes of everything a run fetched, in a fixed order."""
    parts = []
    for key in sorted(out):
        v = out[key]
        if key == "dets":
            parts += dets_bytes(out["dets"], out["n"])
        elif isinstance(v, dict):
            parts += [np.ascontiguousarray(v[k]).tobytes() for k in sorted(v)]
        elif isinstance(v, (tuple, list)):
            for a in v:
                parts += [np.ascontiguousarray(a[k]).tobytes() for k in sorted(a)] if isinstance(a, dict) else [np.ascontiguousarray(a).tobytes()]
        else:
            parts.append(np.ascontiguousarray(v).tobytes())
    return parts


def digest(out):
    h = hashlib.sha256()
    for p in _blobs(out):
        h.update(len(p).to_bytes(8, "little"))
        h.update(p)
    return h.hexdigest()


def same_bytes(got, want, what):
    """Two runs' fetched outputs, byte for byte (the keys both hold)."""
    for key in sorted(set(got) & set(want)):
        a, b = _blobs({key: got[key], "n": got["n"]}), _blobs({key: want[key], "n": want["n"]})
        assert a == b, (what, key)


# ---- driving an Engine (GPU) ----
def configure(pp, eng):
    """Every stage of the cycle on one handle."""
    eng.load_weights(weights(pp, eng.d))
    eng.set_projection(calib(pp)[2])
    eng.set_sweeps(SWEEPS)
    eng.set_tracking(pp.tracking.TrackConfig(**TRACK))
    eng.set_track_ego(True)
    eng.set_costmap(COSTMAP)
    eng.set_occupancy(OCC)
    eng.set_inflation(INFL_COSTMAP, "costmap")
    eng.set_inflation(INFL_OCC, "occupancy")
    for source, nav, loc, mov in (("costmap", NAV_CM, LOC_CM, MOV_CM), ("occupancy", NAV_OCC, LOC_OCC, MOV_OCC)):
        eng.set_navfn(nav, source)
        eng.set_local_planner(loc, source)
        eng.set_local_movers(mov, source)
    rect, trv, _ = calib(pp)
    eng.set_calib(rect, trv, STREAMS)


def engine(pp):
    eng = pp.Engine(config(pp), max_batch=STREAMS, max_points_per_frame=NMAX)
    configure(pp, eng)
    return eng


def plain_engine(pp):
    """The callback's engine: no stage but the same projection, fed synchronously."""
    eng = pp.Engine(config(pp), max_batch=STREAMS, max_points_per_frame=NMAX)
    eng.load_weights(weights(pp, eng.d))
    eng.set_projection(calib(pp)[2])
    return eng


def plain_detector(pp, plain):
    rect, trv, _ = calib(pp)

    def detect(frames):
        B = len(frames)
        dets, n = plain.detect([np.ascontiguousarray(f) for f in frames], rect[:B], trv[:B])
        return dets[:B].copy(), n[:B].copy(), plain.bboxes(B).copy()
    return detect


def reset_all(eng):
    eng.sync()
    eng.sweeps_reset()
    eng.occupancy_reset()
    eng.track_reset()


def reset_stream(eng, stream):
    eng.sweeps_reset(stream)
    eng.occupancy_reset(stream)
    eng.track_reset(stream)


class Dt:
    """The tracker's dt of a run from the cycles' stamps, as HostChain works it out."""

    def __init__(self, pp, eng):
        self.pp, self.last, self.period = pp, np.full(STREAMS, np.nan), eng.tracking.period

    def __call__(self, stamps):
        B = len(stamps)
        dt, self.last[:B] = self.pp.tracking.stamps_to_dt(self.last[:B], stamps, B, self.period)
        return dt

    def reset(self, stream):
        self.last[stream] = np.nan


# THE CALL ORDER OF ONE CYCLE: INTEGRATION.md, "One navigation cycle", lists these thirteen steps, and
# tests/test_nav_cycle_host.py holds both that listing and run_queued's own calls to this tuple
CYCLE_CALLS = ("upload_async", "occupancy_update_async", "crop_to_image_async", "accumulate_sweeps_async", "set_track_dt",
               "set_track_pose", "detect_async", "costmap_async", 'inflate_async("costmap")', 'inflate_async("occupancy")',
               'navfn_async("costmap")', 'local_plan_async("costmap")', 'navfn_async("occupancy")', 'local_plan_async("occupancy")')
SOURCE_CALLS = ("inflate_async", "navfn_async", "local_plan_async")       # ... written with the source they name


def calls_in(text, prefix):
    """The calls `<prefix>.<name>(...)` of a text in order, as CYCLE_CALLS writes them."""
    out = []
    for c in re.finditer(re.escape(prefix) + r"\.(\w+)\(([^\n]*)", text):
        src = re.search(r'"(costmap|occupancy)"', c.group(2)) if c.group(1) in SOURCE_CALLS else None
        out.append(c.group(1) + (f'("{src.group(1)}")' if src else ""))
    return out


def queue_stages(eng, cycle, dt):
    """Steps 2 .. 9 behind a feed, nothing waited for."""
    eng.occupancy_update_async(cycle["poses"])                      # 2. before crop and sweeps: the frames as they arrived
    eng.crop_to_image_async(cycle["planes"])                        # 3.
    queue_behind_crop(eng, cycle, dt)


def queue_behind_crop(eng, cycle, dt):
    eng.accumulate_sweeps_async(cycle["poses"], cycle["stamps"])    # 4.
    eng.set_track_dt(dt)                                            # 5.
    eng.set_track_pose(cycle["poses"])
    eng.detect_async()                                              # 6.
    eng.costmap_async()                                             # 7.
    eng.inflate_async("costmap")                                    # 8.
    eng.inflate_async("occupancy")                                  # 9.
    queue_plan(eng, cycle)


def queue_plan(eng, cycle):
    """Steps 10 .. 13 behind both inflations: the default starts, the default pose in the occupancy maps, the window round
    the velocity."""
    import pp_amd as pp
    wc, wo = (plan_windows(pp, s, cycle["velocities"]) for s, _ in SRC)
    eng.navfn_async(cycle["goals_cm"], "costmap")                   # 10.
    eng.local_plan_async(cycle["poses_cm"], wc, "costmap", dt=PLAN_DT)      # 11.
    eng.navfn_async(cycle["goals_occ"], "occupancy")                # 12.
    eng.local_plan_async(None, wo, "occupancy", dt=PLAN_DT)         # 13.


def fetch_pass(eng, B):
    """What step 6 leaves."""
    out = {}
    dets, n = eng.detections()
    out["dets"], out["n"] = dets[:B].copy(), n[:B].copy()
    out["bboxes"] = eng.bboxes(B).copy()
    out["tracks"] = eng.tracks(B)
    out["tracks_fixed"] = eng.tracks_fixed(B)
    out["track_info"] = eng.track_info()
    return out


def fetch_costmap(eng):
    out = {}
    out["cm_grid"], out["cm_counts"] = eng.costmaps(counts=True)
    out["cm_info"] = eng.costmap_info()
    return out


def fetch_occupancy(eng):
    out = {}
    out["occ_grid"], out["occ_origin"], out["occ_logodds"] = eng.occupancy_maps(logodds=True)
    out["occ_info"] = eng.occupancy_info()
    return out


def fetch_inflated(eng):
    return {"infl_cm": eng._inflated(0, None, True) + (eng.inflation_info("costmap"),),
            "infl_occ": eng._inflated(1, None, True) + (eng.inflation_info("occupancy"),)}


def fetch_navfn(eng, cycle, sources=SRC):
    """What steps 10 and 12 leave, with what they were asked and the frame the engine gave the occupancy run."""
    out = {"plan_in": plan_in(cycle)}
    for s, source in sources:
        if s == "occ":
            out["plan_origin_occ"] = eng._navfn_run[1][3].copy()
        out[f"field_{s}"] = eng.navfn_fields(source)
        out[f"paths_{s}"] = eng.navfn_paths(source)[0]
        out[f"paths_m_{s}"] = eng.navfn_paths(source, metres=True)[0]
        out[f"nav_info_{s}"] = eng.navfn_info(source)
        assert np.array_equal(eng.navfn_paths(source)[1], out[f"nav_info_{s}"]["path_state"])
    return out


def fetch_local(eng, s, source, keys=True):
    """What step 11 or 13 leaves (keys=False: nothing that makes the getter roll the samples again for their keys)."""
    out = {f"plan_info_{s}": eng.local_plan_info(source), f"traj_{s}": eng.local_trajectories(source)}
    if keys:
        out[f"keys_{s}"] = eng.local_keys(source)
    out[f"movers_{s}"], minfo = eng.local_movers(source)
    assert all(np.array_equal(minfo[k], out[f"plan_info_{s}"][k]) for k in minfo)
    sv, sw, state = eng.local_commands(source)
    info = out[f"plan_info_{s}"]
    assert np.array_equal(sv, info["sv"]) and np.array_equal(sw, info["sw"]) and np.array_equal(state, info["cmd_state"])
    return out


def fetch_plan(eng, cycle):
    out = fetch_navfn(eng, cycle)
    for s, source in SRC:
        out.update(fetch_local(eng, s, source))
    return out


def fetch_all(eng, cycle, crop=True):
    out = {"sweeps_info": eng.sweeps_info()}
    if crop:
        out["kept"] = eng.crop_info()
    out.update(fetch_pass(eng, len(cycle["frames"])))
    out.update(fetch_costmap(eng))
    out.update(fetch_occupancy(eng))
    out.update(fetch_inflated(eng))
    out.update(fetch_plan(eng, cycle))
    return out


def run_queued(pp, eng, seq):
    """Every cycle fed by upload_async of a staging and queued with no host wait; fetched at the end of the cycle."""
    reset_all(eng)
    dts, outs, stagings = Dt(pp, eng), [], []
    for cycle in seq:
        st = eng.staging(cycle["frames"])
        stagings.append(st)
        eng.upload_async(st)                                        # 1.
        queue_stages(eng, cycle, dts(cycle["stamps"]))
        outs.append(fetch_all(eng, cycle))
    eng.sync()
    for st in stagings:
        st.close()
    return outs


def child_main():
    """The queued run of the whole sequence in this process; one digest per cycle on stdout."""
    import json
    import pp_amd as pp
    eng = engine(pp)
    try:
        outs = run_queued(pp, eng, sequence(pp))
    finally:
        eng.close()
    found = int(sum(o["n"].sum() for o in outs))
    print("NAV_CYCLE_DIGESTS " + json.dumps({"digests": [digest(o) for o in outs], "detections": found,
                                             "no_graph": os.environ.get("PP_NO_GRAPH", "")}))


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    child_main()
