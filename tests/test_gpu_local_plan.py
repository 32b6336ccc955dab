"""The local planner on the GPU (csrc/local_plan.hip: k_local_rollout, k_local_finish) against local_planner.py's
restatement: result words, scores, trajectories and all keys must be EQUAL (np.array_equal).  No tolerances: the device
works in integers and keys are unique, so no order shows in a result.  Stand-alone on the shared cases
(tests/local_plan_cases.py), then behind the navigation function of the costmap and of the rolling occupancy maps, whose
own outputs must stay the bytes of an engine that never heard of the stage; the getter's second rollout behind a field
that had not converged; a second inflation or a second occupancy update behind the call; the call ring; every refusal."""
import ctypes

import numpy as np
import pytest

import local_plan_cases as K

pytestmark = pytest.mark.gpu

OFF_RING = 4            # csrc/pp_ring.h


@pytest.fixture(scope="module")
def LP(pp, hip_lib):
    return pp.local_planner


def _equal(LP, got, want, what, keys=True):
    """`got` of local_plan / the engine for one grid against best_np's dict."""
    for k in LP.RESULT:
        assert int(got[k]) == want[k], (what, k, int(got[k]), want[k])
    assert int(got["score"]) == want["score"], what
    assert got["traj"].dtype == np.int32 and np.array_equal(got["traj"], want["traj"]), what
    if keys:
        assert got["keys"].dtype == np.uint64 and np.array_equal(got["keys"], want["keys"]), what


# ---- 1. stand-alone ----
@pytest.mark.parametrize("name", K.NAMES)
def test_standalone_equals_the_restatement(LP, name):
    c = K.case(name)
    got = LP.local_plan(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg, goal_state=c.goal_state, keys=True)
    _equal(LP, got, K.reference(name), name)
    again = LP.local_plan(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg, goal_state=c.goal_state, keys=True)      # the same bytes on every run
    assert again["keys"].tobytes() == got["keys"].tobytes() and again["traj"].tobytes() == got["traj"].tobytes()
    assert {k: v for k, v in again.items() if k not in ("keys", "traj")} == {k: v for k, v in got.items() if k not in ("keys", "traj")}
    quiet = LP.local_plan(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg, goal_state=c.goal_state)                 # no keys stored
    assert "keys" not in quiet
    _equal(LP, quiet, K.reference(name), (name, "no keys"), keys=False)


def test_standalone_batch_equals_its_grids_one_by_one(LP):
    got = LP.local_plan(K.BATCH, K.BATCH_POTS, K.BATCH_POSES, K.BATCH_WINDOWS, K.BATCH_NCFG, K.BATCH_CFG, keys=True)
    assert got["cmd_state"].dtype == np.int32 and got["cmd_state"].tolist() == [0, 1, 0] and got["keys"].shape == (3, 72)
    assert got["score"].dtype == np.uint64 and len(got["traj"]) == 3
    for b in range(3):
        one = LP.local_plan(K.BATCH[b], K.BATCH_POTS[b], K.BATCH_POSES[b], K.BATCH_WINDOWS[b], K.BATCH_NCFG, K.BATCH_CFG, keys=True)
        for g in (one, {k: v[b] for k, v in got.items()}):
            _equal(LP, g, K.batch_reference(b), b)


# ---- 2. behind the costmap stage and behind the occupancy maps ----
B = 2
CM = dict(x_min=-0.1, y_min=-0.7, resolution=0.05, width=37, height=29, z_min=-0.2, z_max=0.2)      # rows of 40 cells on the device
INFL = dict(resolution=0.05, inscribed_radius=0.05, inflation_radius=0.2, cost_scaling_factor=8.0)
NAV = dict(lethal_cost=100, allow_unknown=1, max_path=128)
LOC = dict(nv=6, nw=11, steps=8, lookahead=1024, pot_weight=8, occ_weight=4, speed_weight=1, turn_weight=1)
GOALS = np.array([[1.62, 0.31], [1.41, -0.52]])
ORG = (CM["x_min"], CM["y_min"])


def _tiny(pp, batch):
    return pp.config.tiny_config(batch)


def _frames(n, seed=300):
    out = []
    for b in range(n):
        rng = np.random.default_rng(seed + b)
        out.append(rng.uniform([0.05, -0.6, -2.5], [1.3, 0.6, 2.5], (700 + 150 * b, 3)).astype(np.float32))
    return out


def _same_run(LP, e, source, grids, pots, goal_state, poses, windows, ncfg, cfg, what, keys=True):
    """The engine's results of the source's last local_plan_async against best_np on the given grids and fields."""
    info = e.local_plan_info(source)
    traj = e.local_trajectories(source)
    kk = e.local_keys(source) if keys else None
    sv, sw, state = e.local_commands(source)
    assert np.array_equal(sv, info["sv"]) and np.array_equal(sw, info["sw"]) and np.array_equal(state, info["cmd_state"])
    for b in range(len(grids)):
        want = LP.best_np(grids[b], pots[b], poses[b], windows[b], ncfg, cfg, goal_state[b])
        got = {k: v[b] for k, v in info.items()}
        got["traj"] = traj[b]
        if keys:
            got["keys"] = kk[b]
        _equal(LP, got, want, (what, b), keys)
    return info, traj, kk


def test_costmap_source(pp, LP, hip_lib):
    plain_e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    try:
        frames = _frames(B)
        for x in (plain_e, e):
            x.set_costmap(CM)
            x.set_inflation(INFL, "costmap")
            x.set_navfn(NAV, "costmap")
            x.upload(frames)
        assert e.local_planner_config("costmap") is None
        e.set_local_planner(LOC, "costmap")
        cfg = e.local_planner_config("costmap")
        assert cfg == LP.LocalPlanConfig(**LOC) and e.local_planner_config("occupancy") is None
        paths0, states0 = plain_e.plan(GOALS)
        infl0, pots0 = plain_e._inflated(0, None, False)[0], plain_e.navfn_fields("costmap")
        # the sensor at yaw 0, the widest window
        e._plan_async(GOALS, "costmap", None)
        e.local_plan_async()
        infl, pots = e._inflated(0, None, False)[0], e.navfn_fields("costmap")
        gs = e.navfn_info("costmap")["goal_state"]
        poses = LP.pose_ticks(np.zeros((B, 2)), 0.0, ORG, CM["resolution"])
        assert (poses >> 10)[:, :2].tolist() == [[2, 13]] * B or (poses >> 10)[:, :2].tolist() == [[2, 14]] * B
        wide = np.tile(np.array([[0, 204, -512, 102]], np.int32), (B, 1))
        info, _, _ = _same_run(LP, e, "costmap", infl, pots, gs, poses, wide, NAV, cfg, "default")
        print("costmap source:", {k: v.tolist() for k, v in info.items()})
        assert (info["cmd_state"] == 0).all() and (info["n_ok"] >= 8).all() and (info["n_collision"] > 0).all()
        # the inflated grids, the fields and the paths are what they are without the stage
        paths, states = e.navfn_paths("costmap", metres=True)
        assert infl.tobytes() == infl0.tobytes() and pots.tobytes() == pots0.tobytes() and np.array_equal(states, states0)
        assert all(np.array_equal(a, b) for a, b in zip(paths, paths0))
        assert e.costmaps().tobytes() == plain_e.costmaps().tobytes()
        # given poses and windows
        P = np.array([[0.3, -0.2, 0.4], [0.2, 0.1, -0.7]])
        Wn = np.array([[100, 100, -300, 60], [-200, 150, -250, 50]], np.int32)
        e.local_plan_async(P, Wn)
        _same_run(LP, e, "costmap", infl, pots, gs, LP.pose_ticks(P[:, :2], P[:, 2], ORG, CM["resolution"]), Wn, NAV, cfg, "given")
        # drive: plan, then the dynamic window round the current velocity; the command in m/s and rad/s
        lim = LP.LocalLimits(v_min=-0.1, v_max=0.4, w_max=1.5, acc_v=1.0, acc_w=4.0, sim_time=1.0, period=0.2)
        V = np.array([[0.2, 0.0], [0.1, -0.3]])
        v, w, state = e.drive(GOALS, V, lim)
        win = np.array([lim.window(V[b, 0], V[b, 1], cfg.nv, cfg.nw, CM["resolution"]) for b in range(B)], np.int32)
        info, _, _ = _same_run(LP, e, "costmap", infl, pots, gs, poses, win, NAV, cfg, "drive", keys=False)
        mv, mw = LP.command_metric(info["sv"], info["sw"], CM["resolution"], lim.step_dt(CM["resolution"]))
        assert np.array_equal(v, mv) and np.array_equal(w, mw) and np.array_equal(state, info["cmd_state"]) and v.dtype == np.float64
        assert (v >= lim.v_min).all() and (v <= lim.v_max).all() and (np.abs(w) <= lim.w_max).all()
        assert e._inflated(0, None, False)[0].tobytes() == infl0.tobytes() and e.navfn_fields("costmap").tobytes() == pots0.tobytes()
        # off: the call is refused, the navigation function goes on
        e.set_local_planner(None, "costmap")
        assert e.local_planner_config("costmap") is None
        with pytest.raises(RuntimeError, match="local_plan_async: the local planner of the costmap source is not configured"):
            e.local_plan_async()
        assert e.plan(GOALS)[1].tolist() == states0.tolist()
    finally:
        plain_e.close()
        e.close()


S3 = 3
OCC = dict(resolution=0.1, z_min=0.0, z_max=1.0, max_range=2.5, width=37, height=29)       # rows of 40 cells on the device
OCC_INFL = dict(inscribed_radius=0.1, inflation_radius=0.5, cost_scaling_factor=4.0, lethal_threshold=65)
OCC_NAV = dict(allow_unknown=1, unknown_cost=20, max_path=256)
OCC_LOC = dict(nv=5, nw=13, steps=6, lookahead=512, pot_weight=16, occ_weight=8, speed_weight=2, turn_weight=1)


def _occ_frames(k):
    out = []
    for s in range(S3):
        rng = np.random.default_rng(40 + 10 * k + s)
        out.append(rng.uniform([-2.0, -1.6, -0.5], [2.0, 1.6, 1.2], (300 + 37 * s, 3)).astype(np.float32))
    return out


def test_occupancy_source(pp, LP, hip_lib):
    plain_e = pp.Engine(_tiny(pp, S3), max_batch=S3, max_points_per_frame=4096)
    e = pp.Engine(_tiny(pp, S3), max_batch=S3, max_points_per_frame=4096)
    try:
        for x in (plain_e, e):
            x.set_occupancy(OCC)
            x.set_inflation(OCC_INFL, "occupancy")
            x.set_navfn(OCC_NAV, "occupancy")
        e.set_local_planner(OCC_LOC, "occupancy")
        cfg = e.local_planner_config("occupancy")
        ncfg = e.navfn_config("occupancy")
        lim = LP.LocalLimits(v_min=0.0, v_max=0.6, w_max=1.2, acc_v=2.0, acc_w=6.0, sim_time=1.0, period=0.25)
        for k in range(2):                                                 # the window moves
            frames = _occ_frames(k)
            xy = np.array([[0.23 * k + 0.1 * s, -0.17 * k * (s - 1)] for s in range(S3)])
            yaw = np.array([0.3 * k + 0.5 * s for s in range(S3)])
            poses = np.stack([pp.sweeps.pose_from_xyyaw(xy[s, 0], xy[s, 1], yaw[s]) for s in range(S3)])
            for x in (plain_e, e):
                x.upload(frames)
                x.occupancy_update_async(poses)
            G = xy + np.array([[1.2, 0.6], [-1.1, 0.9], [9.0, 0.0]])       # the third lies outside its window
            paths0, states0 = plain_e.plan(G, "occupancy")
            V = np.array([[0.3, 0.1], [0.0, 0.0], [0.6, -1.0]])
            v, w, state = e.drive(G, V, lim, "occupancy")                  # the last update's poses
            infl, org = e._inflated(1, None, False)[0], e._occ_origins.copy()
            pots = e.navfn_fields("occupancy")
            gs = e.navfn_info("occupancy")["goal_state"]
            ticks = LP.pose_ticks(xy, yaw, org, OCC["resolution"])
            win = np.array([lim.window(V[s, 0], V[s, 1], cfg.nv, cfg.nw, OCC["resolution"]) for s in range(S3)], np.int32)
            info, _, _ = _same_run(LP, e, "occupancy", infl, pots, gs, ticks, win, ncfg, cfg, ("occupancy", k))
            print("occupancy source:", k, {key: val.tolist() for key, val in info.items()})
            mv, mw = LP.command_metric(info["sv"], info["sw"], OCC["resolution"], lim.step_dt(OCC["resolution"]))
            assert np.array_equal(v, mv) and np.array_equal(w, mw) and np.array_equal(state, info["cmd_state"])
            assert gs[2] == 2 and state[2] == 4 and (v[2], w[2]) == (0.0, 0.0)
            # the maps, the inflated grids, the fields and the paths are what they are without the stage
            infl0, org0 = plain_e._inflated(1, None, False)[0], plain_e._occ_origins
            assert infl.tobytes() == infl0.tobytes() and org.tobytes() == org0.tobytes(), k
            assert pots.tobytes() == plain_e.navfn_fields("occupancy").tobytes(), k
            paths, states = e.navfn_paths("occupancy", metres=True)
            assert np.array_equal(states, states0) and all(np.array_equal(a, b) for a, b in zip(paths, paths0)), k
            g3, g30 = e.occupancy_maps(logodds=True), plain_e.occupancy_maps(logodds=True)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(g3, g30)), k
        # a reset stream reads all unknown, whatever its grid holds: blocked with allow_unknown 0 -> the pose is blocked
        e.set_navfn(dict(OCC_NAV, allow_unknown=0), "occupancy")
        e.occupancy_reset(1)
        e.inflate_async("occupancy")
        sensor = np.array([[OCC["width"] // 2, OCC["height"] // 2]] * S3, np.int32)
        e._navfn_cells_async(1, sensor * 0 + [20, 10], sensor)
        e._local_cells_async(1, ticks, win)
        info = e.local_plan_info("occupancy")
        assert e.navfn_info("occupancy")["goal_state"][1] == 1 and info["cmd_state"][1] == 4
    finally:
        plain_e.close()
        e.close()


# ---- 3. a field that has not converged when the rollout is queued: the getter settles it and rolls again ----
def _serpentine_frame(period=4, gap=4):
    """One point per cell of the costmap: an obstacle point (z = 0) on every fourth row but for a gap that alternates
    between the right and the left end, a point above the obstacle band (z = 1: observed, free) elsewhere."""
    pts = []
    for iy in range(CM["height"]):
        for ix in range(CM["width"]):
            wall = iy % period == 2 and iy < CM["height"] - 1
            if wall and (ix >= CM["width"] - gap if (iy // period) % 2 == 0 else ix < gap):
                wall = False
            pts.append((CM["x_min"] + (ix + 0.5) * CM["resolution"], CM["y_min"] + (iy + 0.5) * CM["resolution"], 0.0 if wall else 1.0))
    return np.array(pts, np.float32)


def test_getter_rolls_again_behind_the_settled_field(pp, LP, hip_lib):
    N = pp.navfn
    e = pp.Engine(_tiny(pp, 1), max_batch=1, max_points_per_frame=4096)
    try:
        nav = dict(NAV, queued_rounds=1)
        e.set_costmap(CM)
        e.set_inflation(INFL, "costmap")
        e.set_navfn(nav, "costmap")
        e.set_local_planner(LOC, "costmap")
        cfg = e.local_planner_config("costmap")
        e.upload([_serpentine_frame()])
        res = CM["resolution"]
        goal = np.array([[CM["x_min"] + 1.5 * res, CM["y_min"] + 27.5 * res]])         # cell (1, 27): the far end
        pose = np.array([[CM["x_min"] + 2.5 * res, CM["y_min"] + 0.5 * res, 0.0]])      # cell (2, 0): the near end
        win = np.array([[100, 100, -300, 60]], np.int32)
        e._plan_async(goal, "costmap", None)
        e.local_plan_async(pose, win)                      # one round is queued in front of it: the field is nowhere near the pose
        sv, sw, state = e.local_commands("costmap")        # ... and the first thing fetched is the command
        infl = e._inflated(0, None, False)[0]
        assert (infl[0, 2::4][:-1].max(axis=1) == 100).all()       # the walls are there
        exact = N.navfn_np(infl[0], (1, 27), nav)
        ticks = LP.pose_ticks(pose[:, :2], pose[:, 2], ORG, res)
        assert (ticks[0, :2] >> 10).tolist() == [2, 0] and exact[0, 2] > 50000
        want = LP.best_np(infl[0], exact, ticks[0], win[0], nav, cfg)
        assert want["cmd_state"] == 0 and want["n_ok"] >= 8
        assert (int(sv[0]), int(sw[0]), int(state[0])) == (want["sv"], want["sw"], 0)
        ninfo = e.navfn_info("costmap")
        assert ninfo["rounds"][0] > 1 and np.array_equal(e.navfn_fields("costmap")[0], exact)
        _same_run(LP, e, "costmap", infl, exact[None], [0], ticks, win, nav, cfg, "settled")
    finally:
        e.close()


# ---- 3b. the inflated buffers are reused while the shape stands: a second inflation behind the call is refused, never read ----
REMADE = "the inflated grids of the costmap source were re-made since its navigation function ran"


def _blocked_corridor_frame():
    """The serpentine with wider gaps and two obstacle cells in the first corridor, five cells ahead of the pose (the row
    beside them stays open): another field and other collisions than on _serpentine_frame()."""
    pts = _serpentine_frame(gap=9)
    for iy in (0,):
        for ix in (7, 8):
            pts[iy * CM["width"] + ix, 2] = 0.0
    return pts


def test_a_second_inflation_behind_the_call_is_refused_not_read(pp, LP, hip_lib):
    """pp_inflate_async writes the next grids into the buffers the last ones lay in.  A getter that has to roll the samples
    again (here: one queued round, the field is not settled at the call) would roll them over the NEW grid against the
    OLD field; include/pp_hip.h promises PP_ERR_STATE instead, and likewise for a pp_local_plan_async without a new
    pp_navfn_async.  The navigation function copied its costs at the call: its own getters still give the old grid's field."""
    N = pp.navfn
    e = pp.Engine(_tiny(pp, 1), max_batch=1, max_points_per_frame=4096)
    try:
        nav = dict(NAV, queued_rounds=1)
        e.set_costmap(CM)
        e.set_inflation(INFL, "costmap")
        e.set_navfn(nav, "costmap")
        e.set_local_planner(LOC, "costmap")
        cfg = e.local_planner_config("costmap")
        res = CM["resolution"]
        goal = np.array([[CM["x_min"] + 1.5 * res, CM["y_min"] + 27.5 * res]])         # cell (1, 27): the far end
        pose = np.array([[CM["x_min"] + 2.5 * res, CM["y_min"] + 0.5 * res, 0.0]])      # cell (2, 0): the near end
        win = np.array([[100, 100, -300, 60]], np.int32)
        ticks = LP.pose_ticks(pose[:, :2], pose[:, 2], ORG, res)
        e.upload([_serpentine_frame()])
        e._plan_async(goal, "costmap", None)
        e.local_plan_async(pose, win)                      # 1. one round in front of it: a fetch has to settle and roll again
        old = e._inflated(0, None, False)[0].copy()        # (waits for the stream; settles nothing)
        e.upload([_blocked_corridor_frame()])              # 2. other obstacles, the same shape: the same buffers
        e.costmap_async()
        e.inflate_async("costmap")
        new = e._inflated(0, None, False)[0].copy()
        assert new.shape == old.shape and not np.array_equal(new, old)
        exact_old = N.navfn_np(old[0], (1, 27), nav)
        assert np.array_equal(e.navfn_fields("costmap")[0], exact_old)                 # 6. the field is the old grid's, to the last cell
        assert e.navfn_info("costmap")["rounds"][0] > 1
        for fetch in (e.local_commands, e.local_plan_info, e.local_trajectories, e.local_keys):
            with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_local_plan: " + REMADE):       # 3.
                fetch("costmap")
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_local_plan_async: " + REMADE + r" \(pp_navfn_async again\)"):
            e.local_plan_async(pose, win)                  # 4. the old field over the new grid: no
        assert np.array_equal(e.navfn_fields("costmap")[0], exact_old)                 # (the refusals changed nothing)
        e.navfn_async(goal, "costmap")                     # 5. again, in order: the new grid and its exact field
        e.local_plan_async(pose, win)
        exact = N.navfn_np(new[0], (1, 27), nav)
        assert not np.array_equal(exact, exact_old)
        want = LP.best_np(new[0], exact, ticks[0], win[0], nav, cfg)
        was = LP.best_np(old[0], exact_old, ticks[0], win[0], nav, cfg)
        stale = LP.best_np(new[0], exact_old, ticks[0], win[0], nav, cfg)              # what a getter that rolled again would have read
        assert want["cmd_state"] == 0 and want["n_ok"] >= 8
        assert len({(w["score"], w["n_ok"], w["n_collision"]) for w in (was, want, stale)}) == 3      # three answers that cannot pass for each other
        sv, sw, state = e.local_commands("costmap")
        assert (int(sv[0]), int(sw[0]), int(state[0])) == (want["sv"], want["sw"], 0)
        assert np.array_equal(e.navfn_fields("costmap")[0], exact)
        _same_run(LP, e, "costmap", new, exact[None], [0], ticks, win, nav, cfg, "on the new grid")
    finally:
        e.close()


# ---- 3c. the occupancy frame of a plan is the one its inflation read, whatever update has run since ----
def _sparse_frames(k):
    """A few obstacle points behind each sensor, 1.3 to 2 m away (tests/test_gpu_local_movers.py): the way ahead stays
    unknown, which OCC_NAV allows, so every goal and pose below is free."""
    out = []
    for s in range(S3):
        rng = np.random.default_rng(40 + 10 * k + s)
        r, a = rng.uniform(1.3, 2.0, 12 + 5 * s), rng.uniform(2.0, 4.3, 12 + 5 * s)
        out.append(np.stack([r * np.cos(a), r * np.sin(a), np.full(len(r), 0.5)], axis=1).astype(np.float32))
    return out


def test_the_occupancy_frame_is_the_inflations_not_the_last_updates(pp, LP, hip_lib):
    """update, inflate, update under a pose two and three cells on: navfn_async's goals in metres, local_plan_async's
    default poses and navfn_paths(metres=True) belong to the grid that was inflated -- the first update's window and pose."""
    N = pp.navfn
    e = pp.Engine(_tiny(pp, S3), max_batch=S3, max_points_per_frame=4096)
    try:
        e.set_occupancy(OCC)
        e.set_inflation(OCC_INFL, "occupancy")
        e.set_navfn(OCC_NAV, "occupancy")
        e.set_local_planner(OCC_LOC, "occupancy")
        cfg, ncfg, res = e.local_planner_config("occupancy"), e.navfn_config("occupancy"), OCC["resolution"]
        shape = (OCC["height"], OCC["width"])
        xy0 = np.array([[0.02 + 0.1 * s, -0.03] for s in range(S3)])
        yaw0 = np.array([0.2 + 0.5 * s for s in range(S3)])
        xy1, yaw1 = xy0 + [0.3, -0.2], yaw0 + 0.7
        e.upload(_sparse_frames(0))
        e.occupancy_update_async(np.stack([pp.sweeps.pose_from_xyyaw(xy0[s, 0], xy0[s, 1], yaw0[s]) for s in range(S3)]))
        e.inflate_async("occupancy")
        org0 = e.occupancy_maps()[1]
        e.upload(_sparse_frames(1))
        e.occupancy_update_async(np.stack([pp.sweeps.pose_from_xyyaw(xy1[s, 0], xy1[s, 1], yaw1[s]) for s in range(S3)]))
        org1 = e.occupancy_maps()[1]
        assert np.array_equal(np.rint((org1 - org0) / res), np.tile([[3.0, -2.0]], (S3, 1)))      # the window moved by whole cells
        G = xy0 + np.array([[1.2, 0.6], [-1.1, 0.9], [0.8, 0.3]])
        e.navfn_async(G, "occupancy")
        e.local_plan_async(source="occupancy")
        infl = e._inflated(1, None, False)[0]              # the first update's maps, inflated
        goals, moved = N.goal_cells(G, org0, res, shape), N.goal_cells(G, org1, res, shape)
        ticks, ticks1 = LP.pose_ticks(xy0, yaw0, org0, res), LP.pose_ticks(xy1, yaw1, org1, res)
        assert not (goals == moved).all(axis=1).any() and not (ticks == ticks1).all(axis=1).any()
        pots, info = e.navfn_fields("occupancy"), e.navfn_info("occupancy")
        paths, states = e.navfn_paths("occupancy")
        mpaths, _ = e.navfn_paths("occupancy", metres=True)
        assert (info["goal_state"] == 0).all() and (states == 0).all()
        for s in range(S3):
            assert np.array_equal(pots[s], N.navfn_np(infl[s], goals[s], ncfg)), s
            assert np.argwhere(pots[s] == 0)[:, ::-1].tolist() == [goals[s].tolist()], s           # the goal cell is the first window's
            assert paths[s][0].tolist() == [OCC["width"] // 2, OCC["height"] // 2] and paths[s][-1].tolist() == goals[s].tolist(), s
            assert np.array_equal(mpaths[s], N.path_to_metres(paths[s], org0[s], res)), s
        wide = np.tile(np.array([[0, LP.MAX_SV // (cfg.nv - 1), -LP.MAX_SW, 2 * LP.MAX_SW // (cfg.nw - 1)]], np.int32), (S3, 1))
        info, traj, _ = _same_run(LP, e, "occupancy", infl, pots, [0] * S3, ticks, wide, ncfg, cfg, "the first update's frame")
        assert (info["cmd_state"] == 0).all()
        for s in range(S3):
            assert traj[s][0].tolist() == ticks[s].tolist(), s                          # the pose ticks are the first update's
        # the next inflation takes the second update's frame
        _, org = e.inflated_occupancy_maps()
        assert org.tobytes() == org1.tobytes()
        e.navfn_async(G, "occupancy")
        pots = e.navfn_fields("occupancy")
        assert [np.argwhere(pots[s] == 0)[:, ::-1].tolist() for s in range(S3)] == [[g] for g in moved.tolist()]
    finally:
        e.close()


# ---- 4. the call ring: more calls than slots, with and without a fetch between them; the refusals ----
def test_ring_reuse_and_refusals(pp, LP, hip_lib):
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    try:
        L, h = e._lib, e._h
        state = "PP_ERR_STATE.*pp_local_plan_async: "
        trig = np.ascontiguousarray(LP.trig_table())
        pc = pp._lib.PPLocalPlanConfig(**LOC)
        three, four = np.zeros((B, 3), np.int32), np.zeros((B, 4), np.int32)

        def call_async(source=0, poses=three, windows=four, batch=B):
            e._check(L.pp_local_plan_async(h, source, None if poses is None else poses.ctypes.data,
                                           None if windows is None else windows.ctypes.data, batch), "pp_local_plan_async")

        e.set_costmap(CM)
        e.set_inflation(INFL, "costmap")
        # the stage off; the navigation function off; no navigation function run; nothing to fetch
        with pytest.raises(RuntimeError, match=state + "the local planner of the costmap source is not configured"):
            call_async()
        # a bad trig table: its length, a value
        for n_trig, msg in ((4095, "the trig table has 4095 entries"), (0, "the trig table has 0 entries")):
            with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_set_local_plan: " + msg):
                e._check(L.pp_set_local_plan(h, 0, ctypes.byref(pc), trig.ctypes.data, n_trig), "pp_set_local_plan")
        bad = trig.copy()
        bad[4095, 0] = -16385
        with pytest.raises(RuntimeError, match=r"PP_ERR_ARG.*pp_set_local_plan: trig\[4095\] = \(-16385, -25\) outside \[-16384, 16384\]"):
            e._check(L.pp_set_local_plan(h, 0, ctypes.byref(pc), bad.ctypes.data, 4096), "pp_set_local_plan")
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_set_local_plan: trig is NULL"):
            e._check(L.pp_set_local_plan(h, 0, ctypes.byref(pc), None, 4096), "pp_set_local_plan")
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_set_local_plan: source = 2"):
            e._check(L.pp_set_local_plan(h, 2, ctypes.byref(pc), trig.ctypes.data, 4096), "pp_set_local_plan")
        assert e.local_planner_config("costmap") is None
        e.set_local_planner(LOC, "costmap")
        with pytest.raises(RuntimeError, match=state + "the navigation function of the costmap source is not configured"):
            call_async()
        e.set_navfn(NAV, "costmap")
        with pytest.raises(RuntimeError, match=state + "no navigation function has run on this source"):
            call_async()
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_local_plan: no local plan has run on this source"):
            e._check(L.pp_get_local_plan(h, 0, None, None, None, None, B), "pp_get_local_plan")
        e.upload(_frames(B))
        e._plan_async(GOALS, "costmap", None)
        infl, pots = e._inflated(0, None, False)[0], e.navfn_fields("costmap")
        gs = e.navfn_info("costmap")["goal_state"]
        cfg = e.local_planner_config("costmap")
        n_calls = 2 * OFF_RING + 1
        poses = [LP.pose_ticks([[0.1 + 0.05 * i, -0.3 + 0.06 * i], [0.4 - 0.03 * i, 0.35 - 0.05 * i]], [0.2 * i, -0.3 * i], ORG, CM["resolution"])
                 for i in range(n_calls)]
        wins = [np.array([[40 * i, 40 + 10 * i, -300 + 20 * i, 40], [-100 + 20 * i, 100, -40 * i, 30 + 5 * i]], np.int32) for i in range(n_calls)]
        for i in range(OFF_RING + 1):                                      # no fetch: slot 0 comes round again
            e._local_cells_async(0, poses[i], wins[i])
        _same_run(LP, e, "costmap", infl, pots, gs, poses[OFF_RING], wins[OFF_RING], NAV, cfg, "unfetched")
        for i in range(OFF_RING + 1, n_calls):
            e._local_cells_async(0, poses[i], wins[i])
            last = _same_run(LP, e, "costmap", infl, pots, gs, poses[i], wins[i], NAV, cfg, ("fetched", i))

        def unchanged():
            info = e.local_plan_info("costmap")
            assert all(np.array_equal(info[k], v) for k, v in last[0].items())
            assert all(np.array_equal(a, b) for a, b in zip(e.local_trajectories("costmap"), last[1]))
            assert e.local_keys("costmap").tobytes() == last[2].tobytes()

        # refusals leave the last results as they were, and the next call finds its slot
        arg = "PP_ERR_ARG.*pp_local_plan_async: "
        with pytest.raises(RuntimeError, match=arg + "the last navigation function had 2 grids, batch is 1"):
            call_async(batch=1)
        with pytest.raises(RuntimeError, match=arg + "poses or windows is NULL"):
            call_async(poses=None)
        with pytest.raises(RuntimeError, match=arg + "poses or windows is NULL"):
            call_async(windows=None)
        with pytest.raises(RuntimeError, match=arg + "source = 2"):
            call_async(source=2)
        with pytest.raises(RuntimeError, match=arg + r"windows: grid 1: sv runs from 1000 to 1025, outside \[-1024, 1024\]"):
            call_async(windows=np.array([[0, 0, 0, 0], [1000, 5, 0, 0]], np.int32))
        with pytest.raises(RuntimeError, match=arg + r"windows: grid 0: sw runs from -513 to -513, outside \[-512, 512\]"):
            call_async(windows=np.array([[0, 0, -513, 0], [0, 0, 0, 0]], np.int32))
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_get_local_plan: the last run had 2 grids, batch is 1"):
            e._check(L.pp_get_local_plan(h, 0, None, None, None, None, 1), "pp_get_local_plan")
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_get_local_plan: source = -1"):
            e._check(L.pp_get_local_plan(h, -1, None, None, None, None, B), "pp_get_local_plan")
        with pytest.raises(RuntimeError, match=state + "the local planner of the occupancy source is not configured"):
            call_async(source=1)
        unchanged()
        e.set_navfn(None, "costmap")
        with pytest.raises(RuntimeError, match=state + "the navigation function of the costmap source is not configured"):
            e._local_cells_async(0, poses[0], wins[0])
        e.set_navfn(NAV, "costmap")
        e.set_local_planner(None, "costmap")
        with pytest.raises(RuntimeError, match=state + "the local planner of the costmap source is not configured"):
            e._local_cells_async(0, poses[0], wins[0])
        e.set_local_planner(LOC, "costmap")
        unchanged()
        # a pp_navfn_async after the pp_local_plan_async whose result is asked for: the command would rest on another field
        e.navfn_async(GOALS[::-1].copy())
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_local_plan: a pp_navfn_async of the costmap source came after"):
            e.local_plan_info("costmap")
        pots2 = e.navfn_fields("costmap")
        assert not np.array_equal(pots2, pots)
        e._local_cells_async(0, poses[1], wins[1])
        _same_run(LP, e, "costmap", infl, pots2, e.navfn_info("costmap")["goal_state"], poses[1], wins[1], NAV, cfg, "after the refusals")
    finally:
        e.close()
