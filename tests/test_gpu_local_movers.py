"""The local planner's movers on the GPU (csrc/local_plan.hip: the MOVERS instantiations of k_local_rollout and
k_local_finish; csrc/local_movers.hip: k_local_movers) against local_planner.py's restatement: result words, info words,
scores, trajectories, all keys and the movers' tables must be EQUAL (np.array_equal), no tolerances.  Stand-alone on the
shared cases (tests/local_mover_cases.py); then behind the costmap and the occupancy maps with the tables made from the
tracker's slots, against `movers_np` of `tracks()` / `tracks_fixed()`; the getter's second rollout on the table the call
built; the call ring; every refusal; and with the movers off the bytes of an engine that never heard of them."""
import ctypes

import numpy as np
import pytest

import local_mover_cases as M
import local_plan_cases as K

pytestmark = pytest.mark.gpu

OFF_RING = 4            # csrc/pp_ring.h


@pytest.fixture(scope="module")
def LP(pp, hip_lib):
    return pp.local_planner


def _equal(LP, got, want, what, keys=True):
    """`got` of local_plan / the engine for one grid against best_np's dict (with movers)."""
    for k in LP.RESULT + ("n_movers", "n_dynamic", "near"):
        assert int(got[k]) == want[k], (what, k, int(got[k]), want[k])
    assert int(got["score"]) == want["score"], what
    assert got["traj"].dtype == np.int32 and np.array_equal(got["traj"], want["traj"]), what
    if keys:
        assert got["keys"].dtype == np.uint64 and np.array_equal(got["keys"], want["keys"]), what


# ---- 1. stand-alone ----
@pytest.mark.parametrize("name", M.NAMES)
def test_standalone_equals_the_restatement(LP, name):
    c, b = M.case(name), M.case(name).base
    got = LP.local_plan(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, goal_state=b.goal_state, keys=True, movers=c.movers, mover_cfg=c.mcfg)
    _equal(LP, got, M.reference(name), name)
    assert got["n_skipped"] == 0
    quiet = LP.local_plan(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, goal_state=b.goal_state, movers=c.movers, mover_cfg=c.mcfg)    # no keys stored
    assert "keys" not in quiet
    _equal(LP, quiet, M.reference(name), (name, "no keys"), keys=False)


@pytest.mark.parametrize("name", ["a_none", "a_extreme_none", "horizon_0", "cull_beyond", "a_too_late"])
def test_movers_that_touch_nothing_give_the_stage_off_bytes(LP, name):
    c, b = M.case(name), M.case(name).base
    off = LP.local_plan(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, goal_state=b.goal_state, keys=True)
    on = LP.local_plan(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, goal_state=b.goal_state, keys=True, movers=c.movers, mover_cfg=c.mcfg)
    assert on["keys"].tobytes() == off["keys"].tobytes() and on["traj"].tobytes() == off["traj"].tobytes()
    assert all(on[k] == off[k] for k in LP.RESULT + ("score",)) and (on["n_dynamic"], on["near"]) == (0, 0)
    assert set(off) == set(LP.RESULT) | {"score", "traj", "keys"}


@pytest.mark.parametrize("name", ["samples_63", "samples_257", "pitch_37", "wall_ahead", "largest_weights", "goal_blocked"])
def test_an_empty_table_gives_the_stage_off_bytes(LP, name):
    c = K.case(name)
    off = LP.local_plan(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg, goal_state=c.goal_state, keys=True)
    on = LP.local_plan(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg, goal_state=c.goal_state, keys=True, movers=[], mover_cfg=True)
    assert on["keys"].tobytes() == off["keys"].tobytes() and on["traj"].tobytes() == off["traj"].tobytes()
    assert all(on[k] == off[k] for k in LP.RESULT + ("score",)) and (on["n_movers"], on["n_dynamic"], on["near"]) == (0, 0, 0)


def test_standalone_batch_equals_its_grids_one_by_one(LP):
    got = LP.local_plan(K.BATCH, K.BATCH_POTS, K.BATCH_POSES, K.BATCH_WINDOWS, K.BATCH_NCFG, K.BATCH_CFG, keys=True,
                        movers=M.BATCH_MOVERS, n_movers=M.BATCH_N, mover_cfg=M.BATCH_MCFG)
    assert got["n_movers"].dtype == np.int32 and got["n_movers"].tolist() == [5, 0, 64] and got["cmd_state"].tolist() == [0, 1, 0]
    for b in range(3):
        one = LP.local_plan(K.BATCH[b], K.BATCH_POTS[b], K.BATCH_POSES[b], K.BATCH_WINDOWS[b], K.BATCH_NCFG, K.BATCH_CFG, keys=True,
                            movers=M.BATCH_MOVERS[b, :M.BATCH_N[b]], mover_cfg=M.BATCH_MCFG)
        for g in (one, {k: v[b] for k, v in got.items()}):
            _equal(LP, g, M.batch_reference(b), b)


# ---- 2. behind the costmap stage: the tables from the tracker's slots in the sensor frame ----
B = 2
CM = dict(x_min=-0.1, y_min=-0.7, resolution=0.05, width=37, height=29, z_min=-0.2, z_max=0.2)      # rows of 40 cells on the device
INFL = dict(resolution=0.05, inscribed_radius=0.05, inflation_radius=0.2, cost_scaling_factor=8.0)
NAV = dict(lethal_cost=100, allow_unknown=1, max_path=128)
LOC = dict(nv=6, nw=11, steps=8, lookahead=1024, pot_weight=8, occ_weight=4, speed_weight=1, turn_weight=1)
MOV = dict(horizon=8, mover_weight=300, pad_hard=0.03, pad_soft=0.12, confirmed_only=True)
TRK = dict(max_misses=1, min_hits=2, gate=0.6)
GOALS = np.array([[1.62, 0.31], [1.41, -0.52]])
ORG = (CM["x_min"], CM["y_min"])
RES = CM["resolution"]
DT = 0.125              # seconds per rollout step


def _tiny(pp, batch):
    return pp.config.tiny_config(batch)


def _frames(n, seed=300):
    out = []
    for b in range(n):
        rng = np.random.default_rng(seed + b)
        out.append(rng.uniform([0.05, -0.6, -2.5], [1.3, 0.6, 2.5], (700 + 150 * b, 3)).astype(np.float32))
    return out


def _dets(pp, people):
    """people[stream] = [(x, y, w, l)] -> (dets [streams, 8] DET_DTYPE, n_dets)."""
    d = np.zeros((len(people), 8), pp.engine.DET_DTYPE)
    for s, rows in enumerate(people):
        for i, (x, y, w, l) in enumerate(rows):
            d["box3d_lidar"][s, i] = (x, y, 0.1, w, l, 1.7, 0.0)
            d["score"][s, i] = 0.9
    return d, np.array([len(r) for r in people], np.int32)


def _walk(pp, e, steps, poses=None, first=0):
    """Feeds the tracker `steps` steps of 0.1 s.  Stream 0: a walker crosses in front of the robot (slot 0); two people are
    seen once only (slots 1 and 2, which fall free); one stands (slot 3); one appears at the last step, takes slot 1 and
    stays unconfirmed -- slot 2 lies free between live ones.  Stream 1: a walker who comes towards the robot, and a runner at 2.5 m/s, too fast
    for a step of half a second.  Further streams: one walker each."""
    for k in range(first, first + steps):
        once = [(0.9, -0.4, 0.2, 0.2), (1.3, -0.5, 0.2, 0.2)] if k == first else []
        s0 = [(0.3, 0.30 - 0.04 * k, 0.12, 0.16)] + once + [(0.8, 0.05, 0.1, 0.1)]
        if k == first + steps - 1:
            s0.append((0.3, 0.4, 0.1, 0.1))
        s1 = [(0.45 - 0.03 * (k - first), -0.04, 0.1, 0.14), (1.2, -0.6 + 0.25 * (k - first), 0.1, 0.1)]
        people = [s0, s1] + [[(0.4, 0.1 * k, 0.1, 0.1)]] * (e.max_batch - 2)
        d, n = _dets(pp, people[:e.max_batch])
        e.track_update(d, n, np.full(e.max_batch, 0.1), poses)


def _same_run(LP, e, source, grids, pots, goal_state, poses, windows, ncfg, cfg, tables, mcfg, what, keys=True):
    """The engine's results of the source's last local_plan_async with movers against best_np on the given grids, fields
    and tables [(movers [64, 6], n_movers, n_skipped)]."""
    info = e.local_plan_info(source)
    traj = e.local_trajectories(source)
    kk = e.local_keys(source) if keys else None
    got_m, minfo = e.local_movers(source)
    assert got_m.dtype == np.int32 and got_m.shape == (len(grids), 64, 6)
    for b in range(len(grids)):
        m, n, skipped = tables[b]
        assert np.array_equal(got_m[b], m) and (minfo["n_movers"][b], minfo["n_skipped"][b]) == (n, skipped), (what, b, minfo)
        want = LP.best_np(grids[b], pots[b], poses[b], windows[b], ncfg, cfg, goal_state[b], movers=m[:max(n, 0)], mcfg=mcfg)
        want["n_movers"] = n
        got = {k: v[b] for k, v in info.items()}
        got["traj"] = traj[b]
        if keys:
            got["keys"] = kk[b]
        _equal(LP, got, want, (what, b), keys)
        assert (minfo["n_dynamic"][b], minfo["near"][b]) == (want["n_dynamic"], want["near"])
    return info, traj, kk, got_m


def test_costmap_source(pp, LP, hip_lib):
    plain_e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    try:
        frames = _frames(B)
        for x in (plain_e, e):
            x.set_costmap(CM)
            x.set_inflation(INFL, "costmap")
            x.set_navfn(NAV, "costmap")
            x.set_local_planner(LOC, "costmap")
            x.upload(frames)
        assert e.local_movers_config("costmap") is None
        e.set_local_movers(MOV, "costmap")
        mcfg = e.local_movers_config("costmap")
        assert mcfg == LP.MoverConfig(**MOV) and e.local_movers_config("occupancy") is None
        cfg = e.local_planner_config("costmap")
        e.set_tracking(TRK)
        _walk(pp, e, 4)
        tr, n, _ = e.tracks(B)
        assert n.tolist() == [3, 2] and tr["confirmed"][0, :3].tolist() == [1, 0, 1]
        tables = [LP.movers_np(tr[b], n[b], ORG, RES, DT, mcfg) for b in range(B)]
        assert [t[1:] for t in tables] == [(2, 0), (2, 0)]                     # the unconfirmed row is left out
        assert e.track_info()["live"].tolist() == [3, 2] and e.track_info()["next_id"][0] == 6        # five were born, two died
        plain_e._plan_async(GOALS, "costmap", None)
        plain_e.local_plan_async(dt=DT)
        off = (plain_e.local_plan_info("costmap"), plain_e.local_trajectories("costmap"), plain_e.local_keys("costmap"))
        infl0, pots0 = plain_e._inflated(0, None, False)[0], plain_e.navfn_fields("costmap")
        paths0, states0 = plain_e.navfn_paths("costmap", metres=True)
        # the sensor at yaw 0, the widest window
        e._plan_async(GOALS, "costmap", None)
        with pytest.raises(ValueError, match="local_plan_async: dt is None"):
            e.local_plan_async()
        e.local_plan_async(dt=DT)
        infl, pots = e._inflated(0, None, False)[0], e.navfn_fields("costmap")
        gs = e.navfn_info("costmap")["goal_state"]
        poses = LP.pose_ticks(np.zeros((B, 2)), 0.0, ORG, RES)
        wide = np.tile(np.array([[0, 204, -512, 102]], np.int32), (B, 1))
        info, _, kk, _ = _same_run(LP, e, "costmap", infl, pots, gs, poses, wide, NAV, cfg, tables, mcfg, "default")
        print("costmap source:", {k: v.tolist() for k, v in info.items()})
        assert (info["cmd_state"] == 0).all() and (info["n_dynamic"] > 0).all() and (info["n_ok"] > 0).all() and set(info) == set(off[0]) | set(LP.MOVER_INFO)
        assert not np.array_equal(kk, off[2])
        # the inflated grids, the fields and the paths are what they are without the stage
        paths, states = e.navfn_paths("costmap", metres=True)
        assert infl.tobytes() == infl0.tobytes() and pots.tobytes() == pots0.tobytes() and np.array_equal(states, states0)
        assert all(np.array_equal(a, b) for a, b in zip(paths, paths0))
        assert e.costmaps().tobytes() == plain_e.costmaps().tobytes()
        # every track, confirmed or not
        e.set_local_movers(dict(MOV, confirmed_only=False, horizon=3), "costmap")
        mcfg2 = e.local_movers_config("costmap")
        P = np.array([[0.3, -0.2, 0.4], [0.2, 0.1, -0.7]])
        Wn = np.array([[100, 100, -300, 60], [-200, 150, -250, 50]], np.int32)
        e.local_plan_async(P, Wn, dt=0.5)
        tables2 = [LP.movers_np(tr[b], n[b], ORG, RES, 0.5, mcfg2) for b in range(B)]
        assert [t[1:] for t in tables2] == [(3, 0), (1, 1)]                    # ... and the runner is too fast for half a second
        _same_run(LP, e, "costmap", infl, pots, gs, LP.pose_ticks(P[:, :2], P[:, 2], ORG, RES), Wn, NAV, cfg, tables2, mcfg2, "given")
        # drive passes its step's seconds
        e.set_local_movers(MOV, "costmap")
        lim = LP.LocalLimits(v_min=-0.1, v_max=0.4, w_max=1.5, acc_v=1.0, acc_w=4.0, sim_time=1.0, period=0.2)
        V = np.array([[0.2, 0.0], [0.1, -0.3]])
        v, w, state = e.drive(GOALS, V, lim)
        win = np.array([lim.window(V[b, 0], V[b, 1], cfg.nv, cfg.nw, RES) for b in range(B)], np.int32)
        tables3 = [LP.movers_np(tr[b], n[b], ORG, RES, lim.step_dt(RES), mcfg) for b in range(B)]
        info, _, _, _ = _same_run(LP, e, "costmap", infl, pots, gs, poses, win, NAV, cfg, tables3, mcfg, "drive", keys=False)
        mv, mw = LP.command_metric(info["sv"], info["sw"], RES, lim.step_dt(RES))
        assert np.array_equal(v, mv) and np.array_equal(w, mw) and np.array_equal(state, info["cmd_state"])
        # off: the bytes of the engine that never heard of the movers, and no table to fetch
        e.set_local_movers(None, "costmap")
        assert e.local_movers_config("costmap") is None
        e._plan_async(GOALS, "costmap", None)
        e.local_plan_async(dt=DT)
        now = (e.local_plan_info("costmap"), e.local_trajectories("costmap"), e.local_keys("costmap"))
        assert set(now[0]) == set(off[0]) and all(now[0][k].tobytes() == off[0][k].tobytes() for k in off[0])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(now[1], off[1])) and now[2].tobytes() == off[2].tobytes()
        with pytest.raises(RuntimeError, match="local_movers: the last local plan of the costmap source had no movers"):
            e.local_movers("costmap")
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_local_movers: the last run of the costmap source was a pp_local_plan_async"):
            e._check(e._lib.pp_get_local_movers(e._h, 0, None, None, B), "pp_get_local_movers")
    finally:
        plain_e.close()
        e.close()


# ---- 3. behind the occupancy maps: the slots carried into the fixed frame; a stream without a posed step ----
S3 = 3
OCC = dict(resolution=0.1, z_min=0.0, z_max=1.0, max_range=2.5, width=37, height=29)       # rows of 40 cells on the device
OCC_INFL = dict(inscribed_radius=0.1, inflation_radius=0.5, cost_scaling_factor=4.0, lethal_threshold=65)
OCC_NAV = dict(allow_unknown=1, unknown_cost=20, max_path=256)
OCC_LOC = dict(nv=5, nw=13, steps=6, lookahead=512, pot_weight=16, occ_weight=8, speed_weight=2, turn_weight=1)
OCC_MOV = dict(horizon=6, mover_weight=100, pad_hard=0.1, pad_soft=0.3, confirmed_only=False)


def _occ_frames(k):
    """A few obstacle points behind each sensor, 1.3 to 2 m away: the way ahead stays unknown, which OCC_NAV allows."""
    out = []
    for s in range(S3):
        rng = np.random.default_rng(40 + 10 * k + s)
        r, a = rng.uniform(1.3, 2.0, 12 + 5 * s), rng.uniform(2.0, 4.3, 12 + 5 * s)
        out.append(np.stack([r * np.cos(a), r * np.sin(a), np.full(len(r), 0.5)], axis=1).astype(np.float32))
    return out


def test_occupancy_source(pp, LP, hip_lib):
    plain_e = pp.Engine(_tiny(pp, S3), max_batch=S3, max_points_per_frame=4096)
    e = pp.Engine(_tiny(pp, S3), max_batch=S3, max_points_per_frame=4096)
    try:
        for x in (plain_e, e):
            x.set_occupancy(OCC)
            x.set_inflation(OCC_INFL, "occupancy")
            x.set_navfn(OCC_NAV, "occupancy")
            x.set_local_planner(OCC_LOC, "occupancy")
        e.set_local_movers(OCC_MOV, "occupancy")
        e.set_tracking(TRK)
        cfg, mcfg, ncfg = e.local_planner_config("occupancy"), e.local_movers_config("occupancy"), e.navfn_config("occupancy")
        lim = LP.LocalLimits(v_min=0.0, v_max=0.6, w_max=1.2, acc_v=2.0, acc_w=6.0, sim_time=1.0, period=0.25)
        dt = lim.step_dt(OCC["resolution"])
        for k in range(2):                                                 # the window moves, and the tracks with it
            frames = _occ_frames(k)
            xy = np.array([[0.23 * k + 0.1 * s, -0.17 * k * (s - 1)] for s in range(S3)])
            yaw = np.array([0.3 * k + 0.5 * s for s in range(S3)])
            poses = np.stack([pp.sweeps.pose_from_xyyaw(xy[s, 0], xy[s, 1], yaw[s]) for s in range(S3)])
            for x in (plain_e, e):
                x.upload(frames)
                x.occupancy_update_async(poses)
            _walk(pp, e, 3, poses[:2], first=3 * k)                        # streams 0 and 1 posed, stream 2 never
            tr, n = e.tracks_fixed(S3)
            assert n[2] == -1 and (n[:2] > 0).all()
            G = xy + np.array([[1.2, 0.6], [0.9, -0.8], [0.8, 0.3]])
            V = np.array([[0.3, 0.1], [0.0, 0.0], [0.6, -1.0]])
            plain_e.drive(G, V, lim, "occupancy")
            v, w, state = e.drive(G, V, lim, "occupancy")                  # the last update's poses
            infl, org = e._inflated(1, None, False)[0], e._occ_origins.copy()
            pots = e.navfn_fields("occupancy")
            gs = e.navfn_info("occupancy")["goal_state"]
            ticks = LP.pose_ticks(xy, yaw, org, OCC["resolution"])
            win = np.array([lim.window(V[s, 0], V[s, 1], cfg.nv, cfg.nw, OCC["resolution"]) for s in range(S3)], np.int32)
            tables = [LP.movers_np(tr[s], n[s], org[s], OCC["resolution"], dt, mcfg) for s in range(S3)]
            assert tables[2][1:] == (-1, 0) and tables[0][1] >= 2
            info, traj, kk, _ = _same_run(LP, e, "occupancy", infl, pots, gs, ticks, win, ncfg, cfg, tables, mcfg, ("occupancy", k))
            print("occupancy source:", k, {key: val.tolist() for key, val in info.items()})
            assert info["n_movers"].tolist() == [t[1] for t in tables] and (info["n_dynamic"][:2] + info["near"][:2]).sum() > 0
            assert k == 1 or (info["n_dynamic"][:2] > 0).all()
            assert (info["cmd_state"] <= 1).all() and info["cmd_state"][0] == 0 and info["cmd_state"][2] == 0       # (1: it stops for a walker it cannot pass)
            mv, mw = LP.command_metric(info["sv"], info["sw"], OCC["resolution"], dt)
            assert np.array_equal(v, mv) and np.array_equal(w, mw) and np.array_equal(state, info["cmd_state"])
            # the unposed stream is rolled with no movers: the bytes of the engine without them
            assert kk[2].tobytes() == plain_e.local_keys("occupancy")[2].tobytes() and info["n_dynamic"][2] == 0
            assert traj[2].tobytes() == plain_e.local_trajectories("occupancy")[2].tobytes()
            # the maps, the inflated grids, the fields and the paths are what they are without the stage
            assert infl.tobytes() == plain_e._inflated(1, None, False)[0].tobytes() and org.tobytes() == plain_e._occ_origins.tobytes(), k
            assert pots.tobytes() == plain_e.navfn_fields("occupancy").tobytes(), k
            paths, states = e.navfn_paths("occupancy", metres=True)
            paths0, states0 = plain_e.navfn_paths("occupancy", metres=True)
            assert np.array_equal(states, states0) and all(np.array_equal(a, b) for a, b in zip(paths, paths0)), k
            g3, g30 = e.occupancy_maps(logodds=True), plain_e.occupancy_maps(logodds=True)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(g3, g30)), k
    finally:
        plain_e.close()
        e.close()


# ---- 4. a field that has not converged when the rollout is queued: the getter rolls again, on the table the call built ----
def _serpentine_frame(period=4, gap=4):
    """One point per cell of the costmap: an obstacle point (z = 0) on every fourth row but for a gap that alternates
    between the right and the left end, a point above the obstacle band (z = 1: observed, free) elsewhere."""
    pts = []
    for iy in range(CM["height"]):
        for ix in range(CM["width"]):
            wall = iy % period == 2 and iy < CM["height"] - 1
            if wall and (ix >= CM["width"] - gap if (iy // period) % 2 == 0 else ix < gap):
                wall = False
            pts.append((CM["x_min"] + (ix + 0.5) * RES, CM["y_min"] + (iy + 0.5) * RES, 0.0 if wall else 1.0))
    return np.array(pts, np.float32)


def test_getter_rolls_again_on_the_table_the_call_built(pp, LP, hip_lib):
    N = pp.navfn
    e = pp.Engine(_tiny(pp, 1), max_batch=1, max_points_per_frame=4096)
    try:
        nav = dict(NAV, queued_rounds=1)
        e.set_costmap(CM)
        e.set_inflation(INFL, "costmap")
        e.set_navfn(nav, "costmap")
        e.set_local_planner(LOC, "costmap")
        e.set_local_movers(dict(MOV, confirmed_only=False), "costmap")
        e.set_tracking(TRK)
        cfg, mcfg = e.local_planner_config("costmap"), e.local_movers_config("costmap")
        e.upload([_serpentine_frame()])
        goal = np.array([[CM["x_min"] + 1.5 * RES, CM["y_min"] + 27.5 * RES]])         # cell (1, 27): the far end
        pose = np.array([[CM["x_min"] + 2.5 * RES, CM["y_min"] + 0.5 * RES, 0.0]])      # cell (2, 0): the near end
        win = np.array([[100, 100, -300, 60]], np.int32)
        person = (CM["x_min"] + 7.5 * RES, CM["y_min"] + 0.5 * RES, 0.1, 0.1)           # stands in the corridor, five cells ahead
        for _ in range(2):
            tr, n, _ = e.track_update(*_dets(pp, [[person]]), [0.1])
        table = LP.movers_np(tr[0], n[0], ORG, RES, DT, mcfg)
        assert table[1:] == (1, 0)
        e._plan_async(goal, "costmap", None)
        e.local_plan_async(pose, win, dt=DT)               # one round is queued in front of it: the field is nowhere near the pose
        far = (CM["x_min"] + 30.5 * RES, CM["y_min"] + 20.5 * RES, 0.3, 0.3)
        tr2, n2, _ = e.track_update(*_dets(pp, [[far]]), [0.1])                        # the tracks move on behind the call
        assert n2[0] == 2 and not np.array_equal(LP.movers_np(tr2[0], n2[0], ORG, RES, DT, mcfg)[0], table[0])
        sv, sw, state = e.local_commands("costmap")        # ... and the first thing fetched is the command
        infl = e._inflated(0, None, False)[0]
        exact = N.navfn_np(infl[0], (1, 27), nav)
        ticks = LP.pose_ticks(pose[:, :2], pose[:, 2], ORG, RES)
        want = LP.best_np(infl[0], exact, ticks[0], win[0], nav, cfg, movers=table[0][:1], mcfg=mcfg)
        assert want["cmd_state"] == 0 and want["n_dynamic"] > 0 and want["n_ok"] >= 8
        assert (int(sv[0]), int(sw[0]), int(state[0])) == (want["sv"], want["sw"], 0)
        assert e.navfn_info("costmap")["rounds"][0] > 1 and np.array_equal(e.navfn_fields("costmap")[0], exact)
        _same_run(LP, e, "costmap", infl, exact[None], [0], ticks, win, nav, cfg, [table], mcfg, "settled")
    finally:
        e.close()


# ---- 5. the call ring: more calls than slots, with and without a fetch between them; the refusals ----
def test_ring_reuse_and_refusals(pp, LP, hip_lib):
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    try:
        L, h = e._lib, e._h
        three, four = np.zeros((B, 3), np.int32), np.zeros((B, 4), np.int32)
        good = np.tile(np.array([[ORG[0], ORG[1], RES, DT]]), (B, 1))

        def call_async(source=0, poses=three, windows=four, frame=good, batch=B):
            P = lambda a: None if a is None else a.ctypes.data      # noqa: E731
            e._check(L.pp_local_plan_movers_async(h, source, P(poses), P(windows), P(frame), batch), "pp_local_plan_movers_async")

        state, arg = "PP_ERR_STATE.*pp_local_plan_movers_async: ", "PP_ERR_ARG.*pp_local_plan_movers_async: "
        e.set_costmap(CM)
        e.set_inflation(INFL, "costmap")
        e.set_navfn(NAV, "costmap")
        with pytest.raises(RuntimeError, match=state + "the local planner of the costmap source is not configured"):
            call_async()
        e.set_local_planner(LOC, "costmap")
        e.upload(_frames(B))
        e._plan_async(GOALS, "costmap", None)
        with pytest.raises(RuntimeError, match=state + "the movers of the costmap source are not configured"):
            call_async()
        mc = pp._lib.PPLocalMoverConfig(0.03, 0.12, 8, 300, 1, 0)
        for field, v, msg in (("horizon", -1, "horizon = -1"), ("horizon", 257, "horizon = 257"), ("mover_weight", 65536, "mover_weight = 65536"),
                              ("pad_hard", -0.1, "pad_hard = -0.1"), ("pad_soft", 0.01, "pad_soft = 0.01"), ("pad_soft", float("nan"), "pad_soft = nan"),
                              ("confirmed_only", 2, "confirmed_only = 2"), ("reserved", 1, "reserved = 1")):
            bad = pp._lib.PPLocalMoverConfig(0.03, 0.12, 8, 300, 1, 0)
            setattr(bad, field, v)
            with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_set_local_movers: .*" + msg):
                e._check(L.pp_set_local_movers(h, 0, ctypes.byref(bad)), "pp_set_local_movers")
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_set_local_movers: source = 2"):
            e._check(L.pp_set_local_movers(h, 2, ctypes.byref(mc)), "pp_set_local_movers")
        assert e.local_movers_config("costmap") is None
        e.set_local_movers(MOV, "costmap")
        with pytest.raises(RuntimeError, match=state + "the handle has no track tables"):
            call_async()
        e.set_tracking(TRK)
        _walk(pp, e, 4)
        tr, n, _ = e.tracks(B)
        infl, pots = e._inflated(0, None, False)[0], e.navfn_fields("costmap")
        gs = e.navfn_info("costmap")["goal_state"]
        cfg, mcfg = e.local_planner_config("costmap"), e.local_movers_config("costmap")
        n_calls = 2 * OFF_RING + 1
        poses = [LP.pose_ticks([[0.1 + 0.05 * i, -0.3 + 0.06 * i], [0.4 - 0.03 * i, 0.35 - 0.05 * i]], [0.2 * i, -0.3 * i], ORG, RES)
                 for i in range(n_calls)]
        wins = [np.array([[40 * i, 40 + 10 * i, -300 + 20 * i, 40], [-100 + 20 * i, 100, -40 * i, 30 + 5 * i]], np.int32) for i in range(n_calls)]
        frames = [np.array([[ORG[0] + 0.01 * i, ORG[1], RES, DT + 0.02 * i], [ORG[0], ORG[1] - 0.02 * i, RES, DT + 0.05 * i]]) for i in range(n_calls)]
        tables = [[LP.movers_np(tr[b], n[b], f[b, :2], f[b, 2], f[b, 3], mcfg) for b in range(B)] for f in frames]
        assert len({t[0][0].tobytes() for t in tables}) == n_calls                # every call's records differ
        for i in range(OFF_RING + 1):                                      # no fetch: slot 0 comes round again
            e._local_cells_async(0, poses[i], wins[i], frame=frames[i])
        _same_run(LP, e, "costmap", infl, pots, gs, poses[OFF_RING], wins[OFF_RING], NAV, cfg, tables[OFF_RING], mcfg, "unfetched")
        for i in range(OFF_RING + 1, n_calls):
            e._local_cells_async(0, poses[i], wins[i], frame=frames[i])
            last = _same_run(LP, e, "costmap", infl, pots, gs, poses[i], wins[i], NAV, cfg, tables[i], mcfg, ("fetched", i))

        def unchanged():
            info = e.local_plan_info("costmap")
            assert all(np.array_equal(info[k], v) for k, v in last[0].items())
            assert all(np.array_equal(a, b) for a, b in zip(e.local_trajectories("costmap"), last[1]))
            assert e.local_keys("costmap").tobytes() == last[2].tobytes() and e.local_movers("costmap")[0].tobytes() == last[3].tobytes()

        # refusals leave the last results as they were, and the next call finds its slot
        def frame_with(b, i, v):
            f = good.copy()
            f[b, i] = v
            return f

        for f, msg in ((None, "frame is NULL"), (frame_with(1, 2, 0.0), "frame: grid 1: res = 0"), (frame_with(0, 2, -0.05), "frame: grid 0: res = -0.05"),
                       (frame_with(0, 2, np.nan), "frame: grid 0: res = nan"), (frame_with(1, 2, np.inf), "frame: grid 1: res = inf"), (frame_with(1, 3, 0.0), "frame: grid 1: dt = 0"),
                       (frame_with(0, 3, -1.0), "frame: grid 0: dt = -1"), (frame_with(0, 3, np.nan), "frame: grid 0: dt = nan"), (frame_with(1, 3, np.inf), "frame: grid 1: dt = inf"),
                       (frame_with(0, 0, np.nan), "frame: grid 0: origin"), (frame_with(1, 1, -np.inf), "frame: grid 1: origin")):
            with pytest.raises(RuntimeError, match=arg + msg):
                call_async(frame=f)
        with pytest.raises(RuntimeError, match=arg + "the last navigation function had 2 grids, batch is 1"):
            call_async(batch=1)
        with pytest.raises(RuntimeError, match=arg + "poses or windows is NULL"):
            call_async(poses=None)
        with pytest.raises(RuntimeError, match=arg + "source = 2"):
            call_async(source=2)
        with pytest.raises(RuntimeError, match=arg + r"windows: grid 1: sv runs from 1000 to 1025, outside \[-1024, 1024\]"):
            call_async(windows=np.array([[0, 0, 0, 0], [1000, 5, 0, 0]], np.int32))
        with pytest.raises(RuntimeError, match=state + "the local planner of the occupancy source is not configured"):
            call_async(source=1)
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_get_local_movers: the last run had 2 grids, batch is 1"):
            e._check(L.pp_get_local_movers(h, 0, None, None, 1), "pp_get_local_movers")
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_get_local_movers: source = -1"):
            e._check(L.pp_get_local_movers(h, -1, None, None, B), "pp_get_local_movers")
        with pytest.raises(ValueError, match="local_plan_async: dt is None and the movers of the costmap source are on"):
            e.local_plan_async()
        with pytest.raises(ValueError, match=r"frame must be \(ox, oy, res, dt\) \[2, 4\]"):
            e._local_cells_async(0, poses[0], wins[0], frame=good[:1])
        unchanged()
        e.set_local_movers(None, "costmap")
        with pytest.raises(RuntimeError, match=state + "the movers of the costmap source are not configured"):
            e._local_cells_async(0, poses[0], wins[0], frame=frames[0])
        e.set_local_movers(MOV, "costmap")
        unchanged()
        # pp_local_plan_async on a handle with the movers on runs without them
        e._local_cells_async(0, poses[1], wins[1])
        info = e.local_plan_info("costmap")
        assert set(info) == set(LP.RESULT) | {"score"}
        for b in range(B):
            want = LP.best_np(infl[b], pots[b], poses[1][b], wins[1][b], NAV, cfg, gs[b])
            assert all(int(info[k][b]) == want[k] for k in LP.RESULT + ("score",)) and np.array_equal(e.local_keys("costmap")[b], want["keys"])
        e._local_cells_async(0, poses[2], wins[2], frame=frames[2])
        _same_run(LP, e, "costmap", infl, pots, gs, poses[2], wins[2], NAV, cfg, tables[2], mcfg, "after the refusals")
    finally:
        e.close()
