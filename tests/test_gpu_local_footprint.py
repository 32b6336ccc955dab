"""The local planner's footprint on the GPU (csrc/local_plan.hip: the FOOT instantiations of the rollout and the finish)
against local_planner.py's restatement: result words, FOOT_INFO and MOVER_INFO words, scores, trajectories and all keys
must be EQUAL (np.array_equal), no tolerances.  Stand-alone on the shared cases (tests/local_footprint_cases.py: the probe
counts round every lane group and 64-probe trip, the extreme probes, the sample counts round a workgroup, 1 and 256
steps, wrapping headings, negative coordinates, both table orders, every state, foot_lethal, unknown cells, movers); a
batch whose grids are in states 0, 5 and 2; then behind the costmap and the occupancy maps with movers off and on; the
footprint turned off again; every refusal."""
import ctypes

import numpy as np
import pytest

import local_footprint_cases as F
from test_gpu_local_movers import (B, CM, DT, GOALS, INFL, LOC, MOV, NAV, OCC, OCC_INFL, OCC_LOC, OCC_MOV, OCC_NAV, ORG, RES, S3, TRK, _frames,
                                   _occ_frames, _tiny, _walk)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def LP(pp, hip_lib):
    return pp.local_planner


def _equal(LP, got, want, what, keys=True):
    """`got` of local_plan / the engine for one grid against best_np's dict (with a footprint, with or without movers)."""
    names = LP.RESULT + LP.FOOT_INFO + (("n_movers", "n_dynamic", "near") if "n_movers" in want else ())
    for k in names:
        assert int(got[k]) == want[k], (what, k, int(got[k]), want[k])
    assert int(got["score"]) == want["score"], what
    assert got["traj"].dtype == np.int32 and np.array_equal(got["traj"], want["traj"]), what
    if keys:
        assert got["keys"].dtype == np.uint64 and np.array_equal(got["keys"], want["keys"]), what


def _plan(LP, c, keys=True, **kw):
    b = c.base
    more = {} if c.movers is None else dict(movers=c.movers, mover_cfg=c.mcfg)
    return LP.local_plan(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, goal_state=b.goal_state, keys=keys, footprint=c.probes, fcfg=c.fcfg or None,
                         **more, **kw)


# ---- 1. stand-alone ----
@pytest.mark.parametrize("name", F.NAMES)
def test_standalone_equals_the_restatement(LP, name):
    c = F.case(name)
    got = _plan(LP, c)
    want = F.reference(name)
    print(name, {k: int(got[k]) for k in LP.RESULT + LP.FOOT_INFO})
    _equal(LP, got, want, name)
    assert set(got) == set(want) | ({"n_skipped"} if c.movers is not None else set())
    quiet = _plan(LP, c, keys=False)                        # no keys stored
    assert "keys" not in quiet
    _equal(LP, quiet, want, (name, "no keys"), keys=False)


@pytest.mark.parametrize("name", ["outline_256", "samples_513", "movers_and_footprint", "state_5_start_blocked"])
def test_two_runs_give_identical_bytes(LP, name):
    a, b = _plan(LP, F.case(name)), _plan(LP, F.case(name))
    assert set(a) == set(b)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_probes_that_touch_nothing_give_the_point_robots_bytes(LP):
    """One probe on the centre itself is free wherever the centre is: keys, trajectory and words of the run without a
    footprint, through the other instantiation."""
    for name in ("outline_56", "samples_257", "steps_256"):
        b = F.case(name).base
        off = LP.local_plan(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, goal_state=b.goal_state, keys=True)
        on = LP.local_plan(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, goal_state=b.goal_state, keys=True, footprint=[(0, 0)])
        assert on["keys"].tobytes() == off["keys"].tobytes() and on["traj"].tobytes() == off["traj"].tobytes()
        assert all(on[k] == off[k] for k in LP.RESULT + ("score",)) and (on["n_probes"], on["n_footprint"], on["start_probe"]) == (1, 0, -1)
        assert set(off) == set(LP.RESULT) | {"score", "traj", "keys"}


def test_standalone_batch_in_states_0_5_and_2(LP):
    got = LP.local_plan(F.BATCH, F.BATCH_POTS, F.BATCH_POSES, F.BATCH_WINDOWS, F.BATCH_NCFG, F.BATCH_CFG, keys=True, footprint=F.BATCH_PROBES)
    assert got["cmd_state"].tolist() == [0, 5, 2] and got["n_probes"].tolist() == [56] * 3 and got["start_probe"].dtype == np.int32
    assert got["start_probe"][0] == -1 and got["start_probe"][1] >= 0 and got["start_probe"][2] == -1
    for b in range(3):
        one = LP.local_plan(F.BATCH[b], F.BATCH_POTS[b], F.BATCH_POSES[b], F.BATCH_WINDOWS[b], F.BATCH_NCFG, F.BATCH_CFG, keys=True,
                            footprint=F.BATCH_PROBES)
        for g in (one, {k: v[b] for k, v in got.items()}):
            _equal(LP, g, F.batch_reference(b), b)


# ---- 2. behind an engine ----
def _same_run(LP, e, source, grids, pots, goal_state, poses, windows, ncfg, cfg, fp, fc, what, tables=None, mcfg=None, keys=True):
    """The engine's results of the source's last local_plan_async with a footprint (and, with `tables`, movers) against
    best_np on the given grids and fields.  The words come first, the keys after them: the getter rolls once more to
    store them."""
    info = e.local_plan_info(source)
    foot = e.local_footprint(source)
    traj = e.local_trajectories(source)
    kk = e.local_keys(source) if keys else None
    again = e.local_plan_info(source)
    assert all(np.array_equal(info[k], again[k]) for k in info), what       # ... and leaves every word as it was
    for b in range(len(grids)):
        more = {}
        if tables is not None:
            m, n, _ = tables[b]
            more = dict(movers=m[:max(n, 0)], mcfg=mcfg)
        want = LP.best_np(grids[b], pots[b], poses[b], windows[b], ncfg, cfg, goal_state[b], footprint=fp, fcfg=fc, **more)
        if tables is not None:
            want["n_movers"] = tables[b][1]
        got = {k: v[b] for k, v in info.items()}
        got["traj"] = traj[b]
        if keys:
            got["keys"] = kk[b]
        _equal(LP, got, want, (what, b), keys)
        assert all(foot[k][b] == want[k] for k in LP.FOOT_INFO)
    return info, traj, kk


SMALL = dict(length=0.16, width=0.10, resolution=RES)       # 3.2 x 2 cells of the costmap's 0.05 m


@pytest.mark.parametrize("allow_unknown", [1, 0])
def test_costmap_source(pp, LP, hip_lib, allow_unknown):
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    try:
        nav = dict(NAV, allow_unknown=allow_unknown)
        e.set_costmap(CM)
        e.set_inflation(INFL, "costmap")
        e.set_navfn(nav, "costmap")
        e.set_local_planner(LOC, "costmap")
        e.upload(_frames(B))
        cfg = e.local_planner_config("costmap")
        assert e.local_footprint_config("costmap") is None
        # before the footprint was ever set
        e._plan_async(GOALS, "costmap", None)
        e.local_plan_async(dt=DT)
        before = (e.local_plan_info("costmap"), e.local_trajectories("costmap"), e.local_keys("costmap"))
        infl, pots = e._inflated(0, None, False)[0], e.navfn_fields("costmap")
        gs = e.navfn_info("costmap")["goal_state"]
        with pytest.raises(RuntimeError, match="local_footprint: the last local plan of the costmap source had no footprint"):
            e.local_footprint("costmap")
        # the footprint, no movers
        fp = LP.Footprint.rectangle(SMALL["length"], SMALL["width"], resolution=RES)
        e.set_local_footprint(fp, dict(foot_lethal=100), "costmap")
        got_fp, fc = e.local_footprint_config("costmap")
        assert got_fp == fp and fc == LP.FootprintConfig(100) and e.local_footprint_config("occupancy") is None
        e.local_plan_async(dt=DT)
        poses = LP.pose_ticks(np.zeros((B, 2)), 0.0, ORG, RES)
        wide = np.tile(np.array([[0, 204, -512, 102]], np.int32), (B, 1))
        info, _, _ = _same_run(LP, e, "costmap", infl, pots, gs, poses, wide, nav, cfg, fp, fc, "default")
        print("costmap source, allow_unknown", allow_unknown, {k: v.tolist() for k, v in info.items()})
        assert set(info) == set(before[0]) | set(LP.FOOT_INFO)
        # given poses and windows, a stricter foot_lethal, a table of raw probes
        raw = np.array([(300, 0), (0, 260), (-280, 0), (0, -260), (2000, 0)], np.int32)
        e.set_local_footprint(raw, dict(foot_lethal=60), "costmap")
        with pytest.raises(RuntimeError, match="no local plan has run on the costmap source"):
            e.local_plan_info("costmap")                    # the table the last run read is gone
        P = np.array([[0.3, -0.2, 0.4], [0.2, 0.1, -0.7]])
        Wn = np.array([[100, 100, -300, 60], [-200, 150, -250, 50]], np.int32)
        e.local_plan_async(P, Wn, dt=0.5)
        info2, _, _ = _same_run(LP, e, "costmap", infl, pots, gs, LP.pose_ticks(P[:, :2], P[:, 2], ORG, RES), Wn, nav, cfg, raw,
                                LP.FootprintConfig(60), "given")
        print("costmap source, given", {k: v.tolist() for k, v in info2.items()})
        # with the movers on: both async entries pick the footprint up
        e.set_local_footprint(fp, True, "costmap")
        e.set_local_movers(MOV, "costmap")
        e.set_tracking(TRK)
        _walk(pp, e, 4)
        tr, n, _ = e.tracks(B)
        mcfg = e.local_movers_config("costmap")
        tables = [LP.movers_np(tr[b], n[b], ORG, RES, DT, mcfg) for b in range(B)]
        e.local_plan_async(dt=DT)
        info3, _, _ = _same_run(LP, e, "costmap", infl, pots, gs, poses, wide, nav, cfg, fp, fc, "movers", tables, mcfg)
        print("costmap source, movers", {k: v.tolist() for k, v in info3.items()})
        assert set(info3) == set(before[0]) | set(LP.FOOT_INFO) | set(LP.MOVER_INFO)
        lim = LP.LocalLimits(v_min=-0.1, v_max=0.4, w_max=1.5, acc_v=1.0, acc_w=4.0, sim_time=1.0, period=0.2)
        V = np.array([[0.2, 0.0], [0.1, -0.3]])
        v, w, state = e.drive(GOALS, V, lim)                # drive picks it up with no new argument
        win = np.array([lim.window(V[b, 0], V[b, 1], cfg.nv, cfg.nw, RES) for b in range(B)], np.int32)
        tables = [LP.movers_np(tr[b], n[b], ORG, RES, lim.step_dt(RES), mcfg) for b in range(B)]
        info4, _, _ = _same_run(LP, e, "costmap", infl, pots, gs, poses, win, nav, cfg, fp, fc, "drive", tables, mcfg, keys=False)
        mv, mw = LP.command_metric(info4["sv"], info4["sw"], RES, lim.step_dt(RES))
        assert np.array_equal(v, mv) and np.array_equal(w, mw) and np.array_equal(state, info4["cmd_state"])
        # the footprint changed something somewhere, or the runs above show nothing
        runs = (info, info2, info3, info4)
        assert sum(int(r["n_footprint"].sum()) + int((r["cmd_state"] == 5).sum()) for r in runs) > 0
        # off again: the bytes this engine gave before the footprint was ever set, and no words to fetch
        e.set_local_movers(None, "costmap")
        e.set_local_footprint(None, source="costmap")
        assert e.local_footprint_config("costmap") is None
        e._plan_async(GOALS, "costmap", None)
        e.local_plan_async(dt=DT)
        now = (e.local_plan_info("costmap"), e.local_trajectories("costmap"), e.local_keys("costmap"))
        assert set(now[0]) == set(before[0]) and all(now[0][k].tobytes() == before[0][k].tobytes() for k in before[0])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(now[1], before[1])) and now[2].tobytes() == before[2].tobytes()
        with pytest.raises(RuntimeError, match="local_footprint: the last local plan of the costmap source had no footprint"):
            e.local_footprint("costmap")
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_local_footprint: the last run of the costmap source had no footprint"):
            e._check(e._lib.pp_get_local_footprint(e._h, 0, None, B), "pp_get_local_footprint")
    finally:
        e.close()


@pytest.mark.parametrize("movers", [False, True])
def test_occupancy_source(pp, LP, hip_lib, movers):
    e = pp.Engine(_tiny(pp, S3), max_batch=S3, max_points_per_frame=4096)
    try:
        e.set_occupancy(OCC)
        e.set_inflation(OCC_INFL, "occupancy")
        e.set_navfn(OCC_NAV, "occupancy")
        e.set_local_planner(OCC_LOC, "occupancy")
        # a base with a long trailer: the obstacles of _occ_frames lie 1.3 to 2 m behind the sensors, where only its rear reaches
        fp = LP.Footprint.rectangle(2.4, 0.4, -0.6, resolution=OCC["resolution"])
        e.set_local_footprint(fp, source="occupancy")
        assert e.local_footprint_config("costmap") is None and e.local_footprint_config("occupancy")[0] == fp
        if movers:
            e.set_local_movers(OCC_MOV, "occupancy")
            e.set_tracking(TRK)
        cfg, ncfg = e.local_planner_config("occupancy"), e.navfn_config("occupancy")
        mcfg = e.local_movers_config("occupancy")
        lim = LP.LocalLimits(v_min=0.0, v_max=0.6, w_max=1.2, acc_v=2.0, acc_w=6.0, sim_time=1.0, period=0.25)
        dt = lim.step_dt(OCC["resolution"])
        seen = 0
        for k in range(2):                                                 # the window moves
            xy = np.array([[0.23 * k + 0.1 * s, -0.17 * k * (s - 1)] for s in range(S3)])
            yaw = np.array([0.3 * k + 0.5 * s for s in range(S3)])
            poses = np.stack([pp.sweeps.pose_from_xyyaw(xy[s, 0], xy[s, 1], yaw[s]) for s in range(S3)])
            e.upload(_occ_frames(k))
            e.occupancy_update_async(poses)
            tables = None
            if movers:
                _walk(pp, e, 3, poses[:2], first=3 * k)
                tr, n = e.tracks_fixed(S3)
            G = xy + np.array([[1.2, 0.6], [0.9, -0.8], [0.8, 0.3]])
            V = np.array([[0.3, 0.1], [0.0, 0.0], [0.6, -1.0]])
            v, w, state = e.drive(G, V, lim, "occupancy")
            infl, org = e._inflated(1, None, False)[0], e._occ_origins.copy()
            pots = e.navfn_fields("occupancy")
            gs = e.navfn_info("occupancy")["goal_state"]
            ticks = LP.pose_ticks(xy, yaw, org, OCC["resolution"])
            win = np.array([lim.window(V[s, 0], V[s, 1], cfg.nv, cfg.nw, OCC["resolution"]) for s in range(S3)], np.int32)
            if movers:
                tables = [LP.movers_np(tr[s], n[s], org[s], OCC["resolution"], dt, mcfg) for s in range(S3)]
            info, _, _ = _same_run(LP, e, "occupancy", infl, pots, gs, ticks, win, ncfg, cfg, fp, LP.FootprintConfig(), ("occupancy", k), tables, mcfg)
            print("occupancy source:", k, {key: val.tolist() for key, val in info.items()})
            mv, mw = LP.command_metric(info["sv"], info["sw"], OCC["resolution"], dt)
            assert np.array_equal(v, mv) and np.array_equal(w, mw) and np.array_equal(state, info["cmd_state"])
            seen += int(info["n_footprint"].sum()) + int((info["cmd_state"] == 5).sum())
        assert seen > 0
    finally:
        e.close()


# ---- 3. the refusals ----
def test_refusals(pp, LP, hip_lib):
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    try:
        L, h = e._lib, e._h
        probes = np.array([[300, 0], [0, 260]], np.int32)
        good = pp._lib.PPLocalFootprintConfig(100, (0, 0, 0))
        arg = "PP_ERR_ARG.*pp_set_local_footprint: "

        def call(cfg=good, p=probes, n=2, source=0):
            e._check(L.pp_set_local_footprint(h, source, None if cfg is None else ctypes.byref(cfg), None if p is None else p.ctypes.data, n),
                     "pp_set_local_footprint")

        def with_probe(q, v):
            p = probes.copy()
            p[q] = v
            return p

        for kw, msg in ((dict(cfg=pp._lib.PPLocalFootprintConfig(0, (0, 0, 0))), "foot_lethal = 0"),
                        (dict(cfg=pp._lib.PPLocalFootprintConfig(101, (0, 0, 0))), "foot_lethal = 101"),
                        (dict(cfg=pp._lib.PPLocalFootprintConfig(100, (0, 1, 0))), r"reserved\[1\] = 1"),
                        (dict(cfg=None), "cfg is NULL"), (dict(p=None), "probes is NULL"), (dict(n=257), "n_probes = 257"), (dict(n=-1), "n_probes = -1"),
                        (dict(p=with_probe(1, (32768, 0))), r"probe 1: \(32768, 0\)"), (dict(p=with_probe(0, (0, -32768))), r"probe 0: \(0, -32768\)"),
                        (dict(source=2), "source = 2")):
            with pytest.raises(RuntimeError, match=arg + msg):
                call(**kw)
        assert e.local_footprint_config("costmap") is None
        with pytest.raises(ValueError, match="probe 1: "):
            e.set_local_footprint([(0, 0), (0, 40000)])
        with pytest.raises(ValueError, match="foot_lethal = 0"):
            e.set_local_footprint(probes, dict(foot_lethal=0))
        call(n=0, p=None, cfg=None)                          # off while it is off: nothing to do
        call(p=with_probe(1, (32767, -32767)))
        got, fc = e.local_footprint_config("costmap")
        assert got.probes.tolist() == [[300, 0], [32767, -32767]] and fc.foot_lethal == 100
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_local_footprint: no local plan has run"):
            e._check(L.pp_get_local_footprint(h, 0, None, B), "pp_get_local_footprint")
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_get_local_footprint: source = -1"):
            e._check(L.pp_get_local_footprint(h, -1, None, B), "pp_get_local_footprint")
        call(n=0, p=None)
        assert e.local_footprint_config("costmap") is None
    finally:
        e.close()
