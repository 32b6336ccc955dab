"""The navigation function on the GPU (csrc/navfn.hip: k_navfn_init, k_navfn_relax, k_navfn_finish) against navfn.py's
restatement: fields, paths, states and counts must be EQUAL (np.array_equal).  No tolerances: the device works in
integers and the field is the unique fixed point of its relaxation, whatever the tiling or the number of rounds.
Stand-alone on the shared cases (tests/navfn_cases.py), then behind the inflation of the costmap and of the rolling
occupancy maps, whose own outputs must stay the bytes of an engine that never heard of the stage."""
import numpy as np
import pytest

import navfn_cases as K

pytestmark = pytest.mark.gpu

OFF_RING = 4            # csrc/pp_ring.h


@pytest.fixture(scope="module")
def N(pp, hip_lib):
    return pp.navfn


def _check(N, got, name, what=None):
    pot, path, state, info = got
    wpot, winfo, wpath, wstate = K.reference(name)
    what = what or name
    assert pot.dtype == np.uint32 and path.dtype == np.int32 and path.ndim == 2 and path.shape[1] == 2
    assert np.array_equal(pot, wpot), what
    assert np.array_equal(path, wpath), what
    assert state == wstate and info["path_state"] == wstate, what
    assert info["path_len"] == len(wpath) and info["goal_state"] == winfo["goal_state"] and info["reached"] == winfo["reached"], what
    assert info["rounds"] >= 1, what


# ---- 1. stand-alone ----
@pytest.mark.parametrize("name", K.NAMES)
def test_standalone_equals_the_restatement(N, name):
    _, g, goal, start, cfg = K.case(name)
    got = N.navfn(g, goal, cfg, starts=start, info=True)
    _check(N, got, name)
    again = N.navfn(g, goal, cfg, starts=start, info=True)                 # the same bytes on every run
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and again[2] == got[2]
    assert {k: v for k, v in again[3].items() if k != "rounds"} == {k: v for k, v in got[3].items() if k != "rounds"}


def test_standalone_batch_equals_its_grids_one_by_one(N):
    pot, paths, state, info = N.navfn(K.BATCH, K.BATCH_GOALS, K.BATCH_CFG, starts=K.BATCH_STARTS, info=True)
    assert pot.shape == K.BATCH.shape and state.shape == (3,) and len(paths) == 3
    for b in range(3):
        wpot, winfo = N.navfn_np(K.BATCH[b], K.BATCH_GOALS[b], K.BATCH_CFG, info=True)
        wpath, wstate = N.descend_np(wpot, K.BATCH[b], K.BATCH_STARTS[b], K.BATCH_CFG)
        one = N.navfn(K.BATCH[b], K.BATCH_GOALS[b], K.BATCH_CFG, starts=K.BATCH_STARTS[b], info=True)
        for p, pa, s, i in (one, (pot[b], paths[b], state[b], {k: v[b] for k, v in info.items()})):
            assert np.array_equal(p, wpot) and np.array_equal(pa, wpath) and s == wstate, b
            assert (i["goal_state"], i["reached"], i["path_len"]) == (winfo["goal_state"], winfo["reached"], len(wpath)), b
    assert info["goal_state"].tolist() == [1, 0, 0] and state.tolist() == [1, 0, 0]
    assert info["rounds"][2] > info["rounds"][1] >= 1              # the serpentine went on after the open grid stood
    assert len(paths[2]) > 1024


# ---- 2. the getter's continuation, and idle rounds ----
@pytest.mark.parametrize("name", ["serpentine_whole", "corridor"])
def test_queued_rounds_never_show_in_a_result(N, name):
    _, g, goal, start, cfg = K.case(name)
    for q in (1, 2):
        got = N.navfn(g, goal, dict(cfg, queued_rounds=q), starts=start, info=True)
        _check(N, got, name, (name, q))
        assert got[3]["rounds"] > q, (name, q)                     # the rounds still missing were queued behind the first
    got = N.navfn(g, goal, dict(cfg, queued_rounds=512), starts=start, info=True)
    _check(N, got, name, (name, 512))
    assert got[3]["rounds"] < 512                                   # the rounds behind the standing field returned at once


# ---- 3. behind the costmap stage and behind the occupancy maps ----
B = 2
CM = dict(x_min=-0.1, y_min=-0.7, resolution=0.05, width=37, height=29, z_min=-0.2, z_max=0.2)
INFL = dict(resolution=0.05, inscribed_radius=0.05, inflation_radius=0.2, cost_scaling_factor=8.0)
NAV = dict(lethal_cost=100, allow_unknown=1, max_path=128)
GOALS = np.array([[1.62, 0.31], [1.41, -0.52]])


def _tiny(pp, batch):
    return pp.config.tiny_config(batch)


def _weights(pp, d, seed=7):
    w = dict(pp.weights.init_weights(d, seed=seed))
    w["rpn/conv_cls/bias"] = np.array(w["rpn/conv_cls/bias"], np.float32) + np.float32(0.6)
    return w


def _frames(n, seed=300):
    out = []
    for b in range(n):
        rng = np.random.default_rng(seed + b)
        out.append(rng.uniform([0.05, -0.6, -2.5], [1.3, 0.6, 2.5], (700 + 150 * b, 3)).astype(np.float32))
    return out


@pytest.fixture(scope="module")
def pair(pp, hip_lib):
    """Two engines on the same weights: the first never sets the stage."""
    es = []
    for _ in range(2):
        e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
        e.load_weights(_weights(pp, e.d))
        es.append(e)
    yield es
    for e in es:
        e.close()


def _want(N, grid, goal, start, cfg):
    pot, info = N.navfn_np(grid, goal, cfg, info=True)
    path, state = N.descend_np(pot, grid, start, cfg)
    return pot, info, path, state


def _same_run(N, e, source, grids, goals, starts, cfg, what):
    pots = e.navfn_fields(source)
    paths, states = e.navfn_paths(source)
    info = e.navfn_info(source)
    assert pots.dtype == np.uint32 and pots.shape == grids.shape and states.dtype == np.int32
    for b in range(len(grids)):
        pot, winfo, path, state = _want(N, grids[b], goals[b], None if starts is None else starts[b], cfg)
        assert np.array_equal(pots[b], pot), (what, b)
        assert np.array_equal(paths[b], path) and paths[b].dtype == np.int32, (what, b)
        assert states[b] == state == info["path_state"][b], (what, b)
        assert info["goal_state"][b] == winfo["goal_state"] and info["reached"][b] == winfo["reached"], (what, b)
    return pots, paths, states, info


def test_costmap_source(pp, N, pair):
    plain_e, e = pair
    rect, trv, _ = pp.synth.default_calib()
    rect, trv = np.stack([rect] * B), np.stack([trv] * B)
    frames = _frames(B)
    for x in (plain_e, e):
        x.set_costmap(CM)
        x.set_inflation(INFL, "costmap")
    dets0, n0 = plain_e.detect(frames, rect, trv)
    infl0 = plain_e.inflated_costmaps()
    grids0 = plain_e.costmaps()

    assert e.navfn_config("costmap") is None
    e.set_navfn(NAV, "costmap")
    cfg = e.navfn_config("costmap")
    assert cfg == N.NavfnConfig(**NAV) and e.navfn_config("occupancy") is None
    dets, n = e.detect(frames, rect, trv)
    infl = e.inflated_costmaps()
    e.navfn_async(GOALS)
    org, shape = (CM["x_min"], CM["y_min"]), (CM["height"], CM["width"])
    goals = N.goal_cells(GOALS, org, CM["resolution"], shape)
    starts = N.goal_cells(np.zeros((B, 2)), org, CM["resolution"], shape)
    assert starts[:, 0].tolist() == [2] * B and (goals >= 0).all() and (goals < [37, 29]).all()
    pots, paths, states, info = _same_run(N, e, "costmap", infl, goals, starts, cfg, "costmap")
    print("costmap source:", {k: v.tolist() for k, v in info.items()}, [len(p) for p in paths])
    assert (info["goal_state"] == 0).all() and (states == 0).all() and (info["rounds"] >= 1).all()
    assert not np.array_equal(pots[0], pots[1])
    # the source's grids, the inflated grids and the detections are what they are without the stage
    assert e.costmaps().tobytes() == grids0.tobytes() and infl.tobytes() == infl0.tobytes()
    assert e._inflated(0, None, False)[0].tobytes() == infl0.tobytes()
    d1, n1 = e.detections()
    assert (dets.tobytes(), n.tobytes(), d1.tobytes(), n1.tobytes()) == (dets0.tobytes(), n0.tobytes(), dets0.tobytes(), n0.tobytes())
    # plan: the same paths, in metres
    mpaths, mstates = e.plan(GOALS)
    assert np.array_equal(mstates, states)
    for b in range(B):
        assert mpaths[b].dtype == np.float64
        assert np.array_equal(mpaths[b], N.path_to_metres(paths[b], org, CM["resolution"])), b
    # given starts, and none
    S = np.array([[0.4, -0.6], [0.0, 0.0]])
    e.navfn_async(GOALS, starts=S)
    _same_run(N, e, "costmap", infl, goals, N.goal_cells(S, org, CM["resolution"], shape), cfg, "starts")
    e.navfn_async(GOALS, starts=False)
    _, p4, s4, _ = _same_run(N, e, "costmap", infl, goals, None, cfg, "no starts")
    assert s4.tolist() == [4, 4] and all(len(p) == 0 for p in p4)
    # off: the call is refused, the inflation goes on
    e.set_navfn(None, "costmap")
    assert e.navfn_config("costmap") is None
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_navfn_async: the navigation function of the costmap source is not configured"):
        e.navfn_async(GOALS)
    assert e.inflated_costmaps().tobytes() == infl0.tobytes()
    for x in (plain_e, e):
        x.set_inflation(None, "costmap")
        x.set_costmap(None)


S3 = 3
OCC = dict(resolution=0.1, z_min=0.0, z_max=1.0, max_range=2.5, width=37, height=29)       # rows of 40 cells on the device
OCC_INFL = dict(inscribed_radius=0.1, inflation_radius=0.5, cost_scaling_factor=4.0, lethal_threshold=65)
OCC_NAV = dict(allow_unknown=1, unknown_cost=20, max_path=256)


def _occ_frames(k):
    out = []
    for s in range(S3):
        rng = np.random.default_rng(40 + 10 * k + s)
        out.append(rng.uniform([-2.0, -1.6, -0.5], [2.0, 1.6, 1.2], (300 + 37 * s, 3)).astype(np.float32))
    return out


def test_occupancy_source(pp, N, hip_lib):
    plain_e = pp.Engine(_tiny(pp, S3), max_batch=S3, max_points_per_frame=4096)
    e = pp.Engine(_tiny(pp, S3), max_batch=S3, max_points_per_frame=4096)
    try:
        for x in (plain_e, e):
            x.set_occupancy(OCC)
            x.set_inflation(OCC_INFL, "occupancy")
        e.set_navfn(OCC_NAV, "occupancy")
        cfg = e.navfn_config("occupancy")
        shape = (OCC["height"], OCC["width"])
        sensor = np.array([[OCC["width"] // 2, OCC["height"] // 2]] * S3, np.int32)
        for k in range(2):                                                 # the window moves
            frames = _occ_frames(k)
            xy = np.array([[0.23 * k + 0.1 * s, -0.17 * k * (s - 1)] for s in range(S3)])
            poses = np.stack([pp.sweeps.pose_from_xyyaw(xy[s, 0], xy[s, 1], 0.3 * k + 0.5 * s) for s in range(S3)])
            for x in (plain_e, e):
                x.upload(frames)
                x.occupancy_update_async(poses)
            G = xy + np.array([[1.2, 0.6], [-1.1, 0.9], [9.0, 0.0]])       # the third lies outside its window
            mpaths, mstates = e.plan(G, "occupancy")
            infl, org = e._inflated(1, None, False)[0], e._occ_origins.copy()
            infl0, org0 = plain_e.inflated_occupancy_maps()
            assert infl.tobytes() == infl0.tobytes() and org.tobytes() == org0.tobytes(), k
            g3 = e.occupancy_maps(logodds=True)
            g30 = plain_e.occupancy_maps(logodds=True)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(g3, g30)), k
            goals = N.goal_cells(G, org, OCC["resolution"], shape)
            pots, paths, states, info = _same_run(N, e, "occupancy", infl, goals, sensor, cfg, ("occupancy", k))
            print("occupancy source:", k, {key: v.tolist() for key, v in info.items()}, [len(p) for p in paths])
            assert info["goal_state"].tolist()[2] == 2 and (pots[2] == N.UNREACHED).all() and states[2] == 1
            assert np.array_equal(mstates, states)
            for s in range(S3):
                assert np.array_equal(mpaths[s], N.path_to_metres(paths[s], org[s], OCC["resolution"])), (k, s)
        # a reset stream reads all unknown: with unknown cells blocked nothing is reached and a goal in the window is blocked
        e.set_navfn(dict(OCC_NAV, allow_unknown=0), "occupancy")
        e.occupancy_reset(1)
        e.inflate_async("occupancy")
        e._navfn_cells_async(1, goals * 0 + [20, 10], sensor)
        pots = e.navfn_fields("occupancy")
        info = e.navfn_info("occupancy")
        assert (pots[1] == N.UNREACHED).all() and info["goal_state"][1] == 1 and info["reached"][1] == 0 and info["path_state"][1] == 1
        e.navfn_async(G, "occupancy")                                      # its origin is NaN: the goal lies outside
        info = e.navfn_info("occupancy")
        assert info["goal_state"][1] == 2 and (e.navfn_fields("occupancy")[1] == N.UNREACHED).all()
    finally:
        plain_e.close()
        e.close()


# ---- 4. the call ring: more calls than slots, with and without a fetch between them ----
def test_ring_reuse_and_refusals(pp, N, hip_lib):
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    try:
        state = "PP_ERR_STATE.*pp_navfn_async: "
        e.set_costmap(CM)
        # the stage off; the inflation off; no inflation run
        with pytest.raises(RuntimeError, match="navfn_async: no inflation has run on the costmap source"):
            e.navfn_async(GOALS)
        cells = np.array([[30, 20], [33, 3]], np.int32)
        with pytest.raises(RuntimeError, match=state + "the navigation function of the costmap source is not configured"):
            e._check(e._lib.pp_navfn_async(e._h, 0, cells.ctypes.data, None, B), "pp_navfn_async")
        e.set_navfn(NAV, "costmap")
        with pytest.raises(RuntimeError, match=state + "the inflation of the costmap source is not configured"):
            e._check(e._lib.pp_navfn_async(e._h, 0, cells.ctypes.data, None, B), "pp_navfn_async")
        e.set_inflation(INFL, "costmap")
        with pytest.raises(RuntimeError, match=state + "no inflation has run on this source"):
            e._check(e._lib.pp_navfn_async(e._h, 0, cells.ctypes.data, None, B), "pp_navfn_async")
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_navfn: no navigation function has run"):
            e._check(e._lib.pp_get_navfn(e._h, 0, None, None, None, B), "pp_get_navfn")
        e.upload(_frames(B, seed=500))
        infl = e.inflated_costmaps()
        cfg = e.navfn_config("costmap")
        starts = np.array([[2, 14], [2, 14]], np.int32)
        n_calls = 2 * OFF_RING + 1
        goals = [np.array([[36 - i, 3 + 2 * i], [10 + 3 * i, 28 - i]], np.int32) for i in range(n_calls)]
        for i in range(OFF_RING + 1):                                      # no fetch: slot 0 comes round again
            e._navfn_cells_async(0, goals[i], starts)
        _same_run(N, e, "costmap", infl, goals[OFF_RING], starts, cfg, "unfetched")
        for i in range(OFF_RING + 1, n_calls):
            e._navfn_cells_async(0, goals[i], starts)
            last = _same_run(N, e, "costmap", infl, goals[i], starts, cfg, ("fetched", i))

        def unchanged():
            assert e.navfn_fields("costmap").tobytes() == last[0].tobytes()
            p, s = e.navfn_paths("costmap")
            assert all(np.array_equal(a, b) for a, b in zip(p, last[1])) and np.array_equal(s, last[2])
            assert all(np.array_equal(e.navfn_info("costmap")[k], v) for k, v in last[3].items())

        # refusals leave the last results as they were, and the next call finds its slot
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_navfn_async: the last inflation had 2 grids, batch is 1"):
            e._check(e._lib.pp_navfn_async(e._h, 0, cells.ctypes.data, None, 1), "pp_navfn_async")
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_navfn_async: goals is NULL"):
            e._check(e._lib.pp_navfn_async(e._h, 0, None, None, B), "pp_navfn_async")
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_navfn_async: source = 2"):
            e._check(e._lib.pp_navfn_async(e._h, 2, cells.ctypes.data, None, B), "pp_navfn_async")
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_get_navfn: the last run had 2 grids, batch is 1"):
            e._check(e._lib.pp_get_navfn(e._h, 0, None, None, None, 1), "pp_get_navfn")
        with pytest.raises(RuntimeError, match=state + "the navigation function of the occupancy source is not configured"):
            e._check(e._lib.pp_navfn_async(e._h, 1, cells.ctypes.data, None, B), "pp_navfn_async")
        unchanged()
        e.set_inflation(None, "costmap")
        with pytest.raises(RuntimeError, match=state + "the inflation of the costmap source is not configured"):
            e._navfn_cells_async(0, goals[0], starts)
        unchanged()
        e.set_inflation(INFL, "costmap")
        e.set_navfn(None, "costmap")
        with pytest.raises(RuntimeError, match=state + "the navigation function of the costmap source is not configured"):
            e._navfn_cells_async(0, goals[0], starts)
        unchanged()
        e.set_navfn(NAV, "costmap")
        e._navfn_cells_async(0, goals[1], starts)
        _same_run(N, e, "costmap", infl, goals[1], starts, cfg, "after the refusals")
    finally:
        e.close()
