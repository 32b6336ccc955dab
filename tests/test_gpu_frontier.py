"""The frontier stage on the GPU (csrc/frontier.hip: k_frontier_mark, k_frontier_label, k_frontier_stats, k_frontier_rep,
k_frontier_select) against frontier.py's restatement: labels, words and info must be EQUAL (np.array_equal).  No
tolerances: the device works in integers and the labelling, the representatives and the order are unique, whatever the
tiling, the order of the unions or the atomics.  Stand-alone on the shared cases (tests/frontier_cases.py), then behind the
inflation of the rolling occupancy maps and of the costmap, whose own outputs must stay the bytes of an engine that never
heard of the stage."""
import ctypes

import numpy as np
import pytest

import frontier_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F(pp, hip_lib):
    return pp.frontier


def _equal(got, want, what):
    labels, words, info = got
    wl, ww, wi = want
    assert labels.dtype == np.uint32 and words.dtype == np.int32 and words.ndim == 2 and words.shape[1] == 8 and info.dtype == np.int32
    assert np.array_equal(info, wi), (what, info.tolist(), wi.tolist())
    assert np.array_equal(labels, wl), what
    assert np.array_equal(words, ww), (what, words.tolist(), ww.tolist())


# ---- 1. stand-alone ----
@pytest.mark.parametrize("name", K.NAMES)
def test_standalone_equals_the_restatement(F, name):
    _, g, cfg, ref, pot = K.case(name)
    got = F.frontier(g, cfg, ref, pot)
    _equal(got, K.reference(name), name)
    again = F.frontier(g, cfg, ref, pot)                                    # the same bytes on every run
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, got)), name


def test_pinned_on_the_device(F):
    labels, words, info = F.frontier(K.PINNED, {}, K.PINNED_REF)
    want = np.array([[F.NONE if v is None else v for v in row] for row in K.PINNED_LABELS], np.uint32)
    assert np.array_equal(labels, want) and words.tolist() == K.PINNED_WORDS and info.tolist() == K.PINNED_INFO


def test_standalone_batch_equals_its_grids_one_by_one(F):
    labels, words, info = F.frontier(K.BATCH, K.BATCH_CFG, K.BATCH_REFS)
    assert labels.shape == K.BATCH.shape and info.shape == (3, 6) and len(words) == 3
    for b in range(3):
        want = F.frontier_np(K.BATCH[b], K.BATCH_CFG, K.BATCH_REFS[b])
        _equal((labels[b], words[b], info[b]), want, ("batch", b))
        _equal(F.frontier(K.BATCH[b], K.BATCH_CFG, K.BATCH_REFS[b]), want, ("one", b))
    assert info[0].tolist() == [0] * 6 and len({int(i[5]) for i in info}) == 3


def test_standalone_refusals(F):
    g = np.zeros((4, 4), np.int8)
    with pytest.raises(ValueError, match="pp_frontier_grids: refs: grid 0: the reference cell"):
        F.frontier(g, {}, (0, (1 << 20) + 1))
    L = F._lib.lib()
    refs = np.zeros((1, 2), np.int32)
    for field, bad in (("free_max", 100), ("connectivity", 6), ("min_size", 0), ("max_frontiers", 65), ("rank", 2), ("use_field", 2)):
        pc = F._lib.PPFrontierConfig(**dict(F.FrontierConfig().to_dict(), **{field: bad}))
        assert L.pp_frontier_grids(0, g.ctypes.data, None, 1, 4, 4, ctypes.byref(pc), refs.ctypes.data, None, None, None) == 1
        assert field in L.pp_last_error(None).decode()
    pc = F._lib.PPFrontierConfig(**F.FrontierConfig(use_field=1).to_dict())
    assert L.pp_frontier_grids(0, g.ctypes.data, None, 1, 4, 4, ctypes.byref(pc), refs.ctypes.data, None, None, None) == 1
    assert "pot is NULL" in L.pp_last_error(None).decode()


# ---- 2. on the handle ----
S3 = 3
OCC = dict(resolution=0.1, z_min=0.0, z_max=1.0, max_range=2.5, width=37, height=29)       # rows of 40 cells on the device
OCC_INFL = dict(inscribed_radius=0.1, inflation_radius=0.3, cost_scaling_factor=4.0, lethal_threshold=65)
NAV = dict(max_path=512)
SENSOR = np.array([[OCC["width"] // 2, OCC["height"] // 2]] * S3, np.int32)


def _tiny(pp, batch):
    return pp.config.tiny_config(batch)


def _poses(pp, k):
    return np.stack([pp.sweeps.pose_from_xyyaw(0.1 * s + 0.05 * k, -0.05 * s, 0.2 * s) for s in range(S3)])


def _update(pp, engines, k):
    frames = [K.room_points(40 + s + 10 * k) for s in range(S3)]
    for x in engines:
        x.upload(frames)
        x.occupancy_update_async(_poses(pp, k))


def _want(pp, grids, cfg, refs, navcfg=None):
    out = []
    for b in range(len(grids)):
        pot = pp.navfn.navfn_np(grids[b], SENSOR[b], navcfg) if cfg.use_field else None
        out.append(pp.frontier.frontier_np(grids[b], cfg, refs[b], pot))
    return out


def _same_run(pp, e, source, grids, cfg, refs, what, navcfg=None):
    fr, info, labels = e.frontiers(source, labels=True)
    want = _want(pp, grids, cfg, refs, navcfg)
    for b, (wl, ww, wi) in enumerate(want):
        assert np.array_equal(labels[b], wl), (what, b)
        assert [int(info[k][b]) for k in pp.frontier.INFO] == wi.tolist(), (what, b, wi.tolist())
        f = fr[b]
        got = np.stack([f["x"], f["y"], f["cx"], f["cy"], f["n"], f["label"].astype(np.int64)], axis=1).astype(np.int64)
        assert np.array_equal(got, ww[:, :6].astype(np.int64)), (what, b)
        assert f["cost"].tolist() == pp.frontier.cost_of(ww), (what, b)
    return fr, info, labels


def test_occupancy_source(pp, F, hip_lib):
    plain_e = pp.Engine(_tiny(pp, S3), max_batch=S3, max_points_per_frame=4096)
    e = pp.Engine(_tiny(pp, S3), max_batch=S3, max_points_per_frame=4096)
    try:
        for x in (plain_e, e):
            x.set_occupancy(OCC)
            x.set_inflation(OCC_INFL, "occupancy")
            x.set_navfn(NAV, "occupancy")
        assert e.frontier_config("occupancy") is None
        e.set_frontier(dict(min_size=2), "occupancy")
        cfg = e.frontier_config("occupancy")
        assert cfg == F.FrontierConfig(min_size=2) and e.frontier_config("costmap") is None
        for k in range(2):                                                 # the window moves
            _update(pp, (plain_e, e), k)
            G = _poses(pp, k)[:, :2, 3] + np.array([[0.6, 0.3], [-0.5, 0.4], [0.3, -0.5]])
            e.inflate_async("occupancy")
            e.frontier_async("occupancy")
            infl = e._inflated(1, None, False)[0]
            fr, info, _ = _same_run(pp, e, "occupancy", infl, cfg, SENSOR, ("occupancy", k))
            print("occupancy source:", k, {key: v.tolist() for key, v in info.items()})
            assert (info["returned"] > 0).all()
            paths, states = e.plan(G, "occupancy")
            paths0, states0 = plain_e.plan(G, "occupancy")
            # the maps, the inflated grids, the fields and the paths are what they are without the stage
            assert e._inflated(1, None, False)[0].tobytes() == plain_e._inflated(1, None, False)[0].tobytes() == infl.tobytes(), k
            assert all(a.tobytes() == b.tobytes() for a, b in zip(e.occupancy_maps(logodds=True), plain_e.occupancy_maps(logodds=True))), k
            assert e.navfn_fields("occupancy").tobytes() == plain_e.navfn_fields("occupancy").tobytes(), k
            assert np.array_equal(states, states0) and all(np.array_equal(a, b) for a, b in zip(paths, paths0)), k
        # other configurations on the same grids: 4-connected, the largest first, few returned
        for other in (dict(connectivity=4, min_size=1, max_frontiers=5), dict(rank=1, min_size=1), dict(free_max=20, min_size=4)):
            e.set_frontier(other, "occupancy")
            e.frontier_async("occupancy", refs=np.array([[0, 0], [36, 28], [-5, 40]], np.int32))
            _same_run(pp, e, "occupancy", infl, e.frontier_config("occupancy"), [[0, 0], [36, 28], [-5, 40]], other)
        # a stream reset before the inflation reads all unknown and returns nothing
        e.set_frontier(dict(min_size=1), "occupancy")
        e.occupancy_reset(1)
        e.inflate_async("occupancy")
        e.frontier_async("occupancy")
        fr, info, labels = e.frontiers("occupancy", labels=True)
        assert len(fr[1]) == 0 and [int(info[k][1]) for k in F.INFO] == [0] * 6 and (labels[1] == F.NONE).all()
        assert info["returned"][0] > 0 and info["returned"][2] > 0
        _same_run(pp, e, "occupancy", e._inflated(1, None, False)[0], e.frontier_config("occupancy"), SENSOR, "reset")
    finally:
        plain_e.close()
        e.close()


def test_use_field_settles_the_field_first(pp, F, hip_lib):
    e = pp.Engine(_tiny(pp, S3), max_batch=S3, max_points_per_frame=4096)
    try:
        e.set_occupancy(OCC)
        e.set_inflation(OCC_INFL, "occupancy")
        e.set_navfn(dict(NAV, queued_rounds=1), "occupancy")               # one round: the field is far from standing
        e.set_frontier(dict(use_field=1, min_size=2), "occupancy")
        cfg, navcfg = e.frontier_config("occupancy"), e.navfn_config("occupancy")
        _update(pp, (e,), 0)
        goals = e.explore("occupancy")                                     # inflation, navfn from the sensor's cells, the stage
        infl = e._inflated(1, None, False)[0]
        fr, info, _ = _same_run(pp, e, "occupancy", infl, cfg, SENSOR, "use_field", navcfg)
        print("use_field:", {key: v.tolist() for key, v in info.items()}, e.navfn_info("occupancy")["rounds"].tolist())
        assert (e.navfn_info("occupancy")["rounds"] > 1).all()            # the getter's continuation ran
        assert (info["returned"] > 0).all()
        org, res = e._infl_run[1][2], OCC["resolution"]
        for b in range(S3):
            assert goals[b] is not None and goals[b].dtype == np.float64
            cells = np.stack([fr[b]["x"], fr[b]["y"]], axis=1)
            assert np.array_equal(goals[b], F.cells_to_metres(cells, org[b], res)), b
        # explore -> plan: every stream's best goal is reached
        paths, states = e.plan(np.stack([g[0] for g in goals]), "occupancy")
        assert states.tolist() == [0] * S3 and all(len(p) > 1 for p in paths)
        for b in range(S3):
            assert np.allclose(paths[b][-1], goals[b][0], rtol=0, atol=1e-12), b
        # the plan replaced the field: the ranking would have to run again on another field, and is refused
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_frontiers: a pp_navfn_async of the occupancy source came after"):
            e.frontiers("occupancy")
        # metres=True follows the inflation's record across a set_occupancy at another resolution
        e.set_frontier(dict(min_size=2), "occupancy")
        e.frontier_async("occupancy")
        before, _ = e.frontiers("occupancy", metres=True)
        cells, _ = e.frontiers("occupancy")
        e.set_occupancy(dict(OCC, resolution=0.2))
        after, _ = e.frontiers("occupancy", metres=True)
        for b in range(S3):
            assert after[b].tobytes() == before[b].tobytes() and len(after[b]) > 0, b
            xy = F.cells_to_metres(np.stack([cells[b]["x"], cells[b]["y"]], axis=1), org[b], res)
            assert np.array_equal(np.stack([after[b]["x"], after[b]["y"]], axis=1), xy), b
            cxy = F.cells_to_metres(np.stack([cells[b]["cx"], cells[b]["cy"]], axis=1), org[b], res)
            assert np.array_equal(np.stack([after[b]["cx"], after[b]["cy"]], axis=1), cxy), b
    finally:
        e.close()


B = 2
CM = dict(x_min=-0.1, y_min=-0.7, resolution=0.05, width=37, height=29, z_min=-0.2, z_max=0.2)
CM_INFL = dict(resolution=0.05, inscribed_radius=0.05, inflation_radius=0.1, cost_scaling_factor=8.0)


def _cm_frames():
    out = []
    for b in range(B):
        rng = np.random.default_rng(300 + b)
        out.append(rng.uniform([0.05, -0.6, -2.5], [1.3, 0.6, 2.5], (700 + 150 * b, 3)).astype(np.float32))
    return out


def test_costmap_source_and_refusals(pp, F, hip_lib):
    plain_e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    try:
        state, arg = "PP_ERR_STATE.*pp_frontier_async: ", "PP_ERR_ARG.*pp_frontier_async: "
        refs = np.array([[2, 14], [30, 3]], np.int32)

        def call(source=0, r=refs, batch=B):
            e._check(e._lib.pp_frontier_async(e._h, source, None if r is None else r.ctypes.data, batch), "pp_frontier_async")

        for x in (plain_e, e):
            x.set_costmap(CM)
        # the stage off; the inflation off; no inflation run
        with pytest.raises(RuntimeError, match="frontier_async: no inflation has run on the costmap source"):
            e.frontier_async("costmap")
        with pytest.raises(RuntimeError, match=state + "the frontier stage of the costmap source is not configured"):
            call()
        e.set_frontier(dict(min_size=1, max_frontiers=64), "costmap")
        with pytest.raises(RuntimeError, match=state + "the inflation of the costmap source is not configured"):
            call()
        for x in (plain_e, e):
            x.set_inflation(CM_INFL, "costmap")
        with pytest.raises(RuntimeError, match=state + "no inflation has run on this source"):
            call()
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_frontiers: no frontier stage has run"):
            e._check(e._lib.pp_get_frontiers(e._h, 0, None, None, None, B), "pp_get_frontiers")
        frames = _cm_frames()
        for x in (plain_e, e):
            x.upload(frames)
        infl0, grids0 = plain_e.inflated_costmaps(), plain_e.costmaps()
        infl = e.inflated_costmaps()
        cfg = e.frontier_config("costmap")
        e.frontier_async("costmap", refs=refs)
        last = _same_run(pp, e, "costmap", infl, cfg, refs, "costmap")
        print("costmap source:", {key: v.tolist() for key, v in last[1].items()})
        assert (last[1]["clusters"] > 0).all()
        assert infl.tobytes() == infl0.tobytes() and e.costmaps().tobytes() == grids0.tobytes()
        assert e._inflated(0, None, False)[0].tobytes() == infl0.tobytes()
        e.frontier_async("costmap")                                        # the sensor's own cell
        sensor = pp.navfn.goal_cells(np.zeros((B, 2)), (CM["x_min"], CM["y_min"]), CM["resolution"], (CM["height"], CM["width"]))
        last = _same_run(pp, e, "costmap", infl, cfg, sensor, "sensor")

        def unchanged():
            fr, info, labels = e.frontiers("costmap", labels=True)
            assert labels.tobytes() == last[2].tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(fr, last[0]))
            assert all(np.array_equal(info[k], v) for k, v in last[1].items())

        # every refusal leaves the last results as they were
        with pytest.raises(RuntimeError, match=arg + "source = 2"):
            call(source=2)
        with pytest.raises(RuntimeError, match=arg + "refs is NULL"):
            call(r=None)
        with pytest.raises(RuntimeError, match=arg + "the last inflation had 2 grids, batch is 1"):
            call(batch=1)
        for bad in ([[0, 0], [(1 << 20) + 1, 0]], [[0, -(1 << 20) - 1], [0, 0]]):
            with pytest.raises(RuntimeError, match=arg + "refs: grid [01]: the reference cell"):
                call(r=np.array(bad, np.int32))
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_get_frontiers: the last run had 2 grids, batch is 1"):
            e._check(e._lib.pp_get_frontiers(e._h, 0, None, None, None, 1), "pp_get_frontiers")
        with pytest.raises(RuntimeError, match=state + "the frontier stage of the occupancy source is not configured"):
            call(source=1)
        for field, bad in (("free_max", 100), ("connectivity", 5), ("min_size", 0), ("max_frontiers", 65), ("rank", -1), ("use_field", 2)):
            pc = pp._lib.PPFrontierConfig(**dict(F.FrontierConfig().to_dict(), **{field: bad}))
            with pytest.raises(RuntimeError, match=f"PP_ERR_ARG.*pp_set_frontier: {field} = "):
                e._check(e._lib.pp_set_frontier(e._h, 0, ctypes.byref(pc)), "pp_set_frontier")
        pc = pp._lib.PPFrontierConfig(**F.FrontierConfig().to_dict())
        pc.reserved[1] = 1
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_set_frontier: reserved"):
            e._check(e._lib.pp_set_frontier(e._h, 0, ctypes.byref(pc)), "pp_set_frontier")
        assert e.frontier_config("costmap") == cfg
        unchanged()
        # use_field: no field, then a stale one
        e.set_frontier(dict(min_size=1, max_frontiers=64, use_field=1), "costmap")
        with pytest.raises(RuntimeError, match=state + "no navigation function has run on this source"):
            call()
        e.set_navfn(dict(allow_unknown=1, lethal_cost=100), "costmap")
        e._navfn_cells_async(0, sensor, None)
        e.inflate_async("costmap")
        with pytest.raises(RuntimeError, match=state + "the inflated grids of the costmap source were re-made since its navigation function ran"):
            call()
        unchanged()
        e._navfn_cells_async(0, sensor, None)
        call()
        fcfg, navcfg = e.frontier_config("costmap"), e.navfn_config("costmap")
        fr, info, labels = e.frontiers("costmap", labels=True)
        for b in range(B):
            pot = pp.navfn.navfn_np(infl[b], sensor[b], navcfg)
            wl, ww, wi = F.frontier_np(infl[b], fcfg, refs[b], pot)
            assert np.array_equal(labels[b], wl) and [int(info[k][b]) for k in F.INFO] == wi.tolist(), b
            assert fr[b]["label"].tolist() == ww[:, 5].tolist() and fr[b]["cost"].tolist() == F.cost_of(ww), b
        # off: the call is refused, the results stay, the inflation goes on
        e.set_frontier(None, "costmap")
        assert e.frontier_config("costmap") is None
        with pytest.raises(RuntimeError, match=state + "the frontier stage of the costmap source is not configured"):
            call()
        with pytest.raises(RuntimeError, match="explore: the frontier stage of the costmap source is not configured"):
            e.explore("costmap")
        assert e.inflated_costmaps().tobytes() == infl0.tobytes()
    finally:
        plain_e.close()
        e.close()


def test_refusals_while_a_training_step_is_in_flight(pp, F, hip_lib):
    cfg = _tiny(pp, B)
    tr = pp.Trainer(cfg, pp.weights.init_weights(pp.config.Derived(cfg), seed=7), max_batch=B, max_points_per_frame=4096,
                    learning_rate=2e-4, weight_decay=1e-4)
    e = tr.engine
    try:
        e.set_costmap(CM)
        e.set_inflation(CM_INFL, "costmap")
        e.set_frontier(dict(min_size=1), "costmap")
        frames = _cm_frames()
        e.upload(frames)
        infl = e.inflated_costmaps()
        refs = np.array([[2, 14], [30, 3]], np.int32)
        e.frontier_async("costmap", refs=refs)
        last = _same_run(pp, e, "costmap", infl, e.frontier_config("costmap"), refs, "before the step")
        gts = [np.array([[0.8, 0.2 * b, 0.0, 0.6, 0.8, 1.73, 0.1]], np.float32) for b in range(B)]
        e.train_step_gt_async(tr.params.data_ptr(), tr.grads.data_ptr(), tr.state.data_ptr(), *e.pack_gt(gts))
        for call, what in ((lambda: e.set_frontier(dict(min_size=2), "costmap"), "pp_set_frontier"),
                           (lambda: e.set_frontier(None, "costmap"), "pp_set_frontier"),
                           (lambda: e.frontier_async("costmap", refs=refs), "pp_frontier_async"),
                           (lambda: e.frontiers("costmap"), "pp_get_frontiers")):
            with pytest.raises(RuntimeError, match=f"PP_ERR_STATE.*{what}: a training step is in flight"):
                call()
        assert np.isfinite(e.train_step_wait()["loss"])
        assert e.frontier_config("costmap") == F.FrontierConfig(min_size=1)
        fr, info, labels = e.frontiers("costmap", labels=True)
        assert labels.tobytes() == last[2].tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(fr, last[0]))
    finally:
        tr.close()
