"""Obstacle inflation on the GPU (csrc/inflate.hip: k_inflate) against inflation.py's restatement: grids, clearance maps
and counts must be EQUAL (np.array_equal).  No tolerances: the device works in integers and looks the cost up in the
table the host computed.  Stand-alone on the shared cases (tests/inflation_cases.py), then behind the costmap stage and
behind the rolling occupancy maps, whose own outputs must stay the bytes of an engine that never heard of inflation."""
import ctypes

import numpy as np
import pytest

import inflation_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def I(pp, hip_lib):
    return pp.inflation


def _same(got, want, what):
    out, d2, info = got
    wout, wd2, winfo = want
    assert out.dtype == np.int8 and d2.dtype == np.uint16
    assert np.array_equal(d2, wd2), what
    assert np.array_equal(out, wout), what
    assert {k: np.asarray(v).tolist() for k, v in info.items()} == winfo, what


# ---- 1. stand-alone ----
@pytest.mark.parametrize("name", K.NAMES)
def test_standalone_equals_the_restatement(I, name):
    _, g, cfg = K.case(name)
    want = I.inflate_np(g, cfg, clearance=True, info=True)
    got = I.inflate(g, cfg, clearance=True, info=True)
    _same(got, want, name)
    again = I.inflate(g, cfg, clearance=True, info=True)                   # the same bytes on every run
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    assert {k: int(v) for k, v in again[2].items()} == want[2]
    assert np.array_equal(I.inflate(g, cfg), want[0])                      # without the clearance map


def test_standalone_batch_equals_its_batch_one_results(I):
    out, d2, info = I.inflate(K.BATCH, K.BATCH_CFG, clearance=True, info=True)
    assert out.shape == d2.shape == K.BATCH.shape and info["lethal"].shape == (3,)
    for b in range(3):
        one = I.inflate(K.BATCH[b], K.BATCH_CFG, clearance=True, info=True)
        want = I.inflate_np(K.BATCH[b], K.BATCH_CFG, clearance=True, info=True)
        _same(one, want, b)
        _same((out[b], d2[b], {k: v[b] for k, v in info.items()}), want, b)
    assert len({out[b].tobytes() for b in range(3)}) == 3


def test_standalone_largest_window(I):
    """PP_OCC_MAX_CELLS cells in one grid: 16 x 32 tiles, every index of the last rows past 2^20 - 1024."""
    g = K.random_grid(21, 1024, 1024, p_obstacle=0.002)
    g[-1, -1] = g[0, 0] = 100
    cfg = K.cfg(3)
    _same(I.inflate(g, cfg, clearance=True, info=True), I.inflate_np(g, cfg, clearance=True, info=True), "1024 x 1024")


# ---- 2. behind the costmap stage ----
B = 2
GRIDS = {"37x29": dict(x_min=-0.1, y_min=-0.7, resolution=0.05, width=37, height=29, z_min=-0.2, z_max=0.2),
         "200x200": dict(x_min=-0.2, y_min=-1.0, resolution=0.01, width=200, height=200, z_min=-3.0, z_max=3.0)}
# the resolution given, and left to the source's (0.0)
INFL = {"37x29": dict(resolution=0.05, inscribed_radius=0.05, inflation_radius=0.2, cost_scaling_factor=8.0),
        "200x200": dict(inscribed_radius=0.02, inflation_radius=0.1, cost_scaling_factor=20.0, unknown_min_cost=50)}


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
    """Two engines on the same weights: the first never sets inflation."""
    es = []
    for _ in range(2):
        e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
        e.load_weights(_weights(pp, e.d))
        es.append(e)
    yield es
    for e in es:
        e.close()


@pytest.mark.parametrize("shape", list(GRIDS))
def test_costmap_source(pp, I, pair, shape):
    plain_e, e = pair
    rect, trv, _ = pp.synth.default_calib()
    rect, trv = np.stack([rect] * B), np.stack([trv] * B)
    frames = _frames(B)
    cm = GRIDS[shape]
    plain_e.set_costmap(cm)
    dets0, n0 = plain_e.detect(frames, rect, trv)
    grids0 = plain_e.costmaps()
    assert int(n0.sum()) >= 2

    e.set_costmap(cm)
    e.set_inflation(INFL[shape], "costmap")
    c = e.inflation_config("costmap")
    assert c == I.InflationConfig(**dict(INFL[shape], resolution=cm["resolution"]))
    assert e.inflation_config("occupancy") is None
    dets, n = e.detect(frames, rect, trv)
    e.set_profiling(True)
    infl, d2 = e.inflated_costmaps(clearance=True)
    times = e.kernel_times()
    e.set_profiling(False)
    assert [k for k, _ in times] == ["k_inflate"]                         # one launch, whatever the batch
    info = e.inflation_info("costmap")
    grids = e.costmaps()
    # the pass and the costmap are what they are without the stage
    assert (dets.tobytes(), n.tobytes()) == (dets0.tobytes(), n0.tobytes())
    assert grids.tobytes() == grids0.tobytes()
    d1, n1 = e.detections()
    assert (d1.tobytes(), n1.tobytes()) == (dets0.tobytes(), n0.tobytes())
    assert infl.shape == d2.shape == (B, cm["height"], cm["width"]) and infl.dtype == np.int8 and d2.dtype == np.uint16
    for b in range(B):
        want = I.inflate_np(grids[b], c, clearance=True, info=True)
        _same((infl[b], d2[b], {k: v[b] for k, v in info.items()}), want, (shape, b))
        assert want[2]["lethal"] >= 20 and want[2]["raised"] > want[2]["lethal"]
    assert not np.array_equal(infl[0], infl[1])
    # without the clearance map, and through the explicit calls
    e.costmap_async()
    e.inflate_async("costmap")
    assert e._inflated(0, None, False)[0].tobytes() == infl.tobytes()
    assert e.inflated_costmaps().tobytes() == infl.tobytes()
    # off: the buffers stay, the call is refused, the source goes on
    e.set_inflation(None, "costmap")
    assert e.inflation_config("costmap") is None
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_inflate_async: the inflation of the costmap source is not configured"):
        e.inflated_costmaps()
    assert e.costmaps().tobytes() == grids0.tobytes()
    e.set_costmap(None)
    plain_e.set_costmap(None)


# ---- 3. behind the rolling occupancy maps ----
S = 3
OCC = dict(resolution=0.1, z_min=0.0, z_max=1.0, max_range=2.5, width=37, height=29)       # rows of 40 cells on the device
OCC_INFL = dict(inscribed_radius=0.1, inflation_radius=0.5, cost_scaling_factor=4.0, lethal_threshold=65)


def _occ_frames(k):
    out = []
    for s in range(S):
        rng = np.random.default_rng(40 + 10 * k + s)
        out.append(rng.uniform([-2.0, -1.6, -0.5], [2.0, 1.6, 1.2], (300 + 37 * s, 3)).astype(np.float32))
    return out


def test_occupancy_source(pp, I, hip_lib):
    plain_e = pp.Engine(_tiny(pp, S), max_batch=S, max_points_per_frame=4096)
    e = pp.Engine(_tiny(pp, S), max_batch=S, max_points_per_frame=4096)
    try:
        for x in (plain_e, e):
            x.set_occupancy(OCC)
        e.set_inflation(OCC_INFL, "occupancy")
        c = e.inflation_config("occupancy")
        assert c.resolution == 0.1 and I.radius_cells(c) == 5
        seen = set()
        for k in range(3):                                                 # the window moves; the streams' copies alternate
            frames = _occ_frames(k)
            poses = np.stack([pp.sweeps.pose_from_xyyaw(0.23 * k + 0.1 * s, -0.17 * k * (s - 1), 0.3 * k + 0.5 * s) for s in range(S)])
            for x in (plain_e, e):
                x.upload(frames)
                x.occupancy_update_async(poses)
            infl, org_i, d2 = e.inflated_occupancy_maps(clearance=True)
            info = e.inflation_info("occupancy")
            grid, org, lo = e.occupancy_maps(logodds=True)
            grid0, org0, lo0 = plain_e.occupancy_maps(logodds=True)
            assert (grid.tobytes(), org.tobytes(), lo.tobytes()) == (grid0.tobytes(), org0.tobytes(), lo0.tobytes()), k
            for key, v in plain_e.occupancy_info().items():
                assert np.array_equal(e.occupancy_info()[key], v), (k, key)
            assert org_i.tobytes() == org.tobytes(), k
            for s in range(S):
                want = I.inflate_np(grid[s], c, clearance=True, info=True)
                _same((infl[s], d2[s], {key: v[s] for key, v in info.items()}), want, (k, s))
                assert want[2]["lethal"] >= 10 and want[2]["raised"] >= 10
            seen.add(infl.tobytes())
        assert len(seen) == 3
        # a reset stream reads all unknown, with a NaN origin; the others stay
        e.occupancy_reset(1)
        infl2, org2, d22 = e.inflated_occupancy_maps(clearance=True)
        info2 = e.inflation_info("occupancy")
        assert (infl2[1] == -1).all() and (d22[1] == 26).all() and np.isnan(org2[1]).all()
        assert info2["lethal"][1] == 0 and info2["raised"][1] == 0
        for s in (0, 2):
            assert infl2[s].tobytes() == infl[s].tobytes() and org2[s].tobytes() == org[s].tobytes()
            assert info2["lethal"][s] == info["lethal"][s]
        g1, o1 = e.occupancy_maps()
        assert (g1[1] == -1).all() and np.isnan(o1[1]).all() and o1.tobytes() == org2.tobytes()
        e.occupancy_reset()
        e.inflate_async("occupancy")
        infl3, org3 = e.inflated_occupancy_maps()
        assert (infl3 == -1).all() and np.isnan(org3).all()
        assert not e.inflation_info("occupancy")["raised"].any()
    finally:
        plain_e.close()
        e.close()


# ---- 4. refusals: nothing is launched, nothing changes ----
def test_refusals(pp, I, hip_lib):
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    try:
        cm = GRIDS["37x29"]
        cfg = INFL["37x29"]
        state = "PP_ERR_STATE.*pp_inflate_async: "
        # neither configured
        with pytest.raises(RuntimeError, match=state + "the inflation of the occupancy source is not configured"):
            e.inflate_async("occupancy")
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_inflated: no inflation has run"):
            e._inflated(0, 1, False)
        # the source off: resolution 0.0 has nothing to stand for, and an explicit one is kept but cannot run
        with pytest.raises(RuntimeError, match="set_inflation: resolution = 0.0 stands for the costmap stage's"):
            e.set_inflation(True, "costmap")
        assert e.inflation_config("costmap") is None
        e.set_inflation(cfg, "costmap")
        with pytest.raises(RuntimeError, match=state + "the costmap stage is not configured"):
            e.inflate_async("costmap")
        # the source on, no run yet
        e.set_costmap(cm)
        with pytest.raises(RuntimeError, match=state + "no costmap stage has run"):
            e.inflate_async("costmap")
        e.set_occupancy(OCC)
        e.set_inflation(OCC_INFL, "occupancy")
        with pytest.raises(RuntimeError, match=state + "no update has run"):
            e.inflate_async("occupancy")
        # a run, then the refusals that must leave it as it is
        frames = _frames(B, seed=500)
        e.upload(frames)
        e.set_profiling(True)
        infl, d2 = e.inflated_costmaps(clearance=True)
        launched = e.kernel_times()
        assert [k for k, _ in launched] == ["k_inflate"]
        info = e.inflation_info("costmap")

        def unchanged():
            g, d = e._inflated(0, None, True)
            assert (g.tobytes(), d.tobytes()) == (infl.tobytes(), d2.tobytes())
            assert all(np.array_equal(e.inflation_info("costmap")[k], info[k]) for k in info)
            assert e.inflation_config("costmap") == I.InflationConfig(**cfg)

        # the batch is the run's
        with pytest.raises(ValueError, match="inflated_costmaps: the source's run has 2 grids, batch is 1"):
            e.inflated_costmaps(batch=1)
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_get_inflated: the last run had 2 grids, batch is 1"):
            e._inflated(0, 1, True)
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_inflation_info: the last run had 2 grids, batch is 1"):
            e._check(e._lib.pp_inflation_info(e._h, 0, None, None, 1), "pp_inflation_info")
        # a table of another length, a source that does not exist
        pc = pp._lib.PPInflationConfig(**cfg, lethal_threshold=100, unknown_min_cost=1)
        table = I.cost_table(cfg)
        assert len(table) == 17
        with pytest.raises(RuntimeError, match=r"PP_ERR_ARG.*pp_set_inflation: table has 16 entries, R \* R \+ 1 = 17"):
            e._check(e._lib.pp_set_inflation(e._h, 0, ctypes.byref(pc), table.ctypes.data, 16), "pp_set_inflation")
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_inflate_async: source = 2"):
            e._check(e._lib.pp_inflate_async(e._h, 2), "pp_inflate_async")
        # the occupancy source still has no update behind it
        with pytest.raises(RuntimeError, match=state + "no update has run"):
            e.inflate_async("occupancy")
        assert e.kernel_times() == launched                                # a stage that queues anything starts the list anew
        e.set_profiling(False)
        unchanged()
        plain = e.costmaps()
        # the source reconfigured to another resolution, the same shape: the table was built for 0.05
        e.set_costmap(dict(cm, resolution=0.1))
        e.costmap_async()
        with pytest.raises(RuntimeError, match=state + "the costmap stage has resolution = 0.1, the inflation table was built for 0.05"):
            e.inflate_async("costmap")
        e.costmaps()
        e.set_costmap(cm)
        assert e.costmaps().tobytes() == plain.tobytes()
        unchanged()
        # and the occupancy source likewise
        e.occupancy_update_async(np.stack([pp.sweeps.pose_from_xyyaw(0.0, 0.0, 0.0)] * B))
        first = e.inflated_occupancy_maps()[0]
        e.set_occupancy(dict(OCC, resolution=0.2))
        with pytest.raises(RuntimeError, match=state + "the occupancy stage has resolution = 0.2, the inflation table was built for 0.1"):
            e.inflate_async("occupancy")
        assert e._inflated(1, None, False)[0].tobytes() == first.tobytes()
    finally:
        e.close()
