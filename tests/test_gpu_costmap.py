"""The costmap stage on the GPU (csrc/costmap.hip: k_costmap_objects, k_costmap_points, k_costmap_compose) against
costmap.py's restatement: grids and count taps must be EQUAL (np.array_equal).  The rule is float64 + - * /, floor and
comparisons, and the library is built without contraction; only the cos / sin of a footprint's yaw may differ in the last
place between the two, so cells whose centre lies within 1e-9 m of a footprint's edge (costmap.decision_margins) are left
out -- none in the hand-made geometries (asserted), at most 0.1 % of the cells in the seeded 64-track case.  The restatement
is fed with what the engine itself reports: the uploaded points, detections() and tracks()."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 3          # streams of the shared engine
MARGIN = 1e-9  # metres: under it a cell's membership is undecided
# the tiny model's range is x 0 .. 1.6, y -0.64 .. 0.64: a grid of 51 x 43 = 2193 cells around it (a width that is no multiple of 4)
GRID = dict(x_min=-0.5, y_min=-1.0, resolution=0.05, width=51, height=43, z_min=-1.0, z_max=1.0)


def _tiny(pp, B=S, ncls=1, **second):
    cfg = pp.config.tiny_config(B)
    cfg["model"]["second"]["num_class"] = ncls
    cfg["model"]["second"].update(second)
    return cfg


@pytest.fixture(scope="module")
def eng(pp, hip_lib):
    e = pp.Engine(_tiny(pp), max_batch=S, max_points_per_frame=4096)
    yield e
    e.close()


def _want(pp, frames, cfg, dets=None, n=None, tracks=None, nt=None):
    """The restatement per frame -> (grids [B, H, W], counts [B, H, W], undecided [B, H, W] bool)."""
    C = pp.costmap
    c = C.CostmapConfig.from_any(cfg)
    G, K, U = [], [], []
    for b, f in enumerate(frames):
        kw = {}
        if c.objects == 1:
            kw = dict(dets=dets[b], n_dets=int(n[b]))
        elif c.objects == 2:
            kw = dict(tracks=tracks[b], n_tracks=int(nt[b]))
        g, k = C.costmap_np(f, c, **kw)
        G.append(g)
        K.append(k)
        U.append(C.decision_margins(c, C.footprints_np(c, **kw)) < MARGIN if c.objects else np.zeros(g.shape, bool))
    return np.stack(G), np.stack(K), np.stack(U)


def _in_grid(frames, c):
    out = []
    for f in frames:
        fx, fy = (f[:, 0].astype(np.float64) - c["x_min"]) / c["resolution"], (f[:, 1].astype(np.float64) - c["y_min"]) / c["resolution"]
        with np.errstate(invalid="ignore"):
            out.append(int(((fx >= 0) & (fx < c["width"]) & (fy >= 0) & (fy < c["height"])).sum()))
    return out


def _edge_frame(n):
    """n rows: the edge cases of the host test, runs of rows in one cell (one longer than a wavefront, across a workgroup
    boundary of the point kernel), and seeded rows over and around the grid."""
    rng = np.random.default_rng(11)
    x0, y0, r = GRID["x_min"], GRID["y_min"], GRID["resolution"]
    edges = [[x0, y0, 0.0], [x0 + 3 * r, y0 + 2 * r, -1.0], [x0 + 3 * r, y0 + 2 * r, 1.0], [x0 + 51 * r, 0.0, 0.0],
             [0.0, y0 + 43 * r, 0.0], [np.float32(x0) - np.float32(1e-6), 0.0, 0.0], [0.3, 0.3, 1.5], [0.3, 0.3, -1.5],
             [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [-np.inf, 0.0, 0.0], [0.7, -0.2, np.nan], [1e30, 0.0, 0.0], [0.0, -1e30, 0.0]]
    body = rng.uniform([-0.7, -1.2, -1.4], [2.3, 1.3, 1.4], (n - len(edges) - 200, 3))
    run = np.tile([[1.01, 0.52, 0.2]], (150, 1))                 # 150 rows of one cell, every third outside the z range
    run[::3, 2] = 1.3
    walk = np.stack([0.2 + 0.012 * np.arange(50), np.full(50, -0.33), np.full(50, 0.1)], 1)   # short runs, cell after cell
    rows = np.concatenate([np.array(edges), body[:200], run, body[200:], walk])
    assert len(rows) == n
    return rows.astype(np.float32)


# ---- 1. the point layer ----
def test_points_only(pp, eng):
    eng.set_costmap(dict(GRID, min_points=2, point_cost=80))
    assert eng.costmap == pp.costmap.CostmapConfig(**dict(GRID, min_points=2, point_cost=80))
    frames = [np.zeros((0, 3), np.float32), np.array([[0.21, 0.13, 0.0]], np.float32), _edge_frame(1037)]
    assert len(frames[2]) > 2 * 256 and len(frames[2]) % 64
    eng.upload(frames)
    grid, counts = eng.costmaps(counts=True)
    wg, wk, _ = _want(pp, frames, eng.costmap)
    assert grid.dtype == np.int8 and grid.shape == (3, 43, 51) and counts.dtype == np.int32
    assert np.array_equal(counts, wk) and np.array_equal(grid, wg)
    assert (grid[0] == -1).all() and (grid[1] != -1).sum() == 1 and counts[2].max() >= 100 and (grid[2] == 80).any() and (grid[2] == 0).any()
    info = eng.costmap_info()
    assert info["points_in_grid"].tolist() == _in_grid(frames, GRID) and info["footprints"].tolist() == [0, 0, 0]
    # the same bytes on a second call
    g2, k2 = eng.costmaps(counts=True)
    assert g2.tobytes() == grid.tobytes() and k2.tobytes() == counts.tobytes()
    # a smaller batch after a larger one: the count words were cleared -- what a fresh engine gives
    small = [frames[2][::2]]
    eng.upload(small)
    g1, k1 = eng.costmaps(counts=True)
    assert g1.shape == (1, 43, 51)
    fresh = pp.Engine(_tiny(pp), max_batch=S, max_points_per_frame=4096)
    try:
        fresh.set_costmap(eng.costmap)
        fresh.upload(small)
        gf, kf = fresh.costmaps(counts=True)
    finally:
        fresh.close()
    assert g1.tobytes() == gf.tobytes() and k1.tobytes() == kf.tobytes()
    wg, wk, _ = _want(pp, small, eng.costmap)
    assert np.array_equal(k1, wk) and np.array_equal(g1, wg)
    # a width that IS a multiple of 4, a one-cell grid, rows shorter than a quad
    e4 = pp.Engine(_tiny(pp, 1), max_batch=1, max_points_per_frame=4096)
    try:
        for shape in (dict(width=52, height=3), dict(width=1, height=1), dict(width=3, height=50)):
            c = dict(GRID, **shape)
            e4.set_costmap(c)
            e4.upload([frames[2]])
            g, k = e4.costmaps(counts=True)
            wg, wk, _ = _want(pp, [frames[2]], c)
            assert np.array_equal(k, wk) and np.array_equal(g, wg), shape
    finally:
        e4.close()
    eng.set_costmap(None)
    assert eng.costmap is None


# ---- 2. tracks ----
def _rows(per_stream, rows):
    """per_stream: per stream a list of (x, y, w, l, yaw, score) -> (dets [streams, rows], n)."""
    import pp_amd
    d = np.zeros((len(per_stream), rows), pp_amd.Engine.det_dtype())
    n = np.zeros(len(per_stream), np.int32)
    for s, rr in enumerate(per_stream):
        n[s] = len(rr)
        for i, r in enumerate(rr):
            d["box3d_lidar"][s, i] = (r[0], r[1], 0.0, r[2], r[3], 1.6, r[4])
            d["score"][s, i] = r[5]
    return d, n


def _track_cfg(pp):
    return pp.tracking.TrackConfig(gate=1.25, birth_score=0.3, max_misses=2, min_hits=2, q_acc=4.0, r_pos=0.01)


def _compare(pp, eng, frames, cfg, cap, what, **kw):
    grid, counts = eng.costmaps(counts=True)
    wg, wk, und = _want(pp, frames, cfg, **kw)
    left_out = int(und.sum())
    print(f"{what}: {left_out} of {und.size} cells undecided (cap {cap})")
    assert left_out <= cap, what
    assert np.array_equal(counts, wk), what
    assert np.array_equal(grid[~und], wg[~und]), what
    return grid


def test_tracks_footprints_and_horizons(pp, eng):
    eng.set_tracking(_track_cfg(pp))
    eng.set_tracking(None)                    # the stage needs the configuration, not the switch
    eng.track_reset()
    frames = [np.zeros((0, 3), np.float32), np.array([[0.4, 0.1, 0.0]], np.float32), _edge_frame(600)]
    eng.upload(frames)
    # stream 0: a yawed box in the grid, one partly outside (across the lower x edge), one wholly outside
    # stream 1: a box that moves 0.1 m per step in x and y; stream 2: two boxes, the second appears at the last step only
    base = [[(0.63, 0.11, 0.31, 0.52, 0.4, 0.9), (-0.47, -0.31, 0.33, 0.61, -1.2, 0.9), (4.0, 4.0, 0.4, 0.4, 0.3, 0.9)],
            [(0.2, -0.7, 0.23, 0.37, 2.1, 0.9)],
            [(1.11, 0.43, 0.21, 0.27, 0.77, 0.9)]]
    for step in range(3):
        per = [list(base[0]), [(0.2 + 0.1 * step, -0.7 + 0.1 * step, 0.23, 0.37, 2.1, 0.9)], list(base[2])]
        if step == 2:
            per[2].append((1.31, -0.53, 0.19, 0.33, -0.5, 0.9))
        tr, nt, _ = eng.track_update(*_rows(per, 8), [0.1] * S)
    assert nt.tolist() == [3, 1, 2] and tr["confirmed"][2, :2].tolist() == [1, 0] and tr["state"][1, 0, 3] > 0
    before = (tr.tobytes(), nt.tobytes())
    grids = {}
    for steps in (0, 1, 8):
        cfg = dict(GRID, objects="tracks", horizon_steps=steps, horizon_dt=0.2, object_cost=90,
                   predict_cost=[70, 60, 50, 40, 30, 20, 10, 5][:max(steps, 1)])
        eng.set_costmap(cfg)
        grids[steps] = _compare(pp, eng, frames, cfg, 0, f"tracks, horizon {steps}", tracks=tr, nt=nt)
        assert eng.costmap_info()["footprints"].tolist() == [3 * (1 + steps), 1 + steps, 2 * (1 + steps)]
    assert (grids[0][0] == 90).sum() > 20 and (grids[0][0, :, 0] == 90).any()        # the partly-outside box reaches column 0
    assert np.array_equal(grids[8] == 90, grids[0] == 90)                             # the current footprints alone at step 0
    assert (grids[1][1] == 70).any() and not (grids[0][1] == 70).any() and (grids[8][1] == 60).any()
    # confirmed_only drops stream 2's new track; pad widens
    cfg = dict(GRID, objects="tracks", confirmed_only=True, pad=0.07)
    eng.set_costmap(cfg)
    g = _compare(pp, eng, frames, cfg, 0, "confirmed_only, pad", tracks=tr, nt=nt)
    assert eng.costmap_info()["footprints"].tolist() == [3, 1, 1] and (g[0] == 100).sum() > (grids[0][0] == 90).sum()
    # nothing else moved: the tables are what they were
    t2, n2, _ = eng.tracks()
    assert (t2.tobytes(), n2.tobytes()) == before
    eng.set_costmap(None)


def test_64_live_tracks_seeded(pp, eng):
    """64 live tracks per stream from seeded rows, moved once so they carry velocities; 64 x 9 footprints per frame (ten
    LDS tiles of the compose kernel, three passes of the objects kernel's compaction)."""
    eng.set_tracking(_track_cfg(pp))
    eng.set_tracking(None)
    eng.track_reset()
    rng = np.random.default_rng(5)
    big = dict(x_min=-10.0, y_min=-10.0, resolution=0.25, width=79, height=81, z_min=-1.0, z_max=1.0)
    gx, gy = np.meshgrid(np.arange(8), np.arange(8))
    centres = np.stack([gx.ravel() * 2.6 - 9.3, gy.ravel() * 2.7 - 9.6], 1) + rng.uniform(-0.3, 0.3, (64, 2))   # beyond each other's gate
    per = [[(x, y, *rng.uniform(0.4, 1.6, 2), rng.uniform(-3.1, 3.1), 0.9) for x, y in centres] for _ in range(S)]
    frames = [rng.uniform([-11, -11, -1.5], [11, 11, 1.5], (900 + 77 * b, 3)).astype(np.float32) for b in range(S)]
    eng.upload(frames)
    eng.track_update(*_rows(per, 64), [0.1] * S)
    moved = [[(r[0] + 0.08, r[1] - 0.05) + r[2:] for r in rr] for rr in per]
    tr, nt, _ = eng.track_update(*_rows(moved, 64), [0.1] * S)
    assert nt.tolist() == [64] * S and (tr["confirmed"] == 1).all() and np.abs(tr["state"][..., 3]).min() > 0
    cfg = dict(big, objects="tracks", horizon_steps=8, horizon_dt=0.5, object_cost=100)
    eng.set_costmap(cfg)
    cap = int(0.001 * S * 79 * 81)
    g = _compare(pp, eng, frames, cfg, cap, "64 tracks", tracks=tr, nt=nt)
    assert eng.costmap_info()["footprints"].tolist() == [64 * 9] * S
    assert {100, 90, 20} <= set(np.unique(g).tolist())
    eng.set_costmap(None)


@pytest.mark.parametrize("name", ["w300", "w257"])
def test_wide_grids_waves_inside_one_row(pp, eng, name):
    """More than 64 quads a row (300 and 257 cells wide): waves of k_costmap_compose that lie inside one row and start past
    column 0 cull a tile's records by their columns as well (tests/test_costmap_host.py restates which waves).  24 tracks
    with velocities, 24 and 72 footprints (more than one LDS tile), 1 500 seeded rows a frame; no cell is left out."""
    import grid_shape_cases as gc
    eng.set_tracking(gc.wide_track_config())
    eng.set_tracking(None)
    eng.track_reset()
    per = [gc.wide_track_rows(name, s) for s in range(S)]
    frames = gc.wide_frames(name)
    eng.upload(frames)
    eng.track_update(*gc.wide_det_rows(per), [0.1] * S)
    tr, nt, _ = eng.track_update(*gc.wide_det_rows([gc.wide_moved(rr) for rr in per]), [0.1] * S)
    assert nt.tolist() == [24] * S and np.abs(tr["state"][:, :24, 3]).min() > 0
    W = gc.WIDE_COSTMAPS[name]["width"]
    for steps in (0, 2):
        cfg = gc.wide_costmap_config(name, steps, (GRID["z_min"], GRID["z_max"]))
        eng.set_costmap(cfg)
        g = _compare(pp, eng, frames, cfg, 0, f"{name}, horizon {steps}", tracks=tr, nt=nt)
        assert g.shape == (S, gc.WIDE_COSTMAPS[name]["height"], W)
        assert eng.costmap_info()["footprints"].tolist() == [24 * (1 + steps)] * S
        vals = set(np.unique(g).tolist())
        assert 100 in vals and ({70, 60} <= vals) == (steps == 2)
        assert (g[:, :, 256:] >= 60).any() and (g[:, :, :4] >= 60).any()
    eng.set_costmap(None)


# ---- 3. detections behind a pass, the stage's ordering, what it must leave alone ----
def _weights(pp, d, seed=7):
    w = dict(pp.weights.init_weights(d, seed=seed))
    w["rpn/conv_cls/bias"] = np.array(w["rpn/conv_cls/bias"], np.float32) + np.float32(0.6)
    return w


def _frames(B, shift=0.0):
    """The seeded clouds for which the CPU oracle (oracle/, through tests/util_ref.oracle_detect) keeps 9 + 9 rows in the
    joint mode and 10 + 12 with two classes per class on the weights above."""
    out = []
    for b in range(B):
        rng = np.random.default_rng(300 + b)
        pts = rng.uniform([0.05, -0.6, -2.5], [1.3, 0.6, 2.5], (700 + 150 * b, 3))
        pts[:, 0] += shift
        out.append(pts.astype(np.float32))
    return out


def _calib(pp, B):
    rect, trv, _ = pp.synth.default_calib()
    return np.stack([rect] * B), np.stack([trv] * B)


@pytest.mark.parametrize("mode", ["joint", "per_class"])
def test_detections_behind_a_pass(pp, hip_lib, mode):
    B = 2
    second = dict(use_multi_class_nms=True) if mode == "per_class" else {}
    e = pp.Engine(_tiny(pp, B, 2 if mode == "per_class" else 1, **second), max_batch=B, max_points_per_frame=4096)
    try:
        e.load_weights(_weights(pp, e.d))
        rect, trv = _calib(pp, B)
        frames = _frames(B)
        # the stage never set: costmap_async refuses and the pass is what it is
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_costmap_async: the costmap stage is not configured"):
            e.costmap_async()
        dets, n = e.detect(frames, rect, trv)
        plain = (dets.tobytes(), n.tobytes())
        assert int(n.sum()) >= 2, n                      # the oracle's count on the CPU: 18 (joint), 22 (per class)
        cfg = dict(GRID, z_min=-3.0, z_max=3.0, objects="detections", min_score=float(np.median(dets["score"][0, :n[0]])),
                   object_cost=95, point_cost=40)
        e.set_costmap(cfg)
        dets, n = e.detect(frames, rect, trv)
        assert (dets.tobytes(), n.tobytes()) == plain    # a configured stage changes nothing of a pass
        grid = _compare(pp, e, frames, cfg, 0, f"detections, {mode}", dets=dets, n=n)
        fp = e.costmap_info()["footprints"]
        assert 1 <= fp[0] < n[0] and (grid == 95).any() and (grid == 40).any()
        # nothing else moved: the results are the same bytes after the stage, and a replay on the resident frames gives them again
        d2, n2 = e.detections()
        assert (d2.tobytes(), n2.tobytes()) == plain
        e.detect_async()
        d3, n3 = e.detections()
        assert (d3.tobytes(), n3.tobytes()) == plain
        assert e.costmaps().tobytes() == grid.tobytes()
        # ordering: the stage queued behind pass 1 reads pass 1's rows and frames, whatever is queued behind it
        other = _frames(B, shift=0.2)
        st = e.staging(other)
        e.upload(frames)
        e.set_calib(rect, trv, B)
        e.detect_async()
        e.costmap_async()
        e.upload_async(st)
        e.detect_async()
        got = e.costmaps()
        assert got.tobytes() == grid.tobytes()
        d4, n4 = e.detections()                          # ... and the second pass ran on the other frames
        assert d4.tobytes() != plain[0]
        g4 = _compare(pp, e, other, cfg, 0, f"second pass, {mode}", dets=d4, n=n4)
        assert g4.tobytes() != grid.tobytes()
    finally:
        e.close()


def test_flagged_frame_takes_no_objects(pp, hip_lib):
    B = 2
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    try:
        bad = _weights(pp, e.d)
        bad["rpn/deconv2/bn/beta"] = bad["rpn/deconv2/bn/beta"] + np.float32(1e5)     # the head GEMM's operand leaves float16's range
        e.load_weights(bad)
        cfg = dict(GRID, z_min=-3.0, z_max=3.0, objects="detections")
        e.set_costmap(cfg)
        frames = _frames(B)
        e.upload(frames, *_calib(pp, B))
        e.detect_async()
        with pytest.raises(pp.NumericError, match="pp_get_costmaps"):
            e.costmaps()
        # the grids were written all the same: the point layer alone
        grid = np.zeros((B, 43, 51), np.int8)
        assert e._lib.pp_get_costmaps(e._h, grid.ctypes.data_as(ctypes.c_void_p), None, B) == 6      # PP_ERR_NUMERIC
        wg, _, _ = _want(pp, frames, dict(cfg, objects="none"))
        assert np.array_equal(grid, wg) and e.costmap_info()["footprints"].tolist() == [0, 0]
    finally:
        e.close()


# ---- 4. refusals ----
def test_refusals_leave_the_handle_usable(pp, hip_lib):
    e = pp.Engine(_tiny(pp, 2), max_batch=2, max_points_per_frame=4096)
    try:
        L, h = e._lib, e._h
        frames = _frames(2)
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*not configured"):
            e.costmaps()
        g = np.zeros((2, 43, 51), np.int8)
        gp = g.ctypes.data_as(ctypes.c_void_p)
        assert L.pp_get_costmaps(h, gp, None, 2) == 2 and b"no costmap stage has run" in L.pp_last_error(h)
        assert L.pp_costmap_info(h, None, None, 2) == 2
        e.set_costmap(GRID)
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no frames are resident"):
            e.costmap_async()
        e.upload(frames, *_calib(pp, 2))
        e.set_costmap(dict(GRID, objects="detections"))
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no pass has run on the resident frames"):
            e.costmap_async()
        e.load_weights(_weights(pp, e.d))
        e.detect_async()
        e.costmaps()
        e.upload(frames)                                  # new frames: the last pass's rows are not theirs
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no pass has run on the resident frames"):
            e.costmap_async()
        e.set_costmap(dict(GRID, objects="tracks"))
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_set_tracking has given no configuration"):
            e.costmap_async()
        e.set_costmap(GRID)
        grid = e.costmaps()
        assert L.pp_get_costmaps(h, gp, None, 1) == 1 and b"the last run had 2 frames, batch is 1" in L.pp_last_error(h)
        assert L.pp_get_costmaps(h, None, None, 2) == 1 and b"grid is NULL" in L.pp_last_error(h)
        assert L.pp_costmap_info(h, None, None, 1) == 1
        # the C side validates a configuration on its own, naming the field; the one in force stays
        for field, value in (("resolution", 0.0), ("resolution", float("nan")), ("pad", -1.0), ("horizon_dt", 0.0),
                             ("x_min", float("inf")), ("z_min", float("nan")), ("width", 0), ("height", 0), ("width", 1 << 20),
                             ("min_points", 0), ("objects", 3), ("horizon_steps", 9), ("point_cost", 101), ("object_cost", -1)):
            pc = pp._lib.PPCostmapConfig()
            for f, v in pp.costmap.CostmapConfig(**GRID).to_dict().items():
                if f != "predict_cost":
                    setattr(pc, f, v)
            setattr(pc, field, value)
            assert L.pp_set_costmap(h, ctypes.byref(pc)) == 1, field
            assert field.encode() in L.pp_last_error(h), (field, L.pp_last_error(h))
        pc = pp._lib.PPCostmapConfig()
        for f, v in pp.costmap.CostmapConfig(**dict(GRID, horizon_steps=2)).to_dict().items():
            if f != "predict_cost":
                setattr(pc, f, v)
        pc.predict_cost[1] = 101
        assert L.pp_set_costmap(h, ctypes.byref(pc)) == 1 and b"predict_cost[1]" in L.pp_last_error(h)
        pc.z_min, pc.z_max, pc.predict_cost[1] = 1.0, 0.0, 5
        assert L.pp_set_costmap(h, ctypes.byref(pc)) == 1 and b"z_min" in L.pp_last_error(h)
        assert e.costmap == pp.costmap.CostmapConfig(**GRID)
        assert e.costmaps().tobytes() == grid.tobytes()
        wg, _, _ = _want(pp, frames, GRID)
        assert np.array_equal(grid, wg)
    finally:
        e.close()


def test_refusals_while_a_training_step_is_in_flight(pp, hip_lib):
    B = 2
    cfg = _tiny(pp, B)
    tr = pp.Trainer(cfg, pp.weights.init_weights(pp.config.Derived(cfg), seed=7), max_batch=B, max_points_per_frame=4096,
                    learning_rate=2e-4, weight_decay=1e-4)
    e = tr.engine
    try:
        e.set_costmap(GRID)
        frames = _frames(B)
        e.upload(frames)
        grid = e.costmaps()
        gts = [np.array([[0.8, 0.2 * b, 0.0, 0.6, 0.8, 1.73, 0.1]], np.float32) for b in range(B)]
        e.train_step_gt_async(tr.params.data_ptr(), tr.grads.data_ptr(), tr.state.data_ptr(), *e.pack_gt(gts))
        for call, what in ((lambda: e.set_costmap(dict(GRID, pad=0.1)), "pp_set_costmap"), (lambda: e.set_costmap(None), "pp_set_costmap"),
                           (lambda: e.costmap_async(), "pp_costmap_async")):
            with pytest.raises(RuntimeError, match=f"PP_ERR_STATE.*{what}: a training step is in flight"):
                call()
        assert np.isfinite(e.train_step_wait()["loss"])
        assert e.costmap == pp.costmap.CostmapConfig(**GRID)
        e.upload(frames)
        assert e.costmaps().tobytes() == grid.tobytes()
    finally:
        tr.close()


def test_config_key_and_voxelnet(pp, hip_lib):
    cfg = _tiny(pp, 1, costmap=dict(GRID, point_cost=33))
    net = pp.VoxelNet(cfg, max_batch=1, max_points_per_frame=4096)
    try:
        assert net.engine.costmap == pp.costmap.CostmapConfig(**dict(GRID, point_cost=33))
        frames = _frames(1)
        net.engine.upload(frames)
        g = net.costmaps()
        wg, _, _ = _want(pp, frames, dict(GRID, point_cost=33))
        assert np.array_equal(g, wg) and (g == 33).any()
        msg = pp.costmap.to_occupancy_grid(g[0], net.engine.costmap, stamp=1.0, frame_id="lidar")
        assert msg["info"]["width"] == 51 and len(msg["data"]) == 43 * 51
    finally:
        net.engine.close()
