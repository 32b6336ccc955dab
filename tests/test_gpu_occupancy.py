"""The rolling occupancy map on the GPU (csrc/occupancy.hip: k_occ_endpoints, k_occ_rays, k_occ_apply) against
occupancy.py's restatement, fed with the uploaded frames: grids, log-odds, origins and the info counts must be EQUAL
(np.array_equal).  No tolerances: the rule is integer arithmetic apart from one float64 transform per row (+ * / and floor,
the library is built without contraction), and the cost table comes from the host."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 3                    # streams of the shared engine
W, H = 37, 29            # neither a multiple of 4
CFG = dict(resolution=0.1, z_min=0.0, z_max=1.0, max_range=2.5, width=W, height=H)
INFO = ("hits", "ground", "ignored", "cells_hit", "cells_free", "cleared")


def _tiny(pp, B=S):
    return pp.config.tiny_config(B)


@pytest.fixture(scope="module")
def eng(pp, hip_lib):
    e = pp.Engine(_tiny(pp), max_batch=S, max_points_per_frame=4096)
    yield e
    e.close()


def _start(pp, eng, cfg=CFG, streams=S):
    """The stage on with `cfg`, every map forgotten; the restatement's maps next to it."""
    eng.set_occupancy(cfg)
    eng.occupancy_reset()
    return [pp.occupancy.OccupancyMap(cfg) for _ in range(streams)]


def _step(eng, maps, frames, poses, what=""):
    """One update of streams 0 .. len(frames) - 1 on both sides; everything the stage gives must equal the restatement."""
    B = len(frames)
    eng.upload(frames)
    eng.occupancy_update_async(poses)
    grid, org, lo = eng.occupancy_maps(logodds=True)
    info = eng.occupancy_info()
    want = [maps[b].update(frames[b], poses[b]) for b in range(B)]
    c = maps[0].cfg
    assert grid.dtype == np.int8 and lo.dtype == np.int16 and grid.shape == lo.shape == (B, c.height, c.width) and org.shape == (B, 2)
    for b in range(B):
        assert np.array_equal(lo[b], maps[b].logodds()), (what, b)
        assert np.array_equal(grid[b], maps[b].grid()), (what, b)
        assert np.array_equal(grid[b] != -1, maps[b].known()), (what, b)
        assert tuple(org[b]) == maps[b].origin, (what, b)
    for k in INFO:
        assert info[k].tolist() == [w[k] for w in want], (what, k)
    return grid, org, lo, want


def _edge_frame(n):
    """n rows for the pose at the origin: the host test's edge rows, 150 rows of one cell (longer than a wavefront, across
    a workgroup boundary of the endpoint kernel), short runs cell after cell, and seeded rows over and around the window."""
    rng = np.random.default_rng(11)
    r = CFG["resolution"]
    x_lo, x_hi = -(W // 2) * r, (W - W // 2) * r              # the window's edges in x for a pose at the origin
    y_lo, y_hi = -(H // 2) * r, (H - H // 2) * r
    f32 = np.float32
    edges = [[0.55, 0.05, 0.0], [0.65, 0.05, 1.0], [0.05, 0.55, np.nextafter(f32(1.0), f32(2.0))], [0.05, 0.65, -1e-6],
             [2.5, 0.0, 0.5], [0.0, np.nextafter(f32(2.5), f32(3.0)), 0.5], [0.02, 0.03, 0.5],
             [x_lo - 0.05, 0.0, 0.5], [x_hi + 0.05, 0.0, 0.5], [0.0, y_lo - 0.05, 0.5], [0.0, y_hi + 0.05, 0.5],
             [x_lo + 0.05, 0.0, 0.5], [x_hi - 0.05, 0.0, 0.5], [0.0, y_lo + 0.05, 0.5], [0.0, y_hi - 0.05, 0.5],
             [np.nan, 0.0, 0.5], [0.0, np.inf, 0.5], [-np.inf, 0.0, 0.5], [0.7, -0.2, np.nan], [0.7, -0.2, -np.inf],
             [1e30, 0.0, 0.5], [0.0, -1e30, 0.5]]
    body = rng.uniform([-2.2, -1.8, -0.5], [2.2, 1.8, 1.4], (n - len(edges) - 200, 3))
    run = np.tile([[1.01, 0.52, 0.2]], (150, 1))                 # 150 rows of one cell, every third a ground return
    run[::3, 2] = -0.3
    walk = np.stack([0.2 + 0.012 * np.arange(50), np.full(50, -0.33), np.full(50, 0.1)], 1)
    rows = np.concatenate([np.array(edges), body[:200], run, body[200:], walk])
    assert len(rows) == n
    return rows.astype(np.float32)


def test_edge_frame_empty_frame_and_one_row(pp, eng):
    maps = _start(pp, eng)
    assert eng.occupancy == pp.occupancy.OccupancyConfig(**CFG)
    frames = [np.zeros((0, 3), np.float32), np.array([[0.91, -0.43, 0.5]], np.float32), _edge_frame(1037)]
    assert len(frames[2]) > 2 * 256 and len(frames[2]) % 64
    poses = np.stack([pp.sweeps.pose_from_xyyaw(0.3, -0.2, 0.4), pp.sweeps.pose_from_xyyaw(-5.07, 2.01, 2.0),
                      pp.sweeps.pose_from_xyyaw(0.0, 0.0, 0.0)])
    grid, org, lo, want = _step(eng, maps, frames, poses, "edge")
    assert (grid[0] == -1).all() and want[0]["cleared"] == W * H
    assert want[1]["hits"] == 1 and want[1]["cells_free"] >= 6 and (lo[1] == 85).sum() == 1
    assert want[2]["ignored"] >= 12 and want[2]["ground"] >= 50 and want[2]["cells_hit"] >= 200 and want[2]["cells_free"] >= 200
    assert org[1].tolist() == [(-51 - W // 2) * 0.1, (20 - H // 2) * 0.1]            # floor, for a negative t as well
    # the same frames again: one more step on every marked cell, the same window
    g2, _, lo2, w2 = _step(eng, maps, frames, poses, "edge again")
    assert w2[2]["cleared"] == 0 and lo2[2].max() == 170 and lo2[2].min() == -82
    eng.set_occupancy(None)
    assert eng.occupancy is None


def _world():
    """Obstacle points in the fixed frame: walls beside the streams' paths and scattered returns, 0.2 .. 0.8 m high;
    below them a floor."""
    rng = np.random.default_rng(21)
    n = 6000
    walls = np.concatenate([
        np.stack([rng.uniform(-3, 8, n), np.full(n, 1.05), rng.uniform(0.2, 0.8, n)], 1),
        np.stack([rng.uniform(-3, 8, n), np.full(n, -0.95), rng.uniform(0.2, 0.8, n)], 1),
        np.stack([np.full(n, -0.85), rng.uniform(-8, 3, n), rng.uniform(0.2, 0.8, n)], 1),
    ])
    u = rng.uniform(-2, 5, n)
    diagonal = np.stack([u, 1.3 - 0.885 * u, rng.uniform(0.2, 0.8, n)], 1)          # beside stream 2's path
    scatter = np.stack([rng.uniform(-4, 9, n), rng.uniform(-9, 4, n), rng.uniform(0.2, 0.8, n)], 1)
    floor = np.stack([rng.uniform(-4, 9, 4 * n), rng.uniform(-9, 4, 4 * n), np.full(4 * n, -0.4)], 1)
    return np.concatenate([walls, diagonal, scatter, floor])


def _sequence(pp, steps=12, rows=700):
    """steps x (frames [S], poses [S, 3, 4]): every stream on a path of its own through one world; yaw 0.3 k, a
    translation that moves the window on most steps and carries it more than W cells, stream 2 with a small roll and pitch."""
    world = _world()
    rng = np.random.default_rng(22)
    out = []
    for k in range(steps):
        frames, poses = [], []
        for s in range(S):
            yaw = 0.3 * k + 0.5 * s
            t = [(0.37 * k, 0.013 * k, 0.0), (0.021 * k, -0.33 * k, 0.0), (0.26 * k - 0.4, -0.23 * k + 0.1, 0.02)][s]
            P = pp.sweeps.pose_from_xyyaw(t[0], t[1], yaw)
            if s == 2:
                cr, sr, cp, sp = math.cos(0.03), math.sin(0.03), math.cos(-0.02), math.sin(-0.02)
                Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
                Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
                T = np.eye(4)
                T[:3, :3] = P[:, :3] @ Ry @ Rx
                T[:3, 3] = t
                P = pp.sweeps.pose_from_matrix(T)
            local = (world - P[:, 3]) @ P[:, :3]                  # R^T (p - t)
            near = local[(np.abs(local[:, 0]) < 2.4) & (np.abs(local[:, 1]) < 2.0)]
            pick = near[rng.permutation(len(near))[:rows - 20 * s]]
            frames.append(pick.astype(np.float32))
            poses.append(P)
        out.append((frames, np.stack(poses)))
    return out


@pytest.fixture(scope="module")
def sequence(pp):
    return _sequence(pp)


def _play(pp, eng, sequence, what):
    maps = _start(pp, eng)
    used, hit, free, moved = [], [], [], 0
    for k, (frames, poses) in enumerate(sequence):
        before = [m.origin_cell for m in maps]
        grid, org, lo, want = _step(eng, maps, frames, poses, f"{what} step {k}")
        moved += sum(m.origin_cell != o for m, o in zip(maps, before))
        used += [w["hits"] + w["ground"] for w in want]
        hit += [w["cells_hit"] for w in want]
        free += [w["cells_free"] for w in want]
    return maps, grid, org, lo, dict(used=used, hit=hit, free=free, moved=moved)


def test_sequence_jump_small_batch_and_reset(pp, eng, sequence):
    maps, grid, org, lo, st = _play(pp, eng, sequence, "sequence")
    c = maps[0].cfg
    # the sequence does what it is for: rows are used, cells are hit and freed, the windows move and travel more than W
    # cells, and both clamps are reached
    print("used rows", min(st["used"]), max(st["used"]), "cells hit", min(st["hit"]), max(st["hit"]), "freed", min(st["free"]),
          max(st["free"]), "window moves", st["moved"])
    assert min(st["used"]) >= 200 and min(st["hit"]) >= 20 and min(st["free"]) >= 150
    assert st["moved"] >= 2 * S * (len(sequence) - 1) // 3
    assert abs(maps[0].origin_cell[0] - (0 - W // 2)) > W and abs(maps[1].origin_cell[1] - (0 - H // 2)) > H
    for b in range(S):
        assert (lo[b] == c.l_max).any() and (lo[b] == c.l_min).any(), b
    # a jump of more than W cells: nothing from before is known
    frames, poses = sequence[-1]
    far = poses.copy()
    far[:, 0, 3] += (W + 3) * 0.1
    g, _, l2, want = _step(eng, maps, frames, far, "jump")
    assert [w["cleared"] for w in want] == [W * H] * S
    assert np.abs(l2).max() <= c.l_hit                       # one step on an unknown window
    # a batch of 1: streams 1 and 2 stay as they are ...
    kept = [(maps[b].logodds(), maps[b].origin_cell) for b in (1, 2)]
    _step(eng, maps, frames[:1], far[:1], "batch of 1")
    # ... which the next batch of 3 shows: the same poses, so their windows do not move
    g3, o3, l3, want = _step(eng, maps, frames, far, "batch of 3 again")
    assert want[1]["cleared"] == 0 and maps[1].origin_cell == kept[0][1]
    assert (np.abs(l3[1]) > c.l_hit).any()                   # stream 1 took its second step only now
    # reset(1) clears stream 1 only; until its next update the stream reads unknown
    eng.occupancy_reset(1)
    maps[1].reset()
    gr, orr, lr = eng.occupancy_maps(logodds=True)
    assert (gr[1] == -1).all() and (lr[1] == 0).all() and np.isnan(orr[1]).all()
    assert gr[0].tobytes() == g3[0].tobytes() and gr[2].tobytes() == g3[2].tobytes() and np.array_equal(orr[[0, 2]], o3[[0, 2]])
    _, _, _, want = _step(eng, maps, frames, far, "after reset(1)")
    assert [w["cleared"] for w in want] == [0, W * H, 0]
    eng.set_occupancy(None)


def test_fresh_engine_replays_the_same_bytes_off_on_and_reconfigure(pp, hip_lib, eng, sequence):
    _, grid, org, lo, _ = _play(pp, eng, sequence[:6], "first")
    e = pp.Engine(_tiny(pp), max_batch=S, max_points_per_frame=4096)
    try:
        maps, g2, o2, l2, _ = _play(pp, e, sequence[:6], "replay")
        assert g2.tobytes() == grid.tobytes() and l2.tobytes() == lo.tobytes() and o2.tobytes() == org.tobytes()
        # off and on with the same configuration: the maps stay, and so do the last update's results
        e.set_occupancy(None)
        assert e.occupancy is None
        with pytest.raises(RuntimeError, match="not configured"):
            e.occupancy_update_async(sequence[6][1])
        e.set_occupancy(CFG)
        assert e.occupancy_maps()[0].tobytes() == grid.tobytes()
        _step(e, maps, *sequence[6], "after off / on")
        # z_max changes under the maps
        e.set_occupancy(dict(CFG, z_max=0.5))
        for m in maps:
            m.cfg = pp.occupancy.OccupancyConfig(**dict(CFG, z_max=0.5))
        _, _, _, want = _step(e, maps, *sequence[7], "z_max changed")
        assert all(w["cleared"] < W * H for w in want)
        # a changed width forgets them
        wide = dict(CFG, width=40)
        e.set_occupancy(wide)
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no update has run"):
            e.occupancy_maps()
        maps = [pp.occupancy.OccupancyMap(wide) for _ in range(S)]
        g, _, _, want = _step(e, maps, *sequence[8], "width 40")
        assert g.shape == (S, H, 40) and [w["cleared"] for w in want] == [40 * H] * S
        # and so does a changed step
        e.set_occupancy(dict(wide, l_hit=60))
        maps = [pp.occupancy.OccupancyMap(dict(wide, l_hit=60)) for _ in range(S)]
        _, _, l, want = _step(e, maps, *sequence[9], "l_hit 60")
        assert [w["cleared"] for w in want] == [40 * H] * S and l.max() == 60
        # a one-cell window, a width that is a multiple of 4, rows shorter than a quad
        for shape in (dict(width=1, height=1), dict(width=52, height=3), dict(width=3, height=50)):
            c = dict(CFG, **shape)
            e.set_occupancy(c)
            maps = [pp.occupancy.OccupancyMap(c) for _ in range(S)]
            for k in (0, 1, 2):
                _step(e, maps, *sequence[k], f"{shape} step {k}")
    finally:
        e.close()


def _weights(pp, d, seed=7):
    w = dict(pp.weights.init_weights(d, seed=seed))
    w["rpn/conv_cls/bias"] = np.array(w["rpn/conv_cls/bias"], np.float32) + np.float32(0.6)
    return w


def test_the_stage_changes_nothing_of_a_pass_or_a_costmap(pp, hip_lib):
    B = 2
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=4096)
    try:
        e.load_weights(_weights(pp, e.d))
        rect, trv, _ = pp.synth.default_calib()
        rect, trv = np.stack([rect] * B), np.stack([trv] * B)
        frames = []
        for b in range(B):
            rng = np.random.default_rng(300 + b)
            frames.append(rng.uniform([0.05, -0.6, -2.5], [1.3, 0.6, 2.5], (700 + 150 * b, 3)).astype(np.float32))
        cm = dict(x_min=-0.5, y_min=-1.0, resolution=0.05, width=51, height=43, z_min=-1.0, z_max=1.0)
        e.set_costmap(cm)
        dets, n = e.detect(frames, rect, trv)
        plain = (dets.tobytes(), n.tobytes(), e.costmaps().tobytes())
        assert int(n.sum()) >= 2
        e.set_occupancy(dict(CFG, z_min=-1.0))
        maps = [pp.occupancy.OccupancyMap(dict(CFG, z_min=-1.0)) for _ in range(B)]
        poses = np.stack([pp.sweeps.pose_from_xyyaw(0.1 * b, 0.2, 0.3) for b in range(B)])
        dets, n = e.detect(frames, rect, trv)
        assert (dets.tobytes(), n.tobytes(), e.costmaps().tobytes()) == plain      # configured, not yet run
        # behind a pass, in front of the costmap stage: every output is what it was, and the maps are the restatement's
        e.detect_async()
        e.occupancy_update_async(poses)
        e.costmap_async()
        got = (e.detections()[0].tobytes(), e.detections()[1].tobytes(), e.costmaps().tobytes())
        assert got == plain
        grid, org, lo = e.occupancy_maps(logodds=True)
        for b in range(B):
            maps[b].update(frames[b], poses[b])
            assert np.array_equal(grid[b], maps[b].grid()) and np.array_equal(lo[b], maps[b].logodds()) and tuple(org[b]) == maps[b].origin
        assert (grid != -1).sum() > 100
    finally:
        e.close()


def test_refusals_leave_the_handle_usable(pp, hip_lib):
    e = pp.Engine(_tiny(pp), max_batch=S, max_points_per_frame=4096)
    try:
        L, h = e._lib, e._h
        frames = [np.array([[0.5, 0.1 * b, 0.5]], np.float32) for b in range(S)]
        poses = np.stack([pp.sweeps.pose_from_xyyaw(0.0, 0.0, 0.1 * b) for b in range(S)])
        pptr = poses.ctypes.data_as(ctypes.c_void_p)
        g = np.zeros((S, H, W), np.int8)
        o = np.zeros((S, 2))
        gp, op = g.ctypes.data_as(ctypes.c_void_p), o.ctypes.data_as(ctypes.c_void_p)
        # the stage off
        with pytest.raises(RuntimeError, match="not configured"):
            e.occupancy_update_async(poses)
        assert L.pp_occupancy_update_async(h, pptr, S) == 2 and b"not configured" in L.pp_last_error(h)
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no update has run"):
            e.occupancy_maps()
        assert L.pp_occupancy_info(h, None, None, None, None, None, None, S) == 2
        assert L.pp_occupancy_reset(h, S) == 1 and L.pp_occupancy_reset(h, -2) == 1 and L.pp_occupancy_reset(h, -1) == 0
        e.set_occupancy(CFG)
        # nothing resident
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no frames are resident"):
            e.occupancy_update_async(poses)
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no update has run"):
            e.occupancy_maps()
        e.upload(frames)
        # poses: not orthonormal, not finite, too far, too many, too few, a wrong shape
        bad = poses.copy()
        bad[1, 0, 0] += 1e-3
        with pytest.raises(ValueError, match="stream 1 is not orthonormal"):
            e.occupancy_update_async(bad)
        assert L.pp_occupancy_update_async(h, bad.ctypes.data_as(ctypes.c_void_p), S) == 1 and b"stream 1 is not orthonormal" in L.pp_last_error(h)
        bad = poses.copy()
        bad[2, 1, 3] = np.nan
        with pytest.raises(ValueError, match="stream 2 is not finite"):
            e.occupancy_update_async(bad)
        assert L.pp_occupancy_update_async(h, bad.ctypes.data_as(ctypes.c_void_p), S) == 1 and b"not finite" in L.pp_last_error(h)
        bad = poses.copy()
        bad[0, 0, 3] = 0.11 * 2 ** 30
        with pytest.raises(ValueError, match="2\\^30"):
            e.occupancy_update_async(bad)
        assert L.pp_occupancy_update_async(h, bad.ctypes.data_as(ctypes.c_void_p), S) == 1 and b"2^30" in L.pp_last_error(h)
        with pytest.raises(ValueError, match="4 poses, the engine has 3 streams"):
            e.occupancy_update_async(np.concatenate([poses, poses[:1]]))
        four = np.concatenate([poses, poses[:1]])
        assert L.pp_occupancy_update_async(h, four.ctypes.data_as(ctypes.c_void_p), S + 1) == 1
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*3 frames are resident, batch is 2"):
            e.occupancy_update_async(poses[:2])
        with pytest.raises(ValueError, match="poses"):
            e.occupancy_update_async(poses[0])
        assert L.pp_occupancy_update_async(h, None, S) == 1 and b"poses is NULL" in L.pp_last_error(h)
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no update has run"):      # none of these queued anything
            e.occupancy_maps()
        # the C side validates a configuration on its own, naming the field; the one in force stays
        for field, value in (("resolution", 0.0), ("resolution", float("nan")), ("max_range", 0.0), ("max_range", float("inf")),
                             ("z_min", float("nan")), ("z_min", 2.0), ("width", 0), ("height", 0), ("width", 1 << 20),
                             ("l_hit", 0), ("l_hit", 1001), ("l_miss", 0), ("l_min", 0), ("l_min", -1001), ("l_max", 0), ("l_max", 1001)):
            pc = pp._lib.PPOccupancyConfig()
            for f, v in pp.occupancy.OccupancyConfig(**CFG).to_dict().items():
                setattr(pc, f, v)
            setattr(pc, field, value)
            assert L.pp_set_occupancy(h, ctypes.byref(pc), None, 0) == 1, field
            assert field.encode() in L.pp_last_error(h), (field, L.pp_last_error(h))
        pc = pp._lib.PPOccupancyConfig()
        for f, v in pp.occupancy.OccupancyConfig(**CFG).to_dict().items():
            setattr(pc, f, v)
        table = pp.occupancy.cost_table(CFG)
        tp = table.ctypes.data_as(ctypes.c_void_p)
        assert L.pp_set_occupancy(h, ctypes.byref(pc), tp, len(table) - 1) == 1 and b"cost_table has 550 entries" in L.pp_last_error(h)
        worse = table.copy()
        worse[7] = 101
        assert L.pp_set_occupancy(h, ctypes.byref(pc), worse.ctypes.data_as(ctypes.c_void_p), len(table)) == 1
        assert b"cost_table[7]" in L.pp_last_error(h)
        assert e.occupancy == pp.occupancy.OccupancyConfig(**CFG)
        # the handle works: an update, then the fetch's own refusals
        maps = [pp.occupancy.OccupancyMap(CFG) for _ in range(S)]
        _step(e, maps, frames, poses, "after the refusals")
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*the last update had 3 streams, batch is 2"):
            e.occupancy_maps(batch=2)
        assert L.pp_get_occupancy(h, None, None, op, S) == 1 and b"grid is NULL" in L.pp_last_error(h)
        assert L.pp_get_occupancy(h, gp, None, None, S) == 1 and b"origins is NULL" in L.pp_last_error(h)
        assert L.pp_occupancy_info(h, None, None, None, None, None, None, 1) == 1
        # the table the library computes itself when none is given is the host's
        assert L.pp_set_occupancy(h, ctypes.byref(pc), None, 0) == 0
        _step(e, maps, frames, poses, "the library's table")
        assert L.pp_get_occupancy(h, gp, None, op, S) == 0
        assert all(np.array_equal(g[b], maps[b].grid()) for b in range(S))
    finally:
        e.close()
