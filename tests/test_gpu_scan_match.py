"""The scan match on the GPU (csrc/scan_match.hip: k_scan_cells, k_scan_scores, k_scan_finish) against scan_match.py's
restatement: all eight words and every candidate's score must be EQUAL.  No tolerances: apart from one float64 rotation
per row (+ * / and floor, the library is built without contraction) and the sensor's sub-cells (float64 on the host on both
sides) the rule is integer arithmetic."""
import ctypes

import numpy as np
import pytest

import scan_match_cases as K

pytestmark = pytest.mark.gpu

OFF_RING = 4            # csrc/pp_ring.h
LDS_CHUNK = 1024        # csrc/scan_match.hip: SCAN_CHUNK
TILE = 64               # csrc/pp_common.h: SCAN_TILE
S = 2                   # streams of the shared engine
SCALE = 0.4             # the room of the host test shrunk to fit a small window
OCC = dict(resolution=0.1, z_min=0.0, z_max=2.0, max_range=8.0, width=101, height=77)
SCAN = dict(nx=3, ny=3, nt=3, xy_step=1024, theta_step=8, min_cells=20, min_mean=0)
ROWS = 1500


def _same(SM, occ, scan, L, Kn, points, poses, origins, words, scores, what):
    """Stream by stream: the GPU's words and scores against match_grid_np."""
    for b in range(len(points)):
        w, s = SM.match_grid_np(occ, L[b], Kn[b], origins[b], points[b], poses[b], scan)
        assert np.array_equal(scores[b], s), (what, b, int((scores[b] != s).sum()))
        assert words[b].tolist() == w.tolist(), (what, b)
    return True


# ---- through pp_scan_match_grids: the smallest shapes at which the kernels can go wrong ----
@pytest.fixture(scope="module")
def cases(pp):
    return {c["name"]: c for c in K.grid_cases(pp) + [K.tie_case(pp)]}


@pytest.mark.parametrize("name", ["long-list-285-translations", "empty-and-one-row", "one-translation-many-headings", "one-heading",
                                  "no-map-outside-and-matched", "near-the-edge", "ties"])
def test_stand_alone_equals_the_restatement(pp, hip_lib, cases, name):
    SM = pp.scan_match
    c = cases[name]
    cfg = SM.ScanMatchConfig.from_any(c["scan"])
    words, scores = SM.scan_match_grids(c["L"], c["K"], c["points"], c["poses"], c["origins"], c["occ"], cfg)
    assert words.shape == (len(c["points"]), 8) and scores.shape == (len(c["points"]), cfg.candidates) and scores.dtype == np.int32
    _same(SM, c["occ"], cfg, c["L"], c["K"], c["points"], c["poses"], c["origins"], words, scores, name)
    n_trans = (2 * cfg.nx + 1) * (2 * cfg.ny + 1)
    st = words[:, 0]
    # every case is what its name says
    if name == "long-list-285-translations":
        assert words[0, 6] > 3 * LDS_CHUNK and words[0, 6] % LDS_CHUNK and n_trans == 285 and n_trans % TILE and words[0, 7] > 1000
        assert c["occ"].width % 4 and len(set(scores[0].tolist())) > 500
    elif name == "empty-and-one-row":
        assert words[:, 6].tolist() == [0, 1] and st[0] == SM.FEW_CELLS and not st[1] & SM.FEW_CELLS and not scores[0].any() and scores[1].any()
    elif name == "one-translation-many-headings":
        dh = (np.arange(41) - 20) * 100
        assert n_trans == 1 and dh.min() < -1024 and len(set((dh & 4095).tolist())) == 41 and len(set(scores[0].tolist())) > 20
    elif name == "one-heading":
        assert cfg.nt == 0 and n_trans == 143 and c["occ"].width == 15 and c["occ"].height == 50
    elif name == "no-map-outside-and-matched":
        assert st[0] == SM.NO_MAP and st[1] == SM.OUTSIDE and not st[2] & 3 and not scores[:2].any() and scores[2].any()
        assert len(set(words[:, 6].tolist())) == 3 and words[:, 6].min() > 100
    elif name == "near-the-edge":
        # candidates leave the window: the far corner's candidates keep fewer cells inside than the prior does
        assert not (st & 3).any() and (scores == 0).any() and c["occ"].width == 15 and c["occ"].height == 11
    else:
        top = scores[0].max()
        assert (scores[0] == top).sum() > 10 and words[0].tolist()[:5] == [0, 0, 0, 0, int(top)]


def test_stand_alone_refusals(pp, hip_lib, cases):
    SM = pp.scan_match
    c = cases["ties"]
    bad = c["poses"].copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(ValueError):
        SM.scan_match_grids(c["L"], c["K"], c["points"], bad, c["origins"], c["occ"], c["scan"])
    far = c["poses"].copy()
    far[0, 0, 3] = 0.1 * 2.0 ** 30
    with pytest.raises(RuntimeError, match="2\\^30 cells"):
        SM.scan_match_grids(c["L"], c["K"], c["points"], far, c["origins"], c["occ"], c["scan"])


# ---- through the Engine ----
@pytest.fixture(scope="module")
def eng(pp, hip_lib):
    e = pp.Engine(pp.config.tiny_config(S), max_batch=S, max_points_per_frame=4096)
    yield e
    e.close()


def _truth(b, k):
    """Stream b's true pose (x, y, yaw) at step k: a slow drive through the room."""
    return (0.3 * b - 0.2 + 0.04 * k, -0.2 * b + 0.03 * k, 0.5 - 1.1 * b + 0.015 * k)


def _frames(pp, k, seed=0):
    """(frames [S], true poses [S, 3, 4]) of step k."""
    rng = np.random.default_rng(5000 + 10 * k + seed)
    poses = np.stack([K.yaw_pose(pp, *_truth(b, k)) for b in range(S)])
    frames = [K.sensor_frame(K.room_returns(rng, ROWS + 100 * b, SCALE), poses[b], rng) for b in range(S)]
    return frames, poses


def _prior(pp, b, k, steps):
    x, y, yaw = _truth(b, k)
    return K.yaw_pose(pp, x - 0.1 * steps[0], y - 0.1 * steps[1], yaw - steps[2] * 8 * K.TICK)


def _start(pp, eng, occ=OCC, scan=SCAN):
    eng.set_occupancy(occ)
    eng.occupancy_reset()
    eng.set_scan_match(scan)
    return [pp.occupancy.OccupancyMap(occ) for _ in range(S)]


def _build(pp, eng, maps, steps=5):
    for k in range(steps):
        frames, poses = _frames(pp, k)
        eng.upload(frames)
        eng.occupancy_update_async(poses)
        for b in range(S):
            maps[b].update(frames[b], poses[b])


def _maps_equal(eng, maps, what):
    grid, org, lo = eng.occupancy_maps(logodds=True)
    for b in range(S):
        assert np.array_equal(lo[b], maps[b].logodds()) and np.array_equal(grid[b], maps[b].grid()), (what, b)
        assert tuple(org[b]) == maps[b].origin, (what, b)
    return grid, org, lo


def test_engine_match_under_a_displaced_prior(pp, eng):
    SM = pp.scan_match
    maps = _start(pp, eng)
    assert eng.scan_match == SM.ScanMatchConfig(**SCAN)
    _build(pp, eng, maps)
    before = _maps_equal(eng, maps, "built")
    frames, _ = _frames(pp, 5)
    priors = np.stack([_prior(pp, 0, 5, (2, -1, 1)), _prior(pp, 1, 5, (-1, 2, -2))])
    eng.upload(frames)
    eng.scan_match_async(priors)
    words, scores = eng.scan_match_results(scores=True)
    assert words.shape == (S, 8) and scores.shape == (S, 343)
    for b in range(S):
        w, s = SM.match_np(maps[b], frames[b], priors[b], SCAN)
        assert np.array_equal(scores[b], s) and words[b].tolist() == w.tolist(), b
        assert not w[0] & SM.REJECT and w[6] > 200 and w[4] > 4 * max(w[5], 1)      # a map, a scan, a peak well above the prior
    fixed = eng.scan_match_poses()
    for b in range(S):
        assert np.array_equal(fixed[b], SM.corrected_pose(priors[b], words[b], OCC, SCAN))
        assert not np.array_equal(fixed[b], priors[b])
    # the match left the maps' bytes as they were, and the next update fuses as if it had not run
    after = eng.occupancy_maps(logodds=True)
    assert all(a.tobytes() == c.tobytes() for a, c in zip(before, after))
    eng.occupancy_update_async(fixed)
    for b in range(S):
        maps[b].update(frames[b], fixed[b])
    _maps_equal(eng, maps, "fused under the corrected poses")
    eng.set_scan_match(None)
    assert eng.scan_match is None
    with pytest.raises(RuntimeError, match="set_scan_match first"):
        eng.scan_match_async(priors)
    eng.set_occupancy(None)


def test_localize_over_two_turns_of_the_ring_and_one(pp, eng):
    SM = pp.scan_match
    maps = _start(pp, eng)
    seen = set()
    for k in range(2 * OFF_RING + 1):
        frames, _ = _frames(pp, k)
        drift = ((k % 3) - 1, ((k + 1) % 3) - 1, (k % 2))                  # whole steps off the truth, within the window
        priors = np.stack([_prior(pp, b, k, drift) for b in range(S)])
        eng.upload(frames)
        fixed, words = eng.localize(priors)
        for b in range(S):
            w, _ = SM.match_np(maps[b], frames[b], priors[b], SCAN)
            want = SM.corrected_pose(priors[b], w, OCC, SCAN)
            assert words[b].tolist() == w.tolist() and np.array_equal(fixed[b], want), (k, b)
            maps[b].update(frames[b], want)
            seen.add(int(w[0]) & 3)
            if k == 0:
                assert w[0] & SM.NO_MAP and np.array_equal(fixed[b], priors[b])
        _maps_equal(eng, maps, f"step {k}")
    assert seen == {0, SM.NO_MAP}
    eng.set_scan_match(None)
    eng.set_occupancy(None)


def test_queued_matches_without_a_wait_give_the_last_calls_result(pp, eng):
    SM = pp.scan_match
    maps = _start(pp, eng)
    _build(pp, eng, maps, 3)
    frames, _ = _frames(pp, 3)
    eng.upload(frames)
    calls = 2 * OFF_RING + 1
    priors = [np.stack([_prior(pp, b, 3, ((i % 5) - 2, (i % 3) - 1, (i % 4) - 2)) for b in range(S)]) for i in range(calls)]
    for P in priors:
        eng.scan_match_async(P)
    words, scores = eng.scan_match_results(scores=True)
    for b in range(S):
        w, s = SM.match_np(maps[b], frames[b], priors[-1][b], SCAN)
        assert np.array_equal(scores[b], s) and words[b].tolist() == w.tolist(), b
        first, _ = SM.match_np(maps[b], frames[b], priors[0][b], SCAN)
        assert first.tolist() != w.tolist()
    eng.set_scan_match(None)
    eng.set_occupancy(None)


def test_set_occupancy_to_another_width_between_two_matches(pp, eng):
    SM = pp.scan_match
    maps = _start(pp, eng)
    _build(pp, eng, maps, 2)
    frames, poses = _frames(pp, 2)
    eng.upload(frames)
    eng.scan_match_async(poses)
    w0 = eng.scan_match_results()
    assert not (w0[:, 0] & 3).any()
    other = dict(OCC, width=70, height=50)                     # rows of 72 cells on the device: pitch != width
    eng.set_occupancy(other)
    eng.scan_match_async(poses)                                # the maps were forgotten with the shape
    assert (eng.scan_match_results()[:, 0] & 3 == SM.NO_MAP).all()
    maps = [pp.occupancy.OccupancyMap(other) for _ in range(S)]
    eng.occupancy_update_async(poses)
    for b in range(S):
        maps[b].update(frames[b], poses[b])
    priors = np.stack([_prior(pp, b, 2, (1, -1, 1)) for b in range(S)])
    eng.scan_match_async(priors)
    words, scores = eng.scan_match_results(scores=True)
    for b in range(S):
        w, s = SM.match_np(maps[b], frames[b], priors[b], SCAN)
        assert np.array_equal(scores[b], s) and words[b].tolist() == w.tolist(), b
        assert not w[0] & 3 and w[6] > 100
    eng.set_scan_match(None)
    eng.set_occupancy(None)


def test_refusals(pp, eng):
    eng.set_occupancy(None)
    with pytest.raises(RuntimeError, match="the occupancy stage is not configured"):
        eng.set_scan_match(True)
    eng.set_occupancy(OCC)
    eng.set_scan_match(SCAN)
    frames, poses = _frames(pp, 0)
    eng.upload(frames[:1])
    with pytest.raises(RuntimeError, match="1 frames are resident, batch is 2"):
        eng.scan_match_async(poses)
    far = poses[:1].copy()
    far[0, 1, 3] = -0.1 * 2.0 ** 30
    with pytest.raises(RuntimeError, match="2\\^30 cells"):
        eng.scan_match_async(far)
    with pytest.raises(RuntimeError, match="min_mean = 100001 outside"):
        pc = pp._lib.PPScanMatchConfig(1, 1, 1, 1024, 8, 0, 100001, 0)
        trig = np.ascontiguousarray(pp.local_planner.trig_table(), np.int32)
        eng._check(eng._lib.pp_set_scan_match(eng._h, ctypes.byref(pc), trig.ctypes.data, len(trig)), "pp_set_scan_match")
    assert eng.scan_match == pp.scan_match.ScanMatchConfig(**SCAN)          # a refused configuration changes nothing
    eng.set_scan_match(None)
    eng.set_occupancy(None)


def _weights(pp, d, seed=7):
    w = dict(pp.weights.init_weights(d, seed=seed))
    w["rpn/conv_cls/bias"] = np.array(w["rpn/conv_cls/bias"], np.float32) + np.float32(0.6)
    return w


def test_off_is_off(pp, hip_lib):
    """A handle on which the stage was set and then cleared, and one that never heard of it: the maps, their counts and the
    detections of the same frames are the same bytes."""
    rect, trv, _ = pp.synth.default_calib()
    rect, trv = np.stack([rect] * S), np.stack([trv] * S)
    outs = []
    for touched in (False, True):
        e = pp.Engine(pp.config.tiny_config(S), max_batch=S, max_points_per_frame=4096)
        try:
            e.load_weights(_weights(pp, e.d))
            e.set_occupancy(OCC)
            if touched:
                e.set_scan_match(SCAN)
                frames, poses = _frames(pp, 0)
                e.upload(frames)
                e.scan_match_async(poses)
                e.scan_match_results()
                e.set_scan_match(None)
            got = []
            for k in range(3):
                frames, poses = _frames(pp, k)
                dets, n = e.detect(frames, rect, trv)
                e.occupancy_update_async(poses)
                grid, org, lo = e.occupancy_maps(logodds=True)
                info = e.occupancy_info()
                got += [dets.tobytes(), n.tobytes(), grid.tobytes(), org.tobytes(), lo.tobytes()] + [info[key].tobytes() for key in sorted(info)]
            outs.append(got)
        finally:
            e.close()
    assert outs[0] == outs[1]
