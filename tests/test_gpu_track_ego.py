"""The ego-motion carry of the tracking step on the GPU (csrc/track.hip: k_track_step) against tracking.py's restatement:
tracks(), tracks_fixed() and their counts must be EQUAL byte for byte.  Standalone on hand-made rows
(Engine.track_update(poses=)), behind the detector's post-process inside its captured graph (set_track_ego, with the
sweeps off and on), and the refusals of pp_set_track_pose."""
import ctypes

import numpy as np
import pytest

import track_ego_cases as C

pytestmark = pytest.mark.gpu

S, ROWS, STEPS = 3, 100, 12
FIELDS = ("state", "size", "yaw", "score", "id", "label", "hits", "misses", "confirmed", "det_row", "reserved")
FLAG = 1 << 30


def _tiny(pp, B=S, **second):
    cfg = pp.config.tiny_config(B)
    cfg["model"]["second"]["num_class"] = 1
    cfg["model"]["second"].update(second)
    return cfg


@pytest.fixture(scope="module")
def eng(pp, hip_lib):
    e = pp.Engine(_tiny(pp), max_batch=S, max_points_per_frame=4096)
    yield e
    e.close()


def _cfg(pp, **kw):
    base = dict(gate=0.6, birth_score=0.3, max_misses=2, min_hits=3, size_alpha=0.3)
    base.update(kw)
    return pp.tracking.TrackConfig(**base)


def _same(eng, ref, got, want, what):
    (gt, gn, go), (wt, wn, wo) = got, want
    assert np.array_equal(gn, wn), (what, gn, wn)
    assert np.array_equal(go, wo), (what, go, wo)
    for f in FIELDS:
        assert np.array_equal(gt[f], wt[f]), (what, f)
    assert gt.tobytes() == wt.tobytes(), what
    (ft, fn), (rt, rn) = eng.tracks_fixed(len(wn)), ref.tracks_fixed(len(wn))
    assert np.array_equal(fn, rn), (what, "fixed", fn, rn)
    for f in FIELDS:
        assert np.array_equal(ft[f], rt[f]), (what, "fixed", f)
    assert ft.tobytes() == rt.tobytes(), (what, "fixed")


def _fresh(pp, eng, cfg):
    eng.set_tracking(cfg)
    eng.set_tracking(None)          # track_update needs the configuration, not the switch
    eng.track_reset()
    return pp.tracking.Tracker(cfg, eng.max_batch)


def _both(eng, ref, d, n, dt, poses, what):
    got = eng.track_update(d, n, dt, poses=poses)
    want = ref.step(d, n, dt, poses=poses)
    _same(eng, ref, got, want, what)
    return got


def _stream_poses(steps):
    """[steps, S, 3, 4]: stream 0 rolls, pitches and heaves; stream 1 is planar; stream 2 is stream 0's motion backwards."""
    full, planar = C.ego_poses(steps, planar=False), C.ego_poses(steps, planar=True)
    return np.stack([full, planar, full[::-1]], axis=1)


def _scene_rows(pp, poses, step, counts, rng, dropout=0.15):
    """Per stream `counts[s]` objects standing in the fixed frame (8 .. 20 m out, 1.2 m apart at least), seen from the
    stream's pose of this step: float32 sensor-frame rows in a shuffled order, some dropped, one false positive."""
    from pp_amd.engine import DET_DTYPE
    d = np.zeros((S, ROWS), DET_DTYPE)
    n = np.zeros(S, np.int32)
    for s in range(S):
        orng = np.random.default_rng(1000 + s)                   # the objects: the same at every step
        obj = []
        while len(obj) < counts[s]:
            r, a = orng.uniform(8.0, 20.0), orng.uniform(-np.pi, np.pi)
            p = np.array([r * np.cos(a), r * np.sin(a), orng.uniform(-0.5, 0.5)])
            if all(np.hypot(*(p - q)[:2]) >= 1.2 for q in obj):
                obj.append(p)
        lab = orng.integers(0, 2, counts[s])
        R, t = poses[step, s, :, :3], poses[step, s, :, 3]
        local = (np.array(obj) - t) @ R
        rows = [(local[k], int(lab[k])) for k in range(counts[s]) if rng.random() >= dropout]
        rows.append((rng.uniform(-20, 20, 3) * [1, 1, 0.02], 0))
        order = rng.permutation(len(rows))
        n[s] = len(rows)
        for i, k in enumerate(order):
            d["box3d_lidar"][s, i, :3] = rows[k][0]
            d["box3d_lidar"][s, i, 3:6] = rng.uniform(0.4, 0.9, 3)
            d["box3d_lidar"][s, i, 6] = rng.uniform(-3, 3)
            d["score"][s, i] = rng.uniform(0.2, 0.95)
            d["label"][s, i] = rows[k][1]
    return d, n


# ---- 1. track_update with poses ----
def test_twelve_posed_steps_on_three_streams(pp, eng):
    """Stream 0: full 3-D rotations; stream 1: planar; stream 2: no pose until step 3, and a flagged count at step 6.  The
    sensor frames turn by 1 rad/s: unposed, objects 8 .. 20 m out would leave the 0.6 m gate every frame."""
    rng = np.random.default_rng(5)
    ref = _fresh(pp, eng, _cfg(pp))
    poses = _stream_poses(STEPS)
    dts = np.array([C.DT, C.DT, 0.05])
    for step in range(STEPS):
        d, n = _scene_rows(pp, poses, step, (30, 12, 20), rng)
        if step == 6:
            n[2] |= FLAG
        P = poses[step, :2] if step < 3 else poses[step]
        got = _both(eng, ref, d, n, dts, P, f"step {step}")
        if step == 2:
            assert eng.tracks_fixed()[1].tolist()[2] == -1
    tr, nt, _ = got
    info = eng.track_info()
    assert np.array_equal(info["next_id"], ref.next_id) and np.array_equal(info["live"], ref.info()["live"])
    assert ref.has_prev.all()
    # the carry held the tracks: streams 0 and 1 have tracks that were matched in (nearly) every step, and far fewer ids
    # than an unposed tracker of the same rows would open
    assert (tr[0]["hits"][:nt[0]] >= 8).sum() >= 15 and (tr[1]["hits"][:nt[1]] >= 8).sum() >= 6
    assert ref.next_id[0] < 30 + 2 * STEPS
    assert (tr[2]["hits"][:nt[2]] >= 5).sum() >= 8                     # stream 2: since its first posed step, the flagged one aside


def test_all_sixty_four_slots_carry(pp, eng):
    rng = np.random.default_rng(6)
    """71 and 65 rows on streams 0 and 1 (one false positive each), birth_score 0: the tables are full from the first step
    on, so every lane carries in each of the three posed steps that follow; nearly every track is matched each time."""
    ref = _fresh(pp, eng, _cfg(pp, max_misses=5, birth_score=0.0))
    poses = _stream_poses(4)
    for step in range(4):
        d, n = _scene_rows(pp, poses, step, (70, 64, 3), rng, dropout=0.0)
        got = _both(eng, ref, d, n, None, poses[step], f"full table, step {step}")
        assert got[1].tolist()[:2] == [64, 64]
    assert got[2][0] > 0 and got[2][1] > 0
    assert (got[0][0]["hits"][:64] == 4).sum() >= 60 and (got[0][1]["hits"][:64] == 4).sum() >= 60


def test_reset_between_steps_forgets_the_pose(pp, eng):
    rng = np.random.default_rng(7)
    ref = _fresh(pp, eng, _cfg(pp))
    poses = _stream_poses(6)
    for step in range(6):
        if step == 3:
            eng.track_reset(1)
            ref.reset(1)
        d, n = _scene_rows(pp, poses, step, (10, 10, 10), rng)
        got = _both(eng, ref, d, n, None, poses[step], f"reset, step {step}")
    assert got[0][1]["hits"][:got[1][1]].max() == 3 and got[0][0]["hits"][:got[1][0]].max() == 6
    eng.track_reset()
    ref.reset()
    d, n = _scene_rows(pp, poses, 0, (5, 5, 5), rng)
    _both(eng, ref, d, n, None, poses[0], "after reset()")
    assert not np.array_equal(ref.prev_pose[0], poses[5, 0])


def test_an_armed_pose_waits_for_its_step(pp, eng):
    """set_track_pose arms the next step whoever runs it: track_update without poses= does not clear it, a reset in between
    does not either (it forgets the PREVIOUS pose), and a shorter step takes its own streams' poses."""
    rng = np.random.default_rng(8)
    ref = _fresh(pp, eng, _cfg(pp))
    poses = _stream_poses(5)
    frames = [_scene_rows(pp, poses, step, (6, 6, 6), rng, dropout=0.0) for step in range(5)]
    _both(eng, ref, *frames[0], None, poses[0], "first")
    eng.set_track_pose(poses[1])
    _same(eng, ref, eng.track_update(*frames[1]), ref.step(*frames[1], poses=poses[1]), "armed, then a plain track_update")
    _same(eng, ref, eng.track_update(*frames[2]), ref.step(*frames[2]), "spent: the next plain step has no pose")
    assert eng.tracks_fixed()[1].tolist() == [-1, -1, -1]
    eng.set_track_pose(poses[3])
    d, n = frames[3]
    _same(eng, ref, eng.track_update(d[:1], n[:1]), ref.step(d[:1], n[:1], poses=poses[3, :1]), "stream 0 alone")
    # streams 1 and 2 still hold pose 3; arming again replaces it, and the full step runs under pose 4 on every stream
    eng.set_track_pose(poses[4])
    _same(eng, ref, eng.track_update(*frames[4]), ref.step(*frames[4], poses=poses[4]), "armed again")
    eng.set_track_pose(poses[3])                                       # a reset in between forgets the PREVIOUS pose only
    eng.track_reset(2)
    ref.reset(2)
    _same(eng, ref, eng.track_update(*frames[3]), ref.step(*frames[3], poses=poses[3]), "armed, reset, step")
    assert eng.tracks_fixed()[1].tolist() == ref.tracks_fixed()[1].tolist() and (eng.tracks_fixed()[1] >= 0).all()


# ---- 2. behind the detector's post-process ----
def _weights(pp, d, seed=7):
    w = dict(pp.weights.init_weights(d, seed=seed))
    w["rpn/conv_cls/bias"] = np.array(w["rpn/conv_cls/bias"], np.float32) + np.float32(0.6)     # enough detections to track
    return w


def _frames(step, B):
    """Seeded clouds of the tiny grid, moved by 1 cm in x per step."""
    out = []
    for b in range(B):
        rng = np.random.default_rng(300 + b)
        pts = rng.uniform([0.05, -0.6, -2.5], [1.3, 0.6, 2.5], (300 + 50 * b, 3))
        pts[:, 0] += 0.01 * step
        out.append(pts.astype(np.float32))
    return out


def _pass_poses(step, B):
    """Small motions: the tiny grid is 1.5 m long, the tracks must stay near their rows."""
    return np.stack([C.rot_zyx(0.02 * step * (b + 1), 0.003 * step, -0.002 * step * b) @ np.eye(3, 4)
                     + np.array([[0, 0, 0, 0.01 * step], [0, 0, 0, -0.004 * step * (b + 1)], [0, 0, 0, 0.001 * step]])
                     for b in range(B)])


def _dets_bytes(dets, n):
    return [dets[b, :n[b]].tobytes() for b in range(len(n))], n.copy()


@pytest.mark.parametrize("with_sweeps", [False, True])
def test_passes_carry_their_tracks_under_the_poses(pp, hip_lib, with_sweeps):
    """set_track_ego(True): detect(frames, poses=, stamps=) five times with different poses -- the pass captured on the
    first is replayed on the others, the kernel reads the new poses from device memory.  Sweeps off: the detections are a
    plain engine's of the same frames; sweeps on: a plain engine's of the restatement's accumulated frames, and tracker and
    sweeps consume the same poses."""
    B = 2
    sw = {"history": 2, "capacity": 400, "history_decimate": 1, "max_age": 0.25, "time_feature": -1}
    e = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=2048)
    plain = pp.Engine(_tiny(pp, B), max_batch=B, max_points_per_frame=2048)
    try:
        for x in (e, plain):
            x.load_weights(_weights(pp, x.d))
        cfg = _cfg(pp, gate=0.3, birth_score=0.0, max_misses=1, min_hits=2)
        assert e.track_ego is False
        with pytest.raises(ValueError, match="tracking is off"):
            e.set_track_ego(True)
        e.set_tracking(cfg)
        if with_sweeps:
            e.set_sweeps(sw)
            acc = pp.sweeps.SweepAccumulator(sw, B, 3, 2048)
        else:                                                           # ego off: poses= still means sweeps, and they are off
            with pytest.raises(RuntimeError, match="not configured"):
                e.detect(_frames(0, B), poses=_pass_poses(0, B), stamps=[0.5, 0.5])
        e.set_track_ego(True)
        assert e.track_ego is True
        ref = pp.tracking.Tracker(cfg, B)
        stamps = np.array([10.0, 20.0])
        total = 0
        for step in range(5):
            prev, stamps = stamps, stamps + np.array([0.04, 0.05 + 0.01 * step])
            frames, P = _frames(step, B), _pass_poses(step, B)
            want_frames = acc.accumulate(frames, P, stamps)[0] if with_sweeps else frames
            dets, n = e.detect(frames, poses=P, stamps=stamps)
            assert _dets_bytes(dets, n)[0] == _dets_bytes(*plain.detect(want_frames))[0], f"pass {step}: detections differ"
            want = ref.step(dets, n, None if step == 0 else stamps - prev, poses=P)
            _same(e, ref, e.tracks(), want, f"sweeps {with_sweeps}, pass {step}")
            total += int(n.sum())
        print(f"sweeps {with_sweeps}: {total} detections in 5 passes, tracks {want[1].tolist()}, next ids {ref.next_id.tolist()}")
        assert total > 0 and want[1].sum() > 0 and (want[0]["hits"] >= 3).any()
        # the resident frames again with poses set by hand, then without: replays of the same captured pass
        dets, n = e.detections()
        for k, P in enumerate((_pass_poses(6, B), None, _pass_poses(7, B))):
            if P is not None:
                e.set_track_pose(P)
            e.detect_async()
            _same(e, ref, e.tracks(), ref.step(dets, n, None, poses=P), f"replay {k}")
        # a bad pose is refused before the frames are touched or anything is queued
        bad = _pass_poses(8, B)
        bad[1, 0, 0] += 0.01
        before = e.track_info()
        with pytest.raises(ValueError, match="stream 1 is not orthonormal"):
            e.detect(_frames(8, B), poses=bad, stamps=stamps + 1.0)
        assert all(np.array_equal(before[k], e.track_info()[k]) for k in before)
        if not with_sweeps:                                             # the sweeps off: stamps are optional (the period)
            dets, n = e.detect(_frames(5, B), poses=_pass_poses(8, B))
            _same(e, ref, e.tracks(), ref.step(dets, n, None, poses=_pass_poses(8, B)), "no stamps")
        # ego off again: poses= goes to the sweeps alone
        e.set_track_ego(False)
        if with_sweeps:
            stamps = stamps + 2.0
            dets, n = e.detect(_frames(5, B), poses=_pass_poses(9, B), stamps=stamps)
            _same(e, ref, e.tracks(), ref.step(dets, n, np.array([2.0, 2.0])), "ego off")
            assert e.tracks_fixed()[1].tolist() == [-1, -1]
    finally:
        e.close()
        plain.close()


# ---- 3. refusals ----
def _c_pose(e, poses, batch, handle=True):
    P = None if poses is None else np.ascontiguousarray(poses, np.float64)
    st = e._lib.pp_set_track_pose(e._h if handle else None, None if P is None else P.ctypes.data_as(ctypes.c_void_p), batch)
    return st, e._lib.pp_last_error(e._h if handle else None).decode()


def test_refusals_leave_the_tables_as_they_were(pp, hip_lib):
    rng = np.random.default_rng(9)
    e = pp.Engine(_tiny(pp, 2), max_batch=2, max_points_per_frame=4096)
    try:
        poses = _stream_poses(3)[:, :2]
        st, msg = _c_pose(e, poses[0], 2)
        assert st == 2 and "pp_set_track_pose: pp_set_tracking has given no configuration" in msg     # PP_ERR_STATE
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_set_track_pose"):
            e.set_track_pose(poses[0])
        cfg = _cfg(pp)
        e.set_tracking(cfg)
        ref = pp.tracking.Tracker(cfg, 2)
        frames = [tuple(a[:2] for a in _scene_rows(pp, _stream_poses(3), step, (6, 6, 6), rng, dropout=0.0)) for step in range(3)]
        _same(e, ref, e.track_update(*frames[0], poses=poses[0]), ref.step(*frames[0], poses=poses[0]), "before")
        st, msg = _c_pose(e, poses[1], 2, handle=False)
        assert st == 1 and "pp_set_track_pose: NULL handle" in msg
        st, msg = _c_pose(e, None, 2)
        assert st == 1 and "pp_set_track_pose: poses is NULL" in msg
        for batch in (0, 3, -1):
            st, msg = _c_pose(e, np.concatenate([poses[1], poses[1]]), batch)
            assert st == 1 and f"batch {batch} outside" in msg
        bad = poses[1].copy()
        bad[1, 2, 3] = np.inf
        st, msg = _c_pose(e, bad, 2)
        assert st == 1 and "pp_set_track_pose: poses: stream 1: row 2, column 3 is not finite" in msg
        bad = poses[1].copy()
        bad[0, 1, :3] *= 1.0 + 1e-5
        st, msg = _c_pose(e, bad, 2)
        assert st == 1 and "pp_set_track_pose: poses: the rotation of stream 0 is not orthonormal (R R^T [1][1]" in msg
        with pytest.raises(ValueError, match="set_track_pose: poses must be"):
            e.set_track_pose(np.zeros((2, 4, 4)))
        with pytest.raises(ValueError, match="track_update: poses"):
            e.track_update(*frames[1], poses=np.stack([poses[1, 0]] * 3))
        assert e._lib.pp_get_tracks_fixed(e._h, None, None) == 1 and b"pp_get_tracks_fixed: NULL argument" in e._lib.pp_last_error(e._h)
        # nothing of that armed a pose or moved a table: an unposed step, then a posed one that carries from pose 0
        _same(e, ref, e.track_update(*frames[1]), ref.step(*frames[1]), "after the refusals, unposed")
        _same(e, ref, e.track_update(*frames[2], poses=poses[2]), ref.step(*frames[2], poses=poses[2]), "after the refusals, posed")
        good = poses[2].copy()
        good[0, :, :3] *= 1.0 + 1e-7                                    # inside the tolerance: taken as it is
        _same(e, ref, e.track_update(*frames[2], poses=good), ref.step(*frames[2], poses=good), "within the tolerance")
        # a flagged count passes pp_track_update as a pass would hand it on; a negative one does not
        nf = frames[1][1].copy()
        nf[1] |= FLAG
        _same(e, ref, e.track_update(frames[1][0], nf, poses=poses[1]), ref.step(frames[1][0], nf, poses=poses[1]), "flagged")
        _same(e, ref, e.track_update(*frames[2], poses=poses[2]), ref.step(*frames[2], poses=poses[2]), "after the flagged step")
        with pytest.raises(RuntimeError, match=r"n_dets\[1\] = -1 outside"):
            e.track_update(frames[1][0], np.array([1, -1], np.int32))
    finally:
        e.close()
    with pytest.raises(RuntimeError, match="untracked"):
        e2 = pp.Engine(_tiny(pp, 1), max_batch=1, max_points_per_frame=4096)
        try:
            e2.tracks_fixed()
        finally:
            e2.close()


def test_refused_while_a_training_step_is_in_flight(pp, hip_lib):
    B = 2
    cfg = _tiny(pp, B)
    tr = pp.Trainer(cfg, pp.weights.init_weights(pp.config.Derived(cfg), seed=7), max_batch=B, max_points_per_frame=4096,
                    learning_rate=2e-4, weight_decay=1e-4)
    e = tr.engine
    try:
        rng = np.random.default_rng(10)
        tcfg = _cfg(pp)
        e.set_tracking(tcfg)
        ref = pp.tracking.Tracker(tcfg, B)
        poses = _stream_poses(2)[:, :B]
        frames = [tuple(a[:B] for a in _scene_rows(pp, _stream_poses(2), step, (6, 6, 6), rng, dropout=0.0)) for step in range(2)]
        _same(e, ref, e.track_update(*frames[0], poses=poses[0]), ref.step(*frames[0], poses=poses[0]), "before the step")
        gts = [np.array([[0.8, 0.2 * b, 0.0, 0.6, 0.8, 1.73, 0.1]], np.float32) for b in range(B)]
        e.upload(_frames(0, B))
        e.train_step_gt_async(tr.params.data_ptr(), tr.grads.data_ptr(), tr.state.data_ptr(), *e.pack_gt(gts))
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_set_track_pose: a training step is in flight"):
            e.set_track_pose(poses[1])
        assert np.isfinite(e.train_step_wait()["loss"])
        _same(e, ref, e.track_update(*frames[1]), ref.step(*frames[1]), "after the step: no pose was armed")
    finally:
        tr.close()
