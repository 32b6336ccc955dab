"""The ego-motion carry of tracking.py (the GPU step is held to it bit for bit in tests/test_gpu_track_ego.py): a scene
seen from a sensor that drives, sways and turns; the fixed-frame output; the cases around a posed step; and the unposed
path against the bytes the tracker gave before it took poses."""
import os
import re

import numpy as np
import pytest

import track_ego_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 40


@pytest.fixture(scope="module")
def T(pp):
    return pp.tracking


@pytest.fixture(scope="module")
def DET(pp):
    from pp_amd.engine import DET_DTYPE
    return DET_DTYPE


def _relative(pose_c, pose_s):
    """Independent of sweeps.relative_transform: homogeneous matrices, inv(T_c) @ T_s."""
    Tc, Ts = np.eye(4), np.eye(4)
    Tc[:3], Ts[:3] = pose_c, pose_s
    return np.linalg.inv(Tc) @ Ts


# ---- 1. the worked scene ----
@pytest.mark.parametrize("planar", [True, False])
def test_moving_sensor_scene(pp, T, DET, planar):
    """8 objects (6 static, 2 at constant ground velocity) from a sensor at 1.5 m/s, swaying, yawing at 1 rad/s, 30 Hz, 40
    steps, detections = the float32 sensor-frame centres.  With poses: exactly 8 ids; static tracks' fixed-frame speed
    <= 1e-4 m/s (a float32 ulp at 20 m is about 2e-6 m; over the 1/30 s frame time that is 6e-5 m/s: the rounding
    floor); the moving tracks' fixed-frame velocity within 5e-3 m/s of the truth.  Without poses the same detections open
    more than 8 ids.  The fixed-frame positions: within 1e-3 m of the truth -- the velocity bound over the 0.2 s (6 frames)
    the filter's gain remembers.  Measured (printed): planar 8 ids against 68, static 5.1e-07 m/s, moving 4.2e-04 m/s,
    position 7.9e-05 m; with roll and pitch 8 against 68, 2.6e-07 m/s, 4.2e-04 m/s, 7.9e-05 m."""
    poses, frames, pos, vel = C.ego_scene(DET, STEPS, planar)
    if planar:
        for i in (0, 17, STEPS - 1):                 # the planar sequence is what sweeps.pose_from_xyyaw builds
            yaw = 0.3 + i * C.DT
            assert np.array_equal(poses[i], pp.sweeps.pose_from_xyyaw(poses[i, 0, 3], poses[i, 1, 3], yaw))
    else:
        assert np.abs(poses[:, 2, :2]).max() > 0.02 and np.abs(poses[:, 2, 3]).max() > 0.02
    posed, plain = T.Tracker(T.TrackConfig(), 1), T.Tracker(T.TrackConfig(), 1)
    for i, (d, n) in enumerate(frames):
        posed.step(d, n, poses=poses[i:i + 1])
        plain.step(d, n)
    ids_posed, ids_plain = int(posed.next_id[0]) - 1, int(plain.next_id[0]) - 1
    tr, n = posed.tracks_fixed()
    assert n[0] == 8
    by_row = {int(r["det_row"]): r for r in tr[0, :8]}
    assert sorted(by_row) == list(range(8)) and all(by_row[k]["hits"] == STEPS for k in range(8))
    static = max(float(np.sqrt((by_row[k]["state"][3:] ** 2).sum())) for k in range(6))
    moving = max(float(np.abs(by_row[k]["state"][3:] - vel[k]).max()) for k in (6, 7))
    where = max(float(np.abs(by_row[k]["state"][:3] - (pos[k] + vel[k] * (STEPS - 1) * C.DT)).max()) for k in range(8))
    print(f"planar={planar}: ids {ids_posed} posed / {ids_plain} unposed; static fixed-frame speed {static:.3e} m/s; "
          f"moving velocity error {moving:.3e} m/s; fixed-frame position error {where:.3e} m")
    assert ids_posed == 8
    assert ids_plain > 8
    assert static <= 1e-4
    assert moving <= 5e-3
    assert where <= 1e-3
    # the sensor-frame velocity of a static object's track is zero as well: it is over ground, in the sensor's axes
    trs, ns, _ = posed.tracks()
    assert max(float(np.abs(r["state"][3:]).max()) for r in trs[0, :8] if r["det_row"] < 6) <= 1e-4


# ---- 2. the fixed frame ----
def test_tracks_fixed_is_the_pose_applied_in_the_rule_order(pp, T, DET):
    poses, frames, _, _ = C.ego_scene(DET, 6, planar=False)
    t = T.Tracker(T.TrackConfig(), 2)
    for i, (d, n) in enumerate(frames):
        d2, n2 = np.concatenate([d, d]), np.concatenate([n, n])
        tr, nt, _ = t.step(d2, n2, poses=poses[i:i + 1])          # stream 1 steps without a pose
        fx, nf = t.tracks_fixed()
        assert nf.tolist() == [int(nt[0]), -1] and not fx[1].tobytes().strip(b"\0")
        P, psi = poses[i], np.float64(np.arctan2(poses[i, 1, 0], poses[i, 0, 0]))
        want = tr[0].copy()
        for k in range(int(nt[0])):
            x, y, z, vx, vy, vz = tr[0, k]["state"]
            for q in range(3):
                want["state"][k, q] = ((P[q, 0] * x + P[q, 1] * y) + P[q, 2] * z) + P[q, 3]
                want["state"][k, 3 + q] = (P[q, 0] * vx + P[q, 1] * vy) + P[q, 2] * vz
            want["yaw"][k] = tr[0, k]["yaw"] + psi
        assert fx[0].tobytes() == want.tobytes(), i
    assert np.abs(fx[0]["state"][:8, :3] - tr[0]["state"][:8, :3]).max() > 0.1     # (the two frames do differ)


def test_carry_equals_a_homogeneous_matrix_formulation(pp, T, DET):
    """One carry against inv(T_c) T_p applied with numpy: 1e-12 relative to the 20 m scale is what two float64 orderings of
    a rigid transform allow."""
    poses, frames, _, _ = C.ego_scene(DET, 2, planar=False)
    t = T.Tracker(T.TrackConfig(), 1)
    t.step(*frames[0], poses=poses[0:1])
    before, yaw0 = t.x[0, :8].copy(), t.yaw[0, :8].copy()
    before[:, 3:] = [[0.3, -0.2, 0.1]] * 8                           # give the tracks a velocity to rotate
    t.x[0, :8] = before
    empty = (np.zeros((1, 4), DET), np.zeros(1, np.int32))
    t.step(*empty, dt=[1e-9], poses=poses[1:2])                      # no rows: carry, a (negligible) prediction, ageing
    H = _relative(poses[1], poses[0])
    want_x = before[:, :3] @ H[:3, :3].T + H[:3, 3]
    want_v = before[:, 3:] @ H[:3, :3].T
    assert np.abs(t.x[0, :8, 3:] - want_v).max() <= 1e-12
    assert np.abs(t.x[0, :8, :3] - (want_x + want_v * 1e-9)).max() <= 20.0 * 1e-12
    dpsi = np.arctan2(poses[1, 1, 0], poses[1, 0, 0]) - np.arctan2(poses[0, 1, 0], poses[0, 0, 0])
    assert np.array_equal(t.yaw[0, :8], yaw0 + dpsi) and dpsi != 0.0
    assert np.array_equal(t.p[0, 0], T.Tracker.predict_cov(0.01, 0.0, 4.0, np.float64(1e-9), 4.0))   # the covariance: predicted only


# ---- 3. the cases around a posed step ----
def _run(T, frames, poses, plan, streams=1):
    """plan[i]: "pose", "none" or "flag" for step i of stream 0."""
    t = T.Tracker(T.TrackConfig(), streams)
    for i, what in enumerate(plan):
        d, n = frames[i][0].copy(), frames[i][1].copy()
        if what == "flag":
            n[0] |= 1 << 30
        t.step(d, n, poses=None if what == "none" else poses[i:i + 1])
    return t


def test_flagged_step_keeps_the_previous_pose_and_the_next_carries_over_both_intervals(pp, T, DET):
    poses, frames, _, _ = C.ego_scene(DET, 8, planar=False)
    t = T.Tracker(T.TrackConfig(), 1)
    for i in range(4):
        t.step(*frames[i], poses=poses[i:i + 1])
    state = (t.x.copy(), t.p.copy(), t.yaw.copy(), t.prev_pose.copy(), t.prev_psi.copy(), t.has_prev.copy())
    out = [a.copy() for a in t.tracks() + t.tracks_fixed()]
    n = frames[4][1].copy()
    n[0] |= 1 << 30
    t.step(frames[4][0], n, poses=poses[4:5])
    for a, b in zip(state, (t.x, t.p, t.yaw, t.prev_pose, t.prev_psi, t.has_prev)):
        assert np.array_equal(a, b)
    assert all(np.array_equal(a, b) for a, b in zip(out, t.tracks() + t.tracks_fixed()))
    # the next posed step carries from pose 3 to pose 5: the same as a tracker that never saw step 4, given its dt
    t.step(*frames[5], dt=[2 * C.DT], poses=poses[5:6])
    u = _run(T, frames, poses, ["pose"] * 4)
    u.step(*frames[5], dt=[2 * C.DT], poses=poses[5:6])
    assert t.tracks()[0].tobytes() == u.tracks()[0].tobytes() and t.tracks_fixed()[0].tobytes() == u.tracks_fixed()[0].tobytes()
    assert t.next_id[0] == 9 and (t.tracks()[0][0, :8]["hits"] == 5).all()          # and every object kept its track


def test_reset_forgets_the_pose(pp, T, DET):
    poses, frames, _, _ = C.ego_scene(DET, 4, planar=True)
    t = _run(T, frames, poses, ["pose"] * 3)
    assert t.has_prev[0]
    t.reset(0)
    assert not t.has_prev[0]
    t.step(*frames[3], poses=poses[3:4])                              # carries nothing, births from row coordinates
    fresh = T.Tracker(T.TrackConfig(), 1)
    fresh.step(*frames[3], poses=poses[3:4])
    assert t.tracks()[0].tobytes() == fresh.tracks()[0].tobytes() and t.tracks_fixed()[0].tobytes() == fresh.tracks_fixed()[0].tobytes()
    two = T.Tracker(T.TrackConfig(), 2)
    two.step(np.concatenate([frames[0][0]] * 2), np.array([8, 8], np.int32), poses=poses[0:2])
    two.reset()
    assert not two.has_prev.any()


def test_stream_posed_only_from_step_3_carries_nothing_on_that_step(pp, T, DET):
    poses, frames, _, _ = C.ego_scene(DET, 6, planar=False)
    t = _run(T, frames, poses, ["none", "none", "none", "pose"])
    plain = _run(T, frames, poses, ["none"] * 4)
    assert not plain.has_prev[0] and t.has_prev[0] and np.array_equal(t.prev_pose[0], poses[3])
    assert t.tracks()[0].tobytes() == plain.tracks()[0].tobytes()                # step 3 itself: as without a pose
    assert t.tracks_fixed()[1].tolist() == [int(t.tracks()[1][0])] and plain.tracks_fixed()[1].tolist() == [-1]
    t.step(*frames[4], poses=poses[4:5])                                          # ... and the next one carries
    plain.step(*frames[4])
    assert t.tracks()[0].tobytes() != plain.tracks()[0].tobytes()
    # a pose for stream 0 alone in a two-stream step: stream 1 steps unposed
    two = T.Tracker(T.TrackConfig(), 2)
    for i in range(3):
        two.step(np.concatenate([frames[i][0]] * 2), np.array([8, 8], np.int32), poses=poses[i:i + 1])
    assert two.has_prev.tolist() == [True, False] and two.tracks_fixed()[1].tolist() == [8, -1]


def test_a_step_without_poses_leaves_the_previous_pose(pp, T, DET):
    poses, frames, _, _ = C.ego_scene(DET, 4, planar=True)
    t = _run(T, frames, poses, ["pose", "none"])
    assert t.has_prev[0] and np.array_equal(t.prev_pose[0], poses[0]) and t.tracks_fixed()[1].tolist() == [-1]


def test_bad_poses_raise_naming_the_stream(pp, T, DET):
    poses, frames, _, _ = C.ego_scene(DET, 1, planar=True)
    d, n = np.concatenate([frames[0][0]] * 2), np.array([8, 8], np.int32)
    t = T.Tracker(T.TrackConfig(), 2)
    two = np.stack([poses[0], poses[0]])
    bad = two.copy()
    bad[1, 0, 3] = np.nan
    with pytest.raises(ValueError, match="stream 1 is not finite"):
        t.step(d, n, poses=bad)
    bad = two.copy()
    bad[1, :, :3] *= 1.0 + 1e-5
    with pytest.raises(ValueError, match="rotation of stream 1 is not orthonormal"):
        t.step(d, n, poses=bad)
    with pytest.raises(ValueError, match="poses"):
        t.step(d, n, poses=np.stack([poses[0]] * 3))
    with pytest.raises(ValueError, match="poses"):
        t.step(d, n, poses=np.zeros((2, 4, 4)))
    assert t.next_id.tolist() == [1, 1] and not t.has_prev.any()       # refused before anything moved
    good = two.copy()
    good[1, :, :3] *= 1.0 + 1e-7                                       # inside sweeps.ORTHO_TOL
    t.step(d, n, poses=good)
    assert t.has_prev.all()


def test_check_poses_is_the_pose_half_of_check_call(pp):
    S = pp.sweeps
    P = np.stack([S.pose_from_xyyaw(1.0, 2.0, 0.3), S.pose_from_xyyaw(0.0, 0.0, -1.0)])
    assert np.array_equal(S.check_poses(P, 2), P) and S.check_poses(P.tolist(), 2).dtype == np.float64
    got = S.check_call(P, [1.0, 2.0], 2, np.array([np.nan, 1.5]))
    assert np.array_equal(got[0], P) and got[1].tolist() == [1.0, 2.0] and got[2].tolist() == [1.0, 2.0]
    bad = P.copy()
    bad[1, 1, 1] = np.inf
    for call in (lambda: S.check_poses(bad, 2), lambda: S.check_call(bad, [1.0, 2.0], 2, [np.nan, np.nan])):
        with pytest.raises(ValueError, match="the pose of stream 1 is not finite"):
            call()
    with pytest.raises(ValueError, match="2 poses for 3 frames"):
        S.check_poses(P, 3)
    # check_call's order stands: a stream's stamp is looked at before its rotation
    skew = P.copy()
    skew[0, 0, 0] = 2.0
    with pytest.raises(ValueError, match="stamp of stream 0 is not finite"):
        S.check_call(skew, [np.nan, 2.0], 2, [np.nan, np.nan])
    with pytest.raises(ValueError, match="rotation of stream 0 is not orthonormal"):
        S.check_call(skew, [1.0, 2.0], 2, [np.nan, np.nan])


# ---- 4. the unposed path is the tracker as it was ----
GOLD = C.unposed_cases()


@pytest.mark.parametrize("name", sorted(GOLD))
def test_unposed_steps_are_the_bytes_recorded_before_the_carry(pp, T, DET, name):
    from conftest import load_golden
    gold = load_golden("track_ego_unposed.npz")
    digest, (tr, n, ov) = C.run_unposed(T, DET, name)
    assert bytes.fromhex(digest) == gold[name + "/sha256"].tobytes()
    m = gold[name + "/tracks"].shape[1]
    assert tr[:, :m].tobytes() == gold[name + "/tracks"].tobytes()
    assert np.array_equal(n, gold[name + "/n"]) and np.array_equal(ov, gold[name + "/overflow"])


def test_track_np_takes_poses(pp, T, DET):
    poses, frames, _, _ = C.ego_scene(DET, 5, planar=False)
    outs = T.track_np(T.TrackConfig(), frames, poses=[poses[i:i + 1] for i in range(5)])
    t = T.Tracker(T.TrackConfig(), 1)
    for i, (d, n) in enumerate(frames):
        want = t.step(d, n, poses=poses[i:i + 1])
        assert all(np.array_equal(a, b) for a, b in zip(outs[i], want))
    assert outs[-1][0].tobytes() != T.track_np(T.TrackConfig(), frames)[-1][0].tobytes()


# ---- 5. plumbing ----
def test_header_exports_and_engine_name_the_new_calls(pp):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    ex = pp._lib.EXPORTS
    for name in ("pp_set_track_pose", "pp_get_tracks_fixed"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, flags=re.M), name
        assert name in hdr.split("#define PP_ABI_VERSION")[0], "listed among the later additions within 4"
        assert name in ex and ex.index(name) < ex.index("pp_soft_nms")
    for name in ("set_track_pose", "tracks_fixed", "set_track_ego", "track_ego", "track_update"):
        assert hasattr(pp.Engine, name), name
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    # one pose checker for the sweeps and the tracker
    assert "pose_check_orthonormal" in open(os.path.join(csrc, "pp_engine.h")).read()
    for src in ("api_sweeps.hip", "api_track.hip", "api_occupancy.hip"):    # ... reached through check_poses, stream by stream
        text = open(os.path.join(csrc, src)).read()
        assert "check_poses(" in text and "is not orthonormal" not in text and "is not finite\", who, b, i / 4" not in text, src
