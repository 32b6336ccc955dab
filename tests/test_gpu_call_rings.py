"""The pinned call rings (csrc/pp_ring.h) past one full turn: 2 * OFF_RING + 1 = 9 calls queued back to back on every ring
with nothing fetched in between, every call with data of its own, so that a slot handed out early or copied from the wrong
offset shows as a wrong result.  The occupancy call ring, the handle's ring with its riders (offsets, crop planes, sweep
poses; ingest records, feature tables, rig sources) and the tracker's dt and pose rings, each against the host rule of its
stage, bit for bit; calls that must be refused are interleaved and must leave the rings where they were.  No test provokes
a fault: every refused call is refused on the host before anything is queued."""
import ctypes

import numpy as np
import pytest

import depth_cases
import pc2_feature_cases as fc

pytestmark = pytest.mark.gpu

S = 3                    # streams
TURN = 9                 # 2 * OFF_RING + 1
NMAX = 4096
W, H = 37, 29            # the occupancy window: the width no multiple of 4
OCC = dict(resolution=0.1, z_min=0.0, z_max=1.0, max_range=2.5, width=W, height=H)


def _weights(pp, d):
    w = dict(pp.weights.init_weights(d, seed=7))
    w["rpn/conv_cls/bias"] = np.array(w["rpn/conv_cls/bias"], np.float32) + np.float32(0.6)     # enough detections to track
    return w


@pytest.fixture(scope="module")
def eng(pp, hip_lib):
    cfg = pp.config.tiny_config(S)
    cfg["model"]["second"]["num_class"] = 1
    e = pp.Engine(cfg, max_batch=S, max_points_per_frame=NMAX)
    e.load_weights(_weights(pp, e.d))
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng4(pp, hip_lib):
    e = pp.Engine(fc.config4(pp, S), max_batch=S, max_points_per_frame=NMAX)
    e.load_weights(pp.weights.init_weights(e.d, seed=7))
    yield e
    e.close()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _refused(eng, match, name, *args):
    """The C call itself (the Python layer's own checks are bypassed) must refuse with `match`."""
    with pytest.raises(RuntimeError, match=match):
        eng._check(getattr(eng._lib, name)(eng._h, *args), name)


def _cloud(seed, n, lo=(0.05, -0.6, -1.0), hi=(1.55, 0.6, 1.0)):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32))


# ---- the occupancy call ring ----
def test_nine_occupancy_updates_queued_back_to_back(pp, eng):
    eng.set_occupancy(OCC)
    eng.occupancy_reset()
    maps = [pp.occupancy.OccupancyMap(OCC) for _ in range(S)]
    frames = [_cloud(40 + b, n, (-1.7, -1.3, -0.3), (1.7, 1.3, 1.2)) for b, n in enumerate((300, 257, 64))]
    poses = [np.stack([pp.sweeps.pose_from_xyyaw(0.23 * k + 0.1 * b, -0.17 * k * (b - 1), 0.3 * k + 0.5 * b) for b in range(S)])
             for k in range(TURN)]
    eng.upload(frames)
    who = "pp_occupancy_update_async"
    for k, P in enumerate(poses):
        if k in (3, 5, 8):                       # refused between accepted calls: the cursor must stay
            bad = P.copy()
            bad[1, 0, 3] = np.inf
            _refused(eng, f"{who}: poses: stream 1: row 0, column 3 is not finite", who, _p(bad), S)
            _refused(eng, f"{who}: 3 frames are resident, batch is 2", who, _p(P), 2)
        eng.occupancy_update_async(P)
    want = None
    for P in poses:
        want = [maps[b].update(frames[b], P[b]) for b in range(S)]
    grid, org, lo = eng.occupancy_maps(logodds=True)
    info = eng.occupancy_info()
    for b in range(S):
        assert np.array_equal(lo[b], maps[b].logodds()), b
        assert np.array_equal(grid[b], maps[b].grid()), b
        assert tuple(org[b]) == maps[b].origin, b
    for k in ("hits", "ground", "ignored", "cells_hit", "cells_free", "cleared"):
        assert np.array_equal(info[k], np.array([w[k] for w in want], np.int32)), k
    assert all(w["hits"] > 0 and w["cells_free"] > 0 for w in want) and (lo != 0).any()
    eng.set_occupancy(None)


# ---- the handle's ring: offsets, crop planes, sweep poses and stamps ----
def _box_planes(lo, hi):
    """[6, 4]: a point stays where lo < p < hi on every axis (frustum.keep_mask: every plane's value negative)."""
    pl = np.zeros((6, 4), np.float64)
    for k in range(3):
        pl[2 * k, k], pl[2 * k, 3] = 1.0, -hi[k]
        pl[2 * k + 1, k], pl[2 * k + 1, 3] = -1.0, lo[k]
    return pl


def _round(pp, i, B):
    """Round i's own frames, planes, poses and stamps."""
    frames = [_cloud(1000 + 10 * i + b, 200 + 31 * ((i + b) % 4)) for b in range(B)]
    planes = np.stack([_box_planes((0.1 + 0.01 * i, -0.5 + 0.02 * b, -0.9), (1.5 - 0.02 * i, 0.55 - 0.01 * b, 0.8 + 0.01 * i))
                       for b in range(B)])
    poses = np.stack([pp.sweeps.pose_from_xyyaw(0.02 * i + 0.003 * b, -0.01 * i * (b + 1), 0.03 * i * (b + 1)) for b in range(B)])
    stamps = np.array([0.1 * i + b for b in range(B)])
    return frames, planes, poses, stamps


@pytest.mark.parametrize("B", [S, 5])
def test_nine_upload_crop_accumulate_rounds_then_a_synchronous_one(pp, hip_lib, B):
    """B = 3: upload_async feeds zero-copy, the ring carries planes and poses; B = 5: the frames travel by the copy stream,
    their offsets through the ring as well, and nothing on that path waits on the host."""
    sw = {"history": 8, "capacity": 300, "history_decimate": 1, "max_age": 100.0, "time_feature": -1}
    cfg = pp.config.tiny_config(B)
    e = pp.Engine(cfg, max_batch=B, max_points_per_frame=NMAX)
    e.load_weights(pp.weights.init_weights(e.d, seed=7))
    e.set_sweeps(sw)
    ref = pp.sweeps.SweepAccumulator(sw, B, 3, NMAX)
    rounds = [_round(pp, i, B) for i in range(TURN + 1)]
    stagings = [e.staging(r[0]) for r in rounds[:TURN]]
    who = "pp_sweeps_accumulate_async"
    for i, (frames, planes, poses, stamps) in enumerate(rounds[:TURN]):
        e.upload_async(stagings[i])
        e.crop_to_image_async(planes)
        if i in (2, 4, 7):                        # refused between accepted calls
            bad = poses.copy()
            bad[1, 2, 1] = np.nan
            _refused(e, f"{who}: poses: stream 1: row 2, column 1 is not finite", who, _p(bad), _p(stamps), B)
            _refused(e, f"{who}: {B} frames are resident, batch is 2", who, _p(poses), _p(stamps), 2)
            old = stamps.copy()
            old[2] = rounds[i - 1][3][2]
            _refused(e, f"{who}: stamps: the stamp of stream 2 does not increase", who, _p(poses), _p(old), B)
            # (a second crop is refused as well: the first left the frames' sizes on the device)
            _refused(e, "pp_frustum_crop_async: .*sizes are device values", "pp_frustum_crop_async", _p(planes), B, 0)
        e.accumulate_sweeps_async(poses, stamps)
    frames, planes, poses, stamps = rounds[TURN]
    e.upload(frames)
    kept, cropped = e.crop_to_image(planes, return_points=True)
    counts, pts = e.accumulate_sweeps(poses, stamps, return_points=True)
    info = e.sweeps_info()
    for fr, pl, P, st in rounds:
        host_cropped = [pp.frustum.crop_np(fr[b], pl[b]) for b in range(B)]
        want, winfo = ref.accumulate(host_cropped, P, st)
    assert kept.tolist() == [len(c) for c in host_cropped] and 0 < kept.min() and (kept < [len(f) for f in frames]).all()
    for b in range(B):
        assert cropped[b].tobytes() == host_cropped[b].tobytes(), b
        assert pts[b].shape == want[b].shape and pts[b].tobytes() == want[b].tobytes(), b
    assert np.array_equal(counts, winfo["count"])
    for k in ("count", "used", "truncated", "push_truncated"):
        assert np.array_equal(info[k], winfo[k]), k
    assert winfo["used"].tolist() == [8] * B and winfo["truncated"].sum() == 0      # eight of the nine asynchronous rounds
    e.sync()
    for st in stagings:
        st.close()
    e.close()


# ---- the ingest riders: frame records, feature tables, rig sources ----
def _read_back(pp, e, F, batch=S):
    """The resident (ingested) frames through a sweeps call on streams without history: the crop refuses frames whose
    sizes only the device knows, the accumulation hands them out as they are."""
    with pytest.raises(RuntimeError, match="sizes are device values"):
        e.crop_to_image(np.stack([_box_planes((-1e9,) * 3, (1e9,) * 3)] * batch))
    e.set_sweeps({"history": 1, "capacity": 16, "history_decimate": 1, "max_age": 1.0, "time_feature": -1})
    e.sweeps_reset()
    poses = np.stack([pp.sweeps.pose_from_xyyaw(0.0, 0.0, 0.0)] * batch)
    counts, pts = e.accumulate_sweeps(poses, np.zeros(batch), return_points=True)
    e.set_sweeps(None)
    assert all(p.shape == (c, F) for p, c in zip(pts, counts))
    return pts


def test_nine_feature_ingests_queued_back_to_back(pp, eng4):
    mount = fc.identity_mount(pp)
    calls = []
    for k in range(TURN):
        frames = fc.lidar_frames(pp, S, n=150 + 37 * k, frame0=10 * k)
        pairs = [fc.lidar_message(pp, f, ("velodyne", "reflectivity")[k % 2], seed=60 + 10 * k + b) for b, f in enumerate(frames)]
        msgs, feats = [m for m, _ in pairs], pairs[0][1]
        calls.append((msgs, feats, eng4.staging_pointcloud2(msgs, features=feats, mount=mount), k % 3, 1 + k % 2))
    for msgs, feats, st, first, decimate in calls:
        eng4.ingest_pointcloud2_async(st, first=first, decimate=decimate)
    info = eng4.ingest_info()
    got = _read_back(pp, eng4, 4)
    msgs, feats, _, first, decimate = calls[-1]
    for b in range(S):
        want, finite = pp.ingest.ingest_np(msgs[b], first, decimate, mount.lift, mount.matrices, feats)
        assert int(info["finite"][b]) == finite and int(info["kept"][b]) == len(want) > 0, b
        fc.assert_same_points(got[b], want, b)
    for c in calls:
        c[2].close()


def test_nine_rig_ingests_queued_back_to_back(pp, eng4):
    FF, M = pp.ingest.FeatureField, pp.ingest.Mount
    rigs = [pp.ingest.CameraRig([M.realsense(), fc.identity_mount(pp)], first=[1, 0], decimate=[2, 1]),
            pp.ingest.CameraRig([fc.identity_mount(pp), M.realsense(0.7)], first=[0, 2], decimate=[1, 3])]
    per = [[FF("intensity")], [FF("reflectivity", 1.0 / 255.0)]]
    calls = []
    for k in range(TURN):
        frames = []
        for b in range(S):
            a, r = fc.lidar_frames(pp, 2, n=120 + 23 * k + 5 * b, frame0=200 + 10 * k + 2 * b)
            frames.append([fc.lidar_message(pp, a, "velodyne", seed=300 + 10 * k + b)[0],
                           fc.lidar_message(pp, r, "reflectivity", seed=400 + 10 * k + b)[0]])
        calls.append((frames, rigs[k % 2], eng4.staging_rig_pointcloud2(frames, rigs[k % 2], features=per)))
    for frames, rig, st in calls:
        eng4.ingest_rig_pointcloud2_async(st, rig)
    info, src = eng4.ingest_info(), eng4.ingest_rig_info()
    got = _read_back(pp, eng4, 4)
    frames, rig, _ = calls[-1]
    for b in range(S):
        want, finite, kept = pp.ingest.rig_ingest_np(frames[b], rig, per)
        assert src["finite"][b].tolist() == finite.tolist() and src["kept"][b].tolist() == kept.tolist(), b
        assert int(info["finite"][b]) == int(finite.sum()) and int(info["kept"][b]) == len(want) > 0, b
        fc.assert_same_points(got[b], want, b)
    for c in calls:
        c[2].close()


def test_nine_depth_ingests_queued_back_to_back(pp, eng):
    calls = []
    for k in range(TURN):
        scenes = [depth_cases.scene(pp, 500 + 10 * k + b, 36 + 3 * k + b, 24 + k) for b in range(S)]
        images, ks = [s[0] for s in scenes], [s[1] for s in scenes]
        calls.append((images, ks, eng.staging_depth(images), k % 3, 2 + k % 3))
    for images, ks, st, first, decimate in calls:
        eng.ingest_depth_async(st, ks, first=first, decimate=decimate)
    info = eng.ingest_info()
    got = _read_back(pp, eng, 3)
    images, ks, _, first, decimate = calls[-1]
    for b in range(S):
        want, valid = pp.ingest.depth_ingest_np(images[b], ks[b], first, decimate, pp.ingest.SENSOR_HEIGHT)
        assert int(info["finite"][b]) == valid and int(info["kept"][b]) == len(want) > 0, b
        assert got[b].shape == want.shape and (depth_cases.bits(got[b]) == depth_cases.bits(want)).all(), b
    for c in calls:
        c[2].close()


# ---- the tracker's dt and pose rings ----
def test_nine_tracked_passes_each_with_its_own_dt_and_pose(pp, eng):
    cfg = pp.tracking.TrackConfig(gate=0.3, birth_score=0.0, max_misses=1, min_hits=2, size_alpha=0.3)
    eng.set_tracking(cfg)
    eng.track_reset()
    ref = pp.tracking.Tracker(cfg, S)
    frames = [_cloud(300 + b, 300 + 50 * b, (0.05, -0.6, -2.5), (1.3, 0.6, 2.5)) for b in range(S)]
    dts = [np.array([0.03 + 0.004 * k, 0.05 + 0.002 * k * k, 0.1 - 0.007 * k]) for k in range(TURN)]
    poses = [np.stack([pp.sweeps.pose_from_xyyaw(0.004 * k * (b + 1), -0.003 * k, 0.01 * k * (b + 1)) for b in range(S)])
             for k in range(TURN)]
    eng.upload(frames)
    for k in range(TURN):
        if k in (2, 6):                           # refused between accepted calls
            bad = poses[k].copy()
            bad[2, 1, 0] = np.nan
            with pytest.raises(RuntimeError, match="pp_set_track_pose: poses: stream 2: row 1, column 0 is not finite"):
                eng.set_track_pose(bad)
            with pytest.raises(RuntimeError, match="pp_set_track_dt: dt of stream 1 is 0"):
                eng.set_track_dt([0.1, 0.0, 0.1])
        eng.set_track_dt(dts[k])
        eng.set_track_pose(poses[k])
        eng.detect_async()
    eng.sync()
    dets, n = eng.detections()
    assert n.sum() > 0
    for k in range(TURN):                         # the passes are deterministic: every one had these rows
        want = ref.step(dets, n, dts[k], poses=poses[k])
    got, fixed, want_fixed = eng.tracks(S), eng.tracks_fixed(S), ref.tracks_fixed(S)
    for g, w in zip(got, want):
        assert np.array_equal(g, w) and g.tobytes() == w.tobytes()
    for g, w in zip(fixed, want_fixed):
        assert g.tobytes() == w.tobytes()
    assert want[1].sum() > 0 and (want[0]["hits"] >= 3).any()
    eng.set_tracking(None)
