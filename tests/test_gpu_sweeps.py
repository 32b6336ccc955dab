"""Multi-sweep accumulation on the GPU (csrc/sweeps.hip): pp_sweeps_accumulate* against sweeps.SweepAccumulator, bit for bit
-- the point tap, the counts and sweeps_info() after every call of a six-call sequence over 3 streams, for 3- and
4-feature rows, with chunk edges, empty frames and both truncations; the same sequence through ingest_pointcloud2 (sizes
known on the device only); the asynchronous chain against the synchronous one (zero-copy feed, and the copy feed that
voxelises at upload time); detections on the accumulated frames against a plain upload of the restatement's frames;
shorter calls; detect(poses=...); the refusals in C; an engine without set_sweeps."""
import copy
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NMAX, STREAMS = 512, 3
# frames of stream 0, 1, 2 in each of the six calls, drawn from {0, 1, 63, 64, 65, 257}: one and two chunks of 256 rows,
# a wave and one row either side of it, a single row, empty frames; 257 + 200 + 200 rows overflow the 512 of a frame
SIZES = [[257, 64, 0], [257, 65, 1], [257, 63, 257], [0, 257, 64], [65, 1, 257], [63, 0, 65]]
STAMPS = [0.0, 0.1, 0.2, 0.3, 0.5, 0.6]          # max_age 0.25: at call 4 only the newest stored sweep is young enough
# (point features, history_decimate, capacity, time_feature)
SETUPS = [(3, 1, 200, -1), (4, 1, 200, 3), (4, 3, 64, -1)]


def _config(pp, B, F):
    cfg = copy.deepcopy(pp.config.tiny_config(B))
    if F != 3:
        cfg["model"]["second"]["num_point_features"] = F
        for reader in ("eval_input_reader", "train_input_reader"):
            if reader in cfg:
                cfg[reader]["num_point_features"] = F
    return cfg


def _sweep_cfg(dec, cap, tf):
    return {"history": 2, "capacity": cap, "history_decimate": dec, "max_age": 0.25, "time_feature": tf}


def _engine(pp, F, B=STREAMS, sweeps=None, weights=False):
    eng = pp.Engine(_config(pp, B, F), max_batch=B, max_points_per_frame=NMAX)
    if weights:
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    if sweeps is not None:
        eng.set_sweeps(sweeps)
    return eng


def _sequence(F, streams=STREAMS, sizes=SIZES, seed=11):
    """[(frames, poses [B, 3, 4], stamps [B])] of the six calls: points inside tiny_config's range, a slow planar ego
    motion per stream, stamps per STAMPS (stream b offset by b seconds)."""
    from pp_amd import sweeps as S
    rng = np.random.default_rng(seed)
    calls = []
    for i, row in enumerate(sizes):
        frames = []
        for n in row[:streams]:
            f = rng.uniform([0.05, -0.6, -1.0], [1.55, 0.6, 1.0], size=(n, 3)).astype(np.float32)
            if F > 3:
                f = np.concatenate([f, rng.random((n, F - 3), dtype=np.float32)], axis=1)
            frames.append(np.ascontiguousarray(f))
        poses = np.stack([S.pose_from_xyyaw(0.02 * i + rng.normal() * 0.01, rng.normal() * 0.01, 0.03 * i * (b + 1))
                          for b in range(len(frames))])
        calls.append((frames, poses, np.array([STAMPS[i] + b for b in range(len(frames))])))
    return calls


def _same(got_pts, got_counts, got_info, want, winfo, tag):
    assert np.array_equal(got_counts, winfo["count"]), (tag, got_counts, winfo["count"])
    for k in ("count", "used", "truncated", "push_truncated"):
        assert got_info[k].tobytes() == winfo[k].tobytes(), (tag, k, got_info[k], winfo[k])
    for b, (g, w) in enumerate(zip(got_pts, want)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (tag, b)


@pytest.mark.parametrize("F,dec,cap,tf", SETUPS)
def test_six_calls_equal_the_restatement(pp, hip_lib, F, dec, cap, tf):
    eng = _engine(pp, F, sweeps=_sweep_cfg(dec, cap, tf))
    ref = pp.sweeps.SweepAccumulator(_sweep_cfg(dec, cap, tf), STREAMS, F, NMAX)
    assert eng.sweeps().to_dict() == ref.cfg.to_dict()
    seen = {"truncated": 0, "push_truncated": 0, "aged": False}
    for i, (frames, poses, stamps) in enumerate(_sequence(F)):
        want, winfo = ref.accumulate(frames, poses, stamps)
        eng.upload(frames)
        counts, pts = eng.accumulate_sweeps(poses, stamps, return_points=True)
        _same(pts, counts, eng.sweeps_info(), want, winfo, i)
        seen["truncated"] += int(winfo["truncated"].sum())
        seen["push_truncated"] += int(winfo["push_truncated"].sum())
        seen["aged"] |= bool(i >= 2 and (winfo["used"] < 2).any())
    assert seen["push_truncated"] > 0 and seen["aged"]                  # the sequence reaches the edges it is made for
    assert seen["truncated"] > 0 or cap * 2 + 257 <= NMAX
    eng.close()


@pytest.mark.parametrize("F", [3, 4])
def test_ingested_frames_sizes_on_the_device_only(pp, hip_lib, F):
    """The frames arrive as PointCloud2 messages: after the ingest the host holds bounds, the sizes are device values."""
    from pp_amd import ingest
    sw = _sweep_cfg(1, 200, 3 if F == 4 else -1)
    eng = _engine(pp, F, sweeps=sw)
    ref = pp.sweeps.SweepAccumulator(sw, STREAMS, F, NMAX)
    fields = [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1)] + ([("intensity", 12, 7, 1)] if F == 4 else [])
    feats = [ingest.FeatureField("intensity")] if F == 4 else None
    mount = ingest.Mount(np.eye(3), np.eye(3), 0.0)
    for i, (frames, poses, stamps) in enumerate(_sequence(F)):
        msgs = [(f.tobytes(), f.shape[0], 1, 4 * F, 4 * F * f.shape[0], fields) for f in frames]
        ing = eng.ingest_pointcloud2(msgs, first=0, decimate=1, features=feats, mount=mount, return_points=True)
        for f, g in zip(frames, ing):
            assert g.tobytes() == f.tobytes()                          # (an identity mount: the rows as they were packed)
        want, winfo = ref.accumulate(frames, poses, stamps)
        eng.ingest_pointcloud2(msgs, first=0, decimate=1, features=feats, mount=mount)
        assert eng._offsets is None                                    # nothing on the host knows the sizes
        counts, pts = eng.accumulate_sweeps(poses, stamps, return_points=True)
        _same(pts, counts, eng.sweeps_info(), want, winfo, i)
    eng.close()


def _dets_bytes(dets, n):
    return [dets[b, :n[b]].tobytes() for b in range(len(n))], n.copy()


@pytest.mark.parametrize("B", [3, 5])
def test_async_chain_equals_the_synchronous_one(pp, hip_lib, B):
    """B = 3: upload_async feeds zero-copy; B = 5: by the copy stream, which voxelises the batch at upload time -- the
    stage must voxelise its output again."""
    sizes = [(row * 2)[:B] for row in SIZES[:4]]
    seq = _sequence(4, streams=B, sizes=sizes)
    sw = _sweep_cfg(1, 200, 3)
    eng = _engine(pp, 4, B=B, sweeps=sw, weights=True)
    sync = []
    for frames, poses, stamps in seq:
        eng.upload(frames)
        counts = eng.accumulate_sweeps(poses, stamps)
        eng.detect_async()
        eng.sync()
        sync.append((_dets_bytes(*eng.detections()), counts, eng.sweeps_info()))
    eng.sweeps_reset()
    found = 0
    for (frames, poses, stamps), ((want, wn), wcounts, winfo) in zip(seq, sync):
        st = eng.staging(frames)
        eng.upload_async(st)
        eng.accumulate_sweeps_async(poses, stamps)
        eng.detect_async()
        eng.sync()
        got, n = _dets_bytes(*eng.detections())
        info = eng.sweeps_info()
        assert np.array_equal(info["count"], wcounts) and all(info[k].tobytes() == winfo[k].tobytes() for k in info)
        assert np.array_equal(n, wn) and got == want
        found += int(n.sum())
        st.close()
    assert found > 0                                                   # (the comparison is not between empty results)
    eng.close()


def test_detections_equal_a_plain_upload_of_the_restatement(pp, hip_lib):
    sw = _sweep_cfg(1, 200, 3)
    eng = _engine(pp, 4, sweeps=sw, weights=True)
    plain = _engine(pp, 4, weights=True)
    ref = pp.sweeps.SweepAccumulator(sw, STREAMS, 4, NMAX)
    found = 0
    for frames, poses, stamps in _sequence(4)[:4]:
        want_frames, _ = ref.accumulate(frames, poses, stamps)
        eng.upload(frames)
        eng.accumulate_sweeps(poses, stamps)
        eng.detect_async()
        eng.sync()
        got, n = _dets_bytes(*eng.detections())
        want, wn = _dets_bytes(*plain.detect(want_frames))
        assert np.array_equal(n, wn) and got == want
        found += int(n.sum())
    assert found > 0
    eng.close()
    plain.close()


def test_detect_with_poses_runs_the_stage_once(pp, hip_lib):
    sw = _sweep_cfg(1, 200, -1)
    eng = _engine(pp, 3, sweeps=sw, weights=True)
    plain = _engine(pp, 3, weights=True)
    ref = pp.sweeps.SweepAccumulator(sw, STREAMS, 3, NMAX)
    for i, (frames, poses, stamps) in enumerate(_sequence(3)[:3]):
        want_frames, winfo = ref.accumulate(frames, poses, stamps)
        got, n = _dets_bytes(*eng.detect(frames, poses=poses, stamps=stamps))
        want, wn = _dets_bytes(*plain.detect(want_frames))
        assert np.array_equal(n, wn) and got == want
        assert eng.sweeps_info()["used"].tobytes() == winfo["used"].tobytes()
    with pytest.raises(ValueError, match="poses needs stamps"):
        eng.detect(frames, poses=poses)
    with pytest.raises(ValueError, match="stream 0 does not increase"):
        eng.detect(frames, poses=poses, stamps=stamps)                # refused before anything is queued ...
    later = stamps + 1.0
    want_frames, _ = ref.accumulate(frames, poses, later)
    got, n = _dets_bytes(*eng.detect(frames, poses=poses, stamps=later))   # ... so the history is as it was
    want, wn = _dets_bytes(*plain.detect(want_frames))
    assert np.array_equal(n, wn) and got == want
    eng.close()
    plain.close()


def test_a_shorter_call_leaves_the_other_streams_alone(pp, hip_lib):
    sw = _sweep_cfg(1, 200, -1)
    eng = _engine(pp, 3, sweeps=sw)
    ref = pp.sweeps.SweepAccumulator(sw, STREAMS, 3, NMAX)
    seq = _sequence(3)
    plan = [(seq[0], 3), (seq[1], 3), (seq[2], 1), (seq[3], 3), (seq[4], 2), (seq[5], 3)]
    for i, ((frames, poses, stamps), B) in enumerate(plan):
        frames, poses, stamps = frames[:B], poses[:B], stamps[:B]
        want, winfo = ref.accumulate(frames, poses, stamps)
        eng.upload(frames)
        counts, pts = eng.accumulate_sweeps(poses, stamps, return_points=True)
        _same(pts, counts, eng.sweeps_info(), want, winfo, i)
    eng.sweeps_reset(1)                                                # one stream forgets, the others keep their sweeps
    ref.reset(1)
    frames, poses, stamps = seq[5]
    stamps = stamps + 0.1
    want, winfo = ref.accumulate(frames, poses, stamps)
    assert winfo["used"].tolist()[1] == 0 and winfo["used"].tolist()[0] > 0
    eng.upload(frames)
    counts, pts = eng.accumulate_sweeps(poses, stamps, return_points=True)
    _same(pts, counts, eng.sweeps_info(), want, winfo, "reset")
    eng.close()


def _c_call(eng, poses, stamps, B):
    P, S = np.ascontiguousarray(poses, np.float64), np.ascontiguousarray(stamps, np.float64)
    counts = np.zeros(B, np.int32)
    st = eng._lib.pp_sweeps_accumulate(eng._h, P.ctypes.data_as(ctypes.c_void_p), S.ctypes.data_as(ctypes.c_void_p), B,
                                       counts.ctypes.data_as(ctypes.c_void_p), None, ctypes.c_int64(0))
    return st, eng._lib.pp_last_error(eng._h).decode()


def test_refused_in_c_before_anything_is_queued(pp, hip_lib):
    eng = _engine(pp, 3, sweeps=_sweep_cfg(1, 200, -1))
    (frames, poses, stamps), (_, poses1, stamps1) = _sequence(3)[:2]
    eng.upload(frames)
    eng.accumulate_sweeps(poses, stamps)
    eng.upload(frames)
    bad_stamp = stamps1.copy()
    bad_stamp[2] = stamps[2]
    st, msg = _c_call(eng, poses1, bad_stamp, 3)
    assert st == 1 and "stream 2" in msg and "increase" in msg
    bad = poses1.copy()
    bad[1, 0, 0] += 0.01
    st, msg = _c_call(eng, bad, stamps1, 3)
    assert st == 1 and "stream 1" in msg and "orthonormal" in msg
    bad = poses1.copy()
    bad[0, 2, 3] = np.nan
    st, msg = _c_call(eng, bad, stamps1, 3)
    assert st == 1 and "stream 0" in msg and "finite" in msg
    st, msg = _c_call(eng, poses1[:2], stamps1[:2], 2)
    assert st == 1 and "3 frames are resident" in msg
    with pytest.raises(RuntimeError, match="time_feature"):             # the C side's own check (Python's is bypassed)
        pc = pp._lib.PPSweepConfig(max_age=1.0, history=2, capacity=0, history_decimate=1, time_feature=3)
        eng._check(eng._lib.pp_set_sweeps(eng._h, ctypes.byref(pc)), "pp_set_sweeps")
    with pytest.raises(ValueError, match="time_feature"):
        eng.set_sweeps({"time_feature": 3})
    # none of the refused calls touched the frames or the history: the next call is the restatement's second
    ref = pp.sweeps.SweepAccumulator(_sweep_cfg(1, 200, -1), STREAMS, 3, NMAX)
    ref.accumulate(frames, poses, stamps)
    want, winfo = ref.accumulate(frames, poses1, stamps1)
    counts, pts = eng.accumulate_sweeps(poses1, stamps1, return_points=True)
    _same(pts, counts, eng.sweeps_info(), want, winfo, "after refusals")
    eng.close()


def test_an_engine_without_set_sweeps_refuses_and_is_unchanged(pp, hip_lib):
    eng = _engine(pp, 3, weights=True)
    frames, poses, stamps = _sequence(3)[0]
    assert eng.sweeps() is None
    before = _dets_bytes(*eng.detect(frames))
    with pytest.raises(RuntimeError, match="not configured"):
        eng.accumulate_sweeps(poses, stamps)
    with pytest.raises(RuntimeError, match="not configured"):
        eng.detect(frames, poses=poses, stamps=stamps)
    st, msg = _c_call(eng, poses, stamps, 3)
    assert st == 2 and "not configured" in msg                         # PP_ERR_STATE
    eng.detect_async()                                                 # the frames are still resident, as uploaded
    eng.sync()
    after = _dets_bytes(*eng.detections())
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    eng.set_sweeps(True)                                               # the shipped defaults; capacity: max_points_per_frame
    assert eng.sweeps().capacity == NMAX and eng.sweeps().history == 4
    eng.set_sweeps(None)
    assert eng.sweeps() is None
    eng.close()
