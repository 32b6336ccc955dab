"""PointCloud2 feature fields through the GPU rig ingest (csrc/ingest.hip: k_rig_scatter_f,
pp_ingest_rig_pointcloud2_fields*): several sources per frame, each under its own mount, selection and feature layout,
against ingest.rig_ingest_np(..., features) -- bit for bit, NaN by class.  One source per frame against the plain call,
three sources with three layouts, chunk and scan boundaries, the asynchronous call and the refusals.  No test provokes a
fault: every refusal is decided on the host before a launch."""
import ctypes

import numpy as np
import pytest

import pc2_feature_cases as fc

pytestmark = pytest.mark.gpu

B_MAX = 3
NMAX = 36000          # a 260 x 128 source at (0, 1) keeps up to 33280 points, the sources beside it a few hundred


@pytest.fixture(scope="module")
def eng(pp, hip_lib):
    e = pp.Engine(fc.config4(pp, B_MAX), max_batch=B_MAX, max_points_per_frame=NMAX)
    e.load_weights(pp.weights.init_weights(e.d, seed=7))
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(pp):
    return fc.feature_cases(pp)


def _three_mounts(pp):
    ing = pp.ingest
    r, r2 = ing._matrices()
    a = np.deg2rad(40.0)
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ \
        np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    T[:3, 3] = [0.05, -0.2, 0.9]
    return [ing.Mount.realsense(), ing.Mount.from_matrix(T), ing.Mount(r, r2, [0.1, 0.15, 0.7])]


def _check(pp, eng, frames, rig, features, what):
    """One ingest_rig_pointcloud2(features=...) call against the host rule: the frames' points, their sums, the sources'
    counts."""
    got = eng.ingest_rig_pointcloud2(frames, rig, return_points=True, features=features)
    info, per = eng.ingest_info(), eng.ingest_rig_info()
    assert len(got) == len(frames) and per["kept"].shape == (len(frames), len(rig))
    for b, fr in enumerate(frames):
        with np.errstate(over="ignore"):
            want, fin, kept = pp.ingest.rig_ingest_np(fr, rig, features)
        assert per["finite"][b].tolist() == fin.tolist() and per["kept"][b].tolist() == kept.tolist(), (what, b, per, fin, kept)
        assert int(info["finite"][b]) == int(fin.sum()) and int(info["kept"][b]) == len(want), (what, b)
        fc.assert_same_points(got[b], want, (what, b))
    return got


def test_one_source_per_frame_equals_the_plain_call(pp, eng, cases):
    names = ["float32_after", "bigendian_float32", "velodyne"]       # three layouts of one field name
    msgs = [cases[n][0] for n in names]
    feats = [pp.ingest.FeatureField("intensity", 1.0 / 255.0, 0.01)]
    rig = pp.ingest.CameraRig([pp.ingest.Mount.realsense()])
    want = eng.ingest_pointcloud2(msgs, return_points=True, features=feats)
    iw = {k: v.copy() for k, v in eng.ingest_info().items()}
    got = _check(pp, eng, [[m] for m in msgs], rig, feats, "one source")
    info, per = eng.ingest_info(), eng.ingest_rig_info()
    for b in range(3):
        assert got[b].shape == want[b].shape and got[b].shape[1] == 4
        fc.assert_same_points(got[b], want[b], ("plain", b))
    for k in ("finite", "kept"):
        assert info[k].tolist() == iw[k].tolist() == per[k].reshape(-1).tolist(), k


def test_three_sources_three_mounts_three_feature_layouts(pp, eng, cases):
    FF = pp.ingest.FeatureField
    frames = [[cases["velodyne"][0], cases["bigendian_int16"][0], cases["constant"][0]],
              [cases["unaligned_13_of_29"][0], cases["int8_before"][0], cases["nonfinite_feature_f32"][0]]]
    per = [[FF("intensity", 1.0 / 255.0)], [FF("i", 0.25, 1.0)], [FF.constant(0.3)]]
    rig = pp.ingest.CameraRig(_three_mounts(pp), first=[1, 0, 2], decimate=[4, 1, 3])
    got = _check(pp, eng, frames, rig, per, "three sources")
    kept = eng.ingest_rig_info()["kept"]
    assert (kept > 0).all()
    # the constant column sits behind the third source's points only
    assert (got[0][-kept[0, 2]:, 3] == np.float32(0.3)).all() and not (got[0][:kept[0, 0], 3] == np.float32(0.3)).any()
    _check(pp, eng, frames[::-1], rig, per, "three sources, frames swapped")       # (the other input buffer)
    # x y z, the counts and the offsets are the rig's x y z ingest on a 3-feature engine
    eng3 = pp.Engine(pp.config.tiny_config(2), max_batch=2, max_points_per_frame=NMAX)
    xyz = eng3.ingest_rig_pointcloud2(frames[::-1], rig, return_points=True)
    again = eng.ingest_rig_pointcloud2(frames[::-1], rig, return_points=True, features=per)
    assert np.array_equal(eng3.ingest_rig_info()["kept"], eng.ingest_rig_info()["kept"])
    for b in range(2):
        assert np.array_equal(again[b][:, :3], xyz[b]), b
    eng3.close()


def _message(pp, rng, w, h, nan_fraction, seed, kind):
    n = w * h
    xyz = rng.uniform(-3.0, 6.0, (n, 3))
    bad = rng.random(n) < nan_fraction
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = np.nan
    if kind == 0:
        col, fields, kw = rng.uniform(0.0, 1.0, n).astype(np.float32), [("intensity", 7, 16)], dict(point_step=32)
    elif kind == 1:
        col, fields, kw = rng.integers(0, 65536, n), [("intensity", 4, 13)], dict(point_step=15, row_pad=3)
    else:
        col, fields, kw = rng.uniform(-1.0, 1.0, n), [("intensity", 8, 3)], dict(point_step=23, offsets=(11, 15, 19), bigendian=True)
    return pp.synth.pointcloud2_from_points(np.column_stack([xyz, col]), w, h, feature_fields=fields, seed=seed, **kw)


def test_chunk_and_scan_boundaries(pp, eng):
    """Sources of 511, 512 and 513 records in one frame, with and without holes, at every selection; a source of 260 x 128
    records (65 chunks: the wave scan carries once) between two small ones."""
    rng = np.random.default_rng(43)
    FF = pp.ingest.FeatureField
    mounts = _three_mounts(pp)
    per = [[FF("intensity")], [FF("intensity", 1.0 / 65535.0, 0.1)], [FF("intensity", 3.0, -0.5)]]
    sizes = [(511, 1), (64, 8), (27, 19)]
    assert [w * h for w, h in sizes] == [511, 512, 513]
    for first, decimate in fc.SELECTIONS:
        rig = pp.ingest.CameraRig(mounts, first=first, decimate=decimate)
        for nan_fraction in (0.0, 0.3):
            fr = [_message(pp, rng, w, h, nan_fraction, c, c) for c, (w, h) in enumerate(sizes)]
            _check(pp, eng, [fr], rig, per, ("511/512/513", first, decimate, nan_fraction))
    rig = pp.ingest.CameraRig(mounts, first=[0, 0, 3], decimate=[1, 1, 7])
    fr = [_message(pp, rng, 31, 17, 0.3, 5, 1), _message(pp, rng, 260, 128, 0.2, 6, 0), _message(pp, rng, 8, 6, 0.3, 7, 2)]
    _check(pp, eng, [fr], rig, [per[1], per[0], per[2]], "65 chunks")
    # a frame whose middle source keeps nothing, beside a frame that keeps nothing at all
    nothing = _message(pp, rng, 27, 19, 1.1, 8, 1)
    frames = [[fr[0], nothing, fr[2]], [nothing, nothing, nothing]]
    rig = pp.ingest.CameraRig(mounts, first=[0, 1, 2], decimate=[1, 4, 3])
    _check(pp, eng, frames, rig, [per[1], per[1], per[2]], "empty sources")
    assert eng.ingest_info()["kept"][1] == 0


def _same_detections(a, b, what):
    (da, na), (db, nb) = a, b
    assert np.array_equal(na, nb), (what, na, nb)
    for f in range(len(na)):
        assert da[f, :na[f]].tobytes() == db[f, :nb[f]].tobytes(), (what, f)


def test_asynchronous_rig_feed_equals_the_synchronous_one(pp, eng):
    """staging_rig_pointcloud2(features=...) + ingest_rig_pointcloud2_async + detect_async against detect_rig_pointcloud2,
    and against Engine.detect on the host-concatenated frames (two lidars under identity mounts, one without intensity)."""
    B = 2
    FF = pp.ingest.FeatureField
    clouds = [fc.lidar_frames(pp, 2, n, frame0=50 + 2 * b) for b, n in enumerate((700, 900))]
    frames = [[fc.lidar_message(pp, clouds[b][0], "velodyne", seed=b)[0], fc.lidar_message(pp, clouds[b][1], "reflectivity", seed=9 + b)[0]]
              for b in range(B)]
    per = [[FF("intensity")], [FF.constant(0.25)]]
    rig = pp.ingest.CameraRig([fc.identity_mount(pp)] * 2, first=0, decimate=1)
    host = []
    for b in range(B):
        second = clouds[b][1].copy()
        second[:, 3] = np.float32(0.25)
        host.append(np.concatenate([clouds[b][0], second]))
    want = eng.detect(host)
    want = (want[0].copy(), want[1].copy())
    iw = eng.intermediates()
    assert int(iw["n_pillars"][:B].min()) > 0
    got = eng.ingest_rig_pointcloud2(frames, rig, return_points=True, features=per)
    for b in range(B):
        assert got[b].tobytes() == host[b].tobytes(), b
    sync = eng.detect_rig_pointcloud2(frames, rig, features=per)
    _same_detections(sync, want, "rig messages vs host frames")
    st = eng.staging_rig_pointcloud2(frames, rig, features=per)
    other = eng.staging(fc.lidar_frames(pp, B, 800, frame0=60))
    eng.upload_async(other)
    eng.detect_async()
    eng.ingest_rig_pointcloud2_async(st, rig)              # queued while the pass on the uploaded frames is in flight
    eng.detections()
    eng.detect_async()
    d, n = eng.detections()
    _same_detections((d, n), want, "asynchronous rig feed")
    im = eng.intermediates()
    assert np.array_equal(im["n_pillars"], iw["n_pillars"]) and im["box_preds"].tobytes() == iw["box_preds"].tobytes()
    assert eng.ingest_rig_info()["kept"].tolist() == [[700, 700], [900, 900]]
    eng.sync()
    st.close()
    other.close()


def test_rig_refusals_name_the_source_and_the_feature(pp, eng, cases):
    from pp_amd import _lib, engine
    PP_ERR_ARG = 1
    good = cases["constant"][0]
    lay = pp.ingest.layout_of(good)
    data = np.frombuffer(good[0], np.uint8)
    S, B = 3, 2
    both = np.ascontiguousarray(np.concatenate([data] * S))
    offs = np.arange(S + 1, dtype=np.int64) * data.size
    fmap = np.array([0, 0, 1], np.int32)
    arr = (_lib.PPPc2Layout * S)()
    for s in range(S):
        for k, v in lay.items():
            setattr(arr[s], k, v)
    cfgs = (_lib.PPIngestConfig * S)()
    for s in range(S):
        c = engine._ingest_config(1, 4, 1.0)
        ctypes.memmove(ctypes.byref(cfgs[s]), ctypes.byref(c), ctypes.sizeof(c))
    ok = (16, 7, 1.0, 0.0)

    def call(feats, nfeat, asynchronous, null=False):
        tab = (_lib.PPPc2Feature * max(len(feats), 1))()
        for i, (off, typ, scale, bias) in enumerate(feats):
            tab[i].offset, tab[i].datatype, tab[i].scale, tab[i].bias = off, typ, scale, bias
        args = [eng._h, both.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p), arr, cfgs,
                fmap.ctypes.data_as(ctypes.c_void_p), S, B, None if null else tab, nfeat]
        if asynchronous:
            st = eng._lib.pp_ingest_rig_pointcloud2_fields_async(*args)
        else:
            st = eng._lib.pp_ingest_rig_pointcloud2_fields(*args, None, 0)
        return st, (eng._lib.pp_last_error(eng._h) or b"").decode()

    assert call([ok] * S, 1, False)[0] == 0
    frames = fc.lidar_frames(pp, B, 900, frame0=70)
    want = eng.detect(frames)
    want = (want[0].copy(), want[1].copy())
    nan = float("nan")
    refusals = [
        ([ok] * S, 1, True, ["features is NULL", "nfeat is 1"]),
        ([], 0, False, ["nfeat 0", "num_point_features is 4"]),
        ([ok] * 2 * S, 2, False, ["nfeat 2", "num_point_features is 4"]),
        ([ok, ok, (16, 12, 1.0, 0.0)], 1, False, ["source 2", "feature 0", "unknown datatype 12"]),
        ([ok, (18, 7, 1.0, 0.0), ok], 1, False, ["source 1", "feature 0", "offset 18 (4 bytes)", "point_step 20"]),
        ([(-4, 3, 1.0, 0.0), ok, ok], 1, False, ["source 0", "feature 0", "offset -4"]),
        ([ok, ok, (16, 7, 1.0, nan)], 1, False, ["source 2", "feature 0", "bias", "not finite"]),
        ([ok, (16, 7, -float("inf"), 0.0), ok], 1, False, ["source 1", "feature 0", "scale", "not finite"]),
    ]
    for asynchronous in (False, True):
        for feats, nfeat, null, words in refusals:
            st, msg = call(feats, nfeat, asynchronous, null)
            assert st == PP_ERR_ARG, (feats, nfeat, st, msg)
            for w in words:
                assert w in msg, (w, msg)
            assert ("pp_ingest_rig_pointcloud2_fields_async" in msg) == asynchronous, msg
    # what the twin call refuses: the frame map
    fmap[:] = [0, 1, 1]
    fmap[0] = 1
    st, msg = call([ok] * S, 1, False)
    assert st == PP_ERR_ARG and "the frame map starts at frame 0" in msg, msg
    fmap[:] = [0, 0, 1]
    # the x y z rig calls still refuse the 4-feature engine, as do the depth calls
    rig = pp.ingest.CameraRig([pp.ingest.Mount.realsense()])
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*num_point_features is 4"):
        eng.ingest_rig_pointcloud2([[good]], rig)
    with pytest.raises(ValueError, match="no field 'intensity'"):
        eng.ingest_rig_pointcloud2([[good]], rig, features=[pp.ingest.FeatureField("intensity")])
    _same_detections(eng.detect(frames), want, "detect after the refusals")
