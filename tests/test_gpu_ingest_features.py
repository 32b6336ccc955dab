"""PointCloud2 feature fields through the GPU ingest (csrc/ingest.hip: k_ingest_scatter_f, pp_ingest_pointcloud2_fields*):
rows of x y z + intensity for a 4-feature model, against ingest.ingest_np(..., features=...) -- bit for bit, NaN by class
--, against the 3-feature engine's x y z ingest, the lidar round trip into detections, asynchronous feeds with different
feature tables, and every refusal.  No test provokes a fault: every refusal is decided on the host before a launch."""
import ctypes

import numpy as np
import pytest

import pc2_cases
import pc2_feature_cases as fc

pytestmark = pytest.mark.gpu

NMAX = 4096         # a 64 x 48 message at (0, 1) keeps up to 3072 points


@pytest.fixture(scope="module")
def cases(pp):
    return fc.feature_cases(pp)


@pytest.fixture(scope="module")
def wants(pp, cases):
    """The host result of every case at every selection, computed once: (first, decimate) -> name -> (points, finite)."""
    out = {}
    for first, decimate in fc.SELECTIONS:
        with np.errstate(over="ignore"):
            out[(first, decimate)] = {n: pp.ingest.ingest_np(m, first, decimate, features=f) for n, (m, f) in cases.items()}
    return out


def _engine(pp, B, F=4, nmax=NMAX, weights=False):
    eng = pp.Engine(fc.config4(pp, B) if F == 4 else pp.config.tiny_config(B), max_batch=B, max_points_per_frame=nmax)
    if weights:
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    return eng


def _check(eng, cases, wants, names, first, decimate):
    msgs, feats = [cases[n][0] for n in names], [cases[n][1] for n in names]
    got = eng.ingest_pointcloud2(msgs, first=first, decimate=decimate, return_points=True, features=feats)
    info = eng.ingest_info()
    assert len(got) == len(names)
    for b, name in enumerate(names):
        want, n_finite = wants[(first, decimate)][name]
        assert int(info["finite"][b]) == n_finite and int(info["kept"][b]) == len(want), (name, first, decimate, info)
        fc.assert_same_points(got[b], want, (name, first, decimate))
    return got, info


@pytest.mark.parametrize("first,decimate", fc.SELECTIONS)
def test_every_case_alone_equals_the_host_rule(pp, hip_lib, cases, wants, first, decimate):
    eng = _engine(pp, 1)
    for name in cases:
        _check(eng, cases, wants, [name], first, decimate)
    eng.close()


@pytest.mark.parametrize("first,decimate", fc.SELECTIONS)
def test_all_cases_mixed_in_one_batch_and_xyz_equal_the_three_feature_engine(pp, hip_lib, cases, wants, first, decimate):
    names = list(cases)
    eng = _engine(pp, len(names))
    eng3 = _engine(pp, len(names), F=3)
    for order in (names, names[::-1]):             # (the other order lands in the other input buffer)
        got, info = _check(eng, cases, wants, order, first, decimate)
        xyz = eng3.ingest_pointcloud2([cases[n][0] for n in order], first=first, decimate=decimate, return_points=True)
        info3 = eng3.ingest_info()
        assert np.array_equal(info["finite"], info3["finite"]) and np.array_equal(info["kept"], info3["kept"])
        for b, name in enumerate(order):
            assert xyz[b].shape == (len(got[b]), 3), name
            assert np.array_equal(got[b][:, :3], xyz[b]), name
    eng.close()
    eng3.close()


def test_no_feature_on_a_three_feature_engine_is_the_existing_call(pp, hip_lib):
    lay = pc2_cases.layout_cases(pp)
    names = ["d435i_ps20_padded_rows", "bigendian_f64_unaligned", "one_row_partial_chunk", "finite_1", "special_values_f32"]
    msgs = [lay[n] for n in names]
    eng = _engine(pp, len(msgs), F=3)
    for first, decimate in fc.SELECTIONS:
        want = eng.ingest_pointcloud2(msgs, first=first, decimate=decimate, return_points=True)
        iw = {k: v.copy() for k, v in eng.ingest_info().items()}
        got = eng.ingest_pointcloud2(msgs, first=first, decimate=decimate, return_points=True, features=[])
        ig = eng.ingest_info()
        assert np.array_equal(iw["finite"], ig["finite"]) and np.array_equal(iw["kept"], ig["kept"])
        for b, name in enumerate(names):
            assert got[b].shape == want[b].shape and got[b].tobytes() == want[b].tobytes(), (name, first, decimate)
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*nfeat 1, num_point_features is 3"):
        eng.ingest_pointcloud2(msgs[:1], features=[pp.ingest.FeatureField.constant(1.0)])
    eng.close()


def _same_detections(a, b, what):
    (da, na), (db, nb) = a, b
    assert np.array_equal(na, nb), (what, na, nb)
    for f in range(len(na)):
        assert da[f, :na[f]].tobytes() == db[f, :nb[f]].tobytes(), (what, f)


def _same_intermediates(ia, ib, what):
    assert np.array_equal(ia["n_pillars"], ib["n_pillars"]), (what, ia["n_pillars"], ib["n_pillars"])
    for f, P in enumerate(ia["n_pillars"]):
        assert np.array_equal(ia["coors"][f, :P], ib["coors"][f, :P]), (what, f)
        assert np.array_equal(ia["num_points"][f, :P], ib["num_points"][f, :P]), (what, f)
    for k in ("anchors_mask", "box_preds", "cls_preds", "dir_cls_preds"):
        assert ia[k].tobytes() == ib[k].tobytes(), (what, k)


def _calib(pp, B):
    rect, trv, _ = pp.synth.default_calib()
    return np.stack([rect] * B), np.stack([trv] * B)


def test_lidar_round_trip_into_detections(pp, hip_lib):
    """A KITTI-shaped [N, 4] array packed as the message a lidar driver publishes and ingested under the identity mount
    comes back byte for byte, and detect_pointcloud2 on the messages is Engine.detect on the arrays."""
    B = 2
    frames = fc.lidar_frames(pp, B, 1500)                 # 1500 records: three chunks, the last one partial
    packed = [fc.lidar_message(pp, f, "velodyne", seed=50 + b) for b, f in enumerate(frames)]
    msgs, feats = [m for m, _ in packed], packed[0][1]
    mount = fc.identity_mount(pp)
    eng = _engine(pp, B, nmax=2048, weights=True)
    got = eng.ingest_pointcloud2(msgs, first=0, decimate=1, return_points=True, features=feats, mount=mount)
    assert eng.ingest_info()["kept"].tolist() == [1500] * B
    for b in range(B):
        assert got[b].shape == (1500, 4) and got[b].tobytes() == frames[b].tobytes(), b
    R, T = _calib(pp, B)
    want = eng.detect(frames, R, T)
    want = (want[0].copy(), want[1].copy())
    iw = eng.intermediates()
    assert int(iw["n_pillars"].min()) > 0
    det = eng.detect_pointcloud2(msgs, R, T, features=feats, mount=mount, first=0, decimate=1)
    assert np.array_equal(det[1], want[1]) and np.array_equal(det[0], want[0])
    _same_detections(det, want, "messages vs arrays")
    _same_intermediates(eng.intermediates(), iw, "messages vs arrays")
    # the intensity column reaches the network: another constant in its place changes the pillar features' products
    other = eng.detect_pointcloud2(msgs, R, T, features=[pp.ingest.FeatureField.constant(0.9)], mount=mount, first=0, decimate=1)
    io = eng.intermediates()
    assert np.array_equal(io["n_pillars"], iw["n_pillars"]) and io["box_preds"].tobytes() != iw["box_preds"].tobytes()
    assert other[1].shape == want[1].shape
    eng.close()


def test_voxelnet_detect_pointcloud2_with_features(pp, hip_lib):
    B = 2
    frames = fc.lidar_frames(pp, B, 1500, frame0=4)
    packed = [fc.lidar_message(pp, f, "velodyne") for f in frames]
    msgs, feats = [m for m, _ in packed], packed[0][1]
    net = pp.VoxelNet(fc.config4(pp, B), max_batch=B, max_points_per_frame=2048)
    net.load_weights(pp.weights.init_weights(net.d, seed=7))
    R, T = _calib(pp, B)
    want = net.detect(frames, R, T, image_idx=[7, 8])
    got = net.detect_pointcloud2(msgs, R, T, image_idx=[7, 8], features=feats, mount=fc.identity_mount(pp), first=0, decimate=1)
    for g, w in zip(got, want):
        assert g.keys() == w.keys() and g["batch_idx"] == w["batch_idx"]
        for k in w:
            assert (g[k] is None) == (w[k] is None), k
            if w[k] is not None:
                assert np.array_equal(g[k], w[k]), k
    net.engine.close()


def test_asynchronous_feeds_with_different_feature_tables(pp, hip_lib):
    """Two MessageStagings with different feature tables (FLOAT32 intensity at 16 of 32; UINT8 reflectivity / 255 at 12 of
    16) fed back to back through ingest_pointcloud2_async + detect_async with no sync in between, mixed with one
    upload_async: every pass equals its synchronous feed byte for byte."""
    B = 2
    mount = fc.identity_mount(pp)
    fa, fb, fcc = (fc.lidar_frames(pp, B, n, frame0=k) for n, k in ((1500, 10), (1100, 20), (1300, 30)))
    pa = [fc.lidar_message(pp, f, "velodyne", seed=60 + b) for b, f in enumerate(fa)]
    pb = [fc.lidar_message(pp, f, "reflectivity", seed=70 + b) for b, f in enumerate(fb)]
    msgs_a, feats_a, msgs_b, feats_b = [m for m, _ in pa], pa[0][1], [m for m, _ in pb], pb[0][1]
    eng = _engine(pp, B, nmax=2048, weights=True)
    kw = dict(first=0, decimate=1)

    def snap():
        d, n = eng.detections()
        return (d.copy(), n.copy()), eng.intermediates()

    want = []
    for feed in (lambda: eng.ingest_pointcloud2(msgs_a, features=feats_a, mount=mount, **kw),
                 lambda: eng.ingest_pointcloud2(msgs_b, features=feats_b, mount=mount, **kw),
                 lambda: eng.upload(fcc)):
        feed()
        eng.detect_async()
        eng.sync()
        want.append(snap())
    assert all(int(w[1]["n_pillars"].min()) > 0 for w in want)
    assert want[0][1]["box_preds"].tobytes() != want[1][1]["box_preds"].tobytes()
    # the reflectivity messages under the other staging's table would be refused or read garbage: the tables are distinct
    assert [tuple(t) for t in (pp.ingest.feature_layout_of(msgs_a[0], feats_a)[0], pp.ingest.feature_layout_of(msgs_b[0], feats_b)[0])] \
        == [(16, 7, 1.0, 0.0), (12, 2, 1.0 / 255.0, 0.0)]

    st_a = eng.staging_pointcloud2(msgs_a, features=feats_a, mount=mount)
    st_b = eng.staging_pointcloud2(msgs_b, features=feats_b, mount=mount)
    st_c = eng.staging(fcc)
    assert st_a.nfeat == st_b.nfeat == 1
    for rnd in range(2):
        eng.ingest_pointcloud2_async(st_a, **kw)
        eng.detect_async()
        eng.ingest_pointcloud2_async(st_b, **kw)       # queued while pass a is in flight: the other ring slot, the same table
        got_a = snap()
        eng.detect_async()
        eng.upload_async(st_c)
        got_b = snap()
        eng.detect_async()
        got_c = snap()
        for k, got in enumerate((got_a, got_b, got_c)):
            _same_detections(got[0], want[k][0], (rnd, "abc"[k]))
            _same_intermediates(got[1], want[k][1], (rnd, "abc"[k]))
    # two ingests with nothing between them: the second one's frames are the resident ones
    eng.ingest_pointcloud2_async(st_a, **kw)
    eng.ingest_pointcloud2_async(st_b, **kw)
    eng.detect_async()
    got = snap()
    _same_detections(got[0], want[1][0], "a then b")
    _same_intermediates(got[1], want[1][1], "a then b")
    assert eng.ingest_info()["kept"].tolist() == [1100] * B
    # features given with the call instead of the staging
    st_plain = eng.staging_pointcloud2(msgs_a)
    assert st_plain.features is None
    eng.ingest_pointcloud2_async(st_plain, features=feats_a, mount=mount, **kw)
    eng.detect_async()
    _same_detections(snap()[0], want[0][0], "features with the call")
    eng.sync()
    for s in (st_a, st_b, st_c, st_plain):
        s.close()
    eng.close()


def _raw_fields(eng, data, offs, layouts, feats, nfeat, first=1, decimate=4, asynchronous=False, null_features=False):
    """The C-ABI call itself, with a table the Python layer would not let through.  feats: (offset, datatype, scale, bias)
    per frame and feature."""
    from pp_amd import _lib, engine
    arr = (_lib.PPPc2Layout * len(layouts))()
    for b, lay in enumerate(layouts):
        for k, v in lay.items():
            setattr(arr[b], k, v)
    tab = (_lib.PPPc2Feature * max(len(feats), 1))()
    for i, (off, typ, scale, bias) in enumerate(feats):
        tab[i].offset, tab[i].datatype, tab[i].scale, tab[i].bias = off, typ, scale, bias
    cfg = engine._ingest_config(first, decimate, 1.0)
    data = np.ascontiguousarray(data, np.uint8)
    offs = np.ascontiguousarray(offs, np.int64)
    args = [eng._h, data.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p), arr, len(layouts), ctypes.byref(cfg),
            None if null_features else tab, nfeat]
    if asynchronous:
        st = eng._lib.pp_ingest_pointcloud2_fields_async(*args)
    else:
        st = eng._lib.pp_ingest_pointcloud2_fields(*args, None, 0)
    return st, (eng._lib.pp_last_error(eng._h) or b"").decode()


def test_refusals_name_the_frame_and_the_feature_and_leave_the_engine_usable(pp, hip_lib, cases):
    PP_ERR_ARG = 1
    B = 2
    eng = _engine(pp, B, nmax=4096, weights=True)
    frames = fc.lidar_frames(pp, B, 1200, frame0=40)
    good = cases["constant"][0]                       # point_step 20: x y z float32, rgb at 16
    lay = pp.ingest.layout_of(good)
    data = np.frombuffer(good[0], np.uint8)
    two, both, offs = [dict(lay), dict(lay)], np.concatenate([data, data]), [0, data.size, 2 * data.size]
    ok = (16, 7, 1.0, 0.0)
    assert _raw_fields(eng, both, offs, two, [ok, ok], 1)[0] == 0
    want = eng.detect(frames)
    want = (want[0].copy(), want[1].copy())
    nan, inf = float("nan"), float("inf")
    refusals = [
        # (layouts, features, nfeat, first, decimate, null features, words the message must hold)
        (two, [ok, ok], 1, 1, 4, True, ["features is NULL", "nfeat is 1"]),
        (two, [], 0, 1, 4, False, ["nfeat 0", "num_point_features is 4"]),
        (two, [ok] * 4, 2, 1, 4, False, ["nfeat 2", "num_point_features is 4"]),
        (two, [ok] * 2, -1, 1, 4, False, ["nfeat -1 < 0"]),
        (two, [ok, (16, 9, 1.0, 0.0)], 1, 1, 4, False, ["frame 1", "feature 0", "unknown datatype 9"]),
        (two, [(16, -1, 1.0, 0.0), ok], 1, 1, 4, False, ["frame 0", "feature 0", "unknown datatype -1"]),
        (two, [ok, (-1, 7, 1.0, 0.0)], 1, 1, 4, False, ["frame 1", "feature 0", "offset -1"]),
        (two, [(17, 7, 1.0, 0.0), ok], 1, 1, 4, False, ["frame 0", "feature 0", "offset 17 (4 bytes)", "point_step 20"]),
        (two, [ok, (13, 8, 1.0, 0.0)], 1, 1, 4, False, ["frame 1", "feature 0", "offset 13 (8 bytes)", "point_step 20"]),
        (two, [ok, (20, 2, 1.0, 0.0)], 1, 1, 4, False, ["frame 1", "feature 0", "offset 20 (1 bytes)"]),
        (two, [(16, 7, nan, 0.0), ok], 1, 1, 4, False, ["frame 0", "feature 0", "scale", "not finite"]),
        (two, [ok, (16, 7, inf, 0.0)], 1, 1, 4, False, ["frame 1", "feature 0", "scale", "not finite"]),
        (two, [ok, (16, 7, 1.0, -inf)], 1, 1, 4, False, ["frame 1", "feature 0", "bias", "not finite"]),
        (two, [(0, 0, 1.0, nan), ok], 1, 1, 4, False, ["frame 0", "feature 0", "bias", "not finite"]),
        # what the twin call refuses
        (two, [ok, ok], 1, 1, 0, False, ["decimate 0 < 1"]),
        (two, [ok, ok], 1, -1, 4, False, ["first -1 < 0"]),
        ([dict(lay), dict(lay, z_offset=17)], [ok, ok], 1, 1, 4, False, ["frame 1", "z_offset 17", "point_step 20"]),
        ([dict(lay, row_step=lay["width"] * 20 - 1), dict(lay)], [ok, ok], 1, 1, 4, False, ["frame 0", "row_step"]),
    ]
    for asynchronous in (False, True):
        for layouts, feats, nfeat, first, dec, null, words in refusals:
            st, msg = _raw_fields(eng, both, offs, layouts, feats, nfeat, first, dec, asynchronous, null)
            assert st == PP_ERR_ARG, (feats, nfeat, st, msg)
            for w in words:
                assert w in msg, (w, msg)
            assert ("pp_ingest_pointcloud2_fields_async" in msg) == asynchronous, msg
    # a constant column reads nothing: its offset is not looked at
    assert _raw_fields(eng, both, offs, two, [(999, 0, 1.0, 0.5), ok], 1)[0] == 0
    # nothing of the refused calls was queued: upload the frames again and detect
    _same_detections(eng.detect(frames), want, "detect after the refusals")
    # the calls that deliver x y z only still refuse a 4-feature engine, by name
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*num_point_features is 4"):
        eng.ingest_pointcloud2([good])
    st = eng.staging_pointcloud2([good])
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*pp_ingest_pointcloud2_async.*num_point_features is 4"):
        eng.ingest_pointcloud2_async(st)
    st.close()
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*num_point_features is 4"):
        eng.detect_pointcloud2([good])
    # through the Python layer: a missing field is refused on the host with the message's fields, a bad keyword by name
    with pytest.raises(ValueError, match="no field 'intensity'.*rgb"):
        eng.ingest_pointcloud2([good], features=[pp.ingest.FeatureField("intensity")])
    with pytest.raises(ValueError, match="mount must be an ingest.Mount"):
        eng.ingest_pointcloud2([good], features=cases["constant"][1], mount=np.eye(3))
    with pytest.raises(ValueError, match="lift and mount are both given"):
        eng.ingest_pointcloud2([good], features=cases["constant"][1], mount=fc.identity_mount(pp), lift=1.0)
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*nfeat 2, num_point_features is 4"):
        eng.ingest_pointcloud2([good], features=[pp.ingest.FeatureField("rgb"), pp.ingest.FeatureField.constant(1.0)])
    _same_detections(eng.detect(frames), want, "detect after the Python-level refusals")
    eng.close()
