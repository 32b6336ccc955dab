"""Live PointCloud2 ingest on the GPU (csrc/ingest.hip, pp_ingest_pointcloud2*): the resident points and the counts
against the package's host path realsense_to_lidar(pointcloud2_to_xyz(...)) -- exactly, for every layout --, detections
from raw messages against Engine.detect on host-ingested frames, mixed asynchronous feeds, and every refusal."""
import ctypes

import numpy as np
import pytest

import pc2_cases

pytestmark = pytest.mark.gpu

VGA_BOUND = 76800       # ingest.kept_bound(640, 480, 1, 4)


def _engine(pp, cfg, B, nmax=32768, weights=True):
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=nmax)
    if weights:
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    return eng


def _check_ingest(pp, eng, names, msgs, first=1, decimate=4):
    got = eng.ingest_pointcloud2(msgs, first=first, decimate=decimate, return_points=True)
    info = eng.ingest_info()
    assert len(got) == len(msgs)
    for b, (name, msg) in enumerate(zip(names, msgs)):
        with np.errstate(over="ignore"):
            want, n_finite = pc2_cases.host_ingest(pp, msg, first, decimate)
        assert int(info["finite"][b]) == n_finite, (name, first, decimate, int(info["finite"][b]), n_finite)
        assert int(info["kept"][b]) == len(want), (name, first, decimate, int(info["kept"][b]), len(want))
        assert got[b].shape == want.shape and got[b].dtype == np.float32, (name, got[b].shape, want.shape)
        same = pc2_cases.bits(got[b]) == pc2_cases.bits(want)
        assert same.all(), (name, first, decimate, int((~same).sum()), got[b][~same.all(axis=1)][:3], want[~same.all(axis=1)][:3])


@pytest.mark.parametrize("first,decimate", pc2_cases.SELECTIONS)
def test_every_layout_alone_equals_the_host_path(pp, hip_lib, first, decimate):
    eng = _engine(pp, pp.config.pedestrian_d435i_config(1), 1, 8192, weights=False)
    for name, msg in pc2_cases.layout_cases(pp).items():
        _check_ingest(pp, eng, [name], [msg], first, decimate)
    eng.close()


@pytest.mark.parametrize("first,decimate", pc2_cases.SELECTIONS)
def test_all_layouts_mixed_in_one_batch(pp, hip_lib, first, decimate):
    cases = pc2_cases.layout_cases(pp)
    names = list(cases)
    eng = _engine(pp, pp.config.pedestrian_d435i_config(len(names)), len(names), 8192, weights=False)
    _check_ingest(pp, eng, names, [cases[n] for n in names], first, decimate)
    # the other order, into the other input buffer: every frame's bytes now start somewhere else
    _check_ingest(pp, eng, names[::-1], [cases[n] for n in names[::-1]], first, decimate)
    eng.close()


def test_vga_messages_at_max_batch(pp, hip_lib):
    B = 4
    eng = _engine(pp, pp.config.pedestrian_d435i_config(B), B, VGA_BOUND, weights=False)
    msgs = [pp.synth.pointcloud2_message(20 + b, point_step=(20, 32)[b % 2], row_pad=(0, 16)[b // 2]) for b in range(B)]
    _check_ingest(pp, eng, [f"vga{b}" for b in range(B)], msgs)
    _check_ingest(pp, eng, ["vga_alone"], msgs[2:3])
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


def _host_frames(pp, msgs):
    return [pc2_cases.host_ingest(pp, m)[0] for m in msgs]


def _detect_both_ways(pp, cfg, B, msgs, nmax=32768):
    eng = _engine(pp, cfg, B, nmax)
    rect, trv, _ = pp.synth.default_calib()
    R, T = np.stack([rect] * B), np.stack([trv] * B)
    want = eng.detect(_host_frames(pp, msgs), R, T)
    want = (want[0].copy(), want[1].copy())
    iw = eng.intermediates()
    got = eng.detect_pointcloud2(msgs, R, T)
    got = (got[0].copy(), got[1].copy())
    ig = eng.intermediates()
    assert int(iw["n_pillars"].min()) > 0
    _same_detections(got, want, "messages vs host-ingested frames")
    _same_intermediates(ig, iw, "messages vs host-ingested frames")
    again = eng.detect_pointcloud2(msgs, R, T)
    _same_detections(again, got, "second run")
    _same_intermediates(eng.intermediates(), ig, "second run")
    eng.close()
    return got


@pytest.mark.parametrize("B", [1, 4, 16])
def test_detect_from_messages_equals_detect_on_host_frames_cfg_a(pp, hip_lib, B):
    msgs = [pp.synth.pointcloud2_message(40 + b, 320, 240, point_step=(20, 32)[b % 2], row_pad=4 * (b % 3)) for b in range(B)]
    _detect_both_ways(pp, pp.config.pedestrian_d435i_config(B), B, msgs)


def test_detect_from_a_vga_message_cfg_a(pp, hip_lib):
    msg = pp.synth.pointcloud2_message(60, point_step=20)
    _detect_both_ways(pp, pp.config.pedestrian_d435i_config(1), 1, [msg], VGA_BOUND)


def test_detect_from_messages_tiny_config(pp, hip_lib):
    B = 2
    msgs = [pp.synth.pointcloud2_message(70 + b, 96, 64, point_step=32, datatype=(7, 8)[b], offsets=((0, 4, 8), (0, 8, 16))[b])
            for b in range(B)]
    _detect_both_ways(pp, pp.config.tiny_config(B), B, msgs, 4096)


def test_detect_with_frames_that_keep_no_point(pp, hip_lib):
    """An all-NaN message and one with a single finite record (rank 0 < first: nothing kept) inside a batch, and alone:
    the voxeliser, the anchor mask and the post-process see 0-point frames through the device-written offsets, and give
    what Engine.detect gives for an empty frame."""
    cases = pc2_cases.layout_cases(pp)
    msgs = [pp.synth.pointcloud2_message(50, 320, 240), cases["all_nan"], cases["finite_1"],
            pp.synth.pointcloud2_message(51, 200, 150, point_step=32)]
    rect, trv, _ = pp.synth.default_calib()
    for sel in ([0, 1, 2, 3], [1], [1, 2]):
        B = len(sel)
        eng = _engine(pp, pp.config.pedestrian_d435i_config(B), B)
        R, T = np.stack([rect] * B), np.stack([trv] * B)
        frames = _host_frames(pp, [msgs[i] for i in sel])
        assert all(len(frames[k]) == 0 for k, i in enumerate(sel) if i in (1, 2))
        want = eng.detect(frames, R, T)
        want = (want[0].copy(), want[1].copy())
        iw = eng.intermediates()
        got = eng.detect_pointcloud2([msgs[i] for i in sel], R, T)
        ig = eng.intermediates()
        assert eng.ingest_info()["kept"].tolist() == [len(f) for f in frames]
        for k, i in enumerate(sel):
            if i in (1, 2):
                assert ig["n_pillars"][k] == 0 and got[1][k] == 0 and not ig["anchors_mask"][k].any()
        _same_detections(got, want, sel)
        _same_intermediates(ig, iw, sel)
        eng.close()


def test_augment_after_an_ingest_is_refused_clearly(pp, hip_lib):
    eng = _engine(pp, pp.config.pedestrian_d435i_config(1), 1, 8192, weights=False)
    eng.ingest_pointcloud2([pp.synth.pointcloud2_message(1, 64, 48)])
    gt = [np.array([[3.0, 0.0, 0.0, 0.6, 0.8, 1.73, 0.1]], np.float32)]
    draws = pp.augment.draw(np.random.RandomState(1), gt, pp.augment.AugmentConfig.from_input_reader(None))
    with pytest.raises(RuntimeError, match="device only.*upload frames first"):
        eng.augment(gt, draws=draws)
    eng.close()


def test_voxelnet_detect_pointcloud2_returns_detects_dicts(pp, hip_lib):
    cfg = pp.config.pedestrian_d435i_config(2)
    net = pp.VoxelNet(cfg, max_batch=2, max_points_per_frame=32768)
    net.load_weights(pp.weights.init_weights(net.d, seed=7))
    msgs = [pp.synth.pointcloud2_message(80 + b, 320, 240) for b in range(2)]
    rect, trv, _ = pp.synth.default_calib()
    R, T = np.stack([rect] * 2), np.stack([trv] * 2)
    want = net.detect(_host_frames(pp, msgs), R, T, image_idx=[7, 8])
    got = net.detect_pointcloud2(msgs, R, T, image_idx=[7, 8])
    for g, w in zip(got, want):
        assert g.keys() == w.keys() and g["batch_idx"] == w["batch_idx"]
        for k in w:
            assert (g[k] is None) == (w[k] is None), k
            if w[k] is not None:
                assert np.array_equal(g[k], w[k]), k
    net.engine.close()


def test_mixed_feeds_without_a_sync_in_between(pp, hip_lib):
    """upload -> detect_async -> ingest_pointcloud2_async (other frames) -> detect_async -> upload_async -> detect_async,
    each feed queued while the pass before it is still in flight: the main-stream voxeliser of the synchronous feed and
    the copy-stream voxeliser behind the ingest share their scratch."""
    B = 2
    eng = _engine(pp, pp.config.pedestrian_d435i_config(B), B)
    frames_a = [pp.synth.d435i_cloud(300 + b, 16384) for b in range(B)]
    msgs_b = [pp.synth.pointcloud2_message(90 + b, 320, 240, point_step=(32, 20)[b]) for b in range(B)]
    frames_c = [pp.synth.d435i_cloud(310 + b, 12000) for b in range(B)]

    def snap():
        d, n = eng.detections()
        im = eng.intermediates()
        return (d.copy(), n.copy()), im

    want = []
    for feed in (lambda: eng.upload(frames_a), lambda: eng.ingest_pointcloud2(msgs_b), lambda: eng.upload(frames_c)):
        feed()
        eng.detect_async()
        eng.sync()
        want.append(snap())
    # the synchronous ingest itself is held to the host path
    eng.detect(_host_frames(pp, msgs_b))
    _same_detections(snap()[0], want[1][0], "sync ingest vs host frames")

    st_b = eng.staging_pointcloud2(msgs_b)
    st_c = eng.staging(frames_c)
    for rnd in range(3):
        eng.upload(frames_a)
        eng.detect_async()
        eng.ingest_pointcloud2_async(st_b)
        got_a = snap()
        eng.detect_async()
        eng.upload_async(st_c)
        got_b = snap()
        eng.detect_async()
        got_c = snap()
        for k, got in enumerate((got_a, got_b, got_c)):
            _same_detections(got[0], want[k][0], (rnd, "abc"[k]))
            _same_intermediates(got[1], want[k][1], (rnd, "abc"[k]))
        info = eng.ingest_info()
        assert info["kept"].tolist() == [len(f) for f in _host_frames(pp, msgs_b)]
    # and two asynchronous ingests back to back
    st_b2 = eng.staging_pointcloud2(msgs_b[::-1])
    eng.ingest_pointcloud2_async(st_b)
    eng.detect_async()
    eng.ingest_pointcloud2_async(st_b2)
    got_b = snap()
    eng.detect_async()
    got_b2 = snap()
    _same_detections(got_b[0], want[1][0], "async ingest 1")
    assert np.array_equal(got_b2[0][1], want[1][0][1][::-1])
    assert np.array_equal(got_b2[1]["n_pillars"], want[1][1]["n_pillars"][::-1])
    eng.sync()
    for s in (st_b, st_b2, st_c):
        s.close()
    eng.close()


def _raw_ingest(eng, data, offs, layouts, first=1, decimate=4, asynchronous=False):
    """The C-ABI call itself, with a layout the Python layer would not let through."""
    from pp_amd import _lib, engine
    arr = (_lib.PPPc2Layout * len(layouts))()
    for b, lay in enumerate(layouts):
        for k, v in lay.items():
            setattr(arr[b], k, v)
    cfg = engine._ingest_config(first, decimate, 1.0)
    data = np.ascontiguousarray(data, np.uint8)
    offs = np.ascontiguousarray(offs, np.int64)
    if asynchronous:
        st = eng._lib.pp_ingest_pointcloud2_async(eng._h, data.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p),
                                                  arr, len(layouts), ctypes.byref(cfg))
    else:
        st = eng._lib.pp_ingest_pointcloud2(eng._h, data.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p),
                                            arr, len(layouts), ctypes.byref(cfg), None, 0)
    return st, (eng._lib.pp_last_error(eng._h) or b"").decode()


def test_refusals_name_the_field_and_leave_the_engine_usable(pp, hip_lib):
    PP_ERR_ARG, PP_ERR_UNSUPPORTED = 1, 5
    B = 2
    eng = _engine(pp, pp.config.pedestrian_d435i_config(B), B, 8192)
    frames = [pp.synth.d435i_cloud(400 + b, 4096) for b in range(B)]
    good = pp.synth.pointcloud2_message(1, 64, 48, point_step=20, row_pad=12)
    lay = pp.ingest.layout_of(good)
    data = np.frombuffer(good[0], np.uint8)
    two = [dict(lay), dict(lay)]
    both = np.concatenate([data, data])
    offs = [0, data.size, 2 * data.size]
    assert _raw_ingest(eng, both, offs, two)[0] == 0
    want = eng.detect(frames)
    want = (want[0].copy(), want[1].copy())

    def bad(frame, **kw):
        ls = [dict(lay), dict(lay)]
        ls[frame].update(kw)
        return ls

    refusals = [
        # (layouts, offsets, first, decimate, status, words the message must hold)
        (bad(1, width=640, height=480, row_step=640 * 20), [0, data.size, data.size + 480 * 640 * 20], 1, 4, PP_ERR_ARG,
         ["frame 1", "76800", "max_points_per_frame=8192"]),
        (bad(1, row_step=64 * 20 - 1), offs, 1, 4, PP_ERR_ARG, ["frame 1", "row_step 1279 < width 64 x point_step 20"]),
        (bad(0, z_offset=17), offs, 1, 4, PP_ERR_ARG, ["frame 0", "z_offset 17", "point_step 20"]),
        (bad(1, y_offset=-1), offs, 1, 4, PP_ERR_ARG, ["frame 1", "y_offset -1"]),
        (bad(0, datatype=8, x_offset=13), offs, 1, 4, PP_ERR_ARG, ["frame 0", "x_offset 13", "8 bytes"]),
        (two, [0, data.size, 2 * data.size - 1], 1, 4, PP_ERR_ARG, ["frame 1", "byte_offsets", "row_step"]),
        (two, [0, data.size - 12, 2 * data.size], 1, 4, PP_ERR_ARG, ["frame 0", "byte_offsets"]),
        (two, offs, 1, 0, PP_ERR_ARG, ["decimate 0 < 1"]),
        (two, offs, -1, 4, PP_ERR_ARG, ["first -1 < 0"]),
        (bad(1, datatype=5), offs, 1, 4, PP_ERR_UNSUPPORTED, ["frame 1", "datatype 5", "integer"]),
        (bad(0, datatype=2), offs, 1, 4, PP_ERR_UNSUPPORTED, ["frame 0", "datatype 2", "integer"]),
        (bad(1, datatype=7 | 7 << 8 | 8 << 16), offs, 1, 4, PP_ERR_UNSUPPORTED, ["frame 1", "datatype", "differ", "(7, 7, 8)"]),
        (bad(0, datatype=9), offs, 1, 4, PP_ERR_ARG, ["frame 0", "datatype 9"]),
    ]
    for asynchronous in (False, True):
        for layouts, o, first, dec, status, words in refusals:
            st, msg = _raw_ingest(eng, both, o, layouts, first, dec, asynchronous)
            assert st == status, (layouts, o, first, dec, st, msg)
            for w in words:
                assert w in msg, (w, msg)
            assert ("pp_ingest_pointcloud2_async" in msg) == asynchronous, msg
    # too many frames
    st, msg = _raw_ingest(eng, np.concatenate([data] * 3), [0, data.size, 2 * data.size, 3 * data.size], [dict(lay)] * 3)
    assert st == PP_ERR_ARG and "max_batch=2" in msg, msg
    # nothing was queued and nothing changed: the frames uploaded before are still the resident ones
    eng.detect_async()
    _same_detections(eng.detections(), want, "resident frames after the refusals")
    # through the Python layer: the library's text reaches the caller (no host fallback)
    with pytest.raises(RuntimeError, match=r"PP_ERR_ARG.*frame 0.*76800.*max_points_per_frame=8192"):
        eng.ingest_pointcloud2([pp.synth.pointcloud2_message(2)])
    ints = (bytes(4 * 12), 4, 1, 12, 48, [("x", 0, 5, 1), ("y", 4, 5, 1), ("z", 8, 5, 1)], False)
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*integer"):
        eng.detect_pointcloud2([ints])
    mixed = (bytes(4 * 16), 4, 1, 16, 64, [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 8, 1)], False)
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*differ"):
        eng.ingest_pointcloud2([mixed])
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*decimate 0 < 1"):
        eng.ingest_pointcloud2([good], decimate=0)
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*first -2 < 0"):
        eng.ingest_pointcloud2([good], first=-2)
    # the tap's capacity: below the kept total is refused, the frames stay resident
    pts = np.empty((10, 3), np.float32)
    arr = (pp._lib.PPPc2Layout * 1)()
    for k, v in lay.items():
        setattr(arr[0], k, v)
    from pp_amd import engine
    cfg = engine._ingest_config(1, 4, 1.0)
    o1 = np.array([0, data.size], np.int64)
    st = eng._lib.pp_ingest_pointcloud2(eng._h, data.ctypes.data_as(ctypes.c_void_p), o1.ctypes.data_as(ctypes.c_void_p), arr, 1,
                                        ctypes.byref(cfg), pts.ctypes.data_as(ctypes.c_void_p), 10)
    msg = eng._lib.pp_last_error(eng._h).decode()
    n_kept = len(pc2_cases.host_ingest(pp, good)[0])
    assert st == PP_ERR_ARG and "points_out holds 10 points" in msg and str(n_kept) in msg, msg
    kept = np.zeros((1,), np.int32)         # (the raw call went past the Engine: so does the tap)
    assert eng._lib.pp_ingest_info(eng._h, None, kept.ctypes.data_as(ctypes.c_void_p), 1) == 0 and kept.tolist() == [n_kept]
    # ... and the engine still detects correctly
    _same_detections(eng.detect(frames), want, "detect after the refusals")
    with np.errstate(over="ignore"):
        _check_ingest(pp, eng, ["good"], [good])
    eng.close()


def test_point_features_other_than_xyz_are_unsupported(pp, hip_lib):
    eng = _engine(pp, pp.config.kitti_shaped_config(1), 1, 32768, weights=False)
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*num_point_features is 4"):
        eng.ingest_pointcloud2([pp.synth.pointcloud2_message(1, 64, 48)])
    eng.close()


def test_ingest_info_before_any_ingest_is_a_state_error(pp, hip_lib):
    eng = _engine(pp, pp.config.pedestrian_d435i_config(1), 1, 8192, weights=False)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no ingest has run"):
        eng._ing_batch = 1
        eng.ingest_info()
    eng.close()


def test_ingest_while_a_training_step_is_in_flight_is_a_state_error(pp, hip_lib):
    B = 2
    cfg = pp.config.pedestrian_d435i_config(B)
    d = pp.config.Derived(cfg)
    tr = pp.Trainer(cfg, pp.weights.init_weights(d, seed=7), max_batch=B, max_points_per_frame=8192, learning_rate=2e-4,
                    weight_decay=1e-4)
    eng = tr.engine
    frames = [pp.synth.d435i_cloud(500 + b, 4096) for b in range(B)]
    gts = [np.array([[3.0, 0.2 * b, 0.0, 0.6, 0.8, 1.73, 0.1]], np.float32) for b in range(B)]
    msgs = [pp.synth.pointcloud2_message(3 + b, 64, 48) for b in range(B)]
    eng.upload(frames)
    eng.train_step_gt_async(tr.params.data_ptr(), tr.grads.data_ptr(), tr.state.data_ptr(), *eng.pack_gt(gts))
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*training step is in flight"):
        eng.ingest_pointcloud2(msgs)
    st = eng.staging_pointcloud2(msgs)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*training step is in flight"):
        eng.ingest_pointcloud2_async(st)
    losses = eng.train_step_wait()
    assert np.isfinite(losses["loss"])
    # after the step the same handle ingests
    _check_ingest(pp, eng, ["m0", "m1"], msgs)
    st.close()
    tr.close()
