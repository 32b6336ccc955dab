"""Depth-image ingest on the GPU (csrc/ingest.hip, pp_ingest_depth*): the resident points and the counts against
ingest.depth_ingest_np -- exactly, for every case of depth_cases.py --, detections from depth images against detections
from the equivalent PointCloud2 messages and from host-ingested frames, mixed asynchronous feeds, and every refusal.
No test provokes a fault: every refusal is decided on the host before a launch."""
import ctypes

import numpy as np
import pytest

import depth_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(pp):
    return depth_cases.cases(pp)


@pytest.fixture(scope="module")
def nmax(pp, cases):
    """max_points_per_frame just above the largest case bound."""
    return 1 + max(pp.ingest.depth_kept_bound(img[1], img[2], 0, 1) for img, _, _ in cases.values())


def _engine(pp, cfg, B, nmax, weights=True):
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=nmax)
    if weights:
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    return eng


def _check(pp, eng, names, images, intrinsics, first=1, decimate=4, **kw):
    """One ingest_depth call against the host rule, frame by frame.  kw: per-call depth_scale / z_min / z_max."""
    got = eng.ingest_depth(images, intrinsics, first=first, decimate=decimate, return_points=True, **kw)
    info = eng.ingest_info()
    assert len(got) == len(images)
    for b, (name, img) in enumerate(zip(names, images)):
        k = intrinsics[b] if isinstance(intrinsics, list) else intrinsics
        want, n_valid = pp.ingest.depth_ingest_np(img, k, first, decimate, pp.ingest.SENSOR_HEIGHT, **kw)
        assert int(info["finite"][b]) == n_valid, (name, first, decimate, int(info["finite"][b]), n_valid)
        assert int(info["kept"][b]) == len(want), (name, first, decimate, int(info["kept"][b]), len(want))
        assert got[b].shape == want.shape and got[b].dtype == np.float32, (name, got[b].shape, want.shape)
        same = depth_cases.bits(got[b]) == depth_cases.bits(want)
        assert same.all(), (name, first, decimate, int((~same).sum()), got[b][~same.all(axis=1)][:3], want[~same.all(axis=1)][:3])


@pytest.mark.parametrize("first,decimate", depth_cases.SELECTIONS)
def test_every_case_alone_equals_the_host_rule(pp, hip_lib, cases, nmax, first, decimate):
    eng = _engine(pp, pp.config.tiny_config(1), 1, nmax, weights=False)
    for name, (img, k, kw) in cases.items():
        _check(pp, eng, [name], [img], k, first, decimate, **kw)
    eng.close()


def _call_groups(cases):
    """The cases grouped by their per-call arguments (depth_scale, z_min, z_max belong to a call, not to a frame, in the
    Python layer)."""
    groups = {}
    for name, (img, k, kw) in cases.items():
        groups.setdefault(tuple(sorted(kw.items())), []).append(name)
    return groups


@pytest.mark.parametrize("first,decimate", depth_cases.SELECTIONS)
def test_all_cases_mixed_in_one_batch(pp, hip_lib, cases, nmax, first, decimate):
    """Both encodings, different sizes and intrinsics per frame, in one call; then the other order into the other input
    buffer, where every frame's bytes start somewhere else."""
    groups = _call_groups(cases)
    B = max(len(g) for g in groups.values())
    eng = _engine(pp, pp.config.tiny_config(B), B, nmax, weights=False)
    for key, names in groups.items():
        for order in (names, names[::-1]):
            _check(pp, eng, order, [cases[n][0] for n in order], [cases[n][1] for n in order], first, decimate, **dict(key))
    assert {cases[n][0][4] for n in max(groups.values(), key=len)} >= {"16UC1", "32FC1"}
    eng.close()


def _raw_layouts(pp, cases, names):
    from pp_amd import _lib
    arr = (_lib.PPDepthLayout * len(names))()
    for b, n in enumerate(names):
        img, k, kw = cases[n]
        for key, v in pp.ingest.depth_layout_of(img, k, **kw).items():
            setattr(arr[b], key, v)
    return arr


def test_every_case_in_one_c_abi_call_with_per_frame_scale_and_clip(pp, hip_lib, cases, nmax):
    """The C-ABI carries depth_scale / z_min / z_max per frame: every case, the clipped ones among them, in ONE call."""
    from pp_amd import engine
    names = list(cases)
    B = len(names)
    eng = _engine(pp, pp.config.tiny_config(B), B, nmax, weights=False)
    bufs = [np.frombuffer(cases[n][0][0], np.uint8)[:cases[n][0][2] * cases[n][0][3]] for n in names]
    offs = np.concatenate([[0], np.cumsum([b.size for b in bufs])]).astype(np.int64)
    data = np.concatenate(bufs)
    want = [pp.ingest.depth_ingest_np(cases[n][0], cases[n][1], 1, 4, 1.0, **cases[n][2]) for n in names]
    cap = sum(len(w[0]) for w in want)
    pts = np.empty((cap, 3), np.float32)
    cfg = engine._ingest_config(1, 4, 1.0)
    st = eng._lib.pp_ingest_depth(eng._h, data.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p),
                                  _raw_layouts(pp, cases, names), B, ctypes.byref(cfg), pts.ctypes.data_as(ctypes.c_void_p), cap)
    assert st == 0, eng._lib.pp_last_error(eng._h)
    valid, kept = np.zeros(B, np.int32), np.zeros(B, np.int32)
    assert eng._lib.pp_ingest_info(eng._h, valid.ctypes.data_as(ctypes.c_void_p), kept.ctypes.data_as(ctypes.c_void_p), B) == 0
    assert valid.tolist() == [w[1] for w in want] and kept.tolist() == [len(w[0]) for w in want]
    assert np.array_equal(depth_cases.bits(pts), depth_cases.bits(np.concatenate([w[0] for w in want])))
    eng.close()


def test_a_batch_of_18_one_chunk_frames(pp, hip_lib):
    """The scan gives wave w frames w and w + 16: 18 frames of at most 512 pixels each."""
    B = 18
    rng = np.random.default_rng(3)
    images, intrinsics = [], []
    for b in range(B):
        w, h = (8 + b, 20) if b != 5 else (32, 16)          # 160 .. 500 pixels; one of exactly 512
        d = rng.integers(300, 6500, (h, w)).astype(np.float64)
        d[rng.random((h, w)) < 0.25] = 0
        images.append(pp.synth.depth_from_z(d * 0.001, ("16UC1", "32FC1")[b % 2], step_pad=b % 4, bigendian=b % 3 == 0, seed=b))
        intrinsics.append(depth_cases.intr(w, h, b))
    assert max(i[1] * i[2] for i in images) == 512
    eng = _engine(pp, pp.config.tiny_config(B), B, 513, weights=False)
    for first, decimate in depth_cases.SELECTIONS:
        _check(pp, eng, [f"frame{b}" for b in range(B)], images, intrinsics, first, decimate)
    eng.close()


def _same_detections(a, b, what):
    (da, na), (db, nb) = a, b
    assert np.array_equal(na, nb), (what, na, nb)
    for f in range(len(na)):
        assert np.array_equal(da[f, :na[f]], db[f, :nb[f]]) and da[f, :na[f]].tobytes() == db[f, :nb[f]].tobytes(), (what, f)


def _same_intermediates(ia, ib, what):
    assert np.array_equal(ia["n_pillars"], ib["n_pillars"]), (what, ia["n_pillars"], ib["n_pillars"])
    for f, P in enumerate(ia["n_pillars"]):
        assert np.array_equal(ia["coors"][f, :P], ib["coors"][f, :P]), (what, f)
        assert np.array_equal(ia["num_points"][f, :P], ib["num_points"][f, :P]), (what, f)
    for k in ("anchors_mask", "box_preds", "cls_preds", "dir_cls_preds"):
        if k in ia:
            assert ia[k].tobytes() == ib[k].tobytes(), (what, k)


def _copy(r):
    return r[0].copy(), r[1].copy()


def _scenes(pp, B, width, height, empty=None, seed0=0, **kw):
    """B scene images (alternating encodings, padded rows) with per-frame intrinsics; frame `empty` has a single valid
    pixel, so it keeps no point at first = 1."""
    images, intrinsics = [], []
    for b in range(B):
        img, k = depth_cases.scene(pp, seed0 + b, width - 8 * b, height - 6 * b, encoding=("16UC1", "32FC1")[b % 2],
                                   step_pad=(0, 6, 3)[b % 3], **kw)
        if b == empty:
            z = np.zeros((img[2], img[1]))
            z[img[2] // 2, img[1] // 3] = 2.0
            img = pp.synth.depth_from_z(z, img[4])
        images.append(img)
        intrinsics.append(k)
    return images, intrinsics


def _detect_three_ways(pp, cfg, B, images, intrinsics, nmax, empty):
    ing = pp.ingest
    eng = _engine(pp, cfg, B, nmax)
    rect, trv, _ = pp.synth.default_calib()
    R, T = np.stack([rect] * B), np.stack([trv] * B)
    frames = [ing.depth_ingest_np(img, k)[0] for img, k in zip(images, intrinsics)]
    assert len(frames[empty]) == 0 and all(len(f) for b, f in enumerate(frames) if b != empty)
    from_frames = _copy(eng.detect(frames, R, T))
    i_frames = eng.intermediates()
    msgs = [ing.depth_to_pointcloud2(img, k, ordered=bool(b % 2), point_step=(20, 32)[b % 2])
            for b, (img, k) in enumerate(zip(images, intrinsics))]
    from_msgs = _copy(eng.detect_pointcloud2(msgs, R, T))
    i_msgs = eng.intermediates()
    from_depth = _copy(eng.detect_depth(images, intrinsics, R, T))
    i_depth = eng.intermediates()
    assert eng.ingest_info()["kept"].tolist() == [len(f) for f in frames]
    assert all(i_depth["n_pillars"][b] > 0 for b in range(B) if b != empty) and i_depth["n_pillars"][empty] == 0
    assert from_depth[1][empty] == 0
    _same_detections(from_depth, from_msgs, "depth vs messages")
    _same_detections(from_depth, from_frames, "depth vs host frames")
    _same_intermediates(i_depth, i_msgs, "depth vs messages")
    _same_intermediates(i_depth, i_frames, "depth vs host frames")
    _same_detections(eng.detect_depth(images, intrinsics, R, T), from_depth, "second run")
    eng.close()


def test_detections_from_depth_equal_detections_from_the_message_tiny_config(pp, hip_lib):
    images, intrinsics = _scenes(pp, 3, 96, 64, empty=1, scale=0.2)      # (the tiny grid ends 1.6 m in front of the camera)
    _detect_three_ways(pp, pp.config.tiny_config(3), 3, images, intrinsics, 96 * 64, empty=1)


def test_detections_from_depth_equal_detections_from_the_message_cfg_a(pp, hip_lib):
    images, intrinsics = _scenes(pp, 2, 320, 240, empty=0, seed0=10)
    _detect_three_ways(pp, pp.config.pedestrian_d435i_config(2), 2, images, intrinsics, 32768, empty=0)


def test_mixed_feeds_without_a_sync_in_between(pp, hip_lib):
    """upload -> detect_async -> ingest_depth_async (other frames) -> detect_async, and ingest_depth_async ->
    ingest_pointcloud2_async -> ingest_depth_async with a detect_async behind each, every feed queued while the pass
    before it is in flight: byte-identical to the synchronous feeds."""
    B = 2
    eng = _engine(pp, pp.config.pedestrian_d435i_config(B), B, 32768)
    frames_a = [pp.synth.d435i_cloud(300 + b, 16384) for b in range(B)]
    images_b, k_b = _scenes(pp, B, 320, 240, seed0=20)
    msgs_c = [pp.synth.pointcloud2_message(90 + b, 320, 240, point_step=(32, 20)[b]) for b in range(B)]
    images_d, k_d = _scenes(pp, B, 200, 150, seed0=30)

    def snap():
        d, n = eng.detections()
        return (d.copy(), n.copy()), eng.intermediates()

    want = []
    for feed in (lambda: eng.upload(frames_a), lambda: eng.ingest_depth(images_b, k_b),
                 lambda: eng.ingest_pointcloud2(msgs_c), lambda: eng.ingest_depth(images_d, k_d)):
        feed()
        eng.detect_async()
        eng.sync()
        want.append(snap())
    assert all(int(w[1]["n_pillars"].min()) > 0 for w in want)

    st_b, st_c, st_d = eng.staging_depth(images_b), eng.staging_pointcloud2(msgs_c), eng.staging_depth(images_d)
    for rnd in range(2):
        eng.upload(frames_a)
        eng.detect_async()
        eng.ingest_depth_async(st_b, k_b)
        got = [snap()]
        eng.detect_async()
        eng.ingest_pointcloud2_async(st_c)
        got.append(snap())
        eng.detect_async()
        eng.ingest_depth_async(st_d, k_d)
        got.append(snap())
        eng.detect_async()
        got.append(snap())
        for k, g in enumerate(got):
            _same_detections(g[0], want[k][0], (rnd, "abcd"[k]))
            _same_intermediates(g[1], want[k][1], (rnd, "abcd"[k]))
        assert eng.ingest_info()["kept"].tolist() == [len(pp.ingest.depth_ingest_np(i, k)[0]) for i, k in zip(images_d, k_d)]
    eng.sync()
    for s in (st_b, st_c, st_d):
        s.close()
    eng.close()


def _raw(eng, data, offs, layouts, first=1, decimate=4, asynchronous=False):
    """The C-ABI call itself, with a layout the Python layer would not let through."""
    from pp_amd import _lib, engine
    arr = (_lib.PPDepthLayout * len(layouts))()
    for b, lay in enumerate(layouts):
        for k, v in lay.items():
            setattr(arr[b], k, v)
    cfg = engine._ingest_config(first, decimate, 1.0)
    data = np.ascontiguousarray(data, np.uint8)
    offs = np.ascontiguousarray(offs, np.int64)
    pd, po = data.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p)
    if asynchronous:
        st = eng._lib.pp_ingest_depth_async(eng._h, pd, po, arr, len(layouts), ctypes.byref(cfg))
    else:
        st = eng._lib.pp_ingest_depth(eng._h, pd, po, arr, len(layouts), ctypes.byref(cfg), None, 0)
    return st, (eng._lib.pp_last_error(eng._h) or b"").decode()


def test_refusals_name_the_field_and_leave_the_engine_usable(pp, hip_lib):
    PP_ERR_ARG = 1
    B = 2
    eng = _engine(pp, pp.config.pedestrian_d435i_config(B), B, 8192)
    frames = [pp.synth.d435i_cloud(400 + b, 4096) for b in range(B)]
    good, k = depth_cases.scene(pp, 1, 64, 48, step_pad=6)
    lay = pp.ingest.depth_layout_of(good, k)
    data = np.frombuffer(good[0], np.uint8)
    two = [dict(lay), dict(lay)]
    both = np.concatenate([data, data])
    offs = [0, data.size, 2 * data.size]
    assert _raw(eng, both, offs, two)[0] == 0
    want = _copy(eng.detect(frames))

    def bad(frame, **kw):
        ls = [dict(lay), dict(lay)]
        ls[frame].update(kw)
        return ls

    nan, inf = float("nan"), float("inf")
    refusals = [
        # (layouts, offsets, first, decimate, words the message must hold)
        (bad(1, width=640, height=480, row_step=1280), [0, data.size, data.size + 480 * 1280], 1, 4,
         ["frame 1", "76800", "max_points_per_frame=8192"]),
        (bad(1, row_step=127), offs, 1, 4, ["frame 1", "row_step 127 < width 64 x 2 bytes"]),
        (bad(0, encoding=1, row_step=255), offs, 1, 4, ["frame 0", "row_step 255 < width 64 x 4 bytes"]),
        (bad(0, encoding=2), offs, 1, 4, ["frame 0", "unknown encoding 2"]),
        (bad(1, encoding=-1), offs, 1, 4, ["frame 1", "unknown encoding -1"]),
        (bad(1, width=-1), offs, 1, 4, ["frame 1", "width -1"]),
        (two, [0, data.size, 2 * data.size - 1], 1, 4, ["frame 1", "byte_offsets", "row_step"]),
        (two, [0, data.size - 6, 2 * data.size], 1, 4, ["frame 0", "byte_offsets"]),
        (bad(0, fx=0.0), offs, 1, 4, ["frame 0", "fx 0 "]),
        (bad(1, fx=nan), offs, 1, 4, ["frame 1", "fx nan"]),
        (bad(1, fy=0.0), offs, 1, 4, ["frame 1", "fy 0 "]),
        (bad(0, fy=inf), offs, 1, 4, ["frame 0", "fy inf"]),
        (bad(0, ppx=nan), offs, 1, 4, ["frame 0", "ppx nan"]),
        (bad(1, ppy=-inf), offs, 1, 4, ["frame 1", "ppy -inf"]),
        (bad(1, depth_scale=0.0), offs, 1, 4, ["frame 1", "depth_scale 0 "]),
        (bad(0, depth_scale=-0.001), offs, 1, 4, ["frame 0", "depth_scale -0.001"]),
        (bad(0, depth_scale=inf), offs, 1, 4, ["frame 0", "depth_scale inf"]),
        (bad(1, z_min=2.0, z_max=1.0), offs, 1, 4, ["frame 1", "z_min 2 > z_max 1"]),
        (bad(0, z_max=nan), offs, 1, 4, ["frame 0", "z_min", "z_max nan"]),
        (two, offs, 1, 0, ["decimate 0 < 1"]),
        (two, offs, -1, 4, ["first -1 < 0"]),
    ]
    for asynchronous in (False, True):
        for layouts, o, first, dec, words in refusals:
            st, msg = _raw(eng, both, o, layouts, first, dec, asynchronous)
            assert st == PP_ERR_ARG, (layouts, o, first, dec, st, msg)
            for w in words:
                assert w in msg, (w, msg)
            assert ("pp_ingest_depth_async" in msg) == asynchronous and "pp_ingest_depth" in msg, msg
    # too many frames
    st, msg = _raw(eng, np.concatenate([data] * 3), [0, data.size, 2 * data.size, 3 * data.size], [dict(lay)] * 3)
    assert st == PP_ERR_ARG and "max_batch=2" in msg, msg
    # nothing was queued and nothing changed: the frames uploaded before are still the resident ones
    eng.detect_async()
    _same_detections(eng.detections(), want, "resident frames after the refusals")
    # through the Python layer: the library's text reaches the caller (no host fallback) ...
    vga, kv = depth_cases.scene(pp, 2, 640, 480)
    with pytest.raises(RuntimeError, match=r"PP_ERR_ARG.*frame 0.*76800.*max_points_per_frame=8192"):
        eng.ingest_depth([vga], kv)
    with pytest.raises(RuntimeError, match=r"PP_ERR_ARG.*frame 1.*76800.*max_points_per_frame=8192"):
        eng.detect_depth([good, vga], [k, kv])
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*decimate 0 < 1"):
        eng.ingest_depth([good], k, decimate=0)
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*first -2 < 0"):
        eng.ingest_depth([good], k, first=-2)
    # ... and the host layer's own refusals name their field as well
    with pytest.raises(ValueError, match="non-zero distortion"):
        eng.ingest_depth([good], ([k[0], 0, k[2], 0, k[1], k[3], 0, 0, 1], [0.1, 0, 0, 0, 0]))
    with pytest.raises(ValueError, match="not a depth encoding"):
        eng.ingest_depth([good[:4] + ("rgb8", False)], k)
    with pytest.raises(ValueError, match="2 sets of intrinsics for 1 images"):
        eng.ingest_depth([good], [k, k])
    # the tap's capacity: below the kept total is refused, the frames stay resident
    from pp_amd import _lib, engine
    arr = (_lib.PPDepthLayout * 1)()
    for key, v in lay.items():
        setattr(arr[0], key, v)
    pts = np.empty((10, 3), np.float32)
    cfg = engine._ingest_config(1, 4, 1.0)
    o1 = np.array([0, data.size], np.int64)
    st = eng._lib.pp_ingest_depth(eng._h, data.ctypes.data_as(ctypes.c_void_p), o1.ctypes.data_as(ctypes.c_void_p), arr, 1,
                                  ctypes.byref(cfg), pts.ctypes.data_as(ctypes.c_void_p), 10)
    msg = eng._lib.pp_last_error(eng._h).decode()
    n_kept = len(pp.ingest.depth_ingest_np(good, k)[0])
    assert n_kept > 10 and st == PP_ERR_ARG and "pp_ingest_depth: points_out holds 10 points" in msg and str(n_kept) in msg, msg
    kept = np.zeros((1,), np.int32)
    assert eng._lib.pp_ingest_info(eng._h, None, kept.ctypes.data_as(ctypes.c_void_p), 1) == 0 and kept.tolist() == [n_kept]
    # the engine still detects correctly, and a good call returns the right bytes
    _same_detections(eng.detect(frames), want, "detect after the refusals")
    _check(pp, eng, ["good", "good"], [good, good], k)
    eng.close()


def test_point_features_other_than_xyz_are_unsupported(pp, hip_lib):
    eng = _engine(pp, pp.config.kitti_shaped_config(1), 1, 32768, weights=False)
    img, k = depth_cases.scene(pp, 1, 64, 48)
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*pp_ingest_depth: num_point_features is 4"):
        eng.ingest_depth([img], k)
    st = eng.staging_depth([img])
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*pp_ingest_depth_async: num_point_features is 4"):
        eng.ingest_depth_async(st, k)
    st.close()
    eng.close()


def test_depth_ingest_while_a_training_step_is_in_flight_is_a_state_error(pp, hip_lib):
    B = 2
    cfg = pp.config.pedestrian_d435i_config(B)
    d = pp.config.Derived(cfg)
    tr = pp.Trainer(cfg, pp.weights.init_weights(d, seed=7), max_batch=B, max_points_per_frame=8192, learning_rate=2e-4,
                    weight_decay=1e-4)
    eng = tr.engine
    frames = [pp.synth.d435i_cloud(500 + b, 4096) for b in range(B)]
    gts = [np.array([[3.0, 0.2 * b, 0.0, 0.6, 0.8, 1.73, 0.1]], np.float32) for b in range(B)]
    images, k = _scenes(pp, B, 64, 48, seed0=40)
    eng.upload(frames)
    eng.train_step_gt_async(tr.params.data_ptr(), tr.grads.data_ptr(), tr.state.data_ptr(), *eng.pack_gt(gts))
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_ingest_depth: a training step is in flight"):
        eng.ingest_depth(images, k)
    st = eng.staging_depth(images)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_ingest_depth_async: a training step is in flight"):
        eng.ingest_depth_async(st, k)
    losses = eng.train_step_wait()
    assert np.isfinite(losses["loss"])
    _check(pp, eng, ["d0", "d1"], images, k)      # after the step the same handle ingests
    st.close()
    tr.close()


def test_augment_after_a_depth_ingest_is_refused_as_after_a_message_ingest(pp, hip_lib):
    eng = _engine(pp, pp.config.pedestrian_d435i_config(1), 1, 8192, weights=False)
    img, k = depth_cases.scene(pp, 1, 64, 48)
    eng.ingest_depth([img], k)
    gt = [np.array([[3.0, 0.0, 0.0, 0.6, 0.8, 1.73, 0.1]], np.float32)]
    draws = pp.augment.draw(np.random.RandomState(1), gt, pp.augment.AugmentConfig.from_input_reader(None))
    with pytest.raises(RuntimeError, match="device only.*upload frames first"):
        eng.augment(gt, draws=draws)
    eng.close()


def _same_dicts(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.keys() == w.keys() and g["batch_idx"] == w["batch_idx"]
        for key in w:
            assert (g[key] is None) == (w[key] is None), key
            if w[key] is not None:
                assert np.array_equal(g[key], w[key]), key


def test_voxelnet_detect_depth_returns_detect_pointcloud2s_dicts(pp, hip_lib):
    cfg = pp.config.pedestrian_d435i_config(2)
    net = pp.VoxelNet(cfg, max_batch=2, max_points_per_frame=32768)
    net.load_weights(pp.weights.init_weights(net.d, seed=7))
    images, k = _scenes(pp, 2, 320, 240, seed0=50)
    msgs = [pp.ingest.depth_to_pointcloud2(i, kk, point_step=20, ordered=True) for i, kk in zip(images, k)]
    rect, trv, _ = pp.synth.default_calib()
    R, T = np.stack([rect] * 2), np.stack([trv] * 2)
    want = net.detect_pointcloud2(msgs, R, T, image_idx=[7, 8])
    got = net.detect_depth(images, k, R, T, image_idx=[7, 8])
    _same_dicts(got, want)
    net.engine.close()


def test_voxelnet_detect_depth_in_training_mode(pp, hip_lib):
    cfg = pp.config.tiny_config(2)
    net = pp.VoxelNet(cfg, training=True, max_batch=2, max_points_per_frame=96 * 64)
    net.load_weights(pp.weights.init_weights(net.d, seed=7))
    images, k = _scenes(pp, 2, 96, 64, seed0=60, scale=0.2)
    msgs = [pp.ingest.depth_to_pointcloud2(i, kk) for i, kk in zip(images, k)]
    rect, trv, _ = pp.synth.default_calib()
    R, T = np.stack([rect] * 2), np.stack([trv] * 2)
    want = net.detect_pointcloud2(msgs, R, T)
    got = net.detect_depth(images, k, R, T)
    _same_dicts(got, want)
    net.trainer.close()
