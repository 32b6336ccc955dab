"""The frustum crop on the GPU (csrc/frustum_crop.hip): pp_frustum_crop* against tests/golden/ref_frustum.npz -- counts and
bytes of what the reference's remove_outside_points kept, order included --, over the zero-copy and the copy feed, the
on-the-face rule, PP_CROP_BACK, run-to-run identity, the detection pass and the object-database build on the cropped
frames, the asynchronous crop, Engine.detect's crop, the streamed reduced-cloud files, and every refusal."""
import numpy as np
import pytest

from test_frustum_host import FACE_PLANES, check_objects, face_cloud, fixture_frames, labelled_dataset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return fixture_frames()[1]


def _engine(pp, cfg, max_batch):
    eng = pp.Engine(cfg, max_batch=max_batch, max_points_per_frame=4096)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    return eng


@pytest.fixture(scope="module")
def eng_a(pp, hip_lib):
    """cfg-A: three point features."""
    eng = _engine(pp, pp.config.pedestrian_d435i_config(8), 8)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def eng_k(pp, hip_lib):
    """cfg-K: four point features."""
    eng = _engine(pp, pp.config.kitti_shaped_config(8), 8)
    assert eng.d.num_point_features == 4
    yield eng
    eng.close()


def _feed(eng, clouds, how):
    """upload: pp_upload_points; staged: pp_upload_points_async (zero-copy up to 4 frames, the copy stream above)."""
    if how == "upload":
        eng.upload(clouds)
        return None
    st = eng.staging(clouds)
    eng.upload_async(st)
    return st


def _crop(eng, fx, names, how="staged", back=False):
    """Feeds the named fixture frames, crops them with the RECORDED planes; returns (kept counts, per-frame arrays)."""
    st = _feed(eng, [fx[n]["points"] for n in names], how)
    kept, pts = eng.crop_to_image(np.stack([fx[n]["planes"] for n in names]), back=back, return_points=True)
    if st is not None:
        st.close()
    return kept, pts


def _check(fx, names, kept, pts, ref_names=None):
    for n, r, k, p in zip(names, ref_names or names, kept, pts):
        ref = fx[r]["kept"]
        assert k == len(ref), (n, int(k), len(ref))
        assert p.dtype == np.float32 and p.shape == ref.shape and p.tobytes() == ref.tobytes(), n


BATCHES_K = [["a9"], ["a8", "a2", "a5"], ["odd", "neg", "cone", "g1"],                      # 1, 3, 4 frames: the zero-copy feed
             ["a0", "a1", "a2", "a3", "a4", "a5", "a6", "a9"], ["a9", "a7", "a0", "a8", "a1", "a6", "a3", "a5"]]   # the copy feed


@pytest.mark.parametrize("names", BATCHES_K, ids=lambda n: f"B{len(n)}-{n[0]}")
def test_fixture_frames_equal_reference_four_features(eng_k, fx, names):
    kept, pts = _crop(eng_k, fx, names)
    assert kept.dtype == np.int32
    _check(fx, names, kept, pts)
    assert np.array_equal(eng_k.crop_info(), kept)


@pytest.mark.parametrize("names", [["b1"], ["b0", "b1", "b2"], ["b2", "b0", "b1", "b1", "b0", "b2", "b1", "b0"]],
                         ids=lambda n: f"B{len(n)}")
def test_fixture_frames_equal_reference_three_features(eng_a, fx, names):
    kept, pts = _crop(eng_a, fx, names)
    _check(fx, names, kept, pts)


def test_nan_is_kept_and_inf_follows_ieee(eng_k, fx):
    kept, pts = _crop(eng_k, fx, ["odd"])
    _check(fx, ["odd"], kept, pts)
    assert np.isnan(pts[0][:, 0]).sum() == 1 and not np.isinf(pts[0]).any()     # as the reference: recorded, not assumed


@pytest.mark.parametrize("which", ["a", "k"])
def test_point_on_a_face_is_removed(eng_a, eng_k, which):
    eng = eng_a if which == "a" else eng_k
    p = face_cloud(eng.d.num_point_features)
    for how in ("upload", "staged"):
        st = _feed(eng, [p, p[::-1].copy()], how)
        kept, pts = eng.crop_to_image(np.stack([FACE_PLANES] * 2), return_points=True)
        assert kept.tolist() == [1, 1]
        assert pts[0].tobytes() == p[1:2].tobytes() and pts[1].tobytes() == p[1:2].tobytes()
        if st is not None:
            st.close()


def test_crop_back(pp, eng_k, fx):
    for how in ("upload", "staged"):
        kept, pts = _crop(eng_k, fx, ["a8", "a9"], how, back=True)
        _check(fx, ["a8"], kept[:1], pts[:1], ref_names=["back"])
        want = pp.frustum.crop_np(fx["a9"]["points"], fx["a9"]["planes"], back=True)
        assert pts[1].tobytes() == want.tobytes()


def test_same_bytes_on_every_run_and_over_every_feed(eng_k, fx):
    names = ["a9", "a5", "a8", "a4", "g0", "a1"]
    first = _crop(eng_k, fx, names, "upload")
    again = _crop(eng_k, fx, names, "upload")
    staged = _crop(eng_k, fx, names, "staged")
    for got in (again, staged):
        assert np.array_equal(got[0], first[0])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[1], first[1]))
    # a crop of the cropped frames keeps all of them
    kept2, pts2 = eng_k.crop_to_image(np.stack([fx[n]["planes"] for n in names]), return_points=True)
    assert np.array_equal(kept2, first[0]) and all(a.tobytes() == b.tobytes() for a, b in zip(pts2, first[1]))
    # zero-copy feed against the synchronous upload, three frames
    small = _crop(eng_k, fx, names[:3], "staged")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(small[1], first[1][:3]))


def _pass_products(eng):
    im = eng.intermediates()
    return im["n_pillars"].copy(), im["coors"].copy(), im["num_points"].copy()


def _assert_same_pass(got, want, got_dets, want_dets):
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert np.array_equal(got_dets[1], want_dets[1]) and got_dets[0].tobytes() == want_dets[0].tobytes()


def test_detection_pass_sees_the_cropped_frames(pp, eng_k, fx):
    names = ["a9", "g0", "g2"]
    B = len(names)
    rect, trv = np.stack([fx[n]["rect"] for n in names]), np.stack([fx[n]["Trv2c"] for n in names])
    want_dets = eng_k.detect([fx[n]["kept"] for n in names], rect, trv)          # an upload of the host-cropped frames
    want_dets = (want_dets[0].copy(), want_dets[1].copy())
    want = _pass_products(eng_k)
    assert (want[0][:B] > 0).all()
    raw_dets = eng_k.detect([fx[n]["points"] for n in names], rect, trv)
    assert not np.array_equal(_pass_products(eng_k)[0][:B], want[0][:B])           # the raw frames voxelise differently
    del raw_dets
    planes = np.stack([fx[n]["planes"] for n in names])
    # synchronous crop, then the pass
    eng_k.upload([fx[n]["points"] for n in names], rect, trv)
    eng_k.crop_to_image(planes)
    got_dets = eng_k._detect_resident("f32")
    _assert_same_pass(_pass_products(eng_k), want, got_dets, want_dets)
    # asynchronous crop behind an asynchronous upload: the same detections; the sizes stay on the device
    st = eng_k.staging([fx[n]["points"] for n in names])
    eng_k.upload_async(st)
    eng_k.set_calib(rect, trv, B)
    eng_k.crop_to_image_async(planes)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*upload frames first"):
        eng_k.count_points_in_gt([np.zeros((0, 7))] * B)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*upload frames first"):
        eng_k.crop_to_image(planes)                                               # crops do not chain behind device sizes
    got_dets = eng_k._detect_resident("f32")
    _assert_same_pass(_pass_products(eng_k), want, got_dets, want_dets)
    assert eng_k.crop_info().tolist() == [len(fx[n]["kept"]) for n in names]
    st.close()
    # Engine.detect with p2 and image_shape: upload + crop + pass
    p2, shp = np.stack([fx[n]["P2"] for n in names]), np.stack([fx[n]["image_shape"] for n in names])
    got_dets = eng_k.detect([fx[n]["points"] for n in names], rect, trv, p2=p2, image_shape=shp)
    _assert_same_pass(_pass_products(eng_k), want, got_dets, want_dets)
    with pytest.raises(ValueError, match="p2 and image_shape"):
        eng_k.detect([fx[n]["points"] for n in names], rect, trv, p2=p2)
    with pytest.raises(ValueError, match="p2 and image_shape"):
        eng_k.detect([fx[n]["points"] for n in names], rect, trv, image_shape=shp)


def test_database_build_on_the_cropped_frames(pp, eng_k, fx):
    gdb = pp.gt_database
    names = ["g0", "g1", "g2"]
    lidar = [fx[n]["rbbox_lidar"] for n in names]
    for how in ("upload", "staged"):
        st = _feed(eng_k, [fx[n]["points"] for n in names], how)
        eng_k.crop_to_image(np.stack([fx[n]["planes"] for n in names]))
        counts = eng_k.count_points_in_gt(lidar)
        objs = eng_k.build_gt_objects(lidar)
        for n, c, o, bx in zip(names, counts, objs, lidar):
            f = fx[n]
            assert np.array_equal(c, f["num_points_in_gt"][:len(bx)])
            for i, g in enumerate(o):
                ref = f["obj_points"][f["obj_offsets"][i]:f["obj_offsets"][i + 1]]
                assert g.shape == ref.shape and g.tobytes() == ref.tobytes(), (n, i)
        if st is not None:
            st.close()
    infos, clouds = labelled_dataset(fx)
    gdb.calculate_num_points_in_gt(eng_k, infos, clouds, remove_outside=True)
    for k, info in enumerate(infos):
        assert np.array_equal(info["annos"]["num_points_in_gt"], fx[f"g{k}"]["num_points_in_gt"])
    db_infos, db_points = gdb.create_groundtruth_database(eng_k, infos, clouds, used_classes=["Pedestrian", "Cyclist"],
                                                          remove_outside=True)
    assert check_objects(fx, db_infos, db_points) == 8
    gdb.calculate_num_points_in_gt(eng_k, infos, clouds)                           # the default: no crop
    for k, info in enumerate(infos):
        assert np.array_equal(info["annos"]["num_points_in_gt"], fx[f"g{k}"]["num_points_in_gt_raw"])
    ex = pp.prep_example(eng_k, fx["g0"]["points"], fx["g0"]["rect"], fx["g0"]["Trv2c"], fx["g0"]["P2"],
                         image_shape=fx["g0"]["image_shape"], remove_outside=True)
    want = eng_k.points_to_voxel(fx["g0"]["kept"])
    assert ex["voxels"].tobytes() == want[0].tobytes() and np.array_equal(ex["coordinates"], want[1])


def test_reduced_point_cloud_streams_partial_batches(pp, hip_lib, fx, tmp_path):
    gdb = pp.gt_database
    eng = pp.Engine(pp.config.pedestrian_d435i_config(4), max_batch=4, max_points_per_frame=4096)
    rng = np.random.default_rng(5)
    infos, clouds = [], []
    for k in range(11):
        f = fx[f"b{k % 3}"]
        infos.append({"velodyne_path": f"training/velodyne/{k:06d}.bin", "img_shape": f["image_shape"], "calib/R0_rect": f["rect"],
                      "calib/Tr_velo_to_cam": f["Trv2c"], "calib/P2": f["P2"]})
        n = [0, 1, 300, 257, 4096, 64, 1000, 63, 2000, 513, 777][k]
        clouds.append(np.stack([rng.uniform(-10, 70, n), rng.uniform(-30, 30, n), rng.uniform(-3, 2, n)], 1).astype(np.float32))
    for back in (False, True):
        want = gdb.create_reduced_point_cloud(None, infos, clouds, tmp_path / "host", back=back)
        got = gdb.create_reduced_point_cloud(eng, infos, clouds, tmp_path / "gpu", back=back)
        assert got.dtype == np.int32 and np.array_equal(got, want) and 0 < got.sum() < sum(len(c) for c in clouds)
        for k in range(11):
            name = f"{k:06d}.bin" + ("_back" if back else "")
            assert (tmp_path / "gpu" / name).read_bytes() == (tmp_path / "host" / name).read_bytes(), name
    eng.close()


def test_refusals_leave_the_handle_usable(pp, hip_lib, eng_k, fx):
    fresh = pp.Engine(pp.config.kitti_shaped_config(2), max_batch=2, max_points_per_frame=4096)
    planes = np.stack([fx["a8"]["planes"], fx["a5"]["planes"]])
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no frames are resident"):
        fresh.crop_to_image(planes)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no frames are resident"):
        fresh.crop_to_image_async(planes)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no crop has run"):
        fresh.crop_info()
    fresh.close()
    eng = eng_k
    eng.upload([fx["a8"]["points"], fx["a5"]["points"]])
    bad = planes.copy()
    bad[1, 3, 2] = np.nan
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*frame 1.*not finite"):
        eng.crop_to_image(bad)
    bad[1, 3, 2] = np.inf
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*frame 1.*not finite"):
        eng.crop_to_image_async(bad)
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*2 frames are resident, batch is 1"):
        eng.crop_to_image(planes[:1])
    with pytest.raises(ValueError, match=r"\[batch, 6, 4\]"):
        eng.crop_to_image(planes[0])
    kept = np.zeros(2, np.int32)
    ptr = planes.ctypes.data
    assert eng._lib.pp_frustum_crop(eng._h, ptr, 2, 6, kept.ctypes.data, None, 0) == 1          # unknown flag bits
    assert b"flag" in eng._lib.pp_last_error(eng._h)
    assert eng._lib.pp_frustum_crop_async(eng._h, ptr, 2, 2) == 1
    assert eng._lib.pp_frustum_crop(eng._h, None, 2, 0, kept.ctypes.data, None, 0) == 1         # planes NULL
    # points_out too small: PP_ERR_ARG, and the frames stay resident and cropped
    out = np.zeros((4, 4), np.float32)
    assert eng._lib.pp_frustum_crop(eng._h, ptr, 2, 0, kept.ctypes.data, out.ctypes.data, 4) == 1
    assert kept.tolist() == [len(fx["a8"]["kept"]), len(fx["a5"]["kept"])]
    eng._offsets = np.concatenate([[0], np.cumsum(kept)]).astype(np.int32)
    counts = eng.count_points_in_gt([np.array([[30.0, 0, -4, 200, 200, 8, 0]])] * 2)            # a box around everything
    assert counts[0][0] == kept[0] and counts[1][0] == kept[1]
    # sizes known on the device only (after an ingest-like state): refused, then an upload makes it work again
    eng.upload([fx["a8"]["points"], fx["a5"]["points"]])
    eng.crop_to_image_async(planes)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*upload frames first"):
        eng.crop_to_image_async(planes)
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*the last crop had 2 frames"):
        eng._check(eng._lib.pp_frustum_crop_info(eng._h, kept.ctypes.data, 1), "pp_frustum_crop_info")
    # after every refusal the handle works
    got_kept, got = _crop(eng, fx, ["a8", "a5"], "upload")
    _check(fx, ["a8", "a5"], got_kept, got)


def test_crop_while_a_training_step_is_in_flight_is_a_state_error(pp, hip_lib, fx):
    # (nearly all of this test's time is the Trainer's first step -- its plan and graph capture -- at the smallest batch)
    B = 1
    cfg = pp.config.pedestrian_d435i_config(B)
    d = pp.config.Derived(cfg)
    tr = pp.Trainer(cfg, pp.weights.init_weights(d, seed=7), max_batch=B, max_points_per_frame=4096, learning_rate=2e-4,
                    weight_decay=1e-4)
    eng = tr.engine
    frames = [pp.synth.d435i_cloud(500 + b, 2048) for b in range(B)]
    gts = [np.array([[3.0, 0.2 * b, 0.0, 0.6, 0.8, 1.73, 0.1]], np.float32) for b in range(B)]
    planes = np.stack([FACE_PLANES] * B)
    eng.upload(frames)
    eng.train_step_gt_async(tr.params.data_ptr(), tr.grads.data_ptr(), tr.state.data_ptr(), *eng.pack_gt(gts))
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*training step is in flight"):
        eng.crop_to_image(planes)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*training step is in flight"):
        eng.crop_to_image_async(planes)
    losses = eng.train_step_wait()
    assert np.isfinite(losses["loss"])
    # after the step the same handle crops
    eng.upload(frames)
    kept, pts = eng.crop_to_image(planes, return_points=True)
    for b in range(B):
        want = pp.frustum.crop_np(frames[b], FACE_PLANES)
        assert kept[b] == len(want) and pts[b].tobytes() == want.tobytes()
    tr.close()
