"""Camera-rig ingest on the GPU (csrc/ingest.hip, pp_ingest_rig_*): several sources per frame, each under its own
mount and selection, against ingest.rig_depth_ingest_np / rig_ingest_np -- exactly: every comparison is on the float32
bytes, no tolerance, no excluded rows.  One source per frame against the single-camera calls, chunk and scan boundaries,
more sources than the scan has waves, PointCloud2 rigs, detections (synchronous, asynchronous, mixed with the other feeds)
and every refusal.  No test provokes a fault: every refusal is decided on the host before a launch."""
import ctypes

import numpy as np
import pytest

import depth_cases

pytestmark = pytest.mark.gpu

B_MAX = 3
NMAX = 36000          # a 260 x 128 source at (0, 1) keeps up to 33280 points, the sources beside it a few hundred


@pytest.fixture(scope="module")
def eng(pp, hip_lib):
    e = pp.Engine(pp.config.tiny_config(B_MAX), max_batch=B_MAX, max_points_per_frame=NMAX)
    e.load_weights(pp.weights.init_weights(e.d, seed=7))
    yield e
    e.close()


def _same_points(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    same = depth_cases.bits(got) == depth_cases.bits(want)
    assert same.all(), (what, int((~same).sum()), got[~same.all(axis=1)][:3], want[~same.all(axis=1)][:3])


def _check_depth(pp, eng, frames, rig, what):
    """One ingest_rig_depth call against the host rule: the frames' points, the frames' sums, the sources' counts."""
    got = eng.ingest_rig_depth(frames, rig, return_points=True)
    info, per = eng.ingest_info(), eng.ingest_rig_info()
    assert len(got) == len(frames) and per["kept"].shape == (len(frames), len(rig))
    wants = []
    for b, fr in enumerate(frames):
        want, valid, kept = pp.ingest.rig_depth_ingest_np(fr, rig)
        assert per["finite"][b].tolist() == valid.tolist(), (what, b, per["finite"][b], valid)
        assert per["kept"][b].tolist() == kept.tolist(), (what, b, per["kept"][b], kept)
        assert int(info["finite"][b]) == int(valid.sum()) and int(info["kept"][b]) == len(want), (what, b)
        _same_points(got[b], want, (what, b))
        wants.append(want)
    return wants


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
        if k in ia:
            assert ia[k].tobytes() == ib[k].tobytes(), (what, k)


def _copy(r):
    return r[0].copy(), r[1].copy()


def _calib(B):
    import pp_amd
    rect, trv, _ = pp_amd.synth.default_calib()
    return np.stack([rect] * B), np.stack([trv] * B)


def _image(pp, rng, w, h, enc="16UC1", pad=0, big=False, invalid=0.3, lo=0.25, hi=1.5, seed=0):
    """A w x h image of depths lo .. hi m (the tiny grid ends 1.6 m in front of a camera), `invalid` of them holes; a
    32FC1 image carries NaN, inf and negative holes as well."""
    z = rng.uniform(lo, hi, (h, w))
    hole = rng.random((h, w)) < invalid
    z[hole] = 0.0
    if enc == "32FC1" and hole.any():
        z[hole] = rng.choice([0.0, np.nan, np.inf, -1.0], int(hole.sum()))
    return pp.synth.depth_from_z(z, enc, step_pad=pad, bigendian=big, seed=seed)


def _exact(pp, rng, w, h, n_valid, **kw):
    """A w x h 16UC1 image with exactly n_valid valid pixels."""
    z = np.zeros(w * h)
    z[rng.choice(w * h, n_valid, replace=False)] = rng.uniform(0.25, 1.5, n_valid)
    return pp.synth.depth_from_z(z.reshape(h, w), **kw)


# camera axes (x right, y down, z depth) -> lidar axes (x depth, y left, z up), as a column-vector matrix
_AXES = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


def _extrinsic(yaw_deg, t):
    a = np.deg2rad(yaw_deg)
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ _AXES
    T[:3, 3] = t
    return T


def _three_mounts(pp):
    """The reference mount, a general extrinsic (yaw 40 degrees and a translation), the reference matrices under a lift
    with three non-zero entries."""
    ing = pp.ingest
    r, r2 = ing._matrices()
    return [ing.Mount.realsense(), ing.Mount.from_matrix(_extrinsic(40.0, [0.05, -0.2, 0.9])), ing.Mount(r, r2, [0.1, 0.15, 0.7])]


SIZES3 = [(8, 6), (31, 17), (70, 5)]


@pytest.fixture(scope="module")
def three_cameras(pp):
    """Case 2: B = 2 frames of three cameras (8 x 6, 31 x 17, 70 x 5), every size in both encodings, odd steps and
    big-endian images among them; three distinct mounts, intrinsics and selections."""
    rng = np.random.default_rng(31)
    spec = [[("16UC1", 1, True), ("32FC1", 3, False), ("16UC1", 0, False)],
            [("32FC1", 0, True), ("16UC1", 5, True), ("32FC1", 1, True)]]
    frames = [[_image(pp, rng, w, h, enc, pad, big, seed=10 * b + c) for c, ((w, h), (enc, pad, big)) in enumerate(zip(SIZES3, fr))]
              for b, fr in enumerate(spec)]
    assert all(f[c][3] % 2 == 1 for f, c in ((frames[0], 0), (frames[0], 1), (frames[1], 1), (frames[1], 2)))      # odd steps
    rig = pp.ingest.CameraRig(_three_mounts(pp), [depth_cases.intr(w, h, c) for c, (w, h) in enumerate(SIZES3)],
                              first=[1, 0, 2], decimate=[4, 1, 3])
    return frames, rig


def test_one_source_per_frame_equals_the_single_camera_calls(pp, eng):
    """Case 1: B = 3, one camera under the reference mount: the bytes, the counts and the detections of ingest_depth /
    detect_depth, and of ingest_pointcloud2 / detect_pointcloud2 for the cameras' messages."""
    ing = pp.ingest
    pairs = [depth_cases.scene(pp, 70 + b, 96, 64, encoding=("16UC1", "32FC1")[b % 2], step_pad=(0, 3, 6)[b], scale=0.2)
             for b in range(3)]
    images, k = [p[0] for p in pairs], pairs[0][1]
    assert all(p[1] == k for p in pairs)
    rig = ing.CameraRig([ing.Mount.realsense()], k)
    R, T = _calib(3)
    want_pts = eng.ingest_depth(images, k, return_points=True)
    want_info = {n: v.copy() for n, v in eng.ingest_info().items()}
    want_det = _copy(eng.detect_depth(images, k, R, T))
    want_im = eng.intermediates()
    assert int(want_im["n_pillars"].min()) > 0
    got_pts = eng.ingest_rig_depth([[i] for i in images], rig, return_points=True)
    info, per = eng.ingest_info(), eng.ingest_rig_info()
    for b in range(3):
        _same_points(got_pts[b], want_pts[b], ("depth", b))
    for n in ("finite", "kept"):
        assert info[n].tolist() == want_info[n].tolist() == per[n].reshape(-1).tolist(), n
    _same_detections(eng.detect_rig_depth([[i] for i in images], rig, R, T), want_det, "rig depth vs detect_depth")
    _same_intermediates(eng.intermediates(), want_im, "rig depth vs detect_depth")

    msgs = [ing.depth_to_pointcloud2(img, k, ordered=bool(b % 2), point_step=(16, 20, 32)[b]) for b, img in enumerate(images)]
    want_pts = eng.ingest_pointcloud2(msgs, return_points=True)
    want_info = {n: v.copy() for n, v in eng.ingest_info().items()}
    want_det2 = _copy(eng.detect_pointcloud2(msgs, R, T))
    _same_detections(want_det2, want_det, "messages vs depth")
    got_pts = eng.ingest_rig_pointcloud2([[m] for m in msgs], rig, return_points=True)
    info, per = eng.ingest_info(), eng.ingest_rig_info()
    for b in range(3):
        _same_points(got_pts[b], want_pts[b], ("pc2", b))
    for n in ("finite", "kept"):
        assert info[n].tolist() == want_info[n].tolist() == per[n].reshape(-1).tolist(), n
    _same_detections(eng.detect_rig_pointcloud2([[m] for m in msgs], rig, R, T), want_det, "rig pc2 vs detect_depth")
    _same_intermediates(eng.intermediates(), want_im, "rig pc2 vs detect_depth")


def test_three_cameras_per_frame_equal_the_host_concatenation(pp, eng, three_cameras):
    """Case 2."""
    frames, rig = three_cameras
    wants = _check_depth(pp, eng, frames, rig, "three cameras")
    kept = eng.ingest_rig_info()["kept"]
    assert (kept > 0).all() and all(len(w) == kept[b].sum() for b, w in enumerate(wants))
    # the other order of the frames lands in the other input buffer, every source's bytes somewhere else
    _check_depth(pp, eng, frames[::-1], rig, "three cameras, frames swapped")


def test_chunk_and_scan_boundaries(pp, eng):
    """Case 3: sources of 511, 512 and 513 pixels in one frame; a source of 260 x 128 pixels (65 chunks: the wave scan
    carries once); a source with no valid pixel between two that have some; a source whose valid count is <= first; a
    frame that keeps nothing at all."""
    ing = pp.ingest
    rng = np.random.default_rng(41)
    mounts = _three_mounts(pp)

    def rig_of(sizes, first, decimate, n=3):
        return ing.CameraRig(mounts[:n], [depth_cases.intr(w, h, c) for c, (w, h) in enumerate(sizes)], first=first, decimate=decimate)

    # 511, 512, 513 pixels: all valid, then with holes, at every selection
    sizes = [(511, 1), (64, 8), (27, 19)]
    assert [w * h for w, h in sizes] == [511, 512, 513]
    for first, decimate in depth_cases.SELECTIONS:
        for invalid in (0.0, 0.3):
            fr = [_image(pp, rng, w, h, ("16UC1", "32FC1")[c % 2], pad=c, invalid=invalid, seed=c) for c, (w, h) in enumerate(sizes)]
            _check_depth(pp, eng, [fr], rig_of(sizes, first, decimate), ("511/512/513", first, decimate, invalid))
    # exactly 511 / 512 / 513 valid pixels in 64 x 9 (the 513th in the second chunk), selections mixed per source
    fr = [_exact(pp, rng, 64, 9, n, seed=n) for n in (511, 512, 513)]
    _check_depth(pp, eng, [fr], rig_of([(64, 9)] * 3, [1, 0, 3], [4, 1, 5]), "valid 511/512/513")

    # 65 chunks beside an empty source; then a source with <= first valid pixels between two that keep some
    big = _image(pp, rng, 260, 128, "16UC1", pad=1, seed=5)
    none = pp.synth.depth_from_z(np.zeros((9, 40)), "32FC1", step_pad=2)
    small = [_image(pp, rng, 33, 20, ("16UC1", "32FC1")[c % 2], seed=20 + c) for c in range(3)]
    two_valid = _exact(pp, rng, 33, 20, 2, seed=7)
    rig = rig_of([(260, 128), (40, 9), (33, 20)], [0, 1, 2], [1, 4, 3])
    assert ing.rig_kept_bound([(260, 128), (40, 9), (33, 20)], rig) <= NMAX
    wants = _check_depth(pp, eng, [[big, none, small[0]], [small[1], small[2], two_valid]], rig, "65 chunks / empty / <= first")
    per = eng.ingest_rig_info()
    assert per["finite"][0, 0] > 64 * 512 * 0.6 and per["kept"][0].tolist()[1] == 0 and per["kept"][0, 2] > 0
    assert per["finite"][1, 2] == 2 and per["kept"][1, 2] == 0 and per["kept"][1, 0] > 0 and per["kept"][1, 1] > 0
    # the big source behind others (its rows start at a non-zero out_base) and in the second frame
    rig = rig_of([(33, 20), (260, 128), (40, 9)], [2, 1, 0], [3, 4, 1])
    _check_depth(pp, eng, [[small[0], _image(pp, rng, 260, 128, "32FC1", seed=6), none], [small[1], big, none]], rig, "65 chunks second")

    # a frame that keeps nothing at all, between two that keep some; then a call that keeps nothing at all
    rig = rig_of([(33, 20), (40, 9)], [2, 1], [3, 4], n=2)
    one_valid = pp.synth.depth_from_z(np.where(np.arange(360).reshape(9, 40) == 77, 1.0, 0.0), "32FC1")
    frames = [[small[0], one_valid], [two_valid, one_valid], [two_valid, _image(pp, rng, 40, 9, "32FC1", seed=9)]]
    wants = _check_depth(pp, eng, frames, rig, "empty frame")
    assert [len(w) > 0 for w in wants] == [True, False, True]
    dets, n = eng.detect_rig_depth(frames, rig, *_calib(3))
    assert eng.intermediates()["n_pillars"][1] == 0 and n[1] == 0
    wants = _check_depth(pp, eng, [[two_valid, one_valid]] * 2, rig, "nothing kept")
    assert all(len(w) == 0 for w in wants)
    z0 = pp.synth.depth_from_z(np.zeros((0, 0)))
    _check_depth(pp, eng, [[z0, z0]], rig_of([(0, 0), (0, 0)], [1, 0], [4, 1], n=2), "no pixels")


def test_more_sources_than_the_scan_has_waves(pp, eng):
    """Case 4: B = 3 with 6 sources each: wave w of the scan takes sources w and w + 16; selections mixed per camera."""
    ing = pp.ingest
    rng = np.random.default_rng(51)
    sel = [(1, 4), (0, 1), (2, 3), (0, 1), (2, 3), (1, 4)]
    sizes = [(16 + 5 * c, 11 + c) for c in range(6)]
    mounts = (_three_mounts(pp) * 2)[::-1]
    mounts[0] = ing.Mount.from_matrix(_extrinsic(-25.0, [0.0, 0.1, 0.5]))
    rig = ing.CameraRig(mounts, [depth_cases.intr(w, h, c) for c, (w, h) in enumerate(sizes)],
                        first=[s[0] for s in sel], decimate=[s[1] for s in sel], depth_scale=[0.001, 0.00025] * 3,
                        z_max=[np.inf, np.inf, 1.2] * 2)
    frames = [[pp.synth.depth_from_z(np.where(rng.random((h, w)) < 0.25, 0.0, rng.uniform(0.25, 1.5, (h, w))),
                                      ("16UC1", "32FC1")[(b + c) % 2], step_pad=(b + c) % 4, bigendian=(b + 2 * c) % 3 == 0,
                                      depth_scale=rig.depth_scale[c], seed=100 * b + c) for c, (w, h) in enumerate(sizes)]
              for b in range(3)]
    wants = _check_depth(pp, eng, frames, rig, "18 sources")
    assert eng.ingest_rig_info()["kept"].size == 18 and all(len(w) > 0 for w in wants)


def test_pointcloud2_rig(pp, eng):
    """Case 5: two messages per frame: unordered and ordered, point_step 16 / 20 / 32, a FLOAT64 message."""
    ing, s = pp.ingest, pp.synth
    rng = np.random.default_rng(61)
    img_a, img_b = _image(pp, rng, 45, 23, seed=1), _image(pp, rng, 52, 21, "32FC1", pad=3, seed=2)
    ka, kb = depth_cases.intr(45, 23, 1), depth_cases.intr(52, 21, 2)
    frames = [[ing.depth_to_pointcloud2(img_a, ka, ordered=False, point_step=16), ing.depth_to_pointcloud2(img_b, kb, ordered=True, point_step=20)],
              [s.pointcloud2_message(7, 37, 29, point_step=32, row_pad=3, offsets=(4, 12, 20)),
               s.pointcloud2_message(8, 61, 18, point_step=32, datatype=8, bigendian=True, offsets=(1, 9, 17))]]
    mounts = _three_mounts(pp)
    for first, decimate, m in (([1, 2], [4, 3], mounts[:2]), ([0, 1], [1, 4], mounts[1:])):
        rig = ing.CameraRig(m, first=first, decimate=decimate)
        got = eng.ingest_rig_pointcloud2(frames, rig, return_points=True)
        info, per = eng.ingest_info(), eng.ingest_rig_info()
        for b, fr in enumerate(frames):
            want, fin, kept = ing.rig_ingest_np(fr, rig)
            assert per["finite"][b].tolist() == fin.tolist() and per["kept"][b].tolist() == kept.tolist(), (b, per, fin, kept)
            assert int(info["finite"][b]) == fin.sum() and int(info["kept"][b]) == len(want) and (kept > 0).all()
            _same_points(got[b], want, ("pc2 rig", b, first))


def test_detections_from_a_rig_equal_detections_from_the_host_concatenation(pp, eng, three_cameras):
    """Case 6, first three parts: detect_rig_depth against Engine.detect on the host-concatenated frames, twice, and the
    asynchronous feed from a staging."""
    frames, rig = three_cameras
    R, T = _calib(2)
    host = [pp.ingest.rig_depth_ingest_np(fr, rig)[0] for fr in frames]
    want = _copy(eng.detect(host, R, T))
    want_im = eng.intermediates()
    assert int(want_im["n_pillars"].min()) > 0
    got = _copy(eng.detect_rig_depth(frames, rig, R, T))
    _same_detections(got, want, "rig vs host frames")
    _same_intermediates(eng.intermediates(), want_im, "rig vs host frames")
    _same_detections(eng.detect_rig_depth(frames, rig, R, T), got, "second run")
    st = eng.staging_rig_depth(frames, rig)
    for rnd in range(2):
        eng.ingest_rig_depth_async(st, rig)
        eng.detect_async()
        _same_detections(eng.detections(), want, ("asynchronous", rnd))
        _same_intermediates(eng.intermediates(), want_im, ("asynchronous", rnd))
        assert eng.ingest_rig_info()["kept"].sum(axis=1).tolist() == [len(h) for h in host]
    eng.sync()
    st.close()
    # the same cameras as messages, through the message staging
    msgs = [[pp.ingest.depth_to_pointcloud2(img, rig.intrinsics[c], ordered=bool(c % 2), point_step=(16, 20, 32)[c])
             for c, img in enumerate(fr)] for fr in frames]
    _same_detections(eng.detect_rig_pointcloud2(msgs, rig, R, T), want, "rig messages vs host frames")
    st = eng.staging_rig_pointcloud2(msgs, rig)
    eng.ingest_rig_pointcloud2_async(st, rig)
    eng.detect_async()
    _same_detections(eng.detections(), want, "asynchronous messages")
    eng.sync()
    st.close()


def test_rig_feeds_mixed_with_the_other_feeds_without_a_sync_in_between(pp, eng, three_cameras):
    """Case 6, last part: upload_async -> detect_async -> ingest_rig_depth_async -> detect_async -> ingest_depth_async ->
    detect_async -> ingest_rig_depth_async (another rig) -> detect_async, every feed queued while the pass before it is in
    flight: byte-identical to the synchronous feeds."""
    ing = pp.ingest
    B = 2
    frames_b, rig_b = three_cameras
    rng = np.random.default_rng(71)
    frames_a = [np.ascontiguousarray(pp.synth.d435i_cloud(300 + b, 4096) * np.float32(0.25)) for b in range(B)]
    pairs = [depth_cases.scene(pp, 80 + b, 96, 64, encoding=("32FC1", "16UC1")[b], step_pad=3 * b, scale=0.2) for b in range(B)]
    images_c, k_c = [p[0] for p in pairs], [p[1] for p in pairs]
    sizes_d = [(50, 30), (41, 37)]
    rig_d = ing.CameraRig(_three_mounts(pp)[1:], [depth_cases.intr(w, h, 3 + c) for c, (w, h) in enumerate(sizes_d)],
                          first=[0, 1], decimate=[1, 2])
    frames_d = [[_image(pp, rng, w, h, ("16UC1", "32FC1")[(b + c) % 2], pad=c, seed=40 + 2 * b + c) for c, (w, h) in enumerate(sizes_d)]
                for b in range(B)]

    def snap():
        d, n = eng.detections()
        return (d.copy(), n.copy()), eng.intermediates()

    want = []
    for feed in (lambda: eng.upload(frames_a), lambda: eng.ingest_rig_depth(frames_b, rig_b),
                 lambda: eng.ingest_depth(images_c, k_c), lambda: eng.ingest_rig_depth(frames_d, rig_d)):
        feed()
        eng.detect_async()
        eng.sync()
        want.append(snap())
    assert all(int(w[1]["n_pillars"].min()) > 0 for w in want)

    st_a, st_b, st_c, st_d = (eng.staging(frames_a), eng.staging_rig_depth(frames_b, rig_b), eng.staging_depth(images_c),
                              eng.staging_rig_depth(frames_d, rig_d))
    for rnd in range(2):
        eng.upload_async(st_a)
        eng.detect_async()
        eng.ingest_rig_depth_async(st_b, rig_b)
        got = [snap()]
        eng.detect_async()
        eng.ingest_depth_async(st_c, k_c)
        got.append(snap())
        eng.detect_async()
        eng.ingest_rig_depth_async(st_d, rig_d)
        got.append(snap())
        eng.detect_async()
        got.append(snap())
        for k, g in enumerate(got):
            _same_detections(g[0], want[k][0], (rnd, "abcd"[k]))
            _same_intermediates(g[1], want[k][1], (rnd, "abcd"[k]))
        assert eng.ingest_rig_info()["kept"].tolist() == [ing.rig_depth_ingest_np(fr, rig_d)[2].tolist() for fr in frames_d]
    eng.sync()
    for s in (st_a, st_b, st_c, st_d):
        s.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _raw(eng, kind, data, offs, layouts, sel, fmap, batch, asynchronous=False):
    """The C-ABI call itself (kind "depth" or "pointcloud2"), with arguments the Python layer would not let through.
    layouts: one dict per source; sel: one (first, decimate) per source, under the reference mount."""
    from pp_amd import _lib, engine
    S = len(layouts)
    arr = ((_lib.PPDepthLayout if kind == "depth" else _lib.PPPc2Layout) * S)()
    for s, lay in enumerate(layouts):
        for k, v in lay.items():
            setattr(arr[s], k, v)
    cfgs = (_lib.PPIngestConfig * S)()
    for s, (first, decimate) in enumerate(sel):
        cfgs[s] = engine._ingest_config(first, decimate, 1.0)
    data = np.ascontiguousarray(data, np.uint8)
    offs = np.ascontiguousarray(offs, np.int64)
    fm = np.ascontiguousarray(fmap, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    name = f"pp_ingest_rig_{kind}" + ("_async" if asynchronous else "")
    if asynchronous:
        st = getattr(eng._lib, name)(eng._h, p(data), p(offs), arr, cfgs, p(fm), S, batch)
    else:
        st = getattr(eng._lib, name)(eng._h, p(data), p(offs), arr, cfgs, p(fm), S, batch, None, 0)
    return st, (eng._lib.pp_last_error(eng._h) or b"").decode(), name


def test_refusals_name_the_source_and_the_field_and_leave_the_engine_usable(pp, eng):
    """Case 7."""
    PP_ERR_ARG, PP_ERR_UNSUPPORTED = 1, 5
    ing = pp.ingest
    good, k = depth_cases.scene(pp, 1, 64, 48, step_pad=6, scale=0.2)
    lay = ing.depth_layout_of(good, k)
    data = np.frombuffer(good[0], np.uint8)
    msg = ing.depth_to_pointcloud2(good, k, ordered=True, point_step=20)
    mlay = ing.layout_of(msg)
    mdata = np.frombuffer(msg[0], np.uint8)
    frames = [np.ascontiguousarray(pp.synth.d435i_cloud(400 + b, 4096) * np.float32(0.25)) for b in range(2)]
    want = _copy(eng.detect(frames))

    def call(kind, S, fmap, batch, layouts=None, sel=None, offs=None, asynchronous=False):
        d, l = (data, lay) if kind == "depth" else (mdata, mlay)
        return _raw(eng, kind, np.concatenate([d] * S), offs if offs is not None else [d.size * s for s in range(S + 1)],
                    layouts if layouts is not None else [dict(l)] * S, sel if sel is not None else [(1, 4)] * S, fmap, batch,
                    asynchronous)

    for kind in ("depth", "pointcloud2"):
        assert call(kind, 4, [0, 0, 1, 1], 2)[0] == 0
        for asynchronous in (False, True):
            maps = [
                # (sources, frame map, batch, words the message must hold)
                (3, [1, 1, 1], 2, ["source 0", "source_frame 1", "starts at frame 0"]),
                (3, [0, 1, 0], 2, ["source 2", "source_frame 0 < 1", "never decreases"]),
                (3, [0, 0, 2], 3, ["source 2", "source_frame 2 skips frame 1"]),
                (3, [0, 1, 1], 3, ["source 2", "source_frame 1", "ends at frame batch - 1 = 2"]),
                (3, [0, 1, 2], 2, ["source 2", "source_frame 2", "ends at frame batch - 1 = 1"]),
                (18, [0] * 17 + [1], 2, ["source 16", "frame 0 has more than PP_RIG_MAX_SOURCES=16 sources"]),
                (4, [0, 1, 2, 3], 4, ["max_batch=3"]),
                (2, [0, 0], 0, ["batch 0 outside"]),
            ]
            for S, fmap, batch, words in maps:
                st, text, name = call(kind, S, fmap, batch, asynchronous=asynchronous)
                assert st == PP_ERR_ARG, (kind, fmap, batch, st, text)
                for w in words:
                    assert w in text, (w, text)
            st, text, name = call(kind, 2, [0, 1], 2, sel=[(1, 4), (1, 0)], asynchronous=asynchronous)
            assert st == PP_ERR_ARG and f"{name}: source 1: decimate 0 < 1" in text, text
            st, text, name = call(kind, 2, [0, 0], 1, sel=[(-1, 4), (1, 4)], asynchronous=asynchronous)
            assert st == PP_ERR_ARG and f"{name}: source 0: first -1 < 0" in text, text
            d = data if kind == "depth" else mdata
            st, text, name = call(kind, 3, [0, 0, 1], 2, offs=[0, d.size, 2 * d.size - 1, 3 * d.size - 1], asynchronous=asynchronous)
            assert st == PP_ERR_ARG and f"{name}: source 1: byte_offsets" in text and "row_step" in text, text

    def bad(kind, s, **kw):
        ls = [dict(lay if kind == "depth" else mlay) for _ in range(3)]
        ls[s].update(kw)
        return ls

    nan = float("nan")
    per_source = [
        ("depth", bad("depth", 1, row_step=127), PP_ERR_ARG, ["source 1", "row_step 127 < width 64 x 2 bytes"]),
        ("depth", bad("depth", 2, encoding=2), PP_ERR_ARG, ["source 2", "unknown encoding 2"]),
        ("depth", bad("depth", 0, width=-1), PP_ERR_ARG, ["source 0", "width -1"]),
        ("depth", bad("depth", 2, fx=0.0), PP_ERR_ARG, ["source 2", "fx 0 "]),
        ("depth", bad("depth", 1, fy=nan), PP_ERR_ARG, ["source 1", "fy nan"]),
        ("depth", bad("depth", 1, ppx=nan), PP_ERR_ARG, ["source 1", "ppx nan"]),
        ("depth", bad("depth", 0, depth_scale=0.0), PP_ERR_ARG, ["source 0", "depth_scale 0 "]),
        ("depth", bad("depth", 2, z_min=2.0, z_max=1.0), PP_ERR_ARG, ["source 2", "z_min 2 > z_max 1"]),
        ("pointcloud2", bad("pointcloud2", 1, row_step=mlay["row_step"] - 1), PP_ERR_ARG, ["source 1", "row_step", "point_step 20"]),
        ("pointcloud2", bad("pointcloud2", 2, z_offset=17), PP_ERR_ARG, ["source 2", "z_offset 17 (4 bytes) does not fit point_step 20"]),
        ("pointcloud2", bad("pointcloud2", 0, datatype=5), PP_ERR_UNSUPPORTED, ["source 0", "datatype 5 is an integer type"]),
        ("pointcloud2", bad("pointcloud2", 1, datatype=7 | 8 << 8 | 7 << 16), PP_ERR_UNSUPPORTED, ["source 1", "x, y and z differ (7, 8, 7)"]),
        ("pointcloud2", bad("pointcloud2", 2, datatype=9), PP_ERR_ARG, ["source 2", "unknown datatype 9"]),
    ]
    for kind, layouts, status, words in per_source:
        for asynchronous in (False, True):
            st, text, name = call(kind, 3, [0, 0, 1], 2, layouts=layouts, asynchronous=asynchronous)
            assert st == status and name + ": " in text, (kind, words, st, text)
            for w in words:
                assert w in text, (w, text)

    # a frame whose sources' summed bounds exceed max_points_per_frame: 64 x 48 at (0, 1) keeps up to 3072 points, 11 such
    # sources fit a frame of 36000, the 12th does not
    fit = NMAX // 3072
    assert fit == 11 and mlay["width"] * mlay["height"] == 3072
    for kind in ("depth", "pointcloud2"):
        assert call(kind, fit, [0] * fit, 1, sel=[(0, 1)] * fit)[0] == 0
        S = fit + 2
        st, text, name = call(kind, S, [0] + [1] * (S - 1), 2, sel=[(0, 1)] * S)
        assert st == PP_ERR_ARG and f"{name}: source {fit + 1}: frame 1 keeps up to {(fit + 1) * 3072} points" in text, text
        assert f"max_points_per_frame={NMAX}" in text, text
    # null arguments
    st = eng._lib.pp_ingest_rig_depth(eng._h, None, None, None, None, None, 1, 1, None, 0)
    assert st == PP_ERR_ARG and "pp_ingest_rig_depth: null argument" in eng._lib.pp_last_error(eng._h).decode()
    # the sources' counts of a plain ingest do not exist
    eng.ingest_depth([good], k)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_ingest_rig_info: the last ingest was no rig call"):
        eng.ingest_rig_info()
    rig = ing.CameraRig([ing.Mount.realsense()] * 2, k)
    eng.ingest_rig_depth([[good, good]], rig)
    fin = np.zeros(3, np.int32)
    st = eng._lib.pp_ingest_rig_info(eng._h, fin.ctypes.data_as(ctypes.c_void_p), None, 3)
    assert st == PP_ERR_ARG and "had 2 sources, sources is 3" in eng._lib.pp_last_error(eng._h).decode()
    # the tap's capacity: below the kept total is refused, the frames stay resident
    n_kept = len(ing.rig_depth_ingest_np([good, good], rig)[0])
    pts = np.empty((10, 3), np.float32)
    from pp_amd import engine
    offs = np.array([0, data.size, 2 * data.size], np.int64)
    both = np.concatenate([data, data])
    arr = engine._rig_depth_layouts([good, good], rig)
    fm = np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    st = eng._lib.pp_ingest_rig_depth(eng._h, p(both), p(offs), arr, engine._rig_configs(rig, 1), p(fm), 2, 1, p(pts), 10)
    text = eng._lib.pp_last_error(eng._h).decode()
    assert n_kept > 10 and st == PP_ERR_ARG and "pp_ingest_rig_depth: points_out holds 10 points" in text and str(n_kept) in text, text
    assert eng.ingest_info()["kept"].tolist() == [n_kept]
    # through the Python layer the library's text reaches the caller, and the host layer's own refusals name their field
    with pytest.raises(RuntimeError, match=rf"PP_ERR_ARG.*pp_ingest_rig_depth: source 1: frame 0 keeps up to.*max_points_per_frame={NMAX}"):
        eng.ingest_rig_depth([[pp.synth.depth_from_z(np.zeros((128, 260)))] * 2],
                             ing.CameraRig([ing.Mount.realsense()] * 2, k, first=0, decimate=1))
    with pytest.raises(ValueError, match="frame 1 has 1 sources, the rig has 2 cameras"):
        eng.ingest_rig_depth([[good, good], [good]], rig)
    with pytest.raises(ValueError, match="needs intrinsics"):
        eng.ingest_rig_depth([[good]], ing.CameraRig([ing.Mount.realsense()]))
    # nothing of the refused calls was queued: the engine still detects what it detected before
    _same_detections(eng.detect(frames), want, "detect after the refusals")
    _check_depth(pp, eng, [[good, good]], rig, "after the refusals")


def test_point_features_other_than_xyz_are_unsupported(pp, hip_lib):
    ing = pp.ingest
    e4 = pp.Engine(pp.config.kitti_shaped_config(1), max_batch=1, max_points_per_frame=8192)
    img, k = depth_cases.scene(pp, 1, 64, 48)
    rig = ing.CameraRig([ing.Mount.realsense()] * 2, k)
    msgs = [ing.depth_to_pointcloud2(img, k)] * 2
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*pp_ingest_rig_depth: num_point_features is 4"):
        e4.ingest_rig_depth([[img, img]], rig)
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*pp_ingest_rig_pointcloud2: num_point_features is 4"):
        e4.ingest_rig_pointcloud2([msgs], rig)
    st, sm = e4.staging_rig_depth([[img, img]], rig), e4.staging_rig_pointcloud2([msgs], rig)
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*pp_ingest_rig_depth_async: num_point_features is 4"):
        e4.ingest_rig_depth_async(st, rig)
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*pp_ingest_rig_pointcloud2_async: num_point_features is 4"):
        e4.ingest_rig_pointcloud2_async(sm, rig)
    st.close()
    sm.close()
    e4.close()


def test_rig_ingest_while_a_training_step_is_in_flight_is_a_state_error(pp, hip_lib):
    ing = pp.ingest
    B = 2
    cfg = pp.config.pedestrian_d435i_config(B)
    d = pp.config.Derived(cfg)
    tr = pp.Trainer(cfg, pp.weights.init_weights(d, seed=7), max_batch=B, max_points_per_frame=8192, learning_rate=2e-4,
                    weight_decay=1e-4)
    e = tr.engine
    frames = [pp.synth.d435i_cloud(500 + b, 4096) for b in range(B)]
    gts = [np.array([[3.0, 0.2 * b, 0.0, 0.6, 0.8, 1.73, 0.1]], np.float32) for b in range(B)]
    pairs = [depth_cases.scene(pp, 40 + c, 64, 48, encoding=("16UC1", "32FC1")[c]) for c in range(2)]
    rig = ing.CameraRig(_three_mounts(pp)[:2], [p[1] for p in pairs])
    rf = [[p[0] for p in pairs]] * B
    msgs = [[ing.depth_to_pointcloud2(p[0], p[1]) for p in pairs]] * B
    st, sm = e.staging_rig_depth(rf, rig), e.staging_rig_pointcloud2(msgs, rig)
    e.upload(frames)
    e.train_step_gt_async(tr.params.data_ptr(), tr.grads.data_ptr(), tr.state.data_ptr(), *e.pack_gt(gts))
    for name, fn in (("pp_ingest_rig_depth", lambda: e.ingest_rig_depth(rf, rig)),
                     ("pp_ingest_rig_pointcloud2", lambda: e.ingest_rig_pointcloud2(msgs, rig)),
                     ("pp_ingest_rig_depth_async", lambda: e.ingest_rig_depth_async(st, rig)),
                     ("pp_ingest_rig_pointcloud2_async", lambda: e.ingest_rig_pointcloud2_async(sm, rig))):
        with pytest.raises(RuntimeError, match=f"PP_ERR_STATE.*{name}: a training step is in flight"):
            fn()
    losses = e.train_step_wait()
    assert np.isfinite(losses["loss"])
    _check_depth(pp, e, rf, rig, "after the step")      # after the step the same handle ingests
    st.close()
    sm.close()
    tr.close()


def test_augment_after_a_rig_ingest_is_refused_as_after_a_plain_ingest(pp, eng):
    img, k = depth_cases.scene(pp, 1, 64, 48, scale=0.2)
    rig = pp.ingest.CameraRig([pp.ingest.Mount.realsense()] * 2, k)
    eng.ingest_rig_depth([[img, img]], rig)
    gt = [np.array([[0.8, 0.0, 0.0, 0.6, 0.8, 1.73, 0.1]], np.float32)]
    draws = pp.augment.draw(np.random.RandomState(1), gt, pp.augment.AugmentConfig.from_input_reader(None))
    with pytest.raises(RuntimeError, match="device only.*upload frames first"):
        eng.augment(gt, draws=draws)


def _same_dicts(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.keys() == w.keys() and g["batch_idx"] == w["batch_idx"]
        for key in w:
            assert (g[key] is None) == (w[key] is None), key
            if w[key] is not None:
                assert np.array_equal(g[key], w[key]), key


def test_voxelnet_detect_rig_returns_detects_dicts(pp, hip_lib, three_cameras):
    frames, rig = three_cameras
    net = pp.VoxelNet(pp.config.tiny_config(2), max_batch=2, max_points_per_frame=2048)
    net.load_weights(pp.weights.init_weights(net.d, seed=7))
    R, T = _calib(2)
    host = [pp.ingest.rig_depth_ingest_np(fr, rig)[0] for fr in frames]
    want = net.detect(host, R, T, image_idx=[7, 8])
    _same_dicts(net.detect_rig_depth(frames, rig, R, T, image_idx=[7, 8]), want)
    msgs = [[pp.ingest.depth_to_pointcloud2(img, rig.intrinsics[c]) for c, img in enumerate(fr)] for fr in frames]
    _same_dicts(net.detect_rig_pointcloud2(msgs, rig, R, T, image_idx=[7, 8]), want)
    net.engine.close()
