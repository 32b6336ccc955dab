"""Image boxes on the GPU: pp_box3d_to_bbox (csrc/box_project.hip) and the projection at the end of the detector's
post-process (k_postprocess<., true>) against the reference's arrays (tests/golden/ref_bbox.npz), the host restatement
(projection.box3d_to_bbox) and each other.

Tolerance (projection_ref.py derives it, test_projection_host.py measures K_REF): both entry points stay within K = 4 units
of the formula in extended precision, a unit being 2^-52 times the element's condition magnitude.  The two entry points
share one device function: on the same box3d_camera doubles they agree bit for bit.  Measured on an MI355X: 0.51 units at
worst on the fixture's boxes, 0.42 on the detector's -- on every row the restatement's own figure.
"""
import copy

import numpy as np
import pytest

from conftest import load_golden

import projection_ref as pr

pytestmark = pytest.mark.gpu

B = 3


@pytest.fixture(scope="module")
def fx():
    g = load_golden("ref_bbox.npz")
    boxes, counts, p2, kind, frame, pb = pr.fixture(g)
    return dict(g=g, boxes=boxes, counts=counts, p2=p2, kind=kind, frame=frame, pb=pb)


def _within_k(pp, boxes, p2_per_box, got, what):
    """got [N,4] within K units of L on the rows whose corners all keep |w'| >= 0.5 (the regime K was derived for); returns
    the number of rows compared."""
    _, corners, _, cond = pp.projection.box3d_to_bbox(boxes, p2_per_box, return_parts=True)
    P = np.asarray(p2_per_box)
    w = corners[:, :, 0] * P[:, None, 2, 0] + corners[:, :, 1] * P[:, None, 2, 1] + corners[:, :, 2] * P[:, None, 2, 2]
    ok = np.all(np.abs(w) >= 0.5, axis=1)
    if not ok.any():
        return 0
    exact, rows = pr.exact_points(boxes[ok], p2_per_box[ok])
    r = pr.bbox_ratios(got[ok][rows], exact, cond[ok][rows])
    host = pr.bbox_ratios(pp.projection.box3d_to_bbox(boxes[ok], p2_per_box[ok])[rows], exact, cond[ok][rows])
    print(f"{what}: {int(ok.sum())} of {len(boxes)} rows, GPU worst {r.max():.3f} units, restatement {host.max():.3f}; K = {pr.K}")
    assert r.max() <= pr.K, what
    return int(ok.sum())


# ---------------------------------------------------------------- standalone kernel
def test_fixture_within_k_and_degenerate_by_class(pp, hip_lib, fx):
    got = pp.projection.box3d_to_bbox_gpu(fx["boxes"], fx["counts"], fx["p2"])
    assert got.shape == (203, 4) and got.dtype == np.float64
    reg = fx["kind"] != 3
    assert _within_k(pp, fx["boxes"][reg], fx["pb"][reg], got[reg], "fixture") == 202
    assert np.array_equal(pr.number_class(got[~reg]), pr.number_class(fx["g"]["bbox"][~reg]))
    assert np.isfinite(got[reg]).all()
    again = pp.projection.box3d_to_bbox_gpu(fx["boxes"], fx["counts"], fx["p2"])
    assert got.tobytes() == again.tobytes()
    # every frame took its own matrix: frame 1's boxes under frame 0's matrix give other numbers
    f1 = fx["frame"] == 1
    assert not np.array_equal(pp.projection.box3d_to_bbox_gpu(fx["boxes"][f1], [f1.sum()], fx["p2"][0]), got[f1])


def test_empty_calls_and_a_frame_without_boxes(pp, hip_lib, fx):
    assert pp.projection.box3d_to_bbox_gpu(np.zeros((0, 7)), [0, 0], fx["p2"][:2]).shape == (0, 4)
    assert pp.projection.box3d_to_bbox_gpu(np.zeros((0, 7)), [], fx["p2"][:0]).shape == (0, 4)
    L = pp._lib.lib()
    assert L.pp_box3d_to_bbox(0, None, None, 0, None, None) == 0                  # frames = 0: PP_OK, nothing touched
    neg = np.array([2, -1], np.int32)
    assert L.pp_box3d_to_bbox(0, fx["boxes"].ctypes.data, neg.ctypes.data, 2, fx["p2"].ctypes.data, None) == 1   # PP_ERR_ARG
    # counts [3, 0, 4]: the last four boxes belong to the third matrix, not the second
    b = fx["boxes"][:7]
    got = pp.projection.box3d_to_bbox_gpu(b, [3, 0, 4], fx["p2"][:3])
    want = np.concatenate([pp.projection.box3d_to_bbox_gpu(b[:3], [3], fx["p2"][0]),
                           pp.projection.box3d_to_bbox_gpu(b[3:], [4], fx["p2"][2])])
    assert got.tobytes() == want.tobytes()
    assert not np.array_equal(got[3:], pp.projection.box3d_to_bbox_gpu(b[3:], [4], fx["p2"][1]))


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_wavefront_edges(pp, hip_lib, fx, n):
    reg = np.nonzero(fx["kind"] == 0)[0][:n]
    boxes = fx["boxes"][reg]
    split = [n // 2, n - n // 2]
    got = pp.projection.box3d_to_bbox_gpu(boxes, split, fx["p2"][[1, 3]])
    assert got.shape == (n, 4)
    pb = fx["p2"][[1, 3]][np.repeat([0, 1], split)]
    assert _within_k(pp, boxes, pb, got, f"n = {n}") == n
    if n == 65:     # more than one block as well: 257 and 600 boxes, the tail block partly filled
        for m in (257, 600):
            big = np.tile(boxes, (m // n + 1, 1))[:m]
            out = pp.projection.box3d_to_bbox_gpu(big, [m], fx["p2"][2])
            one = pp.projection.box3d_to_bbox_gpu(boxes, [n], fx["p2"][2])
            assert out.tobytes() == np.tile(one, (m // n + 1, 1))[:m].tobytes()


# ---------------------------------------------------------------- fused into the post-process
def _calib():
    """rect = I; Trv2c of the production path with the camera 6 m behind the lidar: every box of the 0 .. 6.4 m grid lies
    well in front of the image plane."""
    rect = np.eye(4, dtype=np.float32)
    trv = np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 6], [0, 0, 0, 1]], dtype=np.float32)
    return np.stack([rect] * B), np.stack([trv] * B)


def _p2s(shift=0.0):
    out = []
    for f, cx, cy, tx in [(721.5377, 609.5593, 172.854, 44.85728), (384.2, 320.7, 243.1, 12.5), (910.25, 640.5, 360.75, -3.5)]:
        m = np.array([[f + shift, 0, cx, tx], [0, f + shift, cy - shift, 0.2], [0, 0, 1, 0.003], [0, 0, 0, 1]], np.float32)
        out.append(m.astype(np.float64))
    return np.stack(out)


def _frames():
    import pp_amd
    return [pp_amd.synth.d435i_cloud(900, 4096), np.zeros((0, 3), np.float32), pp_amd.synth.d435i_cloud(901, 4096)]


def _engine(pp, rotate=False, project=False):
    cfg = pp.config.pedestrian_d435i_config(B)
    if rotate:
        cfg["model"]["second"]["use_rotate_nms"] = True
    if project:
        cfg["model"]["second"]["project_bbox"] = True
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=8192)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    return eng


def _kept_bytes(dets, n):
    return [dets[b][:int(n[b])].tobytes() for b in range(len(n))]


def _check_bboxes(pp, dets, n, bb, p2, what):
    """Rows below a frame's count: bit-equal to the standalone kernel on the same doubles, within K of L; rows at and
    beyond it: not written (zero in Engine.bboxes)."""
    compared = 0
    for b in range(len(n)):
        k = int(n[b])
        assert not bb[b, k:].any(), (what, b)
        if k == 0:
            continue
        cam = np.ascontiguousarray(dets[b]["box3d_camera"][:k])
        alone = pp.projection.box3d_to_bbox_gpu(cam, [k], p2[b])
        assert bb[b, :k].tobytes() == alone.tobytes(), (what, b)
        compared += _within_k(pp, cam, np.broadcast_to(p2[b], (k, 4, 4)), bb[b, :k], f"{what} frame {b}")
    return compared


@pytest.mark.parametrize("mode", ["standup", "rotated"])
def test_fused_projection(pp, hip_lib, mode):
    eng = _engine(pp, rotate=(mode == "rotated"))
    try:
        assert eng.nms_mode == mode and eng.projection is False
        rect, trv = _calib()
        frames, p2 = _frames(), _p2s()
        off, noff = (a.copy() for a in eng.detect(frames, rect, trv))
        with pytest.raises(RuntimeError, match="PP_ERR_STATE"):
            eng.bboxes()
        dets, n = (a.copy() for a in eng.detect(frames, rect, trv, p2=p2, bbox=True))
        assert eng.projection is True
        bb = eng.bboxes(B)
        print(f"{mode}: kept {n.tolist()}")
        assert bb.shape == (B, eng.d.nms_post_max_size, 4) and bb.dtype == np.float64
        assert int(n[1]) == 0 and int(n[0]) > 0 and int(n[2]) > 0
        assert _check_bboxes(pp, dets, n, bb, p2, mode) > 0
        # the detections do not know about the projection
        assert np.array_equal(n, noff) and _kept_bytes(dets, n) == _kept_bytes(off, noff)
        with pytest.raises(ValueError, match="bbox=True needs p2"):
            eng.detect(frames, rect, trv, bbox=True)
        assert eng._lib.pp_set_projection(eng._h, p2.ctypes.data, B + 1) == 1          # PP_ERR_ARG
        assert eng._lib.pp_set_projection(eng._h, p2.ctypes.data, 0) == 1
        assert eng.projection is True
    finally:
        eng.close()


def test_predict_path(pp, hip_lib):
    eng = _engine(pp)
    try:
        rect, trv = _calib()
        frames, p2 = _frames(), _p2s()
        eng.detect(frames, rect, trv)
        im = eng.intermediates()
        args = (im["box_preds"], im["cls_preds"], im["dir_cls_preds"], im["anchors_mask"], rect, trv)
        off, noff = eng.predict(*args)
        with pytest.raises(RuntimeError, match="PP_ERR_STATE"):
            eng.bboxes()
        dets, n = eng.predict(*args, p2=p2)
        bb = eng.bboxes(B)
        assert int(n[1]) == 0 and int(n[0]) > 0
        assert _check_bboxes(pp, dets, n, bb, p2, "predict") > 0
        assert np.array_equal(n, noff) and _kept_bytes(dets, n) == _kept_bytes(off, noff)
        # fewer matrices than frames: refused, not read past
        eng.set_projection(p2[:2])
        with pytest.raises(RuntimeError, match="PP_ERR_STATE"):
            eng.predict(*args)
    finally:
        eng.close()


def test_replay_reads_the_current_matrices(pp, hip_lib):
    eng = _engine(pp)
    try:
        rect, trv = _calib()
        frames = _frames()
        first, second = _p2s(), _p2s(shift=37.5)
        eng.detect(frames, rect, trv, p2=first, bbox=True)             # captures the pass with projection on
        dets, n = (a.copy() for a in eng.detect(frames, rect, trv, p2=first, bbox=True))
        bb1 = eng.bboxes(B)
        dets2, n2 = (a.copy() for a in eng.detect(frames, rect, trv, p2=second, bbox=True))     # the same captured pass
        bb2 = eng.bboxes(B)
        assert _kept_bytes(dets, n) == _kept_bytes(dets2, n2)
        _check_bboxes(pp, dets, n, bb1, first, "first matrices")
        _check_bboxes(pp, dets2, n2, bb2, second, "second matrices")
        k = int(n[0])
        assert k > 0 and not np.array_equal(bb1[0, :k], bb2[0, :k])
        # off again: no boxes to fetch, and the dict holds the placeholder
        eng.set_projection(None)
        assert eng.projection is False
        dets3, n3 = eng.detect(frames, rect, trv)
        assert _kept_bytes(dets, n) == _kept_bytes(dets3, n3)
        out = np.zeros((B, eng.d.nms_post_max_size, 4))
        assert eng._lib.pp_get_bboxes(eng._h, out.ctypes.data) == 2 and not out.any()          # PP_ERR_STATE
        d = pp.VoxelNet._to_dict(dets3[0], int(n3[0]), 0)
        assert np.array_equal(d["bbox"], np.tile([[400., 200., 500., 400.]], (k, 1)))
    finally:
        eng.close()


def test_voxelnet_project_bbox(pp, hip_lib):
    rect, trv = _calib()
    frames, p2 = _frames(), _p2s()
    cfg = pp.config.pedestrian_d435i_config(B)
    plain = pp.VoxelNet(copy.deepcopy(cfg), max_batch=B, max_points_per_frame=8192)
    cfg["model"]["second"]["project_bbox"] = True
    net = pp.VoxelNet(cfg, max_batch=B, max_points_per_frame=8192)
    fresh = _engine(pp)                      # a handle that never heard of projection
    try:
        w = pp.weights.init_weights(net.d, seed=7)
        net.load_weights(w)
        plain.load_weights(w)
        with pytest.raises(ValueError, match="project_bbox"):
            net.detect(frames, rect, trv)
        out = net.detect(frames, rect, trv, p2=p2)
        base = plain.detect(frames, rect, trv)
        fdets, fn = fresh.detect(frames, rect, trv)
        want = [pp.VoxelNet._to_dict(fdets[b], int(fn[b]), b) for b in range(B)]
        for b in range(B):
            assert sorted(base[b]) == sorted(want[b])
            for key in base[b]:           # key absent: byte-equal to a run that never heard of projection
                if base[b][key] is None or np.isscalar(base[b][key]):
                    assert base[b][key] == want[b][key]
                else:
                    assert base[b][key].dtype == want[b][key].dtype and base[b][key].tobytes() == want[b][key].tobytes()
        assert out[1]["bbox"] is None and out[1]["box3d_camera"] is None
        for b in (0, 2):
            n = len(out[b]["scores"])
            assert out[b]["bbox"].shape == (n, 4) and out[b]["bbox"].dtype == np.float64
            assert not np.array_equal(out[b]["bbox"], base[b]["bbox"])
            assert out[b]["bbox"].tobytes() == pp.projection.box3d_to_bbox_gpu(out[b]["box3d_camera"], [n], p2[b]).tobytes()
            for key in ("box3d_camera", "box3d_lidar", "scores", "label_preds"):
                assert out[b][key].tobytes() == base[b][key].tobytes()
        # predict(example, preds) takes P2 from example[5]
        im = net.engine.intermediates()
        ex = (None, None, None, rect, trv, p2, np.stack([net.engine.anchors] * B), im["anchors_mask"], np.arange(B), None)
        again = net.predict(ex, im)
        for b in (0, 2):
            assert again[b]["bbox"].tobytes() == out[b]["bbox"].tobytes()
    finally:
        for e in (net.engine, plain.engine, fresh):
            e.close()


def test_end_to_end_bbox_ap(pp, hip_lib):
    """Detections on 4 frames, ground truth made of the same detections with the restatement's image boxes: the evaluator's
    bbox AP at the lowest tier is above zero with the projected boxes and zero with the placeholder.  The principal point
    is placed so that the scene projects below the placeholder's rows (200 .. 400)."""
    cfg = pp.config.pedestrian_d435i_config(4)
    cfg["model"]["second"]["project_bbox"] = True
    net = pp.VoxelNet(cfg, max_batch=4, max_points_per_frame=8192)
    try:
        net.load_weights(pp.weights.init_weights(net.d, seed=7))
        frames = [pp.synth.d435i_cloud(900 + i, 4096) for i in range(4)]
        rect, trv = (np.stack([m[0]] * 4) for m in _calib())
        p2 = np.array([[700.0, 0, 620.0, 40.0], [0, 700.0, 1400.0, 0.2], [0, 0, 1, 0.003], [0, 0, 0, 1]])
        preds = net.detect(frames, rect, trv, p2=p2)
        placeholder = [dict(p, bbox=np.tile([[400., 200., 500., 400.]], (len(p["scores"]), 1))) for p in preds]
        example = (None,) * 9 + (np.array([[2000, 1300]] * 4),)
        dts = pp.anno.predict_kitti_to_anno(example, ["Pedestrian"], preds)
        dts_placeholder = pp.anno.predict_kitti_to_anno(example, ["Pedestrian"], placeholder)
        gts = []
        for a in dts:
            g = {k: v.copy() for k, v in a.items() if k != "score"}
            cam = np.concatenate([a["location"], a["dimensions"], a["rotation_y"][:, None]], axis=1)
            g["bbox"] = pp.projection.box3d_to_bbox(cam, p2)
            gts.append(g)
        assert sum(len(a["name"]) for a in dts) > 0
        heights = np.concatenate([g["bbox"][:, 3] - g["bbox"][:, 1] for g in gts])
        print(f"{len(heights)} boxes, image heights {heights.min():.1f} .. {heights.max():.1f}")
        _, ap, _, _, _ = pp.kitti_eval.get_official_eval_result(gts, dts, ["Pedestrian"], compute_bbox=True, statistics="gpu")
        _, ap0, _, _, _ = pp.kitti_eval.get_official_eval_result(gts, dts_placeholder, ["Pedestrian"], compute_bbox=True,
                                                                statistics="gpu")
        print(f"bbox AP, lowest tier: projected {ap[0, :, 0].tolist()}, placeholder {ap0[0, :, 0].tolist()}")
        assert (ap[0, :, 0] > 0).all()
        assert (ap0[0, :, 0] == 0).all()
    finally:
        net.engine.close()
