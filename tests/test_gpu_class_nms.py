"""Per-class suppression in the one-launch post-process (pp_set_class_nms, model.second.use_multi_class_nms) on the GPU,
against the host oracle tests/class_nms_ref.py: oracle.ref_numpy.predict once per class on that class's logit column.

Inputs: per frame and class the logits are a permutation of linspace(-4, 4, A), offset by 1e-4 * c, so the scores that
matter are pairwise distinct (asserted on the host first) and the oracle's argpartition / argsort have no ties to break.
Counts, labels, anchor_index and dir_label are compared exactly; scores within 1e-6, lidar boxes within 1e-5 (the
tolerances tests/test_gpu_round2.py uses against this oracle on hand-made head maps), camera boxes within 1e-4."""
import numpy as np
import pytest

from oracle import ref_numpy as rn
import class_nms_ref as cr
import rotate_nms_ref as rr

pytestmark = pytest.mark.gpu

CAM_TOL = 1e-4      # tests/test_gpu_round2.py::_assert_dets


def _config(pp, grid, B, ncls, thr=0.0, post=None, per_class=True):
    cfg = {"d435i": pp.config.pedestrian_d435i_config, "tiny": pp.config.tiny_config,
           "kitti": pp.config.kitti_shaped_config}[grid](B)
    s = cfg["model"]["second"]
    s.update(num_class=ncls, nms_score_threshold=thr, use_multi_class_nms=per_class and ncls > 1)
    if post is not None:
        s["nms_post_max_size"] = post
    return cfg


def _engine(pp, grid, B, ncls, **kw):
    return pp.Engine(_config(pp, grid, B, ncls, **kw), max_batch=B, max_points_per_frame=4096)


def _logits(rng, B, A, ncls, lo=-4.0, hi=4.0):
    return np.stack([np.stack([rng.permutation(np.linspace(lo, hi, A)) + 1e-4 * c for c in range(ncls)], axis=-1)
                     for _ in range(B)]).astype(np.float32)


def _strong_in_both(logits, mask, count, rng):
    """`count` masked anchors of every frame get, in classes 0 and 1, that class's `count` largest logits in the same
    order (values are swapped, so each column stays a permutation): the best anchor of both classes is the same one."""
    for b in range(logits.shape[0]):
        chosen = rng.choice(np.nonzero(mask[b] == 1)[0], size=count, replace=False)
        for c in (0, 1):
            col = logits[b, :, c]
            best = np.argsort(-col, kind="stable")[:count]          # where the largest values are now, largest first
            top = col[best].copy()
            touched = np.union1d(chosen, best)
            rest = np.setdiff1d(col[touched], top)                   # the values the chosen anchors give up
            col[np.setdiff1d(touched, chosen)] = rest
            col[chosen] = top
    return logits


def _heads(d, B, ncls, seed, logits=None):
    rng = np.random.default_rng(seed)
    A, napl = d.num_anchors, d.num_anchor_per_loc
    lg = _logits(rng, B, A, ncls) if logits is None else logits
    return {"box_preds": (0.3 * rng.standard_normal((B, d.head_h, d.head_w, napl * 7))).astype(np.float32),
            "cls_preds": np.ascontiguousarray(lg.reshape(B, d.head_h, d.head_w, napl * ncls)),
            "dir_cls_preds": rng.standard_normal((B, d.head_h, d.head_w, napl * 2)).astype(np.float32)}


def _calib(pp, B):
    rect, trv, _ = pp.synth.default_calib()
    return np.stack([rect] * B), np.stack([trv] * B)


def _example(eng, mask, rect, trv):
    B = mask.shape[0]
    return (None, None, None, rect, trv, None, np.stack([eng.anchors] * B), mask, np.arange(B), None)


def _run(eng, preds, mask, rect, trv, **kw):
    return eng.predict(preds["box_preds"], preds["cls_preds"], preds["dir_cls_preds"], mask, rect, trv, **kw)


def _assert_frames(dets, n, ref, what=""):
    assert dets.shape[0] == len(ref)
    for b, fr in enumerate(ref):
        k = len(fr["scores"])
        got = dets[b][:k]
        print(f"{what} frame {b}: GPU {int(n[b])} rows, oracle per class {fr['class_counts'].tolist()}")
        assert int(n[b]) == k, (what, b, int(n[b]), fr["class_counts"])
        assert np.array_equal(got["label"], fr["label_preds"]), (what, b)
        assert np.array_equal(got["anchor_index"], fr["anchor_index"]), (what, b)
        assert np.array_equal(got["dir_label"], fr["dir_label"]), (what, b)
        if k:
            np.testing.assert_allclose(got["score"], fr["scores"], rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(got["box3d_lidar"], fr["box3d_lidar"], rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(got["box3d_camera"], fr["box3d_camera"], rtol=0, atol=CAM_TOL)


def _kept_bytes(dets, n):
    return [dets[b][:int(n[b])].tobytes() for b in range(len(n))]


def _two_labels(dets, n):
    """Anchors of a frame that are reported under more than one label."""
    out = 0
    for b in range(len(n)):
        rows = dets[b][:int(n[b])]
        pairs = set(zip(rows["anchor_index"].tolist(), rows["label"].tolist()))
        assert len(pairs) == len(rows)                      # an (anchor, class) pair appears once
        out += len(pairs) - len(set(a for a, _ in pairs))
    return out


# ---------------------------------------------------------------- 1: predict on the d435i grid
@pytest.mark.parametrize("ncls", [2, 3, 5])
@pytest.mark.parametrize("thr", [0.0, 0.3])
def test_predict_matches_the_per_class_oracle(pp, hip_lib, ncls, thr):
    """A = 10 240: the keys-in-LDS path; the head rows are scanned (no class plane after pp_predict), 16 strided anchors
    per thread; num_class = 5 is past the four-class fast path's range as well."""
    B = 3
    eng = _engine(pp, "d435i", B, ncls, thr=thr)
    try:
        d = eng.d
        assert d.num_anchors == 10240 and eng.class_nms == "per_class" and eng.detection_rows == ncls * d.nms_post_max_size
        rng = np.random.default_rng(100 + ncls)
        mask = np.stack([(rng.random(d.num_anchors) < p).astype(np.uint8) for p in (0.5, 0.1, 0.9)])
        logits = _strong_in_both(_logits(rng, B, d.num_anchors, ncls), mask, 30, rng)
        preds = _heads(d, B, ncls, 200 + ncls, logits)
        assert cr.distinct_top_scores(preds, mask, ncls)
        rect, trv = _calib(pp, B)
        ref = cr.predict_per_class(_example(eng, mask, rect, trv), preds, d.nms_dict())
        dets, n = _run(eng, preds, mask, rect, trv)
        assert dets.shape == (B, ncls * d.nms_post_max_size)
        _assert_frames(dets, n, ref, f"ncls {ncls} thr {thr}")
        assert all((fr["class_counts"] > 0).all() for fr in ref)
        assert _two_labels(dets, n) >= B, "every frame's best anchor leads two classes: the joint rule cannot report that"
        again, n2 = _run(eng, preds, mask, rect, trv)
        assert np.array_equal(n, n2) and _kept_bytes(dets, n) == _kept_bytes(again, n2)
    finally:
        eng.close()


# ---------------------------------------------------------------- 2: a window of the mask, where suppression happens
def test_clustered_mask_suppresses_within_each_class(pp, hip_lib):
    B, ncls = 2, 2
    eng = _engine(pp, "d435i", B, ncls)
    try:
        d = eng.d
        napl = d.num_anchor_per_loc
        m = np.zeros((B, d.head_h, d.head_w, napl), np.uint8)
        m[0, 10:26, 20:36] = 1
        m[1, 40:56, 3:19] = 1
        mask = m.reshape(B, -1)
        rng = np.random.default_rng(17)
        logits = _strong_in_both(_logits(rng, B, d.num_anchors, ncls), mask, 40, rng)
        preds = _heads(d, B, ncls, 18, logits)
        assert cr.distinct_top_scores(preds, mask, ncls)
        rect, trv = _calib(pp, B)
        ref = cr.predict_per_class(_example(eng, mask, rect, trv), preds, d.nms_dict())
        for fr in ref:
            assert ((fr["class_counts"] >= 2) & (fr["class_counts"] <= d.nms_post_max_size - 1)).all(), fr["class_counts"]
        dets, n = _run(eng, preds, mask, rect, trv)
        _assert_frames(dets, n, ref, "window")
        assert _two_labels(dets, n) >= B
    finally:
        eng.close()


# ---------------------------------------------------------------- 3: empty classes, empty frames, the cap
def test_empty_class_empty_frame_and_the_cap(pp, hip_lib):
    """Frame 0: class 1 has no candidate (threshold 0.3, its logits all below logit(0.3) = -0.847), class 2 follows class
    0 directly.  Frame 1: no anchor is on.  Frame 2: every class keeps exactly nms_post_max_size = 10."""
    B, ncls, post = 3, 3, 10
    eng = _engine(pp, "d435i", B, ncls, thr=0.3, post=post)
    try:
        d = eng.d
        rng = np.random.default_rng(31)
        logits = _logits(rng, B, d.num_anchors, ncls)
        logits[0, :, 1] = rng.permutation(np.linspace(-4.0, -1.0, d.num_anchors)).astype(np.float32)
        mask = (rng.random((B, d.num_anchors)) < 0.5).astype(np.uint8)
        mask[1] = 0
        preds = _heads(d, B, ncls, 32, logits)
        assert cr.distinct_top_scores(preds, mask, ncls)
        rect, trv = _calib(pp, B)
        ref = cr.predict_per_class(_example(eng, mask, rect, trv), preds, d.nms_dict())
        c0 = ref[0]["class_counts"]
        assert c0[1] == 0 and c0[0] > 0 and c0[2] > 0
        assert ref[1]["class_counts"].sum() == 0
        assert (ref[2]["class_counts"] == post).all()
        dets, n = _run(eng, preds, mask, rect, trv)
        _assert_frames(dets, n, ref, "edges")
        assert int(n[1]) == 0 and int(n[2]) == ncls * post == eng.detection_rows
        assert np.array_equal(dets[0]["label"][:int(n[0])], np.repeat([0, 2], [c0[0], c0[2]]))
        # VoxelNet hands every row on; an empty frame is the all-None dict
        dicts = [pp.VoxelNet._to_dict(dets[b], int(n[b]), b) for b in range(B)]
        assert dicts[1]["scores"] is None and len(dicts[2]["scores"]) == ncls * post
    finally:
        eng.close()


# ---------------------------------------------------------------- 4: more candidates than LDS holds
def test_kitti_grid_rescan_path(pp, hip_lib):
    """107 136 anchors, all on: more than the 12 288 candidate keys LDS holds per class, so each class's workgroup takes
    the floor from the first 12 288 and scans the head map once more."""
    B, ncls = 1, 2
    eng = _engine(pp, "kitti", B, ncls)
    try:
        d = eng.d
        assert d.num_anchors == 107136
        mask = np.ones((B, d.num_anchors), np.uint8)
        rng = np.random.default_rng(41)
        logits = _strong_in_both(_logits(rng, B, d.num_anchors, ncls), mask, 20, rng)
        preds = _heads(d, B, ncls, 42, logits)
        assert cr.distinct_top_scores(preds, mask, ncls)
        rect, trv = _calib(pp, B)
        ref = cr.predict_per_class(_example(eng, mask, rect, trv), preds, d.nms_dict())
        dets, n = _run(eng, preds, mask, rect, trv)
        _assert_frames(dets, n, ref, "cfg-K")
        assert (ref[0]["class_counts"] > 0).all() and _two_labels(dets, n) >= 1
    finally:
        eng.close()


# ---------------------------------------------------------------- 5: the fused path
def test_fused_path_graph_replay_and_host_mirrors(pp, hip_lib):
    """detect() on raw clouds: the scan reads the compact class plane (A % 16 == 0), the pass is a captured graph from the
    second call on, and the gather kernel fills the page-locked mirrors.  The expectation is the oracle on the engine's
    own head maps and mask (intermediates()), so both sides read the same bits."""
    B, ncls = 2, 2
    cfg = _config(pp, "tiny", B, ncls)
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=8192)
    try:
        d = eng.d
        assert d.num_anchors % 16 == 0 and eng.class_nms == "per_class"
        eng.load_weights(pp.weights.init_weights(d, seed=7))
        frames = [pp.synth.d435i_cloud(900 + i, 4096) for i in range(B)]
        rect, trv = _calib(pp, B)
        runs = []
        for _ in range(3):
            dets, n = eng.detect(frames, rect, trv)
            runs.append((dets.copy(), n.copy()))
        dets, n = runs[0]
        assert dets.shape == (B, ncls * d.nms_post_max_size)
        im = eng.intermediates()
        preds = {k: im[k] for k in ("box_preds", "cls_preds", "dir_cls_preds")}
        mask = im["anchors_mask"]
        ref = cr.predict_per_class(_example(eng, mask, rect, trv), preds, d.nms_dict())
        _assert_frames(dets, n, ref, "fused")
        assert int(n.sum()) > 0
        for d2, n2 in runs[1:]:
            assert np.array_equal(n, n2) and d2.tobytes() == dets.tobytes()       # rows past the count are zero
        # the stage entry point on the same head maps: the same rows
        pd, pn = _run(eng, preds, mask, rect, trv)
        assert np.array_equal(pn, n) and _kept_bytes(pd, pn) == _kept_bytes(dets, n)
    finally:
        eng.close()


# ---------------------------------------------------------------- 6: switching on one handle
def test_mode_switch_on_one_handle(pp, hip_lib):
    B, ncls = 2, 2
    cfg = _config(pp, "tiny", B, ncls, per_class=False)
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=8192)
    try:
        d = eng.d
        post = d.nms_post_max_size
        assert eng.class_nms == "joint" and eng.detection_rows == post
        eng.load_weights(pp.weights.init_weights(d, seed=7))
        frames = [pp.synth.d435i_cloud(900 + i, 4096) for i in range(B)]
        rect, trv = _calib(pp, B)
        first = tuple(a.copy() for a in eng.detect(frames, rect, trv))
        im = eng.intermediates()
        preds = {k: im[k] for k in ("box_preds", "cls_preds", "dir_cls_preds")}
        mask = im["anchors_mask"]
        joint = rn.predict(_example(eng, mask, rect, trv), preds, d.nms_dict())
        for b in range(B):
            assert int(first[1][b]) == (0 if joint[b]["scores"] is None else len(joint[b]["scores"]))
        eng.set_class_nms("per_class")
        assert eng.class_nms == "per_class" and eng.detection_rows == ncls * post
        with pytest.raises(RuntimeError, match="PP_ERR_STATE"):
            eng.detections()                                   # the resident results have the joint mode's row stride
        second = tuple(a.copy() for a in eng.detect(frames, rect, trv))
        assert second[0].shape == (B, ncls * post)
        _assert_frames(second[0], second[1], cr.predict_per_class(_example(eng, mask, rect, trv), preds, d.nms_dict()), "switched")
        eng.set_class_nms("joint")
        assert eng.detection_rows == post
        with pytest.raises(RuntimeError, match="PP_ERR_STATE"):
            eng.detections()
        third = eng.detect(frames, rect, trv)
        assert third[0].shape == (B, post)
        assert np.array_equal(first[1], third[1]) and first[0].tobytes() == third[0].tobytes()
        with pytest.raises(ValueError):
            eng.set_class_nms("both")
        assert eng._lib.pp_set_class_nms(eng._h, 2) == 1       # PP_ERR_ARG
        assert eng.class_nms == "joint"
    finally:
        eng.close()


# ---------------------------------------------------------------- 7: with the rotated rule
def test_per_class_with_rotated_rule(pp, hip_lib):
    """The rotated rule per class: tests/rotate_nms_ref.predict_rotated as the single pass.  Head maps are redrawn on the
    CPU until no pair's IoU lies within 1e-4 of the threshold, as tests/test_gpu_rotate_nms.py does."""
    B, ncls = 3, 2
    eng = _engine(pp, "tiny", B, ncls)
    try:
        d = eng.d
        eng.set_nms_mode("rotated")
        rect, trv = _calib(pp, B)
        for seed in range(7000, 7400):
            rng = np.random.default_rng(seed)
            mask = (rng.random((B, d.num_anchors)) < 0.6).astype(np.uint8)
            mask[2] = 0
            preds = _heads(d, B, ncls, seed)
            margins = []
            ref = cr.predict_per_class(_example(eng, mask, rect, trv), preds, d.nms_dict(), single=rr.predict_rotated,
                                       margins=margins)
            if min(margins) > 1e-4:
                break
        else:
            raise AssertionError("no draw keeps every IoU 1e-4 from the threshold")
        assert cr.distinct_top_scores(preds, mask, ncls)
        dets, n = _run(eng, preds, mask, rect, trv)
        _assert_frames(dets, n, ref, "rotated")
        assert int(n[2]) == 0 and int(n[0]) > ncls
        eng.set_nms_mode("standup")
        sd, sn = _run(eng, preds, mask, rect, trv)
        _assert_frames(sd, sn, cr.predict_per_class(_example(eng, mask, rect, trv), preds, d.nms_dict()), "standup")
        assert _kept_bytes(sd, sn) != _kept_bytes(dets, n), "the two rules keep different boxes on these maps"
    finally:
        eng.close()


# ---------------------------------------------------------------- 8: with the projection
def test_bboxes_sit_beside_their_detections(pp, hip_lib):
    B, ncls = 3, 2
    eng = _engine(pp, "d435i", B, ncls)
    try:
        d = eng.d
        rng = np.random.default_rng(51)
        mask = (rng.random((B, d.num_anchors)) < 0.5).astype(np.uint8)
        mask[1] = 0
        preds = _heads(d, B, ncls, 52)
        rect, trv = _calib(pp, B)
        p2 = np.stack([np.array([[721.5 + 10 * b, 0, 609.5, 44.8], [0, 721.5, 172.8 + b, 0.2], [0, 0, 1, 0.003], [0, 0, 0, 1]])
                       for b in range(B)])
        off, noff = _run(eng, preds, mask, rect, trv)
        with pytest.raises(RuntimeError, match="PP_ERR_STATE"):
            eng.bboxes()
        dets, n = _run(eng, preds, mask, rect, trv, p2=p2)
        bb = eng.bboxes(B)
        assert bb.shape == (B, ncls * d.nms_post_max_size, 4)
        assert np.array_equal(n, noff) and _kept_bytes(dets, n) == _kept_bytes(off, noff)
        assert int(n[1]) == 0 and int(n[0]) > d.nms_post_max_size
        compared = 0
        for b in range(B):
            k = int(n[b])
            assert not bb[b, k:].any()
            if k == 0:
                continue
            cam = np.ascontiguousarray(dets[b]["box3d_camera"][:k])
            assert bb[b, :k].tobytes() == pp.projection.box3d_to_bbox_gpu(cam, [k], p2[b]).tobytes(), b
            # the host restatement, on the rows whose corners all lie well in front of the camera (float64 on both sides;
            # 1e-9 relative leaves room for the operation order of some thirty operations, nothing more)
            P = np.broadcast_to(p2[b], (k, 4, 4))
            host, corners, _, _ = pp.projection.box3d_to_bbox(cam, P, return_parts=True)
            w = corners @ p2[b][2, :3]
            ok = np.all(w >= 0.5, axis=1)
            np.testing.assert_allclose(bb[b, :k][ok], host[ok], rtol=1e-9, atol=1e-9)
            compared += int(ok.sum())
        assert compared > 20
        # the fused path's mirrors
        eng.set_projection(None)
        eng.close()
        eng = pp.Engine(_config(pp, "tiny", 2, ncls), max_batch=2, max_points_per_frame=8192)
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
        frames = [pp.synth.d435i_cloud(900 + i, 4096) for i in range(2)]
        for _ in range(2):
            fd, fn = eng.detect(frames, rect[:2], trv[:2], p2=p2[:2], bbox=True)
            fb = eng.bboxes(2)
            for b in range(2):
                k = int(fn[b])
                cam = np.ascontiguousarray(fd[b]["box3d_camera"][:k])
                assert not fb[b, k:].any()
                if k:
                    assert fb[b, :k].tobytes() == pp.projection.box3d_to_bbox_gpu(cam, [k], p2[b]).tobytes()
        assert int(fn.sum()) > 0
    finally:
        eng.close()


# ---------------------------------------------------------------- 9: the non-finite flag
def test_nan_in_a_masked_out_class_logit_raises(pp, hip_lib):
    B, ncls = 2, 2
    eng = _engine(pp, "d435i", B, ncls)
    try:
        d = eng.d
        rng = np.random.default_rng(61)
        mask = (rng.random((B, d.num_anchors)) < 0.5).astype(np.uint8)
        preds = _heads(d, B, ncls, 62)
        rect, trv = _calib(pp, B)
        dets, n = _run(eng, preds, mask, rect, trv)
        assert (n > 0).all()
        a = int(np.nonzero(mask[1] == 0)[0][7])
        cls = preds["cls_preds"].reshape(B, -1, ncls)
        cls[1, a, 1] = np.nan
        with pytest.raises(pp.NumericError, match="PP_ERR_NUMERIC"):
            _run(eng, preds, mask, rect, trv)
        cls[1, a, 1] = 0.0
        dets2, n2 = _run(eng, preds, mask, rect, trv)
        assert np.array_equal(n, n2) and _kept_bytes(dets, n) == _kept_bytes(dets2, n2)
    finally:
        eng.close()


# ---------------------------------------------------------------- 10: a class's segment against a one-class engine
def test_segment_equals_a_one_class_engine(pp, hip_lib):
    """Not the oracle, a consistency check: class c's rows are, byte for byte except `label`, what a one-class engine on
    the same grid returns when fed column c -- the default (joint) instantiation, whose code did not change."""
    B, ncls = 2, 3
    eng = _engine(pp, "d435i", B, ncls, thr=0.3)
    one = _engine(pp, "d435i", B, 1, thr=0.3)
    try:
        d = eng.d
        assert one.class_nms == "joint"
        rng = np.random.default_rng(71)
        mask = (rng.random((B, d.num_anchors)) < 0.4).astype(np.uint8)
        preds = _heads(d, B, ncls, 72)
        rect, trv = _calib(pp, B)
        dets, n = _run(eng, preds, mask, rect, trv)
        logits = cr.class_logits(preds, ncls)
        at = np.zeros((B,), np.int64)
        for c in range(ncls):
            p1 = dict(preds, cls_preds=np.ascontiguousarray(logits[:, :, c]).reshape(B, d.head_h, d.head_w, -1))
            od, on = _run(one, p1, mask, rect, trv)
            for b in range(B):
                k = int(on[b])
                seg = dets[b][at[b]:at[b] + k].copy()
                assert k > 0 and (seg["label"] == c).all(), (b, c)
                seg["label"] = 0
                assert seg.tobytes() == od[b][:k].tobytes(), (b, c)
                at[b] += k
        assert np.array_equal(at, n)
    finally:
        eng.close()
        one.close()
