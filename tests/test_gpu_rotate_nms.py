"""Rotated NMS on the GPU: pp_rotate_nms (csrc/rotate_nms.hip) against the reference's keep lists
(tests/golden/ref_rotate_nms.npz) and the host restatement (tests/rotate_nms_ref.py), and the detector's rotated mode
(k_postprocess<PP_NMS_ROTATED>) against predict_rotated.

Keep lists, counts and anchor indices are compared exactly: the kernels share the clip code that test_kitti_eval.py holds
bit-exact to the C oracle, and the inputs keep every IoU at least 1e-4 from its threshold where the two sides may differ
in the last ulp (the reference's emulator; the device's expf in the box decode).  Scores and boxes: 1e-4, as the
existing predict tests.
"""

import numpy as np
import pytest

from conftest import load_golden
from oracle import c_oracle, ref_numpy as rn

import rotate_nms_ref as rr
from test_rotate_nms_host import fixture_cases

pytestmark = pytest.mark.gpu

TOL = 1e-4


def test_fixture_keep_lists(pp, hip_lib):
    g = load_golden("ref_rotate_nms.npz")
    for name, dets, thr, pre, post, keep in fixture_cases(g):
        got = pp.rotate_nms.rotate_nms(dets, thr, pre, post)
        assert got.dtype == np.int64 and np.array_equal(got, keep), name


@pytest.fixture(scope="module")
def thousand():
    rng = np.random.default_rng(1000)
    n = 1000
    side = 1.6 * np.sqrt(n)
    b = np.concatenate([rng.uniform(0, side, (n, 2)), rng.uniform(0.5, 2.5, (n, 2)), rng.uniform(-3.5, 3.5, (n, 1))], axis=1)
    for i in range(n):
        if rng.random() < 0.33:
            j = int(rng.integers(0, n))
            if j != i:
                b[i] = b[j] + np.concatenate([rng.normal(0, 0.06, 2), rng.normal(0, 0.04, 2), rng.normal(0, 0.03, 1)])
    s = (rng.permutation(n).astype(np.float32) + 0.5) / n
    return np.concatenate([b, s[:, None]], axis=1).astype(np.float32)


@pytest.mark.parametrize("thr", [0.3, 0.6])
def test_thousand_boxes_equal_the_host_restatement(pp, hip_lib, thousand, thr):
    ref = rr.rotate_nms_ref(thousand, thr)
    got = pp.rotate_nms.rotate_nms(thousand, thr)
    again = pp.rotate_nms.rotate_nms(thousand, thr)
    print(f"n 1000 thr {thr}: kept {len(got)} (host {len(ref)})")
    assert 0 < len(ref) < 1000
    assert np.array_equal(got, ref)
    assert got.tobytes() == again.tobytes()


def test_cap_ties_and_nan_iou(pp, hip_lib):
    n = pp.rotate_nms.MAX_BOXES + 1
    with pytest.raises(ValueError, match="PP_RNMS_MAX_BOXES"):
        pp.rotate_nms.rotate_nms(np.zeros((n, 6), np.float32), 0.5)
    # under the cap through pre_max_size; equal scores: lower index first; zero-area boxes: NaN IoU suppresses nothing
    got = pp.rotate_nms.rotate_nms(np.zeros((n, 6), np.float32), 0.5, pre_max_size=100)
    assert np.array_equal(got, np.arange(100))
    # bit 63 of a mask word: the box at sorted position 0 suppresses exactly the one at position 63
    d = np.zeros((64, 6), np.float32)
    d[:, 0] = 5.0 * np.arange(64)
    d[:, 2:4] = 1.0
    d[:, 5] = 1.0 - np.arange(64) / 64.0
    d[63, 0] = 0.0
    assert np.array_equal(pp.rotate_nms.rotate_nms(d, 0.5), np.arange(63))


# ---------------------------------------------------------------- detector mode
def _tiny_cfg(pp, pre=100, post=50, rotate=False):
    cfg = pp.config.tiny_config(3)
    s = cfg["model"]["second"]
    s["nms_pre_max_size"], s["nms_post_max_size"] = pre, post
    if rotate:
        s["use_rotate_nms"] = True
    return cfg


def _head_maps(d, seed):
    """B = 3 frames of synthetic head maps: small box codes, distinct class logits, the last frame's mask all zero."""
    rng = np.random.default_rng(seed)
    B = 3
    box = (rng.standard_normal((B, d.head_h, d.head_w, 14)) * 0.3).astype(np.float32)
    ncl = B * d.head_h * d.head_w * 2
    cls = (rng.permutation(ncl).astype(np.float32) / ncl * 4.0 - 2.0).reshape(B, d.head_h, d.head_w, 2)
    dr = rng.standard_normal((B, d.head_h, d.head_w, 4)).astype(np.float32)
    mask = (rng.random((B, d.num_anchors)) < 0.6).astype(np.uint8)
    mask[2] = 0
    return box, cls, dr, mask


def _drawn_case(pp, d, anchors, nms_dict):
    """Head maps redrawn on the CPU until no pair's IoU in the helper lies within 1e-4 of the threshold."""
    rect, trv, _ = pp.synth.default_calib()
    rect, trv = np.stack([rect] * 3), np.stack([trv] * 3)
    for seed in range(4000, 6000):
        box, cls, dr, mask = _head_maps(d, seed)
        ex = (None, None, None, rect, trv, None, np.stack([anchors] * 3), mask, np.arange(3), None)
        margins = []
        ref = rr.predict_rotated(ex, {"box_preds": box, "cls_preds": cls, "dir_cls_preds": dr}, nms_dict, margins)
        if min(margins) > 1e-4:
            return (box, cls, dr, mask, rect, trv), ex, ref
    raise AssertionError("no draw keeps every IoU 1e-4 from the threshold")


def _assert_matches(dets, n, ref):
    for b in range(3):
        r = ref[b]
        k = len(r["anchor_index"])
        assert int(n[b]) == k, (b, int(n[b]), k)
        assert np.array_equal(dets[b]["anchor_index"][:k], r["anchor_index"]), b
        if k:
            np.testing.assert_allclose(dets[b]["score"][:k], r["scores"], rtol=0, atol=TOL)
            np.testing.assert_allclose(dets[b]["box3d_lidar"][:k], r["box3d_lidar"], rtol=0, atol=TOL)
            np.testing.assert_allclose(dets[b]["box3d_camera"][:k], r["box3d_camera"], rtol=0, atol=TOL)
            assert np.array_equal(dets[b]["label"][:k], r["label_preds"])


def _kept_bytes(dets, n):
    return [dets[b][:int(n[b])].tobytes() for b in range(len(n))]


@pytest.mark.parametrize("pre,post", [(100, 100), (60, 100), (100, 3)])
def test_detector_rotated_mode(pp, hip_lib, pre, post):
    """pre < K = 100 and post smaller than the number kept are the second and third case."""
    eng = pp.Engine(_tiny_cfg(pp, pre, post), max_batch=3, max_points_per_frame=4096)
    try:
        d = eng.d
        assert eng.nms_mode == "standup"
        inputs, ex, ref = _drawn_case(pp, d, eng.anchors, dict(d.nms_dict()))
        eng.set_nms_mode("rotated")
        assert eng.nms_mode == "rotated"
        dets, n = eng.predict(*inputs)
        print(f"pre {pre} post {post}: rotated kept {n.tolist()}")
        assert int(n[2]) == 0 and len(ref[2]["anchor_index"]) == 0          # all-zero anchor mask
        _assert_matches(dets, n, ref)
        if post == 3:
            assert n[:2].tolist() == [3, 3]
            free = rr.predict_rotated(ex, {"box_preds": inputs[0], "cls_preds": inputs[1], "dir_cls_preds": inputs[2]},
                                      dict(d.nms_dict(), nms_post_max_size=50))
            assert min(len(free[0]["anchor_index"]), len(free[1]["anchor_index"])) > 3, "the cap must bind"
        # the case discriminates: the stand-up rule keeps another set on the same input ...
        eng.set_nms_mode("standup")
        sdets, sn = eng.predict(*inputs)
        print(f"pre {pre} post {post}: stand-up kept {sn.tolist()}")
        assert any(sdets[b]["anchor_index"][:sn[b]].tolist() != dets[b]["anchor_index"][:n[b]].tolist() for b in range(2))
        sref = rn.predict(ex, {"box_preds": inputs[0], "cls_preds": inputs[1], "dir_cls_preds": inputs[2]}, d.nms_dict())
        assert [int(v) for v in sn] == [0 if r["scores"] is None else len(r["scores"]) for r in sref]
        # ... and is byte for byte what an engine that never left the default returns
        fresh = pp.Engine(_tiny_cfg(pp, pre, post), max_batch=3, max_points_per_frame=4096)
        try:
            fdets, fn = fresh.predict(*inputs)
        finally:
            fresh.close()
        assert np.array_equal(fn, sn) and _kept_bytes(fdets, fn) == _kept_bytes(sdets, sn)
        with pytest.raises(ValueError):
            eng.set_nms_mode("polygon")
        assert eng._lib.pp_set_nms_mode(eng._h, 7) == 1 and eng.nms_mode == "standup"       # PP_ERR_ARG
    finally:
        eng.close()


def test_config_key_equals_the_setter(pp, hip_lib):
    a = pp.Engine(_tiny_cfg(pp, rotate=True), max_batch=3, max_points_per_frame=4096)
    b = pp.Engine(_tiny_cfg(pp), max_batch=3, max_points_per_frame=4096)
    try:
        assert a.nms_mode == "rotated" and b.nms_mode == "standup"
        inputs, _, ref = _drawn_case(pp, a.d, a.anchors, dict(a.d.nms_dict()))
        b.set_nms_mode("rotated")
        adets, an = a.predict(*inputs)
        bdets, bn = b.predict(*inputs)
        _assert_matches(adets, an, ref)
        assert np.array_equal(an, bn) and _kept_bytes(adets, an) == _kept_bytes(bdets, bn)
    finally:
        a.close()
        b.close()
    net = pp.VoxelNet(_tiny_cfg(pp, rotate=True), max_batch=3, max_points_per_frame=4096)
    try:
        assert net.engine.nms_mode == "rotated"
    finally:
        net.engine.close()


def test_detect_rotated_keeps_no_overlapping_pair(pp, hip_lib):
    """Property of the fused path (a captured pass keyed on the rule) at the shipped config: among the boxes a frame
    returns, no pair's rotated IoU, taken by the C oracle on the returned boxes, exceeds the threshold by more than 1e-4."""
    cfg = pp.config.pedestrian_d435i_config(2)
    eng = pp.Engine(cfg, max_batch=2, max_points_per_frame=8192)
    try:
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
        frames = [pp.synth.d435i_cloud(900 + i, 4096) for i in range(2)]
        rect, trv, _ = pp.synth.default_calib()
        rect, trv = np.stack([rect] * 2), np.stack([trv] * 2)
        s0, sn0 = eng.detect(frames, rect, trv)
        s0, sn0 = s0.copy(), sn0.copy()
        eng.set_nms_mode("rotated")
        dets, n = eng.detect(frames, rect, trv)
        dets, n = dets.copy(), n.copy()
        print(f"detect: stand-up kept {sn0.tolist()}, rotated kept {n.tolist()}")
        thr = eng.d.nms_iou_threshold
        for b in range(2):
            k = int(n[b])
            assert k >= int(sn0[b]) and k > 0
            boxes = dets[b]["box3d_lidar"][:k][:, [0, 1, 3, 4, 6]].astype(np.float32)
            iou = c_oracle.rotate_iou_eval(boxes, boxes, -1)
            off = iou[~np.eye(k, dtype=bool)]
            assert not (off > thr + TOL).any(), (b, float(off.max()))
            assert (np.diff(dets[b]["score"][:k]) <= 0).all()
        eng.set_nms_mode("standup")
        s1, sn1 = eng.detect(frames, rect, trv)
        assert np.array_equal(sn0, sn1) and _kept_bytes(s0, sn0) == _kept_bytes(s1, sn1)
    finally:
        eng.close()
