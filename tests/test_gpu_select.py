"""The detector's top-100 selection (csrc/postprocess.hip) against the tie-defined reference (tests/postprocess_ref.py)
on inputs built to break it (tests/select_cases.py; tests/test_select_host.py checks the reference and every fixture
condition without a GPU).

The kernel has three selection paths: all candidates in LDS (at most CCAP = 12288), the re-scan that keeps the keys at or
above a floor taken from the first-stored CCAP, and the select that re-reads the head map in every pass when more than
CCAP keys survive the floor.  These tests assert the RESULT only.  Which path a case took on the GPU is not observed --
the library has no switch or counter for it, and none is added; it is inferred from the input (candidate count against
CCAP, and for the third path logits ascending with the anchor index over several multiples of CCAP).

First half: hand-built head maps through Engine.predict (the strided scan; `cls_plane_live` is false there).  Unless a
case says otherwise the setting is selection-transparent -- nms_iou_threshold 1.0, pre = post = 100 -- so the output rows
are the selected 100 in rank order.  Frame 0 carries the adversarial map, frame 1 a benign random one with another
mask, and both are compared.  Second half: the 16-anchors-per-thread scan of the compact class plane, reached through
the fused path at large batch with weights that make every logit its slot's bias.

Exact: n, anchor_index, label, dir_label.  score: rtol = atol = 1e-6; boxes: rtol = atol = 1e-5 (the tolerances of
test_predict_thresholds_and_caps)."""
import numpy as np
import pytest

import postprocess_ref as pr
import select_cases as sc

pytestmark = pytest.mark.gpu


def _compare(dets, n, ref, what):
    k = int(n)
    assert k == ref["n"], (what, k, ref["n"])
    assert np.array_equal(dets["anchor_index"][:k], ref["anchor_index"]), what
    assert np.array_equal(dets["label"][:k], ref["label"]), what
    assert np.array_equal(dets["dir_label"][:k], ref["dir_label"]), what
    np.testing.assert_allclose(dets["score"][:k], ref["score"], rtol=1e-6, atol=1e-6, err_msg=what)
    np.testing.assert_allclose(dets["box3d_lidar"][:k], ref["box3d_lidar"], rtol=1e-5, atol=1e-5, err_msg=what)
    np.testing.assert_allclose(dets["box3d_camera"][:k], ref["box3d_camera"], rtol=1e-5, atol=1e-5, err_msg=what)


@pytest.fixture(scope="module")
def engines(pp, hip_lib):
    """Batch-2 engines by (grid, num_class, NMS settings); Engine.predict needs no weights."""
    cache = {}

    def get(kind, ncls, nms):
        key = (kind, ncls, tuple(sorted(nms.items())))
        if key not in cache:
            cfg = sc.grid_g_config(2, ncls, **nms) if kind == "G" else sc.kitti_config(2, ncls, **nms)
            cache[key] = pp.Engine(cfg, max_batch=2, max_points_per_frame=4096)
        return cache[key]

    yield get
    for e in cache.values():
        e.close()


def _predict(eng, ex, preds):
    return eng.predict(preds["box_preds"], preds["cls_preds"], preds["dir_cls_preds"], ex[7], ex[3], ex[4])


def _run_case(eng, case, seed=0, **ref_kw):
    d = eng.d
    ex, preds = sc.batch(d, eng.anchors, case, seed)
    ref = pr.predict(ex, preds, d.nms_dict(), **ref_kw)
    dets, n = _predict(eng, ex, preds)
    return dets, n, ref


@pytest.mark.parametrize("name", list(sc.CASES_G))
def test_selection_on_grid_g(engines, name):
    """12800 anchors, the smallest grid above CCAP: candidate counts 0 / 1 / 99 / 100 / 101, one logit everywhere with
    12800, CCAP - 1, CCAP and CCAP + 1 candidates, ties across the cut (also with pre_max 30), keys that make every
    pass of the radix select decide (thin: the candidates fit the LDS; full: they do not), the score threshold at
    exactly 0.5, and two / three classes with tied class logits.  Which selection path ran is inferred, not observed."""
    ncls, nms, build = sc.CASES_G[name]
    eng = engines("G", ncls, nms)
    assert eng.d.num_anchors == 12800 and eng.nms_mode == "standup" and eng.class_nms == "joint"
    case = build(eng.d)
    dets, n, ref = _run_case(eng, case)
    assert np.array_equal(ref[0]["anchor_index"], case["top"]), "the reference selects what the construction wrote down"
    for b in range(2):
        _compare(dets[b], n[b], ref[b], f"{name} frame {b}")


@pytest.mark.parametrize("ncls", [2, 3])
def test_per_class_selection_with_ties(engines, ncls):
    """set_class_nms('per_class') on the tied class maps: ties inside each class plane and across its cut, and anchors
    selected under two labels; class 0's rows, then class 1's, ..."""
    _, nms, build = sc.CASES_G[f"classes_{ncls}"]
    eng = engines("G", ncls, nms)
    eng.set_class_nms("per_class")
    try:
        dets, n, ref = _run_case(eng, build(eng.d), class_nms="per_class")
        assert dets.shape[1] == ncls * 100 and ref[0]["n"] == ncls * 100
        for b in range(2):
            _compare(dets[b], n[b], ref[b], f"per_class {ncls} frame {b}")
    finally:
        eng.set_class_nms("joint")


@pytest.mark.parametrize("name", list(sc.CASES_K))
def test_selection_in_adversarial_order_on_cfg_k(engines, name):
    """107136 candidates: logits strictly ascending with the anchor index (the best are scanned last: the input of the
    select that re-reads the head map in every pass), strictly descending, a sawtooth of period 1000 and ascending
    plateaus of 1000 equal values.  Only the result is asserted; which path ran is inferred from the input."""
    ncls, nms, build = sc.CASES_K[name]
    eng = engines("K", ncls, nms)
    assert eng.d.num_anchors == 107136
    case = build(eng.d)
    dets, n, ref = _run_case(eng, case)
    assert np.array_equal(ref[0]["anchor_index"], case["top"])
    for b in range(2):
        _compare(dets[b], n[b], ref[b], f"{name} frame {b}")


@pytest.mark.parametrize("rule", sc.RULES)
@pytest.mark.parametrize("map_name", list(sc.RULE_MAPS_K))
def test_rules_under_the_config_thresholds_on_cfg_k(engines, map_name, rule):
    """iou 0.5, pre 100, post 50 with the stand-up, rotated and soft rules after a pass whose candidates did not fit the
    LDS (the rotated rule's polygon scratch lies on the candidate keys).  The decision margins of the reference are
    above 1e-4 (the project's north_star tolerance, far above float32 decode noise): asserted here and on the host."""
    build, seed = sc.RULE_MAPS_K[map_name]
    eng = engines("K", 1, {})
    d = eng.d
    assert (d.nms_iou_threshold, d.nms_pre_max_size, d.nms_post_max_size) == (0.5, 100, 50)
    eng.set_nms_mode(rule)
    try:
        soft = eng.soft_nms
        assert (soft["method"], soft["sigma"], np.float32(soft["score_floor"])) == ("gaussian", 0.5, np.float32(0.001))
        dets, n, ref = _run_case(eng, build(d), seed, rule=rule)
        for b in range(2):
            assert ref[b]["iou_margin"] > sc.MARGIN and ref[b]["floor_margin"] > sc.MARGIN
            _compare(dets[b], n[b], ref[b], f"{map_name} {rule} frame {b}")
    finally:
        eng.set_nms_mode("standup")


# ---------------------------------------------------------------------------------------------- the compact-plane scan
def _uniform_deconv3(tags):
    return any(t.endswith(":deconv3") and t.startswith(("k_deconv_r", "k_deconv_u")) for t in tags)


def _fused_check(pp, eng, frames, cls_bias, pick):
    """One fused pass with the all-zero kernels and the given biases; every frame's detections against the tie rule on
    the engine's own anchor mask, the frames `pick(mask sizes)` names also against the whole reference.  Returns the
    mask sizes."""
    d = eng.d
    B = len(frames)
    k = d.num_anchor_per_loc
    bias = np.asarray(cls_bias, np.float32)
    eng.load_weights(sc.zero_weights(d, bias, sc.DIR_BIAS))
    rect, trv, _ = pp.synth.default_calib()
    rects, trvs = np.stack([rect] * B), np.stack([trv] * B)
    dets, n = eng.detect(frames, rects, trvs, on_numeric="raise")
    assert _uniform_deconv3(eng.layer_tags()), eng.layer_tags()
    im = eng.intermediates()
    # every logit is its slot's bias, exactly; the boxes are the anchors
    assert np.array_equal(im["cls_preds"], np.broadcast_to(bias.reshape(-1), im["cls_preds"].shape))
    assert np.array_equal(im["dir_cls_preds"], np.broadcast_to(np.asarray(sc.DIR_BIAS, np.float32).reshape(-1),
                                                               im["dir_cls_preds"].shape))
    assert not im["box_preds"].any()
    mask = im["anchors_mask"]
    sizes = (mask == 1).sum(axis=1)
    dir_of_slot = np.argmax(np.asarray(sc.DIR_BIAS), axis=1)
    for b in range(B):
        top, lab = sc.fused_expected(mask[b], bias)
        kk = int(n[b])
        assert kk == len(top) == min(int(sizes[b]), sc.KTOP), (b, kk, len(top))
        assert np.array_equal(dets[b]["anchor_index"][:kk], top), b
        assert np.array_equal(dets[b]["label"][:kk], lab), b
        assert np.array_equal(dets[b]["dir_label"][:kk], dir_of_slot[top % k]), b
    sel = list(pick(sizes))
    ex = (None, None, None, rects[sel], trvs[sel], None, np.stack([eng.anchors] * len(sel)), mask[sel], np.arange(len(sel)),
          None)
    preds = {key: im[key][sel] for key in ("box_preds", "cls_preds", "dir_cls_preds")}
    ref = pr.predict(ex, preds, d.nms_dict())
    for i, b in enumerate(sel):
        _compare(dets[b], n[b], ref[i], f"frame {b}")
    return sizes


@pytest.fixture(scope="module")
def fused_k(pp, hip_lib):
    cfg = sc.kitti_config(32, 2, **sc.TRANSPARENT)
    eng = pp.Engine(cfg, max_batch=32, max_points_per_frame=20000)
    frames = sc.uniform_frames(eng.d, sc.FUSED_K_POINTS)
    yield eng, frames
    eng.close()


@pytest.mark.parametrize("setting", list(sc.BIASES_K))
def test_compact_plane_scan_on_cfg_k_batch32(pp, fused_k, setting):
    """cfg-K, two classes, B = 32 (the fixture of test_kitti_shaped_batch32_two_classes): deconv3 is a uniform deconv
    kernel, so the post-process scans the compact class plane, 16 anchors per thread.  All kernels zero, the class
    biases the only signal: the expected anchors follow from the anchor mask and the tie rule alone -- the 100
    lowest-index masked anchors of the slot with the largest bias, then the next slot's; labels by first maximum.  At
    least one frame has more than CCAP masked anchors (the re-scan), one is empty, one has fewer than 100 masked anchors."""
    eng, frames = fused_k
    assert (eng.d.num_class, eng.d.num_anchor_per_loc, eng.d.num_anchors % 16) == (2, 2, 0)
    # the whole reference on the frames that differ in kind: the densest, the empty one, the sparse one, the last
    sizes = _fused_check(pp, eng, frames, sc.BIASES_K[setting], lambda sz: (int(np.argmax(sz)), 3, 9, 31))
    assert sizes.max() > sc.CCAP and sizes[3] == 0 and 0 < sizes[9] < sc.KTOP, sizes


def test_compact_plane_scan_on_cfg_a_batch64(pp, hip_lib):
    """cfg-A at B = 64, one bias everywhere: 10240 anchors, below CCAP and divisible by 16 -- the same scan with the
    candidates staying in LDS."""
    cfg = sc._nms(pp.config.pedestrian_d435i_config(64), sc.TRANSPARENT)
    eng = pp.Engine(cfg, max_batch=64, max_points_per_frame=16384)
    try:
        assert eng.d.num_anchors == 10240 < sc.CCAP and eng.d.num_anchors % 16 == 0
        frames = sc.uniform_frames(eng.d, sc.FUSED_A_POINTS, seed=71)
        sizes = _fused_check(pp, eng, frames, [[0.25], [0.25]], lambda sz: (0, 5, 10, 63))
        assert sc.KTOP < sizes.max() <= sc.CCAP and sizes[5] == 0 and 0 < sizes[10] < sc.KTOP, sizes
    finally:
        eng.close()
