"""The tie-defined reference of the post-process (tests/postprocess_ref.py) is the right referee, and the inputs of
tests/test_gpu_select.py are what they claim to be -- all without a GPU.

  * on inputs free of score ties the reference equals oracle.ref_numpy.predict exactly;
  * on tied inputs its selection is a valid refinement of the oracle's: the same multiset of float32 scores as
    np.sort(scores)[-100:], in non-increasing order;
  * the constants the GPU tests are built around are the ones in csrc/postprocess.hip;
  * every fixture condition of the GPU cases (candidate counts around CCAP, the expected anchors written down from the
    construction, threshold gaps, decision margins of the NMS rules, the mask sizes of the fused-path frames).
"""
import os
import re

import numpy as np
import pytest

from oracle import ref_numpy as rn
import postprocess_ref as pr
import select_cases as sc
import util_ref


def _source():
    pkg = os.path.dirname(os.path.abspath(sc.pp.__file__))
    with open(os.path.join(pkg, "csrc", "postprocess.hip")) as f:
        return f.read()


def test_constants_in_step_with_the_kernel():
    src = _source()
    ccap = int(re.search(r"^#define\s+CCAP\s+(\d+)", src, re.M).group(1))
    kmax = int(re.search(r"^#define\s+KMAX\s+(\d+)", src, re.M).group(1))
    ktop = int(re.search(r"^\s*const\s+int\s+KTOP\s*=\s*(\d+)\s*;", src, re.M).group(1))
    assert (ccap, kmax, ktop) == (12288, 128, 100)
    assert (sc.CCAP, sc.KMAX, sc.KTOP, pr.KTOP) == (ccap, kmax, ktop, ktop)
    d, _ = sc.derived(sc.grid_g_config())
    assert d.num_anchors == 12800 > ccap >= sc.derived(sc.pp.config.pedestrian_d435i_config(1))[0].num_anchors
    dk, _ = sc.derived(sc.kitti_config())
    assert dk.num_anchors == 107136 > 8 * ccap


# ---------------------------------------------------------------------------------- agreement with the oracle
def _assert_equals_oracle(ref, got):
    if ref["scores"] is None:
        assert got["n"] == 0
        return
    assert got["n"] == len(ref["scores"])
    assert np.array_equal(got["label"], ref["label_preds"])
    assert np.array_equal(got["score"], ref["scores"]) and got["score"].dtype == ref["scores"].dtype
    assert np.array_equal(got["box3d_lidar"], ref["box3d_lidar"]) and got["box3d_lidar"].dtype == np.float32
    assert np.array_equal(got["box3d_camera"], ref["box3d_camera"]) and got["box3d_camera"].dtype == np.float64


@pytest.mark.parametrize("score_thr,pre_max,post_max", [(0.55, 100, 50), (0.0, 30, 7), (0.3, 1000, 5)])
def test_equals_the_oracle_on_the_seeds_of_test_predict_thresholds_and_caps(pp, score_thr, pre_max, post_max):
    cfg = pp.config.pedestrian_d435i_config(1)
    s = cfg["model"]["second"]
    s["nms_score_threshold"], s["nms_pre_max_size"], s["nms_post_max_size"] = score_thr, pre_max, post_max
    d, anchors = sc.derived(cfg)
    rng = np.random.default_rng(int(score_thr * 100) + pre_max)
    box = (rng.standard_normal((1, d.head_h, d.head_w, 14)) * 0.3).astype(np.float32)
    cls = (rng.standard_normal((1, d.head_h, d.head_w, 2)) * 0.8).astype(np.float32)
    dr = rng.standard_normal((1, d.head_h, d.head_w, 4)).astype(np.float32)
    mask = (rng.random((1, d.num_anchors)) < 0.6).astype(np.uint8)
    rect, trv, _ = pp.synth.default_calib()
    ex = (None, None, None, rect[None], trv[None], None, anchors[None], mask, np.array([0]), None)
    preds = {"box_preds": box, "cls_preds": cls, "dir_cls_preds": dr}
    top = np.sort(pr.sigmoid32(cls.reshape(-1))[mask[0] == 1])[-(sc.KTOP + 1):]
    assert len(np.unique(top)) == len(top), "the seed must be free of score ties where the selection looks"
    ref = rn.predict(ex, preds, d.nms_dict())[0]
    got = pr.predict(ex, preds, d.nms_dict())[0]
    assert ref["scores"] is not None and 0 < len(ref["scores"]) <= post_max
    _assert_equals_oracle(ref, got)


def test_equals_the_oracle_on_the_seed_of_test_multi_class_score_and_label_rule(pp):
    cfg = pp.config.pedestrian_d435i_config(1)
    cfg["model"]["second"]["num_class"] = 3
    cfg["model"]["second"]["nms_score_threshold"] = 0.3
    d, anchors = sc.derived(cfg)
    rng = np.random.default_rng(5)
    box = (rng.standard_normal((1, d.head_h, d.head_w, 14)) * 0.3).astype(np.float32)
    cls = (rng.standard_normal((1, d.head_h, d.head_w, 6)) * 0.8).astype(np.float32)
    dr = rng.standard_normal((1, d.head_h, d.head_w, 4)).astype(np.float32)
    mask = (rng.random((1, d.num_anchors)) < 0.5).astype(np.uint8)
    rect, trv, _ = pp.synth.default_calib()
    ex = (None, None, None, rect[None], trv[None], None, anchors[None], mask, np.array([0]), None)
    preds = {"box_preds": box, "cls_preds": cls, "dir_cls_preds": dr}
    top = np.sort(pr.sigmoid32(cls.reshape(-1, 3)).max(axis=-1)[mask[0] == 1])[-(sc.KTOP + 1):]
    assert len(np.unique(top)) == len(top)
    ref = rn.predict(ex, preds, d.nms_dict())[0]
    got = pr.predict(ex, preds, d.nms_dict())[0]
    assert len(set(ref["label_preds"].tolist())) == 3
    _assert_equals_oracle(ref, got)


def test_candidate_order_is_the_documented_rule():
    tiny = np.array(1, np.uint32).view(np.float32)
    #                 0     1     2    3     4     5      6     7    8     9
    lg = np.array([-0.0, 0.0, 1.0, 0.0, -0.0, tiny, -tiny, 1.0, 5.0, -1.0], np.float32)
    mask = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0, 1], np.uint8)
    assert pr.candidate_order(lg, mask, 0.0).tolist() == [2, 7, 5, 1, 3, 0, 4, 6, 9]
    assert pr.candidate_order(lg, mask, 0.5).tolist() == [2, 7, 5, 1, 3, 0, 4, 6]      # every one of them scores 0.5
    m, lab = pr.joint_logit(np.array([[1.0, 1.0, 0.5], [0.0, 2.0, 2.0], [3.0, 1.0, 3.0]], np.float32))
    assert m.tolist() == [1.0, 2.0, 3.0] and lab.tolist() == [0, 1, 0]


# ---------------------------------------------------------------------------------- the GPU cases, checked on the host
_grids = {}


def _grid(kind, ncls, nms):
    key = (kind, ncls, tuple(sorted(nms.items())))
    if key not in _grids:
        cfg = sc.grid_g_config(2, ncls, **nms) if kind == "G" else sc.kitti_config(2, ncls, **nms)
        _grids[key] = sc.derived(cfg)
    return _grids[key]


def _refinement(case_logit, mask, thr, top_anchors, ncls):
    """The selected scores are np.sort(scores)[-100:] as a multiset, in non-increasing order."""
    lg, _ = pr.joint_logit(case_logit.reshape(-1, ncls))
    s = pr.sigmoid32(lg)
    cand = s[mask == 1]
    if thr > 0:
        cand = cand[cand >= thr]
    want = np.sort(cand)[-sc.KTOP:]
    got = s[top_anchors]
    assert np.array_equal(np.sort(got), want)
    assert (np.diff(got) <= 0).all()


@pytest.mark.parametrize("name", list(sc.CASES_G) + ["K_" + k for k in sc.CASES_K])
def test_case_fixture_and_refinement(name):
    kind = "K" if name.startswith("K_") else "G"
    ncls, nms, build = sc.CASES_K[name[2:]] if kind == "K" else sc.CASES_G[name]
    d, anchors = _grid(kind, ncls, nms)
    case = build(d)
    cfg = d.nms_dict()
    thr = cfg["nms_score_threshold"]
    ex, preds = sc.batch(d, anchors, case)
    out = pr.predict(ex, preds, cfg)
    # frame 0: the construction's own expectation is what the reference selects, and all of it comes out
    lg, _ = pr.joint_logit(case["logit"])
    cand = pr.candidate_order(lg, case["mask"], thr)
    assert len(cand) == case["ncand"]
    pre = cfg["nms_pre_max_size"]
    assert np.array_equal(out[0]["top"][:pre], case["top"])
    assert np.array_equal(out[0]["anchor_index"], case["top"]), "selection-transparent: the rows are the selection"
    assert out[0]["n"] == min(case["ncand"], sc.KTOP, pre)
    if "label" in case:
        assert np.array_equal(out[0]["label"], case["label"][case["top"]])
        assert len(set(out[0]["label"].tolist())) == ncls
    for b in range(2):
        _refinement(preds["cls_preds"][b], ex[7][b], thr, out[b]["top"], ncls)
    assert out[1]["n"] == min(sc.KTOP, pre) and not np.array_equal(ex[7][0], ex[7][1])
    # the conditions the case names
    if name.startswith("all_equal"):
        assert case["ncand"] == int(name.split("_")[-1]) and len(np.unique(case["logit"])) == 1
        assert case["top"].tolist() == np.nonzero(case["mask"])[0][:100].tolist()
        if case["ncand"] == d.num_anchors:
            assert case["top"].tolist() == list(range(100))
    if name.endswith("_full") or name.startswith("ties") or kind == "K":
        assert case["ncand"] == d.num_anchors > sc.CCAP
    if name.endswith("_thin"):
        assert sc.KTOP < case["ncand"] <= sc.CCAP
    if name.startswith("threshold_edge"):
        s = pr.sigmoid32(case["logit"][:, 0])
        assert (s[case["edge"]] == np.float32(0.5)).all() and set(case["edge"]) <= set(cand)
        others = np.delete(s, case["edge"])
        assert np.abs(others.astype(np.float64) - 0.5).min() > 1e-5, "no other score near the threshold"
        assert (case["ncand"] < sc.KTOP) == name.endswith("few")
    if name.startswith("K_"):
        assert case["ncand"] > 8 * sc.CCAP


@pytest.mark.parametrize("ncls", [2, 3])
def test_per_class_fixture(ncls):
    _, nms, build = sc.CASES_G[f"classes_{ncls}"]
    d, anchors = _grid("G", ncls, nms)
    case = build(d)
    ex, preds = sc.batch(d, anchors, case)
    out = pr.predict(ex, preds, d.nms_dict(), class_nms="per_class")[0]
    assert out["n"] == ncls * sc.KTOP
    for c in range(ncls):
        plane = case["logit"][:, c]
        top = out["top"][c]
        assert (out["label"][c * 100:(c + 1) * 100] == c).all()
        assert np.array_equal(out["anchor_index"][c * 100:(c + 1) * 100], top)
        # ties inside the class plane, and across its cut: the last selected value goes on below the cut
        assert len(np.unique(plane[top])) < len(top)
        assert (plane == plane[top[-1]]).sum() > (plane[top] == plane[top[-1]]).sum()
        expect = np.lexsort((np.arange(len(plane)), -plane.astype(np.float64)))[:100]
        assert np.array_equal(top, expect)
    assert len(set(out["top"][0]) & set(out["top"][1])) > 0, "an anchor selected under two labels"


@pytest.mark.parametrize("rule", sc.RULES)
@pytest.mark.parametrize("map_name", list(sc.RULE_MAPS_K))
def test_rule_fixture_margins(map_name, rule):
    build, seed = sc.RULE_MAPS_K[map_name]
    d, anchors = _grid("K", 1, {})
    cfg = d.nms_dict()
    assert (cfg["nms_iou_threshold"], cfg["nms_pre_max_size"], cfg["nms_post_max_size"]) == (0.5, 100, 50)
    case = build(d)
    ex, preds = sc.batch(d, anchors, case, seed)
    out = pr.predict(ex, preds, cfg, rule=rule)        # soft: the engine's defaults (gaussian, 0.5, 0.001)
    for b in range(2):
        assert out[b]["iou_margin"] > sc.MARGIN and out[b]["floor_margin"] > sc.MARGIN, (b, out[b]["iou_margin"],
                                                                                          out[b]["floor_margin"])
        assert 0 < out[b]["n"] <= 50
    assert np.array_equal(out[0]["top"], case["top"])
    if map_name == "plateaus" and rule != "soft":
        assert not np.array_equal(out[0]["anchor_index"], case["top"][:out[0]["n"]]), "the suppression has work to do"


# ---------------------------------------------------------------------------------- the fused-path fixtures
def test_fused_frames_exceed_the_lds_capacity(pp):
    d, _ = sc.derived(sc.kitti_config(32, 2, **sc.TRANSPARENT))
    frames = sc.uniform_frames(d, sc.FUSED_K_POINTS)
    fr = util_ref.oracle_frames(d, frames)
    counts = np.array([int(f["anchors_mask"].sum()) for f in fr])
    assert counts.max() > sc.CCAP and counts[3] == 0 and 0 < counts[9] < sc.KTOP
    assert d.num_anchors % 16 == 0 and d.num_class == 2
    da, _ = sc.derived(sc.pp.config.pedestrian_d435i_config(64))
    assert da.num_anchors == 10240 < sc.CCAP and da.num_anchors % 16 == 0
    fa = util_ref.oracle_frames(da, sc.uniform_frames(da, sc.FUSED_A_POINTS[:11], seed=71))
    ca = [int(f["anchors_mask"].sum()) for f in fa]
    assert sc.KTOP < max(ca) <= sc.CCAP and ca[5] == 0 and 0 < ca[10] < sc.KTOP
    w = sc.zero_weights(d, sc.BIASES_K["slot1_above"], sc.DIR_BIAS)
    pp.weights.check_weights(d, w)
    nonzero = [k for k, v in w.items() if np.any(v != 0) and not (k.endswith("gamma") or k.endswith("moving_variance"))]
    assert sorted(nonzero) == ["rpn/conv_cls/bias", "rpn/conv_dir_cls/bias"]
    # the expectation of the GPU test, on one oracle mask: slot 1's anchors first
    top, lab = sc.fused_expected(fr[0]["anchors_mask"], sc.BIASES_K["slot1_above"])
    assert (top % 2 == 1).all() and (np.diff(top) > 0).all() and (lab == 0).all()
    top, lab = sc.fused_expected(fr[0]["anchors_mask"], sc.BIASES_K["class1_above"])
    assert top.tolist() == np.nonzero(fr[0]["anchors_mask"])[0][:100].tolist() and (lab == 1).all()
