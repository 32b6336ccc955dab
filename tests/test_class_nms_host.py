"""Per-class suppression (model.second.use_multi_class_nms), the parts that need no GPU: the C-ABI's declarations, the
binding's symbol list, the config key, and the properties of the host oracle tests/class_nms_ref.py."""
import copy
import os
import re

import numpy as np
import pytest

from oracle import ref_numpy as rn
import class_nms_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pp_set_class_nms", "pp_get_class_nms", "pp_get_detection_rows")


def test_header_declares_the_class_nms_surface():
    with open(os.path.join(ROOT, "include", "pp_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+PP_ABI_VERSION\s+4\b", h)
    assert re.search(r"enum\s+pp_class_nms\s*\{[^}]*PP_CLASS_NMS_JOINT\s*=\s*0\b[^}]*PP_CLASS_NMS_PER_CLASS\s*=\s*1\b[^}]*\}", h, re.S)
    assert re.search(r"int\s+pp_set_class_nms\s*\(\s*pp_handle\s+h\s*,\s*int32_t\s+mode\s*\)", h)
    assert re.search(r"int\s+pp_get_class_nms\s*\(\s*pp_handle\s+h\s*,\s*int32_t\s*\*\s*mode\s*\)", h)
    assert re.search(r"int\s+pp_get_detection_rows\s*\(\s*pp_handle\s+h\s*,\s*int32_t\s*\*\s*rows\s*\)", h)
    added = h[h.index("later additions within 4"):h.index("#define PP_ABI_VERSION")]
    for name in ("pp_class_nms",) + NEW:
        assert name in added
    assert added.index("pp_box3d_to_bbox") < added.index("pp_class_nms")           # appended, nothing before them changed
    cfg = h[h.index("typedef struct pp_config"):h.index("} pp_config;")]
    assert "class_nms" not in cfg                                                  # pp_config did not change


def test_binding_lists_the_symbols(pp):
    for name in NEW:
        assert name in pp._lib.EXPORTS
    assert pp._lib.EXPORTS.index("pp_box3d_to_bbox") < pp._lib.EXPORTS.index("pp_set_class_nms")
    assert "api_class_nms.hip" in pp._lib.SOURCES
    assert (pp._lib.PP_CLASS_NMS_JOINT, pp._lib.PP_CLASS_NMS_PER_CLASS) == (0, 1)
    for name in ("set_class_nms", "class_nms", "detection_rows"):
        assert hasattr(pp.Engine, name)


def test_config_key(pp):
    # off unless asked for: the shipped config carries the reference's `use_multi_class_nms: false`
    for cfg in (pp.config.pedestrian_d435i_config(1), pp.config.kitti_shaped_config(num_class=2), pp.config.tiny_config(1)):
        assert not cfg["model"]["second"].get("use_multi_class_nms", False)
        d = pp.config.Derived(cfg)
        assert d.use_multi_class_nms is False and d.nms_dict()["use_multi_class_nms"] is False
    two = pp.config.kitti_shaped_config(num_class=2)
    two["model"]["second"]["use_multi_class_nms"] = True
    d2 = pp.config.Derived(two)
    assert d2.use_multi_class_nms is True and d2.nms_dict()["use_multi_class_nms"] is True and d2.num_class == 2
    three = pp.config.pedestrian_d435i_config(1)
    three["model"]["second"].update(num_class=3, use_multi_class_nms=True)
    assert pp.config.Derived(three).use_multi_class_nms is True
    one = pp.config.pedestrian_d435i_config(1)
    one["model"]["second"]["use_multi_class_nms"] = True
    with pytest.raises(NotImplementedError, match="already is the per-class pass"):
        pp.config.Derived(one)
    bg = copy.deepcopy(two)
    bg["model"]["second"]["encode_background_as_zeros"] = False
    with pytest.raises(NotImplementedError):
        pp.config.Derived(bg)


def _case(pp, ncls, thr, seed=3, B=2):
    cfg = pp.config.tiny_config(B)
    cfg["model"]["second"].update(num_class=ncls, nms_score_threshold=thr, use_multi_class_nms=ncls > 1)
    d = pp.config.Derived(cfg)
    assert d.nms_dict()["use_multi_class_nms"] is (ncls > 1)
    A, napl = d.num_anchors, d.num_anchor_per_loc
    rng = np.random.default_rng(seed)
    logits = np.stack([np.stack([rng.permutation(np.linspace(-4, 4, A)) + 1e-4 * c for c in range(ncls)], axis=-1)
                       for _ in range(B)]).astype(np.float32)
    preds = {"box_preds": (0.3 * rng.standard_normal((B, d.head_h, d.head_w, napl * 7))).astype(np.float32),
             "cls_preds": logits.reshape(B, d.head_h, d.head_w, napl * ncls),
             "dir_cls_preds": rng.standard_normal((B, d.head_h, d.head_w, napl * 2)).astype(np.float32)}
    mask = (rng.random((B, A)) < 0.7).astype(np.uint8)
    rect, trv, _ = pp.synth.default_calib()
    anchors = pp.engine.build_anchors(d)
    ex = (None, None, None, np.stack([rect] * B), np.stack([trv] * B), None, np.stack([anchors] * B), mask, np.arange(B), None)
    return d, ex, preds, mask


@pytest.mark.parametrize("ncls,thr", [(2, 0.0), (3, 0.3)])
def test_oracle_groups_by_class_and_sorts_within(pp, ncls, thr):
    d, ex, preds, mask = _case(pp, ncls, thr)
    assert cr.distinct_top_scores(preds, mask, ncls)
    ref = cr.predict_per_class(ex, preds, d.nms_dict())
    logits = cr.class_logits(preds, ncls)
    for b, fr in enumerate(ref):
        n = len(fr["scores"])
        assert n == fr["class_counts"].sum() and (fr["class_counts"] <= d.nms_post_max_size).all() and n > ncls
        assert (np.diff(fr["label_preds"]) >= 0).all()                              # grouped by class, classes ascending
        at = 0
        for c, k in enumerate(fr["class_counts"]):
            seg = slice(at, at + k)
            assert (fr["label_preds"][seg] == c).all()
            assert (np.diff(fr["scores"][seg]) < 0).all()                           # descending within a class
            a = fr["anchor_index"][seg]
            assert (mask[b][a] == 1).all()
            assert np.array_equal(rn.sigmoid_array(logits[b, a, c]), fr["scores"][seg])   # the class's own score
            if thr > 0:
                assert (fr["scores"][seg] >= thr).all()
            at += k
        assert fr["box3d_lidar"].shape == (n, 7) and fr["box3d_camera"].shape == (n, 7)


def test_oracle_with_one_class_is_the_single_pass(pp):
    d, ex, preds, mask = _case(pp, 1, 0.3)
    ref = cr.predict_per_class(ex, preds, d.nms_dict())
    one = rn.predict(ex, preds, d.nms_dict())
    for fr, r in zip(ref, one):
        assert len(fr["scores"]) == len(r["scores"]) > 0
        assert np.array_equal(fr["scores"], r["scores"]) and np.array_equal(fr["box3d_lidar"], r["box3d_lidar"])
        assert np.array_equal(fr["box3d_camera"], r["box3d_camera"]) and np.array_equal(fr["label_preds"], r["label_preds"])


def test_anno_takes_more_rows_than_the_joint_cap(pp):
    """A per-class frame has up to num_class * nms_post_max_size rows: VoxelNet._to_dict and predict_kitti_to_anno pass
    them all through and name each by its label."""
    cfg = pp.config.kitti_shaped_config(num_class=2)
    cfg["model"]["second"].update(use_multi_class_nms=True, nms_post_max_size=4)
    d = pp.config.Derived(cfg)
    assert d.use_multi_class_nms
    post, ncls = d.nms_post_max_size, d.num_class
    n = ncls * post - 1
    dets = np.zeros((ncls * post,), dtype=pp.Engine.det_dtype())
    dets["score"][:n] = np.concatenate([np.linspace(0.9, 0.6, post), np.linspace(0.8, 0.5, post - 1)])
    dets["label"][:n] = [0] * post + [1] * (post - 1)
    dets["box3d_camera"][:n] = np.arange(n * 7, dtype=np.float64).reshape(n, 7) * 0.01 + 1.0
    dets["box3d_lidar"][:n] = dets["box3d_camera"][:n]
    p = pp.VoxelNet._to_dict(dets, n, 7)
    assert len(p["scores"]) == n > post and p["bbox"].shape == (n, 4)
    ex = [None] * 10
    ex[9] = np.array([[375, 1242]])
    anno = pp.anno.predict_kitti_to_anno(ex, ["Pedestrian", "Cyclist"], [p])[0]
    assert list(anno["name"]) == ["Pedestrian"] * post + ["Cyclist"] * (post - 1)
    assert np.allclose(anno["score"], dets["score"][:n])
