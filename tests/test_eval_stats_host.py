"""AP-evaluator statistics, host side: the packing the GPU path takes, the host
`compute_statistics` against the reference's compute_statistics_jit / fused_compute_statistics
(tests/golden/ref_eval_stats.npz, tools/gen_golden_evalstats.py), and the C-ABI's declarations.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden


def fixture_frames(g):
    """The fixture's flat arrays as the per-frame lists eval_class_v3 works on."""
    nd, ng, nc = g["num_dt"], g["num_gt"], g["num_dc"]
    d0 = np.concatenate([[0], np.cumsum(nd)])
    g0 = np.concatenate([[0], np.cumsum(ng)])
    c0 = np.concatenate([[0], np.cumsum(nc)])
    o0 = np.concatenate([[0], np.cumsum(nd * ng)])
    fr = {"overlaps": [], "gt": [], "dt": [], "ign_gt": [], "ign_dt": [], "dc": []}
    for i in range(len(nd)):
        fr["overlaps"].append(g["overlaps"][o0[i]:o0[i + 1]].reshape(nd[i], ng[i]))
        fr["gt"].append(g["gt_datas"][g0[i]:g0[i + 1]])
        fr["dt"].append(g["dt_datas"][d0[i]:d0[i + 1]])
        fr["ign_gt"].append(g["ignored_gt"][g0[i]:g0[i + 1]])
        fr["ign_dt"].append(g["ignored_det"][d0[i]:d0[i + 1]])
        fr["dc"].append(g["dc_bboxes"][c0[i]:c0[i + 1]])
    return fr


def test_fixture_covers_the_rules():
    g = load_golden("ref_eval_stats.npz")
    assert {0, 1, 63, 64, 65, 130} <= set(g["num_dt"].tolist())
    assert {0, 1, 40} <= set(g["num_gt"].tolist())
    assert set(np.unique(g["overlaps"]).tolist()) <= {0.0, 0.3, 0.5, 0.55, 0.7, 0.9}
    assert set(g["min_overlaps"].tolist()) == {0.5, 0.7} and (g["overlaps"] == 0.5).any() and (g["overlaps"] == 0.7).any()
    scores = g["dt_datas"][:, 5]
    assert (scores == -10000000.0).sum() == 1 and set(g["thresholds"].tolist()) <= set(scores.tolist())
    assert set(g["ignored_gt"].tolist()) == {-1, 0, 1} == set(g["ignored_det"].tolist())
    assert g["num_dc"].sum() > 0 and (g["num_dt"][g["num_gt"] == 0] > 0).any()
    assert sorted(zip(g["case_metric"].tolist(), g["case_aos"].tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    # DontCare boxes change the metric-0 false positives; some items have nothing to divide by (similarity -1)
    assert (g["stats"][0, ..., 1] < g["stats"][2, ..., 1]).any() and (g["stats"][1, ..., 3] == -1).any()


def test_host_compute_statistics_matches_reference(pp):
    g = load_golden("ref_eval_stats.npz")
    fr = fixture_frames(g)
    ke = pp.kitti_eval
    total = np.zeros_like(g["fused"])
    for f in range(len(fr["gt"])):
        args = (fr["overlaps"][f], fr["gt"][f], fr["dt"][f], fr["ign_gt"][f], fr["ign_dt"][f], fr["dc"][f])
        for k, mo in enumerate(g["min_overlaps"]):
            for metric in (0, 1):
                sc = ke.compute_statistics(*args, metric, mo, 0.0, False)[4]
                assert np.array_equal(sc, g["tp_scores"][f, k, :g["tp_count"][f, k]]), (f, k)
            for c, (metric, aos) in enumerate(zip(g["case_metric"], g["case_aos"])):
                for t, th in enumerate(g["thresholds"]):
                    tp, fp, fn, sim, _ = ke.compute_statistics(*args, int(metric), mo, th, True, bool(aos))
                    assert (tp, fp, fn, float(sim)) == tuple(g["stats"][c, f, k, t]), (f, k, c, t)
                    total[c, k, t] += (tp, fp, fn, sim if sim != -1 else 0.0)
    assert np.array_equal(total[..., :3], g["fused"][..., :3])
    np.testing.assert_allclose(total[..., 3], g["fused"][..., 3], rtol=0, atol=1e-12)


def test_pack_frames_round_trips(pp):
    g = load_golden("ref_eval_stats.npz")
    fr = fixture_frames(g)
    p = pp.kitti_eval.pack_frames(fr["overlaps"], fr["gt"], fr["dt"], fr["ign_gt"], fr["ign_dt"], fr["dc"])
    n = len(fr["gt"])
    assert p["nframes"] == n
    for key, counts in (("gt_off", g["num_gt"]), ("dt_off", g["num_dt"]), ("dc_off", g["num_dc"]),
                        ("ov_off", g["num_gt"] * g["num_dt"])):
        assert p[key].shape == (n + 1,) and p[key][0] == 0 and np.array_equal(np.diff(p[key]), counts), key
    assert p["ov_off"].dtype == np.int64 and p["gt_off"].dtype == p["dt_off"].dtype == p["dc_off"].dtype == np.int32
    assert p["ign_gt"].dtype == p["ign_dt"].dtype == np.int32 and p["overlaps"].dtype == np.float64
    for key in ("overlaps", "scores", "dt_alphas", "dt_boxes", "gt_alphas", "ign_gt", "ign_dt", "dc_boxes"):
        assert p[key].flags["C_CONTIGUOUS"], key
    for f in range(n):
        G, D = int(g["num_gt"][f]), int(g["num_dt"][f])
        block = p["overlaps"][p["ov_off"][f]:p["ov_off"][f + 1]].reshape(G, D)       # ground-truth major
        assert np.array_equal(block, fr["overlaps"][f].T)
        d = slice(p["dt_off"][f], p["dt_off"][f + 1])
        gs = slice(p["gt_off"][f], p["gt_off"][f + 1])
        assert np.array_equal(p["scores"][d], fr["dt"][f][:, 5]) and np.array_equal(p["dt_alphas"][d], fr["dt"][f][:, 4])
        assert np.array_equal(p["dt_boxes"][d], fr["dt"][f][:, :4]) and np.array_equal(p["gt_alphas"][gs], fr["gt"][f][:, 4])
        assert np.array_equal(p["ign_gt"][gs], fr["ign_gt"][f]) and np.array_equal(p["ign_dt"][d], fr["ign_dt"][f])
        assert np.array_equal(p["dc_boxes"][p["dc_off"][f]:p["dc_off"][f + 1]], fr["dc"][f])


def test_pack_frames_empty_and_detections_only(pp):
    ke = pp.kitti_eval
    p = ke.pack_frames([], [], [], [], [], [])
    assert p["nframes"] == 0 and p["gt_off"].tolist() == [0] and p["ov_off"].tolist() == [0]
    assert p["overlaps"].shape == (0,) and p["dt_boxes"].shape == (0, 4) and p["dc_boxes"].shape == (0, 4)
    e = lambda *s: np.zeros(s)  # noqa: E731
    dt3 = np.arange(18.0).reshape(3, 6)
    # an empty frame, a frame with detections but no ground truth, a frame with ground truths but no detection
    p = ke.pack_frames([e(0, 0), e(3, 0), e(0, 2)], [e(0, 5), e(0, 5), e(2, 5)], [e(0, 6), dt3, e(0, 6)],
                       [[], [], [0, 1]], [[], [0, -1, 1], []], [e(0, 4), e(0, 4), np.ones((1, 4))])
    assert p["gt_off"].tolist() == [0, 0, 0, 2] and p["dt_off"].tolist() == [0, 0, 3, 3]
    assert p["ov_off"].tolist() == [0, 0, 0, 0] and p["dc_off"].tolist() == [0, 0, 0, 1]
    assert p["scores"].tolist() == [5.0, 11.0, 17.0] and p["ign_dt"].tolist() == [0, -1, 1] and p["ign_gt"].tolist() == [0, 1]
    with pytest.raises(ValueError):
        ke.pack_frames([e(0, 3)], [e(0, 5)], [dt3], [[]], [[0, 0, 0]], [e(0, 4)])       # overlaps are [D, G]


def test_header_declares_and_exports_list_the_entry_points(pp):
    with open(os.path.join(ROOT, "include", "pp_hip.h")) as f:
        header = f.read()
    for name in ("pp_eval_match", "pp_eval_pr"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*int device\b", header), name
        assert name in pp._lib.EXPORTS
    assert "eval_stats.hip" in pp._lib.SOURCES
    assert re.search(r"#define\s+PP_EVAL_NTHRESH\s+41\b", header) and pp.kitti_eval.N_SAMPLE_PTS == 41
    assert re.search(r"#define\s+PP_EVAL_MAX_BOXES\s+1024\b", header) and pp.kitti_eval.MAX_BOXES_PER_FRAME == 1024


def test_unknown_statistics_mode_raises(pp):
    ke = pp.kitti_eval
    for call in (lambda: ke.get_official_eval_result([], [], ["Pedestrian"], statistics="bogus"),
                 lambda: ke.get_coco_eval_result([], [], ["Pedestrian"], statistics="bogus"),
                 lambda: ke.do_eval_v2([], [], [1], ke.official_min_overlaps(), statistics="bogus"),
                 lambda: ke.do_coco_style_eval([], [], [1], np.zeros((3, 3, 1)), False, statistics="bogus"),
                 lambda: ke.eval_class_v3([], [], [1], [0], 1, ke.official_min_overlaps(), statistics="bogus")):
        with pytest.raises(ValueError, match="statistics"):
            call()
