"""Soft-NMS, the parts that need no GPU: the host restatement (pp_amd.soft_nms.soft_nms_np) against what the reference's
soft_nms_jit leaves in its array (tests/golden/ref_soft_nms.npz, tools/gen_golden_soft_nms.py), two hand properties, the
C-ABI's declarations, the binding's symbol list, the config keys and the argument checks.

Rows and their order are compared exactly, by coordinates (the reference loses the original indices).  Scores: the fixture
was made by plain Python, which keeps float32 + 1 in float32 where numba -- and the restatement -- widen to float64; the
generator records the largest relative score difference it saw (`max_rel_score_diff`, about 1e-6) and the bound here is
4 x that, for the same typing difference on draws the generator did not see."""
import copy
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from oracle import ref_numpy as rn


@pytest.fixture(scope="module")
def golden():
    return load_golden("ref_soft_nms.npz")


def fixture_cases(g):
    for name in g["names"].tolist():
        method, sigma, nt, thr, pre, post = g[name + "_args"].tolist()
        yield (name, g[name + "_dets"], int(method), sigma, nt, thr, (None if pre < 0 else int(pre)),
               (None if post < 0 else int(post)), g[name + "_kept"])


def assert_matches_fixture(name, dets, keep, scores, kept, rel):
    assert keep.dtype == np.int64 and scores.dtype == np.float32, name
    assert len(keep) == len(kept), (name, len(keep), len(kept))
    assert np.array_equal(dets[keep, :4], kept[:, :4]), name
    if len(keep):
        np.testing.assert_allclose(scores, kept[:, 4], rtol=rel, atol=0, err_msg=name)


def test_fixture_covers_the_issue(golden):
    names = set(golden["names"].tolist())
    for m in (0, 1, 2):
        for n in (0, 1, 2, 7, 33, 64, 65, 100, 300):
            assert golden[f"rand_m{m}_n{n}_dets"].shape == (n, 5)
            assert golden[f"rand_m{m}_n{n}_args"].tolist()[:4] == [m, 0.5, 0.3, 0.001]
        assert golden[f"sig03_nt05_m{m}_n100_args"].tolist()[1:4] == [0.3, 0.5, 0.001]
        assert golden[f"floor005_m{m}_n100_args"].tolist()[1:4] == [0.5, 0.3, 0.05]
        assert "hand_identical_m%d" % m in names
    for h in ("apart_x", "apart_y", "below_floor_overlapping", "below_floor_alone", "accumulated_decay"):
        assert "hand_" + h in names
    assert sum(n.startswith("cap_") for n in names) >= 2
    assert 0.0 < float(golden["max_rel_score_diff"]) < 2.5e-6
    # hard suppression deletes, the soft methods keep more of the same kind of draw
    assert len(golden["rand_m0_n300_kept"]) < len(golden["rand_m2_n300_kept"])


def test_restatement_reproduces_every_reference_result(pp, golden):
    rel = 4.0 * float(golden["max_rel_score_diff"])
    for name, dets, method, sigma, nt, thr, pre, post, kept in fixture_cases(golden):
        keep, scores = pp.soft_nms.soft_nms_np(dets, method, sigma, nt, thr, pre, post)
        assert_matches_fixture(name, dets, keep, scores, kept, rel)


def test_fixture_margins(pp, golden):
    """No decision of the fixture hangs on the last bits of a score: the margins the generator drew for."""
    for name, dets, method, sigma, nt, thr, pre, post, kept in fixture_cases(golden):
        m = pp.soft_nms.decision_margins(dets, method, sigma, nt, thr, pre, post)
        assert m["gap"] > 1e-5 and m["iou"] > 1e-4 and m["floor"] > 1e-6, (name, m)
        assert len(m["decays"]) == len(kept)


def test_floor_cases_as_the_reference_decides_them(golden):
    g = golden
    assert len(g["hand_below_floor_overlapping_kept"]) == 1           # re-scored with weight 1, still dropped
    alone = g["hand_below_floor_alone_kept"]
    assert len(alone) == 2 and alone[1, 4] == np.float32(0.0005)      # never re-scored: kept below the floor
    assert np.array_equal(g["hand_apart_x_kept"], g["hand_apart_x_dets"])
    assert np.array_equal(g["hand_apart_y_kept"], g["hand_apart_y_dets"])
    three, two = g["hand_accumulated_decay_kept"], g["hand_accumulated_decay_two_kept"]
    D = g["hand_accumulated_decay_dets"][3, :4]
    assert len(three) == 3 and not (three[:, :4] == D).all(axis=1).any()      # three decays push D under the floor
    assert len(two) == 3 and (two[2, :4] == D).all() and two[2, 4] > 0.05     # two do not


def test_scores_are_non_increasing_and_ties_take_the_lower_index(pp, golden):
    for name, dets, method, sigma, nt, thr, pre, post, kept in fixture_cases(golden):
        keep, scores = pp.soft_nms.soft_nms_np(dets, method, sigma, nt, thr, pre, post)
        assert (np.diff(scores) <= 0).all(), name
    d = np.array([[0, 0, 10, 10, 0.5], [100, 0, 110, 10, 0.5], [200, 0, 210, 10, 0.7], [300, 0, 310, 10, 0.5]], np.float32)
    keep, scores = pp.soft_nms.soft_nms_np(d, "gaussian")
    assert keep.tolist() == [2, 0, 1, 3] and scores.tolist() == [np.float32(0.7)] + [0.5] * 3
    keep, _ = pp.soft_nms.soft_nms_np(d, "gaussian", pre_max_size=3, post_max_size=2)     # boxes 2, 0, 1 enter
    assert keep.tolist() == [2, 0]


def test_hard_method_is_the_greedy_rule(pp, golden):
    """Method 0 with a floor of 1e-30: the keep list of the stand-up NMS restatement (oracle.ref_numpy.nms_gpu) on the same
    rows, in order, with untouched scores."""
    ran = 0
    for name, dets, method, sigma, nt, thr, pre, post, kept in fixture_cases(golden):
        if not name.startswith("rand_m0_") or len(dets) == 0 or len(dets) > 100:
            continue
        keep, scores = pp.soft_nms.soft_nms_np(dets, "hard", 0.5, nt, 1e-30)
        ref = np.array(rn.nms_gpu(dets, nt), dtype=np.int64)
        assert np.array_equal(keep, ref), name
        assert np.array_equal(scores, dets[ref, 4]), name
        ran += 1
    assert ran >= 7


def test_header_declares_the_soft_nms_surface():
    with open(os.path.join(ROOT, "include", "pp_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+PP_ABI_VERSION\s+4\b", h)
    assert re.search(r"enum\s+pp_nms_mode\s*\{[^}]*PP_NMS_STANDUP\s*=\s*0[^}]*PP_NMS_ROTATED\s*=\s*1[^}]*PP_NMS_SOFT\s*=\s*2[^}]*\}", h, re.S)
    assert re.search(r"enum\s+pp_soft_nms_method\s*\{[^}]*PP_SOFT_NMS_HARD\s*=\s*0[^}]*PP_SOFT_NMS_LINEAR\s*=\s*1[^}]*"
                     r"PP_SOFT_NMS_GAUSSIAN\s*=\s*2[^}]*\}", h, re.S)
    assert re.search(r"int\s+pp_set_soft_nms\s*\(\s*pp_handle\s+h\s*,\s*int32_t\s+method\s*,\s*float\s+sigma\s*,\s*float\s+"
                     r"score_floor\s*\)", h)
    assert re.search(r"int\s+pp_get_soft_nms\s*\(\s*pp_handle\s+h\s*,\s*int32_t\s*\*\s*method\s*,\s*float\s*\*\s*sigma\s*,"
                     r"\s*float\s*\*\s*score_floor\s*\)", h)
    assert re.search(r"int\s+pp_soft_nms\s*\(\s*int\s+device\s*,\s*const\s+float\s*\*\s*dets\s*,\s*int64_t\s+n\s*,\s*int32_t\s+"
                     r"method\s*,\s*float\s+sigma\s*,\s*float\s+iou_threshold\s*,\s*float\s+score_floor\s*,\s*int32_t\s+"
                     r"pre_max_size\s*,\s*int32_t\s+post_max_size\s*,\s*int32_t\s*\*\s*keep\s*,\s*float\s*\*\s*scores\s*,"
                     r"\s*int64_t\s*\*\s*n_keep\s*\)", h)
    assert re.search(r"#define\s+PP_SNMS_MAX_BOXES\s+4096\b", h)
    added = h[h.index("later additions within 4"):h.index("#define PP_ABI_VERSION")]
    new = ("PP_NMS_SOFT", "pp_soft_nms_method", "pp_set_soft_nms", "pp_get_soft_nms", "PP_SNMS_MAX_BOXES", "pp_soft_nms.")
    last_old = added.index("pp_publish_info")
    pos = [added.index(name) for name in new]
    assert pos == sorted(pos) and pos[0] > last_old, "the new names follow the last earlier one, in order"
    # nothing before them moved: the earlier names still stand in their order
    earlier = ("pp_target_config", "pp_rotate_nms", "pp_set_projection", "pp_class_nms", "PP_METRICS_COUNTS",
               "pp_grad_clip_mode", "pp_publish_stats", "pp_publish_info")
    pos = [added.index(name) for name in earlier]
    assert pos == sorted(pos)


def test_binding_lists_the_symbols(pp):
    for name in ("pp_set_soft_nms", "pp_get_soft_nms", "pp_soft_nms"):
        assert name in pp._lib.EXPORTS
    assert "soft_nms.hip" in pp._lib.SOURCES
    assert (pp._lib.PP_NMS_STANDUP, pp._lib.PP_NMS_ROTATED, pp._lib.PP_NMS_SOFT) == (0, 1, 2)
    assert (pp._lib.PP_SOFT_NMS_HARD, pp._lib.PP_SOFT_NMS_LINEAR, pp._lib.PP_SOFT_NMS_GAUSSIAN) == (0, 1, 2)
    assert pp.soft_nms.MAX_BOXES == pp._lib.PP_SNMS_MAX_BOXES == 4096
    assert pp.soft_nms.METHODS == {"hard": 0, "linear": 1, "gaussian": 2}


def test_config_keys(pp):
    cfg = pp.config.pedestrian_d435i_config(1)
    s = cfg["model"]["second"]
    assert "use_soft_nms" not in s and "soft_nms" not in s          # the reference's YAML has neither
    d = pp.config.Derived(cfg)
    assert d.use_soft_nms is False and d.soft_nms is None and d.nms_dict()["use_soft_nms"] is False
    cfg2 = copy.deepcopy(cfg)
    cfg2["model"]["second"].update(use_soft_nms=True, soft_nms={"method": "linear", "sigma": 0.3, "score_floor": 0.01})
    d2 = pp.config.Derived(cfg2)
    assert d2.use_soft_nms is True and d2.soft_nms == {"method": "linear", "sigma": 0.3, "score_floor": 0.01}
    assert d2.nms_dict()["use_soft_nms"] is True and d2.use_rotate_nms is False
    cfg3 = copy.deepcopy(cfg2)
    cfg3["model"]["second"]["use_rotate_nms"] = True
    with pytest.raises(ValueError, match="use_soft_nms"):
        pp.config.Derived(cfg3)
    cfg4 = copy.deepcopy(cfg2)
    cfg4["model"]["second"]["soft_nms"]["gamma"] = 1.0
    with pytest.raises(ValueError, match="gamma"):
        pp.config.Derived(cfg4)


def test_argument_checks(pp):
    sn = pp.soft_nms
    ok = np.array([[0, 0, 10, 10, 0.9], [5, 5, 20, 20, 0.8]], np.float32)
    for f in (sn.soft_nms, sn.soft_nms_np, sn.decision_margins):       # all raise before anything is launched
        with pytest.raises(ValueError):
            f(np.zeros((3, 6), np.float32))
        with pytest.raises(ValueError):
            f(np.zeros((5,), np.float32))
        for bad_score in (np.nan, np.inf):
            bad = ok.copy()
            bad[1, 4] = bad_score
            with pytest.raises(ValueError, match="finite"):
                f(bad)
        for kw in ({"method": "median"}, {"method": 3}, {"sigma": 0.0}, {"sigma": np.nan}, {"score_floor": -1e-3},
                   {"score_floor": np.inf}, {"iou_threshold": np.nan}):
            with pytest.raises(ValueError):
                f(ok, **kw)
    assert sn.method_id("linear") == 1 and sn.method_id(2) == 2
