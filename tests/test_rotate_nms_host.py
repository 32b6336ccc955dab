"""Rotated NMS, the parts that need no GPU: the host restatement (tests/rotate_nms_ref.py) against the reference's keep
lists (tests/golden/ref_rotate_nms.npz: rotate_nms_gpu run by the CUDA-model emulator), the C-ABI's declarations, the
binding's symbol list, the config key and the argument checks of rotate_nms."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

import rotate_nms_ref as rr


@pytest.fixture(scope="module")
def golden():
    return load_golden("ref_rotate_nms.npz")


def fixture_cases(g):
    for name in g["names"].tolist():
        thr, pre, post = g[name + "_args"].tolist()
        yield name, g[name + "_dets"], thr, (None if pre < 0 else int(pre)), (None if post < 0 else int(post)), g[name + "_keep"]


def test_fixture_covers_the_issue(golden):
    names = set(golden["names"].tolist())
    for thr in (0.1, 0.3, 0.5, 0.7):
        for n in (1, 2, 63, 64, 65, 100, 129, 200):
            assert f"rand_t{thr}_n{n}" in names
            k = len(golden[f"rand_t{thr}_n{n}_keep"])
            assert golden[f"rand_t{thr}_n{n}_dets"].shape == (n, 6) and (0 < k < n or n < 63)
    for h in ("identical", "contained", "touching", "octagon", "disjoint", "chain", "far_victim", "victims_63_64"):
        assert "hand_" + h in names
    assert "empty" in names and golden["empty_dets"].shape == (0, 6) and len(golden["empty_keep"]) == 0
    assert sum(n.startswith("cap_") for n in names) >= 5


def test_host_restatement_reproduces_every_reference_keep_list(golden):
    for name, dets, thr, pre, post, keep in fixture_cases(golden):
        got = rr.rotate_nms_ref(dets, thr, pre, post)
        assert got.dtype == np.int64 and np.array_equal(got, keep), name


def test_fixture_margins(golden):
    """No decision of the fixture hangs on the last ulp: every pair's IoU is at least 1e-4 from its threshold."""
    for name, dets, thr, pre, post, keep in fixture_cases(golden):
        if dets.shape[0] >= 2:
            assert rr.min_margin(dets[:, :5], thr) > 1e-4, name


def test_chain_and_block_crossing_cases(golden):
    g = golden
    assert g["hand_chain_keep"].tolist() == [0, 2]                       # A removes B; C survives although IoU(B, C) > thr
    b = g["hand_chain_dets"]
    assert rr.sorted_iou(b[:, :5])[1, 2] > g["hand_chain_args"][0]
    order = np.argsort(-g["hand_far_victim_dets"][:, 5], kind="stable")
    victim = (set(range(140)) - set(g["hand_far_victim_keep"].tolist())).pop()
    assert order[0] == 0 and int(np.where(order == victim)[0][0]) >= 128
    order = np.argsort(-g["hand_victims_63_64_dets"][:, 5], kind="stable")
    gone = set(range(70)) - set(g["hand_victims_63_64_keep"].tolist())
    assert gone == set(order[[63, 64]].tolist())


def test_header_declares_the_nms_surface():
    with open(os.path.join(ROOT, "include", "pp_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+PP_ABI_VERSION\s+4\b", h)
    assert re.search(r"enum\s+pp_nms_mode\s*\{[^}]*PP_NMS_STANDUP\s*=\s*0[^}]*PP_NMS_ROTATED\s*=\s*1[^}]*\}", h, re.S)
    assert re.search(r"int\s+pp_set_nms_mode\s*\(\s*pp_handle\s+h\s*,\s*int32_t\s+mode\s*\)", h)
    assert re.search(r"int\s+pp_get_nms_mode\s*\(\s*pp_handle\s+h\s*,\s*int32_t\s*\*\s*mode\s*\)", h)
    assert re.search(r"int\s+pp_rotate_nms\s*\(\s*int\s+device\s*,\s*const\s+float\s*\*\s*dets\s*,\s*int64_t\s+n\s*,\s*float\s+"
                     r"iou_threshold\s*,\s*int32_t\s+pre_max_size\s*,\s*int32_t\s+post_max_size\s*,\s*int32_t\s*\*\s*keep\s*,"
                     r"\s*int64_t\s*\*\s*n_keep\s*\)", h)
    assert re.search(r"#define\s+PP_RNMS_MAX_BOXES\s+16384\b", h)
    added = h[h.index("later additions within 4"):h.index("#define PP_ABI_VERSION")]
    for name in ("pp_nms_mode", "pp_set_nms_mode", "pp_get_nms_mode", "pp_rotate_nms", "PP_RNMS_MAX_BOXES"):
        assert name in added


def test_binding_lists_the_symbols(pp):
    for name in ("pp_set_nms_mode", "pp_get_nms_mode", "pp_rotate_nms"):
        assert name in pp._lib.EXPORTS
    assert "rotate_nms.hip" in pp._lib.SOURCES and "api_nms.hip" in pp._lib.SOURCES
    assert (pp._lib.PP_NMS_STANDUP, pp._lib.PP_NMS_ROTATED) == (0, 1)
    assert pp.rotate_nms.MAX_BOXES == 16384


def test_config_key(pp):
    import copy
    cfg = pp.config.pedestrian_d435i_config(1)
    assert "use_rotate_nms" not in cfg["model"]["second"]          # the reference's YAML does not have it
    d = pp.config.Derived(cfg)
    assert d.use_rotate_nms is False and d.nms_dict()["use_rotate_nms"] is False
    cfg2 = copy.deepcopy(cfg)
    cfg2["model"]["second"]["use_rotate_nms"] = True
    d2 = pp.config.Derived(cfg2)
    assert d2.use_rotate_nms is True and d2.nms_dict()["use_rotate_nms"] is True
    assert pp.config.Derived(pp.config.kitti_shaped_config(num_class=2)).use_rotate_nms is False
    cfg2["model"]["second"]["use_multi_class_nms"] = True
    with pytest.raises(NotImplementedError):
        pp.config.Derived(cfg2)


def test_rotate_nms_argument_checks(pp):
    rn = pp.rotate_nms
    with pytest.raises(ValueError):
        rn.rotate_nms(np.zeros((3, 5), np.float32), 0.5)
    with pytest.raises(ValueError):
        rn.rotate_nms(np.zeros((6,), np.float32), 0.5)
    bad = np.ones((2, 6), np.float32)
    bad[1, 5] = np.nan
    with pytest.raises(ValueError):
        rn.rotate_nms(bad, 0.5)
    bad[1, 5] = np.inf
    with pytest.raises(ValueError):
        rn.rotate_nms(bad, 0.5)
    with pytest.raises(ValueError):
        rn.boxes_for_rotate_nms(np.zeros((4, 5)))
    b = np.arange(14, dtype=np.float32).reshape(2, 7)
    assert np.array_equal(rn.boxes_for_rotate_nms(b), b[:, [0, 1, 3, 4, 6]])
