"""GPU target assignment (csrc/targets.hip), host side: the threshold reader and the C-ABI surface."""
import ctypes
import os
import re

import pytest

import pp_amd as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpu_target_config_reads_the_thresholds():
    cfg = pp.config.pedestrian_d435i_config()
    assert pp.target_assigner.gpu_target_config(cfg) == (0.5, 0.35)
    assert pp.target_assigner.gpu_target_config(pp.config.Derived(cfg)) == (0.5, 0.35)
    for frac in (None, "None"):
        cfg["model"]["second"]["target_assigner"]["sample_positive_fraction"] = frac
        assert pp.target_assigner.gpu_target_config(cfg) == (0.5, 0.35)


def test_gpu_target_config_refuses_positive_fraction_sampling():
    cfg = pp.config.pedestrian_d435i_config()
    cfg["model"]["second"]["target_assigner"]["sample_positive_fraction"] = 0.25
    with pytest.raises(ValueError, match="global generator"):
        pp.target_assigner.gpu_target_config(cfg)


def test_target_entry_points_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    for name in ("pp_assign_targets", "pp_train_step_gt_async", "pp_train_step_gt"):
        assert name in pp._lib.EXPORTS, name
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, flags=re.M), name
    assert "targets.hip" in pp._lib.SOURCES
    assert re.search(r"#define\s+PP_MAX_GT_PER_FRAME\s+256\b", hdr)


def test_target_config_struct_layout():
    assert ctypes.sizeof(pp._lib.PPTargetConfig) == 16
    assert [f for f, _ in pp._lib.PPTargetConfig._fields_] == ["matched_threshold", "unmatched_threshold", "reserved"]


def test_pack_gt_layout():
    import numpy as np
    boxes, cls, counts = pp.Engine.pack_gt([np.ones((2, 7)), np.zeros((0, 7)), np.full((1, 7), 2.0)], [[1, 2], [], [1]])
    assert boxes.dtype == np.float32 and boxes.shape == (3, 7) and boxes.flags.c_contiguous
    assert cls.dtype == np.int32 and cls.tolist() == [1, 2, 1]
    assert counts.dtype == np.int32 and counts.tolist() == [2, 0, 1]
    assert pp.Engine.pack_gt([np.ones((1, 7))])[1] is None
    with pytest.raises(ValueError):
        pp.Engine.pack_gt([np.ones((2, 7))], [[1]])
