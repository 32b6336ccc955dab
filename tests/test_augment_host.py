"""Training-time augmentation, host side: pp_amd.augment's draws and float64 restatement against the reference's own
stages (tests/golden/ref_augment.npz, tools/gen_golden_augment.py), the shuffle permutation, the config parser and
the C-ABI additions."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

G = load_golden("ref_augment.npz")
CASES = [str(n) for n in G["names"]]
PC_RANGE = np.array([0, -2.56, -3.0, 6.40, 2.56, 3.0])


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    tol = 2e-6 * np.maximum(1.0, np.abs(b))
    bad = np.abs(a - b) > tol
    assert not bad.any(), (np.abs(a - b).max(), a[bad][:5], b[bad][:5])


def case_cfg(pp, c):
    v = G[c + "__cfg"]
    return pp.augment.AugmentConfig(v[0:2], v[2:5], v[5:7], v[7:9], v[9:11], v[11:14], int(v[14]))


def run(pp, c):
    cfg = case_cfg(pp, c)
    boxes = G[c + "__in_boxes"].reshape(-1, 7)
    rs = np.random.RandomState(int(G[c + "__seed"]))
    d = pp.augment.draw(rs, [boxes], cfg)
    return pp.augment.augment_np(G[c + "__in_points"], boxes, None, G[c + "__in_valid"], d.frame(0), cfg, PC_RANGE,
                                 return_info=True)


@pytest.mark.parametrize("case", CASES)
def test_stages_match_reference(pp, case):
    pts, boxes, cls, info = run(pp, case)
    c = case
    np.testing.assert_array_equal(info["selected"], G[c + "__selected"])
    np.testing.assert_array_equal(info["owner"], G[c + "__owner"])
    for s in ("s1", "s3", "s4", "s5", "s6"):
        xyz, bx = info["stages"][s]
        close(xyz, G[f"{c}__{s}_points"][:, :3])
        ref_b = G[f"{c}__{s}_boxes"]
        close(bx, ref_b)
    close(info["stages"]["s7"][1], G[c + "__s7_boxes"])
    assert info["flip"] == bool(np.any(G[c + "__s3_points"][:, 1] != G[c + "__s1_points"][:, 1])) or \
        not np.any(G[c + "__s1_points"][:, 1])
    np.testing.assert_array_equal(info["keep"], G[c + "__keep"])
    close(boxes, G[c + "__out_boxes"])
    np.testing.assert_array_equal(cls, G[c + "__out_classes"])
    # stage 8: the reference's shuffle and ours are permutations of the same stage-6 cloud
    pre = pts[np.argsort(info["perm"])]
    close(pre[:, :3], G[c + "__s6_points"][:, :3])
    key = lambda a: np.lexsort(np.asarray(a, np.float32).T[::-1])  # noqa: E731
    ref8 = G[c + "__s8_points"]
    close(np.sort(ref8[key(ref8)], 0), np.sort(G[c + "__s6_points"], 0))


def test_flip_cases_cover_both_sides(pp):
    flips = [run(pp, c)[3]["flip"] for c in CASES]
    assert any(flips) and not all(flips)


def test_randomstate_shuffle_is_an_index_shuffle():
    pts = np.random.default_rng(0).normal(size=(1000, 4)).astype(np.float32)
    a, b = np.random.RandomState(77), np.random.RandomState(77)
    p1 = pts.copy()
    a.shuffle(p1)
    idx = np.arange(len(pts))
    b.shuffle(idx)
    np.testing.assert_array_equal(p1, pts[idx])


@pytest.mark.parametrize("n", [0, 1, 2, 3, 1000, 32768, 32769])
def test_shuffle_perm_is_a_bijection(pp, n):
    p = pp.augment.shuffle_perm(123456789, n)
    assert p.shape == (n,)
    np.testing.assert_array_equal(np.sort(p), np.arange(n))
    np.testing.assert_array_equal(p, pp.augment.shuffle_perm(123456789, n))
    if n >= 1000:
        assert not np.array_equal(p, pp.augment.shuffle_perm(123456790, n))
        assert not np.array_equal(p, np.arange(n))


def test_draw_consumes_the_reference_stream(pp):
    """Same seed, same numpy calls: after one frame's draws the stream sits where the reference leaves it before the
    shuffle (one extra randint here instead of N swaps)."""
    cfg = pp.augment.AugmentConfig.from_input_reader({})
    boxes = np.array([[1.0, 0.5, -0.6, 0.6, 0.8, 1.7, 0.1], [3.0, -1.0, -0.6, 0.6, 0.8, 1.7, 1.0]])
    d = pp.augment.draw(np.random.RandomState(5), [boxes], cfg).frame(0)
    rs = np.random.RandomState(5)
    loc = rs.normal(scale=np.array([0.15, 0.15, 0.05]), size=[2, 100, 3])
    rot = rs.uniform(cfg.rot_noise[0], cfg.rot_noise[1], size=[2, 100])
    g = np.arctan2(boxes[:, 0], boxes[:, 1])
    grot = rs.uniform((0.0 - g)[:, None], (0.0 - g)[:, None], size=[2, 100])
    np.testing.assert_array_equal(d["boxes"][..., :3], loc)
    np.testing.assert_array_equal(d["boxes"][..., 3], rot)
    np.testing.assert_array_equal(d["boxes"][..., 4], grot)
    assert d["flip"] == bool(rs.choice([False, True], replace=False, p=[0.5, 0.5]))
    assert d["theta"] == rs.uniform(*cfg.global_rot)
    assert d["scale"] == rs.uniform(*cfg.scaling)


def test_config_parses_shipped_yaml(pp):
    cfg = pp.augment.AugmentConfig.from_input_reader({
        "groundtruth_rotation_uniform_noise": [-0.39269908169, 0.39269908169],
        "groundtruth_localization_noise_std": [0.15, 0.15, 0.05],
        "global_random_rotation_range_per_object": [0, 0],
        "global_rotation_uniform_noise": [-0.178539816, 0.178539816],
        "global_scaling_uniform_noise": [0.95, 1.05],
        "global_loc_noise_std": [0.1, 0.1, 0.2]})
    d = pp.augment.AugmentConfig.from_input_reader(None)
    assert vars(cfg) == vars(d)
    assert cfg.num_try == 100 and not cfg.global_rot_per_object
    assert pp.augment.AugmentConfig.from_input_reader(
        {"global_random_rotation_range_per_object": [-0.1, 0.1]}).global_rot_per_object


@pytest.mark.parametrize("bad", [
    {"groundtruth_rotation_uniform_noise": [0.1]},
    {"groundtruth_rotation_uniform_noise": [0.2, 0.1]},
    {"groundtruth_localization_noise_std": [0.1, 0.1]},
    {"groundtruth_localization_noise_std": [0.1, -0.1, 0.1]},
    {"global_random_rotation_range_per_object": [1.0, -1.0]},
    {"global_rotation_uniform_noise": [0.0, 1.0, 2.0]},
    {"global_scaling_uniform_noise": [0.0, 1.05]},
    {"global_scaling_uniform_noise": [1.1, 1.0]},
    {"global_loc_noise_std": [0.1, 0.1, -0.2]},
    {"global_loc_noise_std": 0.1},
    {"num_try": 0},
    {"num_try": 129},
    {"num_try": 2.5},
])
def test_config_refuses_malformed(pp, bad):
    with pytest.raises(ValueError):
        pp.augment.AugmentConfig.from_input_reader(bad)


def test_header_declares_augment_abi(pp):
    h = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    assert re.search(r"#define PP_AUG_MAX_TRY 128", h)
    for sym in ("pp_augment", "pp_train_step_aug_async", "pp_train_step_aug"):
        assert re.search(r"\bint " + sym + r"\(", h), sym
        assert sym in pp._lib.EXPORTS
    assert "pp_augment_config" in h and "pp_aug_frame" in h
    assert pp.augment.FRAME_DTYPE.itemsize == 48
