"""GT-database sampling, host side: pp_amd.gt_sampler's BatchSampler twin and float64 restatement against the
reference's own DataBaseSamplerV2 / BatchSampler / sample_all (tests/golden/ref_gt_sample.npz,
tools/gen_golden_gtsample.py), the config parser, the database's refusals and the C-ABI additions."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

G = load_golden("ref_gt_sample.npz")
CASES = [str(n) for n in G["names"]]
DB_CLASSES = ["Pedestrian", "Cyclist"]


def fixture_db(pp, F=3):
    """The database of the fixture, built by the twin from the recorded inputs and seeds."""
    gts = pp.gt_sampler
    infos, points = {}, {}
    for name in DB_CLASSES:
        boxes, off = G[f"db_in__{name}__boxes"], G[f"db_in__{name}__offsets"]
        infos[name] = [{"box3d_lidar": boxes[i], "difficulty": int(G[f"db_in__{name}__difficulty"][i]),
                        "num_points_in_gt": int(G[f"db_in__{name}__num_points"][i])} for i in range(len(boxes))]
        p = G[f"db_in__{name}__points"]
        if F > 3:
            p = np.concatenate([p, np.linspace(0, 1, len(p) * (F - 3), dtype=np.float32).reshape(len(p), F - 3)], 1)
        points[name] = [p[off[i]:off[i + 1]] for i in range(len(boxes))]
    cfg = gts.SamplerConfig.from_input_reader({"sample_classes": DB_CLASSES, "sample_max_nums": [5, 3]})
    seed = int(G["seed"])
    return gts.GtDatabase(infos, points, cfg, np.random.RandomState(seed), random.Random(seed), F)


def case_cfg(pp, c):
    return pp.gt_sampler.SamplerConfig.from_input_reader({
        "sample_classes": [str(s) for s in G[f"case__{c}__sample_classes"]],
        "sample_max_nums": [int(n) for n in G[f"case__{c}__sample_max_nums"]],
        "sampler_max_point_collision": int(G[f"case__{c}__cfg"][0]),
        "sampler_min_point_collision": int(G[f"case__{c}__cfg"][1])})


def test_batch_sampler_twin_matches_reference(pp):
    db = fixture_db(pp)
    for name in DB_CLASSES:
        np.testing.assert_array_equal(db.samplers[name].indices, G[f"db__{name}__indices"])
        assert db.samplers[name].boxes.dtype == np.float64
        np.testing.assert_array_equal(db.samplers[name].boxes, G[f"db__{name}__boxes"])      # bit for bit
    # difficulty -1 and the Cyclist minimum of points are filtered before the shuffle
    assert len(db.samplers["Pedestrian"].boxes) == int((G["db_in__Pedestrian__difficulty"] != -1).sum())
    assert len(db.samplers["Cyclist"].boxes) == int((G["db_in__Cyclist__num_points"] >= 5).sum())
    # every cursor call since construction, the tail + reshuffle calls among them
    off, wrapped = G["cursor__offsets"], 0
    for i, (name, num) in enumerate(zip(G["cursor__class"], G["cursor__num"])):
        s = db.samplers[str(name)]
        wrapped += s.idx + int(num) >= len(s.boxes)
        np.testing.assert_array_equal(s.sample(int(num)), G["cursor__indices"][off[i]:off[i + 1]], err_msg=f"call {i}")
    assert wrapped >= 1


@pytest.mark.parametrize("case", CASES)
def test_sample_all_np_matches_reference(pp, case):
    gts = pp.gt_sampler
    db = fixture_db(pp)
    pre = f"case__{case}__"
    frame = G["frame__" + str(G[pre + "frame"])]
    pts, boxes, cls, valid, info = gts.sample_all_np(frame, G[pre + "gt_boxes"], G[pre + "gt_classes"], None, db,
                                                     G[pre + "cands"], G[pre + "cand_counts"], case_cfg(pp, case),
                                                     return_info=True)
    np.testing.assert_array_equal(info["accepted"], G[pre + "accepted"])
    want_pts = np.concatenate([G[pre + "pasted"], frame], 0)
    assert pts.dtype == np.float32 and pts.shape == want_pts.shape
    assert pts.tobytes() == want_pts.tobytes()                 # bit-identical
    np.testing.assert_array_equal(boxes, np.concatenate([G[pre + "gt_boxes"], G[pre + "ret_boxes"]], 0))
    np.testing.assert_array_equal(cls, np.concatenate([G[pre + "gt_classes"], G[pre + "ret_classes"]]))
    assert valid.all()
    np.testing.assert_array_equal(info["status"], G[pre + "status"])
    np.testing.assert_array_equal(info["point_counts"], G[pre + "point_counts"])
    assert info["round_used"] == int(G[pre + "round_used"])
    # the survivors of the box test and their point counts as the reference's points_in_rbbox calls saw them
    n = int(G[pre + "cand_counts"].sum())
    surv = [k for k in range(n) if info["status"][k] != gts.BOX_COLLISION]
    np.testing.assert_array_equal(db.boxes[G[pre + "cands"]["object"][surv]], G[pre + "surv_boxes"])
    np.testing.assert_array_equal(info["point_counts"][surv], G[pre + "surv_counts"])


def test_fixture_covers_the_listed_cases(pp):
    gts = pp.gt_sampler
    st = {c: G[f"case__{c}__status"][:int(G[f"case__{c}__cand_counts"].sum())] for c in CASES}
    pc = {c: G[f"case__{c}__point_counts"] for c in CASES}
    assert len(G["case__shipped__gt_boxes"]) == 2 and len(G["case__no_boxes__gt_boxes"]) == 0
    assert (st["max_points"] == gts.TOO_MANY_POINTS).any()
    assert (st["empty_object"] == gts.EMPTY_OBJECT).any()
    assert any(s == gts.ACCEPTED and pc["near_low"][k] == 0 for k, s in enumerate(st["near_low"]))
    assert (st["later_candidate"] == gts.BOX_COLLISION).any()
    assert int(G["case__enough_boxes__cand_counts"].sum()) == 0 and len(G["case__enough_boxes__pasted"]) == 0
    assert set(G["case__two_classes__cands"]["group"][:len(st["two_classes"])]) == {0, 1}


def test_failed_rounds_and_retry(pp):
    """A frame without boxes takes the first round that accepts something; one whose rounds all fail comes back
    unchanged."""
    gts = pp.gt_sampler
    db = fixture_db(pp)
    frame = G["frame__full"]
    empty = [i for i in range(len(db)) if db.offsets[i + 1] == db.offsets[i]]
    full = [i for i in range(len(db)) if db.offsets[i + 1] > db.offsets[i] and db.classes[i] == 1]
    cands = np.zeros(gts.PP_GTS_MAX_CAND, gts.CAND_DTYPE)
    cands["object"][:3] = [empty[0], empty[0], full[0]]       # rounds 0 and 1: an object without points
    counts = np.array([1, 1, 1, 0], np.int32)
    pts, boxes, cls, valid, info = gts.sample_all_np(frame, np.zeros((0, 7)), None, None, db, cands, counts,
                                                     return_info=True)
    assert info["round_used"] == 2 and info["accepted"].tolist() == [full[0]]
    assert info["status"][:3].tolist() == [gts.EMPTY_OBJECT, gts.EMPTY_OBJECT, gts.ACCEPTED]
    assert len(pts) == len(frame) + db.offsets[full[0] + 1] - db.offsets[full[0]] and len(boxes) == 1
    counts = np.array([1, 1, 0, 0], np.int32)
    pts, boxes, cls, valid, info = gts.sample_all_np(frame, np.zeros((0, 7)), None, None, db, cands, counts,
                                                     return_info=True)
    assert info["round_used"] == -1 and len(boxes) == 0 and pts.tobytes() == frame.tobytes()
    # a frame that has boxes uses its first round only
    box = G["case__shipped__gt_boxes"][:1]
    counts = np.array([1, 1, 1, 0], np.int32)
    _, boxes, _, _, info = gts.sample_all_np(frame, box, None, None, db, cands, counts, return_info=True)
    assert info["status"][1:3].tolist() == [gts.ROUND_NOT_USED] * 2 and len(boxes) == 1


def test_draw_candidates(pp):
    gts = pp.gt_sampler
    db = fixture_db(pp)
    c = gts.draw_candidates(db, [[1, 1], [], [1, 1, 1, 1, 1, 2, 2, 2]], random.Random(3))
    assert c.cands.shape == (3, gts.PP_GTS_MAX_CAND) and c.counts.shape == (3, gts.PP_GTS_MAX_ROUNDS)
    assert c.counts[0].tolist()[1:] == [0, 0, 0] and 0 < c.counts[0, 0] <= 6      # 3 Pedestrians + 3 Cyclists wanted
    assert (c.counts[1] > 0).all() and c.counts[1].sum() <= gts.PP_GTS_MAX_CAND   # no boxes: every round drawn
    assert c.counts[2].sum() == 0                                                # enough boxes of both classes
    n0 = int(c.counts[0, 0])
    assert (np.diff(c.cands["group"][0, :n0]) >= 0).all()
    assert (db.classes[c.cands["object"][0, :n0]] == c.cands["group"][0, :n0] + 1).all()
    assert set(np.unique(c.cands["low"])) <= {0, 1}


def test_sampler_config_refusals(pp):
    SC = pp.gt_sampler.SamplerConfig
    d = SC.from_input_reader(None)
    assert d.sample_classes == ["Pedestrian"] and d.sample_max_nums == [8]
    assert (d.max_point_collision, d.min_point_collision, d.noise_x_point) == (500, 1, 2.5)
    assert d.noise_x_closer == (-0.8, 0.2) and d.noise_x_farther == (-0.2, 1.5) and d.noise_y == (-1.25, 1.25)
    assert SC.from_input_reader({"sample_classes": None}) is None
    for bad, key in (({"sample_classes": "Pedestrian"}, "sample_classes"), ({"sample_classes": []}, "sample_classes"),
                     ({"sample_classes": ["a", "a"], "sample_max_nums": [1, 1]}, "sample_classes"),
                     ({"sample_max_nums": [8, 8]}, "sample_max_nums"), ({"sample_max_nums": [-1]}, "sample_max_nums"),
                     ({"sample_max_nums": [2.5]}, "sample_max_nums"), ({"sample_max_nums": [33]}, "sample_max_nums"),
                     ({"sampler_max_point_collision": -1}, "sampler_max_point_collision"),
                     ({"sampler_min_point_collision": 1.5}, "sampler_min_point_collision"),
                     ({"sampler_noise_y": [1.0, -1.0]}, "sampler_noise_y"),
                     ({"sampler_noise_x_closer": [0.0]}, "sampler_noise_x_closer"),
                     ({"sampler_noise_x_farther": [0.0, float("nan")]}, "sampler_noise_x_farther"),
                     ({"sampler_noise_x_point": float("inf")}, "sampler_noise_x_point")):
        with pytest.raises(ValueError, match=key):
            SC.from_input_reader(bad)


def test_database_refusals(pp):
    gts = pp.gt_sampler
    cfg = gts.SamplerConfig.from_input_reader(None)
    obj = {"box3d_lidar": np.array([1, 0, -0.7, 0.6, 0.8, 1.7, 0.0]), "difficulty": 0, "num_points_in_gt": 4}
    mk = lambda infos, points, F=3, c=cfg: gts.GtDatabase(infos, points, c, np.random.RandomState(0),  # noqa: E731
                                                        random.Random(0), F)
    with pytest.raises(ValueError, match="no 'Pedestrian' objects"):
        mk({"Cyclist": [obj]}, {"Cyclist": [np.zeros((4, 3), np.float32)]})
    with pytest.raises(ValueError, match="no 'Pedestrian' objects"):      # all filtered out
        mk({"Pedestrian": [dict(obj, difficulty=-1)]}, {"Pedestrian": [np.zeros((4, 3), np.float32)]})
    with pytest.raises(ValueError, match=r"points must be \[n, 4\]"):
        mk({"Pedestrian": [obj]}, {"Pedestrian": [np.zeros((4, 3), np.float32)]}, F=4)
    with pytest.raises(ValueError, match="1 infos but 0 point arrays"):
        mk({"Pedestrian": [obj]}, {"Pedestrian": []})
    with pytest.raises(ValueError, match="SamplerConfig"):
        mk({"Pedestrian": [obj]}, {"Pedestrian": [np.zeros((4, 3), np.float32)]}, c={})
    db = mk({"Pedestrian": [obj, dict(obj, num_points_in_gt=0)]},
            {"Pedestrian": [np.zeros((4, 3), np.float32), np.zeros((0, 3), np.float32)]})
    assert len(db) == 2 and db.offsets.tolist() in ([0, 4, 4], [0, 0, 4]) and db.classes.tolist() == [1, 1]
    # the minimum-points table is a parameter whose default is the reference's
    db = gts.GtDatabase({"Pedestrian": [obj, dict(obj, num_points_in_gt=9)]},
                        {"Pedestrian": [np.zeros((4, 3), np.float32), np.zeros((9, 3), np.float32)]}, cfg,
                        np.random.RandomState(0), random.Random(0), 3, min_points={"Pedestrian": 5})
    assert len(db) == 1 and db.offsets.tolist() == [0, 9]
    assert gts.MIN_GT_POINTS == {"Cyclist": 5}


def test_from_reference_files(pp, tmp_path):
    import pickle
    gts = pp.gt_sampler
    rng = np.random.default_rng(0)
    infos = {"Pedestrian": [], "Cyclist": []}
    os.makedirs(tmp_path / "gt_database")
    want = {}
    for name, n in (("Pedestrian", 3), ("Cyclist", 1)):
        for i in range(n):
            p = rng.normal(size=(5 + i, 3)).astype(np.float32)
            infos[name].append({"name": name, "path": f"gt_database/{name}_{i}.bin", "difficulty": 0, "num_points_in_gt": len(p),
                                "box3d_lidar": np.array([1.0 + i, 0.5, -0.7, 0.6, 0.8, 1.7, 0.1])})
            with open(tmp_path / f"gt_database/{name}_{i}.pkl", "wb") as f:
                pickle.dump(p, f)
            p.tofile(tmp_path / f"gt_database/{name}_{i}.bin")
            want[(name, i)] = p
    with open(tmp_path / "dbinfos.pkl", "wb") as f:
        pickle.dump(infos, f)
    cfg = gts.SamplerConfig.from_input_reader(None)
    for custom in (True, False):
        db = gts.GtDatabase.from_reference_files(tmp_path / "dbinfos.pkl", tmp_path, custom, cfg, np.random.RandomState(1),
                                                 random.Random(1), 3)
        assert len(db) == 3 and db.classes.tolist() == [1, 1, 1]
        for i in range(3):
            np.testing.assert_array_equal(db.object_points(i), want[("Pedestrian", i)])
            assert db.boxes[i, 2:].tolist() == [-0.7, 0.6, 0.8, 1.7, 0.1] and db.boxes[i, 0] != 1.0 + i


def test_header_declares_gt_sample_abi(pp):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    assert re.search(r"#define\s+PP_ABI_VERSION\s+4\b", hdr)
    assert re.search(r"#define\s+PP_GTS_MAX_CAND\s+32\b", hdr) and pp.gt_sampler.PP_GTS_MAX_CAND == 32
    assert re.search(r"#define\s+PP_GTS_MAX_ROUNDS\s+4\b", hdr) and pp.gt_sampler.PP_GTS_MAX_ROUNDS == 4
    for sym in ("pp_gtdb_load", "pp_gt_sample", "pp_gt_sample_info", "pp_train_step_sample_async", "pp_train_step_sample"):
        assert re.search(r"^int\s+" + sym + r"\s*\(", hdr, flags=re.M), sym
        assert sym in pp._lib.EXPORTS, sym
    for k, name in enumerate(("ACCEPTED", "BOX_COLLISION", "TOO_MANY_POINTS", "TOO_FEW_POINTS", "EMPTY_OBJECT",
                              "ROUND_NOT_USED")):
        assert re.search(r"PP_GTS_" + name + r"\s*=\s*" + str(k) + r"\b", hdr), name
        assert getattr(pp.gt_sampler, name) == k
    assert len(pp.gt_sampler.STATUS_NAMES) == 6


def test_struct_sizes_match_dtypes(pp):
    gts = pp.gt_sampler
    assert ctypes.sizeof(pp._lib.PPGtsCand) == gts.CAND_DTYPE.itemsize == 16
    assert ctypes.sizeof(pp._lib.PPGtSampleConfig) == gts.CONFIG_DTYPE.itemsize == 16
    assert [f[0] for f in pp._lib.PPGtsCand._fields_] == list(gts.CAND_DTYPE.names)
    assert [f[0] for f in pp._lib.PPGtSampleConfig._fields_] == list(gts.CONFIG_DTYPE.names)


def test_from_reference_files_refuses_flat_points(pp, tmp_path):
    import pickle
    gts = pp.gt_sampler
    os.makedirs(tmp_path / "gt_database")
    infos = {"Pedestrian": [{"name": "Pedestrian", "path": "gt_database/p_0.bin", "difficulty": 0, "num_points_in_gt": 2,
                             "box3d_lidar": np.array([1.0, 0.5, -0.7, 0.6, 0.8, 1.7, 0.1])}]}
    with open(tmp_path / "gt_database/p_0.pkl", "wb") as f:
        pickle.dump(np.zeros(6, np.float32), f)               # 1-D: two points flattened
    with open(tmp_path / "dbinfos.pkl", "wb") as f:
        pickle.dump(infos, f)
    with pytest.raises(ValueError, match=r"points must be a 2-D array \[n, F\]"):
        gts.GtDatabase.from_reference_files(tmp_path / "dbinfos.pkl", tmp_path, True, gts.SamplerConfig.from_input_reader(None),
                                            np.random.RandomState(1), random.Random(1), 3)


def test_valid_flags_are_checked_against_boxes_not_draw_rows(pp):
    """A sampled + augmented step has more draw rows (boxes + candidate slots) than boxes; the flags describe the boxes."""
    acfg = pp.augment.AugmentConfig.from_input_reader(None)
    draws = pp.augment.draw(np.random.RandomState(0), [np.zeros((16, 7))], acfg)
    ac, valid, frames, bd = pp.Engine._aug_args(np.ones(3, np.uint8), 16, draws, acfg, n_boxes=3)
    assert len(valid) == 3 and bd.shape[0] == 16
    with pytest.raises(ValueError, match="gt_valid: 3 flags for 16 boxes"):
        pp.Engine._aug_args(np.ones(3, np.uint8), 16, draws, acfg)
    with pytest.raises(ValueError, match="gt_valid: 4 flags for 3 boxes"):
        pp.Engine._aug_args(np.ones(4, np.uint8), 16, draws, acfg, n_boxes=3)
