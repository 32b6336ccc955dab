"""The object-database build on the host (gt_database.py): the float64 restatement, the camera -> lidar conversion,
num_points_in_gt and the info dicts against tests/golden/ref_gt_database.npz -- what the reference's
create_groundtruth_database and _calculate_num_points_in_gt wrote for the same frames (tools/gen_golden_gtdb.py) --, the
round trip through the reference's file layout, and the refusals."""
import random

import numpy as np
import pytest

from conftest import load_golden

ANNO_KEYS = ("name", "location", "dimensions", "rotation_y", "bbox", "difficulty", "index", "score", "group_ids")


def fixture_dataset():
    """(G, infos, clouds): the fixture's frames as kitti-info dicts (without num_points_in_gt) and float32 clouds."""
    G = load_golden("ref_gt_database.npz")
    infos, clouds = [], []
    for k in range(int(G["n_frames"])):
        annos = {key: G[f"f{k}__anno__{key}"] for key in ANNO_KEYS if f"f{k}__anno__{key}" in G}
        infos.append({"image_idx": str(G[f"f{k}__image_idx"]), "calib/R0_rect": G[f"f{k}__calib_R0_rect"],
                      "calib/Tr_velo_to_cam": G[f"f{k}__calib_Tr_velo_to_cam"], "calib/P2": G[f"f{k}__calib_P2"],
                      "annos": annos})
        clouds.append(G[f"f{k}__points"])
    return G, infos, clouds


def check_database(G, db_infos, db_points, classes=None):
    """all_db_infos / points against the reference's dicts and files: fields equal, points bit-identical."""
    classes = list(G["used_classes"]) if classes is None else classes
    assert list(db_infos) == classes and list(db_points) == classes
    n = 0
    for name in classes:
        objs, off = db_infos[name], G[f"db__{name}__offsets"]
        assert len(objs) == len(off) - 1 == len(db_points[name])
        for i, (o, p) in enumerate(zip(objs, db_points[name])):
            want = {"name", "path", "image_idx", "gt_idx", "box3d_lidar", "num_points_in_gt", "difficulty", "group_id"}
            if G[f"db__{name}__has_score"][i]:
                want.add("score")
                assert o["score"] == G[f"db__{name}__score"][i]
            assert set(o) == want
            for key in ("name", "path", "image_idx", "gt_idx", "num_points_in_gt", "difficulty", "group_id"):
                assert o[key] == G[f"db__{name}__{key}"][i], (name, i, key)
            assert np.array_equal(o["box3d_lidar"], G[f"db__{name}__box3d_lidar"][i])
            ref = G[f"db__{name}__points"][off[i]:off[i + 1]]
            assert p.dtype == np.float32 and p.shape == ref.shape and p.tobytes() == ref.tobytes(), (name, i)
            n += 1
    return n


def test_fixture_names_its_producers():
    G = load_golden("ref_gt_database.npz")
    made = set(G["produced_by"].tolist())
    assert {"create_data.create_groundtruth_database", "create_data._calculate_num_points_in_gt",
            "second.core.box_np_ops.points_in_rbbox", "second.core.box_np_ops.box_camera_to_lidar"} <= made


def test_box_camera_to_lidar_equals_reference(pp):
    gdb = pp.gt_database
    G, infos, _ = fixture_dataset()
    seen = 0
    for k, info in enumerate(infos):
        lidar = gdb.frame_boxes(info)
        assert lidar.dtype == np.float64 and np.array_equal(lidar, G[f"f{k}__rbbox_lidar"])
        seen += len(lidar)
    assert seen > 20
    with pytest.raises(ValueError, match=r"\[n, 7\]"):
        gdb.box_camera_to_lidar(np.zeros((2, 6)), np.eye(4), np.eye(4))


def test_build_objects_np_equals_reference_files(pp):
    gdb = pp.gt_database
    G, infos, clouds = fixture_dataset()
    by_path = {}
    for name in G["used_classes"]:
        off = G[f"db__{name}__offsets"]
        for i, path in enumerate(G[f"db__{name}__path"]):
            by_path[str(path)] = (G[f"db__{name}__points"][off[i]:off[i + 1]], int(G[f"db__{name}__num_points_in_gt"][i]))
    empty = shared = checked = 0
    for k, (info, cloud) in enumerate(zip(infos, clouds)):
        lidar = G[f"f{k}__rbbox_lidar"]
        counts, objs = gdb.build_objects_np(cloud, lidar)
        assert counts.dtype == np.int32 and len(objs) == len(lidar)
        assert np.array_equal(counts, G[f"f{k}__num_points_in_gt"][:len(lidar)])
        a = info["annos"]
        for i, o in enumerate(objs):
            ref, n = by_path[f"gt_database/{info['image_idx']}_{a['name'][i]}_{a['index'][i]}.bin"]
            assert n == counts[i] and o.dtype == np.float32 and o.tobytes() == ref.tobytes()
            checked += 1
        empty += int((counts == 0).sum())
        shared += int(counts.sum()) > len(cloud) or (len(lidar) >= 2 and _shared(pp, cloud, lidar) > 0)
    assert checked == 29 and empty >= 1 and shared >= 1
    c0, o0 = gdb.build_objects_np(clouds[0], np.zeros((0, 7)))
    assert len(c0) == 0 and o0 == []
    c0, o0 = gdb.build_objects_np(np.zeros((0, 3), np.float32), G["f0__rbbox_lidar"])
    assert c0.tolist() == [0] * len(G["f0__rbbox_lidar"]) and all(o.shape == (0, 3) for o in o0)


def _shared(pp, cloud, lidar):
    n, d = pp.augment.box_planes(lidar)
    ins = (pp.augment.face_sign(cloud[:, :3].astype(np.float64), n, d) < 0).all(-1)
    return int((ins.sum(1) >= 2).sum())


def test_extra_columns_are_copied(pp):
    gdb = pp.gt_database
    G, _, clouds = fixture_dataset()
    lidar = G["f2__rbbox_lidar"]
    p4 = np.concatenate([clouds[2], np.arange(len(clouds[2]), dtype=np.float32)[:, None]], 1)
    c3, o3 = gdb.build_objects_np(clouds[2], lidar)
    c4, o4 = gdb.build_objects_np(p4, lidar)
    assert np.array_equal(c3, c4)
    for a, b in zip(o3, o4):
        assert a.tobytes() == np.ascontiguousarray(b[:, :3]).tobytes()
        assert np.array_equal(p4[b[:, 3].astype(int), 3], b[:, 3]) and (np.diff(b[:, 3]) > 0).all()    # the frame's order


def test_calculate_num_points_in_gt_equals_reference(pp):
    gdb = pp.gt_database
    G, infos, clouds = fixture_dataset()
    gdb.calculate_num_points_in_gt(None, infos, clouds)
    ignored = 0
    for k, info in enumerate(infos):
        got = info["annos"]["num_points_in_gt"]
        assert got.dtype == np.int32 and np.array_equal(got, G[f"f{k}__num_points_in_gt"])
        ignored += int((got == -1).sum())
    assert ignored >= 4


def test_info_dicts_and_points_equal_reference(pp):
    gdb = pp.gt_database
    G, infos, clouds = fixture_dataset()
    db_infos, db_points = gdb.create_groundtruth_database(None, infos, iter(clouds), used_classes=list(G["used_classes"]))
    assert check_database(G, db_infos, db_points) == 29
    ped, _ = gdb.create_groundtruth_database(None, infos, clouds, used_classes=["Pedestrian"])
    assert [o["path"] for o in ped["Pedestrian"]] == G["ped_only__path"].tolist()
    assert [o["group_id"] for o in ped["Pedestrian"]] == G["ped_only__group_id"].tolist()
    every, _ = gdb.create_groundtruth_database(None, infos, clouds)
    assert list(every) == list(gdb.KITTI_CLASSES) and len(every["Car"]) == 0 and len(every["Cyclist"]) == 9


def test_bev_only_sets_z_and_height(pp):
    gdb = pp.gt_database
    G, infos, clouds = fixture_dataset()
    rng = [0.0, -2.56, -1.5, 6.4, 2.56, 1.5]
    db_infos, db_points = gdb.create_groundtruth_database(None, infos, clouds, used_classes=["Pedestrian"], bev_only=True,
                                                          coors_range=rng)
    for o, p in zip(db_infos["Pedestrian"], db_points["Pedestrian"]):
        assert o["box3d_lidar"][2] == -1.5 and o["box3d_lidar"][5] == 3.0 and o["num_points_in_gt"] == len(p)
    assert sum(len(p) for p in db_points["Pedestrian"]) > int(G["db__Pedestrian__offsets"][-1])


def _sampler_cfg(pp):
    return pp.gt_sampler.SamplerConfig.from_input_reader({"sample_classes": ["Pedestrian", "Cyclist"],
                                                          "sample_max_nums": [5, 3]})


def test_reference_files_round_trip(pp, tmp_path):
    import pickle
    gdb, gts = pp.gt_database, pp.gt_sampler
    G, infos, clouds = fixture_dataset()
    db_infos, db_points = gdb.create_groundtruth_database(None, infos, clouds, used_classes=list(G["used_classes"]))
    pkl = gdb.write_reference_files(db_infos, db_points, tmp_path)
    assert pkl.name == "kitti_dbinfos_train.pkl"
    first = db_infos["Pedestrian"][0]
    with open(str(tmp_path / first["path"])[:-3] + "pkl", "rb") as f:
        head = f.read(2)
        f.seek(0)
        a = pickle.load(f)
    assert head == b"\x80\x02" and a.tobytes() == db_points["Pedestrian"][0].tobytes()       # protocol 2, as the reference
    direct = gts.GtDatabase(db_infos, db_points, _sampler_cfg(pp), np.random.RandomState(3), random.Random(3), 3)
    back = gts.GtDatabase.from_reference_files(pkl, tmp_path, True, _sampler_cfg(pp), np.random.RandomState(3),
                                               random.Random(3), 3)
    assert len(back) == len(direct) > 0
    for key in ("boxes", "points", "offsets", "classes"):
        assert getattr(back, key).tobytes() == getattr(direct, key).tobytes(), key
    # the KITTI layout: raw float32 .bin files
    pkl2 = gdb.write_reference_files(db_infos, db_points, tmp_path / "bin", custom_dataset=False, info_name="kitti_dbinfos_val.pkl")
    back2 = gts.GtDatabase.from_reference_files(pkl2, tmp_path / "bin", False, _sampler_cfg(pp), np.random.RandomState(3),
                                                random.Random(3), 3)
    assert back2.points.tobytes() == direct.points.tobytes() and back2.offsets.tobytes() == direct.offsets.tobytes()


def test_refusals(pp):
    gdb = pp.gt_database
    G, infos, clouds = fixture_dataset()
    with pytest.raises(ValueError, match="float32"):
        gdb.build_objects_np(clouds[0].astype(np.float64), G["f0__rbbox_lidar"])
    with pytest.raises(ValueError, match="float32"):
        gdb.create_groundtruth_database(None, infos, [c.astype(np.float64) for c in clouds])
    with pytest.raises(ValueError, match="float32"):
        gdb.calculate_num_points_in_gt(None, infos, [c.astype(np.float64) for c in clouds])
    with pytest.raises(ValueError, match="differ in length"):
        gdb.create_groundtruth_database(None, infos, clouds[:-1])
    with pytest.raises(ValueError, match="differ in length"):
        gdb.create_groundtruth_database(None, infos[:-1], clouds)
    bad = dict(infos[0], annos=dict(infos[0]["annos"], location=infos[0]["annos"]["location"][:-1]))
    with pytest.raises(ValueError, match="entries of 'location'"):
        gdb.create_groundtruth_database(None, [bad], clouds[:1])
    with pytest.raises(ValueError, match="bev_only needs coors_range"):
        gdb.create_groundtruth_database(None, infos, clouds, bev_only=True)
    with pytest.raises(ValueError, match="at most 256"):
        gdb.build_objects_np(clouds[0], np.repeat(G["f0__rbbox_lidar"][:1], 257, 0))
    with pytest.raises(ValueError, match="not finite"):
        gdb.build_objects_np(clouds[0], np.array([[0, 0, 0, 1, 1, 1, np.nan]]))
    with pytest.raises(ValueError, match="size <= 0"):
        gdb.build_objects_np(clouds[0], np.array([[0, 0, 0, 1, 0, 1, 0.0]]))
    with pytest.raises(ValueError, match="infos but"):
        gdb.write_reference_files({"Pedestrian": [{"path": "gt_database/a.bin"}]}, {"Pedestrian": []}, "unused")
