"""Golden vectors for the object-database build (pp_amd.gt_database, csrc/gt_database.hip), produced by RUNNING the
reference's own create_groundtruth_database and _calculate_num_points_in_gt (create_data.py:365-551, :28-93) on a small
synthetic dataset written to a temporary directory in the reference's file layout (build container only, through
ref_shim).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_gtdb.py   ->  tests/golden/ref_gt_database.npz

Which functions produced it (also stored in the fixture, `produced_by`): create_data.py imports here as it is, with
second.core.box_np_ops behind it -- box_camera_to_lidar, points_in_rbbox (center_to_corner_box3d, corner_to_surfaces_3d)
and second.core.geometry.points_in_convex_polygon_3d_jit / surface_equ_3d_jit; numba's decorators are ref_shim's
identity stand-ins, so the jitted loops run as plain Python; the prebuilt box_ops_cc.so does not load and is not on this
path.  Nothing had to be routed to load_data.py's copies.

Recorded (data only): per frame the cloud, the annotations and the calibration; rbbox_lidar as the reference's
box_camera_to_lidar returned it inside create_groundtruth_database; annos["num_points_in_gt"] as
_calculate_num_points_in_gt left it; per object of kitti_dbinfos_train.pkl the info dict's fields and the points of the
file the reference wrote for it; the paths of a second run with used_classes = ["Pedestrian"].
12 frames, 0-6 objects each (Pedestrian, Cyclist, DontCare last): frame 3 has no annotations, frame 7 only a DontCare, an
object of frame 1 holds no point, two boxes of frame 2 overlap and share points; half the frames carry a score, two
carry group_ids.
Asserted here: no point lies within 1e-5 m of a face of any box of its frame (box_np_ops builds the planes with
np.cross / einsum, the restatement and the device with explicit sums: with that margin membership cannot depend on the
formulation); gt_database.box_camera_to_lidar, build_objects_np, calculate_num_points_in_gt and
create_groundtruth_database (engine=None) reproduce the reference's boxes, bytes, counts and dicts.
"""
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ref_shim.install()
import create_data as cd  # noqa: E402
from second.core import box_np_ops  # noqa: E402
import pp_amd  # noqa: E402

aug, gdb = pp_amd.augment, pp_amd.gt_database
USED = ["Pedestrian", "Cyclist"]
N_FRAMES = 12
PRODUCED_BY = ["create_data.create_groundtruth_database", "create_data._calculate_num_points_in_gt",
               "second.core.box_np_ops.box_camera_to_lidar", "second.core.box_np_ops.points_in_rbbox",
               "second.core.box_np_ops.center_to_corner_box3d", "second.core.box_np_ops.corner_to_surfaces_3d",
               "second.core.geometry.points_in_convex_polygon_3d_jit", "second.core.geometry.surface_equ_3d_jit"]

_lidar_log = []
_orig_c2l = box_np_ops.box_camera_to_lidar


def _rec_c2l(data, r_rect, velo2cam):
    r = _orig_c2l(data, r_rect, velo2cam)
    _lidar_log.append(np.array(r))
    return r


def calib(rng):
    a = rng.uniform(-0.02, 0.02, 3)
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    rot = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
           @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))
    rect = np.eye(4)
    rect[:3, :3] = rot
    trv2c = np.eye(4)
    trv2c[:3, :3] = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]) + rng.uniform(-0.01, 0.01, (3, 3))
    trv2c[:3, 3] = rng.uniform(-0.3, 0.3, 3)
    p2 = np.array([[720.0, 0, 610.0, 45.0], [0, 720.0, 172.0, 0.2], [0, 0, 1.0, 0.003], [0, 0, 0, 1.0]])
    return rect, trv2c, p2


def lidar_box(rng, name):
    w, l, h = (0.6, 0.8, 1.7) if name != "Cyclist" else (0.6, 1.6, 1.6)
    return np.array([rng.uniform(0.8, 5.8), rng.uniform(-2.0, 2.0), rng.uniform(-0.9, -0.5), w * rng.uniform(0.85, 1.15),
                     l * rng.uniform(0.85, 1.15), h * rng.uniform(0.9, 1.1), rng.uniform(-np.pi, np.pi)])


def make_frame(rng, k):
    rect, trv2c, p2 = calib(rng)
    plans = {0: ["Pedestrian", "Cyclist", "DontCare"], 1: ["Pedestrian", "Pedestrian", "Cyclist"], 2: ["Pedestrian", "Pedestrian"],
             3: [], 4: ["Cyclist"] * 2 + ["Pedestrian"] * 4, 5: ["Pedestrian", "DontCare", "DontCare"], 6: ["Cyclist", "Cyclist"],
             7: ["DontCare"], 8: ["Pedestrian"] * 3 + ["Cyclist"], 9: ["Pedestrian", "Cyclist", "Pedestrian", "DontCare"],
             10: ["Cyclist"], 11: ["Pedestrian"] * 5}
    names = plans[k]
    boxes = np.array([lidar_box(rng, n) for n in names]).reshape(-1, 7)
    if k == 1:
        boxes[1, :2] = (9.0, 4.0)                       # an object outside the cloud: no points
    if k == 2:
        boxes[1] = boxes[0] + np.array([0.25, 0.15, 0.05, 0, 0, 0, 0.4])      # overlapping boxes that share points
    # camera boxes: the centre through rect @ trv2c, x y z l h w r
    cam_xyz = (np.concatenate([boxes[:, :3], np.ones((len(boxes), 1))], 1) @ (rect @ trv2c).T)[:, :3]
    n_bg = int(rng.integers(300, 2600))
    p = [np.stack([rng.uniform(0.05, 6.35, n_bg), rng.uniform(-2.5, 2.5, n_bg), rng.uniform(-1.4, 1.4, n_bg)], 1)]
    for b in boxes:                                      # a cluster on every object
        m = int(rng.integers(20, 160))
        u = rng.uniform(-0.6, 0.6, (m, 3))
        c, s = np.cos(b[6]), np.sin(b[6])
        lx, ly = u[:, 0] * b[3], u[:, 1] * b[4]
        p.append(np.stack([lx * c + ly * s + b[0], -lx * s + ly * c + b[1], (u[:, 2] + 0.5) * b[5] + b[2]], 1))
    p = np.concatenate(p, 0)
    p = p[rng.permutation(len(p))].astype(np.float32)
    if k == 1:
        p = p[np.hypot(p[:, 0] - 9.0, p[:, 1] - 4.0) > 2.0]
    n_obj = len([n for n in names if n != "DontCare"])
    annos = {"name": np.array(names, dtype="<U16"), "location": cam_xyz.reshape(-1, 3),
             "dimensions": boxes[:, [4, 5, 3]].reshape(-1, 3), "rotation_y": boxes[:, 6].reshape(-1),
             "bbox": rng.uniform(0, 300, (len(names), 4)), "difficulty": rng.integers(-1, 3, len(names)).astype(np.int32),
             "index": np.array(list(range(n_obj)) + [-1] * (len(names) - n_obj), np.int32),
             "truncated": np.zeros(len(names)), "occluded": np.zeros(len(names), np.int32), "alpha": np.zeros(len(names))}
    if k % 2 == 0:
        annos["score"] = rng.uniform(0, 1, len(names))
    if k == 4:
        annos["group_ids"] = np.array([0, 0, 1, 2, 2, 3], np.int64)
    if k == 8:
        annos["group_ids"] = np.array([5, 5, 5, 1], np.int64)
    info = {"image_idx": f"{k:06d}", "pointcloud_num_features": 3, "velodyne_path": f"velodyne/{k:06d}.bin",
            "img_path": f"image_2/{k:06d}.png", "img_shape": np.array([375, 1242], np.int32),
            "calib/R0_rect": rect, "calib/Tr_velo_to_cam": trv2c, "calib/P2": p2, "annos": annos}
    # the margin: drop what lies within 1e-5 m (and a little) of a face of any box of the frame
    lidar = gdb.box_camera_to_lidar(np.concatenate([annos["location"], annos["dimensions"],
                                                    annos["rotation_y"][:, None]], 1), rect, trv2c)
    if len(lidar):
        pn, pd = aug.box_planes(lidar)
        sg = aug.face_sign(p[:, :3].astype(np.float64), pn, pd)
        p = p[(np.abs(sg) / np.linalg.norm(pn, axis=-1)[None]).min(axis=(1, 2)) > 2e-5]
    return info, p


def near_face(p, lidar, tol):
    if not len(lidar) or not len(p):
        return 0
    pn, pd = aug.box_planes(lidar)
    sg = aug.face_sign(p[:, :3].astype(np.float64), pn, pd)
    return int(((np.abs(sg) / np.linalg.norm(pn, axis=-1)[None]).min(axis=(1, 2)) <= tol).sum())


def main():
    rng = np.random.default_rng(2026)
    infos, clouds = [], []
    for k in range(N_FRAMES):
        info, p = make_frame(rng, k)
        infos.append(info)
        clouds.append(p)
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "velodyne"))
    for info, p in zip(infos, clouds):
        with open(os.path.join(tmp, info["velodyne_path"][:-3] + "pkl"), "wb") as f:
            pickle.dump(p, f, 2)
    out = {"n_frames": np.array(N_FRAMES), "used_classes": np.array(USED), "produced_by": np.array(PRODUCED_BY)}
    for k, (info, p) in enumerate(zip(infos, clouds)):
        out[f"f{k}__points"] = p
        out[f"f{k}__image_idx"] = np.array(info["image_idx"])
        for key in ("calib/R0_rect", "calib/Tr_velo_to_cam", "calib/P2"):
            out[f"f{k}__{key.replace('/', '_')}"] = info[key]
        for key, v in info["annos"].items():
            out[f"f{k}__anno__{key}"] = np.array(v)

    # ---- the reference: num_points_in_gt, then the database ----
    cd._calculate_num_points_in_gt(tmp, infos, True)
    for k, info in enumerate(infos):
        assert info["annos"]["num_points_in_gt"].dtype == np.int32
        out[f"f{k}__num_points_in_gt"] = info["annos"]["num_points_in_gt"]
    with open(os.path.join(tmp, "kitti_infos_train.pkl"), "wb") as f:
        pickle.dump(infos, f)
    box_np_ops.box_camera_to_lidar = _rec_c2l
    cd.create_groundtruth_database(tmp, "train", used_classes=list(USED))
    box_np_ops.box_camera_to_lidar = _orig_c2l
    assert len(_lidar_log) == N_FRAMES
    with open(os.path.join(tmp, "kitti_dbinfos_train.pkl"), "rb") as f:
        ref_infos = pickle.load(f)
    assert list(ref_infos) == USED
    ref_points = {}
    for name in USED:
        objs = ref_infos[name]
        ref_points[name] = []
        for o in objs:
            with open(os.path.join(tmp, o["path"][:-3] + "pkl"), "rb") as f:
                a = pickle.load(f)
            assert a.dtype == np.float32 and a.shape == (o["num_points_in_gt"], 3), (o["path"], a.dtype, a.shape)
            ref_points[name].append(a)
        out[f"db__{name}__name"] = np.array([o["name"] for o in objs])
        out[f"db__{name}__path"] = np.array([o["path"] for o in objs])
        out[f"db__{name}__image_idx"] = np.array([o["image_idx"] for o in objs])
        out[f"db__{name}__gt_idx"] = np.array([o["gt_idx"] for o in objs], np.int32)
        out[f"db__{name}__box3d_lidar"] = np.array([o["box3d_lidar"] for o in objs], np.float64).reshape(-1, 7)
        out[f"db__{name}__num_points_in_gt"] = np.array([o["num_points_in_gt"] for o in objs], np.int64)
        out[f"db__{name}__difficulty"] = np.array([o["difficulty"] for o in objs], np.int32)
        out[f"db__{name}__group_id"] = np.array([o["group_id"] for o in objs], np.int64)
        out[f"db__{name}__has_score"] = np.array(["score" in o for o in objs], bool)
        out[f"db__{name}__score"] = np.array([o.get("score", np.nan) for o in objs], np.float64)
        out[f"db__{name}__points"] = np.concatenate(ref_points[name] + [np.zeros((0, 3), np.float32)], 0)
        out[f"db__{name}__offsets"] = np.concatenate([[0], np.cumsum([len(a) for a in ref_points[name]])]).astype(np.int64)
    for k in range(N_FRAMES):
        out[f"f{k}__rbbox_lidar"] = _lidar_log[k]
    # a second run: the used_classes filter
    tmp2 = os.path.join(tmp, "ped_only.pkl")
    cd.create_groundtruth_database(tmp, "train", used_classes=["Pedestrian"], db_info_save_path=tmp2)
    with open(tmp2, "rb") as f:
        ped = pickle.load(f)
    assert list(ped) == ["Pedestrian"]
    out["ped_only__path"] = np.array([o["path"] for o in ped["Pedestrian"]])
    out["ped_only__group_id"] = np.array([o["group_id"] for o in ped["Pedestrian"]], np.int64)

    # ---- assertions: the margin, and the restatement against the reference ----
    near = sum(near_face(p, _lidar_log[k], 1e-5) for k, p in enumerate(clouds))
    assert near == 0, f"{near} points within 1e-5 m of a face"
    shared = empty = 0
    for k, (info, p) in enumerate(zip(infos, clouds)):
        lidar = gdb.frame_boxes(info)
        assert np.array_equal(lidar, _lidar_log[k]), k
        counts, objs = gdb.build_objects_np(p, lidar)
        a = info["annos"]
        n_obj = len(lidar)
        assert np.array_equal(a["num_points_in_gt"][:n_obj], counts) and (a["num_points_in_gt"][n_obj:] == -1).all(), k
        empty += int((counts == 0).sum())
        if n_obj >= 2:
            pn, pd = aug.box_planes(lidar)
            ins = (aug.face_sign(p[:, :3].astype(np.float64), pn, pd) < 0).all(-1)
            shared += int((ins.sum(1) >= 2).sum())
    assert empty >= 1 and shared >= 10, (empty, shared)
    twin = [dict(i, annos={k: v for k, v in i["annos"].items() if k != "num_points_in_gt"}) for i in infos]
    gdb.calculate_num_points_in_gt(None, twin, clouds)
    for t, i in zip(twin, infos):
        assert t["annos"]["num_points_in_gt"].dtype == np.int32
        assert np.array_equal(t["annos"]["num_points_in_gt"], i["annos"]["num_points_in_gt"])
    my_infos, my_points = gdb.create_groundtruth_database(None, infos, clouds, used_classes=USED)
    assert list(my_infos) == USED
    n_objects = 0
    for name in USED:
        assert len(my_infos[name]) == len(ref_infos[name]), name
        for mo, ro, mp, rp in zip(my_infos[name], ref_infos[name], my_points[name], ref_points[name]):
            assert set(mo) == set(ro), (mo, ro)
            for key in ro:
                assert np.array_equal(mo[key], ro[key]), (key, mo[key], ro[key])
            assert mp.dtype == rp.dtype and mp.shape == rp.shape and mp.tobytes() == rp.tobytes(), ro["path"]
            n_objects += 1
    my_ped, _ = gdb.create_groundtruth_database(None, infos, clouds, used_classes=["Pedestrian"])
    assert [o["path"] for o in my_ped["Pedestrian"]] == out["ped_only__path"].tolist()
    assert [o["group_id"] for o in my_ped["Pedestrian"]] == out["ped_only__group_id"].tolist()
    path = os.path.join(ROOT, "tests", "golden", "ref_gt_database.npz")
    np.savez_compressed(path, **out)
    print("frames", N_FRAMES, "points", [len(p) for p in clouds], "objects", n_objects, "empty objects", empty,
          "shared points", shared, "near-face points", near, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
