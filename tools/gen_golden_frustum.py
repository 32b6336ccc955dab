"""Golden vectors for the frustum crop (pp_amd.frustum, csrc/frustum_crop.hip), produced by RUNNING the reference's own
box_np_ops.remove_outside_points (second/core/box_np_ops.py:647-664) and, for the database path, remove_outside_points
followed by points_in_rbbox as create_groundtruth_database (create_data.py:455-504) and _calculate_num_points_in_gt
(create_data.py:58-84) compose them -- their KITTI branch, which a hard-coded `custom_dataset = True` switches off there
(build container only, through ref_shim).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_frustum.py   ->  tests/golden/ref_frustum.npz

Which functions produced it (also stored in the fixture, `produced_by`): remove_outside_points with
projection_matrix_to_CRT_kitti, get_frustum, camera_to_lidar, corner_to_surfaces_3d_jit and
second.core.geometry.points_in_convex_polygon_3d_jit / surface_equ_3d_jit behind it; box_camera_to_lidar and
points_in_rbbox for the labelled frames.  numba's decorators are ref_shim's identity stand-ins: the jitted loops run as
plain Python (a float32 coordinate times a float64 plane value is a float64 product there as under numba).

Recorded (data only), per frame: the cloud, rect, Trv2c, P2, image_shape; C / R / T as projection_matrix_to_CRT_kitti
returned them, the 8 lidar corners as camera_to_lidar returned them and the planes (n0 n1 n2 d) as surface_equ_3d_jit
returned them, all three INSIDE the remove_outside_points call (the functions are wrapped); the kept rows.
Frames: `a0..a9` F = 4 with 0, 1, 63, 64, 65, 255, 256, 257, 1000, 3000 points (a3 and a7 with a 370 x 1224 image, the rest
375 x 1242); `b0..b2` F = 3; `neg` entirely at x < 0 (nothing kept); `cone` entirely inside a narrow cone in front of the
camera (everything kept); `odd` with a NaN point and a +inf point; `back` = a8's cloud with column 0 negated first, as
_create_reduced_point_cloud does.  Labelled frames `g0..g2` (F = 4): Pedestrian and Cyclist boxes placed across the
frustum's side faces, a DontCare last in g1; per frame the annotations, rbbox_lidar, num_points_in_gt with and without the
crop and the objects' points.
Asserted here: every mixed frame both keeps and removes points; at least one box's count differs with and without the
crop; no finite point lies within 1e-6 m of a frustum plane (|s| / |n|), none within 1e-5 m of a box face; and
frustum.remove_outside_points_np, frustum_planes (rtol 1e-12) and the engine=None database functions reproduce every
recorded array.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ref_shim.install()
from second.core import box_np_ops, geometry  # noqa: E402
import pp_amd  # noqa: E402
import gen_golden_gtdb as gg  # noqa: E402

aug, gdb, fru = pp_amd.augment, pp_amd.gt_database, pp_amd.frustum
PRODUCED_BY = ["second.core.box_np_ops.remove_outside_points", "second.core.box_np_ops.projection_matrix_to_CRT_kitti",
               "second.core.box_np_ops.get_frustum", "second.core.box_np_ops.camera_to_lidar",
               "second.core.box_np_ops.corner_to_surfaces_3d_jit", "second.core.geometry.points_in_convex_polygon_3d_jit",
               "second.core.geometry.surface_equ_3d_jit", "second.core.box_np_ops.box_camera_to_lidar",
               "second.core.box_np_ops.points_in_rbbox"]
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 3000]
SMALL_IMAGE = (3, 7)                       # the frames of set a with a 370 x 1224 image
USED = ["Pedestrian", "Cyclist"]

_log = {}
_orig = {"crt": box_np_ops.projection_matrix_to_CRT_kitti, "c2l": box_np_ops.camera_to_lidar,
         "equ": geometry.surface_equ_3d_jit}


def _rec_crt(proj):
    r = _orig["crt"](proj)
    _log["C"], _log["R"], _log["T"] = (np.array(v) for v in r)
    return r


def _rec_c2l(points, r_rect, velo2cam):
    r = _orig["c2l"](points, r_rect, velo2cam)
    _log["corners"] = np.array(r)
    return r


def _rec_equ(surfaces):
    n, d = _orig["equ"](surfaces)
    _log["planes"] = np.concatenate([np.array(n)[0], np.array(d)[0][:, None]], axis=1)
    return n, d


def reference_crop(points, rect, trv2c, p2, image_shape):
    """remove_outside_points with its three intermediate products recorded."""
    _log.clear()
    box_np_ops.projection_matrix_to_CRT_kitti, box_np_ops.camera_to_lidar = _rec_crt, _rec_c2l
    geometry.surface_equ_3d_jit = _rec_equ
    try:
        with np.errstate(invalid="ignore", over="ignore"):
            kept = box_np_ops.remove_outside_points(points, rect, trv2c, p2, image_shape)
    finally:
        box_np_ops.projection_matrix_to_CRT_kitti, box_np_ops.camera_to_lidar = _orig["crt"], _orig["c2l"]
        geometry.surface_equ_3d_jit = _orig["equ"]
    assert set(_log) == {"C", "R", "T", "corners", "planes"} and _log["planes"].shape == (6, 4) and _log["corners"].shape == (8, 3)
    return np.array(kept), dict(_log)


def uniform_cloud(rng, n, F):
    cols = [rng.uniform(-10, 70, n), rng.uniform(-30, 30, n), rng.uniform(-3, 2, n)] + [rng.uniform(0, 1, n)] * (F - 3)
    return np.stack(cols, 1).astype(np.float32).reshape(n, F)


def plane_margin(points, planes):
    """Smallest |s| / |n| over the finite points of a cloud and the six planes."""
    p = points[np.isfinite(points[:, :3]).all(1), :3].astype(np.float64)
    if not len(p):
        return np.inf
    s = ((p[:, 0:1] * planes[:, 0] + p[:, 1:2] * planes[:, 1]) + p[:, 2:3] * planes[:, 2]) + planes[:, 3]
    return float((np.abs(s) / np.linalg.norm(planes[:, :3], axis=1)).min())


def side_point(corners, face, t, s):
    """A point on side face `face` of the frustum: fraction t of the way from the near to the far edge, fraction s
    along the edge."""
    c = corners[fru.FACE_CORNERS[face]]
    near = [k for k in range(4) if fru.FACE_CORNERS[face][k] < 4]
    far = [k for k in range(4) if fru.FACE_CORNERS[face][k] >= 4]
    a = c[near[0]] + s * (c[near[1]] - c[near[0]])
    b = c[far[0]] + s * (c[far[1]] - c[far[0]])
    return a + t * (b - a)


def labelled_frame(rng, k):
    rect, trv2c, p2 = gg.calib(rng)
    shape = np.array([375, 1242], np.int32)
    corners = fru.frustum_corners_lidar(rect, trv2c, p2, shape)
    names = {0: ["Pedestrian", "Cyclist", "Pedestrian"], 1: ["Cyclist", "Pedestrian", "Pedestrian", "DontCare"],
             2: ["Pedestrian", "Cyclist"]}[k]
    boxes = []
    for i, name in enumerate(names):
        w, l, h = (0.6, 0.8, 1.7) if name != "Cyclist" else (0.6, 1.6, 1.6)
        # faces 4 and 5 are the image's left and right edge; the last Pedestrian of g0 and g1 stands well inside
        inside = name == "Pedestrian" and i == 2
        c = side_point(corners, 4 + (i + k) % 2, rng.uniform(0.06, 0.2), 0.5)
        if inside:
            c = np.array([rng.uniform(8, 20), rng.uniform(-1, 1), c[2]])
        hh = h * rng.uniform(0.9, 1.1)
        boxes.append([c[0], c[1], c[2] - hh / 2, w * rng.uniform(0.85, 1.15), l * rng.uniform(0.85, 1.15), hh,
                      rng.uniform(-np.pi, np.pi)])
    boxes = np.array(boxes).reshape(-1, 7)
    cam_xyz = (np.concatenate([boxes[:, :3], np.ones((len(boxes), 1))], 1) @ (rect @ trv2c).T)[:, :3]
    p = [uniform_cloud(rng, int(rng.integers(900, 1500)), 4).astype(np.float64)]
    for b in boxes:
        m = int(rng.integers(60, 160))
        u = rng.uniform(-0.6, 0.6, (m, 3))
        c, s = np.cos(b[6]), np.sin(b[6])
        lx, ly = u[:, 0] * b[3], u[:, 1] * b[4]
        p.append(np.stack([lx * c + ly * s + b[0], -lx * s + ly * c + b[1], (u[:, 2] + 0.5) * b[5] + b[2],
                           rng.uniform(0, 1, m)], 1))
    p = np.concatenate(p, 0)
    p = p[rng.permutation(len(p))].astype(np.float32)
    n_obj = len([n for n in names if n != "DontCare"])
    annos = {"name": np.array(names, dtype="<U16"), "location": cam_xyz.reshape(-1, 3),
             "dimensions": boxes[:, [4, 5, 3]].reshape(-1, 3), "rotation_y": boxes[:, 6].reshape(-1),
             "bbox": rng.uniform(0, 300, (len(names), 4)), "difficulty": rng.integers(-1, 3, len(names)).astype(np.int32),
             "index": np.array(list(range(n_obj)) + [-1] * (len(names) - n_obj), np.int32)}
    info = {"image_idx": f"{k:06d}", "pointcloud_num_features": 4, "velodyne_path": f"training/velodyne/{k:06d}.bin",
            "img_shape": shape, "calib/R0_rect": rect, "calib/Tr_velo_to_cam": trv2c, "calib/P2": p2, "annos": annos}
    # the margin: drop what lies within 1e-5 m (and a little) of a face of any box of the frame
    lidar = gdb.frame_boxes(info)
    pn, pd = aug.box_planes(lidar)
    sg = aug.face_sign(p[:, :3].astype(np.float64), pn, pd)
    p = p[(np.abs(sg) / np.linalg.norm(pn, axis=-1)[None]).min(axis=(1, 2)) > 2e-5]
    return info, p


def main():
    rng = np.random.default_rng(2027)
    out = {"produced_by": np.array(PRODUCED_BY), "sizes": np.array(SIZES)}
    frames = {}

    def add(name, cloud, cal, shape, back=False):
        rect, trv2c, p2 = cal
        shape = np.array(shape, np.int32)
        src = cloud
        if back:                                   # _create_reduced_point_cloud: negate, then crop
            src = cloud.copy()
            src[:, 0] = -src[:, 0]
        kept, rec = reference_crop(src, rect, trv2c, p2, shape)
        assert kept.dtype == np.float32 and kept.shape[1] == cloud.shape[1]
        frames[name] = dict(points=cloud, rect=rect, Trv2c=trv2c, P2=p2, image_shape=shape, kept=kept,
                            back=np.array(back), **rec)
        return frames[name]

    for i, n in enumerate(SIZES):
        add(f"a{i}", uniform_cloud(rng, n, 4), gg.calib(rng), (370, 1224) if i in SMALL_IMAGE else (375, 1242))
    for i, n in enumerate([130, 517, 777]):
        add(f"b{i}", uniform_cloud(rng, n, 3), gg.calib(rng), (375, 1242))
    neg = uniform_cloud(rng, 300, 4)
    neg[:, 0] = -np.abs(neg[:, 0]) - 1.0
    add("neg", neg, gg.calib(rng), (375, 1242))
    r = rng.uniform(3, 60, 400)
    cone = np.stack([r, r * rng.uniform(-0.2, 0.2, 400), -0.3 + r * rng.uniform(-0.02, 0.02, 400), rng.uniform(0, 1, 400)],
                    1).astype(np.float32)
    add("cone", cone, gg.calib(rng), (375, 1242))
    odd = uniform_cloud(rng, 200, 4)
    odd[17, 0] = np.nan
    odd[101, 0] = np.inf
    add("odd", odd, gg.calib(rng), (375, 1242))
    a8 = frames["a8"]
    add("back", a8["points"], (a8["rect"], a8["Trv2c"], a8["P2"]), a8["image_shape"], back=True)

    # ---- assertions on the plain frames, and the restatement against the reference ----
    margins = []
    for name, f in frames.items():
        src = f["points"]
        if f["back"]:
            src = src.copy()
            src[:, 0] = -src[:, 0]
        margins.append(plane_margin(src, f["planes"]))
        n, k = len(f["points"]), len(f["kept"])
        if name[0] in "ab" and n >= 63:
            assert 0 < k < n, (name, k, n)
        mine = fru.remove_outside_points_np(f["points"], f["rect"], f["Trv2c"], f["P2"], f["image_shape"], back=bool(f["back"]))
        assert mine.dtype == np.float32 and mine.shape == f["kept"].shape and mine.tobytes() == f["kept"].tobytes(), name
        assert fru.crop_np(f["points"], f["planes"], bool(f["back"])).tobytes() == f["kept"].tobytes(), name
        np.testing.assert_allclose(fru.frustum_planes(f["rect"], f["Trv2c"], f["P2"], f["image_shape"]), f["planes"],
                                   rtol=1e-12, atol=0)
        np.testing.assert_allclose(fru.frustum_corners_lidar(f["rect"], f["Trv2c"], f["P2"], f["image_shape"]),
                                   f["corners"], rtol=1e-12, atol=1e-15)
        C, R, T = fru.projection_matrix_to_CRT_kitti(f["P2"])
        for mine_m, key in ((C, "C"), (R, "R"), (T, "T")):
            np.testing.assert_allclose(mine_m, f[key], rtol=1e-12, atol=1e-15)
    assert len(frames["neg"]["kept"]) == 0 and len(frames["cone"]["kept"]) == len(frames["cone"]["points"])
    odd_kept = frames["odd"]["kept"]
    out["odd__nan_kept"] = np.array(bool(np.isnan(odd_kept[:, 0]).any()))
    out["odd__inf_kept"] = np.array(bool(np.isinf(odd_kept[:, 0]).any()))
    assert min(margins) > 1e-6, min(margins)

    # ---- the labelled frames: crop, then points_in_rbbox, as create_groundtruth_database composes them ----
    infos, clouds = [], []
    differ = 0
    for k in range(3):
        info, p = labelled_frame(rng, k)
        f = add(f"g{k}", p, (info["calib/R0_rect"], info["calib/Tr_velo_to_cam"], info["calib/P2"]), info["img_shape"])
        margins.append(plane_margin(p, f["planes"]))
        annos = info["annos"]
        num_obj = int(np.sum(annos["index"] >= 0))
        cam = np.concatenate([annos["location"], annos["dimensions"], annos["rotation_y"][..., np.newaxis]], axis=1)[:num_obj]
        rbbox_lidar = box_np_ops.box_camera_to_lidar(cam, info["calib/R0_rect"], info["calib/Tr_velo_to_cam"])
        points = f["kept"]
        point_indices = box_np_ops.points_in_rbbox(points, rbbox_lidar)
        objs = []
        for i in range(num_obj):
            gt_points = points[point_indices[:, i]]
            gt_points[:, :3] -= rbbox_lidar[i, :3]
            objs.append(np.array(gt_points))
        counts = point_indices.sum(0)
        raw = box_np_ops.points_in_rbbox(p[:, :3], rbbox_lidar).sum(0)
        differ += int((counts != raw).sum())
        num_ignored = len(annos["dimensions"]) - num_obj
        f["num_points_in_gt"] = np.concatenate([counts, -np.ones([num_ignored])]).astype(np.int32)
        f["num_points_in_gt_raw"] = np.concatenate([raw, -np.ones([num_ignored])]).astype(np.int32)
        f["rbbox_lidar"] = np.array(rbbox_lidar)
        f["obj_points"] = np.concatenate(objs + [np.zeros((0, 4), np.float32)], 0)
        f["obj_offsets"] = np.concatenate([[0], np.cumsum([len(o) for o in objs])]).astype(np.int64)
        f["image_idx"] = np.array(info["image_idx"])
        f["velodyne_path"] = np.array(info["velodyne_path"])
        for key, v in annos.items():
            f[f"anno__{key}"] = np.array(v)
        assert gg.near_face(p, rbbox_lidar, 1e-5) == 0
        assert 0 < len(points) < len(p), k
        infos.append(info)
        clouds.append(p)
    assert differ >= 1, "no box's count changes under the crop"
    assert min(margins) > 1e-6, min(margins)

    # the engine=None database functions against the recorded arrays
    twin = [dict(i, annos=dict(i["annos"])) for i in infos]
    gdb.calculate_num_points_in_gt(None, twin, clouds, remove_outside=True)
    for k, t in enumerate(twin):
        assert np.array_equal(t["annos"]["num_points_in_gt"], frames[f"g{k}"]["num_points_in_gt"]), k
    twin = [dict(i, annos=dict(i["annos"])) for i in infos]
    gdb.calculate_num_points_in_gt(None, twin, clouds)
    for k, t in enumerate(twin):
        assert np.array_equal(t["annos"]["num_points_in_gt"], frames[f"g{k}"]["num_points_in_gt_raw"]), k
    db_infos, db_points = gdb.create_groundtruth_database(None, infos, clouds, used_classes=USED, remove_outside=True)
    n_objects = 0
    for k in range(3):
        f = frames[f"g{k}"]
        for i in range(len(f["rbbox_lidar"])):
            name = str(f["anno__name"][i])
            j = [o["image_idx"] == str(f["image_idx"]) and o["gt_idx"] == i for o in db_infos[name]].index(True)
            ref = f["obj_points"][f["obj_offsets"][i]:f["obj_offsets"][i + 1]]
            assert db_points[name][j].tobytes() == ref.tobytes() and db_infos[name][j]["num_points_in_gt"] == len(ref), (k, i)
            assert np.array_equal(db_infos[name][j]["box3d_lidar"], f["rbbox_lidar"][i])
            n_objects += 1
    tmp = tempfile.mkdtemp()
    for back in (False, True):
        kept = gdb.create_reduced_point_cloud(None, infos, clouds, tmp, back=back)
        for k, info in enumerate(infos):
            path = os.path.join(tmp, os.path.basename(info["velodyne_path"]) + ("_back" if back else ""))
            got = np.fromfile(path, np.float32).reshape(-1, 4)
            assert len(got) == kept[k]
            if not back:
                assert got.tobytes() == frames[f"g{k}"]["kept"].tobytes(), k

    for name, f in frames.items():
        for key, v in f.items():
            out[f"{name}__{key}"] = v
    out["frames"] = np.array(list(frames))
    path = os.path.join(ROOT, "tests", "golden", "ref_frustum.npz")
    np.savez_compressed(path, **out)
    print("frames", {n: (len(f["points"]), len(f["kept"])) for n, f in frames.items()}, "objects", n_objects,
          "counts changed by the crop", differ, "smallest plane margin", min(margins), "odd: nan kept",
          bool(out["odd__nan_kept"]), "inf kept", bool(out["odd__inf_kept"]), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
