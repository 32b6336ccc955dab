"""The frustum crop on the host (frustum.py): the restatement against tests/golden/ref_frustum.npz -- what the reference's
remove_outside_points kept of the same clouds (tools/gen_golden_frustum.py) --, the planes, the on-the-face rule, the
reduced-cloud files, the database functions with remove_outside=True, and the C-ABI's declarations."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

ANNO_KEYS = ("name", "location", "dimensions", "rotation_y", "bbox", "difficulty", "index")
# hand-made planes: the face x = 2 (inside: x < 2) and five faces far away
FACE_PLANES = np.array([[1, 0, 0, -2], [-1, 0, 0, -1e6], [0, 1, 0, -1e6], [0, -1, 0, -1e6], [0, 0, 1, -1e6],
                        [0, 0, -1, -1e6]], np.float64)


def fixture_frames():
    """(G, {name: dict of the frame's arrays}) of ref_frustum.npz."""
    G = load_golden("ref_frustum.npz")
    frames = {}
    for name in G["frames"].tolist():
        frames[name] = {k[len(name) + 2:]: v for k, v in G.items() if k.startswith(name + "__")}
    return G, frames


def labelled_dataset(frames):
    """The labelled frames g0..g2 as kitti-info dicts (without num_points_in_gt) and float32 clouds."""
    infos, clouds = [], []
    for k in range(3):
        f = frames[f"g{k}"]
        infos.append({"image_idx": str(f["image_idx"]), "velodyne_path": str(f["velodyne_path"]), "img_shape": f["image_shape"],
                      "calib/R0_rect": f["rect"], "calib/Tr_velo_to_cam": f["Trv2c"], "calib/P2": f["P2"],
                      "annos": {key: f[f"anno__{key}"] for key in ANNO_KEYS}})
        clouds.append(f["points"])
    return infos, clouds


def face_cloud(F):
    """Three points around the face x = 2: on it (removed), one float32 step inside (kept), one step outside (removed)."""
    two = np.float32(2.0)
    x = np.array([two, np.nextafter(two, np.float32(0)), np.nextafter(two, np.float32(3))], np.float32)
    p = np.zeros((3, F), np.float32)
    p[:, 0] = x
    p[:, 1:] = np.arange(3 * (F - 1), dtype=np.float32).reshape(3, F - 1) / 8
    return p


def check_objects(frames, db_infos, db_points):
    """create_groundtruth_database(remove_outside=True) against the recorded objects; returns how many were checked."""
    n = 0
    for k in range(3):
        f = frames[f"g{k}"]
        for i in range(len(f["rbbox_lidar"])):
            name = str(f["anno__name"][i])
            j = [o["image_idx"] == str(f["image_idx"]) and o["gt_idx"] == i for o in db_infos[name]].index(True)
            ref = f["obj_points"][f["obj_offsets"][i]:f["obj_offsets"][i + 1]]
            got = db_points[name][j]
            assert got.dtype == np.float32 and got.shape == ref.shape and got.tobytes() == ref.tobytes(), (k, i)
            assert db_infos[name][j]["num_points_in_gt"] == len(ref) == f["num_points_in_gt"][i]
            assert np.array_equal(db_infos[name][j]["box3d_lidar"], f["rbbox_lidar"][i])
            n += 1
    return n


def test_fixture_names_its_producers_and_frames():
    G, frames = fixture_frames()
    made = set(G["produced_by"].tolist())
    assert {"second.core.box_np_ops.remove_outside_points", "second.core.geometry.surface_equ_3d_jit",
            "second.core.box_np_ops.points_in_rbbox"} <= made
    assert [len(frames[f"a{i}"]["points"]) for i in range(10)] == [0, 1, 63, 64, 65, 255, 256, 257, 1000, 3000]
    assert all(frames[f"a{i}"]["points"].shape[1] == 4 for i in range(10))
    assert all(frames[f"b{i}"]["points"].shape[1] == 3 for i in range(3))
    assert sorted(tuple(frames[f"a{i}"]["image_shape"]) for i in range(10)).count((370, 1224)) == 2
    assert len(frames["neg"]["kept"]) == 0 and len(frames["cone"]["kept"]) == len(frames["cone"]["points"]) > 0
    odd = frames["odd"]["points"]
    assert np.isnan(odd[:, 0]).sum() == 1 and np.isinf(odd[:, 0]).sum() == 1
    # what the reference did with them: the NaN point is kept, the +inf point is not
    assert bool(G["odd__nan_kept"]) and not bool(G["odd__inf_kept"])


def test_restatement_equals_reference_bytes(pp):
    fru = pp.frustum
    _, frames = fixture_frames()
    kept = removed = 0
    for name, f in frames.items():
        back = bool(f["back"])
        got = fru.remove_outside_points_np(f["points"], f["rect"], f["Trv2c"], f["P2"], f["image_shape"], back=back)
        assert got.dtype == np.float32 and got.shape == f["kept"].shape and got.tobytes() == f["kept"].tobytes(), name
        # ... and from the recorded planes (what the device is given)
        assert fru.crop_np(f["points"], f["planes"], back).tobytes() == f["kept"].tobytes(), name
        kept += len(got)
        removed += len(f["points"]) - len(got)
    assert kept > 5000 and removed > 3000
    assert len(frames["back"]["kept"]) > 0 and (frames["back"]["kept"][:, 0] > 0).all()
    assert (frames["back"]["points"][:, 0] < 0).sum() >= len(frames["back"]["kept"])
    nan_rows = np.isnan(frames["odd"]["kept"][:, 0])
    assert nan_rows.sum() == 1
    with pytest.raises(ValueError, match="float32"):
        fru.keep_mask(np.zeros((2, 3), np.float64), FACE_PLANES)


def test_planes_equal_reference(pp):
    fru = pp.frustum
    _, frames = fixture_frames()
    for name, f in frames.items():
        C, R, T = fru.projection_matrix_to_CRT_kitti(f["P2"])
        for got, key in ((C, "C"), (R, "R"), (T, "T")):
            np.testing.assert_allclose(got, f[key], rtol=1e-12, atol=1e-15, err_msg=f"{name} {key}")
        np.testing.assert_allclose(fru.frustum_corners_lidar(f["rect"], f["Trv2c"], f["P2"], f["image_shape"]), f["corners"],
                                   rtol=1e-12, atol=1e-15, err_msg=name)
        planes = fru.frustum_planes(f["rect"], f["Trv2c"], f["P2"], f["image_shape"])
        assert planes.shape == (6, 4) and planes.dtype == np.float64
        np.testing.assert_allclose(planes, f["planes"], rtol=1e-12, atol=0, err_msg=name)
        np.testing.assert_allclose(fru.corner_planes(f["corners"]), f["planes"], rtol=1e-12, atol=0, err_msg=name)
    norms = np.linalg.norm(frames["a9"]["planes"][:, :3], axis=1)
    assert norms.min() < 1e-5 and norms.max() > 1e3          # the normals are used as they come: not unit length


@pytest.mark.parametrize("F", [3, 4])
def test_point_on_a_face_is_removed(pp, F):
    p = face_cloud(F)
    assert p[0, 0] == 2.0 and p[1, 0] < 2.0 < p[2, 0]
    assert pp.frustum.keep_mask(p, FACE_PLANES).tolist() == [False, True, False]
    assert pp.frustum.crop_np(p, FACE_PLANES).tobytes() == p[1:2].tobytes()
    nan = p.copy()
    nan[:, 1] = np.nan
    assert pp.frustum.keep_mask(nan, FACE_PLANES).all()      # !(s >= 0): a NaN survives every face


def test_reduced_point_cloud_files(pp, tmp_path):
    gdb = pp.gt_database
    _, frames = fixture_frames()
    infos, clouds = labelled_dataset(frames)
    kept = gdb.create_reduced_point_cloud(None, infos, clouds, tmp_path / "velodyne_reduced")
    assert kept.dtype == np.int32 and kept.tolist() == [len(frames[f"g{k}"]["kept"]) for k in range(3)]
    for k in range(3):
        path = tmp_path / "velodyne_reduced" / f"{k:06d}.bin"
        assert path.read_bytes() == frames[f"g{k}"]["kept"].tobytes()
    # the `_back` files: the name, and the frame recorded with back=True
    a8, back = frames["a8"], frames["back"]
    info = {"velodyne_path": "training/velodyne/000008.bin", "img_shape": a8["image_shape"], "calib/R0_rect": a8["rect"],
            "calib/Tr_velo_to_cam": a8["Trv2c"], "calib/P2": a8["P2"]}
    src = a8["points"].copy()
    kept = gdb.create_reduced_point_cloud(None, [info], [src], tmp_path, back=True)
    assert kept.tolist() == [len(back["kept"])]
    assert (tmp_path / "000008.bin_back").read_bytes() == back["kept"].tobytes()
    assert src.tobytes() == a8["points"].tobytes()           # the caller's cloud is not negated in place
    with pytest.raises(ValueError, match="differ in length"):
        gdb.create_reduced_point_cloud(None, infos, clouds[:2], tmp_path)


def test_database_functions_with_remove_outside(pp):
    gdb = pp.gt_database
    _, frames = fixture_frames()
    infos, clouds = labelled_dataset(frames)
    gdb.calculate_num_points_in_gt(None, infos, clouds, remove_outside=True)
    changed = 0
    for k, info in enumerate(infos):
        got = info["annos"]["num_points_in_gt"]
        assert got.dtype == np.int32 and np.array_equal(got, frames[f"g{k}"]["num_points_in_gt"]), k
        changed += int((got != frames[f"g{k}"]["num_points_in_gt_raw"]).sum())
    assert changed >= 1                                      # boxes across the frustum's side faces lose points
    gdb.calculate_num_points_in_gt(None, infos, clouds)      # the default: no crop, as before
    for k, info in enumerate(infos):
        assert np.array_equal(info["annos"]["num_points_in_gt"], frames[f"g{k}"]["num_points_in_gt_raw"]), k
    db_infos, db_points = gdb.create_groundtruth_database(None, infos, clouds, used_classes=["Pedestrian", "Cyclist"],
                                                          remove_outside=True)
    assert check_objects(frames, db_infos, db_points) == 8


def test_header_declares_the_crop(pp):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    for sym in ("pp_frustum_crop", "pp_frustum_crop_async", "pp_frustum_crop_info"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in pp._lib.EXPORTS, sym
    m = re.search(r"#define\s+PP_CROP_BACK\s+(\d+)", hdr)
    assert m and int(m.group(1)) == pp._lib.PP_CROP_BACK == 1
    assert re.search(r"#define\s+PP_ABI_VERSION\s+4\b", hdr)
    assert "frustum_crop.hip" in pp._lib.SOURCES and "api_crop.hip" in pp._lib.SOURCES
