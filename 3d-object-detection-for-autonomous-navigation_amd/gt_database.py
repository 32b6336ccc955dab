"""Building the ground-truth object database from labelled frames: the reference's
create_groundtruth_database (create_data.py:365-551) and _calculate_num_points_in_gt (create_data.py:28-93).

Both are one computation -- every point of a frame against every labelled box of that frame:
  1. the frame's camera boxes [x y z l h w r] become lidar boxes [x y z w l h r] on the host (`box_camera_to_lidar`:
     the reference's numpy calls, np.linalg.inv((rect @ trv2c).T) among them; at most 256 boxes per frame, and a LAPACK
     inverse is nothing to reproduce bit for bit on a GPU -- so the device takes lidar boxes);
  2. a point is inside a box iff ((x n0 + y n1) + z n2) + d < 0 for all six faces, in float64 on the widened float32
     coordinates, the planes as augment.box_planes builds them (points_in_rbbox's); a point inside several boxes goes to
     each of them;
  3. an object's points are the frame's members in the frame's order (points[point_indices[:, i]]), x y z stored as
     (float)((double)p - centre): `gt_points[:, :3] -= rbbox_lidar[i, :3]` on a float32 array, one rounding; the other
     columns are copied;
  4. num_points_in_gt is the member count; _calculate_num_points_in_gt counts over the first num_obj (non-DontCare)
     boxes and writes -1 for the rest.
Steps 2-4 run on the GPU over the frames resident in an Engine (csrc/gt_database.hip: Engine.build_gt_objects /
count_points_in_gt); `build_objects_np` is their float64 host restatement, pinned by tests/golden/ref_gt_database.npz,
which tools/gen_golden_gtdb.py produces by running the reference's own functions.  Passing `engine=None` to the
dataset-level functions below runs that restatement instead -- a choice the caller spells out, for machines without a
GPU and for the tests' oracle; an Engine never falls back to it.

The frustum crop (box_np_ops.remove_outside_points; frustum.py states the rule, csrc/frustum_crop.hip runs it): the
reference applies it to KITTI clouds before steps 2-4 and skips it for the custom dataset (custom_dataset = True, the
shipped configuration).  Here it is `remove_outside=True`, off by default; with an Engine the uploaded batch is cropped
on the GPU (Engine.crop_to_image) and the count / build runs on the cropped frames.  `create_reduced_point_cloud` writes
the cropped clouds as _create_reduced_point_cloud (create_data.py:275-323) names them.
"""
import itertools
import pathlib
import pickle

import numpy as np

from . import augment, frustum

PP_MAX_GT_PER_FRAME = 256
# kitti_common.get_classes() without DontCare: the default used_classes
KITTI_CLASSES = ("Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "Truck", "Tram", "Misc")


def box_camera_to_lidar(boxes_cam, rect, trv2c):
    """box_np_ops.box_camera_to_lidar (load_data.py:1498): camera boxes [n, 7] x y z l h w r -> lidar boxes x y z w l h r,
    the centres through np.linalg.inv((rect @ trv2c).T) as camera_to_lidar does it."""
    data = np.asarray(boxes_cam)
    if data.ndim != 2 or data.shape[1] != 7:
        raise ValueError(f"boxes_cam: expected [n, 7], got {data.shape}")
    xyz = data[:, 0:3]
    l, h, w = data[:, 3:4], data[:, 4:5], data[:, 5:6]
    r = data[:, 6:7]
    pts = np.concatenate([xyz, np.ones(list(xyz.shape[0:-1]) + [1])], axis=-1)
    xyz_lidar = (pts @ np.linalg.inv((np.asarray(rect) @ np.asarray(trv2c)).T))[..., :3]
    return np.concatenate([xyz_lidar, w, l, h, r], axis=1)


def _check_cloud(points, F=None, what="cloud"):
    p = np.asarray(points)
    if p.dtype != np.float32:
        raise ValueError(f"{what}: points must be float32 (the engine holds float32 points), got {p.dtype}")
    if p.ndim != 2 or p.shape[1] < 3 or (F is not None and p.shape[1] != F):
        raise ValueError(f"{what}: points must be [n, {F if F is not None else 'F >= 3'}], got {p.shape}")
    return p


def _check_boxes(boxes, what="boxes"):
    b = np.ascontiguousarray(boxes, np.float64).reshape(-1, 7)
    if len(b) > PP_MAX_GT_PER_FRAME:
        raise ValueError(f"{what}: {len(b)} boxes in a frame, at most {PP_MAX_GT_PER_FRAME}")
    if not np.isfinite(b).all():
        raise ValueError(f"{what}: a box is not finite")
    if (b[:, 3:6] <= 0).any():
        raise ValueError(f"{what}: a box has a size <= 0")
    return b


def build_objects_np(points, boxes):
    """One frame on the host, in float64: points [n, F] float32, boxes [G, 7] float64 lidar boxes.  Returns (counts [G]
    int32, [G float32 arrays [counts[i], F]]): what create_groundtruth_database writes per object."""
    p = _check_cloud(points)
    b = _check_boxes(boxes)
    if len(b) == 0:
        return np.zeros(0, np.int32), []
    n, d = augment.box_planes(b)
    inside = np.zeros((len(p), len(b)), bool)
    slab = max(64, 1000000 // len(b))          # [slab, G, 6] plane values at a time
    for s in range(0, len(p), slab):
        inside[s:s + slab] = (augment.face_sign(p[s:s + slab, :3].astype(np.float64), n, d) < 0).all(-1)
    objs = []
    for i in range(len(b)):
        g = p[inside[:, i]]                     # (a copy)
        g[:, :3] -= b[i, :3]
        objs.append(g)
    return inside.sum(0).astype(np.int32), objs


def frame_boxes(info, bev_only=False, coors_range=None):
    """create_groundtruth_database's rbbox_lidar of one info: the first num_obj = sum(index >= 0) annotations."""
    annos = info["annos"]
    n_all = len(annos["name"])
    for k in ("location", "dimensions", "rotation_y", "index", "difficulty"):
        if len(annos[k]) != n_all:
            raise ValueError(f"info {info.get('image_idx')!r}: {n_all} names but {len(annos[k])} entries of {k!r}")
    num_obj = int(np.sum(np.asarray(annos["index"]) >= 0))
    cam = np.concatenate([annos["location"], annos["dimensions"], np.asarray(annos["rotation_y"])[..., np.newaxis]],
                         axis=1)[:num_obj]
    lidar = box_camera_to_lidar(cam, info["calib/R0_rect"], info["calib/Tr_velo_to_cam"])
    if bev_only:
        if coors_range is None:
            raise ValueError("bev_only needs coors_range (z and h are set to its limits)")
        lidar[:, 2] = coors_range[2]
        lidar[:, 5] = coors_range[5] - coors_range[2]
    return lidar


def _pairs(infos, clouds):
    """(info, cloud) pairs; infos and clouds must have the same length."""
    miss = object()
    for k, (info, cloud) in enumerate(itertools.zip_longest(infos, clouds, fillvalue=miss)):
        if info is miss or cloud is miss:
            raise ValueError(f"infos and clouds differ in length (frame {k} has no {'info' if info is miss else 'cloud'})")
        yield info, cloud


def _batches(engine, items):
    """Items `max_batch` at a time (engine None: one at a time)."""
    size = engine.max_batch if engine is not None else 1
    it = iter(items)
    while True:
        chunk = list(itertools.islice(it, size))
        if not chunk:
            return
        yield chunk


class _Feeder:
    """Two page-locked staging buffers, used alternately: while the host unpacks the objects of batch k, the copy of
    batch k + 1 is already under way on the engine's copy stream (Engine.upload_async); the next build waits for it on
    the device."""

    def __init__(self, engine):
        self.engine, self.st, self.k = engine, [None, None], 0

    def upload(self, clouds):
        from .engine import Staging
        eng = self.engine
        F = eng.d.num_point_features
        offs = np.zeros(len(clouds) + 1, np.int32)
        offs[1:] = np.cumsum([len(c) for c in clouds])
        need = max(int(offs[-1]) * F * 4, 4)
        st = self.st[self.k]
        if st is None or st.array.nbytes < need:
            st = self.st[self.k] = Staging(eng._lib, need)
        st.points = st.array[:int(offs[-1]) * F].reshape(int(offs[-1]), F)
        for b, c in enumerate(clouds):
            st.points[offs[b]:offs[b + 1]] = c
        st.offsets = offs
        eng.upload_async(st)
        self.k ^= 1


def _run(engine, frames, want_points):
    """frames: iterable of (cloud, lidar boxes, frustum planes or None).  Yields per frame (counts, objects or None),
    `max_batch` frames per device call, the next batch's upload queued before the current one is unpacked.  Planes: the
    frame is cropped to them first (all frames of a run, or none)."""
    if engine is None:
        for cloud, boxes, planes in frames:
            counts, objs = build_objects_np(cloud if planes is None else frustum.crop_np(cloud, planes), boxes)
            yield counts, (objs if want_points else None)
        return
    F = engine.d.num_point_features
    feeder = _Feeder(engine)
    pending = None
    for chunk in itertools.chain(_batches(engine, frames), [None]):
        if chunk is not None:
            chunk = [(_check_cloud(c, F), _check_boxes(b), pl) for c, b, pl in chunk]
        if pending is not None:
            boxes = [b for _, b, _ in pending]
            if pending[0][2] is not None:
                engine.crop_to_image(np.stack([pl for _, _, pl in pending]))
            if want_points:
                counts, objs = engine.build_gt_objects(boxes, return_counts=True)
            else:
                counts, objs = engine.count_points_in_gt(boxes), [None] * len(boxes)
            if chunk is not None:
                feeder.upload([c for c, _, _ in chunk])
            yield from zip(counts, objs)
        elif chunk is not None:
            feeder.upload([c for c, _, _ in chunk])
        pending = chunk


def calculate_num_points_in_gt(engine, infos, clouds, remove_outside=False):
    """_calculate_num_points_in_gt (create_data.py:28-93): fills info["annos"]["num_points_in_gt"] (int32) of every info --
    the points inside each of the first num_obj (names other than DontCare) boxes, -1 for the rest.  clouds: float32
    [n, F] arrays parallel to infos.  remove_outside: count after the frustum crop (info["img_shape"], calib/P2; the
    reference's default for KITTI is True, the custom dataset's and this function's False).  engine None: on the host
    (build_objects_np, frustum.crop_np)."""
    infos = list(infos)

    def frames():
        for info, cloud in _pairs(infos, clouds):
            annos = info["annos"]
            num_obj = len([n for n in annos["name"] if n != "DontCare"])
            cam = np.concatenate([annos["location"][:num_obj], annos["dimensions"][:num_obj],
                                  np.asarray(annos["rotation_y"])[:num_obj][..., np.newaxis]], axis=1)
            yield (_check_cloud(cloud), box_camera_to_lidar(cam, info["calib/R0_rect"], info["calib/Tr_velo_to_cam"]),
                   frustum.info_planes(info) if remove_outside else None)

    for k, (counts, _) in enumerate(_run(engine, frames(), False)):
        annos = infos[k]["annos"]
        num_ignored = len(annos["dimensions"]) - len(counts)
        annos["num_points_in_gt"] = np.concatenate([counts, -np.ones([num_ignored])]).astype(np.int32)


def create_groundtruth_database(engine, infos, clouds, used_classes=None, bev_only=False, coors_range=None,
                                database_name="gt_database", remove_outside=False):
    """create_groundtruth_database (create_data.py:365-551) without the files: returns (all_db_infos, points), the pair
    GtDatabase(infos, points, ...) takes.  all_db_infos[name]: the reference's dicts (name, path, image_idx, gt_idx,
    box3d_lidar, num_points_in_gt, difficulty, group_id, and score when the annotations have one); points[name]: the
    objects' float32 [n, F] arrays, parallel to it.  The group_dict is per frame, the group_counter global; used_classes
    (default: the KITTI classes without DontCare) filters the infos only.  clouds: any iterable of float32 [n, F]
    arrays parallel to infos; frames go through the engine max_batch at a time, the next batch's upload queued while
    the current one is unpacked.  engine None: on the host (build_objects_np).  remove_outside: every cloud is cropped
    to its image's frustum first (info["img_shape"], calib/P2), as the reference does for KITTI; off by default."""
    infos = list(infos)
    if bev_only and coors_range is None:
        raise ValueError("bev_only needs coors_range (z and h are set to its limits)")
    used_classes = list(KITTI_CLASSES if used_classes is None else used_classes)
    all_db_infos = {name: [] for name in used_classes}
    points = {name: [] for name in used_classes}
    lidar = []

    def frames():
        for info, cloud in _pairs(infos, clouds):
            lidar.append(frame_boxes(info, bev_only, coors_range))
            yield _check_cloud(cloud), lidar[-1], (frustum.info_planes(info) if remove_outside else None)

    group_counter = 0
    for k, (counts, objs) in enumerate(_run(engine, frames(), True)):
        info = infos[k]
        annos, rbbox_lidar = info["annos"], lidar[k]
        lidar[k] = None
        names, image_idx = annos["name"], info["image_idx"]
        group_ids = annos["group_ids"] if "group_ids" in annos else np.arange(len(annos["bbox"]), dtype=np.int64)
        group_dict = {}
        for i in range(len(rbbox_lidar)):
            if names[i] not in used_classes:
                continue
            filename = f"{image_idx}_{names[i]}_{annos['index'][i]}.bin"
            db_info = {"name": names[i], "path": database_name + "/" + filename, "image_idx": image_idx,
                       "gt_idx": annos["index"][i], "box3d_lidar": rbbox_lidar[i], "num_points_in_gt": objs[i].shape[0],
                       "difficulty": annos["difficulty"][i]}
            local_group_id = group_ids[i]
            if local_group_id not in group_dict:
                group_dict[local_group_id] = group_counter
                group_counter += 1
            db_info["group_id"] = group_dict[local_group_id]
            if "score" in annos:
                db_info["score"] = annos["score"][i]
            all_db_infos[names[i]].append(db_info)
            points[names[i]].append(objs[i])
    return all_db_infos, points


def create_reduced_point_cloud(engine, infos, clouds, save_dir, back=False):
    """_create_reduced_point_cloud (create_data.py:275-323) with a save path: every cloud cropped to its image's frustum
    and written with `tofile` (raw float32) as save_dir / <name of info["velodyne_path"]>, `_back` appended when `back`
    (x negated first).  Frames go through the engine max_batch at a time, the next batch's upload queued while the
    current one is written.  engine None: on the host (frustum.crop_np).  Returns the kept counts, int32 [len(infos)]."""
    infos = list(infos)
    save_dir = pathlib.Path(save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    F = None if engine is None else engine.d.num_point_features

    def frames():
        for info, cloud in _pairs(infos, clouds):
            yield info, _check_cloud(cloud, F), frustum.info_planes(info)

    def cropped():
        if engine is None:
            for info, cloud, planes in frames():
                yield info, frustum.crop_np(cloud, planes, back)
            return
        feeder = _Feeder(engine)
        pending = None
        for chunk in itertools.chain(_batches(engine, frames()), [None]):
            if pending is not None:
                _, pts = engine.crop_to_image(np.stack([pl for _, _, pl in pending]), back=back, return_points=True)
                if chunk is not None:
                    feeder.upload([c for _, c, _ in chunk])
                yield from zip([i for i, _, _ in pending], pts)
            elif chunk is not None:
                feeder.upload([c for _, c, _ in chunk])
            pending = chunk

    kept = []
    for info, pts in cropped():
        name = pathlib.Path(info["velodyne_path"]).name + ("_back" if back else "")
        np.ascontiguousarray(pts, np.float32).tofile(str(save_dir / name))
        kept.append(len(pts))
    return np.array(kept, np.int32)


def write_reference_files(all_db_infos, points, root, custom_dataset=True, info_name="kitti_dbinfos_train.pkl"):
    """Writes the database in the reference's layout under `root`: `info_name` (the pickled infos) and one file per object
    at the info's path -- for the custom dataset the path with its last three characters replaced by `pkl`, pickle
    protocol 2 (create_data.py:510-511), else the `.bin` itself (raw float32) -- so that GtDatabase.from_reference_files
    and the reference's DataBaseSamplerV2 read them back.  Returns the info file's path."""
    root = pathlib.Path(root)
    for name, objs in all_db_infos.items():
        if len(points[name]) != len(objs):
            raise ValueError(f"{name}: {len(objs)} infos but {len(points[name])} point arrays")
        for o, p in zip(objs, points[name]):
            path = root / o["path"]
            path.parent.mkdir(parents=True, exist_ok=True)
            if custom_dataset:
                with open(str(path)[:-3] + "pkl", "wb") as f:
                    pickle.dump(np.array(p), f, 2)
            else:
                np.ascontiguousarray(p, np.float32).tofile(str(path))
    info_path = root / info_name
    with open(info_path, "wb") as f:
        pickle.dump(all_db_infos, f)
    return info_path
