"""Live-camera ingest in front of the hot path (the part that needs no ROS).

The reference's production mode (load_data.py:2433-2444) takes a sensor_msgs/PointCloud2 from the RealSense d435i,
keeps every 4th point starting at index 1, rotates camera axes into lidar axes and lifts the cloud by 1 m:

    r  = R.from_euler('y', -90, degrees=True).as_dcm()      # scipy Rotation (as_dcm is today's as_matrix)
    r2 = R.from_euler('x',  90, degrees=True).as_dcm()
    points = np.dot(np.dot(points, r), r2) + [0.0, 0.0, 1.0]

`ros_numpy` / `rospy` are not available here: `pointcloud2_to_xyz` restates what
`ros_numpy.point_cloud2.pointcloud2_to_xyz_array` does with a sensor_msgs/PointCloud2 (third-party dependency of the
reference, not vendored: eric-wieser/ros_numpy, `point_cloud2.py` -- fields -> structured dtype with the message's
offsets, one record per `point_step` bytes, rows of `row_step` bytes, NaN points dropped, x y z stacked) on the
message's plain attributes, so the rest of this module starts from the [N,3] xyz array either way.  `realsense_to_lidar64` evaluates the reference's expression itself --
same scipy matrices (their cos(90 deg) entries are 6.1e-17, not 0), same two float64 products, same addition --
and is bit-identical to it.  `realsense_to_lidar` hands the engine float32 points (the voxeliser's input type):

  * x_lidar = z_cam and y_lidar = -x_cam are float32 values to begin with (the 6e-17-weighted terms vanish in the
    cast), so their cells are the reference's;
  * z_lidar = -y_cam + 1.0 is rounded to float32, which can move a point across a voxel edge only if the float64
    value lies within half a float32 ulp of it: for the shipped grid (z edges at -3, 1, 5) that is 0 < y_cam < 3e-8
    or y_cam within 1.2e-7 of 4 -- values a depth camera does not produce.  `cells_agree` checks a cloud for it.

The functions above are the host restatement and the yardstick.  The live path itself runs on the GPU
(`Engine.ingest_pointcloud2` / `detect_pointcloud2`, csrc/ingest.hip): `layout_of` describes a message to it,
`kept_bound` sizes what follows, and `select_np` + `transform_ordered64` state its per-record rule -- one exclusive scan
of the finite flags for NaN removal and decimation together, the two products summed left to right without fused
multiply-adds -- which `ingest_np` assembles; the tests hold all of them to `realsense_to_lidar(pointcloud2_to_xyz(...))`
bit for bit.
"""
import numpy as np

SENSOR_HEIGHT = 1.0

# sensor_msgs/PointField datatype codes -> numpy (INT8 1 ... FLOAT64 8)
_PF_TYPES = {1: "i1", 2: "u1", 3: "i2", 4: "u2", 5: "i4", 6: "u4", 7: "f4", 8: "f8"}


def _parse(data, width, height, point_step, row_step, fields, is_bigendian=False):
    """The checks and the structured dtype of one message: (dtype of a record, width, height, row_step, byte view)."""
    fl = sorted(((str(n), int(o), int(t), int(c)) for n, o, t, c in fields), key=lambda f: f[1])
    names = {f[0] for f in fl}
    if not {"x", "y", "z"} <= names:
        raise ValueError(f"PointCloud2 without x/y/z fields: {sorted(names)}")
    order = ">" if is_bigendian else "<"
    spec = {"names": [], "formats": [], "offsets": [], "itemsize": int(point_step)}
    for name, off, typ, cnt in fl:
        if typ not in _PF_TYPES:
            raise ValueError(f"PointField {name}: unknown datatype {typ}")
        base = np.dtype(order + _PF_TYPES[typ])
        if off + base.itemsize * max(cnt, 1) > point_step:
            raise ValueError(f"PointField {name} (offset {off}) does not fit point_step {point_step}")
        spec["names"].append(name)
        spec["formats"].append(base if cnt <= 1 else (base, (cnt,)))
        spec["offsets"].append(off)
    dt = np.dtype(spec)
    width, height, row_step = int(width), int(height), int(row_step)
    if row_step < width * point_step:
        raise ValueError(f"row_step {row_step} < width {width} x point_step {point_step}")
    buf = np.frombuffer(data, dtype=np.uint8)
    if buf.size < height * row_step:
        raise ValueError(f"PointCloud2 data holds {buf.size} bytes, {height} rows of {row_step} needed")
    return dt, fl, width, height, row_step, buf


def pointcloud2_to_xyz(data, width, height, point_step, row_step, fields, is_bigendian=False, remove_nans=True):
    """sensor_msgs/PointCloud2 -> [N,3] array of its x y z fields (their own dtype, float32 for the d435i), what
    `ros_numpy.point_cloud2.pointcloud2_to_xyz_array(msg)` returns (load_data.py:2433).

    data: the message's byte buffer; fields: iterable of (name, offset, datatype, count) -- `(f.name, f.offset,
    f.datatype, f.count)` of `msg.fields`.  Points with a non-finite coordinate are dropped (remove_nans), in
    message order (row-major over height x width), as ros_numpy does."""
    dt, _, width, height, row_step, buf = _parse(data, width, height, point_step, row_step, fields, is_bigendian)
    rows = buf[:height * row_step].reshape(height, row_step)[:, :width * point_step]
    rec = np.ascontiguousarray(rows).reshape(-1).view(dt)            # height * width records, row-major
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=-1)
    if remove_nans:
        xyz = xyz[np.isfinite(xyz).all(axis=1)]
    return xyz


def as_tuple(msg):
    """A message as the argument tuple of `pointcloud2_to_xyz`: (data, width, height, point_step, row_step, fields,
    is_bigendian).  msg: that tuple already (is_bigendian optional), or any object with those attributes -- a
    sensor_msgs/PointCloud2, whose `fields` are objects with name / offset / datatype / count (ROS is not imported)."""
    if isinstance(msg, (tuple, list)):
        if len(msg) not in (6, 7):
            raise ValueError(f"a PointCloud2 tuple has 6 or 7 entries (data, width, height, point_step, row_step, fields"
                             f"[, is_bigendian]), got {len(msg)}")
        t = tuple(msg) + ((False,) if len(msg) == 6 else ())
    else:
        t = (msg.data, msg.width, msg.height, msg.point_step, msg.row_step, msg.fields, getattr(msg, "is_bigendian", False))
    fields = [tuple(f) if isinstance(f, (tuple, list)) else (f.name, f.offset, f.datatype, getattr(f, "count", 1))
              for f in t[5]]
    return (t[0], int(t[1]), int(t[2]), int(t[3]), int(t[4]), fields, bool(t[6]))


LAYOUT_KEYS = ("width", "height", "point_step", "row_step", "x_offset", "y_offset", "z_offset", "datatype", "is_bigendian")


def layout_of(msg):
    """The pp_pc2_layout fields of a message (`as_tuple` says what a message is) as a dict -- what the GPU ingest needs
    besides the bytes.  Raises the ValueErrors of `pointcloud2_to_xyz`.  `datatype` is the PointField code of x, y and z
    when they agree, else x | y << 8 | z << 16, which the C-ABI refuses (as it refuses the integer codes 1..6)."""
    data, width, height, point_step, row_step, fields, big = as_tuple(msg)
    _, fl, width, height, row_step, _ = _parse(data, width, height, point_step, row_step, fields, big)
    by = {f[0]: f for f in fl}
    tx, ty, tz = (by[k][2] for k in "xyz")
    return {"width": width, "height": height, "point_step": int(point_step), "row_step": row_step,
            "x_offset": by["x"][1], "y_offset": by["y"][1], "z_offset": by["z"][1],
            "datatype": tx if tx == ty == tz else tx | ty << 8 | tz << 16, "is_bigendian": int(big)}


def kept_bound(width, height, first=1, decimate=4):
    """Most points a width x height message can keep: max(0, ceil((width * height - first) / decimate)) -- the host-side
    size of everything behind the GPU ingest, whose true counts exist on the device only."""
    if decimate < 1:
        raise ValueError(f"decimate {decimate} < 1")
    if first < 0:
        raise ValueError(f"first {first} < 0")
    n = int(width) * int(height) - int(first)
    return max(0, -(-n // int(decimate)))


def select_np(finite, first=1, decimate=4):
    """The GPU ingest's selection rule in numpy: finite [n] bool, one flag per record in message order -> the indices
    of the kept records, in output order.  rank = finite records in front of a record (one exclusive scan); it is kept
    when finite, rank >= first and (rank - first) % decimate == 0, as output row (rank - first) / decimate -- NaN removal
    followed by [first::decimate], in one pass."""
    if decimate < 1:
        raise ValueError(f"decimate {decimate} < 1")
    if first < 0:
        raise ValueError(f"first {first} < 0")
    fin = np.asarray(finite, bool).reshape(-1)
    rank = np.cumsum(fin) - fin
    return np.flatnonzero(fin & (rank >= first) & ((rank - first) % decimate == 0))


def _matrices():
    from scipy.spatial.transform import Rotation as R
    r = R.from_euler('y', -90, degrees=True)
    r2 = R.from_euler('x', 90, degrees=True)
    as_m = "as_matrix" if hasattr(r, "as_matrix") else "as_dcm"
    return getattr(r, as_m)(), getattr(r2, as_m)()


def realsense_to_lidar64(points_xyz, decimate=4, first=1, lift=SENSOR_HEIGHT):
    """The reference's arithmetic, float64 out (load_data.py:2434-2443)."""
    p = np.asarray(points_xyz)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"expected an [N,3] xyz array, got {p.shape}")
    r, r2 = _matrices()
    pts = p[first::decimate]
    pts = np.dot(pts, r)
    pts = np.dot(pts, r2)
    return pts + [0.0, 0.0, lift]


def realsense_to_lidar(points_xyz, decimate=4, first=1, lift=SENSOR_HEIGHT, dtype=np.float32):
    """[N,3] camera-frame points -> [ceil((N-first)/decimate),3] lidar-frame points (x depth, y left, z up),
    ready for `Engine.detect` / `points_to_voxel` (float32 like every cloud the hot path takes)."""
    return realsense_to_lidar64(points_xyz, decimate, first, lift).astype(dtype)


def cells_agree(points64, voxel_size, pc_range):
    """True when the float32 cast of `points64` falls into the same voxels as the float64 values (the reference
    voxelises the float64 array): floor((p - min) / size) evaluated as load_data.py:622 does, both ways."""
    vs, lo = np.asarray(voxel_size, np.float64), np.asarray(pc_range, np.float64)[:3]
    c64 = np.floor((np.asarray(points64, np.float64) - lo) / vs)
    c32 = np.floor((np.asarray(points64).astype(np.float32).astype(np.float64) - lo) / vs)
    return bool(np.array_equal(c64, c32))


def transform_ordered64(points_xyz, lift=SENSOR_HEIGHT, matrices=None):
    """((p . r) . r2) + [0, 0, lift] in float64 with every 3-term dot product summed left to right, products and sums
    rounded separately (no fused multiply-add): the GPU ingest's arithmetic, restated.  Bit-identical to
    `realsense_to_lidar64(points, decimate=1, first=0)` wherever numpy's dot sums a row of three in that order (the
    kernel's contract is this function)."""
    p = np.asarray(points_xyz).astype(np.float64).reshape(-1, 3)
    r, r2 = _matrices() if matrices is None else matrices
    out = p
    for m in (np.asarray(r, np.float64), np.asarray(r2, np.float64)):
        out = np.stack([(out[:, 0] * m[0, j] + out[:, 1] * m[1, j]) + out[:, 2] * m[2, j] for j in range(3)], axis=-1)
    return out + np.array([0.0, 0.0, lift])


def ingest_np(msg, first=1, decimate=4, lift=SENSOR_HEIGHT):
    """What the GPU ingest computes for one message, on the host by its own rule: records -> finite flags -> `select_np`
    -> `transform_ordered64` -> float32.  Returns (points [kept, 3] float32, finite count)."""
    xyz = pointcloud2_to_xyz(*as_tuple(msg), remove_nans=False)
    fin = np.isfinite(xyz).all(axis=1)
    keep = select_np(fin, first, decimate)
    return transform_ordered64(xyz[keep], lift).astype(np.float32), int(fin.sum())
