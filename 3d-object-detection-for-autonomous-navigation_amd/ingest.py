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

A model with more than three point features (x y z intensity: `config.kitti_shaped_config`) is fed from the message's own
fields: `FeatureField` names a field, `feature_layout_of` resolves it against a message, `pointcloud2_to_points` and
`ingest_np(..., features=...)` state the rule -- column j is float32(float64(raw) * scale + bias), validity is x y z's
alone -- and `Engine.ingest_pointcloud2(..., features=...)` runs it on the GPU.

The second half of the module is the same for depth images (`Engine.ingest_depth` / `detect_depth`,
csrc/depth_ingest.hip): the image the camera's point-cloud topic is computed from goes to the GPU instead of the
message, `depth_to_xyz` / `depth_ingest_np` state the rule, and `depth_to_pointcloud2` builds the message it is held to.
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


class FeatureField:
    """One feature column (row entry 3, 4, ...) of a message: the field `name`, element `index` of it when its count is
    above 1, as float32(float64(raw) * scale + bias).  Any PointField datatype (INT8 ... FLOAT64); every integer type and
    float32 widen exactly to float64, the product and the sum are rounded separately in float64 (no fused multiply-add),
    the result is rounded once to float32.  A non-finite value is carried through as it is (NaN as NaN, +-inf as +-inf):
    a record is dropped only when x, y or z is non-finite.  `FeatureField.constant(value)`: a column that reads nothing
    and holds float32(value) -- for a sensor without the field the model was trained with."""

    def __init__(self, name, scale=1.0, bias=0.0, index=0):
        self.name = None if name is None else str(name)
        self.scale, self.bias, self.index = float(scale), float(bias), int(index)
        if not (np.isfinite(self.scale) and np.isfinite(self.bias)):
            raise ValueError(f"FeatureField {name!r}: scale {scale} and bias {bias} must be finite")
        if self.index < 0:
            raise ValueError(f"FeatureField {name!r}: index {index} < 0")

    @classmethod
    def constant(cls, value):
        return cls(None, 1.0, value)

    def __repr__(self):
        if self.name is None:
            return f"FeatureField.constant({self.bias!r})"
        return f"FeatureField({self.name!r}, scale={self.scale!r}, bias={self.bias!r}, index={self.index})"


def _as_feature(f):
    return f if isinstance(f, FeatureField) else FeatureField(*f) if isinstance(f, (tuple, list)) else FeatureField(f)


def feature_layout_of(msg, features):
    """The pp_pc2_feature entries of `features` (FeatureFields, or field names) for ONE message: a list of (offset,
    datatype, scale, bias), datatype 0 for a constant.  offset is the byte offset of the element within a record (field
    offset + index * itemsize).  Raises a ValueError that names the message's fields when a name is missing or index >=
    the field's count."""
    data, width, height, point_step, row_step, fields, big = as_tuple(msg)
    _, fl, _, _, _, _ = _parse(data, width, height, point_step, row_step, fields, big)
    by = {f[0]: f for f in fl}
    have = ", ".join(f"{n} (datatype {t}, count {c})" for n, _, t, c in fl)
    out = []
    for j, f in enumerate(_as_feature(f) for f in features):
        if f.name is None:
            out.append((0, 0, 1.0, f.bias))
            continue
        if f.name not in by:
            raise ValueError(f"feature {j}: the message has no field {f.name!r}; its fields are {have}")
        _, off, typ, cnt = by[f.name]
        if f.index >= max(cnt, 1):
            raise ValueError(f"feature {j}: index {f.index} >= count {max(cnt, 1)} of field {f.name!r}; the message's fields "
                             f"are {have}")
        out.append((off + f.index * np.dtype(_PF_TYPES[typ]).itemsize, typ, f.scale, f.bias))
    return out


def pointcloud2_to_points(msg, features, remove_nans=True):
    """A message (`as_tuple`) -> [N, 3 + len(features)]: x y z as `pointcloud2_to_xyz` gives them, then one column per
    FeatureField, `(rec[name].astype(np.float64) * scale + bias).astype(np.float32)` (a constant: float32(value)).  The
    array has the dtype of x y z (float32 or float64; a float32 feature value is exact in either).  remove_nans drops the
    records whose x, y or z is non-finite, as ros_numpy's remove_nans does; a non-finite FEATURE value stays."""
    t = as_tuple(msg)
    data, width, height, point_step, row_step, fields, big = t
    dt, _, width, height, row_step, buf = _parse(data, width, height, point_step, row_step, fields, big)
    table = feature_layout_of(t, features)          # (raises for a missing name / index)
    rows = buf[:height * row_step].reshape(height, row_step)[:, :width * point_step]
    rec = np.ascontiguousarray(rows).reshape(-1).view(dt)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=-1)
    cols = []
    with np.errstate(all="ignore"):
        for f, (_, typ, scale, bias) in zip((_as_feature(f) for f in features), table):
            if typ == 0:
                cols.append(np.full(len(rec), np.float32(bias), np.float32))
                continue
            raw = rec[f.name]
            raw = raw[:, f.index] if raw.ndim == 2 else raw
            cols.append((raw.astype(np.float64) * scale + bias).astype(np.float32))
    pts = np.concatenate([xyz] + [c.astype(xyz.dtype)[:, None] for c in cols], axis=1) if cols else xyz
    if remove_nans:
        pts = pts[np.isfinite(xyz).all(axis=1)]
    return pts


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
    """((p . r) . r2) + [0, 0, lift] (or + lift, when it is a vector of 3) in float64 with every 3-term dot product summed left to right, products and sums
    rounded separately (no fused multiply-add): the GPU ingest's arithmetic, restated.  Bit-identical to
    `realsense_to_lidar64(points, decimate=1, first=0)` wherever numpy's dot sums a row of three in that order (the
    kernel's contract is this function)."""
    p = np.asarray(points_xyz).astype(np.float64).reshape(-1, 3)
    r, r2 = _matrices() if matrices is None else matrices
    out = p
    for m in (np.asarray(r, np.float64), np.asarray(r2, np.float64)):
        out = np.stack([(out[:, 0] * m[0, j] + out[:, 1] * m[1, j]) + out[:, 2] * m[2, j] for j in range(3)], axis=-1)
    return out + _lift_vector(lift)


def _lift_vector(lift):
    """pp_ingest_config.lift: [0, 0, lift] for a sensor height, or the three numbers themselves."""
    if np.ndim(lift) == 0:
        return np.array([0.0, 0.0, float(lift)])
    v = np.asarray(lift, np.float64).reshape(-1)
    if v.size != 3:
        raise ValueError(f"lift has {v.size} entries, a height or a vector of 3 expected")
    return v


def ingest_np(msg, first=1, decimate=4, lift=SENSOR_HEIGHT, matrices=None, features=None):
    """What the GPU ingest computes for one message, on the host by its own rule: records -> finite flags -> `select_np`
    -> `transform_ordered64` -> float32.  Returns (points [kept, 3] float32, finite count).  matrices: (r, r2) of another
    mount than the reference's (`Mount`); lift may then be a vector of 3.  features: a list of nf `FeatureField`s -- the
    points are then [kept, 3 + nf], the columns behind x y z as `pointcloud2_to_points` gives them for the kept records
    (validity and selection do not look at them; a non-finite feature value is carried through)."""
    if features is None:
        xyz = pointcloud2_to_xyz(*as_tuple(msg), remove_nans=False)
    else:
        full = pointcloud2_to_points(msg, features, remove_nans=False)
        xyz = full[:, :3]
    fin = np.isfinite(xyz).all(axis=1)
    keep = select_np(fin, first, decimate)
    pts = transform_ordered64(xyz[keep], lift, matrices).astype(np.float32)
    if features is not None:
        pts = np.concatenate([pts, full[keep, 3:].astype(np.float32)], axis=1)
    return pts, int(fin.sum())


# ---- depth images (Engine.ingest_depth / detect_depth, csrc/depth_ingest.hip) ---------------------------------------
# The d435i's point-cloud topic is computed on the robot's CPU from a 16-bit depth image a tenth to a sixteenth of its
# size.  The functions below state the rule that takes the image itself to the resident points:
#
#   16UC1 / mono16: z = depth_scale * float32(d), one float32 product; valid when d != 0
#   32FC1:          z is the stored value; valid when it is finite and > 0 (depth_scale is not applied: REP 118)
#   both:           valid only when z > z_min and z <= z_max (0 and +inf leave the conditions above as they are)
#   a valid pixel (v, u) is the float32 point x = z * ((u - ppx) / fx), y = z * ((v - ppy) / fy), z -- every operation
#   rounded separately: the pinhole (no distortion) case of the camera vendor's published rs2_deproject_pixel_to_point
#
# PARITY WITH THE BYTES THE CAMERA DRIVER'S POINT-CLOUD BLOCK PUBLISHES IS NOT PINNED: neither the vendor library nor its
# ROS node is available to this project's tests.  What is pinned is everything behind the point: `depth_ingest_np` (and
# the GPU path) equals `realsense_to_lidar(pointcloud2_to_xyz(*depth_to_pointcloud2(...)), decimate, first, lift)` bit for
# bit.  Not done, and refused by name rather than approximated: lens distortion (`intrinsics_of`), alignment of depth to
# the colour stream, dropping points by texture coordinate, RGB or any feature beyond x y z, the vendor's filters.

DEPTH_ENCODINGS = {"16UC1": ("u2", 0), "mono16": ("u2", 0), "32FC1": ("f4", 1)}     # name -> (numpy type, PP_DEPTH_*)
DEPTH_LAYOUT_KEYS = ("width", "height", "row_step", "encoding", "is_bigendian", "fx", "fy", "ppx", "ppy", "depth_scale",
                     "z_min", "z_max")


def image_as_tuple(msg):
    """A depth image as (data, width, height, step, encoding, is_bigendian).  msg: that tuple already (is_bigendian
    optional), or any object with those attributes -- a sensor_msgs/Image (ROS is not imported)."""
    if isinstance(msg, (tuple, list)):
        if len(msg) not in (5, 6):
            raise ValueError(f"an Image tuple has 5 or 6 entries (data, width, height, step, encoding[, is_bigendian]), "
                             f"got {len(msg)}")
        t = tuple(msg) + ((False,) if len(msg) == 5 else ())
    else:
        t = (msg.data, msg.width, msg.height, msg.step, msg.encoding, getattr(msg, "is_bigendian", False))
    return (t[0], int(t[1]), int(t[2]), int(t[3]), str(t[4]), bool(t[5]))


def intrinsics_of(camera_info):
    """fx, fy, ppx, ppy as float32 (K[0], K[4], K[2], K[5] of the float64 K, cast once).  camera_info: a
    sensor_msgs/CameraInfo (attributes K and D, or k and d), a (K, D) or (K,) tuple with K of 9 entries, or the four
    numbers (fx, fy, ppx, ppy) themselves.  A non-zero distortion coefficient D is refused: the deprojection is the
    pinhole one (the d435i depth stream's coefficients are zero)."""
    K = D = None
    if isinstance(camera_info, (tuple, list, np.ndarray)):
        if len(camera_info) == 4 and all(np.ndim(v) == 0 for v in camera_info):
            fx, fy, ppx, ppy = (np.float32(v) for v in camera_info)
            return fx, fy, ppx, ppy
        if isinstance(camera_info, np.ndarray) or len(camera_info) not in (1, 2):
            K = camera_info
        else:
            K = camera_info[0]
            D = camera_info[1] if len(camera_info) == 2 else None
    else:
        K = getattr(camera_info, "K", None)
        K = getattr(camera_info, "k", None) if K is None else K
        D = getattr(camera_info, "D", None)
        D = getattr(camera_info, "d", None) if D is None else D
        if K is None:
            raise ValueError("intrinsics_of: no K in the camera info")
    K = np.asarray(K, np.float64).reshape(-1)
    if K.size != 9:
        raise ValueError(f"intrinsics_of: K has {K.size} entries, 9 expected")
    if D is not None:
        D = np.asarray(D, np.float64).reshape(-1)
        if np.any(D != 0.0) or np.any(np.isnan(D)):
            raise ValueError(f"intrinsics_of: D {D.tolist()} has a non-zero distortion coefficient; only the pinhole "
                             "model is supported")
    return np.float32(K[0]), np.float32(K[4]), np.float32(K[2]), np.float32(K[5])


def depth_layout_of(image, intrinsics, depth_scale=0.001, z_min=0.0, z_max=np.inf):
    """The pp_depth_layout fields of one frame (DEPTH_LAYOUT_KEYS) as a dict; `image_as_tuple` and `intrinsics_of` say
    what the first two arguments are.  Raises a ValueError that names the field for: step < width * itemsize, an unknown
    encoding, fx or fy zero or non-finite, ppx or ppy non-finite, depth_scale <= 0 or non-finite on 16UC1, z_min > z_max,
    a data buffer shorter than height * step."""
    data, width, height, step, encoding, big = image_as_tuple(image)
    if encoding not in DEPTH_ENCODINGS:
        raise ValueError(f"encoding {encoding!r} is not a depth encoding ({', '.join(DEPTH_ENCODINGS)})")
    typ, code = DEPTH_ENCODINGS[encoding]
    size = np.dtype(typ).itemsize
    if width < 0 or height < 0:
        raise ValueError(f"width {width}, height {height}")
    if step < width * size:
        raise ValueError(f"step {step} < width {width} x {size} bytes")
    have = np.frombuffer(data, dtype=np.uint8).size
    if have < height * step:
        raise ValueError(f"Image data holds {have} bytes, {height} rows of step {step} needed")
    fx, fy, ppx, ppy = intrinsics_of(intrinsics)
    for name, v in (("fx", fx), ("fy", fy)):
        if not np.isfinite(v) or v == 0:
            raise ValueError(f"{name} {v} is not a finite non-zero focal length")
    for name, v in (("ppx", ppx), ("ppy", ppy)):
        if not np.isfinite(v):
            raise ValueError(f"{name} {v} is not finite")
    scale, lo, hi = np.float32(depth_scale), np.float32(z_min), np.float32(z_max)
    if code == 0 and not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"depth_scale {depth_scale} is not a finite positive number")
    if not lo <= hi:
        raise ValueError(f"z_min {z_min} > z_max {z_max}")
    return {"width": width, "height": height, "row_step": step, "encoding": code, "is_bigendian": int(big),
            "fx": float(fx), "fy": float(fy), "ppx": float(ppx), "ppy": float(ppy), "depth_scale": float(scale),
            "z_min": float(lo), "z_max": float(hi)}


def _depth_planes(image, intrinsics, depth_scale, z_min, z_max):
    """Rule 2-3 for every pixel: (x, y, z float32 [height, width], valid bool [height, width])."""
    lay = depth_layout_of(image, intrinsics, depth_scale, z_min, z_max)
    data, width, height, step, encoding, big = image_as_tuple(image)
    typ = np.dtype((">" if big else "<") + DEPTH_ENCODINGS[encoding][0])
    rows = np.frombuffer(data, dtype=np.uint8)[:height * step].reshape(height, step)[:, :width * typ.itemsize]
    raw = np.ascontiguousarray(rows).view(typ).reshape(height, width)
    f32 = np.float32
    with np.errstate(all="ignore"):
        if lay["encoding"] == 0:
            z = f32(lay["depth_scale"]) * raw.astype(f32)
            valid = raw != 0
        else:
            z = raw.astype(f32)
            valid = np.isfinite(z) & (z > 0)
        valid = valid & (z > f32(lay["z_min"])) & (z <= f32(lay["z_max"]))
        tx = (np.arange(width, dtype=f32) - f32(lay["ppx"])) / f32(lay["fx"])
        ty = (np.arange(height, dtype=f32) - f32(lay["ppy"])) / f32(lay["fy"])
        x = z * tx[None, :]
        y = z * ty[:, None]
    return x, y, z, valid


def depth_to_xyz(image, intrinsics, depth_scale=0.001, z_min=0.0, z_max=np.inf):
    """The float32 [N, 3] camera-frame points (x right, y down, z depth) of the valid pixels of a depth image, in
    row-major order: the rule at the head of this section in numpy float32."""
    x, y, z, valid = _depth_planes(image, intrinsics, depth_scale, z_min, z_max)
    return np.stack([x[valid], y[valid], z[valid]], axis=-1).astype(np.float32).reshape(-1, 3)


def depth_to_pointcloud2(image, intrinsics, depth_scale=0.001, z_min=0.0, z_max=np.inf, ordered=False, point_step=16):
    """The message tuple (`as_tuple`) a point-cloud node would publish for the image: FLOAT32 x y z at offsets 0 / 4 / 8 of
    `point_step`-byte records, little-endian.  Unordered: the valid pixels only, height 1.  Ordered: every pixel, width x
    height as the image, the invalid ones NaN."""
    if point_step < 12:
        raise ValueError(f"point_step {point_step} < 12")
    x, y, z, valid = _depth_planes(image, intrinsics, depth_scale, z_min, z_max)
    if ordered:
        xyz = np.stack([x, y, z], axis=-1).astype(np.float32).reshape(-1, 3)
        xyz[~valid.reshape(-1)] = np.nan
        height, width = valid.shape
    else:
        xyz = np.stack([x[valid], y[valid], z[valid]], axis=-1).astype(np.float32).reshape(-1, 3)
        height, width = 1, len(xyz)
    rec = np.zeros((len(xyz), point_step), np.uint8)
    rec[:, :12] = np.ascontiguousarray(xyz.astype("<f4")).view(np.uint8).reshape(len(xyz), 12)
    fields = [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1)]
    return (rec.tobytes(), width, height, int(point_step), width * int(point_step), fields, False)


def depth_kept_bound(width, height, first=1, decimate=4):
    """Most points a width x height depth image can keep: `kept_bound` of its pixels."""
    return kept_bound(width, height, first, decimate)


def depth_ingest_np(image, intrinsics, first=1, decimate=4, lift=SENSOR_HEIGHT, depth_scale=0.001, z_min=0.0, z_max=np.inf,
                    matrices=None):
    """What the GPU depth ingest computes for one image, on the host by its own rule: `depth_to_xyz` -> `select_np` ->
    `transform_ordered64` -> float32.  Returns (points [kept, 3] float32, valid pixels).  matrices / lift as `ingest_np`."""
    xyz = depth_to_xyz(image, intrinsics, depth_scale, z_min, z_max)
    keep = select_np(np.ones(len(xyz), bool), first, decimate)
    return transform_ordered64(xyz[keep], lift, matrices).astype(np.float32), len(xyz)


# ---- camera rigs (Engine.ingest_rig_depth / ingest_rig_pointcloud2, csrc/rig_ingest.hip) ------------------
# A robot carries two to four depth cameras, each with its own mount.  A rig call puts the cameras of one instant into ONE
# frame: the frame's points are the kept points of its cameras in camera order, back to back, each camera computed exactly
# as the single-camera ingest computes it alone under its own (first, decimate, r, r2, lift) -- validity, rank, selection,
# transform and rounding restart per camera.  The reference has no such path (one camera, one frame, load_data.py:2433);
# what is pinned is its single-camera chain, per source.  Not done: time synchronisation, de-duplication where the cameras
# overlap, lens distortion, cameras of both kinds (images and messages) in one call, more than RIG_MAX_SOURCES per frame.

RIG_MAX_SOURCES = 16


class Mount:
    """Where a camera sits: the (r, r2, lift) of pp_ingest_config -- a point (row vector, camera axes) becomes
    ((p . r) . r2) + lift.  r, r2: [3, 3] float64 (r2 defaults to the identity); lift: a height (-> [0, 0, lift]) or a
    vector of 3."""

    def __init__(self, r, r2=None, lift=0.0):
        self.r = np.array(r, np.float64).reshape(3, 3)
        self.r2 = np.eye(3) if r2 is None else np.array(r2, np.float64).reshape(3, 3)
        self.lift = _lift_vector(lift)
        if not (np.isfinite(self.r).all() and np.isfinite(self.r2).all() and np.isfinite(self.lift).all()):
            raise ValueError("Mount: r, r2 and lift must be finite")

    @property
    def matrices(self):
        return self.r, self.r2

    @classmethod
    def realsense(cls, lift=SENSOR_HEIGHT):
        """The reference's mount (load_data.py:2437-2443): its two scipy matrices and [0, 0, lift]."""
        r, r2 = _matrices()
        return cls(r, r2, lift)

    @classmethod
    def from_matrix(cls, T):
        """A general extrinsic [R | t], [4, 4] or [3, 4], taking a camera-frame COLUMN vector to the lidar frame
        (p' = R p + t): r = R transposed, r2 = identity, lift = t -- the existing three steps, no new arithmetic."""
        T = np.asarray(T, np.float64)
        if T.shape not in ((4, 4), (3, 4)):
            raise ValueError(f"Mount.from_matrix: a [4, 4] or [3, 4] matrix expected, got {T.shape}")
        if T.shape == (4, 4) and not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError(f"Mount.from_matrix: the last row is {T[3].tolist()}, not [0, 0, 0, 1]")
        return cls(T[:3, :3].T.copy(), None, T[:3, 3].copy())


class CameraRig:
    """The cameras of one frame, in the order their points are laid down.  mounts: one `Mount` per camera.  intrinsics
    (depth images only: anything `intrinsics_of` takes), first, decimate, depth_scale, z_min, z_max: one value for every
    camera, or a list with one per camera."""

    def __init__(self, mounts, intrinsics=None, first=1, decimate=4, depth_scale=0.001, z_min=0.0, z_max=np.inf):
        self.mounts = list(mounts)
        n = len(self.mounts)
        if not 1 <= n <= RIG_MAX_SOURCES:
            raise ValueError(f"a rig has 1 to {RIG_MAX_SOURCES} cameras, got {n}")
        if not all(isinstance(m, Mount) for m in self.mounts):
            raise ValueError("CameraRig: mounts must be Mount objects (Mount.realsense(), Mount.from_matrix(T))")
        one_set = intrinsics is None or not isinstance(intrinsics, list) or (
            len(intrinsics) in (4, 9) and all(np.ndim(v) == 0 for v in intrinsics))
        if not one_set and len(intrinsics) != n:
            raise ValueError(f"{len(intrinsics)} sets of intrinsics for {n} cameras")
        self.intrinsics = [intrinsics] * n if one_set else list(intrinsics)

        def per(name, v, cast):
            if np.ndim(v) == 0:
                return [cast(v)] * n
            if len(v) != n:
                raise ValueError(f"{len(v)} values of {name} for {n} cameras")
            return [cast(x) for x in v]

        self.first, self.decimate = per("first", first, int), per("decimate", decimate, int)
        self.depth_scale, self.z_min, self.z_max = (per(k, v, float) for k, v in
                                                    (("depth_scale", depth_scale), ("z_min", z_min), ("z_max", z_max)))
        for c in range(n):
            kept_bound(0, 0, self.first[c], self.decimate[c])         # (raises for first < 0, decimate < 1)

    def __len__(self):
        return len(self.mounts)

    def depth_kwargs(self, c):
        """The keyword arguments of `depth_ingest_np` for camera c (behind image and intrinsics)."""
        m = self.mounts[c]
        return dict(first=self.first[c], decimate=self.decimate[c], lift=m.lift, depth_scale=self.depth_scale[c],
                    z_min=self.z_min[c], z_max=self.z_max[c], matrices=m.matrices)

    def _cameras(self, sources, what):
        if len(sources) != len(self):
            raise ValueError(f"{what}: {len(sources)} sources for a rig of {len(self)} cameras")
        return range(len(self))


def rig_features(features, cameras):
    """The `features` of a rig call, per camera (of a plain call: per message): None; one list of FeatureFields for every
    camera; or a list with one such list per camera (the cameras' messages may name, scale or lack the field differently)."""
    if features is None:
        return [None] * cameras
    features = list(features)
    if features and all(isinstance(f, (list, tuple)) and all(isinstance(g, FeatureField) for g in f) for f in features):
        if len(features) != cameras:
            raise ValueError(f"{len(features)} feature lists for a rig of {cameras} cameras")
        widths = {len(f) for f in features}
        if len(widths) != 1:
            raise ValueError(f"the cameras' feature lists differ in length: {sorted(widths)}")
        return [list(f) for f in features]
    return [features] * cameras


def _rig_concat(parts):
    pts = [p for p, _ in parts]
    return (np.concatenate(pts).astype(np.float32).reshape(-1, pts[0].shape[1]), np.array([n for _, n in parts], np.int64),
            np.array([len(p) for p in pts], np.int64))


def rig_depth_ingest_np(images, rig):
    """What the GPU rig ingest computes for ONE frame of depth images (one per camera of the rig), on the host: the
    concatenation, in camera order, of `depth_ingest_np` of each camera alone under its own mount and selection.  Returns
    (points [sum kept, 3] float32, valid pixels per camera, kept points per camera)."""
    if any(k is None for k in rig.intrinsics):
        raise ValueError("rig_depth_ingest_np: the rig has no intrinsics")
    return _rig_concat([depth_ingest_np(images[c], rig.intrinsics[c], **rig.depth_kwargs(c))
                        for c in rig._cameras(images, "rig_depth_ingest_np")])


def rig_ingest_np(msgs, rig, features=None):
    """`rig_depth_ingest_np` for PointCloud2 messages: the concatenation of `ingest_np` per camera.  Returns (points,
    finite records per camera, kept points per camera).  features: `rig_features` -- the points are then [sum kept, 3 + nf]."""
    per = rig_features(features, len(rig))
    return _rig_concat([ingest_np(msgs[c], rig.first[c], rig.decimate[c], rig.mounts[c].lift, rig.mounts[c].matrices, per[c])
                        for c in rig._cameras(msgs, "rig_ingest_np")])


def rig_kept_bound(sizes, rig):
    """Most points ONE frame of the rig can keep: the sum over its cameras of `kept_bound(width, height, first, decimate)`
    -- what the engine's max_points_per_frame must reach.  sizes: one (width, height) per camera."""
    return sum(kept_bound(sizes[c][0], sizes[c][1], rig.first[c], rig.decimate[c]) for c in rig._cameras(sizes, "rig_kept_bound"))


def rig_frame_map(frames, rig, what="rig"):
    """frames: list of B lists with one source per camera -> (the sources in call order, source_frame int32 [B * cameras]);
    raises when a frame has another number of sources than the rig has cameras."""
    flat, fmap = [], []
    for b, fr in enumerate(frames):
        if len(fr) != len(rig):
            raise ValueError(f"{what}: frame {b} has {len(fr)} sources, the rig has {len(rig)} cameras")
        flat.extend(fr)
        fmap.extend([b] * len(fr))
    if not flat:
        raise ValueError(f"{what}: no frames")
    return flat, np.array(fmap, np.int32)


def check_frame_map(source_frame, batch):
    """The rules pp_ingest_rig_* hold a frame map to, on the host: it starts at 0, never decreases, skips no frame, ends at
    batch - 1, and no frame has more than RIG_MAX_SOURCES sources.  Raises a ValueError that names the source."""
    m = [int(v) for v in source_frame]
    if not m:
        raise ValueError("the frame map is empty")
    if m[0] != 0:
        raise ValueError(f"source 0: source_frame {m[0]}, the frame map starts at frame 0")
    run = 1
    for s in range(1, len(m)):
        if m[s] < m[s - 1]:
            raise ValueError(f"source {s}: source_frame {m[s]} < {m[s - 1]} of the source before it (the frame map never decreases)")
        if m[s] > m[s - 1] + 1:
            raise ValueError(f"source {s}: source_frame {m[s]} skips frame {m[s - 1] + 1}")
        run = run + 1 if m[s] == m[s - 1] else 1
        if run > RIG_MAX_SOURCES:
            raise ValueError(f"source {s}: frame {m[s]} has more than {RIG_MAX_SOURCES} sources")
    if m[-1] != int(batch) - 1:
        raise ValueError(f"source {len(m) - 1}: source_frame {m[-1]}, the frame map ends at frame batch - 1 = {int(batch) - 1}")
    return np.array(m, np.int32)
