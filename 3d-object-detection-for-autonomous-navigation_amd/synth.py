"""Seeded synthetic point clouds of the shapes BASELINE.json names (no datasets here).

d435i cloud: N float32 xyz points; depth x ~ 0.3 + 6.1*Beta(2,3),
y ~ U(-0.62 x, 0.62 x) (about 64 deg HFOV), z ~ N(0, 0.45) clipped to (-1, 1.2)
plus a ground band, ~2 % of points outside the voxel range, 1-3 pedestrian
blobs (0.5 x 0.5 x 1.7 m, 400-1500 points each), and a share of points lifted
above z = 1.0 so that the second z-cell of the shipped config is populated
(SURVEY Appendix B).  KITTI-shaped cloud: N xyzi points, 1/r^2 density.
"""
import numpy as np


def d435i_cloud(frame, n_points=16384, num_features=3, seed=1234):
    rng = np.random.default_rng(seed + int(frame))
    n_blobs = int(rng.integers(1, 4))
    blob_sizes = [int(rng.integers(400, 1501)) for _ in range(n_blobs)]
    n_out = int(0.02 * n_points)
    n_ground = int(0.15 * n_points)
    n_bg = n_points - sum(blob_sizes) - n_out - n_ground
    if n_bg < 0:
        blob_sizes = [max(1, n_points // 16)] * n_blobs
        n_out, n_ground = n_points // 50, n_points // 8
        n_bg = n_points - sum(blob_sizes) - n_out - n_ground
    parts = []
    x = 0.3 + 6.1 * rng.beta(2.0, 3.0, n_bg)
    y = np.clip(rng.uniform(-0.62, 0.62, n_bg) * x, -2.559, 2.559)
    z = np.clip(rng.normal(0.0, 0.45, n_bg), -1.0, 1.2)
    parts.append(np.stack([x, y, z], axis=1))
    xg = 0.3 + 6.1 * rng.beta(2.0, 2.0, n_ground)
    yg = np.clip(rng.uniform(-0.62, 0.62, n_ground) * xg, -2.559, 2.559)
    zg = -0.95 + 0.03 * rng.standard_normal(n_ground)
    parts.append(np.stack([xg, yg, zg], axis=1))
    for sz in blob_sizes:
        cx = rng.uniform(1.0, 5.5)
        cy = rng.uniform(-0.5, 0.5) * cx
        px = cx + rng.uniform(-0.25, 0.25, sz)
        py = cy + rng.uniform(-0.25, 0.25, sz)
        pz = rng.uniform(-0.95, 0.75, sz)
        # a d435i cloud is lifted by +1 m before voxelisation (load_data.py:2443):
        # let some blobs reach above z = 1.0 into the second z-cell
        if rng.random() < 0.5:
            pz = pz + 0.6
        parts.append(np.stack([px, py, pz], axis=1))
    xo = rng.uniform(-1.0, 8.0, n_out)
    yo = rng.uniform(-4.0, 4.0, n_out)
    zo = rng.uniform(-4.0, 4.0, n_out)
    parts.append(np.stack([xo, yo, zo], axis=1))
    pts = np.concatenate(parts, axis=0)
    pts = pts[rng.permutation(pts.shape[0])]
    if num_features > 3:
        extra = rng.uniform(0.0, 1.0, (pts.shape[0], num_features - 3))
        pts = np.concatenate([pts, extra], axis=1)
    return np.ascontiguousarray(pts[:n_points].astype(np.float32))


def kitti_cloud(frame, n_points=20000, num_features=4, seed=4321):
    rng = np.random.default_rng(seed + int(frame))
    # 1/r^2 density out to ~70 m within the forward half-plane
    r = 2.0 / (rng.uniform(2.0 / 75.0, 1.0, n_points))
    th = rng.uniform(-0.85, 0.85, n_points)
    x = r * np.cos(th)
    y = r * np.sin(th)
    z = np.clip(-1.6 + 0.25 * rng.standard_normal(n_points) + rng.uniform(0, 1.8, n_points) *
                (rng.random(n_points) < 0.3), -2.99, 0.99)
    cols = [x, y, z]
    for _ in range(num_features - 3):
        cols.append(rng.uniform(0.0, 1.0, n_points))
    return np.ascontiguousarray(np.stack(cols, axis=1).astype(np.float32))


def default_calib():
    """rect = I, Trv2c as in the reference's production path (train.py:681-682)."""
    rect = np.eye(4, dtype=np.float32)
    trv2c = np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], dtype=np.float32)
    p2 = np.eye(4, dtype=np.float32)
    return rect, trv2c, p2


def pointcloud2_from_xyz(xyz, width, height, point_step=20, row_pad=0, datatype=7, bigendian=False, offsets=(0, 4, 8),
                         seed=977):
    """[width * height, 3] camera-frame coordinates (NaN / inf allowed) -> a sensor_msgs/PointCloud2 as the tuple
    `ingest.pointcloud2_to_xyz` takes: (data, width, height, point_step, row_step, fields, is_bigendian).  Records of
    `point_step` bytes in rows padded by `row_pad` bytes; x y z (datatype 7 FLOAT32 or 8 FLOAT64) at `offsets`; every
    other byte is random."""
    rng = np.random.default_rng(seed)
    n = int(width) * int(height)
    cam = np.asarray(xyz, np.float64).reshape(n, 3)
    dt = np.dtype((">" if bigendian else "<") + ("f8" if datatype == 8 else "f4"))
    if max(offsets) + dt.itemsize > point_step:
        raise ValueError(f"offsets {offsets} do not fit point_step {point_step}")
    rec = rng.integers(0, 256, (n, point_step), dtype=np.uint8)
    for k, off in enumerate(offsets):
        rec[:, off:off + dt.itemsize] = np.ascontiguousarray(cam[:, k].astype(dt)).view(np.uint8).reshape(n, dt.itemsize)
    row_step = width * point_step + int(row_pad)
    rows = rng.integers(0, 256, (height, row_step), dtype=np.uint8)
    rows[:, :width * point_step] = rec.reshape(height, width * point_step)
    fields = [("x", offsets[0], datatype, 1), ("y", offsets[1], datatype, 1), ("z", offsets[2], datatype, 1)]
    if point_step >= max(offsets) + dt.itemsize + 4:
        fields.append(("rgb", max(offsets) + dt.itemsize, 7, 1))
    return (rows.tobytes(), int(width), int(height), int(point_step), row_step, fields, bool(bigendian))


_PF_NUMPY = {1: "i1", 2: "u1", 3: "i2", 4: "u2", 5: "i4", 6: "u4", 7: "f4", 8: "f8"}      # PointField datatype codes


def pointcloud2_from_points(points, width, height, feature_fields=(("intensity", 7, 12),), point_step=16, row_pad=0,
                            datatype=7, bigendian=False, offsets=(0, 4, 8), extra_fields=(), seed=977):
    """[width * height, 3 + nf] rows (x y z and nf further columns; NaN / inf allowed) -> a sensor_msgs/PointCloud2 tuple as
    `pointcloud2_from_xyz` gives it, with one more field per column.  feature_fields: one (name, datatype, offset[, count[,
    index]]) per column -- the column's values are stored as that PointField datatype (1 INT8 ... 8 FLOAT64; an integer
    type takes the values as they are, so give it integers in its range) at byte `offset` of a record; with count > 1
    the field has `count` elements, the values go to element `index` and the others are random.  extra_fields: further
    (name, offset, datatype, count) fields that are declared and left random (a lidar driver's `ring`, `time`).  x y z,
    point_step, row_pad, datatype, bigendian, offsets and the random filling as `pointcloud2_from_xyz`."""
    rng = np.random.default_rng(seed)
    n = int(width) * int(height)
    feature_fields = [tuple(f) for f in feature_fields]
    pts = np.asarray(points, np.float64).reshape(n, 3 + len(feature_fields))
    order = ">" if bigendian else "<"
    dt = np.dtype(order + ("f8" if datatype == 8 else "f4"))
    if max(offsets) + dt.itemsize > point_step:
        raise ValueError(f"offsets {offsets} do not fit point_step {point_step}")
    rec = rng.integers(0, 256, (n, point_step), dtype=np.uint8)
    for k, off in enumerate(offsets):
        rec[:, off:off + dt.itemsize] = np.ascontiguousarray(pts[:, k].astype(dt)).view(np.uint8).reshape(n, dt.itemsize)
    fields = [("x", offsets[0], datatype, 1), ("y", offsets[1], datatype, 1), ("z", offsets[2], datatype, 1)]
    for j, ff in enumerate(feature_fields):
        name, typ, off = ff[0], int(ff[1]), int(ff[2])
        count = int(ff[3]) if len(ff) > 3 else 1
        index = int(ff[4]) if len(ff) > 4 else 0
        if typ not in _PF_NUMPY:
            raise ValueError(f"feature field {name}: unknown datatype {typ}")
        fdt = np.dtype(order + _PF_NUMPY[typ])
        if off < 0 or off + fdt.itemsize * count > point_step or not 0 <= index < count:
            raise ValueError(f"feature field {name}: offset {off}, count {count}, index {index} do not fit point_step {point_step}")
        at = off + index * fdt.itemsize
        with np.errstate(invalid="ignore", over="ignore"):
            vals = pts[:, 3 + j].astype(fdt)
        rec[:, at:at + fdt.itemsize] = np.ascontiguousarray(vals).view(np.uint8).reshape(n, fdt.itemsize)
        fields.append((str(name), off, typ, count))
    fields.extend((str(nm), int(o), int(t), int(c)) for nm, o, t, c in extra_fields)
    row_step = width * point_step + int(row_pad)
    rows = rng.integers(0, 256, (height, row_step), dtype=np.uint8)
    rows[:, :width * point_step] = rec.reshape(height, width * point_step)
    return (rows.tobytes(), int(width), int(height), int(point_step), row_step, fields, bool(bigendian))


def pointcloud2_message(frame, width=640, height=480, point_step=20, row_pad=0, nan_fraction=0.3, datatype=7,
                        bigendian=False, offsets=(0, 4, 8), seed=977):
    """A seeded camera message (`pointcloud2_from_xyz`): the points are a `d435i_cloud` turned back into camera axes
    (x right, y down, z depth; the ingest's lift undone), and `nan_fraction` of the records carry a NaN coordinate, as
    a depth camera's invalid pixels do.  The d435i driver's own layout is point_step 20 (x y z float32, rgb at 16)."""
    rng = np.random.default_rng(seed + int(frame))
    n = int(width) * int(height)
    lidar = d435i_cloud(frame, max(n, 1), seed=seed)[:n].astype(np.float64)
    cam = np.stack([-lidar[:, 1], 1.0 - lidar[:, 2], lidar[:, 0]], axis=1)
    bad = rng.random(n) < nan_fraction
    cam[bad, rng.integers(0, 3, int(bad.sum()))] = np.nan
    return pointcloud2_from_xyz(cam, width, height, point_step, row_pad, datatype, bigendian, offsets, seed + int(frame))


def depth_from_z(z, encoding="16UC1", step_pad=0, bigendian=False, depth_scale=0.001, seed=977):
    """[height, width] depths in metres (0 / NaN / inf / negatives allowed for 32FC1; 16UC1 stores round(z / depth_scale),
    0 for an invalid pixel) -> a sensor_msgs/Image as the tuple `ingest.image_as_tuple` gives: (data, width, height, step,
    encoding, is_bigendian).  Rows are padded by `step_pad` random bytes."""
    rng = np.random.default_rng(seed)
    z = np.asarray(z)
    height, width = z.shape
    if encoding == "32FC1":
        dt = np.dtype((">" if bigendian else "<") + "f4")
        px = z.astype(dt)
    else:
        dt = np.dtype((">" if bigendian else "<") + "u2")
        with np.errstate(invalid="ignore"):
            units = np.where(np.isfinite(z) & (z > 0), np.rint(np.asarray(z, np.float64) / depth_scale), 0.0)
        px = np.clip(units, 0, 65535).astype(dt)
    step = width * dt.itemsize + int(step_pad)
    rows = rng.integers(0, 256, (height, step), dtype=np.uint8)
    rows[:, :width * dt.itemsize] = np.ascontiguousarray(px).view(np.uint8).reshape(height, width * dt.itemsize)
    return (rows.tobytes(), int(width), int(height), step, encoding, bool(bigendian))


def depth_image(frame, width=640, height=480, encoding="16UC1", step_pad=0, bigendian=False, invalid_fraction=0.3,
                depth_scale=0.001, scale=1.0, seed=977):
    """A seeded depth image of a d435i-like camera 1 m above a floor, looking at a wall 7 m away with a few person-sized
    columns in front of it (all distances times `scale`: a small grid wants a small scene); `invalid_fraction` of the
    pixels are 0 (no depth), as a stereo camera's holes are.  Returns
    (image tuple of `depth_from_z`, (fx, fy, ppx, ppy))."""
    rng = np.random.default_rng(seed + int(frame))
    fx = fy = 0.6 * max(width, 1)
    ppx, ppy = 0.5 * width - 0.5 + 0.37, 0.5 * height - 0.5 - 0.21
    tx = (np.arange(width) - ppx) / fx
    ty = (np.arange(height) - ppy) / fy
    z = np.full((height, width), 7.0)
    with np.errstate(divide="ignore"):
        floor = np.where(ty > 1e-3, 1.0 / np.maximum(ty, 1e-3), np.inf)
    z = np.minimum(z, floor[:, None])
    for _ in range(4):
        depth, cx, half = rng.uniform(2.0, 5.5), rng.uniform(-1.5, 1.5), rng.uniform(0.2, 0.35)
        cols = np.abs(tx * depth - cx) < half
        rows_ = (ty * depth > -0.7) & (ty * depth < 1.0)
        z = np.where(rows_[:, None] & cols[None, :], np.minimum(z, depth), z)
    z = (z + 0.01 * rng.standard_normal(z.shape)) * scale
    z[rng.random(z.shape) < invalid_fraction] = 0.0
    img = depth_from_z(z, encoding, step_pad, bigendian, depth_scale, seed + int(frame))
    return img, (float(fx), float(fy), float(ppx), float(ppy))
