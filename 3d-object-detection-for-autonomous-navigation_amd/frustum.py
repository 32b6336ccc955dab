"""The frustum crop of KITTI-style clouds (box_np_ops.remove_outside_points, second/core/box_np_ops.py:647-664): a point
stays iff it lies inside the pyramid the camera image spans between 0.001 m and 100 m.  KITTI labels exist inside the image
only, so the reference crops before it counts points per box (_calculate_num_points_in_gt), before it cuts out database
objects (create_groundtruth_database) and when it writes the `velodyne_reduced` files (_create_reduced_point_cloud).

The rule, in two halves:

Per frame, on the host, float64, numpy's calls in the reference's order (a LAPACK inverse and a QR are nothing to
reproduce bit for bit on a device, and it is 24 numbers per frame):
  1. C, R, T = projection_matrix_to_CRT_kitti(P2): inv(P2[:3, :3]) -> QR -> C = inv(upper factor), R = inv(orthogonal
     factor), T = upper factor @ P2[:3, 3];
  2. get_frustum([0, 0, W, H], C): the image's four corners (0, 0), (0, H), (W, H), (W, 0) at depth 0.001 and at depth 100,
     (corner - principal point) / (focal length / depth), 8 camera-frame points;
  3. minus T, through inv(R), through inv((rect @ Trv2c).T): 8 lidar-frame corners;
  4. six faces of four corners each (FACE_CORNERS), and per face the plane through its first three corners:
     n = cross(c0 - c1, c1 - c2), d = -(n . c0).  The normals point inwards and are NOT unit length.
Per point, on the device (csrc/frustum_crop.hip) or here (`keep_mask`):
  5. s_k = ((x n0 + y n1) + z n2) + d in float64 on the widened float32 coordinates, left to right, every product and sum
     rounded on its own; the point is removed iff s_k >= 0 for some face k.  A NaN coordinate therefore survives every
     face and the point is KEPT; +-inf follows IEEE arithmetic.  Kept points keep their order and all their columns.
`back` (the reference's `_back` files): column 0 is negated first; tested negated, stored negated.

`remove_outside_points_np` is the host restatement: the checker of the device path (tests/golden/ref_frustum.npz, which
tools/gen_golden_frustum.py records from the reference's own functions) and what the dataset-level functions of
gt_database.py run with `engine=None`.  An Engine never falls back to it.
"""
import numpy as np

NEAR_CLIP, FAR_CLIP = 0.001, 100.0
# corner numbers of the six faces (corner_to_surfaces_3d_jit's table): near, far, and the four sides
FACE_CORNERS = np.array([0, 1, 2, 3, 7, 6, 5, 4, 0, 3, 7, 4, 1, 5, 6, 2, 0, 4, 5, 1, 3, 2, 6, 7]).reshape(6, 4)


def projection_matrix_to_CRT_kitti(proj):
    """P = C @ [R | T] of a KITTI projection matrix [>=3, 4]: C upper triangular (intrinsics), R, T."""
    proj = np.asarray(proj, np.float64)
    cr, ct = proj[0:3, 0:3], proj[0:3, 3]
    rinv, cinv = np.linalg.qr(np.linalg.inv(cr))
    return np.linalg.inv(cinv), np.linalg.inv(rinv), cinv @ ct


def get_frustum(bbox_image, C, near_clip=NEAR_CLIP, far_clip=FAR_CLIP):
    """The 8 camera-frame corners [8, 3] of the pyramid over the image box (u0, v0, u1, v1): near face first."""
    fku, fkv = C[0, 0], -C[1, 1]
    u0v0 = C[0:2, 2]
    b = bbox_image
    corners = np.array([[b[0], b[1]], [b[0], b[3]], [b[2], b[3]], [b[2], b[1]]], dtype=C.dtype)
    xy = [(corners - u0v0) / np.array([fku / clip, -fkv / clip], dtype=C.dtype) for clip in (near_clip, far_clip)]
    z = np.array([near_clip] * 4 + [far_clip] * 4, dtype=C.dtype)[:, np.newaxis]
    return np.concatenate([np.concatenate(xy, axis=0), z], axis=1)


def frustum_corners_lidar(rect, trv2c, p2, image_shape):
    """The image frustum's 8 corners in the lidar frame [8, 3] float64.  image_shape: (height, width)."""
    C, R, T = projection_matrix_to_CRT_kitti(p2)
    fr = get_frustum([0, 0, image_shape[1], image_shape[0]], C)
    fr = fr - T
    fr = (np.linalg.inv(R) @ fr.T).T
    fr = np.concatenate([fr, np.ones((8, 1))], axis=-1)
    return (fr @ np.linalg.inv((np.asarray(rect, np.float64) @ np.asarray(trv2c, np.float64)).T))[..., :3]


def corner_planes(corners):
    """[8, 3] corners -> [6, 4] planes (n0, n1, n2, d), the normals inwards and not normalised."""
    s = np.asarray(corners, np.float64)[FACE_CORNERS][np.newaxis]            # [1, 6, 4, 3]: one polygon, as the reference holds it
    vec = s[:, :, :2, :] - s[:, :, 1:3, :]
    n = np.cross(vec[:, :, 0, :], vec[:, :, 1, :])
    d = np.einsum("aij, aij->ai", n, s[:, :, 0, :])
    return np.concatenate([n[0], -d[0][:, np.newaxis]], axis=1)


def frustum_planes(rect, trv2c, p2, image_shape):
    """The six planes [6, 4] float64 the crop tests one frame's points against (Engine.crop_to_image takes a stack)."""
    return corner_planes(frustum_corners_lidar(rect, trv2c, p2, image_shape))


def info_planes(info):
    """frustum_planes of a KITTI info dict: calib/R0_rect, calib/Tr_velo_to_cam, calib/P2 and img_shape."""
    return frustum_planes(info["calib/R0_rect"], info["calib/Tr_velo_to_cam"], info["calib/P2"], info["img_shape"])


def keep_mask(xyz, planes):
    """Step 5 for [n, >=3] float32 points and [6, 4] planes: bool [n], True where the point stays."""
    p = np.asarray(xyz)
    if p.dtype != np.float32:
        raise ValueError(f"points must be float32 (the rule widens float32 coordinates), got {p.dtype}")
    pl = np.asarray(planes, np.float64).reshape(6, 4)
    x, y, z = (p[:, k].astype(np.float64)[:, np.newaxis] for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((x * pl[:, 0] + y * pl[:, 1]) + z * pl[:, 2]) + pl[:, 3]
    return ~(s >= 0).any(axis=1)


def crop_np(points, planes, back=False):
    """One frame [n, F] float32 against its planes: the kept rows (a copy), column 0 negated first when `back`."""
    p = np.asarray(points)
    if p.ndim != 2 or p.shape[1] < 3:
        raise ValueError(f"points must be [n, F >= 3], got {p.shape}")
    if back:
        p = p.copy()
        p[:, 0] = -p[:, 0]
    return p[keep_mask(p, planes)]


def remove_outside_points_np(points, rect, trv2c, p2, image_shape, back=False):
    """box_np_ops.remove_outside_points on the host (back: as _create_reduced_point_cloud negates x before it)."""
    return crop_np(points, frustum_planes(rect, trv2c, p2, image_shape), back)
