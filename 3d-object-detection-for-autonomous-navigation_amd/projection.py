"""Image boxes of camera-frame 3D boxes: the eight corners projected by P2, min / max over them.

Replaces second/core/box_np_ops.py:849-857 (box3d_to_bbox: center_to_corner_box3d :335-360, corners_nd :170-201,
rotation_3d_in_axis :259-277, project_to_image :605-611), the computation the reference's predict() commented out
(model/voxelnet.py:1336-1355) in favour of a constant placeholder (:1357-1360).  `box3d_to_bbox` is the host restatement;
`box3d_to_bbox_gpu` runs csrc/box_project.hip through pp_box3d_to_bbox; the detector does the same inside its post-process
with `Engine.set_projection(p2)` or the config key `model.second.project_bbox`.

The rule, with the reference's quirks kept:
  * a box is (x, y, z, l, h, w, ry); its corners are (l (ux - 0.5), h (uy - 1.0), w (uz - 0.5)), u in {0, 1}^3 -- the
    origin is the bottom face centre, camera y points down;
  * rotation about y: X = x c + y 0 + z s, Y = x 0 + y 1 + z 0, Z = x (-s) + y 0 + z c, then the centre is added (the
    zero terms are kept: they decide the sign of a zero and turn an infinity into NaN as the einsum does);
  * project_to_image appends ZEROS, not ones, as the homogeneous coordinate: P2's fourth column never enters,
    u' = X P[0,0] + Y P[0,1] + Z P[0,2] and likewise v', w'; u = u' / w', v = v' / w';
  * bbox = [min u, min v, max u, max v] over the 8 corners in float64, NaN propagating; nothing clips to the image and
    nothing treats corners behind the camera (w' < 0 mirrors them, w' = 0 gives inf / NaN).
"""
import ctypes

import numpy as np

from . import _lib

# corners_nd: unravel_index(arange(8), [2, 2, 2]) reordered by [0, 1, 3, 2, 4, 5, 7, 6]
CORNER_UNITS = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]], np.float64)
_ORIGIN = np.array([0.5, 1.0, 0.5])


def _p2_rows(p2, frames=None):
    p = np.asarray(p2, np.float64)
    if p.ndim == 2:
        p = p[None]
    if p.ndim != 3 or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError(f"p2 must be [4,4] / [3,4] or [F,4,4], got {np.asarray(p2).shape}")
    if p.shape[1] == 3:
        p = np.concatenate([p, np.broadcast_to(np.array([[[0., 0., 0., 1.]]]), (p.shape[0], 1, 4))], axis=1)
    if frames is not None:
        if p.shape[0] not in (1, frames):
            raise ValueError(f"p2 holds {p.shape[0]} matrices for {frames} frames")
        p = np.broadcast_to(p, (frames, 4, 4))
    return np.ascontiguousarray(p)


def box3d_to_bbox(boxes_camera, p2, return_parts=False):
    """boxes_camera [N,7] (x, y, z, l, h, w, ry), p2 [4,4] (or [N,4,4]: one matrix per box) -> bbox [N,4] float64.
    Plain elementwise float64 in the term order of the module docstring: no `@`, no einsum, so the bits do not depend on
    a BLAS.  return_parts: also the corners [N,8,3], the projected points [N,8,2] and, per projected point, the
    condition magnitude [N,8,2] the tests measure errors in (sum of the absolute values of every product and addend of
    the numerator, over |w'|, plus |result|)."""
    b = np.asarray(boxes_camera, np.float64)
    if b.ndim != 2 or b.shape[1] != 7:
        raise ValueError(f"boxes_camera must be [N,7], got {b.shape}")
    n = b.shape[0]
    P = np.asarray(p2, np.float64)
    if P.ndim == 2:
        P = np.broadcast_to(P, (n,) + P.shape)
    if P.shape[0] != n or P.shape[1] < 3 or P.shape[2] < 3:
        raise ValueError(f"p2 must be [4,4] or [N,4,4], got {np.asarray(p2).shape}")
    P = P[:, None]                                           # [N,1,r,c]
    with np.errstate(all="ignore"):
        rel = CORNER_UNITS - _ORIGIN                         # [8,3], exact
        x = b[:, None, 3] * rel[None, :, 0]
        y = b[:, None, 4] * rel[None, :, 1]
        z = b[:, None, 5] * rel[None, :, 2]
        c, s = np.cos(b[:, None, 6]), np.sin(b[:, None, 6])
        X = (x * c + y * 0.0 + z * s) + b[:, None, 0]
        Y = (x * 0.0 + y * 1.0 + z * 0.0) + b[:, None, 1]
        Z = (x * (-s) + y * 0.0 + z * c) + b[:, None, 2]
        num = [X * P[..., r, 0] + Y * P[..., r, 1] + Z * P[..., r, 2] for r in range(3)]
        pts = np.stack([num[0] / num[2], num[1] / num[2]], axis=-1)
        bbox = np.concatenate([np.min(pts, axis=1), np.max(pts, axis=1)], axis=1)
        if not return_parts:
            return bbox
        aX = np.abs(x * c) + np.abs(z * s) + np.abs(b[:, None, 0])
        aY = np.abs(y) + np.abs(b[:, None, 1])
        aZ = np.abs(x * s) + np.abs(z * c) + np.abs(b[:, None, 2])
        mag = [aX * np.abs(P[..., r, 0]) + aY * np.abs(P[..., r, 1]) + aZ * np.abs(P[..., r, 2]) for r in range(2)]
        cond = np.stack([mag[0], mag[1]], axis=-1) / np.abs(num[2])[..., None] + np.abs(pts)
    return bbox, np.stack([X, Y, Z], axis=-1), pts, cond


def box3d_to_bbox_gpu(boxes, box_counts, p2, device_id=0):
    """boxes [N,7] camera-frame boxes of F frames laid end to end, box_counts [F] boxes per frame (sum N), p2 [F,4,4]
    (or one [4,4] for all) -> bbox [N,4] float64, by the kernel the detector's post-process shares its arithmetic with
    (pp_box3d_to_bbox)."""
    b = np.ascontiguousarray(boxes, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != 7:
        raise ValueError(f"boxes must be [N,7], got {b.shape}")
    cnt = np.ascontiguousarray(box_counts, dtype=np.int32).reshape(-1)
    if (cnt < 0).any() or int(cnt.sum()) != b.shape[0]:
        raise ValueError(f"box_counts must be non-negative and sum to N = {b.shape[0]}")
    F = cnt.shape[0]
    P = _p2_rows(p2, F).reshape(F, 16) if F else np.zeros((0, 16))
    out = np.zeros((b.shape[0], 4), dtype=np.float64)
    L = _lib.lib()
    st = L.pp_box3d_to_bbox(int(device_id), b.ctypes.data, cnt.ctypes.data, F, P.ctypes.data, out.ctypes.data)
    if st != 0:
        msg = L.pp_last_error(None)
        cls = ValueError if st == 1 else RuntimeError
        raise cls(f"box3d_to_bbox_gpu: {msg.decode() if msg else st}")
    return out


def clip_bbox_to_image(bbox, image_shape):
    """bbox [N,4] (x0, y0, x1, y1), image_shape (height, width) -> (clipped [M,4], keep [N] bool).  The rule of upstream
    SECOND's predict_kitti_to_anno, which the reference deleted together with the projection (so no reference code
    pins it): a box with x0 > width, y0 > height, x1 < 0 or y1 < 0 is dropped; the others get x1, y1 limited to
    (width, height) and x0, y0 to 0."""
    bb = np.asarray(bbox, np.float64).reshape(-1, 4)
    h, w = float(image_shape[0]), float(image_shape[1])
    keep = ~((bb[:, 0] > w) | (bb[:, 1] > h) | (bb[:, 2] < 0) | (bb[:, 3] < 0))
    out = bb[keep].copy()
    out[:, 2:] = np.minimum(out[:, 2:], [w, h])
    out[:, :2] = np.maximum(out[:, :2], [0, 0])
    return out, keep
