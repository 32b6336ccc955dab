"""Rotated-box NMS on the GPU (csrc/rotate_nms.hip through pp_rotate_nms).

Replaces the reference's rotate_nms_gpu (second/core/non_max_suppression/nms_gpu.py:455-490), which it ships and exports
but never calls, with the pre / post caps of nms() around it (libraries/eval_helper_functions.py:463-492).  The detector
uses the same rule inside its post-process with `Engine.set_nms_mode("rotated")` or the config key
`model.second.use_rotate_nms`.
"""
import ctypes

import numpy as np

from . import _lib

MAX_BOXES = 16384       # PP_RNMS_MAX_BOXES: most boxes that enter the suppression (after pre_max_size)


def boxes_for_rotate_nms(box3d_lidar):
    """[N,7] lidar boxes (x, y, z, w, l, h, r) -> [N,5] (x, y, w, l, r): boxes_for_nms of model/voxelnet.py:1233."""
    b = np.asarray(box3d_lidar)
    if b.ndim != 2 or b.shape[1] != 7:
        raise ValueError(f"box3d_lidar must be [N,7], got {b.shape}")
    return b[:, [0, 1, 3, 4, 6]]


def rotate_nms(dets, iou_threshold, pre_max_size=None, post_max_size=None, device=0):
    """dets [N,6] (centre x, centre y, x size, y size, angle, score) -> int64 indices of the kept boxes, by descending
    score (equal scores: lower index first); empty when nothing is kept.  pre_max_size: only the best that many enter;
    post_max_size: at most that many are returned; None (or <= 0): no cap.  A box is dropped when its rotated IoU with
    an earlier kept box is > iou_threshold (float32, the higher-scoring box as devRotateIoU's first argument)."""
    d = np.ascontiguousarray(dets, dtype=np.float32)
    if d.ndim != 2 or d.shape[1] != 6:
        raise ValueError(f"dets must be [N,6] (x, y, x size, y size, angle, score), got {d.shape}")
    if not np.isfinite(d[:, 5]).all():
        raise ValueError("rotate_nms: scores must be finite")
    n = d.shape[0]
    pre = 0 if pre_max_size is None else int(pre_max_size)
    post = 0 if post_max_size is None else int(post_max_size)
    keep = np.zeros((max(n, 1),), dtype=np.int32)
    nk = ctypes.c_int64(0)
    L = _lib.lib()
    st = L.pp_rotate_nms(int(device), d.ctypes.data, n, ctypes.c_float(iou_threshold), pre, post, keep.ctypes.data,
                         ctypes.byref(nk))
    if st != 0:
        msg = L.pp_last_error(None)
        cls = ValueError if st == 1 else RuntimeError
        raise cls(f"rotate_nms: {msg.decode() if msg else st}")
    return keep[:nk.value].astype(np.int64)
