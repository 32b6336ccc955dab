"""Golden vectors of the image-box projection from the reference's own numpy code:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_bbox.py      -> tests/golden/ref_bbox.npz

  box3d_to_bbox -> center_to_corner_box3d -> corners_nd, rotation_3d_in_axis; project_to_image
            second/core/box_np_ops.py:849-857, :335-360, :170-201, :259-277, :605-611

The reference is imported at run time (tools/ref_shim.py); only arrays are written:
  boxes [N,7] float64 camera boxes (x, y, z, l, h, w, ry), counts [4] boxes per frame (laid end to end), p2 [4,4,4] float64
  (float32 values widened, non-zero fourth column), kind [N] (0 regular, 1 wholly behind the camera, 2 straddling the
  camera plane, 3 degenerate), and the reference's corners [N,8,3], points [N,8,2] and bbox [N,4].

Regular boxes: pedestrian- and car-size, depths 1-40 m, ry over (-2 pi, 2 pi) with 0, +-pi/2 and flipped (+ pi) values
among them; every corner of every non-degenerate box has |w'| >= 0.5 (asserted).  The degenerate box has all dims 0 at
z = 0: every corner has w' = 0 exactly, and the reference's NaN / inf pattern is the expectation.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ref_shim.install()
from second.core import box_np_ops  # noqa: E402
import pp_amd  # noqa: E402

PRODUCED_BY = ["second.core.box_np_ops.box3d_to_bbox", "second.core.box_np_ops.center_to_corner_box3d",
               "second.core.box_np_ops.project_to_image"]
PER_FRAME = 50
W_MIN = 0.5


def camera_matrices():
    """Four KITTI-like P2 (float32 values widened): distinct focal lengths, principal points and fourth columns."""
    out = []
    for f, cx, cy, tx, ty, tz in [(721.5377, 609.5593, 172.854, 44.85728, 0.2163791, 0.002745884),
                                  (707.0493, 604.0814, 180.5066, 45.75831, -0.3454157, 0.004981016),
                                  (718.856, 607.1928, 185.2157, 45.38225, -0.1130887, 0.003779761),
                                  (384.2, 320.7, 243.1, 12.5, 0.75, 0.001)]:
        m = np.array([[f, 0, cx, tx], [0, f, cy, ty], [0, 0, 1, tz], [0, 0, 0, 1]], np.float32)
        out.append(m.astype(np.float64))
    return np.stack(out)


def depth_ok(boxes):
    """Every corner's |w'| >= W_MIN; w' = Z for these matrices (third row 0 0 1), taken from the reference's corners."""
    c = box_np_ops.center_to_corner_box3d(boxes[:, :3], boxes[:, 3:6], boxes[:, 6], [0.5, 1.0, 0.5], axis=1)
    return np.all(np.abs(c[..., 2]) >= W_MIN, axis=1)


def regular(rng, n, frame):
    special = [0.0, np.pi / 2, -np.pi / 2, np.pi, 0.3 + np.pi, -1.2 + np.pi, 2 * np.pi - 1e-3, -2 * np.pi + 1e-3]
    out = []
    while len(out) < n:
        car = rng.random() < 0.5
        dims = (rng.uniform([3.2, 1.3, 1.4], [4.6, 1.9, 2.0]) if car else rng.uniform([0.4, 1.4, 0.4], [1.2, 1.95, 0.9]))
        z = rng.uniform(1.0, 40.0)
        x = rng.uniform(-0.6, 0.6) * z
        y = rng.uniform(0.8, 2.2)
        k = len(out)
        ry = special[(k + frame) % len(special)] if k % 6 == 0 else rng.uniform(-2 * np.pi, 2 * np.pi)
        # values as the detector holds them: float32 widened
        b = np.array([x, y, z, *dims, ry], np.float32).astype(np.float64)[None]
        if depth_ok(b)[0]:
            out.append(b[0])
    return np.stack(out)


def main():
    rng = np.random.default_rng(20240607)
    p2 = camera_matrices()
    boxes, kind, counts = [], [], []
    for f in range(4):
        b = regular(rng, PER_FRAME, f)
        k = np.zeros(len(b), np.int64)
        if f == 1:      # wholly behind the camera: mirrored through the centre
            extra = np.array([[1.5, 1.6, -12.0, 3.9, 1.5, 1.6, 0.4]])
            b, k = np.concatenate([b, extra]), np.concatenate([k, [1]])
        if f == 2:      # a long box across the camera plane: corners at Z about -4 and +4
            extra = np.array([[0.7, 1.6, 0.0, 1.0, 1.5, 8.0, 0.0]])
            b, k = np.concatenate([b, extra]), np.concatenate([k, [2]])
        if f == 3:      # all dims 0 at z = 0: w' = 0 at every corner
            extra = np.array([[0.0, 1.5, 0.0, 0.0, 0.0, 0.0, 0.0]])
            b, k = np.concatenate([b, extra]), np.concatenate([k, [3]])
        boxes.append(b); kind.append(k); counts.append(len(b))
    boxes, kind, counts = np.concatenate(boxes), np.concatenate(kind), np.array(counts, np.int32)
    frame = np.repeat(np.arange(4), counts)

    corners = np.zeros((len(boxes), 8, 3))
    points = np.zeros((len(boxes), 8, 2))
    bbox = np.zeros((len(boxes), 4))
    with np.errstate(all="ignore"):
        for f in range(4):
            m = frame == f
            c = box_np_ops.center_to_corner_box3d(boxes[m, :3], boxes[m, 3:6], boxes[m, 6], [0.5, 1.0, 0.5], axis=1)
            corners[m] = c
            points[m] = box_np_ops.project_to_image(c, p2[f])
            bbox[m] = box_np_ops.box3d_to_bbox(boxes[m], None, None, p2[f])

    # what the fixture promises
    w = corners[..., 2]                                   # third row of every matrix is 0 0 1 (x 0): w' = Z
    assert np.all(np.abs(w[kind != 3]) >= W_MIN), "a corner with |w'| < 0.5"
    assert np.all(w[kind == 1] <= -W_MIN) and (kind == 1).sum() == 1
    ws = w[kind == 2]
    assert (ws < 0).any() and (ws > 0).any() and (kind == 2).sum() == 1
    assert np.all(w[kind == 3] == 0) and (kind == 3).sum() == 1 and not np.isfinite(bbox[kind == 3]).any()
    assert np.isfinite(bbox[kind != 3]).all()
    ry = boxes[kind == 0, 6]
    assert ry.min() < -6 and ry.max() > 6 and (ry == 0).any() and np.isin(np.float64(np.float32(np.pi / 2)), ry)
    z = boxes[kind == 0, 2]
    assert z.min() < 3 and z.max() > 37
    assert np.all(p2[:, :3, 3] != 0)
    # the project's restatement reproduces the arrays (loose here; the tests hold the measured bound)
    got, gc, gp, _ = pp_amd.projection.box3d_to_bbox(boxes, p2[frame], return_parts=True)
    reg = kind != 3
    np.testing.assert_allclose(gc[reg], corners[reg], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got[reg], bbox[reg], rtol=1e-10)
    assert np.array_equal(np.isnan(got), np.isnan(bbox)) and np.array_equal(np.isposinf(got), np.isposinf(bbox))

    out = os.path.join(ROOT, "tests", "golden", "ref_bbox.npz")
    np.savez_compressed(out, boxes=boxes, counts=counts, p2=p2, kind=kind, corners=corners, points=points, bbox=bbox,
                        produced_by=np.array(PRODUCED_BY))
    print(f"{out}: {len(boxes)} boxes, counts {counts.tolist()}, {os.path.getsize(out)} bytes; degenerate bbox {bbox[kind == 3]}")


if __name__ == "__main__":
    main()
