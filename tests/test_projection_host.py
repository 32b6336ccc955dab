"""Image boxes on the host: projection.box3d_to_bbox (the restatement) against the reference's own arrays
(tests/golden/ref_bbox.npz, written by tools/gen_golden_bbox.py from second/core/box_np_ops.py), the declared surface, the
config key, and the image clip of predict_kitti_to_anno.

Tolerance (projection_ref.py derives it): errors are measured against the formula in extended precision, in units of
2^-52 times the element's condition magnitude.  The reference itself is K_REF = 0.61 units away at worst (measured here and
asserted), so the bound is K = 4 * max(K_REF, 1) = 4 units; the restatement measures 0.61 (points) / 0.51 (boxes).
"""
import copy
import os
import re

import numpy as np
import pytest

from conftest import load_golden

import projection_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    g = load_golden("ref_bbox.npz")
    boxes, counts, p2, kind, frame, pb = pr.fixture(g)
    reg = kind != 3
    exact, rows = pr.exact_points(boxes[reg], pb[reg])
    return dict(g=g, boxes=boxes, counts=counts, p2=p2, kind=kind, frame=frame, pb=pb, reg=reg, exact=exact, rows=rows)


def test_fixture_is_what_the_recipe_promises(fx):
    g, kind = fx["g"], fx["kind"]
    assert fx["counts"].tolist() == [50, 51, 51, 51] and len(fx["boxes"]) == 203
    assert [(kind == k).sum() for k in (1, 2, 3)] == [1, 1, 1]
    w = g["corners"][..., 2]
    assert np.all(np.abs(w[kind != 3]) >= 0.5) and np.all(w[kind == 1] <= -0.5) and np.all(w[kind == 3] == 0)
    assert (w[kind == 2] < 0).any() and (w[kind == 2] > 0).any()
    assert np.all(fx["p2"][:, :3, 3] != 0) and np.array_equal(fx["p2"], fx["p2"].astype(np.float32).astype(np.float64))
    assert len({m.tobytes() for m in fx["p2"]}) == 4


def test_k_ref_and_the_restatement_within_k(pp, fx):
    g, reg, rows = fx["g"], fx["reg"], fx["rows"]
    bb, corners, pts, cond = pp.projection.box3d_to_bbox(fx["boxes"][reg], fx["pb"][reg], return_parts=True)
    ref_p = pr.point_ratios(g["points"][reg][rows], fx["exact"], cond[rows]).max()
    ref_b = pr.bbox_ratios(g["bbox"][reg][rows], fx["exact"], cond[rows]).max()
    got_p = pr.point_ratios(pts[rows], fx["exact"], cond[rows]).max()
    got_b = pr.bbox_ratios(bb[rows], fx["exact"], cond[rows]).max()
    print(f"longdouble {pr.HAVE_LONGDOUBLE}: K_ref points {ref_p:.3f} boxes {ref_b:.3f}; restatement points {got_p:.3f} "
          f"boxes {got_b:.3f}; K = {pr.K}")
    assert max(ref_p, ref_b) <= pr.K_REF, "the constant must cover the reference's own error"
    assert pr.K == 4 * max(pr.K_REF, 1)
    assert got_p <= pr.K and got_b <= pr.K
    np.testing.assert_allclose(corners, g["corners"][reg], rtol=0, atol=1e-11)
    assert np.array_equal(pp.projection.box3d_to_bbox(fx["boxes"][reg], fx["pb"][reg]), bb)


def test_degenerate_case_by_class(pp, fx):
    deg = fx["kind"] == 3
    got = pp.projection.box3d_to_bbox(fx["boxes"][deg], fx["pb"][deg])
    want = fx["g"]["bbox"][deg]
    assert pr.number_class(want).tolist() == [[1, 2, 1, 2]]                 # NaN, +inf, NaN, +inf
    assert np.array_equal(pr.number_class(got), pr.number_class(want))
    # NaN propagates through min / max whichever corner holds it
    b = np.array([[0.0, 1.5, 0.0, 2.0, 0.0, 0.0, 0.0]])                      # corners at x = -1, +1, z = 0: u = -inf, +inf
    got = pp.projection.box3d_to_bbox(b, fx["p2"][0])
    assert pr.number_class(got)[0, [0, 2]].tolist() == [3, 2]


def test_zeros_not_ones_quirk(pp, fx):
    """project_to_image appends zeros: the fourth column of P2 never enters."""
    reg = fx["reg"]
    base = pp.projection.box3d_to_bbox(fx["boxes"][reg], fx["pb"][reg])
    other = fx["pb"][reg].copy()
    other[:, :, 3] = [1234.5, -77.0, 3.25, 9.0]
    assert np.array_equal(pp.projection.box3d_to_bbox(fx["boxes"][reg], other), base)
    # ... and with ones it would: the fixture's matrices have a fourth column that shifts u by tx / z
    b, P = fx["boxes"][0], fx["p2"][0]
    centre = P[:3, :3] @ b[:3] + P[:3, 3]
    assert abs(centre[0] / centre[2] - (P[:3, :3] @ b[:3])[0] / b[2]) > 1e-3
    # one matrix for all boxes and one per box agree
    f0 = fx["frame"] == 0
    assert np.array_equal(pp.projection.box3d_to_bbox(fx["boxes"][f0], fx["p2"][0]), base[:f0.sum()])


def test_header_declares_the_projection_surface():
    with open(os.path.join(ROOT, "include", "pp_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+PP_ABI_VERSION\s+4\b", h)
    assert re.search(r"int\s+pp_set_projection\s*\(\s*pp_handle\s+h\s*,\s*const\s+double\s*\*\s*p2\s*,\s*int32_t\s+batch\s*\)", h)
    assert re.search(r"int\s+pp_get_projection\s*\(\s*pp_handle\s+h\s*,\s*int32_t\s*\*\s*on\s*\)", h)
    assert re.search(r"int\s+pp_get_bboxes\s*\(\s*pp_handle\s+h\s*,\s*double\s*\*\s*bbox\s*\)", h)
    assert re.search(r"int\s+pp_box3d_to_bbox\s*\(\s*int\s+device\s*,\s*const\s+double\s*\*\s*boxes_camera\s*,\s*const\s+int32_t\s*\*"
                     r"\s*box_counts\s*,\s*int32_t\s+frames\s*,\s*const\s+double\s*\*\s*p2\s*,\s*double\s*\*\s*bbox\s*\)", h)
    added = h[h.index("later additions within 4"):h.index("#define PP_ABI_VERSION")]
    for name in ("pp_set_projection", "pp_get_projection", "pp_get_bboxes", "pp_box3d_to_bbox"):
        assert name in added
    assert added.index("pp_rotate_nms") < added.index("pp_set_projection")        # appended, nothing before them changed


def test_binding_lists_the_symbols(pp):
    for name in ("pp_set_projection", "pp_get_projection", "pp_get_bboxes", "pp_box3d_to_bbox"):
        assert name in pp._lib.EXPORTS
    assert "box_project.hip" in pp._lib.SOURCES and "api_project.hip" in pp._lib.SOURCES
    assert "projection" in pp.__all__


def test_config_key(pp):
    cfg = pp.config.pedestrian_d435i_config(1)
    assert "project_bbox" not in cfg["model"]["second"]          # the reference's YAML does not have it
    d = pp.config.Derived(cfg)
    assert d.project_bbox is False and d.nms_dict()["project_bbox"] is False
    for v in (True, False):
        cfg2 = copy.deepcopy(cfg)
        cfg2["model"]["second"]["project_bbox"] = v
        d2 = pp.config.Derived(cfg2)
        assert d2.project_bbox is v and d2.nms_dict()["project_bbox"] is v
    assert pp.config.Derived(pp.config.kitti_shaped_config(num_class=2)).project_bbox is False


# one row per drop condition, one clipped row, one untouched row; image (height, width) = (370, 1224)
SHAPE = (370, 1224)
ROWS = np.array([[1225.0, 10.0, 1300.0, 50.0],     # x0 > w: dropped
                 [10.0, 371.0, 50.0, 400.0],       # y0 > h: dropped
                 [-50.0, 10.0, -1.0, 50.0],        # x1 < 0: dropped
                 [10.0, -50.0, 50.0, -0.5],        # y1 < 0: dropped
                 [-20.5, -3.0, 1300.0, 400.0],     # clipped on all four sides
                 [100.25, 120.5, 180.75, 300.0]])  # untouched
KEEP = [False, False, False, False, True, True]
CLIPPED = np.array([[0.0, 0.0, 1224.0, 370.0], [100.25, 120.5, 180.75, 300.0]])


def test_clip_bbox_to_image(pp):
    out, keep = pp.projection.clip_bbox_to_image(ROWS, SHAPE)
    assert keep.tolist() == KEEP and out.dtype == np.float64 and np.array_equal(out, CLIPPED)
    # on the border is inside (strict comparisons)
    edge = np.array([[1224.0, 370.0, 1300.0, 400.0], [-5.0, -5.0, 0.0, 0.0]])
    out, keep = pp.projection.clip_bbox_to_image(edge, SHAPE)
    assert keep.tolist() == [True, True]
    assert np.array_equal(out, [[1224.0, 370.0, 1224.0, 370.0], [0.0, 0.0, 0.0, 0.0]])
    out, keep = pp.projection.clip_bbox_to_image(np.zeros((0, 4)), SHAPE)
    assert out.shape == (0, 4) and keep.shape == (0,)


def _preds(n_frames=2):
    rng = np.random.default_rng(5)
    n = len(ROWS)
    out = []
    for b in range(n_frames):
        cam = np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(2, 9, (n, 1)), rng.uniform(0.5, 1.8, (n, 3)),
                              rng.uniform(-3, 3, (n, 1))], axis=1)
        lid = np.concatenate([rng.uniform(0.5, 9, (n, 1)), rng.uniform(-3, 3, (n, 2)), rng.uniform(0.5, 1.8, (n, 3)),
                              rng.uniform(-3, 3, (n, 1))], axis=1).astype(np.float32)
        out.append({"bbox": ROWS.copy(), "box3d_camera": cam, "box3d_lidar": lid,
                    "scores": rng.uniform(0.1, 0.9, n).astype(np.float32), "label_preds": np.zeros(n, np.int64), "batch_idx": 7 + b})
    out.append({"bbox": None, "box3d_camera": None, "box3d_lidar": None, "scores": None, "label_preds": None, "batch_idx": 99})
    return out


def test_predict_kitti_to_anno_clip_to_image(pp):
    preds = _preds()
    shapes = np.array([SHAPE, (200, 150), SHAPE])
    example = (None,) * 9 + (shapes,)
    plain = pp.anno.predict_kitti_to_anno(example, ["Pedestrian"], preds)
    off = pp.anno.predict_kitti_to_anno(example, ["Pedestrian"], preds, clip_to_image=False)
    assert [sorted(a) for a in plain] == [sorted(a) for a in off]
    for a, b in zip(plain, off):                                      # the default is the output without the keyword
        assert all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    assert np.array_equal(plain[0]["bbox"], ROWS)
    on = pp.anno.predict_kitti_to_anno(example, ["Pedestrian"], preds, clip_to_image=True)
    assert np.array_equal(on[0]["bbox"], CLIPPED)
    for k in ("score", "location", "dimensions", "rotation_y", "alpha", "name"):
        assert np.array_equal(on[0][k], plain[0][k][KEEP])
    assert on[0]["batch_idx"].tolist() == [7, 7]
    # the second frame's image is 200 x 150 (height x width): the row untouched above is clipped here
    assert np.array_equal(on[1]["bbox"], [[0.0, 0.0, 150.0, 200.0], [100.25, 120.5, 150.0, 200.0]])
    assert on[2]["bbox"].shape == (0, 4) and on[2]["name"].shape == (0,)
    # every row outside: the frame's anno is the empty one
    gone = [dict(preds[0], bbox=np.tile(ROWS[0], (len(ROWS), 1)))]
    assert pp.anno.predict_kitti_to_anno(example, ["Pedestrian"], gone, clip_to_image=True)[0]["name"].shape == (0,)


def test_argument_checks(pp):
    pj = pp.projection
    with pytest.raises(ValueError):
        pj.box3d_to_bbox(np.zeros((3, 6)), np.eye(4))
    with pytest.raises(ValueError):
        pj.box3d_to_bbox_gpu(np.zeros((3, 6)), [3], np.eye(4))
    with pytest.raises(ValueError):
        pj.box3d_to_bbox_gpu(np.zeros((3, 7)), [2], np.eye(4))
    with pytest.raises(ValueError):
        pj.box3d_to_bbox_gpu(np.zeros((3, 7)), [4, -1], np.eye(4))
    with pytest.raises(ValueError):
        pj.box3d_to_bbox_gpu(np.zeros((3, 7)), [1, 2], np.zeros((3, 4, 4)))
    assert pj.box3d_to_bbox(np.zeros((0, 7)), np.eye(4)).shape == (0, 4)
