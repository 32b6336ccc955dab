"""Golden vectors for the training-time augmentation (pp_amd.augment, csrc/augment.hip), produced by RUNNING the
reference's own noise_per_object_v3_, random_flip, global_rotation, global_scaling_v2, global_translate, limit_period,
np.random.shuffle and filter_gt_box_outside_range_by_center (load_data.py:2751-2866), seeded, on float32 points and
float64 boxes as the loader holds them (build container only, through ref_shim).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_augment.py   ->  tests/golden/ref_augment.npz

Every stage's output is recorded, and the selected try of every box (the return of noise_per_box / noise_per_box_v2_).
Points are drawn with margins: none lies within 1e-6 m of a box face.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ld, _ = ref_shim.load_reference()
import pp_amd  # noqa: E402

aug = pp_amd.augment
PC_RANGE = np.array([0, -2.56, -3.0, 6.40, 2.56, 3.0])

_selected = {}
_orig_v1, _orig_v2 = ld.noise_per_box, ld.noise_per_box_v2_


def _rec_v1(*a):
    r = _orig_v1(*a)
    _selected["sel"] = np.array(r)
    return r


def _rec_v2(*a):
    r = _orig_v2(*a)
    _selected["sel"] = np.array(r)
    return r


ld.noise_per_box, ld.noise_per_box_v2_ = _rec_v1, _rec_v2

SHIPPED = {}
QUIET = {"groundtruth_rotation_uniform_noise": [0.0, 0.0], "groundtruth_localization_noise_std": [0.0, 0.0, 0.0],
         "global_rotation_uniform_noise": [0.0, 0.0], "global_scaling_uniform_noise": [1.0, 1.0],
         "global_loc_noise_std": [0.0, 0.0, 0.0]}


def box(x, y, z=-0.6, w=0.6, l=0.8, h=1.7, r=0.0):
    return [x, y, z, w, l, h, r]


def cloud(rng, boxes, n_free, n_per_box):
    """Points around and inside the boxes, none within 1e-6 m of a face of any box."""
    pts = [np.stack([rng.uniform(0.2, 6.2, n_free), rng.uniform(-2.4, 2.4, n_free), rng.uniform(-1.5, 1.5, n_free)], 1)]
    for b in boxes:
        u = rng.uniform(-0.45, 0.45, (n_per_box, 3))
        c, s = np.cos(b[6]), np.sin(b[6])
        lx, ly = u[:, 0] * b[3], u[:, 1] * b[4]
        pts.append(np.stack([b[0] + lx * c - ly * s, b[1] + lx * s + ly * c, b[2] + (u[:, 2] + 0.5) * b[5]], 1))
    p = np.concatenate(pts, 0).astype(np.float32)
    if len(boxes):
        n, d = aug.box_planes(np.asarray(boxes, np.float64))
        sg = aug.face_sign(p.astype(np.float64), n, d)
        far = (np.abs(sg) / np.linalg.norm(n, axis=-1)[None]).min(axis=(1, 2)) > 1e-5
        p = p[far]
    return p


def run_case(seed, points, boxes, valid, cfg_dict):
    cfg = aug.AugmentConfig.from_input_reader(cfg_dict)
    full = dict(aug._DEFAULTS)
    full.update(cfg_dict)
    points = points.copy()
    gt = np.asarray(boxes, np.float64).reshape(-1, 7).copy()
    mask = np.asarray(valid, bool).copy()
    names = np.array(["Pedestrian"] * len(gt))
    # the box each point follows (stage 1): the first valid box whose original box contains it, by the reference's
    # own containment test
    owner = -np.ones(len(points), np.int64)
    if len(gt):
        corners = ld.center_to_corner_box3d(gt[:, :3], gt[:, 3:6], gt[:, 6], origin=[0.5, 0.5, 0], axis=2)
        inside = ld.points_in_convex_polygon_3d_jit(points[:, :3], ld.corner_to_surfaces_3d_jit(corners)) & mask[None]
        has = inside.any(1)
        owner[has] = inside[has].argmax(1)
    np.random.seed(seed)
    _selected.clear()
    out = {"in_points": points.copy(), "in_boxes": gt.copy(), "in_valid": mask.copy(),
           "cfg": np.array([*cfg.rot_noise, *cfg.loc_std, *cfg.grot_range, *cfg.global_rot, *cfg.scaling,
                            *cfg.global_loc_std, cfg.num_try]), "seed": np.array(seed), "owner": owner}
    ld.noise_per_object_v3_(gt, points, mask, rotation_perturb=full["groundtruth_rotation_uniform_noise"],
                            center_noise_std=full["groundtruth_localization_noise_std"],
                            global_random_rot_range=full["global_random_rotation_range_per_object"],
                            group_ids=None, num_try=cfg.num_try)
    out["selected"] = _selected.get("sel", np.zeros(0, np.int64))
    out["s1_points"], out["s1_boxes"] = points.copy(), gt.copy()
    gt, names = gt[mask], names[mask]
    cls = np.ones(len(gt), np.int32)
    gt, points = ld.random_flip(gt, points)
    out["s3_points"], out["s3_boxes"] = points.copy(), gt.copy()
    gt, points = ld.global_rotation(gt, points, rotation=full["global_rotation_uniform_noise"])
    out["s4_points"], out["s4_boxes"] = points.copy(), gt.copy()
    gt, points = ld.global_scaling_v2(gt, points, *full["global_scaling_uniform_noise"])
    out["s5_points"], out["s5_boxes"] = points.copy(), gt.copy()
    gt, points = ld.global_translate(gt, points, full["global_loc_noise_std"])
    out["s6_points"], out["s6_boxes"] = points.copy(), gt.copy()
    gt[:, 6] = ld.limit_period(gt[:, 6], offset=0.5, period=2 * np.pi)
    out["s7_boxes"] = gt.copy()
    np.random.shuffle(points)
    out["s8_points"] = points.copy()
    keep = ld.filter_gt_box_outside_range_by_center(gt, PC_RANGE[[0, 1, 3, 4]])
    out["keep"] = np.asarray(keep, bool)
    out["out_boxes"], out["out_classes"] = gt[keep], cls[keep]
    return out


def main():
    rng = np.random.default_rng(2024)
    cases = {}
    b = [box(1.5, -0.8, r=0.3), box(2.6, 0.4, r=-1.1), box(3.9, -1.2, r=2.0), box(4.7, 1.1), box(2.0, 1.6, r=0.7),
         box(5.4, -0.2, r=-2.5)]
    cases["shipped"] = (11, cloud(rng, b, 300, 40), b, [True] * 6, SHIPPED)
    cases["grot"] = (12, cloud(rng, b, 300, 40), b, [True] * 6, {"global_random_rotation_range_per_object": [-0.4, 0.4]})
    cases["invalid"] = (13, cloud(rng, b, 200, 40), b, [True, False, True, False, True, True], SHIPPED)
    crowd = [box(1.2 + 0.62 * i, -1.2 + 0.82 * j) for i in range(5) for j in range(3)]
    cases["crowded"] = (14, cloud(rng, crowd, 100, 10), crowd, [True] * len(crowd), SHIPPED)
    # the small boxes lie inside the large ones: their points are inside two boxes and follow the first of them
    ov = [box(2.0, 0.0, w=1.0, l=1.2), box(2.05, 0.05, w=0.3, l=0.3, r=0.5), box(4.55, -0.5, w=0.3, l=0.3, r=-0.4),
          box(4.5, -0.5, w=1.0, l=1.2, r=0.2)]
    cases["overlap_points"] = (15, cloud(rng, ov, 100, 60), ov, [True] * 4, SHIPPED)
    # standup boxes overlap, rotated boxes apart; a box inside another: neither collides under the executed rule
    pair = [box(2.0, 0.0, w=0.5, l=1.2, r=np.pi / 4), box(2.62, -0.62, w=0.5, l=1.2, r=np.pi / 4),
            box(4.5, 0.5, w=1.6, l=1.6), box(4.5, 0.5, w=0.4, l=0.4, r=0.3)]
    cases["standup_only"] = (16, cloud(rng, pair, 100, 30), pair, [True] * 4, QUIET)
    cases["empty"] = (17, cloud(rng, [], 150, 0), [], [], SHIPPED)
    edge = [box(6.35, 0.0), box(0.05, 2.5), box(3.0, 0.0)]
    cases["out_of_range"] = (18, cloud(rng, edge, 100, 30), edge, [True] * 3,
                             {"global_loc_noise_std": [0.3, 0.3, 0.1]})
    border = [box(0.0, 0.0), box(3.0, 0.0), box(6.4 - 0.0, 0.7)]
    cases["border"] = (19, cloud(rng, border, 100, 20), border, [True] * 3, QUIET)
    out = {}
    for name, (seed, pts, bx, valid, cfgd) in cases.items():
        r = run_case(seed, pts, bx, valid, cfgd)
        for k, v in r.items():
            out[f"{name}__{k}"] = np.asarray(v)
        print(name, "selected", r["selected"].tolist(), "keep", r["keep"].tolist(), "n", len(pts))
    assert (out["crowded__selected"] == -1).any(), "the crowded frame must leave some box without a try"
    assert (out["standup_only__selected"] == 0).all(), "standup-only overlaps must not collide"
    assert not out["out_of_range__keep"].all() and not out["border__keep"].all()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_augment.npz"), names=np.array(list(cases)), **out)


if __name__ == "__main__":
    main()
