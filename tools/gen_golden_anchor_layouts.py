"""Golden vectors for anchor layouts the shipped YAML does not use (one / three rotations, two sizes per location, a
rotation that is neither 0 nor pi/2, an odd 9 x 7 grid), produced by RUNNING the reference's own generate_anchors ->
create_anchors_3d_stride, rbbox2d_to_near_bbox and fused_get_anchors_area (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_anchor_layouts.py   ->  tests/golden/ref_anchor_layouts.npz

Per layout of tests/anchor_layouts.py: `<name>/anchors` [A, 7] float32 in the reference's flattened order, `<name>/bv`
[A, 4] its near (stand-up) boxes, `<name>/occ` three seeded pillar-count maps [3, ny, nx] float32 and `<name>/area`
[3, A] what fused_get_anchors_area returns on their integral images.  The reference has no function that returns an
anchor's corner cells; the areas pin them (counts of 0..3 in every cell: a corner off by one changes a sum).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_shim  # noqa: E402

ld, _ = ref_shim.load_reference()
import pp_amd as pp  # noqa: E402
import anchor_layouts  # noqa: E402

rng = np.random.default_rng(47)
out = {}
for name in anchor_layouts.NAMES:
    d = pp.config.Derived(anchor_layouts.layout_config(pp, name))
    a = ld.generate_anchors(d.feature_map_size, d.anchor_cfg)["anchors"].reshape([-1, 7])
    bv = ld.rbbox2d_to_near_bbox(a[:, [0, 1, 3, 4, 6]])
    occ = rng.integers(0, 4, (3, d.ny, d.nx)).astype(np.float32)
    area = np.stack([ld.fused_get_anchors_area(o.cumsum(0).cumsum(1), bv, d.voxel_size, d.pc_range, d.grid) for o in occ])
    out[name + "/anchors"], out[name + "/bv"], out[name + "/occ"], out[name + "/area"] = a, bv, occ, area
    print(name, a.shape, a.dtype, bv.dtype, area.dtype, "areas", float(area.min()), float(area.max()))
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_anchor_layouts.npz"), **out)
