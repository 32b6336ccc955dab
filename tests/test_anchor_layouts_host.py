"""Anchor layouts beyond the shipped two rotations of one size (anchors.build_anchors / build_anchor_cells, config.Derived),
bit for bit against the reference's own generate_anchors / rbbox2d_to_near_bbox / fused_get_anchors_area
(tests/golden/ref_anchor_layouts.npz, recorded by tools/gen_golden_anchor_layouts.py), and the layouts the 32-column
head row cannot hold, refused by name."""
import numpy as np
import pytest

import anchor_layouts as L
from conftest import load_golden
from oracle import ref_numpy as rn


@pytest.fixture(scope="module")
def gold():
    return load_golden("ref_anchor_layouts.npz")


@pytest.mark.parametrize("name", L.NAMES)
def test_anchors_and_cells_match_the_reference(pp, gold, name):
    rot, sizes, ncls, use_dir, odd, napl, A = L.LAYOUTS[name]
    d = pp.config.Derived(L.layout_config(pp, name))
    assert (d.nx, d.ny) == ((9, 7) if odd else (20, 16)) and (d.head_w, d.head_h) == (d.nx, d.ny)
    assert d.num_anchor_per_loc == napl and d.num_anchors == A and d.num_class == ncls
    assert d.use_direction_classifier == use_dir
    a = pp.anchors.build_anchors(d)
    want = gold[name + "/anchors"]
    assert a.dtype == want.dtype == np.float32 and a.shape == want.shape == (A, 7)
    assert np.array_equal(a, want), "anchors: values and (y, x, size, rotation) order"
    # what the table promises of each layout
    assert len(np.unique(a[:, 6])) == len(rot) and len(np.unique(a[:, 3:6], axis=0)) == (2 if sizes else 1)
    if len(rot) == 3:
        assert np.float32(0.785) in a[:, 6], "a rotation that is neither 0 nor pi/2"
    cells = pp.anchors.build_anchor_cells(a, d)
    assert cells.dtype == np.int32 and cells.shape == (A, 4) and cells.flags["C_CONTIGUOUS"]
    assert (cells[:, 0] <= cells[:, 2]).all() and (cells[:, 1] <= cells[:, 3]).all()
    assert cells.min() >= 0 and cells[:, 2].max() == d.nx - 1 and cells[:, 3].max() == d.ny - 1
    # the cells against the reference: its near boxes through the float64 floor / clamp of fused_get_anchors_area ...
    assert np.array_equal(rn.rbbox2d_to_near_bbox(a[:, [0, 1, 3, 4, 6]]), gold[name + "/bv"])
    assert np.array_equal(cells, rn.anchor_cells(gold[name + "/bv"], d.voxel_size, d.pc_range, d.grid))
    # ... and the areas the reference's own loop returned on three recorded pillar-count maps (integers: exact sums)
    for occ, area in zip(gold[name + "/occ"], gold[name + "/area"]):
        I = occ.astype(np.int64).cumsum(0).cumsum(1)
        got = I[cells[:, 3], cells[:, 2]] - I[cells[:, 3], cells[:, 0]] - I[cells[:, 1], cells[:, 2]] + I[cells[:, 1], cells[:, 0]]
        assert np.array_equal(got.astype(area.dtype), area)
    if 0.785 in rot:      # |limit_period(0.785)| < pi / 4: the 0.785 anchor keeps the footprint of the 0 one
        per_loc = cells.reshape(-1, napl, 4)
        assert np.array_equal(per_loc[:, 0], per_loc[:, 1]) and not np.array_equal(per_loc[:, 0], per_loc[:, 2])


def test_layout_grid_facts():
    """A % 16 and A % 4 as the GPU tests rely on them (k_loss_count's scalar path, the strided candidate scan)."""
    mods = {n: (v[6] % 16, v[6] % 4) for n, v in L.LAYOUTS.items()}
    assert mods == {"one": (0, 0), "three": (0, 0), "two-sizes": (0, 0), "three-2cls-nodir": (0, 0),
                    "three-odd": (13, 1), "one-odd": (15, 3)}


@pytest.mark.parametrize("rotations,num_class,use_dir,cols", [([0, 0.52, 1.05, 1.57], 1, True, 40),
                                                               ([0, 0.785, 1.57], 2, True, 33)])
def test_layouts_past_the_head_row_are_refused(pp, rotations, num_class, use_dir, cols):
    """4 anchors per location with a direction head (40 columns) and 3 with two classes and a direction head (33): Derived
    raises, naming the column count, before anything reaches the GPU."""
    cfg = L.layout_config(pp, "three")
    s = cfg["model"]["second"]
    s["target_assigner"]["anchor_generators"]["anchor_generator_stride"]["rotations"] = rotations
    s["num_class"], s["use_direction_classifier"] = num_class, use_dir
    with pytest.raises(NotImplementedError, match=f"{cols} head columns > 32"):
        pp.config.Derived(cfg)
    with pytest.raises(NotImplementedError, match=f"{cols} head columns > 32"):
        pp.Engine(cfg, max_batch=1)        # (Derived is built first: no library call is made)


def test_widest_accepted_rows(pp):
    """30 of 32 columns (3 x (7 + 1 + 2)) and 27 (3 x (7 + 2), class plane 6 wide) are accepted."""
    for name, cols in (("three", 30), ("three-2cls-nodir", 27), ("two-sizes", 22), ("one", 10)):
        d = pp.config.Derived(L.layout_config(pp, name))
        assert d.num_anchor_per_loc * (7 + d.num_class + (2 if d.use_direction_classifier else 0)) == cols
