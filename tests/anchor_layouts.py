"""The anchor layouts of tests/test_anchor_layouts_host.py, tests/test_gpu_anchor_layouts.py and
tools/gen_golden_anchor_layouts.py: tiny_config with another anchor generator (rotations, sizes), class count and
direction head, on the 20x16 grid or on an odd 9x7 one.  Test infrastructure only."""
import copy

import numpy as np

ROT3 = [0, 0.785, 1.57]
TWO_SIZES = [0.6, 0.8, 1.73, 0.6, 1.76, 1.73]
ODD_SIZE = [0.24, 0.32, 1.73]

# name: (rotations, sizes or None = the config's one size, num_class, use_direction_classifier, odd 9x7 grid,
#        anchors per location, anchors)
LAYOUTS = {
    "one": ([0], None, 1, True, False, 1, 320),
    "three": (ROT3, None, 1, True, False, 3, 960),
    "two-sizes": ([1.57], TWO_SIZES, 2, True, False, 2, 640),
    "three-2cls-nodir": (ROT3, None, 2, False, False, 3, 960),
    "three-odd": (ROT3, None, 1, True, True, 3, 189),
    "one-odd": ([0], None, 1, True, True, 1, 63),
}
NAMES = list(LAYOUTS)


def layout_config(pp, name, batch=2):
    """tiny_config(batch) edited into the named layout.  The odd grid is 9 x 7 cells of 0.08 m with every block at stride
    1 (range, anchor offsets and the pillar cap scaled to the grid) and a 3 x 4 cell anchor."""
    rot, sizes, ncls, use_dir, odd, _, _ = LAYOUTS[name]
    cfg = copy.deepcopy(pp.config.tiny_config(batch))
    s = cfg["model"]["second"]
    ag = s["target_assigner"]["anchor_generators"]["anchor_generator_stride"]
    ag["rotations"] = list(rot)
    if sizes is not None:
        ag["sizes"] = list(sizes)
    s["num_class"] = ncls
    s["use_direction_classifier"] = use_dir
    if ncls > 1:
        cfg["eval_input_reader"]["desired_objects"] = ["Pedestrian", "Cyclist"][:ncls]
    if odd:
        cfg["eval_input_reader"]["feature_map_size"] = [1, 7, 9]
        s["voxel_generator"].update(point_cloud_range=[0, -0.28, -3.0, 0.72, 0.28, 3.0], max_number_of_voxels=63)
        s["rpn"].update(layer_strides=[1, 1, 1], upsample_strides=[1, 1, 1])
        ag.update(offsets=[0.08, -0.28, -1.465], sizes=list(ODD_SIZE))
    return cfg


def layout_frames(d, seed, counts=(700, 400)):
    """Clouds in the low 40 % of x and 30 % of y of the range: the anchor mask comes out mixed."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(d.pc_range[:3]), np.array(d.pc_range[3:])
    top = lo + (hi - lo) * np.array([0.4, 0.3, 1.0])
    return [rng.uniform(lo, top, (n, 3)).astype(np.float32) for n in counts]
